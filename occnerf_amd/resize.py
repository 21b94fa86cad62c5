"""Resizing a prepared frame to the training size (the reference's two cv2.resize lines, core/data/occnerf/train.py:306-314),
as a pure function of its inputs: DESIGN.md section 7g.

The reference blends the photograph over the background at full size in float64 (:296-297), resizes that float64 image
with INTER_LANCZOS4 and the mask / 255. with INTER_LINEAR.  `resize_blend` is that order, written out with one IEEE operation
per operator.  It is the host path of dataset.PreparedDataset(resize_frames=True, device=None) and what csrc/resize.hip
(ops.resize_frame) is held to bit for bit.  Equality with a particular OpenCV build in the last bit is NOT claimed, and at
exactly s = 1/2 OpenCV's INTER_LINEAR takes its 2 x 2 area mean, which is the bilinear value in exact arithmetic; bilinear is
what is built.

An H x W frame at scale s > 0 becomes h x w with h = rint(H s), w = rint(W s), ties to even.  Per axis, n_src -> n_dst, with
inv = 1.0 / s in float64 and for every destination index d

    f = float32((d + 0.5) * inv - 0.5)        i = floor(f)        t = float32(f - float32(i))

Lanczos: eight taps at i - 3 ... i + 4, each clamped to [0, n_src - 1].  With y0 = -(t + 3) * pi * 0.25 and
y_k = -(t + 3 - k) * pi * 0.25 in float64 (sin and cos are the C library's),

    c_k = float32((a_k sin y0 + b_k cos y0) / (y_k * y_k))
    (a_k, b_k) = (1, 0), (-r, -r), (0, 1), (r, -r), (-1, 0), (r, r), (0, -1), (-r, r)        r = 0.70710678118654752440
    sum = c_0 + c_1 + ... + c_7 in float32, left to right;   w_k = float32(c_k * float32(1 / sum))

and (0, 0, 0, 1, 0, 0, 0, 0) when t < FLT_EPSILON.  Bilinear: taps i and i + 1, clamped, weights float32(1 - t) and t.

Both passes are sums of float64(source) * float64(weight), left to right from 0.0: the horizontal one over every source
row, then the vertical one over its result.  The image's source is (m / 255.) * I + (1.0 - m / 255.) * bg per channel, NOT yet
divided by 255; the mask's is m / 255.  The Lanczos result leaves [0, 255] at edges and is carried through unclipped, as the
reference carries it.
"""
import math

import numpy as np

LANCZOS, BILINEAR = 'lanczos', 'bilinear'
TAPS = {LANCZOS: 8, BILINEAR: 2}
_R = 0.70710678118654752440
_CS = ((1.0, 0.0), (-_R, -_R), (0.0, 1.0), (_R, -_R), (-1.0, 0.0), (_R, _R), (0.0, -1.0), (-_R, _R))
_FLT_EPSILON = float(np.finfo(np.float32).eps)


def _scale(s):
    s = float(s)
    if not (s > 0.0 and math.isfinite(s)):
        raise ValueError(f'resize_img_scale={s!r}: the scale must be a positive number')
    return s


def resized_size(H, W, s):
    """(h, w) = (rint(H s), rint(W s)), ties to even: 41 -> 20 and 47 -> 24 at 0.5.  A side that comes out as 0 pixels is a
    ValueError."""
    s = _scale(s)
    h, w = int(np.rint(int(H) * s)), int(np.rint(int(W) * s))
    if int(H) < 1 or int(W) < 1 or h < 1 or w < 1:
        raise ValueError(f'resize_img_scale={s}: a {int(W)} x {int(H)} frame would become {w} x {h} pixels')
    return h, w


def lanczos_weights(t):
    """The eight float32 weights of the fraction t (a float32 in [0, 1))."""
    f32 = np.float32
    if float(t) < _FLT_EPSILON:
        return np.array([0, 0, 0, 1, 0, 0, 0, 0], dtype=f32)
    t = float(t)
    y0 = -(t + 3.0) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    c = np.empty(8, dtype=f32)
    for k in range(8):
        y = -(t + 3.0 - k) * math.pi * 0.25
        c[k] = f32((_CS[k][0] * s0 + _CS[k][1] * c0) / (y * y))
    total = f32(0.0)
    for k in range(8):
        total = f32(total + c[k])
    return (c * f32(f32(1.0) / total)).astype(f32)


def resize_tables(n_src, s, kind):
    """-> (offsets int32 [n_dst, taps], weights float32 [n_dst, taps]) of one axis: the clamped source index and the weight
    of every tap of every destination index; kind is LANCZOS (8 taps) or BILINEAR (2)."""
    if kind not in TAPS:
        raise ValueError(f'resize_tables: kind {kind!r} is neither {LANCZOS!r} nor {BILINEAR!r}')
    s, n_src = _scale(s), int(n_src)
    n_dst = resized_size(n_src, n_src, s)[0]
    inv = 1.0 / s
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * inv - 0.5).astype(np.float32)
    fl = np.floor(f)
    t = (f - fl).astype(np.float32)
    i = fl.astype(np.int64)
    if kind == BILINEAR:
        taps = i[:, None] + np.arange(2)[None, :]
        weights = np.stack([(np.float32(1.0) - t).astype(np.float32), t], 1)
    else:
        taps = i[:, None] + np.arange(-3, 5)[None, :]
        weights = np.stack([lanczos_weights(v) for v in t], 0) if n_dst else np.zeros((0, 8), np.float32)
    return np.clip(taps, 0, n_src - 1).astype(np.int32), np.ascontiguousarray(weights, dtype=np.float32)


def frame_tables(H, W, s):
    """The four tables of an H x W frame at scale s: {'size': (h, w), 'src_size': (H, W), 'x_lanczos', 'y_lanczos',
    'x_bilinear', 'y_bilinear': (offsets, weights)}.  x tables index columns (W -> w), y tables rows (H -> h)."""
    h, w = resized_size(H, W, s)
    out = {'size': (h, w), 'src_size': (int(H), int(W))}
    for kind in (LANCZOS, BILINEAR):
        out['x_' + kind] = resize_tables(W, s, kind)
        out['y_' + kind] = resize_tables(H, s, kind)
    return out


def _separable(src, x_table, y_table):
    """src float64 [H,W,C] -> [h,w,C]: the horizontal pass, then the vertical one, each a left-to-right sum from 0.0."""
    (xo, xw), (yo, yw) = x_table, y_table
    rows = np.zeros((src.shape[0], xo.shape[0], src.shape[2]), dtype=np.float64)
    for k in range(xo.shape[1]):
        rows = rows + src[:, xo[:, k], :] * xw[:, k].astype(np.float64)[None, :, None]
    out = np.zeros((yo.shape[0], xo.shape[0], src.shape[2]), dtype=np.float64)
    for k in range(yo.shape[1]):
        out = out + rows[yo[:, k]] * yw[:, k].astype(np.float64)[:, None, None]
    return out


def resize_blend(image_u8, mask_u8, bgcolor, s, tables=None):
    """image_u8 [H,W,3] uint8 or None, mask_u8 [H,W,3] uint8, bgcolor[3] in 0..255 (taken as float32, as the loaders carry
    it; unused without an image) -> (img64 [h,w,3] or None, alpha64 [h,w,3]), float64: the Lanczos resize of the full-size
    float64 blend (not divided by 255) and the bilinear resize of mask / 255.  tables: frame_tables(H, W, s), built here
    when None."""
    mask = np.asarray(mask_u8)
    if mask.dtype != np.uint8 or mask.ndim != 3 or mask.shape[2] != 3:
        raise ValueError(f'resize_blend: mask must be uint8 [H,W,3], got {mask.dtype} {mask.shape}')
    H, W = mask.shape[:2]
    if tables is None:
        tables = frame_tables(H, W, s)
    if tuple(tables['src_size']) != (H, W):
        raise ValueError(f"resize_blend: the tables are those of a {tables['src_size'][1]} x {tables['src_size'][0]} frame, "
                         f'the mask is {W} x {H}')
    alpha = mask / 255.
    alpha64 = _separable(alpha, tables['x_' + BILINEAR], tables['y_' + BILINEAR])
    if image_u8 is None:
        return None, alpha64
    image = np.asarray(image_u8)
    if image.dtype != np.uint8 or image.shape != mask.shape:
        raise ValueError(f'resize_blend: image must be uint8 {mask.shape} like the mask, got {image.dtype} {image.shape}')
    bg = np.asarray(bgcolor, dtype=np.float32).reshape(3)
    blend = alpha * image + (1.0 - alpha) * bg[None, None, :]
    return _separable(blend, tables['x_' + LANCZOS], tables['y_' + LANCZOS]), alpha64
