"""The cases of the resize tests (tests/test_resize_restatement.py on the CPU, tests/test_m_resize.py on the GPU) and an
independent restatement of DESIGN.md section 7g: a direct loop over the output pixels, straight from the formulas, that
shares no table and no helper with occnerf_amd/resize.py."""
import importlib.util
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W, scale): even sizes, odd sizes with rint ties (41 -> 20, 47 -> 24), scales that are no reciprocal of an integer, a
# frame wider than several tiles of the kernel and lower than its taps, and the smallest frame that survives 0.5
CASES = {'40x48@0.5': (40, 48, 0.5), '41x47@0.5': (41, 47, 0.5), '40x48@0.75': (40, 48, 0.75), '41x47@0.3': (41, 47, 0.3),
         '9x300@0.5': (9, 300, 0.5), '2x2@0.5': (2, 2, 0.5)}
SIZES = {'40x48@0.5': (20, 24), '41x47@0.5': (20, 24), '40x48@0.75': (30, 36), '41x47@0.3': (12, 14), '9x300@0.5': (4, 150),
         '2x2@0.5': (1, 1)}
BGCOLORS = {'black': [0., 0., 0.], 'fractional': [12.25, 200.7, 99.33]}

# the dataset of the consumer tests: 96 x 80 at 0.5 -> 48 x 40, patch.size 16; the band of frame 0 swallows its mask
DATASET = dict(frames=3, width=96, height=80, seed=23, focal=900.0)
BAND = {'range': 1, 'mid': 48, 'width': 96}


def load_tool():
    spec = importlib.util.spec_from_file_location('make_synthetic_dataset', os.path.join(ROOT, 'tools', 'make_synthetic_dataset.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def random_frame(name):
    """(image, mask) uint8 [H,W,3] of random bytes, seeded by the case: not smooth, so every weight meets every value."""
    H, W, _ = CASES[name]
    rng = np.random.RandomState(sorted(CASES).index(name) + 100)
    return rng.randint(0, 256, (H, W, 3)).astype(np.uint8), rng.randint(0, 256, (H, W, 3)).astype(np.uint8)


# ---------------------------------------------------------------- the restatement
_CS = [(1, 0), (-1, -1), (0, 1), (1, -1), (-1, 0), (1, 1), (0, -1), (-1, 1)]      # times sqrt(1/2) where both are set


def position(d, s):
    """(i, t) of destination index d."""
    inv = 1.0 / s
    f = np.float32((d + 0.5) * inv - 0.5)
    i = int(math.floor(float(f)))
    return i, np.float32(f - np.float32(i))


def lanczos(t):
    if float(t) < float(np.finfo(np.float32).eps):
        return [np.float32(v) for v in (0, 0, 0, 1, 0, 0, 0, 0)]
    r = 0.70710678118654752440
    x = float(t)
    y0 = -(x + 3) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    c, total = [], np.float32(0)
    for k in range(8):
        a, b = _CS[k]
        a, b = (a * r, b * r) if a and b else (float(a), float(b))
        y = -(x + 3 - k) * math.pi * 0.25
        c.append(np.float32((a * s0 + b * c0) / (y * y)))
        total = np.float32(total + c[-1])
    scale = np.float32(np.float32(1) / total)
    return [np.float32(v * scale) for v in c]


def taps(d, s, n_src, kind):
    """[(clamped source index, float32 weight)] of destination index d."""
    i, t = position(d, s)
    if kind == 'bilinear':
        pairs = [(i, np.float32(np.float32(1) - t)), (i + 1, t)]
    else:
        pairs = [(i - 3 + k, w) for k, w in enumerate(lanczos(t))]
    return [(min(max(j, 0), n_src - 1), w) for j, w in pairs]


def restate(image, mask, bgcolor, s):
    """-> (img64 or None, alpha64): every output pixel by its own double loop over the taps."""
    H, W = mask.shape[:2]
    h, w = int(np.rint(H * s)), int(np.rint(W * s))
    assert h >= 1 and w >= 1
    a = mask / 255.
    sources = [('bilinear', a)]
    if image is not None:
        bg = np.array(bgcolor, dtype='float32')
        sources.append(('lanczos', a * image + (1.0 - a) * bg[None, None, :]))
    out = []
    for kind, src in sources:
        res = np.zeros((h, w, 3))
        ys = [taps(r, s, H, kind) for r in range(h)]
        xs = [taps(c, s, W, kind) for c in range(w)]
        for r in range(h):
            for c in range(w):
                col = np.zeros(3)
                for y, wy in ys[r]:
                    row = np.zeros(3)
                    for x, wx in xs[c]:
                        row = row + src[y, x] * float(wx)
                    col = col + row * float(wy)
                res[r, c] = col
        out.append(res)
    return (out[1] if image is not None else None), out[0]


def closed_form(t):
    """The normalised sinc(u) sinc(u / 4) at u = t - (k - 3), k = 0..7, in float64 (np.sinc(x) = sin(pi x) / (pi x))."""
    u = float(t) - (np.arange(8) - 3)
    v = np.sinc(u) * np.sinc(u / 4)
    return v / v.sum()


# ---------------------------------------------------------------- the consumer rules on a resized frame, in numpy
def consumer_frame(ds, i, bgcolor, resized):
    """What reads a resized frame: the whole-frame dict of frame i of `ds` (a PreparedDataset
    opened with resize_frames) from `resized` = (img64, alpha64), by the host helpers the uint8 path is tested with."""
    from occnerf_amd.dataset import host_frame
    img64, alpha64 = resized
    f = ds.frames[i]
    bg = np.array(bgcolor, dtype='float32')
    out = host_frame(f['frame_name'], ds.height, ds.width, f['K'], f['E'], f['dst_bbox_min'], f['dst_bbox_max'], bg)
    img = (img64 / 255.).astype('float32')
    out.update(target_rgbs=img.reshape(-1, 3)[out['ray_mask']], ray_alpha=alpha64.reshape(-1, 3)[out['ray_mask']],
               _img=img, _alpha=alpha64)
    return out
