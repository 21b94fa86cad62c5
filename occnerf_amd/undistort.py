"""Undistorting a uint8 photograph (the reference's two cv2.undistort lines, core/data/occnerf/train.py:290-294, and
allview.py:166-170), as a pure function of its inputs: DESIGN.md section 7f.

`undistort_u8` is OpenCV's algorithm where that is determinate -- undistort -> initUndistortRectifyMap into CV_16SC2 maps
(1/32-pixel fractions) -> remap, INTER_LINEAR, BORDER_CONSTANT 0, new camera matrix = K -- written out with one IEEE
operation per operator in a fixed order.  It is the host path of dataset.PreparedDataset(prepare_frames=True, device=None)
and of views.ViewFrames' host dicts, and what csrc/undistort.hip (ops.undistort_u8) is held to bit for bit.  Equality with a
particular OpenCV build is NOT claimed: builds differ among themselves in the last bit of the map (one accumulates along a
row, the SIMD ones fuse multiply-adds), and cv2 is not available to record one.

For output pixel (row i, column j), in float64:

    x = (j - cx) / fx            y = (i - cy) / fy
    x2 = x*x   y2 = y*y   r2 = x2 + y2   _2xy = 2*x*y
    kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2)
    xd = x*kr + p1*_2xy + p2*(r2 + 2*x2)
    yd = y*kr + p1*(r2 + 2*y2) + p2*_2xy
    u = fx*xd + cx               v = fy*yd + cy
    iu = rint(u*32)  iv = rint(v*32)         ties to even, saturated to int32; a non-finite u or v makes the pixel 0
    x0 = iu >> 5  a = iu & 31    y0 = iv >> 5  b = iv & 31
    acc = (32-b)*(32-a)*S(y0,x0) + (32-b)*a*S(y0,x0+1) + b*(32-a)*S(y0+1,x0) + b*a*S(y0+1,x0+1)
    out = (acc + 512) >> 10

S is the source channel, 0 outside the image, tested per tap.
"""
import numpy as np

_INT32_MIN, _INT32_MAX = -2147483648.0, 2147483647.0


def coefficients(D):
    """(k1, k2, p1, p2, k3, k4, k5, k6) as float64 [8] from 4, 5 or 8 coefficients shaped (n,), (n,1) or (1,n); missing ones
    are 0.  12 or 14 coefficients (OpenCV's thin prism and tilt models) are refused by name."""
    d = np.asarray(D, dtype=np.float64)
    if d.ndim > 2 or (d.ndim == 2 and 1 not in d.shape):
        raise ValueError(f'distortions: shape {d.shape} is none of (n,), (n,1), (1,n)')
    d = d.reshape(-1)
    if d.size == 12:
        raise NotImplementedError('distortions: 12 coefficients (the thin prism model s1..s4) are not built; 4, 5 or 8')
    if d.size == 14:
        raise NotImplementedError('distortions: 14 coefficients (the thin prism and tilt models) are not built; 4, 5 or 8')
    if d.size not in (4, 5, 8):
        raise ValueError(f'distortions: {d.size} coefficients; 4, 5 or 8 (k1, k2, p1, p2[, k3[, k4, k5, k6]])')
    out = np.zeros(8, dtype=np.float64)
    out[:d.size] = d
    return out


def camera(K):
    """K[:3,:3] as float64, as stored; a skewed camera is refused by name."""
    K = np.asarray(K, dtype=np.float64)
    if K.ndim != 2 or K.shape[0] < 3 or K.shape[1] < 3:
        raise ValueError(f'intrinsics: shape {K.shape}, not a 3 x 3 camera matrix')
    K = np.ascontiguousarray(K[:3, :3])
    if K[0, 1] != 0.0:
        raise NotImplementedError(f'intrinsics: skew K[0,1] = {K[0, 1]!r}; undistorting with a skewed camera is not built')
    return K


def check_window(window, H, W):
    """window (y0, x0, h, w) inside an H x W image, or None for all of it -> four ints."""
    if window is None:
        return 0, 0, int(H), int(W)
    y0, x0, h, w = (int(v) for v in window)
    if h <= 0 or w <= 0 or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError(f'window (y0, x0, h, w) = {(y0, x0, h, w)} is not inside the {W} x {H} image')
    return y0, x0, h, w


def source_coordinates(H, W, K, D, window=None):
    """The unquantised float64 (u, v) of every output pixel of the window, [h,w] each: where in the distorted photograph
    the pixel is read."""
    K, d = camera(K), coefficients(D)
    y0, x0, h, w = check_window(window, H, W)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    with np.errstate(all='ignore'):
        x = (np.arange(x0, x0 + w, dtype=np.float64)[None, :] - cx) / fx
        y = (np.arange(y0, y0 + h, dtype=np.float64)[:, None] - cy) / fy
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        _2xy = 2 * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
        yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
        u = fx * xd + cx
        v = fy * yd + cy
    return u, v


def undistort_u8(img, K, D, window=None):
    """img uint8 [H,W,3] (any channel count), K 3x3 as stored, D 4 / 5 / 8 coefficients -> the undistorted image, uint8 of
    the same shape, or with window=(y0, x0, h, w) only that window of it ([h,w,C]); the map is that of the full image."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError(f'undistort_u8: img must be uint8 [H,W,C], got {img.dtype} {img.shape}')
    H, W = img.shape[:2]
    u, v = source_coordinates(H, W, K, D, window)
    ok = np.isfinite(u) & np.isfinite(v)
    with np.errstate(all='ignore'):
        iu = np.clip(np.rint(np.where(ok, u, 0.0) * 32), _INT32_MIN, _INT32_MAX).astype(np.int64)
        iv = np.clip(np.rint(np.where(ok, v, 0.0) * 32), _INT32_MIN, _INT32_MAX).astype(np.int64)
    x0, a = iu >> 5, (iu & 31)[..., None]
    y0, b = iv >> 5, (iv & 31)[..., None]
    src = np.zeros((H + 2, W + 2, img.shape[2]), dtype=np.int64)          # a zero border: a tap outside the image reads 0
    src[1:-1, 1:-1] = img
    xa, xb = np.clip(x0, -1, W) + 1, np.clip(x0 + 1, -1, W) + 1
    ya, yb = np.clip(y0, -1, H) + 1, np.clip(y0 + 1, -1, H) + 1
    acc = (32 - b) * (32 - a) * src[ya, xa] + (32 - b) * a * src[ya, xb] + b * (32 - a) * src[yb, xa] + b * a * src[yb, xb]
    out = ((acc + 512) >> 10).astype(np.uint8)
    out[~ok] = 0
    return out
