"""The definition of the geometry maps in numpy: what csrc/gbuffer.hip must equal byte for byte.

Everything is `dtype` arithmetic (float32: the definition; float64: the same definition at higher precision, the judge of the
float32 one's rounding in tests/test_gbuffer_restatement.py).  numpy rounds every array operation on its own and its
division and square root are correctly rounded, which is what the definition asks of the kernels.

  depth-valid   alpha >= min_alpha, alpha > 0, alpha and depth finite
  t             depth / alpha: the ray PARAMETER (the reference's depth; the metric distance is t |d|)
  P             o + t d (product, then sum)
  secants       horizontal a: right P(i,j+1) - P or left P - P(i,j-1); vertical b: down P(i+1,j) - P or up P - P(i-1,j); a
                candidate exists iff its neighbour is inside the image and depth-valid; of two the smaller |dt| wins and a tie
                goes to right / down
  n             a x b, flipped where (n_x d_x + n_y d_y) + n_z d_z > 0; invalid without both secants or with
                l2 = (n_x^2 + n_y^2) + n_z^2 zero or not finite; else n / sqrt(l2)
  shade         clamp01(-((n_x d_x + n_y d_y) + n_z d_z) / sqrt((d_x^2 + d_y^2) + d_z^2))
  panels        to_8b of: grey clamp01((t_hi - t) / (t_hi - t_lo)); 0.5 n + 0.5; grey shade; bg where not valid
"""
import numpy as np


def to_8b(x):
    """occnerf_amd.image.to_8b_image in float32."""
    return (np.float32(255.) * np.clip(np.asarray(x, dtype=np.float32), np.float32(0.), np.float32(1.))).astype(np.uint8)


def clamp01(x):
    """min(max(x, 0), 1), and 0 for NaN."""
    one, zero = x.dtype.type(1), x.dtype.type(0)
    return np.where(x > 0, np.where(x < 1, x, one), zero)


def default_t_range(near, far):
    return np.float32(np.asarray(near, np.float32).min()), np.float32(np.asarray(far, np.float32).max())


def _secant(P, t, v0, axis):
    """The secant along `axis` of the image (0: vertical, 1: horizontal) -> (secant [H,W,3], exists [H,W], took_backward)."""
    P, t, v0 = np.moveaxis(P, axis, 0), np.moveaxis(t, axis, 0), np.moveaxis(v0, axis, 0)
    dP, dt = P[1:] - P[:-1], t[1:] - t[:-1]                    # between a pixel and the next one
    pair = v0[1:] & v0[:-1]
    fwd, bwd = np.zeros_like(v0), np.zeros_like(v0)
    fwd[:-1], bwd[1:] = pair, pair
    sf, sb = np.zeros_like(P), np.zeros_like(P)
    sf[:-1], sb[1:] = dP, dP
    df, db = np.zeros_like(t), np.zeros_like(t)
    df[:-1], db[1:] = dt, dt
    use_b = bwd & (~fwd | (np.abs(db) < np.abs(df)))
    sec = np.where(use_b[..., None], sb, np.where(fwd[..., None], sf, P.dtype.type(0)))
    return np.moveaxis(sec, 0, axis), np.moveaxis(fwd | bwd, 0, axis), np.moveaxis(use_b, 0, axis)


def geometry_maps(H, W, ray_index, rays, depth, alpha, min_alpha=0.5, t_range=None, bg=(1., 1., 1.), dtype=np.float32):
    """ray_index int64 [R] ascending, rays [2,R,3], depth / alpha [R], t_range (t_lo, t_hi) or None (no depth panel).
    -> dict: t [H,W], points [H,W,4], normal [H,W,3], valid uint8 [H,W], shade [H,W], sec_a / sec_b [H,W,3], left / up [H,W]
    (the secant came from the backward neighbour) and the uint8 [H,W,3] panels depth_u8 (with t_range), normal_u8, shaded_u8."""
    f = np.dtype(dtype).type
    n = H * W
    ray_index = np.asarray(ray_index, dtype=np.int64).reshape(-1)
    R = ray_index.size
    assert R <= n and (R == 0 or (np.diff(ray_index) > 0).all() and 0 <= ray_index[0] and ray_index[-1] < n)
    rays = np.asarray(rays).reshape(2, R, 3).astype(dtype)
    dep, al = np.asarray(depth).reshape(R).astype(dtype), np.asarray(alpha).reshape(R).astype(dtype)
    bg8 = to_8b(np.asarray(bg, dtype=np.float32).reshape(3))
    with np.errstate(all='ignore'):
        ok = (al >= f(min_alpha)) & (al > 0) & np.isfinite(al) & np.isfinite(dep)
        t_r = np.where(ok, dep / np.where(ok, al, f(1)), f(0))
        P_r = np.where(ok[:, None], rays[0] + t_r[:, None] * rays[1], f(0))
        t, P, D, v0 = np.zeros(n, dtype), np.zeros((n, 3), dtype), np.zeros((n, 3), dtype), np.zeros(n, bool)
        t[ray_index], P[ray_index], D[ray_index], v0[ray_index] = t_r, P_r, rays[1], ok
        t, P, D, v0 = t.reshape(H, W), P.reshape(H, W, 3), D.reshape(H, W, 3), v0.reshape(H, W)
        a, has_a, left = _secant(P, t, v0, 1)
        b, has_b, up = _secant(P, t, v0, 0)
        nrm = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                        a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
        s = (nrm[..., 0] * D[..., 0] + nrm[..., 1] * D[..., 1]) + nrm[..., 2] * D[..., 2]
        nrm = np.where((s > 0)[..., None], -nrm, nrm)
        l2 = (nrm[..., 0] * nrm[..., 0] + nrm[..., 1] * nrm[..., 1]) + nrm[..., 2] * nrm[..., 2]
        nv = v0 & has_a & has_b & np.isfinite(l2) & (l2 != 0)
        nh = np.where(nv[..., None], nrm / np.sqrt(np.where(nv, l2, f(1)))[..., None], f(0))
        nd = (nh[..., 0] * D[..., 0] + nh[..., 1] * D[..., 1]) + nh[..., 2] * D[..., 2]
        dd = (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]
        shade = np.where(nv, clamp01(-nd / np.sqrt(dd)), f(0))
        out = {'t': t, 'points': np.concatenate([P, t[..., None]], -1), 'normal': nh,
               'valid': (v0.astype(np.uint8) | (nv.astype(np.uint8) << 1)).astype(np.uint8), 'shade': shade,
               'sec_a': a, 'sec_b': b, 'left': left, 'up': up}
        if t_range is not None:
            lo, hi = f(t_range[0]), f(t_range[1])
            grey = to_8b(clamp01((hi - t) / (hi - lo)))
            out['depth_u8'] = np.where(v0[..., None], grey[..., None], bg8)
        out['normal_u8'] = np.where(nv[..., None], to_8b(f(0.5) * nh + f(0.5)), bg8)
        out['shaded_u8'] = np.where(nv[..., None], to_8b(shade)[..., None], bg8)
    return out
