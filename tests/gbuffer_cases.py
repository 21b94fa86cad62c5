"""Frames for the geometry maps, shared by tests/test_gbuffer_restatement.py (the definition held
against what each case was built to show) and tests/test_r_gbuffer.py (the kernels held against the definition).

A hand case is a dict of geometry_maps' arguments: H, W, ray_index, rays, depth, alpha, min_alpha, t_range, bg.  Their rays
are `column` rays -- origin (j, i, 0), direction (0, 0, 1), so that P = (j, i, t) and every expectation can be read off the
depths -- unless the case says otherwise."""
import numpy as np

BG = (1.0, 0.5, 0.25)


def column_rays(H, W, pixels):
    pixels = np.asarray(pixels, dtype=np.int64)
    o = np.stack([pixels % W, pixels // W, np.zeros_like(pixels)], 1).astype(np.float32)
    d = np.tile(np.array([0., 0., 1.], np.float32), (pixels.size, 1))
    return np.stack([o, d], 0)


def _case(H, W, pixels, t, alpha=None, min_alpha=0.5, t_range=(0.0, 8.0), rays=None):
    pixels = np.asarray(pixels, dtype=np.int64).reshape(-1)
    alpha = np.ones(pixels.size, np.float32) if alpha is None else np.asarray(alpha, np.float32)
    depth = (np.asarray(t, np.float32).reshape(-1) * alpha).astype(np.float32)
    return {'H': H, 'W': W, 'ray_index': pixels, 'rays': column_rays(H, W, pixels) if rays is None else rays,
            'depth': depth, 'alpha': alpha, 'min_alpha': min_alpha, 't_range': t_range, 'bg': BG}


def hand_cases():
    c = {}
    ii, jj = np.meshgrid(np.arange(3), np.arange(3), indexing='ij')
    # R = H W; every border pixel has one neighbour per direction only.  The plane t = 1 + j / 2 + i / 4 (exact in float32)
    c['borders'] = _case(3, 3, np.arange(9), 1.0 + 0.5 * jj + 0.25 * ii)
    # only the middle row has rays: no vertical neighbour, so the depth is valid and the normal is not
    c['one_row'] = _case(3, 3, [3, 4, 5], [1.0, 1.5, 2.0])
    # the centre's four neighbours are all 1 away in t, with opposite slopes on the two sides: right and down take the tie
    c['tie'] = _case(3, 3, np.arange(9), [[3.0, 2.0, 3.0], [2.0, 1.0, 2.0], [3.0, 2.0, 3.0]])
    # a silhouette step between columns 1 and 2: each side takes its secant from its own side
    c['step'] = _case(3, 4, np.arange(12), [[1.0, 1.25, 5.0, 5.25], [1.0, 1.25, 5.0, 5.25], [1.5, 1.75, 5.5, 5.75]])
    # alpha just below the threshold (pixel 4) and exactly at it (pixel 5)
    below = np.nextafter(np.float32(0.5), np.float32(0.0))
    c['threshold'] = _case(3, 3, np.arange(9), np.full(9, 2.0), alpha=[1, 1, 1, 1, below, 0.5, 1, 1, 1])
    # alpha = 0 and a negative alpha under a threshold that would admit them
    c['zero_alpha'] = _case(3, 3, np.arange(9), np.full(9, 2.0), alpha=[1, 1, 1, 1, 0.0, -1.0, 1, 1, 1], min_alpha=-2.0)
    # a NaN depth (pixel 4), an infinite alpha (pixel 1), an infinite depth (pixel 7)
    nf = _case(3, 3, np.arange(9), np.full(9, 2.0))
    nf['depth'][4], nf['alpha'][1], nf['depth'][7] = np.nan, np.inf, -np.inf
    c['not_finite'] = nf
    # every ray is the same ray: all points lie on one line, the cross product is exactly zero
    same = np.stack([np.zeros((9, 3), np.float32), np.tile(np.array([0., 0., 1.], np.float32), (9, 1))], 0)
    c['degenerate'] = _case(3, 3, np.arange(9), 1.0 + 0.5 * jj + 0.25 * ii, rays=same)
    # no ray at all
    c['no_rays'] = _case(2, 3, [], [])
    # an empty depth range (t_hi = t_lo = t: the grey is 0 / 0) and a pixel behind t_hi, in front of t_lo
    c['empty_range'] = _case(3, 3, np.arange(9), np.full(9, 2.0), t_range=(2.0, 2.0))
    c['outside_range'] = _case(3, 3, np.arange(9), [[0.5, 9.0, 2.0]] * 3, t_range=(1.0, 8.0))
    return c


def random_frame(H, W, share, seed, exact=False):
    """A seeded frame with about `share` of the pixels carrying a ray (1.0: all): a jittered pinhole bundle, smooth depths with
    steps, alphas on both sides of the threshold with zeros, NaNs and infinities sprinkled in.  exact: depths and alphas on a
    coarse binary grid, so that |dt| ties between the two sides of a pixel happen."""
    rng = np.random.RandomState(seed)
    n = H * W
    pixels = np.arange(n) if share >= 1.0 else np.nonzero(rng.rand(n) < share)[0]
    R = pixels.size
    i, j = (pixels // W).astype(np.float32), (pixels % W).astype(np.float32)
    o = (np.array([0.1, -0.25, 6.0], np.float32) + 0.01 * rng.randn(R, 3)).astype(np.float32)
    d = np.stack([(j - W / 2) / 150.0, (i - H / 2) / 150.0, -np.ones(R)], 1).astype(np.float32)
    d = (d + 0.002 * rng.randn(R, 3)).astype(np.float32)
    if exact:
        t = np.round(4.0 + 2.0 * np.sin(i / 3.0) * np.cos(j / 4.0), 0) / 4.0 + 4.0
        alpha = rng.choice(np.array([0.25, 0.5, 1.0], np.float32), R)
    else:
        t = 5.0 + 0.8 * np.sin(i / 5.0 + 0.3) * np.cos(j / 7.0) + 2.0 * (rng.rand(R) < 0.05)
        alpha = rng.rand(R).astype(np.float32)
    alpha = alpha.astype(np.float32)
    depth = (t.astype(np.float32) * alpha).astype(np.float32)
    for value, target in ((0.0, alpha), (np.nan, depth), (np.inf, alpha), (np.nan, alpha), (-np.inf, depth)):
        target[rng.rand(R) < 0.01] = value
    return {'H': H, 'W': W, 'ray_index': pixels.astype(np.int64), 'rays': np.stack([o, d], 0), 'depth': depth, 'alpha': alpha,
            'min_alpha': 0.5 if exact else 0.3, 't_range': (3.5, 8.5), 'bg': BG,
            'near': np.full((R, 1), 3.75, np.float32) + rng.rand(R, 1).astype(np.float32),
            'far': np.full((R, 1), 7.5, np.float32) + rng.rand(R, 1).astype(np.float32)}


RANDOM_SIZES = ((29, 37), (64, 64), (70, 130))           # (H, W): 37 x 29, 64 x 64 and 130 x 70 pixels wide x high
RANDOM_SHARES = (0.1, 0.6, 1.0)


def random_cases():
    out = {}
    for s, (H, W) in enumerate(RANDOM_SIZES):
        for k, share in enumerate(RANDOM_SHARES):
            out[f'{W}x{H}_{int(share * 100)}'] = random_frame(H, W, share, seed=100 + 10 * s + k, exact=(s + k) % 2 == 1)
    return out


def definition_args(case):
    return {k: case[k] for k in ('H', 'W', 'ray_index', 'rays', 'depth', 'alpha', 'min_alpha', 't_range', 'bg')}
