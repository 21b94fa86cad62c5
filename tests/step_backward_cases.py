"""Seeded inputs of the per-entry tests of warp_backward_kernel and composite_backward_kernel
(tests/test_e_step_backward.py on the GPU, tests/test_step_backward_restatement.py on the CPU): the smallest sizes that still
reach each path of the two kernels.  Every builder returns plain fp32 numpy arrays."""
import itertools

import numpy as np

F32 = np.float32
G = 32


# ---- warp ---------------------------------------------------------------------------------------------------------------
def _rotations(rng, nb):
    """General rotations (QR of a Gaussian matrix, determinant +1): asymmetric, so R and its transpose differ."""
    out = np.empty((nb, 3, 3), F32)
    for b in range(nb):
        q, r = np.linalg.qr(rng.randn(3, 3))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out[b] = q
    return out


def signed_permutations(nb):
    """R[b][i, perms[b % 6][i]] = -1 if bit i of b is set else +1: 24 distinct matrices for b < 24, none symmetric in general."""
    perms = list(itertools.permutations(range(3)))
    R = np.zeros((nb, 3, 3), F32)
    for b in range(nb):
        for i in range(3):
            R[b, i, perms[b % 6][i]] = -1.0 if (b >> i) & 1 else 1.0
    return R


def _rays(rng, n, spread=1.2):
    o = rng.uniform(-spread, spread, (n, 3))
    d = rng.randn(n, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= rng.uniform(0.7, 1.4, (n, 1))
    near = rng.uniform(0.0, 0.5, (n, 1))
    far = near + rng.uniform(1.0, 2.5, (n, 1))
    return np.concatenate([o, d, near, far], 1).astype(F32)


def _warp_case(name, rays8, S, t_vals, t_rand, Rs, Ts, vol, g_mask, bmin=(-1.3, -1.1, -1.2), bscale=(0.77, 0.91, 0.83)):
    n = len(rays8)
    return {'name': name, 'rays8': np.ascontiguousarray(rays8, F32), 'S': S, 't_vals': np.asarray(t_vals, F32),
            't_rand': None if t_rand is None else np.ascontiguousarray(t_rand, F32), 'Rs': np.ascontiguousarray(Rs, F32),
            'Ts': np.ascontiguousarray(Ts, F32), 'vol': np.ascontiguousarray(vol, F32),
            'g_mask': np.ascontiguousarray(g_mask, F32).reshape(n * S), 'bmin': np.asarray(bmin, F32),
            'bscale': np.asarray(bscale, F32)}


def warp_dyadic():
    """n = 257, S = 64, nb = 24.  Origins and directions are multiples of 2^-6, near / far of 1/4, t = k / 64, Rs signed
    permutations, Ts multiples of 2^-5, box (-2, -1, -2) with scale (0.5, 1, 0.5): every grid coordinate is exact in fp32 and in
    float64 alike, so taps on a cell face do not move between the two."""
    rng = np.random.RandomState(11)
    n, S, nb = 257, 64, 24
    o = rng.randint(-96, 97, (n, 3)) / 64.0
    d = rng.randint(-64, 65, (n, 3)) / 64.0
    d[np.abs(d).sum(1) == 0] = 1.0 / 64.0
    near = rng.randint(0, 3, (n, 1)) / 4.0
    far = near + rng.randint(4, 11, (n, 1)) / 4.0
    o[:8] = np.round(o[:8])                                   # a few rays along grid lines: samples exactly on gi = 0 and gi = 31
    d[:8] = np.eye(3)[np.arange(8) % 3] * np.where(np.arange(8) % 2, -1.0, 1.0)[:, None]
    rays8 = np.concatenate([o, d, near, far], 1)
    Ts = rng.randint(-16, 17, (nb, 3)) / 32.0
    vol = rng.uniform(-1, 1, (nb + 1, G, G, G))
    g = rng.randn(n * S)
    return _warp_case('dyadic', rays8, S, np.arange(S) / S, None, signed_permutations(nb), Ts, vol, g,
                      bmin=(-2.0, -1.0, -2.0), bscale=(0.5, 1.0, 0.5))


def warp_random():
    """n = 300, S = 64, nb = 24: general rotations, jittered samples, ~10 % of the upstream gradient exactly zero, and one bone
    (17) moved out of every sample's reach: its whole gradient is exactly zero."""
    rng = np.random.RandomState(12)
    n, S, nb = 300, 64, 24
    Ts = rng.uniform(-0.4, 0.4, (nb, 3))
    Ts[17] = 100.0
    g = rng.randn(n * S)
    g[rng.rand(n * S) < 0.1] = 0.0
    return _warp_case('random', _rays(rng, n), S, np.linspace(0.0, 1.0, S, dtype=F32), rng.rand(n, S), _rotations(rng, nb), Ts,
                      rng.uniform(-1, 1, (nb + 1, G, G, G)), g)


def warp_capped():
    """n = 2 053, S = 128, nb = 2: 262 784 samples -> the slice count's cap of 16, 16 424 samples per slice (no multiple of S:
    every slice boundary falls inside a ray; 16 424 = 64 * 256 + 40: the last trip of the thread loop is ragged)."""
    rng = np.random.RandomState(13)
    n, S, nb = 2053, 128, 2
    return _warp_case('capped', _rays(rng, n), S, np.linspace(0.0, 1.0, S, dtype=F32), rng.rand(n, S), _rotations(rng, nb),
                      rng.uniform(-0.3, 0.3, (nb, 3)), rng.uniform(-1, 1, (nb + 1, G, G, G)), rng.randn(n * S))


def warp_bones(nb):
    """nb = 1 and nb = 32 (the ABI's limits), n = 64, S = 64; the volume has exactly nb channels: no background channel."""
    rng = np.random.RandomState(100 + nb)
    n, S = 64, 64
    return _warp_case(f'bones{nb}', _rays(rng, n), S, np.linspace(0.0, 1.0, S, dtype=F32), rng.rand(n, S), _rotations(rng, nb),
                      rng.uniform(-0.4, 0.4, (nb, 3)), rng.uniform(-1, 1, (nb, G, G, G)), rng.randn(n * S))


def warp_sparse():
    """200 samples (25 rays x 8): most voxels get no term, most touched voxels exactly one -- the bit-equal branch."""
    rng = np.random.RandomState(14)
    n, S, nb = 25, 8, 24
    return _warp_case('sparse', _rays(rng, n), S, np.linspace(0.0, 1.0, S, dtype=F32), None, _rotations(rng, nb),
                      rng.uniform(-0.4, 0.4, (nb, 3)), rng.uniform(-1, 1, (nb + 1, G, G, G)), rng.randn(n * S))


WARP_CASES = {'dyadic': warp_dyadic, 'random': warp_random, 'capped': warp_capped, 'bones1': lambda: warp_bones(1),
              'bones32': lambda: warp_bones(32), 'sparse': warp_sparse}


def warp_populations(c, ref):
    """What a case reaches, from the restatement's own floors (ref = warp_backward_numpy of the case): counts over the
    (sample, bone) pairs the kernel counts."""
    f = np.floor(ref['gi'])[ref['counted']]                                       # [pairs, 3]
    gi = ref['gi'][ref['counted']]
    inb = ((f >= -1) & (f <= G - 1)).all(1)                                       # at least one corner inside on every axis
    pairs = ref['counted'].size
    W = max(1, min(16, (len(c['g_mask']) + 16383) // 16384))
    per = -(-len(c['g_mask']) // W)
    return {'pairs': pairs, 'counted': int(ref['counted'].sum()), 'tap_in_bounds': int(inb.sum()),
            'floor_m1': [int((f[:, a] == -1).sum()) for a in range(3)], 'floor_31': [int((f[:, a] == G - 1).sum()) for a in range(3)],
            'floor_15': [int(((f[:, a] == 15) & inb).sum()) for a in range(3)],
            'on_0': int((gi == 0).any(1).sum()), 'on_31': int((gi == G - 1).any(1).sum()),
            'floor_32': int((f == G).any(1).sum()), 'single': int((ref['vol_n'] == 1).sum()), 'empty': int((ref['vol_n'] == 0).sum()),
            'slices': W, 'per': per, 'boundaries_inside_a_ray': sum(1 for k in range(1, W) if (k * per) % c['S'])}


def assert_warp_populations(c, ref):
    """The populations each case is there for; a case cannot silently stop covering them."""
    pop = warp_populations(c, ref)
    name = c['name']
    if name == 'dyadic':
        assert 0.3 * pop['pairs'] < pop['tap_in_bounds'] < 0.7 * pop['pairs'], pop
        assert min(pop['floor_m1']) >= 1000 and min(pop['floor_31']) >= 1000 and min(pop['floor_15']) >= 1000, pop
        assert pop['on_0'] >= 24 and pop['on_31'] >= 24 and pop['floor_32'] >= 1000, pop
    if name == 'random':
        assert min(pop['floor_m1']) >= 50 and min(pop['floor_31']) >= 50 and min(pop['floor_15']) >= 500, pop
        assert not ref['vol_n'][17].any() and ref['rt_n'][17] == 0, 'bone 17 is out of reach'
        assert 0.05 < float((c['g_mask'] == 0).mean()) < 0.15
    if name == 'capped':
        assert (pop['slices'], pop['per']) == (16, 16424) and pop['boundaries_inside_a_ray'] == 15, pop
        assert pop['tap_in_bounds'] > 100000, pop
    if name.startswith('bones'):
        assert c['vol'].shape[0] == c['Rs'].shape[0] and pop['slices'] == 1 and pop['tap_in_bounds'] > 500, pop
    if name == 'sparse':
        assert len(c['g_mask']) == 200 and pop['single'] >= 2000 and pop['empty'] > 0.95 * ref['vol_n'].size, pop
    if name != 'capped':
        assert pop['slices'] < 16, pop
    return pop


# ---- compositing --------------------------------------------------------------------------------------------------------
COMPOSITE_S = [1, 2, 63, 64, 65, 128, 129, 192, 256]
BACKGROUNDS = [(255.0, 128.0, 0.0), (0.0, 0.0, 0.0)]
KINDS = ['x=25', 'x=20', 'x=20+ulp', 'x=-30', 'mask=0', 'alpha=1', 'alpha>1', 'equal z', 'norm 1e-3', 'norm 1e3', 'zero gradient']


def _composite_random(rng, n, S, bg):
    raw = (rng.randn(n, S, 5) * 2).astype(F32)
    mask = rng.rand(n, S).astype(F32)
    z = np.sort(rng.rand(n, S) * 2 + 2, axis=1).astype(F32)
    rays8 = rng.randn(n, 8).astype(F32)
    return {'raw': raw, 'mask': mask, 'z': z, 'rays8': rays8, 'bg': np.asarray(bg, F32), 'g_rgb': rng.randn(n, 3).astype(F32),
            'g_acc': rng.randn(n).astype(F32), 'g_depth': rng.randn(n).astype(F32), 'groups': {'random': np.arange(n)}}


def composite_case(S, bg=BACKGROUNDS[0]):
    """41 rays of S samples: rays 0..11 are the special kinds of KINDS (ray 11 is a second zero-gradient ray), 12..40 random."""
    rng = np.random.RandomState(1000 + S)
    n = 41
    c = _composite_random(rng, n, S, bg)
    raw, mask, z, rays8 = c['raw'], c['mask'], c['z'], c['rays8']
    mid = (S - 1) // 2
    raw[0, :, 3] = 25.0                                        # softplus' linear branch
    raw[1, :, 3] = 20.0                                        # the switch point itself: still log1p(exp(x))
    raw[2, :, 3] = np.nextafter(F32(20.0), F32(np.inf))        # the first value of the linear branch
    raw[3, :, 3] = -30.0                                       # vanishing density: 1 - em cancels
    mask[4] = 0.0
    for r, m in ((5, 1.0), (6, 1.0 + 2.0 ** -20)):             # alpha = 1 exactly -> tt = 1e-10;  alpha > 1 -> tt < 0
        z[r] = np.linspace(2.0, 4.0, S) if S > 1 else 2.0
        rays8[r, 3:6] = (0.0, 0.0, 1.0)
        raw[r, mid, 3] = 1e5                                   # softplus * dist >= 1e5 * 2 / 255 > 200: em = 0 in fp32 and float64
        mask[r, mid] = m
    if S > 1:
        z[7, mid + 1] = z[7, mid]                              # dist = 0
    rays8[8, 3:6] *= F32(1e-3) / np.linalg.norm(rays8[8, 3:6])
    rays8[9, 3:6] *= F32(1e3) / np.linalg.norm(rays8[9, 3:6])
    for r in (10, 11):
        c['g_rgb'][r], c['g_acc'][r], c['g_depth'][r] = 0.0, 0.0, 0.0
    c['groups'] = {k: np.array([i]) for i, k in enumerate(KINDS)}
    c['groups']['zero gradient'] = np.array([10, 11])
    c['groups']['random'] = np.arange(12, n)
    assert float(mask[5, mid]) == 1.0 and float(mask[6, mid]) > 1.0
    assert S == 1 or (z[7, mid + 1] == z[7, mid] and (np.diff(z, axis=1) >= 0).all())
    return c


def composite_plain(n, S, seed):
    """Random rows only: the single ray, and the 32 768 + 5 rays that reach the second trip of the kernel's grid-stride loop
    (the launch caps at 8 192 blocks of 4 waves)."""
    return _composite_random(np.random.RandomState(seed), n, S, BACKGROUNDS[0])
