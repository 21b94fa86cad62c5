"""Seeded inputs of the per-entry tests of the once-per-step kernels (tests/test_q_step_preamble_per_entry.py on the GPU,
tests/test_step_preamble_restatement.py on the CPU).  Every builder returns float64 numpy arrays whose values are exact in
fp32 (fp64 operands and integer ids apart) and asserts the condition its case is there for."""
import numpy as np
import torch

from tests import step_preamble_restatement as sp
from tests.step_backward_cases import signed_permutations

F32 = np.float32
FILL = -777.0


def _x(a):
    """Round to fp32, keep as float64."""
    return np.asarray(a, np.float64).astype(F32).astype(np.float64)


# ---- pose chain -----------------------------------------------------------------------------------------------------------
REGIMES = ('reference init', 'default init', 'zero rows')
ZERO_BONE = 7                                                 # 'zero rows': rows 3 (b - 1) .. + 2 of the last layer, rvec of bone b = 0
# seeds whose smallest ReLU margin is >= 4 (K + 2) u A (seeds 0..11 give 0.3 to 93; `assert_pose_case` asserts it)
POSE_SEEDS = {'reference init': 1, 'default init': 0, 'zero rows': 3}
PATH_BONES = (15, 22, 23)


def _rodrigues64(r):
    th = np.linalg.norm(r, axis=1)[:, None, None]
    k = r / th[:, :, 0]
    K = np.zeros((len(r), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3)[None] + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def _skeleton(rng):
    dst_Rs = _x(_rodrigues64(rng.randn(24, 3) * 0.6))
    dst_Ts = _x(rng.randn(24, 3) * 0.2)
    cnl = np.zeros((24, 4, 4))
    cnl[:, :3, :3] = _rodrigues64(rng.randn(24, 3) * 0.8)
    cnl[:, :3, 3] = rng.randn(24, 3) * 0.3
    cnl[:, 3, 3] = 1.0
    return dst_Rs, dst_Ts, _x(cnl)


def pose_case(regime, seed=None):
    """The refiner in one of the three regimes of its last layer, a random skeleton and pose vector."""
    committed = seed is None
    seed = POSE_SEEDS[regime] if committed else seed
    from occnerf_amd.modules import BodyPoseRefiner
    gen = torch.Generator().manual_seed(1000 + seed)
    rng = np.random.RandomState(2000 + seed)
    dec = BodyPoseRefiner()
    lin = [m for m in dec.block_mlps if isinstance(m, torch.nn.Linear)]
    W, b = [], []
    for m in lin:                                              # nn.Linear's default: U(+-1 / sqrt(fan_in)) for both
        k = 1.0 / np.sqrt(m.in_features)
        W.append(((torch.rand(m.weight.shape, generator=gen) * 2 - 1) * k).double().numpy())
        b.append(((torch.rand(m.bias.shape, generator=gen) * 2 - 1) * k).double().numpy())
    if regime == 'reference init':                             # mlp_delta_body_pose.py: uniform +-1e-5, bias 0
        W[4] = rng.uniform(-1e-5, 1e-5, W[4].shape)
        b[4] = np.zeros_like(b[4])
    elif regime == 'zero rows':
        rows = slice(3 * (ZERO_BONE - 1), 3 * ZERO_BONE)
        W[4][rows], b[4][rows] = 0.0, 0.0
    else:
        assert regime == 'default init'
    dst_Rs, dst_Ts, cnl = _skeleton(rng)
    c = {'name': regime, 'W': [_x(w) for w in W], 'b': [_x(x) for x in b], 'posevec': _x(rng.uniform(-0.6, 0.6, 69)),
         'dst_Rs': dst_Rs, 'dst_Ts': dst_Ts, 'cnl_gtfms': cnl, 'dRs': _x(rng.randn(24, 3, 3)), 'dTs': _x(rng.randn(24, 3))}
    if committed:                                              # (another seed: the caller is looking for one that holds it)
        assert_pose_case(c)
    return c


def assert_pose_case(c):
    """Every hidden pre-activation is at least 4 (K + 2) u A away from 0; the regime is what it says."""
    margin = sp.relu_margin(c)
    assert margin >= 4.0, (c['name'], margin)
    if c['name'] == 'zero rows':
        rows = slice(3 * (ZERO_BONE - 1), 3 * ZERO_BONE)
        assert not c['W'][4][rows].any() and not c['b'][4][rows].any()
    if c['name'] == 'reference init':
        assert np.abs(c['W'][4]).max() <= 1e-5 and not c['b'][4].any()
    return margin


def pose_exact_case():
    """refine = 0 on dyadic operands: every product, the determinant (+-1) and its reciprocal are exact."""
    rng = np.random.RandomState(31)
    P = signed_permutations(48).astype(np.float64)
    cnl = np.zeros((24, 4, 4))
    cnl[:, :3, :3] = P[24:][::-1]
    cnl[:, :3, 3] = rng.randint(-255, 256, (24, 3)) / 64.0
    cnl[:, 3, 3] = 1.0
    c = {'name': 'exact', 'dst_Rs': P[:24], 'dst_Ts': rng.randint(-255, 256, (24, 3)) / 64.0, 'cnl_gtfms': cnl,
         'posevec': np.zeros(69), 'W': None, 'b': None}
    assert len({P[i].tobytes() for i in range(24)}) == 24, 'a different matrix per bone'
    assert np.all(np.abs(np.linalg.det(P)).round() == 1) and np.all(c['dst_Ts'] * 64 == np.round(c['dst_Ts'] * 64))
    assert np.abs(c['dst_Ts']).max() < 4 and np.abs(cnl[:, :3, 3]).max() < 4
    return c


def pose_random_case():
    """refine = 0: rodrigues rotations rounded to fp32, translations about 0.2."""
    dst_Rs, dst_Ts, cnl = _skeleton(np.random.RandomState(32))
    return {'name': 'random', 'dst_Rs': dst_Rs, 'dst_Ts': dst_Ts, 'cnl_gtfms': cnl, 'posevec': np.zeros(69), 'W': None, 'b': None}


def one_bone_cotangent(c, bone):
    dRs, dTs = np.zeros((24, 3, 3)), np.zeros((24, 3))
    dRs[bone], dTs[bone] = c['dRs'][bone], c['dTs'][bone]
    return dRs, dTs


# ---- prior softmax --------------------------------------------------------------------------------------------------------
PRIOR_C = (1, 2, 25, 32)
PRIOR_V = (1, 255, 256, 257, 1000)


def prior_case(C, V):
    rng = np.random.RandomState(3000 + 1009 * C + V)
    dec = rng.uniform(-30.0, 30.0, (C, V))
    kind = rng.randint(0 if C > 1 else 1, 4, (C, V))
    prior = np.choose(kind, [np.zeros((C, V)), np.full((C, V), 1e-30), 1.0 - rng.rand(C, V), np.ones((C, V))])
    dead = ~(prior > 0).any(0)
    prior[rng.randint(0, C, V)[dead], np.flatnonzero(dead)] = 0.5
    if C > 1:                                                  # one voxel deep in the underflow range: only the max subtraction saves it
        prior[:, 0] = 1e-30
        dec[:, 0] = rng.uniform(-30.0, -29.0, C)
    dec, prior = _x(dec), _x(prior)
    assert (prior > 0).any(0).all() and np.abs(dec).max() <= 30.0
    if C * V >= 64:
        assert all((prior == v).any() for v in ((0.0,) if C > 1 else ()) + (float(F32(1e-30)), 1.0)), 'every kind of prior'
    return dec, prior


# ---- ConvTranspose3d ------------------------------------------------------------------------------------------------------
CONVT_SHAPES = ((1, 1, 1, 1), (3, 1, 2, 3), (2, 3, 1, 2), (5, 2, 3, 1), (2, 5, 3, 7), (25, 4, 4, 4))


def convt_case(shape, dyadic=False):
    Cout, D, H, W = shape
    rng = np.random.RandomState(4000 + Cout * 1000 + D * 100 + H * 10 + W)
    V = D * H * W

    def draw(*s):
        return rng.randint(-64, 65, s) / 64.0 if dyadic else _x(rng.randn(*s))
    c = {'cols': draw(Cout * 64, V), 'bias': draw(Cout), 'gy': draw(Cout, 2 * D, 2 * H, 2 * W)}
    # col2im's total is no multiple of its 256-thread block but on the decoder's own cube (im2col's, 64 Cout V, is one
    # whenever Cout V is a multiple of 4: (2,3,1,2) and the cube)
    assert shape == (25, 4, 4, 4) or (Cout * 8 * V) % 256, 'a ragged last block'
    return c


# ---- agg_weights ----------------------------------------------------------------------------------------------------------
AGG_K = (2, 3, 10, 39, 40)
AGG_N = (1, 255, 256, 257, 600)
AGG_P = 97


def agg_case(N, K):
    """-> counter [P] (1 + Poisson(20), two entries 1, two 1e6), knn [N, K] int32: random rows, the last row all ids equal, the
    one before it ids 0 and P - 1."""
    rng = np.random.RandomState(5000 + 41 * N + K)
    counter = 1.0 + rng.poisson(20.0, AGG_P)
    counter[[3, 50]] = 1.0
    counter[[10, 60]] = 1e6
    counter[0], counter[AGG_P - 1] = 7.0, 1e6
    knn = rng.randint(0, AGG_P, (N, K)).astype(np.int32)
    knn[N - 1] = 7
    if N >= 2:
        knn[N - 2] = np.where(np.arange(K) % 2, AGG_P - 1, 0)
    assert (counter == 1).sum() >= 2 and (counter == 1e6).sum() >= 2
    return _x(counter), knn


# ---- per-point SDF backward -----------------------------------------------------------------------------------------------
SDF_P = (1, 63, 64, 65, 257)


def sdf_case(P):
    """-> dict base [M,3] (M = max(P, 8): the 3-NN search needs three support points), point_dist [P,1], normals [M,3] fp64,
    d_kb [P,3] fp64, d_dist [P].  Every fourth row has point_dist = 0."""
    rng = np.random.RandomState(6000 + P)
    M = max(P, 8)
    base = _x(rng.rand(M, 3))
    dist = _x(rng.choice([-1.0, 1.0], (P, 1)) * rng.uniform(0.01, 0.03, (P, 1)))
    if P > 1:
        dist[::4] = 0.0
    normals = rng.randn(M, 3) * rng.uniform(0.5, 2.0, (M, 1))
    return {'base': base, 'point_dist': dist, 'normals': normals, 'd_kb': rng.randn(P, 3), 'd_dist': _x(rng.randn(P))}


def assert_sdf_case(c, kidx, unit):
    """|dot| >= 64 u sum |dir_k n_k| for every neighbour (the fp32 sign is not in question), and the populations."""
    P = len(c['point_dist'])
    pc = (c['base'][:P].astype(F32) + c['point_dist'].astype(F32)).astype(F32)
    dot, size = sp.sdf_dots32(pc, c['base'], c['normals'], kidx)
    assert np.all(np.abs(dot.astype(np.float64)) >= 64.0 * sp.U32 * size), 'an inside test within rounding of 0'
    dir_ = pc[:, None, :] - c['base'].astype(F32)[kidx]
    zero = ~dir_.any(-1)
    neg = (dot < 0).sum(1) > 1
    cj = (dir_.astype(np.float64) * np.asarray(unit)[kidx]).sum(-1)
    if P >= 63:
        assert zero[::4, 0].all() and not zero[:, 1:].any() and zero.sum() == len(zero[::4])
        assert neg.sum() >= 8 and (~neg).sum() >= 8 and (cj > 0).sum() >= 8 and (cj < 0).sum() >= 8
    return pc


# ---- Adam -----------------------------------------------------------------------------------------------------------------
def adam_sizes():
    from occnerf_amd.optim import CHUNK
    return (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 5)


def adam_case(n):
    """p, g, m, v [n]: entry 0 has g = 0 and v = 0; |g| log-uniform in 1e-12 .. 1e4 (up to 1e-4 for n <= 5: a norm below every
    max_grad_norm but 1e-3); every fifth entry has g = -9 m (1 + 2^-12), where m + (g - m)(1 - beta1) cancels."""
    rng = np.random.RandomState(7000 + n % 1000)
    hi = -4.0 if n <= 5 else 4.0
    g = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-12.0, hi, n)
    m = rng.randn(n) * 10.0 ** rng.uniform(-6.0, 1.0, n)
    v = 10.0 ** rng.uniform(-20.0, 2.0, n)
    v[rng.rand(n) < 0.1] = 0.0
    g[0], v[0] = 0.0, 0.0
    m[2::5] = -g[2::5] / 9.0 * (1.0 + 2.0 ** -12)
    if n > 5:
        g[1], g[3] = 1e-12, -1e4
    return {'p': _x(rng.randn(n)), 'g': _x(g), 'm': _x(m), 'v': _x(v)}


# ---- pack_rays ------------------------------------------------------------------------------------------------------------
PACK_R = (1, 255, 256, 257)


def pack_case(R):
    rng = np.random.RandomState(8000 + R)
    return {'rays': _x(rng.randn(2, R, 3)), 'near': _x(rng.rand(R, 1)), 'far': _x(rng.rand(R, 1) + 2.0), 'order': rng.permutation(R).astype(np.int64)}
