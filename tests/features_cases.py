"""Seeded, small inputs of the render-path feature kernels (occnerf_amd/csrc/features.hip) for
tests/test_features_restatement.py (CPU) and tests/test_v_features_per_entry.py (GPU).  Nothing here can fault: every id, row and
sentinel is a valid index, every denominator positive, no NaN.

model(P)      P points in [-0.35, 0.35]^3 under bound 0.4 (so pn = (p + 0.4) / 0.8 lies in [0.06, 0.94]), the last six at 0.42..0.5
              -- outside the bound: a sample whose neighbours 0..2 are among them has x[0..2] > 1; fp64 normals of any length
              (point 0: an axis-aligned one, for a dot product of exactly 0), unit normals, integer counts 0..6, and the inputs
              of point_table (knn_base beyond the bound and exactly on it, sdf over both clamps).  P = 257 takes its table from
              the restated point_table (the GPU test shows ops.point_table to give the same bits and uses that); P = 9216 and
              9217, the fit limit of the LDS image, take random floats.
layout()      offsets as GridEncoder's constructor forms them (occnerf_amd.gridencoder.grid_offsets) for D = 4, 16 levels,
              base resolution 2, desired resolution 256, log2_hashmap_size = 14: five dense levels, eleven hashed with 2^14
              entries, 1.5 MB of embeddings.  layout(generic=True): the last level cut to 12 344 entries, hashed and no power of
              two (the GENERIC instantiations), levels 0..14 with their entries.
pool(P)       the distinct samples every run draws from, the truth computed once for them: positions near a point, the ten
              finest ids its true nearest in-range points (a quarter in shuffled order), the thirty others random.  Rows 0..95
              are built by hand, see `pool`; `edges` names and checks each edge."""
import functools

import numpy as np

from tests import features_restatement as fr

F32 = np.float32
BOUND = 0.4
N_OUT = 6                                                 # points outside the bound, the last of a model
N_LANES8 = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 97, 6143, 6144, 6145)
N_ONE = (1, 255, 256, 257)
P_TABLE = (1, 255, 256, 257)
LDS_POINTS = 9216                                         # kLdsTailPoints
LDS_MIN_N = 6144                                          # 96 x 64: the LDS form from this N on
SENTINEL = 96                                             # the pool sample behind the dead entries of a row list
LONG_LDS, LONG_256 = 49157, 524293                        # > 2 x 256 x 96 and > 2 x 8192 x 32 sample groups: three pipelined trips
EQ_COUNT = 3.0


def b32():
    return float(F32(BOUND)), float(F32(2 * np.float64(BOUND)))


@functools.lru_cache(None)
def layout(generic=False):
    from occnerf_amd.gridencoder import grid_offsets
    off, pls = grid_offsets(4, 16, None, 2, 14, desired_resolution=256)
    off = off.astype(np.int64)
    rng = np.random.RandomState(11)
    emb = rng.uniform(-1, 1, (int(off[-1]), 2)).astype(F32)
    if generic:
        off = off.copy()
        off[16] = off[15] + 12344
        emb = emb[:off[16]].copy()
    lay = {'emb': emb, 'offsets': off.astype(np.int32), 'S': float(np.log2(pls)), 'H': 2, 'generic': generic}
    scale, res = fr.level_params(16, lay['S'], lay['H'])
    lay['modes'] = fr.level_modes(np.diff(off), res)
    assert lay['modes'][:2] == [fr.DENSE, fr.DENSE] and emb.nbytes < 4 << 20
    assert lay['modes'][15] == (fr.GENERIC if generic else fr.POW2) and set(lay['modes'][:15]) == {fr.DENSE, fr.POW2}
    return lay


@functools.lru_cache(None)
def model(P=257):
    rng = np.random.RandomState(1000 + P)
    base = rng.uniform(-0.35, 0.35, (P, 3)).astype(F32)
    base[P - N_OUT:] = rng.uniform(0.42, 0.5, (N_OUT, 3)).astype(F32)
    normals = rng.randn(P, 3) * rng.uniform(0.5, 2.0, (P, 1))
    normals[0] = (0.0, 2.5, 0.0)
    counter = rng.randint(0, 7, P).astype(F32)
    counter[:48] = EQ_COUNT
    b, tb = b32()
    m = {'P': P, 'base': base, 'normals': normals, 'unit': fr.unit_normals(normals), 'counter': counter, 'bound': b, 'two_bound': tb,
         'knn_base': rng.uniform(-0.38, 0.38, (P, 3)), 'sdf': rng.uniform(-0.3, 0.7, P).astype(F32),
         'learnable': rng.randn(P, 3).astype(F32)}
    kb = m['knn_base']
    kb[5 % P] = 0.41                                                               # beyond the bound: a zero row
    kb[6 % P, 1] = -0.4000001
    kb[7 % P] = np.float64(F32(BOUND))                                             # exactly on it: x = 1, in range
    kb[8 % P] = -np.float64(F32(BOUND))                                            # x = 0
    if P == 257:
        m['table'], m['table_x'] = fr.point_table(kb, m['sdf'], m['learnable'], b, tb, layout())
    else:
        m['table'] = np.concatenate([rng.uniform(-1, 1, (P, 35)).astype(F32), np.zeros((P, 1), F32)], 1)
    return m


def table64(table):
    """[P, 36] -> the device's [P, 64] rows (256-byte pitch), the columns beyond 36 zero."""
    return np.concatenate([table, np.zeros((len(table), 64 - table.shape[1]), F32)], 1)


def _nearest(xyz, base, cand, k):
    out = np.empty((len(xyz), k), cand.dtype)
    for a in range(0, len(xyz), 64):
        d = ((xyz[a:a + 64, None, :].astype(np.float64) - base[cand][None].astype(np.float64)) ** 2).sum(-1)
        out[a:a + 64] = cand[np.argsort(d, 1, kind='stable')[:, :k]]
    return out


@functools.lru_cache(None)
def pool(P=257, D=1200):
    """-> dict xyz [D, 3], knn [D, 40] and the rows built by hand:
    0..63    trip t has exactly one out-of-range sample, at slot t;  64..71  an all-out-of-range trip;
    72..79   one sample in each of the 8 slots;  80  all 40 ids equal;  81, 82  the same 40 ids in the same order (two positions);
    83       the ids of 81 in another order;  84, 85  equal counts;  86  neg = 5;  87  neg = 6;  88  a dot product of exactly 0;
    89       nd clamped at 0;  90  nd clamped at 1;  91  the sample ON its nearest point;  92  the ids 0 and P - 1."""
    m = model(P)
    rng = np.random.RandomState(2000 + P)
    base, inr, outp = m['base'], np.arange(P - N_OUT), np.arange(P - N_OUT, P)
    xyz = (base[rng.choice(inr, D)] + rng.uniform(-0.08, 0.08, (D, 3))).astype(F32)
    xyz[72:80] = xyz[72]
    xyz[91] = base[40]
    xyz[89] = (-0.34, -0.34, -0.34)
    xyz[90] = (0.34, -0.34, 0.34)
    xyz[88] = base[0] + np.array([0.03, 0.0, -0.02], F32)
    oob = [8 * t + t for t in range(8)] + list(range(64, 72))
    xyz[oob] = (base[outp[0]] + rng.uniform(-0.05, 0.0, (len(oob), 3))).astype(F32)
    knn = rng.randint(0, P, (D, 40)).astype(np.int32)
    fin = _nearest(xyz, base, inr, 10)
    for i in range(96, D, 4):
        fin[i] = fin[i][rng.permutation(10)]
    knn[:, :10] = fin
    for i in oob:
        knn[i, :3] = rng.choice(outp, 3)
    knn[72:80] = knn[72]
    knn[80] = 17
    knn[82] = knn[81]
    knn[83] = knn[81][np.concatenate([rng.permutation(10), 10 + rng.permutation(30)])]
    eqp = np.flatnonzero(m['counter'] == EQ_COUNT)
    eqp = eqp[eqp < P - N_OUT]
    for i in (84, 85):
        knn[i] = np.concatenate([_nearest(xyz[i:i + 1], base, eqp, 10)[0], rng.choice(eqp, 30)])
    g = fr.geometry(np.repeat(xyz[86:91], len(inr), 0), np.tile(inr, 5)[:, None].repeat(10, 1), m)
    dots, dist2 = g['dot'][:, 0].reshape(5, -1), (g['dir'][:, 0].astype(np.float64) ** 2).sum(-1).reshape(5, -1)

    def pick(row, n_neg, far):
        order = np.argsort(-dist2[row] if far else dist2[row], kind='stable')
        neg, pos = [p for p in order if dots[row, p] < 0], [p for p in order if dots[row, p] > 0]
        return inr[rng.permutation(np.array(neg[:n_neg] + pos[:10 - n_neg]))]
    knn[86, :10], knn[87, :10] = pick(0, 5, False), pick(1, 6, False)
    knn[88, 4] = 0
    knn[89, :10], knn[90, :10] = pick(3, 10, True), pick(4, 0, True)
    knn[91, :10] = _nearest(xyz[91:92], base, inr, 10)[0]
    knn[92, 10], knn[92, 39] = 0, P - 1
    return {'P': P, 'D': D, 'xyz': xyz, 'knn': knn, 'oob': np.array(oob)}


def edges(P=257):
    """Every edge the pool claims, asserted on the restated geometry.  -> dict of what was found."""
    m, pl = model(P), pool(P)
    g = fr.geometry(pl['xyz'], pl['knn'][:, :10], m)
    x, knn, cnt = g['x'], pl['knn'], m['counter'][pl['knn']]
    oob = ((x < 0) | (x > 1)).any(1)
    assert np.array_equal(np.flatnonzero(oob), np.sort(pl['oob'])) and (x[oob, :3] > 1).all()
    assert (g['den'] > 0).all() and np.isfinite(x).all()
    trips = oob[:72].reshape(9, 8)
    assert all(trips[t].sum() == 1 and trips[t, t] for t in range(8)) and trips[8].all()
    assert (pl['xyz'][72:80] == pl['xyz'][72]).all() and (knn[72:80] == knn[72]).all() and not oob[72:80].any()
    assert (knn[80] == knn[80, 0]).all()
    assert np.array_equal(knn[81], knn[82]) and not np.array_equal(pl['xyz'][81], pl['xyz'][82])
    assert not np.array_equal(knn[81], knn[83]) and np.array_equal(np.sort(knn[81]), np.sort(knn[83]))
    for i in (80, 84, 85):
        assert (cnt[i] == cnt[i, 0]).all()
    assert len(np.unique(knn[84])) > 1 and (cnt[96:] != cnt[96:, :1]).any(1).all()
    assert g['neg'][86] == 5 and g['dist'][86] > 0 and g['neg'][87] == 6 and g['dist'][87] < 0
    assert g['dot'][88, 4] == 0.0 and knn[88, 4] == 0
    assert g['nd_raw'][89] < 0 and x[89, 3] == 0.0 and g['nd_raw'][90] > 1 and x[90, 3] == 1.0
    assert not g['dir'][91, 0].any() and g['att'][91, 0] == 0.0 and (g['att'][91, 1:] > 0).all()
    assert knn[92, 10] == 0 and knn[92, 39] == P - 1
    inside = ~oob & (x[:, 3] > 0) & (x[:, 3] < 1)
    return {'out of range': int(oob.sum()), 'x[3] strictly inside (0, 1)': int(inside.sum()), 'neg histogram': np.bincount(g['neg'], minlength=11).tolist()}


def whole_map(D, N):
    """The pool sample behind row i of a whole-array run of N samples: the pool in its order, then seeded picks."""
    if N <= D:
        return np.arange(N)
    return np.concatenate([np.arange(D), np.random.RandomState(N).randint(0, D, N - D)])


def row_lists(D, cap):
    """Row lists into the pool's own arrays (xyz [D], knn [D]) in a tensor of `cap` entries -> [(name, rows int32 [cap], count)].
    The entries beyond the count hold SENTINEL, a valid sample."""
    rng = np.random.RandomState(cap)
    asc = np.sort(rng.choice(D, cap, replace=cap > D))

    def dead(n):
        r = np.full(cap, SENTINEL, np.int32)
        r[:n] = rng.randint(0, D, n)
        return r
    return [('ascending', asc.astype(np.int32), cap), ('unsorted with repeats', rng.randint(0, D, cap).astype(np.int32), cap),
            ('capacity beyond the count', dead(cap - 39), cap - 39), ('count 1', dead(1), 1), ('count 0', dead(0), 0)]


def long_list(D, n):
    return np.random.RandomState(n).randint(0, D, n).astype(np.int32)


def one_lane_cases(P=257):
    """nscale in {1, 2, 3, 4} x {plain, att_in, geo_idxs, both} with N through 1, 255, 256, 257 -> [dict name, nscale, N, q,
    att_in, geo]; q is features_restatement.problem's."""
    m, pl = model(P), pool(P)
    out = []
    for nscale in (1, 2, 3, 4):
        for k, mode in enumerate(('plain', 'att_in', 'geo_idxs', 'att_in + geo_idxs')):
            N = N_ONE[(nscale + k) % 4]
            rng = np.random.RandomState(100 * nscale + k)
            knn = np.ascontiguousarray(pl['knn'][:N, :10 * nscale])
            att = rng.uniform(0.0, 6.0, (N, 10 * nscale)).astype(F32) if 'att_in' in mode else None
            if att is not None and N > 80:
                att[80] = 2.5                                                       # equal counts through att_in
            geo = np.ascontiguousarray(pl['knn'][:N, :10][:, ::-1]) if 'geo' in mode else None
            out.append({'name': f'nscale {nscale} {mode} N {N}', 'nscale': nscale, 'N': N, 'att_in': att, 'geo': geo,
                        'q': fr.problem(m, pl['xyz'][:N], knn, geo, att)})
    return out


def centre_case(P=257):
    """75 samples around the pool sample 100: inside the radius they carry its 40 ids (copies of the centre, whose encoder input
    is the centre's bit for bit, and points a few 1e-3 off it), outside they are pool samples of their own.  Trips: 0, 1 all
    inside; 2, 3 all outside; 4..7 mixed; 8 inside; 9 the partial last one, its three live samples inside.
    -> dict c [3], r2, xyz [75, 3], knn [75, 40], inside [75]."""
    pl = pool(P)
    rng = np.random.RandomState(7)
    ci, r = 100, 0.02
    c, r2 = pl['xyz'][ci], F32(r * r)
    far = np.flatnonzero(np.sqrt(((pl['xyz'].astype(np.float64) - c) ** 2).sum(1)) > 2 * r)
    far = far[far >= 96][:48]
    inside = np.concatenate([np.ones(16, bool), np.zeros(16, bool), rng.rand(32) < 0.5, np.ones(11, bool)])
    inside[32:40] = [1, 0, 1, 1, 1, 1, 1, 1]
    inside[40:48] = [0, 0, 0, 0, 0, 0, 0, 1]
    N = len(inside)
    xyz, knn = np.empty((N, 3), F32), np.empty((N, 40), np.int32)
    off = (c[None] + rng.uniform(-0.004, 0.004, (N, 3))).astype(F32)
    copy = np.zeros(N, bool)
    copy[:8], copy[64:68], copy[72:] = True, True, True
    k = 0
    for i in range(N):
        if inside[i]:
            xyz[i], knn[i] = (c if copy[i] else off[i]), pl['knn'][ci]
        else:
            xyz[i], knn[i] = pl['xyz'][far[k]], pl['knn'][far[k]]
            k += 1
    d = xyz - c[None]
    d2 = fr.fma32(d[:, 2], d[:, 2], fr.fma32(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))
    assert np.array_equal(d2 < r2, inside) and N == 75
    return {'c': c, 'r2': r2, 'ci': ci, 'xyz': xyz, 'knn': knn, 'inside': inside, 'copy': copy}


_problems = {}


def pool_problem(P=257):
    if P not in _problems:
        _problems[P] = fr.problem(model(P), pool(P)['xyz'], pool(P)['knn'])
    return _problems[P]


@functools.lru_cache(None)
def pool_truth(P=257, generic=False, given=True):
    """The truth of the pool's samples, computed once per (model, layout, host offsets given or NULL) and never changed."""
    return fr.truth(model(P), layout(generic), pool_problem(P), given)
