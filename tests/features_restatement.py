"""Restatements of the render-path feature kernels (occnerf_amd/csrc/features.hip) -- sample_features_kernel (one lane per
sample), sample_features8_kernel (8 lanes per sample), point_table_kernel and point_pack_kernel -- the truth
tests/test_v_features_per_entry.py holds them to PER ENTRY, and tests/test_features_restatement.py keeps honest on the CPU.
u = 2^-24, gamma_k = k u / (1 - k u).

The library is built with -ffp-contract=off and the kernels round every operation on its own (__f*_rn / __d*_rn, plain fp32
`+` and `*`) or through an explicit __fmaf_rn; expf is the only operation that is not a correctly rounded IEEE one.

Bit-exact parts (compared as integers)
--------------------------------------
`fma32`       the fp32 FMA: the product of two fp32 numbers is exact in float64 (24 x 24 bits), TwoSum gives the float64 sum
              s = fl64(p + c) with its exact error e, and where e != 0 and s is even s moves to its odd neighbour on e's side
              (rounding to odd: 53 >= 2 x 24 + 2 bits, so the final rounding to fp32 sees what the exact sum would show it).
              tests/test_features_restatement.py holds it to rational arithmetic on random and on half-way operands.
`geometry`    dir = fl(p - nbr); dot in fp64, ((0 + d0 n0) + d1 n1) + d2 n2; norm3 = sqrtf(fma(z, z, fma(y, y, fl(x x)))); the
              sequential fp32 sum over the ten finest neighbours, / 10, the sign flip only when 2 neg > 10; nd = (dist + 0.2) / 0.5
              clamped; x[0..2] = fl32(num / den), the fp64 sums over neighbours 0..2 of att pn with att = |cos3_unit| (its norm
              clamped at 1e-8) and pn = fl32(fl32(nbr + bound) / two_bound).  The 8-lanes kernel spreads the neighbours over the
              lanes and joins them through shuffles in the same order: one function serves both kernels.
`encode`      per level pos = fma(x, scale, 0.5), the cell floor(pos) and the fraction pos - floor(pos); the 16 corners in the order
              idx = b0 | b1 << 1 | b2 << 2 | b3 << 3 with weight ((f0 f1) f2) f3 and r = fma(w, v, r); the index of a corner
              dense (sum of pg stride_d, uint32), hashed with a power-of-two size (xor of pg prime_d, masked) or generic (the
              reference's stride loop, hash and modulo -- every level when the host offsets are NULL).  level_taps_select's
              shared pair terms give the same integers modulo 2^32.  An input outside [0, 1] gives 32 zeros.
variance      column 35 in each kernel's own order: one lane, sequentially over j (step_preamble_restatement.agg_weights_f32);
              8 lanes, per-lane sums of five from 0 then the xor-1 / 2 / 4 butterfly, ((L0 + L1) + (L2 + L3)) + ((L4 + L5) +
              (L6 + L7)) in every lane (an fp32 addition commutes).
expf argument agg_weights_f32's, the same in both kernels (min, max and the subtraction do not depend on an order).
point_table   x = fl32((knn_base + bound) / two_bound) in fp64, s = (sdf + 0.2) / 0.8 clamped, `encode`, the learnable columns
              copied, column 35 zero.  point_pack: copies (`pack_records`).

Counted bound for the columns 0..34, the ones behind expf
---------------------------------------------------------
Truth: T = sum_j r_j t_j in float64, r = softmax64 of the bit-exact fp32 arguments, t the fp32 table entries; A = sum_j |r_j t_j|.
The kernel forms w_j = fl(e_j / ssum), e_j = expf(arg_j), and adds the rounded products fl(w_j t_j).

weight      |w_j - r_j| <= ew r_j,  ew = c u (K + 4) + (1 + s) u.  The first term is step_preamble_restatement.check_agg_weights'
            bound on agg_weights' softmax, E = r (K + 4) and c = 4 max(rho_ref, 1) with rho_ref measured on torch's CPU fp32
            softmax of the same arguments against float64 (0.03 to 0.3 on these cases, so c = 4: the one measured constant, and
            never measured on the kernel under test).  On top of it this kernel's own division att / ssum (1) and the additions
            an exponential meets on its way into ssum: s = K - 1 in the one-lane kernel (sequential over j, the first addition
            to 0 counted although exact), s = 4 + 3 = 7 in the 8-lanes kernel (five per lane, three butterfly levels).
sum         a term meets its product's rounding and the additions of its chain: columns 0..31 add sequentially over j in both
            kernels, 1 + (K - 1) = K roundings; columns 32..34 the same in the one-lane kernel and 1 + 4 + 3 = 8 in the 8-lanes
            kernel (`tail[c] += a5[k] * tl[k]` per lane, then the butterfly).
bound       |got - T| <= ((1 + ew) (1 + gamma_acc) - 1) A per entry; nothing relative to a tensor's largest entry, no entry
            left out.  K = 40: ew = 216 u (8 lanes) / 248 u (one lane), acc = 40 / 8.

Exact without a bound: when all K neighbours of a sample carry the same count every argument of expf is 0, expf(0) = 1, the
weight is fl(1 / K) and the variance exactly 0, so columns 0..35 are restated bit for bit (`emulate` with exp correctly rounded
is exact there).

`emulate` carries out either kernel in np.float32 with exp taken from float64 and rounded; its `defect` argument plants the
wrong answers the CPU test shows `check_features` to refuse by name."""
import ctypes

import numpy as np

from tests.step_preamble_restatement import (F32, U32, agg_weights_f32, c_of, gamma, ratio, softmax_rows_ref,  # noqa: F401
                                             softmax_rows_ref32, unit_normals)

KNN = 10
DENSE, POW2, GENERIC = 0, 1, 2
PRIMES = (1, 2654435761, 805459861, 3674653429)
DEFECTS = ('skip', 'twice', 'lane_weight', 'neighbour_tail', 'var_K', 'flip_at_5', 'no_clamp', 'oob_untransposed',
           'oob_not_zeroed', 'generic_mask')
SKIP_J = 17                                               # the neighbour the 'skip' / 'twice' defects touch (owner lane 3)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- exact fp32 FMA -------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fl32(a b + c) with one rounding (module docstring)."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, F32).astype(np.float64) for v in (a, b, c)))
    shape = a.shape
    p = np.ascontiguousarray(a * b).reshape(-1)                                    # exact
    c = np.ascontiguousarray(c).reshape(-1)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                                                  # p + c = s + e exactly
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32).reshape(shape)


def norm3(d):
    """d [..., 3] fp32 -> sqrtf(fma(z, z, fma(y, y, fl(x x))))."""
    d = np.asarray(d, F32)
    return np.sqrt(fma32(d[..., 2], d[..., 2], fma32(d[..., 1], d[..., 1], d[..., 0] * d[..., 0])))


# ---- neighbour geometry ---------------------------------------------------------------------------------------------------
def geometry(xyz, gid, m, defect=None):
    """xyz [N, 3] fp32, gid [N, 10] ids of the finest scale, m: a model of tests/features_cases.py.  -> dict dist [N], x [N, 4]
    (fp32, bit-exact), neg [N], dot [N, 10], att [N, 3], den [N], nd_raw [N]."""
    p, gid = np.asarray(xyz, F32), np.asarray(gid, np.int64)
    nbr = m['base'][gid]
    dir_ = p[:, None, :] - nbr
    d64, nm = dir_.astype(np.float64), m['normals'][gid]
    dot = ((0.0 + d64[..., 0] * nm[..., 0]) + d64[..., 1] * nm[..., 1]) + d64[..., 2] * nm[..., 2]
    neg = (dot < 0.0).sum(1)
    nrm = norm3(dir_)
    dsum = np.zeros(len(p), F32)
    for j in range(KNN):
        dsum = dsum + nrm[:, j]
    dist = dsum / F32(KNN)
    dist = np.where(2 * neg >= KNN if defect == 'flip_at_5' else 2 * neg > KNN, -dist, dist)
    nd_raw = (dist + F32(0.2)) / F32(0.5)
    nd = nd_raw if defect == 'no_clamp' else np.where(nd_raw < 0, F32(0), np.where(nd_raw > 1, F32(1), nd_raw))
    na = np.where(nrm[:, :3] < F32(1e-8), F32(1e-8), nrm[:, :3])
    t = (dir_[:, :3] / na[..., None]).astype(np.float64) * m['unit'][gid[:, :3]]
    att = np.abs((t[..., 0] + t[..., 1]) + t[..., 2])
    pn = ((nbr[:, :3] + F32(m['bound'])) / F32(m['two_bound'])).astype(np.float64)
    num, den = np.zeros((len(p), 3)), np.zeros(len(p))
    for j in range(3):
        num = num + att[:, j, None] * pn[:, j]
        den = den + att[:, j]
    with np.errstate(invalid='ignore', divide='ignore'):
        x3 = (num / den[:, None]).astype(F32)
    x = np.concatenate([x3, nd.astype(F32)[:, None]], 1)
    assert dist.dtype == x.dtype == F32
    return {'dist': dist, 'x': x, 'neg': neg, 'dot': dot, 'att': att, 'den': den, 'nd_raw': nd_raw, 'dir': dir_}


# ---- the hash encoding ----------------------------------------------------------------------------------------------------
_exp2f = None


def level_params(L, S, H):
    """make_grid_levels: scale = fmaf(exp2f(l S), H, -1) with the HOST's exp2f, resolution = ceil(scale) + 1."""
    global _exp2f
    if _exp2f is None:
        _exp2f = ctypes.CDLL('libm.so.6').exp2f
        _exp2f.restype, _exp2f.argtypes = ctypes.c_float, [ctypes.c_float]
    scale = np.array([fma32(F32(_exp2f(float(F32(l) * F32(S)))), F32(H), F32(-1.0)) for l in range(L)], F32)
    return scale, (np.ceil(scale).astype(np.int64) + 1)


def level_modes(sizes, res, given=True):
    """make_grid_modes_d4; without the host's copy of the offsets every level is generic."""
    modes = []
    for size, r in zip(sizes, res):
        size, stride, fits = int(size), 1, True
        for _ in range(4):
            if stride > size:
                fits = False
                break
            stride *= int(r) + 1
        if not given:
            modes.append(GENERIC)
        elif fits and stride <= size:
            modes.append(DENSE)
        elif size > 0 and size & (size - 1) == 0 and stride > size:
            modes.append(POW2)
        else:
            modes.append(GENERIC)
    return modes


def _level_index(pl, mode, size, res, mask_generic=False):
    """pl [N, 4] uint32 corner cells -> the entry inside the level, uint32 arithmetic as grid_index's."""
    size, r1 = int(size), (int(res) + 1) & 0xFFFFFFFF
    with np.errstate(over='ignore'):
        if mode == DENSE:
            index, stride = np.zeros(len(pl), np.uint32), 1
            for d in range(4):
                index = index + pl[:, d] * np.uint32(stride)
                stride = (stride * r1) & 0xFFFFFFFF
            return index
        h = np.zeros(len(pl), np.uint32)
        for d in range(4):
            h = h ^ (pl[:, d] * np.uint32(PRIMES[d]))
        if mode == POW2:
            return h & np.uint32(size - 1)
        index, stride = np.zeros(len(pl), np.uint32), 1
        for d in range(4):
            if stride <= size:
                index = index + pl[:, d] * np.uint32(stride)
                stride = (stride * r1) & 0xFFFFFFFF
        if stride > size:
            index = h
        return index & np.uint32(size - 1) if mask_generic else index % np.uint32(size)


def encode(x, lay, given=True, defect=None):
    """x [N, 4] fp32 -> the 32 encoded columns [N, 2 L] fp32, bit-exact.  lay: a layout of tests/features_cases.py."""
    x = np.asarray(x, F32)
    emb, off = lay['emb'], np.asarray(lay['offsets'], np.int64)
    L, N = len(off) - 1, len(x)
    scale, res = level_params(L, lay['S'], lay['H'])
    sizes = np.diff(off)
    modes = level_modes(sizes, res, given)
    oob = ((x < 0) | (x > 1) | np.isnan(x)).any(1)
    xs = np.where(oob[:, None], F32(0.5), x)                                       # (the kernels' discarded gathers stay inside the table)
    out = np.zeros((N, L, 2), F32)
    for l in range(L):
        pos = fma32(xs, scale[l], F32(0.5))
        fl = np.floor(pos)
        pg, fr = fl.astype(np.uint32), pos - fl
        f = (F32(1.0) - fr, fr)
        w01 = [f[i & 1][:, 0] * f[i >> 1][:, 1] for i in range(4)]
        r = np.zeros((N, 2), F32)
        for idx in range(16):
            b = [(idx >> d) & 1 for d in range(4)]
            w = (w01[b[0] | (b[1] << 1)] * f[b[2]][:, 2]) * f[b[3]][:, 3]
            index = _level_index(pg + np.array(b, np.uint32)[None], modes[l], sizes[l], res[l],
                                 mask_generic=(defect == 'generic_mask' and modes[l] == GENERIC))
            assert int(index.max(initial=0)) < int(sizes[l])
            r = fma32(w[:, None], emb[off[l] + index.astype(np.int64)], r)
        out[:, l] = r
    if defect != 'oob_not_zeroed':
        out[oob] = 0.0
    return out.reshape(N, 2 * L)


# ---- the per-point kernels ------------------------------------------------------------------------------------------------
def point_table(knn_base, sdf, learnable, bound, two_bound, lay):
    """-> (table [P, 36] fp32, x [P, 4] fp32)."""
    kb = np.asarray(knn_base, np.float64)
    x3 = ((kb + np.float64(F32(bound))) / np.float64(F32(two_bound))).astype(F32)
    s = (np.asarray(sdf, F32) + F32(0.2)) / F32(0.8)
    s = np.where(s < 0, F32(0), np.where(s > 1, F32(1), s)).astype(F32)
    x = np.concatenate([x3, s[:, None]], 1)
    return np.concatenate([encode(x, lay), np.asarray(learnable, F32), np.zeros((len(kb), 1), F32)], 1), x


def pack_records(m, table):
    """-> (geo [P, 16] fp32 words: xyz, 0 | normal | unit normal as fp64 pairs; tail [P, 4]: table columns 32..34, count)."""
    P = len(m['base'])
    geo = np.zeros((P, 16), F32)
    geo[:, :3] = m['base']
    geo[:, 4:] = np.ascontiguousarray(np.concatenate([m['normals'], m['unit']], 1)).view(F32)
    return geo, np.concatenate([np.asarray(table, F32)[:, 32:35], m['counter'][:, None]], 1).astype(F32)


# ---- the visibility softmax and the gather --------------------------------------------------------------------------------
def _lane_sum(v):
    s = np.zeros(v.shape[:2] + v.shape[3:], F32)
    for k in range(5):
        s = s + v[:, :, k]
    return s


def _butterfly(L):
    s1 = L[:, 0::2] + L[:, 1::2]
    s2 = s1[:, 0::2] + s1[:, 1::2]
    return s2[:, 0] + s2[:, 1]


def softmax_parts(att, defect=None):
    """att [N, K] fp32 counts -> a (normalised), arg (of expf), var_one, var_eight (None unless K = 40): fp32, bit-exact."""
    att = np.asarray(att, F32)
    N, K = att.shape
    var_one, arg = agg_weights_f32(att.reshape(-1), np.arange(N * K).reshape(N, K), 'div_K' if defect == 'var_K' else None)
    a = att + (F32(1.0) - att.min(1))[:, None]
    a = a / a.max(1)[:, None]
    assert np.array_equal(bits(a - a.max(1)[:, None]), bits(arg))
    var_eight = None
    if K == 40:
        lanes = a.reshape(N, 8, 5)
        mean = _butterfly(_lane_sum(lanes)) / F32(K)
        dl = lanes - mean[:, None, None]
        var_eight = _butterfly(_lane_sum(dl * dl)) / F32(K if defect == 'var_K' else K - 1)
    return a, arg, var_one, var_eight


def agg_rel_bound(K, kernel):
    """c-free part of the bound -> (s, acc [35]): the additions into ssum and the roundings of a column's chain."""
    acc = np.full(35, K)
    if kernel == 'eight':
        acc[32:] = 1 + 4 + 3
    return (K - 1 if kernel == 'one' else 4 + 3), acc


def agg_bound(A, K, kernel, rho):
    s, acc = agg_rel_bound(K, kernel)
    ew = c_of(rho) * U32 * (K + 4) + (1 + s) * U32
    return ((1.0 + ew) * (1.0 + gamma(acc.astype(np.float64))) - 1.0)[None, :] * A


def problem(m, xyz, knn, geo=None, att_in=None):
    """One call's operands: knn [N, K] table ids, geo [N, 10] geometry ids (the first ten of knn when absent), att [N, K] counts."""
    knn = np.asarray(knn, np.int32)
    return {'xyz': np.asarray(xyz, F32), 'knn': knn, 'geo': knn[:, :KNN] if geo is None else np.asarray(geo, np.int32),
            'att': m['counter'][knn] if att_in is None else np.asarray(att_in, F32)}


def truth(m, lay, q, given=True):
    """Everything the checks compare against, for the samples of `q` (module docstring)."""
    g = geometry(q['xyz'], q['geo'], m)
    a, arg, var_one, var_eight = softmax_parts(q['att'])
    K = arg.shape[1]
    t = m['table'][q['knn'].astype(np.int64)][:, :, :35].astype(np.float64)
    r, E = softmax_rows_ref(arg)
    terms = r[..., None] * t
    rho = float(ratio(softmax_rows_ref32(arg), r, E).max()) if len(arg) else 0.0
    equal = (q['att'] == q['att'][:, :1]).all(1)
    tr = {'dist': g['dist'], 'x': g['x'], 'enc': encode(g['x'], lay, given), 'var': {'one': var_one, 'eight': var_eight}, 'arg': arg,
          'sum': terms.sum(1), 'A': np.abs(terms).sum(1), 'rho': rho, 'K': K, 'equal': equal, 'geom': g,
          'oob': ((g['x'] < 0) | (g['x'] > 1)).any(1)}
    _, key = np.unique(np.concatenate([q['knn'], bits(q['att']).view(np.int32)], 1), axis=0, return_inverse=True)
    tr['idkey'] = key.reshape(-1)
    tr['exact'] = {k: emulate(m, lay, q, k, given=given)['mlp_in'][:, :36] for k in (('one', 'eight') if K == 40 else ('one',))}
    assert not var_one[equal].any() and not arg[equal].any()
    return tr


def emulate(m, lay, q, kernel, defect=None, given=True):
    """Either kernel in np.float32, exp from float64 rounded once.  -> dict mlp_in [N, 68], dist [N], x [N, 4].  Samples stand in
    trips of 8 in their order (slot = i & 7; the lanes of a short last trip repeat the last sample)."""
    assert defect is None or defect in DEFECTS
    g = geometry(q['xyz'], q['geo'], m, defect)
    N = len(q['xyz'])
    enc = encode(g['x'], lay, given, defect)
    if defect == 'oob_untransposed':                                               # level pair s of a sample zeroed when slot s of its trip is out of range
        oob = ((g['x'] < 0) | (g['x'] > 1)).any(1)
        enc = encode(g['x'], lay, given, 'oob_not_zeroed').reshape(N, 8, 4)
        mate = np.minimum((np.arange(N) & ~7)[:, None] + np.arange(8)[None], N - 1)
        enc = np.where(oob[mate][:, :, None], F32(0), enc).reshape(N, 32)
    a, arg, var_one, var_eight = softmax_parts(q['att'], defect)
    K = arg.shape[1]
    e = np.exp(arg.astype(np.float64)).astype(F32)
    t = m['table'][q['knn'].astype(np.int64)][:, :, :35].astype(F32)
    if kernel == 'one':
        ssum = np.zeros(N, F32)
        for j in range(K):
            ssum = ssum + e[:, j]
    else:
        assert K == 40
        ssum = _butterfly(_lane_sum(e.reshape(N, 8, 5)))
    w = e / ssum[:, None]
    wm, tm = w.copy(), t.copy()
    if defect == 'twice':
        tm[:, SKIP_J] = tm[:, SKIP_J - 1]
    if defect == 'lane_weight':
        wm[:, 15:20] = w[:, 20:25]
    cols = 35 if kernel == 'one' else 32
    agg = np.zeros((N, cols), F32)
    for j in range(K):
        if not (defect == 'skip' and j == SKIP_J):
            agg = agg + wm[:, j, None] * tm[:, j, :cols]
    if kernel == 'eight':
        tail = _butterfly(_lane_sum(w.reshape(N, 8, 5, 1) * t[:, :, 32:].reshape(N, 8, 5, 3)))
        if defect == 'neighbour_tail':
            tail = tail[np.minimum(np.arange(N) ^ 1, N - 1)]
        agg = np.concatenate([agg, tail], 1)
    var = var_one if kernel == 'one' else var_eight
    out = np.concatenate([agg, var[:, None], enc], 1)
    assert out.dtype == F32 and out.shape == (N, 68)
    return {'mlp_in': out, 'dist': g['dist'], 'x': g['x']}


# ---- the checks -----------------------------------------------------------------------------------------------------------
def _where(i, slots, form):
    return f'sample {int(i)} (slot {int(slots[i])} of its trip, {form})'


def _bit_check(name, what, got, want, slots, form):
    ne = bits(got) != bits(want)
    if ne.any():
        i = np.argwhere(ne.reshape(len(ne), -1))[0]
        raise AssertionError(f'{name}: {what} is not bit-equal to the restatement in {int(ne.sum())} entries; first at {_where(i[0], slots, form)} '
                             f'column {int(i[1])}: got {np.asarray(got).reshape(len(ne), -1)[i[0], i[1]]!r}, '
                             f'restated {np.asarray(want).reshape(len(ne), -1)[i[0], i[1]]!r}')


def check_features(name, tr, kernel, mlp_in, dist, x, sel=None, slots=None, form=''):
    """One call's outputs against the truth `tr` of a pool; sel [n]: the pool sample behind output row i (all of them in order
    when absent), slots [n]: its slot in its trip of 8.  Bit-equal: distance, encoder input, the 32 encoded columns, the
    variance, columns 0..35 of the rows of equal counts, the rows of equal (ids, counts) among each other and the rows of one
    sample among each other.  Columns 0..34 within the counted bound, per entry.  Prints and returns the worst error / bound."""
    mlp_in = np.asarray(mlp_in, F32)
    n = len(mlp_in)
    sel = np.arange(n) if sel is None else np.asarray(sel, np.int64)
    slots = (np.arange(n) & 7) if slots is None else slots
    form = form or kernel
    assert mlp_in.shape == (n, 68) and len(sel) == n, (name, mlp_in.shape, len(sel))
    if n == 0:
        return 0.0
    _bit_check(name, 'the signed distance', np.asarray(dist, F32).reshape(n, 1), tr['dist'][sel].reshape(n, 1), slots, form)
    if x is not None:
        _bit_check(name, 'the encoder input', np.asarray(x, F32).reshape(n, 4), tr['x'][sel], slots, form)
    _bit_check(name, 'the hash encoding (columns 36..67)', mlp_in[:, 36:], tr['enc'][sel], slots, form)
    assert not mlp_in[:, 36:][tr['oob'][sel]].any()
    _bit_check(name, 'the variance (column 35)', mlp_in[:, 35:36], tr['var'][kernel][sel].reshape(n, 1), slots, form)
    got64 = mlp_in[:, :35].astype(np.float64)
    assert np.isfinite(got64).all(), f'{name}: entries are not finite'
    bound = agg_bound(tr['A'][sel], tr['K'], kernel, tr['rho'])
    err = np.abs(got64 - tr['sum'][sel])
    r = np.divide(err, bound, out=np.where(err > 0, np.inf, 0.0), where=bound > 0)
    worst = float(r.max())
    if not worst <= 1.0:
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError(f'{name}: {int((r > 1).sum())} entries of columns 0..34 over their bound; worst {worst:.3g} at {_where(i[0], slots, form)} '
                             f'column {int(i[1])}: got {got64[i]!r}, float64 {float(tr["sum"][sel][i])!r}, bound {float(bound[i]):.3e}')
    eq = tr['equal'][sel]
    _bit_check(name, 'a row of equal counts (columns 0..35)', mlp_in[eq, :36], tr['exact'][kernel][sel][eq], slots[eq], form)
    for what, key, cols in (('(ids, counts)', tr['idkey'][sel], 36), ('sample', sel, 68)):
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
        ne = (bits(mlp_in[:, :cols]) != bits(mlp_in[first[inv.reshape(-1)], :cols])).any(1)
        assert not ne.any(), (f'{name}: {_where(np.flatnonzero(ne)[0], slots, form)} has the {what} of row {int(first[inv.reshape(-1)][np.flatnonzero(ne)[0]])} '
                              f'and differs from it in columns 0..{cols - 1}')
    print(f'   {name} [{form}]: {n} rows, {int(tr["oob"][sel].sum())} out of range, {int(eq.sum())} of equal counts; distance, x, encoding, variance '
          f'bit-equal; columns 0..34 worst error / bound {worst:.3f} (rho_ref {tr["rho"]:.2f})')
    return worst
