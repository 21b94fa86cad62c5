"""float64 restatements of ONE launch of the trunk kernels (occnerf_amd/csrc/linear.hip: linear_kernel, wgrad_kernel +
wgrad_reduce_kernel; csrc/trunks.hip: the fused bf16 forward), the ten-layer chain and its backward assembled from them, and
the three kinds of per-entry check the GPU tests apply (tests/test_n_trunks_per_entry.py).  numpy only; nothing of the package.

Operands are the elements exactly as a launch read them (bf16 or fp32 bits widened to float64), so a ReLU unit flipped upstream
changes the operands of the next check, never its verdict.  With u = 2^-24 and gamma_n = n u / (1 - n u):

  1. stored bf16, random operands:  lo = bf16(epi(r - e)) <= got <= hi = bf16(epi(r + e)), e = gamma_{K+2} A: rounding to
     nearest even and ReLU are monotone, so no tolerance is chosen.  A = sum |x||W| + |bias|, K the total reduction length
     (K products + K additions would be 2K roundings, but a term passes through one product rounding -- none in bf16, where
     a product of two 8-bit significands is exact in fp32 -- at most K additions and the bias addition: K + 2).
  2. fp32 result, random operands:  |got - r| <= gamma_n A + u |r|.  Forward: n = K + 2.  Weight gradient: n = rows of the
     largest slice + 8 (wgrad_kernel: a term of dW passes through the product rounding and one addition per row of its
     slice, rows_per_wg of them; a term of db through rows / 2 per-lane additions -- a lane owns every second row in fp32,
     8 of each 16 in bf16, paired before they join the running sum -- and one cross-lane addition; the 8 covers those.  The
     reduce sums the slices in float64 and rounds once: u |r|).  A = 0 entries must be exact zeros.
  3. dyadic operands (small integers): every product and partial sum is an integer below 2^24, so the result equals the
     float64 value bit for bit (a bf16 store: its RNE rounding), whatever the summation order -- any lost, duplicated or
     misplaced term shows at any shape.

Every bound also carries the float64 reference's own error, n 2^-53 A (1e-9 of the bound; zero on dyadic operands).
The bounds assume each fp32 addition inside an MFMA is rounded to nearest or better.
"""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(n, u=U):
    return n * u / (1.0 - n * u)


# ---- bf16 ---------------------------------------------------------------------------------------------------------------
def _quantum(x):
    """Spacing of bf16 at |x| (8 significant bits, subnormals below 2^-126)."""
    _, e = np.frexp(np.abs(x))
    return np.ldexp(1.0, np.maximum(e - 8, -133))


def bf16_rne(x):
    """float64 -> the nearest bf16 value (ties to even), as float64; ONE rounding (not through fp32)."""
    x = np.asarray(x, np.float64)
    q = _quantum(x)
    return np.copysign(np.rint(np.abs(x) / q) * q, x)


def bf16_trunc(x):
    """float64 -> bf16 by dropping bits (the defect a missing rounding increment would be)."""
    x = np.asarray(x, np.float64)
    q = _quantum(x)
    return np.copysign(np.floor(np.abs(x) / q) * q, x)


def bf16_ulp_up(v):
    """The next bf16 value above v (v: bf16 values as float64)."""
    v = np.asarray(v, np.float64)
    up = v + _quantum(v)
    down = v + _quantum(v * (1 - 2.0 ** -9))          # negative v: towards zero, the spacing just below |v|
    return np.where(v >= 0, up, down)


def is_bf16(x):
    x = np.asarray(x, np.float64)
    return bool(np.all(bf16_rne(x) == x))


def rnd(x, bf16):
    """Operand in its stored format, widened: bf16 or fp32 rounding of a float64 array."""
    x = np.asarray(x, np.float64)
    return bf16_rne(x) if bf16 else x.astype(np.float32).astype(np.float64)


# ---- one launch of linear_forward ---------------------------------------------------------------------------------------
def relu(v):
    return np.maximum(v, 0.0)


def ident(v):
    return v


def linear_ref(x0, W, bias=None, x1=None):
    """-> r[M,N] = sum_k x[m,k] W[n,k] + bias[n] over both segments, A[M,N] = sum |x||W| + |bias|, K."""
    x = np.asarray(x0, np.float64) if x1 is None else np.concatenate([np.asarray(x0, np.float64), np.asarray(x1, np.float64)], 1)
    W = np.asarray(W, np.float64)
    assert x.shape[1] == W.shape[1], (x.shape, W.shape)
    r, A = x @ W.T, np.abs(x) @ np.abs(W).T
    if bias is not None:
        b = np.asarray(bias, np.float64)
        r, A = r + b, A + np.abs(b)
    return r, A, x.shape[1]


def live(mask, shape):
    """Entries the masked epilogue keeps: mask > 0 (so -0.0, +0.0 and every negative value kill)."""
    return np.ones(shape, bool) if mask is None else np.asarray(mask, np.float64)[:, :shape[1]] > 0


def interval(r, A, K, epi=ident, mask=None):
    """Kind 1 -> (lo, hi): the bf16 values a correctly rounded fp32 accumulation of any order may store."""
    e = (gamma(K + 2) + (K + 2) * U64) * A
    keep = live(mask, r.shape)
    lo, hi = bf16_rne(epi(r - e)), bf16_rne(epi(r + e))
    return np.where(keep, lo, 0.0), np.where(keep, hi, 0.0)


def check_interval(name, got, r, A, K, epi=ident, mask=None, cap=0.25):
    """Kind 1.  -> share of entries that admit more than one bf16 value (asserted <= cap on the reference alone)."""
    got = np.asarray(got, np.float64)
    assert got.shape == r.shape, (name, got.shape, r.shape)
    lo, hi = interval(r, A, K, epi, mask)
    wide = float(np.mean(lo != hi)) if lo.size else 0.0
    assert wide <= cap, f'{name}: {wide:.3f} of the entries admit two bf16 values: the case does not pin the kernel'
    bad = ~((lo <= got) & (got <= hi))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f'{name}: {int(bad.sum())}/{bad.size} entries outside [lo, hi], first at {i}: got {got[i]!r}, '
                             f'lo {lo[i]!r}, hi {hi[i]!r}, r {r[i]!r}')
    return wide


def f32_bound(r, A, n):
    return (gamma(n) + n * U64) * A + U * np.abs(r)


def check_f32(name, got, r, A, n, mask=None):
    """Kind 2.  -> worst err / bound over the entries with a non-zero bound; zero-bound entries must be exact."""
    got = np.asarray(got, np.float64)
    assert got.shape == r.shape, (name, got.shape, r.shape)
    keep = live(mask, r.shape) if mask is not None else np.ones(r.shape, bool)
    r, A = np.where(keep, r, 0.0), np.where(keep, A, 0.0)
    err, bound = np.abs(got - r), f32_bound(r, A, n)
    bad = ~(err <= bound)                                   # (a NaN fails)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        worst = np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))
        raise AssertionError(f'{name}: {int(bad.sum())}/{bad.size} entries beyond the bound (worst err / bound {worst:.3g}), '
                             f'first at {i}: got {got[i]!r}, want {r[i]!r}, bound {bound[i]:.3e}')
    pos = bound > 0
    return float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0


def assert_dyadic(name, r, A):
    """The operands make every product and partial sum an integer below 2^24 (asserted on the reference)."""
    assert np.all(A < 2.0 ** 24) and np.all(A == np.rint(A)) and np.all(r == np.rint(r)), f'{name}: not a dyadic case'


def check_exact(name, got, want):
    """Kind 3: bit equality (as values; +0.0 and -0.0 are the same result)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = got != want
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f'{name}: {int(bad.sum())}/{bad.size} entries differ, first at {i}: got {got[i]!r}, want {want[i]!r}')
    return 'bit-equal'


def check_linear(name, got, r, A, K, relu_on=False, mask=None, bf16_out=False, dyadic=False):
    """One stored result of a linear_forward launch under the check its kind calls for.  -> what to print."""
    epi = relu if relu_on else ident
    if dyadic:
        assert_dyadic(name, r, A)
        want = np.where(live(mask, r.shape), epi(r), 0.0)
        return check_exact(name, got, bf16_rne(want) if bf16_out else want)
    if bf16_out:
        return 'in [lo, hi], %.1f %% wide' % (100 * check_interval(name, got, r, A, K, epi, mask))
    return '%.3f' % check_f32(name, got, epi(r), A, K + 2, mask)   # (|relu(a) - relu(b)| <= |a - b|: the same bound)


# ---- one launch of linear_wgrad + reduce --------------------------------------------------------------------------------
def wgrad_slices(M):
    """-> (G, rows per slice) of occnerf_linear_wgrad: 32-row tiles dealt to min(tiles, 256) slices, whole tiles each."""
    tiles = (M + 31) // 32
    G = min(tiles, 256)
    return G, (tiles + G - 1) // G * 32


def wgrad_terms(M):
    return min(M, wgrad_slices(M)[1]) + 8


def wgrad_ref(dz, x):
    """-> full[n_pad,k_pad], A_W, db[n_pad], A_b in float64 (before the maps)."""
    dz, x = np.asarray(dz, np.float64), np.asarray(x, np.float64)
    return dz.T @ x, np.abs(dz).T @ np.abs(x), dz.sum(0), np.abs(dz).sum(0)


def scatter(full, row_map, col_map, shape):
    """-> (values placed through the maps into `shape`, which entries were placed)."""
    out, hit = np.zeros(shape), np.zeros(shape, bool)
    rn, ck = np.asarray(row_map), None if col_map is None else np.asarray(col_map)
    for n in np.flatnonzero(rn >= 0):
        if ck is None:
            out[rn[n]], hit[rn[n]] = full[n], True
        else:
            k = np.flatnonzero(ck >= 0)
            out[rn[n], ck[k]], hit[rn[n], ck[k]] = full[n, k], True
    return out, hit


def check_wgrad(name, dW, db, dz, x, row_map, col_map, M, before_W, before_b, accumulate=False, dyadic=False, holes=True):
    """dW / db after one launch against float64 of its operands.  before_*: the buffers' contents before the launch: entries
    no map reaches must still hold them (bit for bit: they may be uninitialised memory), and accumulate adds to them.
    holes: the maps leave part of the buffers out (asserted, so that the case checks it).  -> (what to print for dW, for db)."""
    full, AW, sb, Ab = wgrad_ref(dz, x)
    n = wgrad_terms(M)
    out = []
    for nm, got, ref, A, cm, before in ((name + ' dW', dW, full, AW, col_map, before_W), (name + ' db', db, sb, Ab, None, before_b)):
        if got is None:
            out.append('-')
            continue
        got, before = np.asarray(got, np.float64), np.asarray(before, np.float64)
        want, hit = scatter(ref, row_map, cm, got.shape)
        AA, _ = scatter(A, row_map, cm, got.shape)
        assert hit.any() and not (holes and hit.all()), f'{nm}: the maps of this case must have holes'
        kept = np.where(np.isnan(before), np.isnan(got), got == before)
        assert kept[~hit].all(), f'{nm}: {int((~kept[~hit]).sum())} entries that no map reaches were written'
        if accumulate:
            want, AA = want + np.where(hit, before, 0.0), AA + np.where(hit, np.abs(before), 0.0)
        if dyadic:
            assert_dyadic(nm, want, AA)
            out.append(check_exact(nm, got[hit], want[hit]))
        else:
            out.append('%.3f' % check_f32(nm, got[hit][None], want[hit][None], AA[hit][None], n))
    return tuple(out)


# ---- the ten layers: the layout of occnerf_mlp.py:183-199 ---------------------------------------------------------------
#   h   = [knn_feats 35 | var 1 | enc 32]                       -> pts_linears.{0,2,4,6} -> geo_linear (65 rows: sigma, 64 features)
#   rgb = [features 64 | knn_feats 35 | enc 32]  (131 columns)  -> rgb_linears.{0,2,4,6} -> output_linear (3 rows)
# The kernels' buffers: X0[M,96] = h padded; GEO[M,96] = features in columns 0..63, sigma in column 64, pad; widths padded to 32.
N_AGG, N_VAR, N_ENC, N_FEAT = 35, 1, 32, 64
LAYERS = ['pts_linears.0', 'pts_linears.2', 'pts_linears.4', 'pts_linears.6', 'geo_linear.0',
          'rgb_linears.0', 'rgb_linears.2', 'rgb_linears.4', 'rgb_linears.6', 'output_linear.0']
SHAPES = [(256, 68)] + [(256, 256)] * 3 + [(65, 256), (256, 131)] + [(256, 256)] * 3 + [(3, 256)]


def _padded(entries, width):
    return np.array(list(entries) + [-1] * (width - len(entries)), np.int32)


def trunk_maps():
    """Row / column maps (padded position -> index in the nn.Linear weight, -1: none) derived from the layout above."""
    h_cols = {('agg', j): j for j in range(N_AGG)}
    h_cols[('var', 0)] = N_AGG
    h_cols.update({('enc', j): N_AGG + N_VAR + j for j in range(N_ENC)})
    x0_slots = [('agg', j) for j in range(N_AGG)] + [('var', 0)] + [('enc', j) for j in range(N_ENC)]       # X0's columns
    rgb_cols = {('feat', j): j for j in range(N_FEAT)}
    rgb_cols.update({('agg', j): N_FEAT + j for j in range(N_AGG)})
    rgb_cols.update({('enc', j): N_FEAT + N_AGG + j for j in range(N_ENC)})
    geo_slots = [('feat', j) for j in range(N_FEAT)] + [('sigma', 0)]                                     # GEO's columns
    geo_rows = {('sigma', 0): 0}
    geo_rows.update({('feat', j): 1 + j for j in range(N_FEAT)})
    ident256 = np.arange(256, dtype=np.int32)
    seg0 = _padded([rgb_cols.get(s, -1) for s in geo_slots], 96)
    seg1 = _padded([rgb_cols.get(s, -1) for s in x0_slots], 96)
    rows = [ident256] * 4 + [_padded([geo_rows[s] for s in geo_slots], 96)] + [ident256] * 4 + [_padded([0, 1, 2], 32)]
    cols = [_padded([h_cols[s] for s in x0_slots], 96)] + [ident256] * 4 + [np.concatenate([seg0, seg1])] + [ident256] * 4
    return {'rows': rows, 'cols': cols, 'rgb_seg0': seg0, 'rgb_seg1': seg1}


def pack(W, b, row_map, col_map, bf16=None):
    """-> Wp[n_pad,k_pad], bias_p[n_pad]: the weight through the maps (0 where a map has none), rounded to the flavour."""
    W = np.asarray(W, np.float64)
    Wp, bp = np.zeros((len(row_map), len(col_map))), np.zeros(len(row_map))
    rn, ck = np.flatnonzero(row_map >= 0), np.flatnonzero(col_map >= 0)
    Wp[np.ix_(rn, ck)] = W[np.ix_(row_map[rn], col_map[ck])]
    if b is not None:
        bp[rn] = np.asarray(b, np.float64)[row_map[rn]]
    return (Wp if bf16 is None else rnd(Wp, bf16)), bp


def chain_forward(Ws, bs, agg, var, enc, bf16=None):
    """The ten launches of the staged forward, each linear_ref of the previous one's stored result.  bf16: None = nothing is
    rounded (the float64 restatement), True / False = the flavour's storage roundings.  -> dict of the saved tensors + raw4."""
    maps = trunk_maps()
    store = (lambda v: v) if bf16 is None else (lambda v: rnd(v, bf16))
    P = [pack(Ws[l], bs[l], maps['rows'][l], maps['cols'][l], bf16) for l in range(10)]
    M = agg.shape[0]
    X0 = np.zeros((M, 96))
    X0[:, :35], X0[:, 35:36], X0[:, 36:68] = agg, var, enc
    X0 = store(X0)
    acts = [X0]
    for l in range(4):
        acts.append(store(relu(linear_ref(acts[-1], P[l][0], P[l][1])[0])))
    g = linear_ref(acts[4], P[4][0], P[4][1])[0]
    GEO = store(g)
    B = [store(relu(linear_ref(GEO, P[5][0], P[5][1], x1=X0)[0]))]
    for l in range(6, 9):
        B.append(store(relu(linear_ref(B[-1], P[l][0], P[l][1])[0])))
    rgb = linear_ref(B[3], P[9][0], P[9][1])[0]
    raw4 = np.concatenate([rgb[:, :3], g[:, 64:65]], 1)
    return {'acts': acts, 'GEO': GEO, 'B': B, 'raw4': raw4, 'packs': P}


# the 21 launches of the backward (10 input-gradient passes, 11 weight-gradient passes), in order: ('wgrad', layer, n_pad, k_pad, with_db) / ('dgrad', n_pad, k0, k1, masked, out_f32)
BACKWARD_LAUNCHES = (
    [('wgrad', 9, 32, 256, True), ('dgrad', 256, 32, 0, True, False)]
    + [t for l in (8, 7, 6) for t in (('wgrad', l, 256, 256, True), ('dgrad', 256, 256, 0, True, False))]
    + [('wgrad', 5, 256, 96, True), ('wgrad', 5, 256, 96, False), ('dgrad', 96, 256, 0, False, False)]
    + [('wgrad', 4, 96, 256, True), ('dgrad', 256, 96, 0, True, False)]
    + [t for l in (3, 2, 1) for t in (('wgrad', l, 256, 256, True), ('dgrad', 256, 256, 0, True, False))]
    + [('wgrad', 0, 256, 96, True), ('dgrad', 96, 256, 256, False, True)])


def chain_backward(fw, draw4, bf16=None, log=None):
    """The backward of chain_forward's result from the per-launch restatements, in the order of BACKWARD_LAUNCHES.
    -> dx0[M,96], dW[10], db[10] (dW / db in the nn.Linear layout, through the maps).  log: a list that receives the (r, A) of
    every launch."""
    maps = trunk_maps()
    store = (lambda v: v) if bf16 is None else (lambda v: rnd(v, bf16))
    acts, GEO, B, P = fw['acts'], fw['GEO'], fw['B'], fw['packs']
    X0, M = acts[0], acts[0].shape[0]
    dW = [np.zeros(s) for s in SHAPES]
    db = [np.zeros(s[0]) for s in SHAPES]

    def wgrad(l, dz, x, col_map=None, with_db=True):
        full, AW, sb, Ab = wgrad_ref(dz, x)
        if log is not None:
            log.extend([(full, AW), (sb, Ab)])
        cm = maps['cols'][l] if col_map is None else col_map
        w, hit = scatter(full, maps['rows'][l], cm, SHAPES[l])
        dW[l][hit] = w[hit]
        if with_db:
            v, hb = scatter(sb, maps['rows'][l], None, (SHAPES[l][0],))
            db[l][hb] = v[hb]

    def dgrad(dz, Wt, mask=None, x1=None):
        r, A, _ = linear_ref(dz, Wt, x1=x1)
        if log is not None:
            log.append((r, A))
        return np.where(live(mask, r.shape), r, 0.0)

    Wt = [p[0].T for p in P]
    dz = np.zeros((M, 32))
    dz[:, :3] = draw4[:, :3]
    dz = store(dz)
    wgrad(9, dz, B[3])
    dz = store(dgrad(dz, Wt[9], B[3]))
    for l in (8, 7, 6):
        wgrad(l, dz, B[l - 6])
        dz = store(dgrad(dz, Wt[l], B[l - 6]))
    wgrad(5, dz, GEO, col_map=maps['rgb_seg0'])
    wgrad(5, dz, X0, col_map=maps['rgb_seg1'], with_db=False)
    dgeo = store(dgrad(dz, Wt[5][:96]))
    dz_rgb0 = dz
    dgeo[:, 64] = store(draw4[:, 3])
    wgrad(4, dgeo, acts[4])
    dz = store(dgrad(dgeo, Wt[4], acts[4]))
    for l in (3, 2, 1):
        wgrad(l, dz, acts[l])
        dz = store(dgrad(dz, Wt[l], acts[l]))
    wgrad(0, dz, X0)
    dx0 = dgrad(dz_rgb0, np.concatenate([Wt[5][96:], Wt[0]], 1), x1=dz)
    return dx0, dW, db
