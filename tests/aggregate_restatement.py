"""Float64 restatements of the neighbour aggregation (occnerf_amd/csrc/aggregate.hip), the truth
tests/test_t_aggregate_per_entry.py holds its three kernels to PER ENTRY, and tests/test_aggregate_restatement.py keeps honest
on the CPU.  u = 2^-24, gamma_k = k u / (1 - k u); per entry A = the float64 sum of |terms|.

agg_forward_kernel: agg[n, c] = sum_j atts[n, j] feats[knn[n, j], c]
-------------------------------------------------------------------
The library is built with -ffp-contract=off and the kernel rounds every product with __fmul_rn, so the terms
t_j = fl32(w_j f[id_j, c]) are formed here bit for bit (`forward_terms`); the kernel and the truth sum_j t_j differ ONLY in the
order of the sum, and the bound gamma_k A counts the fp32 additions a term can meet, from the code:

  pair branch (F <= 36 and K <= 64)   group g = 0, 1, 2 adds its m_g = ceil((K - g) / 3) terms j = g, g + 3, ... serially into a
      register that starts at 0: the first addition is exact, m_g - 1 round (the padded trips of a shorter group add w = 0:
      exact).  Two more additions join the three groups, (s_0 + s_1) + s_2; one with an empty group (K < 3) adds 0 and is exact.
      Group 0 is the longest:  k = (ceil(K / 3) - 1) + (min(K, 3) - 1)  -- 0, 1, 2, 15, 23 at K = 1, 2, 3, 40, 64.
  generic branch (F > 36 or K > 64)   one register, j = 0 .. K - 1 in order, the first addition exact:  k = K - 1.

Exact duties on top of the bound: K = 1 is bit-equal to t_0 (k = 0); dyadic operands (every partial sum exact in fp32) are
bit-equal on both branches; rows of equal (ids, weight bits) are bit-equal to each other wherever they stand (the kernel copies
a row from its predecessor inside a group of 8 samples and gathers again otherwise); a row with its predecessor's ids and ONE
other weight bit is not a copy of it.

agg_runs_kernel + agg_backward_tiled_kernel + the sum of the W partial tables: grad_feats[p, c] = sum_{(n, j): knn[n, j] = p} w g
-----------------------------------------------------------------------------------------------------------------------------
The run pre-pass adds the gradient rows of a run (consecutive samples of one 64-sample chunk with bitwise equal ids and
weights) in fp64 and rounds once to fp32 (a run of one row: exact).  The tiled kernel adds the products w gsum, exact in fp64
(24 x 24 bits), into an fp64 LDS cell and rounds the cell to fp32 once; ops.agg_backward adds the W partial tables in fp32, at
most W - 1 additions.  A term meets at most 1 + 1 + (W - 1) = W + 1 fp32 roundings, and the fp64 additions (a run's and a
cell's, fewer than the n pairs (sample, neighbour) that name the point) lose 2^-53 each:

    |got - truth| <= gamma_{W + 1} A + n 2^-53 A,    A = sum |w_nj| |g_n,c| over the n pairs that name the point.

(The count is the "volume" bound's of step_backward_restatement.py plus the run's rounding.)  Exact duties: a point with A = 0
-- no sample names it, or only samples of zero gradient rows -- is exactly zero in EVERY partial table; a point named once, by a
run of one sample, equals fl32(w g).

`forward_emulate` / `backward_emulate` carry out the kernels' own orders and roundings in numpy; their `mutate` arguments make
the wrong answers the CPU test shows the checks to refuse."""
import numpy as np

from tests.aggregate_cases import tile_points
from tests.encoder_backward_restatement import U32, U64, gamma  # noqa: F401

F32 = np.float32
CHUNK = 64                                                # kAggRun: samples a wave walks for runs
GROUP = 8                                                 # kAggFwdRun: samples a forward wave takes


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- forward ------------------------------------------------------------------------------------------------------------
def pair_branch(F, K):
    return F <= 36 and K <= 64


def forward_k(F, K):
    """The fp32 additions a term can meet (module docstring)."""
    return (-(-K // 3) - 1) + (min(K, 3) - 1) if pair_branch(F, K) else K - 1


def forward_terms(c):
    """t[n, j, c] = fl32(w_nj f[id_nj, c]), the kernel's __fmul_rn."""
    return (c['atts'][:, :, None] * c['feats'][c['knn'].astype(np.int64)]).astype(F32)


def forward_truth(c):
    """-> (float64 sum of the fp32 terms [N, F], A = float64 sum of their absolute values)."""
    t = forward_terms(c).astype(np.float64)
    return t.sum(1), np.abs(t).sum(1)


def forward_emulate(c, mutate=None):
    """The kernel's own summation order in np.float32.  mutate = 'copy': a row whose IDS equal its predecessor's inside a group
    of 8 samples is copied from it whatever its weights (the defect the weights' comparison closed)."""
    t = forward_terms(c)
    N, K, F = t.shape
    if pair_branch(F, K):
        s = [np.zeros((N, F), F32) for _ in range(3)]
        for j in range(K):
            s[j % 3] = (s[j % 3] + t[:, j]).astype(F32)
        out = ((s[0] + s[1]).astype(F32) + s[2]).astype(F32)
    else:
        out = np.zeros((N, F), F32)
        for j in range(K):
            out = (out + t[:, j]).astype(F32)
    if mutate == 'copy':
        for n in range(1, N):
            if n % GROUP and np.array_equal(c['knn'][n], c['knn'][n - 1]):
                out[n] = out[n - 1]
    return out


def _raise_worst(name, err, bound, got64, ssum, where):
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, np.where(bound > 0, ratio, np.inf), -1.0)), err.shape)
        raise AssertionError(f'{name}: {int(bad.sum())} entries over their bound; worst at {where(i)}: got {float(got64[i])!r}, '
                             f'float64 sum {float(ssum[i])!r}, bound {bound[i]:.3e}')
    return float(ratio.max()) if ratio.size else 0.0


def check_forward(name, c, got):
    """Every entry within gamma_k A of the float64 sum of the fp32 terms, and the exact duties.  Prints and returns the worst
    error / bound."""
    F, K, N = c['F'], c['K'], c['N']
    got = np.asarray(got, F32)
    assert got.shape == (N, F), (name, got.shape)
    got64 = got.astype(np.float64)
    assert np.isfinite(got64).all(), f'{name}: entries are not finite'
    ssum, A = forward_truth(c)
    k = forward_k(F, K)
    bound = gamma(k) * A if k else np.zeros_like(A)
    worst = _raise_worst(name, np.abs(got64 - ssum), bound, got64, ssum, lambda i: f'row {int(i[0])} column {int(i[1])}')
    exact = ''
    if K == 1 or c['dyadic']:
        want = (forward_terms(c).astype(np.float64).sum(1) + 0.0).astype(F32)                   # exact in fp32 by construction
        assert np.array_equal(want.astype(np.float64), ssum)
        ne = bits(got) != bits(want)
        assert not ne.any(), f'{name}: {int(ne.sum())} entries are not bit-equal; first at row {np.argwhere(ne)[0][0]} column {np.argwhere(ne)[0][1]}'
        exact = ', bit-equal to the exact sum'
    seen = {}
    for n in range(N):                                                                          # rows of equal (ids, weight bits)
        key = c['knn'][n].tobytes() + bits(c['atts'][n]).tobytes()
        if key in seen:
            ne = bits(got[n]) != bits(got[seen[key]])
            assert not ne.any(), f'{name}: row {n} has the ids and weight bits of row {seen[key]} but differs from it at column {np.flatnonzero(ne)[0]}'
        else:
            seen[key] = n
    for n in c['flipped']:
        assert np.array_equal(c['knn'][n], c['knn'][n - 1]) and int((bits(c['atts'][n]) != bits(c['atts'][n - 1])).sum()) == 1
        assert (bits(got[n]) != bits(got[n - 1])).any(), f'{name}: row {n} differs from row {n - 1} in one weight bit and is a copy of it'
    print(f'   forward {name}: {"pair" if pair_branch(F, K) else "generic"} branch, k = {k}, worst error / bound {worst:.3f} over '
          f'{got.size} entries, {N - len(seen)} rows equal to an earlier one{exact}')
    return worst


# ---- backward -----------------------------------------------------------------------------------------------------------
def slices_and_per(N, forced=0):
    """occnerf_agg_backward_slices and the launch's samples per slice, restated (aggregate.hip): whole 64-sample chunks."""
    W = forced if forced >= 1 else min(max(-(-N // 3072), 1), 256)
    return W, -(-(-(-N // W)) // CHUNK) * CHUNK


def scatter64(knn, w, g, P):
    """float64 [P, F]: out[p] = sum over the pairs (n, j) with knn[n, j] = p of w[n, j] g[n], and the pairs' number [P]."""
    knn = np.asarray(knn, np.int64)
    M, K = knn.shape
    out, cnt = np.zeros((P, g.shape[1])), np.zeros(P, np.int64)
    if M == 0:
        return out, cnt
    ids = knn.reshape(-1)
    order = np.argsort(ids, kind='stable')
    sid = ids[order]
    vals = np.asarray(w, np.float64).reshape(-1)[order, None] * np.asarray(g, np.float64)[np.repeat(np.arange(M), K)[order]]
    starts = np.flatnonzero(np.concatenate([[True], sid[1:] != sid[:-1]]))
    out[sid[starts]] = np.add.reduceat(vals, starts, axis=0)
    cnt[sid[starts]] = np.diff(np.concatenate([starts, [len(sid)]]))
    return out, cnt


def backward_truth(c):
    """-> (float64 gradient [P, F], A [P, F], n [P])."""
    ssum, n = scatter64(c['knn'], c['atts'], c['gout'], c['P'])
    A, _ = scatter64(c['knn'], np.abs(c['atts']), np.abs(c['gout']), c['P'])
    return ssum, A, n


def run_heads(c):
    """head[n]: the first sample of sample n's run -- consecutive samples of one 64-sample chunk with bitwise equal ids and
    weights (agg_runs_kernel)."""
    knn, wb = c['knn'], bits(c['atts'])
    N = len(knn)
    new = np.ones(N, bool)
    new[1:] = (knn[1:] != knn[:-1]).any(1) | (wb[1:] != wb[:-1]).any(1) | (np.arange(1, N) % CHUNK == 0)
    return np.maximum.accumulate(np.where(new, np.arange(N), 0))


def backward_emulate(c, mutate=None):
    """The three launches in numpy: run sums in fp64 rounded once, per slice an fp64 cell rounded once, the W partials added in
    fp32 in order.  -> (total [P, F] fp32, partial [W, P, F] fp32).  mutate: 'drop' (the one term of the point named once
    left out), 'boundary' (the id tile_points credited to row tile_points - 1), 'slice' (slice 1's partial left out for the
    point 7), 'head' (a run's head row used unsummed)."""
    knn, atts, gout, P = c['knn'].copy(), c['atts'].astype(np.float64), c['gout'], c['P']
    N, F = gout.shape
    head = run_heads(c)
    gs64 = np.zeros((N, F))
    np.add.at(gs64, head, gout.astype(np.float64))
    gsum = gs64.astype(F32)                                                                     # non-head rows hold zeros: they add nothing
    if mutate == 'head':
        a = c['runs'][-1][0]
        gsum[a] = gout[a]
    if mutate == 'drop':
        atts[c['once']] = 0.0
    if mutate == 'boundary':
        n, j = c['boundary']
        assert knn[n, j] == c['tile_points']
        knn[n, j] -= 1
    live = gsum.any(1)
    W, per = slices_and_per(N, c['forced'])
    partial = np.zeros((W, P, F), F32)
    for s in range(W):
        sel = np.flatnonzero(live[s * per:(s + 1) * per]) + s * per
        partial[s] = scatter64(knn[sel], atts[sel], gsum[sel], P)[0].astype(F32)
    if mutate == 'slice':
        assert W >= 2 and partial[1, 7].any()
        partial[1, 7] = 0.0
    total = partial[0].copy()
    for s in range(1, W):
        total = (total + partial[s]).astype(F32)
    return total, partial


def check_backward(name, c, total, partial=None, truth=None):
    """Every entry of the summed gradient within gamma_{W+1} A + n 2^-53 A; A = 0 exactly zero, in every partial table where
    they are given; the point named once by a run of one sample bit-equal to fl32(w g).  Prints and returns the worst
    error / bound."""
    P, F, N = c['P'], c['F'], c['N']
    W, per = slices_and_per(N, c['forced'])
    ssum, A, n = backward_truth(c) if truth is None else truth
    total = np.asarray(total, F32)
    assert total.shape == (P, F), (name, total.shape)
    got64 = total.astype(np.float64)
    assert np.isfinite(got64).all(), f'{name}: entries are not finite'
    bound = gamma(W + 1) * A + n[:, None] * U64 * A
    tp = c['tile_points']
    worst = _raise_worst(name, np.abs(got64 - ssum), bound, got64, ssum,
                         lambda i: f'point {int(i[0])} (tile {int(i[0]) // tp}, row {int(i[0]) % tp}) column {int(i[1])}, named by {int(n[i[0]])} pairs')
    if partial is not None:
        partial = np.asarray(partial, F32)
        assert partial.shape == (W, P, F), (name, partial.shape)
        stray = (partial != 0) & (A == 0)[None]
        assert not stray.any(), f'{name}: a point without terms is not zero in partial table {np.argwhere(stray)[0][0]}: point {np.argwhere(stray)[0][1]}'
        beyond = [s for s in range(W) if s * per >= N]
        assert not partial[beyond].any(), f'{name}: slices {beyond} start beyond N and must write zeros'
    ns, js = c['once']
    p = int(c['knn'][ns, js])
    assert n[p] == 1 and run_heads(c)[ns] == ns and (ns + 1 == N or run_heads(c)[ns + 1] == ns + 1)
    want = ((np.float64(c['atts'][ns, js]) * c['gout'][ns].astype(np.float64)) + 0.0).astype(F32)
    ne = bits(total[p]) != bits(want)
    assert not ne.any(), f'{name}: point {p}, named once by sample {ns}, is not fl32(w g) at column {np.flatnonzero(ne)[0]}'
    assert n[c['unnamed']] == 0 and not total[c['unnamed']].any()
    print(f'   backward {name}: W = {W} slices of {per}, {c["tiles"]} tiles of {tp}, worst error / bound {worst:.3f} over '
          f'{int((A > 0).sum())} entries with terms of {A.size} (fullest point {int(n.max())} pairs), {int((n == 0).sum())} points unnamed')
    return worst
