"""Seeded inputs of the per-entry tests of agg_forward_kernel, agg_runs_kernel and agg_backward_tiled_kernel
(occnerf_amd/csrc/aggregate.hip; tests/test_t_aggregate_per_entry.py on the GPU, tests/test_aggregate_restatement.py on the
CPU): the smallest sizes that still reach each branch.  Every builder returns plain numpy arrays: feats [P, F] fp32, knn [N, K]
int32 (every id in [0, P)), atts [N, K] fp32, gout [N, F] fp32, and the rows / points planted on purpose."""
import numpy as np

F32 = np.float32
TILE_VALUES = 18432                                       # the kernel's kAggTileValues: doubles of LDS per point tile


def tile_points(F):
    return min(TILE_VALUES // F, 1024)


def _softmax(x):
    e = np.exp(x - x.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(F32)


def flip_bit(w, bit=22):
    """One fp32 with one mantissa bit flipped."""
    return (np.asarray(w, F32).view(np.uint32) ^ np.uint32(1 << bit)).view(F32)


# ---- forward ------------------------------------------------------------------------------------------------------------
FORWARD_N = [1, 7, 8, 9, 63, 64, 65, 2003]                # both sides of the 8-sample group and of the 4-wave block; 2003 = 8 * 250 + 3
PAIR_F, PAIR_K = (1, 2, 35, 36), (1, 2, 3, 40, 64)
GENERIC = [(37, 40), (37, 64), (64, 40), (64, 64), (35, 65), (35, 130), (64, 65), (64, 130)]


def forward_case(F, K, N, dyadic=False):
    """Random rows, and planted among them (as far as N allows): row 3 = row 2 (the same group of 8 samples: the kernel copies),
    row 8 = row 7 (the next group: gathered again), row 12 = row 2 (not a neighbour), and row 5 with row 4's ids and row 4's
    weights but for ONE bit of one entry (mantissa bit 22): no copy.  dyadic: weights 2^-e, e = 0..6, features k / 64 with
    |k| <= 64: every product and every partial sum of up to 130 of them is exact in fp32 (multiples of 2^-12 below 2^8)."""
    rng = np.random.RandomState(7919 * F + 31 * K + N + (1 if dyadic else 0))
    P = 6890 if N > 1000 else 97
    if dyadic:
        feats = (rng.randint(-64, 65, (P, F)) / 64.0).astype(F32)
        atts = (2.0 ** -rng.randint(0, 7, (N, K))).astype(F32)
    else:
        feats = rng.randn(P, F).astype(F32)
        atts = _softmax(rng.randn(N, K))
    knn = rng.randint(0, P, (N, K)).astype(np.int32)
    equal, flipped = [], []
    for dst, src in ((3, 2), (8, 7), (12, 2)):
        if N > dst:
            knn[dst], atts[dst] = knn[src], atts[src]
            equal.append((dst, src))
    if N > 5:
        knn[5], atts[5] = knn[4], atts[4]
        atts[5, K // 2] = flip_bit(atts[4, K // 2])
        flipped.append(5)
    return {'name': f'F={F} K={K} N={N}' + (' dyadic' if dyadic else ''), 'F': F, 'K': K, 'N': N, 'P': P, 'feats': feats, 'knn': knn,
            'atts': atts, 'equal': equal, 'flipped': flipped, 'dyadic': dyadic}


def forward_cases():
    """Pair branch: F in {1, 2, 35, 36} x K in {1, 2, 3, 40, 64}, N cycling through FORWARD_N, and every N at F = 35, K = 40.
    Generic branch: F in {37, 64} x K in {40, 64} (one trip of the j0 loop) and K in {65, 130} at F = 35 and 64 (two and three
    trips).  Dyadic: one case per branch and trip count."""
    out = []
    i = 0
    for F in PAIR_F:
        for K in PAIR_K:
            out.append(forward_case(F, K, FORWARD_N[i % len(FORWARD_N)]))
            i += 1
    out += [forward_case(35, 40, N) for N in FORWARD_N]
    out += [forward_case(F, K, 65 if K <= 64 else 130) for F, K in GENERIC]
    out += [forward_case(35, 40, 65, dyadic=True), forward_case(36, 64, 9, dyadic=True), forward_case(37, 40, 65, dyadic=True),
            forward_case(64, 130, 64, dyadic=True), forward_case(35, 65, 9, dyadic=True)]
    return out


# ---- backward -----------------------------------------------------------------------------------------------------------
BACKWARD_F, BACKWARD_K = (1, 18, 19, 35, 36, 64), (1, 3, 40, 64)
P_KINDS = ('less than a tile', 'one tile', 'one tile + 1')
RUN_LENGTHS = [1, 2, 7, 8, 9, 63, 64, 65, 130, 500, 3, 1, 1000]


def backward_case(F, K, N, P, seed, runs='short', forced=0, name=None):
    """Random ids in [0, P) with, planted:
      point 3       named by no sample: exactly zero in every partial table;
      point 5       named once, by sample `once` = (n, j) whose run has length 1 and whose gradient row is scaled by 2^-20: its
                    entry is fl32(w g), some 1e-8 -- the sparsely visited point a tolerance relative to the largest entry forgets;
      sample b + 1  (b = 0, or 1900 behind the long runs) ids tile_points - 1 and tile_points in the same list (two samples where K = 1), where P reaches past one tile;
      sample b + 2  the same id twice in its list (K >= 2);
      sample b + 4  every id in the first tile;   sample b + 6: ids spread over all tiles, neighbour j in tile j mod tiles;
      point 7       named five times by every sample (K >= 40): contended LDS atomics and the largest entries by far.
    runs = 'short': samples 20..29 and 60..69 are runs (across the 8-sample trip and the 64-sample chunk), row 24 is zero inside
    its run and rows 100..103 are a run of zero rows.  runs = 'long': the lengths RUN_LENGTHS from sample 11 on, two samples apart
    (N >= 1900), zero rows [0, 11), 40, [700, 705) and the last 50.  The gradient rows carry scales 10^-2 .. 1."""
    rng = np.random.RandomState(seed)
    tp = tile_points(F)
    tiles = -(-P // tp)
    assert P >= 12 and N >= 130
    knn = rng.randint(0, P, (N, K)).astype(np.int32)
    atts = _softmax(rng.randn(N, K))
    gout = (rng.randn(N, F) * 10.0 ** rng.uniform(-2, 0, (N, 1))).astype(F32)
    if K >= 40:
        knn[:, :5] = 7
    b = 0 if runs == 'short' else 1900                     # the planted samples stand clear of the runs and of the zero rows
    planted = {}
    if P > tp:
        if K >= 2:
            knn[b + 1, K - 2], knn[b + 1, K - 1] = tp - 1, tp
            planted['boundary'] = (b + 1, K - 1)
        else:
            knn[b + 1, 0], knn[b + 3, 0] = tp - 1, tp
            planted['boundary'] = (b + 3, 0)
    if K >= 2:
        knn[b + 2, K - 1] = knn[b + 2, 0]
    knn[b + 4] = rng.randint(0, min(tp, P), K)
    knn[b + 6] = np.minimum((np.arange(K) % tiles) * tp + rng.randint(0, 5, K), P - 1)
    if runs == 'short':
        for a, b in ((20, 30), (60, 70), (100, 104)):
            knn[a:b], atts[a:b] = knn[a], atts[a]
        gout[24] = 0.0
        gout[100:104] = 0.0
        run_rows = [(20, 30), (60, 70)]
    else:
        pos, run_rows = 11, []
        for ln in RUN_LENGTHS:
            knn[pos:pos + ln], atts[pos:pos + ln] = knn[pos], atts[pos]
            run_rows.append((pos, pos + ln))
            pos += ln + 2
        assert pos <= b and b + 6 < N - 60
        gout[:11] = 0.0
        gout[40] = 0.0
        gout[700:705] = 0.0
        gout[-50:] = 0.0
    once = (N - 55, K // 2)                                # a sample outside every planted run
    knn[np.isin(knn, (3, 5))] = 6
    knn[once] = 5
    gout[once[0]] = (gout[once[0]] * F32(2.0 ** -20)).astype(F32)
    assert gout[once[0]].any() and knn.min() >= 0 and knn.max() < P and not (knn == 3).any() and int((knn == 5).sum()) == 1
    planted.update({'once': once, 'unnamed': 3, 'runs': run_rows})
    return {'name': name or f'F={F} K={K} N={N} P={P}', 'F': F, 'K': K, 'N': N, 'P': P, 'knn': knn, 'atts': atts, 'gout': gout,
            'forced': forced, 'tile_points': tp, 'tiles': tiles, **planted}


def backward_grid():
    """F in {1, 18, 19, 35, 36, 64} x K in {1, 3, 40, 64} at N = 200, P cycling through less than a tile, exactly one tile and
    one tile + 1 (a last tile of one row)."""
    out = []
    i = 0
    for F in BACKWARD_F:
        tp = tile_points(F)
        for K in BACKWARD_K:
            kind = P_KINDS[i % 3]
            P = {'less than a tile': tp // 2 + 3, 'one tile': tp, 'one tile + 1': tp + 1}[kind]
            out.append(backward_case(F, K, 200, P, 500 + i, name=f'F={F} K={K} N=200 P={P} ({kind})'))
            i += 1
    return out


def backward_limits():
    """Exactly 32 point tiles, the accepted limit, at F = 64 (288 rows each) and F = 35 (526 rows each)."""
    return [backward_case(64, 40, 200, 9216, 601, name='F=64 K=40 N=200 P=9216 (32 tiles)'),
            backward_case(35, 40, 200, 16832, 602, name='F=35 K=40 N=200 P=16832 (32 tiles)')]


def backward_slices():
    """N = 3073: two slices, the second from sample 1600, with the long runs (the run of 1000 crosses the slice boundary, which
    is a chunk boundary: it is cut there).  N = 6145: three slices of 2112.  N = 130 with the slice knob forced to 5: slices of 64
    samples, the last two beyond N."""
    return [backward_case(35, 40, 3073, 6890, 701, runs='long', name='F=35 K=40 N=3073 P=6890 (2 slices, long runs)'),
            backward_case(35, 40, 6145, 6890, 702, runs='long', name='F=35 K=40 N=6145 P=6890 (3 slices)'),
            backward_case(35, 40, 130, 6890, 703, forced=5, name='F=35 K=40 N=130 P=6890 (5 forced slices, 2 empty)')]
