"""What tests/test_d_encoder_backward.py and tests/test_encoder_backward_restatement.py feed the D = 4, C = 2 encoder's backward:
the host's dispatch arithmetic restated (index mode per level, tile-jobs of the tiled launch), the level layouts that reach
each branch of that dispatch, and the seeded inputs and gradients."""
import numpy as np

from tests.test_encoder_restatement import level_scale

TILE_ENTRIES = 8192                       # kTileEntries of the tiled D = 4, C = 2 backward


# ---- the host's dispatch arithmetic (common.hip make_grid_modes_d4, grid_encode.hip grid_backward_impl) ----------------
def grid_modes_d4(offsets, S, H):
    """Per level: 'D' dense (all four strides fit the table), 'P' hashed with a power-of-two size, 'G' generic."""
    modes = ''
    for level in range(len(offsets) - 1):
        size = int(offsets[level + 1] - offsets[level])
        res = int(np.ceil(level_scale(level, S, H))) + 1
        stride, fits = 1, True
        for _ in range(4):
            if stride > size:
                fits = False
                break
            stride *= res + 1
        if fits and stride <= size:
            modes += 'D'
        elif size & (size - 1) == 0 and stride > size:
            modes += 'P'
        else:
            modes += 'G'
    return modes


def tile_jobs(offsets, S, H):
    """-> (modes, tiles per level, slices per level, tile-jobs in total) of the tiled backward's launch."""
    modes = grid_modes_d4(offsets, S, H)
    tiles = [(int(offsets[l + 1] - offsets[l]) + TILE_ENTRIES - 1) // TILE_ENTRIES for l in range(len(modes))]
    slices = [16 if m == 'D' else 8 for m in modes]
    return modes, tiles, slices, sum(t * s for t, s in zip(tiles, slices))


def slices_per_entry(offsets, S, H, entries=None):
    """nsl of the level each table entry (all of them, or the given ascending ones) belongs to."""
    _, _, slices, _ = tile_jobs(offsets, S, H)
    if entries is None:
        return np.repeat(np.asarray(slices, np.float64), np.diff(np.asarray(offsets, np.int64)))
    return np.asarray(slices, np.float64)[np.searchsorted(np.asarray(offsets, np.int64), entries, side='right') - 1]


# ---- level layouts of the D = 4, C = 2 encoder that reach every branch of the tiled backward's dispatch -----------------------
LAYOUTS = {
    'default': dict(L=16, H=16, log2=19, desired=2048 * 1.4),                       # masked scan (the training step's table)
    # hashed levels that are no power of two: generic index in the mask pre-pass and the tile scan, partial last tiles
    'generic': dict(L=16, H=16, log2=19, desired=2048 * 1.4, resize={3: 300000, 6: 123456, 15: 500008}),
    'log2_20': dict(L=16, H=16, log2=20, desired=2048 * 1.4),                       # 128 tiles per level: masks dropped
    'log2_14': dict(L=16, H=16, log2=14, desired=2048 * 1.4),                       # 2 tiles per level, 8 slices each
    'L1': dict(L=1, H=16, log2=19, desired=None),
    'L2': dict(L=2, H=16, log2=19, desired=2048 * 1.4),
    'L5': dict(L=5, H=16, log2=19, desired=2048 * 1.4),
    'big_L15': dict(L=15, H=64, log2=22, desired=4096),                             # 61 440 tile-jobs: the largest tiled launch
    'big_L16': dict(L=16, H=64, log2=22, desired=4096),                             # 65 536: falls back to the scatter kernel
}


def layout_offsets(name, with_scale=False):
    """-> (offsets int32 [L+1], S, H) of a named layout; with_scale: also the per-level scale the module is built with."""
    from occnerf_amd.gridencoder import grid_offsets
    spec = LAYOUTS[name]
    off, pls = grid_offsets(4, spec['L'], 2.0, spec['H'], spec['log2'], desired_resolution=spec['desired'])
    if 'resize' in spec:
        sizes = np.diff(off.astype(np.int64))
        for level, size in spec['resize'].items():
            sizes[level] = size
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    if with_scale:
        return off, float(np.log2(pls)), spec['H'], float(pls)
    return off, float(np.log2(pls)), spec['H']


# ---- seeded inputs -----------------------------------------------------------------------------------------------------
RUN_LENGTHS = (2, 63, 64, 65, 129, 700, 5000)


def run_lengths(x):
    """Lengths of the maximal runs of consecutive bitwise identical rows of x (what grid_grad_runs merges, chunk by chunk)."""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32)
    heads = np.flatnonzero(np.r_[True, (bits[1:] != bits[:-1]).any(1)])
    return np.diff(np.r_[heads, len(bits)])


def training_like_inputs(B, seed, D=4):
    """What the training step feeds the encoder, in small: half the rows clustered within 0.002 of an in-range point, a
    quarter of them sharing the last coordinate, runs of bitwise identical rows across the 64- and 512-sample boundaries,
    ~1 % of the rows out of range, rows at exactly 0.0 and 1.0 on every axis, -0.0 inputs."""
    rng = np.random.default_rng(seed)
    x = rng.random((B, D), dtype=np.float32)
    centre = np.array([0.673, 0.412, 0.0203, 0.52], np.float32)[:D - 1]
    x[:B // 2, :D - 1] = centre + 0.002 * rng.standard_normal((B // 2, D - 1)).astype(np.float32)
    x[:B // 4, D - 1] = 0.31
    x[7::97, 1] = 1.5                                            # out of range (after the clustering, BEFORE the runs: a run
    x[11::389, D - 1] = -0.25                                    # overwrites the stamps inside its span and stays whole)
    pos = B // 2 - 100                                          # the first runs copy clustered rows, the later ones uniform rows
    for ln in RUN_LENGTHS:
        assert pos + ln + 64 < B, 'batch too small for the runs'
        x[pos:pos + ln] = np.clip(x[pos], 0.0, 1.0)             # (an in-range head)
        pos += ln + 3
    e = B - 40                                                  # edges: the last rows
    x[e], x[e + 1], x[e + 2] = 0.0, 1.0, -0.0
    for d in range(D):
        x[e + 3 + d, d], x[e + 3 + D + d, d], x[e + 3 + 2 * D + d, d] = 0.0, 1.0, -0.0
    runs = run_lengths(x)
    assert set(RUN_LENGTHS) <= set(runs.tolist()) and runs.max() == max(RUN_LENGTHS), sorted(set(runs.tolist()))[-8:]
    oob = ((x < 0) | (x > 1)).any(1).mean()
    assert 0.008 <= oob <= 0.015, oob
    return x


def training_like_grads(L, B, C, seed):
    """-> rows [B, L*C] as autograd hands them to the module's backward (the operator's [L, B, C] is
    rows.reshape(B, L, C).transpose(1, 0, 2)): normal entries, every 11th row exactly zero (samples the compositor masks
    out), rows with exactly ONE zero channel -- (0, g), (g, 0), (-0.0, g) -- which must contribute, and -0.0 rows."""
    rng = np.random.default_rng(seed + 1000)
    g = rng.standard_normal((B, L, C)).astype(np.float32)
    g[5::11] = 0.0
    g[3::7, :, 0] = 0.0
    g[4::7, :, C - 1] = 0.0
    g[9::31, :, 0] = -0.0
    g[6::53] = -0.0
    return g.reshape(B, L * C)
