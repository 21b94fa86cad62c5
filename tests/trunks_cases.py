"""Inputs of the per-entry trunk tests (tests/test_n_trunks_per_entry.py, tests/test_trunks_restatement.py), built from seeds.
numpy only: every array is float64 holding values that are exact in the flavour's storage format (bf16 or fp32), so the
GPU test's conversion to the device type loses nothing and the restatement sees the bits the kernel reads.

Random operands: rows N(0,1), weights N(0,1/K) (outputs of order 1, the scale at which the share of entries whose interval
admits two bf16 values was measured); dyadic twins: small integers, every product and partial sum an integer below 2^24."""
import numpy as np

from tests import trunks_restatement as tr

# M: one row, both sides of the 32-row wave and of the 128-row workgroup of linear_kernel, a third workgroup with one row
LINEAR_M = (1, 31, 32, 33, 127, 128, 129, 257)
# the ten launch forms of the step (+ the masked fp32 store that no launch of the step uses: in bf16 the direct-store path)
FORMS = {
    'pts_linears.0': dict(k0=96, n=256, bias=True, relu=True),
    'hidden': dict(k0=256, n=256, bias=True, relu=True),                      # one 256-byte K chunk in fp32 is 64 columns: 4 chunks
    'geo head': dict(k0=256, n=96, bias=True, aux_col=64, aux_stride=4),
    'rgb_linears.0': dict(k0=96, k1=96, n=256, bias=True, relu=True),         # second K segment
    'output layer': dict(k0=256, n=32, bias=True, out_f32=True, n_store=3, out_width=4),
    'dgrad output layer': dict(k0=32, n=256, mask=True),
    'dgrad hidden': dict(k0=256, n=256, mask=True),
    'dgeo': dict(k0=256, n=96, w_rows=192),                                   # the weight is rows :96 of a [192, 256] matrix
    'dX0': dict(k0=256, k1=256, n=96, out_f32=True),
    'masked fp32 store': dict(k0=96, n=96, mask=True, out_f32=True),
}
WGRAD_SHAPES = ((256, 256), (256, 96), (96, 256), (32, 256), (64, 128), (192, 32))      # the last two: waves gated off by nact / kact
WGRAD_M_RANDOM = (1, 33, 129)
# M -> slices G of occnerf_linear_wgrad_slices: one slice; a second slice of one row; the reduce's tail loop (5 = 4 + 1); one
# unrolled trip of the reduce (32 slices) + a tail; two tiles per slice with slice 128 holding one row and 129..255 empty;
# three tiles per slice, ragged end
WGRAD_M_DYADIC = {1: 1, 33: 2, 135: 5, 1025: 33, 8193: 256, 16389: 256}
FUSED_M = (1, 31, 32, 33, 127, 128, 129, 4099)
FILL = -7.0                                                                   # what an output buffer holds before a launch

TINY = 2.0 ** -126                                                            # smallest normal value of bf16 and of fp32


def _seed(*key):
    return sum((i + 1) * sum(map(ord, str(k))) for i, k in enumerate(key))    # (hash() of a str changes from run to run)


def linear_case(form, M, bf16, dyadic):
    """-> dict(x0, x1, W, Wfull, bias, mask) of one linear_forward launch of FORMS[form]; None where the form has none."""
    f = FORMS[form]
    g = np.random.default_rng(_seed('linear', form, M, bf16, dyadic))
    k0, k1, n = f['k0'], f.get('k1', 0), f['n']
    K, wr = k0 + k1, f.get('w_rows', f['n'])
    if dyadic:
        x, W = g.integers(-3, 4, (M, K)).astype(np.float64), g.integers(-2, 3, (wr, K)).astype(np.float64)
        bias = g.integers(-4, 5, n).astype(np.float64) if f.get('bias') else None
    else:
        x, W = tr.rnd(g.standard_normal((M, K)), bf16), tr.rnd(g.standard_normal((wr, K)) / np.sqrt(K), bf16)
        bias = tr.rnd(g.standard_normal(n), False) if f.get('bias') else None
    mask = None
    if f.get('mask'):
        mask = tr.rnd(np.maximum(g.standard_normal((M, n)), 0.0), bf16)
        mask[:, 0] = tr.rnd(mask[:, 0] + 0.5, bf16)                           # (a column that is live in every row)
        mask[0, 1:6] = [-0.0, 0.0, TINY, -TINY, -1.0]
        mask[:, 7] = 0.0                                                      # dead columns
        mask[:, n - 1] = -0.0
    return {'x0': np.ascontiguousarray(x[:, :k0]), 'x1': np.ascontiguousarray(x[:, k0:]) if k1 else None, 'Wfull': W,
            'W': W[:n], 'bias': bias, 'mask': mask}


def wgrad_case(n_pad, k_pad, M, bf16, dyadic):
    """-> dict(dz, x, row_map, col_map, dW_shape, db_shape): maps with holes into a dW with a row and two columns no map reaches;
    row M // 2 and column 7 of dz are all zero."""
    g = np.random.default_rng(_seed('wgrad', n_pad, k_pad, M, bf16, dyadic))
    if dyadic:
        dz, x = g.integers(-2, 3, (M, n_pad)).astype(np.float64), g.integers(-3, 4, (M, k_pad)).astype(np.float64)
    else:
        dz, x = tr.rnd(g.standard_normal((M, n_pad)), bf16), tr.rnd(g.standard_normal((M, k_pad)), bf16)
    dz[M // 2, :] = 0.0
    dz[:, 7] = 0.0
    out_dim, in_dim = n_pad - 3, k_pad - 5
    rows, cols = g.permutation(n_pad), g.permutation(k_pad)
    if rows[7] >= out_dim:                                                    # (the zero column of dz must reach dW)
        j = int(np.flatnonzero(rows == 0)[0])
        rows[j], rows[7] = rows[7], rows[j]
    return {'dz': dz, 'x': x, 'row_map': np.where(rows < out_dim, rows, -1).astype(np.int32),
            'col_map': np.where(cols < in_dim, cols, -1).astype(np.int32), 'dW_shape': (out_dim + 1, in_dim + 2),
            'db_shape': (out_dim + 1,), 'zero_row': int(rows[7])}


# ---- networks ---------------------------------------------------------------------------------------------------------
def random_network(seed=0):
    """-> (W[10], b[10]) float64 holding fp32 values: N(0, 2/in) weights (activations stay of order 1 through the ReLUs)."""
    g = np.random.default_rng(_seed('net', seed))
    Ws = [tr.rnd(g.standard_normal(s) * np.sqrt(2.0 / s[1]), False) for s in tr.SHAPES]
    bs = [tr.rnd(0.1 * g.standard_normal(s[0]), False) for s in tr.SHAPES]
    return Ws, bs


def dyadic_network(seed=0):
    """Ten layers of sparse weights in {-1, 0, 1} and integer biases in {-1, 0, 1}: two non-zeros per row (four in the geometry
    head, 86 in the three colour rows), placed round-robin so that every input column of every layer is used by some row."""
    g = np.random.default_rng(_seed('dyadic net', seed))
    Ws, bs = [], []
    for (out_dim, in_dim) in tr.SHAPES:
        nnz = max(2, -(-in_dim // out_dim))
        W = np.zeros((out_dim, in_dim))
        start = int(g.integers(0, in_dim))
        for r in range(out_dim):
            c = (start + r * nnz + np.arange(nnz)) % in_dim
            W[r, c] = g.choice([-1.0, 1.0], nnz)
        assert np.all(np.abs(W).sum(0) > 0), 'every input column is used'
        Ws.append(W)
        bs.append(g.integers(-1, 2, out_dim).astype(np.float64))
    return Ws, bs


def step_inputs(M, dyadic, seed=0):
    """-> agg[M,35], var[M,1], enc[M,32], gout[M,4] (the upstream gradient of raw4)."""
    g = np.random.default_rng(_seed('step', M, dyadic, seed))
    if dyadic:
        return (g.integers(-1, 2, (M, 35)).astype(np.float64), g.integers(0, 2, (M, 1)).astype(np.float64),
                g.integers(-1, 2, (M, 32)).astype(np.float64), g.integers(-1, 2, (M, 4)).astype(np.float64))
    return (tr.rnd(g.standard_normal((M, 35)), False), tr.rnd(g.random((M, 1)), False),
            tr.rnd(g.standard_normal((M, 32)), False), tr.rnd(g.standard_normal((M, 4)), False))


def assert_dyadic_forward(fw):
    """No stored activation of the dyadic network is rounded: every pre-activation is an integer with |v| <= 256 (bf16 holds
    every such integer), raw4 an integer below 2^24; and no layer is dead."""
    for nm, ts in (('A', fw['acts'][1:]), ('GEO', [fw['GEO']]), ('B', fw['B'])):
        for i, t in enumerate(ts):
            assert np.all(t == np.rint(t)) and np.abs(t).max() <= 256, (nm, i, np.abs(t).max())
            assert tr.is_bf16(t)
            assert np.mean(t != 0) > 0.2, (nm, i, 'a dead layer checks nothing')
    assert np.all(fw['raw4'] == np.rint(fw['raw4'])) and np.abs(fw['raw4']).max() < 2.0 ** 24
