"""CPU: the float64 restatement of the grid encoder's backward (tests/encoder_backward_restatement.py) against the C oracle
(oracle/occnerf_oracle.c oc_grid_encode_backward*), the second opinion the oracle's backward did not have.  Every term is
bit-identical on both sides, so the oracle's serial fp32 sum must lie within gamma_{n-1} A of the float64 sum per cell, and
cells with a single term must be bit-equal.  tests/test_d_encoder_backward.py holds the HIP kernels to the same restatement."""
import numpy as np
import pytest

from tests import encoder_backward_cases as cases
from tests import encoder_backward_restatement as ebr
from tests.test_encoder_restatement import F32

DEFAULT = dict(D=4, L=16, pls=2.0, H=16, log2=19, desired=2048 * 1.4)


def _layout(D=4, L=16, pls=2.0, H=16, log2=19, desired=None, align=False):
    from occnerf_amd.gridencoder import grid_offsets
    off, pls = grid_offsets(D, L, pls, H, log2, desired_resolution=desired, align_corners=align)
    return off, float(np.log2(pls)), H


def test_backward_restatement_equals_the_c_oracle_d4c2_contended(oracle):
    """The renderer's encoder (D = 4, C = 2, 2 dense + 14 hashed levels) on a training-like 40 000-sample input: 39 000+
    rows in range, the fullest cell collects thousands of terms.  Oracle within gamma_{n-1} A of the float64 sum on every
    cell, bit-equal where n = 1; the sparse form of the restatement agrees with the dense one.
    Measured: worst error / bound 1.000 (cells of two terms can use the whole of gamma_1 A), fullest cell 11 203 terms."""
    off, S, H = _layout(**DEFAULT)
    B, L, C = 40000, 16, 2
    x = cases.training_like_inputs(B, 5)
    g = cases.training_like_grads(L, B, C, 5).reshape(B, L, C).transpose(1, 0, 2).copy()
    inr = int((~((x < 0) | (x > 1)).any(1)).sum())
    assert 0.97 * B < inr < B and int((~((x[:B // 2] < 0) | (x[:B // 2] > 1)).any(1)).sum()) > 0.97 * (B // 2)
    ssum, A, n = ebr.backward_numpy(g, x, off, C, S, H)
    assert n.max() >= 5000 and n.sum() == inr * 16 * L
    ge, _ = oracle.grid_encode_backward(g, x, off, int(off[-1]), C, S, H)
    worst = ebr.check('C oracle, D = 4 C = 2', ge, ssum, ebr.bound_serial(A, n), n)
    assert worst <= 1.0
    idx, s2, a2, n2 = ebr.backward_numpy_sparse(g, x, off, C, S, H)
    assert np.array_equal(idx, np.flatnonzero(n)) and np.array_equal(n2, n[idx])
    assert (np.abs(s2 - ssum[idx]) <= ebr.U64 * n[idx, None] * A[idx]).all()          # two float64 sums in different orders
    assert (np.abs(a2 - A[idx]) <= ebr.U64 * n[idx, None] * A[idx]).all()


@pytest.mark.parametrize('D,C,gridtype,interp,align', [(3, 2, 0, 1, False), (3, 4, 1, 0, True), (2, 8, 0, 0, False), (5, 2, 0, 0, False),
                                                       (4, 1, 1, 1, True)])
def test_backward_restatement_equals_the_c_oracle_generic(oracle, D, C, gridtype, interp, align):
    """The generic instantiations the forward restatement lists (tiled grids, smoothstep, align_corners, D = 2..5), with
    out-of-range rows, rows on cell corners and a contended cluster."""
    rng = np.random.RandomState(D * 10 + C)
    L = 8
    off, S, H = _layout(D, L, 1.6, 4, 12, align=align)
    B = 3000
    x = rng.uniform(0, 1, (B, D)).astype(F32)
    x[0], x[1], x[2], x[4] = 0.0, 1.0, -1e-6, 0.5
    x[3, -1] = 1.0 + 1e-6
    x[5:40] = np.round(x[5:40] * 8) / 8
    x[1000:2000] = x[1000] + 0.001 * rng.randn(1000, D).astype(F32)
    x[1000:2000] = np.clip(x[1000:2000], 0, 1)
    g = rng.randn(L, B, C).astype(F32)
    g[:, 7::13, 0] = 0.0
    ssum, A, n = ebr.backward_numpy(g, x, off, C, S, H, gridtype, align, interp)
    assert n.max() >= 500
    ge, _ = oracle.grid_encode_backward(g, x, off, int(off[-1]), C, S, H, None, gridtype, align, interp)
    ebr.check(f'C oracle, D = {D} C = {C}', ge, ssum, ebr.bound_serial(A, n), n)


@pytest.mark.parametrize('D,C,gridtype,interp,align', [(4, 2, 0, 0, False), (3, 4, 1, 1, True), (2, 1, 0, 0, False)])
def test_backward_restatement_float64_dispatch(oracle, D, C, gridtype, interp, align):
    """scalar_t = double: the term is `double(w) * g` rounded once to float64 (w the fp32 corner weight); the oracle's serial
    float64 sum lies within n 2^-53 A of the restatement's extended-precision sum, per cell."""
    assert np.finfo(np.longdouble).nmant >= 63
    rng = np.random.RandomState(D * 100 + C)
    L = 6
    off, S, H = _layout(D, L, 1.7, 4, 11, align=align)
    B = 4000
    x = rng.uniform(0, 1, (B, D)).astype(F32)
    x[0], x[1], x[2] = 0.0, 1.0, -1e-6
    x[2000:] = np.clip(x[2000] + 0.001 * rng.randn(B - 2000, D), 0, 1).astype(F32)
    g = rng.randn(L, B, C)
    idx, ssum, A, n = ebr.backward_numpy_sparse(g, x, off, C, S, H, gridtype, align, interp, f64_terms=True)
    assert n.max() >= 1000
    ge, _ = oracle.grid_encode_backward_f64(g, x, off, int(off[-1]), C, S, H, None, gridtype, align, interp)
    rest = np.ones(int(off[-1]), bool)
    rest[idx] = False
    assert not ge[rest].any()
    ebr.check(f'C oracle float64, D = {D} C = {C}', ge[idx], ssum, ebr.bound_f64(A, n), n, bit_equal_single=False)
    one = n == 1
    assert np.array_equal(ge[idx][one], ssum[one])


@pytest.mark.parametrize('D,C,gridtype,interp,align', [(4, 2, 0, 0, False), (3, 4, 1, 1, True), (5, 2, 0, 0, False)])
def test_input_gradient_restatement(oracle, D, C, gridtype, interp, align):
    """gi[b, d] = sum_{l, c} grad[l, b, c] dy_dx[b, l, d, c]: the oracle's float32 result is this file's fp32 chain bit for
    bit and within gamma_{LC} sum|terms| of the float64 sum; the float64 case (one fma per term) within LC 2^-53 sum|terms|."""
    rng = np.random.RandomState(D + 7 * C)
    L = 8
    off, S, H = _layout(D, L, 1.6, 4, 12, align=align)
    B = 1500
    x = rng.uniform(0, 1, (B, D)).astype(F32)
    x[0], x[1], x[2] = 0.0, 1.0, -1e-6
    emb = rng.uniform(-1, 1, (int(off[-1]), C)).astype(F32)
    g = rng.randn(L, B, C).astype(F32)
    _, dy = oracle.grid_encode_forward(x, emb, off, S, H, True, gridtype, align, interp)
    _, gi = oracle.grid_encode_backward(g, x, off, int(off[-1]), C, S, H, dy, gridtype, align, interp)
    want, mag = ebr.input_grad_numpy(g, dy, D)
    assert np.array_equal(gi.view(np.uint32), ebr.input_grad_chain32(g, dy, D).view(np.uint32))
    assert (np.abs(gi - want) <= ebr.gamma(L * C) * mag).all() and not gi[2].any()
    g64 = rng.randn(L, B, C)
    _, dy64 = oracle.grid_encode_forward_f64(x, emb.astype(np.float64), off, S, H, True, gridtype, align, interp)
    _, gi64 = oracle.grid_encode_backward_f64(g64, x, off, int(off[-1]), C, S, H, dy64, gridtype, align, interp)
    want64, mag64 = ebr.input_grad_numpy(g64, dy64, D)
    assert (np.abs(gi64 - want64) <= 2 * L * C * ebr.U64 * mag64).all()        # (both sides sum LC terms in float64)


def test_level_layouts_reach_their_branches():
    """The level layouts tests/test_d_encoder_backward.py runs, through the host's own rule (make_grid_modes_d4 and the
    tile-job count of grid_backward_impl): index modes, tiles per level and tile-jobs, so that a layout cannot silently stop
    reaching the branch it is there for."""
    LAYOUTS, layout_offsets = cases.LAYOUTS, cases.layout_offsets
    want = {
        'default': ('DD' + 'P' * 14, [11, 41] + [64] * 14, 8000),
        'generic': ('DDPGPPGPPPPPPPPG', None, 7384),
        'log2_20': ('DD' + 'P' * 14, [11, 41] + [128] * 14, 15168),
        'log2_14': ('P' * 16, [2] * 16, 256),
        'L1': ('D', [11], 176),
        'L2': ('DP', None, 688),
        'L5': ('DPPPP', [11, 64, 64, 64, 64], 2224),
        'big_L15': ('P' * 15, [512] * 15, 61440),
        'big_L16': ('P' * 16, [512] * 16, 65536),
    }
    assert set(want) == set(LAYOUTS)
    for name, (modes, tiles, jobs) in want.items():
        off, S, H = layout_offsets(name)
        m, t, _, j = cases.tile_jobs(off, S, H)
        assert modes is None or m == modes, (name, m)
        assert tiles is None or t == tiles, (name, t)
        assert jobs is None or j == jobs, (name, j)
    off, S, H = layout_offsets('generic')
    _, t, _, _ = cases.tile_jobs(off, S, H)
    assert (t[3], t[6], t[15]) == (37, 16, 62)
