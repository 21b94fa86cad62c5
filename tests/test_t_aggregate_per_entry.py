"""GPU: agg_forward_kernel, agg_runs_kernel and agg_backward_tiled_kernel (occnerf_amd/csrc/aggregate.hip) PER ENTRY against
float64 of the operands each launch read (tests/aggregate_restatement.py, with the counted bounds derived there):

    forward    |got - sum_j t_j| <= gamma_k A with the fp32 terms t_j restated bit for bit and k counted from the code
               (pair branch (ceil(K / 3) - 1) + (min(K, 3) - 1), generic branch K - 1); K = 1 and dyadic operands bit-equal; rows
               of equal (ids, weight bits) bit-equal to each other; one other weight bit: no copy;
    backward   |got - truth| <= gamma_{W+1} A + n 2^-53 A under every slice count W; a point without terms exactly zero in
               every one of the W partial tables; a point named once by a run of one sample equal to fl32(w g).

No norm over a tensor, no tolerance relative to the largest entry, no entry left out; agg, partial and scratch are over-allocated
by 256 bytes of fill that must survive.  Each test prints what it saw; the worst values seen on an MI355X stand in the
docstrings."""
import numpy as np
import pytest
import torch

from tests import aggregate_cases as cases
from tests import aggregate_restatement as ar
from tests.gpu_util import T, same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FILL, PAD = -7.5, 64                                      # 64 floats: 256 bytes behind every buffer


def _forward(c):
    """occnerf_agg_forward into N F + 64 filled floats -> agg [N, F]."""
    from occnerf_amd import _lib, ops
    N, K, F = c['N'], c['K'], c['F']
    feats, knn, atts = T(c['feats']), T(c['knn']), T(c['atts'])
    agg = torch.full((N * F + PAD,), FILL, device=DEV)
    with ops._guard(feats):
        rc = _lib.lib().occnerf_agg_forward(feats.data_ptr(), F, knn.data_ptr(), atts.data_ptr(), N, K, agg.data_ptr(), ops._stream(feats))
    _lib.check(rc, 'agg_forward')
    torch.cuda.synchronize()
    a = agg.cpu().numpy()
    assert np.all(a[N * F:] == FILL), f'agg_forward {c["name"]}: the fill behind agg must survive'
    return a[:N * F].reshape(N, F)


def _backward_buffers(c, W):
    from occnerf_amd import _lib
    nbytes = int(_lib.lib().occnerf_agg_backward_scratch_bytes(c['N'], c['F']))
    assert nbytes == ((c['N'] * c['F'] * 4 + 255) & ~255) + c['N'] * 4
    partial = torch.full((W * c['P'] * c['F'] + PAD,), FILL, device=DEV)
    scratch = torch.full((nbytes + 256,), 0xA5, device=DEV, dtype=torch.uint8)
    return partial, scratch, nbytes


def _call_backward(c, partial, scratch, nbytes, P=None, K=None):
    from occnerf_amd import _lib, ops
    gout, knn, atts = T(c['gout']), T(c['knn']), T(c['atts'])
    with ops._guard(gout):
        rc = _lib.lib().occnerf_agg_backward(gout.data_ptr(), c['F'], knn.data_ptr(), atts.data_ptr(), c['N'], c['K'] if K is None else K,
                                             c['P'] if P is None else P, partial.data_ptr(), scratch.data_ptr(), nbytes, ops._stream(gout))
    torch.cuda.synchronize()
    return rc


def _backward(c):
    """occnerf_agg_backward under the case's slice knob -> (total [P, F] as ops.agg_backward sums it, partial [W, P, F])."""
    from occnerf_amd import _lib
    N, F, P = c['N'], c['F'], c['P']
    try:
        if c['forced']:
            assert _lib.lib().occnerf_experiment_knob(b'agg_slices', c['forced']) >= 0
        W = int(_lib.lib().occnerf_agg_backward_slices(N))
        assert (W, ) == ar.slices_and_per(N, c['forced'])[:1]
        partial, scratch, nbytes = _backward_buffers(c, W)
        _lib.check(_call_backward(c, partial, scratch, nbytes), 'agg_backward')
    finally:
        if c['forced']:
            _lib.lib().occnerf_experiment_knob(b'agg_slices', 0)
    assert np.all(partial[W * P * F:].cpu().numpy() == FILL), f'agg_backward {c["name"]}: the fill behind partial must survive'
    assert np.all(scratch[nbytes:].cpu().numpy() == 0xA5), f'agg_backward {c["name"]}: the fill behind scratch must survive'
    tables = partial[:W * P * F].reshape(W, P, F)
    return tables.sum(0).cpu().numpy(), tables.cpu().numpy()


# ---- forward ------------------------------------------------------------------------------------------------------------
def test_agg_forward_pair_branch():
    """F in {1, 2, 35, 36} x K in {1, 2, 3, 40, 64} (odd F: the `two == false` lane; K = 1, 2: empty groups; K = 64: the
    accepted limit of the branch), N through 1, 7, 8, 9, 63, 64, 65, 2003, and every such N at F = 35, K = 40.
    MI355X: worst error / bound 0.991 (F = 35, K = 2, k = 1: one rounding, half an ulp of the sum against u A); at most 0.20 at
    K = 40 (k = 15) and 0.084 at K = 64 (k = 23); K = 1 bit-equal; every row of equal (ids, weight bits) bit-equal, no copy of row 4."""
    worst = [ar.check_forward(c['name'], c, _forward(c)) for c in cases.forward_cases()[:28]]
    print(f'pair branch: worst error / bound {max(worst):.3f} over {len(worst)} cases')


def test_agg_forward_generic_branch():
    """F in {37, 64} x K in {40, 64}: one trip of the j0 loop, with the copy of equal neighbours; K in {65, 130} at F = 35 and 64:
    two and three trips, no copy.
    MI355X: worst error / bound 0.108 (F = 37, K = 40, k = 39); 0.072 at K = 65 and 0.041 at K = 130."""
    worst = [ar.check_forward(c['name'], c, _forward(c)) for c in cases.forward_cases()[28:36]]
    print(f'generic branch: worst error / bound {max(worst):.3f} over {len(worst)} cases')


def test_agg_forward_dyadic_is_bit_equal():
    """Weights 2^-e, features k / 64: every partial sum exact, so both branches give the exact sum whatever their order.
    MI355X: all five cases (pair K = 40, 64; generic K = 40, 65, 130) bit-equal."""
    done = cases.forward_cases()[36:]
    assert len(done) == 5 and all(c['dyadic'] for c in done)
    for c in done:
        ar.check_forward(c['name'], c, _forward(c))


def test_agg_forward_through_ops_is_the_same_launch():
    """ops.aggregate's forward gives the bits of the guarded call."""
    from occnerf_amd import ops
    c = cases.forward_case(35, 40, 2003)
    got = ops.aggregate(T(c['feats']), T(c['knn']), T(c['atts']))
    torch.cuda.synchronize()
    same(got.cpu().numpy().view(np.uint32), _forward(c).view(np.uint32), 'ops.aggregate forward')


# ---- backward -----------------------------------------------------------------------------------------------------------
def _check_backward(c):
    total, tables = _backward(c)
    return ar.check_backward(c['name'], c, total, tables)


def test_agg_backward_F_by_K():
    """F in {1, 18, 19, 35, 36, 64} x K in {1, 3, 40, 64} (K = 64: the accepted limit) at N = 200: P less than a tile, exactly
    one tile, one tile + 1 (a last tile of one row); ids tile_points - 1 and tile_points in one list, an id twice in a list, a
    list inside one tile, a list over all tiles; runs across the 8- and 64-sample boundaries, a zero row inside a run, a run of
    zero rows.
    MI355X: worst error / bound 0.800 over the 24 cases (F = 35, K = 1: W + 1 = 2 roundings counted, one met); every unnamed point
    zero in the partial table, the point named once equal to fl32(w g)."""
    worst = [_check_backward(c) for c in cases.backward_grid()]
    print(f'F x K: worst error / bound {max(worst):.3f} over {len(worst)} cases')


def test_agg_backward_32_tiles_are_accepted():
    """Exactly 32 point tiles, F = 64 with P = 9216 and F = 35 with P = 16832: the per-sample tile mask's last bit.
    MI355X: accepted; worst error / bound 0.722 and 0.716."""
    for c in cases.backward_limits():
        assert c['tiles'] == 32
        _check_backward(c)


def test_agg_backward_slices():
    """W = 2 (N = 3073, the second slice from sample 1600, the run lengths of tests/test_f_train.py with a run of 1000 across
    the slice boundary), W = 3 (N = 6145), W = 5 forced by the agg_slices knob at N = 130: slices 3 and 4 start beyond N and
    write zeros.  The same per-entry bound under every W; ops.agg_backward gives the bits of the guarded call.
    MI355X: worst error / bound 0.607 (W = 2), 0.601 (W = 3), 0.328 (W = 5); the empty slices' tables all zero."""
    from occnerf_amd import ops
    for c in cases.backward_slices():
        _check_backward(c)
    c = cases.backward_slices()[0]
    got = ops.agg_backward(T(c['gout']), T(c['knn']), T(c['atts']), c['P'])
    torch.cuda.synchronize()
    same(got.cpu().numpy().view(np.uint32), _backward(c)[0].view(np.uint32), 'ops.agg_backward')


def test_agg_backward_refusals_by_name():
    """33 point tiles (P = 9217 at F = 64) and K = 65 are refused on the host, by name, before any launch: partial and scratch
    keep their fill throughout."""
    from occnerf_amd import _lib
    c = cases.backward_limits()[0]
    for kw, msg in (({'P': 9217}, r'agg_backward: 33 point tiles of 288 rows for P=9217, F=64: at most 32'),
                    ({'K': 65}, r'agg_backward: F=64 \(1\.\.64\), K=65 \(1\.\.64\)')):
        partial, scratch, nbytes = _backward_buffers(dict(c, P=9217), 1)
        rc = _call_backward(c, partial, scratch, nbytes, **kw)
        with pytest.raises(RuntimeError, match=msg):
            _lib.check(rc, 'agg_backward')
        assert bool((partial == FILL).all()) and bool((scratch == 0xA5).all()), f'refused {kw}: nothing may have been written'
        print(f'refused {kw}: {_lib.lib().occnerf_last_error().decode()}')
