"""CPU: keeps tests/aggregate_restatement.py honest without a GPU -- the truth, the counted bounds and the checks that
tests/test_t_aggregate_per_entry.py holds the three aggregation kernels to:

    the numpy emulation of both forward summation orders and of the backward's two roundings stays inside the counted bounds
    on every case, and is bit-equal on the dyadic cases;
    the truth equals torch's float64 gather + sum and its autograd;
    five wrong answers, made by the emulation, fail the per-entry check on a named entry -- and the test prints which of them
    the tolerances of tests/test_f_train.py::test_aggregate_autograd (2e-6 on the forward, 2e-6 of the largest gradient entry
    on the backward) let through: the gap these tests close."""
import numpy as np
import pytest
import torch

from tests import aggregate_cases as cases
from tests import aggregate_restatement as ar

_memo = {}


def _backward_cases():
    if 'b' not in _memo:
        _memo['b'] = cases.backward_grid() + cases.backward_limits() + cases.backward_slices()
    return _memo['b']


def test_forward_count_of_additions():
    """k from the code: 0, 1, 2, 15, 23 on the pair branch at K = 1, 2, 3, 40, 64; K - 1 on the generic branch."""
    assert [ar.forward_k(35, K) for K in cases.PAIR_K] == [0, 1, 2, 15, 23]
    assert [ar.forward_k(F, K) for F, K in cases.GENERIC] == [39, 63, 39, 63, 64, 129, 64, 129]
    assert ar.pair_branch(36, 64) and not ar.pair_branch(37, 64) and not ar.pair_branch(36, 65)


def test_forward_emulation_stays_inside_the_counted_bound():
    """Both summation orders on every forward case; the dyadic cases and K = 1 bit-equal."""
    worst = [ar.check_forward(c['name'], c, ar.forward_emulate(c)) for c in cases.forward_cases()]
    assert max(worst) <= 1.0 and len(worst) == 20 + 8 + 8 + 5


def test_backward_emulation_stays_inside_the_counted_bound():
    """The run sums, the per-slice cells and the sum of the partial tables on every backward case, with the exact duties."""
    for c in _backward_cases():
        W, per = ar.slices_and_per(c['N'], c['forced'])
        total, partial = ar.backward_emulate(c)
        assert ar.check_backward(c['name'], c, total, partial) <= 1.0
    by = {c['name']: c for c in _backward_cases()}
    assert ar.slices_and_per(3073) == (2, 1600) and ar.slices_and_per(6145) == (3, 2112) and ar.slices_and_per(130, 5) == (5, 64)
    assert [c['tiles'] for c in cases.backward_limits()] == [32, 32] and cases.tile_points(18) == 1024 and cases.tile_points(19) == 970
    assert sorted({c['tiles'] for c in cases.backward_grid()}) == [1, 2]
    assert any(c['P'] == c['tile_points'] + 1 for c in by.values())


def test_truth_is_torch_float64_gather_sum_and_autograd():
    """(atts[..., None] * feats[knn]).sum(1) in float64 and its gradient for an upstream gout, to 1e-12 of the absolute sums (the
    forward truth adds fp32-rounded terms: within their one rounding, u A, of torch's unrounded ones)."""
    for c in (cases.forward_case(35, 40, 65), cases.forward_case(64, 130, 9)):
        ssum, A = ar.forward_truth(c)
        want = (torch.from_numpy(c['atts']).double()[..., None] * torch.from_numpy(c['feats']).double()[torch.from_numpy(c['knn']).long()]).sum(1)
        assert np.all(np.abs(ssum - want.numpy()) <= ar.U32 * A)
    for c in (cases.backward_grid()[3], cases.backward_slices()[0]):
        ssum, A, n = ar.backward_truth(c)
        f = torch.zeros(c['P'], c['F'], dtype=torch.float64, requires_grad=True)
        out = (torch.from_numpy(c['atts']).double()[..., None] * f[torch.from_numpy(c['knn']).long()]).sum(1)
        g, = torch.autograd.grad(out, f, torch.from_numpy(c['gout']).double())
        assert np.all(np.abs(ssum - g.numpy()) <= 1e-12 * A)
        assert np.array_equal(n, np.bincount(c['knn'].reshape(-1), minlength=c['P']))


def _old_forward_ok(got, want):
    return float(np.abs(got.astype(np.float64) - want).max()) <= 2e-6


def _old_backward_ok(got, want):
    return float(np.abs(got.astype(np.float64) - want).max()) <= 2e-6 * float(np.abs(want).max())


def test_wrong_answers_are_refused():
    """Each mutant fails the per-entry check on a named entry; at least one of them passes the old tolerances."""
    let_through = []
    # a predecessor's row copied when only one weight bit differs
    c = cases.forward_case(35, 40, 65)
    got = ar.forward_emulate(c, 'copy')
    with pytest.raises(AssertionError, match='row 5 column') as e:
        ar.check_forward('mutant copy', c, got)
    print('refused copy:', str(e.value)[:200])
    if _old_forward_ok(got, ar.forward_truth(c)[0]):
        let_through.append('copy')
    # the backward's four
    c = cases.backward_slices()[0]
    truth = ar.backward_truth(c)
    assert ar.check_backward('no mutant', c, *ar.backward_emulate(c), truth=truth) <= 1.0
    p_once, tp = 5, c['tile_points']
    for mutant, entry in (('drop', f'point {p_once} '), ('boundary', fr'point ({tp - 1}|{tp}) '), ('slice', 'point 7 '), ('head', 'point')):
        total, partial = ar.backward_emulate(c, mutant)
        with pytest.raises(AssertionError, match=entry) as e:
            ar.check_backward(f'mutant {mutant}', c, total, partial, truth=truth)
        print(f'refused {mutant}:', str(e.value)[:200])
        if _old_backward_ok(total, truth[0]):
            let_through.append(mutant)
    print('wrong answers the old tolerances let through:', let_through)
    assert 'drop' in let_through
