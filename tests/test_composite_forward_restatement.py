"""CPU: keeps tests/composite_forward_restatement.py honest without a GPU -- the truth, the error weights and the check that
tests/test_u_composite_forward_per_entry.py holds composite_kernel to:

    the weights E dominate the fp32 reference's error on every case of step_backward_cases.composite_case: rho_ref is finite
    on every kind of ray and flat over the sample counts on the random rows (so 4 max(rho_ref, 1) is a small count of
    roundings, never vacuous);
    the share of random rays whose term the margin leaves undecided is at most 10 %, for the fp32 reference too;
    a forward that is right in another way (em moved by one ulp on the saturated ray) passes;
    four wrong forwards fail, each on a named entry.

Seen here: rho_ref of the random rows 0.17, 0.77, 0.54, 0.52, 0.69, 0.54, 0.55, 0.55, 0.54 at S = 1, 2, 63, 64, 65, 128, 129,
192, 256; at most 0.55 on every special kind; no random ray's term undecided."""
import numpy as np
import pytest
import torch

from tests import composite_forward_restatement as cf
from tests import step_backward_cases as cases

_memo = {}


def _case(S, bg=0):
    if (S, bg) not in _memo:
        c = cases.composite_case(S, cases.BACKGROUNDS[bg])
        _memo[S, bg] = (c, cf.composite_forward_float64(c), cf.forward_torch(c, torch.float32))
    return _memo[S, bg]


def test_forward_reference_ratio_over_S():
    """rho_ref per (S, background, kind): finite everywhere, at most 4 on every kind, and flat on the random rows -- within 4x
    between S = 1 and S = 256 and 6x over all S.  The fp32 numpy forward with a serial product passes the check at every S, and
    the reference's own term obeys the rule with at most 10 % of the random rays undecided."""
    base = {}
    for bg in (0, 1):
        for S in cases.COMPOSITE_S:
            c, ref, r32 = _case(S, bg)
            got = cf.forward_numpy32(c)
            seen = cf.check_forward(f'numpy fp32 S={S} bg={bg}', c, got, ref, r32)
            seen32 = cf.check_forward(f'torch fp32 S={S} bg={bg}', c, r32, ref, r32)
            assert set(seen) == set(cases.KINDS) | {'random', 'term undecided share'}
            assert all(np.isfinite(v[0]) and v[0] <= 4.0 for k, v in seen.items() if k != 'term undecided share'), seen
            assert seen['term undecided share'] <= 0.10 and seen32['term undecided share'] <= 0.10
            base[S, bg] = seen['random'][0]
    print('rho_ref of the random rows:', {k: round(v, 3) for k, v in base.items()})
    for bg in (0, 1):
        assert max(base[256, bg], base[1, bg]) <= 4.0 * min(base[256, bg], base[1, bg]), base
    assert max(base.values()) <= 6.0 * min(base.values()), base


def test_forward_truth_is_raw2outputs_and_weights_bound_it():
    """acc = sum w, depth = sum w z, rgb = sum w c + (1 - acc) bg / 255 of the restated float64 terms equal raw2outputs' float64
    outputs to 1e-12 of their absolute sums; E is positive wherever an output can be non-zero, zero on the mask = 0 ray's
    weights."""
    from tests.step_backward_restatement import composite_running_weights
    for S in (1, 65, 256):
        c, ref, _ = _case(S)
        rw = composite_running_weights(c)
        w, col, z = rw['w'], rw['col'], np.asarray(c['z'], np.float64)
        bg = np.asarray(c['bg'], np.float64)
        assert np.all(np.abs(w.sum(1) - ref['acc']) <= 1e-12 * np.abs(w).sum(1))
        assert np.all(np.abs((w * z).sum(1) - ref['depth']) <= 1e-12 * np.abs(w * z).sum(1))
        rgb = (w[..., None] * col).sum(1) + (1.0 - ref['acc'])[:, None] * bg / 255.0
        assert np.all(np.abs(rgb - ref['rgb']) <= 1e-12 * (np.abs(w).sum(1)[:, None] + 1.0))
        assert np.all(ref['E_w'] >= np.abs(w)) and not ref['E_w'][4].any() and not ref['w'][4].any()
        assert np.all(ref['E_acc'] >= np.abs(ref['acc'])) and np.all(ref['E_depth'] >= np.abs(ref['depth']))


def test_forward_one_ulp_of_em_on_the_saturated_ray_passes():
    for S in (2, 64, 129):
        c, ref, r32 = _case(S)
        cf.check_forward(f'em + ulp S={S}', c, cf.forward_numpy32(c, 'ulp'), ref, r32)


@pytest.mark.parametrize('mutant,S,entry', [('scan', 65, 'sample 64 weights'), ('carry', 129, 'weights'), ('eps', 64, 'ray 5 '),
                                            ('last', 64, 'sample 63 weights')])
def test_forward_wrong_answers_are_refused(mutant, S, entry):
    """scan: the second chunk's transmittance taken inclusive (S = 65: sample 64 alone); carry: the running product dropped at
    the chunk boundaries (S = 129); eps: 1e-10 omitted (the alpha = 1 ray 5: everything behind its middle sample becomes 0);
    last: the last sample's dist 0 instead of 1e10.  Each fails, and the message names the entry."""
    c, ref, r32 = _case(S)
    with pytest.raises(AssertionError, match=entry) as e:
        cf.check_forward(f'mutant {mutant} S={S}', c, cf.forward_numpy32(c, mutant), ref, r32)
    print(f'refused {mutant}: {str(e.value)[:300]}')
