"""CPU: keeps tests/features_restatement.py honest without a GPU -- the truth, the counted bounds and the checks that
tests/test_v_features_per_entry.py holds the feature kernels of occnerf_amd/csrc/features.hip to:

    the fp32 FMA is the rationals' (random operands and operands a hair off a half-way point);
    the bit-exact parts agree with the C oracle where it has the function: the level constants, grid_encode_forward on all three
    index modes, point_table, and canonical_mlp's distance, encoding, variance and (within the counted bound: its expf is libm's)
    aggregate;
    the cases contain every edge they claim;
    the fp32 emulations of both kernels stay inside the derived bounds on every case;
    ten wrong answers, made by the emulations, are refused by the matching check, by name."""
from fractions import Fraction

import numpy as np
import pytest

from tests import features_cases as cases
from tests import features_restatement as fr

F32 = np.float32


def _rn32(v):
    """The float32 nearest to the exact rational v, ties to even."""
    f = F32(float(v))
    best = None
    for cand in (np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))):
        key = (abs(Fraction(float(cand)) - v), int(F32(cand).view(np.int32)) & 1)
        if best is None or key < best[0]:
            best = (key, F32(cand))
    return best[1]


def test_fma32_is_the_rationals():
    """2 000 random triples, 1 800 whose exact a b + c lies beside the middle of two fp32 numbers, and 200 built for double
    rounding: a b = 2^-24 (1 - 2^-2k) under c = 1 + (2 m + 1) 2^-23 lies 2^-(24 + 2k) below the middle, float64 rounds the sum ONTO
    the middle and the tie then goes up to the even neighbour -- the plain float64 evaluation is wrong on every one of them."""
    rng = np.random.RandomState(3)
    a, b = rng.randn(4000).astype(F32), rng.randn(4000).astype(F32)
    c = rng.randn(4000).astype(F32)
    for i in range(2000, 4000):                                                    # c = fl32(middle - a b): the sum lands a hair off the middle
        t = F32(rng.randn())
        mid = (Fraction(float(t)) + Fraction(float(np.nextafter(t, F32(np.inf))))) / 2
        c[i] = _rn32(mid - Fraction(float(a[i])) * Fraction(float(b[i])))
    for i in range(3800, 4000):
        k, sign = rng.randint(15, 23), F32(rng.choice([-1.0, 1.0]))
        a[i], b[i] = sign * F32(2.0 ** -12) * (F32(1) + F32(2.0 ** -k)), F32(2.0 ** -12) * (F32(1) - F32(2.0 ** -k))
        c[i] = sign * (F32(1) + F32(2 * rng.randint(0, 2 ** 22) + 1) * F32(2.0 ** -23))
    want = np.array([_rn32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))) for i in range(4000)], F32)
    got = fr.fma32(a, b, c)
    assert np.array_equal(fr.bits(got), fr.bits(want))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert (fr.bits(naive) != fr.bits(want))[3800:].all() and np.array_equal(fr.bits(want[3800:]), fr.bits(c[3800:]))
    assert fr.fma32(F32(0), F32(-1), F32(0)).view(np.uint32) == 0                  # -0 + +0 = +0


def test_encoding_and_table_agree_with_the_oracle(oracle):
    """Level constants, the three index modes (standard layout: dense + power of two; generic layout: + modulo; host offsets
    NULL: every level through the generic path, the same bits), inputs on cell corners and outside [0, 1]; point_table."""
    rng = np.random.RandomState(4)
    x = rng.uniform(0, 1, (600, 4)).astype(F32)
    x[0], x[1], x[2], x[3, 3], x[4, 0] = 0.0, 1.0, 0.5, 1.0 + 1e-6, -1e-7
    for generic in (False, True):
        lay = cases.layout(generic)
        scale, res = fr.level_params(16, lay['S'], lay['H'])
        o_scale, o_res = oracle.grid_level_params(16, lay['S'], lay['H'])
        assert np.array_equal(fr.bits(scale), fr.bits(o_scale)) and np.array_equal(res, o_res.astype(np.int64))
        want, _ = oracle.grid_encode_forward(x, lay['emb'], lay['offsets'], lay['S'], lay['H'])
        want = want.transpose(1, 0, 2).reshape(len(x), -1)
        got = fr.encode(x, lay)
        assert np.array_equal(fr.bits(got), fr.bits(want)) and not got[3].any() and not got[4].any() and got[2].any()
        assert np.array_equal(fr.bits(fr.encode(x, lay, given=False)), fr.bits(want))
        if generic:
            assert np.array_equal(fr.bits(got[:, :30]), fr.bits(fr.encode(x, cases.layout())[:, :30]))
            assert (fr.bits(fr.encode(x, lay, defect='generic_mask')[:, 30:]) != fr.bits(want[:, 30:])).any()
    m, lay = cases.model(), cases.layout()
    want = oracle.point_table(m['knn_base'], m['sdf'], m['learnable'], cases.BOUND, lay['emb'], lay['offsets'], lay['S'], lay['H'])
    assert np.array_equal(fr.bits(m['table'][:, :35]), fr.bits(want)) and not m['table'][:, 35].any()
    zero = ((m['table_x'] < 0) | (m['table_x'] > 1)).any(1)
    assert zero[5] and zero[6] and not zero[7] and not zero[8] and not m['table'][zero, :32].any() and m['table'][~zero, :32].any(1).all()
    assert (m['table_x'][7, :3] == 1).all() and (m['table_x'][8, :3] == 0).all() and (m['table_x'][:, 3] == 0).any() and (m['table_x'][:, 3] == 1).any()


def test_sample_features_agree_with_the_oracle(oracle):
    """oracle.canonical_mlp (its trunks cut to one zero layer) on the pool: distance, encoding and variance bit for bit -- the
    encoding only if the restated encoder input is the oracle's -- and its aggregate, summed in the one-lane kernel's order with
    libm's expf, inside the one-lane bound."""
    m, lay, pl = cases.model(), cases.layout(), cases.pool()
    zeros = ([np.zeros((65, 68), F32)], [np.zeros(65, F32)], [np.zeros((3, 131), F32)], [np.zeros(3, F32)])
    raw, mi = oracle.canonical_mlp(pl['xyz'], pl['knn'].reshape(-1, 4, 10), m['base'], m['normals'], m['counter'],
                                   np.ascontiguousarray(m['table'][:, :35]), cases.BOUND, lay['emb'], lay['offsets'], lay['S'], lay['H'],
                                   *zeros, want_mlp_in=True)
    worst = fr.check_features('oracle.canonical_mlp', cases.pool_truth(), 'one', mi, raw[:, 4], None, form='the C oracle')
    assert worst <= 1.0


def test_cases_contain_every_edge():
    for P in (257, cases.LDS_POINTS, cases.LDS_POINTS + 1):
        found = cases.edges(P)
        print(f'P = {P}: {found}')
        assert found['x[3] strictly inside (0, 1)'] >= 800 and found['out of range'] == 16
    assert cases.LONG_LDS > 2 * 256 * 96 and cases.LONG_256 > 2 * 8192 * 32 and cases.pool()['D'] <= 4096
    assert {6143, 6144} <= set(cases.N_LANES8) and cases.LDS_MIN_N == 6144
    for cap in (100, 6200):
        lists = dict((n, (r, c)) for n, r, c in cases.row_lists(1200, cap))
        r, c = lists['ascending']
        assert (np.diff(r) >= 0).all() and c == cap
        r, c = lists['unsorted with repeats']
        assert (np.diff(r) < 0).any() and len(np.unique(r)) < len(r)
        r, c = lists['capacity beyond the count']
        assert 1 < c < cap and (r[c:] == cases.SENTINEL).all()
        assert lists['count 1'][1] == 1 and lists['count 0'][1] == 0
        assert all(0 <= r.min() and r.max() < 1200 and r.dtype == np.int32 for r, _ in lists.values())
    cc = cases.centre_case()
    trips = [cc['inside'][a:a + 8] for a in range(0, 75, 8)]
    assert trips[0].all() and trips[1].all() and not trips[2].any() and not trips[3].any() and trips[9].all() and len(trips[9]) == 3
    assert all(0 < t.sum() < 8 for t in trips[4:8])
    one = cases.one_lane_cases()
    assert {(c['nscale'], c['att_in'] is not None, c['geo'] is not None) for c in one} == {(s, a, g) for s in (1, 2, 3, 4) for a in (False, True) for g in (False, True)}
    assert {c['N'] for c in one} == set(cases.N_ONE)


def test_emulations_stay_inside_the_bounds():
    """Both kernels' fp32 emulations on the pool of every model under both layouts, and the one-lane emulation on every one-lane
    case with the host offsets given and NULL (the same bits)."""
    worst = []
    for P, generic in ((257, False), (257, True), (cases.LDS_POINTS, False), (cases.LDS_POINTS + 1, False)):
        m, lay, q, tr = cases.model(P), cases.layout(generic), cases.pool_problem(P), cases.pool_truth(P, generic)
        assert 0.0 < tr['rho'] < 1.0, 'c = 4 max(rho_ref, 1): torch\'s CPU softmax is expected well inside E'
        for kernel in ('one', 'eight'):
            e = fr.emulate(m, lay, q, kernel)
            worst.append(fr.check_features(f'emulated P = {P}{" generic" if generic else ""}', tr, kernel, e['mlp_in'], e['dist'], e['x']))
        sel = cases.whole_map(1200, 6145)                                           # a run longer than the pool: compared by gather
        worst.append(fr.check_features('emulated, by gather', tr, 'eight', e['mlp_in'][sel], e['dist'][sel], e['x'][sel], sel=sel))
    m, lay = cases.model(), cases.layout()
    for c in cases.one_lane_cases():
        tr, e = fr.truth(m, lay, c['q']), fr.emulate(m, lay, c['q'], 'one')
        worst.append(fr.check_features(c['name'], tr, 'one', e['mlp_in'], e['dist'], e['x']))
        assert np.array_equal(fr.bits(fr.emulate(m, lay, c['q'], 'one', given=False)['mlp_in']), fr.bits(e['mlp_in']))
    print(f'worst error / bound of the emulations {max(worst):.3f}')
    assert max(worst) <= 1.0
    assert [fr.agg_rel_bound(40, 'one')[0], fr.agg_rel_bound(40, 'eight')[0]] == [39, 7]
    assert fr.agg_rel_bound(40, 'eight')[1].tolist() == [40] * 32 + [8] * 3 and fr.agg_rel_bound(10, 'one')[1].tolist() == [10] * 35


@pytest.mark.parametrize('defect,kernel,refused', [
    ('skip', 'eight', 'columns 0..34 over their bound'), ('twice', 'one', 'columns 0..34 over their bound'),
    ('lane_weight', 'eight', 'columns 0..34 over their bound'), ('neighbour_tail', 'eight', r'columns 0..34 over their bound.* column 3[234]:'),
    ('var_K', 'eight', 'the variance'), ('var_K', 'one', 'the variance'), ('flip_at_5', 'eight', 'the signed distance'),
    ('no_clamp', 'one', 'the encoder input'), ('oob_untransposed', 'eight', 'the hash encoding'),
    ('oob_not_zeroed', 'eight', 'the hash encoding .* sample 0 '), ('generic_mask', 'eight', r'the hash encoding .* column 3[01]:')])
def test_wrong_answers_are_refused(defect, kernel, refused):
    """Each planted defect fails the matching check, which names the sample, its slot and the column."""
    generic = defect == 'generic_mask'
    m, lay, q, tr = cases.model(), cases.layout(generic), cases.pool_problem(), cases.pool_truth(257, generic)
    e = fr.emulate(m, lay, q, kernel, defect)
    with pytest.raises(AssertionError, match=refused) as err:
        fr.check_features(f'defect {defect}', tr, kernel, e['mlp_in'], e['dist'], e['x'])
    print(f'refused {defect}:', str(err.value)[:240])
