"""CPU: the restatement of the split-operand MLP kernels (tests/split_mlp_restatement.py) and its cases
(tests/split_mlp_cases.py) hold what they promise: every case passes its own exactness assertions, the restatement with
rd = identity is the plain product, the two roundings are the formats', the F16x3 split keeps 22 bits, the fp32 emulation in
the kernels' k-step order passes every check -- and each planted defect fails the check named for it."""
import numpy as np
import pytest
import torch

from tests import split_mlp_cases as C
from tests import split_mlp_restatement as R

SPLIT = ('f16x3', 'bf16x3')
HANN_A = (1, 1, .75, .25, 0, 0)
SELECTED = (0, 40, 64)
N = 65


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope='module')
def canonical_cases():
    out = {}
    for pol in SPLIT:
        x, Ws, Bs = C.canonical_case(pol, N, selected=SELECTED)
        out[pol] = (x, Ws, Bs) + C.check_canonical(pol, x, Ws, Bs)
    return out


@pytest.fixture(scope='module')
def nonrigid_cases():
    out = {}
    for pol in SPLIT:
        for embed in (False, True):
            cond, Ws, Bs, xyz = C.nonrigid_case(pol, N, embed=embed)
            for hann in (C.HANN_B if embed else (HANN_A,)):
                out[pol, embed, hann] = (cond, Ws, Bs, xyz) + C.check_nonrigid(pol, cond, Ws, Bs, hann, xyz)
    return out


@pytest.mark.parametrize('pol', SPLIT)
def test_cases_are_exact_and_exercise_the_split(canonical_cases, nonrigid_cases, pol):
    """(the exactness assertions ran in the fixtures) xl != 0 in thousands of entries, a lo weight meets such an entry (the
    dropped Wl xl is non-zero), about half of the pre-activations are negative in every layer, no site reports."""
    stats = [canonical_cases[pol][5]] + [v[6] for k, v in nonrigid_cases.items() if k[0] == pol]
    for st in stats:
        assert st['xl_nonzero'] > 1000 and st['lo_meets_xl'] > 0 and st['span'] < 24
        assert all(0.2 < f < 0.75 for f in st['negative'][1:]), st['negative']
    assert not any(canonical_cases[pol][4].values())
    # the carry row reaches the high end of the range, the dropped-lo output is 1 + 2 eps and NOT the full product
    raw = canonical_cases[pol][3]
    eps = C.eps_of(pol)
    assert (raw[:, 2] > 1000).all() and (raw[:, 1] == np.float32(1 + 2 * eps)).all()


@pytest.mark.parametrize('pol', SPLIT)
def test_case_b_separates_the_embedding_columns(nonrigid_cases, pol):
    """the three windows give three different offsets; with the all-zero window the embedding contributes exactly nothing
    (== the same weights with the embedding columns zeroed)"""
    outs = [nonrigid_cases[pol, True, h][4] for h in C.HANN_B]
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
    cond, Ws, Bs, xyz = nonrigid_cases[pol, True, C.HANN_B[2]][:4]
    Wz = [w.copy() for w in Ws]
    Wz[0][:, 69:] = 0
    Wz[4][:, 128:] = 0
    assert np.array_equal(_bits(C.check_nonrigid(pol, cond, Wz, Bs, C.HANN_B[0], xyz)[0]), _bits(outs[2]))
    for W, base in ((Ws[0], 69), (Ws[4], 128)):
        w = W[:, base:]
        assert ((w != 0).sum(0) == 1).all() and len(set(np.abs(w).max(0))) == 36


def test_identity_restatement_is_the_plain_product(canonical_cases, nonrigid_cases):
    """rd = identity (the direct-load fp32 kernels): the restatement, exact by its own assertions, == x @ W.T + b in float64"""
    x, Ws, Bs = canonical_cases['f16x3'][:3]
    raw, _ = R.canonical(R.Exact(R.FP32), Ws, Bs, x)
    assert np.array_equal(raw.astype(np.float64), R.plain_canonical(Ws, Bs, x))
    assert not np.array_equal(_bits(raw), _bits(canonical_cases['f16x3'][3]))      # (W x, where the split kernels drop Wl xl)
    for (pol, embed, hann), (cond, Ws, Bs, xyz, *_rest) in nonrigid_cases.items():
        if pol == 'f16x3':
            out, _ = R.nonrigid(R.Exact(R.FP32), Ws, Bs, cond, hann, xyz)
            want = R.plain_nonrigid(Ws, Bs, cond, hann, xyz)
            assert np.array_equal(out.astype(np.float64), want.astype(np.float32).astype(np.float64))
            assert np.array_equal((out - xyz).astype(np.float64), want - xyz)      # (the offset itself is exact)


def test_rd_bf16_is_torchs():
    rng = np.random.default_rng(5)
    u = rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)
    u[:2000] = (u[:2000] & 0xFFFF0000) | 0x8000                                     # ties
    u[2000:4000] &= 0x807FFFFF                                                      # subnormals
    u[4000:4006] = [0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0x00000000, 0x80000000, 0x7F7F8000]
    a = u.view(np.float32)
    want = torch.from_numpy(a.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    got = R.rd_bf16(a)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got[~nan]), _bits(want[~nan]))


def test_f16x3_split_keeps_22_bits():
    """split.h: hi + lo = 22 bits, the residue of the split is at most 2^-22 relative for 2^-7 <= |x| < 4094"""
    rng = np.random.default_rng(6)
    x = np.exp2(rng.uniform(-7, np.log2(4094), 100000)).astype(np.float32) * rng.choice([-1, 1], 100000).astype(np.float32)
    x = x[(np.abs(x) >= 2.0 ** -7) & (np.abs(x) < 4094)]
    v = np.float32(16) * x
    xh, xl, _ = R.split_x(R.F16X3, v)
    res = np.abs(v.astype(np.float64) - xh.astype(np.float64) - xl.astype(np.float64))
    assert (res <= 2.0 ** -22 * np.abs(v.astype(np.float64))).all(), float((res / np.abs(v)).max())


# ---------------------------------------------------------------------------------------------------------------------------
# the emulation (fp32, the kernels' k-step order) and the planted defects
# ---------------------------------------------------------------------------------------------------------------------------
def _emulate_canonical(pol, case, defect=None):
    return R.canonical(R.Emulated(R.POLICIES[pol], defect), case[1], case[2], case[0])


def _emulate_nonrigid(pol, case, hann, defect=None):
    return R.nonrigid(R.Emulated(R.POLICIES[pol], defect), case[1], case[2], case[0], hann, case[3])


@pytest.mark.parametrize('pol', SPLIT + ('fp32',))
def test_emulation_passes_every_check(canonical_cases, nonrigid_cases, pol):
    src = 'f16x3' if pol == 'fp32' else pol
    x, Ws, Bs = canonical_cases[src][:3]
    want, flags = R.canonical(R.Exact(R.POLICIES[pol]), Ws, Bs, x)
    got, gflags = _emulate_canonical(pol, (x, Ws, Bs))
    assert np.array_equal(_bits(got), _bits(want)) and gflags == flags
    for (p, embed, hann), case in nonrigid_cases.items():
        if p == src:
            want, flags = R.nonrigid(R.Exact(R.POLICIES[pol]), case[1], case[2], case[0], hann, case[3])
            got, gflags = _emulate_nonrigid(pol, case, hann)
            assert np.array_equal(_bits(got), _bits(want)) and gflags == flags


def _lo_step(W, pol, kind=None):
    """a k-step of the layer in which a non-zero lo weight sits"""
    _, Wl = R.split_w(R.POLICIES[pol], W)
    col = int(np.nonzero((Wl != 0).any(0))[0][0])
    return next(s for s, cols in enumerate(R.k_steps(kind, W.shape[1])) if col in cols)


def _site_case(pol, site, value):
    """the canonical case with the probe of `site` at `value` for the selected samples (the GPU domain test's construction)"""
    if site == 'in':
        return C.canonical_case(pol, N, selected=SELECTED, x_probe=value)
    return C.canonical_case(pol, N, selected=SELECTED, probe=(site, value))


DEFECTS = {
    'third product dropped in one k-step': lambda c: ('drop3', 'geo2', _lo_step(c[1][2], 'f16x3')),
    '2^-11 applied twice': lambda c: ('twice',),
    'hi and lo pieces of one chunk swapped': lambda c: ('swap', 'rgb1', _lo_step(c[1][6], 'f16x3')),
    'a bias not scaled by kSx': lambda c: ('bias', 'geo1'),
    "sigma's 1/kSx applied after its bias": lambda c: ('late', 'sigma'),
    "rgb's 1/kSx applied after its bias": lambda c: ('late', 'rgb'),
    'geometry features fed to the colour trunk unsplit': lambda c: ('unsplit', 'rgb0'),
    'Wl xl added': lambda c: ('lolo',),
}


@pytest.mark.parametrize('name', sorted(DEFECTS))
def test_planted_defect_fails_bit_equality(canonical_cases, name):
    case = canonical_cases['f16x3']
    want = case[3]
    got, _ = _emulate_canonical('f16x3', case, DEFECTS[name](case))
    assert not np.array_equal(_bits(got), _bits(want)), name
    ok, _ = _emulate_canonical('f16x3', case)
    assert np.array_equal(_bits(ok), _bits(want))


@pytest.mark.parametrize('pol', SPLIT)
def test_planted_lolo_and_drop3_fail_for_both_policies(canonical_cases, nonrigid_cases, pol):
    case = canonical_cases[pol]
    for defect in (('lolo',), ('drop3', 'geo2', _lo_step(case[1][2], pol))):
        got, _ = _emulate_canonical(pol, case, defect)
        assert not np.array_equal(_bits(got), _bits(case[3])), defect
    nr = nonrigid_cases[pol, False, HANN_A]
    for defect in (('lolo',), ('drop3', 'nr2', _lo_step(nr[1][2], pol))):
        got, _ = _emulate_nonrigid(pol, nr, HANN_A, defect)
        assert not np.array_equal(_bits(got), _bits(nr[4])), defect


@pytest.mark.parametrize('pol', SPLIT + ('fp32',))
def test_planted_skipped_embedding_step_fails_case_b(nonrigid_cases, pol):
    """one embedding k-step of the skip layer (steps 8..10 of its 11) skipped: case (B) with the full window fails, and so does the
    half-open window for the steps that hold a non-zero operand"""
    src = 'f16x3' if pol == 'fp32' else pol
    for hann in C.HANN_B[:2]:
        case = nonrigid_cases[src, True, hann]
        want, _ = R.nonrigid(R.Exact(R.POLICIES[pol]), case[1], case[2], case[0], hann, case[3])
        for step in (8, 9, 10):
            got, _ = _emulate_nonrigid(pol, case, hann, ('skipstep', 'skip', step))
            live = any(hann[(c - 128) // 6] != 0 and (c - 128) % 6 >= 3 for c in R.k_steps('NrSkip', 164)[step])
            assert np.array_equal(_bits(got), _bits(want)) != live, (hann, step)
        got, _ = _emulate_nonrigid(pol, case, hann, ('skipstep', 'nr0', 0))
        assert not np.array_equal(_bits(got), _bits(want))


def test_planted_low_clamp_fails_at_4093():
    """the ReLU clamp at 65472 where 65504 belongs: an activation of 4093 (hi 65472, lo 16) loses its lo piece"""
    x, Ws, Bs = _site_case('f16x3', 'geo1', 4093.0)
    want, flags, _ = C.check_canonical('f16x3', x, Ws, Bs)
    assert not any(flags.values())
    good, gflags = _emulate_canonical('f16x3', (x, Ws, Bs))
    assert np.array_equal(_bits(good), _bits(want)) and gflags == flags
    bad, _ = _emulate_canonical('f16x3', (x, Ws, Bs), ('clamp',))
    assert not np.array_equal(_bits(bad), _bits(want))


@pytest.mark.parametrize('site', R.CANONICAL_SITES)
def test_planted_missing_watch_fails_its_site(site):
    """4094 (signed sites: +-4094) at one site sets exactly that site's report; an emulation that does not watch the site
    reports nothing, and the check -- the restatement's report -- fails it"""
    for value in ((4094.0, -4094.0) if site in R.SIGNED_SITES else (4094.0,)):
        x, Ws, Bs = _site_case('f16x3', site, value)
        _, flags = R.canonical(R.Exact(R.F16X3), Ws, Bs, x)
        assert flags == {s: s == site for s in R.CANONICAL_SITES}, (site, value, flags)
        _, good = _emulate_canonical('f16x3', (x, Ws, Bs))
        assert good == flags
        _, bad = _emulate_canonical('f16x3', (x, Ws, Bs), ('nowatch', site))
        assert any(bad.values()) != any(flags.values())


@pytest.mark.parametrize('site', R.NONRIGID_SITES)
def test_planted_missing_watch_fails_its_nonrigid_site(site):
    cond, Ws, Bs, xyz = C.nonrigid_case('f16x3', N, probe=(site, 4094.0))
    _, flags = R.nonrigid(R.Exact(R.F16X3), Ws, Bs, cond, HANN_A, xyz)
    assert flags == {s: s == site for s in R.NONRIGID_SITES}
    _, bad = R.nonrigid(R.Emulated(R.F16X3, ('nowatch', site)), Ws, Bs, cond, HANN_A, xyz)
    assert not any(bad.values())


def test_domain_edges():
    """the numbers of the module docstring: 4093 and +-4093.5 are clear and exact, 4094 reports, 5000 in an unwatched layer is
    exact and silent"""
    for site in R.CANONICAL_SITES:
        for value in ((4093.5, -4093.5) if site in R.SIGNED_SITES else (4093.0,)):
            x, Ws, Bs = _site_case('f16x3', site, value)
            _, flags, _ = C.check_canonical('f16x3', x, Ws, Bs)
            assert not any(flags.values()), (site, value)
    x, Ws, Bs = _site_case('f16x3', 'rgb3', 5000.0)
    raw, flags, _ = C.check_canonical('f16x3', x, Ws, Bs)
    assert not any(flags.values()) and (raw[list(SELECTED), 2] > 2000).all()
    for site in R.NONRIGID_SITES + ('nr5',):
        cond, Ws, Bs, xyz = C.nonrigid_case('f16x3', N, probe=(site, 5000.0 if site == 'nr5' else 4093.0))
        _, flags, _ = C.check_nonrigid('f16x3', cond, Ws, Bs, HANN_A, xyz)
        assert not any(flags.values()), site
    h = np.float16(65504.0)
    assert h == np.finfo(np.float16).max and float(np.nextafter(h, np.float16(0))) == 65472.0
    assert float(np.float32(65488.0).astype(np.float16)) == 65472.0 and float(np.float32(65489.0).astype(np.float16)) == 65504.0
    assert 16 * 4093 == 65488 and 16 * 4094 == 65504 and 16 * 4093.5 == 65496


def test_probe_rows_sit_in_both_half_waves():
    """lane l of a wave holds sample l & 31 and the features with bit 2 equal to l >> 5 (mlp_layout.h): the probe rows of the
    watched ReLU sites, placed at random per layer, cover the lanes below 32 and the lanes from 32 on"""
    layer = {'geo0': 0, 'geo1': 1, 'geo2': 2, 'geo3': 3, 'rgb0': 5, 'rgb1': 6, 'rgb2': 7}
    halves = set()
    for site, l in layer.items():
        _, Ws, _ = _site_case('f16x3', site, 4093.0)
        rows = np.nonzero((Ws[l] == np.float32(4093.0)).any(1))[0]
        assert len(rows) == 1
        halves.add((int(rows[0]) >> 2) & 1)
    assert halves == {0, 1}
