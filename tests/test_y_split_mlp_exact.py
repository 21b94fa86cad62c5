"""GPU: the split-operand MLP kernels (csrc/mlp.hip, csrc/nonrigid.hip under the policies of csrc/split.h) bit for bit against
the NumPy restatement (tests/split_mlp_restatement.py) on cases whose every accumulator is exact in any order
(tests/split_mlp_cases.py, asserted there per accumulator).  No tolerance anywhere: the kernels return the restatement's bits.

Kernels and instantiations covered
  canonical_mlp_split_lds_kernel<Bf16x3, false>           ops.canonical_mlp_bf16x3(variant=0), bf16 pack
  canonical_mlp_bf16x3_kernel (direct load)               ops.canonical_mlp_bf16x3(variant=1), bf16 pack: the same restatement
  canonical_mlp_split_lds_kernel<F16x3, false | true>     fp16 pack without | with a flag word: identical bits, flag stays 0
  nonrigid_split_kernel<Bf16x3, false>                    ops.nonrigid_bf16x3 / _rows, bf16 pack
  nonrigid_split_kernel<F16x3, false | true>              fp16 pack without | with a flag word
  nr16::nonrigid_lds_kernel, nonrigid_kernel (direct)     case (B) only (the embedding at the origin); their other exact cases
                                                          are in test_a_mlp_exact.py
All of them launch ceil(N / 128) workgroups of four 32-sample waves and none is persistent (read in mlp_bf16x3_launch,
occnerf_canonical_mlp_f16x3 and nr_split_launch), so the sizes are waves of 32, workgroups of 128 and two workgroups plus one.

Domain sites (F16x3, WATCH = true), enumerated from the kernel sources: the canonical kernel watches NINE -- the inputs
(watch_abs), relu_split after geo L0, after each of the three geo hidden layers (the last one after the sigma row), the signed
geometry head (watch_abs), relu_split after rgb L0 and after the first two rgb hidden layers; the non-rigid kernel watches
FIVE -- NR_RELU_SPLIT after layers 0..3 and after the skip layer.  The last hidden layer of the colour trunk and of the
non-rigid trunk feeds fp32 dot rows through fmaxf, neither clamped nor watched.  Per site: 4093 (signed sites +-4093.5) leaves
the flag 0 and the output bit-exact, 4094 (+-4094) sets the flag; 5000 in an unwatched layer is exact and silent.  The
numbers are derived from split.h in the restatement's docstring.  In the canonical cases the probe value reaches chosen
samples only: the first lane of the launch, a wave other than wave 0, and the single sample of the last, partial wave (whose
idle lanes replicate it: a flagged last row is reported by them too, which is fine); the probe rows' positions differ from
layer to layer, so both half-waves (lanes < 32 and >= 32 hold different features) are covered.  The non-rigid kernel's
only per-sample input is the embedding, exact at the origin only, so its probes reach every sample (and a row list whose only
flagged sample lies beyond the count can be built for the canonical kernel alone).
"""
import numpy as np
import pytest
import torch

from tests import split_mlp_cases as C
from tests import split_mlp_restatement as R
from tests.gpu_util import DEV, T

pytestmark = pytest.mark.gpu

CANON_N = (1, 31, 32, 33, 127, 128, 129, 257)
NR_N = (1, 31, 32, 33, 128, 129, 389)
HANN_A = (1, 1, .75, .25, 0, 0)
DOM_N = 161                                       # one workgroup, one full wave and one sample of a second workgroup
DOM_SELECTED = (0, 37, 160)                       # first lane | wave 1 | the last, partial wave
FILL = 7.0


def _assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def _flag():
    return torch.zeros(1, device=DEV, dtype=torch.int32)


def _canonical_packs(ops, policy, Ws, Bs):
    Wd, Bd = [T(w) for w in Ws], [T(b) for b in Bs]
    pack = ops.canonical_mlp_pack_f16 if policy == 'f16x3' else ops.canonical_mlp_pack_bf16
    return ops.canonical_mlp_pack(Wd, Bd), pack(Wd)


def _run_canonical(ops, packs, x, flag=None, variant=0, count=None, in_rows=None):
    """-> raw[m + 3, 5] (m outputs, three guard rows) filled with FILL before the launch"""
    m = x.shape[0] if in_rows is None else in_rows.shape[0]
    raw = torch.full((m + 3, 5), FILL, device=DEV)
    ops.canonical_mlp_bf16x3(T(x), packs[0], packs[1], raw[:m], variant=variant, count=count, in_rows=in_rows, domain_flag=flag)
    return raw.cpu().numpy()


@pytest.fixture(scope='module')
def canonical(ops):
    """per policy: x, the packed weights on the device, the restatement's raw -- computed once, never modified"""
    out = {}
    for policy in ('f16x3', 'bf16x3'):
        x, Ws, Bs = C.canonical_case(policy, max(CANON_N), selected=(0, 40, 130, 256))
        want, flags, _ = C.check_canonical(policy, x, Ws, Bs)
        assert not any(flags.values())
        out[policy] = (x, _canonical_packs(ops, policy, Ws, Bs), want)
    return out


# (policy, variant, with a flag word)
CANON_KERNELS = {'bf16x3-lds': ('bf16x3', 0, False), 'bf16x3-direct': ('bf16x3', 1, False),
                 'f16x3': ('f16x3', 0, False), 'f16x3-watched': ('f16x3', 0, True)}


@pytest.mark.parametrize('n', CANON_N)
@pytest.mark.parametrize('kernel', sorted(CANON_KERNELS))
def test_canonical_exact(ops, canonical, kernel, n):
    """bit-equal to the restatement; raw[:, 4] and the guard rows keep their fill; a flag word stays 0 and changes no bit"""
    policy, variant, watched = CANON_KERNELS[kernel]
    x, packs, want = canonical[policy]
    flag = _flag() if watched else None
    got = _run_canonical(ops, packs, x[:n], flag, variant)
    _assert_bits(got[:n, :4], want[:n], kernel)
    assert (got[:n, 4] == FILL).all() and (got[n:] == FILL).all()
    assert flag is None or int(flag.item()) == 0


@pytest.mark.parametrize('kernel', sorted(CANON_KERNELS))
def test_canonical_rows_exact(ops, canonical, kernel):
    """the row-list form: in_rows a permutation with repeats, the count on the device and short of the list == the dense
    restatement on the gathered rows, compact; entries at or beyond the count keep their fill"""
    policy, variant, watched = CANON_KERNELS[kernel]
    x, packs, want = canonical[policy]
    rng = np.random.default_rng(3)
    rows = np.concatenate([rng.permutation(len(x))[:140], rng.integers(0, len(x), 21)]).astype(np.int32)
    count = len(rows) - 7
    flag = _flag() if watched else None
    got = _run_canonical(ops, packs, x, flag, variant, count=T(np.asarray([count], np.int32)), in_rows=T(rows))
    _assert_bits(got[:count, :4], want[rows[:count]], kernel)
    assert (got[:count, 4] == FILL).all() and (got[count:] == FILL).all()
    assert flag is None or int(flag.item()) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# non-rigid
# ---------------------------------------------------------------------------------------------------------------------------
NR_KERNELS = {'bf16x3': ('bf16x3', False), 'f16x3': ('f16x3', False), 'f16x3-watched': ('f16x3', True)}


class _NrDevice:
    def __init__(self, ops, policy, cond, Ws, Bs):
        self.Wd, self.Bd = [T(w) for w in Ws], [T(b) for b in Bs]
        self.cond = T(cond)
        self.packed = ops.nonrigid_pack(self.Wd, self.Bd)
        self.split = None if policy == 'fp32' else (ops.nonrigid_pack_f16 if policy == 'f16x3' else ops.nonrigid_pack_bf16)(self.Wd)


def _run_nonrigid(ops, dev, hann, xyz, kernel='split', flag=None):
    """-> buf[n + 2, 3]: the kernel in place on the first n rows, two guard rows"""
    n = xyz.shape[0]
    buf = torch.full((n + 2, 3), FILL, device=DEV)
    buf[:n] = T(xyz)
    h = np.asarray(hann, np.float32)
    if kernel == 'split':
        ops.nonrigid_bf16x3(buf[:n], dev.cond, h, dev.Wd[0], dev.Bd[0], dev.packed, dev.split, out=buf[:n], domain_flag=flag)
    else:
        ops.nonrigid(buf[:n], dev.cond, h, dev.Wd[0], dev.Bd[0], dev.packed, out=buf[:n], direct=kernel == 'direct')
    return buf.cpu().numpy()


@pytest.fixture(scope='module')
def nonrigid_a(ops):
    out = {}
    for policy in ('f16x3', 'bf16x3'):
        cond, Ws, Bs, xyz = C.nonrigid_case(policy, max(NR_N))
        want, flags, _ = C.check_nonrigid(policy, cond, Ws, Bs, HANN_A, xyz)
        assert not any(flags.values())
        out[policy] = (xyz, _NrDevice(ops, policy, cond, Ws, Bs), want)
    return out


@pytest.mark.parametrize('n', NR_N)
@pytest.mark.parametrize('kernel', sorted(NR_KERNELS))
def test_nonrigid_exact(ops, nonrigid_a, kernel, n):
    """case (A), in place: bit-equal to the restatement, guard rows untouched, the flag word 0 and without influence"""
    policy, watched = NR_KERNELS[kernel]
    xyz, dev, want = nonrigid_a[policy]
    flag = _flag() if watched else None
    got = _run_nonrigid(ops, dev, HANN_A, xyz[:n], flag=flag)
    _assert_bits(got[:n], want[:n], kernel)
    assert (got[n:] == FILL).all()
    assert flag is None or int(flag.item()) == 0


@pytest.mark.parametrize('kernel', sorted(NR_KERNELS))
def test_nonrigid_rows_exact(ops, nonrigid_a, kernel):
    """nonrigid_bf16x3_rows, in place, the count on the device and short of the list: the listed rows get the restatement's
    bits, every other row keeps its own"""
    policy, watched = NR_KERNELS[kernel]
    xyz, dev, want = nonrigid_a[policy]
    n = len(xyz)
    rows = np.random.default_rng(4).permutation(n)[:150].astype(np.int32)
    count = len(rows) - 9
    flag = _flag() if watched else None
    buf = T(xyz).clone()
    ops.nonrigid_bf16x3_rows(buf, T(rows), T(np.asarray([count], np.int32)), dev.cond, np.asarray(HANN_A, np.float32), dev.Wd[0],
                             dev.Bd[0], dev.packed, dev.split, domain_flag=flag)
    got = buf.cpu().numpy()
    keep = np.ones(n, bool)
    keep[rows[:count]] = False
    _assert_bits(got[~keep], want[~keep], kernel)
    _assert_bits(got[keep], xyz[keep], kernel + ': rows not listed')
    assert flag is None or int(flag.item()) == 0


NR_B_KERNELS = {'nr16': ('fp32', 'lds', False), 'direct': ('fp32', 'direct', False), 'bf16x3': ('bf16x3', 'split', False),
                'f16x3': ('f16x3', 'split', False), 'f16x3-watched': ('f16x3', 'split', True)}


@pytest.fixture(scope='module')
def nonrigid_b(ops):
    """case (B) per kernel policy: the fp32 kernels run the F16x3 case's weights under the restatement with rd = identity"""
    out = {}
    for policy in ('fp32', 'f16x3', 'bf16x3'):
        cond, Ws, Bs, xyz = C.nonrigid_case('f16x3' if policy == 'fp32' else policy, 129, embed=True)
        want = {hann: C.check_nonrigid(policy, cond, Ws, Bs, hann, xyz)[0] for hann in C.HANN_B}
        out[policy] = (xyz, _NrDevice(ops, policy, cond, Ws, Bs), want)
    return out


@pytest.mark.parametrize('hann', C.HANN_B, ids=('open', 'half', 'closed'))
@pytest.mark.parametrize('kernel', sorted(NR_B_KERNELS))
def test_nonrigid_embedding_at_the_origin(ops, nonrigid_b, kernel, hann):
    """case (B): xyz = 0, so the embedding operands are the window's values, non-zero and exact, each embedding column of layer 0
    and of the skip layer with a weight of its own; the sine columns and the closed octaves contribute exactly nothing (which
    also says that the device's sinf(0) is 0 and cosf(0) is 1)"""
    policy, which, watched = NR_B_KERNELS[kernel]
    xyz, dev, want = nonrigid_b[policy]
    flag = _flag() if watched else None
    got = _run_nonrigid(ops, dev, hann, xyz, kernel=which, flag=flag)
    _assert_bits(got[:len(xyz)], want[hann], (kernel, hann))
    assert (got[len(xyz):] == FILL).all()
    assert flag is None or int(flag.item()) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the domain report of F16x3, site by site
# ---------------------------------------------------------------------------------------------------------------------------
def _canonical_site(site, value, selected):
    if site == 'in':
        return C.canonical_case('f16x3', DOM_N, selected=selected, x_probe=value)
    return C.canonical_case('f16x3', DOM_N, selected=selected, probe=(site, value))


@pytest.mark.parametrize('site', R.CANONICAL_SITES)
def test_canonical_domain_site(ops, site):
    signed = site in R.SIGNED_SITES
    for value in ((4093.5, -4093.5) if signed else (4093.0,)):          # inside: the flag stays 0 and every bit is the restatement's
        x, Ws, Bs = _canonical_site(site, value, DOM_SELECTED)
        want, flags, _ = C.check_canonical('f16x3', x, Ws, Bs)
        assert not any(flags.values())
        flag = _flag()
        got = _run_canonical(ops, _canonical_packs(ops, 'f16x3', Ws, Bs), x, flag)
        assert int(flag.item()) == 0, (site, value)
        _assert_bits(got[:DOM_N, :4], want, (site, value))
    for value in ((4094.0, -4094.0) if signed else (4094.0,)):          # at the edge: this site, and no other, reports
        packs = None
        for sample in DOM_SELECTED:
            x, Ws, Bs = _canonical_site(site, value, (sample,))
            _, flags = R.canonical(R.Exact(R.F16X3), Ws, Bs, x)
            assert flags == {s: s == site for s in R.CANONICAL_SITES}
            packs = packs or _canonical_packs(ops, 'f16x3', Ws, Bs)     # (the weights do not depend on the sample)
            flag = _flag()
            _run_canonical(ops, packs, x, flag)
            assert int(flag.item()) == 1, (site, value, sample)


def test_canonical_unwatched_last_hidden_layer(ops):
    """5000 in the colour trunk's last hidden layer: fp32 dot rows over an unclamped ReLU, exact and silent"""
    x, Ws, Bs = _canonical_site('rgb3', 5000.0, DOM_SELECTED)
    want, flags, _ = C.check_canonical('f16x3', x, Ws, Bs)
    assert not any(flags.values())
    flag = _flag()
    got = _run_canonical(ops, _canonical_packs(ops, 'f16x3', Ws, Bs), x, flag)
    assert int(flag.item()) == 0
    _assert_bits(got[:DOM_N, :4], want, 'rgb3')


def test_canonical_rows_beyond_the_count_are_not_reported(ops):
    """a row list whose only flagged sample is listed at or beyond the device-side count leaves the flag 0 (and reports it when
    the count includes it)"""
    x, Ws, Bs = _canonical_site('geo1', 4094.0, (5,))
    packs = _canonical_packs(ops, 'f16x3', Ws, Bs)
    rows = np.asarray([r for r in range(DOM_N) if r != 5] + [5, 5], np.int32)
    for count, reported in ((len(rows) - 2, 0), (len(rows) - 1, 1)):
        flag = _flag()
        _run_canonical(ops, packs, x, flag, count=T(np.asarray([count], np.int32)), in_rows=T(rows))
        assert int(flag.item()) == reported, count


@pytest.mark.parametrize('site', R.NONRIGID_SITES + ('nr5',))
def test_nonrigid_domain_site(ops, site):
    """nr5, the last hidden layer, is not watched: 5000 there is exact and silent"""
    watched = site != 'nr5'
    cond, Ws, Bs, xyz = C.nonrigid_case('f16x3', DOM_N, probe=(site, 4093.0 if watched else 5000.0))
    want, flags, _ = C.check_nonrigid('f16x3', cond, Ws, Bs, HANN_A, xyz)
    assert not any(flags.values())
    flag = _flag()
    got = _run_nonrigid(ops, _NrDevice(ops, 'f16x3', cond, Ws, Bs), HANN_A, xyz, flag=flag)
    assert int(flag.item()) == 0, site
    _assert_bits(got[:DOM_N], want, site)
    if watched:
        cond, Ws, Bs, xyz = C.nonrigid_case('f16x3', DOM_N, probe=(site, 4094.0))
        _, flags = R.nonrigid(R.Exact(R.F16X3), Ws, Bs, cond, HANN_A, xyz)
        assert flags == {s: s == site for s in R.NONRIGID_SITES}
        flag = _flag()
        _run_nonrigid(ops, _NrDevice(ops, 'f16x3', cond, Ws, Bs), HANN_A, xyz, flag=flag)
        assert int(flag.item()) == 1, site
