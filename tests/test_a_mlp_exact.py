"""GPU: the two fp32 LDS-staged MLP kernels (mlp16.hip, nonrigid16.hip) on EXACT arithmetic, bit for bit.

Weights are sparse with entries in {0, +-1, +-1/2} (two per row), biases and inputs small multiples of 1/4.  A row's sum
then at most doubles the magnitude (+ 1) and adds one fractional bit per layer: through the ten layers of the canonical MLP
every partial sum needs <= 11 integer + 12 fractional bits < 24, so it is exact in fp32 WHATEVER the order of the k-steps,
and the kernel must return the bits of a plain NumPy restatement -- a weight chunk that lands in the wrong ring slot, a
group read twice or skipped, a wrong bias row all show, because every layer has its own weights.  Each ReLU layer has
   * a row of -0.0 weights with a -0.0 bias (pre-activation -0.0 for the samples whose inputs are all >= +0),
   * a row of +0.0 weights with a +0.0 bias (pre-activation +0.0),
   * a row that carries 2^21 + x from layer to layer (weight 1 on the previous layer's such row),
beside the ordinary rows, which come out negative and positive; no infinities.  The restatement asserts these categories
and its own exactness (fp32 sequential sum == float64 matrix product).  The sign of a zero sum does not depend on the
order either: it is -0.0 only if every term is.  One exception, stated rather than hidden: the colour trunk's first
layer cannot see -0.0 in the KERNEL -- its k-steps include the slot of `var`, which is not one of its inputs and is
packed as a +0.0 weight -- so that layer is not asked for it.  The two direct-load kernels of mlp.hip and nonrigid.hip
(`direct`) run the same cases, the 2^21 and the zero rows included, and need no further exception: their pad k-steps
(+0.0 weights against +0.0 operands) do not change a bit of the outputs.
"""
import numpy as np
import pytest
import torch

from tests import util
from tests.gpu_util import DEV, T

pytestmark = pytest.mark.gpu

BIG = np.float32(2.0 ** 21)


def _with_direct(sizes):
    """every size for the LDS-staged kernel (id: the size) and again for the direct-load kernel (id: size-direct)"""
    return [pytest.param(n, False, id=str(n)) for n in sizes] + [pytest.param(n, True, id='%d-direct' % n) for n in sizes]


def _frac_bits(a):
    """per entry: the number of fractional bits of a (float64 array of dyadic values with at most 30 of them)"""
    m = np.abs(a) * 2.0 ** 30
    assert np.array_equal(m, np.round(m))
    m = m.astype(np.int64)
    low = np.where(m > 0, m & -m, 1 << 30)
    return np.maximum(30 - np.log2(low.astype(np.float64)), 0)


def _lin(h, W, b):
    """fp32 b + sum_k h[:, k] * W[:, k], sequential in k.  Asserts that the sum is exact in ANY order: with q the largest
    number of fractional bits among a row's terms, every partial sum is a multiple of 2^-q below sum |terms| < 2^(24 - q)."""
    acc = np.broadcast_to(b.astype(np.float32), (h.shape[0], W.shape[0])).copy()
    for k in range(W.shape[1]):
        acc = acc + h[:, k:k + 1] * W[None, :, k]
    assert acc.dtype == np.float32
    terms = h[:, None, :].astype(np.float64) * W[None].astype(np.float64)
    q = np.maximum(_frac_bits(terms).max(-1), _frac_bits(b.astype(np.float64))[None])
    assert (np.abs(terms).sum(-1) + np.abs(b.astype(np.float64))[None] < 2.0 ** (24 - q)).all()
    assert np.array_equal(acc.astype(np.float64), terms.sum(-1) + b.astype(np.float64))
    return acc


def _relu(a):
    return np.where(a > 0, a, np.float32(0.0)).astype(np.float32)


def _categories(pre, neg_zero=True):
    """the pre-activations of one ReLU layer take -0.0, +0.0, negative, positive and > 2^20 values"""
    z = pre == 0
    assert (z & ~np.signbit(pre)).any() and (pre < 0).any() and ((pre > 0) & (pre < 2.0 ** 20)).any()
    assert (pre > 2.0 ** 20).any() and np.isfinite(pre).all()
    if neg_zero:
        assert (z & np.signbit(pre)).any()


def _sparse(rng, out_dim, in_dim, avoid=()):
    """two entries of {+-1, +-1/2} per row, every column (but `avoid`) used; biases multiples of 1/4 in [-1, 1]"""
    W = np.zeros((out_dim, in_dim), np.float32)
    cols = np.array([c for c in range(in_dim) if c not in avoid])
    first = np.resize(rng.permutation(cols), out_dim) if out_dim >= len(cols) else rng.permutation(cols)[:out_dim]
    second = rng.choice(cols, out_dim)
    vals = np.array([1, -1, 0.5, -0.5], np.float32)
    W[np.arange(out_dim), second] = rng.choice(vals, out_dim)
    W[np.arange(out_dim), first] = rng.choice(vals, out_dim)
    b = (rng.integers(-4, 5, out_dim) / 4).astype(np.float32)
    return W, b


def _read_out(rng, W, rows, big):
    """the output rows `rows` share all columns but `big` between them (entries of {+-1, +-1/2}), so that every feature of
    the layer before reaches an output"""
    cols = np.array([c for c in range(W.shape[1]) if c != big])
    for i, r in enumerate(rows):
        mine = cols[i::len(rows)]
        W[r] = 0.0
        W[r, mine] = rng.choice(np.array([1, -1, 0.5, -0.5], np.float32), len(mine))


def _special(rng, W, b, big_col, neg_mask=None):
    """-> (the -0.0 row's index, the big row's index); rows (-0.0), (+0.0) and (carry 2^21 + x) of a ReLU layer.  neg_mask: columns whose input is
    negative for every sample (there the -0.0 row holds +0.0, so that the product is -0.0 all the same)."""
    nz, pz, bg = rng.choice(W.shape[0], 3, replace=False)
    W[nz] = -0.0
    if neg_mask is not None:
        W[nz, neg_mask] = 0.0
    b[nz] = -0.0
    W[pz], b[pz] = 0.0, 0.0
    W[bg], b[bg] = 0.0, 0.0
    W[bg, big_col] = 1.0
    return int(nz), int(bg)


# ------------------------------------------------------------------------------------------------------------------
# canonical MLP: x[68] = [agg35, var, enc32] -> 4 x 256 -> (sigma, geo64); [geo64, agg35, enc32] -> 4 x 256 -> rgb
# ------------------------------------------------------------------------------------------------------------------
M16_N = (1, 16, 17, 64, 65)


def _m16_case():
    rng = np.random.default_rng(16)
    n = max(M16_N)
    x = (rng.integers(-4, 5, (n, 68)) / 4).astype(np.float32)
    x[0::2] = np.abs(x[0::2])                          # even samples: all inputs >= +0 (the -0.0 rows)
    Ws, Bs = [], []
    W, b = _sparse(rng, 256, 68, avoid=(0,))
    _, big = _special(rng, W, b, 0)
    b[big] = BIG                                       # 2^21 + x[:, 0]
    Ws.append(W), Bs.append(b)
    for _ in range(3):
        W, b = _sparse(rng, 256, 256, avoid=(big,))
        _, big = _special(rng, W, b, big)
        Ws.append(W), Bs.append(b)
    W, b = _sparse(rng, 65, 256, avoid=(big,))         # row 0: sigma; rows 1..64: the geometry features (no activation)
    _read_out(rng, W, [0], big)
    hb = int(rng.integers(1, 65))
    W[hb], b[hb] = 0.0, 0.0
    W[hb, big] = 1.0
    Ws.append(W), Bs.append(b)
    W, b = _sparse(rng, 256, 131, avoid=(hb - 1,))
    _, big = _special(rng, W, b, hb - 1)
    Ws.append(W), Bs.append(b)
    for _ in range(3):
        W, b = _sparse(rng, 256, 256, avoid=(big,))
        _, big = _special(rng, W, b, big)
        Ws.append(W), Bs.append(b)
    W, b = _sparse(rng, 3, 256, avoid=(big,))
    _read_out(rng, W, [0, 1], big)
    W[2] = 0.0
    W[2, big] = 1.0                                    # blue = 2^21 + x[:, 0] + bias
    Ws.append(W), Bs.append(b)

    h = x
    for l in range(4):
        pre = _lin(h, Ws[l], Bs[l])
        _categories(pre)
        h = _relu(pre)
    geo = _lin(h, Ws[4], Bs[4])
    h = np.concatenate([geo[:, 1:], x[:, :35], x[:, 36:]], -1)
    for l in range(5, 9):
        pre = _lin(h, Ws[l], Bs[l])
        _categories(pre, neg_zero=l > 5)
        h = _relu(pre)
    rgb = _lin(h, Ws[9], Bs[9])
    want = np.concatenate([rgb, geo[:, :1]], -1)
    assert (want != 0).any(0).all() and (np.abs(want[:, 2]) > 2.0 ** 20).all()
    return x, Ws, Bs, want


@pytest.fixture(scope='module')
def m16_case():
    return _m16_case()


@pytest.mark.parametrize('n,direct', _with_direct(M16_N))
def test_canonical_mlp_exact(ops, m16_case, n, direct):
    """Bit-exact against the restatement; column 4 and the guard rows stay untouched (as test_canonical_mlp_ragged).
    direct: the 32-sample-wave direct-load kernel of mlp.hip (canonical_mlp_kernel) on the same case, 2^21 rows included."""
    x, Ws, Bs, want = m16_case
    packed = ops.canonical_mlp_pack([T(w) for w in Ws], [T(b) for b in Bs])
    raw = torch.full((n + 3, 5), 7.0, device=DEV)
    ops.canonical_mlp(T(x[:n]), packed, raw[:n], direct=direct)
    got = raw.cpu().numpy()
    bad = got[:n, :4].view(np.int32) != want[:n].view(np.int32)
    assert not bad.any(), (int(bad.sum()), got[:n, :4][bad][:4], want[:n][bad][:4])
    assert (got[:n, 4] == 7.0).all() and (got[n:] == 7.0).all()


# ------------------------------------------------------------------------------------------------------------------
# non-rigid MLP: [cond69, emb36] -> 4 x 128 -> [h, emb36] -> 128 -> 128 -> 3.  The embedding columns of layer 0 and of the
# skip layer are zero, so the offset is a function of the condition vector and the biases alone.
# ------------------------------------------------------------------------------------------------------------------
# 389 = 4 tiles (one per workgroup; the stream wraps within each); 65 665 = 514 tiles on the 512 persistent workgroups,
# so two of them walk a second tile with the ring still running
NR16_N = (1, 31, 32, 33, 128, 129, 389, 65665)


def _nr16_case():
    rng = np.random.default_rng(9)
    cond = (rng.integers(-4, 5, 69) / 4).astype(np.float32)
    cond[:8] = [-1.0, 0.25, -0.5, 1.0, 0.0, 0.75, -0.25, 0.5]
    Ws, Bs = [], []
    W, b = _sparse(rng, 128, 69, avoid=(3,))
    nz, big = _special(rng, W, b, 3, neg_mask=cond < 0)
    b[big] = BIG                                       # 2^21 + cond[3]
    E = np.zeros((128, 36), np.float32)
    E[nz] = -0.0                                       # (the even samples' sines and cosines are >= +0)
    Ws.append(np.concatenate([W, E], 1)), Bs.append(b)
    for l in range(1, 6):
        W, b = _sparse(rng, 128, 128, avoid=(big,))
        nz, big = _special(rng, W, b, big)
        if l == 4:                                     # the skip layer: [h, emb], the -0.0 row -0.0 throughout
            E = np.zeros((128, 36), np.float32)
            E[nz] = -0.0
            W = np.concatenate([W, E], 1)
        Ws.append(W), Bs.append(b)
    W, b = _sparse(rng, 3, 128, avoid=(big,))
    _read_out(rng, W, [0, 1], big)
    W[2] = 0.0
    W[2, big] = 1.0                                    # z offset = 2^21 + cond[3] + bias
    Ws.append(W), Bs.append(b)

    h = cond[None]
    for l in range(6):
        pre = _lin(h, Ws[l][:, :69] if l == 0 else Ws[l][:, :128], Bs[l])
        _categories(pre)
        h = _relu(pre)
    off = _lin(h, Ws[6], Bs[6])[0]
    assert (off != 0).all()

    n = max(NR16_N)
    xyz = (rng.integers(-64, 65, (n, 3)) / 64).astype(np.float32)
    xyz[0::2] = (rng.integers(0, 11, (xyz[0::2].shape)) / 256).astype(np.float32)    # sin, cos of every octave >= +0
    return cond, Ws, Bs, xyz, off.astype(np.float32)


@pytest.fixture(scope='module')
def nr16_case():
    return _nr16_case()


@pytest.mark.parametrize('n,direct', _with_direct(NR16_N))
def test_nonrigid_exact(ops, nr16_case, n, direct):
    """direct: the direct-load kernel of nonrigid.hip (nonrigid_kernel, ceil(N / 128) workgroups) on the same case"""
    cond, Ws, Bs, xyz, off = nr16_case
    Wd, Bd = [T(w) for w in Ws], [T(b) for b in Bs]
    packed = ops.nonrigid_pack(Wd, Bd)
    buf = torch.full((n + 2, 3), 5.0, device=DEV)
    buf[:n] = T(xyz[:n])
    ops.nonrigid(buf[:n], T(cond), np.ones(6, np.float32), Wd[0], Bd[0], packed, out=buf[:n], direct=direct)
    got = buf.cpu().numpy()
    want = xyz[:n] + off[None]                         # one fp32 addition per coordinate, as the kernel's
    bad = got[:n].view(np.int32) != want.view(np.int32)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], got[:n][bad][:4], want[bad][:4])
    assert (got[n:] == 5.0).all()


def test_nonrigid_rows_equals_dense(ops):
    """The kernel on a row list (device-side count two short of the list) == the dense launch, bit for bit, with random
    weights and the embedding on; rows outside the list keep their bits."""
    ctx = util.model_context(0, False)
    W, B = util.nonrigid_params(ctx['sd'])
    Wd, Bd = [T(w) for w in W], [T(b) for b in B]
    packed = ops.nonrigid_pack(Wd, Bd)
    rng = np.random.default_rng(389)
    n = 389
    xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    cond = (rng.standard_normal(69) * 0.3).astype(np.float32)
    hann = np.array([1, 1, 0.75, 0.25, 0, 0], np.float32)
    dense = ops.nonrigid(T(xyz), T(cond), hann, Wd[0], Bd[0], packed).cpu().numpy()
    rows = torch.arange(0, n, 3, device=DEV, dtype=torch.int32)
    count = torch.tensor([rows.numel() - 2], device=DEV, dtype=torch.int32)
    got = ops.nonrigid_rows(T(xyz).clone(), rows, count, T(cond), hann, Wd[0], Bd[0], packed).cpu().numpy()
    sel = rows.cpu().numpy()[:rows.numel() - 2]
    keep = np.ones(n, bool)
    keep[sel] = False
    assert np.array_equal(got[sel].view(np.int32), dense[sel].view(np.int32))
    assert np.array_equal(got[keep].view(np.int32), xyz[keep].view(np.int32))
    assert (dense.view(np.int32) != xyz.view(np.int32)).mean() > 0.5       # (the kernel moved the samples it was given)
