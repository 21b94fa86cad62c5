"""NumPy restatement of the split-operand MLP kernels (csrc/mlp.hip, csrc/nonrigid.hip) under the precision policies of
csrc/split.h, with float64 bookkeeping that PROVES, case by case, that the result does not depend on the order of the
k-steps or on any intermediate precision of at least fp32.  On such a case a kernel must return the restatement's bits.

The policies (split.h):
  * rd: F16x3 rounds to fp16 (np.float16), Bf16x3 rounds to bfloat16 (RNE on the bit pattern), fp32 is the identity (the two
    direct-load fp32 kernels: one piece, no lo product);
  * weights: Wh = rd(W), Wl' = rd((W - Wh) s), s = 2^11 (F16x3: w_lo) or 1;
  * activations travel scaled by kSx (16 for F16x3, else 1): v = kSx x in fp32, clamped by P::sym (signed) or P::relu, then
    xh = rd(v), xl = rd(v - xh), x3 = P::third(xh) = rd(xh 2^-11) for F16x3 (a packed-half multiply), xh otherwise;
  * one MFMA layer: acc = kSx b + sum_k (Wh xh + Wh xl + Wl' x3).  That is W x - Wl xl: the lo-lo product is DROPPED, and
    the restatement pins what is computed, not what would be better;
  * the heads (sigma, rgb, the non-rigid offset) are fp32 dot rows over max(acc, 0) of the last hidden layer -- NOT clamped, not
    split -- and return (sum) (1 / kSx) + b: the division comes before the bias.

What makes a case exact (asserted per accumulator by `Exact`, never assumed):
  * the split of every weight and of every activation that meets a non-zero weight is lossless: Wh + Wl'/s == W, xh + xl == v
    (an operand column whose weights are all zero contributes +0 whatever it holds and is left out; it must be finite);
  * every x3 that meets a non-zero Wl' is zero or a NORMAL fp16 number (|x3| >= 2^-14), so nothing depends on how the
    packed-half multiply treats subnormal results;
  * the sum of the absolute terms (scaled bias included) is below 2^24 times the lowest set bit among them: every partial sum,
    in any order, is then a multiple of that bit below 2^24 of it and fp32 holds it exactly.
A zero lo weight contributes +0 products, so a -0.0 pre-activation cannot survive in these kernels; the cases ask for no
zero signs and their outputs are non-zero.

The domain watch (F16x3 only; kBound = 65504 is the largest fp16 number).  The numbers are consequences of split.h, not
tolerances:
  * a ReLU site clamps v by fmed3(v, 0, 65504) and watches the HI pieces (watch_hi, left_domain: hi >= 65504), so it reports
    iff rd(min(v, 65504)) == 65504.  fp16 has 11 significand bits; in [32768, 65536) its spacing is 32, the neighbours of
    65504 = 2047 * 32 are 65472 = 2046 * 32 (even) and infinity, and the tie 65488 goes to the even 65472.  So the site reports
    iff v > 65488 = 16 * 4093: an activation of 4093 is the last one that is clear (and exact: hi 65472, lo 16), 4094 = 65504 / 16
    is the first dyadic multiple of 1/16-th that reports;
  * a signed site (the inputs, the geometry head) is watched in fp32, watch_abs: |v| >= 65504, i.e. an activation at or beyond
    4094 = 65504 / 16; +-4093.5 is clear and exact (v = 65496 < 65504 passes the clamp unchanged; its hi piece is 65504, its lo
    piece -8 -- a signed site watches the fp32 value, not the hi piece);
  * the last hidden layer of the colour trunk and of the non-rigid trunk feeds the fp32 dot rows through fmaxf: neither
    clamped nor watched, so 5000 there is exact and silent.
The canonical kernel has nine watched sites (in, geo0..geo3, head, rgb0..rgb2), the non-rigid kernel five (nr0..nr3, skip).

`Emulated` is the same network evaluated in fp32 in the kernels' own k-step order (mlp_layout.h: slot_feature), with
optional planted defects; tests/test_split_mlp_restatement.py shows that it passes every check and that every defect fails
the check named for it.
"""
import collections

import numpy as np

F32 = np.float32
BOUND = 65504.0

Policy = collections.namedtuple('Policy', 'name ksx s bounded')
F16X3 = Policy('f16x3', 16.0, 2048.0, True)
BF16X3 = Policy('bf16x3', 1.0, 1.0, False)
FP32 = Policy('fp32', 1.0, 1.0, False)
POLICIES = {p.name: p for p in (F16X3, BF16X3, FP32)}

CANONICAL_SITES = ('in', 'geo0', 'geo1', 'geo2', 'geo3', 'head', 'rgb0', 'rgb1', 'rgb2')
NONRIGID_SITES = ('nr0', 'nr1', 'nr2', 'nr3', 'skip')
SIGNED_SITES = ('in', 'head')


def rd_bf16(a):
    """fp32 -> bfloat16 -> fp32, round to nearest even on the bit pattern (NaN stays NaN)"""
    a = np.ascontiguousarray(a, F32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    r = np.where(np.isnan(a), np.uint32(0x7FC00000), r).astype(np.uint32)
    return r.view(F32).reshape(a.shape)


def rd(P, a):
    a = np.asarray(a, F32)
    if P.name == 'f16x3':
        with np.errstate(over='ignore'):
            return a.astype(np.float16).astype(F32)
    if P.name == 'bf16x3':
        return rd_bf16(a)
    return a


def third(P, xh):
    if P.name == 'f16x3':
        return (xh.astype(np.float16) * np.float16(2.0 ** -11)).astype(F32)      # one rounding to fp16, subnormals kept
    return xh


def split_w(P, W):
    W = np.asarray(W, F32)
    Wh = rd(P, W)
    return Wh, rd(P, (W - Wh) * F32(P.s))


def split_x(P, v):
    v = np.asarray(v, F32)
    xh = rd(P, v)
    xl = rd(P, v - xh)
    return xh, xl, third(P, xh)


def relu_clamp(P, a, bound=BOUND):
    a = np.maximum(np.asarray(a, F32), F32(0.0))
    return np.minimum(a, F32(bound)) if P.bounded else a


def sym_clamp(P, a):
    return np.clip(np.asarray(a, F32), F32(-BOUND), F32(BOUND)) if P.bounded else np.asarray(a, F32)


def embedding(xyz, hann):
    """[n, 36]: feature octave * 6 + {sin x, sin y, sin z, cos x, cos y, cos z}, each times the octave's window (fp32)"""
    xyz = np.asarray(xyz, F32)
    e = np.zeros((xyz.shape[0], 36), F32)
    for o in range(6):
        a = xyz * F32(2.0 ** o)
        e[:, o * 6:o * 6 + 3] = F32(hann[o]) * np.sin(a).astype(F32)
        e[:, o * 6 + 3:o * 6 + 6] = F32(hann[o]) * np.cos(a).astype(F32)
    return e


def _low(a):
    """log2 of the lowest set bit per entry of a float64 array, +inf for zeros"""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a)
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    tz = np.log2(np.maximum(mi & -mi, 1).astype(np.float64))
    return np.where(a == 0, np.inf, e - 53 + tz)


def _min_plus(lx, lw):
    """out[n, o] = min_k lx[n, k] + lw[o, k] over the finite entries of lw (the weights are sparse)"""
    out = np.full((lx.shape[0], lw.shape[0]), np.inf)
    o_idx, k_idx = np.nonzero(np.isfinite(lw))
    if len(o_idx):
        np.minimum.at(out, (slice(None), o_idx), lx[:, k_idx] + lw[o_idx, k_idx][None])
    return out


class Exact:
    """The restatement proper: float64 bookkeeping, every accumulator asserted exact in any order (module docstring)."""

    def __init__(self, P):
        self.P = P
        self.flags = {}
        self.stats = {'span': 0.0, 'xl_nonzero': 0, 'lo_meets_xl': 0, 'negative': []}

    def _order_free(self, terms_abs, low, what):
        ok = terms_abs < 2.0 ** (24 + low)
        span = np.where(terms_abs > 0, np.log2(np.maximum(terms_abs, 1e-300)) - low, 0.0)
        self.stats['span'] = max(self.stats['span'], float(span.max()))
        assert ok.all(), (what, self.P.name, 'an accumulator spans %.1f bits' % span.max())

    def mfma(self, v, W, b, name, kind=None):
        P = self.P
        v, b = np.asarray(v, F32), np.asarray(b, F32)
        Wh, Wl = split_w(P, W)
        W64, Wh64, Wl64 = np.asarray(W, np.float64), Wh.astype(np.float64), Wl.astype(np.float64)
        assert np.array_equal(Wh64 + Wl64 / P.s, W64), (name, 'a weight does not split losslessly')
        assert np.isfinite(v).all()
        used = ((Wh != 0) | (Wl != 0)).any(0)
        v, Wh64, Wl64 = v[:, used], Wh64[:, used], Wl64[:, used]
        xh, xl, x3 = (a.astype(np.float64) for a in split_x(P, v))
        assert np.array_equal(xh + xl, v.astype(np.float64)), (name, 'an activation does not split losslessly')
        if P.name == 'f16x3':
            m = x3[:, (Wl64 != 0).any(0)]
            assert ((m == 0) | (np.abs(m) >= 2.0 ** -14)).all(), (name, 'a subnormal x3 meets a lo weight')
        sb = np.float64(P.ksx) * b.astype(np.float64)
        assert np.array_equal((F32(P.ksx) * b).astype(np.float64), sb)
        acc = sb[None] + xh @ Wh64.T + xl @ Wh64.T + x3 @ Wl64.T
        tot = np.abs(sb)[None] + np.abs(xh) @ np.abs(Wh64).T + np.abs(xl) @ np.abs(Wh64).T + np.abs(x3) @ np.abs(Wl64).T
        lwh, lwl = _low(Wh64), _low(Wl64)
        low = np.minimum(np.minimum(_min_plus(_low(xh), lwh), _min_plus(_low(xl), lwh)),
                         np.minimum(_min_plus(_low(x3), lwl), _low(sb)[None]))
        self._order_free(tot, low, name)
        assert np.array_equal(acc.astype(F32).astype(np.float64), acc)
        self.stats['xl_nonzero'] += int((xl != 0).sum())
        self.stats['lo_meets_xl'] += int((((xl != 0).astype(np.float64) @ (Wl64 != 0).astype(np.float64).T) > 0).sum())
        self.stats['negative'].append(float((acc < 0).mean()))
        return acc.astype(F32)

    def relu(self, pre, site):
        v = relu_clamp(self.P, pre)
        if self.P.bounded:
            self.flags[site] = bool((rd(self.P, v) == F32(BOUND)).any())
        return v

    def sym(self, v, site):
        if self.P.bounded:
            self.flags[site] = bool((np.abs(v) >= F32(BOUND)).any())
        return sym_clamp(self.P, v)

    def dot(self, pre, W, b, name):
        """fp32 dot rows over the UNCLAMPED ReLU of the last hidden layer: (sum) / kSx + b"""
        h = np.maximum(np.asarray(pre, F32), F32(0.0)).astype(np.float64)
        W64, b64 = np.asarray(W, np.float64), np.asarray(b, np.float64)
        s = h @ W64.T
        self._order_free(np.abs(h) @ np.abs(W64).T, _min_plus(_low(h), _low(W64)), name)
        out = s / self.P.ksx + b64[None]
        assert np.array_equal(out.astype(F32).astype(np.float64), out), (name, 'the head is not exact in fp32')
        return out.astype(F32)

    def fold(self, W, b, cond):
        """the non-rigid layer-0 bias with the condition code folded in: an fp32 chain b + sum_k W[:, k] cond[k]"""
        W64, c64, b64 = np.asarray(W, np.float64), np.asarray(cond, np.float64), np.asarray(b, np.float64)
        out = b64 + W64 @ c64
        tot = np.abs(b64) + np.abs(W64) @ np.abs(c64)
        low = np.minimum(_min_plus(_low(c64)[None], _low(W64))[0], _low(b64))
        self._order_free(tot[None], low[None], 'fold')
        return out.astype(F32)


def hidden_steps(width):
    """the kernels' k-steps of 16 of a hidden layer: step s carries registers 8 s .. 8 s + 7 of both half-waves, register t of
    half h being feature (t >> 4) * 32 + (t & 3) + 8 * ((t & 15) >> 2) + 4 * h  (mlp_layout.h: slot_feature)"""
    steps = []
    for s in range(width // 16):
        cols = []
        for h in range(2):
            for t in range(8 * s, 8 * s + 8):
                r = t & 15
                cols.append((t >> 4) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h)
        steps.append(cols)
    return steps


def _half_steps(per_half, n_steps, base):
    return [[base + h * per_half + t for h in range(2) for t in range(8 * s, 8 * s + 8) if t < per_half] for s in range(n_steps)]


def k_steps(kind, in_dim):
    if kind == 'L0Geo':                                      # 34 inputs per half-wave, 5 steps (6 pad slots)
        return _half_steps(34, 5, 0)
    if kind == 'L0Rgb':                                      # 64 geometry features, then [agg35, var, enc32] without var
        x = [[c for c in st if c != 35] for st in _half_steps(34, 5, 0)]
        return hidden_steps(64) + [[64 + (c if c < 35 else c - 1) for c in st] for st in x]
    if kind == 'NrL0':                                       # 18 embedding features per half-wave, 3 steps
        return _half_steps(18, 3, 0)
    if kind == 'NrSkip':
        return hidden_steps(128) + _half_steps(18, 3, 128)
    return hidden_steps(in_dim)


class Emulated:
    """The kernels' arithmetic in fp32, k-step by k-step, three products per step; `defect` plants one error:
      ('drop3', layer, step)  the third product missing in one k-step      ('twice',)        2^-11 applied twice (x3)
      ('swap', layer, step)   hi and lo weight pieces of one chunk swapped  ('bias', layer)   a bias not scaled by kSx
      ('late', head)          a head's 1/kSx applied after its bias         ('clamp',)        the ReLU clamp at 65472
      ('unsplit', layer)      the layer's first 64 operands fed unsplit     ('skipstep', layer, step)  a k-step skipped
      ('lolo',)               Wl xl added                                   ('nowatch', site) a site not watched"""

    def __init__(self, P, defect=None):
        self.P = P
        self.defect = defect or ('none',)
        self.flags = {}

    def _is(self, *d):
        return self.defect[:len(d)] == d

    def mfma(self, v, W, b, name, kind=None):
        P = self.P
        Wh, Wl = split_w(P, W)
        xh, xl, x3 = split_x(P, v)
        if self._is('twice'):
            x3 = third(P, x3)
        if self._is('unsplit', name):
            xl = xl.copy()
            xl[:, :64] = 0.0
        b = np.asarray(b, F32)
        acc = np.broadcast_to(b if self._is('bias', name) else F32(P.ksx) * b, (xh.shape[0], Wh.shape[0])).astype(F32)
        for s, cols in enumerate(k_steps(kind, Wh.shape[1])):
            if self._is('skipstep', name, s):
                continue
            A, L = Wh[:, cols], Wl[:, cols]
            if self._is('swap', name, s):
                A, L = L, A
            acc = acc + xh[:, cols] @ A.T
            acc = acc + xl[:, cols] @ A.T
            if not self._is('drop3', name, s):
                acc = acc + x3[:, cols] @ L.T
            if self._is('lolo'):
                acc = acc + xl[:, cols] @ (L / F32(P.s)).T
            assert acc.dtype == F32
        return acc

    def relu(self, pre, site):
        v = relu_clamp(self.P, pre, 65472.0 if self._is('clamp') else BOUND)
        if self.P.bounded and not self._is('nowatch', site):
            self.flags[site] = bool((rd(self.P, v) >= F32(BOUND)).any())          # the running maximum of the hi pieces
        elif self.P.bounded:
            self.flags[site] = False
        return v

    def sym(self, v, site):
        if self.P.bounded:
            self.flags[site] = bool((np.abs(v) >= F32(BOUND)).any()) and not self._is('nowatch', site)
        return sym_clamp(self.P, v)

    def dot(self, pre, W, b, name):
        h = np.maximum(np.asarray(pre, F32), F32(0.0))
        W, b = np.asarray(W, F32), np.asarray(b, F32)
        s = np.zeros((h.shape[0], W.shape[0]), F32)
        for k in range(W.shape[1]):
            s = s + h[:, k:k + 1] * W[None, :, k]
        inv = F32(1.0 / self.P.ksx)
        return (s + b[None]) * inv if self._is('late', name) else s * inv + b[None]

    def fold(self, W, b, cond):
        acc = np.asarray(b, F32).copy()
        for k in range(W.shape[1]):
            acc = acc + np.asarray(W, F32)[:, k] * F32(cond[k])
        return acc


# ---------------------------------------------------------------------------------------------------------------------------
# the two trunk shapes, over either evaluator
# ---------------------------------------------------------------------------------------------------------------------------
def canonical(ev, Ws, Bs, x):
    """x[n, 68] = [agg35, var, enc32] -> (raw[n, 4] = rgb, sigma; flags per watched site)"""
    P = ev.P
    v0 = ev.sym(F32(P.ksx) * np.asarray(x, F32), 'in')
    pre = ev.mfma(v0, Ws[0], Bs[0], 'geo0', 'L0Geo')
    for l in range(1, 4):
        pre = ev.mfma(ev.relu(pre, 'geo%d' % (l - 1)), Ws[l], Bs[l], 'geo%d' % l)
    sigma = ev.dot(pre, Ws[4][:1], Bs[4][:1], 'sigma')
    geo = ev.mfma(ev.relu(pre, 'geo3'), Ws[4][1:], Bs[4][1:], 'head')
    vin = np.concatenate([ev.sym(geo, 'head'), v0[:, :35], v0[:, 36:]], 1)
    pre = ev.mfma(vin, Ws[5], Bs[5], 'rgb0', 'L0Rgb')
    for l in range(1, 4):
        pre = ev.mfma(ev.relu(pre, 'rgb%d' % (l - 1)), Ws[5 + l], Bs[5 + l], 'rgb%d' % l)
    rgb = ev.dot(pre, Ws[9], Bs[9], 'rgb')
    return np.concatenate([rgb, sigma], 1), dict(ev.flags)


def nonrigid(ev, Ws, Bs, cond, hann, xyz):
    """-> (xyz + offset, flags per watched site)"""
    P = ev.P
    xyz = np.asarray(xyz, F32)
    b0 = ev.fold(np.asarray(Ws[0])[:, :69], Bs[0], cond)
    ve = F32(P.ksx) * embedding(xyz, hann)
    pre = ev.mfma(ve, np.asarray(Ws[0])[:, 69:], b0, 'nr0', 'NrL0')
    for l in range(1, 4):
        pre = ev.mfma(ev.relu(pre, 'nr%d' % (l - 1)), Ws[l], Bs[l], 'nr%d' % l)
    pre = ev.mfma(np.concatenate([ev.relu(pre, 'nr3'), ve], 1), Ws[4], Bs[4], 'skip', 'NrSkip')
    pre = ev.mfma(ev.relu(pre, 'skip'), Ws[5], Bs[5], 'nr5')
    off = ev.dot(pre, Ws[6], Bs[6], 'off')
    return xyz + off, dict(ev.flags)


def plain_canonical(Ws, Bs, x):
    """x @ W.T + b through the canonical network in float64"""
    W = [np.asarray(w, np.float64) for w in Ws]
    B = [np.asarray(b, np.float64) for b in Bs]
    x = np.asarray(x, np.float64)
    h = x
    for l in range(4):
        pre = h @ W[l].T + B[l]
        h = np.maximum(pre, 0)
    head = h @ W[4].T + B[4]
    h = np.concatenate([head[:, 1:], x[:, :35], x[:, 36:]], 1)
    for l in range(5, 9):
        h = np.maximum(h @ W[l].T + B[l], 0)
    return np.concatenate([h @ W[9].T + B[9], head[:, :1]], 1)


def plain_nonrigid(Ws, Bs, cond, hann, xyz):
    W = [np.asarray(w, np.float64) for w in Ws]
    B = [np.asarray(b, np.float64) for b in Bs]
    e = embedding(xyz, hann).astype(np.float64)
    h = np.concatenate([np.broadcast_to(np.asarray(cond, np.float64), (e.shape[0], 69)), e], 1)
    for l in range(6):
        if l == 4:
            h = np.concatenate([h, e], 1)
        h = np.maximum(h @ W[l].T + B[l], 0)
    return np.asarray(xyz, np.float64) + h @ W[6].T + B[6]
