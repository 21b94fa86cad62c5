"""Seeded cases on which the split-operand MLP kernels are exact (tests/split_mlp_restatement.py asserts it, per accumulator).

The construction, for a policy with weight lo-piece step eps (2^-11 for F16x3 and fp32, 2^-8 for Bf16x3):
  * inputs are multiples of 1/4 in [-1, 1], biases multiples of 1/4;
  * ORDINARY rows carry two weights of +-1/2 on ordinary columns of the layer before: the magnitude stays put, one fractional bit
    is added per layer, about half of the pre-activations come out negative;
  * a CONSTANT row per layer: zero weights, bias 3/4;
  * from layer 1 on, six LO rows: +-(1 + eps) on the constant row of the layer before (a non-zero Wl'; four + and two -, so
    that the lo products cannot cancel in a head's sum) and 1 on a lo row of
    the layer before (layer 1: on an ordinary row).  Their values carry many bits (xl != 0 in thousands of entries) and travel
    on with weight 1 only, so no further bits are added to them;
  * the DROPPED-LO sub-case: layer 0 has a row of value 1, layer 1 a row (1 + eps) * 1 = 1 + eps, whose split has xl != 0
    (a tie, rounded to even), and layer 2 a row (1 + eps) * (1 + eps): the kernels compute 1 + 2 eps, W x - Wl xl, where the
    full product is 1 + 2 eps + eps^2.  The value travels on with weight 1 to an output of its own;
  * a CARRY row per layer holds 1024 + x (weight 1 on the carry row before; the high end of the fp16 range -- the domain ends
    at 4094, so the 2^21 of the fp32 exact test cannot be used) and goes to an output of its own;
  * a PROBE row per layer for the domain tests, read on by the next layer's carry row with weight 1/4 so that nothing behind it
    leaves the domain.  Canonical: a SELECTOR row carries a 0/1 input column from layer to layer and the probe row is
    P * selector (P = 1 in the base case), so that a probe value reaches chosen samples only.  Non-rigid: the only per-sample
    input is the embedding, which is exact at xyz = 0 only, so the probe row has zero weights and bias P (1/4 in the base
    case) and reaches every sample.
Every layer has its own weights and row positions, every column of every layer reaches an output, the outputs are
non-zero.  No zero signs are asked for: a zero lo weight contributes +0 products, so -0.0 does not survive in these kernels.

Non-rigid case (A): zero embedding weights, arbitrary dyadic xyz.  Case (B): xyz = 0 for every sample, so sin = 0 and
cos = 1 exactly and the embedding operands are the Hann window's values; each of the 36 embedding columns of layer 0 and of
the skip layer carries a distinct non-zero dyadic weight on a row of its own (value 1 + weight * window, never clipped by
the ReLU), and the next layer's lo rows carry these rows to the output with weight 1: every cosine column with an open
window moves the output, the sine columns and the closed octaves contribute exactly nothing.  (The three cosine columns of
one octave hold the same operand at the origin: they are told apart by their rows' weights only.)
"""
import numpy as np

from tests import split_mlp_restatement as R

F32 = np.float32
N_LO = 6
HANN_B = ((1, 1, 1, 1, 1, 1), (1, 1, .75, .25, 0, 0), (0, 0, 0, 0, 0, 0))


def eps_of(policy):
    return 2.0 ** -8 if policy == 'bf16x3' else 2.0 ** -11


class _Layer:
    """rows of one layer by role; `prev`: the roles' columns in the layer's input"""

    def __init__(self, rng, out_dim, in_dim, roles):
        self.W = np.zeros((out_dim, in_dim), F32)
        self.b = np.zeros(out_dim, F32)
        self.rows = {}
        perm = rng.permutation(out_dim)
        at = 0
        for name, count in roles:
            self.rows[name] = [int(r) for r in perm[at:at + count]]
            at += count
        self.rows['ord'] = [int(r) for r in perm[at:]]

    def one(self, name):
        return self.rows[name][0] if self.rows.get(name) else None


def _ordinary(rng, L, cols, cover=True):
    """two weights of +-1/2 per ordinary row, every column of `cols` used (cover); bias a multiple of 1/4 in [-1, 1]"""
    rows = L.rows['ord']
    seq = np.resize(rng.permutation(np.asarray(cols)), 2 * len(rows))
    for i, r in enumerate(rows):
        assert seq[2 * i] != seq[2 * i + 1]
        L.W[r, seq[2 * i]] = rng.choice([0.5, -0.5])
        L.W[r, seq[2 * i + 1]] = rng.choice([0.5, -0.5])
        L.b[r] = rng.integers(-4, 5) / 4
    assert not cover or 2 * len(rows) >= len(cols), 'every ordinary column must be read'


def _specials(rng, L, prev, eps, ord_cols, first_lo):
    """const / lo / drop / carry rows of a layer whose input has the roles `prev` (name -> column(s))"""
    c = L.one('const')
    L.b[c] = 0.75
    signs = rng.permutation([1.0, 1.0, 1.0, 1.0, -1.0, -1.0])      # (unequal counts: the lo products do not cancel in the head's sum)
    for i, r in enumerate(L.rows.get('lo', [])):
        sign = signs[i]
        L.W[r, prev['const']] = sign * (1.0 + eps)
        L.W[r, int(rng.choice(ord_cols)) if first_lo else prev['lo'][i]] = 1.0
        L.b[r] = 1.0 if sign < 0 or first_lo else rng.integers(0, 3) / 4
        for c in prev.get('emb', [])[i::N_LO]:               # (non-rigid: the embedding rows of the layer before, one per octave)
            L.W[r, c] = 1.0
    if L.one('one') is not None:
        L.b[L.one('one')] = 1.0
    if L.one('drop') is not None:
        L.W[L.one('drop'), prev['drop']] = (1.0 + eps) if prev['drop_stage'] < 2 else 1.0
    if prev.get('carry') is not None:
        L.W[L.one('carry'), prev['carry']] = 1.0
    if prev.get('probe') is not None:
        L.W[L.one('carry'), prev['probe']] = 0.25


def _roles_of(L, stage):
    out = {'const': L.one('const'), 'lo': L.rows.get('lo', []), 'carry': L.one('carry'), 'probe': L.one('probe'),
           'sel': L.one('sel'), 'ord': L.rows['ord'], 'emb': L.rows.get('emb', [])}
    if L.one('one') is not None:
        out['drop'], out['drop_stage'] = L.one('one'), 0
    elif L.one('drop') is not None:
        out['drop'], out['drop_stage'] = L.one('drop'), stage
    return out


def _read_rows(rng, W, row, roles, width, exclude):
    """a general head row: +-1/2 on every column but `exclude`, 1 on the lo columns"""
    for c in range(width):
        if c not in exclude:
            W[row, c] = 1.0 if c in roles['lo'] else rng.choice([0.5, -0.5])


# ---------------------------------------------------------------------------------------------------------------------------
# canonical: x[68] -> 4 x 256 -> (sigma, geo64); [geo64, agg35, enc32] -> 4 x 256 -> (red: general, green: the dropped-lo
# value, blue: the carry).  Input columns: C0 feeds the carry, SEL is the 0/1 selector, 35 (var) is the probe of the input site.
# ---------------------------------------------------------------------------------------------------------------------------
C0, SEL, VAR = 0, 34, 35
CANONICAL_PROBES = ('geo0', 'geo1', 'geo2', 'geo3', 'head', 'rgb0', 'rgb1', 'rgb2', 'rgb3')


def canonical_case(policy, n, selected=(0,), probe=None, x_probe=None):
    """-> x[n, 68], Ws, Bs.  probe = (layer name, P): that layer's probe weight; x_probe: the value of input column `var` for the
    selected samples (the input site).  Everything else is the same for every call with the same policy."""
    eps = eps_of(policy)
    rng = np.random.default_rng(2048 if policy == 'bf16x3' else 2049)
    xs = (rng.integers(-4, 5, (512, 68)) / 4).astype(F32)
    xs[:, SEL] = 0.0
    Ws, Bs = [], []
    P = dict.fromkeys(CANONICAL_PROBES, 1.0)
    if probe is not None:
        P[probe[0]] = probe[1]

    def hidden(name, in_dim, prev, stage, sel_col, in_ord, first_lo=False, l0=False):
        roles = [('const', 1), ('carry', 1), ('sel', 1), ('probe', 1)]
        roles += [('one', 1)] if l0 else [('drop', 1), ('lo', N_LO)]
        L = _Layer(rng, 256, in_dim, roles)
        _ordinary(rng, L, in_ord)
        _specials(rng, L, prev, eps, in_ord, first_lo)
        L.W[L.one('sel'), sel_col] = 1.0
        L.W[L.one('probe'), sel_col] = P[name]
        Ws.append(L.W), Bs.append(L.b)
        return _roles_of(L, stage)

    # geometry trunk
    roles = hidden('geo0', 68, {'const': None, 'lo': [], 'carry': C0, 'probe': VAR}, 0, SEL,
                   [c for c in range(68) if c not in (C0, SEL, VAR)], l0=True)
    Bs[0][roles['carry']] = 1024.0
    for l in range(1, 4):
        roles = hidden('geo%d' % l, 256, roles, min(l, 2), roles['sel'], roles['ord'], first_lo=l == 1)
    # head: row 0 sigma (general: everything but the carry, the probe and the dropped-lo value), rows 1..64 the geometry features
    H = _Layer(rng, 64, 256, [('const', 1), ('carry', 1), ('probe', 1), ('drop', 1), ('lo', N_LO)])
    _ordinary(rng, H, roles['ord'], cover=False)      # (sigma reads every column)
    _specials(rng, H, roles, eps, roles['ord'], False)
    H.W[H.one('probe'), roles['sel']] = P['head']
    W4, b4 = np.zeros((65, 256), F32), np.zeros(65, F32)
    W4[1:], b4[1:] = H.W, H.b
    _read_rows(rng, W4, 0, roles, 256, (roles['carry'], roles['probe'], roles['drop']))
    b4[0] = 0.25
    Ws.append(W4), Bs.append(b4)
    groles = _roles_of(H, 2)
    # colour trunk: input [geo64, agg35, enc32]; the selector comes from the input column again
    xcol = lambda c: 64 + (c if c < 35 else c - 1)
    in_ord = list(groles['ord']) + [xcol(c) for c in range(68) if c not in (SEL, VAR)]
    roles = hidden('rgb0', 131, groles, 2, xcol(SEL), in_ord)
    for l in range(1, 4):
        roles = hidden('rgb%d' % l, 256, roles, 2, roles['sel'], roles['ord'])
    W9, b9 = np.zeros((3, 256), F32), np.asarray([0.25, 0.0, 0.5], F32)
    _read_rows(rng, W9, 0, roles, 256, (roles['carry'], roles['probe'], roles['drop']))
    W9[1, roles['drop']] = 1.0
    W9[2, roles['carry']], W9[2, roles['probe']] = 1.0, 0.25
    Ws.append(W9), Bs.append(b9)

    x = xs[:n].copy()
    sel = np.asarray(selected, np.int64)
    x[sel, SEL] = 1.0
    if x_probe is not None:
        x[sel, VAR] = x_probe
    return x, Ws, Bs


# ---------------------------------------------------------------------------------------------------------------------------
# non-rigid: [cond69, emb36] -> 4 x 128 -> [h, emb36] -> 128 -> 128 -> (x: general, y: the dropped-lo value, z: the carry)
# ---------------------------------------------------------------------------------------------------------------------------
NONRIGID_PROBES = ('nr0', 'nr1', 'nr2', 'nr3', 'skip', 'nr5')
CC0 = 3


def nonrigid_case(policy, n, embed=False, probe=None):
    """-> cond[69], Ws, Bs, xyz[n, 3].  embed: case (B), xyz = 0 and distinct weights on the embedding columns, else case (A)."""
    eps = eps_of(policy)
    rng = np.random.default_rng(128 if policy == 'bf16x3' else 129)
    cond = (rng.integers(-4, 5, 69) / 4).astype(F32)
    xyz = (rng.integers(-64, 65, (512, 3)) / 64).astype(F32)
    P = dict.fromkeys(NONRIGID_PROBES, 0.25)
    if probe is not None:
        P[probe[0]] = probe[1]
    Ws, Bs = [], []

    def hidden(name, in_dim, prev, stage, in_ord, first_lo=False, l0=False, emb_base=None):
        roles = [('const', 1), ('carry', 1), ('probe', 1)]
        roles += [('one', 1)] if l0 else [('drop', 1), ('lo', N_LO)]
        roles += [('emb', 36)] if emb_base is not None else []
        L = _Layer(rng, 128, in_dim, roles)
        _ordinary(rng, L, in_ord)
        _specials(rng, L, prev, eps, in_ord, first_lo)
        L.b[L.one('probe')] = P[name]
        # EMBEDDING rows: row c of them is 1 + w_c * (embedding column c), w_c = (c + 1) / 32 in case (B) and 0 in case (A); the
        # next layer's lo rows sum them with weight 1 (one per octave each) and carry them to the output with weight 1
        for c, r in enumerate(L.rows.get('emb', [])):
            L.b[r] = 1.0
            if embed:
                L.W[r, emb_base + c] = (c + 1) / 32
        Ws.append(L.W), Bs.append(L.b)
        return L, _roles_of(L, stage)

    L, roles = hidden('nr0', 69 + 36, {'const': None, 'lo': [], 'carry': CC0, 'probe': None}, 0,
                      [c for c in range(69) if c != CC0], l0=True, emb_base=69)
    Bs[0][roles['carry']] = 1024.0
    for l in range(1, 4):
        L, roles = hidden('nr%d' % l, 128, roles, min(l, 2), roles['ord'], first_lo=l == 1)
    L, roles = hidden('skip', 128 + 36, roles, 2, roles['ord'], emb_base=128)
    L, roles = hidden('nr5', 128, roles, 2, roles['ord'])
    W6, b6 = np.zeros((3, 128), F32), np.asarray([0.25, 0.0, 0.5], F32)
    _read_rows(rng, W6, 0, roles, 128, (roles['carry'], roles['probe'], roles['drop']))
    W6[1, roles['drop']] = 1.0
    W6[2, roles['carry']], W6[2, roles['probe']] = 1.0, 0.25
    Ws.append(W6), Bs.append(b6)
    return cond, Ws, Bs, (np.zeros((n, 3), F32) if embed else xyz[:n].copy())


def check_canonical(policy, x, Ws, Bs):
    """the restatement of a canonical case with the properties the construction promises -> (raw, flags, stats)"""
    ev = R.Exact(R.POLICIES[policy])
    raw, flags = R.canonical(ev, Ws, Bs, x)
    assert (raw != 0).all()
    return raw, flags, ev.stats


def check_nonrigid(policy, cond, Ws, Bs, hann, xyz):
    ev = R.Exact(R.POLICIES[policy])
    out, flags = R.nonrigid(ev, Ws, Bs, cond, hann, xyz)
    assert ((out - np.asarray(xyz, F32)) != 0).all()
    return out, flags, ev.stats
