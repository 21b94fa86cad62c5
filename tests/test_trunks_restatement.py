"""CPU: the float64 restatements and the bound / interval helpers of tests/trunks_restatement.py, before the GPU tests
(tests/test_n_trunks_per_entry.py) rely on them:

  * the restated chain of ten launches and its hand-derived backward against torch autograd (float64) over CanonicalMLP's layers;
  * an emulated kernel (fp32 accumulation in two orders, RNE store) stays inside every check, every random case keeps the share
    of two-valued intervals under its cap, every dyadic case is dyadic;
  * eight planted defects, each failing the check that is meant to catch it (matched by that check's message)."""
import numpy as np
import pytest
import torch

from tests import trunks_cases as cases
from tests import trunks_restatement as tr

F32 = np.float32


# ---- restatement against torch --------------------------------------------------------------------------------------------
def _close(name, got, want):
    """1e-12 relative per entry; an entry that cancels far below its tensor's typical size is held to that size instead (the two
    float64 evaluations sum up to 512 terms in different orders: 512 x 2^-53 of the terms' size, not of their sum)."""
    want = np.asarray(want, np.float64)
    tol = 1e-12 * np.maximum(np.abs(want), np.mean(np.abs(want)))
    bad = ~(np.abs(got - want) <= tol)
    assert not bad.any(), (name, int(bad.sum()), float(np.max(np.abs(got - want) / tol)))


def test_restated_chain_and_backward_match_torch_autograd():
    from occnerf_amd.canonical_mlp import CanonicalMLP
    cm = CanonicalMLP(mlp_depth=4, mlp_width=256, skips=[]).double()
    Ws, bs = cases.random_network(1)
    mods = [cm.get_submodule(n) for n in tr.LAYERS]
    assert [tuple(m.weight.shape) for m in mods] == tr.SHAPES
    with torch.no_grad():
        for m, W, b in zip(mods, Ws, bs):
            m.weight.copy_(torch.from_numpy(W))
            m.bias.copy_(torch.from_numpy(b))
    agg, var, enc, gout = cases.step_inputs(37, False)
    ta, tv, te = (torch.from_numpy(a).requires_grad_(True) for a in (agg, var, enc))
    h = torch.cat([ta, tv, te], -1)                                    # occnerf_mlp.py:183-199
    for layer in cm.pts_linears:
        h = layer(h)
    h = cm.geo_linear(h)
    sigma = h[..., [0]]
    h = torch.cat([h[..., 1:], ta, te], -1)
    for layer in cm.rgb_linears:
        h = layer(h)
    raw = torch.cat((cm.output_linear(h), sigma), -1)
    (raw * torch.from_numpy(gout)).sum().backward()

    fw = tr.chain_forward(Ws, bs, agg, var, enc)
    _close('raw4', fw['raw4'], raw.detach().numpy())
    dx0, dW, db = tr.chain_backward(fw, gout)
    _close('agg.grad', dx0[:, :35], ta.grad.numpy())
    _close('enc.grad', dx0[:, 36:68], te.grad.numpy())
    assert not dx0[:, 68:].any()
    for n, m, w, b in zip(tr.LAYERS, mods, dW, db):
        _close(n + '.weight', w, m.weight.grad.numpy())
        _close(n + '.bias', b, m.bias.grad.numpy())


def test_maps_are_the_layout():
    maps = tr.trunk_maps()
    assert [len(r) for r in maps['rows']] == [256] * 4 + [96] + [256] * 4 + [32]
    assert [len(c) for c in maps['cols']] == [96] + [256] * 4 + [192] + [256] * 4
    for l, (o, i) in enumerate(tr.SHAPES):                             # every weight entry is reached exactly once
        r, c = maps['rows'][l], maps['cols'][l]
        assert sorted(r[r >= 0]) == list(range(o)) and sorted(c[c >= 0]) == list(range(i)), l
    s0, s1 = maps['rgb_seg0'], maps['rgb_seg1']
    assert not set(s0[s0 >= 0]) & set(s1[s1 >= 0]) and s0[64] == -1 and s1[35] == -1     # sigma and var: no colour input
    assert maps['rows'][4][64] == 0 and maps['rows'][4][0] == 1


def test_bf16_rounding_helpers():
    g = np.random.default_rng(0)
    x = np.concatenate([g.standard_normal(4000) * 10.0 ** g.integers(-30, 30, 4000), [0.0, -0.0, 1.0, 1.00390625, 1.01171875,
                                                                                    2.0 ** -133 * 1.5, 2.0 ** -134, 255.5, 256.5]])
    want = torch.from_numpy(x.astype(F32)).bfloat16().double().numpy()                   # (torch rounds fp32 -> bf16 RNE)
    x32 = x.astype(F32).astype(np.float64)
    assert np.array_equal(tr.bf16_rne(x32), want)
    assert tr.bf16_rne(1.00390625) == 1.0 and tr.bf16_rne(1.01171875) == 1.015625        # ties go to even
    assert tr.bf16_rne(1.0 + 2.0 ** -8 + 2.0 ** -40) == 1.0078125                        # one rounding, not through fp32
    v = tr.bf16_rne(x32[np.abs(x32) > 1e-30])
    up = tr.bf16_ulp_up(v)
    assert tr.is_bf16(up) and np.all(up > v) and np.all(tr.bf16_rne((up + v) / 2 + (up - v) / 8) == up)
    assert np.all(np.abs(tr.bf16_trunc(x32)) <= np.abs(x32)) and tr.is_bf16(tr.bf16_trunc(x32))


# ---- the emulated kernel --------------------------------------------------------------------------------------------------
def emu_linear(c, bias_first=True, k_drop=None):
    """fp32 accumulation over k, one product and one addition rounded per term (bf16 products are exact in fp32); the bias goes
    in first or last.  -> the fp32 accumulators before the epilogue, as float64."""
    x = c['x0'] if c['x1'] is None else np.concatenate([c['x0'], c['x1']], 1)
    x, W = x.astype(F32), c['W'].astype(F32)
    b = np.zeros(W.shape[0], F32) if c['bias'] is None else c['bias'].astype(F32)
    acc = np.tile(b, (x.shape[0], 1)) if bias_first else np.zeros((x.shape[0], W.shape[0]), F32)
    ks = range(x.shape[1]) if bias_first else range(x.shape[1] - 1, -1, -1)
    for k in ks:
        if k_drop is not None and k_drop <= k < k_drop + 16:
            continue
        acc = acc + x[:, k:k + 1] * W[None, :, k]
    if not bias_first:
        acc = acc + b
    return acc.astype(np.float64)


def emu_store(c, f, acc, bf16, rounder=tr.bf16_rne, neg_zero_live=False):
    v = np.maximum(acc, 0.0) if f.get('relu') else acc
    if c['mask'] is not None:
        keep = (c['mask'] > 0) | (neg_zero_live & (c['mask'] == 0) & np.signbit(c['mask']))
        v = np.where(keep, v, 0.0)
    return rounder(v) if (bf16 and not f.get('out_f32')) else v


def _check_case(form, c, got, bf16, dyadic):
    f = cases.FORMS[form]
    r, A, K = tr.linear_ref(c['x0'], c['W'], c['bias'], c['x1'])
    return tr.check_linear(form, got, r, A, K, bool(f.get('relu')), c['mask'], bf16 and not f.get('out_f32'), dyadic)


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('form', list(cases.FORMS))
def test_emulated_linear_stays_inside(form, bf16):
    f = cases.FORMS[form]
    for M in cases.LINEAR_M:
        c = cases.linear_case(form, M, bf16, False)
        for x in (c['x0'], c['x1'], c['W'], c['mask']):
            assert x is None or (tr.is_bf16(x) if bf16 else np.array_equal(x, x.astype(F32)))
        assert c['bias'] is None or np.array_equal(c['bias'], c['bias'].astype(F32))
        if M in (1, 33, 129):
            for bias_first in (True, False):
                _check_case(form, c, emu_store(c, f, emu_linear(c, bias_first), bf16), bf16, False)
        elif bf16 and not f.get('out_f32'):                              # the cap, on the reference alone
            r, A, K = tr.linear_ref(c['x0'], c['W'], c['bias'], c['x1'])
            lo, hi = tr.interval(r, A, K, tr.relu if f.get('relu') else tr.ident, c['mask'])
            assert np.mean(lo != hi) <= 0.25, (form, M)
        d = cases.linear_case(form, M, bf16, True)
        r, A, K = tr.linear_ref(d['x0'], d['W'], d['bias'], d['x1'])
        tr.assert_dyadic(form, r, A)
        assert A.max() > 10, 'a dyadic case of all zeros checks nothing'
        _check_case(form, d, emu_store(d, f, emu_linear(d), bf16), bf16, True)


def emu_wgrad(c, M, drop_last_row=False, db_skip_slice=None, transpose_tile=False):
    """Slices of whole 32-row tiles, fp32 accumulation row by row in each, float64 sum of the slices, one rounding to fp32."""
    G, per = tr.wgrad_slices(M)
    dz, x = c['dz'].astype(F32), c['x'].astype(F32)
    W, b = np.zeros((dz.shape[1], x.shape[1])), np.zeros(dz.shape[1])
    for g in range(G):
        pw, pb = np.zeros((dz.shape[1], x.shape[1]), F32), np.zeros(dz.shape[1], F32)
        for m in range(g * per, min((g + 1) * per, M - int(drop_last_row))):
            pw = pw + dz[m][:, None] * x[m][None, :]
            pb = pb + dz[m]
        W += pw
        if g != db_skip_slice:
            b += pb
    if transpose_tile:
        W[:32, :32] = W[:32, :32].T.copy()
    W, b = W.astype(F32).astype(np.float64), b.astype(F32).astype(np.float64)
    dW, db = np.full(c['dW_shape'], cases.FILL), np.full(c['db_shape'], cases.FILL)
    w, hit = tr.scatter(W, c['row_map'], c['col_map'], c['dW_shape'])
    dW[hit] = w[hit]
    v, hb = tr.scatter(b, c['row_map'], None, c['db_shape'])
    db[hb] = v[hb]
    return dW, db


def _check_wgrad(c, M, dW, db, dyadic):
    before_W, before_b = np.full(c['dW_shape'], cases.FILL), np.full(c['db_shape'], cases.FILL)
    return tr.check_wgrad('wgrad', dW, db, c['dz'], c['x'], c['row_map'], c['col_map'], M, before_W, before_b, dyadic=dyadic)


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n_pad,k_pad', cases.WGRAD_SHAPES)
def test_emulated_wgrad_stays_inside(n_pad, k_pad, bf16):
    for M in cases.WGRAD_M_RANDOM:
        c = cases.wgrad_case(n_pad, k_pad, M, bf16, False)
        dW, db = emu_wgrad(c, M)
        _check_wgrad(c, M, dW, db, False)
        assert not dW[c['zero_row'], :k_pad - 5].any() and db[c['zero_row']] == 0      # the zero column of dz: exact zeros
    for M, G in cases.WGRAD_M_DYADIC.items():
        assert tr.wgrad_slices(M)[0] == G
        c = cases.wgrad_case(n_pad, k_pad, M, bf16, True)
        full, AW, sb, Ab = tr.wgrad_ref(c['dz'], c['x'])
        tr.assert_dyadic('dW', full, AW)
        tr.assert_dyadic('db', sb, Ab)


def test_wgrad_slices_are_the_ones_the_cases_name():
    """8193 rows: 257 tiles on 256 slices of two tiles each -> slices 0..127 full, slice 128 one row, 129..255 empty."""
    assert tr.wgrad_slices(8193) == (256, 64) and 128 * 64 + 1 == 8193
    assert tr.wgrad_slices(16389) == (256, 96) and 16389 - 170 * 96 == 69 and tr.wgrad_terms(16389) == 104
    assert tr.wgrad_slices(135) == (5, 32) and tr.wgrad_slices(1025) == (33, 32) and tr.wgrad_terms(1) == 9


def test_dyadic_network_stores_every_activation_exactly():
    Ws, bs = cases.dyadic_network()
    for M in (161, 4099):
        agg, var, enc, gout = cases.step_inputs(M, True)
        fw = tr.chain_forward(Ws, bs, agg, var, enc, bf16=True)
        cases.assert_dyadic_forward(fw)
        exact = tr.chain_forward(Ws, bs, agg, var, enc)
        assert all(np.array_equal(a, b) for a, b in zip(fw['acts'] + [fw['GEO']] + fw['B'], exact['acts'] + [exact['GEO']] + exact['B']))
        assert np.array_equal(fw['raw4'], exact['raw4'])
        log = []                                                        # ... and every launch of its backward is dyadic
        dx0, dW, db = tr.chain_backward(fw, gout, bf16=True, log=log)
        assert len(log) == 10 + 2 * 11 and len(tr.BACKWARD_LAUNCHES) == 21
        for i, (r, A) in enumerate(log):
            tr.assert_dyadic(f'backward launch {i}', r, A)
        assert all(w.any() for w in dW) and all(b.any() for b in db) and dx0[:, :68].any(0).all()
        print(M, 'largest A of the backward: %.3g' % max(A.max() for _, A in log), 'largest |activation|:',
              max(np.abs(t).max() for t in fw['acts'] + [fw['GEO']] + fw['B']))


# ---- planted defects ------------------------------------------------------------------------------------------------------
OUTSIDE, BEYOND, DIFFER = r'outside \[lo, hi\]', 'beyond the bound', 'entries differ'


def test_defect_dropped_last_row():
    for M, dyadic, how in ((33, False, BEYOND), (129, False, BEYOND), (8193, True, DIFFER)):
        c = cases.wgrad_case(256, 96, M, True, dyadic)
        if M < 8193:
            dW, db = emu_wgrad(c, M, drop_last_row=True)
        else:                                                            # (exact operands: any order gives the same sums)
            c2 = dict(c, dz=c['dz'][:-1], x=c['x'][:-1])
            full, _, sb, _ = tr.wgrad_ref(c2['dz'], c2['x'])
            dW, db = np.full(c['dW_shape'], cases.FILL), np.full(c['db_shape'], cases.FILL)
            w, hit = tr.scatter(full, c['row_map'], c['col_map'], c['dW_shape'])
            dW[hit] = w[hit]
            db = None
        with pytest.raises(AssertionError, match='wgrad dW.*' + how):
            _check_wgrad(c, M, dW, db, dyadic)


def test_defect_dropped_k_step():
    for form in ('hidden', 'rgb_linears.0'):
        c = cases.linear_case(form, 33, True, False)
        got = emu_store(c, cases.FORMS[form], emu_linear(c, k_drop=176), True)
        with pytest.raises(AssertionError, match=OUTSIDE):
            _check_case(form, c, got, True, False)
    c = cases.linear_case('dX0', 33, False, False)
    with pytest.raises(AssertionError, match=BEYOND):
        _check_case('dX0', c, emu_linear(c, k_drop=496), False, False)
    d = cases.linear_case('hidden', 33, True, True)
    with pytest.raises(AssertionError, match=DIFFER):
        _check_case('hidden', d, emu_store(d, cases.FORMS['hidden'], emu_linear(d, k_drop=0), True), True, True)


def test_defect_swapped_columns():
    c = cases.linear_case('geo head', 129, True, False)
    got = emu_store(c, cases.FORMS['geo head'], emu_linear(c), True)
    got[:, [40, 41]] = got[:, [41, 40]]
    with pytest.raises(AssertionError, match=OUTSIDE):
        _check_case('geo head', c, got, True, False)


def test_defect_transposed_tile():
    c = cases.linear_case('hidden', 129, True, False)
    got = emu_store(c, cases.FORMS['hidden'], emu_linear(c), True)
    got[96:128, 32:64] = got[96:128, 32:64].T.copy()
    with pytest.raises(AssertionError, match=OUTSIDE):
        _check_case('hidden', c, got, True, False)
    w = cases.wgrad_case(64, 128, 33, False, False)
    dW, db = emu_wgrad(w, 33, transpose_tile=True)
    with pytest.raises(AssertionError, match='wgrad dW.*' + BEYOND):
        _check_wgrad(w, 33, dW, db, False)


def test_defect_truncation_instead_of_rne():
    for form in ('pts_linears.0', 'dgeo'):
        c = cases.linear_case(form, 33, True, False)
        got = emu_store(c, cases.FORMS[form], emu_linear(c), True, rounder=tr.bf16_trunc)
        with pytest.raises(AssertionError, match=OUTSIDE):
            _check_case(form, c, got, True, False)


def test_defect_negative_zero_taken_as_live():
    for bf16, form in ((True, 'dgrad hidden'), (False, 'dgrad hidden'), (True, 'masked fp32 store')):
        c = cases.linear_case(form, 1, bf16, False)
        f = cases.FORMS[form]
        good = emu_store(c, f, emu_linear(c), bf16)
        _check_case(form, c, good, bf16, False)
        got = emu_store(c, f, emu_linear(c), bf16, neg_zero_live=True)
        assert got[0, 1] != 0 and np.array_equal(np.flatnonzero(got != good), [1, f['n'] - 1])
        with pytest.raises(AssertionError, match=OUTSIDE if (bf16 and not f.get('out_f32')) else BEYOND):
            _check_case(form, c, got, bf16, False)


def test_defect_db_misses_a_slice():
    c = cases.wgrad_case(96, 256, 33, True, False)                     # the second slice holds one row
    dW, db = emu_wgrad(c, 33, db_skip_slice=1)
    with pytest.raises(AssertionError, match='wgrad db.*' + BEYOND):
        _check_wgrad(c, 33, dW, db, False)
    d = cases.wgrad_case(96, 256, 135, True, True)
    dW, db = emu_wgrad(d, 135, db_skip_slice=4)
    with pytest.raises(AssertionError, match='wgrad db.*' + DIFFER):
        _check_wgrad(d, 135, dW, db, True)


@pytest.mark.parametrize('form,M', [('pts_linears.0', 129), ('rgb_linears.0', 129), ('hidden', 129)])
def test_defect_one_bf16_ulp_high(form, M):
    """K = 96, 192, 256, before the ReLU (no entry is pinned by being clamped): one bf16 ulp above what the emulated kernel stores,
    planted on every positive entry in turn, is outside the interval wherever the interval admits one value -- at least the
    75 % that the cap of check_interval leaves (seen: 97.4 %, 93.9 %, 91.7 % of the positive entries); one such entry fails the check."""
    c = cases.linear_case(form, M, True, False)
    r, A, K = tr.linear_ref(c['x0'], c['W'], c['bias'], c['x1'])
    got = tr.bf16_rne(emu_linear(c))
    lo, hi = tr.interval(r, A, K)
    assert np.all((lo <= got) & (got <= hi))
    pos = got > 0
    caught = tr.bf16_ulp_up(got)[pos] > hi[pos]
    print(f'K={K}: one value admitted on {np.mean(lo == hi):.3f}, an ulp high caught on {np.mean(caught):.3f} of the positive entries')
    assert np.all(caught[(lo == hi)[pos]]) and np.mean(caught) >= 0.75
    i = tuple(np.argwhere(pos & (lo == hi))[0])
    bumped = got.copy()
    bumped[i] = tr.bf16_ulp_up(got[i])
    with pytest.raises(AssertionError, match=OUTSIDE):
        tr.check_interval(form, bumped, r, A, K)
