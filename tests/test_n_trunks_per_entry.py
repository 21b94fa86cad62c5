"""GPU: every launch of the two MLP trunks (occnerf_amd/csrc/linear.hip: linear_kernel, wgrad_kernel + wgrad_reduce_kernel;
csrc/trunks.hip: the fused bf16 forward) PER ENTRY against float64 of the operands that launch read
(tests/trunks_restatement.py, with the three kinds of check derived there):

    stored bf16, random operands    lo <= got <= hi, the RNE roundings of epi(r -+ gamma_{K+2} A): no tolerance;
    fp32 result, random operands    |got - r| <= gamma_n A + u |r|, n = K + 2 (forward) or rows of the largest slice + 8 (wgrad);
    dyadic operands                 bit-equal to the float64 value (a bf16 store: to its RNE rounding), at any shape.

No norm over a tensor, no tolerance relative to the largest entry: a lost row behind the last wave, a lost k-step, a wrong
bias-gradient entry, a -0.0 taken as live, an empty slice read as garbage or a wrong row map each fail by entry.  u = 2^-24
held everywhere (no widening to 2^-23 was needed).  Each test prints what it saw per launch; the worst values seen on an
MI355X stand in the docstrings."""
import numpy as np
import pytest
import torch

from tests import trunks_cases as cases
from tests import trunks_restatement as tr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def D(a, bf16=False):
    """float64 array of values exact in the flavour's format -> device tensor of that format."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    out = t.to(torch.bfloat16 if bf16 else torch.float32)
    assert torch.equal(out.double(), t), 'the case must be exact in its storage format'
    return out.contiguous()


def N(t):
    if t is None:
        return None
    with np.errstate(invalid='ignore'):         # (a torch.empty buffer recorded before its launch may hold signalling NaNs)
        return t.detach().float().cpu().numpy().astype(np.float64)


# ---- linear_forward -------------------------------------------------------------------------------------------------------
def _launch_linear(form, M, bf16, dyadic):
    """One launch of FORMS[form] into over-allocated buffers holding FILL.  -> what the checks saw."""
    from occnerf_amd import train_ops as to
    f = cases.FORMS[form]
    c = cases.linear_case(form, M, bf16, dyadic)
    n, n_store = f['n'], f.get('n_store', f['n'])
    out_f32 = bool(f.get('out_f32'))
    bf16_out = bf16 and not out_f32
    out = torch.full((M + 3, f.get('out_width', n)), cases.FILL, device=DEV, dtype=torch.bfloat16 if bf16_out else torch.float32)
    aux = torch.full((M + 3, 4), cases.FILL, device=DEV) if 'aux_col' in f else None
    Wfull = D(c['Wfull'], bf16)
    got = to.linear_forward(D(c['x0'], bf16), f['k0'], Wfull[:n], n, bf16, x1=D(c['x1'], bf16), k1=f.get('k1', 0),
                            bias=D(c['bias']), relu=bool(f.get('relu')), mask=D(c['mask'], bf16), out=out[:M], out_f32=out_f32,
                            n_store=n_store, aux=None if aux is None else aux[:M, 3:], aux_col=f.get('aux_col', 0),
                            aux_stride=f.get('aux_stride', 0))
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    o = N(out)
    name = f'{form} M={M} {"bf16" if bf16 else "fp32"} {"dyadic" if dyadic else "random"}'
    assert np.all(o[M:] == cases.FILL), name + ': rows >= M must keep their fill'
    assert np.all(o[:, n_store:] == cases.FILL), name + ': columns >= n_store must keep their fill'
    r, A, K = tr.linear_ref(c['x0'], c['W'], c['bias'], c['x1'])
    assert K == f['k0'] + f.get('k1', 0)
    seen = tr.check_linear(name, o[:M, :n_store], r[:, :n_store], A[:, :n_store], K, bool(f.get('relu')),
                           None if c['mask'] is None else c['mask'][:, :n_store], bf16_out, dyadic)
    if c['mask'] is not None:
        assert not o[:M][c['mask'] <= 0].any(), name + ': zero wherever mask <= 0'
    if aux is not None:
        a, j = N(aux), f['aux_col']
        assert np.all(a[M:] == cases.FILL) and np.all(a[:, :3] == cases.FILL), name + ': aux writes one column of M rows'
        seen += ' aux ' + tr.check_linear(name + ' aux', a[:M, 3:], r[:, j:j + 1], A[:, j:j + 1], K, bool(f.get('relu')), None, False, dyadic)
    return seen


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('form', list(cases.FORMS))
def test_linear_forward_per_entry(form, bf16):
    """The ten launch forms at M = 1, 31, 32, 33, 127, 128, 129, 257 (the 32-row wave and the 128-row workgroup from both sides),
    random operands and dyadic twins; mask rows with -0.0, +0.0, +-2^-126 and dead columns; three fill rows behind the M-th.
    The term count of the bound is K + 2: K additions, the product rounding (fp32 flavour), the bias.
    MI355X: every bf16 store inside [lo, hi] (at most 21.9 % of the entries of a case admit two values: the geometry
    head, no ReLU, at M = 1), every dyadic case bit-equal; fp32 results at most 0.122 of the bound in the fp32 flavour (K = 32),
    0.013 in the bf16 flavour (out_f32; aux 0.002)."""
    seen = {}
    for dyadic in (False, True):
        for M in cases.LINEAR_M:
            seen[(M, 'dyadic' if dyadic else 'random')] = _launch_linear(form, M, bf16, dyadic)
    print(form, 'bf16' if bf16 else 'fp32', seen)


# ---- linear_wgrad + reduce ------------------------------------------------------------------------------------------------
def _launch_wgrad(c, n_pad, k_pad, M, bf16, dyadic, name, with_db=True, twice=False):
    from occnerf_amd import train_ops as to
    dz, x = D(c['dz'], bf16), D(c['x'], bf16)
    rm, cm = (torch.from_numpy(c[k]).to(DEV) for k in ('row_map', 'col_map'))
    dW = torch.full(c['dW_shape'], cases.FILL, device=DEV)
    db = torch.full(c['db_shape'], cases.FILL, device=DEV) if with_db else None
    before = (N(dW), N(db))
    to.linear_wgrad(dz, n_pad, x, k_pad, bf16, rm, cm, dW, db)
    torch.cuda.synchronize()
    seen = tr.check_wgrad(name, N(dW), N(db), c['dz'], c['x'], c['row_map'], c['col_map'], M, before[0], before[1], dyadic=dyadic)
    zr = c['zero_row']                          # the all-zero column of dz: exact zeros out, whatever the operands
    assert not N(dW)[zr, :k_pad - 5].any() and (db is None or float(db[zr]) == 0.0), name + ': the zero column of dz'
    if twice:                                   # accumulate on what the first launch left (non-zero): exactly old + new
        before = (N(dW), N(db))
        to.linear_wgrad(dz, n_pad, x, k_pad, bf16, rm, cm, dW, db, accumulate=True)
        torch.cuda.synchronize()
        seen += tr.check_wgrad(name + ' accumulate', N(dW), N(db), c['dz'], c['x'], c['row_map'], c['col_map'], M, before[0],
                               before[1], accumulate=True, dyadic=dyadic)
    return seen


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('n_pad,k_pad', cases.WGRAD_SHAPES)
def test_linear_wgrad_per_entry(n_pad, k_pad, bf16):
    """dW / db through maps with holes into buffers with a row and two columns no map reaches (they keep their fill); a zero row
    and a zero column of dz (exact zeros out).  Random operands at M = 1, 33, 129 under gamma_{rows of the largest slice + 8} A
    + u |r| (count: see tests/trunks_restatement.py); dyadic operands, bit-equal, at M = 1, 33, 135, 1025, 8193, 16389 = 1, 2, 5,
    33, 256, 256 slices (a slice of one row, the reduce's tail loop, one unrolled trip + tail, empty slices 129..255, three
    tiles per slice with a ragged end), each followed by accumulate=True on the non-zero result (exactly old + new); db=None.
    MI355X: every dyadic case bit-equal; random dW at most 0.113 (fp32) / 0.037 (bf16) of the bound, db at most 0.031 / 0.004."""
    from occnerf_amd import _lib
    seen = {}
    for M in cases.WGRAD_M_RANDOM:
        c = cases.wgrad_case(n_pad, k_pad, M, bf16, False)
        seen[(M, 'random')] = _launch_wgrad(c, n_pad, k_pad, M, bf16, False, f'wgrad {n_pad}x{k_pad} M={M} random', twice=True)
    for M, G in cases.WGRAD_M_DYADIC.items():
        assert int(_lib.lib().occnerf_linear_wgrad_slices(M)) == G == tr.wgrad_slices(M)[0], (M, G)
        c = cases.wgrad_case(n_pad, k_pad, M, bf16, True)
        seen[(M, 'dyadic')] = _launch_wgrad(c, n_pad, k_pad, M, bf16, True, f'wgrad {n_pad}x{k_pad} M={M} dyadic', twice=True)
        if M in (33, 8193):
            seen[(M, 'dyadic, no db')] = _launch_wgrad(c, n_pad, k_pad, M, bf16, True, f'wgrad {n_pad}x{k_pad} M={M} db=None',
                                                       with_db=False)
    print(f'{n_pad}x{k_pad}', 'bf16' if bf16 else 'fp32', seen)


# ---- the step's trunks ----------------------------------------------------------------------------------------------------
_nets = {}


def _net(kind):
    """CanonicalMLP on the device with the case's ten layers.  -> (module, W[10], b[10] as float64)."""
    if kind not in _nets:
        from occnerf_amd.canonical_mlp import CanonicalMLP
        Ws, bs = cases.dyadic_network() if kind == 'dyadic' else cases.random_network()
        cm = CanonicalMLP(mlp_depth=4, mlp_width=256, skips=[]).to(DEV)
        with torch.no_grad():
            for n, W, b in zip(tr.LAYERS, Ws, bs):
                m = cm.get_submodule(n)
                m.weight.copy_(D(W))
                m.bias.copy_(D(b))
        _nets[kind] = (cm, Ws, bs)
    return _nets[kind]


def _run_step(kind, M, bf16, fused=True, spy_launches=False):
    """canonical_trunks forward + backward.  -> dict(raw4, saved = the context's tensors, grads, launches)."""
    from occnerf_amd import train_ops as to
    cm, Ws, bs = _net(kind)
    agg, var, enc, gout = cases.step_inputs(M, kind == 'dyadic')
    ta, te = D(agg).requires_grad_(True), D(enc).requires_grad_(True)
    res = {'inputs': (agg, var, enc, gout), 'launches': []}
    real_bw, real_lf, real_wg = to._Trunks.backward, to.linear_forward, to.linear_wgrad

    def spy_bw(ctx, d):
        res['saved'] = [t.clone() for t in ctx.acts] + [ctx.GEO.clone()] + [t.clone() for t in ctx.B]
        if spy_launches:                        # (both are looked up at call time; the scratch buffers are reused: clone)
            to.linear_forward, to.linear_wgrad = spy_lf, spy_wg
        try:
            return real_bw(ctx, d)
        finally:
            to.linear_forward, to.linear_wgrad = real_lf, real_wg

    def spy_lf(x0, k0, W, n_pad, bf16_, x1=None, k1=0, bias=None, relu=False, mask=None, out=None, out_f32=False, **kw):
        assert bias is None and not relu and out is None and not kw, 'the backward passes no bias, ReLU, out buffer or aux'
        rec = {'kind': 'dgrad', 'n_pad': n_pad, 'k0': k0, 'k1': k1, 'out_f32': out_f32, 'bf16': bf16_,
               'x0': N(x0), 'x1': N(x1), 'W': N(W), 'mask': N(mask)}
        y = real_lf(x0, k0, W, n_pad, bf16_, x1=x1, k1=k1, mask=mask, out_f32=out_f32)
        rec['y'], rec['y_dtype'] = N(y), y.dtype
        res['launches'].append(rec)
        return y

    def spy_wg(dz, n_pad, x, k_pad, bf16_, row_map, col_map, dW, db=None, accumulate=False):
        rec = {'kind': 'wgrad', 'n_pad': n_pad, 'k_pad': k_pad, 'bf16': bf16_, 'accumulate': accumulate, 'dz': N(dz), 'x': N(x),
               'row_map': row_map.cpu().numpy(), 'col_map': col_map.cpu().numpy(), 'before_W': N(dW), 'before_b': N(db),
               'shape': tuple(dW.shape)}
        real_wg(dz, n_pad, x, k_pad, bf16_, row_map, col_map, dW, db, accumulate)
        rec['dW'], rec['db'] = N(dW), N(db)
        res['launches'].append(rec)

    to._Trunks.backward = staticmethod(spy_bw)
    try:
        raw = to.canonical_trunks(cm, ta, D(var), te, bf16, fused=fused)
        (raw * D(gout)).sum().backward()
        torch.cuda.synchronize()
    finally:
        to._Trunks.backward = real_bw
    res['raw4'] = N(raw)
    res['grads'] = {'agg': N(ta.grad), 'enc': N(te.grad), **{n: N(p.grad) for n, p in cm.named_parameters() if p.grad is not None}}
    cm.zero_grad(set_to_none=True)
    return res


def _packs(Ws, bs):
    maps = tr.trunk_maps()
    return [tr.pack(Ws[l], bs[l], maps['rows'][l], maps['cols'][l], True) for l in range(10)]


def _x0_of(agg, var, enc):
    X0 = np.zeros((agg.shape[0], 96))
    X0[:, :35], X0[:, 35:36], X0[:, 36:68] = agg, var, enc
    return tr.bf16_rne(X0)


@pytest.mark.parametrize('M', cases.FUSED_M)
def test_fused_forward_per_entry(M):
    """trunks_forward_kernel through canonical_trunks(fused=True), random network: every saved tensor against float64 of the
    PREVIOUS saved tensor of the same run -- X0 the exact RNE rounding of the inputs, pads exactly zero, A1..A4, GEO[:, :64],
    B1..B4 inside [lo, hi]; GEO[:, 64] = bf16(raw4[:, 3]); raw4 (VALU dot products of the UNROUNDED fp32 accumulators with the
    fp32 weights) against the saved bf16 A4 / B4 under (2^-8 + gamma_258) sum |w||a| + u |r|: a stored bf16 value is within
    2^-9 / (1 - 2^-9) < 2^-8 relative of what was rounded.
    MI355X: all inside; at most 13.6 % of a tensor's entries admit two values (GEO); raw4 at most 0.245 of its bound (M = 4099)."""
    _, Ws, bs = _net('random')
    run = _run_step('random', M, True)
    agg, var, enc, _ = run['inputs']
    names = ['X0', 'A1', 'A2', 'A3', 'A4', 'GEO', 'B1', 'B2', 'B3', 'B4']
    assert all(t.dtype == torch.bfloat16 for t in run['saved'])
    S = dict(zip(names, (N(t) for t in run['saved'])))
    assert [S[n].shape for n in names] == [(M, 96)] + [(M, 256)] * 4 + [(M, 96)] + [(M, 256)] * 4
    P = _packs(Ws, bs)
    seen = {'X0': tr.check_exact('X0', S['X0'], _x0_of(agg, var, enc))}
    prev = 'X0'
    for l, nm in enumerate(names[1:5]):
        r, A, K = tr.linear_ref(S[prev], P[l][0], P[l][1])
        seen[nm] = '%.3f wide' % tr.check_interval(f'{nm} M={M}', S[nm], r, A, K, tr.relu)
        prev = nm
    r, A, K = tr.linear_ref(S['A4'], P[4][0][:64], P[4][1][:64])
    seen['GEO'] = '%.3f wide' % tr.check_interval(f'GEO M={M}', S['GEO'][:, :64], r, A, K)
    tr.check_exact('GEO[:, 64] = bf16(sigma)', S['GEO'][:, 64], tr.bf16_rne(run['raw4'][:, 3]))
    assert not S['GEO'][:, 65:].any() and not S['X0'][:, 68:].any(), 'pad columns are exactly zero'
    r, A, K = tr.linear_ref(S['GEO'], P[5][0], P[5][1], x1=S['X0'])
    seen['B1'] = '%.3f wide' % tr.check_interval(f'B1 M={M}', S['B1'], r, A, K, tr.relu)
    for l, nm in ((6, 'B2'), (7, 'B3'), (8, 'B4')):
        r, A, K = tr.linear_ref(S[names[names.index(nm) - 1]], P[l][0], P[l][1])
        seen[nm] = '%.3f wide' % tr.check_interval(f'{nm} M={M}', S[nm], r, A, K, tr.relu)
    for nm, act, W, b, got in (('sigma', S['A4'], Ws[4][:1], bs[4][:1], run['raw4'][:, 3:]),
                               ('rgb', S['B4'], Ws[9], bs[9], run['raw4'][:, :3])):
        r = act @ W.T + b
        bound = (2.0 ** -8 + tr.gamma(258)) * (np.abs(act) @ np.abs(W).T) + tr.U * np.abs(r)
        ratio = np.abs(got - r) / bound
        assert np.all(ratio <= 1), (nm, M, float(ratio.max()), tuple(np.argwhere(~(ratio <= 1))[0]))
        seen[nm] = '%.3f' % ratio.max()
    print(f'fused M={M}', seen)


@pytest.mark.parametrize('M', cases.FUSED_M)
def test_fused_forward_dyadic_is_bit_equal(M):
    """The dyadic network (sparse weights in {-1, 0, 1}, integer biases and inputs; every pre-activation an integer <= 256 in
    size, asserted on the reference): all ten saved tensors and raw4 bit-equal to float64, and to the staged forward
    (fused=False, ten launches of linear_kernel) of the same inputs.  MI355X: bit-equal at every M."""
    _, Ws, bs = _net('dyadic')
    run = _run_step('dyadic', M, True)
    agg, var, enc, _ = run['inputs']
    fw = tr.chain_forward(Ws, bs, agg, var, enc, bf16=True)
    if M >= 127:                                # (its "no layer is dead" share needs more than a few rows)
        cases.assert_dyadic_forward(fw)
    want = fw['acts'] + [fw['GEO']] + fw['B']
    for nm, got, w in zip(['X0', 'A1', 'A2', 'A3', 'A4', 'GEO', 'B1', 'B2', 'B3', 'B4'], run['saved'], want):
        tr.check_exact(f'{nm} M={M}', N(got), w)
    tr.check_exact(f'raw4 M={M}', run['raw4'], fw['raw4'])
    staged = _run_step('dyadic', M, True, fused=False)
    for a, b in zip(run['saved'], staged['saved']):
        assert torch.equal(a, b)
    tr.check_exact('raw4 staged', staged['raw4'], fw['raw4'])
    for k in run['grads']:
        tr.check_exact(f'{k} fused / staged', run['grads'][k], staged['grads'][k])


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('kind,M', [('random', 161), ('dyadic', 161), ('dyadic', 4099)])
def test_backward_launch_by_launch(kind, M, bf16):
    """_Trunks.backward through spies on train_ops.linear_forward / linear_wgrad: the 21 launches (10 input-gradient, 11
    weight-gradient) in their order, each against float64 of ITS OWN recorded operands, through row / column maps derived
    here from the layout of occnerf_mlp.py:183-199 (the recorded ones must equal them); what autograd hands back is exactly
    what the launches wrote: agg.grad = dx0[:, :35], enc.grad = dx0[:, 36:68], the 20 parameter gradients, rgb_linears.0.weight
    from its two launches in disjoint columns.
    MI355X: dyadic runs bit-equal in every launch; random: bf16 stores inside [lo, hi] (at most 9.2 % of a launch's entries
    admit two values), fp32 results at most 0.042 (bf16 flavour) / 0.069 (fp32 flavour) of the bound."""
    dyadic = kind == 'dyadic'
    run = _run_step(kind, M, bf16, spy_launches=True)
    L = run['launches']
    maps = tr.trunk_maps()
    got_order = [('wgrad', None, r['n_pad'], r['k_pad'], r['db'] is not None) if r['kind'] == 'wgrad' else
                 ('dgrad', r['n_pad'], r['k0'], r['k1'], r['mask'] is not None, bool(r['out_f32'])) for r in L]
    want_order = [(t[0], None) + t[2:] if t[0] == 'wgrad' else t for t in tr.BACKWARD_LAUNCHES]
    assert got_order == want_order
    seen, final, rgb0 = [], {}, []
    for i, (r, t) in enumerate(zip(L, tr.BACKWARD_LAUNCHES)):
        name = f'launch {i} {t} M={M}'
        assert r['bf16'] == bf16
        if r['kind'] == 'dgrad':
            ref, A, K = tr.linear_ref(r['x0'], r['W'], None, r['x1'])
            bf16_out = bf16 and not r['out_f32']
            assert r['y_dtype'] == (torch.bfloat16 if bf16_out else torch.float32) and K == r['k0'] + r['k1']
            seen.append(tr.check_linear(name, r['y'], ref, A, K, False, r['mask'], bf16_out, dyadic))
            continue
        l = t[1]
        cm = maps['cols'][l]
        if l == 5:
            cm = maps['rgb_seg0'] if not rgb0 else maps['rgb_seg1']
            rgb0.append(r)
        assert r['shape'] == tr.SHAPES[l] and not r['accumulate']
        assert np.array_equal(r['row_map'], maps['rows'][l]) and np.array_equal(r['col_map'], cm), name + ': the maps'
        seen.append(tr.check_wgrad(name, r['dW'], r['db'], r['dz'], r['x'], maps['rows'][l], cm, M, r['before_W'], r['before_b'],
                                   dyadic=dyadic, holes=False))
        final[l] = (r['dW'] if l != 5 or len(rgb0) == 1 else np.concatenate([final[5][0][:, :64], r['dW'][:, 64:]], 1),
                    r['db'] if r['db'] is not None else final[l][1])
    print(kind, M, 'bf16' if bf16 else 'fp32', seen)
    # autograd hands back what the launches wrote
    dx0 = L[-1]['y']
    assert dx0.shape == (M, 96)
    tr.check_exact('agg.grad', run['grads']['agg'], dx0[:, :35])
    tr.check_exact('enc.grad', run['grads']['enc'], dx0[:, 36:68])
    s0, s1 = maps['rgb_seg0'], maps['rgb_seg1']
    assert sorted(s0[s0 >= 0]) == list(range(64)) and sorted(s1[s1 >= 0]) == list(range(64, 131))
    assert len(rgb0) == 2 and len(final) == 10
    assert len([k for k in run['grads'] if 'linear' in k]) == 20
    for l, n in enumerate(tr.LAYERS):
        tr.check_exact(n + '.weight.grad', run['grads'][n + '.weight'], final[l][0])
        tr.check_exact(n + '.bias.grad', run['grads'][n + '.bias'], final[l][1])
        assert np.abs(final[l][0]).max() > 0
