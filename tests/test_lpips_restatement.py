"""CPU: the helpers of the per-entry LPIPS tests (tests/lpips_restatement.py, tests/lpips_cases.py) checked on their own.

  * the two layouts re-derived in Python against the library's own counts;
  * the float64 restatements against torch's float64 autograd of test_lpips.restate and against both reference fixtures;
  * an emulation of the fp32 kernel set in torch (fp32 im2col matmul accumulated in K steps of 32, split over z and reduced in
    z order, the same workspace, the same ping-pong of the backward) passes every check the GPU tests apply;
  * ten planted defects, one at a time, each fail the check meant for them, on entries of the kind the defect touches.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lpips_cases as cases
from tests import lpips_restatement as lr
from tests.test_lpips import _fixture, _rel, restate

_memo = {}


def packed_of(name):
    """-> (module, regions of the expected pack, the flat blob), once per case."""
    if ('pk', name) not in _memo:
        m = cases.model(name)
        w, b, li, sh, sc = m._weights()
        reg = lr.pack_expected(w, b, li, sh, sc)
        _memo[('pk', name)] = (m, reg, lr.blob(reg))
    return _memo[('pk', name)]


# ---- layouts --------------------------------------------------------------------------------------------------------------------
def test_layouts_match_the_library():
    """pack_layout().total and work_layout's end of `part` equal the library's counts, over shapes on both sides of every
    threshold of splits_for; regions start on multiples of 64 floats."""
    from occnerf_amd import _lib
    lib = _lib.lib()
    assert lr.pack_layout()['total'] == lib.occnerf_lpips_packed_floats()
    assert lr.CIN == [3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512] and lr.TAP_LAYER == [1, 3, 6, 9, 12]
    shapes = [(c['N'], c['H'], c['W']) for c in cases.CASES.values()] + [(6, 32, 32), (2, 512, 512), (1, 16, 4000), (7, 33, 65),
                                                                        (1, 64, 64), (5, 100, 36), (64, 16, 16)]
    for N, H, W in shapes:
        wl = lr.work_layout(N, H, W)
        assert wl['part'] + wl['part_floats'] == wl['total'] == lib.occnerf_lpips_workspace_floats(N, H, W), (N, H, W)
        assert all(o % 64 == 0 for o in [wl['x'], wl['res'], wl['ga'], wl['gb'], wl['gh'], wl['part']] + wl['act'] + wl['pool'])


def test_split_coverage():
    """The case list reaches splits == 1 and splits > 1 of conv3x3_kernel<false>, forward and backward (nb = N and 2 N), and
    splits == 1 of conv1_1's data gradient; conv3x3_kernel<true> (conv1_1's forward, one K step) cannot split at any size."""
    fwd, bwd = set(), set()
    for c in cases.CASES.values():
        fs = lr.forward_splits(c['N'], c['H'], c['W'])
        assert fs[0] == 1
        layers = c.get('layers', range(lr.LAYERS))
        fwd |= {fs[l] > 1 for l in layers if l > 0}
        for nb in (c['N'], 2 * c['N']):
            bs = lr.backward_splits(nb, c['H'], c['W'])
            bwd |= {bs[l] > 1 for l in range(lr.LAYERS)}
    assert fwd == {False, True} and bwd == {False, True}
    w = cases.CASES['wide']
    assert lr.forward_splits(w['N'], w['H'], w['W'])[:2] == [1, 1]
    assert lr.backward_splits(w['N'], w['H'], w['W'])[:2] == [1, 1] and lr.backward_splits(2 * w['N'], w['H'], w['W'])[:2] == [1, 1]
    assert lr.backward_splits(1, 16, 16)[0] > 1
    assert all(lr.splits_for(M, 64, 32) == 1 for M in (1, 2, 64, 512, 1292, 36864, 10 ** 7))
    assert lr.leftover_buffers() == ('ga', 'gb')


# ---- restatement against autograd and the fixtures ----------------------------------------------------------------------------------
def _torch_state(pk_mod, in0, in1):
    """The float64 activations of torch's own forward (F.conv2d, F.max_pool2d), as a state for backward64_state."""
    convs = pk_mod.net.convs()
    x = torch.cat([in0, in1]).double()
    x = (x - pk_mod.scaling_layer.shift.double()) / pk_mod.scaling_layer.scale.double()
    v = {'N': in0.shape[0], 'H': in0.shape[2], 'W': in0.shape[3], 'act': []}
    for l in range(lr.LAYERS):
        if lr.POOL_BEFORE[l]:
            x = F.max_pool2d(x, 2, 2)
        x = F.relu(F.conv2d(x, convs[l].weight.double(), convs[l].bias.double(), padding=1))
        v['act'].append(x.permute(0, 2, 3, 1).contiguous())
    return v


@pytest.mark.parametrize('name', ['odd', 'flat', 'dead'])
def test_restatement_equals_float64_autograd(name):
    """forward64 reproduces restate's val and res, and backward64, fed the float64 activations of torch's forward, its input
    gradients for a random gres (<= 1e-10 relative).  flat: every interior pool window ties, so the route is torch's own
    'first maximum in row-major order'; dead: every gradient is finite and tap 4 contributes exact zeros."""
    m, reg, _ = packed_of(name)
    in0, in1 = (t.double().contiguous().requires_grad_(True) for t in cases.inputs(name))
    trunk = [(c.weight.double(), c.bias.double()) for c in m.net.convs()]
    lins = [li.weight.double() for li in m.lins]
    val, res = restate(trunk, lins, in0, in1)
    N = in0.shape[0]
    gres = cases.gres('random', N).double()
    (res * gres).sum().backward()
    fw = lr.forward64(reg, in0.detach(), in1.detach(), eps=1e-10)
    assert _rel(fw['val'], val.detach()) <= 1e-10 and _rel(fw['res'], res.detach()) <= 1e-10
    st = _torch_state(m, in0.detach(), in1.detach())
    if name == 'flat':
        q = lr.pool_windows(st['act'][1])
        ties = (q[0] == q[1]) & (q[0] == q[2]) & (q[0] == q[3]) & (q[0] > 0)
        assert int(ties.sum()) > 100, 'the flat case must tie with positive values at the first pool'
    scale = reg['scale'].double()
    for need0, need1 in cases.NEEDS:
        ref = lr.backward64_state(st, reg, gres, need0, need1, eps=1e-10)
        d = (ref['dx'] / scale).permute(0, 3, 1, 2)
        want = torch.cat([g for g, need in ((in0.grad, need0), (in1.grad, need1)) if need])
        assert torch.isfinite(d).all() and _rel(d, want) <= 1e-10, (need0, need1, _rel(d, want))
    if name == 'dead':
        assert bool((fw['res'][4] == 0).all())
        z = lr.backward64_state(st, reg, cases.gres('tap4', N).double(), 1, 1, eps=1e-10)
        assert not bool(z['dx'].any())


@pytest.mark.parametrize('case', ['train', 'ragged'])
def test_restatements_reproduce_the_fixtures(case):
    """forward64 and backward64 (on forward64's own state) against the reference's float64 val, res and both input gradients."""
    g = _fixture(case)
    m = cases.model('min')
    w, b, _, sh, sc = m._weights()
    reg = lr.pack_expected(w, b, [torch.from_numpy(g[f'lin{k}']) for k in range(5)], sh, sc)
    in0, in1 = torch.from_numpy(g['in0']).double(), torch.from_numpy(g['in1']).double()
    fw = lr.forward64(reg, in0, in1, eps=1e-10)
    assert _rel(fw['val'], g['val_f64']) <= 1e-10 and _rel(fw['res'], g['res_f64']) <= 1e-10
    ref = lr.backward64_state(fw, reg, torch.ones(5, in0.shape[0]), 1, 1, eps=1e-10)
    d = (ref['dx'] / reg['scale'].double()).permute(0, 3, 1, 2)
    N = in0.shape[0]
    assert _rel(d[:N], g['g0_f64']) <= 1e-10 and _rel(d[N:], g['g1_f64']) <= 1e-10


# ---- the kernel set emulated in fp32 ----------------------------------------------------------------------------------------------
def _conv_emul(x, Wp, Co, bias, relu, mask, d, layer):
    """conv3x3 + conv_reduce: fp32 im2col matmul in K steps of 32, split by splits_for, partials summed in z order, epilogue.
    d: the planted defect (kind, layer) or None."""
    B, H, W, C = x.shape
    kind = d[0] if d is not None and d[1] == layer else None
    if kind == 'clamp':                                     # a border tap clamped instead of zero-padded
        p = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode='replicate').permute(0, 2, 3, 1)
        cols = torch.cat([p[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], 3).reshape(B * H * W, 9 * C)
    else:
        cols = lr.im2col(x)
    Kp = Wp.shape[0]
    cols = F.pad(cols, (0, Kp - cols.shape[1]))
    ktiles, M = Kp // 32, B * H * W
    s = lr.splits_for(M, Co, Kp)
    v = None
    for z in range(s):
        kt0, kt1 = z * ktiles // s, (z + 1) * ktiles // s
        if kind == 'ktile' and z == s // 2:
            kt1 -= 1                                        # the last K tile of one split skipped
        acc = torch.zeros(M, Co)
        for kt in range(kt0, kt1):
            acc = acc + cols[:, kt * 32:(kt + 1) * 32] @ Wp[kt * 32:(kt + 1) * 32, :Co]
        v = acc if v is None else v + acc
    if bias is not None and not (kind == 'bias' and s > 1):
        v = v + bias
    v = v.view(B, H, W, Co)
    if relu:
        v = torch.where(v > 0, v, torch.zeros_like(v))
    if mask is not None:
        v = torch.where(mask > 0, v, torch.zeros_like(v))
    return v


def _head_fwd_emul(act, N, lin):
    C = act.shape[-1]
    a, b = act[:N].reshape(N, -1, C), act[N:].reshape(N, -1, C)
    eps = torch.tensor(1e-10, dtype=torch.float32)
    d0, d1 = torch.sqrt((a * a).sum(-1, keepdim=True) + eps) + eps, torch.sqrt((b * b).sum(-1, keepdim=True) + eps) + eps
    d = a / d0 - b / d1
    return (lin * (d * d)).sum(-1)


def emulate_forward(packed, in0, in1, defect=None):
    """-> val, res, work: occnerf_lpips_forward in fp32 torch, into a workspace of the library's layout."""
    N, _, H, W = in0.shape
    pk = lr.unpack(packed)
    work = torch.full((lr.work_layout(N, H, W)['total'],), float('nan'))
    v = lr.views(work, N, H, W)
    img = torch.cat([in0, in1]).float().permute(0, 2, 3, 1)
    v['x'].copy_((img - pk['shift']) / pk['scale'])
    x, k = v['x'], 0
    for l in range(lr.LAYERS):
        if lr.POOL_BEFORE[l]:
            v['pool'][k].copy_(lr.first_max(lr.pool_windows(x))[0])
            x, k = v['pool'][k], k + 1
        v['act'][l].copy_(_conv_emul(x, pk['Wf'][l], lr.COUT[l], pk['bias'][l], True, None, defect, l))
        x = v['act'][l]
    for t in range(lr.TAPS):
        v['respix'][t].copy_(_head_fwd_emul(v['act'][lr.TAP_LAYER[t]], N, pk['lin'][t]))
    res = torch.stack([r.sum(1) / r.shape[1] for r in v['respix']])
    v['res'].copy_(res)
    return res.sum(0), res, work


def _head_bwd_emul(act, N, lin, gres_t, need0, need1, out):
    B, h, w, C = act.shape
    a, b = act[:N].reshape(N, -1, C), act[N:].reshape(N, -1, C)
    eps = torch.tensor(1e-10, dtype=torch.float32)
    n0, n1 = torch.sqrt((a * a).sum(-1, keepdim=True) + eps), torch.sqrt((b * b).sum(-1, keepdim=True) + eps)
    d0, d1 = n0 + eps, n1 + eps
    coef = (gres_t / torch.tensor(float(h * w))).view(N, 1, 1)
    u = coef * lin * 2.0 * (a / d0 - b / d1)
    k0, k1 = (u * a).sum(-1, keepdim=True) / (d0 * d0 * n0), (u * b).sum(-1, keepdim=True) / (d1 * d1 * n1)
    z = torch.zeros_like(a)
    if need0:
        out[:N].copy_(torch.where(a > 0, u / d0 - k0 * a, z).view(N, h, w, C))
    if need1:
        out[N:].copy_(torch.where(b > 0, -u / d1 + k1 * b, z).view(N, h, w, C))


def _route_emul(act, gp, last=False, odd_row=False):
    """pool_back's routing in fp32: the first maximum (planted: the last; planted: the odd last row served as well)."""
    B, h, w, C = act.shape
    h2, w2 = h // 2, w // 2
    q = lr.pool_windows(act)
    m, arg = q[0], torch.zeros_like(q[0], dtype=torch.int64)
    for i in range(1, 4):
        gt = (q[i] >= m) if last else (q[i] > m)
        m, arg = torch.where(gt, q[i], m), torch.where(gt, torch.full_like(arg, i), arg)
    out = torch.zeros(B, h, w, C)
    for i in range(4):
        out[:, i // 2:2 * h2:2, i % 2:2 * w2:2] = torch.where(arg == i, gp, torch.zeros_like(gp))
    if odd_row and h % 2:
        out[:, h - 1, :2 * w2] = gp[:, h2 - 1].repeat_interleave(2, dim=1)
    return out


def emulate_backward(packed, work, shape, nhwc, gres, need0, need1, defect=None):
    """-> d0, d1 (logical [N,3,H,W], NHWC-dense when nhwc): occnerf_lpips_backward in fp32 torch on `work`, with its buffers."""
    N, _, H, W = shape
    pk, v = lr.unpack(packed), lr.views(work, N, H, W)
    hs, ws = lr.geometry(H, W)
    b0, nb = (0 if need0 else N), (int(need0) + int(need1)) * N
    dk = defect[0] if defect is not None else None
    m0 = 0 if dk == 'half' else b0                          # planted: need1-only reading image n instead of N + n

    def buf(name, l, C, first, count):
        n = hs[l] * ws[l] * C
        return v[name][first * n:(first + count) * n].view(count, hs[l], ws[l], C)
    ga, gb = 'ga', 'gb'
    _head_bwd_emul(v['act'][12], N, pk['lin'][4], gres[4], need0, need1, buf(ga, 12, 512, 0, 2 * N))
    tap = lr.TAPS - 2
    for l in range(lr.LAYERS - 1, -1, -1):
        mask = v['act'][l - 1][m0:m0 + nb] if l > 0 and not lr.POOL_BEFORE[l] else None
        if dk == 'nomask' and defect[1] == l:
            mask = None
        Wd = pk['Wd'][l]
        if dk == 'norot' and defect[1] == l:                # tap instead of 8 - tap
            Wd = Wd.view(9, lr.COUT[l], -1).flip(0).reshape(Wd.shape)
        out = _conv_emul(buf(ga, l, lr.COUT[l], b0, nb), Wd, lr.CIN[l], None, False, mask, None, l)
        if l == 0:
            v[gb][b0 * H * W * 3:(b0 + nb) * H * W * 3].view(nb, H, W, 3).copy_(out)
            break
        if lr.POOL_BEFORE[l]:
            lt, C = l - 1, lr.COUT[l - 1]
            _head_bwd_emul(v['act'][lt], N, pk['lin'][tap], gres[tap], need0, need1, buf('gh', lt, C, 0, 2 * N))
            act = v['act'][lt][m0:m0 + nb]
            g = buf('gh', lt, C, b0, nb) + _route_emul(act, out, last=dk == 'lastmax', odd_row=dk == 'oddrow')
            buf(ga, lt, C, b0, nb).copy_(torch.where(act > 0, g, torch.zeros_like(g)))
            tap -= 1
        else:
            buf(gb, l - 1, lr.CIN[l], b0, nb).copy_(out)
            ga, gb = gb, ga
    dx = v[gb][b0 * H * W * 3:(b0 + nb) * H * W * 3].view(nb, H, W, 3)
    d = dx / pk['scale']
    if nhwc and dk == 'order':                              # planted: the NHWC gradient written in NCHW order
        d = d.permute(0, 3, 1, 2).reshape(nb, H, W, 3)
    d = d.permute(0, 3, 1, 2) if nhwc else d.permute(0, 3, 1, 2).contiguous()
    return (d[:N] if need0 else None), (d[-N:] if need1 else None)


def _emulated(name, defect=None):
    key = ('emu', name, defect)
    if key not in _memo:
        _, _, packed = packed_of(name)
        in0, in1 = cases.inputs(name)
        val, res, work = emulate_forward(packed, in0, in1, defect)
        _memo[key] = (packed, in0, in1, val, res, work)
    return _memo[key]


def _backward_checks(name, defect=None, needs=cases.NEEDS, kinds=None, seen=None):
    packed, in0, in1, _, _, work = _emulated(name)
    c = cases.CASES[name]
    seen = {} if seen is None else seen
    for need0, need1 in needs:
        for kind in kinds or cases.gres_kinds(name):
            g = cases.gres(kind, c['N'])
            w = work.clone()
            d0, d1 = emulate_backward(packed, w, tuple(in0.shape), c['nhwc'], g, need0, need1, defect)
            lr.check_backward(w, packed, g, need0, need1, d0, d1, tuple(in0.shape), seen=seen, name=f'{name} {need0}{need1} {kind}')
    return seen


@pytest.mark.parametrize('name', ['min', 'min_nhwc', 'odd', 'flat', 'dead', 'dyadic'])
def test_emulated_kernels_pass_every_check(name):
    """The emulation (another summation order than the MFMA's, no fma) stays inside every forward and backward check."""
    packed, in0, in1, val, res, work = _emulated(name)
    c = cases.CASES[name]
    seen = lr.check_forward(work, packed, in0, in1, val, res, dyadic_layers=c.get('dyadic_layers', ()))
    _backward_checks(name, seen=seen)
    print(name, {k: round(r, 3) for k, r in seen.items()})
    assert all(r <= 1.0 for r in seen.values())
    if name == 'dead':
        assert not bool(res[4].any())
        w = work.clone()
        d0, d1 = emulate_backward(packed, w, tuple(in0.shape), c['nhwc'], cases.gres('tap4', 1), 1, 1)
        assert not bool(d0.any()) and not bool(d1.any())
    if name == 'flat':
        q = lr.pool_windows(lr.views(work, 1, 16, 16)['act'][1])
        assert int(((q[0] == q[1]) & (q[0] == q[2]) & (q[0] == q[3]) & (q[0] > 0)).sum()) > 100


# ---- planted defects -------------------------------------------------------------------------------------------------------------
def _forward_fails(name, defect, check):
    packed, in0, in1, val, res, work = _emulated(name, defect)
    with pytest.raises(lr.EntryError) as e:
        lr.check_forward(work, packed, in0, in1, val, res)
    assert e.value.check.startswith(check), (e.value.check, check)
    return e.value.bad


def _backward_fails(name, defect, check, **kw):
    with pytest.raises(AssertionError) as e:
        _backward_checks(name, defect, **kw)
    assert check in str(e.value), (str(e.value)[:200], check)
    return getattr(e.value, 'bad', None)


def test_defect_1_operand_not_rotated():
    for layer, check in ((0, 'dgrad conv1_1'), (5, 'd_in')):
        _backward_fails('odd', ('norot', layer), check, needs=((1, 1),), kinds=('ones',))


def test_defect_2_bias_dropped_in_the_reduce():
    assert lr.forward_splits(2, 17, 19)[6] > 1
    bad = _forward_fails('odd', ('bias', 6), 'conv 6 ')
    assert bad.any()


def test_defect_3_last_k_tile_of_a_split_skipped():
    assert lr.forward_splits(2, 17, 19)[3] > 1
    _forward_fails('odd', ('ktile', 3), 'conv 3 ')
    assert lr.forward_splits(1, 16, 16)[12] > 1
    _forward_fails('min', ('ktile', 12), 'conv 12 ')


def test_defect_4_border_tap_clamped():
    """Only border pixels fail, and interior ones never."""
    bad = _forward_fails('odd', ('clamp', 1), 'conv 1 ')
    assert bad[:, 1:-1, 1:-1].sum() == 0 and bad.sum() > 0


def test_defect_5_pool_gradient_to_the_last_maximum():
    """Shows on the case with ties only."""
    _backward_fails('flat', ('lastmax', None), 'd_in', needs=((1, 1),), kinds=('ones',))
    _backward_checks('odd', ('lastmax', None), needs=((1, 1),), kinds=('ones',))


def test_defect_6_pool_gradient_to_the_odd_last_row():
    _backward_fails('odd', ('oddrow', None), 'd_in', needs=((1, 1),), kinds=('tap1',))
    _backward_checks('min', ('oddrow', None), needs=((1, 1),), kinds=('tap1',))


def test_defect_7_relu_mask_omitted():
    _backward_fails('odd', ('nomask', 1), 'must be zero where relu1_1 is', needs=((1, 1),), kinds=('ones',))
    _backward_fails('odd', ('nomask', 6), 'd_in', needs=((1, 1),), kinds=('ones',))


def test_defect_8_need1_only_reads_the_wrong_half():
    _backward_fails('odd', ('half', None), 'must be zero where relu1_1 is', needs=((0, 1),), kinds=('ones',))
    _backward_checks('odd', ('half', None), needs=((1, 1), (1, 0)), kinds=('ones',))


def test_defect_9_nhwc_gradient_in_nchw_order():
    _backward_fails('odd', ('order', None), 'scale_out', needs=((1, 1),), kinds=('ones',))
    _backward_checks('min', ('order', None), needs=((1, 1),), kinds=('ones',))


def test_defect_10_one_ulp_high():
    """A stored activation one fp32 ulp high is caught at EVERY entry whose interval holds a single fp32 value (the entries a
    ReLU holds at zero beyond the bound; a live entry's interval spans about 2 K ulps).  The share is printed."""
    packed, in0, in1, _, _, work = _emulated('odd')
    v, pk = lr.views(work, 2, 17, 19), lr.unpack(packed)
    shares = []
    for l in (0, 1, 6, 12):
        r, A = lr.conv64(lr.conv_input(v, l), pk['Wf'][l][:9 * lr.CIN[l], :lr.COUT[l]], pk['bias'][l])
        lo, hi = lr.relu_interval(lr.np64(r), lr.np64(A), 9 * lr.CIN[l] + 2)
        single = lr.single_valued(lo, hi)
        got = v['act'][l].numpy()
        assert not lr.interval_outside(got.astype(np.float64), lo, hi).any()
        up = np.nextafter(got, np.float32(np.inf)).astype(np.float64)
        assert lr.interval_outside(up, lo, hi)[single].all() and single.any()
        shares.append(float(single.mean()))
        one = got.copy()
        i = tuple(np.argwhere(single)[0])
        one[i] = np.nextafter(one[i], np.float32(np.inf))
        with pytest.raises(lr.EntryError):
            lr.check_relu_interval(f'conv {l}', one.astype(np.float64), lr.np64(r), lr.np64(A), 9 * lr.CIN[l] + 2)
    print('share of single-valued intervals at conv 0, 1, 6, 12:', [round(s, 3) for s in shares])
