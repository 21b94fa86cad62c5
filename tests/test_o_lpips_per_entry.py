"""GPU: every launch of the LPIPS kernel set (occnerf_amd/csrc/lpips.hip) PER ENTRY against float64 of the operands that launch
read, as they lie in the two tensors the public ops return: the workspace of ops.lpips_forward and the blob of LPIPS.packed()
(tests/lpips_restatement.py: the layouts re-derived, the restatements, the bounds and their derivation; tests/lpips_cases.py: the
cases and which path each reaches; tests/test_lpips_restatement.py: the same checks on an emulated kernel and ten planted defects).

    pack_layer / pack_small   bit-equal to the permutation of the module's weights, padding rows and columns exactly zero
    scale_in, scale_out       the correctly rounded fp32 quotient, bit for bit, NCHW and NHWC
    conv3x3 (+ conv_reduce)   stored in [relu(r - e), relu(r + e)], e = gamma_{9 Cin + 2} A + u |r|; 13 layers, splits == 1 and > 1
    maxpool                   bit-equal
    head_fwd, head_finish     first-order bounds per pixel / per image
    backward                  d_in0 / d_in1 for (need0, need1) = (1,1), (1,0), (0,1) and seven gres, under the worst-case chain
                              bound AND the Hoeffding bound over the squared maps (the first has no power beyond tap 0);
                              the three buffers that survive the backward, each from its launch's real operands: gh (head_bwd
                              of tap 0), conv1_1's data gradient from conv1_2's saved output, scale_out.

The ping-pong of occnerf_lpips_backward was replayed from its loop (lpips_restatement.leftover_buffers): eight swaps, so `ga` holds
conv1_2's data gradient masked by relu1_1, `gb` the dx of conv1_1 and `gh` head_bwd of tap 0, as the checks below find them.
Where only N of the 2 N images were computed, the other half of each buffer is not read.

No norm over a tensor, nothing relative to the largest entry.  u = 2^-24 held everywhere; no term for flushed subnormal products
was needed.  The worst error / bound per kernel kind seen on an MI355X stands in test_z_records."""
import pytest
import torch

from tests import lpips_cases as cases
from tests import lpips_restatement as lr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_memo = {}


def _run(name):
    """One forward of a case: module, packed blob, inputs on the device in the case's layout, val, res, workspace."""
    if name not in _memo:
        from occnerf_amd import ops
        c = cases.CASES[name]
        m = cases.model(name).to(DEV)
        packed = m.packed()
        in0, in1 = (cases.to_device(t, DEV, c['nhwc']) for t in cases.inputs(name))
        val, res, work, nhwc = ops.lpips_forward(packed, in0, in1, want_res=True)
        torch.cuda.synchronize()
        assert nhwc == int(c['nhwc']), 'the case must reach the layout it is named for'
        _memo[name] = dict(m=m, packed=packed, in0=in0, in1=in1, val=val, res=res, work=work, nhwc=nhwc, fwd=None, bwd=None)
    return _memo[name]


def _forward_seen(name):
    s, c = _run(name), cases.CASES[name]
    if s['fwd'] is None:
        s['fwd'] = lr.check_forward(s['work'], s['packed'], s['in0'], s['in1'], s['val'], s['res'], layers=c.get('layers'),
                                    taps=c.get('taps'), dyadic_layers=c.get('dyadic_layers', ()))
    return s['fwd']


def _backward_seen(name):
    from occnerf_amd import ops
    s, c = _run(name), cases.CASES[name]
    if s['bwd'] is None:
        seen, shape = {}, tuple(s['in0'].shape)
        for need0, need1 in cases.NEEDS:
            for kind in cases.gres_kinds(name):
                g = cases.gres(kind, c['N']).to(DEV)
                d0, d1 = ops.lpips_backward(s['packed'], s['work'], shape, s['nhwc'], g, need0, need1)
                torch.cuda.synchronize()
                for d in (d0, d1):
                    assert d is None or bool(torch.isfinite(d).all())
                lr.check_backward(s['work'], s['packed'], g, need0, need1, d0, d1, shape, seen=seen,
                                  name=f'{name} need {need0}{need1} {kind}')
                if name == 'dead' and kind == 'tap4':
                    assert all(not bool(d.any()) for d in (d0, d1) if d is not None), 'tap 4 of the dead case contributes exact zeros'
        s['bwd'] = seen
    return s['bwd']


def test_packs_are_bit_equal_and_padded_with_zeros():
    """Wf, Wd, the biases, the lins and shift / scale of the blob equal the torch permutation of the module's weights bit for bit
    (the rotated, transposed data-gradient operand W[co, ci, 2-ky, 2-kx] included); every padding row (Kf up to a multiple of
    32) and column (Nf / Nd up to a multiple of 64) is exactly zero; an in-place change of one conv weight rebuilds the blob."""
    def compare(m):
        got = lr.unpack(m.packed())
        want = lr.pack_expected(*m._weights())
        for k in ('Wf', 'Wd', 'bias', 'lin'):
            for i, (a, b) in enumerate(zip(got[k], want[k])):
                assert torch.equal(a, b), (k, i)
        assert torch.equal(got['shift'], want['shift']) and torch.equal(got['scale'], want['scale'])
        for l in range(lr.LAYERS):
            assert not bool(got['Wf'][l][9 * lr.CIN[l]:].any()) and not bool(got['Wf'][l][:, lr.COUT[l]:].any()), l
            assert not bool(got['Wd'][l][:, lr.CIN[l]:].any()), l
        return m.packed()
    for name in ('min', 'dead', 'dyadic'):
        compare(_run(name)['m'])
    m = cases.model('min').to(DEV)
    before = compare(m).clone()
    with torch.no_grad():
        m.net.convs()[3].weight[5, 7, 0, 2] = 0.375
    after = compare(m)
    assert not torch.equal(before, after)
    assert lr.pack_layout()['kf'][0] == 32 and lr.pack_layout()['nd'][0] == 64       # conv1_1: 5 padding rows, 61 padding columns


@pytest.mark.parametrize('name', list(cases.CASES))
def test_forward_per_launch(name):
    """scale_in, 13 x conv3x3 (+ reduce), 4 x maxpool, 5 x head_fwd and head_finish of one forward, each against float64 of the
    input it read from the workspace (wide: the first block only).  dyadic: x, act[0], act[1] and pool[0] also bit-equal to
    float64; dead: res[4] == 0 exactly; flat: the first pool really ties with positive values."""
    seen = _forward_seen(name)
    print(name, {k: float('%.3g' % r) for k, r in seen.items()})
    assert all(r <= 1.0 for r in seen.values())
    s = _run(name)
    if name == 'dead':
        assert not bool(s['res'][4].any())
    if name == 'flat':
        q = lr.pool_windows(lr.views(s['work'], 1, 16, 16)['act'][1])
        assert int(((q[0] == q[1]) & (q[0] == q[2]) & (q[0] == q[3]) & (q[0] > 0)).sum()) > 100


@pytest.mark.parametrize('name', list(cases.CASES))
def test_backward_per_entry(name):
    """d_in0 / d_in1 per entry for the three (need0, need1), the case's layout and seven gres (all ones, five one-hot-per-tap, a
    random signed one; wide: the tap-0 one-hot) against backward64 on the saved state, with masks and first-maximum routes read
    from the saved fp32 activations; then gh, conv1_1's data gradient and scale_out from their launches' real operands."""
    seen = _backward_seen(name)
    print(name, {k: float('%.3g' % r) for k, r in seen.items()})
    assert all(r <= 1.0 for r in seen.values())


def test_z_records():
    """The largest error / bound per kernel kind over all cases, each <= 1, and every kind reached.
    MI355X: conv3x3<true> 0.142; conv3x3<false> 0.0106 (splits == 1), 0.0028 (splits > 1); conv1_1's data gradient 0.0096 /
    0.0029; head_fwd 0.025; head_finish res 0.32, val 0.40; head_bwd 0.078; the backward chain 3.1e-4 of the worst-case bound and
    1.1e-3 of the Hoeffding bound; maxpool, scale_in, scale_out and the dyadic block bit-equal."""
    total = {}
    for name in cases.CASES:
        for seen in (_forward_seen(name), _backward_seen(name)):
            for k, r in seen.items():
                lr.worst(total, k, r)
    for k in sorted(total):
        print('%-34s %.3g' % (k, total[k]))
    assert all(r <= 1.0 for r in total.values())
    want = {'scale_in', 'scale_out', 'maxpool', 'head_fwd', 'head_finish res', 'head_finish val', 'head_bwd',
            'conv3x3<true> splits == 1', 'conv3x3<false> splits == 1', 'conv3x3<false> splits > 1', 'dgrad conv1_1 splits == 1',
            'dgrad conv1_1 splits > 1', 'backward chain (worst case)', 'backward chain (Hoeffding)'}
    assert set(total) == want, set(total) ^ want
