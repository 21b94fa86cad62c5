"""The cases of the per-entry LPIPS tests (tests/test_o_lpips_per_entry.py on the GPU, tests/test_lpips_restatement.py on the
CPU): the smallest shapes that reach each path of occnerf_amd/csrc/lpips.hip, as read from its source.

    min     1 x 16 x 16   relu5_3 at 1 x 1: M = 2 in a 64-row tile, every tap but the centre out of bounds; both input layouts
    odd     2 x 17 x 19   odd h and w at the first pool (17 -> 8, 19 -> 9 -> 4); M = 1292, no multiple of 64; NHWC input
    ragged  3 x 24 x 40   the shape of the fixture tests/golden/lpips_vgg_ragged.npz, NCHW
    wide    1 x 128 x 144 M = 36 864: 576 tiles at Co = 64, so conv1_1 and conv1_2 run with splits == 1, and so does conv1_1's
                          data gradient over one image (288 tiles) and over two.  Checked: conv1_1, conv1_2, pool1 (and conv2_1 behind it), head 0, the
                          backward with the tap-0 one-hot.  128 x 144 was enough: no enlargement was needed.
    flat    1 x 16 x 16   both images a constant colour (two different ones): positive ties in the pool windows
    dead    1 x 16 x 16   conv5_3 with zero weights and bias -1: relu5_3 all zero, n0 = sqrt(eps), k0 = 0 / (d0^2 n0)
    dyadic  1 x 16 x 16   shift 0, scale 1, images in multiples of 1/8, conv1_1 / conv1_2 sparse multiples of 1/4: x, act[0], act[1]
                          and pool[0] bit-equal to float64 (deeper layers are not claimed)

conv3x3_kernel<true> serves Cin = 3 only, that is conv1_1's forward (its data gradient has Cin = 64 on the GEMM's K side and
runs conv3x3_kernel<false>).  There K = 32 is ONE K step, and splits_for allows a split only from three K steps on: splits > 1
cannot be reached for <true> at any size, which test_split_coverage asserts from the re-derived splits_for instead of looking for
a case.  For <false> the case list holds both, forward and backward.

Models are built on the CPU from the seeded trunk and the seeded lins; inputs are uniform in [-1, 1] from a fixed seed."""
import numpy as np
import torch

CASES = {
    'min': dict(N=1, H=16, W=16, nhwc=False),
    'min_nhwc': dict(N=1, H=16, W=16, nhwc=True),
    'odd': dict(N=2, H=17, W=19, nhwc=True),
    'ragged': dict(N=3, H=24, W=40, nhwc=False),
    'wide': dict(N=1, H=128, W=144, nhwc=False, layers=(0, 1, 2), taps=(0,), gres=('tap0',)),
    'flat': dict(N=1, H=16, W=16, nhwc=False),
    'dead': dict(N=1, H=16, W=16, nhwc=False),
    'dyadic': dict(N=1, H=16, W=16, nhwc=False, dyadic_layers=(0, 1)),
}
NEEDS = ((1, 1), (1, 0), (0, 1))
GRES = ('ones', 'tap0', 'tap1', 'tap2', 'tap3', 'tap4', 'random')


def model(name):
    """The LPIPS module of a case, on the CPU, in eval mode."""
    from occnerf_amd.lpips import LPIPS
    m = LPIPS(pretrained=False, pnet_rand=True, verbose=False)
    convs = m.net.convs()
    with torch.no_grad():
        if name == 'dead':
            convs[12].weight.zero_()
            convs[12].bias.fill_(-1.0)
        if name == 'dyadic':
            m.scaling_layer.shift.zero_()
            m.scaling_layer.scale.fill_(1.0)
            rng = np.random.RandomState(11)
            for c in convs[:2]:
                w = rng.randint(-2, 3, size=tuple(c.weight.shape)) * (rng.uniform(size=tuple(c.weight.shape)) < 0.25) / 4.0
                c.weight.copy_(torch.from_numpy(w.astype(np.float32)))
                c.bias.copy_(torch.from_numpy((rng.randint(-2, 3, size=c.bias.shape[0]) / 4.0).astype(np.float32)))
    return m.eval()


def inputs(name):
    """in0, in1: logical [N,3,H,W] float32 on the CPU; an NHWC case holds them as permuted dense [N,H,W,3] tensors."""
    c = CASES[name]
    N, H, W = c['N'], c['H'], c['W']
    rng = np.random.RandomState(sum(map(ord, name.split('_')[0])))
    if name == 'flat':
        a = np.broadcast_to(np.float32([0.5, -0.25, 0.125]), (N, H, W, 3)).copy()
        b = np.broadcast_to(np.float32([-0.375, 0.75, 0.25]), (N, H, W, 3)).copy()
    elif name == 'dyadic':
        a, b = (rng.randint(-8, 9, size=(N, H, W, 3)).astype(np.float32) / 8 for _ in range(2))
    else:
        a, b = (rng.uniform(-1, 1, size=(N, H, W, 3)).astype(np.float32) for _ in range(2))
    out = []
    for t in (a, b):
        t = torch.from_numpy(t)
        out.append(t.permute(0, 3, 1, 2) if c['nhwc'] else t.permute(0, 3, 1, 2).contiguous())
    return tuple(out)


def to_device(t, dev, nhwc):
    """Move a logical NCHW tensor, keeping its memory layout (NHWC-dense stays a permuted view)."""
    return t.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2) if nhwc else t.contiguous().to(dev)


def gres(kind, N):
    """gres[5, N] = d loss / d res: all ones, one tap's row of ones, or a random signed vector."""
    if kind == 'ones':
        return torch.ones(5, N)
    if kind == 'random':
        return torch.from_numpy(np.random.RandomState(5).uniform(-1, 1, size=(5, N)).astype(np.float32))
    g = torch.zeros(5, N)
    g[int(kind[3:])] = 1.0
    return g


def gres_kinds(name):
    return CASES[name].get('gres', GRES)
