"""Times LPIPS-VGG at the training batch (6 patches of 32 x 32, pred + target) on one GPU:

  * the HIP forward + backward (occnerf_amd/lpips.py; gradient for the prediction, as in training);
  * the same maths restated with torch F.conv2d (MIOpen) in this process, forward + backward, as the baseline;
  * a train.py-style step (network forward + loss + backward, 6 x 32 x 32 rays) with and without the lpips term.

Device events around each repeat, after warm-up; medians of the repeats.  It also prints the floors the shapes imply: FLOP at
the fp32 MFMA peak and the weight bytes (forward + data-gradient layouts) at HBM bandwidth.

    python tools/lpips_bench.py [--repeats 7] [--iters 20] [--no-train]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3          # MI355X fp32 MFMA
HBM_TBPS = 6.0 * 1.04        # ~6.3 TB/s achievable streaming rate


def floors(N, H, W):
    from occnerf_amd.lpips import VGG16_CHANNELS
    pools_before = {2, 4, 7, 10}
    flop, h, w = 0, H, W
    for i, (cin, cout) in enumerate(VGG16_CHANNELS):
        if i in pools_before:
            h, w = h // 2, w // 2
        flop += 2 * (2 * N) * h * w * 9 * cin * cout           # forward, pred + target
        flop += 2 * N * h * w * 9 * cin * cout                 # data gradient, pred only
    wbytes = 2 * 4 * sum(9 * cin * cout + cout for cin, cout in VGG16_CHANNELS)
    return flop, wbytes


def restate_fn(trunk, lins):
    shift = torch.tensor([-.030, -.088, -.188], device='cuda:0')[None, :, None, None]
    scale = torch.tensor([.458, .448, .450], device='cuda:0')[None, :, None, None]

    def taps(x):
        x = (x - shift) / scale
        out, li = [], 0
        for block in (2, 2, 3, 3, 3):
            if out:
                x = F.max_pool2d(x, 2, 2)
            for _ in range(block):
                x = F.relu(F.conv2d(x, trunk[li][0], trunk[li][1], padding=1))
                li += 1
            out.append(x)
        return out

    def unit(f):
        return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True) + 1e-10) + 1e-10)

    def fn(a, b):
        return sum(F.conv2d((unit(x) - unit(y)) ** 2, lw).mean([2, 3]) for x, y, lw in zip(taps(a), taps(b), lins))
    return fn


def timed(step, iters, repeats, warmup=5):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            step()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out)), [round(x, 4) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--no-train', action='store_true')
    a = ap.parse_args()
    from occnerf_amd.lpips import LPIPS, scale_for_lpips
    dev = 'cuda:0'
    N, H, W = 6, 32, 32
    m = LPIPS(pretrained=False, pnet_rand=True, verbose=False).to(dev).eval()
    gen = torch.Generator().manual_seed(0)
    x0 = (torch.rand(N, 3, H, W, generator=gen) * 2 - 1).to(dev).requires_grad_(True)
    x1 = (torch.rand(N, 3, H, W, generator=gen) * 2 - 1).to(dev)

    def hip_step():
        x0.grad = None
        m(x0, x1).mean().backward()

    convs = m.net.convs()
    trunk = [(c.weight.detach(), c.bias.detach()) for c in convs]
    lins = [lin.weight.detach() for lin in m.lins]
    ref = restate_fn(trunk, lins)

    def miopen_step():
        x0.grad = None
        ref(x0, x1).mean().backward()

    flop, wbytes = floors(N, H, W)
    t_flop_us, t_bytes_us = flop / (PEAK_TFLOPS * 1e12) * 1e6, wbytes / (HBM_TBPS * 1e12) * 1e6
    hip_ms, hip_all = timed(hip_step, a.iters, a.repeats)
    mio_ms, mio_all = timed(miopen_step, a.iters, a.repeats)
    bound = 'FLOP' if t_flop_us >= t_bytes_us else 'weight bytes'
    res = {'batch': f'{N}+{N} images of {H}x{W}', 'gflop': round(flop / 1e9, 3), 'weight_mb': round(wbytes / 1e6, 1),
           'floor_flop_us': round(t_flop_us, 1), 'floor_bytes_us': round(t_bytes_us, 1), 'bound_by': bound,
           'hip_fwd_bwd_ms': round(hip_ms, 4), 'hip_repeats_ms': hip_all,
           'hip_share_of_floor': round(max(t_flop_us, t_bytes_us) / 1e3 / hip_ms, 4),
           'hip_tflops': round(flop / hip_ms / 1e9, 2),
           'miopen_fwd_bwd_ms': round(mio_ms, 4), 'miopen_repeats_ms': mio_all,
           'speedup_vs_miopen': round(mio_ms / hip_ms, 2)}
    if not a.no_train:
        res.update(train_step(m, a))
    print(json.dumps(res))


def train_step(m, a):
    """A train.py step on 6 full 32 x 32 patches (network forward + loss + backward; no optimiser), with and without lpips."""
    from occnerf_amd import synth
    from occnerf_amd.lpips import PatchImages, patch_image_loss
    from occnerf_amd.seeded import build_network, frame_to_device, patch_ray_selection_map
    dev = 'cuda:0'
    frame = synth.make_frame(img_size=512, pose72=synth.seeded_pose(101), orbit_frame=5)
    sel, pix = patch_ray_selection_map(frame, np.random.RandomState(0), 6, 32, full=True)
    for k in ('near', 'far'):
        frame[k] = frame[k][sel]
    frame['rays'] = frame['rays'][:, sel]
    data = frame_to_device(frame, dev)
    patches = PatchImages(pix, 6, 32, dev)
    with torch.no_grad():
        target = build_network(seed=1, amplify=True, S=128)(**data, iter_val=1e7)['rgb']
    net = build_network(seed=0, S=128)
    net.cfg.perturb = 1.0
    net.train()
    bg = frame['bgcolor'] / 255.
    out = {}
    for name, weights in (('train_step_ms_mse_comp', None), ('train_step_ms_lpips_mse_comp', {'lpips': 1.0, 'mse': 0.2})):
        def step():
            net.zero_grad(set_to_none=True)
            o = net(**data, iter_val=1)
            if weights is None:
                loss = 0.2 * torch.mean((o['rgb'] - target) ** 2) + o['comp_loss'].mean()
            else:
                loss = patch_image_loss(o['rgb'], target, patches, bg, weights, m) + o['comp_loss'].mean()
            loss.backward()
        ms, _ = timed(step, max(1, a.iters // 4), a.repeats, warmup=3)
        out[name] = round(ms, 3)
    return out


if __name__ == '__main__':
    main()
