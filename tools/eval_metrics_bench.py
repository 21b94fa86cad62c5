"""Times eval.py's per-frame metrics at 512 x 512 on one GPU and writes profiles/eval_metrics_bench.json:

  * the HIP kernel pair (occnerf_frame_metrics: SSIM map + every masked sum + the record) on uint8 images, device events
    around `--iters` calls per repeat, median of the repeats; the same with the S map written;
  * frame_metrics() as eval.py calls it (two image assemblies, the mask scatters, the kernel pair and the record's copy to
    the host), host clock around each call (it ends in a synchronising copy);
  * the same metrics through the float64 numpy / scipy restatement on the host (tests/ssim_restatement.py form (a) inlined
    here: scipy.ndimage.uniform_filter as skimage calls it), from the 8-bit images already on the host;
  * eval.py end to end (render + teacher render + metrics + PNG writing) at render_size 512: frames/s from its metrics.json.

It also prints the floor the shapes imply: the bytes every frame has to read (two uint8 images, alpha, body, gt alpha) at
HBM bandwidth.

    python tools/eval_metrics_bench.py [--repeats 7] [--iters 50] [--eval-frames 8] [--no-eval]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBPS = 6.0 * 1.04        # ~6.3 TB/s achievable streaming rate


def host_metrics(rgb, truth, alpha, body, gt_alpha):
    """eval.py:140-196 on host arrays in float64 (SSIM through scipy.ndimage.uniform_filter, as skimage computes it)."""
    from scipy.ndimage import uniform_filter
    x, y = rgb / 255., truth / 255.
    C1, C2, cov = (0.01 * 2) ** 2, (0.03 * 2) ** 2, 49 / 48
    maps = []
    for c in range(3):
        X, Y = x[..., c], y[..., c]
        ux, uy = uniform_filter(X, 7), uniform_filter(Y, 7)
        uxx, uyy, uxy = uniform_filter(X * X, 7), uniform_filter(Y * Y, 7), uniform_filter(X * Y, 7)
        vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
        maps.append(((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2)))
    S = np.stack(maps, -1).reshape(-1, 3)
    mssim = np.mean([m[3:-3, 3:-3].mean() for m in maps])
    bm, vm = body.reshape(-1), alpha.reshape(-1) > np.float32(0.001)
    fx, fy = x.reshape(-1, 3), y.reshape(-1, 3)
    psnr = lambda a, b: -10 * np.log(np.mean((a - b) ** 2)) / np.log(10)  # noqa: E731
    pm, gm = alpha > np.float32(0.1), gt_alpha > np.float32(0.5)
    return (psnr(fx[vm], fy[vm]), S[vm].mean(), psnr(fx[bm], fy[bm]), S[bm].mean(), psnr(x, y), mssim,
            (pm & gm).sum() / (pm | gm).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--eval-frames', type=int, default=8)
    ap.add_argument('--no-eval', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_metrics_bench.json'))
    a = ap.parse_args()
    from occnerf_amd import metrics
    dev = torch.device('cuda', 0)
    H = W = 512
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[:H, :W]
    body = ((yy - 256) ** 2 / 200 ** 2 + (xx - 256) ** 2 / 90 ** 2) < 1          # a body-like blob of rays
    alpha = np.where(body, rng.uniform(0, 1, (H, W)), 0).astype(np.float32)
    gt_alpha = (((yy - 250) ** 2 / 205 ** 2 + (xx - 258) ** 2 / 92 ** 2) < 1).astype(np.float32)
    truth = np.full((H, W, 3), 255, np.uint8)
    truth[body] = rng.integers(0, 256, (body.sum(), 3), dtype=np.uint8)
    rgb = truth.copy()
    rgb[body] = np.clip(truth[body].astype(int) + rng.integers(-25, 26, (body.sum(), 3)), 0, 255)
    d = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(dev)[None]  # noqa: E731
    args = (d(rgb, np.uint8), d(truth, np.uint8), d(alpha, np.float32), d(body, np.uint8), None, d(gt_alpha, np.float32))

    def events(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        per = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        return float(np.median(per)), [float(p) for p in per]

    kern_us, kern_all = events(lambda: metrics.batch_metrics(*args))
    kern_map_us, _ = events(lambda: metrics.batch_metrics(*args, want_map=True))
    rec = metrics.batch_metrics(*args)[0][0].cpu().numpy()

    # frame_metrics as eval.py calls it: device rays in, seven floats out
    mask = body.reshape(-1)
    ray_index = torch.from_numpy(np.nonzero(mask)[0]).to(dev)
    rgb_rays = torch.from_numpy((rgb.reshape(-1, 3)[mask] / 255.).astype(np.float32) + 1e-4).to(dev)
    tgt_rays = torch.from_numpy((truth.reshape(-1, 3)[mask] / 255.).astype(np.float32) + 1e-4).to(dev)
    a_rays = torch.from_numpy(alpha.reshape(-1)[mask]).to(dev)
    gt_map = torch.from_numpy(gt_alpha).to(dev)
    call = lambda: metrics.frame_metrics(rgb_rays, a_rays, ray_index, tgt_rays, W, H, gt_alpha=gt_map)  # noqa: E731
    for _ in range(5):
        call()
    host_ms = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.iters):
            call()
        host_ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
    frame_ms = float(np.median(host_ms))

    cpu_ms = []
    want = None
    for _ in range(3):
        t0 = time.perf_counter()
        want = host_metrics(rgb, truth, alpha, body, gt_alpha)
        cpu_ms.append((time.perf_counter() - t0) * 1e3)
    agree = float(max(abs(float(g) - float(w)) / max(1.0, abs(float(w))) for g, w in zip(rec[:7], want)))

    floor_bytes = H * W * (3 + 3 + 4 + 1 + 4)
    result = {
        'gpu': torch.cuda.get_device_name(0), 'size': [H, W], 'repeats': a.repeats, 'iters': a.iters,
        'kernel_pair_us': kern_us, 'kernel_pair_us_repeats': kern_all, 'kernel_pair_with_S_map_us': kern_map_us,
        'frame_metrics_ms': frame_ms,
        'frame_metrics_note': 'frame_metrics(): two assemble_uint8_device launches, mask scatters, the kernel pair and the '
                              'record copied to the host; host clock, each call ends in the synchronising copy',
        'numpy_scipy_float64_ms': float(np.median(cpu_ms)),
        'numpy_scipy_threads': int(os.environ.get('OMP_NUM_THREADS', '0') or 0),
        'hip_vs_numpy_max_rel_diff': agree,
        'floor_bytes': floor_bytes, 'floor_us_at_hbm': floor_bytes / (HBM_TBPS * 1e12) * 1e6,
    }
    print(f"kernel pair {kern_us:.1f} us (S map written: {kern_map_us:.1f} us); frame_metrics {frame_ms:.3f} ms; "
          f"numpy/scipy float64 {result['numpy_scipy_float64_ms']:.1f} ms; max rel diff {agree:.2e}")

    if not a.no_eval:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [sys.executable, os.path.join(ROOT, 'eval.py'), '--cfg',
                   os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'), 'render_size', '512',
                   'render_frames', str(a.eval_frames)]
            t0 = time.perf_counter()
            subprocess.run(cmd, cwd=tmp, env={**os.environ, 'PYTHONPATH': ROOT}, check=True, capture_output=True, text=True)
            wall = time.perf_counter() - t0
            js = json.load(open(os.path.join(tmp, 'experiments', 'occnerf', 'synthetic', 'capsule_body', 'occnerf', 'seeded',
                                             'eval', 'metrics.json')))
        result['eval_py'] = {'render_size': 512, 'frames': js['n_frames'], 'frames_per_s': js['frames_per_s'],
                             'loop_seconds': js['seconds'], 'process_wall_seconds': wall,
                             'note': 'frames/s over the frame loop (network render + teacher render + metrics + PNG '
                                     'hand-off, first frame included); the process wall time adds start-up and model load'}
        print(f"eval.py 512x512: {js['frames_per_s']:.2f} frames/s over {js['n_frames']} frames ({wall:.1f} s process)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
