"""Measures the whole frames of a prepared dataset at the size a user runs: 8 tool-made frames of 512 x 512, built on the
host (PreparedDataset.whole_frame, numpy, then frames_to_device's upload: the path `device_frames False` selects) and on the
device (csrc/frame.hip through WholeFrames.device_frames).

    bash tools/whole_frame_bench.sh            # every step under its own time limit -> profiles/whole_frame_bench.json

Steps (each a sub-command, so the shell script can bound each one):
  dataset   tools/make_synthetic_dataset.py writes the frames (CPU);
  loader    (a) the host frames through frames_to_device, (b) device_frames with and without prefetch: host clock per frame
            over a pass of all frames that ends in a device synchronise, nothing rendered in between; the three alternate
            inside one process after a warm-up pass each, `--repeats` times;
  builder   (c) the builder's device time per frame from events: gen_rays + count (2 launches) + gather, the host read of R
            between them left out (R is known from the warm-up);
  eval      (d) eval.py's frame loop -- build, render at 128 samples per ray, metrics; no PNG is written -- frames/s with host
            frames and with device frames, alternating inside one process after a warm-up pass each.  The spread of the host
            passes is the yardstick for the difference;
  merge     the partial results as one JSON object."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMG, BGCOLOR = 512, [255., 255., 255.]


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cmd_dataset(a):
    t0 = time.perf_counter()
    _load(os.path.join(ROOT, 'tools', 'make_synthetic_dataset.py'), 'make_synthetic_dataset').make_dataset(
        a.dir, frames=a.frames, width=IMG, height=IMG, seed=0)
    return {'dataset': f'{a.frames} frames of {IMG} x {IMG}, tools/make_synthetic_dataset.py seed 0',
            'dataset_write_s': round(time.perf_counter() - t0, 2)}


def _loader(a):
    from occnerf_amd.dataset import PreparedDataset, WholeFrames
    return WholeFrames(PreparedDataset(a.dir, device=None), BGCOLOR)


def _frames(loader, mode, dev):
    """The (data, key, meta) triples of one pass: 'host' | 'device_prefetch' | 'device_inline'."""
    from occnerf_amd.config import get_cfg
    from occnerf_amd.sequence import frames_to_device
    if mode == 'device_inline':
        return loader.device_frames(dev, prefetch=False, data_type='movement')
    get_cfg().device_frames = mode != 'host'
    return frames_to_device(loader, 'movement', dev)


def cmd_loader(a):
    import torch
    assert torch.cuda.is_available(), 'the loaders are timed on a GPU only'
    dev, loader = torch.device('cuda', 0), _loader(a)
    modes = ('host', 'device_prefetch', 'device_inline')
    rays = {}

    def one_pass(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for data, _key, meta in _frames(loader, mode, dev):
            n += int(data['rays'].shape[1])
        torch.cuda.synchronize()
        rays[mode] = n
        return (time.perf_counter() - t0) * 1e3 / len(loader)

    for mode in modes:
        one_pass(mode)
    times = {m: [] for m in modes}
    for _ in range(a.repeats):
        for mode in modes:                                              # alternating within the call
            times[mode].append(one_pass(mode))
    res = {'loader_what': f'host clock per frame over a pass of {len(loader)} frames ending in a synchronise, nothing rendered '
                          f'in between; {a.repeats} alternating repeats after one warm-up pass each',
           'loader_rays_per_pass': rays}
    for mode, t in times.items():
        res[f'loader_{mode}_ms_per_frame'] = round(float(np.median(t)), 3)
        res[f'loader_{mode}_repeats_ms'] = [round(x, 3) for x in t]
    return res


def cmd_builder(a):
    import torch
    from occnerf_amd import ops
    from occnerf_amd.dataset import PreparedDataset
    assert torch.cuda.is_available(), 'the builder is timed on a GPU only'
    ds = PreparedDataset(a.dir, device='cuda:0')
    H, W, dev = ds.height, ds.width, ds.device
    rays8 = torch.empty(H * W, 8, device=dev)
    box = torch.empty(H * W, device=dev, dtype=torch.uint8)
    row_start = torch.empty(H + 1, device=dev, dtype=torch.int32)
    bg = np.array(BGCOLOR, 'float32')
    counts, outs = [], []
    for i in range(len(ds)):                                            # warm-up: R and the output buffers of every frame
        f = ds.frames[i]
        ops.gen_rays(f['K'], f['E'], H, W, f['dst_bbox_min'], f['dst_bbox_max'], dev, out=(rays8, box))
        ops.whole_frame_count(box, H, W, row_start)
        counts.append(int(row_start[H].item()))
        outs.append(ops.alloc_whole_frame(H, W, counts[-1], dev))

    def build(i, rays=True):
        i %= len(ds)
        f = ds.frames[i]
        if rays:
            ops.gen_rays(f['K'], f['E'], H, W, f['dst_bbox_min'], f['dst_bbox_max'], dev, out=(rays8, box))
        ops.whole_frame_count(box, H, W, row_start)
        ops.whole_frame(ds._dev['image'][i], ds._dev['alpha'][i], rays8, box, bg, row_start=row_start, R=counts[i], out=outs[i])

    def events(fn):
        for i in range(2 * len(ds)):
            fn(i)
        torch.cuda.synchronize()
        reps = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.iters):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            reps.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        return round(float(np.median(reps)), 2), [round(x, 2) for x in reps]

    full, full_reps = events(build)
    # frame 0 only, its rays left in place: the builder's own three launches
    f = ds.frames[0]
    ops.gen_rays(f['K'], f['E'], H, W, f['dst_bbox_min'], f['dst_bbox_max'], dev, out=(rays8, box))
    own, own_reps = events(lambda i: build(0, rays=False))
    read = H * W * (3 + 3 + 1 + 1) + int(np.mean(counts)) * 32
    write = H * W * (3 + 4 + 4) + int(np.mean(counts)) * (8 + 24 + 8 + 12 + 24)
    return {'builder_us_per_frame': full, 'builder_repeats_us': full_reps, 'builder_own_launches_us_per_frame': own,
            'builder_own_launches_repeats_us': own_reps,
            'builder_what': f'device events over {a.iters} frames, host enqueue included: gen_rays + count (2 launches) + gather; '
                            '"own launches": count + gather on one frame whose rays stay in place',
            'builder_rays_per_frame': counts, 'builder_bytes_read_per_frame': read, 'builder_bytes_written_per_frame': write}


def cmd_eval(a):
    import torch
    from occnerf_amd import metrics
    from occnerf_amd.parallel import ShardedRenderer
    from occnerf_amd.seeded import build_network
    assert torch.cuda.is_available(), 'the eval loop is timed on a GPU only'
    dev, loader = torch.device('cuda', 0), _loader(a)
    renderer = ShardedRenderer(build_network(seed=0, amplify=True, S=128, non_rigid=True), dev)
    bg = np.array(BGCOLOR) / 255.
    last = {}

    def one_pass(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for data, _key, meta in _frames(loader, mode, dev):
                out = renderer.finish(renderer.submit(data, iter_val=1e7))
                W, H, ray_index = meta['width'], meta['height'], meta['ray_index']
                if 'truth_u8' in meta:
                    m = metrics.frame_metrics_from_maps(out['rgb'], out['alpha'], ray_index, meta, W, H, bgcolor=bg)
                else:
                    alpha = loader.dataset.alphas[meta['idx']]
                    gt_alpha = torch.from_numpy((alpha[:, :, 0] / 255.).astype('float32')).to(dev)
                    m = metrics.frame_metrics(out['rgb'], out['alpha'], ray_index, data['target_rgbs'], W, H,
                                              ray_alpha=data['ray_alpha'], gt_alpha=gt_alpha, bgcolor=bg)
                last[mode] = m
        torch.cuda.synchronize()
        return len(loader) / (time.perf_counter() - t0)

    modes = ('host', 'device_prefetch')
    for mode in modes:
        one_pass(mode)
    fps = {m: [] for m in modes}
    for _ in range(a.repeats):
        for mode in modes:
            fps[mode].append(one_pass(mode))
    host, device = float(np.median(fps['host'])), float(np.median(fps['device_prefetch']))
    spread = max(fps['host']) - min(fps['host'])
    return {'eval_host_frames_per_s': round(host, 3), 'eval_host_repeats': [round(x, 3) for x in fps['host']],
            'eval_device_frames_per_s': round(device, 3), 'eval_device_repeats': [round(x, 3) for x in fps['device_prefetch']],
            'eval_host_spread_frames_per_s': round(spread, 3), 'eval_device_minus_host_frames_per_s': round(device - host, 3),
            'eval_device_not_slower_than_host_by_more_than_the_spread': bool(device >= host - spread),
            'eval_last_frame_metrics_equal': bool(all(last['host'][k] == last['device_prefetch'][k] for k in ('psnr_full', 'ssim_full'))),
            'eval_what': f"eval.py's frame loop in one process: frame build, render (seeded amplified checkpoint, 128 samples "
                         f'per ray, non-rigid on), metrics; no PNG written; {len(loader)} frames per pass, {a.repeats} '
                         'alternating repeats after one warm-up pass each'}


def cmd_merge(a):
    res = {}
    for p in a.parts:
        with open(p) as f:
            res.update(json.load(f))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    for name in ('dataset', 'loader', 'builder', 'eval'):
        p = sub.add_parser(name)
        p.add_argument('--dir', required=True)
        p.add_argument('--out')
        p.add_argument('--frames', type=int, default=8)
        p.add_argument('--repeats', type=int, default=3 if name in ('loader', 'eval') else 7)
        p.add_argument('--iters', type=int, default=40)
    p = sub.add_parser('merge')
    p.add_argument('parts', nargs='+')
    p.add_argument('--out')
    a = ap.parse_args()
    res = globals()['cmd_' + a.cmd](a)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
