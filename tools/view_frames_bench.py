"""Measures the ray batch of a derived camera (occnerf_amd/views.py) at the size a user runs: the freeview orbit of an
8-frame 512 x 512 tool-made dataset, built by the device builder (occnerf_gen_rays + occnerf_whole_frame_count +
csrc/view.hip's gather through ops.view_frame) and by rays.frame_rays (the synthetic path: gen_rays, then torch boolean
indexing, torch.stack and torch.nonzero) for the same cameras.

    bash tools/view_frames_bench.sh            # every step under its own time limit -> profiles/view_frames_bench.json

Steps (each a sub-command, so the shell script can bound each one):
  dataset   tools/make_synthetic_dataset.py writes the frames (CPU);
  builder   device time per orbit frame from events, host enqueue included, the two ways alternating inside one process after
            a warm-up pass each.  The builder's R is known from the warm-up, as it is behind the loader's event; frame_rays
            reads its sizes back itself (that read is part of what it costs).  The outputs are compared before anything is
            timed;
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

IMG = 512


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


def cmd_builder(a):
    import torch
    from occnerf_amd import ops
    from occnerf_amd.dataset import PreparedDataset
    from occnerf_amd.rays import frame_rays
    from occnerf_amd.views import ViewFrames
    assert torch.cuda.is_available(), 'the builder is timed on a GPU only'
    dev = torch.device('cuda', 0)
    loader = ViewFrames(PreparedDataset(a.dir, device=None), 'freeview', render_frames=a.cameras, frame_idx=0)
    H, W, n = loader.height, loader.width, len(loader)
    views = [loader.view(i) for i in range(n)]
    rays8 = torch.empty(H * W, 8, device=dev)
    box = torch.empty(H * W, device=dev, dtype=torch.uint8)
    row_start = torch.empty(H + 1, device=dev, dtype=torch.int32)

    def build(i, R=None):
        v = views[i % n]
        ops.gen_rays(v['K'], v['E'], H, W, v['min'], v['max'], dev, out=(rays8, box))
        ops.whole_frame_count(box, H, W, row_start)
        return ops.view_frame(rays8, box, H, W, row_start=row_start, R=int(row_start[H].item()) if R is None else R)

    def torch_way(i):
        v = views[i % n]
        fr = frame_rays(v['K'], v['E'], H, W, v['min'], v['max'], dev)
        return dict(fr, ray_index=torch.nonzero(fr['ray_mask']).squeeze(1))

    counts = []
    for i in range(n):                                                  # warm-up of both, and the outputs compared
        got, want = build(i), torch_way(i)
        counts.append(int(got['ray_index'].numel()))
        for k in ('ray_index', 'rays', 'near', 'far'):
            assert torch.equal(got[k], want[k]), (i, k)

    def events(fn):
        for i in range(n):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.iters):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    ways = {'builder': lambda i: build(i, counts[i % n]), 'frame_rays': torch_way}
    reps = {k: [] for k in ways}
    for _ in range(a.repeats):
        for k, fn in ways.items():                                      # alternating within the call
            reps[k].append(events(fn))
    mean_r = int(np.mean(counts))
    res = {'view_what': f'device events over {a.iters} orbit frames ({n} cameras around frame 0), host enqueue included; '
                        f'{a.repeats} alternating repeats after a warm-up pass each; outputs equal before timing',
           'view_rays_per_frame': counts,
           'view_gather_bytes_read_per_frame': H * W + (H + 1) * 4 + mean_r * 32,
           'view_gather_bytes_written_per_frame': mean_r * 36}
    for k, t in reps.items():
        res[f'view_{k}_us_per_frame'] = round(float(np.median(t)), 2)
        res[f'view_{k}_repeats_us'] = [round(x, 2) for x in t]
    return res


def cmd_merge(a):
    res = {}
    for p in a.parts:
        with open(p) as f:
            res.update(json.load(f))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    for name in ('dataset', 'builder'):
        p = sub.add_parser(name)
        p.add_argument('--dir', required=True)
        p.add_argument('--out')
        p.add_argument('--frames', type=int, default=8)
        p.add_argument('--cameras', type=int, default=8)
        p.add_argument('--repeats', type=int, default=7)
        p.add_argument('--iters', type=int, default=200)
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
