"""Measures the resize of a prepared dataset's frames at the size a user runs (1024 x 1024 -> 512 x 512 at
resize_img_scale 0.5): the kernel (csrc/resize.hip through ops.resize_frame), the numpy definition it is held to
(occnerf_amd/resize.py), and the training step fed by the resizing loader against the same step at scale 1.

    bash tools/resize_bench.sh            # every step under its own time limit -> profiles/resize_bench.json

Steps (each a sub-command, so the shell script can bound each one):
  dataset   tools/make_synthetic_dataset.py writes `--frames` frames of 1024 x 1024 and as many of 512 x 512 (CPU);
  kernel    device time per frame from events over `--iters` launches on one 1024 x 1024 frame, for image + mask and for the
            mask alone (a null image), alternating `--repeats` times after a warm-up, beside the bytes a resize must move;
            and the numpy function on the same frame, host clock;
  step      the bf16 training step of tools/train_batch_bench.py fed two ways that alternate inside one process: (r)
            PatchBatchLoader on the 1024 x 1024 frames with resize_frames at 0.5, (p) PatchBatchLoader on the 512 x 512
            frames at scale 1, both with prefetch.  Host clock around steps that end in a device synchronise, so a wait
            inside next() counts.  The two datasets show the same scene at two resolutions, not the same pixels, so the ray
            counts are reported beside the times; the spread of (p) over the repeats is the yardstick for (r) - (p);
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

N_PATCHES, SIZE, RATIO, IMG, SCALE = 6, 32, 0.8, 1024, 0.5
BG = [30., 200., 90.]


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dirs(a):
    return os.path.join(a.dir, 'full'), os.path.join(a.dir, 'half')


def cmd_dataset(a):
    tool = _load(os.path.join(ROOT, 'tools', 'make_synthetic_dataset.py'), 'make_synthetic_dataset')
    t0 = time.perf_counter()
    full, half = _dirs(a)
    tool.make_dataset(full, frames=a.frames, width=IMG, height=IMG, seed=0)
    tool.make_dataset(half, frames=a.frames, width=IMG // 2, height=IMG // 2, seed=0)
    return {'dataset': f'{a.frames} frames of {IMG} x {IMG} and {a.frames} of {IMG // 2} x {IMG // 2}, '
                       'tools/make_synthetic_dataset.py seed 0',
            'dataset_write_s': round(time.perf_counter() - t0, 2)}


def _spread(reps, digits):
    return {'median': round(float(np.median(reps)), digits), 'min': round(float(min(reps)), digits),
            'max': round(float(max(reps)), digits), 'repeats': [round(float(x), digits) for x in reps]}


def cmd_kernel(a):
    import torch
    from PIL import Image
    from occnerf_amd import ops, resize
    assert torch.cuda.is_available(), 'the kernel is timed on a GPU only'
    dev = torch.device('cuda', 0)
    full = _dirs(a)[0]
    img = np.array(Image.open(os.path.join(full, 'images', 'frame_000000.png')).convert('RGB'))
    mask = np.array(Image.open(os.path.join(full, 'masks', 'frame_000000.png')).convert('RGB'))
    host_tables = resize.frame_tables(img.shape[0], img.shape[1], SCALE)
    tables = ops.upload_resize_tables(host_tables, dev)
    h, w = tables['size']
    d_img, d_mask = torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev)
    out = ops.alloc_resize_frame(h, w, dev)
    forms = {'image_and_mask': lambda: ops.resize_frame(d_img, d_mask, tables, BG, out=out),
             'mask_only': lambda: ops.resize_frame(None, d_mask, tables, out=(None, out[1]))}
    for fn in forms.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    reps = {k: [] for k in forms}
    for _ in range(a.repeats):
        for name, fn in forms.items():                                  # alternating within the call
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            reps[name].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    forms['image_and_mask']()
    torch.cuda.synchronize()
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        h_img, h_alpha = resize.resize_blend(img, mask, BG, SCALE, host_tables)
        host.append(time.perf_counter() - t0)
    equal = bool(np.array_equal(out[0].cpu().numpy(), h_img) and np.array_equal(out[1].cpu().numpy(), h_alpha))
    src_px, dst_px = img.shape[0] * img.shape[1], h * w
    moved = src_px * 6 + dst_px * 48
    med = float(np.median(reps['image_and_mask']))
    return {'kernel_what': f'device events over {a.iters} launches on one {IMG} x {IMG} frame -> {w} x {h}, host enqueue '
                           f'included; {a.repeats} alternating repeats of the two forms after 10 warm-up launches each',
            'kernel_image_and_mask_us_per_frame': _spread(reps['image_and_mask'], 2),
            'kernel_mask_only_us_per_frame': _spread(reps['mask_only'], 2),
            'kernel_bytes_read_per_frame': src_px * 6, 'kernel_bytes_written_per_frame': dst_px * 48,
            'kernel_GB_per_s_of_those_bytes': round(moved / (med * 1e-6) / 1e9, 1),
            'kernel_equals_numpy': equal,
            'numpy_image_and_mask_s_per_frame': _spread(host, 4)}


def cmd_step(a):
    import torch
    from occnerf_amd.dataset import NETWORK_KEYS, PatchBatchLoader, PreparedDataset
    from occnerf_amd.optim import FusedAdam
    from occnerf_amd.seeded import build_network
    assert torch.cuda.is_available(), 'the step is timed on a GPU only'
    full, half = _dirs(a)
    sets = {'r_resized': PreparedDataset(full, device='cuda:0', resize_img_scale=SCALE, resize_frames=True),
            'p_plain': PreparedDataset(half, device='cuda:0')}
    assert all((ds.height, ds.width) == (IMG // 2, IMG // 2) for ds in sets.values())
    net = build_network(seed=0, amplify=False, S=128, non_rigid=True)
    net.cfg.perturb = 1.0
    net.train()
    opt = FusedAdam([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    loaders = {m: PatchBatchLoader(ds, N_PATCHES, SIZE, RATIO, seed=1, prefetch=True) for m, ds in sets.items()}
    rows = {m: [] for m in loaders}

    def step(mode):
        batch = next(loaders[mode])
        rows[mode].append(batch['n_rows'])
        opt.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = net(**{k: batch[k] for k in NETWORK_KEYS}, iter_val=1e7)
            loss = 0.2 * torch.mean((out['rgb'].float() - batch['target_rgbs']) ** 2) + out['comp_loss'].float().mean()
        loss.backward()
        opt.step(max_grad_norm=1.0)

    for mode in rows:
        for _ in range(a.warmup):
            step(mode)
    torch.cuda.synchronize()
    times = {m: [] for m in rows}
    for _ in range(a.repeats):
        for mode in rows:                                               # alternating within the call
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                step(mode)
            torch.cuda.synchronize()
            times[mode].append((time.perf_counter() - t0) * 1e3 / a.iters)
    res = {}
    for mode, t in times.items():
        res[f'step_{mode}_ms'] = round(float(np.median(t)), 3)
        res[f'step_{mode}_repeats_ms'] = [round(x, 3) for x in t]
        res[f'step_{mode}_mean_rows'] = round(float(np.mean(rows[mode])), 1)
    spread = max(times['p_plain']) - min(times['p_plain'])
    diff = res['step_r_resized_ms'] - res['step_p_plain_ms']
    res.update({'step_p_spread_ms': round(spread, 3), 'step_r_minus_p_ms': round(diff, 3),
                'step_r_within_spread_of_p': bool(abs(diff) <= spread),
                'step_what': f'bf16 autocast, 128 samples/ray, non-rigid on, clip + Adam; wall clock over {a.iters} steps ending in '
                             f'a synchronise, {a.repeats} alternating repeats; both loaders prefetch and draw a new frame, new '
                             'patches and a new background colour every step; (r) resizes the 1024 x 1024 frame per batch'})
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
    for name in ('dataset', 'kernel', 'step'):
        p = sub.add_parser(name)
        p.add_argument('--dir', required=True)
        p.add_argument('--out')
        p.add_argument('--frames', type=int, default=4)
        p.add_argument('--repeats', type=int, default=7)
        p.add_argument('--iters', type=int, default=50 if name == 'kernel' else 20)
        p.add_argument('--warmup', type=int, default=5)
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
