"""Measures the training batch of a prepared dataset at the size a user runs: 512 x 512 frames, 6 patches of 32 x 32.

    bash tools/train_batch_bench.sh            # every step under its own time limit -> profiles/train_batch_bench.json

Steps (each a sub-command, so the shell script can bound each one):
  dataset      tools/make_synthetic_dataset.py writes the frames (CPU);
  builder      the device builder's time per batch -- ops.gen_rays + ops.patch_batch, four launches -- from device events;
  restatement  the numpy restatement of the reference's Dataset.__getitem__ (tests/train_batch_restatement.py, loaded by
               path: the one tool that reads the test tree, and it says "not measured" when the tree is absent), wall time per
               batch on the CPUs this process is granted;
  step         the bf16 training step (train.py's: forward, ray-wise MSE + comp, backward, clip + Adam) fed three ways that
               alternate inside one process: (a) one pre-built device batch, reused; (b) PatchBatchLoader with prefetch;
               (c) the loader without prefetch.  Host clock around steps that end in a device synchronise, so a wait inside
               next() counts.  The spread of (a) over the alternating repeats is the yardstick for (b) - (a);
  merge        the partial results as one JSON object.
(a) against BENCH_r06.json's train.ms_per_step is a sanity line only: the inputs differ."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_PATCHES, SIZE, RATIO, IMG = 6, 32, 0.8, 512


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
    assert torch.cuda.is_available(), 'the builder is timed on a GPU only'
    ds = PreparedDataset(a.dir, device='cuda:0')
    out = ops.alloc_patch_batch(N_PATCHES, SIZE, ds.height, ds.device)
    rays8 = torch.empty(ds.height * ds.width, 8, device=ds.device)
    box = torch.empty(ds.height * ds.width, device=ds.device, dtype=torch.uint8)
    rng = np.random.RandomState(0)
    draws = [(i % len(ds), rng.rand(N_PATCHES, 2), (rng.rand(3) * 255).astype('float32')) for i in range(64)]

    def build(i):
        frame, u, bg = draws[i % len(draws)]
        f = ds.frames[frame]
        ops.gen_rays(f['K'], f['E'], ds.height, ds.width, f['dst_bbox_min'], f['dst_bbox_max'], ds.device, out=(rays8, box))
        ops.patch_batch(ds._dev['image'][frame], ds._dev['alpha'][frame], rays8, box, N_PATCHES, SIZE, u, RATIO, bg, out=out)

    for i in range(20):
        build(i)
    torch.cuda.synchronize()
    reps = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.iters):
            build(i)
        e1.record()
        torch.cuda.synchronize()
        reps.append(e0.elapsed_time(e1) / a.iters)
    return {'builder_ms_per_batch': round(float(np.median(reps)), 4), 'builder_repeats_ms': [round(x, 4) for x in reps],
            'builder_what': f'gen_rays + patch_batch (4 launches), device events over {a.iters} batches, host enqueue included',
            'builder_rows_last_batch': int(out['n_rows'].item())}


def cmd_restatement(a):
    path = os.path.join(ROOT, 'tests', 'train_batch_restatement.py')
    if not os.path.exists(path):
        return {'restatement_ms_per_batch': 'not measured', 'restatement_what': 'tests/train_batch_restatement.py is absent'}
    tbr = _load(path, 'train_batch_restatement')
    rs = tbr.Restatement(a.dir, N_patches=N_PATCHES, size=SIZE)
    rng = np.random.RandomState(0)
    reps = []
    for i in range(a.repeats + 1):
        frame = i % len(rs.framelist)
        _, _, subject, off = rs.frame_masks(frame)                      # not timed: only to turn uniforms into draws
        draws = tbr.draws_from_uniforms(rng.rand(N_PATCHES, 2), subject, off, RATIO)
        t0 = time.perf_counter()
        rs.getitem(frame, (rng.rand(3) * 255).astype('float32'), draws)
        reps.append((time.perf_counter() - t0) * 1e3)
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else os.cpu_count()
    return {'restatement_ms_per_batch': round(float(np.median(reps[1:])), 2), 'restatement_repeats_ms': [round(x, 2) for x in reps[1:]],
            'restatement_what': f'numpy __getitem__ in one process (PNG decode included, as the reference does per item); '
                                f'{cpus} CPUs in the affinity mask, OMP_NUM_THREADS={os.environ.get("OMP_NUM_THREADS")}'}


def cmd_step(a):
    import torch
    from occnerf_amd.dataset import NETWORK_KEYS, PatchBatchLoader, PreparedDataset
    from occnerf_amd.optim import FusedAdam
    from occnerf_amd.seeded import build_network
    assert torch.cuda.is_available(), 'the step is timed on a GPU only'
    ds = PreparedDataset(a.dir, device='cuda:0')
    net = build_network(seed=0, amplify=False, S=128, non_rigid=True)
    net.cfg.perturb = 1.0
    net.train()
    opt = FusedAdam([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    loaders = {'b_prefetch': PatchBatchLoader(ds, N_PATCHES, SIZE, RATIO, seed=1, prefetch=True),
               'c_inline': PatchBatchLoader(ds, N_PATCHES, SIZE, RATIO, seed=1, prefetch=False)}
    fixed = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in next(PatchBatchLoader(ds, N_PATCHES, SIZE, RATIO, seed=1,
                                                                                         prefetch=False)).items()}
    rows = {'a_fixed': [], 'b_prefetch': [], 'c_inline': []}

    def step(mode):
        batch = fixed if mode == 'a_fixed' else next(loaders[mode])
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
    spread = max(times['a_fixed']) - min(times['a_fixed'])
    diff = res['step_b_prefetch_ms'] - res['step_a_fixed_ms']
    res.update({'step_a_spread_ms': round(spread, 3), 'step_b_minus_a_ms': round(diff, 3),
                'step_b_within_spread_of_a': bool(abs(diff) <= spread),
                'step_what': f'bf16 autocast, 128 samples/ray, non-rigid on, clip + Adam; wall clock over {a.iters} steps ending in '
                             f'a synchronise, {a.repeats} alternating repeats; (a) reuses one batch, (b)/(c) draw a new frame and '
                             'new patches every step, so their ray counts and sample occupancy vary',
                'sanity_parent_train_ms_per_step': 17.1})
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
    for name in ('dataset', 'builder', 'restatement', 'step'):
        p = sub.add_parser(name)
        p.add_argument('--dir', required=True)
        p.add_argument('--out')
        p.add_argument('--frames', type=int, default=8)
        p.add_argument('--repeats', type=int, default=7)
        p.add_argument('--iters', type=int, default=20)
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
