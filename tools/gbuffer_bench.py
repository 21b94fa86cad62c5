"""Measures the geometry maps of a rendered frame (occnerf_amd/gbuffer.py, csrc/gbuffer.hip) at the
size a user runs: one synthetic 512 x 512 frame (the movement source's frame 0, about 184 K rays) with a seeded depth / alpha
field, and run.py --type movement with and without the panels and the raw export.

    bash tools/gbuffer_bench.sh            # every step under its own time limit -> profiles/gbuffer_bench.json

Steps (each a sub-command, so the shell script can bound each one):
  kernels   device time of the two launches (with all three panels, and with none) from events, host enqueue included, against
            the numpy definition (tests/gbuffer_restatement.py, loaded by path) on the same arrays by the host clock; the
            ways alternate inside one process after a warm-up each, and the outputs are compared before anything is timed;
  movement  one run.py --type movement of `--frames` frames, with the keys (`--geometry 1`) or without; the shell script
            alternates the two.  Frames per second over the frames behind the two warm-up frames, from run.py's own lines;
  merge     the partial results as one JSON object; the repeats of a movement way are collected into a list."""
import argparse
import importlib.util
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMG = 512


def _definition():
    path = os.path.join(ROOT, 'tests', 'gbuffer_restatement.py')
    if not os.path.exists(path):
        raise SystemExit(f'{path}: the numpy definition the kernels are timed against is not there')
    spec = importlib.util.spec_from_file_location('gbuffer_restatement', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _frame():
    """The rays of the movement source's first frame and a smooth seeded depth / alpha field over them."""
    from occnerf_amd import synth
    f = synth.make_frame(img_size=IMG, pose72=synth.movement_pose(0, 100))
    ray_index = np.nonzero(np.asarray(f['ray_mask']).reshape(-1))[0].astype(np.int64)
    i, j = (ray_index // IMG).astype(np.float64), (ray_index % IMG).astype(np.float64)
    rng = np.random.RandomState(0)
    alpha = np.clip(1.2 - ((i - IMG / 2) / 230.0) ** 2 - ((j - IMG / 2) / 120.0) ** 2 + 0.05 * rng.randn(i.size), 0.0, 1.0)
    t = 6.0 + 0.3 * np.sin(i / 23.0) * np.cos(j / 17.0)
    return (f, ray_index, np.ascontiguousarray(f['rays'], dtype=np.float32), (t * alpha).astype(np.float32),
            alpha.astype(np.float32))


def cmd_kernels(a):
    import torch
    from occnerf_amd.gbuffer import PANELS, geometry_maps
    assert torch.cuda.is_available(), 'the kernels are timed on a GPU only'
    G = _definition()
    dev = torch.device('cuda', 0)
    f, ray_index, rays, depth, alpha = _frame()
    R, n = int(ray_index.size), IMG * IMG
    rng = G.default_t_range(f['near'], f['far'])
    d = {k: torch.from_numpy(v).to(dev) for k, v in (('ray_index', ray_index), ('rays', rays), ('depth', depth), ('alpha', alpha))}
    t_range = torch.tensor([float(rng[0]), float(rng[1])], dtype=torch.float32, device=dev)

    def device(panels):
        return geometry_maps(IMG, IMG, d['ray_index'], d['rays'], d['depth'], d['alpha'], 0.5, t_range, (1., 1., 1.), panels)

    t0 = time.perf_counter()
    want = G.geometry_maps(IMG, IMG, ray_index, rays, depth, alpha, 0.5, rng, (1., 1., 1.))
    first_numpy = time.perf_counter() - t0
    got = device(PANELS)
    torch.cuda.synchronize()
    for k in ('points', 'normal', 'valid', 'depth_u8', 'normal_u8', 'shaded_u8'):
        assert np.array_equal(got[k].cpu().numpy().view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), k

    def events(panels):
        for _ in range(10):
            device(panels)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            device(panels)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    def host(_):
        t0 = time.perf_counter()
        G.geometry_maps(IMG, IMG, ray_index, rays, depth, alpha, 0.5, rng, (1., 1., 1.))
        return (time.perf_counter() - t0) * 1e6

    ways = {'kernels_all_panels': lambda: events(PANELS), 'kernels_no_panel': lambda: events(()), 'numpy': lambda: host(None)}
    reps = {k: [] for k in ways}
    for _ in range(a.repeats):
        for k, fn in ways.items():                                      # alternating within the call
            reps[k].append(fn())
    valid = want['valid']
    res = {'gbuffer_what': f'one {IMG} x {IMG} frame of the synthetic movement source, {R} rays, seeded depth / alpha field; the '
                           f'two launches of csrc/gbuffer.hip through gbuffer.geometry_maps from device events over {a.iters} '
                           f'calls, host enqueue and output allocation included; the numpy definition by the host clock on the '
                           f'same arrays; {a.repeats} alternating repeats after a warm-up each; outputs equal before timing',
           'gbuffer_rays': R, 'gbuffer_depth_valid_pixels': int((valid & 1).sum()), 'gbuffer_normal_valid_pixels': int((valid >> 1).sum()),
           # launch 1: the search's probes hit L2; compulsory: ray_index + rays + depth + alpha in, points + valid + column out
           'gbuffer_bytes_read': R * (8 + 24 + 4 + 4) + n * (4 + 16) + R * 12,
           'gbuffer_bytes_written_all_panels': n * (16 + 1 + 4) + n * (12 + 1 + 9),
           'gbuffer_numpy_first_call_s': round(first_numpy, 3)}
    for k, t in reps.items():
        res[f'gbuffer_{k}_us_per_frame'] = round(float(np.median(t)), 2)
        res[f'gbuffer_{k}_repeats_us'] = [round(x, 2) for x in t]
    return res


def cmd_movement(a):
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'),
           '--type', 'movement', 'render_size', str(IMG), 'render_frames', str(a.frames), 'show_alpha', 'True']
    if a.geometry:
        cmd += ['show_depth', 'True', 'show_normal', 'True', 'show_shaded', 'True', 'geometry.save', 'True',
                'geometry.min_alpha', str(a.min_alpha)]
    t0 = time.perf_counter()
    out = subprocess.run(cmd, cwd=a.dir, env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True)
    wall = time.perf_counter() - t0
    if out.returncode != 0:
        sys.stderr.write(out.stderr[-3000:])
        raise SystemExit(out.returncode)
    total = re.search(r'(\d+) rays in ([0-9.]+) s', out.stdout)
    warm = re.search(r'warm-up, pipelined\) (\d+) ms', out.stdout)
    steady = (a.frames - 2) / (float(total.group(2)) - float(warm.group(1)) * 1e-3)
    key = 'movement_geometry' if a.geometry else 'movement_plain'
    extra = {}
    if a.geometry:                                              # how much of each frame the maps actually cover in this run
        import glob
        maps = sorted(glob.glob(os.path.join(a.dir, 'experiments', 'occnerf', 'synthetic', 'capsule_body', 'occnerf', 'seeded',
                                             'movement_geometry', '*.npz')))
        assert len(maps) == a.frames, (len(maps), a.frames)
        valid = [np.load(m)['valid'] for m in maps]
        extra = {'movement_geometry_depth_valid_pixels_per_frame': round(float(np.mean([(v & 1).sum() for v in valid])), 1),
                 'movement_geometry_normal_valid_pixels_per_frame': round(float(np.mean([(v >> 1).sum() for v in valid])), 1)}
    return {**extra, f'{key}_frames_per_s': round(steady, 3), f'{key}_process_wall_s': round(wall, 2),
            'movement_what': f'run.py --type movement, {a.frames} synthetic frames of {IMG} x {IMG}, show_alpha; frames per second '
                             'behind the two warm-up frames from run.py\'s own clock (render, assembly and the hand-over to the '
                             'writer thread; PNG and npz writing run beside it); geometry = show_depth, show_normal, show_shaded and '
                             f'geometry.save at min_alpha {a.min_alpha} (the kernels do the same work per pixel whether or not a pixel turns out valid; '
                             'the valid pixels per frame are recorded); run.py prints its clock to 1 ms, which quantises the figure; the '
                             'two ways alternate, one process each'}


def cmd_merge(a):
    res = {}
    for p in a.parts:
        with open(p) as f:
            for k, v in json.load(f).items():
                if k.endswith('_frames_per_s') or k.endswith('_process_wall_s'):
                    res.setdefault(k, []).append(v)
                else:
                    res[k] = v
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    p = sub.add_parser('kernels')
    p.add_argument('--out')
    p.add_argument('--repeats', type=int, default=7)
    p.add_argument('--iters', type=int, default=200)
    p = sub.add_parser('movement')
    p.add_argument('--dir', required=True)
    p.add_argument('--out')
    p.add_argument('--frames', type=int, default=12)
    p.add_argument('--geometry', type=int, default=0)
    p.add_argument('--min-alpha', dest='min_alpha', type=float, default=0.5)
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
