"""Measures run.py --type animate (occnerf_amd/animate.py, occnerf_amd/skeleton.py, csrc/skeleton.hip)
at the size a user runs: the skeleton panel of one 512 x 512 frame, and the animate sequence of a tool-made 512 x 512 dataset
driven by its own motion, with and without the panel, beside --type movement of the same dataset.

    bash tools/animate_bench.sh [OUT.json [PARENT_TREE]]      # every step under its own time limit -> profiles/animate_bench.json

Steps (each a sub-command, so the shell script can bound each one):
  kernel    device time of the one launch from events, host enqueue and output allocation included, against the numpy
            definition (tests/skeleton_restatement.py, loaded by path) for the same bytes by the host clock; the two ways
            alternate inside one process after a warm-up each, and the outputs are compared before anything is timed;
  dataset   the tool-made dataset every render step reads;
  render    one run.py process: `--way animate`, `animate_skeleton` or `movement`.  `--tree DIR` runs the run.py of another
            checkout with its own built library -- the parent commit for the movement way; without it this tree's.  Frames
            per second over the frames behind the two warm-up frames, from run.py's own lines;
  merge     the partial results as one JSON object; the repeats of a way are collected into a list."""
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


def _load(path, name):
    if not os.path.exists(path):
        raise SystemExit(f'{path}: not there')
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cmd_kernel(a):
    import torch
    from occnerf_amd import synth
    from occnerf_amd.skeleton import BONE_PX, PALETTE, background_u8, counts, skeleton_panel
    assert torch.cuda.is_available(), 'the kernel is timed on a GPU only'
    S = _load(os.path.join(ROOT, 'tests', 'skeleton_restatement.py'), 'skeleton_restatement')
    dev = torch.device('cuda', 0)
    joints = synth.posed_joints(synth.seeded_pose(3), synth.tpose_joints(np.zeros(10, dtype='float32'))).astype(np.float32)
    K, E = (m.astype(np.float64) for m in synth.setup_camera(IMG))
    bg = [255., 255., 255.]

    def device():
        return skeleton_panel(joints, K, E, IMG, IMG, dev, bone_px=BONE_PX, bgcolor=bg)

    def definition():
        return S.skeleton_panel(joints, K, E, IMG, IMG, BONE_PX, PALETTE, background_u8(bg))

    want = definition()
    img, record = device()
    torch.cuda.synchronize()
    assert np.array_equal(img.cpu().numpy(), want['img']) and counts(record) == {'dropped': want['dropped'], 'covered': want['covered']}

    def events():
        for _ in range(10):
            device()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            device()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    def host():
        t0 = time.perf_counter()
        definition()
        return (time.perf_counter() - t0) * 1e6

    ways = {'kernel': events, 'numpy': host}
    reps = {k: [] for k in ways}
    for _ in range(a.repeats):
        for k, fn in ways.items():                                      # alternating within the call
            reps[k].append(fn())
    res = {'skeleton_what': f'the skeleton panel of one {IMG} x {IMG} frame (a seeded pose through the tpose camera, bone_px '
                            f'{BONE_PX}): the one launch of csrc/skeleton.hip through skeleton.skeleton_panel from device events over '
                            f'{a.iters} calls, host enqueue and the allocation of the two outputs included; the numpy definition by '
                            f'the host clock for the same bytes; {a.repeats} alternating repeats after a warm-up each; outputs '
                            'equal before timing',
           'skeleton_pixels_covered': want['covered'], 'skeleton_joints_dropped': want['dropped'],
           'skeleton_bytes_written': IMG * IMG * 3 + 4 * int(record.numel()),
           'skeleton_float64_operations': IMG * IMG * 47 * 20}
    for k, t in reps.items():
        res[f'skeleton_{k}_us_per_frame'] = round(float(np.median(t)), 2)
        res[f'skeleton_{k}_repeats_us'] = [round(x, 2) for x in t]
    return res


def cmd_dataset(a):
    tool = _load(os.path.join(ROOT, 'tools', 'make_synthetic_dataset.py'), 'make_synthetic_dataset')
    tool.make_dataset(a.data, frames=a.frames, width=IMG, height=IMG, seed=0)
    return {'dataset_what': f'tools/make_synthetic_dataset.py: {a.frames} frames of {IMG} x {IMG}, seed 0'}


def cmd_render(a):
    tree = os.path.abspath(a.tree) if a.tree else ROOT
    cmd = [sys.executable, os.path.join(tree, 'run.py'), '--cfg', os.path.join(tree, 'configs/occnerf/synthetic/occnerf.yaml'),
           '--type', 'movement' if a.way == 'movement' else 'animate', 'train.dataset_path', a.data, 'resize_img_scale', '1.0',
           'load_net', 'seeded', 'show_alpha', 'True']
    if a.way != 'movement':                                     # the dataset's own motion, as it is: movement's poses and places
        cmd += ['animate.motion', a.data, 'animate.align', 'False']
    if a.way == 'animate_skeleton':
        cmd += ['show_skeleton', 'True']
    t0 = time.perf_counter()
    out = subprocess.run(cmd, cwd=a.dir, env={**os.environ, 'PYTHONPATH': tree}, capture_output=True, text=True)
    wall = time.perf_counter() - t0
    if out.returncode != 0:
        sys.stderr.write(out.stderr[-3000:])
        raise SystemExit(out.returncode)
    total = re.search(r'(\d+) rays in ([0-9.]+) s', out.stdout)
    warm = re.search(r'warm-up, pipelined\) (\d+) ms', out.stdout)
    frames = len([f for f in os.listdir(os.path.join(a.data, 'images')) if f.endswith('.png')])
    steady = (frames - 2) / (float(total.group(2)) - float(warm.group(1)) * 1e-3)
    return {f'{a.way}_frames_per_s': round(steady, 3), f'{a.way}_process_wall_s': round(wall, 2), f'{a.way}_rays': int(total.group(1)),
            'movement_tree': 'the parent commit' if a.tree and a.way == 'movement' else 'this commit',
            'render_what': f'run.py on a tool-made dataset of {frames} frames of {IMG} x {IMG}, seeded checkpoint, 128 samples, '
                           'show_alpha; animate = the dataset as its own motion (align False, substeps 1, camera fixed: the poses '
                           'and places of movement, every frame through frame 0\'s camera); animate_skeleton adds show_skeleton; '
                           'frames per second behind the two warm-up frames from run.py\'s own clock, which is printed to 1 ms; '
                           'the ways alternate, one process each'}


def cmd_merge(a):
    res = {}
    for p in a.parts:
        with open(p) as f:
            for k, v in json.load(f).items():
                if k.endswith('_frames_per_s') or k.endswith('_process_wall_s'):
                    res.setdefault(k, []).append(v)
                elif k == 'movement_tree':
                    if v != 'this commit' or k not in res:
                        res[k] = v
                else:
                    res[k] = v
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    p = sub.add_parser('kernel')
    p.add_argument('--out')
    p.add_argument('--repeats', type=int, default=7)
    p.add_argument('--iters', type=int, default=200)
    p = sub.add_parser('dataset')
    p.add_argument('--data', required=True)
    p.add_argument('--frames', type=int, default=12)
    p.add_argument('--out')
    p = sub.add_parser('render')
    p.add_argument('--way', required=True, choices=('animate', 'animate_skeleton', 'movement'))
    p.add_argument('--data', required=True)
    p.add_argument('--dir', required=True)
    p.add_argument('--tree', default=None)
    p.add_argument('--out')
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
