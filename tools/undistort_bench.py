"""Measures the undistortion of a prepared dataset's frames at the size a user runs (1024 x 1024): the kernel
(csrc/undistort.hip through ops.undistort_u8), the numpy definition it is held to (occnerf_amd/undistort.py), and the open
of a distorted dataset with a device and without one.

    bash tools/undistort_bench.sh            # every step under its own time limit -> profiles/undistort_bench.json

Steps (each a sub-command, so the shell script can bound each one):
  dataset   tools/make_synthetic_dataset.py writes 8 distorted frames (CPU);
  kernel    device time per frame from events over `--iters` launches on one frame of the dataset, for image + mask (six
            channels from one map) and for the image alone (a null mask), alternating `--repeats` times after a warm-up; and
            the numpy function on the same frame (image, then mask), host clock;
  open      PreparedDataset(prepare_frames=True) with device 'cuda:0' and with device=None, host clock over the whole open
            (PNG decoding, per-frame constants, the upload of the prepared frames), alternating `--repeats` times after one
            warm-up open each;
  merge     the partial results as one JSON object."""
import argparse
import importlib.util
import json
import os
import pickle
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMG, DIST = 1024, (-0.28, 0.11, 0.0012, -0.0009, -0.03)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cmd_dataset(a):
    t0 = time.perf_counter()
    _load(os.path.join(ROOT, 'tools', 'make_synthetic_dataset.py'), 'make_synthetic_dataset').make_dataset(
        a.dir, frames=a.frames, width=IMG, height=IMG, seed=0, distortions=DIST)
    return {'dataset': f'{a.frames} frames of {IMG} x {IMG}, tools/make_synthetic_dataset.py seed 0, distortions {list(DIST)}',
            'dataset_write_s': round(time.perf_counter() - t0, 2)}


def _spread(reps, digits):
    return {'median': round(float(np.median(reps)), digits), 'min': round(float(min(reps)), digits),
            'max': round(float(max(reps)), digits), 'repeats': [round(float(x), digits) for x in reps]}


def cmd_kernel(a):
    import torch
    from PIL import Image
    from occnerf_amd import ops
    from occnerf_amd.undistort import undistort_u8
    assert torch.cuda.is_available(), 'the kernel is timed on a GPU only'
    dev = torch.device('cuda', 0)
    with open(os.path.join(a.dir, 'cameras.pkl'), 'rb') as f:
        cam = pickle.load(f)['frame_000000']
    K, D = cam['intrinsics'], cam['distortions']
    img = np.array(Image.open(os.path.join(a.dir, 'images', 'frame_000000.png')).convert('RGB'))
    mask = np.array(Image.open(os.path.join(a.dir, 'masks', 'frame_000000.png')).convert('RGB'))
    d_img, d_mask = torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev)
    out = (torch.empty_like(d_img), torch.empty_like(d_mask))
    forms = {'image_and_mask': lambda: ops.undistort_u8(d_img, d_mask, K, D, out=out),
             'image_only': lambda: ops.undistort_u8(d_img, None, K, D, out=(out[0], None))}
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
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        h_img, h_mask = undistort_u8(img, K, D), undistort_u8(mask, K, D)
        host.append(time.perf_counter() - t0)
    equal = bool(np.array_equal(out[0].cpu().numpy(), h_img) and np.array_equal(out[1].cpu().numpy(), h_mask))
    px = img.shape[0] * img.shape[1]
    return {'kernel_what': f'device events over {a.iters} launches on one {IMG} x {IMG} frame, host enqueue included; '
                           f'{a.repeats} alternating repeats of the two forms after 10 warm-up launches each',
            'kernel_image_and_mask_us_per_frame': _spread(reps['image_and_mask'], 2),
            'kernel_image_only_us_per_frame': _spread(reps['image_only'], 2),
            'kernel_bytes_written_per_frame': px * 6, 'kernel_bytes_gathered_per_frame': px * 24,
            'kernel_equals_numpy': equal,
            'numpy_image_and_mask_s_per_frame': _spread(host, 4)}


def cmd_open(a):
    import torch
    from occnerf_amd.dataset import PreparedDataset
    assert torch.cuda.is_available(), 'the opens are compared on a GPU only'
    modes = {'device': 'cuda:0', 'host': None}

    def one_open(device):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds = PreparedDataset(a.dir, device=device, prepare_frames=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, len(ds)

    n = 0
    for device in modes.values():
        n = one_open(device)[1]
    reps = {k: [] for k in modes}
    for _ in range(a.repeats):
        for name, device in modes.items():
            reps[name].append(one_open(device)[0])
    return {'open_what': f'PreparedDataset(prepare_frames=True) on {n} distorted frames of {IMG} x {IMG}, host clock over the '
                         f'whole open; {a.repeats} alternating repeats after one warm-up open each.  The device open also '
                         'uploads the prepared frames, the host open keeps them on the host',
            'open_device_s': _spread(reps['device'], 3), 'open_host_s': _spread(reps['host'], 3)}


def cmd_merge(a):
    res = {}
    for p in a.parts:
        with open(p) as f:
            res.update(json.load(f))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    for name in ('dataset', 'kernel', 'open'):
        p = sub.add_parser(name)
        p.add_argument('--dir', required=True)
        p.add_argument('--out')
        p.add_argument('--frames', type=int, default=8)
        p.add_argument('--repeats', type=int, default=3 if name == 'open' else 7)
        p.add_argument('--iters', type=int, default=50)
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
