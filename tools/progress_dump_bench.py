"""Measures the trainer's progress dump (occnerf_amd/progress.py, csrc/progress.hip) at the size a user runs: 16 tool-made
frames of 512 x 512, 128 samples per ray.

    bash tools/progress_dump_bench.sh          # every step under its own time limit -> profiles/progress_dump_bench.json

Steps (each a sub-command, so the shell script can bound each one):
  dataset   tools/make_synthetic_dataset.py writes the frames (CPU);
  dump      one dump of the 16 frames, host clock from the call to the mosaic on the host: (a) ProgressDump.run, the device
            path; (b) a host restatement of the reference's loop (trainer.py:337-383): per frame a blocking copy of the rays'
            colours, numpy scatter of rendered and truth, to_8b_image, allclose, then tile_images.  Both render the same
            frames through the same network; they alternate inside one process after a warm-up each, `--repeats` times.  The
            image steps alone (everything but the render) are timed too: 16 launches of progress_tile + the one copy from
            device events and the host clock, against the numpy work of (b) on colours already on the host;
  steps     steps/s of `--steps` bf16 training steps (MSE + comp, the loader's batches) with progress.dump_interval 50 and
            with 0, alternating, `--repeats` times, each run on a fresh trainer;
  merge     the partial results as one JSON object."""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
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


def _cfg():
    from occnerf_amd import config
    cfg = config.default_cfg()
    config._finish(cfg)
    cfg.smpl_model, cfg.bgcolor, cfg.perturb = 'synthetic', list(BGCOLOR), 1.0
    return config.set_cfg(cfg)


def _network(ds, dev):
    from occnerf_amd.checkpoint import make_state_dict
    from occnerf_amd.network import Network
    net = Network()
    net.generate_neural_points(ds.avg_betas)
    net.load_state_dict(make_state_dict(net.point_base.detach().numpy(), float(net.bound), seed=0, amplify=True), strict=True)
    return net.to(dev).train()


def _progress_loader(a):
    from occnerf_amd.dataset import PreparedDataset, WholeFrames
    return WholeFrames(PreparedDataset(a.dir, device=None), BGCOLOR)


def to_8b_image(image):
    return (255. * np.clip(image, 0., 1.)).astype(np.uint8)


def tile_images(images, per_row=4):
    per_row = min(len(images), per_row)
    return np.concatenate([np.concatenate(images[r * per_row:(r + 1) * per_row], axis=1)
                           for r in range(len(images) // per_row)], axis=0)


def host_panels(rgb, target, ray_index, H, W):
    """trainer.py:350-378 on host arrays -> (the panel pair, is_empty)."""
    rendered = np.full((H * W, 3), np.array(BGCOLOR) / 255., dtype='float32')
    truth = np.full((H * W, 3), np.array(BGCOLOR) / 255., dtype='float32')
    rendered[ray_index] = rgb
    truth[ray_index] = target
    truth = to_8b_image(truth.reshape((H, W, -1)))
    rendered = to_8b_image(rendered.reshape((H, W, -1)))
    return np.concatenate([rendered, truth], axis=1), bool(np.allclose(rendered, np.array(BGCOLOR), atol=3.))


def host_dump(net, loader, it, dev):
    """The reference's loop: eval mode, per frame render -> blocking copy -> numpy; tile at the end."""
    import torch
    from occnerf_amd.dataset import NETWORK_KEYS
    from occnerf_amd.sequence import frames_to_device
    cfg, images = net.cfg, []
    net.eval()
    perturb, cfg.perturb = cfg.perturb, 0.
    try:
        with torch.no_grad():
            for data, _key, meta in frames_to_device(loader, 'progress', dev):
                out = net(**{k: data[k] for k in NETWORK_KEYS}, iter_val=it)
                panel, _empty = host_panels(out['rgb'].cpu().numpy(), meta['target_rgbs'].cpu().numpy(),
                                            meta['ray_index'].cpu().numpy(), meta['height'], meta['width'])
                images.append(panel)
    finally:
        net.train()
        cfg.perturb = perturb
    return tile_images(images)


def cmd_dump(a):
    with tempfile.TemporaryDirectory(prefix='occnerf_progress_bench_') as logdir:      # prog_*.jpg, progress.jsonl: not kept
        return _dump(a, logdir)


def _dump(a, logdir):
    import torch
    from occnerf_amd import _lib, progress
    assert torch.cuda.is_available(), 'the dump is timed on a GPU only'
    dev = torch.device('cuda', 0)
    _cfg()
    loader = _progress_loader(a)
    net = _network(loader.dataset, dev)
    dump = progress.ProgressDump(loader, logdir, device=dev)

    def device_path():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = dump.run(net, net, 10 ** 6)
        t = time.perf_counter() - t0
        dump.close()                                                    # the JPEG is encoded outside the timed part
        return t * 1e3, got['mosaic'].copy()

    def host_path():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = host_dump(net, loader, 10 ** 6, dev)
        return (time.perf_counter() - t0) * 1e3, img

    _, dev_img = device_path()
    _, host_img = host_path()
    times = {'device': [], 'host': []}
    for _ in range(a.repeats):
        times['device'].append(device_path()[0])
        times['host'].append(host_path()[0])

    # the image steps alone, on one frame's colours: n launches of progress_tile + the copy / the numpy work
    n, H, W = len(loader), loader.dataset.height, loader.dataset.width
    frames = []
    with torch.no_grad():
        from occnerf_amd.sequence import frames_to_device
        for data, _key, meta in frames_to_device(loader, 'progress', dev):
            frames.append((torch.rand(meta['ray_index'].numel(), 3, device=dev), meta['ray_index'], meta['truth_u8'],
                           meta['target_rgbs']))
    rows, cols = progress.mosaic_shape(n)
    mosaic = torch.empty(rows * H, cols * 2 * W, 3, device=dev, dtype=torch.uint8)
    host = torch.empty(mosaic.shape, dtype=torch.uint8).pin_memory()
    partial = torch.empty(int(_lib.lib().occnerf_progress_tile_blocks(H, W)), device=dev, dtype=torch.int32)
    counts = torch.empty(n, device=dev, dtype=torch.int32)
    bg255 = np.array(BGCOLOR)
    bg01 = (bg255 / 255.).astype(np.float32)

    def tiles():
        for i, (rgb, idx, truth, _t) in enumerate(frames[:rows * cols]):
            progress.progress_tile(rgb, idx, H, W, bg01, bg255, truth, mosaic, i % cols, i // cols, partial, counts[i:i + 1])

    tiles()
    torch.cuda.synchronize()
    ev_us, wall_ms, numpy_ms = [], [], []
    host_frames = [(rgb.cpu().numpy(), t.cpu().numpy(), idx.cpu().numpy()) for rgb, idx, _truth, t in frames]
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        tiles()
        e1.record()
        host.copy_(mosaic, non_blocking=True)
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        ev_us.append(e0.elapsed_time(e1) * 1e3 / (rows * cols))
        t0 = time.perf_counter()
        tile_images([host_panels(r, t, i, H, W)[0] for r, t, i in host_frames])
        numpy_ms.append((time.perf_counter() - t0) * 1e3)

    def stat(v, digits=2):
        return round(float(np.median(v)), digits), [round(float(x), digits) for x in v]

    res = {'dump_what': f'one dump of {n} frames of {W} x {H}, 128 samples per ray, seeded amplified checkpoint: host clock from '
                        f'the call until the mosaic is on the host (JPEG encoding excluded); {a.repeats} alternating repeats '
                        'after one warm-up each',
           'dump_mosaics_equal': bool(np.array_equal(dev_img, host_img))}
    res['dump_device_ms'], res['dump_device_repeats_ms'] = stat(times['device'])
    res['dump_host_ms'], res['dump_host_repeats_ms'] = stat(times['host'])
    res['dump_host_spread_ms'] = round(max(times['host']) - min(times['host']), 2)
    res['tile_us_per_frame_events'], res['tile_us_per_frame_repeats'] = stat(ev_us)
    res['image_steps_device_ms'], res['image_steps_device_repeats_ms'] = stat(wall_ms, 3)
    res['image_steps_numpy_ms'], res['image_steps_numpy_repeats_ms'] = stat(numpy_ms, 3)
    res['image_steps_what'] = (f'everything but the render, {rows * cols} frames: progress_tile launches (device events, per '
                               'frame) and launches + the one copy of the mosaic (host clock), against the numpy scatter, '
                               'quantisation, allclose and tiling on colours that are already on the host')
    return res


def cmd_steps(a):
    import torch
    from occnerf_amd import trainer as tr
    from occnerf_amd.dataset import PatchBatchLoader, PreparedDataset
    from occnerf_amd.progress import ProgressDump, dump_due
    assert torch.cuda.is_available(), 'the steps are timed on a GPU only'
    dev = torch.device('cuda', 0)
    cfg = _cfg()
    ds = PreparedDataset(a.dir, device=dev)
    prog_loader = _progress_loader(a)

    def run(interval):
        with tempfile.TemporaryDirectory(prefix='occnerf_progress_bench_') as logdir:  # init.tar, its sidecar, prog_*.jpg
            rate = timed(interval, logdir)
        print(f'dump_interval {interval}: {rate:.2f} steps/s', file=sys.stderr, flush=True)
        return rate

    def timed(interval, logdir):
        loader = PatchBatchLoader(ds, n_patches=int(cfg.patch.N_patches), size=int(cfg.patch.size), bgcolor=None, seed=0)
        net = _network(ds, dev)
        tc = dict(tr.TRAIN_DEFAULTS, bf16=True, log_interval=10 ** 9, save_checkpt_interval=10 ** 9)
        progress = ProgressDump(prog_loader, logdir, device=dev) if interval else None
        t = tr.Trainer(net, tr.make_optimizer(net, tc), tc, logdir, lambda it: next(loader),
                       lambda b, it: tr.dataset_step_loss(net, b, it, tc), loader=loader, progress=progress,
                       dump_interval=interval, out=lambda line: None)
        first = t.start()
        for it in range(first, first + a.warmup):                       # graphs captured, caches filled: not timed
            t.step(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(first + a.warmup, first + a.warmup + a.steps):
            t.step(it)
            if progress is not None and dump_due(it - a.warmup, interval):
                progress.run(net, net, it)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if progress is not None:
            progress.close()
        return a.steps / dt

    rates = {50: [], 0: []}
    for _ in range(a.repeats):
        for interval in (50, 0):
            rates[interval].append(run(interval))
    dumps = len([i for i in range(1, a.steps + 1) if dump_due(i, 50)])
    with_d, without = float(np.median(rates[50])), float(np.median(rates[0]))
    return {'steps_what': f'{a.steps} bf16 steps (MSE + comp, loader batches, 6 patches of 32 x 32, 128 samples per ray) after '
                          f'{a.warmup} untimed ones, a fresh trainer per run, {a.repeats} alternating repeats; with '
                          f'progress.dump_interval 50 the run holds {dumps} dumps of {len(prog_loader)} frames of {IMG} x {IMG}',
            'steps_per_s_dump_interval_50': round(with_d, 2), 'steps_per_s_dump_interval_50_repeats': [round(x, 2) for x in rates[50]],
            'steps_per_s_dump_interval_0': round(without, 2), 'steps_per_s_dump_interval_0_repeats': [round(x, 2) for x in rates[0]],
            'steps_per_s_spread_without_dumps': round(max(rates[0]) - min(rates[0]), 2),
            'seconds_per_dump_from_the_difference': round((a.steps / with_d - a.steps / without) / max(dumps, 1), 3)}


def cmd_merge(a):
    res = {}
    for p in a.parts:
        with open(p) as f:
            res.update(json.load(f))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    for name in ('dataset', 'dump', 'steps'):
        p = sub.add_parser(name)
        p.add_argument('--dir', required=True)
        p.add_argument('--out')
        p.add_argument('--frames', type=int, default=16)
        p.add_argument('--repeats', type=int, default=3)
        p.add_argument('--steps', type=int, default=200)
        p.add_argument('--warmup', type=int, default=10)
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
