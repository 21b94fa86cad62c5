"""Evaluation entry point with the reference's command line and output (eval.py:1-222):

    python eval.py --cfg configs/occnerf/synthetic/occnerf.yaml [KEY VALUE ...]

Every frame of the `movement` sequence is rendered at iter_val = cfg.eval_iter with a white background.  Per frame it
prints PSNR and SSIM over the "vis", "body" and "full" pixels and the silhouette IoU in the reference's format, writes the
`rgb | truth | alpha` panel to <logdir>/<load_net>/eval/NNNNNN.png and, after the last frame, the two summary lines.
The metrics are computed on the GPU from the 8-bit images (occnerf_amd/metrics.py, csrc/metrics.hip); only the per-frame
record crosses PCIe.  <logdir>/<load_net>/eval/metrics.json holds the per-frame numbers and their means (the reference
prints them only).

The synthetic source has no photographs: the truth image and the ground-truth alpha image are the teacher's render of the
same rays (run.py `_teacher`, the targets of `run.py --type evaluate`).  Its frames carry no ray_alpha, so "vis" is the
predicted alpha > 0.001, the reference's fallback.  The reference appends each frame's IoU twice; the mean is the same as
with one entry per frame, which is what is kept here.

On a prepared dataset directory (`train.dataset_path DIR`, or a dataset name that occnerf_amd.dataset.resolve_dataset_path
resolves) no teacher is built: the truth image is the photograph blended over the background with its mask, "vis" is
ray_alpha[:, 0] > 0.5 (the reference's eval.py:163-167) and the IoU is taken against the mask's channel 0 > 0.5 (the reference
reads batch['alpha'], which its loader supplies only under include_img; here the mask is always at hand).  Each frame -- rays,
targets and the truth / vis / alpha maps -- is built on the GPU by csrc/frame.hip, one frame ahead of the render
(WholeFrames.device_frames; `device_frames False` selects the host path, numpy per frame, same numbers).  The panels are named
by the dataset's frame names, as the reference names them, and metrics.json says "source": "dataset" ("synthetic" otherwise).

`eval.lpips True` adds an LPIPS column (the reference builds its LPIPS model but never calls it): lpips_metric's
convention (8-bit images / 255, scaled to [-1, 1]) through occnerf_amd.lpips.LPIPS, with the lin layers from
eval.lpips_model_path and the VGG16 trunk from eval.lpips_vgg16_path, each a seeded stand-in when unset (labelled in the
output).

Several GPUs: start it under torchrun like run.py; every rank renders its share of each frame's rays and rank 0 computes
the metrics and writes the images.  On a dataset every rank builds the frame itself (the build is deterministic; the shard
plan's checksum guards the ray count).
"""
import json
import os
import time

import numpy as np
import torch

from configs import cfg
_EVAL_OPTS = dict(cfg.eval) if isinstance(cfg.get('eval'), dict) else {}
cfg.bgcolor = [255., 255., 255.]
cfg.eval = True

import run  # noqa: E402  (_setup, _teacher, _finish_ranks: the same model, loader and sharded renderers as run.py)
from occnerf_amd import metrics  # noqa: E402
from occnerf_amd.dataset import resolve_dataset_path  # noqa: E402
from occnerf_amd.image import ImageWriter  # noqa: E402
from occnerf_amd.sequence import frames_to_device  # noqa: E402

FRAME_LINE = ('PSNR-vis: %.4f, SSIM-vis: %.4f; PSNR-body: %.4f, SSIM-body: %.4f; PSNR-full: %.4f, SSIM-full: %.4f, '
              'IOU: %.4f')


def make_lpips(dev):
    """The optional LPIPS column's model and a label saying which weights it holds."""
    from occnerf_amd.lpips import LPIPS
    model_path, vgg16_path = _EVAL_OPTS.get('lpips_model_path'), _EVAL_OPTS.get('lpips_vgg16_path')
    m = LPIPS(pretrained=model_path is not None, net='vgg', pnet_rand=vgg16_path is None, model_path=model_path,
              vgg16_path=vgg16_path, verbose=False).to(dev).eval()
    seeded = model_path is None or vgg16_path is None
    label = 'LPIPS (seeded weights: not the published metric)' if seeded else 'LPIPS'
    return m, label


def lpips_metric(model, pred_u8, target_u8):
    """eval.py:94-101 on the device: 8-bit [H,W,3] images / 255, scaled to [-1, 1], NCHW."""
    p = pred_u8.float().div(255.).unsqueeze(0) * 2. - 1.
    t = target_u8.float().div(255.).unsqueeze(0) * 2. - 1.
    with torch.no_grad():
        val = model(p.permute(0, 3, 1, 2).contiguous(), t.permute(0, 3, 1, 2).contiguous())
    return float(torch.mean(val).item())


def eval_model(render_folder_name='eval', show_truth=True, show_alpha=True):
    cfg.perturb = 0.
    cfg.occlude = False
    rank, world, model, loader, renderer, dev = run._setup('movement', evaluate=True)
    on_dataset = resolve_dataset_path(cfg, 'movement') is not None
    teach = None if on_dataset else run._teacher(loader, dev)
    if on_dataset and rank == 0:
        print(f'targets are the dataset images (no teacher network): {len(loader)} frames')
    out_dir = os.path.join(cfg.logdir, str(cfg.load_net).replace(':', '_'))
    writer = ImageWriter(output_dir=out_dir, exp_name=render_folder_name) if rank == 0 else None
    lp, lp_label = make_lpips(dev) if _EVAL_OPTS.get('lpips', False) and rank == 0 else (None, None)
    if lp is not None:
        print(f'lpips column: {lp_label}')
    bg = np.array(cfg.bgcolor) / 255.
    frames = []
    t0 = time.perf_counter()
    with torch.no_grad():
        for data, _key, meta in frames_to_device(loader, 'movement', dev):
            target = None if on_dataset else teach.finish(teach.submit(data, iter_val=cfg.eval_iter))
            out = renderer.finish(renderer.submit(data, iter_val=cfg.eval_iter))
            if out is None:                                     # ranks > 0: their rays went to rank 0
                continue
            W, H, ray_index = meta['width'], meta['height'], meta['ray_index']
            name = loader.dataset.frames[meta['idx']]['frame_name'] if on_dataset else None
            if 'truth_u8' in meta:                              # dataset frame built on the device: the maps are there
                m, imgs = metrics.frame_metrics_from_maps(out['rgb'], out['alpha'], ray_index, meta, W, H, bgcolor=bg,
                                                          with_images=True)
            elif on_dataset:                                    # host frames (`device_frames False`)
                gt_alpha = torch.from_numpy(loader.dataset.gt_alpha(meta['idx'])).to(dev)
                m, imgs = metrics.frame_metrics(out['rgb'], out['alpha'], ray_index, data['target_rgbs'], W, H,
                                                ray_alpha=data['ray_alpha'], gt_alpha=gt_alpha, bgcolor=bg, with_images=True)
            else:
                gt_alpha = metrics.pixel_map(ray_index, target['alpha'].reshape(-1), H, W, torch.float32)
                m, imgs = metrics.frame_metrics(out['rgb'], out['alpha'], ray_index, target['rgb'], W, H, gt_alpha=gt_alpha,
                                                bgcolor=bg, with_images=True)
            panel = [imgs['rgb']] + ([imgs['truth']] if show_truth else []) + ([imgs['alpha']] if show_alpha else [])
            _, name = writer.append_device(torch.cat(panel, dim=1), img_name=name)
            line = FRAME_LINE % tuple(m[k] for k in metrics.KEYS)
            if lp is not None:
                m['lpips'] = lpips_metric(lp, imgs['rgb'], imgs['truth'])
                line += ', LPIPS: %.4f' % m['lpips']
            print(line)
            frames.append({'frame': name, **m})
    if rank != 0:
        run._finish_ranks(rank, world)
        return
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    writer.finalize()
    keys = list(metrics.KEYS) + (['lpips'] if lp is not None else [])
    mean = {k: float(np.mean([f[k] for f in frames])) for k in keys}
    print('IOU', mean['iou'])
    print(f"PSNR_vis {mean['psnr_vis']}, SSIM_vis {mean['ssim_vis']}; PSNR_body {mean['psnr_body']}, SSIM_body "
          f"{mean['ssim_body']}; PSNR_full {mean['psnr_full']}, SSIM_full {mean['ssim_full']}")
    if lp is not None:
        print(f"LPIPS {mean['lpips']} ({lp_label})")
    summary = {'frames': frames, 'mean': mean, 'n_frames': len(frames), 'seconds': elapsed,
               'frames_per_s': len(frames) / max(elapsed, 1e-9), 'source': 'dataset' if on_dataset else 'synthetic'}
    if lp is not None:
        summary['lpips_weights'] = lp_label
    with open(os.path.join(writer.image_dir, 'metrics.json'), 'w') as f:
        json.dump(summary, f, indent=1)
    print(f'{len(frames)} frames in {elapsed:.3f} s -> {summary["frames_per_s"]:.2f} frames/s ' +
          ('(frame build, render, metrics)' if on_dataset else '(render, teacher, metrics)'))
    run._finish_ranks(rank, world)


if __name__ == '__main__':
    eval_model(render_folder_name='eval')
