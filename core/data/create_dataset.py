"""create_dataloader(data_type): the reference's data entry point (core/data/create_dataset.py:59-74).

Two sources.  The synthetic subject (occnerf_amd/synth.py, the default: `dataset: 'synthetic'`, no `train.dataset_path`):
the tpose / freeview / movement / allview / progress frame generators, same per-frame dict and shapes as the reference's,
yielded with the leading batch dimension a torch DataLoader with batch_size=1 would add (run.py strips it, run.py:85-86).

A prepared dataset directory in the reference's on-disk layout (occnerf_amd/dataset.py; the ZJU-MoCap / OcMotion pickles
and the SMPL model are not redistributable, tools/make_synthetic_dataset.py writes a stand-in): named by
`train.dataset_path`, or by the reference's dataset names in `<type>.dataset` as dataset_args.py resolves them
(zju_<subject>_train -> dataset/zju_mocap/<subject>, monocular_train -> dataset/wild/<cfg.subject>).
  * 'train': the device-side patch batch loader (dataset.loader_from_cfg: PatchBatchLoader; bgcolor None = a random colour
    per batch, create_dataset.py:31).  Its batches are built on the GPU one step ahead of the optimiser, so next() needs one;
  * 'movement' / 'progress': whole-frame dicts (`ray_shoot_mode 'image'`) with `target_rgbs` and `ray_alpha`, under the
    skip / maxframes rules of create_dataset.py:32-42 (progress: every (total // 16)-th frame, 16 of them; under evaluate
    the first 300; movement under evaluate switches the occlusion band off).  The loader is occnerf_amd.dataset.WholeFrames:
    iterating it gives the host dicts (numpy); sequence.frames_to_device -- run.py, eval.py -- asks it for `device_frames`
    instead, which builds each frame on the GPU (csrc/frame.hip) one frame ahead of the render (occnerf_amd/ahead.py, the
    one frame-ahead scheme of all three loaders);
  * 'freeview' / 'backview' / 'allview' / 'tpose': the cameras derived from a dataset frame (occnerf_amd.views.ViewFrames,
    the reference's freeview.py / backview.py / allview.py / tpose.py).  Host dicts when iterated; `device_frames` builds
    the rays on the GPU (csrc/view.hip), one frame ahead in the same way.  backview reads the directory movement would;
    allview also needs all_cameras.pkl;
  * 'animate': the subject of the directory movement would read, driven by the motion `animate.motion` names
    (occnerf_amd.animate.AnimateFrames; the reference has no such type).  A prepared dataset only."""
import os

import torch

from configs import cfg
from occnerf_amd.animate import AnimateFrames
from occnerf_amd.dataset import PreparedDataset, WholeFrames, loader_from_cfg, resolve_dataset_path
from occnerf_amd.sequence import SyntheticFrames
from occnerf_amd.views import KINDS as VIEW_KINDS, ViewFrames


def _prepared(data_type, evaluate, path):
    if not os.path.isdir(path):
        raise FileNotFoundError(f"dataset directory '{path}' ({data_type}) does not exist")
    device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None
    if data_type == 'train':
        return loader_from_cfg(cfg, path, device=device, seed=int(dict(cfg.get('train', {})).get('seed', 0)),
                               prefetch=bool(dict(cfg.get('train', {})).get('prefetch', True)))
    if data_type in VIEW_KINDS:
        return ViewFrames.from_cfg(cfg, path, data_type, prepare_device=device)
    if data_type == 'animate':
        return AnimateFrames.from_cfg(cfg, path, prepare_device=device)
    if data_type not in ('movement', 'progress'):
        raise NotImplementedError(f"type '{data_type}' on the prepared dataset '{path}': train, movement, progress, "
                                  'freeview, backview, allview, tpose and animate read a dataset')
    skip, maxframes = 1, -1
    if data_type == 'progress':
        total = len([f for f in os.listdir(os.path.join(path, 'images')) if f.endswith('.png')])
        skip, maxframes = (1, 300) if evaluate else (max(total // 16, 1), 16)
    if data_type == 'movement' and evaluate:
        cfg.occlude = False
    return WholeFrames(PreparedDataset.from_cfg(cfg, path, device=None, skip=skip, maxframes=maxframes, prepare_device=device),
                       cfg.bgcolor)


def create_dataloader(data_type='train', evaluate=False, **_):
    # backview has no dataset node of its own in the reference's configs: it reads the directory movement would; so does animate
    path = resolve_dataset_path(cfg, 'movement' if data_type in ('backview', 'animate') else data_type)
    if path is not None:
        return _prepared(data_type, evaluate, path)
    if data_type == 'animate':
        raise NotImplementedError('--type animate drives the subject of a prepared dataset; the synthetic frame source has '
                                  'none (set train.dataset_path or movement.dataset)')
    if cfg.get('dataset', 'synthetic') != 'synthetic' or \
            data_type not in ('tpose', 'freeview', 'movement', 'allview', 'progress'):
        raise NotImplementedError(
            f"dataset '{cfg.get('dataset')}' / type '{data_type}': without a prepared dataset directory (train.dataset_path) "
            'only the synthetic tpose / freeview / movement / allview / progress frame generators are available')
    return SyntheticFrames(data_type, img_size=int(cfg.get('render_size', 512)), render_frames=int(cfg.render_frames),
                           bgcolor=cfg.bgcolor, device_rays=bool(cfg.get('device_rays', True)),
                           freeview_frame_idx=int(cfg.freeview.get('frame_idx', 0)))
