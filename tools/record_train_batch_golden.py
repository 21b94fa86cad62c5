"""Record tests/golden/train_batch_ref.npz from the UNMODIFIED reference Dataset (core/data/occnerf/train.py) in patch mode,
on the CPU, where the reference tree is present:

    python tools/record_train_batch_golden.py

The reference is imported under oracle.ref_harness.shims.install; what that leaves open is added here: a
`torchvision.transforms` stand-in (train.py:25 imports it; the transforms are only constructed), and `np.bool`, which
train.py:176 uses and this numpy no longer has.  cv2.resize / cv2.undistort are not reached at resize_img_scale 1 without
distortions.  The dataset is written by tools/make_synthetic_dataset.py into a temporary directory.  np.random is seeded,
and np.random.rand / np.random.choice are wrapped so that each patch's class and select_idx are stored next to the outputs.

Only arrays and names are stored: the tool's arguments, the configuration, the recorded draws and every key of
__getitem__ that the build produces ('verts' needs an SMPL model and is left out)."""
import importlib.util
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from oracle.ref_harness import shims  # noqa: E402

OUT_DIR = os.environ.get('OCCNERF_GOLDEN_DIR') or os.path.join(REPO, 'tests', 'golden')

TOOL_ARGS = {'frames': 3, 'width': 96, 'height': 80, 'seed': 3, 'focal': 900.0}
CONFIG = {'N_patches': 4, 'size': 16, 'sample_subject_ratio': 0.8, 'occlude': True,
          'occlusion': {'range': 1, 'mid': 48, 'width': 20}, 'bbox_offset': 0.3, 'resize_img_scale': 1.0, 'volume_size': 8}
KEYFILTER = ['rays', 'target_rgbs', 'motion_bases', 'motion_weights_priors', 'cnl_bbox', 'dst_posevec_69']
KEYS = ['idx', 'time', 'poses', 'betas', 'Rh', 'Th', 'joints', 'ray_alpha', 'img_width', 'img_height', 'ray_mask', 'rays', 'near',
        'far', 'bgcolor', 'patch_div_indices', 'patch_masks', 'patch_mask', 'target_patches', 'target_rgbs', 'dst_Rs', 'dst_Ts',
        'cnl_gtfms', 'motion_weights_priors', 'cnl_bbox_min_xyz', 'cnl_bbox_max_xyz', 'cnl_bbox_scale_xyz', 'dst_posevec']


def _load_tool():
    spec = importlib.util.spec_from_file_location('make_synthetic_dataset', os.path.join(HERE, 'make_synthetic_dataset.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    tmp = tempfile.mkdtemp(prefix='occnerf_train_batch_')
    _load_tool().make_dataset(tmp, **TOOL_ARGS)
    occ = CONFIG['occlusion']
    cfg = shims.install(['train.py', '--cfg', 'configs/occnerf/zju_mocap/387/occnerf.yaml',
                         'resize_img_scale', str(CONFIG['resize_img_scale']), 'occlude', str(CONFIG['occlude']),
                         'occlusion.range', str(occ['range']), 'occlusion.mid', str(occ['mid']),
                         'occlusion.width', str(occ['width']), 'patch.N_patches', str(CONFIG['N_patches']),
                         'patch.size', str(CONFIG['size']), 'patch.sample_subject_ratio', str(CONFIG['sample_subject_ratio']),
                         'bbox_offset', str(CONFIG['bbox_offset']), 'mweight_volume.volume_size', str(CONFIG['volume_size']),
                         'include_img', 'False'])                      # :400-404: the normalised whole image, not built
    assert not (hasattr(cfg, 'crop_image_scale') and cfg.crop_image_scale[0] != -1) and not cfg.upsample_pc
    tv = sys.modules['torchvision']
    keep = lambda *a, **k: None                                        # noqa: E731
    tv.transforms = shims._mod('torchvision.transforms', Compose=keep, ToTensor=keep, Normalize=keep)
    if not hasattr(np, 'bool'):
        np.bool = bool
    from core.data.occnerf.train import Dataset                        # the reference's

    draws = {}
    real_rand, real_choice = np.random.rand, np.random.choice

    def rand(*shape):
        v = real_rand(*shape)
        if shape == (1,):                                              # train.py:195: the class draw
            draws['cls'].append(0 if v[0] < cfg.patch.sample_subject_ratio else 1)
        return v

    def choice(*a, **k):
        v = real_choice(*a, **k)
        draws['select_idx'].append(int(v[0]))                          # train.py:239
        draws['count'].append(int(a[0]))
        return v

    np.random.rand, np.random.choice = rand, choice
    try:
        ds = Dataset(tmp, keyfilter=KEYFILTER, bgcolor=None, ray_shoot_mode='patch')
        out = {'meta.tool_args': np.array([TOOL_ARGS[k] for k in ('frames', 'width', 'height', 'seed', 'focal')], np.float64),
               'meta.patch': np.array([CONFIG['N_patches'], CONFIG['size']], np.int64),
               'meta.sample_subject_ratio': np.float64(CONFIG['sample_subject_ratio']),
               'meta.occlusion': np.array([int(CONFIG['occlude']), occ['range'], occ['mid'], occ['width']], np.int64),
               'meta.bbox_offset': np.float64(CONFIG['bbox_offset']), 'meta.volume_size': np.int64(CONFIG['volume_size']),
               'meta.framelist': np.array(ds.framelist)}
        np.random.seed(7)
        for idx in range(len(ds)):
            draws.update(cls=[], select_idx=[], count=[])
            r = ds[idx]
            assert r['frame_name'] == ds.framelist[idx], 'the reference substituted another frame (empty mask)'
            for k in KEYS:
                out[f'f{idx}.{k}'] = np.asarray(r[k])
            for k in ('cls', 'select_idx', 'count'):
                out[f'f{idx}.draw.{k}'] = np.array(draws[k], np.int64)
            assert len(draws['cls']) == len(draws['select_idx']) == CONFIG['N_patches']
    finally:
        np.random.rand, np.random.choice = real_rand, real_choice
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, 'train_batch_ref.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
