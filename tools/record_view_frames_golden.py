"""Record tests/golden/view_frames_ref.npz from the UNMODIFIED reference datasets of the derived cameras
(core/data/occnerf/freeview.py, backview.py, allview.py, tpose.py), on the CPU, where the reference tree is present:

    python tools/record_view_frames_golden.py

The reference is imported under oracle.ref_harness.shims.install; what that leaves open is added here: `np.bool`, which the
reference's camera_util uses and this numpy no longer has, and a `cv2.Rodrigues` that also turns a 3x3 rotation into its
axis-angle vector (tpose.py:150 feeds it the root rotation).  cv2.resize / cv2.undistort are not reached at
resize_img_scale 1 without distortions.  The dataset is written by tools/make_synthetic_dataset.py into a temporary
directory (with all_cameras.pkl; a second copy under a path holding 'wild' is not needed: 23 cameras are recorded).

Only arrays and names are stored: the tool's arguments, the configuration and, per recorded frame, every key of
__getitem__ (the photograph `target_rgbs` as the reference's own 8-bit truth panel, image_util.to_8b_image).  The tpose
frame is 512 x 512 (the reference's RENDER_SIZE): its ray_mask is stored as packed bits with the ray count, and every 64th
row of rays / near / far."""
import importlib.util
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from occnerf_amd import synth  # noqa: E402
from oracle.ref_harness import shims  # noqa: E402

OUT_DIR = os.environ.get('OCCNERF_GOLDEN_DIR') or os.path.join(REPO, 'tests', 'golden')

TOOL_ARGS = {'frames': 4, 'width': 48, 'height': 40, 'seed': 3, 'focal': 900.0, 'all_cameras': 23}
CONFIG = {'render_frames': 6, 'frame_idx': 1, 'bbox_offset': 0.3, 'resize_img_scale': 1.0, 'volume_size': 8}
PLAN = [('freeview_zju', 'freeview', 'zju_mocap', [0, 1, 4]), ('freeview_wild', 'freeview', 'wild', [1, 4]),
        ('backview', 'backview', 'zju_mocap', [0, 1, 3]), ('allview', 'allview', 'zju_mocap', [0, 7, 22]),
        ('tpose', 'tpose', 'zju_mocap', [0])]
KEYFILTER = ['rays', 'target_rgbs', 'motion_bases', 'motion_weights_priors', 'cnl_bbox', 'dst_posevec_69']
KEYS = ['ray_mask', 'rays', 'near', 'far', 'bgcolor', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'cnl_bbox_min_xyz', 'cnl_bbox_max_xyz',
        'cnl_bbox_scale_xyz', 'dst_posevec']
TPOSE_ROW_STRIDE = 64


def _load_tool():
    spec = importlib.util.spec_from_file_location('make_synthetic_dataset', os.path.join(HERE, 'make_synthetic_dataset.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rodrigues(v):
    """cv2.Rodrigues for both directions: a 3-vector -> (3x3, None) as the shim's; a 3x3 rotation -> (3x1 axis-angle, None)."""
    v = np.asarray(v)
    if v.size == 3:
        return synth.rodrigues_exact(v.ravel()), None
    R = v.reshape(3, 3).astype(np.float64)
    theta = np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    r = np.zeros(3) if theta < 1e-12 else axis * (theta / (2.0 * np.sin(theta)))
    return r.reshape(3, 1), None


def main():
    tmp = tempfile.mkdtemp(prefix='occnerf_view_frames_')
    _load_tool().make_dataset(tmp, **TOOL_ARGS)
    cfg = shims.install(['run.py', '--cfg', 'configs/occnerf/zju_mocap/387/occnerf.yaml',
                         'resize_img_scale', str(CONFIG['resize_img_scale']), 'render_frames', str(CONFIG['render_frames']),
                         'freeview.frame_idx', str(CONFIG['frame_idx']), 'bbox_offset', str(CONFIG['bbox_offset']),
                         'mweight_volume.volume_size', str(CONFIG['volume_size'])])
    sys.modules['cv2'].Rodrigues = rodrigues
    if not hasattr(np, 'bool'):
        np.bool = bool
    from core.data.occnerf import allview, backview, freeview, tpose          # the reference's
    from core.utils.image_util import to_8b_image
    modules = {'freeview': freeview, 'backview': backview, 'allview': allview, 'tpose': tpose}
    assert tpose.Dataset.RENDER_SIZE == 512

    out = {'meta.tool_args': np.array([TOOL_ARGS[k] for k in ('frames', 'width', 'height', 'seed', 'focal', 'all_cameras')],
                                      np.float64),
           'meta.config': np.array([CONFIG[k] for k in ('render_frames', 'frame_idx', 'bbox_offset', 'resize_img_scale',
                                                        'volume_size')], np.float64),
           'meta.tpose_row_stride': np.int64(TPOSE_ROW_STRIDE),
           'meta.plan': np.array([f'{tag}:{kind}:{src}:' + ','.join(map(str, frames)) for tag, kind, src, frames in PLAN])}
    try:
        for tag, kind, src_type, frames in PLAN:
            ds = modules[kind].Dataset(tmp, keyfilter=KEYFILTER, bgcolor=[255., 255., 255.], src_type=src_type)
            out[f'{tag}.len'] = np.int64(len(ds))
            # the reference's DataLoader walks the frames in order; backview fixes its camera at the first one it is asked for
            got = {i: ds[i] for i in range(max(frames) + 1)} if kind == 'backview' else {i: ds[i] for i in frames}
            out[f'{tag}.motion_weights_priors'] = np.asarray(got[frames[0]]['motion_weights_priors'])
            for i in frames:
                r = got[i]
                assert np.array_equal(r['motion_weights_priors'], out[f'{tag}.motion_weights_priors'])
                for k in KEYS:
                    out[f'{tag}.f{i}.{k}'] = np.asarray(r[k])
                out[f'{tag}.f{i}.size'] = np.array([r['img_width'], r['img_height']], np.int64)
                if kind == 'tpose':
                    rows = slice(None, None, TPOSE_ROW_STRIDE)
                    out[f'{tag}.f{i}.ray_count'] = np.int64(r['ray_mask'].sum())
                    out[f'{tag}.f{i}.ray_mask'] = np.packbits(r['ray_mask'])
                    out[f'{tag}.f{i}.rays'] = np.asarray(r['rays'])[:, rows]
                    out[f'{tag}.f{i}.near'], out[f'{tag}.f{i}.far'] = r['near'][rows], r['far'][rows]
                else:
                    out[f'{tag}.f{i}.frame_name'] = np.array(r['frame_name'])
                    out[f'{tag}.f{i}.truth_u8'] = to_8b_image(r['target_rgbs'])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, 'view_frames_ref.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
