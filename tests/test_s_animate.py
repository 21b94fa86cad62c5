"""GPU: the skeleton panel kernel (occnerf_amd/csrc/skeleton.hip, ops.skeleton_panel, occnerf_amd/skeleton.py) equals its
numpy definition (tests/skeleton_restatement.py) byte for byte on the cases of tests/animate_cases.py at
four image sizes; the device frames of an animate source equal its host frames; and run.py --type animate writes the frames,
the skeleton panel and animate.json."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import animate_cases as cases
from tests import skeleton_restatement as S
from tests.gpu_util import DEV, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml')
ALL_CASES = cases.all_cases()


@pytest.mark.parametrize('size', cases.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('name', sorted(ALL_CASES))
def test_kernel_equals_the_definition(name, size):
    """The panel's bytes and its count record; a second run gives the same bytes."""
    from occnerf_amd import ops
    from occnerf_amd.skeleton import counts
    case, (w, h) = ALL_CASES[name], size
    args = cases.definition_args(case, w, h)
    want = S.skeleton_panel(**args)
    img, record = ops.skeleton_panel(device=DEV, **args)
    again, record2 = ops.skeleton_panel(device=DEV, **args)
    torch.cuda.synchronize()
    assert img.dtype == torch.uint8 and tuple(img.shape) == (h, w, 3)
    same(img.cpu().numpy(), want['img'], f'{name} {w} x {h}: panel')
    same(again.cpu().numpy(), img.cpu().numpy(), f'{name} {w} x {h}: second run')
    assert counts(record) == counts(record2) == {'dropped': want['dropped'], 'covered': want['covered']}
    assert want['dropped'] == case['dropped']
    assert record.numel() == 1 + (w * h + 255) // 256


def test_the_public_wrapper_and_the_refusals():
    from occnerf_amd import _lib, ops
    from occnerf_amd.skeleton import PALETTE, background_u8, counts, skeleton_panel
    case = cases.generic_case()
    bg = [10., 200., 255.]
    want = S.skeleton_panel(**{**cases.definition_args(case), 'bone_px': 2.0, 'bgcolor_u8': background_u8(bg)})
    img, record = skeleton_panel(case['joints'], case['K'], case['E'], cases.H, cases.W, DEV, bone_px=2.0, bgcolor=bg)
    torch.cuda.synchronize()
    same(img.cpu().numpy(), want['img'], 'another width and background')
    assert counts(record) == {'dropped': 0, 'covered': want['covered']} and (want['img'][0, 0] == [10, 200, 255]).all()
    a = {**cases.definition_args(case), 'device': DEV}
    with pytest.raises(NotImplementedError, match='skew'):
        ops.skeleton_panel(**{**a, 'K': np.array([[100., 1., 48.], [0., 100., 40.], [0., 0., 1.]])})
    with pytest.raises(RuntimeError, match=r'joints must be float32 \[24,3\]'):
        ops.skeleton_panel(**{**a, 'joints': case['joints'][:23]})
    with pytest.raises(RuntimeError, match='must be positive'):
        ops.skeleton_panel(**{**a, 'height': 0})
    with pytest.raises(RuntimeError, match='bone_px'):
        ops.skeleton_panel(**{**a, 'bone_px': float('nan')})
    with pytest.raises(RuntimeError, match='palette must be uint8'):
        ops.skeleton_panel(**{**a, 'palette': PALETTE.astype(np.int32)})
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.skeleton_panel(**{**a, 'device': 'cpu'})
    # the C entry refuses on its own, before any launch
    lib = _lib.lib()
    j, K, E = case['joints'], np.ascontiguousarray(case['K']), np.ascontiguousarray(case['E'])
    pal, bg8 = np.ascontiguousarray(PALETTE), background_u8(bg)
    p = [j.ctypes.data, K.ctypes.data, E.ctypes.data, 3.0, pal.ctypes.data, bg8.ctypes.data, cases.H, cases.W, img.data_ptr(),
         record.data_ptr(), None]
    for i, v, word in ((6, 0, b'bad sizes'), (7, -3, b'bad sizes'), (8, None, b'null argument'), (0, None, b'null argument'),
                       (3, -1.0, b'bone_px')):
        args = list(p)
        args[i] = v
        assert lib.occnerf_skeleton_panel(*args) != 0 and word in lib.occnerf_last_error(), (i, lib.occnerf_last_error())
    assert lib.occnerf_skeleton_panel_blocks(cases.H, cases.W) == 30 and lib.occnerf_skeleton_panel_blocks(0, 5) == 0
    torch.cuda.synchronize()


@pytest.fixture(scope='module')
def paths(tmp_path_factory):
    return cases.make_datasets(tmp_path_factory.mktemp('animate_gpu'), frames=3)


def test_device_frames_equal_the_host_frames(paths):
    """Rays, near, far, ray index and constants at 96 x 80, with and without prefetch: the cameras are float64, so gen_rays
    performs numpy's operations in numpy's order (tests/test_i_view_frames.py) and every entry is equal."""
    from occnerf_amd import animate as A
    from occnerf_amd.dataset import PreparedDataset
    ds = PreparedDataset(paths[0], device=None, volume_size=4)
    frames = A.AnimateFrames(ds, A.read_motion(paths[1]), substeps=2, camera='follow')
    host = [frames.frame(i) for i in range(len(frames))]
    assert len(host) == 5
    for prefetch in (True, False):
        n = 0
        for data, key, meta in frames.device_frames(DEV, prefetch=prefetch):
            torch.cuda.synchronize()
            want, i = host[meta['idx']], meta['idx']
            assert key is None and i == n and meta['frame_name'] == want['frame_name'] and 'truth_u8' not in meta
            assert (meta['width'], meta['height']) == (96, 80)
            same(meta['ray_index'].cpu().numpy(), np.nonzero(want['ray_mask'])[0], f'{i}: ray_index')
            for k in ('rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'dst_posevec', 'cnl_gtfms', 'motion_weights_priors',
                      'cnl_bbox_min_xyz', 'cnl_bbox_max_xyz', 'cnl_bbox_scale_xyz', 'bgcolor'):
                got = data[k].cpu().numpy() if torch.is_tensor(data[k]) else np.asarray(data[k])
                assert got.dtype == np.asarray(want[k]).dtype, (k, got.dtype)
                same(got, want[k], f'prefetch {prefetch} frame {i}: {k}')
            same(meta['joints'], frames.view(i)['joints'], f'{i}: joints')
            same(meta['K'], want['camera_K'], f'{i}: K')
            same(meta['E'], want['camera_E'], f'{i}: E')
            n += 1
        assert n == 5


def test_run_py_animate(tmp_path):
    """python run.py --type animate: a 2-frame 96 x 80 dataset as its own motion, substeps 2, show_skeleton and show_alpha ->
    3 PNGs of [rgb, skeleton, alpha], the middle panel the definition for that frame's joints and camera, and animate.json."""
    from PIL import Image
    from occnerf_amd import animate as A
    from occnerf_amd.dataset import PreparedDataset
    from occnerf_amd.skeleton import PALETTE, background_u8
    path = str(tmp_path / 'data')
    cases.load_tool().make_dataset(path, frames=2, width=96, height=80, seed=0, focal=900.0)
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', CFG, '--type', 'animate', 'train.dataset_path', path,
           'resize_img_scale', '1.0', 'N_samples', '32', 'load_net', 'seeded', 'animate.motion', path, 'animate.substeps', '2',
           'show_skeleton', 'True', 'show_alpha', 'True']
    out = subprocess.run(cmd, cwd=str(tmp_path), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True,
                         timeout=170)
    assert out.returncode == 0, out.stderr[-3000:]
    base = tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded'
    assert sorted(os.listdir(base)) == ['animate', 'animate.json']
    assert sorted(os.listdir(base / 'animate')) == ['000000.png', '000001.png', '000002.png']
    frames = A.AnimateFrames(PreparedDataset(path, device=None, volume_size=4), A.read_motion(path), substeps=2)
    log = json.load(open(base / 'animate.json'))
    assert (log['motion'], log['motion_frames'], log['frames'], log['substeps'], log['align'], log['camera'], log['source_frame']) \
        == (os.path.abspath(path), 2, 3, 2, True, 'fixed', 0)
    assert [f['keyframes'] for f in log['per_frame']] == [[0, 1], [0, 1], [1, 1]] and [f['u'] for f in log['per_frame']] == [0, .5, 0]
    for i, entry in enumerate(log['per_frame']):
        panel = np.asarray(Image.open(base / 'animate' / f'{i:06d}.png'))
        assert panel.shape == (80, 3 * 96, 3)
        v = frames.view(i)
        want = S.skeleton_panel(v['joints'], v['K'], v['E'], 80, 96, 3.0, PALETTE, background_u8([255., 255., 255.]))
        same(panel[:, 96:192], want['img'], f'frame {i}: the middle panel is the definition')
        assert want['covered'] > 200 and entry['pixels_covered'] == want['covered'] and entry['joints_dropped'] == want['dropped'] == 0
        alpha = panel[:, 192:]
        assert (alpha[..., 0] == alpha[..., 1]).all() and (alpha[..., 0] == alpha[..., 2]).all()
        assert entry['idx'] == i and entry['rays'] > 100
        assert np.allclose(entry['bbox_min'], v['min']) and np.allclose(entry['bbox_max'], v['max'])
    # the type is this feature's: the message that lists the supported types names it
    src = open(os.path.join(ROOT, 'run.py')).read()
    assert 'def run_animate():' in src and 'animate' in src.split('supported are')[1].split('\n')[1]
