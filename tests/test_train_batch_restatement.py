"""CPU: the prepared-dataset side of training.  tools/make_synthetic_dataset.py writes the reference's on-disk layout
deterministically; tests/train_batch_restatement.py equals the recording of the UNMODIFIED reference Dataset
(tests/golden/train_batch_ref.npz, tools/record_train_batch_golden.py) bit for bit; occnerf_amd.dataset.PreparedDataset's host
constants match the recording; create_dataloader hands out the loader.  The device batch is held to the restatement in
tests/test_g_train_batch.py."""
import importlib.util
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from tests import train_batch_restatement as tbr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'train_batch_ref.npz')
RECORDED_KEYS = ['idx', 'time', 'poses', 'betas', 'Rh', 'Th', 'joints', 'ray_alpha', 'img_width', 'img_height', 'ray_mask', 'rays',
                 'near', 'far', 'bgcolor', 'patch_div_indices', 'patch_masks', 'patch_mask', 'target_patches', 'target_rgbs',
                 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'cnl_bbox_min_xyz', 'cnl_bbox_max_xyz',
                 'cnl_bbox_scale_xyz', 'dst_posevec']


def load_tool():
    spec = importlib.util.spec_from_file_location('make_synthetic_dataset', os.path.join(ROOT, 'tools', 'make_synthetic_dataset.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def golden_tool_args(g):
    frames, width, height, seed, focal = g['meta.tool_args']
    return {'frames': int(frames), 'width': int(width), 'height': int(height), 'seed': int(seed), 'focal': float(focal)}


def golden_cfg(g):
    occlude, rng, mid, width = (int(v) for v in g['meta.occlusion'])
    return {'N_patches': int(g['meta.patch'][0]), 'size': int(g['meta.patch'][1]),
            'sample_subject_ratio': float(g['meta.sample_subject_ratio']), 'occlude': bool(occlude),
            'occlusion': {'range': rng, 'mid': mid, 'width': width}, 'bbox_offset': float(g['meta.bbox_offset']),
            'volume_size': int(g['meta.volume_size'])}


@pytest.fixture(scope='module')
def golden_dataset(tmp_path_factory):
    g = golden()
    path = str(tmp_path_factory.mktemp('golden_dataset'))
    load_tool().make_dataset(path, **golden_tool_args(g))
    return g, path


def _read_dir(path):
    out = {}
    for name in ('cameras.pkl', 'mesh_infos.pkl', 'canonical_joints.pkl'):
        with open(os.path.join(path, name), 'rb') as f:
            out[name] = pickle.load(f)
    for sub in ('images', 'masks'):
        for f in sorted(os.listdir(os.path.join(path, sub))):
            out[sub + '/' + f] = np.array(Image.open(os.path.join(path, sub, f)))
    return out


def test_tool_is_deterministic_and_writes_the_reference_layout(tmp_path):
    tool = load_tool()
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    names = tool.make_dataset(a, frames=2, width=48, height=40, seed=5)
    assert tool.make_dataset(b, frames=2, width=48, height=40, seed=5) == names == ['frame_000000', 'frame_000001']
    da, db = _read_dir(a), _read_dir(b)
    assert sorted(da) == sorted(db)
    for k in da:
        if k.endswith('.png'):
            assert np.array_equal(da[k], db[k]), k
        elif k == 'canonical_joints.pkl':
            assert all(np.array_equal(da[k][f], db[k][f]) and da[k][f].dtype == db[k][f].dtype for f in da[k]), k
        else:
            assert list(da[k]) == list(db[k]) == names
            for n in names:
                assert all(np.array_equal(da[k][n][f], db[k][n][f]) and da[k][n][f].dtype == db[k][n][f].dtype
                           for f in da[k][n]), (k, n)
    # the reference's key names and shapes (core/data/occnerf/train.py:97-156, :421-432)
    assert {k: v.shape for k, v in da['canonical_joints.pkl'].items()} == {'joints': (24, 3), 'avg_betas': (10,)}
    for n in names:
        cam, info = da['cameras.pkl'][n], da['mesh_infos.pkl'][n]
        assert {k: (v.shape, v.dtype) for k, v in cam.items()} == {'intrinsics': ((3, 3), np.float64),
                                                                   'extrinsics': ((4, 4), np.float64)}
        assert {k: v.shape for k, v in info.items()} == {'poses': (72,), 'betas': (10,), 'tpose_joints': (24, 3),
                                                         'joints': (24, 3), 'Rh': (3,), 'Th': (3,)}
        assert np.abs(info['Rh']).min() > 0 and np.abs(info['Th']).min() > 0        # apply_global_tfm_to_camera is exercised
        assert int(n[-6:]) == names.index(n)
        img, mask = da[f'images/{n}.png'], da[f'masks/{n}.png']
        assert img.shape == (40, 48, 3) and img.dtype == np.uint8 and mask.shape == (40, 48) and mask.dtype == np.uint8
        vals = np.unique(mask)
        assert vals.min() == 0 and vals.max() == 255 and ((vals > 0) & (vals < 255)).sum() >= 8      # fractional coverage
    # another seed is another dataset
    c = str(tmp_path / 'c')
    tool.make_dataset(c, frames=2, width=48, height=40, seed=6)
    assert not np.array_equal(_read_dir(c)['images/frame_000001.png'], da['images/frame_000001.png'])


def test_restatement_equals_the_recorded_reference_bit_for_bit(golden_dataset):
    """Both sides are numpy running the same operations: any difference is a defect in the restatement."""
    g, path = golden_dataset
    cfg = golden_cfg(g)
    rs = tbr.Restatement(path, **cfg)
    assert rs.framelist == [str(n) for n in g['meta.framelist']]
    holes = off_subject = fractional = 0
    for i in range(len(rs.framelist)):
        draws = list(zip(g[f'f{i}.draw.cls'].tolist(), g[f'f{i}.draw.select_idx'].tolist()))
        r = rs.getitem(i, g[f'f{i}.bgcolor'], draws)
        assert not r['_empty']
        for k in RECORDED_KEYS:
            want, got = g[f'f{i}.{k}'], np.asarray(r[k])
            assert got.shape == want.shape and got.dtype == want.dtype, (i, k, got.shape, got.dtype, want.shape, want.dtype)
            assert np.array_equal(got, want), (i, k)
        # the recorded class sizes are the restatement's (np.random.choice's first argument)
        counts = (int(r['_subject'].sum()), int(r['_off_subject'].sum()))
        assert [counts[c] for c, _ in draws] == g[f'f{i}.draw.count'].tolist()
        holes += int((~g[f'f{i}.patch_masks']).sum() > 0)
        off_subject += int((g[f'f{i}.draw.cls'] == 1).sum())
        a = g[f'f{i}.ray_alpha']
        fractional += int(((a > 0) & (a < 1)).sum() > 0)
    # the recording reaches the branches: a patch with holes, an off-subject draw, a fractional alpha, the band
    assert holes >= 1 and off_subject >= 1 and fractional == len(rs.framelist)
    c0, c1 = cfg['occlusion']['mid'] - cfg['occlusion']['width'] // 2, cfg['occlusion']['mid'] + cfg['occlusion']['width'] // 2
    a0, _, _, _ = rs.frame_masks(0)
    a1, _, _, _ = rs.frame_masks(1)
    assert a0[:, c0:c1].sum() == 0 and a1[:, c0:c1].sum() > 0


def test_prepared_dataset_host_constants_match_the_recording(golden_dataset):
    from occnerf_amd.dataset import PreparedDataset
    g, path = golden_dataset
    cfg = golden_cfg(g)
    ds = PreparedDataset(path, device=None, bbox_offset=cfg['bbox_offset'], volume_size=cfg['volume_size'],
                         occlude=cfg['occlude'], occlusion=cfg['occlusion'])
    assert ds.framelist == [str(n) for n in g['meta.framelist']] and ds.epoch_frames == [0, 1, 2]
    assert (ds.height, ds.width) == (int(g['f0.img_height']), int(g['f0.img_width']))
    rs = tbr.Restatement(path, **cfg)
    for i in range(len(ds)):
        c = ds.host_constants(i)
        for k in ('dst_Rs', 'dst_Ts', 'cnl_gtfms'):            # tests/test_a_rows.py holds the motion bases to 2e-6
            assert c[k].shape == g[f'f{i}.{k}'].shape and np.abs(c[k] - g[f'f{i}.{k}']).max() <= 2e-6, (i, k)
        k = 'motion_weights_priors'                            # tests/test_a_rows.py holds the weight volume to 1e-5
        assert c[k].shape == g[f'f{i}.{k}'].shape and np.abs(c[k] - g[f'f{i}.{k}']).max() <= 1e-5
        for k in ('cnl_bbox_min_xyz', 'cnl_bbox_max_xyz', 'cnl_bbox_scale_xyz', 'dst_posevec'):
            assert c[k].dtype == g[f'f{i}.{k}'].dtype and np.array_equal(c[k], g[f'f{i}.{k}']), (i, k)
        f = ds.frames[i]
        assert f['idx'] == int(g[f'f{i}.idx']) and f['time'] == float(g[f'f{i}.time'])
        assert np.array_equal(f['Rh'], g[f'f{i}.Rh']) and np.array_equal(f['Th'], g[f'f{i}.Th'])
        # the observation box and the camera are the restatement's, exactly (they feed occnerf_gen_rays)
        r = rs.getitem(i, g[f'f{i}.bgcolor'], None)
        assert np.array_equal(f['dst_bbox_min'], r['_bbox']['min_xyz']) and np.array_equal(f['dst_bbox_max'], r['_bbox']['max_xyz'])
        assert np.array_equal(f['K'], r['_K']) and np.array_equal(f['E'], r['_E']) and f['E'].dtype == np.float64
        # the resident mask is the reference's alpha * 255 with the band applied at open
        assert np.array_equal(ds.alphas[i] / 255., r['_alpha'])
        assert f['band'] == (i < cfg['occlusion']['range'])
        # the whole-frame dict (`movement` / `progress`) is the reference's image mode on the same frame
        w = ds.whole_frame(i, g[f'f{i}.bgcolor'])
        assert np.array_equal(w['ray_mask'], g[f'f{i}.ray_mask']) and np.array_equal(w['ray_alpha'], g[f'f{i}.ray_alpha'])
        sel = g[f'f{i}.patch_mask']
        assert np.array_equal(w['target_rgbs'][sel], g[f'f{i}.target_rgbs'])
        assert np.array_equal(w['rays'][:, sel], g[f'f{i}.rays'].astype('float32')) and np.array_equal(w['near'][sel], g[f'f{i}.near'])


def test_prepared_dataset_frame_rules_and_refusals(tmp_path):
    from occnerf_amd.dataset import PreparedDataset
    path = str(tmp_path / 'd')
    load_tool().make_dataset(path, frames=5, width=48, height=40, seed=1)
    assert PreparedDataset(path, device=None, skip=2, volume_size=4).framelist == ['frame_000000', 'frame_000002', 'frame_000004']
    assert PreparedDataset(path, device=None, skip=2, maxframes=2, volume_size=4).framelist == ['frame_000000', 'frame_000002']
    # the band's range counts positions in the frame list, not frame numbers: with skip 2, position 1 is frame 2
    occ = {'range': 2, 'mid': 24, 'width': 10}
    ds = PreparedDataset(path, device=None, skip=2, volume_size=4, occlude=True, occlusion=occ)
    assert [f['band'] for f in ds.frames] == [True, True, False]
    assert ds.alphas[1][:, 19:29].sum() == 0 and ds.alphas[2][:, 19:29].sum() > 0 and ds.alphas[1][:, :19].sum() > 0
    # a band that swallows the whole mask leaves the frame out of the epoch (train.py:395-396)
    ds = PreparedDataset(path, device=None, volume_size=4, occlude=True, occlusion={'range': 2, 'mid': 24, 'width': 48})
    assert ds.epoch_frames == [2, 3, 4] and ds.frames[0]['empty'] and len(ds) == 5
    for kw, word in (({'crop_image_scale': [32, 32]}, 'crop_image_scale'), ({'upsample_pc': True}, 'upsample_pc'),
                     ({'resize_img_scale': 0.5}, 'resize_img_scale')):
        with pytest.raises(NotImplementedError, match=word):
            PreparedDataset(path, device=None, volume_size=4, **kw)
    half = PreparedDataset(path, device=None, volume_size=4, resize_img_scale=0.5, images_prescaled=True)
    full = PreparedDataset(path, device=None, volume_size=4)
    assert np.array_equal(half.frames[0]['K'][:2], full.frames[0]['K'][:2] * 0.5) and half.frames[0]['K'][2, 2] == 1.0
    with open(os.path.join(path, 'cameras.pkl'), 'rb') as f:
        cams = pickle.load(f)
    cams['frame_000003']['distortions'] = np.zeros(5)
    with open(os.path.join(path, 'cameras.pkl'), 'wb') as f:
        pickle.dump(cams, f)
    with pytest.raises(NotImplementedError, match='distortions'):
        PreparedDataset(path, device=None, volume_size=4)


def test_draws_from_uniforms_inverts_the_recorded_draws(golden_dataset):
    """u1 = (select_idx + 0.5) / count maps back to select_idx, so the device builder can replay the recording."""
    g, path = golden_dataset
    rs = tbr.Restatement(path, **golden_cfg(g))
    for i in range(len(rs.framelist)):
        _, _, subject, off = rs.frame_masks(i)
        cls, idx, count = g[f'f{i}.draw.cls'], g[f'f{i}.draw.select_idx'], g[f'f{i}.draw.count']
        u = np.stack([np.where(cls == 0, 0.0, 0.9), (idx + 0.5) / count], 1)
        assert tbr.draws_from_uniforms(u, subject, off, 0.8) == list(zip(cls.tolist(), idx.tolist()))


def test_recorder_reproduces_the_committed_recording(tmp_path):
    from oracle.ref_harness import shims
    if not os.path.isdir(shims.REF):
        pytest.skip('the reference tree is not on this machine')
    env = {**os.environ, 'OCCNERF_GOLDEN_DIR': str(tmp_path)}
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tools', 'record_train_batch_golden.py')], env=env,
                          stdout=subprocess.DEVNULL, timeout=150)
    new, old = np.load(str(tmp_path / 'train_batch_ref.npz')), golden()
    assert sorted(new.files) == sorted(old)
    for k in old:
        assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k]), k
    assert os.path.getsize(GOLDEN) <= max(os.path.getsize(os.path.join(ROOT, 'tests', 'golden', f))
                                          for f in os.listdir(os.path.join(ROOT, 'tests', 'golden')) if f != 'train_batch_ref.npz')


_LOADER_SCRIPT = '''
import sys
data_type = sys.argv.pop(1)                 # configs parses sys.argv at import
from core.data import create_dataloader
loader = create_dataloader(data_type)
print('LOADER', type(loader).__module__, type(loader).__name__, len(loader), len(loader.dataset))
'''


def _loader(data_type, *opts, cwd=None):
    cmd = [sys.executable, '-c', _LOADER_SCRIPT, data_type, '--cfg',
           os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml')] + list(opts)
    out = subprocess.check_output(cmd, env={**os.environ, 'PYTHONPATH': ROOT}, text=True, timeout=150, cwd=cwd)
    return [line for line in out.splitlines() if line.startswith('LOADER')][0].split()[1:]


def test_create_dataloader_returns_the_loader_for_a_dataset_path(tmp_path):
    path = str(tmp_path / 'd')
    load_tool().make_dataset(path, frames=3, width=48, height=40, seed=2)
    opts = ['train.dataset_path', path, 'resize_img_scale', '1.0', 'patch.size', '16', 'mweight_volume.volume_size', '4']
    assert _loader('train', *opts) == ['occnerf_amd.dataset', 'PatchBatchLoader', '3', '3']
    assert _loader('movement', *opts) == ['occnerf_amd.dataset', 'WholeFrames', '3', '3']
    # the reference's dataset names resolve as dataset_args.py resolves them, relative to the working directory
    os.makedirs(str(tmp_path / 'dataset' / 'zju_mocap'))
    os.symlink(path, str(tmp_path / 'dataset' / 'zju_mocap' / '387'))
    assert _loader('train', 'train.dataset', 'zju_387_train', *opts[2:], cwd=str(tmp_path)) == \
        ['occnerf_amd.dataset', 'PatchBatchLoader', '3', '3']
    # the synthetic default is what it was
    assert _loader('movement', 'render_frames', '7') == ['occnerf_amd.sequence', 'SyntheticFrames', '7', '7']
    with pytest.raises(subprocess.CalledProcessError):
        _loader('train')


def test_whole_frames_have_the_batch_dimension(tmp_path):
    import torch
    from occnerf_amd.dataset import PreparedDataset, WholeFrames
    path = str(tmp_path / 'd')
    load_tool().make_dataset(path, frames=2, width=48, height=40, seed=2)
    batches = list(WholeFrames(PreparedDataset(path, device=None, volume_size=4), [0., 0., 0.]))
    assert len(batches) == 2
    b = batches[1]
    n = int(b['ray_mask'].sum())
    assert b['rays'].shape == (1, 2, n, 3) and b['target_rgbs'].shape == (1, n, 3) and b['ray_alpha'].shape == (1, n, 3)
    assert b['frame_name'] == ['frame_000001'] and b['img_width'] == 48 and b['rays'].dtype == torch.float32


def test_every_device_case_meets_its_coverage_condition(tmp_path):
    """The cases tests/test_g_train_batch.py compares on the GPU, checked here on the restatement's side: both classes
    non-empty except where the case is built otherwise, a clip / hole / duplicate row where the case claims one."""
    from tests import train_batch_cases as cases
    paths = cases.make_datasets(tmp_path)
    for name in cases.CASES:
        r, draws = cases.restate(cases.build_case(name, paths))
        assert len(draws) == r['patch_masks'].shape[0] and r['patch_div_indices'][-1] == r['rays'].shape[1] > 0, name
