"""GPU: the device-side patch batch builder (occnerf_amd/csrc/batch.hip, ops.patch_batch), the loader around it
(occnerf_amd/dataset.py) and train.py on a prepared dataset.

The HIP batch is compared with tests/train_batch_restatement.py on the same draws.  Integer results and the float64 blend
are the same operations on both sides, so they must be EQUAL: patch_masks, patch_div_indices, xy_min, the row count, both
row <-> pixel maps, target_patches, target_rgbs.  rays / near / far must equal a gather, by the restatement's select_inds,
of what ops.gen_rays returns for the frame; how close gen_rays is to numpy is tests/test_f_image_rays.py's business."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import train_batch_cases as cases
from tests import train_batch_restatement as tbr
from tests.gpu_util import DEV, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def paths(tmp_path_factory):
    return cases.make_datasets(tmp_path_factory.mktemp('train_batch'))


def hip_batch(path, cfg, frame, bgcolor, u):
    """(batch dict as numpy, rays8, box mask) of one frame through PreparedDataset + ops.gen_rays + ops.patch_batch."""
    from occnerf_amd import ops
    from occnerf_amd.dataset import PreparedDataset
    ds = PreparedDataset(path, device=DEV, volume_size=cfg['volume_size'], occlude=cfg['occlude'], occlusion=cfg['occlusion'])
    f = ds.frames[frame]
    rays8, box = ops.gen_rays(f['K'], f['E'], ds.height, ds.width, f['dst_bbox_min'], f['dst_bbox_max'], DEV)
    out = ops.patch_batch(ds._dev['image'][frame], ds._dev['alpha'][frame], rays8, box, cfg['N_patches'], cfg['size'], u,
                          cfg['sample_subject_ratio'], bgcolor)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, rays8.cpu().numpy(), box.cpu().numpy().astype(bool)


def compare(got, rays8, box, r, n_patches, size):
    """The device batch `got` against the restatement's result r (or a recording with the same keys)."""
    same(box, np.asarray(r['ray_mask']), 'box mask (gen_rays) vs the restatement ray_mask')
    sel = np.asarray(r['patch_mask'])
    R = int(got['n_rows'][0])
    print(f'   rows {R} of {n_patches * size * size}; holes {int((~np.asarray(r["patch_masks"])).sum())}; duplicate rows '
          f'{sel.size - np.unique(sel).size}')
    assert R == sel.size == int(r['patch_div_indices'][-1])
    same(got['patch_div_indices'], np.asarray(r['patch_div_indices']).astype(np.int32), 'patch_div_indices')
    same(got['patch_masks'], np.asarray(r['patch_masks']), 'patch_masks')
    if '_xy_min' in r:
        same(got['xy_min'], np.asarray(r['_xy_min']).astype(np.int32), 'xy_min')
    pix_of_row, row_of_pix = tbr.pixel_maps(r['patch_masks'])
    same(got['pix_of_row'][:R], pix_of_row, 'pix_of_row')
    same(got['row_of_pix'], row_of_pix, 'row_of_pix')
    same(got['target_patches'], np.asarray(r['target_patches']), 'target_patches')
    same(got['target_rgbs'][:R], np.asarray(r['target_rgbs']), 'target_rgbs')
    compact = rays8[box]                                   # the frame's ray list, as occnerf_amd/rays.py compacts it
    same(got['rays'][0, :R], compact[sel, 0:3], 'rays_o')
    same(got['rays'][1, :R], compact[sel, 3:6], 'rays_d')
    same(got['near'][:R, 0], compact[sel, 6], 'near')
    same(got['far'][:R, 0], compact[sel, 7], 'far')


@pytest.mark.parametrize('name', cases.CASES)
def test_hip_batch_equals_the_restatement(name, paths):
    case = cases.build_case(name, paths)
    r, draws = cases.restate(case)                          # asserts the coverage conditions first
    cfg = case['cfg']
    print(f'\n   {name}: draws {draws}')
    got, rays8, box = hip_batch(case['path'], cfg, case['frame'], case['bgcolor'], case['u'])
    compare(got, rays8, box, r, cfg['N_patches'], cfg['size'])


def test_hip_batch_equals_the_recorded_reference(tmp_path):
    """The recorded select_idx values map to u1 = (select_idx + 0.5) / count, which maps back to the same index; the device
    batch then equals the recording of the unmodified reference itself, not only the restatement."""
    from tests.test_train_batch_restatement import golden, golden_cfg, golden_tool_args
    g = golden()
    cfg = golden_cfg(g)
    path = str(tmp_path / 'golden')
    cases.load_tool().make_dataset(path, **golden_tool_args(g))
    rs = tbr.Restatement(path, **cfg)
    for i in range(len(rs.framelist)):
        _, _, subject, off = rs.frame_masks(i)
        counts = (int(subject.sum()), int(off.sum()))
        assert min(counts) > 0
        draws = list(zip(g[f'f{i}.draw.cls'].tolist(), g[f'f{i}.draw.select_idx'].tolist()))
        u = cases.u_for(draws, counts)
        assert tbr.draws_from_uniforms(u, subject, off, cfg['sample_subject_ratio']) == draws
        got, rays8, box = hip_batch(path, cfg, i, g[f'f{i}.bgcolor'], u)
        rec = {k: g[f'f{i}.{k}'] for k in ('ray_mask', 'patch_mask', 'patch_div_indices', 'patch_masks', 'target_patches',
                                           'target_rgbs')}
        compare(got, rays8, box, rec, cfg['N_patches'], cfg['size'])


def test_patch_batch_refuses_bad_arguments(paths):
    from occnerf_amd import ops
    from occnerf_amd.dataset import PreparedDataset
    ds = PreparedDataset(paths['wide'], device=DEV, volume_size=4)
    f = ds.frames[0]
    rays8, box = ops.gen_rays(f['K'], f['E'], ds.height, ds.width, f['dst_bbox_min'], f['dst_bbox_max'], DEV)
    img, alpha = ds._dev['image'][0], ds._dev['alpha'][0]
    with pytest.raises(RuntimeError, match='does not fit'):
        ops.patch_batch(img, alpha, rays8, box, 2, 96, np.zeros((2, 2)), 0.8, [0, 0, 0])
    with pytest.raises(RuntimeError, match='not in'):
        ops.patch_batch(img, alpha, rays8, box, 2, 16, np.ones((2, 2)), 0.8, [0, 0, 0])
    with pytest.raises(RuntimeError, match='n_patches'):
        ops.patch_batch(img, alpha, rays8, box, 65, 8, np.zeros((65, 2)), 0.8, [0, 0, 0])
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.patch_batch(img.cpu(), alpha, rays8, box, 2, 16, np.zeros((2, 2)), 0.8, [0, 0, 0])


def _epochs(path, prefetch, n_batches, occlusion):
    from occnerf_amd.dataset import PatchBatchLoader, PreparedDataset
    ds = PreparedDataset(path, device=DEV, volume_size=4, occlude=True, occlusion=occlusion)
    loader = PatchBatchLoader(ds, n_patches=4, size=16, bgcolor=None, seed=5, prefetch=prefetch)
    out = []
    for _ in range(n_batches):
        b = next(loader)
        torch.cuda.synchronize()
        out.append({k: (v.cpu().numpy().copy() if torch.is_tensor(v) else np.copy(v)) for k, v in b.items()})
    return ds, out


def test_loader_prefetch_equals_inline_and_skips_empty_frames(tmp_path):
    path = str(tmp_path / 'four')
    cases.load_tool().make_dataset(path, frames=4, width=64, height=64, seed=21, focal=900.0)
    occlusion = {'range': 1, 'mid': 32, 'width': 64}          # the band swallows frame 0's whole mask
    ds, a = _epochs(path, True, 6, occlusion)
    _, b = _epochs(path, False, 6, occlusion)
    assert ds.frames[0]['empty'] and ds.epoch_frames == [1, 2, 3] and len(a) == len(b) == 6
    assert sorted(x['frame'] for x in a[:3]) == sorted(x['frame'] for x in a[3:]) == [1, 2, 3]      # two epochs, no frame 0
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for k in x:
            assert np.array_equal(x[k], y[k]), k
        assert x['n_rows'] == x['patch_div_indices'][-1] == x['rays'].shape[1] == x['pix_of_row'].shape[0] > 0
    assert any(not np.array_equal(a[0]['bgcolor'], x['bgcolor']) for x in a[1:])                    # a colour per batch
    # a batch is what the restatement makes of the same draws
    rs = tbr.Restatement(path, N_patches=4, size=16, occlude=True, occlusion=occlusion, volume_size=4)
    x = a[4]
    _, _, subject, off = rs.frame_masks(x['frame'])
    r = rs.getitem(x['frame'], x['bgcolor'], tbr.draws_from_uniforms(x['u'], subject, off, 0.8))
    same(x['target_patches'], r['target_patches'], 'loader target_patches')
    same(x['target_rgbs'], r['target_rgbs'], 'loader target_rgbs')
    same(x['patch_masks'], r['patch_masks'], 'loader patch_masks')
    same(x['patch_div_indices'], r['patch_div_indices'], 'loader patch_div_indices')
    for k in ('dst_Rs', 'dst_Ts', 'cnl_gtfms', 'dst_posevec'):
        assert np.abs(x[k] - r[k]).max() <= 2e-6, k


def test_patch_images_from_device_maps_assembles_like_the_host_constructor(paths):
    from occnerf_amd.lpips import PatchImages
    case = cases.build_case('box_edge_holes', paths)
    got, _, _ = hip_batch(case['path'], case['cfg'], case['frame'], case['bgcolor'], case['u'])
    R = int(got['n_rows'][0])
    dev_maps = PatchImages.from_device_maps(torch.from_numpy(got['pix_of_row'][:R].copy()).to(DEV),
                                            torch.from_numpy(got['row_of_pix']).to(DEV), 4, 16)
    host = PatchImages(got['pix_of_row'][:R], 4, 16, DEV)
    rgb = torch.rand(R, 3, device=DEV)
    assert torch.equal(dev_maps.assemble(rgb, [0.1, 0.2, 0.3]), host.assemble(rgb, [0.1, 0.2, 0.3]))
    with pytest.raises(RuntimeError, match='int32'):
        PatchImages.from_device_maps(dev_maps.pix_of_row.long(), dev_maps.row_of_pix, 4, 16)


@pytest.mark.parametrize('lossweights', ["{'mse': 0.2, 'comp': 1.0}", "{'lpips': 1.0, 'mse': 0.2, 'comp': 1.0}"],
                         ids=['mse', 'lpips'])
def test_train_py_on_a_prepared_dataset(lossweights, tmp_path):
    """python train.py on a tool-made dataset: exit status 0, a finite loss on every logged line, latest.tar written, no
    teacher network.  Whether the loss falls is not asserted: nobody has measured how fast this field fits disc-splat
    images."""
    path = str(tmp_path / 'data')
    cases.load_tool().make_dataset(path, frames=4, width=64, height=64, seed=31, focal=900.0)
    cmd = [sys.executable, os.path.join(ROOT, 'train.py'), '--cfg', os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'),
           'train.dataset_path', path, 'resize_img_scale', '1.0', 'N_samples', '32', 'train.maxiter', '6',
           'train.log_interval', '1', 'patch.size', '16', 'patch.N_patches', '4', 'occlude', 'True', 'occlusion.range', '2',
           'occlusion.mid', '32', 'occlusion.width', '10', 'train.lossweights', lossweights]
    out = subprocess.check_output(cmd, cwd=str(tmp_path), env={**os.environ, 'PYTHONPATH': ROOT}, text=True, timeout=170)
    print(out)
    assert 'targets are the dataset images (no teacher network)' in out and '4 frames of 64 x 64' in out
    assert ('lpips: trunk' in out) == ('lpips' in lossweights)
    lines = [line for line in out.splitlines() if line.startswith('iter')]
    losses = [float(line.split('loss')[1].split()[0]) for line in lines]
    assert len(losses) == 6 and all(np.isfinite(losses))
    assert all(int(line.split('rays')[1].split()[0]) > 0 for line in lines)
    ckpt = torch.load(tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'latest.tar',
                      map_location='cpu')
    assert set(ckpt) == {'iter', 'network', 'optimizer'} and ckpt['iter'] == 6
