"""GPU: the mesh rasteriser.  csrc/mesh_raster.hip against the numpy definition
(tests/mesh_raster_restatement.py) -- xy, z, vflag, cover, tri, depth, rgb and the counts all EQUAL, floats as bit patterns --
and run.py --type mesh with mesh_view.frames end to end.  The cases are those of tests/test_mesh_raster_restatement.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_raster_restatement as rr
from tests import mesh_restatement as mr
from tests.gpu_util import T, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ('xy', 'z', 'vflag', 'cover', 'tri', 'depth', 'rgb')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _device(c, **kw):
    from occnerf_amd import mesh_view
    H, W = kw.get('H', c['H']), kw.get('W', c['W'])
    out = mesh_view.rasterize(T(c['pos']), T(c['faces']), T(c['colors']), c['K'], c['E'], H, W, kw.get('bgcolor', (255, 255, 255)),
                              faces_checked=kw.get('faces_checked', False))
    V = len(c['pos'])
    assert all(v.is_cuda for v in out.values())
    assert [out[k].dtype for k in OUTPUTS] == [torch.int32, torch.float64, torch.uint8, torch.uint8, torch.int32, torch.float32,
                                               torch.uint8]
    assert tuple(out['xy'].shape) == (V, 2) and tuple(out['cover'].shape) == (H, W) and tuple(out['rgb'].shape) == (H, W, 3)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _equal(got, want, name):
    for k in OUTPUTS:
        same(_bits(got[k]), _bits(want[k]), f'{name}: {k}')
    same(got['counts'], rr.count_vector(want['counts']), f'{name}: counts {rr.COUNTS}')


@pytest.mark.parametrize('name', sorted(rr.CASES))
def test_kernels_are_the_restatement_on_the_hand_cases(name):
    c = rr.CASES[name]()
    want = rr.run_case(c, bgcolor=(10, 200, 30))
    got = _device(c, bgcolor=(10, 200, 30), faces_checked=True)      # (flags: the index outside [0, V) reaches the kernels)
    _equal(got, want, name)
    n = want['counts']
    if name == 'mixed':
        # the wide pass is taken for exactly the two large triangles, and both passes own pixels of the final image
        big = np.nonzero((c['faces'] < 4).all(1))[0]
        assert n['wide'] == 2 and got['counts'][5] == 2
        from_big = np.isin(got['tri'], big)
        assert from_big.any() and (~from_big & (got['tri'] >= 0)).any() and n['covered'] == c['H'] * c['W']
    if name == 'grid':
        assert n['wide'] == len(c['faces'])
    if name == 'grid4':
        assert n['wide'] == 0 and n['covered'] > 0
    if name == 'offscreen':
        assert n['covered'] == 0 and n['offscreen'] == len(c['faces']) and (got['tri'] == -1).all()
        assert np.isposinf(got['depth']).all() and (got['rgb'] == np.array([10, 200, 30], np.uint8)).all()
    if name == 'flags':
        assert [n[k] for k in rr.COUNTS[:5]] == [1, 1, 1, 2, 1]


@pytest.mark.parametrize('n_tri', [0, 1, 63, 64, 65, 257])
def test_triangle_counts_around_the_block_size(n_tri):
    c = rr.case_random(n_tri)
    _equal(_device(c), rr.run_case(c), f'T = {n_tri}')


@pytest.mark.parametrize('size', [(48, 63), (47, 65), (5, 130), (33, 1)])
def test_widths_that_are_no_multiple_of_the_wave(size):
    H, W = size
    c = rr.case_blobs()
    _equal(_device(c, H=H, W=W), rr.run_case(c, H=H, W=W), f'{W} x {H}')


@pytest.fixture(scope='module')
def smpl_frames(tmp_path_factory):
    """A tool-made dataset of 3 frames of 64 x 48 and, per frame, the posed SyntheticSMPL mesh in the body's own space with the
    frame's K and body-space E, and the restatement's image of it -- computed once, never changed."""
    from occnerf_amd.dataset import PreparedDataset
    tool = rr.load_tool()
    path = str(tmp_path_factory.mktemp('raster') / 'ds')
    tool.make_dataset(path, frames=3, width=64, height=48, seed=0)
    ds = PreparedDataset(path, device=None)
    import pickle
    with open(os.path.join(path, 'mesh_infos.pkl'), 'rb') as f:
        infos = pickle.load(f)
    out = []
    for i in (0, 2):
        f = ds.frames[i]
        pos, faces, colors = rr.posed_smpl(tool, infos[f['frame_name']])
        c = {'pos': pos, 'faces': faces, 'colors': colors, 'K': f['K'], 'E': f['E'], 'H': 48, 'W': 64}
        out.append((c, rr.run_case(c), ds.gt_alpha(i)))
    return out


def test_the_posed_smpl_mesh_in_a_dataset_frame(smpl_frames):
    from occnerf_amd import mesh_view
    for k, (c, want, gt) in enumerate(smpl_frames):
        assert len(c['faces']) > 13000 and want['counts']['covered'] > 100
        got = _device(c)
        _equal(got, want, f'smpl frame {k}')
        stats = mesh_view.silhouette_iou(T(got['cover']), T(gt))
        assert stats == rr.mask_iou(want['cover'], gt)
        print(f"\n   frame {k}: {want['counts']}, IoU {stats[2]:.4f}, inside share {stats[4]:.4f}")


def test_two_runs_give_the_same_bytes(smpl_frames):
    for c in (smpl_frames[0][0], rr.case_mixed()):
        a, b = _device(c), _device(c)
        for k in OUTPUTS + ('counts',):
            assert a[k].tobytes() == b[k].tobytes(), k


def test_refusals():
    from occnerf_amd import mesh_view, ops
    c = rr.case_ties()
    pos, faces, colors = T(c['pos']), T(c['faces']), T(c['colors'])
    bad = faces.clone()
    bad[1, 2] = len(c['pos'])
    with pytest.raises(RuntimeError, match=r'mesh_raster: face index 9 outside \[0, 9\)'):
        mesh_view.rasterize(pos, bad, colors, c['K'], c['E'], 48, 64)
    bad[1, 2] = -3
    with pytest.raises(RuntimeError, match=r'mesh_raster: face index -3 outside'):
        mesh_view.rasterize(pos, bad, colors, c['K'], c['E'], 48, 64)
    with pytest.raises(RuntimeError, match='mesh_project: pos must be a CUDA'):
        mesh_view.rasterize(pos.cpu(), faces, colors, c['K'], c['E'], 48, 64)
    with pytest.raises(RuntimeError, match='mesh_raster: faces must be a CUDA'):
        mesh_view.rasterize(pos, faces.cpu(), colors, c['K'], c['E'], 48, 64)
    with pytest.raises(RuntimeError, match='mesh_raster: faces must be torch.int32'):
        mesh_view.rasterize(pos, faces.long(), colors, c['K'], c['E'], 48, 64)
    with pytest.raises(RuntimeError, match='mesh_resolve: colors must be a CUDA'):
        mesh_view.rasterize(pos, faces, colors.cpu(), c['K'], c['E'], 48, 64)
    with pytest.raises(RuntimeError, match='mesh_raster: H = 0'):
        mesh_view.rasterize(pos, faces, colors, c['K'], c['E'], 0, 64)
    with pytest.raises(RuntimeError, match='mesh_raster: H = 48, W = 16385'):
        mesh_view.rasterize(pos, faces, colors, c['K'], c['E'], 48, 16385)
    K = c['K'].copy()
    K[0, 1] = 0.5
    with pytest.raises(NotImplementedError, match='mesh_project: skew'):
        mesh_view.rasterize(pos, faces, colors, K, c['E'], 48, 64)
    # V = 0 or T = 0: the empty image, nothing is launched
    out = mesh_view.rasterize(pos[:0].contiguous(), faces[:0].contiguous(), colors[:0].contiguous(), c['K'], c['E'], 48, 64, (1, 2, 3))
    assert not out['cover'].any() and (out['tri'] == -1).all() and torch.isinf(out['depth']).all() and not out['counts'].any()
    assert (out['rgb'].cpu() == torch.tensor([1, 2, 3], dtype=torch.uint8)).all() and tuple(out['xy'].shape) == (0, 2)
    assert ops.MESH_RASTER_COUNTS == rr.COUNTS
    torch.cuda.synchronize()


# ------------------------------------------------------------------ end to end
def _run_py(tmp, *extra, ok=True):
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'),
           '--type', 'mesh', 'mesh.resolution', '24', 'N_samples', '16'] + list(extra)
    os.makedirs(str(tmp), exist_ok=True)
    out = subprocess.run(cmd, cwd=str(tmp), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True)
    if not ok:
        return out
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return tmp / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'mesh'


def test_run_py_views_the_posed_mesh(tmp_path):
    """The command of DESIGN.md section 7j on the seeded checkpoint and a tool-made 64 x 64 dataset.  The seeded weights put no
    surface at the default level, so -- as tests/test_p_mesh_pose.py does -- the level is the median of the 24-grid's density: a
    surface of random weights all over the box, no body, whose IoU with the mask means nothing; what is checked is that every
    integer of view.json is the restatement's on the vertices of the posed PLY the same run wrote."""
    from PIL import Image
    from occnerf_amd.dataset import PreparedDataset
    tool = rr.load_tool()
    path = str(tmp_path / 'ds')
    tool.make_dataset(path, frames=3, width=64, height=64, seed=0)
    common = ('train.dataset_path', path, 'resize_img_scale', '1.0', 'mesh.level', '0.7231')
    folder = _run_py(tmp_path / 'view', *common, 'mesh_view.frames', '[0, 2]', 'mesh_pose.frames', '[0, 2]')
    plain = _run_py(tmp_path / 'plain', *common)
    blob = (folder / 'mesh.ply').read_bytes()
    assert blob == (plain / 'mesh.ply').read_bytes()
    assert sorted(os.listdir(plain)) == ['mesh.json', 'mesh.ply']
    canon = mr.parse_ply(blob)
    colors = np.stack([canon['red'], canon['green'], canon['blue']], 1)
    info = json.loads((folder / 'view.json').read_text())
    ds = PreparedDataset(path, device=None)
    V, n_tri = canon['x'].shape[0], canon['faces'].shape[0]
    assert V > 500 and (info['vertices'], info['triangles'], info['height'], info['width']) == (V, n_tri, 64, 64)
    assert [f['frame'] for f in info['frames']] == [0, 2]
    assert sorted(os.listdir(folder / 'view')) == ['frame_000000.png', 'frame_000002.png']
    ious = []
    for f in info['frames']:
        ply = mr.parse_ply((folder / 'posed' / (f['name'] + '.ply')).read_bytes())
        p = np.ascontiguousarray(np.stack([ply['x'], ply['y'], ply['z']], 1))
        fr = ds.frames[f['frame']]
        assert f['name'] == fr['frame_name']
        want = rr.rasterize(p, canon['faces'], colors, fr['K'], fr['E'], 64, 64)
        inter, union, iou, covered, inside = rr.mask_iou(want['cover'], ds.gt_alpha(f['frame']))
        assert (f['intersection'], f['union'], f['covered']) == (inter, union, covered) and covered == want['counts']['covered']
        assert f['iou'] == iou and f['inside_share'] == inside
        assert f['dropped'] == {k: want['counts'][k] for k in rr.COUNTS[:5]} and f['wide'] == want['counts']['wide']
        assert set(f['seconds']) == {'unoffset', 'pose', 'raster', 'compare'} and f['posing_flagged'] >= 0
        img = np.array(Image.open(folder / 'view' / (f['name'] + '.png')))
        assert img.shape == (64, 128, 3)
        same(img[:, :64], want['rgb'], 'the mesh panel')
        same(img[:, 64:], ds.truth_u8(f['frame']), 'the photograph')
        ious.append(iou)
        print(f"\n   {f['name']}: IoU {iou}, covered {covered}, dropped {f['dropped']}, wide {f['wide']}")
    assert info['mean_iou'] == float(np.mean([v for v in ious if v is not None]))


def test_run_py_refuses_views_without_a_dataset(tmp_path):
    out = _run_py(tmp_path, 'mesh_view.frames', '[0]', ok=False)
    assert out.returncode != 0 and 'mesh_view.frames' in out.stderr and 'prepared dataset' in out.stderr
    assert not (tmp_path / 'experiments').exists() or not list((tmp_path / 'experiments').rglob('view*'))
