"""GPU: the geometry maps (occnerf_amd/csrc/gbuffer.hip, ops.gbuffer_points / gbuffer_normals, occnerf_amd/gbuffer.py) equal
their numpy definition (tests/gbuffer_restatement.py) byte for byte -- t, the points, the normals, the
valid bits and the three 8-bit panels -- on the hand cases and the seeded frames of tests/gbuffer_cases.py, on one rendered
frame, and through run.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import gbuffer_cases as cases
from tests import gbuffer_restatement as G
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml')

_want = {}


def want_of(name, case):
    """The definition's maps of a case, computed once and shared."""
    if name not in _want:
        _want[name] = G.geometry_maps(**cases.definition_args(case))
    return _want[name]


def dev_args(case):
    return {'width': case['W'], 'height': case['H'], 'ray_index': torch.from_numpy(case['ray_index']).to(DEV),
            'rays': torch.from_numpy(case['rays']).to(DEV), 'depth': torch.from_numpy(case['depth']).to(DEV),
            'alpha': torch.from_numpy(case['alpha']).to(DEV), 'min_alpha': case['min_alpha'], 'bgcolor': case['bg']}


def same_bytes(got, want, name):
    """Equal as bytes: a -0.0 for a 0.0 or another NaN would count."""
    got, want = np.ascontiguousarray(got.cpu().numpy() if torch.is_tensor(got) else got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.uint8).reshape(got.shape + (-1,)) != want.view(np.uint8).reshape(want.shape + (-1,))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad.any(-1))[0])
        raise AssertionError(f'{name}: {int(bad.any(-1).sum())}/{got.size} entries differ, first at {i}: got {got[i]!r} '
                             f'want {want[i]!r}')


def compare(got, want, name, panels=('depth', 'normal', 'shaded')):
    torch.cuda.synchronize()
    same_bytes(got['points'], want['points'], f'{name}: points')
    same_bytes(got['t'].contiguous(), want['t'], f'{name}: t')
    same_bytes(got['normal'], want['normal'], f'{name}: normal')
    same_bytes(got['valid'], want['valid'], f'{name}: valid')
    for k in ('depth', 'normal', 'shaded'):
        assert (f'{k}_u8' in got) == (k in panels), (name, k)
        if k in panels:
            same_bytes(got[f'{k}_u8'], want[f'{k}_u8'], f'{name}: {k} panel')


ALL_CASES = {**{f'hand_{k}': v for k, v in cases.hand_cases().items()}, **cases.random_cases()}


@pytest.mark.parametrize('name', sorted(ALL_CASES))
def test_kernels_equal_the_definition(name):
    """Every map and panel, byte for byte, with a fixed depth range; and a second run gives the same bytes."""
    from occnerf_amd.gbuffer import geometry_maps
    case = ALL_CASES[name]
    want = want_of(name, case)
    got = geometry_maps(**dev_args(case), t_range=case['t_range'])
    compare(got, want, name)
    again = geometry_maps(**dev_args(case), t_range=torch.tensor(case['t_range'], dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    for k in ('points', 'normal', 'valid', 'depth_u8', 'normal_u8', 'shaded_u8'):
        same_bytes(again[k], got[k].cpu().numpy(), f'{name}: second run {k}')
    same_bytes(got['t_range'], np.asarray(case['t_range'], np.float32), f'{name}: t_range')


@pytest.mark.parametrize('name', ['37x29_60', '130x70_100'])
def test_default_range_and_each_panel_alone(name):
    """t_range None: the frame's near.min() .. far.max(), reduced on the device; each panel pointer null in turn, and all."""
    from occnerf_amd.gbuffer import geometry_maps
    case = ALL_CASES[name]
    rng = G.default_t_range(case['near'], case['far'])
    want = G.geometry_maps(**{**cases.definition_args(case), 't_range': rng})
    near, far = torch.from_numpy(case['near']).to(DEV), torch.from_numpy(case['far']).to(DEV)
    got = geometry_maps(**dev_args(case), near=near, far=far)
    compare(got, want, f'{name}: default range')
    same_bytes(got['t_range'], np.asarray(rng, np.float32), f'{name}: default t_range')
    for panels in (('normal', 'shaded'), ('depth', 'shaded'), ('depth', 'normal'), ('shaded',), ()):
        got = geometry_maps(**dev_args(case), near=near, far=far, panels=panels)
        compare(got, want, f'{name}: panels {panels}', panels)
    got = geometry_maps(**dev_args(case), panels=('normal',))                  # no range at all: only the depth panel needs one
    compare(got, want, f'{name}: no range', ('normal',))
    assert got['t_range'] is None


def test_refusals_are_made_by_name():
    from occnerf_amd import _lib, ops
    from occnerf_amd.gbuffer import geometry_maps
    case = ALL_CASES['hand_borders']
    a = dev_args(case)
    for k in ('ray_index', 'rays', 'depth', 'alpha'):
        with pytest.raises(RuntimeError, match=f'geometry_maps: {k} must be a CUDA'):
            geometry_maps(**{**a, k: a[k].cpu()}, t_range=(0., 8.))
    with pytest.raises(RuntimeError, match='t_range must be a CUDA'):
        geometry_maps(**a, t_range=torch.tensor([0., 8.]))
    with pytest.raises(RuntimeError, match='depth panel needs t_range'):
        geometry_maps(**a)
    with pytest.raises(RuntimeError, match='near must be a CUDA'):
        geometry_maps(**a, near=torch.ones(9, 1), far=torch.ones(9, 1, device=DEV))
    with pytest.raises(RuntimeError, match="unknown panel 'albedo'"):
        geometry_maps(**a, t_range=(0., 8.), panels=('albedo',))
    with pytest.raises(RuntimeError, match='R = 9 is larger than height \\* width = 6'):
        geometry_maps(**{**a, 'height': 2}, t_range=(0., 8.))
    with pytest.raises(RuntimeError, match='must be positive'):
        geometry_maps(**{**a, 'height': 0}, t_range=(0., 8.))
    with pytest.raises(RuntimeError, match='depth and alpha must be \\[9\\]'):
        geometry_maps(**{**a, 'depth': a['depth'][:8]}, t_range=(0., 8.))
    with pytest.raises(RuntimeError, match='gbuffer_points: ray_index must be torch.int64'):
        geometry_maps(**{**a, 'ray_index': a['ray_index'].int()}, t_range=(0., 8.))
    with pytest.raises(RuntimeError, match='rays must be float32 \\[2,R,3\\]'):
        geometry_maps(**{**a, 'rays': a['rays'].permute(1, 0, 2).contiguous()}, t_range=(0., 8.))
    points, valid, pix_ray = ops.gbuffer_points(a['ray_index'], a['rays'], a['depth'], a['alpha'], 0.5, 3, 3)
    with pytest.raises(RuntimeError, match='pix_ray must be int32 \\[3,3\\]'):
        ops.gbuffer_normals(points, pix_ray[:2].contiguous(), a['rays'], None, case['bg'], ('normal',))
    with pytest.raises(RuntimeError, match='points must be float32 \\[H,W,4\\]'):
        ops.gbuffer_normals(points[..., :3].contiguous(), pix_ray, a['rays'], None, case['bg'], ('normal',))
    # the C entries refuse on their own, before any launch
    lib = _lib.lib()
    p, v, q = points.data_ptr(), valid.data_ptr(), pix_ray.data_ptr()
    r, z = a['rays'].data_ptr(), a['depth'].data_ptr()
    assert lib.occnerf_gbuffer_points(a['ray_index'].data_ptr(), 10, r, z, z, 0.5, 3, 3, p, v, q, None) != 0
    assert b'gbuffer_points: R = 10 is larger than height * width = 9' in lib.occnerf_last_error()
    assert lib.occnerf_gbuffer_points(None, 9, r, z, z, 0.5, 3, 3, p, v, q, None) != 0
    assert b'gbuffer_points: null argument' in lib.occnerf_last_error()
    assert lib.occnerf_gbuffer_points(a['ray_index'].data_ptr(), 9, r, z, z, 0.5, 0, 3, p, v, q, None) != 0
    assert b'gbuffer_points: bad sizes' in lib.occnerf_last_error()
    bg = np.asarray(case['bg'], np.float32)
    pbg = bg.ctypes.data
    nrm = torch.empty(3, 3, 3, device=DEV)
    assert lib.occnerf_gbuffer_normals(p, q, r, 9, 3, 3, None, pbg, nrm.data_ptr(), v, v, None, None, None) != 0
    assert b'gbuffer_normals: null argument' in lib.occnerf_last_error()                  # a depth panel without a range
    assert lib.occnerf_gbuffer_normals(p, q, r, 10, 3, 3, None, pbg, nrm.data_ptr(), v, None, None, None, None) != 0
    assert b'gbuffer_normals: R = 10 is larger' in lib.occnerf_last_error()
    assert lib.occnerf_gbuffer_normals(p, q, r, 9, 3, -3, None, pbg, nrm.data_ptr(), v, None, None, None, None) != 0
    assert b'gbuffer_normals: bad sizes' in lib.occnerf_last_error()
    torch.cuda.synchronize()


RENDER_MIN_ALPHA = 0.05


def test_one_rendered_frame():
    """The tpose frame at 48 x 48, N_samples 32, of the seeded amplified checkpoint (run.py `_teacher`'s kind): the renderer's
    depth / alpha through geometry_maps equal the definition on the same arrays, and at least 5 % of the frame's rays carry a
    valid normal at min_alpha = RENDER_MIN_ALPHA.

    Measured on an MI355X: the frame has 2 021 rays; 32 samples of this checkpoint accumulate an alpha of at most 0.314 (mean
    0.020), so at the default min_alpha 0.5 no pixel has a depth (share 0.0).  The share of rays with a valid normal is 0.002 at
    0.3, 0.029 at 0.2, 0.055 at 0.1, 0.129 at 0.05 (depth-valid 0.132) and 0.204 at 0.01; the test uses 0.05, the largest of
    these thresholds that clears the 5 % condition by more than a few pixels."""
    from occnerf_amd import synth
    from occnerf_amd.gbuffer import geometry_maps
    from occnerf_amd.seeded import build_network, frame_to_device
    size = 48
    frame = synth.make_frame(img_size=size, pose72=None)
    data = frame_to_device(frame, DEV)
    net = build_network(seed=1, amplify=True, S=32)
    with torch.no_grad():
        out = net(**data, iter_val=1e7)
    ray_index = torch.from_numpy(np.nonzero(np.asarray(frame['ray_mask']).reshape(-1))[0]).to(DEV)
    got = geometry_maps(size, size, ray_index, data['rays'], out['depth'], out['alpha'], min_alpha=RENDER_MIN_ALPHA,
                        near=data['near'], far=data['far'], bgcolor=(1., 1., 1.))
    torch.cuda.synchronize()
    host = lambda t: t.detach().cpu().numpy()  # noqa: E731
    want = G.geometry_maps(size, size, host(ray_index), host(data['rays']), host(out['depth']), host(out['alpha']),
                           min_alpha=RENDER_MIN_ALPHA, t_range=G.default_t_range(host(data['near']), host(data['far'])))
    compare(got, want, 'rendered tpose frame')
    R = int(ray_index.numel())
    share = float((want['valid'] & 2).astype(bool).sum()) / R
    alpha = host(out['alpha'])
    print(f'\n   tpose {size}^2: {R} rays, alpha max {alpha.max():.4f} mean {alpha.mean():.4f}, depth-valid '
          f'{float((want["valid"] & 1).sum()) / R:.4f}, valid normal {share:.4f} of the rays at min_alpha {RENDER_MIN_ALPHA}')
    assert share >= 0.05, share


_sequence = {}


def sequence_frame(size=48, min_alpha=0.01):
    """The synthetic tpose frame through run.py's own route -- SyntheticFrames, frames_to_device, ShardedRenderer,
    render_sequence -- with the seeded checkpoint run.py loads, N_samples 32: (geometry_maps of what on_frame receives, the
    definition on host copies of the same out['depth'] / out['alpha'] / meta['rays']).  Computed once."""
    if not _sequence:
        from occnerf_amd.gbuffer import geometry_maps
        from occnerf_amd.parallel import ShardedRenderer
        from occnerf_amd.seeded import build_network
        from occnerf_amd.sequence import SyntheticFrames, render_sequence
        net = build_network(seed=0, amplify=False, S=32)
        loader = SyntheticFrames('tpose', img_size=size, device_rays=True)
        seen = []

        def on_frame(out, meta):
            got = geometry_maps(meta['width'], meta['height'], meta['ray_index'], meta['rays'], out['depth'], out['alpha'],
                                min_alpha=min_alpha, near=meta['near'], far=meta['far'], bgcolor=(1., 1., 1.))
            torch.cuda.synchronize()
            host = lambda t: t.detach().cpu().numpy()  # noqa: E731
            want = G.geometry_maps(meta['height'], meta['width'], host(meta['ray_index']), host(meta['rays']), host(out['depth']),
                                   host(out['alpha']), min_alpha=min_alpha,
                                   t_range=G.default_t_range(host(meta['near']), host(meta['far'])))
            want['near_far'] = (host(meta['near']), host(meta['far']))
            seen.append((got, want))

        assert render_sequence(ShardedRenderer(net, torch.device(DEV)), loader, 'tpose', 1e7, on_frame, torch.device(DEV)) == 1
        _sequence['frame'], = seen
    return _sequence['frame']


def test_the_render_sequence_route_equals_the_definition():
    """What run.py's on_frame receives -- the gathered depth and alpha of the ShardedRenderer and the rays render_sequence put
    into meta -- through geometry_maps equals the definition on the same arrays: a wrong or reordered rays tensor in meta would
    turn the normals."""
    got, want = sequence_frame()
    compare(got, want, 'render_sequence tpose frame')
    assert (want['valid'] & 2).astype(bool).sum() > 100


def test_run_py_writes_the_panels_and_the_raw_maps(tmp_path):
    """python run.py --type tpose with show_alpha and the three new keys and geometry.save: the PNG is five panels wide, the
    depth and shaded panels are grey, the first two panels are the PNG of a run without the new keys byte for byte, the raw
    maps and their sidecar are in the sibling folder and equal the definition of the same frame rendered in this process, the
    image folder holds what it held before, and a stale <folder>_geometry of an earlier run is removed with the image folder."""
    from PIL import Image
    size = 48
    base = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', CFG, '--type', 'tpose', 'render_size', str(size),
            'N_samples', '32', 'show_alpha', 'True']
    env = {**os.environ, 'PYTHONPATH': ROOT}
    folder = os.path.join('experiments', 'occnerf', 'synthetic', 'capsule_body', 'occnerf', 'seeded')
    runs = {}
    for tag, extra in (('plain', []), ('geometry', ['show_depth', 'True', 'show_normal', 'True', 'show_shaded', 'True',
                                                    'geometry.save', 'True', 'geometry.min_alpha', '0.01'])):
        cwd = tmp_path / tag
        cwd.mkdir()
        if tag == 'plain':                                         # an earlier run's raw maps: removed with the image folder
            os.makedirs(cwd / folder / 'tpose_geometry')
            (cwd / folder / 'tpose_geometry' / '000000.npz').write_bytes(b'stale')
        out = subprocess.run(base + extra, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=170)
        assert out.returncode == 0, out.stderr[-3000:]
        runs[tag] = cwd / folder
    for tag in runs:
        assert sorted(os.listdir(runs[tag] / 'tpose')) == ['000000.png']
    assert sorted(os.listdir(runs['plain'])) == ['tpose']
    assert sorted(os.listdir(runs['geometry'])) == ['tpose', 'tpose_geometry']
    plain = np.asarray(Image.open(runs['plain'] / 'tpose' / '000000.png'))
    img = np.asarray(Image.open(runs['geometry'] / 'tpose' / '000000.png'))
    assert plain.shape == (size, 2 * size, 3) and img.shape == (size, 5 * size, 3)
    assert np.array_equal(img[:, :2 * size], plain)
    depth, normal, shaded = (img[:, k * size:(k + 1) * size] for k in (2, 3, 4))
    for grey in (depth, shaded):
        assert (grey[..., 0] == grey[..., 1]).all() and (grey[..., 0] == grey[..., 2]).all()
    assert sorted(os.listdir(runs['geometry'] / 'tpose_geometry')) == ['000000.npz', 'geometry.json']
    import json
    side = json.load(open(runs['geometry'] / 'tpose_geometry' / 'geometry.json'))
    assert side['min_alpha'] == 0.01 and 'ray PARAMETER' in side['t'] and 't * |d|' in side['t']      # the unit is stated
    assert 'not rotated' in side['normal'] and side['depth_range'].startswith('per frame')
    z = np.load(runs['geometry'] / 'tpose_geometry' / '000000.npz')
    assert sorted(z.files) == ['normal', 't', 't_range', 'valid']
    assert (z['t'].shape, z['t'].dtype) == ((size, size), np.float32)
    assert (z['normal'].shape, z['normal'].dtype) == ((size, size, 3), np.float32)
    assert (z['valid'].shape, z['valid'].dtype) == ((size, size), np.uint8)
    assert (z['t_range'].shape, z['t_range'].dtype) == ((2,), np.float32) and z['t_range'][0] < z['t_range'][1]
    # the panels are the raw maps' own: white where a map is not valid, the definition's quantisation where it is
    dv, nv = (z['valid'] & 1).astype(bool), (z['valid'] & 2).astype(bool)
    assert (depth[~dv] == 255).all() and (normal[~nv] == 255).all() and (shaded[~nv] == 255).all()
    lo, hi = z['t_range']
    assert np.array_equal(depth[..., 0][dv], G.to_8b(G.clamp01((hi - z['t']) / (hi - lo)))[dv])
    assert np.array_equal(normal[nv], G.to_8b(np.float32(0.5) * z['normal'] + np.float32(0.5))[nv])
    assert dv.any() and set(np.unique(z['valid']).tolist()) <= {0, 1, 3}
    # ... and the maps are the definition's of the same frame rendered in this process through the same route (the renderer
    # is deterministic): run.py handed geometry_maps the frame's own rays, depth and alpha in the same order
    _, want = sequence_frame(size, 0.01)
    for k in ('t', 'normal', 'valid'):
        same_bytes(z[k], want[k], f'run.py npz {k} vs the definition of the in-process frame')
    same_bytes(z['t_range'], np.asarray(G.default_t_range(*want['near_far']), np.float32), 'run.py npz t_range')
