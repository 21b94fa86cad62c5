"""GPU: the tangent-space normal map of the exported mesh.  csrc/mesh_normal.hip against the numpy
definition (tests/mesh_normal_restatement.py) -- the atlas, the offsets, the flags and the normals as bit patterns, the two lit
panels byte for byte on the device's own raster keys --, the plane, sphere and flag cases of
tests/test_mesh_normal_restatement.py through the kernel, and run.py --type mesh with mesh_normal.enable end to end."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_normal_restatement as nr
from tests import mesh_raster_restatement as mrr
from tests import mesh_restatement as mr
from tests import mesh_texture_restatement as tex
from tests import test_mesh_normal_restatement as cpu
from tests.gpu_util import DEV, T, build_network, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _device_bake(ops, verts, faces, normals, tangents, creased, pts, n, field, lo, h, level, S, twice=False):
    size = len(faces)
    C, _, W, H, P = tex.layout(size, n)
    args = (T(verts), T(normals), T(faces), T(tangents), T(np.asarray(creased).astype(np.uint8)), T(pts), n, C)
    out = []
    for _ in range(2 if twice else 1):
        atlas = T(np.broadcast_to(nr.FLAT_CODE, (H, W, 3)).copy())
        got = ops.mesh_normal_bake(*args, atlas, T(field), lo, h, level, S)
        assert got[0] is atlas and got[1].dtype == torch.float32 and got[2].dtype == torch.uint8 and tuple(got[3].shape) == (size, P, 3)
        out.append({k: v.cpu().numpy() for k, v in zip(('atlas', 'offset', 'flags', 'normal'), got)})
    if twice:
        for k in out[0]:
            assert out[0][k].tobytes() == out[1][k].tobytes(), k                # the same bytes again
    return out[0]


def _kernel(ops):
    return lambda *a: _device_bake(ops, *a)


def _compare(got, want, name):
    for k in ('atlas', 'offset', 'flags', 'normal'):
        same(_bits(got[k]), _bits(want[k]), f'{name}: {k}')


@pytest.mark.parametrize('n', nr.CELLS)
def test_bake_is_the_definition(ops, n):
    """Every T x both fields x S = 1, 2, 64: the four outputs as bit patterns."""
    plane = nr.plane_field()[:4]
    sphere = nr.sphere_field(17) + (np.float32(0.0),)
    flagged = set()
    for size in nr.T_SIZES:
        verts, faces = tex.welded_mesh(size, seed=n)
        for name, (field, lo, h, level), shift in (('plane', plane, 0.0), ('sphere', sphere, nr.SPHERE_SHIFT)):
            v = (verts + np.float32(shift)).astype(np.float32)
            normals, tangents, creased, pts = cpu._inputs(v, faces, n)
            for S in (1, 2, 64):
                want = nr.bake(v, faces, normals, tangents, creased, pts, n, field, lo, h, level, S)
                got = _device_bake(ops, v, faces, normals, tangents, creased, pts, n, field, lo, h, level, S, twice=S == 2)
                _compare(got, want, f'{name} T={size} n={n} S={S}')
                flagged |= set(np.unique(want['flags']).tolist())
    assert {0, nr.NO_CROSSING, nr.FLAT} <= flagged
    torch.cuda.synchronize()


def test_bake_without_triangles_and_with_a_bad_index(ops):
    field, lo, h, level = nr.plane_field()[:4]
    n = 5
    verts, faces = tex.welded_mesh(3, seed=n)
    normals, tangents, creased, pts = cpu._inputs(verts, faces, n)
    atlas = T(np.broadcast_to(nr.FLAT_CODE, (n, n, 3)).copy())
    empty = ops.mesh_normal_bake(T(verts), T(normals), T(faces[:0]), T(tangents[:0]), T(creased[:0].astype(np.uint8)), T(pts[:0]), n, 1,
                                 atlas, T(field), lo, h, level, 2)
    assert empty[0] is atlas and tuple(empty[1].shape) == (0, 10) and tuple(empty[3].shape) == (0, 10, 3)
    assert (atlas.cpu().numpy() == nr.FLAT_CODE).all()
    C, _, W, H, _ = tex.layout(3, n)
    for index in (len(verts), -1):
        bad = faces.copy()
        bad[-1, 2] = index                                       # never used as an address
        with pytest.raises(RuntimeError, match=f'mesh_normal_bake: a face index lies outside \\[0, {len(verts)}\\)'):
            ops.mesh_normal_bake(T(verts), T(normals), T(bad), T(tangents), T(creased.astype(np.uint8)), T(pts), n, C,
                                 T(np.zeros((H, W, 3), np.uint8)), T(field), lo, h, level, 2)
    with pytest.raises(RuntimeError, match='mesh_normal_bake: S = 65 steps outside 1..64'):
        ops.mesh_normal_bake(T(verts), T(normals), T(faces), T(tangents), T(creased.astype(np.uint8)), T(pts), n, C,
                             T(np.zeros((H, W, 3), np.uint8)), T(field), lo, h, level, 65)
    with pytest.raises(RuntimeError, match='mesh_normal_bake: an atlas of .* does not hold T = 3 triangles'):
        ops.mesh_normal_bake(T(verts), T(normals), T(faces), T(tangents), T(creased.astype(np.uint8)), T(pts), n, C,
                             T(np.zeros((H - 1, W, 3), np.uint8)), T(field), lo, h, level, 2)
    torch.cuda.synchronize()


def test_flags_through_the_kernel(ops):
    got, want = cpu.flag_cases(_kernel(ops)), cpu.flag_cases()
    cpu.check_flags(got)
    for k in want:
        same(got[k], want[k], k)


@pytest.mark.parametrize('n', nr.CELLS)
def test_plane_through_the_kernel(ops, n):
    for size, S in ((3, 2), (65, 2), (257, 2), (64, 1)):
        count, worst, ratio, _ = cpu.plane_case(size, n, S, _kernel(ops))
        print(f'\n   plane T = {size} n = {n} S = {S}: {count} unflagged texels, max |N_f - truth| = {worst:.3g}, '
              f'decoded angle / bound = {ratio:.4f}')
        assert count > 0 and ratio <= 1.0


def test_sphere_through_the_kernel(ops):
    r, want = cpu.sphere_case(_kernel(ops)), cpu.sphere_case()
    print(f"\n   sphere: largest |s| = {r['offset_coarse_voxels']:.3f} coarse voxels; the decoded map {r['mapped_deg'][0]:.3f} deg mean "
          f"from the radial direction, the interpolated vertex normals {r['geometry_deg'][0]:.3f}")
    assert r['mapped_deg'][0] < r['geometry_deg'][0]
    assert r['flat'] == want['flat'] and np.array_equal(r['mapped_deg'], want['mapped_deg'])


# ------------------------------------------------------------------ the lit resolve
def _keys(ops, c):
    """The device rasteriser's keys of a raster case (tests/test_p_mesh_raster.py holds them to the definition)."""
    pos, faces = T(c['pos']), T(c['faces'])
    xy, z, vflag = ops.mesh_project(pos, c['K'], c['E'])
    keys, _ = ops.mesh_raster(faces, xy, z, vflag, c['H'], c['W'])
    return faces, xy, z, keys


@pytest.mark.parametrize('name', ('grid', 'ties', 'mixed', 'random257'))
def test_resolve_lit(ops, name):
    for n in (4, 8):
        c, normals, tangents, atlas, C, M = cpu.lit_case(name, n)
        if n == 4:
            faces, xy, z, keys = _keys(ops, c)
            k_np = keys.cpu().numpy().view(np.uint64)
            assert (k_np != mrr.EMPTY_KEY).sum() > 50
            assert np.array_equal(M, ops.mesh_ray_matrix(c['K'], c['E']))
        want = nr.resolve_lit(k_np, c['faces'], xy.cpu().numpy(), z.cpu().numpy(), normals, tangents, atlas, n, C, M, (255, 0, 255))
        got = ops.mesh_resolve_lit(keys, faces, xy, z, T(normals), T(tangents), T(atlas), n, C, M, (255, 0, 255))
        for g, w, panel in zip(got, want, ('shade_geometry', 'shade_mapped')):
            assert g.dtype == torch.uint8 and tuple(g.shape) == (c['H'], c['W'], 3)
            same(g.cpu().numpy(), w, f'{name} n={n} {panel}')
        again = ops.mesh_resolve_lit(keys, faces, xy, z, T(normals), T(tangents), T(atlas), n, C, M, (255, 0, 255))
        assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
        assert not torch.equal(got[0], got[1])
        # the flat atlas adds nothing: the two panels are the same bytes
        flat = T(np.broadcast_to(nr.FLAT_CODE, atlas.shape).copy())
        geo, mapped = ops.mesh_resolve_lit(keys, faces, xy, z, T(normals), T(tangents), flat, n, C, M, (255, 0, 255))
        assert torch.equal(geo, got[0]) and torch.equal(mapped, geo)
    torch.cuda.synchronize()


def test_resolve_lit_without_a_hit(ops):
    c = mrr.case_offscreen()
    faces, xy, z, keys = _keys(ops, c)
    normals = nr.vertex_normals(c['pos'], c['faces'])
    tangents, _ = nr.corner_tangents(c['pos'], c['faces'], normals)
    atlas, C = tex.random_atlas(len(c['faces']), 8)
    M = nr.ray_matrix(c['K'], c['E'])
    for f, t in ((faces, tangents), (faces[:0].contiguous(), tangents[:0])):
        geo, mapped = ops.mesh_resolve_lit(keys, f, xy, z, T(normals), T(t), T(atlas), 8, C, M, (1, 2, 3))
        assert (geo.cpu().numpy() == np.array([1, 2, 3], np.uint8)).all() and torch.equal(geo, mapped)
    with pytest.raises(RuntimeError, match='mesh_resolve_lit: an atlas of .* does not hold'):
        ops.mesh_resolve_lit(keys, faces, xy, z, T(normals), T(tangents), T(atlas), 8, C + 1, M, (1, 2, 3))
    with pytest.raises(RuntimeError, match=r'mesh_resolve_lit: vnormals \[120,3\] and tangents \[40,3,4\]'):
        ops.mesh_resolve_lit(keys, faces, xy, z, T(normals), T(tangents[:5]), T(atlas), 8, C, M, (1, 2, 3))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ end to end
def _run_py(tmp, *extra):
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'),
           '--type', 'mesh', 'mesh.resolution', '16', 'N_samples', '16'] + list(extra)
    os.makedirs(str(tmp), exist_ok=True)
    out = subprocess.run(cmd, cwd=str(tmp), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return tmp / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'mesh'


def _setup(tmp_path):
    from occnerf_amd import mesh
    from occnerf_amd.dataset import PreparedDataset
    path = str(tmp_path / 'ds')
    mrr.load_tool().make_dataset(path, frames=4, width=64, height=64, seed=0)
    net, _ = build_network(0, False, S=32, non_rigid=True)
    ds = PreparedDataset(path, device=None)
    bmin, bmax = ds.cnl_bbox_min_xyz, ds.cnl_bbox_max_xyz
    field, _, _ = mesh.density_grid(net, bmin, bmax, 16)
    level = float(field.median().item())
    common = ('train.dataset_path', path, 'resize_img_scale', '1.0', 'mesh.level', repr(level), 'mesh_texture.enable', 'True',
              'mesh_texture.cell', '5', 'mesh_rig.enable', 'True', 'mesh_rig.frames', '[0, 3]', 'mesh_view.frames', '[0, 1]',
              'bgcolor', '[255.0, 255.0, 255.0]')
    return net, ds, path, bmin, bmax, level, common


def test_run_py_writes_the_normal_map(ops, tmp_path):
    """run.py --type mesh with mesh_texture.enable and mesh_normal.enable on a tool-made dataset of 64 x 64 frames, at the
    16-grid's median level, cell 5, a bake grid of 32, the rig of frames 0 and 3 and the views of frames 0 and 1."""
    from PIL import Image

    from occnerf_amd import mesh
    net, ds, path, bmin, bmax, level, common = _setup(tmp_path)
    out = _run_py(tmp_path / 'run', *common, 'mesh_normal.enable', 'True', 'mesh_normal.resolution', '32')
    assert sorted(os.listdir(out)) == ['mesh.json', 'mesh.ply', 'rig.json', 'rigged.glb', 'texture.json', 'texture.png',
                                       'texture_normal.json', 'texture_normal.png', 'view', 'view.json']
    canon = mr.parse_ply((out / 'mesh.ply').read_bytes())
    verts = np.ascontiguousarray(np.stack([canon['x'], canon['y'], canon['z']], 1))
    faces = np.ascontiguousarray(canon['faces'].astype(np.int32))
    size, n = len(faces), 5
    info = json.loads((out / 'texture_normal.json').read_text())
    h = json.loads((out / 'mesh.json').read_text())['h']
    C, R, W, H, P = tex.layout(size, n)
    assert [info[k] for k in ('n', 'C', 'R', 'W', 'H', 'triangles', 'texels')] == [n, C, R, W, H, size, size * P]
    assert info['resolution'] == 32 and info['cage'] == h and info['h_f'] == h / 2 and info['S'] == 4 and info['samples_per_texel'] == 15
    assert sum(info['texels_per_flag'][k] for k in ('none',)) > 0 and set(info['seconds']) == {'grid', 'tangents', 'points', 'bake', 'write'}
    png = (out / 'texture_normal.png').read_bytes()
    disk = np.asarray(Image.open(io.BytesIO(png)).convert('RGB'))
    assert disk.shape == (H, W, 3) and info['bytes']['png'] == len(png)
    atlas, offset, flags, stats = mesh.bake_normal_map(net, T(verts), faces, n, level, bmin, bmax, 32, h)
    same(disk, atlas.cpu().numpy(), 'texture_normal.png against bake_normal_map here')
    assert stats['texels_per_flag'] == info['texels_per_flag'] and stats['creased_triangles'] == info['creased_triangles']
    assert info['texels_per_flag']['none'] == int((flags == 0).sum().item())
    # rigged.glb: TANGENT, two images, the normal texture
    doc, buf, att, image, image_n = nr.read_normal_mapped((out / 'rigged.glb').read_bytes())
    assert np.array_equal(image_n, disk) and np.array_equal(image, np.asarray(Image.open(out / 'texture.png').convert('RGB')))
    assert att['TANGENT'].tobytes() == stats['tangents'].tobytes() and att['POSITION'].tobytes() == verts[faces.reshape(-1)].tobytes()
    assert len(doc['skins']) == 1 and len(doc['animations']) == 1 and json.loads((out / 'rig.json').read_text())['normal_mapped'] is True
    # the views: [vertex colours | textured | geometry shade | mapped shade | photograph]
    views = json.loads((out / 'view.json').read_text())
    for row in views['frames']:
        img = np.array(Image.open(out / 'view' / (row['name'] + '.png')))
        assert img.shape == (64, 320, 3) and row['covered'] > 50 and row['lit_mean_abs_diff'] is not None
        geo, mapped = img[:, 128:192], img[:, 192:256]
        assert (geo[..., 0] == geo[..., 1]).all() and (geo != 255).any() and not np.array_equal(geo, mapped)
        same(img[:, 256:], ds.truth_u8(row['frame']), 'the photograph')


def test_run_py_without_the_keys_writes_what_it_wrote(ops, tmp_path):
    """Without the mesh_normal keys: mesh.ply, texture.png, rigged.glb and the views of run.py are the bytes of export_mesh,
    export_texture, export_rig and export_views called here without the new arguments."""
    from occnerf_amd import mesh, mesh_view
    net, ds, path, bmin, bmax, level, common = _setup(tmp_path)
    out = _run_py(tmp_path / 'run', *common)
    assert sorted(os.listdir(out)) == ['mesh.json', 'mesh.ply', 'rig.json', 'rigged.glb', 'texture.json', 'texture.png', 'view', 'view.json']
    here, kept = tmp_path / 'here', {}
    mesh.export_mesh(net, str(here), bmin, bmax, resolution=16, level=level, keep=kept)
    mesh.export_texture(net, str(here), kept, {'enable': True, 'cell': 5, 'fill': [0, 0, 0]})
    mesh.export_rig(net, str(here), kept, mesh.PoseFrames(path), {**mesh.RIG_DEFAULTS, 'enable': True, 'frames': [0, 3]},
                    texture=kept['texture'])
    views = mesh_view.export_views(net, str(here), kept, ds, [0, 1], texture=kept['texture'])
    assert 'lit_mean_abs_diff' not in views['frames'][0] and 'normal_mapped' not in json.loads((out / 'rig.json').read_text())
    names = ['mesh.ply', 'texture.png', 'rigged.glb'] + [os.path.join('view', r['name'] + '.png') for r in views['frames']]
    for name in names:
        assert (out / name).read_bytes() == (here / name).read_bytes(), name
    tex.read_textured((out / 'rigged.glb').read_bytes())
