"""GPU: the texture of the exported mesh.  csrc/mesh_texture.hip against the numpy definition
(tests/mesh_texture_restatement.py) -- points as bit patterns, atlas and image bytes EQUAL --, the affine bound of
tests/test_mesh_texture_restatement.py through the three kernels, and run.py --type mesh with mesh_texture.enable end to end."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import gltf_restatement as gr
from tests import mesh_raster_restatement as mrr
from tests import mesh_restatement as mr
from tests import mesh_texture_restatement as tex
from tests import test_mesh_texture_restatement as cpu
from tests.gpu_util import DEV, T, build_network, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = (9, 200, 31)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize('n', tex.CELLS)
def test_texel_points(ops, n):
    P = n * (n - 1) // 2
    for size in tex.T_SIZES:
        verts, faces = tex.welded_mesh(size, seed=n)
        want, status = tex.texel_points(verts, faces, n)
        assert status == 0
        v, f = T(verts), T(faces)
        got = ops.mesh_texel_points(v, f, n)
        assert got.dtype == torch.float32 and tuple(got.shape) == (size, P, 3) and got.is_cuda
        same(_bits(got.cpu().numpy()), _bits(want), f'texel points T={size} n={n}')
        assert torch.equal(got.view(torch.int32), ops.mesh_texel_points(v, f, n).view(torch.int32))           # the same bytes again
    empty = ops.mesh_texel_points(v, f[:0].contiguous(), n)
    assert tuple(empty.shape) == (0, P, 3)
    bad = faces.copy()
    bad[-1, 2] = verts.shape[0]                                  # one past the last vertex: never used as an address
    with pytest.raises(RuntimeError, match=f'mesh_texel_points: a face index lies outside \\[0, {verts.shape[0]}\\)'):
        ops.mesh_texel_points(v, T(bad), n)
    bad[-1, 2] = -1
    with pytest.raises(RuntimeError, match='mesh_texel_points: a face index lies outside'):
        ops.mesh_texel_points(v, T(bad), n)
    torch.cuda.synchronize()


@pytest.mark.parametrize('n', tex.CELLS)
def test_texture_fill(ops, n):
    """Values below 0, above 1 and NaN; odd T leaves the upper half of the last cell, T = 65 and 257 unused cells in the last
    row: all of them keep the caller's colour."""
    for size in tex.T_SIZES:
        C, R, W, H, P = tex.layout(size, n)
        rgb = tex.fill_input(size, n)
        want = np.empty((H, W, 3), np.uint8)
        want[:] = FILL
        tex.fill(rgb, size, n, C, want)
        atlas = T(np.broadcast_to(np.array(FILL, np.uint8), (H, W, 3)).copy())
        got = ops.mesh_texture_fill(T(rgb), size, n, C, atlas)
        assert got is atlas
        same(got.cpu().numpy(), want, f'atlas T={size} n={n}')
        unowned = H * W - size * P
        assert int((want == np.array(FILL, np.uint8)).all(-1).sum()) >= unowned > 0
    assert C * R > (size + 1) // 2 and size % 2 == 1            # the last size: unused cells and a half-empty one
    with pytest.raises(RuntimeError, match='mesh_texture_fill: an atlas of .* does not hold T = 257 triangles'):
        ops.mesh_texture_fill(T(rgb), size, n, C, atlas[:H - n].contiguous())
    with pytest.raises(RuntimeError, match='mesh_texture_fill: rgb must be float32'):
        ops.mesh_texture_fill(T(rgb[:-1]), size, n, C, atlas)
    torch.cuda.synchronize()


def _keys(ops, c):
    """The device rasteriser's keys of a raster case (tests/test_p_mesh_raster.py holds them to the definition)."""
    pos, faces = T(c['pos']), T(c['faces'])
    xy, z, vflag = ops.mesh_project(pos, c['K'], c['E'])
    keys, counts = ops.mesh_raster(faces, xy, z, vflag, c['H'], c['W'])
    return pos, faces, xy, z, vflag, keys, counts


@pytest.mark.parametrize('name', ('grid', 'ties', 'mixed', 'random257'))
def test_resolve_textured(ops, name):
    c = mrr.case_random(257) if name == 'random257' else mrr.CASES[name]()
    pos, faces, xy, z, vflag, keys, _ = _keys(ops, c)
    k_np = keys.cpu().numpy().view(np.uint64)
    assert (k_np != mrr.EMPTY_KEY).sum() > 50
    for n in (4, 8):
        atlas, C = tex.random_atlas(len(c['faces']), n)
        want = tex.resolve_textured(k_np, c['faces'], xy.cpu().numpy(), z.cpu().numpy(), atlas, n, C, (255, 0, 255))
        got = ops.mesh_resolve_textured(keys, faces, xy, z, T(atlas), n, C, (255, 0, 255))
        assert got.dtype == torch.uint8 and tuple(got.shape) == (c['H'], c['W'], 3)
        same(got.cpu().numpy(), want, f'{name} n={n}')
        assert torch.equal(got, ops.mesh_resolve_textured(keys, faces, xy, z, T(atlas), n, C, (255, 0, 255)))
    torch.cuda.synchronize()


def test_resolve_textured_without_a_hit(ops):
    c = mrr.case_offscreen()
    _, faces, xy, z, _, keys, _ = _keys(ops, c)
    atlas, C = tex.random_atlas(len(c['faces']), 8)
    got = ops.mesh_resolve_textured(keys, faces, xy, z, T(atlas), 8, C, (1, 2, 3)).cpu().numpy()
    assert (got == np.array([1, 2, 3], np.uint8)).all()
    none = ops.mesh_resolve_textured(keys, faces[:0].contiguous(), xy, z, T(atlas), 8, C, (1, 2, 3)).cpu().numpy()
    assert (none == np.array([1, 2, 3], np.uint8)).all()
    with pytest.raises(RuntimeError, match='mesh_resolve_textured: an atlas of .* does not hold'):
        ops.mesh_resolve_textured(keys, faces, xy, z, T(atlas), 8, C + 1, (1, 2, 3))
    torch.cuda.synchronize()


def test_an_affine_colour_through_the_definitions_sampler(ops):
    """The CPU test's case with the two baking kernels in place of the definition's."""
    def points(v, f, n):
        return ops.mesh_texel_points(T(v), T(f), n).cpu().numpy()

    def fill(rgb, size, n, C, atlas):
        return ops.mesh_texture_fill(T(rgb), size, n, C, T(atlas)).cpu().numpy()
    for n in (4, 8):
        worst, bound = cpu.affine_case(9, n, points, fill)
        print(f'\n   n = {n}: max |byte - 255 c(p)| = {worst:.4f}, bound {bound:.6f}')
        assert worst <= bound


@pytest.mark.parametrize('name,n', (('blobs', 8), ('grid', 5)))
def test_an_affine_colour_through_the_three_kernels(ops, name, n):
    """c(p) = a . p + b in [0.1, 0.9] on every texel point of a raster case's mesh, baked by mesh_texel_points and
    mesh_texture_fill, drawn by mesh_resolve_textured: at every covered pixel |byte - 255 c(p)| <= 1.5 + 255 eps, the bound of
    tests/mesh_texture_restatement.py affine_bound, with p the winner's perspective-correct point in float64."""
    c = mrr.CASES[name]()
    pos, faces, xy, z, vflag, keys, counts = _keys(ops, c)
    size = len(c['faces'])
    C, _, W, H, P = tex.layout(size, n)
    pts = ops.mesh_texel_points(pos, faces, n)
    a, b = tex.affine_colour(pts.cpu().numpy(), seed=n)
    colour = (pts.cpu().numpy().astype(np.float64).reshape(-1, 3) @ a.T + b).astype(np.float32)
    atlas = ops.mesh_texture_fill(T(colour), size, n, C, torch.zeros(H, W, 3, device=DEV, dtype=torch.uint8))
    got = ops.mesh_resolve_textured(keys, faces, xy, z, atlas, n, C, (0, 0, 0)).cpu().numpy().astype(np.float64)
    _, tri, _, _ = ops.mesh_resolve(keys, counts, faces, xy, z, vflag, T(mrr.vertex_colors(len(c['pos']))), (0, 0, 0))
    tri, xy_np, z_np = tri.cpu().numpy(), xy.cpu().numpy(), z.cpu().numpy()
    _, idx, A = mrr.setup(c['faces'], xy_np, vflag.cpu().numpy())
    bound, worst, hits = tex.affine_bound(a, pts.cpu().numpy()), 0.0, 0
    for i, j in zip(*np.nonzero(tri >= 0)):
        t = int(tri[i, j])
        v = idx[t]
        e, _ = mrr.edges(xy_np[v, 0].astype(np.int64), xy_np[v, 1].astype(np.int64), np.int64(256 * j), np.int64(256 * i))
        q, iz = mrr.inverse_depth(e, A[t], z_np[v])
        p = sum((q[k] / iz) * c['pos'][v[k]].astype(np.float64) for k in range(3))
        worst = max(worst, float(np.abs(got[i, j] - 255.0 * (a @ p + b)).max()))
        hits += 1
    print(f'\n   {name} n = {n}: {hits} pixels, max |byte - 255 c(p)| = {worst:.4f}, bound {bound:.6f}')
    assert hits > 200 and worst <= bound


def test_export_views_adds_the_textured_panel(ops, tmp_path):
    """export_mesh, export_texture and export_views in this process on the 16-grid's median level and a tool-made dataset of
    64 x 64 frames: every view is [vertex colours | textured | photograph], the textured panel is the definition's image of the
    posed mesh and the atlas, and view.json reports the panels' mean absolute difference over the covered pixels."""
    from PIL import Image

    from occnerf_amd import mesh, mesh_view
    from occnerf_amd.dataset import PreparedDataset
    net, _ = build_network(0, False, S=32, non_rigid=True)
    path = str(tmp_path / 'ds')
    mrr.load_tool().make_dataset(path, frames=3, width=64, height=64, seed=0)
    ds = PreparedDataset(path, device=None)
    bmin, bmax = ds.cnl_bbox_min_xyz, ds.cnl_bbox_max_xyz
    field, _, _ = mesh.density_grid(net, bmin, bmax, 16)
    out, kept, n = str(tmp_path / 'mesh'), {}, 5
    mesh.export_mesh(net, out, bmin, bmax, resolution=16, level=float(field.median().item()), keep=kept)
    mesh.export_texture(net, out, kept, {'enable': True, 'cell': n, 'fill': [3, 4, 5]})
    info = mesh_view.export_views(net, out, kept, ds, [0, 2], texture=kept['texture'])
    faces, colors = T(kept['faces']), T(kept['colors'])
    atlas = kept['texture']['atlas'].cpu().numpy()
    assert (atlas == np.array([3, 4, 5], np.uint8)).all(-1).any()
    for row in info['frames']:
        f, fr = ds.frames[row['frame']], ds.host_constants(row['frame'])
        data = {k: T(fr[k]) for k in mesh._POSE_KEYS}
        data.update({k: np.asarray(fr[k], dtype=np.float32) for k in ('cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz')})
        p = mesh.pose_mesh(net, kept['verts'], data)[0]
        r = mesh_view.rasterize(p, faces, colors, f['K'], f['E'], 64, 64, (255., 255., 255.), texture=kept['texture'])
        xy, z, vflag = r['xy'].cpu().numpy(), r['z'].cpu().numpy(), r['vflag'].cpu().numpy()
        keys, _ = mrr.raster_keys(kept['faces'], xy, z, vflag, 64, 64)
        want = tex.resolve_textured(keys, kept['faces'], xy, z, atlas, n, kept['texture']['C'], (255, 255, 255))
        img = np.array(Image.open(os.path.join(out, 'view', row['name'] + '.png')))
        assert img.shape == (64, 192, 3)
        same(img[:, :64], r['rgb'].cpu().numpy(), 'the vertex-colour panel')
        same(img[:, 64:128], want, 'the textured panel')
        same(img[:, 128:], ds.truth_u8(row['frame']), 'the photograph')
        cover = r['cover'].cpu().numpy() > 0
        assert cover.sum() == row['covered'] > 50
        diff = np.abs(img[:, 64:128].astype(np.int64) - img[:, :64].astype(np.int64))[cover].mean()
        print(f"\n   {row['name']}: {row['covered']} pixels, textured against vertex colours: mean |difference| = {diff:.3f} bytes")
        assert abs(row['textured_mean_abs_diff'] - float(diff)) <= 1e-9
    plain = mesh_view.export_views(net, str(tmp_path / 'plain'), kept, ds, [0])
    assert 'textured_mean_abs_diff' not in plain['frames'][0]
    assert np.array(Image.open(str(tmp_path / 'plain' / 'view' / (plain['frames'][0]['name'] + '.png')))).shape == (64, 128, 3)


# ------------------------------------------------------------------ end to end
def _run_py(tmp, *extra):
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'),
           '--type', 'mesh', 'mesh.resolution', '16', 'N_samples', '16'] + list(extra)
    os.makedirs(str(tmp), exist_ok=True)
    out = subprocess.run(cmd, cwd=str(tmp), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return tmp / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'mesh'


def test_run_py_writes_the_texture(ops, tmp_path):
    """run.py --type mesh mesh.resolution 16 mesh_texture.enable True mesh_texture.cell 5 with the rig of frames [0, 3], at the
    grid's median density (the seeded weights put no surface at the default level); then the same without the texture keys,
    and the texture without the rig."""
    from PIL import Image

    from occnerf_amd import mesh
    from tests import mesh_pose_restatement as mp
    net, _ = build_network(0, False, S=32, non_rigid=True)
    fr = mp.synthetic_frame(0)
    bmin, bsc = fr['cnl_bbox_min_xyz'], fr['cnl_bbox_scale_xyz']
    bmax = (np.asarray(bmin, np.float32) + np.float32(2.0) / np.asarray(bsc, np.float32)).astype(np.float32)
    field, _, _ = mesh.density_grid(net, bmin, bmax, 16)
    level = repr(float(field.median().item()))
    rig = ('mesh_rig.enable', 'True', 'mesh_rig.frames', '[0, 3]')
    both = _run_py(tmp_path / 'both', 'mesh.level', level, 'mesh_texture.enable', 'True', 'mesh_texture.cell', '5', *rig)
    plain = _run_py(tmp_path / 'plain', 'mesh.level', level, *rig)
    static = _run_py(tmp_path / 'static', 'mesh.level', level, 'mesh_texture.enable', 'True', 'mesh_texture.cell', '5')
    assert sorted(os.listdir(both)) == ['mesh.json', 'mesh.ply', 'rig.json', 'rigged.glb', 'texture.json', 'texture.png']
    assert sorted(os.listdir(plain)) == ['mesh.json', 'mesh.ply', 'rig.json', 'rigged.glb']
    assert sorted(os.listdir(static)) == ['mesh.json', 'mesh.ply', 'texture.json', 'texture.png', 'textured.glb']
    blob = (both / 'mesh.ply').read_bytes()
    assert blob == (plain / 'mesh.ply').read_bytes() == (static / 'mesh.ply').read_bytes()
    canon = mr.parse_ply(blob)
    verts = np.ascontiguousarray(np.stack([canon['x'], canon['y'], canon['z']], 1))
    faces = np.ascontiguousarray(canon['faces'].astype(np.int32))
    colors = np.stack([canon['red'], canon['green'], canon['blue']], 1)
    size, n = faces.shape[0], 5
    assert size > 100 and verts.shape[0] > 100
    # the atlas: its size is the sidecar's, its corner texels are the vertex colours of mesh.ply
    info = json.loads((both / 'texture.json').read_text())
    C, R, W, H, P = tex.layout(size, n)
    assert [info[k] for k in ('n', 'C', 'R', 'W', 'H', 'triangles', 'texels_queried')] == [n, C, R, W, H, size, size * P]
    assert info['unowned_share'] == 1.0 - float(size * P) / float(W * H) and info['fill'] == [0, 0, 0]
    assert set(info['seconds']) == {'points', 'colour', 'fill', 'write'} and set(info['bytes']) == {'points', 'colours', 'atlas', 'png'}
    edge = np.concatenate([np.linalg.norm(verts[faces[:, a]].astype(np.float64) - verts[faces[:, b]].astype(np.float64), axis=1)
                           for a, b in ((0, 1), (1, 2), (2, 0))])
    assert info['texel_edge_m'] == {'mean': float(edge.mean()) / 2, 'max': float(edge.max()) / 2}
    png = (both / 'texture.png').read_bytes()
    atlas = np.asarray(Image.open(io.BytesIO(png)).convert('RGB'))
    assert atlas.shape == (H, W, 3) and info['bytes']['png'] == len(png) and png == (static / 'texture.png').read_bytes()
    corner = tex.corner_texels(size, n, C)
    same(atlas[corner[..., 1], corner[..., 0]], colors[faces], 'corner texels against the vertex colours of mesh.ply')
    own = np.zeros((H, W), bool)
    for t in range(size):
        x, y = tex.atlas_position(t, tex.owned(n), n, C)
        own[y, x] = True
    assert (atlas[~own] == 0).all()
    # rigged.glb with the texture: unwelded, the image inside
    doc, buf, att, idx, image = tex.read_textured((both / 'rigged.glb').read_bytes())
    assert att['POSITION'].tobytes() == verts[faces.reshape(-1)].tobytes() and np.array_equal(image, atlas)
    assert att['TEXCOORD_0'].tobytes() == mesh.texture_uv(size, n).tobytes() and len(doc['skins']) == 1 and len(doc['animations']) == 1
    rig_json = json.loads((both / 'rig.json').read_text())
    assert rig_json['textured'] is True and rig_json['unwelded_vertices'] == 3 * size and rig_json['vertices'] == verts.shape[0]
    # without the keys: the files of the parent commit -- the writer's default path (the CPU test pins its bytes) on the
    # module's own arrays
    assert cpu.write_recorded(tmp_path / 'recorded') == [cpu.PLAIN_SHA256, cpu.FULL_SHA256]
    kept = {'verts': T(verts), 'faces': faces, 'colors': colors}
    here = mesh.export_rig(net, str(tmp_path / 'here'), kept, mesh.PoseFrames(None, total_frames=100),
                           {**mesh.RIG_DEFAULTS, 'enable': True, 'frames': [0, 3]})
    glb = (plain / 'rigged.glb').read_bytes()
    assert glb == (tmp_path / 'here' / 'rigged.glb').read_bytes()
    gr.check_rules(glb)
    there = json.loads((plain / 'rig.json').read_text())
    assert 'textured' not in there and 'unwelded_vertices' not in there and list(there) == list(here)
    assert {k: v for k, v in there.items() if k != 'seconds'} == json.loads(json.dumps({k: v for k, v in here.items() if k != 'seconds'}))
    joints = gr.accessor(*gr.parse(glb), gr.parse(glb)[0]['meshes'][0]['primitives'][0]['attributes']['JOINTS_0'])
    assert np.array_equal(att['JOINTS_0'], joints[faces.reshape(-1)])
    # without the rig: a static textured file
    doc, buf, att, idx, image = tex.read_textured((static / 'textured.glb').read_bytes())
    assert 'skins' not in doc and 'animations' not in doc and np.array_equal(image, atlas)
    assert att['POSITION'].tobytes() == verts[faces.reshape(-1)].tobytes() and set(att) == {'POSITION', 'NORMAL', 'TEXCOORD_0'}
