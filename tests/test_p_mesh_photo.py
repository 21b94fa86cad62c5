"""GPU: the photographs on the atlas.  csrc/mesh_texture.hip's mesh_texture_project and mesh_texture_blend
against the numpy definition (tests/mesh_photo_restatement.py) -- accumulators, seen counts and both images EQUAL, on the device's
own raster keys --, the exact photographs and the visibility cases of tests/test_mesh_photo_restatement.py through the kernels,
the exports in this process on a tool-made dataset and run.py --type mesh with mesh_photo.enable end to end."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_photo_restatement as ph
from tests import mesh_raster_restatement as mrr
from tests import mesh_texture_restatement as tex
from tests import test_mesh_photo_restatement as cpu
from tests.gpu_util import DEV, T, build_network, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_SIZES = (1, 2, 3, 63, 64, 65, 257)
CELLS = (4, 5, 8)


def _device_keys(ops, pos, faces, K, E, H, W):
    xy, z, vflag = ops.mesh_project(pos, K, E)
    return ops.mesh_raster(faces, xy, z, vflag, H, W)[0]


def _both(ops, faces, n, items, bias, atlas, C, min_seen=1):
    """The frames `items` (numpy, as the definition takes them) through mesh.project_photos and ops.mesh_texture_blend, and
    through the definition on the device's own keys -> ((acc, seen, photo, seen image) of the device as numpy, the definition's)."""
    from occnerf_amd import mesh
    f = T(faces)
    size = len(faces)
    dev_items = [(T(p), T(pf), K, E, T(photo), T(inside)) for p, pf, K, E, photo, inside in items]
    acc, seen, figures = mesh.project_photos(iter(dev_items), f, n, bias)
    photo, img = ops.mesh_texture_blend(acc, seen, size, n, C, T(atlas), min_seen)
    got = tuple(a.cpu().numpy() for a in (acc, seen, photo, img))
    wacc, wseen = ph.accumulators(size, n)
    total = 0
    for (p, pf, K, E, pic, inside), d, row in zip(items, dev_items, figures):
        keys = _device_keys(ops, d[0], f, K, E, pic.shape[0], pic.shape[1]).cpu().numpy().view(np.uint64) if size else None
        tri_w, _ = ph.project_frame(faces, n, p, pf, K, E, pic, inside, bias, wacc, wseen, keys=keys)
        assert row['triangles_facing_away'] == int((tri_w < 0).sum()) and row['triangles_weighted'] == int((tri_w > 0).sum())
        assert row['texels_seen'] == int(wseen.sum()) - total
        total = int(wseen.sum())
    return got, (wacc, wseen, *ph.blend(wacc, wseen, size, n, C, atlas, min_seen))


def _check(ops, c, n, frames, seed, name):
    faces, V, H, W = c['faces'], len(c['pos']), c['H'], c['W']
    atlas, C = cpu.field_atlas(len(faces), n, seed)
    items = []
    for k, (K, E) in enumerate(ph.perturbed_cameras(c['K'], c['E'], frames, seed)):
        photo, inside, pflag = ph.random_frame_inputs(V, H, W, seed + 10 * k)
        items.append((c['pos'], pflag, K, E, photo, inside))
    got, want = _both(ops, faces, n, items, 0.05, atlas, C)
    for g, w, what in zip(got, want, ('acc', 'seen', 'texture_photo', 'texture_seen')):
        same(g, w, f'{name}: {what}')
    again, _ = _both(ops, faces, n, items, 0.05, atlas, C)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), name        # the same bytes again
    return int((want[1] > 0).sum())


@pytest.mark.parametrize('n', CELLS)
@pytest.mark.parametrize('H,W', ((64, 64), (64, 96)))
def test_kernels_are_the_definition_on_welded_grids(ops, n, H, W):
    """T = 63 .. 65 at n = 5 and 8 put the 256-thread workgroup boundary inside a triangle's P texels, n = 4 is m = 1, odd T
    leaves the last cell half empty; the grids reach two image borders and leave empty pixels at the other two; even T keeps
    the grid's mixed windings (half the triangles face away), odd T faces the camera."""
    seen = 0
    for size in T_SIZES:
        c = ph.surface_case(size, H, W, seed=n, face=bool(size % 2))
        for frames in (1, 3):
            seen += _check(ops, c, n, frames, size + n, f'T={size} n={n} {H}x{W} frames={frames}')
    assert seen > 1000
    torch.cuda.synchronize()


@pytest.mark.parametrize('name', ('grid', 'ties', 'mixed', 'blobs', 'random257'))
def test_kernels_are_the_definition_on_the_raster_cases(ops, name):
    c = mrr.case_random(257) if name == 'random257' else mrr.CASES[name]()
    facing = {**c, 'faces': ph.face_the_camera(c['pos'], c['faces'], c['K'], c['E'])}
    seen = 0
    for n in CELLS:
        seen += _check(ops, c, n, 1, n, f'{name} n={n}') + _check(ops, facing, n, 3, n, f'{name} facing n={n}')
    print(f'\n   {name}: {seen} texels seen over the six runs')
    assert seen > 30
    torch.cuda.synchronize()


def test_no_triangles_and_bad_indices(ops):
    from occnerf_amd import mesh
    c = ph.surface_case(65)
    V, H, W, n = len(c['pos']), c['H'], c['W'], 5
    photo, inside, pflag = ph.random_frame_inputs(V, H, W)
    item = (T(c['pos']), T(pflag), c['K'], c['E'], T(photo), T(inside))
    acc, seen, figures = mesh.project_photos(iter([item]), T(c['faces'][:0]), n, 0.05)
    assert tuple(acc.shape) == (0, 4) and tuple(seen.shape) == (0,) and figures[0]['texels_seen'] == 0
    atlas = T(np.full((8, 8, 3), 7, np.uint8))
    out, img = ops.mesh_texture_blend(acc, seen, 0, n, 1, atlas[:5, :5].contiguous())
    assert (out == 7).all() and (img == 0).all()
    # an index equal to V, and a negative one: refused by name by the entry itself, never an address
    f = T(c['faces'])
    q = ops.mesh_texel_points(item[0], f, n).reshape(-1, 3)
    xy, z, vflag = ops.mesh_project(q, c['K'], c['E'])
    keys = _device_keys(ops, item[0], f, c['K'], c['E'], H, W)
    P = n * (n - 1) // 2
    for value in (V, -1):
        bad = c['faces'].copy()
        bad[-1, 2] = value
        acc = torch.zeros(65 * P, 4, device=DEV, dtype=torch.int64)
        seen = torch.zeros(65 * P, device=DEV, dtype=torch.int32)
        with pytest.raises(RuntimeError, match=f'mesh_texture_project: a face index lies outside \\[0, {V}\\)'):
            ops.mesh_texture_project(xy, z, vflag, item[0], item[1], T(bad), n, c['K'], c['E'], keys, item[4], item[5], 0.05, acc, seen)
        with pytest.raises(RuntimeError, match='mesh_texel_points: a face index lies outside'):
            mesh.project_photos(iter([item]), T(bad), n, 0.05)
    with pytest.raises(RuntimeError, match='mesh_texture_project: bias'):
        ops.mesh_texture_project(xy, z, vflag, item[0], item[1], f, n, c['K'], c['E'], keys, item[4], item[5], -1.0, acc, seen)
    with pytest.raises(RuntimeError, match='mesh_texture_project: acc must be int64'):
        ops.mesh_texture_project(xy, z, vflag, item[0], item[1], f, n, c['K'], c['E'], keys, item[4], item[5], 0.05, acc[:-1], seen)
    with pytest.raises(RuntimeError, match='mesh_texture_blend: an atlas of .* does not hold'):
        ops.mesh_texture_blend(acc, seen, 65, n, 1, atlas)
    torch.cuda.synchronize()


@pytest.mark.parametrize('frames', (1, 3))
def test_a_constant_photograph_through_the_kernels(ops, frames):
    c = ph.surface_case(129)
    V, size, n, H, W = len(c['pos']), len(c['faces']), 5, c['H'], c['W']
    atlas, C = cpu.field_atlas(size, n)
    items = [(c['pos'], np.zeros(V, np.uint8), K, E, ph.constant_photo(H, W, 173), np.ones((H, W), np.uint8))
             for K, E in ph.perturbed_cameras(c['K'], c['E'], frames)]
    (acc, seen, photo, img), _ = _both(ops, c['faces'], n, items, 0.05, atlas, C)
    x, y = ph.atlas_index(size, n, C)
    hit = seen > 0
    assert hit.sum() > 100 and (~hit).sum() > 100 and (photo[y[hit], x[hit]] == 173).all()
    assert np.array_equal(photo[y[~hit], x[~hit]], atlas[y[~hit], x[~hit]])
    own = cpu.owned_mask(size, n, C, img.shape)
    assert (photo[~own] == np.array(cpu.FILL, np.uint8)).all() and (img[~own] == 0).all()


def test_an_integer_affine_photograph_through_the_kernels(ops):
    for name, n in (('surface', 8), ('blobs', 8), ('grid', 5), ('ties', 8)):
        c = ph.surface_case(65) if name == 'surface' else {**cpu.facing_case(name), 'H': 64, 'W': 64}
        V, size = len(c['pos']), len(c['faces'])
        atlas, C = cpu.field_atlas(size, n)
        items = [(c['pos'], np.zeros(V, np.uint8), c['K'], c['E'], ph.affine_photo(), np.ones((64, 64), np.uint8))]
        (acc, seen, photo, img), _ = _both(ops, c['faces'], n, items, 0.05, atlas, C)
        xy, _, _ = ops.mesh_project(ops.mesh_texel_points(T(c['pos']), T(c['faces']), n).reshape(-1, 3), c['K'], c['E'])
        x, y = ph.atlas_index(size, n, C)
        ok = seen > 0
        assert ok.sum() > 20, name
        same(photo[y[ok], x[ok]], ph.affine_expected(xy.cpu().numpy()[ok]), f'{name}: the affine photograph')


def test_the_depth_bias_and_the_winding_through_the_kernels(ops):
    H = W = 48
    pos, faces, K, E = ph.two_quads(0.25, H, W)
    n = 8
    P = n * (n - 1) // 2
    atlas, C = cpu.field_atlas(4, n)
    item = (pos, np.zeros(8, np.uint8), K, E, ph.constant_photo(H, W, 50), np.ones((H, W), np.uint8))
    (_, near, _, _), (_, want, _, _) = _both(ops, faces, n, [item], 0.1, atlas, C)
    near = near.reshape(4, P)
    assert np.array_equal(near.ravel(), want) and near[:2].sum() > 10 and near[2:].sum() == 0       # b < D
    (_, both, _, _), _ = _both(ops, faces, n, [item], 0.3, atlas, C)
    both = both.reshape(4, P)
    assert np.array_equal(both[:2], near[:2]) and both[2:].sum() > 10                               # b > D
    (_, rev, _, _), _ = _both(ops, np.ascontiguousarray(faces[:, [0, 2, 1]]), n, [item], 0.3, atlas, C)
    assert rev.sum() == 0                                                                           # reversed winding: unseen
    (_, none, _, _), _ = _both(ops, faces, n, [(*item[:5], np.zeros((H, W), np.uint8))], 0.3, atlas, C)
    assert none.sum() == 0                                                                          # inside all zero


# ------------------------------------------------------------------ the exports in this process
def test_exports_on_a_tool_made_dataset(ops, tmp_path):
    """export_mesh, export_texture, export_photo_texture and export_views on the 16-grid's median level and a tool-made dataset
    of 4 frames of 64 x 64 with mesh_photo.frames [0, 2]."""
    from PIL import Image

    from occnerf_amd import mesh, mesh_view
    from occnerf_amd.dataset import PreparedDataset
    net, _ = build_network(0, False, S=32, non_rigid=True)
    path = str(tmp_path / 'ds')
    mrr.load_tool().make_dataset(path, frames=4, width=64, height=64, seed=0)
    ds = PreparedDataset(path, device=None)
    bmin, bmax = ds.cnl_bbox_min_xyz, ds.cnl_bbox_max_xyz
    field, _, _ = mesh.density_grid(net, bmin, bmax, 16)
    out, kept, n, fill = str(tmp_path / 'mesh'), {}, 5, [3, 4, 5]
    mesh.export_mesh(net, out, bmin, bmax, resolution=16, level=float(field.median().item()), keep=kept)
    mesh.export_texture(net, out, kept, {'enable': True, 'cell': n, 'fill': fill})
    with pytest.raises(RuntimeError, match='mesh_photo.frames: frame 4 outside the 4 frames'):
        mesh.export_photo_texture(net, out, kept, ds, {**mesh.PHOTO_DEFAULTS, 'enable': True, 'frames': [4]})
    with pytest.raises(RuntimeError, match='mesh_texture.enable, which is not set'):
        mesh.export_photo_texture(net, out, {k: v for k, v in kept.items() if k != 'texture'}, ds, {**mesh.PHOTO_DEFAULTS, 'enable': True})
    poser = mesh.MeshPoser(net, kept['verts'])
    info = mesh.export_photo_texture(net, out, kept, ds, {**mesh.PHOTO_DEFAULTS, 'enable': True, 'frames': [0, 2]}, poser=poser)
    assert all(os.path.exists(os.path.join(out, f)) for f in ('texture_photo.png', 'texture_seen.png', 'texture_photo.json'))
    faces_np = np.asarray(kept['faces'], np.int32)
    size = len(faces_np)
    C, R, W, H, P = tex.layout(size, n)
    photo = np.asarray(Image.open(os.path.join(out, 'texture_photo.png')).convert('RGB'))
    seen_img = np.asarray(Image.open(os.path.join(out, 'texture_seen.png')))
    field_png = np.asarray(Image.open(os.path.join(out, 'texture.png')).convert('RGB'))
    disk = json.load(open(os.path.join(out, 'texture_photo.json')))
    assert photo.shape == (H, W, 3) and seen_img.shape == (H, W) and seen_img.dtype == np.uint8
    assert (disk['H'], disk['W'], disk['frames'], disk['bias_m'], disk['bias_is_voxel_edge']) == (H, W, [0, 2], kept['h'], True)
    assert disk['bytes']['accumulators'] == size * P * 36 and [r['frame'] for r in disk['per_frame']] == [0, 2]
    assert set(disk['per_frame'][0]['seconds']) == {'points', 'project', 'raster', 'accumulate', 'pose_and_load'}
    x, y = ph.atlas_index(size, n, C)
    counts = seen_img[y, x]
    assert disk['seen_histogram'] == ph.seen_histogram(counts) and sum(disk['seen_histogram'].values()) == size * P
    assert disk['seen_share'] == (size * P - int((counts == 0).sum())) / (size * P)
    assert sum(r['texels_seen'] for r in disk['per_frame']) == int(counts.astype(np.int64).sum())
    print(f"\n   {size} triangles, {int((counts > 0).sum())} of {size * P} texels seen, histogram {disk['seen_histogram']}")
    assert (counts > 0).sum() > 0 and (counts == 0).sum() > 0
    same(photo[y[counts == 0], x[counts == 0]], field_png[y[counts == 0], x[counts == 0]], 'unseen texels are the field')
    own = cpu.owned_mask(size, n, C, seen_img.shape)
    assert (photo[~own] == np.array(fill, np.uint8)).all() and (seen_img[~own] == 0).all()
    # the whole export against the definition on the posed vertices, with the definition's own keys
    items = []
    for i in (0, 2):
        f = ds.frames[i]
        _, _, p, flag, _, _, _ = poser.frame(i, mesh._device_frame(ds.host_constants(i), torch.device(DEV)))
        items.append((p.cpu().numpy(), flag.cpu().numpy(), f['K'], f['E'], ds.truth_u8(i), (np.asarray(ds.gt_alpha(i)) > 0.5).astype(np.uint8)))
    want_photo, want_seen, _, _ = ph.photo_texture(faces_np, n, items, kept['h'], field_png, C)
    same(photo, want_photo, 'texture_photo.png')
    same(seen_img, want_seen, 'texture_seen.png')
    assert poser.solved == 2
    # the views: [vertex colours | field texture | photo texture | photograph]
    views = mesh_view.export_views(net, out, kept, ds, 'all', texture=kept['texture'], photo=kept['texture_photo'], poser=poser)
    assert poser.solved == 4 and [r['projected'] for r in views['frames']] == [True, False, True, False]
    for row in views['frames']:
        i = row['frame']
        f = ds.frames[i]
        _, _, p, _, _, _, _ = poser.frame(i, mesh._device_frame(ds.host_constants(i), torch.device(DEV)))
        xy, z, vflag = (a.cpu().numpy() for a in ops.mesh_project(p, f['K'], f['E']))
        keys, _ = mrr.raster_keys(faces_np, xy, z, vflag, 64, 64)
        want = tex.resolve_textured(keys, faces_np, xy, z, photo, n, C, (255, 255, 255))
        img = np.array(Image.open(os.path.join(out, 'view', row['name'] + '.png')))
        assert img.shape == (64, 256, 3)
        same(img[:, 128:192], want, 'the photo-textured panel')
        same(img[:, 192:], ds.truth_u8(i), 'the photograph')
        sel = (keys != mrr.EMPTY_KEY) & (np.asarray(ds.gt_alpha(i)) > 0.5)
        diff = np.abs(want.astype(np.int64) - ds.truth_u8(i).astype(np.int64))[sel]
        assert (row['photo_mean_abs_diff'] is None) == (diff.size == 0)
        if diff.size:
            assert abs(row['photo_mean_abs_diff'] - float(diff.mean())) <= 1e-9
        print(f"\n   {row['name']}: projected {row['projected']}, photo panel against the photograph over {int(sel.sum())} pixels: "
              f"mean |difference| = {row['photo_mean_abs_diff']}")
    plain = mesh_view.export_views(net, str(tmp_path / 'plain'), kept, ds, [0], texture=kept['texture'])
    assert 'photo_mean_abs_diff' not in plain['frames'][0] and 'projected' not in plain['frames'][0]


def test_the_capsule_body_in_the_tools_own_pose(ops, tmp_path):
    """The planted colours of the CPU test through the kernels: the same figures, since the kernels give the definition's bits
    (the device's keys are the definition's on this mesh: tests/test_p_mesh_raster.py)."""
    import pickle

    from occnerf_amd import mesh, synth
    from occnerf_amd.dataset import PreparedDataset
    tool, path, n = mrr.load_tool(), str(tmp_path / 'ds'), 4
    tool.make_dataset(path, frames=4, width=64, height=64, seed=0)
    ds = PreparedDataset(path, device=None)
    infos = pickle.load(open(os.path.join(path, 'mesh_infos.pkl'), 'rb'))
    canonical, _ = synth.SyntheticSMPL()(np.zeros(72), np.zeros(10, np.float32))
    items = []
    for i in (0, 1, 3):
        f = ds.frames[i]
        pos, faces, _ = mrr.posed_smpl(tool, infos[f['frame_name']])
        items.append((T(pos), torch.zeros(len(pos), device=DEV, dtype=torch.uint8), f['K'], f['E'], T(ds.truth_u8(i)),
                      T((np.asarray(ds.gt_alpha(i)) > 0.5).astype(np.uint8))))
    size = len(faces)
    C, _, W, H, P = tex.layout(size, n)
    acc, seen, _ = mesh.project_photos(iter(items), T(faces), n, 0.05)
    photo, _ = ops.mesh_texture_blend(acc, seen, size, n, C, torch.zeros(H, W, 3, device=DEV, dtype=torch.uint8))
    photo, seen = photo.cpu().numpy(), seen.cpu().numpy()
    truth = tool.vertex_colours(tex.texel_points(canonical.astype(np.float32), faces, n)[0].reshape(-1, 3).astype(np.float64)).astype(np.int64)
    x, y = ph.atlas_index(size, n, C)
    hit = seen > 0
    err = np.abs(photo[y[hit], x[hit]].astype(np.int64) - truth[hit])
    print(f'\n   {int(hit.sum())} of {size * P} texels seen; |byte error| median {np.median(err)}, 95 % {np.percentile(err, 95)}; '
          f'an atlas of zeros: median {np.median(truth[hit])}')
    assert hit.sum() > 0 and (~hit).sum() > 0 and np.median(err) < np.median(np.abs(truth[hit]))


# ------------------------------------------------------------------ end to end
def _run_py(tmp, *extra):
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), '--cfg', os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'),
           '--type', 'mesh', 'mesh.resolution', '16', 'N_samples', '16'] + list(extra)
    os.makedirs(str(tmp), exist_ok=True)
    out = subprocess.run(cmd, cwd=str(tmp), env={**os.environ, 'PYTHONPATH': ROOT}, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return tmp / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'seeded' / 'mesh'


def test_run_py_writes_the_photo_texture(ops, tmp_path):
    """run.py --type mesh with mesh_texture.enable and mesh_photo.enable on a tool-made dataset; with in_glb False (the glb is the
    one of the run without mesh_photo); and without mesh_photo (the files of the parent commit, as this process writes them
    through the unchanged functions)."""
    from PIL import Image

    from occnerf_amd import mesh
    from occnerf_amd.dataset import PreparedDataset
    path = str(tmp_path / 'ds')
    mrr.load_tool().make_dataset(path, frames=4, width=64, height=64, seed=0)
    net, _ = build_network(0, False, S=32, non_rigid=True)
    ds = PreparedDataset(path, device=None)
    bmin, bmax = ds.cnl_bbox_min_xyz, ds.cnl_bbox_max_xyz
    field, _, _ = mesh.density_grid(net, bmin, bmax, 16)
    level = repr(float(field.median().item()))
    common = ('train.dataset_path', path, 'resize_img_scale', '1.0', 'mesh.level', level, 'mesh_texture.enable', 'True',
              'mesh_texture.cell', '5')
    keys = ('mesh_photo.enable', 'True', 'mesh_photo.frames', '[0, 2]')
    both = _run_py(tmp_path / 'both', *common, *keys, 'mesh_view.frames', '[0, 1]')
    out_glb = _run_py(tmp_path / 'out_glb', *common, *keys, 'mesh_photo.in_glb', 'False')
    plain = _run_py(tmp_path / 'plain', *common)
    assert sorted(os.listdir(plain)) == ['mesh.json', 'mesh.ply', 'texture.json', 'texture.png', 'textured.glb']
    extra = ['texture_photo.json', 'texture_photo.png', 'texture_seen.png']
    assert sorted(os.listdir(out_glb)) == sorted(os.listdir(plain) + extra)
    assert sorted(os.listdir(both)) == sorted(os.listdir(plain) + extra + ['view', 'view.json'])
    for name in ('mesh.ply', 'texture.png'):
        assert (both / name).read_bytes() == (plain / name).read_bytes() == (out_glb / name).read_bytes(), name
    assert (out_glb / 'textured.glb').read_bytes() == (plain / 'textured.glb').read_bytes()
    for name in ('texture_photo.png', 'texture_seen.png'):
        assert (both / name).read_bytes() == (out_glb / name).read_bytes(), name
    # the glb carries the photo atlas, same UVs
    photo = np.asarray(Image.open(io.BytesIO((both / 'texture_photo.png').read_bytes())).convert('RGB'))
    doc, buf, att, idx, image = tex.read_textured((both / 'textured.glb').read_bytes())
    _, _, att0, _, image0 = tex.read_textured((plain / 'textured.glb').read_bytes())
    assert np.array_equal(image, photo) and np.array_equal(image0, np.asarray(Image.open(plain / 'texture.png').convert('RGB')))
    assert all(att[k].tobytes() == att0[k].tobytes() for k in att0) and set(att) == set(att0)
    disk = json.loads((both / 'texture_photo.json').read_text())
    seen_img = np.asarray(Image.open(both / 'texture_seen.png'))
    assert disk['frames'] == [0, 2] and disk['bias_is_voxel_edge'] and disk['bias_m'] == json.loads((both / 'mesh.json').read_text())['h']
    assert photo.shape == (disk['H'], disk['W'], 3) and seen_img.shape == (disk['H'], disk['W'])
    assert disk['owned_texels'] - disk['seen_histogram']['0'] == int((seen_img > 0).sum())
    views = json.loads((both / 'view.json').read_text())
    assert [(r['frame'], r['projected']) for r in views['frames']] == [(0, True), (1, False)]
    assert np.array(Image.open(both / 'view' / (views['frames'][0]['name'] + '.png'))).shape == (64, 256, 3)
    # without mesh_photo: the parent commit's files, as the unchanged functions write them here
    kept = {}
    here = tmp_path / 'here'
    mesh.export_mesh(net, str(here), bmin, bmax, resolution=16, level=float(level), keep=kept)
    mesh.export_texture(net, str(here), kept, {'enable': True, 'cell': 5, 'fill': [0, 0, 0]})
    mesh.export_textured(str(here), kept)
    for name in ('mesh.ply', 'texture.png', 'textured.glb'):
        assert (plain / name).read_bytes() == (here / name).read_bytes(), name

