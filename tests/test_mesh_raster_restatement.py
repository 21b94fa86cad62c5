"""CPU: the numpy definition of the mesh rasteriser (tests/mesh_raster_restatement.py) does what it
claims, and what surrounds the kernels works without a GPU.

The independent judge of coverage and depth (test_float64_judge_*) rests on two small derivations.

Coverage.  Snapping moves a vertex by at most 1/512 px per axis, i.e. by at most sqrt(2)/512 < 1/256 px; a point of an edge is
a convex combination of the edge's two vertices, so every point of a snapped edge lies within 1/256 px of the same point of the
true edge.  Move the three vertices linearly from their true to their snapped places: the triangle's outline stays within 1/256
px of the true outline all the way, so it never passes through a sample that is farther than 1/128 px from every true edge,
and the sample's winding number -- inside or outside -- is the same at both ends.  At such samples the float64 point-in-triangle
test on the unsnapped projections must therefore agree with `cover` exactly, whatever the fill rule.

Depth.  Over a triangle, 1/z is an affine function f of the screen position, with gradient g = (n_x / (fx D), n_y / (fy D)) for
the plane n . X = D of its camera-space vertices.  The definition interpolates the true values f(X_k) from the snapped places
X'_k = X_k + d_k; barycentric weights b'_k reproduce affine functions, so at a sample inside the snapped triangle
f'(P) - f(P) = - sum b'_k g . d_k, and with b'_k in [0, 1], sum b'_k = 1 and |d_k| <= 1/512 per axis:
|f' - f| <= Delta = (|g_x| + |g_y|) / 512.  Then |z' - z| = |f' - f| z z' <= e = Delta z^2 / (1 - Delta z), and the float32
rounding adds at most 2^-24 (z + e); 1e-12 covers the float64 arithmetic of either side.  Where several triangles cover a sample
the nearest of either side is compared, under the largest of their bounds.

Recorded by test_tool_made_dataset (64 x 64, 3 frames; printed, not gated): 288, 288 and 286 pixels of SyntheticSMPL silhouette,
all of them (share 1.0) inside the mask, IoU 0.5714, 0.5455 and 0.5277 -- the mask is painted from 3 cm discs of at least 1.6
px and is wider than the mesh by construction; 3, 5 and 1 of the 13 684 triangles have no fixed-point area at this size."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from tests import mesh_raster_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _alone(c, r, t):
    """cover of triangle t alone, on the vertices already projected."""
    keys, _ = rr.raster_keys(c['faces'][t:t + 1], r['xy'], r['z'], r['vflag'], c['H'], c['W'])
    return (keys != rr.EMPTY_KEY).astype(np.int64)


@pytest.mark.parametrize('name', ['grid', 'grid4'])
def test_fill_rule_covers_shared_edges_and_vertices_once(name):
    c = rr.CASES[name]()
    r = rr.run_case(c)
    assert np.array_equal(r['xy'], (c['uv'] * 256).astype(np.int32)) and not r['vflag'].any()      # vertices ON samples
    total = sum(_alone(c, r, t) for t in range(len(c['faces'])))
    i, j = np.mgrid[0:c['H'], 0:c['W']]
    inside = (j >= 4) & (j < 52) & (i >= 4) & (i < 36)            # the union's interior with its top and left borders
    strictly = (j > 4) & (j < 52) & (i > 4) & (i < 36)
    assert (total[strictly] == 1).all() and np.array_equal(total, inside.astype(np.int64))
    assert np.array_equal(r['cover'], inside.astype(np.uint8)) and r['counts']['covered'] == int(inside.sum())
    on_edges = inside & (((j - 4) % 4 == 0) | ((i - 4) % 4 == 0) | ((i - j) % 4 == 0) | ((i + j) % 4 == 0))
    assert on_edges.sum() > 300                                      # the samples the rule is about


@pytest.mark.parametrize('name', ['grid', 'blobs', 'ties', 'mixed'])
def test_reversed_winding_gives_the_same_image(name):
    c = rr.CASES[name]()
    r = rr.run_case(c)
    back = rr.run_case(dict(c, faces=np.ascontiguousarray(c['faces'][:, [0, 2, 1]])))
    for k in ('cover', 'tri', 'rgb'):
        assert np.array_equal(r[k], back[k]), k
    assert np.array_equal(r['depth'].view(np.uint32), back['depth'].view(np.uint32)) and r['counts'] == back['counts']


def test_depth_ties_and_nearer_triangles():
    c = rr.case_ties()
    r = rr.run_case(c)
    alone = [_alone(c, r, t).astype(bool) for t in range(4)]
    assert np.array_equal(alone[0], alone[1]) and alone[0].sum() > 300 and alone[2].sum() > 50
    assert (alone[2] & alone[0]).sum() == alone[2].sum() and (alone[0] & ~alone[2]).any()
    tri = r['tri']
    assert (tri[alone[2]] == 2).all()                                # the nearer triangle wins whatever its index
    assert (tri[alone[0] & ~alone[2]] == 0).all() and not (tri == 1).any()      # coincident: the lower index
    assert (tri[alone[3] & ~alone[0]] == 3).all() and (alone[3] & ~alone[0]).any() and (tri[~alone[3] & ~alone[0]] == -1).all()
    assert np.isposinf(r['depth'][tri == -1]).all() and (r['rgb'][tri == -1] == 255).all()
    d = r['depth']
    assert d[tri == 2].max() < 2.3 and d[tri == 0].min() > 2.9 and d[tri == 3].min() > 4.9
    # the colour of a pixel lies between its triangle's vertex colours
    cols = c['colors'][c['faces'][2]].astype(np.int64)
    px = r['rgb'][tri == 2].astype(np.int64)
    assert (px >= cols.min(0)).all() and (px <= cols.max(0)).all()


def test_flags_and_counts():
    c = rr.case_flags()
    r = rr.run_case(c)
    assert r['vflag'][2] == 1 and r['vflag'][5] == 2 and r['vflag'].sum() == 3
    assert not r['xy'][[2, 5]].any() and not r['z'][[2, 5]].any() and (r['z'][r['vflag'] == 0] > 2.9).all()
    n = r['counts']
    assert [n[k] for k in rr.COUNTS[:5]] == [1, 1, 1, 2, 1] and n['wide'] == 2
    assert sorted(np.unique(r['tri']).tolist()) == [-1, 5, 6]
    assert (r['tri'][:, 63] == 5).any() and n['covered'] == int((r['tri'] >= 0).sum())       # partly off screen: drawn up to the border
    # a NaN or infinite position is a flag, never an index into the image
    pos = c['pos'].copy()
    pos[18] = [np.nan, 0, 0]
    pos[19] = [0, 0, np.inf]
    pos[20] = [np.inf, 0, 0]
    xy, z, vflag = rr.project(pos, c['K'], c['E'])
    assert vflag[18] == 1 and vflag[19] == 2 and vflag[20] == 1 and not xy[18:21].any() and not z[18:21].any()
    K = c['K'].copy()
    K[0, 1] = 1e-3
    with pytest.raises(NotImplementedError, match='mesh_project: skew'):
        rr.project(pos, K, c['E'])
    with pytest.raises(ValueError, match='mesh_raster: H=0'):
        rr.raster_keys(c['faces'], xy, z, vflag, 0, 64)
    off = rr.run_case(rr.case_offscreen())
    assert off['counts']['offscreen'] == 40 and off['counts']['covered'] == 0 and not off['cover'].any()
    empty = rr.run_case(rr.case_random(0), bgcolor=(1, 2, 3))
    assert not empty['cover'].any() and (empty['rgb'] == [1, 2, 3]).all() and not any(empty['counts'].values())


def _judge(c):
    """float64, unsnapped: per sample (inside any triangle, nearest ray-triangle depth, its bound, near an edge)."""
    fx, fy, cx, cy, R, t = rr.camera(c['K'], c['E'])
    cam = c['pos'].astype(np.float64) @ R.T + t
    uv = np.stack([fx * cam[:, 0] / cam[:, 2] + cx, fy * cam[:, 1] / cam[:, 2] + cy], 1)
    H, W = c['H'], c['W']
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    P = np.stack([j, i], -1)
    inside_any, near_edge = np.zeros((H, W), bool), np.zeros((H, W), bool)
    depth, bound = np.full((H, W), np.inf), np.zeros((H, W))
    for f in c['faces']:
        a = uv[f]
        s = []
        for k in range(3):
            p0, p1 = a[k], a[(k + 1) % 3]
            d = p1 - p0
            s.append(d[0] * (P[..., 1] - p0[1]) - d[1] * (P[..., 0] - p0[0]))
            u = np.clip(((P - p0) @ d) / (d @ d), 0.0, 1.0)
            near_edge |= np.linalg.norm(P - (p0 + u[..., None] * d), axis=-1) <= 1.0 / 128.0
        inside = ((s[0] > 0) & (s[1] > 0) & (s[2] > 0)) | ((s[0] < 0) & (s[1] < 0) & (s[2] < 0))
        n = np.cross(cam[f[1]] - cam[f[0]], cam[f[2]] - cam[f[0]])
        D = n @ cam[f[0]]
        zt = D / (n[0] * (j - cx) / fx + n[1] * (i - cy) / fy + n[2])
        delta = (abs(n[0] / (fx * D)) + abs(n[1] / (fy * D))) / 512.0
        with np.errstate(all='ignore'):
            e = delta * zt ** 2 / (1.0 - delta * zt)
            b = e + 2.0 ** -24 * (zt + e) + 1e-12
        assert (delta * zt[inside] < 0.5).all()
        depth = np.where(inside & (zt < depth), zt, depth)
        bound = np.where(inside, np.maximum(bound, b), bound)
        inside_any |= inside
    return inside_any, depth, bound, near_edge


@pytest.mark.parametrize('name', ['blobs', 'ties'])
def test_float64_judge_of_coverage_and_depth(name):
    c = rr.CASES[name]()
    r = rr.run_case(c)
    inside, depth, bound, near_edge = _judge(c)
    checked = ~near_edge
    left_out = float(near_edge.mean())
    err = np.abs(r['depth'].astype(np.float64)[checked & inside] - depth[checked & inside])
    print(f'\n   {name}: {left_out:.4f} of the samples within 1/128 px of an edge; {int((checked & inside).sum())} covered samples '
          f'checked, max |depth - judge| = {err.max():.3e} m under a bound of {bound[checked & inside].min():.3e} .. '
          f'{bound[checked & inside].max():.3e}')
    assert left_out <= 0.05
    assert np.array_equal(r['cover'][checked].astype(bool), inside[checked])
    assert (checked & inside).sum() > 300 and (err <= bound[checked & inside]).all()


def test_camera_convention_is_the_renderers():
    """A point on the ray get_rays_from_KRT gives pixel (i, j) projects to (256 j, 256 i)."""
    from occnerf_amd import synth
    from occnerf_amd.dataset import apply_global_tfm_to_camera
    H, W = 48, 64
    K32, E32 = synth.setup_camera(64)
    K = K32.astype(np.float64)
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    E = apply_global_tfm_to_camera(synth.rotate_camera(E32.astype(np.float64), 0.4), np.array([0.05, 0.25, -0.04], np.float32),
                                   np.array([0.08, -0.05, 0.12], np.float32))
    rays_o, rays_d = synth.get_rays_from_KRT(H, W, K, E[:3, :3], E[:3, 3])
    i, j = np.mgrid[0:H, 0:W]
    for s in (4.0, 6.5):
        pos = (rays_o + s * rays_d).reshape(-1, 3).astype(np.float32)
        xy, z, vflag = rr.project(pos, K, E)
        assert not vflag.any() and np.abs(z - s).max() < 1e-5
        assert np.abs(xy[:, 0] - 256 * j.ravel()).max() <= 1 and np.abs(xy[:, 1] - 256 * i.ravel()).max() <= 1
    # ... and a one-pixel triangle around a sample covers that pixel and no other
    uv = np.array([[20.0, 9.6], [20.4, 10.3], [19.6, 10.3]])
    r = rr.rasterize(rr.unproject(K, E, uv, [5.0, 5.0, 5.0]), [[0, 1, 2]], rr.vertex_colors(3), K, E, H, W)
    assert r['counts']['covered'] == 1 and r['cover'][10, 20] == 1 and abs(float(r['depth'][10, 20]) - 5.0) < 1e-5


def test_tool_made_dataset(tmp_path):
    """The SyntheticSMPL mesh posed by the tool's own forward kinematics lands where the tool's own projection puts it."""
    from occnerf_amd import synth
    from occnerf_amd.dataset import PreparedDataset
    tool = rr.load_tool()
    path = str(tmp_path / 'ds')
    tool.make_dataset(path, frames=3, width=64, height=64, seed=0)
    ds = PreparedDataset(path, device=None)
    with open(os.path.join(path, 'mesh_infos.pkl'), 'rb') as f:
        infos = pickle.load(f)
    with open(os.path.join(path, 'cameras.pkl'), 'rb') as f:
        cameras = pickle.load(f)
    for i in range(3):
        f = ds.frames[i]
        info, cam = infos[f['frame_name']], cameras[f['frame_name']]
        verts, _ = synth.SyntheticSMPL()(np.zeros(72), info['betas'])
        posed, _ = tool.posed_body(info['poses'].astype(np.float64), info['tpose_joints'].astype(np.float64), verts,
                                   tool.vertex_joints())
        pos, faces, colors = rr.posed_smpl(tool, info)
        assert np.array_equal(pos, posed.astype(np.float32)) and faces.shape[0] > 13000 and faces.shape[1] == 3
        # the tool's projection (make_dataset): the body into the world by Rh / Th, then the calibrated camera
        world = posed.dot(synth.rodrigues_exact(info['Rh']).T) + info['Th'].astype(np.float64)
        c = world.dot(cam['extrinsics'][:3, :3].T) + cam['extrinsics'][:3, 3]
        pix = c.dot(cam['intrinsics'].T)
        uv = pix[:, :2] / pix[:, 2:3]
        r = rr.rasterize(pos, faces, colors, f['K'], f['E'], 64, 64)
        assert not r['vflag'].any()
        # the float32 rounding of a vertex (2^-24 of at most 2 m per axis) moves its projection by at most
        # 2 fx / z sqrt(3) 2^-23 pixels (the factor 2 covers the oblique rays of a camera this narrow)
        rounding = 256.0 * 2.0 * f['K'][0, 0] / c[:, 2].min() * np.sqrt(3.0) * 2.0 ** -23
        worst = np.abs(r['xy'] - 256.0 * uv).max()
        assert np.abs(posed).max() < 2.0 and worst <= 1.0 + rounding, (worst, rounding)
        inter, union, iou, covered, inside = rr.mask_iou(r['cover'], ds.gt_alpha(i))
        print(f"\n   {f['frame_name']}: worst |xy - 256 uv| = {worst:.3f} units (rounding term {rounding:.4f}); {covered} pixels "
              f"covered, {inside:.4f} of them inside the mask, IoU {iou:.4f}; counts {r['counts']}")
        assert covered > 100 and sum(r['counts'][k] for k in rr.COUNTS[:3]) == 0      # (a few slivers have no fixed-point area)


def test_mask_iou():
    cover = np.zeros((4, 6), np.uint8)
    cover[1:3, 1:4] = 1
    gt = np.zeros((4, 6), np.float32)
    gt[1:4, 2:6] = 1.0
    gt[0, 0] = 0.5                                                   # not above the threshold
    assert rr.mask_iou(cover, gt) == (4, 14, 4 / 14, 6, 4 / 6)
    assert rr.mask_iou(np.zeros((2, 2), np.uint8), np.zeros((2, 2), np.float32)) == (0, 0, None, 0, None)


def test_configuration_and_plumbing():
    from occnerf_amd import mesh_view
    from occnerf_amd.config import default_cfg
    assert dict(default_cfg().mesh_view) == {'frames': None, 'panels': True}
    cfg = default_cfg().merge_from_list(['mesh_view.frames', '[0, 17]', 'mesh_view.panels', 'False'])
    assert cfg.mesh_view.frames == [0, 17] and cfg.mesh_view.panels is False
    assert default_cfg().merge_from_list(['mesh_view.frames', 'all']).mesh_view.frames == 'all'
    src = open(os.path.join(ROOT, 'run.py')).read()
    assert 'export_views(' in src and "mv.get('frames') is not None" in src and 'mesh/view.json' in src
    with pytest.raises(RuntimeError, match='mesh_view.frames: .*prepared dataset'):
        mesh_view.export_views(None, 'nowhere', {}, None, [0])
    for word in ('clipping', 'anti-aliasing', 'lighting and textures', 'rendered', 'all_cameras.pkl'):
        assert word in mesh_view.__doc__, word
    assert mesh_view.COUNTS == rr.COUNTS


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from occnerf_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    K = (ctypes.c_double * 9)(50.0, 0.0, 32.0, 0.0, 50.0, 24.0, 0.0, 0.0, 1.0)
    skew = (ctypes.c_double * 9)(50.0, 0.25, 32.0, 0.0, 50.0, 24.0, 0.0, 0.0, 1.0)

    def refused(rc, who, word):
        msg = lib.occnerf_last_error()
        assert rc != 0 and msg.startswith(who.encode()) and word.encode() in msg, (rc, msg)

    def project(V=5, pos=p, K=K, E=p, out=p):
        return lib.occnerf_mesh_project(pos, V, K, E, out, p, p, None)
    refused(project(K=None), 'mesh_project', 'null')
    refused(project(E=None), 'mesh_project', 'null')
    refused(project(pos=None), 'mesh_project', 'null')
    refused(project(out=None), 'mesh_project', 'null')
    refused(project(K=skew), 'mesh_project', 'skew K[0,1] = 0.25')
    refused(project(V=-1), 'mesh_project', 'V=-1')
    refused(project(V=1 << 31), 'mesh_project', 'V=2147483648')
    assert project(V=0, pos=None, out=None) == 0                   # nothing to do: 0 without a launch (there is no GPU here)

    def raster(T=4, V=5, H=48, W=64, faces=p, keys=p, counts=p):
        return lib.occnerf_mesh_raster(faces, T, V, p, p, p, H, W, keys, p, counts, None)
    refused(raster(faces=None), 'mesh_raster', 'null')
    refused(raster(keys=None), 'mesh_raster', 'null')
    refused(raster(counts=None), 'mesh_raster', 'null')
    refused(raster(H=0), 'mesh_raster', 'H=0')
    refused(raster(W=16385), 'mesh_raster', 'W=16385')
    refused(raster(H=16384 + 1, W=1), 'mesh_raster', 'H=16385')
    refused(raster(T=-1), 'mesh_raster', 'T=-1')
    refused(raster(T=1 << 31), 'mesh_raster', 'T=2147483648')
    refused(raster(V=1 << 31), 'mesh_raster', 'V=2147483648')
    assert raster(T=0, faces=None, keys=None) == 0 and raster(V=0, faces=None) == 0

    def resolve(T=4, V=5, H=48, W=64, keys=p, bg=p, rgb=p):
        return lib.occnerf_mesh_resolve(keys, p, T, V, p, p, p, p, bg, H, W, p, p, p, rgb, p, None)
    refused(resolve(keys=None), 'mesh_resolve', 'null')
    refused(resolve(bg=None), 'mesh_resolve', 'null')
    refused(resolve(rgb=None), 'mesh_resolve', 'null')
    refused(resolve(H=-3), 'mesh_resolve', 'H=-3')
    refused(resolve(T=1 << 31), 'mesh_resolve', 'T=2147483648')
    refused(resolve(V=-2), 'mesh_resolve', 'V=-2')
    assert resolve(T=0, keys=None, rgb=None) == 0 and resolve(V=0, keys=None) == 0
    assert lib.occnerf_abi_version() == 5
    # the definition and the kernels state the same constants
    src = open(os.path.join(ROOT, 'occnerf_amd', 'csrc', 'mesh_raster.hip')).read()
    screen = open(os.path.join(ROOT, 'occnerf_amd', 'csrc', 'mesh_screen.h')).read()          # the vertex rule's limits live there
    for text, value, where in (('kRasterWide = 64', rr.WIDE, src), ('kScreenNear = 1e-3', rr.NEAR, screen),
                               ('kScreenFar = 1048576.0', rr.FAR, screen), ('kScreenGuard = 4194304.0', rr.GUARD, screen),
                               ('kRasterMaxSide = 16384', rr.MAX_SIDE, src)):
        assert text in where and float(text.split('= ')[1]) == float(value), text
    assert 'fma' not in re.sub(r'//[^\n]*', '', src).lower()
    make = open(os.path.join(ROOT, 'occnerf_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bmesh_raster\.hip\b', make, flags=re.M)


def test_wrappers_refuse_host_tensors():
    import torch
    from occnerf_amd import mesh_view, ops
    c = rr.case_ties()
    pos, faces, colors = torch.from_numpy(c['pos']), torch.from_numpy(c['faces']), torch.from_numpy(c['colors'])
    with pytest.raises(RuntimeError, match='mesh_project: pos must be a CUDA'):
        ops.mesh_project(pos, c['K'], c['E'])
    with pytest.raises(RuntimeError, match='mesh_project: pos must be a CUDA'):
        mesh_view.rasterize(pos, faces, colors, c['K'], c['E'], 48, 64)
    xy, z, vflag = (torch.from_numpy(a) for a in rr.project(c['pos'], c['K'], c['E']))
    with pytest.raises(RuntimeError, match='mesh_raster: faces must be a CUDA'):
        ops.mesh_raster(faces, xy, z, vflag, 48, 64)
    with pytest.raises(RuntimeError, match='mesh_resolve: keys must be a CUDA'):
        ops.mesh_resolve(torch.zeros(48, 64, dtype=torch.int64), torch.zeros(7, dtype=torch.int32), faces, xy, z, vflag, colors,
                         (255, 255, 255))
