"""CPU: the tangent-space normal map of the exported mesh.  The numpy definition
(tests/mesh_normal_restatement.py) on a plane field, where the trilinear sample is exact, and on a sphere, where the map has to
beat the coarse geometry's own normals; every flag provoked by the smallest input; the atlas, the corner tangents, the glTF
writer with the two new keys and every refusal.  The cases take the baker as an argument: tests/test_p_mesh_normal.py runs them
again through the kernel."""
import io
import os
import re

import numpy as np
import pytest

from tests import mesh_normal_restatement as nr
from tests import mesh_texture_restatement as tex
from tests import test_mesh_texture_restatement as cpu_tex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def definition(verts, faces, normals, tangents, creased, pts, n, field, lo, h, level, S):
    return nr.bake(verts, faces, normals, tangents, creased, pts, n, field, lo, h, level, S)


def _inputs(verts, faces, n):
    normals = nr.vertex_normals(verts, faces)
    tangents, creased = nr.corner_tangents(verts, faces, normals)
    pts, status = tex.texel_points(verts, faces, n)
    assert status == 0
    return normals, tangents, creased, pts


def _decoded(out, faces, normals, tangents, n):
    """Every texel's bytes read forwards by the glTF rule (nr.decode) -> (unit normals [T,P,3], condition numbers [T,P])."""
    T = len(faces)
    C, _, _, _, P = tex.layout(T, n)
    ij = tex.owned(n)
    b = np.stack([n - 3 - ij[:, 0] - ij[:, 1], ij[:, 0], ij[:, 1]], -1).astype(np.float64) / (n - 3)     # the barycentrics
    N = np.einsum('pc,tck->tpk', b, normals.astype(np.float64)[faces])
    Tg = np.einsum('pc,tck->tpk', b, tangents.astype(np.float64)[..., :3])
    Tg = np.concatenate([Tg, np.ones((T, P, 1))], -1)
    code = np.stack([out['atlas'][tuple(reversed(tex.atlas_position(t, ij, n, C)))] for t in range(T)])
    return nr.decode(code, N, Tg)


# ------------------------------------------------------------------ the plane
def plane_case(T, n, S, baker=definition):
    """-> (unflagged texels, worst |N_f - truth|, worst angle / bound of the decoded bytes)."""
    field, lo, h, level, truth = nr.plane_field()
    verts, faces = tex.welded_mesh(T, seed=n)
    normals, tangents, creased, pts = _inputs(verts, faces, n)
    out = baker(verts, faces, normals, tangents, creased, pts, n, field, lo, h, level, S)
    clean = out['flags'] == 0
    # float64 rounding where the definition hands out its float64 values; the float32 output adds half an ulp of a number <= 1
    exact = 'N_f' in out
    Nf = out['N_f'] if exact else out['normal'].astype(np.float64)
    worst = float(np.abs(Nf[clean] - truth).max()) if clean.any() else 0.0
    assert worst <= (1e-12 if exact else 2.0 ** -24), worst
    assert np.abs(out['normal'][clean].astype(np.float64) - truth).max(initial=0.0) <= 2.0 ** -24
    dec, kappa = _decoded(out, faces, normals, tangents, n)
    bound = np.arcsin(np.minimum(kappa * np.sqrt(3.0) / 255.0, 1.0)) + 1e-6
    ratio = (nr.angle(dec, truth) / bound)[clean]
    return int(clean.sum()), worst, float(ratio.max()) if clean.any() else 0.0, out


@pytest.mark.parametrize('n', nr.CELLS)
def test_plane(n):
    total = 0
    for T, S in ((3, 2), (65, 2), (257, 2), (64, 1), (63, 2)):
        count, worst, ratio, out = plane_case(T, n, S)
        print(f'\n   plane T = {T} n = {n} S = {S}: {count} unflagged texels, max |N_f - truth| = {worst:.3g}, '
              f'decoded angle / bound = {ratio:.4f}')
        assert ratio <= 1.0
        total += count
        if S == 2 and T >= 65:
            assert (out['flags'] & nr.FLAT).any() and count > T          # the triangles wound the other way are creased
    assert total > 1000


# ------------------------------------------------------------------ the sphere
def sphere_case(baker=definition, n=5):
    verts, faces, h_c = nr.sphere_mesh()
    field, lo, h_f = nr.sphere_field(17)
    normals, tangents, creased, pts = _inputs(verts, faces, n)
    S = nr.steps(h_c, h_f)
    out = baker(verts, faces, normals, tangents, creased, pts, n, field, lo, h_f, np.float32(0.0), S)
    assert S == 4 and len(faces) > 100
    assert not (out['flags'] & nr.NO_CROSSING).any()
    p = pts.astype(np.float64)
    nh = nr.bake(verts, faces, normals, tangents, creased, pts, n, field, lo, h_f, np.float32(0.0), S)['nh']
    q = p + out['offset'].astype(np.float64)[..., None] * nh
    dist = lambda x: np.abs(np.sqrt(((x - nr.SPHERE_C) ** 2).sum(-1)) - nr.SPHERE_R)                       # noqa: E731
    assert ((dist(q) < dist(p)) | (dist(q) <= 0.05 * h_f)).all()
    radial = (p - nr.SPHERE_C) / np.sqrt(((p - nr.SPHERE_C) ** 2).sum(-1))[..., None]
    dec, _ = _decoded(out, faces, normals, tangents, n)
    geometry = nr.angle(nh, radial)
    mapped = nr.angle(dec, radial)
    field_n = nr.angle(out['normal'].astype(np.float64), radial)
    return {'offset_coarse_voxels': float(np.abs(out['offset']).max() / h_c), 'geometry_deg': np.degrees([geometry.mean(), geometry.max()]),
            'mapped_deg': np.degrees([mapped.mean(), mapped.max()]), 'field_deg': np.degrees([field_n.mean(), field_n.max()]),
            'flat': int((out['flags'] & nr.FLAT != 0).sum()), 'texels': int(out['flags'].size)}


def test_sphere():
    r = sphere_case()
    print(f"\n   sphere: {r['texels']} texels, {r['flat']} flat, largest |s| = {r['offset_coarse_voxels']:.3f} coarse voxels; to the "
          f"radial direction: N_f {r['field_deg'][0]:.3f} deg mean / {r['field_deg'][1]:.3f} max, the decoded map "
          f"{r['mapped_deg'][0]:.3f} / {r['mapped_deg'][1]:.3f}, the interpolated vertex normals {r['geometry_deg'][0]:.3f} / "
          f"{r['geometry_deg'][1]:.3f}")
    assert r['mapped_deg'][0] < r['geometry_deg'][0]


# ------------------------------------------------------------------ the flags
def _one_triangle(z=0.0, flip=False, area=True):
    verts = np.array([[0.1, 0.1, z], [0.3, 0.1, z], [0.1, 0.3, z]], np.float32)
    if not area:
        verts[2] = verts[1]
    faces = np.array([[0, 2, 1] if flip else [0, 1, 2]], np.int32)
    return verts, faces


def flag_cases(baker=definition, n=4):
    """-> {name: the flags of the P texels}: a field f = level + (z0 - z) whose surface is the plane z = z0, normal +z."""
    h, lo, shape = 0.125, np.array([-0.125, -0.125, -0.375]), (9, 8, 7)
    g = nr.grid_points(lo, h, shape)
    up = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (3, 1))

    def run(verts, faces, normals, field, S):
        tangents, creased = nr.corner_tangents(verts, faces, normals)
        pts, _ = tex.texel_points(verts, faces, n)
        return baker(verts, faces, normals, tangents, creased, pts, n, field, lo, h, np.float32(0.25), S)
    plane = (0.25 + (0.15625 - g[..., 2])).astype(np.float32)                # the surface at z = 0.15625 = 2.5 delta
    verts, faces = _one_triangle()
    out = {'reached': run(verts, faces, up, plane, 3)['flags'],              # 3 steps of 0.0625 reach 0.1875
           'one step short': run(verts, faces, up, plane, 2)['flags'],       # 2 steps end at 0.125
           'constant': run(verts, faces, up, np.full_like(plane, 0.5), 3)['flags']}
    holed = plane.copy()
    holed[4:6] = np.nan                                                      # the slabs z = 0.125 and 0.25 around the surface
    out['nan tap'] = run(verts, faces, up, holed, 3)['flags']
    far = plane.copy()
    far[6] = np.nan                                                          # only the gradient's upper sample meets a NaN
    out['nan at the gradient'] = run(verts, faces, up, far, 3)['flags']
    v0, f0 = _one_triangle(area=False)
    out['zero area'] = run(v0, f0, up, plane, 3)['flags']
    v1, f1 = _one_triangle(flip=True)
    out['normal behind'] = run(v1, f1, up, plane, 3)['flags']
    outside = verts + np.array([2.0, -1.0, 0.0], np.float32)                 # far outside the grid in x and y: the clamp serves it
    out['outside'] = run(outside, faces, up, plane, 3)['flags']
    res = run(outside, faces, up, plane, 3)
    assert np.abs(res['normal'] - np.array([0.0, 0.0, 1.0], np.float32)).max() == 0.0
    assert np.abs(res['offset'] - np.float32(0.15625)).max() <= 2.0 ** -24
    assert (res['atlas'] == nr.FLAT_CODE).all()                              # the normal is the vertex normal: (0, 0, 1) in its frame
    return out


def check_flags(f):
    assert (f['reached'] == 0).all() and (f['outside'] == 0).all()
    assert (f['one step short'] == nr.NO_CROSSING).all()
    assert (f['constant'] == nr.NO_CROSSING | nr.NO_GRADIENT).all()
    assert (f['nan tap'] & nr.NO_GRADIENT).all() and (f['nan at the gradient'] == nr.NO_GRADIENT).all()
    assert (f['zero area'] & nr.FLAT).all() and (f['normal behind'] == nr.FLAT).all()


def test_flags():
    check_flags(flag_cases())


def test_a_zero_vertex_normal_takes_the_face_direction():
    field, lo, h, level, truth = nr.plane_field()
    verts, faces = _one_triangle()
    zero = np.zeros((3, 3), np.float32)
    tangents, creased = nr.corner_tangents(verts, faces, zero)
    pts, _ = tex.texel_points(verts, faces, 4)
    out = nr.bake(verts, faces, zero, tangents, creased, pts, 4, field, lo, h, level, 4)
    assert creased.all() and (out['flags'] == nr.FACE_DIRECTION | nr.FLAT).all()
    assert np.abs(out['nh'] - np.array([0.0, 0.0, 1.0])).max() == 0.0 and np.abs(out['N_f'] - truth).max() <= 1e-12


def test_steps_and_a_face_index():
    assert nr.steps(0.25, 0.125) == 4 and nr.steps(0.26, 0.125) == 5 and nr.steps(1e-9, 0.125) == 1 and nr.steps(4.0, 0.125) == 64
    with pytest.raises(ValueError, match='S = 65 steps, outside 1..64'):
        nr.steps(4.01, 0.125)
    field, lo, h, level, _ = nr.plane_field()
    verts, faces = tex.welded_mesh(3)
    normals, tangents, creased, pts = _inputs(verts, faces, 4)
    bad = faces.copy()
    bad[1, 2] = len(verts)
    pts_bad, status = tex.texel_points(verts, bad, 4)
    out = nr.bake(verts, bad, normals, tangents, creased, pts_bad, 4, field, lo, h, level, 2)
    assert status == 1 and out['status'] == 1 and np.isnan(out['normal'][1]).all() and np.isnan(out['offset'][1]).all()
    assert (out['flags'][1] == 0).all() and np.isfinite(out['normal'][[0, 2]]).all()


# ------------------------------------------------------------------ the atlas and the tangents
@pytest.mark.parametrize('n', nr.CELLS)
def test_unowned_texels_are_flat_and_owned_ones_are_written(n):
    field, lo, h, level, _ = nr.plane_field()
    for T in (1, 3, 65):
        verts, faces = tex.welded_mesh(T, seed=n)
        out = nr.bake_mesh(verts, faces, n, field, lo, h, level, 2)
        C, _, W, H, P = tex.layout(T, n)
        own = np.zeros((H, W), bool)
        for t in range(T):
            x, y = tex.atlas_position(t, tex.owned(n), n, C)
            own[y, x] = True
        assert own.sum() == T * P and (out['atlas'][~own] == nr.FLAT_CODE).all()
        # every owned texel decodes to a unit vector of the upper half space, as the bake normalised it
        c = out['atlas'][own].astype(np.float64) / 127.5 - 1.0
        assert (c[:, 2] > 0).all() and np.abs(np.sqrt((c * c).sum(1)) - 1.0).max() <= np.sqrt(3.0) / 255.0 + 1e-12


def test_corner_tangents():
    from occnerf_amd import mesh
    seen = {0: 0, 1: 0}
    for T in (1, 2, 3, 64, 257):
        verts, faces = tex.welded_mesh(T, seed=T)
        normals = nr.vertex_normals(verts, faces)
        tangents, creased = nr.corner_tangents(verts, faces, normals)
        mine, mask = mesh.corner_tangents(verts, faces, normals, 8)
        assert mine.dtype == np.float32 and mine.tobytes() == tangents.tobytes() and np.array_equal(mask, creased)
        assert tangents.shape == (T, 3, 4) and (tangents[..., 3] == 1.0).all()
        v = verts.astype(np.float64)
        for t in np.nonzero(~creased)[0]:
            sigma = 1.0 if t % 2 == 0 else -1.0
            e2 = v[faces[t, 2]] - v[faces[t, 0]]
            e1 = v[faces[t, 1]] - v[faces[t, 0]]
            for c in range(3):
                # the properties hold for the float64 tangent of the definition; the stored float32 is within half an ulp
                N = normals[faces[t, c]].astype(np.float64)
                Tc = sigma * e1 - N * ((N @ (sigma * e1)) / (N @ N))
                Tc /= np.sqrt(Tc @ Tc)
                assert np.abs(tangents[t, c, :3].astype(np.float64) - Tc).max() <= 2.0 ** -24
                assert abs(np.sqrt(Tc @ Tc) - 1.0) <= 1e-12 and abs(Tc @ N) <= 1e-12 * max(1.0, N @ N)
                assert np.cross(N, Tc) @ (sigma * e2) > 0.0
            seen[int(t) % 2] += 1
    assert seen[0] > 50 and seen[1] > 50                                      # even and odd triangles
    # the chart's axes: texture_uv's column grows along sigma e1 and its row along sigma e2
    uv = tex.texture_uv(4, 8).astype(np.float64)
    for t in range(4):
        sigma = 1.0 if t % 2 == 0 else -1.0
        assert sigma * (uv[t, 1, 0] - uv[t, 0, 0]) > 0 and uv[t, 1, 1] == uv[t, 0, 1]
        assert sigma * (uv[t, 2, 1] - uv[t, 0, 1]) > 0 and uv[t, 2, 0] == uv[t, 0, 0]


# ------------------------------------------------------------------ the lit resolve on the host
def lit_case(name, n, flat=False):
    from tests import mesh_raster_restatement as mrr
    c = mrr.case_random(257) if name == 'random257' else mrr.CASES[name]()
    faces = c['faces']
    ok = ((faces >= 0) & (faces < len(c['pos']))).all(1)
    normals = -nr.vertex_normals(c['pos'], faces[ok])                        # towards the camera, so that the panels are not black
    tangents, _ = nr.corner_tangents(c['pos'], np.where(ok[:, None], faces, 0), normals)
    atlas, C = tex.random_atlas(len(faces), n, seed=7)
    if flat:
        atlas[:] = nr.FLAT_CODE
    return c, normals, tangents, atlas, C, nr.ray_matrix(c['K'], c['E'])


def test_resolve_lit_definition():
    from tests import mesh_raster_restatement as mrr
    c, normals, tangents, atlas, C, M = lit_case('grid', 4)
    r = mrr.run_case(c)
    geo, mapped = nr.resolve_lit(r['keys'], c['faces'], r['xy'], r['z'], normals, tangents, atlas, 4, C, M, (9, 8, 7))
    hit = r['keys'] != mrr.EMPTY_KEY
    assert hit.sum() > 500 and (geo[~hit] == (9, 8, 7)).all() and (mapped[~hit] == (9, 8, 7)).all()
    assert (geo[hit][:, 0] == geo[hit][:, 1]).all() and (geo[hit] != mapped[hit]).any() and geo[hit].max() > 100
    flat = np.empty_like(atlas)
    flat[:] = nr.FLAT_CODE
    geo2, mapped2 = nr.resolve_lit(r['keys'], c['faces'], r['xy'], r['z'], normals, tangents, flat, 4, C, M, (9, 8, 7))
    assert np.array_equal(geo2, geo) and np.array_equal(mapped2, geo)


# ------------------------------------------------------------------ the writer
def _png(atlas):
    from PIL import Image
    blob = io.BytesIO()
    Image.fromarray(atlas).save(blob, format='PNG')
    return blob.getvalue()


def test_write_glb_with_a_normal_map(tmp_path):
    from occnerf_amd import gltf, mesh
    v, f, c, j, w, g, nrm, anim, corr = cpu_tex.tiny_rig()
    T, n = f.shape[0], 5
    _, _, W, H, _ = mesh.atlas_layout(T, n)
    rng = np.random.RandomState(2)
    colour, normal = rng.randint(0, 256, (H, W, 3)).astype(np.uint8), rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    tangents, _ = mesh.corner_tangents(v, f, nrm, n)
    texture = {'uv': mesh.texture_uv(T, n), 'png': _png(colour), 'normal_png': _png(normal), 'tangents': tangents}
    path = str(tmp_path / 'rigged.glb')
    size = gltf.write_glb(path, v, f, c, j, w, g, normals=nrm, animation=anim, correctives=corr, fps=25.0, texture=texture)
    blob = open(path, 'rb').read()
    assert size == len(blob)
    doc, buf, att, image, image_n = nr.read_normal_mapped(blob)
    corner = f.reshape(-1)
    assert att['TANGENT'].shape == (3 * T, 4) and (att['TANGENT'][:, 3] == 1.0).all()
    assert att['TANGENT'].tobytes() == tangents.tobytes() and att['NORMAL'].tobytes() == nrm[corner].tobytes()
    assert np.array_equal(image, colour) and np.array_equal(image_n, normal)
    assert doc['materials'][0]['normalTexture']['index'] == 1 and len(doc['skins']) == 1
    assert len(doc['meshes'][0]['primitives'][0]['targets']) == 2
    # the static file
    gltf.write_glb(path, v, f, None, None, None, None, normals=nrm, texture=texture)
    doc, buf, att, image, image_n = nr.read_normal_mapped(open(path, 'rb').read())
    assert 'skins' not in doc and set(att) == {'POSITION', 'NORMAL', 'TANGENT', 'TEXCOORD_0'} and np.array_equal(image_n, normal)
    # without the two keys: the file the writer wrote before them
    plain = {'uv': texture['uv'], 'png': texture['png']}
    gltf.write_glb(path, v, f, None, None, None, None, normals=nrm, texture=plain)
    doc, buf, att, idx, image = tex.read_textured(open(path, 'rb').read())
    assert 'TANGENT' not in att and 'normalTexture' not in doc['materials'][0]
    assert cpu_tex.write_recorded(tmp_path / 'recorded') == [cpu_tex.PLAIN_SHA256, cpu_tex.FULL_SHA256]
    with pytest.raises(RuntimeError, match='go together'):
        gltf.write_glb(path, v, f, c, j, w, g, normals=nrm, texture={**plain, 'normal_png': texture['normal_png']})
    with pytest.raises(RuntimeError, match=r"texture\['tangents'\] must be float32 \[4,3,4\]"):
        gltf.write_glb(path, v, f, c, j, w, g, normals=nrm, texture={**texture, 'tangents': tangents[:3]})
    with pytest.raises(RuntimeError, match='a PNG file'):
        gltf.write_glb(path, v, f, c, j, w, g, normals=nrm, texture={**texture, 'normal_png': b'no'})
    with pytest.raises(RuntimeError, match='a normal map needs normals'):
        gltf.write_glb(path, v, f, c, j, w, g, texture=texture)


# ------------------------------------------------------------------ keys, refusals and wiring without a GPU
def test_keys_refusals_and_wiring():
    import torch

    from occnerf_amd import _lib, mesh, ops
    from occnerf_amd.config import default_cfg
    want = {'enable': False, 'resolution': None, 'cage': None, 'in_glb': True}
    assert dict(default_cfg().mesh_normal) == want == mesh.NORMAL_DEFAULTS
    cfg = default_cfg().merge_from_list(['mesh_normal.enable', 'True', 'mesh_normal.resolution', '32', 'mesh_normal.cage', '0.02',
                                         'mesh_normal.in_glb', 'False'])
    assert mesh.check_normal(cfg.mesh_normal) == {'enable': True, 'resolution': 32, 'cage': 0.02, 'in_glb': False}
    assert mesh.check_normal({}) == want
    for key, value, word in (('enable', 1, 'mesh_normal.enable = 1'), ('in_glb', 'yes', "mesh_normal.in_glb = 'yes'"),
                             ('resolution', 0, 'mesh_normal.resolution = 0'), ('resolution', 4096, 'mesh_normal.resolution = 4096'),
                             ('resolution', 64.0, 'mesh_normal.resolution'), ('resolution', True, 'mesh_normal.resolution'),
                             ('cage', 0.0, 'mesh_normal.cage = 0.0'), ('cage', -1.0, 'mesh_normal.cage'),
                             ('cage', float('nan'), 'mesh_normal.cage'), ('cage', float('inf'), 'mesh_normal.cage'),
                             ('cage', 'h', 'mesh_normal.cage'), ('cage', True, 'mesh_normal.cage')):
        with pytest.raises(RuntimeError, match=re.escape(word)):
            mesh.check_normal({**mesh.NORMAL_DEFAULTS, key: value})
    assert ops.mesh_normal_steps(0.25, 0.125) == 4 == nr.steps(0.25, 0.125)
    with pytest.raises(RuntimeError, match=r'takes S = 65 steps, outside 1\.\.64'):
        ops.mesh_normal_steps(4.01, 0.125)
    with pytest.raises(RuntimeError, match='must be positive finite lengths'):
        ops.mesh_normal_steps(0.0, 0.125)
    assert ops.MESH_NORMAL_FLAGS == {'no_crossing': nr.NO_CROSSING, 'no_gradient': nr.NO_GRADIENT, 'flat': nr.FLAT,
                                     'face_direction': nr.FACE_DIRECTION} and ops.MESH_NORMAL_FLAT == tuple(nr.FLAT_CODE)
    K, E = np.array([[50.0, 0, 32], [0, 60.0, 24], [0, 0, 1]]), np.eye(4)
    E[:3, :3] = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    assert np.array_equal(ops.mesh_ray_matrix(K, E), nr.ray_matrix(K, E))
    # the C entries refuse before any launch
    lib = _lib.lib()
    p = 4096
    lo3 = np.zeros(3).ctypes.data

    def refused(rc, who, word):
        msg = lib.occnerf_last_error().decode()
        assert rc != 0 and msg.startswith(who) and word in msg, (rc, msg)

    def bake(T=9, n=8, C=3, H=16, W=24, nx=9, ny=8, nz=7, h=0.125, S=4, field=p, lo=lo3, atlas=p, status=p, V=5):
        return lib.occnerf_mesh_normal_bake(p, p, V, p, T, p, p, p, n, C, H, W, field, nx, ny, nz, lo, h, 0.0, S, atlas, p, p, p, status, None)
    refused(bake(W=25), 'mesh_normal_bake', 'does not hold')
    refused(bake(H=8), 'mesh_normal_bake', 'does not hold')
    refused(bake(C=0, W=0), 'mesh_normal_bake', 'does not hold')
    refused(bake(n=3), 'mesh_normal_bake', 'n=3')
    refused(bake(n=65), 'mesh_normal_bake', 'n=65')
    refused(bake(nx=1), 'mesh_normal_bake', 'every axis needs two')
    refused(bake(nz=0), 'mesh_normal_bake', 'every axis needs two')
    refused(bake(nx=2048, ny=2048, nz=512), 'mesh_normal_bake', 'fewer than 2^31')
    refused(bake(S=0), 'mesh_normal_bake', 'S=0')
    refused(bake(S=65), 'mesh_normal_bake', 'S=65')
    refused(bake(h=0.0), 'mesh_normal_bake', 'h_f=0')
    refused(bake(T=(1 << 31) // 28 + 1, C=1 << 14, W=0), 'mesh_normal_bake', 'reaches 2^31')
    refused(bake(field=None), 'mesh_normal_bake', 'null')
    refused(bake(lo=None), 'mesh_normal_bake', 'null')
    refused(bake(status=None), 'mesh_normal_bake', 'null')
    refused(bake(V=-1), 'mesh_normal_bake', 'V=-1 outside')
    refused(bake(V=1 << 31), 'mesh_normal_bake', 'V=2147483648 outside')
    refused(bake(T=-1), 'mesh_normal_bake', 'T=-1')
    refused(bake(h=float('nan')), 'mesh_normal_bake', 'h_f=nan')
    refused(bake(h=float('inf')), 'mesh_normal_bake', 'h_f=inf')
    assert bake(T=0, field=None, atlas=None) == 0
    bg, M = np.zeros(3, np.uint8).ctypes.data, np.eye(3).ctypes.data

    def lit(keys=p, T=9, V=5, H=4, W=4, atlas=p, aH=16, aW=24, n=8, C=3, M=M, bg=bg, out=p, tangents=p):
        return lib.occnerf_mesh_resolve_lit(keys, p, T, V, p, p, H, W, p, tangents, atlas, aH, aW, n, C, M, bg, out, out, None)
    refused(lit(aW=25), 'mesh_resolve_lit', 'does not hold')
    refused(lit(aH=15), 'mesh_resolve_lit', 'does not hold')
    refused(lit(n=70), 'mesh_resolve_lit', 'n=70')
    refused(lit(H=0), 'mesh_resolve_lit', 'H=0')
    refused(lit(atlas=None), 'mesh_resolve_lit', 'null')
    refused(lit(tangents=None), 'mesh_resolve_lit', 'null')
    refused(lit(M=None), 'mesh_resolve_lit', 'null')
    refused(lit(bg=None), 'mesh_resolve_lit', 'null')
    refused(lit(keys=None), 'mesh_resolve_lit', 'null')
    refused(lit(out=None), 'mesh_resolve_lit', 'null')
    refused(lit(T=-1), 'mesh_resolve_lit', 'T=-1 outside')
    refused(lit(T=1 << 31), 'mesh_resolve_lit', 'T=2147483648 outside')
    refused(lit(V=-1), 'mesh_resolve_lit', 'V=-1 outside')
    refused(lit(V=1 << 31), 'mesh_resolve_lit', 'V=2147483648 outside')
    refused(lit(n=3), 'mesh_resolve_lit', 'n=3')
    refused(lit(H=16385), 'mesh_resolve_lit', 'H=16385')
    # the wrappers refuse host tensors by name
    z3 = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match='mesh_normal_bake: verts must be a CUDA'):
        ops.mesh_normal_bake(z3, z3, torch.zeros(1, 3, dtype=torch.int32), None, None, None, 8, 1, None, None, [0, 0, 0], 0.1, 0.0, 2)
    with pytest.raises(RuntimeError, match='mesh_normal_bake: cell = 3'):
        ops.mesh_normal_bake(z3, z3, torch.zeros(1, 3, dtype=torch.int32), None, None, None, 3, 1, None, None, [0, 0, 0], 0.1, 0.0, 2)
    with pytest.raises(RuntimeError, match='mesh_resolve_lit: keys must be a CUDA'):
        ops.mesh_resolve_lit(torch.zeros(4, 4, dtype=torch.int64), None, None, None, None, None, None, 8, 1, np.eye(3), (0, 0, 0))
    run = open(os.path.join(ROOT, 'run.py')).read()
    assert 'export_normal_map(' in run and "mnor.get('enable', False)" in run and 'mesh_normal.enable' in run
    assert 'mesh_normal.enable: the normal map lies on the atlas of mesh_texture.enable' in run and 'mesh_normal.in_glb: glTF' in run
    make = open(os.path.join(ROOT, 'occnerf_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bmesh_normal\.hip\b', make, flags=re.M)
    for name in ('mesh_texture.hip', 'mesh_normal.hip'):                      # the atlas' layout is shared, not copied
        src = open(os.path.join(ROOT, 'occnerf_amd', 'csrc', name)).read()
        assert '#include "mesh_atlas.h"' in src and 'void texel_of(' not in src and 'void atlas_of(' not in src
