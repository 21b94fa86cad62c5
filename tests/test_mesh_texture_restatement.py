"""CPU: the numpy definition of the mesh's texture (tests/mesh_texture_restatement.py) keeps its claims --
a chart is closed under bilinear filtering, the layout puts every owned texel at a place of its own, the corner texels are the
vertices, an affine colour comes back within a derived bound --, and occnerf_amd.gltf.write_glb writes the bytes it wrote before
without texture= and a file that parses with it."""
import hashlib
import io
import os

import numpy as np
import pytest

from tests import mesh_texture_restatement as tex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _edge_and_corner_barycentrics(steps=257):
    s = np.linspace(0.0, 1.0, steps)
    z = np.zeros_like(s)
    return np.concatenate([np.stack([1.0 - s, s, z], 1), np.stack([z, 1.0 - s, s], 1), np.stack([s, z, 1.0 - s], 1), np.eye(3)])


@pytest.mark.parametrize('n', (4, 5, 8, 16, 64))
def test_a_chart_is_closed_under_bilinear_filtering(n):
    """20 K random barycentric points, the three edges and the corners through the sampler's own x, y: every tap with a non-zero
    weight is a texel its own triangle owns; the two halves of a cell share no texel and each holds n (n - 1) / 2."""
    w = np.concatenate([tex.interior_barycentrics(20000, seed=n), _edge_and_corner_barycentrics()])
    assert tex.closed_taps(w[:, 1], w[:, 2], n)
    # weights a hair outside the triangle (what a rasteriser's rounding can hand over) are clamped onto it
    assert tex.closed_taps(w[:, 1] + 1e-12, w[:, 2] + 1e-12, n) and tex.closed_taps(w[:, 1] - 1e-12, w[:, 2] - 1e-12, n)
    own = tex.owned(n)
    assert own.shape == (n * (n - 1) // 2, 2) and (own.sum(1) <= n - 2).all()
    order = own[:, 1] * n + own[:, 0]
    assert (np.diff(order) > 0).all()                                      # ascending j', then ascending i'
    lower = {tuple(p) for p in tex.cell_position(0, own, n).tolist()}
    upper = {tuple(p) for p in tex.cell_position(1, own, n).tolist()}
    assert len(lower) == len(upper) == n * (n - 1) // 2 and not (lower & upper)
    nobody = {(i, j) for i in range(n) for j in range(n)} - lower - upper
    assert nobody == {(i, n - 1 - i) for i in range(n)}                    # the anti-diagonal


@pytest.mark.parametrize('T', (1, 2, 3, 7, 8, 9, 353444))
def test_layout(T):
    from occnerf_amd import mesh
    for n in (4, 8, 13):
        C, R, W, H, P = mesh.atlas_layout(T, n)
        assert (C, R, W, H, P) == tex.layout(T, n)
        cells = (T + 1) // 2
        assert C * C >= cells > (C - 1) * (C - 1) and C * R >= cells > C * (R - 1) and (W, H, P) == (C * n, R * n, n * (n - 1) // 2)
    n = 5
    C, R, W, H, P = tex.layout(T, n)
    own = tex.owned(n)
    some = range(T) if T < 100 else list(range(0, T, 997)) + [T - 2, T - 1]
    seen = np.zeros((H, W), np.int32)
    for t in some:
        x, y = tex.atlas_position(t, own, n, C)
        assert x.min() >= 0 and y.min() >= 0 and x.max() < W and y.max() < H
        assert (x // n == (t >> 1) % C).all() and (y // n == (t >> 1) // C).all()
        seen[y, x] += 1
    assert seen.max() == 1 and int(seen.sum()) == len(some) * P          # every owned texel at a place of its own


def test_the_side_limit_is_refused():
    from occnerf_amd import mesh
    T = 2 * 257 * 256                                                    # 257 cells per row at 64 texels: 16448
    assert mesh.atlas_layout(2 * 256 * 256, 64)[2:4] == (16384, 16384)
    with pytest.raises(RuntimeError, match='an atlas of 16448 x 16384 texels .* exceeds 16384'):
        mesh.atlas_layout(T, 64)
    with pytest.raises(ValueError, match='exceeds 16384'):
        tex.layout(T, 64)
    for n in (3, 65, 8.0, True):
        with pytest.raises(RuntimeError, match='cell = .* is not a whole number in 4..64'):
            mesh.atlas_layout(10, n)
    with pytest.raises(RuntimeError, match='T = 0: a mesh without triangles has no atlas'):
        mesh.atlas_layout(0, 8)


@pytest.mark.parametrize('n', tex.CELLS)
def test_corner_texels_are_the_vertices(n):
    from occnerf_amd import mesh
    T = 65
    verts, faces = tex.welded_mesh(T)
    pts, status = tex.texel_points(verts, faces, n)
    assert status == 0 and pts.dtype == np.float32 and pts.shape == (T, n * (n - 1) // 2, 3)
    own, m = tex.owned(n), n - 3
    C, _, W, H, _ = tex.layout(T, n)
    uv = mesh.texture_uv(T, n)
    assert uv.dtype == np.float32 and uv.shape == (T, 3, 2) and np.array_equal(uv.view(np.uint32), tex.texture_uv(T, n).view(np.uint32))
    assert uv.min() > 0.0 and uv.max() < 1.0
    for corner, ij in enumerate(((0, 0), (m, 0), (0, m))):
        k = int(np.nonzero((own == ij).all(1))[0][0])
        assert np.array_equal(pts[:, k].view(np.uint32), verts[faces[:, corner]].view(np.uint32))
        for t in (0, 1, 2, T - 1):
            x, y = tex.atlas_position(t, np.array(ij), n, C)
            assert uv[t, corner, 0] == np.float32((x + 0.5) / W) and uv[t, corner, 1] == np.float32((y + 0.5) / H)
    bad = faces.copy()
    bad[3, 1] = verts.shape[0]
    pts2, status = tex.texel_points(verts, bad, n)
    assert status == 1 and np.isnan(pts2[3]).all() and np.array_equal(np.delete(pts2, 3, 0).view(np.uint32), np.delete(pts, 3, 0).view(np.uint32))


def test_fill_is_to_8b_image():
    from occnerf_amd.image import to_8b_image
    c = np.random.RandomState(3).uniform(-0.2, 1.2, 20000).astype(np.float32)
    assert np.array_equal(tex.to_byte(c), to_8b_image(c))
    assert tex.to_byte(np.array([np.nan, 0.0, -0.0, 1.0, 2.0, -1.0], np.float32)).tolist() == [0, 0, 0, 255, 255, 0]


def affine_case(T, n, points=lambda v, f, n: tex.texel_points(v, f, n)[0], fill=None, sampler=None):
    """The affine reproduction through a (points, fill) pair -> (max |byte - 255 c(p)|, the bound); the GPU test hands in the
    kernels."""
    verts, faces = tex.welded_mesh(T, seed=n)
    C, _, W, H, P = tex.layout(T, n)
    pts = points(verts, faces, n)
    a, b = tex.affine_colour(pts, seed=n)
    colour = (pts.astype(np.float64).reshape(-1, 3) @ a.T + b).astype(np.float32)
    assert colour.min() >= np.float32(0.1) - 1e-6 and colour.max() <= np.float32(0.9) + 1e-6
    atlas = np.full((H, W, 3), 7, np.uint8)
    atlas = (fill or (lambda rgb, T, n, C, atlas: tex.fill(rgb, T, n, C, atlas)))(colour, T, n, C, atlas)
    w = tex.interior_barycentrics(400, seed=T)
    worst = 0.0
    for t in range(T):
        tri = verts[faces[t]].astype(np.float64)
        p = w @ tri
        want = 255.0 * (p @ a.T + b)
        got = tex.sample(atlas, t, w[:, 1], w[:, 2], n, C).astype(np.float64)
        worst = max(worst, float(np.abs(got - want).max()))
    return worst, tex.affine_bound(a, pts)


@pytest.mark.parametrize('n', tex.CELLS)
def test_an_affine_colour_comes_back_within_the_derived_bound(n):
    """c(p) = a . p + b in [0.1, 0.9] on every texel point: texel points, fill, then the sampler at 400 random interior points of
    every triangle.  |byte - 255 c(p)| <= 1.5 + 255 eps (tests/mesh_texture_restatement.py affine_bound: 1 for the fill's
    truncation, 0.5 for the sampler's rounding, eps = 2^-24 (sum_c |a_c| max|p_c| + 2) + 2^-45 (...) for the float32 rounding
    of the texel positions carried through a, of the colour and of its product with 255)."""
    worst, bound = affine_case(9, n)
    print(f'\n   n = {n}: max |byte - 255 c(p)| = {worst:.4f}, bound {bound:.6f}')
    assert 1.5 < bound < 1.51 and worst <= bound


# ------------------------------------------------------------------ the glTF writer
def tiny_rig():
    rng = np.random.RandomState(7)
    verts = rng.uniform(-1, 1, (6, 3)).astype(np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 5], [0, 5, 4]], np.int32)
    colors = rng.randint(0, 256, (6, 3)).astype(np.uint8)
    joints = rng.randint(0, 24, (6, 4)).astype(np.uint8)
    w = rng.uniform(0.1, 1, (6, 4))
    weights = (w / w.sum(1, keepdims=True)).astype(np.float32)
    g = np.tile(np.eye(4), (24, 1, 1))
    g[:, :3, 3] = rng.uniform(-1, 1, (24, 3))
    normals = rng.normal(size=(6, 3)).astype(np.float32)
    q = rng.normal(size=(2, 24, 4))
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    anim = {'rotation': q, 'translation': rng.uniform(-1, 1, (2, 24, 3))}
    corr = rng.uniform(-.01, .01, (2, 6, 3)).astype(np.float32)
    return verts, faces, colors, joints, weights, g.astype(np.float32), normals, anim, corr


# sha256 of the two files below as the writer of the commit before texture= and joints=None wrote them
PLAIN_SHA256 = 'c277335083c22c9328a0f89043b59af45159a104f0a15a0ccc13c05ecc329b18'
FULL_SHA256 = 'cb5bb3506980ab64318e27324cb1ccbfd34bdc1e6031a9c8c3e220e15c5894f1'


def write_recorded(folder):
    """The two recorded calls -> the files' sha256."""
    from occnerf_amd import gltf
    v, f, c, j, w, g, nrm, anim, corr = tiny_rig()
    os.makedirs(str(folder), exist_ok=True)
    gltf.write_glb(os.path.join(str(folder), 'a.glb'), v, f, c, j, w, g)
    gltf.write_glb(os.path.join(str(folder), 'b.glb'), v, f, c, j, w, g, normals=nrm, animation=anim, correctives=corr, fps=25.0)
    return [hashlib.sha256(open(os.path.join(str(folder), x), 'rb').read()).hexdigest() for x in ('a.glb', 'b.glb')]


def test_write_glb_without_texture_writes_the_bytes_it_wrote(tmp_path):
    assert write_recorded(tmp_path) == [PLAIN_SHA256, FULL_SHA256]


def _png(atlas):
    from PIL import Image
    blob = io.BytesIO()
    Image.fromarray(atlas).save(blob, format='PNG')
    return blob.getvalue()


def test_write_glb_with_a_texture(tmp_path):
    from occnerf_amd import gltf, mesh
    v, f, c, j, w, g, nrm, anim, corr = tiny_rig()
    T, n = f.shape[0], 5
    _, _, W, H, _ = mesh.atlas_layout(T, n)
    atlas = np.random.RandomState(1).randint(0, 256, (H, W, 3)).astype(np.uint8)
    texture = {'uv': mesh.texture_uv(T, n), 'png': _png(atlas)}
    path = str(tmp_path / 'rigged.glb')
    size = gltf.write_glb(path, v, f, c, j, w, g, normals=nrm, animation=anim, correctives=corr, fps=25.0, texture=texture)
    blob = open(path, 'rb').read()
    assert size == len(blob)
    gltf.write_glb(str(tmp_path / 'again.glb'), v, f, None, j, w, g, normals=nrm, animation=anim, correctives=corr, fps=25.0, texture=texture)
    assert blob == open(str(tmp_path / 'again.glb'), 'rb').read()            # the colours are not read
    doc, buf, att, idx, image = tex.read_textured(blob)
    corner = f.reshape(-1)
    assert all(a.shape[0] == 3 * T for a in att.values()) and idx.shape[0] == 3 * T
    assert np.array_equal(image, atlas)
    uv = att['TEXCOORD_0']
    assert uv.min() > 0.0 and uv.max() < 1.0 and uv.tobytes() == texture['uv'].tobytes()
    assert att['POSITION'].tobytes() == v[corner].tobytes() and att['NORMAL'].tobytes() == nrm[corner].tobytes()
    assert np.array_equal(att['JOINTS_0'], j[corner]) and att['WEIGHTS_0'].tobytes() == w[corner].tobytes()
    prim = doc['meshes'][0]['primitives'][0]
    for k in range(2):
        assert tex.accessor(doc, buf, prim['targets'][k]['POSITION']).tobytes() == corr[k][corner].tobytes()
    assert len(doc['skins']) == 1 and len(doc['animations']) == 1 and doc['nodes'][0] == {'name': 'body', 'mesh': 0, 'skin': 0}
    # the static variant
    path = str(tmp_path / 'textured.glb')
    gltf.write_glb(path, v, f, None, None, None, None, normals=nrm, texture=texture)
    doc, buf, att, idx, image = tex.read_textured(open(path, 'rb').read())
    assert 'skins' not in doc and 'animations' not in doc and doc['nodes'] == [{'name': 'body', 'mesh': 0}]
    assert doc['scenes'] == [{'nodes': [0]}] and set(att) == {'POSITION', 'NORMAL', 'TEXCOORD_0'}
    assert att['POSITION'].tobytes() == v[corner].tobytes() and np.array_equal(image, atlas)
    # a static mesh with vertex colours, and the refusals
    gltf.write_glb(path, v, f, c, None, None, None)
    doc, buf = tex.parse_glb(open(path, 'rb').read())
    assert 'skins' not in doc and 'COLOR_0' in doc['meshes'][0]['primitives'][0]['attributes'] and 'images' not in doc
    with pytest.raises(RuntimeError, match='a mesh without joints is static'):
        gltf.write_glb(path, v, f, c, None, None, None, animation=anim)
    with pytest.raises(RuntimeError, match=r"texture\['uv'\] must be float32 \[4,3,2\]"):
        gltf.write_glb(path, v, f, c, j, w, g, texture={'uv': texture['uv'][:3], 'png': texture['png']})
    with pytest.raises(RuntimeError, match='a PNG file'):
        gltf.write_glb(path, v, f, c, j, w, g, texture={'uv': texture['uv'], 'png': b'not a png'})


# ------------------------------------------------------------------ keys, refusals and wiring without a GPU
def test_keys_refusals_and_wiring():
    import re

    import torch

    from occnerf_amd import _lib, mesh, ops
    from occnerf_amd.config import default_cfg
    assert dict(default_cfg().mesh_texture) == {'enable': False, 'cell': 8, 'fill': [0, 0, 0]} == mesh.TEXTURE_DEFAULTS
    cfg = default_cfg().merge_from_list(['mesh_texture.enable', 'True', 'mesh_texture.cell', '5', 'mesh_texture.fill', '[255, 0, 255]'])
    assert mesh.check_texture(cfg.mesh_texture) == {'enable': True, 'cell': 5, 'fill': [255, 0, 255]}
    for key, value, word in (('cell', 3, 'mesh_texture.cell = 3'), ('cell', 65, 'mesh_texture.cell = 65'), ('cell', 8.0, 'mesh_texture.cell'),
                             ('cell', True, 'mesh_texture.cell'), ('enable', 1, 'mesh_texture.enable = 1'),
                             ('fill', [0, 0], 'mesh_texture.fill'), ('fill', [0, 0, 256], 'mesh_texture.fill'),
                             ('fill', [0.5, 0, 0], 'mesh_texture.fill'), ('fill', 'black', 'mesh_texture.fill')):
        with pytest.raises(RuntimeError, match=re.escape(word)):
            mesh.check_texture({**mesh.TEXTURE_DEFAULTS, key: value})
    # the C entries refuse before any launch
    lib = _lib.lib()
    p = 4096

    def refused(rc, who, word):
        msg = lib.occnerf_last_error().decode()
        assert rc != 0 and msg.startswith(who) and word in msg, (rc, msg)
    refused(lib.occnerf_mesh_texel_points(p, 3, p, 1, 3, p, p, None), 'mesh_texel_points', 'n=3')
    refused(lib.occnerf_mesh_texel_points(p, 3, p, 1, 65, p, p, None), 'mesh_texel_points', 'n=65')
    refused(lib.occnerf_mesh_texel_points(p, 3, p, (1 << 31) // 28 + 1, 8, p, p, None), 'mesh_texel_points', 'reaches 2^31')
    refused(lib.occnerf_mesh_texel_points(p, 3, None, 1, 8, p, p, None), 'mesh_texel_points', 'null')
    refused(lib.occnerf_mesh_texel_points(p, 3, p, 1, 8, p, None, None), 'mesh_texel_points', 'null')
    assert lib.occnerf_mesh_texel_points(None, 0, None, 0, 8, None, None, None) == 0
    refused(lib.occnerf_mesh_texture_fill(p, 9, 8, 3, 16, 25, p, None), 'mesh_texture_fill', 'does not hold')        # W != C n
    refused(lib.occnerf_mesh_texture_fill(p, 9, 8, 3, 8, 24, p, None), 'mesh_texture_fill', 'does not hold')         # a row short
    refused(lib.occnerf_mesh_texture_fill(p, 9, 8, 0, 16, 0, p, None), 'mesh_texture_fill', 'does not hold')
    refused(lib.occnerf_mesh_texture_fill(None, 9, 8, 3, 16, 24, p, None), 'mesh_texture_fill', 'null')
    refused(lib.occnerf_mesh_texture_fill(p, 9, 2, 3, 16, 24, p, None), 'mesh_texture_fill', 'n=2')
    bg = (np.zeros(3, np.uint8)).ctypes.data

    def resolve(keys=p, T=9, V=5, H=4, W=4, atlas=p, aH=16, aW=24, n=8, C=3, bg=bg, rgb=p):
        return lib.occnerf_mesh_resolve_textured(keys, p, T, V, p, p, H, W, atlas, aH, aW, n, C, bg, rgb, None)
    refused(resolve(aW=25), 'mesh_resolve_textured', 'does not hold')
    refused(resolve(aH=15), 'mesh_resolve_textured', 'does not hold')
    refused(resolve(C=2, aW=16), 'mesh_resolve_textured', 'does not hold')       # 5 cells in rows of 2: 3 rows, 24 > 16
    refused(resolve(n=70), 'mesh_resolve_textured', 'n=70')
    refused(resolve(H=0), 'mesh_resolve_textured', 'H=0')
    refused(resolve(atlas=None), 'mesh_resolve_textured', 'null')
    refused(resolve(bg=None), 'mesh_resolve_textured', 'null')
    refused(resolve(keys=None), 'mesh_resolve_textured', 'null')
    # the wrappers refuse host tensors by name
    with pytest.raises(RuntimeError, match='mesh_texel_points: verts must be a CUDA'):
        ops.mesh_texel_points(torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32), 8)
    with pytest.raises(RuntimeError, match='mesh_texture_fill: rgb must be a CUDA'):
        ops.mesh_texture_fill(torch.zeros(28, 3), 1, 8, 1, torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='mesh_resolve_textured: keys must be a CUDA'):
        ops.mesh_resolve_textured(torch.zeros(4, 4, dtype=torch.int64), None, None, None, None, 8, 1, (0, 0, 0))
    with pytest.raises(RuntimeError, match='mesh_texel_points: cell = 3'):
        ops.mesh_texel_points(torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32), 3)
    run = open(os.path.join(ROOT, 'run.py')).read()
    assert 'export_texture(' in run and "mtex.get('enable', False)" in run and 'mesh_texture.enable' in run
    make = open(os.path.join(ROOT, 'occnerf_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bmesh_texture\.hip\b', make, flags=re.M)
