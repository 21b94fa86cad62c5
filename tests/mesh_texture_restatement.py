"""The numpy definition of the texture of the exported mesh: a per-triangle atlas, the canonical points of
its texels, the bytes written into it and the bilinear sampler that reads it back.  csrc/mesh_texture.hip must give these bits.

With n = the cell edge in texels (4 <= n <= 64) and m = n - 3:

  layout    triangles 2c and 2c + 1 share cell c, n x n texels, at column c % C and row c // C of the atlas;
            C = ceil(sqrt(ceil(T / 2))), R = ceil(ceil(T / 2) / C), W = C n, H = R n, uint8 RGB; W or H above 16384 is refused.
  owner     texel (i, j) of a cell (i the column, j the row) belongs to the even triangle when i + j <= n - 2 and to the odd one
            when i' + j' <= n - 2 with i' = n - 1 - i, j' = n - 1 - j (the even triangle's frame is the cell's: i' = i, j' = j).
            The anti-diagonal i + j = n - 1 belongs to nobody.  Every triangle owns P = n (n - 1) / 2 texels, numbered
            k = 0 .. P - 1 by ascending j', then ascending i'.
  point     texel (i', j') of triangle (v0, v1, v2) stands for the barycentric numerators (m - i' - j', i', j') over m:
            float32(((f64(m - i' - j') v0 + f64(i') v1) + f64(j') v2) / f64(m)) per coordinate, in float64 on the float32
            vertices, one rounding per operator.  The corners are the texels (0, 0), (m, 0), (0, m) and reproduce their vertices
            (m v is exact, the other products are zeros; a coordinate -0.0 comes out +0.0); the rim i' + j' = m + 1 is a linear
            extrapolation one texel beyond the triangle.  A face with an index outside [0, V): NaN rows, status 1.
  fill      an owned texel's byte is uint8(float32(255) * min(max(c, 0), 1)) with the product in float32 and truncation --
            image.to_8b_image on a float32 array --, 0 for a NaN.  Nothing else of the atlas is written.
  sample    for barycentric weights (w0, w1, w2) of a triangle: x = min(max(w1 m, 0), m), y = min(max(w2 m, 0), m - x) in its own
            frame; taps (floor x + {0, 1}, floor y + {0, 1}) clamped to [0, n - 1]; ax = x - floor x, ay = y - floor y; weights
            (1 - ax)(1 - ay), ax (1 - ay), (1 - ax) ay, ax ay; per channel s = ((w00 c00 + w10 c10) + w01 c01) + w11 c11 in
            float64; the byte is min(max(rint(s), 0), 255).
  resolve   per pixel of mesh_raster's keys: the winner t and the perspective-correct weights exactly as
            tests/mesh_raster_restatement.py resolve states them; that file re-orders vertices 1 and 2 of a triangle of negative
            area, and the weights are put back into the face's own order before they are sampled.  A vertex with z = 0 is a
            flagged one (mesh_project gives every other z >= 1e-3): the vflag array is not needed.  Empty: the background.

Why no gutter is needed: x + y <= m, so floor x + floor y <= m; below m the four taps have i' + j' <= m + 1 = n - 2, the owner's
own texels (the rim exists for them), and at m the fractions are 0, so the taps beyond the rim have weight 0.  closed_taps
states it as a check, which the CPU test runs."""
import json
import struct

import numpy as np

from tests import mesh_raster_restatement as mrr

MIN_CELL, MAX_CELL = 4, 64
MAX_SIDE = 16384


def check_cell(n):
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or not MIN_CELL <= int(n) <= MAX_CELL:
        raise ValueError(f'mesh_texture: cell = {n!r} is not a whole number in {MIN_CELL}..{MAX_CELL}')
    return int(n)


def isqrt_ceil(v):
    r = int(np.floor(np.sqrt(float(v))))
    while r * r > v:
        r -= 1
    while r * r < v:
        r += 1
    return r


def layout(T, n):
    """-> (C, R, W, H, P)."""
    T, n = int(T), check_cell(n)
    if T < 1:
        raise ValueError(f'mesh_texture: T = {T}: a mesh without triangles has no atlas')
    cells = (T + 1) // 2
    C = isqrt_ceil(cells)
    R = (cells + C - 1) // C
    W, H = C * n, R * n
    if W > MAX_SIDE or H > MAX_SIDE:
        raise ValueError(f'mesh_texture: an atlas of {W} x {H} texels for {T} triangles at cell {n} exceeds {MAX_SIDE}')
    return C, R, W, H, n * (n - 1) // 2


def owned(n):
    """int64 [P,2]: (i', j') of texel k, by ascending j' then ascending i'."""
    n = check_cell(n)
    return np.array([(i, j) for j in range(n - 1) for i in range(n - 1 - j)], dtype=np.int64)


def cell_position(t, ij, n):
    """(i, j) inside the cell of the texels ij [..,2] (own frame) of triangle t: mirrored for an odd t."""
    ij = np.asarray(ij, dtype=np.int64)
    return (n - 1 - ij) if int(t) & 1 else ij


def atlas_position(t, ij, n, C):
    """(column x, row y) in the atlas of the texels ij [..,2] (own frame) of triangle t."""
    c = int(t) >> 1
    p = cell_position(t, ij, n)
    return p[..., 0] + (c % C) * n, p[..., 1] + (c // C) * n


def texel_points(verts, faces, n):
    """-> (pts float32 [T,P,3], status 0 / 1)."""
    n = check_cell(n)
    m = n - 3
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    V, T = v.shape[0], f.shape[0]
    ij = owned(n)
    if T == 0:
        return np.zeros((0, ij.shape[0], 3), np.float32), 0
    bad = ((f < 0) | (f >= V)).any(1)
    tri = v[np.where(bad[:, None], 0, f)].astype(np.float64) if V else np.zeros((T, 3, 3))
    b0 = (m - ij[:, 0] - ij[:, 1]).astype(np.float64)[None, :, None]
    b1, b2 = ij[:, 0].astype(np.float64)[None, :, None], ij[:, 1].astype(np.float64)[None, :, None]
    with np.errstate(all='ignore'):
        p = ((b0 * tri[:, None, 0, :] + b1 * tri[:, None, 1, :]) + b2 * tri[:, None, 2, :]) / np.float64(m)
    pts = p.astype(np.float32)
    pts[bad] = np.nan
    return pts, int(bad.any())


def to_byte(c):
    """image.to_8b_image's rule on float32, NaN -> 0."""
    c = np.asarray(c, dtype=np.float32)
    with np.errstate(all='ignore'):
        s = np.float32(255.0) * np.minimum(np.maximum(c, np.float32(0.0)), np.float32(1.0))
    return np.where(np.isnan(c), np.float32(0.0), s).astype(np.uint8)


def fill(rgb, T, n, C, atlas):
    """The owned texels of the T triangles written into atlas uint8 [H,W,3] (in place) from rgb float32 [T P,3] -> atlas."""
    ij = owned(n)
    b = to_byte(np.asarray(rgb, dtype=np.float32).reshape(T, ij.shape[0], 3))
    for t in range(T):
        x, y = atlas_position(t, ij, n, C)
        atlas[y, x] = b[t]
    return atlas


def corner_texels(T, n, C):
    """int64 [T,3,2]: the atlas (column, row) of the three corner texels of every triangle."""
    m = n - 3
    own = np.array([[0, 0], [m, 0], [0, m]], dtype=np.int64)
    out = np.zeros((T, 3, 2), np.int64)
    for t in range(T):
        out[t, :, 0], out[t, :, 1] = atlas_position(t, own, n, C)
    return out


def texture_uv(T, n):
    """float32 [T,3,2]: ((x + 0.5) / W, (y + 0.5) / H) of the corner texels, in float64 rounded once."""
    C, _, W, H, _ = layout(T, n)
    c = corner_texels(T, n, C).astype(np.float64)
    return np.stack([(c[..., 0] + 0.5) / np.float64(W), (c[..., 1] + 0.5) / np.float64(H)], -1).astype(np.float32)


def sample_xy(w1, w2, n):
    m = np.float64(n - 3)
    x = np.minimum(np.maximum(np.asarray(w1, np.float64) * m, 0.0), m)
    y = np.minimum(np.maximum(np.asarray(w2, np.float64) * m, 0.0), m - x)
    return x, y


def taps(x, y, n):
    """-> (ij int64 [...,4,2] in the own frame, order 00, 10, 01, 11; weights float64 [...,4])."""
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = x - fx, y - fy
    i0, j0 = fx.astype(np.int64), fy.astype(np.int64)
    ii = np.clip(np.stack([i0, i0 + 1, i0, i0 + 1], -1), 0, n - 1)
    jj = np.clip(np.stack([j0, j0, j0 + 1, j0 + 1], -1), 0, n - 1)
    w = np.stack([(1.0 - ax) * (1.0 - ay), ax * (1.0 - ay), (1.0 - ax) * ay, ax * ay], -1)
    return np.stack([ii, jj], -1), w


def closed_taps(w1, w2, n):
    """True when every tap with a non-zero weight of the sample points lies in the owner's set i' + j' <= n - 2."""
    ij, w = taps(*sample_xy(w1, w2, n), n)
    inside = (ij[..., 0] + ij[..., 1] <= n - 2) & (ij >= 0).all(-1)
    return bool((inside | (w == 0.0)).all())


def sample(atlas, t, w1, w2, n, C):
    """uint8 [...,3]: the atlas read at the barycentric weights (w1, w2 arrays) of triangle t."""
    ij, w = taps(*sample_xy(w1, w2, n), n)
    x, y = atlas_position(t, ij, n, C)
    c = atlas[y, x].astype(np.float64)                                   # [...,4,3]
    s = ((w[..., 0, None] * c[..., 0, :] + w[..., 1, None] * c[..., 1, :]) + w[..., 2, None] * c[..., 2, :]) + \
        w[..., 3, None] * c[..., 3, :]
    return np.minimum(np.maximum(np.rint(s), 0.0), 255.0).astype(np.uint8)


def resolve_textured(keys, faces, xy, z, atlas, n, C, bgcolor):
    """-> rgb uint8 [H,W,3] of mesh_raster's keys uint64 [H,W]."""
    H, W = keys.shape
    faces = np.asarray(faces).reshape(-1, 3)
    z = np.asarray(z, dtype=np.float64)
    vflag = np.where(z > 0.0, 0, 1).astype(np.uint8)
    reason, idx, A = mrr.setup(faces, xy, vflag)
    T = faces.shape[0]
    rgb = np.empty((H, W, 3), dtype=np.uint8)
    rgb[:] = np.asarray(bgcolor, dtype=np.uint8).reshape(3)
    for i, j in zip(*np.nonzero(keys != mrr.EMPTY_KEY)):
        t = int(keys[i, j] & np.uint64(0xFFFFFFFF))
        if t >= T or reason[t] != 0:
            continue
        v = idx[t]
        e, _ = mrr.edges(xy[v, 0].astype(np.int64), xy[v, 1].astype(np.int64), np.int64(256 * j), np.int64(256 * i))
        q, iz = mrr.inverse_depth(e, A[t], z[v])
        w = [q[k] / iz for k in range(3)]
        flipped = int(v[1]) != int(faces[t, 1])
        w1, w2 = (w[2], w[1]) if flipped else (w[1], w[2])
        rgb[i, j] = sample(atlas, t, np.float64(w1), np.float64(w2), n, C)
    return rgb


# ------------------------------------------------------------------ the cases the CPU and the GPU tests share
T_SIZES = (1, 2, 3, 63, 64, 65, 257)
CELLS = (4, 5, 8, 16)


def welded_mesh(T, seed=0):
    """(verts float32 [V,3], faces int32 [T,3]): the first T triangles of a grid mesh (mesh_raster_restatement.grid_mesh: shared
    vertices, mixed windings) with its vertices jittered in 3-D."""
    nx = max(1, int(np.ceil(np.sqrt(T / 2.0))))
    ny = max(1, -(-T // (2 * nx)))
    g, faces = mrr.grid_mesh(nx, ny)
    rng = np.random.RandomState(100 + seed + T)
    verts = np.concatenate([g.astype(np.float64) * 0.05, np.zeros((g.shape[0], 1))], 1) + rng.uniform(-0.02, 0.02, (g.shape[0], 3))
    return verts.astype(np.float32), np.ascontiguousarray(faces[:T])


def fill_input(T, n, seed=0):
    """float32 [T P,3] with values below 0, above 1 and NaN among ordinary ones."""
    P = n * (n - 1) // 2
    rng = np.random.RandomState(200 + seed + 31 * T + n)
    rgb = rng.uniform(-0.2, 1.2, (T * P, 3)).astype(np.float32)
    rgb.reshape(-1)[rng.randint(0, rgb.size, max(1, rgb.size // 50))] = np.nan
    rgb.reshape(-1)[rng.randint(0, rgb.size, 3)] = [0.0, 1.0, np.float32(1.0 / 255.0)]
    return rgb


def random_atlas(T, n, seed=0):
    C, _, W, H, _ = layout(T, n)
    return np.random.RandomState(300 + seed + n).randint(0, 256, (H, W, 3)).astype(np.uint8), C


def affine_colour(pts, seed=0):
    """(a float64 [3,3], b float64 [3]): per channel c(p) = a . p + b with c in [0.1, 0.9] on every one of the texel points pts
    (the extrapolated rim included, so that the fill's clamp never acts)."""
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    rng = np.random.RandomState(400 + seed)
    a = rng.normal(size=(3, 3))
    d = p @ a.T
    lo, hi = d.min(0), d.max(0)
    scale = 0.8 / np.maximum(hi - lo, 1e-12)
    return a * scale[:, None], 0.1 - lo * scale


def affine_bound(a, pts):
    """The bound of the affine test on |byte - 255 c(p)|, from the inputs alone:

        1.5 + 255 eps,  eps = 2^-24 (sum_c |a_c| max|p_c| + 2) + 2^-45 (sum_c |a_c| max|p_c| + 1)

    1: the fill truncates, every tap's byte is 255 c_k - tau_k with 0 <= tau_k < 1, and the sampler's weights are >= 0 and sum
    to 1, so the interpolated truncation stays in [0, 1).  0.5: the sampler's rint.  The first eps term: a texel's position is
    rounded to float32 (relative 2^-24 per coordinate, carried through a), its colour is rounded to float32 when it is handed
    to the fill (<= 2^-24 on a value <= 1) and again by the float32 product with 255 (2^-24 relative).  The second: the
    float64 roundings of x, y, the four weights and the sum (a few 2^-53 on values <= m <= 61, here 2^-45 for all of them).
    Bilinear interpolation reproduces an affine function exactly; nothing else enters."""
    reach = (np.abs(np.asarray(a, np.float64)) * np.abs(np.asarray(pts, np.float64).reshape(-1, 3)).max(0)[None, :]).sum(1).max()
    eps = 2.0 ** -24 * (reach + 2.0) + 2.0 ** -45 * (reach + 1.0)
    return 1.5 + 255.0 * eps


def interior_barycentrics(count, seed=0):
    """float64 [count,3]: random weights w0 + w1 + w2 = 1 inside the triangle."""
    u = np.random.RandomState(500 + seed).uniform(0.0, 1.0, (count, 2))
    flip = u.sum(1) > 1.0
    u[flip] = 1.0 - u[flip]
    return np.stack([1.0 - u[:, 0] - u[:, 1], u[:, 0], u[:, 1]], 1)


# ------------------------------------------------------------------ a reader of the textured glTF binaries
COMPONENTS = {'SCALAR': 1, 'VEC2': 2, 'VEC3': 3, 'VEC4': 4, 'MAT4': 16}
DTYPES = {5121: 'u1', 5123: '<u2', 5125: '<u4', 5126: '<f4'}


def parse_glb(blob):
    magic, version, length = struct.unpack_from('<4sII', blob, 0)
    assert magic == b'glTF' and version == 2 and length == len(blob)
    n_json, kind = struct.unpack_from('<I4s', blob, 12)
    assert kind == b'JSON' and n_json % 4 == 0
    doc = json.loads(blob[20:20 + n_json].decode('utf-8'))
    n_bin, kind = struct.unpack_from('<I4s', blob, 20 + n_json)
    assert kind == b'BIN\0' and n_bin % 4 == 0 and 28 + n_json + n_bin == length
    return doc, blob[28 + n_json:]


def accessor(doc, buf, index):
    acc = doc['accessors'][index]
    view = doc['bufferViews'][acc['bufferView']]
    dt, nc = np.dtype(DTYPES[acc['componentType']]), COMPONENTS[acc['type']]
    assert 'byteStride' not in view and view['byteOffset'] % 4 == 0
    return np.frombuffer(buf, dtype=dt, count=acc['count'] * nc, offset=view['byteOffset'] + acc.get('byteOffset', 0)).reshape(acc['count'], nc)


def read_textured(blob):
    """The rules a textured file has to keep, as assertions -> (doc, buf, attributes dict of arrays, indices, image uint8
    [H,W,3])."""
    import io

    from PIL import Image
    doc, buf = parse_glb(blob)
    assert doc['asset']['version'] == '2.0' and len(doc['meshes']) == 1 and len(doc['meshes'][0]['primitives']) == 1
    prim = doc['meshes'][0]['primitives'][0]
    att = {k: accessor(doc, buf, a) for k, a in prim['attributes'].items()}
    n = att['POSITION'].shape[0]
    for k, a in prim['attributes'].items():
        assert doc['accessors'][a]['count'] == n and doc['bufferViews'][doc['accessors'][a]['bufferView']]['target'] == 34962, k
    pa = doc['accessors'][prim['attributes']['POSITION']]
    assert pa['min'] == att['POSITION'].min(0).astype(np.float64).tolist() and pa['max'] == att['POSITION'].max(0).astype(np.float64).tolist()
    idx = accessor(doc, buf, prim['indices'])[:, 0]
    assert doc['accessors'][prim['indices']]['componentType'] == 5125 and np.array_equal(idx, np.arange(n)) and n % 3 == 0
    assert 'COLOR_0' not in att and doc['accessors'][prim['attributes']['TEXCOORD_0']]['type'] == 'VEC2'
    assert doc['accessors'][prim['attributes']['TEXCOORD_0']]['componentType'] == 5126
    assert len(doc['images']) == len(doc['samplers']) == len(doc['textures']) == len(doc['materials']) == 1 and prim['material'] == 0
    img = doc['images'][0]
    assert img['mimeType'] == 'image/png' and 'uri' not in img
    view = doc['bufferViews'][img['bufferView']]
    assert 'target' not in view and view['byteOffset'] + view['byteLength'] <= doc['buffers'][0]['byteLength']
    png = bytes(buf[view['byteOffset']:view['byteOffset'] + view['byteLength']])
    image = np.asarray(Image.open(io.BytesIO(png)).convert('RGB'))
    assert doc['samplers'][0] == {'magFilter': 9729, 'minFilter': 9729, 'wrapS': 33071, 'wrapT': 33071}
    assert doc['textures'][0] == {'sampler': 0, 'source': 0}
    pbr = doc['materials'][0]['pbrMetallicRoughness']
    assert pbr['baseColorTexture'] == {'index': 0} and pbr['metallicFactor'] == 0.0 and pbr['roughnessFactor'] == 1.0
    for tgt in prim.get('targets', []):
        assert set(tgt) == {'POSITION'} and doc['accessors'][tgt['POSITION']]['count'] == n
    return doc, buf, att, idx, image
