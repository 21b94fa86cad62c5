"""The numpy definition of the photographs on the atlas: which texels of the per-triangle atlas of
section 7o a frame's camera saw, what it photographed there, and the blend of the frames with the colour field.
csrc/mesh_texture.hip (mesh_texture_project, mesh_texture_blend) must give these bits.

A pure function of faces [T,3] int32, the cell edge n (m = n - 3), per frame the posed vertices p [V,3] float32, their posing
flags [V], K, the body-space E, H, W, the photograph uint8 [H,W,3] and inside uint8 [H,W], and a depth bias b >= 0 (metres,
float64).  Floating point is float64 with + - * / rint and comparisons only, one rounding per operator in the order written
here, nothing fused; the colour path has no floating point at all.

  point     q = mesh_texture_restatement.texel_points(p, faces, n): section 7o's formula on the posed vertices, rim included.
  screen    (X, Y, z, flag) = mesh_raster_restatement.project(q, K, E): int32 in 1/256 pixel, float64 z.
  keys      mesh_raster_restatement.raster_keys of project(p, K, E) and faces.
  weight    c_k the camera-space vertices (section 7j's vertex formula), e1 = c_1 - c_0, e2 = c_2 - c_0, N = e1 x e2 (each
            component a b - c d), g = (c_0 + c_1) + c_2, d = (N_x g_x + N_y g_y) + N_z g_z, NN and gg likewise, q = NN gg,
            r = 256 ((d d) / q), w = min(rint(r), 256).  w = 0 when q is 0 or not finite, r is not finite, a vertex has a
            non-zero posing flag or a section 7j flag, or an index lies outside [0, V) (status 1).  The triangle FACES AWAY
            when d > 0, and then w = 0 as well: marching tetrahedra winds (b - a) x (c - a) from the inside to the outside
            (section 7h), g points from the camera to the triangle, so a triangle seen from outside has d < 0
            (test_mesh_photo_restatement.py establishes the sign on an extracted sphere).
  taps      j0 = X >> 8, i0 = Y >> 8, fx = X & 255, fy = Y & 255; taps (i0 + {0,1}, j0 + {0,1}).  SEEN in this frame: w > 0,
            flag == 0, all four taps inside the image, non-empty in the keys, inside != 0 and
            z <= float64(float32 depth of the tap's key) + b.
  sample    per channel s = (256-fx)(256-fy) c00 + fx (256-fy) c01 + (256-fx) fy c10 + fx fy c11, c01 the next column, c10 the
            next row: an integer <= 65536 * 255.
  sum       over the frames, int64 acc [T P,4] and int32 seen [T P]: acc_c += w s_c, acc_3 += w, seen += 1.
  blend     an owned texel with seen >= min_seen (>= 1) and acc_3 > 0: byte_c = min((acc_c + 32768 acc_3) // (65536 acc_3), 255);
            any other owned texel keeps the field's byte; unowned texels keep what the field's atlas holds (the fill).  The
            seen image holds min(seen, 255) at the owned texels, 0 elsewhere.
"""
import numpy as np

from tests import mesh_raster_restatement as mrr
from tests import mesh_texture_restatement as mtr

BUCKETS = ('0', '1', '2-3', '4-7', '8-15', '16+')


def check_bias(b):
    b = float(b)
    if not b >= 0.0:
        raise ValueError(f'mesh_photo: bias = {b!r} is negative or not a number')
    return b


def camera_space(p, K, E):
    """(c float64 [V,3], flag uint8 [V]): section 7j's vertex formula and its flags."""
    fx, fy, cx, cy, R, t = mrr.camera(K, E)
    p = np.asarray(p, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all='ignore'):
        c = np.stack([((R[k, 0] * p[:, 0] + R[k, 1] * p[:, 1]) + R[k, 2] * p[:, 2]) + t[k] for k in range(3)], 1)
        near = ~(c[:, 2] >= mrr.NEAR)
        a = 256.0 * (fx * (c[:, 0] / c[:, 2]) + cx)
        b = 256.0 * (fy * (c[:, 1] / c[:, 2]) + cy)
        out = ~((np.abs(a) <= mrr.GUARD) & (np.abs(b) <= mrr.GUARD) & (c[:, 2] <= mrr.FAR))
    return c, np.where(near, 1, np.where(out, 2, 0)).astype(np.uint8)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def triangle_weights(p, pflag, faces, K, E):
    """-> (tri_w int32 [T]: 1..256, 0 unusable, -1 facing away; status 0 / 1)."""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    c, vflag = camera_space(p, K, E)
    V, T = c.shape[0], f.shape[0]
    if T == 0:
        return np.zeros(0, np.int32), 0
    bad = ((f < 0) | (f >= V)).any(1)
    idx = np.where(bad[:, None], 0, f)
    if V == 0:
        return np.zeros(T, np.int32), 1
    fl = (np.asarray(pflag, dtype=np.uint8).reshape(-1)[idx] | vflag[idx]).any(1)
    c0, c1, c2 = c[idx[:, 0]], c[idx[:, 1]], c[idx[:, 2]]
    with np.errstate(all='ignore'):
        e1, e2, g = c1 - c0, c2 - c0, (c0 + c1) + c2
        N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        d, NN, gg = _dot(N, g), _dot(N, N), _dot(g, g)
        q = NN * gg
        r = 256.0 * ((d * d) / q)
        ok = ~bad & ~fl & (q > 0.0) & np.isfinite(q) & (r >= 0.0) & np.isfinite(r)
        w = np.minimum(np.rint(np.where(ok, r, 0.0)), 256.0).astype(np.int32)
    tri_w = np.where(ok, np.where(d > 0.0, -1, w), 0).astype(np.int32)
    return tri_w, int(bad.any())


def frame_keys(p, faces, K, E, H, W):
    xy, z, vflag = mrr.project(p, K, E)
    return mrr.raster_keys(faces, xy, z, vflag, H, W)[0]


def project_frame(faces, n, p, pflag, K, E, photo, inside, b, acc, seen, keys=None):
    """One frame into acc int64 [T P,4] and seen int32 [T P] (in place) -> (tri_w, seen mask bool [T P]).  keys: the frame's
    uint64 [H,W] where the caller has them (the definition's are frame_keys')."""
    b = np.float64(check_bias(b))
    photo = np.asarray(photo, dtype=np.uint8)
    H, W = photo.shape[:2]
    inside = np.asarray(inside, dtype=np.uint8).reshape(H, W)
    faces = np.asarray(faces).reshape(-1, 3)
    T = faces.shape[0]
    tri_w, status = triangle_weights(p, pflag, faces, K, E)
    if status:
        raise ValueError(f'mesh_photo: a face index lies outside [0, {np.asarray(p).reshape(-1, 3).shape[0]})')
    if T == 0:
        return tri_w, np.zeros(0, bool)
    if keys is None:
        keys = frame_keys(p, faces, K, E, H, W)
    keys = np.asarray(keys)
    keys = keys.view(np.uint64) if keys.dtype == np.int64 else keys
    q, _ = mtr.texel_points(p, faces, n)
    P = q.shape[1]
    xy, z, flag = mrr.project(q.reshape(-1, 3), K, E)
    w = np.repeat(np.maximum(tri_w, 0), P).astype(np.int64)
    X, Y = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
    j0, i0, fx, fy = X >> 8, Y >> 8, X & 255, Y & 255
    ok = (w > 0) & (flag == 0) & (j0 >= 0) & (i0 >= 0) & (j0 + 1 <= W - 1) & (i0 + 1 <= H - 1)
    ii, jj = np.where(ok, i0, 0), np.where(ok, j0, 0)
    depth = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
    i1, j1 = np.minimum(ii + 1, H - 1), np.minimum(jj + 1, W - 1)         # (only a texel that is not ok anyway is clipped)
    taps = [(ii, jj), (ii, j1), (i1, jj), (i1, j1)]                          # c00, c01 (next column), c10 (next row), c11
    for ti, tj in taps:
        ok &= (keys[ti, tj] != mrr.EMPTY_KEY) & (inside[ti, tj] != 0) & (z <= depth[ti, tj] + b)
    wt = [(256 - fx) * (256 - fy), fx * (256 - fy), (256 - fx) * fy, fx * fy]
    s = sum(wt[k][:, None] * photo[taps[k][0], taps[k][1]].astype(np.int64) for k in range(4))
    acc[ok, :3] += w[ok, None] * s[ok]
    acc[ok, 3] += w[ok]
    seen[ok] += 1
    return tri_w, ok


def accumulators(T, n):
    P = n * (n - 1) // 2
    return np.zeros((T * P, 4), np.int64), np.zeros(T * P, np.int32)


def atlas_index(T, n, C):
    """(x, y) int64 [T P]: the atlas column and row of every owned texel, in the accumulators' order."""
    ij = mtr.owned(n)
    xs, ys = zip(*(mtr.atlas_position(t, ij, n, C) for t in range(T))) if T else ((), ())
    return (np.concatenate(xs), np.concatenate(ys)) if T else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def blend(acc, seen, T, n, C, atlas, min_seen=1):
    """-> (photo uint8 [H,W,3], seen image uint8 [H,W]) from the field's atlas uint8 [H,W,3] (not written)."""
    if isinstance(min_seen, (bool, np.bool_)) or not isinstance(min_seen, (int, np.integer)) or int(min_seen) < 1:
        raise ValueError(f'mesh_photo: min_seen = {min_seen!r} is not a whole number >= 1')
    out = np.array(atlas, dtype=np.uint8, copy=True)
    img = np.zeros(out.shape[:2], np.uint8)
    x, y = atlas_index(T, n, C)
    acc, seen = np.asarray(acc, dtype=np.int64), np.asarray(seen, dtype=np.int32)
    img[y, x] = np.clip(seen, 0, 255).astype(np.uint8)
    use = (seen >= int(min_seen)) & (acc[:, 3] > 0)
    a3 = np.where(use, acc[:, 3], 1)[:, None]
    byte = np.clip((acc[:, :3] + 32768 * a3) // (65536 * a3), 0, 255).astype(np.uint8)
    out[y[use], x[use]] = byte[use]
    return out, img


def photo_texture(faces, n, frames, b, atlas, C, min_seen=1):
    """The whole definition.  frames: an iterable of (p, pflag, K, E, photo, inside) -> (photo atlas, seen image, acc, seen)."""
    T = np.asarray(faces).reshape(-1, 3).shape[0]
    acc, seen = accumulators(T, n)
    for p, pflag, K, E, photo, inside in frames:
        project_frame(faces, n, p, pflag, K, E, photo, inside, b, acc, seen)
    return (*blend(acc, seen, T, n, C, atlas, min_seen), acc, seen)


def seen_histogram(seen):
    """The seen counts of the owned texels in the buckets 0, 1, 2-3, 4-7, 8-15, 16+."""
    s = np.asarray(seen).reshape(-1)
    edges = [(0, 0), (1, 1), (2, 3), (4, 7), (8, 15), (16, np.iinfo(np.int32).max)]
    return {name: int(((s >= lo) & (s <= hi)).sum()) for name, (lo, hi) in zip(BUCKETS, edges)}


# ------------------------------------------------------------------ the cases the CPU and the GPU tests share
def constant_photo(H, W, c):
    return np.full((H, W, 3), c, dtype=np.uint8)


def affine_photo(H=64, W=64):
    """R = 2j + i + 10, G = j + 2i + 5, B = 3i + 7 (i the row, j the column): at most 255 on 64 x 64."""
    i, j = np.mgrid[0:H, 0:W]
    img = np.stack([2 * j + i + 10, j + 2 * i + 5, 3 * i + 7], -1)
    assert img.max() <= 255
    return img.astype(np.uint8)


def affine_expected(xy):
    """uint8 [N,3]: the half-up rounding of the affine photograph at (X, Y) / 256, in integers."""
    X, Y = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
    v = np.stack([2 * X + Y + 10 * 256, X + 2 * Y + 5 * 256, 3 * Y + 7 * 256], 1)          # 256 x the value
    return ((v + 128) // 256).astype(np.uint8)


def random_frame_inputs(V, H, W, seed=0, flag_share=0.05, outside_share=0.1):
    """(photo uint8 [H,W,3], inside uint8 [H,W], pflag uint8 [V]): random, with a few vertices flagged and a tenth of the
    pixels outside the mask."""
    rng = np.random.RandomState(700 + seed)
    photo = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    inside = (rng.uniform(size=(H, W)) >= outside_share).astype(np.uint8)
    pflag = np.where(rng.uniform(size=V) < flag_share, rng.randint(1, 3, V), 0).astype(np.uint8)
    return photo, inside, pflag


def perturbed_cameras(K, E, count, seed=0):
    """count cameras: the first is (K, E), the others are E turned by a few degrees and moved by a few centimetres."""
    rng = np.random.RandomState(800 + seed)
    out = [(np.asarray(K, np.float64), np.asarray(E, np.float64))]
    for _ in range(count - 1):
        a = rng.uniform(-0.06, 0.06, 3)
        th = np.linalg.norm(a)
        k = a / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
        D = np.eye(4)
        D[:3, :3], D[:3, 3] = R, rng.uniform(-0.05, 0.05, 3)
        out.append((out[0][0], D @ out[0][1]))
    return out


def face_the_camera(pos, faces, K, E):
    """faces with every triangle that faces away from the camera (K, E) turned round."""
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    tri_w, _ = triangle_weights(pos, np.zeros(len(pos), np.uint8), np.clip(faces, 0, max(len(pos) - 1, 0)), K, E)
    return np.ascontiguousarray(np.where((tri_w < 0)[:, None], faces[:, [0, 2, 1]], faces).astype(np.int32))


def surface_case(T, H=64, W=64, seed=0, face=True):
    """The first T triangles of a welded grid (mrr.grid_mesh: shared vertices, mixed windings) that spans the image from two
    pixels outside its left and top border to four pixels inside its right and bottom one, its vertices jittered by half a
    pixel and by 5 cm in depth about z = 3: a surface the camera of mrr.pinhole(H, W) sees almost everywhere, whose texels
    reach the image border on two sides and empty pixels on the other two.  face: wound to face the camera (else the grid's
    mixed windings stay: half of the triangles face away)."""
    nx = max(1, int(np.ceil(np.sqrt(T / 2.0))))
    ny = max(1, -(-T // (2 * nx)))
    g, faces = mrr.grid_mesh(nx, ny)
    K, E = mrr.pinhole(H, W)
    rng = np.random.RandomState(600 + seed + T)
    uv = np.stack([-2.0 + g[:, 0] * (W - 2.0) / nx, -2.0 + g[:, 1] * (H - 2.0) / ny], 1) + rng.uniform(-0.5, 0.5, (len(g), 2))
    pos = mrr.unproject(K, E, uv, 3.0 + rng.uniform(-0.05, 0.05, len(g)))
    faces = np.ascontiguousarray(faces[:T])
    return {'pos': pos, 'faces': face_the_camera(pos, faces, K, E) if face else faces, 'K': K, 'E': E, 'H': H, 'W': W}


def two_quads(D, H=48, W=48, z0=3.0):
    """Two parallel quads facing the camera of mrr.pinhole(H, W) (which looks along +z from z = -3 ... E translates by +3), the
    near one at camera depth z0 and the far one D behind it, both wound so that they face the camera.  -> (pos, faces, K, E);
    triangles 0, 1 are the near quad, 2, 3 the far one."""
    K, E = mrr.pinhole(H, W)
    uv = np.array([[8, 8], [W - 9, 8], [8, H - 9], [W - 9, H - 9]], dtype=np.float64)
    near = mrr.unproject(K, E, uv, np.full(4, z0))
    far = mrr.unproject(K, E, uv, np.full(4, z0 + D))
    pos = np.concatenate([near, far])
    quad = np.array([[0, 1, 2], [3, 2, 1]], dtype=np.int32)
    faces = np.concatenate([quad, quad + 4])
    tri_w, _ = triangle_weights(pos, np.zeros(8, np.uint8), faces, K, E)
    faces = np.where((tri_w < 0)[:, None], faces[:, [0, 2, 1]], faces)       # wound to face the camera
    return pos, np.ascontiguousarray(faces.astype(np.int32)), K, E
