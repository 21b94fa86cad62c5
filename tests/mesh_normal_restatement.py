"""The numpy definition of the tangent-space normal map of the exported mesh: every texel of the coarse
mesh's per-triangle atlas (section 7o, tests/mesh_texture_restatement.py) is projected along the interpolated vertex normal onto
the iso-surface of a fine density grid, and the field's normal there is stored in the tangent frame the glTF carries.
csrc/mesh_normal.hip must give these bits.

float64 on the float32 inputs, one rounding per operator in the order written below, nothing fused, + - * / sqrt floor rint and
comparisons only.  dot(a, b) = (a0 b0 + a1 b1) + a2 b2; cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0);
normalise(v) = v / sqrt(dot(v, v)) per component, and *fails* when dot(v, v) is zero or not finite (0 < l2 <= the largest
float64; a NaN fails); blend(b, A) = (b0 A0 + b1 A1) + b2 A2 per component.

  tangents  per triangle (v0, v1, v2) and corner c with N_c the float32 vertex normal: e1 = v1 - v0, e2 = v2 - v0, sigma = +1
            for an even triangle, -1 for an odd one (the odd triangle's chart is the mirrored one: texture_uv's column grows
            against i' and its row against j'), T_c = normalise(sigma e1 - N_c (dot(N_c, sigma e1) / dot(N_c, N_c))), w = +1 (the
            float32 normal is a unit vector only to 2^-24; the division keeps T_c orthogonal to it in float64).  A triangle with a
            corner whose dot(N_c, cross(e1, e2)) <= 0 (a NaN too), a zero cross(e1, e2) or a failed T_c is *creased*: its
            three tangents are stored as (1, 0, 0, 1).  float32 [T,3,4] and a mask.
  sample    f(q) on field [nz,ny,nx] with point (i,j,k) at lo + (i,j,k) h: per axis g = (q_a - lo_a) / h, c = min(max(g, 0),
            n_a - 1) with a NaN -> 0, cell = min(floor(c), n_a - 2), fraction t = c - cell; with u = 1 - t per axis:
            x first, c_jk = v_0jk ux + v_1jk tx; then y, c_k = c_0k uy + c_1k ty; then z, f = c_0 uz + c_1 tz.  A NaN tap
            gives a NaN sample.
  texel     with numerators b = (m - i' - j', i', j'), m = n - 3, p its float32 point (texel_points), level the float32 level:
            1. nh = normalise(blend(b, N)); failed: nh = normalise(cross(e1, e2)) -- (0, 0, 1) if that fails too -- and flag 8;
            2. delta = h / 2; u_k = f(p + (f64(k) delta) nh) - level, k = -S .. S; a crossing between k and k + 1 iff
               (u_k > 0) != (u_k+1 > 0) and both are finite; s = (f64(k) + u_k / (u_k - u_k+1)) delta; the smallest |s| wins, a
               tie goes to the positive one; none: s = 0 and flag 1; q = p + s nh;
            3. g_a = f(q + h e_a) - f(q - h e_a), l2 = dot(g, g), N_f = (-g) / sqrt(l2); l2 zero or not finite: N_f = nh, flag 2;
            4. Th = normalise(blend(b, T_c xyz)), B = cross(nh, Th), det = dot(Th, cross(B, nh)),
               tx = dot(N_f, cross(B, nh)) / det, ty = dot(N_f, cross(nh, Th)) / det, tz = dot(N_f, cross(Th, B)) / det,
               c = normalise((tx, ty, tz)); a creased triangle, a failed Th, |det| < 2^-20 (a NaN too), a non-finite tx, ty or
               tz, tz <= 0 or a failed c: c = (0, 0, 1) and flag 4;
            5. byte = min(max(rint(127.5 (c + 1)), 0), 255): the flat normal is (128, 128, 255), also the fill of every texel
               nobody owns.
            Outputs per texel: the three bytes at its place in the atlas, offset = float32(s), flags, normal = float32(N_f); a
            NaN is stored as 0x7FC00000.  A face with an index outside [0, V): offset and normal NaN, flags 0, flat bytes,
            status 1.
  lit       per pixel of mesh_raster's keys, the winner t and weights (w0, w1, w2) as resolve_textured forms them:
            Nh = normalise(blend(w, N)) of the posed mesh's float32 vertex normals, Th likewise of its corner tangents,
            B = cross(Nh, Th); the atlas through section 7o's taps and weights with the blend s left unrounded,
            c = s / 127.5 - 1, nm = normalise((cx Th + cy B) + cz Nh) -- but where all four taps are the flat code, nm = Nh:
            128 is the code nearest to zero, not zero, and a texel that carries no detail must not tilt the normal;
            d_r = (M_r0 f64(column) + M_r1 f64(row)) + M_r2; the grey is float32((-dot(n, d)) / sqrt(dot(d, d))), clamped to
            [0, 1] with NaN -> 0 in float32, then uint8(float32(255) * grey), truncated: image.to_8b_image.  A failed
            normalise gives the grey 0.  shade_geometry takes Nh, shade_mapped nm; an empty pixel the background."""
import numpy as np

from tests import mesh_raster_restatement as mrr
from tests import mesh_texture_restatement as tex

NO_CROSSING, NO_GRADIENT, FLAT, FACE_DIRECTION = 1, 2, 4, 8
MAX_STEPS = 64
MIN_DET = 2.0 ** -20
FLAT_CODE = np.array([128, 128, 255], np.uint8)
F64_MAX = np.finfo(np.float64).max
CANONICAL_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def usable(l2):
    with np.errstate(invalid='ignore'):
        return (l2 > 0.0) & (l2 <= F64_MAX)


def finite(x):
    with np.errstate(invalid='ignore'):
        return np.abs(x) <= F64_MAX


def normalise(v):
    """-> (v / sqrt(dot(v, v)) where that is usable, v itself elsewhere; the mask of the usable ones)."""
    l2 = dot(v, v)
    ok = usable(l2)
    with np.errstate(all='ignore'):
        out = v / np.sqrt(np.where(ok, l2, 1.0))[..., None]
    return np.where(ok[..., None], out, v), ok


def blend(b, A):
    """b [...,3] weights, A [...,3 corners,3] -> (b0 A0 + b1 A1) + b2 A2."""
    return (b[..., 0, None] * A[..., 0, :] + b[..., 1, None] * A[..., 1, :]) + b[..., 2, None] * A[..., 2, :]


def steps(cage, h):
    """S = ceil(cage / (h / 2)); outside 1..64 it is refused by name."""
    S = int(np.ceil(np.float64(cage) / (np.float64(h) / 2.0)))
    if not 1 <= S <= MAX_STEPS:
        raise ValueError(f'mesh_normal: cage = {cage!r} at a fine voxel of {h!r} takes S = {S} steps, outside 1..{MAX_STEPS}')
    return S


def vertex_normals(verts, faces):
    """The export's area-weighted vertex normals (occnerf_amd.synth.vertex_normals) as the float32 the files carry."""
    from occnerf_amd.synth import vertex_normals as vn
    return vn(np.asarray(verts, np.float32), np.asarray(faces)).astype(np.float32)


def corner_tangents(verts, faces, normals):
    """-> (tangents float32 [T,3,4], creased bool [T])."""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    N = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)[f]           # [T,3,3]
    T = f.shape[0]
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    sigma = np.where(np.arange(T) % 2 == 0, 1.0, -1.0)[:, None]
    se1 = (sigma * e1)[:, None, :]
    with np.errstate(all='ignore'):
        t = se1 - N * (dot(N, se1) / dot(N, N))[..., None]
        t, ok = normalise(t)
        fn = cross(e1, e2)
        front = dot(N, fn[:, None, :]) > 0.0
    creased = ~(front.all(1) & ok.all(1) & usable(dot(fn, fn)))
    out = np.concatenate([t, np.ones((T, 3, 1))], -1)
    out[creased] = [1.0, 0.0, 0.0, 1.0]
    return out.astype(np.float32), creased


def trilinear(field, lo, h, q):
    """field float32 [nz,ny,nx], q float64 [N,3] -> float64 [N]."""
    f = np.asarray(field, np.float32)
    nz, ny, nx = f.shape
    lo, h = np.asarray(lo, np.float64).reshape(3), np.float64(h)
    cell, t = [], []
    for a, n in enumerate((nx, ny, nz)):
        with np.errstate(all='ignore'):
            g = (q[:, a] - lo[a]) / h
            c = np.where(g > 0.0, np.where(g < np.float64(n - 1), g, np.float64(n - 1)), 0.0)
        k = np.minimum(np.floor(c).astype(np.int64), n - 2)
        cell.append(k)
        t.append(c - k.astype(np.float64))
    (ix, iy, iz), (tx, ty, tz) = cell, t
    ux, uy, uz = 1.0 - tx, 1.0 - ty, 1.0 - tz
    v = lambda dz, dy, dx: f[iz + dz, iy + dy, ix + dx].astype(np.float64)                # noqa: E731
    with np.errstate(all='ignore'):
        c00, c10 = v(0, 0, 0) * ux + v(0, 0, 1) * tx, v(0, 1, 0) * ux + v(0, 1, 1) * tx
        c01, c11 = v(1, 0, 0) * ux + v(1, 0, 1) * tx, v(1, 1, 0) * ux + v(1, 1, 1) * tx
        c0, c1 = c00 * uy + c10 * ty, c01 * uy + c11 * ty
        return c0 * uz + c1 * tz


def to_code(c):
    with np.errstate(invalid='ignore'):
        return np.minimum(np.maximum(np.rint(127.5 * (c + 1.0)), 0.0), 255.0).astype(np.uint8)


def canonical32(x):
    out = np.asarray(x, np.float64).astype(np.float32)
    out[np.isnan(out)] = CANONICAL_NAN
    return out


def bake(verts, faces, normals, tangents, creased, pts, n, field, lo, h, level, S, atlas=None):
    """-> dict: atlas uint8 [H,W,3] (a given one is written in place), offset float32 [T,P], flags uint8 [T,P], normal float32
    [T,P,3], status, and the float64 values the tests judge: nh, q, s, N_f, c [T,P,...]."""
    n = tex.check_cell(n)
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    V, T = v.shape[0], f.shape[0]
    C, _, W, H, P = tex.layout(T, n)
    if not 1 <= int(S) <= MAX_STEPS:
        raise ValueError(f'mesh_normal: S = {S} steps outside 1..{MAX_STEPS}')
    if atlas is None:
        atlas = np.empty((H, W, 3), np.uint8)
        atlas[:] = FLAT_CODE
    bad = ((f < 0) | (f >= V)).any(1)
    fs = np.where(bad[:, None], 0, f)
    ij = tex.owned(n)
    m = n - 3
    b = np.stack([m - ij[:, 0] - ij[:, 1], ij[:, 0], ij[:, 1]], -1).astype(np.float64)      # [P,3]
    b = np.broadcast_to(b[None], (T, P, 3)).reshape(-1, 3)
    tri = np.repeat(np.arange(T), P)
    Nc = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)[fs][tri]      # [N,3,3]
    Tc = np.asarray(tangents, np.float32).astype(np.float64).reshape(T, 3, 4)[tri][..., :3]
    p = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    level, h = np.float64(np.float32(level)), np.float64(h)
    flags = np.zeros(T * P, np.int64)
    with np.errstate(all='ignore'):
        # 1
        nh, ok = normalise(blend(b, Nc))
        e1, e2 = (v[fs[:, 1]] - v[fs[:, 0]])[tri], (v[fs[:, 2]] - v[fs[:, 0]])[tri]
        fn, fok = normalise(cross(e1, e2))
        fn = np.where(fok[:, None], fn, np.array([0.0, 0.0, 1.0]))
        nh = np.where(ok[:, None], nh, fn)
        flags |= np.where(ok, 0, FACE_DIRECTION)
        # 2
        delta = h / 2.0
        s, found = np.zeros(T * P), np.zeros(T * P, bool)
        u0 = trilinear(field, lo, h, p + (np.float64(-S) * delta) * nh) - level
        for k in range(-S, S):
            u1 = trilinear(field, lo, h, p + (np.float64(k + 1) * delta) * nh) - level
            hit = finite(u0) & finite(u1) & ((u0 > 0.0) != (u1 > 0.0))
            c = (np.float64(k) + u0 / (u0 - u1)) * delta
            take = hit & (~found | (np.abs(c) < np.abs(s)) | ((np.abs(c) == np.abs(s)) & (c > s)))
            s = np.where(take, c, s)
            found |= hit
            u0 = u1
        flags |= np.where(found, 0, NO_CROSSING)
        q = p + s[:, None] * nh
        # 3
        g = np.stack([trilinear(field, lo, h, q + h * np.eye(3)[a]) - trilinear(field, lo, h, q - h * np.eye(3)[a]) for a in range(3)], -1)
        l2 = dot(g, g)
        gok = usable(l2)
        Nf = np.where(gok[:, None], (-g) / np.sqrt(np.where(gok, l2, 1.0))[:, None], nh)
        flags |= np.where(gok, 0, NO_GRADIENT)
        # 4
        Th, tok = normalise(blend(b, Tc))
        B = cross(nh, Th)
        Bn, nT, TB = cross(B, nh), cross(nh, Th), cross(Th, B)
        det = dot(Th, Bn)
        t3 = np.stack([dot(Nf, Bn) / det, dot(Nf, nT) / det, dot(Nf, TB) / det], -1)
        good = ~np.asarray(creased, bool)[tri] & tok & (np.abs(det) >= MIN_DET) & finite(t3).all(1) & (t3[:, 2] > 0.0)
        c3, cok = normalise(t3)
        good &= cok
        c3 = np.where(good[:, None], c3, np.array([0.0, 0.0, 1.0]))
        flags |= np.where(good, 0, FLAT)
    code = to_code(c3)
    badx = bad[tri]
    code[badx] = FLAT_CODE
    flags[badx] = 0
    offset, normal = canonical32(s), canonical32(Nf)
    offset[badx] = CANONICAL_NAN
    normal[badx] = CANONICAL_NAN
    code = code.reshape(T, P, 3)
    for t in range(T):
        x, y = tex.atlas_position(t, ij, n, C)
        atlas[y, x] = code[t]
    return {'atlas': atlas, 'offset': offset.reshape(T, P), 'flags': flags.astype(np.uint8).reshape(T, P),
            'normal': normal.reshape(T, P, 3), 'status': int(bad.any()), 'nh': nh.reshape(T, P, 3), 'q': q.reshape(T, P, 3),
            's': s.reshape(T, P), 'N_f': Nf.reshape(T, P, 3), 'c': c3.reshape(T, P, 3), 'C': C, 'b': b.reshape(T, P, 3)}


def bake_mesh(verts, faces, n, field, lo, h, level, S):
    """bake on a mesh alone: its vertex normals, corner tangents and texel points by their definitions."""
    normals = vertex_normals(verts, faces)
    tangents, creased = corner_tangents(verts, faces, normals)
    pts, _ = tex.texel_points(verts, faces, n)
    out = bake(verts, faces, normals, tangents, creased, pts, n, field, lo, h, level, S)
    out.update(normals=normals, tangents=tangents, creased=creased, pts=pts)
    return out


def ray_matrix(K, E):
    K, E = np.asarray(K, np.float64), np.asarray(E, np.float64)
    return np.ascontiguousarray(E[:3, :3].T @ np.linalg.inv(K))


def headlight(nrm, d, ok):
    with np.errstate(all='ignore'):
        v = np.float32((-dot(nrm, d)) / np.sqrt(dot(d, d)))
        u = v if v > 0 else np.float32(0.0)
        u = u if u < 1 else np.float32(1.0)
        if not ok or np.isnan(v):
            u = np.float32(0.0)
        return np.uint8(np.float32(255.0) * np.float32(u))


def resolve_lit(keys, faces, xy, z, normals, tangents, atlas, n, C, M, bgcolor):
    """-> (shade_geometry, shade_mapped) uint8 [H,W,3] of mesh_raster's keys uint64 [H,W]."""
    H, W = keys.shape
    faces = np.asarray(faces).reshape(-1, 3)
    z = np.asarray(z, dtype=np.float64)
    vflag = np.where(z > 0.0, 0, 1).astype(np.uint8)
    reason, idx, A = mrr.setup(faces, xy, vflag)
    T = faces.shape[0]
    N = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
    Tc = np.asarray(tangents, np.float32).astype(np.float64).reshape(-1, 3, 4)[..., :3]
    M = np.asarray(M, np.float64).reshape(3, 3)
    geo = np.empty((H, W, 3), dtype=np.uint8)
    geo[:] = np.asarray(bgcolor, dtype=np.uint8).reshape(3)
    mapped = geo.copy()
    for i, j in zip(*np.nonzero(keys != mrr.EMPTY_KEY)):
        t = int(keys[i, j] & np.uint64(0xFFFFFFFF))
        if t >= T or reason[t] != 0:
            continue
        v = idx[t]
        e, _ = mrr.edges(xy[v, 0].astype(np.int64), xy[v, 1].astype(np.int64), np.int64(256 * j), np.int64(256 * i))
        q, iz = mrr.inverse_depth(e, A[t], z[v])
        w = [q[k] / iz for k in range(3)]
        flipped = int(v[1]) != int(faces[t, 1])
        w = np.array([w[0], w[2], w[1]] if flipped else w, np.float64)
        Nh, okN = normalise(blend(w, N[faces[t]]))
        Th, okT = normalise(blend(w, Tc[t]))
        d = np.array([(M[r, 0] * np.float64(j) + M[r, 1] * np.float64(i)) + M[r, 2] for r in range(3)])
        geo[i, j] = headlight(Nh, d, okN)
        ij, wt = tex.taps(*tex.sample_xy(w[1], w[2], n), n)
        x, y = tex.atlas_position(t, ij, n, C)
        taps = atlas[y, x]                                                   # [4,3]
        if (taps == FLAT_CODE).all():
            mapped[i, j] = geo[i, j]
            continue
        c = taps.astype(np.float64)
        s = ((wt[0] * c[0] + wt[1] * c[1]) + wt[2] * c[2]) + wt[3] * c[3]
        c = s / 127.5 - 1.0
        B = cross(Nh, Th)
        nm, okM = normalise((c[0] * Th + c[1] * B) + c[2] * Nh)
        mapped[i, j] = headlight(nm, d, bool(okN and okT and okM))
    return geo, mapped


# ------------------------------------------------------------------ the cases the CPU and the GPU tests share
T_SIZES = (1, 2, 3, 63, 64, 65, 257)
CELLS = (4, 5, 8)

# f = a . x + b on 9 x 8 x 7 points: h, lo, a and b are sums of a few powers of two, so every grid value is exact in float32 and
# the trilinear sample of the field is the field up to float64 rounding.  The jittered grid meshes of section 7o (x, y in
# -0.02 .. 0.62, |z| <= 0.02, three triangles in four wound towards +z) straddle the plane f = level.
# The grid reaches beyond the meshes on every side by more than the rim's extrapolation (one triangle edge, 0.1), the reach of
# S = 2 steps (h) and the central difference (h): a sample must not meet the clamp, where the field stops changing along the
# clamped axis -- the plane assertions hold for S <= 2 only, the bit comparisons of the GPU tests for every S.
PLANE_H, PLANE_LO, PLANE_SHAPE = 0.3125, np.array([-0.9375, -0.8125, -0.9375]), (9, 8, 7)
PLANE_A, PLANE_B, PLANE_LEVEL = np.array([0.125, -0.0625, -1.0]), 0.234375, np.float32(0.25)


def grid_points(lo, h, shape):
    nx, ny, nz = shape
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing='ij')
    return np.stack([lo[0] + x * h, lo[1] + y * h, lo[2] + z * h], -1)


def plane_field():
    """-> (field float32 [7,8,9], lo, h, level, the outward unit normal -a / |a|)."""
    g = grid_points(PLANE_LO, PLANE_H, PLANE_SHAPE)
    f64 = g @ PLANE_A + PLANE_B
    f = f64.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), f64)
    return f, PLANE_LO, PLANE_H, PLANE_LEVEL, -PLANE_A / np.sqrt((PLANE_A * PLANE_A).sum())


SPHERE_R, SPHERE_C = 0.66, np.array([1.03, 0.98, 1.01])


def sphere_field(points):
    """R - |x - c| on `points` per axis over the box [0, 2]^3 -> (field float32, lo, h)."""
    h = 2.0 / (points - 1)
    g = grid_points(np.zeros(3), h, (points, points, points))
    return (SPHERE_R - np.sqrt(((g - SPHERE_C) ** 2).sum(-1))).astype(np.float32), np.zeros(3), h


# the jittered grid meshes moved onto the top of the sphere, where their +z windings look outwards
SPHERE_SHIFT = np.array([0.75, 0.70, 1.62], np.float32)


def sphere_mesh():
    """The coarse mesh of the sphere: tests/mesh_restatement.extract_mesh on the 9-point grid at level 0 -> (verts, faces, h)."""
    from tests import mesh_restatement as mr
    f, lo, h = sphere_field(9)
    verts, faces = mr.extract_mesh(f, 0.0, lo.astype(np.float32), h)
    return verts, faces, h


def angle(a, b):
    """The angle in radians between unit vectors, by atan2 of |a x b| and a . b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.sqrt((cross(a, b) ** 2).sum(-1)), dot(a, b))


def decode(code, normal3, tangent4):
    """The glTF rule read forwards, independent of bake's algebra: the texel's bytes -> c = byte / 127.5 - 1, the interpolated
    and normalised NORMAL and TANGENT.xyz (float32 attributes, given here already interpolated in float64), the bitangent
    cross(NORMAL, TANGENT.xyz) * TANGENT.w, the matrix [T B N] applied to c, normalised -> object-space unit normals [N,3] and
    the condition number of [T B N] per texel."""
    c = np.asarray(code, np.float64) / 127.5 - 1.0
    N = normal3 / np.linalg.norm(normal3, axis=-1, keepdims=True)
    T = tangent4[..., :3] / np.linalg.norm(tangent4[..., :3], axis=-1, keepdims=True)
    B = np.cross(N, T) * tangent4[..., 3:4]
    frame = np.stack([T, B, N], -1)                                          # columns
    out = np.einsum('...ij,...j->...i', frame, c)
    return out / np.linalg.norm(out, axis=-1, keepdims=True), np.linalg.cond(frame)


# ------------------------------------------------------------------ a reader of the normal-mapped glTF binaries
def read_normal_mapped(blob):
    """The rules a file with a normal map has to keep, as assertions -> (doc, buf, attributes, colour image, normal image)."""
    import io

    from PIL import Image
    doc, buf = tex.parse_glb(blob)
    assert doc['asset']['version'] == '2.0' and len(doc['meshes']) == 1 and len(doc['meshes'][0]['primitives']) == 1
    prim = doc['meshes'][0]['primitives'][0]
    att = {k: tex.accessor(doc, buf, a) for k, a in prim['attributes'].items()}
    count = att['POSITION'].shape[0]
    for k, a in prim['attributes'].items():
        assert doc['accessors'][a]['count'] == count and doc['bufferViews'][doc['accessors'][a]['bufferView']]['target'] == 34962, k
    assert {'NORMAL', 'TANGENT', 'TEXCOORD_0'} <= set(att) and 'COLOR_0' not in att
    ta = doc['accessors'][prim['attributes']['TANGENT']]
    assert ta['type'] == 'VEC4' and ta['componentType'] == 5126 and 'normalized' not in ta
    idx = tex.accessor(doc, buf, prim['indices'])[:, 0]
    assert np.array_equal(idx, np.arange(count)) and count % 3 == 0
    assert len(doc['images']) == len(doc['textures']) == 2 and len(doc['samplers']) == len(doc['materials']) == 1
    assert doc['samplers'][0] == {'magFilter': 9729, 'minFilter': 9729, 'wrapS': 33071, 'wrapT': 33071}
    assert doc['textures'] == [{'sampler': 0, 'source': 0}, {'sampler': 0, 'source': 1}]
    mat = doc['materials'][0]
    assert mat['pbrMetallicRoughness']['baseColorTexture'] == {'index': 0} and mat['normalTexture'] == {'index': 1}
    images = []
    for img in doc['images']:
        assert img['mimeType'] == 'image/png' and 'uri' not in img
        view = doc['bufferViews'][img['bufferView']]
        assert 'target' not in view and view['byteOffset'] % 4 == 0 and view['byteOffset'] + view['byteLength'] <= doc['buffers'][0]['byteLength']
        images.append(np.asarray(Image.open(io.BytesIO(bytes(buf[view['byteOffset']:view['byteOffset'] + view['byteLength']]))).convert('RGB')))
    for tgt in prim.get('targets', []):
        assert set(tgt) == {'POSITION'}                                      # morph targets carry no tangent deltas
    return doc, buf, att, images[0], images[1]
