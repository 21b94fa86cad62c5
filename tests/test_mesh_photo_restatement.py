"""CPU: the photographs on the atlas.  The numpy definition (tests/mesh_photo_restatement.py) with the
numpy rasteriser and atlas of sections 7j and 7o, against facts that do not come from it: a constant and an integer-affine
photograph come back exactly, the blend's rounding on hand-made accumulators, what the depth bias, the mask, the image border,
the posing flags and the winding do to visibility, the weight of a tilted triangle, the sign of "facing" on an extracted sphere,
and colours planted in a tool-made dataset; then the refusals of the keys, the C entries and the wrappers."""
import json
import os
import pickle
import re

import numpy as np
import pytest

from tests import mesh_photo_restatement as ph
from tests import mesh_raster_restatement as mrr
from tests import mesh_restatement as mr
from tests import mesh_texture_restatement as tex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = (9, 200, 31)


def field_atlas(T, n, seed=0):
    """A random 'field' atlas whose unowned texels are FILL."""
    C, _, W, H, P = tex.layout(T, n)
    atlas = np.empty((H, W, 3), np.uint8)
    atlas[:] = FILL
    tex.fill(np.random.RandomState(900 + seed).uniform(0, 1, (T * P, 3)).astype(np.float32), T, n, C, atlas)
    return atlas, C


def owned_mask(T, n, C, shape):
    own = np.zeros(shape, bool)
    x, y = ph.atlas_index(T, n, C)
    own[y, x] = True
    return own


def facing_case(name):
    """A section 7j case with every triangle wound to face its camera, so that the photographs reach it."""
    c = mrr.CASES[name]()
    c['faces'] = ph.face_the_camera(c['pos'], c['faces'], c['K'], c['E'])
    return c


# ------------------------------------------------------------------ exact photographs
@pytest.mark.parametrize('frames', (1, 3))
def test_a_constant_photograph_comes_back_exactly(frames):
    c = ph.surface_case(129)
    V, T, n, H, W = len(c['pos']), len(c['faces']), 5, c['H'], c['W']
    atlas, C = field_atlas(T, n)
    cams = ph.perturbed_cameras(c['K'], c['E'], frames)
    inside = np.ones((H, W), np.uint8)
    items = [(c['pos'], np.zeros(V, np.uint8), K, E, ph.constant_photo(H, W, 173), inside) for K, E in cams]
    photo, img, acc, seen = ph.photo_texture(c['faces'], n, items, 0.05, atlas, C)
    hit = seen > 0
    assert hit.sum() > 100 and (~hit).sum() > 100
    x, y = ph.atlas_index(T, n, C)
    assert (photo[y[hit], x[hit]] == 173).all()                              # any weights: the mean of a constant
    assert np.array_equal(photo[y[~hit], x[~hit]], atlas[y[~hit], x[~hit]])
    own = owned_mask(T, n, C, img.shape)
    assert (photo[~own] == np.array(FILL, np.uint8)).all() and (img[~own] == 0).all()
    assert np.array_equal(img[y, x], np.minimum(seen, 255).astype(np.uint8)) and seen.max() <= frames
    if frames == 3:
        assert seen.max() >= 2                                               # some texel was blended from several frames
        again = ph.photo_texture(c['faces'], n, items[::-1], 0.05, atlas, C)
        assert np.array_equal(again[2], acc) and np.array_equal(again[0], photo)      # the order of the frames does not matter


def test_an_integer_affine_photograph_comes_back_exactly():
    """Step 6 is exactly affine in (X, Y) / 256 on R = 2j + i + 10, G = j + 2i + 5, B = 3i + 7, so with one frame every seen
    texel's byte is the half-up rounding of that function at its own (X, Y): no tolerance."""
    for name, n in (('surface', 8), ('blobs', 8), ('grid', 5), ('ties', 8)):
        c = ph.surface_case(65) if name == 'surface' else {**facing_case(name), 'H': 64, 'W': 64}
        V, T = len(c['pos']), len(c['faces'])
        atlas, C = field_atlas(T, n)
        acc, seen = ph.accumulators(T, n)
        _, ok = ph.project_frame(c['faces'], n, c['pos'], np.zeros(V, np.uint8), c['K'], c['E'], ph.affine_photo(), np.ones((64, 64), np.uint8),
                                 0.05, acc, seen)
        photo, _ = ph.blend(acc, seen, T, n, C, atlas)
        q, _ = tex.texel_points(c['pos'], c['faces'], n)
        xy, _, _ = mrr.project(q.reshape(-1, 3), c['K'], c['E'])
        x, y = ph.atlas_index(T, n, C)
        print(f'\n   {name}: {ok.sum()} of {ok.size} texels seen')
        assert ok.sum() > 20, name
        assert np.array_equal(photo[y[ok], x[ok]], ph.affine_expected(xy[ok])), name


def test_blend_alone():
    T, n = 3, 4
    atlas, C = field_atlas(T, n)
    P = n * (n - 1) // 2
    acc, seen = ph.accumulators(T, n)
    x, y = ph.atlas_index(T, n, C)
    for g, (w, k) in enumerate(((1, 0), (256, 17), (3 * 256, 254), (7, 100))):
        acc[g] = [65536 * w * k + 32768 * w, 65536 * w * k + 32768 * w - 1, 65536 * w * k, w]      # a tie, one below it, exact
        seen[g] = 1
    seen[4], acc[4] = 1, [65536 * 5 * 255] * 3 + [5]                          # the largest mean a frame can give
    seen[5], acc[5] = 2, [65536 * 2 * 9] * 3 + [2]                            # seen twice: used at min_seen 2 as well
    seen[6], acc[6] = 300, [65536 * 300 * 40] * 3 + [300]                     # the seen image saturates
    photo, img = ph.blend(acc, seen, T, n, C, atlas)
    for g, k in enumerate((0, 17, 254, 100)):
        assert photo[y[g], x[g]].tolist() == [k + 1, k, k]
    assert photo[y[4], x[4]].tolist() == [255] * 3 and photo[y[5], x[5]].tolist() == [9] * 3 and photo[y[6], x[6]].tolist() == [40] * 3
    assert img[y[6], x[6]] == 255 and img[y[5], x[5]] == 2 and img[y[0], x[0]] == 1
    rest = np.ones(T * P, bool)
    rest[:7] = False
    assert np.array_equal(photo[y[rest], x[rest]], atlas[y[rest], x[rest]]) and (img[y[rest], x[rest]] == 0).all()
    own = owned_mask(T, n, C, img.shape)
    assert (~own).sum() > 0 and (photo[~own] == np.array(FILL, np.uint8)).all() and (img[~own] == 0).all()
    two, img2 = ph.blend(acc, seen, T, n, C, atlas, min_seen=2)
    assert np.array_equal(img2, img)
    assert np.array_equal(two[y[:5], x[:5]], atlas[y[:5], x[:5]])            # seen < min_seen: the field's byte
    assert two[y[5], x[5]].tolist() == [9] * 3 and two[y[6], x[6]].tolist() == [40] * 3
    for bad in (0, -1, 1.0, True):
        with pytest.raises(ValueError, match='min_seen'):
            ph.blend(acc, seen, T, n, C, atlas, min_seen=bad)


# ------------------------------------------------------------------ visibility
def _seen_of(pos, faces, K, E, H, W, b, n=5, pflag=None, inside=None, photo=None):
    T = len(faces)
    acc, seen = ph.accumulators(T, n)
    tri_w, ok = ph.project_frame(faces, n, pos, np.zeros(len(pos), np.uint8) if pflag is None else pflag, K, E,
                                 ph.constant_photo(H, W, 50) if photo is None else photo,
                                 np.ones((H, W), np.uint8) if inside is None else inside, b, acc, seen)
    return tri_w, ok.reshape(T, -1), acc


def test_two_quads_and_the_depth_bias():
    H = W = 48
    D = 0.25
    pos, faces, K, E = ph.two_quads(D, H, W)
    tri_w, near_only, _ = _seen_of(pos, faces, K, E, H, W, b=0.1, n=8)
    assert (tri_w > 200).all()
    assert near_only[:2].sum() > 10 and near_only[2:].sum() == 0             # b < D: the far quad lies behind the near one
    _, both, _ = _seen_of(pos, faces, K, E, H, W, b=0.3, n=8)
    assert np.array_equal(both[:2], near_only[:2]) and both[2:].sum() > 10   # b > D: the rule lets it through
    # the far quad alone is seen at any bias
    _, alone, _ = _seen_of(pos, faces[2:], K, E, H, W, b=0.0, n=8)
    assert alone.sum() >= both[2:].sum() > 10
    with pytest.raises(ValueError, match='bias'):
        _seen_of(pos, faces, K, E, H, W, b=-0.1)
    with pytest.raises(ValueError, match='bias'):
        _seen_of(pos, faces, K, E, H, W, b=float('nan'))


def test_mask_border_empty_keys_flags_and_winding():
    H = W = 48
    pos, faces, K, E = ph.two_quads(0.25, H, W)
    faces, n = faces[:2], 8
    _, ok, _ = _seen_of(pos, faces, K, E, H, W, 0.05, n)
    assert ok.sum() > 20
    _, none, acc = _seen_of(pos, faces, K, E, H, W, 0.05, n, inside=np.zeros((H, W), np.uint8))
    assert none.sum() == 0 and not acc.any()                                 # inside all zero: nothing seen
    # a hole in the mask takes out the texels whose taps touch it, and no other
    inside = np.ones((H, W), np.uint8)
    inside[20, 20] = 0
    _, holed, _ = _seen_of(pos, faces, K, E, H, W, 0.05, n, inside=inside)
    q, _ = tex.texel_points(pos, faces, n)
    xy, _, _ = mrr.project(q.reshape(-1, 3), K, E)
    j0, i0 = xy[:, 0] >> 8, xy[:, 1] >> 8
    touch = ((i0 == 20) | (i0 == 19)) & ((j0 == 20) | (j0 == 19))
    assert np.array_equal(holed.ravel(), ok.ravel() & ~touch) and (ok.ravel() & touch).sum() > 0
    # taps on an empty key: the quad's own edge texels (the rim lies outside the triangle, on pixels nothing covers)
    keys = ph.frame_keys(pos, faces, K, E, H, W)
    empty = keys == mrr.EMPTY_KEY
    inb = (i0 >= 0) & (j0 >= 0) & (i0 + 1 < H) & (j0 + 1 < W)
    e = np.zeros(len(i0), bool)
    e[inb] = empty[i0[inb], j0[inb]] | empty[i0[inb] + 1, j0[inb]] | empty[i0[inb], j0[inb] + 1] | empty[i0[inb] + 1, j0[inb] + 1]
    assert (e & inb).sum() > 0 and not (ok.ravel() & e).any()
    # a quad that fills the image: texels whose taps reach the last row or column, or leave the image, are not seen
    uv = np.array([[-6, -6], [W + 5, -6], [-6, H + 5], [W + 5, H + 5]], dtype=np.float64)
    big = mrr.unproject(K, E, uv, np.full(4, 3.0))
    tri_w, okb, _ = _seen_of(big, faces, K, E, H, W, 0.05, 64)
    qb, _ = tex.texel_points(big, faces, 64)                                 # (less than a pixel between texels)
    xyb, _, _ = mrr.project(qb.reshape(-1, 3), K, E)
    jb, ib = xyb[:, 0] >> 8, xyb[:, 1] >> 8
    outside = (jb < 0) | (ib < 0) | (jb + 1 > W - 1) | (ib + 1 > H - 1)
    assert (tri_w > 0).all() and outside.sum() > 0 and not (okb.ravel() & outside).any()
    assert np.array_equal(okb.ravel(), ~outside)                              # every other texel of it is seen
    assert ((jb == W - 2) & ~outside).any() and (jb == W - 1).any()           # the last column is a tap of some, the origin of others
    assert ((ib == H - 2) & ~outside).any() and (ib == H - 1).any() and ((jb == 0) & ~outside).any() and (jb == -1).any()
    # a flagged vertex: its triangles unseen, the others as before
    pflag = np.zeros(len(pos), np.uint8)
    pflag[0] = 2                                                              # vertex 0 belongs to triangle 0 alone
    tri_w, flagged, _ = _seen_of(pos, faces, K, E, H, W, 0.05, n, pflag=pflag)
    assert tri_w[0] == 0 and tri_w[1] > 0 and flagged[0].sum() == 0 and np.array_equal(flagged[1], ok[1])
    # reversed winding: unseen, and counted as facing away
    tri_w, rev, _ = _seen_of(pos, np.ascontiguousarray(faces[:, [0, 2, 1]]), K, E, H, W, 0.05, n)
    assert (tri_w == -1).all() and rev.sum() == 0
    # an index outside [0, V)
    bad = faces.copy()
    bad[1, 2] = len(pos)
    with pytest.raises(ValueError, match=r'a face index lies outside \[0, 8\)'):
        _seen_of(pos, bad, K, E, H, W, 0.05, n)


def test_weight():
    K, E = np.array([[64.0, 0, 32], [0, 64.0, 32], [0, 0, 1]]), np.eye(4)
    tri = np.array([[1.0, 0, 0], [-0.5, np.sqrt(0.75), 0], [-0.5, -np.sqrt(0.75), 0]]) * 0.1      # centred on the origin, in z = 0
    facing = tri[[0, 2, 1]]                                                  # normal towards -z: towards the camera at the origin

    def weight(p, pflag=(0, 0, 0), faces=((0, 1, 2),)):
        return ph.triangle_weights(p.astype(np.float32), np.array(pflag, np.uint8), np.array(faces, np.int32), K, E)
    assert weight(facing + [0, 0, 4.0])[0].tolist() == [256]
    assert weight(tri + [0, 0, 4.0])[0].tolist() == [-1]
    a = np.pi / 3
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    assert weight(facing @ R.T + [0, 0, 4.0])[0].tolist() == [64]             # cos^2 60 deg = 1/4
    edge_on = np.array([[0, -0.1, 3.9], [0, 0.1, 4.0], [0, 0.0, 4.1]])        # in the plane x = 0 through the camera
    assert weight(edge_on)[0].tolist() == [0]
    assert weight(np.array([[0, 0, 4.0], [0.1, 0, 4.0], [0.2, 0, 4.0]]))[0].tolist() == [0]       # collinear: N = 0
    assert weight(facing[[0, 0, 1]] + [0, 0, 4.0])[0].tolist() == [0]                             # a repeated vertex
    assert weight(facing + [0, 0, 4.0], pflag=(0, 1, 0))[0].tolist() == [0]                       # a posing flag
    assert weight(facing + [0, 0, 0.0])[0].tolist() == [0]                                        # nearer than NEAR: section 7j's flag 1
    assert weight(facing * 1e5 + [0, 0, 4.0])[0].tolist() == [0]                                  # past the guard band: flag 2
    w, status = weight(facing + [0, 0, 4.0], faces=((0, 1, 3),))
    assert w.tolist() == [0] and status == 1                                                      # an index equal to V
    assert weight(facing + [0, 0, 4.0], faces=((0, -1, 2),))[1] == 1
    w, status = weight(np.full((3, 3), np.nan))
    assert w.tolist() == [0] and status == 0
    assert ph.triangle_weights(np.zeros((0, 3), np.float32), np.zeros(0, np.uint8), np.zeros((0, 3), np.int32), K, E)[0].shape == (0,)


def test_the_sign_of_facing_on_an_extracted_sphere():
    """Marching tetrahedra winds its triangles so that the signed volume of a solid is positive (sections 7h, 7m): (b - a) x
    (c - a) points outwards.  Seen from outside, the near side of the sphere has d < 0 and a weight, the far side d > 0."""
    field, centre = mr.sphere_field()
    verts, faces = mr.extract_mesh(field, 0.0, np.zeros(3), 1.0)
    assert mr.is_closed(faces) and mr.signed_volume(verts, faces) > 0.0
    K, E = mrr.pinhole(64, 64, cz=30.0)
    E[:3, 3] = [-centre[0], -centre[1], 30.0 - centre[2]]                     # the camera 30 voxels in front of the centre, on -z
    tri_w, status = ph.triangle_weights(verts, np.zeros(len(verts), np.uint8), faces, K, E)
    mid = verts[faces].astype(np.float64).mean(1) - centre
    assert status == 0 and (tri_w[mid[:, 2] < -2.0] > 0).all() and (tri_w[mid[:, 2] > 2.0] == -1).all()
    assert (tri_w > 0).sum() > 100 and (tri_w < 0).sum() > 100
    # and through the whole definition: only the near side receives the photograph
    n = 4
    _, ok, _ = _seen_of(verts, faces, K, E, 64, 64, 0.5, n)
    assert ok[mid[:, 2] < -2.0].sum() > 100 and ok[mid[:, 2] > 0.5].sum() == 0


# ------------------------------------------------------------------ planted colours
def planted_colours(path, frames=(0, 1, 3), n=4, size=64):
    """The capsule body (occnerf_amd.synth.SyntheticSMPL: canonical vertices and faces, all 13 684 triangles) posed per frame by
    the dataset tool's own forward kinematics, the frames of a tool-made dataset as photographs and masks -> the absolute byte
    errors of the seen texels against vertex_colours of their canonical texel points, the same for an atlas of the fill colour
    (no checkpoint is at hand without a GPU), and the seen counts."""
    from occnerf_amd import synth
    from occnerf_amd.dataset import PreparedDataset
    tool = mrr.load_tool()
    tool.make_dataset(path, frames=4, width=size, height=size, seed=0)
    ds = PreparedDataset(path, device=None)
    with open(os.path.join(path, 'mesh_infos.pkl'), 'rb') as f:
        infos = pickle.load(f)
    canonical, _ = synth.SyntheticSMPL()(np.zeros(72), np.zeros(10, np.float32))
    items, faces = [], None
    for i in frames:
        f = ds.frames[i]
        pos, faces, _ = mrr.posed_smpl(tool, infos[f['frame_name']])
        items.append((pos, np.zeros(len(pos), np.uint8), f['K'], f['E'], ds.truth_u8(i), (np.asarray(ds.gt_alpha(i)) > 0.5).astype(np.uint8)))
    assert mr.signed_volume(canonical, faces) > 0.0                          # wound as the exported mesh is
    T = len(faces)
    C, _, W, H, P = tex.layout(T, n)
    baseline = np.zeros((H, W, 3), np.uint8)                                  # mesh_texture.fill's default
    photo, img, acc, seen = ph.photo_texture(faces, n, items, 0.05, baseline, C)
    q, _ = tex.texel_points(canonical.astype(np.float32), faces, n)
    truth = tool.vertex_colours(q.reshape(-1, 3).astype(np.float64)).astype(np.int64)
    x, y = ph.atlas_index(T, n, C)
    hit = seen > 0
    err = np.abs(photo[y[hit], x[hit]].astype(np.int64) - truth[hit])
    base = np.abs(baseline[y[hit], x[hit]].astype(np.int64) - truth[hit])
    return {'frames': list(frames), 'cell': n, 'image': [size, size], 'triangles': T, 'owned_texels': T * P, 'seen_texels': int(hit.sum()),
            'unseen_texels': int((~hit).sum()), 'seen_histogram': ph.seen_histogram(seen),
            'abs_byte_error': {'median': float(np.median(err)), 'p95': float(np.percentile(err, 95))},
            'baseline_fill_colour': {'median': float(np.median(base)), 'p95': float(np.percentile(base, 95))}}


def test_planted_colours_come_back(tmp_path):
    got = planted_colours(str(tmp_path / 'ds'))
    print(f"\n   {got['seen_texels']} of {got['owned_texels']} texels seen; |byte error| median {got['abs_byte_error']['median']}, 95 % "
          f"{got['abs_byte_error']['p95']}; an atlas of the fill colour: {got['baseline_fill_colour']}")
    assert got['seen_texels'] > 0 and got['unseen_texels'] > 0
    assert got['abs_byte_error']['median'] < got['baseline_fill_colour']['median']
    recorded = json.load(open(os.path.join(ROOT, 'profiles', 'mesh_photo_check.json')))
    for key in ('frames', 'cell', 'image', 'triangles', 'owned_texels'):      # the recorded run is this case (its figures: measured, not judged)
        assert recorded['planted_colours'][key] == json.loads(json.dumps(got[key])), key


# ------------------------------------------------------------------ keys, refusals, wiring and the writer
def test_keys_refusals_and_wiring():
    import torch

    from occnerf_amd import _lib, mesh, ops
    from occnerf_amd.config import default_cfg
    want = {'enable': False, 'frames': 'all', 'bias': None, 'min_seen': 1, 'in_glb': True}
    assert dict(default_cfg().mesh_photo) == want == mesh.PHOTO_DEFAULTS
    cfg = default_cfg().merge_from_list(['mesh_photo.enable', 'True', 'mesh_photo.frames', '[0, 3, 17]', 'mesh_photo.bias', '0.02',
                                         'mesh_photo.min_seen', '2', 'mesh_photo.in_glb', 'False'])
    assert mesh.check_photo(cfg.mesh_photo) == {'enable': True, 'frames': [0, 3, 17], 'bias': 0.02, 'min_seen': 2, 'in_glb': False}
    assert mesh.check_photo({}) == want
    for key, value, word in (('enable', 1, 'mesh_photo.enable = 1'), ('in_glb', 'yes', "mesh_photo.in_glb = 'yes'"),
                             ('frames', 'some', "mesh_photo.frames = 'some'"), ('frames', [], 'mesh_photo.frames = []'),
                             ('frames', [0, -1], 'mesh_photo.frames'), ('frames', [0.5], 'mesh_photo.frames'), ('frames', None, 'mesh_photo.frames'),
                             ('bias', -0.1, 'mesh_photo.bias = -0.1'), ('bias', float('nan'), 'mesh_photo.bias'), ('bias', 'h', 'mesh_photo.bias'),
                             ('bias', float('inf'), 'mesh_photo.bias'), ('min_seen', 0, 'mesh_photo.min_seen = 0'),
                             ('min_seen', 1.5, 'mesh_photo.min_seen'), ('min_seen', True, 'mesh_photo.min_seen')):
        with pytest.raises(RuntimeError, match=re.escape(word)):
            mesh.check_photo({**mesh.PHOTO_DEFAULTS, key: value})
    with pytest.raises(RuntimeError, match='mesh_photo.enable: the photographs and masks are those of a prepared dataset'):
        mesh.export_photo_texture(None, '/nonexistent', {}, None, want)
    # the C entries refuse before any launch
    lib = _lib.lib()
    p = 4096
    K = np.array([[64.0, 0, 32], [0, 64.0, 32], [0, 0, 1]])
    E = np.eye(4)

    def refused(rc, who, word):
        msg = lib.occnerf_last_error().decode()
        assert rc != 0 and msg.startswith(who) and word in msg, (rc, msg)

    def project(xy=p, V=3, faces=p, T=1, n=8, K=K, E=E, keys=p, H=8, W=8, bias=0.01, acc=p, status=p):
        return lib.occnerf_mesh_texture_project(xy, p, p, p, p, V, faces, T, n, None if K is None else K.ctypes.data,
                                                None if E is None else E.ctypes.data, keys, p, p, H, W, bias, acc, p, p, status, None)
    skew = K.copy()
    skew[0, 1] = 0.5
    refused(project(xy=None), 'mesh_texture_project', 'null')
    refused(project(acc=None), 'mesh_texture_project', 'null')
    refused(project(status=None), 'mesh_texture_project', 'null')
    refused(project(K=None), 'mesh_texture_project', 'null')
    refused(project(H=0), 'mesh_texture_project', 'H=0')
    refused(project(W=16385), 'mesh_texture_project', 'W=16385')
    refused(project(T=(1 << 31) // 28 + 1), 'mesh_texture_project', 'reaches 2^31')
    refused(project(K=skew), 'mesh_texture_project', 'skew')
    refused(project(bias=-1.0), 'mesh_texture_project', 'bias')
    refused(project(bias=float('nan')), 'mesh_texture_project', 'bias')
    refused(project(n=3), 'mesh_texture_project', 'n=3')
    assert project(T=0, xy=None, faces=None, keys=None, acc=None, status=None) == 0
    refused(lib.occnerf_mesh_texture_blend(p, p, 9, 8, 3, 16, 25, 1, p, p, None), 'mesh_texture_blend', 'does not hold')     # W != C n
    refused(lib.occnerf_mesh_texture_blend(p, p, 9, 8, 3, 8, 24, 1, p, p, None), 'mesh_texture_blend', 'does not hold')      # a row short
    refused(lib.occnerf_mesh_texture_blend(p, p, 9, 8, 3, 16, 24, 0, p, p, None), 'mesh_texture_blend', 'min_seen=0')
    refused(lib.occnerf_mesh_texture_blend(None, p, 9, 8, 3, 16, 24, 1, p, p, None), 'mesh_texture_blend', 'null')
    refused(lib.occnerf_mesh_texture_blend(p, p, 9, 8, 3, 16, 24, 1, p, None, None), 'mesh_texture_blend', 'null')
    refused(lib.occnerf_mesh_texture_blend(p, p, 9, 65, 3, 16, 24, 1, p, p, None), 'mesh_texture_blend', 'n=65')
    assert lib.occnerf_mesh_texture_blend(None, None, 0, 8, 1, 8, 8, 1, None, None, None) == 0
    # the wrappers refuse host tensors by name
    z = torch.zeros
    with pytest.raises(RuntimeError, match='mesh_texture_project: verts must be a CUDA'):
        ops.mesh_texture_project(z(28, 2, dtype=torch.int32), z(28, dtype=torch.float64), z(28, dtype=torch.uint8), z(3, 3),
                                 z(3, dtype=torch.uint8), z(1, 3, dtype=torch.int32), 8, K, E, z(8, 8, dtype=torch.int64),
                                 z(8, 8, 3, dtype=torch.uint8), z(8, 8, dtype=torch.uint8), 0.01, z(28, 4, dtype=torch.int64),
                                 z(28, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='mesh_texture_blend: acc must be a CUDA'):
        ops.mesh_texture_blend(z(28, 4, dtype=torch.int64), z(28, dtype=torch.int32), 1, 8, 1, z(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='mesh_texture_blend: cell = 3'):
        ops.mesh_texture_blend(z(28, 4, dtype=torch.int64), z(28, dtype=torch.int32), 1, 3, 1, z(8, 8, 3, dtype=torch.uint8))
    run = open(os.path.join(ROOT, 'run.py')).read()
    assert 'export_photo_texture(' in run and "mph.get('enable', False)" in run and 'mesh_photo.enable' in run
    header = open(os.path.join(ROOT, 'include', 'occnerf_hip.h')).read()
    for name in ('occnerf_mesh_texture_project', 'occnerf_mesh_texture_blend'):
        assert name in _lib.SIGNATURES and f'int {name}(' in header
    assert '#define OCCNERF_ABI_VERSION 5' in header and _lib.ABI_VERSION == 5
    # the definition and the kernels state the same constants: once, in the header the rasteriser and the weights share
    csrc = os.path.join(ROOT, 'occnerf_amd', 'csrc')
    src = open(os.path.join(csrc, 'mesh_screen.h')).read()
    for text, value in (('kScreenNear = 1e-3', mrr.NEAR), ('kScreenFar = 1048576.0', mrr.FAR), ('kScreenGuard = 4194304.0', mrr.GUARD)):
        assert src.count(text) == 1 and float(text.split('= ')[1]) == float(value), text
    for name in ('mesh_raster.hip', 'mesh_texture.hip'):
        own = re.sub(r'//[^\n]*', '', open(os.path.join(csrc, name)).read())
        assert not re.search(r'\bk\w*(Near|Far|Guard)\w*\s*=', own), name
        assert not re.search(r'1e-3|1048576|4194304|struct \w*Camera', own), name


def test_write_glb_depends_on_the_png_only_through_its_bytes(tmp_path):
    """The photo atlas replaces the field's in rigged.glb / textured.glb through the `png` handed to gltf.write_glb alone:
    equal inputs give equal files, two images of different length give files that differ in the image and the lengths that
    follow from it, and the default path still writes its recorded bytes."""
    from occnerf_amd import gltf, mesh
    from tests import test_mesh_texture_restatement as cpu
    v, f, c, j, w, g, nrm, anim, corr = cpu.tiny_rig()
    T, n = f.shape[0], 5
    _, _, W, H, _ = mesh.atlas_layout(T, n)
    rng = np.random.RandomState(3)
    noisy, flat = rng.randint(0, 256, (H, W, 3)).astype(np.uint8), np.full((H, W, 3), 77, np.uint8)
    uv = mesh.texture_uv(T, n)
    blobs = {}
    for name, atlas in (('a', noisy), ('b', noisy), ('c', flat)):
        path = str(tmp_path / f'{name}.glb')
        gltf.write_glb(path, v, f, None, j, w, g, normals=nrm, animation=anim, texture={'uv': uv, 'png': cpu._png(atlas)})
        blobs[name] = open(path, 'rb').read()
    assert blobs['a'] == blobs['b'] and len(cpu._png(noisy)) != len(cpu._png(flat))
    for name, atlas in (('a', noisy), ('c', flat)):
        doc, buf, att, idx, image = tex.read_textured(blobs[name])
        assert np.array_equal(image, atlas) and att['TEXCOORD_0'].tobytes() == uv.tobytes()
        assert att['POSITION'].tobytes() == v[f.reshape(-1)].tobytes()
    assert cpu.write_recorded(tmp_path / 'recorded') == [cpu.PLAIN_SHA256, cpu.FULL_SHA256]
