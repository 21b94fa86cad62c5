"""CPU: the numpy definition of the geometry maps (tests/gbuffer_restatement.py) held against analytic
surfaces and against hand cases whose answer can be read off their inputs.  The kernels are held against the definition in
tests/test_r_gbuffer.py."""
import numpy as np
import pytest

from occnerf_amd import synth
from tests import gbuffer_cases as cases
from tests import gbuffer_restatement as G

U = float(np.finfo(np.float32).eps) / 2            # the unit roundoff of float32: one rounding errs by at most U |x|


def _camera_rays(size):
    K, E = synth.setup_camera(size)
    o, d = synth.get_rays_from_KRT(size, size, K, E[:3, :3], E[:3, 3])
    return np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)


def _angle(u, v):
    """Angle between unit vectors, accurate near 0."""
    return 2.0 * np.arcsin(np.clip(np.linalg.norm(u - v, axis=-1) / 2.0, 0.0, 1.0))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rounding_bound(o, d, t, sec_a, sec_b):
    """First-order bound on the angle (radians) by which float32 rounding turns the definition's normal, from the inputs:
    a point component errs by U |t d_c| (t's own rounding) + U |t d_c| (the product) + U |P_c| (the sum) <= E; a secant
    component by 2 E + U |a_c| (its subtraction), so the secant turns by at most eps = sqrt(3) (2 E + U max|a_c|) / |a|; each
    cross-product component carries three roundings of terms bounded by |a| |b|, and the normalisation four more.  The
    normal of secants meeting at the angle phi then turns by at most (eps_a + eps_b + eps_a eps_b + 6 sqrt(3) U) / sin(phi) + 4 U."""
    td = np.abs(t[:, None] * d)
    E = U * (2.0 * td.max() + np.abs(o + t[:, None] * d).max())
    la, lb = np.linalg.norm(sec_a, axis=-1), np.linalg.norm(sec_b, axis=-1)
    ea = np.sqrt(3.0) * (2.0 * E + U * np.abs(sec_a).max(-1)) / la
    eb = np.sqrt(3.0) * (2.0 * E + U * np.abs(sec_b).max(-1)) / lb
    sin_phi = np.linalg.norm(np.cross(sec_a, sec_b), axis=-1) / (la * lb)
    return (ea + eb + ea * eb + 6.0 * np.sqrt(3.0) * U) / sin_phi + 4.0 * U


def test_plane_float32_against_float64():
    """A tilted plane in front of the camera, alpha = 1: the float64 evaluation returns the plane's normal, and the float32
    definition stays within the rounding bound derived from the inputs (the rounding of P over the secant length)."""
    size = 64
    o, d = _camera_rays(size)
    normal = _unit(np.array([0.3, -0.2, 1.0]))
    t = (normal @ np.array([0.1, -0.2, 0.4]) - o @ normal) / (d @ normal)
    assert (t > 1.0).all()
    idx = np.arange(size * size)
    kw = dict(H=size, W=size, ray_index=idx, rays=np.stack([o, d], 0), alpha=np.ones(size * size), min_alpha=0.5)
    g64 = G.geometry_maps(depth=t, dtype=np.float64, **kw)
    g32 = G.geometry_maps(depth=t.astype(np.float32), dtype=np.float32,
                          **{**kw, 'rays': np.stack([o, d], 0).astype(np.float32)})
    assert (g64['valid'] == 3).all() and (g32['valid'] == 3).all()
    n64 = g64['normal'].reshape(-1, 3)
    assert _angle(n64, np.broadcast_to(normal, n64.shape)).max() < 1e-9          # facing the camera: d . n < 0 everywhere
    # the camera's rays are float32 values, so both evaluations start from the same o and d; t is rounded for float32 only
    bound = _rounding_bound(o, d, t, g64['sec_a'].reshape(-1, 3), g64['sec_b'].reshape(-1, 3))
    err = _angle(g32['normal'].reshape(-1, 3).astype(np.float64), n64)
    print(f'\n   plane {size}^2: max angle float32 vs float64 {err.max():.3e} rad, bound {bound.min():.3e} .. {bound.max():.3e}')
    assert (err <= bound).all() and bound.max() < 1e-2
    assert np.abs(g32['t'].astype(np.float64) - g64['t']).max() <= U * np.abs(t).max()
    shade = -(n64 * _unit(d)).sum(-1)
    assert np.abs(g32['shade'].reshape(-1) - shade).max() <= bound.max() + 8 * U


def _sphere(size, dtype):
    rho, centre = 0.6, np.array([0.05, -0.3, 0.2])
    o, d = _camera_rays(size)
    oc = o - centre
    A, B, C = (d * d).sum(-1), (oc * d).sum(-1), (oc * oc).sum(-1) - rho * rho
    disc = B * B - A * C
    hit = disc > 0
    t = np.where(hit, (-B - np.sqrt(np.where(hit, disc, 0.0))) / A, 0.0)           # the near intersection
    g = G.geometry_maps(size, size, np.arange(size * size), np.stack([o, d], 0).astype(dtype), t.astype(dtype),
                        hit.astype(dtype), min_alpha=0.5, dtype=dtype)
    P = o + t[:, None] * d
    truth = np.where(hit[:, None], (P - centre) / rho, 0.0)
    return g, o, d, t, truth, rho


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_sphere_secants_stay_inside_the_chord_bound(dtype):
    """A sphere of radius rho: a secant of chord c leaves the tangent plane at its pixel's point by delta = asin(c / 2 rho).
    With a = cos(da) u + sin(da) N and b = cos(db) v + sin(db) N (u, v unit tangents meeting at phi, N the true normal)
    a x b = cos(da) cos(db) sin(phi) N + a tangent part of length <= sin(da + db), so the normal is off by at most
    atan((tan(da) + tan(db)) / sin(phi)).  Checked per pixel whose secants meet at 60..120 degrees, with the float32 rounding
    bound on top; and the worst error falls when the resolution doubles."""
    worst = []
    for size in (64, 128):
        g, o, d, t, truth, rho = _sphere(size, dtype)
        a, b = g['sec_a'].reshape(-1, 3).astype(np.float64), g['sec_b'].reshape(-1, 3).astype(np.float64)
        nv = (g['valid'].reshape(-1) & 2) != 0
        with np.errstate(all='ignore'):
            cos_ab = (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))
        use = nv & (np.abs(cos_ab) <= 0.5)                                        # 60 .. 120 degrees
        assert use.sum() > 0.5 * nv.sum() > 0.02 * size * size
        a, b, N = a[use], b[use], truth[use]
        da = np.arcsin(np.linalg.norm(a, axis=-1) / (2 * rho))
        db = np.arcsin(np.linalg.norm(b, axis=-1) / (2 * rho))
        ua, ub = _unit(a - (a * N).sum(-1, keepdims=True) * N), _unit(b - (b * N).sum(-1, keepdims=True) * N)
        sin_phi = np.linalg.norm(np.cross(ua, ub), axis=-1)
        bound = np.arctan((np.tan(da) + np.tan(db)) / sin_phi) * (1 + 1e-9) + 1e-12
        if dtype == np.float32:
            bound = bound + _rounding_bound(o[use], d[use], t[use], a, b)
        err = _angle(g['normal'].reshape(-1, 3)[use].astype(np.float64), N)
        print(f'\n   sphere {size}^2 {np.dtype(dtype).name}: {int(use.sum())} pixels, max angle {err.max():.4e} rad, '
              f'largest bound {bound.max():.4e}, smallest slack {(bound - err).min():.3e}')
        assert (err <= bound).all()
        assert ((g['normal'].reshape(-1, 3)[use] * d[use]).sum(-1) < 0).all()       # towards the camera
        worst.append(err.max())
    assert worst[1] < worst[0]


def _run(case, **kw):
    return G.geometry_maps(**{**cases.definition_args(case), **kw})


def test_borders_and_a_full_frame():
    g = _run(cases.hand_cases()['borders'])
    assert (g['valid'] == 3).all()                                               # R = H W, one-sided secants at the borders
    want = np.array([0.5, 0.25, -1.0], np.float32) / np.sqrt(np.float32(1.3125))  # (1,0,.5) x (0,1,.25) = (-.5,-.25,1), flipped
    assert np.array_equal(g['normal'], np.broadcast_to(want, (3, 3, 3)))
    assert g['left'][:, 2].all() and not g['left'][:, :2].any() and g['up'][2].all() and not g['up'][:2].any()
    assert np.array_equal(g['t'], cases.hand_cases()['borders']['depth'].reshape(3, 3))
    grey = G.to_8b((np.float32(8.0) - g['t']) / np.float32(8.0))
    assert np.array_equal(g['depth_u8'], np.repeat(grey[..., None], 3, -1))
    assert np.array_equal(g['shaded_u8'], np.full((3, 3, 3), G.to_8b(-want[2]), np.uint8))
    assert np.array_equal(g['normal_u8'], np.broadcast_to(G.to_8b(np.float32(0.5) * want + np.float32(0.5)), (3, 3, 3)))


def test_a_pixel_without_a_vertical_neighbour_keeps_its_depth():
    g = _run(cases.hand_cases()['one_row'])
    assert np.array_equal(g['valid'], [[0, 0, 0], [1, 1, 1], [0, 0, 0]])
    assert np.array_equal(g['t'][1], [1.0, 1.5, 2.0]) and not g['normal'].any()
    bg8 = G.to_8b(np.array(cases.BG, np.float32))
    assert (g['normal_u8'] == bg8).all() and (g['shaded_u8'] == bg8).all() and (g['depth_u8'][0] == bg8).all()
    assert (g['depth_u8'][1, :, 0] == G.to_8b((np.float32(8) - g['t'][1]) / np.float32(8))).all()


def test_ties_go_right_and_down():
    g = _run(cases.hand_cases()['tie'])
    assert not g['left'][1, 1] and not g['up'][1, 1]
    # horizontally 2, 1, 2 and vertically 2, 1, 2: |dt| = 1 on every side.  Right gives (1, 0, +1), left would give (1, 0, -1)
    assert np.array_equal(g['sec_a'][1, 1], [1.0, 0.0, 1.0]) and np.array_equal(g['sec_b'][1, 1], [0.0, 1.0, 1.0])
    # the other middles tie too: (0, 1) between 3 and 3 horizontally, (1, 0) and (1, 2) between 3 and 3 vertically
    assert not g['left'][0, 1] and np.array_equal(g['sec_a'][0, 1], [1.0, 0.0, 1.0])
    for j in (0, 2):
        assert not g['up'][1, j] and np.array_equal(g['sec_b'][1, j], [0.0, 1.0, 1.0])
    assert g['up'][2, 1] and g['left'][1, 2]                                     # borders: the only candidate


def test_a_silhouette_step_takes_the_near_side():
    g = _run(cases.hand_cases()['step'])
    assert g['left'][:, 1].all() and not g['left'][:, 2].any()                   # column 1 looks left, column 2 looks right
    assert np.array_equal(g['sec_a'][0, 1], [1.0, 0.0, 0.25]) and np.array_equal(g['sec_a'][0, 2], [1.0, 0.0, 0.25])
    assert (g['valid'] == 3).all()
    assert np.array_equal(g['normal'][0, 1], g['normal'][0, 2])                  # the step leaves no trace in the normals


def test_alpha_threshold_zero_and_not_finite():
    h = cases.hand_cases()
    g = _run(h['threshold'])
    assert g['valid'][1, 1] == 0 and g['valid'][1, 2] & 1 and g['t'][1, 1] == 0 and g['t'][1, 2] == 2.0
    assert not g['points'][1, 1].any()
    g = _run(h['zero_alpha'])
    assert g['valid'][1, 1] == 0 and g['valid'][1, 2] == 0 and (np.delete(g['valid'].ravel(), [4, 5]) & 1).all()
    g = _run(h['not_finite'])
    assert [g['valid'].ravel()[k] for k in (1, 4, 7)] == [0, 0, 0] and (np.delete(g['valid'].ravel(), [1, 4, 7]) & 1).all()
    assert np.isfinite(g['normal']).all() and np.isfinite(g['points']).all()
    # the column 1 is gone altogether: the pixels of columns 0 and 2 have a horizontal neighbour only through it
    assert not (g['valid'] & 2).any()


def test_degenerate_cross_product_and_no_rays():
    h = cases.hand_cases()
    g = _run(h['degenerate'])
    assert (g['valid'] == 1).all() and not g['normal'].any()                     # l2 = 0: the depth stays valid
    g = _run(h['no_rays'])
    bg8 = G.to_8b(np.array(cases.BG, np.float32))
    assert not g['valid'].any() and not g['points'].any() and not g['normal'].any()
    for k in ('depth_u8', 'normal_u8', 'shaded_u8'):
        assert g[k].shape == (2, 3, 3) and (g[k] == bg8).all()


def test_depth_range_edges():
    h = cases.hand_cases()
    g = _run(h['empty_range'])
    assert (g['valid'] & 1).all() and not g['depth_u8'].any()                    # 0 / 0 -> grey 0, not the background
    g = _run(h['outside_range'])
    assert np.array_equal(g['depth_u8'][0, :, 0], [255, 0, G.to_8b(np.float32(6.0) / np.float32(7.0))])
    near, far = np.array([[2.0], [1.5]], np.float32), np.array([[3.0], [4.5]], np.float32)
    assert G.default_t_range(near, far) == (np.float32(1.5), np.float32(4.5))


def test_random_frames_cover_what_they_are_for():
    """The seeded frames of the GPU test: every validity class, both secant sides, ties and all three ray shares occur."""
    ties = vties = 0
    for name, case in cases.random_cases().items():
        g = _run(case)
        H, W = case['H'], case['W']
        share = case['ray_index'].size / (H * W)
        assert abs(share - float(name.rsplit('_', 1)[1]) / 100) < 0.05
        v = g['valid']
        if share > 0.5:
            assert {0, 1, 3} <= set(np.unique(v).tolist())
            assert g['left'][v == 3].any() and (~g['left'][v == 3]).any() and g['up'][v == 3].any()
        t = g['t']
        inner = (v[1:-1, 1:-1] & 1) & (v[1:-1, 2:] & 1) & (v[1:-1, :-2] & 1)
        ties += int((inner & (np.abs(t[1:-1, 2:] - t[1:-1, 1:-1]) == np.abs(t[1:-1, 1:-1] - t[1:-1, :-2]))).sum())
        inner = (v[1:-1, 1:-1] & 1) & (v[2:, 1:-1] & 1) & (v[:-2, 1:-1] & 1)
        vties += int((inner & (np.abs(t[2:, 1:-1] - t[1:-1, 1:-1]) == np.abs(t[1:-1, 1:-1] - t[:-2, 1:-1]))).sum())
        assert np.isfinite(g['normal']).all()
    assert ties > 100 and vties > 100
