"""GPU: the collapsed-sample classification (csrc/center.hip) against the feature kernel it stands in for, and the list split
(csrc/compact.hip) against NumPy.

A flagged sample leaves the list the kNN and feature kernels run on and the canonical MLP reads the centre row for it.  That is
only right if the feature kernel WOULD have written the centre row for it, bit for bit, whatever the other seven samples of its
trip are -- which is what this file checks on a hand-made list: copies of the collapse point, points a few ulp off it, points on
both sides of the radius to the last bit, far points and real samples of a body ray, in all-inside, all-outside and mixed
trips of 8, 4 099 entries (no multiple of 8, 64 or 256) in a list with spare capacity."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV, T

pytestmark = pytest.mark.gpu

N_LIST = 4099
N_XYZ = 49 * 128            # the kNN kernel takes rays x samples; the list picks N_LIST of these positions (a capacity of
                            # 6 144 or more selects the feature kernel's one-workgroup-per-CU form, the renderer's)
N_COPIES = 1024


def _rn32(v):
    """The float32 nearest to the exact rational v, ties to even."""
    f = np.float32(float(v))
    best = None
    for cand in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
        key = (abs(Fraction(float(cand)) - v), int(np.float32(cand).view(np.int32)) & 1)
        if best is None or key < best[0]:
            best = (key, np.float32(cand))
    return best[1]


def _d2(p, c):
    """fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with float32 differences: the kernels' squared distance, every rounding exact."""
    dx, dy, dz = (np.float32(p[k]) - np.float32(c[k]) for k in range(3))
    t = np.float32(dx * dx)
    t = _rn32(Fraction(float(dy)) ** 2 + Fraction(float(t)))
    return _rn32(Fraction(float(dz)) ** 2 + Fraction(float(t)))


def _boundary_points(c, target, rng, want):
    """`want` points whose squared distance to c, as the kernels compute it, is exactly `target`."""
    r = float(np.sqrt(np.float64(target)))
    out = []
    for _ in range(64):
        u = rng.randn(3)
        u /= np.linalg.norm(u)
        u = np.where(np.abs(u) < 0.2, 0.2 * np.sign(u + 1e-30), u)
        u /= np.linalg.norm(u)
        base = (c.astype(np.float64) + u * r).astype(np.float32)

        def steps(v, n):
            a = np.full(2 * n + 1, v, np.float32)
            a = (a.view(np.int32) + np.arange(-n, n + 1, dtype=np.int32)).view(np.float32)
            return a
        px, py, pz = steps(base[0], 24), steps(base[1], 24), steps(base[2], 96)
        dx, dy, dz = (px - c[0]).astype(np.float64), (py - c[1]).astype(np.float64), (pz - c[2]).astype(np.float64)
        t = (dx * dx).astype(np.float32).astype(np.float64)
        t = (dy[None, :] ** 2 + t[:, None]).astype(np.float32).astype(np.float64)             # [x, y]
        d2 = (dz[None, None, :] ** 2 + t[:, :, None]).astype(np.float32)                     # (search only: verified below)
        for i, j, k in np.argwhere(d2 == target)[:16]:
            p = np.array([px[i], py[j], pz[k]], np.float32)
            if _d2(p, c) == target:
                out.append(p)
        if len(out) >= want:
            return np.stack(out[:want])
    raise AssertionError('no points at the wanted squared distance found')


@pytest.fixture(scope='module')
def scene(ops):
    from occnerf_amd import seeded, synth
    from occnerf_amd.modules import hann_window_weights
    net = seeded.build_network(seed=0, S=128, non_rigid=True, device=DEV)
    data = seeded.frame_to_device(synth.make_frame(img_size=32, pose72=synth.seeded_pose(1), orbit_frame=28), DEV)
    cfg, ctx = net.cfg, net._context()
    nr = cfg.non_rigid_motion_mlp
    hann = hann_window_weights(nr.multires, 1e7, nr.kick_in_iter, nr.full_band_iter).tolist()
    cond = data['dst_posevec'].float().reshape(-1).contiguous()
    wc = net._weight_constants()
    pack = net._point_pack(wc)
    center, idx, agg, _ = net._knn_center(cond, hann, wc['table'], pack)
    c = center[:3].cpu().numpy()
    r2 = np.float32(center[3].item())
    assert (c != 0).all() and r2 > 0, 'pose 1 of the random-init checkpoint has a centre radius (profiles/r05_collapse_fraction.md)'
    r = float(np.sqrt(np.float64(r2)))

    # samples of the frame's busiest ray, offset like the renderer's: body-surface points and collapsed ones
    Rs, Ts, vol = net.render_preamble(data)
    rays = data['rays'].float().reshape(2, -1, 3).contiguous()
    rays8 = ops.pack_rays(rays, data['near'].float().reshape(-1), data['far'].float().reshape(-1), None)
    S = 128
    _, xyz_f, mask_f, _ = ops.sample_warp(rays8, S, torch.linspace(0., 1., steps=S, device=DEV), Rs, Ts, vol,
                                          net._host3(data['cnl_bbox_min_xyz']), net._host3(data['cnl_bbox_scale_xyz']))
    lrows, lcount = ops.live_rows(mask_f)
    pk = net._packed_weights()
    ops.nonrigid_rows(xyz_f, lrows, lcount, cond, hann, pk.nr_w0, pk.nr_b0, pk.nr)
    live = (mask_f.view(-1, S) != 0)
    ray = int(live.sum(1).argmax())
    body = xyz_f.view(-1, S, 3)[ray][live[ray]].cpu().numpy()
    assert len(body) >= 8

    rng = np.random.RandomState(5)

    def ulps(n):
        k = rng.randint(1, 4, (n, 3)) * rng.choice([-1, 1], (n, 3))
        return (np.tile(c, (n, 1)).view(np.int32) + k.astype(np.int32)).view(np.float32)

    def far(n):
        u = rng.randn(n, 3)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        return (c[None].astype(np.float64) + 2.0 * r * u).astype(np.float32)
    b_in = _boundary_points(c, np.nextafter(r2, np.float32(0)), rng, 32)
    b_out = _boundary_points(c, r2, rng, 32)
    pools = [np.tile(c, (1, 1)), ulps(256), b_in, b_out, far(256), body]
    pick = lambda pool, n: pool[rng.randint(0, len(pool), n)]              # noqa: E731
    parts = [np.tile(c, (N_COPIES, 1)),                                     # all-inside trips, the centre itself
             ulps(512)]                                                     # all-inside trips, 1..3 ulp off per coordinate
    mixed = np.empty((512, 3), np.float32)                                  # mixed trips: every kind side by side
    for s in range(8):
        mixed[s::8] = pick(pools[(s * 5) % 6], 64)
    parts += [mixed, far(256),                                              # all-outside trips
              pick(b_in, 128), pick(b_out, 128),                            # the last value inside, the first outside
              pick(body, 256)]
    n_rest = N_LIST - sum(len(p) for p in parts)
    kinds = rng.randint(0, 6, n_rest)
    parts.append(np.stack([pick(pools[k], 1)[0] for k in kinds]))           # ragged tail: kinds at random
    pts = np.concatenate(parts).astype(np.float32)
    assert pts.shape == (N_LIST, 3)

    # the list: N_LIST ascending positions of an xyz array of N_XYZ, in a rows tensor with spare capacity
    pos = np.sort(rng.choice(N_XYZ, N_LIST, replace=False)).astype(np.int32)
    xyz = far(N_XYZ)
    xyz[pos] = pts
    rows_np = np.zeros(N_XYZ, np.int32)
    rows_np[:N_LIST] = pos
    xyz_d, rows, count = T(xyz), T(rows_np), T(np.array([N_LIST], np.int32))

    # the parent's chain on the same list: kNN with the centre cache, feature kernel with the centre aggregate
    enc = net.cnl_mlp.module.encoder
    knn = ops.msknn_clustered(xyz_d, N_XYZ // 128, 128, ctx['clusters'], ctx['seed'], center=(center, idx))
    mlp_in, raw, enc_in = ops.sample_features(
        xyz_d, knn, net.point_base.detach(), ctx['normals'], ctx['unit'], net.point_counter.detach(), wc['table'],
        ctx['bound32'], ctx['two_bound32'], enc.embeddings.detach(), enc.offsets, enc.log2_per_level_scale,
        enc.base_resolution, rows=rows, count=count, pack=pack, center=center, center_agg=agg, want_enc_in=True)
    inside = np.array([_d2(p, c) < r2 for p in pts])
    assert (knn.cpu().numpy()[pos][inside] == idx.cpu().numpy()[None]).all(), 'inside samples carry the centre\'s lists'

    # the stage under test
    raw_c = torch.full((N_XYZ, 5), float('nan'), device=DEV)
    flag = ops.center_classify(xyz_d, rows, count, pack[0], center, idx, agg, ctx['bound32'], ctx['two_bound32'], raw_c)
    torch.cuda.synchronize()
    return {'pts': pts, 'inside': inside, 'agg': agg.cpu().numpy(), 'mlp_in': mlp_in[:N_LIST].cpu().numpy(),
            'raw': raw[:N_LIST].cpu().numpy(), 'enc_in': enc_in[:N_LIST].cpu().numpy(), 'flag': flag, 'raw_c': raw_c,
            'rows': rows, 'count': count, 'rows_np': rows_np}


def test_flagged_samples_have_the_centre_row(scene):
    """(a) flagged => inside; (b) the feature kernel's row of a flagged sample is the centre row, as int32; (c) its distance is
    the feature kernel's, as int32; (d) every inside sample with the centre's encoder input is flagged; (e) the copies of the
    centre are all flagged."""
    s = scene
    flag = s['flag'][:N_LIST].cpu().numpy()
    assert set(np.unique(flag)) <= {0, 1}
    f = flag == 1
    inside, agg = s['inside'], s['agg']
    print(f'\n   {int(f.sum())} of {N_LIST} flagged; {int(inside.sum())} inside the radius')
    assert not (f & ~inside).any(), '(a) a flagged sample lies outside the radius'
    centre_row = np.concatenate([agg[:36], agg[40:72]]).view(np.int32)
    rows_f = s['mlp_in'][f].view(np.int32)
    bad = (rows_f != centre_row[None]).any(1)
    assert not bad.any(), f'(b) {int(bad.sum())} flagged samples whose feature row is not the centre row'
    dist = s['raw_c'][:N_LIST, 4].cpu().numpy()
    assert np.array_equal(dist[f].view(np.int32), s['raw'][f, 4].view(np.int32)), '(c) signed distance'
    assert np.isnan(dist[~f]).all() and np.isnan(s['raw_c'][:, :4].cpu().numpy()).all(), 'nothing else of raw_c is written'
    assert np.isnan(s['raw_c'][N_LIST:].cpu().numpy()).all()
    same_x = (s['enc_in'].view(np.int32) == agg[36:40].view(np.int32)[None]).all(1)
    assert np.array_equal(f, inside & same_x), '(d) flagged == inside and the centre\'s encoder input'
    assert f[:N_COPIES].all(), '(e) the copies of the centre'
    # the list holds what it claims: trips of 8 that are all inside, all outside and mixed, and both sides of the radius
    trips = inside[:N_LIST // 8 * 8].reshape(-1, 8).sum(1)
    assert (trips == 8).sum() >= 128 and (trips == 0).sum() >= 32 and ((trips > 0) & (trips < 8)).sum() >= 64
    assert inside[2304:2432].all() and not inside[2432:2560].any()
    assert 0 < int((inside & ~same_x).sum()), 'some inside samples differ from the centre in the last bits of x'


def _split_reference(flag, rows, n, centre_row):
    keep = np.nonzero(flag[:n] == 0)[0].astype(np.int32)
    in_rows = np.full(n, centre_row, np.int32)
    in_rows[keep] = np.arange(len(keep), dtype=np.int32)
    return keep, rows[keep], in_rows


@pytest.mark.parametrize('case', ['classified', 'count0', 'all', 'none'])
def test_split_against_numpy(ops, scene, case):
    s = scene
    rows, M = s['rows'], s['rows'].shape[0]
    flag, count = s['flag'], s['count']
    if case == 'count0':
        count = torch.zeros(1, device=DEV, dtype=torch.int32)
    elif case == 'all':
        flag = torch.ones(M, device=DEV, dtype=torch.uint8)
    elif case == 'none':
        flag = torch.zeros(M, device=DEV, dtype=torch.uint8)
    n = int(count)
    keep, rows2, count2, in_rows, taken = ops.center_split(flag, rows, count, M)
    wk, wr, wi = _split_reference(flag.cpu().numpy(), s['rows_np'], n, M)
    n2 = int(count2)
    assert n2 == len(wk) and int(taken) == n - n2
    assert np.array_equal(keep[:n2].cpu().numpy(), wk) and np.array_equal(rows2[:n2].cpu().numpy(), wr)
    assert np.array_equal(in_rows[:n].cpu().numpy(), wi)
    if case == 'classified':
        assert 0 < n2 < n and (np.diff(wr) > 0).all()
        # the kept entries' distance back at their list positions
        raw2 = torch.arange(M * 5, device=DEV, dtype=torch.float32).reshape(M, 5)
        raw_c = torch.full((M, 5), -1.0, device=DEV)
        ops.center_merge_dist(raw2, keep, count2, raw_c)
        want = np.full((M, 5), -1.0, np.float32)
        want[wk, 4] = np.arange(M * 5, dtype=np.float32).reshape(M, 5)[:n2, 4]
        assert np.array_equal(raw_c.cpu().numpy(), want)
