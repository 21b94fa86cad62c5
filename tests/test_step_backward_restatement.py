"""CPU: keeps tests/step_backward_restatement.py honest without a GPU -- the references tests/test_e_step_backward.py holds
warp_backward_kernel and composite_backward_kernel to, each against a second, independent opinion:

    warp, `dyadic`   torch's float64 autograd over train_path.warp_to_canonical (F.grid_sample): the positions are exact in both
                     formats there, so the restatement's unrounded mode equals autograd up to float64 summation, and its fp32
                     mode -- the kernel's terms -- lies within the taps' three fp32 roundings of it;
    warp, `random`   the adjoint identity <g, mask(dv)> = <d_vol, dv> against the C oracle's FORWARD (bit-exact with the HIP
                     forward), for volumes dv on a face shell, on the z = 15 | 16 planes and on an interior block;
    compositing      the condition weight B bounds the true gradient entry by entry, the error weight E bounds B, and the fp32
                     reference's ratio is finite on every case and flat over the sample counts (so the tolerance
                     4 max(rho_ref, 1) is a small count of roundings, never vacuous)."""
import numpy as np
import pytest
import torch

from tests import step_backward_cases as cases
from tests import step_backward_restatement as sbr

F32 = np.float32
_memo = {}


def _warp(name, oracle):
    """(case, z of the oracle's sampler, pts, restatement), computed once."""
    if name not in _memo:
        c = cases.WARP_CASES[name]()
        z, pts = oracle.sample_rays(c['rays8'], c['t_vals'], c['t_rand'])
        ref = sbr.warp_backward_numpy(c['rays8'], z, c['g_mask'], c['Rs'], c['Ts'], c['vol'], c['bmin'], c['bscale'])
        _memo[name] = (c, z, pts, ref)
    return _memo[name]


@pytest.mark.parametrize('name', list(cases.WARP_CASES))
def test_warp_cases_reach_their_paths(oracle, name):
    """Volume faces, the z = 15 | 16 seam, samples exactly on gi = 0 / 31, floor = 32, the slice cap, slice boundaries inside
    a ray, single-term voxels: each case still holds the population it was built for."""
    c, z, pts, ref = _warp(name, oracle)
    pop = cases.assert_warp_populations(c, ref)
    assert pop['slices'] == sbr.slices_and_per(len(c['g_mask']))[0] and pop['per'] == sbr.slices_and_per(len(c['g_mask']))[1]
    assert int(ref['vol_n'].sum()) > 0 and not ref['vol_n'][c['Rs'].shape[0]:].any()
    # p = fl(o + fl(d z)) is the sampler's own point, bit for bit
    p = (c['rays8'][:, None, 0:3] + (c['rays8'][:, None, 3:6] * z[..., None]).astype(F32)).astype(F32)
    assert np.array_equal(p, pts.reshape(p.shape))


def test_warp_restatement_equals_float64_autograd_on_dyadic(oracle):
    """Exact positions: fp32 and float64 grid coordinates are the same numbers (np.array_equal), so both scatter to the same
    voxels.  Unrounded mode vs autograd: 1e-12 of the entry's absolute sum (float64 summation only), for the volume and for
    Rs / Ts -- a transposed R, a wrong tap at a face or a wrong sign in dix shows here.  fp32 mode (the kernel's terms) vs
    autograd: gamma_3 A per voxel, the roundings of (w_x w_y) w_z and of the product with g."""
    from occnerf_amd.train_path import warp_to_canonical
    c, z, pts, ref = _warp('dyadic', oracle)
    ex = sbr.warp_backward_numpy(c['rays8'], z, c['g_mask'], c['Rs'], c['Ts'], c['vol'], c['bmin'], c['bscale'], exact=True)
    assert np.array_equal(ex['gi'], ref['gi'].astype(np.float64)) and np.array_equal(ex['counted'], ref['counted'])
    assert np.array_equal(ex['vol_n'], ref['vol_n'])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()                                    # noqa: E731
    R64, T64, V64 = (t(c[k]).requires_grad_(True) for k in ('Rs', 'Ts', 'vol'))
    _, mk = warp_to_canonical(t(pts).reshape(z.shape + (3,)), R64, T64, V64, t(c['bmin']), t(c['bscale']))
    (mk.reshape(-1) * t(c['g_mask'])).sum().backward()
    dv, drt = V64.grad.numpy(), np.concatenate([R64.grad.numpy().reshape(-1, 9), T64.grad.numpy()], 1)
    assert (np.abs(dv - ex['vol_ssum']) <= 1e-12 * ex['vol_A']).all()
    assert (np.abs(drt - ex['rt_ssum']) <= 1e-12 * ex['rt_A']).all()
    assert (ex['rt_A'] > 0).all() and (np.abs(drt) > 1e-3 * ex['rt_A']).mean() > 0.9          # (the comparison is not vacuous)
    assert (np.abs(dv - ref['vol_ssum']) <= (sbr.gamma(3) + 1e-12) * ref['vol_A']).all()
    # Rs / Ts in fp32 mode: dix is a sum of +-v taps that cancel, so its roundings are bounded by the taps' absolute values
    # (the unrounded mode's A): 2 roundings per tap product, 7 additions, 3 products for dp, 1 for dp p
    assert (np.abs(drt - ref['rt_ssum']) <= (sbr.gamma(13) + 1e-12) * ex['rt_A']).all()


def test_warp_restatement_is_the_adjoint_of_the_oracle_forward(oracle):
    """mask is linear in the volume: <g, mask(dv)> = <d_vol, dv>.  The oracle's forward adds v fl(fl(w_x w_y) w_z) over 8 taps
    and nb bones serially in fp32 (at most 8 nb roundings per term; the restatement's own fl(g w) is one of them on the other
    side): |difference| <= gamma_{8 nb} sum |g| |dv| w, the restatement's A weighted by |dv|."""
    c, z, pts, ref = _warp('random', oracle)
    nb = c['Rs'].shape[0]
    rng = np.random.RandomState(3)
    ax = np.arange(cases.G)
    zz, yy, xx = np.meshgrid(ax, ax, ax, indexing='ij')
    face = lambda a: (a == 0) | (a == cases.G - 1)                                                     # noqa: E731
    supports = {'face shell': face(zz) | face(yy) | face(xx), 'seam planes': (zz == 15) | (zz == 16),
                'interior block': (zz >= 8) & (zz < 14) & (yy >= 10) & (yy < 20) & (xx >= 5) & (xx < 9),
                'everything': np.ones_like(zz, bool)}
    g = c['g_mask'].astype(np.float64)
    for name, sup in supports.items():
        dv = (rng.uniform(-1, 1, c['vol'].shape) * sup[None]).astype(F32)
        _, mk = oracle.motion_field(pts, c['Rs'], c['Ts'], dv, c['bmin'], c['bscale'])
        lhs = float((g * mk.astype(np.float64)).sum())
        rhs = float((ref['vol_ssum'] * dv.astype(np.float64)).sum())
        bound = float(sbr.gamma(8 * nb) * (ref['vol_A'] * np.abs(dv)).sum())
        print(f'   {name}: <g, mask(dv)> = {lhs:.9g}, <d_vol, dv> = {rhs:.9g}, difference / bound {abs(lhs - rhs) / bound:.3f}')
        assert bound > 0 and abs(lhs - rhs) <= bound, name


def _composite_cases():
    for S in cases.COMPOSITE_S:
        for bg in cases.BACKGROUNDS:
            yield f'S={S} bg={int(bg[0])}', cases.composite_case(S, bg)
    yield 'n=1', cases.composite_plain(1, 64, 1)
    yield 'n=32773 S=2', cases.composite_plain(32768 + 5, 2, 2)


def test_composite_condition_weight_bounds_the_gradient():
    """B >= |float64 gradient| entry by entry (a bound, not an estimate; 1e-12 for the float64 evaluation of both sides), the
    fifth raw channel and every entry with B = 0 exactly zero in the truth and in the fp32 reference, whose ratio is finite.
    Prints rho_ref per kind of ray."""
    for name, c in _composite_cases():
        ref = sbr.composite_backward_float64(c)
        assert np.isfinite(ref['d_raw']).all() and np.isfinite(ref['d_mask']).all(), name
        assert (np.abs(ref['d_raw']) <= ref['B_raw'] * (1 + 1e-12)).all(), name
        assert (np.abs(ref['d_mask']) <= ref['B_mask'] * (1 + 1e-12)).all(), name
        assert not ref['d_raw'][..., 4].any() and not ref['B_raw'][..., 4].any()
        r32 = sbr.composite_backward_ref32(c)
        seen = sbr.check_composite(name, c, r32[0], r32[1], ref, r32)          # the reference against itself: ratio = rho_ref
        assert all(np.isfinite(a) for a, _ in seen.values()), (name, seen)
        if 'zero gradient' in c['groups']:
            rows = c['groups']['zero gradient']
            assert not ref['B_raw'][rows].any() and not ref['B_mask'][rows].any() and not r32[0][rows].any()
            assert not ref['B_raw'][c['groups']['mask=0']][..., :4].any()
            S = c['z'].shape[1]
            mid = (S - 1) // 2                                  # the opaque sample: softplus * dist >= 200, em = 0 in both formats
            gap = 1e10 if mid == S - 1 else float(c['z'][5, mid + 1]) - float(c['z'][5, mid])
            assert float(c['raw'][5, mid, 3]) * gap >= 200.0 and float(c['mask'][5, mid]) == 1.0
        assert (ref['E_raw'] >= ref['B_raw']).all() and (ref['E_mask'] >= ref['B_mask']).all(), name


def test_composite_reference_ratio_over_S():
    """The fp32 reference's ratio on the random rows over the sample counts.  With the scale S u B it grows from 135 (S = 2)
    to 18 000 (S = 256) -- the measurement that made tests/step_backward_restatement.py replace that scale by the error weight
    E, under which it is flat: within 10 x between any two sample counts, and of order 1 (asserted: below 8, so that the
    tolerance 4 max(rho_ref, 1) stays a count of roundings)."""
    rho, old = {}, {}
    for S in cases.COMPOSITE_S:
        c = cases.composite_case(S)
        ref, r32 = sbr.composite_backward_float64(c), sbr.composite_backward_ref32(c)
        per_ray, _, _ = sbr.composite_ratio(r32[0], r32[1], ref, S)
        rows = c['groups']['random']
        rho[S] = float(per_ray[rows].max())
        err = np.abs(r32[0] - ref['d_raw'])[rows]
        old[S] = float(np.divide(err, S * sbr.U32 * ref['B_raw'][rows], out=np.zeros_like(err), where=ref['B_raw'][rows] > 0).max())
    print('   rho_ref of the random rows, scale u E:   ' + ', '.join(f'S={S}: {v:.3g}' for S, v in rho.items()))
    print('   the same with the scale S u B (d_raw):   ' + ', '.join(f'S={S}: {v:.3g}' for S, v in old.items()))
    assert max(rho.values()) <= 10 * min(rho.values()) and max(rho.values()) < 8
    assert old[256] > 10 * old[2]
