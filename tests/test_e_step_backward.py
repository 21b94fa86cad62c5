"""GPU: warp_backward_kernel and composite_backward_kernel (occnerf_amd/csrc/train_ops.hip) through their autograd Functions,
PER ENTRY against the float64 restatements of tests/step_backward_restatement.py with the bounds derived there -- no tolerance
relative to the largest entry, under which a tap lost at a volume face or at the z = 15 | 16 seam, a sample lost at a slice
boundary, a transposed gradient of a bone few samples reach, or anything at all far down a nearly opaque ray would pass.

    warp        volume: gamma_W A + n 2^-53 A per voxel, one-term voxels bit-equal, voxels without terms and channels >= nb
                exactly zero;  Rs / Ts: gamma_{ceil(per / 256) + 7 + W} A per entry.  The restatement is fed the z the kernel
                returned (asserted bit-equal to the C oracle's sampler).
    composite   (err - floor) / (u E) <= 4 max(rho_ref, 1) per kind of ray, rho_ref from the fp32 CPU autograd; B = 0 entries and
                d_raw[..., 4] exactly zero.

Each test prints its worst error / bound (composite: rho_ref / the kernel's ratio per kind of ray); the values seen on an MI355X
stand in the docstrings."""
import numpy as np
import pytest
import torch

from tests import step_backward_cases as cases
from tests import step_backward_restatement as sbr
from tests.gpu_util import T, same

pytestmark = pytest.mark.gpu


# ---- warp ---------------------------------------------------------------------------------------------------------------
def _run_warp(c):
    """-> (z, d_vol, d_Rs, d_Ts) as numpy, through train_ops.sample_warp(...).backward."""
    from occnerf_amd import train_ops as to
    Rg, Tg, Vg = (T(c[k]).requires_grad_(True) for k in ('Rs', 'Ts', 'vol'))
    t_rand = None if c['t_rand'] is None else T(c['t_rand'])
    z, xs, mk = to.sample_warp(T(c['rays8']), c['S'], T(c['t_vals']), t_rand, Rg, Tg, Vg, c['bmin'], c['bscale'])
    mk.backward(T(c['g_mask']))
    torch.cuda.synchronize()
    return z.cpu().numpy(), Vg.grad.cpu().numpy(), Rg.grad.cpu().numpy(), Tg.grad.cpu().numpy()


def _check_warp(name, oracle):
    from occnerf_amd import _lib
    c = cases.WARP_CASES[name]()
    total = len(c['g_mask'])
    W = int(_lib.lib().occnerf_warp_backward_slices(total))
    assert W == sbr.slices_and_per(total)[0] and ((W == 16) if name == 'capped' else (W < 16)), W
    z, d_vol, d_Rs, d_Ts = _run_warp(c)
    same(z, oracle.sample_rays(c['rays8'], c['t_vals'], c['t_rand'])[0], f'{name}: z')
    ref = sbr.warp_backward_numpy(c['rays8'], z, c['g_mask'], c['Rs'], c['Ts'], c['vol'], c['bmin'], c['bscale'])
    cases.assert_warp_populations(c, ref)
    assert d_vol.shape == c['vol'].shape and d_Rs.shape == c['Rs'].shape and d_Ts.shape == c['Ts'].shape
    return sbr.check_warp(name, d_vol, d_Rs, d_Ts, ref, total, c['S'])


def test_warp_backward_dyadic(oracle):
    """Exact grid coordinates, taps on every face, on the seam and exactly on gi = 0 / 31, floor = 32; 2 slices whose boundary
    falls inside a ray.  MI355X: volume 0.868, Rs/Ts 0.003 of the bound."""
    _check_warp('dyadic', oracle)


def test_warp_backward_random(oracle):
    """General rotations, jitter, 10 % exact zeros in the upstream gradient, bone 17 out of reach (all of its gradient exactly
    zero).  MI355X: volume 0.930, Rs/Ts 0.003 of the bound."""
    _check_warp('random', oracle)


def test_warp_backward_capped(oracle):
    """The production launch shape: 16 slices (the cap) of 16 424 samples, every boundary inside a ray, a ragged last trip of the
    thread loop; nb = 2.  MI355X: volume 0.125, Rs/Ts below 0.001 of the bound
    (the Rs/Ts count is a worst case that grows with the 65 serial additions of a thread; 132 591 terms per entry)."""
    _check_warp('capped', oracle)


@pytest.mark.parametrize('nb', [1, 32])
def test_warp_backward_bone_counts(oracle, nb):
    """nb = 1 and nb = 32 with a volume of exactly nb channels (no background channel behind the last bone).
    MI355X: nb = 1 volume 0.980, Rs/Ts 0.006; nb = 32 volume 1.000 (one slice: a two-term voxel can use all of
    gamma_1 A), Rs/Ts 0.008 of the bound."""
    _check_warp(f'bones{nb}', oracle)


def test_warp_backward_sparse(oracle):
    """200 samples: 17 000+ voxels of exactly one term (bit-equal to fl(g w)), 97 % of the volume exactly zero.
    MI355X: volume 0.953, Rs/Ts 0.073 of the bound."""
    _check_warp('sparse', oracle)


def test_warp_backward_refuses_another_volume_size():
    """A 16^3 volume goes through the forward; its backward raises by name, on the host, before any launch."""
    from occnerf_amd import train_ops as to
    c = cases.warp_sparse()
    vol = T(np.ascontiguousarray(c['vol'][:, ::2, ::2, ::2])).requires_grad_(True)
    z, xs, mk = to.sample_warp(T(c['rays8']), c['S'], T(c['t_vals']), None, T(c['Rs']), T(c['Ts']), vol, c['bmin'], c['bscale'])
    assert mk.shape == (len(c['g_mask']),) and bool(torch.isfinite(mk).all())
    with pytest.raises(RuntimeError, match=r'warp_backward.*32\^3'):
        mk.backward(T(c['g_mask']))


# ---- compositing --------------------------------------------------------------------------------------------------------
def _run_composite(c):
    from occnerf_amd import train_ops as to
    n, S = c['z'].shape
    raw, mask = T(c['raw']).requires_grad_(True), T(c['mask']).requires_grad_(True)
    rgb, acc, depth, term = to.composite(raw, mask, T(c['z']), T(c['rays8']), c['bg'])
    torch.autograd.backward([rgb, acc, depth], [T(c['g_rgb']), T(c['g_acc']), T(c['g_depth'])])
    torch.cuda.synchronize()
    d_raw, d_mask = raw.grad.cpu().numpy().reshape(n, S, 5), mask.grad.cpu().numpy().reshape(n, S)
    assert not d_raw[..., 4].any(), 'd_raw[..., 4] is exactly zero'
    return d_raw, d_mask


@pytest.mark.parametrize('bg', [0, 1])
@pytest.mark.parametrize('S', cases.COMPOSITE_S)
def test_composite_backward_per_entry(S, bg):
    """41 rays: x = 25 / 20 / 20 + ulp / -30, mask 0, alpha = 1 exactly (tt = 1e-10, the divisor of R / tt), alpha > 1 (tt < 0),
    equal consecutive z, direction norms 1e-3 and 1e3, zero upstream gradients (exact zeros out), 29 random rays; both
    backgrounds; S on both sides of every 64-sample chunk boundary, and S = 1.
    MI355X, rho_ref / kernel on the random rows at S = 1, 2, 63, 64, 65, 128, 129, 192, 256: 0.74/0.72, 1.3/1.3, 0.82/0.81,
    0.89/0.89, 0.91/0.91, 0.97/0.97, 0.93/0.92, 0.79/0.78, 1.1/1.1; every special kind below 1 on both sides except the
    alpha > 1 ray at S = 2 (0.73/2.2 against a tolerance of 4 x 1.3)."""
    c = cases.composite_case(S, cases.BACKGROUNDS[bg])
    d_raw, d_mask = _run_composite(c)
    sbr.check_composite(f'S={S} bg={bg}', c, d_raw, d_mask)


def test_composite_backward_one_ray():
    """n = 1: one block, three idle waves.  MI355X: rho_ref 0.49, kernel 0.49."""
    c = cases.composite_plain(1, 64, 1)
    sbr.check_composite('n=1', c, *_run_composite(c))


def test_composite_backward_grid_stride():
    """n = 32 768 + 5 rays of 2 samples: the launch caps at 8 192 blocks of 4 waves, so rays 32 768.. are the second trip of the
    grid-stride loop.  MI355X: rho_ref / kernel 1.4/2.9 on the first
    trip, 0.53/0.59 on the second."""
    c = cases.composite_plain(32768 + 5, 2, 2)
    d_raw, d_mask = _run_composite(c)
    c['groups'] = {'random': np.arange(32768), 'second trip': np.arange(32768, 32768 + 5)}
    sbr.check_composite('n=32773 S=2', c, d_raw, d_mask)


def test_composite_backward_refuses_more_than_256_samples():
    """S = 257 goes through the forward (any S); the backward keeps a ray in 4 chunks of registers and raises by name."""
    c = cases.composite_plain(3, 257, 3)
    with pytest.raises(RuntimeError, match=r'composite_backward: S=257'):
        _run_composite(c)
