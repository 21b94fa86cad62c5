"""CPU: the restatements, weights and check functions of tests/step_preamble_restatement.py, before the GPU tests
(tests/test_q_step_preamble_per_entry.py) rely on them:

  * every committed case meets its condition (ReLU margins, inside tests away from rounding, the kinds of prior, ...);
  * the restated pose chain and its hand-derived backward against torch's float64 autograd of the modules; col2im against
    conv_transpose3d and im2col as its exact adjoint; the per-point SDF backward against float64 autograd of the torch path;
  * rho_ref of every measured check, printed, with its spread over the cases of one check at most 10 x;
  * an emulated fp32 kernel passes every check in two summation orders, and each planted defect fails the check meant for it
    (matched by that check's message)."""
import numpy as np
import pytest
import torch

from tests import step_preamble_cases as cases
from tests import step_preamble_restatement as sp

F32 = np.float32


def _close(name, got, want):
    """1e-12 relative per entry; an entry that cancels far below its tensor's typical size is held to that size instead (the rule
    of tests/test_trunks_restatement.py)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    tol = 1e-12 * np.maximum(np.abs(want), np.mean(np.abs(want)))
    bad = ~(np.abs(got - want) <= tol)
    assert not bad.any(), (name, int(bad.sum()), float(np.max(np.abs(got - want) / np.maximum(tol, 1e-300))))


@pytest.fixture(scope='module')
def pose():
    """Per regime: the case, torch's float64 truth, the weights and the fp32 reference, evaluated once."""
    out = {}
    for regime in cases.REGIMES:
        c = cases.pose_case(regime)
        args = (c, True, c['dRs'], c['dTs'])
        out[regime] = {'c': c, 'truth': sp.pose_truth(*args), 'E': sp.pose_weights(*args), 'ref32': sp.pose_ref32(*args)}
    return out


def _fwd(d):
    return {k: d[k] for k in ('Rs', 'Ts')}


# ---- the cases ------------------------------------------------------------------------------------------------------------
def test_every_case_meets_its_condition():
    for regime in cases.REGIMES:
        print(regime, 'smallest ReLU margin / ((K + 2) u A):', round(cases.assert_pose_case(cases.pose_case(regime)), 1))
    cases.pose_exact_case()
    for C in cases.PRIOR_C:
        for V in cases.PRIOR_V:
            cases.prior_case(C, V)
    for shape in cases.CONVT_SHAPES:
        cases.convt_case(shape)
    for K in cases.AGG_K:
        for N in cases.AGG_N:
            counter, knn = cases.agg_case(N, K)
            assert knn.min() >= 0 and knn.max() < cases.AGG_P and (knn[N - 1] == knn[N - 1, 0]).all()
            assert N < 2 or set(knn[N - 2]) == {0, cases.AGG_P - 1}
    for P in cases.SDF_P:
        c = cases.sdf_case(P)
        pc = (c['base'][:P].astype(F32) + c['point_dist'].astype(F32)).astype(F32)
        cases.assert_sdf_case(c, sp.knn3(pc, c['base']), sp.unit_normals(c['normals']))
    for n in cases.adam_sizes():
        c = cases.adam_case(n)
        assert c['g'][0] == 0 and c['v'][0] == 0 and np.abs(c['g']).max() <= 1e4
        if n > 5:
            assert np.abs(c['g'][c['g'] != 0]).min() <= 1e-11 and np.abs(c['g']).max() == 1e4
            assert np.all(np.sign(c['m'][2::5]) == -np.sign(c['g'][2::5]))


# ---- restatements against torch -------------------------------------------------------------------------------------------
def test_restated_pose_chain_and_backward_match_torch_autograd(pose):
    for regime, d in pose.items():
        c = d['c']
        mine = sp.pose_chain(c, 'f64', True, c['dRs'], c['dTs'])
        for (k, a), (_, b) in zip(sp.pose_outputs(_fwd(mine)) + sp.pose_outputs(mine), sp.pose_outputs(_fwd(d['truth'])) + sp.pose_outputs(d['truth'])):
            _close(f'{regime} {k}', np.asarray(a).reshape(b.shape), b)
    for c in (cases.pose_exact_case(), cases.pose_random_case()):
        mine, want = sp.pose_chain(c, 'f64', False), sp.pose_truth(c, False)
        _close(c['name'] + ' Rs', mine['Rs'], want['Rs'])
        _close(c['name'] + ' Ts', mine['Ts'], want['Ts'])


def test_exact_pose_case_is_exact_in_every_arithmetic():
    c = cases.pose_exact_case()
    want = sp.pose_exact_truth(c)                              # (torch's LU inverse is off by 6e-17 on 17 entries: _close above)
    for mode in ('f64', 'f32'):
        got = sp.pose_chain(c, mode, False)
        assert np.asarray(got['Rs']).dtype == (F32 if mode == 'f32' else np.float64)
        sp.check_equal(f'pose forward exact Rs ({mode})', got['Rs'], want['Rs'])
        sp.check_equal(f'pose forward exact Ts ({mode})', got['Ts'], want['Ts'])
    assert not sp.pose_weights(c, False)['Rs'][want['Rs'] == 0].any(), 'exact zeros carry no weight'


def test_col2im_is_conv_transpose3d_and_im2col_its_adjoint():
    for shape in cases.CONVT_SHAPES:
        Cout, D, H, W = shape
        rng = np.random.RandomState(sum(shape))
        Cin = 3
        x, wt, bias = rng.randn(Cin, D, H, W), rng.randn(Cin, Cout, 4, 4, 4), rng.randn(Cout)
        cols = wt.reshape(Cin, Cout * 64).T @ x.reshape(Cin, -1)
        want = torch.nn.functional.conv_transpose3d(torch.from_numpy(x)[None], torch.from_numpy(wt), torch.from_numpy(bias), stride=2, padding=1)[0]
        _close(f'col2im {shape}', sp.col2im(cols, bias, Cout, D, H, W, np.float64), want.numpy())
        want0 = torch.nn.functional.conv_transpose3d(torch.from_numpy(x)[None], torch.from_numpy(wt), None, stride=2, padding=1)[0]
        _close(f'col2im {shape} no bias', sp.col2im(cols, None, Cout, D, H, W, np.float64), want0.numpy())
        c = cases.convt_case(shape, dyadic=True)
        lhs = float((sp.col2im(c['cols'], None, Cout, D, H, W, np.float64) * c['gy']).sum())
        rhs = float((c['cols'] * sp.im2col(c['gy'], Cout, D, H, W)).sum())
        assert lhs == rhs, (shape, lhs, rhs)


def _sdf_torch64(pc, base, normals, kidx, d_kb, d_dist):
    """train_path.point_sdf_block's torch path (network.py:263-284) in float64 under autograd, neighbours given."""
    dist = torch.zeros(len(pc), 1, dtype=torch.float64, requires_grad=True)
    nbr = torch.from_numpy(np.asarray(base, np.float64))[torch.from_numpy(kidx).long()]
    dir32 = np.asarray(pc, F32)[:, None, :] - np.asarray(base, F32)[kidx]             # the fp32 difference both paths start from
    direction = torch.from_numpy(dir32.astype(np.float64)) + dist[:, None, :]
    norms = torch.from_numpy(np.asarray(normals, np.float64))[torch.from_numpy(kidx).long()]
    att = torch.abs(torch.nn.functional.cosine_similarity(direction, norms, dim=-1))[..., None]
    knn_base = (att * nbr).sum(1) / att.sum(1)
    inside = ((direction.float() * norms.float()).sum(-1) < 0).sum(1) > 1.5
    d = torch.norm(direction, dim=-1).mean(1, keepdim=True)
    d = torch.where(inside[:, None], -d, d)
    ((knn_base * torch.from_numpy(d_kb)).sum() + (d[:, 0] * torch.from_numpy(np.asarray(d_dist, np.float64))).sum()).backward()
    return dist.grad[:, 0].numpy()


def test_point_sdf_backward_restatement_matches_torch_autograd():
    for P in cases.SDF_P:
        c = cases.sdf_case(P)
        unit = sp.unit_normals(c['normals'])
        pc = (c['base'][:P].astype(F32) + c['point_dist'].astype(F32)).astype(F32)
        kidx = sp.knn3(pc, c['base'])
        for d_kb, d_dist in ((c['d_kb'], c['d_dist']), (c['d_kb'], 0 * c['d_dist']), (0 * c['d_kb'], c['d_dist'])):
            g, B = sp.point_sdf_backward_f64(pc, c['base'], c['normals'], unit, kidx, d_kb, d_dist)
            away = (pc[:, None, :] - c['base'].astype(F32)[kidx]).any(-1).all(1)        # rows without a dir = 0 neighbour
            want = _sdf_torch64(pc, c['base'], c['normals'], kidx, d_kb, d_dist)
            assert away.sum() >= min(P, 3 * P // 4) and np.all(B >= np.abs(g))
            assert np.all(np.abs(g[away] - want[away]) <= 1e-12 * B[away]), (P, float(np.max(np.abs(g[away] - want[away]) / B[away])))


# ---- rho_ref and the emulated kernels -------------------------------------------------------------------------------------
def _spread(name, rhos):
    rhos = [max(r, 1e-3) for r in rhos]
    print(f'   rho_ref {name}: ' + ', '.join(f'{r:.2f}' for r in rhos))
    assert max(rhos) <= 10.0 * min(rhos), (name, rhos)


def test_pose_rho_ref_is_flat_and_the_emulated_kernel_passes(pose):
    fw, bw = [], []
    for regime, d in pose.items():
        c = d['c']
        fw.append(max(float(sp.ratio(d['ref32'][k], d['truth'][k], d['E'][k]).max()) for k in ('Rs', 'Ts')))
        for order in (0, 1):
            emu = sp.pose_chain(c, 'f32', True, c['dRs'], c['dTs'], order=order)
            rho, _ = sp.check_pose(f'pose backward {regime} order {order}', emu, d['truth'], d['E'], d['ref32'])
            sp.check_pose(f'pose forward {regime} order {order}', _fwd(emu), _fwd(d['truth']), _fwd(d['E']), _fwd(d['ref32']))
        bw.append(rho)
    c = cases.pose_random_case()
    truth, E, ref32 = sp.pose_truth(c, False), sp.pose_weights(c, False), sp.pose_ref32(c, False)
    rho0, _ = sp.check_pose('pose forward refine = 0 random', sp.pose_chain(c, 'f32', False), truth, E, ref32)
    _spread('pose forward (refine = 0 random, then the regimes)', [rho0] + fw)
    _spread('pose backward (the regimes)', bw)


@pytest.mark.parametrize('defect', sp.DEFECTS)
def test_planted_pose_defect_fails_its_check(pose, defect):
    d = pose['default init']
    c = d['c']
    emu = sp.pose_chain(c, 'f32', True, c['dRs'], c['dTs'], defect=defect)
    if defect == 'parent13':                                   # the forward has the parent table too
        with pytest.raises(AssertionError, match='pose forward .* over c u E'):
            sp.check_pose('pose forward', _fwd(emu), _fwd(d['truth']), _fwd(d['E']), _fwd(d['ref32']))
    with pytest.raises(AssertionError, match='pose backward .* over c u E'):
        sp.check_pose('pose backward', emu, d['truth'], d['E'], d['ref32'])


def test_wrong_parent_fails_the_one_bone_structure(pose):
    """A cotangent on bone 23 alone: with bone 13 hung on 12 the path root -> 23 changes, and an entry off the true path is no
    longer an exact zero (or one on it is lost)."""
    d = pose['default init']
    c = d['c']
    dRs, dTs = cases.one_bone_cotangent(c, 16)                 # 16 hangs on 13: its path runs through the planted parent
    truth, E, ref32 = (f(c, True, dRs, dTs) for f in (sp.pose_truth, sp.pose_weights, sp.pose_ref32))
    on = sorted(sp.path_to_root(16))
    assert on == [3, 6, 9, 13, 16]
    off = np.array([b not in on for b in range(1, 24)]).repeat(3)
    assert not E['db'][4][off].any() and E['db'][4][~off].all(), 'E = 0 exactly off the path'
    good = sp.pose_chain(c, 'f32', True, dRs, dTs)
    sp.check_pose('pose backward one bone', good, truth, E, ref32)
    bad = sp.pose_chain(c, 'f32', True, dRs, dTs, defect='parent13')
    with pytest.raises(AssertionError, match='pose backward one bone db\\[4\\]'):
        sp.check_bounded('pose backward one bone db[4]', bad['db'][4], truth['db'][4], E['db'][4], 4.0)


def test_zero_and_root_cotangents_carry_no_weight(pose):
    c = pose['reference init']['c']
    for dRs, dTs in ((np.zeros((24, 3, 3)), np.zeros((24, 3))), cases.one_bone_cotangent(c, 0)):
        E = sp.pose_weights(c, True, dRs, dTs)
        emu = sp.pose_chain(c, 'f32', True, dRs, dTs)
        for (k, e), (_, g) in zip(sp.pose_outputs(E), sp.pose_outputs(emu)):
            assert not e.any() and not np.asarray(g).any(), k


def _softmax32(dec, prior, no_max=False):
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        x = dec.astype(F32) + np.log(prior.astype(F32))
        e = np.exp(x if no_max else x - x.max(0, keepdims=True))
        return e / e.sum(0, keepdims=True, dtype=F32)


def test_prior_softmax_rho_ref_emulation_and_defect():
    rhos = []
    for C in cases.PRIOR_C:
        for V in cases.PRIOR_V:
            dec, prior = cases.prior_case(C, V)
            rho, _ = sp.check_prior_softmax(f'prior_softmax C={C} V={V}', _softmax32(dec, prior), dec, prior)
            rhos.append(rho)
            if C > 1:
                with pytest.raises(AssertionError, match='prior_softmax'):
                    sp.check_prior_softmax(f'prior_softmax C={C} V={V}', _softmax32(dec, prior, no_max=True), dec, prior)
    for C, per_C in zip(cases.PRIOR_C, np.reshape(rhos, (len(cases.PRIOR_C), -1))):
        if C > 1:                                              # (C = 1 is exact; V = 1 is C entries, no population to measure on)
            _spread(f'prior_softmax C={C} over V >= 255', [r for r, V in zip(per_C, cases.PRIOR_V) if V >= 255])


def test_convt_defects_fail_bit_equality():
    for shape in cases.CONVT_SHAPES:
        Cout, D, H, W = shape
        c = cases.convt_case(shape)
        want = sp.col2im(c['cols'], c['bias'], Cout, D, H, W)
        assert want.dtype == F32
        with pytest.raises(AssertionError, match='col2im .* not bit-equal'):
            sp.check_equal(f'col2im {shape}', sp.col2im(c['cols'], c['bias'], Cout, D, H, W, defect='kd_parity'), want)
        swapped = sp.col2im(c['cols'], c['bias'], Cout, D, H, W, defect='swap_hw')
        if H != W and W > 1:                                   # (with W = 1 the two index maps coincide)
            with pytest.raises(AssertionError, match='col2im .* not bit-equal'):
                sp.check_equal(f'col2im {shape}', swapped, want)


def _agg32(counter, knn, reverse=False):
    """The kernel's tail in fp32 with numpy's expf, the sum in either order."""
    var, arg = sp.agg_weights_f32(counter, knn)
    e = np.exp(arg)
    s = np.zeros(len(e), F32)
    for j in (range(e.shape[1] - 1, -1, -1) if reverse else range(e.shape[1])):
        s = s + e[:, j]
    return e / s[:, None], var


def test_agg_weights_rho_ref_emulation_and_defect():
    rhos = []
    for K in cases.AGG_K:
        for N in cases.AGG_N:
            counter, knn = cases.agg_case(N, K)
            for reverse in (False, True):
                atts, var = _agg32(counter, knn, reverse)
                rho, _ = sp.check_agg_weights(f'agg_weights N={N} K={K}', atts, var, counter, knn)
            if N < 3:                                          # (only the special rows: variance 0 under any divisor, exact weights)
                continue
            rhos.append(rho)
            with pytest.raises(AssertionError, match='agg_weights .* var'):
                sp.check_agg_weights(f'agg_weights N={N} K={K}', atts, sp.agg_weights_f32(counter, knn, defect='div_K')[0], counter, knn)
    for K, per_K in zip(cases.AGG_K, np.reshape(rhos, (len(cases.AGG_K), -1))):
        _spread(f'agg_weights atts K={K} over N >= 255', list(per_K))


def test_point_sdf_backward_bound_and_zero_dir_defect():
    for P in cases.SDF_P[1:]:
        c = cases.sdf_case(P)
        unit = sp.unit_normals(c['normals'])
        pc = (c['base'][:P].astype(F32) + c['point_dist'].astype(F32)).astype(F32)
        kidx = sp.knn3(pc, c['base'])
        g, B = sp.point_sdf_backward_f64(pc, c['base'], c['normals'], unit, kidx, c['d_kb'], c['d_dist'])
        sp.check_point_sdf_backward(f'point_sdf_backward P={P}', g.astype(F32), g, B)
        leak, _ = sp.point_sdf_backward_f64(pc, c['base'], c['normals'], unit, kidx, c['d_kb'], c['d_dist'], zero_dir_leak=True)
        with pytest.raises(AssertionError, match='point_sdf_backward .* over their bound'):
            sp.check_point_sdf_backward(f'point_sdf_backward P={P}', leak.astype(F32), g, B)


def test_adam_counts_hold_for_the_fp32_restatement_and_swapped_corrections_fail():
    for n in cases.adam_sizes():
        c = cases.adam_case(n)
        k = sp.adam_constants(1e-3, 3)
        for coef in (1.0, float(F32(1e-3) / F32(12345.678)), float(F32(1.0) / F32(3.7))):
            ref = sp.adam_ref(c['p'], c['g'], c['m'], c['v'], coef, k)
            p, m, v = sp.adam1_f32(c['p'], c['g'], c['m'], c['v'], coef, k)
            sp.check_adam(f'adam n={n} coef={coef:.3g}', p, m, v, ref)
        p, m, v = sp.adam1_f32(c['p'], c['g'], c['m'], c['v'], 1.0, k, swap_bc=True)
        with pytest.raises(AssertionError, match='adam .* p: .* over their bound'):
            sp.check_adam(f'adam n={n}', p, m, v, sp.adam_ref(c['p'], c['g'], c['m'], c['v'], 1.0, k))
    assert sp.clip_coef32(F32(4.0), 1.0) == F32(1.0) / (F32(2.0) + F32(1e-6)) and sp.clip_coef32(F32(0.25), 1.0) == 1.0
    assert sp.clip_coef32(F32(4.0), None) == 1.0


def test_pack_rays_restatement():
    c = cases.pack_case(5)
    got = sp.pack_rays_ref(c['rays'], c['near'], c['far'], c['order'])
    for r in range(5):
        s = c['order'][r]
        assert list(got[r]) == list(c['rays'][0, s].astype(F32)) + list(c['rays'][1, s].astype(F32)) + [F32(c['near'][s, 0]), F32(c['far'][s, 0])]
