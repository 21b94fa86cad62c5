"""CPU: the numpy definition of the rig (tests/mesh_rig_restatement.py) selects, normalises and skins as
it says; the glTF writer (occnerf_amd/gltf.py) keeps the specification's rules and its files, evaluated by the independent
float64 evaluator of tests/gltf_restatement.py, give the definition's positions; and what surrounds the kernels works without a
GPU.

Measured here (seeded checkpoint, its 6 890 body points, frames 0, 3 and 17 of the synthetic movement sequence; DESIGN.md
section 7n repeats them):
  * the corrective returns to the target within 1.9e-9 m by component at worst (the correctives are at most 5 cm long and
    their float32 rounding is what is left); every vertex is inside its own bound, the smallest of which is 1.1e-9 m;
  * the bases of the seeded pose refiner are 7.0e-5 .. 7.7e-5 away from rotations (rotation_defect; the reference's Rodrigues
    formula divides by theta + 1e-5), and a quaternion can only hold a rotation: the file of 48 body points evaluates within
    5.14e-5 m of the definition's posed at worst (bound 1.01e-3 m), with correctives within 5.14e-5 m of the targets (bound
    1.03e-3 m), under a world node within 5.13e-5 m (bound 1.09e-3 m).  The bound takes the defects of the links and of
    R^-1 against R^T from the inputs; its slack is the constants of its derivation (5.6 for Shepperd's transfer of a defect, the
    reach and the span of the whole body for every vertex), not a fitted factor."""
import ctypes
import functools
import json
import os
import re

import numpy as np
import pytest

from tests import gltf_restatement as gr
from tests import mesh_pose_restatement as mp
from tests import mesh_rig_restatement as rig
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = (np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32))
INSIDE = np.array([[0.1, -0.2, 0.3], [-0.55, 0.4, 0.0], [0.0, 0.0, 0.0]], np.float32)


# ------------------------------------------------------------------ selection and weights
@pytest.mark.parametrize('K', [4, 8])
def test_selection_on_hand_made_volumes(K):
    # exactly K positive bones: all taken, the largest first
    vol, bmin, bsc = rig.ladder(K)
    j, w, n, kept = rig.skin(INSIDE, vol, bmin, bsc, K)
    assert j.dtype == np.uint8 and w.dtype == np.float32 and n.dtype == np.uint8 and kept.dtype == np.float32
    assert (n == K).all() and (j == np.arange(K)[::-1]).all() and (kept == 1.0).all()
    s = K * (K + 1) / 2
    assert np.array_equal(w, np.broadcast_to((np.arange(K, 0, -1) / s).astype(np.float32), w.shape))
    # K + 1 positive bones, the K-th and the (K + 1)-th tied (bones 0 and 1 hold the same value): the lower index is taken
    vol, bmin, bsc = rig.ladder(K + 1, tie=(0, 1))
    j, w, n, kept = rig.skin(INSIDE, vol, bmin, bsc, K)
    assert (n == K).all() and (j[:, :K - 1] == np.arange(K, 1, -1)).all() and (j[:, K - 1] == 0).all()
    total = 1.0 + 1.0 + sum(range(3, K + 2))
    assert np.array_equal(kept, np.full(3, np.float32((total - 1.0) / total)))
    # ... and a tie among the taken ones keeps the index order
    vol, bmin, bsc = rig.ladder(K + 1, tie=(K, K - 1))
    j, _, _, _ = rig.skin(INSIDE, vol, bmin, bsc, K)
    assert (j[:, 0] == K - 1).all() and (j[:, 1] == K).all()
    # more than K positive bones: the K largest
    vol, bmin, bsc = rig.ladder(K + 3)
    j, w, n, kept = rig.skin(INSIDE, vol, bmin, bsc, K)
    assert (n == K).all() and (j == np.arange(K + 2, 2, -1)).all()
    taken, total = sum(range(4, K + 4)), sum(range(1, K + 4))
    assert np.array_equal(kept, np.full(3, np.float32(taken / total)))
    # no positive bone, and a vertex outside the grid: bound to joint 0 with weight 1, kept 0
    for vol, x in ((np.zeros((3, 4, 4, 4), np.float32), INSIDE), (rig.ladder(3)[0], np.array([[5.0, 0.0, 0.0], [0.0, -7.0, 0.0]], np.float32))):
        j, w, n, kept = rig.skin(x, vol, *BOX, K)
        assert not n.any() and not j.any() and not kept.any() and (w[:, 0] == 1.0).all() and not w[:, 1:].any()
    # a negative channel is no influence
    vol = rig.ladder(3)[0]
    vol[1] = -2.0
    j, w, n, kept = rig.skin(INSIDE, vol, *BOX, K)
    assert (n == 2).all() and (j[:, :2] == [2, 0]).all() and not j[:, 2:].any() and not w[:, 2:].any()
    assert np.array_equal(kept, np.full(3, np.float32(4.0 / 2.0)))


@pytest.mark.parametrize('K', [4, 8])
def test_skin_of_the_pose_volumes(K):
    """one_bone, two_bones (G = 2 too: one cell, pure interpolation) and corner_bone, whose second bone runs into the padding."""
    for G in (2, 8):
        _, _, vol, bmin, bsc = mp.two_bones(G)
        x = mp.box_points(200, 2)
        j, w, n, kept = rig.skin(x, vol, bmin, bsc, K)
        c = mp.canonical_weights(x, vol, bmin, bsc)
        assert (n == 2).all() and (kept == 1.0).all()
        first = np.where(c[:, 1] > c[:, 0], 1, 0)
        assert np.array_equal(j[:, 0], first) and np.array_equal(j[:, 1], 1 - first) and not j[:, 2:].any()
        assert np.array_equal(w[:, 0], (c.max(1) / (c.max(1) + c.min(1))).astype(np.float32))
    _, _, vol, bmin, bsc = mp.one_bone(4)
    j, w, n, kept = rig.skin(mp.box_points(50, 1, -0.7, 0.7), vol, bmin, bsc, K)
    assert (n == 1).all() and not j.any() and (w[:, 0] == 1.0).all() and not w[:, 1:].any() and (kept == 1.0).all()
    _, _, vol, bmin, bsc = mp.corner_bone(6)
    x = np.concatenate([mp.box_points(200, 3, -1.6, 1.6), mp.box_points(200, 4, 0.5, 1.3)])
    j, w, n, kept = rig.skin(x, vol, bmin, bsc, K)
    assert set(n.tolist()) == {0, 1, 2} and ((n == 2) == (j[:, 1] == 1) | (j[:, 0] == 1)).all()


def _weight_sum_is_one(w, n):
    """Each quotient c_k / s is at most 1 and rounded once: the float64 sum of the float32 weights is within n * 2^-25 of 1."""
    got = w.astype(np.float64).sum(1)
    bound = np.maximum(n, 1).astype(np.float64) * 2.0 ** -25
    assert (np.abs(got - 1.0) <= bound).all(), float(np.abs(got - 1.0).max())
    assert ((w > 0).sum(1) == np.maximum(n, 1)).all() and (w >= 0).all()


@pytest.mark.parametrize('K', [4, 8])
def test_weights_sum_to_one(K):
    rng = np.random.RandomState(7)
    vol = rng.uniform(0.0, 1.0, (12, 5, 5, 5)).astype(np.float32)
    vol[rng.uniform(size=vol.shape) < 0.97] = 0.0
    j, w, n, kept = rig.skin(mp.box_points(500, 9, -1.2, 1.2), vol, *BOX, K)
    assert len(set(n.tolist())) > 3
    _weight_sum_is_one(w, n)
    order = np.take_along_axis(mp.canonical_weights(mp.box_points(500, 9, -1.2, 1.2), vol, *BOX), j.astype(np.int64), 1)
    for k in range(K - 1):
        live = n > k + 1
        assert (order[live, k] >= order[live, k + 1]).all()                 # selection order: descending
    assert ((kept >= 0) & (kept <= 1)).all() and (kept[n == 0] == 0).all()
    with pytest.raises(ValueError, match='K=5'):
        rig.skin(INSIDE, vol, *BOX, 5)


# ------------------------------------------------------------------ linear blend skinning
def test_lbs_with_one_bone():
    Rs, Ts, vol, bmin, bsc = mp.one_bone(4)
    x = mp.box_points(100, 1, -0.5, 0.5)
    j, w, n, kept = rig.skin(x, vol, bmin, bsc, 4)
    posed = rig.lbs(x, j, w, Rs[None], Ts[None])
    want = np.einsum('ij,ni->nj', Rs[0].astype(np.float64), x.astype(np.float64) - Ts[0].astype(np.float64))
    assert posed.shape == (1, 100, 3) and posed.dtype == np.float32
    assert (np.abs(posed[0].astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-15).all()
    # ... and it is the start point of pose_points, which one bone of weight 1 solves in no step: the same bits
    p, flag, iters, _ = mp.pose_points(x, Rs, Ts, vol, bmin, bsc)
    assert (iters == 0).all() and np.array_equal(posed[0].view(np.uint32), p.view(np.uint32))
    # the corrective of target = posed: what the rounding of posed to float32 left, carried back through M^-1 = R (rows of
    # absolute sum <= sqrt(3)) -- and exactly 0 where that rounding left nothing (z, which this bone does not turn)
    _, delta, dflag, p64, M = rig.lbs(x, j, w, Rs[None], Ts[None], posed, np.zeros((1, 100), np.uint8), parts=True)
    assert not dflag.any() and delta.dtype == np.float32 and dflag.dtype == np.uint8
    left = posed[0].astype(np.float64) - p64[0]
    assert (np.abs(delta[0]).max(1) <= 1.01 * np.sqrt(3.0) * np.abs(left).max(1)).all() and np.abs(left).max() <= 2.0 ** -25
    exact_z = left[:, 2] == 0.0
    assert exact_z.sum() > 10 and not delta[0][exact_z, 2].any()
    # a quarter turn and dyadic coordinates: R^T (x - T) is exact in float32, so target = posed gives a corrective of exactly 0
    Rq, Tq = np.array([[[0, -1, 0], [1, 0, 0], [0, 0, 1]]], np.float32), np.array([[0.25, -0.5, 0.125]], np.float32)
    xq = (np.round(x * 1024) / 1024).astype(np.float32)
    pq = rig.lbs(xq, j, w, Rq[None], Tq[None])
    assert np.array_equal(pq[0], np.stack([xq[:, 1] + 0.5, -(xq[:, 0] - 0.25), xq[:, 2] - 0.125], 1).astype(np.float32))
    _, delta_q, dflag_q = rig.lbs(xq, j, w, Rq[None], Tq[None], pq, np.zeros((1, 100), np.uint8))
    assert not dflag_q.any() and not delta_q.any()
    # a displaced target: the corrective brings the skinned vertex onto it; beyond max_delta, and a flagged target: flagged
    shift = np.array([0.01, -0.02, 0.03], np.float32)
    target = (posed + shift).astype(np.float32)
    tf = np.zeros((1, 100), np.uint8)
    tf[0, ::7] = 1
    _, delta, dflag = rig.lbs(x, j, w, Rs[None], Ts[None], target, tf, max_delta=0.05)
    assert np.array_equal(dflag, tf) and not delta[0, ::7].any()
    back = p64[0] + np.einsum('nij,nj->ni', M[0], delta[0].astype(np.float64))
    ok = dflag[0] == 0
    assert (np.abs(back - target[0])[ok] <= gr.corrective_bound(M[0], delta[0], target[0])[ok, None]).all()
    _, delta, dflag = rig.lbs(x, j, w, Rs[None], Ts[None], target, np.zeros_like(tf), max_delta=0.029)
    assert dflag.all() and not delta.any()                              # |d|_inf = 0.03 up to rounding
    _, delta, dflag = rig.lbs(x, j, w, Rs[None], Ts[None], target, np.zeros_like(tf), max_delta=0.031)
    assert not dflag.any()


def test_lbs_singular_blend_and_slots():
    """Two opposite half-weights of a rotation by pi: M = diag(0, 0, 1), determinant 0 -> flagged, d = 0.  A slot of weight 0
    adds nothing, whatever its joint; a joint index past nb adds nothing."""
    Rs = np.stack([np.eye(3), np.diag([-1.0, -1.0, 1.0])]).astype(np.float32)[None]
    Ts = np.zeros((1, 2, 3), np.float32)
    x = mp.box_points(10, 3)
    j = np.tile(np.array([0, 1, 0, 0], np.uint8), (10, 1))
    w = np.tile(np.array([0.5, 0.5, 0.0, 0.0], np.float32), (10, 1))
    posed, delta, dflag, p64, M = rig.lbs(x, j, w, Rs, Ts, x[None] + np.float32(0.01), np.zeros((1, 10), np.uint8), parts=True)
    assert np.array_equal(M[0], np.broadcast_to(np.diag([0.0, 0.0, 1.0]), (10, 3, 3))) and dflag.all() and not delta.any()
    assert not posed[0, :, :2].any() and np.array_equal(posed[0, :, 2], x[:, 2])
    j2 = j.copy()
    j2[:, 2:] = 1
    assert np.array_equal(rig.lbs(x, j2, w, Rs, Ts), posed)
    j2[:, 1] = 7
    assert np.array_equal(rig.lbs(x, j2, w, Rs, Ts)[0], (0.5 * x.astype(np.float64)).astype(np.float32))
    # F frames at once are F single calls
    Rs3, Ts3 = rig.random_bases(3, 2, 11)
    all3 = rig.lbs(x, j, w, Rs3, Ts3)
    for f in range(3):
        assert np.array_equal(all3[f], rig.lbs(x, j, w, Rs3[f:f + 1], Ts3[f:f + 1])[0])


# ------------------------------------------------------------------ the seeded body
@functools.lru_cache(maxsize=None)
def _body():
    """The seeded checkpoint's body points and, for the recorded frames, the CPU per-frame constants, the definition's skin (K 4
    and 8), Newton's positions and the definition's skinning with correctives -- computed once, never changed."""
    from oracle.chain import per_frame_cpu
    ctx = util.model_context(0, False)
    base = np.ascontiguousarray(ctx['point_base'])
    frames = [mp.synthetic_frame(i) for i in mp.FRAMES]
    per = [per_frame_cpu(ctx, fr) for fr in frames]
    Rs, Ts = np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
    vol = np.ascontiguousarray(per[0][2][:24])
    bmin, bsc = frames[0]['cnl_bbox_min_xyz'], frames[0]['cnl_bbox_scale_xyz']
    skins = {K: rig.skin(base, vol, bmin, bsc, K) for K in (4, 8)}
    newton = [mp.pose_points(base, Rs[f], Ts[f], vol, bmin, bsc) for f in range(len(frames))]
    target, tflag = np.stack([n[0] for n in newton]), np.stack([n[1] for n in newton])
    return {'base': base, 'frames': frames, 'Rs': Rs, 'Ts': Ts, 'vol': vol, 'box': (bmin, bsc), 'skins': skins, 'target': target,
            'tflag': tflag}


def test_the_volume_does_not_depend_on_the_frame():
    from oracle.chain import per_frame_cpu
    b = _body()
    ctx = util.model_context(0, False)
    assert np.array_equal(per_frame_cpu(ctx, b['frames'][2])[2][:24], b['vol'])


@pytest.mark.parametrize('K', [4, 8])
def test_the_corrective_returns_to_the_target(K):
    """With d32 = float32(d): p + M float64(d32) is the target within gltf_restatement.corrective_bound -- the float32 rounding of
    d carried through M, the float32 rounding of the target, and the float64 solve (the derivation is that function's
    docstring).  Measured: 1.9e-9 m at worst."""
    b = _body()
    j, w, n, kept = b['skins'][K]
    _weight_sum_is_one(w, n)
    posed, delta, dflag, p64, M = rig.lbs(b['base'], j, w, b['Rs'], b['Ts'], b['target'], b['tflag'], 0.05, parts=True)
    assert (b['tflag'] == 0).all() and (n > 0).all()
    worst = 0.0
    for f, idx in enumerate(mp.FRAMES):
        ok = dflag[f] == 0
        back = p64[f] + np.einsum('nij,nj->ni', M[f], delta[f].astype(np.float64))
        err = np.abs(back - b['target'][f].astype(np.float64)).max(1)
        bound = gr.corrective_bound(M[f], delta[f], b['target'][f])
        i = int(np.argmax(np.where(ok, err / bound, 0.0)))
        gap = np.linalg.norm(posed[f].astype(np.float64) - b['target'][f], axis=1)
        print(f'\n   K {K} frame {idx}: {int((~ok).sum())} flagged; max |p + M d32 - target| = {err[ok].max():.3e} m, nearest the bound '
              f'{err[i]:.3e} of {bound[i]:.3e}; LBS to Newton {gap.mean():.3e} mean, {np.percentile(gap, 99):.3e} p99, '
              f'{gap.max():.3e} max; largest |d| {np.abs(delta[f]).max():.3e}; kept min {kept.min():.4f}')
        assert ok.mean() > 0.5 and (err[ok] <= bound[ok]).all()
        worst = max(worst, float(err[ok].max()))
    assert worst > 0.0


# ------------------------------------------------------------------ the file
def _small_mesh(K, correct, world=False):
    """48 of the body points under 16 triangles, the definition's skin and skinning in the three recorded frames."""
    from occnerf_amd import mesh
    b = _body()
    pick = np.arange(0, 6890, 144)[:48]
    verts = b['base'][pick]
    faces = np.arange(48, dtype=np.int32).reshape(16, 3)
    colors = (np.arange(48 * 3) % 251).astype(np.uint8).reshape(48, 3)
    j, w = b['skins'][K][0][pick], b['skins'][K][1][pick]
    cnl = b['frames'][0]['cnl_gtfms']
    rot, tra, prev = [], [], None
    for f in range(3):
        r, t = mesh.local_keys(mesh.joint_transforms(b['Rs'][f], b['Ts'][f], cnl), prev)
        rot.append(r), tra.append(t)
        prev = r
    out = {'verts': verts, 'faces': faces, 'colors': colors, 'joints': j, 'weights': w, 'cnl': cnl,
           'animation': {'rotation': np.stack(rot), 'translation': np.stack(tra)}, 'Rs': b['Rs'], 'Ts': b['Ts']}
    target, tflag = b['target'][:, pick], b['tflag'][:, pick].copy()
    tflag[1, 5] = 1                                                    # one vertex Newton is said not to have solved
    out['posed'], out['delta'], out['dflag'], out['p64'], out['M'] = rig.lbs(verts, j, w, b['Rs'], b['Ts'], target, tflag, 0.05, parts=True)
    out['target'] = target
    if not correct:
        out['delta'] = None
    if world:
        from occnerf_amd import gltf
        Rh = [mp.two_bones()[0][1], mp.one_bone()[0][0], mp.corner_bone()[0][1]]
        q, prev = [], None
        for R in Rh:
            prev = gltf.quaternion(R.astype(np.float64), prev)
            q.append(prev)
        out['Rh'], out['Th'] = Rh, np.array([[0.5, 1.0, -2.0], [0.6, 1.0, -2.1], [0.7, 1.1, -2.2]], np.float32)
        out['world'] = {'rotation': np.stack(q), 'translation': out['Th'].astype(np.float64)}
    return out


def _write(path, m, fps=30.0, animated=True):
    from occnerf_amd import gltf, synth
    return gltf.write_glb(str(path), m['verts'], m['faces'], m['colors'], m['joints'], m['weights'], m['cnl'],
                          normals=synth.vertex_normals(m['verts'], m['faces']), animation=m['animation'] if animated else None,
                          world=m.get('world') if animated else None, correctives=m['delta'] if animated else None, fps=fps)


def _bounds(m, doc, buf, world=False):
    joints_at = m['cnl'][:, :3, 3].astype(np.float64)
    reach = np.linalg.norm(m['verts'][:, None].astype(np.float64) - joints_at[None], axis=2).max() + (0.05 if m['delta'] is not None else 0.0)
    span = np.abs(m['verts']).max() + np.abs(m['Ts']).max()
    t_max = max(np.abs(gr.accessor(doc, buf, s['output'])).max() for a in doc['animations'] for s in a['samplers']
                if doc['accessors'][s['output']]['type'] == 'VEC3')
    p_max = np.abs(m['posed']).max()
    extra = 0.0
    if world:
        extra, reach = gr.rotation_defect(np.stack(m['Rh'])), max(reach, p_max * np.sqrt(3.0))
        p_max = p_max * np.sqrt(3.0) + np.abs(m['Th']).max()
    return gr.chain_bound(m['Rs'], reach, span, float(t_max), float(p_max), gr.LONGEST_CHAIN + (1 if world else 0), extra)


@pytest.mark.parametrize('K', [4, 8])
def test_the_file_keeps_the_rules_and_evaluates_to_the_definition(tmp_path, K):
    from occnerf_amd import gltf
    m = _small_mesh(K, correct=False)
    size = _write(tmp_path / 'a.glb', m, fps=24.0)
    blob = (tmp_path / 'a.glb').read_bytes()
    _write(tmp_path / 'b.glb', m, fps=24.0)
    assert size == len(blob) and blob == (tmp_path / 'b.glb').read_bytes()                 # the same inputs, the same bytes
    doc, buf = gr.check_rules(blob)
    assert doc['asset'] == {'version': '2.0', 'generator': gltf.GENERATOR}
    text = blob[20:20 + int.from_bytes(blob[12:16], 'little')].decode('utf-8').rstrip(' ')
    assert text == json.dumps(doc, sort_keys=True, separators=(',', ':'))                   # sorted keys, nothing else in it
    att = doc['meshes'][0]['primitives'][0]['attributes']
    assert set(att) == {'POSITION', 'NORMAL', 'COLOR_0', 'JOINTS_0', 'WEIGHTS_0'} | ({'JOINTS_1', 'WEIGHTS_1'} if K == 8 else set())
    # the rest pose: the vertices, faces and colours as they went in ...
    assert gr.accessor(doc, buf, att['POSITION']).tobytes() == m['verts'].tobytes()
    assert np.array_equal(gr.accessor(doc, buf, doc['meshes'][0]['primitives'][0]['indices']).reshape(-1, 3), m['faces'])
    assert np.array_equal(gr.accessor(doc, buf, att['COLOR_0'])[:, :3], m['colors'])
    got_j = np.concatenate([gr.accessor(doc, buf, att[f'JOINTS_{s}']) for s in range(K // 4)], 1)
    got_w = np.concatenate([gr.accessor(doc, buf, att[f'WEIGHTS_{s}']) for s in range(K // 4)], 1)
    assert np.array_equal(got_j, m['joints']) and got_w.tobytes() == m['weights'].tobytes()
    # ... the skeleton: names, hierarchy, rest offsets, and inverse bind matrices that are exact (pure translations)
    skin = doc['skins'][0]
    names = [doc['nodes'][n]['name'] for n in skin['joints']]
    assert names == list(gltf.JOINT_NAMES) and names[0] == 'pelvis' and names[15] == 'head' and skin['skeleton'] == skin['joints'][0]
    from occnerf_amd.synth import SMPL_PARENT
    for b in range(1, 24):
        assert skin['joints'][b] in doc['nodes'][skin['joints'][SMPL_PARENT[b]]]['children']
    ibm = gr.accessor(doc, buf, skin['inverseBindMatrices']).reshape(24, 4, 4).transpose(0, 2, 1)
    want = np.tile(np.eye(4, dtype=np.float32), (24, 1, 1))
    want[:, :3, 3] = -m['cnl'][:, :3, 3]
    assert np.array_equal(ibm, want) and np.array_equal(m['cnl'][:, :3, :3], want[:, :3, :3])
    # ... and evaluated through the skin at rest every joint matrix is the identity EXACTLY, so the vertex is (sum of its
    # float32 weights) x itself: the vertex up to the n * 2^-25 the weights' sum may miss 1 by (and two float64 roundings)
    rest = gr.evaluate(doc, buf, None)
    n = (m['weights'] > 0).sum(1)
    assert (np.abs(rest - m['verts']) <= (n[:, None] * 2.0 ** -25 + 2.0 ** -51) * np.abs(m['verts'])).all()
    total = m['weights'].astype(np.float64).sum(1)
    assert np.abs(rest - total[:, None] * m['verts'].astype(np.float64)).max() <= 2.0 ** -50
    # at every key time: the definition's posed, within the chain's bound
    t = gr.key_times(doc, buf)
    assert np.array_equal(t, (np.arange(3) / 24.0).astype(np.float32).astype(np.float64))
    bound = _bounds(m, doc, buf)
    for f in range(3):
        err = np.linalg.norm(gr.evaluate(doc, buf, t[f]) - m['posed'][f].astype(np.float64), axis=1)
        print(f'\n   K {K} key {f}: max |file - posed| = {err.max():.3e} m, bound {bound:.3e} m')
        assert err.max() <= bound
    # between two keys the file moves (LINEAR), and the rest-pose file has no animation at all
    mid = gr.evaluate(doc, buf, 0.5 * (t[0] + t[1]))
    assert np.abs(mid - gr.evaluate(doc, buf, t[0])).max() > 1e-4
    _write(tmp_path / 'rest.glb', m, animated=False)
    rdoc, rbuf = gr.check_rules((tmp_path / 'rest.glb').read_bytes())
    assert 'animations' not in rdoc and np.array_equal(gr.evaluate(rdoc, rbuf, None), rest)


@pytest.mark.parametrize('K', [4, 8])
def test_the_file_with_correctives_shows_the_targets(tmp_path, K):
    m = _small_mesh(K, correct=True)
    _write(tmp_path / 'c.glb', m)
    blob = (tmp_path / 'c.glb').read_bytes()
    _write(tmp_path / 'd.glb', m)
    assert blob == (tmp_path / 'd.glb').read_bytes()
    doc, buf = gr.check_rules(blob)
    prim = doc['meshes'][0]['primitives'][0]
    assert len(prim['targets']) == 3 and doc['meshes'][0]['weights'] == [0.0, 0.0, 0.0]
    for f in range(3):
        assert gr.accessor(doc, buf, prim['targets'][f]['POSITION']).tobytes() == m['delta'][f].tobytes()
    assert m['dflag'][1, 5] == 1 and not m['delta'][1, 5].any() and (m['dflag'] == 0).mean() > 0.8
    t = gr.key_times(doc, buf)
    chain = _bounds(m, doc, buf)
    for f in range(3):
        ok = m['dflag'][f] == 0
        err = np.linalg.norm(gr.evaluate(doc, buf, t[f]) - m['target'][f].astype(np.float64), axis=1)
        bound = chain + np.sqrt(3.0) * gr.corrective_bound(m['M'][f], m['delta'][f], m['target'][f])
        print(f'\n   K {K} key {f}: max |file - target| = {err[ok].max():.3e} m, bound {bound[ok].min():.3e} m')
        assert (err[ok] <= bound[ok]).all()
        # the flagged vertex is shown where plain skinning puts it
        if not ok.all():
            plain = np.linalg.norm(gr.evaluate(doc, buf, t[f]) - m['posed'][f].astype(np.float64), axis=1)
            assert (plain[~ok] <= chain).all()
    # STEP: just before the next key the earlier key's target is still the one that is on
    late = gr.evaluate(doc, buf, t[1] - 1e-4)
    assert np.abs(late - gr.evaluate(doc, buf, t[1])).max() > 0


def test_the_file_with_a_world_node(tmp_path):
    m = _small_mesh(4, correct=False, world=True)
    _write(tmp_path / 'w.glb', m)
    doc, buf = gr.check_rules((tmp_path / 'w.glb').read_bytes())
    top = [i for i, n in enumerate(doc['nodes']) if n['name'] == 'world'][0]
    assert doc['nodes'][top]['children'] == [doc['skins'][0]['skeleton']] and doc['scenes'][0]['nodes'] == [0, top]
    t = gr.key_times(doc, buf)
    bound = _bounds(m, doc, buf, world=True)
    for f in range(3):
        want = m['posed'][f].astype(np.float64) @ m['Rh'][f].astype(np.float64).T + m['Th'][f].astype(np.float64)
        err = np.linalg.norm(gr.evaluate(doc, buf, t[f]) - want, axis=1)
        print(f'\n   key {f}: max |file - (R(Rh) posed + Th)| = {err.max():.3e} m, bound {bound:.3e} m')
        assert err.max() <= bound


def test_quaternions_and_keys():
    from occnerf_amd import gltf, mesh, synth
    rng = np.random.RandomState(5)
    for _ in range(200):                                    # every branch of Shepperd's choice, angles up to pi
        R = synth.rodrigues_exact(rng.uniform(-1, 1, 3) * rng.choice([0.1, 1.0, 1.8, 3.1]))
        q = gltf.quaternion(R)
        assert abs((q * q).sum() - 1.0) < 1e-15 and np.abs(gr._rotation(q) - R).max() < 1e-14
    R = synth.rodrigues_exact([0.0, 0.0, np.pi])
    assert np.abs(gr._rotation(gltf.quaternion(R)) - R).max() < 1e-14
    q = gltf.quaternion(R)
    assert np.array_equal(gltf.quaternion(R, -q), -q) and np.array_equal(gltf.quaternion(R, q), q)
    # the keys compose back to G, and the local translation is the rest offset up to the float32 rounding inside Rs / Ts
    b = _body()
    cnl = b['frames'][0]['cnl_gtfms']
    G = mesh.joint_transforms(b['Rs'][1], b['Ts'][1], cnl)
    rot, tra = mesh.local_keys(G)
    rest = gltf.rest_translations(cnl)
    assert np.abs(tra[1:] - rest[1:]).max() < 2e-6 and np.array_equal(rest[0], cnl[0, :3, 3].astype(np.float64))
    again = np.zeros_like(G)
    for j in range(24):
        L = np.eye(4)
        L[:3, :3], L[:3, 3] = gr._rotation(rot[j]), tra[j]
        again[j] = L if j == 0 else again[synth.SMPL_PARENT[j]] @ L
    assert np.abs(again - G).max() < 20 * gr.rotation_defect(b['Rs'][1]) + 1e-12
    print(f"\n   largest |local translation - rest offset| = {np.abs(tra[1:] - rest[1:]).max():.3e} m")


# ------------------------------------------------------------------ what surrounds the kernels
def test_c_entries_refuse_bad_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from occnerf_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def skin(V=5, x=p, vol=p, nb=24, G=32, bmin=p, K=4, out=p):
        return lib.occnerf_mesh_skin(x, V, vol, nb, G, bmin, p, K, out, p, p, p, None)

    def lbs(V=5, x=p, K=4, Rs=p, F=1, nb=24, target=None, tflag=None, max_delta=0.05, posed=p, delta=None):
        return lib.occnerf_mesh_lbs(x, V, p, p, K, Rs, p, F, nb, target, tflag, max_delta, posed, delta, None, None)

    def refused(rc, who, word):
        msg = lib.occnerf_last_error()
        assert rc != 0 and msg.startswith(who.encode()) and word.encode() in msg, (rc, msg)
    for K in (0, 3, 5, 16):
        refused(skin(K=K), 'mesh_skin', f'K={K}')
        refused(lbs(K=K), 'mesh_lbs', f'K={K}')
    refused(skin(nb=33), 'mesh_skin', 'nb=33')
    refused(skin(nb=0), 'mesh_skin', 'nb=0')
    refused(skin(G=1), 'mesh_skin', 'G=1')
    refused(skin(G=1025), 'mesh_skin', 'G=1025')
    refused(skin(vol=None), 'mesh_skin', 'null')
    refused(skin(bmin=None), 'mesh_skin', 'null')
    refused(skin(x=None), 'mesh_skin', 'null')
    refused(skin(out=None), 'mesh_skin', 'null')
    refused(skin(V=-1), 'mesh_skin', 'V=-1')
    assert skin(V=0, x=None, out=None) == 0                  # nothing to do: 0 without a launch (there is no GPU here to launch on)
    refused(lbs(F=0), 'mesh_lbs', 'F=0')
    refused(lbs(F=-2), 'mesh_lbs', 'F=-2')
    refused(lbs(nb=33), 'mesh_lbs', 'nb=33')
    refused(lbs(max_delta=-1.0), 'mesh_lbs', 'max_delta')
    refused(lbs(max_delta=float('nan')), 'mesh_lbs', 'max_delta')
    refused(lbs(max_delta=float('inf')), 'mesh_lbs', 'max_delta')
    refused(lbs(Rs=None), 'mesh_lbs', 'null')
    refused(lbs(x=None), 'mesh_lbs', 'null')
    refused(lbs(posed=None), 'mesh_lbs', 'null')
    refused(lbs(target=p), 'mesh_lbs', 'null')               # a target without its flags and outputs
    refused(lbs(V=-1), 'mesh_lbs', 'V=-1')
    assert lbs(V=0, x=None, posed=None) == 0
    assert lib.occnerf_abi_version() == 5


def test_configuration_wrappers_and_sources():
    import torch
    from occnerf_amd import gltf, mesh, ops
    from occnerf_amd.config import default_cfg
    assert dict(default_cfg().mesh_rig) == {'enable': False, 'frames': None, 'influences': 4, 'fps': 30.0, 'correctives': False,
                                            'max_correctives': 16, 'max_delta': 0.05, 'world': False} == mesh.RIG_DEFAULTS
    cfg = default_cfg().merge_from_list(['mesh_rig.enable', 'True', 'mesh_rig.frames', '[0, 3, 17]', 'mesh_rig.influences', '8'])
    got = mesh.check_rig(cfg.mesh_rig)
    assert got['enable'] is True and got['frames'] == [0, 3, 17] and got['influences'] == 8
    assert mesh.check_rig(default_cfg().merge_from_list(['mesh_rig.frames', 'all']).mesh_rig)['frames'] == 'all'
    for key, value, word in (('influences', 5, 'mesh_rig.influences = 5'), ('influences', 4.5, 'mesh_rig.influences'),
                             ('fps', 0.0, 'mesh_rig.fps = 0.0'), ('fps', float('inf'), 'mesh_rig.fps'),
                             ('max_delta', -0.1, 'mesh_rig.max_delta = -0.1'), ('max_delta', float('nan'), 'mesh_rig.max_delta'),
                             ('max_correctives', 0, 'mesh_rig.max_correctives = 0'), ('correctives', 1, 'mesh_rig.correctives = 1'),
                             ('enable', 'yes', 'mesh_rig.enable'), ('world', None, 'mesh_rig.world'),
                             ('frames', 3, 'mesh_rig.frames = 3'), ('frames', 'some', 'mesh_rig.frames')):
        with pytest.raises(RuntimeError, match=re.escape(word)):
            mesh.check_rig({**mesh.RIG_DEFAULTS, key: value})
    with pytest.raises(RuntimeError, match='mesh_rig.frames: frame 100 outside the 100 frames'):
        mesh._frame_indices(mesh.PoseFrames(None, total_frames=100), [0, 100], 'mesh_rig.frames')
    x = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match='mesh_skin: x_c must be a CUDA'):
        ops.mesh_skin(x, torch.zeros(24, 4, 4, 4), BOX[0], BOX[1])
    with pytest.raises(RuntimeError, match='mesh_lbs: x_c must be a CUDA'):
        ops.mesh_lbs(x, torch.zeros(5, 4, dtype=torch.uint8), torch.zeros(5, 4), torch.zeros(1, 24, 3, 3), torch.zeros(1, 24, 3))
    m = _small_mesh(4, correct=False)
    for kw, word in (({'joints': m['joints'][:, :3]}, 'K 4 or 8'), ({'faces': m['faces'] + 40}, 'face index'),
                     ({'verts': m['verts'][:0], 'colors': m['colors'][:0], 'joints': m['joints'][:0], 'weights': m['weights'][:0]},
                      'without vertices')):
        a = {**m, **kw}
        with pytest.raises(RuntimeError, match=word):
            gltf.write_glb(os.devnull, a['verts'], a['faces'], a['colors'], a['joints'], a['weights'], a['cnl'])
    with pytest.raises(RuntimeError, match='fps = 0.0'):
        gltf.write_glb(os.devnull, m['verts'], m['faces'], m['colors'], m['joints'], m['weights'], m['cnl'], fps=0.0)
    run = open(os.path.join(ROOT, 'run.py')).read()
    assert 'export_rig(' in run and "mrig.get('enable', False)" in run and 'mesh_rig.enable' in run
    make = open(os.path.join(ROOT, 'occnerf_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bmesh_rig\.hip\b', make, flags=re.M)
    src = re.sub(r'//[^\n]*', '', open(os.path.join(ROOT, 'occnerf_amd', 'csrc', 'mesh_rig.hip')).read()).lower()
    assert 'fma' not in src and 'atomic' not in src
    head = open(os.path.join(ROOT, 'include', 'occnerf_hip.h')).read()
    assert 'int occnerf_mesh_skin(' in head and 'int occnerf_mesh_lbs(' in head
    assert 'import trimesh' not in open(gltf.__file__).read() and 'export_rig' in mesh.__doc__
