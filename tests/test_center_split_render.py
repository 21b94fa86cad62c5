"""GPU: whole frames with cfg.center_split on against off (csrc/center.hip, Network._render_rays): the classification
stage takes the collapsed samples out of the kNN and feature kernels' list and the canonical MLP reads the centre row for
them -- rgb, alpha, depth and the per-sample raw values must not move by a bit, on every path that goes through the stage."""
import numpy as np
import pytest
import torch

from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

S = 128


def _frame(pose):
    from occnerf_amd import seeded, synth
    return seeded.frame_to_device(synth.make_frame(img_size=64, pose72=synth.seeded_pose(pose), orbit_frame=28), DEV)


def _render(net, data, split, watch_raw=True):
    """(outputs, per-pass raw tensors, live count, taken count or None) of one frame."""
    from occnerf_amd import ops
    before = net.cfg.get('center_split', 'auto')
    net.cfg.center_split = split                # (True forces the stage on where 'auto' leaves it off: the f16x3 offsets)
    raws, taken, live = [], [], []
    real = ops.composite

    def composite(raw, *a, **k):
        raws.append(raw.clone())
        live.append(net.last_live_count.clone())
        taken.append(None if net.last_center_taken is None else net.last_center_taken.clone())
        return real(raw, *a, **k)
    ops.composite = composite if watch_raw else real
    try:
        with torch.no_grad():
            out = net(**data, iter_val=1e7)
    finally:
        ops.composite = real
        net.cfg.center_split = before
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in ('rgb', 'alpha', 'depth')}, raws, live, taken


def _same_frames(net, data):
    on, raw_on, live, taken = _render(net, data, True)
    off, raw_off, live_off, taken_off = _render(net, data, False)
    assert all(t is None for t in taken_off), 'cfg.center_split=False runs without the stage'
    for k in ('rgb', 'alpha', 'depth'):
        assert torch.equal(on[k], off[k]) and torch.equal(on[k].view(torch.int32), off[k].view(torch.int32)), k
    assert len(raw_on) == len(raw_off) > 0
    for a, b in zip(raw_on, raw_off):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'raw (rgb, density, distance per sample)'
    assert float(on['alpha'].max()) > 0.05, 'the frame is not empty'
    n_live = sum(int(x) for x in live)
    n_taken = sum(int(t) for t in taken if t is not None)
    assert all(t is not None for t in taken), 'the stage ran in every pass'
    assert n_live == sum(int(x) for x in live_off)
    return n_live, n_taken, len(raw_on)


def _net(amplify=False, non_rigid=True, precision='fp32'):
    from occnerf_amd import seeded
    net = seeded.build_network(seed=0, amplify=amplify, S=S, non_rigid=non_rigid, device=DEV, mlp_precision=precision)
    net.cfg.dedup_repeated_samples = False
    return net


@pytest.mark.parametrize('pose', [1, 2])
def test_random_init_frames(pose):
    n_live, n_taken, _ = _same_frames(_net(), _frame(pose))
    print(f'\n   pose {pose}: {n_taken} of {n_live} live samples taken ({100.0 * n_taken / n_live:.1f} %)')
    if pose == 1:       # the stage does take what it was built for: at least a quarter of the live samples
        assert n_taken >= 0.25 * n_live, (n_taken, n_live)


def test_amplified_checkpoint():
    n_live, n_taken, _ = _same_frames(_net(amplify=True), _frame(1))
    print(f'\n   amplified, pose 1: {n_taken} of {n_live} live samples taken')
    assert n_taken > 0


def test_f16x3_watched():
    """cfg.mlp_precision = 'f16x3' with its domain check on: the split-operand kernels read the same in_rows (the stage forced
    on: by default it is off behind the split-operand non-rigid kernel, where it does not pay)."""
    net = _net(precision='f16x3')
    assert net.cfg.get('f16x3_domain_check', True)
    n_live, n_taken, _ = _same_frames(net, _frame(1))
    assert n_taken > 0


def test_three_passes():
    net, data = _net(), _frame(1)
    R = int(data['near'].numel())
    net.cfg.max_samples_per_pass = (-(-R // 3)) * S
    n_live, n_taken, passes = _same_frames(net, data)
    assert passes == 3 and n_taken > 0


def test_ignore_non_rigid_motions():
    n_live, n_taken, _ = _same_frames(_net(non_rigid=False), _frame(1))
    print(f'\n   no non-rigid offset, pose 1: {n_taken} of {n_live} live samples taken')


def test_radius_zero_takes_nothing():
    """Pose 10 of the random-init checkpoint has no provable centre radius (profiles/r05_collapse_fraction.md): the stage runs,
    flags nothing and changes nothing."""
    from occnerf_amd.modules import hann_window_weights
    net, data = _net(), _frame(10)
    nr = net.cfg.non_rigid_motion_mlp
    wc = net._weight_constants()
    center = net._knn_center(data['dst_posevec'].float().reshape(-1).contiguous(),
                             hann_window_weights(nr.multires, 1e7, nr.kick_in_iter, nr.full_band_iter).tolist(), wc['table'],
                             net._point_pack(wc))
    assert float(center[0][3]) == 0.0, 'pose 10 is the recorded radius-0 frame'
    n_live, n_taken, _ = _same_frames(net, data)
    assert n_live > 0 and n_taken == 0


def test_stale_centre_is_refused_before_any_feature_launch():
    """The centre record carries what its cached feature row was computed from (table, visibility counter, embeddings).  A
    record from before a counter update must not reach the feature kernel -- its row would be silently wrong
    (ops.sample_features' freshness contract) -- and a record of the frame's own versions renders."""
    from occnerf_amd import ops, seeded, synth
    from occnerf_amd.modules import hann_window_weights
    net = seeded.build_network(seed=0, S=32, non_rigid=True, device=DEV)
    data = seeded.frame_to_device(synth.make_frame(img_size=16, pose72=synth.seeded_pose(1), orbit_frame=28), DEV)
    nr = net.cfg.non_rigid_motion_mlp
    wc = net._weight_constants()
    stale = net._knn_center(data['dst_posevec'].float().reshape(-1).contiguous(),
                            hann_window_weights(nr.multires, 1e7, nr.kick_in_iter, nr.full_band_iter).tolist(), wc['table'],
                            net._point_pack(wc))
    assert stale.row is not None and stale.stamp == net._center_stamp(wc['table'])
    torch.autograd.graph.increment_version(net.point_counter)          # (what a training step's counter update does)
    launches, real = [], ops.sample_features

    def sample_features(*a, **k):
        launches.append(a[0].shape[0])
        return real(*a, **k)
    ops.sample_features = sample_features
    try:
        net._knn_center = lambda *a, **k: stale                        # the frame is handed the old record ...
        with torch.no_grad(), pytest.raises(RuntimeError, match='stale kNN centre'):
            net(**data, iter_val=1e7)
        assert launches == [], 'refused before the feature kernel ran'
        del net._knn_center                                            # ... and then builds its own
        with torch.no_grad():
            out = net(**data, iter_val=1e7)
    finally:
        ops.sample_features = real
        net.__dict__.pop('_knn_center', None)
    torch.cuda.synchronize()
    assert len(launches) == 2 and launches[0] == 8, 'the centre\'s own row, then the frame\'s samples'
    assert bool(torch.isfinite(out['rgb']).all()) and float(out['alpha'].max()) > 0.0, 'the frame is not empty'
