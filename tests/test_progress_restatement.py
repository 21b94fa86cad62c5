"""CPU: the numpy restatement of the reference's progress image (tests/progress_restatement.py) against the recording of the
reference's own to_8b_image / tile_images (tests/golden/progress_mosaic_ref.npz, tools/record_progress_golden.py), the crop
rule of the early stop, the dump schedule, and the trainer's checkpoints and resume (occnerf_amd/trainer.py) on a stub
network on the host."""
import os

import numpy as np
import pytest
import torch

from tests import progress_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def golden():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'progress_mosaic_ref.npz'))
    return {k: z[k] for k in z.files}


def test_restatement_tiles_and_quantises_like_the_recorded_reference(golden):
    assert list(golden['ks']) == [1, 3, 4, 5, 9, 16] and golden['panels'].shape == (16, 6, 10, 3)
    for k in golden['ks']:
        got = pr.tile_images([golden['panels'][i] for i in range(k)])
        want = golden[f'tiled.{k}']
        assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape, (k, got.shape, want.shape)
        assert np.array_equal(got, want), k
    q = pr.to_8b_image(golden['q.in'])
    assert q.dtype == np.uint8 and np.array_equal(q, golden['q.out'])
    # the product's host quantiser is the same function
    from occnerf_amd import image
    assert np.array_equal(image.to_8b_image(golden['q.in']), golden['q.out'])


def _sixteen(seed, H=6, W=10):
    rng = np.random.RandomState(seed)
    return [(rng.randint(40, 256, size=(H, W, 3)).astype(np.uint8), rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8))
            for _ in range(16)]


@pytest.mark.parametrize('k', range(1, 17))
def test_early_stop_image_is_the_stated_crop_of_the_full_mosaic(k):
    from occnerf_amd import progress
    H, W, bg = 6, 10, [0., 0., 0.]
    frames = _sixteen(3)
    full, empty, seen = pr.progress_image(frames, bg, 100)
    assert not empty and seen == 16 and full.shape == (4 * H, 4 * 2 * W, 3)
    frames[k - 1] = (np.full((H, W, 3), 3, np.uint8), frames[k - 1][1])      # within atol of the background: empty
    for later in range(k + 2, 16, 5):                                        # a later empty frame changes nothing
        frames[later] = (np.zeros((H, W, 3), np.uint8), frames[later][1])
    img, empty, seen = pr.progress_image(frames, bg, 100)
    assert empty and seen == k
    full_k = pr.tile_images([np.concatenate(f, axis=1) for f in frames])
    assert np.array_equal(img, pr.crop_of_full(full_k, k, 16, H, W))
    assert np.array_equal(img, progress.crop_for_first_empty(full_k, k, 16, H, W))
    # past iteration 5000 the reference does not look
    img, empty, seen = pr.progress_image(frames, bg, 5001)
    assert not empty and seen == 16 and np.array_equal(img, full_k)


def test_mosaic_shape_drops_the_incomplete_row():
    from occnerf_amd import progress
    for n in range(1, 18):
        panels = [np.full((2, 3, 3), i, np.uint8) for i in range(n)]
        rows, cols = progress.mosaic_shape(n)
        assert pr.tile_images(panels).shape == (rows * 2, cols * 3, 3), n
    assert progress.mosaic_shape(5) == (1, 4) and progress.mosaic_shape(3) == (1, 3)


def test_record_line_is_strict_json():
    import json
    from occnerf_amd import progress
    line = progress.record_line(20, 1.23456, {'psnr_full': 21.5, 'psnr_vis': float('nan'), 'ssim': float('inf')}, False)

    def refuse(name):
        raise ValueError(name)

    got = json.loads(line, parse_constant=refuse)            # NaN / Infinity as bare words would call `refuse`
    assert got == {'iter': 20, 'wall_s': 1.235, 'psnr_full': 21.5, 'psnr_vis': None, 'ssim': None, 'is_empty': False}


def test_dump_refuses_frames_built_on_the_host():
    """sequence.frames_to_device takes the host path on a CPU device and under `device_frames False`; those frames have no
    truth_u8 and no maps, so the dump says so when it is built, not at iteration 20."""
    from occnerf_amd import config, progress

    class Frames:
        def device_frames(self, *a, **k):
            raise AssertionError('not reached')

    with pytest.raises(TypeError, match='synthetic subject'):
        progress.ProgressDump(object(), 'unused', device='cpu')
    with pytest.raises(ValueError, match='runs on a GPU'):
        progress.ProgressDump(Frames(), 'unused', device='cpu')
    cfg = config.default_cfg()
    config._finish(cfg)
    cfg.device_frames = False
    old = config._cfg
    config.set_cfg(cfg)
    try:
        with pytest.raises(ValueError, match='device_frames False'):
            progress.ProgressDump(Frames(), 'unused', device='cuda:0')
    finally:
        config.set_cfg(old)


def test_off_background_is_allclose():
    rng = np.random.RandomState(0)
    for bg in ([0., 0., 0.], [255., 255., 255.], [127.5, 3., 252.]):
        img = np.clip(np.array(bg)[None, None] + rng.randint(-6, 7, size=(8, 9, 3)), 0, 255).astype(np.uint8)
        assert (pr.off_background(img, bg) == 0) == pr.is_empty(img, bg)
        near = np.clip(np.array(bg)[None, None] + rng.randint(-2, 3, size=(8, 9, 3)), 0, 255).astype(np.uint8)
        assert pr.off_background(near, bg) == 0 and pr.is_empty(near, bg)


def test_schedule_is_the_references():
    from occnerf_amd import progress
    want = [it for it in range(1, 3001) if it in [20, 100, 300, 1000, 2500] or it % 500 == 0]
    assert want == [20, 100, 300, 500, 1000, 1500, 2000, 2500, 3000]
    assert [it for it in range(1, 3001) if progress.dump_due(it, 500)] == want
    assert [it for it in range(1, 3001) if pr.schedule(it, 500)] == want
    assert not any(progress.dump_due(it, 0) for it in range(1, 3001))
    from occnerf_amd import config
    d = config.default_cfg()
    assert d.train.save_checkpt_interval == 2000 and d.train.save_model_interval == 40000 and d.progress.dump_interval == 500
    assert d.save_all is True and d.resume is False


# ---- checkpoints and resume on the host ---------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.a = torch.nn.Linear(3, 4)
        self.pose_decoder = torch.nn.Linear(4, 2)


class HostLoader:
    """What the trainer asks of a loader: state / load_state / reseed around a numpy RandomState."""

    def __init__(self, seed=0):
        self.rng = np.random.RandomState(seed)

    def state(self):
        from occnerf_amd.dataset import pack_random_state
        return dict(pack_random_state(self.rng), order=[])

    def load_state(self, st):
        from occnerf_amd.dataset import unpack_random_state
        unpack_random_state(self.rng, st)

    def reseed(self, seed):
        self.rng.seed(seed)


def _stub_trainer(logdir, lines, tc_over=None):
    from occnerf_amd import trainer as tr
    net = Stub()
    tc = dict(tr.TRAIN_DEFAULTS, lr=1e-2, lr_pose_decoder=1e-3, lrate_decay=1, log_interval=1, save_checkpt_interval=2,
              **(tc_over or {}))
    groups = [{'params': [p], 'lr': tc['lr_pose_decoder' if 'pose_decoder' in n else 'lr'], 'name': n,
               'base_lr': tc['lr_pose_decoder' if 'pose_decoder' in n else 'lr']} for n, p in net.named_parameters()]
    opt = torch.optim.Adam(groups, lr=tc['lr'])
    opt.step = (lambda orig: lambda max_grad_norm=None: orig())(opt.step)
    loader = HostLoader(5)
    drawn = []

    def next_batch(it):
        x = torch.from_numpy(loader.rng.rand(6, 3).astype('float32'))
        drawn.append(x)
        return x

    t = tr.Trainer(net, opt, tc, logdir, next_batch, lambda x, it: net.pose_decoder(net.a(x)).pow(2).mean(),
                   describe=lambda x: 'rays 6  ', loader=loader, cuda_rng=False, out=lines.append)
    return t, drawn


def test_checkpoint_keys_sidecar_and_atomic_replace(tmp_path, monkeypatch):
    from occnerf_amd import trainer as tr
    lines = []
    t, _ = _stub_trainer(str(tmp_path), lines)
    assert t.start() == 1
    init = torch.load(tmp_path / 'init.tar', map_location='cpu')
    assert set(init) == {'iter', 'network', 'optimizer'} and init['iter'] == 0
    assert (tmp_path / 'init.resume.tar').exists()
    t.run(1, 3)
    ckpt = torch.load(tmp_path / 'latest.tar', map_location='cpu')
    assert set(ckpt) == {'iter', 'network', 'optimizer'} and ckpt['iter'] == 3
    side = torch.load(tmp_path / 'latest.resume.tar', map_location='cpu')
    assert side['iter'] == 3 and 'loader' in side and 'cuda_rng' not in side
    assert [ln.split()[0] for ln in lines] == ['iter', 'iter', 'saved', 'iter', 'saved']
    assert sorted(os.listdir(tmp_path)) == ['init.resume.tar', 'init.tar', 'latest.resume.tar', 'latest.tar']

    # os.replace moves a finished temporary file of the same directory over the checkpoint
    moves = []
    real_replace = os.replace
    monkeypatch.setattr(tr.os, 'replace', lambda a, b: (moves.append((a, b)), real_replace(a, b))[1])
    t.save_ckpt('latest')
    assert [os.path.basename(b) for _, b in moves] == ['latest.tar', 'latest.resume.tar']
    assert all(os.path.dirname(a) == str(tmp_path) and a != b for a, b in moves)
    monkeypatch.setattr(tr.os, 'replace', real_replace)

    # a save that raises midway leaves the old file whole and no temporary file behind
    before = (tmp_path / 'latest.tar').read_bytes()
    real_save = torch.save

    def failing_save(obj, f, *a, **k):
        real_save({'half': torch.zeros(3)}, f)
        raise OSError('disk full')

    monkeypatch.setattr(tr.torch, 'save', failing_save)
    t.iter = 99
    with pytest.raises(OSError, match='disk full'):
        t.save_ckpt('latest')
    monkeypatch.setattr(tr.torch, 'save', real_save)
    assert (tmp_path / 'latest.tar').read_bytes() == before
    assert torch.load(tmp_path / 'latest.tar', map_location='cpu')['iter'] == 3
    assert sorted(os.listdir(tmp_path)) == ['init.resume.tar', 'init.tar', 'latest.resume.tar', 'latest.tar']


def test_resume_continues_at_the_next_step_with_closed_form_rates(tmp_path):
    a_dir, b_dir = str(tmp_path / 'a'), str(tmp_path / 'b')
    straight, drawn_a = _stub_trainer(a_dir, [])
    straight.run(straight.start(), 6)
    first, _ = _stub_trainer(b_dir, [])
    first.run(first.start(), 3)
    lines = []
    second, drawn_b = _stub_trainer(b_dir, lines)
    start = second.start(resume=True, load_net='latest')
    assert start == 4 and any('resumed from' in ln for ln in lines) and not any('reseeded' in ln for ln in lines)
    for grp in second.opt.param_groups:                      # the rates the uninterrupted run holds after step 3
        base = 1e-3 if 'pose_decoder' in grp['name'] else 1e-2
        assert grp['base_lr'] == base and grp['lr'] == base * 0.1 ** (3 / 1000.)
    second.run(start, 6)
    assert [ln.split()[1] for ln in lines if ln.startswith('iter')] == ['4', '5', '6']
    assert all(torch.equal(x, y) for x, y in zip(drawn_a[3:], drawn_b)) and len(drawn_b) == 3
    for (n, p), (_, q) in zip(straight.net.named_parameters(), second.net.named_parameters()):
        assert torch.equal(p, q), n
    for ga, gb in zip(straight.opt.param_groups, second.opt.param_groups):
        assert ga['lr'] == gb['lr'] == ga['base_lr'] * 0.1 ** (6 / 1000.)
    sa, sb = straight.opt.state_dict()['state'], second.opt.state_dict()['state']
    assert all(float(sa[k]['step']) == float(sb[k]['step']) == 6 for k in sa)
    assert torch.load(os.path.join(b_dir, 'latest.tar'), map_location='cpu')['iter'] == 6


def test_a_step_that_raises_still_waits_for_the_image_writer(tmp_path):
    class Dump:
        closed = 0

        def close(self):
            self.closed += 1

    t, _ = _stub_trainer(str(tmp_path), [])
    t.progress = Dump()
    t.run(t.start(), 2)
    assert t.progress.closed == 1

    def broken(it):
        raise RuntimeError('no batch')

    t.next_batch = broken
    with pytest.raises(RuntimeError, match='no batch'):
        t.run(3, 4)
    assert t.progress.closed == 2


def test_resume_without_a_sidecar_says_so(tmp_path):
    first, _ = _stub_trainer(str(tmp_path), [])
    first.run(first.start(), 2)
    os.remove(tmp_path / 'latest.resume.tar')                # a checkpoint as the reference writes it
    lines = []
    second, drawn = _stub_trainer(str(tmp_path), lines)
    assert second.start(resume=True, load_net='latest') == 3
    assert any('not the uninterrupted one' in ln and 'latest.resume.tar' in ln for ln in lines)
    # no checkpoint of that name: a fresh start with `init`
    third, _ = _stub_trainer(str(tmp_path / 'fresh'), [])
    assert third.start(resume=True, load_net='latest') == 1 and os.path.exists(tmp_path / 'fresh' / 'init.tar')


def test_binding_declares_the_progress_kernel():
    from occnerf_amd import _lib
    assert 'occnerf_progress_tile' in _lib.SIGNATURES and 'occnerf_progress_tile_blocks' in _lib.SIGNATURES
    lib = _lib.lib()
    assert lib.occnerf_abi_version() == 5
    assert lib.occnerf_progress_tile_blocks(37, 53) == (37 * 53 + 255) // 256 and lib.occnerf_progress_tile_blocks(0, 5) == -1
    rc = lib.occnerf_progress_tile(None, None, 0, 4, 4, None, None, None, None, 4, 8, 0, 0, None, None, None)
    assert rc != 0 and b'null' in lib.occnerf_last_error()
