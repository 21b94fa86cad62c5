"""GPU: the progress dump -- csrc/progress.hip against the numpy restatement of the reference's loop
(tests/progress_restatement.py), byte for byte; occnerf_amd/progress.py's ProgressDump against the existing host path on the
same frames; that a dump leaves the training state alone; resume (occnerf_amd/trainer.py); and train.py's command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import progress_restatement as pr
from tests import train_batch_cases as cases
from tests.gpu_util import DEV, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xAB


# ---- 1, 2: the kernel ------------------------------------------------------------------------------------------------------
def _rgb_values(rng, R):
    """Finite colours: below 0, above 1, exact k/255 and their float32 neighbours, and uniform ones."""
    grid = (rng.randint(0, 256, size=(R, 3)) / 255.).astype(np.float32)
    kind = rng.randint(0, 5, size=(R, 3))
    rgb = np.where(kind == 0, grid, rng.uniform(-0.5, 1.5, size=(R, 3)).astype(np.float32))
    rgb = np.where(kind == 1, np.nextafter(grid, np.float32(-1)), rgb)
    rgb = np.where(kind == 2, np.nextafter(grid, np.float32(2)), rgb)
    return np.ascontiguousarray(rgb.astype(np.float32))


def _ray_sets(rng, n):
    return {'none': np.zeros(0, np.int64), 'all': np.arange(n, dtype=np.int64), 'ends': np.array([0, n - 1], np.int64),
            'half': np.sort(rng.choice(n, n // 2, replace=False)).astype(np.int64)}


def _run_tile(H, W, rows, cols, tx, ty, ray_index, rgb, truth, bg255):
    from occnerf_amd import _lib, progress
    mosaic = torch.full((rows * H, cols * 2 * W, 3), FILL, dtype=torch.uint8, device=DEV)
    partial = torch.empty(int(_lib.lib().occnerf_progress_tile_blocks(H, W)), dtype=torch.int32, device=DEV)
    counts = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    bg01 = (np.array(bg255) / 255.).astype(np.float32)
    progress.progress_tile(torch.from_numpy(rgb).to(DEV), torch.from_numpy(ray_index).to(DEV), H, W, bg01, bg255,
                           torch.from_numpy(truth).to(DEV), mosaic, tx, ty, partial, counts[1:2])
    torch.cuda.synchronize()
    return mosaic.cpu().numpy(), counts.cpu().numpy()


def _check_tile(H, W, rows, cols, tx, ty, ray_index, rgb, truth, bg255, name):
    got, counts = _run_tile(H, W, rows, cols, tx, ty, ray_index, rgb, truth, bg255)
    mask = np.zeros(H * W, bool)
    mask[ray_index] = True
    rendered, tr = pr.panels(W, H, mask, bg255, rgb, truth_u8=truth)
    want = np.full_like(got, FILL)
    want[ty * H:(ty + 1) * H, tx * 2 * W:(tx + 1) * 2 * W] = np.concatenate([rendered, tr], axis=1)
    same(got, want, f'{name}: mosaic (tile and every byte around it)')
    assert counts[0] == -7 and counts[2] == -7, name
    assert int(counts[1]) == pr.off_background(rendered, bg255), (name, int(counts[1]))
    assert (int(counts[1]) == 0) == pr.is_empty(rendered, bg255), name
    return rendered


@pytest.mark.parametrize('H,W,rows,cols,tiles', [(37, 53, 2, 3, [(0, 0), (2, 1)]),
                                                 (64, 64, 4, 4, [(x, y) for y in range(4) for x in range(4)])],
                         ids=['37x53', '64x64'])
def test_kernel_writes_the_restatements_panels_into_its_tile_only(H, W, rows, cols, tiles):
    rng = np.random.RandomState(H)
    n = H * W
    truth = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    sets = _ray_sets(rng, n)
    bg255 = [30., 200., 90.5]
    for tx, ty in tiles:
        for name, idx in sets.items():                                       # every ray set at every tile position
            _check_tile(H, W, rows, cols, tx, ty, idx, _rgb_values(rng, len(idx)), truth, bg255, f'{H}x{W} {name} tile {tx},{ty}')


@pytest.mark.parametrize('bg255', [[0., 0., 0.], [255., 255., 255.], [127.5, 3., 252.]], ids=['black', 'white', 'odd'])
def test_off_bg_counts_what_allclose_objects_to(bg255):
    H, W = 37, 53
    n = H * W
    rng = np.random.RandomState(1)
    truth = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    idx = np.arange(n, dtype=np.int64)
    bg = np.array(bg255)

    def frame_of_bytes(b):                                    # colours that quantise to exactly the bytes b [n,3]
        rgb = ((b.astype(np.float64) + 0.5) / 255.).astype(np.float32)
        assert np.array_equal(pr.to_8b_image(rgb), b)
        return rgb

    # every rendered byte within tolerance: 0, the frame is empty
    near = np.clip(np.floor(bg)[None] + rng.randint(-2, 3, size=(n, 3)), 0, 255).astype(np.uint8)
    rgb = frame_of_bytes(near)
    q = pr.to_8b_image(rgb)
    assert pr.off_background(q.reshape(H, W, 3), bg255) == 0
    rendered = _check_tile(H, W, 1, 1, 0, 0, idx, rgb, truth, bg255, f'{bg255} near')
    assert pr.is_empty(rendered, bg255)

    # planted bytes at exactly 3 and 4 grey levels from each channel's background (for 127.5: 125, 130 in, 124, 131 out)
    planted = near.copy()
    for c in range(3):
        for j, v in enumerate((bg[c] - 3, bg[c] + 3, bg[c] - 4, bg[c] + 4, np.ceil(bg[c] - 3), np.floor(bg[c] + 3),
                               np.ceil(bg[c] - 3) - 1, np.floor(bg[c] + 3) + 1)):
            if 0 <= v <= 255 and float(v).is_integer():
                planted[100 * c + 7 * j + 3, c] = int(v)
    rgb = frame_of_bytes(planted)
    q = pr.to_8b_image(rgb).reshape(H, W, 3)
    want = pr.off_background(q, bg255)
    far = np.abs(q.reshape(-1, 3).astype(np.float64) - bg[None]) > 3 + 1e-5 * np.abs(bg[None])
    assert want == int(far.sum()) > 0
    if bg255 == [127.5, 3., 252.]:
        col = q.reshape(-1, 3)[:, 0]
        assert {124, 125, 130, 131} <= set(col.tolist())
        assert not far[col == 125, 0].any() and not far[col == 130, 0].any()
        assert far[col == 124, 0].all() and far[col == 131, 0].all()
    _check_tile(H, W, 1, 1, 0, 0, idx, rgb, truth, bg255, f'{bg255} planted')


def test_kernel_refuses_a_tile_outside_the_mosaic():
    from occnerf_amd import progress
    H, W = 8, 8
    mosaic = torch.zeros(H, 2 * W, 3, dtype=torch.uint8, device=DEV)
    args = (torch.zeros(0, 3, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), H, W, [0, 0, 0], [0, 0, 0],
            torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV), mosaic)
    work = (torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
    for tx, ty in ((1, 0), (0, 1), (-1, 0)):
        with pytest.raises(RuntimeError, match='does not fit'):
            progress.progress_tile(*args, tx, ty, *work)
    torch.cuda.synchronize()


# ---- 3-5: the dump and the trainer on a tool-made dataset --------------------------------------------------------------------
BGCOLOR = [255., 255., 255.]


@pytest.fixture(scope='module')
def data_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('progress') / 'data')
    cases.load_tool().make_dataset(path, frames=5, width=64, height=64, seed=31, focal=900.0)
    return path


def _cfg():
    from occnerf_amd import config
    cfg = config.default_cfg()
    config._finish(cfg)
    cfg.N_samples, cfg.smpl_model, cfg.bgcolor, cfg.perturb = 32, 'synthetic', list(BGCOLOR), 1.0
    return config.set_cfg(cfg)


def _network(ds, train):
    from occnerf_amd.checkpoint import make_state_dict
    from occnerf_amd.network import Network
    net = Network()
    net.generate_neural_points(ds.avg_betas)
    net.load_state_dict(make_state_dict(net.point_base.detach().numpy(), float(net.bound), seed=0), strict=True)
    net = net.to(DEV)
    return net.train() if train else net.eval()


def _progress_loader(path):
    from occnerf_amd.dataset import PreparedDataset, WholeFrames
    return WholeFrames(PreparedDataset(path, device=None), BGCOLOR)


def _host_path_frames(net, loader, it):
    """run.py's path: frames_to_device, the network, image.unpack_to_image with meta['truth_u8'] as the truth panel."""
    from occnerf_amd import image, metrics, sequence
    from occnerf_amd.dataset import NETWORK_KEYS
    frames, records = [], []
    with torch.no_grad():
        for data, _key, meta in sequence.frames_to_device(loader, 'progress', DEV):
            out = net(**{k: data[k] for k in NETWORK_KEYS}, iter_val=it)
            H, W = meta['height'], meta['width']
            mask = np.zeros(H * W, bool)
            mask[meta['ray_index'].cpu().numpy()] = True
            rgb_img, _, _ = image.unpack_to_image(W, H, mask, np.array(BGCOLOR) / 255., out['rgb'].cpu().numpy(),
                                                  out['alpha'].cpu().numpy())
            frames.append((rgb_img, meta['truth_u8'].cpu().numpy()))
            records.append(metrics.frame_metrics_from_maps(out['rgb'], out['alpha'], meta['ray_index'], meta, W, H,
                                                           bgcolor=np.array(BGCOLOR) / 255.))
    return frames, records


def test_dump_equals_the_host_path_and_the_early_stop_crop(data_path, tmp_path):
    from PIL import Image
    from occnerf_amd import metrics
    from occnerf_amd.progress import ProgressDump
    cfg = _cfg()
    loader = _progress_loader(data_path)
    net = _network(loader.dataset, train=True)
    cfg.perturb = 0.
    net.eval()
    frames, records = _host_path_frames(net, loader, 100)
    net.train()
    cfg.perturb = 1.0
    want, empty, seen = pr.progress_image(frames, BGCOLOR, 100)
    assert not empty and seen == 5 and want.shape == (64, 4 * 128, 3)            # 5 frames: one row of 4
    dump = ProgressDump(loader, str(tmp_path), device=DEV)
    got = dump.run(net, net, 100)
    assert net.training and cfg.perturb == 1.0
    assert not got['is_empty']
    same(got['mosaic'], want, 'dump mosaic vs the restatement on the host path')
    assert [int(c) for c in got['off_bg']] == [pr.off_background(r, BGCOLOR) for r, _ in frames]
    dump.close()
    assert Image.open(tmp_path / 'prog_000100.jpg').size == (4 * 128, 64)
    line = json.loads((tmp_path / 'progress.jsonl').read_text().splitlines()[-1])
    assert line['iter'] == 100 and line['is_empty'] is False and line['wall_s'] >= 0
    for k in metrics.KEYS:
        mean = float(np.mean([r[k] for r in records]))
        assert line[k] == mean or (line[k] is None and not np.isfinite(mean)), (k, line[k], mean)

    # through a one-GPU ShardedRenderer (submit / finish): the same rays in the same order, so the same bytes
    from occnerf_amd.parallel import ShardedRenderer
    got = dump.run(net, ShardedRenderer(net, DEV, single=True), 100)
    assert net.training and cfg.perturb == 1.0 and not got['is_empty']
    same(got['mosaic'], want, 'dump mosaic through a ShardedRenderer vs the restatement on the host path')
    assert [int(c) for c in got['off_bg']] == [pr.off_background(r, BGCOLOR) for r, _ in frames]
    dump.close()

    # a network that renders nothing: the density head far below the softplus, every frame is the background
    with torch.no_grad():
        net.cnl_mlp.module.geo_linear[0].bias.fill_(-1e4)
        torch.autograd.graph.increment_version(net.cnl_mlp.module.geo_linear[0].bias)
    cfg.perturb = 0.
    net.eval()
    frames, _ = _host_path_frames(net, loader, 100)
    net.train()
    cfg.perturb = 1.0
    want, empty, seen = pr.progress_image(frames, BGCOLOR, 100)
    assert empty and seen == 1 and want.shape == (64, 128, 3)                    # the host path stops after the first frame
    got = dump.run(net, net, 100)
    assert got['is_empty'] and all(int(c) == 0 for c in got['off_bg'])
    same(got['mosaic'], want, 'early stop: the k = 1 crop')
    dump.close()
    assert Image.open(tmp_path / 'prog_000100.jpg').size == (128, 64)
    # past iteration 5000 the reference does not look: the full mosaic
    got = dump.run(net, net, 5001)
    full, empty, _ = pr.progress_image(frames, BGCOLOR, 5001)
    assert not got['is_empty'] and not empty
    same(got['mosaic'], full, 'no early stop past iteration 5000')
    dump.close()
    assert [json.loads(ln)['is_empty'] for ln in (tmp_path / 'progress.jsonl').read_text().splitlines()] == [False, False, True, False]

    # a frame that raises: train mode and cfg.perturb come back
    class Broken:
        def __init__(self, inner):
            self.inner, self.dataset = inner, inner.dataset

        def __len__(self):
            return len(self.inner)

        def device_frames(self, *a, **k):
            it = self.inner.device_frames(*a, **k)
            yield next(it)
            raise ValueError('frame 1 is broken')

    with pytest.raises(ValueError, match='frame 1 is broken'):
        ProgressDump(Broken(loader), str(tmp_path), device=DEV).run(net, net, 7)
    assert net.training and cfg.perturb == 1.0
    torch.cuda.synchronize()


def _trainer(data_path, logdir, dump, lines=None):
    """A trainer as train.py builds it on a prepared dataset (MSE + comp), with the batches it drew on record."""
    from occnerf_amd import trainer as tr
    from occnerf_amd.dataset import PatchBatchLoader, PreparedDataset
    from occnerf_amd.progress import ProgressDump
    torch.manual_seed(0)                                      # a fresh process's generators: the stratified jitter draws from
    torch.cuda.manual_seed(0)                                 # torch.cuda's
    ds = PreparedDataset(data_path, device=DEV)
    loader = PatchBatchLoader(ds, n_patches=4, size=16, bgcolor=None, seed=0, prefetch=True)
    net = _network(ds, train=True)
    tc = dict(tr.TRAIN_DEFAULTS, log_interval=10 ** 6, save_checkpt_interval=10 ** 6)
    opt = tr.make_optimizer(net, tc)
    drawn = []

    def next_batch(it):
        b = next(loader)
        drawn.append({'it': it, 'frame_name': b['frame_name'], 'frame': b['frame'], 'u': b['u'].copy(),
                      'bgcolor': np.array(b['bgcolor']).copy(), 'rays': b['rays'].clone(),
                      'cuda_rng': torch.cuda.get_rng_state().clone()})      # the generator the step's jitter is drawn from
        return b

    progress = ProgressDump(_progress_loader(data_path), logdir, device=DEV) if dump else None
    t = tr.Trainer(net, opt, tc, logdir, next_batch, lambda b, it: tr.dataset_step_loss(net, b, it, tc), loader=loader,
                   progress=progress, dump_interval=0, keep_losses=True, out=(lines.append if lines is not None else print))
    return t, drawn


_twins = {}
STRAIGHT = ('a', 'b', 'c', 'd')


def _pairs(key, differ, upto=None):
    return [differ(_twins[x][key][:upto] if upto else _twins[x][key], _twins[y][key][:upto] if upto else _twins[y][key])
            for i, x in enumerate(STRAIGHT) for y in STRAIGHT[i + 1:]]


def _jitter(state, rows, samples=32):
    """The stratified jitter train_path draws for `rows` rays from a generator in `state`: torch.rand(rows, N_samples)."""
    gen = torch.Generator(device=DEV)
    gen.set_state(state)
    return torch.rand(rows, samples, device=DEV, generator=gen)


def _straight_twins(data_path, tmp_path_factory):
    """Four trainers on one dataset and seed, six steps each, no dump: what run-to-run agreement this step has.  The step
    sums with float atomics, so two runs need not agree bit for bit; every one of the six pairs is compared, and the largest
    difference among them is the twin-against-twin figure the tests below allow twice of (one pair alone is one sample of a
    maximum over all parameters and underestimates it at random)."""
    if not _twins:
        for name in STRAIGHT:
            _cfg()
            t, drawn = _trainer(data_path, str(tmp_path_factory.mktemp('twin_' + name)), dump=False)
            t.run(t.start(), 6)
            torch.cuda.synchronize()
            _twins[name] = {'iter': t.iter, 'groups': [{k: g[k] for k in ('name', 'lr', 'base_lr')} for g in t.opt.param_groups],
                            'steps': {k: float(v['step']) for k, v in t.opt.state_dict()['state'].items()}, 'drawn': drawn, 'losses': [float(l.double()) for _, l in t.losses],
                            'loss_bits': [l.clone() for _, l in t.losses],
                            'params': {n: p.detach().clone() for n, p in t.net.named_parameters()}}
        _twins['loss_diff4'] = max(_pairs('losses', lambda p, q: max(abs(x - y) for x, y in zip(p, q)), upto=4))
        _twins['bitwise4'] = all(_pairs('loss_bits', lambda p, q: all(torch.equal(x, y) for x, y in zip(p, q)), upto=4))
        _twins['param_diff'] = max(_pairs('params', lambda p, q: max(float((p[n].double() - q[n].double()).abs().max()) for n in p)))
        _twins['params_bitwise'] = all(_pairs('params', lambda p, q: all(torch.equal(p[n], q[n]) for n in p)))
        # what does not pass through a float atomic is the same in every run, bit for bit: the draws and the generator
        for name in STRAIGHT[1:]:
            for mine, twin in zip(_twins[name]['drawn'], _twins['a']['drawn']):
                assert mine['frame_name'] == twin['frame_name'] and torch.equal(mine['rays'], twin['rays'])
                assert torch.equal(mine['cuda_rng'], twin['cuda_rng']), (name, mine['it'])
        states = [d['cuda_rng'] for d in _twins['a']['drawn']]
        assert not any(torch.equal(x, y) for x, y in zip(states, states[1:]))        # every step draws from the generator
    return _twins


def test_dump_leaves_training_alone(data_path, tmp_path, tmp_path_factory):
    tw = _straight_twins(data_path, tmp_path_factory)
    cfg = _cfg()
    t, drawn = _trainer(data_path, str(tmp_path), dump=True)
    first = t.start()
    for it in (first, first + 1):
        loss, _ = t.step(it)
        t.losses.append((it, loss.detach()))
    torch.cuda.synchronize()
    before = {'training': t.net.training, 'perturb': cfg.perturb, 'rng': torch.cuda.get_rng_state().clone(),
              'params': {n: p.detach().clone() for n, p in t.net.named_parameters()},
              'versions': {n: p._version for n, p in t.net.named_parameters()},
              'pending': t.loader._pending[1]}
    assert 'point_counter' in before['params'] and before['training'] and before['perturb'] == 1.0
    got = t.progress.run(t.net, t.net, 2)
    torch.cuda.synchronize()
    assert got['mosaic'].shape == (64, 4 * 128, 3)
    assert t.net.training is before['training'] and cfg.perturb == before['perturb']
    assert torch.equal(torch.cuda.get_rng_state(), before['rng'])
    for n, p in t.net.named_parameters():
        assert torch.equal(p.detach(), before['params'][n]), n
        assert p._version == before['versions'][n], n
    frame, u, bg = t.loader._pending[1]
    assert frame == before['pending'][0] and np.array_equal(u, before['pending'][1]) and np.array_equal(bg, before['pending'][2])
    for it in (3, 4):                                            # hipGraph replay after an eval-mode render
        loss, _ = t.step(it)
        t.losses.append((it, loss.detach()))
    torch.cuda.synchronize()
    t.progress.close()
    for mine, twin in zip(drawn, tw['a']['drawn']):              # the loader's next batches, bit for bit
        assert mine['frame_name'] == twin['frame_name'] and mine['frame'] == twin['frame']
        assert np.array_equal(mine['u'], twin['u']) and np.array_equal(mine['bgcolor'], twin['bgcolor'])
        assert torch.equal(mine['rays'], twin['rays']), mine['it']
        assert torch.equal(mine['cuda_rng'], twin['cuda_rng']), mine['it']           # steps 3 and 4 draw the twin's jitter
    losses = [float(l.double()) for _, l in t.losses]
    diffs = [abs(x - y) for x, y in zip(losses, tw['a']['losses'])]
    twin4, bitwise4 = tw['loss_diff4'], tw['bitwise4']
    print(f'\n   twin against twin ({len(STRAIGHT)} runs, every pair), 4 steps, no dump: bitwise {bitwise4}, max |loss difference| '
          f'{twin4:.3e}; '
          f'with the dump against twin a: {[f"{d:.3e}" for d in diffs]}')
    record = {'what': 'tests/test_k_progress.py::test_dump_leaves_training_alone: losses of 4 steps (5 frames of 64 x 64, '
                      'N_samples 32, MSE + comp), a dump after step 2, against a twin trainer without one; the twin-against-twin figure is the largest over every pair of '
                      f'{len(STRAIGHT)} such twins',
              'twins_bitwise_equal': bool(bitwise4), 'twin_against_twin_max_loss_difference': twin4,
              'allowance': 0.0 if bitwise4 else 2 * twin4, 'dump_against_twin_loss_differences': diffs}
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'progress_dump_check.json'), 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    if bitwise4:
        assert all(torch.equal(l, w) for (_, l), w in zip(t.losses, tw['a']['loss_bits'])), diffs
    else:
        assert max(diffs) <= 2 * twin4, (diffs, twin4)


def _optimizer_state(opt):
    """{parameter name: {key: tensor or number}} of an optimiser whose groups hold one named parameter each."""
    sd = opt.state_dict()
    return {g['name']: sd['state'].get(g['params'][0], {}) for g in sd['param_groups']}


def test_resume_continues_the_straight_run(data_path, tmp_path, tmp_path_factory):
    """Two halves.  What a resume restores is compared at the resume point, bit for bit, with the trainer that saved and with
    the uninterrupted twin -- nothing there passes through a float atomic, so a correct resume always meets it and one that
    restores any part wrongly (the generator, the loader, a moment of Adam) never does.  The three steps after it are then
    compared with the twin's under the rule of test_dump_leaves_training_alone."""
    tw = _straight_twins(data_path, tmp_path_factory)
    a = tw['a']
    _cfg()
    first, first_drawn = _trainer(data_path, str(tmp_path), dump=False)
    first.run(first.start(), 3)
    torch.cuda.synchronize()
    saved = {'params': {n: p.detach().clone() for n, p in first.net.named_parameters()},
             'opt': {n: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
                     for n, st in _optimizer_state(first.opt).items()},
             'groups': [{k: g[k] for k in ('name', 'lr', 'base_lr')} for g in first.opt.param_groups],
             'cuda_rng': torch.cuda.get_rng_state().clone(), 'loader': first.loader.state()}
    for mine, twin in zip(first_drawn, a['drawn']):           # the saving run is the twin's first half
        assert torch.equal(mine['rays'], twin['rays']) and torch.equal(mine['cuda_rng'], twin['cuda_rng'])
    del first
    lines = []
    _cfg()
    second, drawn = _trainer(data_path, str(tmp_path), dump=False, lines=lines)      # fresh objects
    start = second.start(resume=True, load_net='latest')
    assert start == 4 and not any('reseeded' in ln for ln in lines)

    # the resume point: network, Adam, rates, generator and loader are the saving trainer's after step 3, bit for bit
    for n, p in second.net.named_parameters():
        assert torch.equal(p.detach(), saved['params'][n]), n
    got = _optimizer_state(second.opt)
    assert sorted(got) == sorted(saved['opt'])
    for n, st in got.items():
        assert sorted(st) == sorted(saved['opt'][n]), n
        for k, v in st.items():
            w = saved['opt'][n][k]
            assert (torch.equal(v.cpu(), w.cpu()) if torch.is_tensor(v) else v == w), (n, k)
    assert [{k: g[k] for k in ('name', 'lr', 'base_lr')} for g in second.opt.param_groups] == saved['groups']
    assert torch.equal(torch.cuda.get_rng_state(), saved['cuda_rng'])
    assert torch.equal(torch.cuda.get_rng_state(), a['drawn'][3]['cuda_rng'])        # the twin's generator before its step 4
    assert not torch.equal(torch.cuda.get_rng_state(), a['drawn'][2]['cuda_rng'])
    state = second.loader.state()
    assert sorted(state) == sorted(saved['loader'])
    for k, v in state.items():
        assert (torch.equal(v, saved['loader'][k]) if torch.is_tensor(v) else v == saved['loader'][k]), k

    second.run(start, 6)
    torch.cuda.synchronize()
    assert [d['it'] for d in drawn] == [4, 5, 6]
    for mine, twin in zip(drawn, a['drawn'][3:]):
        assert mine['frame_name'] == twin['frame_name'] and mine['frame'] == twin['frame']
        assert np.array_equal(mine['u'], twin['u']) and np.array_equal(mine['bgcolor'], twin['bgcolor'])
        assert torch.equal(mine['rays'], twin['rays']), mine['it']
        # the generator each resumed step draws from, and the jitter it gives for the step's rays, are the twin's
        assert torch.equal(mine['cuda_rng'], twin['cuda_rng']), mine['it']
        rows = int(mine['rays'].shape[1])
        assert torch.equal(_jitter(mine['cuda_rng'], rows), _jitter(twin['cuda_rng'], rows)), mine['it']
    assert not torch.equal(_jitter(drawn[0]['cuda_rng'], 64), _jitter(a['drawn'][2]['cuda_rng'], 64))
    assert second.iter == a['iter'] == 6
    assert torch.load(tmp_path / 'latest.tar', map_location='cpu')['iter'] == 6
    assert len(a['groups']) == len(second.opt.param_groups)
    for ga, gb in zip(a['groups'], second.opt.param_groups):
        assert ga['name'] == gb['name'] and ga['lr'] == gb['lr'] and ga['base_lr'] == gb['base_lr']
    sb = second.opt.state_dict()['state']
    assert sorted(a['steps']) == sorted(sb) and all(a['steps'][k] == float(sb[k]['step']) == 6 for k in sb)
    diff = max(float((a['params'][n].double() - p.detach().double()).abs().max()) for n, p in second.net.named_parameters())
    print(f'\n   straight twins ({len(STRAIGHT)} runs, every pair) after 6 steps: parameters bitwise {tw["params_bitwise"]}, '
          f'max |difference| {tw["param_diff"]:.3e}; resumed against twin a: {diff:.3e}')
    if tw['params_bitwise']:
        for n, p in second.net.named_parameters():
            assert torch.equal(p.detach(), a['params'][n]), n
    else:
        assert diff <= 2 * tw['param_diff'], (diff, tw['param_diff'])


def test_loader_restored_in_place_builds_the_batch_ahead_again(data_path):
    """load_state / reseed on a loader that has a batch in flight: the ticket is taken and dropped, the batch is drawn again."""
    from occnerf_amd.dataset import PatchBatchLoader, PreparedDataset
    ds = PreparedDataset(data_path, device=DEV)
    twin = PatchBatchLoader(ds, n_patches=4, size=16, bgcolor=None, seed=3, prefetch=True)
    want = []
    for _ in range(3):                                        # (a batch's tensors are views of a buffer set: copy at once)
        b = next(twin)
        want.append({'frame': b['frame'], 'u': b['u'].copy(), 'rays': b['rays'].clone()})
    loader = PatchBatchLoader(ds, n_patches=4, size=16, bgcolor=None, seed=3, prefetch=True)
    next(loader)
    assert loader._pending is not None
    loader.load_state(loader.state())
    assert loader._pending is None
    for w in want[1:]:
        b = next(loader)
        assert b['frame'] == w['frame'] and np.array_equal(b['u'], w['u']) and torch.equal(b['rays'], w['rays'])
    loader.reseed(3)                                          # a fresh stream and epoch: the twin's first batch
    b = next(loader)
    assert b['frame'] == want[0]['frame'] and np.array_equal(b['u'], want[0]['u']) and torch.equal(b['rays'], want[0]['rays'])
    torch.cuda.synchronize()


# ---- 6: the command line ---------------------------------------------------------------------------------------------------
def test_train_py_checkpoints_dumps_and_resumes(tmp_path):
    from PIL import Image
    path = str(tmp_path / 'data')
    cases.load_tool().make_dataset(path, frames=4, width=64, height=64, seed=31, focal=900.0)
    cmd = [sys.executable, os.path.join(ROOT, 'train.py'), '--cfg', os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'),
           'train.dataset_path', path, 'resize_img_scale', '1.0', 'N_samples', '32', 'train.log_interval', '1', 'patch.size', '16',
           'patch.N_patches', '4', 'occlude', 'True', 'occlusion.range', '2', 'occlusion.mid', '32', 'occlusion.width', '10',
           'train.lossweights', "{'mse': 0.2, 'comp': 1.0}"]
    env = {**os.environ, 'PYTHONPATH': ROOT}
    out = subprocess.check_output(cmd + ['train.maxiter', '4', 'train.save_checkpt_interval', '2', 'progress.dump_interval', '2'],
                                  cwd=str(tmp_path), env=env, text=True, timeout=170)
    print(out)
    logdir = tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf'
    assert [int(ln.split()[1]) for ln in out.splitlines() if ln.startswith('iter')] == [1, 2, 3, 4]
    assert (logdir / 'init.tar').exists() and torch.load(logdir / 'init.tar', map_location='cpu')['iter'] == 0
    ckpt = torch.load(logdir / 'latest.tar', map_location='cpu')
    assert set(ckpt) == {'iter', 'network', 'optimizer'} and ckpt['iter'] == 4
    assert (logdir / 'latest.resume.tar').exists()
    for name in ('prog_000002.jpg', 'prog_000004.jpg'):           # 4 frames of 64 x 64: one row of four panel pairs
        assert Image.open(logdir / name).size == (4 * 128, 64), name
    records = [json.loads(ln) for ln in (logdir / 'progress.jsonl').read_text().splitlines()]
    assert [r['iter'] for r in records] == [2, 4] and all('psnr_full' in r and 'is_empty' in r for r in records)
    out = subprocess.check_output(cmd + ['train.maxiter', '4', 'train.save_checkpt_interval', '2', 'progress.dump_interval', '2',
                                         'resume', 'True', 'train.maxiter', '6'],
                                  cwd=str(tmp_path), env=env, text=True, timeout=170)
    print(out)
    assert [int(ln.split()[1]) for ln in out.splitlines() if ln.startswith('iter')] == [5, 6]
    assert torch.load(logdir / 'latest.tar', map_location='cpu')['iter'] == 6
    assert (logdir / 'prog_000006.jpg').exists()
