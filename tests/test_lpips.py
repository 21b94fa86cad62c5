"""LPIPS-VGG (occnerf_amd/lpips.py, csrc/lpips.hip) and the lpips term of train.py.

The fixtures tests/golden/lpips_vgg_{train,ragged}.npz are the reference's unmodified third_parties/lpips run in float32 and
float64 on the seeded trunk and the real v0.1 lin weights (tools/make_lpips_golden.py).  `restate` below is an independent
torch statement of the same maths; on the CPU it is pinned to the fixture in float64, on the GPU it is the baseline the HIP
path is compared with where the fixture has no case."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
CASES = ('train', 'ragged')


def _fixture(case):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', f'lpips_vgg_{case}.npz'))
    return {k: z[k] for k in z.files}


def _trunk(dtype=torch.float64, device='cpu'):
    from occnerf_amd.lpips import VGG16_CONVS, seeded_vgg16_features
    sd = seeded_vgg16_features(0)
    return [(torch.from_numpy(sd[f'features.{i}.weight']).to(device, dtype),
             torch.from_numpy(sd[f'features.{i}.bias']).to(device, dtype)) for i in VGG16_CONVS]


def restate(trunk, lins, in0, in1):
    """lpips.py:96-124 + pretrained_networks.py:121-134 with F.conv2d: val[N], res[5, N]."""
    dt, dev = in0.dtype, in0.device
    shift = torch.tensor([-.030, -.088, -.188], dtype=torch.float32).to(dev, dt)[None, :, None, None]
    scale = torch.tensor([.458, .448, .450], dtype=torch.float32).to(dev, dt)[None, :, None, None]

    def taps(x):
        x = (x - shift) / scale
        out, li = [], 0
        for block in (2, 2, 3, 3, 3):
            if out:
                x = F.max_pool2d(x, 2, 2)
            for _ in range(block):
                w, b = trunk[li]
                x = F.relu(F.conv2d(x, w, b, padding=1))
                li += 1
            out.append(x)
        return out

    def unit(f):
        return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True) + 1e-10) + 1e-10)

    res = [F.conv2d((unit(a) - unit(b)) ** 2, lw).mean([2, 3]).reshape(-1)
           for a, b, lw in zip(taps(in0), taps(in1), lins)]
    val = res[0]
    for r in res[1:]:
        val = val + r
    return val, torch.stack(res)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _hip_model(g):
    from occnerf_amd.lpips import LPIPS
    m = LPIPS(pretrained=False, pnet_rand=True, verbose=False)
    m.load_state_dict({f'lin{k}.model.1.weight': torch.from_numpy(g[f'lin{k}']) for k in range(5)}, strict=False)
    return m.to(DEV).eval()


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize('case', CASES)
def test_fixture_matches_float64_restatement(case):
    """The restatement in float64 reproduces the reference's float64 val and both input gradients (<= 1e-10 relative), so it
    is pinned to the unmodified reference; the seeded trunk is the one the fixture was made with."""
    from occnerf_amd.lpips import seeded_vgg16_features, weights_checksum
    g = _fixture(case)
    assert str(g['trunk_sha256']) == weights_checksum(seeded_vgg16_features(0))
    x0 = torch.from_numpy(g['in0']).double().requires_grad_(True)
    x1 = torch.from_numpy(g['in1']).double().requires_grad_(True)
    lins = [torch.from_numpy(g[f'lin{k}']).double() for k in range(5)]
    val, res = restate(_trunk(), lins, x0, x1)
    val.sum().backward()
    assert _rel(val.detach(), g['val_f64']) <= 1e-10
    assert _rel(res.detach(), g['res_f64']) <= 1e-10
    assert _rel(x0.grad, g['g0_f64']) <= 1e-10
    assert _rel(x1.grad, g['g1_f64']) <= 1e-10


def test_state_dict_names_and_lin_weights_match_the_reference():
    """LPIPS's state_dict has the reference's key names and shapes (a reference checkpoint loads with strict=True); the lin
    weights load from the reference's vgg.pth layout through model_path."""
    from occnerf_amd.lpips import LPIPS
    g = _fixture('train')
    meta = json.loads(str(g['state_dict_json']))
    m = LPIPS(pretrained=False, pnet_rand=True, verbose=False)
    sd = m.state_dict()
    assert list(sd.keys()) == meta['keys']
    assert [list(v.shape) for v in sd.values()] == meta['shapes']
    ref_like = {k: v.clone() for k, v in sd.items()}
    for k in range(5):
        ref_like[f'lin{k}.model.1.weight'] = torch.from_numpy(g[f'lin{k}'])
        ref_like[f'lins.{k}.model.1.weight'] = torch.from_numpy(g[f'lin{k}'])
    m.load_state_dict(ref_like, strict=True)
    assert torch.equal(m.lin3.model[1].weight, torch.from_numpy(g['lin3']))


def test_model_path_loads_the_lin_file(tmp_path):
    from occnerf_amd.lpips import LPIPS
    g = _fixture('train')
    path = tmp_path / 'vgg.pth'
    torch.save({f'lin{k}.model.1.weight': torch.from_numpy(g[f'lin{k}']) for k in range(5)}, path)
    m = LPIPS(pretrained=True, pnet_rand=True, model_path=str(path), verbose=False)
    for k in range(5):
        assert torch.equal(m.lins[k].model[1].weight, torch.from_numpy(g[f'lin{k}']))


def test_unsupported_options_are_refused_by_name():
    from occnerf_amd.lpips import LPIPS
    for kw, name in ((dict(net='alex'), 'net'), (dict(net='squeeze'), 'net'), (dict(version='0.0'), 'version'),
                     (dict(lpips=False), 'lpips'), (dict(spatial=True), 'spatial'), (dict(pnet_tune=True), 'pnet_tune')):
        with pytest.raises(NotImplementedError, match=name):
            LPIPS(pretrained=False, pnet_rand=True, verbose=False, **kw)
    with pytest.raises(RuntimeError, match='model_path'):
        LPIPS(pretrained=True, pnet_rand=True, verbose=False)
    with pytest.raises(RuntimeError, match='vgg16_path'):
        LPIPS(pretrained=False, verbose=False)
    with pytest.raises(RuntimeError, match='CUDA'):
        LPIPS(pretrained=False, pnet_rand=True, verbose=False)(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))


def test_load_vgg16_features_maps_torchvision_keys():
    from occnerf_amd.lpips import LPIPS, load_vgg16_features, seeded_vgg16_features
    sd = seeded_vgg16_features(5)
    m = load_vgg16_features(LPIPS(pretrained=False, pnet_rand=True, verbose=False), sd)
    assert torch.equal(m.net.slice3._modules['14'].weight, torch.from_numpy(sd['features.14.weight']))
    assert torch.equal(m.net.slice5._modules['28'].bias, torch.from_numpy(sd['features.28.bias']))
    with pytest.raises(KeyError, match='features.0.weight'):
        load_vgg16_features(m, {})


def test_argument_errors_are_reported_through_the_abi():
    from occnerf_amd import _lib
    lib = _lib.lib()
    assert lib.occnerf_lpips_workspace_floats(2, 15, 32) == -1 and lib.occnerf_lpips_workspace_floats(0, 32, 32) == -1
    assert lib.occnerf_lpips_workspace_floats(2, 16, 16) > 0
    rc = lib.occnerf_lpips_forward(None, None, None, 2, 8, 32, 0, None, None, None, None)
    assert rc != 0 and b'H and W must be >= 16' in lib.occnerf_last_error()
    rc = lib.occnerf_lpips_forward(None, None, None, 2, 32, 32, 0, None, None, None, None)
    assert rc != 0 and b'null' in lib.occnerf_last_error()
    rc = lib.occnerf_lpips_backward(None, None, 1, 32, 12, 0, None, None, None, None)
    assert rc != 0 and b'H and W must be >= 16' in lib.occnerf_last_error()
    rc = lib.occnerf_lpips_pack(None, None, None, None, None, None, None)
    assert rc != 0 and b'null' in lib.occnerf_last_error()
    rc = lib.occnerf_patch_assemble(None, None, 5, 1, 2, None, None, None)
    assert rc != 0 and b'bad sizes' in lib.occnerf_last_error()
    rc = lib.occnerf_patch_assemble_backward(None, None, 3, None, None)
    assert rc != 0 and b'null' in lib.occnerf_last_error()


def _unpack_imgs_np(rgbs, patch_masks, bgcolor, div_indices):
    """trainer.py:31-41 in numpy."""
    P, S = patch_masks.shape[:2]
    imgs = np.broadcast_to(bgcolor, (P, S, S, 3)).copy()
    for i in range(P):
        imgs[i, patch_masks[i]] = rgbs[div_indices[i]:div_indices[i + 1]]
    return imgs


@pytest.mark.parametrize('full', [True, False])
def test_patch_map_reproduces_unpack_imgs(full):
    """patch_ray_selection_map returns patch_ray_selection's rows and a row -> pixel map with which the assembly equals the
    reference's _unpack_imgs; its patch_masks are replayed here from the same draws.  Overlapping patches give duplicate rays
    as separate rows."""
    from occnerf_amd import synth
    from occnerf_amd.seeded import patch_ray_selection, patch_ray_selection_map
    frame = synth.make_frame(img_size=48, pose72=synth.seeded_pose(2), orbit_frame=3)
    P, S = 10, 8
    sel, pix = patch_ray_selection_map(frame, np.random.RandomState(7), P, S, full=full)
    assert np.array_equal(sel, patch_ray_selection(frame, np.random.RandomState(7), P, S, full=full))
    assert pix.shape == sel.shape and np.unique(pix).size == pix.size
    # replay the draws (core/data sample_patch_rays): masks and div_indices as the reference's dataset hands them over
    mask = np.asarray(frame['ray_mask']).reshape(48, 48)
    rng, masks = np.random.RandomState(7), []
    while len(masks) < P:
        y, x = rng.randint(0, 48 - S), rng.randint(0, 48 - S)
        m = mask[y:y + S, x:x + S]
        if m.all() if full else m.mean() > 0.5:
            masks.append(m.copy())
    masks = np.stack(masks)
    div = np.concatenate([[0], np.cumsum(masks.reshape(P, -1).sum(1))])
    assert div[-1] == len(sel)
    rgbs = np.random.RandomState(1).uniform(size=(len(sel), 3)).astype(np.float32)
    bg = np.array([0.25, 0.5, 0.75], np.float32)
    want = _unpack_imgs_np(rgbs, masks, bg, div)
    got = np.broadcast_to(bg, (P, S, S, 3)).copy().reshape(-1, 3)
    got[pix] = rgbs
    assert np.array_equal(got.reshape(P, S, S, 3), want)
    assert len(np.unique(sel)) < len(sel)                   # some rays lie in two patches


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_hip_matches_the_reference_fixture(case):
    """HIP val, per-tap res and both input gradients against the reference's float64; the budget is twice the reference's
    own float32-vs-float64 distance plus a 1e-6 relative floor."""
    g = _fixture(case)
    m = _hip_model(g)
    x0 = torch.from_numpy(g['in0']).to(DEV).requires_grad_(True)
    x1 = torch.from_numpy(g['in1']).to(DEV).requires_grad_(True)
    val, res = m(x0, x1, retPerLayer=True)
    val.sum().backward()
    got = {'val': val.reshape(-1), 'res': torch.cat([r.reshape(1, -1) for r in res]), 'g0': x0.grad, 'g1': x1.grad}
    for k, v in got.items():
        want, ref32 = g[f'{k}_f64'], g[f'{k}_f32']
        budget = 2 * _rel(ref32, want) + 1e-6
        err = _rel(v.detach().cpu().numpy(), want)
        print(f'{case} {k}: hip {err:.2e}  reference fp32 {_rel(ref32, want):.2e}  budget {budget:.2e}')
        assert err <= budget, (k, err, budget)


@pytest.mark.gpu
def test_eval_size_forward_matches_torch():
    """The forward at evaluation size (2 x 3 x 512 x 512) against the float32 torch restatement on the GPU."""
    g = _fixture('train')
    m = _hip_model(g)
    gen = torch.Generator(device='cpu').manual_seed(3)
    x0 = (torch.rand(2, 3, 512, 512, generator=gen) * 2 - 1).to(DEV)
    x1 = (x0.cpu() + 0.2 * torch.randn(2, 3, 512, 512, generator=gen)).clamp(-1, 1).to(DEV)
    with torch.no_grad():
        val, res = m(x0, x1, retPerLayer=True)
        want, want_res = restate(_trunk(torch.float32, DEV), [torch.from_numpy(g[f'lin{k}']).to(DEV) for k in range(5)],
                                 x0, x1)
    assert _rel(val.reshape(-1).cpu(), want.cpu()) <= 1e-4
    assert _rel(torch.cat([r.reshape(1, -1) for r in res]).cpu(), want_res.cpu()) <= 1e-4


@pytest.mark.gpu
def test_forward_backward_and_patch_gradients_are_bitwise_deterministic():
    from occnerf_amd.lpips import PatchImages, scale_for_lpips
    g = _fixture('train')
    m = _hip_model(g)
    rng = np.random.RandomState(4)
    P, S = 6, 32
    pix = np.sort(rng.choice(P * S * S, size=5000, replace=False))
    patches = PatchImages(pix, P, S, DEV)
    rgb_np = rng.uniform(size=(5000, 3)).astype(np.float32)
    tgt = torch.from_numpy(rng.uniform(size=(5000, 3)).astype(np.float32)).to(DEV)

    def run():
        rgb = torch.from_numpy(rgb_np).to(DEV).requires_grad_(True)
        img, timg = patches.assemble(rgb, (0.1, 0.2, 0.3)), patches.assemble(tgt, (0.1, 0.2, 0.3))
        val, res = m(scale_for_lpips(img.permute(0, 3, 1, 2)), scale_for_lpips(timg.permute(0, 3, 1, 2)), retPerLayer=True)
        val.mean().backward()
        return [val.detach().cpu(), torch.cat([r.reshape(-1) for r in res]).detach().cpu(), rgb.grad.cpu(), img.detach().cpu()]
    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # the assembly itself: rows at their pixels, background elsewhere, gradient = gather
    img = a[3].reshape(-1, 3).numpy()
    assert np.array_equal(img[pix], rgb_np)
    rest = np.setdiff1d(np.arange(P * S * S), pix)
    assert np.array_equal(img[rest], np.broadcast_to(np.float32([0.1, 0.2, 0.3]), (rest.size, 3)))
    assert torch.count_nonzero(a[2]) > 0


@pytest.mark.gpu
def test_training_step_with_lpips_matches_torch_restatement():
    """The train.py step with `lpips` in lossweights: every parameter gradient with the HIP LPIPS against the same step with
    the loss computed by the torch restatement (fresh identical networks, the same injected jitter)."""
    from occnerf_amd import synth
    from occnerf_amd.lpips import PatchImages, patch_image_loss
    from occnerf_amd.seeded import build_network, frame_to_device, patch_ray_selection_map
    frame = synth.make_frame(img_size=64, pose72=synth.seeded_pose(101), orbit_frame=5)
    sel, pix = patch_ray_selection_map(frame, np.random.RandomState(0), 4, 16)
    for k in ('near', 'far'):
        frame[k] = frame[k][sel]
    frame['rays'] = frame['rays'][:, sel]
    data = frame_to_device(frame, DEV)
    patches = PatchImages(pix, 4, 16, DEV)
    t_rand = torch.rand(len(sel), 32, generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        target = build_network(seed=1, amplify=True, S=32)(**data, iter_val=1e7)['rgb']
    g = _fixture('train')
    hip = _hip_model(g)
    trunk, lins = _trunk(torch.float32, DEV), [torch.from_numpy(g[f'lin{k}']).to(DEV) for k in range(5)]

    def torch_lpips(a, b):
        return restate(trunk, lins, a, b)[0]
    weights = {'lpips': 1.0, 'mse': 0.2, 'comp': 1.0}
    grads, losses = [], []
    for fn in (hip, torch_lpips):
        net = build_network(seed=0, S=32)
        net.cfg.perturb = 1.0
        net.train()
        out = net(**data, iter_val=1, t_rand=t_rand)
        loss = patch_image_loss(out['rgb'], target, patches, frame['bgcolor'] / 255., weights, fn) \
            + out['comp_loss'].float().mean()
        loss.backward()
        losses.append(float(loss))
        grads.append({n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None})
    assert abs(losses[0] - losses[1]) <= 1e-5 * abs(losses[1])
    assert sorted(grads[0]) == sorted(grads[1]) and len(grads[0]) > 0
    for n in grads[0]:
        a, b = grads[0][n].double().flatten(), grads[1][n].double().flatten()
        if torch.count_nonzero(b) == 0:
            assert torch.count_nonzero(a) == 0, n
            continue
        cos = float(a @ b / (a.norm() * b.norm()))
        assert cos >= 0.9999 and float((a - b).norm() / b.norm()) <= 1e-3, (n, cos)


@pytest.mark.gpu
def test_train_py_with_the_lpips_term(tmp_path):
    """python train.py ... train.lossweights "{'lpips': 1.0, 'mse': 0.2, 'comp': 1.0}": 12 steps at patch.size 16, a finite
    loss that falls, a checkpoint that loads with strict=True."""
    cmd = [sys.executable, os.path.join(ROOT, 'train.py'), '--cfg',
           os.path.join(ROOT, 'configs/occnerf/synthetic/occnerf.yaml'), 'render_size', '128', 'N_samples', '32',
           'train.maxiter', '12', 'train.log_interval', '1', 'patch.size', '16', 'patch.N_patches', '4',
           'train.lossweights', "{'lpips': 1.0, 'mse': 0.2, 'comp': 1.0}"]
    out = subprocess.check_output(cmd, cwd=str(tmp_path), env={**os.environ, 'PYTHONPATH': ROOT}, text=True, timeout=170)
    assert 'lpips: trunk seeded random trunk' in out
    losses = [float(line.split('loss')[1].split()[0]) for line in out.splitlines() if line.startswith('iter')]
    assert len(losses) >= 12 and all(np.isfinite(losses))
    assert np.mean(losses[-3:]) < np.mean(losses[:3])
    ckpt = torch.load(tmp_path / 'experiments' / 'occnerf' / 'synthetic' / 'capsule_body' / 'occnerf' / 'latest.tar',
                      map_location='cpu')
    assert set(ckpt) == {'iter', 'network', 'optimizer'} and ckpt['iter'] == 12
    from occnerf_amd.seeded import build_network
    net = build_network(0, S=32)
    net.load_state_dict(ckpt['network'], strict=True)
