"""Writes tests/golden/lpips_vgg_{train,ragged}.npz: the reference's own LPIPS-VGG (third_parties/lpips, unmodified) run on the
CPU in float32 and float64 with autograd.  CPU only; it reads the reference checkout and is never run on a GPU machine.

    python tools/make_lpips_golden.py --reference <path to the OccNeRF checkout>

The reference builds its trunk with torchvision.models.vgg16(pretrained=True).features (pretrained_networks.py:99).  Neither
torchvision nor the ImageNet weights are available, so a minimal stand-in module `torchvision.models` is registered first whose
vgg16() returns the `features` Sequential of torchvision's VGG16 (31 layers) holding the seeded trunk of
occnerf_amd.lpips.seeded_vgg16_features(0).  The lin layers are the reference's real v0.1 weights (weights/v0.1/vgg.pth).

Each file holds, per case: the inputs in0, in1 (float32, [-1, 1]); val, the per-tap res and d val.sum() / d in0, d in1 in
float64 (`*_f64`) and float32 (`*_f32`); the lin weights as arrays; a checksum of the seeded trunk; and the reference's
state_dict key names and shapes.  No trunk weights are stored (59 MB); the tests regenerate them from the seed.
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {'train': (6, 32, 32), 'ragged': (3, 24, 40)}     # the training batch; floored pools with conv5 at 1 x 2


def _stand_in_torchvision(seeded):
    """`torchvision.models.vgg16(pretrained=...)` -> an object whose .features is VGG16's features Sequential (conv 3x3 pad 1 +
    ReLU(inplace) blocks and 2x2 max-pools, torchvision's indices) loaded with `seeded` (features.N.* arrays)."""
    cfg = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']

    def vgg16(pretrained=False, **_):
        layers, cin = [], 3
        for v in cfg:
            if v == 'M':
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        features = nn.Sequential(*layers)
        with torch.no_grad():
            for k, v in seeded.items():
                idx, name = k.split('.')[1:]
                getattr(features[int(idx)], name).copy_(torch.from_numpy(v))
        return types.SimpleNamespace(features=features)

    tv = types.ModuleType('torchvision')
    tv.models = types.ModuleType('torchvision.models')
    tv.models.vgg16 = vgg16
    sys.modules['torchvision'] = tv
    sys.modules['torchvision.models'] = tv.models


def _inputs(N, H, W, seed):
    rng = np.random.RandomState(seed)
    in0 = rng.uniform(-1, 1, size=(N, 3, H, W)).astype(np.float32)
    in1 = np.clip(in0 + 0.3 * rng.standard_normal((N, 3, H, W)), -1, 1).astype(np.float32)
    return in0, in1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference OccNeRF checkout (holds third_parties/lpips)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))

    sys.path.insert(0, ROOT)
    from occnerf_amd.lpips import seeded_vgg16_features, weights_checksum
    seeded = seeded_vgg16_features(0)
    _stand_in_torchvision(seeded)
    sys.path.insert(0, os.path.abspath(a.reference))       # the reference's third_parties shadows the repository's
    for name in [m for m in sys.modules if m == 'third_parties' or m.startswith('third_parties.')]:
        del sys.modules[name]
    from third_parties.lpips import LPIPS as RefLPIPS
    from third_parties.lpips import lpips as ref_lpips
    import third_parties.lpips as ref_pkg
    assert os.path.abspath(ref_pkg.__file__).startswith(os.path.abspath(a.reference)), ref_pkg.__file__

    model_path = os.path.join(a.reference, 'third_parties', 'lpips', 'weights', 'v0.1', 'vgg.pth')
    ref = RefLPIPS(pretrained=True, net='vgg', version='0.1', model_path=model_path, verbose=False).eval()
    sd = ref.state_dict()
    keys = list(sd.keys())
    meta = json.dumps({'keys': keys, 'shapes': [list(sd[k].shape) for k in keys]})
    lins = {f'lin{k}': sd[f'lin{k}.model.1.weight'].numpy().astype(np.float32) for k in range(5)}
    common = dict(state_dict_json=np.array(meta), trunk_sha256=np.array(weights_checksum(seeded)), **lins)

    for ci, (case, (N, H, W)) in enumerate(CASES.items()):
        in0, in1 = _inputs(N, H, W, 10 + ci)
        out = dict(common, in0=in0, in1=in1)
        for dt, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
            m = ref.to(dt)
            x0 = torch.from_numpy(in0).to(dt).requires_grad_(True)
            x1 = torch.from_numpy(in1).to(dt).requires_grad_(True)
            # the reference's retPerLayer res[0] is its val (lpips.py:111-113 sums into res[0] in place): the per-tap
            # means are taken from the lin layers' outputs instead, with the reference's own spatial_average
            lin_out = []
            hooks = [lin.register_forward_hook(lambda mod, inp, o: lin_out.append(o.detach())) for lin in m.lins]
            val = m(x0, x1)
            for h in hooks:
                h.remove()
            val.sum().backward()
            out[f'val_{tag}'] = val.detach().reshape(N).numpy()
            out[f'res_{tag}'] = torch.stack([ref_lpips.spatial_average(o).reshape(N) for o in lin_out]).numpy()
            out[f'g0_{tag}'] = x0.grad.numpy()
            out[f'g1_{tag}'] = x1.grad.numpy()
        path = os.path.join(a.out, f'lpips_vgg_{case}.npz')
        np.savez_compressed(path, **out)
        err = np.abs(out['val_f32'] - out['val_f64']).max() / np.abs(out['val_f64']).max()
        print(f'{path}: N={N} {H}x{W} val {out["val_f64"][:3]} ... fp32-vs-f64 rel {err:.2e}, {os.path.getsize(path)} B')


if __name__ == '__main__':
    main()
