"""LPIPS v0.1 with the VGG16 trunk -- the perceptual term of the reference's training objective (trainer.py:92-106,
lossweights.lpips) and the third metric of its eval.py -- on the gfx950 kernels of occnerf_amd/csrc/lpips.hip.

`LPIPS` has the reference's constructor and forward (third_parties/lpips/lpips.py:23-124) and the reference's parameter and
buffer names (`net.slice1.0.weight` ... `net.slice5.28.bias`, `lin0.model.1.weight` ... `lin4.model.1.weight`,
`scaling_layer.shift` / `.scale`), so a reference checkpoint loads with strict=True.  Only what the reference's trainer uses
is built: net='vgg', version='0.1', lpips=True, spatial=False, a frozen trunk; anything else is refused by name.

Weights.  There is no torchvision here and nothing is downloaded:
  * pnet_rand=True (the reference's flag for a random trunk): a trunk drawn from numpy RandomState(0) (Kaiming fan-out
    normal weights, small non-zero biases), identical under every torch version (`seeded_vgg16_features`);
  * vgg16_path / load_vgg16_features(): torchvision's `features.N.*` keys of a VGG16 state_dict mapped onto the slices;
  * model_path: the reference's weights/v0.1/vgg.pth lin file (its `lin{k}.model.1.weight` keys).
pretrained=True without a model_path, or a non-random trunk without vgg16_path, raises and says what to supply.

forward(retPerLayer=True) returns the five per-tap means as they are; the reference's own res[0] comes back equal to val,
because its sum accumulates into res[0] in place (lpips.py:111-113).

The forward runs pred and target as one batch (one launch per conv layer); the backward returns gradients for whichever of
in0 / in1 require them.  There is no eager-torch path: a missing kernel is an error.
"""
import hashlib

import numpy as np
import torch
from torch import nn

from . import ops

# torchvision vgg16().features[0:30]: the conv indices and the slices of pretrained_networks.py:96-134
VGG16_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG16_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512),
                  (512, 512), (512, 512), (512, 512), (512, 512))
VGG16_POOLS = (4, 9, 16, 23)
SLICES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))
CHNS = (64, 128, 256, 512, 512)


def scale_for_lpips(image_tensor):
    """trainer.py:44-45: [0, 1] -> [-1, 1]."""
    return image_tensor * 2. - 1.


def seeded_vgg16_features(seed=0):
    """torchvision-style `features.N.weight/bias` (float32 numpy) of a random VGG16 trunk: Kaiming fan-out normal weights
    (std sqrt(2 / (9 Cout))) and biases 0.01 N(0, 1), drawn in layer order from numpy RandomState(seed)."""
    rng = np.random.RandomState(seed)
    sd = {}
    for idx, (cin, cout) in zip(VGG16_CONVS, VGG16_CHANNELS):
        std = np.sqrt(2.0 / (9 * cout))
        sd[f'features.{idx}.weight'] = (rng.standard_normal((cout, cin, 3, 3)) * std).astype(np.float32)
        sd[f'features.{idx}.bias'] = (0.01 * rng.standard_normal(cout)).astype(np.float32)
    return sd


def seeded_lin_weights(seed=0):
    """Non-negative lin weights (the learned v0.1 ones are clamped >= 0) for pretrained=False: uniform [0, 2/C)."""
    rng = np.random.RandomState(seed + 1)
    return {f'lin{k}.model.1.weight': rng.uniform(0, 2.0 / c, size=(1, c, 1, 1)).astype(np.float32)
            for k, c in enumerate(CHNS)}


def weights_checksum(state_dict, keys=None):
    """sha256 over the float32 bytes of `keys` (default: every key, sorted) of a state_dict -- pins the seeded weights."""
    h = hashlib.sha256()
    for k in sorted(state_dict) if keys is None else keys:
        v = state_dict[k]
        v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        h.update(k.encode())
        h.update(np.ascontiguousarray(v, dtype=np.float32).tobytes())
    return h.hexdigest()


class vgg16(nn.Module):
    """pretrained_networks.py:96-134 without torchvision: slice1..slice5 over features[0:30], frozen."""

    def __init__(self, requires_grad=False):
        super().__init__()
        convs = dict(zip(VGG16_CONVS, VGG16_CHANNELS))
        for s, (a, b) in enumerate(SLICES):
            seq = nn.Sequential()
            for i in range(a, b):
                if i in convs:
                    seq.add_module(str(i), nn.Conv2d(convs[i][0], convs[i][1], kernel_size=3, padding=1))
                elif i in VGG16_POOLS:
                    seq.add_module(str(i), nn.MaxPool2d(kernel_size=2, stride=2, padding=0, dilation=1, ceil_mode=False))
                else:
                    seq.add_module(str(i), nn.ReLU(inplace=True))
            setattr(self, f'slice{s + 1}', seq)
        self.N_slices = 5
        for p in self.parameters():
            p.requires_grad = requires_grad

    def convs(self):
        out = []
        for s in range(5):
            out += [m for m in getattr(self, f'slice{s + 1}') if isinstance(m, nn.Conv2d)]
        return out


def load_vgg16_features(model, state_dict):
    """Copy torchvision VGG16 `features.N.weight/bias` (N in 0..28; other keys ignored) into the slices of `model` (an LPIPS
    or its `net`)."""
    net = model.net if isinstance(model, LPIPS) else model
    mods = {}
    for s, (a, b) in enumerate(SLICES):
        for i in range(a, b):
            mods[i] = getattr(net, f'slice{s + 1}')._modules[str(i)]
    missing = []
    with torch.no_grad():
        for idx in VGG16_CONVS:
            for name in ('weight', 'bias'):
                key = f'features.{idx}.{name}'
                if key not in state_dict:
                    missing.append(key)
                    continue
                getattr(mods[idx], name).copy_(torch.as_tensor(state_dict[key]))
    if missing:
        raise KeyError(f'load_vgg16_features: missing {missing[:4]}{" ..." if len(missing) > 4 else ""}')
    return model


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer('shift', torch.Tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer('scale', torch.Tensor([.458, .448, .450])[None, :, None, None])


class NetLinLayer(nn.Module):
    """A 1x1 conv to one channel, no bias; the Dropout in front (use_dropout) is inactive in eval mode and only fixes the
    parameter's name (`model.1.weight`)."""

    def __init__(self, chn_in, chn_out=1, use_dropout=False):
        super().__init__()
        layers = [nn.Dropout(), ] if use_dropout else []
        layers += [nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False), ]
        self.model = nn.Sequential(*layers)

    @property
    def weight(self):
        return self.model[-1].weight


class _LPIPSFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, packed, in0, in1):
        val, res, work, nhwc = ops.lpips_forward(packed, in0, in1, want_res=True)
        ctx.state = (packed, work, tuple(in0.shape), nhwc)
        return val, res

    @staticmethod
    def backward(ctx, gval, gres):
        need0, need1 = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (need0 or need1):
            return None, None, None
        packed, work, shape, nhwc = ctx.state
        g = (gres + gval[None, :]).contiguous()          # val = res_0 + ... + res_4
        d0, d1 = ops.lpips_backward(packed, work, shape, nhwc, g, need0, need1)
        return None, d0, d1


class LPIPS(nn.Module):
    def __init__(self, pretrained=True, net='vgg', version='0.1', lpips=True, spatial=False, pnet_rand=False,
                 pnet_tune=False, use_dropout=True, model_path=None, eval_mode=True, verbose=True, vgg16_path=None):
        super().__init__()
        for name, got, want in (('net', net in ('vgg', 'vgg16'), "'vgg'"), ('version', version == '0.1', "'0.1'"),
                                ('lpips', lpips is True, 'True'), ('spatial', spatial is False, 'False'),
                                ('pnet_tune', pnet_tune is False, 'False')):
            if not got:
                raise NotImplementedError(f'LPIPS: {name}={locals()[name]!r} is not built here; only {name}={want} (the '
                                          'VGG16 v0.1 metric with a frozen trunk that the reference trains with)')
        if verbose:
            print('Setting up [LPIPS] perceptual loss: trunk [vgg], v[0.1], spatial [off]')
        self.pnet_type, self.pnet_tune, self.pnet_rand = 'vgg', False, pnet_rand
        self.spatial, self.lpips, self.version = False, True, version
        self.scaling_layer = ScalingLayer()
        self.chns = list(CHNS)
        self.L = 5
        self.net = vgg16(requires_grad=False)
        if pnet_rand:
            load_vgg16_features(self.net, seeded_vgg16_features(0))
        elif vgg16_path is not None:
            load_vgg16_features(self.net, torch.load(vgg16_path, map_location='cpu'))
        else:
            raise RuntimeError('LPIPS: no VGG16 trunk to load (torchvision and its download are not available): pass '
                               'vgg16_path=<torchvision vgg16 state_dict .pth>, call load_vgg16_features() after '
                               'constructing with pnet_rand=True, or use pnet_rand=True for the seeded random trunk')
        self.lin0 = NetLinLayer(CHNS[0], use_dropout=use_dropout)
        self.lin1 = NetLinLayer(CHNS[1], use_dropout=use_dropout)
        self.lin2 = NetLinLayer(CHNS[2], use_dropout=use_dropout)
        self.lin3 = NetLinLayer(CHNS[3], use_dropout=use_dropout)
        self.lin4 = NetLinLayer(CHNS[4], use_dropout=use_dropout)
        self.lins = nn.ModuleList([self.lin0, self.lin1, self.lin2, self.lin3, self.lin4])
        with torch.no_grad():
            for k, w in enumerate(seeded_lin_weights(0).values()):
                self.lins[k].weight.copy_(torch.from_numpy(w))
        if pretrained:
            if model_path is None:
                raise RuntimeError('LPIPS: pretrained=True needs model_path=<the reference\'s weights/v0.1/vgg.pth> (the lin '
                                   'layers); or pass pretrained=False for seeded lin weights')
            if verbose:
                print('Loading model from: %s' % model_path)
            self.load_state_dict(torch.load(model_path, map_location='cpu'), strict=False)
        self._pack_key, self._packed = None, None
        if eval_mode:
            self.eval()

    def _weights(self):
        convs = self.net.convs()
        return ([c.weight for c in convs], [c.bias for c in convs], [lin.weight for lin in self.lins],
                self.scaling_layer.shift, self.scaling_layer.scale)

    def packed(self):
        """The packed weight blob, rebuilt (one pass on the device) whenever a weight was replaced or modified in place."""
        w, b, li, sh, sc = self._weights()
        ts = w + b + li + [sh, sc]
        key = tuple((t.data_ptr(), t._version, t.device) for t in ts)
        if key != self._pack_key:
            self._packed = ops.lpips_pack(w, b, li, sh.reshape(3), sc.reshape(3))
            self._pack_key = key
        return self._packed

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        if normalize:                       # [0, 1] -> [-1, 1]
            in0 = 2 * in0 - 1
            in1 = 2 * in1 - 1
        if not (in0.is_cuda and in1.is_cuda):
            raise RuntimeError('LPIPS: in0 and in1 must be CUDA(HIP) tensors; there is no CPU path')
        if self.training and any(isinstance(m, nn.Dropout) for m in self.lin0.model):
            raise RuntimeError('LPIPS: train mode would make the lin layers\' dropout active; the kernels evaluate the '
                               'eval-mode metric (call .eval())')
        val, res = _LPIPSFunction.apply(self.packed(), in0.float(), in1.float())
        N = val.shape[0]
        val = val.view(N, 1, 1, 1)
        if retPerLayer:
            return val, [res[k].view(N, 1, 1, 1) for k in range(5)]
        return val


# ------------------------------------------------------------------ the patch images of the training batch
class _PatchAssemble(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, patches, bgcolor01):
        ctx.patches = patches
        return ops.patch_assemble(rgb, patches.row_of_pix, patches.n_patches, patches.size, bgcolor01)

    @staticmethod
    def backward(ctx, d_img):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return ops.patch_assemble_backward(d_img.contiguous(), ctx.patches.pix_of_row), None, None


class PatchImages:
    """The row -> pixel map of a patch batch on the device (the reference's patch_masks / patch_div_indices,
    trainer.py:31-41): pix_of_row[R] = patch * size^2 + y * size + x and its inverse row_of_pix[P * size^2] (-1: no ray).
    Overlapping patches hold duplicate rays as separate rows, so the map is a bijection between rows and covered pixels."""

    def __init__(self, pix, n_patches, size, device):
        pix = np.asarray(pix, dtype=np.int64)
        n = int(n_patches) * int(size) ** 2
        if pix.size and (pix.min() < 0 or pix.max() >= n or np.unique(pix).size != pix.size):
            raise ValueError('PatchImages: pixel indices must be distinct and inside the patches')
        inv = -np.ones(n, dtype=np.int32)
        inv[pix] = np.arange(pix.size, dtype=np.int32)
        self.n_patches, self.size = int(n_patches), int(size)
        self.pix_of_row = torch.from_numpy(pix.astype(np.int32)).to(device)
        self.row_of_pix = torch.from_numpy(inv).to(device)

    @classmethod
    def from_device_maps(cls, pix_of_row, row_of_pix, n_patches, size):
        """The two maps as the device batch builder wrote them (ops.patch_batch: int32, pix_of_row[R] cut to the batch's row
        count, row_of_pix[P * size^2]); nothing is copied or checked on the host."""
        n = int(n_patches) * int(size) ** 2
        for name, t in (('pix_of_row', pix_of_row), ('row_of_pix', row_of_pix)):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous()):
                raise RuntimeError(f'PatchImages.from_device_maps: {name} must be a contiguous 1-D int32 device tensor')
        if row_of_pix.shape[0] != n or pix_of_row.shape[0] > n:
            raise RuntimeError(f'PatchImages.from_device_maps: {row_of_pix.shape[0]} pixels / {pix_of_row.shape[0]} rows do not '
                               f'fit {n_patches} patches of {size} x {size}')
        self = cls.__new__(cls)
        self.n_patches, self.size = int(n_patches), int(size)
        self.pix_of_row, self.row_of_pix = pix_of_row, row_of_pix
        return self

    def assemble(self, rgb, bgcolor01):
        """img[P, size, size, 3] (the reference's _unpack_imgs layout): each row's rgb at its pixel, bgcolor01 elsewhere."""
        if rgb.dim() != 2 or rgb.shape != (self.pix_of_row.shape[0], 3):
            raise RuntimeError(f'PatchImages: rgb must be [{self.pix_of_row.shape[0]}, 3] (one row per mapped ray), got '
                               f'{tuple(rgb.shape)}')
        return _PatchAssemble.apply(rgb.float().contiguous(), self, [float(c) for c in np.asarray(bgcolor01).ravel()])


def patch_image_loss(rgb, target, patches, bgcolor01, lossweights, lpips):
    """The reference's image terms (trainer.py:92-106, 135-200): predicted and target rows assembled into patch images, then
    lossweights['mse'] * MSE + lossweights['lpips'] * mean(LPIPS) on the images scaled to [-1, 1].  `lpips` is any callable
    with LPIPS's forward (the HIP module here; the tests pass a torch restatement)."""
    img = patches.assemble(rgb, bgcolor01)
    tgt = patches.assemble(target, bgcolor01)
    loss = lossweights.get('mse', 0.0) * torch.mean((img - tgt) ** 2)
    if lossweights.get('lpips', 0.0):
        val = lpips(scale_for_lpips(img.permute(0, 3, 1, 2)), scale_for_lpips(tgt.permute(0, 3, 1, 2)))
        loss = loss + lossweights['lpips'] * torch.mean(val)
    return loss


def patch_target_loss(rgb, target_patches, patches, bgcolor01, lossweights, lpips):
    """patch_image_loss against target IMAGES, the reference trainer's own form (trainer.py:135-146 get_loss): the prediction
    is assembled into the patch images (_unpack_imgs, :31-41), the target is the dataset's `target_patches` [P,S,S,3] itself
    -- every pixel of the patch, also those without a ray, where the prediction holds bgcolor01."""
    img = patches.assemble(rgb, bgcolor01)
    tgt = target_patches.float()
    loss = lossweights.get('mse', 0.0) * torch.mean((img - tgt) ** 2)
    if lossweights.get('lpips', 0.0):
        val = lpips(scale_for_lpips(img.permute(0, 3, 1, 2)), scale_for_lpips(tgt.permute(0, 3, 1, 2)))
        loss = loss + lossweights['lpips'] * torch.mean(val)
    return loss


def make_training_lpips(model_path=None, vgg16_path=None, device='cuda:0'):
    """The LPIPS of train.py's `lpips` term and a line saying which weights it holds."""
    m = LPIPS(pretrained=model_path is not None, net='vgg', pnet_rand=vgg16_path is None, model_path=model_path,
              vgg16_path=vgg16_path, verbose=False).to(device).eval()
    trunk = vgg16_path or 'seeded random trunk (numpy RandomState(0); set train.lpips_vgg16_path for VGG16 weights)'
    lin = model_path or 'seeded lin weights (set train.lpips_model_path to the v0.1 vgg.pth)'
    return m, f'lpips: trunk {trunk}; lin {lin}'
