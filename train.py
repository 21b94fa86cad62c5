"""Training entry point with the reference's command line (train.py:48-49):

    python train.py --cfg configs/occnerf/synthetic/occnerf.yaml [train.maxiter 200 ...]

Scope: one optimisation step = Network.forward in
training mode through the differentiable path (occnerf_amd/train_path.py: torch autograd over
the HIP kNN and the HIP grid-encoder forward/backward) + MSE and completeness losses +
clip_grad_norm + Adam with the reference's per-group learning rates (optimizer.py:12-43) +
exponential decay (exp_decay.py:7-19).  Real datasets and progress dumps are out of scope; the
supervision here is a synthetic teacher (the same network with a second seeded checkpoint) rendered
through the HIP path.

`train.lossweights` containing `lpips` switches on the reference's objective (trainer.py:92-106,
135-200): predicted and teacher rays are assembled into the patch images (trainer.py:31-41), and
mse * MSE + lpips * mean(LPIPS-VGG) on those images (inputs scaled to [-1, 1]) + comp is minimised,
e.g. `train.lossweights "{'lpips': 1.0, 'mse': 0.2, 'comp': 1.0}"`.  LPIPS runs on the HIP kernels of
occnerf_amd/lpips.py; its weights come from train.lpips_model_path (the v0.1 vgg.pth lin layers) and
train.lpips_vgg16_path (a torchvision VGG16 state_dict), each a seeded stand-in when unset.  Without
`lpips` the step is the ray-wise MSE + comp one.

With a prepared dataset configured (`train.dataset_path DIR`, or the reference's `train.dataset zju_<subject>_train` /
`monocular_train`; occnerf_amd/dataset.py) the batches come from the device-side patch batch loader instead: the teacher is
not built, the target is the dataset's blended image, and the image terms are the reference trainer's own
(trainer.py:135-146: the prediction assembled into patch images against `target_patches`); without `lpips` the loss is the
ray-wise MSE against `target_rgbs` + comp.  Checkpoints use the reference's layout
({'iter','network','optimizer'} -> experiments/.../latest.tar, trainer.py:398-406)."""
import os
import time

import numpy as np
import torch

from configs import cfg, args  # noqa: F401
from core.nets import create_network
from occnerf_amd import synth
from occnerf_amd.checkpoint import make_state_dict

LR_GROUPS = (('mweight_vol_decoder', 'lr_mweight_vol_decoder'), ('pose_decoder', 'lr_pose_decoder'),
             ('non_rigid_mlp', 'lr_non_rigid_mlp'), ('point_dist', 'lr_point_dist'))
TRAIN_DEFAULTS = {'maxiter': 100, 'lr': 5e-4, 'lr_point_dist': 1e-4, 'lr_mweight_vol_decoder': 5e-5,
                  'lr_pose_decoder': 5e-5, 'lr_non_rigid_mlp': 5e-5, 'lrate_decay': 500, 'log_interval': 10,
                  'bf16': False, 'lossweights': {'mse': 0.2, 'comp': 1.0},
                  'lpips_model_path': None, 'lpips_vgg16_path': None}


def make_optimizer(net, tc):
    groups = []
    for name, p in net.named_parameters():
        if not p.requires_grad:
            continue
        lr = tc['lr']
        for key, lr_name in LR_GROUPS:
            if key in name:
                lr = tc[lr_name]
        groups.append({'params': [p], 'lr': lr, 'name': name, 'base_lr': lr})
    from occnerf_amd.optim import FusedAdam
    return FusedAdam(groups, lr=tc['lr'], betas=(0.9, 0.999))


def patch_rays(frame, rng, n_patches=6, size=32):
    """6 random 32x32 pixel patches (default.yaml:147-150) restricted to rays that hit the bbox."""
    from occnerf_amd.seeded import patch_ray_selection
    return patch_ray_selection(frame, rng, n_patches, size)


def dataset_step_loss(net, batch, it, tc, lpips=None):
    """Forward + loss of one step on a loader batch (occnerf_amd/dataset.py): trainer.py:135-146 with `lpips` in the loss
    weights, the ray-wise MSE against `target_rgbs` without; + comp."""
    from occnerf_amd.dataset import NETWORK_KEYS
    weights = tc['lossweights']
    out = net(**{k: batch[k] for k in NETWORK_KEYS}, iter_val=it)
    if 'lpips' in weights:
        from occnerf_amd.lpips import PatchImages, patch_target_loss
        n_patches, size = batch['patch_masks'].shape[0], batch['patch_masks'].shape[1]
        patches = PatchImages.from_device_maps(batch['pix_of_row'], batch['row_of_pix'], n_patches, size)
        loss = patch_target_loss(out['rgb'], batch['target_patches'], patches, batch['bgcolor'] / 255., weights, lpips)
    else:
        loss = weights['mse'] * torch.mean((out['rgb'].float() - batch['target_rgbs']) ** 2)
    return loss + weights.get('comp', 1.0) * out['comp_loss'].float().mean()


def train_on_dataset(tc, dev, dataset_path):
    """The optimisation loop on a prepared dataset: batches from create_dataloader('train'), built on the device one step
    ahead; no teacher network exists in this mode."""
    from core.data import create_dataloader
    loader = create_dataloader('train')
    ds = loader.dataset
    print(f'dataset: {dataset_path}: {len(ds)} frames of {ds.width} x {ds.height}, {len(ds.epoch_frames)} per epoch; '
          'targets are the dataset images (no teacher network)')
    net = create_network()
    net.generate_neural_points(ds.avg_betas)
    net.load_state_dict(make_state_dict(net.point_base.detach().numpy(), float(net.bound), seed=0), strict=True)
    net = net.to(dev).train()
    opt = make_optimizer(net, tc)
    cfg.perturb = 1.0
    os.makedirs(cfg.logdir, exist_ok=True)
    lpips = None
    if 'lpips' in tc['lossweights']:
        from occnerf_amd.lpips import make_training_lpips
        lpips, what = make_training_lpips(tc['lpips_model_path'], tc['lpips_vgg16_path'], dev)
        print(what)
    t0 = time.time()
    for it in range(1, int(tc['maxiter']) + 1):
        batch = next(loader)
        opt.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=bool(tc['bf16'])):
            loss = dataset_step_loss(net, batch, it, tc, lpips)
        loss.backward()
        opt.step(max_grad_norm=1.0)                                     # trainer.py:248-249
        decay = 0.1 ** (it / (tc['lrate_decay'] * 1000))                # exp_decay.py:7-19
        for grp in opt.param_groups:
            grp['lr'] = grp['base_lr'] * decay
        if it % int(tc['log_interval']) == 0 or it == 1:
            print(f"iter {it:5d}  loss {float(loss):.6f}  rays {batch['n_rows']}  frame {batch['frame_name']}  "
                  f'{time.time() - t0:.1f} s')
    torch.save({'iter': it, 'network': net.state_dict(), 'optimizer': opt.state_dict()},
               os.path.join(cfg.logdir, 'latest.tar'))
    print('saved', os.path.join(cfg.logdir, 'latest.tar'))


def main():
    tc = dict(TRAIN_DEFAULTS)
    tc.update({k: v for k, v in dict(cfg.get('train', {})).items() if k in TRAIN_DEFAULTS})
    dev = torch.device('cuda:0')
    from occnerf_amd.dataset import resolve_dataset_path
    dataset_path = resolve_dataset_path(cfg, 'train')
    if dataset_path is not None:
        return train_on_dataset(tc, dev, dataset_path)
    net = create_network()
    net.generate_neural_points(np.zeros(10, 'float32'))
    net.load_state_dict(make_state_dict(net.point_base.detach().numpy(), float(net.bound), seed=0), strict=True)
    teacher = create_network()
    teacher.generate_neural_points(np.zeros(10, 'float32'))
    teacher.load_state_dict(make_state_dict(teacher.point_base.detach().numpy(), float(teacher.bound), seed=1,
                                            amplify=True), strict=True)
    net, teacher = net.to(dev).train(), teacher.to(dev).eval()
    opt = make_optimizer(net, tc)
    cfg.perturb = 1.0
    rng = np.random.RandomState(0)
    size = int(cfg.get('render_size', 256))
    os.makedirs(cfg.logdir, exist_ok=True)
    use_lpips = 'lpips' in tc['lossweights']
    if use_lpips:
        from occnerf_amd.lpips import PatchImages, make_training_lpips, patch_image_loss
        from occnerf_amd.seeded import patch_ray_selection_map
        lpips, what = make_training_lpips(tc['lpips_model_path'], tc['lpips_vgg16_path'], dev)
        print(what)
    t0 = time.time()
    for it in range(1, int(tc['maxiter']) + 1):
        frame = synth.make_frame(img_size=size, pose72=synth.seeded_pose(100 + it % 16), orbit_frame=it % 50,
                                 orbit_period=50, bgcolor=cfg.bgcolor)
        if use_lpips:
            sel, pix = patch_ray_selection_map(frame, rng, int(cfg.patch.N_patches), int(cfg.patch.size))
            patches = PatchImages(pix, int(cfg.patch.N_patches), int(cfg.patch.size), dev)
        else:
            sel = patch_rays(frame, rng, int(cfg.patch.N_patches), int(cfg.patch.size))
        frame['rays'], frame['near'], frame['far'] = frame['rays'][:, sel], frame['near'][sel], frame['far'][sel]
        keys = ['rays', 'near', 'far', 'bgcolor', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors',
                'cnl_bbox_min_xyz', 'cnl_bbox_max_xyz', 'cnl_bbox_scale_xyz', 'dst_posevec']
        data = {k: torch.from_numpy(np.ascontiguousarray(frame[k])).to(dev) for k in keys}
        with torch.no_grad():
            target = teacher(**data, iter_val=cfg.eval_iter)['rgb']
        opt.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=bool(tc['bf16'])):
            out = net(**data, iter_val=it)
            if use_lpips:
                loss = patch_image_loss(out['rgb'], target, patches, frame['bgcolor'] / 255., tc['lossweights'], lpips) \
                    + tc['lossweights'].get('comp', 1.0) * out['comp_loss'].float().mean()
            else:
                loss = tc['lossweights']['mse'] * torch.mean((out['rgb'].float() - target) ** 2) \
                    + tc['lossweights']['comp'] * out['comp_loss'].float().mean()
        loss.backward()
        opt.step(max_grad_norm=1.0)                                     # trainer.py:248-249: clip + Adam, one device pass
        decay = 0.1 ** (it / (tc['lrate_decay'] * 1000))                # exp_decay.py:7-19
        for grp in opt.param_groups:
            grp['lr'] = grp['base_lr'] * decay
        if it % int(tc['log_interval']) == 0 or it == 1:
            print(f'iter {it:5d}  loss {float(loss):.6f}  rays {len(sel)}  {time.time() - t0:.1f} s')
    torch.save({'iter': it, 'network': net.state_dict(), 'optimizer': opt.state_dict()},
               os.path.join(cfg.logdir, 'latest.tar'))
    print('saved', os.path.join(cfg.logdir, 'latest.tar'))


if __name__ == '__main__':
    main()
