"""Training entry point with the reference's command line (train.py:48-49):

    python train.py --cfg configs/occnerf/synthetic/occnerf.yaml [train.maxiter 200 ...]

Scope: one optimisation step = Network.forward in
training mode through the differentiable path (occnerf_amd/train_path.py: torch autograd over
the HIP kNN and the HIP grid-encoder forward/backward) + MSE and completeness losses +
clip_grad_norm + Adam with the reference's per-group learning rates (optimizer.py:12-43) +
exponential decay (exp_decay.py:7-19).  Without a prepared dataset the supervision is a synthetic
teacher (the same network with a second seeded checkpoint) rendered through the HIP path.

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
ray-wise MSE against `target_rgbs` + comp.

The loop around the step is occnerf_amd/trainer.py's (the reference's trainer.py:58-63, :266-288): `init.tar` before the first
step, `latest.tar` every train.save_checkpt_interval and at the end, `iter_N.tar` every train.save_model_interval under
save_all, each in the reference's layout ({'iter','network','optimizer'}, trainer.py:398-406) with a `<name>.resume.tar`
sidecar beside it.  `resume True` continues from <load_net>.tar in the logdir (`latest` where load_net names the seeded
checkpoint).  On a prepared dataset the held-out `progress` frames are rendered into prog_NNNNNN.jpg and progress.jsonl at
iterations 20, 100, 300, 1000, 2500 and every progress.dump_interval (occnerf_amd/progress.py; 0 switches it off); the
synthetic subject has no photographs and gets no dump."""
import os

import numpy as np
import torch

from configs import cfg, args  # noqa: F401
from core.nets import create_network
from occnerf_amd import synth
from occnerf_amd.checkpoint import make_state_dict
from occnerf_amd.trainer import LR_GROUPS, TRAIN_DEFAULTS, Trainer, dataset_step_loss, make_optimizer  # noqa: F401


def patch_rays(frame, rng, n_patches=6, size=32):
    """6 random 32x32 pixel patches (default.yaml:147-150) restricted to rays that hit the bbox."""
    from occnerf_amd.seeded import patch_ray_selection
    return patch_ray_selection(frame, rng, n_patches, size)


def run_trainer(trainer, tc):
    """trainer.py:58-63 and the loop: resume or `init`, the steps up to train.maxiter, the final `latest`."""
    load_net = str(cfg.load_net)
    first = trainer.start(resume=bool(cfg.get('resume', False)), load_net='latest' if load_net.startswith('seeded') else load_net)
    trainer.run(first, int(tc['maxiter']))


def schedule_kwargs():
    return {'dump_interval': int(dict(cfg.get('progress', {}) or {}).get('dump_interval', 500)),
            'save_all': bool(cfg.get('save_all', True))}


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
    kw, progress = schedule_kwargs(), None
    if kw['dump_interval'] > 0:
        from occnerf_amd.progress import ProgressDump
        progress = ProgressDump(create_dataloader('progress'), cfg.logdir, device=dev)
    trainer = Trainer(net, opt, tc, cfg.logdir, next_batch=lambda it: next(loader),
                      loss_fn=lambda batch, it: dataset_step_loss(net, batch, it, tc, lpips),
                      describe=lambda batch: f"rays {batch['n_rows']}  frame {batch['frame_name']}  ",
                      loader=loader, progress=progress, **kw)
    run_trainer(trainer, tc)


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
    keys = ['rays', 'near', 'far', 'bgcolor', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors',
            'cnl_bbox_min_xyz', 'cnl_bbox_max_xyz', 'cnl_bbox_scale_xyz', 'dst_posevec']

    def next_batch(it):
        frame = synth.make_frame(img_size=size, pose72=synth.seeded_pose(100 + it % 16), orbit_frame=it % 50,
                                 orbit_period=50, bgcolor=cfg.bgcolor)
        patches = None
        if use_lpips:
            sel, pix = patch_ray_selection_map(frame, rng, int(cfg.patch.N_patches), int(cfg.patch.size))
            patches = PatchImages(pix, int(cfg.patch.N_patches), int(cfg.patch.size), dev)
        else:
            sel = patch_rays(frame, rng, int(cfg.patch.N_patches), int(cfg.patch.size))
        frame['rays'], frame['near'], frame['far'] = frame['rays'][:, sel], frame['near'][sel], frame['far'][sel]
        data = {k: torch.from_numpy(np.ascontiguousarray(frame[k])).to(dev) for k in keys}
        with torch.no_grad():
            target = teacher(**data, iter_val=cfg.eval_iter)['rgb']
        return {'data': data, 'target': target, 'patches': patches, 'bgcolor': frame['bgcolor'], 'n_rays': len(sel)}

    def loss_fn(batch, it):
        out = net(**batch['data'], iter_val=it)
        if use_lpips:
            return patch_image_loss(out['rgb'], batch['target'], batch['patches'], batch['bgcolor'] / 255., tc['lossweights'],
                                    lpips) + tc['lossweights'].get('comp', 1.0) * out['comp_loss'].float().mean()
        return tc['lossweights']['mse'] * torch.mean((out['rgb'].float() - batch['target']) ** 2) \
            + tc['lossweights']['comp'] * out['comp_loss'].float().mean()

    kw = schedule_kwargs()
    if kw['dump_interval'] > 0:
        print('synthetic subject: checkpoints and resume only; progress dumps need the photographs of a prepared dataset')
    trainer = Trainer(net, opt, tc, cfg.logdir, next_batch=next_batch, loss_fn=loss_fn,
                      describe=lambda batch: f"rays {batch['n_rays']}  ", host_rng=rng, **dict(kw, dump_interval=0))
    run_trainer(trainer, tc)


if __name__ == '__main__':
    main()
