"""The geometry the volume renderer sees: per pixel the ray parameter t = depth / alpha of the
composited depth, the surface point o + t d, a normal from the secants to the neighbouring pixels' points, and the depth /
normal / shaded panels as 8-bit images -- two HIP launches (csrc/gbuffer.hip) on the tensors rank 0 holds after the gather.

t is the ray PARAMETER, which the reference calls depth: its rays are not normalised, the metric distance is t |d|.  The
normals are in the space of the rays -- the body space of the frame's camera matrix E -- and are not rotated into the camera.
The numpy definition, tests/gbuffer_restatement.py, is the host function; everything here refuses host tensors."""
import numpy as np
import torch

from . import ops

PANELS = ops.GBUFFER_PANELS


def device_t_range(near, far):
    """The frame's default depth range (near.min(), far.max()) as a float32 [2] device tensor; nothing waits for it."""
    for name, v in (('near', near), ('far', far)):
        if not torch.is_tensor(v) or not v.is_cuda:
            raise RuntimeError(f'device_t_range: {name} must be a CUDA(HIP) tensor; there is no CPU path')
        if v.numel() == 0:
            raise RuntimeError(f'device_t_range: {name} is empty: a frame without a ray has no range')
    return torch.stack([near.float().amin(), far.float().amax()])


def geometry_maps(width, height, ray_index, rays, depth, alpha, min_alpha=0.5, t_range=None, bgcolor=(1.0, 1.0, 1.0),
                  panels=PANELS, near=None, far=None):
    """ray_index int64 [R] ascending flat pixels (nonzero(ray_mask)), rays float32 [2,R,3] in the caller's ray order, depth and
    alpha [R] (or [R,1]) as the renderer returns them, all on one GPU; bgcolor: cfg.bgcolor / 255 on the host.
    t_range: (t_lo, t_hi) of the depth panel -- two host numbers, a float32 [2] device tensor, or None: the frame's
    (near.min(), far.max()) from the `near` / `far` device tensors, reduced on the device.  Nothing synchronises.
    -> {'t' [H,W] float32 (a view of 'points' [H,W,4]: x, y, z, t), 'normal' [H,W,3] float32, 'valid' [H,W] uint8 (bit 0: t is
    valid, bit 1: the normal is), 't_range' float32 [2] or None, and the uint8 [H,W,3] panels named in `panels` under
    'depth_u8' / 'normal_u8' / 'shaded_u8'}, on the GPU."""
    for name, v in (('ray_index', ray_index), ('rays', rays), ('depth', depth), ('alpha', alpha)):
        if not torch.is_tensor(v) or not v.is_cuda:
            raise RuntimeError(f'geometry_maps: {name} must be a CUDA(HIP) tensor; tests/gbuffer_restatement.py is the host '
                               'function')
    dev = rays.device
    panels = tuple(panels)
    if t_range is None:
        if near is not None and far is not None:
            t_range = device_t_range(near, far)
        elif 'depth' in panels:
            raise RuntimeError('geometry_maps: the depth panel needs t_range, or the frame\'s near and far for the default')
    elif torch.is_tensor(t_range):
        if not t_range.is_cuda:
            raise RuntimeError('geometry_maps: a tensor t_range must be a CUDA(HIP) tensor (pass two numbers from the host)')
        t_range = t_range.to(torch.float32).reshape(-1).contiguous()
    else:
        lo, hi = (float(v) for v in t_range)
        t_range = torch.from_numpy(np.array([lo, hi], dtype=np.float32)).to(dev, non_blocking=True)
    points, valid, pix_ray = ops.gbuffer_points(ray_index, rays, depth.reshape(-1).contiguous(), alpha.reshape(-1).contiguous(),
                                            min_alpha, height, width)
    # launch 2 sets bit 1 in launch 1's valid bytes: one buffer
    normal, valid, imgs = ops.gbuffer_normals(points, pix_ray, rays, t_range, np.asarray(bgcolor, dtype=np.float32), panels,
                                              valid=valid)
    out = {'t': points[..., 3], 'points': points, 'normal': normal, 'valid': valid, 't_range': t_range}
    out.update({f'{k}_u8': v for k, v in imgs.items()})
    return out
