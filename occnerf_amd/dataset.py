"""Training on a prepared dataset directory (the reference's core/data/occnerf/train.py Dataset in patch mode).

`PreparedDataset` opens a directory in the reference's layout (cameras.pkl, mesh_infos.pkl, canonical_joints.pkl,
images/NAME.png, masks/NAME.png -- tools/make_synthetic_dataset.py writes one from a seed) and computes, once, everything
that is constant per frame; the PNGs go to the device once, as uint8.  `PatchBatchLoader` then builds every training batch
on the device (csrc/batch.hip through ops.patch_batch: four launches with the ray generation), one step ahead of the
optimiser on a side stream.  The reference builds the same batch in numpy inside two DataLoader workers
(create_dataset.py:67-72): blend of the whole image in float64, rays of every pixel, box test, one cumulative sum per patch.

What is NOT the reference's, each refused by name where it would matter:
  * a camera with 'distortions' (train.py:290-294 calls cv2.undistort);
  * crop_image_scale other than [-1, -1] (:300-304, :422-427);
  * upsample_pc (:384-385, needs trimesh and the SMPL faces);
  * resize_img_scale != 1 on PNGs that are not already at the training size.  The reference blends at full size and then
    resizes the float image with cv2's Lanczos filter and the mask with its bilinear one (:306-314); neither filter nor that
    order exists here, so nothing is resized: with `train.images_prescaled True` the PNGs are taken to BE the training images
    (resized by the user, any filter) and only K[:2] is scaled (:430); otherwise the scale is refused;
  * the 'verts' key (:381, :416): it needs an SMPL model and Network.forward does not read it.
"""
import os
import pickle

import numpy as np
import torch

from . import synth

WHOLE_FRAME_KEYS = ('rays', 'near', 'far', 'ray_mask', 'bgcolor', 'target_rgbs', 'ray_alpha')


def resolve_dataset_path(cfg, data_type='train'):
    """The directory `data_type` reads, or None for the synthetic frame source.  `train.dataset_path` wins (every data type
    of a run reads the directory the run trains on); otherwise the reference's dataset names as dataset_args.py:9-57 resolves
    them: zju_<subject>_train / _test -> dataset/zju_mocap/<subject>, monocular_train / _test -> dataset/wild/<cfg.subject>."""
    path = dict(cfg.get('train', {}) or {}).get('dataset_path')
    if path:
        return str(path)
    node = cfg.get(data_type, {})
    name = node.get('dataset') if isinstance(node, dict) else None
    if not isinstance(name, str):
        return None
    parts = name.split('_')
    if len(parts) == 3 and parts[0] == 'zju' and parts[2] in ('train', 'test'):
        return os.path.join('dataset', 'zju_mocap', parts[1])
    if name in ('monocular_train', 'monocular_test'):
        return os.path.join('dataset', 'wild', str(cfg.subject))
    raise NotImplementedError(f"dataset name '{name}' ({data_type}.dataset): only zju_<subject>_train/_test and "
                              "monocular_train/_test resolve to a directory (the reference's dataset_args.py)")


def apply_global_tfm_to_camera(E, Rh, Th):
    """camera_util.py:113-130: the camera seen from the body's own space."""
    g = np.eye(4)
    rot = synth.rodrigues_exact(Rh).T
    g[:3, :3] = rot
    g[:3, 3] = -rot.dot(Th)
    return E.dot(np.linalg.inv(g))


def occlusion_columns(occlusion, W):
    """The mask columns train.py:286-287 zeroes: [mid - width // 2, mid + width // 2) as a python slice of W columns."""
    mid, width = int(occlusion['mid']), int(occlusion['width'])
    return slice(mid - width // 2, mid + width // 2).indices(W)[:2]


def skeleton_to_bbox(skeleton, bbox_offset):
    return {'min_xyz': np.min(skeleton, axis=0) - bbox_offset, 'max_xyz': np.max(skeleton, axis=0) + bbox_offset}


def load_canonical(dataset_path, bbox_offset=0.3, volume_size=32):
    """What canonical_joints.pkl alone determines (train.py:96-113, :503-535), as the attributes PreparedDataset carries:
    canonical_joints, avg_betas, canonical_bbox, motion_weights_priors, cnl_gtfms and the three float32 box constants."""
    with open(os.path.join(dataset_path, 'canonical_joints.pkl'), 'rb') as f:
        cnl = pickle.load(f)
    joints = cnl['joints'].astype('float32')
    bbox = skeleton_to_bbox(joints, bbox_offset)
    mn, mx = bbox['min_xyz'].astype('float32'), bbox['max_xyz'].astype('float32')
    return {'canonical_joints': joints, 'avg_betas': cnl['avg_betas'].astype('float32'), 'canonical_bbox': bbox,
            'motion_weights_priors': synth.approx_gaussian_bone_volumes(
                joints, bbox['min_xyz'], bbox['max_xyz'], grid_size=int(volume_size)).astype('float32'),
            'cnl_gtfms': synth.get_canonical_global_tfms(joints),
            'cnl_bbox_min_xyz': mn, 'cnl_bbox_max_xyz': mx, 'cnl_bbox_scale_xyz': 2.0 / (mx - mn)}


class PreparedDataset:
    """A prepared directory, opened once.

    The frame list is the sorted PNG names, then [::skip], then [:maxframes] (train.py:68-75).  Per frame, on the host:
    the joints box +- bbox_offset (:115-133), K with K[:2] *= resize_img_scale (:430), E through apply_global_tfm_to_camera,
    dst_Rs / dst_Ts / cnl_gtfms / dst_posevec = poses[3:] + 1e-2 (:503-535); per subject the canonical box, its scale and
    motion_weights_priors.  The raw `extrinsics` and the axis-angle `Rh_vec` are kept too (views.py derives cameras from
    them).  Image and mask are uploaded as uint8 [H,W,3] each (6 bytes per pixel).

    The simulated occlusion (:286-287) zeroes the mask columns [mid - width//2, mid + width//2) of the frames whose POSITION
    in the frame list (not their frame number) is below occlusion.range when `occlude` is set; it is constant per frame, so
    it is applied here, at open.

    A frame whose mask sums to less than 255 after the band is left out of the epoch (`self.epoch_frames`).  This is the
    reference's `while np.sum(alpha) < 1` test (:395): the reference returns a RANDOM OTHER frame in its place (:396), so
    its epoch keeps its length and shows some frame twice; here the epoch is shorter instead.

    device=None keeps everything on the host (the host constants can be checked without a GPU)."""

    def __init__(self, dataset_path, device='cuda:0', skip=1, maxframes=-1, bbox_offset=0.3, volume_size=32,
                 resize_img_scale=1.0, images_prescaled=False, occlude=False, occlusion=None,
                 crop_image_scale=(-1, -1), upsample_pc=False):
        from PIL import Image
        self.dataset_path, self.device = dataset_path, None if device is None else torch.device(device)
        if not os.path.isdir(os.path.join(dataset_path, 'images')):
            raise FileNotFoundError(f'{dataset_path}: no images/ directory: not a prepared dataset')
        if list(crop_image_scale)[0] != -1:
            raise NotImplementedError(f'crop_image_scale={list(crop_image_scale)}: cropping (train.py:300-304) is not built; '
                                      'only [-1, -1]')
        if upsample_pc:
            raise NotImplementedError('upsample_pc: subdividing the SMPL mesh (train.py:384-385) needs trimesh and the SMPL '
                                      'faces; not built')
        scale = self.resize_img_scale = float(resize_img_scale)
        if scale != 1.0 and not images_prescaled:
            raise NotImplementedError(
                f'resize_img_scale={scale}: the reference resizes the blended image with cv2 (train.py:306-314), which is not '
                'available. Resize the PNGs yourself and set train.images_prescaled True (K is then scaled, the PNGs are '
                'not), or set resize_img_scale 1')

        def load(name):
            with open(os.path.join(dataset_path, name), 'rb') as f:
                return pickle.load(f)

        self.__dict__.update(load_canonical(dataset_path, bbox_offset, volume_size))
        cameras, mesh_infos = load('cameras.pkl'), load('mesh_infos.pkl')

        names = sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(dataset_path, 'images'))
                       if f.endswith('.png') and os.path.isfile(os.path.join(dataset_path, 'images', f)))
        names = names[::int(skip)]
        if int(maxframes) > 0:
            names = names[:int(maxframes)]
        if not names:
            raise FileNotFoundError(f'{dataset_path}/images holds no PNG')
        self.framelist, self.occlude = names, bool(occlude)
        self.frames, self.images, self.alphas = [], [], []
        for idx, name in enumerate(names):
            if name not in cameras:
                raise KeyError(f'{dataset_path}/cameras.pkl has no camera for frame {name}')
            if 'distortions' in cameras[name]:
                raise NotImplementedError(f"frame {name}: the camera has 'distortions'; undistorting the image "
                                          '(train.py:290-294, cv2.undistort) is not built. Undistort the PNGs and drop the key')
            img = np.array(Image.open(os.path.join(dataset_path, 'images', name + '.png')).convert('RGB'))
            alpha = np.array(Image.open(os.path.join(dataset_path, 'masks', name + '.png')).convert('RGB'))
            if alpha.shape != img.shape:
                raise ValueError(f'frame {name}: image is {img.shape}, mask is {alpha.shape}')
            if self.frames and img.shape[:2] != (self.height, self.width):
                raise ValueError(f'frame {name}: {img.shape[1]} x {img.shape[0]} pixels, the first frame has '
                                 f'{self.width} x {self.height}: one resident ray buffer serves every frame')
            self.height, self.width = int(img.shape[0]), int(img.shape[1])
            band = self.occlude and idx < int(occlusion['range'])
            if band:
                c0, c1 = occlusion_columns(occlusion, self.width)
                alpha[:, c0:c1] = 0
            info = mesh_infos[name]
            poses = info['poses'].astype('float32')
            joints = info['joints'].astype('float32')
            bbox = self.skeleton_to_bbox(info['joints'], bbox_offset)        # on the pickle's own dtype, as :130 does
            K = np.array(cameras[name]['intrinsics'])[:3, :3].copy()
            K[:2] *= scale
            Rh, Th = info['Rh'].astype('float32'), info['Th'].astype('float32')
            E = apply_global_tfm_to_camera(np.asarray(cameras[name]['extrinsics']), Rh, Th)
            dst_Rs, dst_Ts = synth.body_pose_to_body_RTs(poses, info['tpose_joints'].astype('float32'))
            self.frames.append({
                'frame_name': name, 'idx': int(name[-6:]), 'time': idx / len(names), 'band': band, 'K': K, 'E': E,
                'dst_bbox_min': bbox['min_xyz'], 'dst_bbox_max': bbox['max_xyz'], 'joints': joints, 'poses': poses,
                'betas': info['betas'].astype('float32'), 'Rh': synth.rodrigues_exact(Rh).astype(np.float32), 'Th': Th,
                'dst_Rs': dst_Rs, 'dst_Ts': dst_Ts, 'dst_posevec': poses[3:] + 1e-2,
                'empty': int(alpha.astype(np.int64).sum()) < 255,
                # what the derived cameras of views.py start from: the camera as calibrated and the body's axis-angle Rh
                'extrinsics': np.asarray(cameras[name]['extrinsics']), 'Rh_vec': Rh})
            self.images.append(np.ascontiguousarray(img))
            self.alphas.append(np.ascontiguousarray(alpha))
        self.epoch_frames = [i for i, f in enumerate(self.frames) if not f['empty']]
        if not self.epoch_frames:
            raise ValueError(f'{dataset_path}: every mask is empty (after the occlusion band)')
        self.dataset = self                          # run.py reads loader.dataset.avg_betas
        self._dev = None
        if self.device is not None:
            self.to_device(self.device)

    def to_device(self, device):
        """Upload the images, the masks (uint8 [H,W,3] each) and the per-frame constants; a second call for the same device
        is free.  -> self."""
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError(f'PreparedDataset.to_device: {dev} is not a GPU; the host arrays are self.images / self.alphas')
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        if self._dev is not None and self.device == dev:
            return self
        self.device = dev
        self._dev = {
            'image': [torch.from_numpy(a).to(dev) for a in self.images],
            'alpha': [torch.from_numpy(a).to(dev) for a in self.alphas],
            'frame': [{k: torch.from_numpy(np.ascontiguousarray(f[k])).to(dev) for k in ('dst_Rs', 'dst_Ts', 'dst_posevec')}
                      for f in self.frames],
            'cnl_gtfms': torch.from_numpy(self.cnl_gtfms).to(dev),
            'motion_weights_priors': torch.from_numpy(self.motion_weights_priors).to(dev)}
        return self

    skeleton_to_bbox = staticmethod(skeleton_to_bbox)

    @classmethod
    def from_cfg(cls, cfg, dataset_path, device='cuda:0', skip=1, maxframes=-1):
        tr = dict(cfg.get('train', {}) or {})
        return cls(dataset_path, device=device, skip=skip, maxframes=maxframes, bbox_offset=float(cfg.bbox_offset),
                   volume_size=int(cfg.mweight_volume.volume_size), resize_img_scale=float(cfg.resize_img_scale),
                   images_prescaled=bool(tr.get('images_prescaled', False)), occlude=cfg.get('occlude', False) is True,
                   occlusion=cfg.get('occlusion'), crop_image_scale=cfg.get('crop_image_scale', [-1, -1]),
                   upsample_pc=bool(cfg.get('upsample_pc', False)))

    def __len__(self):
        return len(self.framelist)

    def host_constants(self, i):
        """The reference's per-frame keys that do not depend on the draws (train.py:503-535), as numpy."""
        f = self.frames[i]
        return {'dst_Rs': f['dst_Rs'], 'dst_Ts': f['dst_Ts'], 'cnl_gtfms': self.cnl_gtfms,
                'motion_weights_priors': self.motion_weights_priors, 'cnl_bbox_min_xyz': self.cnl_bbox_min_xyz,
                'cnl_bbox_max_xyz': self.cnl_bbox_max_xyz, 'cnl_bbox_scale_xyz': self.cnl_bbox_scale_xyz,
                'dst_posevec': f['dst_posevec']}

    def device_constants(self, i):
        """The same on the device (uploaded at open); the three float[3] box constants stay on the host, the kernels take
        them by value."""
        d = dict(self._dev['frame'][i])
        d.update(cnl_gtfms=self._dev['cnl_gtfms'], motion_weights_priors=self._dev['motion_weights_priors'],
                 cnl_bbox_min_xyz=self.cnl_bbox_min_xyz, cnl_bbox_max_xyz=self.cnl_bbox_max_xyz,
                 cnl_bbox_scale_xyz=self.cnl_bbox_scale_xyz)
        return d

    def whole_frame(self, i, bgcolor):
        """Frame i as the reference's `ray_shoot_mode 'image'` dict (train.py:353-537 without the patch keys), numpy on the
        host: every ray that hits the box, with `target_rgbs` and `ray_alpha`."""
        f, H, W = self.frames[i], self.height, self.width
        bg = np.array(bgcolor, dtype='float32')
        alpha = self.alphas[i] / 255.
        img = alpha * self.images[i] + (1.0 - alpha) * bg[None, None, :]
        img = (img / 255.).astype('float32')
        rays_o, rays_d = synth.get_rays_from_KRT(H, W, f['K'], f['E'][:3, :3], f['E'][:3, 3])
        rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3).copy()
        near, far, ray_mask = synth.rays_intersect_3d_bbox({'min_xyz': f['dst_bbox_min'], 'max_xyz': f['dst_bbox_max']},
                                                           rays_o, rays_d)
        out = {'frame_name': f['frame_name'], 'img_width': W, 'img_height': H, 'ray_mask': ray_mask,
               'rays': np.stack([rays_o[ray_mask], rays_d[ray_mask]], 0).astype('float32'),
               'near': near[:, None].astype('float32'), 'far': far[:, None].astype('float32'), 'bgcolor': bg,
               'target_rgbs': img.reshape(-1, 3)[ray_mask], 'ray_alpha': alpha.reshape(-1, 3)[ray_mask]}
        out.update(self.host_constants(i))
        return out


class WholeFrames:
    """`movement` / `progress` on a prepared dataset: every frame as the whole-frame dict, with the leading batch dimension
    a DataLoader with batch_size 1 adds (run.py strips it)."""

    def __init__(self, dataset, bgcolor):
        self.dataset, self.bgcolor = dataset, bgcolor

    def __len__(self):
        return len(self.dataset)

    def __iter__(self):
        for i in range(len(self.dataset)):
            batch = {}
            for k, v in self.dataset.whole_frame(i, self.bgcolor).items():
                batch[k] = [v] if isinstance(v, str) else v if np.isscalar(v) else torch.as_tensor(np.asarray(v))[None]
            yield batch

    def device_frames(self, device, prefetch=True, data_type=None):
        """The same frames built on the device (csrc/frame.hip through ops.whole_frame), as the
        (data, key, meta) triples sequence.frames_to_device yields: `data` holds what Network.forward takes plus
        `target_rgbs` and `ray_alpha`, as device tensors (the float[3] constants on the host); `meta` holds idx, ray_index,
        width, height, frame_name, target_rgbs, ray_alpha and the maps truth_u8 / gt_vis / gt_alpha / body the metrics take.
        Images, masks and per-frame constants are uploaded on first use.

        prefetch=True: the rays, the box test and the row scan of frame t+1 run on a side stream, into the other of two
        buffer sets, while the consumer renders frame t; its ray count is copied to pinned memory behind an event.  The
        consumer waits on that event only, makes its stream wait for it and enqueues the gather there: the render stream is
        never synchronised.  prefetch=False enqueues everything on the current stream and reads the count with one blocking
        copy.  Both give identical tensors.  data_type 'movement' names the camera for the renderer's ray order, as
        frames_to_device does.  A frame without a ray raises ValueError."""
        from . import ops
        ds = self.dataset.to_device(device)
        dev, H, W, n = ds.device, ds.height, ds.width, len(ds)
        bg = np.array(self.bgcolor, dtype='float32')
        sets = [{'rays8': torch.empty(H * W, 8, device=dev, dtype=torch.float32),
                 'box': torch.empty(H * W, device=dev, dtype=torch.uint8),
                 'row_start': torch.empty(H + 1, device=dev, dtype=torch.int32),
                 'host': torch.empty(1, dtype=torch.int32).pin_memory(),
                 'event': torch.cuda.Event()} for _ in range(2 if prefetch else 1)]
        side = torch.cuda.Stream(device=dev) if prefetch else None

        def enqueue(i):
            """gen_rays, the count and the copy of R to pinned memory for frame i, on the current stream."""
            bufs, f = sets[i % len(sets)], ds.frames[i]
            ops.gen_rays(f['K'], f['E'], H, W, f['dst_bbox_min'], f['dst_bbox_max'], dev, out=(bufs['rays8'], bufs['box']))
            ops.whole_frame_count(bufs['box'], H, W, bufs['row_start'])
            bufs['host'].copy_(bufs['row_start'][H:], non_blocking=True)
            bufs['event'].record()
            return bufs

        def start(i):
            if side is None:
                return enqueue(i)
            # the buffer set was last read by the gather of frame i - 2, on the consumer's stream
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                return enqueue(i)

        pending = start(0) if n else None
        for i in range(n):
            bufs = pending
            bufs['event'].synchronize()
            torch.cuda.current_stream(dev).wait_event(bufs['event'])
            R = int(bufs['host'][0])
            name = ds.frames[i]['frame_name']
            if R == 0:
                raise ValueError(f'frame {name}: no ray of its camera hits the box around the body (the box misses the '
                                 f'{W} x {H} image); nothing to render')
            out = ops.whole_frame(ds._dev['image'][i], ds._dev['alpha'][i], bufs['rays8'], bufs['box'], bg,
                                  row_start=bufs['row_start'], R=R)
            body = bufs['box'].view(H, W).clone()              # the buffer set is rewritten two frames on
            pending = start(i + 1) if i + 1 < n else None
            data = {'rays': out['rays'], 'near': out['near'], 'far': out['far'], 'bgcolor': torch.from_numpy(bg),
                    'target_rgbs': out['target_rgbs'], 'ray_alpha': out['ray_alpha']}
            data.update({k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v)
                         for k, v in ds.device_constants(i).items()})
            meta = {'idx': i, 'ray_index': out['ray_index'], 'width': W, 'height': H, 'frame_name': name,
                    'target_rgbs': out['target_rgbs'], 'ray_alpha': out['ray_alpha'], 'truth_u8': out['truth_u8'],
                    'gt_vis': out['gt_vis'], 'gt_alpha': out['gt_alpha'], 'body': body}
            yield data, ('movement', R) if data_type == 'movement' else None, meta


class PatchBatchLoader:
    """The training batches of a PreparedDataset, built on the device.

    A seeded host RNG (numpy RandomState) draws, per epoch, the permutation of `dataset.epoch_frames`, and per batch the
    uniforms u[N,2] and -- when `bgcolor` is None, train.py:387-390 -- the background colour (rand(3) * 255 as float32).
    The draws are made in batch order whether or not batches are prefetched, so `prefetch` does not change a batch.

    prefetch=True: batch t+1 is enqueued on a side stream when batch t is handed out, into the other of two buffer sets; its
    row count and patch_div_indices are copied to pinned memory behind an event, and `next()` waits on that event only, then
    makes the current stream wait for it.  A batch's tensors are views of its buffer set, which the batch
    after the next overwrites: work enqueued on the current stream before the next `next()` reads them safely (the side
    stream waits for it), anything later must copy.  prefetch=False builds the batch in line on the current stream.

    Every batch is a dict with the keys Network.forward takes plus `target_rgbs`, `target_patches`, `patch_masks`,
    `patch_div_indices` (host int64), `xy_min`, `pix_of_row`, `row_of_pix`, `n_rows` (host int), `frame` (position in the
    frame list), `frame_name`, `bgcolor` (host float32, 0..255)."""

    def __init__(self, dataset, n_patches=6, size=32, sample_subject_ratio=0.8, bgcolor=None, seed=0, prefetch=True):
        from . import ops
        self._ops, self.dataset = ops, dataset
        self.n_patches, self.size, self.ratio = int(n_patches), int(size), float(sample_subject_ratio)
        if self.size > min(dataset.height, dataset.width):
            raise ValueError(f'patch.size {self.size} does not fit {dataset.width} x {dataset.height} frames')
        self.bgcolor = None if bgcolor is None else np.array(bgcolor, dtype='float32')
        self.rng, self.prefetch = np.random.RandomState(seed), bool(prefetch)
        self._sets, self._stream = None, None
        self._order, self._pending, self._turn = [], None, 0

    def _allocate(self):
        ds = self.dataset
        if ds.device is None:
            raise RuntimeError('PatchBatchLoader: the dataset was opened without a GPU (device=None); the batches are built '
                               'by HIP kernels, there is no CPU path')
        dev, H, W = ds.device, ds.height, ds.width
        self._sets = [{'out': self._ops.alloc_patch_batch(self.n_patches, self.size, H, dev),
                       'rays8': torch.empty(H * W, 8, device=dev, dtype=torch.float32),
                       'box': torch.empty(H * W, device=dev, dtype=torch.uint8),
                       'host': torch.empty(self.n_patches + 2, dtype=torch.int32).pin_memory(),
                       'event': torch.cuda.Event()} for _ in range(2 if self.prefetch else 1)]
        self._stream = torch.cuda.Stream(device=dev) if self.prefetch else None

    def __len__(self):
        return len(self.dataset.epoch_frames)

    def __iter__(self):
        return self

    def _draw(self):
        if not self._order:
            self._order = [self.dataset.epoch_frames[j] for j in self.rng.permutation(len(self.dataset.epoch_frames))]
        frame = self._order.pop(0)
        bg = (self.rng.rand(3) * 255.).astype('float32') if self.bgcolor is None else self.bgcolor
        return frame, self.rng.rand(self.n_patches, 2), bg

    def _enqueue(self, draw, bufs):
        """The four launches of one batch and the copy of its counts to pinned memory, on the current stream."""
        frame, u, bg = draw
        ds, f = self.dataset, self.dataset.frames[draw[0]]
        self._ops.gen_rays(f['K'], f['E'], ds.height, ds.width, f['dst_bbox_min'], f['dst_bbox_max'], ds.device,
                           out=(bufs['rays8'], bufs['box']))
        out = self._ops.patch_batch(ds._dev['image'][frame], ds._dev['alpha'][frame], bufs['rays8'], bufs['box'],
                                    self.n_patches, self.size, u, self.ratio, bg, out=bufs['out'])
        bufs['host'][:self.n_patches + 1].copy_(out['patch_div_indices'], non_blocking=True)
        bufs['host'][self.n_patches + 1:].copy_(out['n_rows'], non_blocking=True)
        bufs['event'].record()
        return draw, bufs

    def _start(self):
        if self._sets is None:
            self._allocate()
        bufs = self._sets[self._turn % len(self._sets)]
        self._turn += 1
        draw = self._draw()
        if self._stream is None:
            return self._enqueue(draw, bufs)
        # the buffer set was last read by the step before the previous one, on the consumer's stream
        self._stream.wait_stream(torch.cuda.current_stream(self.dataset.device))
        with torch.cuda.stream(self._stream):
            return self._enqueue(draw, bufs)

    def __next__(self):
        (frame, u, bg), bufs = self._pending if self._pending is not None else self._start()
        self._pending = None
        bufs['event'].synchronize()
        torch.cuda.current_stream(self.dataset.device).wait_event(bufs['event'])
        host = bufs['host'].numpy().astype(np.int64)
        R, out, ds = int(host[-1]), bufs['out'], self.dataset
        rays = out['rays'][:, :R]
        batch = {'rays': rays if rays.is_contiguous() else rays.contiguous(), 'near': out['near'][:R], 'far': out['far'][:R],
                 'bgcolor': bg, 'target_rgbs': out['target_rgbs'][:R], 'target_patches': out['target_patches'],
                 'patch_masks': out['patch_masks'], 'patch_div_indices': host[:-1].copy(), 'xy_min': out['xy_min'],
                 'pix_of_row': out['pix_of_row'][:R], 'row_of_pix': out['row_of_pix'], 'n_rows': R, 'frame': frame,
                 'frame_name': ds.frames[frame]['frame_name'], 'u': u}
        batch.update(ds.device_constants(frame))
        if self.prefetch:
            self._pending = self._start()
        return batch

    next = __next__


NETWORK_KEYS = ('rays', 'near', 'far', 'bgcolor', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors',
                'cnl_bbox_min_xyz', 'cnl_bbox_max_xyz', 'cnl_bbox_scale_xyz', 'dst_posevec')


def loader_from_cfg(cfg, dataset_path, device='cuda:0', seed=0, prefetch=True):
    """create_dataloader('train') on a prepared directory: bgcolor None (create_dataset.py:31: a random colour per batch)."""
    ds = PreparedDataset.from_cfg(cfg, dataset_path, device=device)
    return PatchBatchLoader(ds, n_patches=int(cfg.patch.N_patches), size=int(cfg.patch.size),
                            sample_subject_ratio=float(cfg.patch.sample_subject_ratio), bgcolor=None, seed=seed,
                            prefetch=prefetch)
