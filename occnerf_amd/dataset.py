"""Training on a prepared dataset directory (the reference's core/data/occnerf/train.py Dataset in patch mode).

`PreparedDataset` opens a directory in the reference's layout (cameras.pkl, mesh_infos.pkl, canonical_joints.pkl,
images/NAME.png, masks/NAME.png -- tools/make_synthetic_dataset.py writes one from a seed) and computes, once, everything
that is constant per frame; the PNGs go to the device once, as uint8.  `PatchBatchLoader` then builds every training batch
on the device (csrc/batch.hip through ops.patch_batch: four launches with the ray generation), one step ahead of the
optimiser (ahead.FrameAhead, which `WholeFrames.device_frames` and views.py use for their frames too).  The reference
builds the same batch in numpy inside two DataLoader workers (create_dataset.py:67-72): blend of the whole image in float64,
rays of every pixel, box test, one cumulative sum per patch.

Frames are PREPARED at open when `prepare_frames` is set (PreparedDataset.from_cfg sets it unless `train.prepare_frames False`
is configured), in the reference's order (train.py:286-304): the occlusion band on the raw mask, then image and mask
undistorted with the frame's own 'intrinsics' / 'distortions' (:290-294; undistort.undistort_u8 on the host,
csrc/undistort.hip through ops.undistort_u8 with a device -- DESIGN.md section 7f), then the crop_image_scale window
(:300-304, with K's principal point as :422-427 sets it).  A prepared photograph is again a uint8 photograph, so everything
downstream reads the 6-byte-per-pixel resident frame as before.  Without `prepare_frames` (the constructor's default) such
a dataset is refused by name.

What is NOT the reference's, each refused by name where it would matter:
  * upsample_pc (:384-385, needs trimesh and the SMPL faces);
  * resize_img_scale != 1 unless `resize_frames` (train.resize_frames True) or `images_prescaled` is set.  The reference
    blends at full size and then resizes the float image with cv2's Lanczos filter and the mask with its bilinear one
    (:306-314).  With resize_frames that is done here (resize.py on the host, csrc/resize.hip through ops.resize_frame on
    the device): the prepared full-size uint8 pair stays resident (`src_height` x `src_width`),
    `height` x `width` is the training size rint(H s) x rint(W s) of every ray buffer, and each batch or frame is resized
    with its own background colour into a float64 frame of the loader's buffer set, which the _f64 entries of the batch
    and frame builders read.  'distortions' and a crop are then legal with a scale: the full-size PNG still matches K.
    With `train.images_prescaled True` instead, the PNGs are taken to BE the training images (resized by the user, any
    filter) and only K[:2] is scaled (:430); prescaled PNGs no longer match the stored K, so 'distortions' or a crop
    together with a scale other than 1 are refused there.  With neither key the scale is refused;
  * 12 or 14 distortion coefficients (OpenCV's thin prism and tilt models) and a skewed camera matrix;
  * the 'verts' key (:381, :416): it needs an SMPL model and Network.forward does not read it.
"""
import os
import pickle

import numpy as np
import torch

from . import synth
from .undistort import undistort_u8
from . import resize
from .ahead import FrameAhead, cuda_device

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


def crop_window(crop, H, W):
    """The window (y0, x0, h, w) of train.py:300-304: img[mid_x - dx//2 : mid_x + (dx - dx//2), mid_y - dy//2 : mid_y +
    (dy - dy//2)] with mid_x, mid_y = H // 2, W // 2 and dx, dy = crop_image_scale -- dx counts rows.  A crop that does not
    lie inside the image is a ValueError (numpy would silently clip or wrap the slice)."""
    dx, dy = int(crop[0]), int(crop[1])
    y0, x0 = H // 2 - dx // 2, W // 2 - dy // 2
    if dx <= 0 or dy <= 0 or y0 < 0 or x0 < 0 or y0 + dx > H or x0 + dy > W:
        raise ValueError(f'crop_image_scale={[dx, dy]}: a crop of {dx} rows x {dy} columns does not lie inside the '
                         f'{W} x {H} image')
    return y0, x0, dx, dy


def skeleton_to_bbox(skeleton, bbox_offset):
    return {'min_xyz': np.min(skeleton, axis=0) - bbox_offset, 'max_xyz': np.max(skeleton, axis=0) + bbox_offset}


class Subject:
    """What canonical_joints.pkl alone determines (train.py:96-113, :503-535): canonical_joints, avg_betas, canonical_bbox,
    motion_weights_priors, cnl_gtfms and the three float32 box constants, on the host and -- after to_device -- on one
    GPU; and the per-frame constants every loader assembles from them and a pose."""

    def __init__(self, dataset_path, bbox_offset=0.3, volume_size=32):
        with open(os.path.join(dataset_path, 'canonical_joints.pkl'), 'rb') as f:
            cnl = pickle.load(f)
        joints = self.canonical_joints = cnl['joints'].astype('float32')
        bbox = self.canonical_bbox = skeleton_to_bbox(joints, bbox_offset)
        self.dataset_path, self.avg_betas = dataset_path, cnl['avg_betas'].astype('float32')
        self.motion_weights_priors = synth.approx_gaussian_bone_volumes(
            joints, bbox['min_xyz'], bbox['max_xyz'], grid_size=int(volume_size)).astype('float32')
        self.cnl_gtfms = synth.get_canonical_global_tfms(joints)
        self.cnl_bbox_min_xyz, self.cnl_bbox_max_xyz = bbox['min_xyz'].astype('float32'), bbox['max_xyz'].astype('float32')
        self.cnl_bbox_scale_xyz = 2.0 / (self.cnl_bbox_max_xyz - self.cnl_bbox_min_xyz)
        self.device, self._dev = None, None          # set by to_device

    def upload(self, dev):
        """What to_device keeps in self._dev."""
        return {'cnl_gtfms': torch.from_numpy(self.cnl_gtfms).to(dev),
                'motion_weights_priors': torch.from_numpy(self.motion_weights_priors).to(dev)}

    @staticmethod
    def upload_pose(pose, dev):
        return {k: torch.from_numpy(np.ascontiguousarray(pose[k])).to(dev) for k in ('dst_Rs', 'dst_Ts', 'dst_posevec')}

    def to_device(self, device):
        """Upload once per device; a second call for the same device is free.  -> self."""
        dev = cuda_device(device, type(self).__name__ + '.to_device', 'the host arrays are self.images / self.alphas')
        if self._dev is None or self.device != dev:
            self.device = dev
            self._dev = self.upload(dev)
        return self

    def constants(self, pose, device=False):
        """The reference's per-frame keys that do not depend on the draws (train.py:503-535) for the pose triple `pose`
        (dst_Rs, dst_Ts, dst_posevec): numpy on the host, or with device=True the tensors to_device and upload_pose made;
        the three float[3] box constants stay on the host, the kernels take them by value."""
        gtfms, priors = self.cnl_gtfms, self.motion_weights_priors
        if device:
            gtfms, priors = self._dev['cnl_gtfms'], self._dev['motion_weights_priors']
        return {'dst_Rs': pose['dst_Rs'], 'dst_Ts': pose['dst_Ts'], 'cnl_gtfms': gtfms,
                'motion_weights_priors': priors, 'cnl_bbox_min_xyz': self.cnl_bbox_min_xyz,
                'cnl_bbox_max_xyz': self.cnl_bbox_max_xyz, 'cnl_bbox_scale_xyz': self.cnl_bbox_scale_xyz,
                'dst_posevec': pose['dst_posevec']}


def host_frame(frame_name, H, W, K, E, box_min, box_max, bgcolor):
    """What every host frame dict starts with: the rays of an H x W camera that hit the box, as the reference carries them
    (ray_mask [H*W], rays [2,R,3], near and far [R,1], float32), under the frame's name and size."""
    rays_o, rays_d = synth.get_rays_from_KRT(H, W, K, E[:3, :3], E[:3, 3])
    rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3).copy()
    near, far, ray_mask = synth.rays_intersect_3d_bbox({'min_xyz': box_min, 'max_xyz': box_max}, rays_o, rays_d)
    return {'frame_name': frame_name, 'img_width': W, 'img_height': H, 'ray_mask': ray_mask,
            'rays': np.stack([rays_o[ray_mask], rays_d[ray_mask]], 0).astype('float32'),
            'near': near[:, None].astype('float32'), 'far': far[:, None].astype('float32'), 'bgcolor': bgcolor}


def with_batch_dimension(frame):
    """A host frame dict with the leading batch dimension a DataLoader with batch_size 1 adds (run.py strips it)."""
    return {k: [v] if isinstance(v, str) else v if np.isscalar(v) else torch.as_tensor(np.asarray(v))[None]
            for k, v in frame.items()}


class CameraRaysAhead:
    """What WholeFrames.device_frames and ViewFrames.device_frames build ahead (ahead.FrameAhead): the ray of every pixel of
    an H x W camera and its box test (ops.gen_rays), the hits above every image row (ops.whole_frame_count) and, on the
    host, their total R.  A buffer set is rays8 [H*W,8], box [H*W] and row_start [H+1]."""

    def __init__(self, device, H, W, prefetch, extra=None):
        """extra: a callable -> further tensors of every buffer set (a resized float frame), for start's `also`."""
        from . import ops
        self._ops, self.H, self.W = ops, H, W
        self._ahead = FrameAhead(device, lambda: dict({
            'rays8': torch.empty(H * W, 8, device=device, dtype=torch.float32),
            'box': torch.empty(H * W, device=device, dtype=torch.uint8),
            'row_start': torch.empty(H + 1, device=device, dtype=torch.int32)}, **(extra() if extra else {})),
            host_words=1, prefetch=prefetch)

    def start(self, item, K, E, box_min, box_max, also=None):
        """also(bufs): more work for the same buffer set, enqueued ahead with the rays."""
        def enqueue(bufs, _item):
            if also is not None:
                also(bufs)
            self._ops.gen_rays(K, E, self.H, self.W, box_min, box_max, self._ahead.device, out=(bufs['rays8'], bufs['box']))
            self._ops.whole_frame_count(bufs['box'], self.H, self.W, bufs['row_start'])
            return bufs['row_start'][self.H:]
        return self._ahead.start(item, enqueue)

    def take(self, ticket):
        """-> the buffer set, R and start's `item`, a dict with 'frame_name'.  A frame without a ray raises ValueError."""
        bufs, host, item = self._ahead.take(ticket)
        R = int(host[0])
        if R == 0:
            raise ValueError(f"frame {item['frame_name']}: no ray of its camera hits the box around the body (the box misses "
                             f'the {self.W} x {self.H} image); nothing to render')
        return bufs, R, item


class PreparedDataset(Subject):
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

    prepare_frames=True undistorts and crops every frame at open (the module docstring): a camera with 'distortions' and
    a crop_image_scale other than [-1, -1] are then opened instead of refused; `height`, `width`, `empty` and K are those of
    the prepared frame.  With a `device` the kernel does the work and the prepared pair is copied back once per frame, so
    `self.images` / `self.alphas` (whole_frame(), views.py) hold prepared frames on either route, identical ones.
    prepare_device: the GPU that prepares the frames of a dataset that itself stays on the host (device=None).

    resize_frames=True with a resize_img_scale other than 1 resizes every batch and frame to the training size `height` x
    `width` = rint(src_height s) x rint(src_width s) (the module docstring): `self.images` /
    `self.alphas` stay the prepared full-size pair, `empty` is the reference's test on the resized mask (its float64 sum
    below 1), and the tap tables are built once (`self.resize_tables`) and uploaded with the frames.  At scale 1 the key
    changes nothing; together with images_prescaled it is a ValueError.

    device=None keeps everything on the host (the host constants can be checked without a GPU)."""

    def __init__(self, dataset_path, device='cuda:0', skip=1, maxframes=-1, bbox_offset=0.3, volume_size=32,
                 resize_img_scale=1.0, images_prescaled=False, occlude=False, occlusion=None,
                 crop_image_scale=(-1, -1), upsample_pc=False, prepare_frames=False, prepare_device=None,
                 resize_frames=False):
        from PIL import Image
        if not os.path.isdir(os.path.join(dataset_path, 'images')):
            raise FileNotFoundError(f'{dataset_path}: no images/ directory: not a prepared dataset')
        crop = None if list(crop_image_scale)[0] == -1 else tuple(int(v) for v in crop_image_scale)
        if crop is not None and not prepare_frames:
            raise NotImplementedError(f'crop_image_scale={list(crop_image_scale)}: cropping (train.py:300-304) is not built; '
                                      'only [-1, -1]')
        if upsample_pc:
            raise NotImplementedError('upsample_pc: subdividing the SMPL mesh (train.py:384-385) needs trimesh and the SMPL '
                                      'faces; not built')
        scale = self.resize_img_scale = float(resize_img_scale)
        if resize_frames and images_prescaled:
            raise ValueError('resize_frames together with images_prescaled: the PNGs are either resized here '
                             '(train.resize_frames) or already at the training size (train.images_prescaled), not both')
        resizing = self.resizing = bool(resize_frames) and scale != 1.0      # scale 1: nothing is resized (train.py:306)
        if scale != 1.0 and not images_prescaled and not resizing:
            raise NotImplementedError(
                f'resize_img_scale={scale}: frames are resized (train.py:306-314) only when asked to. Set train.resize_frames '
                'True (the blend is resized with the Lanczos filter, the mask with the bilinear one), or resize the PNGs '
                'yourself and set train.images_prescaled True (K is then scaled, the PNGs are not), or set resize_img_scale 1')
        if scale != 1.0 and crop is not None and not resizing:
            raise NotImplementedError(f'crop_image_scale={list(crop)} with resize_img_scale={scale}: the crop (train.py:300-304) '
                                      'is in pixels of the full-size image, which prescaled PNGs no longer are')
        if prepare_device is None:
            prepare_device = device
        if prepare_frames and prepare_device is not None:
            prepare_device = cuda_device(prepare_device, 'PreparedDataset', 'device=None prepares the frames on the host')

        def load(name):
            with open(os.path.join(dataset_path, name), 'rb') as f:
                return pickle.load(f)

        Subject.__init__(self, dataset_path, bbox_offset, volume_size)
        self.dataset = self                          # run.py reads loader.dataset.avg_betas
        cameras, mesh_infos = load('cameras.pkl'), load('mesh_infos.pkl')

        names = sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(dataset_path, 'images'))
                       if f.endswith('.png') and os.path.isfile(os.path.join(dataset_path, 'images', f)))
        names = names[::int(skip)]
        if int(maxframes) > 0:
            names = names[:int(maxframes)]
        if not names:
            raise FileNotFoundError(f'{dataset_path}/images holds no PNG')
        self.framelist, self.occlude = names, bool(occlude)
        self.frames, self.images, self.alphas, raw_size, self.resize_tables = [], [], [], None, None
        for idx, name in enumerate(names):
            if name not in cameras:
                raise KeyError(f'{dataset_path}/cameras.pkl has no camera for frame {name}')
            distorted = 'distortions' in cameras[name]
            if distorted and not prepare_frames:
                raise NotImplementedError(f"frame {name}: the camera has 'distortions'; undistorting the image "
                                          '(train.py:290-294, cv2.undistort) is not built. Undistort the PNGs and drop the key')
            if distorted and scale != 1.0 and not resizing:
                raise NotImplementedError(f"frame {name}: the camera has 'distortions' and resize_img_scale is {scale}: "
                                          'prescaled PNGs no longer match the stored intrinsics, so they cannot be undistorted')
            img = np.array(Image.open(os.path.join(dataset_path, 'images', name + '.png')).convert('RGB'))
            alpha = np.array(Image.open(os.path.join(dataset_path, 'masks', name + '.png')).convert('RGB'))
            if alpha.shape != img.shape:
                raise ValueError(f'frame {name}: image is {img.shape}, mask is {alpha.shape}')
            if self.frames and img.shape[:2] != raw_size:
                raise ValueError(f'frame {name}: {img.shape[1]} x {img.shape[0]} pixels, the first frame has '
                                 f'{raw_size[1]} x {raw_size[0]}: one resident ray buffer serves every frame')
            raw_size = img.shape[:2]
            band = self.occlude and idx < int(occlusion['range'])
            if band:                                 # on the raw mask, before it is undistorted (:286-287, then :290-294)
                c0, c1 = occlusion_columns(occlusion, raw_size[1])
                alpha[:, c0:c1] = 0
            window = None if crop is None else crop_window(crop, *raw_size)
            if distorted:
                img, alpha = self._undistorted(img, alpha, cameras[name], window, prepare_device)
            elif window is not None:
                y0, x0, h, w = window
                img, alpha = img[y0:y0 + h, x0:x0 + w], alpha[y0:y0 + h, x0:x0 + w]
            self.src_height, self.src_width = int(img.shape[0]), int(img.shape[1])
            self.height, self.width = self.src_height, self.src_width
            empty = int(alpha.astype(np.int64).sum()) < 255
            if resizing:                             # the training size; `empty` is the reference's test on the resized mask
                if self.resize_tables is None:
                    self.resize_tables = resize.frame_tables(self.src_height, self.src_width, scale)
                self.height, self.width = self.resize_tables['size']
                empty = bool(np.sum(resize.resize_blend(None, alpha, None, scale, self.resize_tables)[1]) < 1)
            info = mesh_infos[name]
            poses = info['poses'].astype('float32')
            joints = info['joints'].astype('float32')
            bbox = self.skeleton_to_bbox(info['joints'], bbox_offset)        # on the pickle's own dtype, as :130 does
            K = np.array(cameras[name]['intrinsics'])[:3, :3].copy()
            if crop is not None:
                # :422-427 to the letter: dx is the crop's ROW extent (img[mid_x - dx//2 : ...] slices rows) and yet it sets
                # cx, the principal point's COLUMN; dy, the column extent, sets cy.  The original principal point is dropped.
                K[0, 2], K[1, 2] = crop[0] / 2, crop[1] / 2
            K[:2] *= scale
            Rh, Th = info['Rh'].astype('float32'), info['Th'].astype('float32')
            E = apply_global_tfm_to_camera(np.asarray(cameras[name]['extrinsics']), Rh, Th)
            dst_Rs, dst_Ts = synth.body_pose_to_body_RTs(poses, info['tpose_joints'].astype('float32'))
            self.frames.append({
                'frame_name': name, 'idx': int(name[-6:]), 'time': idx / len(names), 'band': band, 'K': K, 'E': E,
                'dst_bbox_min': bbox['min_xyz'], 'dst_bbox_max': bbox['max_xyz'], 'joints': joints, 'poses': poses,
                'betas': info['betas'].astype('float32'), 'Rh': synth.rodrigues_exact(Rh).astype(np.float32), 'Th': Th,
                'dst_Rs': dst_Rs, 'dst_Ts': dst_Ts, 'dst_posevec': poses[3:] + 1e-2,
                'empty': empty,
                # what the derived cameras of views.py start from: the camera as calibrated and the body's axis-angle Rh
                'extrinsics': np.asarray(cameras[name]['extrinsics']), 'Rh_vec': Rh})
            self.images.append(np.ascontiguousarray(img))
            self.alphas.append(np.ascontiguousarray(alpha))
        self.epoch_frames = [i for i, f in enumerate(self.frames) if not f['empty']]
        if not self.epoch_frames:
            raise ValueError(f'{dataset_path}: every mask is empty (after the occlusion band)')
        if device is not None:
            self.to_device(device)

    @staticmethod
    def _undistorted(img, alpha, cam, window, device):
        """Image and (banded) mask of one frame undistorted with the frame's own camera, the window only: numpy on the host,
        or with a device one launch on it and one copy back."""
        K, D = cam['intrinsics'], cam['distortions']
        if device is None:
            return undistort_u8(img, K, D, window), undistort_u8(alpha, K, D, window)
        from . import ops
        pair = ops.undistort_u8(torch.from_numpy(np.ascontiguousarray(img)).to(device),
                                torch.from_numpy(np.ascontiguousarray(alpha)).to(device), K, D, window)
        return pair[0].cpu().numpy(), pair[1].cpu().numpy()

    def upload(self, dev):
        """The images, the masks (uint8 [H,W,3] each) and the per-frame constants, with the subject's."""
        from . import ops
        return dict(Subject.upload(self, dev),
                    resize=ops.upload_resize_tables(self.resize_tables, dev) if self.resizing else None,
                    image=[torch.from_numpy(a).to(dev) for a in self.images],
                    alpha=[torch.from_numpy(a).to(dev) for a in self.alphas],
                    frame=[self.upload_pose(f, dev) for f in self.frames])

    skeleton_to_bbox = staticmethod(skeleton_to_bbox)

    @classmethod
    def from_cfg(cls, cfg, dataset_path, device='cuda:0', skip=1, maxframes=-1, crop_image_scale=None, prepare_device=None):
        """The dataset as the configuration describes it; frames are prepared (undistorted, cropped) unless
        `train.prepare_frames False`.  crop_image_scale: in the place of the configured one (views.py: [-1, -1]);
        prepare_device: as the constructor's."""
        tr = dict(cfg.get('train', {}) or {})
        crop = cfg.get('crop_image_scale', [-1, -1]) if crop_image_scale is None else crop_image_scale
        return cls(dataset_path, device=device, skip=skip, maxframes=maxframes, bbox_offset=float(cfg.bbox_offset),
                   volume_size=int(cfg.mweight_volume.volume_size), resize_img_scale=float(cfg.resize_img_scale),
                   images_prescaled=bool(tr.get('images_prescaled', False)), occlude=cfg.get('occlude', False) is True,
                   occlusion=cfg.get('occlusion'), crop_image_scale=crop,
                   upsample_pc=bool(cfg.get('upsample_pc', False)), prepare_frames=bool(tr.get('prepare_frames', True)),
                   prepare_device=prepare_device, resize_frames=bool(tr.get('resize_frames', False)))

    def __len__(self):
        return len(self.framelist)

    def host_constants(self, i):
        """Subject.constants for frame i, as numpy."""
        return self.constants(self.frames[i])

    def device_constants(self, i):
        """The same on the device (uploaded by to_device)."""
        return self.constants(self._dev['frame'][i], device=True)

    def resized_frame(self, i, bgcolor):
        """(img64, alpha64) of frame i at the training size, numpy on the host (resize.resize_blend): the blend over
        `bgcolor`, not divided by 255, and the mask / 255."""
        if not self.resizing:
            raise RuntimeError('resized_frame: the dataset was opened without resize_frames (or at scale 1)')
        return resize.resize_blend(self.images[i], self.alphas[i], bgcolor, self.resize_img_scale, self.resize_tables)

    def truth_u8(self, i):
        """The photograph of frame i as the truth panel of views.py shows it, uint8 [height, width, 3]: the resident image,
        or with resize_frames the Lanczos resize of the photograph itself (the blend under a full mask is the photograph,
        exactly) through to_8b_image: uint8(255.f * clip(float32(img64 / 255.), 0, 1))."""
        if not self.resizing:
            return self.images[i]
        full = np.full_like(self.images[i], 255)
        img64 = resize.resize_blend(self.images[i], full, [0., 0., 0.], self.resize_img_scale, self.resize_tables)[0]
        return (np.float32(255.) * np.clip((img64 / 255.).astype('float32'), 0., 1.)).astype(np.uint8)

    def truth_u8_device(self, i):
        """truth_u8 on the device the dataset was uploaded to (ops.resize_frame, then the panel's few elementwise steps), on
        the current stream; identical to the host's."""
        if not self.resizing:
            return self._dev['image'][i]
        from . import ops
        if self._dev.get('full_mask') is None:
            self._dev['full_mask'] = torch.full_like(self._dev['image'][i], 255)
        img64 = ops.resize_frame(self._dev['image'][i], self._dev['full_mask'], self._dev['resize'], [0., 0., 0.])[0]
        return (img64 / 255.).float().clamp_(0., 1.).mul_(255.).to(torch.uint8)

    def gt_alpha(self, i):
        """float32 [height, width]: channel 0 of frame i's mask at the training size, as the metrics take it."""
        if self.resizing:
            return resize.resize_blend(None, self.alphas[i], None, self.resize_img_scale, self.resize_tables)[1][:, :, 0] \
                .astype('float32')
        return (self.alphas[i][:, :, 0] / 255.).astype('float32')

    def whole_frame(self, i, bgcolor):
        """Frame i as the reference's `ray_shoot_mode 'image'` dict (train.py:353-537 without the patch keys), numpy on the
        host: every ray that hits the box, with `target_rgbs` and `ray_alpha`."""
        f, H, W = self.frames[i], self.height, self.width
        bg = np.array(bgcolor, dtype='float32')
        if self.resizing:
            img, alpha = self.resized_frame(i, bg)
        else:
            alpha = self.alphas[i] / 255.
            img = alpha * self.images[i] + (1.0 - alpha) * bg[None, None, :]
        img = (img / 255.).astype('float32')
        out = host_frame(f['frame_name'], H, W, f['K'], f['E'], f['dst_bbox_min'], f['dst_bbox_max'], bg)
        out.update(target_rgbs=img.reshape(-1, 3)[out['ray_mask']], ray_alpha=alpha.reshape(-1, 3)[out['ray_mask']])
        out.update(self.host_constants(i))
        return out


class WholeFrames:
    """`movement` / `progress` on a prepared dataset: every frame as the whole-frame dict (with_batch_dimension)."""

    def __init__(self, dataset, bgcolor):
        self.dataset, self.bgcolor = dataset, bgcolor

    def __len__(self):
        return len(self.dataset)

    def __iter__(self):
        for i in range(len(self.dataset)):
            yield with_batch_dimension(self.dataset.whole_frame(i, self.bgcolor))

    def device_frames(self, device, prefetch=True, data_type=None):
        """The same frames built on the device (csrc/frame.hip through ops.whole_frame), as the
        (data, key, meta) triples sequence.frames_to_device yields: `data` holds what Network.forward takes plus
        `target_rgbs` and `ray_alpha`, as device tensors (the float[3] constants on the host); `meta` holds idx, ray_index,
        width, height, frame_name, target_rgbs, ray_alpha and the maps truth_u8 / gt_vis / gt_alpha / body the metrics take.
        Images, masks and per-frame constants are uploaded on first use.

        prefetch=True: the rays, the box test and the row scan of frame t+1 run ahead of the consumer, who renders frame
        t (CameraRaysAhead); the gather is enqueued on the consumer's stream, which is never synchronised.  prefetch=False
        enqueues everything on the current stream and reads the count with one blocking copy.  Both give identical
        tensors.  data_type 'movement' names the camera for the renderer's ray order, as frames_to_device does.  A frame
        without a ray raises ValueError."""
        from . import ops
        ds = self.dataset.to_device(device)
        H, W, n = ds.height, ds.width, len(ds)
        bg = np.array(self.bgcolor, dtype='float32')
        extra = None
        if ds.resizing:                                        # the float frame of every buffer set, resized ahead
            extra = lambda: dict(zip(('img64', 'alpha64'), ops.alloc_resize_frame(H, W, ds.device)))      # noqa: E731
        ahead = CameraRaysAhead(ds.device, H, W, prefetch, extra)

        def start(i):
            f, also = ds.frames[i], None
            if ds.resizing:
                def also(bufs):
                    ops.resize_frame(ds._dev['image'][i], ds._dev['alpha'][i], ds._dev['resize'], bg,
                                     out=(bufs['img64'], bufs['alpha64']))
            return ahead.start(f, f['K'], f['E'], f['dst_bbox_min'], f['dst_bbox_max'], also)

        pending = start(0) if n else None
        for i in range(n):
            bufs, R, f = ahead.take(pending)
            if ds.resizing:
                out = ops.whole_frame_f64(bufs['img64'], bufs['alpha64'], bufs['rays8'], bufs['box'], bg,
                                          row_start=bufs['row_start'], R=R)
            else:
                out = ops.whole_frame(ds._dev['image'][i], ds._dev['alpha'][i], bufs['rays8'], bufs['box'], bg,
                                      row_start=bufs['row_start'], R=R)
            body = bufs['box'].view(H, W).clone()              # the buffer set is rewritten two frames on
            pending = start(i + 1) if i + 1 < n else None      # after the gather is enqueued, before the consumer renders
            data = {'rays': out['rays'], 'near': out['near'], 'far': out['far'], 'bgcolor': torch.from_numpy(bg),
                    'target_rgbs': out['target_rgbs'], 'ray_alpha': out['ray_alpha']}
            data.update({k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v)
                         for k, v in ds.device_constants(i).items()})
            meta = {'idx': i, 'ray_index': out['ray_index'], 'width': W, 'height': H, 'frame_name': f['frame_name'],
                    'target_rgbs': out['target_rgbs'], 'ray_alpha': out['ray_alpha'], 'truth_u8': out['truth_u8'],
                    'gt_vis': out['gt_vis'], 'gt_alpha': out['gt_alpha'], 'body': body}
            yield data, ('movement', R) if data_type == 'movement' else None, meta


def pack_random_state(rng):
    """numpy RandomState -> plain tensors and numbers (the trainer's resume sidecar loads without unpickling numpy objects)."""
    kind, key, pos, has_gauss, cached = rng.get_state()
    return {'kind': str(kind), 'key': torch.from_numpy(np.asarray(key, dtype=np.int64).copy()), 'pos': int(pos),
            'has_gauss': int(has_gauss), 'cached_gaussian': float(cached)}


def unpack_random_state(rng, st):
    rng.set_state((st['kind'], st['key'].numpy().astype(np.uint32), int(st['pos']), int(st['has_gauss']),
                   float(st['cached_gaussian'])))


class PatchBatchLoader:
    """The training batches of a PreparedDataset, built on the device.

    A seeded host RNG (numpy RandomState) draws, per epoch, the permutation of `dataset.epoch_frames`, and per batch the
    uniforms u[N,2] and -- when `bgcolor` is None, train.py:387-390 -- the background colour (rand(3) * 255 as float32).
    The draws are made in batch order whether or not batches are prefetched, so `prefetch` does not change a batch.

    prefetch=True: batch t+1 is built ahead (ahead.FrameAhead) when batch t is handed out; its row count and
    patch_div_indices come back through pinned memory.  A batch's tensors are views of its buffer set, which the batch
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
        self._ahead, self._order, self._pending, self._before_draw = None, [], None, None

    def __len__(self):
        return len(self.dataset.epoch_frames)

    def __iter__(self):
        return self

    def _draw(self):
        self._before_draw = (self.rng.get_state(), list(self._order))
        if not self._order:
            self._order = [self.dataset.epoch_frames[j] for j in self.rng.permutation(len(self.dataset.epoch_frames))]
        frame = self._order.pop(0)
        bg = (self.rng.rand(3) * 255.).astype('float32') if self.bgcolor is None else self.bgcolor
        return frame, self.rng.rand(self.n_patches, 2), bg

    def state(self):
        """The host generator and the rest of the epoch as of the NEXT batch this loader hands out: with a batch built ahead,
        the state before its draws, so that a loader restored from it (load_state) draws that batch again and none twice.
        Plain tensors and numbers (the trainer's resume sidecar, occnerf_amd/trainer.py)."""
        if self._pending is not None:
            rng = np.random.RandomState()
            rng.set_state(self._before_draw[0])
            return dict(pack_random_state(rng), order=[int(i) for i in self._before_draw[1]])
        return dict(pack_random_state(self.rng), order=[int(i) for i in self._order])

    def load_state(self, st):
        """Continue from state(): a batch that was built ahead is dropped, its draws are made again."""
        self._drop_pending()
        unpack_random_state(self.rng, st)
        self._order = [int(i) for i in st['order']]

    def reseed(self, seed):
        """A fresh stream and a fresh epoch (a resume that has no recorded state)."""
        self._drop_pending()
        self.rng.seed(int(seed))
        self._order = []

    def _drop_pending(self):
        """Take the batch that is being built ahead and discard it: the next start() then finds no build in flight in the
        buffer set it rotates onto."""
        if self._pending is not None:
            self._ahead.take(self._pending)
            self._pending = None

    def _enqueue(self, bufs, draw):
        """The four launches of one batch on the current stream -> what the host reads: patch_div_indices, the row count."""
        frame, u, bg = draw
        ds, f = self.dataset, self.dataset.frames[draw[0]]
        self._ops.gen_rays(f['K'], f['E'], ds.height, ds.width, f['dst_bbox_min'], f['dst_bbox_max'], ds.device,
                           out=(bufs['rays8'], bufs['box']))
        if ds.resizing:                                # the batch's own background colour: resized per batch (section 7g)
            self._ops.resize_frame(ds._dev['image'][frame], ds._dev['alpha'][frame], ds._dev['resize'], bg,
                                   out=(bufs['img64'], bufs['alpha64']))
            out = self._ops.patch_batch_f64(bufs['img64'], bufs['alpha64'], bufs['rays8'], bufs['box'],
                                            self.n_patches, self.size, u, self.ratio, bg, out=bufs['out'])
        else:
            out = self._ops.patch_batch(ds._dev['image'][frame], ds._dev['alpha'][frame], bufs['rays8'], bufs['box'],
                                        self.n_patches, self.size, u, self.ratio, bg, out=bufs['out'])
        return out['patch_div_indices'], out['n_rows']

    def _start(self):
        ds = self.dataset
        if ds.device is None:
            raise RuntimeError('PatchBatchLoader: the dataset was opened without a GPU (device=None); the batches are built '
                               'by HIP kernels, there is no CPU path')
        if self._ahead is None:                        # the buffers are allocated by the first next()
            dev, H, W = ds.device, ds.height, ds.width
            def buffers():
                bufs = {'out': self._ops.alloc_patch_batch(self.n_patches, self.size, H, dev),
                        'rays8': torch.empty(H * W, 8, device=dev, dtype=torch.float32),
                        'box': torch.empty(H * W, device=dev, dtype=torch.uint8)}
                if ds.resizing:                        # the resized float frame: 48 bytes per training pixel
                    bufs['img64'], bufs['alpha64'] = self._ops.alloc_resize_frame(H, W, dev)
                return bufs
            self._ahead = FrameAhead(dev, buffers, host_words=self.n_patches + 2, prefetch=self.prefetch)
        return self._ahead.start(self._draw(), self._enqueue)

    def __next__(self):
        ticket = self._pending if self._pending is not None else self._start()
        self._pending = None
        bufs, host, (frame, u, bg) = self._ahead.take(ticket)
        host = host.numpy().astype(np.int64)
        R, out, ds = int(host[-1]), bufs['out'], self.dataset
        rays = out['rays'][:, :R]
        batch = {'rays': rays if rays.is_contiguous() else rays.contiguous(), 'near': out['near'][:R], 'far': out['far'][:R],
                 'bgcolor': bg, 'target_rgbs': out['target_rgbs'][:R], 'target_patches': out['target_patches'],
                 'patch_masks': out['patch_masks'], 'patch_div_indices': host[:-1].copy(), 'xy_min': out['xy_min'],
                 'pix_of_row': out['pix_of_row'][:R], 'row_of_pix': out['row_of_pix'], 'n_rows': R, 'frame': frame,
                 'frame_name': ds.frames[frame]['frame_name'], 'u': u}
        batch.update(ds.device_constants(frame))
        if self.prefetch:
            self._pending = self._start()              # before the batch is handed out: the consumer's step is not yet enqueued
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
