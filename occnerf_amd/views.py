"""The cameras DERIVED from a prepared dataset: freeview, backview, allview and tpose (the reference's
core/data/occnerf/freeview.py, backview.py, allview.py, tpose.py).  None of them has a photograph to blend: a frame is a
camera, a box and the pose constants of a dataset frame (tpose: of the canonical subject).

`ViewFrames` yields what dataset.WholeFrames yields: host dicts with the leading batch dimension when iterated, and
`device_frames` -- (data, key, meta) triples built on the GPU (occnerf_gen_rays, occnerf_whole_frame_count, then
csrc/view.hip's rays-only row gather through ops.view_frame), one frame ahead of the render (dataset.CameraRaysAhead).

  freeview   frame `frame_idx` of the unskipped frame list seen from `render_frames` cameras on an orbit around the body's
             Th (freeview.py:133-142, :197-204); K, box, pose constants and photograph are that frame's;
  backview   every dataset frame (after skip / maxframes) seen from ONE camera: the first yielded frame's camera turned by
             angle index render_frames // 2 of period render_frames about the world origin (trans None), computed once
             together with its K (backview.py:203-211); each frame applies its own Rh / Th, box and pose;
  allview    frame `frame_idx` from the cameras of all_cameras.pkl ({frame: {'intrinsics' [C,3,3], 'extrinsics' [C,4,4]}});
             with all_mesh_infos.pkl the body (joints, poses, tpose_joints, Rh, Th) is indexed per camera too
             (allview.py:108-129, :204-215); 6 cameras when 'wild' is in the dataset path, else 23 (:69);
  tpose      the canonical subject only (canonical_joints.pkl): canonical box, zero pose, one frame, the float32 camera of
             synth.setup_camera(render_size) (tpose.py:50-84, :133-205); no photograph.

`truth_u8` (host dict and meta) is the resident uint8 photograph itself: the reference shows to_8b_image(img / 255.) as its
truth panel (freeview.py:187, :234), which maps each of the 256 grey levels to itself.  The resident photograph is the
PREPARED one: from_cfg opens the dataset with prepare_frames (dataset.py), so a frame whose camera has 'distortions' is
undistorted with that camera (freeview.py:156, backview.py:159); these loaders have no crop code, so nothing is cropped.
An allview rig with 'distortions' undistorts the RAW photograph of the source frame with rig camera idx's own K and D for
every output frame (allview.py:166-170): the raw photograph is kept, and the truth panel of frame idx is
undistort.undistort_u8 of it on the host, csrc/undistort.hip's on the device.
A dataset opened with resize_frames at a scale other than 1 renders at the training size, and its
truth panel -- built only under `show_truth` -- is dataset.truth_u8: to_8b_image of the Lanczos resize of the photograph."""
import os
import pickle

import numpy as np
import torch

from . import synth
from .undistort import undistort_u8
from .ahead import cuda_device
from .dataset import (CameraRaysAhead, PreparedDataset, Subject, apply_global_tfm_to_camera, host_frame, skeleton_to_bbox,
                      with_batch_dimension)

KINDS = ('freeview', 'backview', 'allview', 'tpose')
ROT_CAM_PARAMS = {'zju_mocap': {'rotate_axis': 'z', 'inv_angle': True},          # freeview.py:25-28
                  'wild': {'rotate_axis': 'y', 'inv_angle': False}}


def rotate_camera_by_frame_idx(extrinsics, frame_idx, trans=None, rotate_axis='y', period=196, inv_angle=False):
    """camera_util.py:85-110."""
    angle = 2 * np.pi * (frame_idx / period)
    return synth.rotate_camera(extrinsics, -angle if inv_angle else angle, trans=trans, rotate_axis=rotate_axis)


def src_type_of(cfg, data_type):
    """'zju_mocap' for the reference's zju_* dataset names, 'wild' for monocular_* (dataset_args.py:21,35,51); with only
    train.dataset_path, the key freeview.src_type."""
    if not dict(cfg.get('train', {}) or {}).get('dataset_path'):
        node = cfg.get('movement' if data_type == 'backview' else data_type, {})      # backview reads movement's directory
        name = node.get('dataset') if isinstance(node, dict) else None
        if isinstance(name, str) and name.startswith('zju_'):
            return 'zju_mocap'
        if isinstance(name, str) and name.startswith('monocular_'):
            return 'wild'
    return str(dict(cfg.get('freeview', {}) or {}).get('src_type', 'zju_mocap'))


class CanonicalSubject(Subject):
    """What tpose reads of a dataset directory: canonical_joints.pkl (dataset.Subject)."""

    def __init__(self, dataset_path, bbox_offset=0.3, volume_size=32):
        Subject.__init__(self, dataset_path, bbox_offset, volume_size)
        self.dataset, self.bbox_offset = self, float(bbox_offset)


class ViewFrames:
    """dataset: a PreparedDataset opened with skip 1 and all frames (tpose: a CanonicalSubject will do).  bgcolor in 0..255.
    src_type, render_frames, frame_idx: see the module docstring; render_size: tpose's image side; bbox_offset: the box
    margin of the bodies of all_mesh_infos.pkl (the dataset's own boxes are already built); skip / maxframes: backview's
    frame list, the reference's framelist[::skip][:maxframes].  truth: False leaves the truth panel of an allview rig with
    'distortions' out (it costs an undistortion per output frame); every other panel is the resident photograph and is
    always handed over."""

    def __init__(self, dataset, kind, bgcolor=(255., 255., 255.), src_type='zju_mocap', render_frames=100, frame_idx=0,
                 render_size=512, bbox_offset=0.3, skip=1, maxframes=-1, truth=True):
        if kind not in KINDS:
            raise ValueError(f"ViewFrames: kind '{kind}' is none of {KINDS}")
        if kind != 'tpose' and src_type not in ROT_CAM_PARAMS:
            raise ValueError(f"ViewFrames: src_type '{src_type}' is none of {tuple(ROT_CAM_PARAMS)}")
        self.dataset, self.kind, self.bgcolor = dataset, kind, np.array(bgcolor, dtype='float32')
        self.src_type, self.period, self.frame_idx = src_type, int(render_frames), int(frame_idx)
        self.truth, self._D, self._raw, self._raw_dev = bool(truth), None, None, None
        self._custom = {}                                  # the poses that are no dataset frame's
        self._uploaded, self._uploaded_to = {}, None       # ... on the device they were last asked for
        if kind == 'tpose':
            self.height = self.width = int(render_size)
            self.total_frames = 1
            K, E = synth.setup_camera(self.width)
            box = dataset.canonical_bbox
            pose = np.zeros(72, dtype='float32')
            dst_Rs, dst_Ts = synth.body_pose_to_body_RTs(pose, dataset.canonical_joints)
            self._views = [{'K': K, 'E': E, 'min': box['min_xyz'], 'max': box['max_xyz'], 'src': None, 'frame_name': 'tpose'}]
            self._custom[0] = {'dst_Rs': dst_Rs, 'dst_Ts': dst_Ts, 'dst_posevec': pose[3:] + 1e-2}
            return
        if not isinstance(dataset, PreparedDataset):
            raise TypeError(f'ViewFrames: {kind} needs a PreparedDataset')
        self.height, self.width = dataset.height, dataset.width
        if kind == 'backview':
            self._sel = list(range(len(dataset)))[::int(skip)]
            if int(maxframes) > 0:
                self._sel = self._sel[:int(maxframes)]
            self.total_frames = len(self._sel)
            self._reference = None
        else:
            if not 0 <= self.frame_idx < len(dataset):
                raise IndexError(f'freeview.frame_idx {self.frame_idx}: {dataset.dataset_path} has {len(dataset)} frames')
            self.total_frames = self.period
        if kind == 'allview':
            self._open_allview(float(bbox_offset))

    def _open_allview(self, bbox_offset):
        ds, path = self.dataset, os.path.join(self.dataset.dataset_path, 'all_cameras.pkl')
        self.total_frames = 6 if 'wild' in ds.dataset_path else 23
        if not os.path.isfile(path):
            raise FileNotFoundError(f'{path}: allview reads the cameras of the rig from all_cameras.pkl '
                                    "({frame: {'intrinsics' [C,3,3], 'extrinsics' [C,4,4]}}); the file is missing")
        with open(path, 'rb') as f:
            cams = pickle.load(f)
        name = ds.framelist[self.frame_idx]
        if name not in cams:
            raise KeyError(f'{path} has no cameras for frame {name}')
        self._K, self._E = np.asarray(cams[name]['intrinsics']), np.asarray(cams[name]['extrinsics'])
        if self._K.shape[0] < self.total_frames or self._E.shape[0] < self.total_frames:
            raise ValueError(f'{path}: frame {name} has {min(self._K.shape[0], self._E.shape[0])} cameras, allview renders '
                             f'{self.total_frames}')
        if 'distortions' in cams[name]:                    # allview.py:166-170: the raw photograph, rig camera idx's K and D
            from PIL import Image
            if ds.resize_img_scale != 1.0:
                raise NotImplementedError(f"{path}, frame {name}: the cameras have 'distortions' and resize_img_scale is "
                                          f'{ds.resize_img_scale}: prescaled PNGs no longer match the stored intrinsics, and '
                                          "resizing a rig's undistorted photograph (train.resize_frames) is not built")
            self._D = np.asarray(cams[name]['distortions'], dtype=np.float64)
            if self._D.shape[0] < self.total_frames:
                raise ValueError(f"{path}: frame {name} has {self._D.shape[0]} 'distortions', allview renders "
                                 f'{self.total_frames}')
            self._raw = np.ascontiguousarray(np.array(
                Image.open(os.path.join(ds.dataset_path, 'images', name + '.png')).convert('RGB')))
            if self._raw.shape != (ds.height, ds.width, 3):
                raise ValueError(f'{path}: the raw photograph of frame {name} is {self._raw.shape[1]} x {self._raw.shape[0]}, '
                                 f'the opened dataset has {ds.width} x {ds.height} (allview does not crop)')
        mesh = os.path.join(ds.dataset_path, 'all_mesh_infos.pkl')
        self._all_mesh = None
        if os.path.isfile(mesh):                           # has_all_mesh: the body is given per camera
            with open(mesh, 'rb') as f:
                info = pickle.load(f)[name]
            if info['joints'].shape[0] < self.total_frames:
                raise ValueError(f'{mesh}: frame {name} has {info["joints"].shape[0]} bodies, allview renders '
                                 f'{self.total_frames}')
            self._all_mesh = info
            for c in range(self.total_frames):
                poses = info['poses'].astype('float32')[c]
                dst_Rs, dst_Ts = synth.body_pose_to_body_RTs(poses, info['tpose_joints'].astype('float32')[c])
                self._custom[c] = {'dst_Rs': dst_Rs, 'dst_Ts': dst_Ts, 'dst_posevec': poses[3:] + 1e-2,
                                   'bbox': skeleton_to_bbox(info['joints'][c], bbox_offset)}

    @classmethod
    def from_cfg(cls, cfg, dataset_path, kind, prepare_device=None):
        """create_dataloader(kind) on a prepared directory.  The dataset is opened as PreparedDataset.from_cfg opens it
        (frames undistorted), without a crop: the reference's freeview / backview / allview loaders have no crop code.  The
        truth panel of a distorted allview rig is built only under `show_truth`.  prepare_device: the GPU that undistorts
        the frames at open (None: numpy on the host)."""
        common = dict(bgcolor=cfg.bgcolor, src_type=src_type_of(cfg, kind), render_frames=int(cfg.render_frames),
                      frame_idx=int(cfg.freeview.get('frame_idx', 0)), render_size=int(cfg.get('render_size', 512)),
                      bbox_offset=float(cfg.bbox_offset), truth=bool(cfg.get('show_truth', False)))
        if kind == 'tpose':
            return cls(CanonicalSubject(dataset_path, float(cfg.bbox_offset), int(cfg.mweight_volume.volume_size)), kind,
                       **common)
        return cls(PreparedDataset.from_cfg(cfg, dataset_path, device=None, skip=1, maxframes=-1, crop_image_scale=[-1, -1],
                                            prepare_device=prepare_device), kind, **common)

    def __len__(self):
        return self.total_frames

    def view(self, idx):
        """Camera, box and source frame of output frame idx: {'K', 'E', 'min', 'max', 'src', 'frame_name'}."""
        if not 0 <= idx < self.total_frames:
            raise IndexError(f'{self.kind} frame {idx} of {self.total_frames}')
        if self.kind == 'tpose':
            return self._views[0]
        ds = self.dataset
        if self.kind == 'backview':
            src = self._sel[idx]
            f = ds.frames[src]
            if self._reference is None:                    # once, from the first frame yielded (backview.py:203-211)
                first = ds.frames[self._sel[0]]
                self._reference = first['K'], rotate_camera_by_frame_idx(
                    first['extrinsics'], self.period // 2, trans=None, period=self.period, **ROT_CAM_PARAMS[self.src_type])
            K, E = self._reference
            Rh, Th = f['Rh_vec'], f['Th']
        else:
            src = self.frame_idx
            f = ds.frames[src]
            Rh, Th = f['Rh_vec'], f['Th']
            if self.kind == 'freeview':
                K = f['K']
                E = rotate_camera_by_frame_idx(f['extrinsics'], idx, trans=Th, period=self.total_frames,
                                               **ROT_CAM_PARAMS[self.src_type])
            else:
                K = self._K[idx, :3, :3].copy()
                K[:2] *= ds.resize_img_scale                # allview.py:221-222
                E = self._E[idx]
                if self._all_mesh is not None:
                    Rh, Th = self._all_mesh['Rh'].astype('float32')[idx], self._all_mesh['Th'].astype('float32')[idx]
        E = apply_global_tfm_to_camera(E, Rh, Th)
        box = self._custom[idx]['bbox'] if idx in self._custom else {'min_xyz': f['dst_bbox_min'], 'max_xyz': f['dst_bbox_max']}
        return {'K': K, 'E': E, 'min': box['min_xyz'], 'max': box['max_xyz'], 'src': src, 'frame_name': f['frame_name']}

    def frame(self, idx):
        """Output frame idx as the reference's dict, numpy on the host (freeview.py:177-269 and its siblings)."""
        v, H, W, ds = self.view(idx), self.height, self.width, self.dataset
        out = host_frame(v['frame_name'], H, W, v['K'], v['E'], v['min'], v['max'], self.bgcolor)
        if v['src'] is not None and self._D is None and ds.resizing:
            if self.truth:                                 # the photograph at the training size (dataset.truth_u8)
                out['truth_u8'] = ds.truth_u8(v['src'])
        elif v['src'] is not None and self._D is None:
            out['truth_u8'] = ds.images[v['src']]
        elif v['src'] is not None and self.truth:
            out['truth_u8'] = undistort_u8(self._raw, self._K[idx], self._D[idx])
        out.update(ds.constants(self._custom[idx]) if idx in self._custom else ds.host_constants(v['src']))
        return out

    def __iter__(self):
        for i in range(self.total_frames):
            yield with_batch_dimension(self.frame(i))

    def device_frames(self, device, prefetch=True, data_type=None):
        """The same frames built on the device, as the (data, key, meta) triples
        sequence.frames_to_device yields: `data` holds what Network.forward takes, as device tensors (the float[3] constants
        on the host); `meta` holds idx, ray_index, width, height, frame_name and, where the frame has a photograph, truth_u8:
        the resident uint8 image itself (a distorted allview rig: the raw photograph undistorted for the frame's camera).
        The scheme is WholeFrames.device_frames': with prefetch the rays, the box test and the row scan of frame t+1 run
        ahead of the consumer (dataset.CameraRaysAhead); prefetch=False enqueues everything on the current stream.  Both give identical tensors.  The ray-order key is None: the camera changes every frame.
        A frame without a ray raises ValueError."""
        from . import ops
        dev = cuda_device(device, 'ViewFrames.device_frames', 'iterate the loader for the host frames')
        ds = self.dataset.to_device(dev)                   # a CanonicalSubject uploads its two tensors, a dataset its frames
        H, W, n = self.height, self.width, self.total_frames
        ahead = CameraRaysAhead(dev, H, W, prefetch)
        if self._uploaded_to != dev:                       # once per device, kept over calls
            self._uploaded = {i: ds.upload_pose(pose, dev) for i, pose in self._custom.items()}
            self._raw_dev = None if self._raw is None else torch.from_numpy(self._raw).to(dev)
            self._uploaded_to = dev

        def start(i):
            v = self.view(i)
            return ahead.start(v, v['K'], v['E'], v['min'], v['max'])

        pending = start(0) if n else None
        for i in range(n):
            bufs, R, v = ahead.take(pending)
            out = ops.view_frame(bufs['rays8'], bufs['box'], H, W, row_start=bufs['row_start'], R=R)
            pending = start(i + 1) if i + 1 < n else None  # after the gather is enqueued, before the consumer renders
            data = {'rays': out['rays'], 'near': out['near'], 'far': out['far'], 'bgcolor': torch.from_numpy(self.bgcolor)}
            consts = ds.constants(self._uploaded[i], device=True) if i in self._custom else ds.device_constants(v['src'])
            data.update({k: (torch.from_numpy(c) if isinstance(c, np.ndarray) else c) for k, c in consts.items()})
            meta = {'idx': i, 'ray_index': out['ray_index'], 'width': W, 'height': H, 'frame_name': v['frame_name']}
            if v['src'] is not None and self._D is None and ds.resizing:
                if self.truth:                             # on the consumer's stream, like the gather
                    meta['truth_u8'] = ds.truth_u8_device(v['src'])
            elif v['src'] is not None and self._D is None:
                meta['truth_u8'] = ds._dev['image'][v['src']]
            elif v['src'] is not None and self.truth:      # on the consumer's stream, like the gather
                meta['truth_u8'] = ops.undistort_u8(self._raw_dev, None, self._K[i], self._D[i])[0]
            yield data, None, meta
