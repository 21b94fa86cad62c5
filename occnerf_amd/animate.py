"""Driving a trained subject with a motion it has not seen (run.py --type animate; the reference has no
such entry point).  A motion is a sequence of poses -- another capture's prepared directory (only its mesh_infos.pkl is read)
or an .npz with `poses` and optionally `Rh` / `Th`; only the pose is taken from it.  The skeleton is the subject's own: the
tpose_joints of the subject's dataset frame `animate.frame_idx`, the SOURCE frame, whose calibrated camera also shoots
the sequence; the canonical constants are those of dataset.Subject.

  read_motion      the two sources, refused by name when they are not a motion;
  align_motion     the one rigid map that puts the motion's frame 0 where the source frame stands;
  resample_motion  `substeps` frames per interval: quaternion slerp of the joints and Rh along the shorter arc, Th linear;
  AnimateFrames    every pose as a frame -- pose constants, box, camera -- yielding what views.ViewFrames yields: host dicts when
                   iterated, `device_frames` triples built one frame ahead (dataset.CameraRaysAhead, ops.view_frame).

All of it is vectorised numpy on the host, float64 inside and float32 axis-angle out, which is what a dataset's poses are; the
per-frame constants come from the functions PreparedDataset uses for its own frames (synth.body_pose_to_body_RTs,
synth.posed_joints, dataset.skeleton_to_bbox, dataset.apply_global_tfm_to_camera)."""
import json
import os
import pickle

import numpy as np
import torch

from . import synth
from .ahead import cuda_device
from .dataset import (CameraRaysAhead, PreparedDataset, apply_global_tfm_to_camera, host_frame, skeleton_to_bbox,
                      with_batch_dimension)
from .views import ROT_CAM_PARAMS, rotate_camera_by_frame_idx, src_type_of

CAMERAS = ('fixed', 'follow', 'orbit')


# ------------------------------------------------------------------ reading
def _checked(name, a, shape_tail, T, path):
    """`a` as float32 [T] + shape_tail, refused by name when it cannot be that."""
    try:
        a = np.asarray(a)
        if a.dtype == object or a.dtype.kind not in 'fiu':
            raise TypeError(f'dtype {a.dtype}')
        a = a.astype(np.float64)
    except (TypeError, ValueError) as e:
        raise TypeError(f"animate.motion {path}: '{name}' cannot be cast to float ({e})") from None
    if T is None:
        T = a.shape[0] if a.ndim else -1
    if a.shape != (T,) + shape_tail and not (name == 'poses' and a.shape == (T, 24, 3)):
        raise ValueError(f"animate.motion {path}: '{name}' has shape {a.shape}, expected {('T',) + shape_tail}"
                         + (' or (T, 24, 3)' if name == 'poses' else f' with T = {T}'))
    a = a.reshape((T,) + shape_tail)
    if T == 0:
        raise ValueError(f'animate.motion {path}: the motion has no frame (T == 0)')
    if not np.isfinite(a).all():
        raise ValueError(f"animate.motion {path}: '{name}' holds non-finite values")
    return a.astype(np.float32)


def read_motion(path):
    """-> {'path', 'kind' ('dataset' | 'npz'), 'poses' float32 [T,72], 'Rh' float32 [T,3], 'Th' float32 [T,3] or None (the
    source frame's Th then serves every frame)}.  A prepared dataset directory: its mesh_infos.pkl alone, frames in
    sorted name order; betas, joints and tpose_joints are never read.  An .npz: poses [T,72] or [T,24,3], optionally Rh and
    Th; without Rh the root rotation poses[:, :3] becomes Rh and is zeroed in poses."""
    path = str(path)
    if not os.path.exists(path):
        raise FileNotFoundError(f"animate.motion '{path}' does not exist (a prepared dataset directory or an .npz file)")
    if os.path.isdir(path):
        pkl = os.path.join(path, 'mesh_infos.pkl')
        if not os.path.isfile(pkl):
            raise FileNotFoundError(f'animate.motion {path}: the directory has no mesh_infos.pkl: not a prepared dataset')
        with open(pkl, 'rb') as f:
            infos = pickle.load(f)
        names = sorted(infos)
        if not names:
            raise ValueError(f'animate.motion {path}: the motion has no frame (T == 0)')
        for k in ('poses', 'Rh', 'Th'):
            missing = [n for n in names if k not in infos[n]]
            if missing:
                raise KeyError(f"animate.motion {pkl}: frame {missing[0]} has no '{k}'")
        cols = {k: [np.asarray(infos[n][k]).reshape(-1) for n in names] for k in ('poses', 'Rh', 'Th')}
        for k, size in (('poses', 72), ('Rh', 3), ('Th', 3)):
            bad = [n for n, a in zip(names, cols[k]) if a.size != size]
            if bad:
                raise ValueError(f"animate.motion {pkl}: '{k}' of frame {bad[0]} has {cols[k][names.index(bad[0])].size} "
                                 f'values, expected {size}')
        out = {'kind': 'dataset'}
        raw = {k: np.stack(v) for k, v in cols.items()}
    elif path.endswith('.npz'):
        try:
            with np.load(path, allow_pickle=False) as z:
                raw = {k: z[k] for k in ('poses', 'Rh', 'Th') if k in z.files}
        except ValueError as e:                            # an object array: numpy will not unpickle it
            raise TypeError(f'animate.motion {path}: an array cannot be cast to float ({e})') from None
        if 'poses' not in raw:
            raise KeyError(f"animate.motion {path}: the archive has no 'poses' ([T,72] or [T,24,3])")
        out = {'kind': 'npz'}
    else:
        raise ValueError(f"animate.motion '{path}' is neither a directory nor an .npz file")
    poses = _checked('poses', raw['poses'], (72,), None, path)
    T = poses.shape[0]
    if 'Rh' in raw:
        Rh = _checked('Rh', raw['Rh'], (3,), T, path)
    else:                                                  # the split both of the reference's preparation tools make
        Rh = poses[:, :3].copy()
        poses = poses.copy()
        poses[:, :3] = 0
    Th = _checked('Th', raw['Th'], (3,), T, path) if 'Th' in raw else None
    return dict(out, path=path, poses=poses, Rh=Rh, Th=Th)


# ------------------------------------------------------------------ rotations, float64
def quat_of_axis_angle(v):
    """Axis-angle [...,3] -> unit quaternion [...,4] (w, x, y, z), float64; an exactly zero rotation is (1, 0, 0, 0)."""
    v = np.asarray(v, dtype=np.float64)
    theta = np.sqrt((v * v).sum(-1, keepdims=True))
    small = theta < 1e-12
    scale = np.where(small, 0.5, np.sin(0.5 * theta) / np.where(small, 1.0, theta))      # sin(t / 2) / t -> 1 / 2
    return np.concatenate([np.where(small, 1.0, np.cos(0.5 * theta)), scale * v], -1)


def axis_angle_of_quat(q):
    """Unit quaternion [...,4] -> axis-angle [...,3] of an angle in [0, pi], float64 (q and -q give the same vector)."""
    q = np.asarray(q, dtype=np.float64)
    q = np.where(q[..., :1] < 0.0, -q, q)
    s = np.sqrt((q[..., 1:] * q[..., 1:]).sum(-1, keepdims=True))
    angle = 2.0 * np.arctan2(s, q[..., :1])
    small = s < 1e-300
    return np.where(small, 2.0 * q[..., 1:], q[..., 1:] * (angle / np.where(small, 1.0, s)))


def quat_of_matrix(R):
    """Rotation matrices [...,3,3] -> unit quaternions [...,4], by the largest of the four squared components."""
    R = np.asarray(R, dtype=np.float64)
    m = lambda i, j: R[..., i, j]       # noqa: E731
    four = np.stack([1.0 + m(0, 0) + m(1, 1) + m(2, 2), 1.0 + m(0, 0) - m(1, 1) - m(2, 2),
                     1.0 - m(0, 0) + m(1, 1) - m(2, 2), 1.0 - m(0, 0) - m(1, 1) + m(2, 2)], -1)
    cand = np.stack([
        np.stack([four[..., 0], m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)], -1),
        np.stack([m(2, 1) - m(1, 2), four[..., 1], m(0, 1) + m(1, 0), m(0, 2) + m(2, 0)], -1),
        np.stack([m(0, 2) - m(2, 0), m(0, 1) + m(1, 0), four[..., 2], m(1, 2) + m(2, 1)], -1),
        np.stack([m(1, 0) - m(0, 1), m(0, 2) + m(2, 0), m(1, 2) + m(2, 1), four[..., 3]], -1)], -2)
    pick = np.argmax(four, -1)
    q = np.take_along_axis(cand, pick[..., None, None], -2)[..., 0, :]
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def axis_angle_of_matrix(R):
    return axis_angle_of_quat(quat_of_matrix(R))


def slerp(q0, q1, u):
    """Unit quaternions q0, q1 [...,4] at the fractions u (broadcast against [...,1]) along the SHORTER arc: q1 and -q1 are
    the same rotation, the one nearer to q0 is taken.  The angle between them is 2 atan2(|q1 - q0|, |q1 + q0|), exact for
    small and for large angles alike; below 1e-12 rad the weights are those of the chord."""
    q0, q1 = np.asarray(q0, dtype=np.float64), np.asarray(q1, dtype=np.float64)
    q1 = np.where((q0 * q1).sum(-1, keepdims=True) < 0.0, -q1, q1)
    diff, summ = q1 - q0, q1 + q0
    omega = 2.0 * np.arctan2(np.sqrt((diff * diff).sum(-1, keepdims=True)), np.sqrt((summ * summ).sum(-1, keepdims=True)))
    small = omega < 1e-12
    den = np.where(small, 1.0, np.sin(omega))
    w0 = np.where(small, 1.0 - u, np.sin((1.0 - u) * omega) / den)
    w1 = np.where(small, u, np.sin(u * omega) / den)
    q = w0 * q0 + w1 * q1
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


# ------------------------------------------------------------------ into the subject's world, and resampling
def align_motion(Rh, Th, Rh_src, Th_src):
    """R'_t = R_src R_0^T R_t and Th'_t = Th_src + R_src R_0^T (Th_t - Th_0), R = rodrigues_exact(Rh): the rigid map that puts
    the motion's frame 0 where the source frame stands.  -> (Rh' float32 [T,3] axis-angle, Th' float32 [T,3])."""
    R = np.stack([synth.rodrigues_exact(r) for r in np.asarray(Rh)])
    M = synth.rodrigues_exact(Rh_src).dot(R[0].T)
    Th64, src64 = np.asarray(Th, dtype=np.float64), np.asarray(Th_src, dtype=np.float64)
    return (axis_angle_of_matrix(np.matmul(M, R)).astype(np.float32),
            (src64 + (Th64 - Th64[0]).dot(M.T)).astype(np.float32))


def _same_bytes(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all(-1, keepdims=True)


def resample_motion(poses, Rh, Th, substeps):
    """`substeps` n frames per interval of the motion: (T - 1) n + 1 frames.  poses float32 [T,72], Rh and Th float32 [T,3] ->
    (poses', Rh', Th' float32, key int64 [T',2] the keyframe pair of every output frame, u float64 [T'] its fraction between
    them).  Joints and Rh: quaternion slerp along the shorter arc in float64, written back as float32 axis-angle; Th linear.
    Keyframes are copied (n == 1: the inputs themselves), and a joint whose two keyframes have identical bytes keeps them in
    every in-between."""
    n = int(substeps)
    if n < 1:
        raise ValueError(f'animate.substeps = {substeps}: at least 1 (1 takes the motion as it is)')
    T = poses.shape[0]
    last = max(T - 1, 0)
    if n == 1 or T == 1:
        idx = np.arange(T, dtype=np.int64)
        return poses, Rh, Th, np.stack([idx, np.minimum(idx + 1, last)], 1), np.zeros(T)
    rot = np.concatenate([poses.reshape(T, 24, 3), Rh[:, None]], 1)                      # [T,25,3] float32
    u = (np.arange(1, n, dtype=np.float64) / n)[None, :, None, None]                     # [1,n-1,1,1]
    q = quat_of_axis_angle(rot)
    mid = axis_angle_of_quat(slerp(q[:-1, None], q[1:, None], u)).astype(np.float32)     # [T-1,n-1,25,3]
    mid = np.where(_same_bytes(rot[:-1], rot[1:])[:, None], rot[:-1, None], mid)
    th64 = Th.astype(np.float64)
    th_mid = (th64[:-1, None] + u[..., 0] * (th64[1:, None] - th64[:-1, None])).astype(np.float32)
    th_mid = np.where(_same_bytes(Th[:-1], Th[1:])[:, None], Th[:-1, None], th_mid)
    out_rot = np.concatenate([np.concatenate([rot[:-1, None], mid], 1).reshape((T - 1) * n, 25, 3), rot[-1:]], 0)
    out_th = np.concatenate([np.concatenate([Th[:-1, None], th_mid], 1).reshape((T - 1) * n, 3), Th[-1:]], 0)
    idx = np.arange((T - 1) * n + 1, dtype=np.int64)
    k0 = idx // n
    return (np.ascontiguousarray(out_rot[:, :24].reshape(-1, 72)), np.ascontiguousarray(out_rot[:, 24]), out_th,
            np.stack([k0, np.minimum(k0 + 1, last)], 1), (idx % n) / n)


# ------------------------------------------------------------------ the frame source
class AnimateFrames:
    """The frames of a motion on a subject.  dataset: the subject's PreparedDataset, opened with skip 1 and all frames (as
    views.ViewFrames takes it); motion: read_motion's dict; bgcolor in 0..255.  frame_idx: the source frame; substeps, align,
    camera: the module docstring and DESIGN.md section 7l; src_type and render_frames: the orbit of camera 'orbit', turned as
    freeview turns its camera, one turn in render_frames frames.

    Everything per frame is computed here, once, on the host (about 2 ms per frame): `poses`, `Rh`, `Th`, `key`, `u` of the
    resampled motion and `frames`, a list of {'K', 'E', 'min', 'max', 'frame_name', 'joints', 'src', dst_Rs, dst_Ts,
    dst_posevec}.  There is no photograph: no frame carries truth_u8."""

    def __init__(self, dataset, motion, bgcolor=(255., 255., 255.), frame_idx=0, substeps=1, align=True, camera='fixed',
                 src_type='zju_mocap', render_frames=100, bbox_offset=0.3):
        if not isinstance(dataset, PreparedDataset):
            raise TypeError('AnimateFrames: the subject must be a PreparedDataset')
        if camera not in CAMERAS:
            raise ValueError(f"animate.camera '{camera}' is none of {CAMERAS}")
        if camera == 'orbit' and src_type not in ROT_CAM_PARAMS:
            raise ValueError(f"AnimateFrames: src_type '{src_type}' is none of {tuple(ROT_CAM_PARAMS)}")
        if int(substeps) < 1:
            raise ValueError(f'animate.substeps = {substeps}: at least 1 (1 takes the motion as it is)')
        if not 0 <= int(frame_idx) < len(dataset):
            raise IndexError(f'animate.frame_idx {frame_idx}: {dataset.dataset_path} has {len(dataset)} frames')
        self.dataset, self.motion, self.bgcolor = dataset, motion, np.array(bgcolor, dtype='float32')
        self.frame_idx, self.substeps, self.align, self.camera = int(frame_idx), int(substeps), bool(align), camera
        self.height, self.width = dataset.height, dataset.width
        src = dataset.frames[self.frame_idx]
        with open(os.path.join(dataset.dataset_path, 'mesh_infos.pkl'), 'rb') as f:      # the subject's own skeleton
            tpose_joints = pickle.load(f)[src['frame_name']]['tpose_joints'].astype('float32')
        Rh_src, Th_src = src['Rh_vec'], src['Th']
        poses, Rh, Th = motion['poses'], motion['Rh'], motion['Th']
        if Th is None:
            Th = np.repeat(Th_src[None], poses.shape[0], 0)
        if self.align:
            Rh, Th = align_motion(Rh, Th, Rh_src, Th_src)
        self.poses, self.Rh, self.Th, self.key, self.u = resample_motion(poses, Rh, Th, self.substeps)
        self.total_frames = self.poses.shape[0]
        self.frames = []
        for t in range(self.total_frames):
            p = self.poses[t]
            dst_Rs, dst_Ts = synth.body_pose_to_body_RTs(p, tpose_joints)
            joints = synth.posed_joints(p, tpose_joints)
            box = skeleton_to_bbox(joints, float(bbox_offset))
            E_world = src['extrinsics']
            if camera == 'orbit':
                E_world = rotate_camera_by_frame_idx(E_world, t, trans=Th_src, period=int(render_frames),
                                                     **ROT_CAM_PARAMS[src_type])
            E = apply_global_tfm_to_camera(E_world, self.Rh[t], self.Th[t] if camera == 'fixed' else Th_src)
            self.frames.append({'K': src['K'], 'E': E, 'min': box['min_xyz'], 'max': box['max_xyz'], 'src': None,
                                'frame_name': f'animate_{t:06d}', 'joints': joints,
                                'dst_Rs': dst_Rs, 'dst_Ts': dst_Ts, 'dst_posevec': p[3:] + 1e-2})
        self._uploaded, self._uploaded_to = None, None     # the pose constants on the device they were last asked for

    @classmethod
    def from_cfg(cls, cfg, dataset_path, prepare_device=None):
        """create_dataloader('animate') on the prepared directory `movement` would read.  The motion is read and checked
        first: nothing of the subject is opened, let alone uploaded, for a motion that is refused."""
        node = cfg.get('animate') or {}
        if not node.get('motion'):
            raise ValueError('--type animate needs animate.motion PATH: a prepared dataset directory or an .npz with poses '
                             '[T,72]')
        if int(node.get('substeps', 1)) < 1:
            raise ValueError(f"animate.substeps = {node.get('substeps')}: at least 1 (1 takes the motion as it is)")
        if str(node.get('camera', 'fixed')) not in CAMERAS:
            raise ValueError(f"animate.camera '{node.get('camera')}' is none of {CAMERAS}")
        motion = read_motion(node['motion'])
        dataset = PreparedDataset.from_cfg(cfg, dataset_path, device=None, skip=1, maxframes=-1, crop_image_scale=[-1, -1],
                                           prepare_device=prepare_device)
        return cls(dataset, motion, bgcolor=cfg.bgcolor, frame_idx=int(node.get('frame_idx', 0)),
                   substeps=int(node.get('substeps', 1)), align=bool(node.get('align', True)),
                   camera=str(node.get('camera', 'fixed')), src_type=src_type_of(cfg, 'movement'),
                   render_frames=int(cfg.render_frames), bbox_offset=float(cfg.bbox_offset))

    def __len__(self):
        return self.total_frames

    def view(self, idx):
        """Camera, box, pose constants and body-space joints of output frame idx."""
        if not 0 <= idx < self.total_frames:
            raise IndexError(f'animate frame {idx} of {self.total_frames}')
        return self.frames[idx]

    def frame(self, idx):
        """Output frame idx as the reference's dict, numpy on the host, with the camera that made its rays."""
        v, ds = self.view(idx), self.dataset
        out = host_frame(v['frame_name'], self.height, self.width, v['K'], v['E'], v['min'], v['max'], self.bgcolor)
        out.update(ds.constants(v), camera_K=v['K'], camera_E=v['E'])
        return out

    def __iter__(self):
        for i in range(self.total_frames):
            yield with_batch_dimension(self.frame(i))

    def device_frames(self, device, prefetch=True, data_type=None):
        """The same frames built on the device, as ViewFrames.device_frames builds its own: (data, None, meta) triples, the
        rays, the box test and the row scan of frame t+1 ahead of the consumer with prefetch, identical tensors without.
        `meta` holds idx, ray_index, width, height, frame_name and what the skeleton panel takes: joints [24,3] float32 in
        body space and the K and E that made the rays, on the host.  A frame without a ray raises ValueError."""
        from . import ops
        dev = cuda_device(device, 'AnimateFrames.device_frames', 'iterate the loader for the host frames')
        ds = self.dataset.to_device(dev)
        H, W, n = self.height, self.width, self.total_frames
        ahead = CameraRaysAhead(dev, H, W, prefetch)
        if self._uploaded_to != dev:                       # once per device, kept over calls
            self._uploaded = [ds.upload_pose(f, dev) for f in self.frames]
            self._uploaded_to = dev

        def start(i):
            v = self.frames[i]
            return ahead.start(v, v['K'], v['E'], v['min'], v['max'])

        pending = start(0) if n else None
        for i in range(n):
            bufs, R, v = ahead.take(pending)
            out = ops.view_frame(bufs['rays8'], bufs['box'], H, W, row_start=bufs['row_start'], R=R)
            pending = start(i + 1) if i + 1 < n else None  # after the gather is enqueued, before the consumer renders
            data = {'rays': out['rays'], 'near': out['near'], 'far': out['far'], 'bgcolor': torch.from_numpy(self.bgcolor)}
            data.update({k: (torch.from_numpy(c) if isinstance(c, np.ndarray) else c)
                         for k, c in ds.constants(self._uploaded[i], device=True).items()})
            yield data, None, {'idx': i, 'ray_index': out['ray_index'], 'width': W, 'height': H, 'frame_name': v['frame_name'],
                               'joints': v['joints'], 'K': v['K'], 'E': v['E']}

    def describe(self):
        """What animate.json records of the run, without the per-frame entries."""
        return {'motion': os.path.abspath(self.motion['path']), 'motion_kind': self.motion['kind'],
                'motion_frames': int(self.motion['poses'].shape[0]), 'frames': self.total_frames, 'substeps': self.substeps,
                'align': self.align, 'camera': self.camera, 'source_frame': self.frame_idx,
                'source_frame_name': self.dataset.frames[self.frame_idx]['frame_name'],
                'subject': os.path.abspath(self.dataset.dataset_path)}

    def describe_frame(self, idx):
        v = self.frames[idx]
        return {'idx': idx, 'keyframes': [int(k) for k in self.key[idx]], 'u': float(self.u[idx]),
                'bbox_min': [float(x) for x in v['min']], 'bbox_max': [float(x) for x in v['max']]}


def write_json(path, source, per_frame):
    """animate.json beside the image folder: source.describe() and, per rendered frame, describe_frame with what the run
    added (the ray count, the joints the skeleton panel dropped)."""
    with open(path, 'w') as f:
        json.dump(dict(source.describe(), per_frame=per_frame, definition='DESIGN.md section 7l'), f, indent=1)
