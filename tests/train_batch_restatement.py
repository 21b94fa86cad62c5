"""numpy restatement of the reference's training Dataset in patch mode (core/data/occnerf/train.py:276-316 load_image and
:353-537 __getitem__, with :167-273 the patch draw), the truth the device batch builder (occnerf_amd/csrc/batch.hip,
occnerf_amd/dataset.py) is tested against.  It follows the reference line by line -- the line is cited at each step -- and is
itself held to a recording of the unmodified reference (tests/golden/train_batch_ref.npz, tools/record_train_batch_golden.py).

Randomness is an INPUT: the background colour, and per patch its class (0: subject, 1: box and not subject) and its
`select_idx`, the value np.random.choice returned at :239.  Nothing is drawn here.

Not restated: 'distortions' (:290-294), crop_image_scale (:300-304), resize_img_scale != 1 (:306-314), upsample_pc (:384)
and the SMPL 'verts' (:381) -- the build refuses or omits them.  get_rays_from_KRT and rays_intersect_3d_bbox are
occnerf_amd.synth's, which tests/test_oracle_golden.py pins to the reference's.
"""
import os
import pickle
from math import cos, sin

import numpy as np
from PIL import Image

from occnerf_amd import synth

DEFAULTS = {'bbox_offset': 0.3, 'resize_img_scale': 1.0, 'occlude': False, 'occlusion': {'range': 0, 'mid': 0, 'width': 0},
            'N_patches': 6, 'size': 32, 'sample_subject_ratio': 0.8, 'volume_size': 32, 'skip': 1, 'maxframes': -1}


def _load_image(path):                                            # image_util.py:9-11
    return Image.open(path).convert('RGB')


def skeleton_to_bbox(skeleton, bbox_offset):                      # :115-122
    return {'min_xyz': np.min(skeleton, axis=0) - bbox_offset, 'max_xyz': np.max(skeleton, axis=0) + bbox_offset}


def apply_global_tfm_to_camera(E, Rh, Th):                        # camera_util.py:113-130
    global_tfms = np.eye(4)
    global_rot = synth.rodrigues_exact(Rh).T                      # cv2.Rodrigues(Rh)[0].T
    global_trans = Th
    global_tfms[:3, :3] = global_rot
    global_tfms[:3, 3] = -global_rot.dot(global_trans)
    return E.dot(np.linalg.inv(global_tfms))


def rvec_to_rmtx(rvec):
    """body_util.py:200-219 in the dtype it is given (float32 poses): the axis is rvec / (|rvec| + 1e-5); the cos and
    1 - cos terms meet a float64 identity / python floats, the sin term stays in the vector's dtype."""
    rvec = rvec.reshape(3, 1)
    theta = np.linalg.norm(rvec)
    r = rvec / (theta + 1e-5)
    rx, ry, rz = r.ravel()
    skew = np.array([[0, -rz, ry], [rz, 0, -rx], [-ry, rx, 0]])                      # body_util.py:48-61
    return cos(theta) * np.eye(3) + sin(theta) * skew + (1 - cos(theta)) * r.dot(r.T)


def body_pose_to_body_RTs(jangles, tpose_joints):                  # body_util.py:222-248
    jangles = jangles.reshape(-1, 3)
    n = jangles.shape[0]
    Rs = np.zeros(shape=[n, 3, 3], dtype='float32')
    Ts = np.zeros(shape=[n, 3], dtype='float32')
    Rs[0] = rvec_to_rmtx(jangles[0, :])
    Ts[0] = tpose_joints[0, :]
    for i in range(1, n):
        Rs[i] = rvec_to_rmtx(jangles[i, :])
        Ts[i] = tpose_joints[i, :] - tpose_joints[synth.SMPL_PARENT[i], :]
    return Rs, Ts


def get_rotation_mtx(v1, v2):
    """body_util.py:83-114 for one pair of float32 vectors: the rotation taking v1's direction to v2's.  The cosine is kept
    in a float64 array, so the quadratic term is formed in float64 before the float32 store."""
    v1 = v1 / np.clip(np.linalg.norm(v1, axis=-1, keepdims=True), 1e-5, None)
    v2 = v2 / np.clip(np.linalg.norm(v2, axis=-1, keepdims=True), 1e-5, None)
    nx, ny, nz = np.cross(v1, v2, axis=-1).ravel()
    cos_v = np.zeros(shape=(1,))
    cos_v[0] = v1.ravel().dot(v2.ravel())
    skew = np.zeros(shape=(3, 3), dtype=np.float32)
    skew[:] = np.array([[0, -nz, ny], [nz, 0, -nx], [-ny, nx, 0]])
    R = np.zeros(shape=(3, 3), dtype=np.float32)
    R[:] = np.eye(3) + skew + (skew.dot(skew)) * (1. / (1. + cos_v))
    return R


def deform_gaussian_volume(grid_size, bbox_min_xyz, bbox_max_xyz, center, S, R):    # body_util.py:138-179
    sigma = R.dot(S).dot(S).dot(R.T)
    zgrid, ygrid, xgrid = np.meshgrid(np.linspace(bbox_min_xyz[2], bbox_max_xyz[2], grid_size),
                                      np.linspace(bbox_min_xyz[1], bbox_max_xyz[1], grid_size),
                                      np.linspace(bbox_min_xyz[0], bbox_max_xyz[0], grid_size), indexing='ij')
    grid = np.stack([xgrid - center[0], ygrid - center[1], zgrid - center[2]], axis=-1)
    dist = np.einsum('abci, abci->abc', np.einsum('abci, ij->abcj', grid, sigma), grid)
    return np.exp(-1 * dist)


def std_to_scale_mtx(stds):                                       # body_util.py:182-197
    scale_mtx = np.eye(3, dtype=np.float32)
    for a in range(3):
        scale_mtx[a][a] = 1.0 / stds[a]
    return scale_mtx


def approx_gaussian_bone_volumes(tpose_joints, bbox_min_xyz, bbox_max_xyz, grid_size=32):    # body_util.py:274-350
    bone_stds, head_stds, joint_stds = np.array([0.03, 0.06, 0.03]), np.array([0.06] * 3), np.array([0.02] * 3)   # :43-45
    total_joints = tpose_joints.shape[0]
    tpose_joints = tpose_joints.astype(np.float32)
    calibrated_bone = np.array([0.0, 1.0, 0.0], dtype=np.float32)[None, :]
    g_volumes = []
    for joint_idx in range(0, total_joints):
        gaussian_volume = np.zeros(shape=[grid_size] * 3, dtype='float32')
        is_parent_joint = False
        for bone_idx, parent_idx in synth.SMPL_PARENT.items():
            if joint_idx != parent_idx:
                continue
            S = std_to_scale_mtx(bone_stds * 2.)
            if joint_idx in synth.TORSO_JOINTS:
                S[0][0] *= 1 / 1.5
                S[2][2] *= 1 / 1.5
            start_joint = tpose_joints[synth.SMPL_PARENT[bone_idx]]
            end_joint = tpose_joints[bone_idx]
            R = get_rotation_mtx(calibrated_bone, (end_joint - start_joint)[None, :]).astype(np.float32)
            center = (start_joint + end_joint) / 2.0
            gaussian_volume = gaussian_volume + deform_gaussian_volume(grid_size, bbox_min_xyz, bbox_max_xyz, center, S, R)
            is_parent_joint = True
        if not is_parent_joint:                                   # an end joint
            S = std_to_scale_mtx((head_stds if joint_idx == synth.HEAD_JOINT else joint_stds) * 2.)
            gaussian_volume = deform_gaussian_volume(grid_size, bbox_min_xyz, bbox_max_xyz, tpose_joints[joint_idx], S,
                                                     np.eye(3, dtype='float32'))
        g_volumes.append(gaussian_volume)
    g_volumes = np.stack(g_volumes, axis=0)
    bg_volume = 1.0 - np.sum(g_volumes, axis=0, keepdims=True).clip(min=0.0, max=1.0)
    g_volumes = np.concatenate([g_volumes, bg_volume], axis=0)
    return g_volumes / np.sum(g_volumes, axis=0, keepdims=True).clip(min=0.001)


def frame_list(dataset_path, skip=1, maxframes=-1):               # :135-138, :68-75
    d = os.path.join(dataset_path, 'images')
    names = sorted(os.path.join(d, f) for f in os.listdir(d) if os.path.isfile(os.path.join(d, f)) and f.endswith('.png'))
    names = [os.path.splitext(os.path.split(p)[1])[0] for p in names][::skip]
    return names[:maxframes] if maxframes > 0 else names


def load_image(dataset_path, frame_name, bg_color, idx, cfg):     # :276-316
    orig_img = np.array(_load_image(os.path.join(dataset_path, 'images', '{}.png'.format(frame_name))))
    alpha_mask = np.array(_load_image(os.path.join(dataset_path, 'masks', '{}.png'.format(frame_name))))
    if cfg['occlude'] and idx < cfg['occlusion']['range']:        # :286-287
        mid, width = cfg['occlusion']['mid'], cfg['occlusion']['width']
        alpha_mask[:, mid - width // 2:mid + width // 2] *= 0
    alpha_mask = alpha_mask / 255.                                # :296
    img = alpha_mask * orig_img + (1.0 - alpha_mask) * bg_color[None, None, :]      # :297
    assert cfg['resize_img_scale'] == 1.
    return img, alpha_mask


def class_masks(alpha, ray_mask, H, W):
    """(subject, box and not subject) as :470-471 and :179-182 form them."""
    subject_mask = alpha[:, :, 0] > 0.
    bbox_mask = ray_mask.reshape(H, W)
    return subject_mask, np.bitwise_and(bbox_mask, np.bitwise_not(subject_mask))


def _get_patch_ray_indices(ray_mask, candidate_mask, select_idx, patch_size, H, W):    # :225-273
    valid_ys, valid_xs = np.where(candidate_mask)                 # :236
    center_x = valid_xs[select_idx]                               # :241-242
    center_y = valid_ys[select_idx]
    half_patch_size = patch_size // 2                             # :245-253
    x_min = np.clip(a=center_x - half_patch_size, a_min=0, a_max=W - patch_size)
    x_max = x_min + patch_size
    y_min = np.clip(a=center_y - half_patch_size, a_min=0, a_max=H - patch_size)
    y_max = y_min + patch_size
    sel_ray_mask = np.zeros_like(candidate_mask)                  # :255-256
    sel_ray_mask[y_min:y_max, x_min:x_max] = True
    sel_ray_mask = sel_ray_mask.reshape(-1)                       # :262-267
    inter_mask = np.bitwise_and(sel_ray_mask, ray_mask)
    select_masked_inds = np.where(inter_mask)
    masked_indices = np.cumsum(ray_mask) - 1
    select_inds = masked_indices[select_masked_inds]
    inter_mask = inter_mask.reshape(H, W)                         # :269-273
    return select_inds, inter_mask[y_min:y_max, x_min:x_max], np.array([x_min, y_min]), np.array([x_max, y_max])


def get_patch_ray_indices(draws, ray_mask, subject_mask, bbox_mask, patch_size, H, W):    # :167-222
    bbox_exclude_subject_mask = np.bitwise_and(bbox_mask, np.bitwise_not(subject_mask))
    list_ray_indices, list_mask, list_xy_min, list_xy_max = [], [], [], []
    total_rays = 0
    patch_div_indices = [total_rays]
    for cls, select_idx in draws:                                 # :191-198: the class is the caller's draw
        candidate_mask = subject_mask if cls == 0 else bbox_exclude_subject_mask
        ray_indices, mask, xy_min, xy_max = _get_patch_ray_indices(ray_mask, candidate_mask, int(select_idx), patch_size, H, W)
        total_rays += len(ray_indices)
        list_ray_indices.append(ray_indices)
        list_mask.append(mask)
        list_xy_min.append(xy_min)
        list_xy_max.append(xy_max)
        patch_div_indices.append(total_rays)
    select_inds = np.concatenate(list_ray_indices, axis=0)        # :214
    patch_info = {'mask': np.stack(list_mask, axis=0), 'xy_min': np.stack(list_xy_min, axis=0),
                  'xy_max': np.stack(list_xy_max, axis=0)}
    return select_inds, patch_info, np.array(patch_div_indices)


class Restatement:
    """The reference Dataset's __init__ (:34-95) on a directory; `getitem` is its __getitem__ in patch mode."""

    def __init__(self, dataset_path, **cfg):
        self.cfg = {**DEFAULTS, **cfg}
        self.dataset_path = dataset_path
        with open(os.path.join(dataset_path, 'canonical_joints.pkl'), 'rb') as f:      # :97-106
            cl = pickle.load(f)
        self.canonical_joints = cl['joints'].astype('float32')
        self.canonical_bbox = skeleton_to_bbox(self.canonical_joints, self.cfg['bbox_offset'])
        self.avg_betas = cl['avg_betas'].astype('float32')
        self.motion_weights_priors = approx_gaussian_bone_volumes(                # :56-62
            self.canonical_joints, self.canonical_bbox['min_xyz'], self.canonical_bbox['max_xyz'],
            grid_size=self.cfg['volume_size']).astype('float32')
        with open(os.path.join(dataset_path, 'cameras.pkl'), 'rb') as f:            # :108-112
            self.cameras = pickle.load(f)
        with open(os.path.join(dataset_path, 'mesh_infos.pkl'), 'rb') as f:         # :124-133
            self.mesh_infos = pickle.load(f)
        for name in self.mesh_infos:
            self.mesh_infos[name]['bbox'] = skeleton_to_bbox(self.mesh_infos[name]['joints'], self.cfg['bbox_offset'])
        self.framelist = frame_list(dataset_path, self.cfg['skip'], self.cfg['maxframes'])

    def frame_masks(self, idx):
        """(alpha [H,W,3] float64, ray_mask [H*W], subject, off-subject) of frame idx: what the draw of a patch sees."""
        r = self.getitem(idx, np.zeros(3, 'float32'), None)
        return r['_alpha'], r['ray_mask'], r['_subject'], r['_off_subject']

    def getitem(self, idx, bgcolor, draws):
        """draws: [(class, select_idx)] * N_patches, or None for everything up to the patch draw."""
        cfg = self.cfg
        frame_name = self.framelist[idx]                                            # :356-363
        results = {'frame_name': frame_name, 'idx': int(frame_name[-6:]), 'time': idx / len(self.framelist)}
        info = self.mesh_infos[frame_name]                                          # :140-156
        dst_bbox = info['bbox'].copy()
        dst_poses = info['poses'].astype('float32')
        dst_betas = info['betas'].astype('float32')
        dst_tpose_joints = info['tpose_joints'].astype('float32')
        Rh, Th = info['Rh'].astype('float32'), info['Th'].astype('float32')
        bgcolor = np.array(bgcolor, dtype='float32')                                # :387-390
        img, alpha = load_image(self.dataset_path, frame_name, bgcolor, idx, cfg)   # :393
        results['_empty'] = bool(np.sum(alpha) < 1)                                 # :395: the reference draws another frame
        img = (img / 255.).astype('float32')                                        # :398
        H, W = img.shape[0:2]
        results.update({'poses': dst_poses, 'betas': dst_betas, 'Rh': synth.rodrigues_exact(Rh).astype(np.float32),
                        'Th': Th, 'joints': info['joints'].astype('float32')})      # :410-417 without 'verts'
        K = self.cameras[frame_name]['intrinsics'][:3, :3].copy()                   # :421-430
        K[:2] *= cfg['resize_img_scale']
        E = apply_global_tfm_to_camera(E=self.cameras[frame_name]['extrinsics'], Rh=Rh, Th=Th)     # :432-438
        R, T = E[:3, :3], E[:3, 3]
        rays_o, rays_d = synth.get_rays_from_KRT(H, W, K, R, T)                      # :440
        ray_img = img.reshape(-1, 3)                                                # :443-445
        rays_o = rays_o.reshape(-1, 3)
        rays_d = rays_d.reshape(-1, 3)
        near, far, ray_mask = synth.rays_intersect_3d_bbox(dst_bbox, rays_o, rays_d)    # :448
        rays_o, rays_d, ray_img = rays_o[ray_mask], rays_d[ray_mask], ray_img[ray_mask]   # :449-451
        results['ray_alpha'] = alpha.reshape(-1, 3)[ray_mask]                       # :453-458
        near = near[:, None].astype('float32')                                      # :461-462
        far = far[:, None].astype('float32')
        subject_mask = alpha[:, :, 0] > 0.                                          # :470
        results.update({'_alpha': alpha, '_subject': subject_mask, 'ray_mask': ray_mask,
                        '_off_subject': class_masks(alpha, ray_mask, H, W)[1], '_K': K, '_E': E, '_bbox': dst_bbox})
        if draws is None:
            return results
        select_inds, patch_info, patch_div_indices = get_patch_ray_indices(       # :326-333
            draws, ray_mask, subject_mask, ray_mask.reshape(H, W), cfg['size'], H, W)
        rays_o, rays_d, ray_img, near, far = rays_o[select_inds], rays_d[select_inds], ray_img[select_inds], \
            near[select_inds], far[select_inds]                                     # :159-165
        targets = []                                                                # :338-343
        for i in range(len(draws)):
            x_min, y_min = patch_info['xy_min'][i]
            x_max, y_max = patch_info['xy_max'][i]
            targets.append(img[y_min:y_max, x_min:x_max])
        results.update({                                                            # :481-501
            'img_width': W, 'img_height': H, 'rays': np.stack([rays_o, rays_d], axis=0), 'near': near, 'far': far,
            'bgcolor': bgcolor, 'patch_div_indices': patch_div_indices, 'patch_masks': patch_info['mask'],
            'patch_mask': select_inds, 'target_patches': np.stack(targets, axis=0), 'target_rgbs': ray_img,
            '_xy_min': patch_info['xy_min']})
        dst_Rs, dst_Ts = body_pose_to_body_RTs(dst_poses, dst_tpose_joints)         # :503-513
        results.update({'dst_Rs': dst_Rs, 'dst_Ts': dst_Ts, 'cnl_gtfms': synth.get_canonical_global_tfms(self.canonical_joints)})
        results['motion_weights_priors'] = self.motion_weights_priors.copy()        # :515-516
        min_xyz = self.canonical_bbox['min_xyz'].astype('float32')                  # :519-527
        max_xyz = self.canonical_bbox['max_xyz'].astype('float32')
        results.update({'cnl_bbox_min_xyz': min_xyz, 'cnl_bbox_max_xyz': max_xyz,
                        'cnl_bbox_scale_xyz': 2.0 / (max_xyz - min_xyz)})
        results['dst_posevec'] = dst_poses[3:] + 1e-2                               # :529-535
        return results


# ---------------------------------------------------------------- the device builder's draw, in the restatement's terms
def draws_from_uniforms(u, subject_mask, off_subject_mask, sample_subject_ratio):
    """What the batch builder makes of its uniforms u[N,2] (include/occnerf_hip.h, occnerf_patch_batch): class 0 when
    u0 < ratio (:195), the other class when that one is empty, select_idx = min(floor(u1 * count), count - 1)."""
    counts = (int(subject_mask.sum()), int(off_subject_mask.sum()))
    out = []
    for u0, u1 in np.asarray(u, dtype=np.float64):
        cls = 0 if u0 < sample_subject_ratio else 1
        if counts[cls] == 0:
            cls ^= 1
        out.append((cls, min(int(np.floor(u1 * counts[cls])), counts[cls] - 1)))
    return out


def pixel_maps(patch_masks):
    """(pix_of_row, row_of_pix) of a batch from its patch_masks [N,S,S]: rows are the set pixels in patch, row-major order."""
    flat = np.asarray(patch_masks).reshape(-1)
    pix_of_row = np.nonzero(flat)[0].astype(np.int32)
    row_of_pix = -np.ones(flat.size, dtype=np.int32)
    row_of_pix[pix_of_row] = np.arange(pix_of_row.size, dtype=np.int32)
    return pix_of_row, row_of_pix
