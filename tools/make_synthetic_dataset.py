"""Write a dataset directory in the reference's prepared layout (what core/data/occnerf/train.py's Dataset opens), made
from a seed: the SMPL model is licensed and the ZJU-MoCap / OcMotion pickles are not redistributable, so this is the
stand-in a user -- and the tests -- can train on.

    python tools/make_synthetic_dataset.py OUT_DIR [--frames 8 --width 512 --height 512 --seed 0 --all-cameras 0
                                                    --distortions k1,k2,p1,p2[,k3[,k4,k5,k6]]]

    OUT_DIR/cameras.pkl            {frame: {'intrinsics' 3x3, 'extrinsics' 4x4[, 'distortions' n]}}    float64
    OUT_DIR/mesh_infos.pkl         {frame: {'poses' 72, 'betas' 10, 'tpose_joints' 24x3, 'joints' 24x3, 'Rh' 3, 'Th' 3}}
    OUT_DIR/canonical_joints.pkl   {'joints' 24x3, 'avg_betas' 10}
    OUT_DIR/images/NAME.png, OUT_DIR/masks/NAME.png        NAME = frame_%06d (train.py:358 parses the six digits)
    OUT_DIR/all_cameras.pkl        {frame: {'intrinsics' Nx3x3, 'extrinsics' Nx4x4[, 'distortions' Nxn]}}     float64; only with --all-cameras N > 0:
                                   the rig `--type allview` renders from (allview.py:92-96), a ring of N cameras around the body

The subject is occnerf_amd/synth.py's capsule body walking between two seeded poses (synth.movement_pose), each vertex
carried rigidly by the joint its capsule hangs from, seen from the orbit camera of synth.setup_camera / rotate_camera as
float64 matrices (calibrated datasets are float64).  The body is placed in the world by a non-zero Rh / Th per frame, so a
loader has to apply apply_global_tfm_to_camera (camera_util.py:113-130) to find it.  Painting is numpy on the CPU: every
posed vertex is projected and splatted as a disc, far to near (the nearest vertex ends on top), coloured by a fixed function
of the vertex's CANONICAL position, so the views agree with one another; the mask is the discs' coverage with an
anti-aliased rim, i.e. it holds fractional values, not only 0 and 255.  The background of the image is seeded noise: only
the blend with the mask removes it.  Same arguments, same bytes in every array and pixel.

With --distortions the cameras carry the coefficients (OpenCV's order) and every photograph and mask is what a lens with those
coefficients would have recorded of the clean one (lens_image), so a loader has to undistort them (core/data/occnerf/
train.py:290-294) to see the body where the cameras put it."""
import argparse
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from occnerf_amd import synth  # noqa: E402

DISC_RADIUS_M = 0.03          # world radius of a vertex disc
MIN_DISC_PX = 1.6


def vertex_joints():
    """The joint each of the 6890 synthetic vertices hangs from: a capsule parent -> child turns with its parent joint, the
    head capsule with the head joint."""
    joints = synth.tpose_joints(np.zeros(1))
    parts = synth._part_list(joints)
    segs, rings = synth._plan_tessellation(parts, synth.N_VERTS)
    owner = [synth.SMPL_PARENT[i] for i in range(1, synth.TOTAL_BONES)] + [synth.HEAD_JOINT]
    return np.concatenate([np.full(int(s) * int(k) + 2, j, dtype=np.int64) for j, s, k in zip(owner, segs, rings)])


def posed_body(pose72, tjoints, verts, owner):
    """(posed vertices, posed joints) in the body's own space: forward kinematics of body_pose_to_body_RTs."""
    Rs, Ts = synth.body_pose_to_body_RTs(pose72, tjoints)
    G = np.zeros((synth.TOTAL_BONES, 4, 4))
    for i in range(synth.TOTAL_BONES):
        L = np.eye(4)
        L[:3, :3], L[:3, 3] = Rs[i], Ts[i]
        G[i] = L if i == 0 else G[synth.SMPL_PARENT[i]].dot(L)
    local = verts - tjoints[owner]
    posed = np.einsum('nij,nj->ni', G[owner, :3, :3], local) + G[owner, :3, 3]
    return posed, G[:, :3, 3]


def vertex_colours(canonical):
    """uint8 colour of a vertex: a fixed smooth function of its canonical position."""
    f = np.array([[7.0, 3.0, 5.0], [4.0, 9.0, 2.0], [3.0, 5.0, 11.0]])
    ph = np.array([0.3, 1.7, 2.9])
    c = 0.5 + 0.5 * np.sin(canonical.dot(f.T) + ph)
    return np.round(40.0 + 200.0 * c).astype(np.uint8)


def paint(uv, depth, radius_px, colours, H, W, background):
    """Painter's algorithm over discs: -> (image uint8 [H,W,3], mask uint8 [H,W])."""
    img = background.copy()
    cover = np.zeros((H, W), dtype=np.float64)
    for v in np.argsort(-depth, kind='stable'):
        cx, cy, r = uv[v, 0], uv[v, 1], radius_px[v]
        x0, x1 = int(np.floor(cx - r - 1)), int(np.ceil(cx + r + 1)) + 1
        y0, y1 = int(np.floor(cy - r - 1)), int(np.ceil(cy + r + 1)) + 1
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
        if x0 >= x1 or y0 >= y1:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1]
        c = np.clip(r + 0.5 - np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2), 0.0, 1.0)
        on = c > 0
        img[y0:y1, x0:x1][on] = colours[v]
        cover[y0:y1, x0:x1] = np.maximum(cover[y0:y1, x0:x1], c)
    return img, np.round(cover * 255.0).astype(np.uint8)


def lens_image(clean, K, dist):
    """What a lens with the coefficients dist = (k1, k2, p1, p2[, k3[, k4, k5, k6]]) records of the clean image (uint8 [H,W] or
    [H,W,C]) of camera K: every recorded pixel is a DISTORTED position; the ideal position that the model sends there is
    found by fixed-point iteration (20 rounds of x <- (xd - tangential(x)) / radial(x), OpenCV's undistortPoints), and the
    clean image is sampled there bilinearly, zero outside."""
    d = np.zeros(8)
    d[:len(dist)] = np.asarray(dist, dtype=np.float64).ravel()
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    H, W = clean.shape[:2]
    xd = ((np.arange(W, dtype=np.float64) - K[0, 2]) / K[0, 0])[None, :] + np.zeros((H, 1))
    yd = ((np.arange(H, dtype=np.float64) - K[1, 2]) / K[1, 1])[:, None] + np.zeros((1, W))
    x, y = xd.copy(), yd.copy()
    for _ in range(20):
        r2 = x * x + y * y
        inv = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (xd - dx) * inv, (yd - dy) * inv
    u, v = K[0, 0] * x + K[0, 2], K[1, 1] * y + K[1, 2]
    u, v = np.clip(np.nan_to_num(u, nan=-2.0), -2.0, W + 1.0), np.clip(np.nan_to_num(v, nan=-2.0), -2.0, H + 1.0)
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    a, b = u - x0, v - y0
    src = np.zeros((H + 2, W + 2) + clean.shape[2:], dtype=np.float64)
    src[1:-1, 1:-1] = clean
    if clean.ndim == 3:
        a, b = a[..., None], b[..., None]
    xa, xb, ya, yb = (np.clip(t, -1, n) + 1 for t, n in ((x0, W), (x0 + 1, W), (y0, H), (y0 + 1, H)))
    out = (1 - b) * ((1 - a) * src[ya, xa] + a * src[ya, xb]) + b * ((1 - a) * src[yb, xa] + a * src[yb, xb])
    return np.round(out).astype(np.uint8)


def frame_camera(i, frames, H, W, focal):
    K32, E32 = synth.setup_camera(max(H, W), focal=focal)
    E = E32.astype(np.float64)
    if i:
        E = synth.rotate_camera(E, 2 * np.pi * i / (4.0 * max(frames, 1)))      # a quarter orbit over the sequence
    K = K32.astype(np.float64)
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    return K, np.asarray(E, dtype=np.float64)


def camera_ring(K, E, Th, n):
    """n cameras for all_cameras.pkl: the frame's own camera turned about the vertical through the body (Th) in n equal
    steps, camera 0 being the frame's camera itself; all share its K."""
    Es = [np.asarray(E, dtype=np.float64) if c == 0 else
          synth.rotate_camera(E, 2 * np.pi * c / n, trans=Th.astype(np.float64), rotate_axis='y') for c in range(n)]
    return {'intrinsics': np.repeat(K[None], n, axis=0), 'extrinsics': np.stack(Es, 0)}


def make_dataset(out_dir, frames=8, width=512, height=512, seed=0, focal=1250.0, all_cameras=0, distortions=None):
    """Write the directory; -> the list of frame names.  all_cameras=N > 0 also writes all_cameras.pkl (camera_ring); with
    0 the directory is exactly what it is without the argument.  distortions: 4, 5 or 8 lens coefficients, written into
    both camera files, and every photograph and mask as that lens records it (lens_image); None changes nothing."""
    from PIL import Image
    H, W = int(height), int(width)
    if distortions is not None:
        distortions = np.asarray(distortions, dtype=np.float64).ravel()
        if distortions.size not in (4, 5, 8):
            raise ValueError(f'distortions: {distortions.size} coefficients; 4, 5 or 8 (k1, k2, p1, p2[, k3[, k4, k5, k6]])')
    rng = np.random.RandomState(seed)
    betas = np.zeros(10, dtype='float32')
    tjoints = synth.tpose_joints(betas)
    verts, _ = synth.SyntheticSMPL()(np.zeros(72), betas)
    owner = vertex_joints()
    assert owner.shape[0] == verts.shape[0]
    colours = vertex_colours(verts)
    os.makedirs(os.path.join(out_dir, 'images'), exist_ok=True)
    os.makedirs(os.path.join(out_dir, 'masks'), exist_ok=True)
    cameras, mesh_infos, names, rigs = {}, {}, [], {}
    for i in range(int(frames)):
        name = f'frame_{i:06d}'
        pose = synth.movement_pose(i, frames, seed_a=11 + 2 * seed, seed_b=12 + 2 * seed)
        posed, joints = posed_body(pose, tjoints, verts, owner)
        Rh = (np.array([0.05, 0.25, -0.04]) + 0.1 * rng.uniform(-1, 1, 3)).astype('float32')
        Th = (np.array([0.08, -0.05, 0.12]) + 0.05 * rng.uniform(-1, 1, 3)).astype('float32')
        K, E = frame_camera(i, frames, H, W, focal)
        world = posed.dot(synth.rodrigues_exact(Rh).T) + Th.astype(np.float64)
        cam = world.dot(E[:3, :3].T) + E[:3, 3]
        pix = cam.dot(K.T)
        uv, depth = pix[:, :2] / pix[:, 2:3], cam[:, 2]
        radius = np.maximum(DISC_RADIUS_M * K[0, 0] / depth, MIN_DISC_PX)
        background = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
        img, mask = paint(uv, depth, radius, colours, H, W, background)
        if distortions is not None:
            img, mask = lens_image(img, K, distortions), lens_image(mask, K, distortions)
        Image.fromarray(img, 'RGB').save(os.path.join(out_dir, 'images', name + '.png'))
        Image.fromarray(mask, 'L').save(os.path.join(out_dir, 'masks', name + '.png'))
        cameras[name] = {'intrinsics': K, 'extrinsics': E}
        if int(all_cameras) > 0:
            rigs[name] = camera_ring(K, E, Th, int(all_cameras))
        if distortions is not None:
            cameras[name]['distortions'] = distortions.copy()
            if int(all_cameras) > 0:
                rigs[name]['distortions'] = np.repeat(distortions[None], int(all_cameras), axis=0)
        mesh_infos[name] = {'poses': pose.astype('float32'), 'betas': betas.copy(),
                            'tpose_joints': tjoints.astype('float32'), 'joints': joints.astype('float32'), 'Rh': Rh, 'Th': Th}
        names.append(name)
    for fname, obj in (('cameras.pkl', cameras), ('mesh_infos.pkl', mesh_infos),
                       ('canonical_joints.pkl', {'joints': tjoints.astype('float32'), 'avg_betas': betas.copy()})):
        with open(os.path.join(out_dir, fname), 'wb') as f:
            pickle.dump(obj, f, protocol=4)
    if rigs:
        with open(os.path.join(out_dir, 'all_cameras.pkl'), 'wb') as f:
            pickle.dump(rigs, f, protocol=4)
    return names


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('out_dir')
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--focal', type=float, default=1250.0, help='focal length at 512 pixels (scaled with the larger side)')
    ap.add_argument('--all-cameras', type=int, default=0, help='N > 0: also write all_cameras.pkl, a ring of N cameras '
                                                               'around the body for every frame (--type allview)')
    ap.add_argument('--distortions', type=lambda t: [float(v) for v in t.split(',')], default=None,
                    help='k1,k2,p1,p2[,k3[,k4,k5,k6]]: the cameras carry these lens coefficients and the photographs and '
                         'masks are recorded through that lens')
    a = ap.parse_args()
    names = make_dataset(a.out_dir, a.frames, a.width, a.height, a.seed, a.focal, a.all_cameras, a.distortions)
    print(f'wrote {len(names)} frames of {a.width} x {a.height} to {a.out_dir}')


if __name__ == '__main__':
    main()
