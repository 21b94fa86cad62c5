"""The body as a triangle mesh (run.py --type mesh).  The reference exports no geometry; this has no
counterpart there.

  density_grid   the canonical density softplus(raw[..., 3]) (the reference's _raw2alpha activation) on a grid of cubic voxels
                 over the canonical box, through Network.query_canonical: no warp, no non-rigid offset;
  extract_mesh   marching tetrahedra on the Kuhn split in HIP (csrc/mesh.hip: count, emit, vertices), the row scan and the
                 welding (torch.cumsum, torch.unique) as plumbing between the launches;
  export_mesh    grid, surface, vertex colours by a second query at the vertices, host float64 area-weighted normals, a binary
                 little-endian PLY and a JSON sidecar;
  pose_mesh      the vertices in the pose of a frame: the frame's non-rigid offset undone by a fixed point
                 on the renderer's own kernel (Network.unoffset_canonical), then the skeletal warp inverted per vertex by a
                 damped Newton iteration in HIP (csrc/mesh_pose.hip) -- the model only knows the map from a frame to the
                 canonical body;
  export_posed   posed/<frame name>.ply per frame -- the faces and colours of mesh.ply, the posed vertices, their normals --
                 and posed.json.

Every step is a pure function of its inputs: the same checkpoint and settings give the same PLY byte for byte (the sidecars
differ in their wall times only).  Floater removal, decimation, smoothing, OBJ and a mesh welded from the f16x3 kernels' field
are not offered; nor, for the posed mesh, roots of the warp other than the owning bone's or changes of topology."""
import json
import math
import os
import time
import warnings

import numpy as np
import torch

from . import ops
from .image import to_8b_image
from .synth import vertex_normals


def grid_shape(bbox_min, bbox_max, resolution):
    """(h, (nx, ny, nz)) of the grid over the box: cubic voxels of edge h = max extent / resolution in float64 of the float32
    box; an axis as long as the longest gets resolution + 1 points by rule (extent / h need not round to `resolution`), every
    other axis floor(extent / h) + 1, so the last point never lies outside the box."""
    lo = np.asarray(bbox_min, dtype=np.float32).reshape(3).astype(np.float64)
    hi = np.asarray(bbox_max, dtype=np.float32).reshape(3).astype(np.float64)
    resolution = int(resolution)
    ext = hi - lo
    if resolution < 1 or not np.all(np.isfinite(ext)) or not np.all(ext > 0):
        raise RuntimeError(f'mesh: resolution {resolution} / box {lo.tolist()} .. {hi.tolist()}: a positive resolution and a '
                           'box with a positive finite extent on every axis are needed')
    h = float(ext.max() / resolution)
    n = [resolution + 1 if e == ext.max() else min(int(math.floor(e / h)), resolution) + 1 for e in ext]
    if min(n) < 2:
        raise RuntimeError(f'mesh: resolution {resolution} leaves an axis of the box {ext.tolist()} with a single grid point')
    if n[0] * n[1] * n[2] >= 1 << 31:
        raise RuntimeError(f'mesh: a grid of {n[0]} x {n[1]} x {n[2]} points reaches the limit of 2^31; lower mesh.resolution')
    return h, tuple(n)


def default_level(h):
    """The density at which one voxel edge of matter is half opaque: 1 - exp(-sigma h) = 0.5."""
    return math.log(2.0) / float(h)


def grid_axes(bbox_min, h, shape):
    """Per axis, the float32 coordinates float32(min + float64(i) * h) of the grid points."""
    lo = np.asarray(bbox_min, dtype=np.float32).reshape(3).astype(np.float64)
    return [(lo[a] + np.arange(shape[a], dtype=np.float64) * np.float64(h)).astype(np.float32) for a in range(3)]


def density_grid(net, bbox_min, bbox_max, resolution, chunk=1 << 21):
    """-> (field float32 [nz,ny,nx] on the module's device, x fastest; h; (nx, ny, nz))."""
    h, (nx, ny, nz) = grid_shape(bbox_min, bbox_max, resolution)
    dev = net.point_base.device
    ax, ay, az = (torch.from_numpy(a).to(dev) for a in grid_axes(bbox_min, h, (nx, ny, nz)))
    field = torch.empty(nz, ny, nx, device=dev)
    slabs = max(1, int(chunk) // (nx * ny))            # whole z slabs per query (rows are independent: any split gives the same bits)
    for z0 in range(0, nz, slabs):
        z1 = min(nz, z0 + slabs)
        pts = torch.stack([ax[None, None, :].expand(z1 - z0, ny, nx), ay[None, :, None].expand(z1 - z0, ny, nx),
                           az[z0:z1, None, None].expand(z1 - z0, ny, nx)], dim=-1).reshape(-1, 3).contiguous()
        raw = net.query_canonical(pts, chunk=chunk)
        field[z0:z1] = torch.nn.functional.softplus(raw[:, 3]).reshape(z1 - z0, ny, nx)
    return field, h, (nx, ny, nz)


def extract_mesh(field, level, bbox_min, h):
    """(verts float32 [V,3], faces int32 [T,3]) on the field's device: the surface f = level (rounded to float32) of field
    [nz,ny,nx], grid point (i,j,k) at bbox_min + (i,j,k) * h.  The triangle total is read back with one blocking copy."""
    level = float(np.float32(level))
    row_count = ops.mesh_count(field, level)
    ends = torch.cumsum(row_count, 0, dtype=torch.int64)
    T = int(ends[-1].item())
    tri_keys = ops.mesh_emit(field, level, (ends - row_count).contiguous(), T)
    if T == 0:
        return torch.empty(0, 3, device=field.device), torch.empty(0, 3, device=field.device, dtype=torch.int32)
    keys, inverse = torch.unique(tri_keys, sorted=True, return_inverse=True)
    return ops.mesh_vertices(keys, field, level, bbox_min, h), inverse.reshape(T, 3).to(torch.int32)


def boundary_inside(field, level):
    """Inside grid points on the six boundary faces: where there are any the surface meets the grid's boundary and is open."""
    inside = field > float(np.float32(level))
    return int(inside.sum().item()) - int(inside[1:-1, 1:-1, 1:-1].sum().item())


def write_ply(path, verts, faces, colors, normals=None):
    """Binary little-endian PLY: x y z float32, optionally nx ny nz float32, red green blue uchar; faces uchar 3 + 3 x int32."""
    verts, faces = np.asarray(verts, dtype='<f4').reshape(-1, 3), np.asarray(faces, dtype='<i4').reshape(-1, 3)
    props = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    if normals is not None:
        props += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
    props += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
    v = np.zeros(verts.shape[0], dtype=np.dtype(props))
    v['x'], v['y'], v['z'] = verts[:, 0], verts[:, 1], verts[:, 2]
    if normals is not None:
        n = np.asarray(normals, dtype='<f4').reshape(-1, 3)
        v['nx'], v['ny'], v['nz'] = n[:, 0], n[:, 1], n[:, 2]
    c = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)
    v['red'], v['green'], v['blue'] = c[:, 0], c[:, 1], c[:, 2]
    f = np.zeros(faces.shape[0], dtype=np.dtype([('n', 'u1'), ('v', '<i4', (3,))]))
    f['n'], f['v'] = 3, faces
    head = ['ply', 'format binary_little_endian 1.0', f'element vertex {verts.shape[0]}']
    head += [f"property {'uchar' if t == 'u1' else 'float'} {name}" for name, t in props]
    head += [f'element face {faces.shape[0]}', 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as out:
        out.write(('\n'.join(head) + '\n').encode('ascii'))
        out.write(v.tobytes())
        out.write(f.tobytes())


def export_mesh(net, out_dir, bbox_min, bbox_max, resolution=256, level=None, normals=True, chunk=1 << 21, keep=None):
    """<out_dir>/mesh.ply and mesh.json of the canonical body -> the sidecar's dict.  keep: a dict that receives what
    export_posed needs of the mesh ('verts' float32 [V,3] on the device, 'faces' int32 [T,3] and 'colors' uint8 [V,3] numpy)."""
    dev = net.point_base.device

    def clock():
        torch.cuda.synchronize(dev)
        return time.perf_counter()
    t0 = clock()
    field, h, (nx, ny, nz) = density_grid(net, bbox_min, bbox_max, resolution, chunk)
    t1 = clock()
    used = default_level(h) if level is None else float(level)
    lo = np.asarray(bbox_min, dtype=np.float32).reshape(3).astype(np.float64)
    verts, faces = extract_mesh(field, used, lo, h)
    on_boundary = boundary_inside(field, used)
    t2 = clock()
    rgb = torch.sigmoid(net.query_canonical(verts, chunk=chunk)[:, :3])
    colors = to_8b_image(rgb.cpu().numpy())
    t3 = clock()
    if on_boundary:
        warnings.warn(f'export_mesh: {on_boundary} grid points on the boundary of the box are inside the surface (density above '
                      f'{float(np.float32(used)):g}): the mesh is open there and is written as it is')
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    if keep is not None:
        keep.update(verts=verts, faces=f, colors=colors)
    os.makedirs(out_dir, exist_ok=True)
    write_ply(os.path.join(out_dir, 'mesh.ply'), v, f, colors, vertex_normals(v, f) if normals and len(f) else
              (np.zeros_like(v) if normals else None))
    info = {'resolution': int(resolution), 'h': h, 'level': float(np.float32(used)), 'level_is_default': level is None,
            'grid_shape_xyz': [nx, ny, nz], 'vertices': int(v.shape[0]), 'triangles': int(f.shape[0]),
            'inside_points_on_boundary': on_boundary, 'normals': bool(normals),
            'seconds': {'grid': round(t1 - t0, 4), 'extract': round(t2 - t1, 4), 'colour': round(t3 - t2, 4)}}
    with open(os.path.join(out_dir, 'mesh.json'), 'w') as out:
        json.dump(info, out, indent=1)
        out.write('\n')
    return info


# ------------------------------------------------------------------ the mesh in the pose of a frame
def pose_mesh(net, verts, data, candidates=3, max_iter=20, tol=1e-7, non_rigid=True, iter_val=1e7, stats=None):
    """(posed float32 [V,3], flag uint8 [V], iters uint8 [V], resid float32 [V]) on the device: where the frame `data` (the
    renderer's per-frame dict: dst_Rs, dst_Ts, dst_posevec, cnl_gtfms, motion_weights_priors as tensors, the box constants) puts
    the canonical vertices `verts`, in the body's own space -- the p the render of that frame maps onto the vertex: the
    non-rigid offset undone (Network.unoffset_canonical; non_rigid False: taken as absent), then ops.mesh_pose on the frame's
    Rs / Ts / motion-weight volume as Network.render_preamble computes them.  flag: 0 solved, 1 not converged, 2 no bone
    carries the vertex.  stats: a dict that receives the rows the fixed point left moving and the wall times."""
    dev = net.point_base.device

    def clock():
        torch.cuda.synchronize(dev)
        return time.perf_counter()
    t0 = clock()
    Rs, Ts, vol = net.render_preamble(data, iter_val)
    if non_rigid:
        s, moving = net.unoffset_canonical(verts, data, iter_val)
    else:
        s, moving = verts.detach().contiguous(), None
    t1 = clock()
    out = ops.mesh_pose(s, Rs, Ts, vol[:Rs.shape[0]], ops.host_float3(data['cnl_bbox_min_xyz']),
                        ops.host_float3(data['cnl_bbox_scale_xyz']), candidates=candidates, max_iter=max_iter, tol=tol)
    t2 = clock()
    if stats is not None:
        stats.update(non_rigid_moving=0 if moving is None else int(moving.sum().item()),
                     seconds={'unoffset': round(t1 - t0, 4), 'pose': round(t2 - t1, 4)})
    return out


def to_world(p, Rh, Th):
    """float32(R(Rh) p + Th) in host float64, rounded once: the body's own space -> the space of the cameras in cameras.pkl."""
    p64 = np.asarray(p, dtype=np.float32).astype(np.float64)
    R, t = np.asarray(Rh, dtype=np.float32).astype(np.float64).reshape(3, 3), np.asarray(Th, dtype=np.float32).astype(np.float64).reshape(3)
    return ((p64[:, 0:1] * R[:, 0] + p64[:, 1:2] * R[:, 1]) + p64[:, 2:3] * R[:, 2] + t).astype(np.float32)


class PoseFrames:
    """The per-frame body constants of the source run.py --type movement renders, nothing else: no rays, no images.  A prepared
    dataset directory (canonical_joints.pkl, mesh_infos.pkl and the names of images/*.png, as dataset.PreparedDataset lists
    them; the PNGs are not opened) or, with path None, the synthetic movement sequence of `total_frames` frames.
    frame(i) -> (frame name, the renderer's per-frame constants as numpy, Rh float32 [3,3], Th float32 [3])."""

    def __init__(self, path=None, total_frames=100, bbox_offset=0.3, volume_size=32):
        from . import synth
        self.path, self._synth = path, synth
        if path is None:
            self.names = [f'frame_{i:06d}' for i in range(int(total_frames))]
            return
        import pickle
        from .dataset import Subject
        self.subject = Subject(path, bbox_offset, volume_size)
        with open(os.path.join(path, 'mesh_infos.pkl'), 'rb') as f:
            self.infos = pickle.load(f)
        self.names = sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(path, 'images'))
                            if f.endswith('.png') and os.path.isfile(os.path.join(path, 'images', f)))

    def __len__(self):
        return len(self.names)

    def frame(self, i):
        synth, name = self._synth, self.names[i]
        if self.path is None:
            fr = synth.make_frame(img_size=8, pose72=synth.movement_pose(i, len(self.names)), with_rays=False)
            return name, fr, np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
        info = self.infos[name]
        poses = info['poses'].astype('float32')
        dst_Rs, dst_Ts = synth.body_pose_to_body_RTs(poses, info['tpose_joints'].astype('float32'))
        data = self.subject.constants({'dst_Rs': dst_Rs, 'dst_Ts': dst_Ts, 'dst_posevec': poses[3:] + 1e-2})
        return name, data, synth.rodrigues_exact(info['Rh'].astype('float32')).astype(np.float32), info['Th'].astype('float32')


_POSE_KEYS = ('dst_Rs', 'dst_Ts', 'dst_posevec', 'cnl_gtfms', 'motion_weights_priors')


def export_posed(net, out_dir, kept, source, frames, candidates=3, max_iter=20, tol=1e-7, non_rigid=True, world=False,
                 normals=True, iter_val=1e7):
    """<out_dir>/posed/<frame name>.ply for the frames (indices into `source`, a PoseFrames; 'all': every one) and
    <out_dir>/posed.json -> its dict.  kept: what export_mesh(keep=...) left of mesh.ply: every posed PLY has its faces and
    colours, the posed vertices and (normals) the normals recomputed from them."""
    dev = net.point_base.device
    idxs = list(range(len(source))) if isinstance(frames, str) and frames == 'all' else [int(i) for i in frames]
    for i in idxs:
        if not 0 <= i < len(source):
            raise RuntimeError(f'mesh_pose.frames: frame {i} outside the {len(source)} frames of the source')
    verts, faces, colors = kept['verts'], kept['faces'], kept['colors']
    os.makedirs(os.path.join(out_dir, 'posed'), exist_ok=True)
    V, per_frame = int(verts.shape[0]), []
    for i in idxs:
        name, fr, Rh, Th = source.frame(i)
        data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in _POSE_KEYS}
        data.update({k: np.asarray(fr[k], dtype=np.float32) for k in ('cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz')})
        stats = {}
        p, flag, iters, resid = pose_mesh(net, verts, data, candidates, max_iter, tol, non_rigid, iter_val, stats)
        t0 = time.perf_counter()
        p, flag = p.cpu().numpy(), flag.cpu().numpy()
        if world:
            p = to_world(p, Rh, Th)
        write_ply(os.path.join(out_dir, 'posed', f'{name}.ply'), p, faces, colors,
                  vertex_normals(p, faces) if normals and len(faces) else (np.zeros_like(p) if normals else None))
        stats['seconds']['write'] = round(time.perf_counter() - t0, 4)
        counts = np.bincount(flag, minlength=3)
        per_frame.append({'frame': i, 'name': name, 'converged': int(counts[0]), 'not_converged': int(counts[1]),
                          'no_bone': int(counts[2]), 'flagged_share': float(counts[1] + counts[2]) / max(V, 1),
                          'worst_resid': float(resid.max().item()) if V else 0.0,
                          'mean_iters': float(iters.float().mean().item()) if V else 0.0, **stats})
    info = {'vertices': V, 'candidates': int(candidates), 'max_iter': int(max_iter), 'tol': float(tol),
            'non_rigid': bool(non_rigid and not net.cfg.ignore_non_rigid_motions), 'world': bool(world), 'frames': per_frame}
    with open(os.path.join(out_dir, 'posed.json'), 'w') as out:
        json.dump(info, out, indent=1)
        out.write('\n')
    return info
