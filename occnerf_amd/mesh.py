"""The body as a triangle mesh (run.py --type mesh).  The reference exports no geometry; this has no
counterpart there.

  density_grid   the canonical density softplus(raw[..., 3]) (the reference's _raw2alpha activation) on a grid of cubic voxels
                 over the canonical box, through Network.query_canonical: no warp, no non-rigid offset;
  extract_mesh   marching tetrahedra on the Kuhn split in HIP (csrc/mesh.hip: count, emit, vertices), the row scan and the
                 welding (torch.cumsum, torch.unique) as plumbing between the launches;
  export_mesh    grid, surface, vertex colours by a second query at the vertices, host float64 area-weighted normals, a binary
                 little-endian PLY and a JSON sidecar;
  component_table, select_components, filter_mesh
                 the opt-in clean-up between the surface and the colours (mesh.components,
                 mesh.drop_cavities): connected components labelled in HIP (csrc/mesh_components.hip), an integer record per
                 component, detached blobs dropped by their triangle count and closed shells of negative volume as cavities;
  pose_mesh      the vertices in the pose of a frame: the frame's non-rigid offset undone by a fixed point
                 on the renderer's own kernel (Network.unoffset_canonical), then the skeletal warp inverted per vertex by a
                 damped Newton iteration in HIP (csrc/mesh_pose.hip) -- the model only knows the map from a frame to the
                 canonical body; MeshPoser: pose_mesh with its settings, every frame solved once for all the exports below;
  export_posed   posed/<frame name>.ply per frame -- the faces and colours of mesh.ply, the posed vertices, their normals --
                 and posed.json;
  skin_mesh, rig_frames, export_rig
                 the mesh as a rig (mesh_rig.enable): skin weights read off the motion-weight volume and
                 forward linear blend skinning in HIP (csrc/mesh_rig.hip), the frames' joint transforms as keys of one
                 animation, rigged.glb (occnerf_amd/gltf.py) and rig.json;
  atlas_layout, texture_uv, bake_texture, export_texture
                 the mesh's colour as a texture (mesh_texture.enable): a per-triangle atlas whose texels
                 are canonical points (csrc/mesh_texture.hip), coloured by Network.query_canonical -> texture.png, texture.json
                 and the image inside rigged.glb or a static textured.glb;
  check_photo, project_photos, export_photo_texture
                 the photographs of a prepared dataset on that atlas (mesh_photo.enable): per frame the
                 posed mesh's texels through the frame's camera, tested against the rasteriser's depth keys and the frame's
                 mask and summed in integers (csrc/mesh_texture.hip mesh_texture_project / mesh_texture_blend) ->
                 texture_photo.png (the frames' weighted mean where a frame saw the texel, the colour field elsewhere),
                 texture_seen.png (how many frames saw each texel) and texture_photo.json;
  check_normal, corner_tangents, bake_normal_map, export_normal_map
                 a tangent-space normal map on that atlas (mesh_normal.enable): a fine density grid is
                 the detail source, every texel is projected along the interpolated vertex normal onto its iso-surface and the
                 field's normal there is stored in the frame of the vertex normals and the per-corner tangents
                 (csrc/mesh_normal.hip) -> texture_normal.png, texture_normal.json, TANGENT and normalTexture in the glTF files.

Every step is a pure function of its inputs: the same checkpoint and settings give the same PLY byte for byte (the sidecars
differ in their wall times only).  Decimation, smoothing, hole filling, OBJ, a mesh welded from the f16x3 kernels' field,
area-proportional or merged texture charts, mip-safe padding, object-space normal maps, displacement or occlusion maps (the
normal map's offsets are only reported) and MikkTSpace tangents are not offered; nor, for the posed mesh, roots of
the warp other than the owning bone's or changes of topology; nor, for the photo texture, a robust blend (median, best frame),
exposure compensation between frames, the all_cameras.pkl rig, a pose refined against the photograph or anything that repairs a
wrong mask."""
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


def _clock(dev):
    """The wall time once the device has finished what was queued: every 'seconds' entry of the sidecars is a difference of two."""
    torch.cuda.synchronize(dev)
    return time.perf_counter()


def _write_sidecar(path, info):
    with open(path, 'w') as out:
        json.dump(info, out, indent=1)
        out.write('\n')


def _normals(v, faces, normals):
    """What write_ply and gltf.write_glb take as normals: None when not asked for, zeros for a mesh without triangles."""
    return (vertex_normals(v, faces) if len(faces) else np.zeros_like(v)) if normals else None


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


# ------------------------------------------------------------------ connected components
SNAP = 1024                  # the records' coordinates: 1/1024 of a voxel edge from the box minimum
TABLE_ROWS = 16


def check_components(components):
    """mesh.components as select_components takes it: 'all', 'largest' or a float in (0, 1]; anything else is refused by name."""
    if isinstance(components, str):
        if components in ('all', 'largest'):
            return components
    elif isinstance(components, (int, float, np.integer, np.floating)) and not isinstance(components, (bool, np.bool_)):
        if 0.0 < float(components) <= 1.0:
            return float(components)
    raise RuntimeError(f"mesh.components = {components!r}: 'all', 'largest' or a number in (0, 1] (the share of the largest "
                       "component's triangle count a component needs to stay)")


def check_drop_cavities(drop_cavities):
    if not isinstance(drop_cavities, (bool, np.bool_)):
        raise RuntimeError(f'mesh.drop_cavities = {drop_cavities!r}: True or False')
    return bool(drop_cavities)


def component_table(verts, faces, bbox_min, h, shape):
    """(labels int32 [V] on the device, records, passes): ops.mesh_components on the mesh verts float32 [V,3] / faces int32
    [T,3] over the grid `shape` = (nx, ny, nz) of voxel edge h at bbox_min, the records brought to the host with one copy per
    column: a dict of numpy arrays, one row per component in ascending label order (label, vertices, triangles,
    boundary_vertices int32 [C]; smin, smax int32 [C,3]; volume6_q int64 [C])."""
    labels, rec = ops.mesh_components(verts, faces, bbox_min, h, shape)
    return labels, {k: rec[k].cpu().numpy() for k in ops.MESH_RECORD_COLUMNS}, int(rec['passes'])


def component_verdicts(records, components='all', drop_cavities=False):
    """Per component 'kept', 'small' (the size rule dropped it) or 'cavity' (the size rule kept it; it has no boundary vertex
    and a negative volume).  The size rule comes first and is relative to the largest component of the whole mesh: 'largest'
    keeps the component with the most triangles (ties: the smaller label), a number f every one with triangles >= f * that
    count (in float64)."""
    components, drop_cavities = check_components(components), check_drop_cavities(drop_cavities)
    tri = np.asarray(records['triangles'], dtype=np.int64).reshape(-1)
    n = tri.shape[0]
    if n == 0:
        return []
    if components == 'all':
        keep = np.ones(n, dtype=bool)
    elif components == 'largest':
        keep = np.zeros(n, dtype=bool)
        keep[int(np.argmax(tri))] = True               # the first of equals: the rows ascend by label
    else:
        keep = tri.astype(np.float64) >= np.float64(components) * np.float64(tri.max())
    cavity = (np.asarray(records['boundary_vertices']).reshape(-1) == 0) & \
        (np.asarray(records['volume6_q'], dtype=np.int64).reshape(-1) < 0)
    return ['small' if not k else ('cavity' if drop_cavities and c else 'kept') for k, c in zip(keep, cavity)]


def select_components(records, components='all', drop_cavities=False):
    """bool [C]: which components stay.  A pure host function of the record table."""
    return np.array([v == 'kept' for v in component_verdicts(records, components, drop_cavities)], dtype=bool)


def filter_mesh(verts, faces, labels, keep):
    """(verts [V',3], faces int32 [T',3]) on the device of verts: the components whose flag in keep (bool [C], ascending label
    order) is set.  Kept vertices and triangles keep their order; the indices are remapped by the exclusive scan of the
    vertices' keep flags.  Plumbing: torch indexing and one cumsum."""
    dev = verts.device
    keep = torch.as_tensor(np.asarray(keep, dtype=bool), device=dev)
    vrank, roots = ops.mesh_component_ranks(labels)
    if keep.shape != roots.shape:
        raise RuntimeError(f'filter_mesh: keep holds {tuple(keep.shape)} flags for {int(roots.numel())} components')
    keep_v = keep[vrank.long()] if vrank.numel() else torch.zeros(0, dtype=torch.bool, device=dev)
    new_index = (torch.cumsum(keep_v, 0, dtype=torch.int32) - keep_v.to(torch.int32))
    keep_t = keep_v[faces[:, 0].long()]
    return verts[keep_v].contiguous(), new_index[faces[keep_t].long()].reshape(-1, 3).contiguous()


def components_report(records, verdicts, components, drop_cavities, passes, h, bbox_min):
    """The sidecar's 'components' entry."""
    tri, nv = records['triangles'].astype(np.int64), records['vertices'].astype(np.int64)
    kept = np.array([v == 'kept' for v in verdicts], dtype=bool)
    lo = np.asarray(bbox_min, dtype=np.float64).reshape(3)
    unit = float(h) / SNAP
    rows = []
    for r in sorted(range(len(verdicts)), key=lambda r: (-int(tri[r]), r))[:TABLE_ROWS]:
        rows.append({'label': int(records['label'][r]), 'vertices': int(nv[r]), 'triangles': int(tri[r]),
                     'volume_m3': float(records['volume6_q'][r]) * unit ** 3 / 6.0,
                     'boundary_vertices': int(records['boundary_vertices'][r]),
                     'box_min': (lo + records['smin'][r].astype(np.float64) * unit).tolist(),
                     'box_max': (lo + records['smax'][r].astype(np.float64) * unit).tolist(),
                     'verdict': verdicts[r]})
    return {'policy': {'components': components, 'drop_cavities': bool(drop_cavities)}, 'found': len(verdicts),
            'kept': int(kept.sum()), 'dropped_vertices': int(nv[~kept].sum()), 'dropped_triangles': int(tri[~kept].sum()),
            'cavities_dropped': sum(v == 'cavity' for v in verdicts), 'passes': int(passes), 'largest': rows}


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


def export_mesh(net, out_dir, bbox_min, bbox_max, resolution=256, level=None, normals=True, chunk=1 << 21, keep=None,
                components='all', drop_cavities=False):
    """<out_dir>/mesh.ply and mesh.json of the canonical body -> the sidecar's dict.  keep: a dict that receives what
    export_posed needs of the mesh ('verts' float32 [V,3] on the device, 'faces' int32 [T,3] and 'colors' uint8 [V,3] numpy, 'h'
    the voxel edge, 'level' the float32 level).
    components / drop_cavities: the clean-up of DESIGN.md section 7m; at their defaults nothing is labelled and the files are
    those written without them.  Otherwise the colours, the normals and `keep` are those of the kept mesh, and the sidecar
    gains 'components', 'extracted_vertices' / 'extracted_triangles' and seconds['components']."""
    components, drop_cavities = check_components(components), check_drop_cavities(drop_cavities)
    cleaning = components != 'all' or drop_cavities
    dev = net.point_base.device
    t0 = _clock(dev)
    field, h, (nx, ny, nz) = density_grid(net, bbox_min, bbox_max, resolution, chunk)
    t1 = _clock(dev)
    used = default_level(h) if level is None else float(level)
    lo = np.asarray(bbox_min, dtype=np.float32).reshape(3).astype(np.float64)
    verts, faces = extract_mesh(field, used, lo, h)
    on_boundary = boundary_inside(field, used)
    t2 = t_clean = _clock(dev)
    if cleaning:
        extracted = (int(verts.shape[0]), int(faces.shape[0]))
        labels, records, passes = component_table(verts, faces, lo, h, (nx, ny, nz))
        verdicts = component_verdicts(records, components, drop_cavities)
        verts, faces = filter_mesh(verts, faces, labels, [v == 'kept' for v in verdicts])
        report = components_report(records, verdicts, components, drop_cavities, passes, h, lo)
        t_clean = _clock(dev)
    rgb = torch.sigmoid(net.query_canonical(verts, chunk=chunk)[:, :3])
    colors = to_8b_image(rgb.cpu().numpy())
    t3 = _clock(dev)
    if on_boundary:
        warnings.warn(f'export_mesh: {on_boundary} grid points on the boundary of the box are inside the surface (density above '
                      f'{float(np.float32(used)):g}): the mesh is open there and is written as it is')
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    if keep is not None:
        keep.update(verts=verts, faces=f, colors=colors, h=h, level=float(np.float32(used)))
    os.makedirs(out_dir, exist_ok=True)
    write_ply(os.path.join(out_dir, 'mesh.ply'), v, f, colors, _normals(v, f, normals))
    info = {'resolution': int(resolution), 'h': h, 'level': float(np.float32(used)), 'level_is_default': level is None,
            'grid_shape_xyz': [nx, ny, nz], 'vertices': int(v.shape[0]), 'triangles': int(f.shape[0]),
            'inside_points_on_boundary': on_boundary, 'normals': bool(normals),
            'seconds': {'grid': round(t1 - t0, 4), 'extract': round(t2 - t1, 4), 'colour': round(t3 - t_clean, 4)}}
    if cleaning:
        info.update(extracted_vertices=extracted[0], extracted_triangles=extracted[1], components=report)
        info['seconds']['components'] = round(t_clean - t2, 4)
    _write_sidecar(os.path.join(out_dir, 'mesh.json'), info)
    return info


# ------------------------------------------------------------------ the mesh in the pose of a frame
def pose_mesh(net, verts, data, candidates=3, max_iter=20, tol=1e-7, non_rigid=True, iter_val=1e7, stats=None, preamble=None):
    """(posed float32 [V,3], flag uint8 [V], iters uint8 [V], resid float32 [V]) on the device: where the frame `data` (the
    renderer's per-frame dict: dst_Rs, dst_Ts, dst_posevec, cnl_gtfms, motion_weights_priors as tensors, the box constants) puts
    the canonical vertices `verts`, in the body's own space -- the p the render of that frame maps onto the vertex: the
    non-rigid offset undone (Network.unoffset_canonical; non_rigid False: taken as absent), then ops.mesh_pose on the frame's
    Rs / Ts / motion-weight volume as Network.render_preamble computes them.  flag: 0 solved, 1 not converged, 2 no bone
    carries the vertex.  stats: a dict that receives the rows the fixed point left moving and the wall times.  preamble: what
    net.render_preamble(data, iter_val) returned, where the caller has it."""
    dev = net.point_base.device
    t0 = _clock(dev)
    Rs, Ts, vol = preamble or net.render_preamble(data, iter_val)
    if non_rigid:
        s, moving = net.unoffset_canonical(verts, data, iter_val)
    else:
        s, moving = verts.detach().contiguous(), None
    t1 = _clock(dev)
    out = ops.mesh_pose(s, Rs, Ts, vol[:Rs.shape[0]], ops.host_float3(data['cnl_bbox_min_xyz']),
                        ops.host_float3(data['cnl_bbox_scale_xyz']), candidates=candidates, max_iter=max_iter, tol=tol)
    t2 = _clock(dev)
    if stats is not None:
        stats.update(non_rigid_moving=0 if moving is None else int(moving.sum().item()),
                     seconds={'unoffset': round(t1 - t0, 4), 'pose': round(t2 - t1, 4)})
    return out


class MeshPoser:
    """pose_mesh of one mesh's `verts` with its five settings, every frame solved once.  frame(key, data) -> (Rs, Ts, p, flag,
    iters, resid, stats): the frame's backward bases and pose_mesh's result and stats from one Network.render_preamble call,
    computed at the first call for `key` (the frame's index in its source: one poser serves one source) and kept on the device,
    18 bytes per vertex and frame (keep False: nothing is kept, for an export that asks for every frame once); `solved`
    counts the solves.  A pure function of the inputs: a kept result is the bytes a second solve would give.  The
    motion-weight volume is not kept.  of(poser, ...): the poser an export was handed, refused when it is another mesh's,
    or a new one."""

    def __init__(self, net, verts, candidates=3, max_iter=20, tol=1e-7, non_rigid=True, iter_val=1e7, keep=True):
        self.net, self.verts, self.keep = net, verts, keep
        self.candidates, self.max_iter, self.tol, self.non_rigid, self.iter_val = candidates, max_iter, tol, non_rigid, iter_val
        self.solved, self._frames = 0, {}

    @classmethod
    def of(cls, poser, net, verts, *settings, keep=True):
        if poser is not None and poser.verts is not verts:
            raise RuntimeError("poser: a MeshPoser of other vertices than kept['verts']: its frames are another mesh's")
        return poser or cls(net, verts, *settings, keep=keep)

    def frame(self, key, data):
        found = self._frames.get(key)
        if found is None:
            stats, pre = {}, self.net.render_preamble(data, self.iter_val)
            posed = pose_mesh(self.net, self.verts, data, self.candidates, self.max_iter, self.tol, self.non_rigid, self.iter_val,
                              stats, pre)
            found = (*pre[:2], *posed, stats)
            self.solved += 1
            if self.keep:
                self._frames[key] = found
        *out, stats = found
        return (*out, {**stats, 'seconds': dict(stats['seconds'])})         # the callers add their own wall times


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


def _frame_indices(source, frames, key):
    idxs = list(range(len(source))) if isinstance(frames, str) and frames == 'all' else [int(i) for i in (frames or [])]
    for i in idxs:
        if not 0 <= i < len(source):
            raise RuntimeError(f'{key}: frame {i} outside the {len(source)} frames of the source')
    return idxs


def _device_frame(fr, dev):
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in _POSE_KEYS}
    data.update({k: np.asarray(fr[k], dtype=np.float32) for k in ('cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz')})
    return data


def export_posed(net, out_dir, kept, source, frames, candidates=3, max_iter=20, tol=1e-7, non_rigid=True, world=False,
                 normals=True, iter_val=1e7, poser=None):
    """<out_dir>/posed/<frame name>.ply for the frames (indices into `source`, a PoseFrames; 'all': every one) and
    <out_dir>/posed.json -> its dict.  kept: what export_mesh(keep=...) left of mesh.ply: every posed PLY has its faces and
    colours, the posed vertices and (normals) the normals recomputed from them.  poser: a MeshPoser of kept['verts'] over
    `source` to take the frames from (its settings replace candidates .. iter_val); None: one is built here."""
    dev = net.point_base.device
    idxs = _frame_indices(source, frames, 'mesh_pose.frames')
    verts, faces, colors = kept['verts'], kept['faces'], kept['colors']
    poser = MeshPoser.of(poser, net, verts, candidates, max_iter, tol, non_rigid, iter_val, keep=False)
    os.makedirs(os.path.join(out_dir, 'posed'), exist_ok=True)
    V, per_frame = int(verts.shape[0]), []
    for i in idxs:
        name, fr, Rh, Th = source.frame(i)
        _, _, p, flag, iters, resid, stats = poser.frame(i, _device_frame(fr, dev))
        t0 = time.perf_counter()
        p, flag = p.cpu().numpy(), flag.cpu().numpy()
        if world:
            p = to_world(p, Rh, Th)
        write_ply(os.path.join(out_dir, 'posed', f'{name}.ply'), p, faces, colors, _normals(p, faces, normals))
        stats['seconds']['write'] = round(time.perf_counter() - t0, 4)
        counts = np.bincount(flag, minlength=3)
        per_frame.append({'frame': i, 'name': name, 'converged': int(counts[0]), 'not_converged': int(counts[1]),
                          'no_bone': int(counts[2]), 'flagged_share': float(counts[1] + counts[2]) / max(V, 1),
                          'worst_resid': float(resid.max().item()) if V else 0.0,
                          'mean_iters': float(iters.float().mean().item()) if V else 0.0, **stats})
    info = {'vertices': V, 'candidates': int(poser.candidates), 'max_iter': int(poser.max_iter), 'tol': float(poser.tol),
            'non_rigid': bool(poser.non_rigid and not net.cfg.ignore_non_rigid_motions), 'world': bool(world), 'frames': per_frame}
    _write_sidecar(os.path.join(out_dir, 'posed.json'), info)
    return info


# ------------------------------------------------------------------ the mesh as a rig
RIG_DEFAULTS = {'enable': False, 'frames': None, 'influences': 4, 'fps': 30.0, 'correctives': False, 'max_correctives': 16,
                'max_delta': 0.05, 'world': False}


def check_rig(rig):
    """The mesh_rig keys as export_rig takes them (a dict with every key of RIG_DEFAULTS); a value out of range is refused by
    name."""
    rig = {k: (rig.get(k, v) if hasattr(rig, 'get') else v) for k, v in RIG_DEFAULTS.items()}

    def number(v):
        return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
    for k in ('enable', 'correctives', 'world'):
        if not isinstance(rig[k], (bool, np.bool_)):
            raise RuntimeError(f'mesh_rig.{k} = {rig[k]!r}: True or False')
    if not number(rig['influences']) or rig['influences'] not in (4, 8):
        raise RuntimeError(f"mesh_rig.influences = {rig['influences']!r}: 4 or 8 (JOINTS_0 / WEIGHTS_0, or those and JOINTS_1 / WEIGHTS_1)")
    if not number(rig['fps']) or not 0.0 < float(rig['fps']) < float('inf'):
        raise RuntimeError(f"mesh_rig.fps = {rig['fps']!r}: a positive finite number of keys per second")
    if not number(rig['max_delta']) or not 0.0 <= float(rig['max_delta']) < float('inf'):
        raise RuntimeError(f"mesh_rig.max_delta = {rig['max_delta']!r}: a finite number of metres >= 0")
    if not isinstance(rig['max_correctives'], (int, np.integer)) or isinstance(rig['max_correctives'], (bool, np.bool_)) \
            or rig['max_correctives'] < 1:
        raise RuntimeError(f"mesh_rig.max_correctives = {rig['max_correctives']!r}: a whole number >= 1")
    frames = rig['frames']
    if not (frames is None or frames == 'all' or (isinstance(frames, (list, tuple)) and all(
            isinstance(i, (int, np.integer)) and not isinstance(i, (bool, np.bool_)) for i in frames))):
        raise RuntimeError(f"mesh_rig.frames = {frames!r}: None, 'all' or a list of frame indices")
    return rig


def skin_mesh(net, verts, data, influences=4, iter_val=1e7):
    """(joints uint8 [V,K], weights float32 [V,K], count uint8 [V], kept float32 [V]) on the device: the K = influences (4 or
    8) skinning influences of the canonical vertices, read off the model's motion-weight volume as Network.render_preamble
    returns it (the background channel dropped) by ops.mesh_skin.  The volume is decoded from the subject's priors and the
    module's constants, not from the pose: the `data` of any one frame of the subject serves, and every frame gives the same
    bytes."""
    Rs, _, vol = net.render_preamble(data, iter_val)
    return ops.mesh_skin(verts.detach().contiguous(), vol[:Rs.shape[0]], ops.host_float3(data['cnl_bbox_min_xyz']),
                         ops.host_float3(data['cnl_bbox_scale_xyz']), K=influences)


def joint_transforms(Rs, Ts, cnl_gtfms):
    """G [nb,4,4] float64 = inv([R_b | T_b]) cnl_gtfms_b: where the frame puts every joint, from the frame's backward bases
    (observation -> canonical, float32 [nb,3,3] / [nb,3]) and the canonical global transforms [nb,4,4]."""
    R, T = np.asarray(Rs, dtype=np.float32).astype(np.float64), np.asarray(Ts, dtype=np.float32).astype(np.float64)
    A = np.tile(np.eye(4), (R.shape[0], 1, 1))
    A[:, :3, :3], A[:, :3, 3] = R, T
    return np.linalg.inv(A) @ np.asarray(cnl_gtfms, dtype=np.float32).astype(np.float64)


def local_keys(G, previous=None):
    """(rotation [nb,4] float64 unit quaternions (x, y, z, w), translation [nb,3] float64) of the local transforms
    L_b = inv(G_parent) G_b over synth.SMPL_PARENT, L_0 = G_0; previous: the last key's quaternions, for the sign."""
    from .gltf import PARENTS, quaternion
    rot, tra = np.zeros((G.shape[0], 4)), np.zeros((G.shape[0], 3))
    for b in range(G.shape[0]):
        L = G[b] if PARENTS[b] < 0 else np.linalg.inv(G[PARENTS[b]]) @ G[b]
        rot[b], tra[b] = quaternion(L[:3, :3], None if previous is None else previous[b]), L[:3, 3]
    return rot, tra


def rig_frames(net, source, frames, iter_val=1e7, poser=None):
    """The skeleton's keys for the frames (indices into `source`, a PoseFrames; 'all': every one) -> a dict: 'index', 'name',
    'data' (the frames' device constants) per frame; 'Rs' [F,nb,3,3] / 'Ts' [F,nb,3] on the device, the backward bases of
    Network.render_preamble with the pose refiner in them; 'G' [F,nb,4,4] float64, the global joint transforms
    inv([R_b | T_b]) cnl_gtfms_b; 'rotation' [F,nb,4] / 'translation' [F,nb,3] float64, the local transforms over
    synth.SMPL_PARENT as unit quaternions (Shepperd's branch; the sign of the non-negative dot product with the key before) and
    offsets -- the offset is written per key: it is the rest offset up to the float32 rounding inside Rs / Ts, and with it the
    file reproduces G; 'world_rotation' [F,4] / 'world_translation' [F,3]: R(Rh) and Th, what to_world applies.  poser: a
    MeshPoser over `source` whose frames carry the Rs / Ts (the same bits); None: Network.render_preamble is called here."""
    from .gltf import quaternion
    dev = net.point_base.device
    out = {k: [] for k in ('index', 'name', 'data', 'Rs', 'Ts', 'G', 'rotation', 'translation', 'world_rotation', 'world_translation')}
    for i in _frame_indices(source, frames, 'mesh_rig.frames'):
        name, fr, Rh, Th = source.frame(i)
        data = _device_frame(fr, dev)
        Rs, Ts = (net.render_preamble(data, iter_val) if poser is None else poser.frame(i, data))[:2]
        G = joint_transforms(Rs.cpu().numpy(), Ts.cpu().numpy(), fr['cnl_gtfms'])
        rot, tra = local_keys(G, out['rotation'][-1] if out['rotation'] else None)
        wq = quaternion(np.asarray(Rh, dtype=np.float32).astype(np.float64), out['world_rotation'][-1] if out['world_rotation'] else None)
        for k, v in (('index', i), ('name', name), ('data', data), ('Rs', Rs), ('Ts', Ts), ('G', G), ('rotation', rot),
                     ('translation', tra), ('world_rotation', wq), ('world_translation', np.asarray(Th, dtype=np.float32).astype(np.float64))):
            out[k].append(v)
    if out['index']:
        out['Rs'], out['Ts'] = torch.stack(out['Rs']).contiguous(), torch.stack(out['Ts']).contiguous()
        for k in ('G', 'rotation', 'translation', 'world_rotation', 'world_translation'):
            out[k] = np.stack(out[k])
    return out


def _spread(d):
    d = np.asarray(d, dtype=np.float64)
    if d.size == 0:
        return {'vertices': 0, 'mean': None, 'p99': None, 'max': None}
    return {'vertices': int(d.size), 'mean': float(d.mean()), 'p99': float(np.percentile(d, 99)), 'max': float(d.max())}


def export_rig(net, out_dir, kept, source, rig=None, candidates=3, max_iter=20, tol=1e-7, non_rigid=True, normals=True, iter_val=1e7,
               texture=None, poser=None):
    """<out_dir>/rigged.glb and rig.json -> the sidecar's dict: the kept mesh of export_mesh(keep=...) with a skeleton, skin
    weights (skin_mesh) and, for rig['frames'] of `source` (a PoseFrames), the capture's motion as one animation (rig_frames).
    rig: the mesh_rig keys (RIG_DEFAULTS).  No frames: the rigged rest pose.  Per animated frame rig.json holds how far the
    rig's linear blend skinning (ops.mesh_lbs) is from the model's own posed mesh (pose_mesh with candidates / max_iter / tol /
    non_rigid, over its converged vertices); rig['correctives'] stores that difference as one morph target per frame, so that
    at its key time the file shows the model's mesh.  rig['world']: a node above the root carries R(Rh), Th.  texture: None or
    what export_texture left in kept['texture']: the file carries the atlas instead of COLOR_0, its primitive unwelded (DESIGN.md
    section 7o), and rig.json gains 'textured' and 'unwelded_vertices'.  poser: as for export_posed; a frame it has solved is
    not solved again, the others are where rig_frames asks for their Rs / Ts: seconds['keys'] holds those solves,
    seconds['pose'] the fetching of their results."""
    from . import gltf
    rig = check_rig(RIG_DEFAULTS if rig is None else rig)
    dev = net.point_base.device
    K, correct = int(rig['influences']), bool(rig['correctives'])
    verts, faces, colors = kept['verts'], kept['faces'], kept['colors']
    V = int(verts.shape[0])
    if V == 0 or len(faces) == 0:
        raise RuntimeError(f'mesh_rig: the mesh has {V} vertices and {len(faces)} triangles: there is nothing to rig (on a '
                           'checkpoint without a surface at the default level set mesh.level)')
    idxs = _frame_indices(source, rig['frames'], 'mesh_rig.frames')
    if correct and len(idxs) > int(rig['max_correctives']):
        raise RuntimeError(f"mesh_rig.correctives: {len(idxs)} frames are more than mesh_rig.max_correctives = "
                           f"{int(rig['max_correctives'])}: every frame adds a morph target of {V} x 12 bytes to the file")
    poser = MeshPoser.of(poser, net, verts, candidates, max_iter, tol, non_rigid, iter_val)
    if not poser.keep:
        raise RuntimeError('export_rig: a MeshPoser with keep=False would solve every frame twice, for its key and for its target')
    t0 = _clock(dev)
    keys = rig_frames(net, source, idxs, poser.iter_val, poser)
    t1 = _clock(dev)
    fr0 = source.frame(idxs[0] if idxs else 0)[1]               # the subject's constants: any frame has them
    cnl, data0 = np.asarray(fr0['cnl_gtfms']), keys['data'][0] if idxs else _device_frame(fr0, dev)
    joints, weights, count, kept_share = skin_mesh(net, verts, data0, K, poser.iter_val)
    t2 = _clock(dev)
    F, per_frame, delta = len(idxs), [], None
    t_pose = t_lbs = 0.0
    if F:
        ta = _clock(dev)
        model = [poser.frame(i, data) for i, data in zip(idxs, keys['data'])]       # (solved when rig_frames asked for Rs / Ts)
        tb = _clock(dev)
        target, tflag = torch.stack([m[2] for m in model]).contiguous(), torch.stack([m[3] for m in model]).contiguous()
        x = verts.detach().contiguous()
        if correct:
            posed, delta, dflag = ops.mesh_lbs(x, joints, weights, keys['Rs'], keys['Ts'], target, tflag, float(rig['max_delta']))
        else:
            posed = ops.mesh_lbs(x, joints, weights, keys['Rs'], keys['Ts'])
        t_pose, t_lbs = tb - ta, _clock(dev) - tb
        rest = gltf.rest_translations(cnl)
        dist = (posed.double() - target.double()).norm(dim=2).cpu().numpy()
        solved = tflag.cpu().numpy() == 0
        for f in range(F):
            row = {'frame': idxs[f], 'name': keys['name'][f], 'lbs_to_model_m': _spread(dist[f][solved[f]]),
                   'translation_minus_rest_offset_max_m': float(np.abs(keys['translation'][f] - rest).max())}
            if correct:
                row.update(corrective_flagged=int(dflag[f].sum().item()), corrective_stored=int(V - dflag[f].sum().item()),
                           corrective_max_m=float(delta[f].abs().max().item()))
            per_frame.append(row)
    t3 = _clock(dev)
    v = verts.cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    size = gltf.write_glb(
        os.path.join(out_dir, 'rigged.glb'), v, faces, colors, joints.cpu().numpy(), weights.cpu().numpy(), cnl,
        normals=_normals(v, faces, normals),
        animation={'rotation': keys['rotation'], 'translation': keys['translation']} if F else None,
        world={'rotation': keys['world_rotation'], 'translation': keys['world_translation']} if F and rig['world'] else None,
        correctives=delta.cpu().numpy() if correct and F else None, fps=float(rig['fps']),
        **({} if texture is None else {'texture': _glb_texture(texture)}))
    t4 = time.perf_counter()
    n, share = count.cpu().numpy(), kept_share.cpu().numpy().astype(np.float64)
    bound = share[n > 0]
    info = {'K': K, 'vertices': V, 'triangles': int(len(faces)), 'bytes': int(size), 'fps': float(rig['fps']),
            'influences_histogram': np.bincount(n, minlength=K + 1).tolist(), 'bound_to_root_for_want_of_a_bone': int((n == 0).sum()),
            'kept_share': {'min': float(bound.min()) if bound.size else None, 'mean': float(bound.mean()) if bound.size else None,
                           'p01': float(np.percentile(bound, 1)) if bound.size else None},
            'joint_names': list(gltf.JOINT_NAMES), 'joint_parents': list(gltf.PARENTS),
            'axes': "the body's own space, as mesh.ply: x body left, y up, z front of the canonical body, metres; nothing is "
                    "rotated to glTF's +Y-up, +Z-front convention and nothing is rescaled",
            'correctives': correct, 'max_delta': float(rig['max_delta']), 'world': bool(rig['world']),
            'candidates': int(poser.candidates), 'max_iter': int(poser.max_iter), 'tol': float(poser.tol),
            'non_rigid': bool(poser.non_rigid and not net.cfg.ignore_non_rigid_motions), 'frames': per_frame,
            'seconds': {'keys': round(t1 - t0, 4), 'skin': round(t2 - t1, 4), 'pose': round(t_pose, 4), 'lbs': round(t_lbs, 4),
                        'report': round(t3 - t2 - t_pose - t_lbs, 4), 'write': round(t4 - t3, 4)}}
    if texture is not None:
        info.update(textured=True, unwelded_vertices=3 * int(len(faces)))
        if 'normal_png' in texture:
            info.update(normal_mapped=True)
    _write_sidecar(os.path.join(out_dir, 'rig.json'), info)
    return info


# ------------------------------------------------------------------ the mesh's colour as a texture
TEXTURE_DEFAULTS = {'enable': False, 'cell': 8, 'fill': [0, 0, 0]}


def check_texture(texture):
    """The mesh_texture keys as export_texture takes them (a dict with every key of TEXTURE_DEFAULTS); a value out of range is
    refused by name."""
    texture = {k: (texture.get(k, v) if hasattr(texture, 'get') else v) for k, v in TEXTURE_DEFAULTS.items()}
    if not isinstance(texture['enable'], (bool, np.bool_)):
        raise RuntimeError(f"mesh_texture.enable = {texture['enable']!r}: True or False")
    cell = texture['cell']
    if isinstance(cell, (bool, np.bool_)) or not isinstance(cell, (int, np.integer)) or \
            not ops.MESH_TEXTURE_MIN_CELL <= int(cell) <= ops.MESH_TEXTURE_MAX_CELL:
        raise RuntimeError(f'mesh_texture.cell = {cell!r}: a whole number of texels in {ops.MESH_TEXTURE_MIN_CELL}..'
                           f'{ops.MESH_TEXTURE_MAX_CELL} (the edge of the cell two triangles share)')
    fill = texture['fill']
    if not (isinstance(fill, (list, tuple)) and len(fill) == 3 and all(
            isinstance(c, (int, np.integer)) and not isinstance(c, (bool, np.bool_)) and 0 <= int(c) <= 255 for c in fill)):
        raise RuntimeError(f'mesh_texture.fill = {fill!r}: three whole numbers in 0..255 (the colour of the texels no triangle owns)')
    texture['cell'], texture['fill'] = int(cell), [int(c) for c in fill]
    return texture


def atlas_layout(T, n):
    """(C, R, W, H, P) of the atlas of T triangles at cell edge n: triangles 2c and 2c + 1 share the n x n cell c at column
    c % C, row c // C; C = ceil(sqrt(ceil(T / 2))), R = ceil(ceil(T / 2) / C), W = C n, H = R n, P = n (n - 1) / 2 texels per
    triangle.  W or H above 16384, a cell outside 4..64 and an empty mesh are refused by name."""
    return ops.mesh_texture_layout(T, n)


def texture_uv(T, n):
    """float32 [T,3,2]: per triangle and corner ((x + 0.5) / W, (y + 0.5) / H) of the texel that carries the corner, x / y the
    atlas column / row; image row 0 is v = 0.  In the triangle's own frame the corners are the texels (0, 0), (m, 0), (0, m),
    m = n - 3; an odd triangle's frame is the cell's, mirrored."""
    C, _, W, H, _ = atlas_layout(T, n)
    n, m = int(n), int(n) - 3
    t = np.arange(int(T), dtype=np.int64)
    own = np.array([[0, 0], [m, 0], [0, m]], dtype=np.int64)
    inside = np.where((t & 1)[:, None, None] == 1, n - 1 - own[None], own[None])
    cell = t >> 1
    x = (cell % C)[:, None] * n + inside[..., 0]
    y = (cell // C)[:, None] * n + inside[..., 1]
    return np.stack([(x.astype(np.float64) + 0.5) / np.float64(W), (y.astype(np.float64) + 0.5) / np.float64(H)], -1).astype(np.float32)


def bake_texture(net, verts, faces, n=8, fill=(0, 0, 0), chunk=1 << 21):
    """(atlas uint8 [H,W,3] on the device, stats): the colour field on the per-triangle atlas of the mesh verts float32 [V,3]
    (device) / faces int32 [T,3] (device or numpy): ops.mesh_texel_points, then sigmoid(Network.query_canonical(points)[:, :3])
    in chunks of whole rows (rows are independent: any split gives the same bits), then ops.mesh_texture_fill into an atlas of
    the colour `fill`.  A corner texel's point is its vertex, so its bytes are the vertex colour of mesh.ply."""
    dev = verts.device
    faces = torch.as_tensor(np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1, 3))).to(dev) \
        if not torch.is_tensor(faces) else faces
    T = int(faces.shape[0])
    if T == 0 or int(verts.shape[0]) == 0:
        raise RuntimeError(f'mesh_texture: the mesh has {int(verts.shape[0])} vertices and {T} triangles: there is nothing to bake '
                           '(on a checkpoint without a surface at the default level set mesh.level)')
    C, R, W, H, P = atlas_layout(T, n)
    t0 = _clock(dev)
    pts = ops.mesh_texel_points(verts.detach().contiguous(), faces.contiguous(), int(n)).reshape(-1, 3)
    t1 = _clock(dev)
    rgb = torch.empty(T * P, 3, device=dev)
    step = max(1, int(chunk))
    for r0 in range(0, T * P, step):
        rgb[r0:r0 + step] = torch.sigmoid(net.query_canonical(pts[r0:r0 + step].contiguous(), chunk=chunk)[:, :3])
    t2 = _clock(dev)
    atlas = torch.from_numpy(np.asarray(fill, dtype=np.uint8).reshape(3)).to(dev).expand(H, W, 3).contiguous()
    ops.mesh_texture_fill(rgb, T, int(n), C, atlas)
    t3 = _clock(dev)
    return atlas, {'n': int(n), 'C': C, 'R': R, 'W': W, 'H': H, 'triangles': T, 'texels_queried': T * P,
                   'unowned_share': 1.0 - float(T * P) / float(W * H),
                   'bytes': {'points': T * P * 12, 'colours': T * P * 12, 'atlas': W * H * 3},
                   'seconds': {'points': round(t1 - t0, 4), 'colour': round(t2 - t1, 4), 'fill': round(t3 - t2, 4)}}


def export_texture(net, out_dir, kept, texture=None, chunk=1 << 21):
    """<out_dir>/texture.png (through PIL, as image.py writes) and texture.json of the kept mesh of export_mesh(keep=...) -> the
    sidecar's dict.  texture: the mesh_texture keys (TEXTURE_DEFAULTS).  kept receives 'texture': {'atlas': the device tensor,
    'n', 'C', 'uv': texture_uv's, 'png': the bytes of texture.png}, what gltf.write_glb and mesh_view.export_views take."""
    import io

    from PIL import Image
    texture = check_texture(TEXTURE_DEFAULTS if texture is None else texture)
    verts, faces = kept['verts'], np.asarray(kept['faces'], dtype=np.int32).reshape(-1, 3)
    n = int(texture['cell'])
    atlas, info = bake_texture(net, verts, faces, n, texture['fill'], chunk)
    t0 = time.perf_counter()
    blob = io.BytesIO()
    Image.fromarray(atlas.cpu().numpy()).save(blob, format='PNG')
    png = blob.getvalue()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'texture.png'), 'wb') as out:
        out.write(png)
    v = verts.cpu().numpy().astype(np.float64)
    edge = np.concatenate([np.linalg.norm(v[faces[:, a]] - v[faces[:, b]], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))])
    info.update(fill=list(texture['fill']), texel_edge_m={'mean': float(edge.mean()) / (n - 3), 'max': float(edge.max()) / (n - 3)})
    info['bytes']['png'] = len(png)
    info['seconds']['write'] = round(time.perf_counter() - t0, 4)
    kept['texture'] = {'atlas': atlas, 'n': n, 'C': info['C'], 'uv': texture_uv(len(faces), n), 'png': png}
    _write_sidecar(os.path.join(out_dir, 'texture.json'), info)
    return info


def export_textured(out_dir, kept, normals=True):
    """<out_dir>/textured.glb: the kept mesh with its texture (export_texture has run) as a static glTF binary -> its size."""
    from . import gltf
    v, faces, tex = kept['verts'].cpu().numpy(), kept['faces'], kept['texture']
    return gltf.write_glb(os.path.join(out_dir, 'textured.glb'), v, faces, None, None, None, None,
                          normals=_normals(v, faces, normals), texture=_glb_texture(tex))


def _glb_texture(texture):
    """What gltf.write_glb takes of a kept texture: the colour image and, where with_normal_map has put one in, the normal map."""
    return {k: texture[k] for k in ('uv', 'png', 'normal_png', 'tangents') if k in texture}


def with_normal_map(texture, normal):
    """The kept colour texture (kept['texture'] or kept['texture_photo']) with the normal map of kept['texture_normal'] beside
    it, for export_rig and export_textured: the two share the atlas' layout and TEXCOORD_0."""
    if int(texture['n']) != int(normal['n']) or int(texture['C']) != int(normal['C']):
        raise RuntimeError(f"mesh_normal: the normal map's cells ({normal['n']}, {normal['C']} per row) are not the colour atlas' "
                           f"({texture['n']}, {texture['C']} per row)")
    return {**texture, 'normal_png': normal['png'], 'tangents': normal['tangents']}


# ------------------------------------------------------------------ the normal map of the exported mesh
NORMAL_DEFAULTS = {'enable': False, 'resolution': None, 'cage': None, 'in_glb': True}
NORMAL_MIN_RESOLUTION = 256


def check_normal(normal):
    """The mesh_normal keys as export_normal_map takes them (a dict with every key of NORMAL_DEFAULTS); a value out of range is
    refused by name.  resolution None: max(256, mesh.resolution); cage None: the mesh's own voxel edge."""
    normal = {k: (normal.get(k, v) if hasattr(normal, 'get') else v) for k, v in NORMAL_DEFAULTS.items()}
    for key in ('enable', 'in_glb'):
        if not isinstance(normal[key], (bool, np.bool_)):
            raise RuntimeError(f'mesh_normal.{key} = {normal[key]!r}: True or False')
    res = normal['resolution']
    if res is not None:
        if isinstance(res, (bool, np.bool_)) or not isinstance(res, (int, np.integer)) or not 1 <= int(res) <= 2048:
            raise RuntimeError(f'mesh_normal.resolution = {res!r}: None (max({NORMAL_MIN_RESOLUTION}, mesh.resolution)) or a whole '
                               'number of voxels along the longest axis of the box in 1..2048')
        normal['resolution'] = int(res)
    cage = normal['cage']
    if cage is not None:
        if isinstance(cage, (bool, np.bool_)) or not isinstance(cage, (int, float, np.integer, np.floating)) or \
                not 0.0 < float(cage) < float('inf'):
            raise RuntimeError(f'mesh_normal.cage = {cage!r}: None (the voxel edge of the mesh) or a positive finite number of metres')
        normal['cage'] = float(cage)
    return normal


def corner_tangents(verts, faces, normals, n=None):
    """(tangents float32 [T,3,4], creased bool [T]) of the mesh verts float32 [V,3] / faces int32 [T,3] with the float32 vertex
    normals the file carries, on the host in float64: with e1 = v1 - v0, e2 = v2 - v0 and sigma = +1 for
    an even triangle, -1 for an odd one -- in the per-triangle chart of texture_uv the column grows along sigma e1 and the row
    along sigma e2 --, T_c = normalise(sigma e1 - N_c ((N_c . sigma e1) / (N_c . N_c))) and w = +1.  A triangle with a corner whose vertex normal
    does not lie on the face's front side (N_c . (e1 x e2) <= 0), a zero e1 x e2 or a zero or non-finite T_c is creased: its
    tangents are (1, 0, 0, 1) and the bake gives it the flat normal.  n (the cell edge) does not enter: the chart's axes are
    parallel to e1 and e2 at every n."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    N = np.asarray(normals, dtype=np.float32).astype(np.float64).reshape(-1, 3)[f]
    T = f.shape[0]

    def dot(a, b):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    big = np.finfo(np.float64).max
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    se1 = (np.where(np.arange(T) % 2 == 0, 1.0, -1.0)[:, None] * e1)[:, None, :]
    with np.errstate(all='ignore'):
        t = se1 - N * (dot(N, se1) / dot(N, N))[..., None]
        l2 = dot(t, t)
        ok = (l2 > 0.0) & (l2 <= big)
        t = np.where(ok[..., None], t / np.sqrt(np.where(ok, l2, 1.0))[..., None], t)
        fn = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)
        front = dot(N, fn[:, None, :]) > 0.0
        a2 = dot(fn, fn)
        creased = ~(front.all(1) & ok.all(1) & (a2 > 0.0) & (a2 <= big))
    out = np.concatenate([t, np.ones((T, 3, 1))], -1)
    out[creased] = [1.0, 0.0, 0.0, 1.0]
    return out.astype(np.float32), creased


def bake_normal_map(net, verts, faces, n, level, bbox_min, bbox_max, resolution, cage, chunk=1 << 21):
    """(atlas uint8 [H,W,3], offsets float32 [T,P], flags uint8 [T,P], stats) on the device: the tangent-space normal map of the
    mesh verts float32 [V,3] (device) / faces int32 [T,3] on the atlas of cell edge n.  A density grid of
    `resolution` voxels along the longest axis of the box is computed anew (density_grid); every texel point
    (ops.mesh_texel_points) is projected along the interpolated vertex normal onto that grid's surface at `level`, at most `cage`
    metres away, and the field's normal there is stored in the frame of the vertex normals and corner_tangents
    (ops.mesh_normal_bake).  stats['tangents'] / ['creased'] / ['normals'] are the host arrays the glTF carries."""
    dev = verts.device
    f_np = np.ascontiguousarray(np.asarray(faces.cpu().numpy() if torch.is_tensor(faces) else faces, dtype=np.int32).reshape(-1, 3))
    T, n = int(f_np.shape[0]), int(n)
    if T == 0 or int(verts.shape[0]) == 0:
        raise RuntimeError(f'mesh_normal: the mesh has {int(verts.shape[0])} vertices and {T} triangles: there is nothing to bake '
                           '(on a checkpoint without a surface at the default level set mesh.level)')
    C, R, W, H, P = atlas_layout(T, n)
    h_f, shape = grid_shape(bbox_min, bbox_max, resolution)
    S = ops.mesh_normal_steps(cage, h_f, 'mesh_normal')
    t0 = _clock(dev)
    field, h_f, shape = density_grid(net, bbox_min, bbox_max, resolution, chunk)
    t1 = _clock(dev)
    v_np = verts.detach().cpu().numpy()
    normals = vertex_normals(v_np, f_np).astype(np.float32)
    tangents, creased = corner_tangents(v_np, f_np, normals, n)
    t2 = time.perf_counter()
    faces_d = torch.from_numpy(f_np).to(dev)
    vn_d, tan_d, cr_d = torch.from_numpy(normals).to(dev), torch.from_numpy(tangents).to(dev), torch.from_numpy(creased.astype(np.uint8)).to(dev)
    pts = ops.mesh_texel_points(verts.detach().contiguous(), faces_d, n)
    t3 = _clock(dev)
    atlas = torch.from_numpy(np.array(ops.MESH_NORMAL_FLAT, dtype=np.uint8)).to(dev).expand(H, W, 3).contiguous()
    lo = np.asarray(bbox_min, dtype=np.float32).reshape(3).astype(np.float64)
    level = float(np.float32(level))
    _, offset, flags, normal = ops.mesh_normal_bake(verts.detach().contiguous(), vn_d, faces_d, tan_d, cr_d, pts, n, C, atlas, field,
                                                    lo, h_f, level, S)
    t4 = _clock(dev)
    # how far the texels moved and how much the map adds: the angle between the field's normal and the search direction
    m = n - 3
    ij = torch.tensor([(i, j) for j in range(n - 1) for i in range(n - 1 - j)], device=dev, dtype=torch.float64)
    b = torch.stack([m - ij[:, 0] - ij[:, 1], ij[:, 0], ij[:, 1]], -1)                    # [P,3]
    nh = torch.einsum('pc,tck->tpk', b, vn_d.double()[faces_d.long()])
    nh = nh / nh.norm(dim=-1, keepdim=True).clamp_min(1e-300)
    nf = normal.double()
    ang = torch.rad2deg(torch.atan2(torch.linalg.cross(nh, nf).norm(dim=-1), (nh * nf).sum(-1))).reshape(-1)
    ang = ang[torch.isfinite(ang) & (flags.reshape(-1) & 3 == 0)]
    off = offset.reshape(-1).abs().double()
    off = off[torch.isfinite(off) & (flags.reshape(-1) & 1 == 0)]

    def spread(x, scale=1.0):
        if x.numel() == 0:
            return {'mean': None, 'p99': None, 'max': None}
        s = torch.sort(x).values
        return {'mean': float(s.mean()) * scale, 'p99': float(s[min(s.numel() - 1, int(0.99 * s.numel()))]) * scale,
                'max': float(s[-1]) * scale}
    counts = {name: int((flags & bit != 0).sum().item()) for name, bit in ops.MESH_NORMAL_FLAGS.items()}
    counts['none'] = int((flags == 0).sum().item())
    stats = {'n': n, 'C': C, 'R': R, 'W': W, 'H': H, 'triangles': T, 'texels': T * P, 'resolution': int(resolution),
             'grid_shape_xyz': list(shape), 'h_f': h_f, 'cage': float(cage), 'S': S, 'level': level,
             'samples_per_texel': 2 * S + 7, 'texels_per_flag': counts, 'creased_triangles': int(creased.sum()),
             'offset_m': spread(off), 'angle_to_search_direction_deg': spread(ang),
             'bytes': {'grid': int(field.numel()) * 4, 'points': T * P * 12, 'tangents': T * 48, 'atlas': W * H * 3,
                       'per_texel_outputs': T * P * 17},
             'seconds': {'grid': round(t1 - t0, 4), 'tangents': round(t2 - t1, 4), 'points': round(t3 - t2, 4), 'bake': round(t4 - t3, 4)},
             'tangents': tangents, 'creased': creased, 'normals': normals}
    return atlas, offset, flags, stats


def export_normal_map(net, out_dir, kept, bbox_min, bbox_max, level, mesh_resolution, cell, normal=None, chunk=1 << 21):
    """<out_dir>/texture_normal.png and texture_normal.json of the kept mesh of export_mesh(keep=...) -> the sidecar's dict.
    normal: the mesh_normal keys (NORMAL_DEFAULTS); cell: mesh_texture.cell, so that the map shares the colour atlas' layout and
    TEXCOORD_0.  kept receives 'texture_normal': {'atlas': the device tensor, 'n', 'C', 'png': the bytes of the PNG file,
    'tangents': float32 [T,3,4]}, what gltf.write_glb and mesh_view.export_views take."""
    import io

    from PIL import Image
    normal = check_normal(NORMAL_DEFAULTS if normal is None else normal)
    resolution = max(NORMAL_MIN_RESOLUTION, int(mesh_resolution)) if normal['resolution'] is None else normal['resolution']
    cage = float(kept['h']) if normal['cage'] is None else normal['cage']
    n = int(cell)
    atlas, offset, flags, info = bake_normal_map(net, kept['verts'], kept['faces'], n, level, bbox_min, bbox_max, resolution, cage, chunk)
    tangents = info.pop('tangents')
    info.pop('creased'), info.pop('normals')
    t0 = time.perf_counter()
    blob = io.BytesIO()
    Image.fromarray(atlas.cpu().numpy()).save(blob, format='PNG')
    png = blob.getvalue()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'texture_normal.png'), 'wb') as out:
        out.write(png)
    h = float(kept['h'])
    info['offset_coarse_voxels'] = {k: (None if v is None else v / h) for k, v in info['offset_m'].items()}
    info['bytes']['png'] = len(png)
    info['seconds']['write'] = round(time.perf_counter() - t0, 4)
    total = sum(info['seconds'].values())
    info['share_of_seconds'] = {k: (round(v / total, 4) if total > 0 else None) for k, v in info['seconds'].items()}
    kept['texture_normal'] = {'atlas': atlas, 'n': n, 'C': info['C'], 'png': png, 'tangents': tangents}
    _write_sidecar(os.path.join(out_dir, 'texture_normal.json'), info)
    return info


# ------------------------------------------------------------------ the photographs on the atlas
PHOTO_DEFAULTS = {'enable': False, 'frames': 'all', 'bias': None, 'min_seen': 1, 'in_glb': True}
SEEN_BUCKETS = (('0', 0, 0), ('1', 1, 1), ('2-3', 2, 3), ('4-7', 4, 7), ('8-15', 8, 15), ('16+', 16, (1 << 31) - 1))


def check_photo(photo):
    """The mesh_photo keys as export_photo_texture takes them (a dict with every key of PHOTO_DEFAULTS); a value out of range is
    refused by name."""
    photo = {k: (photo.get(k, v) if hasattr(photo, 'get') else v) for k, v in PHOTO_DEFAULTS.items()}
    for key in ('enable', 'in_glb'):
        if not isinstance(photo[key], (bool, np.bool_)):
            raise RuntimeError(f'mesh_photo.{key} = {photo[key]!r}: True or False')

    def whole(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    frames = photo['frames']
    if not (isinstance(frames, str) and frames == 'all') and not (
            hasattr(frames, '__len__') and not isinstance(frames, str) and len(frames) > 0 and all(whole(i) and int(i) >= 0 for i in frames)):
        raise RuntimeError(f"mesh_photo.frames = {frames!r}: 'all' or a list of frame indices of the prepared dataset, at least one")
    photo['frames'] = frames if isinstance(frames, str) else [int(i) for i in frames]
    bias = photo['bias']
    if bias is not None:
        if isinstance(bias, (bool, np.bool_)) or not isinstance(bias, (int, float, np.integer, np.floating)) or \
                not 0.0 <= float(bias) < float('inf'):
            raise RuntimeError(f'mesh_photo.bias = {bias!r}: None (the voxel edge of the mesh) or a finite number of metres >= 0')
        photo['bias'] = float(bias)
    if not whole(photo['min_seen']) or not 1 <= int(photo['min_seen']) < 1 << 31:
        raise RuntimeError(f"mesh_photo.min_seen = {photo['min_seen']!r}: a whole number of frames >= 1")
    photo['min_seen'] = int(photo['min_seen'])
    return photo


def project_photos(frames_iter, faces, n, bias):
    """(acc int64 [T P,4], seen int32 [T P], per-frame figures): the frames summed onto the atlas of cell edge n of the mesh
    `faces` int32 [T,3] (on the GPU).  frames_iter yields (p float32 [V,3], flag uint8 [V], K, E, photo uint8 [H,W,3], inside
    uint8 [H,W]) with the tensors on the device of faces: the posed vertices and their posing flags, the frame's intrinsics and
    body-space extrinsics (host), the photograph and the mask's inside.  Per frame: ops.mesh_texel_points of the posed vertices,
    ops.mesh_project of the texels and of the vertices, ops.mesh_raster, ops.mesh_texture_project.  Where the posed vertices
    come from is the caller's business."""
    n, T = int(n), int(faces.shape[0])
    dev, P = faces.device, int(n) * (int(n) - 1) // 2
    acc = torch.zeros(T * P, 4, device=dev, dtype=torch.int64)
    seen = torch.zeros(T * P, device=dev, dtype=torch.int32)
    figures, total = [], 0
    for p, flag, K, E, photo, inside in frames_iter:
        H, W = int(photo.shape[0]), int(photo.shape[1])
        p = p.detach().contiguous()
        t0 = _clock(dev)
        q = ops.mesh_texel_points(p, faces, n).reshape(-1, 3)                 # (refuses a face index outside [0, V) by name)
        t1 = _clock(dev)
        xy, z, vflag = ops.mesh_project(q, K, E)
        vxy, vz, vvflag = ops.mesh_project(p, K, E)
        t2 = _clock(dev)
        keys, _ = ops.mesh_raster(faces, vxy, vz, vvflag, H, W, faces_checked=True)
        t3 = _clock(dev)
        tri_w = ops.mesh_texture_project(xy, z, vflag, p, flag, faces, n, K, E, keys, photo, inside, bias, acc, seen)
        t4 = _clock(dev)
        now, away, used = (int(v) for v in torch.stack([seen.sum(), (tri_w < 0).sum(), (tri_w > 0).sum()]).tolist())
        figures.append({'texels_seen': now - total, 'triangles_facing_away': away, 'triangles_weighted': used,
                        'seconds': {'points': round(t1 - t0, 4), 'project': round(t2 - t1, 4), 'raster': round(t3 - t2, 4),
                                    'accumulate': round(t4 - t3, 4)}})
        total = now
    return acc, seen, figures


def seen_histogram(seen):
    """The seen counts of the owned texels in the buckets 0, 1, 2-3, 4-7, 8-15, 16+ -> a dict of whole numbers."""
    counts = torch.stack([((seen >= lo) & (seen <= hi)).sum() for _, lo, hi in SEEN_BUCKETS]).tolist()
    return {name: int(c) for (name, _, _), c in zip(SEEN_BUCKETS, counts)}


def export_photo_texture(net, out_dir, kept, dataset, photo=None, poser=None, candidates=3, max_iter=20, tol=1e-7, non_rigid=True,
                         iter_val=1e7):
    """<out_dir>/texture_photo.png, texture_seen.png and texture_photo.json of the kept mesh, whose field texture export_texture
    has baked (kept['texture']) -> the sidecar's dict.  dataset: a dataset.PreparedDataset; the frames mesh_photo.frames of it are
    posed as export_posed and mesh_view.export_views pose them (poser: a MeshPoser of kept['verts'] over the dataset; None: one
    is built here from candidates .. iter_val), photographed by truth_u8 and masked by gt_alpha > 0.5.  kept receives
    'texture_photo': {'atlas', 'seen' (device tensors), 'n', 'C', 'uv', 'png', 'frames'}."""
    import io

    from PIL import Image
    photo = check_photo(PHOTO_DEFAULTS if photo is None else photo)
    if dataset is None:
        raise RuntimeError('mesh_photo.enable: the photographs and masks are those of a prepared dataset; the synthetic frame '
                           'source has none (set train.dataset_path or movement.dataset)')
    if 'texture' not in kept:
        raise RuntimeError('mesh_photo.enable: the photographs are blended into the atlas of mesh_texture.enable, which is not set')
    dev = net.point_base.device
    tex, verts = kept['texture'], kept['verts']
    n, C = int(tex['n']), int(tex['C'])
    idxs = _frame_indices(dataset, photo['frames'], 'mesh_photo.frames')
    bias = float(kept['h']) if photo['bias'] is None else float(photo['bias'])
    poser = MeshPoser.of(poser, net, verts, candidates, max_iter, tol, non_rigid, iter_val, keep=False)
    f_host = np.ascontiguousarray(np.asarray(kept['faces'], dtype=np.int32).reshape(-1, 3))
    faces = torch.from_numpy(f_host).to(dev)
    T, P = int(f_host.shape[0]), n * (n - 1) // 2
    pose_seconds = []

    def frames_iter():
        for i in idxs:
            f = dataset.frames[i]
            t0 = _clock(dev)
            _, _, p, flag, _, _, _ = poser.frame(i, _device_frame(dataset.host_constants(i), dev))
            pose_seconds.append(_clock(dev) - t0)
            truth = torch.from_numpy(np.ascontiguousarray(dataset.truth_u8(i))).to(dev)
            inside = torch.from_numpy(np.ascontiguousarray((np.asarray(dataset.gt_alpha(i)) > 0.5).astype(np.uint8))).to(dev)
            yield p, flag, f['K'], f['E'], truth, inside
    t0 = _clock(dev)
    acc, seen, figures = project_photos(frames_iter(), faces, n, bias)
    t1 = _clock(dev)
    atlas, seen_img = ops.mesh_texture_blend(acc, seen, T, n, C, tex['atlas'], photo['min_seen'])
    t2 = _clock(dev)
    hist = seen_histogram(seen)
    os.makedirs(out_dir, exist_ok=True)
    blobs = {}
    for name, img in (('texture_photo.png', atlas), ('texture_seen.png', seen_img)):
        blob = io.BytesIO()
        Image.fromarray(img.cpu().numpy()).save(blob, format='PNG')
        blobs[name] = blob.getvalue()
        with open(os.path.join(out_dir, name), 'wb') as out:
            out.write(blobs[name])
    t3 = time.perf_counter()
    for i, row, sec in zip(idxs, figures, pose_seconds):
        row.update(frame=i, name=dataset.frames[i]['frame_name'])
        row['seconds']['pose_and_load'] = round(sec, 4)
    owned = T * P
    info = {'frames': idxs, 'bias_m': bias, 'bias_is_voxel_edge': photo['bias'] is None, 'min_seen': photo['min_seen'],
            'n': n, 'C': C, 'H': int(atlas.shape[0]), 'W': int(atlas.shape[1]), 'triangles': T, 'owned_texels': owned,
            'seen_share': (owned - hist['0']) / owned if owned else None, 'seen_histogram': hist,
            'texels_blended': int((seen >= photo['min_seen']).sum().item()), 'per_frame': figures,
            'bytes': {'accumulators': owned * (4 * 8 + 4), 'png': len(blobs['texture_photo.png']), 'seen_png': len(blobs['texture_seen.png'])},
            'seconds': {'frames': round(t1 - t0, 4), 'pose_and_load': round(sum(pose_seconds), 4), 'blend': round(t2 - t1, 4),
                        'write': round(t3 - t2, 4)}}
    kept['texture_photo'] = {'atlas': atlas, 'seen': seen_img, 'n': n, 'C': C, 'uv': tex['uv'], 'png': blobs['texture_photo.png'],
                             'frames': list(idxs)}
    _write_sidecar(os.path.join(out_dir, 'texture_photo.json'), info)
    return info
