"""The posed mesh seen from the camera that photographed its frame, and held against that frame's mask (run.py --type mesh
with mesh_view.frames).  The reference draws no geometry; this has no counterpart there.

  rasterize      a triangle mesh through a pinhole camera in HIP (csrc/mesh_raster.hip: project, raster, resolve): per pixel
                 coverage, the nearest triangle, its depth and its interpolated vertex colour.  Screen positions are snapped to
                 1/256 pixel, coverage is integer arithmetic with the top-left fill rule and the depth merge is a 64-bit minimum,
                 so the image is a pure function of its inputs: tests/mesh_raster_restatement.py states it in numpy, and the
                 kernels give its bytes on every run.  Pixel (row i, column j) is sampled at (u, v) = (j, i), where the
                 renderer's rays (synth.get_rays_from_KRT) leave the camera, so the silhouette, the masks and the renderer's
                 alpha map speak about the same pixels;
  silhouette_iou the silhouette against gt_alpha > 0.5 (eval.py's threshold for the ground-truth silhouette): exact integers;
  export_views   per frame of a prepared dataset: the posed mesh (mesh.pose_mesh, in the body's own space) through the frame's K
                 and body-space E -> view/<frame name>.png, the mesh beside the photograph, and view.json.

Not offered: clipping at the near plane (a triangle with a vertex nearer than a millimetre is dropped and counted),
anti-aliasing, lighting and textures other than the baked atlases of mesh_texture.enable and mesh_photo.enable (one more panel
each) and the headlight of mesh_normal.enable (two grey panels, the geometry's normals beside the normal map's; DESIGN.md
section 7q), a comparison of the silhouette with the *rendered* alpha map, and the all_cameras.pkl rig."""
import os

import numpy as np
import torch

from . import ops

COUNTS = ops.MESH_RASTER_COUNTS


def rasterize(verts, faces, colors, K, E, H, W, bgcolor=(255, 255, 255), faces_checked=False, texture=None, photo=None, normal=None):
    """verts float32 [V,3], faces int32 [T,3] and colors uint8 [V,3] on one GPU; K 3x3 and E 4x4 (the camera seen from the space
    of verts) on the host; bgcolor 0..255 -> a dict of device tensors: xy int32 [V,2], z float64 [V], vflag uint8 [V], cover
    uint8 [H,W], tri int32 [H,W] (-1 where empty), depth float32 [H,W] (+inf where empty), rgb uint8 [H,W,3] and counts int32
    [7] in the order COUNTS (triangles dropped per reason, triangles of the wide pass, pixels covered).  Nothing is read back.
    texture: None or a dict with 'atlas' uint8 [aH,aW,3] on the GPU, 'n' and 'C' (mesh.export_texture's): the dict gains
    'rgb_textured' uint8 [H,W,3], the same raster keys resolved through the atlas (ops.mesh_resolve_textured).  photo: None or
    such a dict of the photo atlas (mesh.export_photo_texture's): 'rgb_photo', the keys resolved through that atlas.  normal:
    None or such a dict of the normal atlas (mesh.export_normal_map's): 'shade_geometry' and 'shade_mapped' uint8 [H,W,3], the
    keys lit by a headlight through the interpolated vertex normals and through the normal map (ops.mesh_resolve_lit); the
    normals and corner tangents are those of `verts` as given -- the posed mesh's, recomputed on the host by the functions the
    export uses, so this path reads the vertices back."""
    xy, z, vflag = ops.mesh_project(verts, K, E)
    keys, counts = ops.mesh_raster(faces, xy, z, vflag, H, W, faces_checked=faces_checked)
    cover, tri, depth, rgb = ops.mesh_resolve(keys, counts, faces, xy, z, vflag, colors, bgcolor)
    out = {'xy': xy, 'z': z, 'vflag': vflag, 'cover': cover, 'tri': tri, 'depth': depth, 'rgb': rgb, 'counts': counts}
    if texture is not None:
        out['rgb_textured'] = ops.mesh_resolve_textured(keys, faces, xy, z, texture['atlas'], texture['n'], texture['C'], bgcolor)
    if photo is not None:
        out['rgb_photo'] = ops.mesh_resolve_textured(keys, faces, xy, z, photo['atlas'], photo['n'], photo['C'], bgcolor)
    if normal is not None:
        from .mesh import corner_tangents
        from .synth import vertex_normals
        v, f = verts.detach().cpu().numpy(), faces.cpu().numpy()
        if len(f) and (f.min() < 0 or f.max() >= len(v)):      # the kernels check every index; the host functions index with them
            raise RuntimeError(f'mesh_view.rasterize: normal= needs the posed normals and tangents of every triangle, and a face '
                               f'index lies outside [0, {len(v)})')
        vn = (vertex_normals(v, f) if len(f) else np.zeros_like(v)).astype(np.float32)
        tangents, _ = corner_tangents(v, f, vn, normal['n'])
        out['shade_geometry'], out['shade_mapped'] = ops.mesh_resolve_lit(
            keys, faces, xy, z, torch.from_numpy(vn).to(verts.device), torch.from_numpy(tangents).to(verts.device), normal['atlas'],
            normal['n'], normal['C'], ops.mesh_ray_matrix(K, E), bgcolor)
    return out


def silhouette_iou(cover, gt_alpha):
    """cover uint8 [H,W] and gt_alpha float32 [H,W] on one device -> (intersection, union, IoU, covered, inside share): integer
    counts, IoU = I / U in float64 (None when the union is empty), the share of the covered pixels that lie inside the mask
    (None when nothing is covered).  One blocking copy of three integers."""
    a, b = cover > 0, gt_alpha > 0.5
    inter, union, covered = (int(v) for v in torch.stack([(a & b).sum(), (a | b).sum(), a.sum()]).tolist())
    return inter, union, (inter / union if union else None), covered, (inter / covered if covered else None)


def export_views(net, out_dir, kept, dataset, frames, candidates=3, max_iter=20, tol=1e-7, non_rigid=True, panels=True,
                 bgcolor=(255., 255., 255.), iter_val=1e7, texture=None, poser=None, photo=None, normal=None):
    """<out_dir>/view/<frame name>.png (panels: the mesh render beside the photograph) for the frames (indices into `dataset`,
    a dataset.PreparedDataset; 'all': every one) and <out_dir>/view.json -> its dict.  kept: what export_mesh(keep=...) left of
    mesh.ply.  Every frame is posed here, in memory, as mesh.export_posed poses it (the same call, the same bits).  texture:
    None or what mesh.export_texture left in kept['texture']: every view gets one more panel, the same raster keys resolved
    through the atlas, and view.json per frame 'textured_mean_abs_diff', the mean absolute byte difference between that panel
    and the vertex-colour one over the covered pixels (None when nothing is covered): reported, not judged.  poser: a
    mesh.MeshPoser of kept['verts'] over `dataset` (its settings replace candidates .. iter_val); None: one is built here.
    photo: None or what mesh.export_photo_texture left in kept['texture_photo']: one more panel, the keys resolved through the
    photo atlas, and per frame 'photo_mean_abs_diff', the mean absolute byte difference between that panel and the photograph
    over the pixels covered and inside the mask (None when there is none), and 'projected': whether the frame was among
    mesh_photo.frames -- a frame that was not is held out, and its figure is the honest one.  Reported, not judged.
    normal: None or what mesh.export_normal_map left in kept['texture_normal']: two more panels, the posed mesh under a headlight
    by its vertex normals and by the normal map, and per frame 'lit_mean_abs_diff', the mean absolute byte difference between the
    two over the covered pixels (None when nothing is covered).  Reported, not judged."""
    from .image import ImageWriter
    from .mesh import MeshPoser, _clock, _device_frame, _frame_indices, _write_sidecar
    if dataset is None:
        raise RuntimeError('mesh_view.frames: the silhouette is held against the masks of a prepared dataset; the synthetic frame '
                           'source has none (set train.dataset_path or movement.dataset)')
    dev = net.point_base.device
    idxs = _frame_indices(dataset, frames, 'mesh_view.frames')
    verts = kept['verts']
    poser = MeshPoser.of(poser, net, verts, candidates, max_iter, tol, non_rigid, iter_val, keep=False)
    V, T = int(verts.shape[0]), int(np.asarray(kept['faces']).shape[0])
    f_host = np.ascontiguousarray(np.asarray(kept['faces'], dtype=np.int32).reshape(-1, 3))
    if T and (f_host.min() < 0 or f_host.max() >= V):
        raise RuntimeError(f'mesh_raster: face index outside [0, {V})')
    faces = torch.from_numpy(f_host).to(dev)
    colors = torch.from_numpy(np.ascontiguousarray(np.asarray(kept['colors'], dtype=np.uint8).reshape(-1, 3))).to(dev)
    H, W = int(dataset.height), int(dataset.width)
    os.makedirs(out_dir, exist_ok=True)
    writer = ImageWriter(output_dir=out_dir, exp_name='view') if panels else None
    per_frame = []
    for i in idxs:
        f = dataset.frames[i]
        _, _, p, flag, _, _, stats = poser.frame(i, _device_frame(dataset.host_constants(i), dev))
        t0 = _clock(dev)
        r = rasterize(p, faces, colors, f['K'], f['E'], H, W, bgcolor, faces_checked=True, texture=texture, photo=photo,
                      **({} if normal is None else {'normal': normal}))
        t1 = _clock(dev)
        gt = torch.from_numpy(np.ascontiguousarray(dataset.gt_alpha(i))).to(dev)
        inter, union, iou, covered, inside = silhouette_iou(r['cover'], gt)
        counts = r['counts'].tolist()
        flagged = int((flag != 0).sum().item())
        t2 = _clock(dev)
        truth = torch.from_numpy(np.ascontiguousarray(dataset.truth_u8(i))).to(dev) if writer is not None or photo is not None else None
        if writer is not None:
            writer.append_device(torch.cat([r['rgb']] + ([r['rgb_textured']] if texture is not None else []) +
                                           ([r['rgb_photo']] if photo is not None else []) +
                                           ([r['shade_geometry'], r['shade_mapped']] if normal is not None else []) + [truth], dim=1),
                                 img_name=f['frame_name'])
        stats['seconds'].update(raster=round(t1 - t0, 4), compare=round(t2 - t1, 4))
        per_frame.append({'frame': i, 'name': f['frame_name'], 'iou': iou, 'intersection': inter, 'union': union,
                          'covered': covered, 'inside_share': inside,
                          'dropped': dict(zip(COUNTS[:5], counts[:5])), 'wide': counts[5], 'posing_flagged': flagged,
                          'seconds': stats['seconds']})
        if texture is not None:
            diff = (r['rgb_textured'].int() - r['rgb'].int()).abs()[r['cover'] > 0]
            per_frame[-1]['textured_mean_abs_diff'] = float(diff.double().mean().item()) if covered else None
        if photo is not None:
            diff = (r['rgb_photo'].int() - truth.int()).abs()[(r['cover'] > 0) & (gt > 0.5)]
            per_frame[-1]['photo_mean_abs_diff'] = float(diff.double().mean().item()) if diff.numel() else None
            per_frame[-1]['projected'] = i in photo['frames']
        if normal is not None:
            diff = (r['shade_mapped'][..., 0].int() - r['shade_geometry'][..., 0].int()).abs()[r['cover'] > 0]
            per_frame[-1]['lit_mean_abs_diff'] = float(diff.double().mean().item()) if covered else None
    if writer is not None:
        writer.finalize()
    ious = [f['iou'] for f in per_frame if f['iou'] is not None]
    info = {'vertices': V, 'triangles': T, 'height': H, 'width': W, 'mask_threshold': 0.5,
            'mean_iou': float(np.mean(ious)) if ious else None, 'frames': per_frame}
    _write_sidecar(os.path.join(out_dir, 'view.json'), info)
    return info
