"""Render entry point with the reference's command line (run.py:246-247, configs/config.py:65-72):

    python run.py --cfg configs/occnerf/synthetic/occnerf.yaml --type {tpose,freeview,backview,movement,allview,evaluate,mesh,animate} [KEY VALUE ...]

Frames go to experiments/<category>/<task>/<subject>/<experiment>/<load_net>/<folder>/NNNNNN.png
exactly like the reference (run.py:79-81, image_util.py:53-75).  `load_net: seeded[:N]` renders the
seeded random-init checkpoint (occnerf_amd/checkpoint.py) when no .tar is on disk.  `--type mesh` writes no frames but
<...>/<load_net>/mesh/mesh.ply and mesh.json; with `mesh_pose.frames` also mesh/posed/<frame name>.ply and mesh/posed.json;
with `mesh_view.frames` (a prepared dataset only) also mesh/view/<frame name>.png and mesh/view.json; with `mesh_rig.enable True`
also mesh/rigged.glb, the mesh with a skeleton, skin weights and the motion of `mesh_rig.frames`, and mesh/rig.json; with
`mesh_texture.enable True` also mesh/texture.png, the model's colour on a per-triangle atlas of the mesh; with
`mesh_photo.enable True` also mesh/texture_photo.png, the dataset's photographs projected onto that atlas; with
`mesh_normal.enable True` also mesh/texture_normal.png, a tangent-space normal map of the density field (run_mesh below).
`show_depth` / `show_normal` / `show_shaded True` append the geometry the renderer sees as panels behind [rgb, truth, alpha];
`geometry.save True` writes its raw maps to <folder>_geometry/NNNNNN.npz beside geometry.json (occnerf_amd/gbuffer.py).
`--type animate animate.motion PATH` drives the subject of a prepared dataset with a motion it has not seen (occnerf_amd/
animate.py): frames to <...>/<load_net>/animate/NNNNNN.png, what was rendered to animate.json beside the folder; `show_skeleton
True` puts the driving skeleton directly behind rgb (occnerf_amd/skeleton.py).

Several GPUs: start it under torchrun, one process per GPU --
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 run.py --cfg ... --type movement
every rank renders its share of each frame's rays (occnerf_amd/parallel.py) and rank 0 gathers them over
RCCL, assembles and writes the images."""
import os
import time

import numpy as np
import torch

from configs import cfg, args
cfg.bgcolor = [255., 255., 255.]

from core.data import create_dataloader  # noqa: E402
from core.nets import create_network  # noqa: E402
from occnerf_amd.dataset import resolve_dataset_path  # noqa: E402
from occnerf_amd.image import ImageWriter, assemble_uint8_device  # noqa: E402
from occnerf_amd.parallel import ShardedRenderer  # noqa: E402
from occnerf_amd.sequence import frames_to_device, render_sequence  # noqa: E402


def load_network(model):
    ckpt_path = os.path.join(cfg.logdir, f'{cfg.load_net}.tar')
    if os.path.exists(ckpt_path):
        ckpt = torch.load(ckpt_path, map_location='cpu')
        model.load_state_dict(ckpt['network'], strict=True)
        print('load network from ', ckpt_path)
    elif str(cfg.load_net).startswith('seeded'):
        from occnerf_amd.checkpoint import make_state_dict
        seed = int(str(cfg.load_net).split(':')[1]) if ':' in str(cfg.load_net) else 0
        model.load_state_dict(make_state_dict(model.point_base.detach().numpy(), float(model.bound), seed=seed),
                              strict=True)
        print(f'seeded random-init checkpoint (seed {seed})')
    else:
        raise FileNotFoundError(ckpt_path)
    return model.cuda().deploy_mlps_to_secondary_gpus()


def _init_ranks():
    """One process per GPU under torchrun (RANK / LOCAL_RANK / WORLD_SIZE); a plain launch is world 1.
    OCC_DIST_BACKEND=gloo OCC_FORCE_DEVICE=0 (tests): several ranks share one GPU and exchange through the host -- RCCL
    refuses two ranks per device; everything but the collective itself is then the production path.
    OCC_FORCE_COLLECTIVE=1 under a launcher with ONE rank: the one-rank `nccl` group is formed too and ShardedRenderer takes
    its N > 1 branch (plan, checksum all-gather, device-buffer gather, un-permutation) -- the RCCL path on a single-GPU box."""
    world = int(os.environ.get('WORLD_SIZE', 1))
    rank = int(os.environ.get('RANK', 0))
    torch.cuda.set_device(int(os.environ.get('OCC_FORCE_DEVICE', os.environ.get('LOCAL_RANK', 0))))
    forced = 'WORLD_SIZE' in os.environ and os.environ.get('OCC_FORCE_COLLECTIVE', '0') == '1'
    if (world > 1 or forced) and not torch.distributed.is_initialized():
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        backend = os.environ.get('OCC_DIST_BACKEND', 'nccl')
        if backend == 'nccl':
            torch.distributed.init_process_group('nccl', rank=rank, world_size=world,
                                                 device_id=torch.device('cuda', torch.cuda.current_device()))
        else:
            torch.distributed.init_process_group(backend, rank=rank, world_size=world)
    return rank, world


def _setup(data_type, **loader_kw):
    cfg.perturb = 0.
    rank, world = _init_ranks()
    model = create_network()
    loader = create_dataloader(data_type, **loader_kw)
    model.generate_neural_points(loader.dataset.avg_betas)
    model = load_network(model).eval()
    dev = torch.device('cuda', torch.cuda.current_device())
    return rank, world, model, loader, ShardedRenderer(model, dev), dev


def _finish_ranks(rank, world):
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def _render(data_type, folder_name):
    """run.py:66-119 (_freeview) and :137-186 (run_movement): every frame of the loader through the network, images to
    <logdir>/<load_net>/<folder>/NNNNNN.png.  One process per GPU: each renders its share of the frame's rays, rank 0
    receives the gathered (rgb, alpha, depth) while the ranks already render the NEXT frame (ShardedRenderer: one frame of
    lag), assembles the image on the device and hands the uint8 pixels to the PNG writer thread."""
    rank, world, model, loader, renderer, dev = _setup(data_type)
    writer = ImageWriter(output_dir=os.path.join(cfg.logdir, str(cfg.load_net).replace(':', '_')),
                         exp_name=folder_name) if rank == 0 else None
    stats = {'rays': 0, 'first_s': 0.0, 'per_frame': [], 'frames': 0}
    # the geometry the renderer sees (occnerf_amd/gbuffer.py): the panels behind [rgb, truth, alpha] and
    # the raw maps in the sibling folder <folder>_geometry; every key defaults to off and nothing below runs then
    geo = cfg.get('geometry') or {}
    geo_panels = [k for k in ('depth', 'normal', 'shaded') if cfg.get(f'show_{k}')]
    geo_dir = None
    if rank == 0 and os.path.isdir(writer.image_dir + '_geometry'):
        # the image folder was just recreated: an earlier run's raw maps beside it no longer belong to its PNGs
        import shutil
        shutil.rmtree(writer.image_dir + '_geometry')
    if rank == 0 and geo.get('save'):
        geo_dir = writer.image_dir + '_geometry'
        os.makedirs(geo_dir)
        import json
        with open(os.path.join(geo_dir, 'geometry.json'), 'w') as f:      # the sidecar: what the arrays of every <name>.npz mean
            json.dump({'t': 'float32 [H,W]: the ray PARAMETER depth / alpha of the composited depth (the reference\'s depth); '
                            'the rays are not normalised, the metric distance is t * |d|; 0 where valid bit 0 is clear',
                       'normal': 'float32 [H,W,3]: unit normal facing the camera, in the space of the rays (the body space of '
                                 'the frame\'s camera matrix E), not rotated into the camera; 0 where valid bit 1 is clear',
                       'valid': 'uint8 [H,W]: bit 0 the pixel has a depth (alpha >= min_alpha, alpha > 0, finite values), '
                                'bit 1 it has a normal',
                       't_range': 'float32 [2]: (t_lo, t_hi) of the depth panel\'s grey (t_hi - t) / (t_hi - t_lo)',
                       'min_alpha': float(geo.get('min_alpha', 0.5)),
                       'depth_range': 'per frame: near.min() .. far.max()' if geo.get('depth_range') is None
                       else [float(v) for v in geo.depth_range],
                       'definition': 'DESIGN.md section 7k'}, f, indent=1)
    # --type animate (occnerf_amd/animate.py): what was rendered goes to <folder>.json, and with
    # show_skeleton the driving skeleton from the frame's own camera stands directly behind rgb -- one launch per frame here,
    # on rank 0 after the gather.  No other type takes either branch
    animate_log = [] if data_type == 'animate' and rank == 0 else None
    show_skeleton = data_type == 'animate' and bool(cfg.get('show_skeleton'))
    torch.cuda.synchronize()
    t_wall0 = time.perf_counter()

    def skeleton_of(meta):
        from occnerf_amd.skeleton import skeleton_panel
        v = meta if 'joints' in meta else loader.view(meta['idx'])         # the host route's meta carries no camera
        return skeleton_panel(v['joints'], v['K'], v['E'], meta['height'], meta['width'], dev,
                              bone_px=float(cfg.animate.get('bone_px', 3.0)), bgcolor=cfg.bgcolor)

    def on_frame(out, meta):                           # rank 0 only
        rgb_img, alpha_img = assemble_uint8_device(meta['width'], meta['height'], meta['ray_index'],
                                                   np.array(cfg.bgcolor) / 255., out['rgb'], out['alpha'],
                                                   want_alpha=bool(cfg.show_alpha))
        # the reference's panel order [rgb, truth, alpha] (run.py:109-116, :177-183); the truth panel is the frame's
        # photograph as 8-bit pixels, where the loader has one (a prepared dataset; tpose has none)
        panels = [rgb_img] + ([meta['truth_u8']] if cfg.show_truth and 'truth_u8' in meta else []) + \
            ([alpha_img] if cfg.show_alpha else [])
        if animate_log is not None:
            animate_log.append(dict(loader.describe_frame(meta['idx']), rays=int(meta['ray_index'].numel())))
            if show_skeleton:                              # [rgb, skeleton, alpha, ...]; its count record is read after the run
                skeleton_img, animate_log[-1]['record'] = skeleton_of(meta)
                panels.insert(1, skeleton_img)
        maps = None
        if geo_panels or geo_dir:
            # [rgb, truth, alpha, depth, normal, shaded]: two launches on what rank 0 holds after the gather; the depth range
            # is geometry.depth_range or the frame's own near.min() .. far.max(), reduced on the device
            from occnerf_amd.gbuffer import geometry_maps
            maps = geometry_maps(meta['width'], meta['height'], meta['ray_index'], meta['rays'].to(dev, non_blocking=True),
                                 out['depth'], out['alpha'], min_alpha=float(geo.get('min_alpha', 0.5)),
                                 t_range=geo.get('depth_range'), bgcolor=np.array(cfg.bgcolor) / 255., panels=geo_panels,
                                 near=meta['near'].to(dev, non_blocking=True), far=meta['far'].to(dev, non_blocking=True))
            panels += [maps[f'{k}_u8'] for k in geo_panels]
        img_dev = torch.cat(panels, dim=1) if len(panels) > 1 else rgb_img
        # uint8 over PCIe into a pinned staging buffer; the writer thread waits for the copy and encodes the PNG
        # while the next frame renders (nothing here blocks on the GPU)
        _, name = writer.append_device(img_dev, img_name=f"{meta['idx']:06d}" if data_type in ('movement', 'backview', 'animate') else None)
        if geo_dir:                                        # the raw maps, by the same writer thread and staging scheme
            writer.append_device_npz({k: maps[k] for k in ('t', 'normal', 'valid', 't_range')},
                                     os.path.join(geo_dir, f'{name}.npz'))
        stats['rays'] += int(meta['ray_index'].numel())
        stats['per_frame'].append(int(meta['ray_index'].numel()))
        stats['frames'] += 1
        if meta['idx'] == 0:
            # With one frame of lag this runs after frame 1 has been submitted, so the synchronisation covers frames 0 AND 1
            # (weight packing and the per-model kNN layout included): the steady-state figure below counts neither their
            # time nor their rays.
            torch.cuda.synchronize()
            stats['first_s'] = time.perf_counter() - t_wall0

    render_sequence(renderer, loader, data_type, cfg.eval_iter, on_frame, dev)
    if rank != 0:
        _finish_ranks(rank, world)
        return
    torch.cuda.synchronize()
    t_render = time.perf_counter() - t_wall0
    writer.finalize()
    if animate_log is not None:
        from occnerf_amd.animate import write_json
        from occnerf_amd.skeleton import counts
        for entry in animate_log:
            if 'record' in entry:
                c = counts(entry.pop('record'))
                entry.update(joints_dropped=c['dropped'], pixels_covered=c['covered'])
        write_json(writer.image_dir + '.json', loader, animate_log)
    n_rays = stats['rays']
    print(f'{n_rays} rays in {t_render:.3f} s -> {n_rays / max(t_render, 1e-9):.0f} rays/s (frame generation and image '
          f'assembly included; PNG encoding runs beside it)')
    if stats['frames'] > 2:
        print(f"frames 1-2 (warm-up, pipelined) {stats['first_s'] * 1e3:.0f} ms; frames 3..{stats['frames']}: "
              f"{sum(stats['per_frame'][2:]) / max(t_render - stats['first_s'], 1e-9):.0f} rays/s; wall clock with PNG "
              f'writing {time.perf_counter() - t_wall0:.2f} s')
    _finish_ranks(rank, world)


def PSNR(img1, img2, scale=255.):
    """run.py:21-23."""
    mse = torch.mean((img1 - img2) ** 2)
    return 20 * torch.log10(scale / torch.sqrt(mse))


def run_tpose():
    cfg.ignore_non_rigid_motions = True
    _render('tpose', 'tpose' if not cfg.render_folder_name else cfg.render_folder_name)


def run_freeview():
    _render('freeview', f'freeview_{cfg.freeview.frame_idx}' if not cfg.render_folder_name else cfg.render_folder_name)


def run_movement():
    _render('movement', 'movement' if not cfg.render_folder_name else cfg.render_folder_name)


def run_backview():
    """Every frame of the dataset from the camera behind the first frame's (core/data/occnerf/backview.py)."""
    _render('backview', 'backview' if not cfg.render_folder_name else cfg.render_folder_name)


def run_animate():
    """The subject of the movement source's prepared dataset driven by the motion animate.motion names (occnerf_amd/animate.py;
    the reference has no such type): frames named by their index like movement's, animate.json beside the folder."""
    _render('animate', 'animate' if not cfg.render_folder_name else cfg.render_folder_name)


def run_allview():
    """run.py:188-192: the frame cfg.freeview.frame_idx from every camera of the rig."""
    _render('allview', f'allview_{cfg.freeview.frame_idx}' if not cfg.render_folder_name else cfg.render_folder_name)


def _teacher(loader, dev):
    """The synthetic source has no photographs: its targets are a teacher's render of the same rays, the seeded, amplified
    checkpoint (seed `cfg.evaluate_teacher_seed`, default 1), like train.py's supervision.  -> its ShardedRenderer."""
    from occnerf_amd.checkpoint import make_state_dict
    teacher = create_network()
    teacher.generate_neural_points(loader.dataset.avg_betas)
    seed = int(cfg.get('evaluate_teacher_seed', 1))
    teacher.load_state_dict(make_state_dict(teacher.point_base.detach().numpy(), float(teacher.bound), seed=seed,
                                            amplify=True), strict=True)
    teacher = teacher.to(dev).eval()
    return ShardedRenderer(teacher, dev)


def run_evaluate():
    """run.py:194-244: PSNR of the rendered rays against the frames' target colours over the `progress` frames (frames
    4 and 15 skipped, the network called with iter_val = 1 exactly as the reference does, run.py:224-230: pose refinement
    and the non-rigid condition are then below their kick-in iterations).  The targets are the teacher's render
    (`_teacher`) on the synthetic source and the frames' own `target_rgbs` (the photographs) on a prepared dataset.  The
    paper's metrics -- PSNR and SSIM over the vis / body / full pixels and the silhouette IoU, the reference's eval.py --
    are computed by eval.py at the repository root."""
    rank, world, model, loader, renderer, dev = _setup('progress', evaluate=True)
    on_dataset = resolve_dataset_path(cfg, 'progress') is not None
    teach = None if on_dataset else _teacher(loader, dev)
    psnrs, skips = [], [4, 15]
    with torch.no_grad():
        for data, key, meta in frames_to_device(loader, 'progress', dev):
            if meta['idx'] in skips:
                continue
            target = {'rgb': data['target_rgbs']} if on_dataset else teach.finish(teach.submit(data, iter_val=cfg.eval_iter))
            out = renderer.finish(renderer.submit(data, iter_val=1))       # run.py:224 `batch['iter_val'] = torch.full((1,), 1)`
            if out is not None:
                psnrs.append(PSNR(out['rgb'], target['rgb'], 1.))
    if rank == 0:
        print('AVG PSNR %.4f' % torch.mean(torch.stack(psnrs)))
    _finish_ranks(rank, world)


def run_mesh():
    """The canonical body as a triangle mesh (occnerf_amd/mesh.py; the reference has no such type): the checkpoint loaded as
    run_tpose loads it, the density on a grid over the canonical box the tpose frame of the configured source carries,
    marching tetrahedra in HIP -> <logdir>/<load_net>/mesh/mesh.ply and mesh.json.  With mesh_pose.frames set, also the mesh in
    the pose of those frames of the movement source -> mesh/posed/<frame name>.ply and mesh/posed.json.  With mesh_view.frames
    set, also the posed mesh seen from the camera of those frames of the movement source's prepared dataset (occnerf_amd/
    mesh_view.py) -> mesh/view/<frame name>.png, the mesh beside the photograph, and mesh/view.json with
    the silhouette's IoU against the frame's mask.  With mesh_rig.enable, also the kept mesh as a rigged glTF binary (occnerf_amd/
    mesh.py export_rig) -> mesh/rigged.glb: 24 SMPL joints, skin weights from the motion-weight volume, the
    frames mesh_rig.frames of the movement source as one animation (none: the rest pose), with mesh_rig.correctives a morph
    target per frame that closes the gap to the model's own posed mesh; mesh/rig.json says how large that gap is.  With
    mesh_texture.enable, also the model's colour baked into a per-triangle atlas of the kept mesh (occnerf_amd/mesh.py
    export_texture) -> mesh/texture.png and texture.json; the image replaces the vertex colours in
    rigged.glb, without the rig it goes into a static mesh/textured.glb, and every mesh_view panel gains a textured render.
    With mesh_photo.enable as well (a prepared dataset only), also the photographs of mesh_photo.frames projected onto that atlas
    (occnerf_amd/mesh.py export_photo_texture) -> mesh/texture_photo.png (what the frames saw, the colour
    field elsewhere), texture_seen.png (how many frames saw each texel) and texture_photo.json; with mesh_photo.in_glb the
    glTF files carry that image, and every mesh_view panel gains a photo-textured render.
    With mesh_normal.enable as well (it needs mesh_texture.enable), also a tangent-space normal map on that atlas (occnerf_amd/
    mesh.py export_normal_map): a fine density grid of mesh_normal.resolution voxels is the detail source,
    every texel is projected onto its surface, at most mesh_normal.cage metres away, and the field's normal there is stored in
    the tangent frame of the glTF -> mesh/texture_normal.png and texture_normal.json; with mesh_normal.in_glb (it needs
    mesh.normals) the glTF files carry TANGENT and the map as the material's normalTexture, and every mesh_view panel gains two
    grey renders under a headlight, the geometry's normals beside the map's.
    Rank 0 alone works."""
    from occnerf_amd.mesh import MeshPoser, PoseFrames, export_mesh, export_posed
    ignore_non_rigid = bool(cfg.ignore_non_rigid_motions)
    cfg.ignore_non_rigid_motions = True
    rank, world, model, loader, _, _ = _setup('tpose')
    if rank == 0:
        frame = next(iter(loader))
        box = [np.asarray(torch.as_tensor(frame[k]).cpu().numpy(), dtype=np.float32).reshape(3)
               for k in ('cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz')]
        bbox_max = np.asarray(torch.as_tensor(frame['cnl_bbox_max_xyz']).cpu().numpy(), dtype=np.float32).reshape(3) \
            if 'cnl_bbox_max_xyz' in frame else (box[0] + np.float32(2.0) / box[1]).astype(np.float32)
        m = cfg.mesh
        out_dir = os.path.join(cfg.logdir, str(cfg.load_net).replace(':', '_'),
                               'mesh' if not cfg.render_folder_name else cfg.render_folder_name)
        mp = cfg.get('mesh_pose') or {}
        posing = mp.get('frames') is not None
        mv = cfg.get('mesh_view') or {}
        viewing = mv.get('frames') is not None
        if viewing and resolve_dataset_path(cfg, 'movement') is None:
            raise SystemExit('mesh_view.frames: the silhouette is held against the masks of a prepared dataset; the synthetic frame '
                             'source has none (set train.dataset_path or movement.dataset)')
        mrig = cfg.get('mesh_rig') or {}
        rigging = bool(mrig.get('enable', False))
        if rigging:
            from occnerf_amd.mesh import check_rig
            mrig = check_rig(mrig)
        mtex = cfg.get('mesh_texture') or {}
        texturing = bool(mtex.get('enable', False))
        if texturing:
            from occnerf_amd.mesh import check_texture
            mtex = check_texture(mtex)
        mph = cfg.get('mesh_photo') or {}
        photographing = bool(mph.get('enable', False))
        if photographing:
            from occnerf_amd.mesh import check_photo
            mph = check_photo(mph)
            if not texturing:
                raise SystemExit('mesh_photo.enable: the photographs are blended into the atlas of mesh_texture.enable, which is '
                                 'not set')
            if resolve_dataset_path(cfg, 'movement') is None:
                raise SystemExit('mesh_photo.enable: the photographs and masks are those of a prepared dataset; the synthetic '
                                 'frame source has none (set train.dataset_path or movement.dataset)')
        mnor = cfg.get('mesh_normal') or {}
        mapping = bool(mnor.get('enable', False))
        if mapping:
            from occnerf_amd.mesh import check_normal
            mnor = check_normal(mnor)
            if not texturing:
                raise SystemExit('mesh_normal.enable: the normal map lies on the atlas of mesh_texture.enable, which is not set')
            if mnor['in_glb'] and not bool(m.normals):
                raise SystemExit("mesh_normal.in_glb: glTF's TANGENT is read against NORMAL, and mesh.normals is False")
        kept = {} if posing or viewing or rigging or texturing else None
        info = export_mesh(model, out_dir, box[0], bbox_max, resolution=int(m.resolution), level=m.get('level'),
                           normals=bool(m.normals), chunk=int(m.chunk), keep=kept, components=m.get('components', 'all'),
                           drop_cavities=m.get('drop_cavities', False))
        print(f"mesh: {info['vertices']} vertices, {info['triangles']} triangles on a {info['grid_shape_xyz']} grid at level "
              f"{info['level']:g} -> {os.path.join(out_dir, 'mesh.ply')}")
        if 'components' in info:
            c = info['components']
            print(f"mesh: {c['kept']} of {c['found']} components kept ({c['passes']} labelling passes): {c['dropped_vertices']} "
                  f"vertices and {c['dropped_triangles']} triangles dropped, {c['cavities_dropped']} of the components as cavities")
        if texturing:
            # the colour field baked into a per-triangle atlas of the kept mesh
            from occnerf_amd.mesh import export_texture, export_textured
            tex = export_texture(model, out_dir, kept, mtex, chunk=int(m.chunk))
            print(f"texture: {tex['texels_queried']} texels of {tex['triangles']} triangles in cells of {tex['n']} -> "
                  f"{os.path.join(out_dir, 'texture.png')} ({tex['W']} x {tex['H']}, {100.0 * tex['unowned_share']:.1f} % unowned)")
            if mapping:
                # the density field's normals on the same atlas
                from occnerf_amd.mesh import export_normal_map, with_normal_map
                nm = export_normal_map(model, out_dir, kept, box[0], bbox_max, kept['level'], int(m.resolution), mtex['cell'], mnor,
                                       chunk=int(m.chunk))
                print(f"normal map: {nm['texels']} texels against a {nm['grid_shape_xyz']} grid, {nm['texels_per_flag']['none']} "
                      f"without a flag, {nm['creased_triangles']} creased triangles -> {os.path.join(out_dir, 'texture_normal.png')}")
                if mnor['in_glb']:
                    kept['texture'] = with_normal_map(kept['texture'], kept['texture_normal'])
            if not rigging and not photographing:
                size = export_textured(out_dir, kept, normals=bool(m.normals))
                print(f"texture: the static textured mesh -> {os.path.join(out_dir, 'textured.glb')} ({size} bytes)")
        if posing or rigging or viewing or photographing:
            cfg.ignore_non_rigid_motions = ignore_non_rigid
            solver = dict(candidates=int(mp.get('candidates', 3)), max_iter=int(mp.get('max_iter', 20)),
                          tol=float(mp.get('tol', 1e-7)), non_rigid=bool(mp.get('non_rigid', True)), iter_val=cfg.eval_iter)
        if viewing or photographing:
            # the dataset as --type movement opens it, so K, the mask and the photograph are those of the training size, and a
            # poser of its own, which keeps nothing unless two exports ask for its frames (the dataset's frames are not the
            # indices of the source below)
            from occnerf_amd.dataset import PreparedDataset
            dev = torch.device('cuda', torch.cuda.current_device())
            dataset = PreparedDataset.from_cfg(cfg, resolve_dataset_path(cfg, 'movement'), device=None, prepare_device=dev)
            view_poser = MeshPoser(model, kept['verts'], keep=viewing and photographing, **solver)
        if photographing:
            # the photographs on the atlas: what the frames saw, the colour field elsewhere
            from occnerf_amd.mesh import export_photo_texture, export_textured
            ph = export_photo_texture(model, out_dir, kept, dataset, mph, poser=view_poser)
            print(f"photo texture: {len(ph['frames'])} frames, {100.0 * ph['seen_share']:.1f} % of {ph['owned_texels']} texels seen at "
                  f"least once (depth bias {ph['bias_m']:g} m) -> {os.path.join(out_dir, 'texture_photo.png')}")
            glb_texture = kept['texture']             # (with mesh_normal.in_glb it carries the normal map already)
            if mph['in_glb']:
                glb_texture = kept['texture_photo']
                if mapping and mnor['in_glb']:
                    glb_texture = with_normal_map(glb_texture, kept['texture_normal'])
            if not rigging:
                size = export_textured(out_dir, {**kept, 'texture': glb_texture}, normals=bool(m.normals))
                print(f"texture: the static textured mesh -> {os.path.join(out_dir, 'textured.glb')} ({size} bytes)")
        elif texturing:
            glb_texture = kept['texture']
        if posing or rigging:
            # the movement source's body constants only, and one poser over them: a frame both
            # mesh_pose.frames and mesh_rig.frames name is solved once
            source = PoseFrames(resolve_dataset_path(cfg, 'movement'), total_frames=int(cfg.render_frames),
                                bbox_offset=float(cfg.bbox_offset), volume_size=int(cfg.mweight_volume.volume_size))
            poser = MeshPoser(model, kept['verts'], **solver)
        if posing:
            # the mesh in the pose of frames of the movement source
            posed = export_posed(model, out_dir, kept, source, mp.frames, world=bool(mp.world), normals=bool(m.normals), poser=poser)
            for f in posed['frames']:
                print(f"posed {f['name']}: {f['not_converged']} not converged, {f['no_bone']} without a bone of {posed['vertices']} "
                      f"vertices, worst residual {f['worst_resid']:.3g} m, {f['mean_iters']:.2f} Newton steps per vertex")
        if rigging:
            # the kept mesh with a skeleton, skin weights and the frames' motion as one glTF
            from occnerf_amd.mesh import export_rig
            rigged = export_rig(model, out_dir, kept, source, mrig, normals=bool(m.normals), poser=poser,
                                **({'texture': glb_texture} if texturing else {}))
            print(f"rig: {rigged['vertices']} vertices with up to {rigged['K']} joints each ({rigged['bound_to_root_for_want_of_a_bone']} "
                  f"bound to the root for want of a bone), {len(rigged['frames'])} keys -> {os.path.join(out_dir, 'rigged.glb')} "
                  f"({rigged['bytes']} bytes)")
            for f in rigged['frames']:
                d = f['lbs_to_model_m']
                if d['vertices']:
                    print(f"rig {f['name']}: linear blend skinning is {d['mean']:.3g} m (mean), {d['p99']:.3g} m (99 %), {d['max']:.3g} m "
                          f"(max) from the model's mesh over {d['vertices']} solved vertices")
        if viewing:
            # the posed mesh through each frame's own camera, against the frame's mask: the dataset as
            # --type movement opens it, so K, the mask and the photograph are those of the training size
            from occnerf_amd.mesh_view import export_views
            views = export_views(model, out_dir, kept, dataset, mv.frames, panels=bool(mv.get('panels', True)), bgcolor=cfg.bgcolor,
                                 poser=view_poser,
                                 **({'texture': kept['texture']} if texturing else {}),
                                 **({'photo': kept['texture_photo']} if photographing else {}),
                                 **({'normal': kept['texture_normal']} if mapping else {}))
            for f in views['frames']:
                iou = 'none (empty union)' if f['iou'] is None else f"{f['iou']:.4f}"
                print(f"view {f['name']}: IoU {iou} ({f['intersection']} / {f['union']} pixels), {f['covered']} pixels covered, "
                      f"{sum(f['dropped'].values())} of {views['triangles']} triangles dropped, {f['posing_flagged']} vertices "
                      f"flagged by the posing")
    _finish_ranks(rank, world)


if __name__ == '__main__':
    fn = globals().get(f'run_{args.type}')
    if fn is None:
        raise SystemExit(f"--type {args.type}: supported are tpose, freeview, backview, movement, allview, evaluate, mesh, "
                         'animate')
    fn()
