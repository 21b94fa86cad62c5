"""Configuration node + defaults for the hot path.

The reference builds a YACS singleton at import time from sys.argv
(configs/config.py:36-72).  The keys the renderer reads are kept with the same names and
default values (configs/default.yaml, configs/occnerf/zju_mocap/387/occnerf.yaml); the
node itself is a small attribute dict with the merge order defaults <- yaml file <- KEY VALUE
list.  `configs/__init__.py` at the repo root exposes `cfg`/`args` under the reference's
import path for the run.py / train.py entry points.
"""
import argparse
import ast
import copy
import os

import yaml


class CfgNode(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v

    def get(self, k, default=None):
        return dict.get(self, k, default)

    @staticmethod
    def wrap(d):
        if isinstance(d, dict) and not isinstance(d, CfgNode):
            return CfgNode({k: CfgNode.wrap(v) for k, v in d.items()})
        return d

    def merge(self, other):
        for k, v in other.items():
            if isinstance(v, dict) and isinstance(self.get(k), dict):
                self[k].merge(v)
            else:
                self[k] = CfgNode.wrap(copy.deepcopy(v))
        return self

    def merge_from_file(self, path):
        with open(path) as f:
            return self.merge(yaml.safe_load(f) or {})

    def merge_from_list(self, opts):
        assert len(opts) % 2 == 0, 'opts must be KEY VALUE pairs'
        for key, val in zip(opts[0::2], opts[1::2]):
            node = self
            parts = key.split('.')
            for p in parts[:-1]:
                node = node[p]
            try:
                val = ast.literal_eval(val)
            except (ValueError, SyntaxError):
                pass
            node[parts[-1]] = val
        return self

    def clone(self):
        return CfgNode.wrap(copy.deepcopy(dict(self)))


_DEFAULTS = {
    'category': 'occnerf', 'task': 'zju_mocap', 'subject': 'p387', 'experiment': 'occnerf',
    'resume': False, 'eval_iter': 10000000, 'render_folder_name': '',
    'ignore_non_rigid_motions': False, 'render_skip': 1, 'render_frames': 100, 'num_workers': 4,
    'network_module': 'core.nets.occnerf.network',
    'embedder': {'module': 'core.nets.occnerf.embedders.fourier'},
    'non_rigid_embedder': {'module': 'core.nets.occnerf.embedders.hannw_fourier'},
    'canonical_mlp': {'module': 'core.nets.occnerf.canonical_mlps.occnerf_mlp', 'mlp_depth': 4,
                      'mlp_width': 256, 'multires': 10, 'i_embed': 0},
    'mweight_volume': {'module': 'core.nets.occnerf.mweight_vol_decoders.deconv_vol_decoder',
                       'embedding_size': 256, 'volume_size': 32, 'dst_voxel_size': 0.0625},
    'non_rigid_motion_mlp': {'module': 'core.nets.occnerf.non_rigid_motion_mlps.mlp_offset',
                             'condition_code_size': 69, 'mlp_width': 128, 'mlp_depth': 6,
                             'skips': [4], 'multires': 6, 'i_embed': 0, 'kick_in_iter': 100000,
                             'full_band_iter': 200000},
    'pose_decoder': {'module': 'core.nets.occnerf.pose_decoders.mlp_delta_body_pose',
                     'embedding_size': 69, 'mlp_width': 256, 'mlp_depth': 4,
                     'kick_in_iter': 2000000},
    'sex': 'neutral', 'total_bones': 24, 'bbox_offset': 0.3, 'load_net': 'latest',
    'N_samples': 128, 'perturb': 1.0, 'netchunk_per_gpu': 300000, 'chunk': 32768, 'n_gpus': 1,
    'bgcolor': [0.0, 0.0, 0.0], 'resize_img_scale': 0.5, 'show_alpha': False, 'show_truth': False,
    'patch': {'sample_subject_ratio': 0.8, 'N_patches': 6, 'size': 32},
    # freeview.src_type: the orbit of the derived cameras (occnerf_amd/views.py) when only train.dataset_path names the
    # dataset: 'zju_mocap' (axis z, inverted angle) or 'wild' (axis y); zju_* / monocular_* dataset names decide it themselves
    'freeview': {'frame_idx': 0, 'src_type': 'zju_mocap'}, 'tpose': {}, 'movement': {},
    # train.dataset_path: a prepared dataset directory (occnerf_amd/dataset.py) -- train.py then trains on it and `movement` /
    # `progress` read it; None: the synthetic subject.  train.images_prescaled: with resize_img_scale != 1, the PNGs are
    # already at the training size (only K is scaled; nothing is resized here).  train.resize_frames: with resize_img_scale
    # != 1, resize every batch and frame to the training size as the reference does (the float64 blend with the Lanczos
    # filter, the mask with the bilinear one; occnerf_amd/resize.py, csrc/resize.hip); False refuses such a scale unless
    # the PNGs are prescaled.  train.prepare_frames: undistort the frames of
    # cameras with 'distortions' and apply crop_image_scale when the dataset is opened (occnerf_amd/dataset.py); False refuses both
    # train.seed: the loader's host RNG (frame order, patch draws, background colours); train.prefetch: build batch t+1 on a
    # side stream while step t runs
    # train.save_checkpt_interval / save_model_interval, save_all, progress.dump_interval: the reference's checkpoint and
    # progress-dump schedule (occnerf_amd/trainer.py; its default.yaml:93-94, :106, :145); progress.dump_interval 0: no dumps.
    # `resume True` continues from <load_net>.tar in the logdir (`latest` where load_net names the seeded checkpoint)
    'train': {'dataset_path': None, 'images_prescaled': False, 'resize_frames': False, 'prepare_frames': True, 'seed': 0, 'prefetch': True,
              'save_checkpt_interval': 2000, 'save_model_interval': 40000},
    'progress': {'dump_interval': 500}, 'save_all': True,
    # the simulated occlusion of the reference's training set (core/data/occnerf/train.py:286-287): the mask columns
    # [mid - width // 2, mid + width // 2) of the first `range` frames of the frame list are zeroed
    'occlude': False, 'occlusion': {'range': 405, 'mid': 451, 'width': 86},
    # eval.py: `eval.lpips True` adds an LPIPS column (weights: the LPIPS model_path / vgg16_path, else the seeded trunk)
    'eval': {'lpips': False, 'lpips_model_path': None, 'lpips_vgg16_path': None},
    # build-specific keys
    'smpl_model': 'auto',            # 'auto' | 'synthetic' | directory holding the SMPL pickles
    # samples resident per pipeline pass (~470 B each): 2^28 keeps a whole 1024^2 x 192 frame (141 M samples, 63 GiB peak of the
    # 288 GB) in ONE pass; larger frames run in several, bit-identically.  The renderer additionally caps a pass at half of
    # the device memory that is free when the frame starts (Network.forward: min(this, free / 2 / 470 B)), so a smaller GPU
    # or ranks sharing one device split a large frame instead of running out of memory.
    'max_samples_per_pass': 1 << 28,
    # 'fp32': exact fp32 MFMA (default, the parity/benchmark path); 'f16x3': split-fp16 MFMA with scaled pieces, 22
    # significand bits per operand -- fp32-grade (csrc/split.h; domain: hidden activations below 4 094); 'bf16x3':
    # split-bf16 MFMA, 16 bits per operand (meets the pixel gate on the random-init checkpoint only)
    'mlp_precision': 'fp32',
    # mlp_precision='f16x3': True / 'sync' reads the kernels' out-of-domain flag after the frame and re-renders in fp32 when set;
    # 'deferred' checks it when a later frame starts / in Network.check_f16x3_domain() and raises; False: no check
    'f16x3_domain_check': True,
    'train_fused_trunks': True,      # bf16 training step: the trunks' forward as one kernel (csrc/trunks.hip); False: ten layer passes
    'skip_empty_samples': True,      # drop samples whose motion-weight sum is exactly 0 (identical pixels)
    'device_rays': True,             # run.py: generate the frame's ray batch on the GPU (occnerf_amd/rays.py)
    'device_frames': True,           # movement / progress / eval.py on a prepared dataset: build each frame on the GPU (csrc/frame.hip)
    'ray_patch_order': True,         # render rays in Morton-ordered pixel patches (any order is exact)
    'knn_culling': True,             # cluster-culled exact kNN (False: brute force)
    'knn_center_cache': True,        # kNN queries within a proven radius of the frame's collapse point take its cached lists (same bits)
    'warp_bone_culling': True,       # warp kernel skips bones whose weight channel cannot reach a wave's samples (same bits)
    # run.py --type mesh (occnerf_amd/mesh.py): resolution = voxels along the longest axis of the canonical box; level = the
    # iso density, None: ln 2 / h (one voxel edge of matter half opaque); normals: write vertex normals; chunk: points per
    # Network.query_canonical chunk; components: 'all' (nothing is labelled), 'largest' (only the connected component with the
    # most triangles stays) or a number f in (0, 1] (every component with at least f x the largest one's triangles stays);
    # drop_cavities: also drop closed components that enclose negative volume
    'mesh': {'resolution': 256, 'level': None, 'normals': True, 'chunk': 1 << 21, 'components': 'all', 'drop_cavities': False},
    # run.py --type mesh, the mesh in the pose of frames (occnerf_amd/mesh.py export_posed): frames = None
    # (canonical mesh only), a list of frame indices of the movement source, or 'all'; candidates / max_iter / tol = the bones
    # tried per vertex, the Newton steps per bone and the residual (metres, on the fp64 iterate) that counts as converged;
    # non_rigid: undo the frame's non-rigid offset too; world: write R(Rh) p + Th instead of the body's own space
    'mesh_pose': {'frames': None, 'candidates': 3, 'max_iter': 20, 'tol': 1e-7, 'non_rigid': True, 'world': False},
    # run.py --type mesh, the mesh as a rigged, animated glTF (occnerf_amd/mesh.py export_rig): enable
    # writes mesh/rigged.glb and rig.json; frames = None (the rigged rest pose), a list of frame indices of the movement source,
    # or 'all': the keys of the animation, fps of them per second; influences: 4 or 8 joints per vertex; correctives: store per
    # frame the difference between the rig's linear blend skinning and the model's own posed mesh (the mesh_pose keys apply) as
    # a morph target -- at most max_correctives frames, each target is vertices x 12 bytes --, none longer than max_delta metres;
    # world: a node above the root carries R(Rh), Th
    'mesh_rig': {'enable': False, 'frames': None, 'influences': 4, 'fps': 30.0, 'correctives': False, 'max_correctives': 16,
                 'max_delta': 0.05, 'world': False},
    # run.py --type mesh, the mesh's colour as a texture (occnerf_amd/mesh.py export_texture): enable
    # writes mesh/texture.png and texture.json and puts the image into rigged.glb (mesh_rig.enable) or else into a static
    # mesh/textured.glb, in place of the vertex colours; cell: the edge in texels (4..64) of the atlas cell two triangles share
    # -- a triangle's edge spans cell - 3 texels --; fill: the colour 0..255 of the texels no triangle owns
    'mesh_texture': {'enable': False, 'cell': 8, 'fill': [0, 0, 0]},
    # run.py --type mesh, the photographs of the prepared dataset on the atlas (occnerf_amd/mesh.py export_photo_texture, DESIGN.md
    # section 7p; needs mesh_texture.enable and a prepared dataset): enable writes mesh/texture_photo.png (what the frames saw,
    # the colour field elsewhere), texture_seen.png (how many frames saw each texel) and texture_photo.json; frames: 'all' or a
    # list of frame indices; bias: the depth tolerance in metres of the visibility test (None: the mesh's voxel edge); min_seen:
    # the frames that must have seen a texel before their mean replaces the field's colour; in_glb: the photo atlas goes into
    # rigged.glb / textured.glb in place of texture.png
    'mesh_photo': {'enable': False, 'frames': 'all', 'bias': None, 'min_seen': 1, 'in_glb': True},
    # run.py --type mesh, a tangent-space normal map of the density field on the atlas (occnerf_amd/mesh.py export_normal_map,
    # DESIGN.md section 7q; needs mesh_texture.enable): enable writes mesh/texture_normal.png and texture_normal.json;
    # resolution: the voxels along the longest axis of the fine density grid the detail is read from (None:
    # max(256, mesh.resolution)); cage: how far in metres a texel may lie from that grid's surface (None: the mesh's voxel
    # edge); in_glb: rigged.glb / textured.glb carry TANGENT and the map as materials[0].normalTexture (needs mesh.normals)
    'mesh_normal': {'enable': False, 'resolution': None, 'cage': None, 'in_glb': True},
    # run.py --type mesh, the posed mesh seen from its frame's camera (occnerf_amd/mesh_view.py export_views, DESIGN.md section
    # 7j): frames = None (nothing happens), a list of frame indices of the movement source's prepared dataset, or 'all'; per
    # frame the silhouette's IoU with the frame's mask goes to mesh/view.json; panels: also write mesh/view/<frame name>.png, the
    # mesh render beside the photograph.  The frames are posed with the mesh_pose keys
    'mesh_view': {'frames': None, 'panels': True},
    # run.py tpose / freeview / backview / movement / allview, the geometry the volume renderer sees (occnerf_amd/gbuffer.py,
    # DESIGN.md section 7k): show_depth / show_normal / show_shaded add a panel each behind [rgb, truth, alpha].
    # geometry.min_alpha: a pixel has a depth where its accumulated alpha reaches this; geometry.depth_range: [t_lo, t_hi] of
    # the depth panel's grey, None: the frame's own near.min() .. far.max() (it follows the frame's box, so the grey of a
    # movement sequence flickers: fix the range there); geometry.save: also write each frame's t, normal, valid and t_range
    # to <folder>_geometry/<name>.npz.  t is the ray parameter of the unnormalised rays, the metric distance is t |d|
    'show_depth': False, 'show_normal': False, 'show_shaded': False,
    'geometry': {'min_alpha': 0.5, 'depth_range': None, 'save': False},
    # run.py --type animate (occnerf_amd/animate.py): the subject of the movement source's prepared dataset
    # driven by animate.motion, a prepared dataset directory (only its mesh_infos.pkl is read) or an .npz with poses [T,72] and
    # optionally Rh / Th.  frame_idx: the subject's source frame (its skeleton, its calibrated camera, where the motion is put);
    # substeps n: n - 1 slerped frames between consecutive frames of the motion; align: map the motion's frame 0 onto the
    # source frame's Rh / Th (False: take Rh / Th as they are -- a motion of the subject's own capture); camera: 'fixed' (the
    # body moves through the image), 'follow' (it turns on the spot) or 'orbit' (follow, the camera turning as freeview's
    # does, one turn in render_frames frames); bone_px: a bone's half-width in the skeleton panel.  show_skeleton: the
    # driving skeleton from the frame's camera as a panel directly behind rgb (occnerf_amd/skeleton.py); animate only
    'animate': {'motion': None, 'frame_idx': 0, 'substeps': 1, 'align': True, 'camera': 'fixed', 'bone_px': 3.0},
    'show_skeleton': False,
}
# resolution + 1 points on the longest axis, at most as many on the others: the default grid stays below the kernels' 2^31
assert (_DEFAULTS['mesh']['resolution'] + 1) ** 3 < 1 << 31

_cfg = None


def default_cfg():
    return CfgNode.wrap(copy.deepcopy(_DEFAULTS))


def get_cfg():
    global _cfg
    if _cfg is None:
        _cfg = default_cfg()
        _finish(_cfg)
    return _cfg


def set_cfg(cfg):
    global _cfg
    _cfg = cfg
    return cfg


def _finish(cfg):
    import torch
    cfg.logdir = os.path.join('experiments', cfg.category, cfg.task, cfg.subject, cfg.experiment)
    n = torch.cuda.device_count()
    cfg.n_gpus = n
    cfg.primary_gpus = [0] if n > 0 else ['cpu']
    cfg.secondary_gpus = ([g for g in range(n) if g != 0] or cfg.primary_gpus) if n > 1 \
        else cfg.primary_gpus


def make_cfg(argv=None):
    """Same CLI as the reference (configs/config.py:65-72): --cfg FILE [--type T] [KEY VALUE ...]."""
    parser = argparse.ArgumentParser()
    parser.add_argument('--cfg', required=True, type=str)
    parser.add_argument('--eval', default='full', type=str)
    parser.add_argument('--type', default='skip', type=str)
    parser.add_argument('opts', default=None, nargs=argparse.REMAINDER)
    args = parser.parse_args(argv)
    cfg = default_cfg()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    default_yaml = os.path.join(here, 'configs', 'default.yaml')
    if os.path.exists(default_yaml):
        cfg.merge_from_file(default_yaml)
    cfg.merge_from_file(args.cfg)
    cfg.merge_from_list(args.opts or [])
    _finish(cfg)
    set_cfg(cfg)
    return cfg, args
