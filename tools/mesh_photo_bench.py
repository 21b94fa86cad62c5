"""Measures the photographs on the atlas (occnerf_amd/mesh.py project_photos / export_photo_texture, csrc/mesh_texture.hip, DESIGN.md
section 7p) on the seeded checkpoint: mesh.resolution 256 with mesh_texture.cell 8, and mesh.resolution 64 with cell 16, on
512 x 512 frames.

    bash tools/mesh_photo_bench.sh           # every step under its own time limit -> profiles/mesh_photo_bench.json

As for the texture row, the iso level is the median of the grid (the seeded weights put no body-shaped surface at the default
level): a surface all over the canonical box.  No trained body is measured.

Steps (each a sub-command, so the shell script can bound each one):
  device    per case and frame: occnerf_mesh_texel_points of the mesh, occnerf_mesh_project (texels and vertices),
            occnerf_mesh_raster and occnerf_mesh_texture_project (its two launches) on a 512 x 512 pinhole view of the canonical
            mesh with a random photograph and a mask that leaves a tenth of the pixels out, and occnerf_mesh_texture_blend once,
            from device events (host enqueue and output allocation included) over `--iters` calls, `--repeats` repeats
            alternating between the cases after a warm-up pass, median and range.  Two calls are compared before anything is
            timed.  The first `SUBSET` triangles of every case, projected on their own, are saved with the device's results;
  export    mesh.export_texture and mesh.export_photo_texture on a tool-made dataset of 4 frames of 512 x 512 by wall clock: the
            frame loop beside the share of posing and loading, and the field's bake the photographs are laid over;
  numpy     the numpy definition (tests/mesh_photo_restatement.py) on the saved subsets, on the host: its time, and its results
            against the device's;
  merge     the partial results as one JSON object."""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((256, 8), (64, 16))            # (mesh.resolution, mesh_texture.cell)
SUBSET = 2000
VIEW, SMALL_VIEW = 512, 96


def _stats(times):
    return {'median': round(float(np.median(times)), 4), 'min': round(float(min(times)), 4), 'max': round(float(max(times)), 4)}


def _camera(size):
    f = 0.9 * size
    K = np.array([[f, 0.0, size / 2.0], [0.0, f, size / 2.0], [0.0, 0.0, 1.0]])
    E = np.eye(4)
    E[2, 3] = 3.0
    return K, E


def _close_camera(size, centre, distance=0.4):
    """A camera looking along +z at `centre` from `distance` metres: the subset of a mesh fills the small frame."""
    K, E = _camera(size)
    E[:3, 3] = [-centre[0], -centre[1], distance - centre[2]]
    return K, E


def _frame_inputs(size, seed, dev=None):
    import torch
    rng = np.random.RandomState(seed)
    photo = rng.randint(0, 256, (size, size, 3)).astype(np.uint8)
    inside = (rng.uniform(size=(size, size)) >= 0.1).astype(np.uint8)
    return (photo, inside) if dev is None else (torch.from_numpy(photo).to(dev), torch.from_numpy(inside).to(dev))


def _meshes():
    import torch
    from occnerf_amd import mesh, synth
    from occnerf_amd.seeded import build_network
    assert torch.cuda.is_available(), 'the photo texture is timed on a GPU only'
    net = build_network(seed=0, S=128, non_rigid=True, device='cuda:0')
    canon = synth.make_frame(img_size=8, with_rays=False)
    lo, hi = canon['cnl_bbox_min_xyz'], canon['cnl_bbox_max_xyz']
    for resolution, n in CASES:
        field, h, shape = mesh.density_grid(net, lo, hi, resolution)
        verts, faces = mesh.extract_mesh(field, float(field.median().item()), lo.astype(np.float64), h)
        del field
        yield net, f'r{resolution}_cell{n}', resolution, n, h, shape, verts, faces.contiguous()


def cmd_device(a):
    import torch
    from occnerf_amd import mesh, ops
    dev = torch.device('cuda', 0)

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / iters

    res, runs, saved, keep = {}, {}, {}, []
    for _, name, resolution, n, h, shape, verts, faces in _meshes():
        V, T = int(verts.shape[0]), int(faces.shape[0])
        C, R, W, H, P = mesh.atlas_layout(T, n)
        N = T * P
        K, E = _camera(VIEW)
        photo, inside = _frame_inputs(VIEW, 1, dev)
        pflag = torch.zeros(V, device=dev, dtype=torch.uint8)

        def one_frame(acc, seen, verts=verts, faces=faces, n=n, K=K, E=E, photo=photo, inside=inside, pflag=pflag, h=h):
            q = ops.mesh_texel_points(verts, faces, n).reshape(-1, 3)
            xy, z, vflag = ops.mesh_project(q, K, E)
            vxy, vz, vvflag = ops.mesh_project(verts, K, E)
            keys, _ = ops.mesh_raster(faces, vxy, vz, vvflag, VIEW, VIEW, faces_checked=True)
            tri_w = ops.mesh_texture_project(xy, z, vflag, verts, pflag, faces, n, K, E, keys, photo, inside, h, acc, seen)
            return q, xy, z, vflag, vxy, vz, vvflag, keys, tri_w
        accs = [torch.zeros(N, 4, device=dev, dtype=torch.int64) for _ in range(2)]
        seens = [torch.zeros(N, device=dev, dtype=torch.int32) for _ in range(2)]
        first, second = one_frame(accs[0], seens[0]), one_frame(accs[1], seens[1])
        assert torch.equal(accs[0], accs[1]) and torch.equal(seens[0], seens[1]) and torch.equal(first[8], second[8])
        q, xy, z, vflag, vxy, vz, vvflag, keys, tri_w = first
        del second
        acc, seen = accs[0], seens[0]
        del accs, seens
        field_atlas = torch.zeros(H, W, 3, device=dev, dtype=torch.uint8)
        out = ops.mesh_texture_blend(acc, seen, T, n, C, field_atlas)
        again = ops.mesh_texture_blend(acc, seen, T, n, C, field_atlas)
        assert torch.equal(out[0], again[0]) and torch.equal(out[1], again[1])
        del again
        n_seen = int((seen > 0).sum().item())
        runs[f'{name}_texel_points'] = lambda v=verts, f=faces, n=n: ops.mesh_texel_points(v, f, n)                        # noqa: E731
        runs[f'{name}_project_texels'] = lambda q=q, K=K, E=E: ops.mesh_project(q, K, E)                                   # noqa: E731
        runs[f'{name}_project_vertices'] = lambda v=verts, K=K, E=E: ops.mesh_project(v, K, E)                             # noqa: E731
        runs[f'{name}_raster'] = lambda f=faces, a=vxy, b=vz, c=vvflag: ops.mesh_raster(f, a, b, c, VIEW, VIEW, faces_checked=True)   # noqa: E731
        runs[f'{name}_texture_project'] = lambda xy=xy, z=z, vf=vflag, v=verts, pf=pflag, f=faces, n=n, K=K, E=E, k=keys, ph=photo, \
            ins=inside, h=h, acc=acc, seen=seen: ops.mesh_texture_project(xy, z, vf, v, pf, f, n, K, E, k, ph, ins, h, acc, seen)   # noqa: E731
        runs[f'{name}_texture_blend'] = lambda acc=acc, seen=seen, T=T, n=n, C=C, at=field_atlas: \
            ops.mesh_texture_blend(acc, seen, T, n, C, at)                                                                  # noqa: E731
        keep.append((q, xy, z, vflag, vxy, vz, vvflag, keys, acc, seen, field_atlas))
        per_texel, per_seen = 1 + 8 + 8, 4 * 8 + 4 + 4 * 3 + 2 * 32 + 2 * 4
        res[name] = {'resolution': resolution, 'cell': n, 'grid_shape_xyz': list(shape), 'vertices': V, 'triangles': T, 'atlas': [W, H],
                     'owned_texels': N, 'frame': [VIEW, VIEW], 'bias_m': h,
                     'texels_seen_in_the_frame': n_seen, 'triangles_facing_away': int((tri_w < 0).sum().item()),
                     'triangles_weighted': int((tri_w > 0).sum().item()),
                     # the whole outputs, for holding two builds of the library against each other (OCCNERF_HIP_LIB)
                     'sha256': {k: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
                                for k, t in (('texel_points', q), ('xy', xy), ('z', z), ('vflag', vflag), ('keys', keys), ('tri_w', tri_w),
                                             ('acc', acc), ('seen', seen), ('photo_atlas', out[0]), ('seen_img', out[1]))},
                     'bytes': {'texel_points': {'read': V * 12 + T * 12, 'written': N * 12},
                               'project_texels': {'read': N * 12, 'written': N * 17},
                               'project_vertices': {'read': V * 12, 'written': V * 17},
                               'raster': {'read': T * 12 + V * 17, 'written': VIEW * VIEW * 8},
                               'texture_project': {'read': T * 12 + N * per_texel + T * 4 + n_seen * (per_seen - 36),
                                                   'written': T * 4 + n_seen * 36,
                                                   'note': 'every texel reads its flag, xy and z; a seen one also 4 keys, 4 mask '
                                                           'bytes, 12 photograph bytes and its 32 + 4 accumulator bytes, which it '
                                                           'writes back; taps are counted per texel, caches ignored'},
                               'texture_blend': {'read': N * 36, 'written': N + 3 * n_seen},
                               'accumulators': N * 36}}
        S = min(SUBSET, T)
        fs = faces[:S].contiguous()
        Ks, Es = _close_camera(SMALL_VIEW, verts[fs.reshape(-1).long()].double().mean(0).cpu().numpy())
        photo_s, inside_s = _frame_inputs(SMALL_VIEW, 2, dev)
        acc_s, seen_s, _ = mesh.project_photos(iter([(verts, pflag, Ks, Es, photo_s, inside_s)]), fs, n, h)
        vxy_s, vz_s, vf_s = ops.mesh_project(verts, Ks, Es)
        keys_s, _ = ops.mesh_raster(fs, vxy_s, vz_s, vf_s, SMALL_VIEW, SMALL_VIEW, faces_checked=True)
        Cs, _, Ws, Hs, _ = mesh.atlas_layout(S, n)
        photo_atlas, seen_img = ops.mesh_texture_blend(acc_s, seen_s, S, n, Cs, torch.full((Hs, Ws, 3), 77, device=dev, dtype=torch.uint8))
        for k, t in (('verts', verts), ('faces', fs), ('keys', keys_s), ('acc', acc_s), ('seen', seen_s), ('photo_atlas', photo_atlas),
                     ('seen_img', seen_img)):
            saved[f'{name}_{k}'] = t.cpu().numpy()
        saved[f'{name}_h'], saved[f'{name}_K'], saved[f'{name}_E'] = np.float64(h), Ks, Es
    np.savez(a.state, **saved)
    for run in runs.values():                                               # warm-up pass
        run()
    reps = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, run in runs.items():                                         # alternating within the call
            reps[k].append(events(run, a.iters))
    res['ms'] = {k: _stats(t) for k, t in reps.items()}
    for name in [k for k in res if k.startswith('r')]:
        res[name]['gb_per_s'] = {k: round((b['read'] + b['written']) / (res['ms'][f'{name}_{k}']['median'] * 1e-3) / 1e9, 1)
                                 for k, b in res[name]['bytes'].items() if isinstance(b, dict)}
    res['what'] = ('seeded checkpoint (seed 0, non-rigid MLP on; no trained body was measured), iso level = median of the grid; per '
                   f'case the whole canonical mesh as the posed one, a {VIEW} x {VIEW} pinhole frame from 3 m with a random photograph '
                   'and a mask without a tenth of its pixels, bias = the voxel edge; device events '
                   f'over {a.iters} calls, host enqueue and output allocation included, {a.repeats} repeats alternating between the '
                   'cases after a warm-up pass; two calls gave equal outputs before timing; gb_per_s = the bytes listed / the median')
    return res


def cmd_export(a):
    import importlib.util

    import torch
    from occnerf_amd import mesh
    from occnerf_amd.dataset import PreparedDataset
    spec = importlib.util.spec_from_file_location('make_synthetic_dataset', os.path.join(ROOT, 'tools', 'make_synthetic_dataset.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    dev = torch.device('cuda', 0)
    res = {}
    with tempfile.TemporaryDirectory() as work:
        path = os.path.join(work, 'ds')
        tool.make_dataset(path, frames=4, width=VIEW, height=VIEW, seed=0)
        ds = PreparedDataset(path, device=None)
        for net, name, resolution, n, h, shape, verts, faces in _meshes():
            kept = {'verts': verts, 'faces': faces.cpu().numpy(), 'h': h}
            out = os.path.join(work, name)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            tex = mesh.export_texture(net, out, kept, {'enable': True, 'cell': n, 'fill': [0, 0, 0]})
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            info = mesh.export_photo_texture(net, out, kept, ds, {**mesh.PHOTO_DEFAULTS, 'enable': True})
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
            res[name] = {'frames': len(info['frames']), 'export_texture_wall_s': round(t1 - t0, 4), 'export_texture_seconds': tex['seconds'],
                         'export_photo_texture_wall_s': round(t2 - t1, 4), 'export_photo_texture_seconds': info['seconds'],
                         'per_frame_seconds': [r['seconds'] for r in info['per_frame']], 'seen_share': info['seen_share'],
                         'seen_histogram': info['seen_histogram']}
    return {'export': res, 'export_what': f'mesh.export_texture, then mesh.export_photo_texture over the 4 frames of a tool-made {VIEW} x '
                                          f'{VIEW} dataset, in one process, by wall clock around synchronised calls, one run; '
                                          "seconds.frames is the frame loop, pose_and_load its share of MeshPoser.frame and of "
                                          'reading the photograph and the mask; the surface is not a body, so few texels are seen'}


def cmd_numpy(a):
    import importlib
    ph = importlib.import_module('tests.mesh_photo_restatement')
    s = np.load(a.state)
    res = {}
    for resolution, n in CASES:
        name = f'r{resolution}_cell{n}'
        faces, verts = s[f'{name}_faces'], s[f'{name}_verts']
        S = faces.shape[0]
        C = ph.mtr.layout(S, n)[0]
        K, E = s[f'{name}_K'], s[f'{name}_E']
        photo, inside = _frame_inputs(SMALL_VIEW, 2)
        acc, seen = ph.accumulators(S, n)
        t0 = time.perf_counter()
        ph.project_frame(faces, n, verts, np.zeros(len(verts), np.uint8), K, E, photo, inside, float(s[f'{name}_h']), acc, seen,
                         keys=s[f'{name}_keys'])
        t1 = time.perf_counter()
        atlas, img = ph.blend(acc, seen, S, n, C, np.full(s[f'{name}_photo_atlas'].shape, 77, np.uint8))
        t2 = time.perf_counter()
        equal = (np.array_equal(acc, s[f'{name}_acc']) and np.array_equal(seen, s[f'{name}_seen'])
                 and np.array_equal(atlas, s[f'{name}_photo_atlas']) and np.array_equal(img, s[f'{name}_seen_img']))
        res[name] = {'triangles': int(S), 'project_frame_ms': round((t1 - t0) * 1e3, 1), 'blend_ms': round((t2 - t1) * 1e3, 1),
                     'frame': [SMALL_VIEW, SMALL_VIEW], 'texels_seen': int((seen > 0).sum()), 'equal_to_the_device': bool(equal)}
    return {'numpy': res, 'numpy_what': f'tests/mesh_photo_restatement.py project_frame (texel points, projection, weights, taps, sums; '
                                        f"the device's keys) and blend on the first {SUBSET} triangles of every case and a {SMALL_VIEW} x "
                                        f"{SMALL_VIEW} frame from 0.4 m in front of their centroid, one run, host; its four outputs compared with the device's"}


def cmd_merge(a):
    out = {}
    for p in a.parts:
        with open(p) as f:
            for k, v in json.load(f).items():
                if isinstance(v, dict) and isinstance(out.get(k), dict):
                    out[k].update(v)
                else:
                    out[k] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    sp = ap.add_subparsers(dest='cmd', required=True)
    d = sp.add_parser('device')
    d.add_argument('--iters', type=int, default=10)
    d.add_argument('--repeats', type=int, default=7)
    d.add_argument('--state', required=True)
    e = sp.add_parser('export')
    n = sp.add_parser('numpy')
    n.add_argument('--state', required=True)
    m = sp.add_parser('merge')
    m.add_argument('parts', nargs='+')
    for p in (d, e, n, m):
        p.add_argument('--out', required=True)
    a = ap.parse_args()
    res = {'device': cmd_device, 'export': cmd_export, 'numpy': cmd_numpy, 'merge': cmd_merge}[a.cmd](a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res)[:2000])


if __name__ == '__main__':
    main()
