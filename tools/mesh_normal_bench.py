"""Measures the normal map of the exported mesh (occnerf_amd/mesh.py bake_normal_map, csrc/mesh_normal.hip)
on the seeded checkpoint, on the cases of tools/mesh_texture_bench.py: mesh.resolution 256 with mesh_texture.cell 8, and
mesh.resolution 64 with cell 16, both against a bake grid of 256 voxels and a cage of the mesh's own voxel edge.

    bash tools/mesh_normal_bench.sh           # every step under its own time limit -> profiles/mesh_normal_bench.json

As for the texture row, the iso level is the median of the coarse grid (the seeded weights put no body-shaped surface at the
default level): a surface all over the canonical box.  No trained body is measured.

Steps (each a sub-command, so the shell script can bound each one):
  device    per case: occnerf_mesh_normal_bake and occnerf_mesh_resolve_lit (a 512 x 512 pinhole view of the canonical mesh) from
            device events (host enqueue, output allocation and the status read included; the atlas is filled once before) over `--iters` calls, `--repeats` repeats alternating between the cases after a
            warm-up pass, median and range; the fine grid (mesh.density_grid at 256) and the whole mesh.bake_normal_map by wall
            clock around synchronised calls, and the share of the grid's query and of the kernel in that.  The outputs of two
            calls are compared before anything is timed.  The first `SUBSET` triangles of every case, baked on their own, are
            saved with the device's results;
  numpy     the numpy definition (tests/mesh_normal_restatement.py, loaded by path) on the saved subsets, on the host: its time,
            and its four outputs against the device's as bit patterns;
  merge     the partial results as one JSON object."""
import argparse
import hashlib
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((256, 8), (64, 16))            # (mesh.resolution, mesh_texture.cell)
BAKE_RESOLUTION = 256
SUBSET = 2000
VIEW = 512


def _stats(times):
    return {'median': round(float(np.median(times)), 4), 'min': round(float(min(times)), 4), 'max': round(float(max(times)), 4)}


def _camera(size):
    f = 0.9 * size
    K = np.array([[f, 0.0, size / 2.0], [0.0, f, size / 2.0], [0.0, 0.0, 1.0]])
    E = np.eye(4)
    E[2, 3] = 3.0
    return K, E


def cmd_device(a):
    import torch
    from occnerf_amd import mesh, ops, synth
    from occnerf_amd.seeded import build_network
    assert torch.cuda.is_available(), 'the normal map is timed on a GPU only'
    dev = torch.device('cuda', 0)
    net = build_network(seed=0, S=128, non_rigid=True, device='cuda:0')
    canon = synth.make_frame(img_size=8, with_rays=False)
    lo, hi = canon['cnl_bbox_min_xyz'], canon['cnl_bbox_max_xyz']
    lo64 = np.asarray(lo, np.float32).astype(np.float64)

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / iters

    grid_ms = []
    for _ in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fine, h_f, fine_shape = mesh.density_grid(net, lo, hi, BAKE_RESOLUTION)
        torch.cuda.synchronize(dev)
        grid_ms.append((time.perf_counter() - t0) * 1e3)
    res = {'fine_grid': {'resolution': BAKE_RESOLUTION, 'grid_shape_xyz': list(fine_shape), 'h_f': h_f, 'bytes': int(fine.numel()) * 4,
                         'wall_ms': _stats(grid_ms)}}
    runs, saved, keep = {}, {}, []
    for resolution, n in CASES:
        name = f'r{resolution}_cell{n}'
        field, h, shape = mesh.density_grid(net, lo, hi, resolution)
        level = float(np.float32(field.median().item()))
        verts, faces = mesh.extract_mesh(field, level, lo64, h)
        del field
        faces = faces.contiguous()
        v_np, f_np = verts.cpu().numpy(), faces.cpu().numpy()
        V, T = int(verts.shape[0]), int(faces.shape[0])
        C, R, W, H, P = mesh.atlas_layout(T, n)
        S = ops.mesh_normal_steps(h, h_f)
        t0 = time.perf_counter()
        normals = synth.vertex_normals(v_np, f_np).astype(np.float32)
        tangents, creased = mesh.corner_tangents(v_np, f_np, normals, n)
        host_ms = (time.perf_counter() - t0) * 1e3
        vn, tg, cr = (torch.from_numpy(x).to(dev) for x in (normals, tangents, creased.astype(np.uint8)))
        pts = ops.mesh_texel_points(verts, faces, n)

        def flat(H, W):
            return torch.tensor(ops.MESH_NORMAL_FLAT, device=dev, dtype=torch.uint8).expand(H, W, 3).contiguous()

        # the atlas is filled once, outside what is timed: the kernel writes the owned texels only, every other byte stays
        def bake(atlas, fs=faces, tg=tg, cr=cr, pts=pts, C=C, n=n, S=S, level=level, verts=verts, vn=vn):
            return ops.mesh_normal_bake(verts, vn, fs, tg, cr, pts, n, C, atlas, fine, lo64, h_f, level, S)
        first, second = bake(flat(H, W)), bake(flat(H, W))
        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(first, second))
        atlas, offset, flags, normal = first
        Kc, Ec = _camera(VIEW)
        xy, z, vflag = ops.mesh_project(verts, Kc, Ec)
        keys, _ = ops.mesh_raster(faces, xy, z, vflag, VIEW, VIEW, faces_checked=True)
        M = ops.mesh_ray_matrix(Kc, Ec)
        lit = ops.mesh_resolve_lit(keys, faces, xy, z, vn, tg, atlas, n, C, M, (255, 255, 255))
        again = ops.mesh_resolve_lit(keys, faces, xy, z, vn, tg, atlas, n, C, M, (255, 255, 255))
        assert torch.equal(lit[0], again[0]) and torch.equal(lit[1], again[1])
        whole = []
        for _ in range(3):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            _, _, _, stats = mesh.bake_normal_map(net, verts, f_np, n, level, lo, hi, BAKE_RESOLUTION, h)
            torch.cuda.synchronize(dev)
            whole.append((time.perf_counter() - t0) * 1e3)
        runs[f'{name}_normal_bake'] = lambda bake=bake, at=atlas: bake(at)                                               # noqa: E731
        runs[f'{name}_resolve_lit'] = lambda k=keys, f=faces, xy=xy, z=z, vn=vn, tg=tg, at=atlas, n=n, C=C, M=M: \
            ops.mesh_resolve_lit(k, f, xy, z, vn, tg, at, n, C, M, (255, 255, 255))                                       # noqa: E731
        keep.append((pts, atlas, keys, xy, z))
        cover = keys != -1
        diff = (lit[1][..., 0].int() - lit[0][..., 0].int()).abs()[cover]
        res[name] = {'resolution': resolution, 'cell': n, 'vertices': V, 'triangles': T, 'atlas': [W, H], 'texels': T * P,
                     'cage_m': h, 'S': S, 'samples_per_texel': 2 * S + 7, 'taps_per_texel': 8 * (2 * S + 7),
                     'texels_per_flag': stats['texels_per_flag'], 'creased_triangles': stats['creased_triangles'],
                     'offset_m': stats['offset_m'], 'angle_to_search_direction_deg': stats['angle_to_search_direction_deg'],
                     'tangents_host_ms': round(host_ms, 1), 'bake_normal_map_wall_ms': _stats(whole),
                     'bake_normal_map_seconds': stats['seconds'],
                     'view': [VIEW, VIEW], 'view_pixels_covered': int(cover.sum().item()),
                     'lit_mean_abs_diff': float(diff.double().mean().item()) if diff.numel() else None,
                     # the whole outputs, for holding two builds of the library against each other (OCCNERF_HIP_LIB)
                     'sha256': {k: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
                                for k, t in (('atlas', atlas), ('offset', offset), ('flags', flags), ('normal', normal),
                                             ('shade_geometry', lit[0]), ('shade_mapped', lit[1]))}}
        Ts = min(SUBSET, T)
        fs = faces[:Ts].contiguous()
        Cs, _, Ws, Hs, _ = mesh.atlas_layout(Ts, n)
        sub = bake(flat(Hs, Ws), fs=fs, tg=tg[:Ts].contiguous(), cr=cr[:Ts].contiguous(), pts=pts[:Ts].contiguous(), C=Cs)
        for k, t in (('verts', verts), ('faces', fs), ('normals', vn), ('tangents', tg[:Ts]), ('creased', cr[:Ts]), ('pts', pts[:Ts]),
                     ('atlas', sub[0]), ('offset', sub[1]), ('flags', sub[2]), ('normal', sub[3])):
            saved[f'{name}_{k}'] = t.cpu().numpy()
        saved[f'{name}_scalars'] = np.array([h_f, level, S], np.float64)
    saved['field'], saved['lo'] = fine.cpu().numpy(), lo64
    np.savez(a.state, **saved)
    for run in runs.values():                                               # warm-up pass
        run()
    reps = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, run in runs.items():                                         # alternating within the call
            reps[k].append(events(run, a.iters))
    res['ms'] = {k: _stats(t) for k, t in reps.items()}
    for resolution, n in CASES:
        name = f'r{resolution}_cell{n}'
        whole = res[name]['bake_normal_map_wall_ms']['median']
        res[name]['share_of_bake_normal_map'] = {'fine_grid': round(res['fine_grid']['wall_ms']['median'] / whole, 4),
                                                 'kernel': round(res['ms'][f'{name}_normal_bake']['median'] / whole, 4)}
    res['what'] = ('seeded checkpoint (seed 0, non-rigid MLP on; no trained body was measured), iso level = median of the coarse grid, '
                   f'the bake grid at {BAKE_RESOLUTION}, cage = the coarse voxel edge; per case the whole mesh; the view is a {VIEW} x '
                   f'{VIEW} pinhole image of the canonical mesh from 3 m; device events over {a.iters} calls, host enqueue, the '
                   'allocation of the three per-texel outputs and the read of the status word included, the atlas filled once '
                   f'before, {a.repeats} repeats alternating between the cases after a warm-up pass; two calls gave equal '
                   'outputs before timing; the fine grid and the whole bake_normal_map by wall clock around synchronised calls, 3 each')
    return res


def cmd_numpy(a):
    sys.path.insert(0, ROOT)
    spec = importlib.util.spec_from_file_location('mesh_normal_restatement', os.path.join(ROOT, 'tests', 'mesh_normal_restatement.py'))
    nr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(nr)
    s = np.load(a.state)
    res = {}
    for resolution, n in CASES:
        name = f'r{resolution}_cell{n}'
        h_f, level, S = s[f'{name}_scalars']
        t0 = time.perf_counter()
        out = nr.bake(s[f'{name}_verts'], s[f'{name}_faces'], s[f'{name}_normals'], s[f'{name}_tangents'], s[f'{name}_creased'],
                      s[f'{name}_pts'], n, s['field'], s['lo'], h_f, np.float32(level), int(S))
        ms = (time.perf_counter() - t0) * 1e3
        equal = all(np.ascontiguousarray(out[k]).tobytes() == np.ascontiguousarray(s[f'{name}_{k}']).tobytes()
                    for k in ('atlas', 'offset', 'flags', 'normal'))
        res[name] = {'triangles': int(s[f'{name}_faces'].shape[0]), 'bake_ms': round(ms, 1), 'equal_to_the_device': bool(equal)}
    return {'numpy': res, 'numpy_what': f'tests/mesh_normal_restatement.py bake on the first {SUBSET} triangles of every case, one run, '
                                        "host; its four outputs compared with the device's as bit patterns"}


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
    d.add_argument('--iters', type=int, default=5)
    d.add_argument('--repeats', type=int, default=7)
    d.add_argument('--state', required=True)
    n = sp.add_parser('numpy')
    n.add_argument('--state', required=True)
    m = sp.add_parser('merge')
    m.add_argument('parts', nargs='+')
    for p in (d, n, m):
        p.add_argument('--out', required=True)
    a = ap.parse_args()
    res = {'device': cmd_device, 'numpy': cmd_numpy, 'merge': cmd_merge}[a.cmd](a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res)[:2000])


if __name__ == '__main__':
    main()
