"""Measures the texture of the exported mesh (occnerf_amd/mesh.py bake_texture, csrc/mesh_texture.hip) on the
seeded checkpoint: mesh.resolution 256 with mesh_texture.cell 8, and mesh.resolution 64 with cell 16.

    bash tools/mesh_texture_bench.sh           # every step under its own time limit -> profiles/mesh_texture_bench.json

As for the mesh-export row, the iso level is the median of the grid (the seeded weights put no body-shaped surface at the default
level): a surface all over the canonical box.  No trained body is measured.

Steps (each a sub-command, so the shell script can bound each one):
  device    per case: occnerf_mesh_texel_points, occnerf_mesh_texture_fill and occnerf_mesh_resolve_textured (a 512 x 512
            pinhole view of the canonical mesh, beside occnerf_mesh_resolve on the same keys) from device events (host enqueue
            included) over `--iters` calls, `--repeats` repeats alternating between the cases after a warm-up pass, median and
            range; the colour query (sigmoid of Network.query_canonical on every texel point) by wall clock around a
            synchronised call.  The outputs of two calls are compared before anything is timed.  The first `SUBSET` triangles
            of every case, baked and drawn on their own, are saved with the device's results;
  numpy     the numpy definition (tests/mesh_texture_restatement.py, loaded by path) on the saved subsets, on the host: its
            time, and its results against the device's;
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


def cmd_device(a):
    import torch
    from occnerf_amd import mesh, ops, synth
    from occnerf_amd.seeded import build_network
    assert torch.cuda.is_available(), 'the texture is timed on a GPU only'
    dev = torch.device('cuda', 0)
    net = build_network(seed=0, S=128, non_rigid=True, device='cuda:0')
    canon = synth.make_frame(img_size=8, with_rays=False)
    lo, hi = canon['cnl_bbox_min_xyz'], canon['cnl_bbox_max_xyz']

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
    for resolution, n in CASES:
        name = f'r{resolution}_cell{n}'
        field, h, shape = mesh.density_grid(net, lo, hi, resolution)
        verts, faces = mesh.extract_mesh(field, float(field.median().item()), lo.astype(np.float64), h)
        del field
        faces = faces.contiguous()
        V, T = int(verts.shape[0]), int(faces.shape[0])
        C, R, W, H, P = mesh.atlas_layout(T, n)
        pts = ops.mesh_texel_points(verts, faces, n)
        assert torch.equal(pts.view(torch.int32), ops.mesh_texel_points(verts, faces, n).view(torch.int32))
        flat = pts.reshape(-1, 3)
        query = []
        for _ in range(3):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            rgb = torch.sigmoid(net.query_canonical(flat, chunk=1 << 21)[:, :3]).contiguous()
            torch.cuda.synchronize(dev)
            query.append((time.perf_counter() - t0) * 1e3)
        blank = torch.zeros(H, W, 3, device=dev, dtype=torch.uint8)
        atlas = ops.mesh_texture_fill(rgb, T, n, C, blank.clone())
        assert torch.equal(atlas, ops.mesh_texture_fill(rgb, T, n, C, blank.clone()))
        Kc, Ec = _camera(VIEW)
        xy, z, vflag = ops.mesh_project(verts, Kc, Ec)
        keys, counts = ops.mesh_raster(faces, xy, z, vflag, VIEW, VIEW, faces_checked=True)
        colors = (rgb.reshape(T, P, 3)[:, 0] * 255).to(torch.uint8)         # any bytes: the vertex-colour resolve is timed beside
        vcol = torch.zeros(V, 3, device=dev, dtype=torch.uint8)
        vcol[faces[:, 0].long()] = colors
        image = ops.mesh_resolve_textured(keys, faces, xy, z, atlas, n, C, (255, 255, 255))
        assert torch.equal(image, ops.mesh_resolve_textured(keys, faces, xy, z, atlas, n, C, (255, 255, 255)))
        cover, _, _, plain = ops.mesh_resolve(keys, counts.clone(), faces, xy, z, vflag, vcol, (255, 255, 255))
        runs[f'{name}_texel_points'] = lambda v=verts, f=faces, n=n: ops.mesh_texel_points(v, f, n)                       # noqa: E731
        runs[f'{name}_texture_fill'] = lambda r=rgb, T=T, n=n, C=C, at=atlas: ops.mesh_texture_fill(r, T, n, C, at)        # noqa: E731
        runs[f'{name}_resolve_textured'] = lambda k=keys, f=faces, xy=xy, z=z, at=atlas, n=n, C=C: \
            ops.mesh_resolve_textured(k, f, xy, z, at, n, C, (255, 255, 255))                                           # noqa: E731
        runs[f'{name}_resolve_vertex_colours'] = lambda k=keys, c=counts, f=faces, xy=xy, z=z, vf=vflag, vc=vcol: \
            ops.mesh_resolve(k, c.clone(), f, xy, z, vf, vc, (255, 255, 255))                                           # noqa: E731
        keep.append((pts, rgb, atlas, keys, xy, z, vflag, vcol))
        res[name] = {'resolution': resolution, 'cell': n, 'grid_shape_xyz': list(shape), 'vertices': V, 'triangles': T,
                     'atlas': [W, H], 'texels_queried': T * P, 'unowned_share': 1.0 - float(T * P) / float(W * H),
                     'bytes': {'points': T * P * 12, 'colours': T * P * 12, 'atlas': W * H * 3},
                     'view': [VIEW, VIEW], 'view_pixels_covered': int(cover.sum().item()),
                     'colour_query_wall_ms': _stats(query),
                     # the whole outputs, for holding two builds of the library against each other (OCCNERF_HIP_LIB)
                     'sha256': {k: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
                                for k, t in (('atlas', atlas), ('resolve_textured', image), ('resolve_vertex_colours', plain))}}
        # the first SUBSET triangles on their own, for the numpy definition
        S = min(SUBSET, T)
        fs = faces[:S].contiguous()
        Cs, _, Ws, Hs, _ = mesh.atlas_layout(S, n)
        pts_s = ops.mesh_texel_points(verts, fs, n)
        rgb_s = rgb[:S * P].contiguous()
        atlas_s = ops.mesh_texture_fill(rgb_s, S, n, Cs, torch.full((Hs, Ws, 3), 77, device=dev, dtype=torch.uint8))
        Ks, Es = _camera(SMALL_VIEW)
        xy_s, z_s, vflag_s = ops.mesh_project(verts, Ks, Es)
        keys_s, _ = ops.mesh_raster(fs, xy_s, z_s, vflag_s, SMALL_VIEW, SMALL_VIEW, faces_checked=True)
        image_s = ops.mesh_resolve_textured(keys_s, fs, xy_s, z_s, atlas_s, n, Cs, (255, 255, 255))
        for k, t in (('verts', verts), ('faces', fs), ('pts', pts_s), ('rgb', rgb_s), ('atlas', atlas_s), ('xy', xy_s), ('z', z_s),
                     ('keys', keys_s), ('image', image_s)):
            saved[f'{name}_{k}'] = t.cpu().numpy()
    np.savez(a.state, **saved)
    for run in runs.values():                                               # warm-up pass
        run()
    reps = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, run in runs.items():                                         # alternating within the call
            reps[k].append(events(run, a.iters))
    res['ms'] = {k: _stats(t) for k, t in reps.items()}
    res['what'] = ('seeded checkpoint (seed 0, non-rigid MLP on; no trained body was measured), iso level = median of the grid; per '
                   f'case the whole mesh; the view is a {VIEW} x {VIEW} pinhole image of the canonical mesh from 3 m; device events '
                   f'over {a.iters} calls, host enqueue included, {a.repeats} repeats alternating between the cases after a warm-up '
                   'pass; two calls gave equal outputs before timing; the colour query is sigmoid(Network.query_canonical) on every '
                   'texel point by wall clock around a synchronised call, 3 calls')
    return res


def cmd_numpy(a):
    spec = importlib.util.spec_from_file_location('mesh_texture_restatement', os.path.join(ROOT, 'tests', 'mesh_texture_restatement.py'))
    tex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tex)
    s = np.load(a.state)
    res = {}
    for resolution, n in CASES:
        name = f'r{resolution}_cell{n}'
        faces = s[f'{name}_faces']
        S = faces.shape[0]
        C = tex.layout(S, n)[0]
        t0 = time.perf_counter()
        pts, _ = tex.texel_points(s[f'{name}_verts'], faces, n)
        t1 = time.perf_counter()
        atlas = np.full(s[f'{name}_atlas'].shape, 77, np.uint8)
        tex.fill(s[f'{name}_rgb'], S, n, C, atlas)
        t2 = time.perf_counter()
        image = tex.resolve_textured(s[f'{name}_keys'].view(np.uint64), faces, s[f'{name}_xy'], s[f'{name}_z'], atlas, n, C, (255, 255, 255))
        t3 = time.perf_counter()
        equal = (np.array_equal(pts.view(np.uint32), s[f'{name}_pts'].view(np.uint32)) and np.array_equal(atlas, s[f'{name}_atlas'])
                 and np.array_equal(image, s[f'{name}_image']))
        res[name] = {'triangles': int(S), 'texel_points_ms': round((t1 - t0) * 1e3, 1), 'fill_ms': round((t2 - t1) * 1e3, 1),
                     'resolve_textured_ms': round((t3 - t2) * 1e3, 1), 'view': [SMALL_VIEW, SMALL_VIEW],
                     'view_pixels_covered': int((s[f'{name}_keys'].view(np.uint64) != np.uint64(0xFFFFFFFFFFFFFFFF)).sum()),
                     'equal_to_the_device': bool(equal)}
    return {'numpy': res, 'numpy_what': f'tests/mesh_texture_restatement.py texel_points, fill and resolve_textured on the first {SUBSET} '
                                        f'triangles of every case and a {SMALL_VIEW} x {SMALL_VIEW} view of them, one run, host; its '
                                        "three outputs compared with the device's, the points as bit patterns"}


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
