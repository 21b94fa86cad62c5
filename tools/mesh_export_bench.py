"""Measures the mesh export (occnerf_amd/mesh.py) on the seeded checkpoint at mesh.resolution 128 and
256, the sizes a user runs: the density grid, the three kernels of csrc/mesh.hip, the welding and the colour query.

    bash tools/mesh_export_bench.sh            # every step under its own time limit -> profiles/mesh_export_bench.json

The seeded weights put no body-shaped surface at the default level ln 2 / h, so the iso level is the median of each grid: half
of the grid points are inside and the surface is far larger than a body's -- an upper bound on the extraction's work.

Steps (each a sub-command, so the shell script can bound each one):
  device    per resolution: wall time of density_grid and of the colour query (synchronised, second call); device events around count +
            row scan + emit + vertices with the triangle total known from the warm-up, and around torch.unique, host enqueue
            included -- 7 repeats alternating between the two resolutions after a warm-up pass, median and range.  The
            outputs are compared with extract_mesh's before anything is timed; the 128 grid is saved for the next step;
  numpy     the vectorised numpy definition (tests/mesh_restatement.py, loaded by path) on the saved 128 grid, on the host;
  merge     the partial results as one JSON object."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RESOLUTIONS = (128, 256)


def _stats(times):
    return {'median': round(float(np.median(times)), 3), 'min': round(float(min(times)), 3),
            'max': round(float(max(times)), 3)}


def cmd_device(a):
    import torch
    from occnerf_amd import mesh, ops, synth
    from occnerf_amd.seeded import build_network
    assert torch.cuda.is_available(), 'the export is timed on a GPU only'
    dev = torch.device('cuda', 0)
    net = build_network(seed=0, S=128, device='cuda:0')
    frame = synth.make_frame(img_size=8, with_rays=False)
    lo, hi = frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz']
    lo64 = lo.astype(np.float64)

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return out, (time.perf_counter() - t0) * 1e3

    res, state = {}, {}
    for r in RESOLUTIONS:
        mesh.density_grid(net, lo, hi, r)                                   # warm-up at the size that is timed
        (field, h, shape), grid_ms = wall(lambda: mesh.density_grid(net, lo, hi, r))
        level = float(field.median().item())
        verts, faces = mesh.extract_mesh(field, level, lo64, h)             # warm-up, and the result the timed path must give
        T = int(faces.shape[0])

        def kernels(field=field, level=level, h=h, T=T):
            row_count = ops.mesh_count(field, level)
            ends = torch.cumsum(row_count, 0, dtype=torch.int64)
            return ops.mesh_emit(field, level, (ends - row_count).contiguous(), T)
        tri_keys = kernels()
        keys, inverse = torch.unique(tri_keys, sorted=True, return_inverse=True)
        assert torch.equal(inverse.reshape(T, 3).to(torch.int32), faces)
        assert torch.equal(ops.mesh_vertices(keys, field, level, lo64, h), verts)
        net.query_canonical(verts)                                          # warm-up at the size that is timed
        _, colour_ms = wall(lambda: torch.sigmoid(net.query_canonical(verts)[:, :3]))
        state[r] = (field, level, h, kernels, tri_keys, keys)
        res[f'res{r}'] = {'grid_shape_xyz': list(shape), 'grid_points': int(field.numel()), 'h': h, 'level_median': level,
                          'triangles': T, 'vertices': int(verts.shape[0]), 'density_grid_wall_ms': round(grid_ms, 2),
                          'colour_query_wall_ms': round(colour_ms, 2)}
        if r == 128:
            np.save(a.field, field.cpu().numpy())
            with open(a.field + '.json', 'w') as f:
                json.dump({'level': level, 'h': h, 'bbox_min': lo64.tolist(), 'triangles': T, 'vertices': int(verts.shape[0])}, f)

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / iters

    reps = {r: {'extract': [], 'unique': []} for r in RESOLUTIONS}
    for _ in range(a.repeats):
        for r in RESOLUTIONS:                                               # alternating within the call
            field, level, h, kernels, tri_keys, keys = state[r]
            def extract():
                kernels()
                ops.mesh_vertices(keys, field, level, lo64, h)
            reps[r]['extract'].append(events(extract, a.iters))
            reps[r]['unique'].append(events(lambda: torch.unique(tri_keys, sorted=True, return_inverse=True), a.iters))
    for r in RESOLUTIONS:
        res[f'res{r}']['count_scan_emit_vertices_ms'] = _stats(reps[r]['extract'])
        res[f'res{r}']['torch_unique_ms'] = _stats(reps[r]['unique'])
    res['what'] = (f'seeded checkpoint (seed 0), canonical box of the synthetic subject, iso level = median of the grid; device '
                   f'events over {a.iters} calls, host enqueue included, {a.repeats} repeats alternating between the '
                   'resolutions after a warm-up pass; outputs equal to extract_mesh before timing; wall times: the second call, synchronised')
    return res


def cmd_numpy(a):
    spec = importlib.util.spec_from_file_location('mesh_restatement', os.path.join(ROOT, 'tests', 'mesh_restatement.py'))
    mr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mr)
    field = np.load(a.field)
    with open(a.field + '.json') as f:
        meta = json.load(f)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        verts, faces = mr.extract_mesh(field, meta['level'], meta['bbox_min'], meta['h'])
        times.append((time.perf_counter() - t0) * 1e3)
    assert faces.shape[0] == meta['triangles'] and verts.shape[0] == meta['vertices']
    return {'numpy_restatement_res128_host_ms': _stats(times),
            'numpy_what': 'tests/mesh_restatement.py extract_mesh (keys, np.unique, vertices) on the saved 128 grid, 3 runs, host'}


def cmd_merge(a):
    res = {}
    for p in a.parts:
        with open(p) as f:
            res.update(json.load(f))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    for name in ('device', 'numpy'):
        p = sub.add_parser(name)
        p.add_argument('--field', required=True, help='.npy path of the 128 grid handed from `device` to `numpy`')
        p.add_argument('--out')
        p.add_argument('--repeats', type=int, default=7)
        p.add_argument('--iters', type=int, default=10)
    p = sub.add_parser('merge')
    p.add_argument('parts', nargs='+')
    p.add_argument('--out')
    a = ap.parse_args()
    res = globals()['cmd_' + a.cmd](a)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
