"""Measures the mesh clean-up (occnerf_amd/mesh.py component_table / filter_mesh, csrc/mesh_components.hip, DESIGN.md section
7m) on the median-level noise mesh of the seeded checkpoint at mesh.resolution 256 and 128: many components, a hard case.

    bash tools/mesh_components_bench.sh        # every step under its own time limit -> profiles/mesh_components_bench.json

Steps (each a sub-command, so the shell script can bound each one):
  device    per resolution: the mesh, its components and the pass count; device events (host enqueue and the per-pass read
            of the status word included) around the labelling, around ranks + statistics and around selection + filter under
            'largest' -- 7 repeats alternating between the two resolutions after a warm-up; two calls give equal bytes before
            anything is timed.  Then one frame of the synthetic movement sequence posed with and without `mesh.components
            largest` at 256: the time of occnerf_mesh_pose and the flagged vertices.  The meshes and the device's labels
            and records are saved for the next step;
  numpy     the numpy definition (tests/mesh_components_restatement.py, loaded by path) on the saved meshes, timed and
            compared with the device's outputs, and scipy.sparse.csgraph.connected_components where scipy is importable;
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

RESOLUTIONS = (256, 128)
FRAME = 3
COLUMNS = ('label', 'vertices', 'triangles', 'boundary_vertices', 'smin', 'smax', 'volume6_q')


def _stats(times):
    return {'median': round(float(np.median(times)), 3), 'min': round(float(min(times)), 3),
            'max': round(float(max(times)), 3)}


def cmd_device(a):
    import torch
    from occnerf_amd import mesh, ops, synth
    from occnerf_amd.seeded import build_network
    assert torch.cuda.is_available(), 'the clean-up is timed on a GPU only'
    dev = torch.device('cuda', 0)
    net = build_network(seed=0, S=128, device='cuda:0')
    frame = synth.make_frame(img_size=8, with_rays=False)
    lo, hi = frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz']
    lo64 = lo.astype(np.float64)

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / iters

    res, state, saved = {}, {}, {}
    for r in RESOLUTIONS:
        field, h, shape = mesh.density_grid(net, lo, hi, r)
        level = float(field.median().item())
        verts, faces = mesh.extract_mesh(field, level, lo64, h)
        del field
        V, T = int(verts.shape[0]), int(faces.shape[0])
        labels, rec = ops.mesh_components(verts, faces, lo64, h, shape)
        again_labels, again = ops.mesh_components(verts, faces, lo64, h, shape)
        assert torch.equal(labels, again_labels) and all(torch.equal(rec[k], again[k]) for k in COLUMNS)
        host = {k: rec[k].cpu().numpy() for k in COLUMNS}
        keep = mesh.select_components(host, 'largest', False)
        kept_v, kept_f = mesh.filter_mesh(verts, faces, labels, keep)
        vrank, roots = ops.mesh_component_ranks(labels)

        def label(faces=faces, V=V):
            ops.mesh_label(faces, V)

        def stats(verts=verts, faces=faces, labels=labels, h=h, shape=shape):
            vrank, roots = ops.mesh_component_ranks(labels)
            ops.mesh_component_stats(verts, faces, vrank, int(roots.numel()), lo64, h, shape)

        def filt(verts=verts, faces=faces, labels=labels, host=host):
            mesh.filter_mesh(verts, faces, labels, mesh.select_components(host, 'largest', False))
        state[r] = {'label': label, 'stats': stats, 'filter': filt}
        tri = host['triangles'].astype(np.int64)
        res[f'res{r}'] = {'grid_shape_xyz': list(shape), 'h': h, 'level_median': level, 'vertices': V, 'triangles': T,
                          'components': int(roots.numel()), 'passes': int(rec['passes']),
                          'largest_component_triangles': int(tri.max()), 'components_with_one_triangle': int((tri == 1).sum()),
                          'cavities': int(((host['boundary_vertices'] == 0) & (host['volume6_q'] < 0)).sum()),
                          'kept_vertices_largest': int(kept_v.shape[0]), 'kept_triangles_largest': int(kept_f.shape[0])}
        saved.update({f'verts{r}': verts.cpu().numpy(), f'faces{r}': faces.cpu().numpy(), f'labels{r}': labels.cpu().numpy(),
                      f'h{r}': np.float64(h), f'shape{r}': np.asarray(shape)})
        saved.update({f'{k}{r}': host[k] for k in COLUMNS})
        if r == 256:
            posing = (verts, kept_v)
    saved['lo'] = lo64
    np.savez(a.state, **saved)

    reps = {(r, k): [] for r in RESOLUTIONS for k in ('label', 'stats', 'filter')}
    for _ in range(a.repeats):
        for r in RESOLUTIONS:                                               # alternating within the call
            for k, fn in state[r].items():
                reps[r, k].append(events(fn, a.iters))
    for (r, k), t in reps.items():
        res[f'res{r}'][{'label': 'labelling_ms', 'stats': 'ranks_and_statistics_ms', 'filter': 'select_and_filter_ms'}[k]] = _stats(t)

    # what the feature is for: one frame posed with and without the detached blobs
    fr = synth.make_frame(img_size=8, pose72=synth.movement_pose(FRAME, 100), with_rays=False)
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in mesh._POSE_KEYS}
    bmin, bsc = fr['cnl_bbox_min_xyz'], fr['cnl_bbox_scale_xyz']
    Rs, Ts, vol = net.render_preamble(data)
    pose_reps = {'all': [], 'largest': []}
    runs = {}
    for name, x in zip(('all', 'largest'), posing):
        runs[name] = lambda x=x: ops.mesh_pose(x, Rs, Ts, vol, bmin, bsc)    # noqa: E731
        out = runs[name]()
        counts = torch.bincount(out[1].long(), minlength=3).tolist()
        res[f'posing_frame{FRAME}_{name}'] = {'vertices': int(x.shape[0]), 'not_converged': counts[1], 'no_bone': counts[2],
                                             'flagged_share': round((counts[1] + counts[2]) / max(int(x.shape[0]), 1), 4),
                                             'mean_iters': round(float(out[2].float().mean().item()), 3)}
    for _ in range(a.repeats):
        for name, run in runs.items():
            pose_reps[name].append(events(run, a.iters))
    for name, t in pose_reps.items():
        res[f'posing_frame{FRAME}_{name}']['mesh_pose_ms'] = _stats(t)
    res['what'] = (f'seeded checkpoint (seed 0), canonical box of the synthetic subject, iso level = median of the grid; device '
                   f'events over {a.iters} calls, host enqueue and the blocking two-word read per labelling pass included, '
                   f'{a.repeats} repeats alternating between the resolutions after a warm-up; two calls gave equal bytes before '
                   f'timing; posing: frame {FRAME} of the synthetic movement sequence of 100, the mesh at 256 as extracted and '
                   "under mesh.components 'largest', candidates 3, max_iter 20, tol 1e-7, no non-rigid offset")
    return res


def cmd_numpy(a):
    spec = importlib.util.spec_from_file_location('mesh_components_restatement',
                                                  os.path.join(ROOT, 'tests', 'mesh_components_restatement.py'))
    cr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cr)
    st = np.load(a.state)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        connected_components = None
    res = {}
    for r in RESOLUTIONS:
        verts, faces, shape, h = st[f'verts{r}'], st[f'faces{r}'], tuple(int(s) for s in st[f'shape{r}']), float(st[f'h{r}'])
        rounds = []
        t0 = time.perf_counter()
        lab = cr.labels(faces, verts.shape[0], rounds)
        t1 = time.perf_counter()
        rec = cr.records(verts, faces, lab, st['lo'], h, shape)
        t2 = time.perf_counter()
        keep = cr.select(rec, 'largest')
        cr.filter_mesh(verts, faces, lab, keep)
        t3 = time.perf_counter()
        assert np.array_equal(lab, st[f'labels{r}'])
        for k in COLUMNS:
            assert np.array_equal(rec[k], st[f'{k}{r}']), k
        out = {'labels_host_ms': round((t1 - t0) * 1e3, 1), 'synchronous_rounds': rounds[0],
               'records_host_ms': round((t2 - t1) * 1e3, 1), 'select_and_filter_host_ms': round((t3 - t2) * 1e3, 1),
               'equal_to_device': True}
        if connected_components is not None:
            f = faces.astype(np.int64)
            V = verts.shape[0]
            t0 = time.perf_counter()
            rows = np.concatenate([f[:, 0], f[:, 1]])
            cols = np.concatenate([f[:, 1], f[:, 2]])
            n, comp = connected_components(coo_matrix((np.ones(rows.shape[0], np.int8), (rows, cols)), shape=(V, V)), directed=False)
            out['scipy_connected_components_host_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
            first = np.full(n, V, dtype=np.int64)
            np.minimum.at(first, comp, np.arange(V))
            assert n == rec['label'].shape[0] and np.array_equal(first[comp], lab)
            out['scipy_partition_equal'] = True
        res[f'numpy_res{r}'] = out
    res['numpy_what'] = ('tests/mesh_components_restatement.py on the meshes the device step saved, one run each, host; labels, '
                         'every record column equal to the device outputs; ' +
                         ('scipy.sparse.csgraph.connected_components on the vertex graph (two edges per face), its partition '
                          'equal to the labels' if connected_components is not None else
                          'scipy is not importable here: no comparison with scipy.sparse.csgraph was made'))
    return res


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
        p.add_argument('--state', required=True, help='.npz path of the meshes handed from `device` to `numpy`')
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
