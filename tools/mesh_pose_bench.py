"""Measures the posing of the exported mesh (occnerf_amd/mesh.py pose_mesh) on the seeded checkpoint at
mesh.resolution 256, the size tools/mesh_export_bench.py measures the extraction at, in three frames of the synthetic movement
sequence.

    bash tools/mesh_pose_bench.sh              # every step under its own time limit -> profiles/mesh_pose_bench.json

The seeded weights put no body-shaped surface at the default level, so -- as in mesh_export_bench.py -- the iso level is the
median of the grid: 178 K vertices all over the canonical box.  Most of them lie where no bone has a weight and end after a
few evaluations (flag 2, or flag 1 in the clamped region), so the seeded body itself (the 6 890 body points tiled to the same
vertex count, every one of which is solved) is measured beside them: that is what a trained subject's mesh costs.

Steps (each a sub-command, so the shell script can bound each one):
  device    per point set and frame: occnerf_mesh_pose from device events (host enqueue included) over `--iters` calls, `--repeats`
            repeats alternating between the frames and the point sets after a warm-up pass, median and range; the flag shares and
            the mean Newton steps; the wall time of the non-rigid fixed point (second call, synchronised).  The outputs of
            two calls are compared before anything is timed.  A 6 890-point subset of the mesh and the frames' constants are
            saved for the next step;
  numpy     the numpy definition (tests/mesh_pose_restatement.py, loaded by path) on the saved subsets, on the host: its time,
            scaled to the vertex count and labelled as scaled, its results against the device's, and its count of the corner
            values read, from which the kernel's achieved bytes per second follow;
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

FRAMES = (0, 3, 17)
SUBSET = 6890


def _stats(times):
    return {'median': round(float(np.median(times)), 3), 'min': round(float(min(times)), 3),
            'max': round(float(max(times)), 3)}


def cmd_device(a):
    import torch
    from occnerf_amd import mesh, ops, synth
    from occnerf_amd.seeded import build_network
    assert torch.cuda.is_available(), 'the posing is timed on a GPU only'
    dev = torch.device('cuda', 0)
    net = build_network(seed=0, S=128, non_rigid=True, device='cuda:0')
    canon = synth.make_frame(img_size=8, with_rays=False)
    lo, hi = canon['cnl_bbox_min_xyz'], canon['cnl_bbox_max_xyz']
    field, h, shape = mesh.density_grid(net, lo, hi, a.resolution)
    level = float(field.median().item())
    verts, faces = mesh.extract_mesh(field, level, lo.astype(np.float64), h)
    del field
    V = int(verts.shape[0])
    body = net.point_base.detach().float()
    body = body.repeat(-(-V // body.shape[0]), 1)[:V].contiguous()
    sets = {'mesh': verts, 'body': body}
    sub = torch.arange(0, V, max(V // SUBSET, 1), device=dev)[:SUBSET]

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return out, (time.perf_counter() - t0) * 1e3

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
    for idx in FRAMES:
        fr = synth.make_frame(img_size=8, pose72=synth.movement_pose(idx, 100), with_rays=False)
        data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in mesh._POSE_KEYS}
        bmin, bsc = fr['cnl_bbox_min_xyz'], fr['cnl_bbox_scale_xyz']
        Rs, Ts, vol = net.render_preamble(data)
        net.unoffset_canonical(verts, data)                                 # warm-up at the size that is timed
        (s, moving), fixed_ms = wall(lambda: net.unoffset_canonical(verts, data))
        saved.update({f'Rs{idx}': Rs.cpu().numpy(), f'Ts{idx}': Ts.cpu().numpy(), f'vol{idx}': vol.cpu().numpy()[:Rs.shape[0]]})
        for name, x in sets.items():
            run = lambda x=x, Rs=Rs, Ts=Ts, vol=vol, bmin=bmin, bsc=bsc: ops.mesh_pose(x, Rs, Ts, vol, bmin, bsc)    # noqa: E731
            out, again = run(), run()                                       # warm-up, and the same bytes twice
            assert all(torch.equal(p, q) for p, q in zip(out, again))
            flag = out[1]
            counts = torch.bincount(flag.long(), minlength=3).tolist()
            state[name, idx] = run
            res[f'{name}_frame{idx}'] = {
                'vertices': V, 'converged_share': round(counts[0] / V, 4), 'not_converged_share': round(counts[1] / V, 4),
                'no_bone_share': round(counts[2] / V, 4), 'mean_iters': round(float(out[2].float().mean().item()), 3),
                'worst_resid_converged': float(out[3][flag == 0].max().item()) if counts[0] else None,
                # the whole outputs, for holding two builds of the library against each other (OCCNERF_HIP_LIB)
                'sha256': {k: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for k, t in zip(('p', 'flag', 'iters', 'resid'), out)}}
            for k, t in zip(('p', 'flag', 'iters', 'resid'), out):
                saved[f'{name}{idx}_{k}'] = t[sub].cpu().numpy()
        res[f'mesh_frame{idx}']['non_rigid_fixed_point_wall_ms'] = round(fixed_ms, 2)
        res[f'mesh_frame{idx}']['non_rigid_rows_still_moving'] = int(moving.sum().item())
    for name, x in sets.items():
        saved[f'{name}_x'] = x[sub].cpu().numpy()
    saved.update(bmin=bmin, bsc=bsc)
    np.savez(a.state, **saved)

    reps = {k: [] for k in state}
    for _ in range(a.repeats):
        for k, run in state.items():                                        # alternating within the call
            reps[k].append(events(run, a.iters))
    for (name, idx), t in reps.items():
        res[f'{name}_frame{idx}']['mesh_pose_ms'] = _stats(t)
    res['resolution'] = a.resolution
    res['grid_shape_xyz'] = list(shape)
    res['what'] = (f'seeded checkpoint (seed 0, non-rigid MLP on), mesh.resolution {a.resolution}, iso level = median of the grid '
                   f'({V} vertices: "mesh"), and the 6 890 body points tiled to as many ("body"); frames {list(FRAMES)} of the '
                   f'synthetic movement sequence of 100; candidates 3, max_iter 20, tol 1e-7; device events over {a.iters} calls, '
                   f'host enqueue included, {a.repeats} repeats alternating between the frames and the point sets after a warm-up '
                   'pass; two calls gave equal bytes before timing; wall times: the second call, synchronised')
    return res


def cmd_numpy(a):
    spec = importlib.util.spec_from_file_location('mesh_pose_restatement', os.path.join(ROOT, 'tests', 'mesh_pose_restatement.py'))
    mp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mp)
    st = np.load(a.state)
    with open(a.device) as f:
        dev = json.load(f)
    res = {}
    for name in ('mesh', 'body'):
        x = st[f'{name}_x']
        for idx in FRAMES:
            args = (st[f'Rs{idx}'], st[f'Ts{idx}'], st[f'vol{idx}'], st['bmin'], st['bsc'])
            mp.COUNT.update(evaluations=0, taps=0)
            t0 = time.perf_counter()
            out = mp.pose_points(x, *args)
            ms = (time.perf_counter() - t0) * 1e3
            for k, w in zip(('p', 'flag', 'iters', 'resid'), out):
                assert st[f'{name}{idx}_{k}'].tobytes() == w.tobytes(), (name, idx, k)
            d = dev[f'{name}_frame{idx}']
            V = d['vertices']
            taps = mp.COUNT['taps'] / len(x)
            res[f'{name}_frame{idx}'] = {
                'numpy_subset_points': int(len(x)), 'numpy_subset_host_ms': round(ms, 1),
                'numpy_scaled_to_all_vertices_ms': round(ms * V / len(x), 0),
                'evaluations_per_vertex_subset': round(mp.COUNT['evaluations'] / len(x), 2),
                'corner_values_read_per_vertex_subset': round(taps, 1),
                'achieved_gather_GBps_estimated': round(taps * 4 * V / (d['mesh_pose_ms']['median'] * 1e-3) / 1e9, 1)}
    res['numpy_what'] = ('tests/mesh_pose_restatement.py pose_points on every (V // 6890)-th vertex, one run, host; its four outputs '
                         'equal the kernel\'s rows byte for byte; the scaled time is that time x V / subset size; corner values '
                         'read = the on-grid corners of every bone evaluated, 4 B each, counted by the restatement on the subset '
                         'and scaled to V for the bytes per second of the kernel\'s median time')
    return res


def cmd_merge(a):
    res = {}
    for p in a.parts:
        with open(p) as f:
            for k, v in json.load(f).items():
                if isinstance(v, dict) and isinstance(res.get(k), dict):
                    res[k].update(v)
                else:
                    res[k] = v
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    p = sub.add_parser('device')
    p.add_argument('--state', required=True, help='.npz path of what `device` hands to `numpy`')
    p.add_argument('--out')
    p.add_argument('--resolution', type=int, default=256)
    p.add_argument('--repeats', type=int, default=7)
    p.add_argument('--iters', type=int, default=10)
    p = sub.add_parser('numpy')
    p.add_argument('--state', required=True)
    p.add_argument('--device', required=True, help="the JSON `device` wrote")
    p.add_argument('--out')
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
