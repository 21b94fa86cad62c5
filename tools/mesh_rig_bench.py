"""Measures the rig of the exported mesh (occnerf_amd/mesh.py skin_mesh / export_rig, csrc/mesh_rig.hip) on
the seeded checkpoint at mesh.resolution 256, the size tools/mesh_pose_bench.py measures the posing at.

    bash tools/mesh_rig_bench.sh               # every step under its own time limit -> profiles/mesh_rig_bench.json

As there, the iso level is the median of the grid (the seeded weights put no body-shaped surface at the default level): a
surface all over the canonical box ("mesh"), most of whose vertices no bone carries, and beside it the 6 890 body points tiled
to the same vertex count ("body"): what a trained subject's mesh costs.  No trained body is measured.

Steps (each a sub-command, so the shell script can bound each one):
  device    per point set: occnerf_mesh_skin (K 4 and 8) and occnerf_mesh_lbs for 1 and for 16 frames of the synthetic movement
            sequence, with and without targets (the targets: occnerf_mesh_pose's positions and flags), from device events (host
            enqueue included) over `--iters` calls, `--repeats` repeats alternating between the cases after a warm-up pass,
            median and range.  The outputs of two calls are compared before anything is timed.  The deviation figures of
            rig.json (the distance between the rig's skinning and the model's posed mesh over the solved vertices) and the
            correctives' flags for the frames 0, 3 and 17.  A subset of the points and the device's results on it are saved;
  numpy     the numpy definition (tests/mesh_rig_restatement.py, loaded by path) on the saved subset, on the host: its time,
            and its results against the device's;
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

FRAMES = (0, 3, 17) + tuple(range(20, 85, 5))          # 16 frames; the first three are the recorded ones
SUBSET = 6890


def _stats(times):
    return {'median': round(float(np.median(times)), 4), 'min': round(float(min(times)), 4), 'max': round(float(max(times)), 4)}


def cmd_device(a):
    import torch
    from occnerf_amd import mesh, ops, synth
    from occnerf_amd.seeded import build_network
    assert torch.cuda.is_available(), 'the rig is timed on a GPU only'
    dev = torch.device('cuda', 0)
    net = build_network(seed=0, S=128, non_rigid=True, device='cuda:0')
    canon = synth.make_frame(img_size=8, with_rays=False)
    lo, hi = canon['cnl_bbox_min_xyz'], canon['cnl_bbox_max_xyz']
    field, h, shape = mesh.density_grid(net, lo, hi, a.resolution)
    verts, _ = mesh.extract_mesh(field, float(field.median().item()), lo.astype(np.float64), h)
    del field
    V = int(verts.shape[0])
    body = net.point_base.detach().float()
    body = body.repeat(-(-V // body.shape[0]), 1)[:V].contiguous()
    sets = {'mesh': verts, 'body': body}
    sub = torch.arange(0, V, max(V // SUBSET, 1), device=dev)[:SUBSET]
    bmin, bsc = canon['cnl_bbox_min_xyz'], canon['cnl_bbox_scale_xyz']
    pre = []
    for idx in FRAMES:
        fr = synth.make_frame(img_size=8, pose72=synth.movement_pose(idx, 100), with_rays=False)
        pre.append(net.render_preamble({k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in mesh._POSE_KEYS}))
    Rs, Ts = torch.stack([p[0] for p in pre]).contiguous(), torch.stack([p[1] for p in pre]).contiguous()
    vol = pre[0][2]
    vol24 = vol[:Rs.shape[1]]

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / iters

    def same(p, q):
        p, q = (p, q) if isinstance(p, tuple) else ((p,), (q,))
        return all(torch.equal(s, t) for s, t in zip(p, q))

    res, runs = {}, {}
    saved = {'Rs': Rs.cpu().numpy(), 'Ts': Ts.cpu().numpy(), 'vol': vol24.cpu().numpy(), 'bmin': bmin, 'bsc': bsc}
    for name, x in sets.items():
        newton = [ops.mesh_pose(x, Rs[f], Ts[f], vol, bmin, bsc) for f in range(len(FRAMES))]
        target, tflag = torch.stack([n[0] for n in newton]).contiguous(), torch.stack([n[1] for n in newton]).contiguous()
        del newton
        saved[f'{name}_x'], saved[f'{name}_target'], saved[f'{name}_tflag'] = x[sub].cpu().numpy(), target[:3, sub].cpu().numpy(), tflag[:3, sub].cpu().numpy()
        for K in (4, 8):
            skin = lambda x=x, K=K: ops.mesh_skin(x, vol24, bmin, bsc, K)                           # noqa: E731
            out = skin()
            assert same(out, skin())
            joints, weights, count, kept = out
            runs[f'{name}_skin_K{K}'] = skin
            n = count.cpu().numpy()
            share = kept.cpu().numpy().astype(np.float64)[n > 0]
            entry = {'vertices': V, 'influences_histogram': np.bincount(n, minlength=K + 1).tolist(),
                     # the whole outputs, for holding two builds of the library against each other (OCCNERF_HIP_LIB)
                     'sha256': {k: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
                                for k, t in zip(('joints', 'weights', 'count', 'kept'), out)},
                     'kept_share': {'min': float(share.min()), 'mean': float(share.mean()), 'p01': float(np.percentile(share, 1))}}
            for F in (1, 16):
                R, T_, tg, tf = Rs[:F].contiguous(), Ts[:F].contiguous(), target[:F].contiguous(), tflag[:F].contiguous()
                plain = lambda x=x, j=joints, w=weights, R=R, T_=T_: ops.mesh_lbs(x, j, w, R, T_, joints_checked=True)     # noqa: E731
                full = lambda x=x, j=joints, w=weights, R=R, T_=T_, tg=tg, tf=tf: ops.mesh_lbs(x, j, w, R, T_, tg, tf, 0.05, joints_checked=True)     # noqa: E731
                assert same(plain(), plain()) and same(full(), full())
                runs[f'{name}_lbs_K{K}_F{F}'], runs[f'{name}_lbs_targets_K{K}_F{F}'] = plain, full
            posed, delta, dflag = ops.mesh_lbs(x, joints, weights, Rs[:3].contiguous(), Ts[:3].contiguous(), target[:3].contiguous(),
                                               tflag[:3].contiguous(), 0.05)
            dist = (posed.double() - target[:3].double()).norm(dim=2).cpu().numpy()
            ok = tflag[:3].cpu().numpy() == 0
            entry['frames'] = {str(FRAMES[f]): {'lbs_to_model_m': mesh._spread(dist[f][ok[f]]),
                                                'corrective_flagged': int(dflag[f].sum().item()),
                                                'corrective_max_m': float(delta[f].abs().max().item())} for f in range(3)}
            res[f'{name}_K{K}'] = entry
            for k, t in (('joints', joints), ('weights', weights), ('count', count), ('kept', kept)):
                saved[f'{name}{K}_{k}'] = t[sub].cpu().numpy()
            for k, t in (('posed', posed), ('delta', delta), ('dflag', dflag)):
                saved[f'{name}{K}_{k}'] = t[:, sub].cpu().numpy()
        del target, tflag
    np.savez(a.state, **saved)
    for run in runs.values():                                               # warm-up pass
        run()
    reps = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, run in runs.items():                                         # alternating within the call
            reps[k].append(events(run, a.iters))
    res['ms'] = {k: _stats(t) for k, t in reps.items()}
    res['resolution'], res['grid_shape_xyz'] = a.resolution, list(shape)
    res['what'] = (f'seeded checkpoint (seed 0, non-rigid MLP on; no trained body was measured), mesh.resolution {a.resolution}, iso '
                   f'level = median of the grid ({V} vertices: "mesh"), and the 6 890 body points tiled to as many ("body"); frames '
                   f'{list(FRAMES)} of the synthetic movement sequence of 100 (F 1: the first, F 16: all); targets = occnerf_mesh_pose '
                   f'(candidates 3, max_iter 20, tol 1e-7, the non-rigid offset not undone), max_delta 0.05; device events over '
                   f'{a.iters} calls, host enqueue included, {a.repeats} repeats alternating between the cases after a warm-up pass; '
                   'two calls gave equal outputs before timing; the deviation figures are those of rig.json, over the vertices '
                   'mesh_pose solved')
    return res


def cmd_numpy(a):
    sys.path.insert(0, ROOT)
    spec = importlib.util.spec_from_file_location('mesh_rig_restatement', os.path.join(ROOT, 'tests', 'mesh_rig_restatement.py'))
    rig = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rig)
    s = np.load(a.state)
    res = {}
    for name in ('mesh', 'body'):
        x = s[f'{name}_x']
        for K in (4, 8):
            t0 = time.perf_counter()
            skin = rig.skin(x, s['vol'], s['bmin'], s['bsc'], K)
            t1 = time.perf_counter()
            lbs = rig.lbs(x, skin[0], skin[1], s['Rs'][:3], s['Ts'][:3], s[f'{name}_target'], s[f'{name}_tflag'], 0.05)
            t2 = time.perf_counter()
            equal = all(np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)
                        for g, w in zip(skin + lbs, [s[f'{name}{K}_{k}'] for k in ('joints', 'weights', 'count', 'kept', 'posed', 'delta', 'dflag')]))
            res[f'{name}_K{K}'] = {'points': int(x.shape[0]), 'skin_ms': round((t1 - t0) * 1e3, 1),
                                   'lbs_3_frames_with_targets_ms': round((t2 - t1) * 1e3, 1), 'equal_to_the_device': bool(equal)}
    return {'numpy': res, 'numpy_what': 'tests/mesh_rig_restatement.py skin and lbs (3 frames, with targets) on every (V // 6890)-th '
                                        'point, one run, host; its seven outputs compared with the device\'s as bit patterns'}


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
    d.add_argument('--resolution', type=int, default=256)
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
