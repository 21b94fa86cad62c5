"""Measures the mesh rasteriser (occnerf_amd/mesh_view.py rasterize) on the seeded checkpoint and one
tool-made 512 x 512 dataset frame (tools/make_synthetic_dataset.py), whose K and body-space E are the camera.

    bash tools/mesh_view_bench.sh              # every step under its own time limit -> profiles/mesh_view_bench.json

Three meshes, each posed into the frame or made in it:
  mesh256   the export at mesh.resolution 256 at the median level of the grid (as tools/mesh_export_bench.py takes it: the
            seeded weights put no body-shaped surface at the default level), posed by mesh.pose_mesh: hundreds of thousands of
            triangles smaller than a pixel, all over the box -- more pixels than a body covers;
  mesh32    the same at mesh.resolution 32: triangles of many pixels, the wide pass;
  body      the body points' own mesh: the SyntheticSMPL faces over the vertices the tool posed for the frame.

Steps (each a sub-command, so the shell script can bound each one):
  device    per mesh: the three stages (ops.mesh_project, ops.mesh_raster with the fill of its keys, ops.mesh_resolve) from
            device events over `--iters` calls, host enqueue included, `--repeats` repeats alternating between the meshes and the
            stages after a warm-up pass, median and range; the counts; two calls compared byte for byte before anything is
            timed.  The body's inputs and outputs are saved for the next step;
  numpy     the numpy definition (tests/mesh_raster_restatement.py, loaded by path) on the body mesh, on the host: its time, and
            its outputs against the device's, byte for byte;
  merge     the partial results as one JSON object."""
import argparse
import hashlib
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUTPUTS = ('xy', 'z', 'vflag', 'cover', 'tri', 'depth', 'rgb', 'counts')


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _stats(times):
    return {'median': round(float(np.median(times)), 4), 'min': round(float(min(times)), 4), 'max': round(float(max(times)), 4)}


def cmd_device(a):
    import pickle
    import torch
    from occnerf_amd import mesh, mesh_view, ops, synth
    from occnerf_amd.dataset import PreparedDataset
    from occnerf_amd.seeded import build_network
    assert torch.cuda.is_available(), 'the rasteriser is timed on a GPU only'
    dev = torch.device('cuda', 0)
    tool = _load('make_synthetic_dataset', 'tools', 'make_synthetic_dataset.py')
    rr = _load('mesh_raster_restatement', 'tests', 'mesh_raster_restatement.py')
    with tempfile.TemporaryDirectory() as tmp:
        tool.make_dataset(tmp, frames=1, width=a.size, height=a.size, seed=0)
        ds = PreparedDataset(tmp, device=None)
        with open(os.path.join(tmp, 'mesh_infos.pkl'), 'rb') as f:
            info = pickle.load(f)[ds.frames[0]['frame_name']]
    fr, H, W = ds.frames[0], ds.height, ds.width
    K, E = fr['K'], fr['E']
    net = build_network(seed=0, S=128, non_rigid=True, device='cuda:0')
    canon = synth.make_frame(img_size=8, with_rays=False)
    lo, hi = canon['cnl_bbox_min_xyz'], canon['cnl_bbox_max_xyz']
    consts = ds.host_constants(0)
    data = {k: torch.from_numpy(np.ascontiguousarray(consts[k])).to(dev) for k in mesh._POSE_KEYS}
    data.update({k: np.asarray(consts[k], dtype=np.float32) for k in ('cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz')})
    rng = np.random.RandomState(0)
    sets = {}
    for name, res in (('mesh256', a.resolution), ('mesh32', 32)):
        field, h, _ = mesh.density_grid(net, lo, hi, res)
        verts, faces = mesh.extract_mesh(field, float(field.median().item()), lo.astype(np.float64), h)
        del field
        posed = mesh.pose_mesh(net, verts, data)[0]
        colors = torch.from_numpy(rng.randint(0, 256, (int(verts.shape[0]), 3)).astype(np.uint8)).to(dev)
        sets[name] = (posed, faces.contiguous(), colors)
    pos, faces, colors = rr.posed_smpl(tool, info)
    sets['body'] = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pos, faces, colors))

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / iters

    res, runs = {}, {}
    for name, (p, f, c) in sets.items():
        one, two = (mesh_view.rasterize(p, f, c, K, E, H, W) for _ in range(2))        # warm-up, and the same bytes twice
        assert all(torch.equal(one[k], two[k]) for k in OUTPUTS), name
        xy, z, vflag = ops.mesh_project(p, K, E)
        keys, counts = ops.mesh_raster(f, xy, z, vflag, H, W, faces_checked=True)
        n = dict(zip(mesh_view.COUNTS, one['counts'].tolist()))
        res[name] = {'vertices': int(p.shape[0]), 'triangles': int(f.shape[0]), 'counts': n,
                     'flagged_vertices': int((one['vflag'] != 0).sum().item()),
                     # the whole outputs, for holding two builds of the library against each other (OCCNERF_HIP_LIB)
                     'sha256': {k: hashlib.sha256(one[k].cpu().numpy().tobytes()).hexdigest() for k in OUTPUTS}}
        runs[name, 'project'] = lambda p=p: ops.mesh_project(p, K, E)
        runs[name, 'raster'] = lambda f=f, xy=xy, z=z, vflag=vflag: ops.mesh_raster(f, xy, z, vflag, H, W, faces_checked=True)
        runs[name, 'resolve'] = lambda f=f, xy=xy, z=z, vflag=vflag, c=c, keys=keys, counts=counts: \
            ops.mesh_resolve(keys, counts.clone(), f, xy, z, vflag, c, (255, 255, 255))
        runs[name, 'all'] = lambda p=p, f=f, c=c: mesh_view.rasterize(p, f, c, K, E, H, W, faces_checked=True)
        if name == 'body':
            np.savez(a.state, pos=pos, faces=faces, colors=colors, K=K, E=E, H=H, W=W,
                     **{'out_' + k: one[k].cpu().numpy() for k in OUTPUTS})
    reps = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, run in runs.items():                                         # alternating within the call
            reps[k].append(events(run, a.iters))
    for (name, stage), t in reps.items():
        res[name][stage + '_ms'] = _stats(t)
    res['image'] = [H, W]
    res['what'] = (f'seeded checkpoint (seed 0, non-rigid MLP on); one tool-made {W} x {H} dataset frame, its K and body-space E; '
                   f'mesh256 / mesh32: mesh.resolution {a.resolution} / 32 at the median level of the grid, posed by pose_mesh '
                   '(a noise surface all over the box, not a body), random vertex colours; body: the SyntheticSMPL faces over the '
                   f'vertices the tool posed; device events over {a.iters} calls, host enqueue and the fill of the keys '
                   f'included, {a.repeats} repeats alternating between meshes and stages after a warm-up pass; `all` = '
                   'mesh_view.rasterize (the three stages in one call); two calls gave equal bytes before timing')
    return res


def cmd_numpy(a):
    rr = _load('mesh_raster_restatement', 'tests', 'mesh_raster_restatement.py')
    st = np.load(a.state)
    t0 = time.perf_counter()
    out = rr.rasterize(st['pos'], st['faces'], st['colors'], st['K'], st['E'], int(st['H']), int(st['W']))
    ms = (time.perf_counter() - t0) * 1e3
    out['counts'] = rr.count_vector(out['counts'])
    for k in OUTPUTS:
        assert st['out_' + k].tobytes() == np.ascontiguousarray(out[k]).tobytes(), k
    return {'body': {'numpy_host_ms': round(ms, 1)},
            'numpy_what': 'tests/mesh_raster_restatement.py rasterize on the body mesh, one run, host; its eight outputs equal the '
                          "kernels' byte for byte"}


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
    p.add_argument('--size', type=int, default=512)
    p.add_argument('--repeats', type=int, default=7)
    p.add_argument('--iters', type=int, default=10)
    p = sub.add_parser('numpy')
    p.add_argument('--state', required=True)
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
