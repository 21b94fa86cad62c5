"""The cases of tests/test_g_train_batch.py, built on the CPU from tool-made datasets and the restatement: which frame, which
configuration, which uniforms, and the coverage condition each case has to meet BEFORE anything is compared -- a case that
silently degenerates (no clip where it claims one, no hole, no duplicate row, a class that is not empty) shows nothing."""
import importlib.util
import os
import shutil

import numpy as np
from PIL import Image

from tests import train_batch_restatement as tbr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO = 0.8
BAND = {'range': 1, 'mid': 46, 'width': 20}
CASES = ['band_on', 'band_off', 'corners', 'box_edge_holes', 'overlap_duplicates', 'size16', 'size20', 'size32', 'n1', 'n8',
         'tall_frame', 'random_bgcolor', 'u1_first_and_last', 'empty_off_subject']


def load_tool():
    spec = importlib.util.spec_from_file_location('make_synthetic_dataset', os.path.join(ROOT, 'tools', 'make_synthetic_dataset.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_datasets(base):
    """wide: 96 x 80, the box edge inside the image; near: 96 x 80 at a longer focal length, subject and box reach the image
    border; tall: 64 x 112; full: `wide` with every mask at 255, so box-and-not-subject is empty."""
    tool = load_tool()
    paths = {k: os.path.join(str(base), k) for k in ('wide', 'near', 'tall', 'full')}
    tool.make_dataset(paths['wide'], frames=2, width=96, height=80, seed=11, focal=900.0)
    tool.make_dataset(paths['near'], frames=1, width=96, height=80, seed=12, focal=2600.0)
    tool.make_dataset(paths['tall'], frames=1, width=64, height=112, seed=13, focal=900.0)
    shutil.copytree(paths['wide'], paths['full'])
    for f in os.listdir(os.path.join(paths['full'], 'masks')):
        Image.fromarray(np.full((80, 96), 255, np.uint8), 'L').save(os.path.join(paths['full'], 'masks', f))
    return paths


def u_for(draws, counts):
    """Uniforms that make the builder draw (class, select_idx): u0 on the class's side of RATIO, u1 the middle of
    select_idx's interval of [0, 1)."""
    return np.array([[0.0 if c == 0 else 0.9, (k + 0.5) / counts[c]] for c, k in draws], dtype=np.float64)


def build_case(name, paths):
    """-> dict(path, cfg, frame, bgcolor, u, check): `check(r)` asserts the case's coverage condition on the restatement's
    result r."""
    rng = np.random.RandomState(CASES.index(name) + 100)
    c = {'name': name, 'path': paths['wide'], 'frame': 1, 'bgcolor': np.array([0., 0., 0.], 'float32'),
         'cfg': {'N_patches': 4, 'size': 16, 'occlude': False, 'occlusion': dict(BAND), 'volume_size': 4,
                 'sample_subject_ratio': RATIO}, 'check': lambda r: None}

    def masks():
        rs = tbr.Restatement(c['path'], **c['cfg'])
        _, ray_mask, subject, off = rs.frame_masks(c['frame'])
        return subject, off, ray_mask.reshape(subject.shape)

    def random_u():
        u = rng.rand(c['cfg']['N_patches'], 2)
        u[0, 0], u[-1, 0] = 0.1, 0.95             # both classes are drawn whenever there are two patches
        return u

    if name in ('band_on', 'band_off'):
        c['frame'] = 0
        c['cfg']['occlude'] = name == 'band_on'
        c['u'] = random_u()
        subject, _, _ = masks()
        cols = subject[:, BAND['mid'] - BAND['width'] // 2:BAND['mid'] + BAND['width'] // 2]
        assert (cols.sum() == 0) if name == 'band_on' else (cols.sum() > 50), 'the band does not cross the subject'
    elif name == 'corners':
        c['path'], c['frame'] = paths['near'], 0
        subject, off, _ = masks()
        H, W = subject.shape
        draws = []
        for cy, cx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            best = None
            for cls, m in ((0, subject), (1, off)):
                ys, xs = np.where(m)
                if ys.size:
                    j = int(np.argmin((ys - cy) ** 2 + (xs - cx) ** 2))
                    d = (ys[j] - cy) ** 2 + (xs[j] - cx) ** 2
                    if best is None or d < best[0]:
                        best = (d, cls, j, ys[j], xs[j])
            draws.append(best[1:3])
        c['u'] = u_for(draws, (int(subject.sum()), int(off.sum())))
        S = c['cfg']['size']

        def check(r):                             # every patch is moved by the clip in both axes, one per corner
            want = [(0, 0), (W - S, 0), (0, H - S), (W - S, H - S)]
            assert [tuple(v) for v in r['_xy_min'].tolist()] == want, r['_xy_min']
        c['check'] = check
    elif name == 'box_edge_holes':
        subject, off, box = masks()
        H, W = box.shape
        S = c['cfg']['size']
        ys, xs = np.where(off)
        edge = [j for j in range(ys.size) if S // 2 <= ys[j] < H - S // 2 and S // 2 <= xs[j] < W - S // 2
                and 0.3 < box[ys[j] - S // 2:ys[j] + S // 2, xs[j] - S // 2:xs[j] + S // 2].mean() < 0.8]
        assert len(edge) >= 4, 'no off-subject pixel next to the box edge'
        draws = [(1, edge[0]), (1, edge[len(edge) // 3]), (1, edge[2 * len(edge) // 3]), (1, edge[-1])]
        c['u'] = u_for(draws, (int(subject.sum()), int(off.sum())))

        def check(r):
            holes = (~r['patch_masks']).reshape(4, -1).sum(1)
            assert (holes > 0).all() and (holes < S * S).all(), holes
        c['check'] = check
    elif name == 'overlap_duplicates':
        subject, off, _ = masks()
        k = int(subject.sum()) // 2
        c['u'] = u_for([(0, k), (0, k), (0, k + 3), (1, 5)], (int(subject.sum()), int(off.sum())))

        def check(r):
            sel = r['patch_mask']
            assert np.unique(sel).size < sel.size and np.array_equal(r['patch_masks'][0], r['patch_masks'][1])
            assert r['patch_div_indices'][1] > 0
        c['check'] = check
    elif name in ('size16', 'size20', 'size32'):
        c['cfg']['size'] = int(name[4:])
        c['u'] = random_u()
    elif name in ('n1', 'n8'):
        c['cfg']['N_patches'] = int(name[1:])
        c['u'] = random_u()
    elif name == 'tall_frame':
        c['path'], c['frame'] = paths['tall'], 0
        c['u'] = random_u()
        subject, _, _ = masks()
        assert subject.shape == (112, 64)
    elif name == 'random_bgcolor':
        c['bgcolor'] = (rng.rand(3) * 255.).astype('float32')      # train.py:388
        c['u'] = random_u()

        def check(r):                             # the colour reaches the target: some patch pixel is pure background
            bg = (c['bgcolor'].astype(np.float64) / 255.).astype('float32')
            assert (r['target_patches'] == bg).all(-1).any()
        c['check'] = check
    elif name == 'u1_first_and_last':
        below_one = np.nextafter(1.0, 0.0)
        c['u'] = np.array([[0.0, 0.0], [0.0, below_one], [0.9, 0.0], [0.9, below_one]])
        subject, off, _ = masks()
        counts = (int(subject.sum()), int(off.sum()))
        want = [(0, 0), (0, counts[0] - 1), (1, 0), (1, counts[1] - 1)]
        assert tbr.draws_from_uniforms(c['u'], subject, off, RATIO) == want
    elif name == 'empty_off_subject':
        c['path'] = paths['full']
        c['u'] = random_u()                       # its last patch asks for the off-subject class
        subject, off, _ = masks()
        assert off.sum() == 0 and subject.all()
        assert [d[0] for d in tbr.draws_from_uniforms(c['u'], subject, off, RATIO)] == [0, 0, 0, 0]
    else:
        raise KeyError(name)
    return c


def restate(case):
    """(restatement result, draws) of a case; asserts the common coverage condition: both classes non-empty on the frame
    (except the case built to have one empty) and the case's own condition."""
    rs = tbr.Restatement(case['path'], **case['cfg'])
    _, _, subject, off = rs.frame_masks(case['frame'])
    if case['name'] == 'empty_off_subject':
        assert subject.sum() > 0 and off.sum() == 0
    else:
        assert subject.sum() > 0 and off.sum() > 0, (int(subject.sum()), int(off.sum()))
    draws = tbr.draws_from_uniforms(case['u'], subject, off, case['cfg']['sample_subject_ratio'])
    r = rs.getitem(case['frame'], case['bgcolor'], draws)
    assert not r['_empty']
    case['check'](r)
    return r, draws
