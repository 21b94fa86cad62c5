"""The cases of tests/test_h_whole_frame.py: which tool-made dataset, which frame, and the coverage condition each case has
to meet on the host path BEFORE anything is compared -- a case that silently degenerates (no empty row, no second chunk, a
box that covers the image) shows nothing.  Loaded the way tests/train_batch_cases.py loads its datasets."""
import os

import numpy as np

from tests.train_batch_cases import load_tool

# name -> (dataset key, frame); dataset key -> make_dataset arguments (2 frames each)
DATASETS = {'wide': dict(width=96, height=80, focal=900.0, seed=11), 'near': dict(width=96, height=80, focal=2600.0, seed=12),
            'long': dict(width=300, height=37, focal=2200.0, seed=16), 'tall': dict(width=40, height=300, focal=900.0, seed=15),
            'tiny': dict(width=7, height=7, focal=900.0, seed=17)}
CASES = {'wide': ('wide', 0), 'full': ('near', 1), 'nearly_full': ('near', 0), 'two_chunks': ('long', 0),
         'tall_scan': ('tall', 0), 'tiny': ('tiny', 0)}
BGCOLORS = {'white': [255., 255., 255.], 'colour': [30., 200., 90.]}


def make_datasets(base, only=None):
    paths = {}
    for key, kw in DATASETS.items():
        if only is None or key in only:
            paths[key] = os.path.join(str(base), key)
            load_tool().make_dataset(paths[key], frames=2, **kw)
    return paths


def open_case(name, paths, device=None):
    from occnerf_amd.dataset import PreparedDataset
    key, frame = CASES[name]
    return PreparedDataset(paths[key], device=device, volume_size=4), frame


def check_condition(name, ds, frame, w):
    """Asserts the case's coverage condition on the host dict `w` = ds.whole_frame(frame, bgcolor); -> a line to print."""
    H, W = ds.height, ds.width
    mask = np.asarray(w['ray_mask']).reshape(H, W)
    R, per_row = int(mask.sum()), mask.sum(1)
    empty_rows = int((per_row == 0).sum())
    m = ds.alphas[frame]
    fractional = int(((m > 0) & (m < 255)).any(-1).sum())
    assert fractional > 0, f'{name}: no fractional mask value, the blend is not exercised'
    outside_subject = int(((m[:, :, 0] > 0) & ~mask).sum())
    if name == 'wide':
        assert 0 < R < H * W and empty_rows >= 1, (R, empty_rows)
    elif name == 'full':
        assert R == H * W, R
    elif name == 'nearly_full':
        assert H * W - 64 < R < H * W, R
    elif name == 'two_chunks':
        assert per_row.max() > 256 and R < H * W and W % 64 != 0, (int(per_row.max()), R, W)
    elif name == 'tall_scan':
        assert H > 256 and empty_rows >= 1, (H, empty_rows)
    elif name == 'tiny':
        assert 0 < R < 49 and (H, W) == (7, 7) and outside_subject > 0, (R, outside_subject)
    else:
        raise KeyError(name)
    return (f'{name}: {W} x {H}, R {R} of {H * W}, {empty_rows} empty rows, max {int(per_row.max())} per row, '
            f'{fractional} fractional mask pixels, {outside_subject} subject pixels outside the box')
