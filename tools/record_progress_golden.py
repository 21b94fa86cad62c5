"""Record tests/golden/progress_mosaic_ref.npz from the UNMODIFIED reference's core.utils.image_util.to_8b_image and
tile_images (image_util.py:19-20, :38-50), on the CPU, where the reference tree is present:

    python tools/record_progress_golden.py

Both functions are pure numpy; the reference module is imported under oracle.ref_harness.shims.install (the stand-ins for
what its imports need), as tools/record_view_frames_golden.py does.  Only arrays are stored: for k in 1, 3, 4, 5, 9 and 16
random uint8 panels of 6 x 10 x 3 the reference's tiling of the first k, and for one float32 array (values below 0, above 1,
exact multiples of 1/255 and their float32 neighbours, random ones) its quantisation."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from oracle.ref_harness import shims  # noqa: E402

OUT_DIR = os.environ.get('OCCNERF_GOLDEN_DIR') or os.path.join(REPO, 'tests', 'golden')
KS = (1, 3, 4, 5, 9, 16)
PANEL = (6, 10, 3)


def quantiser_input():
    rng = np.random.RandomState(11)
    grid = (np.arange(256) / 255.).astype(np.float32)
    return np.concatenate([grid, np.nextafter(grid, np.float32(-1)), np.nextafter(grid, np.float32(2)),
                           np.array([-1.5, -1e-7, -0.0, 0.0, 1.0, 1.0000001, 7.25], np.float32),
                           rng.uniform(-0.25, 1.25, 512).astype(np.float32)]).astype(np.float32)


def main():
    shims.install(['run.py', '--cfg', 'configs/occnerf/zju_mocap/387/occnerf.yaml'])
    from core.utils.image_util import tile_images, to_8b_image          # the reference's
    rng = np.random.RandomState(7)
    panels = rng.randint(0, 256, size=(max(KS),) + PANEL).astype(np.uint8)
    x = quantiser_input()
    out = {'panels': panels, 'ks': np.array(KS, np.int64), 'q.in': x, 'q.out': to_8b_image(x)}
    for k in KS:
        out[f'tiled.{k}'] = tile_images([panels[i] for i in range(k)])
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, 'progress_mosaic_ref.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
