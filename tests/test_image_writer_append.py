"""CPU: ImageWriter.append -- the host-array entry of the PNG writer thread, the reference's image_util.py:53-75 -- still
writes its files now that the same thread also writes the geometry maps' archives (ImageWriter.append_device_npz)."""
import os

import numpy as np


def test_append_of_host_arrays_writes_the_pngs(tmp_path):
    from PIL import Image
    from occnerf_amd.image import ImageWriter
    rng = np.random.RandomState(3)
    imgs = [rng.randint(0, 256, (5, 7, 3)).astype(np.uint8), rng.randint(0, 256, (4, 4, 3)).astype(np.uint8)]
    w = ImageWriter(output_dir=str(tmp_path), exp_name='host')
    assert w.append(imgs[0]) == (0, '000000')
    assert w.append(imgs[1], img_name='named') == (1, 'named')
    w.finalize()                                               # an error of the writer thread would be raised here
    assert not w._thread.is_alive()
    assert sorted(os.listdir(tmp_path / 'host')) == ['000000.png', 'named.png']
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'host' / '000000.png')), imgs[0])
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'host' / 'named.png')), imgs[1])
