"""A numpy statement of the reference trainer's progress image (core/train/trainers/occnerf/trainer.py:337-383 with
core/utils/image_util.py:19-20 and :38-50), written from those lines for the tests of occnerf_amd/progress.py and
csrc/progress.hip.  Nothing here is shared with the code under test.

  * panels (trainer.py:350-372): two float32 images filled with cfg.bgcolor / 255, the rays' colours and the targets written
    at ray_mask, each quantised by to_8b_image (image_util.py:19-20: (255. * clip(x, 0, 1)).astype(uint8)), the rendered one
    left of the truth;
  * the empty test (trainer.py:375-378): only while iter <= 5000, np.allclose(rendered, cfg.bgcolor, atol=3.) on the 8-bit
    rendered panel against the float64 colour -- |a - b| <= atol + rtol * |b| elementwise, rtol 1e-5 -- ends the loop AFTER
    the frame's panels were appended;
  * tile_images (image_util.py:38-50): rows of min(len, 4) panels; a row is kept only when full (the `rows.pop()` of :47-48
    compares the heights of two full rows and never fires for equal-sized panels)."""
import numpy as np

PER_ROW = 4
EMPTY_CHECK_UNTIL = 5000


def to_8b_image(image):
    """image_util.py:19-20."""
    return (255. * np.clip(image, 0., 1.)).astype(np.uint8)


def panels(width, height, ray_mask, bgcolor, rgb, target_rgbs=None, truth_u8=None):
    """trainer.py:350-372 -> (rendered, truth) uint8 [H,W,3].  truth_u8: the truth panel itself where the caller already holds
    the frame's photograph as 8-bit pixels (a prepared dataset's device frame) instead of target_rgbs."""
    rendered = np.full((height * width, 3), np.array(bgcolor) / 255., dtype='float32')
    rendered[np.asarray(ray_mask, bool)] = rgb
    rendered = to_8b_image(rendered.reshape((height, width, -1)))
    if truth_u8 is None:
        truth = np.full((height * width, 3), np.array(bgcolor) / 255., dtype='float32')
        truth[np.asarray(ray_mask, bool)] = target_rgbs
        truth_u8 = to_8b_image(truth.reshape((height, width, -1)))
    return rendered, np.asarray(truth_u8)


def off_background(rendered, bgcolor, atol=3., rtol=1e-5):
    """The elements of the 8-bit rendered panel np.allclose(rendered, bgcolor, atol=3.) objects to: numpy's rule
    |a - b| <= atol + rtol * |b| with a promoted to float64 -> their count."""
    b = np.array(bgcolor)
    return int((~(np.abs(rendered - b) <= atol + rtol * np.abs(b))).sum())


def is_empty(rendered, bgcolor):
    """trainer.py:376."""
    return bool(np.allclose(rendered, np.array(bgcolor), atol=3.))


def tile_images(images, imgs_per_row=PER_ROW):
    """image_util.py:38-50 for panels of one size."""
    per_row = min(len(images), imgs_per_row)
    n_rows = len(images) // per_row
    return np.concatenate([np.concatenate(images[r * per_row:(r + 1) * per_row], axis=1) for r in range(n_rows)], axis=0)


def progress_image(frames, bgcolor, it):
    """trainer.py:337-383 over `frames`, a list of (rendered, truth) panel pairs in loader order -> (the tiled image, is_empty,
    the number of frames the loop visited)."""
    images, empty = [], False
    for rendered, truth in frames:
        images.append(np.concatenate([rendered, truth], axis=1))
        if it <= EMPTY_CHECK_UNTIL and is_empty(rendered, bgcolor):
            empty = True
            break
    return tile_images(images), empty, len(images)


def crop_of_full(full, k, n, height, width):
    """What the issue states about the early stop: the image of "frame k-1 is the first empty one" as a crop of the full
    n-frame mosaic -- the top k // 4 tile rows for k >= 4, the first k tiles of row 0 for k < 4 (n >= k)."""
    per_row = min(n, PER_ROW)
    if k >= per_row:
        return full[:(k // per_row) * height]
    return full[:height, :k * 2 * width]


def schedule(it, dump_interval=500):
    """trainer.py:269-270 as a literal rule."""
    return it in [20, 100, 300, 1000, 2500] or (dump_interval > 0 and it % dump_interval == 0)
