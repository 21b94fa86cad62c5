"""The three per-pixel maps of a dataset frame in numpy, from a PreparedDataset.whole_frame() dict: what eval.py's metrics
take as truth image, gt_vis and gt_alpha.  tests/test_train_batch_restatement.py holds whole_frame() itself to a recording of
the unmodified reference; image.unpack_to_image is the reference's run.py:46-63."""
import numpy as np

from occnerf_amd.image import unpack_to_image


def maps(w, mask_u8, bgcolor):
    """w: the whole_frame() dict; mask_u8: the frame's resident mask uint8 [H,W,3]; bgcolor in 0..255.
    -> truth_u8 [H,W,3] uint8, gt_vis [H,W] float32, gt_alpha [H,W] float32."""
    H, W = int(w['img_height']), int(w['img_width'])
    ray_mask = np.asarray(w['ray_mask'])
    bg01 = np.array(bgcolor, dtype='float32').astype(np.float64) / 255.              # eval.py: np.array(cfg.bgcolor) / 255.
    R = int(ray_mask.sum())
    _, _, truth = unpack_to_image(W, H, ray_mask, bg01, np.zeros((R, 3), 'float32'), np.zeros(R, 'float32'),
                                  truth=np.asarray(w['target_rgbs']))
    gt_vis = np.zeros(H * W, dtype='float32')                                        # metrics.pixel_map's scatter
    gt_vis[ray_mask] = np.asarray(w['ray_alpha'])[:, 0]
    gt_alpha = (mask_u8[:, :, 0] / 255.).astype('float32')
    return truth, gt_vis.reshape(H, W), gt_alpha
