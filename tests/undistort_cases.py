"""What tests/test_undistort_restatement.py (CPU) and tests/test_l_undistort.py (GPU) share: the two cameras of the issue,
the smooth test image, the forward lens model, and the tool-made distorted datasets."""
import os
import pickle

import numpy as np

from tests.train_batch_cases import load_tool

# name -> ((H, W), (fx, fy, cx, cy), D)
CAMERAS = {
    'A': ((96, 128), (110., 112., 63.3, 47.1), (-0.28, 0.11, 0.0012, -0.0009, -0.03)),
    'B': ((40, 72), (60., 58., 35.6, 19.2), (0.35, -0.05, 0.004, -0.003, 0.02, 0.01, 0.002, -0.001)),
}
D_RATIONAL = (0.2, -0.05, 0.004, -0.003, 0.02, 0.01, 0.002, -0.001)          # case A's camera with 8 coefficients
# the tool-made dataset of the dataset tests: 48 x 40, 5 frames, a mild barrel lens with tangential terms
TOOL = dict(frames=5, width=48, height=40, seed=41, focal=900.0)
TOOL_D = (-0.9, 0.6, 0.004, -0.003, -0.2)
# the band sits off the image's centre, where the lens moves the mask's columns: [31, 37)
BAND = {'range': 2, 'mid': 34, 'width': 6}


def matrix(fx, fy, cx, cy):
    return np.array([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]])


def case(name):
    (H, W), cam, D = CAMERAS[name]
    return H, W, matrix(*cam), np.array(D)


def smooth_image(H, W):
    """127+120 sin(x/9) cos(y/11), 127+120 sin((x+y)/13), 100+x+y (clipped at 255) as uint8 [H,W,3]."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    im = np.stack([127 + 120 * np.sin(x / 9) * np.cos(y / 11), 127 + 120 * np.sin((x + y) / 13), 100 + x + y], -1)
    return np.clip(np.rint(im), 0, 255).astype(np.uint8)


def forward_model(px, py, K, D):
    """Where the lens (K, D) records the ideal pixel position (px, py): OpenCV's projection model."""
    d = np.zeros(8)
    d[:len(D)] = D
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    x, y = (px - K[0, 2]) / K[0, 0], (py - K[1, 2]) / K[1, 1]
    r2 = x * x + y * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]


def make_tool_dataset(path, distortions=TOOL_D, all_cameras=0, **changes):
    load_tool().make_dataset(str(path), **{**TOOL, **changes}, all_cameras=all_cameras, distortions=distortions)
    return str(path)


def edit_pickle(path, name, fn):
    with open(os.path.join(path, name), 'rb') as f:
        obj = pickle.load(f)
    fn(obj)
    with open(os.path.join(path, name), 'wb') as f:
        pickle.dump(obj, f, protocol=4)
    return obj
