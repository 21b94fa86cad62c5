"""The cases of tests/test_animate_restatement.py and tests/test_s_animate.py: tool-made datasets (5 frames of 96 x 80, seeds 0
and 1), and the skeletons of the panel's hand cases with the property each is there for.

A hand case is written in PIXELS: {joint: (u, v, z)} through the camera K = [[100, 0, 48], [0, 100, 40], [0, 0, 1]], E = I;
every joint it does not name stands behind the camera (z = -1) and is dropped.  All of them share BASE, five joints and four
bones in the middle of a 96 x 80 image, so every case covers pixels with at least two bones; what a case adds stands in the
free corners.  The same skeletons are painted at every size of SIZES: a smaller image is a crop, the camera stays."""
import importlib.util
import os

import numpy as np

from occnerf_amd import synth
from occnerf_amd.skeleton import PALETTE, background_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 80
SIZES = ((1, 1), (64, 1), (67, 45), (96, 80))              # (width, height)
K_HAND = np.array([[100., 0., 48.], [0., 100., 40.], [0., 0., 1.]])
E_HAND = np.eye(4)
BG = background_u8([255., 255., 255.])
BONE_PX = 3.0

# pelvis, the hips and the knees: bones (1,0), (2,0), (4,1), (5,2); the two hip bones and the pelvis disc overlap at joint 0
BASE = {0: (48., 20., 2.), 1: (30., 40., 2.), 2: (66., 40., 2.), 4: (30., 70., 2.5), 5: (66., 70., 1.5)}
BONE_OF = {child: child - 1 for child in range(1, 24)}     # the primitive index of the bone that ends in `child`


def load_tool():
    spec = importlib.util.spec_from_file_location('make_synthetic_dataset', os.path.join(ROOT, 'tools', 'make_synthetic_dataset.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_datasets(base, frames=5):
    """{0: the subject's directory (seed 0), 1: the motion's (seed 1)}, 96 x 80."""
    tool = load_tool()
    paths = {seed: os.path.join(str(base), f'seed{seed}') for seed in (0, 1)}
    for seed, path in paths.items():
        tool.make_dataset(path, frames=frames, width=W, height=H, seed=seed, focal=900.0)
    return paths


def joints_of_pixels(spec):
    """float32 [24,3] camera-space joints (E = I) that K_HAND sends to the (u, v) of `spec` at depth z; the rest behind."""
    j = np.zeros((24, 3), dtype=np.float64)
    j[:, 2] = -1.0
    for k, (u, v, z) in spec.items():
        j[k] = ((u - K_HAND[0, 2]) * z / K_HAND[0, 0], (v - K_HAND[1, 2]) * z / K_HAND[1, 1], z)
    return j.astype(np.float32)


def hand_cases():
    """name -> {'joints', 'K', 'E', 'dropped' (expected count), 'what'}."""
    def case(extra, what, **more):
        spec = {**BASE, **extra}
        joints = joints_of_pixels(spec)
        return dict({'joints': joints, 'K': K_HAND, 'E': E_HAND, 'dropped': 24 - len(spec), 'what': what}, **more)

    nan_joint = case({8: (66., 70., 1.5)}, 'bone (8,5) has zero length: a disc of the bone\'s width; joint 11 is not finite')
    nan_joint['joints'][11] = (np.nan, 0.1, 2.0)
    return {
        # bone (18,16) lies beyond the right and lower border; its parent bone (16,13) is dropped with joint 13
        'off_screen': case({16: (200., 300., 2.), 18: (260., 320., 2.)}, 'bone (18,16) is entirely off screen'),
        # bone (19,17) leaves through the upper right corner
        'border': case({17: (80., 10., 2.), 19: (120., -20., 2.)}, 'bone (19,17) crosses the border'),
        # joint 7 behind the camera: bones (7,4) and (10,7) go, the disc of joint 10 stays
        'behind': case({10: (12., 12., 2.)}, 'joint 7 is behind the camera, its two bones are dropped', behind=7),
        'zero_length': nan_joint,
        # two bones crossing in the lower left corner at (13, 60): (18,16) at depth 1, (19,17) at depth 3 -> the nearer wins
        'cross_depths': case({16: (4., 48., 1.), 18: (22., 72., 1.), 17: (4., 72., 3.), 19: (22., 48., 3.)},
                             'two bones cross at different depths', cross=((13, 60), BONE_OF[18])),
        # ... and at equal depth keys (1 + 3) / 2 = (2 + 2) / 2: the higher index wins
        'cross_equal': case({16: (4., 48., 1.), 18: (22., 72., 3.), 17: (4., 72., 2.), 19: (22., 48., 2.)},
                            'two bones cross at equal depth keys', cross=((13, 60), BONE_OF[19])),
    }


def generic_case():
    """A seeded pose of the synthetic skeleton through the tpose camera at 96 pixels, raised to the image's middle."""
    joints = synth.posed_joints(synth.seeded_pose(3), synth.tpose_joints(np.zeros(10, dtype='float32')))
    K, E = synth.setup_camera(W, focal=1250.0)
    K = K.astype(np.float64)
    K[1, 2] = H / 2.0
    return {'joints': joints.astype(np.float32), 'K': K, 'E': E.astype(np.float64), 'dropped': 0, 'what': 'a generic pose'}


def all_dropped_case():
    return {'joints': joints_of_pixels({}), 'K': K_HAND, 'E': E_HAND, 'dropped': 24, 'what': 'every joint is dropped'}


def all_cases():
    return dict(hand_cases(), generic=generic_case(), all_dropped=all_dropped_case())


def definition_args(case, width=W, height=H):
    return {'joints': case['joints'], 'K': case['K'], 'E': case['E'], 'height': height, 'width': width, 'bone_px': BONE_PX,
            'palette': PALETTE, 'bgcolor_u8': BG}
