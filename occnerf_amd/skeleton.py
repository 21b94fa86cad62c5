"""The driving skeleton of an animate frame as a panel: the 23 bones and 24 joints of the frame's
posed skeleton, projected through the camera that made the frame's rays and drawn over the background colour by one HIP
launch (csrc/skeleton.hip).  A novel pose has no photograph to hold the render against; this panel is what tells an artefact
of the motion from one of the model.  The numpy definition, tests/skeleton_restatement.py, is the host function."""
import numpy as np

from . import ops

# One colour per joint; a bone takes its child's.  Left limbs warm, right limbs cold, the spine and head grey to white.
PALETTE = np.array([
    [120, 120, 120],   # 0  pelvis
    [230, 60, 50],     # 1  left hip
    [50, 110, 230],    # 2  right hip
    [150, 150, 150],   # 3  spine 1
    [240, 110, 40],    # 4  left knee
    [40, 160, 240],    # 5  right knee
    [175, 175, 175],   # 6  spine 2
    [250, 160, 30],    # 7  left ankle
    [30, 200, 230],    # 8  right ankle
    [200, 200, 200],   # 9  spine 3
    [250, 210, 20],    # 10 left foot
    [20, 230, 200],    # 11 right foot
    [225, 225, 225],   # 12 neck
    [200, 40, 120],    # 13 left collar
    [90, 60, 200],     # 14 right collar
    [90, 90, 90],      # 15 head
    [220, 50, 170],    # 16 left shoulder
    [120, 70, 220],    # 17 right shoulder
    [235, 80, 210],    # 18 left elbow
    [150, 90, 235],    # 19 right elbow
    [245, 120, 235],   # 20 left wrist
    [180, 120, 245],   # 21 right wrist
    [250, 170, 245],   # 22 left hand
    [210, 165, 250],   # 23 right hand
], dtype=np.uint8)
BONE_PX = 3.0          # animate.bone_px: a bone's half-width in pixels; a joint's disc has 1.5 x that


def background_u8(bgcolor):
    """cfg.bgcolor (0..255 floats) as the 3 bytes of an uncovered pixel: what to_8b_image makes of bgcolor / 255."""
    bg = np.clip(np.asarray(bgcolor, dtype=np.float32).reshape(3) / np.float32(255.), 0., 1.)
    return (np.float32(255.) * bg).astype(np.uint8)


def skeleton_panel(joints, K, E, height, width, device, bone_px=BONE_PX, bgcolor=(255., 255., 255.)):
    """joints [24,3] float32 in the body space of the camera matrix E, K [3,3], E [4,4] on the host -> (uint8 [H,W,3] on
    `device`, the count record of ops.skeleton_panel, for `counts`).  Nothing synchronises."""
    return ops.skeleton_panel(np.ascontiguousarray(joints, dtype=np.float32), K, E, height, width, bone_px, PALETTE,
                              background_u8(bgcolor), device)


def counts(record):
    """The count record of a panel on the host (one copy of 4 bytes per workgroup): joints dropped and pixels covered."""
    r = record.cpu().numpy() if hasattr(record, 'cpu') else np.asarray(record)
    return {'dropped': int(r[0]), 'covered': int(r[1:].astype(np.int64).sum())}
