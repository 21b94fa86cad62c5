"""CPU: occnerf_amd/undistort.py's undistort_u8 -- the definition the kernel csrc/undistort.hip is held to bit for bit
(tests/test_l_undistort.py) -- and what PreparedDataset(prepare_frames=True, device=None) makes of a distorted, cropped
dataset.  cv2 is not available, so the definition is held to what it claims to be instead of to a recording: the identity
for zero coefficients, exact bilinear sampling (scipy) of the unquantised map within the bound that the two quantisations
allow, the direction of the map (blobs painted through the forward lens model come back to their ideal positions), and a
round trip through the dataset tool's lens."""
import ctypes
import os

import numpy as np
import pytest
from scipy import ndimage

from occnerf_amd.undistort import source_coordinates, undistort_u8
from tests import undistort_cases as uc


# ---------------------------------------------------------------- 1. zero coefficients
@pytest.mark.parametrize('n', [4, 5, 8])
def test_zero_coefficients_reproduce_the_image(n):
    img = np.random.RandomState(n).randint(0, 256, size=(72, 40, 3)).astype(np.uint8)
    K = uc.matrix(61.3, 59.9, 19.37, 35.81)
    assert np.array_equal(undistort_u8(img, K, np.zeros(n)), img)
    assert np.array_equal(undistort_u8(img, K, np.zeros(n), window=(5, 3, 31, 17)), img[5:36, 3:20])


# ---------------------------------------------------------------- 2. against exact bilinear sampling
@pytest.mark.parametrize('name', ['A', 'B'])
def test_within_one_grey_level_of_exact_bilinear_sampling(name):
    """0.5 for the output rounding plus (16 + 16) / 64 for coordinates quantised to 1/32 px (at most 1/64 px off in either
    direction, on an image whose neighbours differ by at most 16).  Measured: A 0.76, B 0.70."""
    H, W, K, D = uc.case(name)
    img = uc.smooth_image(H, W)
    steps = img.astype(np.int64)
    assert max(np.abs(np.diff(steps, axis=0)).max(), np.abs(np.diff(steps, axis=1)).max()) <= 16
    out = undistort_u8(img, K, D)
    u, v = source_coordinates(H, W, K, D)
    inside = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    outside = (u <= -1) | (u >= W) | (v <= -1) | (v >= H)
    padded = np.pad(img.astype(np.float64), ((1, 1), (1, 1), (0, 0)))
    worst = 0.0
    for c in range(3):
        exact = ndimage.map_coordinates(padded[:, :, c], [v + 1, u + 1], order=1, mode='constant', cval=0.0)
        worst = max(worst, float(np.abs(out[:, :, c] - exact)[inside].max()))
    shares = float(outside.mean()), float((~inside & ~outside).mean())
    print(f'\n   {name}: worst |out - exact| = {worst:.3f} on {int(inside.sum())} pixels; outside {shares[0]:.3f}, '
          f'straddling {shares[1]:.3f}')
    assert inside.sum() > 0 and worst <= 1.0
    assert (out[outside] == 0).all()
    if name == 'B':                                       # the border taps are really exercised
        assert shares[0] >= 0.05 and shares[1] >= 0.03, shares


# ---------------------------------------------------------------- 3. direction of the map
@pytest.mark.parametrize('D', [uc.CAMERAS['A'][2], uc.D_RATIONAL], ids=['k3', 'rational'])
def test_blobs_painted_through_the_lens_come_back_to_their_ideal_positions(D):
    """An inverted map misses by more than 2 px; measured worst 0.095 px and 0.040 px."""
    H, W, K, _ = uc.case('A')
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    moved, worst = 0, 0.0
    for px in 20.37 + 22 * np.arange(5):
        for py in 18.61 + 20 * np.arange(4):
            assert px < W and py < H
            qx, qy = uc.forward_model(px, py, K, D)
            blob = 255.0 * np.exp(-((xx - qx) ** 2 + (yy - qy) ** 2) / (2 * 2.0 ** 2))
            img = np.repeat(np.rint(blob).astype(np.uint8)[:, :, None], 3, axis=2)
            out = undistort_u8(img, K, D)[:, :, 0].astype(np.float64)
            cx, cy = (out * xx).sum() / out.sum(), (out * yy).sum() / out.sum()
            if np.hypot(qx - px, qy - py) >= 1.0:
                moved += 1
                miss = float(np.hypot(cx - px, cy - py))
                worst = max(worst, miss)
                assert miss <= 0.25, (px, py, qx, qy, cx, cy)
    print(f'\n   {moved} of 20 points moved by >= 1 px; worst centroid miss {worst:.3f} px')
    assert moved >= 4


# ---------------------------------------------------------------- 4. coefficient shapes and refusals
@pytest.mark.parametrize('name', ['A', 'B'])
def test_coefficient_shapes_give_equal_results(name):
    H, W, K, D = uc.case(name)
    img = uc.smooth_image(H, W)
    want = undistort_u8(img, K, D)
    assert np.array_equal(undistort_u8(img, K, D.reshape(-1, 1)), want)
    assert np.array_equal(undistort_u8(img, K, D.reshape(1, -1)), want)
    assert np.array_equal(undistort_u8(img, K, list(D)), want)
    K4 = np.eye(4)
    K4[:3, :3] = K
    assert np.array_equal(undistort_u8(img, K4, D), want)
    if len(D) == 5:                                       # missing coefficients are 0
        assert np.array_equal(undistort_u8(img, K, np.concatenate([D, np.zeros(3)])), want)


def test_refusals_by_name(tmp_path):
    from occnerf_amd.dataset import PreparedDataset
    H, W, K, D = uc.case('B')
    img = uc.smooth_image(H, W)
    with pytest.raises(NotImplementedError, match='thin prism'):
        undistort_u8(img, K, np.zeros(12))
    with pytest.raises(NotImplementedError, match='tilt'):
        undistort_u8(img, K, np.zeros(14))
    skewed = K.copy()
    skewed[0, 1] = 0.01
    with pytest.raises(NotImplementedError, match='skew'):
        undistort_u8(img, skewed, D)
    with pytest.raises(ValueError, match='coefficients'):
        undistort_u8(img, K, np.zeros(6))
    with pytest.raises(ValueError, match='window'):
        undistort_u8(img, K, D, window=(0, 0, H + 1, W))
    path = uc.make_tool_dataset(tmp_path / 'd', frames=2)
    with pytest.raises(NotImplementedError, match='resize_img_scale'):
        PreparedDataset(path, device=None, volume_size=4, resize_img_scale=0.5, images_prescaled=True, prepare_frames=True)


# ---------------------------------------------------------------- 5. dataset rules, device=None
@pytest.fixture(scope='module')
def tool_path(tmp_path_factory):
    """48 x 40, 5 frames with 'distortions'; frame 3's camera has lost the key."""
    path = uc.make_tool_dataset(tmp_path_factory.mktemp('undistort') / 'data')
    uc.edit_pickle(path, 'cameras.pkl', lambda cams: cams['frame_000003'].pop('distortions'))
    return path


def raw(path, kind, name):
    from PIL import Image
    return np.array(Image.open(os.path.join(path, kind, name + '.png')).convert('RGB'))


def test_dataset_is_refused_by_default_and_opened_with_prepare_frames(tool_path):
    from occnerf_amd.dataset import PreparedDataset
    with pytest.raises(NotImplementedError, match='distortions'):
        PreparedDataset(tool_path, device=None, volume_size=4)
    with pytest.raises(NotImplementedError, match='crop_image_scale'):
        PreparedDataset(tool_path, device=None, volume_size=4, crop_image_scale=[31, 26])
    cams = uc.edit_pickle(tool_path, 'cameras.pkl', lambda cams: None)
    ds = PreparedDataset(tool_path, device=None, volume_size=4, occlude=True, occlusion=uc.BAND, prepare_frames=True)
    assert (ds.height, ds.width, len(ds)) == (40, 48, 5)
    for i, name in enumerate(ds.framelist):
        img, mask = raw(tool_path, 'images', name), raw(tool_path, 'masks', name)
        banded = mask.copy()
        if i < uc.BAND['range']:
            banded[:, 31:37] = 0
        cam = cams[name]
        assert np.array_equal(ds.frames[i]['K'], cam['intrinsics'])
        if i == 3:                                         # no key: the frame passes through unchanged
            assert 'distortions' not in cam
            assert np.array_equal(ds.images[i], img) and np.array_equal(ds.alphas[i], mask)
            continue
        assert np.array_equal(ds.images[i], undistort_u8(img, cam['intrinsics'], cam['distortions']))
        assert np.array_equal(ds.alphas[i], undistort_u8(banded, cam['intrinsics'], cam['distortions']))
        assert not np.array_equal(ds.images[i], img)
        if i < uc.BAND['range']:
            # the band is applied BEFORE the undistortion: the raw columns are zero, the prepared ones are what the
            # lens makes of them -- not all zero, and not what zeroing the undistorted mask would leave
            assert (banded[:, 31:37] == 0).all() and mask[:, 31:37].any()
            assert ds.alphas[i][:, 31:37].any()
            assert ds.frames[i]['band']


@pytest.mark.parametrize('crop', [[31, 26], [30, 27], [24, 24], [40, 48]], ids=lambda c: f'{c[0]}x{c[1]}')
def test_crop_is_the_reference_slice_and_sets_the_principal_point(crop, tool_path):
    from occnerf_amd.dataset import PreparedDataset
    full = PreparedDataset(tool_path, device=None, volume_size=4, occlude=True, occlusion=uc.BAND, prepare_frames=True)
    ds = PreparedDataset(tool_path, device=None, volume_size=4, occlude=True, occlusion=uc.BAND, prepare_frames=True,
                         crop_image_scale=crop)
    dx, dy = crop
    assert (ds.height, ds.width) == (dx, dy)
    mid_x, mid_y = 40 // 2, 48 // 2
    rows, cols = slice(mid_x - dx // 2, mid_x + (dx - dx // 2)), slice(mid_y - dy // 2, mid_y + (dy - dy // 2))
    for i in range(len(ds)):
        assert np.array_equal(ds.images[i], full.images[i][rows, cols])
        assert np.array_equal(ds.alphas[i], full.alphas[i][rows, cols])
        K, K0 = ds.frames[i]['K'], full.frames[i]['K']
        assert K[0, 2] == dx / 2 and K[1, 2] == dy / 2             # train.py:426-427, the row extent in cx
        assert K[0, 0] == K0[0, 0] and K[1, 1] == K0[1, 1]
        assert ds.frames[i]['empty'] == (int(ds.alphas[i].astype(np.int64).sum()) < 255)
    if crop == [31, 26]:
        assert ds.frames[0]['K'][0, 2] == 15.5 and ds.frames[0]['K'][1, 2] == 13.0
        assert (rows, cols) == (slice(5, 36), slice(11, 37))
    w = ds.whole_frame(2, [255., 255., 255.])                       # the host frame is built at the prepared size
    assert w['img_height'] == dx and w['img_width'] == dy and w['ray_mask'].shape == (dx * dy,)


@pytest.mark.parametrize('crop', [[41, 26], [31, 49], [0, 10]], ids=lambda c: f'{c[0]}x{c[1]}')
def test_a_crop_that_does_not_fit_is_refused(crop, tool_path):
    from occnerf_amd.dataset import PreparedDataset
    with pytest.raises(ValueError, match='crop_image_scale'):
        PreparedDataset(tool_path, device=None, volume_size=4, prepare_frames=True, crop_image_scale=crop)


def test_empty_follows_the_prepared_mask(tmp_path):
    """A mask that lives in the image's corner only: not empty as recorded, empty once the crop has taken the corner."""
    from PIL import Image
    from occnerf_amd.dataset import PreparedDataset
    path = uc.make_tool_dataset(tmp_path / 'corner', frames=3)
    corner = np.zeros((40, 48), np.uint8)
    corner[:4, :4] = 255
    Image.fromarray(corner, 'L').save(os.path.join(path, 'masks', 'frame_000001.png'))
    ds = PreparedDataset(path, device=None, volume_size=4, prepare_frames=True)
    assert [f['empty'] for f in ds.frames] == [False, False, False] and ds.alphas[1].any()
    ds = PreparedDataset(path, device=None, volume_size=4, prepare_frames=True, crop_image_scale=[31, 26])
    assert [f['empty'] for f in ds.frames] == [False, True, False] and ds.epoch_frames == [0, 2]
    assert not ds.alphas[1].any()


def test_from_cfg_prepares_unless_told_not_to(tool_path):
    from occnerf_amd import config
    from occnerf_amd.dataset import PreparedDataset
    cfg = config.default_cfg()
    cfg.resize_img_scale = 1.0
    cfg.mweight_volume.volume_size = 4
    cfg.crop_image_scale = [31, 26]
    ds = PreparedDataset.from_cfg(cfg, tool_path, device=None)
    assert (ds.height, ds.width) == (31, 26)
    ds = PreparedDataset.from_cfg(cfg, tool_path, device=None, crop_image_scale=[-1, -1])      # views.py's open
    assert (ds.height, ds.width) == (40, 48)
    cfg.train.prepare_frames = False
    with pytest.raises(NotImplementedError, match='crop_image_scale'):
        PreparedDataset.from_cfg(cfg, tool_path, device=None)


def test_allview_host_truth_is_the_raw_photograph_through_each_rig_camera(tmp_path):
    from occnerf_amd.dataset import PreparedDataset
    from occnerf_amd.views import ViewFrames
    path = uc.make_tool_dataset(tmp_path / 'wild_rig', frames=2, all_cameras=6)

    def vary(rigs):                                        # a lens of its own for every camera of the rig
        for rig in rigs.values():
            rig['distortions'] = rig['distortions'] * (1.0 + 0.1 * np.arange(6))[:, None]
            rig['intrinsics'] = rig['intrinsics'].copy()
            rig['intrinsics'][:, 0, 2] += 0.25 * np.arange(6)
    rigs = uc.edit_pickle(path, 'all_cameras.pkl', vary)
    ds = PreparedDataset(path, device=None, volume_size=4, prepare_frames=True)
    views = ViewFrames(ds, 'allview', src_type='wild', frame_idx=1)
    assert len(views) == 6
    photo, rig = raw(path, 'images', 'frame_000001'), rigs['frame_000001']
    panels = [views.frame(i)['truth_u8'] for i in range(6)]
    for i in range(6):
        assert np.array_equal(panels[i], undistort_u8(photo, rig['intrinsics'][i], rig['distortions'][i]))
    assert np.array_equal(panels[0], ds.images[1])          # camera 0 is the frame's own camera and lens
    assert not np.array_equal(panels[5], panels[0]) and not np.array_equal(panels[5], photo)
    assert 'truth_u8' not in ViewFrames(ds, 'allview', src_type='wild', frame_idx=1, truth=False).frame(0)


# ---------------------------------------------------------------- 6. round trip through the tool
def test_undistorting_the_tools_masks_gives_back_the_clean_masks(tmp_path):
    """Two bilinear resamplings move an edge by at most a pixel each, and a sample whose four taps are 255 (or 0) is 255 (or
    0): away from the clean mask's edges, and from the image's, the round trip is exact."""
    H, W = 96, 128                                         # the body is wide enough for an interior 3 px from its edges
    clean_path = uc.make_tool_dataset(tmp_path / 'clean', distortions=None, frames=2, width=W, height=H)
    path = uc.make_tool_dataset(tmp_path / 'lens', frames=2, width=W, height=H)
    cams = uc.edit_pickle(path, 'cameras.pkl', lambda cams: None)
    for name in ('frame_000000', 'frame_000001'):
        clean, recorded = raw(clean_path, 'masks', name)[:, :, 0], raw(path, 'masks', name)
        assert not np.array_equal(clean, recorded[:, :, 0])
        K, D = cams[name]['intrinsics'], cams[name]['distortions']
        got = undistort_u8(recorded, K, D)[:, :, 0]
        # >= 3 px (Chebyshev) from any edge of the clean mask: the 7 x 7 neighbourhood is constant; beyond the image counts
        # as an edge (-1 is no mask value)
        ext = np.pad(clean.astype(np.int64), 3, constant_values=-1)
        flat = (ndimage.minimum_filter(ext, size=7) == ndimage.maximum_filter(ext, size=7))[3:-3, 3:-3]
        u, v = source_coordinates(H, W, K, D)
        kept = (u >= 3) & (u <= W - 1 - 3) & (v >= 3) & (v <= H - 1 - 3)
        ok = flat & kept
        print(f'\n   {name}: {int(ok.sum())} of {H * W} pixels qualify, {int((clean[ok] == 255).sum())} of them on the body')
        assert ok.sum() >= H * W // 2 and (clean[ok] == 255).any() and (clean[ok] == 0).any()
        assert np.array_equal(got[ok], clean[ok])


# ---------------------------------------------------------------- 7. ABI
def test_entry_point_is_declared_exported_and_refuses_bad_arguments():
    from occnerf_amd import _lib
    assert 'occnerf_undistort_u8' in _lib.SIGNATURES
    lib = _lib.lib()
    assert lib.occnerf_abi_version() == 5 == _lib.ABI_VERSION
    rc = lib.occnerf_undistort_u8(None, None, 8, 8, None, None, 0, 0, 8, 8, None, None, None)
    assert rc != 0 and b'null' in lib.occnerf_last_error() and b'undistort_u8' in lib.occnerf_last_error()
    # non-null (host) pointers that are never dereferenced: the arguments are refused before any launch
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    K = np.ascontiguousarray(uc.matrix(10., 10., 4., 4.).reshape(9))
    d = np.zeros(8)
    for window in ((0, 0, 9, 8), (0, 1, 8, 8), (-1, 0, 4, 4), (0, 0, 0, 4)):
        rc = lib.occnerf_undistort_u8(p, None, 8, 8, K.ctypes.data, d.ctypes.data, *window, p, None, None)
        assert rc != 0 and b'window' in lib.occnerf_last_error() and b'undistort_u8' in lib.occnerf_last_error(), window
    rc = lib.occnerf_undistort_u8(p, None, 1 << 14, 1 << 14, K.ctypes.data, d.ctypes.data, 0, 0, 8, 8, p, None, None)
    assert rc != 0 and b'bad image size' in lib.occnerf_last_error()
    rc = lib.occnerf_undistort_u8(p, p, 8, 8, K.ctypes.data, d.ctypes.data, 0, 0, 8, 8, p, None, None)
    assert rc != 0 and b'come together' in lib.occnerf_last_error()
    K[1] = 0.5
    rc = lib.occnerf_undistort_u8(p, None, 8, 8, K.ctypes.data, d.ctypes.data, 0, 0, 8, 8, p, None, None)
    assert rc != 0 and b'skew' in lib.occnerf_last_error()
