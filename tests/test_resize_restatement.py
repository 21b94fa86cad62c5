"""CPU: occnerf_amd/resize.py against an independent restatement of the same formulas
(tests/resize_cases.py), the filters against their closed forms, and the dataset rules of `resize_frames`."""
import numpy as np
import pytest

from occnerf_amd import resize
from tests import resize_cases as rc
from tests import undistort_cases as uc


# ---------------------------------------------------------------- 1. resize.py is the restatement, bit for bit
@pytest.mark.parametrize('bg', list(rc.BGCOLORS))
@pytest.mark.parametrize('name', list(rc.CASES))
def test_resize_blend_equals_the_restatement(name, bg):
    H, W, s = rc.CASES[name]
    image, mask = rc.random_frame(name)
    assert resize.resized_size(H, W, s) == rc.SIZES[name]
    img64, alpha64 = resize.resize_blend(image, mask, rc.BGCOLORS[bg], s)
    want_img, want_alpha = rc.restate(image, mask, rc.BGCOLORS[bg], s)
    assert img64.dtype == alpha64.dtype == np.float64 and img64.shape == alpha64.shape == rc.SIZES[name] + (3,)
    assert np.array_equal(img64, want_img) and np.array_equal(alpha64, want_alpha)
    none, alone = resize.resize_blend(None, mask, None, s)
    assert none is None and np.array_equal(alone, want_alpha)
    print(f'\n   {name}: img64 in [{img64.min():.1f}, {img64.max():.1f}]')


def test_sizes_round_ties_to_even_and_an_empty_result_is_refused_by_name():
    assert resize.resized_size(41, 47, 0.5) == (20, 24) and resize.resized_size(43, 45, 0.5) == (22, 22)
    assert resize.resized_size(2, 2, 0.5) == (1, 1)
    with pytest.raises(ValueError, match='resize_img_scale'):
        resize.resized_size(1, 1, 0.5)                         # rint(0.5) = 0
    with pytest.raises(ValueError, match='resize_img_scale'):
        resize.resize_blend(None, np.zeros((1, 1, 3), np.uint8), None, 0.5)
    for bad in (0.0, -0.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='resize_img_scale'):
            resize.resized_size(40, 48, bad)
    with pytest.raises(ValueError, match='kind'):
        resize.resize_tables(40, 0.5, 'cubic')
    with pytest.raises(ValueError, match='mask'):
        resize.resize_blend(None, np.zeros((4, 4), np.uint8), None, 0.5)
    with pytest.raises(ValueError, match='image'):
        resize.resize_blend(np.zeros((4, 6, 3), np.uint8), np.zeros((4, 4, 3), np.uint8), [0, 0, 0], 0.5)


def test_tables_are_clamped_and_shaped():
    for n_src, s in ((40, 0.5), (41, 0.3), (9, 0.5), (2, 0.5), (48, 0.75), (7, 2.0)):
        n_dst = int(np.rint(n_src * s))
        for kind, taps in ((resize.LANCZOS, 8), (resize.BILINEAR, 2)):
            off, w = resize.resize_tables(n_src, s, kind)
            assert off.shape == w.shape == (n_dst, taps) and off.dtype == np.int32 and w.dtype == np.float32
            assert off.min() >= 0 and off.max() <= n_src - 1 and (np.diff(off, axis=0) >= 0).all() and (np.diff(off, axis=1) >= 0).all()
            for d in range(n_dst):                             # the restatement's taps, entry for entry
                want = rc.taps(d, s, n_src, kind)
                assert [int(v) for v in off[d]] == [j for j, _ in want]
                assert all(np.float32(a) == b for a, (_, b) in zip(w[d], want))


# ---------------------------------------------------------------- 2. the filters
def test_lanczos_weights_are_the_closed_form_within_1e_6():
    worst = 0.0
    ts = [np.float32(v) for v in np.linspace(0.0, 1.0, 4097)[:-1]] + [np.float32(0.5), np.float32(1e-6), np.float32(1 - 1e-6)]
    for n_src, s in ((41, 0.3), (48, 0.75), (300, 0.5)):      # and every fraction the cases meet
        ts += [rc.position(d, s)[1] for d in range(int(np.rint(n_src * s)))]
    for t in ts:
        w = resize.lanczos_weights(t)
        assert w.dtype == np.float32 and w.shape == (8,)
        worst = max(worst, float(np.abs(w.astype(np.float64) - rc.closed_form(t)).max()))
    print(f'\n   {len(ts)} fractions: max |w - closed form| = {worst:.3e}')
    assert worst <= 1e-6
    assert np.array_equal(resize.lanczos_weights(np.float32(0.0)), np.array([0, 0, 0, 1, 0, 0, 0, 0], np.float32))


@pytest.mark.parametrize('name', ['40x48@0.5', '41x47@0.3', '40x48@0.75'])
def test_a_constant_image_comes_back_within_1e_6(name):
    """Eight float32 weights per axis that sum to 1 within float32 rounding, sum |w| < 2, two axes."""
    H, W, s = rc.CASES[name]
    full = np.full((H, W, 3), 255, np.uint8)
    for c in (1, 37, 200, 255):
        img64, alpha64 = resize.resize_blend(np.full((H, W, 3), c, np.uint8), full, [9., 9., 9.], s)
        err = float(np.abs(img64 - c).max()) / c
        print(f'\n   {name} c={c}: max |img64 - c| / c = {err:.3e}')
        assert err <= 1e-6
        assert np.abs(alpha64 - 1.0).max() <= 1e-6


@pytest.mark.parametrize('name', ['40x48@0.5', '2x2@0.5'])
def test_bilinear_at_one_half_on_even_sizes_is_the_block_mean(name):
    H, W, s = rc.CASES[name]
    _, mask = rc.random_frame(name)
    alpha64 = resize.resize_blend(None, mask, None, s)[1]
    a = mask / 255.
    mean = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]) / 4
    assert np.abs(alpha64 - mean).max() <= 1e-15


# ---------------------------------------------------------------- 3. the dataset rules, device=None
@pytest.fixture(scope='module')
def plain_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('resize') / 'plain')
    rc.load_tool().make_dataset(path, **rc.DATASET)
    return path


def test_refusals_are_unchanged_without_the_flag(plain_path):
    from occnerf_amd.dataset import PreparedDataset
    with pytest.raises(NotImplementedError, match='resize_img_scale.*resize_frames'):
        PreparedDataset(plain_path, device=None, volume_size=4, resize_img_scale=0.5)
    with pytest.raises(NotImplementedError, match='resize_img_scale'):
        PreparedDataset(plain_path, device=None, volume_size=4, resize_img_scale=0.5, images_prescaled=True,
                        prepare_frames=True, crop_image_scale=[40, 48])
    with pytest.raises(ValueError, match='images_prescaled'):
        PreparedDataset(plain_path, device=None, volume_size=4, resize_img_scale=0.5, images_prescaled=True, resize_frames=True)
    with pytest.raises(ValueError, match='images_prescaled'):
        PreparedDataset(plain_path, device=None, volume_size=4, images_prescaled=True, resize_frames=True)


def test_scale_one_resizes_nothing(plain_path):
    from occnerf_amd.dataset import PreparedDataset
    a = PreparedDataset(plain_path, device=None, volume_size=4, resize_frames=True)
    b = PreparedDataset(plain_path, device=None, volume_size=4)
    assert not a.resizing and a.resize_tables is None and (a.height, a.width) == (b.height, b.width) == (80, 96)
    wa, wb = a.whole_frame(1, [3., 4., 5.]), b.whole_frame(1, [3., 4., 5.])
    assert all(np.array_equal(wa[k], wb[k]) for k in ('target_rgbs', 'ray_alpha', 'ray_mask', 'rays'))


def test_sizes_K_empty_and_the_host_whole_frame(plain_path):
    from occnerf_amd.dataset import PreparedDataset, WholeFrames
    full = PreparedDataset(plain_path, device=None, volume_size=4, occlude=True, occlusion=rc.BAND)
    ds = PreparedDataset(plain_path, device=None, volume_size=4, occlude=True, occlusion=rc.BAND, resize_img_scale=0.5,
                         resize_frames=True)
    assert ds.resizing and (ds.src_height, ds.src_width, ds.height, ds.width) == (80, 96, 40, 48)
    assert ds.frames[0]['empty'] and ds.epoch_frames == [1, 2] and len(ds) == 3
    bg = [12.25, 200.7, 99.33]
    for i in range(3):
        assert np.array_equal(ds.images[i], full.images[i]) and np.array_equal(ds.alphas[i], full.alphas[i])    # resident: full size
        assert np.array_equal(ds.frames[i]['K'][:2], full.frames[i]['K'][:2] * 0.5) and ds.frames[i]['K'][2, 2] == 1.0
        img64, alpha64 = resize.resize_blend(ds.images[i], ds.alphas[i], bg, 0.5)
        assert ds.frames[i]['empty'] == bool(np.sum(alpha64) < 1)
        w = ds.whole_frame(i, bg)
        want = rc.consumer_frame(ds, i, bg, (img64, alpha64))
        assert sorted(k for k in want if not k.startswith('_')) == sorted(k for k in w if k in want)
        assert w['img_height'] == 40 and w['img_width'] == 48 and w['ray_mask'].shape == (40 * 48,)
        n = int(w['ray_mask'].sum())
        assert w['rays'].shape == (2, n, 3) and w['target_rgbs'].shape == (n, 3) and w['ray_alpha'].shape == (n, 3)
        assert w['target_rgbs'].dtype == np.float32 and w['ray_alpha'].dtype == np.float64
        for k in ('ray_mask', 'rays', 'near', 'far', 'target_rgbs', 'ray_alpha'):
            assert np.array_equal(w[k], want[k]), k
        assert np.array_equal(ds.gt_alpha(i), alpha64[:, :, 0].astype('float32'))
        assert ds.truth_u8(i).shape == (40, 48, 3) and ds.truth_u8(i).dtype == np.uint8
    # a subject pixel is alpha64 > 0 and both pixel classes occur inside the box on the frames of the epoch
    for i in ds.epoch_frames:
        w = ds.whole_frame(i, bg)
        subject = w['ray_alpha'][:, 0] > 0
        assert subject.any() and (~subject).any()
    b = list(WholeFrames(ds, bg))[1]
    assert b['rays'].shape[0] == 1 and b['img_width'] == 48 and b['img_height'] == 40


def test_a_distorted_and_cropped_dataset_opens_at_one_half(tmp_path):
    from occnerf_amd.dataset import PreparedDataset
    path = uc.make_tool_dataset(tmp_path / 'd')
    crop = [31, 26]
    full = PreparedDataset(path, device=None, volume_size=4, prepare_frames=True, crop_image_scale=crop)
    with pytest.raises(NotImplementedError, match='resize_img_scale'):
        PreparedDataset(path, device=None, volume_size=4, prepare_frames=True, crop_image_scale=crop, resize_img_scale=0.5,
                        images_prescaled=True)
    ds = PreparedDataset(path, device=None, volume_size=4, prepare_frames=True, crop_image_scale=crop, resize_img_scale=0.5,
                         resize_frames=True)
    assert (ds.src_height, ds.src_width) == (31, 26) and (ds.height, ds.width) == (16, 13)      # rint(15.5) = 16
    for i in range(len(ds)):
        assert np.array_equal(ds.images[i], full.images[i]) and np.array_equal(ds.alphas[i], full.alphas[i])
        K = ds.frames[i]['K']
        assert K[0, 2] == 31 / 2 * 0.5 and K[1, 2] == 26 / 2 * 0.5                            # the crop's point, then the scale
        assert np.array_equal(K[:2], full.frames[i]['K'][:2] * 0.5)
    w = ds.whole_frame(0, [0., 0., 0.])
    assert w['ray_mask'].shape == (16 * 13,) and w['target_rgbs'].shape == (int(w['ray_mask'].sum()), 3)


def test_from_cfg_reads_train_resize_frames(plain_path):
    from occnerf_amd import config
    from occnerf_amd.dataset import PreparedDataset
    cfg = config.default_cfg()
    assert cfg.train.resize_frames is False and cfg.resize_img_scale == 0.5
    cfg.mweight_volume.volume_size = 4
    with pytest.raises(NotImplementedError, match='resize_img_scale'):         # the default configuration: still refused
        PreparedDataset.from_cfg(cfg, plain_path, device=None)
    cfg.train.resize_frames = True
    ds = PreparedDataset.from_cfg(cfg, plain_path, device=None)
    assert ds.resizing and (ds.height, ds.width) == (40, 48)
    cfg.train.images_prescaled = True
    with pytest.raises(ValueError, match='images_prescaled'):
        PreparedDataset.from_cfg(cfg, plain_path, device=None)


# ---------------------------------------------------------------- 4. the entry points, without a GPU
def test_entry_points_are_exported_and_refuse_bad_arguments_without_a_gpu():
    import torch
    from occnerf_amd import _lib, ops
    lib = _lib.lib()
    for name in ('occnerf_resize_frame', 'occnerf_patch_batch_f64', 'occnerf_whole_frame_gather_f64'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    null = [None] * 8 + [None] * 4
    assert lib.occnerf_resize_frame(None, None, 4, 4, 2, 2, *null, None, None, None, None) != 0
    assert b'null' in lib.occnerf_last_error()
    assert lib.occnerf_patch_batch_f64(None, None, None, None, 4, 4, 1, 2, None, 0.8, None, *([None] * 12), None) != 0
    assert b'null' in lib.occnerf_last_error()
    assert lib.occnerf_whole_frame_gather_f64(None, None, None, None, 4, 4, None, None, 0, *([None] * 9), None) != 0
    assert b'null' in lib.occnerf_last_error()
    # the checks that need no device memory: every pointer is only tested against NULL before the sizes and tables are
    tables = resize.frame_tables(8, 8, 0.5)
    host = {k: np.ascontiguousarray(tables[k][0]) for k in ('x_lanczos', 'y_lanczos', 'x_bilinear', 'y_bilinear')}
    fake = np.zeros(16, np.float64).ctypes.data                # never dereferenced: the entry refuses before it launches

    def call(H=8, W=8, h=4, w=4, **replace):
        t = {**host, **replace}
        return lib.occnerf_resize_frame(fake, fake, H, W, h, w, *([fake] * 8), t['x_lanczos'].ctypes.data,
                                        t['y_lanczos'].ctypes.data, t['x_bilinear'].ctypes.data, t['y_bilinear'].ctypes.data,
                                        np.zeros(3, np.float32).ctypes.data, fake, fake, None)
    assert call(H=1 << 14, W=1 << 14) != 0 and b'source size' in lib.occnerf_last_error()
    assert call(h=0) != 0 and b'destination size' in lib.occnerf_last_error()
    bad = host['x_lanczos'].copy()
    bad[3, 7] = 8
    assert call(x_lanczos=bad) != 0 and b'x_off_lanczos[31] = 8 reads outside' in lib.occnerf_last_error()
    bad = host['y_bilinear'].copy()
    bad[0, 0] = -1
    assert call(y_bilinear=bad) != 0 and b'y_off_bilinear[0] = -1 reads outside' in lib.occnerf_last_error()
    bad = host['y_lanczos'][::-1].copy()
    assert call(y_lanczos=bad) != 0 and b'do not ascend' in lib.occnerf_last_error()
    # the torch-facing wrappers refuse host tensors: there is no CPU path behind them
    mask = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='not a GPU'):
        ops.upload_resize_tables(tables, 'cpu')
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.resize_frame(None, mask, {'device': {}, 'size': (4, 4), 'src_size': (8, 8)})
    f64 = torch.zeros(4, 4, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.patch_batch_f64(f64, f64, torch.zeros(16, 8), torch.zeros(16, dtype=torch.uint8), 1, 2, np.zeros((1, 2)), 0.8,
                            [0, 0, 0], out=ops.alloc_patch_batch(1, 2, 4, 'cpu'))
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.whole_frame_f64(f64, f64, torch.zeros(16, 8), torch.zeros(16, dtype=torch.uint8), [0, 0, 0])
