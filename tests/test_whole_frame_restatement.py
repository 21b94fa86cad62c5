"""CPU: the host side of the whole-frame builder (csrc/frame.hip) -- the cases tests/test_h_whole_frame.py compares on the
GPU meet their coverage conditions on the host path, the two entry points are declared, exported and refuse null pointers
without a launch, and the loader's host path is what it was."""
import numpy as np
import pytest
import torch

from tests import whole_frame_cases as cases
from tests import whole_frame_restatement as wfr


@pytest.fixture(scope='module')
def paths(tmp_path_factory):
    return cases.make_datasets(tmp_path_factory.mktemp('whole_frame'))


@pytest.mark.parametrize('name', list(cases.CASES))
def test_every_case_meets_its_condition_on_the_host_path(name, paths):
    ds, frame = cases.open_case(name, paths)
    w = ds.whole_frame(frame, cases.BGCOLORS['white'])
    print('\n   ' + cases.check_condition(name, ds, frame, w))
    truth, gt_vis, gt_alpha = wfr.maps(w, ds.alphas[frame], cases.BGCOLORS['white'])
    H, W = ds.height, ds.width
    mask = w['ray_mask'].reshape(H, W)
    assert truth.shape == (H, W, 3) and truth.dtype == np.uint8 and (truth[~mask] == 255).all()
    assert gt_vis.dtype == gt_alpha.dtype == np.float32 and np.array_equal(gt_vis[mask], gt_alpha[mask])
    assert (gt_vis[~mask] == 0).all()
    if name == 'tiny':
        assert not np.array_equal(gt_vis, gt_alpha)


def test_entry_points_are_declared_exported_and_refuse_null_pointers():
    from occnerf_amd import _lib
    assert 'occnerf_whole_frame_count' in _lib.SIGNATURES and 'occnerf_whole_frame_gather' in _lib.SIGNATURES
    lib = _lib.lib()                                      # getattr of every declared symbol: AttributeError if one is missing
    assert lib.occnerf_abi_version() == 5 == _lib.ABI_VERSION
    rc = lib.occnerf_whole_frame_count(None, 8, 8, None, None)
    assert rc != 0 and b'null' in lib.occnerf_last_error() and b'whole_frame_count' in lib.occnerf_last_error()
    rc = lib.occnerf_whole_frame_gather(None, None, None, None, 8, 8, None, None, 0, *([None] * 9), None)
    assert rc != 0 and b'null' in lib.occnerf_last_error() and b'whole_frame_gather' in lib.occnerf_last_error()


def _plain(triple):
    data, key, meta = triple
    return ({k: np.asarray(v) for k, v in data.items()}, key,
            {k: (np.asarray(v) if torch.is_tensor(v) else v) for k, v in meta.items()})


def test_host_path_of_frames_to_device_is_unchanged(paths, monkeypatch):
    """On a host device, or with `device_frames False`, frames_to_device yields what it yielded before the loader had
    device_frames: every tensor of the host WholeFrames dict, the index list of the host mask, idx / width / height."""
    from occnerf_amd import config, sequence
    from occnerf_amd.dataset import PreparedDataset, WholeFrames
    loader = WholeFrames(PreparedDataset(paths['wide'], device=None, volume_size=4), [255., 255., 255.])
    assert callable(getattr(WholeFrames, 'device_frames', None))

    def refuse(*a, **k):
        raise AssertionError('device_frames was called on the host path')
    monkeypatch.setattr(loader, 'device_frames', refuse, raising=False)
    cfg = config.default_cfg()
    monkeypatch.setattr(sequence, 'get_cfg', lambda: cfg)
    got = [_plain(t) for t in sequence.frames_to_device(loader, 'movement', 'cpu')]
    cfg.device_frames = False                            # (on a GPU with the switch off: tests/test_h_whole_frame.py)
    off = [_plain(t) for t in sequence.frames_to_device(loader, 'movement', 'cpu')]
    for (d0, k0, m0), (d1, k1, m1) in zip(got, off):
        assert k0 == k1 and sorted(d0) == sorted(d1) and all(np.array_equal(d0[k], d1[k]) for k in d0)
    assert len(got) == len(loader) == 2
    for i, (data, key, meta) in enumerate(got):
        w = loader.dataset.whole_frame(i, [255., 255., 255.])
        tensors = {k for k, v in w.items() if not isinstance(v, str) and not np.isscalar(v)} - {'ray_mask'}
        assert set(data) == tensors
        for k in tensors:
            assert data[k].dtype == np.asarray(w[k]).dtype and np.array_equal(data[k], w[k]), k
        assert sorted(meta) == ['height', 'idx', 'ray_index', 'width']
        assert np.array_equal(meta['ray_index'], np.nonzero(w['ray_mask'])[0]) and meta['idx'] == i
        assert (meta['width'], meta['height']) == (96, 80) and key == ('movement', int(w['ray_mask'].sum()))
