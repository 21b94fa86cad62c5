"""The trainer's progress dump (the reference's trainer.py:293-392 without the matplotlib scatter): every frame of the
`progress` loader rendered in eval mode, the rendered and truth panels tiled four to a row into prog_NNNNNN.jpg, and -- what
the reference does not have -- one line of validation metrics per dump in progress.jsonl.

The reference copies every frame's colours to the host, scatters, quantises and tiles them in numpy.  Here csrc/progress.hip
writes both panels of a frame straight into the frame's tile of ONE device mosaic and counts the rendered bytes that are off
the background (`progress_tile`); the frames are rendered through the existing path (sequence.frames_to_device, one frame of
lag), the stream is not synchronised per frame, and the mosaic and the counts cross PCIe once, after the last frame.  The
JPEG is encoded on a writer thread (image.ImageWriter's pattern) while training goes on.

The early exit (trainer.py:375-378, iter <= 5000): the reference stops at the first frame whose render is all background and
tiles the panels it has.  That image is a crop of the full mosaic, so every frame is rendered here regardless (nothing waits
for a count in the loop) and the crop is taken on the host: the top k // 4 tile rows for k >= 4 visited frames, the first k
tiles of row 0 below that."""
import json
import os
import threading
import time

import numpy as np
import torch

from . import _lib, ops
from .config import get_cfg

PER_ROW = 4                   # image_util.py:38 imgs_per_row
EMPTY_CHECK_UNTIL = 5000      # trainer.py:375
DUMP_ITERS = (20, 100, 300, 1000, 2500)       # trainer.py:269


def dump_due(it, dump_interval):
    """trainer.py:269-270; `progress.dump_interval 0` switches the dumps off."""
    dump_interval = int(dump_interval)
    return dump_interval > 0 and (it in DUMP_ITERS or it % dump_interval == 0)


def mosaic_shape(n):
    """(tile rows, tile columns) image_util.tile_images keeps of n panels: min(n, 4) to a row, full rows only."""
    cols = min(int(n), PER_ROW)
    return (int(n) // cols if cols else 0), cols


def crop_for_first_empty(mosaic, k, n, height, width):
    """The reference's image when its loop stops after k of n frames, as a view of the full mosaic [rows*H, cols*2W, 3]."""
    cols = mosaic_shape(n)[1]
    if k >= cols:
        return mosaic[:(k // cols) * height]
    return mosaic[:height, :k * 2 * width]


def record_line(it, wall_s, means, is_empty):
    """One line of progress.jsonl.  A mean that is not finite (psnr_vis of a frame without a visible pixel) is written as
    null: strict JSON has no NaN."""
    record = dict({'iter': int(it), 'wall_s': round(float(wall_s), 3)},
                  **{k: (float(v) if np.isfinite(v) else None) for k, v in means.items()}, is_empty=bool(is_empty))
    return json.dumps(record, allow_nan=False)


def progress_tile(rgb, ray_index, height, width, bg01, bg255, truth_u8, mosaic, tile_x, tile_y, partial, off_bg):
    """One frame into its tile (include/occnerf_hip.h occnerf_progress_tile).  rgb [R,3] float32, ray_index [R] int64
    ascending, truth_u8 [H,W,3] uint8, mosaic [rows, cols, 3] uint8, partial int32 [>= progress_tile_blocks(H, W)] and off_bg
    (an int32 tensor of one element, e.g. counts[i:i + 1]) on one GPU; bg01 = float32(cfg.bgcolor / 255), bg255 = cfg.bgcolor."""
    dev = mosaic.device
    R = int(ray_index.numel())
    if tuple(truth_u8.shape) != (height, width, 3) or mosaic.dim() != 3 or mosaic.shape[2] != 3:
        raise ValueError(f'progress_tile: truth_u8 must be [{height},{width},3] and the mosaic [rows,cols,3], got '
                         f'{tuple(truth_u8.shape)} and {tuple(mosaic.shape)}')
    if R and tuple(rgb.shape) != (R, 3):
        raise ValueError(f'progress_tile: rgb must be [{R},3], got {tuple(rgb.shape)}')
    blocks = int(_lib.lib().occnerf_progress_tile_blocks(int(height), int(width)))
    if blocks < 0 or partial.numel() < blocks or off_bg.numel() != 1:
        raise ValueError(f'progress_tile: {height} x {width} needs {blocks} int32 of workspace (got {partial.numel()}) and one '
                         'int32 for the count')
    _b01, p01 = ops._host_f32(bg01, 3)
    b255 = np.ascontiguousarray(np.asarray(bg255, dtype=np.float64).ravel())
    assert b255.size == 3
    with ops._guard_dev(dev):
        rc = _lib.lib().occnerf_progress_tile(
            ops._chk(rgb.contiguous(), torch.float32, 'rgb') if R else None,
            ops._chk(ray_index, torch.int64, 'ray_index') if R else None, R, int(height), int(width), p01,
            b255.ctypes.data, ops._chk(truth_u8, torch.uint8, 'truth_u8'), ops._chk(mosaic, torch.uint8, 'mosaic'),
            int(mosaic.shape[0]), int(mosaic.shape[1]), int(tile_x), int(tile_y), ops._chk(partial, torch.int32, 'partial'),
            ops._chk(off_bg, torch.int32, 'off_bg'), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, 'progress_tile')


class ProgressDump:
    """ProgressDump(loader, logdir).run(net, renderer_or_net, it) -> {'is_empty', 'mosaic', 'metrics', 'path'}.

    loader: create_dataloader('progress') on a prepared dataset (dataset.WholeFrames: the truth panel is the frame's
    truth_u8).  renderer_or_net: a parallel.ShardedRenderer (submit / finish) or the network itself.  run() returns once the
    mosaic and the counts are on the host; the JPEG is written behind it (close() waits for the writer).  'mosaic' is the
    image that is being written, a view of the pinned staging buffer: valid until the next run()."""

    def __init__(self, loader, logdir, device=None, bgcolor=None):
        if not hasattr(loader, 'device_frames'):
            raise TypeError('ProgressDump: the loader must build its frames on the device with a truth_u8 panel (a prepared '
                            "dataset's create_dataloader('progress')); the synthetic subject has no photographs")
        self.loader, self.logdir = loader, str(logdir)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        # sequence.frames_to_device builds the frames on the host in these two cases, and those carry no truth_u8 and no maps
        if self.device.type != 'cuda':
            raise ValueError(f'ProgressDump: the dump runs on a GPU (csrc/progress.hip, csrc/frame.hip), not on {self.device}')
        if not get_cfg().get('device_frames', True):
            raise ValueError('ProgressDump: `device_frames False` is configured; the dump needs the truth_u8 panel and the '
                             'metric maps of the frames built on the device (set progress.dump_interval 0 or device_frames True)')
        self.bgcolor = bgcolor
        self._bufs, self._thread, self._error = None, None, None
        self._t0 = time.time()

    def _buffers(self, n, H, W):
        key = (n, H, W)
        if self._bufs is None or self._bufs['key'] != key:
            rows, cols = mosaic_shape(n)
            all_rows = -(-n // cols)                         # frames of an incomplete last row get a tile that is not kept
            blocks = int(_lib.lib().occnerf_progress_tile_blocks(H, W))
            if blocks < 0:
                raise ValueError(f'ProgressDump: frames of {H} x {W} are not supported')
            self._bufs = {'key': key, 'rows': rows, 'cols': cols,
                          'mosaic': torch.empty(all_rows * H, cols * 2 * W, 3, device=self.device, dtype=torch.uint8),
                          'partial': torch.empty(blocks, device=self.device, dtype=torch.int32),
                          'counts': torch.empty(n, device=self.device, dtype=torch.int32),
                          'host_mosaic': torch.empty(rows * H, cols * 2 * W, 3, dtype=torch.uint8).pin_memory(),
                          'host_counts': torch.empty(n, dtype=torch.int32).pin_memory()}
        return self._bufs

    def _join(self):
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        if self._error is not None:
            err, self._error = self._error, None
            raise err

    def close(self):
        """Wait for the JPEG that is still being written."""
        self._join()

    def _encode(self, image, path):
        def work():
            try:
                from PIL import Image
                tmp = f'{path}.tmp{os.getpid()}'             # as the checkpoints: the final name holds a whole image or none
                try:
                    Image.fromarray(np.ascontiguousarray(image)).save(tmp, format='JPEG')
                    os.replace(tmp, path)
                finally:
                    if os.path.exists(tmp):
                        os.remove(tmp)
            except Exception as e:                           # surfaced by the next run() or close()
                self._error = e
        self._thread = threading.Thread(target=work, daemon=True)
        self._thread.start()

    def run(self, net, renderer_or_net, it):
        from .dataset import NETWORK_KEYS
        from .metrics import KEYS, frame_metrics_from_maps
        from .sequence import frames_to_device
        cfg = getattr(net, 'cfg', None) or get_cfg()
        bg255 = np.array(cfg.bgcolor if self.bgcolor is None else self.bgcolor, dtype=np.float64)
        bg01 = (bg255 / 255.).astype(np.float32)             # np.full(..., bgcolor / 255., dtype='float32')
        n = len(self.loader)
        sharded = hasattr(renderer_or_net, 'submit')
        was_training, perturb = net.training, cfg.perturb
        kept, bufs = [], None
        self._join()                                         # the pinned mosaic of the previous dump may still be encoding

        def deliver(pending, meta):
            out = renderer_or_net.finish(pending) if sharded else pending
            i, H, W = meta['idx'], meta['height'], meta['width']
            progress_tile(out['rgb'], meta['ray_index'], H, W, bg01, bg255, meta['truth_u8'], bufs['mosaic'],
                          i % bufs['cols'], i // bufs['cols'], bufs['partial'], bufs['counts'][i:i + 1])
            kept.append((out['rgb'], out['alpha'], meta))

        net.eval()                                           # trainer.py:293-295 progress_begin
        cfg.perturb = 0.
        try:
            with torch.no_grad():
                prev = None
                for data, key, meta in frames_to_device(self.loader, 'progress', self.device):
                    if bufs is None:
                        bufs = self._buffers(n, meta['height'], meta['width'])
                    if sharded:
                        cur = renderer_or_net.submit(data, iter_val=it, ray_order_key=key)
                    else:
                        cur = renderer_or_net(**{k: data[k] for k in NETWORK_KEYS}, iter_val=it)
                    if prev is not None:
                        deliver(*prev)
                    prev = (cur, meta)
                if prev is not None:
                    deliver(*prev)
                if bufs is None:
                    raise ValueError('ProgressDump: the progress loader has no frame')
                H, W = bufs['key'][1:]
                # the one transfer of the dump: the kept rows of the mosaic and the counts, behind every frame's launches
                bufs['host_mosaic'].copy_(bufs['mosaic'][:bufs['rows'] * H], non_blocking=True)
                bufs['host_counts'].copy_(bufs['counts'], non_blocking=True)
                done = torch.cuda.Event()
                done.record(torch.cuda.current_stream(self.device))
                # the validation record: the maps are in `meta` already; this is where the host first waits for the device
                per_frame = [frame_metrics_from_maps(rgb, alpha, meta['ray_index'], meta, meta['width'], meta['height'],
                                                     bgcolor=bg255 / 255.) for rgb, alpha, meta in kept]
                done.synchronize()
        finally:
            net.train(was_training)                          # trainer.py:297-299 progress_end
            cfg.perturb = perturb
        counts = bufs['host_counts'].numpy()
        mosaic = bufs['host_mosaic'].numpy()
        empty = np.nonzero(counts == 0)[0] if it <= EMPTY_CHECK_UNTIL else []
        is_empty = len(empty) > 0
        image = crop_for_first_empty(mosaic, int(empty[0]) + 1, n, H, W) if is_empty else mosaic
        os.makedirs(self.logdir, exist_ok=True)
        path = os.path.join(self.logdir, f'prog_{it:06d}.jpg')
        self._encode(image, path)
        if is_empty:
            print('Produce empty images!')
        means = {k: float(np.mean([m[k] for m in per_frame])) for k in KEYS}
        with open(os.path.join(self.logdir, 'progress.jsonl'), 'a') as f:
            f.write(record_line(it, time.time() - self._t0, means, is_empty) + '\n')
        return {'is_empty': is_empty, 'mosaic': image, 'metrics': means, 'path': path, 'off_bg': counts.copy()}
