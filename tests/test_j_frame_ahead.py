"""The frame-ahead helper alone (occnerf_amd/ahead.py), no dataset: the buffer-set reuse rule under a BUSY consumer.

The loaders' own GPU tests (test_g_train_batch.py, test_h_whole_frame.py, test_i_view_frames.py) synchronise the device
after every batch or frame, so there a buffer set is never rewritten while a consumer still reads it, whatever the helper
waits for.  Here the consumer's stream is kept tens of milliseconds behind the host."""
import pytest
import torch

DEV = 'cuda:0'
ITEMS, N = 6, 4096
# unrelated work per item on the consumer's stream: 4096^3 * 2 = 0.14 TFLOP per fp32 matmul, a millisecond or two each on an
# MI355X, so a chain of 16 keeps the stream busy for a few tens of milliseconds; 6 items, twice, stay well under a second
BUSY = 16


def _run(prefetch):
    from occnerf_amd.ahead import FrameAhead
    ahead = FrameAhead(DEV, lambda: {'buf': torch.empty(N, device=DEV, dtype=torch.int32)}, host_words=1, prefetch=prefetch)

    def enqueue(bufs, i):
        bufs['buf'].fill_(i)
        return torch.full((1,), i, device=DEV, dtype=torch.int32)

    a = torch.full((N, N), 1.0 / N, device=DEV)             # a @ a == a up to rounding: the chain neither grows nor vanishes
    b = a.clone()
    clones, words, items = [], [], []
    pending = ahead.start(0, enqueue)
    for t in range(ITEMS):
        bufs, host, item = ahead.take(pending)
        words.append(int(host[0]))
        items.append(item)
        for _ in range(BUSY):
            b = torch.matmul(a, b)
        clones.append(bufs['buf'].clone())                  # the consumer's read of the set, behind the busy work
        pending = ahead.start(t + 1, enqueue) if t + 1 < ITEMS else None      # where the loaders call it: after the read
    torch.cuda.synchronize()
    return [c.cpu() for c in clones], words, items


@pytest.mark.gpu
@pytest.mark.parametrize('prefetch', [True, False])
def test_a_buffer_set_is_not_rewritten_under_a_busy_consumer(prefetch):
    """6 items through FrameAhead; per item the consumer enqueues a few tens of milliseconds of matmuls, then a clone of
    the buffer, then calls start() for the next item, and synchronises only once, at the end.  Clone t must hold t
    everywhere and the host word of item t must have been t.

    A correctness check only, no time is asserted.  It cannot prove the absence of a race; it fails on the commonest
    mistake, a missing or misplaced wait_stream in start(): the fill of item t+1 then runs at once on the side stream
    while the clone of item t-1, which reads the same set, still waits behind the consumer's matmuls."""
    clones, words, items = _run(prefetch)
    assert items == list(range(ITEMS)) and words == list(range(ITEMS)), (items, words)
    for t, c in enumerate(clones):
        assert c.shape == (N,) and bool((c == t).all()), (t, c.unique().tolist())


def test_the_helper_refuses_a_device_that_is_no_gpu():
    from occnerf_amd.ahead import FrameAhead
    with pytest.raises(RuntimeError, match='not a GPU'):
        FrameAhead('cpu', dict)
