"""The frame-ahead scheme of the dataset loaders (dataset.PatchBatchLoader, WholeFrames.device_frames and
views.ViewFrames.device_frames): item t+1 is built on a side stream into the other of two buffer sets
while the consumer works on item t, and what the host must know of it (a row count) comes back through pinned memory behind
an event.  The consumer waits on that event only and makes its stream wait for it: its stream is never synchronised."""
import torch


def cuda_device(device, who, instead):
    """`device` as a torch.device with its index filled in; anything else is refused in `who`'s name with the hint `instead`."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError(f'{who}: {dev} is not a GPU; {instead}')
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


class FrameAhead:
    """Buffers, streams and events; nothing of what is built.  make_buffers() -> a dict of device tensors, called once per
    buffer set: two sets with prefetch, one without.  Each set gets `host_words` pinned int32 words and an event.

        ticket = ahead.start(item, enqueue)     # enqueue(bufs, item) launches the build of `item` into the next set in turn
                                                # and returns the small device tensor(s) to copy into the host words
        bufs, host, item = ahead.take(ticket)   # waits for it; `host`: the pinned words, valid until the set's next start

    The one rule: with two sets, the set `start` hands to item t+1 was last read by the work the consumer enqueued for item
    t-1.  `start` makes the side stream wait for everything on the consumer's current stream AT THE MOMENT OF THE CALL, so
    it must come after that work is enqueued -- and before the consumer enqueues its work on item t, or the build would
    queue behind that work and nothing would overlap.  The loaders therefore call start(t+1) right after they have enqueued
    their own reads of item t's set and before they hand item t out; what the consumer keeps of a set past the call after
    the next, it must copy.  With one set (prefetch False) everything runs in line on the current stream."""

    def __init__(self, device, make_buffers, host_words=1, prefetch=True):
        self.device = cuda_device(device, 'FrameAhead', 'its buffer sets are device memory')
        self._sets = [{'bufs': make_buffers(), 'host': torch.empty(int(host_words), dtype=torch.int32).pin_memory(),
                       'event': torch.cuda.Event()} for _ in range(2 if prefetch else 1)]
        self._side = torch.cuda.Stream(device=self.device) if prefetch else None
        self._turn = 0

    def start(self, item, enqueue):
        s = self._sets[self._turn % len(self._sets)]
        self._turn += 1
        if self._side is not None:
            self._side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self._side):                # None: stay on the current stream
            words = enqueue(s['bufs'], item)
            at = 0
            for w in (words,) if torch.is_tensor(words) else words:
                s['host'][at:at + w.numel()].copy_(w, non_blocking=True)
                at += w.numel()
            s['event'].record()
        return s, item

    def take(self, ticket):
        s, item = ticket
        s['event'].synchronize()
        torch.cuda.current_stream(self.device).wait_event(s['event'])
        return s['bufs'], s['host'], item
