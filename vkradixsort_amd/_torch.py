"""What the torch entry points (sort_rows, topk, sort, unique) share: contexts, row bounds, Buffers over tensors and int64 positions."""
from contextlib import contextmanager

from . import engine

_contexts: dict = {}


def context_for(device):
    """One context per (device, torch stream), borrowing that stream."""
    import torch

    stream = torch.cuda.current_stream(device)
    key = (device.index, stream.cuda_stream)
    if key not in _contexts:
        ctx = engine.GPUContext(device.index, stream=stream.cuda_stream)
        ctx.init()
        _contexts[key] = ctx
    return _contexts[key]


def row_offsets(rows: int, length: int, device):
    """The rows + 1 bounds i * length of rows of `length` elements, as uint32 bit patterns in an int32 tensor."""
    import torch

    bounds = torch.arange(rows + 1, dtype=torch.int64, device=device) * length
    return ((bounds + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)


def aligned(t):
    """t, or a copy of it when its memory starts off a 4-byte boundary (vrs_buffer_wrap takes no other): a contiguous view of a 1- or
    2-byte dtype that begins 1 to 3 bytes into its allocation, x[1:] of an int8 tensor."""
    return t.clone() if t.data_ptr() % 4 else t


@contextmanager
def buffers(ctx, *tensors):
    """Buffers over the tensors' device memory (numel * element_size bytes each): yields their handles in order, None for a tensor that
    is None or empty, and releases the Buffers on exit."""
    S = engine.Buffer.BufferSettings
    bufs = [None if t is None or t.numel() == 0 else engine.Buffer(ctx, S(t.numel() * t.element_size()), device_ptr=t.data_ptr())
            for t in tensors]
    try:
        yield [b.handle if b is not None else None for b in bufs]
    finally:
        for b in bufs:
            if b is not None:
                b.release()


def positions_to_int64(t, limit: int):
    """uint32 positions held in an int32 tensor, as int64.  An int32 view of them goes negative from 2^31 on, so they are masked when
    `limit` (what bounds them) is above 2^31; below it the mask would only cost a launch."""
    w = t.long()
    return w & 0xFFFFFFFF if limit > 1 << 31 else w
