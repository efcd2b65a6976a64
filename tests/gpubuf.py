"""Guarded device buffers for the GPU tests that call the C ABI directly (tests/test_solver_fp64.py,
tests/test_exact_fp64.py): every array has exactly the size the header states, sits at a chosen offset inside its
allocation and is followed by sentinel elements, so a store past the end or into an input shows."""
import ctypes

import torch

SENTINEL = 12345.6796875
GUARD = 64


class Buf:
    """A device array of exactly `count` elements, `offset` elements into an allocation and followed by GUARD sentinel
    elements; remembers what it was filled with."""

    def __init__(self, data=None, count=None, offset=0, dtype=torch.float32, fill=None):
        if data is not None:
            data = torch.as_tensor(data).to(dtype).reshape(-1)
            count = data.numel()
        self.count, self.offset, self.dtype = count, offset, dtype
        self.sent = SENTINEL if dtype.is_floating_point else 0x5A5A5A5A if dtype in (torch.int32, torch.int64) else 0x5A
        self.raw = torch.full((offset + count + GUARD,), self.sent, dtype=dtype, device="cuda")
        self.view = self.raw[offset: offset + count]
        if data is not None:
            self.view.copy_(data)
        elif fill is not None:
            self.view.fill_(fill)
        self.before = self.view.cpu().clone()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.raw.data_ptr() + self.offset * self.raw.element_size())

    def cpu(self, *shape):
        out = self.view.cpu()
        return out.reshape(*shape) if shape else out

    def np(self, *shape):
        return self.cpu(*shape).numpy()

    def guards_intact(self):
        r = self.raw.cpu()
        return bool((r[: self.offset] == self.sent).all() and (r[self.offset + self.count:] == self.sent).all())

    def unchanged(self):
        return _bits_equal(self.view.cpu(), self.before)


def _bits_equal(a, b):
    view = {4: torch.int32, 2: torch.int16, 8: torch.int64, 1: torch.uint8}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def check_buffers(inputs=(), outputs=()):
    for b in inputs:
        assert b.unchanged(), "an input buffer was written"
        assert b.guards_intact(), "a store past the end of an input buffer"
    for b in outputs:
        assert b.guards_intact(), "a store outside an output or work buffer"
