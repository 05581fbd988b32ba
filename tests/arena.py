"""Guarded memory for the workspace contract (tests/test_gpu_workspace_contract.py): a plain helper, no pytest hooks.

  Arena(need, fill)      one uint8 tensor [front guard | region of exactly `need` bytes | back guard]; the region's base is
                         256-byte aligned, each guard is GUARD bytes of GUARD_BYTE.  ptr / bytes go to the entry; damage()
                         reports the first and last guard byte that no longer holds GUARD_BYTE, as offsets RELATIVE TO THE REGION
                         (negative: in front of it; >= need: behind it), or None
  guarded(shape, dtype, fill_byte)
                         an output tensor with the same two guards round its exact extent, every byte of it pre-filled with
                         fill_byte: elements a call must not write keep it (Guarded.untouched)
  frozen(*tensors)       context manager: clones the read-only inputs and asserts on exit that each is bit-identical

0x5C differs from every fill of a workspace region (FILLS) and from the 0xA5 other tests fill with.  Everything works on CPU
tensors as well (tests/test_workspace_contract_host.py checks the module there)."""
import contextlib

import torch

GUARD = 64 * 1024
GUARD_BYTE = 0x5C
ALIGN = 256
FILLS = {"zeros": 0x00, "ones": 0xFF, "a5": 0xA5}            # `leftover` is a tensor of bytes, not a byte
OUT_FILL = 0xA5


def _damage(raw, start, extent):
    """first and last byte of raw outside [start, start + extent) that is not GUARD_BYTE, relative to start; None if none"""
    bad = torch.cat([raw[:start], raw[start + extent:]]) != GUARD_BYTE
    if not bool(bad.any()):
        return None
    at = torch.nonzero(bad).reshape(-1)
    rel = lambda i: i - start if i < start else i + extent - start
    return rel(int(at[0])), rel(int(at[-1]))


class _Block:
    def __init__(self, extent, device):
        self.extent = int(extent)
        self.raw = torch.full((2 * GUARD + self.extent + ALIGN,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.start = GUARD + (-(self.raw.data_ptr() + GUARD)) % ALIGN
        assert (self.raw.data_ptr() + self.start) % ALIGN == 0 and self.start + self.extent + GUARD <= self.raw.numel()
        self.region = self.raw[self.start:self.start + self.extent]

    def damage(self):
        return _damage(self.raw, self.start, self.extent)


class Arena(_Block):
    """a workspace of exactly `need` bytes between two guards.  fill: a name of FILLS, or a uint8 tensor (a `leftover`) that is
    copied into the front of the region and repeated if the region is longer"""

    def __init__(self, need, fill="zeros", device="cuda:0"):
        super().__init__(need, device)
        self.set(fill)

    def set(self, fill):
        if isinstance(fill, str):
            self.region.fill_(FILLS[fill])
        elif self.extent:
            src = fill.reshape(-1).to(self.region.device)
            assert src.dtype == torch.uint8 and src.numel() > 0
            reps = -(-self.extent // src.numel())
            self.region.copy_(src.repeat(reps)[:self.extent])
        self.before = self.region.clone()

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.start

    @property
    def bytes(self):
        return self.extent

    def untouched(self):
        """the region holds what set() put there"""
        return torch.equal(self.region, self.before)


class Guarded(_Block):
    """an output of `shape` and `dtype` between two guards, pre-filled with fill_byte; .t is the tensor handed to the entry"""

    def __init__(self, shape, dtype, fill_byte=OUT_FILL, device="cuda:0"):
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        size = torch.empty(0, dtype=dtype).element_size()
        super().__init__(numel * size, device)
        self.fill_byte = fill_byte
        self.region.fill_(fill_byte)
        self.t = self.region.view(dtype).reshape(shape)

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.start

    def bits(self):
        """the extent as bytes, cloned: what two runs are compared by"""
        return self.region.clone()

    def untouched(self, where=None):
        """every byte (where None) or every element of the boolean mask `where` (the tensor's shape) still holds the pre-fill"""
        if where is None:
            return bool((self.region == self.fill_byte).all())
        size = self.t.element_size()
        by = self.region.reshape(-1, size)[where.reshape(-1).to(self.region.device)]
        return bool((by == self.fill_byte).all())


def guarded(shape, dtype, fill_byte=OUT_FILL, device="cuda:0"):
    return Guarded(shape, dtype, fill_byte, device)


def _int_view(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


@contextlib.contextmanager
def frozen(*tensors):
    """the tensors (None entries are skipped) are bit-identical when the block ends"""
    kept = [(i, t, _int_view(t).clone()) for i, t in enumerate(tensors) if t is not None]
    yield
    for i, t, was in kept:
        assert torch.equal(_int_view(t), was), f"read-only input {i} of shape {tuple(t.shape)} was written"
