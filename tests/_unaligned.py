"""Helpers of the unaligned-view tests: device tensors whose base pointer is NOT what a fresh torch allocation gives
(256-byte aligned), with sentinel-filled guard elements around them."""
import torch

SENTINEL = 12345.678            # rounds to one float32 value; never produced by the cases of these tests
_GUARD = 4                      # guard elements before the view (a multiple of 4: keeps the 16-byte phase)


def misaligned(t: torch.Tensor, off: int) -> torch.Tensor:
    """A contiguous float32 tensor equal to `t` whose data_ptr() is `4 * off` bytes past a 16-byte boundary, cut out
    of a sentinel-filled buffer with at least one guard element on either side (`guards_intact`)."""
    assert t.dtype == torch.float32 and 0 <= off < 4
    n = t.numel()
    buf = torch.full((n + 2 * _GUARD + 4,), SENTINEL, dtype=torch.float32, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[_GUARD + off:_GUARD + off + n].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off, (v.data_ptr(), off)   # never silently aligned
    return v


def guards_intact(v: torch.Tensor) -> bool:
    """True when every element of the buffer of `misaligned(...)` outside the view still holds the sentinel."""
    base, s, n = v._base, v.storage_offset(), v.numel()
    assert base is not None and base.dim() == 1
    want = torch.tensor(SENTINEL, dtype=torch.float32, device=v.device)
    return bool((base[:s] == want).all()) and bool((base[s + n:] == want).all())
