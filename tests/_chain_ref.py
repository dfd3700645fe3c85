"""Yardsticks of the forward-chain tests (tests/test_chain_ref_cpu.py, tests/test_gpu_chain_variants.py): float64
references with DERIVED elementwise bounds for all three activation types, CPU models of the kernels' arithmetic that the
CPU test uses to prove the yardsticks discriminate, sentinel-guarded strided tensors, and a raw C ABI launcher.  Importing
this file needs no GPU and no built library.

16-bit types: `linear_bound` of tests/_fp16_ref.py, unchanged, with u = 2^-8 (bfloat16) or 2^-11 (float16).

float32 (three bf16 planes per operand, csrc/chain.hip): every operand splits exactly into x = x1 + x2 + x3 with
|x2| <= 2^-8 |x| and |x3| <= 2^-16 |x|.  Of the nine partial products the kernel keeps six and drops x2y3, x3y2, x3y3:
at most (2^-24 + 2^-24 + 2^-32) |x||y| <= 2^-23 |x||y| per product, i.e. two units of 2^-24 for each of the chain's two
products.  Every kept bf16 x bf16 product is exact in fp32; what remains is the fp32 accumulation of n terms in an unknown
order and one rounding at the bias add.  With `n` and `allabs` those of `linear_ref`:

    |y - ref| <= 1.5 * (n + 5) * 2^-24 * allabs            (n accumulation terms + 1 bias add + 2 + 2 dropped terms)

(1.5 covers the second-order terms, as in _fp16_ref.py).  Nothing here is fitted to what a kernel returns."""
import ctypes as C

import torch

from _fp16_ref import ACC, U, bits, image_rows, linear_bound, linear_ref, report, rows_image  # noqa: F401  (re-exported)

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
PLANES = {torch.float32: 3, torch.bfloat16: 1, torch.float16: 1}
# the six partial products the three-plane kernels keep, in the order they are accumulated (smallest first); xi = plane i
# of the token operand, yj = plane j of the weight
KEPT_PAIRS = ("x3y1", "x1y3", "x2y2", "x2y1", "x1y2", "x1y1")


# ------------------------------------------------------------------ bounds
def linear_bound_f32(x, ws, bias):
    """(ref, bound) of the three-plane float32 mode, float64, elementwise.  ws = [W1 (R, K), W2 (N, R)] or [W]."""
    ref, _, allabs, n = linear_ref(x, ws, bias)
    return ref, 1.5 * (n + 5) * ACC * allabs


def bound_of(x, ws, bias, dtype):
    """(ref, bound) of the dtype's mode; `ws` are the values the kernel multiplies (rounded planes for 16-bit types)."""
    if dtype == torch.float32:
        return linear_bound_f32(x, ws, bias)
    return linear_bound(x, ws, bias, dtype)


def _chain64(x, ws, bias):
    y = x.double()
    for w in ws:
        y = y @ w.double().t()
    return y + bias.double() if bias is not None else y


def rms_ratio_vs_fp32(y, x, ws, bias):
    """rms(y - ref64) / rms(plain32 - ref64), plain32 = the same chain by float32 `@` on the CPU.  "As accurate as an
    fp32 GEMM" means parity: both are fp32 accumulations that differ in order only, so the tests assert ratio <= 2."""
    y, x = y.detach().cpu(), x.detach().cpu().float()
    ws = [w.detach().cpu().float() for w in ws]
    b = None if bias is None else bias.detach().cpu().float()
    ref = _chain64(x, ws, b)
    plain = x
    for w in ws:
        plain = plain @ w.t()
    if b is not None:
        plain = plain + b
    rms = lambda t: (t.double() - ref).pow(2).mean().sqrt().item()   # noqa: E731
    return rms(y) / rms(plain)


def same_bits(a, b):
    """Bitwise equality of two tensors of one dtype (float32, bfloat16 or float16), any strides."""
    it = torch.int32 if a.element_size() == 4 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ------------------------------------------------------------------ CPU models of the kernels' arithmetic
def split3(a):
    """a (float32) -> [a1, a2, a3], float32 tensors holding bfloat16 values with a1 + a2 + a3 == a exactly."""
    r, out = a.float(), []
    for _ in range(3):
        t = r.bfloat16().float()
        out.append(t)
        r = r - t
    assert bool((out[0].double() + out[1].double() + out[2].double() == a.double()).all())
    return out


def three_plane_emulation(x, w, drop=None):
    """x (T, K) @ w (N, K)^T as the three-plane kernels compute it: the six kept partial products of the exact bf16
    splits, each an exact-product fp32-accumulated matmul, added smallest first.  `drop`: one of KEPT_PAIRS to leave
    out (what a kernel with a missing entry in its pair table computes)."""
    assert drop is None or drop in KEPT_PAIRS
    xs, ws = split3(x), split3(w)
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32)
    for name in KEPT_PAIRS:
        if name != drop:
            acc = acc + xs[int(name[1]) - 1] @ ws[int(name[3]) - 1].t()
    return acc


def three_plane_chain(x, ws, bias, drop=None):
    y = x.float()
    for w in ws:
        y = three_plane_emulation(y, w.float(), drop)
    return y + bias.float() if bias is not None else y


def half_chain_model(x, ws, bias, dtype, fault=None):
    """The one-plane kernels on the CPU: operands rounded to `dtype`, fp32 accumulation, every intermediate rounded to
    `dtype`, the output rounded to `dtype`.  Returns (y, rounded x, rounded ws): the bound is taken on the rounded
    operands.  Faults:
      "mid_twice"   the intermediate is rounded twice.  A second rounding at the same width is the identity, so the fault
                    is a conversion through a narrower format first (`coarse_round`, four significand bits fewer), then
                    the rounding of its type.  A worst-case bound of a rank-R sum is loose by about sqrt(R) against
                    rounding errors of random sign: three bits fewer stay inside it at R = 256.
      "skip_kstep"  product 1 leaves out one k-step, the 32 columns [32, 64)."""
    assert fault in (None, "mid_twice", "skip_kstep")
    xq = x.to(dtype)
    wq = [w.to(dtype) for w in ws]
    h = xq.float()
    for i, w in enumerate(wq):
        wf = w.float()
        if fault == "skip_kstep" and i == 0:
            keep = torch.ones(wf.shape[1], dtype=torch.bool)
            keep[32:64] = False
            h = h[:, keep] @ wf[:, keep].t()
        else:
            h = h @ wf.t()
        if i + 1 < len(wq):
            if fault == "mid_twice":
                h = coarse_round(h, dtype)
            h = h.to(dtype).float()
    if bias is not None:
        h = h + bias.float()
    return h.to(dtype), xq, wq


def coarse_round(h, dtype, fewer=4):
    """fp32 values rounded (to nearest, ties away) to a significand `fewer` bits shorter than `dtype`'s: 4 of bfloat16's
    8 bits, 7 of float16's 11."""
    shift = 24 - ({torch.bfloat16: 8, torch.float16: 11}[dtype] - fewer)
    i = h.float().contiguous().view(torch.int32)
    return ((i + (1 << (shift - 1))) & ~((1 << shift) - 1)).view(torch.float32)


# ------------------------------------------------------------------ guarded operands
# exact in float32, bfloat16 (8 significant bits) and float16 (below 65504); the cases' outputs are O(1) sums
SENTINEL = 24576.0
_GUARD = 64                      # guard elements before and after (a multiple of 8: keeps the 16-byte phase of both sizes)


def guarded(shape, dtype, ld=None, off=0, device="cuda"):
    """A sentinel-filled (rows, cols) tensor of row stride `ld` (default cols), or -- any other rank -- a contiguous
    tensor, whose first element lies `off` elements past a 16-byte boundary, cut out of a sentinel-filled flat buffer:
    guard elements before it, after it and in the `ld - cols` gap behind every row (`guards_intact`)."""
    esz = torch.empty((), dtype=dtype).element_size()
    assert 0 <= off < 16 // esz
    if len(shape) == 2:
        rows, cols = shape
        ld = cols if ld is None else ld
        assert ld >= cols
        span = (rows - 1) * ld + cols if rows else 0
    else:
        assert ld is None
        span = 1
        for s in shape:
            span *= s
    buf = torch.full((_GUARD + off + span + _GUARD,), SENTINEL, dtype=dtype, device=device)
    assert buf.data_ptr() % 16 == 0
    start = _GUARD + off
    if len(shape) == 2:
        v = buf.as_strided((rows, cols), (ld, 1), start)
    else:
        v = buf[start:start + span].view(shape)
    assert v.data_ptr() % 16 == (off * esz) % 16, (v.data_ptr(), off)          # never silently aligned
    return v


def guards_intact(v):
    """True when every element of the buffer of `guarded(...)` outside the view still holds the sentinel."""
    base = v._base
    assert base is not None and base.dim() == 1
    mask = torch.ones(base.numel(), dtype=torch.bool, device=base.device)
    if v.dim() == 2:
        rows, cols = v.shape
        idx = v.storage_offset() + (torch.arange(rows, device=base.device) * v.stride(0)).view(-1, 1) \
            + torch.arange(cols, device=base.device).view(1, -1)
        mask[idx.reshape(-1)] = False
    else:
        mask[v.storage_offset():v.storage_offset() + v.numel()] = False
    return bool((base[mask] == SENTINEL).all())


def untouched(v):
    """True when the view itself still holds nothing but the sentinel (a refused launch wrote nothing)."""
    return bool((v == SENTINEL).all())


# ------------------------------------------------------------------ raw C ABI launch
def launch_desc(entry, X, Y, win, wout, bias, T, kin, r, nout, ldx=0, ldy=0, x_hw=0, y_hw=0, tile_tokens=0, dtype=None):
    """Fills a `_cabi.ChainDesc` from explicit pointers (tensors or integers) and leading dimensions, calls `entry` on
    the current stream and returns its status code.  `win` / `wout` are plane tensors of `ops.weight_planes`; `dtype`
    defaults to the C ABI code of X's dtype."""
    from tadmm import _cabi, ops
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())   # noqa: E731
    d = _cabi.ChainDesc()
    d.X, d.Y, d.Win, d.Wout, d.bias = ptr(X), ptr(Y), ptr(win), ptr(wout), ptr(bias)
    d.T, d.Kin, d.R, d.Nout = T, kin, r, nout
    d.ldx, d.ldy = ldx, ldy
    d.win_plane = win[0].numel()
    d.wout_plane = 0 if wout is None else wout[0].numel()
    d.x_hw, d.y_hw, d.tile_tokens = x_hw, y_hw, tile_tokens
    if dtype is None:
        dtype = {torch.float32: _cabi.CHAIN_F32, torch.bfloat16: _cabi.CHAIN_BF16, torch.float16: _cabi.CHAIN_F16}[X.dtype]
    d.dtype = dtype
    dev = torch.cuda.current_device()
    h = ops.Handle.get(dev)
    return getattr(h.lib, entry)(h.ptr, C.byref(d), torch.cuda.current_stream().cuda_stream)
