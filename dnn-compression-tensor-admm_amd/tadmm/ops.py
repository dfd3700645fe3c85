"""Torch-facing wrappers over the C ABI: device memory, streams and pointer plumbing only.

Nothing here computes; every function hands raw device pointers of torch tensors
to libtadmm_hip.so on the current HIP stream.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import struct
import weakref
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _cabi
from ._cabi import (FLAG_SKIP_ROTATIONS, KIND_SVD, KIND_TT_CONV, KIND_TT_LINEAR, KIND_TUCKER2, GemmDesc, Handle,
                    LayerDesc, StiefelDesc, TadmmError, make_layer_desc)


def _handle(device) -> Handle:
    """The library handle of a torch device; a device without an index is the current one."""
    return Handle.get(device.index if device.index is not None else torch.cuda.current_device())


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _operand(t, who: str, what: str, dtypes=None, shape=None, layout: Optional[str] = "raise"):
    """The one check of a device operand; returns the tensor to hand to the library.  `who` (the entry; may be empty)
    and `what` (the operand) word the message.  `t` must be a tensor on a HIP device, of one of `dtypes` and exactly of
    `shape` (each checked when given).  `layout`: a non-contiguous tensor is an error ("raise"), is replaced by
    `.contiguous()` ("copy"), or has a layout rule of its own at the call site (None)."""
    name = f"{who}: {what}" if who else what
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise TadmmError(-1, f"{name} must live on a HIP device (got {where}); there is no CPU path")
    if dtypes is not None and t.dtype not in dtypes:
        want = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise TadmmError(-1, f"{name} must be {want} (got {t.dtype})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise TadmmError(-1, f"{name} must be {tuple(shape)} (got {tuple(t.shape)})")
    if layout is not None and not t.is_contiguous():
        if layout != "copy":
            raise TadmmError(-1, f"{name} must be contiguous")
        t = t.contiguous()
    return t


def _output(out, shape, dtype, device, name: str, fresh=torch.empty, strided_rows: bool = False):
    """The caller's output tensor where given, else a `fresh` one: `dtype`, `device` and exactly `shape`, contiguous --
    or, with `strided_rows`, any row stride under a unit column stride."""
    if out is None:
        return fresh(shape, dtype=dtype, device=device)
    ok = isinstance(out, torch.Tensor) and out.dtype == dtype and out.device == device and tuple(out.shape) == tuple(shape)
    if ok:
        ok = (shape[-1] <= 1 or out.stride(-1) == 1) if strided_rows else out.is_contiguous()
    if not ok:
        how = "with unit column stride" if strided_rows else "contiguous"
        raise TadmmError(-1, f"{name} must be a {dtype} {tuple(shape)} tensor on {device}, {how}")
    return out


def _scratch(nbytes: int, device) -> torch.Tensor:
    """The uint8 device buffer of a scratch size the library reported."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


class _LayerPlan:
    """What the grouped projections share: W / U / Z of every layer validated and captured by pointer, the workspace
    the library sizes, the per-layer ||W-Z||^2 buffer, run / enable_timing / close, and the teardown of the native plan
    when the object goes away.  A subclass names the prefix of its C entries (`<prefix>workspace_bytes`, `create`,
    `run`, `enable_timing`, `destroy`), builds the descriptor of a layer, and calls `_create` once it has its own buffers."""
    _PREFIX = ""
    _plan = None
    _fin = None

    def __init__(self, layers: Sequence[dict], make_desc):
        if not layers:
            raise ValueError("empty plan")
        dev = layers[0]["W"].device
        self.device = dev
        n = len(layers)
        self.n = n
        self._descs = (LayerDesc * n)()
        self._keep = []
        self._ptrs = tuple((C.c_void_p * n)() for _ in "WUZ")
        for i, L in enumerate(layers):
            for key in ("W", "U", "Z"):
                _operand(L[key], "", key, (torch.float32,))
                if L[key].shape != L["W"].shape:
                    raise TadmmError(-1, f"{key} shape differs from W")
            self._descs[i] = make_desc(L)
            for p, key in zip(self._ptrs, "WUZ"):
                p[i] = L[key].data_ptr()
            self._keep.append((L["W"], L["U"], L["Z"]))
        self.h = _handle(dev)
        size = C.c_size_t()
        self.h.check(self._entry("workspace_bytes")(self.h.ptr, n, self._descs, C.byref(size)))
        self.workspace_bytes = int(size.value)
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)
        self.resid_sq = torch.zeros(n, dtype=torch.float64, device=dev)

    def _entry(self, name: str):
        return getattr(self.h.lib, self._PREFIX + name)

    def _create(self, *extra):
        """The native plan over the captured pointers; `extra`: the subclass's own pointer arrays."""
        plan = C.c_void_p()
        self.h.check(self._entry("create")(self.h.ptr, self.n, self._descs, *self._ptrs, *extra, self.workspace.data_ptr(),
                                         self.workspace_bytes, C.byref(plan)))
        self._plan = plan
        self._fin = weakref.finalize(self, self._entry("destroy"), plan)

    def run(self, update_u: bool = True, use_u: bool = True) -> torch.Tensor:
        """One projection; returns the device tensor of per-layer ||W-Z||^2 (float64)."""
        self.h.check(self._entry("run")(self._plan, int(update_u), int(use_u), self.resid_sq.data_ptr(),
                                      _stream(self.device)))
        return self.resid_sq

    def enable_timing(self, on: bool = True):
        self.h.check(self._entry("enable_timing")(self._plan, int(on)))

    def close(self):
        """Destroys the native plan now instead of with the object.  Idempotent, and a no-op on an object whose
        constructor raised before the plan existed."""
        if self._fin is not None:
            self._fin()
        self._plan = None


class ProjectionPlan(_LayerPlan):
    """Grouped TT/SVD projection of a set of layers (ADMM.update, admm.py:42-78).

    layers: sequence of dicts with keys
        kind       : KIND_TT_CONV | KIND_TT_LINEAR | KIND_SVD
        W, U, Z    : float32 device tensors of identical shape (captured by pointer)
        tt_shapes  : list[int]   (TT kinds)
        ranks      : list[int] (TT) | int / [int] (SVD)
    """

    _PREFIX = "tadmm_plan_"

    def __init__(self, layers: Sequence[dict], want_cores: bool = False, skip_rotations: bool = True):
        flags = 0 if want_cores or not skip_rotations else FLAG_SKIP_ROTATIONS
        super().__init__(layers, lambda L: make_layer_desc(L["kind"], list(L["W"].shape), L.get("tt_shapes"), L["ranks"],
                                                           flags))
        n, dev = self.n, self.device
        Cp = (C.c_void_p * n)()
        self.cores: List[Optional[torch.Tensor]] = [None] * n
        self._core_shapes = []
        # clamped ranks are a pure function of the shapes: compute them to size the core buffers
        self.ranks = []
        for i, L in enumerate(layers):
            d = self._descs[i]
            if L["kind"] == KIND_SVD:
                o, k = int(L["W"].shape[0]), int(L["W"].shape[1])
                r = min(int(d.ranks[0]), o, k)
                shapes, ranks = [o, k], [1, r, 1]
            else:
                shapes = [int(d.tt_shapes[j]) for j in range(d.d)]
                ranks = _cabi.clamp_ranks(shapes, [int(d.ranks[j]) for j in range(d.d + 1)])
            self.ranks.append(ranks)
            self._core_shapes.append([(ranks[j], shapes[j], ranks[j + 1]) for j in range(len(shapes))])
            if want_cores:
                tot = sum(a * b * c for a, b, c in self._core_shapes[i])
                self.cores[i] = torch.empty(tot, dtype=torch.float32, device=dev)
                Cp[i] = self.cores[i].data_ptr()
            else:
                Cp[i] = None
        self._create(Cp)

    def set_jacobi(self, tol=0.0, inner_sweeps=0, max_sweeps=0):
        """Jacobi tunables (<= 0 keeps a value).  `inner_sweeps` is ignored: a 16x16 sub-problem gets one cyclic sweep."""
        self.h.check(self.h.lib.tadmm_plan_set_jacobi(self._plan, float(tol), int(inner_sweeps), int(max_sweeps)))

    def last_timing(self):
        out = (C.c_double * 8)()
        self.h.check(self.h.lib.tadmm_plan_last_timing(self._plan, out))
        keys = ["unfold_ms", "gram_ms", "eig_ms", "project_ms", "reconstruct_ms", "fold_update_ms", "jacobi_sweeps"]
        return {k: float(out[i]) for i, k in enumerate(keys)}

    def lanes(self) -> List[int]:
        """Lane of every layer: all 0 for a one-lane plan; long chains 0 / the rest 1 when the plan runs as two
        concurrent sub-plans (include/tadmm.h, tadmm_plan_lanes)."""
        out = (C.c_int32 * self.n)()
        self.h.lib.tadmm_plan_lanes(self._plan, out)
        return [int(x) for x in out]

    def filter_stats(self) -> dict:
        """Filtered eigen-solver counters: eligible problems of the plan; of the last run: solves, fallbacks, stages."""
        out = (C.c_int32 * 4)()
        self.h.check(self.h.lib.tadmm_plan_filter_stats(self._plan, out))
        return dict(eligible=int(out[0]), solves=int(out[1]), fallbacks=int(out[2]), stages=int(out[3]))

    def filter_timing(self) -> dict:
        """Instrumented runs: summed duration, count and executed FLOPs of the filter's fp64 GEMM launches."""
        out = (C.c_double * 4)()
        self.h.check(self.h.lib.tadmm_plan_filter_timing(self._plan, out))
        return dict(gemm_ms=float(out[0]), gemm_launches=int(out[1]), gemm_flops=float(out[2]))

    def filter_timing_fast(self) -> dict:
        """Instrumented runs: the filter products that ran at fp32 accuracy on the bf16 matrix cores (dgemm3_kernel)."""
        out = (C.c_double * 4)()
        self.h.check(self.h.lib.tadmm_plan_filter_timing_fast(self._plan, out))
        return dict(ms=float(out[0]), launches=int(out[1]), flops=float(out[2]))

    def jacobi_timing(self) -> dict:
        """Instrumented runs: summed duration, count, executed matrix-core FLOPs and workgroups of the jacobi_tick3 launches."""
        out = (C.c_double * 4)()
        self.h.check(self.h.lib.tadmm_plan_jacobi_timing(self._plan, out))
        return dict(tick_ms=float(out[0]), tick_launches=int(out[1]), tick_flops=float(out[2]), tick_wgs=float(out[3]))

    def singular_values(self, layer: int, step: int) -> np.ndarray:
        r = self.ranks[layer][step + 1]
        out = (C.c_double * r)()
        self.h.check(self.h.lib.tadmm_plan_singular_values(self._plan, layer, step, out, _stream(self.device)))
        return np.array(out[:], dtype=np.float64)

    def core_tensors(self, layer: int) -> List[torch.Tensor]:
        """Views (r_j, n_j, r_{j+1}) into the core buffer of a layer (want_cores=True)."""
        buf = self.cores[layer]
        if buf is None:
            raise TadmmError(-1, "plan was created without cores")
        out, off = [], 0
        for a, b, c in self._core_shapes[layer]:
            out.append(buf[off:off + a * b * c].view(a, b, c))
            off += a * b * c
        return out


# ------------------------------------------------------------------ grouped GEMM
def gemm_desc(A, B, Cout, M, N, K, a_strides, b_strides, c_strides, alpha=1.0, beta=0.0, bias_n=None, bias_m=None):
    g = GemmDesc()
    g.A, g.B, g.C = A, B, Cout
    g.M, g.N, g.K = M, N, K
    g.a_rs, g.a_cs = a_strides
    g.b_rs, g.b_cs = b_strides
    g.c_rs, g.c_cs = c_strides
    g.alpha, g.beta = alpha, beta
    g.bias_n = bias_n
    g.bias_m = bias_m
    return g


class TuckerPlan(_LayerPlan):
    """Grouped Tucker-2 projection of a set of layers (the 'tk' branches of ADMM.update, admm.py:47-50, :59-62).

    layers: sequence of dicts with keys W, U, Z (float32 device tensors, 4-D (O,I,kh,kw) or 2-D (out,in)) and
    ranks = [r_out, r_in].  HOSVD + HOOI for all layers in lock-step on the device (csrc/tucker_plan.hip).
    """

    _PREFIX = "tadmm_tucker_"

    def __init__(self, layers: Sequence[dict], n_iter_max: int = 100, tol: float = 1e-4):
        self._shapes = []

        def desc(L):
            shape = list(L["W"].shape)
            if len(shape) not in (2, 4):
                raise TadmmError(-1, "Tucker layers are 2-D or 4-D")
            self._shapes.append((shape, int(L["ranks"][0]), int(L["ranks"][1])))
            return make_layer_desc(KIND_TUCKER2, shape, None, L["ranks"], 0, n_iter_max, tol)

        super().__init__(layers, desc)
        self._create()

    def _view(self, ptr: int, numel: int) -> torch.Tensor:
        off = ptr - self.workspace.data_ptr()
        return self.workspace[off:off + 4 * numel].view(torch.float32)

    def factors(self, layer: int):
        """(core, U_out, U_in) of the last run as tensors shaped like tensorly's partial_tucker output:
        core (r_out, r_in, kh, kw) | (r_out, r_in), U_out (O, r_out), U_in (I, r_in).  Copies."""
        shape, ro, ri = self._shapes[layer]
        c, a, b = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.h.check(self.h.lib.tadmm_tucker_factors(self._plan, layer, C.byref(c), C.byref(a), C.byref(b)))
        k2 = shape[2] * shape[3] if len(shape) == 4 else 1
        core = self._view(c.value, ro * k2 * ri).view(ro, k2, ri).permute(0, 2, 1).contiguous()
        core = core.view(ro, ri, shape[2], shape[3]) if len(shape) == 4 else core.view(ro, ri)
        u_out = self._view(a.value, shape[0] * ro).view(shape[0], ro).clone()
        u_in = self._view(b.value, shape[1] * ri).view(shape[1], ri).clone()
        return core, u_out, u_in

    def iterations(self):
        """(HOOI sweeps per layer, final relative reconstruction error per layer) of the last run."""
        it = (C.c_int32 * self.n)()
        err = (C.c_double * self.n)()
        self.h.check(self.h.lib.tadmm_tucker_iterations(self._plan, it, err, _stream(self.device)))
        return list(it), list(err)

    def jacobi_sweeps(self) -> int:
        """Jacobi sweeps summed over all eigen-solve groups of the last run."""
        return int(self.h.lib.tadmm_tucker_jacobi_sweeps(self._plan))

    def last_timing(self) -> dict:
        """Instrumented run: eigen-solver launches timed one by one with HIP events on the launch stream."""
        out = (C.c_double * 8)()
        self.h.check(self.h.lib.tadmm_tucker_last_timing(self._plan, out))
        return dict(eig_ms=out[0], eig_launches=int(out[1]), eig_model_flops=out[2], total_ms=out[3], hooi_sweeps=int(out[4]))


class GemmBatch:
    """A packed group of strided GEMMs; `run()` is one kernel launch."""

    def __init__(self, descs: Sequence[GemmDesc], device):
        self.device = device
        self.h = _handle(device)
        lib = self.h.lib
        n = len(descs)
        arr = (GemmDesc * n)(*descs)
        nbytes = lib.tadmm_gemm_pack_bytes(n, arr)
        if nbytes == 0:
            raise TadmmError(-1, "tadmm_gemm_pack: invalid GEMM descriptor (positive extents, and each "
                                                "operand needs one unit stride)")
        host = torch.empty(nbytes, dtype=torch.uint8).pin_memory() if torch.cuda.is_available() else \
            torch.empty(nbytes, dtype=torch.uint8)
        nblocks = C.c_int()
        rc = lib.tadmm_gemm_pack(n, arr, host.data_ptr(), nbytes, C.byref(nblocks))
        if rc < 0:
            raise TadmmError(rc, "tadmm_gemm_pack: invalid GEMM descriptor (each operand needs one unit stride)")
        # a blocking copy: `run()` may be called under any stream and the caller holds no tensor to wait on, so the blob is
        # valid for every stream when the constructor returns (what the native `*_plan_create` entries keep)
        self.blob = host.to(device, non_blocking=False)
        self.n, self.nblocks = n, int(nblocks.value)

    def run(self):
        self.h.check(self.h.lib.tadmm_gemm_run(self.h.ptr, self.blob.data_ptr(), self.n, self.nblocks,
                                               _stream(self.device)))


def mm(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, alpha=1.0, bias_n=None, bias_m=None,
       beta=0.0):
    """out = alpha * a @ b (+ beta * out) (+bias) for 2-D float32 device tensors with arbitrary (one unit) strides.
    `out` is read only when beta != 0."""
    assert a.dim() == 2 and b.dim() == 2 and a.shape[1] == b.shape[0]
    M, K = a.shape
    N = b.shape[1]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    d = gemm_desc(a.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K, a.stride(), b.stride(), out.stride(), alpha, beta,
                  None if bias_n is None else bias_n.data_ptr(), None if bias_m is None else bias_m.data_ptr())
    dev = a.device
    h = _handle(dev)
    h.check(h.lib.tadmm_gemm(h.ptr, C.byref(d), _stream(dev)))       # descriptor by value: one launch, no upload
    return out


def mm_nt_bf16(a: torch.Tensor, bt: torch.Tensor, bias_n: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a (M,K) @ bt (N,K)^T [+ bias over N] in bf16 with fp32 accumulation; rows contiguous along K."""
    assert a.dim() == 2 and bt.dim() == 2 and a.shape[1] == bt.shape[1]
    for t, what in ((a, "a"), (bt, "bt")):
        _operand(t, "", what, (torch.bfloat16,), layout=None)
        if t.stride(1) != 1:
            raise TadmmError(-1, f"{what} must be contiguous along K")
    M, K = a.shape
    N = bt.shape[0]
    out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    if bias_n is not None:
        bias_n = bias_n.float().contiguous()
    dev = a.device
    h = _handle(dev)
    h.check(h.lib.tadmm_gemm_bf16_nt(h.ptr, a.data_ptr(), bt.data_ptr(), out.data_ptr(), M, N, K, a.stride(0),
                                     bt.stride(0), N, None if bias_n is None else bias_n.data_ptr(), _stream(dev)))
    return out


# ------------------------------------------------------------------ weight gradients (csrc/wgrad.hip)
def _wgrad_operands(a: torch.Tensor, b: torch.Tensor):
    """Validated (a, b, T, M, N, hw) of a weight-gradient product; the only copies are `.contiguous()` of a row tensor
    without unit feature stride or of a non-contiguous image (alignment is the kernel's business)."""
    for t, what in ((a, "a"), (b, "b")):
        _operand(t, "wgrad", what, layout=None)
    if a.device != b.device:
        raise TadmmError(-1, f"wgrad: operands on different devices ({a.device}, {b.device})")
    if a.dtype != b.dtype:
        raise TadmmError(-1, f"wgrad: operands must share one dtype (got {a.dtype}, {b.dtype})")
    if a.dtype not in (torch.float32, torch.bfloat16):
        raise TadmmError(-1, f"wgrad: operands must be float32 or bfloat16 (got {a.dtype})")
    if a.dim() != b.dim() or a.dim() not in (2, 4):
        raise TadmmError(-1, f"wgrad: two (T, features) row tensors or two NCHW images (got {a.dim()}-D and {b.dim()}-D)")
    if a.dim() == 4:
        if (a.shape[0],) + tuple(a.shape[2:]) != (b.shape[0],) + tuple(b.shape[2:]):
            raise TadmmError(-1, f"wgrad: images differ in (B, H, W): {tuple(a.shape)} vs {tuple(b.shape)}")
        hw = a.shape[2] * a.shape[3]
        if a.shape[0] > 0 and hw == 0:
            raise TadmmError(-1, "wgrad: images without pixels")
        a = a if a.is_contiguous() else a.contiguous()
        b = b if b.is_contiguous() else b.contiguous()
        return a, b, a.shape[0] * hw, a.shape[1], b.shape[1], max(hw, 1)
    if a.shape[0] != b.shape[0]:
        raise TadmmError(-1, f"wgrad: operands differ in T: {a.shape[0]} vs {b.shape[0]}")
    a = a if a.stride(1) == 1 and a.stride(0) >= a.shape[1] else a.contiguous()
    b = b if b.stride(1) == 1 and b.stride(0) >= b.shape[1] else b.contiguous()
    return a, b, a.shape[0], a.shape[1], b.shape[1], 0


def _wgrad_desc(a, b, T, M, N, hw, alpha: float = 1.0):
    d = _cabi.WgradDesc()
    d.A, d.B, d.T, d.M, d.N, d.hw = a.data_ptr(), b.data_ptr(), T, M, N, hw
    d.lda, d.ldb = (0, 0) if hw else (a.stride(0), b.stride(0))
    d.dtype = _cabi.CHAIN_F32 if a.dtype == torch.float32 else _cabi.CHAIN_BF16
    d.alpha = float(alpha)
    return d


def wgrad_plan(a: torch.Tensor, b: torch.Tensor):
    """(workspace bytes, slices of T) `wgrad(a, b)` will use: `tadmm_wgrad_workspace_bytes`, a pure function of the
    shapes."""
    a, b, T, M, N, hw = _wgrad_operands(a, b)
    if M == 0 or N == 0:
        return 0, 1
    nbytes, slices = C.c_size_t(), C.c_int()
    rc = _cabi.load().tadmm_wgrad_workspace_bytes(C.byref(_wgrad_desc(a, b, T, M, N, hw)), C.byref(nbytes),
                                                  C.byref(slices))
    if rc < 0:
        raise TadmmError(rc, "tadmm_wgrad_workspace_bytes: the launch does not take this shape")
    return nbytes.value, slices.value


def wgrad(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, alpha: float = 1.0) -> torch.Tensor:
    """out (M, N) float32 = alpha * sum_t a[t, :]^T b[t, :]: the weight-gradient product of the factorised layers
    (`tadmm_wgrad`, csrc/wgrad.hip).  `a`, `b`: two row tensors (T, M) / (T, N) or two NCHW images (B, M, H, W) /
    (B, N, H, W), t = (batch, pixel), both float32 or both bfloat16, read in place; split over T, deterministic."""
    a, b, T, M, N, hw = _wgrad_operands(a, b)
    out = _output(out, (M, N), torch.float32, a.device, "wgrad: out", strided_rows=True)
    if M == 0 or N == 0:
        return out
    d = _wgrad_desc(a, b, T, M, N, hw, alpha)
    d.C, d.ldc = out.data_ptr(), out.stride(0) if M > 1 else max(out.stride(0), N)
    dev = a.device
    h = _handle(dev)
    nbytes, slices = C.c_size_t(), C.c_int()
    h.check(h.lib.tadmm_wgrad_workspace_bytes(C.byref(d), C.byref(nbytes), C.byref(slices)))
    ws = _scratch(nbytes.value, dev) if nbytes.value else None
    h.check(h.lib.tadmm_wgrad(h.ptr, C.byref(d), None if ws is None else ws.data_ptr(), nbytes.value, _stream(dev)))
    return out


# ------------------------------------------------------------------ forward chains (csrc/chain.hip)
def weight_planes(w: torch.Tensor, planes: int, pad_rows: int = 16, pad_cols: int = 32,
                  dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """(N, K) weight -> (planes, Np/16, Kp/32, 64, 8) bfloat16 in the fragment-major order of csrc/chain.hip
    (Kp = K rounded up to `pad_cols`, a multiple of 32; Np = N rounded up to `pad_rows`, a multiple of 16; zero
    padded).  The fused chain wants its middle rank padded to 64: `pad_rows=64` for Win, `pad_cols=64` for Wout.
    planes == 3: the exact three-term split w = w1 + w2 + w3 of a float32 weight; planes == 1: its bf16 rounding.
    `dtype=torch.float16` (planes == 1 only): the binary16 rounding of w in the same order, for float16 activations."""
    assert w.dim() == 2 and planes in (1, 3) and pad_rows % 16 == 0 and pad_cols % 32 == 0
    if dtype not in (torch.bfloat16, torch.float16):
        raise TadmmError(-1, f"weight planes are bfloat16 or float16 (got {dtype})")
    if dtype == torch.float16 and planes != 1:
        raise TadmmError(-1, "float16 weights are ONE plane: the three-plane split belongs to float32 activations")
    _operand(w, "", "weights", layout=None)
    N, K = w.shape
    Np, Kp = -(-N // pad_rows) * pad_rows, -(-K // pad_cols) * pad_cols
    flat = torch.zeros(planes, Np, Kp, dtype=dtype, device=w.device)
    r = w.detach().float()
    for p in range(planes):
        t = r.to(dtype)
        flat[p, :N, :K] = t
        if p + 1 < planes:
            r = r - t.float()
    # (p, n/16, n%16, k/32, (k%32)/8, k%8) -> (p, n/16, k/32, (k%32)/8, n%16, k%8)
    return flat.view(planes, Np // 16, 16, Kp // 32, 4, 8).permute(0, 1, 3, 4, 2, 5).contiguous().view(
        planes, Np // 16, Kp // 32, 64, 8)


def unpack_planes(wp: torch.Tensor) -> torch.Tensor:
    """Inverse of `weight_planes`: (planes, Np, Kp) bfloat16 row-major (tests, debugging)."""
    P, nt, ks = wp.shape[:3]
    return wp.view(P, nt, ks, 4, 16, 8).permute(0, 1, 4, 2, 3, 5).reshape(P, nt * 16, ks * 32)


class _LruMemo(collections.OrderedDict):
    """Validated descriptors of recent chain launches, keyed on geometry + weight-plane addresses.  An entry pins its
    plane tensors (that is what keeps the addresses meaningful), so the memo is a small LRU: callers whose planes are
    short-lived (the autograd Functions pack fresh planes every call) pass `memo=False` and never enter it."""
    CAP = 128

    def lookup(self, key):
        hit = self.get(key)
        if hit is not None:
            self.move_to_end(key)
        return hit

    def store(self, key, value):
        self[key] = value
        self.move_to_end(key)
        while len(self) > self.CAP:
            self.popitem(last=False)


_CHAIN_MEMO = _LruMemo()


def _memoised(key, build):
    """The launch record of `key`: the memo's, else `build()`'s, which is then stored.  A key of None is not memoised."""
    if key is None:
        return build()
    hit = _CHAIN_MEMO.lookup(key)
    if hit is None:
        hit = build()
        _CHAIN_MEMO.store(key, hit)
    return hit

# activation dtypes whose one 16-bit weight plane runs the single-plane kernels (float16: inference entries only)
HALF_DTYPES = (torch.bfloat16, torch.float16)


def _chain_dtype(xdtype, who: str):
    """(C ABI dtype, plane count, plane dtype) of an activation dtype.  The library sees `void*` planes and cannot tell
    a bfloat16 plane from a binary16 one, so the callers compare the plane tensors' dtype with the third element."""
    if xdtype == torch.float32:
        return _cabi.CHAIN_F32, 3, torch.bfloat16
    if xdtype == torch.bfloat16:
        return _cabi.CHAIN_BF16, 1, torch.bfloat16
    if xdtype == torch.float16:
        return _cabi.CHAIN_F16, 1, torch.float16
    raise TadmmError(-1, f"{who}: unsupported dtype {xdtype}")


def _f32_bias(bias):
    """(the bias as the kernels read it: contiguous float32, its launch-memo key).  The key is None for a converted copy:
    nothing to memoise."""
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous()):
        return bias.detach().float().contiguous(), None
    return bias, 0 if bias is None else bias.data_ptr()


def _out_tensors(out, shapes, like):
    """One contiguous tensor of `like`'s dtype and device per shape: the caller's (`out`: a tensor or a sequence, None
    entries allowed) where given, else a fresh one."""
    given = (out,) if isinstance(out, torch.Tensor) else (tuple(out) if out is not None else ())
    return [_output(t, tuple(shape), like.dtype, like.device, "conv chain: `out`")
            for shape, t in zip(shapes, given + (None,) * len(shapes))]


def _check_planes(planes, nplanes: int, dtype, who: str):
    """Weight planes as `weight_planes` packs them: `nplanes` contiguous 5-D planes of `dtype`."""
    if (not isinstance(planes, torch.Tensor) or planes.dtype != dtype or planes.dim() != 5 or planes.shape[0] != nplanes
            or not planes.is_contiguous()):
        raise TadmmError(-1, f"{who}: weights must be {nplanes} contiguous {dtype} plane(s) (ops.weight_planes)")


def _chain_call(entry: str, x: torch.Tensor, win: torch.Tensor, wout, bias, kin: int, n1: int, n_out: int,
                image_out: bool, tile_tokens: int, prepare_only: bool = False, use_memo: bool = True, save_rank: int = 0):
    """`save_rank` > 0: `entry` is one of the `_save` entries; the launch also stores the first `save_rank` columns of the
    middle-rank vector and the result is (y, h).  Such a launch never enters the memo."""
    if save_rank:
        use_memo = False
    _operand(x, "", "x", layout=None)
    if x.dim() == 4:                                   # (B, C, H, W) read in place
        if not x.is_contiguous():
            x = x.contiguous()
    elif x.stride(1) != 1 or (x.stride(0) * x.element_size()) % 16 or x.data_ptr() % 16:
        x = x.contiguous()
    bias, bias_key = _f32_bias(bias)
    if not use_memo:
        bias_key = None                                 # short-lived planes (training): build, launch, forget
    # geometry + weight identity -> validated descriptor; only the activation pointers change between calls
    # (the planes' dtype is part of their identity: a bfloat16 view of a binary16 plane shares its address)
    key = (entry, tuple(x.shape), x.stride(0), x.dtype, x.device, win.data_ptr(), win.dtype,
           (0, None) if wout is None else (wout.data_ptr(), wout.dtype), bias_key, kin, n1, n_out, image_out, tile_tokens)

    def build():
        dtype, planes, pdt = _chain_dtype(x.dtype, "chain")
        _check_planes(win, planes, pdt, "chain")
        d = _cabi.ChainDesc()
        if x.dim() == 4:
            B, Cc, H, W = x.shape
            assert Cc == kin
            T, hw = B * H * W, H * W
            d.x_hw, d.ldx = hw, 0
        else:
            assert x.dim() == 2 and x.shape[1] == kin
            T, hw = x.shape[0], 0
            d.x_hw, d.ldx = 0, x.stride(0)
        feat = n_out if wout is not None else n1
        if image_out:
            assert hw > 0
            yshape = (x.shape[0], feat, x.shape[2], x.shape[3])
            d.y_hw, d.ldy = hw, 0
        else:
            yshape = (T, feat)
            d.y_hw, d.ldy = 0, feat
        d.Win = win.data_ptr()
        d.Wout = None if wout is None else wout.data_ptr()
        d.bias = None if bias is None else bias.data_ptr()
        d.T, d.Kin, d.R, d.Nout = T, kin, n1, n_out if wout is not None else 0
        if win.shape[2] != -(-kin // 32) or win.shape[1] * 16 < n1:
            raise TadmmError(-1, "chain: weight planes do not match the operand shape")
        d.win_plane = win[0].numel()
        if wout is not None:
            _check_planes(wout, planes, pdt, "chain")
            if wout.shape[2] * 32 != n1 or wout.shape[1] * 16 < n_out:
                raise TadmmError(-1, "chain: output weight planes do not match the middle rank / output size")
            d.wout_plane = wout[0].numel()
        d.dtype, d.tile_tokens = dtype, tile_tokens
        h = _handle(x.device)
        return d, getattr(h.lib, entry), h, yshape, T, (win, wout, bias)     # the tuple keeps the weights alive

    d, fn, h, yshape, T, _ = _memoised(key if bias_key is not None else None, build)
    y = torch.empty(yshape, dtype=x.dtype, device=x.device)
    hbuf, ldh = None, 0
    if save_rank:
        if not 0 < save_rank <= n1:
            raise TadmmError(-1, f"chain: true rank {save_rank} outside (0, {n1}]")
        if x.dim() == 4:                               # one contiguous NCHW tensor: the image layout of `wgrad`
            ldh = save_rank
            hbuf = torch.empty((x.shape[0], save_rank, x.shape[2], x.shape[3]), dtype=x.dtype, device=x.device)
        else:                                          # rows padded to whole 16-byte units: every store is a vector
            epl = 16 // x.element_size()
            ldh = -(-save_rank // epl) * epl
            hbuf = torch.empty((T, ldh), dtype=x.dtype, device=x.device)[:, :save_rank]

    def launch():
        d.X, d.Y = x.data_ptr(), y.data_ptr()
        if T > 0 and save_rank:
            h.check(fn(h.ptr, C.byref(d), save_rank, hbuf.data_ptr(), ldh, _stream(x.device)))
        elif T > 0:
            h.check(fn(h.ptr, C.byref(d), _stream(x.device)))
        return (y, hbuf) if save_rank else y

    if prepare_only:
        return launch
    return launch()


def chain_fused(x, win_planes, wout_planes, bias, n_out: int, entry: str = "tadmm_ttlinear_fwd", tile_tokens: int = 0,
                prepare_only: bool = False, memo: bool = True):
    """y (T, n_out) = (x (T, Kin) @ Win^T) @ Wout^T + bias in one launch (TTLinear.py:75-93).  `win_planes` (rows
    padded to the middle rank R, a multiple of 64, <= 256) and `wout_planes` come from `weight_planes`."""
    return _chain_call(entry, x, win_planes, wout_planes, bias, x.shape[-1], win_planes.shape[1] * 16, n_out, False,
                       tile_tokens, prepare_only, memo)


def chain_fused_save(x, win_planes, wout_planes, bias, n_out: int, r: int, entry: str = "tadmm_ttlinear_fwd_save",
                     tile_tokens: int = 0):
    """`chain_fused` that also returns the middle-rank vector of every token: (y (T, n_out), h (T, r)) with
    h = x @ Win^T -- what the launch keeps in LDS between its two products, stored in x's dtype (bfloat16: the rounding
    product 2 reads; float32: the fp32 accumulator).  `r` is the true middle rank, at most the planes' padded one; y is
    bit-identical to `chain_fused`'s.  `entry="tadmm_ttlinear_bwd_save"` with the transposed planes of the data gradient:
    (dX, dH = dY @ Wout).  h is a (T, r) view of rows padded to whole 16-byte units (`ops.wgrad` reads it in place); it
    lives as long as the caller keeps it: T x r elements the plain launch never materialises.  float32 and bfloat16
    only; no launch memo (training packs its planes every step)."""
    return _chain_call(entry, x, win_planes, wout_planes, bias, x.shape[-1], win_planes.shape[1] * 16, n_out, False,
                       tile_tokens, save_rank=r)


def chain_single(x, w_planes, bias, n_out: int, entry: str = "tadmm_ttconv_chain_in", image_out: bool = False,
                 tile_tokens: int = 0, prepare_only: bool = False, memo: bool = True):
    """y = x @ W^T + bias for token rows (T, Kin) or, in place, a channels-first image (B, Kin, H, W) ->
    (B, n_out, H, W) when `image_out` (TTConv.py:131-137 / :141-151, TKConv.py:93-98).  `prepare_only` returns a
    zero-argument launcher over the same buffers (benchmarks: no per-call descriptor building)."""
    kin = x.shape[1]
    return _chain_call(entry, x, w_planes, None, bias, kin, n_out, 0, image_out, tile_tokens, prepare_only, memo)


def svd_conv(x, win_planes, wout_planes, bias, n_out: int, entry: str = "tadmm_svdconv_fwd", tile_tokens: int = 0,
             prepare_only: bool = False, memo: bool = True):
    """y (B, n_out, H, W) = Wout (Win x[b,:,p]) + bias for every pixel of an NCHW image, in one launch, in place on both
    sides (SVDConv.py: SVDConv2dC / SVDConv2dM at padding 0).  Planes as for `chain_fused`: `win_planes` with the rank
    padded to a multiple of 64 (<= 256), `wout_planes` with `pad_cols=64`."""
    if x.dim() != 4:
        raise TadmmError(-1, "svd_conv: x must be an NCHW image")
    return _chain_call(entry, x, win_planes, wout_planes, bias, x.shape[1], win_planes.shape[1] * 16, n_out, True,
                       tile_tokens, prepare_only, memo)


def svd_conv_save(x, win_planes, wout_planes, bias, n_out: int, r: int, entry: str = "tadmm_svdconv_fwd_save",
                  tile_tokens: int = 0):
    """`svd_conv` that also returns the rank-r image between its two products: (y (B, n_out, H, W), h (B, r, H, W)),
    h = Win x per pixel, contiguous NCHW in x's dtype (see `chain_fused_save`).  `entry="tadmm_svdconv_bwd_save"` with the
    transposed planes: (dX, dH = Wout^T dY).  Keeps B x r x H x W elements alive that the plain launch does not."""
    if x.dim() != 4:
        raise TadmmError(-1, "svd_conv_save: x must be an NCHW image")
    return _chain_call(entry, x, win_planes, wout_planes, bias, x.shape[1], win_planes.shape[1] * 16, n_out, True,
                       tile_tokens, save_rank=r)


def chain_train_pays(x: torch.Tensor, r: int, n_in: int, n_out: int, image: bool, factor_grad: bool = True) -> bool:
    """True when a training step of the fused chain -- token rows (T, n_in), or with `image` an NCHW tensor
    (B, n_in, H, W), through middle rank `r` to `n_out` features -- should store its middle-rank intermediates
    (`chain_fused_save` / `svd_conv_save`: four launches, H kept from forward to backward) instead of recomputing them in
    the backward (two extra `chain_single` launches, nothing kept).  A pure function of its arguments: dtype, shape, the
    numbers given.  Always False where the saving entries do not exist or nothing would read what they store: float16,
    ranks above 256 (or below 1), and `factor_grad=False` -- no factor wants a gradient.
    The rule proper is set by `scripts/bench_linear_train.py`: True only for a dtype / shape
    class in which the saved route is ahead of the recomputing one by more than the min..max spread of both.  No class
    has been shown to be: the rule is False everywhere, today's route stays the default, and the saving entries are
    reached with `save=True`."""
    if not factor_grad or x.dtype not in (torch.float32, torch.bfloat16) or not 0 < r <= 256:
        return False
    return False


def svd_conv_pays(x: torch.Tensor, rank: int) -> bool:
    """True when the one-launch 1x1 chain (`svd_conv`) is the path to take for a rank-`rank` 1x1 convolution of x; False:
    two `tadmm_tucker_1x1` launches.  Measured (scripts/bench_svd_layers.py): in bf16 the fused
    launch is faster on all 56 single-rank layers of svd_mobilenetv2_cifar / tk_resnet50 (1.06x - 2.3x); in fp32 (three
    planes, six MFMA products per product, the rank padded to 64) the second product's padded work costs more than the
    intermediate's round trip saves, and two launches are 4 - 17 % faster over each table.  Ranks above 256 never fit
    the LDS of the fused kernel.  float16 (inference) runs the bf16 kernel with the f16 MFMA and takes bf16's rule: it times
    as bf16 does on the chain kernels (the SVD tables themselves were not re-timed in float16)."""
    return x.dtype in HALF_DTYPES and 0 < rank <= 256


_INT32_MAX = 2 ** 31 - 1


@functools.lru_cache(maxsize=256)
def _conv_plan(x_shape, dtype, r1: int, r2: int, kernel_size, stride, padding, dilation, mode: int):
    """(pixels per workgroup, rows per workgroup, halo tiles, workgroups per image) of the one-launch factorised
    convolution (`mode` FWD) or of its data gradient (BWD) on an input of shape x_shape, or None where the launch does
    not apply: `tadmm_ttconv_fused_plan`, the library's own statement of the tile search (host only; plan_tt_conv in
    csrc/convchain.hip; tests/test_conv_chain_plan_cpu.py holds an independent statement against it).  The plan reads
    neither the channel count nor the output features, only that they are positive.  A pure function of hashable
    arguments, cached: the layers ask on every routed forward, and the ctypes call costs three times the Python loop
    it replaced (12 us against 4 us)."""
    dtypes = {torch.float32: _cabi.CHAIN_F32, torch.bfloat16: _cabi.CHAIN_BF16}
    if mode == _cabi.CONV_CHAIN_FWD:
        dtypes[torch.float16] = _cabi.CHAIN_F16
    if len(x_shape) != 4 or dtype not in dtypes:
        return None
    B, Cc, H, W = (int(v) for v in x_shape)
    geom = tuple(int(v) for pair in (kernel_size, stride, padding, dilation) for v in pair)
    ranks = (-(-int(r1) // 32) * 32, -(-int(r2) // 32) * 32)
    # a value ctypes would wrap into an int32 field never reaches the library
    if max(B, Cc, H, W, *ranks, *(abs(v) for v in geom)) > _INT32_MAX or H <= 0 or W <= 0:
        return None
    ho, wo = _conv_out_hw(H, W, geom[0:2], geom[2:4], geom[4:6], geom[6:8])
    if ho <= 0 or wo <= 0 or max(ho, wo) > _INT32_MAX:
        return None
    d = _cabi.ConvChainDesc()
    d.dtype, d.B, d.C, d.Nout, d.H, d.W, d.Ho, d.Wo = dtypes[dtype], B, Cc, 1, H, W, ho, wo
    d.R1, d.R2 = ranks
    d.kh, d.kw, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = geom
    out = [C.c_int() for _ in range(4)]
    rc = _cabi.load().tadmm_ttconv_fused_plan(C.byref(d), mode, *[C.byref(v) for v in out], None)
    if rc == -5:
        return None
    if rc < 0:
        raise TadmmError(rc, "tadmm_ttconv_fused_plan: invalid descriptor")
    return tuple(v.value for v in out)


def _conv_chain_plan(x: torch.Tensor, r1: int, r2: int, kernel_size, stride, padding, dilation):
    """(pixels per workgroup, output rows per workgroup, halo tiles, workgroups per image) of the one-launch factorised
    convolution, or None when it does not apply -- the rule tadmm_ttconv_fused applies.  The tile is a run of output
    rows, its halo the input rows the taps reach."""
    return _conv_plan(tuple(x.shape), x.dtype, r1, r2, tuple(kernel_size), tuple(stride), tuple(padding), tuple(dilation),
                      _cabi.CONV_CHAIN_FWD)


def conv_chain_fits(x: torch.Tensor, r1: int, r2: int, kernel_size, stride, padding, dilation) -> bool:
    """True when the one-launch factorised convolution (csrc/convchain.hip) applies: output rows of at most 64 pixels,
    a tile of output rows whose halo is at most three pixel tiles, ranks at most 256 and both intermediates inside the
    160 KiB of LDS."""
    return _conv_chain_plan(x, r1, r2, kernel_size, stride, padding, dilation) is not None


def conv_chain_pays(x: torch.Tensor, r1: int, r2: int, kernel_size, stride, padding, dilation) -> bool:
    """... and is the faster path (measured, scripts/bench_conv_layers.py): always in bf16; in fp32 (three planes, six
    MFMA products per product) only while an image is at most two workgroups -- with more row tiles the recomputed halos
    cost more than the two launches and the round trip of the intermediates they save."""
    plan = _conv_chain_plan(x, r1, r2, kernel_size, stride, padding, dilation)
    return plan is not None and (x.dtype in HALF_DTYPES or plan[3] <= 2)     # float16: bf16's rule (times as bf16; three f16 launches are ~14 % ahead at 28x28 and 56x56, left open)


def conv_core_planes(core: torch.Tensor, planes: int, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """(r2, r1, kh, kw) core kernel -> fragment-major planes of the (r2 x kh*kw*r1p) tap-major matrix convchain.hip
    multiplies with (r1p = r1 rounded up to 32, rows rounded up to 32).  `dtype`: as for `weight_planes`."""
    r2, r1, kh, kw = core.shape
    r1p = -(-r1 // 32) * 32
    m = torch.zeros(r2, kh * kw, r1p, dtype=torch.float32, device=core.device)
    m[:, :, :r1] = core.detach().float().permute(0, 2, 3, 1).reshape(r2, kh * kw, r1)
    return weight_planes(m.reshape(r2, kh * kw * r1p), planes, pad_rows=32, dtype=dtype)


def _conv_chain_bwd_plan(x_shape, dtype, r1: int, r2: int, kernel_size, stride, padding, dilation):
    """(pixels per workgroup, dX rows per workgroup, halo tiles, workgroups per image) of the one-launch data gradient of
    the factorised convolution of an input of shape x_shape, or None when it does not apply -- the rule
    `tadmm_ttconv_fused_bwd` applies.  The tile is a run of dX rows, its halo the dY rows the taps reach, and the tap
    table joins the LDS.  float32 and bfloat16 only."""
    return _conv_plan(tuple(x_shape), dtype, r1, r2, tuple(kernel_size), tuple(stride), tuple(padding), tuple(dilation),
                      _cabi.CONV_CHAIN_BWD)


def conv_chain_bwd_fits(x: torch.Tensor, r1: int, r2: int, kernel_size, stride, padding, dilation) -> bool:
    """True when the one-launch data gradient (`conv_chain_bwd`) applies to the layer whose INPUT is x: input rows of at
    most 64 pixels, a tile of dX rows whose dY halo is at most three pixel tiles, ranks at most 256 and the intermediates
    plus the tap table inside the 160 KiB of LDS.  Host-only shape logic."""
    return _conv_chain_bwd_plan(tuple(x.shape), x.dtype, r1, r2, kernel_size, stride, padding, dilation) is not None


def conv_chain_train_pays(x: torch.Tensor, r1: int, r2: int, kernel_size, stride, padding, dilation,
                          training: bool) -> bool:
    """True when a layer in grad mode routes to `functional.conv_chain` (one forward launch, one data-gradient launch)
    instead of the three differentiable launches.  Two classes: `training` False is the FROZEN class (only x, or x and
    the bias, want a gradient: nothing is saved), True the TRAINING class (a factor wants a gradient: the launches also
    store H1 / H2 and dH1 / dH2, and three weight gradients follow).
    Measured (scripts/bench_conv_train.py) on the 30 distinct 3 x 3 layers of resnet18_tt 2x,
    resnet50_tt 3x, tk_resnet50 3x (batch 32) and tk_resnet32 3x (batch 128), forward + backward against the three-launch
    path in the same process; "ahead" = the new median below the old path's fastest round:
      frozen, bf16: ahead at 30 of 30 (1.23x - 3.31x): always.
      frozen, fp32 (22 fit): ahead at all 19 layers of at most 1024 workgroups (batch x row tiles; 1.23x - 3.93x), behind
        at the 3 of 1792 and more (56 x 56 planes at batch 32, 32 x 32 at batch 128: 0.81x - 0.87x, the recomputed halos
        at six MFMA products per product): up to 1024 workgroups.  Nothing was measured between 1024 and 1792.
      training, fp32: behind at 22 of 22 with either weight gradient of the core (0.64x - 1.11x): never.
      training, bf16: with dWc through `core_conv_wgrad` ahead at all 21 layers whose input plane has at most 1024 pixels
        (1.13x - 1.47x; through the device library's weight gradient 1.01x - 1.34x and ahead at 18 of them) and at 3 of the
        9 on 56 x 56 inputs (0.82x - 1.20x): planes of at most 1024 pixels, dWc native."""
    plan = _conv_chain_plan(x, r1, r2, kernel_size, stride, padding, dilation)
    if plan is None or x.dtype == torch.float16:         # float16 is inference only: no saved intermediates, no dX
        return False
    bf16 = x.dtype == torch.bfloat16
    if not training:
        return bf16 or x.shape[0] * plan[3] <= 1024
    return bf16 and x.shape[2] * x.shape[3] <= 1024


def _conv_chain_desc(B, Cc, H, W, n_out, w1p, w2p, w3p, bias, dtype, kernel_size, stride, padding, dilation, bwd=False):
    d = _cabi.ConvChainDesc()
    d.dtype, nplanes, pdt = _chain_dtype(dtype, "conv chain")
    for wp in (w1p, w2p, w3p):
        _check_planes(wp, nplanes, pdt, "conv chain")
    ho, wo = _conv_out_hw(H, W, kernel_size, stride, padding, dilation)
    d.W1, d.W2, d.W3 = w1p.data_ptr(), w2p.data_ptr(), w3p.data_ptr()
    d.bias = None if bias is None else bias.data_ptr()
    d.w1_plane, d.w2_plane, d.w3_plane = w1p[0].numel(), w2p[0].numel(), w3p[0].numel()
    # forward: W1 (R1 x C), W2 (R2 x taps*R1), W3 (Nout x R2); data gradient: W3^T (R2 x Nout), core^T (R1 x taps*R2), W1^T (C x R1)
    ra, rb = w1p.shape[1] * 16, w2p.shape[1] * 16
    d.R1, d.R2 = (rb, ra) if bwd else (ra, rb)
    d.B, d.C, d.Nout = B, Cc, n_out
    d.H, d.W, d.Ho, d.Wo, d.kh, d.kw = H, W, ho, wo, kernel_size[0], kernel_size[1]
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = (stride[0], stride[1], padding[0], padding[1],
                                                                  dilation[0], dilation[1])
    if (w2p.shape[2] * 32 != kernel_size[0] * kernel_size[1] * ra or w3p.shape[2] * 32 != rb
            or w1p.shape[2] != -(-(n_out if bwd else Cc) // 32)):
        raise TadmmError(-1, "conv chain: weight planes do not match each other")
    return d, ho, wo


def conv_chain(x: torch.Tensor, w1p: torch.Tensor, w2p: torch.Tensor, w3p: torch.Tensor, bias, n_out: int, kernel_size,
               stride, padding, dilation, save_ranks=None, memo: bool = True, out=None):
    """y (B, n_out, Ho, Wo) = W3 conv_kxk(W1 x; Wc) + bias for NCHW images in one launch (`tadmm_ttconv_fused`; see
    `conv_chain_fits` for what is eligible).
    w1p = weight_planes(W1, P, pad_rows=32), w2p = conv_core_planes(core, P), w3p = weight_planes(W3, P).
    `save_ranks` = (r1, r2): see `conv_chain_save`.  `memo` False: planes packed for this call only stay out of the launch
    memo.  `out`: contiguous tensors to write instead of fresh ones -- y, or (y, H1, H2) with `save_ranks`."""
    x = _operand(x, "", "x", layout="copy")
    bias, bias_key = _f32_bias(bias)
    if save_ranks is not None or not memo:
        bias_key = None                                 # training: the planes are short-lived -- build, launch, forget
    key = ("conv", tuple(x.shape), x.dtype, x.device, w1p.data_ptr(), w2p.data_ptr(), w3p.data_ptr(),
           (w1p.dtype, w2p.dtype, w3p.dtype), bias_key, n_out, tuple(kernel_size), tuple(stride), tuple(padding), tuple(dilation))

    def build():
        if x.dim() != 4:
            raise TadmmError(-1, "conv chain: x must be an NCHW image")
        if x.dtype == torch.float16 and save_ranks is not None:
            raise TadmmError(-1, "conv chain: float16 is inference only; the saved intermediates feed the weight gradients")
        B, Cc, H, W = x.shape
        d, ho, wo = _conv_chain_desc(B, Cc, H, W, n_out, w1p, w2p, w3p, bias, x.dtype, kernel_size, stride, padding, dilation)
        h = _handle(x.device)
        return d, h.lib.tadmm_ttconv_fused, h, (B, n_out, ho, wo), (w1p, w2p, w3p, bias)

    d, fn, h, yshape, _ = _memoised(key if bias_key is not None else None, build)

    shapes = [yshape]
    if save_ranks is not None:
        r1, r2 = save_ranks
        shapes += [(x.shape[0], r1, x.shape[2], x.shape[3]), (yshape[0], r2, yshape[2], yshape[3])]
    y, *saved = _out_tensors(out, shapes, x)
    d.X, d.Y = x.data_ptr(), y.data_ptr()
    if save_ranks is None:
        if yshape[0] > 0:
            h.check(fn(h.ptr, C.byref(d), _stream(x.device)))
        return y
    h1, h2 = saved
    h.check(h.lib.tadmm_ttconv_fused_save(h.ptr, C.byref(d), r1, r2, h1.data_ptr(), h2.data_ptr(), _stream(x.device)))
    return y, h1, h2


def conv_chain_save(x: torch.Tensor, w1p: torch.Tensor, w2p: torch.Tensor, w3p: torch.Tensor, bias, n_out: int, r1: int,
                    r2: int, kernel_size, stride, padding, dilation, out=None):
    """`conv_chain` that also returns its two intermediates, (y, H1 (B, r1, H, W), H2 (B, r2, Ho, Wo)), of x's dtype
    (`tadmm_ttconv_fused_save`): what the weight gradients of a training step read.  r1, r2: the true ranks.  A pixel of
    H1 that no tap of any output pixel reads is stored as zero."""
    return conv_chain(x, w1p, w2p, w3p, bias, n_out, kernel_size, stride, padding, dilation, save_ranks=(r1, r2), out=out)


def conv_chain_bwd(dy: torch.Tensor, w3tp: torch.Tensor, w2tp: torch.Tensor, w1tp: torch.Tensor, x_shape, r1: int, r2: int,
                   kernel_size, stride, padding, dilation, save: bool = False, out=None):
    """dX (x_shape) = W1^T conv^T_kxk(W3^T dY; Wc) of the one-launch factorised convolution, in one launch
    (`tadmm_ttconv_fused_bwd`; `conv_chain_bwd_fits` says where).  w3tp = weight_planes(W3.t(), P, pad_rows=32), w2tp =
    conv_core_planes(core.permute(1, 0, 2, 3), P), w1tp = weight_planes(W1.t(), P); nothing is flipped.  `save`: returns
    (dX, dH1 (B, r1, H, W), dH2 (B, r2, Ho, Wo)), the gradients of the two intermediates.  `out`: contiguous tensors to
    write instead of fresh ones -- dX, or (dX, dH1, dH2) with `save`."""
    dy = _operand(dy, "conv chain", "dy", (torch.float32, torch.bfloat16), layout="copy")
    if dy.dim() != 4:
        raise TadmmError(-1, f"conv chain: dy must be an NCHW image (got {dy.dim()}-D)")
    B, Cc, H, W = x_shape
    d, ho, wo = _conv_chain_desc(B, Cc, H, W, dy.shape[1], w3tp, w2tp, w1tp, None, dy.dtype, kernel_size, stride, padding,
                                 dilation, bwd=True)
    if tuple(dy.shape) != (B, dy.shape[1], ho, wo) or w1tp.shape[1] * 16 < Cc:
        raise TadmmError(-1, f"conv chain: dy of shape {tuple(dy.shape)} is not the output of x {tuple(x_shape)}")
    dev = dy.device
    h = _handle(dev)
    shapes = [tuple(x_shape)] + ([(B, r1, H, W), (B, r2, ho, wo)] if save else [])
    dx, dh1, dh2 = _out_tensors(out, shapes, dy) + [None] * (3 - len(shapes))
    d.X, d.Y = dy.data_ptr(), dx.data_ptr()
    h.check(h.lib.tadmm_ttconv_fused_bwd(h.ptr, C.byref(d), r1, r2, None if dh1 is None else dh1.data_ptr(),
                                         None if dh2 is None else dh2.data_ptr(), _stream(dev)))
    return (dx, dh1, dh2) if save else dx


# ------------------------------------------------------------------ k x k core convolution (csrc/coreconv.hip)
def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def _conv_out_hw(h: int, w: int, kernel_size, stride, padding, dilation):
    ho = (h + 2 * padding[0] - dilation[0] * (kernel_size[0] - 1) - 1) // stride[0] + 1
    wo = (w + 2 * padding[1] - dilation[1] * (kernel_size[1] - 1) - 1) // stride[1] + 1
    return ho, wo


def core_conv_fits(x: torch.Tensor, r2: int, kernel_size, stride, padding, dilation, groups: int = 1) -> bool:
    """True when the native core convolution (csrc/coreconv.hip) takes this call: a 4-D float32 or bfloat16 input,
    groups == 1 and a non-empty output plane.  Neither the plane's width nor a rank bounds it.  Host-only shape logic."""
    if x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16) or groups != 1 or r2 <= 0 or x.shape[1] <= 0:
        return False
    k, s, p, dl = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
    if min(k) <= 0 or min(s) <= 0 or min(dl) <= 0 or min(p) < 0 or x.shape[2] <= 0 or x.shape[3] <= 0:
        return False
    ho, wo = _conv_out_hw(x.shape[2], x.shape[3], k, s, p, dl)
    return ho > 0 and wo > 0


def core_conv_pays(x: torch.Tensor, r2: int, kernel_size, stride, padding, dilation, groups: int = 1,
                   training: bool = False) -> bool:
    """True when the layers route their k x k core convolution to `core_conv` instead of the device library's conv2d:
    bfloat16 inference only.  Measured (scripts/bench_core_conv.py) on the 30 distinct 3 x 3 core
    shapes of resnet18_tt 2x, resnet50_tt 3x, tk_resnet50 3x and tk_resnet32 3x: the bf16 forward is ahead of the library
    beyond its round-to-round spread at all 30 (1.05x - 3.6x).  The fp32 forward (three planes, six MFMA products per
    product) is ahead at 5, inside the spread at 4 and behind at 21 (0.46x - 1.9x) with no shape class that separates
    them, and forward + backward (`training`: something the convolution reads wants a gradient) is behind at all 30 in
    both dtypes (0.28x - 0.96x: the element-load tap-shifted weight gradient and the zero rows of the strided data
    gradient): both keep the library."""
    if not core_conv_fits(x, r2, kernel_size, stride, padding, dilation, groups):
        return False
    return x.dtype == torch.bfloat16 and not training


def _core_conv_desc(x_shape, r2: int, dtype, kernel_size, stride, padding, dilation):
    B, r1, H, W = x_shape
    k, s, p, dl = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
    d = _cabi.CoreConvDesc()
    d.dtype = _cabi.CHAIN_F32 if dtype == torch.float32 else _cabi.CHAIN_BF16
    d.B, d.R1, d.R2, d.H, d.W = B, r1, r2, H, W
    d.Ho, d.Wo = _conv_out_hw(H, W, k, s, p, dl)
    d.kh, d.kw, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = k + s + p + dl
    return d


def _core_conv_call(entry: str, src: torch.Tensor, planes: torch.Tensor, x_shape, r2: int, kernel_size, stride, padding,
                    dilation, memo: bool):
    """Forward (src = x, result y) or data gradient (src = dy, result dx) of the core convolution on x_shape inputs."""
    src = _operand(src, "core conv", "the image", (torch.float32, torch.bfloat16), layout="copy")
    if src.dim() != 4:
        raise TadmmError(-1, f"core conv: an NCHW image is needed (got {src.dim()}-D)")
    fwd = entry == "tadmm_core_conv_fwd"
    key = (entry, tuple(x_shape), r2, src.dtype, src.device, planes.data_ptr(), _pair(kernel_size), _pair(stride),
           _pair(padding), _pair(dilation))

    def build():
        d = _core_conv_desc(x_shape, r2, src.dtype, kernel_size, stride, padding, dilation)
        rows, cols = (r2, x_shape[1]) if fwd else (x_shape[1], r2)
        _check_planes(planes, 3 if src.dtype == torch.float32 else 1, torch.bfloat16, "core conv")
        if planes.shape[1] * 16 < rows or planes.shape[2] != d.kh * d.kw * -(-cols // 32):
            raise TadmmError(-1, "core conv: weight planes do not match the tap-major core (ops.conv_core_planes)")
        if d.Ho <= 0 or d.Wo <= 0:
            raise TadmmError(-1, "core conv: empty output plane")
        d.Wc, d.wc_plane = planes.data_ptr(), planes[0].numel()
        h = _handle(src.device)
        return d, getattr(h.lib, entry), h, (x_shape[0], r2, d.Ho, d.Wo), planes     # the tuple keeps the planes alive

    d, fn, h, y_shape, _ = _memoised(key if memo else None, build)
    if tuple(src.shape) != (tuple(x_shape) if fwd else y_shape):
        raise TadmmError(-1, f"core conv: operand of shape {tuple(src.shape)} does not match the geometry")
    out = torch.empty(y_shape if fwd else tuple(x_shape), dtype=src.dtype, device=src.device)
    if fwd:
        d.X, d.Y = src.data_ptr(), out.data_ptr()
    else:
        d.X, d.Y = out.data_ptr(), src.data_ptr()
    if x_shape[0] > 0:
        h.check(fn(h.ptr, C.byref(d), _stream(src.device)))
    return out


def core_conv(x: torch.Tensor, planes: torch.Tensor, r2: int, kernel_size, stride=1, padding=0, dilation=1,
              memo: bool = True) -> torch.Tensor:
    """y (B, r2, Ho, Wo) = conv2d(x (B, r1, H, W), core) with groups = 1, `planes = conv_core_planes(core, P)` (P = 3 for
    float32, 1 for bfloat16): `tadmm_core_conv_fwd`, NCHW in place, any plane size and any rank."""
    if isinstance(x, torch.Tensor) and x.dim() != 4:
        raise TadmmError(-1, "core conv: x must be an NCHW image")
    return _core_conv_call("tadmm_core_conv_fwd", x, planes, tuple(x.shape), r2, kernel_size, stride, padding, dilation, memo)


def core_conv_dgrad(dy: torch.Tensor, planes_t: torch.Tensor, x_shape, kernel_size, stride=1, padding=0, dilation=1,
                    memo: bool = True) -> torch.Tensor:
    """dx (x_shape) of `core_conv` from dy (B, r2, Ho, Wo); `planes_t = conv_core_planes(core.permute(1, 0, 2, 3), P)` --
    the kernel's transposed gather maps the taps, nothing is flipped (`tadmm_core_conv_dgrad`)."""
    r2 = dy.shape[1] if isinstance(dy, torch.Tensor) and dy.dim() == 4 else 0
    return _core_conv_call("tadmm_core_conv_dgrad", dy, planes_t, tuple(x_shape), r2, kernel_size, stride, padding,
                           dilation, memo)


def _core_wgrad_operands(dy, x, kernel_size, stride, padding, dilation):
    for t, what in ((dy, "dy"), (x, "x")):
        _operand(t, "core conv wgrad", what, layout=None)
    if dy.dtype != x.dtype or x.dtype not in (torch.float32, torch.bfloat16) or dy.dim() != 4 or x.dim() != 4:
        raise TadmmError(-1, f"core conv wgrad: two NCHW images of one dtype, float32 or bfloat16 (got {dy.dtype}, {x.dtype})")
    if dy.device != x.device:
        raise TadmmError(-1, f"core conv wgrad: operands on different devices ({dy.device}, {x.device})")
    d = _core_conv_desc(tuple(x.shape), dy.shape[1], x.dtype, kernel_size, stride, padding, dilation)
    if tuple(dy.shape) != (x.shape[0], dy.shape[1], d.Ho, d.Wo) or d.Ho <= 0 or d.Wo <= 0:
        raise TadmmError(-1, f"core conv wgrad: dy of shape {tuple(dy.shape)} is not the output of x {tuple(x.shape)}")
    dy = dy if dy.is_contiguous() else dy.contiguous()
    x = x if x.is_contiguous() else x.contiguous()
    d.X, d.Y = x.data_ptr(), dy.data_ptr()
    return dy, x, d


def core_conv_wgrad_plan(dy: torch.Tensor, x: torch.Tensor, kernel_size, stride=1, padding=0, dilation=1):
    """(workspace bytes, slices) `core_conv_wgrad` will use: a pure function of the shapes."""
    dy, x, d = _core_wgrad_operands(dy, x, kernel_size, stride, padding, dilation)
    nbytes, slices = C.c_size_t(), C.c_int()
    rc = _cabi.load().tadmm_core_conv_wgrad_workspace_bytes(C.byref(d), C.byref(nbytes), C.byref(slices))
    if rc < 0:
        raise TadmmError(rc, "tadmm_core_conv_wgrad_workspace_bytes: the launch does not take this shape")
    return nbytes.value, slices.value


def core_conv_wgrad(dy: torch.Tensor, x: torch.Tensor, kernel_size, stride=1, padding=0, dilation=1,
                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW (r2, r1, kh, kw) float32 of `core_conv` from dy (B, r2, Ho, Wo) and x (B, r1, H, W), both read in place
    (`tadmm_core_conv_wgrad`): split over (batch, output pixel), deterministic.  `workspace`: a uint8 device tensor of at
    least `core_conv_wgrad_plan(...)[0]` bytes to use instead of a fresh one."""
    dy, x, d = _core_wgrad_operands(dy, x, kernel_size, stride, padding, dilation)
    out = torch.empty(d.R2, d.R1, d.kh, d.kw, dtype=torch.float32, device=x.device)
    if out.numel() == 0:
        return out
    dev = x.device
    h = _handle(dev)
    nbytes = C.c_size_t()
    h.check(h.lib.tadmm_core_conv_wgrad_workspace_bytes(C.byref(d), C.byref(nbytes), None))
    ws = workspace
    if ws is None and nbytes.value:
        ws = _scratch(nbytes.value, dev)
    h.check(h.lib.tadmm_core_conv_wgrad(h.ptr, C.byref(d), out.data_ptr(), None if ws is None else ws.data_ptr(),
                                        0 if ws is None else ws.numel() * ws.element_size(), _stream(dev)))
    return out


# ------------------------------------------------------------------ Gram / eigh (tests, Tucker)
def gram(a: torch.Tensor):
    """fp64 Gram of a float32 (m,n) matrix: A A^T if m<=n else A^T A.  Returns (N,N) float64."""
    _operand(a, "", "A", (torch.float32,))
    h = _handle(a.device)
    lib = h.lib
    m, n = a.shape
    npad, ld = C.c_int(), C.c_int()
    N = lib.tadmm_gram_ld(m, n, C.byref(npad), C.byref(ld))
    G = torch.empty(npad.value, ld.value, dtype=torch.float64, device=a.device)
    scratch = _scratch(lib.tadmm_gram_scratch_bytes(m, n), a.device)
    h.check(lib.tadmm_gram_f64(h.ptr, a.data_ptr(), m, n, G.data_ptr(), ld.value, scratch.data_ptr(), scratch.numel(),
                               _stream(a.device)))
    return G[:N, :N]


def _eigh(G: torch.Tensor, r: Optional[int]):
    """The full solve (r None: N pairs, third result the sweeps) or the leading r pairs (third result the route)."""
    assert G.dtype == torch.float64 and G.is_cuda and G.dim() == 2 and G.shape[0] == G.shape[1]
    G = G.contiguous()
    h = _handle(G.device)
    N = G.shape[0]
    rows = N if r is None else max(r, 1)
    ev = torch.empty(rows, dtype=torch.float64, device=G.device)
    vec = torch.empty(rows, N, dtype=torch.float64, device=G.device)
    scratch = _scratch(h.lib.tadmm_eigh_scratch_bytes(N), G.device)
    info = C.c_int(0 if r is None else -1)
    tail = (ev.data_ptr(), vec.data_ptr(), scratch.data_ptr(), scratch.numel(), C.byref(info), _stream(G.device))
    if r is None:
        h.check(h.lib.tadmm_eigh_f64(h.ptr, G.data_ptr(), N, *tail))
    else:
        h.check(h.lib.tadmm_eigh_partial_f64(h.ptr, G.data_ptr(), N, int(r), *tail))
    return ev, vec, int(info.value)


def eigh(G: torch.Tensor):
    """Symmetric PSD eigen-decomposition (descending).  Returns (evals (N,), evecs (N,N) rows, sweeps)."""
    return _eigh(G, None)


def eigh_partial(G: torch.Tensor, r: int):
    """Leading r pairs of a symmetric PSD G (descending), as the plans solve them.  Returns (evals (r,),
    evecs (r,N) rows, route): route 0 = direct solver, 1 = single-launch Jacobi, 2 = Jacobi tournament."""
    return _eigh(G, r)


# ------------------------------------------------------------------ filtered eigen-solver building blocks (tests)
def dgemm(a: torch.Tensor, b: torch.Tensor, b_transposed: bool = True) -> torch.Tensor:
    """fp64 matrix-core GEMM: a (M,K) @ b^T with b (N,K) (b_transposed) or a @ b with b (K,N); row-major float64."""
    assert a.dtype == torch.float64 and b.dtype == torch.float64 and a.is_cuda and b.is_cuda
    a, b = a.contiguous(), b.contiguous()
    M, K = a.shape
    N = b.shape[0] if b_transposed else b.shape[1]
    out = torch.empty(M, N, dtype=torch.float64, device=a.device)
    h = _handle(a.device)
    scratch = _scratch(h.lib.tadmm_dgemm_scratch_bytes(M, N), a.device)
    h.check(h.lib.tadmm_dgemm_f64(h.ptr, a.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K, a.stride(0), b.stride(0),
                                  N, int(b_transposed), scratch.data_ptr(), scratch.numel(), _stream(a.device)))
    return out


def dgemm_tile_probs(probs):
    """The C array of `tadmm_dgemm_tile_prob` for a list of dicts (tests).  Keys: A, B, C, P, Q, rot, coef, theta,
    rowpart, gate (device tensors or None; of A, B, C, P the data pointer and of A, B, C the row stride are taken),
    ring (three tensors shaped like C), selA .. selQ (default -1), M, N, K, mode, gate_min, and lda / ldb / ldc where no
    tensor gives them."""
    from ._cabi import DgemmTileProb
    arr = (DgemmTileProb * len(probs))()
    ptr = lambda t: None if t is None else t.data_ptr()
    for q, p in zip(arr, probs):
        ring = p.get("ring")
        for name in ("A", "B", "C", "P", "Q", "rot", "coef", "theta", "rowpart", "gate"):
            setattr(q, name, ptr(p.get(name)))
        if ring is not None:
            q.ring[0], q.ring[1], q.ring[2] = (t.data_ptr() for t in ring)
        for name in ("selA", "selB", "selC", "selP", "selQ"):
            setattr(q, name, int(p.get(name, -1)))
        q.M, q.N, q.K, q.mode, q.gate_min = int(p["M"]), int(p["N"]), int(p["K"]), int(p.get("mode", 0)), int(p.get("gate_min", 0))
        for ld, name, sel in (("lda", "A", "selA"), ("ldb", "B", "selB"), ("ldc", "C", "selC")):
            t = p.get(name) if p.get(sel, -1) < 0 else ring[0]
            setattr(q, ld, int(p[ld]) if ld in p else (0 if t is None else t.stride(0)))
    return arr


def dgemm_tile(probs, tile_m: int, tile_n: int, axpby: bool = False, device=None) -> None:
    """One grouped launch of the filter's NT tile product (or of its daxpby) on `probs` (see `dgemm_tile_probs`), with
    (tile_m, tile_n) = (32, 32), (64, 32) or (64, 64); results land in the tensors the problems name.  For tests."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    arr = dgemm_tile_probs(probs)
    h = _handle(device)
    scratch = _scratch(max(256, h.lib.tadmm_dgemm_tile_scratch_bytes(len(probs), arr)), device)
    h.check(h.lib.tadmm_dgemm_tile_f64(h.ptr, len(probs), arr, tile_m, tile_n, int(axpby), scratch.data_ptr(),
                                       scratch.numel(), _stream(device)))


def tile_map(probs):
    """The block map of one grouped tile product on `probs`, a list of (M, N, K, tile_m, tile_n), as the filter and
    `dgemm_tile` build it (csrc/host.h `tile_map_build`): a list of (prob, local), position i expected on XCD i % 8,
    with the modelled operand bytes of that map and of the problem-major order.  Host only, no device."""
    import ctypes as C
    from . import _cabi
    lib = _cabi.load()
    arr = (_cabi.TileMapProb * len(probs))(*[_cabi.TileMapProb(*map(int, p)) for p in probs])
    n = lib.tadmm_tile_map(len(probs), arr, None, 0, None)
    if n < 0:
        raise ValueError(f"tadmm_tile_map refuses {probs!r}: status {n}")
    out = (C.c_int32 * (2 * n))()
    cost = (C.c_double * 2)()
    got = lib.tadmm_tile_map(len(probs), arr, out, n, cost)
    assert got == n, (got, n)
    return [(out[2 * i], out[2 * i + 1]) for i in range(n)], float(cost[0]), float(cost[1])


def dgemm3(a: torch.Tensor, g: torch.Tensor, repeats: int = 1) -> torch.Tensor:
    """a (M, N) @ g (N, N)^T at fp32 accuracy on the bf16 matrix cores (float64 in / out): the product the early
    stages of the filtered eigen-solver use (csrc/dgemm3.hip)."""
    assert a.dtype == torch.float64 and g.dtype == torch.float64 and a.is_cuda and g.is_cuda
    assert a.is_contiguous() and g.is_contiguous() and g.shape[0] == g.shape[1] == a.shape[1]
    M, N = a.shape
    h = _handle(a.device)
    out = torch.empty(M, N, dtype=torch.float64, device=a.device)
    scratch = _scratch(h.lib.tadmm_dgemm3_scratch_bytes(M, N), a.device)
    h.check(h.lib.tadmm_dgemm3_f64(h.ptr, a.data_ptr(), g.data_ptr(), out.data_ptr(), M, N, N, N, N, repeats,
                                   scratch.data_ptr(), scratch.numel(), _stream(a.device)))
    return out


def cholqr_(yt: torch.Tensor) -> bool:
    """In-place Cholesky QR of the block whose columns are the ROWS of yt (n, ncols) float64.  Returns False when a
    pivot broke down (numerically rank-deficient block)."""
    assert yt.dtype == torch.float64 and yt.is_cuda and yt.is_contiguous()
    n, ncols = yt.shape
    h = _handle(yt.device)
    scratch = _scratch(h.lib.tadmm_cholqr_scratch_bytes(n, ncols), yt.device)
    bad = C.c_int(0)
    h.check(h.lib.tadmm_cholqr_f64(h.ptr, yt.data_ptr(), n, ncols, yt.stride(0), scratch.data_ptr(), scratch.numel(),
                                   C.byref(bad), _stream(yt.device)))
    return bad.value == 0


# ------------------------------------------------------------------ Stiefel manifold (csrc/stiefel.hip)
STIEFEL_LDS_BYTES = 160 * 1024
STIEFEL_PIVOT_FLOOR = 4e-14      # kStfPivotFloor of csrc/stiefel.hip
STIEFEL_SECOND_PASS = 1e4       # kStfSecondPass: pivot spread above which the kernel runs a second Cholesky-QR pass


def _align16(v: int) -> int:
    return (v + 15) & ~15


def stiefel_lds_bytes(n: int, p: int) -> int:
    """LDS of the resident step for one n x p factor, as csrc/stiefel.hip sizes it: three fp32 tiles and two fp64 p x p
    matrices at a row pitch of p|1, two fp64 p-vectors, each carve rounded up to 16 bytes."""
    pitch = p | 1
    return 3 * _align16(n * pitch * 4) + 2 * _align16(p * pitch * 8) + 2 * _align16(p * 8)


def stiefel_fits(n: int, p: int) -> bool:
    """True when an n x p factor takes the one-launch LDS-resident route (64 x 64 and 123 x 64 do, 124 x 64 does not);
    the others take the composed device route of `StiefelPlan`.  Pure host logic."""
    return 1 <= p <= n and p <= 128 and stiefel_lds_bytes(n, p) <= STIEFEL_LDS_BYTES


def stiefel_desc(x: torch.Tensor, g: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None) -> StiefelDesc:
    """`tadmm_stiefel_desc` of a factor, its gradient and its momentum buffer (either may be None).  Host only: raises,
    before anything is launched, for a factor that is not a float32 row-major n x p matrix with n >= p, and for a
    gradient or buffer that is not laid out like the factor."""
    if x.dim() != 2:
        raise TadmmError(-1, f"a Stiefel factor is a matrix (got shape {tuple(x.shape)})")
    n, p = int(x.shape[0]), int(x.shape[1])
    if p < 1 or n < p:
        raise TadmmError(-1, f"a Stiefel factor is n x p with n >= p >= 1 (got {n} x {p})")
    ld = int(x.stride(0)) if n > 1 else max(int(x.stride(0)), p)
    for what, t in (("factor", x), ("gradient", g), ("momentum buffer", m)):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise TadmmError(-1, f"the Stiefel {what} must be float32 (got {t.dtype})")
        if tuple(t.shape) != (n, p) or t.device != x.device:
            raise TadmmError(-1, f"the Stiefel {what} must match its {n} x {p} factor on {x.device} "
                                 f"(got {tuple(t.shape)} on {t.device})")
        if (p > 1 and t.stride(1) != 1) or (n > 1 and (t.stride(0) < p or t.stride(0) != ld)):
            raise TadmmError(-1, f"the Stiefel {what} must be stored row-major with the factor's row stride {ld} "
                                 f"(strides {tuple(t.stride())})")
    d = StiefelDesc()
    d.X = x.data_ptr()
    d.G = g.data_ptr() if g is not None else None
    d.M = m.data_ptr() if m is not None else None
    d.rows, d.cols, d.ld = n, p, ld
    return d


def _sym(a: torch.Tensor) -> torch.Tensor:
    return 0.5 * (a + a.t())


def _cholqr_composed(y: torch.Tensor):
    """Q factor (positive diagonal of R) of a float64 device matrix by two Cholesky-QR passes of library calls; returns
    (Q, ok) with ok a 0-dim bool tensor -- nothing synchronises."""
    ok = None
    for _ in range(2):
        s = y.t() @ y
        l, info = torch.linalg.cholesky_ex(s)                                # Y^T Y = L L^T, R = L^T
        y = torch.linalg.solve_triangular(l, y.t(), upper=False).t()         # Y R^-1 = (L^-1 Y^T)^T
        # the kernel's rule: every squared pivot above STIEFEL_PIVOT_FLOOR times its column's squared norm, and finite
        floor = (torch.diagonal(l) ** 2 > STIEFEL_PIVOT_FLOOR * torch.diagonal(s)).all()
        good = (info == 0) & floor & torch.isfinite(y).all()
        ok = good if ok is None else ok & good
    return y, ok


class StiefelPlan:
    """One set of Stiefel factors updated together (`tadmm_stiefel_plan`): `factors` is a list of (X, G, M) float32
    row-major device matrices, G and M laid out like X or None (G None: the factor is skipped by `step` and `adam_step`;
    M None: only with momentum == 0 and for `project_`).  The factors that fit the LDS (`stiefel_fits`) go through ONE native launch
    per call; the others take the composed device route, a few float64 library calls per factor (products,
    `torch.linalg.cholesky_ex`, `solve_triangular`) with the same arithmetic.  Neither route synchronises: a factor whose
    Cholesky pivot broke down keeps X and M and has its word of `status` (int32, sticky) set; `failed()` reads them.
    Both routes refuse a factor by the same rule (a squared pivot not above 4e-14 times its column's squared norm, or a
    non-finite value); the composed route always runs two Cholesky-QR passes where the kernel runs the second only for
    a pivot spread above 1e4, so the two agree to fp32 rounding, not bit for bit.
    `native=False` sends every factor through the composed route (the comparator of scripts/bench_stiefel.py)."""

    def __init__(self, factors: Sequence, native: bool = True):
        if not factors:
            raise TadmmError(-1, "StiefelPlan: no factors")
        dev = factors[0][0].device
        if dev.type != "cuda":
            raise TadmmError(-1, f"Stiefel factors must live on a HIP device (got {dev}); there is no CPU path")
        descs = []
        for x, g, m in factors:
            if x.device != dev:
                raise TadmmError(-1, f"Stiefel factors of one plan share a device (got {x.device} and {dev})")
            descs.append(stiefel_desc(x, g, m))
        self.device = dev
        self.factors = [tuple(f) for f in factors]
        self.native = [i for i, d in enumerate(descs) if native and stiefel_fits(d.rows, d.cols)]
        self.composed = [i for i in range(len(descs)) if i not in set(self.native)]
        self.order = self.native + self.composed                  # status word k belongs to factor order[k]
        self.status = torch.zeros(len(descs), dtype=torch.int32, device=dev)
        self._plan = None
        if self.native:
            self.h = _handle(dev)
            lib = self.h.lib
            n = len(self.native)
            arr = (StiefelDesc * n)(*[descs[i] for i in self.native])
            size = C.c_size_t()
            self.h.check(lib.tadmm_stiefel_workspace_bytes(n, arr, C.byref(size)))
            self.workspace = _scratch(size.value, dev)
            plan = C.c_void_p()
            self.h.check(lib.tadmm_stiefel_plan_create(self.h.ptr, n, arr, self.workspace.data_ptr(), int(size.value),
                                                       _stream(dev), C.byref(plan)))
            self._plan = plan
            self._fin = weakref.finalize(self, lib.tadmm_stiefel_plan_destroy, plan)

    def _touched(self, with_m: bool, skipped_too: bool):
        # the launches write through raw pointers: tell autograd and the layers' inference caches (`param_key`);
        # a factor skipped for a null G was not written and keeps its caches
        for x, g, m in self.factors:
            if g is None and not skipped_too:
                continue
            torch.autograd.graph.increment_version(x)
            if with_m and m is not None:
                torch.autograd.graph.increment_version(m)

    def step(self, lr: float, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
             nesterov: bool = False):
        if momentum < 0:
            raise TadmmError(-1, f"Stiefel step: momentum {momentum} < 0")
        if momentum > 0 and any(m is None for _, _, m in self.factors):
            raise TadmmError(-1, "Stiefel step: momentum > 0 needs a momentum buffer for every factor")
        if self._plan is not None:
            self.h.check(self.h.lib.tadmm_stiefel_step(self._plan, float(lr), float(momentum), float(dampening),
                                                       float(weight_decay), int(bool(nesterov)), self.status.data_ptr(),
                                                       _stream(self.device)))
        with torch.no_grad():
            for k, i in enumerate(self.composed, start=len(self.native)):
                x, g, m = self.factors[i]
                if g is None:
                    continue
                x64 = x.double()
                g64 = g.double() + weight_decay * x64
                r = g64 - x64 @ _sym(x64.t() @ g64)
                if momentum > 0:
                    m64 = momentum * m.double() + (1.0 - dampening) * r
                    d = r + momentum * m64 if nesterov else m64
                else:
                    d = r
                q, ok = _cholqr_composed(x64 - lr * d)
                if momentum > 0:
                    m64 = m64 - q @ _sym(q.t() @ m64)
                    ok = ok & torch.isfinite(m64).all()
                    m.copy_(torch.where(ok, m64.float(), m))
                x.copy_(torch.where(ok, q.float(), x))
                self.status[k:k + 1] |= (~ok).to(torch.int32)
        self._touched(momentum > 0, False)

    def adam_step(self, lr: float, betas, eps: float, weight_decay: float, amsgrad: bool, v: torch.Tensor,
                  vmax: Optional[torch.Tensor], steps: torch.Tensor):
        """One Riemannian Adam step (`tadmm_stiefel_adam_step`): M of every factor is `exp_avg`; `v` (float32, the second
        moment, ONE number per factor), `vmax` (float32, its running maximum; needed with amsgrad only) and `steps` (int32
        counters) are contiguous 1-D device tensors with one entry per factor in the order of `order` -- entry k belongs
        to factor `order[k]`, as the status words do (`slot_of`).  A skipped (G None) or failed factor keeps X, M and its
        three entries.  The composed route computes the same arithmetic with float64 library calls."""
        b1, b2 = float(betas[0]), float(betas[1])
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise TadmmError(-1, f"Stiefel Adam step: betas {tuple(betas)} outside [0, 1)")
        if not (eps >= 0 and lr >= 0 and weight_decay >= 0):
            raise TadmmError(-1, f"Stiefel Adam step: eps {eps}, lr {lr}, weight_decay {weight_decay} must not be negative")
        if any(m is None for _, _, m in self.factors):
            raise TadmmError(-1, "Stiefel Adam step: every factor needs M (exp_avg)")
        n = len(self.factors)
        for what, t, dt in (("v", v, torch.float32), ("vmax", vmax, torch.float32), ("steps", steps, torch.int32)):
            if t is None and what == "vmax" and not amsgrad:
                continue
            if t is None or t.dtype != dt or t.device != self.device or t.dim() != 1 or t.numel() != n \
                    or not t.is_contiguous():
                raise TadmmError(-1, f"Stiefel Adam step: {what} must be a contiguous 1-D {dt} tensor of {n} entries on "
                                     f"{self.device}")
        if not amsgrad:
            vmax = None
        if self._plan is not None:
            self.h.check(self.h.lib.tadmm_stiefel_adam_step(
                self._plan, float(lr), b1, b2, float(eps), float(weight_decay), int(bool(amsgrad)), v.data_ptr(),
                vmax.data_ptr() if vmax is not None else None, steps.data_ptr(), self.status.data_ptr(),
                _stream(self.device)))
        with torch.no_grad():
            for k, i in enumerate(self.composed, start=len(self.native)):
                x, g, m = self.factors[i]
                if g is None:
                    continue
                x64 = x.double()
                g64 = g.double() + weight_decay * x64
                r = g64 - x64 @ _sym(x64.t() @ g64)
                m64 = b1 * m.double() + (1.0 - b1) * r
                t_new = steps[k] + 1
                v_new = b2 * v[k].double() + (1.0 - b2) * (r * r).sum()
                top = torch.maximum(vmax[k].double(), v_new) if amsgrad else v_new
                tf = t_new.double()
                scale = lr / ((1.0 - b1 ** tf) * (torch.sqrt(top / (1.0 - b2 ** tf)) + eps))
                q, ok = _cholqr_composed(x64 - scale * m64)
                m64 = m64 - q @ _sym(q.t() @ m64)
                ok = ok & torch.isfinite(m64).all() & torch.isfinite(v_new)
                m.copy_(torch.where(ok, m64.float(), m))
                x.copy_(torch.where(ok, q.float(), x))
                v[k:k + 1] = torch.where(ok, v_new.float(), v[k])
                if amsgrad:
                    vmax[k:k + 1] = torch.where(ok, top.float(), vmax[k])
                steps[k:k + 1] = torch.where(ok, t_new, steps[k])
                self.status[k:k + 1] |= (~ok).to(torch.int32)
        self._touched(True, False)
        for t in (v, vmax, steps):
            if t is not None:
                torch.autograd.graph.increment_version(t)

    def slot_of(self, i: int) -> int:
        """The position of factor i in the status words and in the per-factor state arrays of `adam_step`."""
        return self.order.index(i)

    def project_(self):
        """Replaces every X by the Q factor (positive diagonal of R) of its QR decomposition."""
        if self._plan is not None:
            self.h.check(self.h.lib.tadmm_stiefel_project(self._plan, self.status.data_ptr(), _stream(self.device)))
        with torch.no_grad():
            for k, i in enumerate(self.composed, start=len(self.native)):
                x = self.factors[i][0]
                q, ok = _cholqr_composed(x.double())
                x.copy_(torch.where(ok, q.float(), x))
                self.status[k:k + 1] |= (~ok).to(torch.int32)
        self._touched(False, True)

    def status_of(self, i: int) -> torch.Tensor:
        """The status word of factor i as a one-element device view (no synchronisation)."""
        k = self.slot_of(i)
        return self.status[k:k + 1]

    def failed(self) -> List[int]:
        """Indices (into `factors`) of the factors whose status word is set; one synchronisation."""
        flags = self.status.cpu().tolist()
        return sorted(self.order[k] for k, f in enumerate(flags) if f)


def stiefel_step(factors: Sequence, lr: float, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False) -> StiefelPlan:
    """One Riemannian SGD step on a list of (X, G, M) (see `StiefelPlan`), in place; returns the plan, whose `failed()`
    names the factors that were left untouched.  Callers that step repeatedly keep a `StiefelPlan` (and use its
    `adam_step` for Riemannian Adam)."""
    plan = StiefelPlan(factors)
    plan.step(lr, momentum, dampening, weight_decay, nesterov)
    return plan


def stiefel_project_(*xs: torch.Tensor) -> StiefelPlan:
    """Puts every given matrix on the Stiefel manifold in place (Q factor of its QR decomposition, diag(R) > 0)."""
    plan = StiefelPlan([(x, None, None) for x in xs])
    plan.project_()
    return plan


# ------------------------------------------------------------------ BertAdam (csrc/bertadam.hip)
BERTADAM_CHUNK = _cabi.BERTADAM_CHUNK      # elements one workgroup takes at a time; a chunk never spans two tensors


def bert_adam_native(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor) -> bool:
    """True when (p, g, m, v) can go into a `BertAdamPlan`: float32, dense-contiguous, on one HIP device, of one shape.
    Everything else takes `bert_adam_composed`.  Pure host logic."""
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and not t.is_sparse
               and t.is_contiguous() and t.numel() > 0 and t.shape == p.shape and t.device == p.device
               for t in (p, g, m, v))


class BertAdamPlan:
    """One set of tensors stepped together by the reference's BertAdam rule (`tadmm_bertadam_plan`): `tensors` is a list
    of (p, g, m, v), float32 dense-contiguous device tensors of one shape each (`bert_adam_native`; 4-byte alignment is
    enough, 16-byte aligned tensors take 16-byte accesses).  `step` is two launches for the whole list (one without
    clipping), copies nothing and never synchronises; g is left as it was.  The table is uploaded once, here."""

    def __init__(self, tensors: Sequence):
        if not tensors:
            raise TadmmError(-1, "BertAdamPlan: no tensors")
        dev = tensors[0][0].device
        if dev.type != "cuda":
            raise TadmmError(-1, f"BertAdamPlan tensors must live on a HIP device (got {dev}); use bert_adam_composed")
        n = len(tensors)
        arr = (_cabi.BertAdamDesc * n)()
        for i, (p, g, m, v) in enumerate(tensors):
            if not bert_adam_native(p, g, m, v) or p.device != dev:
                raise TadmmError(-1, f"BertAdamPlan tensor {i}: p, g, m and v must be float32 dense-contiguous tensors of "
                                     f"one shape on {dev}; everything else takes bert_adam_composed")
            arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), \
                p.numel()
        self.device = dev
        self.tensors = [tuple(t) for t in tensors]
        self._written = [t for p, _, m, v in self.tensors for t in (p, m, v)]
        self.h = _handle(dev)
        lib = self.h.lib
        size = C.c_size_t()
        self.h.check(lib.tadmm_bertadam_workspace_bytes(n, arr, C.byref(size)))
        self.workspace = _scratch(size.value, dev)
        plan = C.c_void_p()
        self.h.check(lib.tadmm_bertadam_plan_create(self.h.ptr, n, arr, self.workspace.data_ptr(), int(size.value),
                                                    _stream(dev), C.byref(plan)))
        self._plan = plan
        self._fin = weakref.finalize(self, lib.tadmm_bertadam_plan_destroy, plan)
        ptr = C.c_void_p()
        self.h.check(lib.tadmm_bertadam_norms(plan, C.byref(ptr)))
        off = ptr.value - self.workspace.data_ptr()
        self._norms = self.workspace[off:off + 8 * n].view(torch.float64)

    def step(self, lr: float, b1: float = 0.9, b2: float = 0.999, e: float = 1e-6, weight_decay: float = 0.01,
             max_grad_norm: float = 1.0):
        """c = min(1, max_grad_norm / (||g|| + 1e-6)) per tensor (1 with max_grad_norm <= 0); gc = g c;
        m <- b1 m + (1-b1) gc;  v <- b2 v + (1-b2) gc^2;  p <- p - lr (m / (sqrt(v) + e) + weight_decay p).
        b1 or b2 outside [0, 1), e < 0 and lr < 0 are refused by the library before anything is launched."""
        self.h.check(self.h.lib.tadmm_bertadam_step(self._plan, float(lr), float(b1), float(b2), float(e),
                                                    float(weight_decay), float(max_grad_norm), _stream(self.device)))
        self._touched()

    def _touched(self):
        # the launches write through raw pointers: tell autograd and the layers' inference caches (`param_key`)
        torch.autograd.graph.increment_version(self._written)

    def grad_norms(self) -> torch.Tensor:
        """Every tensor's gradient norm as the last step with max_grad_norm > 0 computed it (zeros before the first): a
        float64 device tensor, a view of the plan's workspace that the next such step overwrites.  No synchronisation."""
        return self._norms


def bert_adam_composed(ps: Sequence[torch.Tensor], gs: Sequence[torch.Tensor], ms: Sequence[torch.Tensor],
                       vs: Sequence[torch.Tensor], lr: float, b1: float = 0.9, b2: float = 0.999, e: float = 1e-6,
                       weight_decay: float = 0.01, max_grad_norm: float = 1.0):
    """The arithmetic of `BertAdamPlan.step` on `torch._foreach_*` calls, in the tensors' own dtype, in place on ps, ms
    and vs (gs untouched): the route of everything the kernel does not take (other dtypes, non-contiguous parameters,
    CPU tensors) and its CPU-testable twin.  Returns the list of gradient norms (0-dim tensors), or None without
    clipping.  Sparse gradients raise, as in the reference."""
    ps, gs, ms, vs = list(ps), list(gs), list(ms), list(vs)
    if any(g.is_sparse for g in gs):
        raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
    if not ps:
        return None
    norms = None
    with torch.no_grad():
        if max_grad_norm > 0:
            norms = torch._foreach_norm(gs)
            coef = torch._foreach_add(norms, 1e-6)
            torch._foreach_reciprocal_(coef)
            torch._foreach_mul_(coef, float(max_grad_norm))
            torch._foreach_clamp_max_(coef, 1.0)
            gs = torch._foreach_mul(gs, coef)
        torch._foreach_mul_(ms, b1)
        torch._foreach_add_(ms, gs, alpha=1.0 - b1)
        torch._foreach_mul_(vs, b2)
        torch._foreach_addcmul_(vs, gs, gs, value=1.0 - b2)
        upd = torch._foreach_sqrt(vs)
        torch._foreach_add_(upd, e)
        upd = torch._foreach_div(ms, upd)
        if weight_decay > 0:
            torch._foreach_add_(upd, ps, alpha=weight_decay)
        torch._foreach_add_(ps, upd, alpha=-lr)
    return norms


# ------------------------------------------------------------------ gathered TT-matrix chain (csrc/ttm_gather.hip)
TTM_MAX_D = _cabi.TTM_MAX_D
TTM_LDS_BYTES = 160 * 1024


def ttm_core_shapes(cores: Sequence[torch.Tensor]):
    """(n, m, r) of a chain of cores (r_k, n_k, m_k, r_{k+1}).  Host only; ValueError for an empty chain, a core that is
    not 4-D, ranks that do not chain, or r_0 != 1."""
    if len(cores) == 0:
        raise ValueError("ttm_gather: at least one core (d = 0 has no index to split)")
    n, m, r = [], [], []
    for k, c in enumerate(cores):
        if c.dim() != 4:
            raise ValueError(f"ttm_gather: core {k} must be (r, n, m, r') (got shape {tuple(c.shape)})")
        if k and int(c.shape[0]) != r[-1]:
            raise ValueError(f"ttm_gather: core {k} has left rank {int(c.shape[0])}, "
                             f"core {k - 1} has right rank {r[-1]}")
        if not k:
            r.append(int(c.shape[0]))
        n.append(int(c.shape[1]))
        m.append(int(c.shape[2]))
        r.append(int(c.shape[3]))
    if r[0] != 1:
        raise ValueError(f"ttm_gather: r_0 must be 1 (got {r[0]})")
    return n, m, r


def _ttm_desc(n, m, r) -> _cabi.TtmDesc:
    d = len(n)
    if d == 0:
        raise ValueError("ttm_gather: at least one mode (d = 0 has no index to split)")
    if len(m) != d or len(r) != d + 1:
        raise ValueError(f"ttm_gather: {d} modes want {d} output sizes and {d + 1} ranks (got {len(m)}, {len(r)})")
    if int(r[0]) != 1:
        raise ValueError(f"ttm_gather: r_0 must be 1 (got {r[0]})")
    if d > TTM_MAX_D:
        raise ValueError(f"ttm_gather: the launch takes at most {TTM_MAX_D} modes (got {d})")
    if min(list(n) + list(m) + list(r)) <= 0:
        raise ValueError("ttm_gather: every mode size and rank must be positive")
    desc = _cabi.TtmDesc()
    desc.d = d
    for k in range(d):
        desc.n[k], desc.m[k], desc.r[k] = int(n[k]), int(m[k]), int(r[k])
    desc.r[d] = int(r[d])
    return desc


def ttm_gather_plan(n, m, r):
    """(fits, LDS bytes of the larger launch, tokens per forward workgroup) for mode sizes n, output sizes m and ranks
    r: `tadmm_ttm_gather_fits`, a pure function of the shapes.  Host only.  ValueError for d = 0, d > 4 and r_0 != 1.  A
    core of 2^31 elements or a running product beyond 2^30 floats does not fit and is not sized: (False, 0, 0)."""
    desc = _ttm_desc(n, m, r)
    nbytes, tile = C.c_size_t(), C.c_int()
    rc = _cabi.load().tadmm_ttm_gather_fits(C.byref(desc), C.byref(nbytes), C.byref(tile))
    if rc < 0:
        raise TadmmError(rc, "tadmm_ttm_gather_fits: invalid descriptor")
    return bool(rc), int(nbytes.value), int(tile.value)


def ttm_gather_fits(n, m, r) -> bool:
    """True when the one-launch gather takes the shape: at most 4 modes and the products of one token within the 160 KiB
    of LDS of a CU, forward and backward.  False sends `functional.ttm_embedding` down the composed device route.
    ValueError for d = 0 and r_0 != 1.  Pure host logic."""
    if len(n) > TTM_MAX_D:
        if len(n) and int(r[0]) != 1:
            raise ValueError(f"ttm_gather: r_0 must be 1 (got {r[0]})")
        return False
    return ttm_gather_plan(n, m, r)[0]


def ttm_index_split(index: torch.Tensor, n: Sequence[int]) -> List[torch.Tensor]:
    """Mode indices (i_1 .. i_d), i_1 slowest, of a flat integer index tensor; indices outside [0, prod(n)) are clamped
    into the range first (callers mask them).  Torch ops on the tensor's device, no synchronisation."""
    total = 1
    for v in n:
        total *= int(v)
    idx = index.reshape(-1).to(torch.int64).clamp(0, total - 1)
    out, stride = [], total
    for v in n:
        stride //= int(v)
        out.append(torch.remainder(torch.div(idx, stride, rounding_mode="floor"), int(v)))
    return out


def ttm_groups(index: torch.Tensor, n: Sequence[int]):
    """For every mode k: (order_k, offsets_k), the tokens grouped by i_k by a stable sort (ascending token order inside
    a group) and the n_k + 1 group offsets.  Sizes depend on n_k alone, so nothing synchronises."""
    out = []
    for k, ik in enumerate(ttm_index_split(index, n)):
        keys, order = torch.sort(ik, stable=True)
        edges = torch.arange(int(n[k]) + 1, device=ik.device, dtype=torch.int64)
        out.append((order, torch.searchsorted(keys, edges)))
    return out


def _ttm_operands(cores, index, who):
    n, m, r = ttm_core_shapes(cores)
    desc = _ttm_desc(n, m, r)
    if not isinstance(index, torch.Tensor) or index.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{who}: index must be an int32 or int64 tensor (got {getattr(index, 'dtype', type(index))})")
    dev = cores[0].device
    for k, c in enumerate(cores):
        _operand(c, who, f"core {k}", (torch.float32,))
        if c.device != dev:
            raise TadmmError(-1, f"{who}: core {k} on {c.device}, core 0 on {dev}")
    if index.device != dev:
        raise TadmmError(-1, f"{who}: index on {index.device}, cores on {dev}")
    flat = index.reshape(-1)
    flat = flat if flat.is_contiguous() else flat.contiguous()
    for k, c in enumerate(cores):
        desc.cores[k] = c.data_ptr()
    desc.index, desc.index_dtype, desc.B = flat.data_ptr(), int(flat.dtype == torch.int64), flat.numel()
    row = r[-1]
    for v in m:
        row *= v
    return desc, flat, row, dev


def ttm_gather(cores: Sequence[torch.Tensor], index: torch.Tensor, counter: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, m_1 ... m_d r_d) float32 rows of the gathered TT-matrix chain for the B indices of `index` (any shape, int32
    or int64), in one launch (`tadmm_ttm_gather_fwd`).  An index outside [0, prod(n)) gives a zero row and adds 1 to
    `counter` (one int32 on the device; a fresh zero when None).  Raises for shapes `ttm_gather_fits` refuses."""
    desc, flat, row, dev = _ttm_operands(cores, index, "ttm_gather")
    B = flat.numel()
    out = _output(out, (B, row), torch.float32, dev, "ttm_gather: out")
    # one int32 of any shape: the launch sees its address
    counter = _output(None if counter is None else counter.reshape(-1), (1,), torch.int32, dev, "ttm_gather: counter",
                      fresh=torch.zeros)
    desc.Y, desc.bad_count = out.data_ptr(), counter.data_ptr()
    h = _handle(dev)
    h.check(h.lib.tadmm_ttm_gather_fwd(h.ptr, C.byref(desc), _stream(dev)))
    return out


def ttm_gather_bwd(cores: Sequence[torch.Tensor], index: torch.Tensor, dy: torch.Tensor,
                   needs: Optional[Sequence[bool]] = None) -> List[Optional[torch.Tensor]]:
    """Gradients of sum(ttm_gather(cores, index) * dy) with respect to every core with needs[k] (all when None), one
    launch per core (`tadmm_ttm_gather_bwd`): every slice is written by one workgroup that adds its tokens in
    ascending order, so the result is bitwise reproducible and slices no token selects are exactly zero."""
    desc, flat, row, dev = _ttm_operands(cores, index, "ttm_gather_bwd")
    B = flat.numel()
    if dy.dtype != torch.float32 or dy.device != dev or dy.numel() != B * row:
        raise TadmmError(-1, f"ttm_gather_bwd: dy must hold ({B}, {row}) float32 values on {dev}")
    dy = dy.reshape(B, row)
    dy = dy if dy.is_contiguous() else dy.contiguous()
    needs = [True] * len(cores) if needs is None else list(needs)
    n = [int(c.shape[1]) for c in cores]
    groups = ttm_groups(flat, n)
    grads: List[Optional[torch.Tensor]] = [None] * len(cores)
    for k, c in enumerate(cores):
        if not needs[k]:
            continue
        grads[k] = torch.empty_like(c)
        desc.dcores[k] = grads[k].data_ptr()
        desc.order[k], desc.offsets[k] = groups[k][0].data_ptr(), groups[k][1].data_ptr()
    desc.dY = dy.data_ptr()
    if any(needs):
        h = _handle(dev)
        h.check(h.lib.tadmm_ttm_gather_bwd(h.ptr, C.byref(desc), _stream(dev)))
    return grads


TTM_GRAD_MAX_TOKENS = 512


def ttm_gather_pays(n, m, r, tokens: int, grad: bool = False) -> bool:
    """True when `functional.ttm_embedding` sends a shape the launch takes to the launch and not to the composed device
    route.  A pure function of the shapes, the token count and whether core gradients will be asked for.  Measured
    (scripts/bench_embeddings.py): without gradients the launch is ahead of or level with the
    composed route at every shape and token count of the table (up to 4.4x), so inference always takes it.  With
    gradients the one-workgroup-per-slice backward is behind the composed route for chains of two and more modes (0.23x
    at the TT-matrix table) and for one mode at 4096 tokens (0.94x); it is ahead for one mode at 512 tokens (1.30x).
    Token counts between the two were not measured and stay on the composed route."""
    if not grad:
        return True
    return len(n) == 1 and tokens <= TTM_GRAD_MAX_TOKENS


# ------------------------------------------------------------------ LSTM recurrence over a sequence (csrc/lstm.hip)
LSTM_MAX_H = 256                 # kLstmMaxH of csrc/lstm.hip: four waves of at most four 16-unit tiles
LSTM_ROWS = 16                   # batch rows of a workgroup
LSTM_LDS_BYTES = 160 * 1024


def lstm_plan(H: int):
    """(fits, LDS bytes of the larger launch, batch rows per workgroup) for hidden size H: `tadmm_lstm_fits`, a pure
    function of H.  Host only.  ValueError for H < 1; (False, 0, 16) for a hidden size the launch does not take."""
    if int(H) < 1:
        raise ValueError(f"lstm: the hidden size must be positive (got {H})")
    desc = _cabi.LstmDesc()
    desc.H = min(int(H), 2 ** 31 - 1)
    nbytes, rows = C.c_size_t(), C.c_int()
    rc = _cabi.load().tadmm_lstm_fits(C.byref(desc), C.byref(nbytes), C.byref(rows))
    if rc < 0:
        raise TadmmError(rc, "tadmm_lstm_fits: invalid descriptor")
    return bool(rc), int(nbytes.value), int(rows.value)


def lstm_fits(H: int) -> bool:
    """True when the one-launch recurrence takes hidden size H (1 <= H <= 256).  False sends
    `functional.lstm_sequence` down the composed step loop.  Pure host logic."""
    return lstm_plan(H)[0]


def lstm_planes(w_hh: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    """Three bf16 planes of the hidden-to-hidden weight (4H, H), gate order [i | f | g | o], as csrc/lstm.hip reads them:
    every gate's H rows padded to Hp = ceil16(H) with zeros, so that unit u of gate g is row g * Hp + u, then packed with
    `weight_planes(…, 3, pad_cols=32)`: (3, 4Hp/16, ceil32(H)/32, 64, 8).  `transpose=True`: the planes of the
    TRANSPOSED padded weight (H, 4Hp) -> (3, Hp/16, 4Hp/32, 64, 8), what the backward multiplies dz by."""
    if w_hh.dim() != 2 or w_hh.shape[0] != 4 * w_hh.shape[1] or w_hh.shape[1] < 1:
        raise ValueError(f"lstm_planes: w_hh must be (4H, H) (got {tuple(w_hh.shape)})")
    _operand(w_hh, "lstm_planes", "the weight", layout=None)
    H = w_hh.shape[1]
    Hp = -(-H // 16) * 16
    wp = torch.zeros(4, Hp, H, dtype=torch.float32, device=w_hh.device)
    wp[:, :H] = w_hh.detach().float().view(4, H, H)
    wp = wp.view(4 * Hp, H)
    return weight_planes(wp.t() if transpose else wp, 3, 16, 32)


def _lstm_tensor(t, shape, who, what, optional=False):
    """A float32 device operand of the recurrence, contiguous (copied if need be); `shape` None: any shape."""
    if t is None:
        if optional:
            return None
        raise TadmmError(-1, f"{who}: {what} is required")
    return _operand(t, who, what, (torch.float32,), shape, layout="copy")


def _lstm_out(out, shape, like, who, what):
    return _output(out, tuple(shape), torch.float32, like.device, f"{who}: {what}")


def _lstm_check_planes(planes, H, transpose, dev, who):
    Hp, Kp = -(-H // 16) * 16, -(-H // 32) * 32
    want = (3, Hp // 16, 4 * Hp // 32, 64, 8) if transpose else (3, 4 * Hp // 16, Kp // 32, 64, 8)
    _check_planes(planes, 3, torch.bfloat16, who)
    if tuple(planes.shape) != want or planes.device != dev:
        raise TadmmError(-1, f"{who}: the weight planes must be `lstm_planes(w_hh, transpose={transpose})`: bfloat16 "
                             f"{want} on {dev}")


def _lstm_fwd(entry, xp, planes, h0, c0, sigmoid, save, out):
    who = "lstm_seq_save" if save else "lstm_seq"
    xp = _lstm_tensor(xp, None, who, "xp")
    if xp.dim() != 3 or xp.shape[2] % 4 or xp.shape[2] == 0:
        raise TadmmError(-1, f"{who}: xp must be (T, B, 4H)")
    T, B, H = xp.shape[0], xp.shape[1], xp.shape[2] // 4
    dev = xp.device
    if not lstm_fits(H):
        raise TadmmError(-5, f"{who}: H = {H}, the launch takes 1 <= H <= {LSTM_MAX_H}")
    _lstm_check_planes(planes, H, False, dev, who)
    h0 = _lstm_tensor(h0, (B, H), who, "h0", optional=True)
    c0 = _lstm_tensor(c0, (B, H), who, "c0", optional=True)
    out = dict(out or {})
    y = _lstm_out(out.get("y"), (T, B, H), xp, who, "y")
    hT = _lstm_out(out.get("hT"), (B, H), xp, who, "hT")
    cT = _lstm_out(out.get("cT"), (B, H), xp, who, "cT")
    d = _cabi.LstmDesc()
    d.Xp, d.W, d.Y, d.hT, d.cT = xp.data_ptr(), planes.data_ptr(), y.data_ptr(), hT.data_ptr(), cT.data_ptr()
    d.h0 = None if h0 is None else h0.data_ptr()
    d.c0 = None if c0 is None else c0.data_ptr()
    d.T, d.B, d.H, d.sigmoid = T, B, H, int(bool(sigmoid))
    res = (y, hT, cT)
    if save:
        g = torch.empty(T, B, 4 * H, dtype=torch.float32, device=dev)
        c = torch.empty(T, B, H, dtype=torch.float32, device=dev)
        d.G, d.C = g.data_ptr(), c.data_ptr()
        res = (y, hT, cT, g, c)
    if T == 0 or B == 0:
        raise TadmmError(-1, f"{who}: T >= 1 and B >= 1 are required")
    h = _handle(dev)
    h.check(getattr(h.lib, entry)(h.ptr, C.byref(d), _stream(dev)))
    return res


def lstm_seq(xp: torch.Tensor, planes: torch.Tensor, h0: Optional[torch.Tensor] = None, c0: Optional[torch.Tensor] = None,
             sigmoid: bool = False, out: Optional[dict] = None):
    """(y (T, B, H), hT, cT (B, H)) of the LSTM recurrence over the whole sequence in ONE launch (`tadmm_lstm_seq_fwd`).
    xp (T, B, 4H) float32: the input pre-activations, bias included, gate order [i | f | g | o]; planes:
    `lstm_planes(w_hh)`; h0, c0 (B, H), zeros when None; i, f, o through Hardsigmoid, or the logistic function with
    `sigmoid`.  `out`: optional {"y", "hT", "cT"} tensors to write into (any 4-byte aligned contiguous view)."""
    return _lstm_fwd("tadmm_lstm_seq_fwd", xp, planes, h0, c0, sigmoid, False, out)


def lstm_seq_save(xp: torch.Tensor, planes: torch.Tensor, h0: Optional[torch.Tensor] = None,
                  c0: Optional[torch.Tensor] = None, sigmoid: bool = False, out: Optional[dict] = None):
    """`lstm_seq` for a training step (`tadmm_lstm_seq_fwd_save`): (y, hT, cT, G, C) with G (T, B, 4H) the four gate
    activations and C (T, B, H) every cell state, what `lstm_seq_bwd` reads.  y, hT, cT are bitwise those of `lstm_seq`."""
    return _lstm_fwd("tadmm_lstm_seq_fwd_save", xp, planes, h0, c0, sigmoid, True, out)


def lstm_seq_bwd(planes_t: torch.Tensor, g: torch.Tensor, c: torch.Tensor, c0: Optional[torch.Tensor] = None,
                 dy: Optional[torch.Tensor] = None, dhT: Optional[torch.Tensor] = None, dcT: Optional[torch.Tensor] = None,
                 sigmoid: bool = False, dz: Optional[torch.Tensor] = None):
    """Backward through time in one launch (`tadmm_lstm_seq_bwd`): (dZ (T, B, 4H), dh0, dc0 (B, H)) from the saved G, C
    of `lstm_seq_save`, c0 and the gradients of y, hT, cT (each zeros when None).  planes_t:
    `lstm_planes(w_hh, transpose=True)`.  dZ is the gradient of the pre-activations and so of xp; the weight gradient is
    `wgrad(dZ.view(T*B, 4H), Hprev.view(T*B, H))` with Hprev = [h0, y[0 .. T-2]], the bias gradient `dZ.sum((0, 1))`.
    `dz`: optional tensor to write dZ into."""
    who = "lstm_seq_bwd"
    c = _lstm_tensor(c, None, who, "C")
    if c.dim() != 3:
        raise TadmmError(-1, f"{who}: C must be (T, B, H)")
    T, B, H = c.shape
    dev = c.device
    if T == 0 or B == 0 or H == 0:
        raise TadmmError(-1, f"{who}: T >= 1, B >= 1 and H >= 1 are required")
    if not lstm_fits(H):
        raise TadmmError(-5, f"{who}: H = {H}, the launch takes 1 <= H <= {LSTM_MAX_H}")
    g = _lstm_tensor(g, (T, B, 4 * H), who, "G")
    _lstm_check_planes(planes_t, H, True, dev, who)
    c0 = _lstm_tensor(c0, (B, H), who, "c0", optional=True)
    dy = _lstm_tensor(dy, (T, B, H), who, "dy", optional=True)
    dhT = _lstm_tensor(dhT, (B, H), who, "dhT", optional=True)
    dcT = _lstm_tensor(dcT, (B, H), who, "dcT", optional=True)
    dz = _lstm_out(dz, (T, B, 4 * H), c, who, "dz")
    dh0 = torch.empty(B, H, dtype=torch.float32, device=dev)
    dc0 = torch.empty(B, H, dtype=torch.float32, device=dev)
    d = _cabi.LstmDesc()
    d.W, d.G, d.C, d.dZ, d.dh0, d.dc0 = planes_t.data_ptr(), g.data_ptr(), c.data_ptr(), dz.data_ptr(), dh0.data_ptr(), \
        dc0.data_ptr()
    for name, t in (("c0", c0), ("dY", dy), ("dhT", dhT), ("dcT", dcT)):
        setattr(d, name, None if t is None else t.data_ptr())
    d.T, d.B, d.H, d.sigmoid = T, B, H, int(bool(sigmoid))
    h = _handle(dev)
    h.check(h.lib.tadmm_lstm_seq_bwd(h.ptr, C.byref(d), _stream(dev)))
    return dz, dh0, dc0


def lstm_seq_pays(T: int, B: int, H: int, grad: bool = False) -> bool:
    """True when `functional.lstm_sequence` sends a shape the launch takes to the launch and not to the composed step
    loop.  A pure function of the sequence length, the batch, the hidden size and whether gradients will be asked for.
    Measured (scripts/bench_lstm.py) at H in {64, 128, 256}, T in {6, 64}, B in {1, 16, 64, 256}:
    the launch is ahead of the composed loop beyond the spread of both in every class, forward (2.1x - 18.5x) and
    training step (3.3x - 30.6x); the smallest margin is H = 256, T = 6, B = 256.  No class of the table goes the other
    way, so every shape the launch takes is sent to it.  Batches beyond 256 rows were not measured."""
    return True


# ------------------------------------------------------------------ distillation loss (csrc/distill.hip)
DISTILL_BASES = {"none": _cabi.DISTILL_BASE_NONE, "index": _cabi.DISTILL_BASE_INDEX, "dense": _cabi.DISTILL_BASE_DENSE}
DISTILL_KDS = {"none": _cabi.DISTILL_KD_NONE, "soft": _cabi.DISTILL_KD_SOFT_KL, "hard": _cabi.DISTILL_KD_HARD,
               "soft_ce": _cabi.DISTILL_KD_SOFT_CE}
DISTILL_DTYPES = {torch.float32: _cabi.CHAIN_F32, torch.bfloat16: _cabi.CHAIN_BF16, torch.float16: _cabi.CHAIN_F16}
DISTILL_NO_IGNORE = -2 ** 63         # an ignore_index no label can equal out of range by accident: "ignore nothing"


def distill_workspace_bytes(B: int) -> int:
    """Bytes of the row-term workspace of `tadmm_distill_loss` for B rows (`tadmm_distill_workspace_bytes`).  Host only."""
    d = _cabi.DistillDesc()
    d.B = int(B)
    size = C.c_size_t()
    rc = _cabi.load().tadmm_distill_workspace_bytes(C.byref(d), C.byref(size))
    if rc < 0:
        raise TadmmError(rc, f"tadmm_distill_workspace_bytes: B = {B}")
    return int(size.value)


def _distill_rows(t, who, what, shape, dtypes):
    """A (B, C) operand read by rows: unit column stride and a row stride >= C as it stands (a row slice of a wider
    tensor), anything else as a contiguous copy.  Returns (tensor, row stride)."""
    t = _operand(t, who, what, dtypes, shape, layout=None)
    B, Cc = t.shape
    if (Cc > 1 and t.stride(1) != 1) or (B > 1 and t.stride(0) < Cc):
        t = t.contiguous()
    return t, (max(int(t.stride(0)), Cc) if B > 1 else Cc)


def distill_loss(outputs, outputs_kd, teacher, target, *, base: str, kd: str, alpha: float = 0.5, tau: float = 1.0,
                 smoothing: float = 0.0, ignore_index: Optional[int] = -100, grad=True, out: Optional[dict] = None):
    """(loss, counts, grad_s, grad_k) of `tadmm_distill_loss`: the base criterion on `outputs` (B, C), the distillation
    term of `outputs_kd` against `teacher`, mixed as (1-alpha) base + alpha kd (`kd="none"`: the base alone;
    `base="none"`: alpha kd), in two launches, gradients included.  base: "none", "index" (`target` int64 (B,); labels
    equal to `ignore_index` or outside [0, C) are dropped from the mean, the latter counted; `ignore_index=None`: nothing
    is ignored), "dense" (`target` float32 (B, C) rows).  kd: "none", "soft" (KL at temperature tau, times tau^2 / (B C)),
    "hard" (cross entropy against the teacher's first argmax), "soft_ce" (task_distill.py:721-724 at temperature tau).
    The logits are float32, bfloat16 or float16, all of one type, with unit column stride and any row stride >= C (no
    copy is made of such views).  loss: float32 0-dim; counts: int64 [kept rows, bad labels]; grad_s, grad_k: float32
    (B, C) gradients with respect to `outputs` / `outputs_kd` (`grad`: a bool or a pair of bools; None where not asked
    for).  `out`: optional {"grad_s", "grad_k"} tensors to write them into; handing the same tensor for both yields the
    sum of the two in it (what a caller wants when `outputs_kd` is `outputs`).  Nothing synchronises."""
    who = "distill_loss"
    if base not in DISTILL_BASES or kd not in DISTILL_KDS:
        raise ValueError(f"{who}: base is one of {sorted(DISTILL_BASES)}, kd one of {sorted(DISTILL_KDS)} "
                         f"(got {base!r}, {kd!r})")
    if base == "none" and kd == "none":
        raise ValueError(f"{who}: base and kd are both 'none'")
    first = outputs if base != "none" else outputs_kd
    first = _operand(first, who, "outputs" if base != "none" else "outputs_kd", tuple(DISTILL_DTYPES), layout=None)
    if first.dim() != 2 or first.shape[0] < 1 or first.shape[1] < 1:
        raise TadmmError(-1, f"{who}: the logits must be (B >= 1, C >= 1) (got {tuple(first.shape)})")
    B, Cc = first.shape
    dev, dt = first.device, first.dtype
    d = _cabi.DistillDesc()
    keep = []
    for name, field, t, used in (("outputs", "s", outputs, base != "none"), ("outputs_kd", "k", outputs_kd, kd != "none"),
                                 ("teacher", "t", teacher, kd != "none")):
        if not used:
            continue
        t, ld = _distill_rows(t, who, name, (B, Cc), (dt,))
        if t.device != dev:
            raise TadmmError(-1, f"{who}: {name} on {t.device}, the other logits on {dev}")
        keep.append(t)
        setattr(d, field, t.data_ptr())
        setattr(d, field + "_ld", ld)
    if base == "index":
        target = _operand(target, who, "target", (torch.int64,), (B,), layout="copy")
        d.labels = target.data_ptr()
    elif base == "dense":
        target, d.dense_ld = _distill_rows(target, who, "target", (B, Cc), (torch.float32,))
        d.dense = target.data_ptr()
    if base != "none" and target.device != dev:
        raise TadmmError(-1, f"{who}: target on {target.device}, the logits on {dev}")
    want_s, want_k = (bool(grad), bool(grad)) if isinstance(grad, bool) else (bool(grad[0]), bool(grad[1]))
    out = dict(out or {})
    gs = _output(out.get("grad_s"), (B, Cc), torch.float32, dev, f"{who}: grad_s") if want_s and base != "none" else None
    gk = _output(out.get("grad_k"), (B, Cc), torch.float32, dev, f"{who}: grad_k") if want_k and kd != "none" else None
    loss = torch.empty((), dtype=torch.float32, device=dev)
    wide = torch.empty(3, dtype=torch.int64, device=dev)          # [loss as double | kept rows | bad labels]
    nbytes = distill_workspace_bytes(B)
    ws = _scratch(nbytes, dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    d.loss_dev, d.counts_dev, d.loss_f32_dev = wide.data_ptr(), wide.data_ptr() + 8, loss.data_ptr()
    d.grad_s = None if gs is None else gs.data_ptr()
    d.grad_k = None if gk is None else gk.data_ptr()
    d.ignore_index = DISTILL_NO_IGNORE if ignore_index is None else int(ignore_index)
    d.eps, d.alpha, d.tau = float(smoothing), float(alpha), float(tau)
    d.B, d.C, d.dtype = B, Cc, DISTILL_DTYPES[dt]
    d.base_kind, d.kd_kind = DISTILL_BASES[base], DISTILL_KDS[kd]
    h = _handle(dev)
    h.check(h.lib.tadmm_distill_loss(h.ptr, C.byref(d), _stream(dev)))
    return loss, wide[1:], gs, gk


def distill_loss_pays(B: int, C: int, dtype, grad: bool = False) -> bool:
    """True when `functional.distillation_loss` sends a call to the launch and not to the composed torch route.  A pure
    function of the batch, the class count, the logit type and whether gradients will be asked for.  Measured
    (scripts/bench_distill.py) at (B, C) from (32, 2) to (1024, 1000), soft and hard distillation,
    float32 and float16, value only and value + backward: the launch's slowest window is below the composed route's
    fastest in all 48 classes (2.1x - 4.2x; both routes are bound by the host at these sizes), so the rule is a
    constant.  Batches beyond 1024 rows and class counts beyond 1000 were not measured."""
    return True


# ------------------------------------------------------------------ TinyBERT layer losses (csrc/layermse.hip)
LAYER_MSE_MAX_PAIRS = _cabi.LAYER_MSE_MAX_PAIRS
LAYER_MSE_DTYPES = DISTILL_DTYPES
LAYER_MSE_GROUPS = {"att": _cabi.LAYER_MSE_ATT, "rep": _cabi.LAYER_MSE_REP}


def layer_mse_geometry():
    """(chunk_elems, max_blocks) of `tadmm_layer_mse`: the elements of one chunk of a pair and the cap of the streaming
    launch's grid (`tadmm_layer_mse_geometry`).  Host only."""
    chunk, blocks = C.c_int(), C.c_int()
    rc = _cabi.load().tadmm_layer_mse_geometry(C.byref(chunk), C.byref(blocks))
    if rc < 0:
        raise TadmmError(rc, "tadmm_layer_mse_geometry")
    return int(chunk.value), int(blocks.value)


def layer_mse_workspace_bytes(numels: Sequence[int]) -> int:
    """Bytes of the partial-sum workspace of `tadmm_layer_mse` for pairs of `numels` elements
    (`tadmm_layer_mse_workspace_bytes`: one double per pair and workgroup).  Host only."""
    numels = [int(n) for n in numels]
    d = _cabi.LayerMseDesc()
    d.npairs = len(numels)
    for i, n in enumerate(numels[:LAYER_MSE_MAX_PAIRS]):
        d.pairs[i].n = n
    size = C.c_size_t()
    rc = _cabi.load().tadmm_layer_mse_workspace_bytes(C.byref(d), C.byref(size))
    if rc < 0:
        raise TadmmError(rc, f"tadmm_layer_mse_workspace_bytes: numels = {numels}")
    return int(size.value)


def _per_pair(v, n, what):
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise ValueError(f"layer_mse: {len(v)} {what} for {n} pairs")
        return list(v)
    return [v] * n


def layer_mse(students, teachers, scales, groups, clamp, thr, *, grads=None):
    """(loss, terms) of `tadmm_layer_mse` for the pairs (students[i], teachers[i]): equal shapes, float32, bfloat16 or
    float16 of one type on one HIP device (a non-contiguous tensor is copied).  With s' and t' the values of a pair whose
    entries <= `thr` are replaced by zero where `clamp` is set, term_i = scales[i] * sum((s' - t')^2); loss: float32 (2,) =
    the sums of the terms of group "att" (0) and of group "rep" (1); terms: float64 (npairs,).  `groups`, `clamp` and `thr`
    are one value for all pairs or a sequence.  `grads`: per pair None or a contiguous float32 tensor of the pair's
    element count that receives d term_i / d students[i] = 2 scales[i] (s' - t'), zero where s was clamped.  Two launches
    whatever the number of pairs (at most `LAYER_MSE_MAX_PAIRS`); nothing synchronises."""
    who = "layer_mse"
    students, teachers = list(students), list(teachers)
    n = len(students)
    if len(teachers) != n:
        raise ValueError(f"{who}: {n} students and {len(teachers)} teachers")
    if not 1 <= n <= LAYER_MSE_MAX_PAIRS:
        raise TadmmError(-1, f"{who}: {n} pairs; one call takes 1 to {LAYER_MSE_MAX_PAIRS}")
    scales, groups = _per_pair(scales, n, "scales"), _per_pair(groups, n, "groups")
    clamp, thr = _per_pair(clamp, n, "clamp flags"), _per_pair(thr, n, "thresholds")
    grads = _per_pair(grads, n, "gradient buffers")
    first = _operand(students[0], who, "students[0]", tuple(LAYER_MSE_DTYPES), layout=None)
    dev, dt = first.device, first.dtype
    d = _cabi.LayerMseDesc()
    hold = []
    for i in range(n):
        s = _operand(students[i], who, f"students[{i}]", (dt,), layout="copy")
        t = _operand(teachers[i], who, f"teachers[{i}]", (dt,), tuple(s.shape), layout="copy")
        if s.device != dev or t.device != dev:
            raise TadmmError(-1, f"{who}: pair {i} on {s.device} / {t.device}, students[0] on {dev}")
        if s.numel() < 1:
            raise TadmmError(-1, f"{who}: pair {i} is empty")
        if groups[i] not in (0, 1) and groups[i] not in LAYER_MSE_GROUPS:
            raise ValueError(f"{who}: group {groups[i]!r} of pair {i} is none of 0, 1, 'att', 'rep'")
        hold += [s, t]
        q = d.pairs[i]
        q.s, q.t, q.n = s.data_ptr(), t.data_ptr(), s.numel()
        q.scale = float(scales[i])
        q.clamp = 1 if clamp[i] and thr[i] is not None else 0
        q.thr = float(thr[i]) if q.clamp else 0.0
        q.group = LAYER_MSE_GROUPS.get(groups[i], groups[i])
        if grads[i] is not None:
            g = _output(grads[i], tuple(grads[i].shape), torch.float32, dev, f"{who}: grads[{i}]")
            if g.numel() != s.numel():
                raise TadmmError(-1, f"{who}: grads[{i}] has {g.numel()} elements, the pair {s.numel()}")
            q.grad = g.data_ptr()
    d.npairs, d.dtype = n, LAYER_MSE_DTYPES[dt]
    wide = torch.empty(n + 3, dtype=torch.float64, device=dev)      # [terms | loss as double (2) | loss as float32 (2)]
    loss = wide[n + 2:].view(torch.float32)
    size = C.c_size_t()
    h = _handle(dev)
    rc = h.lib.tadmm_layer_mse_workspace_bytes(C.byref(d), C.byref(size))
    if rc < 0:
        raise TadmmError(rc, f"{who}: the pairs hold more chunks than one call takes")
    ws = _scratch(size.value, dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), size.value
    d.terms_dev, d.loss_dev, d.loss_f32_dev = wide.data_ptr(), wide.data_ptr() + 8 * n, loss.data_ptr()
    h.check(h.lib.tadmm_layer_mse(h.ptr, C.byref(d), _stream(dev)))
    return loss, wide[:n]


def layer_mse_pays(numel: int, npairs: int, dtype, grad: bool = False) -> bool:
    """True when `functional.intermediate_distillation_loss` sends a call the launch can take to it and not to the
    composed torch route.  A pure function of the total element count of the students, the number of pairs, the element
    type and whether gradients will be asked for.  Measured (scripts/bench_layer_mse.py) against
    `intermediate_distillation_loss_composed` in the same run, three runs, float32 and bfloat16, value only and value +
    backward, at four classes: the reference's step (1 + 1 pairs, 9.4 M elements), a small step (1 + 1 pairs, 0.55 M),
    and per-layer loops of 4 + 5 pairs (31.6 M) and 12 + 13 pairs (29.1 M).  In every run the launch's slowest window is
    below the composed route's fastest for the value (2.0x - 11.3x), for the bfloat16 training step (1.5x - 8.4x) and
    for the float32 training step of the 9- and 25-pair classes (3.3x - 5.5x).  The float32 training step of the two
    2-pair classes is ahead by the medians in all three runs (1.3x - 2.2x) but level by the windows in two of them
    (the launch's slowest window 0.17 - 0.20 ms against the composed route's fastest 0.16 - 0.17 ms: both are bound by the
    host there), so it goes to the composed route until it has 9 pairs or 29.1 M elements, the smallest classes
    measured ahead.  Not measured: float16 (treated as bfloat16), between 2 and 9 pairs, more than 32 M elements, calls
    in which only some students require a gradient."""
    if grad and dtype == torch.float32:
        return npairs >= 9 or numel >= 29_097_984
    return True


# ------------------------------------------------------------------ BERT self-attention (csrc/attn.hip)
ATTN_DTYPES = DISTILL_DTYPES


def attn_fits(S: int, d: int, H: int = 1, dtype=torch.float32) -> bool:
    """True when `tadmm_attn_fwd` / `_bwd` take sequences of S tokens with heads of width d (`tadmm_attn_fits`:
    1 <= S <= 512, 1 <= d <= 64).  Raises TadmmError for S < 1, d < 1 or H < 1.  Host only."""
    dsc = _cabi.AttnDesc()
    dsc.S, dsc.d, dsc.H, dsc.dtype = int(S), int(d), int(H), ATTN_DTYPES[dtype]
    rc = _cabi.load().tadmm_attn_fits(C.byref(dsc), None)
    if rc < 0:
        raise TadmmError(rc, f"tadmm_attn_fits: S = {S}, d = {d}, H = {H}")
    return rc == 1


def attn_workspace_bytes(B: int, H: int, S: int) -> int:
    """Bytes of the backward's workspace (`tadmm_attn_workspace_bytes`: one double per query row and head)."""
    dsc = _cabi.AttnDesc()
    dsc.B, dsc.H, dsc.S = int(B), int(H), int(S)
    size = C.c_size_t()
    rc = _cabi.load().tadmm_attn_workspace_bytes(C.byref(dsc), C.byref(size))
    if rc < 0:
        raise TadmmError(rc, f"tadmm_attn_workspace_bytes: B = {B}, H = {H}, S = {S}")
    return int(size.value)


def _attn_heads(t, who, what, shape, dt):
    """A (B, S, H*d) operand read in place by heads: unit element stride and a row stride >= H*d as it stands (a slice
    of a packed qkv tensor), anything else as a contiguous copy.  Returns (tensor, row stride, batch stride)."""
    t = _operand(t, who, what, (dt,), shape, layout=None)
    B, S, Hd = t.shape
    if (Hd > 1 and t.stride(2) != 1) or (S > 1 and t.stride(1) < Hd) or (B > 1 and t.stride(0) < 0):
        t = t.contiguous()
    ld = max(int(t.stride(1)), Hd) if S > 1 else Hd
    return t, ld, (int(t.stride(0)) if B > 1 else 0)


def _attn_desc(q, k, v, mask, num_heads, p, keep, who):
    q = _operand(q, who, "q", tuple(ATTN_DTYPES), layout=None)
    if q.dim() != 3 or num_heads < 1 or q.shape[2] % num_heads or q.shape[1] < 1 or q.shape[2] < 1:
        raise TadmmError(-1, f"{who}: q must be (B, S >= 1, H*d) with H = {num_heads} (got {tuple(q.shape)})")
    B, S, Hd = q.shape
    H, hd = int(num_heads), Hd // int(num_heads)
    dev, dt = q.device, q.dtype
    dsc = _cabi.AttnDesc()
    hold = []
    for name, t in (("q", q), ("k", k), ("v", v)):
        t, ld, bs = _attn_heads(t, who, name, (B, S, Hd), dt)
        if t.device != dev:
            raise TadmmError(-1, f"{who}: {name} on {t.device}, q on {dev}")
        hold.append(t)
        setattr(dsc, name, t.data_ptr())
        setattr(dsc, name + "_ld", ld)
        setattr(dsc, name + "_bs", bs)
    if mask is not None:
        mask = _operand(mask, who, "mask", None, (B, 1, 1, S), layout=None)
        if mask.device != dev:
            raise TadmmError(-1, f"{who}: mask on {mask.device}, q on {dev}")
        mask = mask.reshape(B, S).to(torch.float32).contiguous()
        hold.append(mask)
        dsc.mask = mask.data_ptr()
    p = float(p)
    if p > 0.0:
        if keep is None:
            raise TadmmError(-1, f"{who}: dropout p = {p} needs the keep tensor")
        if keep.dtype == torch.bool:
            keep = keep.view(torch.uint8)
        keep = _operand(keep, who, "keep", (torch.uint8,), (B, H, S, S), layout="copy")
        if keep.device != dev:
            raise TadmmError(-1, f"{who}: keep on {keep.device}, q on {dev}")
        hold.append(keep)
        dsc.keep = keep.data_ptr()
    dsc.p = p
    dsc.B, dsc.H, dsc.S, dsc.d, dsc.dtype = B, H, S, hd, ATTN_DTYPES[dt]
    return dsc, hold, (B, H, S, hd, dev, dt)


def attn_fwd(q, k, v, mask, num_heads: int, *, p: float = 0.0, keep=None, need_scores: bool = True,
             need_stats: bool = False):
    """(context, scores, stats) of `tadmm_attn_fwd`: q, k, v (B, S, H*d) float32, bfloat16 or float16 of one type, read in
    place by heads (unit element stride, any row stride >= H*d: slices of a packed qkv tensor are not copied); `mask`
    additive (B, 1, 1, S) or None; `keep` (B, H, S, S) uint8 / bool, read when p > 0.  context (B, S, H*d) and scores
    (B, H, S, S; None unless `need_scores`) in the input type, stats float32 (B, H, S, 2) = (row maximum, row sum of
    exp(score - maximum)) (None unless `need_stats`; the backward reads it).  One launch; nothing synchronises."""
    who = "attn_fwd"
    dsc, hold, (B, H, S, hd, dev, dt) = _attn_desc(q, k, v, mask, num_heads, p, keep, who)
    ctx = torch.empty((B, S, H * hd), dtype=dt, device=dev)
    scores = torch.empty((B, H, S, S), dtype=dt, device=dev) if need_scores else None
    stats = torch.empty((B, H, S, 2), dtype=torch.float32, device=dev) if need_stats else None
    dsc.ctx = ctx.data_ptr()
    dsc.scores = None if scores is None else scores.data_ptr()
    dsc.stats = None if stats is None else stats.data_ptr()
    h = _handle(dev)
    h.check(h.lib.tadmm_attn_fwd(h.ptr, C.byref(dsc), _stream(dev)))
    return ctx, scores, stats


def attn_bwd(q, k, v, mask, num_heads: int, stats, g_ctx, g_sc, *, p: float = 0.0, keep=None):
    """(dq, dk, dv) of `tadmm_attn_bwd` for the upstream gradients `g_ctx` (of the context) and `g_sc` (of the scores),
    either None: float32 or bfloat16 (float16 is refused), each (B, S, H*d) contiguous in the input type.  P is
    recomputed from q, k, the mask and `stats` (float32 (B, H, S, 2), from `attn_fwd(need_stats=True)`).  Two launches, no
    atomics, bitwise reproducible; nothing synchronises."""
    who = "attn_bwd"
    dsc, hold, (B, H, S, hd, dev, dt) = _attn_desc(q, k, v, mask, num_heads, p, keep, who)
    stats = _operand(stats, who, "stats", (torch.float32,), (B, H, S, 2), layout="copy")
    dsc.stats = stats.data_ptr()
    if g_ctx is not None:
        g_ctx = _operand(g_ctx, who, "g_ctx", (dt,), (B, S, H * hd), layout="copy")
        dsc.g_ctx = g_ctx.data_ptr()
        nbytes = attn_workspace_bytes(B, H, S)
        ws = _scratch(nbytes, dev)
        dsc.workspace, dsc.workspace_bytes = ws.data_ptr(), nbytes
    if g_sc is not None:
        g_sc = _operand(g_sc, who, "g_sc", (dt,), (B, H, S, S), layout="copy")
        dsc.g_sc = g_sc.data_ptr()
    out = torch.empty((3, B, S, H * hd), dtype=dt, device=dev)
    dsc.dq, dsc.dk, dsc.dv = out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()
    h = _handle(dev)
    h.check(h.lib.tadmm_attn_bwd(h.ptr, C.byref(dsc), _stream(dev)))
    return out[0], out[1], out[2]


def attn_pays(B: int, H: int, S: int, d: int, dtype, grad: bool = False) -> bool:
    """True when `functional.self_attention` sends a call the launch can take to it and not to the composed torch route.
    A pure function of its arguments.  Measured (scripts/bench_attention.py) at H = 12, d = 64,
    B in {1, 8, 32}, S in {64, 128, 384, 512}, float32 and bfloat16, forward with and without the scores output and a
    training step with gradients into both outputs, against `self_attention_composed` in the same run.  At S = 64 and
    128 the launch's slowest window is below the composed route's fastest in all 36 classes (forward 1.4x - 3.8x, training
    step 1.5x - 4.2x; the composed route is bound by the host's nine launches there).  At S = 384 and 512 the composed
    route is ahead in 32 of 36 classes (the launch at 0.47x - 0.88x of it), two are level and two go to the launch
    (B = 1, S = 384: bfloat16 training 1.23x): the launch computes the score product twice and stages its tiles with
    element loads, which the batched BLAS products of the composed route do not.  So the rule is the sequence length alone: the launch up to 128
    tokens, the composed route beyond.  Not measured: lengths between 129 and 383 (sent to the composed route), head
    widths other than 64, head counts other than 12, float16, dropout on."""
    return S <= 128


# ------------------------------------------------------------------ BERT sub-layer tail (csrc/bertnorm.hip)
BERTNORM_DTYPES = DISTILL_DTYPES


def bertnorm_hmax() -> int:
    """The widest row `tadmm_bertnorm_fwd` / `_bwd` take (what `tadmm_bertnorm_fits` reports).  Host only."""
    hmax = C.c_int()
    _cabi.load().tadmm_bertnorm_fits(None, C.byref(hmax))
    return int(hmax.value)


def bertnorm_fits(hidden: int, dtype=torch.float32) -> bool:
    """True when the launches take rows of `hidden` columns (`tadmm_bertnorm_fits`: 1 <= hidden <= `bertnorm_hmax()`).
    Raises TadmmError for hidden < 1.  Host only."""
    dsc = _cabi.BertNormDesc()
    dsc.hidden, dsc.dtype = int(hidden), BERTNORM_DTYPES[dtype]
    rc = _cabi.load().tadmm_bertnorm_fits(C.byref(dsc), None)
    if rc < 0:
        raise TadmmError(rc, f"tadmm_bertnorm_fits: hidden = {hidden}")
    return rc == 1


def bertnorm_workspace_bytes(rows: int, hidden: int) -> int:
    """Bytes of the backward's workspace (`tadmm_bertnorm_workspace_bytes`: one float32 (2, hidden rounded up to 4)
    partial per workgroup of the row launch, min(ceil(rows / 4), 512) of them, rounded up to 256 bytes).  Host only."""
    dsc = _cabi.BertNormDesc()
    dsc.rows, dsc.hidden = int(rows), int(hidden)
    size = C.c_size_t()
    rc = _cabi.load().tadmm_bertnorm_workspace_bytes(C.byref(dsc), C.byref(size))
    if rc < 0:
        raise TadmmError(rc, f"tadmm_bertnorm_workspace_bytes: rows = {rows}, hidden = {hidden}")
    return int(size.value)


def _bertnorm_rows(t, who, what, shape, dt):
    """A (rows, hidden) operand read in place: unit column stride and a row stride >= hidden as it stands (a column
    slice of a wider tensor, a view that starts anywhere), anything else as a contiguous copy.  Returns (tensor, row
    stride)."""
    t = _operand(t, who, what, (dt,), shape, layout=None)
    rows, hidden = t.shape
    if (hidden > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) < hidden):
        t = t.contiguous()
    return t, (max(int(t.stride(0)), hidden) if rows > 1 else hidden)


def _bertnorm_desc(x, res, gamma, beta, p, keep, eps, who):
    x = _operand(x, who, "x", tuple(BERTNORM_DTYPES), layout=None)
    if x.dim() != 2 or x.shape[1] < 1:
        raise TadmmError(-1, f"{who}: x must be (rows, hidden >= 1) (got {tuple(x.shape)})")
    rows, hidden = x.shape
    dev, dt = x.device, x.dtype
    dsc = _cabi.BertNormDesc()
    hold = []
    x, dsc.x_ld = _bertnorm_rows(x, who, "x", (rows, hidden), dt)
    dsc.x = x.data_ptr()
    hold.append(x)
    if res is not None:
        res, dsc.res_ld = _bertnorm_rows(res, who, "res", (rows, hidden), dt)
        dsc.res = res.data_ptr()
        hold.append(res)
    pdt = gamma.dtype if isinstance(gamma, torch.Tensor) else None
    for name, t in (("gamma", gamma), ("beta", beta)):
        if t is None and name == "beta":
            continue
        t = _operand(t, who, name, (torch.float32, dt), (hidden,), layout="copy")
        if t.dtype != pdt:
            raise TadmmError(-1, f"{who}: gamma and beta must be of one type (got {pdt} and {t.dtype})")
        hold.append(t)
        setattr(dsc, name, t.data_ptr())
    p = float(p)
    if p > 0.0:
        if keep is None:
            raise TadmmError(-1, f"{who}: dropout p = {p} needs the keep tensor")
        if keep.dtype == torch.bool:
            keep = keep.view(torch.uint8)
        keep = _operand(keep, who, "keep", (torch.uint8,), (rows, hidden), layout="copy")
        hold.append(keep)
        dsc.keep = keep.data_ptr()
    for t in hold:
        if t.device != dev:
            raise TadmmError(-1, f"{who}: an operand on {t.device}, x on {dev}")
    dsc.p, dsc.eps = p, float(eps)
    dsc.rows, dsc.hidden, dsc.dtype, dsc.param_dtype = rows, hidden, BERTNORM_DTYPES[dt], BERTNORM_DTYPES[pdt]
    return dsc, hold, (rows, hidden, dev, dt)


def bertnorm_fwd(x, res, gamma, beta, *, eps: float = 1e-12, p: float = 0.0, keep=None, need_stats: bool = False):
    """(y, stats) of `tadmm_bertnorm_fwd`: y = LayerNorm(x keep / (1 - p) + res) over the last dimension of x (rows,
    hidden), float32, bfloat16 or float16; `res` of the same type and shape or None; both read in place (unit element
    stride, any row stride >= hidden, any element alignment).  `gamma`, `beta`: (hidden,), both float32 or both of the
    type of x.  `keep` (rows, hidden) uint8 / bool, read when p > 0.  y (rows, hidden) contiguous in the type of x;
    stats float32 (rows, 2) = (mean, 1 / sqrt(var + eps)) (None unless `need_stats`; the backward reads it).  One launch;
    nothing synchronises."""
    who = "bertnorm_fwd"
    dsc, hold, (rows, hidden, dev, dt) = _bertnorm_desc(x, res, gamma, beta, p, keep, eps, who)
    y = torch.empty((rows, hidden), dtype=dt, device=dev)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=dev) if need_stats else None
    dsc.y = y.data_ptr()
    dsc.stats = None if stats is None else stats.data_ptr()
    h = _handle(dev)
    h.check(h.lib.tadmm_bertnorm_fwd(h.ptr, C.byref(dsc), _stream(dev)))
    return y, stats


def bertnorm_bwd(x, res, gamma, stats, g, *, eps: float = 1e-12, p: float = 0.0, keep=None,
                 need=(True, True, True, True)):
    """(dx, dres, dgamma, dbeta) of `tadmm_bertnorm_bwd` for the upstream gradient `g` (rows, hidden) of y: float32 or
    bfloat16 (float16 is refused).  s and xhat are recomputed from x, res, keep and `stats` (from
    `bertnorm_fwd(need_stats=True)`).  dx and dres are two tensors in the type of x, dgamma and dbeta float32 (hidden,);
    `need` says which of the four are wanted (None for the others; dres is None without `res`).  Two launches (one when
    neither dgamma nor dbeta is wanted), no atomics, bitwise reproducible; nothing synchronises."""
    who = "bertnorm_bwd"
    dsc, hold, (rows, hidden, dev, dt) = _bertnorm_desc(x, res, gamma, None, p, keep, eps, who)
    stats = _operand(stats, who, "stats", (torch.float32,), (rows, 2), layout="copy")
    g = _operand(g, who, "g", (dt,), (rows, hidden), layout="copy")
    dsc.stats, dsc.g = stats.data_ptr(), g.data_ptr()
    want_dx, want_dres, want_dg, want_db = (bool(n) for n in need)
    dx = torch.empty((rows, hidden), dtype=dt, device=dev) if want_dx else None
    dres = torch.empty((rows, hidden), dtype=dt, device=dev) if want_dres and res is not None else None
    dgamma = torch.empty(hidden, dtype=torch.float32, device=dev) if want_dg else None
    dbeta = torch.empty(hidden, dtype=torch.float32, device=dev) if want_db else None
    for name, t in (("dx", dx), ("dres", dres), ("dgamma", dgamma), ("dbeta", dbeta)):
        setattr(dsc, name, None if t is None else t.data_ptr())
    if want_dg or want_db:
        nbytes = bertnorm_workspace_bytes(rows, hidden)
        ws = _scratch(nbytes, dev)
        dsc.workspace, dsc.workspace_bytes = ws.data_ptr(), nbytes
    h = _handle(dev)
    h.check(h.lib.tadmm_bertnorm_bwd(h.ptr, C.byref(dsc), _stream(dev)))
    return dx, dres, dgamma, dbeta


def bertnorm_pays(rows: int, hidden: int, dtype, grad: bool = False) -> bool:
    """True when `functional.residual_layer_norm` sends a call the launch can take to it and not to the composed torch
    route.  A pure function of its arguments.  Measured (scripts/bench_bertlayer.py) at rows = B S
    for B in {1, 8, 32}, S in {64, 128, 512}, hidden in {312, 768, 1024}, float32 and bfloat16, a forward under no_grad
    and a training step with dropout 0.1, against `residual_layer_norm_composed` in the same run.  Up to 4096 rows both
    routes are bound by the host and the composed route is ahead beyond the spread in 88 of 96 classes, level in 8
    (forward 0.018 against 0.024 ms, training step 0.085 against 0.13 - 0.17 ms): F.layer_norm behind one add is two
    native calls, the launch pays its Python descriptor and, in training, three torch calls for the keep mask.  At 16384
    rows the kernel's one pass shows: float32 forward 1.3x - 1.9x at all three widths, float32 training 1.2x at 768 and
    1024 (behind at 312), bfloat16 forward 1.5x at 768 and 1024 (level at 312), bfloat16 training behind everywhere.  So
    the rule goes by the element count rows * hidden, from the smallest class measured ahead: float32 forward from
    16384 x 312, float32 training and 16-bit forward from 16384 x 768, 16-bit training never.  Not measured: row counts
    between 4096 and 16384 and beyond 16384, widths other than the three, float16 (treated as bfloat16)."""
    n = int(rows) * int(hidden)
    if grad:
        return dtype == torch.float32 and n >= 16384 * 768
    return n >= (16384 * 312 if dtype == torch.float32 else 16384 * 768)


# ------------------------------------------------------------------ pre-norm block tail (csrc/prenorm.hip)
PRENORM_DTYPES = BERTNORM_DTYPES


def prenorm_fits(hidden: int, dtype=torch.float32) -> bool:
    """True when the launches take rows of `hidden` columns (`tadmm_prenorm_fits`: 1 <= hidden <= `bertnorm_hmax()`).
    Raises TadmmError for hidden < 1.  Host only."""
    dsc = _cabi.PreNormDesc()
    dsc.hidden, dsc.dtype = int(hidden), PRENORM_DTYPES[dtype]
    rc = _cabi.load().tadmm_prenorm_fits(C.byref(dsc), None)
    if rc < 0:
        raise TadmmError(rc, f"tadmm_prenorm_fits: hidden = {hidden}")
    return rc == 1


def prenorm_workspace_bytes(rows: int, hidden: int) -> int:
    """Bytes of the backward's workspace (`tadmm_prenorm_workspace_bytes`: that of `bertnorm_workspace_bytes`, one
    float32 (2, hidden rounded up to 4) partial per workgroup of the row launch).  Host only."""
    dsc = _cabi.PreNormDesc()
    dsc.rows, dsc.hidden = int(rows), int(hidden)
    size = C.c_size_t()
    rc = _cabi.load().tadmm_prenorm_workspace_bytes(C.byref(dsc), C.byref(size))
    if rc < 0:
        raise TadmmError(rc, f"tadmm_prenorm_workspace_bytes: rows = {rows}, hidden = {hidden}")
    return int(size.value)


def _prenorm_desc(like, gamma, beta, p, keep, p_path, path_keep, rows_per_sample, eps, who):
    """The descriptor fields forward and backward share, for a (rows, hidden) tensor `like` that fixes shape, type and
    device.  Returns (descriptor, tensors to keep alive, (rows, hidden, device, dtype))."""
    like = _operand(like, who, "x", tuple(PRENORM_DTYPES), layout=None)
    if like.dim() != 2 or like.shape[1] < 1:
        raise TadmmError(-1, f"{who}: x must be (rows, hidden >= 1) (got {tuple(like.shape)})")
    rows, hidden = like.shape
    dev, dt = like.device, like.dtype
    nper = int(rows_per_sample)
    if nper < 1 or rows % nper:
        raise TadmmError(-1, f"{who}: {rows} rows are not whole samples of {nper} rows")
    dsc = _cabi.PreNormDesc()
    hold = []
    pdt = gamma.dtype if isinstance(gamma, torch.Tensor) else None
    for name, t in (("gamma", gamma), ("beta", beta)):
        if t is None and name == "beta":
            continue
        t = _operand(t, who, name, (torch.float32, dt), (hidden,), layout="copy")
        if t.dtype != pdt:
            raise TadmmError(-1, f"{who}: gamma and beta must be of one type (got {pdt} and {t.dtype})")
        hold.append(t)
        setattr(dsc, name, t.data_ptr())
    p, p_path = float(p), float(p_path)
    for rate, name, t, shape in ((p, "keep", keep, (rows, hidden)), (p_path, "path_keep", path_keep, (rows // nper,))):
        if rate > 0.0:
            if t is None:
                raise TadmmError(-1, f"{who}: a rate of {rate} needs the {name} tensor")
            if t.dtype == torch.bool:
                t = t.view(torch.uint8)
            t = _operand(t, who, name, (torch.uint8,), shape, layout="copy")
            hold.append(t)
            setattr(dsc, name, t.data_ptr())
    for t in hold:
        if t.device != dev:
            raise TadmmError(-1, f"{who}: an operand on {t.device}, x on {dev}")
    dsc.p, dsc.p_path, dsc.eps = p, p_path, float(eps)
    dsc.rows, dsc.rows_per_sample, dsc.hidden = rows, nper, hidden
    dsc.dtype, dsc.param_dtype = PRENORM_DTYPES[dt], PRENORM_DTYPES[pdt]
    return dsc, hold, (rows, hidden, dev, dt)


def prenorm_fwd(x, b, gamma, beta, *, eps: float = 1e-6, p: float = 0.0, keep=None, p_path: float = 0.0,
                path_keep=None, rows_per_sample: int = 1, need_stats: bool = False):
    """(s, y, stats) of `tadmm_prenorm_fwd`: s = x + b keep / (1 - p) path_keep[sample] / (1 - p_path), y = LayerNorm(s)
    over the last dimension, with the statistics of s as stored.  x, b: (rows, hidden) float32, bfloat16 or float16, read
    in place (unit element stride, any row stride >= hidden, any element alignment); rows = B * `rows_per_sample`.
    `gamma`, `beta`: (hidden,), both float32 or both of the type of x.  `keep` (rows, hidden) and `path_keep` (B,) uint8 /
    bool, read when their rate is > 0.  s and y (rows, hidden) contiguous in the type of x; stats float32 (rows, 2) =
    (mean, 1 / sqrt(var + eps)) (None unless `need_stats`; the backward reads it).  One launch; nothing synchronises."""
    who = "prenorm_fwd"
    dsc, hold, (rows, hidden, dev, dt) = _prenorm_desc(x, gamma, beta, p, keep, p_path, path_keep, rows_per_sample, eps, who)
    x, dsc.x_ld = _bertnorm_rows(x, who, "x", (rows, hidden), dt)
    b, dsc.b_ld = _bertnorm_rows(b, who, "b", (rows, hidden), dt)
    if b.device != dev:
        raise TadmmError(-1, f"{who}: b on {b.device}, x on {dev}")
    dsc.x, dsc.b = x.data_ptr(), b.data_ptr()
    s = torch.empty((rows, hidden), dtype=dt, device=dev)
    y = torch.empty((rows, hidden), dtype=dt, device=dev)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=dev) if need_stats else None
    dsc.s, dsc.y = s.data_ptr(), y.data_ptr()
    dsc.stats = None if stats is None else stats.data_ptr()
    h = _handle(dev)
    h.check(h.lib.tadmm_prenorm_fwd(h.ptr, C.byref(dsc), _stream(dev)))
    return s, y, stats


def prenorm_bwd(s, gamma, stats, g_y, g_s, *, eps: float = 1e-6, p: float = 0.0, keep=None, p_path: float = 0.0,
                path_keep=None, rows_per_sample: int = 1, need=(True, True, True, True)):
    """(dx, db, dgamma, dbeta) of `tadmm_prenorm_bwd` for the gradients `g_y` of y and `g_s` of s ((rows, hidden),
    float32 or bfloat16; either may be None, not both).  `s` and `stats` are what `prenorm_fwd(need_stats=True)`
    returned; x and b are not needed.  dx and db are two tensors in the type of s, dgamma and dbeta float32 (hidden,);
    `need` says which of the four are wanted (None for the others).  Two launches (one when neither dgamma nor dbeta is
    wanted), no atomics, bitwise reproducible; nothing synchronises."""
    who = "prenorm_bwd"
    dsc, hold, (rows, hidden, dev, dt) = _prenorm_desc(s, gamma, None, p, keep, p_path, path_keep, rows_per_sample, eps, who)
    s = _operand(s, who, "s", (dt,), (rows, hidden), layout="copy")
    stats = _operand(stats, who, "stats", (torch.float32,), (rows, 2), layout="copy")
    dsc.s, dsc.stats = s.data_ptr(), stats.data_ptr()
    if g_y is None and g_s is None:
        raise TadmmError(-1, f"{who}: g_y and g_s are both None")
    if g_y is not None:
        g_y = _operand(g_y, who, "g_y", (dt,), (rows, hidden), layout="copy")
        dsc.g_y = g_y.data_ptr()
    if g_s is not None:
        g_s = _operand(g_s, who, "g_s", (dt,), (rows, hidden), layout="copy")
        dsc.g_s = g_s.data_ptr()
    want_dx, want_db, want_dg, want_dbeta = (bool(n) for n in need)
    dx = torch.empty((rows, hidden), dtype=dt, device=dev) if want_dx else None
    db = torch.empty((rows, hidden), dtype=dt, device=dev) if want_db else None
    dgamma = torch.empty(hidden, dtype=torch.float32, device=dev) if want_dg else None
    dbeta = torch.empty(hidden, dtype=torch.float32, device=dev) if want_dbeta else None
    for name, t in (("dx", dx), ("db", db), ("dgamma", dgamma), ("dbeta", dbeta)):
        setattr(dsc, name, None if t is None else t.data_ptr())
    if want_dg or want_dbeta:
        nbytes = prenorm_workspace_bytes(rows, hidden)
        ws = _scratch(nbytes, dev)
        dsc.workspace, dsc.workspace_bytes = ws.data_ptr(), nbytes
    h = _handle(dev)
    h.check(h.lib.tadmm_prenorm_bwd(h.ptr, C.byref(dsc), _stream(dev)))
    return dx, db, dgamma, dbeta


def prenorm_pays(rows: int, hidden: int, dtype, grad: bool = False) -> bool:
    """True when `functional.add_layer_norm` sends a call the launch can take to it and not to the composed torch route.
    A pure function of its arguments.  Measured (scripts/bench_vit_block.py, two runs) at rows =
    197 B for B in {1, 64, 256}, hidden in {192, 384, 768}, float32 and bfloat16, a forward under no_grad and a training
    step with drop_path_p = 0.1, against `add_layer_norm_composed` in the same run.  Up to 12608 x 384 both routes are
    bound by the host and the composed route is ahead or level (forward 0.018 - 0.027 against 0.027 ms, training step
    0.12 - 0.21 against 0.14 - 0.30 ms).  The launch's slowest window is below the composed route's fastest in both runs
    for the forward of both types at 50432 x 192 and 12608 x 768 (one element count; 1.1x - 2.4x) and everything
    larger (1.2x - 1.8x), the float32 training step at 50432 x 384, 12608 x 768 and 50432 x 768 (1.2x - 2.5x; at
    50432 x 192 one run has the composed route ahead), the bfloat16 training step at 50432 rows of all three widths
    (1.4x - 1.9x; behind at 12608 x 768).  So: a forward from 50432 x 192 elements, a float32 training step from
    50432 x 384, a 16-bit training step from 50432 rows of at least 192 columns.  Not measured: row counts between 12608
    and 50432 below 768 columns and beyond 50432, other widths, float16 (treated as bfloat16), dropout on the branch."""
    n = int(rows) * int(hidden)
    if not grad:
        return n >= 50432 * 192
    if dtype == torch.float32:
        return n >= 50432 * 384
    return rows >= 50432 and hidden >= 192


# ------------------------------------------------------------------ ResNet block tail (csrc/bnact.hip)
BNACT_DTYPES = BERTNORM_DTYPES


def _bnact_shape_desc(n, c, h, w, dtype):
    dsc = _cabi.BnActDesc()
    dsc.N, dsc.C, dsc.H, dsc.W, dsc.dtype = int(n), int(c), int(h), int(w), BNACT_DTYPES[dtype]
    return dsc


def bnact_max_m() -> int:
    """The most values per channel (N H W) `tadmm_bnact_fwd` / `_bwd` take (what `tadmm_bnact_fits` reports).  Host only."""
    m = C.c_int64()
    _cabi.load().tadmm_bnact_fits(None, C.byref(m))
    return int(m.value)


def bnact_fits(n: int, c: int, h: int, w: int, dtype=torch.float32) -> bool:
    """True when the launches take an (n, c, h, w) tensor (`tadmm_bnact_fits`: n h w <= `bnact_max_m()`).  Raises
    TadmmError for a dimension < 1.  Host only."""
    rc = _cabi.load().tadmm_bnact_fits(C.byref(_bnact_shape_desc(n, c, h, w, dtype)), None)
    if rc < 0:
        raise TadmmError(rc, f"tadmm_bnact_fits: shape = {(n, c, h, w)}")
    return rc == 1


def bnact_workspace_bytes(n: int, c: int, h: int, w: int, dtype=torch.float32) -> int:
    """Bytes of the workspace of the training forward and of the backward (`tadmm_bnact_workspace_bytes`: a pair of
    doubles per channel and split for min(trips, 128, ceil(2048 / c)) splits, a trip being 1024 float32 or 2048 16-bit
    values; rounded up to 256 bytes; never smaller for a larger n, h or w).  Host only."""
    size = C.c_size_t()
    rc = _cabi.load().tadmm_bnact_workspace_bytes(C.byref(_bnact_shape_desc(n, c, h, w, dtype)), C.byref(size))
    if rc < 0:
        raise TadmmError(rc, f"tadmm_bnact_workspace_bytes: shape = {(n, c, h, w)}")
    return int(size.value)


def bnact_plan(n: int, c: int, h: int, w: int, dtype=torch.float32) -> dict:
    """The ownership `tadmm_bnact_plan` derives from (n h w, c, dtype) alone, as a dict: a channel's n h w values go to
    `S` workgroups of `span` consecutive values each (a whole number of trips of 1024 float32 or 2048 16-bit values);
    the workspace is sized for `cap` splits.  Host only."""
    out = (C.c_int32 * 3)()
    rc = _cabi.load().tadmm_bnact_plan(C.byref(_bnact_shape_desc(n, c, h, w, dtype)), out)
    if rc < 0:
        raise TadmmError(rc, f"tadmm_bnact_plan: shape = {(n, c, h, w)}")
    return dict(zip(("S", "span", "cap"), (int(v) for v in out)))


def _bnact_desc(x, gamma, who):
    """The descriptor fields forward and backward share.  Returns (descriptor, tensors to keep alive, (shape, device,
    dtype))."""
    x = _operand(x, who, "x", tuple(BNACT_DTYPES), layout="copy")
    if x.dim() != 4 or min(x.shape) < 1:
        raise TadmmError(-1, f"{who}: x must be (N, C, H, W) with every dimension >= 1 (got {tuple(x.shape)})")
    n, c, h, w = x.shape
    dsc = _bnact_shape_desc(n, c, h, w, x.dtype)
    gamma = _operand(gamma, who, "gamma", (torch.float32,), (c,), layout="copy")
    if gamma.device != x.device:
        raise TadmmError(-1, f"{who}: gamma on {gamma.device}, x on {x.device}")
    dsc.x, dsc.gamma = x.data_ptr(), gamma.data_ptr()
    return dsc, [x, gamma], ((n, c, h, w), x.device, x.dtype)


def bnact_fwd(x, gamma, beta, running_mean, running_var, res=None, *, c0: int = 0, training: bool, momentum: float = 0.1,
              eps: float = 1e-5, relu: bool = True, num_batches_tracked=None, need_stats: bool = False):
    """(y, stats) of `tadmm_bnact_fwd`: y = act(BatchNorm2d(x) + res) for x (N, C, H, W) float32, bfloat16 or float16
    (a non-contiguous x is copied).  `gamma`, `beta`, `running_mean`, `running_var`: float32 (C,).  `res`: (N, Cr, H, W)
    of the type of x with any non-negative strides, read in place and added to the channels [c0, c0 + Cr).  With
    `training` the batch statistics are used, the running statistics (both or neither) are updated in place with
    `momentum` and the unbiased variance, `num_batches_tracked` (int64 scalar tensor, optional) rises by one, and
    stats is float32 (C, 2) = (mean, 1 / sqrt(var + eps)) when `need_stats` (the backward reads it); two launches.
    Without, the running statistics are read and nothing but y is written; one launch.  Nothing synchronises."""
    who = "bnact_fwd"
    dsc, hold, ((n, c, h, w), dev, dt) = _bnact_desc(x, gamma, who)
    named = [("beta", beta), ("running_mean", running_mean), ("running_var", running_var)]
    for name, t in named:
        if t is None and name != "beta" and training:
            continue
        # updated in place: a copy would take the update with it
        t = _operand(t, who, name, (torch.float32,), (c,), layout="copy" if name == "beta" else "raise")
        hold.append(t)
        setattr(dsc, name, t.data_ptr())
    if num_batches_tracked is not None and training:
        nbt = _operand(num_batches_tracked, who, "num_batches_tracked", (torch.int64,), (), layout="raise")
        hold.append(nbt)
        dsc.num_batches_tracked = nbt.data_ptr()
    if res is not None:
        res = _operand(res, who, "res", (dt,), layout=None)
        if res.dim() != 4 or (res.shape[0], res.shape[2], res.shape[3]) != (n, h, w):
            raise TadmmError(-1, f"{who}: res must be ({n}, Cr, {h}, {w}) (got {tuple(res.shape)})")
        hold.append(res)
        dsc.res, dsc.c0, dsc.Cr = res.data_ptr(), int(c0), res.shape[1]
        for i in range(4):
            dsc.res_stride[i] = res.stride(i)
    for t in hold:
        if t.device != dev:
            raise TadmmError(-1, f"{who}: an operand on {t.device}, x on {dev}")
    dsc.eps, dsc.momentum, dsc.training, dsc.relu = float(eps), float(momentum), int(bool(training)), int(bool(relu))
    y = torch.empty((n, c, h, w), dtype=dt, device=dev)
    stats = torch.empty((c, 2), dtype=torch.float32, device=dev) if need_stats and training else None
    dsc.y = y.data_ptr()
    dsc.stats = None if stats is None else stats.data_ptr()
    if training:
        nbytes = bnact_workspace_bytes(n, c, h, w, dt)
        ws = _scratch(nbytes, dev)
        dsc.workspace, dsc.workspace_bytes = ws.data_ptr(), nbytes
    hd = _handle(dev)
    hd.check(hd.lib.tadmm_bnact_fwd(hd.ptr, C.byref(dsc), _stream(dev)))
    return y, stats


def bnact_bwd(g, y, x, gamma, stats, *, relu: bool = True, c0: int = 0, res_channels: int = 0,
              need=(True, True, True, True)):
    """(dx, dres, dgamma, dbeta) of `tadmm_bnact_bwd` for the gradient `g` of y: float32 or bfloat16 (float16 is
    refused).  `y` is the output as `bnact_fwd(training=True)` stored it (the ReLU mask is y > 0; None without relu),
    `stats` what it returned.  dx in the type and shape of x; dres (N, `res_channels`, H, W) contiguous, the masked
    gradient over the channels [c0, c0 + res_channels) (None when res_channels is 0); dgamma and dbeta float32 (C,).
    `need` says which of the four are wanted (None for the others).  Two launches (one for dres alone), no atomics,
    bitwise reproducible; nothing synchronises."""
    who = "bnact_bwd"
    dsc, hold, ((n, c, h, w), dev, dt) = _bnact_desc(x, gamma, who)
    stats = _operand(stats, who, "stats", (torch.float32,), (c, 2), layout="copy")
    g = _operand(g, who, "g", (dt,), (n, c, h, w), layout="copy")
    dsc.stats, dsc.g = stats.data_ptr(), g.data_ptr()
    if relu:
        y = _operand(y, who, "y", (dt,), (n, c, h, w), layout="copy")
        dsc.y = y.data_ptr()
    want_dx, want_dres, want_dg, want_db = (bool(v) for v in need)
    cr = int(res_channels)
    dx = torch.empty((n, c, h, w), dtype=dt, device=dev) if want_dx else None
    dres = torch.empty((n, cr, h, w), dtype=dt, device=dev) if want_dres and cr > 0 else None
    dgamma = torch.empty(c, dtype=torch.float32, device=dev) if want_dg else None
    dbeta = torch.empty(c, dtype=torch.float32, device=dev) if want_db else None
    for name, t in (("dx", dx), ("dres", dres), ("dgamma", dgamma), ("dbeta", dbeta)):
        setattr(dsc, name, None if t is None else t.data_ptr())
    dsc.c0, dsc.Cr, dsc.relu, dsc.training = int(c0), cr, int(bool(relu)), 1
    if want_dx or want_dg or want_db:
        nbytes = bnact_workspace_bytes(n, c, h, w, dt)
        ws = _scratch(nbytes, dev)
        dsc.workspace, dsc.workspace_bytes = ws.data_ptr(), nbytes
    hd = _handle(dev)
    hd.check(hd.lib.tadmm_bnact_bwd(hd.ptr, C.byref(dsc), _stream(dev)))
    return dx, dres, dgamma, dbeta


def bnact_pays(n: int, c: int, hw: int, dtype, grad: bool = False, residual: bool = False) -> bool:
    """True when `functional.batch_norm_act` sends a call the launch can take to it and not to the composed torch route.
    A pure function of its arguments.  Measured (scripts/bench_resnet_block.py, two runs) at
    (n, c, hw) = CIFAR n in {1, 128} x (16, 1024), (32, 256), (64, 64) and ImageNet n in {1, 32} x (64, 3136), (256, 3136),
    (512, 784), (2048, 49), float32 and bfloat16, without a residual, with a full-width one and (CIFAR, c > 16) with the
    option-A window, a forward in eval mode under no_grad and a training step, against `batch_norm_act_composed` in the
    same run.  Most classes are bound by the host: the launch's floor is 0.021 - 0.027 ms for the forward and 0.087 -
    0.127 ms for the step, the composed route's 0.019 - 0.044 and 0.064 - 0.126.  The launch's slowest window is below
    the composed route's fastest in both runs for
      * the forward with a residual in every class measured (1.03x - 2.5x; option A 1.37x - 1.6x: the slice copy and the
        pad are gone);
      * the forward without one at n >= 32 from 128 x 64 x 64 values and planes of at least 64 (1.07x - 1.9x), not at
        n = 1 (0.88x - 1.0x) and not at 32 x 2048 x 49 (0.9x);
      * the float32 step at 32 x 512 x 784 (1.15x, 1.34x with a residual), 32 x 256 x 3136 (1.38x, 1.44x) and, without a
        residual, 32 x 64 x 3136 (1.33x; with one a window of one run was behind);
      * the bfloat16 step at 32 x 256 x 3136 (1.69x, 1.8x; at 32 x 64 x 3136 1.01x - 1.06x, not taken; at 32 x 512 x 784
        and below the composed route leads, 0.73x - 0.88x).
    Every other step is behind or level (option A level, 0.99x - 1.09x).  So: a forward with a residual always; without,
    from n = 32, hw = 64 and 128 * 64 * 64 values; a float32 step from 32 * 512 * 784 values (32 * 64 * 3136 without a
    residual); a 16-bit step from 32 * 256 * 3136 values.  Not measured: batch sizes between 1 and 32 / 128 and beyond,
    other planes and widths, float16 (treated as bfloat16), a step in eval mode (the composed route takes it)."""
    total = int(n) * int(c) * int(hw)
    if not grad:
        return bool(residual) or (n >= 32 and hw >= 64 and total >= 128 * 64 * 64)
    if dtype == torch.float32:
        return total >= (32 * 512 * 784 if residual else 32 * 64 * 3136)
    return total >= 32 * 256 * 3136


# ------------------------------------------------------------------ DenseNet pre-activation (csrc/densebn.hip)
DENSEBN_DTYPES = BERTNORM_DTYPES


_DENSEBN_ROWS = {}


def _densebn_table(dsc, xs, stats, dxs, channels):
    """Writes the first len(channels) rows of the segment table (data, stats and dx addresses, 0 for NULL, and the
    channel counts) in one call: a ctypes store per field costs more than the launch of a small layer."""
    k = len(channels)
    rows = _DENSEBN_ROWS.get(k)
    if rows is None:
        rows = _DENSEBN_ROWS[k] = struct.Struct("=" + "QQQii" * k)
    rows.pack_into(dsc, 0, *[v for row in zip(xs, stats, dxs, channels) for v in (*row, 0)])


def _densebn_shape_desc(n, channels, h, w, dtype):
    dsc = _cabi.DenseBnDesc()
    channels = [int(c) for c in channels]
    dsc.N, dsc.H, dsc.W, dsc.nseg, dsc.dtype = int(n), int(h), int(w), len(channels), DENSEBN_DTYPES[dtype]
    channels = channels[:_cabi.DENSEBN_MAX_SEGMENTS]
    zeros = [0] * len(channels)
    if channels:
        _densebn_table(dsc, zeros, zeros, zeros, channels)
    return dsc


def densebn_max_segments() -> int:
    """The most feature tensors one `tadmm_densebn_fwd` / `_bwd` call takes (TADMM_DENSEBN_MAX_SEGMENTS: the segment
    table travels in the kernel arguments).  Host only."""
    return int(_cabi.load().tadmm_densebn_max_segments())


def densebn_max_m() -> int:
    """The most values per channel (N H W) the launches take (what `tadmm_densebn_fits` reports).  Host only."""
    m = C.c_int64()
    _cabi.load().tadmm_densebn_fits(None, C.byref(m))
    return int(m.value)


def densebn_fits(n: int, channels: Sequence[int], h: int, w: int, dtype=torch.float32) -> bool:
    """True when the launches take segments of `channels` = (C_0, C_1, ...) channels over an (n, ., h, w) plane
    (`tadmm_densebn_fits`: n h w <= `densebn_max_m()`, at most `densebn_max_segments()` segments).  Raises TadmmError for
    a dimension or a C_k < 1 or an empty list.  Host only."""
    rc = _cabi.load().tadmm_densebn_fits(C.byref(_densebn_shape_desc(n, channels, h, w, dtype)), None)
    if rc < 0:
        raise TadmmError(rc, f"tadmm_densebn_fits: n, channels, h, w = {(n, tuple(channels), h, w)}")
    return rc == 1


def densebn_workspace_bytes(n: int, channels: Sequence[int], h: int, w: int, dtype=torch.float32) -> int:
    """Bytes of the workspace of `densebn_stats` (channels = (C_k,)) and of `densebn_bwd` (every segment's channels)
    (`tadmm_densebn_workspace_bytes`: a pair of doubles per channel and split for min(trips, 128, ceil(2048 / C)) splits,
    C the sum of `channels`, a trip being 1024 float32 or 2048 16-bit values; rounded up to 256 bytes).  Host only."""
    size = C.c_size_t()
    rc = _cabi.load().tadmm_densebn_workspace_bytes(C.byref(_densebn_shape_desc(n, channels, h, w, dtype)), C.byref(size))
    if rc < 0:
        raise TadmmError(rc, f"tadmm_densebn_workspace_bytes: n, channels, h, w = {(n, tuple(channels), h, w)}")
    return int(size.value)


def densebn_plan(n: int, channels: Sequence[int], h: int, w: int, dtype=torch.float32) -> dict:
    """The ownership `tadmm_densebn_plan` derives from (n h w, sum of `channels`, dtype) alone, as `bnact_plan` returns
    it: channels = (C_k,) for the plan of `densebn_stats` on that segment, every segment's channels for the plan of
    `densebn_fwd` and `densebn_bwd`.  Host only."""
    out = (C.c_int32 * 3)()
    rc = _cabi.load().tadmm_densebn_plan(C.byref(_densebn_shape_desc(n, channels, h, w, dtype)), out)
    if rc < 0:
        raise TadmmError(rc, f"tadmm_densebn_plan: n, channels, h, w = {(n, tuple(channels), h, w)}")
    return dict(zip(("S", "span", "cap"), (int(v) for v in out)))


def _densebn_segments(segments, who):
    """The segments checked against the first: (list, (n, channels, h, w), device, dtype)."""
    segments = list(segments)
    if not segments or len(segments) > _cabi.DENSEBN_MAX_SEGMENTS:
        raise TadmmError(-1, f"{who}: 1 .. {_cabi.DENSEBN_MAX_SEGMENTS} segments are taken (got {len(segments)})")
    x0 = _operand(segments[0], who, "segment 0", tuple(DENSEBN_DTYPES))
    if x0.dim() != 4 or min(x0.shape) < 1:
        raise TadmmError(-1, f"{who}: a segment must be (N, C, H, W) with every dimension >= 1 (got {tuple(x0.shape)})")
    n, c0, h, w = x0.shape
    channels = [c0]
    for k in range(1, len(segments)):
        x = segments[k]
        ok = isinstance(x, torch.Tensor) and x.dim() == 4 and x.dtype == x0.dtype and x.device == x0.device \
            and x.is_contiguous()
        if not ok or x.shape[1] < 1 or (x.shape[0], x.shape[2], x.shape[3]) != (n, h, w):
            x = _operand(x, who, f"segment {k}", (x0.dtype,))         # words the common refusals
            raise TadmmError(-1, f"{who}: segment {k} must be ({n}, C, {h}, {w}) on {x0.device} (got {tuple(x.shape)} on "
                                 f"{x.device})")
        channels.append(x.shape[1])
    return segments, (n, channels, h, w), x0.device, x0.dtype


def _densebn_stats_ptrs(stats, channels, dev, who):
    if stats is None or len(stats) != len(channels):
        raise TadmmError(-1, f"{who}: one stats tensor per segment is read")
    for k, st in enumerate(stats):
        ok = isinstance(st, torch.Tensor) and st.dtype == torch.float64 and st.device == dev and st.is_contiguous() \
            and tuple(st.shape) == (channels[k], 2)
        if not ok:
            _operand(st, who, f"stats {k}", (torch.float64,), (channels[k], 2))
            raise TadmmError(-1, f"{who}: stats {k} on {st.device}, the segments on {dev}")
    return [st.data_ptr() for st in stats]


def _densebn_workspace(dsc, dev, who):
    size = C.c_size_t()
    rc = _cabi.load().tadmm_densebn_workspace_bytes(C.byref(dsc), C.byref(size))
    if rc < 0:
        raise TadmmError(rc, f"{who}: tadmm_densebn_workspace_bytes")
    ws = _scratch(size.value, dev)
    dsc.workspace, dsc.workspace_bytes = ws.data_ptr(), size.value
    return ws


def densebn_stats(x, out=None):
    """stats of `tadmm_densebn_stats` for ONE contiguous (N, C, H, W) feature tensor (float32, bfloat16 or float16):
    float64 (C, 2) = (batch mean, biased batch variance) per channel, into `out` where given.  The variance is stored,
    not rstd: every layer that consumes the tensor applies its own eps.  Two launches, no atomics; nothing synchronises."""
    who = "densebn_stats"
    (x,), (n, (c,), h, w), dev, dt = _densebn_segments([x], who)
    stats = _output(out, (c, 2), torch.float64, dev, "stats")
    dsc = _cabi.DenseBnDesc()
    dsc.N, dsc.H, dsc.W, dsc.nseg, dsc.dtype = n, h, w, 1, DENSEBN_DTYPES[dt]
    _densebn_table(dsc, [x.data_ptr()], [stats.data_ptr()], [0], [c])
    _ws = _densebn_workspace(dsc, dev, who)                  # noqa: F841 (held until the launches are queued)
    hd = _handle(dev)
    hd.check(hd.lib.tadmm_densebn_stats(hd.ptr, C.byref(dsc), _stream(dev)))
    return stats


def densebn_fwd(segments, stats, gamma, beta, running_mean, running_var, *, training: bool, momentum: float = 0.1,
                eps: float = 1e-5, relu: bool = True, num_batches_tracked=None):
    """y of `tadmm_densebn_fwd`: act(BatchNorm2d(cat(segments, 1))) as one contiguous (N, sum C_k, H, W) tensor, with no
    concatenation formed.  `segments`: contiguous (N, C_k, H, W) tensors of one type (float32, bfloat16 or float16);
    `stats`: what `densebn_stats` returned for each of them (read with `training`; None otherwise).  `gamma`, `beta`,
    `running_mean`, `running_var`: float32 (sum C_k,), those of the consuming layer.  With `training` the running
    statistics (both or neither) are updated in place with `momentum` and the unbiased variance and
    `num_batches_tracked` (int64 scalar tensor, optional) rises by one.  Without, the running statistics are read and
    nothing but y is written.  One launch either way; nothing synchronises."""
    who = "densebn_fwd"
    segments, (n, channels, h, w), dev, dt = _densebn_segments(segments, who)
    c = sum(channels)
    dsc = _cabi.DenseBnDesc()
    dsc.N, dsc.H, dsc.W, dsc.nseg, dsc.dtype = n, h, w, len(segments), DENSEBN_DTYPES[dt]
    hold = []
    zeros = [0] * len(segments)
    _densebn_table(dsc, [x.data_ptr() for x in segments],
                   _densebn_stats_ptrs(stats, channels, dev, who) if training else zeros, zeros, channels)
    for name, t in (("gamma", gamma), ("beta", beta), ("running_mean", running_mean), ("running_var", running_var)):
        if t is None and name.startswith("running") and training:
            continue
        # the running statistics are updated in place: a copy would take the update with it
        t = _operand(t, who, name, (torch.float32,), (c,), layout="raise" if name.startswith("running") else "copy")
        hold.append(t)
        setattr(dsc, name, t.data_ptr())
    if num_batches_tracked is not None and training:
        nbt = _operand(num_batches_tracked, who, "num_batches_tracked", (torch.int64,), ())
        hold.append(nbt)
        dsc.num_batches_tracked = nbt.data_ptr()
    for t in hold:
        if t.device != dev:
            raise TadmmError(-1, f"{who}: an operand on {t.device}, the segments on {dev}")
    dsc.eps, dsc.momentum, dsc.training, dsc.relu = float(eps), float(momentum), int(bool(training)), int(bool(relu))
    y = torch.empty((n, c, h, w), dtype=dt, device=dev)
    dsc.y = y.data_ptr()
    hd = _handle(dev)
    hd.check(hd.lib.tadmm_densebn_fwd(hd.ptr, C.byref(dsc), _stream(dev)))
    return y


def densebn_bwd(g, y, segments, stats, gamma, *, eps: float = 1e-5, relu: bool = True, need_dx=None,
                need_dgamma: bool = True, need_dbeta: bool = True):
    """(dxs, dgamma, dbeta) of `tadmm_densebn_bwd` for the gradient `g` (N, sum C_k, H, W) of y: float32 or bfloat16
    (float16 is refused).  `y` is the output as `densebn_fwd(training=True)` stored it (the ReLU mask is y > 0; None
    without relu), `segments`, `stats`, `gamma` and `eps` what it was called with.  dxs: one fresh contiguous
    (N, C_k, H, W) gradient per segment, None where `need_dx[k]` is false (a sequence of one flag per segment; None
    wants all) -- such a segment is only summed, and nothing of it is written.  dgamma and dbeta: float32 (sum C_k,) or
    None.  Two launches, no atomics, bitwise reproducible; nothing synchronises."""
    who = "densebn_bwd"
    segments, (n, channels, h, w), dev, dt = _densebn_segments(segments, who)
    c = sum(channels)
    need_dx = [True] * len(segments) if need_dx is None else [bool(v) for v in need_dx]
    if len(need_dx) != len(segments):
        raise TadmmError(-1, f"{who}: need_dx has {len(need_dx)} flags for {len(segments)} segments")
    dsc = _cabi.DenseBnDesc()
    dsc.N, dsc.H, dsc.W, dsc.nseg, dsc.dtype = n, h, w, len(segments), DENSEBN_DTYPES[dt]
    gamma = _operand(gamma, who, "gamma", (torch.float32,), (c,), layout="copy")
    g = _operand(g, who, "g", (dt,), (n, c, h, w), layout="copy")
    dsc.gamma, dsc.g = gamma.data_ptr(), g.data_ptr()
    if relu:
        y = _operand(y, who, "y", (dt,), (n, c, h, w), layout="copy")
        dsc.y = y.data_ptr()
    dxs = [torch.empty_like(x) if want else None for x, want in zip(segments, need_dx)]
    _densebn_table(dsc, [x.data_ptr() for x in segments], _densebn_stats_ptrs(stats, channels, dev, who),
                   [0 if dx is None else dx.data_ptr() for dx in dxs], channels)
    dgamma = torch.empty(c, dtype=torch.float32, device=dev) if need_dgamma else None
    dbeta = torch.empty(c, dtype=torch.float32, device=dev) if need_dbeta else None
    dsc.dgamma = None if dgamma is None else dgamma.data_ptr()
    dsc.dbeta = None if dbeta is None else dbeta.data_ptr()
    dsc.eps, dsc.relu, dsc.training = float(eps), int(bool(relu)), 1
    _ws = _densebn_workspace(dsc, dev, who) if any(need_dx) or need_dgamma or need_dbeta else None      # noqa: F841
    hd = _handle(dev)
    hd.check(hd.lib.tadmm_densebn_bwd(hd.ptr, C.byref(dsc), _stream(dev)))
    return dxs, dgamma, dbeta


def densebn_pays(n: int, c: int, hw: int, nseg: int, dtype, grad: bool = False) -> bool:
    """True when `functional.dense_batch_norm_act` sends a call the launch can take to it and not to the composed torch
    route (`torch.cat` + `F.batch_norm` + relu).  A pure function of its arguments: n the batch, c the channels of the
    concatenation, hw the plane, nseg the feature tensors, grad whether a gradient is wanted.  Measured
    (scripts/bench_densenet_block.py, two runs) at the first, middle and last layer of every block,
    every transition and the final norm of DenseNet-40 (n in {1, 128}; hw 1024, 256, 64; c 32 .. 344; nseg 1, 7, 12, 13)
    and DenseNet-121 (n in {1, 32}; hw 3136, 784, 196, 49; c 64 .. 1024; nseg 1 .. 25), float32 and bfloat16, a forward
    in eval mode under no_grad and a training step in which the launch computes the statistics of the newest feature
    tensor only, against `dense_batch_norm_act_composed` in the same run.  Both routes are bound by the host in most
    classes: the launch costs 0.027 ms + 0.0022 ms per feature tensor for a forward (0.080 ms at 25 tensors) and 0.11 ms +
    0.010 ms per tensor for a step, whatever the sizes measured; the composed route 0.019 - 0.036 ms and 0.063 - 0.19 ms
    at a batch of one.  The launch's slowest window is below the composed route's fastest in both runs for
      * the forward at n = 128 on planes of 1024 and 256 values in every class (1.30x - 2.76x; one tensor 1.3x - 1.6x,
        thirteen tensors at hw 1024 2.7x float32, 2.0x bfloat16), and on the 64-value plane in bfloat16 (1.18x - 1.42x;
        float32 there 0.91x - 1.19x, not taken);
      * the forward at n = 32, hw 3136 from four feature tensors (1.44x - 2.62x); with one tensor the composed route
        leads (0.82x - 0.89x: nothing is concatenated), and on planes of 784 values and below it leads or is level
        (0.46x - 1.02x);
      * the training step at n = 128, hw 1024 with 12 and 13 tensors (208 and 224 channels: 1.51x - 1.66x float32,
        1.19x - 1.26x bfloat16; with 7 tensors and 128 channels one run was ahead, 1.2x, and one behind, 0.7x - 0.8x);
      * the training step at n = 32, hw 3136 with 4, 6 and 7 tensors in float32 (1.41x - 1.94x) and with 6 and 7 in
        bfloat16 (1.29x - 1.36x; with 4 tensors 1.22x, but a window of one run overlapped).
    Every class at a batch of one (0.43x - 0.90x) and every other step (0.51x - 0.95x) is behind.  A whole dense block's
    training step with every BatchNorm forced to the launch is ahead for block 1 of tkr_densenet40 at n = 128 (9.25 -
    9.33 ms against 9.98 - 9.99, 1.07x - 1.08x) and denseblock1 of tkc_densenet121 at n = 32 (6.17 - 6.63 against 6.97 -
    6.98, 1.05x - 1.13x).  So: a forward from n = 128 and hw = 256 (16-bit: hw = 64), or from four tensors on planes of
    at least 3136 values with 32 * 160 * 3136 values in all; a step from four tensors and either 128 * 208 * 1024 values
    or hw >= 3136 with 32 * 160 * 3136 values (16-bit: 32 * 224 * 3136).  Not measured: batch sizes between 1 and 32 /
    128 and beyond, other planes, widths and growth rates, more than 25 feature tensors, float16 (treated as bfloat16),
    a step in eval mode (the composed route takes it)."""
    total = int(n) * int(c) * int(hw)
    wide = dtype == torch.float32
    if not grad:
        if n >= 128 and hw >= (256 if wide else 64):
            return True
        return nseg >= 4 and hw >= 3136 and total >= 32 * 160 * 3136
    if nseg < 4:
        return False
    return total >= 128 * 208 * 1024 or (hw >= 3136 and total >= 32 * (160 if wide else 224) * 3136)


# ------------------------------------------------------------------ MobileNetV2 depthwise stage (csrc/dwbn.hip)
DWBN_DTYPES = BERTNORM_DTYPES


def _dwbn_shape_desc(n, c, h, w, stride, dtype):
    dsc = _cabi.DwBnDesc()
    dsc.N, dsc.C, dsc.H, dsc.W, dsc.stride, dsc.dtype = int(n), int(c), int(h), int(w), int(stride), DWBN_DTYPES[dtype]
    return dsc


def dwbn_out_hw(h: int, w: int, stride: int):
    """(Ho, Wo) of a 3x3 convolution with padding 1: (h - 1) // stride + 1 and (w - 1) // stride + 1."""
    return (int(h) - 1) // int(stride) + 1, (int(w) - 1) // int(stride) + 1


def dwbn_max_w() -> int:
    """The widest plane `tadmm_dwbn_fwd` / `_bwd` take (three haloed rows fit the staged tile).  Host only."""
    m = C.c_int32()
    _cabi.load().tadmm_dwbn_fits(None, C.byref(m))
    return int(m.value)


def dwbn_fits(n: int, c: int, h: int, w: int, stride: int = 1, dtype=torch.float32) -> bool:
    """True when the launches take an (n, c, h, w) tensor (`tadmm_dwbn_fits`: w <= `dwbn_max_w()` and n h w <= 2^31 -
    4096).  Raises TadmmError for a dimension < 1 or a stride other than 1 and 2.  Host only."""
    rc = _cabi.load().tadmm_dwbn_fits(C.byref(_dwbn_shape_desc(n, c, h, w, stride, dtype)), None)
    if rc < 0:
        raise TadmmError(rc, f"tadmm_dwbn_fits: shape = {(n, c, h, w)}, stride = {stride}")
    return rc == 1


def dwbn_plan(n: int, c: int, h: int, w: int, stride: int = 1, dtype=torch.float32) -> dict:
    """The ownership `tadmm_dwbn_plan` derives from the shape alone, as a dict: `G` images share a staged tile (whole
    planes), or the plane is cut into `NB` bands of `RB` output rows (G = 1); a channel's `U` = ceil(n / G) NB units go
    to `S` workgroups of `per` consecutive units each.  The element type does not enter.  Host only."""
    out = (C.c_int32 * 6)()
    rc = _cabi.load().tadmm_dwbn_plan(C.byref(_dwbn_shape_desc(n, c, h, w, stride, dtype)), out)
    if rc < 0:
        raise TadmmError(rc, f"tadmm_dwbn_plan: shape = {(n, c, h, w)}, stride = {stride}")
    return dict(zip(("G", "RB", "NB", "U", "S", "per"), (int(v) for v in out)))


def dwbn_workspace_bytes(n: int, c: int, h: int, w: int, stride: int = 1, dtype=torch.float32) -> int:
    """Bytes of the workspace of the training forward and of the backward (`tadmm_dwbn_workspace_bytes`: eleven doubles
    per channel and split for min(128, ceil(1024 / c)) splits, rounded up to 256 bytes; a function of c alone, so never
    smaller for a larger n, h or w).  Host only."""
    size = C.c_size_t()
    rc = _cabi.load().tadmm_dwbn_workspace_bytes(C.byref(_dwbn_shape_desc(n, c, h, w, stride, dtype)), C.byref(size))
    if rc < 0:
        raise TadmmError(rc, f"tadmm_dwbn_workspace_bytes: shape = {(n, c, h, w)}, stride = {stride}")
    return int(size.value)


def _dwbn_desc(x, conv_weight, gamma, stride, who):
    """The descriptor fields forward and backward share.  Returns (descriptor, tensors to keep alive, (shape, device,
    dtype))."""
    x = _operand(x, who, "x", tuple(DWBN_DTYPES), layout="copy")
    if x.dim() != 4 or min(x.shape) < 1:
        raise TadmmError(-1, f"{who}: x must be (N, C, H, W) with every dimension >= 1 (got {tuple(x.shape)})")
    if int(stride) not in (1, 2):
        raise TadmmError(-1, f"{who}: stride is 1 or 2 (got {stride})")
    n, c, h, w = x.shape
    dsc = _dwbn_shape_desc(n, c, h, w, stride, x.dtype)
    conv_weight = _operand(conv_weight, who, "conv_weight", (torch.float32,), (c, 1, 3, 3), layout="copy")
    gamma = _operand(gamma, who, "gamma", (torch.float32,), (c,), layout="copy")
    for t in (conv_weight, gamma):
        if t.device != x.device:
            raise TadmmError(-1, f"{who}: a parameter on {t.device}, x on {x.device}")
    dsc.x, dsc.w, dsc.gamma = x.data_ptr(), conv_weight.data_ptr(), gamma.data_ptr()
    return dsc, [x, conv_weight, gamma], ((n, c, h, w), x.device, x.dtype)


def dwbn_fwd(x, conv_weight, gamma, beta, running_mean, running_var, *, stride: int, training: bool,
             momentum: float = 0.1, eps: float = 1e-5, num_batches_tracked=None, need_stats: bool = False):
    """(y, z, stats) of `tadmm_dwbn_fwd`: y = relu6(BatchNorm2d(depthwise_conv3x3(x))) for x (N, C, H, W) float32,
    bfloat16 or float16 (a non-contiguous x is copied), `conv_weight` float32 (C, 1, 3, 3), padding 1, `stride` 1 or 2.
    `gamma`, `beta`, `running_mean`, `running_var`: float32 (C,).  With `training` the batch statistics of the
    convolution's output z as stored are used, the running statistics (both or neither) are updated in place with
    `momentum` and the unbiased variance, `num_batches_tracked` (int64 scalar tensor, optional) rises by one, z is
    returned (the backward reads it) and stats is float32 (C, 2) = (mean, 1 / sqrt(var + eps)) when `need_stats`; two
    launches.  Without, the running statistics are read, nothing but y is written and z and stats are None; one launch.
    Nothing synchronises."""
    who = "dwbn_fwd"
    dsc, hold, ((n, c, h, w), dev, dt) = _dwbn_desc(x, conv_weight, gamma, stride, who)
    for name, t in (("beta", beta), ("running_mean", running_mean), ("running_var", running_var)):
        if t is None and name != "beta" and training:
            continue
        # updated in place: a copy would take the update with it
        t = _operand(t, who, name, (torch.float32,), (c,), layout="copy" if name == "beta" else "raise")
        hold.append(t)
        setattr(dsc, name, t.data_ptr())
    if num_batches_tracked is not None and training:
        nbt = _operand(num_batches_tracked, who, "num_batches_tracked", (torch.int64,), (), layout="raise")
        hold.append(nbt)
        dsc.num_batches_tracked = nbt.data_ptr()
    for t in hold:
        if t.device != dev:
            raise TadmmError(-1, f"{who}: an operand on {t.device}, x on {dev}")
    dsc.eps, dsc.momentum, dsc.training = float(eps), float(momentum), int(bool(training))
    ho, wo = dwbn_out_hw(h, w, stride)
    y = torch.empty((n, c, ho, wo), dtype=dt, device=dev)
    z = torch.empty((n, c, ho, wo), dtype=dt, device=dev) if training else None
    stats = torch.empty((c, 2), dtype=torch.float32, device=dev) if need_stats and training else None
    dsc.y = y.data_ptr()
    dsc.z = None if z is None else z.data_ptr()
    dsc.stats = None if stats is None else stats.data_ptr()
    if training:
        nbytes = dwbn_workspace_bytes(n, c, h, w, stride, dt)
        ws = _scratch(nbytes, dev)
        dsc.workspace, dsc.workspace_bytes = ws.data_ptr(), nbytes
    hd = _handle(dev)
    hd.check(hd.lib.tadmm_dwbn_fwd(hd.ptr, C.byref(dsc), _stream(dev)))
    return y, z, stats


def dwbn_bwd(g, y, z, x, conv_weight, gamma, stats, *, stride: int, need=(True, True, True, True)):
    """(dx, dw, dgamma, dbeta) of `tadmm_dwbn_bwd` for the gradient `g` of y: float32 or bfloat16 (float16 is refused).
    `y`, `z` and `stats` are what `dwbn_fwd(training=True, need_stats=True)` returned (the mask is 0 < y < 6).  dx in the
    type and shape of x; dw float32 (C, 1, 3, 3); dgamma and dbeta float32 (C,).  `need` says which of the four are
    wanted (None for the others).  Three launches (two without dw), no atomics, bitwise reproducible; nothing
    synchronises."""
    who = "dwbn_bwd"
    dsc, hold, ((n, c, h, w), dev, dt) = _dwbn_desc(x, conv_weight, gamma, stride, who)
    ho, wo = dwbn_out_hw(h, w, stride)
    stats = _operand(stats, who, "stats", (torch.float32,), (c, 2), layout="copy")
    g = _operand(g, who, "g", (dt,), (n, c, ho, wo), layout="copy")
    y = _operand(y, who, "y", (dt,), (n, c, ho, wo), layout="copy")
    z = _operand(z, who, "z", (dt,), (n, c, ho, wo), layout="copy")
    dsc.stats, dsc.g, dsc.y, dsc.z = stats.data_ptr(), g.data_ptr(), y.data_ptr(), z.data_ptr()
    want_dx, want_dw, want_dg, want_db = (bool(v) for v in need)
    dx = torch.empty((n, c, h, w), dtype=dt, device=dev) if want_dx else None
    dw = torch.empty((c, 1, 3, 3), dtype=torch.float32, device=dev) if want_dw else None
    dgamma = torch.empty(c, dtype=torch.float32, device=dev) if want_dg else None
    dbeta = torch.empty(c, dtype=torch.float32, device=dev) if want_db else None
    for name, t in (("dx", dx), ("dw", dw), ("dgamma", dgamma), ("dbeta", dbeta)):
        setattr(dsc, name, None if t is None else t.data_ptr())
    dsc.training = 1
    if want_dx or want_dw or want_dg or want_db:
        nbytes = dwbn_workspace_bytes(n, c, h, w, stride, dt)
        ws = _scratch(nbytes, dev)
        dsc.workspace, dsc.workspace_bytes = ws.data_ptr(), nbytes
    hd = _handle(dev)
    hd.check(hd.lib.tadmm_dwbn_bwd(hd.ptr, C.byref(dsc), _stream(dev)))
    return dx, dw, dgamma, dbeta


def dwbn_pays(n: int, c: int, h: int, w: int, stride: int, dtype, grad: bool = False) -> bool:
    """True when `functional.depthwise_bn_relu6` sends a call the launch can take to it and not to the composed torch
    route.  A pure function of its arguments.  Measured (scripts/bench_mobilenet_block.py, two runs, DESIGN.md section
    25) at (c, h = w, stride) = CIFAR n in {1, 128} x (32, 32, 1), (96, 32, 1), (144, 32, 1), (192, 32, 2), (384, 16, 1),
    (576, 16, 2), (960, 8, 1) and ImageNet n in {1, 32} x (32, 112, 1), (96, 112, 2), (144, 56, 2), (192, 28, 1),
    (384, 14, 1), (576, 14, 2), (960, 7, 1), float32 and bfloat16, a forward in eval mode under no_grad and a training
    step, against `depthwise_bn_relu6_composed` in the same run.  The launch's floor is 0.023 - 0.026 ms for the forward
    and 0.102 - 0.112 ms for the step, the composed route's 0.043 - 0.047 and 0.137 - 0.146 ms: torch's grouped
    convolution, batch norm and hardtanh are three to four launches forward and more backward.  The launch's slowest
    window is below the composed route's fastest in both runs for
      * the forward in all 56 classes (n = 1: 1.5x - 2.8x; n = 128 / 32: 1.2x - 7.0x, 5x - 7x for the CIFAR classes from
        96 channels);
      * the bfloat16 step in all 28 classes (n = 1: 1.1x - 2.6x; n = 128 / 32: 3.1x - 30x: torch's bfloat16 depthwise
        weight gradient is slow);
      * the float32 step in 26 of 28 classes (n = 1: 1.3x - 1.9x; n = 128 / 32: 2.8x - 14x).  At 1 x 32 x 32 x 32 and
        1 x 192 x 32 x 32 (stride 2) one run had a launch window inside the composed route's spread (0.69x - 2.1x), so
        those two are not taken.
    So: every forward; every 16-bit step; a float32 step unless n == 1 with fewer than 2^18 input values per image, which
    keeps the two classes that were not ahead in both runs, and the six batch-1 classes below that size that were, with
    the composed route.  Not measured: batch sizes between 1 and 32 / 128 and beyond, planes that are not square, other
    widths, float16 (treated as bfloat16), a step in eval mode (the composed route takes it)."""
    if not grad or dtype != torch.float32:
        return True
    return not (int(n) == 1 and int(c) * int(h) * int(w) < 2 ** 18)
