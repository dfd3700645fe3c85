"""Differentiable building blocks on top of the HIP grouped GEMM.

`mm(a, b)` is the one contraction primitive of the factorised layers: forward and both gradients run
on the fp32 matrix cores through `tadmm_gemm_run`, with transposes expressed as operand strides (no
materialised `.t()`), replacing the `torch.mm` / `F.linear` calls of TTLinear.py:79-86,
TTConv.py:133-147, TKConv.py:210-214 and TKLinear.py:66-71.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ops
from ._cabi import TadmmError


def _as_gemm_operand(t: torch.Tensor) -> torch.Tensor:
    """Return a 2-D float32 device view with one unit stride (copying only if there is none)."""
    if t.dim() != 2:
        raise ValueError("mm expects 2-D operands")
    if not t.is_cuda:
        raise TadmmError(-1, "mm operands must live on the HIP device (no CPU fallback)")
    if t.dtype != torch.float32:
        t = t.float()
    if 1 not in t.stride():
        t = t.contiguous()
    return t


class _Mm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, bias_n):
        a_, b_ = _as_gemm_operand(a), _as_gemm_operand(b)
        ctx.save_for_backward(a_, b_)
        ctx.has_bias = bias_n is not None
        return ops.mm(a_, b_, bias_n=bias_n)

    @staticmethod
    def backward(ctx, g):
        a_, b_ = ctx.saved_tensors
        g_ = _as_gemm_operand(g)
        ga = gb = gbias = None
        if ctx.needs_input_grad[0]:
            ga = ops.mm(g_, b_.t())            # dA = dC B^T   (B^T is a stride swap)
        if ctx.needs_input_grad[1]:            # dB = A^T dC
            gb = ops.wgrad(a_, g_) if mm_wgrad_pays(a_, g_) else ops.mm(a_.t(), g_)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gbias = g.sum(0)
        return ga, gb, gbias


_MM_WGRAD_MIN_T = 512


def mm_wgrad_pays(a: torch.Tensor, g: torch.Tensor) -> bool:
    """True when `dB = A^T dC` of `mm` goes to the split-T kernel (`ops.wgrad`); False: `ops.mm`, which keeps the short
    reductions of the core contractions that share `_Mm`.  A pure function of the shapes and strides: both operands are
    token rows (unit feature stride, so nothing is copied) and the reduction has at least `_MM_WGRAD_MIN_T` rows.
    Measured (`scripts/bench_wgrad.py --threshold`): the two routes cross between 128 and 256 rows,
    where their spreads still overlap; from 512 rows the kernel is ahead beyond the spread at every (M, N) of the sweep
    (1.8x - 2.5x there, growing linearly with the rows).  Reductions of 512 rows and more also occur in the later steps
    of `_chain_recover` (up to out_features rows); they switch as well, which is what the sweep favours."""
    return a.shape[0] >= _MM_WGRAD_MIN_T and a.stride(1) == 1 and g.stride(1) == 1 and a.shape[1] > 0 and g.shape[1] > 0


def mm(a: torch.Tensor, b: torch.Tensor, bias_n: torch.Tensor = None) -> torch.Tensor:
    """(M,K) @ (K,N) [+ bias over N] on the MI355X matrix cores; differentiable."""
    return _Mm.apply(a, b, bias_n)


def linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor = None) -> torch.Tensor:
    """F.linear semantics: x (..., in) @ weight(out, in)^T + bias."""
    lead = x.shape[:-1]
    y = mm(x.reshape(-1, x.shape[-1]), weight.t(), bias)
    return y.reshape(*lead, weight.shape[0])


# ---------------------------------------------------------------------------------------------------------------
# Forward chains on the bf16 matrix cores (csrc/chain.hip): one launch per chain, the per-token intermediate of the
# fused TT-linear chain stays in LDS.  float32 tensors go through the exact three-plane bf16 split (fp32-GEMM
# accuracy), bfloat16 tensors through one plane.  float16 tensors (inference only: what the reference's evaluate() under
# autocast hands a layer) run the one-plane kernels with ONE binary16 plane.
# ---------------------------------------------------------------------------------------------------------------
def planes_of(w: torch.Tensor, nplanes: int, pad_rows: int = 16, pad_cols: int = 32, transpose: bool = False,
              cache: dict = None, tag=None, like: torch.Tensor = None):
    """Fragment-major planes of a 2-D weight (`ops.weight_planes`): bfloat16, or binary16 when `like` -- the activations
    the planes will multiply -- is float16.  With `cache` (a dict owned by the layer) the packing is reused until the
    weight's version counter or storage address changes -- inference packs a layer once (`param_key` for what that
    cannot see); the plane dtype is part of the key, so bfloat16 and float16 planes of one weight are kept side by side here
    (the layers' contracted-factor caches hold one entry and repack when the activation dtype changes)."""
    pdt = plane_dtype(like)
    key = None
    if cache is not None:
        key = (tag, (w._version, w.data_ptr()), tuple(w.shape), nplanes, pad_rows, pad_cols, transpose, pdt)
        hit = cache.get(key)
        if hit is not None:
            return hit
    src = w.detach()
    wp = ops.weight_planes(src.t() if transpose else src, nplanes, pad_rows, pad_cols, dtype=pdt)
    if cache is not None:
        for k in [k for k in cache if k[0] == tag and k[3:] == key[3:]]:
            del cache[k]                                            # older versions of the same weight
        cache[key] = wp
    return wp


def param_key(*params):
    """Identity of a set of parameters for the inference caches: version counter AND storage address.  `p.data = t`
    re-points the storage without touching the counter; an in-place write THROUGH `.data` (`p.data.copy_(t)`,
    `p.data.mul_()`) changes neither -- nothing observable from the outside does -- so the layers also drop their
    caches on `train()` / `eval()`, `_apply` (`.to()`, `.half()`) and `load_state_dict`, and expose
    `invalidate_caches()` for callers that write through `.data` between two inference calls."""
    return tuple((p._version, p.data_ptr()) for p in params if p is not None)


class InferenceCacheMixin:
    """Inference-only caches of the factorised layers (contracted factors, packed bf16 planes): see `param_key`."""
    _CACHE_ATTRS = ("_chain_cache", "_plane_cache", "_fused_cache", "_core_cache")

    def invalidate_caches(self):
        for a in self._CACHE_ATTRS:
            self.__dict__.pop(a, None)

    def train(self, mode: bool = True):
        self.invalidate_caches()
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_caches()
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self.invalidate_caches()
        return super()._load_from_state_dict(*args, **kwargs)


def _nplanes(x: torch.Tensor) -> int:
    if x.dtype == torch.float32:
        return 3
    if x.dtype in (torch.bfloat16, torch.float16):
        return 1
    raise TadmmError(-1, f"chain kernels take float32, bfloat16 or (inference) float16 activations (got {x.dtype})")


def plane_dtype(x: torch.Tensor = None) -> torch.dtype:
    """dtype of the weight planes that multiply activations x: binary16 for float16, bfloat16 otherwise (float32
    activations read three bfloat16 planes)."""
    return torch.float16 if x is not None and x.dtype == torch.float16 else torch.bfloat16


def chain_dtype_ok(x: torch.Tensor, *params) -> bool:
    """True when the chain kernels take x on behalf of a layer with these parameters: float32 and bfloat16 always,
    float16 for inference only -- nothing among x and the parameters may want a gradient (there is no float16 weight
    gradient; grad mode keeps the per-core route)."""
    if x.dtype in (torch.float32, torch.bfloat16):
        return True
    return x.dtype == torch.float16 and not _needs_grad(x, *params)


def _inference_only(x: torch.Tensor):
    if x.dtype == torch.float16:
        raise TadmmError(-1, "float16 activations are inference only: nothing they meet may require a gradient")


def _needs_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def fused_rank_ok(r: int) -> bool:
    """The fused chain keeps a token's middle-rank vector in LDS: ranks up to 256 (padded to a multiple of 64)."""
    return 0 < r <= 256


def _chain_planes(x: torch.Tensor, w_in: torch.Tensor, w_out: torch.Tensor = None, given=None, transpose: bool = False):
    """(planes, memo) of one chain launch on activations x: the planes of a single map `w_in`, or the pair of the fused
    chain through `w_in` then `w_out` (middle rank padded to 64); with `transpose` those of the data gradient, which runs
    the same kernels on the transposed factors in the opposite order.  `given`: prebuilt planes (the layers' inference
    caches), passed through.  Planes packed here live for this call only, so memo is False: they stay out of the launch
    memo (`ops._CHAIN_MEMO`)."""
    if given is not None:
        return given, True
    n = _nplanes(x)
    if w_out is None:
        return planes_of(w_in, n, transpose=transpose, like=x), False
    if transpose:
        return (planes_of(w_out, n, pad_rows=64, transpose=True), planes_of(w_in, n, pad_cols=64, transpose=True)), False
    return (planes_of(w_in, n, pad_rows=64, like=x), planes_of(w_out, n, pad_cols=64, like=x)), False


class _ChainSingle(torch.autograd.Function):
    """y = x W^T + bias on token rows (T, K) or, in place, on channels-first images (B, K, H, W) -> (B, N, H, W)."""

    @staticmethod
    def forward(ctx, x, w, bias, entry, wp):
        if not x.is_cuda:
            raise TadmmError(-1, "chain operands must live on the HIP device (no CPU fallback)")
        _inference_only(x)
        image = x.dim() == 4
        wp, memo = _chain_planes(x, w, given=wp)
        y = ops.chain_single(x, wp, bias, w.shape[0], entry=entry, image_out=image, memo=memo)
        ctx.save_for_backward(x, w)
        ctx.entry, ctx.has_bias, ctx.image = entry, bias is not None, image
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:                 # dX = dY W : the same kernel with the transposed weight
            wp, memo = _chain_planes(g, w, transpose=True)
            gx = ops.chain_single(g, wp, None, w.shape[1], entry=ctx.entry, image_out=ctx.image, memo=memo)
        if ctx.needs_input_grad[1]:                 # dW = dY^T X  (N x K) over tokens / pixels, operands in place
            gw = ops.wgrad(g, x)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = g.sum((0, 2, 3)) if ctx.image else g.sum(0)
        return gx, gw, gb, None, None


def pointwise(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor = None, entry: str = "tadmm_tucker_1x1",
              planes: torch.Tensor = None):
    """Per-token / per-pixel linear map `x W^T + bias` with W (N, K): rows (..., K) or an image (B, K, H, W) in place
    (the 1x1 convolutions of TKConv.py:93-98 and the core chains of TTConv.py:131-151).  Differentiable.  `planes`:
    prebuilt `planes_of(w, ...)` (inference caches)."""
    if not _needs_grad(x, w, bias):                   # inference: straight to the C ABI, no autograd node
        planes, memo = _chain_planes(x, w, given=planes)
        if x.dim() == 4:
            return ops.chain_single(x, planes, bias, w.shape[0], entry=entry, image_out=True, memo=memo)
        lead = x.shape[:-1]
        return ops.chain_single(x.reshape(-1, x.shape[-1]), planes, bias, w.shape[0], entry=entry,
                                memo=memo).reshape(*lead, w.shape[0])
    if x.dim() == 4:
        return _ChainSingle.apply(x.contiguous(), w, bias, entry, planes)
    lead = x.shape[:-1]
    return _ChainSingle.apply(x.reshape(-1, x.shape[-1]), w, bias, entry, planes).reshape(*lead, w.shape[0])


# What tells the fused chain on token rows (T, K) from the one on NCHW images, keyed on x.dim() == 4: the `ops` wrappers
# (looked up at call time), the prefix of the entry names, how the recomputing `ops.chain_single` launches are addressed
# and the dims the bias gradient sums over.
_CHAIN_LAYOUTS = {
    False: ("chain_fused", "chain_fused_save", "tadmm_ttlinear_", {}, 0),
    True: ("svd_conv", "svd_conv_save", "tadmm_svdconv_", dict(entry="tadmm_tucker_1x1", image_out=True), (0, 2, 3)),
}


class _FusedChain(torch.autograd.Function):
    """y = Wout (Win x) + bias in one launch, per token of rows (T, K) or per pixel of an NCHW image (`_CHAIN_LAYOUTS`);
    Win (R, K), Wout (N, R), R <= 256.  On the saved route (`save`: None = `ops.chain_train_pays` decides, True / False =
    the caller does; with no factor gradient wanted there is nothing to save either way) the forward launch also stores
    H = Win x and the data-gradient launch dH = Wout^T dY, and the two weight gradients read them: four launches a step
    and no recomputation, for T x R elements (H) kept alive from forward to backward that the other route does not keep."""

    @staticmethod
    def forward(ctx, x, w_in, w_out, bias, planes, save):
        if not x.is_cuda:
            raise TadmmError(-1, "chain operands must live on the HIP device (no CPU fallback)")
        _inference_only(x)
        image = x.dim() == 4
        plain, saving = _CHAIN_LAYOUTS[image][:2]
        (p_in, p_out), memo = _chain_planes(x, w_in, w_out, planes)
        factor_grad = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        ctx.saved_route = bool(factor_grad and save is not False and (
            save or ops.chain_train_pays(x, w_in.shape[0], w_in.shape[1], w_out.shape[0], image)))
        h = None
        if ctx.saved_route and ctx.needs_input_grad[2]:              # H feeds dWout alone
            y, h = getattr(ops, saving)(x, p_in, p_out, bias, w_out.shape[0], w_in.shape[0])
        else:
            y = getattr(ops, plain)(x, p_in, p_out, bias, w_out.shape[0], memo=memo)
        ctx.save_for_backward(x, w_in, w_out, h)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, w_in, w_out, h = ctx.saved_tensors
        plain, saving, prefix, single, bias_dims = _CHAIN_LAYOUTS[x.dim() == 4]
        need = ctx.needs_input_grad
        g = g.contiguous()
        gx = gr = gwi = gwo = gb = None
        if need[0]:                                 # dX = Win^T (Wout^T dY): the fused kernel on the transposed factors
            (p_out, p_in), memo = _chain_planes(g, w_in, w_out, transpose=True)
            if ctx.saved_route and need[1]:         # ... and dH = Wout^T dY from the same launch
                gx, gr = getattr(ops, saving)(g, p_out, p_in, None, w_in.shape[1], w_in.shape[0], entry=prefix + "bwd_save")
            else:
                gx = getattr(ops, plain)(g, p_out, p_in, None, w_in.shape[1], entry=prefix + "bwd", memo=memo)
        # (the weight gradients are float32; `.to` is the identity for float32 factors, and autograd would cast a
        # mismatched gradient to the factor's dtype anyway)
        if need[1]:                                 # dWin = (Wout^T dY) X^T over all tokens / pixels
            if gr is None:                          # no fused launch delivered it: product 1 alone
                wp, memo = _chain_planes(g, w_out, transpose=True)
                gr = ops.chain_single(g, wp, None, w_out.shape[1], memo=memo, **single)
            gwi = ops.wgrad(gr, x).to(w_in.dtype)
            del gr                                  # released before the other intermediate is made
        if need[2]:                                 # dWout = dY (Win X)^T, H from the forward launch where it saved it
            if h is None:
                wp, memo = _chain_planes(x, w_in)
                h = ops.chain_single(x, wp, None, w_in.shape[0], memo=memo, **single)
            gwo = ops.wgrad(g, h).to(w_out.dtype)
        if ctx.has_bias and need[3]:
            gb = g.sum(bias_dims)
        return gx, gwi, gwo, gb, None, None


def linear_chain(x: torch.Tensor, w_in: torch.Tensor, w_out: torch.Tensor, bias: torch.Tensor = None, planes=None,
                 save=None):
    """(..., K) -> (..., N): x Win^T Wout^T + bias through the fused chain kernel (TTLinear.py:75-93 with the input
    cores contracted into Win and the output cores into Wout).  Differentiable.  `planes`: prebuilt
    (planes_of(w_in, n, pad_rows=64), planes_of(w_out, n, pad_cols=64)).
    `save` picks the route of a training step in which a factor wants a gradient.  True: the forward launch stores
    H = x Win^T (`tadmm_ttlinear_fwd_save`), the data-gradient launch stores dH = dY Wout (`tadmm_ttlinear_bwd_save`), and
    the weight gradients are `ops.wgrad(dH, x)` and `ops.wgrad(dY, H)`: four launches, nothing recomputed, at the price of
    T x R elements of x's dtype (H, rows padded to 16 bytes) alive from forward to backward.  False: both intermediates
    are recomputed in the backward by two `ops.chain_single` launches and nothing extra is kept.  None:
    `ops.chain_train_pays` decides.  dX is bit-identical on both routes."""
    lead = x.shape[:-1]
    if not _needs_grad(x, w_in, w_out, bias):         # inference: straight to the C ABI, no autograd node
        # (given planes go round the helper: this is what TTLinearM's fast path calls, and a Python frame shows there)
        (p_in, p_out), memo = (planes, True) if planes is not None else _chain_planes(x, w_in, w_out)
        return ops.chain_fused(x.reshape(-1, x.shape[-1]), p_in, p_out, bias, w_out.shape[0],
                               memo=memo).reshape(*lead, w_out.shape[0])
    return _FusedChain.apply(x.reshape(-1, x.shape[-1]), w_in, w_out, bias, planes, save).reshape(*lead, w_out.shape[0])


def conv1x1_chain(x: torch.Tensor, w_in: torch.Tensor, w_out: torch.Tensor, bias: torch.Tensor = None, planes=None,
                  save=None):
    """(B, C, H, W) -> (B, N, H, W): the 1x1 convolution with the rank-R factorisation Wout Win (SVDConv.py) as one launch
    of the fused chain on the NCHW tensors in place (`tadmm_svdconv_fwd`).  Differentiable; the data gradient is one
    `tadmm_svdconv_bwd` launch.  `planes`: prebuilt (planes_of(w_in, n, pad_rows=64), planes_of(w_out, n, pad_cols=64)).
    `save` as for `linear_chain`: True stores H = Win x in the forward launch and dH = Wout^T dY in the data-gradient
    launch (`tadmm_svdconv_fwd_save` / `_bwd_save`) for the two weight gradients, keeping B x R x H x W elements of x's
    dtype alive from forward to backward; False recomputes both; None: `ops.chain_train_pays` decides."""
    if x.dim() != 4:
        raise ValueError("conv1x1_chain expects an NCHW image")
    if not fused_rank_ok(w_in.shape[0]):
        raise TadmmError(-5, f"conv1x1_chain: rank {w_in.shape[0]} does not fit the fused kernel (at most 256)")
    if not _needs_grad(x, w_in, w_out, bias):         # inference: straight to the C ABI, no autograd node
        (p_in, p_out), memo = _chain_planes(x, w_in, w_out, planes)
        return ops.svd_conv(x, p_in, p_out, bias, w_out.shape[0], memo=memo)
    return _FusedChain.apply(x.contiguous(), w_in, w_out, bias, planes, save)


# ---------------------------------------------------------------------------------------------------------------
# The k x k core convolution between the two 1x1 stages (csrc/coreconv.hip, csrc/wgrad.hip): forward, data gradient
# (the same kernel with a transposed gather) and weight gradient (split over batch * output pixels, deterministic).
# ---------------------------------------------------------------------------------------------------------------
class _CoreConv(torch.autograd.Function):
    """y = conv2d(x, core) with groups = 1 on NCHW images in place; core (r2, r1, kh, kw)."""

    @staticmethod
    def forward(ctx, x, core, stride, padding, dilation, planes):
        if not x.is_cuda:
            raise TadmmError(-1, "core conv operands must live on the HIP device (no CPU fallback)")
        fresh = planes is None                      # planes packed for this call only: keep them out of the launch memo
        if fresh:
            planes = ops.conv_core_planes(core, _nplanes(x))
        y = ops.core_conv(x, planes, core.shape[0], core.shape[2:], stride, padding, dilation, memo=not fresh)
        ctx.save_for_backward(x, core)
        ctx.geom = (tuple(core.shape[2:]), stride, padding, dilation)
        return y

    @staticmethod
    def backward(ctx, g):
        x, core = ctx.saved_tensors
        ksize, stride, padding, dilation = ctx.geom
        g = g.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:                 # dX: the same kernel, transposed gather, planes of the transposed core
            gx = ops.core_conv_dgrad(g, ops.conv_core_planes(core.permute(1, 0, 2, 3), _nplanes(g)), x.shape, ksize,
                                     stride, padding, dilation, memo=False)
        if ctx.needs_input_grad[1]:                 # dWc over (batch, output pixel), float32, cast to the parameter's dtype
            gw = ops.core_conv_wgrad(g, x, ksize, stride, padding, dilation).to(core.dtype)
        return gx, gw, None, None, None, None


def core_conv(x: torch.Tensor, core: torch.Tensor, stride=1, padding=0, dilation=1, cache: dict = None):
    """(B, r1, H, W) -> (B, r2, Ho, Wo): `F.conv2d(x, core, None, stride, padding, dilation, 1)` on the native kernel
    (`tadmm_core_conv_fwd` / `_dgrad` / `_wgrad`).  Differentiable.  `cache` (a dict owned by the layer): in inference
    the packed planes are reused until the core's version counter or storage address changes (`param_key`)."""
    if x.dim() != 4 or core.dim() != 4 or x.shape[1] != core.shape[1]:
        raise ValueError("core_conv expects an NCHW image and a (r2, r1, kh, kw) core with r1 = the image's channels")
    stride, padding, dilation = ops._pair(stride), ops._pair(padding), ops._pair(dilation)
    if _needs_grad(x, core):
        return _CoreConv.apply(x.contiguous(), core, stride, padding, dilation, None)
    n = _nplanes(x)
    planes = None
    if cache is not None:
        key = ("core", n, x.device, param_key(core), tuple(core.shape))
        if cache.get("core_key") != key:
            cache.update(core_key=key, core_planes=ops.conv_core_planes(core, n))
        planes = cache["core_planes"]
    fresh = planes is None
    if fresh:
        planes = ops.conv_core_planes(core, n)
    return ops.core_conv(x, planes, core.shape[0], core.shape[2:], stride, padding, dilation, memo=not fresh)


def conv_stages(layer, x: torch.Tensor, w_in: torch.Tensor, w_out: torch.Tensor, entries, planes=None):
    """A factorised convolution layer as three launches: (f1, f2, f3) = the 1x1 map `w_in` (entries[0]) on the NCHW tensor
    as it stands (no NHWC copies), the k x k convolution with `layer.core_kernel` -- the native kernel of csrc/coreconv.hip
    where `ops.core_conv_pays` routes it there (its planes cached on the layer in inference), else the device library's
    conv2d -- and the 1x1 map `w_out` + `layer.bias` (entries[1], bias in the epilogue).  Differentiable.  `planes`: the
    caller's prebuilt (planes_of(w_in, n), planes_of(w_out, n)); without them, outside grad mode, the layer's
    `_plane_cache` holds them."""
    n = _nplanes(x)
    p_in, p_out = planes if planes is not None else (None, None)
    cache = None if planes is not None or torch.is_grad_enabled() else layer.__dict__.setdefault("_plane_cache", {})
    if cache is not None:
        p_in = planes_of(w_in, n, cache=cache, tag="first", like=x)
    f1 = pointwise(x, w_in, None, entries[0], p_in)
    core = layer.core_kernel
    grad = _needs_grad(f1, core)
    if layer.groups == 1 and ops.core_conv_pays(f1, core.shape[0], layer.kernel_size, layer.stride, layer.padding,
                                                layer.dilation, layer.groups, training=grad):
        f2 = core_conv(f1, core, layer.stride, layer.padding, layer.dilation,
                       cache=None if grad else layer.__dict__.setdefault("_core_cache", {}))
    else:
        f2 = F.conv2d(f1, core if x.dtype == core.dtype else core.to(x.dtype), None, layer.stride, layer.padding,
                      layer.dilation, layer.groups)
    if cache is not None:
        p_out = planes_of(w_out, n, cache=cache, tag="last", like=x)
    return f1, f2, pointwise(f2, w_out, layer.bias, entries[1], p_out)


# ---------------------------------------------------------------------------------------------------------------
# The whole factorised convolution y = W3 conv_kxk(W1 x; Wc) + b of a small plane as ONE launch forward and ONE launch
# for the data gradient (csrc/convchain.hip): both intermediates stay in LDS, and only a step that trains a factor
# stores them (H1, H2 forward; dH1, dH2 backward) for the three weight gradients.
# ---------------------------------------------------------------------------------------------------------------
# dWc through `ops.core_conv_wgrad` (float32, deterministic) rather than the device library's weight gradient: the faster of
# the two inside `conv_chain` at 25 of 30 bf16 and 18 of 22 fp32 layers (scripts/bench_conv_train.py)
CONV_CHAIN_DWC_NATIVE = True


def _core_wgrad_library(h1, dh2, core, stride, padding, dilation):
    w = core.detach().to(h1.dtype)
    return torch.ops.aten.convolution_backward(dh2, h1, w, None, list(stride), list(padding), list(dilation), False, [0, 0],
                                               1, [False, True, False])[1]


def _core_dgrad_library(dh2, h1_shape, core, stride, padding, dilation):
    w = core.detach().to(dh2.dtype)
    h1 = dh2.new_empty(h1_shape)                      # the data gradient reads the input's shape only
    return torch.ops.aten.convolution_backward(dh2, h1, w, None, list(stride), list(padding), list(dilation), False, [0, 0],
                                               1, [True, False, False])[0]


def _conv_chain_planes(w_in, core, w_out, n, transposed, pdt=torch.bfloat16):
    if transposed:                                    # nothing is flipped: the kernel's transposed gather maps the taps
        return (ops.weight_planes(w_out.detach().t(), n, pad_rows=32, dtype=pdt),
                ops.conv_core_planes(core.permute(1, 0, 2, 3), n, dtype=pdt), ops.weight_planes(w_in.detach().t(), n, dtype=pdt))
    return (ops.weight_planes(w_in.detach(), n, pad_rows=32, dtype=pdt), ops.conv_core_planes(core, n, dtype=pdt),
            ops.weight_planes(w_out.detach(), n, dtype=pdt))


def _cached_conv_chain_planes(cache, w_in, core, w_out, n, device, transposed, pdt=torch.bfloat16):
    if cache is None:
        return _conv_chain_planes(w_in, core, w_out, n, transposed, pdt)
    tag = "tplanes_t" if transposed else "tplanes"
    key = (n, pdt, device, param_key(w_in, core, w_out))
    if cache.get(tag + "_key") != key:
        cache[tag + "_key"], cache[tag] = key, _conv_chain_planes(w_in, core, w_out, n, transposed, pdt)
    return cache[tag]


class _ConvChain(torch.autograd.Function):
    """y = W3 conv_kxk(W1 x; Wc) + bias on NCHW images; W1 (r1, C), Wc (r2, r1, kh, kw), W3 (O, r2)."""

    @staticmethod
    def forward(ctx, x, w_in, core, w_out, bias, stride, padding, dilation, cache):
        if not x.is_cuda:
            raise TadmmError(-1, "conv chain operands must live on the HIP device (no CPU fallback)")
        _inference_only(x)
        n = _nplanes(x)
        ksize = tuple(core.shape[2:])
        r1, r2 = w_in.shape[0], w_out.shape[1]
        train = any(ctx.needs_input_grad[1:4])      # a factor wants a gradient: the launch also stores H1 and H2
        p1, p2, p3 = _cached_conv_chain_planes(None if train else cache, w_in, core, w_out, n, x.device, False)
        if train:
            y, h1, h2 = ops.conv_chain_save(x, p1, p2, p3, bias, w_out.shape[0], r1, r2, ksize, stride, padding, dilation)
            ctx.save_for_backward(w_in, core, w_out, x, h1, h2)
        else:
            y = ops.conv_chain(x, p1, p2, p3, bias, w_out.shape[0], ksize, stride, padding, dilation, memo=cache is not None)
            ctx.save_for_backward(w_in, core, w_out)
        ctx.train, ctx.cache, ctx.x_shape, ctx.has_bias = train, cache, tuple(x.shape), bias is not None
        ctx.geom = (ksize, stride, padding, dilation)
        return y

    @staticmethod
    def backward(ctx, g):
        w_in, core, w_out = ctx.saved_tensors[:3]
        x, h1, h2 = ctx.saved_tensors[3:] if ctx.train else (None, None, None)
        ksize, stride, padding, dilation = ctx.geom
        need = ctx.needs_input_grad
        g = g.contiguous()
        n = _nplanes(g)
        r1, r2 = w_in.shape[0], w_out.shape[1]
        gx = gwi = gc = gwo = gb = None
        want_h = need[1] or need[2]                     # dW_in reads dH1, dWc reads dH2
        if need[0] or want_h:
            if ops._conv_chain_bwd_plan(ctx.x_shape, g.dtype, r1, r2, ksize, stride, padding, dilation) is not None:
                planes = _cached_conv_chain_planes(None if ctx.train else ctx.cache, w_in, core, w_out, n, g.device, True)
                out = ops.conv_chain_bwd(g, *planes, ctx.x_shape, r1, r2, ksize, stride, padding, dilation, save=want_h)
                gx, dh1, dh2 = out if want_h else (out, None, None)
            else:                                       # the forward fitted, its data gradient does not: three launches
                dh2 = ops.chain_single(g, planes_of(w_out, n, transpose=True), None, r2, entry="tadmm_ttconv_chain_out",
                                       image_out=True, memo=False)
                dh1 = None
                if need[0] or need[1]:
                    h1_shape = (ctx.x_shape[0], r1, ctx.x_shape[2], ctx.x_shape[3])
                    dh1 = _core_dgrad_library(dh2, h1_shape, core, stride, padding, dilation)
                if need[0]:
                    gx = ops.chain_single(dh1, planes_of(w_in, n, transpose=True), None, w_in.shape[1],
                                          entry="tadmm_ttconv_chain_in", image_out=True, memo=False)
            if not need[0]:
                gx = None
        if need[3]:                                     # dW_out = dY H2^T over batch and pixels
            gwo = ops.wgrad(g, h2).to(w_out.dtype)
        if need[1]:                                     # dW_in = dH1 X^T
            gwi = ops.wgrad(dh1, x).to(w_in.dtype)
        if need[2]:
            if CONV_CHAIN_DWC_NATIVE:
                gc = ops.core_conv_wgrad(dh2, h1, ksize, stride, padding, dilation).to(core.dtype)
            else:
                gc = _core_wgrad_library(h1, dh2, core, stride, padding, dilation).to(core.dtype)
        if ctx.has_bias and need[4]:
            gb = g.sum((0, 2, 3), dtype=torch.float32)
        return gx, gwi, gc, gwo, gb, None, None, None, None


def conv_chain(x: torch.Tensor, w_in: torch.Tensor, core: torch.Tensor, w_out: torch.Tensor, bias: torch.Tensor = None,
               stride=1, padding=0, dilation=1, cache: dict = None):
    """(B, C, H, W) -> (B, O, Ho, Wo): y = W3 conv_kxk(W1 x; Wc) + bias with w_in = W1 (r1, C), core = Wc (r2, r1, kh, kw),
    w_out = W3 (O, r2), groups = 1, as one `tadmm_ttconv_fused` launch (`ops.conv_chain_fits` says where it applies).
    Differentiable on the contracted factors: the data gradient is one `tadmm_ttconv_fused_bwd` launch (three launches
    where `ops.conv_chain_bwd_fits` is False).  With only x (and bias) wanting a gradient nothing is saved; when a factor
    wants one the two launches also store H1 / H2 and dH1 / dH2, and dW_out = `ops.wgrad(dY, H2)`, dW_in =
    `ops.wgrad(dH1, x)`, dWc = the weight gradient of the core convolution on (H1, dH2).  `cache` (a dict owned by the
    layer): packed planes of frozen factors are reused until their version counters or storage change (`param_key`)."""
    if x.dim() != 4 or core.dim() != 4 or w_in.dim() != 2 or w_out.dim() != 2 or x.shape[1] != w_in.shape[1] \
            or core.shape[1] != w_in.shape[0] or core.shape[0] != w_out.shape[1]:
        raise ValueError("conv_chain expects an NCHW image, W1 (r1, C), a (r2, r1, kh, kw) core and W3 (O, r2)")
    stride, padding, dilation = ops._pair(stride), ops._pair(padding), ops._pair(dilation)
    ksize = tuple(core.shape[2:])
    if not ops.conv_chain_fits(x, w_in.shape[0], w_out.shape[1], ksize, stride, padding, dilation):
        raise TadmmError(-5, "conv_chain: the plane, halo or ranks do not fit the one-launch kernel (ops.conv_chain_fits)")
    if _needs_grad(x, w_in, core, w_out, bias):
        return _ConvChain.apply(x.contiguous(), w_in, core, w_out, bias, stride, padding, dilation, cache)
    p1, p2, p3 = _cached_conv_chain_planes(cache, w_in, core, w_out, _nplanes(x), x.device, False, plane_dtype(x))
    return ops.conv_chain(x, p1, p2, p3, bias, w_out.shape[0], ksize, stride, padding, dilation, memo=cache is not None)


def conv_chain_layer(layer, x: torch.Tensor, w_in: torch.Tensor, w_out: torch.Tensor, inference: bool):
    """A factorised convolution layer (`layer.core_kernel` between the 1x1 maps w_in (r1, C) and w_out (O, r2)) in ONE
    launch, or None where that does not apply and the caller keeps `conv_stages`.  `inference` (the caller's decision:
    the route builds no autograd node): where `ops.conv_chain_pays` says so, the planes packed once into the layer's
    `_fused_cache` (`_cached_conv_chain_planes`).  Otherwise `conv_chain` where something wants a gradient and
    `ops.conv_chain_train_pays` routes it there; frozen factors keep their planes in the same cache."""
    core = layer.core_kernel
    if layer.groups != 1:
        return None
    r1, r2 = w_in.shape[0], w_out.shape[1]
    geom = (layer.kernel_size, layer.stride, layer.padding, layer.dilation)
    if inference:
        if not ops.conv_chain_pays(x, r1, r2, *geom):
            return None
        cache = layer.__dict__.setdefault("_fused_cache", {})
        p1, p2, p3 = _cached_conv_chain_planes(cache, w_in, core, w_out, _nplanes(x), x.device, False, plane_dtype(x))
        return ops.conv_chain(x, p1, p2, p3, layer.bias, w_out.shape[0], *geom)
    if not _needs_grad(x, w_in, core, w_out, layer.bias) or x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16) \
            or not ops.conv_chain_fits(x, r1, r2, *geom):
        return None
    training = _needs_grad(w_in, core, w_out)         # a factor wants a gradient: the intermediates are saved
    if not ops.conv_chain_train_pays(x, r1, r2, *geom, training=training):
        return None
    cache = None if training else layer.__dict__.setdefault("_fused_cache", {})
    return conv_chain(x, w_in, core, w_out, layer.bias, layer.stride, layer.padding, layer.dilation, cache=cache)


# ---------------------------------------------------------------------------------------------------------------
# Factorised embedding lookup (csrc/ttm_gather.hip): the gathered TT-matrix chain of TTMEmbedding.py:96-129,
# TTEmbedding.py:91-118 and SVDEmbedding.py:34-42 as one launch, its core gradients as one launch per core.
# ---------------------------------------------------------------------------------------------------------------
class _TtmGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, index, counter, *cores):
        cs = [c.detach() if c.is_contiguous() else c.detach().contiguous() for c in cores]
        y = ops.ttm_gather(cs, index, counter)
        ctx.save_for_backward(index, *cs)
        return y

    @staticmethod
    def backward(ctx, g):
        index, *cs = ctx.saved_tensors
        grads = ops.ttm_gather_bwd(cs, index, g if g.dtype == torch.float32 else g.float(), ctx.needs_input_grad[2:])
        return (None, None, *grads)


def ttm_embedding_composed(cores, index: torch.Tensor, counter: torch.Tensor = None) -> torch.Tensor:
    """The lookup as the reference composes it (index split by div / fmod, the selected slices of every core, one batched
    product per mode), as torch ops under autograd, in the cores' dtype: the route of shapes `ops.ttm_gather_fits`
    refuses, and the baseline of scripts/bench_embeddings.py.  Bad indices give zero rows and count like the launch."""
    n, m, r = ops.ttm_core_shapes(cores)
    flat = index.reshape(-1)
    total = 1
    for v in n:
        total *= v
    valid = (flat >= 0) & (flat < total)
    if counter is not None:
        counter += (~valid).sum().to(counter.dtype)
    B = flat.numel()
    res = None
    for k, ik in enumerate(ops.ttm_index_split(flat, n)):
        # advanced indexing, not index_select: its backward is torch's sort-based accumulation (tokens of a slice added in
        # a fixed order), so this route's gradients are reproducible from run to run like the launch's
        sl = cores[k][:, ik].permute(1, 0, 2, 3)                                # B x r_{k-1} x m_k x r_k
        if res is None:
            res = sl.reshape(B, m[0], r[1])
        else:
            res = torch.bmm(res.reshape(B, -1, r[k]), sl.reshape(B, r[k], m[k] * r[k + 1]))
    res = res.reshape(B, -1) * valid.to(res.dtype).unsqueeze(1)
    return res.reshape(tuple(index.shape) + (res.shape[1],))


def ttm_embedding(cores, index: torch.Tensor, counter: torch.Tensor = None, route: str = None) -> torch.Tensor:
    """Rows of the TT-matrix the cores (r_{k-1}, n_k, m_k, r_k), r_0 = 1, stand for: `index` (int32 / int64, any shape or
    stride, values in [0, n_1 ... n_d)) -> index.shape + (m_1 ... m_d r_d,), float32, differentiable in the cores.
    An index outside the range gives a zero row, no gradient, and adds 1 to `counter` (one int32 on the device, optional);
    nothing synchronises.  Shapes the launch takes (`ops.ttm_gather_fits`: d <= 4, one token's products within the LDS
    of a CU) run `tadmm_ttm_gather_fwd` / `_bwd` where the measured rule `ops.ttm_gather_pays` says they are ahead
    (always without gradients); the others the composed device route.  `route`: None (by that rule), "native" (the
    launches; shapes they do not take raise) or "composed".  ValueError for no cores and r_0 != 1, TypeError for an
    index that is not of an integer dtype; both before anything is launched."""
    if route not in (None, "native", "composed"):
        raise ValueError(f"ttm_embedding: route is None, 'native' or 'composed' (got {route!r})")
    cores = list(cores)
    n, m, r = ops.ttm_core_shapes(cores)
    if not isinstance(index, torch.Tensor) or index.dtype.is_floating_point or index.dtype.is_complex \
            or index.dtype == torch.bool:
        raise TypeError(f"ttm_embedding: index must be an integer tensor (got {getattr(index, 'dtype', type(index))})")
    if not cores[0].is_cuda:
        raise TadmmError(-1, "ttm_embedding: the cores must live on the HIP device (no CPU fallback)")
    if index.dtype not in (torch.int32, torch.int64):
        index = index.to(torch.int64)
    if index.device != cores[0].device:
        index = index.to(cores[0].device)
    if route is None:
        grad = torch.is_grad_enabled() and any(c.requires_grad for c in cores)
        native = index.numel() > 0 and all(c.dtype == torch.float32 for c in cores) and ops.ttm_gather_fits(n, m, r) \
            and ops.ttm_gather_pays(n, m, r, index.numel(), grad)
    else:
        native = route == "native"
    if not native:
        return ttm_embedding_composed(cores, index, counter)
    y = _TtmGather.apply(index, counter, *cores)
    return y.reshape(tuple(index.shape) + (y.shape[1],))


# ---------------------------------------------------------------------------------------------------------------
# LSTM recurrence over a whole sequence (csrc/lstm.hip): the step function of ablation/tt_lstm_inference.py:44-77 for
# all T steps in one launch, its backward through time in one launch; the products over all T*B tokens (weight and
# bias gradients) go through `ops.wgrad` and a reduction.
# ---------------------------------------------------------------------------------------------------------------
LSTM_GATES = ("hardsigmoid", "sigmoid")


class _LstmSeq(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xp, w_hh, h0, c0, sigmoid):
        w = w_hh.detach()
        planes = ops.lstm_planes(w)
        grad = any(ctx.needs_input_grad[:4])
        if not grad:
            return ops.lstm_seq(xp, planes, h0, c0, sigmoid)
        y, hT, cT, g, c = ops.lstm_seq_save(xp, planes, h0, c0, sigmoid)
        ctx.save_for_backward(w, y, g, c, h0, c0)
        ctx.sigmoid = sigmoid
        return y, hT, cT

    @staticmethod
    def backward(ctx, dy, dhT, dcT):
        w, y, g, c, h0, c0 = ctx.saved_tensors
        T, B, H = y.shape
        f32 = lambda t: None if t is None else (t if t.dtype == torch.float32 else t.float())
        dz, dh0, dc0 = ops.lstm_seq_bwd(ops.lstm_planes(w, transpose=True), g, c, c0, f32(dy), f32(dhT), f32(dcT),
                                        ctx.sigmoid)
        dw = None
        if ctx.needs_input_grad[1]:
            hprev = torch.empty_like(y)
            if h0 is None:
                hprev[0].zero_()
            else:
                hprev[0].copy_(h0)
            hprev[1:].copy_(y[:-1])
            dw = ops.wgrad(dz.view(T * B, 4 * H), hprev.view(T * B, H))
        return (dz if ctx.needs_input_grad[0] else None, dw, dh0 if ctx.needs_input_grad[2] else None,
                dc0 if ctx.needs_input_grad[3] else None, None)


def _lstm_gate(z: torch.Tensor, gate: str) -> torch.Tensor:
    return torch.sigmoid(z) if gate == "sigmoid" else F.hardsigmoid(z)


def lstm_sequence_composed(xp: torch.Tensor, w_hh: torch.Tensor, h0: torch.Tensor = None, c0: torch.Tensor = None,
                           gate: str = "hardsigmoid"):
    """`lstm_sequence` as the reference composes a step (tt_lstm_inference.py:61-77): one `mm` and torch pointwise
    operations per step, on the device, under autograd.  The route of hidden sizes `ops.lstm_fits` refuses and of the
    classes `ops.lstm_seq_pays` sends here, and the yardstick of scripts/bench_lstm.py."""
    if gate not in LSTM_GATES:
        raise ValueError(f"lstm_sequence: gate is 'hardsigmoid' or 'sigmoid' (got {gate!r})")
    T, B, H = xp.shape[0], xp.shape[1], w_hh.shape[1]
    h = xp.new_zeros(B, H) if h0 is None else h0
    c = xp.new_zeros(B, H) if c0 is None else c0
    wt = w_hh.t()
    ys = []
    for t in range(T):
        z = xp[t] + mm(h, wt)
        zi, zf, zg, zo = z.split(H, dim=1)
        c = _lstm_gate(zf, gate) * c + _lstm_gate(zi, gate) * torch.tanh(zg)
        h = _lstm_gate(zo, gate) * torch.tanh(c)
        ys.append(h)
    return torch.stack(ys), (h, c)


def lstm_sequence(xp: torch.Tensor, w_hh: torch.Tensor, h0: torch.Tensor = None, c0: torch.Tensor = None,
                  gate: str = "hardsigmoid", route: str = None):
    """(y (T, B, H), (h_T, c_T)) of the LSTM recurrence  z_t = xp[t] + h_{t-1} w_hh^T,  i, f, o = S(z), g = tanh(z),
    c_t = f c_{t-1} + i g,  h_t = o tanh(c_t),  gate order [i | f | g | o], S = Hardsigmoid (the reference) or the logistic
    function (`gate="sigmoid"`, torch.nn.LSTM).  xp (T, B, 4H) float32 carries the input map and the bias; h0, c0 (B, H)
    default to zeros.  Differentiable in xp, w_hh, h0 and c0.  Hidden sizes the launch takes (`ops.lstm_fits`) run
    `tadmm_lstm_seq_fwd` / `_bwd` where the measured rule `ops.lstm_seq_pays` says so, everything else the composed step
    loop.  `route`: None (by that rule), "launch" (shapes the launch does not take raise) or "composed".  ValueError for
    another route or gate and for shapes that do not agree, TadmmError for tensors that are not float32 on the device."""
    if route not in (None, "launch", "composed"):
        raise ValueError(f"lstm_sequence: route is None, 'launch' or 'composed' (got {route!r})")
    if gate not in LSTM_GATES:
        raise ValueError(f"lstm_sequence: gate is 'hardsigmoid' or 'sigmoid' (got {gate!r})")
    if w_hh.dim() != 2 or w_hh.shape[0] != 4 * w_hh.shape[1] or w_hh.shape[1] < 1:
        raise ValueError(f"lstm_sequence: w_hh must be (4H, H) (got {tuple(w_hh.shape)})")
    H = w_hh.shape[1]
    if xp.dim() != 3 or xp.shape[2] != 4 * H or xp.shape[0] < 1 or xp.shape[1] < 1:
        raise ValueError(f"lstm_sequence: xp must be (T >= 1, B >= 1, {4 * H}) (got {tuple(xp.shape)})")
    T, B = xp.shape[0], xp.shape[1]
    for t, what in ((h0, "h0"), (c0, "c0")):
        if t is not None and tuple(t.shape) != (B, H):
            raise ValueError(f"lstm_sequence: {what} must be ({B}, {H}) (got {tuple(t.shape)})")
    for t, what in ((xp, "xp"), (w_hh, "w_hh"), (h0, "h0"), (c0, "c0")):
        if t is None:
            continue
        if not t.is_cuda:
            raise TadmmError(-1, f"lstm_sequence: {what} must live on the HIP device (no CPU fallback)")
        if t.dtype != torch.float32:
            raise TadmmError(-1, f"lstm_sequence: {what} must be float32 (got {t.dtype}); the recurrence has no "
                                 "bfloat16 / float16 form")
    if route is None:
        grad = torch.is_grad_enabled() and _needs_grad(xp, w_hh, h0, c0)
        launch = ops.lstm_fits(H) and ops.lstm_seq_pays(T, B, H, grad)
    else:
        launch = route == "launch"
    if not launch:
        return lstm_sequence_composed(xp, w_hh, h0, c0, gate)
    y, hT, cT = _LstmSeq.apply(xp, w_hh, h0, c0, gate == "sigmoid")
    return y, (hT, cT)


# ---------------------------------------------------------------------------------------------------------------
# Distillation loss (csrc/distill.hip): the criterion of losses.py: DistillationLoss -- base cross entropy, the
# distillation term and the gradients of both logit tensors in two launches -- and task_distill.py: soft_cross_entropy.
# ---------------------------------------------------------------------------------------------------------------
DISTILL_BASES = ("none", "index", "dense")
DISTILL_KDS = ("none", "soft", "hard", "soft_ce")


def _same_memory(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.data_ptr() == b.data_ptr() and a.stride() == b.stride() and a.shape == b.shape and a.dtype == b.dtype


class _DistillFn(torch.autograd.Function):
    """The forward computes the value and the float32 gradients of both logit tensors; the backward multiplies them by the
    incoming gradient and only then rounds to the logits' type (a float16 gradient of a 1000-class row is below float16's
    normal range before GradScaler's 2^16 is applied)."""

    @staticmethod
    def forward(ctx, outputs, outputs_kd, teacher, target, cfg, counts_box):
        base, kd, alpha, tau, smoothing, ignore_index = cfg
        want_s = ctx.needs_input_grad[0] and base != "none"
        want_k = ctx.needs_input_grad[1] and kd != "none"
        ref = outputs if base != "none" else outputs_kd
        ctx.same = want_s and want_k and _same_memory(outputs, outputs_kd)
        out = {}
        if ctx.same:
            flat = torch.empty((1,) + tuple(ref.shape), dtype=torch.float32, device=ref.device)
            out = {"grad_s": flat[0], "grad_k": flat[0]}
        elif want_s or want_k:
            flat = torch.empty((int(want_s) + int(want_k),) + tuple(ref.shape), dtype=torch.float32, device=ref.device)
            out = {"grad_s": flat[0]} if want_s else {}
            if want_k:
                out["grad_k"] = flat[-1]
        else:
            flat = None
        loss, counts, _, _ = ops.distill_loss(outputs, outputs_kd, teacher, target, base=base, kd=kd, alpha=alpha, tau=tau,
                                              smoothing=smoothing, ignore_index=ignore_index, grad=(want_s, want_k),
                                              out=out)
        if counts_box is not None:
            counts_box.append(counts)
        ctx.flat, ctx.wants, ctx.dtype = flat, (want_s, want_k), ref.dtype
        return loss

    @staticmethod
    def backward(ctx, gout):
        flat = ctx.flat
        if flat is None:
            return (None,) * 6
        g = gout if gout.dtype == torch.float32 else gout.float()
        if ctx.dtype == torch.float32:
            res = flat * g
        else:          # scale in float32, round once on the store
            res = torch.empty(flat.shape, dtype=ctx.dtype, device=flat.device)
            torch.mul(flat, g, out=res)
        want_s, want_k = ctx.wants
        gs = res[0] if want_s else None
        gk = res[-1] if (want_k and not ctx.same) else None       # same memory: the sum went to the first
        return gs, gk, None, None, None, None


def _distill_args(outputs, outputs_kd, teacher, target, base, kd, who):
    if base not in DISTILL_BASES or kd not in DISTILL_KDS:
        raise ValueError(f"{who}: base is one of {DISTILL_BASES}, kd one of {DISTILL_KDS} (got {base!r}, {kd!r})")
    if base == "none" and kd == "none":
        raise ValueError(f"{who}: base and kd are both 'none'")
    logits = [(n, t) for n, t, used in (("outputs", outputs, base != "none"), ("outputs_kd", outputs_kd, kd != "none"),
                                        ("teacher", teacher, kd != "none")) if used]
    for n, t in logits:
        if not isinstance(t, torch.Tensor):
            raise TadmmError(-1, f"{who}: {n} must be a tensor (got {type(t).__name__})")
    n0, t0 = logits[0]
    if t0.dim() != 2 or t0.shape[0] < 1 or t0.shape[1] < 1:
        raise ValueError(f"{who}: {n0} must be (B >= 1, C >= 1) (got {tuple(t0.shape)})")
    for n, t in logits:
        if not t.is_cuda:
            raise TadmmError(-1, f"{who}: {n} must live on the HIP device (got {t.device}); there is no CPU path")
        if t.dtype not in ops.DISTILL_DTYPES:
            raise TadmmError(-1, f"{who}: {n} must be float32, bfloat16 or float16 (got {t.dtype})")
        if t.dtype != t0.dtype:
            raise TadmmError(-1, f"{who}: {n} is {t.dtype}, {n0} is {t0.dtype}; one type per call")
        if t.device != t0.device:
            raise TadmmError(-1, f"{who}: {n} on {t.device}, {n0} on {t0.device}")
        if t.shape != t0.shape:
            raise ValueError(f"{who}: {n} is {tuple(t.shape)}, {n0} is {tuple(t0.shape)}")
    if base != "none":
        if not isinstance(target, torch.Tensor) or not target.is_cuda:
            where = target.device if isinstance(target, torch.Tensor) else type(target).__name__
            raise TadmmError(-1, f"{who}: target must live on the HIP device (got {where}); there is no CPU path")
        if target.device != t0.device:
            raise TadmmError(-1, f"{who}: target on {target.device}, {n0} on {t0.device}")
        if base == "index":
            if target.dtype.is_floating_point or target.dtype.is_complex or target.dtype == torch.bool:
                raise TypeError(f"{who}: integer labels are required for base='index' (got {target.dtype})")
            if tuple(target.shape) != (t0.shape[0],):
                raise ValueError(f"{who}: target must be ({t0.shape[0]},) (got {tuple(target.shape)})")
            target = target if target.dtype == torch.int64 else target.to(torch.int64)
        else:
            if not target.dtype.is_floating_point:
                raise TypeError(f"{who}: dense target rows must be of a floating type (got {target.dtype})")
            if target.shape != t0.shape:
                raise ValueError(f"{who}: target must be {tuple(t0.shape)} (got {tuple(target.shape)})")
            target = target if target.dtype == torch.float32 else target.float()
    return target


def distillation_loss_composed(outputs, outputs_kd, teacher, target, *, base: str = "index", kd: str = "soft",
                               alpha: float = 0.5, tau: float = 1.0, smoothing: float = 0.0, ignore_index=-100,
                               counts=None) -> torch.Tensor:
    """`distillation_loss` as the reference composes it (losses.py:35-61, task_distill.py:721-724) from torch
    operations on the device, under autograd, in float32 whatever the logits' type: the route where
    `ops.distill_loss_pays` says the launch is not ahead, and the yardstick of tests/test_gpu_distill.py and
    scripts/bench_distill.py.  Labels outside [0, C) are mapped to the ignored label first (torch would fault on them)
    and counted into `counts` (a list that receives the int64 [kept rows, bad labels] tensor) when that is given."""
    target = _distill_args(outputs, outputs_kd, teacher, target, base, kd, "distillation_loss_composed")
    base_loss = None
    if base == "index":
        C = outputs.shape[1]
        ign = ops.DISTILL_NO_IGNORE if ignore_index is None else int(ignore_index)
        valid = (target != ign) & (target >= 0) & (target < C)
        fill = ign if ignore_index is not None else -100
        safe = torch.where(valid, target, torch.full_like(target, fill))
        base_loss = F.cross_entropy(outputs.float(), safe, ignore_index=fill, label_smoothing=float(smoothing))
        if counts is not None:
            counts.append(torch.stack([valid.sum(), ((target != ign) & ~valid).sum()]))
    elif base == "dense":
        base_loss = F.cross_entropy(outputs.float(), target, label_smoothing=float(smoothing))
    if base != "index" and counts is not None:
        ref = outputs if base != "none" else outputs_kd
        counts.append(torch.tensor([ref.shape[0], 0], dtype=torch.int64, device=ref.device))
    if kd == "none":
        return base_loss
    k, t, T = outputs_kd.float(), teacher.float(), float(tau)
    if kd == "soft":
        kd_loss = F.kl_div(F.log_softmax(k / T, dim=1), F.log_softmax(t / T, dim=1), reduction="sum",
                           log_target=True) * (T * T) / k.numel()
    elif kd == "hard":
        kd_loss = F.cross_entropy(k, t.argmax(dim=1))
    else:
        kd_loss = (-F.softmax(t / T, dim=-1) * F.log_softmax(k / T, dim=-1)).mean()
    if base_loss is None:
        return kd_loss * alpha
    return base_loss * (1 - alpha) + kd_loss * alpha


def distillation_loss(outputs, outputs_kd, teacher, target, *, base: str = "index", kd: str = "soft", alpha: float = 0.5,
                      tau: float = 1.0, smoothing: float = 0.0, ignore_index=-100, route: str = None,
                      counts=None) -> torch.Tensor:
    """The training criterion of losses.py: DistillationLoss as one differentiable call, float32 0-dim:

        base  "index": cross entropy of `outputs` (B, C) against integer labels `target` (B,), label smoothing
                       `smoothing`, mean over the rows whose label is neither `ignore_index` (None: ignore nothing) nor
                       outside [0, C) -- the latter are counted, contribute nothing and are never used as an address;
              "dense": soft-target cross entropy against float rows `target` (B, C), mean over B;
              "none":  no base term (`outputs`, `target` unused)
        kd    "soft":  KL(softmax(teacher / tau) || softmax(outputs_kd / tau)) * tau^2 / (B C)   (losses.py:51-56)
              "hard":  cross entropy of outputs_kd against the teacher's argmax                  (losses.py:58)
              "soft_ce": mean over B C of -softmax(teacher / tau) log_softmax(outputs_kd / tau)  (task_distill.py:721)
              "none":  the base term alone
        loss = (1 - alpha) base + alpha kd       (kd "none": base; base "none": alpha kd)

    The logits are float32, bfloat16 or float16 HIP tensors of one type, unit column stride (row slices of a wider
    tensor are read in place); `outputs_kd` may be `outputs`.  Differentiable in `outputs` and `outputs_kd`; the teacher
    gets no gradient.  `route`: None (by the measured rule `ops.distill_loss_pays`), "launch" (csrc/distill.hip: value
    and gradients in two launches, the backward one or two more) or "composed" (torch operations).  `counts`: a list
    that receives the int64 device tensor [kept rows, bad labels] of the call.  Nothing synchronises."""
    if route not in (None, "launch", "composed"):
        raise ValueError(f"distillation_loss: route is None, 'launch' or 'composed' (got {route!r})")
    target = _distill_args(outputs, outputs_kd, teacher, target, base, kd, "distillation_loss")
    ref = outputs if base != "none" else outputs_kd
    if route is None:
        grad = torch.is_grad_enabled() and _needs_grad(*[t for t in (outputs, outputs_kd) if isinstance(t, torch.Tensor)])
        launch = ops.distill_loss_pays(ref.shape[0], ref.shape[1], ref.dtype, grad)
    else:
        launch = route == "launch"
    kw = dict(base=base, kd=kd, alpha=alpha, tau=tau, smoothing=smoothing, ignore_index=ignore_index)
    if not launch:
        return distillation_loss_composed(outputs, outputs_kd, teacher, target, counts=counts, **kw)
    cfg = (base, kd, float(alpha), float(tau), float(smoothing), ignore_index)
    s = outputs if base != "none" else None
    k = outputs_kd if kd != "none" else None
    return _DistillFn.apply(s, k, None if teacher is None else teacher.detach(), target, cfg, counts)


def soft_cross_entropy(predicts: torch.Tensor, targets: torch.Tensor, temperature: float = 1.0,
                       route: str = None) -> torch.Tensor:
    """task_distill.py:721-724 with the division of :833 folded in: mean over all elements of
    -softmax(targets / temperature) * log_softmax(predicts / temperature), class dimension last; float32 0-dim,
    differentiable in `predicts`."""
    if not isinstance(predicts, torch.Tensor) or not isinstance(targets, torch.Tensor) or predicts.dim() < 1:
        raise TadmmError(-1, "soft_cross_entropy: predicts and targets must be tensors with a class dimension")
    C = predicts.shape[-1]
    p = predicts if predicts.dim() == 2 else predicts.reshape(-1, C)
    t = targets if targets.dim() == 2 else targets.reshape(-1, C)
    return distillation_loss(None, p, t.detach(), None, base="none", kd="soft_ce", alpha=1.0, tau=temperature, route=route)


# ---------------------------------------------------------------------------------------------------------------
# TinyBERT layer losses (csrc/layermse.hip): the intermediate-layer step of task_distill.py:810-828 -- the MSE of the
# attention scores with the masked entries zeroed, the MSE of the hidden states, and the students' gradients, for all
# pairs of a step in two launches.
# ---------------------------------------------------------------------------------------------------------------
LAYER_MSE_REDUCTIONS = ("batch_sum", "mean")


def _layer_mse_list(x, who, what):
    if x is None:
        return []
    if isinstance(x, torch.Tensor):
        return [x]
    x = list(x)
    for i, t in enumerate(x):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {what}[{i}] must be a tensor (got {type(t).__name__})")
    return x


def _layer_mse_args(student_atts, teacher_atts, student_reps, teacher_reps, reduction, att_weights, rep_weights, who):
    """The four arguments as lists, and the scale c of every pair: w B / numel ("batch_sum") or w / numel ("mean")."""
    if reduction not in LAYER_MSE_REDUCTIONS:
        raise ValueError(f"{who}: reduction is one of {LAYER_MSE_REDUCTIONS} (got {reduction!r})")
    sides = []
    for name, ss, ts, ws in (("atts", student_atts, teacher_atts, att_weights), ("reps", student_reps, teacher_reps, rep_weights)):
        ss, ts = _layer_mse_list(ss, who, "student_" + name), _layer_mse_list(ts, who, "teacher_" + name)
        if len(ss) != len(ts):
            raise ValueError(f"{who}: {len(ss)} student_{name} and {len(ts)} teacher_{name}")
        if ws is None:
            ws = [1.0] * len(ss)
        elif isinstance(ws, (int, float)):
            ws = [float(ws)] * len(ss)
        else:
            ws = [float(w) for w in ws]
            if len(ws) != len(ss):
                raise ValueError(f"{who}: {len(ws)} weights for {len(ss)} student_{name}")
        scales = []
        for i, (s, t, w) in enumerate(zip(ss, ts, ws)):
            if s.shape != t.shape:
                raise ValueError(f"{who}: student_{name}[{i}] is {tuple(s.shape)}, teacher_{name}[{i}] is {tuple(t.shape)}")
            if s.dim() < 1 or s.numel() < 1:
                raise ValueError(f"{who}: student_{name}[{i}] must have a batch dimension and at least one element "
                                 f"(got {tuple(s.shape)})")
            scales.append(w * (s.shape[0] if reduction == "batch_sum" else 1) / s.numel())
        sides.append((ss, ts, scales))
    return sides


def intermediate_distillation_loss_composed(student_atts, teacher_atts, student_reps, teacher_reps, *,
                                            threshold=-1e2, reduction: str = "batch_sum", att_weights=None,
                                            rep_weights=None):
    """`intermediate_distillation_loss` as the reference composes it (task_distill.py:810-828) from `torch.where` and
    `F.mse_loss` under autograd, on any device and any floating type: 16-bit tensors are widened to float32 first, float64
    stays float64 (and so does the result).  The route for what the launch refuses and where `ops.layer_mse_pays` says
    it is not ahead, and the yardstick of tests/test_gpu_layer_mse.py and scripts/bench_layer_mse.py."""
    who = "intermediate_distillation_loss_composed"
    sides = _layer_mse_args(student_atts, teacher_atts, student_reps, teacher_reps, reduction, att_weights, rep_weights, who)
    anyt = next((s for ss, _, _ in sides for s in ss), None)
    out = []
    for k, (ss, ts, scales) in enumerate(sides):
        total = None
        for s, t, c in zip(ss, ts, scales):
            t = t.detach()
            if s.dtype in (torch.bfloat16, torch.float16):
                s, t = s.float(), t.float()
            elif t.dtype != s.dtype:
                t = t.to(s.dtype)
            if k == 0 and threshold is not None:
                s = torch.where(s <= threshold, torch.zeros_like(s), s)
                t = torch.where(t <= threshold, torch.zeros_like(t), t)
            term = F.mse_loss(s, t) * (c * s.numel())
            total = term if total is None else total + term
        if total is None:
            total = torch.zeros((), dtype=torch.float32, device=None if anyt is None else anyt.device)
        out.append(total)
    return out[0], out[1]


def layer_mse_launch_refusal(is_cuda: bool, dtypes, npairs: int, teacher_foreign: bool = False):
    """None when csrc/layermse.hip takes a call with these properties, else the reason it does not (a string): CPU
    tensors, an element type other than float32 / bfloat16 / float16, more than one type in the call (`dtypes`: the
    types of all students and teachers), more than `ops.LAYER_MSE_MAX_PAIRS` pairs, or a tensor that lives on another
    device than the first student (`teacher_foreign`).  A pure function."""
    if not is_cuda:
        return "operands that are not on a HIP device"
    dtypes = list(dict.fromkeys(dtypes))
    for dt in dtypes:
        if dt not in ops.LAYER_MSE_DTYPES:
            return f"{dt} operands"
    if len(dtypes) > 1:
        return "mixed element types in one call (" + ", ".join(str(dt) for dt in dtypes) + ")"
    if npairs > ops.LAYER_MSE_MAX_PAIRS:
        return f"{npairs} pairs (one call takes {ops.LAYER_MSE_MAX_PAIRS})"
    if teacher_foreign:
        return "a teacher on another device than its student"
    return None


class _LayerMseFn(torch.autograd.Function):
    """apply(cfg, *students, *teachers): the forward computes both losses and the float32 gradients of the students that
    need one into one flat buffer, attention pairs first; the backward multiplies each group's slice by its incoming
    gradient and only then rounds to the students' type (a float16 gradient 2 d B / numel is below float16's normal
    range before GradScaler's 2^16 is applied)."""

    @staticmethod
    def forward(ctx, cfg, *tensors):
        natt, nrep, scales, threshold = cfg
        n = natt + nrep
        students, teachers = tensors[:n], tensors[n:]
        ctx.set_materialize_grads(False)
        needs = ctx.needs_input_grad[1:1 + n]
        spans, cursor, cut = [None] * n, 0, None         # flat[:cut]: the attention pairs, flat[cut:]: the hidden pairs
        for i, s in enumerate(students):
            if i == natt:
                cut = cursor
            if needs[i]:
                start = (cursor + 3) // 4 * 4            # 16-byte aligned: wide gradient stores
                cursor = start + s.numel()
                spans[i] = (start, cursor)
        cut = cursor if cut is None else cut
        flat = torch.empty(cursor, dtype=torch.float32, device=students[0].device) if cursor else None
        grads = [None if sp is None else flat[sp[0]:sp[1]] for sp in spans]
        loss, _ = ops.layer_mse(students, teachers, scales, [0] * natt + [1] * nrep,
                                [threshold is not None] * natt + [False] * nrep, threshold, grads=grads)
        ctx.flat, ctx.spans, ctx.cut, ctx.natt = flat, spans, cut, natt
        ctx.meta = [(s.dtype, s.shape) for s in students]
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_att, g_rep):
        flat, n, cut = ctx.flat, len(ctx.spans), ctx.cut
        out = [None] * (1 + 2 * n)
        if flat is None or (g_att is None and g_rep is None):
            return tuple(out)
        res = torch.empty(flat.shape, dtype=ctx.meta[0][0], device=flat.device)
        for g, lo, hi in ((g_att, 0, cut), (g_rep, cut, flat.numel())):
            if g is not None and hi > lo:             # scale in float32, round once on the store
                torch.mul(flat[lo:hi], g if g.dtype == torch.float32 else g.float(), out=res[lo:hi])
        for i, sp in enumerate(ctx.spans):
            if sp is not None and (g_att if i < ctx.natt else g_rep) is not None:
                out[1 + i] = res[sp[0]:sp[1]].view(ctx.meta[i][1])
        return tuple(out)


def intermediate_distillation_loss(student_atts, teacher_atts, student_reps, teacher_reps, *, threshold=-1e2,
                                   reduction: str = "batch_sum", att_weights=None, rep_weights=None, route: str = None):
    """(att_loss, rep_loss) of TinyBERT's intermediate-layer distillation step (task_distill.py:810-828), both float32
    0-dim and differentiable in the student tensors; the teachers are detached:

        att_loss = sum_i w_i R((s_i where s_i > threshold else 0) - (t_i where t_i > threshold else 0))
        rep_loss = sum_i w_i R(s_i - t_i)
        R(d) = "batch_sum": sum_b mean(d[b]^2)   (the reference's loop over the batch axis of the last layer)
               "mean":      mean(d^2)            (MSELoss over the whole tensor: upstream TinyBERT's per-layer loop)

    Each of the four arguments is a tensor or a sequence of tensors, paired by position; either side may be empty (its
    loss is then a float32 zero without a graph).  `threshold=None` switches the clamp off.  `att_weights`, `rep_weights`:
    None, one number or one per pair (task_distill1.py's beta_scale).  `route`: None (the launch where it takes the call
    and the measured rule `ops.layer_mse_pays` says it is ahead), "launch" (csrc/layermse.hip: values and gradients in
    two launches, the backward at most two more) or "composed" (torch operations).  The launch takes HIP tensors of one
    type (float32, bfloat16 or float16) on one device, at most `ops.LAYER_MSE_MAX_PAIRS` pairs; anything else goes to
    the composed route under `route=None` and raises under `route="launch"`.  Students that are not contiguous are
    copied.  Nothing synchronises."""
    who = "intermediate_distillation_loss"
    if route not in (None, "launch", "composed"):
        raise ValueError(f"{who}: route is None, 'launch' or 'composed' (got {route!r})")
    sides = _layer_mse_args(student_atts, teacher_atts, student_reps, teacher_reps, reduction, att_weights, rep_weights, who)
    (sa, ta, ca), (sr, tr, cr) = sides
    students, teachers = sa + sr, ta + tr
    n = len(students)
    kw = dict(threshold=threshold, reduction=reduction, att_weights=att_weights, rep_weights=rep_weights)
    if n == 0:
        return intermediate_distillation_loss_composed(sa, ta, sr, tr, **kw)
    every = students + teachers
    dev = students[0].device
    why = layer_mse_launch_refusal(all(t.is_cuda for t in every), [t.dtype for t in every], n,
                                   any(t.device != dev for t in every))
    if route == "launch" and why is not None:
        raise TadmmError(-1, f"{who}: route='launch' cannot take {why}")
    launch = why is None and route != "composed"
    if launch and route is None:
        launch = ops.layer_mse_pays(sum(s.numel() for s in students), n, students[0].dtype, _needs_grad(*students))
    if not launch:
        att, rep = intermediate_distillation_loss_composed(sa, ta, sr, tr, **kw)
        return att.float(), rep.float()
    students = [s if s.is_contiguous() else s.contiguous() for s in students]       # the gradient returns through the copy
    cfg = (len(sa), len(sr), tuple(ca + cr), None if threshold is None else float(threshold))
    att, rep = _LayerMseFn.apply(cfg, *students, *[t.detach() for t in teachers])
    return (att if sa else att.detach()), (rep if sr else rep.detach())


# ---------------------------------------------------------------------------------------------------------------
# BERT self-attention (csrc/attn.hip): the body of compressed_modeling*.py: *BertSelfAttention.forward after the three
# projections -- raw masked scores (a differentiable output: TinyBERT regresses them), softmax, dropout, context.
# ---------------------------------------------------------------------------------------------------------------
class _AttnFn(torch.autograd.Function):
    """Two differentiable outputs; the backward recomputes P from q, k, the mask and the saved row statistics."""

    @staticmethod
    def forward(ctx, q, k, v, mask, keep, num_heads, p, need_scores):
        need = any(ctx.needs_input_grad[:3])
        ctx.set_materialize_grads(False)
        context, scores, stats = ops.attn_fwd(q, k, v, mask, num_heads, p=p, keep=keep, need_scores=need_scores,
                                              need_stats=need)
        if need:
            ctx.save_for_backward(q, k, v, stats)
        ctx.mask, ctx.keep, ctx.cfg = mask, keep, (num_heads, p)
        if scores is None:
            return context
        return context, scores

    @staticmethod
    def backward(ctx, g_ctx, g_sc=None):
        q, k, v, stats = ctx.saved_tensors
        num_heads, p = ctx.cfg
        if g_ctx is None and g_sc is None:
            return (None,) * 8
        dq, dk, dv = ops.attn_bwd(q, k, v, ctx.mask, num_heads, stats, g_ctx, g_sc, p=p, keep=ctx.keep)
        need = ctx.needs_input_grad
        return (dq if need[0] else None, dk if need[1] else None, dv if need[2] else None, None, None, None, None, None)


def _attn_args(q, k, v, mask, num_heads, dropout_p, who):
    for n, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(f"{who}: {n} must be a (B, S, H*d) tensor")
        if t.shape != q.shape or t.dtype != q.dtype or t.device != q.device:
            raise ValueError(f"{who}: q, k and v must agree in shape, type and device")
    if num_heads < 1 or q.shape[2] % num_heads:
        raise ValueError(f"{who}: the hidden size ({q.shape[2]}) is not a multiple of the number of heads ({num_heads})")
    if not 0.0 <= float(dropout_p) < 1.0:
        raise ValueError(f"{who}: dropout_p must be in [0, 1) (got {dropout_p})")


def attention_keep_mask(B: int, H: int, S: int, p: float, device, generator=None) -> torch.Tensor:
    """The byte tensor (B, H, S, S) of kept probabilities of a dropout at rate p, drawn with torch's generator (so that
    a seed reproduces a run and both routes of `self_attention` can be handed the same mask)."""
    return (torch.rand((B, H, S, S), device=device, generator=generator) >= p).to(torch.uint8)


def self_attention_composed(q, k, v, mask, num_heads: int, *, dropout_p: float = 0.0, training: bool = False,
                            need_scores: bool = True, keep=None):
    """`self_attention` as the reference composes it (compressed_modeling_tt.py:379-403) from torch operations, under
    autograd, on any device: the route for shapes the launch refuses, masks that are not (B, 1, 1, S), masks that
    require grad, CPU tensors and float16 training, and the yardstick of tests/test_gpu_attn.py and
    scripts/bench_attention.py.  Dropout multiplies by `keep` / (1 - p) (drawn here when not given)."""
    _attn_args(q, k, v, mask, num_heads, dropout_p, "self_attention_composed")
    B, S, Hd = q.shape
    d = Hd // num_heads
    ql, kl, vl = (t.view(B, S, num_heads, d).permute(0, 2, 1, 3) for t in (q, k, v))
    scores = torch.matmul(ql, kl.transpose(-1, -2))
    scores = scores / (d ** 0.5)
    if mask is not None:
        scores = scores + mask
    probs = torch.softmax(scores, dim=-1)
    if training and dropout_p > 0.0:
        if keep is None:
            keep = attention_keep_mask(B, num_heads, S, dropout_p, q.device)
        probs = probs * (keep != 0).to(probs.dtype) / (1.0 - dropout_p)
    context = torch.matmul(probs, vl).permute(0, 2, 1, 3).contiguous().view(B, S, Hd)
    return context, (scores if need_scores else None)


def attention_launch_refusal(is_cuda: bool, dtype, B: int, H: int, S: int, d: int, grad: bool, mask_shape=None,
                             mask_foreign: bool = False):
    """None when csrc/attn.hip takes a call with these properties, else the reason it does not (a string): CPU tensors,
    a type other than float32 / bfloat16 / float16, float16 with gradients, S or d out of range, a mask that is not
    (B, 1, 1, S), or one that requires grad or lives elsewhere (`mask_foreign`).  A pure function."""
    if not is_cuda:
        return "operands that are not on a HIP device"
    if dtype not in ops.ATTN_DTYPES:
        return f"{dtype} operands"
    if dtype == torch.float16 and grad:
        return "float16 with gradients"
    if B < 1 or S < 1 or d < 1 or not ops.attn_fits(S, d, H, dtype):
        return f"S = {S}, d = {d}"
    if mask_shape is not None and tuple(mask_shape) != (B, 1, 1, S):
        return f"a mask of shape {tuple(mask_shape)}"
    if mask_foreign:
        return "a mask that requires grad or lives on another device"
    return None


def self_attention(q, k, v, mask, num_heads: int, *, dropout_p: float = 0.0, training: bool = False,
                   need_scores: bool = True, keep=None, route: str = None):
    """(context, scores or None) of a BERT self-attention for projected q, k, v of shape (B, S, H*d):

        scores[b,h,i,j] = (Q[b,i,h,:] . K[b,j,h,:]) / sqrt(d) + mask[b,0,0,j]
        context[b,i,h*d:(h+1)*d] = sum_j dropout(softmax_j(scores))[b,h,i,j] V[b,j,h,:]

    Both outputs are differentiable in q, k and v.  `mask`: additive, (B, 1, 1, S) or None.  Dropout acts only when
    `training` and `dropout_p` > 0: `keep` (B, H, S, S) bytes, nonzero = kept, is drawn with torch's generator when not
    given.  `route`: None (the launch where it takes the call and the measured rule `ops.attn_pays` says it is ahead),
    "launch" (csrc/attn.hip: one launch forward, two backward) or "composed" (torch operations).  The launch takes HIP
    tensors of float32 or bfloat16 (float16 without gradients), S <= 512, d <= 64, a (B, 1, 1, S) mask that requires no
    gradient; everything else goes to the composed route under `route=None` and raises under `route="launch"`."""
    who = "self_attention"
    if route not in (None, "launch", "composed"):
        raise ValueError(f"{who}: route is None, 'launch' or 'composed' (got {route!r})")
    _attn_args(q, k, v, mask, num_heads, dropout_p, who)
    B, S, Hd = q.shape
    d = Hd // num_heads
    p = float(dropout_p) if training else 0.0
    grad = torch.is_grad_enabled() and _needs_grad(q, k, v)
    why = attention_launch_refusal(q.is_cuda, q.dtype, B, num_heads, S, d, grad,
                                   None if mask is None else tuple(mask.shape),
                                   mask is not None and (mask.requires_grad or mask.device != q.device))
    if route == "launch" and why is not None:
        raise TadmmError(-1, f"{who}: route='launch' cannot take {why}")
    launch = why is None and (route == "launch" or (route is None and ops.attn_pays(B, num_heads, S, d, q.dtype, grad)))
    if not launch:
        return self_attention_composed(q, k, v, mask, num_heads, dropout_p=dropout_p, training=training,
                                       need_scores=need_scores, keep=keep)
    if p > 0.0 and keep is None:
        keep = attention_keep_mask(B, num_heads, S, p, q.device)
    out = _AttnFn.apply(q, k, v, None if mask is None else mask.detach(), keep if p > 0.0 else None, int(num_heads), p,
                        bool(need_scores))
    return out if need_scores else (out, None)


# ---------------------------------------------------------------------------------------------------------------
# BERT sub-layer tail (csrc/bertnorm.hip): LayerNorm(dropout(x) + res) of compressed_modeling*.py: *SelfOutput,
# BertOutput, BertEmbeddings and BertPredictionHeadTransform, with the reference's BertLayerNorm (eps inside the root).
# ---------------------------------------------------------------------------------------------------------------
class _BertNormFn(torch.autograd.Function):
    """x, res: (rows, hidden).  The backward recomputes s and xhat from x, res, keep and the saved (mean, rstd)."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, keep, eps, p):
        need = any(ctx.needs_input_grad[:4])
        y, stats = ops.bertnorm_fwd(x, res, weight, bias, eps=eps, p=p, keep=keep, need_stats=need)
        if need:
            ctx.save_for_backward(x, res, weight, stats)
        ctx.keep, ctx.cfg = keep, (eps, p)
        return y

    @staticmethod
    def backward(ctx, g):
        x, res, weight, stats = ctx.saved_tensors
        eps, p = ctx.cfg
        need = ctx.needs_input_grad
        dx, dres, dgamma, dbeta = ops.bertnorm_bwd(x, res, weight, stats, g, eps=eps, p=p, keep=ctx.keep,
                                                   need=(need[0], need[1] and res is not None, need[2], need[3]))
        if dgamma is not None:
            dgamma = dgamma.to(weight.dtype)
        if dbeta is not None:
            dbeta = dbeta.to(weight.dtype)
        return dx, dres, dgamma, dbeta, None, None, None


def _layer_norm_args(x, res, weight, bias, dropout_p, keep, who):
    if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.shape[-1] < 1:
        raise ValueError(f"{who}: x must be a tensor (..., hidden >= 1)")
    if res is not None and (not isinstance(res, torch.Tensor) or res.shape != x.shape):
        raise ValueError(f"{who}: res must have the shape of x")
    for n, t in (("weight", weight), ("bias", bias)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (x.shape[-1],):
            raise ValueError(f"{who}: {n} must be a ({x.shape[-1]},) tensor")
    if not 0.0 <= float(dropout_p) < 1.0:
        raise ValueError(f"{who}: dropout_p must be in [0, 1) (got {dropout_p})")
    if keep is not None and (not isinstance(keep, torch.Tensor) or keep.shape != x.shape):
        raise ValueError(f"{who}: keep must have the shape of x")


def residual_keep_mask(shape, p: float, device, generator=None) -> torch.Tensor:
    """The byte tensor of `shape` of kept elements of a dropout at rate p, drawn with torch's generator (so that a seed
    reproduces a run and both routes of `residual_layer_norm` can be handed the same mask)."""
    return (torch.rand(tuple(shape), device=device, generator=generator) >= p).to(torch.uint8)


def residual_layer_norm_composed(x, res, weight, bias, *, eps: float = 1e-12, dropout_p: float = 0.0,
                                 training: bool = False, keep=None):
    """`residual_layer_norm` from torch operations, under autograd, on any device: `F.dropout` (or `keep` / (1 - p) where
    a mask is given), the add, `F.layer_norm` -- the arithmetic of the reference's ten-call BertLayerNorm
    (compressed_modeling_tt.py:145-158) behind its dropout and add, in the fewest launches torch has.  The route for what
    the launch refuses (CPU tensors, float64, float16 training, rows wider than `ops.bertnorm_hmax()`), and the yardstick
    of tests/test_gpu_bertnorm.py and scripts/bench_bertlayer.py.  Parameters of another type than x are converted."""
    _layer_norm_args(x, res, weight, bias, dropout_p, keep, "residual_layer_norm_composed")
    h = x
    if training and dropout_p > 0.0:
        if keep is None:
            h = F.dropout(x, dropout_p, True)
        else:
            h = x * (keep != 0).to(x.dtype) / (1.0 - dropout_p)
    if res is not None:
        h = h + res
    return F.layer_norm(h, (h.shape[-1],), weight.to(h.dtype), bias.to(h.dtype), eps)


def layer_norm_launch_refusal(is_cuda: bool, dtype, rows: int, hidden: int, grad: bool, param_dtype=None,
                              foreign: bool = False):
    """None when csrc/bertnorm.hip takes a call with these properties, else the reason it does not (a string): CPU
    tensors, a type other than float32 / bfloat16 / float16, float16 with gradients, no rows, a row wider than the
    launch holds, parameters that are neither float32 nor of the type of x, or a residual, parameter or keep tensor of
    another type or on another device (`foreign`).  A pure function."""
    if not is_cuda:
        return "operands that are not on a HIP device"
    if dtype not in ops.BERTNORM_DTYPES:
        return f"{dtype} operands"
    if dtype == torch.float16 and grad:
        return "float16 with gradients"
    if rows < 1 or hidden < 1 or not ops.bertnorm_fits(hidden, dtype):
        return f"rows = {rows}, hidden = {hidden}"
    if param_dtype is not None and param_dtype not in (torch.float32, dtype):
        return f"{param_dtype} parameters beside {dtype} operands"
    if foreign:
        return "a residual, parameter or keep tensor of another type or on another device"
    return None


def residual_layer_norm(x, res, weight, bias, *, eps: float = 1e-12, dropout_p: float = 0.0, training: bool = False,
                        keep=None, route: str = None):
    """LayerNorm(dropout(x) + res) over the last dimension, the tail of every BERT sub-layer:

        s = x * keep / (1 - p) + res,   y = weight * (s - mean(s)) / sqrt(var(s) + eps) + bias

    with the biased variance and eps inside the root (the reference's BertLayerNorm).  `res`: a tensor of the shape and
    type of x, or None (a plain LayerNorm).  Dropout acts only when `training` and `dropout_p` > 0: `keep` (the shape of
    x, bytes, nonzero = kept) is drawn with torch's generator when not given.  Differentiable in x, res, weight and
    bias; the gradients of x and res are always two tensors.  `route`: None (the launch where it takes the call and the
    measured rule `ops.bertnorm_pays` says it is ahead), "launch" (csrc/bertnorm.hip: one launch forward, two backward)
    or "composed" (torch operations).  The launch takes HIP tensors of float32 or bfloat16 (float16 without gradients)
    with at most `ops.bertnorm_hmax()` columns and parameters in float32 or the type of x; leading dimensions are
    flattened to rows, without a copy where the strides allow it (unit element stride, one row stride).  Everything
    else goes to the composed route under `route=None` and raises under `route="launch"`."""
    who = "residual_layer_norm"
    if route not in (None, "launch", "composed"):
        raise ValueError(f"{who}: route is None, 'launch' or 'composed' (got {route!r})")
    _layer_norm_args(x, res, weight, bias, dropout_p, keep, who)
    hidden = x.shape[-1]
    rows = x.numel() // hidden
    p = float(dropout_p) if training else 0.0
    grad = _needs_grad(x, res, weight, bias)
    foreign = (res is not None and (res.dtype != x.dtype or res.device != x.device)) \
        or weight.device != x.device or bias.device != x.device or weight.dtype != bias.dtype \
        or (keep is not None and p > 0.0 and keep.device != x.device)
    why = layer_norm_launch_refusal(x.is_cuda, x.dtype, rows, hidden, grad, weight.dtype, foreign)
    if route == "launch" and why is not None:
        raise TadmmError(-1, f"{who}: route='launch' cannot take {why}")
    launch = why is None and (route == "launch" or (route is None and ops.bertnorm_pays(rows, hidden, x.dtype, grad)))
    if not launch:
        return residual_layer_norm_composed(x, res, weight, bias, eps=eps, dropout_p=dropout_p, training=training,
                                            keep=keep)
    if p > 0.0 and keep is None:
        keep = residual_keep_mask(x.shape, p, x.device)
    y = _BertNormFn.apply(x.reshape(rows, hidden), None if res is None else res.reshape(rows, hidden), weight, bias,
                          keep.reshape(rows, hidden) if p > 0.0 else None, float(eps), p)
    return y.view(x.shape)


# ---------------------------------------------------------------------------------------------------------------
# Pre-norm block tail (csrc/prenorm.hip): x + drop_path(dropout(branch)) and the LayerNorm of that sum, the step between
# the branches of vit_tt.py: TTBlock (timm's Block.forward) -- two outputs, the stream and what the next branch reads.
# ---------------------------------------------------------------------------------------------------------------
class _PreNormFn(torch.autograd.Function):
    """x, b: (rows, hidden).  Returns (s, y); the backward recomputes xhat from the saved output s and (mean, rstd)."""

    @staticmethod
    def forward(ctx, x, b, weight, bias, keep, path_keep, eps, p, p_path, nper):
        need = any(ctx.needs_input_grad[:4])
        ctx.set_materialize_grads(False)
        s, y, stats = ops.prenorm_fwd(x, b, weight, bias, eps=eps, p=p, keep=keep, p_path=p_path, path_keep=path_keep,
                                      rows_per_sample=nper, need_stats=need)
        if need:
            ctx.save_for_backward(s, weight, stats)
        ctx.keep, ctx.path_keep, ctx.cfg = keep, path_keep, (eps, p, p_path, nper)
        return s, y

    @staticmethod
    def backward(ctx, g_s, g_y):
        if g_s is None and g_y is None:
            return (None,) * 10
        s, weight, stats = ctx.saved_tensors
        eps, p, p_path, nper = ctx.cfg
        need = ctx.needs_input_grad
        dx, db, dgamma, dbeta = ops.prenorm_bwd(s, weight, stats, g_y, g_s, eps=eps, p=p, keep=ctx.keep, p_path=p_path,
                                                path_keep=ctx.path_keep, rows_per_sample=nper, need=need[:4])
        if dgamma is not None:
            dgamma = dgamma.to(weight.dtype)
        if dbeta is not None:
            dbeta = dbeta.to(weight.dtype)
        return (dx, db, dgamma, dbeta) + (None,) * 6


def _add_layer_norm_args(x, branch, weight, bias, dropout_p, drop_path_p, keep, path_keep, who):
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or x.shape[-1] < 1:
        raise ValueError(f"{who}: x must be a (B, N, C) or (rows, C) tensor with C >= 1")
    if not isinstance(branch, torch.Tensor) or branch.shape != x.shape:
        raise ValueError(f"{who}: branch must have the shape of x")
    for n, t in (("weight", weight), ("bias", bias)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (x.shape[-1],):
            raise ValueError(f"{who}: {n} must be a ({x.shape[-1]},) tensor")
    for n, r in (("dropout_p", dropout_p), ("drop_path_p", drop_path_p)):
        if not 0.0 <= float(r) < 1.0:
            raise ValueError(f"{who}: {n} must be in [0, 1) (got {r})")
    if keep is not None and (not isinstance(keep, torch.Tensor) or keep.shape != x.shape):
        raise ValueError(f"{who}: keep must have the shape of x")
    if path_keep is not None and (not isinstance(path_keep, torch.Tensor) or tuple(path_keep.shape) != (x.shape[0],)):
        raise ValueError(f"{who}: path_keep must be a ({x.shape[0]},) tensor")


def drop_path_keep_mask(B: int, p: float, device, generator=None) -> torch.Tensor:
    """The byte tensor (B,) of the samples a DropPath at rate p keeps, drawn with torch's generator (so that a seed
    reproduces a run and both routes of `add_layer_norm` can be handed the same mask).  timm keeps a sample where
    floor(1 - p + rand) is 1, which is rand >= p."""
    return (torch.rand((B,), device=device, generator=generator) >= p).to(torch.uint8)


def add_layer_norm_composed(x, branch, weight, bias, *, eps: float = 1e-6, dropout_p: float = 0.0,
                            drop_path_p: float = 0.0, training: bool = False, keep=None, path_keep=None):
    """`add_layer_norm` from torch operations, under autograd, on any device: `F.dropout` of the branch (or `keep` /
    (1 - p) where a mask is given), timm's DropPath arithmetic `x.div(keep_prob) * floor(keep_prob + rand((B, 1, 1)))`
    (or `path_keep` in place of the drawn factor), the add, `F.layer_norm`.  The route for what the launch refuses and
    the yardstick of tests/test_gpu_prenorm.py and scripts/bench_vit_block.py.  Parameters of another type than x are
    converted.  Returns (stream, normed)."""
    _add_layer_norm_args(x, branch, weight, bias, dropout_p, drop_path_p, keep, path_keep, "add_layer_norm_composed")
    h = branch
    if training and dropout_p > 0.0:
        if keep is None:
            h = F.dropout(h, dropout_p, True)
        else:
            h = h * (keep != 0).to(h.dtype) / (1.0 - dropout_p)
    if training and drop_path_p > 0.0:
        keep_prob = 1.0 - drop_path_p
        shape = (x.shape[0],) + (1,) * (x.dim() - 1)
        if path_keep is None:
            factor = (keep_prob + torch.rand(shape, dtype=h.dtype, device=h.device)).floor_()
        else:
            factor = (path_keep != 0).to(h.dtype).view(shape)
        h = h.div(keep_prob) * factor
    s = x + h
    return s, F.layer_norm(s, (s.shape[-1],), weight.to(s.dtype), bias.to(s.dtype), eps)


def add_layer_norm_launch_refusal(is_cuda: bool, dtype, rows: int, hidden: int, grad: bool, param_dtype=None,
                                  foreign: bool = False):
    """None when csrc/prenorm.hip takes a call with these properties, else the reason it does not (a string): CPU
    tensors, a type other than float32 / bfloat16 / float16, float16 with gradients, no rows, a row wider than the
    launch holds, parameters that are neither float32 nor of the type of x, or a branch, parameter or keep tensor of
    another type or on another device (`foreign`).  A pure function."""
    if not is_cuda:
        return "operands that are not on a HIP device"
    if dtype not in ops.PRENORM_DTYPES:
        return f"{dtype} operands"
    if dtype == torch.float16 and grad:
        return "float16 with gradients"
    if rows < 1 or hidden < 1 or not ops.prenorm_fits(hidden, dtype):
        return f"rows = {rows}, hidden = {hidden}"
    if param_dtype is not None and param_dtype not in (torch.float32, dtype):
        return f"{param_dtype} parameters beside {dtype} operands"
    if foreign:
        return "a branch, parameter or keep tensor of another type or on another device"
    return None


def add_layer_norm(x, branch, weight, bias, *, eps: float = 1e-6, dropout_p: float = 0.0, drop_path_p: float = 0.0,
                   training: bool = False, keep=None, path_keep=None, route: str = None):
    """(stream, normed): the step between the branches of a pre-norm transformer block,

        stream = x + branch * keep / (1 - p) * path_keep[sample] / (1 - p_path)
        normed = weight * (stream - mean(stream)) / sqrt(var(stream) + eps) + bias

    with the biased variance and eps inside the root (nn.LayerNorm).  x: (B, N, C), a sample being x[b], or (rows, C)
    with every row its own sample.  Dropout and DropPath act only when `training` and their rate is > 0: `keep` (the
    shape of x) and `path_keep` ((B,)), bytes with nonzero = kept, are drawn with torch's generator when not given.
    Both outputs are differentiable in x, branch, weight and bias; the gradients of x and branch are always two
    tensors.  `route`: None (the launch where it takes the call and the measured rule `ops.prenorm_pays` says it is
    ahead), "launch" (csrc/prenorm.hip: one launch forward, two backward; the statistics are those of the stream as
    stored in the type of x) or "composed" (torch operations).  The launch takes HIP tensors of float32 or bfloat16
    (float16 without gradients) with at most `ops.bertnorm_hmax()` columns and parameters in float32 or the type of x,
    read in place where the strides allow it.  Everything else goes to the composed route under `route=None` and raises
    under `route="launch"`."""
    who = "add_layer_norm"
    if route not in (None, "launch", "composed"):
        raise ValueError(f"{who}: route is None, 'launch' or 'composed' (got {route!r})")
    _add_layer_norm_args(x, branch, weight, bias, dropout_p, drop_path_p, keep, path_keep, who)
    hidden = x.shape[-1]
    rows = x.numel() // hidden
    nper = x.shape[1] if x.dim() == 3 else 1
    p = float(dropout_p) if training else 0.0
    p_path = float(drop_path_p) if training else 0.0
    grad = _needs_grad(x, branch, weight, bias)
    foreign = branch.dtype != x.dtype or branch.device != x.device or weight.device != x.device \
        or bias.device != x.device or weight.dtype != bias.dtype \
        or (keep is not None and p > 0.0 and keep.device != x.device) \
        or (path_keep is not None and p_path > 0.0 and path_keep.device != x.device)
    why = add_layer_norm_launch_refusal(x.is_cuda, x.dtype, rows, hidden, grad, weight.dtype, foreign)
    if route == "launch" and why is not None:
        raise TadmmError(-1, f"{who}: route='launch' cannot take {why}")
    launch = why is None and (route == "launch" or (route is None and ops.prenorm_pays(rows, hidden, x.dtype, grad)))
    if not launch:
        return add_layer_norm_composed(x, branch, weight, bias, eps=eps, dropout_p=dropout_p, drop_path_p=drop_path_p,
                                       training=training, keep=keep, path_keep=path_keep)
    if p > 0.0 and keep is None:
        keep = residual_keep_mask(x.shape, p, x.device)
    if p_path > 0.0 and path_keep is None:
        path_keep = drop_path_keep_mask(x.shape[0], p_path, x.device)
    s, y = _PreNormFn.apply(x.reshape(rows, hidden), branch.reshape(rows, hidden), weight, bias,
                            keep.reshape(rows, hidden) if p > 0.0 else None, path_keep if p_path > 0.0 else None,
                            float(eps), p, p_path, int(nper))
    return s.view(x.shape), y.view(x.shape)


# ---------------------------------------------------------------------------------------------------------------
# ResNet block tail (csrc/bnact.hip): BatchNorm2d, the shortcut added over a channel window, ReLU -- relu(bn(conv(x)))
# and relu(bn(conv(x)) + shortcut(x)) of resnet_cifar_tt.py and resnet_inet_tt.py.
# ---------------------------------------------------------------------------------------------------------------
class _BnActFn(torch.autograd.Function):
    """x (N, C, H, W); `buffers` = (running_mean, running_var, num_batches_tracked), updated in place by the launch and
    handed over as a tuple: they are no inputs of the graph."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, buffers, c0, training, momentum, eps, relu):
        need = any(ctx.needs_input_grad[:4])
        running_mean, running_var, nbt = buffers
        y, stats = ops.bnact_fwd(x, weight, bias, running_mean, running_var, residual, c0=c0, training=training,
                                 momentum=momentum, eps=eps, relu=relu, num_batches_tracked=nbt, need_stats=need)
        if need:
            ctx.save_for_backward(x, y, weight, stats)
        ctx.cfg = (c0, 0 if residual is None else residual.shape[1], relu)
        return y

    @staticmethod
    def backward(ctx, g):
        x, y, weight, stats = ctx.saved_tensors
        c0, cr, relu = ctx.cfg
        need = ctx.needs_input_grad
        dx, dres, dgamma, dbeta = ops.bnact_bwd(g, y if relu else None, x, weight, stats, relu=relu, c0=c0,
                                                res_channels=cr, need=(need[0], need[3], need[1], need[2]))
        return (dx, dgamma, dbeta, dres) + (None,) * 6


def _batch_norm_act_args(x, running_mean, running_var, weight, bias, residual, c0, momentum, who):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{who}: x must be an (N, C, H, W) tensor")
    c = x.shape[1]
    for n, t in (("running_mean", running_mean), ("running_var", running_var), ("weight", weight), ("bias", bias)):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (c,)):
            raise ValueError(f"{who}: {n} must be a ({c},) tensor or None")
    if momentum is not None and not 0.0 <= float(momentum) <= 1.0:
        raise ValueError(f"{who}: momentum must be in [0, 1] or None (got {momentum})")
    if residual is not None:
        ok = isinstance(residual, torch.Tensor) and residual.dim() == 4 and residual.shape[1] >= 1 \
            and (residual.shape[0], residual.shape[2], residual.shape[3]) == (x.shape[0], x.shape[2], x.shape[3])
        if not ok:
            raise ValueError(f"{who}: residual must be ({x.shape[0]}, Cr, {x.shape[2]}, {x.shape[3]})")
        if int(c0) < 0 or int(c0) + residual.shape[1] > c:
            raise ValueError(f"{who}: the residual's channels [{c0}, {c0} + {residual.shape[1]}) are not inside the {c} of x")
    elif int(c0) != 0:
        raise ValueError(f"{who}: res_channel_offset without a residual")


def batch_norm_act_composed(x, running_mean, running_var, weight, bias, residual=None, *, res_channel_offset: int = 0,
                            training: bool, momentum=0.1, eps: float = 1e-5, relu: bool = True, num_batches_tracked=None):
    """`batch_norm_act` from torch operations, under autograd, on any device and in float64: `F.batch_norm`, the
    residual through `F.pad` over the channels where it is narrower than x, the add, `F.relu`.  As nn.BatchNorm2d does,
    a training call first adds one to `num_batches_tracked` (where given and the running statistics are tracked) and
    `momentum=None` is the cumulative average 1 / num_batches_tracked.  The route for what the launch refuses and the
    yardstick of tests/test_gpu_bnact.py and scripts/bench_resnet_block.py."""
    _batch_norm_act_args(x, running_mean, running_var, weight, bias, residual, res_channel_offset, momentum,
                         "batch_norm_act_composed")
    factor = 0.0 if momentum is None else float(momentum)
    if training and running_mean is not None and num_batches_tracked is not None:
        num_batches_tracked.add_(1)
        if momentum is None:
            factor = 1.0 / float(num_batches_tracked)
    y = F.batch_norm(x, running_mean, running_var, weight, bias, training, factor, eps)
    if residual is not None:
        c0, extra = int(res_channel_offset), x.shape[1] - residual.shape[1]
        if extra:
            residual = F.pad(residual, (0, 0, 0, 0, c0, extra - c0), "constant", 0)
        y = y + residual
    return F.relu(y) if relu else y


def batch_norm_act_launch_refusal(is_cuda: bool, dtype, shape, grad: bool, training: bool, contiguous: bool = True,
                                  param_dtypes=(torch.float32,), affine: bool = True, tracked: bool = True,
                                  momentum_given: bool = True, foreign: bool = False):
    """None when csrc/bnact.hip takes a call with these properties, else the reason it does not (a string): CPU
    tensors, a type other than float32 / bfloat16 / float16, float16 with gradients, eval mode with gradients, an x that
    is not NCHW contiguous, more values per channel than the launch takes, parameters or running statistics that are
    missing (`affine=False`, `track_running_stats=False`) or not float32, `momentum=None`, or an operand of another
    type or on another device (`foreign`).  A pure function."""
    if not is_cuda:
        return "operands that are not on a HIP device"
    if dtype not in ops.BNACT_DTYPES:
        return f"{dtype} operands"
    if dtype == torch.float16 and grad:
        return "float16 with gradients"
    if grad and not training:
        return "eval mode with gradients"
    if not contiguous:
        return "an x that is not NCHW contiguous"
    if min(shape) < 1 or not ops.bnact_fits(*shape, dtype):
        return f"shape = {tuple(shape)}"
    if training and shape[0] * shape[2] * shape[3] < 2:
        return "one value per channel in training"
    if not affine:
        return "affine=False"
    if not tracked:
        return "track_running_stats=False"
    if any(d != torch.float32 for d in param_dtypes):
        return "parameters or running statistics that are not float32"
    if not momentum_given:
        return "momentum=None"
    if foreign:
        return "a residual, parameter or buffer of another type or on another device"
    return None


def batch_norm_act(x, running_mean, running_var, weight, bias, residual=None, *, res_channel_offset: int = 0,
                   training: bool, momentum=0.1, eps: float = 1e-5, relu: bool = True, num_batches_tracked=None,
                   route: str = None):
    """The tail of a ResNet block,

        y = act(weight (x - mean) / sqrt(var + eps) + bias + residual),    act = relu or the identity,

    over x (N, C, H, W) with the arguments of `F.batch_norm`: batch statistics (biased variance) when `training`, which
    also updates `running_mean` / `running_var` in place (momentum, unbiased variance) and adds one to
    `num_batches_tracked`; the running statistics otherwise.  `residual` (N, Cr, H, W) is added to the channels
    [res_channel_offset, res_channel_offset + Cr) -- the whole of x, or the option-A shortcut
    `x_in[:, :, ::2, ::2]` at offset planes // 4, read through its strides with neither the slice nor the zero padding
    materialised.  Differentiable in x, weight, bias and residual.  `route`: None (the launch where it takes the call
    and the measured rule `ops.bnact_pays` says it is ahead), "launch" (csrc/bnact.hip: two launches in training, one in
    eval, two backward) or "composed" (torch operations).  The launch takes NCHW-contiguous HIP tensors of float32 or
    bfloat16 (float16 without gradients) with float32 parameters and running statistics, a momentum, and gradients only
    in training mode.  Everything else goes to the composed route under `route=None` and raises under `route="launch"`."""
    who = "batch_norm_act"
    if route not in (None, "launch", "composed"):
        raise ValueError(f"{who}: route is None, 'launch' or 'composed' (got {route!r})")
    _batch_norm_act_args(x, running_mean, running_var, weight, bias, residual, res_channel_offset, momentum, who)
    training = bool(training)
    grad = _needs_grad(x, weight, bias, residual)
    params = [t for t in (weight, bias, running_mean, running_var) if t is not None]
    foreign = any(t.device != x.device for t in params) \
        or (residual is not None and (residual.dtype != x.dtype or residual.device != x.device)) \
        or (num_batches_tracked is not None and (num_batches_tracked.device != x.device
                                                 or num_batches_tracked.dtype != torch.int64))
    why = None
    if route != "composed":
        why = batch_norm_act_launch_refusal(x.is_cuda, x.dtype, tuple(x.shape), grad, training, x.is_contiguous(),
                                            tuple(t.dtype for t in params), weight is not None and bias is not None,
                                            running_mean is not None and running_var is not None, momentum is not None,
                                            foreign)
    if route == "launch" and why is not None:
        raise TadmmError(-1, f"{who}: route='launch' cannot take {why}")
    n, c, h, w = x.shape
    launch = route != "composed" and why is None and (
        route == "launch" or ops.bnact_pays(n, c, h * w, x.dtype, grad, residual is not None))
    if not launch:
        return batch_norm_act_composed(x, running_mean, running_var, weight, bias, residual,
                                       res_channel_offset=res_channel_offset, training=training, momentum=momentum,
                                       eps=eps, relu=relu, num_batches_tracked=num_batches_tracked)
    return _BnActFn.apply(x, weight, bias, residual, (running_mean, running_var, num_batches_tracked),
                          int(res_channel_offset), training, float(momentum), float(eps), bool(relu))


def batch_norm_act_module(bn, x, residual=None, res_channel_offset: int = 0, relu: bool = True, route: str = None):
    """`batch_norm_act` with the parameters, buffers and mode of the module `bn`.  An nn.BatchNorm2d keeps its state-dict
    keys and semantics (batch statistics in training mode or when it tracks none); any other norm layer is called as
    it is and the residual and the ReLU are composed around it."""
    if not isinstance(bn, torch.nn.BatchNorm2d):
        y = bn(x)
        if residual is not None:
            extra = y.shape[1] - residual.shape[1]
            if extra:
                residual = F.pad(residual, (0, 0, 0, 0, res_channel_offset, extra - res_channel_offset), "constant", 0)
            y = y + residual
        return F.relu(y) if relu else y
    training = bn.training or (bn.running_mean is None and bn.running_var is None)
    return batch_norm_act(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, residual,
                          res_channel_offset=res_channel_offset, training=training, momentum=bn.momentum, eps=bn.eps,
                          relu=relu, num_batches_tracked=bn.num_batches_tracked if bn.training else None, route=route)


# ---------------------------------------------------------------------------------------------------------------
# DenseNet pre-activation (csrc/densebn.hip): relu(bn(torch.cat(features, 1))) in front of every convolution of a dense
# block of densenet_cifar_tt.py and densenet_inet_tt.py, with neither the concatenation nor repeated statistics.
# ---------------------------------------------------------------------------------------------------------------
class DenseFeatures:
    """The feature tensors of one dense block, in order: a small list-like holder (`append`, `len`, indexing,
    iteration, `channels`, `cat()`) that also keeps, per segment, the batch statistics `ops.densebn_stats` computed for
    it -- float64 (C_k, 2) = (mean, biased variance), created on first use in training mode and kept for the life of
    the holder: channel c of the concatenation holds the same numbers for every later layer of the block, so its mean
    and variance are computed once per feature tensor, not once per consumer."""

    def __init__(self, tensors=()):
        self._segments = []
        self._stats = []
        for t in ([tensors] if isinstance(tensors, torch.Tensor) else tensors):
            self.append(t)

    def append(self, t):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError("DenseFeatures: a segment is an (N, C, H, W) tensor")
        self._segments.append(t)
        self._stats.append(None)
        return self

    def __len__(self):
        return len(self._segments)

    def __getitem__(self, i):
        return self._segments[i]

    def __iter__(self):
        return iter(self._segments)

    @property
    def channels(self) -> int:
        return sum(t.shape[1] for t in self._segments)

    def cat(self):
        """torch.cat(segments, 1); a single segment is returned as it is."""
        return self._segments[0] if len(self._segments) == 1 else torch.cat(self._segments, 1)

    def stats(self):
        """One stats tensor per segment (two launches for each segment that has none yet)."""
        for k, t in enumerate(self._segments):
            if self._stats[k] is None:
                self._stats[k] = ops.densebn_stats(t.detach())
        return list(self._stats)


def _dense_features(feats):
    if isinstance(feats, DenseFeatures):
        return feats
    return DenseFeatures(feats)


class _DenseBnFn(torch.autograd.Function):
    """The tensor inputs are weight, bias and the segments.  `buffers` = (running_mean, running_var,
    num_batches_tracked), updated in place by the launch, and `stats` (one per segment, from the holder) are handed over
    as tuples: they are no inputs of the graph.  The backward returns one fresh contiguous gradient per segment that
    needs one; torch's own accumulation adds the contributions of the layers that share a segment."""

    @staticmethod
    def forward(ctx, weight, bias, buffers, stats, training, momentum, eps, relu, *segments):
        running_mean, running_var, nbt = buffers
        y = ops.densebn_fwd(segments, stats, weight, bias, running_mean, running_var, training=training,
                            momentum=momentum, eps=eps, relu=relu, num_batches_tracked=nbt)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(y, weight, *segments)
            ctx.stats = stats
        ctx.cfg = (eps, relu)
        return y

    @staticmethod
    def backward(ctx, g):
        y, weight, *segments = ctx.saved_tensors
        eps, relu = ctx.cfg
        need = ctx.needs_input_grad
        dxs, dgamma, dbeta = ops.densebn_bwd(g, y if relu else None, segments, ctx.stats, weight, eps=eps, relu=relu,
                                             need_dx=need[8:], need_dgamma=need[0], need_dbeta=need[1])
        return (dgamma, dbeta) + (None,) * 6 + tuple(dxs)


def _dense_batch_norm_act_args(feats, running_mean, running_var, weight, bias, momentum, who):
    if len(feats) < 1:
        raise ValueError(f"{who}: at least one feature tensor is needed")
    c = feats.channels
    for n, t in (("running_mean", running_mean), ("running_var", running_var), ("weight", weight), ("bias", bias)):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (c,)):
            raise ValueError(f"{who}: {n} must be a ({c},) tensor or None")
    if momentum is not None and not 0.0 <= float(momentum) <= 1.0:
        raise ValueError(f"{who}: momentum must be in [0, 1] or None (got {momentum})")


def dense_batch_norm_act_composed(feats, running_mean, running_var, weight, bias, *, training: bool, momentum=0.1,
                                  eps: float = 1e-5, relu: bool = True, num_batches_tracked=None):
    """`dense_batch_norm_act` from torch operations, under autograd, on any device and in float64: `torch.cat` of the
    feature tensors, `F.batch_norm`, `F.relu`.  As nn.BatchNorm2d does, a training call first adds one to
    `num_batches_tracked` (where given and the running statistics are tracked) and `momentum=None` is the cumulative
    average 1 / num_batches_tracked.  The route for everything the launch refuses and the yardstick of
    tests/test_gpu_densebn.py and scripts/bench_densenet_block.py."""
    feats = _dense_features(feats)
    _dense_batch_norm_act_args(feats, running_mean, running_var, weight, bias, momentum, "dense_batch_norm_act_composed")
    factor = 0.0 if momentum is None else float(momentum)
    if training and running_mean is not None and num_batches_tracked is not None:
        num_batches_tracked.add_(1)
        if momentum is None:
            factor = 1.0 / float(num_batches_tracked)
    y = F.batch_norm(feats.cat(), running_mean, running_var, weight, bias, training, factor, eps)
    return F.relu(y) if relu else y


def dense_batch_norm_act_launch_refusal(is_cuda: bool, dtypes, shapes, grad: bool, training: bool,
                                        contiguous: bool = True, param_dtypes=(torch.float32,), affine: bool = True,
                                        tracked: bool = True, momentum_given: bool = True, foreign: bool = False):
    """None when csrc/densebn.hip takes a call with these properties, else the reason it does not (a string).  `dtypes`
    and `shapes` are those of the feature tensors, in order.  Reasons: CPU tensors, mixed types, a type other than float32
    / bfloat16 / float16, float16 with gradients, a step in eval mode, a segment that is not NCHW contiguous, segments
    whose (N, H, W) differ, more segments than `ops.densebn_max_segments()`, more values per channel than the launch
    takes, one value per channel in training, parameters or running statistics that are missing (`affine=False`,
    `track_running_stats=False`) or not float32, `momentum=None`, or an operand on another device (`foreign`).  A pure
    function."""
    if not is_cuda:
        return "operands that are not on a HIP device"
    dtypes, shapes = tuple(dtypes), tuple(tuple(s) for s in shapes)
    if len(set(dtypes)) != 1:
        return "feature tensors of mixed types"
    if dtypes[0] not in ops.DENSEBN_DTYPES:
        return f"{dtypes[0]} operands"
    if dtypes[0] == torch.float16 and grad:
        return "float16 with gradients"
    if grad and not training:
        return "eval mode with gradients"
    if not contiguous:
        return "a feature tensor that is not NCHW contiguous"
    if any(len(s) != 4 or min(s) < 1 for s in shapes) or len({(s[0], s[2], s[3]) for s in shapes}) != 1:
        return "feature tensors of mixed shapes"
    if len(shapes) > ops.densebn_max_segments():
        return f"{len(shapes)} feature tensors (at most {ops.densebn_max_segments()})"
    n, _, h, w = shapes[0]
    if not ops.densebn_fits(n, [s[1] for s in shapes], h, w, dtypes[0]):
        return f"shape = {(n, sum(s[1] for s in shapes), h, w)}"
    if training and n * h * w < 2:
        return "one value per channel in training"
    if not affine:
        return "affine=False"
    if not tracked:
        return "track_running_stats=False"
    if any(d != torch.float32 for d in param_dtypes):
        return "parameters or running statistics that are not float32"
    if not momentum_given:
        return "momentum=None"
    if foreign:
        return "a feature tensor, parameter or buffer on another device"
    return None


def dense_batch_norm_act(feats, running_mean, running_var, weight, bias, *, training: bool, momentum=0.1,
                         eps: float = 1e-5, relu: bool = True, num_batches_tracked=None, route: str = None):
    """The pre-activation of a DenseNet layer,

        y = act(weight (cat(feats, 1) - mean) / sqrt(var + eps) + bias),    act = relu or the identity,

    over the feature tensors `feats` (a `DenseFeatures`, a sequence of (N, C_k, H, W) tensors, or a plain tensor as a
    one-segment list) with the arguments of `F.batch_norm`: batch statistics (biased variance) when `training`, which
    also updates `running_mean` / `running_var` in place (momentum, unbiased variance) and adds one to
    `num_batches_tracked`; the running statistics otherwise.  Differentiable in every feature tensor, weight and bias.
    `route`: None (the launch where it takes the call and the measured rule `ops.densebn_pays` says it is ahead),
    "launch" (csrc/densebn.hip: every channel read from the tensor that owns it, y written once; the batch statistics
    of a feature tensor are computed once, by the `DenseFeatures` that holds it, so hand the same holder to every layer
    of a block; two launches backward) or "composed" (torch.cat + F.batch_norm + relu).  The launch takes NCHW-contiguous
    HIP tensors of one type, float32 or bfloat16 (float16 without gradients), with float32 parameters and running
    statistics, a momentum, and gradients only in training mode.  Everything else goes to the composed route under
    `route=None` and raises under `route="launch"`."""
    who = "dense_batch_norm_act"
    if route not in (None, "launch", "composed"):
        raise ValueError(f"{who}: route is None, 'launch' or 'composed' (got {route!r})")
    feats = _dense_features(feats)
    _dense_batch_norm_act_args(feats, running_mean, running_var, weight, bias, momentum, who)
    training = bool(training)
    segments = list(feats)
    x0 = segments[0]
    grad = _needs_grad(weight, bias, *segments)
    params = [t for t in (weight, bias, running_mean, running_var) if t is not None]
    foreign = any(t.device != x0.device for t in params + segments) \
        or (num_batches_tracked is not None and (num_batches_tracked.device != x0.device
                                                 or num_batches_tracked.dtype != torch.int64))
    why = None
    if route != "composed":
        why = dense_batch_norm_act_launch_refusal(
            all(t.is_cuda for t in segments), [t.dtype for t in segments], [t.shape for t in segments], grad, training,
            all(t.is_contiguous() for t in segments), tuple(t.dtype for t in params),
            weight is not None and bias is not None, running_mean is not None and running_var is not None,
            momentum is not None, foreign)
    if route == "launch" and why is not None:
        raise TadmmError(-1, f"{who}: route='launch' cannot take {why}")
    launch = route != "composed" and why is None and (
        route == "launch" or ops.densebn_pays(x0.shape[0], feats.channels, x0.shape[2] * x0.shape[3], len(segments),
                                              x0.dtype, grad))
    if not launch:
        return dense_batch_norm_act_composed(feats, running_mean, running_var, weight, bias, training=training,
                                             momentum=momentum, eps=eps, relu=relu,
                                             num_batches_tracked=num_batches_tracked)
    stats = tuple(feats.stats()) if training else None
    return _DenseBnFn.apply(weight, bias, (running_mean, running_var, num_batches_tracked), stats, training,
                            float(momentum), float(eps), bool(relu), *segments)


def dense_batch_norm_act_module(bn, feats, route: str = None, relu: bool = True):
    """`dense_batch_norm_act` with the parameters, buffers and mode of the module `bn`.  An nn.BatchNorm2d keeps its
    state-dict keys and semantics (batch statistics in training mode or when it tracks none); any other norm layer is
    called on the concatenation and the ReLU is composed behind it."""
    feats = _dense_features(feats)
    if not isinstance(bn, torch.nn.BatchNorm2d):
        y = bn(feats.cat())
        return F.relu(y) if relu else y
    training = bn.training or (bn.running_mean is None and bn.running_var is None)
    return dense_batch_norm_act(feats, bn.running_mean, bn.running_var, bn.weight, bn.bias, training=training,
                                momentum=bn.momentum, eps=bn.eps, relu=relu,
                                num_batches_tracked=bn.num_batches_tracked if bn.training else None, route=route)


# ---------------------------------------------------------------------------------------------------------------
# MobileNetV2 depthwise stage (csrc/dwbn.hip): relu6(bn(depthwise_conv3x3(x))), the middle of every inverted-residual
# block of mobilenetv2_cifar_tt.py and mobilenetv2_tt.py.
# ---------------------------------------------------------------------------------------------------------------
class _DwBnFn(torch.autograd.Function):
    """x (N, C, H, W); `buffers` = (running_mean, running_var, num_batches_tracked), updated in place by the launch and
    handed over as a tuple: they are no inputs of the graph."""

    @staticmethod
    def forward(ctx, x, conv_weight, weight, bias, buffers, stride, training, momentum, eps):
        need = any(ctx.needs_input_grad[:4])
        running_mean, running_var, nbt = buffers
        y, z, stats = ops.dwbn_fwd(x, conv_weight, weight, bias, running_mean, running_var, stride=stride,
                                   training=training, momentum=momentum, eps=eps, num_batches_tracked=nbt,
                                   need_stats=need)
        if need:
            ctx.save_for_backward(x, y, z, conv_weight, weight, stats)
        ctx.stride = stride
        return y

    @staticmethod
    def backward(ctx, g):
        x, y, z, conv_weight, weight, stats = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dw, dgamma, dbeta = ops.dwbn_bwd(g, y, z, x, conv_weight, weight, stats, stride=ctx.stride,
                                             need=(need[0], need[1], need[2], need[3]))
        return (dx, dw, dgamma, dbeta) + (None,) * 5


def _depthwise_args(x, conv_weight, running_mean, running_var, weight, bias, momentum, who):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{who}: x must be an (N, C, H, W) tensor")
    c = x.shape[1]
    if not isinstance(conv_weight, torch.Tensor) or conv_weight.dim() != 4 or conv_weight.shape[0] != c \
            or conv_weight.shape[1] != 1:
        raise ValueError(f"{who}: conv_weight must be a ({c}, 1, kh, kw) tensor (depth multiplier 1)")
    for n, t in (("running_mean", running_mean), ("running_var", running_var), ("weight", weight), ("bias", bias)):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (c,)):
            raise ValueError(f"{who}: {n} must be a ({c},) tensor or None")
    if momentum is not None and not 0.0 <= float(momentum) <= 1.0:
        raise ValueError(f"{who}: momentum must be in [0, 1] or None (got {momentum})")


def depthwise_bn_relu6_composed(x, conv_weight, running_mean, running_var, weight, bias, *, stride=1, padding=1,
                                dilation=1, training: bool, momentum=0.1, eps: float = 1e-5, num_batches_tracked=None):
    """`depthwise_bn_relu6` from torch operations, under autograd, on any device and in float64: `F.conv2d` with
    `groups = C` (the weight cast to the type of x), `F.batch_norm`, `F.relu6`.  As nn.BatchNorm2d does, a training
    call first adds one to `num_batches_tracked` (where given and the running statistics are tracked) and
    `momentum=None` is the cumulative average 1 / num_batches_tracked.  The route for what the launch refuses and the
    yardstick of tests/test_gpu_dwbn.py and scripts/bench_mobilenet_block.py."""
    _depthwise_args(x, conv_weight, running_mean, running_var, weight, bias, momentum, "depthwise_bn_relu6_composed")
    factor = 0.0 if momentum is None else float(momentum)
    if training and running_mean is not None and num_batches_tracked is not None:
        num_batches_tracked.add_(1)
        if momentum is None:
            factor = 1.0 / float(num_batches_tracked)
    z = F.conv2d(x, conv_weight.to(x.dtype), None, stride, padding, dilation, x.shape[1])
    return F.relu6(F.batch_norm(z, running_mean, running_var, weight, bias, training, factor, eps))


def depthwise_bn_relu6_launch_refusal(is_cuda: bool, dtype, shape, stride, grad: bool, training: bool,
                                      contiguous: bool = True, kernel=(3, 3), padding=(1, 1), dilation=(1, 1),
                                      param_dtypes=(torch.float32,), affine: bool = True, tracked: bool = True,
                                      momentum_given: bool = True, foreign: bool = False):
    """None when csrc/dwbn.hip takes a call with these properties, else the reason it does not (a string): CPU tensors,
    a type other than float32 / bfloat16 / float16, float16 with gradients, eval mode with gradients, an x that is not
    NCHW contiguous, a kernel other than 3x3 with padding 1 and dilation 1, a stride other than 1 and 2 (or two
    different ones), a plane wider than the launch takes, fewer than two output values per channel in training,
    parameters or running statistics that are missing (`affine=False`, `track_running_stats=False`) or not float32,
    `momentum=None`, or an operand on another device (`foreign`).  A pure function."""
    if not is_cuda:
        return "operands that are not on a HIP device"
    if dtype not in ops.DWBN_DTYPES:
        return f"{dtype} operands"
    if dtype == torch.float16 and grad:
        return "float16 with gradients"
    if grad and not training:
        return "eval mode with gradients"
    if not contiguous:
        return "an x that is not NCHW contiguous"
    if ops._pair(kernel) != (3, 3) or ops._pair(padding) != (1, 1) or ops._pair(dilation) != (1, 1):
        return f"kernel {ops._pair(kernel)}, padding {ops._pair(padding)}, dilation {ops._pair(dilation)}"
    st = ops._pair(stride)
    if st not in ((1, 1), (2, 2)):
        return f"stride {st}"
    if min(shape) < 1 or not ops.dwbn_fits(*shape, st[0], dtype):
        return f"shape = {tuple(shape)}"
    ho, wo = ops.dwbn_out_hw(shape[2], shape[3], st[0])
    if training and shape[0] * ho * wo < 2:
        return "one output value per channel in training"
    if not affine:
        return "affine=False"
    if not tracked:
        return "track_running_stats=False"
    if any(d != torch.float32 for d in param_dtypes):
        return "parameters or running statistics that are not float32"
    if not momentum_given:
        return "momentum=None"
    if foreign:
        return "a parameter or buffer of another type or on another device"
    return None


def depthwise_bn_relu6(x, conv_weight, running_mean, running_var, weight, bias, *, stride, padding=1, dilation=1,
                       training: bool, momentum=0.1, eps: float = 1e-5, num_batches_tracked=None, route: str = None):
    """The middle of a MobileNetV2 inverted-residual block,

        y = relu6(weight (z - mean) / sqrt(var + eps) + bias),    z = depthwise_conv3x3(x; conv_weight, stride, padding 1),

    over x (N, C, H, W) and `conv_weight` (C, 1, 3, 3) with the batch-norm arguments of `F.batch_norm`: batch statistics
    (biased variance) when `training`, which also updates `running_mean` / `running_var` in place (momentum, unbiased
    variance) and adds one to `num_batches_tracked`; the running statistics otherwise.  Differentiable in x,
    conv_weight, weight and bias.  `route`: None (the launch where it takes the call and the measured rule
    `ops.dwbn_pays` says it is ahead), "launch" (csrc/dwbn.hip: two launches in training, one in eval, three backward)
    or "composed" (`F.conv2d(groups=C)`, `F.batch_norm`, `F.relu6`).  The launch takes NCHW-contiguous HIP tensors of
    float32 or bfloat16 (float16 without gradients), a 3x3 kernel with padding 1, dilation 1 and stride 1 or 2, float32
    parameters and running statistics, a momentum, and gradients only in training mode.  Everything else goes to the
    composed route under `route=None` and raises under `route="launch"`."""
    who = "depthwise_bn_relu6"
    if route not in (None, "launch", "composed"):
        raise ValueError(f"{who}: route is None, 'launch' or 'composed' (got {route!r})")
    _depthwise_args(x, conv_weight, running_mean, running_var, weight, bias, momentum, who)
    training = bool(training)
    grad = _needs_grad(x, conv_weight, weight, bias)
    params = [t for t in (conv_weight, weight, bias, running_mean, running_var) if t is not None]
    foreign = any(t.device != x.device for t in params) \
        or (num_batches_tracked is not None and (num_batches_tracked.device != x.device
                                                 or num_batches_tracked.dtype != torch.int64))
    why = None
    if route != "composed":
        why = depthwise_bn_relu6_launch_refusal(
            x.is_cuda, x.dtype, tuple(x.shape), stride, grad, training, x.is_contiguous(), tuple(conv_weight.shape[2:]),
            padding, dilation, tuple(t.dtype for t in params), weight is not None and bias is not None,
            running_mean is not None and running_var is not None, momentum is not None, foreign)
    if route == "launch" and why is not None:
        raise TadmmError(-1, f"{who}: route='launch' cannot take {why}")
    n, c, h, w = x.shape
    launch = route != "composed" and why is None and (
        route == "launch" or ops.dwbn_pays(n, c, h, w, ops._pair(stride)[0], x.dtype, grad))
    if not launch:
        return depthwise_bn_relu6_composed(x, conv_weight, running_mean, running_var, weight, bias, stride=stride,
                                           padding=padding, dilation=dilation, training=training, momentum=momentum,
                                           eps=eps, num_batches_tracked=num_batches_tracked)
    return _DwBnFn.apply(x, conv_weight, weight, bias, (running_mean, running_var, num_batches_tracked),
                         ops._pair(stride)[0], training, float(momentum), float(eps))


def depthwise_bn_relu6_module(conv, bn, x, route: str = None):
    """`depthwise_bn_relu6` with the parameters, buffers and mode of the modules `conv` (an nn.Conv2d with groups equal
    to its channels) and `bn`.  An nn.BatchNorm2d keeps its state-dict keys and semantics; a convolution with a bias or a
    depth multiplier, or any other norm layer, is called as it is with `F.relu6` behind it."""
    ok = isinstance(conv, torch.nn.Conv2d) and isinstance(bn, torch.nn.BatchNorm2d) and conv.bias is None \
        and conv.groups == conv.in_channels == conv.out_channels and conv.padding_mode == "zeros" \
        and not isinstance(conv.padding, str)
    if not ok:
        return F.relu6(bn(conv(x)))
    training = bn.training or (bn.running_mean is None and bn.running_var is None)
    return depthwise_bn_relu6(x, conv.weight, bn.running_mean, bn.running_var, bn.weight, bn.bias, stride=conv.stride,
                              padding=conv.padding, dilation=conv.dilation, training=training, momentum=bn.momentum,
                              eps=bn.eps, num_batches_tracked=bn.num_batches_tracked if bn.training else None,
                              route=route)
