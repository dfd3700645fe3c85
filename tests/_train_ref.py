"""Yardsticks and case tables of the training-side kernel tests (tests/test_train_ref_cpu.py, tests/test_gpu_train_variants.py):
the weight gradient `wgrad_kernel`, the core-convolution weight gradient `core_wgrad_kernel` (csrc/wgrad.hip), the core
convolution `core_conv_kernel` (csrc/coreconv.hip) and the one-launch factorised convolution `tt_conv_kernel`
(csrc/convchain.hip).  Importing this file needs no GPU and, apart from the plan queries, no built library.

It holds
  * the variant tables: every instantiation of the four templates;
  * Python restatements of the three host rules that pick a variant (`wgrad_tile` with the slice rule of `wgrad_geom` /
    `core_wgrad_geom`, the NBW rule of `cc_launch`, and the conv-chain tile rule, which tests/test_conv_chain_plan_cpu.py
    states and this file imports);
  * the case tables of the GPU file, with the variant each case is meant to reach (the CPU file checks that it does);
  * float64 references with DERIVED elementwise bounds.  Guards, the CPU models and the bounds' constants are those of
    tests/_chain_ref.py and tests/_fp16_ref.py.

Bounds, with u the unit roundoff of a 16-bit type, ACC = 2^-24 and every `allabs` the same computation on absolute values
in float64:
  weight gradients (one product of T terms, float32 result, nothing rounded to 16 bits)
      float32 operands   1.5 (T + 5) ACC |alpha| (|A|^T |B|)     the six kept pairs drop at most 2^-23 |a||b| per product
      bfloat16 operands  1.5 (T + 1) ACC |alpha| (|A|^T |B|)     products are exact
  chains of p products (core convolution p = 1; H1, H2, Y and dH2, dH1, dX p = 1, 2, 3) of n accumulated terms in all
      16-bit types       1.5 [u (|ref| + sum over earlier intermediates of |later factors| |intermediate|) + n ACC allabs]
                         -- `conv_bound` of _fp16_ref.py for p = 3 and its prefixes for p = 1, 2
      float32            1.5 (n + 1 + 2 p) ACC allabs            -- `linear_bound_f32` of _chain_ref.py, whose two
                         products give its n + 5: one bias add and two units of 2^-24 per product for the dropped pairs
  rms criterion (float32, and bfloat16 weight gradients): rms(got - ref64) <= 2 rms(plain32 - ref64), plain32 the same
      operation in float32 by torch on the CPU (the factor 2 of _chain_ref.py).
Nothing here is fitted to what a kernel returns."""
import collections
import ctypes as C
import functools
import itertools

import torch
import torch.nn.functional as F

from _chain_ref import ACC, DTYPES, KEPT_PAIRS, U, guarded, guards_intact, same_bits, three_plane_emulation, untouched  # noqa: F401
from test_conv_chain_plan_cpu import _py_plan

ESZ = {"f32": 4, "bf16": 2, "f16": 2}


def _ceil(a, b):
    return -(-a // b)


def pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


# =====================================================================================================================
# variant tables: every instantiation of the four templates
# =====================================================================================================================
TILES = (16, 32, 64)
# wgrad_kernel<P, TM, TN, TIn, IMG>: 36 kernels, each with two epilogues (one slice writes C, several go through the
# workspace and the fp64 reduce)
WGRAD_VARIANTS = [(dn, lay, tm, tn) for dn in ("f32", "bf16") for lay in ("rows", "img") for tm in TILES for tn in TILES]
# core_wgrad_kernel<P, TM, TN, TIn>: 18 kernels, two epilogues each
CORE_WGRAD_VARIANTS = [(dn, tm, tn) for dn in ("f32", "bf16") for tm in TILES for tn in TILES]
# core_conv_kernel<P, KC, NBW, T>: 6 kernels, each forward and data gradient
CORE_CONV_VARIANTS = [(dn, nbw) for dn in ("f32", "bf16") for nbw in (1, 2, 4)]
# tt_conv_kernel<P, TM, KC, NBW, T, BWD, SAVE>: 54 instantiations; float16 has the plain forward only
CONV_MODES = ("fwd", "fwd_save", "bwd", "bwd_save")
CONV_CHAIN_VARIANTS = [(dn, tm, nbw, mode) for dn in ("f32", "bf16") for tm in (32, 64) for nbw in (1, 2, 4) for mode in CONV_MODES] \
    + [("f16", tm, nbw, "fwd") for tm in (32, 64) for nbw in (1, 2, 4)]
assert (len(WGRAD_VARIANTS), len(CORE_WGRAD_VARIANTS), len(CORE_CONV_VARIANTS), len(CONV_CHAIN_VARIANTS)) == (36, 18, 6, 54)


# =====================================================================================================================
# the host rules, restated
# =====================================================================================================================
WG_KC, WG_FOLD, WG_MIN_SLICE, WG_TARGET_WG = 128, 8, 256, 512          # kWgKC, kWgFold, kWgMinSlice, kWgTargetWG


def wgrad_tile(m):
    """Largest tile of {64, 32, 16} that pads the side by at most 1/8 more than 16-wide tiles would (csrc/wgrad.hip)."""
    p16 = _ceil(m, 16) * 16
    for t in (64, 32):
        if _ceil(m, t) * t * 8 <= p16 * 9:
            return t
    return 16


Geom = collections.namedtuple("Geom", "TM TN tiles slices nchunks ws_bytes")


def wgrad_geom(M, N, T, taps=1):
    """`wgrad_geom` (taps == 1) and `core_wgrad_geom` (M = R2, N = R1, T = B * Ho * Wo): tiles, slices of T, chunks of
    128 tokens and the workspace, a function of the shapes alone."""
    tm, tn = wgrad_tile(M), wgrad_tile(N)
    tiles = _ceil(M, tm) * _ceil(N, tn)
    slices = max(1, min(_ceil(WG_TARGET_WG, tiles * taps), T // WG_MIN_SLICE))
    return Geom(tm, tn, tiles, slices, _ceil(T, WG_KC), taps * slices * tiles * tm * tn * 4 if slices > 1 else 0)


def slice_chunks(g):
    """Chunks each slice walks (the kernel's c_begin / c_end)."""
    return [(i + 1) * g.nchunks // g.slices - i * g.nchunks // g.slices for i in range(g.slices)]


def wgrad_vec(byte_offset, step_elems, esz):
    """`wgrad_vec`: 2 = 16-byte loads, 1 = 8-byte loads, 0 = elements, from the base's offset past a 16-byte boundary and
    the step between rows (token rows) or planes (images)."""
    epl = 16 // esz
    if byte_offset % 16 == 0 and step_elems % epl == 0:
        return 2
    if byte_offset % 8 == 0 and step_elems % (epl // 2) == 0:
        return 1
    return 0


def align_class(byte_offset):
    """`align_class` of csrc/coreconv.hip."""
    return 2 if byte_offset % 16 == 0 else (1 if byte_offset % 8 == 0 else 0)


def cc_nbw(features):
    """`cc_launch` / `launch_conv_variant`: 16-wide feature tiles per wave, from the (padded) feature count."""
    tiles = _ceil(features, 16)
    return 1 if tiles <= 4 else (2 if tiles <= 8 else 4)


def conv_chain_variant(dn, x_shape, r1, r2, k, s, p, dl, bwd):
    """(TM, NBW) of `tadmm_ttconv_fused*` by the Python rule, or None where the launch does not apply."""
    plan = _py_plan(tuple(x_shape), DTYPES[dn], r1, r2, pair(k), pair(s), pair(p), pair(dl), bwd)
    if plan is None:
        return None
    return plan[0], cc_nbw(max(_ceil(r1, 32) * 32, _ceil(r2, 32) * 32))


def conv_chain_variant_lib(dn, x_shape, r1, r2, k, s, p, dl, bwd):
    """The same from the library's own `tadmm_ttconv_fused_plan` (host only)."""
    from tadmm import _cabi, ops
    plan = ops._conv_plan(tuple(x_shape), DTYPES[dn], r1, r2, pair(k), pair(s), pair(p), pair(dl),
                          _cabi.CONV_CHAIN_BWD if bwd else _cabi.CONV_CHAIN_FWD)
    if plan is None:
        return None
    return plan[0], cc_nbw(max(_ceil(r1, 32) * 32, _ceil(r2, 32) * 32))


@functools.lru_cache(maxsize=None)
def conv_chain_reachable():
    """{(dn, TM, NBW, "fwd" | "bwd"): first (plane, kernel, stride, R1, R2) that reaches it} over this grid:
    planes 1x1 .. 32x32 and 1x64 (smallest first), kernels 1 / 3 / 5 with padding k // 2, strides 1 / 2, every padded
    rank pair in 32 .. 256, both modes, all three dtypes (float16: forward only), through `tadmm_ttconv_fused_plan`."""
    from tadmm import _cabi
    lib = _cabi.load()
    d = _cabi.ConvChainDesc()
    out = [C.c_int() for _ in range(4)]
    refs = [C.byref(v) for v in out]
    found = {}
    planes = sorted([(h, w) for h in range(1, 33) for w in range(1, 33)] + [(1, 64)], key=lambda q: (q[0] * q[1], q))
    d.B, d.C, d.Nout = 2, 8, 8
    ranks = range(32, 257, 32)
    for (h, w), k, s in itertools.product(planes, (1, 3, 5), (1, 2)):
        p = k // 2
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        if ho <= 0 or wo <= 0:
            continue
        d.H, d.W, d.Ho, d.Wo, d.kh, d.kw = h, w, ho, wo, k, k
        d.stride_h = d.stride_w = s
        d.pad_h = d.pad_w = p
        d.dil_h = d.dil_w = 1
        for dn, code in (("f32", _cabi.CHAIN_F32), ("bf16", _cabi.CHAIN_BF16), ("f16", _cabi.CHAIN_F16)):
            d.dtype = code
            for mode in (("fwd", "bwd") if dn != "f16" else ("fwd",)):
                for r1, r2 in itertools.product(ranks, ranks):
                    d.R1, d.R2 = r1, r2
                    rc = lib.tadmm_ttconv_fused_plan(C.byref(d), _cabi.CONV_CHAIN_BWD if mode == "bwd" else _cabi.CONV_CHAIN_FWD,
                                                     *refs, None)
                    assert rc in (0, -5), rc
                    if rc == 0:
                        found.setdefault((dn, out[0].value, cc_nbw(max(r1, r2)), mode), ((h, w), k, s, r1, r2))
    return found


def conv_chain_targets():
    """The instantiations the grid reaches: SAVE is the caller's choice, so both of a mode's kernels are reachable with it."""
    t = set()
    for dn, tm, nbw, mode in conv_chain_reachable():
        t.add((dn, tm, nbw, mode))
        if dn != "f16":
            t.add((dn, tm, nbw, mode + "_save"))
    return t


# =====================================================================================================================
# case tables of tests/test_gpu_train_variants.py
# =====================================================================================================================
SIDE = {16: 40, 32: 89, 64: 120}          # ragged last tile: three tiles of 16, three of 32, two of 64
SINGLE = {16: 9, 32: 23, 64: 50}          # one ragged tile
T_ONE, T_MULTI, T_FOLD = 261, 1157, 2309  # one slice of 2 + a 5-token chunk; four slices of 2, 3, 2, 3 chunks; two of 9 and 10
IMG_PLANES = ((3, 3), (6, 6), (8, 8))     # 9 pixels: element loads; 36: 16-byte in float32, 8-byte in bfloat16; 64: 16-byte
IMG_B = {(9, False): 29, (36, False): 8, (64, False): 5, (9, True): 129, (36, True): 33, (64, True): 19}
FOLD_MN = (1000, 1010)                    # 16 x 16 tiles of 64: two slices, so each walks more than kWgFold chunks

# M, N: output; T (rows) or B, hw (images); row operands: (ld, element offset past a 16-byte boundary) of A and B; images:
# element offset of both bases; `want`: the variant and epilogue the case is meant to reach
WgradCase = collections.namedtuple("WgradCase", "id dn layout M N T B hw lda offa ldb offb alpha want")


def _row_operand(width, vec, esz):
    """(row stride, base offset in elements) that gives a (T, width) row tensor the load width `vec`."""
    epl = 16 // esz
    if vec == 2:
        return _ceil(width, epl) * epl, 0
    if vec == 1:
        return _ceil(width, epl // 2) * (epl // 2), epl // 2
    return width | 1, 1


def _wgrad_case(name, dn, lay, M, N, multi, va, vb, T=None, alpha=1.0, plane=None, off=0):
    esz = ESZ[dn]
    tm, tn = wgrad_tile(M), wgrad_tile(N)
    want = (dn, lay, tm, tn, "multi" if multi else "one")
    if lay == "rows":
        (lda, offa), (ldb, offb) = _row_operand(M, va, esz), _row_operand(N, vb, esz)
        return WgradCase(name, dn, lay, M, N, T, 0, None, lda, offa, ldb, offb, alpha, want)
    hw = plane[0] * plane[1]
    B = T // hw if T else IMG_B[(hw, multi)]
    return WgradCase(name, dn, lay, M, N, B * hw, B, plane, 0, off, 0, off, alpha, want)


def _wgrad_cases():
    cases = []
    for dn, lay in itertools.product(("f32", "bf16"), ("rows", "img")):
        for (i, tm), (j, tn), multi in itertools.product(enumerate(TILES), enumerate(TILES), (False, True)):
            name = f"{dn}-{lay}-{tm}x{tn}-{'multi' if multi else 'one'}"
            if lay == "rows":       # the load widths of A and B rotate, so that every loader sees all three
                va, vb = ((i + j) % 3, (i + j + 1) % 3) if not multi else ((i + j + 2) % 3, (i + j) % 3)
                cases.append(_wgrad_case(name, dn, lay, SIDE[tm], SIDE[tn], multi, va, vb, T=T_MULTI if multi else T_ONE))
            else:                   # the plane rotates; float32 reaches 8-byte loads by an 8-byte-aligned base on 36 pixels
                plane = IMG_PLANES[(i + j + multi) % 3]
                off = 2 if (dn == "f32" and plane == (6, 6) and not multi) else 0
                cases.append(_wgrad_case(name, dn, lay, SIDE[tm], SIDE[tn], multi, 0, 0, plane=plane, off=off))
        for a, b in ((16, 32), (32, 64), (64, 16)):
            cases.append(_wgrad_case(f"{dn}-{lay}-single-{SINGLE[a]}x{SINGLE[b]}", dn, lay, SINGLE[a], SINGLE[b], False, 2, 0,
                                     T=T_ONE, plane=(3, 3)))
        cases.append(_wgrad_case(f"{dn}-{lay}-fold", dn, lay, *FOLD_MN, True, 2, 2, T=T_FOLD if lay == "rows" else 257 * 9,
                                 plane=(3, 3)))
    cases.append(_wgrad_case("f32-rows-alpha", "f32", "rows", SIDE[16], SIDE[32], False, 2, 2, T=T_ONE, alpha=-0.375))
    cases.append(_wgrad_case("bf16-img-alpha", "bf16", "img", SIDE[32], SIDE[16], True, 0, 0, alpha=-0.375, plane=(6, 6)))
    return cases


WGRAD_CASES = _wgrad_cases()


def wgrad_case_resolves(c):
    """(variant + epilogue, vec_a, vec_b, chunks per slice) of a case by the restated rules."""
    g = wgrad_geom(c.M, c.N, c.T)
    esz = ESZ[c.dn]
    if c.layout == "rows":
        va, vb = wgrad_vec(c.offa * esz, c.lda, esz), wgrad_vec(c.offb * esz, c.ldb, esz)
    else:
        hw = c.hw[0] * c.hw[1]
        va, vb = wgrad_vec(c.offa * esz, hw, esz), wgrad_vec(c.offb * esz, hw, esz)
    return (c.dn, c.layout, g.TM, g.TN, "multi" if g.slices > 1 else "one"), va, vb, slice_chunks(g)


# R2 x R1 output tiles; x (B, R1, H, W); geometry (kernel, stride, padding, dilation)
CoreWgradCase = collections.namedtuple("CoreWgradCase", "id dn R2 R1 B hw k s p dl want")
_CW_ONE = ((1, (6, 6), 3, 1, 1, 1), (2, (9, 8), 3, 2, 1, 1))           # 36 and 2 x 20 output pixels
_CW_MULTI = ((8, (8, 8), 3, 1, 1, 1), (32, (8, 8), 3, 2, 1, 1))        # B x Ho x Wo = 512: two slices of two chunks


def _core_wgrad_cases():
    cases = []
    for dn in ("f32", "bf16"):
        for (i, tm), (j, tn), multi in itertools.product(enumerate(TILES), enumerate(TILES), (False, True)):
            B, hw, k, s, p, dl = (_CW_MULTI if multi else _CW_ONE)[(i + j) % 2]
            tag = "multi" if multi else "one"
            cases.append(CoreWgradCase(f"{dn}-core-{tm}x{tn}-{tag}", dn, SIDE[tm], SIDE[tn], B, hw, k, s, p, dl, (dn, tm, tn, tag)))
        cases.append(CoreWgradCase(f"{dn}-core-5x5-dil2-64x64", dn, SINGLE[64], SINGLE[64], 2, (9, 9), 5, 1, 4, 2, (dn, 64, 64, "one")))
    return cases


CORE_WGRAD_CASES = _core_wgrad_cases()


def out_hw(hw, k, s, p, dl):
    k, s, p, dl = pair(k), pair(s), pair(p), pair(dl)
    return tuple((hw[i] + 2 * p[i] - dl[i] * (k[i] - 1) - 1) // s[i] + 1 for i in (0, 1))


def core_wgrad_case_resolves(c):
    ho, wo = out_hw(c.hw, c.k, c.s, c.p, c.dl)
    k = pair(c.k)
    g = wgrad_geom(c.R2, c.R1, c.B * ho * wo, taps=k[0] * k[1])
    return (c.dn, g.TM, g.TN, "multi" if g.slices > 1 else "one"), g


# direction "fwd": x (B, src, H, W) -> y (B, dst, Ho, Wo); "dgrad": dy (B, src, Ho, Wo) -> dx (B, dst, H, W).
# `align`: the class of the source base (2: 16-byte aligned, 1: 8-byte, 0: element)
CoreConvCase = collections.namedtuple("CoreConvCase", "id dn direction dst src B hw k s p dl align want")
_CC_GEOM = (((9, 9), 3, 1, 1, 1), ((9, 8), 3, 2, 1, 1))
CC_DST = {1: 40, 2: 100, 4: 136}          # NBW 1, 2, 4
CC_SRC = (40, 72)                         # KC = 32 (float32): two chunks, the last ragged; KC = 64 (bfloat16): one ragged, then two


def _core_conv_cases():
    cases = []
    for dn in ("f32", "bf16"):
        for (i, (nbw, dst)), (j, direction) in itertools.product(enumerate(CC_DST.items()), enumerate(("fwd", "dgrad"))):
            hw, k, s, p, dl = _CC_GEOM[(i + j) % 2]
            cases.append(CoreConvCase(f"{dn}-{direction}-nbw{nbw}", dn, direction, dst, CC_SRC[(i + j) % 2], 2, hw, k, s, p, dl,
                                      (2, 1, 0)[(i + j) % 3], (dn, nbw, direction)))
    return cases


CORE_CONV_CASES = _core_conv_cases()


def align_offset(dn, cls):
    """Element offset past a 16-byte boundary that puts a base into alignment class `cls`."""
    return {2: 0, 1: 8 // ESZ[dn], 0: 1}[cls]


# (C, O, r1, r2, (H, W), kernel, stride, padding, dilation): true ranks that are no multiple of 16, ragged C and O
ConvChainCase = collections.namedtuple("ConvChainCase", "id dn C O r1 r2 hw k s p dl")
_CO = (24, 40)
_CONV_SHAPES = {
    # the 64-pixel tile, NBW 1 / 2 / 4: a 3 x 3 and a 1 x 1 stride-2 case each
    "tm64-nbw1-3x3": (20, 28, (7, 7), 3, 1, 1, 1),
    "tm64-nbw1-1x1s2": (20, 28, (8, 8), 1, 2, 0, 1),
    "tm64-nbw2-3x3": (81, 113, (7, 7), 3, 1, 1, 1),
    "tm64-nbw2-1x1s2": (113, 81, (8, 8), 1, 2, 0, 1),
    "tm64-nbw4-3x3": (150, 20, (7, 7), 3, 1, 1, 1),
    "tm64-nbw4-1x1s2": (20, 150, (8, 8), 1, 2, 0, 1),
}
_CONV_SHAPES_32 = {
    "f32": {
        # the LDS forces the 32-pixel tile (three planes)
        "tm32-nbw1-1x1s2": (50, 60, (5, 26), 1, 2, 0, 1),
        "tm32-nbw1-3x3s2": (50, 60, (5, 26), 3, 2, 1, 1),
        "tm32-nbw1-5x5": (50, 60, (7, 19), 5, 1, 2, 1),
        "tm32-nbw2-3x3": (81, 113, (5, 13), 3, 1, 1, 1),
        "tm32-nbw2-1x1s2": (81, 113, (5, 13), 1, 2, 0, 1),
        "tm32-nbw4-3x3": (113, 150, (7, 7), 3, 1, 1, 1),
        "tm32-nbw4-1x1s2": (150, 113, (8, 8), 1, 2, 0, 1),
    },
    "bf16": {
        "tm32-nbw4-1x1s2": (250, 210, (5, 26), 1, 2, 0, 1),
        "tm32-nbw4-3x3s2": (250, 210, (5, 26), 3, 2, 1, 1),
        "tm32-nbw4-5x5": (180, 250, (7, 19), 5, 1, 2, 1),
    },
    "f16": {
        "tm32-nbw4-1x1s2": (250, 210, (5, 26), 1, 2, 0, 1),
        "tm32-nbw4-3x3s2": (250, 210, (5, 26), 3, 2, 1, 1),
    },
}


def _conv_chain_cases():
    cases = []
    for dn in ("f32", "bf16", "f16"):
        for name, shape in list(_CONV_SHAPES.items()) + list(_CONV_SHAPES_32[dn].items()):
            cases.append(ConvChainCase(f"{dn}-{name}", dn, *_CO, *shape))
    return cases


CONV_CHAIN_CASES = _conv_chain_cases()


def conv_chain_case_resolves(c, lib=False):
    """{mode: (dn, TM, NBW, mode)} the launches of a case reach (both SAVE settings of a mode run); float16: forward."""
    rule = conv_chain_variant_lib if lib else conv_chain_variant
    x_shape = (2, c.C, *c.hw)
    got = {}
    for bwd, modes in ((False, ("fwd", "fwd_save")), (True, ("bwd", "bwd_save"))):
        if c.dn == "f16" and bwd:
            continue
        v = rule(c.dn, x_shape, c.r1, c.r2, c.k, c.s, c.p, c.dl, bwd)
        if v is None:
            continue
        for m in modes:
            if c.dn == "f16" and m != "fwd":
                continue
            got[m] = (c.dn, v[0], v[1], m)
    return got


# =====================================================================================================================
# references and bounds
# =====================================================================================================================
def token_rows(t):
    """(T, features) float64 view of a row tensor or of an NCHW image with t = (batch, pixel)."""
    t = t.double()
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) if t.dim() == 4 else t


def wgrad_bound(a, b, alpha, dn):
    """(ref, bound) of C = alpha A^T B for operands of type `dn`, float64 on the operands' device."""
    a, b = token_rows(a), token_rows(b)
    T = a.shape[0]
    ref = alpha * (a.t() @ b)
    allabs = abs(alpha) * (a.abs().t() @ b.abs())
    return ref, 1.5 * (T + (5 if dn == "f32" else 1)) * ACC * allabs


def wgrad_plain32(a, b, alpha):
    """The same product by a float32 matmul of torch on the CPU."""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    if a.dim() == 4:
        a, b = a.permute(0, 2, 3, 1).reshape(-1, a.shape[1]), b.permute(0, 2, 3, 1).reshape(-1, b.shape[1])
    return (a.t() @ b) * alpha


def unfold_rows(x, k, s, p, dl):
    """x (B, R1, H, W) -> (B * Ho * Wo, R1 * kh * kw): row t holds what output pixel t reads, columns (r1, ky, kx)."""
    cols = F.unfold(x, pair(k), pair(dl), pair(p), pair(s))
    return cols.permute(0, 2, 1).reshape(-1, cols.shape[1])


def core_wgrad_bound(dy, x, k, s, p, dl, dn):
    """(ref, bound) of dWc (R2, R1, kh, kw): the weight-gradient product of dY's rows with the unfolded X."""
    k = pair(k)
    ref, bound = wgrad_bound(token_rows(dy), unfold_rows(x.double(), k, s, p, dl), 1.0, dn)
    shape = (dy.shape[1], x.shape[1], *k)
    return ref.reshape(shape), bound.reshape(shape)


def core_wgrad_plain32(dy, x, k, s, p, dl):
    dy, x = dy.detach().cpu().float(), x.detach().cpu().float()
    a = dy.permute(0, 2, 3, 1).reshape(-1, dy.shape[1])
    return (a.t() @ unfold_rows(x, k, s, p, dl)).reshape(dy.shape[1], x.shape[1], *pair(k))


def _conv_t(t, w, x_hw, s, p, dl):
    """conv^T: (B, R2, Ho, Wo) -> (B, R1, H, W) with the core w (R2, R1, kh, kw)."""
    s, p, dl = pair(s), pair(p), pair(dl)
    opad = tuple(x_hw[i] - ((t.shape[2 + i] - 1) * s[i] - 2 * p[i] + dl[i] * (w.shape[2 + i] - 1) + 1) for i in (0, 1))
    return F.conv_transpose2d(t, w, None, s, p, opad, 1, dl)


def chain_steps(w1, core, w3, x_hw, s, p, dl):
    """(forward steps, data-gradient steps) of 1x1 -> k x k -> 1x1: lists of (f(t, w), w, accumulated terms per output)."""
    one = lambda t, w: F.conv2d(t, w[:, :, None, None])                       # noqa: E731
    taps = core.shape[2] * core.shape[3]
    fwd = [(one, w1, w1.shape[1]), (lambda t, w: F.conv2d(t, w, None, pair(s), pair(p), pair(dl)), core, core.shape[1] * taps),
           (one, w3, w3.shape[1])]
    bwd = [(one, w3.t(), w3.shape[0]), (lambda t, w: _conv_t(t, w, x_hw, s, p, dl), core, core.shape[0] * taps),
           (one, w1.t(), w1.shape[0])]
    return fwd, bwd


def prefix_bounds(x, steps, dn, bias=None):
    """[(ref, bound)] of every prefix of a chain of linear steps on x, float64, in the form of the module docstring."""
    h = x.double()
    allabs, mids, n, out = h.abs(), [], 0, []
    for i, (f, w, terms) in enumerate(steps):
        w = w.double()
        h, allabs, mids = f(h, w), f(allabs, w.abs()), [f(m, w.abs()) for m in mids]
        n += terms
        if bias is not None and i + 1 == len(steps):
            b = bias.double().view(1, -1, 1, 1) if h.dim() == 4 else bias.double()
            h, allabs = h + b, allabs + b.abs()
        if dn == "f32":
            bound = 1.5 * (n + 1 + 2 * (i + 1)) * ACC * allabs
        else:
            bound = 1.5 * (U[DTYPES[dn]] * (h.abs() + sum(mids)) + n * ACC * allabs)
        out.append((h, bound))
        mids.append(h.abs())
    return out


def prefix_plain32(x, steps, bias=None):
    """The same prefixes in float32 by torch on the CPU."""
    h, out = x.detach().cpu().float(), []
    for i, (f, w, _) in enumerate(steps):
        h = f(h, w.detach().cpu().float())
        if bias is not None and i + 1 == len(steps):
            h = h + (bias.detach().cpu().float().view(1, -1, 1, 1) if h.dim() == 4 else bias.detach().cpu().float())
        out.append(h)
    return out


def core_conv_steps(core, direction, x_hw, s, p, dl):
    taps = core.shape[2] * core.shape[3]
    if direction == "fwd":
        return [(lambda t, w: F.conv2d(t, w, None, pair(s), pair(p), pair(dl)), core, core.shape[1] * taps)]
    return [(lambda t, w: _conv_t(t, w, x_hw, s, p, dl), core, core.shape[0] * taps)]


def reached(x_hw, k, s, p, dl, device="cpu"):
    """(H, W) bool: the input pixels some tap of some output pixel reads."""
    k = pair(k)
    ho, wo = out_hw(x_hw, k, s, p, dl)
    ones = torch.ones(1, 1, ho, wo, dtype=torch.float64, device=device)
    return _conv_t(ones, torch.ones(1, 1, *k, dtype=torch.float64, device=device), x_hw, s, p, dl)[0, 0] != 0


# =====================================================================================================================
# the judge
# =====================================================================================================================
FIGURES = collections.defaultdict(lambda: [0.0, 0.0])       # family-dtype -> [worst err / bound, worst rms ratio]


def rms_ratio(got, ref, plain):
    rms = lambda t: (t.detach().to(ref.device).double() - ref).pow(2).mean().sqrt().item()       # noqa: E731
    num, den = rms(got), rms(plain)
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def judge(name, got, ref, bound, plain=None, family=None):
    """Prints the figures, then asserts |got - ref| <= bound elementwise (exact where the bound is zero) and, with
    `plain`, rms(got - ref) <= 2 rms(plain - ref).  Returns (worst err / bound, rms ratio or None)."""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got.detach().to(ref.device).double() - ref).abs()
    pos = bound > 0
    worst = (err[pos] / bound[pos]).max().item() if bool(pos.any()) else 0.0
    ratio = None if plain is None else rms_ratio(got, ref, plain)
    print(f"train {name}: worst err / bound {worst:.4f}" + ("" if ratio is None else f", rms ratio {ratio:.3f}"))
    if family is not None:
        FIGURES[family][0] = max(FIGURES[family][0], worst)
        FIGURES[family][1] = max(FIGURES[family][1], ratio or 0.0)
    assert bool(torch.isfinite(got.float()).all()), name
    assert bool((err <= bound).all()), (name, worst)
    if ratio is not None:
        assert ratio <= 2.0, (name, ratio)
    return worst, ratio
