"""Core-convolution kernels (csrc/coreconv.hip, csrc/wgrad.hip) without a device: the C ABI surface, the descriptor
layout, the weight gradient's slice rule as a pure host function, refusals, and the host-only shape logic of ops."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tadmm_core_conv_desc_bytes", "tadmm_core_conv_fwd", "tadmm_core_conv_dgrad",
           "tadmm_core_conv_wgrad_workspace_bytes", "tadmm_core_conv_wgrad")


def desc(B=4, R1=16, R2=24, H=32, W=32, k=(3, 3), s=(1, 1), p=(1, 1), dl=(1, 1), dtype=0, X=4096, Y=8192, out=None):
    from tadmm import _cabi
    d = _cabi.CoreConvDesc()
    d.X, d.Y, d.B, d.R1, d.R2, d.H, d.W, d.dtype = X, Y, B, R1, R2, H, W, dtype
    d.kh, d.kw, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = k + s + p + dl
    ho = (H + 2 * p[0] - dl[0] * (k[0] - 1) - 1) // s[0] + 1 if s[0] > 0 else 0
    wo = (W + 2 * p[1] - dl[1] * (k[1] - 1) - 1) // s[1] + 1 if s[1] > 0 else 0
    d.Ho, d.Wo = out if out is not None else (ho, wo)
    return d


def plan(d):
    from tadmm import _cabi
    nbytes, slices = C.c_size_t(12345), C.c_int(-7)
    rc = _cabi.load().tadmm_core_conv_wgrad_workspace_bytes(C.byref(d), C.byref(nbytes), C.byref(slices))
    return rc, nbytes.value, slices.value


def test_header_declares_the_symbols_and_the_struct():
    text = open(os.path.join(ROOT, "include", "tadmm.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"}\s*tadmm_core_conv_desc\s*;", text)
    struct = text[:text.index("} tadmm_core_conv_desc;")]
    struct = struct[struct.rindex("typedef struct"):]
    for field in ("X", "Y", "Wc", "wc_plane", "B", "R1", "R2", "H", "W", "Ho", "Wo", "kh", "kw", "stride_h", "stride_w",
                  "pad_h", "pad_w", "dil_h", "dil_w", "dtype"):
        assert re.search(r"\b%s\b" % field, struct), field


def test_cabi_table_lists_them_and_the_library_exports_them():
    from tadmm import _cabi
    lib = _cabi.load()
    for name in SYMBOLS:
        assert name in _cabi.ABI
        assert hasattr(lib, name)


def test_desc_bytes_equals_ctypes_size():
    from tadmm import _cabi
    assert _cabi.load().tadmm_core_conv_desc_bytes() == C.sizeof(_cabi.CoreConvDesc)


@pytest.mark.parametrize("dtype", [0, 1])
def test_workspace_bytes_is_a_pure_function(dtype):
    first = plan(desc(dtype=dtype))
    assert first[0] == 0 and first[2] >= 1
    assert plan(desc(dtype=dtype)) == first
    assert plan(desc(dtype=dtype, X=1 << 20, Y=1 << 21)) == first       # operand addresses do not enter


def test_one_slice_needs_no_workspace_and_many_need_some():
    assert plan(desc(B=1, H=6, W=6)) == (0, 0, 1)                        # 36 output pixels: one slice
    rc, nbytes, slices = plan(desc(B=4, R1=1, R2=1, H=32, W=32))         # 4096 output pixels
    assert rc == 0 and slices > 1
    assert nbytes >= 9 * slices * 4
    assert plan(desc(B=0)) == (0, 0, 1)


def test_invalid_descriptors_are_refused_without_a_device():
    assert plan(desc(R1=0))[0] == -1
    assert plan(desc(R2=-3))[0] == -1
    assert plan(desc(H=0))[0] == -1
    assert plan(desc(B=-1))[0] == -1
    assert plan(desc(k=(0, 3)))[0] == -1
    assert plan(desc(s=(0, 1), out=(32, 32)))[0] == -1
    assert plan(desc(dl=(1, 0)))[0] == -1
    assert plan(desc(p=(-1, 1)))[0] == -1
    assert plan(desc(dtype=2))[0] == -1
    assert plan(desc(H=2, W=2, k=(5, 5), p=(0, 0)))[0] == -1             # empty output plane
    assert plan(desc(out=(31, 32)))[0] == -1                             # not the geometry's output size
    assert plan(desc(X=0))[0] == -1                                      # null operand with work to do
    assert plan(desc(Y=0))[0] == -1
    assert plan(desc(X=0, Y=0, B=0))[0] == 0                             # nothing is read when B == 0
    from tadmm import _cabi
    lib = _cabi.load()
    assert lib.tadmm_core_conv_wgrad_workspace_bytes(None, C.byref(C.c_size_t()), None) == -1
    assert lib.tadmm_core_conv_wgrad_workspace_bytes(C.byref(desc()), None, None) == -1
    # the launching entries refuse a null handle before anything else
    assert lib.tadmm_core_conv_fwd(None, C.byref(desc()), None) == -1
    assert lib.tadmm_core_conv_dgrad(None, C.byref(desc()), None) == -1
    assert lib.tadmm_core_conv_wgrad(None, C.byref(desc()), None, None, 0, None) == -1


def test_sizes_the_launch_cannot_take_are_unsupported():
    assert plan(desc(B=2 ** 20, R1=1, R2=1, H=64, W=64))[0] == -5        # 2^32 output pixels in the batch
    assert plan(desc(H=80, W=80, k=(70, 70), p=(0, 0)))[0] == -5         # 4900 taps


def test_fits_is_pure_host_logic():
    import torch
    from tadmm import ops
    x = torch.zeros(1, 8, 112, 112)
    assert ops.core_conv_fits(x, 8, (3, 3), (1, 1), (1, 1), (1, 1))                      # a 112-wide plane
    assert ops.core_conv_fits(torch.zeros(1, 300, 7, 7), 300, (3, 3), (1, 1), (1, 1), (1, 1))   # rank 300
    assert ops.core_conv_fits(x.bfloat16(), 8, (3, 3), (2, 2), (1, 1), (1, 1))
    assert not ops.core_conv_fits(x.double(), 8, (3, 3), (1, 1), (1, 1), (1, 1))
    assert not ops.core_conv_fits(x, 8, (3, 3), (1, 1), (1, 1), (1, 1), groups=2)
    assert not ops.core_conv_fits(torch.zeros(1, 8, 2, 2), 8, (5, 5), (1, 1), (0, 0), (1, 1))   # empty output plane
    assert not ops.core_conv_fits(torch.zeros(8, 112, 112), 8, (3, 3), (1, 1), (1, 1), (1, 1))
    # what does not fit never pays
    assert not ops.core_conv_pays(x.double(), 8, (3, 3), (1, 1), (1, 1), (1, 1))
    assert not ops.core_conv_pays(x, 8, (3, 3), (1, 1), (1, 1), (1, 1), groups=2, training=True)


def test_ops_refuse_host_tensors_without_a_device():
    import torch
    from tadmm import ops
    from tadmm._cabi import TadmmError
    planes = torch.zeros(3, 2, 9, 64, 8, dtype=torch.bfloat16)
    with pytest.raises(TadmmError, match="no CPU path"):
        ops.core_conv(torch.zeros(1, 8, 6, 6), planes, 8, (3, 3), 1, 1, 1)
    with pytest.raises(TadmmError, match="no CPU path"):
        ops.core_conv_dgrad(torch.zeros(1, 8, 6, 6), planes, (1, 8, 6, 6), (3, 3), 1, 1, 1)
    with pytest.raises(TadmmError, match="no CPU path"):
        ops.core_conv_wgrad(torch.zeros(1, 8, 6, 6), torch.zeros(1, 8, 6, 6), (3, 3), 1, 1, 1)
