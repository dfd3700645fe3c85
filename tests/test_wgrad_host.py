"""Weight-gradient kernel (csrc/wgrad.hip) without a device: the C ABI surface, the descriptor layout, and the slice
rule as a pure host function of the descriptor."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tadmm_wgrad_desc_bytes", "tadmm_wgrad_workspace_bytes", "tadmm_wgrad")


def desc(M=18, N=24, T=131072, hw=1024, dtype=0, A=4096, B=8192, lda=0, ldb=0):
    from tadmm import _cabi
    d = _cabi.WgradDesc()
    d.A, d.B, d.C, d.T, d.M, d.N, d.hw, d.dtype, d.alpha = A, B, 16384, T, M, N, hw, dtype, 1.0
    d.lda, d.ldb, d.ldc = (lda or M, ldb or N, N) if hw == 0 else (0, 0, N)
    return d


def plan(d):
    from tadmm import _cabi
    nbytes, slices = C.c_size_t(12345), C.c_int(-7)
    rc = _cabi.load().tadmm_wgrad_workspace_bytes(C.byref(d), C.byref(nbytes), C.byref(slices))
    return rc, nbytes.value, slices.value


def test_header_declares_the_symbols_and_the_struct():
    text = open(os.path.join(ROOT, "include", "tadmm.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"}\s*tadmm_wgrad_desc\s*;", text)
    struct = text[:text.index("} tadmm_wgrad_desc;")]
    struct = struct[struct.rindex("typedef struct"):]
    for field in ("A", "B", "C", "T", "M", "N", "lda", "ldb", "ldc", "hw", "dtype", "alpha"):
        assert re.search(r"\b%s\b" % field, struct), field


def test_cabi_table_lists_them_and_the_library_exports_them():
    from tadmm import _cabi
    lib = _cabi.load()
    for name in SYMBOLS:
        assert name in _cabi.ABI
        assert hasattr(lib, name)


def test_desc_bytes_equals_ctypes_size():
    from tadmm import _cabi
    assert _cabi.load().tadmm_wgrad_desc_bytes() == C.sizeof(_cabi.WgradDesc)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hw", [0, 196])
def test_workspace_bytes_is_a_pure_function(dtype, hw):
    first = plan(desc(T=12544 * 8, hw=hw, dtype=dtype))
    assert first[0] == 0 and first[2] >= 1
    assert plan(desc(T=12544 * 8, hw=hw, dtype=dtype)) == first
    # operand addresses do not enter
    assert plan(desc(T=12544 * 8, hw=hw, dtype=dtype, A=1 << 20, B=1 << 21)) == first


def test_one_slice_needs_no_workspace_and_many_need_some():
    rc, nbytes, slices = plan(desc(T=31, hw=0))
    assert (rc, nbytes, slices) == (0, 0, 1)
    rc, nbytes, slices = plan(desc(M=18, N=24, T=131072, hw=1024))
    assert rc == 0 and slices > 1
    assert nbytes >= slices * 18 * 24 * 4
    rc, nbytes, slices = plan(desc(T=0, hw=0))
    assert (rc, nbytes, slices) == (0, 0, 1)


@pytest.mark.parametrize("mn", [(1, 1), (18, 24), (64, 65), (256, 2048), (300, 10)])
def test_slices_monotone_in_t(mn):
    prev = 0
    ts = sorted(set(list(range(0, 4100, 37)) + [2 ** k + o for k in range(8, 22) for o in (-1, 0, 1)]
                    + [12608, 131072, 200704]))
    for t in ts:
        rc, nbytes, slices = plan(desc(M=mn[0], N=mn[1], T=t, hw=0))
        assert rc == 0 and slices >= 1
        assert slices >= prev, (mn, t, slices, prev)
        assert (nbytes == 0) == (slices == 1)
        prev = slices


def test_invalid_descriptors():
    assert plan(desc(M=0))[0] == -1
    assert plan(desc(M=-3))[0] == -1
    assert plan(desc(N=0))[0] == -1
    assert plan(desc(T=-1, hw=0))[0] == -1
    assert plan(desc(dtype=2))[0] == -1
    assert plan(desc(A=0))[0] == -1                      # null operand with T > 0
    assert plan(desc(B=0))[0] == -1
    assert plan(desc(A=0, B=0, T=0, hw=0))[0] == 0       # nothing is read when T == 0
    assert plan(desc(T=1000, hw=196))[0] == -1           # not whole images
    assert plan(desc(M=18, T=512, hw=0, lda=17))[0] == -1
    from tadmm import _cabi
    assert _cabi.load().tadmm_wgrad_workspace_bytes(None, C.byref(C.c_size_t()), None) == -1
    assert _cabi.load().tadmm_wgrad_workspace_bytes(C.byref(desc()), None, None) == -1


def test_sizes_the_launch_cannot_take_are_unsupported():
    assert plan(desc(M=1, N=1, T=2 ** 31, hw=0))[0] == -5
    assert plan(desc(M=2 ** 20, N=2 ** 20, T=512, hw=0))[0] == -5


def test_ops_refuses_host_tensors_without_a_device():
    import torch
    from tadmm import ops
    from tadmm._cabi import TadmmError
    with pytest.raises(TadmmError, match="no CPU path"):
        ops.wgrad(torch.zeros(8, 4), torch.zeros(8, 3))


def test_no_channel_major_copy_left_in_backward():
    src = open(os.path.join(ROOT, "dnn-compression-tensor-admm_amd", "tadmm", "functional.py")).read()
    assert "_channel_major" not in src
    assert not re.search(r"permute\([^)]*\)\.reshape\([^)]*\)\.float\(\)", src)
