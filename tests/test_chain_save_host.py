"""Host side of the saving launches of the fused chains: the binding lists the four entries, and the routing rule
`ops.chain_train_pays` is a pure function of its arguments.  No GPU: the tensors are CPU tensors or meta tensors."""
import ctypes as C

import torch

SAVE_ENTRIES = ("tadmm_ttlinear_fwd_save", "tadmm_ttlinear_bwd_save", "tadmm_svdconv_fwd_save", "tadmm_svdconv_bwd_save")


def test_cabi_lists_the_four_entries():
    from tadmm import _cabi
    for name in SAVE_ENTRIES:
        res, args = _cabi.ABI[name]
        assert res is C.c_int
        # handle, descriptor, true rank, h_out, ldh, stream
        assert args == [C.c_void_p, C.POINTER(_cabi.ChainDesc), C.c_int, C.c_void_p, C.c_int64, C.c_void_p], name
    lib = _cabi.load()                       # raises when the built library lacks one of them
    for name in SAVE_ENTRIES:
        assert hasattr(lib, name)


def test_header_declares_the_four_entries():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "tadmm.h")).read()
    for name in SAVE_ENTRIES:
        assert f"int {name}(tadmm_handle h, const tadmm_chain_desc* d, int r, void* " in text, name


def _cases():
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        for shape, image in (((12608, 384), False), ((70, 40), False), ((128, 24, 16, 16), True), ((2, 40, 7, 7), True)):
            for r in (1, 20, 64, 200, 256, 257, 512):
                for n_out in (24, 1152):
                    yield dtype, shape, image, r, n_out


def test_chain_train_pays_is_a_pure_function_of_its_arguments():
    from tadmm import ops
    for dtype, shape, image, r, n_out in _cases():
        x = torch.empty(shape, dtype=dtype, device="meta")
        n_in = shape[1]
        first = ops.chain_train_pays(x, r, n_in, n_out, image)
        assert isinstance(first, bool)
        # the same arguments, whatever happened in between and whatever the tensor holds or wants
        with torch.no_grad():
            assert ops.chain_train_pays(x, r, n_in, n_out, image) is first
        y = torch.zeros(shape, dtype=dtype).requires_grad_()
        assert ops.chain_train_pays(y, r, n_in, n_out, image) is first
        assert ops.chain_train_pays(y.detach() + 1, r, n_in, n_out, image) is first


def test_chain_train_pays_refuses_what_the_entries_refuse():
    from tadmm import ops
    for dtype, shape, image, r, n_out in _cases():
        x = torch.empty(shape, dtype=dtype, device="meta")
        pays = ops.chain_train_pays(x, r, shape[1], n_out, image)
        if dtype == torch.float16 or r > 256:
            assert pays is False, (dtype, r)
        # nothing wants a factor gradient: nothing to save, whatever the shape
        assert ops.chain_train_pays(x, r, shape[1], n_out, image, factor_grad=False) is False
    assert ops.chain_train_pays(torch.empty(70, 40, dtype=torch.float64, device="meta"), 20, 40, 24, False) is False
    assert ops.chain_train_pays(torch.empty(70, 40, device="meta"), 0, 40, 24, False) is False
