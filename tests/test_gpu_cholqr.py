"""GPU tests of the Cholesky QR kernels (csrc/chol.hip): the factor's step loop with its look-ahead hand-over and
the strip-per-workgroup forward substitution, against numpy Householder QR, on the shapes at which their tile and
wave arithmetic changes, on a row-strided image, on blocks that break down in every part of the step loop, and for
run-to-run reproducibility."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (n, ncols, cond): two steps only / fewer tiles than slots, ncols no multiple of 128 / the block size of the critical
# chain / nbt = 14, odd against 7 tile waves and 4 solve waves / every accumulator slot in use
SHAPES = [(32, 64, 1e2), (96, 192, 1e2), (160, 448, 1e3), (224, 448, 1e3), (256, 512, 10.0)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _block(n, ncols, cond):
    """ncols x n block with condition number `cond`: orthonormal factors times a log-spaced spectrum"""
    rng = np.random.default_rng(n + ncols)
    q1, _ = np.linalg.qr(rng.standard_normal((ncols, n)))
    q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.exp(np.linspace(0.0, -np.log(cond), n))
    return (q1 * s) @ q2.T


_REF = {}


def _reference(n, ncols, cond):
    """(block, Q of its Householder QR with the diagonal of R made positive), computed once per shape"""
    key = (n, ncols, cond)
    if key not in _REF:
        y = _block(n, ncols, cond)
        q, r = np.linalg.qr(y)
        q = q * np.sign(np.diag(r))
        y.setflags(write=False)
        q.setflags(write=False)
        _REF[key] = (y, q)
    return _REF[key]


def _cholqr_view(view):
    """tadmm_cholqr_f64 on a row-strided (n, ncols) view; ops.cholqr_ takes contiguous images only"""
    from tadmm import ops
    n, ncols = view.shape
    assert view.stride(1) == 1
    h = ops.Handle.get(view.device.index)
    sb = h.lib.tadmm_cholqr_scratch_bytes(n, ncols)
    scratch = torch.empty(sb, dtype=torch.uint8, device=view.device)
    bad = C.c_int(0)
    h.check(h.lib.tadmm_cholqr_f64(h.ptr, view.data_ptr(), n, ncols, view.stride(0), scratch.data_ptr(), sb,
                                   C.byref(bad), torch.cuda.current_stream(view.device).cuda_stream))
    return bad.value == 0


def _check_q(q, q_ref, n, cond):
    bound = 1e-13 * cond * cond + 1e-12           # one pass: ~cond^2 * eps
    err_q = np.abs(q - q_ref).max()
    err_o = np.abs(q.T @ q - np.eye(n)).max()
    print(f"n={n} cond={cond:g}: max|Q-Qref|={err_q:.3e} max|QtQ-I|={err_o:.3e} bound={bound:.3e}")
    assert err_q <= bound, err_q
    assert err_o <= bound, err_o


@pytest.mark.parametrize("n,ncols,cond", SHAPES)
def test_cholqr_matches_householder_qr(dev, n, ncols, cond):
    from tadmm import ops
    y, q_ref = _reference(n, ncols, cond)
    yt = torch.from_numpy(np.ascontiguousarray(y.T)).to(dev)
    assert ops.cholqr_(yt)
    _check_q(yt.cpu().numpy().T, q_ref, n, cond)


def test_cholqr_on_a_row_strided_image_leaves_the_padding_alone(dev):
    n, ncols, cond = 96, 192, 1e2
    y, q_ref = _reference(n, ncols, cond)
    rng = np.random.default_rng(7)
    big = rng.standard_normal((n, ncols + 64))
    big[:, :ncols] = y.T
    img = torch.from_numpy(big).to(dev)
    assert _cholqr_view(img[:, :ncols])
    out = img.cpu().numpy()
    assert np.array_equal(out[:, ncols:], big[:, ncols:])
    _check_q(out[:, :ncols].T, q_ref, n, cond)


def _deficient(kind):
    rng = np.random.default_rng(11)
    n, ncols = 96, 192
    if kind == "first tile":                      # column 1 a copy of column 0
        y = rng.standard_normal((ncols, n))
        y[:, 1] = y[:, 0]
    elif kind == "middle tile":                   # rank 40 of 96: the pivot breaks down in tile 2
        y = rng.standard_normal((ncols, 40)) @ rng.standard_normal((40, n))
    elif kind == "last tile":                     # rank 90 of 96: tile 5
        y = rng.standard_normal((ncols, 90)) @ rng.standard_normal((90, n))
    else:                                         # a single NaN
        y = rng.standard_normal((ncols, n))
        y[100, 50] = np.nan
    return np.ascontiguousarray(y.T)


@pytest.mark.parametrize("kind", ["first tile", "middle tile", "last tile", "nan"])
def test_cholqr_breakdown_returns_false_and_keeps_the_image(dev, kind):
    from tadmm import ops
    src = _deficient(kind)
    yt = torch.from_numpy(src).to(dev)
    assert not ops.cholqr_(yt)
    torch.cuda.synchronize()
    assert np.array_equal(yt.cpu().numpy(), src, equal_nan=True)     # the solve is skipped: the image is untouched


def test_cholqr_is_bitwise_reproducible(dev):
    from tadmm import ops
    n, ncols, cond = 160, 448, 1e3
    y, _ = _reference(n, ncols, cond)
    runs = []
    for _ in range(2):
        yt = torch.from_numpy(np.ascontiguousarray(y.T)).to(dev)
        assert ops.cholqr_(yt)
        runs.append(yt.cpu().numpy())
    assert np.array_equal(runs[0], runs[1])
