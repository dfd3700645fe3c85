"""Strided fp32 GEMM (csrc/gemm.hip: by-value and grouped entry) and bf16 NT GEMM (csrc/gemm_bf16.hip) on the
arguments and operand layouts no other test passes: beta, sub-block views of larger buffers (row stride > extent, base
pointer off the 16-byte grid), the grouped `ops.GemmBatch`, refused descriptors, long K, and bf16 views whose K tail
falls inside a 16-byte load.

fp32 bar, per element, against fp64:  err <= tol * scale,
    scale = |alpha| * (|A| @ |B|) + |bias_n| + |bias_m| + |beta * C0|
    tol = 4e-7 for K <= 480 (the bar of tests/test_gpu_kernels.py::test_gemm_strided);
    tol = (64 + K / 64 + 4) * 2^-24 for long K: gemm.hip accumulates chunks of 64 products in one fp32 accumulator and
    adds the K / 64 chunk sums in a second one; 4 roundings for the epilogue.
Neither number comes from what the kernel returns.

Measured on MI355X, worst err / scale of the (70, 90, K) products: chunked (the product path) 7.9e-7 at K = 4608 and
1.6e-6 at K = 12608 for constant operands, 2.5e-8 for Gaussian and rank-1 ones; with TADMM_GEMM_PLAIN=1 (one fp32
accumulator over all of K; the child run of this file, an A/B switch, nothing asserted) 2.9e-5 / 3.6e-5 for constant
operands, 1.9e-7 for Gaussian ones."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_SHORT = 4e-7
ERR_INVALID, ERR_WORKSPACE = -1, -2
CSENT = -4321.5                  # sentinel of output buffers


def tol_long(K):
    return (64 + K / 64 + 4) * 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _ref_and_scale(a, b, alpha, beta, c0, bn, bm):
    """fp64 reference and per-element error scale of C = alpha a b + beta c0 + bias_n + bias_m (host tensors)."""
    a, b = a.double(), b.double()
    ref = alpha * (a @ b)
    scale = abs(alpha) * (a.abs() @ b.abs())
    if beta != 0.0:
        ref = ref + beta * c0.double()
        scale = scale + (beta * c0.double()).abs()
    if bn is not None:
        ref = ref + bn.double()[None, :]
        scale = scale + bn.double().abs()[None, :]
    if bm is not None:
        ref = ref + bm.double()[:, None]
        scale = scale + bm.double().abs()[:, None]
    return ref, scale


def _assert_close(got, ref, scale, tol, what):
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all(), what
    ratio = float((err / scale.clamp_min(1e-300)).max())
    bad = err > tol * scale
    if bool(bad.any()):
        i, j = [int(x) for x in bad.nonzero()[0]]
        raise AssertionError(f"{what}: element ({i}, {j}) err {float(err[i, j]):.3e} > {tol:.3e} * scale "
                             f"{float(scale[i, j]):.3e} (tile {i // 64}, {j // 64}); worst err / scale {ratio:.3e}")
    return ratio


def _strided(host2d, dev, trans, pad=0, off=0, fill=float("nan")):
    """Device view equal to `host2d` (rows x cols) cut out of a larger `fill`-filled flat buffer: row stride =
    extent + pad, first element `off` elements into the buffer; `trans`: stored column-major (unit ROW stride).
    Returns (view, buffer, bool mask of the buffer elements that belong to the view)."""
    src = host2d.t() if trans else host2d
    rows, cols = src.shape
    ld = cols + pad
    buf = torch.full((off + rows * ld + 4,), fill, dtype=torch.float32, device=dev)
    mask = torch.zeros(buf.shape, dtype=torch.bool, device=dev)
    v = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    mask[off:off + rows * ld].view(rows, ld)[:, :cols] = True
    v.copy_(src)
    return (v.t() if trans else v), buf, mask


# ---------------------------------------------------------------------------------------------- B1
@pytest.mark.parametrize("M,N,K", [(130, 33, 77), (64, 64, 16), (1, 5, 3), (257, 129, 65)])
@pytest.mark.parametrize("tc", [0, 1], ids=["Crow", "Ccol"])
def test_gemm_beta_and_biases(dev, M, N, K, tc):
    from tadmm import ops
    a, b = _randn((M, K), 1), _randn((K, N), 2)
    c0, bn, bm = _randn((M, N), 3), _randn((N,), 4), _randn((M,), 5)
    ad, bd, bnd, bmd = a.to(dev), b.to(dev), bn.to(dev), bm.to(dev)
    worst = 0.0
    for beta in (1.0, -0.5):
        for alpha in (1.0, 0.25):
            for use_n, use_m in ((1, 1), (1, 0), (0, 1), (0, 0)):
                cv, _, _ = _strided(c0, dev, tc)
                ops.mm(ad, bd, out=cv, alpha=alpha, beta=beta, bias_n=bnd if use_n else None,
                       bias_m=bmd if use_m else None)
                ref, scale = _ref_and_scale(a, b, alpha, beta, c0, bn if use_n else None, bm if use_m else None)
                worst = max(worst, _assert_close(cv.cpu(), ref, scale, TOL_SHORT,
                                                 f"beta {beta} alpha {alpha} bias_n {use_n} bias_m {use_m}"))
    print(f"({M}, {N}, {K}) tc {tc}: worst err / scale {worst:.3e} (bar {TOL_SHORT:.1e})")
    # beta == 0: C is write-only -- a NaN-filled output must come back finite
    nan = torch.full((M, N), float("nan"))
    cv, _, _ = _strided(nan, dev, tc)
    ops.mm(ad, bd, out=cv, alpha=0.25, beta=0.0, bias_n=bnd)
    ref, scale = _ref_and_scale(a, b, 0.25, 0.0, None, bn, None)
    _assert_close(cv.cpu(), ref, scale, TOL_SHORT, "beta 0 over NaN")


# ---------------------------------------------------------------------------------------------- B2
@pytest.mark.parametrize("M,N,K", [(75, 70, 37), (64, 64, 64), (3, 200, 5)])
@pytest.mark.parametrize("ta,tb,tc", [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)])
def test_gemm_on_views_of_larger_buffers(dev, M, N, K, ta, tb, tc):
    """Everything around A and B is NaN (a load outside the view poisons the result), everything around C a sentinel
    that must survive."""
    from tadmm import ops
    a, b = _randn((M, K), 11), _randn((K, N), 12)
    ref, scale = _ref_and_scale(a, b, 1.0, 0.0, None, None, None)
    worst = 0.0
    for pad in (1, 3, 4):
        for off in (0, 1, 3):
            av, _, _ = _strided(a, dev, ta, pad, off)
            bv, _, _ = _strided(b, dev, tb, pad, off)
            cv, cbuf, cmask = _strided(torch.full((M, N), CSENT), dev, tc, pad, off, fill=CSENT)
            assert max(av.stride()) == (M if ta else K) + pad and av.data_ptr() % 16 == (4 * off) % 16
            ops.mm(av, bv, out=cv)
            worst = max(worst, _assert_close(cv.cpu(), ref, scale, TOL_SHORT, f"pad {pad} off {off}"))
            assert bool((cbuf[~cmask] == CSENT).all()), f"pad {pad} off {off}: store outside the C view"
    print(f"({M}, {N}, {K}) t {ta}{tb}{tc}: worst err / scale {worst:.3e} (bar {TOL_SHORT:.1e})")


# ---------------------------------------------------------------------------------------------- B3
def _group(dev):
    """>= 6 problems of mixed shape, layout, beta and biases; every C its own tensor.  Returns a list of dicts with the
    host operands, the device views (kept alive) and the descriptor."""
    from tadmm import ops
    specs = [  # M, N, K, ta, tb, tc, alpha, beta, bias_n, bias_m
        (1, 1, 1, 0, 0, 0, 1.0, 0.0, 0, 0),
        (300, 200, 50, 0, 0, 0, 1.0, 0.0, 1, 0),
        (75, 70, 37, 1, 0, 1, 0.5, 1.0, 0, 1),
        (64, 64, 64, 0, 1, 0, 1.0, -0.5, 1, 1),
        (3, 200, 5, 1, 1, 0, 2.0, 0.0, 0, 0),
        (130, 33, 77, 0, 0, 1, 1.0, 0.0, 1, 1),
        (257, 129, 65, 1, 1, 1, 0.25, 1.0, 0, 0),
    ]
    out = []
    for i, (M, N, K, ta, tb, tc, alpha, beta, un, um) in enumerate(specs):
        p = dict(M=M, N=N, K=K, alpha=alpha, beta=beta, a=_randn((M, K), 100 + i), b=_randn((K, N), 200 + i),
                 c0=_randn((M, N), 300 + i), bn=_randn((N,), 400 + i) if un else None,
                 bm=_randn((M,), 500 + i) if um else None)
        p["av"], p["bv"] = _strided(p["a"], dev, ta)[0], _strided(p["b"], dev, tb)[0]
        p["cv"] = _strided(p["c0"], dev, tc)[0]
        p["bnd"] = None if p["bn"] is None else p["bn"].to(dev)
        p["bmd"] = None if p["bm"] is None else p["bm"].to(dev)
        p["desc"] = ops.gemm_desc(p["av"].data_ptr(), p["bv"].data_ptr(), p["cv"].data_ptr(), M, N, K, p["av"].stride(),
                                  p["bv"].stride(), p["cv"].stride(), alpha, beta,
                                  None if un == 0 else p["bnd"].data_ptr(), None if um == 0 else p["bmd"].data_ptr())
        out.append(p)
    return out


def test_grouped_gemm_matches_reference_and_the_by_value_entry(dev):
    from tadmm import ops
    from tadmm._cabi import GemmDesc
    probs = _group(dev)
    descs = [p["desc"] for p in probs]
    n = len(descs)
    h = ops.Handle.get(dev.index)
    # pack contract (host only): block count, and a blob one byte short
    arr = (GemmDesc * n)(*descs)
    nbytes = h.lib.tadmm_gemm_pack_bytes(n, arr)
    want_blocks = sum(-(-p["M"] // 64) * -(-p["N"] // 64) for p in probs)
    blob = (C.c_char * nbytes)()
    nb = C.c_int(-7)
    assert h.lib.tadmm_gemm_pack(n, arr, blob, nbytes - 1, C.byref(nb)) == ERR_WORKSPACE
    assert h.lib.tadmm_gemm_pack(n, arr, blob, nbytes, C.byref(nb)) == 0 and nb.value == want_blocks

    batch = ops.GemmBatch(descs, dev)
    assert batch.nblocks == want_blocks
    batch.run()
    torch.cuda.synchronize()
    first = [p["cv"].clone() for p in probs]
    for i, p in enumerate(probs):
        ref, scale = _ref_and_scale(p["a"], p["b"], p["alpha"], p["beta"], p["c0"], p["bn"], p["bm"])
        r = _assert_close(first[i].cpu(), ref, scale, TOL_SHORT, f"grouped problem {i}")
        print(f"grouped {i} ({p['M']}, {p['N']}, {p['K']}): err / scale {r:.3e}")
    # a second launch: same bits wherever C is not an input
    batch.run()
    torch.cuda.synchronize()
    for i, p in enumerate(probs):
        if p["beta"] == 0.0:
            assert torch.equal(p["cv"], first[i]), i
    # one by one through tadmm_gemm from the same C0: both entries instantiate the same gemm_tile
    for i, p in enumerate(probs):
        p["cv"].copy_(p["c0"].to(dev))
        h.check(h.lib.tadmm_gemm(h.ptr, C.byref(p["desc"]), torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    for i, p in enumerate(probs):
        assert torch.equal(p["cv"], first[i]), i


# ---------------------------------------------------------------------------------------------- B4
def test_refused_descriptors_do_no_work(dev):
    from tadmm import ops
    from tadmm._cabi import GemmDesc, TadmmError
    h = ops.Handle.get(dev.index)
    M, N, K = 12, 10, 8
    a2 = torch.zeros(M, 2 * K, 2, device=dev)                                # A with strides (2K, 2): no unit stride
    a = torch.ones(M, K, device=dev)
    b = torch.ones(K, N, device=dev)
    b2 = torch.zeros(K, N, 3, device=dev)                                    # B with strides (3N, 3)
    c = torch.full((M, N), CSENT, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def desc(A=a.data_ptr(), B=b.data_ptr(), Cp=c.data_ptr(), m=M, n=N, k=K, sa=(K, 1), sb=(N, 1)):
        return ops.gemm_desc(A, B, Cp, m, n, k, sa, sb, (N, 1))

    bad = {
        "A strides (2K, 2)": (desc(A=a2.data_ptr(), sa=(2 * K, 2)), "unit stride"),
        "B without unit stride": (desc(B=b2.data_ptr(), sb=(3 * N, 3)), "unit stride"),
        "M == 0": (desc(m=0), "empty"), "N == 0": (desc(n=0), "empty"), "K == 0": (desc(k=0), "empty"),
        "M < 0": (desc(m=-5), "empty"), "N < 0": (desc(n=-64), "empty"), "K < 0": (desc(k=-1), "empty"),
    }
    null = {"A null": desc(A=None), "B null": desc(B=None), "C null": desc(Cp=None)}
    for what, (d, cause) in bad.items():
        assert h.lib.tadmm_gemm(h.ptr, C.byref(d), stream) == ERR_INVALID, what
        assert cause in h.lib.tadmm_last_error(h.ptr).decode(), (what, h.lib.tadmm_last_error(h.ptr))
        # grouped entry: INVALID whatever the blob size, alone and behind a valid descriptor; no byte count
        for group in ([d], [desc(), d]):
            arr = (GemmDesc * len(group))(*group)
            blob, nb = (C.c_char * 4096)(), C.c_int(-7)
            assert h.lib.tadmm_gemm_pack_bytes(len(group), arr) == 0, what
            assert h.lib.tadmm_gemm_pack(len(group), arr, blob, 4096, C.byref(nb)) == ERR_INVALID, what
            assert h.lib.tadmm_gemm_pack(len(group), arr, blob, 0, C.byref(nb)) == ERR_INVALID, what
            with pytest.raises(TadmmError) as e:
                ops.GemmBatch(group, dev)
            assert e.value.status == ERR_INVALID, what
    for what, d in null.items():
        assert h.lib.tadmm_gemm(h.ptr, C.byref(d), stream) == ERR_INVALID, what
        assert "empty operand" in h.lib.tadmm_last_error(h.ptr).decode(), what
    torch.cuda.synchronize()
    assert bool((c == CSENT).all())                                          # nothing was launched
    # and the handle still works
    h.check(h.lib.tadmm_gemm(h.ptr, C.byref(desc()), stream))
    torch.cuda.synchronize()
    assert bool((c == float(K)).all())


# ---------------------------------------------------------------------------------------------- B5
LONG_K = (4608, 12608)
LONG_MN = (70, 90)


def _long_k_operands(kind, K):
    M, N = LONG_MN
    if kind == "gauss":
        return _randn((M, K), K), _randn((K, N), K + 1)
    if kind == "const":      # 0.1f * 0.3f is not representable: every product rounds the same way
        return torch.full((M, K), 0.1), torch.full((K, N), 0.3)
    assert kind == "rank1"
    return (torch.outer(_randn((M,), K + 2), _randn((K,), K + 3)),
            torch.outer(_randn((K,), K + 4), _randn((N,), K + 5)))


def _long_k_ratio(dev, kind, K):
    """max err / scale of one (70, 90, K) product on the device."""
    from tadmm import ops
    a, b = _long_k_operands(kind, K)
    got = ops.mm(a.to(dev), b.to(dev)).cpu()
    ref, scale = _ref_and_scale(a, b, 1.0, 0.0, None, None, None)
    assert torch.isfinite(got).all()
    return float(((got.double() - ref).abs() / scale).max())


@pytest.mark.parametrize("K", LONG_K)
@pytest.mark.parametrize("kind", ["gauss", "const", "rank1"])
def test_gemm_long_k(dev, kind, K):
    tol = tol_long(K)
    assert K != 4608 or tol < 1e-5                 # 8.3e-6: under the parity bar, under the plain accumulator's 1.3e-5
    ratio = _long_k_ratio(dev, kind, K)
    print(f"K {K} {kind}: err / scale {ratio:.3e} (bar {tol:.3e})")
    assert ratio <= tol, (kind, K, ratio, tol)


def test_gemm_long_k_plain_accumulator_is_recorded(dev, capsys):
    """TADMM_GEMM_PLAIN=1 (one fp32 accumulator over all of K) in a fresh child process, so that the switch never
    enters this process.  The figures are printed for the record; nothing about them is asserted: the switch is an
    A/B measurement aid, not a product path."""
    env = dict(os.environ, TADMM_GEMM_PLAIN="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    with capsys.disabled():
        print("\nplain accumulator (TADMM_GEMM_PLAIN=1), err / scale:", json.dumps(rec))


# ---------------------------------------------------------------------------------------------- B6
def _bf16_view(host2d, dev, ld, off):
    """bf16 device view (rows, K) with row stride ld, `off` elements into a NaN-filled buffer."""
    rows, K = host2d.shape
    buf = torch.full((off + rows * ld + 8,), float("nan"), dtype=torch.bfloat16, device=dev)
    v = buf[off:off + rows * ld].view(rows, ld)[:, :K]
    v.copy_(host2d)
    return v


@pytest.mark.parametrize("K", [24, 25, 28, 31, 300])
def test_gemm_bf16_nt_on_views(dev, K):
    """ld % 8 == 0 (16-byte loads) with K % 8 in {0, 1, 4, 7} -- the K tail inside a vector load --, ld % 8 != 0, and
    base offsets of 0 / 8 elements (16-byte aligned) and 1 element (not)."""
    from tadmm import ops
    M, N = 100, 70
    g = torch.Generator().manual_seed(K)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    bt = torch.randn(N, K, generator=g).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    ref = a.float().double() @ bt.float().double().T + bias.double()
    ld8 = -(-K // 8) * 8
    lds = sorted({ld8, ld8 + 8, K + 1 if (K + 1) % 8 else K + 3, ld8 + 3})
    assert {ld % 8 == 0 for ld in lds} == {True, False}
    seen = set()
    for lda in lds:
        for ldb in lds:
            for offa, offb in ((0, 0), (8, 8), (1, 0), (0, 1), (8, 1)):
                av, bv = _bf16_view(a, dev, lda, offa), _bf16_view(bt, dev, ldb, offb)
                seen.add((lda % 8 == 0 and av.data_ptr() % 16 == 0, ldb % 8 == 0 and bv.data_ptr() % 16 == 0, K % 8))
                got = ops.mm_nt_bf16(av, bv, bias.to(dev)).float().cpu()
                assert torch.isfinite(got).all(), (K, lda, ldb, offa, offb)     # NaN: a load outside the view
                err = (got.double() - ref).abs()
                worst = float((err / (ref.abs() + 1e-2 * ref.abs().max())).max())
                assert worst <= 6e-3, (K, lda, ldb, offa, offb, worst)
    assert {(va, vb) for va, vb, _ in seen} == {(True, True), (True, False), (False, True), (False, False)}


def test_gemm_bf16_nt_refuses_short_leading_dimensions(dev):
    from tadmm import ops
    h = ops.Handle.get(dev.index)
    M, N, K = 9, 7, 24
    a = torch.ones(M, K, dtype=torch.bfloat16, device=dev)
    bt = torch.ones(N, K, dtype=torch.bfloat16, device=dev)
    out = torch.full((M, N), 5.0, dtype=torch.bfloat16, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(lda=K, ldb=K, ldc=N):
        return h.lib.tadmm_gemm_bf16_nt(h.ptr, a.data_ptr(), bt.data_ptr(), out.data_ptr(), M, N, K, lda, ldb, ldc,
                                        None, stream)
    assert call(ldc=N - 1) == ERR_INVALID
    assert call(lda=K - 1) == ERR_INVALID
    assert call(ldb=K - 1) == ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out == float(K)).all())


if __name__ == "__main__":       # the child of test_gemm_long_k_plain_accumulator_is_recorded
    for p in (ROOT, os.path.join(ROOT, "dnn-compression-tensor-admm_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    device = torch.device("cuda:0")
    print(json.dumps({f"{kind}_K{K}": float("%.3e" % _long_k_ratio(device, kind, K))
                      for K in LONG_K for kind in ("gauss", "const", "rank1")}))
