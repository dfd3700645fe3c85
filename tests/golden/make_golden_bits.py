"""Writes g12_gemm_gram_bits.json: sha256 of what `ops.mm`, `ops.GemmBatch`, `ops.gram` and a small `ProjectionPlan`
compute on seeded inputs, recorded on the build of the commit named in the file.  The fp32 GEMM and the fp64 Gram promise
the same arithmetic per output element whatever their data movement looks like, so tests/test_gpu_gemm_gram_bits.py asks
for equal hashes.

    python tests/golden/make_golden_bits.py <commit id>        (on the MI355X, from the repository root, after build())

`cases()` is shared with the test: it yields (name, inputs sha256, output array) and is the only definition of the cases.

A second list, `eigh_cases()`, covers the Jacobi eigen-solver the same way (g13_eigh_bits.json, tests/test_gpu_eigh_bits.py):
every launch shape of csrc/jacobi.hip through `ops.eigh`, `ops.eigh_partial` and two `ProjectionPlan`s.

    python tests/golden/make_golden_bits.py <commit id> [output file] eigh
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "g12_gemm_gram_bits.json")
EIGH_FIXTURE = os.path.join(HERE, "g13_eigh_bits.json")

MM_SHAPES = [(1, 5, 3), (64, 64, 16), (64, 64, 64), (70, 90, 65), (130, 33, 77), (75, 70, 200), (257, 129, 333)]
LAYOUT_SHAPES = [(70, 90, 65), (130, 33, 77)]
VIEW_SHAPES = [(70, 90, 65), (75, 70, 200)]
GRAM_SHAPES = [(5, 5), (17, 33), (33, 17), (30, 1000), (32, 5000), (105, 300), (300, 105), (130, 2048), (945, 512),
               (720, 900)]
N_SAMPLES = 64


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def _mat(rng, rows, cols, transposed, dev, padded=False):
    """(rows, cols) float32 device matrix and its host copy; transposed: stored as (cols, rows) and viewed back;
    padded: rows 3 elements longer than cols and the first element one past the buffer's start (unaligned rows)."""
    import torch
    host = rng.standard_normal((rows, cols)).astype(np.float32)
    if padded:
        buf = torch.zeros(1 + rows * (cols + 3), dtype=torch.float32, device=dev)
        t = buf.as_strided((rows, cols), (cols + 3, 1), 1)
        t.copy_(torch.from_numpy(host))
    elif transposed:
        t = torch.from_numpy(np.ascontiguousarray(host.T)).to(dev).t()
    else:
        t = torch.from_numpy(host).to(dev)
    return t, host


def _out(rows, cols, transposed, dev, padded=False):
    import torch
    if padded:
        return torch.zeros(1 + rows * (cols + 3), dtype=torch.float32, device=dev).as_strided((rows, cols), (cols + 3, 1), 1)
    if transposed:
        return torch.zeros(cols, rows, dtype=torch.float32, device=dev).t()
    return torch.zeros(rows, cols, dtype=torch.float32, device=dev)


def _mm_case(name, M, N, K, ta=0, tb=0, tc=0, padded=False, const=False, full=False):
    import torch
    from tadmm import ops
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(_seed(name))
    a, ah = _mat(rng, M, K, ta, dev, padded)
    b, bh = _mat(rng, K, N, tb, dev, padded)
    if const:
        a.fill_(0.37)
        b.fill_(-1.3)
        ah, bh = np.full_like(ah, 0.37), np.full_like(bh, -1.3)
    out = _out(M, N, tc, dev, padded)
    ins = [ah, bh]
    kw = {}
    if full:
        c0 = rng.standard_normal((M, N)).astype(np.float32)
        bn = rng.standard_normal(N).astype(np.float32)
        bm = rng.standard_normal(M).astype(np.float32)
        out.copy_(torch.from_numpy(c0))
        kw = dict(alpha=0.75, beta=-0.5, bias_n=torch.from_numpy(bn).to(dev), bias_m=torch.from_numpy(bm).to(dev))
        ins += [c0, bn, bm]
    ops.mm(a, b, out=out, **kw)
    torch.cuda.synchronize()
    return name, _sha(*ins), out.cpu().numpy()


def _batch_case(name):
    """One grouped launch of seven problems of mixed shapes and layouts."""
    import torch
    from tadmm import ops
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(_seed(name))
    probs = [(1, 5, 3, 0, 0, 0), (64, 64, 64, 1, 0, 0), (70, 90, 65, 0, 1, 1), (130, 33, 77, 1, 1, 0),
             (75, 70, 200, 0, 0, 1), (257, 129, 333, 1, 0, 1), (33, 130, 480, 0, 1, 0)]
    descs, outs, ins, keep = [], [], [], []
    for M, N, K, ta, tb, tc in probs:
        a, ah = _mat(rng, M, K, ta, dev)
        b, bh = _mat(rng, K, N, tb, dev)
        o = _out(M, N, tc, dev)
        descs.append(ops.gemm_desc(a.data_ptr(), b.data_ptr(), o.data_ptr(), M, N, K, a.stride(), b.stride(), o.stride()))
        outs.append(o)
        ins += [ah, bh]
        keep += [a, b]
    ops.GemmBatch(descs, dev).run()
    torch.cuda.synchronize()
    return name, _sha(*ins), np.concatenate([o.cpu().numpy().ravel() for o in outs])


def _gram_case(m, n):
    import torch
    from tadmm import ops
    name = "gram_%dx%d" % (m, n)
    rng = np.random.default_rng(_seed(name))
    ah = rng.standard_normal((m, n)).astype(np.float32)
    g = ops.gram(torch.from_numpy(ah).to("cuda:0"))
    torch.cuda.synchronize()
    return name, _sha(ah), g.cpu().numpy()


def _plan_case(name):
    """Three TT layers through one ProjectionPlan, two iterations with update_u=True: Z, U and the residuals."""
    import torch
    from tadmm import ops
    from tadmm._cabi import KIND_TT_CONV, KIND_TT_LINEAR
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(_seed(name))
    table = [(KIND_TT_CONV, (64, 64, 3, 3), [8, 8, 9, 8, 8], [1, 6, 20, 20, 6, 1]),
             (KIND_TT_LINEAR, (48, 24), [6, 8, 4, 6], [1, 5, 20, 5, 1]),
             (KIND_TT_CONV, (16, 16, 3, 3), [4, 4, 9, 4, 4], [1, 4, 12, 12, 4, 1])]
    layers, ins = [], []
    for kind, shape, tts, ranks in table:
        wh = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        w = torch.from_numpy(wh).to(dev)
        layers.append(dict(kind=kind, W=w, U=torch.zeros_like(w), Z=torch.zeros_like(w), tt_shapes=tts, ranks=ranks))
        ins.append(wh)
    plan = ops.ProjectionPlan(layers)
    parts = []
    for _ in range(2):
        r = plan.run(update_u=True)
        torch.cuda.synchronize()
        parts.append(r.detach().cpu().numpy().astype(np.float64).view(np.uint8))
    for L in layers:
        parts.append(L["Z"].cpu().numpy().view(np.uint8).ravel())
        parts.append(L["U"].cpu().numpy().view(np.uint8).ravel())
    plan.close()
    return name, _sha(*ins), np.concatenate([p.ravel() for p in parts])


def cases():
    for M, N, K in MM_SHAPES:
        yield lambda s=(M, N, K): _mm_case("mm_%dx%dx%d" % s, *s)
    yield lambda: _mm_case("mm_const_70x90x4608", 70, 90, 4608, const=True)
    for M, N, K in LAYOUT_SHAPES:
        for lay in range(8):
            ta, tb, tc = lay & 1, (lay >> 1) & 1, (lay >> 2) & 1
            yield lambda s=(M, N, K), l=(ta, tb, tc): _mm_case("mm_%dx%dx%d_t%d%d%d" % (s + l), *s, *l)
    for M, N, K in VIEW_SHAPES:
        yield lambda s=(M, N, K): _mm_case("mm_%dx%dx%d_padded_view" % s, *s, padded=True)
    yield lambda: _mm_case("mm_130x33x77_alpha_beta_biases", 130, 33, 77, full=True)
    yield lambda: _batch_case("gemm_batch_7")
    for m, n in GRAM_SHAPES:
        yield lambda s=(m, n): _gram_case(*s)
    yield lambda: _plan_case("plan_tt3_two_iterations")


# N of `ops.eigh`: 48 single-launch solver | 96 .. 500 super-pair kernel + self pass (ld 128 .. 512; 500 pads to 512, the
# largest that fits) | 520, 1100 resident pair kernel (ld 640, 1152: smallest and largest) | 1160, 2080 streamed pair
# kernel (ld 1280 = one full chunk + 256, ld 2176 = two full chunks + 128)
EIGH_N = [48, 96, 130, 288, 500, 520, 1100, 1160, 2080]
EIGH_LOW_RANK_N = [130, 520]
# one plan, four TT-linear layers: the level of the (r1 n2) x (n3 n4) unfoldings holds full solves of 96, 128 and 160 columns
# (6, 8 and 10 super-block players: an aligned period with idle ticks, problems finishing at different sweeps) and, for the
# 384-column layer, the filter's 96-column Rayleigh-Ritz problem
PLAN_SUPER = [((96, 96), [8, 12, 12, 8], [1, 8, 24, 8, 1]), ((128, 128), [8, 16, 16, 8], [1, 8, 32, 8, 1]),
              ((160, 160), [8, 20, 20, 8], [1, 8, 40, 8, 1]), ((384, 384), [16, 24, 24, 16], [1, 16, 64, 16, 1])]
# the 640-column full solve (rank 400: no filter) puts its whole group on the pair kernel
PLAN_PAIRS = [((640, 640), [20, 32, 32, 20], [1, 20, 400, 20, 1])]


def _eigh_gram(name, N, kind):
    """Symmetric PSD test matrix: "gauss" / "decay" as tests/test_gpu_kernels.py::test_eigh_jacobi, "rank4" = exactly
    rank N/4 (unrotated pairs, the weighted measure, workgroups that return before the update).  The factor is rounded to
    a grid (2^-16 of entries below 8, 2^-20 of entries below 1) on which every product and every partial sum of a a^T is
    an fp64 number, so G does not depend on the order in which the host's BLAS adds."""
    rng = np.random.default_rng(_seed(name))
    if kind == "gauss":
        a, grid = rng.standard_normal((N, 3 * N)), 2.0 ** 16
    elif kind == "decay":
        q, _ = np.linalg.qr(rng.standard_normal((N, N)))
        a, grid = q * np.exp(-6.0 * np.arange(N) / N), 2.0 ** 20
    else:
        a, grid = rng.standard_normal((N, N // 4)), 2.0 ** 16
    a = np.round(a * grid) / grid
    G = a @ a.T
    return 0.5 * (G + G.T)


def _eigh_case(N, kind, r=None):
    import torch
    from tadmm import ops
    name = "eigh_%d_%s" % (N, kind) if r is None else "eigh_partial_%d_r%d_%s" % (N, r, kind)
    G = _eigh_gram(name, N, kind)
    g = torch.from_numpy(G).to("cuda:0")
    ev, vec, info = ops.eigh(g) if r is None else ops.eigh_partial(g, r)
    torch.cuda.synchronize()
    # eigenvalues, eigenvectors, and the sweep count (eigh) / the route (eigh_partial)
    out = np.concatenate([ev.cpu().numpy().ravel(), vec.cpu().numpy().ravel(), np.array([float(info)])])
    return name, _sha(G), out


def _tt_linear_plan_case(name, table):
    """TT-linear layers through one ProjectionPlan, two iterations with update_u=True: the residuals, Z and U."""
    import torch
    from tadmm import ops
    from tadmm._cabi import KIND_TT_LINEAR
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(_seed(name))
    layers, ins = [], []
    for shape, tts, ranks in table:
        wh = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        w = torch.from_numpy(wh).to(dev)
        layers.append(dict(kind=KIND_TT_LINEAR, W=w, U=torch.zeros_like(w), Z=torch.zeros_like(w), tt_shapes=tts,
                           ranks=ranks))
        ins.append(wh)
    plan = ops.ProjectionPlan(layers)
    parts = []
    for _ in range(2):
        r = plan.run(update_u=True)
        torch.cuda.synchronize()
        parts.append(r.detach().cpu().numpy().astype(np.float64).view(np.uint8))
    for L in layers:
        parts.append(L["Z"].cpu().numpy().view(np.uint8).ravel())
        parts.append(L["U"].cpu().numpy().view(np.uint8).ravel())
    plan.close()
    return name, _sha(*ins), np.concatenate([p.ravel() for p in parts])


def eigh_cases():
    for N in EIGH_N:
        for kind in ("gauss", "decay"):
            yield lambda a=(N, kind): _eigh_case(*a)
    for N in EIGH_LOW_RANK_N:
        yield lambda n=N: _eigh_case(n, "rank4")
    yield lambda: _eigh_case(130, "gauss", r=20)
    yield lambda: _tt_linear_plan_case("plan_super_pairs_6_8_10_players_and_rr96", PLAN_SUPER)
    yield lambda: _tt_linear_plan_case("plan_pairs_640", PLAN_PAIRS)


def samples(out):
    """64 evenly spaced entries of the flattened output, as (index, hex of the bytes) for diagnostics."""
    flat = np.ascontiguousarray(out).ravel()
    idx = np.unique(np.linspace(0, flat.size - 1, N_SAMPLES).astype(np.int64))
    return [[int(i), flat[i:i + 1].tobytes().hex()] for i in idx]


def main():
    commit = sys.argv[1] if len(sys.argv) > 1 else "unknown"
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "dnn-compression-tensor-admm_amd"))
    eigh = len(sys.argv) > 3 and sys.argv[3] == "eigh"
    doc = {"commit": commit, "cases": {}}
    for make in (eigh_cases() if eigh else cases()):
        name, in_sha, out = make()
        doc["cases"][name] = {"inputs_sha256": in_sha, "output_sha256": _sha(out), "dtype": str(out.dtype),
                              "numel": int(out.size), "samples": samples(out)}
        print(name, doc["cases"][name]["output_sha256"][:16], flush=True)
    with open(sys.argv[2] if len(sys.argv) > 2 else (EIGH_FIXTURE if eigh else FIXTURE), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
