"""Writes g14_filter_chain_bits.json: sha256 of what the fp64 kernels on the filter's critical chain compute on seeded
inputs -- the NT tile product `dgemm_nt_tile_kernel` in its three instantiations with every epilogue mode, the ring and
the gate, `daxpby_kernel`, the stand-alone `ops.dgemm` kernels, `ops.cholqr_` and two small filtered `ProjectionPlan`s --
recorded on the build of the commit named in the file.  These kernels promise the same arithmetic per output element
whatever the order of their loads and of their passes through LDS, so tests/test_gpu_filter_chain_bits.py asks for equal
hashes.

    python tests/golden/make_golden_filter_bits.py <commit id> [output file]   (on the MI355X, from the repository root)

`cases()` is shared with the test and is the only definition of the cases.  A case returns (name, inputs sha256, output
array, checks): `checks` is a list of (what, got, reference, bound) for the elementwise comparison against numpy float64.

Inputs come straight from the seeded generator, rounded to a grid of 2^-40 (entries below 8: 43 significant bits, so
products and sums of them are NOT exact and the order of the additions shows in the bytes); no input is the result of a
host matrix product, so the fixture does not depend on the host's BLAS.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_bits import _seed, _sha, samples  # noqa: E402

FIXTURE = os.path.join(HERE, "g14_filter_chain_bits.json")
GRID = 2.0 ** 40
U = 2.0 ** -53                                    # unit roundoff of fp64

TILES = [(32, 32), (64, 32), (64, 64)]            # (tile_m, tile_n): <32,4,32>, <32,2,64>, <64,2,64>
TILE_K = [32, 64, 96, 480]                        # one chunk | both register sets, no steady state | odd count | the chain's
DGEMM_SHAPES = [(32, 32, 32), (64, 64, 64), (96, 160, 96)]
CHOL_N = [32, 64, 128, 160, 192, 224, 256]
CHOL_NCOLS = [256, 448]
PLAN_TWO = [((384, 384), [16, 24, 24, 16], [1, 16, 64, 16, 1]), ((256, 256), [16, 16, 16, 16], [1, 16, 40, 16, 1])]
PLAN_224 = [((512, 512), [16, 32, 32, 16], [1, 16, 140, 16, 1])]
COEF = {"s2_zero": (-0.5, -0.75, 0.0), "s2": (-0.5, -0.75, 0.375)}


def _grid(a):
    return np.round(a * GRID) / GRID


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to("cuda:0")


def _operands(rng, M, N, K):
    """A (M, K), B (N, K), P, Q (M, N), theta (M,): exact zeros in A (row 1, a band of columns) and B (row 2); row 1 of
    P is +0.0, so that mode 1 with s0, s1 < 0 gives -0.0 in row 1 (s0 * (+0) + s1 * (+0)), which s2 * Q = +0 turns back."""
    A, B = _grid(rng.standard_normal((M, K))), _grid(rng.standard_normal((N, K)))
    P, Q = _grid(rng.standard_normal((M, N))), _grid(rng.standard_normal((M, N)))
    th = _grid(rng.standard_normal(M))
    A[1, :] = 0.0
    A[:, 5:9] = 0.0
    B[2, :] = 0.0
    P[1, :] = 0.0
    Q[1, :] = 0.0
    return A, B, P, Q, th


def _acc_ref(A, B):
    """numpy's product and the componentwise bound K * 2^-52 * |A| |B|^T: K * 2^-53 for each of the two sums compared."""
    K = A.shape[1]
    return A @ B.T, K * 2.0 * U * (np.abs(A) @ np.abs(B).T)


def _epilogue_ref(mode, coef, ref, bacc, P, Q, th, tile_n):
    """Reference and bound of one epilogue from the product's.  Each fp64 operation of the epilogue adds at most U times
    the magnitude it produces; g counts them generously."""
    M, N = ref.shape
    tn = (N + tile_n - 1) // tile_n
    pad = tn * tile_n - N

    def tiles(x):                                  # (M, N) -> (tn, M): fixed-order row sums per tile_n-column tile
        x = np.pad(x, ((0, 0), (0, pad)))
        return x.reshape(M, tn, tile_n).sum(axis=2).T
    if mode == 0:
        return [("C", ref, bacc)]
    if mode == 1:
        s0, s1, s2 = coef
        mag = abs(s0) * np.abs(ref) + abs(s1) * np.abs(P) + abs(s2) * np.abs(Q)
        return [("C", s0 * ref + s1 * P + s2 * Q, abs(s0) * bacc + 6 * U * mag)]
    if mode == 2:
        g = (tile_n + 2) * U
        return [("C", ref, bacc), ("rowpart", tiles(ref * P), tiles(bacc * np.abs(P)) + g * tiles(np.abs(ref * P)))]
    e = ref - th[:, None] * P
    be = bacc + 3 * U * (np.abs(ref) + np.abs(th[:, None] * P))
    g = (tile_n + 3) * U
    return [("rowpart", tiles(e * e), tiles(2 * np.abs(e) * be + be * be) + g * tiles(e * e))]


def _tile_case(tile, K, whole):
    """The five epilogues (0, 1 with s2 = 0, 1 with s2 != 0, 2, 3) of one product, one launch each."""
    import torch
    from tadmm import ops
    tile_m, tile_n = tile
    M, N = (tile_m, tile_n) if whole else (96, 160)
    name = "tile_%dx%d_K%d_%dx%d" % (tile_m, tile_n, K, M, N)
    rng = np.random.default_rng(_seed(name))
    A, B, P, Q, th = _operands(rng, M, N, K)
    ref, bacc = _acc_ref(A, B)
    a, b, p, q, t = _dev(A), _dev(B), _dev(P), _dev(Q), _dev(th)
    tn = (N + tile_n - 1) // tile_n
    outs, checks = [], []
    for mode, ck in ((0, None), (1, "s2_zero"), (1, "s2"), (2, None), (3, None)):
        coef = COEF[ck] if ck else None
        c = torch.full((M, N), 7.0, dtype=torch.float64, device="cuda:0")
        rp = torch.full((tn, M), 7.0, dtype=torch.float64, device="cuda:0")
        ops.dgemm_tile([dict(A=a, B=b, C=c, P=p, Q=q, M=M, N=N, K=K, mode=mode, theta=t, rowpart=rp,
                             coef=None if coef is None else _dev(np.array(coef)))], tile_m, tile_n)
        got = {"C": c.cpu().numpy(), "rowpart": rp.cpu().numpy()}
        outs += [got["C"].ravel(), got["rowpart"].ravel()]
        for what, want, bound in _epilogue_ref(mode, coef, ref, bacc, P, Q, th, tile_n):
            checks.append(("%s mode %d %s %s" % (name, mode, ck or "", what), got[what], want, bound))
        if mode == 1 and ck == "s2_zero":
            checks.append((name + " row 1 is -0.0", np.signbit(got["C"][1]).astype(np.float64), np.ones(N), np.zeros(N)))
    return name, _sha(A, B, P, Q, th), np.concatenate(outs), checks


def _ring_case(rot):
    """Recurrence step k = 2 on a ring of three images: C = slot (rot + 2) % 3, A = P = slot (rot + 1) % 3, Q = slot rot,
    B = G explicit; every tile shape.  All three slots are hashed: only C's may change."""
    import torch
    from tadmm import ops
    name = "ring_rot%d" % rot
    rng = np.random.default_rng(_seed(name))
    M, N = 96, 160
    G = _grid(rng.standard_normal((N, N)))
    slots = [_grid(rng.standard_normal((M, N))) for _ in range(3)]
    coef = COEF["s2"]
    iA, iQ = (rot + 1) % 3, rot % 3
    ref, bacc = _acc_ref(slots[iA], G)
    want, bound = _epilogue_ref(1, coef, ref, bacc, slots[iA], slots[iQ], None, 32)[0][1:]
    outs, checks = [], []
    for tile_m, tile_n in TILES:
        ring = [_dev(s) for s in slots]
        ops.dgemm_tile([dict(B=_dev(G), ring=ring, rot=_dev(np.array([rot], dtype=np.int32)), selA=1, selP=1, selQ=0, selC=2,
                             M=M, N=N, K=N, ldb=N, mode=1, coef=_dev(np.array(coef)))], tile_m, tile_n)
        got = [r.cpu().numpy() for r in ring]
        outs += [g.ravel() for g in got]
        checks.append(("%s tile %dx%d C" % (name, tile_m, tile_n), got[(rot + 2) % 3], want, bound))
        for i in (iA, iQ):
            checks.append(("%s slot %d untouched" % (name, i), got[i], slots[i], np.zeros((M, N))))
    return name, _sha(G, *slots), np.concatenate(outs), checks


def _gate_case():
    """Three problems in one launch, the middle one gated off (gate word 1 < gate_min 2): its C and rowpart keep their fill."""
    import torch
    from tadmm import ops
    name = "gate_three_problems"
    rng = np.random.default_rng(_seed(name))
    shapes = [(32, 32, 32), (96, 160, 96), (64, 64, 64)]
    outs, checks, ins = [], [], []
    for tile_m, tile_n in TILES:
        probs, keep = [], []
        for i, (M, N, K) in enumerate(shapes):
            A, B, P, Q, th = _operands(rng, M, N, K)
            ins += [A, B, P]
            tn = (N + tile_n - 1) // tile_n
            c = torch.full((M, N), 7.0, dtype=torch.float64, device="cuda:0")
            rp = torch.full((tn, M), 7.0, dtype=torch.float64, device="cuda:0")
            gate = _dev(np.array([1 if i == 1 else 2], dtype=np.int32))
            probs.append(dict(A=_dev(A), B=_dev(B), C=c, P=_dev(P), M=M, N=N, K=K, mode=2, rowpart=rp, gate=gate, gate_min=2))
            keep.append((A, B, P, c, rp))
        ops.dgemm_tile(probs, tile_m, tile_n)
        for i, (A, B, P, c, rp) in enumerate(keep):
            got = {"C": c.cpu().numpy(), "rowpart": rp.cpu().numpy()}
            outs += [got["C"].ravel(), got["rowpart"].ravel()]
            if i == 1:
                for what in got:
                    checks.append(("%s gated %s untouched" % (name, what), got[what], np.full_like(got[what], 7.0),
                                   np.zeros_like(got[what])))
            else:
                ref, bacc = _acc_ref(A, B)
                for what, want, bound in _epilogue_ref(2, None, ref, bacc, P, None, None, tile_n):
                    checks.append(("%s tile %dx%d problem %d %s" % (name, tile_m, tile_n, i, what), got[what], want, bound))
    return name, _sha(*ins), np.concatenate(outs), checks


def _axpby_case(M, ldc, ring):
    """C <- s0 * C + s1 * P in place over M * ldc elements (2048: two whole blocks; 1088: a part block), C and P named
    explicitly or through the ring."""
    from tadmm import ops
    name = "daxpby_%dx%d%s" % (M, ldc, "_ring" if ring else "")
    rng = np.random.default_rng(_seed(name))
    Ch, Ph, X = (_grid(rng.standard_normal((M, ldc))) for _ in range(3))
    Ch[1, :] = 0.0
    Ph[1, :] = 0.0
    s0, s1 = -0.5, -0.75
    coef = _dev(np.array([s0, s1, 0.0]))
    if ring:
        bufs = [_dev(X), _dev(Ch), _dev(Ph)]                      # rot = 1: C = slot 1, P = slot 2
        ops.dgemm_tile([dict(ring=bufs, rot=_dev(np.array([1], dtype=np.int32)), selC=0, selP=1, M=M, N=32, K=32, coef=coef,
                             lda=32, ldb=32)], 32, 32, axpby=True)
        got, rest = bufs[1].cpu().numpy(), [bufs[0].cpu().numpy(), bufs[2].cpu().numpy()]
    else:
        c, p = _dev(Ch), _dev(Ph)
        ops.dgemm_tile([dict(C=c, P=p, M=M, N=32, K=32, coef=coef, lda=32, ldb=32)], 32, 32, axpby=True)
        got, rest = c.cpu().numpy(), [p.cpu().numpy()]
    bound = 3 * U * (abs(s0) * np.abs(Ch) + abs(s1) * np.abs(Ph))
    checks = [(name, got, s0 * Ch + s1 * Ph, bound),
              (name + " row 1 is -0.0", np.signbit(got[1]).astype(np.float64), np.ones(ldc), np.zeros(ldc))]
    return name, _sha(Ch, Ph, X), np.concatenate([got.ravel()] + [r.ravel() for r in rest]), checks


def _dgemm_case(M, N, K, nt, old):
    """`ops.dgemm`: the 64x64 tile kernel, or with TADMM_DGEMM_OLD (read at every call) and for NN the 32x32 K-split kernel."""
    from tadmm import ops
    name = "dgemm_%s_%dx%dx%d%s" % ("nt" if nt else "nn", M, N, K, "_old" if old else "")
    rng = np.random.default_rng(_seed(name))
    A, B = _grid(rng.standard_normal((M, K))), _grid(rng.standard_normal((N, K)))
    A[1, :] = 0.0
    before = os.environ.pop("TADMM_DGEMM_OLD", None)
    try:
        if old:
            os.environ["TADMM_DGEMM_OLD"] = "1"
        got = ops.dgemm(_dev(A), _dev(B if nt else B.T), nt).cpu().numpy()
    finally:
        os.environ.pop("TADMM_DGEMM_OLD", None)
        if before is not None:
            os.environ["TADMM_DGEMM_OLD"] = before
    ref, bacc = _acc_ref(A, B)
    return name, _sha(A, B), got, [(name, got, ref, bacc)]


def _chol_block(name, n, ncols):
    """Rows close to orthonormal: the identity pattern plus Gaussian noise of norm ~0.25 per row (condition number < 3)."""
    rng = np.random.default_rng(_seed(name))
    y = np.zeros((n, ncols))
    y[np.arange(n), np.arange(n)] = 1.0
    return _grid(y + 0.25 * rng.standard_normal((n, ncols)) / np.sqrt(ncols))


def _cholqr_case(n, ncols):
    from tadmm import ops
    name = "cholqr_%dx%d" % (n, ncols)
    y = _chol_block(name, n, ncols)
    yt = _dev(y)
    ok = ops.cholqr_(yt)
    got = yt.cpu().numpy()
    # one pass leaves cond^2 * O(n) roundings: 1e-12 is a sanity bound on a known-good result, far above that
    checks = [(name + " flag", np.array([float(ok)]), np.ones(1), np.zeros(1)),
              (name + " Q Q^T = I", got @ got.T, np.eye(n), np.full((n, n), 1e-12))]
    return name, _sha(y), np.concatenate([got.ravel(), np.array([float(ok)])]), checks


def _cholqr_equal_columns_case():
    from tadmm import ops
    name = "cholqr_128x256_two_equal_columns"
    y = _chol_block(name, 128, 256)
    y[77] = y[5]
    ok = ops.cholqr_(_dev(y))
    return name, _sha(y), np.array([float(ok)]), [(name + " flag", np.array([float(ok)]), np.zeros(1), np.zeros(1))]


def _plan_case(name, table):
    """As `_tt_linear_plan_case` of make_golden_bits.py, and every eligible problem must take the filter in both runs."""
    import torch
    from tadmm import ops
    from tadmm._cabi import KIND_TT_LINEAR
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(_seed(name))
    layers, ins = [], []
    for shape, tts, ranks in table:
        wh = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        w = torch.from_numpy(wh).to(dev)
        layers.append(dict(kind=KIND_TT_LINEAR, W=w, U=torch.zeros_like(w), Z=torch.zeros_like(w), tt_shapes=tts, ranks=ranks))
        ins.append(wh)
    plan = ops.ProjectionPlan(layers)
    parts, checks = [], []
    for it in range(2):
        r = plan.run(update_u=True)
        torch.cuda.synchronize()
        parts.append(r.detach().cpu().numpy().astype(np.float64).view(np.uint8))
        st = plan.filter_stats()
        print(name, "run", it, st, flush=True)
        took = float(st["eligible"] == st["solves"] and st["solves"] > 0 and st["fallbacks"] == 0)
        checks.append(("%s run %d filter_stats %s" % (name, it, st), np.array([took]), np.ones(1), np.zeros(1)))
    for L in layers:
        parts.append(L["Z"].cpu().numpy().view(np.uint8).ravel())
        parts.append(L["U"].cpu().numpy().view(np.uint8).ravel())
    plan.close()
    return name, _sha(*ins), np.concatenate([p.ravel() for p in parts]), checks


def cases():
    for tile in TILES:
        for K in TILE_K:
            for whole in (True, False):
                yield lambda a=(tile, K, whole): _tile_case(*a)
    for rot in range(3):
        yield lambda r=rot: _ring_case(r)
    yield _gate_case
    yield lambda: _axpby_case(32, 64, False)
    yield lambda: _axpby_case(32, 34, False)
    yield lambda: _axpby_case(32, 34, True)
    for old in (False, True):
        for s in DGEMM_SHAPES:
            yield lambda a=(s, old): _dgemm_case(*a[0], True, a[1])
    yield lambda: _dgemm_case(64, 96, 48, False, False)
    for ncols in CHOL_NCOLS:
        for n in CHOL_N:
            yield lambda a=(n, ncols): _cholqr_case(*a)
    yield _cholqr_equal_columns_case
    yield lambda: _plan_case("plan_filter_96_and_64_columns", PLAN_TWO)
    yield lambda: _plan_case("plan_filter_224_columns", PLAN_224)


def failed_checks(checks):
    """(what, largest excess over the bound, index) of every elementwise check that does not hold; NaN fails."""
    bad = []
    for what, got, want, bound in checks:
        got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound)
        if got.shape != want.shape:
            bad.append((what, "shape %s vs %s" % (got.shape, want.shape), None))
            continue
        excess = np.abs(got - want) - bound
        if not np.all(excess <= 0):                # (NaN compares false)
            i = int(np.nanargmax(np.where(np.isnan(excess), np.inf, excess)))
            bad.append((what, float(excess.ravel()[i]), i))
    return bad


def main():
    commit = sys.argv[1] if len(sys.argv) > 1 else "unknown"
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "dnn-compression-tensor-admm_amd"))
    doc = {"commit": commit, "cases": {}}
    status = 0
    for make in cases():
        name, in_sha, out, checks = make()
        doc["cases"][name] = {"inputs_sha256": in_sha, "output_sha256": _sha(out), "dtype": str(out.dtype),
                              "numel": int(out.size), "samples": samples(out)}
        bad = failed_checks(checks)
        print(name, doc["cases"][name]["output_sha256"][:16], "checks %d" % len(checks), "FAILED %s" % bad if bad else "ok",
              flush=True)
        status |= bool(bad)
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
