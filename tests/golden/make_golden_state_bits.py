"""Writes g16_state_bits.json: sha256 of what small filtered `ProjectionPlan`s and split-K Grams compute on seeded
inputs, recorded on the build of the commit named in the file, with the course the filter took (`filter_stats()` and the
Jacobi sweep count of each run).  The cases sit where the filter's STATE kernels (csrc/filter.hip: plan, flags, theta,
moments, verdict, emit, init) and the Gram's split-K reduce (csrc/gram.hip) can go wrong and the cases of g13 / g14 do not
reach.  Those kernels only move state and add in a fixed order, so tests/test_gpu_state_bits.py asks for equal hashes and
an equal course.

    python tests/golden/make_golden_state_bits.py <commit id> [output file]   (on the MI355X, from the repository root)

`cases()` is shared with the test and is the only definition of the cases.  A case returns (name, inputs sha256, output
array, record): `record` holds the per-run filter statistics and sweep counts (empty for the Gram cases).

No input is the result of a host matrix product whose rounding could depend on the host's BLAS: weights come straight
from the seeded generator, are scaled by exact powers of two, or are products of small dyadic factors whose every partial
sum is a float32 number.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_bits import _seed, _sha, samples  # noqa: E402

FIXTURE = os.path.join(HERE, "g16_state_bits.json")

# (name, shape, tt_shapes, ranks, kind of weight).  The level of the (r1 n2) x (n3 n4) unfoldings holds the problems
# described; the outer levels are 16-column full solves whose Grams are split over K.
#   cap256_and_160: N = 512 keeping 200 -> the block is capped at 256 columns (one full pass of the 256-thread rank loop;
#     r32 = 224 > r: zero tail of theta, the c < r bounds); N = 384 keeping 100 -> a block of 160 columns (r32 = 128 > r).
#     Both Grams are written directly (no split), the 16-column ones of the outer levels are reduced from partials.
#   two_stage_counts: two 256-column problems keeping 50 (block 96, r32 = 64) in one group, a flat Gaussian spectrum and
#     one whose columns decay by powers of two: the second needs fewer stages, so the plan kernel's gated branch runs for
#     it while the first still filters.
#   low_rank_beside_healthy: an exactly rank-40 weight keeping 64 (the Cholesky breaks down: `bad`, early-outs of plan,
#     flags, moments, verdict and emit, fallback solve) beside a healthy problem keeping 40, and a 160 x 640 full solve
#     whose Gram is split 3 ways in the same level as the two direct-write Grams.
PLANS = [
    ("plan_cap256_and_160", [((512, 512), [16, 32, 32, 16], [1, 16, 200, 16, 1], "gauss"),
                             ((384, 384), [16, 24, 24, 16], [1, 16, 100, 16, 1], "gauss")], None),
    ("plan_two_stage_counts", [((256, 256), [16, 16, 16, 16], [1, 16, 50, 16, 1], "gauss"),
                               ((256, 256), [16, 16, 16, 16], [1, 16, 50, 16, 1], "decay")], None),
    ("plan_low_rank_beside_healthy", [((256, 256), [16, 16, 16, 16], [1, 16, 64, 16, 1], "rank40"),
                                      ((256, 256), [16, 16, 16, 16], [1, 16, 40, 16, 1], "gauss"),
                                      ((160, 640), [10, 16, 32, 20], [1, 10, 60, 20, 1], "gauss")], 1),
]
# stand-alone Gram (`ops.gram`: chunks of 256 columns for these shapes): ksplit 2, 3 (tail only), 5, 11 (one full group of
# eight plus a tail of three); N no multiple of the 32-wide tile, one and three tile pairs
GRAM_SPLIT = [((30, 500), 2), ((17, 700), 3), ((45, 1200), 5), ((33, 2700), 11)]


def _weight(rng, shape, kind):
    if kind == "gauss":
        return (0.1 * rng.standard_normal(shape)).astype(np.float32)
    if kind == "decay":                       # column j scaled by 2^-(j // 8): exact in float32
        w = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        return w * np.exp2(-(np.arange(shape[1]) // 8)).astype(np.float32)
    # rank40: factors on a grid of 2^-4 below 4 in magnitude -> every product is a multiple of 2^-8 and every partial sum
    # of 40 of them stays below 2^10: 18 bits, exact in float32 whatever the order of the additions
    a = np.clip(np.round(rng.standard_normal((shape[0], 40)) * 16.0) / 16.0, -3.9375, 3.9375)
    b = np.clip(np.round(rng.standard_normal((40, shape[1])) * 16.0) / 16.0, -3.9375, 3.9375)
    w = (a @ b) * 2.0 ** -6
    assert np.array_equal(w.astype(np.float32).astype(np.float64), w)
    return w.astype(np.float32)


def _plan_case(name, table, want_fallbacks):
    """TT-linear layers through one ProjectionPlan, two iterations with update_u=True: the residuals, Z and U, and the
    course of each run."""
    import torch
    from tadmm import ops
    from tadmm._cabi import KIND_TT_LINEAR
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(_seed(name))
    layers, ins = [], []
    for shape, tts, ranks, kind in table:
        wh = _weight(rng, shape, kind)
        w = torch.from_numpy(wh).to(dev)
        layers.append(dict(kind=KIND_TT_LINEAR, W=w, U=torch.zeros_like(w), Z=torch.zeros_like(w), tt_shapes=tts, ranks=ranks))
        ins.append(wh)
    plan = ops.ProjectionPlan(layers)
    parts, record = [], {"filter_stats": [], "jacobi_sweeps": []}
    for it in range(2):
        r = plan.run(update_u=True)
        torch.cuda.synchronize()
        parts.append(r.detach().cpu().numpy().astype(np.float64).view(np.uint8))
        st = plan.filter_stats()
        record["filter_stats"].append([st["eligible"], st["solves"], st["fallbacks"], st["stages"]])
        record["jacobi_sweeps"].append(int(plan.last_timing()["jacobi_sweeps"]))
        print(name, "run", it, st, "sweeps", record["jacobi_sweeps"][-1], flush=True)
    for L in layers:
        parts.append(L["Z"].cpu().numpy().view(np.uint8).ravel())
        parts.append(L["U"].cpu().numpy().view(np.uint8).ravel())
    plan.close()
    record["want_fallbacks"] = want_fallbacks
    return name, _sha(*ins), np.concatenate([p.ravel() for p in parts]), record


def _gram_case(shape, ksplit):
    import torch
    from tadmm import ops
    m, n = shape
    name = "gram_%dx%d_ksplit%d" % (m, n, ksplit)
    rng = np.random.default_rng(_seed(name))
    ah = rng.standard_normal((m, n)).astype(np.float32)
    g = ops.gram(torch.from_numpy(ah).to("cuda:0"))
    torch.cuda.synchronize()
    return name, _sha(ah), g.cpu().numpy(), {}


def cases():
    for name, table, fb in PLANS:
        yield lambda a=(name, table, fb): _plan_case(*a)
    for shape, ks in GRAM_SPLIT:
        yield lambda a=(shape, ks): _gram_case(*a)


def main():
    commit = sys.argv[1] if len(sys.argv) > 1 else "unknown"
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "dnn-compression-tensor-admm_amd"))
    doc = {"commit": commit, "cases": {}}
    for make in cases():
        name, in_sha, out, record = make()
        want_fb = record.pop("want_fallbacks", None)
        if want_fb is not None:               # the chosen input must send exactly this many problems to the full solve
            assert record["filter_stats"][0][2] == want_fb, (name, record)
        doc["cases"][name] = {"inputs_sha256": in_sha, "output_sha256": _sha(out), "dtype": str(out.dtype),
                              "numel": int(out.size), "samples": samples(out), **record}
        print(name, doc["cases"][name]["output_sha256"][:16], flush=True)
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
