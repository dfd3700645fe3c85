"""Writes g17_tick_bits.json: sha256 of what the super-pair route of the Jacobi eigen-solver (csrc/jacobi.hip,
jacobi_tick3_kernel: N > 64, rows of at most 512 doubles) computes on inputs that steer single workgroups through each of
its exits, recorded on the build of the commit named in the file.  tests/test_gpu_tick_fused_bits.py asks for equal hashes:
the within-super-block rotations of the first tick of a sweep may run in a launch of their own or inside the tick, the
floating-point operations and their order are the same.

    python tests/golden/make_golden_tick_bits.py <commit id> [output file]     (on the MI355X, after build())

`cases()` is shared with the test and is the only definition of the cases.  A case returns
(name, inputs sha256, output array, [(eigenvalues, float64 reference eigenvalues), ...]): the test also holds every
solve against numpy.linalg.eigvalsh.

  blockdiag96   six aligned 16x16 blocks: every cross Gram is exactly zero, only the within-super-block rotations act,
                and the columns they rotated must still be stored although neither round of the tick rotated
  diag96        nothing rotates at all: every workgroup leaves early and the image stays the input
  coupled128    diagonal but for one dense 32x32 block on super-blocks 2 and 5: the other workgroups leave early
  gauss160      the Rayleigh-Ritz shape: rows of 256 doubles with pad rows (and its leading 40 pairs, eigh_partial)
  plan_two_svd  two problems on one aligned schedule (6 and 10 players); the first has an exactly diagonal Gram and is
                finished after the first sweep, the second needs several: its `done` word must hold in every later tick
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "g17_tick_bits.json")
N_SAMPLES = 64


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def _grid_gram(rng, n, k):
    """a a^T of an n x k Gaussian factor rounded to a 2^-16 grid: every product and partial sum is an fp64 number, so the
    matrix does not depend on the order in which the host's BLAS adds."""
    a = np.round(rng.standard_normal((n, k)) * 2.0 ** 16) / 2.0 ** 16
    g = a @ a.T
    return 0.5 * (g + g.T)


def _matrix(name):
    rng = np.random.default_rng(_seed(name))
    if name == "blockdiag96":
        G = np.zeros((96, 96))
        for b in range(6):
            G[16 * b:16 * b + 16, 16 * b:16 * b + 16] = _grid_gram(rng, 16, 48)
        return G
    if name == "diag96":
        return np.diag(1.0 + rng.permutation(96) / 32.0)
    if name == "coupled128":
        G = np.diag(200.0 + rng.permutation(128) / 4.0)
        idx = np.concatenate([np.arange(32, 48), np.arange(80, 96)])
        G[np.ix_(idx, idx)] = _grid_gram(rng, 32, 96)
        return G
    if name == "gauss160":
        return _grid_gram(rng, 160, 480)
    raise ValueError(name)


def _eigh_case(name, matrix, r=None):
    import torch
    from tadmm import ops
    G = _matrix(matrix)
    g = torch.from_numpy(G).to("cuda:0")
    ev, vec, info = ops.eigh(g) if r is None else ops.eigh_partial(g, r)
    torch.cuda.synchronize()
    ev = ev.cpu().numpy()
    # eigenvalues, eigenvectors, and the sweep count (eigh) / the route (eigh_partial)
    out = np.concatenate([ev.ravel(), vec.cpu().numpy().ravel(), np.array([float(info)])])
    ref = np.linalg.eigvalsh(G)[::-1][:ev.size]
    return name, _sha(G), out, [(ev, ref)]


def _plan_case(name):
    """Two SVD layers through one ProjectionPlan (full solves of 96 and 160 columns in one group), two iterations with
    update_u=True: the singular values of the first iteration, the residuals, Z and U."""
    import torch
    from tadmm import ops
    from tadmm._cabi import KIND_SVD
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(_seed(name))
    w0 = np.zeros((96, 200), dtype=np.float32)
    w0[np.arange(96), 2 * np.arange(96)] = (1.0 + rng.permutation(96) / 64.0).astype(np.float32)   # W W^T is diagonal
    w1 = (0.1 * rng.standard_normal((160, 300))).astype(np.float32)
    ranks = [24, 40]
    layers = []
    for wh, r in zip((w0, w1), ranks):
        w = torch.from_numpy(wh).to(dev)
        layers.append(dict(kind=KIND_SVD, W=w, U=torch.zeros_like(w), Z=torch.zeros_like(w), ranks=r))
    plan = ops.ProjectionPlan(layers)
    parts, checks = [], []
    for it in range(2):
        res = plan.run(update_u=True)
        torch.cuda.synchronize()
        parts.append(res.detach().cpu().numpy().astype(np.float64).view(np.uint8))
        if it == 0:
            assert plan.filter_stats()["solves"] == 0, "the case is meant for full solves on the tournament kernels"
            for i, wh in enumerate((w0, w1)):
                sv = plan.singular_values(i, 0)
                parts.append(sv.view(np.uint8))
                w64 = wh.astype(np.float64)
                checks.append((sv * sv, np.linalg.eigvalsh(w64 @ w64.T)[::-1][:ranks[i]]))
    for L in layers:
        parts.append(L["Z"].cpu().numpy().view(np.uint8).ravel())
        parts.append(L["U"].cpu().numpy().view(np.uint8).ravel())
    plan.close()
    return name, _sha(w0, w1), np.concatenate([p.ravel() for p in parts]), checks


def cases():
    for m in ("blockdiag96", "diag96", "coupled128", "gauss160"):
        yield lambda m=m: _eigh_case("eigh_" + m, m)
    yield lambda: _eigh_case("eigh_partial_gauss160_r40", "gauss160", r=40)
    yield lambda: _plan_case("plan_two_svd_96_diagonal_160_gauss")


def samples(out):
    """64 evenly spaced entries of the flattened output, as (index, hex of the bytes) for diagnostics."""
    flat = np.ascontiguousarray(out).ravel()
    idx = np.unique(np.linspace(0, flat.size - 1, N_SAMPLES).astype(np.int64))
    return [[int(i), flat[i:i + 1].tobytes().hex()] for i in idx]


def main():
    commit = sys.argv[1] if len(sys.argv) > 1 else "unknown"
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "dnn-compression-tensor-admm_amd"))
    doc = {"commit": commit, "cases": {}}
    for make in cases():
        name, in_sha, out, checks = make()
        doc["cases"][name] = {"inputs_sha256": in_sha, "output_sha256": _sha(out), "dtype": str(out.dtype),
                              "numel": int(out.size), "samples": samples(out)}
        err = max(float(np.abs(ev - ref).max() / ref[0]) for ev, ref in checks)
        print(name, doc["cases"][name]["output_sha256"][:16], "eigenvalue error / lambda_max %.3g" % err, flush=True)
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
