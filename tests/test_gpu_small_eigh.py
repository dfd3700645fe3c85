"""The small eigen-solver routes (N <= 64: csrc/tridiag.hip, then jacobi_small_kernel for what it does not certify;
N > 64: the Jacobi tournament) against LAPACK in float64, on the spectra where such solvers go wrong.

Kernel level: `ops.eigh_partial(G, r)` on fp64 G built on the host, once with the default route and once with
TADMM_SMALL_DIRECT=0.  The reference is `numpy.linalg.eigh` of that same G.  Plan level: SVD, Tucker and TT
projections of fp32 weights with engineered singular values against the fp64 SVD of the rounded weights.

Conventions checked, not tolerated: eigenvalues are column norms of G V, i.e. |lambda|, in descending order; the
leading r of them are returned; rows whose eigenvalue is at most 1e-12 of the largest are exactly zero (kResidueCut).
"""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RESIDUE_CUT = 1e-12
# Bounds per route, relative to lambda_max; measured worst cases over the whole parametrisation in the comments.
# Direct route (csrc/tridiag.hip): backward stable, orthogonal to rounding whatever the spectrum.
TOL_EVAL = 1e-13        # |lambda_dev - lambda_ref|                        (measured 5.1e-14)
TOL_RESID = 5e-13       # ||G v - lambda v||                               (1.4e-13)
TOL_ORTH = 1e-13        # |V V^T - I| over the rows above the residue cut   (1.8e-15)
TOL_SUBSPACE = 1e-13    # ||P_dev - P_ref||_2 * gap                         (1.7e-15)
# Jacobi routes (jacobi_small_kernel, the tournament): the same bars for values and subspaces.  One-sided Jacobi takes
# v_j = x_j / |x_j| from X = G V, whose columns carry ~eps lambda_max of rounding each (jacobi.hip, "Convergence"), so a
# vector of a small eigenvalue is good to ~eps lambda_max / lambda_j only: residual and orthogonality bars are
# a + b lambda_max / lambda_j, with a the direct route's bar.  Measured: rows with lambda >= 1e-4 lambda_max 3.9e-14
# residual, 9e-16 orthogonality; rows near the residue cut lambda_j * residual / lambda_max <= 4.2e-16.
JAC_EVAL = 1e-12        # (3.9e-14)
JAC_RESID = (1e-12, 1e-14)
JAC_ORTH = (1e-11, 1e-13)
JAC_SUBSPACE = 1e-12
# Relaxed for one case only: a cluster of relative width 0 < delta <= 1e-9 on a Jacobi route.  Its stopping measure
# |x_i.x_j| / (|x_i||x_j|) sees a rotation theta inside the cluster only as ~2 theta delta, so at tol = 1e-9 the vectors
# inside such a cluster are resolved to O(1) angles; values and residuals then carry up to ~delta lambda.  Measured
# worst (five members at 1e-9, N = 5): eigenvalue 1.7e-12, residual 4.2e-11, orthogonality 4.5e-11.
TIGHT_EVAL, TIGHT_RESID, TIGHT_ORTH = 5e-12, 1e-10, 1e-10
SIZES = [1, 2, 3, 4, 5, 8, 31, 32, 33, 48, 63, 64, 65]
SPACINGS = [1e-2, 1e-4, 1e-6, 1e-9, 1e-12, 0.0]
DIRECT_MAX_N = 64
MAX_CLUSTER = 6         # kTMaxCluster: longer chains of close eigenvalues go to Jacobi by design
CLUSTER_TOL = 1e-3      # kTClusterTol, relative to the Gershgorin bound of the scaled tridiagonal


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ spectra
def _orth(n, rng):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def _sym(q, lam):
    g = (q * lam) @ q.T
    return 0.5 * (g + g.T)


def _ranks(n):
    return sorted({r for r in (1, max(1, n // 4), n - 3, n) if 1 <= r <= n})


def _geometric(n):
    return 0.75 ** np.arange(n)


def _with_cluster(n, start, m, spacing):
    lam = _geometric(n)
    c = lam[start]
    lam[start:start + m] = c * (1.0 - spacing * np.arange(m))
    return lam


def _cluster_starts(n, r, m):
    """Start index of an m-member cluster inside the leading r, straddling r, and entirely past r + 2."""
    out = {}
    if m <= r:
        out["inside"] = r - m
    if 1 <= r < n and m >= 2:
        s = max(0, r - m // 2)
        if s < r < s + m <= n:
            out["straddle"] = s
    if r + 2 + m <= n:
        out["past"] = r + 2
    return out


def _wilkinson_plus(n):
    h = (n - 1) / 2.0
    return np.diag(np.abs(np.arange(n) - h)) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)


def family_cases(family, n, r, seed):
    """(label, G, straddle) for one family, size and rank.  straddle: a cluster crosses the truncation (the leading-r
    subspace is not determined; only values, residuals and orthogonality are checked)."""
    rng = np.random.default_rng(seed)
    out = []
    if family == "geometric":
        out.append(("geometric", _sym(_orth(n, rng), _geometric(n)), False))
    elif family in ("cluster", "cluster_big", "cluster_scaled"):
        sizes = [2, 3, 4, 5, 6] if family != "cluster_big" else [7, 10]
        for i, sp in enumerate(SPACINGS if family != "cluster_big" else [1e-6, 0.0]):
            m = sizes[i % len(sizes)]
            for where, s in _cluster_starts(n, r, m).items():
                lam = _with_cluster(n, s, m, sp)
                sc = {"cluster": 1.0, "cluster_big": 1.0, "cluster_scaled": 1e-60}[family]
                out.append((f"m={m} sp={sp:g} {where}", _sym(_orth(n, rng), lam) * sc, where == "straddle"))
                if family == "cluster_scaled":
                    out.append((f"m={m} sp={sp:g} {where} x1e60", _sym(_orth(n, rng), lam) * 1e60, where == "straddle"))
    elif family == "graded":
        lam = 10.0 ** (-16.0 * np.arange(n) / max(n - 1, 1))
        out.append(("graded", _sym(_orth(n, rng), lam), False))
    elif family == "rank_deficient":
        for k in sorted({1, n - 3, n - 1}):
            if 1 <= k < n:
                a = rng.standard_normal((n, k)) * (0.8 ** np.arange(k))
                out.append((f"rank {k}", a @ a.T, False))
        if n >= 4:
            # a Gram accumulated in fp32: the null space carries rounding eigenvalues of either sign at ~1e-7
            a = rng.standard_normal((n, n - 3)) * (0.8 ** np.arange(n - 3))
            g32 = (a.astype(np.float32) @ a.astype(np.float32).T).astype(np.float64)
            out.append(("fp32 Gram, rank n-3", 0.5 * (g32 + g32.T), False))
    elif family == "split":
        perm = rng.permutation(n)
        out.append(("diagonal", np.diag(_geometric(n)[perm]), False))
        if n >= 2:
            h = n // 2
            blk = _sym(_orth(h, rng), 0.75 ** (2 * np.arange(h)))
            g = np.zeros((n, n))
            g[:h, :h] = blk
            g[h:2 * h, h:2 * h] = blk
            if n % 2:
                g[-1, -1] = 0.3 ** n        # below the shared spectrum
            # every eigenvalue of the block twice: exact multiplicities across the split; the pair straddles r when r is odd
            out.append(("two identical blocks", g, r % 2 == 1 and r < 2 * h))
    elif family == "wilkinson":
        w = _wilkinson_plus(n)
        w = w - (np.linalg.eigvalsh(w)[0] - 1e-3) * np.eye(n)
        # the top pairs agree to ~1e-14: a cluster straddles every odd r at the top
        lam = np.linalg.eigvalsh(w)[::-1]
        straddle = r < n and abs(lam[r - 1] - lam[r]) <= 1e-8 * lam[0]
        out.append(("W+ shifted", w, straddle))
    elif family == "scaled":
        for sc in (1e-60, 1e60):
            out.append((f"geometric x{sc:g}", _sym(_orth(n, rng), _geometric(n)) * sc, False))
    else:
        raise ValueError(family)
    return out


# Why a route other than the direct one is expected (the key is what expected_route returns as its reason)
BY_DESIGN = {
    "tournament": "N > 64: the Jacobi tournament kernels (the direct solver holds at most 64 columns)",
    "below direct": "N <= 2: below eig_small_direct_kernel (N < 3 returns at once), jacobi_small_kernel solves it",
    "zero": "zero matrix: the direct solver leaves it to Jacobi",
    "long chain": "a chain of more than kTMaxCluster = 6 eigenvalues among the leading r + 2, each within kTClusterTol "
                  "of the next (large clusters, exactly rank-deficient inputs, the tail of a geometric or graded "
                  "spectrum when r + 2 reaches it): Jacobi by design",
}


def expected_route(G, n, r):
    """(route, reason): route 0 / 1 / 2 when the design determines it, None when it does not (a chain of exactly
    kTMaxCluster members, or a chain whose length depends on where the Gershgorin bound of the tridiagonal falls).
    The reason of a fallback is a key of BY_DESIGN."""
    if n > DIRECT_MAX_N:
        return 2, "tournament"
    if n <= 2:
        return 1, "below direct"
    lam = np.linalg.eigvalsh(G)[::-1]
    rho = np.abs(lam).max()
    if not rho > 0:
        return 1, "zero"
    rw = min(n, r + 2)
    top = lam[:rw]

    def longest_chain(tol):
        run = best = 1
        for j in range(1, rw):
            run = run + 1 if top[j - 1] - top[j] <= tol else 1
            best = max(best, run)
        return best
    # the kernel's threshold is CLUSTER_TOL times its Gershgorin bound, which lies in [rho, 3 rho].  A cluster of exactly
    # MAX_CLUSTER members sits at the edge of the kernel's own checks (measured: one of 826 scaled six-member clusters at
    # 1e-12 spacing rejected, the solve then correct through Jacobi), so only shorter chains make route 0 certain
    if longest_chain(3.0 * CLUSTER_TOL * rho) < MAX_CLUSTER:
        return 0, "direct"
    if longest_chain(CLUSTER_TOL * rho) > MAX_CLUSTER:
        return 1, "long chain"
    return None, "undetermined"


# ------------------------------------------------------------------------------------------------ checks
def check_pairs(G, r, ev, vec, straddle, what, route=0, tight=False):
    """All assertions of one solve; returns the measured errors (relative to lambda_max, the residual and orthogonality
    ones before the Jacobi routes' 1 / lambda_j weighting).  tight: G has a cluster of relative width <= 1e-9."""
    direct = route == 0
    tight = tight and not direct
    n = G.shape[0]
    w, q = np.linalg.eigh(G)
    order = np.argsort(-np.abs(w), kind="stable")
    w, q = w[order], q[:, order]
    aw = np.abs(w)
    lmax = aw[0]
    assert ev.shape == (r,) and vec.shape == (r, n), what
    assert np.all(np.isfinite(ev)) and np.all(np.isfinite(vec)), what
    # values: the r largest of |eig(G)|, in descending order
    tol_e = TOL_EVAL if direct else (TIGHT_EVAL if tight else JAC_EVAL)
    e_err = np.abs(ev - aw[:r]).max() / lmax
    assert e_err <= tol_e, (what, "eigenvalues", e_err)
    assert np.all(np.diff(ev) <= 0), (what, "not descending")
    # leading, not just correct: no eigenvalue of G above the returned k-th beyond the k before it
    for k in range(r):
        assert np.count_nonzero(aw > ev[k] + tol_e * lmax) <= k, (what, "skipped eigenvalue", k)
    # residue rows: exactly zero; rows near the cut may go either way
    cut = RESIDUE_CUT * lmax
    kept = ev > cut
    residue = aw[:r] <= 0.1 * cut
    assert not np.any(vec[residue]), (what, "residue rows are not zero")
    sure = kept & (aw[:r] > 10.0 * cut)
    assert np.all(np.any(vec[sure] != 0.0, axis=1)), (what, "kept row is zero")
    live = kept & np.any(vec != 0.0, axis=1)
    V = vec[live]
    res = o_err = s_err = 0.0
    if V.shape[0]:
        lam_signed = np.einsum("ij,jk,ik->i", V, G, V)       # Rayleigh quotients carry the sign |lambda| drops
        R = G @ V.T - V.T * (np.sign(lam_signed) * ev[live])
        rj = np.linalg.norm(R, axis=0) / lmax
        O = np.abs(V @ V.T - np.eye(V.shape[0]))
        res, o_err = rj.max(), O.max()
        if direct:
            assert res <= TOL_RESID, (what, "residual", res)
            assert o_err <= TOL_ORTH, (what, "orthonormality", o_err)
        else:
            inv = lmax / ev[live]
            a_res, a_orth = (TIGHT_RESID, TIGHT_ORTH) if tight else (JAC_RESID[0], JAC_ORTH[0])
            bad = rj - (a_res + JAC_RESID[1] * inv)
            assert bad.max() <= 0.0, (what, "residual", res)
            bad = O - (a_orth + JAC_ORTH[1] * np.maximum.outer(inv, inv))
            assert bad.max() <= 0.0, (what, "orthonormality", o_err)
    # subspace of the leading r when the truncation is well posed
    k = int(np.count_nonzero(live))
    if not straddle and k == r and r < n and aw[r - 1] > 10.0 * cut:
        gap = aw[r - 1] - aw[r]
        if gap > 0.0:
            Pd = vec.T @ vec
            Pr = q[:, :r] @ q[:, :r].T
            s_err = np.linalg.norm(Pd - Pr, 2) * gap / lmax
            assert s_err <= (TOL_SUBSPACE if direct else JAC_SUBSPACE), (what, "subspace", s_err)
    return e_err, res, o_err, s_err


def solve(G, r, dev, direct):
    from tadmm import ops
    import os
    old = os.environ.get("TADMM_SMALL_DIRECT")
    try:
        if direct:
            os.environ.pop("TADMM_SMALL_DIRECT", None)
        else:
            os.environ["TADMM_SMALL_DIRECT"] = "0"
        ev, vec, route = ops.eigh_partial(torch.from_numpy(np.ascontiguousarray(G)).to(dev), r)
    finally:
        if old is None:
            os.environ.pop("TADMM_SMALL_DIRECT", None)
        else:
            os.environ["TADMM_SMALL_DIRECT"] = old
    return ev.cpu().numpy(), vec.cpu().numpy(), route


FAMILIES = ["geometric", "cluster", "cluster_big", "graded", "rank_deficient", "split", "scaled", "cluster_scaled"]


def _family_sizes(family):
    if family == "wilkinson":
        return [21, 33]
    return SIZES


def _tight(label):
    m = re.search(r"sp=([0-9.e+-]+)", label)
    return m is not None and 0.0 < float(m.group(1)) <= 1e-9


def run_family(dev, family, n, seed=0, both=True):
    """Every rank and case of one family at one size, the default route and (both) the one with the direct solver off.
    Returns [(label, r, route, expected route, errors of the default route, errors with the direct solver off)];
    errors = (eigenvalue, residual, orthonormality, subspace)."""
    out = []
    for r in _ranks(n):
        for label, G, straddle in family_cases(family, n, r, seed=1000 * n + 7 * r + seed):
            what = f"{family} N={n} r={r} {label}"
            tight = _tight(label)
            want, why = expected_route(G, n, r)
            ev, vec, route = solve(G, r, dev, direct=True)
            if want is not None:
                assert route == want, (what, "route", route, "expected", want, BY_DESIGN.get(why, why))
            errs = check_pairs(G, r, ev, vec, straddle, what + " [default]", route, tight)
            errs1 = None
            if both:
                ev1, vec1, route1 = solve(G, r, dev, direct=False)
                errs1 = check_pairs(G, r, ev1, vec1, straddle, what + " [TADMM_SMALL_DIRECT=0]", route1, tight)
                assert route1 == (2 if n > DIRECT_MAX_N else 1), (what, "route with the direct solver off", route1)
            out.append((label, r, route, want, errs, errs1))
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", FAMILIES)
def test_small_eigh_against_lapack(dev, family, n):
    run_family(dev, family, n)


@pytest.mark.parametrize("n", [21, 33])
def test_small_eigh_wilkinson(dev, n):
    run_family(dev, "wilkinson", n)


def test_direct_route_certifies_what_it_exists_for(dev):
    """The file must not pass by everything falling back: count the direct-route certifications of the families the
    direct solver is for (well separated, clusters of at most 6, split, Wilkinson, scaled) at sizes 3..64, on a second
    seed and the default route only.  Every case whose route the design determines is checked in run_family; here the
    share it leaves undetermined stays small, and route 0 carries most of the set (measured 376 of 544 = 69 %; the
    rest are BY_DESIGN["long chain"]: tails of the geometric spectra at r >= N - 3)."""
    total = direct = undetermined = 0
    cases = [(f, n) for f in ["geometric", "cluster", "split", "scaled"] for n in [3, 4, 5, 8, 31, 32, 33, 48, 63, 64]]
    for family, n in cases + [("wilkinson", 21), ("wilkinson", 33)]:
        for _, _, route, want, _, _ in run_family(dev, family, n, seed=1, both=False):
            total += 1
            direct += route == 0
            undetermined += want is None
    assert direct >= 0.65 * total, (direct, total)
    assert undetermined <= 0.05 * total, (undetermined, total)


def test_eigh_partial_rejects_bad_rank(dev):
    from tadmm import ops
    from tadmm._cabi import TadmmError
    G = torch.eye(5, dtype=torch.float64, device=dev)
    for r in (0, 6):
        with pytest.raises(TadmmError):
            ops.eigh_partial(G, r)
    ev, vec, route = ops.eigh_partial(G * 3.0, 5)
    assert route in (0, 1)
    np.testing.assert_allclose(ev.cpu().numpy(), 3.0, rtol=1e-14)
    v = vec.cpu().numpy()
    np.testing.assert_allclose(v @ v.T, np.eye(5), atol=1e-11)


# ------------------------------------------------------------------------------------------------ plan level
Z_BAR = 1e-5            # the project's bar: max |Z - Z_ref| <= 1e-5 max |W|


def _engineered(m, n, s, seed):
    """fp32 W = U diag(s) V^T (m x n) and its fp64 SVD after the fp32 rounding."""
    rng = np.random.default_rng(seed)
    k = len(s)
    u = _orth(m, rng)[:, :k]
    v = _orth(n, rng)[:, :k]
    w = ((u * s) @ v.T).astype(np.float32)
    uu, ss, vt = np.linalg.svd(w.astype(np.float64), full_matrices=False)
    return w, uu, ss, vt


def _truncated(uu, ss, vt, r):
    return (uu[:, :r] * ss[:r]) @ vt[:r]


def _gapped(k, r, seed_ratio=0.85):
    """Descending singular values with s_{r+1} / s_r = 0.6 (and a second 0.6 drop at r2 when given as a tuple)."""
    rs = r if isinstance(r, tuple) else (r,)
    s = seed_ratio ** np.arange(k)
    for q in rs:
        s[q:] *= 0.6
    return s


def _wilkinson_like(k, r):
    """Three pairs of singular values that agree to ~1e-14 at the top (squares of W21+'s top pairs), a drop at r."""
    w = np.linalg.eigvalsh(_wilkinson_plus(21))[::-1]
    top = np.sqrt(w[:r] / w[0])
    rest = top[-1] * 0.6 * 0.85 ** np.arange(k - r)
    return np.concatenate([top, rest])


def _cluster4(k, r, at=5, spacing=1e-9):
    s = _gapped(k, r)
    s[at:at + 4] = s[at] * (1.0 - spacing * np.arange(4))
    return s


def _svd_layers(dev, order):
    from tadmm._cabi import KIND_SVD
    specs = [
        ("clean", 48, 96, 12, _gapped(48, 12)),
        ("wilkinson-like", 40, 72, 6, _wilkinson_like(40, 6)),
        ("cluster of 4 kept", 56, 64, 16, _cluster4(56, 16)),
        ("rank 5 of 30, r 20", 30, 60, 20, 0.8 ** np.arange(5)),
        ("clean, n < m", 64, 33, 9, _gapped(33, 9)),
    ]
    out = []
    for i in order:
        name, m, n, r, s = specs[i]
        w, uu, ss, vt = _engineered(m, n, s, seed=100 + i)
        W = torch.from_numpy(w).to(dev)
        out.append(dict(name=name, r=r, ref=_truncated(uu, ss, vt, r), sv=ss, w=w,
                        layer=dict(kind=KIND_SVD, W=W, U=torch.zeros_like(W), Z=torch.empty_like(W), ranks=r)))
    return out


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))


def test_projection_plan_svd_layers_mixed_routes(dev, monkeypatch):
    from tadmm import ops
    order = [0, 1, 2, 3, 4]
    L = _svd_layers(dev, order)
    plan = ops.ProjectionPlan([x["layer"] for x in L])
    z_route = {}
    for route_env in ("1", "0"):
        monkeypatch.setenv("TADMM_SMALL_DIRECT", route_env)
        plan.run(update_u=False, use_u=False)
        z_route[route_env] = [x["layer"]["Z"].cpu().numpy() for x in L]
        for i, x in enumerate(L):
            z = z_route[route_env][i]
            err = np.abs(z - x["ref"]).max()
            assert err <= Z_BAR * np.abs(x["w"]).max(), (x["name"], route_env, err)
            sv = plan.singular_values(i, 0)
            big = x["sv"][:x["r"]] >= 1e-3 * x["sv"][0]
            np.testing.assert_allclose(sv[big], x["sv"][:x["r"]][big], rtol=0, atol=1e-10 * x["sv"][0],
                                       err_msg=f"{x['name']} TADMM_SMALL_DIRECT={route_env}")
    for i, x in enumerate(L):
        assert _rel(z_route["1"][i], z_route["0"][i].astype(np.float64)) <= 1e-6, x["name"]
    # U fixed: three runs, bitwise the same
    monkeypatch.delenv("TADMM_SMALL_DIRECT")
    zs = []
    for _ in range(3):
        plan.run(update_u=False, use_u=False)
        zs.append([x["layer"]["Z"].clone() for x in L])
    for a, b in zip(zs[0], zs[1]):
        assert torch.equal(a, b)
    for a, b in zip(zs[0], zs[2]):
        assert torch.equal(a, b)
    plan.close()
    # the same layers in another order: the per-problem words (skip, fast_done) follow the problem, not the slot
    order2 = [3, 0, 4, 2, 1]
    L2 = _svd_layers(dev, order2)
    plan2 = ops.ProjectionPlan([x["layer"] for x in L2])
    plan2.run(update_u=False, use_u=False)
    for j, i in enumerate(order2):
        z = L2[j]["layer"]["Z"].cpu().numpy()
        err = np.abs(z - L2[j]["ref"]).max()
        assert err <= Z_BAR * np.abs(L2[j]["w"]).max(), (L2[j]["name"], "reordered", err)
        assert _rel(z, zs[0][i].cpu().numpy().astype(np.float64)) <= 1e-6, (L2[j]["name"], "reordered")
    plan2.close()


def test_small_solver_routes_of_the_plan_layers(dev):
    """The SVD layers above are meant to mix routes.  The plan does not report the route of a layer, so this is
    inferred, not observed: the standalone entry point solves each layer's Gram (formed in fp64 on the host, not by the
    plan's Gram kernel) at the plan's rank and reports its route."""
    routes = {}
    for x in _svd_layers(dev, [0, 1, 2, 3, 4]):
        w = x["w"].astype(np.float64)
        G = w @ w.T if w.shape[0] <= w.shape[1] else w.T @ w
        ev, vec, route = solve(G, x["r"], dev, direct=True)
        check_pairs(G, x["r"], ev, vec, False, x["name"], route)
        routes[x["name"]] = route
    assert routes["clean"] == 0 and routes["cluster of 4 kept"] == 0 and routes["wilkinson-like"] == 0, routes
    assert routes["rank 5 of 30, r 20"] == 1, routes       # 17 rounding-level eigenvalues in one cluster


def _tucker_layers(dev):
    specs = [
        ("clean", 40, 24, [8, 8], _gapped(24, 8)),
        ("unequal ranks", 32, 48, [10, 6], _gapped(32, (6, 10))),
        ("cluster of 4 kept", 48, 40, [12, 12], _cluster4(40, 12, at=3, spacing=1e-6)),
        ("wilkinson-like", 30, 36, [6, 9], _wilkinson_like(30, 6) * np.where(np.arange(30) >= 9, 0.6, 1.0)),
    ]
    out = []
    for i, (name, m, n, rk, s) in enumerate(specs):
        s = np.sort(np.asarray(s, dtype=np.float64))[::-1]
        w, uu, ss, vt = _engineered(m, n, s, seed=200 + i)
        W = torch.from_numpy(w).to(dev)
        out.append(dict(name=name, ref=_truncated(uu, ss, vt, min(rk)), w=w,
                        layer=dict(W=W, U=torch.zeros_like(W), Z=torch.empty_like(W), ranks=rk)))
    return out


def _tucker_run(dev, monkeypatch, L, plan, route_env):
    monkeypatch.setenv("TADMM_SMALL_DIRECT", route_env)
    plan.run(update_u=False, use_u=False)
    return [x["layer"]["Z"].cpu().numpy() for x in L]


def test_tucker_plan_2d_layers_exact_reference_and_route_switches(dev, monkeypatch):
    from tadmm import ops
    L = _tucker_layers(dev)
    plan = ops.TuckerPlan([x["layer"] for x in L])
    seq = ["1", "0", "1", "0"]
    got = [_tucker_run(dev, monkeypatch, L, plan, e) for e in seq]
    plan.close()
    fresh = {}
    for e in ("1", "0"):
        Lf = _tucker_layers(dev)
        pf = ops.TuckerPlan([x["layer"] for x in Lf])
        fresh[e] = _tucker_run(dev, monkeypatch, Lf, pf, e)
        pf.close()
    for k, e in enumerate(seq):
        for i, x in enumerate(L):
            err = np.abs(got[k][i] - x["ref"]).max()
            assert err <= Z_BAR * np.abs(x["w"]).max(), (x["name"], k, e, err)
            # after a route change, HOOI's warm start must not reuse a stale image
            assert _rel(got[k][i], fresh[e][i].astype(np.float64)) <= 1e-6, (x["name"], "run", k, "route", e)


def test_tt_conv_first_unfolding_clustered(dev):
    from oracle import tt_oracle as O
    from tadmm import ops
    from tadmm._cabi import KIND_TT_CONV
    o, i, kh, kw, r1 = 32, 16, 3, 3, 10
    s = _cluster4(32, r1, at=2, spacing=1e-9)
    s[6] = s[7] * (1.0 + 1e-12)       # and a pair
    s = np.sort(s)[::-1]
    m0, _, _, _ = _engineered(o, kh * kw * i, s, seed=300)
    w = np.ascontiguousarray(O.conv_fold(m0.reshape(o, kh * kw, i), (o, i, kh, kw)))
    W = torch.from_numpy(w).to(dev)
    layer = dict(kind=KIND_TT_CONV, W=W, U=torch.zeros_like(W), Z=torch.empty_like(W), tt_shapes=[o, kh * kw, i],
                 ranks=[1, r1, i, 1])
    plan = ops.ProjectionPlan([layer])
    plan.run(update_u=False, use_u=False)
    ref = O.prune_conv_rank_tt(w.astype(np.float64), [o, kh * kw, i], [1, r1, i, 1])
    err = np.abs(layer["Z"].cpu().numpy() - ref).max()
    assert err <= Z_BAR * np.abs(w).max(), err
    plan.close()
