"""numpy restatement of the gathered TT-matrix chain and its core gradients, written from the formula.

Cores G_k (r_{k-1}, n_k, m_k, r_k), k = 1 .. d, r_0 = 1.  Token t carries an index in [0, n_1 ... n_d), split into
(i_1 .. i_d) with i_1 slowest.  With S_k = G_k[:, i_k, :, :]
    y[t][j_1 .. j_d, b] = sum_{a_1 .. a_{d-1}} S_1[0, j_1, a_1] S_2[a_1, j_2, a_2] ... S_d[a_{d-1}, j_d, b]
and the gradient of sum(y * dy) with respect to the slice of core k is
    dS_k[a, j_k, b] = sum L_k[j_<k, a] dy[j_<k, j_k, j_>k] R_k[b, j_>k]
with L_k / R_k the partial products to the left / right of mode k.  An index outside the range gives a zero row and no
gradient.  `dtype` is the type every product and sum is carried in (float64: the reference; float32: what a float32
implementation may at best be expected to give); tokens are added in ascending order.
"""
import numpy as np

# the shapes (n, m, r) every test of the embedding kernels runs
SHAPES = {
    "svd_row": ([7], [1], [1, 33]),
    "d2": ([3, 2], [2, 3], [1, 5, 1]),
    "d3": ([4, 3, 5], [3, 1, 5], [1, 17, 33, 1]),
    "d4": ([3, 2, 2, 3], [2, 1, 3, 2], [1, 4, 6, 5, 1]),
    "tt_in": ([5, 7, 3], [1, 1, 1], [1, 16, 20, 24]),
    "bert_ttm": ([32, 31, 31], [12, 8, 8], [1, 57, 57, 1]),
    "lds_last_fit": ([2, 2, 2], [32, 37, 2], [1, 16, 16, 1]),     # 163 088 of 163 840 bytes: the launch still takes it
    "lds_past": ([2, 2, 2], [32, 38, 2], [1, 16, 16, 1]),          # 167 440 bytes: composed route
}
TOKEN_SETS = ("one", "tile_plus_one", "random130", "last130", "ends", "transposed")


def make_cores(shape, seed=0, dtype=np.float32):
    n, m, r = shape
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((r[k], n[k], m[k], r[k + 1])) / np.sqrt(r[k])).astype(dtype) for k in range(len(n))]


def token_set(name, shape, tile, seed=0):
    """Index array of the named token set (int64; "transposed" is a 2-D array whose transpose the test views)."""
    total = int(np.prod(shape[0]))
    rng = np.random.default_rng(seed + 17)
    if name == "one":
        return rng.integers(0, total, size=1)
    if name == "tile_plus_one":
        return rng.integers(0, total, size=tile + 1)
    if name == "random130":
        return rng.integers(0, total, size=130)
    if name == "last130":
        return np.full(130, total - 1, dtype=np.int64)
    if name == "ends":
        idx = rng.integers(0, total, size=9)
        idx[2], idx[6] = 0, total - 1
        return idx
    if name == "transposed":
        return rng.integers(0, total, size=(5, 7))
    raise KeyError(name)


def split_index(index, n):
    """(B, d) mode indices, i_1 slowest, of a flat index array."""
    idx = np.asarray(index, dtype=np.int64).reshape(-1)
    cols, stride = [], int(np.prod(n))
    for v in n:
        stride //= int(v)
        cols.append((idx // stride) % int(v))
    return np.stack(cols, 1)


def groups(index, n):
    """Per mode: (order, offsets) of the tokens grouped by i_k, ascending token order inside a group."""
    ik = split_index(index, n)
    out = []
    for k, v in enumerate(n):
        order = np.argsort(ik[:, k], kind="stable")
        counts = np.bincount(ik[:, k], minlength=int(v))
        out.append((order, np.concatenate([[0], np.cumsum(counts)])))
    return out


def lds_bytes(n, m, r):
    """(forward bytes of one token, backward bytes) the launches should ask for, restated from the layout
    csrc/ttm_gather.hip documents, as an oracle for `ops.ttm_gather_plan`.  The running product after mode k
    has P_k r_k floats (P_k = m_1 ... m_k); the forward keeps the products of odd and of even k < d in two buffers, the
    backward adds two buffers for the right products (r_k Q_k floats, Q_k = m_{k+1} ... m_d r_d, 1 <= k < d), one for
    dY R (max_k P_k r_k floats) and 16 bytes of mode indices."""
    d = len(n)
    P, s, maxv = 1, [0, 0], 0
    for k in range(d):
        P *= m[k]
        e = P * r[k + 1]
        maxv = max(maxv, e)
        if k + 1 < d:
            s[(k + 1) & 1] = max(s[(k + 1) & 1], e)
    Q, maxr = r[d], 0
    for k in range(d - 1, 0, -1):
        Q *= m[k]
        maxr = max(maxr, Q * r[k])
    return 4 * (s[0] + s[1]), 16 + 4 * (s[0] + s[1] + 2 * maxr + maxv)


def _valid(index, n):
    idx = np.asarray(index, dtype=np.int64).reshape(-1)
    return (idx >= 0) & (idx < int(np.prod(n)))


def forward(cores, index, dtype=np.float64):
    """(B, m_1 ... m_d r_d) rows, in `dtype`."""
    cs = [np.asarray(c, dtype=dtype) for c in cores]
    n = [c.shape[1] for c in cs]
    idx = np.asarray(index, dtype=np.int64).reshape(-1)
    ok = _valid(idx, n)
    ik = split_index(np.where(ok, idx, 0), n)
    row = int(np.prod([c.shape[2] for c in cs])) * cs[-1].shape[3]
    y = np.zeros((idx.size, row), dtype=dtype)
    for t in range(idx.size):
        if not ok[t]:
            continue
        state = np.ones((1, 1), dtype=dtype)
        for k, c in enumerate(cs):
            s = c[:, ik[t, k]]                                   # r_{k-1} x m_k x r_k
            state = (state @ s.reshape(s.shape[0], -1)).reshape(-1, s.shape[2])
        y[t] = state.reshape(-1)
    return y


def backward(cores, index, dy, dtype=np.float64):
    """Gradients of sum(forward * dy) with respect to every core, in `dtype`."""
    cs = [np.asarray(c, dtype=dtype) for c in cores]
    d = len(cs)
    n = [c.shape[1] for c in cs]
    idx = np.asarray(index, dtype=np.int64).reshape(-1)
    ok = _valid(idx, n)
    ik = split_index(np.where(ok, idx, 0), n)
    dy = np.asarray(dy, dtype=dtype).reshape(idx.size, -1)
    grads = [np.zeros_like(c) for c in cs]
    for t in range(idx.size):
        if not ok[t]:
            continue
        sl = [c[:, ik[t, k]] for k, c in enumerate(cs)]
        left = [np.ones((1, 1), dtype=dtype)]                    # left[k]: (m_1 ... m_k) x r_k
        for s in sl[:-1]:
            left.append((left[-1] @ s.reshape(s.shape[0], -1)).reshape(-1, s.shape[2]))
        right = [None] * d                                       # right[k]: r_k x (m_{k+1} ... m_d r_d)
        right[d - 1] = np.eye(cs[-1].shape[3], dtype=dtype)
        for k in range(d - 1, 0, -1):
            s = sl[k]
            right[k - 1] = (s.reshape(-1, s.shape[2]) @ right[k]).reshape(s.shape[0], -1)
        for k in range(d):
            g = dy[t].reshape(left[k].shape[0], sl[k].shape[1], -1)
            grads[k][:, ik[t, k]] += np.einsum("pa,pjq,bq->ajb", left[k], g, right[k]).astype(dtype)
    return grads


def rel_err(a, ref):
    """max|a - ref| / max|ref|."""
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / (scale if scale > 0 else 1.0))
