"""float64 numpy restatement of one Riemannian SGD step on the Stiefel manifold (tadmm.riemannian, csrc/stiefel.hip).
The retraction is Householder `numpy.linalg.qr` with the sign fix, not a Cholesky QR: it shares no algorithm with the
code under test."""
import numpy as np


def sym(a):
    return 0.5 * (a + a.T)


def qr_pos(y):
    """Q of the QR decomposition of y whose R has a positive diagonal (unique for a full-rank y)."""
    q, r = np.linalg.qr(np.asarray(y, dtype=np.float64))
    s = np.sign(np.diag(r))
    s[s == 0] = 1.0
    return q * s[None, :]


def step(x, g, m, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """Returns (X+, M+) in float64; M+ is m (as float64) when momentum == 0."""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64) + weight_decay * x
    m = None if m is None else np.asarray(m, dtype=np.float64)
    r = g - x @ sym(x.T @ g)
    if momentum > 0:
        m = momentum * m + (1.0 - dampening) * r
        d = r + momentum * m if nesterov else m
    else:
        d = r
    xn = qr_pos(x - lr * d)
    if momentum > 0:
        m = m - xn @ sym(xn.T @ m)
    return xn, m


def orth_error(x):
    """max |X^T X - I| in float64."""
    x = np.asarray(x, dtype=np.float64)
    return float(np.abs(x.T @ x - np.eye(x.shape[1])).max())
