"""float64 numpy restatement of one Riemannian Adam step on the Stiefel manifold (tadmm.riemannian.StiefelAdam,
csrc/stiefel.hip), and the same step in float32 as the CPU yardstick.  The retraction is Householder
`numpy.linalg.qr` with the sign fix, not a Cholesky QR: it shares no algorithm with the code under test.

Per factor X (n x p), gradient G, first moment M (laid out like X), ONE second moment v per factor, its running maximum
vmax (amsgrad) and the factor's own step counter t:
    t' = t + 1;   g = G + wd X;   r = g - X sym(X^T g);   s = sum r^2
    M' = b1 M + (1 - b1) r;   v' = b2 v + (1 - b2) s;   u = amsgrad ? max(vmax, v') : v'
    Y = X - lr / ((1 - b1^t') (sqrt(u / (1 - b2^t')) + eps)) M';   X+ = qr_pos(Y);   M+ = M' - X+ sym(X+^T M')
"""
import numpy as np
import torch

from _stiefel_ref import orth_error, qr_pos, sym  # noqa: F401  (re-exported for the tests)


def tangent(x, g, weight_decay=0.0):
    """r of the step above, float64."""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64) + weight_decay * x
    return g - x @ sym(x.T @ g)


def pre_retraction(x, g, m, v, vmax, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False):
    """(Y, M', v', u, t') in float64: everything of the step before the retraction."""
    b1, b2 = betas
    x = np.asarray(x, dtype=np.float64)
    r = tangent(x, g, weight_decay)
    s = float((r * r).sum())
    t = int(t) + 1
    m = b1 * np.asarray(m, dtype=np.float64) + (1.0 - b1) * r
    v = b2 * float(v) + (1.0 - b2) * s
    u = max(float(vmax), v) if amsgrad else v
    c1, c2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    y = x - lr / (c1 * (np.sqrt(u / c2) + eps)) * m
    return y, m, v, u, t


def step(x, g, m, v, vmax, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False):
    """Returns (X+, M+, v+, vmax+, t+) in float64 (t+ an int); vmax+ is vmax unchanged without amsgrad."""
    y, m, v, u, t = pre_retraction(x, g, m, v, vmax, t, lr, betas, eps, weight_decay, amsgrad)
    xn = qr_pos(y)
    m = m - xn @ sym(xn.T @ m)
    return xn, m, v, (u if amsgrad else float(vmax)), t


def step_f32(x, g, m, v, vmax, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False):
    """The same step with every array and every product in float32 and Householder QR in float32 (the scalars of the
    bias correction are Python floats): what plain single precision leaves, the yardstick the device is held to."""
    f = np.float32
    b1, b2 = betas
    x = np.asarray(x, dtype=f)
    g = np.asarray(g, dtype=f) + f(weight_decay) * x
    a = x.T @ g
    r = g - x @ (f(0.5) * (a + a.T))
    s = f((r * r).sum(dtype=f))
    t = int(t) + 1
    m = f(b1) * np.asarray(m, dtype=f) + f(1.0 - b1) * r
    v = f(b2) * f(v) + f(1.0 - b2) * s
    u = max(f(vmax), v) if amsgrad else v
    c1, c2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    y = x - f(lr / (c1 * (np.sqrt(float(u) / c2) + eps))) * m
    # (numpy.linalg.qr would factor a float32 matrix in double precision; torch's runs LAPACK's single-precision routine)
    q, rr = (a.numpy() for a in torch.linalg.qr(torch.from_numpy(np.ascontiguousarray(y, dtype=f))))
    sg = np.sign(np.diag(rr)).astype(f)
    sg[sg == 0] = 1.0
    xn = (q * sg[None, :]).astype(f)
    b = xn.T @ m
    m = m - xn @ (f(0.5) * (b + b.T))
    return xn, m.astype(f), f(v), (f(u) if amsgrad else f(vmax)), t
