"""float64 references and DERIVED elementwise error bounds for the 16-bit chain kernels (shared by the test_gpu_fp16_*
files).  Operands are the values the kernel multiplies: x as given, the weights as rounded into their one plane.

With u the unit roundoff of the 16-bit type (2^-11 binary16, 2^-8 bfloat16) and every product of absolute values taken
in float64, a chain of products with fp32 accumulation of n terms in an unknown order, one rounding of each intermediate
kept in 16 bits and one rounding of the output obeys

    |y - ref| <= 1.5 * [ u * (|ref| + sum over intermediates of |later factors| . |intermediate|)
                         + n * 2^-24 * (|all factors| . |x| + |bias|) ]

(1.5 covers the second-order terms).  Nothing here is fitted to what a kernel returns."""
import torch
import torch.nn.functional as F

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
ACC = 2.0 ** -24


def bits(t):
    return t.contiguous().view(torch.int16)


def linear_ref(x, ws, bias):
    """x (T, K) through the factors ws = [W1 (R, K), W2 (N, R)] or [W]: (ref, bound / u-independent parts) in float64."""
    x = x.double()
    ws = [w.double() for w in ws]
    b = bias.double() if bias is not None else torch.zeros(ws[-1].shape[0], dtype=torch.float64, device=x.device)
    n_terms = sum(w.shape[1] for w in ws)
    if len(ws) == 1:
        ref = x @ ws[0].t() + b
        mid = torch.zeros_like(ref)
        allabs = x.abs() @ ws[0].abs().t() + b.abs()
    else:
        h = x @ ws[0].t()
        ref = h @ ws[1].t() + b
        mid = h.abs() @ ws[1].abs().t()
        allabs = (x.abs() @ ws[0].abs().t()) @ ws[1].abs().t() + b.abs()
    return ref, mid, allabs, n_terms


def linear_bound(x, ws, bias, dtype):
    ref, mid, allabs, n = linear_ref(x, ws, bias)
    return ref, 1.5 * (U[dtype] * (ref.abs() + mid) + n * ACC * allabs)


def image_rows(x):
    """(B, C, H, W) -> (B*H*W, C)."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def rows_image(y, B, H, W):
    return y.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def conv_bound(x, w1, core, w3, bias, stride, padding, dilation, dtype):
    """1x1 -> k x k -> 1x1 + bias on an NCHW image: (ref, bound), float64, every term by F.conv2d on absolute values."""
    x = x.double()
    w1, core, w3 = (w.double() for w in (w1, core, w3))
    b = bias.double() if bias is not None else torch.zeros(w3.shape[0], dtype=torch.float64, device=x.device)
    k1, k3 = w1[:, :, None, None], w3[:, :, None, None]
    h1 = F.conv2d(x, k1)
    h2 = F.conv2d(h1, core, None, stride, padding, dilation)
    ref = F.conv2d(h2, k3, b)
    t_h2 = F.conv2d(h2.abs(), k3.abs())                                                      # |W3| |H2|
    t_h1 = F.conv2d(F.conv2d(h1.abs(), core.abs(), None, stride, padding, dilation), k3.abs())  # |W3| |Wc| (*) |H1|
    allabs = F.conv2d(F.conv2d(F.conv2d(x.abs(), k1.abs()), core.abs(), None, stride, padding, dilation), k3.abs(), b.abs())
    n = w1.shape[1] + core.shape[1] * core.shape[2] * core.shape[3] + w3.shape[1]
    return ref, 1.5 * (U[dtype] * (ref.abs() + t_h2 + t_h1) + n * ACC * allabs)


def report(name, y, ref, bound):
    """Prints the measured figures, then asserts the bound elementwise."""
    err = (y.double() - ref).abs()
    worst = (err / bound).max().item()
    rel = err.max().item() / ref.abs().max().item()
    print(f"fp16 {name}: max err / max|ref| {rel:.3e}, worst err / bound {worst:.3f}")
    assert torch.isfinite(y.float()).all(), name
    assert worst <= 1.0, (name, worst, rel)
    return rel
