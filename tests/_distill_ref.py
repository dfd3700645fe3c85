"""Float64 restatement of the distillation loss (csrc/distill.hip, include/tadmm.h), the case table of the device
tests, input builders and 16-bit misaligned views.  Everything here is torch on whatever device the inputs live on."""
import functools
import json
import os

import numpy as np
import torch

SENTINEL = 1234.5                # exact in float32, bfloat16 and float16; never produced by the cases
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
NO_IGNORE = -2 ** 63


def restate(s, k, t, target, *, base, kd, alpha=0.5, tau=1.0, smoothing=0.0, ignore_index=-100, grads=True):
    """(loss, grad_s, grad_k, kept, bad) in float64 from the formulas of include/tadmm.h; the gradients are with respect
    to s and k as SEPARATE tensors (a caller that passes one tensor for both adds them)."""
    f64 = lambda x: None if x is None else x.detach().to(torch.float64)
    s, k, t = f64(s), f64(k), f64(t)
    ref = s if base != "none" else k
    B, C = ref.shape
    if grads:
        s = None if s is None else s.requires_grad_(True)
        k = None if k is None else k.requires_grad_(True)
    kept, bad = B, 0
    base_v = None
    if base == "index":
        ign = NO_IGNORE if ignore_index is None else ignore_index
        valid = (target != ign) & (target >= 0) & (target < C)
        kept, bad = int(valid.sum()), int(((target != ign) & ~valid).sum())
        lp = s - torch.logsumexp(s, dim=1, keepdim=True)
        q = torch.zeros_like(lp)
        rows = torch.nonzero(valid).flatten()
        q[rows, target[rows]] = 1.0
        q = ((1 - smoothing) * q + smoothing / C) * valid.to(torch.float64).unsqueeze(1)
        base_v = -(q * lp).sum() / kept if kept else torch.full((), float("nan"), dtype=torch.float64, device=ref.device)
    elif base == "dense":
        lp = s - torch.logsumexp(s, dim=1, keepdim=True)
        q = (1 - smoothing) * target.to(torch.float64) + smoothing / C
        base_v = -(q * lp).sum() / B
    kd_v = None
    if kd == "hard":
        lk = k - torch.logsumexp(k, dim=1, keepdim=True)
        idx = torch.arange(C, device=t.device).expand(B, C)
        first = torch.where(t == t.max(dim=1, keepdim=True).values, idx, torch.full_like(idx, C)).min(dim=1).values
        kd_v = -lk.gather(1, first.unsqueeze(1)).sum() / B
    elif kd in ("soft", "soft_ce"):
        lt = t / tau - torch.logsumexp(t / tau, dim=1, keepdim=True)
        lk = k / tau - torch.logsumexp(k / tau, dim=1, keepdim=True)
        pt = lt.exp()
        kd_v = (pt * (lt - lk)).sum() * tau * tau / (B * C) if kd == "soft" else -(pt * lk).sum() / (B * C)
    if kd == "none":
        loss = base_v
    elif base == "none":
        loss = alpha * kd_v
    else:
        loss = (1 - alpha) * base_v + alpha * kd_v
    gs = gk = None
    if grads and bool(torch.isfinite(loss)):
        leaves = [x for x in (s if base != "none" else None, k if kd != "none" else None) if x is not None]
        got = list(torch.autograd.grad(loss, leaves, allow_unused=True))
        if base != "none":
            gs = got.pop(0)
            gs = torch.zeros_like(s) if gs is None else gs
        if kd != "none":
            gk = got.pop(0)
    return loss.detach(), gs, gk, kept, bad


# ---------------------------------------------------------------------------------------------- the device case table
SHAPES = [(1, 1), (1, 2), (3, 3), (4, 10), (5, 63), (5, 64), (5, 65), (64, 100), (257, 17), (33, 1000), (3, 1024),
          (3, 1025), (2, 4099)]
KDS = [("soft", 1.0), ("soft", 3.0), ("hard", 1.0), ("soft_ce", 2.0)]
BASES = [("index", 0.0), ("index", 0.1), ("dense", 0.0), ("none", 0.0)]


def _table():
    cases = []
    n = 0
    for shape in SHAPES:                 # every C with every type; kd and base kinds dealt round-robin
        for dt in DTYPES:
            kd, base = KDS[n % 4], BASES[(n // 4 + n) % 4]
            cases.append(dict(B=shape[0], C=shape[1], dtype=dt, kd=kd[0], tau=kd[1], base=base[0], eps=base[1]))
            n += 1
    for i, kd in enumerate(KDS):         # every (kd, base) pair at a size with a tail and two workgroups
        for j, base in enumerate(BASES):
            cases.append(dict(B=5, C=65, dtype=list(DTYPES)[(i + j) % 3], kd=kd[0], tau=kd[1], base=base[0], eps=base[1]))
    for j, base in enumerate(BASES[:3]):  # the base term alone
        cases.append(dict(B=64, C=100, dtype=list(DTYPES)[j], kd="none", tau=1.0, base=base[0], eps=base[1]))
        cases.append(dict(B=3, C=1025, dtype=list(DTYPES)[(j + 1) % 3], kd="none", tau=1.0, base=base[0], eps=base[1]))
    for c in cases:
        c["alpha"] = 0.5 if c["kd"] != "none" else 0.0
        c["id"] = "{B}x{C}-{dtype}-{kd}{tau:g}-{base}{eps:g}".format(**c)
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


CASES = _table()
CASE_BY_ID = {c["id"]: c for c in CASES}


def make_inputs(B, C, dtype, seed, base="index", scale=3.0, same=False, device="cpu"):
    """Seeded logits of `dtype` (generated on the host, so every machine sees the same values): s, k, t and the target
    of the base kind.  The teacher's row maximum is raised by one so that it is unique after rounding to `dtype`."""
    g = torch.Generator().manual_seed(seed)
    dt = DTYPES[dtype] if isinstance(dtype, str) else dtype
    s = (scale * torch.randn(B, C, generator=g)).to(dt)
    k = s if same else (scale * torch.randn(B, C, generator=g)).to(dt)
    t = scale * torch.randn(B, C, generator=g)
    top = t.argmax(dim=1, keepdim=True)
    t = t.scatter(1, top, t.gather(1, top).abs() + 1.0 + scale).to(dt)
    if base == "dense":
        target = torch.softmax(2.0 * torch.randn(B, C, generator=g), dim=1)
    else:
        target = torch.randint(0, C, (B,), generator=g)
    return tuple(x.to(device) for x in (s, k, t, target))


def case_inputs(case, device="cpu"):
    seed = sum(map(ord, case["id"]))
    return make_inputs(case["B"], case["C"], case["dtype"], seed, case["base"], device=device)


def case_kwargs(case):
    return dict(base=case["base"], kd=case["kd"], alpha=case["alpha"], tau=case["tau"], smoothing=case["eps"])


def teacher_ties(t):
    """Rows of t whose maximum occurs more than once."""
    return int(((t == t.max(dim=1, keepdim=True).values).sum(dim=1) > 1).sum())


# labels of the ignore / bad-label test: rows 1, 3 and 4 are dropped, 3 and 4 are counted
def label_case(C):
    return torch.tensor([0, -100, C - 1, C, -1, 1 % C, C // 2])


def ulp(x64, dtype):
    """One unit in the last place of `dtype` at the magnitude of every element of the float64 tensor x64 (the spacing
    of the subnormals below the smallest normal)."""
    bits, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}[dtype]
    _, e = torch.frexp(x64.abs())
    e = torch.clamp(e.to(torch.float64) - 1, min=emin)
    e = torch.where(x64 == 0, torch.full_like(e, emin), e)          # frexp(0) = (0, 0)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=x64.device), e - bits)


def workspace_bytes_by_hand(B):
    up = lambda v: (v + 255) // 256 * 256
    return up(16 * B) + up(4 * B)


# ------------------------------------------------------------------------------------------------- misaligned views
_GUARD = 16


def misaligned_rows(t, off_bytes, row_stride=None):
    """A (B, C) view equal to `t` (any of the three types) whose data_ptr() is `off_bytes` past a 16-byte boundary and
    whose row stride is `row_stride` elements (default C), cut out of a sentinel-filled 1-D buffer with guard elements
    on either side and, for wide strides, between the rows (`guards_intact`)."""
    es = t.element_size()
    assert off_bytes % es == 0 and 0 <= off_bytes < 16
    B, C = t.shape
    ld = C if row_stride is None else row_stride
    assert ld >= C
    n = (B - 1) * ld + C
    buf = torch.full((n + 2 * _GUARD + 16,), SENTINEL, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    start = _GUARD + off_bytes // es                 # _GUARD elements are whole 16-byte units in every type
    v = torch.as_strided(buf, (B, C), (ld, 1), start)
    v.copy_(t)
    assert v.data_ptr() % 16 == off_bytes, (v.data_ptr(), off_bytes)
    return v


def guards_intact(v):
    """True when every element of the buffer of `misaligned_rows(...)` outside the view still holds the sentinel."""
    base = v._base
    assert base is not None and base.dim() == 1
    mask = torch.ones(base.numel(), dtype=torch.bool, device=v.device)
    B, C = v.shape
    idx = v.storage_offset() + torch.arange(B, device=v.device).unsqueeze(1) * v.stride(0) + \
        torch.arange(C, device=v.device).unsqueeze(0)
    mask[idx.flatten()] = False
    return bool((base[mask] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ recorded reference
def golden_index(golden_dir):
    with open(os.path.join(golden_dir, "g15_distill.json")) as f:
        return json.load(f)["cases"]


@functools.lru_cache(maxsize=None)
def _golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "g15_distill.npz"))
    return {k: z[k] for k in z.files}


def recorded(golden_dir, name):
    z = _golden(golden_dir)
    return {k.split(".", 1)[1]: torch.from_numpy(v) for k, v in z.items() if k.startswith(name + ".")}


def recorded_kwargs(meta):
    """How a recorded case maps to the restatement: base kind and smoothing from the criterion, kd kind from the type."""
    crit = meta["criterion"]
    base = "dense" if crit == "ce_prob" else "index"
    kd = {"none": "none", "soft": "soft", "hard": "hard"}[meta["type"]]
    return dict(base=base, kd=kd, alpha=meta["alpha"], tau=meta["tau"], smoothing=0.1 if crit == "ce_ls" else 0.0)
