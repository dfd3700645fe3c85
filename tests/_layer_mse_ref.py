"""Float64 restatement of TinyBERT's intermediate-layer losses (csrc/layermse.hip, include/tadmm.h), the inputs and the
case table of the device tests, and the recorded reference runs (G20).  No GPU is needed to import or evaluate this."""
import functools
import json
import os

import numpy as np
import torch

DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
MASK = -10000.0


def _as_list(x):
    if x is None:
        return []
    return [x] if isinstance(x, torch.Tensor) else list(x)


def restate(student_atts, teacher_atts, student_reps, teacher_reps, threshold=-100.0, reduction="batch_sum",
            att_weights=None, rep_weights=None):
    """(att_loss, rep_loss, terms, grads) in float64 from the formulas of include/tadmm.h, on the device of the inputs:
    every value widened to float64 (exact), s' = 0 where s <= threshold, the same for t, d = s' - t', term = c sum d^2
    with c = w B / numel ("batch_sum") or w / numel ("mean"), gradient 2 c d and zero where s was clamped.  terms and
    grads list the attention pairs first."""
    out, terms, grads = [], [], []
    for k, (ss, ts, ws) in enumerate(((student_atts, teacher_atts, att_weights), (student_reps, teacher_reps, rep_weights))):
        ss, ts = _as_list(ss), _as_list(ts)
        ws = [1.0] * len(ss) if ws is None else ([float(ws)] * len(ss) if isinstance(ws, (int, float)) else list(ws))
        total = torch.zeros((), dtype=torch.float64, device=ss[0].device if ss else None)
        for s, t, w in zip(ss, ts, ws):
            s64, t64 = s.detach().to(torch.float64), t.detach().to(torch.float64)
            c = w * (s.shape[0] if reduction == "batch_sum" else 1) / s.numel()
            cs = (s64 <= threshold) if (k == 0 and threshold is not None) else torch.zeros_like(s64, dtype=torch.bool)
            ct = (t64 <= threshold) if (k == 0 and threshold is not None) else cs
            d = torch.where(cs, torch.zeros_like(s64), s64) - torch.where(ct, torch.zeros_like(t64), t64)
            term = c * (d * d).sum()
            terms.append(term)
            grads.append(torch.where(cs, torch.zeros_like(d), 2.0 * c * d))
            total = total + term
        out.append(total)
    return out[0], out[1], terms, grads


def ulp(x64, dtype):
    """One unit in the last place of `dtype` at the magnitude of every element of the float64 tensor x64 (the spacing
    of the subnormals below the smallest normal)."""
    bits, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}[dtype]
    _, e = torch.frexp(x64.abs())
    e = torch.clamp(e.to(torch.float64) - 1, min=emin)
    e = torch.where(x64 == 0, torch.full_like(e, emin), e)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=x64.device), e - bits)


def workspace_bytes_by_hand(numels, chunk, max_blocks):
    """One double per pair and workgroup; min(chunks, max_blocks) workgroups; rounded up to 256 bytes."""
    chunks = sum((n + chunk - 1) // chunk for n in numels)
    return (min(chunks, max_blocks) * len(numels) * 8 + 255) // 256 * 256


# ----------------------------------------------------------------------------------------------------------- inputs
def suffix_mask(B, S, kept):
    """(B, 1, 1, S): 0 over the first kept[b] keys of sample b, -10000 over the rest."""
    m = torch.zeros(B, 1, 1, S)
    for b, n in enumerate(kept):
        m[b, 0, 0, n:] = MASK
    return m


def att_pair(B, H, S, seed, dtype="float32"):
    """Student and teacher scores (B, H, S, S) = randn + suffix mask.  About 30 % of the keys are masked; in even samples
    the student masks one key more than the teacher, in odd samples one key fewer (so B >= 2 has elements clamped on
    either side alone)."""
    g = torch.Generator().manual_seed(seed)
    base = max(1, (3 * S + 5) // 10)
    ks = [max(0, S - base - (1 if b % 2 == 0 else 0)) for b in range(B)]
    kt = [max(0, S - base - (0 if b % 2 == 0 else 1)) for b in range(B)]
    s = torch.randn(B, H, S, S, generator=g) + suffix_mask(B, S, ks)
    t = torch.randn(B, H, S, S, generator=g) + suffix_mask(B, S, kt)
    return s.to(DTYPES[dtype]), t.to(DTYPES[dtype])


def flat_pair(n, seed, dtype="float32", batch=1):
    """Student and teacher scores (batch, n / batch) of n elements in all: randn, with a quarter of the elements at -10000
    + randn in each; the two masked windows overlap by half, so that (n >= 8) some elements are clamped in the student
    alone and some in the teacher alone."""
    assert n % batch == 0
    g = torch.Generator().manual_seed(seed)
    s, t = torch.randn(n, generator=g), torch.randn(n, generator=g)
    m = max(1, n // 4) if n > 1 else 0
    d = max(1, m // 2) if n >= 8 else 0
    s[n - m:] += MASK
    t[n - m - d:n - d] += MASK
    return s.view(batch, -1).to(DTYPES[dtype]), t.view(batch, -1).to(DTYPES[dtype])


def rep_pair(shape, seed, dtype="float32"):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DTYPES[dtype]), torch.randn(*shape, generator=g).to(DTYPES[dtype])


def clamp_census(s, t, threshold=-100.0):
    """(share of student elements clamped, clamped in the student alone, clamped in the teacher alone)."""
    cs, ct = s.double() <= threshold, t.double() <= threshold
    return float(cs.double().mean()), int((cs & ~ct).sum()), int((ct & ~cs).sum())


def shape_cases(chunk, max_blocks):
    """The attention-side cases of tests/test_gpu_layer_mse.py that can break the decomposition into chunks, as
    (id, [element counts or 4-d shapes of the attention pairs]); sizes come from the library's geometry."""
    return [
        ("one", [1]), ("chunk-1", [chunk - 1]), ("chunk", [chunk]), ("chunk+1", [chunk + 1]),
        ("odd-tail", [(3, 2, 37, 37)]),
        ("one-between", [2 * chunk + 5, 1, 3 * chunk - 7]),
        ("pairs-9", [(2, 2, 9, 9)] * 4 + [chunk + 3] * 5),
        ("pairs-32", [(2, 1, 7, 7)] * 31 + [chunk + 9]),
        ("second-trip", [max_blocks * chunk + chunk + 3]),
    ]


def case_pairs(spec, seed, dtype="float32"):
    """The student and teacher lists of one `shape_cases` entry."""
    ss, ts = [], []
    for i, item in enumerate(spec):
        s, t = att_pair(*item[:3], seed + i, dtype) if isinstance(item, tuple) else flat_pair(item, seed + i, dtype)
        ss.append(s)
        ts.append(t)
    return ss, ts


def offset_view(t, off_elems):
    """A contiguous view equal to `t` that starts `off_elems` elements into a 16-byte aligned buffer."""
    buf = torch.empty(t.numel() + off_elems + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[off_elems:off_elems + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (off_elems * t.element_size()) % 16
    return v


# ------------------------------------------------------------------------------------------------ recorded reference
def golden_index(golden_dir):
    with open(os.path.join(golden_dir, "g20_layer_mse.json")) as f:
        return json.load(f)["cases"]


@functools.lru_cache(maxsize=None)
def _golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "g20_layer_mse.npz"))
    return {k: z[k] for k in z.files}


def recorded(golden_dir, name):
    z = _golden(golden_dir)
    return {k.split(".", 1)[1]: torch.from_numpy(v) for k, v in z.items() if k.startswith(name + ".")}
