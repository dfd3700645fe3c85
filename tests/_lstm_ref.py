"""Reference side of the TT-LSTM tests: the case table, seeded inputs that reach saturation, the step loop of
ablation/tt_lstm_inference.py:44-77 restated with torch on the CPU in float64 and float32, and the hand count of what
the launch takes.  Nothing here touches the device or the library.

Error measure everywhere: max|a - ref| / max|ref| per tensor.  `e32(case, gate)` is that error of the float32
restatement against the float64 one; the device tests allow `bar(e) = max(4 e, 2e-6)`."""
import functools

import numpy as np
import torch

# name: (T, B, in_tt, out_tt, ranks, seed).  tt_shapes of the layer = [4 * out_tt[0], out_tt[1:], in_tt]
# (tt_lstm_inference.py:31-32).  The seed is part of the case: `saturation(case)` must hold for it (asserted in
# tests/test_lstm_host_cpu.py), a property of the float64 reference alone; of seeds 0 .. 3 each case has the first whose
# smallest distance from +-3 is above 5e-5.
CASES = {
    "odd": (5, 3, (3, 4, 5), (2, 3, 4), (1, 3, 4, 5, 4, 3, 1), 0),
    "two_wg": (7, 17, (4, 5, 6), (4, 4, 4), (1, 4, 8, 8, 6, 4, 1), 1),
    "b1": (6, 1, (5, 7, 9), (4, 8, 8), (1, 2, 2, 4, 2, 2, 1), 0),
    "ucf11": (6, 16, (8, 20, 20, 18), (4, 8, 8), (1, 4, 8, 16, 8, 4, 4, 1), 3),
    "long": (64, 2, (4, 4), (4, 4), (1, 4, 4, 4, 1), 1),
}
GATES = ("hardsigmoid", "sigmoid")
KERNEL_TENSORS = ("y", "hT", "cT", "dXp", "dWhh", "dbias", "dh0", "dc0")


def tt_shapes(case):
    _, _, in_tt, out_tt, _, _ = CASES[case]
    return [4 * out_tt[0]] + list(out_tt[1:]) + list(in_tt)


def sizes(case):
    T, B, in_tt, out_tt, _, _ = CASES[case]
    return T, B, int(np.prod(in_tt)), int(np.prod(out_tt))


def recover(cores):
    """core_0 (core_1 (...)) left to right: the (4H * in) entries of the dense input map, output modes slowest."""
    w = cores[0].reshape(-1, cores[0].shape[-1])
    for c in cores[1:]:
        w = w.reshape(-1, c.shape[0]) @ c.reshape(c.shape[0], -1)
    return w


@functools.lru_cache(maxsize=None)
def inputs(case):
    """Seeded float32 inputs of a case as numpy arrays.  The recovered W_ih has standard deviation 1.5 / sqrt(in) (x is
    N(0, 1), so the input pre-activations have standard deviation about 1.5 and a good share of them lies beyond the
    Hardsigmoid's +-3); Whh is uniform in +-2 / sqrt(H); bias, h0, c0 are 0.5 N(0, 1).  dy, dhT, dcT are N(0, 1)."""
    T, B, n_in, H = sizes(case)
    ranks, seed = CASES[case][4], CASES[case][5]
    rng = np.random.default_rng(1000 + seed)
    shapes = tt_shapes(case)
    cores = [rng.standard_normal((ranks[i], shapes[i], ranks[i + 1])) for i in range(len(shapes))]
    w = recover(cores)
    cores[0] = cores[0] * (1.5 / (w.std() * np.sqrt(n_in)))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    d = {
        "cores": [f32(c) for c in cores],
        "x": f32(rng.standard_normal((T, B, n_in))),
        "w_hh": f32(rng.uniform(-2 / np.sqrt(H), 2 / np.sqrt(H), (4 * H, H))),
        "bias": f32(0.5 * rng.standard_normal(4 * H)),
        "h0": f32(0.5 * rng.standard_normal((B, H))),
        "c0": f32(0.5 * rng.standard_normal((B, H))),
        "dy": f32(rng.standard_normal((T, B, H))),
        "dhT": f32(rng.standard_normal((B, H))),
        "dcT": f32(rng.standard_normal((B, H))),
    }
    # the float32 pre-activations the kernel-level tests feed the recurrence: the float64 input map, rounded once
    w64 = recover([c.astype(np.float64) for c in d["cores"]]).reshape(4 * H, n_in)
    d["xp"] = f32(d["x"].astype(np.float64) @ w64.T + d["bias"].astype(np.float64))
    return d


def _gate(z, gate):
    return torch.sigmoid(z) if gate == "sigmoid" else torch.nn.functional.hardsigmoid(z)


def step_loop(xp, w_hh, h, c, gate, keep_z=None):
    """tt_lstm_inference.py:61-77 over a sequence: (y, h_T, c_T) from the pre-activations xp (T, B, 4H)."""
    H = w_hh.shape[1]
    ys = []
    for t in range(xp.shape[0]):
        z = xp[t] + h @ w_hh.t()
        if keep_z is not None:
            keep_z.append(z.detach())
        i, f, o = _gate(z[:, :H], gate), _gate(z[:, H:2 * H], gate), _gate(z[:, 3 * H:], gate)
        c = f * c + i * torch.tanh(z[:, 2 * H:3 * H])
        h = o * torch.tanh(c)
        ys.append(h)
    return torch.stack(ys), h, c


def _np(t):
    return t.detach().double().numpy()


@functools.lru_cache(maxsize=None)
def kernel_reference(case, gate, dtype=torch.float64):
    """The recurrence alone, from the float32 `xp` of `inputs(case)`: outputs and the gradients of
    sum(y dy) + sum(hT dhT) + sum(cT dcT), as float64 numpy arrays (computed in `dtype`)."""
    d = inputs(case)
    leaf = lambda a: torch.from_numpy(a).to(dtype).requires_grad_(True)
    xp, w, h0, c0 = leaf(d["xp"]), leaf(d["w_hh"]), leaf(d["h0"]), leaf(d["c0"])
    y, hT, cT = step_loop(xp, w, h0, c0, gate)
    co = lambda a: torch.from_numpy(a).to(dtype)
    ((y * co(d["dy"])).sum() + (hT * co(d["dhT"])).sum() + (cT * co(d["dcT"])).sum()).backward()
    return {"y": _np(y), "hT": _np(hT), "cT": _np(cT), "dXp": _np(xp.grad), "dWhh": _np(w.grad),
            "dbias": _np(xp.grad.sum((0, 1))), "dh0": _np(h0.grad), "dc0": _np(c0.grad)}


@functools.lru_cache(maxsize=None)
def layer_reference(case, gate, dtype=torch.float64):
    """The whole layer from x and the TT cores: outputs, and the gradients of the same scalar with respect to the cores,
    the recurrent weight and the bias."""
    d = inputs(case)
    T, B, n_in, H = sizes(case)
    leaf = lambda a: torch.from_numpy(a).to(dtype).requires_grad_(True)
    cores = [leaf(c) for c in d["cores"]]
    w, b = leaf(d["w_hh"]), leaf(d["bias"])
    co = lambda a: torch.from_numpy(a).to(dtype)
    w_ih = recover(cores).reshape(4 * H, n_in)
    xp = (co(d["x"]).reshape(T * B, n_in) @ w_ih.t() + b).reshape(T, B, 4 * H)
    y, hT, cT = step_loop(xp, w, co(d["h0"]), co(d["c0"]), gate)
    ((y * co(d["dy"])).sum() + (hT * co(d["dhT"])).sum() + (cT * co(d["dcT"])).sum()).backward()
    out = {"y": _np(y), "hT": _np(hT), "cT": _np(cT), "dWhh": _np(w.grad), "dbias": _np(b.grad)}
    for k, c in enumerate(cores):
        out[f"dcore{k}"] = _np(c.grad)
    return out


def rel_err(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def e32(case, gate, level="kernel"):
    """{tensor: error of the float32 restatement against the float64 one}."""
    fn = kernel_reference if level == "kernel" else layer_reference
    ref, f32 = fn(case, gate, torch.float64), fn(case, gate, torch.float32)
    return {k: rel_err(f32[k], ref[k]) for k in ref}


def bar(e: float) -> float:
    """Allowed device error for a tensor whose float32 restatement is `e` from float64: 4 e covers another accumulation
    order, the three dropped plane products (<= 2^-23 each) and a tanh a few ulp from libm's; 2e-6 is the floor."""
    return max(4.0 * e, 2e-6)


@functools.lru_cache(maxsize=None)
def saturation(case):
    """(share of the Hardsigmoid pre-activations beyond +-3, smallest distance of one of them from +-3), float64."""
    d = inputs(case)
    H = d["w_hh"].shape[1]
    t64 = lambda a: torch.from_numpy(a).double()
    zs = []
    step_loop(t64(d["xp"]), t64(d["w_hh"]), t64(d["h0"]), t64(d["c0"]), "hardsigmoid", keep_z=zs)
    z = torch.stack(zs)
    z = torch.cat([z[..., :2 * H], z[..., 3 * H:]], -1).abs()
    return float((z > 3).double().mean()), float((z - 3).abs().min())


# ---- what the launch takes, counted by hand from the scheme of csrc/lstm.hip
ROWS, WAVES, MAX_TPW, PAD = 16, 4, 4, 8
MAX_H = 16 * WAVES * MAX_TPW


def plan_by_hand(H):
    """(fits, LDS bytes of the larger launch, rows per workgroup).  Forward: h as 3 bf16 planes of 16 rows, twice, each row
    ceil32(H) + 8 elements.  Backward: dz as 3 planes of 16 rows of 4 ceil16(H) + 8 elements.  Both: a staging area of
    16 rows of (16 tiles-per-wave + 4) floats for each of the 4 waves; tiles per wave are 1, 2 or 4."""
    if H > MAX_H:
        return False, 0, ROWS
    Hp, Kp = -(-H // 16) * 16, -(-H // 32) * 32
    need = -(-(Hp // 16) // WAVES)
    tpw = 1 if need <= 1 else 2 if need <= 2 else 4
    stage = WAVES * ROWS * (16 * tpw + 4) * 4
    fwd = 2 * 3 * ROWS * (Kp + PAD) * 2 + stage
    bwd = 3 * ROWS * (4 * Hp + PAD) * 2 + stage
    return max(fwd, bwd) <= 160 * 1024, max(fwd, bwd), ROWS


# ---- the recorded runs of the reference's own lstm_step (tests/golden/g11_tt_lstm.npz)
RECORDED = ("r_odd", "r_wide", "r_b1")


def recorded(golden_dir, name):
    """One recorded case as a dict of numpy arrays: x, h0, c0, w_hh, bias, cores, tt_shapes, ranks, y, cT."""
    import os
    z = np.load(os.path.join(golden_dir, "g11_tt_lstm.npz"))
    d = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + ".")}
    d["cores"] = [d.pop(f"core{k}") for k in range(len(d["tt_shapes"]))]
    return d


def restate_recorded(d, dtype=torch.float64):
    """(y, c_T) of the restatement on a recorded case: dense input map from the cores, then the step loop."""
    co = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    T, B, n_in = d["x"].shape
    H = d["w_hh"].shape[1]
    w_ih = recover([co(c) for c in d["cores"]]).reshape(4 * H, n_in)
    xp = (co(d["x"]).reshape(T * B, n_in) @ w_ih.t() + co(d["bias"])).reshape(T, B, 4 * H)
    y, _, cT = step_loop(xp, co(d["w_hh"]), co(d["h0"]), co(d["c0"]), "hardsigmoid")
    return _np(y), _np(cT)
