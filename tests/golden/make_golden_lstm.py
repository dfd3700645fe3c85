"""Generate golden vectors G11 (the TT-LSTM step function) from the REAL reference.

    python tests/golden/make_golden_lstm.py <path of the reference checkout>

Runs only where the reference is at hand.  Loads its ablation/tt_lstm_inference.py as a module object (its top level
builds the UCF11 example and prints that example's compression ratio, which is recorded), then sets the module's
globals -- the TT shapes, ranks, cores, recurrent weight, bias and sizes its `lstm_step` reads -- to small seeded cases
and calls the reference's OWN `lstm_step` over a sequence.  Recorded per case: inputs, weights, every h_t and the final
c.  ablation/compare_tt_lstm.py is run as a script and the figures it prints for its own (TIMIT) shapes are recorded as
well.  The reference never travels with the tests; this data file does.
"""
import contextlib
import importlib.util
import io
import os
import re
import runpy
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

# name: (T, B, in_tt, out_tt, ranks, nonzero initial state)
CASES = {
    "r_odd": (5, 3, [3, 4, 5], [2, 3, 4], [1, 3, 4, 5, 4, 3, 1], False),
    "r_wide": (4, 2, [4, 5, 6], [4, 4, 4], [1, 4, 8, 8, 6, 4, 1], True),
    "r_b1": (6, 1, [2, 3, 2, 2], [2, 2, 5], [1, 2, 3, 4, 3, 2, 2, 1], True),
}


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "ablation", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        spec.loader.exec_module(mod)
    return mod, out.getvalue()


def numbers(text, label):
    return [float(v) for v in re.findall(re.escape(label) + r":\s*([0-9.eE+-]+)", text)]


def main(path):
    torch.manual_seed(11)
    mod, printed = load(path, "tt_lstm_inference")
    rec = {"inference_ratio": np.array(numbers(printed, "Compression ratio")),
           "inference_in_tt": np.array([8, 20, 20, 18]), "inference_out_tt": np.array([4, 8, 8]),
           "inference_ranks": np.array([1, 4, 5, 9, 12, 6, 3, 1])}
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        runpy.run_path(os.path.join(path, "ablation", "compare_tt_lstm.py"))
    text = out.getvalue()
    rec["compare_in_tt"], rec["compare_out_tt"] = np.array([5, 7, 9]), np.array([4, 8, 16])
    rec["compare_ranks"] = np.array([1, 2, 2, 4, 2, 2, 1])
    rec["compare_tt_params"] = np.array(numbers(text, "# tt_params")[-1:])
    rec["compare_ratio"] = np.array(numbers(text, "Compression ratio"))
    rec["compare_tt_flops"] = np.array(numbers(text, "# tt_flops")[-1:])
    rec["compare_speedup"] = np.array(numbers(text, "Speedup"))
    for name, (T, B, in_tt, out_tt, ranks, state) in CASES.items():
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        H, n_in = int(np.prod(out_tt)), int(np.prod(in_tt))
        shapes = [4 * out_tt[0]] + out_tt[1:] + in_tt
        cores = [torch.randn(ranks[i], shapes[i], ranks[i + 1], generator=g) for i in range(len(shapes))]
        w = cores[0].reshape(-1, ranks[1])
        for core in cores[1:]:
            w = w.reshape(-1, core.shape[0]) @ core.reshape(core.shape[0], -1)
        cores[0] = cores[0] * (1.5 / (float(w.std()) * n_in ** 0.5))     # pre-activations of standard deviation ~1.5
        mod.in_tt_shapes, mod.in_tt_order = list(in_tt), len(in_tt)
        mod.out_tt_shapes, mod.out_tt_order = shapes[:len(out_tt)], len(out_tt)
        mod.tt_ranks, mod.tt_shapes, mod.tt_cores = list(ranks), shapes, cores
        mod.in_features, mod.out_features, mod.hidden_size = n_in, H, H
        mod.h2h_weight = (torch.rand(4 * H, H, generator=g) * 2 - 1) * (2 / H ** 0.5)
        mod.bias = 0.5 * torch.randn(4 * H, generator=g)
        x = torch.randn(T, B, n_in, generator=g)
        h = 0.5 * torch.randn(B, H, generator=g) if state else torch.zeros(B, H)
        c = 0.5 * torch.randn(B, H, generator=g) if state else torch.zeros(B, H)
        rec[f"{name}.meta"] = np.array([T, B, len(in_tt), len(out_tt)])
        rec[f"{name}.tt_shapes"], rec[f"{name}.ranks"] = np.array(shapes), np.array(ranks)
        rec[f"{name}.x"], rec[f"{name}.h0"], rec[f"{name}.c0"] = x.numpy(), h.numpy().copy(), c.numpy().copy()
        rec[f"{name}.w_hh"], rec[f"{name}.bias"] = mod.h2h_weight.numpy(), mod.bias.numpy()
        for k, core in enumerate(cores):
            rec[f"{name}.core{k}"] = core.numpy()
        ys = []
        for t in range(T):
            h, c = mod.lstm_step(x[t], h, c)
            ys.append(h.numpy().copy())
        rec[f"{name}.y"], rec[f"{name}.cT"] = np.stack(ys), c.numpy().copy()
    dst = os.path.join(HERE, "g11_tt_lstm.npz")
    np.savez_compressed(dst, **rec)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
