"""Generate golden vectors G18 (the self-attention of a BERT encoder layer) from the REAL reference.

    python tests/golden/make_golden_attn.py <path of the reference checkout>

Runs only where the reference is at hand: imports its xcompression/transformer/compressed_modeling_tt.py, builds its
own TTBertSelfAttention, feeds fixed q / k / v through the `weights=` hook of its forward (no projection weights are
involved) and records, on the CPU in float32 with dropout off (`eval()`): q, k, v, the additive mask, the context, the
raw masked scores, and the autograd gradients of q, k, v for fixed upstream gradients of both outputs.  The reference
never travels with the tests; these data files do.

The `transformer` package is entered without running its __init__ (which pulls in tokenizers and download helpers), and
third-party packages that are not installed (boto3, botocore, requests, tqdm, tensorly, ...) get empty stand-in modules:
none of them is touched by the attention.  The three projections the constructor builds are never called; where the
reference's hard-wired TT shapes (24 x 32 -> 768) do not fit a small hidden size, `nn.Identity` stands in for them.

Inputs and upstream gradients are multiples of 2^-6 so that the archive compresses; the outputs are what they are."""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

# (name, B, H, S, d, kept tokens per batch row; None: no padding).  The reference's BERT-base layer is (1, 12, 128, 64);
# its arrays (and those of 4 heads: 1.06 MB compressed) would pass the size limit of a committed file, so it is recorded
# with 2 of the 12 heads; heads never interact.
CASES = [
    ("b2_h3_s8_d32", 2, 3, 8, 32, [8, 5]),
    ("b2_h2_s17_d26", 2, 2, 17, 26, [11, 1]),
    ("b2_h2_s17_d26_nopad", 2, 2, 17, 26, None),
    ("b1_h2_s128_d64", 1, 2, 128, 64, [100]),
]


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (Exception,), {})


def load_reference(path):
    root = os.path.join(path, "xcompression")
    pkg = types.ModuleType("transformer")
    pkg.__path__ = [os.path.join(root, "transformer")]
    sys.modules["transformer"] = pkg
    sys.path.insert(0, root)
    for _ in range(32):
        try:
            return importlib.import_module("transformer.compressed_modeling_tt")
        except ModuleNotFoundError as e:
            if e.name is None or e.name.split(".")[0] == "transformer":
                raise
            parts = e.name.split(".")
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault(".".join(parts[:i]), _Stub(".".join(parts[:i])))
    raise RuntimeError("too many missing modules")


def quantised(g, shape, scale=1.0):
    return (torch.randn(shape, generator=g) * scale * 64).round().clamp(-255, 255) / 64


class Hook:
    def __init__(self, q, k, v):
        self.qkv = (q, k, v)

    def qkv_transform(self, hidden_states, layer_id):
        return self.qkv


def main(path):
    mod = load_reference(path)
    rec, index = {}, {"cases": []}
    for name, B, H, S, d, lengths in CASES:
        cfg = types.SimpleNamespace(hidden_size=H * d, num_attention_heads=H, attention_probs_dropout_prob=0.1)
        try:
            layer = mod.TTBertSelfAttention(cfg, layer_id=3)
        except Exception:
            real, mod.TTLinear = mod.TTLinear, (lambda **kw: torch.nn.Identity())
            try:
                layer = mod.TTBertSelfAttention(cfg, layer_id=3)
            finally:
                mod.TTLinear = real
        layer.eval()
        g = torch.Generator().manual_seed(1800 + S * 3 + d)
        q, k, v = (quantised(g, (B, S, H * d)).requires_grad_() for _ in range(3))
        g_ctx = quantised(g, (B, S, H * d))
        g_sc = quantised(g, (B, H, S, S), 0.25)
        mask = None
        if lengths is not None:
            mask = torch.zeros(B, 1, 1, S)
            for b, n in enumerate(lengths):
                mask[b, 0, 0, n:] = -10000.0
        ctx, scores = layer(torch.zeros(B, S, H * d), 0.0 if mask is None else mask, weights=Hook(q, k, v))
        dq, dk, dv = torch.autograd.grad((ctx, scores), (q, k, v), (g_ctx, g_sc))
        arrays = dict(q=q, k=k, v=v, g_ctx=g_ctx, g_sc=g_sc, ctx=ctx, scores=scores, dq=dq, dk=dk, dv=dv)
        if mask is not None:
            arrays["mask"] = mask
        for key, t in arrays.items():
            rec[f"{name}/{key}"] = t.detach().contiguous().numpy().astype(np.float32)
        index["cases"].append(dict(name=name, B=B, H=H, S=S, d=d, lengths=lengths))
    np.savez_compressed(os.path.join(HERE, "g18_attention.npz"), **rec)
    with open(os.path.join(HERE, "g18_attention.json"), "w") as f:
        json.dump(index, f, indent=1)
    print("wrote", len(rec), "arrays,", os.path.getsize(os.path.join(HERE, "g18_attention.npz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
