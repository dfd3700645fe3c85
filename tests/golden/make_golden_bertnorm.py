"""Generate golden vectors G19 (the dropout + residual + LayerNorm tail of a BERT encoder layer) from the REAL reference.

    python tests/golden/make_golden_bertnorm.py <path of the reference checkout>

Runs only where the reference is at hand: imports its xcompression/transformer/compressed_modeling_tt.py (the loader and
stand-in modules of make_golden_attn.py), builds its own BertLayerNorm, TTBertSelfOutput and BertOutput, gives them
non-trivial `weight` and `bias`, feeds a fixed dense output through the `weights=` hook of the two sub-layer forwards (no
projection weights are involved) and records, on the CPU in float32 with dropout off (`eval()`): the inputs, the output,
and the autograd gradients of both inputs, `weight` and `bias` for a fixed upstream gradient.  Where the reference's
hard-wired TT shapes (24 x 32 -> 768, 48 x 64 -> 768) do not fit a small hidden size, `nn.Identity` stands in for the
projection the constructor builds and the forward never calls.  It also records, as lists of names, the `state_dict()`
keys of the reference's BertLayer and of a two-layer BertEncoder at BERT-base sizes.

Inputs, parameters and upstream gradients are multiples of 2^-6 within +-127/64 (the upstream gradient: multiples of
2^-4) and are stored as int8 numerators over 64 (`<name>/<key>.q6`); the outputs are float32 and what they are.  With
dropout off the gradients of the two inputs are one array: it is stored once and the index says so (`dres_is_dx`).  To
stay under the size limit the three modules are all recorded at (2, 8, 96), BertLayerNorm also at (2, 17, 312) and
TTBertSelfOutput also at (1, 16, 768)."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
from make_golden_attn import load_reference  # noqa: E402

# (name, module, B, S, hidden)
CASES = [
    ("ln_b2_s8_h96", "BertLayerNorm", 2, 8, 96),
    ("selfout_b2_s8_h96", "TTBertSelfOutput", 2, 8, 96),
    ("out_b2_s8_h96", "BertOutput", 2, 8, 96),
    ("ln_b2_s17_h312", "BertLayerNorm", 2, 17, 312),
    ("selfout_b1_s16_h768", "TTBertSelfOutput", 1, 16, 768),
]


def quantised(g, shape, step=64):
    """normal draws of deviation 1/2, rounded to multiples of 1/step, within +-127/64"""
    lim = 127 * step // 64
    return (torch.randn(shape, generator=g) * 0.5 * step).round().clamp(-lim, lim) / step


class Hook:
    def __init__(self, x):
        self.x = x

    def output_transform(self, hidden_states, layer_id):
        return self.x

    def ffn_output_transform(self, hidden_states, layer_id):
        return self.x


def build(mod, kind, cfg):
    if kind == "BertLayerNorm":
        return mod.BertLayerNorm(cfg.hidden_size, eps=1e-12)
    try:
        return getattr(mod, kind)(cfg, layer_id=3)
    except Exception:
        real, mod.TTLinear = mod.TTLinear, (lambda **kw: torch.nn.Identity())
        try:
            return getattr(mod, kind)(cfg, layer_id=3)
        finally:
            mod.TTLinear = real


def main(path):
    mod = load_reference(path)
    rec, index = {}, {"cases": []}
    for name, kind, B, S, hidden in CASES:
        cfg = types.SimpleNamespace(hidden_size=hidden, intermediate_size=4 * hidden, hidden_dropout_prob=0.1)
        layer = build(mod, kind, cfg).eval()
        norm = layer if kind == "BertLayerNorm" else layer.LayerNorm
        g = torch.Generator().manual_seed(1900 + S * 3 + hidden)
        with torch.no_grad():
            norm.weight.copy_(1.0 + quantised(g, (hidden,), 32) / 2)
            norm.bias.copy_(quantised(g, (hidden,)))
        x = quantised(g, (B, S, hidden)).requires_grad_()
        up = quantised(g, (B, S, hidden), 16)
        arrays = dict(x=x, g=up, weight=norm.weight, bias=norm.bias)
        if kind == "BertLayerNorm":
            y = layer(x)
            dx, dw, db = torch.autograd.grad(y, (x, norm.weight, norm.bias), up)
            same = None
        else:
            res = quantised(g, (B, S, hidden)).requires_grad_()
            arrays["res"] = res
            y = layer(torch.zeros(B, S, hidden), res, weights=Hook(x))
            dx, dres, dw, db = torch.autograd.grad(y, (x, res, norm.weight, norm.bias), up)
            same = bool(torch.equal(dx, dres))
            if not same:
                rec[f"{name}/dres"] = dres.numpy().astype(np.float32)
        for key, t in arrays.items():
            q = (t.detach() * 64).round()
            assert torch.equal(q / 64, t.detach()) and float(q.abs().max()) < 128
            rec[f"{name}/{key}.q6"] = q.numpy().astype(np.int8)
        for key, t in dict(y=y, dx=dx, dweight=dw, dbias=db).items():
            rec[f"{name}/{key}"] = t.detach().contiguous().numpy().astype(np.float32)
        index["cases"].append(dict(name=name, module=kind, B=B, S=S, hidden=hidden, dres_is_dx=same))
    base = mod.CompressedBertConfig(30522, num_hidden_layers=2)
    base.load_compressed_model = False
    index["bert_layer_keys"] = list(mod.BertLayer(base, layer_id=0).state_dict())
    index["bert_encoder_keys"] = list(mod.BertEncoder(base).state_dict())
    np.savez_compressed(os.path.join(HERE, "g19_bertnorm.npz"), **rec)
    with open(os.path.join(HERE, "g19_bertnorm.json"), "w") as f:
        json.dump(index, f, indent=1)
    print("wrote", len(rec), "arrays,", os.path.getsize(os.path.join(HERE, "g19_bertnorm.npz")), "+",
          os.path.getsize(os.path.join(HERE, "g19_bertnorm.json")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
