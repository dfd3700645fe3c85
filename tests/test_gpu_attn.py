"""csrc/attn.hip on the device: the launch (`route="launch"`) against the float64 restatement of tests/_attn_ref.py,
with the composed torch route in the same input type as the yardstick.  With e_f the launch's error and e_c the composed
route's, both against float64 on the same (already rounded) inputs, and u one unit of the delivered type (2^-23 float32,
2^-8 bfloat16, 2^-11 float16):

    scores    max_ij |err_ij| / A_ij     A_ij = sum_k |Q_ik K_jk| / sqrt(d) + |mask_j|        e_f <= 2 max(e_c, u)
    context   max_ic |err_ic| / C_ic     C_ic = sum_j Pd_ij |V_jc|                            e_f <= 2 max(e_c, u)
    dq,dk,dv  max |err| / max |float64 gradient|                                              e_f <= 2 max(e_c, u)
              (a float64 gradient that is exactly zero -- dq and dk of a one-token sequence under a context gradient
              alone, dv under a score gradient alone -- has no max norm: there the scale is max |upstream| max |input|)

The factor two: the routes add the same terms in another order with another exp; the floor u: a composed route that
lands exactly must not fail the launch.  Scores that are -inf in the reference must be -inf.  Every case prints both
errors (run with -s to see them); DESIGN.md section 20 quotes the worst."""
import math

import pytest
import torch

import _attn_ref as R
from tadmm import _cabi, ops
from tadmm import functional as HF
from tadmm.bert_layers import BertSelfAttention

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNIT = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}

# (name, B, H, S, d, layout)
SHAPES = [
    ("s1", 2, 3, 1, 64, "plain"), ("s5", 2, 3, 5, 26, "plain"), ("s17", 2, 2, 17, 32, "plain"),
    ("s100", 2, 2, 100, 64, "plain"), ("s128", 1, 3, 128, 64, "plain"), ("s129", 2, 2, 129, 26, "plain"),
    ("s384", 1, 2, 384, 64, "plain"), ("s512", 1, 2, 512, 64, "plain"),
    ("packed", 2, 3, 40, 26, "packed"), ("odd", 2, 2, 33, 64, "odd"),
]
MASKS = ("none", "pad", "inf")
GRADS = ("ctx", "scores", "both", "scaled")


def make_qkv(B, H, S, d, layout, dtype, seed):
    """q, k, v (B, S, H*d) on the device: separate tensors, slices of one packed (B, S, 3*H*d) tensor, or tensors that
    start one element into their allocation."""
    g = torch.Generator().manual_seed(seed)
    Hd = H * d
    if layout == "packed":
        qkv = torch.randn(B, S, 3 * Hd, generator=g).to(dtype).to(DEV)
        return tuple(qkv[:, :, i * Hd:(i + 1) * Hd] for i in range(3))
    out = []
    for _ in range(3):
        t = torch.randn(B, S, Hd, generator=g).to(dtype)
        if layout == "odd":
            buf = torch.empty(B * S * Hd + 1, dtype=dtype, device=DEV)
            buf[1:].copy_(t.reshape(-1))
            t = buf[1:].view(B, S, Hd)
            assert (t.data_ptr() // t.element_size()) % 2 == 1
        else:
            t = t.to(DEV)
        out.append(t)
    return tuple(out)


def make_mask(kind, B, S, dtype):
    if kind == "none":
        return None
    lengths = [max(1, S - S // 3), 1][:B] if B > 1 else [max(1, S - S // 3)]
    if kind == "inf":                                  # a partly masked row with -inf in place of -10000
        m = R.padding_mask(lengths, S, dtype=torch.float32)
        m[0] = R.padding_mask([lengths[0]], S, fill=-math.inf)[0]
        return m.to(dtype).to(DEV)
    return R.padding_mask(lengths, S).to(dtype).to(DEV)


def scores_err(got, ref):
    got = got.detach().to("cpu", torch.float64)
    inf = torch.isinf(ref["scores"])
    assert torch.equal(torch.isinf(got) & (got < 0), inf), "-inf entries of the scores differ"
    err = torch.where(inf, torch.zeros_like(got), (got - ref["scores"]).abs())
    return float((err / ref["A"].clamp_min(1e-300)).max())


def ctx_err(got, ref):
    got = got.detach().to("cpu", torch.float64)
    return float(((got - ref["ctx"]).abs() / ref["C"].clamp_min(1e-300)).max())


def grad_err(got, want, scale):
    got = got.detach().to("cpu", torch.float64)
    return float((got - want).abs().max()) / scale


def bar(e_f, e_c, dtype, what):
    print(f"    {what:<28s} launch {e_f:.3e}   composed {e_c:.3e}   unit {UNIT[dtype]:.3e}")
    assert e_f <= 2.0 * max(e_c, UNIT[dtype]), (what, e_f, e_c)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_forward_against_float64(shape, dtype):
    name, B, H, S, d, layout = shape
    q, k, v = make_qkv(B, H, S, d, layout, dtype, seed=S * 7 + d)
    if layout != "plain":
        for t in (q, k, v):                            # read in place: no copy is made of such views
            assert ops._attn_heads(t, "t", "t", tuple(t.shape), dtype)[0].data_ptr() == t.data_ptr()
    g = torch.Generator(device=DEV).manual_seed(S)
    for kind in MASKS:
        mask = make_mask(kind, B, S, dtype)
        for p in (0.0, 0.1):
            keep = HF.attention_keep_mask(B, H, S, p, DEV, generator=g) if p > 0 else None
            kw = dict(dropout_p=p, training=p > 0, keep=keep)
            ref = R.restate(q, k, v, mask, H, p=p, keep=keep)
            cf, sf = HF.self_attention(q, k, v, mask, H, route="launch", **kw)
            cc, sc = HF.self_attention(q, k, v, mask, H, route="composed", **kw)
            assert cf.shape == (B, S, H * d) and cf.dtype == dtype and cf.is_contiguous()
            assert sf.shape == (B, H, S, S) and sf.dtype == dtype
            print(f"  {name} {dtype} mask={kind} p={p}")
            bar(scores_err(sf, ref), scores_err(sc, ref), dtype, "scores")
            bar(ctx_err(cf, ref), ctx_err(cc, ref), dtype, "context")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_gradients_against_float64(shape, dtype):
    name, B, H, S, d, layout = shape
    q, k, v = make_qkv(B, H, S, d, layout, dtype, seed=S * 11 + d)
    g = torch.Generator().manual_seed(S + 1)
    g_ctx = (torch.randn(B, S, H * d, generator=g)).to(dtype).to(DEV)
    g_sc = (torch.randn(B, H, S, S, generator=g) * 0.1).to(dtype).to(DEV)
    gd = torch.Generator(device=DEV).manual_seed(S + 2)
    for n, which in enumerate(GRADS):
        kind = MASKS[(n + S) % 3]
        p = 0.1 if n % 2 == 0 else 0.0
        mask = make_mask(kind, B, S, dtype)
        keep = HF.attention_keep_mask(B, H, S, p, DEV, generator=gd) if p > 0 else None
        mul = 3.75 if which == "scaled" else 1.0
        uc = g_ctx * mul if which in ("ctx", "both", "scaled") else None
        us = g_sc * mul if which in ("scores", "both", "scaled") else None
        ref = R.restate(q, k, v, mask, H, p=p, keep=keep, g_ctx=uc, g_sc=us)
        res = {}
        for route in ("launch", "composed"):
            leaves = [t.detach().requires_grad_() for t in (q, k, v)]
            assert all(a.stride() == b.stride() for a, b in zip(leaves, (q, k, v)))
            c, s = HF.self_attention(*leaves, mask, H, dropout_p=p, training=p > 0, keep=keep, route=route)
            outs, ups = zip(*[(o, u) for o, u in ((c, uc), (s, us)) if u is not None])
            got = torch.autograd.grad(outs, leaves, ups, allow_unused=True)
            res[route] = [torch.zeros_like(t) if g_ is None else g_ for g_, t in zip(got, leaves)]
        print(f"  {name} {dtype} grads={which} mask={kind} p={p}")
        ups = [float(u.abs().max()) for u in (uc, us) if u is not None]
        natural = max(ups) * max(float(t.abs().max()) for t in (q, k, v))
        for i, nm in enumerate(("dq", "dk", "dv")):
            scale = float(ref[nm].abs().max()) or natural
            bar(grad_err(res["launch"][i], ref[nm], scale), grad_err(res["composed"][i], ref[nm], scale), dtype, nm)


def test_recorded_reference_through_the_module(golden_dir):
    """G18 (the reference's own TTBertSelfAttention on the CPU, float32) through BertSelfAttention with the projections
    replaced by the `weights=` hook: 1e-5 of the largest magnitude, float32 against a float32 run in another order."""
    class Hook:
        def __init__(self, d):
            self.d = d

        def qkv_transform(self, hidden_states, layer_id):
            return self.d["q"], self.d["k"], self.d["v"]

    for meta in R.golden_index(golden_dir):
        d = {key: t.to(DEV) for key, t in R.recorded(golden_dir, meta["name"]).items()}
        for key in ("q", "k", "v"):
            d[key].requires_grad_()
        mod = BertSelfAttention(meta["H"] * meta["d"], meta["H"], 0.1).to(DEV).eval()
        mod.route = "launch"
        ctx, sc = mod(d["q"], d.get("mask"), weights=Hook(d))
        gq, gk, gv = torch.autograd.grad((ctx, sc), (d["q"], d["k"], d["v"]), (d["g_ctx"], d["g_sc"]))
        for got, want in ((ctx, d["ctx"]), (sc, d["scores"]), (gq, d["dq"]), (gk, d["dk"]), (gv, d["dv"])):
            assert float((got.detach() - want).abs().max()) <= 1e-5 * float(want.abs().max()), meta


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_two_runs_are_bit_identical(dtype):
    B, H, S, d = 2, 2, 129, 26
    q, k, v = make_qkv(B, H, S, d, "plain", dtype, seed=5)
    mask = make_mask("pad", B, S, dtype)
    keep = HF.attention_keep_mask(B, H, S, 0.1, DEV)
    g = torch.Generator().manual_seed(9)
    uc = torch.randn(B, S, H * d, generator=g).to(dtype).to(DEV)
    us = torch.randn(B, H, S, S, generator=g).to(dtype).to(DEV)
    runs = []
    for _ in range(2):
        leaves = [t.detach().requires_grad_() for t in (q, k, v)]
        c, s = HF.self_attention(*leaves, mask, H, dropout_p=0.1, training=True, keep=keep, route="launch")
        runs.append((c, s) + torch.autograd.grad((c, s), leaves, (uc, us)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_float16_is_forward_only():
    B, H, S, d = 2, 2, 100, 64
    dtype = torch.float16
    q, k, v = make_qkv(B, H, S, d, "plain", dtype, seed=3)
    mask = make_mask("pad", B, S, dtype)
    ref = R.restate(q, k, v, mask, H)
    cf, sf = HF.self_attention(q, k, v, mask, H, route="launch")
    cc, sc = HF.self_attention(q, k, v, mask, H, route="composed")
    bar(scores_err(sf, ref), scores_err(sc, ref), dtype, "scores f16")
    bar(ctx_err(cf, ref), ctx_err(cc, ref), dtype, "context f16")
    _, _, stats = ops.attn_fwd(q, k, v, mask, H, need_stats=True)
    with pytest.raises(_cabi.TadmmError, match="forward only"):
        ops.attn_bwd(q, k, v, mask, H, stats, cf, None)
    with pytest.raises(_cabi.TadmmError, match="float16 with gradients"):
        HF.self_attention(q.detach().requires_grad_(), k, v, mask, H, route="launch")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_context_does_not_depend_on_need_scores(dtype):
    B, H, S, d = 2, 3, 70, 26
    q, k, v = make_qkv(B, H, S, d, "plain", dtype, seed=4)
    mask = make_mask("pad", B, S, dtype)
    a, sa = HF.self_attention(q, k, v, mask, H, need_scores=True, route="launch")
    b, sb = HF.self_attention(q, k, v, mask, H, need_scores=False, route="launch")
    assert sa is not None and sb is None and torch.equal(a, b)


def test_module_dropout_follows_the_seed():
    torch.manual_seed(0)
    mod = BertSelfAttention(96, 3, 0.1).to(DEV).train()
    mod.route = "launch"
    x = torch.randn(2, 37, 96, device=DEV)
    mask = make_mask("pad", 2, 37, torch.float32)
    outs = []
    for seed in (11, 11, 12):
        torch.manual_seed(seed)
        outs.append(mod(x, mask)[0])
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    mod.eval()
    assert torch.equal(mod(x, mask)[0], mod(x, mask)[0])


@pytest.mark.parametrize("B,H,S,d", [(1, 2, 513, 16), (1, 2, 20, 65)])
def test_shapes_beyond_the_launch_take_the_composed_route(B, H, S, d):
    q, k, v = make_qkv(B, H, S, d, "plain", torch.float32, seed=6)
    mask = make_mask("pad", B, S, torch.float32)
    assert not ops.attn_fits(S, d, H)
    a, sa = HF.self_attention(q, k, v, mask, H, route=None)
    b, sb = HF.self_attention_composed(q, k, v, mask, H)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    with pytest.raises(_cabi.TadmmError):
        HF.self_attention(q, k, v, mask, H, route="launch")
