"""tadmm/vit_layers.py on the device, float32: a TTBlock and a small TTVisionTransformer with every route forced to the
launch, against the float64 restatement of tests/_vit_ref.py; the composed routes are the yardstick under the rule of
tests/test_gpu_prenorm.py, in the max norm: with e_f the launch route's error and e_c the composed route's, both
max |err| / max |float64 value|, e_f <= 2 max(e_c, 2^-23), for the output and every parameter gradient.  The TT-matrix
blocks are restated too: their dense weights are the cores multiplied left to right (`_vit_ref.tt_weight`), and float64
autograd carries the gradients to the cores.  The shipped DeiT-tiny rank table has shapes for 192 channels only, so the
TT blocks run at (2, 197, 192, 3) and (2, 5, 192, 3) and the 64-channel shape is dense."""
import pytest
import torch

import _vit_ref as R
from tadmm import get_hp_dict, workloads
from tadmm import vit_layers as VL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -23


class NoRanks:
    ranks = {}
    tt_shapes = {}


def bar(e_f, e_c, what):
    print(f"    {what:<40s} launch {e_f:.3e}   composed {e_c:.3e}")
    assert e_f <= 2.0 * max(e_c, U), (what, e_f, e_c)
    return e_f


def rel(got, want):
    return float((got.detach().to("cpu", torch.float64) - want.detach()).abs().max()) / float(want.detach().abs().max())


def randomise(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, prm in mod.named_parameters():
            if name.endswith("norm1.weight") or name.endswith("norm2.weight") or name == "norm.weight":
                prm.copy_(1 + 0.3 * torch.randn(prm.shape, generator=g))
            elif prm.dim() == 1:
                prm.copy_(0.2 * torch.randn(prm.shape, generator=g))
    return mod


@pytest.mark.parametrize("case", [("dense", 2, 197, 192, 3), ("dense", 2, 5, 64, 2), ("ttm", 2, 197, 192, 3),
                                  ("ttm", 2, 5, 192, 3)], ids=lambda c: "-".join(str(v) for v in c))
def test_block_against_float64(case):
    kind, B, N, C, heads = case
    torch.manual_seed(B * N + C)
    hp = get_hp_dict("ttm_deit_tiny_patch16_224", "2") if kind == "ttm" else NoRanks
    blk = randomise(VL.TTBlock(C, heads, qkv_bias=True, linear=VL.TTLinearM, block_id=0, hp_dict=hp), 2).to(DEV).eval()
    assert isinstance(blk.attn.qkv, VL.TTLinearM) == (kind == "ttm") and isinstance(blk.mlp.fc2, VL.TTLinearM) == (kind == "ttm")
    x, up = torch.randn(B, N, C), torch.randn(B, N, C)
    names = [n for n, _ in blk.named_parameters()]
    sd = R.state64(blk, requires_grad=True)
    want = R.block(R.f64(x), R.with_tt_weights(sd, blk), "", heads, eps=blk.norm1.eps)
    want_g = torch.autograd.grad(want, [sd[n] for n in names], R.f64(up))
    got = {}
    for route in ("launch", "composed"):
        out = blk.set_route(route)(x.to(DEV))
        got[route] = [out] + list(torch.autograd.grad(out, list(blk.parameters()), up.to(DEV)))
    worst = 0.0
    for i, (what, ref) in enumerate(zip(["output"] + names, [want] + list(want_g))):
        worst = max(worst, bar(rel(got["launch"][i], ref), rel(got["composed"][i], ref), what))
    print(f"    worst launch error of the {kind} block {worst:.3e}")


def test_chained_blocks_equal_two_plain_calls():
    """Two blocks chained (norm1 of the second from the first block's second tail, a final LayerNorm from the second's)
    against two plain forward(x) calls, composed route, both against float64."""
    torch.manual_seed(7)
    blocks = [randomise(VL.TTBlock(64, 2, qkv_bias=True, block_id=i, hp_dict=NoRanks), 3 + i).to(DEV).eval().set_route("composed")
              for i in range(2)]
    last = randomise(torch.nn.LayerNorm(64, eps=1e-6), 9).to(DEV)
    x = torch.randn(2, 5, 64)
    ref = R.f64(x)
    for blk in blocks:
        ref = R.block(ref, R.state64(blk), "", 2, eps=blk.norm1.eps)
    ref_n = R.plain_layer_norm(ref, R.f64(last.weight), R.f64(last.bias), 1e-6)
    with torch.no_grad():
        plain = blocks[1](blocks[0](x.to(DEV)))
        h, n = blocks[0](x.to(DEV), None, blocks[1].norm1)
        chained, normed = blocks[1](h, n, last)
        bar(rel(chained, ref), rel(plain, ref), "chained stream")
        bar(rel(normed, ref_n), rel(last(plain), ref_n), "chained final norm")
        for blk in blocks:
            blk.set_route("launch")
        h, n = blocks[0](x.to(DEV), None, blocks[1].norm1)
        chained_l, normed_l = blocks[1](h, n, last)
        bar(rel(chained_l, ref), rel(plain, ref), "chained stream, launch")
        bar(rel(normed_l, ref_n), rel(last(plain), ref_n), "chained final norm, launch")


@pytest.mark.parametrize("distilled", [False, True], ids=["plain", "distilled"])
def test_small_model(distilled):
    torch.manual_seed(3)
    model = randomise(VL.TTVisionTransformer(img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=2, num_classes=10,
                                             distilled=distilled, drop_path_rate=0.5, hp_dict=NoRanks), 4).eval()
    img = torch.randn(8, 3, 32, 32)
    want = R.vit(R.f64(img), R.state64(model), 2, 2, 16)
    model.to(DEV)
    with torch.no_grad():
        got = {route: model.set_route(route)(img.to(DEV)) for route in ("launch", "composed")}
    assert got["launch"].shape == (8, 10)
    bar(rel(got["launch"], want), rel(got["composed"], want), "eval logits")
    model.train().set_route("launch")                  # a training step whose DropPath follows the seed
    outs = []
    for seed in (21, 21, 22):
        torch.manual_seed(seed)
        model.zero_grad(set_to_none=True)
        out = model(img.to(DEV))
        assert isinstance(out, tuple) == distilled
        out = sum(out) if distilled else out
        out.square().mean().backward()
        outs.append((out.detach(), model.blocks[1].mlp.fc1.weight.grad.clone(), model.cls_token.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    assert not torch.equal(outs[0][0], outs[2][0])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def test_state_dict_of_deit_small_is_timm_s():
    """The names and shapes of the four projections of every block are those of `workloads.deit_small_shape` (what the
    rank table is keyed by); the rest are timm 0.4.x's VisionTransformer(distilled=False) at DeiT-small sizes."""
    model = VL.ttm_deit_small_patch16_224(NoRanks)
    sd = model.state_dict()
    table = get_hp_dict("ttm_deit_small_patch16_224", "2")
    proj = [k for k in sd if k.endswith(("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight"))]
    assert set(proj) == set(table.ranks) and len(proj) == 48
    for k in proj:
        assert tuple(sd[k].shape) == workloads.deit_small_shape(k), k
        assert tuple(sd[k[:-6] + "bias"].shape) == workloads.deit_small_shape(k)[:1]
    want = {"cls_token": (1, 1, 384), "pos_embed": (1, 197, 384), "patch_embed.proj.weight": (384, 3, 16, 16),
            "patch_embed.proj.bias": (384,), "norm.weight": (384,), "norm.bias": (384,), "head.weight": (1000, 384),
            "head.bias": (1000,)}
    for i in range(12):
        for n in ("norm1", "norm2"):
            want[f"blocks.{i}.{n}.weight"] = want[f"blocks.{i}.{n}.bias"] = (384,)
    rest = {k: tuple(v.shape) for k, v in sd.items() if k not in proj and k[:-4] + "weight" not in proj}
    assert rest == want
    other = VL.ttm_deit_small_patch16_224(NoRanks)
    other.load_state_dict(sd)
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in sd.items())
    tt = VL.ttm_deit_tiny_patch16_224(get_hp_dict("ttm_deit_tiny_patch16_224", "2"), depth=1)
    again = VL.ttm_deit_tiny_patch16_224(get_hp_dict("ttm_deit_tiny_patch16_224", "2"), depth=1)
    again.load_state_dict(tt.state_dict())
    assert "blocks.0.attn.qkv.tt_cores.0" in tt.state_dict() and "blocks.0.attn.qkv.weight" not in tt.state_dict()
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in tt.state_dict().items())
