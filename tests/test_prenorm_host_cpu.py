"""Host side of the pre-norm block tail and the vision transformer (no GPU): every refusal of the C entries of
csrc/prenorm.hip, the workspace and fits queries, the refusal function, the composed route of `add_layer_norm` and the
dense modules of tadmm/vit_layers.py against the float64 restatement of tests/_vit_ref.py, the factories' argument errors
and the import lines."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import _vit_ref as R
from tadmm import _cabi, ops
from tadmm import functional as HF
from tadmm import vit_layers as VL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HMAX = ops.bertnorm_hmax()


class NoRanks:
    ranks = {}
    tt_shapes = {}


def test_descriptor_size_fits_and_workspace():
    lib = _cabi.load()
    assert lib.tadmm_prenorm_desc_bytes() == C.sizeof(_cabi.PreNormDesc)
    for hidden, want in ((1, True), (HMAX, True), (HMAX + 1, False)):
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            assert ops.prenorm_fits(hidden, dt) is want
    for hidden in (0, -1):
        with pytest.raises(_cabi.TadmmError):
            ops.prenorm_fits(hidden)
    hmax = C.c_int(7)
    assert lib.tadmm_prenorm_fits(None, C.byref(hmax)) == -1 and hmax.value == HMAX
    assert lib.tadmm_prenorm_fits(None, None) == -1
    # the geometry of the bertnorm backward: min(ceil(rows / 4), 512) partials of (2, hidden rounded up to 4) floats
    assert ops.prenorm_workspace_bytes(1, 1) == 256
    assert ops.prenorm_workspace_bytes(2 * 197, 192) == 99 * 2 * 192 * 4       # ceil(394 / 4) workgroups, 594 units of 256
    assert ops.prenorm_workspace_bytes(5, 65) == 2 * 2 * 68 * 4 + 192
    assert ops.prenorm_workspace_bytes(10 ** 6, 768) == 512 * 2 * 768 * 4
    assert ops.prenorm_workspace_bytes(0, 768) == 0
    for rows, hidden in ((130, 312), (7, 63), (4097, 1000)):
        assert ops.prenorm_workspace_bytes(rows, hidden) == ops.bertnorm_workspace_bytes(rows, hidden)
    dsc = _cabi.PreNormDesc()
    dsc.rows, dsc.hidden = 4, 0
    assert lib.tadmm_prenorm_workspace_bytes(C.byref(dsc), C.byref(C.c_size_t())) == -1
    dsc.rows, dsc.hidden = -1, 8
    assert lib.tadmm_prenorm_workspace_bytes(C.byref(dsc), C.byref(C.c_size_t())) == -1
    assert lib.tadmm_prenorm_workspace_bytes(None, C.byref(C.c_size_t())) == -1
    dsc.rows = 4
    assert lib.tadmm_prenorm_workspace_bytes(C.byref(dsc), None) == -1


def test_launch_entries_refuse_before_launching():
    """No device is needed: every refusal comes before the first HIP call that would want one."""
    lib = _cabi.load()
    h = C.c_void_p()
    lib.tadmm_create(0, C.byref(h))
    assert h, "a handle needs no device"
    raw = (C.c_char * 16384)()
    p = C.addressof(raw) + (-C.addressof(raw)) % 16

    def desc(**kw):
        d = _cabi.PreNormDesc()
        d.x, d.b = p, p + 512
        d.x_ld = d.b_ld = 8
        d.keep, d.path_keep, d.gamma, d.beta = p + 1024, p + 1280, p + 1536, p + 1600
        d.s, d.y, d.stats = p + 2048, p + 2560, p + 3072
        d.g_y, d.g_s = p + 3584, p + 4096
        d.dx, d.db, d.dgamma, d.dbeta = p + 4608, p + 5120, p + 5632, p + 5696
        d.workspace, d.workspace_bytes = p + 6144, 256
        d.p, d.p_path, d.eps = 0.1, 0.2, 1e-6
        d.rows, d.rows_per_sample, d.hidden, d.dtype, d.param_dtype = 6, 3, 8, _cabi.CHAIN_F32, _cabi.CHAIN_F32
        for key, val in kw.items():
            setattr(d, key, val)
        return d

    bf = dict(dtype=_cabi.CHAIN_BF16, param_dtype=_cabi.CHAIN_BF16)
    both = [
        (dict(hidden=0), "hidden >= 1"), (dict(hidden=-3), "hidden >= 1"), (dict(rows=-1), "rows >= 0"),
        (dict(rows_per_sample=4), "whole samples"), (dict(rows_per_sample=0), "whole samples"),
        (dict(rows_per_sample=-3), "whole samples"),
        (dict(dtype=3), "type"), (dict(dtype=-1), "type"),
        (dict(param_dtype=_cabi.CHAIN_BF16), "gamma and beta are float32 or of the type of x"),
        (dict(p=1.0), "p 1 outside"), (dict(p=-0.1), "outside"), (dict(p=float("nan")), "outside"),
        (dict(p_path=1.0), "p_path 1 outside"), (dict(p_path=-0.5), "p_path"), (dict(p_path=float("nan")), "p_path"),
        (dict(keep=None), "without a keep"), (dict(path_keep=None), "without a path_keep"),
        (dict(eps=-1.0), "eps"), (dict(eps=float("inf")), "eps"), (dict(eps=float("nan")), "eps"),
        (dict(gamma=None), "gamma"), (dict(gamma=p + 1538), "gamma"),
        (dict(s=None), "s is NULL"), (dict(s=p + 2049, **bf), "s is NULL or misaligned"), (dict(stats=p + 3074), "stats"),
    ]
    fwd_only = [(dict(x=None), "x is NULL"), (dict(x=p + 2), "x is NULL or misaligned"), (dict(b=None), "b is NULL"),
                (dict(b=p + 513, **bf), "b is NULL or misaligned"),
                (dict(x_ld=7), "stride of x"), (dict(x_ld=0), "stride of x"), (dict(b_ld=-8), "stride of b"),
                (dict(beta=None), "beta"), (dict(beta=p + 1601, **bf), "beta"), (dict(y=None), "y is NULL"),
                (dict(y=p + 2562), "y is NULL or misaligned"), (dict(y=p + 2048), "one buffer")]
    bwd_only = [(dict(dtype=_cabi.CHAIN_F16), "forward only"), (dict(stats=None), "stats is NULL"),
                (dict(g_y=None, g_s=None), "both NULL"), (dict(g_y=p + 3586), "g_y / g_s"), (dict(g_s=p + 4097, **bf), "g_y / g_s"),
                (dict(dx=p + 4610), "dx / db"), (dict(db=p + 5121, **bf), "dx / db"), (dict(db=p + 4608), "one buffer"),
                (dict(dgamma=p + 5634), "dgamma / dbeta"), (dict(dbeta=p + 5697), "dgamma / dbeta")]
    for entry, cases in ((lib.tadmm_prenorm_fwd, both + fwd_only), (lib.tadmm_prenorm_bwd, both + bwd_only)):
        for kw, text in cases:
            assert entry(h, C.byref(desc(**kw)), None) == -1, kw
            assert text in lib.tadmm_last_error(h).decode(), (kw, lib.tadmm_last_error(h))
        big = dict(hidden=HMAX + 1, x_ld=HMAX + 1, b_ld=HMAX + 1)
        assert entry(h, C.byref(desc(**big)), None) == -5
        assert str(HMAX) in lib.tadmm_last_error(h).decode()
        assert entry(h, None, None) == -1 and "NULL" in lib.tadmm_last_error(h).decode()
        assert entry(None, C.byref(desc()), None) == -1
        assert entry(h, C.byref(desc(rows=0)), None) == 0             # no rows: success, nothing to launch
    for kw in (dict(workspace=None), dict(workspace_bytes=255), dict(workspace=p + 6148)):
        assert lib.tadmm_prenorm_bwd(h, C.byref(desc(**kw)), None) == -2, kw
        assert "workspace" in lib.tadmm_last_error(h).decode()
    # one gradient alone is accepted up to the launch: with no rows nothing is launched
    for kw in (dict(g_y=None), dict(g_s=None)):
        assert lib.tadmm_prenorm_bwd(h, C.byref(desc(rows=0, **kw)), None) == 0
    lib.tadmm_destroy(h)


def test_refusal_rule_and_routing_rule():
    ok = dict(is_cuda=True, dtype=torch.float32, rows=394, hidden=192, grad=True, param_dtype=torch.float32)
    fn = HF.add_layer_norm_launch_refusal
    assert fn(**ok) is None
    assert fn(**dict(ok, dtype=torch.bfloat16)) is None
    assert fn(**dict(ok, dtype=torch.bfloat16, param_dtype=torch.bfloat16)) is None
    assert fn(**dict(ok, dtype=torch.float16, grad=False)) is None
    assert fn(**dict(ok, hidden=HMAX)) is None
    assert "HIP device" in fn(**dict(ok, is_cuda=False))
    assert "float64" in fn(**dict(ok, dtype=torch.float64))
    assert "float16 with gradients" in fn(**dict(ok, dtype=torch.float16))
    assert f"hidden = {HMAX + 1}" in fn(**dict(ok, hidden=HMAX + 1))
    assert "rows = 0" in fn(**dict(ok, rows=0))
    assert "bfloat16 parameters" in fn(**dict(ok, param_dtype=torch.bfloat16))
    assert "another" in fn(**dict(ok, foreign=True))
    # the measured classes: the launch only where it was ahead beyond the spread in both runs
    ahead = {(torch.float32, False): {(256, 192), (256, 384), (64, 768), (256, 768)},
             (torch.float32, True): {(256, 384), (256, 768)},
             (torch.bfloat16, False): {(256, 192), (256, 384), (64, 768), (256, 768)},
             (torch.bfloat16, True): {(256, 192), (256, 384), (256, 768)}}
    for B in (1, 64, 256):
        for hidden in (192, 384, 768):
            for (dt, grad), yes in ahead.items():
                assert ops.prenorm_pays(B * 197, hidden, dt, grad) is ((B, hidden) in yes), (B, hidden, dt, grad)
    assert ops.prenorm_pays(256 * 197, 768, torch.float16, False) and not ops.prenorm_pays(197, 768, torch.float16, False)


def tail_case(dtype, shape, p, p_path, seed=5):
    g = torch.Generator().manual_seed(seed)
    C_ = shape[-1]
    x = torch.randn(shape, generator=g, dtype=dtype).requires_grad_()
    b = torch.randn(shape, generator=g, dtype=dtype).requires_grad_()
    w = (1 + 0.5 * torch.randn(C_, generator=g, dtype=dtype)).requires_grad_()
    beta = torch.randn(C_, generator=g, dtype=dtype).requires_grad_()
    keep = HF.residual_keep_mask(shape, p, "cpu", generator=g) if p else None
    path_keep = HF.drop_path_keep_mask(shape[0], p_path, "cpu", generator=g) if p_path else None
    g_s, g_y = torch.randn(shape, generator=g, dtype=dtype), torch.randn(shape, generator=g, dtype=dtype)
    return x, b, w, beta, keep, path_keep, g_s, g_y


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 2e-5)], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(3, 7, 45), (6, 33)], ids=["BNC", "rowsC"])
@pytest.mark.parametrize("p,p_path", [(0.0, 0.0), (0.25, 0.0), (0.0, 0.5), (0.25, 0.5)])
def test_composed_route_on_the_cpu_is_the_restatement(p, p_path, shape, dtype, tol):
    """float64: 1e-12 of the largest magnitude (one formula twice).  float32: 2e-5, some hundred units of 2^-23 for
    sums of 45 terms in another order."""
    x, b, w, beta, keep, path_keep, g_s, g_y = tail_case(dtype, shape, p, p_path)
    nper = shape[1] if len(shape) == 3 else 1
    if p_path:
        path_keep[0], path_keep[1] = 0, 1                 # one dropped, one kept, whatever the draw
    s_ref, _, factor = R.stream(x, b, p, keep, p_path, path_keep, nper)
    ln = R.layer_norm(s_ref, w, beta)
    gr = R.tail_grads(s_ref, w, factor, g_y, g_s)
    training = bool(p or p_path)
    for fn in (HF.add_layer_norm_composed, HF.add_layer_norm):
        s, y = fn(x, b, w, beta, dropout_p=p, drop_path_p=p_path, training=training, keep=keep, path_keep=path_keep)
        assert s.shape == shape and y.shape == shape
        grads = torch.autograd.grad([s, y], [x, b, w, beta], [g_s, g_y])
        for key, got, want in [("s", s, s_ref), ("y", y, ln["y"])] + list(zip(("dx", "db", "dgamma", "dbeta"), grads,
                                                                              (gr[k] for k in ("dx", "db", "dgamma", "dbeta")))):
            err = float((got.detach().double().reshape(want.shape) - want).abs().max())
            assert err <= tol * float(want.abs().max()), (key, err)
    if p_path:
        assert torch.equal(s[0], x[0]) and float(grads[1][0].abs().max()) == 0.0       # the dropped sample
    # one gradient alone
    s, y = HF.add_layer_norm_composed(x, b, w, beta, dropout_p=p, drop_path_p=p_path, training=training, keep=keep,
                                      path_keep=path_keep)
    only_s = torch.autograd.grad(s, [x, b], g_s, retain_graph=True)
    want = R.tail_grads(s_ref, w, factor, None, g_s)
    assert float((only_s[1].double().reshape(want["db"].shape) - want["db"]).abs().max()) <= tol * float(want["db"].abs().max())
    assert float(want["dgamma"].abs().max()) == 0.0


def test_composed_route_draws_masks_and_argument_errors():
    x, b, w, beta, keep, path_keep, _, _ = tail_case(torch.float32, (4, 5, 8), 0.5, 0.5)
    torch.manual_seed(1)
    a = HF.add_layer_norm_composed(x, b, w, beta, dropout_p=0.5, drop_path_p=0.5, training=True)
    torch.manual_seed(1)
    c = HF.add_layer_norm_composed(x, b, w, beta, dropout_p=0.5, drop_path_p=0.5, training=True)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    ev = HF.add_layer_norm_composed(x, b, w, beta, dropout_p=0.5, drop_path_p=0.5, training=False)
    assert torch.equal(ev[0], x + b) and not torch.equal(ev[0], a[0])
    # timm's DropPath arithmetic on the same draw
    torch.manual_seed(2)
    mine = HF.add_layer_norm_composed(x, b, w, beta, drop_path_p=0.5, training=True)[0]
    torch.manual_seed(2)
    mod = VL.DropPath(0.5).train()
    assert torch.equal(mine, x + mod(b))
    torch.manual_seed(2)
    want = b.div(0.5) * (0.5 + torch.rand(4, 1, 1)).floor_()
    torch.manual_seed(2)
    assert torch.equal(mod(b), want)
    assert VL.DropPath(0.5).eval()(b) is b
    m = HF.drop_path_keep_mask(64, 0.3, "cpu", generator=torch.Generator().manual_seed(1))
    m2 = HF.drop_path_keep_mask(64, 0.3, "cpu", generator=torch.Generator().manual_seed(1))
    assert m.dtype == torch.uint8 and m.shape == (64,) and torch.equal(m, m2) and 0 < int(m.sum()) < 64
    with pytest.raises(ValueError):
        HF.add_layer_norm(x, b, w, beta, route="fastest")
    with pytest.raises(_cabi.TadmmError, match="HIP device"):
        HF.add_layer_norm(x, b, w, beta, route="launch")              # CPU tensors: there is no CPU kernel
    for bad in (dict(weight=w[:-1]), dict(branch=b[:1]), dict(dropout_p=1.0), dict(drop_path_p=-0.1),
                dict(keep=keep[:1]), dict(path_keep=path_keep[:2]), dict(x=x[0, 0], branch=b[0, 0])):
        kw = dict(x=x, branch=b, weight=w, bias=beta)
        kw.update(bad)
        with pytest.raises(ValueError):
            HF.add_layer_norm(kw.pop("x"), kw.pop("branch"), kw.pop("weight"), kw.pop("bias"), **kw)


def randomise(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, prm in mod.named_parameters():
            if name.endswith("norm1.weight") or name.endswith("norm2.weight") or name == "norm.weight":
                prm.copy_(1 + 0.3 * torch.randn(prm.shape, generator=g))
            elif prm.dim() == 1:
                prm.copy_(0.2 * torch.randn(prm.shape, generator=g))
    return mod


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-11), (torch.float32, 1e-4)], ids=["f64", "f32"])
def test_dense_block_on_the_cpu_is_the_restatement(dtype, tol):
    """An empty rank table: every projection is nn.Linear.  Output and every parameter gradient, max norm."""
    torch.manual_seed(0)
    blk = randomise(VL.TTBlock(32, 4, qkv_bias=True, linear=VL.TTLinearM, block_id=0, hp_dict=NoRanks), 1).to(dtype).eval()
    assert all(isinstance(m, torch.nn.Linear) for m in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2))
    x, up = torch.randn(2, 5, 32, dtype=dtype), torch.randn(2, 5, 32, dtype=dtype)
    sd = R.state64(blk, requires_grad=True)
    assert blk.norm1.eps == 1e-5                                       # nn.LayerNorm's own default, as in timm's Block
    want = R.block(R.f64(x), sd, "", 4, eps=1e-5)
    names = [n for n, _ in blk.named_parameters()]
    want_g = torch.autograd.grad(want, [sd[n] for n in names], R.f64(up))
    got = blk(x)
    got_g = torch.autograd.grad(got, list(blk.parameters()), up)
    for key, a, b in [("out", got, want)] + list(zip(names, got_g, want_g)):
        assert float((a.detach().double() - b.detach()).abs().max()) <= tol * float(b.abs().max()), key
    # the chained form: the caller's norm1, and the next LayerNorm from the second tail
    nxt = torch.nn.LayerNorm(32, eps=1e-6).to(dtype)
    out, normed = blk(x, blk.norm1(x), nxt)
    assert torch.allclose(out, got, rtol=0, atol=1e-6) and torch.allclose(normed, nxt(got), rtol=0, atol=1e-5)
    # a norm layer that is not nn.LayerNorm: plain composition
    odd = VL.TTBlock(32, 4, norm_layer=lambda d: torch.nn.GroupNorm(1, d), hp_dict=NoRanks, block_id=0)
    with pytest.raises(Exception):
        odd(torch.randn(2, 5, 32))                                     # GroupNorm wants (B, C, ...): it was really called
    ident = VL.TTBlock(32, 4, norm_layer=lambda d: torch.nn.Identity(), hp_dict=NoRanks, block_id=0).eval()
    xi = torch.randn(2, 5, 32)
    o, n = ident(xi, None, torch.nn.Identity())
    assert torch.equal(o, n) and torch.equal(o, ident(xi))
    assert blk.set_route("composed") is blk and blk.route == "composed" and blk.attn.route == "composed"


@pytest.mark.parametrize("distilled", [False, True], ids=["plain", "distilled"])
def test_small_model_on_the_cpu_is_the_restatement(distilled):
    torch.manual_seed(3)
    kw = dict(img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=2, num_classes=10, distilled=distilled,
              drop_path_rate=0.5, hp_dict=NoRanks)
    model = randomise(VL.TTVisionTransformer(**kw), 4).eval()
    img = torch.randn(3, 3, 32, 32)
    want = R.vit(R.f64(img), R.state64(model), 2, 2, 16)
    got = model(img)
    assert got.shape == (3, 10)
    assert float((got.detach().double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
    want64 = model.double()(img.double())
    assert float((want64.detach() - want).abs().max()) <= 1e-11 * float(want.abs().max())
    model.float().train()
    assert [b.drop_path.drop_prob if isinstance(b.drop_path, VL.DropPath) else 0.0 for b in model.blocks] == [0.0, 0.5]
    torch.manual_seed(8)
    a = model(img)
    torch.manual_seed(8)
    b = model(img)
    if distilled:
        assert isinstance(a, tuple) and len(a) == 2 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    else:
        assert torch.equal(a, b)
    keys = list(model.state_dict())
    assert keys[:3 if distilled else 2] == (["cls_token", "dist_token", "pos_embed"] if distilled else ["cls_token", "pos_embed"])
    assert ("head_dist.weight" in keys) == distilled and model.pos_embed.shape == (1, 4 + (2 if distilled else 1), 64)
    other = VL.TTVisionTransformer(**kw)
    other.load_state_dict(model.state_dict())
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in model.state_dict().items())
    with pytest.raises(ValueError, match="doesn't match"):
        model(torch.randn(1, 3, 48, 48))
    with pytest.raises(NotImplementedError):
        VL.TTVisionTransformer(representation_size=64, hp_dict=NoRanks, depth=1)


def test_factories_argument_errors(tmp_path):
    assert len(VL.FACTORIES) == 12 and "ttm_vit_small_patch16_224" in VL.FACTORIES and "tkr_deit_small_patch16_224" in VL.FACTORIES
    small = dict(img_size=32, depth=1, num_classes=5)               # keyword arguments override the architecture's
    for name in VL.FACTORIES:
        fn = getattr(VL, name)
        assert fn.__name__ == name
    fn = VL.ttm_deit_tiny_patch16_224
    with pytest.raises(ValueError, match="nothing is downloaded"):
        fn(NoRanks, decompose=True, **small)
    with pytest.raises(ValueError, match="URL"):
        fn(NoRanks, decompose=True, path="https://example.org/deit.pth", **small)
    with pytest.raises(ValueError, match="nothing is downloaded"):
        fn(NoRanks, pretrained=True, **small)
    dense = fn(NoRanks, **small)
    assert dense.embed_dim == 192 and dense.blocks[0].attn.num_heads == 3 and isinstance(dense.blocks[0].attn.qkv, torch.nn.Linear)
    sd = {k: v + 1 for k, v in dense.state_dict().items()}
    again = fn(NoRanks, decompose=True, dense_dict=sd, **small)
    assert all(torch.equal(v, sd[k]) for k, v in again.state_dict().items())
    path = os.path.join(tmp_path, "dense.pth")
    torch.save(sd, path)
    for kw in (dict(decompose=True), dict(pretrained=True)):
        loaded = fn(NoRanks, path=path, **kw, **small)
        assert all(torch.equal(v, sd[k]) for k, v in loaded.state_dict().items())
    assert VL.tkr_vit_small_patch16_224(NoRanks, **small).embed_dim == 384


def test_import_lines():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import vit_tt as D; import tadmm; from tadmm import vit_layers as V; "
            "names = ['DropPath', 'PatchEmbed', 'TTAttention', 'TTMlp', 'TTBlock', 'TTVisionTransformer'] + list(V.FACTORIES); "
            "assert len(names) == 18; "
            "assert all(getattr(D, n) is getattr(V, n) and getattr(tadmm, n) is getattr(V, n) for n in names)")
    subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "dnn-compression-tensor-admm_amd", "dropin")], check=True)
