"""SVD layers (SVDConv.py) on the MI355X: the fused 1x1 chain entries (tadmm_svdconv_fwd / _bwd) against fp64, the
layers against the G8 fixtures recorded from the reference, autograd, fallbacks, caches, the `--decompose` hand-off
and one ADMM round trip.

Kernel tolerances as tests/test_gpu_chain.py: fp32 (three-plane split) <= 2e-6 of max|y|, bf16 <= 2e-2."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


class HP:
    def __init__(self, ranks):
        self.ranks = ranks


def _ops():
    from tadmm import ops
    return ops


def _rel(y, ref):
    return (y.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _chain_ref(x, win, wout, bias):
    """fp64 y[b,:,p] = wout (win x[b,:,p]) + bias"""
    h = torch.einsum("rc,bcp->brp", win.double(), x.double().flatten(2))
    y = torch.einsum("nr,brp->bnp", wout.double(), h)
    if bias is not None:
        y = y + bias.double()[None, :, None]
    return y.reshape(x.shape[0], wout.shape[0], *x.shape[2:])


# (B, C_in, (H, W), rank, C_out, bias): ranks 1 17 64 65 192 256, planes 1 49 196 784 3136, batch 1 and 128,
# MobileNetV2-CIFAR (bottlenecks.3.conv1, 16x16 stage) and ResNet-50 (layer1.x.conv3 56x56, layer4.x.conv1 7x7) at size
KERNEL_CASES = [
    (1, 24, (1, 1), 1, 144, True),
    (128, 24, (1, 1), 17, 144, False),
    (1, 64, (7, 7), 64, 256, True),
    (3, 48, (7, 7), 17, 300, False),          # more than 256 output features, images straddle token tiles
    (2, 65, (14, 14), 65, 96, False),
    (128, 96, (14, 14), 192, 40, True),
    (4, 144, (28, 28), 256, 24, True),
    (128, 24, (16, 16), 18, 144, True),       # svd_mobilenetv2_cifar bottlenecks.3.conv1
    (8, 64, (56, 56), 32, 256, True),         # tk_resnet50 3x layer1.x.conv3
    (128, 2048, (7, 7), 96, 512, True),       # tk_resnet50 3x layer4.x.conv1
    (1, 32, (56, 56), 256, 64, False),
]


def _case_tensors(B, cin, hw, r, cout, bias, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, *hw, generator=g).to(DEV)
    win = (torch.randn(r, cin, generator=g) / cin ** 0.5).to(DEV)
    wout = (torch.randn(cout, r, generator=g) / r ** 0.5).to(DEV)
    b = torch.randn(cout, generator=g).to(DEV) if bias else None
    return x, win, wout, b


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,cin,hw,r,cout,bias", KERNEL_CASES)
def test_svdconv_entries_match_fp64(B, cin, hw, r, cout, bias, dtype):
    ops = _ops()
    x, win, wout, b = _case_tensors(B, cin, hw, r, cout, bias, B * 1000 + cin + r)
    P, tol = (3, 2e-6) if dtype == torch.float32 else (1, 2e-2)
    x = x.to(dtype)
    pin, pout = ops.weight_planes(win, P, pad_rows=64), ops.weight_planes(wout, P, pad_cols=64)
    if dtype == torch.bfloat16:                    # the reference multiplies the rounded weights
        win_r, wout_r = ops.unpack_planes(pin)[0, :r, :cin].float(), ops.unpack_planes(pout)[0, :cout, :r].float()
    else:
        win_r, wout_r = win, wout
    y = ops.svd_conv(x, pin, pout, b, cout)
    assert y.shape == (B, cout, *hw) and y.dtype == dtype and y.is_contiguous()
    err = _rel(y, _chain_ref(x, win_r, wout_r, b))
    assert err < tol, err
    # data gradient: dX = Win^T (Wout^T dY), the same kernel on the transposed factor planes
    g = torch.randn(B, cout, *hw, generator=torch.Generator().manual_seed(5)).to(DEV).to(dtype)
    qin, qout = ops.weight_planes(wout.t(), P, pad_rows=64), ops.weight_planes(win.t(), P, pad_cols=64)
    if dtype == torch.bfloat16:
        wt_in, wt_out = ops.unpack_planes(qin)[0, :r, :cout].float(), ops.unpack_planes(qout)[0, :cin, :r].float()
    else:
        wt_in, wt_out = wout.t(), win.t()
    gx = ops.svd_conv(g, qin, qout, None, cin, entry="tadmm_svdconv_bwd")
    assert gx.shape == x.shape
    err = _rel(gx, _chain_ref(g, wt_in, wt_out, None))
    assert err < tol, err


def test_svdconv_entry_validation():
    from tadmm._cabi import TadmmError
    ops = _ops()
    x, win, wout, b = _case_tensors(2, 16, (5, 5), 8, 24, True, 1)
    pin, pout = ops.weight_planes(win, 3, pad_rows=64), ops.weight_planes(wout, 3, pad_cols=64)
    # token rows instead of an image: refused with a message that names the entry's contract
    with pytest.raises(TadmmError, match="svdconv: x_hw and y_hw"):
        ops._chain_call("tadmm_svdconv_fwd", x.permute(0, 2, 3, 1).reshape(-1, 16).contiguous(), pin, pout, b, 16, 64,
                        24, False, 0)
    # rank above 256
    big_in, big_out = torch.randn(320, 16, device=DEV), torch.randn(24, 320, device=DEV)
    with pytest.raises(TadmmError, match="at most 256"):
        ops.svd_conv(x, ops.weight_planes(big_in, 3, pad_rows=64), ops.weight_planes(big_out, 3, pad_cols=64), b, 24)
    # the TT-linear entry keeps refusing image descriptors as before
    with pytest.raises(TadmmError, match="token tile does not fit"):
        ops._chain_call("tadmm_ttlinear_fwd", x, pin, pout, b, 16, 64, 24, True, 0)


# ------------------------------------------------------------------------------------------------ layers against G8
@pytest.fixture(scope="module")
def g8(golden_dir):
    return (np.load(os.path.join(golden_dir, "g8_svd_layers.npz")),
            json.load(open(os.path.join(golden_dir, "g8_svd_layers.json"))))


def _classes():
    from tadmm import svd_layers
    return {"R": svd_layers.SVDConv2dR, "C": svd_layers.SVDConv2dC, "M": svd_layers.SVDConv2dM}


# (name of U, name of diag(s) V^T) per class, and whether they are 1x1 kernels
_FACTORS = {"R": ("left_factor", "right_factor"), "C": ("right_kernel", "left_kernel"), "M": ("right_factor", "left_factor")}


def _build_from_g8(data, key, m):
    wd = torch.from_numpy(data[key + "_w"]).to(DEV)
    bd = torch.from_numpy(data[key + "_b"]).to(DEV) if m["bias"] else None
    return _classes()[m["cls"]](m["in_channels"], m["out_channels"], 1, padding=m["padding"], bias=m["bias"],
                                hp_dict=HP({"l.weight": m["rank"]}), name="l.weight", dense_w=wd, dense_b=bd)


def test_layers_match_g8(g8):
    data, meta = g8
    for key, m in meta["cases"].items():
        layer = _build_from_g8(data, key, m)
        sd = layer.state_dict()
        assert [[n, list(t.shape)] for n, t in sd.items()] == m["state_dict"], key
        # factors up to the sign of each singular pair
        un, svn = _FACTORS[m["cls"]]
        u, sv = sd[un].reshape(sd[un].shape[0], -1).cpu().numpy(), sd[svn].reshape(sd[svn].shape[0], -1).cpu().numpy()
        ru = data[f"{key}_sd_{un}"].reshape(u.shape)
        rsv = data[f"{key}_sd_{svn}"].reshape(sv.shape)
        sign = np.sign(np.sum(u * ru, axis=0))
        assert np.all(sign != 0), key
        for a, ra in ((u * sign, ru), (sv * sign[:, None], rsv)):
            np.testing.assert_allclose(a, ra, rtol=0, atol=2e-5 * max(1.0, np.abs(ra).max()), err_msg=key)
        if m["bias"]:
            np.testing.assert_array_equal(sd["bias"].cpu().numpy(), data[key + "_b"])
        x = torch.from_numpy(data[key + "_x"]).to(DEV)
        with torch.no_grad():
            y = layer(x)
        ref = data[key + "_y"]
        assert tuple(y.shape) == ref.shape, key
        err = np.abs(y.cpu().numpy() - ref).max() / np.abs(ref).max()
        assert err <= 1e-5, (key, err)


def test_forward_flops_matches_g8(g8, capsys):
    data, meta = g8
    n = 0
    for key, m in meta["cases"].items():
        if m["cls"] != "C":
            continue
        layer = _build_from_g8(data, key, m)
        capsys.readouterr()
        with torch.no_grad():
            out, base, compr = layer.forward_flops(torch.from_numpy(data[key + "_x"]).to(DEV))
        assert capsys.readouterr().out == m["flops_line"], key
        assert base == m["base_flops"] and compr == m["compr_flops"], key
        assert layer.extra_repr() == m["extra_repr"]
        n += 1
    assert n >= 3


def test_eligible_forward_is_the_fused_entry(monkeypatch):
    ops = _ops()
    calls = []
    real = ops.svd_conv
    monkeypatch.setattr(ops, "svd_conv", lambda *a, **k: calls.append(k.get("entry", "fwd")) or real(*a, **k))
    for cls in ("C", "M"):
        layer = _classes()[cls](64, 256, 1, hp_dict=HP({"l.weight": 32}), name="l.weight").to(DEV)
        x = torch.randn(2, 64, 7, 7, device=DEV)
        with torch.no_grad():
            y = layer(x.bfloat16())                 # bf16: one fused launch (ops.svd_conv_pays)
            assert calls == ["fwd"] * (1 + (cls == "M"))
            y32 = layer(x)                          # fp32: two tadmm_tucker_1x1 launches (measured faster)
            assert calls == ["fwd"] * (1 + (cls == "M"))
        assert y.dtype == torch.bfloat16 and _rel(y.float(), y32.double()) < 2e-2


def test_conv1x1_chain_autograd_fp32():
    from tadmm import functional as HF
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 40, 7, 7, generator=g).to(DEV).requires_grad_()
    wi = (torch.randn(20, 40, generator=g) / 40 ** 0.5).to(DEV).requires_grad_()
    wo = (torch.randn(72, 20, generator=g) / 20 ** 0.5).to(DEV).requires_grad_()
    b = torch.randn(72, generator=g).to(DEV).requires_grad_()
    gout = torch.randn(3, 72, 7, 7, generator=g).to(DEV)
    y = HF.conv1x1_chain(x, wi, wo, b)
    (y * gout).sum().backward()
    leaves = [t.detach().double().requires_grad_() for t in (x, wi, wo, b)]
    y64 = F.conv2d(F.conv2d(leaves[0], leaves[1][:, :, None, None]), leaves[2][:, :, None, None], leaves[3])
    (y64 * gout.double()).sum().backward()
    assert _rel(y.detach(), y64.detach()) < 2e-6
    for t, r, what in zip((x, wi, wo, b), leaves, ("dX", "dWin", "dWout", "dbias")):
        assert _rel(t.grad, r.grad) < 1e-5, what


# ------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("cls,bias,hw", [("C", True, (7, 7)), ("C", False, (16, 16)), ("M", True, (16, 16)),
                                         ("M", False, (7, 7))])
def test_autograd_matches_fp64(cls, bias, hw):
    torch.manual_seed(3)
    layer = _classes()[cls](24, 144, 1, bias=bias, hp_dict=HP({"l.weight": 18}), name="l.weight").to(DEV)
    if bias:
        with torch.no_grad():
            layer.bias.normal_()
    x = torch.randn(4, 24, *hw, device=DEV, requires_grad=True)
    gout = torch.randn(4, 144, *hw, device=DEV)
    y = layer(x)
    (y * gout).sum().backward()
    if cls == "C":
        wi, wo = layer.left_kernel, layer.right_kernel
    else:
        wi, wo = layer.left_factor, layer.right_factor
    wi64 = wi.detach().double().reshape(18, 24).requires_grad_()
    wo64 = wo.detach().double().reshape(144, 18).requires_grad_()
    b64 = layer.bias.detach().double().requires_grad_() if bias else None
    x64 = x.detach().double().requires_grad_()
    y64 = F.conv2d(F.conv2d(x64, wi64[:, :, None, None]), wo64[:, :, None, None], b64)
    (y64 * gout.double()).sum().backward()
    assert _rel(y.detach(), y64.detach()) < 2e-6
    for got, ref, what in ((x.grad, x64.grad, "dX"), (wi.grad.reshape(18, 24), wi64.grad, "dWin"),
                           (wo.grad.reshape(144, 18), wo64.grad, "dWout")):
        assert _rel(got, ref) < 1e-5, what
    if bias:
        assert _rel(layer.bias.grad, b64.grad) < 1e-5


# ------------------------------------------------------------------------------------------------ fallbacks, caches
def test_padding_falls_back_to_reference_composition():
    layer = _classes()["C"](16, 32, 1, padding=1, hp_dict=HP({"l.weight": 8}), name="l.weight").to(DEV)
    with torch.no_grad():
        layer.bias.normal_()
        x = torch.randn(2, 16, 5, 5, device=DEV)
        y = layer(x)
    assert y.shape == (2, 32, 7, 7)
    ref = F.conv2d(F.conv2d(x.double(), layer.left_kernel.double()), layer.right_kernel.double(), layer.bias.double(),
                   padding=1)
    assert _rel(y, ref) < 1e-5
    torch.testing.assert_close(y[:, :, 0, 0], layer.bias.detach().expand(2, 32))   # the border is the bias


def test_other_dtype_takes_reference_composition():
    for cls in ("C", "M"):
        layer = _classes()[cls](24, 40, 1, hp_dict=HP({"l.weight": 6}), name="l.weight").to(DEV).double()
        x = torch.randn(2, 24, 5, 5, device=DEV, dtype=torch.float64)
        with torch.no_grad():
            y = layer(x)
            wi = (layer.left_kernel if cls == "C" else layer.left_factor).reshape(6, 24)
            wo = (layer.right_kernel if cls == "C" else layer.right_factor).reshape(40, 6)
        assert y.dtype == torch.float64
        torch.testing.assert_close(y, _chain_ref(x, wi, wo, layer.bias.detach()), rtol=1e-12, atol=1e-12)


def test_rank_512_vgg16_fc2_takes_two_launches():
    # tk_vgg16_bn 10x pre_logits.fc2: 1x1 convolution 4096 -> 4096 on a 1x1 plane, rank 512
    ops = _ops()
    layer = _classes()["C"](4096, 4096, 1, hp_dict=HP({"pre_logits.fc2.weight": [512]}), name="pre_logits.fc2.weight")
    layer = layer.to(DEV)
    assert not ops.svd_conv_pays(torch.empty(1, 4096, 1, 1, device=DEV), 512)
    with torch.no_grad():
        layer.bias.normal_()
        for dtype, tol in ((torch.float32, 2e-6), (torch.bfloat16, 2e-2)):
            x = torch.randn(16, 4096, 1, 1, device=DEV).to(dtype)
            y = layer(x)
            ref = _chain_ref(x.float(), layer.left_kernel.reshape(512, 4096), layer.right_kernel.reshape(4096, 512),
                             layer.bias)
            assert y.dtype == dtype and _rel(y, ref) < tol


def test_inference_cache_follows_parameter_updates():
    for cls in ("C", "M"):
        layer = _classes()[cls](24, 144, 1, hp_dict=HP({"l.weight": 18}), name="l.weight").to(DEV).eval()
        x = torch.randn(2, 24, 16, 16, device=DEV)
        params = list(layer.parameters())
        with torch.no_grad():
            y0 = layer(x)
        opt = torch.optim.SGD(params, lr=0.1)
        for p in params:
            p.grad = torch.ones_like(p)
        opt.step()                                  # in-place update: version counters move, addresses stay
        with torch.no_grad():
            y1 = layer(x)
            wi = params[1].reshape(18, 24)
            wo = params[2].reshape(144, 18)
            ref = _chain_ref(x, wi, wo, params[0])
        assert _rel(y1, ref) < 2e-6 and _rel(y0, ref) > 1e-3


# ------------------------------------------------------------------------------------------------ decompose
def _table_model(key, seed=0):
    from tadmm import hp, workloads
    table = hp.table(key)
    fn = workloads.shape_fn_for(key)
    shapes = {name: fn(name) for name in table.ranks}
    return workloads.SyntheticModel(shapes, seed), table


def _truncate64(w, r):
    u, s, vt = torch.linalg.svd(w.double().reshape(w.shape[0], -1), full_matrices=False)
    return ((u[:, :r] * s[:r]) @ vt[:r]).reshape(w.shape)


@pytest.mark.parametrize("variant", ["R", "C", "M"])
def test_decompose_svd_mobilenetv2_cifar(variant):
    from tadmm.decompose import decompose_state_dict
    model, table = _table_model("svd_mobilenetv2_cifar_hp.HyperParamsDictRatio2x")
    assert len(table.ranks) == 28
    dense = {n: p.detach() for n, p in model.named_parameters()}
    dense["head.bias"] = torch.randn(10)
    sd = decompose_state_dict(dense, table, "svd", variant)
    assert torch.equal(sd["head.bias"], dense["head.bias"])
    cls = _classes()[variant]
    names = list(table.ranks)
    for name in names[:3] + names[-3:]:
        w = dense[name]
        o, i = w.shape[:2]
        r = table.ranks[name]
        r = r if isinstance(r, int) else r[0]
        # (SVDConv2dR cannot be built without dense_w unless in == out: the reference's reset_parameters)
        layer = cls(i, o, 1, bias=False, hp_dict=table, name=name, dense_w=w if variant == "R" else None)
        p = name[:-len("weight")]
        own = {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
        assert sorted(own) == sorted(layer.state_dict()), name
        assert all(own[k].shape == t.shape for k, t in layer.state_dict().items()), name
        if variant == "R":                          # the reference's (O, r) / (r, I) layout, not the declared one
            layer.left_factor.data = own["left_factor"]
            layer.right_factor.data = own["right_factor"]
        else:
            layer.load_state_dict(own)
        layer = layer.to(DEV)
        x = torch.randn(2, i, 4, 4, device=DEV)
        with torch.no_grad():
            y = layer(x)
        ref = F.conv2d(x.double(), _truncate64(w, r).to(DEV))
        assert _rel(y, ref) < 2e-5, name


def test_decompose_tk_resnet50_single_rank_entries():
    from tadmm import tucker
    from tadmm.decompose import decompose_state_dict
    model, table = _table_model("tk_resnet50_hp.HyperParamsDictRatio3x")
    dense = {n: p.detach() for n, p in model.named_parameters()}
    sd = decompose_state_dict(dense, table, "tk", "C")
    single = [n for n, r in table.ranks.items() if len(r) == 1]
    multi = [n for n, r in table.ranks.items() if len(r) > 1]
    assert len(single) == 28 and len(multi) == 16
    for name in single:
        p = name[:-len("weight")]
        w = dense[name]
        assert sd[p + "left_kernel"].shape == (table.ranks[name][0], w.shape[1], 1, 1)
        assert sd[p + "right_kernel"].shape == (w.shape[0], table.ranks[name][0], 1, 1)
        rec = (sd[p + "right_kernel"].flatten(1).double() @ sd[p + "left_kernel"].flatten(1).double())
        assert _rel(rec, _truncate64(w, table.ranks[name][0]).reshape(rec.shape)) < 2e-5, name
    # the Tucker entries come out of the same grouped plan as before
    ws = [dense[n].to(DEV).float().contiguous() for n in multi]
    res = tucker._plan_decompose(ws, [table.ranks[n] for n in multi])
    for name, (core, (u_out, u_in), _, _) in zip(multi, res):
        p = name[:-len("weight")]
        torch.testing.assert_close(sd[p + "core_kernel"], core.cpu(), rtol=0, atol=1e-6)
        torch.testing.assert_close(sd[p + "first_kernel"], u_in.t().cpu()[:, :, None, None], rtol=0, atol=1e-6)
        torch.testing.assert_close(sd[p + "last_kernel"], u_out.cpu()[:, :, None, None], rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------------ end to end
def test_admm_svd_then_decompose_reproduces_z():
    from tadmm.admm import ADMM
    from tadmm.decompose import decompose_state_dict

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(11)
            self.a = torch.nn.Conv2d(32, 96, 1, bias=False)
            self.b = torch.nn.Conv2d(96, 40, 1)
            with torch.no_grad():
                self.a.weight.copy_(torch.randn(96, 32, 1, 1, generator=g))
                self.b.weight.copy_(torch.randn(40, 96, 1, 1, generator=g))

    ranks = {"a.weight": 12, "b.weight": 20}
    model = M().to(DEV)
    admm = ADMM(model, 1e-3, HP(dict(ranks)), "svd", DEV)
    admm.update()
    dense = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for k in ranks:
        dense[k] = admm.z[k].detach().cpu()
    sd = decompose_state_dict(dense, HP(dict(ranks)), "svd", "C")
    x = torch.randn(2, 32, 9, 9, device=DEV)
    for name, cin, cout, bias in (("a", 32, 96, False), ("b", 96, 40, True)):
        layer = _classes()["C"](cin, cout, 1, bias=bias, hp_dict=HP(dict(ranks)), name=name + ".weight")
        layer.load_state_dict({k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")})
        layer = layer.to(DEV)
        with torch.no_grad():
            y = layer(x)
            ref = F.conv2d(x.double(), admm.z[name + ".weight"].double(),
                           None if not bias else model.b.bias.double())
        assert _rel(y, ref) < 2e-5, name
        x = torch.randn(2, 96, 9, 9, device=DEV)
