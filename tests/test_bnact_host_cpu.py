"""Host side of the ResNet block tail and the ResNets (no GPU): every refusal of the C entries of csrc/bnact.hip, the
workspace and fits queries, the refusal function and the routing, the composed route of `batch_norm_act` and the dense
blocks and small models of tadmm/resnet_cifar_layers.py / resnet_inet_layers.py against the float64 restatement of
tests/_resnet_ref.py, the state-dict keys of two shipped tables, the factories' argument errors and the import lines."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import _resnet_ref as R
from tadmm import _cabi, get_hp_dict, ops
from tadmm import functional as HF
from tadmm import resnet_cifar_layers as RC
from tadmm import resnet_inet_layers as RI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_M = 2 ** 31 - 4096


class NoRanks:
    ranks = {}
    tt_shapes = {}


def test_descriptor_size_fits_and_workspace():
    lib = _cabi.load()
    assert lib.tadmm_bnact_desc_bytes() == C.sizeof(_cabi.BnActDesc)
    assert ops.bnact_max_m() == MAX_M
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert ops.bnact_fits(1, 1, 1, 1, dt) is True and ops.bnact_fits(128, 16, 32, 32, dt) is True
        assert ops.bnact_fits(2 ** 15, 3, 2 ** 8, 2 ** 8 - 1, dt) is True          # 2^31 - 2^23 values
        assert ops.bnact_fits(2 ** 15, 3, 2 ** 8, 2 ** 8, dt) is False             # 2^31 values per channel
    for shape in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, -1, 1), (1, 1, 1, 0)):
        with pytest.raises(_cabi.TadmmError):
            ops.bnact_fits(*shape)
        with pytest.raises(_cabi.TadmmError):
            ops.bnact_workspace_bytes(*shape)
    m = C.c_int64(7)
    assert lib.tadmm_bnact_fits(None, C.byref(m)) == -1 and m.value == MAX_M
    assert lib.tadmm_bnact_fits(None, None) == -1
    # a pair of doubles per channel and split; min(trips, 128, ceil(2048 / C)) splits, trips of 1024 / 2048 values
    assert ops.bnact_workspace_bytes(1, 1, 1, 1) == 256
    assert ops.bnact_workspace_bytes(128, 16, 32, 32) == 16 * 128 * 16              # the CIFAR stem: 128 trips, 128 splits
    assert ops.bnact_workspace_bytes(128, 16, 32, 32, torch.bfloat16) == 16 * 64 * 16
    assert ops.bnact_workspace_bytes(2, 2048, 7, 7) == 2048 * 16                    # one split
    assert ops.bnact_workspace_bytes(32, 64, 56, 56) == 64 * 32 * 16                # 98 trips, ceil(2048 / 64) splits
    assert ops.bnact_workspace_bytes(9, 1, 256, 257) == 128 * 16                    # the cap
    assert ops.bnact_workspace_bytes(5, 3, 1, 1) == 256                             # 48 bytes, rounded up
    for dt in (torch.float32, torch.bfloat16):
        for c, h, w in ((1, 7, 7), (16, 32, 32), (64, 56, 56), (300, 5, 3)):
            sizes = [ops.bnact_workspace_bytes(n, c, h, w, dt) for n in (1, 2, 3, 5, 8, 21, 64, 65, 128, 1000)]
            assert sizes == sorted(sizes) and all(s % 16 == 0 and s > 0 for s in sizes), (c, h, w, sizes)
        sizes = [ops.bnact_workspace_bytes(4, 8, h, 33, dt) for h in range(1, 400, 13)]
        assert sizes == sorted(sizes)
    dsc = _cabi.BnActDesc()
    dsc.N, dsc.C, dsc.H, dsc.W, dsc.dtype = 2, 2, 2, 2, 7
    assert lib.tadmm_bnact_workspace_bytes(C.byref(dsc), C.byref(C.c_size_t())) == -1
    dsc.dtype = _cabi.CHAIN_F32
    assert lib.tadmm_bnact_workspace_bytes(C.byref(dsc), None) == -1
    assert lib.tadmm_bnact_workspace_bytes(None, C.byref(C.c_size_t())) == -1
    assert lib.tadmm_bnact_plan(C.byref(dsc), None) == -1 and lib.tadmm_bnact_plan(None, (C.c_int32 * 3)()) == -1
    dsc.dtype = 7
    assert lib.tadmm_bnact_plan(C.byref(dsc), (C.c_int32 * 3)()) == -1
    dsc.dtype = _cabi.CHAIN_F32
    dsc.N, dsc.H, dsc.W = 2 ** 15, 2 ** 8, 2 ** 8
    assert lib.tadmm_bnact_workspace_bytes(C.byref(dsc), C.byref(C.c_size_t())) == -5
    assert lib.tadmm_bnact_plan(C.byref(dsc), (C.c_int32 * 3)()) == -5


def test_plan_query():
    """`tadmm_bnact_plan`: S splits of `span` values, span a whole number of trips, `cap` what the workspace holds."""
    plan = ops.bnact_plan
    for shape in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, -1, 1), (1, 1, 1, 0)):
        with pytest.raises(_cabi.TadmmError):
            plan(*shape)
    assert plan(1, 1, 1, 1) == dict(S=1, span=1024, cap=1)
    assert plan(128, 16, 32, 32) == dict(S=128, span=1024, cap=128)                 # the CIFAR stem: a split per trip
    assert plan(128, 16, 32, 32, torch.bfloat16) == dict(S=64, span=2048, cap=64)
    assert plan(2, 2048, 7, 7) == dict(S=1, span=1024, cap=1)
    assert plan(15, 2048, 12, 12) == dict(S=1, span=3072, cap=1)                    # one workgroup walks three trips
    assert plan(15, 2048, 12, 12, torch.bfloat16) == dict(S=1, span=4096, cap=1)
    assert plan(9, 1, 256, 257) == dict(S=116, span=5120, cap=128)                  # 579 trips, 5 to a split: 116 of 128
    assert plan(32, 64, 56, 56) == dict(S=25, span=4096, cap=32)                    # 98 trips, 4 to a split
    assert plan(8, 3, 7, 7, torch.float16) == plan(8, 3, 7, 7, torch.bfloat16) == dict(S=1, span=2048, cap=1)
    for dt, trip in ((torch.float32, 1024), (torch.bfloat16, 2048), (torch.float16, 2048)):
        for n, c, h, w in ((1, 1, 1, 1), (7, 3, 33, 70), (128, 64, 8, 8), (32, 32, 112, 112), (5, 2000, 9, 1363),
                           (300, 1, 64, 64), (3, 40, 200, 31), (65, 2, 32, 32), (130, 2, 32, 32)):
            p, m = plan(n, c, h, w, dt), n * h * w
            trips = -(-m // trip)
            assert p["cap"] == min(trips, 128, -(-2048 // c)) and 1 <= p["S"] <= p["cap"], (n, c, h, w, p)
            assert p["span"] % trip == 0 and p["S"] * p["span"] >= m > (p["S"] - 1) * p["span"]   # covered, none empty
            assert p["span"] // trip == -(-trips // p["cap"])                                      # evened out
            assert c * p["cap"] * 16 <= ops.bnact_workspace_bytes(n, c, h, w, dt)


def test_launch_entries_refuse_before_launching():
    """No device is needed: every refusal comes before the first HIP call that would want one."""
    lib = _cabi.load()
    h = C.c_void_p()
    lib.tadmm_create(0, C.byref(h))
    assert h, "a handle needs no device"
    raw = (C.c_char * 32768)()
    p = C.addressof(raw) + (-C.addressof(raw)) % 16

    def desc(**kw):
        d = _cabi.BnActDesc()
        d.x, d.res = p, p + 1024
        strides = kw.pop("res_stride", (8 * 4 * 4, 4 * 4, 4, 1))
        for i, s in enumerate(strides):
            d.res_stride[i] = s
        d.gamma, d.beta, d.running_mean, d.running_var, d.num_batches_tracked = p + 2048, p + 2112, p + 2176, p + 2240, p + 2304
        d.y, d.stats, d.g = p + 3072, p + 4096, p + 5120
        d.dx, d.dres, d.dgamma, d.dbeta = p + 6144, p + 7168, p + 8192, p + 8256
        d.workspace, d.workspace_bytes = p + 9216, 256
        d.eps, d.momentum = 1e-5, 0.1
        d.N, d.C, d.H, d.W, d.c0, d.Cr = 2, 8, 4, 4, 2, 4
        d.dtype, d.training, d.relu = _cabi.CHAIN_F32, 1, 1
        for key, val in kw.items():
            setattr(d, key, val)
        return d

    bf = dict(dtype=_cabi.CHAIN_BF16)
    both = [
        (dict(N=0), "N, C, H, W >= 1"), (dict(C=0), "N, C, H, W >= 1"), (dict(H=-1), "N, C, H, W >= 1"),
        (dict(W=0), "N, C, H, W >= 1"),
        (dict(N=1, H=1, W=1), "more than one value"),                  # training with M < 2 (torch raises there too)
        (dict(dtype=3), "type"), (dict(dtype=-1), "type"),
        (dict(c0=-1), "window"), (dict(c0=5), "window"), (dict(Cr=9, c0=0), "window"), (dict(Cr=0), "window"),
        (dict(eps=-1.0), "eps"), (dict(eps=float("inf")), "eps"), (dict(eps=float("nan")), "eps"),
        (dict(momentum=-0.1), "momentum"), (dict(momentum=1.5), "momentum"), (dict(momentum=float("nan")), "momentum"),
        (dict(x=None), "x is NULL"), (dict(x=p + 2), "x is NULL or misaligned"), (dict(x=p + 1, **bf), "x is NULL or misaligned"),
        (dict(gamma=None), "gamma"), (dict(gamma=p + 2050), "gamma"), (dict(stats=p + 4098), "stats"),
    ]
    fwd_only = [(dict(beta=None), "beta"), (dict(beta=p + 2113), "beta"), (dict(y=None), "y is NULL"),
                (dict(y=p + 3074), "y is NULL or misaligned"), (dict(y=p + 3073, **bf), "y is NULL or misaligned"),
                (dict(res=p + 1026), "res is misaligned"), (dict(res=p + 1025, **bf), "res is misaligned"),
                (dict(y=p), "one buffer"), (dict(y=p + 1024), "one buffer"),
                (dict(res_stride=(128, 16, -4, 1)), "negative"),
                (dict(running_mean=p + 2178), "running statistics are misaligned"),
                (dict(running_var=None), "together"), (dict(running_mean=None), "together"),
                (dict(training=0, running_mean=None, running_var=None), "eval mode"),
                (dict(num_batches_tracked=p + 2308), "num_batches_tracked")]
    bwd_only = [(dict(dtype=_cabi.CHAIN_F16), "forward only"), (dict(stats=None), "stats is NULL"),
                (dict(g=None), "g is NULL"), (dict(g=p + 5122), "g is NULL or misaligned"),
                (dict(y=None), "ReLU mask"), (dict(y=p + 3073, **bf), "ReLU mask"),
                (dict(dx=p + 6146), "dx / dres"), (dict(dres=p + 7169, **bf), "dx / dres"), (dict(dres=p + 6144), "one buffer"),
                (dict(dgamma=p + 8194), "dgamma / dbeta"), (dict(dbeta=p + 8257), "dgamma / dbeta"),
                (dict(training=0, N=1, H=1, W=1), "more than one value")]
    for entry, cases in ((lib.tadmm_bnact_fwd, both + fwd_only), (lib.tadmm_bnact_bwd, both + bwd_only)):
        for kw, text in cases:
            assert entry(h, C.byref(desc(**kw)), None) == -1, kw
            assert text in lib.tadmm_last_error(h).decode(), (kw, lib.tadmm_last_error(h))
        assert entry(h, C.byref(desc(N=2 ** 15, H=2 ** 8, W=2 ** 8)), None) == -5
        assert str(MAX_M) in lib.tadmm_last_error(h).decode()
        assert entry(h, None, None) == -1 and "NULL" in lib.tadmm_last_error(h).decode()
        assert entry(None, C.byref(desc()), None) == -1
        for kw in (dict(workspace=None), dict(workspace_bytes=255), dict(workspace=p + 9220)):
            assert entry(h, C.byref(desc(**kw)), None) == -2, kw
            assert "workspace" in lib.tadmm_last_error(h).decode()
    # the window is read only where there is a residual; a backward that wants nothing launches nothing
    nothing = dict(dx=None, dres=None, dgamma=None, dbeta=None, workspace=None)
    assert lib.tadmm_bnact_bwd(h, C.byref(desc(c0=-3, **nothing)), None) == 0
    assert lib.tadmm_bnact_bwd(h, C.byref(desc(y=None, relu=0, **nothing)), None) == 0
    lib.tadmm_destroy(h)


def test_refusal_rule_and_routing_rule():
    ok = dict(is_cuda=True, dtype=torch.float32, shape=(2, 16, 8, 8), grad=True, training=True)
    fn = HF.batch_norm_act_launch_refusal
    assert fn(**ok) is None
    assert fn(**dict(ok, dtype=torch.bfloat16)) is None
    assert fn(**dict(ok, dtype=torch.float16, grad=False)) is None
    assert fn(**dict(ok, grad=False, training=False)) is None
    assert "HIP device" in fn(**dict(ok, is_cuda=False))
    assert "float64" in fn(**dict(ok, dtype=torch.float64))
    assert "float16 with gradients" in fn(**dict(ok, dtype=torch.float16))
    assert "eval mode with gradients" in fn(**dict(ok, training=False))
    assert "NCHW contiguous" in fn(**dict(ok, contiguous=False))
    assert "shape" in fn(**dict(ok, shape=(2 ** 15, 3, 2 ** 8, 2 ** 8)))
    assert "one value per channel" in fn(**dict(ok, shape=(1, 4, 1, 1)))
    assert fn(**dict(ok, shape=(1, 4, 1, 1), grad=False, training=False)) is None
    assert "affine=False" in fn(**dict(ok, affine=False))
    assert "track_running_stats=False" in fn(**dict(ok, tracked=False))
    assert "not float32" in fn(**dict(ok, param_dtypes=(torch.float32, torch.bfloat16)))
    assert "momentum=None" in fn(**dict(ok, momentum_given=False))
    assert "another" in fn(**dict(ok, foreign=True))
    # the measured classes: the launch only where it was ahead beyond the spread in both runs
    cifar = [(n, c, hw) for c, hw in ((16, 1024), (32, 256), (64, 64)) for n in (1, 128)]
    inet = [(n, c, hw) for c, hw in ((64, 3136), (256, 3136), (512, 784), (2048, 49)) for n in (1, 32)]
    big = {(32, 256, 3136), (32, 512, 784)}
    for n, c, hw in cifar + inet:
        for dt in (torch.float32, torch.bfloat16):
            assert ops.bnact_pays(n, c, hw, dt, False, True) is True
            assert ops.bnact_pays(n, c, hw, dt, False, False) is (n > 1 and hw > 49), (n, c, hw)
        assert ops.bnact_pays(n, c, hw, torch.float32, True, True) is ((n, c, hw) in big)
        assert ops.bnact_pays(n, c, hw, torch.float32, True, False) is ((n, c, hw) in big | {(32, 64, 3136)})
        for residual in (False, True):
            assert ops.bnact_pays(n, c, hw, torch.bfloat16, True, residual) is ((n, c, hw) == (32, 256, 3136))
            assert ops.bnact_pays(n, c, hw, torch.float16, True, residual) is ops.bnact_pays(n, c, hw, torch.bfloat16, True, residual)


def tail_case(dtype, shape, res_kind, seed=5):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    x = (0.5 + 2 * torch.randn(shape, generator=g, dtype=dtype)).requires_grad_()
    gamma = (1 + 0.5 * torch.randn(c, generator=g, dtype=dtype)).requires_grad_()
    beta = torch.randn(c, generator=g, dtype=dtype).requires_grad_()
    res, view, c0 = None, None, 0
    if res_kind == "full":
        res = torch.randn(shape, generator=g, dtype=dtype).requires_grad_()
        view = res
    elif res_kind == "optionA":                        # x_in[:, :, ::2, ::2] of half the channels, at offset c // 4
        res = torch.randn(n, c // 2, 2 * h, 2 * w - 1, generator=g, dtype=dtype).requires_grad_()
        view, c0 = res[:, :, ::2, ::2], c // 4
    up = torch.randn(shape, generator=g, dtype=dtype)
    rm, rv = torch.randn(c, generator=g, dtype=dtype), 0.5 + torch.rand(c, generator=g, dtype=dtype)
    return x, gamma, beta, res, view, c0, up, rm, rv


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 2e-5)], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(3, 8, 5, 7), (2, 4, 1, 1)], ids=["3x8x5x7", "2x4x1x1"])
@pytest.mark.parametrize("res_kind", ["none", "full", "optionA"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_composed_route_on_the_cpu_is_the_restatement(relu, res_kind, shape, dtype, tol):
    """float64: 1e-12 of the largest magnitude (one formula twice).  float32: 2e-5, some hundred units of 2^-23 for
    sums of at most 105 terms in another order."""
    x, gamma, beta, res, view, c0, up, rm, rv = tail_case(dtype, shape, res_kind)
    n, c, h, w = shape
    want = R.tail(x, gamma, beta, view, c0, relu)
    want_rm, want_rv = R.running(rm, rv, want["mean"], want["var"], n * h * w, 0.25)
    for fn in (HF.batch_norm_act_composed, HF.batch_norm_act):
        rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(3)
        y = fn(x, rm_, rv_, gamma, beta, view, res_channel_offset=c0, training=True, momentum=0.25, relu=relu,
               num_batches_tracked=nbt)
        assert y.shape == shape and int(nbt) == 4
        leaves = [x, gamma, beta] + ([] if res is None else [res])
        grads = torch.autograd.grad(y, leaves, up)
        ref = R.tail_grads(x, gamma, beta, view, c0, up, (y > 0) if relu else None)
        pairs = [("y", y, want["y"]), ("running_mean", rm_, want_rm), ("running_var", rv_, want_rv),
                 ("dx", grads[0], ref["dx"]), ("dgamma", grads[1], ref["dgamma"]), ("dbeta", grads[2], ref["dbeta"])]
        if res is not None:                            # the gradient of the view, carried back to its base by autograd
            base = torch.zeros(res.shape, dtype=torch.float64)
            (base[:, :, ::2, ::2] if res_kind == "optionA" else base).copy_(ref["dres"])
            pairs.append(("dres", grads[3], base))
        for key, got, ref_t in pairs:
            err = float((got.detach().double() - ref_t).abs().max())
            assert err <= tol * max(float(ref_t.abs().max()), 1.0), (key, err)
        if res_kind == "optionA":                      # the pad is exact: F.pad of the reference's LambdaLayer
            pad = F.pad(view, (0, 0, 0, 0, c // 4, c // 4), "constant", 0)
            y2 = F.batch_norm(x, None, None, gamma, beta, True, 0.0, 1e-5) + pad
            assert torch.equal(y.detach(), (F.relu(y2) if relu else y2).detach())
    # eval mode: the running statistics are read, nothing is updated
    rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(3)
    y = HF.batch_norm_act(x, rm_, rv_, gamma, beta, view, res_channel_offset=c0, training=False, relu=relu,
                          num_batches_tracked=nbt)
    ref_y, _ = R.tail_eval(x, rm, rv, gamma, beta, view, c0, relu)
    assert float((y.detach().double() - ref_y).abs().max()) <= tol * max(float(ref_y.abs().max()), 1.0)
    assert torch.equal(rm_, rm) and torch.equal(rv_, rv) and int(nbt) == 3


def test_composed_route_options_and_argument_errors(monkeypatch):
    x, gamma, beta, res, view, c0, up, rm, rv = tail_case(torch.float32, (2, 8, 4, 4), "optionA")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        HF.batch_norm_act(torch.randn(1, 8, 1, 1), rm.clone(), rv.clone(), gamma, beta, training=True)
    assert HF.batch_norm_act(torch.randn(1, 8, 1, 1), rm.clone(), rv.clone(), gamma, beta, training=False).shape == (1, 8, 1, 1)
    # momentum=None is nn.BatchNorm2d's cumulative average; affine=False and no tracked statistics are F.batch_norm's
    bn = torch.nn.BatchNorm2d(8, momentum=None)
    twin = torch.nn.BatchNorm2d(8, momentum=None)
    for _ in range(3):
        xi = torch.randn(2, 8, 4, 4)
        assert torch.equal(HF.batch_norm_act_module(bn, xi, relu=False), twin(xi))
    assert int(bn.num_batches_tracked) == 3 and torch.equal(bn.running_var, twin.running_var)
    for mod in (torch.nn.BatchNorm2d(8, affine=False), torch.nn.BatchNorm2d(8, track_running_stats=False).eval(),
                torch.nn.GroupNorm(2, 8)):
        xi = torch.randn(2, 8, 4, 4)
        assert torch.equal(HF.batch_norm_act_module(mod, xi, xi), F.relu(mod(xi) + xi))
    # everything the launch refuses reaches the composed route under route=None and raises under route="launch"
    calls = []
    composed = HF.batch_norm_act_composed
    monkeypatch.setattr(HF, "batch_norm_act_composed", lambda *a, **k: calls.append(1) or composed(*a, **k))
    monkeypatch.setattr(ops, "bnact_pays", lambda *a, **k: True)
    xcl = x.detach().contiguous(memory_format=torch.channels_last)
    cases = [dict(x=xcl, training=True), dict(x=x.detach()[:, :, :, ::2], training=True), dict(momentum=None, training=True),
             dict(training=False), dict(x=x.detach().half(), training=True), dict(weight=None, bias=None, training=True),
             dict(running_mean=None, running_var=None, training=True), dict(weight=gamma.double(), training=True)]
    for case in cases:
        kw = dict(x=x, running_mean=rm.clone(), running_var=rv.clone(), weight=gamma, bias=beta)
        kw.update(case)
        args = [kw.pop(k) for k in ("x", "running_mean", "running_var", "weight", "bias")]
        before = len(calls)
        try:
            HF.batch_norm_act(*args, **kw)
        except RuntimeError:
            pass                                      # torch refuses mixed float64 / float16 operands on its own
        assert len(calls) == before + 1, case
        with pytest.raises(_cabi.TadmmError, match="route='launch' cannot take"):
            HF.batch_norm_act(*args, route="launch", **kw)
    with pytest.raises(ValueError):
        HF.batch_norm_act(x, rm, rv, gamma, beta, training=True, route="fastest")
    for bad in (dict(weight=gamma[:-1]), dict(residual=view[:1]), dict(residual=view, res_channel_offset=5),
                dict(res_channel_offset=2), dict(momentum=1.5), dict(x=x[0]), dict(running_mean=rm[:3])):
        kw = dict(x=x, running_mean=rm, running_var=rv, weight=gamma, bias=beta, training=True)
        kw.update(bad)
        args = [kw.pop(k) for k in ("x", "running_mean", "running_var", "weight", "bias")]
        with pytest.raises(ValueError):
            HF.batch_norm_act(*args, **kw)


def randomise(mod, seed):
    """BatchNorm weights around 1, biases and running means off zero, running variances off one."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(1 + 0.3 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))
    return mod


def check_module(mod, ref_fn, x, tol, training):
    """Output and every parameter gradient of `mod` against the float64 restatement `ref_fn(x64, sd)`, max norm."""
    mod.train(training)
    sd = R.state64(mod, requires_grad=True)
    up = torch.randn(mod(x).shape, generator=torch.Generator().manual_seed(1), dtype=x.dtype)
    names = [n for n, _ in mod.named_parameters()]
    want = ref_fn(R.f64(x), sd)
    want_g = torch.autograd.grad(want, [sd[n] for n in names], R.f64(up))
    got = mod(x)
    got_g = torch.autograd.grad(got, list(mod.parameters()), up)
    for key, a, b in [("out", got, want)] + list(zip(names, got_g, want_g)):
        assert float((a.detach().double() - b.detach()).abs().max()) <= tol * max(float(b.detach().abs().max()), 1e-3), key


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 2e-4)], ids=["f64", "f32"])
def test_dense_blocks_on_the_cpu_are_the_restatement(dtype, tol):
    torch.manual_seed(0)
    for option in ("A", "B"):
        blk = randomise(RC.TTBasicBlock(8, 16, 2, option=option, conv=RC.TTConv2dM, stage=2, id=0, hp_dict=NoRanks), 1).to(dtype)
        assert isinstance(blk.conv1, torch.nn.Conv2d) and (blk.pad == 4) == (option == "A")
        x = torch.randn(3, 8, 6, 6, dtype=dtype)
        for training in (True, False):
            check_module(blk, lambda x64, sd: R.cifar_block(x64, sd, "", blk, training), x, tol, training)
        if option == "A":                              # the tail's window is the reference's LambdaLayer
            blk.eval()
            want = F.relu(blk.bn2(blk.conv2(F.relu(blk.bn1(blk.conv1(x))))) + blk.shortcut(x))
            assert torch.allclose(blk(x), want, rtol=0, atol=1e-5)
    same = RC.TTBasicBlock(8, 8, 1, stage=1, id=0, hp_dict=NoRanks)
    assert len(same.shortcut) == 0 and same.pad is None
    ds = torch.nn.Sequential(RI.conv1x1(8, 16, 2), torch.nn.BatchNorm2d(16))
    bott = randomise(RI.TTBottleneck(8, 4, 2, ds, stage=1, id=0, hp_dict=NoRanks), 2).to(dtype)
    x = torch.randn(3, 8, 6, 6, dtype=dtype)
    for training in (True, False):
        check_module(bott, lambda x64, sd: R.inet_block(x64, sd, "", bott, training), x, tol, training)
    basic = randomise(RI.TTBasicBlock(8, 8, stage=1, id=1, hp_dict=NoRanks), 3).to(dtype)
    check_module(basic, lambda x64, sd: R.inet_block(x64, sd, "", basic, True), x, tol, True)
    assert bott.set_route("composed") is bott and bott.route == "composed"


def test_small_models_on_the_cpu_are_the_restatement():
    """Output and every parameter gradient in float64, where one formula is computed twice (1e-9 of the largest
    magnitude), in eval and in training mode; in float32 the eval logits (1e-4: a ReLU or max-pool decision that falls
    the other way in float32 moves a gradient of a net this small by more than rounding, so those stay with float64)."""
    torch.manual_seed(3)
    cifar = randomise(RC._tt_resnet([1, 1, 1], hp_dict=NoRanks, num_classes=7), 4)
    inet = randomise(RI._tt_resnet(RI.TTBasicBlock, [1, 1, 1, 1], RI.TTConv2dM, NoRanks, num_classes=5,
                                   zero_init_residual=True), 5)
    for model, ref, img in ((cifar, R.cifar_resnet, torch.randn(3, 3, 16, 16)), (inet, R.inet_resnet, torch.randn(4, 3, 64, 64))):
        want = ref(R.f64(img), R.state64(model), model, False)
        got = model.eval()(img)
        assert float((got.detach().double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
        model.double()
        for training in (False, True):
            check_module(model, lambda x64, sd: ref(x64, sd, model, training), img.double(), 1e-9, training)
        model.float()
    assert int(cifar.bn1.num_batches_tracked) == 2 and int(cifar.layer2[0].bn2.num_batches_tracked) == 2
    assert cifar.eval()(torch.randn(3, 3, 16, 16)).shape == (3, 7)
    z = RI._tt_resnet(RI.TTBottleneck, [1, 1, 1, 1], RI.TTConv2dR, NoRanks, num_classes=5, zero_init_residual=True)
    assert float(z.layer1[0].bn3.weight.detach().abs().max()) == 0.0 and float(z.layer1[0].bn2.weight.detach().min()) == 1.0
    assert float(RI._tt_resnet(RI.TTBasicBlock, [1, 1, 1, 1], RI.TTConv2dR, NoRanks, zero_init_residual=True)
                 .layer3[0].bn2.weight.detach().abs().max()) == 0.0
    with pytest.raises(ValueError, match="replace_stride_with_dilation"):
        RI.TTResNet(RI.TTBasicBlock, [1, 1, 1, 1], replace_stride_with_dilation=[True], hp_dict=NoRanks)
    with pytest.raises(ValueError, match="groups=1"):
        RI.TTBasicBlock(8, 8, groups=2, hp_dict=NoRanks)
    out2, base, compr = cifar.eval().forward_flops(torch.randn(1, 3, 16, 16))
    assert out2.shape == (1, 7) and base == compr and base > 0
    out3, base, compr = inet.eval().forward_flops(torch.randn(1, 3, 32, 32))
    assert out3.shape == (1, 5) and base == compr and base > 0


def test_state_dict_keys_of_the_shipped_tables():
    """The key sets of ttm_resnet32 (table tt_resnet32 3x) and ttr_resnet50 (general 3x) against the lists under
    tests/golden/.  timm is not installed where the reference could have been constructed, so the lists were derived by
    reading it: nn.Module registration of resnet_cifar_tt.py / resnet_inet_tt.py (conv1, bn1, layerS.I.{convK, bnK,
    downsample.0, downsample.1}, linear / fc; an option-A shortcut and an empty nn.Sequential own no keys), the
    BatchNorm2d entries weight, bias, running_mean, running_var, num_batches_tracked, and for a convolution named in the
    table the parameters TTConv.py registers -- TTConv2dM: in_tt_cores.i, core_kernel, out_tt_cores.i; TTConv2dR:
    out_tt_cores.i, conv_core, in_tt_cores.i -- with the number of cores read from the table's tt_shapes."""
    for name, ratio, mod in (("ttm_resnet32", "3", RC), ("ttr_resnet50", "3", RI)):
        with open(os.path.join(GOLDEN, f"{name}_state_dict_keys.json")) as f:
            want = json.load(f)
        model = getattr(mod, name)(get_hp_dict(name, ratio))
        got = list(model.state_dict())
        assert len(want) == len(set(want)) and set(got) == set(want), sorted(set(got) ^ set(want))[:8]
        other = getattr(mod, name)(get_hp_dict(name, ratio))
        other.load_state_dict(model.state_dict())
    assert any(k.endswith("num_batches_tracked") for k in want) and "layer1.0.conv2.conv_core" in want


def test_factories_argument_errors(tmp_path):
    assert len(RC.FACTORIES) == 13 and len(RI.FACTORIES) == 11 and not set(RC.FACTORIES) & set(RI.FACTORIES)
    for mod in (RC, RI):
        for name in mod.FACTORIES:
            assert getattr(mod, name).__name__ == name
    assert "stftkc_resnet32" in RC.FACTORIES and "ttm_resnet56" not in RC.FACTORIES and "tkr_resnet34" in RI.FACTORIES
    fn = RC.tkc_resnet20
    with pytest.raises(ValueError, match="nothing is downloaded"):
        fn(NoRanks, decompose=True)
    with pytest.raises(ValueError, match="URL"):
        fn(NoRanks, decompose=True, path="https://example.org/resnet20.pth")
    with pytest.raises(ValueError, match="nothing is downloaded"):
        fn(NoRanks, pretrained=True)
    with pytest.raises(ValueError, match="nothing is downloaded"):
        RI.ttr_resnet18(NoRanks, decompose=True, pretrained=True)      # the reference downloads timm's resnet18 here
    dense = fn(NoRanks, num_classes=4)
    assert dense.linear.out_features == 4 and len(dense.layer1) == 3 and isinstance(dense.layer3[2].conv2, torch.nn.Conv2d)
    sd = {k: v + 1 for k, v in dense.state_dict().items()}
    again = fn(NoRanks, decompose=True, dense_dict=sd, num_classes=4)
    assert all(torch.equal(v, sd[k]) for k, v in again.state_dict().items())
    path = os.path.join(tmp_path, "dense.pth")
    torch.save(sd, path)
    for kw in (dict(decompose=True), dict(pretrained=True)):
        loaded = fn(NoRanks, path=path, num_classes=4, **kw)
        assert all(torch.equal(v, sd[k]) for k, v in loaded.state_dict().items())
    r18 = RI.tkr_resnet18(NoRanks, num_classes=3)
    assert r18.fc.out_features == 3 and [len(l) for l in (r18.layer1, r18.layer2, r18.layer3, r18.layer4)] == [2, 2, 2, 2]
    assert isinstance(RI.ttr_resnet50(NoRanks, num_classes=3).layer1[0], RI.TTBottleneck)


def test_import_lines():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import resnet_cifar_tt as DC; import resnet_inet_tt as DI; "
            "import tadmm; from tadmm import resnet_cifar_layers as C, resnet_inet_layers as I; "
            "assert tadmm.resnet_cifar_layers is C and tadmm.resnet_inet_layers is I; "
            "assert all(getattr(DC, n) is getattr(C, n) and getattr(tadmm, n) is getattr(C, n) for n in C.FACTORIES); "
            "assert all(getattr(DI, n) is getattr(I, n) and getattr(tadmm, n) is getattr(I, n) for n in I.FACTORIES); "
            "assert all(getattr(DC, n) is getattr(C, n) for n in ('LambdaLayer', 'TTBasicBlock', 'TTResNet', '_tt_resnet')); "
            "assert all(getattr(DI, n) is getattr(I, n) for n in ('tt_conv3x3', 'tt_conv1x1', 'TTBasicBlock', 'TTBottleneck', "
            "'TTResNet', '_tt_resnet')); assert C.TTBasicBlock is not I.TTBasicBlock")
    subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "dnn-compression-tensor-admm_amd", "dropin")], check=True)
