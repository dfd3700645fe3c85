"""Host side of the MobileNetV2 depthwise stage and the MobileNetV2s (no GPU): every refusal of the C entries of
csrc/dwbn.hip, the plan, workspace and fits queries, the refusal function and the routing, the composed route of
`depthwise_bn_relu6`, the blocks and the two shipped svd models of tadmm/mobilenet_cifar_layers.py /
mobilenet_inet_layers.py against the float64 restatement of tests/_mobilenet_ref.py, their state-dict keys and shapes,
the factories and the import lines."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import _mobilenet_ref as R
from test_bnact_host_cpu import check_module, randomise
from tadmm import _cabi, get_hp_dict, ops
from tadmm import functional as HF
from tadmm import mobilenet_cifar_layers as MC
from tadmm import mobilenet_inet_layers as MI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_W = 4096 // 3 - 2
CIFAR = [(n, c, h, s) for c, h, s in ((32, 32, 1), (96, 32, 1), (144, 32, 1), (192, 32, 2), (384, 16, 1), (576, 16, 2),
                                      (960, 8, 1)) for n in (1, 128)]
INET = [(n, c, h, s) for c, h, s in ((32, 112, 1), (96, 112, 2), (144, 56, 2), (192, 28, 1), (384, 14, 1), (576, 14, 2),
                                     (960, 7, 1)) for n in (1, 32)]


class NoRanks:
    ranks = {}


def test_descriptor_size_fits_plan_and_workspace():
    lib = _cabi.load()
    assert lib.tadmm_dwbn_desc_bytes() == C.sizeof(_cabi.DwBnDesc)
    assert ops.dwbn_max_w() == MAX_W == 1363
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        for s in (1, 2):
            assert ops.dwbn_fits(1, 1, 1, 1, s, dt) is True and ops.dwbn_fits(128, 192, 32, 32, s, dt) is True
            assert ops.dwbn_fits(1, 1, 3, MAX_W, s, dt) is True and ops.dwbn_fits(1, 1, 3, MAX_W + 1, s, dt) is False
            assert ops.dwbn_fits(2 ** 15, 3, 2 ** 8, 2 ** 8 - 1, s, dt) is True      # 2^31 - 2^23 values
            assert ops.dwbn_fits(2 ** 15, 3, 2 ** 8, 2 ** 8, s, dt) is False         # 2^31 values per channel
    for bad in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, -1, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), (1, 1, 1, 1, 3)):
        for fn in (ops.dwbn_fits, ops.dwbn_workspace_bytes, ops.dwbn_plan):
            with pytest.raises(_cabi.TadmmError):
                fn(*bad)
    m = C.c_int32(7)
    assert lib.tadmm_dwbn_fits(None, C.byref(m)) == -1 and m.value == MAX_W
    assert lib.tadmm_dwbn_fits(None, None) == -1
    # the plan at named shapes: whole planes G to a tile, or NB bands of RB output rows; U units in S splits of `per`
    plan = ops.dwbn_plan
    assert plan(2, 1, 1, 1) == dict(G=1, RB=1, NB=1, U=2, S=2, per=1)
    assert plan(2, 960, 2, 2) == dict(G=1, RB=2, NB=1, U=2, S=2, per=1)
    assert plan(128, 192, 32, 32, 2) == dict(G=3, RB=16, NB=1, U=43, S=6, per=8)      # three whole planes to a tile
    assert plan(32, 96, 112, 112, 2) == dict(G=1, RB=17, NB=4, U=128, S=11, per=12)   # 17 rows: 35 x 114 floats staged
    assert plan(1, 2, 112, 112, 1) == dict(G=1, RB=4, NB=28, U=28, S=28, per=1)       # few channels: short bands
    assert plan(2, 1024, 3, 1022, 1) == dict(G=1, RB=2, NB=2, U=4, S=1, per=4)        # one workgroup, two bands, two images
    assert plan(1, 1, 3, MAX_W, 1) == dict(G=1, RB=1, NB=3, U=3, S=3, per=1)
    for n, c, h, w, s in ((1, 1, 1, 1, 1), (7, 3, 33, 70, 2), (128, 960, 8, 8, 1), (32, 32, 112, 112, 1), (5, 2000, 9, 1363, 2),
                          (300, 1, 64, 64, 2), (3, 40, 200, 31, 1)):
        p = plan(n, c, h, w, s)
        ho, wo = ops.dwbn_out_hw(h, w, s)
        rows_in = (p["RB"] - 1) * s + 3
        assert p["G"] * rows_in * (w + 2) <= 4096 and p["G"] * (p["RB"] + 2) * (wo + 2) <= 4096, p      # both tiles fit
        assert p["NB"] == -(-ho // p["RB"]) and (p["G"] == 1 or p["NB"] == 1) and p["U"] == -(-n // p["G"]) * p["NB"]
        assert p["S"] == -(-p["U"] // p["per"]) and (p["S"] - 1) * p["per"] < p["U"] and p["S"] <= 128   # none empty
        assert plan(n, c, h, w, s, torch.bfloat16) == p                                  # the element type does not enter
    # eleven doubles per channel and split, min(128, ceil(1024 / C)) splits: a function of C alone
    ws = ops.dwbn_workspace_bytes
    assert ws(1, 1, 1, 1) == 128 * 88 and ws(128, 192, 32, 32, 2) == 192 * 6 * 88 and ws(2, 960, 2, 2) == 960 * 2 * 88
    assert ws(2, 2048, 7, 7) == 2048 * 88 and ws(5, 3, 1, 1) == 3 * 128 * 88 and ws(2, 16, 8, 8, 1, torch.bfloat16) == 16 * 64 * 88
    for c, h, w in ((1, 7, 7), (16, 32, 32), (64, 56, 56), (300, 5, 3)):
        sizes = [ws(n, c, h, w, s) for s in (1, 2) for n in (1, 2, 3, 5, 8, 21, 64, 65, 128, 1000)]
        assert len(set(sizes)) == 1 and sizes[0] % 256 == 0                            # never smaller for a larger N
        for n, p in ((n, plan(n, c, h, w)) for n in (1, 5, 64, 1000)):
            assert c * p["S"] * 88 <= sizes[0]                                           # the splits used fit it
    sizes = [ws(4, 8, h, 33) for h in range(1, 400, 13)] + [ws(4, 8, 9, w) for w in range(1, MAX_W, 97)]
    assert len(set(sizes)) == 1                                                         # nor for a larger plane
    dsc = _cabi.DwBnDesc()
    dsc.N, dsc.C, dsc.H, dsc.W, dsc.stride, dsc.dtype = 2, 2, 2, 2, 1, 7
    assert lib.tadmm_dwbn_workspace_bytes(C.byref(dsc), C.byref(C.c_size_t())) == -1
    dsc.dtype = _cabi.CHAIN_F32
    assert lib.tadmm_dwbn_workspace_bytes(C.byref(dsc), None) == -1
    assert lib.tadmm_dwbn_workspace_bytes(None, C.byref(C.c_size_t())) == -1
    assert lib.tadmm_dwbn_plan(C.byref(dsc), None) == -1 and lib.tadmm_dwbn_plan(None, (C.c_int32 * 6)()) == -1
    dsc.W = MAX_W + 1
    assert lib.tadmm_dwbn_workspace_bytes(C.byref(dsc), C.byref(C.c_size_t())) == -5
    assert lib.tadmm_dwbn_plan(C.byref(dsc), (C.c_int32 * 6)()) == -5


def test_launch_entries_refuse_before_launching():
    """No device is needed: every refusal comes before the first HIP call that would want one."""
    lib = _cabi.load()
    h = C.c_void_p()
    lib.tadmm_create(0, C.byref(h))
    assert h, "a handle needs no device"
    raw = (C.c_char * 65536)()
    p = C.addressof(raw) + (-C.addressof(raw)) % 16

    def desc(**kw):
        d = _cabi.DwBnDesc()
        d.x, d.w = p, p + 1024
        d.gamma, d.beta, d.running_mean, d.running_var, d.num_batches_tracked = p + 2048, p + 2112, p + 2176, p + 2240, p + 2304
        d.z, d.y, d.stats, d.g = p + 3072, p + 4096, p + 5120, p + 6144
        d.dx, d.dw, d.dgamma, d.dbeta = p + 7168, p + 8192, p + 8704, p + 8768
        d.workspace, d.workspace_bytes = p + 16384, 8 * 128 * 88
        d.eps, d.momentum = 1e-5, 0.1
        d.N, d.C, d.H, d.W, d.stride = 2, 8, 4, 4, 1
        d.dtype, d.training = _cabi.CHAIN_F32, 1
        for key, val in kw.items():
            setattr(d, key, val)
        return d

    bf = dict(dtype=_cabi.CHAIN_BF16)
    both = [
        (dict(N=0), "N, C, H, W >= 1"), (dict(C=0), "N, C, H, W >= 1"), (dict(H=-1), "N, C, H, W >= 1"),
        (dict(W=0), "N, C, H, W >= 1"),
        (dict(stride=0), "stride"), (dict(stride=3), "stride"), (dict(stride=-1), "stride"),
        (dict(N=1, H=1, W=1), "more than one output value"), (dict(N=1, H=2, W=2, stride=2), "more than one output value"),
        (dict(dtype=3), "type"), (dict(dtype=-1), "type"),
        (dict(eps=-1.0), "eps"), (dict(eps=float("inf")), "eps"), (dict(eps=float("nan")), "eps"),
        (dict(momentum=-0.1), "momentum"), (dict(momentum=1.5), "momentum"), (dict(momentum=float("nan")), "momentum"),
        (dict(x=None), "x is NULL"), (dict(x=p + 2), "x is NULL or misaligned"), (dict(x=p + 1, **bf), "x is NULL or misaligned"),
        (dict(w=None), "w is NULL"), (dict(w=p + 1026), "w is NULL or misaligned"),
        (dict(gamma=None), "gamma"), (dict(gamma=p + 2050), "gamma"), (dict(stats=p + 5122), "stats"),
        (dict(z=None), "z is NULL"), (dict(z=p + 3074), "z is NULL or misaligned"), (dict(z=p + 3073, **bf), "z is NULL or misaligned"),
        (dict(y=None), "y is NULL"), (dict(y=p + 4098), "y is NULL or misaligned"), (dict(y=p + 4097, **bf), "y is NULL or misaligned"),
    ]
    fwd_only = [(dict(beta=None), "beta"), (dict(beta=p + 2113), "beta"),
                (dict(y=p), "three buffers"), (dict(z=p), "three buffers"), (dict(z=p + 4096), "three buffers"),
                (dict(training=0, y=p), "three buffers"),
                (dict(running_mean=p + 2178), "running statistics are misaligned"),
                (dict(running_var=None), "together"), (dict(running_mean=None), "together"),
                (dict(training=0, running_mean=None, running_var=None), "eval mode"),
                (dict(num_batches_tracked=p + 2308), "num_batches_tracked")]
    bwd_only = [(dict(dtype=_cabi.CHAIN_F16), "forward only"), (dict(stats=None), "stats is NULL"),
                (dict(g=None), "g is NULL"), (dict(g=p + 6146), "g is NULL or misaligned"),
                (dict(dx=p + 7170), "dx is not aligned"), (dict(dx=p + 7169, **bf), "dx is not aligned"),
                (dict(dx=p), "one buffer"), (dict(dx=p + 6144), "one buffer"), (dict(dx=p + 4096), "one buffer"),
                (dict(dx=p + 3072), "one buffer"),
                (dict(dw=p + 8194), "dw / dgamma / dbeta"), (dict(dgamma=p + 8706), "dw / dgamma / dbeta"),
                (dict(dbeta=p + 8769), "dw / dgamma / dbeta"),
                (dict(training=0, N=1, H=1, W=1), "more than one output value")]
    for entry, cases in ((lib.tadmm_dwbn_fwd, both + fwd_only), (lib.tadmm_dwbn_bwd, both + bwd_only)):
        for kw, text in cases:
            assert entry(h, C.byref(desc(**kw)), None) == -1, kw
            assert text in lib.tadmm_last_error(h).decode(), (kw, lib.tadmm_last_error(h))
        assert entry(h, C.byref(desc(W=MAX_W + 1)), None) == -5 and str(MAX_W) in lib.tadmm_last_error(h).decode()
        assert entry(h, C.byref(desc(N=2 ** 15, H=2 ** 8, W=2 ** 8)), None) == -5
        assert entry(h, None, None) == -1 and "NULL" in lib.tadmm_last_error(h).decode()
        assert entry(None, C.byref(desc()), None) == -1
        for kw in (dict(workspace=None), dict(workspace_bytes=8 * 128 * 88 - 1), dict(workspace=p + 16388)):
            assert entry(h, C.byref(desc(**kw)), None) == -2, kw
            assert "workspace" in lib.tadmm_last_error(h).decode()
    # eval mode wants neither z nor a workspace to pass its checks; a backward that wants nothing launches nothing
    assert lib.tadmm_dwbn_bwd(h, C.byref(desc(dx=None, dw=None, dgamma=None, dbeta=None, workspace=None)), None) == 0
    lib.tadmm_destroy(h)


def test_refusal_rule_and_routing_rule():
    ok = dict(is_cuda=True, dtype=torch.float32, shape=(2, 16, 8, 8), stride=1, grad=True, training=True)
    fn = HF.depthwise_bn_relu6_launch_refusal
    assert fn(**ok) is None
    assert fn(**dict(ok, dtype=torch.bfloat16)) is None and fn(**dict(ok, stride=2)) is None and fn(**dict(ok, stride=(2, 2))) is None
    assert fn(**dict(ok, dtype=torch.float16, grad=False)) is None
    assert fn(**dict(ok, grad=False, training=False)) is None
    assert "HIP device" in fn(**dict(ok, is_cuda=False))
    assert "float64" in fn(**dict(ok, dtype=torch.float64))
    assert "float16 with gradients" in fn(**dict(ok, dtype=torch.float16))
    assert "eval mode with gradients" in fn(**dict(ok, training=False))
    assert "NCHW contiguous" in fn(**dict(ok, contiguous=False))
    assert "kernel (5, 5)" in fn(**dict(ok, kernel=(5, 5))) and "kernel (1, 1)" in fn(**dict(ok, kernel=1))
    assert "padding (0, 0)" in fn(**dict(ok, padding=0)) and "dilation (2, 2)" in fn(**dict(ok, dilation=2))
    assert "stride (3, 3)" in fn(**dict(ok, stride=3)) and "stride (1, 2)" in fn(**dict(ok, stride=(1, 2)))
    assert "shape" in fn(**dict(ok, shape=(2, 3, 4, MAX_W + 1))) and "shape" in fn(**dict(ok, shape=(2 ** 15, 3, 2 ** 8, 2 ** 8)))
    assert "one output value per channel" in fn(**dict(ok, shape=(1, 4, 1, 1)))
    assert "one output value per channel" in fn(**dict(ok, shape=(1, 4, 2, 2), stride=2))
    assert fn(**dict(ok, shape=(1, 4, 1, 1), grad=False, training=False)) is None
    assert "affine=False" in fn(**dict(ok, affine=False))
    assert "track_running_stats=False" in fn(**dict(ok, tracked=False))
    assert "not float32" in fn(**dict(ok, param_dtypes=(torch.float32, torch.bfloat16)))
    assert "momentum=None" in fn(**dict(ok, momentum_given=False))
    assert "another" in fn(**dict(ok, foreign=True))
    # the measured classes: the launch only where it was ahead beyond the spread in both runs
    for n, c, h, s in CIFAR + INET:
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            for grad in (False, True):
                assert ops.dwbn_pays(n, c, h, h, s, dt, grad) is PAYS(n, c, h, s, dt, grad), (n, c, h, s, dt, grad)
    assert ops.dwbn_pays(1, 32, 32, 32, 1, torch.float32, True) is False and ops.dwbn_pays(1, 192, 32, 32, 2, torch.float32, True) is False
    assert ops.dwbn_pays(1, 32, 112, 112, 1, torch.float32, True) is True and ops.dwbn_pays(1, 32, 32, 32, 1, torch.bfloat16, True) is True


def PAYS(n, c, h, s, dt, grad):
    """What both runs of scripts/bench_mobilenet_block.py gave: every forward, every 16-bit step, and the float32 step
    but for batch 1 below 2^18 values (two of those eight classes were not ahead in both runs; none above was behind)."""
    return not (grad and dt == torch.float32 and n == 1 and c * h * h < 2 ** 18)


def stage_case(dtype, shape, stride, seed=5):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    x = torch.randn(shape, generator=g, dtype=dtype).requires_grad_()
    filt = (torch.randn(c, 1, 3, 3, generator=g, dtype=dtype) / 3).requires_grad_()
    gamma = (2 + 0.3 * torch.randn(c, generator=g, dtype=dtype)).requires_grad_()
    beta = (3 + 0.2 * torch.randn(c, generator=g, dtype=dtype)).requires_grad_()
    up = torch.randn((n, c) + R.out_hw(h, w, stride), generator=g, dtype=dtype)
    rm, rv = torch.randn(c, generator=g, dtype=dtype), 0.5 + torch.rand(c, generator=g, dtype=dtype)
    return x, filt, gamma, beta, up, rm, rv


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 2e-5)], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(3, 8, 5, 7), (2, 4, 1, 2), (2, 3, 8, 6)], ids=["3x8x5x7", "2x4x1x2", "2x3x8x6"])
@pytest.mark.parametrize("stride", [1, 2], ids=["s1", "s2"])
def test_composed_route_on_the_cpu_is_the_restatement(stride, shape, dtype, tol):
    """float64: 1e-12 of the largest magnitude (one formula twice).  float32: 2e-5, some hundred units of 2^-23 for
    sums of at most 105 terms in another order."""
    x, filt, gamma, beta, up, rm, rv = stage_case(dtype, shape, stride)
    want = R.stage(x, filt, gamma, beta, stride)
    M = shape[0] * want["z"].shape[2] * want["z"].shape[3]
    want_rm, want_rv = R.running(rm, rv, want["mean"], want["var"], M, 0.25)
    for fn in (HF.depthwise_bn_relu6_composed, HF.depthwise_bn_relu6):
        rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(3)
        y = fn(x, filt, rm_, rv_, gamma, beta, stride=stride, training=True, momentum=0.25, num_batches_tracked=nbt)
        assert y.shape == up.shape and int(nbt) == 4
        grads = torch.autograd.grad(y, [x, filt, gamma, beta], up)
        ref = R.stage_grads(x, filt, gamma, beta, stride, up, (y > 0) & (y < 6))
        pairs = [("y", y, want["y"]), ("running_mean", rm_, want_rm), ("running_var", rv_, want_rv),
                 ("dx", grads[0], ref["dx"]), ("dw", grads[1], ref["dw"]), ("dgamma", grads[2], ref["dgamma"]),
                 ("dbeta", grads[3], ref["dbeta"])]
        for key, got, ref_t in pairs:
            err = float((got.detach().double() - ref_t).abs().max())
            assert err <= tol * max(float(ref_t.abs().max()), 1.0), (key, err)
    rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(3)
    y = HF.depthwise_bn_relu6(x, filt, rm_, rv_, gamma, beta, stride=stride, training=False, num_batches_tracked=nbt)
    ref_y, _ = R.stage_eval(x, filt, rm, rv, gamma, beta, stride)
    assert float((y.detach().double() - ref_y).abs().max()) <= tol * max(float(ref_y.abs().max()), 1.0)
    assert torch.equal(rm_, rm) and torch.equal(rv_, rv) and int(nbt) == 3


def test_composed_route_options_and_argument_errors(monkeypatch):
    x, filt, gamma, beta, up, rm, rv = stage_case(torch.float32, (2, 8, 6, 6), 1)
    with pytest.raises(_cabi.TadmmError, match="HIP device"):
        HF.depthwise_bn_relu6(x, filt, rm.clone(), rv.clone(), gamma, beta, stride=1, training=True, route="launch")
    # the module form: an nn.Conv2d with groups = channels and an nn.BatchNorm2d; anything else is called as it is
    conv = torch.nn.Conv2d(8, 8, 3, 2, 1, groups=8, bias=False)
    bn, twin = torch.nn.BatchNorm2d(8, momentum=None), torch.nn.BatchNorm2d(8, momentum=None)
    for _ in range(3):
        xi = torch.randn(2, 8, 6, 6)
        assert torch.equal(HF.depthwise_bn_relu6_module(conv, bn, xi), F.relu6(twin(conv(xi))))
    assert int(bn.num_batches_tracked) == 3 and torch.equal(bn.running_var, twin.running_var)
    for cv, mod in ((conv, torch.nn.BatchNorm2d(8, affine=False)), (conv, torch.nn.BatchNorm2d(8, track_running_stats=False).eval()),
                    (conv, torch.nn.GroupNorm(2, 8)), (torch.nn.Conv2d(8, 8, 3, 1, 1, groups=8), torch.nn.BatchNorm2d(8)),
                    (torch.nn.Conv2d(8, 16, 3, 1, 1, groups=8, bias=False), torch.nn.BatchNorm2d(16)),
                    (torch.nn.Conv2d(8, 8, 5, 1, 2, groups=8, bias=False), torch.nn.BatchNorm2d(8).eval())):
        xi = torch.randn(2, 8, 6, 6)
        twin_mod = torch.nn.BatchNorm2d(mod.num_features).train(mod.training) if type(mod) is torch.nn.BatchNorm2d and mod.affine \
            and mod.track_running_stats else mod
        assert torch.equal(HF.depthwise_bn_relu6_module(cv, mod, xi), F.relu6(twin_mod(cv(xi))))
    # everything the launch refuses reaches the composed route under route=None and raises under route="launch"
    calls = []
    composed = HF.depthwise_bn_relu6_composed
    monkeypatch.setattr(HF, "depthwise_bn_relu6_composed", lambda *a, **k: calls.append(1) or composed(*a, **k))
    monkeypatch.setattr(ops, "dwbn_pays", lambda *a, **k: True)
    xd = x.detach()
    xcl = xd.contiguous(memory_format=torch.channels_last)
    k5 = torch.randn(8, 1, 5, 5)
    cases = [dict(x=xcl, training=True), dict(x=xd[:, :, :, ::2], training=True), dict(momentum=None, training=True),
             dict(training=False), dict(x=xd.half(), training=True), dict(weight=None, bias=None, training=True),
             dict(running_mean=None, running_var=None, training=True), dict(weight=gamma.double(), training=True),
             dict(conv_weight=k5, padding=2, training=True), dict(padding=0, training=True), dict(dilation=2, padding=2, training=True),
             dict(stride=3, training=True), dict(conv_weight=filt.double(), training=True)]
    for case in cases:
        kw = dict(x=x, conv_weight=filt, running_mean=rm.clone(), running_var=rv.clone(), weight=gamma, bias=beta, stride=1)
        kw.update(case)
        args = [kw.pop(k) for k in ("x", "conv_weight", "running_mean", "running_var", "weight", "bias")]
        before = len(calls)
        try:
            HF.depthwise_bn_relu6(*args, **kw)
        except RuntimeError:
            pass                                      # torch refuses mixed float64 / float16 operands on its own
        assert len(calls) == before + 1, case
        with pytest.raises(_cabi.TadmmError, match="route='launch' cannot take"):
            HF.depthwise_bn_relu6(*args, route="launch", **kw)
    with pytest.raises(ValueError):
        HF.depthwise_bn_relu6(x, filt, rm, rv, gamma, beta, stride=1, training=True, route="fastest")
    for bad in (dict(weight=gamma[:-1]), dict(conv_weight=filt[:-1]), dict(conv_weight=torch.randn(8, 2, 3, 3)), dict(momentum=1.5),
                dict(x=x[0]), dict(running_mean=rm[:3])):
        kw = dict(x=x, conv_weight=filt, running_mean=rm, running_var=rv, weight=gamma, bias=beta, stride=1, training=True)
        kw.update(bad)
        args = [kw.pop(k) for k in ("x", "conv_weight", "running_mean", "running_var", "weight", "bias")]
        with pytest.raises(ValueError):
            HF.depthwise_bn_relu6(*args, **kw)


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 2e-4)], ids=["f64", "f32"])
def test_blocks_on_the_cpu_are_the_restatement(dtype, tol):
    torch.manual_seed(0)
    hp_c, hp_i = get_hp_dict("svdc_mobilenetv2_cifar", "2"), get_hp_dict("svdm_mobilenetv2", "2")
    MC.TTBaseBlock.alpha = 1
    blocks = [(MC.TTBaseBlock(32, 64, downsample=True, conv=MC.SVDConv2dC, id=6, hp_dict=hp_c), R.cifar_block, 32),
              (MC.TTBaseBlock(32, 32, conv=MC.SVDConv2dC, id=4, hp_dict=hp_c), R.cifar_block, 32),
              (MC.TTBaseBlock(8, 8, t=2, conv=MC.TKConv2dC, id=0, hp_dict=NoRanks), R.cifar_block, 8),
              (MI.TTInvertedResidual(8, 16, 1, 1, id=1, conv=MI.SVDConv2dM, hp_dict=hp_i), R.inet_block, 8),
              (MI.TTInvertedResidual(32, 32, 1, 6, id=5, conv=MI.SVDConv2dM, hp_dict=hp_i), R.inet_block, 32),
              (MI.TTInvertedResidual(24, 32, 2, 6, id=4, conv=MI.SVDConv2dM, hp_dict=hp_i), R.inet_block, 24)]
    assert blocks[0][0].shortcut is False and blocks[1][0].shortcut is True and blocks[4][0].identity and not blocks[5][0].identity
    assert isinstance(blocks[1][0].conv3, MC.SVDConv2dC) and isinstance(blocks[2][0].conv1, torch.nn.Conv2d)
    assert isinstance(blocks[4][0].conv[0], MI.SVDConv2dM) and isinstance(blocks[4][0].conv[3], torch.nn.Conv2d)
    for i, (blk, ref, c) in enumerate(blocks):
        blk = randomise(blk, i).to(dtype)
        x = torch.randn(3, c, 7, 7, dtype=dtype)
        for training in (True, False):
            check_module(blk, lambda x64, sd: ref(x64, sd, "", blk, training), x, tol, training)
        assert blk.set_route("composed") is blk and blk.route == "composed"
    # the forward is the reference's: relu6(bn1(conv1)), relu6(bn2(conv2)), bn3(conv3) + inputs
    blk = blocks[1][0].float().eval()
    x = torch.randn(2, 32, 5, 5)
    want = blk.bn3(blk.conv3(F.relu6(blk.bn2(blk.conv2(F.relu6(blk.bn1(blk.conv1(x)))))))) + x
    assert torch.allclose(blk(x), want, rtol=0, atol=1e-5)
    blk = blocks[5][0].float().eval()
    x = torch.randn(2, 24, 5, 5)
    assert torch.allclose(blk(x), blk.conv(x), rtol=0, atol=1e-5)


def test_shipped_svd_models_on_the_cpu_are_the_restatement():
    """Eval logits of `svdc_mobilenetv2_cifar` on (2, 3, 32, 32) and `svdm_mobilenetv2` on (2, 3, 64, 64) in float32
    (1e-4 of the largest logit), then output and every parameter gradient in float64, where one formula is computed
    twice (1e-9 of the largest magnitude), in eval and in training mode."""
    torch.manual_seed(3)
    cifar = randomise(MC.svdc_mobilenetv2_cifar(get_hp_dict("svdc_mobilenetv2_cifar", "2")), 4)
    inet = randomise(MI.svdm_mobilenetv2(get_hp_dict("svdm_mobilenetv2", "2"), num_classes=11), 5)
    for model, ref, img in ((cifar, R.cifar_mobilenet, torch.randn(2, 3, 32, 32)), (inet, R.inet_mobilenet, torch.randn(2, 3, 64, 64))):
        want = ref(R.f64(img), R.state64(model), model, False)
        got = model.eval()(img)
        assert float((got.detach().double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
        model.double()
        for training in (False, True):
            check_module(model, lambda x64, sd: ref(x64, sd, model, training), img.double(), 1e-9, training)
        model.float()
    assert int(cifar.bn0.num_batches_tracked) == 2 and int(cifar.bottlenecks[6].bn2.num_batches_tracked) == 2
    assert int(inet.features[8].conv[4].num_batches_tracked) == 2
    assert cifar.set_route("composed") is cifar and all(b.route == "composed" for b in cifar.bottlenecks)
    assert inet.set_route("launch") is inet and all(b.route == "launch" for b in list(inet.features)[1:])


def test_state_dict_keys_and_shapes_of_the_shipped_svd_tables():
    """Names and shapes of `svdc_mobilenetv2_cifar` and `svdm_mobilenetv2` with the shipped svd 2x tables against the
    lists under tests/golden/ (names and shapes only).  timm is not installed where the reference could have been
    constructed, so the lists were derived by reading it: nn.Module registration of mobilenetv2_cifar_tt.py (conv0, bn0,
    bottlenecks.i.{conv1, bn1, conv2, bn2, conv3, bn3}, conv1, bn1, fc) and mobilenetv2_tt.py (features.0.{0, 1},
    features.k.conv.{0, 1, 3, 4} for expansion 1 and {0, 1, 3, 4, 6, 7} otherwise, conv.{0, 1}, classifier; a ReLU6 owns
    no keys), the widths from the two block tables, the BatchNorm2d entries weight, bias, running_mean, running_var,
    num_batches_tracked, and for a 1x1 convolution named in the table the parameters SVDConv.py registers -- SVDConv2dC:
    left_kernel (r, I, 1, 1), right_kernel (O, r, 1, 1); SVDConv2dM: left_factor (r, I), right_factor (O, r) -- with r read
    from the table."""
    for name, mod in (("svdc_mobilenetv2_cifar", MC), ("svdm_mobilenetv2", MI)):
        with open(os.path.join(GOLDEN, f"{name}_state_dict_keys.json")) as f:
            want = [(k, tuple(s)) for k, s in json.load(f)]
        model = getattr(mod, name)(get_hp_dict(name, "2"))
        got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        assert len(want) == len(set(want)) and got == want, sorted(set(got) ^ set(want))[:8]
        other = getattr(mod, name)(get_hp_dict(name, "2"))
        other.load_state_dict(model.state_dict())
    assert ("features.17.conv.6.right_factor", (320, 172)) in want or any(k == "features.17.conv.6.right_factor" for k, _ in want)
    assert ("features.1.conv.0.weight", (32, 1, 3, 3)) in want and ("features.2.conv.3.weight", (96, 1, 3, 3)) in want


def test_factories_tables_and_argument_errors(tmp_path):
    assert MC.FACTORIES == tuple(f"{k}_mobilenetv2_cifar" for k in ("tkr", "tkc", "tkm", "svdr", "svdc", "svdm"))
    assert MI.FACTORIES == tuple(f"{k}_mobilenetv2" for k in ("ttr", "tkc", "svdc", "svdm"))
    built = {}
    for mod in (MC, MI):
        for name in mod.FACTORIES:
            assert getattr(mod, name).__name__ == name
            if name == "svdr_mobilenetv2_cifar":
                continue
            built[name] = getattr(mod, name)(get_hp_dict(name, "2"))
    # svdr_: SVDConv2dR initialises through left_factor (r, I) times right_factor (O, r), as SVDConv.py does, which only
    # a square layer survives; with the shipped table it constructs from a dense weight (decompose=True, on the device:
    # tests/test_gpu_mobilenet.py) and not from scratch, there and here
    with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
        MC.svdr_mobilenetv2_cifar(get_hp_dict("svdr_mobilenetv2_cifar", "2"))
    assert isinstance(MC.svdr_mobilenetv2_cifar(NoRanks).conv1, torch.nn.Conv2d)

    def factorised(model):
        return [n for n, m in model.named_modules() if not isinstance(m, torch.nn.Conv2d) and hasattr(m, "in_channels")]

    assert len(factorised(built["tkc_mobilenetv2_cifar"])) == 28 and len(factorised(built["svdm_mobilenetv2_cifar"])) == 28
    assert isinstance(built["tkr_mobilenetv2_cifar"].bottlenecks[3].conv1, MC.TKConv2dR)
    assert len(factorised(built["svdc_mobilenetv2"])) == 29 and isinstance(built["svdm_mobilenetv2"].conv[0], MI.SVDConv2dM)
    # the reference's own tables for ttr_ and tkc_mobilenetv2 key their ranks by other names than mobilenetv2_tt.py asks
    # for (features.2.conv.0.0.weight, blocks.1.0.conv_pw.weight against features.2.conv.0.weight): all dense, as there
    for name, foreign in (("ttr_mobilenetv2", "features.2.conv.0.0.weight"), ("tkc_mobilenetv2", "blocks.1.0.conv_pw.weight")):
        hp = get_hp_dict(name, "2")
        assert foreign in hp.ranks and "features.2.conv.0.weight" not in hp.ranks
        assert factorised(built[name]) == [] and not set(hp.ranks) & set(built[name].state_dict())
        assert sum(p.numel() for p in built[name].parameters()) == 3504872              # the dense mobilenetv2 at width 1
    # a table that lists a depthwise kernel is refused
    class Depthwise:
        ranks = {"bottlenecks.2.conv2.weight": 8, "features.1.conv.0.weight": 8, "features.3.conv.3.weight": 8}
    for make in (lambda: MC.svdc_mobilenetv2_cifar(Depthwise), lambda: MI.svdm_mobilenetv2(Depthwise),
                 lambda: MI.TTInvertedResidual(24, 24, 1, 6, id=3, conv=MI.SVDConv2dM, hp_dict=Depthwise)):
        with pytest.raises(ValueError, match="depthwise kernel"):
            make()
    # width_mult, alpha, num_classes
    assert MI._make_divisible(32 * 0.75, 8) == 24 and MI._make_divisible(10, 8) == 16 and MI._make_divisible(3.2, 4) == 4
    thin = MI.TTMobileNetV2(num_classes=5, width_mult=0.5, hp_dict=NoRanks)
    assert thin.features[0][0].out_channels == 16 and thin.classifier.in_features == 1280 and thin.classifier.out_features == 5
    assert MI.TTMobileNetV2(width_mult=1.4, hp_dict=NoRanks, cfgs=[[1, 16, 1, 1]]).classifier.in_features == 1792
    half = MC.TTMobileNetV2(output_size=3, alpha=0.5, hp_dict=NoRanks)
    assert half.conv0.out_channels == 16 and half.bottlenecks[16].conv3.out_channels == 160 and MC.TTBaseBlock.alpha == 0.5
    MC.TTBaseBlock.alpha = 1
    # decompose / pretrained / path / dense_dict
    fn = MC.tkc_mobilenetv2_cifar
    with pytest.raises(ValueError, match="nothing is downloaded"):
        fn(NoRanks, decompose=True)
    with pytest.raises(ValueError, match="URL"):
        fn(NoRanks, decompose=True, path="https://example.org/mobilenetv2.pth")
    with pytest.raises(ValueError, match="nothing is downloaded"):
        fn(NoRanks, pretrained=True)
    with pytest.raises(ValueError, match="mobilenetv2_100"):
        MI.svdm_mobilenetv2(NoRanks, decompose=True, pretrained=True)     # the reference downloads timm's model here
    dense = fn(NoRanks, num_classes=4)
    assert dense.fc.out_features == 4 and len(dense.bottlenecks) == 17
    sd = {k: v + 1 for k, v in dense.state_dict().items()}
    again = fn(NoRanks, decompose=True, dense_dict=sd, num_classes=4)
    assert all(torch.equal(v, sd[k]) for k, v in again.state_dict().items())
    path = os.path.join(tmp_path, "dense.pth")
    torch.save(sd, path)
    for kw in (dict(decompose=True), dict(pretrained=True)):
        loaded = fn(NoRanks, path=path, num_classes=4, **kw)
        assert all(torch.equal(v, sd[k]) for k, v in loaded.state_dict().items())
    inet = MI.ttr_mobilenetv2(NoRanks, num_classes=3)
    sd = {k: v + 1 for k, v in inet.state_dict().items()}
    torch.save(sd, path)
    loaded = MI.ttr_mobilenetv2(NoRanks, decompose=True, pretrained=True, path=path, num_classes=3)
    assert all(torch.equal(v, sd[k]) for k, v in loaded.state_dict().items())
    # initialisation: normal(0, sqrt(2 / (k k out))) for nn.Conv2d, ones and zeros for BatchNorm, 0.01 for the classifier
    w = inet.features[2].conv[3].weight
    assert abs(float(w.detach().std()) - (2 / (9 * 96)) ** 0.5) < 0.2 * (2 / (9 * 96)) ** 0.5 and float(inet.classifier.bias.detach().abs().max()) == 0.0
    assert float(inet.features[2].conv[4].weight.detach().min()) == 1.0 and abs(float(inet.classifier.weight.detach().std()) - 0.01) < 0.003


def test_import_lines():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import mobilenetv2_cifar_tt as DC; import mobilenetv2_tt as DI; "
            "import tadmm; from tadmm import mobilenet_cifar_layers as C, mobilenet_inet_layers as I; "
            "assert tadmm.mobilenet_cifar_layers is C and tadmm.mobilenet_inet_layers is I; "
            "assert all(getattr(DC, n) is getattr(C, n) and getattr(tadmm, n) is getattr(C, n) for n in C.FACTORIES); "
            "assert all(getattr(DI, n) is getattr(I, n) and getattr(tadmm, n) is getattr(I, n) for n in I.FACTORIES); "
            "assert all(getattr(DC, n) is getattr(C, n) for n in ('TTBaseBlock', 'TTMobileNetV2', '_tt_mobilenetv2_cifar')); "
            "assert all(getattr(DI, n) is getattr(I, n) for n in ('_make_divisible', 'TTInvertedResidual', 'TTMobileNetV2', "
            "'_tt_mobilenetv2', 'conv_3x3_bn', 'conv_1x1_bn', 'tt_conv_1x1_bn')); assert C.TTMobileNetV2 is not I.TTMobileNetV2")
    subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "dnn-compression-tensor-admm_amd", "dropin")], check=True)
