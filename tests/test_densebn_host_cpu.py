"""Host side of the DenseNet pre-activation and the DenseNets (no GPU): every refusal of the C entries of
csrc/densebn.hip, the workspace and fits queries, the refusal function and the routing, the composed route of
`dense_batch_norm_act` and small models of tadmm/densenet_cifar_layers.py / densenet_inet_layers.py against the float64
restatement of tests/_densenet_ref.py, `DenseFeatures` bookkeeping, the state-dict keys of two shipped tables, the
factories' argument errors and the import lines."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import _densenet_ref as D
from tadmm import _cabi, get_hp_dict, ops
from tadmm import densenet_cifar_layers as DC
from tadmm import densenet_inet_layers as DI
from tadmm import functional as HF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_M = 2 ** 31 - 4096
MAX_SEG = _cabi.DENSEBN_MAX_SEGMENTS


class NoRanks:
    ranks = {}
    tt_shapes = {}


def test_descriptor_size_fits_and_workspace():
    lib = _cabi.load()
    assert lib.tadmm_densebn_desc_bytes() == C.sizeof(_cabi.DenseBnDesc)
    assert ops.densebn_max_segments() == MAX_SEG and MAX_SEG >= 65
    assert ops.densebn_max_m() == MAX_M == ops.bnact_max_m()
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert ops.densebn_fits(1, (1,), 1, 1, dt) is True and ops.densebn_fits(128, (32, 16, 16), 32, 32, dt) is True
        assert ops.densebn_fits(2, (1,) * MAX_SEG, 4, 4, dt) is True
        assert ops.densebn_fits(2, (1,) * (MAX_SEG + 1), 4, 4, dt) is False            # the bound on nseg
        assert ops.densebn_fits(2 ** 15, (3, 2), 2 ** 8, 2 ** 8 - 1, dt) is True       # 2^31 - 2^23 values
        assert ops.densebn_fits(2 ** 15, (3, 2), 2 ** 8, 2 ** 8, dt) is False          # 2^31 values per channel
    for args in ((0, (1,), 1, 1), (1, (0,), 1, 1), (1, (2, -1), 1, 1), (1, (1,), -1, 1), (1, (1,), 1, 0), (1, (), 1, 1)):
        with pytest.raises(_cabi.TadmmError):
            ops.densebn_fits(*args)
        with pytest.raises(_cabi.TadmmError):
            ops.densebn_workspace_bytes(*args)
    m = C.c_int64(7)
    assert lib.tadmm_densebn_fits(None, C.byref(m)) == -1 and m.value == MAX_M
    assert lib.tadmm_densebn_fits(None, None) == -1
    # the size is bnact's for the channels of the call, however they are cut into segments
    for n, chans, h, w in ((1, (1,), 1, 1), (128, (16,), 32, 32), (128, (8, 4, 4), 32, 32), (2, (2048,), 7, 7),
                           (2, (1024, 512, 512), 7, 7), (32, (64,), 56, 56), (9, (1,), 256, 257), (5, (1, 1, 1), 1, 1)):
        for dt in (torch.float32, torch.bfloat16):
            assert ops.densebn_workspace_bytes(n, chans, h, w, dt) == ops.bnact_workspace_bytes(n, sum(chans), h, w, dt)
    assert ops.densebn_workspace_bytes(128, (16,), 32, 32) == 16 * 128 * 16
    for dt in (torch.float32, torch.bfloat16):
        for chans, h, w in (((1,), 7, 7), ((8, 8), 32, 32), ((32, 16, 16), 56, 56), ((100, 200), 5, 3)):
            sizes = [ops.densebn_workspace_bytes(n, chans, h, w, dt) for n in (1, 2, 3, 5, 8, 21, 64, 65, 128, 1000)]
            assert sizes == sorted(sizes) and all(s % 16 == 0 and s > 0 for s in sizes), (chans, h, w, sizes)
        sizes = [ops.densebn_workspace_bytes(4, (5, 3), h, 33, dt) for h in range(1, 400, 13)]
        assert sizes == sorted(sizes)
    dsc = _cabi.DenseBnDesc()
    dsc.N, dsc.H, dsc.W, dsc.nseg, dsc.dtype = 2, 2, 2, 1, 7
    dsc.seg[0].C = 2
    assert lib.tadmm_densebn_workspace_bytes(C.byref(dsc), C.byref(C.c_size_t())) == -1
    dsc.dtype = _cabi.CHAIN_F32
    assert lib.tadmm_densebn_workspace_bytes(C.byref(dsc), None) == -1
    assert lib.tadmm_densebn_workspace_bytes(None, C.byref(C.c_size_t())) == -1
    dsc.nseg = MAX_SEG + 1
    assert lib.tadmm_densebn_workspace_bytes(C.byref(dsc), C.byref(C.c_size_t())) == -1
    assert lib.tadmm_densebn_plan(C.byref(dsc), (C.c_int32 * 3)()) == -1
    dsc.nseg = 1
    assert lib.tadmm_densebn_plan(C.byref(dsc), None) == -1 and lib.tadmm_densebn_plan(None, (C.c_int32 * 3)()) == -1
    dsc.dtype = 7
    assert lib.tadmm_densebn_plan(C.byref(dsc), (C.c_int32 * 3)()) == -1
    dsc.dtype = _cabi.CHAIN_F32
    dsc.N, dsc.H, dsc.W = 2 ** 15, 2 ** 8, 2 ** 8
    assert lib.tadmm_densebn_workspace_bytes(C.byref(dsc), C.byref(C.c_size_t())) == -5
    assert lib.tadmm_densebn_plan(C.byref(dsc), (C.c_int32 * 3)()) == -5


def test_plan_query():
    """`tadmm_densebn_plan`: bnact's plan for the channels of the descriptor, however they are cut into segments -- one
    segment for its statistics launch, all of them for the consumer."""
    plan = ops.densebn_plan
    for args in ((0, (1,), 1, 1), (1, (0,), 1, 1), (1, (2, -1), 1, 1), (1, (1,), -1, 1), (1, (1,), 1, 0), (1, (), 1, 1),
                 (2, (1,) * (MAX_SEG + 1), 4, 4)):
        with pytest.raises(_cabi.TadmmError):
            plan(*args)
    assert plan(1, (1,), 1, 1) == dict(S=1, span=1024, cap=1)
    assert plan(4, (5, 3, 3), 24, 24) == dict(S=3, span=1024, cap=3)                # a split per trip
    assert plan(15, (1024, 512, 512), 12, 12) == dict(S=1, span=3072, cap=1)        # the consumer: three trips in one split
    assert plan(15, (1024,), 12, 12) == dict(S=2, span=2048, cap=2)                 # the statistics of its segments
    assert plan(15, (512,), 12, 12) == dict(S=3, span=1024, cap=3)
    assert plan(65, (1, 1), 32, 32) == dict(S=65, span=1024, cap=65)
    assert plan(130, (1, 1), 32, 32, torch.bfloat16) == dict(S=65, span=2048, cap=65)
    for n, chans, h, w in ((1, (1,), 1, 1), (128, (16,), 32, 32), (128, (8, 4, 4), 32, 32), (2, (2048,), 7, 7),
                           (2, (1024, 512, 512), 7, 7), (32, (64,), 56, 56), (9, (1,), 256, 257), (5, (1, 1, 1), 1, 1),
                           (8, (5, 3, 3), 7, 7), (2, (1,) * MAX_SEG, 4, 4)):
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            assert plan(n, chans, h, w, dt) == ops.bnact_plan(n, sum(chans), h, w, dt)


def test_launch_entries_refuse_before_launching():
    """No device is needed: every refusal comes before the first HIP call that would want one."""
    lib = _cabi.load()
    h = C.c_void_p()
    lib.tadmm_create(0, C.byref(h))
    assert h, "a handle needs no device"
    raw = (C.c_char * 65536)()
    p = C.addressof(raw) + (-C.addressof(raw)) % 16
    y_at = p + 16384                                   # (2, 8, 4, 4) float32 = 1024 bytes

    def desc(**kw):
        d = _cabi.DenseBnDesc()
        d.nseg = kw.pop("nseg", 2)
        chans = kw.pop("chans", (5, 3))
        for k in range(min(d.nseg, MAX_SEG)):
            s = d.seg[k]
            s.x, s.stats, s.dx, s.C = p + 1024 * k, p + 4096 + 256 * k, p + 8192 + 1024 * k, chans[k] if k < len(chans) else 1
        for key in [k for k in kw if k.startswith("seg")]:           # seg1_x=..., seg0_stats=...
            name, field = key.split("_", 1)
            setattr(d.seg[int(name[3:])], field, kw.pop(key))
        d.gamma, d.beta, d.running_mean, d.running_var, d.num_batches_tracked = p + 12288, p + 12352, p + 12416, p + 12480, p + 12544
        d.y, d.g, d.dgamma, d.dbeta = y_at, p + 20480, p + 24576, p + 24640
        d.workspace, d.workspace_bytes = p + 28672, 256
        d.eps, d.momentum = 1e-5, 0.1
        d.N, d.H, d.W = 2, 4, 4
        d.dtype, d.training, d.relu = _cabi.CHAIN_F32, 1, 1
        for key, val in kw.items():
            setattr(d, key, val)
        return d

    bf = dict(dtype=_cabi.CHAIN_BF16)
    shape = [
        (dict(N=0), "N, H, W >= 1"), (dict(H=-1), "N, H, W >= 1"), (dict(W=0), "N, H, W >= 1"),
        (dict(nseg=0), "segments"), (dict(nseg=-2), "segments"), (dict(nseg=MAX_SEG + 1), "segments"),
        (dict(chans=(5, 0)), "at least one channel"), (dict(chans=(-1, 3)), "at least one channel"),
        (dict(N=1, H=1, W=1), "more than one value"),                  # training with M < 2 (torch raises there too)
        (dict(dtype=3), "type"), (dict(dtype=-1), "type"),
    ]
    both = shape + [
        (dict(eps=-1.0), "eps"), (dict(eps=float("inf")), "eps"), (dict(eps=float("nan")), "eps"),
        (dict(momentum=-0.1), "momentum"), (dict(momentum=1.5), "momentum"), (dict(momentum=float("nan")), "momentum"),
        (dict(seg1_x=None), "x of segment 1"), (dict(seg0_x=p + 2), "x of segment 0"), (dict(seg1_x=p + 1025, **bf), "x of segment 1"),
        (dict(seg1_stats=None), "stats of segment 1"), (dict(seg0_stats=p + 4100), "stats of segment 0"),
        (dict(gamma=None), "gamma"), (dict(gamma=p + 12290), "gamma"),
    ]
    fwd_only = [(dict(beta=None), "beta"), (dict(beta=p + 12353), "beta"), (dict(y=None), "y is NULL"),
                (dict(y=y_at + 2), "y is NULL or misaligned"), (dict(y=y_at + 1, **bf), "y is NULL or misaligned"),
                (dict(y=p), "y overlaps segment 0"), (dict(y=p + 1024), "y overlaps segment 1"),
                (dict(y=p + 1024 + 64), "y overlaps segment 1"), (dict(seg1_x=y_at + 1020), "y overlaps segment 1"),
                (dict(running_mean=p + 12418), "running statistics are misaligned"),
                (dict(running_var=None), "together"), (dict(running_mean=None), "together"),
                (dict(training=0, running_mean=None, running_var=None), "eval mode"),
                (dict(num_batches_tracked=p + 12548), "num_batches_tracked")]
    bwd_only = [(dict(dtype=_cabi.CHAIN_F16), "forward only"),
                (dict(g=None), "g is NULL"), (dict(g=p + 20482), "g is NULL or misaligned"),
                (dict(y=None), "ReLU mask"), (dict(y=y_at + 1, **bf), "ReLU mask"),
                (dict(seg1_dx=p + 9218), "dx of segment 1"), (dict(seg0_dx=p + 8193, **bf), "dx of segment 0"),
                (dict(seg0_dx=p), "one buffer"), (dict(seg1_dx=p + 20480), "one buffer"), (dict(seg1_dx=y_at), "one buffer"),
                (dict(dgamma=p + 24578), "dgamma / dbeta"), (dict(dbeta=p + 24641), "dgamma / dbeta"),
                (dict(training=0, N=1, H=1, W=1), "more than one value")]
    one = dict(nseg=1, chans=(8,))
    stats_only = [(dict(nseg=2), "one segment per call"), (dict(seg0_x=None, **one), "x is NULL"),
                  (dict(seg0_x=p + 2, **one), "x is NULL or misaligned"), (dict(seg0_stats=None, **one), "stats is NULL"),
                  (dict(seg0_stats=p + 4100, **one), "stats is NULL or misaligned"),
                  (dict(training=0, N=1, H=1, W=1, **one), "more than one value")]
    for entry, cases in ((lib.tadmm_densebn_fwd, both + fwd_only), (lib.tadmm_densebn_bwd, both + bwd_only),
                         (lib.tadmm_densebn_stats, shape + stats_only)):
        for kw, text in cases:
            assert entry(h, C.byref(desc(**kw)), None) == -1, kw
            assert text in lib.tadmm_last_error(h).decode(), (kw, lib.tadmm_last_error(h))
        big = dict(N=2 ** 15, H=2 ** 8, W=2 ** 8)
        if entry is lib.tadmm_densebn_stats:
            big.update(one)
        assert entry(h, C.byref(desc(**big)), None) == -5
        assert str(MAX_M) in lib.tadmm_last_error(h).decode()
        assert entry(h, None, None) == -1 and "NULL" in lib.tadmm_last_error(h).decode()
        assert entry(None, C.byref(desc()), None) == -1
    for entry, base in ((lib.tadmm_densebn_bwd, {}), (lib.tadmm_densebn_stats, one)):
        for kw in (dict(workspace=None), dict(workspace_bytes=255), dict(workspace=p + 28676)):
            assert entry(h, C.byref(desc(**kw, **base)), None) == -2, kw
            assert "workspace" in lib.tadmm_last_error(h).decode()
    # eval mode reads no stats; a backward that wants nothing launches nothing and needs no workspace
    nothing = dict(seg0_dx=None, seg1_dx=None, dgamma=None, dbeta=None, workspace=None)
    assert lib.tadmm_densebn_bwd(h, C.byref(desc(**nothing)), None) == 0
    assert lib.tadmm_densebn_bwd(h, C.byref(desc(y=None, relu=0, **nothing)), None) == 0
    lib.tadmm_destroy(h)


def test_refusal_rule_and_routing_rule():
    f32 = torch.float32
    ok = dict(is_cuda=True, dtypes=(f32, f32), shapes=((2, 8, 8, 8), (2, 4, 8, 8)), grad=True, training=True)
    fn = HF.dense_batch_norm_act_launch_refusal
    assert fn(**ok) is None
    assert fn(**dict(ok, dtypes=(torch.bfloat16,) * 2)) is None
    assert fn(**dict(ok, dtypes=(torch.float16,) * 2, grad=False)) is None
    assert fn(**dict(ok, grad=False, training=False)) is None
    assert "HIP device" in fn(**dict(ok, is_cuda=False))
    assert "mixed types" in fn(**dict(ok, dtypes=(f32, torch.bfloat16)))
    assert "float64" in fn(**dict(ok, dtypes=(torch.float64,) * 2))
    assert "float16 with gradients" in fn(**dict(ok, dtypes=(torch.float16,) * 2))
    assert "eval mode with gradients" in fn(**dict(ok, training=False))
    assert "NCHW contiguous" in fn(**dict(ok, contiguous=False))
    assert "mixed shapes" in fn(**dict(ok, shapes=((2, 8, 8, 8), (2, 4, 8, 4))))
    assert "mixed shapes" in fn(**dict(ok, shapes=((2, 8, 8, 8), (3, 4, 8, 8))))
    many = MAX_SEG + 1
    assert f"{many} feature tensors" in fn(**dict(ok, dtypes=(f32,) * many, shapes=((2, 1, 4, 4),) * many))
    assert fn(**dict(ok, dtypes=(f32,) * MAX_SEG, shapes=((2, 1, 4, 4),) * MAX_SEG)) is None
    assert "shape" in fn(**dict(ok, shapes=((2 ** 15, 3, 2 ** 8, 2 ** 8),) * 2))
    assert "one value per channel" in fn(**dict(ok, shapes=((1, 4, 1, 1),) * 2))
    assert fn(**dict(ok, shapes=((1, 4, 1, 1),) * 2, grad=False, training=False)) is None
    assert "affine=False" in fn(**dict(ok, affine=False))
    assert "track_running_stats=False" in fn(**dict(ok, tracked=False))
    assert "not float32" in fn(**dict(ok, param_dtypes=(f32, torch.bfloat16)))
    assert "momentum=None" in fn(**dict(ok, momentum_given=False))
    assert "another" in fn(**dict(ok, foreign=True))
    # the measured classes: the launch only where it was ahead beyond the spread in both runs
    bf = torch.bfloat16
    d40 = [(128, c, hw, k) for hw, row in ((1024, ((32, 1), (128, 7), (208, 12), (224, 13))),
                                           (256, ((112, 1), (208, 7), (288, 12), (304, 13))),
                                           (64, ((152, 1), (248, 7), (328, 12), (344, 13)))) for c, k in row]
    d121 = [(32, c, hw, k) for hw, row in ((3136, ((64, 1), (160, 4), (224, 6), (256, 7))),
                                           (784, ((128, 1), (320, 7), (480, 12), (512, 13))),
                                           (196, ((256, 1), (640, 13), (992, 24), (1024, 25))),
                                           (49, ((512, 1), (768, 9), (992, 16), (1024, 17)))) for c, k in row]
    for n, c, hw, k in d40 + d121:
        for dt in (f32, bf, torch.float16):
            for grad in (False, True):
                assert ops.densebn_pays(1, c, hw, k, dt, grad) is False, (c, hw, k)      # a batch of one never pays
        assert ops.densebn_pays(n, c, hw, k, f32, False) is ((n == 128 and hw >= 256) or (hw == 3136 and k >= 4)), (c, hw)
        assert ops.densebn_pays(n, c, hw, k, bf, False) is (n == 128 or (hw == 3136 and k >= 4)), (c, hw)
        assert ops.densebn_pays(n, c, hw, k, f32, True) is ((hw == 1024 and k >= 12) or (hw == 3136 and k >= 4)), (c, hw)
        assert ops.densebn_pays(n, c, hw, k, bf, True) is ((hw == 1024 and k >= 12) or (hw == 3136 and k >= 6)), (c, hw)
        for grad in (False, True):
            assert ops.densebn_pays(n, c, hw, k, torch.float16, grad) is ops.densebn_pays(n, c, hw, k, bf, grad)


def segments_case(dtype, chans, n, h, w, seed=5):
    g = torch.Generator().manual_seed(seed)
    segs = [(0.5 + 2 * torch.randn(n, c, h, w, generator=g, dtype=dtype)).requires_grad_() for c in chans]
    c = sum(chans)
    gamma = (1 + 0.5 * torch.randn(c, generator=g, dtype=dtype)).requires_grad_()
    beta = torch.randn(c, generator=g, dtype=dtype).requires_grad_()
    up = torch.randn(n, c, h, w, generator=g, dtype=dtype)
    rm, rv = torch.randn(c, generator=g, dtype=dtype), 0.5 + torch.rand(c, generator=g, dtype=dtype)
    return segs, gamma, beta, up, rm, rv


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 2e-5)], ids=["f64", "f32"])
@pytest.mark.parametrize("case", [((5, 3, 3), 3, 5, 7), ((4,), 2, 1, 1), ((1,) * 6, 2, 3, 3)], ids=["5+3+3", "4", "6x1"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_composed_route_on_the_cpu_is_the_restatement(relu, case, dtype, tol):
    """float64: 1e-12 of the largest magnitude (one formula twice).  float32: 2e-5, some hundred units of 2^-23 for
    sums of at most 105 terms in another order."""
    chans, n, h, w = case
    segs, gamma, beta, up, rm, rv = segments_case(dtype, chans, n, h, w)
    want = D.pre_act(segs, gamma, beta, relu)
    want_rm, want_rv = D.R.running(rm, rv, want["mean"], want["var"], n * h * w, 0.25)
    for fn, feats in ((HF.dense_batch_norm_act_composed, segs), (HF.dense_batch_norm_act, HF.DenseFeatures(segs)),
                      (HF.dense_batch_norm_act, tuple(segs))):
        rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(3)
        y = fn(feats, rm_, rv_, gamma, beta, training=True, momentum=0.25, relu=relu, num_batches_tracked=nbt)
        assert y.shape == (n, sum(chans), h, w) and int(nbt) == 4
        grads = torch.autograd.grad(y, segs + [gamma, beta], up)
        ref = D.pre_act_grads(segs, gamma, beta, up, (y > 0) if relu else None)
        pairs = [("y", y, want["y"]), ("running_mean", rm_, want_rm), ("running_var", rv_, want_rv),
                 ("dgamma", grads[-2], ref["dgamma"]), ("dbeta", grads[-1], ref["dbeta"])]
        pairs += [(f"dx{k}", grads[k], ref["dx"][k]) for k in range(len(segs))]
        for key, got, ref_t in pairs:
            err = float((got.detach().double() - ref_t).abs().max())
            assert err <= tol * max(float(ref_t.abs().max()), 1.0), (key, err)
    # eval mode: the running statistics are read, nothing is updated
    rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(3)
    y = HF.dense_batch_norm_act(segs, rm_, rv_, gamma, beta, training=False, relu=relu, num_batches_tracked=nbt)
    ref_y = D.pre_act_eval(segs, rm, rv, gamma, beta, relu)
    assert float((y.detach().double() - ref_y).abs().max()) <= tol * max(float(ref_y.abs().max()), 1.0)
    assert torch.equal(rm_, rm) and torch.equal(rv_, rv) and int(nbt) == 3
    # a plain tensor is a one-segment list
    one = HF.dense_batch_norm_act(segs[0], None, None, gamma[:chans[0]], beta[:chans[0]], training=True, relu=relu)
    two = F.batch_norm(segs[0], None, None, gamma[:chans[0]], beta[:chans[0]], True, 0.0, 1e-5)
    assert torch.equal(one.detach(), (F.relu(two) if relu else two).detach())


def test_dense_features_bookkeeping():
    a, b = torch.randn(2, 3, 4, 4), torch.randn(2, 5, 4, 4)
    feats = HF.DenseFeatures(a)
    assert len(feats) == 1 and feats.channels == 3 and feats.cat() is a and feats[0] is a
    assert feats.append(b) is feats and len(feats) == 2 and feats.channels == 8 and list(feats) == [a, b]
    assert torch.equal(feats.cat(), torch.cat([a, b], 1))
    assert len(HF.DenseFeatures()) == 0 and len(HF.DenseFeatures([a, b])) == 2 and HF.DenseFeatures((a, b))[1] is b
    for bad in (torch.randn(3, 4), "x", None):
        with pytest.raises(ValueError, match="segment"):
            feats.append(bad)
    assert len(feats) == 2
    with pytest.raises(_cabi.TadmmError, match="HIP device"):
        feats.stats()                                  # the statistics are the launch's: there is no CPU path
    assert feats._stats == [None, None]
    # the composed route creates no statistics
    HF.dense_batch_norm_act(feats, None, None, torch.ones(8), torch.zeros(8), training=True)
    assert feats._stats == [None, None]
    with pytest.raises(ValueError, match="at least one"):
        HF.dense_batch_norm_act(HF.DenseFeatures(), None, None, None, None, training=True)


def test_composed_route_options_and_argument_errors(monkeypatch):
    segs, gamma, beta, up, rm, rv = segments_case(torch.float32, (5, 3), 2, 4, 4)
    segs = [s.detach() for s in segs]
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        HF.dense_batch_norm_act([torch.randn(1, 5, 1, 1), torch.randn(1, 3, 1, 1)], rm.clone(), rv.clone(), gamma, beta,
                                training=True)
    # momentum=None is nn.BatchNorm2d's cumulative average; affine=False and no tracked statistics are F.batch_norm's
    bn = torch.nn.BatchNorm2d(8, momentum=None)
    twin = torch.nn.BatchNorm2d(8, momentum=None)
    for _ in range(3):
        xs = [torch.randn(2, 5, 4, 4), torch.randn(2, 3, 4, 4)]
        assert torch.equal(HF.dense_batch_norm_act_module(bn, xs, relu=False), twin(torch.cat(xs, 1)))
    assert int(bn.num_batches_tracked) == 3 and torch.equal(bn.running_var, twin.running_var)
    for mod in (torch.nn.BatchNorm2d(8, affine=False), torch.nn.BatchNorm2d(8, track_running_stats=False).eval(),
                torch.nn.GroupNorm(2, 8)):
        xs = [torch.randn(2, 5, 4, 4), torch.randn(2, 3, 4, 4)]
        assert torch.equal(HF.dense_batch_norm_act_module(mod, HF.DenseFeatures(xs)), F.relu(mod(torch.cat(xs, 1))))
    # everything the launch refuses reaches the composed route under route=None and raises under route="launch"
    calls = []
    composed = HF.dense_batch_norm_act_composed
    monkeypatch.setattr(HF, "dense_batch_norm_act_composed", lambda *a, **k: calls.append(1) or composed(*a, **k))
    monkeypatch.setattr(ops, "densebn_pays", lambda *a, **k: True)
    cl = [s.contiguous(memory_format=torch.channels_last) for s in segs]
    many = [torch.randn(2, 1, 4, 4) for _ in range(MAX_SEG + 1)]
    w_many, rm_many = torch.ones(MAX_SEG + 1), torch.zeros(MAX_SEG + 1)
    cases = [(dict(feats=segs, training=True), "HIP device"), (dict(feats=cl, training=True), "HIP device"),
             (dict(feats=[segs[0], segs[1].double()], training=True), "HIP device")]
    for case, text in cases:
        kw = dict(feats=segs, running_mean=rm.clone(), running_var=rv.clone(), weight=gamma, bias=beta)
        kw.update(case)
        args = [kw.pop(k) for k in ("feats", "running_mean", "running_var", "weight", "bias")]
        before = len(calls)
        try:
            HF.dense_batch_norm_act(*args, **kw)
        except RuntimeError:
            pass                                      # torch refuses mixed operands on its own
        assert len(calls) == before + 1, case
        with pytest.raises(_cabi.TadmmError, match="route='launch' cannot take .*" + text):
            HF.dense_batch_norm_act(*args, route="launch", **kw)
    before = len(calls)
    HF.dense_batch_norm_act(many, rm_many.clone(), w_many.clone(), w_many, rm_many, training=True)
    assert len(calls) == before + 1
    with pytest.raises(ValueError):
        HF.dense_batch_norm_act(segs, rm, rv, gamma, beta, training=True, route="fastest")
    for bad in (dict(weight=gamma[:-1]), dict(momentum=1.5), dict(running_mean=rm[:3]), dict(feats=[segs[0][0]]),
                dict(feats=[])):
        kw = dict(feats=segs, running_mean=rm, running_var=rv, weight=gamma, bias=beta, training=True)
        kw.update(bad)
        args = [kw.pop(k) for k in ("feats", "running_mean", "running_var", "weight", "bias")]
        with pytest.raises(ValueError):
            HF.dense_batch_norm_act(*args, **kw)


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
    sd = D.state64(mod, requires_grad=True)
    up = torch.randn(mod(x).shape, generator=torch.Generator().manual_seed(1), dtype=x.dtype)
    names = [n for n, _ in mod.named_parameters()]
    want = ref_fn(D.f64(x), sd)
    want_g = torch.autograd.grad(want, [sd[n] for n in names], D.f64(up))
    got = mod(x)
    got_g = torch.autograd.grad(got, list(mod.parameters()), up)
    for key, a, b in [("out", got, want)] + list(zip(names, got_g, want_g)):
        assert float((a.detach().double() - b.detach()).abs().max()) <= tol * max(float(b.detach().abs().max()), 1e-3), key


def small_cifar(**kw):
    return DC.TenDenseNet(10, num_classes=7, growth_rate=4, bottleneck=False, hp_dict=NoRanks, **kw)


def small_inet(**kw):
    return DI.TenDenseNet(growth_rate=4, block_config=(2, 2), num_classes=5, hp_dict=NoRanks, **kw)


def test_small_models_on_the_cpu_are_the_restatement():
    """Depth 10 with growth 4 (CIFAR, two basic layers per block) and block_config (2, 2) with growth 4 (ImageNet) on
    the composed route.  Output and every parameter gradient in float64, where one formula is computed twice (1e-9 of
    the largest magnitude), in eval and in training mode; in float32 the eval logits (1e-4)."""
    torch.manual_seed(3)
    cifar, inet = randomise(small_cifar(), 4), randomise(small_inet(), 5)
    assert [len(b.layer) for b in (cifar.block1, cifar.block2, cifar.block3)] == [2, 2, 2] and cifar.in_planes == 16
    assert cifar.trans1.conv1.in_channels == 16 and cifar.trans1.conv1.out_channels == 8
    assert inet.num_features == 16 and len(inet.features.denseblock2) == 2 and not hasattr(inet.features, "transition2")
    for model, ref, img in ((cifar, D.cifar_densenet, torch.randn(3, 3, 32, 32)), (inet, D.inet_densenet, torch.randn(3, 3, 32, 32))):
        assert model.set_route("composed") is model
        want = ref(D.f64(img), D.state64(model), model, False)
        got = model.eval()(img)
        assert float((got.detach().double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
        model.double()
        for training in (False, True):
            check_module(model, lambda x64, sd: ref(x64, sd, model, training), img.double(), 1e-9, training)
        model.float()
    assert int(cifar.bn1.num_batches_tracked) == 2 and int(cifar.block2.layer[1].bn1.num_batches_tracked) == 2
    assert int(inet.features.norm5.num_batches_tracked) == 2
    # the bottleneck blocks and the reference's other options run: dropout, the deep stems, checkpointing
    bott = randomise(DC.TenDenseNet(16, num_classes=7, growth_rate=4, bottleneck=True, dropRate=0.1, hp_dict=NoRanks), 6)
    assert isinstance(bott.block1.layer[1], DC.TenBottleneckBlock) and bott(torch.randn(2, 3, 32, 32)).shape == (2, 7)
    bott.double().eval()
    img = torch.randn(2, 3, 32, 32, dtype=torch.float64)
    check_module(bott, lambda x64, sd: D.cifar_densenet(x64, sd, bott, False), img, 1e-9, False)
    for kw in (dict(stem_type="deep"), dict(stem_type="deep_tiered"), dict(stem_type="deep_tiered_narrow"),
               dict(memory_efficient=True), dict(drop_rate=0.2), dict(global_pool="max")):
        model = small_inet(**kw)
        out = model(torch.randn(2, 3, 32, 32))
        assert out.shape == (2, 5)
        out.sum().backward()
        assert all(p.grad is not None for p in model.parameters())
    eff, plain = small_inet(memory_efficient=True).double(), small_inet().double()
    plain.load_state_dict(eff.state_dict())
    x = torch.randn(2, 3, 32, 32, dtype=torch.float64)
    assert float((eff(x) - plain(x)).detach().abs().max()) <= 1e-12
    model = small_inet()
    model.reset_classifier(3)
    assert model(torch.randn(2, 3, 32, 32)).shape == (2, 3) and model.get_classifier() is model.classifier
    # a block returns the holder; its concatenation is the reference's output
    blk = cifar.block1.eval()
    x = torch.randn(2, 8, 8, 8)
    feats = blk(x)
    assert isinstance(feats, HF.DenseFeatures) and len(feats) == 3 and feats[0] is x and feats.cat().shape == (2, 16, 8, 8)
    layer = blk.layer[0]
    want = torch.cat([x, layer.conv1(F.relu(layer.bn1(x)))], 1)
    assert torch.allclose(layer(x).cat(), want, rtol=0, atol=1e-6)
    with pytest.raises(_cabi.TadmmError, match="route='launch' cannot take"):
        cifar.set_route("launch")(torch.randn(2, 3, 32, 32))
    with pytest.raises(_cabi.TadmmError, match="route='launch' cannot take"):
        inet.set_route("launch")(torch.randn(2, 3, 32, 32))
    with pytest.raises(ValueError):
        inet.set_route("fastest")


def test_state_dict_keys_of_the_shipped_tables():
    """The key sets of tkr_densenet40 (table tk_densenet40 2x) and tkc_densenet121 (tk_densenet121 2x) against the lists
    under tests/golden/.  timm is not installed where the reference could have been constructed, so the lists were derived
    by reading it: nn.Module registration of densenet_cifar_tt.py (conv1, block{S}.layer.{I}.bn1 / conv1, trans{S}.bn1 /
    conv1, bn1, fc; depth 40 without bottleneck is twelve basic layers per block) and densenet_inet_tt.py
    (features.conv0, norm0, denseblock{S}.denselayer{I}.norm1 / conv1 / norm2 / conv2, transition{S}.norm / conv, norm5,
    classifier; pools and ReLUs own no keys), the BatchNorm2d entries weight, bias, running_mean, running_var,
    num_batches_tracked, and for a convolution named in the table the parameters its class registers -- TKConv2dR:
    first_factor, core_tensor, last_factor; TKConv2dC: first_kernel, core_kernel, last_kernel; SVDConv2dC (conv1 and the
    transitions of the ImageNet file): left_kernel, right_kernel."""
    for name, mod in (("tkr_densenet40", DC), ("tkc_densenet121", DI)):
        with open(os.path.join(GOLDEN, f"{name}_state_dict_keys.json")) as f:
            want = json.load(f)
        model = getattr(mod, name)(get_hp_dict(name, "2"))
        got = list(model.state_dict())
        assert len(want) == len(set(want)) and set(got) == set(want), sorted(set(got) ^ set(want))[:8]
        other = getattr(mod, name)(get_hp_dict(name, "2"))
        other.load_state_dict(model.state_dict())
        assert all(torch.equal(v, model.state_dict()[k]) for k, v in other.state_dict().items())
    assert "features.transition1.conv.left_kernel" in want and "features.denseblock1.denselayer1.conv2.core_kernel" in want
    assert isinstance(model.features.denseblock2.denselayer1.conv1, DI.SVDConv2dC)
    assert isinstance(model.features.denseblock1.denselayer1.conv1, torch.nn.Conv2d)
    assert isinstance(model.features.denseblock4.denselayer16.conv2, DI.TKConv2dC)


def test_factories_argument_errors(tmp_path):
    assert DC.FACTORIES == ("tkr_densenet40",) and DI.FACTORIES == ("tkc_densenet121", "tkc_densenet201", "tkc_densenet264")
    for mod in (DC, DI):
        for name in mod.FACTORIES:
            assert getattr(mod, name).__name__ == name
    for fn in (DC.tkr_densenet40, DI.tkc_densenet121):
        with pytest.raises(ValueError, match="nothing is downloaded"):
            fn(NoRanks, decompose=True)
        with pytest.raises(ValueError, match="URL"):
            fn(NoRanks, decompose=True, path="https://example.org/densenet.pth")
        with pytest.raises(ValueError, match="nothing is downloaded"):
            fn(NoRanks, pretrained=True)
    with pytest.raises(ValueError, match="nothing is downloaded"):
        DI.tkc_densenet201(NoRanks, decompose=True, pretrained=True)   # the reference downloads timm's densenet201 here
    dense = DC.tkr_densenet40(NoRanks, num_classes=4)
    assert dense.fc.out_features == 4 and len(dense.block3.layer) == 12 and dense.in_planes == 344
    assert isinstance(dense.block2.layer[3].conv1, torch.nn.Conv2d)
    sd = {k: v + 1 for k, v in dense.state_dict().items()}
    again = DC.tkr_densenet40(NoRanks, decompose=True, dense_dict=sd, num_classes=4)
    assert all(torch.equal(v, sd[k]) for k, v in again.state_dict().items())
    path = os.path.join(tmp_path, "dense.pth")
    torch.save(sd, path)
    for kw in (dict(decompose=True), dict(pretrained=True)):
        loaded = DC.tkr_densenet40(NoRanks, path=path, num_classes=4, **kw)
        assert all(torch.equal(v, sd[k]) for k, v in loaded.state_dict().items())
    # no table ships for densenet264: the factory takes the caller's; its third block has 64 layers, 65 segments at norm5
    d264 = DI.tkc_densenet264(NoRanks, num_classes=3)
    assert [len(getattr(d264.features, f"denseblock{s}")) for s in (1, 2, 3, 4)] == [6, 12, 64, 48]
    assert d264.classifier.out_features == 3 and len(d264.features.denseblock3) + 1 <= ops.densebn_max_segments()
    assert get_hp_dict("tkc_densenet264", "2") is None


def test_import_lines():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import densenet_cifar_tt as DC; import densenet_inet_tt as DI; "
            "import tadmm; from tadmm import densenet_cifar_layers as C, densenet_inet_layers as I; "
            "assert tadmm.densenet_cifar_layers is C and tadmm.densenet_inet_layers is I; "
            "assert all(getattr(DC, n) is getattr(C, n) and getattr(tadmm, n) is getattr(C, n) for n in C.FACTORIES); "
            "assert all(getattr(DI, n) is getattr(I, n) and getattr(tadmm, n) is getattr(I, n) for n in I.FACTORIES); "
            "assert all(getattr(DC, n) is getattr(C, n) for n in ('TenBasicBlock', 'TenBottleneckBlock', "
            "'TenTransitionBlock', 'TenDenseBlock', 'TenDenseNet', '_ten_densenet')); "
            "assert all(getattr(DI, n) is getattr(I, n) for n in ('TenDenseLayer', 'TenDenseBlock', 'TenDenseTransition', "
            "'TenDenseNet', '_ten_densenet')); assert C.TenDenseBlock is not I.TenDenseBlock; "
            "from tadmm.functional import DenseFeatures; assert tadmm.DenseFeatures is DenseFeatures")
    subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "dnn-compression-tensor-admm_amd", "dropin")], check=True)
