"""Host side of TinyBERT's layer losses (no GPU): the float64 restatement of tests/_layer_mse_ref.py against the
reference's recorded runs (G20), the composed route on the CPU against the restatement, the descriptor and workspace
arithmetic of the C ABI, every refusal of `tadmm_layer_mse`, the launch-refusal table, the module's errors and the
invariants of the case table the device tests rely on."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import _layer_mse_ref as R
from tadmm import _cabi, ops
from tadmm import functional as HF
from tadmm import losses as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_matches_the_recorded_reference(golden_dir):
    """Losses and gradients within 1e-6 relative: the reference's own float32 statements (a loop over the batch axis of
    the last layer) against the batch_sum formula in float64."""
    index = R.golden_index(golden_dir)
    assert {(m["B"], m["H"], m["S"], m["D"]) for m in index} == {(1, 1, 1, 1), (2, 2, 5, 4), (3, 2, 9, 7), (2, 3, 37, 5)}
    assert sum(m["differ"] for m in index) >= 2 and sum(not m["differ"] for m in index) >= len(index) // 2
    for m in index:
        d = R.recorded(golden_dir, m["name"])
        att, rep, _, (ga, gr) = R.restate(d["s_att"], d["t_att"], d["s_rep"], d["t_rep"])
        for got, want in ((att, d["att_loss"][0]), (rep, d["rep_loss"][0])):
            assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want)), m
        for got, want in ((ga, d["grad_att"]), (gr, d["grad_rep"])):
            assert (got - want).abs().max() <= 1e-6 * max(float(want.abs().max()), 1e-30), m
        if m["differ"]:
            assert m["kept_student"] != m["kept_teacher"]


def test_fixture_is_small(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "g20_layer_mse.npz")) < 300 * 1024


def _inputs(dtype):
    sa = [R.att_pair(3, 2, 9, 11, "float32"), R.att_pair(2, 2, 5, 12, "float32")]
    sr = [R.rep_pair((3, 9, 7), 13), R.rep_pair((2, 5, 4), 14), R.rep_pair((2, 5, 6), 15)]
    cast = lambda pairs: ([s.to(dtype) for s, _ in pairs], [t.to(dtype) for _, t in pairs])
    return cast(sa) + cast(sr)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-6), (torch.float64, 1e-13)])
@pytest.mark.parametrize("reduction", ["batch_sum", "mean"])
def test_composed_route_on_the_cpu(dtype, tol, reduction):
    sa, ta, sr, tr = _inputs(dtype)
    aw, rw = [0.5, 2.0], [1.0, 0.25, 3.0]
    for kw in (dict(), dict(att_weights=aw, rep_weights=rw), dict(threshold=None), dict(threshold=-0.5)):
        kw = dict(kw, reduction=reduction)
        a64, r64, _, g64 = R.restate(sa, ta, sr, tr, **dict(dict(threshold=-100.0), **kw))
        leaves = [s.clone().requires_grad_(True) for s in sa + sr]
        att, rep = HF.intermediate_distillation_loss_composed(leaves[:2], ta, leaves[2:], tr, **kw)
        assert att.dtype == dtype and rep.dtype == dtype and att.dim() == 0 and rep.dim() == 0
        (att + rep).backward()
        assert abs(att.item() - float(a64)) <= tol * abs(float(a64)) and abs(rep.item() - float(r64)) <= tol * abs(float(r64))
        for leaf, g in zip(leaves, g64):
            assert (leaf.grad.double() - g).abs().max() <= tol * float(g.abs().max())
        # the public entry takes the same route for CPU tensors and returns float32
        a2, r2 = HF.intermediate_distillation_loss(sa, ta, sr, tr, **kw)
        assert a2.dtype == torch.float32 and r2.dtype == torch.float32
        assert abs(float(a2) - float(a64)) <= 2e-6 * abs(float(a64))


def test_composed_route_empty_side_and_bare_tensors():
    sa, ta, sr, tr = _inputs(torch.float64)
    a64, r64, _, _ = R.restate(sa[:1], ta[:1], sr[:1], tr[:1])
    s = sa[0].clone().requires_grad_(True)
    att, rep = HF.intermediate_distillation_loss_composed(s, ta[0], sr[0], tr[0])          # tensors in place of lists
    assert abs(att.item() - float(a64)) <= 1e-13 * float(a64) and abs(rep.item() - float(r64)) <= 1e-13 * float(r64)
    for fn in (HF.intermediate_distillation_loss_composed, HF.intermediate_distillation_loss):
        att, rep = fn(s, ta[0], [], [])
        assert rep.dtype == torch.float32 and float(rep) == 0.0 and rep.grad_fn is None and att.grad_fn is not None
        att, rep = fn(None, None, sr[:2], tr[:2])
        assert att.dtype == torch.float32 and float(att) == 0.0 and att.grad_fn is None
        att, rep = fn([], [], [], [])
        assert float(att) == 0.0 and float(rep) == 0.0 and att.grad_fn is None and rep.grad_fn is None
    # the same student in two pairs: autograd sums
    (HF.intermediate_distillation_loss_composed([s, s], [ta[0], ta[0]], [], [])[0]).backward()
    _, _, _, g = R.restate(sa[:1], ta[:1], [], [])
    assert (s.grad - 2 * g[0]).abs().max() <= 1e-13 * float(g[0].abs().max())
    # a teacher that requires grad gets nothing
    t = ta[0].clone().requires_grad_(True)
    HF.intermediate_distillation_loss_composed(sa[0].clone().requires_grad_(True), t, [], [])[0].backward()
    assert t.grad is None


def test_descriptor_size_and_constants_match_the_library():
    lib = _cabi.load()
    assert lib.tadmm_layer_mse_desc_bytes() == C.sizeof(_cabi.LayerMseDesc)
    assert lib.tadmm_layer_mse_max_pairs() == ops.LAYER_MSE_MAX_PAIRS == _cabi.LAYER_MSE_MAX_PAIRS == 32
    chunk, blocks = ops.layer_mse_geometry()
    assert chunk >= 256 and chunk % 16 == 0 and blocks >= 1
    assert lib.tadmm_layer_mse_geometry(None, None) == -1


def test_workspace_matches_hand_count():
    chunk, blocks = ops.layer_mse_geometry()
    for numels in ([1], [chunk - 1], [chunk], [chunk + 1], [1] * 32, [3 * chunk + 1, 1, 2 * chunk],
                   [blocks * chunk], [blocks * chunk + 1], [blocks * chunk + chunk + 3], [blocks * chunk] * 5 + [7],
                   [2 ** 40, 5]):
        assert ops.layer_mse_workspace_bytes(numels) == R.workspace_bytes_by_hand(numels, chunk, blocks), numels


def test_workspace_query_refusals():
    lib = _cabi.load()
    chunk, _ = ops.layer_mse_geometry()
    size = C.c_size_t()
    d = _cabi.LayerMseDesc()
    d.npairs = 1
    d.pairs[0].n = 4
    assert lib.tadmm_layer_mse_workspace_bytes(C.byref(d), C.byref(size)) == 0
    assert lib.tadmm_layer_mse_workspace_bytes(None, C.byref(size)) == -1
    assert lib.tadmm_layer_mse_workspace_bytes(C.byref(d), None) == -1
    for npairs in (0, -1, 33):
        d.npairs = npairs
        assert lib.tadmm_layer_mse_workspace_bytes(C.byref(d), C.byref(size)) == -1
    d.npairs = 1
    for n in (0, -5):
        d.pairs[0].n = n
        assert lib.tadmm_layer_mse_workspace_bytes(C.byref(d), C.byref(size)) == -1
    d.pairs[0].n = chunk * 2 ** 31                     # 2^31 chunks: one beyond int32
    assert lib.tadmm_layer_mse_workspace_bytes(C.byref(d), C.byref(size)) < 0
    d.pairs[0].n = chunk * (2 ** 31 - 1)
    assert lib.tadmm_layer_mse_workspace_bytes(C.byref(d), C.byref(size)) == 0
    with pytest.raises(_cabi.TadmmError):
        ops.layer_mse_workspace_bytes([0])


def test_launch_entry_refuses_before_launching():
    """No device is needed: every refusal comes before the first HIP call that would want one."""
    lib = _cabi.load()
    chunk, _ = ops.layer_mse_geometry()
    h = C.c_void_p()
    lib.tadmm_create(0, C.byref(h))
    assert h, "a handle needs no device"
    raw = (C.c_char * 8192)()
    p = C.addressof(raw) + (-C.addressof(raw)) % 16

    def desc(pair=None, **kw):
        d = _cabi.LayerMseDesc()
        d.npairs, d.dtype = 2, _cabi.CHAIN_F32
        for i in range(2):
            q = d.pairs[i]
            q.s, q.t, q.grad, q.n = p + 512 * i, p + 512 * i + 128, p + 512 * i + 256, 8
            q.scale, q.thr, q.clamp, q.group = 0.125, -100.0, 1 - i, i
        d.workspace, d.workspace_bytes = p + 2048, 256
        d.terms_dev, d.loss_dev, d.loss_f32_dev = p + 4096, p + 4160, p + 4224
        for k, v in (pair or {}).items():
            setattr(d.pairs[1], k, v)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    invalid = [
        (dict(npairs=0), "npairs"), (dict(npairs=33), "npairs"), (dict(npairs=-1), "npairs"),
        (dict(dtype=3), "type"), (dict(dtype=-1), "type"),
        (dict(pair=dict(n=0)), "n = 0"), (dict(pair=dict(n=-3)), "n = -3"),
        (dict(pair=dict(group=2)), "group"), (dict(pair=dict(group=-1)), "group"),
        (dict(pair=dict(s=None)), "NULL"), (dict(pair=dict(t=None)), "NULL"),
        (dict(pair=dict(s=p + 514)), "aligned"), (dict(pair=dict(t=p + 641)), "aligned"),
        (dict(pair=dict(grad=p + 770)), "aligned"), (dict(dtype=_cabi.CHAIN_F16, pair=dict(s=p + 513)), "aligned"),
        (dict(terms_dev=None), "terms_dev"), (dict(loss_dev=None), "loss_dev"), (dict(terms_dev=p + 4100), "terms_dev"),
        (dict(loss_dev=p + 4164), "loss_dev"), (dict(loss_f32_dev=p + 4226), "loss_dev"),
    ]
    for kw, text in invalid:
        assert lib.tadmm_layer_mse(h, C.byref(desc(**kw)), None) == -1, kw
        assert text in lib.tadmm_last_error(h).decode(), (kw, lib.tadmm_last_error(h))
    assert lib.tadmm_layer_mse(h, C.byref(desc(pair=dict(n=chunk * 2 ** 31))), None) < 0
    assert "chunks" in lib.tadmm_last_error(h).decode()
    for kw in (dict(workspace=None), dict(workspace_bytes=255), dict(workspace_bytes=0), dict(workspace=p + 2052)):
        assert lib.tadmm_layer_mse(h, C.byref(desc(**kw)), None) == -2, kw
        assert "workspace" in lib.tadmm_last_error(h).decode()
    assert lib.tadmm_layer_mse(h, None, None) == -1
    assert "NULL" in lib.tadmm_last_error(h).decode()
    assert lib.tadmm_layer_mse(None, C.byref(desc()), None) == -1
    lib.tadmm_destroy(h)


def test_launch_refusal_table():
    ok = dict(is_cuda=True, dtypes=[torch.float32] * 4, npairs=2)
    assert HF.layer_mse_launch_refusal(**ok) is None
    assert HF.layer_mse_launch_refusal(**dict(ok, dtypes=[torch.bfloat16] * 4)) is None
    assert HF.layer_mse_launch_refusal(**dict(ok, dtypes=[torch.float16], npairs=32)) is None
    assert "HIP device" in HF.layer_mse_launch_refusal(**dict(ok, is_cuda=False))
    assert "float64" in HF.layer_mse_launch_refusal(**dict(ok, dtypes=[torch.float64] * 4))
    assert "int64" in HF.layer_mse_launch_refusal(**dict(ok, dtypes=[torch.float32, torch.int64]))
    assert "mixed" in HF.layer_mse_launch_refusal(**dict(ok, dtypes=[torch.float32, torch.bfloat16]))
    assert "33 pairs" in HF.layer_mse_launch_refusal(**dict(ok, npairs=33))
    assert "another device" in HF.layer_mse_launch_refusal(**dict(ok, teacher_foreign=True))


def test_errors_of_the_functions_and_the_module():
    x, y = torch.zeros(2, 3), torch.zeros(2, 4)
    for fn in (HF.intermediate_distillation_loss, HF.intermediate_distillation_loss_composed):
        with pytest.raises(ValueError, match=r"\(2, 3\).*\(2, 4\)"):
            fn([x], [y], [], [])
        with pytest.raises(ValueError, match=r"\(2, 3\).*\(2, 4\)"):
            fn([], [], x, y)
        with pytest.raises(ValueError, match="1 student_atts and 2 teacher_atts"):
            fn([x], [x, x], [], [])
        with pytest.raises(ValueError, match="reduction"):
            fn(x, x, x, x, reduction="sum")
        with pytest.raises(ValueError, match="weights"):
            fn([x, x], [x, x], [], [], att_weights=[1.0])
        with pytest.raises(TypeError, match="student_reps"):
            fn([], [], [3.0], [x])
    with pytest.raises(ValueError, match="route"):
        HF.intermediate_distillation_loss(x, x, x, x, route="native")
    with pytest.raises(_cabi.TadmmError, match="HIP device"):
        HF.intermediate_distillation_loss(x, x, x, x, route="launch")
    with pytest.raises(_cabi.TadmmError, match="no CPU path"):
        ops.layer_mse([x], [x], [1.0], 0, True, -100.0)
    with pytest.raises(_cabi.TadmmError, match="33 pairs"):
        ops.layer_mse([x] * 33, [x] * 33, 1.0, 0, True, -100.0)
    with pytest.raises(ValueError, match="reduction"):
        L.TinyBertLayerLoss(reduction="sum")
    crit = L.TinyBertLayerLoss()
    assert crit.route is None and crit.threshold == -100.0 and crit.reduction == "batch_sum"
    att, rep = crit(x, x + 1, y, y)                           # CPU tensors under the rule: the composed route
    assert float(att) == 2.0 and float(rep) == 0.0            # batch_sum: two samples of mean 1
    crit.route = "launch"
    with pytest.raises(_cabi.TadmmError, match="route='launch' cannot take"):
        crit(x, x, y, y)
    assert ops.layer_mse_pays(1 << 20, 2, torch.float32, True) in (True, False)


def test_dropin_and_package_exports():
    code = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]\n"
            "from losses import TinyBertLayerLoss\n"
            "import tadmm, tadmm.losses\n"
            "assert TinyBertLayerLoss is tadmm.losses.TinyBertLayerLoss is tadmm.TinyBertLayerLoss\n"
            "print('ok')")
    pkg = os.path.join(ROOT, "dnn-compression-tensor-admm_amd")
    out = subprocess.run([sys.executable, "-c", code, os.path.join(pkg, "dropin"), pkg], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_case_table_invariants(golden_dir):
    """What tests/test_gpu_layer_mse.py relies on, checked on the inputs so that no case passes with the clamp idle: in
    every attention pair of at least ten elements that runs on the device, the clamped share of the student's elements
    lies in [0.1, 0.6], and some element is clamped in the student and not in the teacher and some the other way.
    Pairs of fewer than ten elements (the one-element cases, whose share can only be 0 or 1) are exempt; the recorded
    cases are held to the share, and to the two-sided difference where they were drawn with differing masks."""
    chunk, blocks = ops.layer_mse_geometry()
    seen = 0
    for tag, spec in R.shape_cases(chunk, blocks):
        ss, ts = R.case_pairs(spec, 100)
        for s, t in zip(ss, ts):
            if s.numel() < 10:
                continue
            share, s_only, t_only = R.clamp_census(s, t)
            assert 0.1 <= share <= 0.6 and s_only >= 1 and t_only >= 1, (tag, tuple(s.shape), share, s_only, t_only)
            seen += 1
    assert seen >= 40
    for dtype in R.DTYPES:
        for s, t in (R.att_pair(3, 2, 9, 1, dtype), R.att_pair(2, 12, 16, 2, dtype), R.flat_pair(chunk + 1, 3, dtype)):
            share, s_only, t_only = R.clamp_census(s, t)
            assert 0.1 <= share <= 0.6 and s_only >= 1 and t_only >= 1, (dtype, tuple(s.shape))
    for m in R.golden_index(golden_dir):
        d = R.recorded(golden_dir, m["name"])
        if d["s_att"].numel() < 10:
            continue
        share, s_only, t_only = R.clamp_census(d["s_att"], d["t_att"])
        assert 0.1 <= share <= 0.6, m
        assert (s_only >= 1 and t_only >= 1) == m["differ"], m
