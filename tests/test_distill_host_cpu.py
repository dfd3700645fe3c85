"""Host side of the distillation loss (no GPU): the float64 restatement of tests/_distill_ref.py against the reference's
recorded runs (G15), the descriptor and workspace arithmetic of the C ABI, every refusal of `tadmm_distill_loss`, the
module's recognition of base criteria and its errors, and the invariants of the case table the device tests rely on."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import _distill_ref as R
from tadmm import _cabi, ops
from tadmm import functional as HF
from tadmm import losses as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_matches_the_recorded_reference(golden_dir):
    """Loss and gradients within 1e-6 relative (the same formulas in float64 against the reference's float32 run)."""
    index = R.golden_index(golden_dir)
    assert len(index) >= 24
    seen = set()
    for meta in index:
        d = R.recorded(golden_dir, meta["name"])
        k = d["k"] if meta["tuple"] else d["s"]
        kw = R.recorded_kwargs(meta)
        loss, gs, gk, _, _ = R.restate(d["s"], k if kw["kd"] != "none" else None, d["t"], d["target"], **kw)
        ref = float(d["loss"][0])
        assert abs(float(loss) - ref) <= 1e-6 * abs(ref), meta
        if not meta["tuple"] and gk is not None:
            gs, gk = gs + gk, None
        assert (gs - d["grad_s"]).abs().max() <= 1e-6 * d["grad_s"].abs().max(), meta
        if meta["tuple"]:
            want = d["grad_k"].to(torch.float64)
            got = gk if gk is not None else torch.zeros_like(want)
            assert (got - want).abs().max() <= 1e-6 * max(float(want.abs().max()), 1e-30), meta
        seen.add((meta["type"], meta["criterion"], meta["tuple"]))
    assert {t for t, _, _ in seen} == {"none", "soft", "hard"} and {c for _, c, _ in seen} == {"ce", "ce_ls", "ce_prob"}
    assert {(m["B"], m["C"]) for m in index} == {(2, 3), (5, 10), (7, 100), (3, 257)}
    assert {m["alpha"] for m in index} == {0.0, 0.5, 1.0} and {m["tau"] for m in index} == {1.0, 3.0}


def test_fixture_is_small(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "g15_distill.npz")) < 300 * 1024


def test_descriptor_size_matches_library():
    assert _cabi.load().tadmm_distill_desc_bytes() == C.sizeof(_cabi.DistillDesc)


@pytest.mark.parametrize("B", [1, 2, 16, 17, 64, 65, 1024, 100000])
def test_workspace_matches_hand_count(B):
    assert ops.distill_workspace_bytes(B) == R.workspace_bytes_by_hand(B)


def test_workspace_query_refusals():
    lib = _cabi.load()
    size = C.c_size_t()
    d = _cabi.DistillDesc()
    d.B = 0
    assert lib.tadmm_distill_workspace_bytes(C.byref(d), C.byref(size)) == -1
    assert lib.tadmm_distill_workspace_bytes(None, C.byref(size)) == -1
    d.B = 4
    assert lib.tadmm_distill_workspace_bytes(C.byref(d), None) == -1


def test_launch_entry_refuses_before_launching():
    """No device is needed: every refusal comes before the first HIP call that would want one."""
    lib = _cabi.load()
    h = C.c_void_p()
    lib.tadmm_create(0, C.byref(h))
    assert h, "a handle needs no device"
    raw = (C.c_char * 8192)()
    p = C.addressof(raw) + (-C.addressof(raw)) % 16

    def desc(**kw):
        d = _cabi.DistillDesc()
        d.s, d.k, d.t, d.labels, d.dense = p, p + 256, p + 512, p + 768, p + 1024
        d.s_ld = d.k_ld = d.t_ld = d.dense_ld = 4
        d.workspace, d.workspace_bytes = p + 2048, 1024
        d.loss_dev, d.loss_f32_dev, d.counts_dev = p + 4096, p + 4160, p + 4224
        d.grad_s, d.grad_k = p + 5120, p + 6144
        d.ignore_index, d.eps, d.alpha, d.tau = -100, 0.1, 0.5, 2.0
        d.B, d.C, d.dtype = 3, 4, _cabi.CHAIN_F32
        d.base_kind, d.kd_kind = _cabi.DISTILL_BASE_INDEX, _cabi.DISTILL_KD_SOFT_KL
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    invalid = [
        (dict(B=0), "B >= 1"), (dict(C=0), "C >= 1"), (dict(B=-2), "B >= 1"),
        (dict(dtype=3), "type"), (dict(dtype=-1), "type"),
        (dict(base_kind=3), "base kind"), (dict(base_kind=-1), "base kind"),
        (dict(kd_kind=4), "KD kind"), (dict(kd_kind=-1), "KD kind"),
        (dict(base_kind=0, kd_kind=0), "both kinds"),
        (dict(s=None), "s is NULL"), (dict(k=None), "k is NULL"), (dict(t=None), "t is NULL"),
        (dict(labels=None), "labels"), (dict(base_kind=2, dense=None), "dense"),
        (dict(s_ld=3), "stride of s"), (dict(k_ld=3), "stride of k"), (dict(t_ld=0), "stride of t"),
        (dict(base_kind=2, dense_ld=3), "dense"),
        (dict(tau=0.0), "tau"), (dict(tau=-1.0), "tau"), (dict(kd_kind=3, tau=0.0), "tau"),
        (dict(eps=-0.1), "eps"), (dict(eps=1.5), "eps"), (dict(eps=float("nan")), "eps"),
        (dict(s=p + 2), "s is not aligned"), (dict(dtype=_cabi.CHAIN_F16, k=p + 257), "k is not aligned"),
        (dict(t=p + 513), "t is not aligned"), (dict(labels=p + 772), "labels"),
        (dict(base_kind=2, dense=p + 1026), "dense"), (dict(loss_dev=None), "loss_dev"),
        (dict(loss_dev=p + 4100), "loss_dev"), (dict(counts_dev=None), "counts_dev"), (dict(counts_dev=p + 4228), "counts"),
        (dict(loss_f32_dev=p + 4162), "loss_dev"), (dict(grad_s=p + 5122), "gradient"), (dict(grad_k=p + 6145), "gradient"),
    ]
    for kw, text in invalid:
        assert lib.tadmm_distill_loss(h, C.byref(desc(**kw)), None) == -1, kw
        assert text in lib.tadmm_last_error(h).decode(), (kw, lib.tadmm_last_error(h))
    for kw in (dict(workspace=None), dict(workspace_bytes=511), dict(workspace_bytes=0), dict(workspace=p + 2052)):
        assert lib.tadmm_distill_loss(h, C.byref(desc(**kw)), None) == -2, kw
        assert "workspace" in lib.tadmm_last_error(h).decode()
    assert lib.tadmm_distill_loss(h, None, None) == -1
    assert "NULL" in lib.tadmm_last_error(h).decode()
    assert lib.tadmm_distill_loss(None, C.byref(desc()), None) == -1
    lib.tadmm_destroy(h)


def test_type_string_assertion_and_missing_kd_output():
    with pytest.raises(AssertionError):
        L.DistillationLoss(torch.nn.CrossEntropyLoss(), None, "medium", 0.5, 1.0)
    for kind in ("none", "soft", "hard"):
        L.DistillationLoss(torch.nn.CrossEntropyLoss(), None, kind, 0.5, 1.0)

    class Own(torch.nn.Module):           # a criterion the module calls as it is; it accepts a list
        def forward(self, outputs, labels):
            return outputs[0].sum() * 0.0

    crit = L.DistillationLoss(Own(), torch.nn.Identity(), "soft", 0.5, 1.0)
    with pytest.raises(ValueError, match="Tuple"):
        crit(torch.zeros(2, 3), [torch.zeros(2, 3), torch.zeros(2, 3)], torch.zeros(2, dtype=torch.int64))


def test_criterion_recognition():
    ce = torch.nn.CrossEntropyLoss
    assert L.recognise(ce()) == ("by_target", 0.0, -100)
    assert L.recognise(ce(label_smoothing=0.1, ignore_index=7)) == ("by_target", pytest.approx(0.1), 7)
    assert L.recognise(ce(weight=torch.ones(3))) is None
    assert L.recognise(ce(reduction="sum")) is None and L.recognise(ce(reduction="none")) is None
    assert L.recognise(L.LabelSmoothingCrossEntropy(0.2)) == ("index", pytest.approx(0.2), None)
    assert L.recognise(L.SoftTargetCrossEntropy()) == ("dense", 0.0, None)
    assert L.recognise(torch.nn.MSELoss()) is None and L.recognise(torch.nn.NLLLoss()) is None

    # classes that are only NAMED like them and carry the same attributes (another library's own)
    LabelSmoothingCrossEntropy = type("LabelSmoothingCrossEntropy", (), {"smoothing": 0.3, "confidence": 0.7})
    SoftTargetCrossEntropy = type("SoftTargetCrossEntropy", (), {})
    CrossEntropyLoss = type("CrossEntropyLoss", (), {"weight": None, "reduction": "mean", "ignore_index": -1,
                                                     "label_smoothing": 0.05})
    assert L.recognise(LabelSmoothingCrossEntropy()) == ("index", pytest.approx(0.3), None)
    assert L.recognise(SoftTargetCrossEntropy()) == ("dense", 0.0, None)
    assert L.recognise(CrossEntropyLoss()) == ("by_target", pytest.approx(0.05), -1)
    assert L.recognise(type("LabelSmoothingCrossEntropy", (), {})()) is None          # the attribute is missing
    assert L.recognise(type("CrossEntropyLoss", (), {"weight": None})()) is None


def test_the_two_small_criteria_are_the_formulas():
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(6, 9, generator=g, dtype=torch.float64), torch.randint(0, 9, (6,), generator=g)
    want = torch.nn.functional.cross_entropy(x, y, label_smoothing=0.1)
    assert torch.allclose(L.LabelSmoothingCrossEntropy(0.1)(x, y), want, rtol=1e-12)
    q = torch.softmax(torch.randn(6, 9, generator=g, dtype=torch.float64), dim=1)
    assert torch.allclose(L.SoftTargetCrossEntropy()(x, q), torch.nn.functional.cross_entropy(x, q), rtol=1e-12)


def test_unknown_criterion_is_called_as_it_is():
    calls = []

    class Own(torch.nn.Module):
        def forward(self, outputs, labels):
            calls.append((outputs, labels))
            return outputs.sum()

    x, y = torch.ones(2, 3), torch.zeros(2, dtype=torch.int64)
    crit = L.DistillationLoss(Own(), None, "none", 0.5, 1.0)
    assert float(crit(None, x, y)) == 6.0 and calls[0][0] is x and crit.bad_labels() == 0
    # with distillation on, the criterion runs first (on the host tensors), then the KD term refuses the CPU tensor
    crit = L.DistillationLoss(Own(), lambda inp: torch.zeros(2, 3), "hard", 0.5, 1.0)
    with pytest.raises(_cabi.TadmmError, match="outputs_kd"):
        crit(None, x, y)
    assert len(calls) == 2


def test_cpu_tensors_and_mixed_inputs_raise():
    x, y = torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)
    crit = L.DistillationLoss(torch.nn.CrossEntropyLoss(), lambda inp: torch.zeros(2, 3), "soft", 0.5, 1.0)
    with pytest.raises(_cabi.TadmmError, match="outputs.*no CPU path"):
        crit(None, x, y)
    with pytest.raises(_cabi.TadmmError, match="outputs"):
        L.DistillationLoss(torch.nn.CrossEntropyLoss(), None, "none", 0.5, 1.0)(None, (x, x), y)
    for fn in (HF.distillation_loss, HF.distillation_loss_composed):
        with pytest.raises(_cabi.TadmmError, match="outputs .*no CPU path"):
            fn(x, x, x, y)
        with pytest.raises(_cabi.TadmmError, match="outputs_kd"):
            fn(None, x, x, None, base="none", kd="hard")
        with pytest.raises(ValueError, match="base"):
            fn(x, x, x, y, base="weighted")
        with pytest.raises(ValueError, match="both"):
            fn(x, x, x, y, base="none", kd="none")
    with pytest.raises(ValueError, match="route"):
        HF.distillation_loss(x, x, x, y, route="native")
    with pytest.raises(_cabi.TadmmError):
        HF.soft_cross_entropy(x, x)
    with pytest.raises(_cabi.TadmmError, match="no CPU path"):
        ops.distill_loss(x, x, x, y, base="index", kd="soft")
    with pytest.raises(ValueError):
        ops.distill_loss(x, x, x, y, base="index", kd="medium")
    assert ops.distill_loss_pays(256, 1000, torch.float16, True) in (True, False)


def test_dropin_import_line():
    code = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]\n"
            "from losses import DistillationLoss\n"
            "import tadmm.losses\n"
            "assert DistillationLoss is tadmm.losses.DistillationLoss\n"
            "print('ok')")
    pkg = os.path.join(ROOT, "dnn-compression-tensor-admm_amd")
    out = subprocess.run([sys.executable, "-c", code, os.path.join(pkg, "dropin"), pkg], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_case_table_invariants():
    """What tests/test_gpu_distill.py relies on: about 60 cases, every C with every type, every kind present, no teacher
    tie in any case, and at least one kept row in the ignore / bad-label case."""
    assert 55 <= len(R.CASES) <= 70
    assert {(c["B"], c["C"], c["dtype"]) for c in R.CASES} >= {(b, c, d) for b, c in R.SHAPES for d in R.DTYPES}
    assert {(c["kd"], c["tau"]) for c in R.CASES} >= set(R.KDS) and {(c["base"], c["eps"]) for c in R.CASES} >= set(R.BASES)
    assert {(c["kd"], c["base"]) for c in R.CASES} >= {(k, b) for k, _ in R.KDS for b, _ in R.BASES}
    for c in R.CASES:
        s, k, t, target = R.case_inputs(c)
        assert R.teacher_ties(t) == 0, c["id"]
        assert s.dtype == R.DTYPES[c["dtype"]] and tuple(s.shape) == (c["B"], c["C"])
    for C_ in (3, 17, 1000):
        y = R.label_case(C_)
        kept = (y != -100) & (y >= 0) & (y < C_)
        assert int(kept.sum()) >= 1 and int(((y != -100) & ~kept).sum()) == 2
    t = torch.zeros(1, 8)
    t[0, 2] = t[0, 5] = 4.0
    assert R.teacher_ties(t) == 1


def test_restatement_label_rules_and_ulp():
    s, k, t, _ = R.make_inputs(7, 5, "float32", 1)
    y = R.label_case(5)
    loss, gs, gk, kept, bad = R.restate(s, None, None, y, base="index", kd="none")
    rows = torch.tensor([0, 2, 5, 6])
    want = torch.nn.functional.cross_entropy(s[rows].double(), y[rows])
    assert kept == 4 and bad == 2 and abs(float(loss) - float(want)) < 1e-12
    assert float(gs[[1, 3, 4]].abs().max()) == 0.0
    nan, _, _, kept, _ = R.restate(s, None, None, torch.full((7,), -100), base="index", kd="none")
    assert kept == 0 and bool(torch.isnan(nan))
    x = torch.tensor([1.0, 1.5, 2.0, 3e-5, 1e-9, 0.0], dtype=torch.float64)
    assert R.ulp(x, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -26 * 4, 2.0 ** -24, 2.0 ** -24]
    assert R.ulp(x[:3], torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6]
