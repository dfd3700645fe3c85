"""The one-launch LSTM recurrence (csrc/lstm.hip), its backward through time and the TTLSTM layer on the MI355X, against
the float64 restatement of tests/_lstm_ref.py.  Error measure: max|a - ref| / max|ref| per tensor, every element
compared; bar `R.bar(e32)` = max(4 e32, 2e-6) with e32 the error of the float32 restatement of the same case and tensor
against float64 (tests/test_lstm_host_cpu.py prints them), so the yardstick never involves the kernel.

Measured on the device (all cases, both gate kinds): see DESIGN.md section 17."""
import functools

import numpy as np
import pytest
import torch

import _lstm_ref as R
from _unaligned import guards_intact, misaligned
from tadmm import ops
from tadmm import functional as HF
from tadmm._cabi import TadmmError
from tadmm.rnn_layers import TTLSTM, entry

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = list(R.CASES)


@functools.lru_cache(maxsize=None)
def dev_inputs(case):
    d = R.inputs(case)
    out = {k: torch.from_numpy(v).to(DEV) for k, v in d.items() if k != "cores"}
    out["cores"] = [torch.from_numpy(c).to(DEV) for c in d["cores"]]
    return out


def check(case, gate, got: dict, level="kernel"):
    ref, e32 = (R.kernel_reference if level == "kernel" else R.layer_reference)(case, gate), R.e32(case, gate, level)
    bad = []
    for k, t in got.items():
        err = R.rel_err(t.detach().cpu().numpy(), ref[k])
        print(f"{case}/{gate}/{level} {k}: device {err:.2e}  float32 restatement {e32[k]:.2e}  bar {R.bar(e32[k]):.2e}")
        if not err <= R.bar(e32[k]):
            bad.append((k, err, R.bar(e32[k])))
    assert not bad, bad


def run(case, gate, route, grad=False, rows=None):
    """lstm_sequence on the case's inputs (optionally a slice of batch rows); with `grad` also the gradients of
    sum(y dy) + sum(hT dhT) + sum(cT dcT)."""
    d = dev_inputs(case)
    sl = slice(None) if rows is None else rows
    xp0, h0, c0 = d["xp"][:, sl].contiguous(), d["h0"][sl].contiguous(), d["c0"][sl].contiguous()
    if not grad:
        with torch.no_grad():
            y, (hT, cT) = HF.lstm_sequence(xp0, d["w_hh"], h0, c0, gate, route)
        return {"y": y, "hT": hT, "cT": cT}
    xp0, h0, c0 = (t.clone().requires_grad_(True) for t in (xp0, h0, c0))
    w = d["w_hh"].clone().requires_grad_(True)
    b = torch.zeros(xp0.shape[2], device=DEV, requires_grad=True)
    y, (hT, cT) = HF.lstm_sequence(xp0 + b, w, h0, c0, gate, route)
    ((y * d["dy"][:, sl]).sum() + (hT * d["dhT"][sl]).sum() + (cT * d["dcT"][sl]).sum()).backward()
    return {"y": y, "hT": hT, "cT": cT, "dXp": xp0.grad, "dWhh": w.grad, "dbias": b.grad, "dh0": h0.grad, "dc0": c0.grad}


@pytest.mark.parametrize("route", ["launch", "composed"])
@pytest.mark.parametrize("gate", R.GATES)
@pytest.mark.parametrize("case", CASES)
def test_forward_against_float64(case, gate, route):
    assert ops.lstm_fits(R.sizes(case)[3])
    check(case, gate, run(case, gate, route))


@pytest.mark.parametrize("gate", R.GATES)
@pytest.mark.parametrize("case", CASES)
def test_backward_against_float64_and_run_to_run(case, gate):
    a, b = run(case, gate, "launch", grad=True), run(case, gate, "launch", grad=True)
    check(case, gate, a)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs from run to run"


@pytest.mark.parametrize("gate", R.GATES)
@pytest.mark.parametrize("case", ["odd", "two_wg"])
def test_composed_backward_against_float64(case, gate):
    check(case, gate, run(case, gate, "composed", grad=True))


def make_layer(case, gate):
    T, B, n_in, H = R.sizes(case)
    d = dev_inputs(case)
    m = TTLSTM(n_in, H, hp_dict=entry("rnn", R.tt_shapes(case), R.CASES[case][4]), name="rnn", dense_w_hh=d["w_hh"],
               dense_b=d["bias"], gate=gate).to(DEV)
    with torch.no_grad():
        for p, c in zip(m.i2h.tt_cores, d["cores"]):
            p.copy_(c)
    return m


@pytest.mark.parametrize("gate", R.GATES)
@pytest.mark.parametrize("case", CASES)
def test_layer_outputs_and_core_gradients(case, gate):
    d = dev_inputs(case)
    m = make_layer(case, gate)
    y, (hT, cT) = m(d["x"], (d["h0"], d["c0"]))
    ((y * d["dy"]).sum() + (hT * d["dhT"]).sum() + (cT * d["dcT"]).sum()).backward()
    got = {"y": y, "hT": hT, "cT": cT, "dWhh": m.h2h_weight.grad, "dbias": m.bias.grad}
    for k, p in enumerate(m.i2h.tt_cores):
        got[f"dcore{k}"] = p.grad
    check(case, gate, got, "layer")
    m.batch_first = True
    with torch.no_grad():
        yb, (hb, cb) = m(d["x"].transpose(0, 1).contiguous(), (d["h0"], d["c0"]))
        y2, (h2, c2) = m.eval()(d["x"].transpose(0, 1).contiguous(), (d["h0"], d["c0"]))
    assert yb.shape == (y.shape[1], y.shape[0], y.shape[2]) and torch.equal(yb, y2) and torch.equal(hb, h2)
    check(case, gate, {"y": yb.transpose(0, 1), "hT": hb, "cT": cb}, "layer")


@pytest.mark.parametrize("gate", R.GATES)
@pytest.mark.parametrize("case", CASES)
def test_save_is_invisible(case, gate):
    d = dev_inputs(case)
    planes = ops.lstm_planes(d["w_hh"])
    a = ops.lstm_seq(d["xp"], planes, d["h0"], d["c0"], gate == "sigmoid")
    b = ops.lstm_seq_save(d["xp"], planes, d["h0"], d["c0"], gate == "sigmoid")
    for x, y in zip(a, b[:3]):
        assert torch.equal(x, y)
    assert torch.equal(b[4][-1], a[2])                          # the last saved cell state is cT
    assert torch.isfinite(b[3]).all() and b[3].min() >= -1 and b[3].max() <= 1


@pytest.mark.parametrize("gate", R.GATES)
def test_rows_are_independent(gate):
    """Every row of `two_wg` run alone (B = 1) is bitwise its row of the B = 17 launch, forward and dXp: padding rows or
    units that leak into real ones would show here."""
    full = run("two_wg", gate, "launch", grad=True)
    for r in range(R.sizes("two_wg")[1]):
        one = run("two_wg", gate, "launch", grad=True, rows=slice(r, r + 1))
        for k in ("y", "dXp"):
            assert torch.equal(one[k][:, 0], full[k][:, r]), (k, r)
        for k in ("hT", "cT", "dh0", "dc0"):
            assert torch.equal(one[k][0], full[k][r]), (k, r)


@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("case", ["odd", "two_wg", "b1"])
def test_unaligned_operands(case, off):
    """Xp, Y and dZ cut out of sentinel-filled buffers 4 and 12 bytes past a 16-byte boundary: bitwise the aligned run
    (which takes the 16-byte paths: H % 4 == 0 in these cases), guards untouched."""
    d = dev_inputs(case)
    T, B, _, H = R.sizes(case)
    planes, planes_t = ops.lstm_planes(d["w_hh"]), ops.lstm_planes(d["w_hh"], transpose=True)
    y, hT, cT, g, c = ops.lstm_seq_save(d["xp"], planes, d["h0"], d["c0"])
    dz, dh0, dc0 = ops.lstm_seq_bwd(planes_t, g, c, d["c0"], d["dy"], d["dhT"], d["dcT"])
    xp_u = misaligned(d["xp"], off)
    y_u = misaligned(torch.zeros(T, B, H, device=DEV), off)
    dz_u = misaligned(torch.zeros(T, B, 4 * H, device=DEV), off)
    y2, hT2, cT2, g2, c2 = ops.lstm_seq_save(xp_u, planes, d["h0"], d["c0"], out={"y": y_u})
    assert y2.data_ptr() == y_u.data_ptr()
    dz2, dh02, dc02 = ops.lstm_seq_bwd(planes_t, g2, c2, d["c0"], misaligned(d["dy"], off), d["dhT"], d["dcT"], dz=dz_u)
    assert dz2.data_ptr() == dz_u.data_ptr()
    for a, b in ((y, y2), (hT, hT2), (cT, cT2), (g, g2), (c, c2), (dz, dz2), (dh0, dh02), (dc0, dc02)):
        assert torch.equal(a, b)
    assert guards_intact(xp_u) and guards_intact(y_u) and guards_intact(dz_u)


@pytest.mark.parametrize("case", ["long", "ucf11"])
def test_state_chaining(case):
    d = dev_inputs(case)
    T = R.sizes(case)[0]
    planes = ops.lstm_planes(d["w_hh"])
    y, hT, cT = ops.lstm_seq(d["xp"], planes, d["h0"], d["c0"])
    y1, h1, c1 = ops.lstm_seq(d["xp"][:T // 2], planes, d["h0"], d["c0"])
    y2, h2, c2 = ops.lstm_seq(d["xp"][T // 2:], planes, h1, c1)
    assert torch.equal(torch.cat([y1, y2]), y) and torch.equal(h2, hT) and torch.equal(c2, cT)


def test_default_state_is_zeros():
    d = dev_inputs("odd")
    T, B, _, H = R.sizes("odd")
    planes = ops.lstm_planes(d["w_hh"])
    z = torch.zeros(B, H, device=DEV)
    for a, b in zip(ops.lstm_seq(d["xp"], planes), ops.lstm_seq(d["xp"], planes, z, z)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", R.RECORDED)
def test_layer_against_the_recorded_reference(golden_dir, name):
    """TTLSTM on the recorded weights and inputs against the reference's own float32 run.  The recorded run is e_rec
    from the float64 restatement; the device may be bar(e_rec) from float64, hence bar(e_rec) + e_rec from the record."""
    d = R.recorded(golden_dir, name)
    y64, c64 = R.restate_recorded(d)
    T, B, n_in = d["x"].shape
    H = d["w_hh"].shape[1]
    t = lambda a: torch.from_numpy(np.asarray(a)).to(DEV)
    m = TTLSTM(n_in, H, hp_dict=entry("rnn", d["tt_shapes"].tolist(), d["ranks"].tolist()), name="rnn",
               dense_w_hh=t(d["w_hh"]), dense_b=t(d["bias"])).to(DEV)
    with torch.no_grad():
        for p, c in zip(m.i2h.tt_cores, d["cores"]):
            p.copy_(t(c))
        y, (hT, cT) = m(t(d["x"]), (t(d["h0"]), t(d["c0"])))
    for got, rec, ref in ((y, d["y"], y64), (cT, d["cT"], c64), (hT, d["y"][-1], y64[-1])):
        e_rec = R.rel_err(rec, ref)
        err = R.rel_err(got.cpu().numpy(), rec.astype(np.float64))
        print(f"{name}: device vs record {err:.2e}, record vs float64 {e_rec:.2e}")
        assert err <= R.bar(e_rec) + e_rec


def test_from_lstm_full_ranks_against_torch_lstm():
    """Full TT ranks: the decomposition of weight_ih_l0 is exact to rounding, so the layer must agree with torch.nn.LSTM
    (float64, CPU) on the bar of the float32 torch.nn.LSTM's own error."""
    torch.manual_seed(3)
    n_in, H, T, B = 60, 24, 5, 3
    lstm = torch.nn.LSTM(n_in, H)
    x = torch.randn(T, B, n_in)
    h0, c0 = 0.5 * torch.randn(1, B, H), 0.5 * torch.randn(1, B, H)
    l64 = torch.nn.LSTM(n_in, H).double()
    l64.load_state_dict({k: v.double() for k, v in lstm.state_dict().items()})
    with torch.no_grad():
        y64, (h64, c64) = l64(x.double(), (h0.double(), c0.double()))
        y32, (h32, c32) = lstm(x, (h0, c0))
    m = TTLSTM.from_lstm(lstm.to(DEV), entry("rnn", [8, 3, 4, 3, 4, 5], [1, 8, 24, 60, 20, 5, 1]), "rnn").to(DEV)
    assert m.gate == "sigmoid" and not m.batch_first
    with torch.no_grad():
        y, (hT, cT) = m(x.to(DEV), (h0[0].to(DEV), c0[0].to(DEV)))
    for got, f32, ref, what in ((y, y32, y64, "y"), (hT, h32[0], h64[0], "hT"), (cT, c32[0], c64[0], "cT")):
        e = R.rel_err(f32.numpy(), ref.numpy())
        err = R.rel_err(got.cpu().numpy(), ref.numpy())
        print(f"from_lstm {what}: device {err:.2e}, float32 nn.LSTM {e:.2e}")
        assert err <= R.bar(e)


def test_hidden_size_above_the_limit_takes_the_composed_route():
    H, n_in, T, B = 272, 16, 3, 2
    assert not ops.lstm_fits(H)
    torch.manual_seed(5)
    m = TTLSTM(n_in, H, hp_dict=entry("rnn", [64, 17, 4, 4], [1, 4, 4, 4, 1]), name="rnn").to(DEV)
    x = torch.randn(T, B, n_in, device=DEV)
    with torch.no_grad():
        y, (hT, cT) = m(x)
        with pytest.raises(TadmmError):
            m(x, route="launch")
    outs = {}
    for dtype in (torch.float64, torch.float32):
        co = lambda a: a.detach().cpu().to(dtype)
        w_ih = R.recover([co(c) for c in m.i2h.tt_cores]).reshape(4 * H, n_in)
        xp = (co(x).reshape(T * B, n_in) @ w_ih.t() + co(m.bias)).reshape(T, B, 4 * H)
        z = torch.zeros(B, H, dtype=dtype)
        outs[dtype] = [t.double().numpy() for t in R.step_loop(xp, co(m.h2h_weight), z, z, "hardsigmoid")]
    for got, ref, f32 in zip((y, hT, cT), outs[torch.float64], outs[torch.float32]):
        assert R.rel_err(got.cpu().numpy(), ref) <= R.bar(R.rel_err(f32, ref))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_inputs_are_refused(dtype):
    m = make_layer("odd", "hardsigmoid")
    x = dev_inputs("odd")["x"].to(dtype)
    with pytest.raises(TadmmError):
        m(x)
    with pytest.raises(TadmmError):
        HF.lstm_sequence(dev_inputs("odd")["xp"].to(dtype), dev_inputs("odd")["w_hh"])
