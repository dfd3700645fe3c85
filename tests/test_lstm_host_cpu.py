"""Host side of the TT-LSTM (no GPU): the float64 restatement of tests/_lstm_ref.py against the reference's recorded
runs, the descriptor and plan arithmetic of the C ABI, refusals, argument errors, state-dict keys, the reference's
compression and flop figures, and the invariants of the case table the device tests rely on."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _lstm_ref as R
from tadmm import _cabi, ops
from tadmm import functional as HF
from tadmm.rnn_layers import TTLSTM, entry


@pytest.mark.parametrize("name", R.RECORDED)
def test_restatement_matches_the_recorded_reference(golden_dir, name):
    d = R.recorded(golden_dir, name)
    y, cT = R.restate_recorded(d)
    assert y.shape == d["y"].shape
    assert np.abs(y - d["y"]).max() <= 1e-6 * np.abs(d["y"]).max()
    assert np.abs(cT - d["cT"]).max() <= 1e-6 * np.abs(d["cT"]).max()


def test_fixture_is_small(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "g11_tt_lstm.npz")) < 300 * 1024


def test_descriptor_size_matches_library():
    assert _cabi.load().tadmm_lstm_desc_bytes() == C.sizeof(_cabi.LstmDesc)


@pytest.mark.parametrize("H", [1, 15, 16, 17, 24, 32, 33, 64, 65, 128, 129, 144, 255, 256, 257, 512, 100000])
def test_plan_matches_hand_count(H):
    assert ops.lstm_plan(H) == R.plan_by_hand(H)
    assert ops.lstm_fits(H) == (H <= R.MAX_H)
    if H <= R.MAX_H:
        assert ops.lstm_plan(H)[1] <= ops.LSTM_LDS_BYTES
    assert ops.LSTM_MAX_H == R.MAX_H and ops.LSTM_ROWS == R.ROWS


def test_malformed_descriptors_are_refused():
    lib = _cabi.load()
    nbytes, rows = C.c_size_t(), C.c_int()
    assert lib.tadmm_lstm_fits(None, C.byref(nbytes), C.byref(rows)) == -1
    for H in (0, -3):
        d = _cabi.LstmDesc()
        d.H = H
        assert lib.tadmm_lstm_fits(C.byref(d), None, None) == -1
    d = _cabi.LstmDesc()
    d.H = 16
    assert lib.tadmm_lstm_fits(C.byref(d), None, None) == 1       # null outputs are allowed
    with pytest.raises(ValueError):
        ops.lstm_plan(0)


def test_launch_entries_refuse_before_launching():
    """No device is needed: every refusal comes before the first HIP call that would want one."""
    lib = _cabi.load()
    h = C.c_void_p()
    lib.tadmm_create(0, C.byref(h))
    assert h, "a handle needs no device"
    buf = (C.c_float * 64)()
    planes = (C.c_char * 4096)()
    base = C.addressof(planes) + (-C.addressof(planes)) % 16

    def desc(**kw):
        d = _cabi.LstmDesc()
        p = C.addressof(buf)
        d.Xp, d.W, d.Y, d.hT, d.cT, d.G, d.C, d.dZ = p, base, p, p, p, p, p, p
        d.T, d.B, d.H, d.sigmoid = 1, 1, 4, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    cases = [(dict(H=0), -1, "H >= 1"), (dict(H=257), -5, "256"), (dict(T=0), -1, "T >= 1"), (dict(B=0), -1, "B >= 1"),
             (dict(sigmoid=2), -1, "sigmoid"), (dict(W=None), -1, "W"), (dict(W=base + 4), -1, "W"),
             (dict(T=2 ** 41), -1, "2^40")]
    for entry_name in ("tadmm_lstm_seq_fwd", "tadmm_lstm_seq_fwd_save", "tadmm_lstm_seq_bwd"):
        fn = getattr(lib, entry_name)
        for kw, rc, text in cases:
            assert fn(h, C.byref(desc(**kw)), None) == rc, (entry_name, kw)
            assert text in lib.tadmm_last_error(h).decode(), (entry_name, kw, lib.tadmm_last_error(h))
        assert fn(None, C.byref(desc()), None) == -1
    for kw in (dict(Xp=None), dict(Y=C.addressof(buf) + 2), dict(hT=None), dict(cT=None), dict(h0=C.addressof(buf) + 1)):
        assert lib.tadmm_lstm_seq_fwd(h, C.byref(desc(**kw)), None) == -1, kw
    for kw in (dict(G=None), dict(C=None)):
        assert lib.tadmm_lstm_seq_fwd_save(h, C.byref(desc(**kw)), None) == -1, kw
        assert lib.tadmm_lstm_seq_bwd(h, C.byref(desc(**kw)), None) == -1, kw
    for kw in (dict(dZ=None), dict(dY=C.addressof(buf) + 2), dict(dh0=C.addressof(buf) + 1)):
        assert lib.tadmm_lstm_seq_bwd(h, C.byref(desc(**kw)), None) == -1, kw
    lib.tadmm_destroy(h)


def test_route_gate_and_shape_errors():
    xp, w = torch.zeros(2, 3, 16), torch.zeros(16, 4)
    with pytest.raises(ValueError, match="route"):
        HF.lstm_sequence(xp, w, route="native")
    with pytest.raises(ValueError, match="gate"):
        HF.lstm_sequence(xp, w, gate="relu")
    with pytest.raises(ValueError, match="gate"):
        HF.lstm_sequence_composed(xp, w, gate="relu")
    with pytest.raises(ValueError, match="w_hh"):
        HF.lstm_sequence(xp, torch.zeros(12, 4))
    with pytest.raises(ValueError, match="xp"):
        HF.lstm_sequence(torch.zeros(2, 3, 12), w)
    with pytest.raises(ValueError, match="xp"):
        HF.lstm_sequence(torch.zeros(0, 3, 16), w)
    with pytest.raises(ValueError, match="h0"):
        HF.lstm_sequence(xp, w, h0=torch.zeros(3, 5))
    with pytest.raises(_cabi.TadmmError):                     # no CPU path
        HF.lstm_sequence(xp, w)
    with pytest.raises(ValueError):
        ops.lstm_planes(torch.zeros(12, 4))


def _layer(case="odd", **kw):
    T, B, n_in, H = R.sizes(case)
    return TTLSTM(n_in, H, hp_dict=entry("rnn", R.tt_shapes(case), R.CASES[case][4]), name="rnn", **kw)


def test_from_lstm_argument_errors():
    hp = entry("rnn", R.tt_shapes("odd"), R.CASES["odd"][4])
    with pytest.raises(ValueError, match="torch.nn.LSTM"):
        TTLSTM.from_lstm(torch.nn.GRU(60, 24), hp, "rnn")
    for kw in (dict(num_layers=2), dict(bidirectional=True), dict(proj_size=8)):
        with pytest.raises(ValueError, match="one layer"):
            TTLSTM.from_lstm(torch.nn.LSTM(60, 24, **kw), hp, "rnn")
    with pytest.raises(ValueError, match="gate"):
        _layer(gate="tanh")


def test_state_dict_keys_shapes_and_init():
    m = _layer()
    sd = m.state_dict()
    shapes, ranks = R.tt_shapes("odd"), R.CASES["odd"][4]
    assert list(sd) == ["h2h_weight", "bias"] + [f"i2h.tt_cores.{k}" for k in range(len(shapes))]
    assert tuple(sd["h2h_weight"].shape) == (96, 24) and tuple(sd["bias"].shape) == (96,)
    for k, n in enumerate(shapes):
        assert tuple(sd[f"i2h.tt_cores.{k}"].shape) == (ranks[k], n, ranks[k + 1])
    bound = 1 / np.sqrt(24)
    assert sd["h2h_weight"].abs().max() <= bound and sd["bias"].abs().max() <= bound
    assert sd["h2h_weight"].abs().max() > 0.8 * bound
    assert m.i2h.bias is None and m.get_ranks() == ", ".join(map(str, ranks))
    nb = _layer(bias=False)
    assert nb.bias is None and "bias" not in nb.state_dict()
    w = torch.randn(96, 24)
    assert torch.equal(_layer(dense_w_hh=w, dense_b=torch.ones(96)).h2h_weight, w)
    with pytest.raises(_cabi.TadmmError):
        m(torch.zeros(5, 3, 60, dtype=torch.float16))
    with pytest.raises(ValueError):
        m(torch.zeros(5, 3, 61))


def test_compression_and_flops_match_the_reference_scripts(golden_dir):
    z = np.load(os.path.join(golden_dir, "g11_tt_lstm.npz"))
    for tag in ("inference", "compare"):
        in_tt, out_tt, ranks = (z[f"{tag}_{k}"].tolist() for k in ("in_tt", "out_tt", "ranks"))
        H, n_in = int(np.prod(out_tt)), int(np.prod(in_tt))
        m = TTLSTM(n_in, H, hp_dict=entry("rnn", [4 * out_tt[0]] + out_tt[1:] + in_tt, ranks), name="rnn")
        assert m.compression_ratio() == pytest.approx(float(z[f"{tag}_ratio"][0]), rel=1e-9)
        if tag == "compare":
            dense, tt = m.forward_flops()
            assert sum(p.numel() for p in m.i2h.tt_cores) == int(z["compare_tt_params"][0])
            assert tt == int(z["compare_tt_flops"][0])
            assert dense / tt == pytest.approx(float(z["compare_speedup"][0]), rel=1e-9)
            assert m.forward_flops(3) == (3 * dense, 3 * tt)


@pytest.mark.parametrize("case", list(R.CASES))
def test_case_table_invariants_and_e32(case):
    """Every case saturates (>= 1 % of the Hardsigmoid pre-activations beyond +-3) and none sits closer than 2e-5 to the
    kink, so that every element can be compared; the float32 restatement stays within a few 1e-6 of float64."""
    share, dist = R.saturation(case)
    print(f"{case}: {100 * share:.1f} % saturated, nearest to the kink {dist:.2e}")
    assert share >= 0.01 and dist >= 2e-5
    for gate in R.GATES:
        for level in ("kernel", "layer"):
            e = R.e32(case, gate, level)
            print(f"{case}/{gate}/{level}: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
            assert max(e.values()) < 1e-5
