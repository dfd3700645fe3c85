"""Orthogonality regulariser (orthogonal.py) without a device: factor selection, orientation and the squeeze errors
against the G9 fixtures recorded from the reference (tests/golden/make_golden_orth.py), and the drop-in module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "dnn-compression-tensor-admm_amd")


@pytest.fixture(scope="module")
def g9(golden_dir):
    return json.load(open(os.path.join(golden_dir, "g9_orthogonal.json")))


def build(params, values=None):
    """Module tree with the given dotted parameter names, created in order (as the G9 generator does)."""
    root = torch.nn.Module()
    for name, shape, rg in params:
        *path, leaf = name.split(".")
        m = root
        for part in path:
            if not hasattr(m, part):
                m.add_module(part, torch.nn.Module())
            m = getattr(m, part)
        t = torch.from_numpy(values[name]).clone() if values is not None else torch.randn(shape)
        m.register_parameter(leaf, torch.nn.Parameter(t, requires_grad=rg))
    return root


def test_select_matches_g9(g9):
    from tadmm.orthogonal import select
    for key, case in g9["cases"].items():
        model = build(case["params"])
        assert [n for n, _ in model.named_parameters()] == case["order"], key
        sel = select(model)
        assert [n for n, _, _ in sel] == case["matched"], key
        assert {n: rows for n, _, rows in sel} == case["gram_of_rows"], key
        params = dict(model.named_parameters())
        assert all(p is params[n] for n, p, _ in sel), key


def test_square_factors_follow_the_reference_rule(g9):
    # shape[0] < shape[1] is false for a square factor: E = P^T P - I
    rows = g9["cases"]["tk_linear"]["gram_of_rows"]
    assert rows["head.first_factor"] is False and rows["head.last_factor"] is False
    assert rows["fc.first_factor"] is True and rows["fc.last_factor"] is False


@pytest.mark.parametrize("key", ["rank1", "unit_channel", "left_kernel_3x3"])
def test_squeeze_errors_before_device_work(g9, key, monkeypatch):
    from tadmm import orthogonal
    err = g9["errors"][key]
    assert err["type"] == "RuntimeError"
    model = build(err["params"])
    with pytest.raises(RuntimeError, match=err["failing"].replace(".", r"\.")):
        orthogonal.select(model)

    def no_device(*a, **k):
        raise AssertionError("device work started before the selection error")

    monkeypatch.setattr(orthogonal, "_plan_for", no_device)
    monkeypatch.setattr(orthogonal._OrthFn, "apply", no_device)
    with pytest.raises(RuntimeError, match=err["failing"].replace(".", r"\.")):
        orthogonal.append_double_l2_loss(model, torch.zeros(()), 0.1, "cuda")


def test_no_match_returns_the_callers_loss_without_a_device(g9):
    from tadmm.orthogonal import append_double_l2_loss
    model = build(g9["cases"]["no_match"]["params"])
    loss = torch.zeros(())
    assert append_double_l2_loss(model, loss, 0.1, "cuda") is loss


def test_matched_cpu_factor_raises_naming_it():
    from tadmm.orthogonal import append_double_l2_loss
    model = build([("blk.first_factor", (4, 9), True)])
    with pytest.raises(RuntimeError, match=r"blk\.first_factor"):
        append_double_l2_loss(model, torch.zeros(()), 0.1, "cpu")


def test_g9_fixture_consistency(g9, golden_dir):
    # the fp64 golden is the reference's own formula in fp64: restate it here to pin what G9 holds
    data = np.load(os.path.join(golden_dir, "g9_orthogonal.npz"))
    rho = g9["rho"]
    for key, case in g9["cases"].items():
        total = 0.0
        for n in case["matched"]:
            p = data[f"{key}__{n}"].astype(np.float64).squeeze()
            g = p @ p.T if case["gram_of_rows"][n] else p.T @ p
            total += 0.5 * rho * np.sum((g - np.eye(g.shape[0])) ** 2)
        assert abs(total - case["loss64"]) <= 1e-12 * max(1.0, abs(total)), key


def test_package_and_dropin_expose_append_double_l2_loss():
    import tadmm
    from tadmm import orthogonal
    assert tadmm.append_double_l2_loss is orthogonal.append_double_l2_loss
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import orthogonal, tadmm.orthogonal as t; "
            "assert orthogonal.append_double_l2_loss is t.append_double_l2_loss; print('ok')")
    r = subprocess.run([sys.executable, "-c", code, os.path.join(PKG_DIR, "dropin")], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


@pytest.mark.parametrize("shape", [(1, 4, 8), (4, 1, 8)])
def test_unit_leading_dimension_that_squeezes_to_a_matrix_is_refused(shape):
    # the reference would broadcast eye(1) against the squeezed Gram here; refused rather than computed differently
    from tadmm.orthogonal import select
    model = build([("blk.first_factor", shape, True)])
    with pytest.raises(RuntimeError, match=r"blk\.first_factor"):
        select(model)


def test_c_abi_workspace_bytes_rejects_bad_descriptors():
    import ctypes as C
    from tadmm import _cabi
    lib = _cabi.load()
    size = C.c_size_t()

    def descs(*rows_cols_ld):
        d = (_cabi.OrthDesc * len(rows_cols_ld))()
        for i, (r, c, ld) in enumerate(rows_cols_ld):
            d[i].P, d[i].rows, d[i].cols, d[i].ld, d[i].gram_of_rows, d[i].grad_offset = 4096, r, c, ld, 1, -1
        return d

    ok = descs((8, 16, 16), (4096, 256, 256))
    assert lib.tadmm_orth_workspace_bytes(2, ok, C.byref(size)) == 0 and size.value > 0
    assert lib.tadmm_orth_workspace_bytes(0, ok, C.byref(size)) == -1                  # n <= 0
    assert lib.tadmm_orth_workspace_bytes(1, descs((0, 16, 16)), C.byref(size)) == -1  # rows * cols == 0
    assert lib.tadmm_orth_workspace_bytes(1, descs((8, 0, 16)), C.byref(size)) == -1
    assert lib.tadmm_orth_workspace_bytes(1, descs((8, 16, 12)), C.byref(size)) == -1  # ld < cols
    bad = descs((8, 16, 16))
    bad[0].P = 4098                                                                     # not 4-byte aligned
    assert lib.tadmm_orth_workspace_bytes(1, bad, C.byref(size)) == -1
