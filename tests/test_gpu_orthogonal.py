"""Orthogonality regulariser (orthogonal.py: append_double_l2_loss) on the MI355X: G9 parity with the reference, whole
rank tables against fp64, near-orthonormal factors, autograd, autocast, caches, determinism and errors."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TABLES = ["tk_resnet50_3x", "tk_resnet32_2x", "tk_deit_tiny_2x", "tk_vgg16_2x", "svd_mobilenetv2_cifar_2x"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g9(golden_dir):
    return json.load(open(os.path.join(golden_dir, "g9_orthogonal.json"))), \
        np.load(os.path.join(golden_dir, "g9_orthogonal.npz"))


def build(params, values, dev, key=None):
    root = torch.nn.Module()
    for name, shape, rg in params:
        *path, leaf = name.split(".")
        m = root
        for part in path:
            if not hasattr(m, part):
                m.add_module(part, torch.nn.Module())
            m = getattr(m, part)
        v = values[f"{key}__{name}"] if key is not None else values[name]
        m.register_parameter(leaf, torch.nn.Parameter(torch.from_numpy(np.asarray(v)).clone().to(dev), requires_grad=rg))
    return root


def fp64(model, rho):
    """The reference's formula in float64 on P.double(): (loss, {name: gradient})."""
    from tadmm.orthogonal import select
    loss, grads = 0.0, {}
    for name, p, rows in select(model):
        P = p.detach().double().squeeze()
        G = P @ P.t() if rows else P.t() @ P
        E = G - torch.eye(G.shape[0], dtype=torch.float64, device=G.device)
        loss += 0.5 * rho * float((E * E).sum())
        grads[name] = (2 * rho * (E @ P if rows else P @ E)).reshape(p.shape)
    return loss, grads


def orth(model, rho, dev, dtype=torch.float32):
    from tadmm.orthogonal import append_double_l2_loss
    return append_double_l2_loss(model, torch.zeros((), device=dev, dtype=dtype), rho, dev)


def zero_grads(model):
    for p in model.parameters():
        p.grad = None


# ---------------------------------------------------------------- G9: the reference itself
def test_g9_parity(g9, dev):
    meta, data = g9
    rho = meta["rho"]
    for key, case in meta["cases"].items():
        if not case["matched"]:
            continue
        model = build(case["params"], data, dev, key)
        loss = orth(model, rho, dev)
        assert loss.dtype == torch.float32
        assert abs(loss.item() - case["loss32"]) <= 1e-5 * abs(case["loss32"]), key
        loss.backward()
        l64 = orth(build(case["params"], data, dev, key), rho, dev, torch.float64)
        assert abs(l64.item() - case["loss64"]) <= 1e-9 * abs(case["loss64"]), key
        for name, p in model.named_parameters():
            if name in case["with_grad"]:
                np.testing.assert_allclose(p.grad.cpu().numpy(), data[f"{key}__grad32__{name}"], rtol=1e-4, atol=1e-7,
                                           err_msg=f"{key}:{name}")
            else:
                assert p.grad is None, f"{key}:{name}"     # frozen or not regularised


def test_g9_frozen_factor_adds_to_the_loss(g9, dev):
    meta, data = g9
    case = meta["cases"]["frozen"]
    model = build(case["params"], data, dev, "frozen")
    assert not model.blk.first_factor.requires_grad
    loss = orth(model, meta["rho"], dev, torch.float64)
    assert abs(loss.item() - case["loss64"]) <= 1e-9 * case["loss64"]
    loss.backward()
    assert model.blk.first_factor.grad is None and model.blk.last_factor.grad is not None


def test_g9_no_match_returns_the_callers_loss(g9, dev):
    from tadmm.orthogonal import append_double_l2_loss
    meta, data = g9
    model = build(meta["cases"]["no_match"]["params"], data, dev, "no_match")
    loss = torch.full((), 2.5, device=dev)
    out = append_double_l2_loss(model, loss, meta["rho"], dev)
    assert out is loss and float(out) == 2.5


# ---------------------------------------------------------------- whole rank tables against fp64
@pytest.mark.parametrize("table", TABLES)
def test_tables_against_fp64(table, dev):
    from tadmm import workloads
    rho = 3e-3
    model = workloads.orth_model(table).to(dev)
    loss = orth(model, rho, dev, torch.float64)
    loss.backward()
    l64, g64 = fp64(model, rho)
    assert abs(loss.item() - l64) <= 1e-9 * abs(l64), (loss.item(), l64)
    params = dict(model.named_parameters())
    assert g64
    for name, g in g64.items():
        got = params[name].grad.double()
        err = float((got - g).abs().max())
        assert err <= 1e-6 * float(g.abs().max()), (name, err, float(g.abs().max()))


def _near_orthonormal(dev):
    gen = torch.Generator().manual_seed(7)
    m = torch.nn.Module()
    for i, (rows, cols) in enumerate([(16, 256), (288, 96), (48, 48), (64, 4096)]):
        a = torch.randn(max(rows, cols), min(rows, cols), generator=gen, dtype=torch.float64)
        q, _ = torch.linalg.qr(a)
        q = q if rows > cols else q.t()
        q = q + 1e-4 * torch.randn(q.shape, generator=gen, dtype=torch.float64)
        name = "first_factor" if rows < cols else "last_factor"
        sub = torch.nn.Module()
        sub.register_parameter(name, torch.nn.Parameter(q.float().contiguous()))
        m.add_module(f"l{i}", sub)
    return m.to(dev)


def test_near_orthonormal_factors_keep_their_digits(dev):
    from tadmm.orthogonal import select
    model = _near_orthonormal(dev)
    rho = 1.0
    loss = orth(model, rho, dev, torch.float64)
    l64, _ = fp64(model, rho)
    assert 1e-9 < l64 < 1e-2                      # entries of E ~ 1e-4
    assert abs(loss.item() - l64) <= 1e-8 * l64, (loss.item(), l64)
    # an fp32 torch.mm restatement of the reference misses the same bound on the same inputs
    l32 = 0.0
    for _, p, rows in select(model):
        P = p.detach().squeeze()
        G = torch.mm(P, P.t()) if rows else torch.mm(P.t(), P)
        l32 += 0.5 * rho * float(torch.norm(G - torch.eye(G.shape[0], device=dev), p=2) ** 2)
    assert abs(l32 - l64) > 1e-8 * l64, (l32, l64)


# ---------------------------------------------------------------- autograd
def _tk_model(dev, seed=0):
    from tadmm import workloads
    return workloads.orth_model("tk_resnet32_2x", seed).to(dev)


def test_upstream_gradient_scales(dev):
    model = _tk_model(dev)
    orth(model, 0.05, dev).backward()
    g1 = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    zero_grads(model)
    (3 * orth(model, 0.05, dev)).backward()
    for n, g in g1.items():
        torch.testing.assert_close(dict(model.named_parameters())[n].grad, 3 * g, rtol=1e-6, atol=0)


def test_two_live_losses_keep_their_gradients(dev):
    model = _tk_model(dev)
    orth(model, 0.05, dev).backward()
    ga = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    zero_grads(model)
    orth(model, 0.2, dev).backward()
    gb = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    zero_grads(model)
    la = orth(model, 0.05, dev)
    lb = orth(model, 0.2, dev)                    # a second call before the first loss is used
    la.backward()
    for n, p in model.named_parameters():
        if n in ga:
            assert torch.equal(p.grad, ga[n]), n
    zero_grads(model)
    lb.backward()
    for n, p in model.named_parameters():
        if n in gb:
            assert torch.equal(p.grad, gb[n]), n


def test_combines_with_admm_penalty(dev):
    from tadmm.admm import ADMM
    from tadmm.tk_layers import TKLinearM

    class HP:
        ranks = {"fc.first_factor": 4, "fc.last_factor": 4}

    class Tab:
        ranks = {"fc": [8, 6]}

    torch.manual_seed(3)
    model = torch.nn.Module()
    model.fc = TKLinearM(40, 48, hp_dict=Tab, name="fc")
    model = model.to(dev)
    admm = ADMM(model, 2e-3, HP, "svd", dev)
    with torch.no_grad():                         # move W away from Z so that the penalty has a gradient
        for p in model.parameters():
            p.add_(0.01)
    admm.append_admm_loss(torch.zeros((), device=dev)).backward()
    g_admm = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    zero_grads(model)
    orth(model, 0.1, dev).backward()
    g_orth = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    zero_grads(model)
    loss = admm.append_admm_loss(torch.zeros((), device=dev))
    from tadmm.orthogonal import append_double_l2_loss
    loss = append_double_l2_loss(model, loss, 0.1, dev)
    loss.backward()
    for n, p in model.named_parameters():
        want = g_admm.get(n, 0) + g_orth.get(n, 0)
        if isinstance(want, int):
            assert p.grad is None
            continue
        torch.testing.assert_close(p.grad, want, rtol=1e-6, atol=1e-9)
    assert set(g_admm) & set(g_orth)              # both terms reach the same factors


def test_sgd_step_matches_fp64(dev):
    model = _tk_model(dev, seed=5)
    before = {n: p.detach().double().clone() for n, p in model.named_parameters()}
    rho, lr = 0.05, 0.5
    _, g64 = fp64(model, rho)
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    orth(model, rho, dev).backward()
    opt.step()
    for n, p in model.named_parameters():
        want = before[n] - lr * g64[n] if n in g64 else before[n]
        err = float((p.detach().double() - want).abs().max())
        assert err <= 1e-6 * float(want.abs().max()), (n, err)


def test_autocast_and_grad_scaler(g9, dev):
    meta, data = g9
    case = meta["cases"]["tk_linear"]
    model = build(case["params"], data, dev, "tk_linear")
    scale = 1024.0
    scaler = torch.amp.GradScaler("cuda", init_scale=scale)
    with torch.autocast("cuda", dtype=torch.float16):
        x = torch.ones(4, 8, device=dev)
        task = (x @ torch.zeros(8, 8, device=dev)).float().sum()
        assert (x @ x.t()).dtype == torch.float16          # autocast really is active here
        from tadmm.orthogonal import append_double_l2_loss
        total = append_double_l2_loss(model, task, meta["rho"], dev)
    assert total.dtype == torch.float32
    ref = orth(model, meta["rho"], dev, torch.float64).item()
    assert abs(total.item() - ref) <= 1e-6 * ref                     # the value does not depend on autocast
    assert abs(total.item() - case["loss32"]) <= 1e-5 * case["loss32"]
    scaler.scale(total).backward()
    for n, p in model.named_parameters():
        if n in case["with_grad"]:
            np.testing.assert_allclose(p.grad.cpu().numpy() / scale, data[f"tk_linear__grad32__{n}"], rtol=1e-4,
                                       atol=1e-7, err_msg=n)
    zero_grads(model)
    with torch.autocast("cuda", dtype=torch.float16):
        t16 = append_double_l2_loss(model, torch.zeros((), device=dev, dtype=torch.float16), meta["rho"], dev)
    assert t16.dtype == torch.float16
    assert abs(t16.item() - case["loss32"]) <= 2e-3 * case["loss32"]
    t16.backward()
    for n, p in model.named_parameters():
        if n in case["with_grad"]:
            np.testing.assert_allclose(p.grad.cpu().numpy(), data[f"tk_linear__grad32__{n}"], rtol=2e-3, atol=1e-7,
                                       err_msg=n)


# ---------------------------------------------------------------- caches, determinism
def test_data_swap_and_new_layer_repack(dev):
    from tadmm.tk_layers import TKLinearM
    model = _tk_model(dev)
    rho = 0.05
    orth(model, rho, dev)
    p = model[0].first_kernel
    p.data = torch.randn(p.shape, device=dev) * 0.2                 # new storage
    loss = orth(model, rho, dev, torch.float64)
    assert abs(loss.item() - fp64(model, rho)[0]) <= 1e-9 * fp64(model, rho)[0]

    class Tab:
        ranks = {"extra": [12, 10]}

    model.append(TKLinearM(64, 96, hp_dict=Tab, name="extra").to(dev))
    loss = orth(model, rho, dev, torch.float64)
    loss.backward()
    l64, g64 = fp64(model, rho)
    assert abs(loss.item() - l64) <= 1e-9 * l64
    torch.testing.assert_close(model[-1].last_factor.grad.double(), g64[f"{len(model) - 1}.last_factor"], rtol=1e-6,
                               atol=1e-9)


def test_bitwise_deterministic(dev):
    from tadmm import workloads
    model = workloads.orth_model("tk_vgg16_2x").to(dev)
    out = []
    for _ in range(2):
        zero_grads(model)
        loss = orth(model, 0.01, dev, torch.float64)
        loss.backward()
        out.append((loss.detach().clone(), [p.grad.clone() for p in model.parameters() if p.grad is not None]))
    assert torch.equal(out[0][0], out[1][0])
    assert len(out[0][1]) == 26
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- errors
def test_errors_name_the_parameter(dev):
    from tadmm.orthogonal import append_double_l2_loss
    loss = torch.zeros((), device=dev)

    def one(p, device=dev):
        m = torch.nn.Module()
        m.blk = torch.nn.Module()
        m.blk.register_parameter("last_factor", torch.nn.Parameter(p))
        return append_double_l2_loss(m, loss, 0.1, device)

    with pytest.raises(RuntimeError, match=r"blk\.last_factor"):
        one(torch.randn(12, 4))                                          # CPU
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError, match=r"blk\.last_factor"):
            one(torch.randn(12, 4, device=dev, dtype=dt))
    with pytest.raises(RuntimeError, match=r"blk\.last_factor"):
        one(torch.randn(12, 4, device=dev), device="cuda:1")             # another device than `device`
    assert torch.isfinite(one(torch.randn(12, 4, device=dev), device="cuda"))   # 'cuda' = the current device


def test_c_abi_plan_create_status_codes(dev):
    import ctypes as C
    from tadmm import _cabi
    h = _cabi.Handle.get(0)
    lib = h.lib
    P = torch.randn(8, 16, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def descs(rows, cols, ld):
        d = (_cabi.OrthDesc * 1)()
        d[0].P, d[0].rows, d[0].cols, d[0].ld, d[0].gram_of_rows, d[0].grad_offset = P.data_ptr(), rows, cols, ld, 1, 0
        return d

    size = C.c_size_t()
    assert lib.tadmm_orth_workspace_bytes(1, descs(8, 16, 16), C.byref(size)) == 0
    ws = torch.empty(size.value, dtype=torch.uint8, device=dev)
    plan = C.c_void_p()

    def create(n, d, nbytes):
        return lib.tadmm_orth_plan_create(h.ptr, n, d, ws.data_ptr(), nbytes, stream, C.byref(plan))

    assert create(0, descs(8, 16, 16), size.value) == -1                   # n <= 0
    assert create(1, descs(0, 16, 16), size.value) == -1                   # empty factor
    assert create(1, descs(8, 16, 8), size.value) == -1                    # ld < cols
    assert create(1, descs(8, 16, 16), size.value - 1) == -2               # workspace too small
    assert b"workspace" in lib.tadmm_last_error(h.ptr)
    assert create(1, descs(8, 16, 16), size.value) == 0
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    grad = torch.empty(8, 16, device=dev)
    assert lib.tadmm_orth_l2(plan, 0.5, grad.data_ptr(), loss.data_ptr(), stream) == 0
    assert lib.tadmm_orth_l2(plan, 0.5, grad.data_ptr(), None, stream) == -1  # no loss buffer
    lib.tadmm_orth_plan_destroy(plan)
    Pd = P.double()
    E = Pd @ Pd.t() - torch.eye(8, dtype=torch.float64, device=dev)
    assert abs(loss.item() - 0.25 * float((E * E).sum())) <= 1e-12 * loss.item()
    torch.testing.assert_close(grad.double(), (E @ Pd), rtol=1e-6, atol=1e-9)


def test_loss_without_gradient_buffer_is_bitwise_the_same(dev):
    # under no_grad the call passes no gradient buffer and launches only the norm workgroups
    from tadmm import workloads
    model = workloads.orth_model("tk_vgg16_2x").to(dev)
    with_grad = orth(model, 0.01, dev, torch.float64)
    with torch.no_grad():
        no_grad = orth(model, 0.01, dev, torch.float64)
    assert not no_grad.requires_grad
    assert torch.equal(with_grad.detach(), no_grad)
