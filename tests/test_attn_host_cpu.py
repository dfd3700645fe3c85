"""Host side of the self-attention (no GPU): the float64 restatement of tests/_attn_ref.py against the reference's
recorded runs (G18), the composed torch route against the restatement, `attn_fits` over its edges, every refusal of the
three C entries, and the module: state-dict keys, the reference's ValueError, the `weights=` hook and the routing rule."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import _attn_ref as R
from tadmm import _cabi, ops
from tadmm import functional as HF
from tadmm.bert_layers import BertSelfAttention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("ctx", "scores", "dq", "dk", "dv")


def test_restatement_matches_the_recorded_reference(golden_dir):
    """Both outputs and the three gradients within 1e-6 relative in the max norm (one formula in float64 against the
    reference's float32 run)."""
    index = R.golden_index(golden_dir)
    assert {(m["B"], m["H"], m["S"], m["d"]) for m in index} == {(2, 3, 8, 32), (2, 2, 17, 26), (1, 2, 128, 64)}
    assert any(m["lengths"] is None for m in index)
    assert all(len(set(m["lengths"])) == len(m["lengths"]) for m in index if m["lengths"])
    for meta in index:
        d = R.recorded(golden_dir, meta["name"])
        assert ("mask" in d) == (meta["lengths"] is not None)
        out = R.restate(d["q"], d["k"], d["v"], d.get("mask"), meta["H"], g_ctx=d["g_ctx"], g_sc=d["g_sc"])
        for key in KEYS:
            want = d[key].to(torch.float64)
            assert float((out[key] - want).abs().max()) <= 1e-6 * float(want.abs().max()), (meta, key)


def test_fixture_is_small(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "g18_attention.npz")) < 700 * 1024


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_composed_route_on_the_cpu_is_the_restatement(p):
    B, H, S, d = 2, 3, 19, 10
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B, S, H * d, generator=g, dtype=torch.float64).requires_grad_() for _ in range(3))
    mask = R.padding_mask([13, 1], S, dtype=torch.float64)
    keep = HF.attention_keep_mask(B, H, S, p, "cpu", generator=g) if p else None
    g_ctx = torch.randn(B, S, H * d, generator=g, dtype=torch.float64)
    g_sc = torch.randn(B, H, S, S, generator=g, dtype=torch.float64)
    ref = R.restate(q, k, v, mask, H, p=p, keep=keep, g_ctx=g_ctx, g_sc=g_sc)
    for fn in (HF.self_attention_composed, HF.self_attention):
        ctx, sc = fn(q, k, v, mask, H, dropout_p=p, training=p > 0, keep=keep)
        dq, dk, dv = torch.autograd.grad((ctx, sc), (q, k, v), (g_ctx, g_sc))
        for key, got in zip(KEYS, (ctx, sc, dq, dk, dv)):
            assert float((got.detach() - ref[key]).abs().max()) <= 1e-12 * float(ref[key].abs().max()), key
    ctx2, none = HF.self_attention_composed(q, k, v, None, H, need_scores=False)
    assert none is None and ctx2.shape == (B, S, H * d)
    with pytest.raises(ValueError):
        HF.self_attention(q, k, v, mask, H, route="fastest")
    with pytest.raises(_cabi.TadmmError):
        HF.self_attention(q, k, v, mask, H, route="launch")          # CPU tensors: there is no CPU kernel


def test_descriptor_size_matches_library():
    assert _cabi.load().tadmm_attn_desc_bytes() == C.sizeof(_cabi.AttnDesc)


def test_fits_over_the_edges():
    for S, want in ((1, True), (512, True), (513, False)):
        assert ops.attn_fits(S, 64) is want
    for d, want in ((1, True), (64, True), (65, False)):
        assert ops.attn_fits(128, d) is want
    for S, d, H in ((0, 64, 1), (128, 0, 1), (128, 64, 0), (-1, 64, 1)):
        with pytest.raises(_cabi.TadmmError):
            ops.attn_fits(S, d, H)
    lib = _cabi.load()
    assert lib.tadmm_attn_fits(None, None) == -1
    size = C.c_size_t(7)
    dsc = _cabi.AttnDesc()
    dsc.S, dsc.d, dsc.H = 512, 64, 12
    assert lib.tadmm_attn_fits(C.byref(dsc), C.byref(size)) == 1 and 0 < size.value <= 64 * 1024
    dsc.S = 513
    assert lib.tadmm_attn_fits(C.byref(dsc), C.byref(size)) == 0 and size.value == 0


def test_workspace_bytes():
    assert ops.attn_workspace_bytes(2, 3, 17) == 1024           # 102 doubles, rounded up to 256 bytes
    assert ops.attn_workspace_bytes(32, 12, 512) == 32 * 12 * 512 * 8
    assert ops.attn_workspace_bytes(0, 12, 512) == 0
    lib = _cabi.load()
    dsc = _cabi.AttnDesc()
    dsc.B, dsc.H, dsc.S = 1, 1, 0
    assert lib.tadmm_attn_workspace_bytes(C.byref(dsc), C.byref(C.c_size_t())) == -1
    assert lib.tadmm_attn_workspace_bytes(None, C.byref(C.c_size_t())) == -1
    dsc.S = 4
    assert lib.tadmm_attn_workspace_bytes(C.byref(dsc), None) == -1


def test_launch_entries_refuse_before_launching():
    """No device is needed: every refusal comes before the first HIP call that would want one."""
    lib = _cabi.load()
    h = C.c_void_p()
    lib.tadmm_create(0, C.byref(h))
    assert h, "a handle needs no device"
    raw = (C.c_char * 16384)()
    p = C.addressof(raw) + (-C.addressof(raw)) % 16

    def desc(**kw):
        d = _cabi.AttnDesc()
        d.q, d.k, d.v = p, p + 512, p + 1024
        d.q_ld = d.k_ld = d.v_ld = 8
        d.q_bs = d.k_bs = d.v_bs = 24
        d.mask, d.keep = p + 1536, p + 1600
        d.ctx, d.scores, d.stats = p + 2048, p + 2560, p + 3072
        d.g_ctx, d.g_sc = p + 3584, p + 4096
        d.dq, d.dk, d.dv = p + 4608, p + 5120, p + 5632
        d.workspace, d.workspace_bytes = p + 6144, 256
        d.p = 0.1
        d.B, d.H, d.S, d.d, d.dtype = 2, 2, 3, 4, _cabi.CHAIN_F32
        for key, val in kw.items():
            setattr(d, key, val)
        return d

    both = [
        (dict(S=0), "S >= 1"), (dict(d=0), "d >= 1"), (dict(H=0), "H >= 1"), (dict(B=-1), "B >= 0"),
        (dict(dtype=3), "type"), (dict(dtype=-1), "type"),
        (dict(q=None), "q is NULL"), (dict(k=None), "k is NULL"), (dict(v=None), "v is NULL"),
        (dict(q=p + 2), "q is not aligned"), (dict(dtype=_cabi.CHAIN_BF16, k=p + 513), "k is not aligned"),
        (dict(v=p + 1025), "v is not aligned"),
        (dict(q_ld=7), "stride of q"), (dict(k_ld=0), "stride of k"), (dict(v_ld=-8), "stride of v"),
        (dict(mask=p + 1538), "mask"),
        (dict(p=1.0), "outside"), (dict(p=-0.1), "outside"), (dict(p=float("nan")), "outside"),
        (dict(keep=None), "without a keep"),
    ]
    fwd_only = [(dict(ctx=None), "ctx"), (dict(ctx=p + 2050), "ctx"), (dict(scores=p + 2561), "scores"),
                (dict(stats=p + 3074), "stats")]
    bwd_only = [(dict(dtype=_cabi.CHAIN_F16), "forward only"), (dict(stats=None), "stats"), (dict(stats=p + 3073), "stats"),
                (dict(g_ctx=p + 3586), "upstream"), (dict(g_sc=p + 4097), "upstream"),
                (dict(dq=None), "dq / dk / dv"), (dict(dk=None), "dq / dk / dv"), (dict(dv=p + 5634), "dq / dk / dv")]
    for entry, cases in ((lib.tadmm_attn_fwd, both + fwd_only), (lib.tadmm_attn_bwd, both + bwd_only)):
        for kw, text in cases:
            assert entry(h, C.byref(desc(**kw)), None) == -1, kw
            assert text in lib.tadmm_last_error(h).decode(), (kw, lib.tadmm_last_error(h))
        for kw in (dict(S=513), dict(d=65)):
            assert entry(h, C.byref(desc(q_ld=200, k_ld=200, v_ld=200, **kw)), None) == -5, kw
        assert entry(h, None, None) == -1 and "NULL" in lib.tadmm_last_error(h).decode()
        assert entry(None, C.byref(desc()), None) == -1
        assert entry(h, C.byref(desc(B=0)), None) == 0               # an empty batch succeeds, nothing to launch
    for kw in (dict(workspace=None), dict(workspace_bytes=255), dict(workspace=p + 6148)):
        assert lib.tadmm_attn_bwd(h, C.byref(desc(**kw)), None) == -2, kw
        assert "workspace" in lib.tadmm_last_error(h).decode()
    lib.tadmm_destroy(h)


def test_module_state_dict_keys_and_errors():
    mod = BertSelfAttention(48, 4, 0.1)
    assert list(mod.state_dict()) == ["query.weight", "query.bias", "key.weight", "key.bias", "value.weight", "value.bias"]
    assert [n for n, _ in mod.named_children()] == ["query", "key", "value", "dropout"]
    assert mod.dropout.p == 0.1 and mod.attention_head_size == 12 and mod.all_head_size == 48
    with pytest.raises(ValueError, match=r"The hidden size \(50\) is not a multiple of the number of attention heads \(4\)"):
        BertSelfAttention(50, 4)
    built = []

    def factory(i, o):
        built.append((i, o))
        return torch.nn.Linear(i, o, bias=False)

    mod = BertSelfAttention(48, 4, 0.0, linear=factory, layer_id=5)
    assert built == [(48, 48)] * 3 and list(mod.state_dict()) == ["query.weight", "key.weight", "value.weight"]


def test_module_forward_and_the_weights_hook():
    torch.manual_seed(0)
    mod = BertSelfAttention(24, 3, 0.1, layer_id=7).eval()
    x = torch.randn(2, 6, 24)
    mask = R.padding_mask([6, 2], 6)
    ctx, sc = mod(x, mask)
    want = HF.self_attention_composed(mod.query(x), mod.key(x), mod.value(x), mask, 3)
    assert torch.equal(ctx, want[0]) and torch.equal(sc, want[1]) and sc.shape == (2, 3, 6, 6)
    seen = []

    class W:
        def qkv_transform(self, hidden_states, layer_id):
            seen.append(layer_id)
            return hidden_states * 2, hidden_states + 1, hidden_states - 1

    ctx, sc = mod(x, mask, output_att=True, weights=W())
    want = HF.self_attention_composed(x * 2, x + 1, x - 1, mask, 3)
    assert seen == [7] and torch.equal(ctx, want[0]) and torch.equal(sc, want[1])


def test_routing_rule():
    ok = dict(is_cuda=True, dtype=torch.float32, B=2, H=12, S=128, d=64, grad=True, mask_shape=(2, 1, 1, 128))
    assert HF.attention_launch_refusal(**ok) is None
    assert HF.attention_launch_refusal(**dict(ok, mask_shape=None)) is None
    assert HF.attention_launch_refusal(**dict(ok, dtype=torch.bfloat16)) is None
    assert HF.attention_launch_refusal(**dict(ok, dtype=torch.float16, grad=False)) is None
    assert "mask of shape" in HF.attention_launch_refusal(**dict(ok, mask_shape=(2, 1, 128, 128)))
    assert "mask of shape" in HF.attention_launch_refusal(**dict(ok, mask_shape=(2, 12, 128, 128)))
    assert "float16 with gradients" in HF.attention_launch_refusal(**dict(ok, dtype=torch.float16))
    assert "requires grad" in HF.attention_launch_refusal(**dict(ok, mask_foreign=True))
    assert "S = 513" in HF.attention_launch_refusal(**dict(ok, S=513, mask_shape=None))
    assert "d = 65" in HF.attention_launch_refusal(**dict(ok, d=65))
    assert "float64" in HF.attention_launch_refusal(**dict(ok, dtype=torch.float64))
    assert "HIP device" in HF.attention_launch_refusal(**dict(ok, is_cuda=False))
    assert isinstance(ops.attn_pays(8, 12, 128, 64, torch.float32, True), bool)
    # a 4-D mask of another shape and float16 under grad reach the composed route (here on the CPU, where it runs)
    q = torch.randn(1, 4, 8, requires_grad=True)
    full = torch.zeros(1, 1, 4, 4)
    a = HF.self_attention(q, q, q, full, 2)
    b = HF.self_attention_composed(q, q, q, full, 2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_dropin_import_line():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from bert_layers import BertSelfAttention; import tadmm; "
            "assert BertSelfAttention is tadmm.BertSelfAttention")
    subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "dnn-compression-tensor-admm_amd", "dropin")], check=True)
