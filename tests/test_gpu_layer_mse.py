"""TinyBERT's layer losses on the device (csrc/layermse.hip through tadmm.losses / tadmm.functional / tadmm.ops) against
the reference's recorded runs (G20) and the float64 restatement of tests/_layer_mse_ref.py evaluated on the device.

Bars.  With e_f the launch's error and e_c that of `intermediate_distillation_loss_composed` (torch operations in
float32), both against float64: each loss needs e_f <= 2 max(e_c, 2^-23) (relative); float32 gradients the same in the max
norm with the floor 2^-23 max|g64|; gradients delivered in a 16-bit type are within one unit in the last place of that
type at the reference element's magnitude.  Both sides are float32 element arithmetic and differ in summation order,
hence the factor two.  All sizes come from `ops.layer_mse_geometry()`.  The tests print their figures (run with -s);
DESIGN.md section 22 quotes the worst.
"""
import copy

import pytest
import torch

import _layer_mse_ref as R
from tadmm import _cabi
from tadmm import functional as HF
from tadmm import losses as L
from tadmm import ops
from tadmm.bert_layers import BertEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2.0 ** -23
LAUNCH = lambda *a, **q: HF.intermediate_distillation_loss(*a, route="launch", **q)
COMPOSED = HF.intermediate_distillation_loss_composed


def _dev(ts):
    return [t.to(DEV) for t in ts]


def _leaves(ts):
    """Leaves that share the memory (and so the address and the strides) of the given tensors; nothing writes to them."""
    return [t.detach().requires_grad_(True) for t in ts]


def _run(fn, sa, ta, sr, tr, gouts=None, **kw):
    """(att, rep, grads of the attention students + grads of the hidden students) of one differentiable route."""
    la, lr = _leaves(sa), _leaves(sr)
    att, rep = fn(la, ta, lr, tr, **kw)
    for v in (att, rep):
        assert v.dtype == torch.float32 and v.dim() == 0
    outs = [v for v, ss in ((att, la), (rep, lr)) if ss]
    gouts = [torch.ones((), device=DEV)] * 2 if gouts is None else gouts
    torch.autograd.backward(outs, [g for g, ss in zip(gouts, (la, lr)) if ss])
    return att.detach(), rep.detach(), [x.grad for x in la + lr]


def _check_loss(tag, what, lf, lc, l64):
    scale = abs(float(l64))
    e_f = abs(float(lf) - float(l64)) / (scale or 1.0)
    e_c = abs(float(lc) - float(l64)) / (scale or 1.0)
    print(f"{tag}: {what} e_f {e_f:.2e} e_c {e_c:.2e}")
    assert e_f <= 2 * max(e_c, FLOOR if scale else 0.0), (tag, what, e_f, e_c)


def _check_grad(tag, i, gf, gc, g64, dtype):
    assert gf.dtype == dtype and gf.shape == g64.shape
    assert bool(torch.isfinite(gf).all()), (tag, i)
    err = (gf.to(torch.float64) - g64).abs()
    if dtype == torch.float32:
        top = float(g64.abs().max())
        e_f, e_c = float(err.max()), float((gc.to(torch.float64) - g64).abs().max())
        print(f"{tag}: grad {i} e_f {e_f / max(top, 1e-300):.2e} e_c {e_c / max(top, 1e-300):.2e} (of max |g|)")
        assert e_f <= 2 * max(e_c, FLOOR * top), (tag, i, e_f, e_c, top)
    else:
        ulps = float((err / R.ulp(g64, dtype)).max())
        print(f"{tag}: grad {i} worst {ulps:.3f} ulp of {dtype}")
        assert ulps <= 1.0, (tag, i, ulps)


def _compare(tag, sa, ta, sr, tr, gouts=None, scale=(1.0, 1.0), **kw):
    """Both routes against float64 under the bars of the module docstring; returns the launch's results."""
    a64, r64, _, g64 = R.restate(sa, ta, sr, tr, **dict(dict(threshold=-100.0), **kw))
    af, rf, gf = _run(LAUNCH, sa, ta, sr, tr, gouts, **kw)
    ac, rc, gc = _run(COMPOSED, sa, ta, sr, tr, gouts, **kw)
    if sa:
        _check_loss(tag, "att", af, ac, a64)
    if sr:
        _check_loss(tag, "rep", rf, rc, r64)
    for i, (a, b, c) in enumerate(zip(gf, gc, g64)):
        _check_grad(tag, i, a, b, c * (scale[0] if i < len(sa) else scale[1]), (sa + sr)[i].dtype)
    return af, rf, gf


# ------------------------------------------------------------------------------------------------------- 1. golden
def test_recorded_reference_on_both_routes(golden_dir):
    """The reference's float32 CPU losses and gradients.  Bar: the restatement sits within 1e-6 of the record
    (test_layer_mse_host_cpu), either route within 2^-22 of the restatement: 2e-6 relative, 2e-6 of max|g|."""
    for meta in R.golden_index(golden_dir):
        d = {k: v.to(DEV) for k, v in R.recorded(golden_dir, meta["name"]).items()}
        for route in ("launch", "composed"):
            crit = L.TinyBertLayerLoss()
            crit.route = route
            s_att, s_rep = _leaves([d["s_att"], d["s_rep"]])
            att, rep = crit(s_att, d["t_att"], s_rep, d["t_rep"])
            (att + rep).backward()
            for got, want in ((att, d["att_loss"][0]), (rep, d["rep_loss"][0])):
                assert abs(float(got.detach()) - float(want)) <= 2e-6 * abs(float(want)), (meta, route)
            for got, want in ((s_att.grad, d["grad_att"]), (s_rep.grad, d["grad_rep"])):
                assert (got - want).abs().max() <= 2e-6 * max(float(want.abs().max()), 1e-30), (meta, route)
        sa, ta, sr, tr = [d["s_att"]], [d["t_att"]], [d["s_rep"]], [d["t_rep"]]
        _compare(meta["name"], sa, ta, sr, tr)


# --------------------------------------------------------------------------------------------------------- 2. bars
@pytest.mark.parametrize("dtype", list(R.DTYPES))
@pytest.mark.parametrize("reduction", ["batch_sum", "mean"])
def test_types_reductions_and_weights(dtype, reduction):
    sa, ta = zip(R.att_pair(3, 2, 9, 1, dtype), R.att_pair(2, 12, 16, 2, dtype))
    sr, tr = zip(R.rep_pair((3, 9, 7), 3, dtype), R.rep_pair((2, 16, 24), 4, dtype), R.rep_pair((5, 3), 5, dtype))
    sa, ta, sr, tr = _dev(sa), _dev(ta), _dev(sr), _dev(tr)
    _compare(f"{dtype}-{reduction}", sa, ta, sr, tr, reduction=reduction)
    _compare(f"{dtype}-{reduction}-w", sa, ta, sr, tr, reduction=reduction, att_weights=[0.5, 2.0], rep_weights=[1.0, 0.25, 3.0])


# ------------------------------------------------------------------------------------------------------- 3. shapes
_GEOM = None


def _geom():
    global _GEOM
    _GEOM = _GEOM or ops.layer_mse_geometry()
    return _GEOM


@pytest.mark.parametrize("tag", ["one", "chunk-1", "chunk", "chunk+1", "odd-tail", "one-between", "pairs-9", "pairs-32",
                                 "second-trip"])
def test_shapes_that_can_break_the_decomposition(tag):
    chunk, blocks = _geom()
    table = dict(R.shape_cases(chunk, blocks))
    assert set(table) >= {tag}
    sa, ta = R.case_pairs(table[tag], 100)
    sa, ta = _dev(sa), _dev(ta)
    sr, tr = ([], []) if tag in ("pairs-32", "second-trip") else zip(*[R.rep_pair((2, 5, 3), 7), R.rep_pair((chunk + 5,), 8)])
    sr, tr = _dev(sr), _dev(tr)
    _compare(tag, sa, ta, sr, tr)
    if tag == "pairs-9":
        assert len(sa) == 9
    if tag == "pairs-32":
        assert len(sa) == ops.LAYER_MSE_MAX_PAIRS
    if tag == "second-trip":
        assert sa[0].numel() > blocks * chunk + chunk


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_sixteen_bit_chunks(dtype):
    chunk, _ = _geom()
    sa, ta = R.case_pairs([chunk - 1, 2 * chunk + 9, 1], 200, dtype)
    sr, tr = R.rep_pair((3, chunk // 2 + 1), 9, dtype)
    _compare(f"chunks-{dtype}", _dev(sa), _dev(ta), _dev([sr]), _dev([tr]))


def test_one_side_only():
    chunk, _ = _geom()
    sa, ta = R.case_pairs([(3, 2, 37, 37), chunk + 1], 300)
    sr, tr = zip(R.rep_pair((3, 9, 7), 10), R.rep_pair((2, chunk), 11))
    sa, ta, sr, tr = _dev(sa), _dev(ta), _dev(sr), _dev(tr)
    af, rf, _ = _compare("att-only", sa, ta, [], [])
    assert float(rf) == 0.0
    af2, rf2, _ = _compare("rep-only", [], [], sr, tr)
    assert float(af2) == 0.0
    for fn in (LAUNCH, COMPOSED):
        att, rep = fn(_leaves(sa), ta, [], [])
        assert att.grad_fn is not None and rep.grad_fn is None and rep.dtype == torch.float32
        att, rep = fn([], [], _leaves(sr), tr)
        assert rep.grad_fn is not None and att.grad_fn is None and att.dtype == torch.float32


# ---------------------------------------------------------------------------------------------------- 4. addresses
@pytest.mark.parametrize("dtype", list(R.DTYPES))
@pytest.mark.parametrize("offs", [(1, 0), (0, 1), (1, 1), (1, 3), (2, 1)])
def test_views_off_the_sixteen_byte_grid(dtype, offs):
    chunk, _ = _geom()
    s, t = R.flat_pair(2 * chunk + 11, 400, dtype, batch=1)
    rs, rt = R.rep_pair((3, chunk // 3 + 2), 401, dtype)
    s, t, rs, rt = _dev([s, t, rs, rt])
    vs, vt = R.offset_view(s, offs[0]), R.offset_view(t, offs[1])
    vrs, vrt = R.offset_view(rs, offs[1]), R.offset_view(rt, offs[0])
    assert (vs.data_ptr() % 16 != 0) == (offs[0] != 0) and (vt.data_ptr() % 16 != 0) == (offs[1] != 0)
    af, rf, gf = _compare(f"offs-{dtype}-{offs}", [vs], [vt], [vrs], [vrt])
    a0, r0, g0 = _run(LAUNCH, [s], [t], [rs], [rt])
    # element loads give every lane other elements to sum: the gradients keep their bits, the sums their value
    assert all(torch.equal(a, b) for a, b in zip(gf, g0))
    assert abs(float(af) - float(a0)) <= FLOOR * float(a0) and abs(float(rf) - float(r0)) <= FLOOR * float(r0)


def test_misaligned_gradient_buffer():
    """ops.layer_mse with gradient buffers that start one float off the 16-byte grid: element stores, same bits."""
    chunk, _ = _geom()
    s, t = _dev(R.flat_pair(chunk + 7, 410))
    flat = torch.full((2 * s.numel() + 16,), 7.0, device=DEV)
    g0, g1 = flat[:s.numel()], flat[s.numel() + 6:2 * s.numel() + 6]
    assert g0.data_ptr() % 16 == 0 and g1.data_ptr() % 16 != 0
    loss, terms = ops.layer_mse([s, s], [t, t], [0.5, 0.5], ["att", "rep"], [True, True], -100.0, grads=[g0, g1])
    assert torch.equal(g0, g1) and float(terms[0]) == float(terms[1]) and float(loss[0]) == float(loss[1])
    assert float(flat[s.numel():s.numel() + 6].min()) == 7.0 and float(flat[2 * s.numel() + 6:].min()) == 7.0
    _, _, _, g64 = R.restate([s], [t], [], [], reduction="mean", att_weights=[0.5 * s.numel()])
    assert (g0.double() - g64[0].view(-1)).abs().max() <= 2 * FLOOR * float(g64[0].abs().max())


def test_transposed_student():
    s, t = _dev(R.att_pair(3, 2, 9, 420))
    rs, rt = _dev(R.rep_pair((7, 9, 3), 421))
    # leaves that ARE transposed views; and a transposed view of a contiguous leaf
    va = s.transpose(2, 3).contiguous().transpose(2, 3).detach().requires_grad_(True)
    vr = rs.permute(2, 1, 0).contiguous().permute(2, 1, 0).detach().requires_grad_(True)
    base = s.transpose(2, 3).contiguous().requires_grad_(True)
    assert not va.is_contiguous() and not vr.is_contiguous() and torch.equal(va, s) and torch.equal(base.transpose(2, 3), s)
    att, rep = LAUNCH([va, base.transpose(2, 3)], [t, t], vr, rt)
    (att + rep).backward()
    assert va.grad.shape == va.shape and va.grad.stride() == va.stride()
    assert vr.grad.shape == vr.shape and vr.grad.stride() == vr.stride()
    a64, r64, _, g64 = R.restate([s], [t], [rs], [rt])
    ac, rc, gc = _run(COMPOSED, [s], [t], [rs], [rt])
    _check_loss("transposed", "att", att.detach() / 2, ac, a64)
    _check_loss("transposed", "rep", rep.detach(), rc, r64)
    _check_grad("transposed", 0, va.grad, gc[0], g64[0], torch.float32)
    _check_grad("transposed", 0, base.grad.transpose(2, 3), gc[0], g64[0], torch.float32)
    _check_grad("transposed", 1, vr.grad, gc[1], g64[1], torch.float32)


# ---------------------------------------------------------------------------------------------------- 5. threshold
def test_threshold_edges():
    s, t = _dev(R.flat_pair(64, 430))
    up = torch.nextafter(torch.tensor(-100.0), torch.tensor(0.0)).item()
    s[0, :4] = torch.tensor([-100.0, up, float("-inf"), -100.0], device=DEV)
    t[0, :4] = torch.tensor([1.0, 2.0, 3.0, float("-inf")], device=DEV)
    t[0, 4], s[0, 4] = -100.0, 0.5
    af, _, gf = _compare("edges", [s], [t], [], [])
    g = gf[0][0]
    assert float(g[0]) == 0.0 and float(g[2]) == 0.0 and float(g[3]) == 0.0            # clamped: exactly zero
    assert float(g[1]) == pytest.approx(2 * (up - 2.0) / 64, rel=1e-6)                 # nextafter(-100, 0) is kept
    assert float(g[4]) == pytest.approx(2 * 0.5 / 64, rel=1e-6)                        # a teacher at -100 is zeroed
    assert bool(torch.isfinite(af))
    for dtype in ("bfloat16", "float16"):
        s16, t16 = s.to(R.DTYPES[dtype]), t.to(R.DTYPES[dtype])
        _compare(f"edges-{dtype}", [s16], [t16], [], [])


def test_nan_stays_in_its_group():
    s, t = _dev(R.att_pair(2, 2, 9, 431))
    rs, rt = _dev(R.rep_pair((2, 9, 5), 432))
    s[0, 0, 0, 0] = float("nan")
    for fn in (LAUNCH, COMPOSED):
        att, rep = fn(s, t, rs, rt)
        assert bool(torch.isnan(att)) and bool(torch.isfinite(rep))
    rs[1, 2, 3] = float("nan")
    s[0, 0, 0, 0] = 0.25
    for fn in (LAUNCH, COMPOSED):
        att, rep = fn(s, t, rs, rt)
        assert bool(torch.isfinite(att)) and bool(torch.isnan(rep))


def test_clamp_off_is_plain_mse():
    s, t = _dev(R.att_pair(2, 2, 9, 433))
    _compare("thr-none", [s], [t], [], [], threshold=None)
    att, _ = LAUNCH(s, t, [], [], threshold=None, reduction="mean")
    want = torch.nn.functional.mse_loss(s.double(), t.double())
    assert abs(float(att) - float(want)) <= 2 * FLOOR * float(want)
    loss, terms = ops.layer_mse([s], [t], [1.0 / s.numel()], 0, False, -100.0)
    assert abs(float(terms[0]) - float(want)) <= 1e-12 * float(want) and float(loss[1]) == 0.0
    _compare("thr-other", [s], [t], [], [], threshold=-0.5)


# ----------------------------------------------------------------------------------------------------- 6. autograd
def test_backward_of_a_mix_and_explicit_upstream():
    sa, ta = zip(*[_dev(R.att_pair(3, 2, 9, 440)), _dev(R.att_pair(2, 2, 5, 441))])
    sr, tr = zip(*[_dev(R.rep_pair((3, 9, 7), 442))])
    sa, ta, sr, tr = list(sa), list(ta), list(sr), list(tr)
    gouts = [torch.tensor(0.5, device=DEV), torch.tensor(1.0, device=DEV)]
    _compare("mix", sa, ta, sr, tr, gouts=gouts, scale=(0.5, 1.0))
    la, lr = _leaves(sa), _leaves(sr)
    att, rep = LAUNCH(la, ta, lr, tr)
    (0.5 * att + rep).backward()
    _, _, gf = _run(LAUNCH, sa, ta, sr, tr, gouts)
    assert all(torch.equal(x.grad, g) for x, g in zip(la + lr, gf))
    gouts = [torch.tensor(-3.0, device=DEV), torch.tensor(7.5, device=DEV)]
    _compare("upstream", sa, ta, sr, tr, gouts=gouts, scale=(-3.0, 7.5))


def test_unused_loss_leaves_its_students_without_gradient():
    sa, ta = _dev(R.att_pair(2, 2, 9, 443))
    sr, tr = _dev(R.rep_pair((2, 9, 5), 444))
    la, lr = _leaves([sa]), _leaves([sr])
    att, rep = LAUNCH(la, [ta], lr, [tr])
    att.backward()
    assert la[0].grad is not None and lr[0].grad is None
    la, lr = _leaves([sa]), _leaves([sr])
    att, rep = LAUNCH(la, [ta], lr, [tr])
    rep.backward()
    assert la[0].grad is None and lr[0].grad is not None
    # only some students require grad
    la = [sa.clone(), sa.clone().requires_grad_(True)]
    att, _ = LAUNCH(la, [ta, ta], [sr], [tr])
    att.backward()
    _, _, _, g64 = R.restate([sa], [ta], [], [])
    assert la[0].grad is None and (la[1].grad.double() - g64[0]).abs().max() <= 2 * FLOOR * float(g64[0].abs().max())


def test_shared_student_and_teacher_that_requires_grad():
    sa, ta = _dev(R.att_pair(2, 2, 9, 445))
    tb = _dev(R.att_pair(2, 2, 9, 446))[1]
    s = sa.clone().requires_grad_(True)
    t = ta.clone().requires_grad_(True)
    att, _ = LAUNCH([s, s], [t, tb], [], [])
    att.backward()
    _, _, _, g64 = R.restate([sa, sa], [ta, tb], [], [])
    want = g64[0] + g64[1]
    assert (s.grad.double() - want).abs().max() <= 3 * FLOOR * float(want.abs().max())
    assert t.grad is None


def test_scaled_float16_backward():
    """GradScaler's case: the saved gradients are float32 and are multiplied by 2^16 before they are rounded to float16.
    Unscaled, most elements of this gradient are below float16's normal range."""
    sa, ta = _dev(R.att_pair(8, 12, 64, 447, "float16"))
    sr, tr = _dev(R.rep_pair((8, 64, 768), 448, "float16"))
    gout = torch.tensor(65536.0, device=DEV)
    _, _, gf = _compare("scaled-f16", [sa], [ta], [sr], [tr], gouts=[gout, gout], scale=(65536.0, 65536.0))
    _, _, _, g64 = R.restate([sa], [ta], [sr], [tr])
    for got, g in zip(gf, g64):
        assert float((g.abs() < 2.0 ** -14).double().mean()) > 0.5              # the premise: unscaled, mostly subnormal
        assert bool(torch.isfinite(got).all())
        normal = (g.abs() * 65536.0) >= 2.0 ** -14
        assert bool((got[normal] != 0).all()) and int(normal.sum()) > g.numel() // 2


# ---------------------------------------------------------------------------------------------- 7. reproducibility
def test_two_calls_give_the_same_bits():
    chunk, blocks = _geom()
    sa, ta = R.case_pairs([(3, 2, 37, 37), 5 * chunk + 3, 1, blocks * chunk // 8 + 77], 450)
    sr, tr = zip(R.rep_pair((3, 37, 11), 451), R.rep_pair((2, chunk + 1), 452))
    sa, ta, sr, tr = _dev(sa), _dev(ta), _dev(sr), _dev(tr)
    a = _run(LAUNCH, sa, ta, sr, tr)
    b = _run(LAUNCH, sa, ta, sr, tr)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


# ------------------------------------------------------------------------------------------------- 8. route errors
def test_route_errors_and_the_rule():
    s, t = _dev(R.att_pair(2, 2, 5, 460))
    r, q = _dev(R.rep_pair((2, 5, 4), 461))
    refused = [
        (([s], [t], [r.bfloat16()], [q.bfloat16()]), "mixed"),
        (([s] * 20, [t] * 20, [r] * 13, [q] * 13), "33 pairs"),
        (([s.cpu()], [t.cpu()], [r.cpu()], [q.cpu()]), "HIP device"),
        (([s.double()], [t.double()], [], []), "float64"),
    ]
    for args, text in refused:
        with pytest.raises(_cabi.TadmmError, match=text):
            LAUNCH(*args)
        got = HF.intermediate_distillation_loss(*args)                  # route=None: the composed route
        want = COMPOSED(*args)
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.float32
        assert torch.equal(got[0], want[0].float()) and torch.equal(got[1], want[1].float())
    with pytest.raises(_cabi.TadmmError, match="HIP device"):
        LAUNCH([s], [t.cpu()], [], [])
    with pytest.raises(ValueError, match="teacher_atts"):
        LAUNCH([s], [t[:1]], [], [])


def test_rule_routes_by_layer_mse_pays(monkeypatch):
    s, t = _dev(R.att_pair(2, 2, 5, 462))
    for pays in (True, False):
        seen = []
        monkeypatch.setattr(ops, "layer_mse_pays", lambda n, p, dt, grad=False: seen.append((n, p, dt, grad)) or pays)
        att, _ = HF.intermediate_distillation_loss(s.clone().requires_grad_(True), t, [], [])
        assert seen == [(s.numel(), 1, torch.float32, True)]
        assert (att.grad_fn.name() == "_LayerMseFnBackward") == pays


# ------------------------------------------------------------------------------------------ 9. through the encoder
@pytest.mark.parametrize("attention_route", ["launch", "composed"])
def test_through_the_encoder(attention_route):
    """Student and teacher encoders; the loss on the last layer's scores and outputs; the gradients of two student
    weights under the launch against a float64 CPU copy of the same modules on the composed routes.  With the
    attention on "launch" the gradient of the scores reaches `tadmm_attn_bwd` as g_sc."""
    torch.manual_seed(470)
    B, S, hidden = 3, 9, 32
    make = lambda: BertEncoder(2, hidden, 2, 64, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                               linear=torch.nn.Linear)
    student, teacher = make(), make()
    x = torch.randn(B, S, hidden)
    mask = R.suffix_mask(B, S, [9, 6, 4])
    names = ["layer.1.attention.self.query.weight", "layer.0.output.dense.weight"]

    def grads(enc_s, enc_t, x, mask, loss_fn):
        enc_s.zero_grad()
        reps, atts = enc_s(x, mask)
        with torch.no_grad():
            treps, tatts = enc_t(x, mask)
        att, rep = loss_fn(atts[-1], tatts[-1], reps[-1], treps[-1])
        (att + rep).backward()
        params = dict(enc_s.named_parameters())
        return [params[n].grad.detach().clone() for n in names], atts[-1].detach()

    s64, t64 = copy.deepcopy(student).double(), copy.deepcopy(teacher).double()
    for enc in (s64, t64):
        for layer in enc.layer:
            layer.set_route("composed")
    g64, atts64 = grads(s64, t64, x.double(), mask.double(), COMPOSED)
    share, s_only, t_only = R.clamp_census(atts64, atts64)
    assert 0.1 <= share <= 0.6                                         # the clamp is at work in this case
    student, teacher = student.to(DEV), teacher.to(DEV)
    for enc in (student, teacher):
        for layer in enc.layer:
            layer.attention.self.route = attention_route
    xd, md = x.to(DEV), mask.to(DEV)
    gf, _ = grads(student, teacher, xd, md, LAUNCH)
    gc, _ = grads(student, teacher, xd, md, COMPOSED)
    for n, a, b, c in zip(names, gf, gc, g64):
        _check_grad(f"encoder-{attention_route}", n, a, b, c.to(DEV), torch.float32)
