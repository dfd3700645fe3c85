"""The routing of the seven `route=` functions of tadmm/functional.py and the words of their refusals (no GPU).

REFUSALS pins, for each `*_launch_refusal` function, the exact string (or None) of every reason it can give, in the
order in which it tests them, and then cases in which two reasons apply and the earlier one must win; a table entry is
(keyword arguments laid over the table's base call, expected).  The seven routing blocks and the five norm families'
refusals are copies of one another, and these tables are what a fold of them has to keep.  The second half drives the
routing of the seven public functions on CPU tensors at the smallest shapes that reach every branch: an unknown route,
`route="launch"` on what the launch refuses, `route=None` against `route="composed"` bit for bit, and the composed
function, the refusal and the `ops.*_pays` rule looked up at call time."""
import pytest
import torch

from tadmm import ops
from tadmm import functional as HF
from tadmm._cabi import TadmmError

REFUSALS = [
    ("batch_norm_act_launch_refusal",
     dict(is_cuda=True, dtype=torch.float32, shape=(2, 4, 3, 3), grad=True, training=True), [
        (dict(), None),
        (dict(dtype=torch.bfloat16), None),
        (dict(dtype=torch.float16, grad=False), None),
        (dict(grad=False, training=False), None),
        (dict(is_cuda=False), 'operands that are not on a HIP device'),
        (dict(dtype=torch.float64), 'torch.float64 operands'),
        (dict(dtype=torch.float16), 'float16 with gradients'),
        (dict(training=False), 'eval mode with gradients'),
        (dict(contiguous=False), 'an x that is not NCHW contiguous'),
        (dict(shape=(2, 0, 3, 3)), 'shape = (2, 0, 3, 3)'),
        (dict(shape=(2 ** 20, 1, 2 ** 12, 1)), 'shape = (1048576, 1, 4096, 1)'),
        (dict(shape=(1, 4, 1, 1)), 'one value per channel in training'),
        (dict(affine=False), 'affine=False'),
        (dict(tracked=False), 'track_running_stats=False'),
        (dict(param_dtypes=(torch.float32, torch.bfloat16)), 'parameters or running statistics that are not float32'),
        (dict(momentum_given=False), 'momentum=None'),
        (dict(foreign=True), 'a residual, parameter or buffer of another type or on another device'),
        (dict(is_cuda=False, dtype=torch.float64), 'operands that are not on a HIP device'),
        (dict(contiguous=False, affine=False), 'an x that is not NCHW contiguous'),
        (dict(momentum_given=False, foreign=True), 'momentum=None'),
    ]),
    ("depthwise_bn_relu6_launch_refusal",
     dict(is_cuda=True, dtype=torch.float32, shape=(2, 4, 3, 3), stride=1, grad=True, training=True), [
        (dict(), None),
        (dict(stride=(2, 2), dtype=torch.bfloat16), None),
        (dict(dtype=torch.float16, grad=False), None),
        (dict(is_cuda=False), 'operands that are not on a HIP device'),
        (dict(dtype=torch.float64), 'torch.float64 operands'),
        (dict(dtype=torch.float16), 'float16 with gradients'),
        (dict(training=False), 'eval mode with gradients'),
        (dict(contiguous=False), 'an x that is not NCHW contiguous'),
        (dict(kernel=(5, 5)), 'kernel (5, 5), padding (1, 1), dilation (1, 1)'),
        (dict(padding=0), 'kernel (3, 3), padding (0, 0), dilation (1, 1)'),
        (dict(dilation=2), 'kernel (3, 3), padding (1, 1), dilation (2, 2)'),
        (dict(stride=3), 'stride (3, 3)'),
        (dict(stride=(1, 2)), 'stride (1, 2)'),
        (dict(shape=(2, 4, 0, 3)), 'shape = (2, 4, 0, 3)'),
        (dict(shape=(1, 1, 3, 10 ** 5)), 'shape = (1, 1, 3, 100000)'),
        (dict(shape=(1, 4, 2, 2), stride=2), 'one output value per channel in training'),
        (dict(affine=False), 'affine=False'),
        (dict(tracked=False), 'track_running_stats=False'),
        (dict(param_dtypes=(torch.float32, torch.float64)), 'parameters or running statistics that are not float32'),
        (dict(momentum_given=False), 'momentum=None'),
        (dict(foreign=True), 'a parameter or buffer of another type or on another device'),
        (dict(dtype=torch.float16, training=False), 'float16 with gradients'),
        (dict(stride=3, tracked=False), 'stride (3, 3)'),
    ]),
    ("dense_batch_norm_act_launch_refusal",
     dict(is_cuda=True, dtypes=[torch.float32, torch.float32], shapes=[(2, 3, 3, 3), (2, 1, 3, 3)], grad=True,
          training=True), [
        (dict(), None),
        (dict(dtypes=[torch.float16, torch.float16], grad=False), None),
        (dict(is_cuda=False), 'operands that are not on a HIP device'),
        (dict(dtypes=[torch.float32, torch.bfloat16]), 'feature tensors of mixed types'),
        (dict(dtypes=[torch.float64, torch.float64]), 'torch.float64 operands'),
        (dict(dtypes=[torch.float16, torch.float16]), 'float16 with gradients'),
        (dict(training=False), 'eval mode with gradients'),
        (dict(contiguous=False), 'a feature tensor that is not NCHW contiguous'),
        (dict(shapes=[(2, 3, 3, 3), (2, 1, 4, 3)]), 'feature tensors of mixed shapes'),
        (dict(shapes=[(2, 3, 3, 3), (2, 3, 3)]), 'feature tensors of mixed shapes'),
        (dict(shapes=[(2, 3, 3, 3), (2, 0, 3, 3)]), 'feature tensors of mixed shapes'),
        (dict(dtypes=[torch.float32] * 129, shapes=[(2, 1, 3, 3)] * 129), '129 feature tensors (at most 128)'),
        (dict(shapes=[(2 ** 20, 3, 2 ** 12, 1), (2 ** 20, 1, 2 ** 12, 1)]), 'shape = (1048576, 4, 4096, 1)'),
        (dict(shapes=[(1, 3, 1, 1), (1, 1, 1, 1)]), 'one value per channel in training'),
        (dict(affine=False), 'affine=False'),
        (dict(tracked=False), 'track_running_stats=False'),
        (dict(param_dtypes=(torch.bfloat16,)), 'parameters or running statistics that are not float32'),
        (dict(momentum_given=False), 'momentum=None'),
        (dict(foreign=True), 'a feature tensor, parameter or buffer on another device'),
        (dict(dtypes=[torch.float32, torch.float64], training=False), 'feature tensors of mixed types'),
        (dict(shapes=[(1, 3, 1, 1), (1, 1, 1, 1)], foreign=True), 'one value per channel in training'),
    ]),
    ("layer_norm_launch_refusal",
     dict(is_cuda=True, dtype=torch.float32, rows=6, hidden=8, grad=True, param_dtype=torch.float32), [
        (dict(), None),
        (dict(dtype=torch.bfloat16, param_dtype=torch.bfloat16), None),
        (dict(dtype=torch.float16, grad=False), None),
        (dict(param_dtype=None), None),
        (dict(is_cuda=False), 'operands that are not on a HIP device'),
        (dict(dtype=torch.float64), 'torch.float64 operands'),
        (dict(dtype=torch.float16), 'float16 with gradients'),
        (dict(rows=0), 'rows = 0, hidden = 8'),
        (dict(hidden=0), 'rows = 6, hidden = 0'),
        (dict(hidden=10 ** 6), 'rows = 6, hidden = 1000000'),
        (dict(param_dtype=torch.bfloat16), 'torch.bfloat16 parameters beside torch.float32 operands'),
        (dict(foreign=True), 'a residual, parameter or keep tensor of another type or on another device'),
        (dict(dtype=torch.float64, rows=0), 'torch.float64 operands'),
        (dict(param_dtype=torch.float64, foreign=True), 'torch.float64 parameters beside torch.float32 operands'),
    ]),
    ("add_layer_norm_launch_refusal",
     dict(is_cuda=True, dtype=torch.float32, rows=6, hidden=8, grad=True, param_dtype=torch.float32), [
        (dict(), None),
        (dict(dtype=torch.bfloat16, param_dtype=torch.bfloat16), None),
        (dict(dtype=torch.float16, grad=False), None),
        (dict(param_dtype=None), None),
        (dict(is_cuda=False), 'operands that are not on a HIP device'),
        (dict(dtype=torch.float64), 'torch.float64 operands'),
        (dict(dtype=torch.float16), 'float16 with gradients'),
        (dict(rows=0), 'rows = 0, hidden = 8'),
        (dict(hidden=0), 'rows = 6, hidden = 0'),
        (dict(hidden=10 ** 6), 'rows = 6, hidden = 1000000'),
        (dict(param_dtype=torch.bfloat16), 'torch.bfloat16 parameters beside torch.float32 operands'),
        (dict(foreign=True), 'a branch, parameter or keep tensor of another type or on another device'),
        (dict(dtype=torch.float64, rows=0), 'torch.float64 operands'),
        (dict(param_dtype=torch.float64, foreign=True), 'torch.float64 parameters beside torch.float32 operands'),
    ]),
    ("attention_launch_refusal",
     dict(is_cuda=True, dtype=torch.float32, B=1, H=2, S=4, d=8, grad=True, mask_shape=(1, 1, 1, 4)), [
        (dict(), None),
        (dict(mask_shape=None), None),
        (dict(dtype=torch.float16, grad=False), None),
        (dict(is_cuda=False), 'operands that are not on a HIP device'),
        (dict(dtype=torch.float64), 'torch.float64 operands'),
        (dict(dtype=torch.float16), 'float16 with gradients'),
        (dict(B=0), 'S = 4, d = 8'),
        (dict(S=513, mask_shape=None), 'S = 513, d = 8'),
        (dict(d=65), 'S = 4, d = 65'),
        (dict(mask_shape=(1, 2, 4, 4)), 'a mask of shape (1, 2, 4, 4)'),
        (dict(mask_foreign=True), 'a mask that requires grad or lives on another device'),
        (dict(is_cuda=False, S=513), 'operands that are not on a HIP device'),
        (dict(mask_shape=(1, 1, 4, 4), mask_foreign=True), 'a mask of shape (1, 1, 4, 4)'),
    ]),
    ("layer_mse_launch_refusal", dict(is_cuda=True, dtypes=[torch.float32, torch.float32], npairs=1), [
        (dict(), None),
        (dict(dtypes=[torch.bfloat16] * 4, npairs=2), None),
        (dict(is_cuda=False), 'operands that are not on a HIP device'),
        (dict(dtypes=[torch.float64, torch.float64]), 'torch.float64 operands'),
        (dict(dtypes=[torch.float32, torch.bfloat16]), 'mixed element types in one call (torch.float32, torch.bfloat16)'),
        (dict(npairs=10 ** 4), '10000 pairs (one call takes 32)'),
        (dict(teacher_foreign=True), 'a teacher on another device than its student'),
        (dict(dtypes=[torch.float32, torch.float64], npairs=10 ** 4), 'torch.float64 operands'),
        (dict(npairs=10 ** 4, teacher_foreign=True), '10000 pairs (one call takes 32)'),
    ]),
]


@pytest.mark.parametrize("name, base, cases", REFUSALS, ids=[t[0] for t in REFUSALS])
def test_refusal_strings_and_their_order(name, base, cases):
    fn = getattr(HF, name)
    for over, want in cases:
        got = fn(**dict(base, **over))
        assert got == want and type(got) is type(want), (name, over, got)
    assert fn(**base) is None


def _tensors(*shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes]


def _bn_state(c):
    """weight, bias and fresh running_mean, running_var, num_batches_tracked of a c-channel BatchNorm2d."""
    w, b, rm = _tensors((c,), (c,), (c,), seed=1)
    return w, b, rm, torch.rand(c, generator=torch.Generator().manual_seed(2)) + 0.5, torch.tensor(3)


def _attention(route):
    q, k, v = _tensors((1, 4, 16), (1, 4, 16), (1, 4, 16))
    mask = torch.tensor([0.0, 0.0, -1e4, 0.0]).view(1, 1, 1, 4)
    return HF.self_attention(q, k, v, mask, 2, route=route)


def _layer_losses(route):
    sa, ta, sr, tr = _tensors((1, 2, 4, 4), (1, 2, 4, 4), (1, 4, 16), (1, 4, 16))
    return HF.intermediate_distillation_loss([sa], [ta], [sr], [tr], route=route)


def _layer_norm(route):
    x, res, w, b = _tensors((2, 3, 8), (2, 3, 8), (8,), (8,))
    return HF.residual_layer_norm(x, res, w, b, route=route)


def _add_layer_norm(route):
    x, branch, w, b = _tensors((2, 3, 8), (2, 3, 8), (8,), (8,))
    return HF.add_layer_norm(x, branch, w, b, route=route)


def _batch_norm_act(route):
    x, residual = _tensors((2, 4, 3, 3), (2, 2, 3, 3))
    w, b, rm, rv, nbt = _bn_state(4)
    y = HF.batch_norm_act(x, rm, rv, w, b, residual, res_channel_offset=1, training=True, num_batches_tracked=nbt,
                          route=route)
    return y, rm, rv, nbt


def _dense_batch_norm_act(route):
    w, b, rm, rv, nbt = _bn_state(4)
    y = HF.dense_batch_norm_act(_tensors((2, 3, 3, 3), (2, 1, 3, 3)), rm, rv, w, b, training=True,
                                num_batches_tracked=nbt, route=route)
    return y, rm, rv, nbt


def _depthwise(route):
    x, cw = _tensors((2, 4, 3, 3), (4, 1, 3, 3))
    w, b, rm, rv, nbt = _bn_state(4)
    y = HF.depthwise_bn_relu6(x, cw, rm, rv, w, b, stride=1, training=True, num_batches_tracked=nbt, route=route)
    return y, rm, rv, nbt


ROUTED = [("self_attention", _attention), ("intermediate_distillation_loss", _layer_losses),
          ("residual_layer_norm", _layer_norm), ("add_layer_norm", _add_layer_norm),
          ("batch_norm_act", _batch_norm_act), ("dense_batch_norm_act", _dense_batch_norm_act),
          ("depthwise_bn_relu6", _depthwise)]
routed = pytest.mark.parametrize("who, call", ROUTED, ids=[r[0] for r in ROUTED])


@routed
def test_unknown_route_is_a_value_error(who, call):
    with pytest.raises(ValueError) as e:
        call("fast")
    assert str(e.value) == f"{who}: route is None, 'launch' or 'composed' (got 'fast')"
    with pytest.raises(ValueError) as e:
        call("native")
    assert str(e.value) == f"{who}: route is None, 'launch' or 'composed' (got 'native')"


@routed
def test_launch_route_refuses_cpu_tensors(who, call):
    with pytest.raises(TadmmError, match=f"{who}: route='launch' cannot take operands that are not on a HIP device"):
        call("launch")


@routed
def test_no_route_and_composed_route_agree_bit_for_bit(who, call):
    a, b = call(None), call("composed")
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert len(a) == len(b) and len(a) >= 1
    for s, t in zip(a, b):
        assert s.dtype == t.dtype and s.shape == t.shape and torch.equal(s, t), who


LOOKED_UP = {"self_attention": ("attention_launch_refusal", "attn_pays"),
             "intermediate_distillation_loss": ("layer_mse_launch_refusal", "layer_mse_pays"),
             "residual_layer_norm": ("layer_norm_launch_refusal", "bertnorm_pays"),
             "add_layer_norm": ("add_layer_norm_launch_refusal", "prenorm_pays"),
             "batch_norm_act": ("batch_norm_act_launch_refusal", "bnact_pays"),
             "dense_batch_norm_act": ("dense_batch_norm_act_launch_refusal", "densebn_pays"),
             "depthwise_bn_relu6": ("depthwise_bn_relu6_launch_refusal", "dwbn_pays")}


@routed
def test_composed_function_is_looked_up_at_call_time(who, call, monkeypatch):
    calls = []
    real = getattr(HF, who + "_composed")
    monkeypatch.setattr(HF, who + "_composed", lambda *a, **k: calls.append(who) or real(*a, **k))
    for n, route in enumerate((None, "composed"), 1):
        call(route)
        assert calls == [who] * n


@routed
def test_pays_rule_is_looked_up_at_call_time_and_asked_only_without_a_route(who, call, monkeypatch):
    """With the refusal patched to take the call, route=None must ask the patched rule, whose False sends the call to the
    composed route; route="composed" asks neither."""
    asked, composed = [], []
    refusal, pays = LOOKED_UP[who]
    real = getattr(HF, who + "_composed")
    monkeypatch.setattr(HF, who + "_composed", lambda *a, **k: composed.append(who) or real(*a, **k))
    monkeypatch.setattr(HF, refusal, lambda *a, **k: asked.append("refusal"))          # None: the launch takes it
    monkeypatch.setattr(ops, pays, lambda *a, **k: bool(asked.append("pays")))         # False: it does not pay
    call(None)
    assert asked[-1] == "pays" and asked.count("pays") == 1 and "refusal" in asked and composed == [who]
    n = len(asked)
    call("composed")
    assert asked.count("pays") == 1 and composed == [who, who]
    assert len(asked) == n or who in ("self_attention", "intermediate_distillation_loss", "residual_layer_norm",
                                      "add_layer_norm")             # these compute the refusal on every route
