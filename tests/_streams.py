"""Every native launch on a side stream behind a delayed producer (tests/test_gpu_streams.py).

Each entry of the C ABI takes a stream and every wrapper passes the caller's current one.  On PyTorch-ROCm the default
stream is the null stream and side streams do not block against it, so a launch, memset or copy that lands on stream
0, an internal event that is not joined around the caller's stream, or an upload ordered elsewhere passes every
default-stream test and corrupts results for a caller who overlaps work.  The harness makes that visible:

  1. reference: the real inputs x go into the staged buffers, the call (and its backward) runs on the default stream;
  2. decoy: a second seeded draw x' of the same kind goes into the buffers, the same call runs, and at least one result
     must differ bitwise from the reference -- a case that could not notice an early launch fails here.  x' stays;
  3. side stream: a device-side delay, then `buf.copy_(x)` for every buffer, then the call, then clones of the results,
     all enqueued on a side stream while the delay still runs.  The stream is one that the default stream was SEEN to
     overtake (`Delay._open_stream`): streams share a few hardware queues, and a null-stream launch that lands in the
     sleeping stream's queue would be ordered by accident;
  4. every result and every buffer the call updates in place must equal the reference bitwise.  A launch (or a part of
     it) that ran in front of the producer read the decoy: the mismatch report says whether the result equals the decoy's.

Safety rule (enforced by `run_case`, never by a case): every buffer a launch could read holds a valid decoy before the
delay starts, plans / batches / descriptor uploads are built and synchronised before it, random masks are explicit
buffers.  An early launch therefore computes a valid wrong answer; no missed ordering can fault.

The table (`CASES`) imports without a GPU: `inputs`, `build` and `call` only run on the device."""
import dataclasses
import importlib.util
import os
import time
from typing import Callable, Optional, Sequence

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
TARGET_DELAY_MS = 40.0
HOST_MARGIN = 4.0             # host time to the return of call() must stay below delay / HOST_MARGIN


# ------------------------------------------------------------------ the delay
class Delay:
    """A device-side delay of about `target_ms`, calibrated once with device events."""

    def __init__(self, device, target_ms: float = TARGET_DELAY_MS):
        self.device = device
        self.target_ms = target_ms
        self._sleep = getattr(torch.cuda, "_sleep", None)
        self._mats = None
        if self._sleep is None:                       # a chain of large matmuls instead
            self._mats = (torch.randn(4096, 4096, device=device), torch.empty(4096, 4096, device=device))
        self.units = 1_000_000 if self._sleep is not None else 4
        self.enqueue()                                # code objects loaded
        torch.cuda.synchronize(device)
        for _ in range(8):
            ms = self.measure()
            if 0.9 * target_ms <= ms <= 1.5 * target_ms:
                break
            self.units = max(1, int(self.units * 1.1 * target_ms / max(ms, 1e-3)))
        self.calibrated_ms = self.measure()
        self.rejected = 0
        self.side = self._open_stream()

    def _open_stream(self, tries: int = 16):
        """A side stream whose queued work the default stream does NOT wait behind.  Streams share the process's few
        hardware queues; work of the null stream that lands in the queue of a sleeping side stream runs behind the
        sleep, and a stray null-stream launch would then be ordered by accident and go unnoticed.  So the stream is
        chosen by experiment, and every case checks its own window again (`Report.window_open`)."""
        for _ in range(tries):
            s = torch.cuda.Stream(self.device)
            if window_open(s, self):
                return s
            self.rejected += 1
        raise AssertionError(f"none of {tries} side streams runs beside the default stream: the table would prove nothing")

    def enqueue(self):
        if self._sleep is not None:
            self._sleep(self.units)
        else:
            a, out = self._mats
            for _ in range(self.units):
                torch.mm(a, a, out=out)

    def measure(self) -> float:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.enqueue()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)


def window_open(side, delay) -> bool:
    """True when a copy on the default stream overtakes work queued behind a delay on `side`."""
    probe = torch.zeros(1, dtype=torch.int32, device=delay.device)
    torch.cuda.synchronize(delay.device)
    with torch.cuda.stream(side):
        delay.enqueue()
        probe.fill_(1)
    seen = probe.clone()                       # default stream, while the side stream sleeps
    torch.cuda.synchronize(delay.device)
    side.synchronize()
    return int(seen.item()) == 0


# ------------------------------------------------------------------ a case and its run
@dataclasses.dataclass
class Case:
    name: str
    entries: Sequence[str]              # the functions / methods of tadmm/ops.py with a `_stream(` call this case reaches
    inputs: Callable                    # (seed, device) -> {name: tensor}: everything the call reads or updates in place
    call: Callable                      # (bufs, ctx) -> sequence of tensors to compare
    build: Optional[Callable] = None    # (bufs) -> ctx: plans and batches over the buffers (their pointers stay)
    inplace: Sequence[str] = ()         # buffers the call updates in place: compared too
    wrt: Sequence[str] = ()             # buffers to differentiate: the case has a backward, through every result that
    #                                     requires grad, with seeded upstream gradients staged like the inputs
    host_sync: bool = False             # the entry waits for the device by design: no host-time bar
    check: Optional[Callable] = None    # (ctx) -> None: asserts on the reference run (the route that was taken)


def stream_callers_of(ops):
    """{code object: qualified name} of the module-level functions and the methods of tadmm/ops.py: what
    `reached_by` looks up the frames of a `_stream` call in."""
    import inspect
    names = {}
    for k, v in vars(ops).items():
        if inspect.isfunction(v) and v.__module__ == ops.__name__:
            names[v.__code__] = k
        elif inspect.isclass(v) and v.__module__ == ops.__name__:
            for mk, mv in vars(v).items():
                if inspect.isfunction(mv):
                    names[mv.__code__] = f"{k}.{mk}"
    return names


def recording_stream(ops, reached: set):
    """A stand-in for `ops._stream` that answers what the real one answers and notes which function or method of ops.py
    asked (the innermost named frame: a nested launcher counts for the function that holds it)."""
    import sys
    names, real = stream_callers_of(ops), ops._stream

    def _stream(device):
        f = sys._getframe(1)
        while f is not None:
            if f.f_code in names:
                reached.add(names[f.f_code])
                break
            f = f.f_back
        return real(device)

    return _stream


@dataclasses.dataclass
class Report:
    ok: bool
    equals_decoy: bool
    message: str
    host_ms: float
    delay_ms: float
    window_open: bool = True        # the default stream overtook this case's producer: an early launch was observable


def _seeded_like(outs, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.randn(o.shape, generator=g, dtype=torch.float32).to(o.dtype).to(o.device) for o in outs]


class _Run:
    """The staged buffers of one case and the three passes over them."""

    def __init__(self, case: Case, device):
        self.case, self.device = case, device
        self.x = {k: v.to(device).detach() for k, v in case.inputs(0, device).items()}
        self.xd = {k: v.to(device).detach() for k, v in case.inputs(1, device).items()}
        assert self.x.keys() == self.xd.keys()
        for k in self.x:
            assert self.x[k].shape == self.xd[k].shape and self.x[k].dtype == self.xd[k].dtype, k
        # the safety rule: the buffers are born holding the decoy, never uninitialised
        self.bufs = {k: v.clone() for k, v in self.xd.items()}
        for k in case.wrt:
            self.bufs[k].requires_grad_(True)
        self.ctx = None
        self.up = self.upd = self.gbufs = None
        self.probe = torch.zeros(1, dtype=torch.int32, device=device)

    def restore(self, src):
        with torch.no_grad():
            for k, b in self.bufs.items():
                b.copy_(src[k])

    def forward(self):
        with torch.set_grad_enabled(bool(self.case.wrt)):
            outs = list(self.case.call(self.bufs, self.ctx))
        res = [o.detach().clone() for o in outs]
        res += [self.bufs[k].detach().clone() for k in self.case.inplace]
        return outs, res

    def backward(self, outs, up):
        diff = [o for o in outs if o.requires_grad]
        with torch.no_grad():
            for b, u in zip(self.gbufs, up):
                b.copy_(u)
        grads = torch.autograd.grad(diff, [self.bufs[k] for k in self.case.wrt], self.gbufs)
        return [g.detach().clone() for g in grads]

    def default_pass(self, src, first: bool):
        self.restore(src)
        if first:
            self.ctx = self.case.build(self.bufs) if self.case.build is not None else None
        outs, res = self.forward()
        if self.case.wrt:
            if first:
                diff = [o for o in outs if o.requires_grad]
                assert diff, "a case with a backward needs a result that requires grad"
                self.up, self.upd = _seeded_like(diff, 0), _seeded_like(diff, 1)
                self.gbufs = [u.clone() for u in self.upd]
            res += self.backward(outs, self.up if src is self.x else self.upd)
        torch.cuda.synchronize(self.device)
        return res

    def side_pass(self, delay: Delay):
        side = delay.side
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        with torch.cuda.stream(side):
            e0.record()
            delay.enqueue()
            e1.record()
            self.probe.fill_(1)
            self.restore(self.x)
            with torch.cuda.stream(torch.cuda.default_stream(self.device)):
                seen = self.probe.clone()          # the witness: the default stream, while the delay still runs (taken
                #                                    in front of the call: an entry that waits for the device ends the delay)
            with torch.set_grad_enabled(bool(self.case.wrt)):
                outs = list(self.case.call(self.bufs, self.ctx))
            host_ms = (time.perf_counter() - t0) * 1e3
            res = [o.detach().clone() for o in outs]
            res += [self.bufs[k].detach().clone() for k in self.case.inplace]
            if self.case.wrt:
                delay.enqueue()
                res += self.backward(outs, self.up)
        side.synchronize()
        torch.cuda.synchronize(self.device)
        return res, host_ms, e0.elapsed_time(e1), int(seen.item()) == 0


def run_case(case: Case, device, delay: Delay) -> Report:
    """The four steps of the module docstring; the caller asserts on the report."""
    run = _Run(case, device)
    ref = run.default_pass(run.x, first=True)
    if case.check is not None:
        case.check(run.ctx)
    decoy = run.default_pass(run.xd, first=False)
    assert len(ref) == len(decoy) and len(ref) > 0
    assert any(not torch.equal(a, b) for a, b in zip(ref, decoy)), \
        f"{case.name}: the decoy inputs give the reference results bitwise: the case could not notice an early launch"
    got, host_ms, delay_ms, is_open = run.side_pass(delay)
    assert len(got) == len(ref)
    bad = [i for i, (a, b) in enumerate(zip(got, ref)) if not torch.equal(a, b)]
    equals_decoy = bool(bad) and any(torch.equal(got[i], decoy[i]) for i in bad)
    if not bad:
        msg = ""
    elif equals_decoy:
        msg = (f"{case.name}: results {bad} differ from the default-stream reference and equal the DECOY result: the "
               f"launch, or a part of it, ran in front of the producer on the caller's stream")
    else:
        msg = (f"{case.name}: results {bad} differ from the default-stream reference (and from the decoy result): the "
               f"outputs were read before the launch finished, or a part of the launch saw the decoy")
    del run
    torch.cuda.synchronize(device)
    return Report(not bad, equals_decoy, msg, host_ms, delay_ms, is_open)


# ------------------------------------------------------------------ the table
CASES = []


def case(name, entries, inputs, call, **kw):
    CASES.append(Case(name, tuple(entries), inputs, call, **kw))


def _gen(seed, salt=0):
    return torch.Generator().manual_seed(7919 * salt + 31 + seed)


def _randn(g, *shape, dtype=torch.float32, scale=1.0):
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype)


def _ops():
    from tadmm import ops
    return ops


def _load_bits():
    spec = importlib.util.spec_from_file_location("make_golden_filter_bits",
                                                  os.path.join(_HERE, "golden", "make_golden_filter_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- projection and linear algebra
PENALTY_SIZES = (7, 8193, 4099)          # three odd sizes of test_gpu_sweeps_unaligned.SIZES_HEAD; slot 1 has no gradient


def _penalty_inputs(seed, dev):
    rng = np.random.default_rng(5 + seed)
    out = {}
    for name, a in (("w", 1.0), ("z", 0.9), ("u", 0.3)):
        for i, k in enumerate(PENALTY_SIZES):
            out[f"{name}{i}"] = torch.from_numpy((a * rng.standard_normal(k)).astype(np.float32))
    out["loss"] = torch.tensor([2.5 + seed], dtype=torch.float64)
    return out


def _penalty_build(b):
    ops = _ops()
    dev = b["w0"].device
    n = len(PENALTY_SIZES)
    g = [None if i == 1 else torch.zeros(k, dtype=torch.float32, device=dev) for i, k in enumerate(PENALTY_SIZES)]
    ptrs = [b[f"{name}{i}"].data_ptr() for name in "wzu" for i in range(n)] + [0 if t is None else t.data_ptr() for t in g]
    h = ops.Handle.get(dev.index)
    ctx = dict(h=h, g=g, ptrs=torch.tensor(ptrs, dtype=torch.int64).to(dev),
               numel=torch.tensor(PENALTY_SIZES, dtype=torch.int64).to(dev),
               partial=torch.zeros(h.lib.tadmm_penalty_scratch_doubles(), dtype=torch.float64, device=dev))
    torch.cuda.synchronize(dev)
    return ctx


def _penalty_call(b, c):
    dev = b["w0"].device
    h = c["h"]
    h.check(h.lib.tadmm_penalty(h.ptr, len(PENALTY_SIZES), c["ptrs"].data_ptr(), c["numel"].data_ptr(),
                                int(sum(PENALTY_SIZES)), 1e-3, 0.37, b["loss"].data_ptr(), c["partial"].data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream))
    return [t for t in c["g"] if t is not None]


case("penalty", [], _penalty_inputs, _penalty_call, build=_penalty_build, inplace=("loss",))


def _jacobi_plan_inputs(seed, dev):
    """The four 16x16x3x3 TT layers of test_constant_weight_tensor_projects_like_the_oracle (two constant tensors)."""
    g = _gen(seed, 2)
    consts = ((0.37, -2.5e-3), (0.53, -4.0e-3))[seed]
    ws = [torch.full((16, 16, 3, 3), consts[0]), _randn(g, 16, 16, 3, 3, scale=0.1),
          torch.full((16, 16, 3, 3), consts[1]), _randn(g, 16, 16, 3, 3, scale=0.1)]
    out = {}
    for i, w in enumerate(ws):
        out[f"W{i}"] = w
        out[f"U{i}"] = _randn(g, 16, 16, 3, 3, scale=0.01)
        out[f"Z{i}"] = _randn(g, 16, 16, 3, 3, scale=0.1)
    return out


def _plan_layers(b, n, **extra):
    return [dict(W=b[f"W{i}"], U=b[f"U{i}"], Z=b[f"Z{i}"], **{k: (v[i] if isinstance(v, tuple) else v)
                                                             for k, v in extra.items()}) for i in range(n)]


def _jacobi_plan_build(b):
    from tadmm._cabi import KIND_TT_CONV
    plan = _ops().ProjectionPlan(_plan_layers(b, 4, kind=KIND_TT_CONV, tt_shapes=[4, 4, 9, 4, 4], ranks=[1, 4, 12, 12, 4, 1]))
    torch.cuda.synchronize()
    return plan


def _wuz(n):
    return tuple(f"{k}{i}" for k in "ZU" for i in range(n))


case("plan_jacobi", ["_LayerPlan.run"], _jacobi_plan_inputs, lambda b, plan: [plan.run(update_u=True)],
     build=_jacobi_plan_build, inplace=_wuz(4), host_sync=True)       # waits for the solver's convergence verdict


def _filter_plan_inputs(seed, dev):
    """The filter-eligible 1x1 layer of test_gpu_filter._layers."""
    rng = np.random.default_rng(3 + seed)
    shape = (1024, 256, 1, 1)
    w = (rng.standard_normal(shape) * np.sqrt(2.0 / 256)).astype(np.float32)
    return {"W0": torch.from_numpy(w), "U0": torch.from_numpy((0.01 * rng.standard_normal(shape)).astype(np.float32)),
            "Z0": torch.from_numpy((0.05 * rng.standard_normal(shape)).astype(np.float32))}


def _filter_plan_build(b):
    from tadmm._cabi import KIND_TT_CONV
    plan = _ops().ProjectionPlan(_plan_layers(b, 1, kind=KIND_TT_CONV, tt_shapes=[1024, 1, 256], ranks=[1, 75, 75, 1]))
    torch.cuda.synchronize()
    return plan


def _filter_plan_call(b, plan):
    resid = plan.run(update_u=True)
    sv = plan.singular_values(0, 0)
    return [resid, torch.from_numpy(sv)]


def _filter_plan_check(plan):
    st = plan.filter_stats()
    assert st["solves"] == 1 and st["fallbacks"] == 0, st


case("plan_filter", ["_LayerPlan.run", "ProjectionPlan.singular_values"], _filter_plan_inputs, _filter_plan_call,
     build=_filter_plan_build, inplace=_wuz(1), host_sync=True, check=_filter_plan_check)

TUCKER = (((24, 20, 3, 3), [20, 4]), ((12, 40), [5, 6]))      # of test_tucker_plan_odd_shapes_vs_oracle


def _tucker_inputs(seed, dev):
    rng = np.random.default_rng(12 + seed)
    out = {}
    for i, (s, _) in enumerate(TUCKER):
        out[f"W{i}"] = torch.from_numpy((rng.standard_normal(s) * 0.3).astype(np.float32))
        out[f"U{i}"] = torch.from_numpy((rng.standard_normal(s) * 0.01).astype(np.float32))
        out[f"Z{i}"] = torch.from_numpy((rng.standard_normal(s) * 0.3).astype(np.float32))
    return out


def _tucker_build(b):
    plan = _ops().TuckerPlan(_plan_layers(b, 2, ranks=tuple(r for _, r in TUCKER)))
    torch.cuda.synchronize()
    return plan


def _tucker_call(b, plan):
    out = [plan.run(update_u=True)]
    for i in range(2):
        out += list(plan.factors(i))
    it, err = plan.iterations()
    return out + [torch.tensor(it), torch.tensor(err, dtype=torch.float64)]


case("tucker_plan", ["_LayerPlan.run", "TuckerPlan.iterations"], _tucker_inputs, _tucker_call, build=_tucker_build,
     inplace=_wuz(2), host_sync=True)

# the stand-alone hooks (gram, eigh, dgemm, dgemm_tile, dgemm3, cholqr_) upload their descriptors and block maps from
# host vectors that die at return: they copy on the caller's stream and wait for it (csrc/abi_ops.hip)
case("gram", ["gram"], lambda s, dev: {"a": _randn(_gen(s, 3), 75, 1024)}, lambda b, c: [_ops().gram(b["a"])], host_sync=True)
case("gram_tall", ["gram"], lambda s, dev: {"a": _randn(_gen(s, 4), 33, 17)}, lambda b, c: [_ops().gram(b["a"])],
     host_sync=True)


def _psd(seed, n, salt):
    w = _randn(_gen(seed, salt), n, 2 * n, dtype=torch.float64)
    return {"G": (w @ w.t()) / (2 * n)}


def _eigh_call(b, c):
    ev, vec, sweeps = _ops().eigh(b["G"])
    return [ev, vec, torch.tensor([sweeps])]


def _eigh_partial_call(b, c):
    ev, vec, route = _ops().eigh_partial(b["G"], 12)
    return [ev, vec, torch.tensor([route])]


case("eigh_48", ["_eigh"], lambda s, dev: _psd(s, 48, 5), _eigh_call, host_sync=True)
case("eigh_160", ["_eigh"], lambda s, dev: _psd(s, 160, 6), _eigh_call, host_sync=True)
case("eigh_partial", ["_eigh"], lambda s, dev: _psd(s, 160, 7), _eigh_partial_call, host_sync=True)


def _dgemm_inputs(seed, dev):
    g = _gen(seed, 8)
    M, N, K = 96, 480, 224
    bt = _randn(g, N, K, dtype=torch.float64)
    return {"a": _randn(g, M, K, dtype=torch.float64), "bt": bt, "b": bt.t().contiguous()}


case("dgemm", ["dgemm"], _dgemm_inputs,
     lambda b, c: [_ops().dgemm(b["a"], b["bt"], True), _ops().dgemm(b["a"], b["b"], False)], host_sync=True)

TILE_SHAPES = ((96, 160), (64, 96))       # GROUPED of test_gpu_tile_map: one grouped launch, problem 0 gated off
TILE_COEF = (-0.5, -0.75, 0.375)


def _tile_inputs(seed, dev):
    bits = _load_bits()
    rng = np.random.default_rng(20240611 + seed)
    out = {}
    for i, (M, N) in enumerate(TILE_SHAPES):
        out[f"G{i}"] = torch.from_numpy(bits._grid(rng.standard_normal((N, N))))
        for k in range(3):
            out[f"ring{i}_{k}"] = torch.from_numpy(bits._grid(rng.standard_normal((M, N))))
        out[f"theta{i}"] = torch.from_numpy(bits._grid(rng.standard_normal(M)))
        out[f"rowpart{i}"] = torch.full(((N + 31) // 32, M), 7.0, dtype=torch.float64)
        out[f"gate{i}"] = torch.tensor([1 if i == 0 else 2], dtype=torch.int32)
    out["rot"] = torch.tensor([1], dtype=torch.int32)
    out["coef"] = torch.tensor(TILE_COEF, dtype=torch.float64)
    return out


def _tile_call(b, c):
    probs = []
    for i, (M, N) in enumerate(TILE_SHAPES):
        probs.append(dict(B=b[f"G{i}"], ring=[b[f"ring{i}_{k}"] for k in range(3)], rot=b["rot"], selA=1, selP=1, selQ=0,
                          selC=2, M=M, N=N, K=N, ldb=N, mode=1, coef=b["coef"], theta=b[f"theta{i}"],
                          rowpart=b[f"rowpart{i}"], gate=b[f"gate{i}"], gate_min=2))
    _ops().dgemm_tile(probs, 32, 32, device=b["rot"].device)
    return []


case("dgemm_tile", ["dgemm_tile"], _tile_inputs, _tile_call,
     inplace=tuple(f"ring{i}_{k}" for i in range(2) for k in range(3)) + ("rowpart0", "rowpart1"), host_sync=True)


def _dgemm3_inputs(seed, dev):
    g = _gen(seed, 9)
    M, N = 64, 288
    w = _randn(g, N, 2 * N, dtype=torch.float64)
    return {"a": _randn(g, M, N, dtype=torch.float64), "g": (w @ w.t()).contiguous()}


case("dgemm3", ["dgemm3"], _dgemm3_inputs, lambda b, c: [_ops().dgemm3(b["a"], b["g"])], host_sync=True)


def _cholqr_inputs(seed, dev):
    """A (96, 192) block of condition 1e2, built like test_cholqr_orthonormalises_and_keeps_the_span."""
    n, ncols, cond = 96, 192, 1e2
    rng = np.random.default_rng(n + ncols + seed)
    q1, _ = np.linalg.qr(rng.standard_normal((ncols, n)))
    q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.exp(np.linspace(0.0, -np.log(cond), n))
    return {"yt": torch.from_numpy(np.ascontiguousarray(((q1 * s) @ q2.T).T))}


case("cholqr", ["cholqr_"], _cholqr_inputs, lambda b, c: [torch.tensor([_ops().cholqr_(b["yt"])])], inplace=("yt",),
     host_sync=True)


# ---- GEMM and weight gradients
def _mm_inputs(seed, dev):
    g = _gen(seed, 10)
    M, N, K = 130, 33, 77
    return {"a": _randn(g, M, K), "b": _randn(g, K, N), "out": _randn(g, M, N), "bias_n": _randn(g, N)}


case("mm", ["mm"], _mm_inputs,
     lambda b, c: [_ops().mm(b["a"], b["b"], out=b["out"], alpha=0.5, beta=0.75, bias_n=b["bias_n"])], inplace=("out",))

BATCH = ((75, 70, 37), (3, 200, 5))


def _batch_inputs(seed, dev):
    g = _gen(seed, 11)
    out = {}
    for i, (M, N, K) in enumerate(BATCH):
        out.update({f"a{i}": _randn(g, M, K), f"b{i}": _randn(g, K, N), f"c{i}": _randn(g, M, N)})
    return out


def _batch_build(b):
    ops = _ops()
    descs = [ops.gemm_desc(b[f"a{i}"].data_ptr(), b[f"b{i}"].data_ptr(), b[f"c{i}"].data_ptr(), M, N, K, b[f"a{i}"].stride(),
                           b[f"b{i}"].stride(), b[f"c{i}"].stride(), alpha=1.0, beta=0.5 * i)
             for i, (M, N, K) in enumerate(BATCH)]
    batch = ops.GemmBatch(descs, b["a0"].device)
    torch.cuda.synchronize()
    return batch


def _batch_call(b, batch):
    batch.run()
    return []


case("gemm_batch", ["GemmBatch.run"], _batch_inputs, _batch_call, build=_batch_build, inplace=("c0", "c1"))


def _bf16_inputs(seed, dev):
    g = _gen(seed, 12)
    M, N, K = 100, 70, 25
    return {"a": _randn(g, M, K, dtype=torch.bfloat16), "bt": _randn(g, N, K, dtype=torch.bfloat16), "bias": _randn(g, N)}


case("mm_nt_bf16", ["mm_nt_bf16"], _bf16_inputs, lambda b, c: [_ops().mm_nt_bf16(b["a"], b["bt"], b["bias"])])


def _wgrad_inputs(seed, dev):
    """Rows split over T (two slices of 1000 x 1010 would be slow: the small fold shape) and an image pair."""
    g = _gen(seed, 13)
    return {"a": _randn(g, 3000, 89), "b": _randn(g, 3000, 40), "ai": _randn(g, 8, 23, 6, 6, dtype=torch.bfloat16),
            "bi": _randn(g, 8, 50, 6, 6, dtype=torch.bfloat16)}


case("wgrad", ["wgrad"], _wgrad_inputs,
     lambda b, c: [_ops().wgrad(b["a"], b["b"], alpha=0.5), _ops().wgrad(b["ai"], b["bi"])])


# ---- chains and convolutions: raw launches over staged weight planes
def _nplanes(dtype):
    return 3 if dtype == torch.float32 else 1


def _fused_inputs(seed, dev, T=50, kin=72, r=20, nout=40, dtype=torch.float32, image=None):
    ops = _ops()
    g = _gen(seed, 14)
    x = _randn(g, T, kin) if image is None else _randn(g, *image)
    win = (_randn(g, r, kin) / kin ** 0.5).to(dev)
    wout = (_randn(g, nout, r) / r ** 0.5).to(dev)
    n = _nplanes(dtype)
    return {"x": x.to(dtype), "win": ops.weight_planes(win, n, pad_rows=64), "wout": ops.weight_planes(wout, n, pad_cols=64),
            "bias": _randn(g, nout)}


case("chain_fused", ["_chain_call"], _fused_inputs,
     lambda b, c: [_ops().chain_fused(b["x"], b["win"], b["wout"], b["bias"], 40)])
case("chain_fused_save", ["_chain_call"], lambda s, dev: _fused_inputs(s, dev, T=77, kin=64, r=32, nout=24, dtype=torch.bfloat16),
     lambda b, c: list(_ops().chain_fused_save(b["x"], b["win"], b["wout"], b["bias"], 24, 32)))


def _single_inputs(seed, dev):
    ops = _ops()
    g = _gen(seed, 15)
    w = (_randn(g, 36, 48) / 48 ** 0.5).to(dev)
    return {"x": _randn(g, 3, 48, 7, 7), "w": ops.weight_planes(w, 3), "bias": _randn(g, 36)}


case("chain_single", ["_chain_call"], _single_inputs,
     lambda b, c: [_ops().chain_single(b["x"], b["w"], b["bias"], 36, image_out=True)])
case("svd_conv", ["_chain_call"], lambda s, dev: _fused_inputs(s, dev, kin=48, r=17, nout=100, image=(2, 48, 8, 8)),
     lambda b, c: [_ops().svd_conv(b["x"], b["win"], b["wout"], b["bias"], 100)])
case("svd_conv_save", ["_chain_call"],
     lambda s, dev: _fused_inputs(s, dev, kin=48, r=17, nout=100, image=(2, 48, 8, 8), dtype=torch.bfloat16),
     lambda b, c: list(_ops().svd_conv_save(b["x"], b["win"], b["wout"], b["bias"], 100, 17)))

CONV = dict(B=2, C=24, O=40, r1=12, r2=20, hw=(9, 9), k=(3, 3), s=(1, 1), p=(1, 1), dl=(1, 1))


def _conv_chain_inputs(seed, dev, dtype=torch.float32):
    ops = _ops()
    g = _gen(seed, 16)
    c = CONV
    w1 = (_randn(g, c["r1"], c["C"]) / c["C"] ** 0.5).to(dev)
    core = (_randn(g, c["r2"], c["r1"], 3, 3) / (c["r1"] * 9) ** 0.5).to(dev)
    w3 = (_randn(g, c["O"], c["r2"]) / c["r2"] ** 0.5).to(dev)
    n = _nplanes(dtype)
    return {"x": _randn(g, c["B"], c["C"], *c["hw"]).to(dtype), "dy": _randn(g, c["B"], c["O"], *c["hw"]).to(dtype),
            "bias": _randn(g, c["O"]),
            "p1": ops.weight_planes(w1, n, pad_rows=32), "p2": ops.conv_core_planes(core, n), "p3": ops.weight_planes(w3, n),
            "p3t": ops.weight_planes(w3.t(), n, pad_rows=32), "p2t": ops.conv_core_planes(core.permute(1, 0, 2, 3), n),
            "p1t": ops.weight_planes(w1.t(), n)}


def _geom():
    c = CONV
    return c["k"], c["s"], c["p"], c["dl"]


case("conv_chain", ["conv_chain"], _conv_chain_inputs,
     lambda b, c: [_ops().conv_chain(b["x"], b["p1"], b["p2"], b["p3"], b["bias"], CONV["O"], *_geom())])
case("conv_chain_save", ["conv_chain"], lambda s, dev: _conv_chain_inputs(s, dev, torch.bfloat16),
     lambda b, c: list(_ops().conv_chain_save(b["x"], b["p1"], b["p2"], b["p3"], b["bias"], CONV["O"], CONV["r1"], CONV["r2"],
                                              *_geom())))
case("conv_chain_bwd", ["conv_chain_bwd"], _conv_chain_inputs,
     lambda b, c: list(_ops().conv_chain_bwd(b["dy"], b["p3t"], b["p2t"], b["p1t"], b["x"].shape, CONV["r1"], CONV["r2"],
                                             *_geom(), save=True)))

CORE = dict(B=2, r1=16, r2=24, hw=(9, 8), k=(3, 3), s=2, p=1, dl=1)      # stride 2: the last input row has no output


def _core_inputs(seed, dev):
    ops = _ops()
    g = _gen(seed, 17)
    c = CORE
    core = (_randn(g, c["r2"], c["r1"], 3, 3) / (c["r1"] * 9) ** 0.5).to(dev)
    return {"x": _randn(g, c["B"], c["r1"], *c["hw"]), "dy": _randn(g, c["B"], c["r2"], 5, 4),
            "planes": ops.conv_core_planes(core, 3), "planes_t": ops.conv_core_planes(core.permute(1, 0, 2, 3), 3)}


def _cgeom():
    c = CORE
    return c["k"], c["s"], c["p"], c["dl"]


case("core_conv", ["_core_conv_call"], _core_inputs,
     lambda b, c: [_ops().core_conv(b["x"], b["planes"], CORE["r2"], *_cgeom())])
case("core_conv_dgrad", ["_core_conv_call"], _core_inputs,
     lambda b, c: [_ops().core_conv_dgrad(b["dy"], b["planes_t"], b["x"].shape, *_cgeom())])
case("core_conv_wgrad", ["core_conv_wgrad"], _core_inputs,
     lambda b, c: [_ops().core_conv_wgrad(b["dy"], b["x"], *_cgeom())])


# ---- layer kernels through their autograd wrappers (tadmm/functional.py): forward and backward on the side stream
def _hf():
    from tadmm import functional
    return functional


def _lin_inputs(seed, dev, image=None):
    g = _gen(seed, 20)
    kin, r, nout = 72, 20, 40
    x = _randn(g, 50, kin) if image is None else _randn(g, image[0], kin, *image[1:])
    return {"x": x, "w_in": _randn(g, r, kin) / kin ** 0.5, "w_out": _randn(g, nout, r) / r ** 0.5, "bias": _randn(g, nout)}


_CHAIN_BWD = ["_chain_call", "wgrad"]
case("linear_chain", _CHAIN_BWD, _lin_inputs,
     lambda b, c: [_hf().linear_chain(b["x"], b["w_in"], b["w_out"], b["bias"], save=True)],
     wrt=("x", "w_in", "w_out", "bias"))
case("linear_chain_recompute", ["_chain_call"], _lin_inputs,
     lambda b, c: [_hf().linear_chain(b["x"], b["w_in"], b["w_out"], b["bias"], save=False)],
     wrt=("x", "w_in", "w_out", "bias"))
case("conv1x1_chain", _CHAIN_BWD, lambda s, dev: _lin_inputs(s, dev, image=(3, 7, 7)),
     lambda b, c: [_hf().conv1x1_chain(b["x"], b["w_in"], b["w_out"], b["bias"], save=True)],
     wrt=("x", "w_in", "w_out", "bias"))


def _conv_layer_inputs(seed, dev, dtype=torch.bfloat16):
    g = _gen(seed, 21)
    c = CONV
    return {"x": _randn(g, c["B"], c["C"], *c["hw"]).to(dtype), "w_in": (_randn(g, c["r1"], c["C"]) / c["C"] ** 0.5).to(dtype),
            "core": (_randn(g, c["r2"], c["r1"], 3, 3) / (c["r1"] * 9) ** 0.5).to(dtype),
            "w_out": (_randn(g, c["O"], c["r2"]) / c["r2"] ** 0.5).to(dtype), "bias": _randn(g, c["O"]).to(dtype)}


case("conv_chain_layer", ["conv_chain", "conv_chain_bwd", "wgrad"], _conv_layer_inputs,
     lambda b, c: [_hf().conv_chain(b["x"], b["w_in"], b["core"], b["w_out"], b["bias"], 1, 1, 1)],
     wrt=("x", "w_in", "core", "w_out", "bias"))
case("conv_chain_layer_f32", ["conv_chain", "conv_chain_bwd", "wgrad"],
     lambda s, dev: _conv_layer_inputs(s, dev, torch.float32),
     lambda b, c: [_hf().conv_chain(b["x"], b["w_in"], b["core"], b["w_out"], b["bias"], 1, 1, 1)],
     wrt=("x", "w_in", "core", "w_out", "bias"))


def _core_layer_inputs(seed, dev):
    g = _gen(seed, 22)
    c = CORE
    return {"x": _randn(g, c["B"], c["r1"], *c["hw"]), "core": _randn(g, c["r2"], c["r1"], 3, 3) / (c["r1"] * 9) ** 0.5}


case("core_conv_layer", ["_core_conv_call"], _core_layer_inputs,
     lambda b, c: [_hf().core_conv(b["x"], b["core"], CORE["s"], CORE["p"], CORE["dl"])], wrt=("x", "core"))

EMB = ([4, 3, 5], [3, 1, 5], [1, 17, 33, 1])         # _emb_ref.SHAPES["d3"]


def _emb_inputs(seed, dev):
    import _emb_ref as E
    out = {f"core{k}": torch.from_numpy(c) for k, c in enumerate(E.make_cores(EMB, seed=seed))}
    idx = E.token_set("random130", EMB, 64, seed=seed)
    idx[5] = 4 * 3 * 5 + seed                          # one index out of range: a zero row and the counter
    out["index"] = torch.from_numpy(idx)
    out["counter"] = torch.tensor([3 + seed], dtype=torch.int32)
    return out


case("ttm_embedding", ["ttm_gather", "ttm_gather_bwd"], _emb_inputs,
     lambda b, c: [_hf().ttm_embedding([b[f"core{k}"] for k in range(3)], b["index"], b["counter"], route="native")],
     wrt=("core0", "core1", "core2"), inplace=("counter",))


def _lstm_inputs(seed, dev):
    """The sizes and distributions of _lstm_ref.CASES["odd"]: T = 5, B = 3, H = 24."""
    T, B, H = 5, 3, 24
    g = _gen(seed, 23)
    return {"xp": _randn(g, T, B, 4 * H, scale=1.5),
            "w_hh": (torch.rand(4 * H, H, generator=g, dtype=torch.float64) * 2 - 1).float() * (2 / H ** 0.5),
            "h0": _randn(g, B, H, scale=0.5), "c0": _randn(g, B, H, scale=0.5)}


def _lstm_call(b, c):
    y, (hT, cT) = _hf().lstm_sequence(b["xp"], b["w_hh"], b["h0"], b["c0"], route="launch")
    return [y, hT, cT]


case("lstm_sequence", ["_lstm_fwd", "lstm_seq_bwd"], _lstm_inputs, _lstm_call, wrt=("xp", "w_hh", "h0", "c0"))


def _distill_inputs(seed, dev):
    import _distill_ref as D
    s, k, t, target = D.make_inputs(5, 65, "float32", 40 + seed, "index")
    return {"s": s, "k": k, "t": t, "target": target}


case("distillation_loss", ["distill_loss"], _distill_inputs,
     lambda b, c: [_hf().distillation_loss(b["s"], b["k"], b["t"], b["target"], base="index", kd="soft", alpha=0.5, tau=3.0,
                                           smoothing=0.1, route="launch")], wrt=("s", "k"))


def _mse_inputs(seed, dev):
    import _layer_mse_ref as L
    out = {}
    for i in range(2):
        out[f"sa{i}"], out[f"ta{i}"] = L.att_pair(2, 2, 33, 50 + 10 * seed + i)
        out[f"sr{i}"], out[f"tr{i}"] = L.rep_pair((2, 33, 52), 60 + 10 * seed + i)
    return out


def _mse_call(b, c):
    return list(_hf().intermediate_distillation_loss([b["sa0"], b["sa1"]], [b["ta0"], b["ta1"]], [b["sr0"], b["sr1"]],
                                                     [b["tr0"], b["tr1"]], route="launch"))


case("intermediate_distillation_loss", ["layer_mse"], _mse_inputs, _mse_call, wrt=("sa0", "sa1", "sr0", "sr1"))


def _attn_inputs(seed, dev):
    import _attn_ref as A
    B, H, S, d = 2, 2, 33, 26
    g = _gen(seed, 24)
    return {"q": _randn(g, B, S, H * d), "k": _randn(g, B, S, H * d), "v": _randn(g, B, S, H * d),
            "mask": A.padding_mask([33, 20] if seed == 0 else [27, 33], S),
            "keep": (torch.rand(B, H, S, S, generator=g) >= 0.1).to(torch.uint8)}


case("self_attention", ["attn_fwd", "attn_bwd"], _attn_inputs,
     lambda b, c: list(_hf().self_attention(b["q"], b["k"], b["v"], b["mask"], 2, dropout_p=0.1, training=True,
                                            keep=b["keep"], route="launch")), wrt=("q", "k", "v"))


def _norm_inputs(seed, dev, shape, salt):
    g = _gen(seed, salt)
    hidden = shape[-1]
    return {"x": _randn(g, *shape), "res": _randn(g, *shape), "weight": 1.0 + 0.1 * _randn(g, hidden),
            "bias": 0.1 * _randn(g, hidden), "keep": (torch.rand(*shape, generator=g) >= 0.1).to(torch.uint8)}


def _rln_call(b, c):
    return [_hf().residual_layer_norm(b["x"], b["res"], b["weight"], b["bias"], dropout_p=0.1, training=True, keep=b["keep"],
                                      route="launch")]


_NORM_WRT = ("x", "res", "weight", "bias")
case("residual_layer_norm_5x65", ["bertnorm_fwd", "bertnorm_bwd"], lambda s, dev: _norm_inputs(s, dev, (5, 65), 25), _rln_call,
     wrt=_NORM_WRT)
case("residual_layer_norm_17x768", ["bertnorm_fwd", "bertnorm_bwd"], lambda s, dev: _norm_inputs(s, dev, (17, 768), 26),
     _rln_call, wrt=_NORM_WRT)


def _aln_inputs(seed, dev):
    out = _norm_inputs(seed, dev, (3, 5, 65), 27)
    out["path_keep"] = torch.tensor([[1, 0, 1], [0, 1, 1]][seed], dtype=torch.uint8)
    return out


case("add_layer_norm", ["prenorm_fwd", "prenorm_bwd"], _aln_inputs,
     lambda b, c: list(_hf().add_layer_norm(b["x"], b["res"], b["weight"], b["bias"], dropout_p=0.1, drop_path_p=0.2,
                                            training=True, keep=b["keep"], path_keep=b["path_keep"], route="launch")),
     wrt=_NORM_WRT)


def _bn_params(g, c):
    return {"rm": 0.1 * _randn(g, c), "rv": 1.0 + 0.1 * torch.rand(c, generator=g), "weight": 1.0 + 0.1 * _randn(g, c),
            "bias": 0.1 * _randn(g, c)}


def _bnact_inputs(seed, dev):
    g = _gen(seed, 28)
    shape = (8, 3, 7, 7)                               # _bn_ownership.BNACT: the element walk that crosses planes
    return {"x": _randn(g, *shape), "residual": _randn(g, *shape), **_bn_params(g, 3)}


case("batch_norm_act", ["bnact_fwd", "bnact_bwd"], _bnact_inputs,
     lambda b, c: [_hf().batch_norm_act(b["x"], b["rm"], b["rv"], b["weight"], b["bias"], b["residual"], training=True,
                                        route="launch")],
     wrt=("x", "residual", "weight", "bias"), inplace=("rm", "rv"))

DENSE = ((5, 3, 3), 8, 7, 7)                          # _bn_ownership.DENSEBN: three segments, element walk


def _dense_inputs(seed, dev):
    g = _gen(seed, 29)
    chans, n, h, w = DENSE
    out = {f"seg{k}": _randn(g, n, c, h, w) for k, c in enumerate(chans)}
    out.update(_bn_params(g, sum(chans)))
    return out


case("dense_batch_norm_act", ["densebn_stats", "densebn_fwd", "densebn_bwd"], _dense_inputs,
     lambda b, c: [_hf().dense_batch_norm_act([b["seg0"], b["seg1"], b["seg2"]], b["rm"], b["rv"], b["weight"], b["bias"],
                                              training=True, route="launch")],
     wrt=("seg0", "seg1", "seg2", "weight", "bias"), inplace=("rm", "rv"))


def _dw_inputs(seed, dev):
    g = _gen(seed, 30)
    n, c, h, w = 6, 512, 7, 8                          # _bn_ownership.DWBN: stride 2, G > 1, odd H
    return {"x": _randn(g, n, c, h, w), "conv_weight": _randn(g, c, 1, 3, 3) / 3.0, **_bn_params(g, c)}


case("depthwise_bn_relu6", ["dwbn_fwd", "dwbn_bwd"], _dw_inputs,
     lambda b, c: [_hf().depthwise_bn_relu6(b["x"], b["conv_weight"], b["rm"], b["rv"], b["weight"], b["bias"], stride=2,
                                            training=True, route="launch")],
     wrt=("x", "conv_weight", "weight", "bias"), inplace=("rm", "rv"))

# the cheap elementwise launch the sensitivity test sends to the null stream
case("bertnorm_fwd", ["bertnorm_fwd"], lambda s, dev: _norm_inputs(s, dev, (5, 65), 31),
     lambda b, c: [_ops().bertnorm_fwd(b["x"], b["res"], b["weight"], b["bias"], p=0.1, keep=b["keep"])[0]])


# ---- plans with state
ORTH = ((24, 20), (7, 33), (64, 23))                  # tall, wide (Gram of rows) and tall factors


def _orth_inputs(seed, dev):
    g = _gen(seed, 32)
    return {f"p{i}": _randn(g, *s) / max(s) ** 0.5 for i, s in enumerate(ORTH)}


def _orth_build(b):
    from tadmm import orthogonal
    sel = []
    for i, s in enumerate(ORTH):
        b[f"p{i}"].requires_grad_(True)
        sel.append((f"p{i}", b[f"p{i}"], s[0] < s[1]))
    plan = orthogonal._OrthPlan(sel, b["p0"].device)
    torch.cuda.synchronize()
    return plan


def _orth_call(b, plan):
    loss, grads = plan.run(0.01, True)
    return [loss.reshape(1)] + list(grads)


case("orth_regulariser", [], _orth_inputs, _orth_call, build=_orth_build)

STIEFEL = ((24, 20), (33, 7), (64, 23))               # of test_gpu_stiefel.SHAPES: all resident in the LDS


def _stiefel_inputs(seed, dev, adam=False):
    import _stiefel_ref as S
    out = {}
    for i, (n, p) in enumerate(STIEFEL):
        rng = np.random.default_rng(100 * seed + n + p)
        out[f"x{i}"] = torch.from_numpy(S.qr_pos(rng.standard_normal((n, p))).astype(np.float32))
        out[f"g{i}"] = torch.from_numpy(rng.standard_normal((n, p)).astype(np.float32))
        out[f"m{i}"] = torch.from_numpy(0.1 * rng.standard_normal((n, p)).astype(np.float32))
    if adam:
        rng = np.random.default_rng(7 + seed)
        out["v"] = torch.from_numpy(rng.uniform(0.5, 2.0, 3).astype(np.float32))
        out["vmax"] = out["v"] * 1.5
        out["steps"] = torch.tensor([3, 1, 7] if seed == 0 else [2, 5, 1], dtype=torch.int32)
    return out


def _stiefel_build(b):
    plan = _ops().StiefelPlan([(b[f"x{i}"], b[f"g{i}"], b[f"m{i}"]) for i in range(3)])
    assert len(plan.native) == 3
    torch.cuda.synchronize()
    return plan


def _stiefel_step(b, plan):
    plan.step(0.01, 0.9, 0.0, 0.05, True)
    return [plan.status]


def _stiefel_adam(b, plan):
    plan.adam_step(1e-2, (0.9, 0.999), 1e-8, 0.05, True, b["v"], b["vmax"], b["steps"])
    return [plan.status]


def _stiefel_project(b, c):
    plan = _ops().stiefel_project_(*[b[f"x{i}"] for i in range(3)])      # builds its plan under the caller's stream
    return [plan.status]


_XM = tuple(f"{k}{i}" for k in "xm" for i in range(3))
case("stiefel_step", ["StiefelPlan.step"], _stiefel_inputs, _stiefel_step, build=_stiefel_build, inplace=_XM)
case("stiefel_adam_step", ["StiefelPlan.adam_step"], lambda s, dev: _stiefel_inputs(s, dev, True), _stiefel_adam,
     build=_stiefel_build, inplace=_XM + ("v", "vmax", "steps"))


def _project_inputs(seed, dev):
    rng = np.random.default_rng(11 + seed)
    return {f"x{i}": torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for i, s in enumerate(STIEFEL)}


case("stiefel_project", ["StiefelPlan.__init__", "StiefelPlan.project_"], _project_inputs, _stiefel_project,
     inplace=("x0", "x1", "x2"), host_sync=True)

ADAM_SIZES = (4095, 4096, 4097, 7)                    # either side of ops.BERTADAM_CHUNK, and a tiny tensor


def _adam_inputs(seed, dev):
    g = _gen(seed, 33)
    out = {}
    for i, n in enumerate(ADAM_SIZES):
        out[f"p{i}"], out[f"g{i}"] = _randn(g, n), _randn(g, n, scale=0.05 * (i + 1))
        out[f"m{i}"], out[f"v{i}"] = _randn(g, n, scale=0.01), torch.rand(n, generator=g) * 1e-3
    return out


def _adam_build(b):
    plan = _ops().BertAdamPlan([tuple(b[f"{k}{i}"] for k in "pgmv") for i in range(len(ADAM_SIZES))])
    torch.cuda.synchronize()
    return plan


def _adam_step(b, plan):
    plan.step(1e-3, 0.9, 0.999, 1e-6, 0.01, 1.0)
    return [plan.grad_norms()]


_PMV = tuple(f"{k}{i}" for k in "pmv" for i in range(len(ADAM_SIZES)))
case("bert_adam_step", ["BertAdamPlan.step"], _adam_inputs, _adam_step, build=_adam_build, inplace=_PMV)
case("bert_adam_create_and_step", ["BertAdamPlan.__init__", "BertAdamPlan.step"], _adam_inputs,
     lambda b, c: _adam_step(b, _adam_build_here(b)), inplace=_PMV, host_sync=True)


def _adam_build_here(b):
    """The plan built inside the call: its table upload goes to the caller's stream and is waited for."""
    return _ops().BertAdamPlan([tuple(b[f"{k}{i}"] for k in "pgmv") for i in range(len(ADAM_SIZES))])


BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Entries that wait for the device by design; the table flags exactly their cases `host_sync`.
EXCLUDED = {}
