"""Every native launch on a side stream behind a delayed producer: the table of tests/_streams.py, one test per case,
and two tests that prove the harness can fail.  `pytest -s` prints every case's host time and delay."""
import pytest
import torch

import _streams as S

pytestmark = pytest.mark.gpu

RECORD = {}
FAULT = []            # the first device error of the module: nothing more is started on the device behind it


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def delay(dev):
    d = S.Delay(dev)
    print(f"\nstreams: delay calibrated to {d.calibrated_ms:.1f} ms ({d.units} units, target {d.target_ms:.0f} ms); "
          f"{d.rejected} side streams queued behind the default stream's queue and were passed over")
    yield d
    torch.cuda.synchronize(dev)
    timed = {k: v for k, v in RECORD.items() if not S.BY_NAME[k].host_sync}
    if timed:
        worst = max(timed, key=lambda k: timed[k][0])
        print(f"\nstreams: {len(RECORD)} cases, {len(timed)} with a host-time bar; worst host time "
              f"{timed[worst][0]:.2f} ms ({worst}) under a delay of {timed[worst][1]:.1f} ms; calibrated delay "
              f"{d.calibrated_ms:.1f} ms")


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_side_stream_behind_a_delayed_producer(name, dev, delay, monkeypatch):
    case = S.BY_NAME[name]
    assert not FAULT, f"not run: the device reported an error in {FAULT[0]}"
    from tadmm import ops
    reached = set()
    monkeypatch.setattr(ops, "_stream", S.recording_stream(ops, reached))
    try:
        rep = S.run_case(case, dev, delay)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            FAULT.append(name)
        raise
    RECORD[name] = (rep.host_ms, rep.delay_ms)
    print(f"\nstreams: {name}: host {rep.host_ms:.2f} ms, delay {rep.delay_ms:.1f} ms"
          + (" (the entry waits for the device by design)" if case.host_sync else "") + f"; reached {sorted(reached)}")
    assert rep.ok, rep.message
    assert rep.window_open, f"{name}: the default stream ran behind this case's producer: an early launch was not observable"
    assert set(case.entries) <= reached, f"{name} declares {sorted(set(case.entries) - reached)} and did not reach them"
    if not case.host_sync:
        assert rep.host_ms <= rep.delay_ms / S.HOST_MARGIN, \
            f"{name}: call() returned after {rep.host_ms:.2f} ms of host time under a delay of {rep.delay_ms:.1f} ms: " \
            f"the producer's copies were not safely behind the launch call (or the entry waited for the device)"


def test_the_window_is_open(dev, delay):
    """Torch only: while the side stream sleeps, the default stream still sees the decoy in a buffer whose restoring copy
    is queued behind the delay -- the window every case of the table relies on."""
    g = torch.Generator().manual_seed(5)
    x, decoy = torch.randn(5, 65, generator=g).to(dev), torch.randn(5, 65, generator=g).to(dev)
    buf = decoy.clone()
    torch.cuda.synchronize(dev)
    side = delay.side
    with torch.cuda.stream(side):
        delay.enqueue()
        buf.copy_(x)
    early = buf.clone()                       # default stream, in front of the synchronisation
    torch.cuda.current_stream(dev).synchronize()
    early_is_decoy = torch.equal(early, decoy)
    side.synchronize()
    assert early_is_decoy, "the default stream waited for the side stream: the window is closed and the table proves nothing"
    assert torch.equal(buf, x)


def test_a_launch_on_the_null_stream_is_caught(dev, delay, monkeypatch):
    """The same harness with `ops._stream` answering 0 for one cheap elementwise launch: it runs in front of the
    producer on valid decoy inputs, and the report says the result equals the decoy's."""
    from tadmm import ops
    monkeypatch.setattr(ops, "_stream", lambda device: 0)
    rep = S.run_case(S.BY_NAME["bertnorm_fwd"], dev, delay)
    torch.cuda.synchronize(dev)
    assert not rep.ok, "a launch on the null stream went unnoticed"
    assert rep.equals_decoy and "DECOY" in rep.message, rep.message
