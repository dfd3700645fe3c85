"""bench.py as a caller runs it: a plain run times exactly --steps steps and prints the headline line without the
--full blocks; --dump-outputs writes Z / U / residuals of the last timed step, the same for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("config", ["resnet32_tt", "resnet32_tk"])
def test_plain_run_dumps_the_last_step(tmp_path, config):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = _bench("--config", config, "--steps", "3", "--warmup", "1", "--dump-outputs", a)
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6 * 1e3
    for key in ("roofline", "phases_ms", "per_layer_svd_gflops", "forward", "cpu_baseline"):
        assert key not in line, key
    _bench("--config", config, "--steps", "3", "--warmup", "1", "--dump-outputs", b)
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) and "residual_sq.npy" in files
    n_layers = sum(f.endswith(".Z.npy") for f in files)
    assert n_layers == 30 and sum(f.endswith(".U.npy") for f in files) == n_layers
    assert sum(os.path.getsize(os.path.join(a, f)) for f in files) <= 64 << 20
    resid = np.load(os.path.join(a, "residual_sq.npy"))
    assert resid.dtype == np.float64 and resid.shape == (n_layers,)
    assert abs(resid.sum() - line["residual_sq"]) <= 1e-9 * abs(line["residual_sq"])
    for f in files:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all()
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-6 * max(1.0, float(np.abs(x).max())), err_msg=f)
