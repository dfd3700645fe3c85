"""The super-pair route of the Jacobi eigen-solver (N > 64, rows of at most 512 doubles) against the bytes recorded in
tests/golden/g17_tick_bits.json (written by `tests/golden/make_golden_tick_bits.py <commit>` on the commit named in the
fixture, where the within-super-block rotations of a sweep's first tick still ran in a launch of their own).  The cases
steer single workgroups of jacobi_tick3_kernel through each of its exits: columns rotated by the self pass alone (stored
although neither round rotated), nothing to rotate at all, one coupled super-pair among idle ones, the Rayleigh-Ritz
shape with pad rows, and a group in which one problem is finished sweeps before the other.  Same operations in the same
order on the same data, so the test asks for equal sha256; every solve is also held against numpy.linalg.eigvalsh in
float64 with the bound of tests/test_gpu_kernels.py::test_eigh_jacobi (1e-12 of the largest eigenvalue)."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_tick_bits", os.path.join(_GOLDEN, "make_golden_tick_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

_CASES = list(bits.cases())


@pytest.fixture(scope="module")
def fixture_doc():
    with open(bits.FIXTURE) as f:
        return json.load(f)


def test_fixture_names_its_commit_and_every_case(fixture_doc):
    assert len(fixture_doc["commit"]) >= 7
    assert len(fixture_doc["cases"]) == len(_CASES)


@pytest.mark.parametrize("index", range(len(_CASES)))
def test_bits_equal_recorded(fixture_doc, index):
    name, in_sha, out, checks = _CASES[index]()
    want = fixture_doc["cases"][name]
    assert in_sha == want["inputs_sha256"], "%s: the seeded inputs differ from the recorded ones" % name
    for ev, ref in checks:
        err = np.abs(ev - ref).max()
        print("%s: eigenvalue error %.3g, bound %.3g" % (name, err, 1e-12 * ref[0]))
        np.testing.assert_allclose(ev, ref, rtol=0, atol=1e-12 * ref[0])
    assert out.size == want["numel"] and str(out.dtype) == want["dtype"]
    got = bits._sha(out)
    if got != want["output_sha256"]:
        flat = np.ascontiguousarray(out).ravel()
        bad = [(i, h, flat[i:i + 1].tobytes().hex()) for i, h in want["samples"] if flat[i:i + 1].tobytes().hex() != h]
        print("%s: %d of %d sampled entries differ (index, recorded, got): %s" % (name, len(bad), len(want["samples"]), bad[:8]))
    assert got == want["output_sha256"], "%s: output bytes differ from commit %s" % (name, fixture_doc["commit"])
