"""The fp64 kernels on the filter's critical chain -- `dgemm_nt_tile_kernel` <32,4,32>, <32,2,64>, <64,2,64> with every
epilogue, ring and gate, `daxpby_kernel`, the `ops.dgemm` kernels, `ops.cholqr_` and two filtered `ProjectionPlan`s --
against the bytes recorded in tests/golden/g14_filter_chain_bits.json (written by tests/golden/make_golden_filter_bits.py
on the commit named in the fixture, with the kernels as they were before their loads were reordered).  The kernels keep
every floating-point operation and its order, so the test asks for equal sha256; a different hash of the seeded INPUTS is
a failure of the test's own set-up.  Each case also holds its outputs elementwise against numpy float64 within
K * 2^-52 * |A| |B|^T carried through the epilogue, so the recorded bytes are those of a known-good result."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_filter_bits", os.path.join(_GOLDEN, "make_golden_filter_bits.py"))
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
def test_bits_equal_recorded_and_close_to_float64(fixture_doc, index):
    name, in_sha, out, checks = _CASES[index]()
    want = fixture_doc["cases"][name]
    assert in_sha == want["inputs_sha256"], "%s: the seeded inputs differ from the recorded ones" % name
    bad = bits.failed_checks(checks)
    assert not bad, "%s: outside the elementwise bound (what, excess, index): %s" % (name, bad[:4])
    assert out.size == want["numel"] and str(out.dtype) == want["dtype"]
    got = bits._sha(out)
    if got != want["output_sha256"]:
        flat = np.ascontiguousarray(out).ravel()
        diff = [(i, h, flat[i:i + 1].tobytes().hex()) for i, h in want["samples"] if flat[i:i + 1].tobytes().hex() != h]
        print("%s: %d of %d sampled entries differ (index, recorded, got): %s" % (name, len(diff), len(want["samples"]), diff[:8]))
    assert got == want["output_sha256"], "%s: output bytes differ from commit %s" % (name, fixture_doc["commit"])
