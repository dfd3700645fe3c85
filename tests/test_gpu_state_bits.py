"""The filter's state kernels (csrc/filter.hip: init, plan, flags, theta, moments, verdict, emit) and the Gram's split-K
reduce (csrc/gram.hip) against the bytes and the course recorded in tests/golden/g16_state_bits.json (written by
tests/golden/make_golden_state_bits.py on the commit named in the fixture, before these kernels' loads were hoisted and
their pointers pinned to the global address space).  They keep every floating-point operation, its operands and its
order, and every state word they write, so the test asks for equal sha256 of the residuals, Z and U of two plan
iterations, for the recorded `filter_stats()` (eligible, solves, fallbacks, stages) and Jacobi sweep count of each run,
and for equal bytes of the split-K Grams (ksplit 2, 3, 5, 11).  A different hash of the seeded INPUTS is a failure of the
test's own set-up."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_state_bits", os.path.join(_GOLDEN, "make_golden_state_bits.py"))
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


def test_low_rank_case_recorded_one_fallback(fixture_doc):
    runs = fixture_doc["cases"]["plan_low_rank_beside_healthy"]["filter_stats"]
    assert runs[0][2] == 1, runs


@pytest.mark.parametrize("index", range(len(_CASES)))
def test_bits_and_course_equal_recorded(fixture_doc, index):
    name, in_sha, out, record = _CASES[index]()
    want = fixture_doc["cases"][name]
    assert in_sha == want["inputs_sha256"], "%s: the seeded inputs differ from the recorded ones" % name
    for key in ("filter_stats", "jacobi_sweeps"):
        if key in record:
            print(name, key, "got", record[key], "recorded", want[key])
            assert record[key] == want[key], "%s: %s differs from commit %s" % (name, key, fixture_doc["commit"])
    assert out.size == want["numel"] and str(out.dtype) == want["dtype"]
    got = bits._sha(out)
    if got != want["output_sha256"]:
        flat = np.ascontiguousarray(out).ravel()
        bad = [(i, h, flat[i:i + 1].tobytes().hex()) for i, h in want["samples"] if flat[i:i + 1].tobytes().hex() != h]
        print("%s: %d of %d sampled entries differ (index, recorded, got): %s" % (name, len(bad), len(want["samples"]), bad[:8]))
    assert got == want["output_sha256"], "%s: output bytes differ from commit %s" % (name, fixture_doc["commit"])
