"""The Jacobi eigen-solver (`ops.eigh`, `ops.eigh_partial` and the eigen groups of two `ProjectionPlan`s) against the bytes
recorded in tests/golden/g13_eigh_bits.json (written by `tests/golden/make_golden_bits.py <commit> <file> eigh` on the
commit named in the fixture).  The cases reach every launch shape of csrc/jacobi.hip: the single-launch solver, the
super-pair kernel with its self pass from 6 super-blocks up to the largest row that fits, the resident and the streamed pair
kernel, rank-deficient inputs, a group of problems with different player counts on one aligned schedule, and a group on
the pair kernel.  The kernels promise the same floating-point operations in the same order on the same data however their
stages are written down, so the test asks for equal sha256; a different hash of the seeded INPUTS is a failure of the
test's own set-up, not a skip."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_bits", os.path.join(_GOLDEN, "make_golden_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

_CASES = list(bits.eigh_cases())


@pytest.fixture(scope="module")
def fixture_doc():
    with open(bits.EIGH_FIXTURE) as f:
        return json.load(f)


def test_fixture_names_its_commit_and_every_case(fixture_doc):
    assert len(fixture_doc["commit"]) >= 7
    assert len(fixture_doc["cases"]) == len(_CASES)


@pytest.mark.parametrize("index", range(len(_CASES)))
def test_bits_equal_recorded(fixture_doc, index):
    name, in_sha, out = _CASES[index]()
    want = fixture_doc["cases"][name]
    assert in_sha == want["inputs_sha256"], "%s: the seeded inputs differ from the recorded ones" % name
    assert out.size == want["numel"] and str(out.dtype) == want["dtype"]
    got = bits._sha(out)
    if got != want["output_sha256"]:
        flat = np.ascontiguousarray(out).ravel()
        bad = [(i, h, flat[i:i + 1].tobytes().hex()) for i, h in want["samples"] if flat[i:i + 1].tobytes().hex() != h]
        print("%s: %d of %d sampled entries differ (index, recorded, got): %s" % (name, len(bad), len(want["samples"]), bad[:8]))
    assert got == want["output_sha256"], "%s: output bytes differ from commit %s" % (name, fixture_doc["commit"])
