"""Completeness of the stream table (tests/_streams.py): every function or method of tadmm/ops.py that hands
`_stream(...)` to the library is reached by a named case, or excluded with a reason.  A new entry without a stream case
fails here, without a GPU."""
import ast
import os

import _streams as S

OPS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dnn-compression-tensor-admm_amd", "tadmm",
                   "ops.py")


def _calls_stream(node) -> bool:
    return any(isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "_stream" for n in ast.walk(node))


def stream_callers():
    """Qualified names of the module-level functions and the methods of ops.py whose body (nested functions included)
    calls `_stream(`."""
    with open(OPS) as f:
        tree = ast.parse(f.read())
    found = set()
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name != "_stream" and _calls_stream(node):
            found.add(node.name)
        elif isinstance(node, ast.ClassDef):
            for m in node.body:
                if isinstance(m, ast.FunctionDef) and _calls_stream(m):
                    found.add(f"{node.name}.{m.name}")
    return found


def test_the_table_imports_without_a_device():
    assert len(S.CASES) >= 40 and len(S.BY_NAME) == len(S.CASES)
    for c in S.CASES:
        assert callable(c.inputs) and callable(c.call) and isinstance(c.entries, tuple), c.name
        assert not (set(c.inplace) & set(c.wrt)), c.name


def test_every_stream_caller_has_a_case_or_a_reason():
    callers = stream_callers()
    assert len(callers) >= 40, "the parse lost the call sites"
    reached = {e for c in S.CASES for e in c.entries}
    assert reached <= callers, f"cases name entries that hand no stream to the library: {sorted(reached - callers)}"
    assert set(S.EXCLUDED) <= callers and not (set(S.EXCLUDED) & reached)
    assert all(isinstance(r, str) and r.strip() for r in S.EXCLUDED.values())
    missing = callers - reached - set(S.EXCLUDED)
    assert not missing, f"no stream case reaches {sorted(missing)}: add one to tests/_streams.py (or a reason to EXCLUDED)"


def test_the_parse_sees_nested_launchers_and_methods():
    callers = stream_callers()
    assert {"_chain_call", "_LayerPlan.run", "GemmBatch.run", "BertAdamPlan.__init__", "mm"} <= callers
    assert "_stream" not in callers
