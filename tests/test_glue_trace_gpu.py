"""The Python glue's native calls, line for line against the recording made before the glue got its shared helpers
(tests/glue_trace/recorder.py says what a line holds): every call, its order, every argument with pointers as
name+offset, every exception text, and the bytes each scenario asked of the allocator.  There is no allow list."""
import difflib
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "glue_trace")


def _recorder():
    spec = importlib.util.spec_from_file_location("glue_trace_recorder", os.path.join(HERE, "recorder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_glue_trace_matches_the_recording(gpu, monkeypatch):
    if os.environ.get("SMX_TEST_OPTS"):
        pytest.skip("the recording holds the plans of the default options")
    r = _recorder()
    rec = r.Recorder(gpu)
    rec.install(monkeypatch)
    got = r.record(rec)
    with open(os.path.join(HERE, "expected.txt")) as f:
        want = f.read().splitlines()
    diff = list(difflib.unified_diff(want, got, "expected.txt", "this run", n=2, lineterm=""))
    changed = sum(1 for d in diff if d[:1] in "+-" and d[:3] not in ("+++", "---"))
    assert not diff, f"{changed} lines differ:\n" + "\n".join(diff[:80])
