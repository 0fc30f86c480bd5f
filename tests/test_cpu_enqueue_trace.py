"""The engine's enqueue sequence, pinned (no GPU, no libmgr.so): every case of tests/enqueue_recorder.py gives the trace recorded in
tests/golden/enqueue_traces.json - which calls, in which order, with which buffers, scan forms, seeds and gate words.  A change of the
host-side scheduling code that is meant to change nothing must leave every trace as it is; one that is meant to change the schedule
regenerates the goldens (tests/golden/make_enqueue_traces.py) and shows its effect as a diff of the two traces kept in full."""
import importlib.util
import json
import os

import pytest

import enqueue_recorder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_enqueue_traces", os.path.join(GOLDEN, "make_enqueue_traces.py"))
make = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make)

with open(make.JSON) as f:
    WANT = json.load(f)
CASES = enqueue_recorder.enqueue_cases()


def test_the_goldens_cover_exactly_the_cases():
    assert sorted(WANT) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_enqueue_trace_equals_the_golden(name):
    text = CASES[name]()
    got, want = make.digest(text), WANT[name]
    if got == want:
        if name in enqueue_recorder.FULL_TEXT:
            with open(make.text_path(name)) as f:
                assert f.read() == text, "tests/golden/enqueue_trace_%s.txt is not the trace enqueue_traces.json describes" % name
        return
    lines = text.splitlines()
    gm, wm = got["line_marks"], want["line_marks"]
    i = next((k for k in range(min(len(gm), len(wm)) // 3) if gm[3 * k:3 * k + 3] != wm[3 * k:3 * k + 3]), min(len(gm), len(wm)) // 3)
    was = ""
    if name in enqueue_recorder.FULL_TEXT:
        with open(make.text_path(name)) as f:
            old = f.read().splitlines()
        was = "\n  golden: %s" % (old[i] if i < len(old) else "<end of trace>")
    pytest.fail("case %s: %d lines (golden: %d), first difference at line %d:\n  now:    %s%s\n"
                "the traces in full: python tests/golden/make_enqueue_traces.py --dump DIR"
                % (name, got["lines"], want["lines"], i + 1, lines[i] if i < len(lines) else "<end of trace>", was))
