"""Writes tests/golden/enqueue_traces.json: per case of tests/enqueue_recorder.py the line count and the sha256 of the trace, and the
traces of enqueue_recorder.FULL_TEXT in full beside it (a later schedule change then shows as a readable diff).

    python tests/golden/make_enqueue_traces.py            write the goldens from the mgr_amd that is importable
    python tests/golden/make_enqueue_traces.py --check    compare, write nothing (exit status 1 on a difference)
    python tests/golden/make_enqueue_traces.py --dump DIR every trace in full into DIR

The package under test is the `mgr_amd` found first on PYTHONPATH (a worktree of another commit records THAT commit's engine with
this recorder), else this checkout's.
"""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.append(os.path.dirname(TESTS))      # (behind PYTHONPATH: mgr_amd, oracle)
sys.path.insert(0, TESTS)
import mgr_amd  # noqa: E402,F401
import enqueue_recorder  # noqa: E402

JSON = os.path.join(HERE, "enqueue_traces.json")


def digest(text):
    """line_marks: three hex digits per line, so that a mismatch can name its first line without the full text being committed."""
    marks = "".join(hashlib.sha256(line.encode()).hexdigest()[:3] for line in text.splitlines())
    return {"lines": text.count("\n"), "sha256": hashlib.sha256(text.encode()).hexdigest(), "line_marks": marks}


def text_path(name):
    return os.path.join(HERE, "enqueue_trace_%s.txt" % name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--dump")
    a = ap.parse_args()
    traces = {name: run() for name, run in enqueue_recorder.enqueue_cases().items()}
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
        for name, text in traces.items():
            with open(os.path.join(a.dump, name + ".txt"), "w") as f:
                f.write(text)
        return 0
    got = {name: digest(text) for name, text in traces.items()}
    if a.check:
        with open(JSON) as f:
            want = json.load(f)
        bad = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
        for name in enqueue_recorder.FULL_TEXT:
            with open(text_path(name)) as f:
                if f.read() != traces[name]:
                    bad.append(name + " (full text)")
        print("engine: %s" % os.path.dirname(mgr_amd.__file__))
        print("%d cases, %d differ%s" % (len(got), len(bad), ": " + ", ".join(bad) if bad else ""))
        return 1 if bad else 0
    with open(JSON, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    for name in enqueue_recorder.FULL_TEXT:
        with open(text_path(name), "w") as f:
            f.write(traces[name])
    return 0


if __name__ == "__main__":
    sys.exit(main())
