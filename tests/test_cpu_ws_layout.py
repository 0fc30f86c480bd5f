"""The mgr_*_ws_bytes queries against tests/golden/ws_bytes.json: the byte counts recorded from the library of the commit named in the
fixture (tests/golden/make_ws_bytes.py), before the workspace layouts moved into one layout function each.  The queries are pure host
functions, so the library answers them on a machine without a GPU."""
import json
import os

import pytest

import mgr_amd  # noqa: F401
from mgr_amd import _capi

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ws_bytes.json")) as _f:
    GOLDEN = json.load(_f)
QUERIES = sorted({name for name, _, _ in GOLDEN["rows"]})


def test_every_scalar_query_is_recorded():
    scalar = {n for n, (_, args) in _capi.SIGNATURES.items() if n.endswith("_ws_bytes") and _capi.vp not in args}
    assert scalar == set(QUERIES)
    assert len(GOLDEN["rows"]) >= 300


@pytest.mark.parametrize("name", QUERIES)
def test_ws_bytes_match_the_recorded_layouts(name):
    fn = getattr(_capi.load_library(), name)
    rows = [(args, want) for n, args, want in GOLDEN["rows"] if n == name]
    assert len(rows) >= 20
    wrong = [(args, want, got) for args, want in rows for got in [int(fn(*args))] if got != want]
    assert not wrong, "%s: %d of %d shapes differ from commit %s, e.g. (args, recorded, now) %s" % (
        name, len(wrong), len(rows), GOLDEN["commit"], wrong[:3])
