"""-m gpu: mgr_segment_overlap - per-class frame intersection / union counts - against the numpy frame masks of tests/overlap_ref.py
(exact integers: ==), on random segment sets and on the hand-worked cases of tests/overlap_ref.py, and jaccard_index on top of it.
The kernel takes a sample's frames in tiles of 256: n_frames is met one below, at and one above a tile and a wave (64)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap_ref as ov  # noqa: E402

from mgr_amd import decoding  # noqa: E402

pytestmark = pytest.mark.gpu


def _random_segments(rng, B, S, Cn, n):
    """Per sample up to S segments; some reach past n, some have a label outside [0, Cn) or a negative first frame, some are empty."""
    out = []
    for b in range(B):
        rows = []
        for k in range(int(rng.integers(0, S + 1)) if b else S):
            first = int(rng.integers(-2, n + 3))
            rows.append((int(rng.integers(-1, Cn + 1)), first, first + int(rng.integers(-1, max(2, n // 4)))))
        out.append(rows)
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1900])
@pytest.mark.parametrize("B,Sh,Sr,Cn", [(1, 1, 7, 1), (5, 7, 256, 21), (5, 256, 1, 64), (1, 256, 256, 64)])
def test_overlap_equals_frame_masks(device, n, B, Sh, Sr, Cn):
    rng = np.random.default_rng(n * 1000 + Sh + Cn)
    hyp, ref = _random_segments(rng, B, Sh, Cn, n), _random_segments(rng, B, Sr, Cn, n)
    nf = n if B == 1 else np.asarray([n, max(1, n // 2), n, 0, n][:B])
    ignore = () if Cn < 3 else (1, Cn - 1)
    got = decoding.segment_overlap(hyp, ref, Cn, nf, ignore=ignore, dev=device)
    want = ov.overlap(hyp, ref, Cn, nf, ignore)
    for g, w in zip(got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w)


@pytest.mark.parametrize("case", ov.HAND, ids=[c[0] for c in ov.HAND])
def test_overlap_hand_worked(device, case):
    _, hyp, ref, Cn, n, ignore, inter, union, hf, rf = case
    got = decoding.segment_overlap([hyp], [ref], Cn, n, ignore=ignore, dev=device)
    assert [list(a[0]) for a in got] == [inter, union, hf, rf]


def test_jaccard_index_and_mlf_score(device, tmp_path):
    hyp = [[(0, 0, 4, 0.9), (1, 5, 9, 0.8)], [(2, 0, 9, 0.5)], []]
    ref = [[(0, 0, 4), (1, 7, 9)], [(2, 5, 14)], []]
    r = decoding.jaccard_index(hyp, ref, 4, [10, 20, 10], dev=device)
    assert r["per_sample"][0] == (1.0 + 3 / 5) / 2 and r["per_sample"][1] == 5 / 15 and np.isnan(r["per_sample"][2])
    assert r["jaccard"] == ((1.0 + 3 / 5) / 2 + 5 / 15) / 2
    names = ["wave", "point", "stop", "sil"]
    to_names = lambda segs: [[names[s[0]] for s in row] for row in segs]
    rec_path, ref_path = str(tmp_path / "rec.mlf"), str(tmp_path / "ref.mlf")
    decoding.write_mlf(rec_path, to_names(hyp), [1, 2, 3], [], segments=hyp)
    decoding.write_mlf(ref_path, to_names(ref), [1, 2, 3], [], segments=ref)
    s = decoding.score_mlf_overlap(ref_path, rec_path, names, dev=device)
    assert s["n_samples"] == 3 and s["jaccard"] == r["jaccard"] and s["samples"] == ["Sample00001", "Sample00002", "Sample00003"]
