"""The fp64 restatements of tests/occupancy_ref.py and tests/overlap_ref.py against first principles, the host arithmetic of the Jaccard
index, and the timed MLF round trip (no GPU)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as ar  # noqa: E402
import occupancy_ref as oc  # noqa: E402
import overlap_ref as ov  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import keras_ref as kr  # noqa: E402

from mgr_amd import decoding  # noqa: E402


@pytest.mark.parametrize("labels", [[], [0], [1], [0, 1], [1, 1], [0, 1, 0], [1, 1, 0]])
@pytest.mark.parametrize("T", [3, 6])
def test_gamma_equals_enumeration_of_every_alignment(labels, T):
    rng = np.random.default_rng(10 * T + len(labels))
    Cn, blank = 3, 2
    P = rng.dirichlet(np.full(Cn, 0.7), size=T).astype(np.float32)
    logy = ar.log_emissions(P, skip=0)
    brute, tot = oc.brute_force_gamma(logy, labels, blank)
    g, logp = oc.forward_backward(logy, labels, blank)
    if brute is None:                       # ([1, 1, 0] needs four frames)
        assert g is None and logp == -np.inf and T == 3
        return
    assert abs(logp - np.log(tot)) <= 1e-12 * max(1.0, abs(logp))
    assert np.abs(g - brute).max() <= 1e-12
    assert np.abs(g.sum(axis=1) - 1.0).max() <= 1e-12


def test_class_sums_equal_the_oracle_gradient():
    """The oracle's CTC gradient is y - (per-class sums of gamma) chained through log(P + eps) and the softmax: undo the chain."""
    rng = np.random.default_rng(3)
    T, Cn, skip = 19, 5, 2
    labels = [1, 1, 0, 3, 2]
    P = rng.dirichlet(np.full(Cn, 0.6), size=T)
    P32 = P.astype(np.float32)
    P = P32.astype(np.float64)
    eps = np.float64(np.float32(1e-8))
    _, dz = kr.ctc_loss_grad(P[None], np.asarray([labels]), [T - skip], [len(labels)], skip=skip, eps=eps)
    Pp, dz = P[skip:], dz[0, skip:]
    u = Pp + eps
    h = dz / Pp                               # = gP - sum_c P gP, and sum_c u gP = sum_c du = 0 fixes the constant
    k = -(u * h).sum(axis=1, keepdims=True) / u.sum(axis=1, keepdims=True)
    du = u * (h + k)
    occ_oracle = u / u.sum(axis=1, keepdims=True) - du
    res = oc.occupancy(P32, labels, q=0.5, skip=skip)
    ext = ar.extended(labels, Cn - 1)
    occ = np.zeros((T - skip, Cn))
    np.add.at(occ.T, ext, res["gamma"].T)
    assert np.abs(occ - occ_oracle).max() <= 1e-9


@pytest.mark.parametrize("q", [0.5, 0.2, 0.05])
def test_extents_are_ordered(q):
    rng = np.random.default_rng(int(q * 100))
    for trial in range(40):
        Cn = int(rng.integers(3, 7))
        L = int(rng.integers(1, 6))
        T = int(rng.integers(2 * L + 1, 40))
        labels = [int(v) for v in rng.integers(0, Cn - 1, L)]
        P = rng.dirichlet(np.full(Cn, float(rng.choice([0.1, 0.5, 2.0]))), size=T).astype(np.float32)
        res = oc.occupancy(P, labels, q=q, skip=0)
        seg = res["seg"]
        assert all(0 <= f <= l < T for f, l in seg), (trial, seg)
        assert all(seg[i][0] < seg[i + 1][0] for i in range(L - 1)), (trial, seg)


def test_planted_extents_at_the_median():
    rng = np.random.default_rng(5)
    Cn, blank, skip = 6, 5, 2
    for labels in ([0], [3, 3], [1, 2, 2, 0], [4, 0, 1, 1, 1, 3]):
        states = ar.planted_alignment(rng, 60, labels, blank)
        P = ar.planted_posteriors(states, labels, blank, Cn, skip=skip, hi=0.999)
        planted = ar.states_to_segments(states, len(labels), skip)
        res = oc.occupancy(P, labels, q=0.5, skip=skip)
        _, vit = ar.viterbi(ar.log_emissions(P, skip), labels, blank)
        assert res["seg"] == planted == ar.states_to_segments(vit, len(labels), skip)
        g32 = res["gamma"].astype(np.float32)
        assert oc.extents_from_gamma(g32, 0.5, len(labels), skip) == planted


def test_does_not_fit_and_empty():
    P = np.full((5, 3), 1.0 / 3, np.float32)
    res = oc.occupancy(P, [1, 1], skip=2)              # three frames: label, blank, label fits exactly
    assert np.isfinite(res["logp"]) and res["seg"] == [(2, 2), (4, 4)]
    res = oc.occupancy(P, [1, 1], input_len=2, skip=2)
    assert res["logp"] == -np.inf and res["seg"] == [(-1, -1)] * 2 and not res["gamma"].any()
    res = oc.occupancy(P, [], skip=2)
    assert res["seg"] == [] and np.all(res["gamma"][:, 0] == 1.0)


# ---- overlap and the Jaccard index: hand-worked cases ---------------------------------------------------------------------------
HAND = ov.HAND


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_overlap_ref_hand_worked(case):
    _, hyp, ref, Cn, n, ignore, inter, union, hf, rf = case
    got = ov.overlap([hyp], [ref], Cn, n, ignore)
    assert [list(a[0]) for a in got] == [inter, union, hf, rf]


def test_jaccard_host_arithmetic():
    by = {c[0]: c for c in HAND}

    def jac(name, fp):
        c = by[name]
        return decoding.jaccard_from_counts(*[np.asarray([v], np.int32) for v in c[6:10]], false_positives=fp)
    assert jac("disjoint", True)["jaccard"] == 0.0
    assert jac("nested", True)["jaccard"] == 2 / 6
    assert jac("same class united", False)["jaccard"] == 0.5
    assert jac("class only in the hypothesis", False)["jaccard"] == 1.0        # the extra class does not count ...
    assert jac("class only in the hypothesis", True)["jaccard"] == 0.5         # ... or counts as a class that scored 0
    assert jac("ignored class", True)["jaccard"] == 1.0
    assert jac("clipped at n_frames", True)["jaccard"] == 2 / 5
    r = jac("empty reference", False)
    assert np.isnan(r["jaccard"]) and np.isnan(r["per_sample"][0])             # nothing to average over
    assert jac("empty reference", True)["jaccard"] == 0.0
    # two samples, one without classes: left out of the mean
    inter = np.asarray([[3, 0], [0, 0]])
    union = np.asarray([[4, 0], [0, 0]])
    r = decoding.jaccard_from_counts(inter, union, inter, union, false_positives=True)
    assert r["jaccard"] == 0.75 and np.isnan(r["per_sample"][1]) and r["per_class"][0] == 0.75 and np.isnan(r["per_class"][1])
    assert r["inter"].dtype == np.int64 and r["per_sample"].dtype == np.float64


def test_pack_segments_and_new_names():
    lab, seg = decoding.pack_segments([[(3, 1, 2, 0.5, 1.5), (4, 5, 9)], []])
    assert lab.tolist() == [[3, 4], [-1, -1]] and seg.tolist() == [[[1, 2], [5, 9]], [[-1, -1], [-1, -1]]]
    op = decoding.occupancy_op(22, 2, quantile=0.2, return_gamma=True)
    shapes = op.outputs(3, 12, 4)
    assert shapes[0] == ((3, 10, 9), np.float32) and shapes[1] == ((3, 4, 2), np.int32) and shapes[4] == ((3,), np.float64)
    assert decoding.occupancy_op(22, 2).outputs(3, 12, 4)[0] is None
    for q in (0.0, 0.51, -1):
        with pytest.raises(ValueError):
            decoding.occupancy_op(22, 2, quantile=q)
    with pytest.raises(ValueError):
        decoding.segment_overlap([[]], [[]], 65, 10)


def test_timed_mlf_round_trip(tmp_path):
    segs = [[(0, 2, 5, 0.9, 3.2), (1, 9, 9, 0.8, 1.0)], [(1, 0, 40, 0.7, 39.0)], [(0, 1, 2, 1.0, 1.0)]]
    names = [["wave", "point"], ["point"], ["wave"]]
    path = str(tmp_path / "rec.mlf")
    decoding.write_mlf(path, names, [1, 2, 3], ignore_list=[3], segments=segs)
    back = decoding.read_mlf_segments(path)
    assert back == {"Sample00001": [("wave", 2, 5), ("point", 9, 9)], "Sample00002": [("point", 0, 40)]}
    assert decoding.read_mlf(path) == {"Sample00001": ["wave", "point"], "Sample00002": ["point"]}
    plain = str(tmp_path / "plain.mlf")
    decoding.write_mlf(plain, names, [1, 2, 3], ignore_list=[])
    with pytest.raises(ValueError):
        decoding.read_mlf_segments(plain)
