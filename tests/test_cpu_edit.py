"""The scoring reference (tests/edit_ref.py) against exhaustive enumeration and the existing host edit distances, the form the
kernel computes in against that reference, and the host arithmetic of decoding.score_sequences / nbest_attainable / mbr_decode with
the device call replaced by the reference.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as br  # noqa: E402
import edit_ref as er  # noqa: E402

ASYM = (5, 2, 9)      # catches a swapped deletion / insertion


def random_pairs(seed, count, n_labels, max_len):
    rng = np.random.default_rng(seed)
    return [([int(v) for v in rng.integers(0, n_labels, int(rng.integers(0, max_len + 1)))],
             [int(v) for v in rng.integers(0, n_labels, int(rng.integers(0, max_len + 1)))]) for _ in range(count)]


def ref_edit_distances(hyps, refs, pairs=None, costs=(1, 1, 1), ignore=(), return_ops=False, dev=None):
    """decoding.edit_distances with tests/edit_ref.py where the device call is."""
    from mgr_amd import decoding
    costs = decoding.check_costs(costs)
    mask = decoding.ignore_mask(ignore)
    h, _ = decoding.pack_labels(hyps)
    r, _ = decoding.pack_labels(refs)
    pr = None if pairs is None else np.asarray(pairs, np.int64).reshape(-1, 2)
    if pr is None and h.shape[0] != r.shape[0]:
        raise ValueError("%d hypotheses for %d references" % (h.shape[0], r.shape[0]))
    if pr is not None and len(pr) and (pr.min() < 0 or pr[:, 0].max() >= h.shape[0] or pr[:, 1].max() >= r.shape[0]):
        raise IndexError("pair index out of range")
    dist, counts, lens, n_ops, ops = er.kernel_ref(h, None, r, None, None if pr is None else pr[:, 0], None if pr is None else pr[:, 1],
                                                   costs, mask)
    res = (dist, counts, lens)
    return res + ([ops[p, :n_ops[p]].copy() for p in range(len(dist))],) if return_ops else res


@pytest.fixture
def host_scoring(monkeypatch):
    from mgr_amd import decoding
    monkeypatch.setattr(decoding, "edit_distances", ref_edit_distances)
    return decoding


# ---- the N-best inputs the GPU test shares (tests/test_gpu_edit.py) ----------------------------------------------------------------
NBEST_SHAPE = (4, 50, 22, 10, 10)      # (N, T, C, W, top_paths)
MBR_SCALES = (1.0, 0.25)
_NBEST = {}


def nbest_case():
    """Posteriors, input lengths, a random bigram table (without one the 1-best of these posteriors is also the lists' medoid and
    the minimum-Bayes-risk pick never leaves it), reference labels and the fp64 reference's N-best lists (seqs, score, logp_ctc,
    gap)."""
    if not _NBEST:
        N, T, Cn, W, NP = NBEST_SHAPE
        rng = np.random.default_rng(2013)
        P = rng.dirichlet(0.3 * np.ones(Cn), size=(N, T)).astype(np.float32)
        il = np.array([T - 2, T - 9, T - 2, 30])
        ext, fin = 0.5 * rng.standard_normal((Cn + 1, Cn)), 0.5 * rng.standard_normal(Cn + 1)
        refs = [[int(v) for v in rng.integers(0, Cn - 1, int(rng.integers(8, 20)))] for _ in range(N)]
        _NBEST.update(P=P, il=il, ext=ext, fin=fin, refs=refs, nbest=br.beam_search_lm(P, il, ext, fin, W, NP))
    return _NBEST


def test_tuple_dp_equals_enumeration():
    n = 0
    for costs in er.COST_SETS + [ASYM]:
        for h, r in random_pairs(11, 250, 3, 5):
            best = er.enumerate_best(h, r, costs)
            c, (H, S, D, I), ops = er.align(h, r, costs)
            assert (c, S, D, I) == best and H == len(r) - S - D
            n += 1
    assert n == 1000


def test_unit_costs_equal_the_existing_edit_distances():
    from mgr_amd import decoding
    from oracle import keras_ref as kr
    for h, r in random_pairs(12, 300, 4, 12):
        c, (H, S, D, I), _ = er.align(h, r, (1, 1, 1))
        assert c == decoding.edit_distance(h, r) == kr.edit_distance(h, r) == S + D + I


def test_weighted_alignment_is_not_the_levenshtein_alignment():
    """Why the costs are a parameter: S + D + I of the min-cost (10, 7, 7) alignment exceeds the Levenshtein distance on some pairs."""
    diff = sum(sum(er.align(h, r, (10, 7, 7))[1][1:]) != er.align(h, r, (1, 1, 1))[0] for h, r in random_pairs(13, 3000, 3, 5))
    assert diff > 0


def test_replaying_ops_consumes_both_and_reproduces_the_counts():
    for costs in er.COST_SETS + [ASYM]:
        for h, r in random_pairs(14, 200, 3, 9):
            c, cnt, ops = er.align(h, r, costs)
            ok, cost, got = er.replay(h, r, ops, costs)
            assert ok and cost == c and got == cnt and len(ops) == sum(cnt)


@pytest.mark.parametrize("n", [0, 1, 15, 16, 63, 64, 65, 150])
def test_packed_prefix_min_form_equals_the_tuple_dp(n):
    """The kernel's form (edit_ref.packed_form: packed keys, rows relative to j * K_del, two passes and a lane scan) gives the tuple
    DP's result and the tie rule's alignment, at the lane boundaries of the column split and with alphabets that make ties common."""
    rng = np.random.default_rng(100 + n)
    for costs in er.COST_SETS + [ASYM]:
        for m in (0, 1, 2, 40, 70):
            for A in (2, 5):
                h, r = [int(v) for v in rng.integers(0, A, m)], [int(v) for v in rng.integers(0, A, n)]
                assert er.packed_form(h, r, costs) == er.align(h, r, costs)


def test_packed_form_at_the_limits_cannot_overflow():
    """4095 labels a side at the largest costs: cost < 2^27, every count fits 12 bits, the packed key stays below 2^63 (and the
    relative form above -2^63)."""
    L, Cmax = 4095, 16384
    assert 2 * L * Cmax < 1 << 27
    assert (((2 * L * Cmax) << 36) | (L << 24) | (L << 12) | L) < (1 << 63)
    assert -(L + 64) * ((Cmax << 36) | (1 << 12)) - ((Cmax << 36) | (1 << 12)) > -(1 << 63)


def test_filter_semantics():
    row = [3, -1, 0, 5, 63, 64, 2, -7, 5]
    assert er.filter_row(row) == [3, 0, 5, 63, 64, 2, 5]
    assert er.filter_row(row, 4) == [3, 0, 5] and er.filter_row(row, 0) == [] and er.filter_row(row, -3) == []
    assert er.filter_row(row, 99) == er.filter_row(row)
    assert er.filter_row(row, None, (1 << 0) | (1 << 5) | (1 << 63)) == [3, 64, 2]
    hyp = np.array([[1, -1, 2, 21, 3], [4, 4, -1, -1, -1]])
    ref = np.array([[1, 2, 3], [21, 4, -1]])
    dist, counts, lens, n_ops, ops = er.kernel_ref(hyp, [5, 1], ref, None, [0, 1, 1], [0, 1, 0], (1, 1, 1), 1 << 21)
    assert lens.tolist() == [[3, 3], [1, 1], [1, 3]] and dist.tolist() == [0, 0, 3]
    assert counts.tolist() == [[3, 0, 0, 0], [1, 0, 0, 0], [0, 1, 2, 0]] and n_ops.tolist() == [3, 1, 3]
    assert ops[2].tolist() == [2, 2, 1, -1, -1, -1, -1, -1]      # the diagonal is tried first on the way BACK: the substitution comes last


def test_score_sequences_and_confusion_by_hand(host_scoring):
    d = host_scoring
    hyps = [[1, 2, 3], [4], [], [2, 2, 5]]
    refs = [[1, 3], [4, 0], [1], [2, 5]]
    s = d.score_sequences(hyps, refs, confusion=True, n_classes=6)
    # [1 2 3] / [1 3]: one insertion; [4] / [4 0]: one deletion; [] / [1]: one deletion; [2 2 5] / [2 5]: one insertion
    assert (s["H"], s["S"], s["D"], s["I"], s["N"]) == (5, 0, 2, 2, 7)
    assert s["ler"] == 4 / 7 and s["corr"] == 5 / 7 and s["acc"] == 3 / 7 and s["dist_sum"] == 4
    assert s["per_sample"]["dist"].tolist() == [1, 1, 1, 1] and s["per_sample"]["lens"].tolist() == [[3, 2], [1, 2], [0, 1], [3, 2]]
    conf = s["confusion"]
    assert conf.shape == (7, 7) and conf.sum() == 5 + 2 + 2
    assert conf[1, 1] == 1 and conf[3, 3] == 1 and conf[4, 4] == 1 and conf[2, 2] == 1 and conf[5, 5] == 1
    assert conf[0, 6] == 1 and conf[1, 6] == 1 and conf[6, 2] == 2 and conf[6, 6] == 0
    # a substitution lands off the diagonal; the ignored label is gone from both sides
    s = d.score_sequences([[1, 9, 2]], [[9, 1, 3, 9]], ignore=(9,), confusion=True, n_classes=10, costs=d.HTK_COSTS)
    assert (s["H"], s["S"], s["D"], s["I"], s["N"]) == (1, 1, 0, 0, 2) and s["confusion"][3, 2] == 1 and s["dist_sum"] == 10
    assert d.score_sequences([], [])["ler"] == 0.0
    with pytest.raises(ValueError):
        d.score_sequences([[1]], [[1]], costs=(0, 1, 1))
    with pytest.raises(ValueError):
        d.score_sequences([[1]], [[1]], costs=(1, 1, 16385))
    with pytest.raises(ValueError):
        d.score_sequences([[1]], [[1]], ignore=(64,))
    with pytest.raises(ValueError):
        d.score_sequences([[1]], [[1], [2]])
    with pytest.raises(IndexError):
        d.edit_distances([[1]], [[1]], pairs=[(0, 1)])


def test_score_mlf_counts(host_scoring, tmp_path):
    d = host_scoring
    d.write_mlf(str(tmp_path / "ref.mlf"), [["sil", "a", "b", "sil"], ["c"]], [1, 2], [])
    d.write_mlf(str(tmp_path / "rec.mlf"), [["a", "sil", "c", "b"], ["sil"]], [1, 2], [])
    s = d.score_mlf_counts(str(tmp_path / "ref.mlf"), str(tmp_path / "rec.mlf"))
    assert (s["H"], s["S"], s["D"], s["I"], s["N"], s["n_samples"]) == (2, 0, 1, 1, 3, 2) and s["names"] == ["a", "b", "c"]
    assert s["ler"] == d.score_mlf(str(tmp_path / "ref.mlf"), str(tmp_path / "rec.mlf"))[0]


def test_mbr_leaves_the_one_best_on_the_planted_case(host_scoring):
    d = host_scoring
    paths = [[[5], [1, 2], [1, 2, 3]], [[7, 7]], []]
    w = np.array([0.4, 0.3, 0.3])
    scores = np.full((3, 3), -np.inf)
    scores[0] = np.log(w)
    scores[1, 0] = -3.0
    picks, ranks, risk = d.mbr_decode(paths, scores)
    assert picks == [[1, 2], [7, 7], []] and ranks.tolist() == [1, 0, -1]
    assert np.allclose(risk[0], [1.5, 1.1, 1.5], rtol=1e-12, atol=0) and risk[1].tolist() == [0.0, np.inf, np.inf]
    assert np.all(np.isinf(risk[2]))
    rp, rr, rrisk, gap = er.mbr_ref(paths, scores)
    assert rp == picks and rr.tolist() == ranks.tolist() and np.allclose(rrisk[0], risk[0], rtol=1e-12, atol=0)
    # a sharp posterior (large scale) returns the 1-best
    assert d.mbr_decode(paths, scores, scale=50.0)[1].tolist() == [0, 0, -1]


def test_nbest_attainable_by_hand(host_scoring):
    d = host_scoring
    paths = [[[1, 2], [1, 3], [1, 3, 4]], [[2], [2]], []]
    refs = [[1, 3, 4], [2, -1, -1], [5, 6, -1]]
    dist, rank, ler = d.nbest_attainable(paths, refs)
    assert dist.tolist() == [0, 0, 2] and rank.tolist() == [2, 0, -1] and ler == 2 / 6
    rd, rr, rl = er.nbest_attainable_ref(paths, refs)
    assert rd.tolist() == dist.tolist() and rr.tolist() == rank.tolist() and rl == ler


def test_the_shared_nbest_inputs_are_no_near_ties():
    """What tests/test_gpu_edit.py relies on: the fp64 search's own cuts are clear (the kernel returns the same lists), the lists are
    full, and no sample's two smallest risks are within 1e-9 (4 samples: 'at most 1 in 20' excuses none)."""
    case = nbest_case()
    seqs, score, logp, gap = case["nbest"]
    assert gap > 1e-9
    assert [len(s) for s in seqs] == [NBEST_SHAPE[4]] * NBEST_SHAPE[0]
    sc = np.asarray(score)
    for costs in ((1, 1, 1), (10, 7, 7)):
        for scale in MBR_SCALES:
            picks, ranks, risk, gaps = er.mbr_ref(seqs, sc, scale, costs)
            assert np.all(gaps > 1e-9), (costs, scale, gaps)
    # the pick leaves the 1-best somewhere, and depends on the scale: the comparison is about something
    assert np.any(er.mbr_ref(seqs, sc, MBR_SCALES[0])[1] != 0)
    assert not np.array_equal(er.mbr_ref(seqs, sc, MBR_SCALES[0])[1], er.mbr_ref(seqs, sc, MBR_SCALES[1])[1])
    d, r, ler = er.nbest_attainable_ref(seqs, case["refs"])
    assert np.all(r >= 0) and 0 < ler


def test_callbacks_treat_val_ler_as_smaller_is_better(tmp_path):
    from mgr_amd.keras_like import EarlyStopping, ModelCheckpoint

    class Saves:
        stop_training = False

        def __init__(self):
            self.saved = []

        def save_weights(self, path):
            self.saved.append(path)

    m = Saves()
    ck = ModelCheckpoint(str(tmp_path / "w{epoch:02d}.npz"), monitor="val_ler", save_best_only=True)
    ck.set_model(m)
    assert ck.sign == 1.0 and ModelCheckpoint("x", monitor="val_acc").sign == -1.0
    for epoch, ler in enumerate([0.5, 0.6, 0.4, 0.4]):
        ck.on_epoch_end(epoch, {"val_ler": ler, "val_loss": 1.0})
    assert [os.path.basename(p) for p in m.saved] == ["w01.npz", "w03.npz"]
    es = EarlyStopping(monitor="val_ler", patience=2)
    es.set_model(m)
    for epoch, ler in enumerate([0.5, 0.4, 0.45, 0.41]):
        assert not m.stop_training
        es.on_epoch_end(epoch, {"val_ler": ler})
    assert m.stop_training


def test_decode_score_of_the_decode_modules(host_scoring):
    from mgr_amd.audio_network import sequence_decoding as ad
    from mgr_amd.multimodal_fusion import sequence_decoding as sd
    s = sd.decode_score([[21, 3, 21, 4, 21]], [[3, 5]])          # "sil" (the blank, 21) is dropped; PF hit, FU for CP
    assert (s["H"], s["S"], s["D"], s["I"], s["N"], s["dist_sum"]) == (1, 1, 0, 0, 2, 10)
    assert s["confusion"].shape == (23, 23) and s["confusion"][5, 4] == 1 and s["confusion"][3, 3] == 1
    a = ad.decode_score([[43, 1, 2]], [[1, 2, 7]], confusion=False)
    assert (a["H"], a["D"], a["N"]) == (2, 1, 3) and "confusion" not in a
