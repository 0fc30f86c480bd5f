"""Rescoring off the GPU: the fp64 restatement (tests/rescore_ref.py) against plain enumeration and against the oracle's CTC loss, the
host functions of decoding.py against it, the workspace query against its closed formula, and the margins of the planted ranking
cases the GPU tests rank without allowance."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import align_ref as ar  # noqa: E402
import rescore_cases as rc  # noqa: E402
import rescore_ref as rr  # noqa: E402
from oracle import keras_ref as kr  # noqa: E402


def _close(a, b, rel=1e-12):
    return (a == b) if not (np.isfinite(a) and np.isfinite(b)) else abs(a - b) <= rel * max(abs(b), 1e-300)


def test_restatement_equals_enumeration():
    """The forward recursion is the sum over ALL C^T frame paths that collapse to the labels, to 1e-12 relative, at T <= 6, C <= 3 -
    the empty sequence, repeated labels, sequences that do not fit (-inf on both sides) and every position of the blank included."""
    n, dead = 0, 0
    for case in range(90):
        rng = np.random.default_rng(case)
        Cn, T = 2 + case % 2, 1 + case % 6
        blank = case % Cn
        logy = ar.log_emissions(rng.dirichlet(np.full(Cn, 0.6), size=T).astype(np.float32), 0, 1e-8)
        others = [c for c in range(Cn) if c != blank]
        for L in range(0, 4):
            labels = [int(v) for v in rng.choice(others, size=L)]
            got, want = rr.forward(logy, labels, blank), rr.enumerate_logp(logy, labels, blank)
            assert _close(got, want), (case, labels, got, want)
            assert (want == -np.inf) == (rr.needs(labels) > T)
            n += 1
            dead += want == -np.inf
    assert n == 360 and 30 < dead < 200
    assert rr.forward(np.zeros((0, 3)), [], 2) == 0.0 and rr.forward(np.zeros((0, 3)), [1], 2) == -np.inf


def test_restatement_equals_the_oracles_ctc_loss():
    """... and minus oracle.keras_ref.ctc_loss_grad's loss (run in fp64 on the same float32 inputs) to 1e-12 relative.  eps = 2^-27 is
    the same number in float32 and in fp64, so both sides add the same eps."""
    eps = 2.0 ** -27
    for case in range(12):
        rng = np.random.default_rng(100 + case)
        B, T, Cn, Lmax, skip = 3, int(rng.integers(8, 40)), int(rng.integers(3, 9)), 6, case % 3
        P = rng.dirichlet(np.full(Cn, 0.4), size=(B, T)).astype(np.float32)
        labels = rng.integers(0, Cn - 1, size=(B, Lmax))
        ll = rng.integers(0, Lmax + 1, size=B)
        il = rng.integers(2 * Lmax + 1, T - skip + 1, size=B) if T - skip > 2 * Lmax + 1 else np.full(B, T - skip)
        loss, _ = kr.ctc_loss_grad(P.astype(np.float64), labels, il, ll, skip=skip, eps=eps, need_grad=False)
        for b in range(B):
            got, _ = rr.score_slot(P[b], [int(v) for v in labels[b, :ll[b]]], Cn - 1, skip, eps, il[b])
            assert _close(got, -float(loss[b])), (case, b, got, -loss[b])


def test_slot_conventions_of_the_restatement():
    rng = np.random.default_rng(5)
    P = rng.dirichlet(np.full(5, 0.5), size=10).astype(np.float32)
    lex = [[0, 1], [1]]
    assert rr.score_slot(P, None, 4) == (-np.inf, -1)
    assert rr.score_slot(P, [0, 2], 4, lexicon=lex)[1] == -1 and np.isnan(rr.score_slot(P, [0, 2], 4, lexicon=lex)[0])
    assert rr.score_slot(P, [0, 1, 1], 4, lexicon=lex)[1] == 4
    lp, n = rr.score_slot(P, [0] * 256, 4, input_len=8)
    assert np.isnan(lp) and n == 256
    assert rr.score_slot(P, [1, 1, 1, 1, 1], 4, input_len=8) == (-np.inf, 5)          # 5 labels + 4 forced blanks > 8 frames
    assert rr.score_slot(P, [], 4, input_len=0) == (0.0, 0) and rr.score_slot(P, [1], 4, input_len=-3) == (-np.inf, 1)
    logy = ar.log_emissions(P, 2, 1e-8)
    assert abs(rr.score_slot(P, [], 4)[0] - logy[:, 4].sum()) < 1e-12
    assert rr.score_slot(P, [7, -2], 4)[0] == rr.score_slot(P, [4, 0], 4)[0]           # clipped into the class range


def test_pack_nbest():
    from mgr_amd import decoding
    paths = [[[1, 2, 3], [4]], [], [[], [5, 5]]]
    hyp, hl = decoding.pack_nbest(paths)
    assert hyp.dtype == np.int32 and hl.dtype == np.int32 and hyp.shape == (3, 2, 3)
    assert hl.tolist() == [[3, 1], [-1, -1], [0, 2]]
    assert hyp[0].tolist() == [[1, 2, 3], [4, -1, -1]] and hyp[2].tolist() == [[-1, -1, -1], [5, 5, -1]]
    hyp, hl = decoding.pack_nbest(paths, K=4, width=7)
    assert hyp.shape == (3, 4, 7) and hl[:, 2:].tolist() == [[-1, -1]] * 3
    want = rc.pack([[[1, 2, 3], [4], None, None], [None] * 4, [[], [5, 5], None, None]], 4, 7)
    assert np.array_equal(hyp, want[0]) and np.array_equal(hl, want[1])
    assert decoding.pack_nbest([[]])[0].shape == (1, 1, 1)
    for kw in ({"K": 1}, {"width": 2}, {"width": 1 << 20}):
        with pytest.raises(ValueError):
            decoding.pack_nbest(paths, **kw)


def test_pool_hypotheses():
    from mgr_amd import decoding
    a = [[[1, 2], [3], [1, 2]], [[4]], []]
    b = [[[3], [5]], [[4], []], [[6]]]
    c = [[[5], [1]], [[7]], [[6], [6, 6]]]
    for lists, cap in (((a,), None), ((a, b), None), ((a, b, c), None), ((a, b, c), 2), ((b, a), 1)):
        assert decoding.pool_hypotheses(*lists, cap=cap) == rr.pool(*lists, cap=cap)
    assert decoding.pool_hypotheses(a, b, c) == [[[1, 2], [3], [5], [1]], [[4], [], [7]], [[6], [6, 6]]]
    assert decoding.pool_hypotheses(a, b, c, cap=2)[0] == [[1, 2], [3]]
    with pytest.raises(ValueError):
        decoding.pool_hypotheses(a, b[:2])


def test_combine_scores_against_the_restatement():
    """Random parts with ties, -inf and NaN entries, short pools, a bigram with forbidden entries, zero weights."""
    from mgr_amd import decoding
    G = 5
    for case in range(40):
        rng = np.random.default_rng(300 + case)
        N, K, M = 4, 6, 1 + case % 3
        paths = [[[int(v) for v in rng.integers(0, G, int(rng.integers(0, 4)))] for _ in range(int(rng.integers(0, K + 1)))] for _ in range(N)]
        parts = np.round(rng.normal(-20, 5, size=(N, K, M)), 0 if case % 2 else 6)       # (rounded to integers: many exact ties)
        parts[rng.random(parts.shape) < 0.1] = -np.inf
        parts[rng.random(parts.shape) < 0.05] = np.nan
        w = rng.choice([0.0, 0.5, 1.0, 2.0], size=M)
        lm = lm_end = None
        if case % 4 >= 2:
            lm = np.where(rng.random((G + 1, G)) < 0.2, -np.inf, np.round(rng.normal(-2, 1, size=(G + 1, G))))
            lm_end = np.where(rng.random(G + 1) < 0.2, -np.inf, np.round(rng.normal(-2, 1, size=G + 1))) if case % 4 == 3 else None
        alpha, beta = (0.5, 1.0) if case % 3 else (1.0, 0.0)
        order, total = decoding.combine_scores(parts, paths, w, lm, lm_end, alpha, beta)
        worder, wtotal = rr.combine(parts, paths, w, lm, lm_end, alpha, beta)
        assert order.shape == (N, K) and np.array_equal(order, worder), case
        assert np.allclose(total, wtotal, rtol=1e-13, atol=0, equal_nan=True)
        for b in range(N):
            fin = np.isfinite(total[b])
            assert not fin[np.argmin(fin):].any() or fin.all()                       # everything not finite comes last ...
            assert list(order[b, ~fin]) == sorted(order[b, ~fin])                     # ... in pool order
            assert np.all(np.diff(total[b, fin]) <= 0)
            ties = np.flatnonzero(np.diff(total[b, fin]) == 0)
            assert np.all(order[b, ties] < order[b, ties + 1])                        # ties go to pool order
            assert set(order[b]) == set(range(K))
    # a forbidden transition: -inf whatever alpha is; an absent slot: -inf whatever its parts hold
    lm = np.zeros((G + 1, G))
    lm[2, 3] = -np.inf
    order, total = decoding.combine_scores(np.zeros((1, 3, 1)), [[[1, 3], [3, 1]]], None, lm, None, alpha=0.0)
    assert order.tolist() == [[1, 0, 2]] and total.tolist() == [[0.0, -np.inf, -np.inf]]
    with pytest.raises(ValueError):
        decoding.combine_scores(np.zeros((1, 2, 1)), [[[1], [2], [3]]])
    with pytest.raises(ValueError):
        decoding.combine_scores(np.zeros((1, 2, 2)), [[[1]]], weights=[1.0])


def test_rescore_nbest_with_scores_computed_elsewhere():
    """rescore_nbest on (N, K) score arrays involves no GPU: ranked paths, totals and parts are the restatement's, in the shapes
    mbr_decode / nbest_attainable take (per sample the present hypotheses best first, total[b, :len] their scores)."""
    from mgr_amd import decoding
    paths = [[[1], [2, 3], [4]], [[5]], []]
    s0 = np.array([[-3.0, -1.0, -2.0], [-1.0, -np.inf, -np.inf], [-np.inf] * 3])
    s1 = np.array([[-1.0, -4.0, -1.5], [-2.0, -np.inf, -np.inf], [-np.inf] * 3])
    ranked, total, parts, order = decoding.rescore_nbest([(s0, None), (s1, {})], paths, weights=(1.0, 0.5))
    worder, wtotal = rr.combine(np.stack([s0, s1], axis=2), paths, (1.0, 0.5))
    assert np.array_equal(order, worder) and np.array_equal(total, wtotal)
    assert total[0].tolist() == [-2.75, -3.0, -3.5]
    assert ranked == [[[4], [2, 3], [1]], [[5]], []] and order[0].tolist() == [2, 1, 0]
    assert parts.shape == (3, 3, 2) and parts[0, :, 0].tolist() == [-2.0, -1.0, -3.0]
    with pytest.raises(ValueError):
        decoding.rescore_nbest([(s0[:, :2], None)], paths)


def test_workspace_query_is_the_documented_layout():
    """mgr_ctc_rescore_ws_bytes (a pure host function: no GPU needed) against the layout stated in csrc/rescore.hip: the emission rows
    only, B * C * TS floats with TS = T + 16 rounded up to 4, padded to 256 bytes - with and without a lexicon, which changes nothing
    (hypotheses are expanded in LDS).  The query takes the lexicon's offsets, so it is not one of the scalar queries
    tests/golden/ws_bytes.json records; this grid pins it instead."""
    from mgr_amd import _capi
    fn = _capi.load_library().mgr_ctc_rescore_ws_bytes
    pad = lambda n: (4 * n + 255) // 256 * 256
    rows = 0
    for B, T, Cn, G in itertools.product((1, 2, 3, 16, 17, 64), (1, 31, 32, 33, 40, 200, 1900), (2, 5, 22, 44, 64), (0, 1, 21, 64)):
        want = pad(B * Cn * ((T + 16 + 3) // 4 * 4))
        off = np.arange(G + 1, dtype=np.int32)
        assert int(fn(B, T, Cn, G, off.ctypes.data if G else None)) == want, (B, T, Cn, G)
        rows += 1
    assert rows >= 800
    off = np.asarray([0, 1, 2, 4, 5, 8, 11, 13, 15, 17, 19, 24, 25, 28, 29, 32, 36, 38, 41, 42, 46, 48], np.int32)
    assert int(fn(64, 1900, 44, 21, off.ctypes.data)) == int(fn(64, 1900, 44, 0, None)) == 64 * 44 * 1916 * 4       # 21.6 MB


def test_planted_ranking_cases_have_their_margins():
    """On every planted ranking case the GPU test ranks: each stream alone prefers the pool's substitution on its own sample, the
    weighted sum prefers the truth wherever the bigram allows it, and neighbouring fp64 totals - best against second, and every further
    pair of finite neighbours - lie at least 1e-3 of |best| apart: an f32-accurate kernel (1e-7 relative) cannot flip the order."""
    n = 0
    for case in rc.ranking_cases():
        order, total, parts = rc.reference_ranking(case)
        wrong0, wrong1 = case["wrong"]
        assert wrong0 != wrong1
        forbidden = []
        for b, hyps in enumerate(case["paths"]):
            assert len(hyps) == 4 and len(set(map(tuple, hyps))) == 4
            t, s = case["truth"][b], case["sub"][b]
            for m, wb in enumerate(case["wrong"]):
                alone = int(np.argmax(parts[b, :, m]))
                assert alone == (s if b == wb else t), (case["name"], b, m)
            lt = rr.lm_term(hyps[t], case["lm"], case["lm_end"])
            if lt == -np.inf:
                forbidden.append(b)
                assert order[b, -1] == t or total[b, list(order[b]).index(t)] == -np.inf
                assert list(order[b]).index(t) >= int(np.isfinite(total[b]).sum())
            else:
                assert order[b, 0] == t, (case["name"], b)
            fin = total[b][np.isfinite(total[b])]
            assert len(fin) >= 2
            gaps = -np.diff(fin)
            print("%s sample %d: best %.4f, gaps %s" % (case["name"], b, fin[0], np.round(gaps, 4)))
            assert gaps.min() >= rc.MARGIN * abs(fin[0]), (case["name"], b, fin)
            n += 1
        assert (forbidden == [0]) == (case["lm"] is not None) and (case["lm"] is not None or not forbidden)
    assert n == 12
