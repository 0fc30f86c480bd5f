"""CPU: the label bigram (decoding.bigram_lm), the host-side tables, and the fp64 reference of the beam search with a bigram and an
N-best list (tests/beam_lm_ref.py) against exhaustive enumeration and against the oracle's search without tables."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as br  # noqa: E402
from mgr_amd import decoding  # noqa: E402
from oracle import keras_ref as kr  # noqa: E402

TINY = [(3, 5), (4, 3), (5, 3), (3, 4)]      # (C, T'): at most 31, 13, 21, 15 prefixes before the last frame - a beam of 32 never prunes there


def tiny_case(Cn, Tp, seed, with_inf):
    """One tiny sample (skip = 0) with random tables: ext ~ N(0, 1) (one entry -inf with with_inf), fin ~ N(0, 0.5)."""
    rng = np.random.default_rng(seed)
    P = rng.dirichlet(np.ones(Cn), size=Tp).astype(np.float32)
    ext = rng.standard_normal((Cn + 1, Cn))
    if with_inf:
        ext[1 + int(rng.integers(0, Cn - 1)), int(rng.integers(0, Cn - 1))] = -np.inf
    fin = 0.5 * rng.standard_normal(Cn + 1)
    return P, ext, fin


def check_tiny_inputs(ranked, pruned_order, n_top=8, keep=32):
    """What makes a tiny case a fair one, from the enumeration alone: the best n_top labellings are separated by more than 1e-9, and
    each of them is among the `keep` best by the score the search prunes with (fin takes no part in the pruning), by the same margin."""
    top = ranked[:n_top + 1]
    gaps = [a[1] - b[1] for a, b in zip(top, top[1:])]
    assert min(gaps) > 1e-9, gaps
    if len(pruned_order) > keep:
        kept = {e[0] for e in pruned_order[:keep]}
        assert all(e[0] in kept for e in ranked[:n_top])
        assert pruned_order[keep - 1][1] - pruned_order[keep][1] > 1e-9


def test_bigram_lm_counts_by_hand():
    seqs = [[0, 1, 2], [0, 1], [2, 0, 1, 1], []]
    Cn = 4                                   # labels 0..2, blank 3
    lm, lm_end = decoding.bigram_lm(seqs, Cn, add_k=0.0)
    assert lm.shape == (Cn + 1, Cn) and lm_end.shape == (Cn + 1,) and lm.dtype == np.float64
    # start: 0 twice, 2 once, end once (the empty sequence)
    assert np.allclose(np.exp(lm[0]), [2 / 4, 0, 1 / 4, 0]) and math.isclose(math.exp(lm_end[0]), 1 / 4)
    # after 0: 1 three times; after 1: 2 once, 1 once, end twice; after 2: 0 once, end once
    assert np.allclose(np.exp(lm[1]), [0, 1, 0, 0]) and lm_end[1] == -np.inf
    assert np.allclose(np.exp(lm[2]), [0, 1 / 4, 1 / 4, 0]) and math.isclose(math.exp(lm_end[2]), 2 / 4)
    assert np.allclose(np.exp(lm[3]), [1 / 2, 0, 0, 0]) and math.isclose(math.exp(lm_end[3]), 1 / 2)
    # -inf exactly where a transition was never seen; the row of a label that never occurs (the blank) is all -inf
    seen = np.zeros((Cn + 1, Cn), bool)
    for s in seqs:
        prev = 0
        for v in s:
            seen[prev, v] = True
            prev = v + 1
    assert np.array_equal(np.isneginf(lm), ~seen)
    assert np.all(np.isneginf(lm[4])) and lm_end[4] == -np.inf
    # add-k: every row sums to 1 with end, the blank column stays impossible, unseen transitions get k / (n + k * C)
    for k in (1.0, 0.25):
        lm, lm_end = decoding.bigram_lm(seqs, Cn, add_k=k)
        assert np.allclose(np.exp(lm).sum(axis=1) + np.exp(lm_end), 1.0, rtol=0, atol=1e-15)
        assert np.all(np.isneginf(lm[:, 3])) and np.all(np.isfinite(lm[:, :3])) and np.all(np.isfinite(lm_end))
        assert math.isclose(math.exp(lm[1, 0]), k / (3 + 4 * k)) and math.isclose(math.exp(lm[1, 1]), (3 + k) / (3 + 4 * k))
    # padded arrays (-1 or NaN padding) and lists agree; so does a generator
    pad = -np.ones((4, 4))
    for i, s in enumerate(seqs):
        pad[i, :len(s)] = s
    nanpad = np.where(pad < 0, np.nan, pad)
    want = decoding.bigram_lm(seqs, Cn, add_k=0.5)
    for other in (pad.astype(np.int32), pad, nanpad, (s for s in seqs)):
        got = decoding.bigram_lm(other, Cn, add_k=0.5)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(ValueError):
        decoding.bigram_lm([[0, 3]], Cn)     # the blank is no label


def test_lm_tables_scale_and_refuse():
    lm, lm_end = decoding.bigram_lm([[0, 1], [1]], 3, add_k=0.0)
    ext, fin = decoding.lm_tables(3, lm, lm_end, alpha=0.5, beta=0.25)
    fl = np.isfinite(lm)
    assert np.array_equal(np.isneginf(ext), ~fl) and np.array_equal(ext[fl], 0.5 * lm[fl] + 0.25)
    assert np.array_equal(fin[np.isfinite(lm_end)], 0.5 * lm_end[np.isfinite(lm_end)])
    ext0, fin0 = decoding.lm_tables(3, lm, None, alpha=0.0, beta=0.0)          # (0 * -inf must not turn into NaN)
    assert fin0 is None and np.array_equal(np.isneginf(ext0), ~fl) and np.all(ext0[fl] == 0.0)
    ext, fin = decoding.lm_tables(3, None, None, beta=1.5)
    assert fin is None and ext.shape == (4, 3) and np.all(ext == 1.5)
    bad = np.zeros((4, 3))
    bad[2, 1] = np.nan
    for args in ((bad, None), (np.zeros((4, 3)), np.array([0, np.nan, 0, 0])), (np.zeros((3, 3)), None), (np.full((4, 3), np.inf), None)):
        with pytest.raises(ValueError):
            decoding.lm_tables(3, *args)


@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("Cn,Tp", TINY)
def test_reference_equals_exhaustive_enumeration(Cn, Tp, with_inf):
    for seed in range(4):
        P, ext, fin = tiny_case(Cn, Tp, 100 * Cn + 10 * Tp + seed, with_inf)
        ranked, pruned_order = br.enumerate_labellings(P, ext, fin)
        check_tiny_inputs(ranked, pruned_order)
        seqs, score, logp, gap = br.beam_search_lm(P[None], [Tp], ext, fin, beam_width=32, top_paths=8, skip=0, eps=0.0)
        n = min(8, len(ranked))
        assert [tuple(s) for s in seqs[0]] == [e[0] for e in ranked[:n]]
        assert np.allclose(score[0], [e[1] for e in ranked[:n]], rtol=1e-12, atol=0)
        assert np.allclose(logp[0], [e[2] for e in ranked[:n]], rtol=1e-12, atol=0)
        if with_inf:
            p, c = [(int(a) - 1, int(b)) for a, b in zip(*np.nonzero(np.isneginf(ext)))][0]
            pairs = {(a, b) for s in seqs[0] for a, b in zip([-1] + s, s)}
            assert (p, c) not in pairs


@pytest.mark.parametrize("N,T,Cn,W", [(3, 60, 22, 10), (2, 40, 5, 4), (2, 30, 44, 16)])
def test_reference_with_zero_tables_is_the_oracle_search(N, T, Cn, W):
    rng = np.random.default_rng(7 * T + Cn)
    P = rng.dirichlet(0.3 * np.ones(Cn), size=(N, T)).astype(np.float32)
    il = np.array([T - 2] + [int(v) for v in rng.integers(T // 2, T - 2, N - 1)])
    for NP in (1, 3):
        want, wsc = kr.ctc_beam_search(P, il, beam_width=W, merge_repeated=False, top_paths=NP)
        for tables in ((None, None), (np.zeros((Cn + 1, Cn)), np.zeros(Cn + 1))):
            seqs, score, logp, gap = br.beam_search_lm(P, il, *tables, beam_width=W, top_paths=NP)
            assert gap > 1e-9
            if NP == 1:
                assert [s[0] for s in seqs] == want and [s[0] for s in score] == wsc
            else:
                assert seqs == want and score == wsc
            assert logp == score
