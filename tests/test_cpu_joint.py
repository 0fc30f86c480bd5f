"""No GPU: the fp64 restatement of the joint decode (tests/joint_ref.py, mgr_ctc_joint_decode's definition) against brute force over
all frame paths, its early stop against the search without one, the decision margins of every input the GPU tests use
(tests/joint_cases.py), the planted pool-miss case against the restatements of the shipped decoders, and the table semantics."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as br  # noqa: E402
import joint_cases as jc  # noqa: E402
import joint_ref as jr  # noqa: E402
import lexicon_ref as lr  # noqa: E402
import rescore_ref as rr  # noqa: E402

NEG = float("-inf")
_cache = {}


def decoded(case, early=True):
    """The restatement's result of a case, computed once per session."""
    key = (case["name"], early)
    if key not in _cache:
        _cache[key] = jr.decode_case(case, early)
    return _cache[key]


def close(a, b, tol):
    return (a == NEG and b == NEG) or abs(a - b) <= tol


def labelling_table(ly, blank):
    """ln p of every labelling of a tiny sample, from all C^T frame paths."""
    T, C = ly.shape
    tab = {}
    for path in itertools.product(range(C), repeat=T):
        lab = jr.collapse(path, blank)
        tab[lab] = jr.lse(tab.get(lab, NEG), float(sum(ly[t, c] for t, c in enumerate(path))))
    return tab


def test_recursion_equals_enumeration_of_all_frame_paths():
    """(a) ln p and ln psi of the chained extensions against brute force, T = 5, C = 3 (blank last)."""
    for seed in range(4):
        rng = np.random.default_rng(seed)
        ly = jr.log_emissions(rng.dirichlet(np.full(3, 0.5), 5).astype(np.float32), 0, jc.EPS)
        for seq in [(), (0,), (0, 0), (0, 1), (1, 0, 1), (1, 1)]:
            lp, psi = jr.prefix_scores(ly, 2, seq)
            assert close(lp, jr.brute_force(ly, 2, seq), 1e-12), (seed, seq)
            assert close(psi, jr.brute_force(ly, 2, seq, prefix=True), 1e-12), (seed, seq)
    ly0 = np.zeros((0, 3))
    assert jr.prefix_scores(ly0, 2, ()) == (0.0, 0.0) and jr.prefix_scores(ly0, 2, (1,))[0] == NEG


def test_wide_beam_equals_exhaustive_enumeration():
    """(b) two streams (T = 6 and 5, C = 4), G = 3, a lexicon on the second, weights (1, 0.7), beam 32, max_len 3: the four returned
    sequences are the argmax over all 40 sequences scored path by path."""
    lex = [[0, 1], [1], [2, 0]]
    smallest = float("inf")
    for seed in range(4):
        rng = np.random.default_rng(100 + seed)
        ly = [jr.log_emissions(rng.dirichlet(np.full(4, 0.4), T).astype(np.float32), 0, jc.EPS) for T in (6, 5)]
        streams = [dict(ly=ly[0], blank=3, lex=None, w=1.0), dict(ly=ly[1], blank=3, lex=lex, w=0.7)]
        res = jr.search(streams, 3, beam=32, top_paths=4, max_len=3)
        tabs = [labelling_table(l, 3) for l in ly]
        seqs = [()] + [q for n in (1, 2, 3) for q in itertools.product(range(3), repeat=n)]
        assert len(seqs) == 40
        sc = [1.0 * tabs[0].get(q, NEG) + 0.7 * tabs[1].get(tuple(jc.expand(q, lex)), NEG) for q in seqs]
        order = sorted(range(40), key=lambda i: (-sc[i], i))[:4]
        assert [list(seqs[i]) for i in order] == res["paths"], seed
        assert max(abs(sc[i] - s) for i, s in zip(order, res["score"])) < 1e-11
        assert res == {**jr.search(streams, 3, beam=32, top_paths=4, max_len=3, early=False), "rounds": res["rounds"], "margin": res["margin"]}
        smallest = min(smallest, res["margin"])
    print("joint: wide beam == exhaustive on 4 seeds, smallest decision margin %.3e" % smallest)


@pytest.mark.parametrize("case", jc.gpu_cases(), ids=lambda c: c["name"])
def test_early_stop_equals_no_stop(case):
    """(c) the stop never changes the output: sequences, scores and per-stream parts are the same bits."""
    a, b = decoded(case), decoded(case, early=False)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y), case["name"]
    assert np.all(a[4] <= b[4])


@pytest.mark.parametrize("case", jc.gpu_cases(), ids=lambda c: c["name"])
def test_gpu_cases_have_a_decision_margin(case):
    """(d) what lets the GPU tests ask for equal sequences on every sample: no cut, no neighbouring pair of the final list and no stop
    test of any case is closer than MARGIN.  The tie case is exact ties by construction and stands apart."""
    margin = decoded(case)[5]
    print("joint: case %-16s smallest decision margin %.3e" % (case["name"], margin))
    if case["name"] == jc.TIE:
        assert margin == 0.0
    else:
        assert margin >= jc.MARGIN, (case["name"], margin)


def test_tie_case_takes_the_smaller_gesture():
    """Gesture 1 is gesture 0's twin: hypotheses that differ by swapping the two score the same bits, and the one with the smaller
    gesture at the first difference was found earlier, so it comes first."""
    out, out_len, score = decoded(jc.tie_case())[:3]
    twins = 0
    for b in range(out.shape[0]):
        for k in range(out.shape[1] - 1):
            if out_len[b, k + 1] >= 0 and score[b, k] == score[b, k + 1]:
                twins += 1
                assert np.array_equal(np.where(out[b, k] == 1, 0, out[b, k]), np.where(out[b, k + 1] == 1, 0, out[b, k + 1]))
                assert list(out[b, k]) < list(out[b, k + 1])
    assert twins >= 1


def test_pool_miss_case():
    """(e) the planted case: the skeletal beam search's 2-best and the audio lexicon 1-best - decode_rescoring's pool - do not hold the
    truth, re-ranking the pool returns a wrong sequence, the joint search with equal weights returns the truth."""
    c = jc.pool_miss_case()
    sk, au = c["streams"]
    lex = au["lexicon"]
    nbest, _, _, gap = br.beam_search_lm(sk["P"], [38], beam_width=10, top_paths=2, skip=2, eps=jc.EPS)
    assert gap > jc.MARGIN
    one = lr.decode(au["P"][0], lex, 43, skip=2, eps=jc.EPS)["seq"]
    pool = [list(h) for h in nbest[0]]
    if list(one) not in pool:
        pool.append(list(one))
    assert nbest[0] == [c["sk_wrong"], c["sk_wrong2"]] and list(one) == c["au_wrong"]
    assert c["truth"] not in pool
    parts = np.stack([rr.score_paths(sk["P"], [pool], 21, len(pool)), rr.score_paths(au["P"], [pool], 43, len(pool), lexicon=lex)], axis=2)
    order, total = rr.combine(parts, [pool], (1.0, 1.0))
    assert pool[order[0, 0]] != c["truth"] and total[0, 0] - total[0, 1] > jc.MARGIN
    out, out_len, score = decoded(c)[:3]
    assert list(out[0, 0, :out_len[0, 0]]) == c["truth"]
    assert score[0, 0] > total[0, 0]                   # and it beats everything in the pool


def test_tables():
    """(f) the score is the definition's sum; a -inf entry of ext forbids the transition; fin takes no part in the pruning."""
    c = [x for x in jc.shape_cases() if x["name"] == "m3_tables"][0]
    out, out_len, score, logp = decoded(c)[:4]
    w = [s["weight"] for s in c["streams"]]
    for b in range(out.shape[0]):
        for k in range(out.shape[1]):
            if out_len[b, k] < 0:
                continue
            seq = [int(g) for g in out[b, k, :out_len[b, k]]]
            want = float(np.dot(w, logp[b, k])) + jr.table_terms(seq, c["G"], c["ext"], c["fin"])
            assert abs(score[b, k] - want) <= 1e-12 * abs(want)
            assert all(c["ext"][p + 1, g] != NEG for p, g in zip([-1] + seq[:-1], seq))
            # each part is the stream's own likelihood of the expansion
            for m, s in enumerate(c["streams"]):
                words = seq if s["lexicon"] is None else jc.expand(seq, s["lexicon"])
                ly = jr.log_emissions(s["P"][b], s["skip"], s["eps"], None if s["il"] is None else s["il"][b])
                assert close(logp[b, k, m], jr.prefix_scores(ly, s["blank"], words)[0], 1e-10)
    # a hard grammar: only (), (1), (1, 0), (1, 0, 2) are sequences at all, and fin forbids ending in gesture 1
    c = [x for x in jc.shape_cases() if x["name"] == "hard_grammar"][0]
    out, out_len = decoded(c)[:2]
    got = [sorted(tuple(out[b, k, :out_len[b, k]]) for k in range(4) if out_len[b, k] >= 0) for b in range(2)]
    assert got == [[(), (1, 0), (1, 0, 2)]] * 2
    # fin does not prune: (1) may not end a sequence, yet it is extended - above - and with fin alone forbidding the planted prefix
    rng = np.random.default_rng(7)
    ly = jr.log_emissions(jc.peaky(rng, 20, 3, 2, [0, 1], skip=0, lo=1e-3), 0, jc.EPS)
    st = [dict(ly=ly, blank=2, lex=None, w=1.0)]
    fin = np.array([0.0, NEG, 0.0])
    with_fin = jr.search(st, 2, None, fin, beam=1, top_paths=1, max_len=4)
    without = jr.search(st, 2, None, None, beam=1, top_paths=1, max_len=4)
    assert with_fin["paths"] == without["paths"] == [[0, 1]] and with_fin["score"] == without["score"]
