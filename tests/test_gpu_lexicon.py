"""-m gpu: mgr_ctc_lexicon_decode - the best phrase sequence over a lexicon composed with the CTC topology - against the fp64 restatement
of tests/lexicon_ref.py, against mgr_ctc_align, through decoding.lexicon_decode and through the facade.  The inputs are those of
tests/lexicon_cases.py (tests/test_cpu_lexicon.py checks on them that near ties are as rare as the allowance below assumes)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as ar  # noqa: E402
import lexicon_cases as lc  # noqa: E402
import lexicon_ref as lr  # noqa: E402

pytestmark = pytest.mark.gpu

SKIP, EPS = lc.SKIP, lc.EPS
REL = 1e-4          # the project's bound for the CTC loss (README, north_star; REL of test_gpu_align.py)
CONF_TOL = 1e-6
TIE_TOL = 1e-6      # a near tie: the fp64 score of the returned sequence within TIE_TOL * max(1, |optimum|) of the optimum


def _lex_raw(device, P, lexicon, ext=None, fin=None, il=None, cap=None, skip=SKIP, eps=EPS, want_path=True):
    """mgr_ctc_lexicon_decode through the C ABI: dict of n, phr, seg, conf, path, score, logp."""
    from mgr_amd import decoding
    P = np.ascontiguousarray(P, np.float32)
    B, T, Cn = P.shape
    off, words = decoding.compile_lexicon(lexicon, Cn)
    G = len(off) - 1
    cap = T - skip if cap is None else cap
    il = np.full(B, T - skip, np.int32) if il is None else np.asarray(il, np.int32)
    ext = np.zeros((G + 1, G)) if ext is None else np.ascontiguousarray(ext, np.float64)
    ins = [device.array(P), device.array(il), device.array(ext)]
    dfin = device.array(np.ascontiguousarray(fin, np.float64)) if fin is not None else None
    outs = {"n": device.empty((B,), np.int32), "phr": device.empty((B, cap), np.int32), "seg": device.empty((B, cap, 2), np.int32),
            "conf": device.empty((B, cap), np.float32), "path": device.empty((B, T - skip), np.int32) if want_path else None,
            "score": device.empty((B,), np.float64), "logp": device.empty((B,), np.float64)}
    ws = device.bytes(device.lib.mgr_ctc_lexicon_ws_bytes(B, T, Cn, G, off.ctypes.data))
    device.call("mgr_ctc_lexicon_decode", ins[0], ins[1], B, T, Cn, skip, Cn - 1, C.c_float(eps), off.ctypes.data, words.ctypes.data, G,
                ins[2], dfin, cap, outs["n"], outs["phr"], outs["seg"], outs["conf"], outs["path"], outs["score"], outs["logp"], ws, ws.nbytes)
    res = {k: (v.download() if v is not None else None) for k, v in outs.items()}
    for a in ins + [dfin, ws] + list(outs.values()):
        if a is not None:
            a.free()
    return res


class Tally:
    """Largest measured gaps and the number of near ties, per test."""

    def __init__(self):
        self.score = self.logp = self.conf = 0.0
        self.n = {True: 0, False: 0}
        self.ties = {True: 0, False: 0}

    def line(self, what):
        return ("%-34s samples %4d planted / %4d random   score vs fp64 optimum %.3e   logp vs fp64 score of the path %.3e   conf abs %.3e   "
                "near ties %d planted / %d random" % (what, self.n[True], self.n[False], self.score, self.logp, self.conf, self.ties[True],
                                                      self.ties[False]))

    def check_allowance(self):
        assert self.ties[True] == 0, self.ties
        assert self.ties[False] <= 0.02 * self.n[False], (self.ties, self.n)


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def _check_sample(res, b, P, lexicon, ext, fin, il, planted, tally, cap=None):
    """Sample b of a raw result against the fp64 restatement: everything the issue lists."""
    Cn = P.shape[1]
    blank, To = Cn - 1, P.shape[0] - SKIP
    Tp = To if il is None else max(0, min(int(il), To))
    ref = lr.decode(P, lexicon, blank, ext, fin, SKIP, EPS, Tp)
    n = int(res["n"][b])
    cap = res["phr"].shape[1] if cap is None else cap
    if ref["seq"] is None:
        assert n == -1 and res["score"][b] == -np.inf and res["logp"][b] == -np.inf
        assert np.all(res["phr"][b] == -1) and np.all(res["seg"][b] == -1) and np.all(res["path"][b] == -1) and np.all(res["conf"][b] == 0)
        return
    assert n >= 0, (b, n, ref["seq"])
    assert n <= cap, "the checks below need the whole sequence"
    seq = [int(g) for g in res["phr"][b, :n]]
    assert np.all(res["phr"][b, n:] == -1) and np.all(res["seg"][b, n:] == -1) and np.all(res["conf"][b, n:] == 0)
    logy = ar.log_emissions(P[:Tp + SKIP], SKIP, EPS)
    path = res["path"][b, :Tp]
    assert np.all(res["path"][b, Tp:] == -1) and (Tp == 0 or path.min() >= 0)
    # the path is an alignment of the returned phrases' words; its fp64 score is logp; seg and conf are read off it
    assert ar.collapse(path, blank) == lr.expand(seq, lexicon), (b, seq)
    pscore = ar.path_score(logy, path) if Tp else 0.0
    g_logp = _rel(res["logp"][b], pscore)
    assert g_logp <= REL, (b, res["logp"][b], pscore)
    segs = lr.path_phrase_segments(path, seq, lexicon, blank, SKIP)
    assert [tuple(int(v) for v in s) for s in res["seg"][b, :n]] == segs, b
    want_conf = lr.phrase_conf(P, path, segs, blank, SKIP)
    g_conf = max([abs(float(c) - w) for c, w in zip(res["conf"][b, :n], want_conf)] + [0.0])
    assert g_conf <= CONF_TOL, (b, res["conf"][b, :n], want_conf)
    # score: the fp64 optimum (a near tie is within TIE_TOL of it, far inside REL); score - logp is the table terms of the sequence
    g_score = _rel(res["score"][b], ref["score"])
    assert g_score <= REL, (b, res["score"][b], ref["score"])
    tt = lr.table_terms(seq, len(lr.as_lists(lexicon)), ext, fin)
    assert abs((res["score"][b] - res["logp"][b]) - tt) <= 1e-9 * max(1.0, abs(tt))
    if seq == ref["seq"]:
        assert _rel(res["logp"][b], ref["logp"]) <= REL
    else:
        own = lr.sequence_score(logy, seq, lexicon, blank, ext, fin)
        assert own >= ref["score"] - TIE_TOL * max(1.0, abs(ref["score"])), (b, seq, ref["seq"], own, ref["score"])
        tally.ties[planted] += 1
    tally.n[planted] += 1
    tally.score, tally.logp, tally.conf = max(tally.score, g_score), max(tally.logp, g_logp), max(tally.conf, g_conf)


def _run_cases(device, cases, tally, via_host_api_every=4):
    from mgr_amd import decoding
    for i, case in enumerate(cases):
        res = _lex_raw(device, case["P"], case["lexicon"], case["ext"], case["fin"])
        for b in range(case["P"].shape[0]):
            _check_sample(res, b, case["P"][b], case["lexicon"], case["ext"], case["fin"], None, case["planted"], tally)
        if case["planted"] and case["kind"] == "zero":           # planted by a wide margin: the planted sequence itself comes back
            for b, q in enumerate(case["seqs"]):
                assert [int(g) for g in res["phr"][b, :res["n"][b]]] == q, (case["name"], b)
        if i % via_host_api_every == 0:                          # the same through decoding.lexicon_decode
            segs, score, logp, path = decoding.lexicon_decode(case["P"], case["lexicon"], lm=case["ext"], lm_end=case["fin"], dev=device,
                                                              return_path=True)
            assert np.array_equal(score, res["score"]) and np.array_equal(logp, res["logp"]) and np.array_equal(path, res["path"])
            for b, sg in enumerate(segs):
                n = max(0, int(res["n"][b]))
                assert sg == [(int(res["phr"][b, k]), int(res["seg"][b, k, 0]), int(res["seg"][b, k, 1]), float(res["conf"][b, k]))
                              for k in range(n)]


def _record(lines):
    print("\n".join(lines))
    out = os.environ.get("MGR_LEXICON_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("To", lc.REF_TOS)
def test_reference_lexicon_against_fp64(device, To):
    """The reference's 21 gesture phrases (97 states: two waves), C = 44, B = 5, planted and Dirichlet(0.1) posteriors, without
    tables, with a random bigram (15 % of it -inf) and with a hard grammar (whole rows -inf).  All shapes keep the back-pointers in
    LDS.  The near-tie allowance is asserted per length: no planted sample, and at most 2 % of the random ones - of 15, that is none."""
    tally = Tally()
    _run_cases(device, lc.reference_cases((To,)), tally)
    assert tally.n[True] == 15 and tally.n[False] >= 10      # (a random sample the grammar leaves no sequence is checked, not counted)
    tally.check_allowance()
    _record([tally.line("reference lexicon T-skip=%d" % To)])


@pytest.mark.slow
def test_full_length_planted(device):
    """B = 2, T = 1900: the running values are renormalised 118 times, and the back-pointers (46 KB + 40 KB) still fit LDS."""
    lex, Cn, T = lc.reference_lexicon(), 44, 1900
    rng = np.random.default_rng(1900)
    ext, fin = lc.tables(rng, len(lex), "bigram")
    seqs = [lc.random_sequence(rng, lex, T - SKIP, 20, ext, fin) for _ in range(2)]
    P = np.stack([lr.planted_case(rng, T - SKIP, q, lex, Cn - 1, Cn, SKIP)[0] for q in seqs])
    tally = Tally()
    res = _lex_raw(device, P, lex, ext, fin)
    for b in range(2):
        _check_sample(res, b, P[b], lex, ext, fin, None, True, tally)
        assert [int(g) for g in res["phr"][b, :res["n"][b]]] == seqs[b]
    tally.check_allowance()
    _record([tally.line("reference lexicon T=1900 planted")])


def test_topology_edges(device):
    """T - skip = 40, C = 8: one one-word phrase; 64 one-word phrases (the full width of the phrase-entry maximum); a 16-word phrase
    with adjacent repeated words (a blank inside is mandatory); a phrase whose last word is its first, planted twice in a row (a blank
    between the phrases is mandatory); phrases that are prefixes of each other.  Back-pointers in LDS."""
    tally = Tally()
    cases = list(lc.topology_cases())
    assert len(cases) == 18
    _run_cases(device, cases, tally)
    for case in cases:          # the mandatory blanks, spelled out
        if case["planted"] and case["name"].startswith(("16_words_repeat", "last_equals_first")):
            res = _lex_raw(device, case["P"][:1], case["lexicon"], case["ext"], case["fin"])
            path = res["path"][0]
            words = lr.expand(case["seqs"][0], case["lexicon"])
            assert ar.collapse(path, 7) == words and any(a == b for a, b in zip(words, words[1:]))
            runs = ar.path_segments(path, 7, 0)
            for (l0, _, e0), (l1, f1, _) in zip(runs, runs[1:]):
                assert l0 != l1 or f1 > e0 + 1
    tally.check_allowance()
    _record([tally.line("topology edges T-skip=40 C=8")])


def test_capacity_edge(device):
    """255 words in 64 phrases = 511 states (a workgroup of 512 threads), C = 64.  At T - skip = 40 the back-pointers (3 * 511 + 10 *
    64 words = 8.7 KB) live in LDS; at T - skip = 1400 they are 88 * 511 + 350 * 64 words = 269 KB and live in the workspace."""
    tally = Tally()
    _run_cases(device, lc.capacity_cases(), tally)
    lex, Cn, To = lc.capacity_lexicon(), 64, 1400
    rng = np.random.default_rng(1400)
    ext, fin = lc.tables(rng, len(lex), "bigram")
    seqs = [lc.random_sequence(rng, lex, To, 30, ext, fin) for _ in range(2)]
    P = np.stack([lr.planted_case(rng, To, q, lex, Cn - 1, Cn, SKIP)[0] for q in seqs])
    res = _lex_raw(device, P, lex, ext, fin)
    for b in range(2):
        _check_sample(res, b, P[b], lex, ext, fin, None, True, tally)
        assert [int(g) for g in res["phr"][b, :res["n"][b]]] == seqs[b]
    tally.check_allowance()
    _record([tally.line("capacity 511 states C=64")])


def test_length_and_table_edges_in_one_batch(device):
    lex, Cn, To = lc.reference_lexicon(), 44, 60
    G, blank = len(lex), Cn - 1
    rng = np.random.default_rng(60)
    seq = [5, 6, 10, 15, 1, 1, 2]                   # shared first words (8; 18), a repeated one-word phrase
    il = [0, 1, 37, To, To, To]
    B = len(il)
    P = np.stack([lr.planted_case(rng, To, seq, lex, blank, Cn, SKIP)[0] for _ in range(B)])
    P[1] = lr.planted_case(rng, To, [3], lex, blank, Cn, SKIP)[0]
    P[1, SKIP] = 0.1 / (Cn - 1)
    P[1, SKIP, 4] = 0.9                             # the single frame sample 1 decodes emits word 4 = phrase 3
    P[2, :37 + SKIP] = lr.planted_case(rng, 37, seq[:4], lex, blank, Cn, SKIP)[0]
    tally = Tally()
    res = _lex_raw(device, P, lex, None, None, il)
    for b in range(B):
        _check_sample(res, b, P[b], lex, None, None, il[b], True, tally)
    assert res["n"].tolist() == [0, 1, 4, 7, 7, 7] and res["score"][0] == 0.0 and res["logp"][0] == 0.0
    assert res["phr"][1, 0] == 3 and res["seg"][1, 0].tolist() == [SKIP, SKIP] and res["phr"][3, :7].tolist() == seq
    # cap smaller than the true count: n_phr is true, the rows are the first cap of the full result
    small = _lex_raw(device, P, lex, None, None, il, cap=3)
    assert small["n"].tolist() == res["n"].tolist()
    for k in ("score", "logp", "path"):
        assert np.array_equal(small[k], res[k])
    for b in range(B):
        m = min(3, int(res["n"][b]))
        assert np.array_equal(small["phr"][b, :m], res["phr"][b, :m]) and np.all(small["phr"][b, m:] == -1)
        assert np.array_equal(small["seg"][b, :m], res["seg"][b, :m]) and np.array_equal(small["conf"][b, :m], res["conf"][b, :m])
    from mgr_amd import decoding
    segs = decoding.lexicon_decode(P, lex, input_length=il, dev=device, max_phrases=3)[0]      # the host API runs again with room
    assert [[s[0] for s in sg] for sg in segs] == [[int(g) for g in res["phr"][b, :res["n"][b]]] for b in range(B)]
    # nothing may start: the empty sequence with score = the blanks + fin[0]; with fin[0] = -inf nothing at all
    ext = np.zeros((G + 1, G))
    ext[0] = -np.inf
    fin = np.zeros(G + 1)
    fin[0] = -1.25
    e = _lex_raw(device, P, lex, ext, fin, il)
    for b in range(B):
        _check_sample(e, b, P[b], lex, ext, fin, il[b], True, tally)
    assert e["n"].tolist() == [0] * B and e["score"][0] == -1.25 and np.all(e["path"][3] == blank)
    assert np.allclose(e["score"] - e["logp"], -1.25, rtol=0, atol=1e-12)
    fin[0] = -np.inf
    e = _lex_raw(device, P, lex, ext, fin, il)
    assert e["n"].tolist() == [-1] * B and np.all(e["score"] == -np.inf) and np.all(e["logp"] == -np.inf)
    assert np.all(e["phr"] == -1) and np.all(e["seg"] == -1) and np.all(e["path"] == -1) and np.all(e["conf"] == 0)
    # ... and per sample: only the samples the tables leave no sequence get it, their neighbours keep their results bit for bit
    ext2 = np.zeros((G + 1, G))
    ext2[0] = -np.inf
    ext2[0, 5] = 0.0                                 # a sequence must start with phrase 5 ...
    fin2 = np.zeros(G + 1)
    fin2[0] = -np.inf                                # ... and may not be empty: samples 0 (no frames) and 1 (one frame, phrase 5 has three words) have none
    m = _lex_raw(device, P, lex, ext2, fin2, il)
    assert m["n"].tolist() == [-1, -1, 4, 7, 7, 7]
    for b in range(B):
        _check_sample(m, b, P[b], lex, ext2, fin2, il[b], True, tally)
    alone = _lex_raw(device, P[2:], lex, ext2, fin2, il[2:])
    for k in m:
        assert np.array_equal(m[k][2:], alone[k])
    tally.check_allowance()


def test_independence_and_determinism(device):
    """A sample decoded alone equals, bit for bit, the same sample inside a batch of 7; two runs are bit-identical."""
    lex, Cn, To = lc.reference_lexicon(), 44, 120
    rng = np.random.default_rng(7)
    ext, fin = lc.tables(rng, len(lex), "bigram")
    P = rng.dirichlet(np.full(Cn, 0.1), size=(7, To + SKIP)).astype(np.float32)
    il = [To, 100, To, 17, To, To, 64]
    full = _lex_raw(device, P, lex, ext, fin, il)
    again = _lex_raw(device, P, lex, ext, fin, il)
    assert sum(full["n"]) > 7
    for k in full:
        assert np.array_equal(full[k], again[k]), k
    for b in (0, 3, 6):
        one = _lex_raw(device, P[b:b + 1], lex, ext, fin, il[b:b + 1])
        for k in full:
            assert np.array_equal(full[k][b:b + 1], one[k]), (b, k)


def test_logp_is_the_aligners_for_the_returned_sequence(device):
    """Without tables score = logp = A(words(Q)): mgr_ctc_align of the returned sequence's word expansion gives the same logp (1e-4
    relative; measured: profiles/lexicon_parity.txt) - and, being the best alignment of those words, the same path unless two
    alignments tie."""
    from test_gpu_align import _align_raw, _pad
    lex, Cn, To = lc.reference_lexicon(), 44, 200
    rng = np.random.default_rng(21)
    P = rng.dirichlet(np.full(Cn, 0.1), size=(6, To + SKIP)).astype(np.float32)
    P[3:] = np.stack([lr.planted_case(rng, To, lc.random_sequence(rng, lex, To, 12), lex, Cn - 1, Cn, SKIP)[0] for _ in range(3)])
    res = _lex_raw(device, P, lex)
    words = [lr.expand([int(g) for g in res["phr"][b, :res["n"][b]]], lex) for b in range(6)]
    Lmax = max(len(w) for w in words)
    path, seg, conf, logp = _align_raw(device, P, _pad(words, Lmax), [To] * 6, [len(w) for w in words])
    gap = max(_rel(res["logp"][b], logp[b]) for b in range(6))
    assert gap <= REL and np.array_equal(res["score"], res["logp"])
    same = sum(bool(np.array_equal(path[b], res["path"][b])) for b in range(6))
    assert same >= 3            # (the planted ones at the least)
    _record(["logp vs mgr_ctc_align of the returned sequence's words (no tables, T-skip=200): largest relative gap %.3e; paths equal %d/6"
             % (gap, same)])


def _batches(spec, B, T, Lmax, n, seed0=300):
    from mgr_amd.synthetic import synthetic_arrays
    return [synthetic_arrays(spec, B, T, Lmax, seed0 + i, lmin=2, lmax=5) for i in range(n)]


def test_facade_lexicon(device, tmp_path):
    """predict_generator(decode="lexicon", lexicon=GESTURE_LEXICON) on a tiny audio model equals lexicon_decode of predict_generator()'s
    posteriors of the same batches (a short last batch included), with and without a gesture bigram; pipelined equals one batch at a
    time; decode_lexicon writes an MLF that read_mlf reads back with gesture names and "start end name" lines."""
    from mgr_amd import decoding, keras_like as K
    from mgr_amd.audio_network import sequence_decoding as sd
    from mgr_amd.configs import audio_spec
    from mgr_amd.keras_like import Model
    from mgr_amd.synthetic import synthetic_weights
    K.set_learning_phase(0)
    decoding._DEV[0] = device
    spec = audio_spec(h=16)
    assert spec.num_classes == 44
    B, T, Lmax = 8, 64, 4
    data = [b[0] for b in _batches(spec, B, T, Lmax, 4, seed0=500)]
    data[-1] = {k: v[:3] for k, v in data[-1].items()}
    m = Model(spec, device=device)
    m.set_weights_dict(synthetic_weights(spec, 13))
    P = m.predict_generator(iter(data), steps=4)
    G = len(sd.GESTURE_LEXICON)
    rng = np.random.default_rng(2)
    blm, bend = decoding.bigram_lm([[int(g) for g in rng.integers(0, G, 5)] for _ in range(40)], G + 1, blank=G)
    lm, lm_end = blm[:G + 1, :G], bend[:G + 1]
    for kw in ({}, {"lm": lm, "lm_end": lm_end, "alpha": 0.7, "beta": 0.5}):
        segs, score, logp = m.predict_generator(iter(data), steps=4, decode="lexicon", lexicon=sd.GESTURE_LEXICON, **kw)
        hsegs, hscore, hlogp = decoding.lexicon_decode(P, sd.GESTURE_LEXICON, dev=device, eps=float(spec.ctc["eps"]), **kw)
        assert len(segs) == 3 * B + 3 and segs == hsegs and np.array_equal(score, hscore) and np.array_equal(logp, hlogp)
        assert np.all(np.isfinite(score))
    assert np.array_equal(P, m.predict_generator(iter(data), steps=4))          # the other modes are as they were
    e = m._engine
    pipe = list(e.predict_stream(iter(data[:3]), output="lexicon", lexicon=sd.GESTURE_LEXICON))
    single = [list(e.predict_stream([d], output="lexicon", lexicon=sd.GESTURE_LEXICON))[0] for d in data[:3]]
    for a, b in zip(pipe, single):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    with pytest.raises(ValueError):
        list(e.predict_stream(iter(data[:1]), output="lexicon"))
    # the module: planted gestures come back by name, with their times
    seqs = [[5, 6], [10, 15, 1], [], [19, 20, 0]]
    Pp = np.stack([lr.planted_case(rng, 80, q, sd.GESTURE_LEXICON, 43, 44, SKIP)[0] for q in seqs])
    f_list = [1, 2, 3, 4]
    names, gsegs = sd.decode_lexicon(Pp, f_list, out_file=str(tmp_path / "g.mlf"))
    assert names == [[sd.gesture_names[g] for g in q] for q in seqs] and [[s[0] for s in sg] for sg in gsegs] == seqs
    back = decoding.read_mlf(str(tmp_path / "g.mlf"))
    assert [back["Sample%05d_audio" % f] for f in f_list] == names
    timed = [l.split() for l in open(tmp_path / "g.mlf").read().split("\n") if l[:1].isdigit()]
    flat = [(s_, n_) for sg, ns in zip(gsegs, names) for s_, n_ in zip(sg, ns)]
    assert len(timed) == len(flat) == 8
    for (start, end, name), (s_, n_) in zip(timed, flat):
        assert (int(start), int(end), name) == (s_[1] * 500000, (s_[2] + 1) * 500000, n_)
    names2, _ = sd.decode_lexicon(m.predict_generator(iter(data), steps=4, decode="lexicon", lexicon=sd.GESTURE_LEXICON),
                                  list(range(1, 3 * B + 4)), out_file=None)
    assert len(names2) == 3 * B + 3
