"""Seeded inputs shared by tests/test_cpu_rescore.py and tests/test_gpu_rescore.py: the GPU tests rank them with rescore_nbest and
demand the restatement's order without allowance; the CPU test shows on the same inputs that the fp64 totals lie far enough apart
for that (an f32-accurate kernel cannot flip them) and that the cases plant what they claim."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as ar  # noqa: E402
import rescore_ref as rr  # noqa: E402

SKIP = 2
EPS = 1e-8
REL = 1e-4            # the project's bound for the CTC loss (README, north_star; REL of test_gpu_align.py)
MARGIN = 1e-3         # the least gap between neighbouring totals of a planted ranking case, relative to |best|
N_GESTURES = 21       # the shared gesture alphabet: ids 0 .. 20, blank 21
HI, LEAN = 0.9, 0.6   # planted posteriors: HI on the aligned class; a confused stream's weight on the wrong hypothesis


def reference_lexicon():
    from mgr_amd.audio_network.sequence_decoding import GESTURE_LEXICON
    return [list(p) for p in GESTURE_LEXICON]


# shared words (1 in four phrases), repeated words inside a phrase ([1, 1, 2], [3, 3]) and across phrases (... 2 | 2, ... 1 | 1 ...): C = 8
SHARED_LEXICON = [[0, 1], [1, 1, 2], [2], [0, 1, 1], [3, 3], [6, 5, 4, 6]]


def random_hyps(rng, n_ids, B, K, max_len, p_absent=0.0):
    """Per sample K hypotheses (None: an absent slot) of 0 .. max_len ids below n_ids."""
    return [[None if rng.random() < p_absent else [int(v) for v in rng.integers(0, n_ids, int(rng.integers(0, max_len + 1)))]
             for _ in range(K)] for _ in range(B)]


def pack(hyps, K, Lh):
    """The list form above (None = absent) -> (hyp (B, K, Lh) int32 padded -1, hyp_len (B, K) int32)."""
    hyp, hl = -np.ones((len(hyps), K, Lh), np.int32), -np.ones((len(hyps), K), np.int32)
    for b, row in enumerate(hyps):
        for k, h in enumerate(row):
            if h is not None:
                hyp[b, k, :len(h)] = h
                hl[b, k] = len(h)
    return hyp, hl


def _planted(To, labels, blank, Cn, hi):
    """Posteriors with hi on an alignment that spreads the frames evenly over the labels and the blanks around them (the remainder
    goes to the leading blank): how many frames speak for a label is then known, not drawn."""
    S = 2 * len(labels) + 1
    frames = np.full(S, To // S)
    frames[0] += To - int(frames.sum())
    return ar.planted_posteriors(np.repeat(np.arange(S), frames), labels, blank, Cn, SKIP, hi)


def _pool_around(rng, truth, alphabet):
    """The truth among a substitution, a deletion and an insertion of it (alphabet: gesture -> what may stand in for it), in a drawn order; returns (pool, index of the truth, index of
    the substitution)."""
    other = lambda g: int(rng.choice([a for a in alphabet[g] if a != g]))
    sub = list(truth)
    i = int(rng.integers(0, len(truth)))
    sub[i] = other(truth[i])
    ins = list(truth)
    ins.insert(int(rng.integers(0, len(truth) + 1)), int(rng.choice(sorted(alphabet))))
    cand = [list(truth), sub, list(truth[:-1]), ins]
    perm = rng.permutation(4)
    pool = [cand[j] for j in perm]
    return pool, int(np.flatnonzero(perm == 0)[0]), int(np.flatnonzero(perm == 1)[0])


def ranking_cases(n_cases=4, N=3):
    """Two-stream planted cases.  Stream 0: gesture posteriors, C = 22, T = 40; stream 1: word posteriors, C = 44, T = 23, read through
    the reference lexicon.  Every stream is planted on the truth, but on sample wrong[m] stream m is a mixture of that and of posteriors
    planted on the pool's substitution, LEAN to (1 - LEAN): alone it prefers the wrong hypothesis there - by ln(LEAN / (1 - LEAN)) per
    frame of the gesture in question -, the other stream prefers the truth by much more, and so does the sum, on every sample.
    The last case carries a bigram that forbids one transition of sample 0's truth.  Yields dicts."""
    lex = reference_lexicon()
    short = [g for g in range(N_GESTURES) if len(lex[g]) <= 2]      # (gestures of one or two words: no two of them share a word)
    alike = {g: [a for a in short if len(lex[a]) == len(lex[g])] for g in short}     # ... and a substitution keeps the word count
    shapes = ((22, 40, None), (44, 23, lex))        # (C, T, lexicon)
    for case in range(n_cases):
        rng = np.random.default_rng(4200 + case)
        truths = [[int(v) for v in rng.choice(short, size=int(rng.integers(2, 4)))] for _ in range(N)]
        pools, t_idx, s_idx = zip(*[_pool_around(rng, t, alike) for t in truths])
        wrong = [int(v) for v in rng.permutation(N)[:2]]
        streams = []
        for m, (Cn, T, lexicon) in enumerate(shapes):
            P = []
            for b in range(N):
                words = lambda seq: seq if lexicon is None else rr.expand(seq, lexicon)
                Pb = _planted(T - SKIP, words(truths[b]), Cn - 1, Cn, HI)
                if b == wrong[m]:       # the stream confuses the two gestures, and leans to the wrong one
                    Pb = (LEAN * _planted(T - SKIP, words(pools[b][s_idx[b]]), Cn - 1, Cn, HI) + (1.0 - LEAN) * Pb).astype(np.float32)
                P.append(Pb)
            streams.append({"P": np.stack(P), "C": Cn, "lexicon": lexicon})
        lm = lm_end = None
        if case == n_cases - 1:
            # the first of the truth's transitions (start and end included) whose ban leaves two hypotheses of sample 0's pool allowed
            t0 = truths[0]
            for i in range(len(t0) + 1):
                lm, lm_end = np.zeros((N_GESTURES + 1, N_GESTURES)), np.zeros(N_GESTURES + 1)
                if i < len(t0):
                    lm[t0[i - 1] + 1 if i else 0, t0[i]] = -np.inf
                else:
                    lm_end[t0[-1] + 1] = -np.inf
                if sum(rr.lm_term(h, lm, lm_end) == 0.0 for h in pools[0]) >= 2:
                    break
            else:
                raise AssertionError("no ban leaves two hypotheses")
        yield {"name": "case %d" % case, "streams": streams, "paths": [list(p) for p in pools], "truth": list(t_idx), "sub": list(s_idx),
               "wrong": wrong, "weights": (1.0, 1.0), "lm": lm, "lm_end": lm_end, "alpha": 0.7, "beta": 0.0}


def reference_ranking(case):
    """(order, total, parts) of a ranking case by the restatement."""
    K = max(len(p) for p in case["paths"])
    parts = np.stack([rr.score_paths(s["P"], case["paths"], s["C"] - 1, K, SKIP, EPS, None, s["lexicon"]) for s in case["streams"]], axis=2)
    order, total = rr.combine(parts, case["paths"], case["weights"], case["lm"], case["lm_end"], case["alpha"], case["beta"])
    return order, total, parts
