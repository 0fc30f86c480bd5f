"""fp64 restatements the rescoring tests compare against (plain numpy, no GPU): the CTC likelihood of a label sequence - the alpha
recursion in log space over align_ref.log_emissions, summing where align_ref.viterbi maximises -, the phrase expansion, the slot
conventions of mgr_ctc_rescore, and the pooling / combination / ranking of decoding.py, each stated on its own.
"""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as ar  # noqa: E402

NEG_INF = -np.inf
MAX_LABELS = 255


def _lse(vals):
    m = max(vals)
    if m == NEG_INF:
        return NEG_INF
    return m + np.log(sum(np.exp(v - m) for v in vals))


def forward(logy, labels, blank):
    """ln sum over all alignments of `labels` of prod_t y[t, pi_t]; logy (T, C) fp64.  T = 0: 0 for the empty sequence, -inf else.
    The step over a blank goes only onto a label that differs from the previous one (and is not the blank itself)."""
    logy = np.asarray(logy, np.float64)
    T = logy.shape[0]
    ext = ar.extended(labels, blank)
    S = len(ext)
    if T == 0:
        return 0.0 if S == 1 else NEG_INF
    skip_ok = np.zeros(S, bool)
    skip_ok[3::2] = (ext[3::2] != ext[1:-2:2]) & (ext[3::2] != blank)
    a = np.full(S, NEG_INF)
    a[0] = logy[0, ext[0]]
    if S > 1:
        a[1] = logy[0, ext[1]]
    for t in range(1, T):
        c = np.full((3, S), NEG_INF)
        c[0] = a
        c[1, 1:] = a[:-1]
        c[2, 2:] = np.where(skip_ok[2:], a[:-2], NEG_INF)
        m = c.max(axis=0)
        ms = np.where(m == NEG_INF, 0.0, m)          # (a dead state: every term is exp(-inf) = 0, log 0 = -inf)
        with np.errstate(divide="ignore"):
            a = ms + np.log(np.exp(c - ms).sum(axis=0)) + logy[t, ext]
    return float(_lse([a[S - 1]] + ([a[S - 2]] if S > 1 else [])))


def enumerate_logp(logy, labels, blank):
    """The same by its definition: the sum over ALL C^T frame labellings that collapse to the labels (small T, C only)."""
    T, Cn = logy.shape
    target = [int(l) for l in labels]
    tot = 0.0
    for path in itertools.product(range(Cn), repeat=T):
        if ar.collapse(path, blank) == target:
            tot += np.exp(ar.path_score(logy, path))
    with np.errstate(divide="ignore"):
        return float(np.log(tot))


def expand(entries, lexicon):
    """Phrase ids -> words; None where an id is outside the lexicon."""
    lex = [[int(w) for w in p] for p in ([lexicon[g] for g in range(len(lexicon))] if isinstance(lexicon, dict) else lexicon)]
    if any(not 0 <= int(g) < len(lex) for g in entries):
        return None
    return [w for g in entries for w in lex[int(g)]]


def needs(labels):
    """Frames a label sequence needs: one per label and a blank between equal neighbours."""
    return len(labels) + sum(a == b for a, b in zip(labels, labels[1:]))


def score_slot(P, entries, blank, skip=2, eps=1e-8, input_len=None, lexicon=None):
    """One slot of mgr_ctc_rescore by the table of include/mgr.h: P (T, C) float32, entries = the hypothesis (None: absent slot).
    Returns (logp, n_lab)."""
    P = np.asarray(P, np.float32)
    To = P.shape[0] - skip
    Tp = To if input_len is None else max(0, min(int(input_len), To))
    if entries is None:
        return NEG_INF, -1
    if lexicon is not None:
        labels = expand(entries, lexicon)
        if labels is None:
            return np.nan, -1
    else:
        labels = [min(max(int(v), 0), P.shape[1] - 1) for v in entries]      # (clipped into the class range, as the loss clips)
    if len(labels) > MAX_LABELS:
        return np.nan, len(labels)
    return forward(ar.log_emissions(P[:skip + Tp], skip, eps), labels, blank), len(labels)


def score_batch(P, hyp, hyp_len, blank, skip=2, eps=1e-8, input_len=None, lexicon=None):
    """(hyp (N, K, Lh), hyp_len (N, K)) -> (logp (N, K) float64, n_lab (N, K) int32)."""
    N, K = hyp_len.shape
    logp, n_lab = np.zeros((N, K)), np.zeros((N, K), np.int32)
    for b in range(N):
        for k in range(K):
            n = int(hyp_len[b, k])
            ent = None if n < 0 else [int(v) for v in hyp[b, k, :min(n, hyp.shape[2])]]
            logp[b, k], n_lab[b, k] = score_slot(P[b], ent, blank, skip, eps, None if input_len is None else input_len[b], lexicon)
    return logp, n_lab


def score_paths(P, paths, blank, K, skip=2, eps=1e-8, input_len=None, lexicon=None):
    """Per sample a list of hypotheses -> logp (N, K), -inf in the slots behind a sample's list."""
    out = np.full((len(paths), K), NEG_INF)
    for b, hyps in enumerate(paths):
        for k, h in enumerate(hyps):
            out[b, k] = score_slot(P[b], list(h), blank, skip, eps, None if input_len is None else input_len[b], lexicon)[0]
    return out


def pool(*lists, cap=None):
    """Per sample the ordered union without duplicates: the first list's order, then what each further list adds."""
    out = []
    for b in range(len(lists[0])):
        cur = []
        for lst in lists:
            for h in lst[b]:
                h = [int(v) for v in h]
                if h not in cur:
                    cur.append(h)
        out.append(cur[:cap] if cap is not None else cur)
    return out


def lm_term(h, lm=None, lm_end=None):
    """The bigram terms of one hypothesis: lm[prev + 1, g] over it + lm_end[last + 1] (index 0: start / empty)."""
    t, prev = 0.0, -1
    for g in h:
        if lm is not None:
            t += float(np.asarray(lm, np.float64)[prev + 1, g])
        prev = int(g)
    if lm_end is not None:
        t += float(np.asarray(lm_end, np.float64)[prev + 1])
    return t


def combine(parts, paths, weights=None, lm=None, lm_end=None, alpha=1.0, beta=0.0):
    """(order (N, K), total in that order): total = sum_m w_m parts + alpha * bigram terms + beta * length; descending, ties in pool
    order; -inf, NaN and absent slots last, in pool order."""
    parts = np.asarray(parts, np.float64)
    N, K, M = parts.shape
    w = [1.0] * M if weights is None else [float(v) for v in weights]
    order, total = np.zeros((N, K), np.int64), np.zeros((N, K))
    for b in range(N):
        tot = []
        for k in range(K):
            if k >= len(paths[b]):
                tot.append(NEG_INF)
                continue
            t = sum(w[m] * parts[b, k, m] for m in range(M) if w[m] != 0.0)
            lt = lm_term(paths[b][k], lm, lm_end)
            t += (alpha * lt if lt != NEG_INF else NEG_INF) + beta * len(paths[b][k])
            tot.append(t)
        good = [k for k in range(K) if np.isfinite(tot[k])]
        good.sort(key=lambda k: -tot[k])          # (stable: ties keep pool order)
        order[b] = good + [k for k in range(K) if not np.isfinite(tot[k])]
        total[b] = [tot[k] for k in order[b]]
    return order, total
