"""fp64 reference for the beam search with a label bigram and an N-best list (mgr_ctc_beam_search_lm), and an exhaustive
enumerator to hold it against.

beam_search_lm restates oracle.keras_ref.ctc_beam_search(merge_repeated=False) - the same candidate numbering, the same lse formula,
the same tie rule - with the accumulated bonus per beam, the final ranking and the top_paths read-out, and reports the smallest score
gap at any cut, so that a test can prove its inputs are no near-ties before it asks for equal sequences.  enumerate_labellings visits
all C^T' frame paths of a tiny case, sums them per labelling, adds the bonuses and ranks: independent of any search."""
import itertools
import math

import numpy as np

NEG_INF = float("-inf")


def _lse64(a, b):
    """oracle.keras_ref._lse64's formula (= lse64 of the HIP kernels)."""
    if a == NEG_INF:
        return b
    if b == NEG_INF:
        return a
    m = a if a > b else b
    return m + math.log1p(math.exp(-abs(a - b)))


def beam_search_lm(P, input_length, ext=None, fin=None, beam_width=10, top_paths=1, skip=2, blank=None, eps=1e-8):
    """P (B, T, C) posteriors; ext (C + 1, C) or None (zeros): the bonus for appending c after label p is ext[p + 1, c], row 0 = the
    empty prefix; fin (C + 1,) or None: added once at the end, indexed by last label + 1.
    Per frame the candidates are idx = r * (C + 1) + slot (slot 0: stay on beam r, slot 1 + c: extend it by c); an extension onto a
    live beam merges its network mass into that beam's stay candidate (stay term first); a candidate ranks by lse(pb, pnb) + lm, ties
    to the smaller idx, -inf dropped; the beam_width best survive.  After the last frame the survivors are ranked by total +
    fin[last + 1] (ties to the better rank before, -inf dropped) and the first top_paths are returned.
    Returns (seqs, score, logp_ctc, gap): per sample the ranked list of at most top_paths label lists, their scores and the network's
    part of each; gap = the smallest difference between two scores whose order decides something: at every frame's cut the last
    survivor against the first candidate dropped, at the end each returned hypothesis against the next one in the final ranking."""
    P = np.asarray(P)
    B, T, C = P.shape
    blank = C - 1 if blank is None else blank
    ext = np.zeros((C + 1, C)) if ext is None else np.asarray(ext, np.float64).reshape(C + 1, C)
    fin = None if fin is None else np.asarray(fin, np.float64).reshape(C + 1)
    input_length = np.asarray(input_length).reshape(B).astype(np.int64)
    seqs, scores, logps, gap = [], [], [], float("inf")
    for b in range(B):
        Tp = int(min(max(input_length[b], 0), T - skip))
        beams = [((), 0.0, NEG_INF, 0.0)]          # ranked: (prefix, log p_blank, log p_nonblank, lm)
        for t in range(Tp):
            u = P[b, skip + t].astype(np.float64) + eps
            with np.errstate(divide="ignore"):
                logy = np.log(u) - math.log(float(u.sum()))
            index = {beam[0]: r for r, beam in enumerate(beams)}
            cand = {}
            for r, (pref, pb, pnb, lm) in enumerate(beams):
                tot = _lse64(pb, pnb)
                cand[r * (C + 1)] = [pref, tot + logy[blank], pnb + logy[pref[-1]] if pref else NEG_INF, lm]
            for r, (pref, pb, pnb, lm) in enumerate(beams):
                tot = _lse64(pb, pnb)
                for c in range(C):
                    if c == blank:
                        continue
                    val = (pb if (pref and c == pref[-1]) else tot) + logy[c]
                    r2 = index.get(pref + (c,))
                    if r2 is not None:
                        e = cand[r2 * (C + 1)]
                        e[2] = _lse64(e[2], val)
                    else:
                        cand[r * (C + 1) + 1 + c] = [pref + (c,), NEG_INF, val, lm + float(ext[(pref[-1] + 1) if pref else 0, c])]
            ranked = sorted((-(_lse64(e[1], e[2]) + e[3]), idx) for idx, e in cand.items() if _lse64(e[1], e[2]) + e[3] != NEG_INF)
            if len(ranked) > beam_width:
                gap = min(gap, ranked[beam_width][0] - ranked[beam_width - 1][0])
            beams = [tuple(cand[idx]) for _, idx in ranked[:beam_width]]
        final = []
        for r, (pref, pb, pnb, lm) in enumerate(beams):
            net = _lse64(pb, pnb)
            f = net + lm
            if fin is not None:
                f = f + float(fin[(pref[-1] + 1) if pref else 0])
            if f != NEG_INF:
                final.append((-f, r, list(pref), net))
        final.sort(key=lambda e: (e[0], e[1]))
        for k in range(min(top_paths, len(final) - 1)):
            gap = min(gap, final[k + 1][0] - final[k][0])
        final = final[:top_paths]
        seqs.append([e[2] for e in final])
        scores.append([-e[0] for e in final])
        logps.append([e[3] for e in final])
    return seqs, scores, logps, gap


def collapse(path, blank):
    """A frame path -> its labelling: equal neighbours merged, blanks removed."""
    return tuple(k for k, _ in itertools.groupby(path) if k != blank)


def enumerate_labellings(P1, ext=None, fin=None, skip=0, blank=None, eps=0.0):
    """P1 (T, C) posteriors of one tiny sample.  Visits all C^(T - skip) frame paths, sums their probabilities (under y = (P + eps) /
    sum(P + eps), as the search) per labelling, and adds the bonuses.  Returns (ranked, net_ranked): the labellings with a finite score
    as (labelling tuple, score, log p_ctc), best score first, and the same entries ordered by log p_ctc + the ext bonuses alone - the
    order the search prunes in."""
    P1 = np.asarray(P1)
    T, C = P1.shape
    blank = C - 1 if blank is None else blank
    ext = np.zeros((C + 1, C)) if ext is None else np.asarray(ext, np.float64).reshape(C + 1, C)
    y = P1[skip:].astype(np.float64) + eps
    y = y / y.sum(axis=1, keepdims=True)
    terms = {}
    for path in itertools.product(range(C), repeat=T - skip):
        p = 1.0
        for t, c in enumerate(path):
            p *= y[t, c]
        terms.setdefault(collapse(path, blank), []).append(p)
    rows = []
    for lab, ps in terms.items():
        mass = math.fsum(ps)
        if mass <= 0.0:
            continue
        net = math.log(mass)
        lm, prev = 0.0, 0
        for c in lab:
            lm += float(ext[prev, c])
            prev = c + 1
        pruned = net + lm
        score = pruned + (float(fin[prev]) if fin is not None else 0.0)
        if score != NEG_INF:
            rows.append((lab, score, net, pruned))
    ranked = sorted(rows, key=lambda e: (-e[1], e[0]))
    net_ranked = sorted(rows, key=lambda e: (-e[3], e[0]))
    return [e[:3] for e in ranked], [(e[0], e[3], e[2]) for e in net_ranked]
