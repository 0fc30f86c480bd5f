"""fp64 restatements the alignment / segment tests compare against (plain numpy, no GPU).

viterbi: the most probable CTC alignment of a label sequence - the alpha recursion over l' = [blank, l1, blank, ..., lL, blank] with max
in place of log-sum-exp.  Ties: a back-pointer tie takes the smallest step (stay, one state, two states), a tie of the two final states
the last blank; the step over two states only onto a label that differs from the previous label (and is not the blank).
greedy_segments: frame argmax, the reference's confidence filter in its net effect (decoding.py), the collapse - with the frame
positions and mean confidences kept.
"""
import itertools

import numpy as np

NEG_INF = -np.inf


def log_emissions(P, skip=2, eps=1e-8):
    """P (T, C) -> ln softmax(log(P[skip:] + eps)) in fp64 (the float32 input values, the float32 eps, fp64 arithmetic)."""
    u = np.asarray(P, np.float64)[skip:] + np.float64(np.float32(eps))
    with np.errstate(divide="ignore"):
        return np.log(u) - np.log(u.sum(axis=1, keepdims=True))


def extended(labels, blank):
    ext = [blank]
    for l in labels:
        ext += [int(l), blank]
    return np.asarray(ext, np.int64)


def viterbi(logy, labels, blank, dtype=np.float64):
    """logy (T, C).  Returns (score, states (T,) int) or (-inf, None) when no alignment fits."""
    logy = np.asarray(logy, dtype)
    T = logy.shape[0]
    ext = extended(labels, blank)
    S = len(ext)
    if T == 0:
        return NEG_INF, None
    s_idx = np.arange(S)
    skip_ok = np.zeros(S, bool)
    skip_ok[3::2] = (ext[3::2] != ext[1:-2:2]) & (ext[3::2] != blank)
    v = np.full(S, NEG_INF, dtype)
    v[0] = logy[0, ext[0]]
    if S > 1:
        v[1] = logy[0, ext[1]]
    bp = np.zeros((T, S), np.int8)
    for t in range(1, T):
        c = np.full((3, S), NEG_INF, dtype)
        c[0] = v
        c[1, 1:] = v[:-1]
        c[2, 2:] = np.where(skip_ok[2:], v[:-2], NEG_INF)
        step = np.argmax(c, axis=0)          # (the first maximum: the smallest step)
        bp[t] = step
        v = (c[step, s_idx] + logy[t, ext]).astype(dtype)
    fin = S - 1
    if S > 1 and v[S - 2] > v[S - 1]:        # (a tie takes the last blank)
        fin = S - 2
    if v[fin] == NEG_INF:
        return NEG_INF, None
    states = np.zeros(T, np.int64)
    s = fin
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    return float(v[fin]), states


def states_to_path(states, labels, blank):
    return extended(labels, blank)[states]


def states_to_segments(states, n_labels, skip=2):
    """[(first, last)] per label, original frame indices."""
    out = []
    for k in range(n_labels):
        f = np.flatnonzero(states == 2 * k + 1)
        out.append((int(f[0]) + skip, int(f[-1]) + skip))
    return out


def path_score(logy, path):
    path = np.asarray(path)
    return float(np.asarray(logy, np.float64)[np.arange(len(path)), path].sum())


def collapse(path, blank):
    return [int(k) for k, _ in itertools.groupby(path) if k != blank]


def path_segments(path, blank, skip=2):
    """(label, first, last) of every maximal non-blank run of a frame path, original frame indices."""
    out, t = [], 0
    for k, g in itertools.groupby(path):
        n = len(list(g))
        if k != blank:
            out.append((int(k), t + skip, t + n - 1 + skip))
        t += n
    return out


def brute_force_best(logy, labels, blank):
    """The best score over ALL C^T frame labellings that collapse to the labels (small T, C only)."""
    T, Cn = logy.shape
    best = NEG_INF
    target = [int(l) for l in labels]
    for path in itertools.product(range(Cn), repeat=T):
        if collapse(path, blank) == target:
            best = max(best, path_score(logy, path))
    return best


def planted_alignment(rng, To, labels, blank):
    """A valid alignment drawn at random: every label at least one frame, a blank between repeated labels, the remaining frames
    spread at random over all states.  Returns the state sequence (To,)."""
    L = len(labels)
    S = 2 * L + 1
    need = np.zeros(S, np.int64)
    need[1::2] = 1
    for k in range(1, L):
        if labels[k] == labels[k - 1]:
            need[2 * k] = 1
    spare = To - int(need.sum())
    assert spare >= 0, "labels do not fit"
    extra = np.bincount(rng.integers(0, S, spare), minlength=S)
    return np.repeat(np.arange(S), need + extra)


def planted_posteriors(states, labels, blank, Cn, skip=2, hi=0.9):
    """P (To + skip, C) float32: hi on the aligned class, (1 - hi) / (C - 1) elsewhere (the skipped frames are uniform)."""
    path = states_to_path(states, labels, blank)
    P = np.full((len(path) + skip, Cn), (1.0 - hi) / (Cn - 1), np.float32)
    P[:skip] = 1.0 / Cn
    P[np.arange(len(path)) + skip, path] = hi
    return P


def greedy_segments(P, thr, skip=2, with_count=False):
    """One sample, P (T, C) float32 -> [(label, first, last, mean confidence in fp64)] (with_count: and the number of surviving frames
    of the run), original frame indices.  The filter: for every
    label s the first k_s frames whose best label is s are dropped, k_s = the number of such frames with probability below thr."""
    P = np.asarray(P, np.float32)[skip:]
    best = P.argmax(axis=1)
    prob = P.max(axis=1)
    keep = np.ones(len(best), bool)
    if thr is not None:
        low = prob < thr                      # float32 values against a Python float, as decoding.py compares them
        for s in np.unique(best):
            where = np.flatnonzero(best == s)
            keep[where[:int(low[where].sum())]] = False
    frames = np.flatnonzero(keep)
    out, i = [], 0
    while i < len(frames):
        j = i
        while j + 1 < len(frames) and best[frames[j + 1]] == best[frames[i]]:
            j += 1
        run = (int(best[frames[i]]), int(frames[i]) + skip, int(frames[j]) + skip, float(prob[frames[i:j + 1]].astype(np.float64).mean()))
        out.append(run + (j - i + 1,) if with_count else run)
        i = j + 1
    return out
