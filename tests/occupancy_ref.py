"""fp64 restatement of mgr_ctc_occupancy (plain numpy, no GPU): the forward-backward state posteriors of a label sequence under the loss's
conventions, the quantile extents read off them, and - extents_from_gamma - the float32 sequential restatement of how the kernel forms
the extents from the float32 gamma it writes (the arithmetic include/mgr.h pins).
"""
import itertools

import numpy as np

import align_ref as ar

NEG_INF = -np.inf


def _lse(*xs):
    m = np.maximum.reduce(xs)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = m + np.log(sum(np.exp(x - m) for x in xs))
    return np.where(np.isneginf(m), NEG_INF, r)


def clip_labels(labels, Cn):
    return [min(max(int(l), 0), Cn - 1) for l in labels]


def forward_backward(logy, labels, blank):
    """logy (T, C) fp64 -> (gamma (T, 2 L + 1), logp), or (None, -inf) when no alignment fits (or T = 0)."""
    logy = np.asarray(logy, np.float64)
    T = logy.shape[0]
    ext = ar.extended(labels, blank)
    S = len(ext)
    if T == 0:
        return None, NEG_INF
    can = np.zeros(S, bool)
    can[3::2] = (ext[3::2] != ext[1:-2:2]) & (ext[3::2] != blank)
    em = logy[:, ext]
    alpha = np.full((T, S), NEG_INF)
    alpha[0, 0] = em[0, 0]
    if S > 1:
        alpha[0, 1] = em[0, 1]
    for t in range(1, T):
        a = alpha[t - 1]
        a1 = np.r_[NEG_INF, a[:-1]]
        a2 = np.where(can, np.r_[NEG_INF, NEG_INF, a[:-2]][:S], NEG_INF)
        alpha[t] = em[t] + _lse(a, a1, a2)
    beta = np.full((T, S), NEG_INF)
    beta[T - 1, S - 1] = 0.0
    if S > 1:
        beta[T - 1, S - 2] = 0.0
    can_in = np.r_[can[2:], False, False][:S]     # the step from s over a blank INTO s + 2
    for t in range(T - 2, -1, -1):
        nb = beta[t + 1] + em[t + 1]
        n1 = np.r_[nb[1:], NEG_INF]
        n2 = np.where(can_in, np.r_[nb[2:], NEG_INF, NEG_INF][:S], NEG_INF)
        beta[t] = _lse(nb, n1, n2)
    logp = float(_lse(alpha[T - 1, S - 1], alpha[T - 1, S - 2])) if S > 1 else float(alpha[T - 1, 0])
    if not np.isfinite(logp):
        return None, NEG_INF
    with np.errstate(invalid="ignore"):
        g = np.exp(alpha + beta - logp)
    g = np.where(np.isfinite(g), g, 0.0)
    return g / g.sum(axis=1, keepdims=True), logp


def extents(gamma, n_labels, q, dtype=np.float64, skip=0):
    """gamma (T, S') with S' >= 2 n_labels + 1 -> [(first, last)] per label: cum(t, s) = sum_{s' >= s} gamma(t, s') added one state at a
    time from the last state downwards in `dtype`; first = min{t : cum(t, 2i+1) >= q}, last = max{t : cum(t, 2i+2) <= 1 - q}, q and
    1 - q formed in `dtype`.  -1 where no frame qualifies."""
    g = np.asarray(gamma, dtype)
    qq = dtype(q)
    omq = dtype(1.0) - qq
    cum = np.cumsum(g[:, ::-1], axis=1, dtype=dtype)[:, ::-1]        # (numpy accumulates sequentially: plain adds in this order)
    out = []
    for i in range(n_labels):
        f = np.flatnonzero(cum[:, 2 * i + 1] >= qq)
        l = np.flatnonzero(cum[:, 2 * i + 2] <= omq)
        out.append((int(f[0]) + skip if len(f) else -1, int(l[-1]) + skip if len(l) else -1))
    return out


def extents_from_gamma(gamma_f32, q, n_labels=None, skip=0):
    """The kernel's seg from the kernel's own float32 gamma (T, S): bit for bit."""
    g = np.asarray(gamma_f32)
    assert g.dtype == np.float32
    if n_labels is None:
        n_labels = (g.shape[1] - 1) // 2
    return extents(g, n_labels, np.float32(q), np.float32, skip)


def occupancy(P, labels, input_len=None, q=0.5, skip=2, blank=None, eps=1e-8):
    """One sample, P (T, C) float32 -> dict(gamma (T - skip, 2 L + 1) fp64 zero from input_len on, seg [(first, last)] in original frame
    indices, occ (L,), conf (L,), logp); what does not fit gives logp = -inf, gamma 0, seg -1, occ and conf 0."""
    P = np.asarray(P, np.float32)
    T, Cn = P.shape
    blank = Cn - 1 if blank is None else blank
    lab = clip_labels(labels, Cn)
    L = len(lab)
    To = T - skip
    Tp = To if input_len is None else min(max(int(input_len), 0), To)
    logy = ar.log_emissions(P[:skip + Tp], skip, eps)
    g, logp = forward_backward(logy, lab, blank)
    gamma = np.zeros((To, 2 * L + 1))
    if g is None:
        return dict(gamma=gamma, seg=[(-1, -1)] * L, occ=np.zeros(L), conf=np.zeros(L), logp=NEG_INF)
    gamma[:Tp] = g
    occ = g[:, 1::2].sum(axis=0)
    Pl = np.asarray(P[skip:skip + Tp], np.float64)[:, lab] if L else np.zeros((Tp, 0))
    with np.errstate(invalid="ignore", divide="ignore"):
        conf = np.where(occ > 0, (g[:, 1::2] * Pl).sum(axis=0) / occ, 0.0)
    return dict(gamma=gamma, seg=extents(g, L, q, skip=skip), occ=occ, conf=conf, logp=logp)


def brute_force_gamma(logy, labels, blank):
    """gamma (T, 2 L + 1) by enumerating every state sequence of the lattice (small T only): start in state 0 or 1, end in the last two,
    steps of 0, 1, or 2 - the last only from a label onto a different label."""
    logy = np.asarray(logy, np.float64)
    T = logy.shape[0]
    ext = ar.extended(labels, blank)
    S = len(ext)
    acc = np.zeros((T, S))
    tot = 0.0
    for seq in itertools.product(range(S), repeat=T):
        if seq[0] > 1 or seq[-1] < S - 2:
            continue
        ok = True
        for a, b in zip(seq[:-1], seq[1:]):
            d = b - a
            if d < 0 or d > 2 or (d == 2 and not (b % 2 == 1 and ext[b] != ext[a])):
                ok = False
                break
        if not ok:
            continue
        w = np.exp(sum(logy[t, ext[s]] for t, s in enumerate(seq)))
        tot += w
        acc[np.arange(T), list(seq)] += w
    return (acc / tot if tot > 0 else None), tot
