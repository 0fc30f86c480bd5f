"""fp64 restatement of mgr_ctc_entropy_grad's entropy term (plain numpy, no GPU): the entropy H = - sum_pi q(pi) ln q(pi) of
q(pi) = p(pi) / Z over the alignments pi of a label sequence, Z = p(labels | x), and its gradient, under the loss's conventions (frames
skip .., u = ln y, y = (P + eps) / sum (P + eps), states l' = [blank, l_1, blank, ..., l_L, blank]).

H = ln Z - m, m = E_q[ln p(pi)].  Beside alpha runs a(t, s) = E[ln p(pi_0..t) | the prefix ends in s at t] = u(t, l'_s) + sum_r w_r
a(t - 1, r) over alpha's predecessors r with the weights w_r = alpha(t - 1, r) / sum alpha(t - 1, .); beside beta (which, as in
tests/occupancy_ref.py, leaves frame t's own emission out) b(t, s) = E[ln p(pi_t+1..) | the suffix starts in s at t].  With c = a + b and
gamma the state posteriors, sum_s gamma(t, s) c(t, s) = m at every t and dH/du(t, k) = -(sum_{s: l'_s = k} gamma c - gamma_k(t) m).
A predecessor of weight 0 is left out (its a may be -inf); a dead state keeps a = b = 0.

enumerate_paths restates the same quantities from the definition, path by path (small lattices only).  ascent_inputs are the planted
inputs of the ascent tests (tests/test_cpu_entropy.py fixes ASCENT_LR on them, tests/test_gpu_entropy.py takes the kernel's own step).
"""
import numpy as np

import align_ref as ar
import occupancy_ref as oc

NEG_INF = -np.inf


def _weights(terms):
    """terms (R, S) log-values -> (lse (S,), weights (R, S) summing to 1 where any term is alive, else 0)"""
    m = terms.max(axis=0)
    live = ~np.isneginf(m)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(live, np.exp(terms - np.where(live, m, 0.0)), 0.0)
        s = e.sum(axis=0)
        return np.where(live, m + np.log(s), NEG_INF), np.where(live, e / np.where(live, s, 1.0), 0.0)


def _mean(w, x):
    """sum_r w_r x_r with the terms of weight 0 left out"""
    return np.where(w > 0, w * np.where(w > 0, x, 0.0), 0.0).sum(axis=0)


def lattice(logy, labels, blank):
    """logy (T, C) fp64 -> dict(logp, m, H, gamma (T, S), c (T, S), mt (T,), dHdu (T, C)), or None when no alignment fits (or T = 0)."""
    logy = np.asarray(logy, np.float64)
    T, Cn = logy.shape
    ext = ar.extended(labels, blank)
    S = len(ext)
    if T == 0:
        return None
    can = np.zeros(S, bool)
    can[3::2] = (ext[3::2] != ext[1:-2:2]) & (ext[3::2] != blank)
    can_in = np.r_[can[2:], False, False][:S]
    em = logy[:, ext]
    sh1 = lambda v, fill: np.r_[fill, v[:-1]]
    sh2 = lambda v, fill: np.r_[fill, fill, v[:-2]][:S]
    up1 = lambda v, fill: np.r_[v[1:], fill]
    up2 = lambda v, fill: np.r_[v[2:], fill, fill][:S]
    alpha, a = np.full((T, S), NEG_INF), np.zeros((T, S))
    alpha[0, :2] = em[0, :2]
    a[0, :2] = np.where(np.isneginf(em[0, :2]), 0.0, em[0, :2])
    for t in range(1, T):
        p = alpha[t - 1]
        lse, w = _weights(np.stack([p, sh1(p, NEG_INF), np.where(can, sh2(p, NEG_INF), NEG_INF)]))
        alpha[t] = em[t] + lse
        x = a[t - 1]
        with np.errstate(invalid="ignore"):
            v = em[t] + _mean(w, np.stack([x, sh1(x, 0.0), sh2(x, 0.0)]))
        a[t] = np.where(np.isneginf(alpha[t]), 0.0, v)
    beta, bx = np.full((T, S), NEG_INF), np.zeros((T, S))
    beta[T - 1, max(S - 2, 0):] = 0.0
    for t in range(T - 2, -1, -1):
        nb = beta[t + 1] + em[t + 1]
        with np.errstate(invalid="ignore"):
            z = np.where(np.isneginf(nb), 0.0, bx[t + 1] + em[t + 1])
        beta[t], w = _weights(np.stack([nb, up1(nb, NEG_INF), np.where(can_in, up2(nb, NEG_INF), NEG_INF)]))
        bx[t] = np.where(np.isneginf(beta[t]), 0.0, _mean(w, np.stack([z, up1(z, 0.0), up2(z, 0.0)])))
    fin = alpha[T - 1, max(S - 2, 0):]
    logp, wf = _weights(fin[:, None])
    logp = float(logp[0])
    if not np.isfinite(logp):
        return None
    m = float(_mean(wf, a[T - 1, max(S - 2, 0):][:, None])[0])
    with np.errstate(invalid="ignore"):
        g = np.exp(alpha + beta - logp)
    g = np.where(np.isfinite(g), g, 0.0)
    g = g / g.sum(axis=1, keepdims=True)
    c = a + bx
    gc = g * c
    mt = gc.sum(axis=1)
    occ, occ_c = np.zeros((T, Cn)), np.zeros((T, Cn))
    for s in range(S):
        occ[:, ext[s]] += g[:, s]
        occ_c[:, ext[s]] += gc[:, s]
    return dict(logp=logp, m=m, H=logp - m, gamma=g, c=c, mt=mt, dHdu=-(occ_c - occ * mt[:, None]), occ=occ)


def entropy(P, labels, input_len=None, skip=2, blank=None, eps=1e-8):
    """One sample, P (T, C) (float32 as the kernel reads it, or fp64 for differences) -> dict(H, logp, m, mt (T',), dHdu (T', C), dlogits
    (T, C)): dlogits = dH / d(Dense logits) through y = softmax(log(P + eps)) and P = softmax(logits), zero on dropped and out-of-length
    frames.  What does not fit, and no frames at all: H = 0, logp = -inf, a zero gradient.  Labels are clipped into the class range."""
    P = np.asarray(P)
    T, Cn = P.shape
    blank = Cn - 1 if blank is None else blank
    lab = oc.clip_labels(labels, Cn)
    To = T - skip
    Tp = To if input_len is None else min(max(int(input_len), 0), To)
    P64 = np.asarray(P, np.float64)
    r = lattice(ar.log_emissions(P64[:skip + Tp], skip, eps), lab, blank)
    dz = np.zeros((T, Cn))
    if r is None:
        return dict(H=0.0, logp=NEG_INF, m=0.0, mt=np.zeros(Tp), dHdu=np.zeros((Tp, Cn)), dlogits=dz)
    rows = P64[skip:skip + Tp]
    u = rows + np.float64(np.float32(eps))
    with np.errstate(invalid="ignore", divide="ignore"):
        gp = np.where(u > 0, r["dHdu"] / u, 0.0)       # (the rows of dH/du sum to zero: the normaliser of y takes no part)
    dz[skip:skip + Tp] = rows * (gp - (rows * gp).sum(axis=1, keepdims=True))
    r = dict(r, dlogits=dz)
    return r


def batch(P, labels, il, ll, skip=2, blank=None, eps=1e-8):
    """A batch as the kernel takes it (lengths clipped) -> (H (B,), m (B,), dlogits (B, T, C), logp (B,))"""
    B, T, Cn = P.shape
    Lmax = labels.shape[1]
    out = [entropy(P[b], labels[b, :min(max(int(ll[b]), 0), Lmax)], il[b], skip, blank, eps) for b in range(B)]
    return (np.array([o["H"] for o in out]), np.array([o["m"] for o in out]), np.stack([o["dlogits"] for o in out]),
            np.array([o["logp"] for o in out]))


def enumerate_paths(logy, labels, blank):
    """Every alignment of the labels (state sequences of the lattice: start in state 0 or 1, end in the last two, steps of 0, 1, or - from
    a label onto a different label - 2), one at a time: dict(n, logp, m, H, dHdu (T, C)) from the definitions, paths of probability 0
    contributing 0; None when no path has probability > 0."""
    logy = np.asarray(logy, np.float64)
    T, Cn = logy.shape
    ext = ar.extended(labels, blank)
    S = len(ext)
    paths = []

    def walk(seq):
        s = seq[-1]
        if len(seq) == T:
            if s >= S - 2:
                paths.append(tuple(seq))
            return
        for d in (0, 1, 2):
            n = s + d
            if n >= S or (d == 2 and not (n % 2 == 1 and ext[n] != ext[s])):
                continue
            walk(seq + [n])
    for s0 in range(min(2, S)):
        walk([s0])
    lp = np.array([sum(logy[t, ext[s]] for t, s in enumerate(p)) for p in paths])
    live = np.isfinite(lp)
    if not live.any():
        return None
    logp = float(np.log(np.exp(lp[live]).sum()))
    q = np.where(live, np.exp(np.where(live, lp, 0.0) - logp), 0.0)
    lq = np.where(live, np.where(live, lp, 0.0) - logp, 0.0)
    H = float(-(q * lq).sum())
    m = float((q * np.where(live, lp, 0.0)).sum())
    occ, occ_lp = np.zeros((T, Cn)), np.zeros((T, Cn))
    for p, qq, l in zip(paths, q, np.where(live, lp, 0.0)):
        for t, s in enumerate(p):
            occ[t, ext[s]] += qq
            occ_lp[t, ext[s]] += qq * l
    return dict(n=len(paths), logp=logp, m=m, H=H, dHdu=-(occ_lp - occ * m))


# ---- the planted inputs of the ascent tests ----------------------------------------------------------------------------------------
ASCENT_SKIP, ASCENT_EPS = 2, 1e-8
# z + ASCENT_LR * dH/dz: fixed in tests/test_cpu_entropy.py (the restatement's H rises by far more than float32 resolves on every sample
# with a gradient), used unchanged in tests/test_gpu_entropy.py
ASCENT_LR = 2.0


def softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def ascent_inputs():
    """(z (B, T, C) fp64 logits, labels (B, Lmax) int32, il, ll): logits peaked (+4) along a planted alignment of each sample's labels - a
    CTC-trained network's posteriors in small - for label rows with repeats, one label, no label (one alignment: H = 0, no gradient) and
    a row that does not fit its input (no gradient)."""
    rng = np.random.default_rng(17)
    B, T, Cn, Lmax = 5, 34, 6, 7
    rows = [[0, 1, 1, 3, 2, 0, 4], [2], [], [1, 1, 1, 1], [3, 0, 3]]
    il = np.array([T - ASCENT_SKIP, 20, T - ASCENT_SKIP, 6, 27], np.int32)      # (row 3: four equal labels need 7 frames)
    z = rng.standard_normal((B, T, Cn))
    lab = -np.ones((B, Lmax), np.int32)
    for b, r in enumerate(rows):
        lab[b, :len(r)] = r
        if b != 3:
            states = ar.planted_alignment(rng, int(il[b]), r, Cn - 1)
            cls = ar.extended(r, Cn - 1)[np.asarray(states)]
            z[b, ASCENT_SKIP + np.arange(il[b]), cls] += 4.0
    return z, lab, il, np.array([len(r) for r in rows], np.int32)
