"""fp64 numpy restatement of the joint decode over several CTC streams (mgr_ctc_joint_decode, K19): the label-synchronous
prefix search of include/mgr.h, operation for operation - the same lse formula, the same order of the sums that make a rank, the same
tie rules, the same stop - and, beside the result, the smallest DECISION MARGIN of the run: the smallest gap between two numbers whose
order decides something.  A test proves with it that its inputs are no near-ties before it asks a kernel for equal sequences.

The recursion exists twice: extend() is the definition one frame and one class at a time (what the enumeration tests hold against
brute force), run_round runs a whole round's candidates at once - one numpy lse per frame over (candidates x words) - so
that T = 1900 takes seconds."""
import itertools
import math

import numpy as np

NEG = float("-inf")


# ---- the definition, scalar ----------------------------------------------------------------------------------------------------------
def lse(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = a if a > b else b
    return m + math.log1p(math.exp(-abs(a - b)))


def log_emissions(P, skip, eps, input_len=None):
    """P (T, C) float32 -> ln y (Tp, C) float64 over the frames skip .. skip + Tp - 1, as the kernel forms them: eps is the C ABI's
    float, widened."""
    To = P.shape[0] - skip
    Tp = To if input_len is None else max(0, min(int(input_len), To))
    u = P[skip:skip + Tp].astype(np.float64) + np.float64(np.float32(eps))
    with np.errstate(divide="ignore"):
        return np.log(u) - np.log(u.sum(axis=1, keepdims=True))


def empty_prefix(ly, blank):
    T = len(ly)
    return np.full(T, NEG), (np.cumsum(ly[:, blank]) if T else np.zeros(0))


def extend(ly, blank, gn, gb, last, c):
    """One class c appended to the prefix with arrays gn, gb and last class `last` (None: the empty prefix).  Returns (gn_h, gb_h,
    ln psi)."""
    T = len(ly)
    hn, hb, psi = np.full(T, NEG), np.full(T, NEG), NEG
    if T == 0:
        return hn, hb, psi
    hn[0] = ly[0, c] if last is None else NEG
    psi = hn[0]
    for t in range(1, T):
        phi = lse(gb[t - 1], gn[t - 1] if last != c else NEG)
        hn[t] = lse(hn[t - 1], phi) + ly[t, c]
        hb[t] = lse(hb[t - 1], hn[t - 1]) + ly[t, blank]
        psi = lse(psi, phi + ly[t, c])
    return hn, hb, psi


def complete(gn, gb):
    return 0.0 if len(gn) == 0 else lse(gn[-1], gb[-1])


def prefix_scores(ly, blank, classes):
    """(ln p, ln psi) of the class sequence by chained extensions; the empty sequence has psi = 1."""
    gn, gb = empty_prefix(ly, blank)
    last, psi = None, 0.0
    for c in classes:
        gn, gb, psi = extend(ly, blank, gn, gb, last, c)
        last = c
    if len(ly) == 0:
        return (0.0 if not len(classes) else NEG), psi
    return complete(gn, gb), psi


def collapse(path, blank):
    return tuple(k for k, _ in itertools.groupby(path) if k != blank)


def brute_force(ly, blank, classes, prefix=False):
    """ln of the summed probability of all frame paths whose labelling equals (prefix: begins with) `classes`."""
    T, C = ly.shape
    classes, tot = tuple(classes), NEG
    for path in itertools.product(range(C), repeat=T):
        lab = collapse(path, blank)
        if (lab[:len(classes)] if prefix else lab) == classes:
            tot = lse(tot, float(sum(ly[t, c] for t, c in enumerate(path))))
    return tot


# ---- a round's candidates of one stream at once ---------------------------------------------------------------------------------------
def vlse(a, b):
    """lse over arrays (call under np.errstate(invalid="ignore")): with one side -inf the formula gives the other side exactly
    (m + log1p(0)), as the scalar form returns it; with both it gives NaN, put back to -inf."""
    m = np.maximum(a, b)
    r = m + np.log1p(np.exp(-np.abs(a - b)))
    return np.where(m == NEG, NEG, r)


def words_of(stream, g):
    return stream["lex"][g] if stream["lex"] is not None else [g]


def _setup(stream, parents, cands):
    """The arrays of one stream's candidates: classes (n, W) padded with the blank, which words exist, the prefix' rows."""
    ly, blank = stream["ly"], stream["blank"]
    Tp, n = len(ly), len(cands)
    wl = [words_of(stream, g) for _, g in cands]
    nw = np.array([len(w) for w in wl], np.int64)
    W = int(nw.max())
    cls = np.full((n, W), blank, np.int64)
    for i, w in enumerate(wl):
        cls[i, :len(w)] = w
    plast = np.array([-1 if parents[r] is None else parents[r][2] for r, _ in cands])
    PN, PB = np.full((Tp, n), NEG), np.full((Tp, n), NEG)
    for r in sorted(set(r for r, _ in cands if parents[r] is not None)):
        sel = np.array([rr == r for rr, _ in cands])
        PN[:, sel] = parents[r][0][:, None]
        PB[:, sel] = parents[r][1][:, None]
    return dict(n=n, W=W, nw=nw, cls=cls, same=cls == np.concatenate([plast[:, None], cls[:, :-1]], axis=1),
                empty=np.array([parents[r] is None for r, _ in cands]), PN=PN, PB=PB, E=ly[:, cls],
                EB=np.repeat(ly[:, blank][:, None], n, axis=1), dead=np.array([stream["lex"] is None and g == blank for _, g in cands]))


def _pad(a, W, fill):
    """(.., n, w) -> (.., n, W)"""
    if a.shape[-1] == W:
        return a
    out = np.full(a.shape[:-1] + (W,), fill, a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def run_round(jobs):
    """jobs: list of (stream dict(ly (Tp, C), blank, lex), parents, cands) - parents: per live prefix None (the empty one) or (gn
    (Tp,), gb (Tp,), last class); cands: list of (r, g).  Per job (psi (n,), lnp (n,), GN (Tp, n), GB (Tp, n)): every candidate's
    prefix and complete log-probability and its arrays.  A gesture that is the stream's blank has probability 0.  Jobs with the same
    number of frames run as ONE set of chains (the chains are independent: what is computed per chain does not depend on the set)."""
    res = [None] * len(jobs)
    groups = {}
    for i, (stream, parents, cands) in enumerate(jobs):
        Tp, n = len(stream["ly"]), len(cands)
        if Tp == 0 or n == 0:
            res[i] = (np.full(n, NEG), np.full(n, NEG), np.full((Tp, n), NEG), np.full((Tp, n), NEG))
        else:
            groups.setdefault(Tp, []).append(i)
    for Tp, members in groups.items():
        ss = [_setup(*jobs[i]) for i in members]
        W = max(q["W"] for q in ss)
        cat = lambda k, ax=0: np.concatenate([q[k] for q in ss], axis=ax)
        nw, empty, dead = cat("nw"), cat("empty"), cat("dead")
        same = np.concatenate([_pad(q["same"], W, False) for q in ss])
        E = np.concatenate([_pad(q["E"], W, 0.0) for q in ss], axis=1)
        PN, PB, EB = cat("PN", 1), cat("PB", 1), cat("EB", 1)
        n = len(nw)
        on = np.arange(W)[None, :] < nw[:, None]
        rows, lastw = np.arange(n), nw - 1
        EL = E[:, rows, lastw]              # (Tp, n): the last word's emissions
        cumb = np.cumsum(EB, axis=0)
        GN, GB = np.full((Tp, n), NEG), np.full((Tp, n), NEG)
        hn, hb = np.full((n, W), NEG), np.full((n, W), NEG)
        hn[:, 0] = np.where(empty, E[0, :, 0], NEG)
        ps = np.where(nw == 1, hn[:, 0], NEG)
        GN[0] = ps
        same0, same1 = same[:, 0], same[:, 1:]
        phi = np.empty((n, W))
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(1, Tp):
                phi[:, 0] = np.where(empty, cumb[t - 1], vlse(PB[t - 1], np.where(same0, NEG, PN[t - 1])))
                if W > 1:
                    phi[:, 1:] = vlse(hb[:, :-1], np.where(same1, NEG, hn[:, :-1]))
                nn = np.where(on, vlse(hn, phi) + E[t], NEG)
                nb = np.where(on, vlse(hb, hn) + EB[t][:, None], NEG)
                ps = vlse(ps, phi[rows, lastw] + EL[t])
                hn, hb = nn, nb
                GN[t], GB[t] = hn[rows, lastw], hb[rows, lastw]
            lnp = np.where(dead, NEG, vlse(GN[-1], GB[-1]))
        psi = np.where(dead, NEG, ps)
        at = 0
        for i, q in zip(members, ss):
            sl = slice(at, at + q["n"])
            res[i] = (psi[sl], lnp[sl], GN[:, sl], GB[:, sl])
            at += q["n"]
    return res


def search(streams, G, ext=None, fin=None, beam=10, top_paths=1, max_len=8, early=True):
    """One sample.  streams: list of dict(ly, blank, lex, w).  ext (G + 1, G) / fin (G + 1,) or None.  Returns a dict: paths (best
    first), score, logp (per path the streams' ln p), rounds, margin."""
    M = len(streams)
    ext = np.zeros((G + 1, G)) if ext is None else np.asarray(ext, np.float64).reshape(G + 1, G)
    fin = None if fin is None else np.asarray(fin, np.float64).reshape(G + 1)
    finite_ext = ext[np.isfinite(ext)]
    u_ext = max(0.0, float(finite_ext.max())) if finite_ext.size else 0.0
    u_fin = 0.0
    if fin is not None and np.isfinite(fin).any():
        u_fin = max(0.0, float(fin[np.isfinite(fin)].max()))
    margin = float("inf")
    found = []          # (score, seq, [ln p_m]) in arrival order
    lp0 = [float(np.sum(np.cumsum(s["ly"][:, s["blank"]])[-1:])) for s in streams]      # the sequential sum, as the kernel adds
    sc = 0.0
    for m in range(M):
        sc += streams[m]["w"] * lp0[m]
    sc += 0.0
    if fin is not None:
        sc += fin[0]
    if sc > NEG:
        found.append((sc, (), lp0))
    live = [dict(seq=(), lm=0.0, last=-1, arrays=[None] * M)]
    rounds = 0
    for n in range(1, max_len + 1):
        rounds = n
        cands = [(r, g) for r, b in enumerate(live) for g in range(G) if ext[b["last"] + 1, g] != NEG]
        per = run_round([(streams[m], [b["arrays"][m] for b in live], cands) for m in range(M)])
        pre = np.zeros(len(cands))
        for m in range(M):
            with np.errstate(invalid="ignore"):
                pre = pre + streams[m]["w"] * per[m][0]
        lm = np.array([live[r]["lm"] + ext[live[r]["last"] + 1, g] for r, g in cands]) if cands else np.zeros(0)
        pre = pre + lm
        order = [i for i in sorted(range(len(cands)), key=lambda i: (-pre[i], i)) if pre[i] > NEG]
        if len(order) > beam:
            margin = min(margin, pre[order[beam - 1]] - pre[order[beam]])
        kept = order[:beam]
        new = []
        for i in kept:
            r, g = cands[i]
            fl = 0.0
            for m in range(M):
                fl += streams[m]["w"] * per[m][1][i]
            fl += lm[i]
            if fin is not None:
                fl += fin[g + 1]
            if fl > NEG:
                found.append((float(fl), live[r]["seq"] + (g,), [float(per[m][1][i]) for m in range(M)]))
            arrays = []
            for m in range(M):
                s = streams[m]
                arrays.append((per[m][2][:, i].copy(), per[m][3][:, i].copy(), words_of(s, g)[-1]))
            new.append(dict(seq=live[r]["seq"] + (g,), lm=float(lm[i]), last=g, arrays=arrays, pre=float(pre[i])))
        live = new
        if not live or n == max_len:
            break
        if len(found) >= top_paths:
            worst = sorted((f[0] for f in found), reverse=True)[top_paths - 1]
            bound = live[0]["pre"] + ((max_len - n) * u_ext + u_fin)
            margin = min(margin, abs(worst - bound))
            if early and bound < worst:
                break
    idx = sorted(range(len(found)), key=lambda i: (-found[i][0], i))
    for a, b in zip(idx[:top_paths], idx[1:top_paths + 1]):
        margin = min(margin, found[a][0] - found[b][0])
    idx = idx[:top_paths]
    return dict(paths=[list(found[i][1]) for i in idx], score=[found[i][0] for i in idx], logp=[found[i][2] for i in idx], rounds=rounds,
                margin=margin)


def prepare(case, b):
    """The streams of sample b of a case of joint_cases.py, with their emissions."""
    out = []
    for s in case["streams"]:
        il = None if s.get("il") is None else s["il"][b]
        out.append(dict(ly=log_emissions(s["P"][b], s["skip"], s["eps"], il), blank=s["blank"],
                        lex=None if s.get("lexicon") is None else [list(p) for p in s["lexicon"]], w=float(s["weight"])))
    return out


def decode_case(case, early=True):
    """A whole case -> the arrays mgr_ctc_joint_decode writes (out, out_len, score, logp, rounds) and the smallest margin."""
    B, M = case["streams"][0]["P"].shape[0], len(case["streams"])
    NP, L = case["top_paths"], case["max_len"]
    out, out_len = -np.ones((B, NP, L), np.int32), -np.ones((B, NP), np.int32)
    score, logp = np.full((B, NP), NEG), np.full((B, NP, M), NEG)
    rounds, margin = np.zeros(B, np.int32), float("inf")
    for b in range(B):
        r = search(prepare(case, b), case["G"], case.get("ext"), case.get("fin"), case["beam"], NP, L, early)
        for k, p in enumerate(r["paths"]):
            out[b, k, :len(p)] = p
            out_len[b, k] = len(p)
            score[b, k] = r["score"][k]
            logp[b, k] = r["logp"][k]
        rounds[b] = r["rounds"]
        margin = min(margin, r["margin"])
    return out, out_len, score, logp, rounds, margin


def table_terms(seq, G, ext=None, fin=None):
    """sum_i ext[prev_i + 1, g_i] + fin[g_n + 1], the definition's table part."""
    t, prev = 0.0, 0
    for g in seq:
        if ext is not None:
            t += float(np.asarray(ext).reshape(G + 1, G)[prev, g])
        prev = g + 1
    if fin is not None:
        t += float(np.asarray(fin).reshape(G + 1)[prev])
    return t
