"""Plain-Python statement of mgr_edit_distance (include/mgr.h) and of what decoding.py builds on it: the DP over
(cost, S, D, I) tuples, the walk that reports one alignment under the header's tie rule, an exhaustive enumerator of all
alignments (the DP's own check), the row filter, and the N-best attainable-error / minimum-Bayes-risk restatements in fp64."""
import numpy as np

COST_SETS = [(1, 1, 1), (10, 7, 7), (4, 3, 3)]
HIT, SUB, DEL, INS = 0, 1, 2, 3


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3])


def steps(costs):
    cs, cd, ci = costs
    return (cs, 1, 0, 0), (cd, 0, 1, 0), (ci, 0, 0, 1)


def tuple_dp(h, r, costs):
    """The full table of lexicographically smallest (cost, S, D, I): d[i][j] aligns h[:i] to r[:j]."""
    ks, kd, ki = steps(costs)
    m, n = len(h), len(r)
    d = [[None] * (n + 1) for _ in range(m + 1)]
    d[0][0] = (0, 0, 0, 0)
    for j in range(1, n + 1):
        d[0][j] = _add(d[0][j - 1], kd)
    for i in range(1, m + 1):
        d[i][0] = _add(d[i - 1][0], ki)
        for j in range(1, n + 1):
            diag = d[i - 1][j - 1] if h[i - 1] == r[j - 1] else _add(d[i - 1][j - 1], ks)
            d[i][j] = min(diag, _add(d[i][j - 1], kd), _add(d[i - 1][j], ki))
    return d


def align(h, r, costs):
    """(dist, (H, S, D, I), ops): ops in forward order, the walk back from (m, n) that takes at each cell the first of diagonal,
    deletion, insertion whose predecessor tuple plus the step's tuple equals the cell's tuple."""
    ks, kd, ki = steps(costs)
    d = tuple_dp(h, r, costs)
    i, j, ops = len(h), len(r), []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and (d[i - 1][j - 1] if h[i - 1] == r[j - 1] else _add(d[i - 1][j - 1], ks)) == d[i][j]:
            ops.append(HIT if h[i - 1] == r[j - 1] else SUB)
            i, j = i - 1, j - 1
        elif j > 0 and _add(d[i][j - 1], kd) == d[i][j]:
            ops.append(DEL)
            j -= 1
        else:
            assert i > 0 and _add(d[i - 1][j], ki) == d[i][j]
            ops.append(INS)
            i -= 1
    c, S, D, I = d[len(h)][len(r)]
    return c, (len(r) - S - D, S, D, I), ops[::-1]


def enumerate_best(h, r, costs):
    """The smallest (cost, S, D, I) over ALL monotone alignments, by recursion over every choice (tiny inputs only)."""
    ks, kd, ki = steps(costs)

    def rec(i, j):
        if i == len(h) and j == len(r):
            yield (0, 0, 0, 0)
            return
        if i < len(h) and j < len(r):
            st = (0, 0, 0, 0) if h[i] == r[j] else ks
            for t in rec(i + 1, j + 1):
                yield _add(st, t)
        if j < len(r):
            for t in rec(i, j + 1):
                yield _add(kd, t)
        if i < len(h):
            for t in rec(i + 1, j):
                yield _add(ki, t)

    return min(rec(0, 0))


def replay(h, r, ops, costs):
    """Run an alignment over h and r: (consumed both exactly, cost, (H, S, D, I))."""
    i = j = cost = 0
    cnt = [0, 0, 0, 0]
    for o in ops:
        o = int(o)
        if o in (HIT, SUB):
            if i >= len(h) or j >= len(r) or (h[i] == r[j]) != (o == HIT):
                return False, None, None
            i, j = i + 1, j + 1
        elif o == DEL:
            j += 1
        elif o == INS:
            i += 1
        else:
            return False, None, None
        cnt[o] += 1
        cost += (0, costs[0], costs[1], costs[2])[o]
    return i == len(h) and j == len(r), cost, tuple(cnt)


def filter_row(row, length=None, ignore_mask=0):
    """What the kernel compares of a padded row: the first clip(length) entries without those < 0 and those in the mask."""
    row = [int(v) for v in row]
    k = len(row) if length is None else max(0, min(int(length), len(row)))
    return [v for v in row[:k] if v >= 0 and not (v < 64 and (ignore_mask >> v) & 1)]


def kernel_ref(hyp, hyp_len, ref, ref_len, pair_h, pair_r, costs, ignore_mask=0):
    """mgr_edit_distance on host arrays: dist (P,), counts (P, 4), lens (P, 2), n_ops (P,), ops (P, Lh + Lr) int8 padded -1."""
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    P = hyp.shape[0] if pair_h is None else len(pair_h)
    W = hyp.shape[1] + ref.shape[1]
    dist, counts, lens = np.zeros(P, np.int32), np.zeros((P, 4), np.int32), np.zeros((P, 2), np.int32)
    n_ops, ops = np.zeros(P, np.int32), -np.ones((P, W), np.int8)
    memo = {}
    for p in range(P):
        a, b = (p, p) if pair_h is None else (int(pair_h[p]), int(pair_r[p]))
        h = filter_row(hyp[a], None if hyp_len is None else hyp_len[a], ignore_mask)
        r = filter_row(ref[b], None if ref_len is None else ref_len[b], ignore_mask)
        key = (tuple(h), tuple(r))
        if key not in memo:
            memo[key] = align(h, r, costs)
        c, cnt, o = memo[key]
        dist[p], counts[p], lens[p], n_ops[p] = c, cnt, (len(h), len(r)), len(o)
        ops[p, :len(o)] = o
    return dist, counts, lens, n_ops, ops


def nbest_attainable_ref(paths, refs, costs=(1, 1, 1)):
    """Per sample the smallest distance over its hypotheses and the first rank that attains it (none: the empty hypothesis, -1)."""
    best, rank = [], []
    for hyps, r in zip(paths, refs):
        r = [int(v) for v in r if v >= 0]
        d = [align(list(h), r, costs)[0] for h in hyps]
        if d:
            k = min(range(len(d)), key=lambda q: (d[q], q))
            best.append(d[k])
            rank.append(k)
        else:
            best.append(align([], r, costs)[0])
            rank.append(-1)
    den = sum(len([v for v in r if v >= 0]) for r in refs)
    return np.asarray(best, np.int64), np.asarray(rank, np.int64), sum(best) / max(1, den)


def mbr_ref(paths, scores, scale=1.0, costs=(1, 1, 1)):
    """(picks, ranks, risk (N, NP) with +inf, gap (N,)): gap = the difference of the two smallest risks (+inf with one hypothesis)."""
    import math
    scores = np.asarray(scores, np.float64).reshape(len(paths), -1)
    NP = scores.shape[1]
    risk = np.full((len(paths), NP), np.inf)
    picks, ranks, gaps = [], [], []
    for b, hyps in enumerate(paths):
        K = len(hyps)
        if K == 0:
            picks.append([])
            ranks.append(-1)
            gaps.append(np.inf)
            continue
        z = [float(scale) * float(scores[b, k]) for k in range(K)]
        zm = max(z)
        w = [math.exp(v - zm) for v in z]
        tot = math.fsum(w)
        for k in range(K):
            risk[b, k] = math.fsum(w[j] / tot * align(list(hyps[k]), list(hyps[j]), costs)[0] for j in range(K))
        order = sorted(range(K), key=lambda q: (risk[b, q], q))
        ranks.append(order[0])
        picks.append(list(hyps[order[0]]))
        gaps.append(risk[b, order[1]] - risk[b, order[0]] if K > 1 else np.inf)
    return picks, np.asarray(ranks, np.int64), risk, np.asarray(gaps)


def packed_form(h, r, costs, lanes=64):
    """The form csrc/edit.hip computes in, restated with Python integers: tuples packed as cost << 36 | S << 24 | D << 12 | I, a
    row kept as e[j] = d[i][j] - j * K_del, so that a row is c[j] = min(e'[j] + K_ins, e'[j - 1] - K_del + (K_sub or 0)) followed
    by a prefix minimum - formed as the kernel forms it: per lane over its cpl = ceil((n + 1) / lanes) contiguous columns, an
    exclusive scan of the lane minima, a second pass.  Returns (dist, (H, S, D, I), ops) like align()."""
    cs, cd, ci = costs
    Ks, Kd, Ki = (cs << 36) | (1 << 24), (cd << 36) | (1 << 12), (ci << 36) | 1
    m, n = len(h), len(r)
    cpl = (n + 1 + lanes - 1) // lanes
    ncol = lanes * cpl
    INF = (1 << 63) - 1
    rl = [r[j - 1] if 1 <= j <= n else -2 for j in range(ncol)]
    e = [0] * ncol
    bp = []
    for i in range(1, m + 1):
        hi = h[i - 1]

        def cands(j):
            diag = INF if j == 0 else e[j - 1] - Kd + (0 if rl[j] == hi else Ks)
            return diag, e[j] + Ki

        loc = [min(min(cands(l * cpl + k)) for k in range(cpl)) for l in range(lanes)]
        excl = [INF] * lanes
        for l in range(1, lanes):
            excl[l] = min(excl[l - 1], loc[l - 1])
        new, row = [0] * ncol, [0] * ncol
        for l in range(lanes):
            run = excl[l]
            for k in range(cpl):
                j = l * cpl + k
                diag, ins = cands(j)
                v = min(diag, ins, run)
                row[j] = (HIT if rl[j] == hi else SUB) if diag == v else (DEL if run == v else INS)
                new[j] = run = v
        e = new
        bp.append(row)
    d = e[n] + n * Kd
    cost, S, D, I = d >> 36, (d >> 24) & 4095, (d >> 12) & 4095, d & 4095
    i, j, ops = m, n, []
    while i > 0 or j > 0:
        op = DEL if i == 0 else (INS if j == 0 else bp[i - 1][j])
        ops.append(op)
        i -= op != DEL
        j -= op != INS
    return cost, (n - S - D, S, D, I), ops[::-1]
