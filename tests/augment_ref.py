"""numpy restatement of mgr_augment_plan / mgr_augment_apply (csrc/augment.hip; test infrastructure, NOT product code and not
imported from it).  The plan is integers drawn with tests/update_ref.py's rand_u32 on np.uint64; the apply step is float32 with
the four operations (divide, subtract, multiply, add) rounded one by one, as the kernel's explicit intrinsics are.

Plan row (include/mgr.h): [0 .. K] the targets q_j, [K + 1] the dropped stream or -1, then per stream n_t (start, width) time
masks and n_f (start, width) feature masks.  Entry p of sample b is drawn at index b * len + p."""
import numpy as np

from tests import update_ref as ur

U64 = np.uint64


def plan_len(S, K, n_t, n_f):
    return K + 2 + 2 * S * (n_t + n_f)


def drop_thresh(p):
    return int(float(p) * 16777216.0)


def sources(T, K):
    """a_0 .. a_K."""
    return np.array([j * (T - 1) // K for j in range(K + 1)], np.int64)


def _draw(seed, idx, lo, hi):
    """Integers in [lo, hi] (arrays broadcast) from the draws at `idx`."""
    u = ur.rand_u32(seed, idx).astype(U64)
    span = (np.asarray(hi, np.int64) - np.asarray(lo, np.int64) + 1).astype(U64)
    return np.asarray(lo, np.int64) + ((u * span) >> U64(32)).astype(np.int64)


def plan_ref(B, T, streams, K, D, n_t, n_f, thresh, seed):
    """streams: [(F, time masks used, Wt, feature masks used, Wf)] per stream.  Returns int32 [B, len]."""
    S = len(streams)
    n = plan_len(S, K, n_t, n_f)
    plan = np.zeros((B, n), np.int64)
    base = np.arange(B, dtype=U64) * U64(n)
    a = sources(T, K)
    for j in range(K + 1):
        plan[:, j] = a[j]
        if 0 < j < K and D > 0:
            plan[:, j] += _draw(seed, base + U64(j), -D, D)
    plan[:, K + 1] = -1
    if thresh > 0:
        r = (ur.rand_u32(seed, base + U64(K + 1)) >> np.uint32(8)).astype(U64)
        hit = r < U64(thresh)
        plan[hit, K + 1] = ((r[hit] * U64(S)) // U64(thresh)).astype(np.int64)
    p = K + 2
    for F, nt, wt, nf, wf in streams:
        for m in range(n_t + n_f):
            time = m < n_t
            used, wmax, axis = (nt, wt, T) if time else (nf, wf, F)
            if (m if time else m - n_t) < used:
                width = _draw(seed, base + U64(p + 1), 0, wmax)
                plan[:, p + 1] = width
                plan[:, p] = _draw(seed, base + U64(p), 0, axis - width)
            p += 2
    return plan.astype(np.int32)


def frames(row, T, K):
    """(i0, rem, den) for every output frame t of one plan row: the first segment j with t <= q_{j+1}."""
    q = np.asarray(row[:K + 1], np.int64)
    a = sources(T, K)
    t = np.arange(T, dtype=np.int64)
    j = np.searchsorted(q[1:K], t, side="left")          # how many inner targets lie below t
    den = q[j + 1] - q[j]
    num = (t - q[j]) * (a[j + 1] - a[j])
    safe = np.maximum(den, 1)
    i0 = np.where(den > 0, a[j] + num // safe, a[j])
    rem = np.where(den > 0, num % safe, 0)
    return i0, rem, den


def time_blank(row, T, K, n_t, n_f, S, si):
    """bool [T]: frames of stream si this row blanks (its time masks, or the whole stream when it is the dropped one)."""
    out = np.full(T, int(row[K + 1]) == si)
    off = K + 2 + si * 2 * (n_t + n_f)
    t = np.arange(T)
    for m in range(n_t):
        st, w = int(row[off + 2 * m]), int(row[off + 2 * m + 1])
        out |= (t >= st) & (t < st + w)
    return out


def feature_blank(row, F, K, n_t, n_f, S, si):
    out = np.zeros(F, bool)
    off = K + 2 + si * 2 * (n_t + n_f) + 2 * n_t
    f = np.arange(F)
    for m in range(n_f):
        st, w = int(row[off + 2 * m]), int(row[off + 2 * m + 1])
        out |= (f >= st) & (f < st + w)
    return out


def apply_ref(X, plan, K, n_t, n_f, S, si, fill=0.0):
    """mask(warp(X)) of stream si: float32 [B, T, F].  A frame with rem == 0 is a copy (its bits stay); row i0 + 1 is not touched."""
    X = np.ascontiguousarray(X, np.float32)
    B, T, F = X.shape
    Y = np.empty_like(X)
    for b in range(B):
        i0, rem, den = frames(plan[b], T, K)
        same = rem == 0
        Y[b, same] = X[b, i0[same]]
        mv = ~same
        if mv.any():
            x0, x1 = X[b, i0[mv]], X[b, i0[mv] + 1]
            frac = (rem[mv].astype(np.float32) / den[mv].astype(np.float32))[:, None]
            with np.errstate(invalid="ignore", over="ignore"):
                d = (x1 - x0).astype(np.float32)
                pr = (frac * d).astype(np.float32)
                Y[b, mv] = (x0 + pr).astype(np.float32)
        Y[b, time_blank(plan[b], T, K, n_t, n_f, S, si)] = np.float32(fill)
        Y[b][:, feature_blank(plan[b], F, K, n_t, n_f, S, si)] = np.float32(fill)
    return Y


def augment_ref(inputs, norm, seed):
    """The restated plan and augmented float32 inputs of a batch under normalized settings `norm` (the dict
    mgr_amd.augment.normalize_config returns - plain data, read here, nothing of the product is run)."""
    names = [s["name"] for s in norm["streams"]]
    B, T = np.asarray(inputs[names[0]]).shape[:2]
    table = [(s["F"], s["time_masks"], s["time_width"], s["feature_masks"], s["feature_width"]) for s in norm["streams"]]
    K, S = norm["segments"], len(names)
    plan = plan_ref(B, T, table, K, norm["max_shift"], norm["n_t"], norm["n_f"], norm["drop_thresh"], seed)
    out = {n: apply_ref(inputs[n], plan, K, norm["n_t"], norm["n_f"], S, si, norm["streams"][si]["fill"]) for si, n in enumerate(names)}
    return out, plan
