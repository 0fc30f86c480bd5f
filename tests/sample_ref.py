"""A numpy restatement of mgr_ctc_sample_paths (include/mgr.h, K16): the draw in float32, one operation at a time in the stated order
(the class loop below is the kernel's; numpy only runs it for all frames of a draw at once), the uniforms from update_ref.rand_u32,
the collapse and the merge in plain Python.  The GPU tests ask for `==` with it."""
import numpy as np

import update_ref as ur

F32 = np.float32
INV24 = F32(1.0) / F32(16777216.0)


def clip_len(n, To):
    return max(0, min(int(n), To))


def draw_frames(P_b, seed, row, T, skip, Tp, blank, eps):
    """The classes drawn at frames skip .. skip + Tp - 1 of one (sample, draw): row = b * K + k.  P_b (T, C) float32."""
    C = P_b.shape[1]
    if Tp == 0:
        return np.zeros(0, np.int32)
    w = P_b[skip:skip + Tp].astype(F32) + F32(eps)                    # w_c = P + eps
    assert w.dtype == F32
    cum = np.empty_like(w)
    run = np.zeros(Tp, F32)
    for c in range(C):                                               # cum_c = cum_{c-1} + w_c, class order
        run = run + w[:, c]
        cum[:, c] = run
    S = cum[:, C - 1]
    idx = np.uint64(row) * np.uint64(T) + np.arange(skip, skip + Tp, dtype=np.uint64)
    u = (ur.rand_u32(seed, idx) >> np.uint32(8)).astype(F32) * INV24
    thr = u * S
    assert thr.dtype == F32 and cum.dtype == F32
    hit = cum > thr[:, None]
    return np.where(hit.any(axis=1), hit.argmax(axis=1), blank).astype(np.int32)    # the first c with cum_c > thr, else blank


def collapse(path, blank):
    """CTC collapse of a frame path: drop a frame equal to its predecessor, then drop blanks."""
    path = np.asarray(path).reshape(-1)
    if path.size == 0:
        return []
    keep = np.r_[True, path[1:] != path[:-1]] & (path != blank)
    return [int(v) for v in path[keep]]


def merge(labellings):
    """Draws in order -> (unique labellings in order of first occurrence, their counts)."""
    uniq, counts = [], []
    for lab in labellings:
        if lab in uniq:
            counts[uniq.index(lab)] += 1
        else:
            uniq.append(lab)
            counts.append(1)
    return uniq, counts


def sample_paths(P, input_len, skip, blank, eps, seed, K):
    """-> (out (B, K, T - skip), out_len (B, K), count (B, K), n_unique (B,), path (B, K, T - skip)), all int32, as the kernel writes them."""
    P = np.asarray(P, F32)
    B, T, _ = P.shape
    To = T - skip
    out, path = -np.ones((B, K, To), np.int32), -np.ones((B, K, To), np.int32)
    out_len, count, n_unique = -np.ones((B, K), np.int32), np.zeros((B, K), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        Tp = To if input_len is None else clip_len(input_len[b], To)
        labs = []
        for k in range(K):
            fr = draw_frames(P[b], seed, b * K + k, T, skip, Tp, blank, eps)
            path[b, k, :Tp] = fr
            labs.append(collapse(fr, blank))
        uniq, cnt = merge(labs)
        n_unique[b] = len(uniq)
        for j, (lab, n) in enumerate(zip(uniq, cnt)):
            out[b, j, :len(lab)] = lab
            out_len[b, j], count[b, j] = len(lab), n
    return out, out_len, count, n_unique, path


def lists(out, out_len, count):
    """The arrays -> (per sample its unique labellings as lists, per sample their counts): what decoding.sample_hypotheses returns."""
    B, K = out_len.shape
    paths = [[[int(v) for v in out[b, j, :out_len[b, j]]] for j in range(K) if out_len[b, j] >= 0] for b in range(B)]
    counts = [[int(count[b, j]) for j in range(K) if out_len[b, j] >= 0] for b in range(B)]
    return paths, counts
