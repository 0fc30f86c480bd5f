#!/usr/bin/env python3
"""Device time of CTC hypothesis scoring (csrc/rescore.hip) against the only way to get the same numbers without it: K calls of
mgr_ctc_loss_grad (loss only, no gradient) on the same posteriors, one hypothesis column each.  Same process, the two alternating
window by window, HIP events around `iters` repetitions, median (min) over `reps` windows.  Two workloads at B = 64, T = 1900, K = 32:
  * gestures: C = 22, hypotheses of at most 40 labels
  * words through the lexicon: C = 44, hypotheses of phrase ids over the reference's 21 gesture phrases (the baseline gets their
    host-expanded word rows, uploaded outside the timed windows)
Posteriors are run-structured and blank-dominated like a trained CTC network's and follow the sample's first hypothesis; the others
are edits of it.  The two ways are also compared: the largest relative gap between logp and minus the (float32) loss is reported.
Prints one JSON line and writes the table to --out."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mgr_amd  # noqa: E402,F401  (before numpy: _hostenv.py)
import numpy as np  # noqa: E402
from mgr_amd import _capi, decoding  # noqa: E402
from mgr_amd.audio_network.sequence_decoding import GESTURE_LEXICON  # noqa: E402

EV0, EV1 = 10, 11
SKIP, EPS = 2, 1e-8


def peaky(rng, T, Cn, labels):
    """Blank-dominated posteriors (T, C) with a short run per label, in order."""
    z = rng.standard_normal((T, Cn)).astype(np.float32)
    z[:, Cn - 1] += 9.0
    gap = max(4, (T - 60) // max(1, len(labels)))
    t = 20
    for w in labels:
        run = int(rng.integers(2, max(3, gap // 2)))
        z[t:t + run, w] += rng.uniform(12.0, 18.0)
        t += run + int(rng.integers(1, gap))
    P = np.exp(z - z.max(-1, keepdims=True))
    return (P / P.sum(-1, keepdims=True)).astype(np.float32)


def edits(rng, truth, n_ids, K, max_len):
    """The truth and K - 1 hypotheses one to three random edits away from it, none longer than max_len."""
    out = [list(truth)]
    while len(out) < K:
        h = list(truth)
        for _ in range(int(rng.integers(1, 4))):
            kind, i = int(rng.integers(0, 3)), int(rng.integers(0, max(1, len(h))))
            if kind == 0 and h:
                h[i] = int(rng.integers(0, n_ids))
            elif kind == 1 and len(h) > 1:
                del h[i]
            elif len(h) < max_len:
                h.insert(i, int(rng.integers(0, n_ids)))
        out.append(h)
    return out


def workload(dev, name, P, paths, lexicon, iters, reps):
    B, T, Cn = P.shape
    K = len(paths[0])
    hyp, hyp_len = decoding.pack_nbest(paths, K=K, width=T - SKIP)            # (rows as wide as the beam decoder writes them)
    off, words = decoding.compile_lexicon(lexicon, Cn) if lexicon is not None else (None, None)
    G = 0 if off is None else len(off) - 1
    host = lambda a: None if a is None else a.ctypes.data
    labels = paths if lexicon is None else [[[w for g in h for w in lexicon[g]] for h in hyps] for hyps in paths]
    lab, lab_len = decoding.pack_nbest(labels, K=K)                            # the baseline's label rows: [B, K, Lmax]
    Lmax = lab.shape[2]
    dP, dil = dev.array(P), dev.array(np.full(B, T - SKIP, np.int32))
    dhyp, dhl = dev.array(hyp), dev.array(hyp_len)
    dlogp, dn = dev.empty((B, K), np.float64), dev.empty((B, K), np.int32)
    ws = dev.bytes(dev.lib.mgr_ctc_rescore_ws_bytes(B, T, Cn, G, host(off)))
    cols = [(dev.array(np.ascontiguousarray(lab[:, k])), dev.array(np.ascontiguousarray(lab_len[:, k]))) for k in range(K)]
    dloss = [dev.empty((B,), np.float32) for _ in range(K)]
    wsl = dev.bytes(dev.lib.mgr_ctc_ws_bytes(B, T, Cn, Lmax))
    eps = C.c_float(EPS)

    def new():
        dev.call("mgr_ctc_rescore", dP, dil, B, T, Cn, SKIP, Cn - 1, eps, host(off), host(words), G, dhyp, dhl, K, T - SKIP, dlogp, dn, ws,
                 ws.nbytes)

    def old():
        for k in range(K):
            dev.call("mgr_ctc_loss_grad", dP, cols[k][0], dil, cols[k][1], B, T, Cn, Lmax, SKIP, Cn - 1, eps, C.c_float(1.0), dloss[k], None,
                     wsl, wsl.nbytes)

    calls = {"rescore": new, "k_loss_calls": old}
    for fn in calls.values():
        for _ in range(3):
            fn()
    dev.sync()
    logp = dlogp.download()
    loss = np.stack([d.download().astype(np.float64) for d in dloss], axis=1)
    fin = np.isfinite(loss)
    assert np.array_equal(np.isfinite(logp), fin), "the two ways disagree on which hypotheses fit"
    gap = float(np.max(np.abs(logp[fin] + loss[fin]) / np.abs(loss[fin]))) if fin.any() else 0.0
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            dev.record(EV0)
            for _ in range(iters):
                fn()
            dev.record(EV1)
            dev.sync()
            times[k].append(dev.elapsed_ms(EV0, EV1) / iters)
    res = {"workload": name, "B": B, "T": T, "C": Cn, "K": K, "lexicon_phrases": G, "labels_max": int(lab_len.max()),
           "labels_mean": round(float(lab_len.mean()), 1), "baseline_Lmax": int(Lmax), "finite": int(fin.sum()),
           "max_rel_gap_logp_vs_minus_loss": gap,
           "ms_median": {k: round(float(np.median(v)), 4) for k, v in times.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()}}
    for a in [dP, dil, dhyp, dhl, dlogp, dn, ws, wsl] + dloss + [x for c in cols for x in c]:
        a.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--maxlen", type=int, default=1900)
    ap.add_argument("--hyps", type=int, default=32, help="hypotheses per sample (K)")
    ap.add_argument("--iters", type=int, default=10, help="repetitions per timed window")
    ap.add_argument("--reps", type=int, default=7, help="timed windows per way")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescore_timing.txt"))
    a = ap.parse_args()
    dev = _capi.Device(0)
    rng = np.random.default_rng(14)
    B, T, K = a.batch, a.maxlen, a.hyps
    G = len(GESTURE_LEXICON)
    truths = [[int(g) for g in rng.integers(0, 21, int(rng.integers(8, 37)))] for _ in range(B)]
    w1 = workload(dev, "gestures", np.stack([peaky(rng, T, 22, t) for t in truths]), [edits(rng, t, 21, K, 40) for t in truths], None,
                  a.iters, a.reps)
    truths = [[int(g) for g in rng.integers(0, G, 12)] for _ in range(B)]
    Pw = np.stack([peaky(rng, T, 44, [w for g in t for w in GESTURE_LEXICON[g]]) for t in truths])
    w2 = workload(dev, "words through the lexicon", Pw, [edits(rng, t, G, K, 16) for t in truths], GESTURE_LEXICON, a.iters, a.reps)
    res = {"metric": "ctc_rescore_ms", "device": dev.name, "iters": a.iters, "reps": a.reps, "workloads": [w1, w2]}
    dev.close()
    lines = ["mgr_ctc_rescore against K calls of mgr_ctc_loss_grad (loss only) on the same posteriors, one MI355X (%s): device time per" % res["device"],
             "B x K scores in ms, HIP events around %d repetitions, median (min) of %d windows, the two ways alternating window by window." % (a.iters, a.reps),
             "", "%-28s %4s %5s %3s %3s %11s  %-20s %-20s %7s  %s" % ("workload", "B", "T", "C", "K", "labels max", "rescore", "K loss calls", "ratio",
                                                                       "gap logp vs -loss")]
    for w in res["workloads"]:
        m, lo = w["ms_median"], w["ms_min"]
        lines.append("%-28s %4d %5d %3d %3d %11d  %-20s %-20s %6.1fx  %.3e" % (
            w["workload"], w["B"], w["T"], w["C"], w["K"], w["labels_max"], "%.4f (%.4f)" % (m["rescore"], lo["rescore"]),
            "%.4f (%.4f)" % (m["k_loss_calls"], lo["k_loss_calls"]), m["k_loss_calls"] / m["rescore"], w["max_rel_gap_logp_vs_minus_loss"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
