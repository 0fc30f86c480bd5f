#!/usr/bin/env python3
"""Device time of the lexicon-constrained decode (csrc/lexicon.hip) alone, beside the shipped decodes of the same posteriors, same run:
  * mgr_ctc_lexicon_decode over the reference's 21 gesture phrases (97 states), without tables and with a gesture bigram
  * mgr_ctc_align of the word sequence it returns (the same recursion over ONE word sequence), mgr_greedy_segments
at the audio shape (B = 64, T = 1900, C = 44), posteriors and tables device-resident, HIP events around `iters` launches, median over
`reps` windows, the calls interleaved window by window.  There is no parent implementation: the numbers are recorded, not compared
with a target.  --host: the restatement's host loop (tests/lexicon_ref.py, numpy, fp64) on `--host-samples` samples of the same input,
wall clock.  Posteriors are run-structured and blank-dominated like a trained CTC network's, following random gesture sequences.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mgr_amd  # noqa: E402,F401  (before numpy: _hostenv.py)
import numpy as np  # noqa: E402
from mgr_amd import _capi, decoding  # noqa: E402
from mgr_amd.audio_network.sequence_decoding import GESTURE_LEXICON  # noqa: E402

EV0, EV1 = 10, 11


def peaky_gestures(rng, B, T, Cn, n_gestures):
    """Blank-dominated posteriors with a short run per word of n_gestures random gestures per sample; returns (P, gesture lists)."""
    z = rng.standard_normal((B, T, Cn)).astype(np.float32)
    z[:, :, Cn - 1] += 9.0          # (well above the noise: a word the sequence does not hold is not worth a phrase)
    seqs = []
    for b in range(B):
        seq = [int(g) for g in rng.integers(0, len(GESTURE_LEXICON), n_gestures)]
        words = [w for g in seq for w in GESTURE_LEXICON[g]]
        gap = max(4, (T - 60) // max(1, len(words)))
        t = 20
        for w in words:
            run = int(rng.integers(2, max(3, gap // 2)))
            z[b, t:t + run, w] += rng.uniform(12.0, 18.0)
            t += run + int(rng.integers(1, gap))
        seqs.append(seq)
    P = np.exp(z - z.max(-1, keepdims=True))
    return (P / P.sum(-1, keepdims=True)).astype(np.float32), seqs


def kernels(dev, P, seqs, iters, reps):
    rng = np.random.default_rng(1)
    B, T, Cn = P.shape
    skip, cap = 2, T - 2
    off, words = decoding.compile_lexicon(GESTURE_LEXICON, Cn)
    G = len(off) - 1
    lm, lm_end = decoding.bigram_lm([[int(g) for g in rng.integers(0, G, 8)] for _ in range(200)], G + 1, blank=G)
    ext0, _ = decoding.phrase_lm_tables(G)
    ext1, fin1 = decoding.phrase_lm_tables(G, lm[:G + 1, :G], lm_end[:G + 1])
    dP, dil = dev.array(P), dev.array(np.full(B, T - skip, np.int32))
    dext0, dext1, dfin1 = dev.array(ext0), dev.array(ext1), dev.array(fin1)
    n, phr, seg, conf = dev.empty((B,), np.int32), dev.empty((B, cap), np.int32), dev.empty((B, cap, 2), np.int32), dev.empty((B, cap))
    score, logp = dev.empty((B,), np.float64), dev.empty((B,), np.float64)
    ws = dev.bytes(dev.lib.mgr_ctc_lexicon_ws_bytes(B, T, Cn, G, off.ctypes.data))
    eps = C.c_float(1e-8)

    def lexicon(dext, dfin):
        dev.call("mgr_ctc_lexicon_decode", dP, dil, B, T, Cn, skip, Cn - 1, eps, off.ctypes.data, words.ctypes.data, G, dext, dfin, cap, n, phr,
                 seg, conf, None, score, logp, ws, ws.nbytes)

    lexicon(dext0, None)
    got = decoding.lexicon_from_arrays(n.download(), phr.download(), seg.download(), conf.download())
    found = [[s[0] for s in sg] for sg in got]
    labels = [[w for g in q for w in GESTURE_LEXICON[g]] for q in found]
    lab, ll = decoding.pack_labels(labels)
    Lmax = lab.shape[1]
    dlab, dll = dev.array(lab), dev.array(ll)
    apath, aseg, aconf, alogp = dev.empty((B, T - skip), np.int32), dev.empty((B, Lmax, 2), np.int32), dev.empty((B, Lmax)), dev.empty((B,), np.float64)
    wsa = dev.bytes(dev.lib.mgr_ctc_align_ws_bytes(B, T, Cn, Lmax))
    gn, gl, gs, gc = dev.empty((B,), np.int32), dev.empty((B, cap), np.int32), dev.empty((B, cap, 2), np.int32), dev.empty((B, cap))
    calls = {
        "lexicon_no_tables": lambda: lexicon(dext0, None),
        "lexicon_bigram": lambda: lexicon(dext1, dfin1),
        "ctc_align_of_its_words": lambda: dev.call("mgr_ctc_align", dP, dlab, dil, dll, B, T, Cn, Lmax, skip, Cn - 1, eps, apath, aseg, aconf, alogp,
                                                   wsa, wsa.nbytes),
        "greedy_segments": lambda: dev.call("mgr_greedy_segments", dP, B, T, Cn, skip, C.c_float(0.5), cap, gn, gl, gs, gc),
    }
    times = {k: [] for k in calls}
    for fn in calls.values():
        for _ in range(3):
            fn()
    dev.sync()
    for _ in range(reps):
        for k, fn in calls.items():
            dev.record(EV0)
            for _ in range(iters):
                fn()
            dev.record(EV1)
            dev.sync()
            times[k].append(dev.elapsed_ms(EV0, EV1) / iters)
    res = {"B": B, "T": T, "C": Cn, "G": G, "states": 1 + 2 * len(words), "planted_recovered": sum(a == b for a, b in zip(found, seqs)),
           "mean_phrases": round(float(np.mean([len(q) for q in found])), 1), "align_Lmax": int(Lmax),
           "ms_median": {k: round(float(np.median(v)), 4) for k, v in times.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()}}
    for a in (dP, dil, dext0, dext1, dfin1, n, phr, seg, conf, score, logp, ws, dlab, dll, apath, aseg, aconf, alogp, wsa, gn, gl, gs, gc):
        a.free()
    return res, found


def host_loop(P, found, samples):
    """tests/lexicon_ref.py's token pass (numpy, fp64) on the first `samples` samples: seconds per sample, and whether it agrees."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import align_ref as ar
    import lexicon_ref as lr
    Cn = P.shape[2]
    gr = lr.Graph(GESTURE_LEXICON, Cn - 1)
    secs, same = [], 0
    for b in range(samples):
        t0 = time.perf_counter()
        logy = ar.log_emissions(P[b], 2, 1e-8)
        seq = lr.token_pass(logy, gr, Cn - 1)[1]
        secs.append(time.perf_counter() - t0)
        same += seq == found[b]
    return {"samples": samples, "s_per_sample_median": round(float(np.median(secs)), 4), "same_sequence": same,
            "ms_per_batch_of_64_extrapolated": round(float(np.median(secs)) * 64e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--maxlen", type=int, default=1900)
    ap.add_argument("--gestures", type=int, default=12, help="gestures per sample")
    ap.add_argument("--iters", type=int, default=10, help="launches per timed window")
    ap.add_argument("--reps", type=int, default=7, help="timed windows")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-samples", type=int, default=4)
    a = ap.parse_args()
    dev = _capi.Device(0)
    P, seqs = peaky_gestures(np.random.default_rng(44), a.batch, a.maxlen, 44, a.gestures)
    kern, found = kernels(dev, P, seqs, a.iters, a.reps)
    res = {"metric": "lexicon_decode_ms", "device": dev.name, "audio_shape": kern}
    if a.host:
        res["host_restatement"] = host_loop(P, found, min(a.host_samples, a.batch))
    dev.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
