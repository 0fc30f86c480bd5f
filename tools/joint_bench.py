#!/usr/bin/env python3
"""Device time of the joint decode over several CTC streams (csrc/joint.hip, mgr_ctc_joint_decode) against what the library had
before it for the same kind of answer.  Same process, the ways alternating window by window, HIP events around `iters` repetitions,
median (min) over `reps` windows, after warm-up calls.
  * two streams at B = 64, T = 1900: 22 gesture classes and 44 word classes through the reference's gesture lexicon, beam 10,
    top_paths 1 and 8.  Baseline: the rescoring route's device work - mgr_ctc_beam_search_lm (top_paths 8) on the gesture stream,
    mgr_ctc_lexicon_decode on the word stream, and two mgr_ctc_rescore calls over the 8-best (the host's pooling between them, and the
    one hypothesis the pool may gain from the lexicon decode, are left out: the baseline is a lower bound of that route).
  * one stream without a lexicon, beam 10, top_paths 8, against mgr_ctc_beam_search_lm on the same posteriors - planted-peaky and
    near-uniform posteriors, since the number of rounds depends on them.
Also recorded: workspace bytes, the mean number of rounds, and the parity gaps - each stream's logp against mgr_ctc_rescore on the
returned hypotheses, and how often the 1-best equals the frame-synchronous beam search's.
Prints one JSON line, writes the table to --out and the gaps to --parity."""
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
    """Blank-dominated posteriors (T, C) as a trained CTC network's: unit-variance logit noise, the blank 12 above it, and per label,
    in order, a run of two to five frames 5 to 9 above the blank.  A spurious label somewhere in 1900 frames, or a blank that splits
    a run, is then less probable than none, so the planted sequence is the most probable labelling."""
    z = rng.standard_normal((T, Cn)).astype(np.float32)
    z[:, Cn - 1] += 12.0
    gap = max(8, (T - 60) // max(1, len(labels)))
    t = 20
    for w in labels:
        run = int(rng.integers(2, 6))
        z[t:t + run, w] += rng.uniform(17.0, 21.0)
        t += run + int(rng.integers(2, gap - 6))
    P = np.exp(z - z.max(-1, keepdims=True))
    return (P / P.sum(-1, keepdims=True)).astype(np.float32)


def near_uniform(rng, B, T, Cn):
    z = 0.3 * rng.standard_normal((B, T, Cn)).astype(np.float32)
    P = np.exp(z)
    return (P / P.sum(-1, keepdims=True)).astype(np.float32)


class Joint:
    """One prepared mgr_ctc_joint_decode call."""

    def __init__(self, dev, streams, G, beam, top_paths, max_len):
        self.dev, self.M, self.G, self.W, self.NP, self.L = dev, len(streams), G, beam, top_paths, max_len
        self.B = streams[0]["P"].shape[0]
        self.keep = [s.get("phrase_off") for s in streams] + [s.get("phrase_words") for s in streams]
        self.arr = _capi.make_joint_streams(streams)
        self.ext = dev.array(np.zeros((G + 1, G)))
        B, NP, M = self.B, top_paths, self.M
        self.out, self.out_len = dev.empty((B, NP, max_len), np.int32), dev.empty((B, NP), np.int32)
        self.score, self.logp, self.rounds = dev.empty((B, NP), np.float64), dev.empty((B, NP, M), np.float64), dev.empty((B,), np.int32)
        self.ws_bytes = dev.lib.mgr_ctc_joint_ws_bytes(B, M, self.arr, G, beam, top_paths, max_len)
        self.ws = dev.bytes(self.ws_bytes)

    def __call__(self):
        self.dev.call("mgr_ctc_joint_decode", self.B, self.M, self.arr, self.G, self.ext, None, self.W, self.NP, self.L, self.out, self.out_len,
                      self.score, self.logp, self.rounds, self.ws, self.ws.nbytes)

    def free(self):
        for a in (self.ext, self.out, self.out_len, self.score, self.logp, self.rounds, self.ws):
            a.free()


def desc(dP, dil, T, Cn, lexicon=None):
    off, words = decoding.compile_lexicon(lexicon, Cn) if lexicon is not None else (None, None)
    return dict(T=T, C=Cn, skip=SKIP, blank=Cn - 1, eps=EPS, weight=1.0, P=dP, input_len=dil, phrase_off=off, phrase_words=words)


def beam_lm_call(dev, dP, dil, B, T, Cn, beam, top):
    ext = dev.array(np.zeros((Cn + 1, Cn)))
    out, out_len = dev.empty((B, top, T - SKIP), np.int32), dev.empty((B, top), np.int32)
    score, lctc = dev.empty((B, top), np.float64), dev.empty((B, top), np.float64)
    ws = dev.bytes(dev.lib.mgr_ctc_beam_lm_ws_bytes(B, T, Cn, beam, top))

    def call():
        dev.call("mgr_ctc_beam_search_lm", dP, dil, B, T, Cn, SKIP, Cn - 1, beam, C.c_float(EPS), ext, None, top, out, out_len, score, lctc, ws,
                 ws.nbytes)
    return call, (out, out_len, score, lctc)


def rescore_call(dev, dP, dil, B, T, Cn, lexicon, hyp, hyp_len):
    off, words = decoding.compile_lexicon(lexicon, Cn) if lexicon is not None else (None, None)
    G = 0 if off is None else len(off) - 1
    host = lambda a: None if a is None else a.ctypes.data
    logp = dev.empty(hyp_len.shape, np.float64)
    ws = dev.bytes(dev.lib.mgr_ctc_rescore_ws_bytes(B, T, Cn, G, host(off)))

    def call():
        dev.call("mgr_ctc_rescore", dP, dil, B, T, Cn, SKIP, Cn - 1, C.c_float(EPS), host(off), host(words), G, hyp, hyp_len, hyp.shape[1],
                 hyp.shape[2], logp, None, ws, ws.nbytes)
    return call, logp


def lexicon_call(dev, dP, dil, B, T, Cn, lexicon, cap=64):
    off, words = decoding.compile_lexicon(lexicon, Cn)
    G = len(off) - 1
    ext = dev.array(np.zeros((G + 1, G)))
    outs = [dev.empty((B,), np.int32), dev.empty((B, cap), np.int32), dev.empty((B, cap, 2), np.int32), dev.empty((B, cap), np.float32)]
    score, logp = dev.empty((B,), np.float64), dev.empty((B,), np.float64)
    ws = dev.bytes(dev.lib.mgr_ctc_lexicon_ws_bytes(B, T, Cn, G, off.ctypes.data))

    def call():
        dev.call("mgr_ctc_lexicon_decode", dP, dil, B, T, Cn, SKIP, Cn - 1, C.c_float(EPS), off.ctypes.data, words.ctypes.data, G, ext, None, cap,
                 outs[0], outs[1], outs[2], outs[3], None, score, logp, ws, ws.nbytes)
    return call


def timed(dev, calls, iters, reps, warm=2):
    for fn in calls.values():
        for _ in range(warm):
            fn()
    dev.sync()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            dev.record(EV0)
            for _ in range(iters):
                fn()
            dev.record(EV1)
            dev.sync()
            times[k].append(dev.elapsed_ms(EV0, EV1) / iters)
    return ({k: round(float(np.median(v)), 3) for k, v in times.items()}, {k: round(float(np.min(v)), 3) for k, v in times.items()})


def rel_gap(a, b):
    fin = np.isfinite(b) & np.isfinite(a)
    return float(np.max(np.abs(a[fin] - b[fin]) / np.abs(b[fin]))) if fin.any() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--maxlen", type=int, default=1900)
    ap.add_argument("--gestures", type=int, default=10, help="planted gestures per sample")
    ap.add_argument("--rounds", type=int, default=16, help="max_len of the joint decode")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_timing.txt"))
    ap.add_argument("--parity", default=os.path.join(ROOT, "profiles", "joint_parity.txt"))
    a = ap.parse_args()
    dev = _capi.Device(0)
    rng = np.random.default_rng(19)
    B, T, L = a.batch, a.maxlen, a.rounds
    G = len(GESTURE_LEXICON)
    truths = [[int(g) for g in rng.integers(0, G, a.gestures)] for _ in range(B)]
    dsk = dev.array(np.stack([peaky(rng, T, 22, t) for t in truths]))
    dau = dev.array(np.stack([peaky(rng, T, 44, [w for g in t for w in GESTURE_LEXICON[g]]) for t in truths]))
    dil = dev.array(np.full(B, T - SKIP, np.int32))
    rows, parity = [], []

    # ---- two streams
    j1 = Joint(dev, [desc(dsk, dil, T, 22), desc(dau, dil, T, 44, GESTURE_LEXICON)], G, 10, 1, L)
    j8 = Joint(dev, [desc(dsk, dil, T, 22), desc(dau, dil, T, 44, GESTURE_LEXICON)], G, 10, 8, L)
    beam8, (bout, blen, _, _) = beam_lm_call(dev, dsk, dil, B, T, 22, 10, 8)
    lexd = lexicon_call(dev, dau, dil, B, T, 44, GESTURE_LEXICON)
    beam8()
    rs_sk, lp_sk = rescore_call(dev, dsk, dil, B, T, 22, None, bout, blen)
    rs_au, lp_au = rescore_call(dev, dau, dil, B, T, 44, GESTURE_LEXICON, bout, blen)

    def route():
        beam8()
        lexd()
        rs_sk()
        rs_au()
    med, lo = timed(dev, {"joint_top1": j1, "joint_top8": j8, "rescoring_route": route, "beam_lm_top8_alone": beam8}, a.iters, a.reps)
    j8()
    dev.sync()
    out, out_len, logp, rounds8 = j8.out.download(), j8.out_len.download(), j8.logp.download(), j8.rounds.download()
    j1()
    dev.sync()
    rounds1 = j1.rounds.download()
    found = float(np.mean([list(out[b, 0, :out_len[b, 0]]) == truths[b] for b in range(B)]))
    hyp, hl = dev.array(out), dev.array(out_len)
    for name, dP, Cn, lex, m in (("gestures", dsk, 22, None, 0), ("words through the lexicon", dau, 44, GESTURE_LEXICON, 1)):
        call, lp = rescore_call(dev, dP, dil, B, T, Cn, lex, hyp, hl)
        call()
        dev.sync()
        parity.append("two streams, %-26s logp[.., %d] against mgr_ctc_rescore on the returned hypotheses: largest relative gap %.3e" %
                      (name + ":", m, rel_gap(logp[:, :, m], lp.download())))
    parity.append("two streams: the planted sequence is the 1-best on %.0f%% of the samples" % (100 * found))
    rows.append(dict(workload="two streams, 22 + 44 classes (lexicon)", B=B, T=T, beam=10, max_len=L, ws_bytes=int(j8.ws_bytes),
                     rounds_mean={"top1": float(rounds1.mean()), "top8": float(rounds8.mean())}, ms_median=med, ms_min=lo))
    j1.free()
    j8.free()

    # ---- one stream, no lexicon, against the frame-synchronous beam search
    for name, P in (("planted-peaky", None), ("near-uniform", near_uniform(rng, B, T, 22))):
        dP = dsk if P is None else dev.array(P)
        j = Joint(dev, [desc(dP, dil, T, 22)], 21, 10, 8, L)
        bl, (bo, bn, bs, _) = beam_lm_call(dev, dP, dil, B, T, 22, 10, 8)
        med, lo = timed(dev, {"joint_top8": j, "beam_lm_top8": bl}, a.iters, a.reps)
        j()
        bl()
        dev.sync()
        jo, jn, js, r = j.out.download(), j.out_len.download(), j.score.download(), j.rounds.download()
        bo, bn, bs = bo.download(), bn.download(), bs.download()
        same = float(np.mean([list(jo[b, 0, :max(jn[b, 0], 0)]) == list(bo[b, 0, :max(bn[b, 0], 0)]) for b in range(B)]))
        ahead = float(np.mean(js[:, 0] >= bs[:, 0]))
        parity.append("one stream, %-14s 1-best equal to mgr_ctc_beam_search_lm's on %.0f%% of the samples; the joint 1-best's score (the full "
                      "sum over alignments) is >= the beam search's (a pruned sum) on %.0f%%; max_len %d" % (name + ":", 100 * same, 100 * ahead, L))
        rows.append(dict(workload="one stream, 22 classes, %s" % name, B=B, T=T, beam=10, max_len=L, ws_bytes=int(j.ws_bytes),
                         rounds_mean={"top8": float(r.mean())}, ms_median=med, ms_min=lo))
        j.free()
    res = {"metric": "ctc_joint_decode_ms", "device": dev.name, "iters": a.iters, "reps": a.reps, "workloads": rows, "parity": parity}
    dev.close()
    lines = ["mgr_ctc_joint_decode on one MI355X (%s): device time per call in ms, HIP events around %d repetitions, median (min) of %d" %
             (res["device"], a.iters, a.reps), "windows after warm-up, the ways of a workload alternating window by window in one process.", ""]
    for w in rows:
        lines.append("%s: B = %d, T = %d, beam %d, max_len %d, workspace %d bytes, mean rounds %s" %
                     (w["workload"], w["B"], w["T"], w["beam"], w["max_len"], w["ws_bytes"], w["rounds_mean"]))
        for k in w["ms_median"]:
            lines.append("    %-22s %10.3f (%.3f)" % (k, w["ms_median"][k], w["ms_min"][k]))
    for path, text in ((a.out, lines), (a.parity, parity)):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(text) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
