#!/usr/bin/env python3
"""Device time of mgr_ctc_beam_search_lm beside mgr_ctc_beam_search - the two entry points of the one search body in csrc/beam.hip -
in one process on one GPU: N = 276 sequences of T = 1900 frames, beam 10, C = 22 (gesture networks) and C = 44 (audio network),
posteriors run-structured and blank-dominated like a trained CTC network's (tools/decode_bench.py), device-resident.  Each form is
timed with HIP events around ONE launch, `launches` times, the forms interleaved launch by launch after a warm-up of each; the median
(and the minimum) per form and the ratios of the medians to the plain entry point's are reported.
  beam           mgr_ctc_beam_search(merge_repeated=0)
  lm_zero        mgr_ctc_beam_search_lm, all-zero ext, fin = NULL, top_paths = 1      (the same search bit for bit)
  lm_dense       ... a dense random ext ~ N(0, 1) and fin
  lm_zero_top10  ... zero tables, top_paths = 10
  lm_dense_top10 ... dense tables, top_paths = 10
--parity: the largest relative score deviation from the fp64 reference (tests/beam_lm_ref.py) over the shapes of
tests/test_gpu_beam_lm.py, and from the exhaustive enumeration over its tiny shapes.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mgr_amd  # noqa: E402,F401  (before numpy: _hostenv.py)
import numpy as np  # noqa: E402
from mgr_amd import _capi  # noqa: E402

EV0, EV1 = 10, 11


def timing(dev, N, T, Cn, W, launches, warmup):
    from decode_bench import peaky_posteriors
    skip = 2
    P, _ = peaky_posteriors(N, T, Cn, 20131900 + Cn)
    rng = np.random.default_rng(Cn)
    dP, dil = dev.array(P), dev.array(np.full(N, T - skip, np.int32))
    zero, dense, fin = dev.array(np.zeros((Cn + 1, Cn))), dev.array(rng.standard_normal((Cn + 1, Cn))), dev.array(rng.standard_normal(Cn + 1))
    out1, len1, lp1 = dev.empty((N, T - skip), np.int32), dev.empty((N,), np.int32), dev.empty((N,), np.float64)
    outs = {NP: (dev.empty((N, NP, T - skip), np.int32), dev.empty((N, NP), np.int32), dev.empty((N, NP), np.float64),
                 dev.empty((N, NP), np.float64)) for NP in (1, W)}
    ws = dev.bytes(dev.lib.mgr_ctc_beam_lm_ws_bytes(N, T, Cn, W, W))
    eps = C.c_float(1e-8)
    lm = lambda ext, f, NP: lambda: dev.call("mgr_ctc_beam_search_lm", dP, dil, N, T, Cn, skip, Cn - 1, W, eps, ext, f, NP, *outs[NP], ws,
                                             ws.nbytes)
    calls = {
        "beam": lambda: dev.call("mgr_ctc_beam_search", dP, dil, N, T, Cn, skip, Cn - 1, W, eps, 0, out1, len1, lp1, ws, ws.nbytes),
        "lm_zero": lm(zero, None, 1),
        "lm_dense": lm(dense, fin, 1),
        "lm_zero_top%d" % W: lm(zero, None, W),
        "lm_dense_top%d" % W: lm(dense, fin, W),
    }
    times = {k: [] for k in calls}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    dev.sync()
    for _ in range(launches):
        for k, fn in calls.items():
            dev.record(EV0)
            fn()
            dev.record(EV1)
            dev.sync()
            times[k].append(dev.elapsed_ms(EV0, EV1))
    calls["beam"]()
    calls["lm_zero"]()
    same = bool(np.array_equal(out1.download(), outs[1][0].download()[:, 0]) and np.array_equal(lp1.download(), outs[1][2].download()[:, 0]))
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"N": N, "T": T, "C": Cn, "beam": W, "launches": launches, "mean_labels_per_sequence": round(float(len1.download().mean()), 1),
           "zero_tables_bit_equal_to_beam": same,
           "ms_median": {k: round(v, 3) for k, v in med.items()}, "ms_min": {k: round(float(np.min(v)), 3) for k, v in times.items()},
           "ratio_to_beam": {k: round(v / med["beam"], 3) for k, v in med.items() if k != "beam"}}
    for a in (dP, dil, zero, dense, fin, out1, len1, lp1, ws) + outs[1] + outs[W]:
        a.free()
    return res


def parity(dev):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import beam_lm_ref as br
    import test_gpu_beam_lm as tg
    worst = lambda got, want: max([abs(g - w) / abs(w) for g, w in zip(got, want) if w != 0] + [0.0])
    dev_ref, dev_enum, min_gap, n_hyp = 0.0, 0.0, float("inf"), 0
    for shape in tg.SHAPES + [tg.AUDIO]:
        N, T, Cn, W = shape
        P, il = tg.case(shape)
        for frac in (0.0, 0.2):
            ext, fin = tg.tables(Cn, 50 + Cn, frac)
            seqs, rs, rl, gap = br.beam_search_lm(P, il, ext, fin, beam_width=W, top_paths=W)
            out, olen, score, logp = tg.run_nbest(dev, P, il, ext, fin, W, W)
            min_gap = min(min_gap, gap)
            for b in range(N):
                n = len(seqs[b])
                assert [out[b, k, :olen[b, k]].tolist() for k in range(n)] == seqs[b]
                dev_ref = max(dev_ref, worst(score[b, :n], rs[b]), worst(logp[b, :n], rl[b]))
                n_hyp += n
    for Cn, Tp in tg.TINY:
        for with_inf in (False, True):
            for seed in range(4):
                P, ext, fin = tg.tiny_case(Cn, Tp, 100 * Cn + 10 * Tp + seed, with_inf)
                ranked, _ = br.enumerate_labellings(P, ext, fin)
                out, olen, score, logp = tg.run_nbest(dev, P[None], [Tp], ext, fin, 32, 8, skip=0, eps=0.0)
                n = min(8, len(ranked))
                assert [tuple(out[0, k, :olen[0, k]].tolist()) for k in range(n)] == [e[0] for e in ranked[:n]]
                dev_enum = max(dev_enum, worst(score[0, :n], [e[1] for e in ranked[:n]]), worst(logp[0, :n], [e[2] for e in ranked[:n]]))
    return {"hypotheses_compared_with_reference": n_hyp, "sequences_equal": True, "max_rel_score_deviation_from_reference": dev_ref,
            "smallest_cut_gap_of_reference": min_gap, "max_rel_score_deviation_from_enumeration": dev_enum}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=276)
    ap.add_argument("--maxlen", type=int, default=1900)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--launches", type=int, default=21, help="timed launches per form")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parity", action="store_true")
    a = ap.parse_args()
    dev = _capi.Device(0)
    res = {"metric": "beam_lm_ms", "device": dev.name}
    if a.parity:
        res["parity"] = parity(dev)
    res["gesture_shape"] = timing(dev, a.n, a.maxlen, 22, a.beam, a.launches, a.warmup)
    res["audio_shape"] = timing(dev, a.n, a.maxlen, 44, a.beam, a.launches, a.warmup)
    dev.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
