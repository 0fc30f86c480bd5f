#!/usr/bin/env python3
"""Device time of mgr_edit_distance (csrc/edit.hip) in one process on one GPU.  Each form is timed with HIP events around
ONE launch, `launches` times, the forms interleaved launch by launch after a warm-up of each; the median and the minimum per form
are reported.  Inputs are device-resident; hypotheses are the references with a fifth of the labels edited (a decode's errors, not
two random strings).
  gesture          276 pairs, m, n <= 40, 21 labels, rows of 40                     (one ChaLearn test set against its labels)
  gesture_ops      ... with the alignment (ops)
  gesture_wide     the same pairs in hyp rows of 1898 labels                         (what the pipelined pass feeds: T - skip wide rows)
  audio            276 pairs, m = n = 150, 43 labels
  audio_ops        ... with the alignment
  mbr              276 x 32 x 32 pairs over 276 x 32 hypotheses, m, n <= 40          (the minimum-Bayes-risk workload)
and beside them the host's decoding.label_error_rate on the gesture pairs (time.perf_counter, the Python double loop).
--parity: random pairs (lengths 0 .. 300, alphabets 2 / 5 / 44, four cost sets, ops on) against tests/edit_ref.py: the number of
pairs compared and the number whose dist, counts, lens, n_ops or ops differ.
--pipeline: Engine.predict_stream(output="score") against output="loss" per batch of 64 at the fusion shape (T = 1900), runs of
`--batches` batches alternating in one process, the median per-batch time of each, the spread of the "loss" runs, and the device
times of the decode kernel and of mgr_edit_distance alone on a batch's posteriors.
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
from mgr_amd import _capi  # noqa: E402

EV0, EV1 = 10, 11


def noisy_copy(rng, ref, n_labels, rate=0.2):
    out = []
    for v in ref:
        u = rng.random()
        if u < rate / 3:
            continue                                    # deleted
        out.append(int(rng.integers(0, n_labels)) if u < 2 * rate / 3 else int(v))
        if u > 1 - rate / 3:
            out.append(int(rng.integers(0, n_labels)))  # inserted
    return out


def rows(seqs, width):
    a = -np.ones((len(seqs), width), np.int32)
    for i, s in enumerate(seqs):
        a[i, :min(len(s), width)] = s[:width]
    return a


class Form:
    """One call of mgr_edit_distance with everything on the device."""

    def __init__(self, dev, hyp, ref, pairs=None, costs=(10, 7, 7), want_ops=False):
        self.dev = dev
        self.hyp, self.ref = dev.array(hyp), dev.array(ref)
        self.nh, self.Lh, self.nr, self.Lr = hyp.shape[0], hyp.shape[1], ref.shape[0], ref.shape[1]
        self.P = hyp.shape[0] if pairs is None else len(pairs)
        self.ph = self.pr = None
        if pairs is not None:
            self.ph, self.pr = dev.array(np.ascontiguousarray(pairs[:, 0], np.int32)), dev.array(np.ascontiguousarray(pairs[:, 1], np.int32))
        self.out = (dev.empty((self.P,), np.int32), dev.empty((self.P, 4), np.int32), dev.empty((self.P, 2), np.int32))
        self.ops = self.nops = self.ws = None
        if want_ops:
            self.ops, self.nops = dev.empty((self.P, self.Lh + self.Lr), np.int8), dev.empty((self.P,), np.int32)
            self.ws = dev.bytes(dev.lib.mgr_edit_distance_ws_bytes(self.P, self.Lh, self.Lr, 1))
        self.costs = costs

    def __call__(self):
        self.dev.call("mgr_edit_distance", self.hyp, None, self.nh, self.Lh, self.ref, None, self.nr, self.Lr, self.ph, self.pr, self.P,
                      self.costs[0], self.costs[1], self.costs[2], 0, *self.out, self.ops, self.nops, self.ws,
                      self.ws.nbytes if self.ws is not None else 0)


def interleaved(dev, calls, launches, warmup):
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
    return ({k: round(float(np.median(v)), 4) for k, v in times.items()}, {k: round(float(np.min(v)), 4) for k, v in times.items()})


def timing(dev, launches, warmup, n=276, nbest=32):
    from mgr_amd import decoding
    rng = np.random.default_rng(2013)
    g_ref = [[int(v) for v in rng.integers(0, 21, int(rng.integers(8, 37)))] for _ in range(n)]
    g_hyp = [noisy_copy(rng, r, 21)[:40] for r in g_ref]
    a_ref = [[int(v) for v in rng.integers(0, 43, 150)] for _ in range(n)]
    a_hyp = [(noisy_copy(rng, r, 43) + r)[:150] for r in a_ref]
    lists = [noisy_copy(rng, g_ref[b], 21)[:40] for b in range(n) for _ in range(nbest)]
    pairs = np.array([(b * nbest + k, b * nbest + j) for b in range(n) for k in range(nbest) for j in range(nbest)], np.int64)
    calls = {
        "gesture": Form(dev, rows(g_hyp, 40), rows(g_ref, 40)),
        "gesture_ops": Form(dev, rows(g_hyp, 40), rows(g_ref, 40), want_ops=True),
        "gesture_wide": Form(dev, rows(g_hyp, 1898), rows(g_ref, 40)),
        "audio": Form(dev, rows(a_hyp, 150), rows(a_ref, 150)),
        "audio_ops": Form(dev, rows(a_hyp, 150), rows(a_ref, 150), want_ops=True),
        "mbr": Form(dev, rows(lists, 40), rows(lists, 40), pairs=pairs),
    }
    med, mn = interleaved(dev, calls, launches, warmup)
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        ler = decoding.label_error_rate(g_hyp, g_ref)
        host.append((time.perf_counter() - t0) * 1e3)
    unit = Form(dev, rows(g_hyp, 40), rows(g_ref, 40), costs=(1, 1, 1))
    unit()
    same = int(unit.out[0].download().astype(np.int64).sum()) == round(ler * sum(len(r) for r in g_ref))
    return {"pairs": {k: f.P for k, f in calls.items()}, "launches": launches, "ms_median": med, "ms_min": mn,
            "host_label_error_rate_ms_median": round(float(np.median(host)), 3), "host_ler_equals_device_unit_cost_sum": bool(same),
            "us_per_pair_median": {k: round(1e3 * med[k] / calls[k].P, 4) for k in calls}}


def parity(dev):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import edit_ref as er
    rng = np.random.default_rng(99)
    n_pairs = bad = 0
    for A in (2, 5, 44):
        for costs in er.COST_SETS + [(5, 2, 9)]:
            lens = [0, 1, 2, 15, 16, 17, 40, 63, 64, 65, 127, 128, 129, 150, 257, 300]
            hyps = [[int(v) for v in rng.integers(0, A, int(rng.choice(lens)))] for _ in range(64)]
            refs = [noisy_copy(rng, h, A) if k % 2 else [int(v) for v in rng.integers(0, A, int(rng.choice(lens)))] for k, h in enumerate(hyps)]
            hyp, ref = rows(hyps, 300), rows(refs, 400)
            f = Form(dev, hyp, ref, costs=costs, want_ops=True)
            f()
            got = [o.download() for o in f.out] + [f.nops.download(), f.ops.download()]
            want = er.kernel_ref(hyp, None, ref, None, None, None, costs)
            ok = np.ones(64, bool)
            for g, w in zip(got, want):
                ok &= (g.reshape(64, -1) == np.asarray(w).reshape(64, -1)).all(axis=1)
            n_pairs += 64
            bad += int((~ok).sum())
    return {"pairs_compared_with_reference": n_pairs, "mismatches": bad}


def pipeline(dev, n_batches, reps, beam_width):
    from mgr_amd.configs import baseline_config
    from mgr_amd.engine import Engine
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    spec, B, T, Lmax = baseline_config("F")
    Cn, skip = spec.num_classes, int(spec.ctc["skip"])
    data = [synthetic_arrays(spec, B, T, Lmax, 40 + i) for i in range(2)]
    feed = lambda: (data[i & 1] for i in range(n_batches))
    eng = Engine(spec, B, T, Lmax, device=dev, seed=5)
    eng.set_weights(synthetic_weights(spec, 11))
    forms = {"loss": dict(output="loss"), "score_greedy": dict(output="score", decode="greedy"),
             "score_beam": dict(output="score", decode="beam", beam_width=beam_width)}
    per = {k: [] for k in forms}
    for k, kw in forms.items():                         # warm-up of every form
        list(eng.predict_stream(feed(), **kw))
    for _ in range(reps):
        for k, kw in forms.items():
            dev.sync()
            t0 = time.perf_counter()
            list(eng.predict_stream(feed(), **kw))
            per[k].append((time.perf_counter() - t0) * 1e3 / n_batches)
    # the added kernels alone, on the posteriors of the last batch
    P = eng.P
    cap = T - skip
    seg = (dev.empty((B,), np.int32), dev.empty((B, cap), np.int32), dev.empty((B, cap, 2), np.int32), dev.empty((B, cap), np.float32))
    dil = dev.array(np.full(B, cap, np.int32))
    bout, blen, blogp = dev.empty((B, cap), np.int32), dev.empty((B,), np.int32), dev.empty((B,), np.float64)
    wsb = dev.bytes(dev.lib.mgr_ctc_beam_ws_bytes(B, T, Cn, beam_width))
    sc = (dev.empty((B,), np.int32), dev.empty((B, 4), np.int32), dev.empty((B, 2), np.int32))
    lab = dev.array(np.where(data[1][1] >= 0, data[1][1], -1).astype(np.int32))
    edit = lambda hyp, hl: lambda: dev.call("mgr_edit_distance", hyp, hl, B, cap, lab, None, B, Lmax, None, None, B, 1, 1, 1, 1 << (Cn - 1),
                                            *sc, None, None, None, 0)
    calls = {
        "greedy_segments": lambda: dev.call("mgr_greedy_segments", P, B, T, Cn, skip, C.c_float(-1.0), cap, *seg),
        "beam_search": lambda: dev.call("mgr_ctc_beam_search", P, dil, B, T, Cn, skip, Cn - 1, beam_width, C.c_float(1e-8), 1, bout, blen,
                                        blogp, wsb, wsb.nbytes),
    }
    dev.stream(0)
    calls["greedy_segments"]()
    calls["beam_search"]()
    calls["edit_after_greedy"] = edit(seg[1], seg[0])
    calls["edit_after_beam"] = edit(bout, blen)
    med, mn = interleaved(dev, calls, 11, 2)
    hyp_labels = {"greedy": float(seg[0].download().mean()), "beam": float(blen.download().mean())}
    eng.close()
    m = {k: float(np.median(v)) for k, v in per.items()}
    spread = float(np.max(per["loss"]) - np.min(per["loss"]))
    res = {"B": B, "T": T, "Lmax": Lmax, "batches_per_run": n_batches, "runs_per_form": reps,
           "ms_per_batch_median": {k: round(v, 3) for k, v in m.items()},
           "ms_per_batch_all": {k: [round(x, 3) for x in v] for k, v in per.items()},
           "loss_run_to_run_spread_ms": round(spread, 3), "standalone_ms_median": med, "standalone_ms_min": mn,
           "mean_hyp_labels_per_sample": hyp_labels}
    for k, dec in (("score_greedy", "greedy_segments"), ("score_beam", "beam_search")):
        bound = m["loss"] + med[dec] + med["edit_after_" + k.split("_")[1]] + spread
        res[k + "_bound_ms"] = round(bound, 3)
        res[k + "_within_bound"] = bool(m[k] <= bound)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=21, help="timed launches per form")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--pipeline", action="store_true")
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--batches", type=int, default=6, help="--pipeline: batches per run")
    ap.add_argument("--reps", type=int, default=5, help="--pipeline: runs per form")
    ap.add_argument("--beam", type=int, default=10)
    a = ap.parse_args()
    dev = _capi.Device(0)
    res = {"metric": "edit_distance_ms", "device": dev.name}
    if a.parity:
        res["parity"] = parity(dev)
    if not a.no_timing:
        res["timing"] = timing(dev, a.launches, a.warmup)
    if a.pipeline:
        res["pipeline"] = pipeline(dev, a.batches, a.reps, a.beam)
    dev.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
