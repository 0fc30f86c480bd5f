#!/usr/bin/env python3
"""Device time of the two localisation calls (csrc/align.hip) beside the parent kernels they are measured against, same run:
  * mgr_ctc_align          against  mgr_ctc_loss_grad with dLogits = NULL (emissions + alpha / beta chains, no gradient)
  * mgr_greedy_segments    against  mgr_frame_argmax
at the fusion / skeletal shape (B = 64, T = 1900, C = 22, Lmax = 35) and the audio shape (C = 44, Lmax = 150), posteriors and labels
device-resident, HIP events around `iters` launches, median over `reps` windows, the calls interleaved window by window.
--pipeline: pipelined fusion inference (Engine.predict_stream, config F's network, B = 64, T = 1900) per batch with output="segments"
against output="argmax", alternating in one session.
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


def peaky(rng, B, T, Cn, Lmax):
    """Run-structured, blank-dominated posteriors like a trained CTC network's, and label sequences that follow them."""
    z = rng.standard_normal((B, T, Cn)).astype(np.float32) * 1.5
    z[:, :, Cn - 1] += 3.0
    lab = -np.ones((B, Lmax), np.int32)
    ll = np.zeros(B, np.int32)
    gap = max(4, (T - 60) // Lmax)
    for b in range(B):
        t, k = 20, 0
        while t < T - 20 and k < Lmax:
            c = int(rng.integers(0, Cn - 1))
            run = int(rng.integers(2, max(3, gap // 2)))
            z[b, t:t + run, c] += rng.uniform(3.0, 9.0)
            lab[b, k] = c
            k += 1
            t += run + int(rng.integers(1, gap))
        ll[b] = k
    P = np.exp(z - z.max(-1, keepdims=True))
    return (P / P.sum(-1, keepdims=True)).astype(np.float32), lab, ll


def kernels(dev, B, T, Cn, Lmax, iters, reps):
    rng = np.random.default_rng(Cn)
    skip = 2
    P, lab, ll = peaky(rng, B, T, Cn, Lmax)
    dP, dlab, dil, dll = dev.array(P), dev.array(lab), dev.array(np.full(B, T - skip, np.int32)), dev.array(ll)
    path, seg, conf, logp = dev.empty((B, T - skip), np.int32), dev.empty((B, Lmax, 2), np.int32), dev.empty((B, Lmax)), dev.empty((B,), np.float64)
    wsa = dev.bytes(dev.lib.mgr_ctc_align_ws_bytes(B, T, Cn, Lmax))
    loss, wsl = dev.empty((B,)), dev.bytes(dev.lib.mgr_ctc_ws_bytes(B, T, Cn, Lmax))
    cap = T - skip
    n, rl, rs, rc = dev.empty((B,), np.int32), dev.empty((B, cap), np.int32), dev.empty((B, cap, 2), np.int32), dev.empty((B, cap))
    best, prob = dev.empty((B, T - skip), np.int32), dev.empty((B, T - skip))
    eps = C.c_float(1e-8)
    calls = {
        "ctc_align": lambda: dev.call("mgr_ctc_align", dP, dlab, dil, dll, B, T, Cn, Lmax, skip, Cn - 1, eps, path, seg, conf, logp, wsa, wsa.nbytes),
        "ctc_loss_no_grad": lambda: dev.call("mgr_ctc_loss_grad", dP, dlab, dil, dll, B, T, Cn, Lmax, skip, Cn - 1, eps, C.c_float(1.0), loss, 0,
                                             wsl, wsl.nbytes),
        "greedy_segments": lambda: dev.call("mgr_greedy_segments", dP, B, T, Cn, skip, C.c_float(0.5), cap, n, rl, rs, rc),
        "frame_argmax": lambda: dev.call("mgr_frame_argmax", dP, B, T, Cn, skip, best, prob),
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
    lp, ls = logp.download(), loss.download()
    res = {"B": B, "T": T, "C": Cn, "Lmax": Lmax, "mean_label_len": round(float(ll.mean()), 1), "mean_runs": round(float(n.download().mean()), 1),
           "all_feasible": bool(np.all(np.isfinite(lp)) and np.all(np.isfinite(ls))),
           "ms_median": {k: round(float(np.median(v)), 4) for k, v in times.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()}}
    for a in (dP, dlab, dil, dll, path, seg, conf, logp, wsa, loss, wsl, n, rl, rs, rc, best, prob):
        a.free()
    return res


def pipeline(dev, batches, rounds):
    from mgr_amd.configs import fusion_spec
    from mgr_amd.engine import Engine
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    spec, B, T = fusion_spec(), 64, 1900
    eng = Engine(spec, B, T, 1, device=dev, seed=1, inference_only=True)
    eng.set_weights(synthetic_weights(spec, 7))
    chunks = [synthetic_arrays(spec, B, T, 1, 100 + i)[0] for i in range(3)]
    feed = lambda: (chunks[i % 3] for i in range(batches))
    out = {"segments": [], "argmax": []}
    for mode in out:
        list(eng.predict_stream(feed(), output=mode, threshold=0.5))        # warm-up (pinned buffers)
    for _ in range(rounds):
        for mode in out:
            t0 = time.perf_counter()
            list(eng.predict_stream(feed(), output=mode, threshold=0.5))
            out[mode].append((time.perf_counter() - t0) / batches * 1e3)
    eng.close()
    return {"B": B, "T": T, "batches_per_run": batches, "ms_per_batch_median": {k: round(float(np.median(v)), 3) for k, v in out.items()},
            "ms_per_batch_runs": {k: [round(x, 3) for x in v] for k, v in out.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--maxlen", type=int, default=1900)
    ap.add_argument("--iters", type=int, default=10, help="launches per timed window")
    ap.add_argument("--reps", type=int, default=7, help="timed windows")
    ap.add_argument("--lib", default=None, help="another build of libmgr.so (e.g. an ablation of align.hip) instead of the package's")
    ap.add_argument("--pipeline", action="store_true")
    ap.add_argument("--pipeline-batches", type=int, default=6)
    ap.add_argument("--pipeline-rounds", type=int, default=4)
    a = ap.parse_args()
    if a.lib:
        _capi.LIB_PATH = os.path.abspath(a.lib)
    dev = _capi.Device(0)
    res = {"metric": "align_kernels_ms", "device": dev.name,
           "fusion_shape": kernels(dev, a.batch, a.maxlen, 22, 35, a.iters, a.reps),
           "audio_shape": kernels(dev, a.batch, a.maxlen, 44, 150, a.iters, a.reps)}
    if a.pipeline:
        res["pipelined_inference"] = pipeline(dev, a.pipeline_batches, a.pipeline_rounds)
    dev.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
