#!/usr/bin/env python3
"""HTK MFCC_0_D_A front-end (csrc/mfcc.hip) throughput: a batch of 64 utterances of 95 s at 16 kHz (9,500 frames each) written as
the padded (64, 1900, 39) batch with audio_stride 5 (the shape of config F), timed in HIP events around the launches only; and the
same per-utterance work done by the fp64 numpy reference tests/htk_ref.py on the CPU (a few utterances, extrapolated as a rate).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mgr_amd  # noqa: E402,F401
from mgr_amd import _capi  # noqa: E402
from mgr_amd.audio_network import feature_extraction as fe  # noqa: E402

EV0, EV1 = 10, 11
FLOP_PER_FRAME = 25e3   # rough: 512-point real FFT ~ 12 kFLOP, window / magnitude / filterbank / DCT / deltas the rest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1520240)
    ap.add_argument("--stride", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-utts", type=int, default=2, help="utterances run through the CPU reference (0: skip)")
    a = ap.parse_args()
    rate = 16000
    cfg = fe.parse_hcopy_config(fe.REFERENCE_CONFIG)
    frame_size, frame_rate, fft_n = fe.frame_params(rate, cfg)
    rng = np.random.RandomState(0)
    waves = [np.clip(rng.standard_normal(a.samples) * 3000, -32768, 32767).astype(np.int16) for _ in range(a.utts)]
    nfr = (a.samples - frame_size) // frame_rate + 1
    T = -(-nfr // a.stride)
    n_frames = nfr * a.utts
    lo_chan, lo_wt = fe.filterbank_table(rate, fft_n, cfg["NUMCHANS"])
    dev = _capi.Device(0)
    s_offs = np.arange(a.utts + 1, dtype=np.int64) * a.samples
    o_offs = np.arange(a.utts + 1, dtype=np.int64) * T
    ws_bytes = dev.lib.mgr_mfcc_ws_bytes(a.utts, n_frames, frame_size, fft_n, cfg["NUMCHANS"], cfg["NUMCEPS"])
    d_s, d_so, d_oo = dev.array(np.concatenate(waves)), dev.array(s_offs), dev.array(o_offs)
    d_lc, d_lw = dev.array(lo_chan), dev.array(lo_wt)
    d_out, d_ws = dev.empty((a.utts * T, 39)), dev.bytes(ws_bytes)
    args = (d_s, d_so, a.utts, n_frames, frame_size, frame_rate, fft_n, cfg["NUMCHANS"], cfg["NUMCEPS"], cfg["CEPLIFTER"],
            float(cfg["PREEMCOEF"]), 1, 1, a.stride, d_lc, d_lw, d_out, d_oo, d_ws, ws_bytes)
    for _ in range(a.warmup):
        dev.call("mgr_mfcc", *args)
    dev.sync()
    times = []
    for _ in range(a.iters):
        dev.record(EV0)
        dev.call("mgr_mfcc", *args)
        dev.record(EV1)
        dev.sync()
        times.append(dev.elapsed_ms(EV0, EV1))
    out = d_out.download()
    assert np.isfinite(out).all()
    ms = float(np.median(times))
    res = {"metric": "mfcc_frames_per_s", "utts": a.utts, "frames": int(n_frames), "T": int(T), "fftN": fft_n,
           "gpu_ms_median": round(ms, 3), "gpu_ms_min": round(float(np.min(times)), 3), "gpu_ms_max": round(float(np.max(times)), 3),
           "gpu_frames_per_s": round(n_frames / (ms * 1e-3)), "gpu_gflop_s_rough": round(n_frames * FLOP_PER_FRAME / (ms * 1e-3) / 1e9, 1),
           "device": dev.name}
    if a.ref_utts > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import htk_ref
        t0 = time.perf_counter()
        for w in waves[:a.ref_utts]:
            htk_ref.mfcc_0_d_a(w, rate)
        dt = time.perf_counter() - t0
        res["cpu_ref_frames_per_s"] = round(a.ref_utts * nfr / dt)
        res["cpu_ref_utts"] = a.ref_utts
    dev.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
