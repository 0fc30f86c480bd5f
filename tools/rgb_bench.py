#!/usr/bin/env python3
"""RGB network (rgb_network/cnn_lstm.py) timing: whole train steps at B = 2 and B = 8, T = 1900, and the CNN front-end's forward and
backward (dW / db of every layer, dX of conv_3 / conv_5) alone, in HIP events, with their fraction of the 157.3 TFLOP/s f32-MFMA
ceiling.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgr_amd  # noqa: E402,F401
from mgr_amd import configs  # noqa: E402
from mgr_amd.engine import Engine  # noqa: E402
from mgr_amd.keras_like import Model  # noqa: E402
from mgr_amd.spec import frontend_layers  # noqa: E402

F32_MFMA_TFLOPS = 157.3
EV0, EV1 = 10, 11


def cnn_flop(spec, backward):
    """USEFUL FLOP per frame of the front-end: forward over the four conv outputs of every pooled window; backward (dW, and dX of
    every layer but the first) over the one routed position per window only - the pre-activation gradient is zero at the other three.
    (The MFMA weight gradient multiplies those zeros too: it executes 4x its useful dW work; the vector kernels skip them.)"""
    tot = 0
    for i, c in enumerate(frontend_layers(spec.streams[0]["frontend"])):
        mac = c["Hp"] * c["Wp"] * c["ks"] * c["ks"] * c["Cin"] * c["Cout"]
        tot += mac * ((2 if i > 0 else 1) if backward else 4)
    return 2 * tot


def run(B, T, steps, warmup, seed=0):
    spec = configs.rgb_spec()
    eng = Engine(spec, B, T, 35, device=0)
    eng.set_weights(Model(spec, device=eng.dev).get_weights_dict())
    rng = np.random.RandomState(seed)
    x = ((rng.randint(0, 256, (B, T, 60, 60, 1)) - 128.) / 255.).astype(np.float32)
    labels = rng.randint(0, 21, (B, 35)).astype(np.int32)
    il = np.full(B, T - 2, np.int32)
    ll = np.full(B, 20, np.int32)
    for _ in range(warmup):
        eng.train_step({"the_input": x}, labels, il, ll)
    eng.dev.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = eng.train_step({"the_input": x}, labels, il, ll)
    eng.dev.sync()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    # the front-end alone, on the step's own buffers (the last step left its activations and its LSTM dX in place)
    dev = eng.dev
    dev.stream(0)
    reps = 3
    dev.record(EV0)
    for _ in range(reps):
        eng._frontend_fwd("the_input", eng.Xin["the_input"])
    dev.record(EV1)
    fwd_ms = dev.elapsed_ms(EV0, EV1) / reps
    dev.record(EV0)
    for _ in range(reps):
        eng._frontend_bwd("the_input")
    dev.record(EV1)
    bwd_ms = dev.elapsed_ms(EV0, EV1) / reps
    eng.close()
    N = B * T
    frac = lambda flop, t: flop * N / (t * 1e-3) / (F32_MFMA_TFLOPS * 1e12)
    return {"B": B, "T": T, "ms_per_step": round(ms, 3), "frames_per_s": round(N / (ms * 1e-3), 1), "loss": float(loss),
            "cnn_fwd_ms": round(fwd_ms, 3), "cnn_bwd_ms": round(bwd_ms, 3),
            "cnn_fwd_useful_frac_f32_mfma": round(frac(cnn_flop(spec, False), fwd_ms), 4),
            "cnn_bwd_useful_frac_f32_mfma": round(frac(cnn_flop(spec, True), bwd_ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="2,8")
    ap.add_argument("--T", type=int, default=1900)
    a = ap.parse_args()
    res = [run(int(b), a.T, a.steps, a.warmup) for b in a.batches.split(",")]
    print(json.dumps({"metric": "rgb_train_step", "ceiling_tflops": F32_MFMA_TFLOPS, "results": res}))


if __name__ == "__main__":
    main()
