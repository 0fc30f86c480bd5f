#!/usr/bin/env python3
"""Device time and parity of the train-time augmentation calls; writes profiles/augment_timing.txt and
profiles/augment_parity.txt (--out-dir: elsewhere).

  timing   mgr_augment_plan + one mgr_augment_apply per stream against the mgr_add_gaussian_noise calls they replace, on the same
           buffers, at B = 64, T = 1900, F = 39 + 20 (both streams noised at 0.5 for the comparison; the flagship noises the first
           only): same process, the two sets interleaved window by window.  HIP events around `iters` repetitions, median of 5 windows.
  step     a config-F training step with the mode on against off: one engine, one batch, the two modes alternating window by
           window (a window = `steps` pipelined steps between device syncs, host wall time).
  parity   the bit comparisons of tests/test_gpu_augment.py (differing elements per case) and the first-step errors against the
           fp64 oracle of tests/test_gpu_augment_step.py.
Each step runs in a child process of its own under a time limit; a step that fails or runs out of time is reported as such."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mgr_amd  # noqa: E402,F401  (before numpy: _hostenv.py)
import numpy as np  # noqa: E402

EV0, EV1 = 10, 11
WINDOWS = 5
B, T, FS = 64, 1900, (39, 20)
CFG = dict(segments=16, max_shift=40, time_masks=2, time_width=100, feature_masks=2, feature_width=8, stream_drop=0.2)


def _timed(dev, calls, iters):
    times = {k: [] for k in calls}
    for fn in calls.values():
        for _ in range(3):
            fn()
    dev.sync()
    for _ in range(WINDOWS):
        for k, fn in calls.items():
            dev.record(EV0)
            for _ in range(iters):
                fn()
            dev.record(EV1)
            dev.sync()
            times[k].append(dev.elapsed_ms(EV0, EV1) / iters)
    return {k: [round(float(np.median(v)), 4), round(float(np.min(v)), 4)] for k, v in times.items()}


def step_timing(a):
    from mgr_amd import _capi, augment
    dev = _capi.Device(0)
    rng = np.random.default_rng(1)
    norm = augment.normalize_config(CFG, [dict(name="s%d" % i, F=F) for i, F in enumerate(FS)], T)
    ident = augment.normalize_config({}, [dict(name="s%d" % i, F=F) for i, F in enumerate(FS)], T)
    X = [dev.array(rng.standard_normal((B, T, F)).astype(np.float32)) for F in FS]
    Y = [dev.empty((B, T, F)) for F in FS]
    plan, table = dev.empty((B, augment.plan_len(norm)), np.int32), augment.stream_table(norm)
    iplan, itable = dev.empty((B, augment.plan_len(ident)), np.int32), augment.stream_table(ident)
    seed = 20131900

    def noise():
        for x, y in zip(X, Y):
            dev.call("mgr_add_gaussian_noise", x, y, x.size, 0.5, C.c_uint64(seed))

    def fused(n, p, t):
        def run():
            augment.enqueue_plan(dev, n, t, B, T, seed, p)
            for si in range(len(FS)):
                augment.enqueue_apply(dev, n, si, X[si], Y[si], p, B, T, 0.5, seed)
        return run
    ms = _timed(dev, {"noise_x2": noise, "plan+apply_x2": fused(norm, plan, table), "plan+apply_x2_identity": fused(ident, iplan, itable),
                      "plan_only": lambda: augment.enqueue_plan(dev, norm, table, B, T, seed, plan)}, a.iters)
    dev.close()
    return {"device": dev.name, "ms": ms, "bytes": 2 * 4 * B * T * sum(FS), "cfg": CFG}


def step_step(a):
    """config F, the benchmark's engine and batch: `steps` pipelined steps a window, the mode off and on alternating"""
    from mgr_amd import _capi
    from mgr_amd.configs import baseline_config
    from mgr_amd.engine import Engine
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    dev = _capi.Device(0)
    spec, Bf, Tf, Lmax = baseline_config("F")
    eng = Engine(spec, Bf, Tf, Lmax, device=dev, seed=1000)
    eng.set_weights(synthetic_weights(spec, 20131900 + 3))
    xs, labels, il, ll = synthetic_arrays(spec, Bf, Tf, Lmax, 20131900 + 3)
    eng._upload_inputs(xs, None, True)
    eng._upload_labels(labels, il, ll)
    dev.sync()

    def window(n):
        dev.sync()
        t0 = time.perf_counter()
        for i in range(n):
            eng.enqueue_train_step(None, None, None, None, rand=None, apply_update=True, upload=False, prefetch_next=i + 1 < n,
                                   prefetch_after_next=i + 2 < n)
            loss = eng.read_loss(local=True)
        dev.sync()
        return (time.perf_counter() - t0) * 1e3 / n, loss
    times, last = {"off": [], "on": []}, {}
    for mode in ("off", "on"):
        eng.set_augment(CFG if mode == "on" else None)
        window(3)
    for _ in range(WINDOWS):
        for mode in ("off", "on"):
            eng.set_augment(CFG if mode == "on" else None)
            ms, last[mode] = window(a.steps)
            times[mode].append(ms)
    eng.close()
    dev.close()
    return {"config": "F", "B": Bf, "T": Tf, "Lmax": Lmax, "steps": a.steps, "cfg": CFG, "last": last,
            "ms_per_step": {k: [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for k, v in times.items()}}


def step_parity(a):
    import test_gpu_augment as tg
    import test_gpu_augment_step as ts
    from mgr_amd import _capi, augment
    from tests import rng_cases as rc
    dev = _capi.Device(0)
    rows = []
    for seed in (0, 5, (1 << 62) + 20131901):
        norm = augment.normalize_config(tg.PLAN_CFG, tg.streams(7, 4), 23)
        got, ref = tg.device_plan(dev, norm, 5, 23, seed), tg.ref_plan(norm, 5, 23, seed)
        rows.append(["plan B5 T23 seed %d" % seed, int(ref.size), int((got != ref).sum())])
    for name, (Bc, Tc, Fs, cfg) in tg.APPLY_CASES.items():
        norm = augment.normalize_config(cfg, tg.streams(*Fs), Tc)
        x = tg.case_inputs(name)
        got, plan = augment.augment_batch(x, cfg, 77, device=dev)          # (the public call: plan drawn and applied on the device)
        ref, rplan = tg.ar.augment_ref(x, norm, 77)
        rows.append(["plan of %s" % name, int(rplan.size), int((plan != rplan).sum())])
        for si, (k, F) in enumerate(zip(x, Fs)):
            moved = int(sum((tg.ar.frames(rplan[b], Tc, norm["segments"])[1] != 0).sum() for b in range(Bc))) * F
            rows.append(["augment_batch %s stream %d (%d interpolated)" % (name, si, moved), int(ref[k].size),
                         int((tg.bits(got[k]) != tg.bits(ref[k])).sum())])
    x = tg.batch(np.random.default_rng(11), 5, 23, 7)
    norm = augment.normalize_config(tg.PLAN_CFG, tg.streams(7, 4), 23)
    plan = tg.ref_plan(norm, 5, 23, 6)
    clean = tg.device_apply(dev, norm, x, plan)
    noisy = tg.device_apply(dev, norm, x, plan, stddev=0.5, seed=99)
    rows.append(["apply(0.5) against mgr_add_gaussian_noise(apply(0)), B5 T23 F7", int(x.size),
                 int((tg.bits(noisy) != tg.bits(tg.device_noise(dev, clean, 0.5, 99))).sum())])
    steps = []
    for name in ts.CFGS:
        c = rc.case(name)
        seed = ts.seed_with_a_dropped_and_an_undropped_sample(c, name) if name == "fusion_tiny" else rc.SEEDS[name]
        batch = (c["inputs"], c["labels"], c["il"], c["ll"])
        (loss, lb, g, P), _, _ = ts.oracle(c, name, batch, seed, 0)
        eng = ts.make_engine(dev, c, seed)
        eng.set_augment(ts.CFGS[name])
        got = ts.run_step(eng, batch)
        eng.close()
        steps.append([name, abs(got["loss"] - loss) / abs(loss), float((np.abs(got["loss_b"] - lb) / np.abs(lb)).max()),
                      float(ts.rel_err(got["P"], P)), float(max(ts.rel_err(got["g"][k], g[k]) for k in g))])
    dev.close()
    return {"rows": rows, "steps": steps}


STEPS = {"timing": (step_timing, 120), "step": (step_step, 300), "parity": (step_parity, 120)}


def write_reports(res, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    t, st, p = res.get("timing"), res.get("step"), res.get("parity")
    with open(os.path.join(out_dir, "augment_timing.txt"), "w") as f:
        f.write("mgr_augment_plan / mgr_augment_apply on one MI355X (python tools/augment_bench.py): device time in ms, HIP events around %d\n"
                "repetitions, median (min) of %d windows, the sets interleaved window by window in one process.  B=%d T=%d F=%s, both\n"
                "streams noised at 0.5.  No time target was set.\n\n" % (res["iters"], WINDOWS, B, T, "+".join(str(F) for F in FS)))
        if isinstance(t, dict) and "ms" in t:
            f.write("device: %s; settings %s\n" % (t["device"], t["cfg"]))
            for k, v in t["ms"].items():
                f.write("  %-26s %8.4f (%.4f)\n" % (k, v[0], v[1]))
            f.write("  bytes read + written by either set: %.1f MB; fused / noise, ratio of the medians: %.2f\n"
                    % (t["bytes"] / 1e6, t["ms"]["plan+apply_x2"][0] / t["ms"]["noise_x2"][0]))
        else:
            f.write("timing step: %s\n" % (t,))
        if isinstance(st, dict) and "ms_per_step" in st:
            off, on = st["ms_per_step"]["off"], st["ms_per_step"]["on"]
            f.write("\nconfig F training step (B=%d T=%d Lmax=%d; one engine, one batch, %d pipelined steps a window, host wall time per step in\n"
                    "ms, median (min .. max) of %d windows, the two modes alternating):\n"
                    "  mode off                     %8.3f (%.3f .. %.3f)\n"
                    "  set_augment(the settings)    %8.3f (%.3f .. %.3f)\n"
                    "  ratio of the medians %.3f; last losses off / on: %s / %s\n"
                    % (st["B"], st["T"], st["Lmax"], st["steps"], WINDOWS, *off, *on, on[0] / off[0], st["last"]["off"], st["last"]["on"]))
        else:
            f.write("\nstep: %s\n" % (st,))
    with open(os.path.join(out_dir, "augment_parity.txt"), "w") as f:
        f.write("mgr_augment_plan / mgr_augment_apply against the numpy restatement tests/augment_ref.py on one MI355X (python\n"
                "tools/augment_bench.py): elements compared and elements whose BITS differ (the tests assert 0), then the first device-RNG\n"
                "training step with the mode on against the fp64 oracle under the restated augmentation and the replayed randomness\n"
                "(bounds 1e-4 on loss / loss_b / P, 2e-4 on gradients).\n\n")
        if isinstance(p, dict) and "rows" in p:
            for what, n, bad in p["rows"]:
                f.write("%-70s %8d %6d\n" % (what, n, bad))
            f.write("\n%-14s %10s %10s %10s %14s\n" % ("step", "loss", "loss_b", "P", "worst gradient"))
            for name, *e in p["steps"]:
                f.write("%-14s %10.2e %10.2e %10.2e %14.2e\n" % (name, *e))
        else:
            f.write("parity step: %s\n" % (p,))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="repetitions per timed window")
    ap.add_argument("--steps", type=int, default=20, help="training steps per timed window")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process and print its JSON line")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(STEPS[a.step][0](a)))
        return
    res = {"iters": a.iters}
    for name, (_, limit) in STEPS.items():
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--iters", str(a.iters), "--steps", str(a.steps)],
                               stdout=subprocess.PIPE, timeout=limit)
            res[name] = json.loads(r.stdout.decode().strip().splitlines()[-1]) if r.returncode == 0 else "failed (exit status %d)" % r.returncode
        except subprocess.TimeoutExpired:
            res[name] = "ran out of its %d s" % limit
            break               # (nothing more is started on the device behind a step that hung)
        if not isinstance(res[name], dict):
            break
    write_reports(res, a.out_dir)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
