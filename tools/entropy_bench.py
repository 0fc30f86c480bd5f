#!/usr/bin/env python3
"""Device time and parity of the entropy-regularised CTC call; writes profiles/entropy_timing.txt and
profiles/entropy_parity.txt (--out-dir: elsewhere).

  timing   mgr_ctc_entropy_grad (with its gradient, scales 1 / B and 0.2 / B, and without) beside mgr_ctc_loss_grad (with and without
           its gradient kernel) - the loss's kernels are the parent's, untouched by the template flag - same process, calls interleaved
           window by window, at B = 64, T = 1900, C = 22, Lmax = 20 and 145.  HIP events around `iters` launches, the median of 5
           windows.
  step     a config-F training step with the entropy mode on against the same step with the mode off: one engine, one batch, the
           two modes alternating window by window (a window = `steps` pipelined steps between device syncs, host wall time).
  parity   the maxima behind the bounds of tests/test_gpu_entropy.py over tests/ctc_cases.ALL_NAMES: |H - H_ref| / max(1, |m_ref|) per
           sample and the pure-entropy gradient's error over the restatement's largest entry, against tests/entropy_ref.py in fp64.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mgr_amd  # noqa: E402,F401  (before numpy: _hostenv.py)
import numpy as np  # noqa: E402

EV0, EV1 = 10, 11
SKIP, EPS, WEIGHT = 2, 1e-8, 0.2
SHAPES = [(64, 1900, 22, 20), (64, 1900, 22, 145)]
WINDOWS = 5


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
    from align_bench import peaky
    from mgr_amd import _capi
    dev = _capi.Device(0)
    res = {"device": dev.name, "shapes": []}
    for shape in SHAPES:
        B, T, Cn, Lmax = shape
        P, lab, ll = peaky(np.random.default_rng(Lmax), B, T, Cn, Lmax)
        ins = [dev.array(P), dev.array(lab), dev.array(np.full(B, T - SKIP, np.int32)), dev.array(ll)]
        loss, H, dlog = dev.empty((B,)), dev.empty((B,)), dev.empty((B, T, Cn))
        ws = dev.bytes(2 * dev.lib.mgr_ctc_ws_bytes(B, T, Cn, Lmax))
        tail = (B, T, Cn, Lmax, SKIP, Cn - 1, C.c_float(EPS))
        sc = (C.c_float(1.0 / B), C.c_float(WEIGHT / B))
        calls = {
            "entropy_grad": lambda: dev.call("mgr_ctc_entropy_grad", *ins, *tail, *sc, loss, H, dlog, ws, ws.nbytes),
            "entropy_no_grad": lambda: dev.call("mgr_ctc_entropy_grad", *ins, *tail, *sc, loss, H, 0, ws, ws.nbytes),
            "ctc_loss_grad": lambda: dev.call("mgr_ctc_loss_grad", *ins, *tail, sc[0], loss, dlog, ws, ws.nbytes),
            "ctc_loss_no_grad": lambda: dev.call("mgr_ctc_loss_grad", *ins, *tail, sc[0], loss, 0, ws, ws.nbytes),
        }
        ms = _timed(dev, calls, a.iters)
        calls["entropy_no_grad"]()
        Hh, lo = H.download(), loss.download()
        res["shapes"].append({"shape": shape, "mean_label_len": round(float(ll.mean()), 1), "ms": ms, "mean_H": round(float(Hh.mean()), 3),
                              "all_feasible": bool(np.all(np.isfinite(lo)))})
        for x in ins + [loss, H, dlog, ws]:
            x.free()
    dev.close()
    return res


def step_step(a):
    """config F, the benchmark's engine and batch: `steps` pipelined steps a window, the mode off and on alternating"""
    from mgr_amd import _capi
    from mgr_amd.configs import baseline_config
    from mgr_amd.engine import Engine
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    dev = _capi.Device(0)
    spec, B, T, Lmax = baseline_config("F")
    eng = Engine(spec, B, T, Lmax, device=dev, seed=1000)
    eng.set_weights(synthetic_weights(spec, 20131900 + 3))
    xs, labels, il, ll = synthetic_arrays(spec, B, T, Lmax, 20131900 + 3)
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
        eng.set_entropy(dict(weight=WEIGHT) if mode == "on" else None)
        window(3)
    for _ in range(WINDOWS):
        for mode in ("off", "on"):
            eng.set_entropy(dict(weight=WEIGHT) if mode == "on" else None)
            ms, loss = window(a.steps)
            times[mode].append(ms)
            last[mode] = [loss, eng.last_ctc_loss, eng.last_entropy]
    eng.close()
    dev.close()
    return {"config": "F", "B": B, "T": T, "Lmax": Lmax, "steps": a.steps, "weight": WEIGHT,
            "ms_per_step": {k: [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for k, v in times.items()},
            "last": last}


def step_parity(a):
    import test_gpu_entropy as tg
    from mgr_amd import _capi
    from tests import ctc_cases as cc
    dev = _capi.Device(0)
    rows = []
    for name in cc.ALL_NAMES:
        c = cc.case(name)
        with_grad = name != "f-logzero"
        H_ref, m_ref, dH_ref, logp_ref = tg._reference(name)
        loss, H, dz = tg._entropy(dev, c, 0.0, 1.0, need_grad=with_grad)
        top = float(np.abs(dH_ref).max())
        rows.append({"case": name, "samples": len(H), "H": float((np.abs(H - H_ref) / np.maximum(1.0, np.abs(m_ref))).max()),
                     "max_m": float(np.abs(m_ref).max()), "max_H": float(H_ref.max()), "top": top,
                     "grad": float(np.abs(dz.astype(np.float64) + dH_ref).max() / top) if with_grad else None})
    dev.close()
    return {"rows": rows}


STEPS = {"timing": (step_timing, 240), "step": (step_step, 300), "parity": (step_parity, 300)}


def write_reports(res, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    t, st, p = res.get("timing"), res.get("step"), res.get("parity")
    with open(os.path.join(out_dir, "entropy_timing.txt"), "w") as f:
        f.write("mgr_ctc_entropy_grad on one MI355X (python tools/entropy_bench.py): device time per call in ms, HIP events around %d launches,\n"
                "median (min) of %d windows, the calls of a shape interleaved window by window in one process.  Posteriors are run-structured and\n"
                "blank-dominated (tools/align_bench.py: peaky); every sample carries up to Lmax labels.  mgr_ctc_loss_grad's kernels are the\n"
                "parent's (the template flag off).  No time target was set.  The box's run-to-run spread is about 2 %%.\n\n" % (res["iters"], WINDOWS))
        if isinstance(t, dict) and "shapes" in t:
            f.write("device: %s\n" % t["device"])
            for s_ in t["shapes"]:
                ms = s_["ms"]
                f.write("\nB=%d T=%d C=%d Lmax=%d (mean label length %.1f, all feasible: %s, mean H %.3f nats)\n"
                        % (*s_["shape"], s_["mean_label_len"], s_["all_feasible"], s_["mean_H"]))
                for k, v in ms.items():
                    f.write("  %-20s %8.4f (%.4f)\n" % (k, v[0], v[1]))
                f.write("  ratios of the medians: entropy+grad / loss+grad %.2f, entropy without grad / loss without grad %.2f\n"
                        % (ms["entropy_grad"][0] / ms["ctc_loss_grad"][0], ms["entropy_no_grad"][0] / ms["ctc_loss_no_grad"][0]))
        else:
            f.write("timing step: %s\n" % (t,))
        if isinstance(st, dict) and "ms_per_step" in st:
            off, on = st["ms_per_step"]["off"], st["ms_per_step"]["on"]
            f.write("\nconfig F training step (B=%d T=%d Lmax=%d; one engine, one batch, %d pipelined steps a window, host wall time per step in\n"
                    "ms, median (min .. max) of %d windows, the two modes alternating):\n"
                    "  mode off (mgr_head_fwd_bwd)            %8.3f (%.3f .. %.3f)\n"
                    "  set_entropy(weight=%.1f)               %8.3f (%.3f .. %.3f)\n"
                    "  ratio of the medians %.3f; last step's loss / ctc_loss / entropy with the mode on: %s\n"
                    % (st["B"], st["T"], st["Lmax"], st["steps"], WINDOWS, *off, st["weight"], *on, on[0] / off[0], st["last"]["on"]))
        else:
            f.write("\nstep: %s\n" % (st,))
    with open(os.path.join(out_dir, "entropy_parity.txt"), "w") as f:
        f.write("mgr_ctc_entropy_grad against the fp64 restatement of tests/entropy_ref.py on one MI355X (python tools/entropy_bench.py), over\n"
                "the cases of tests/ctc_cases.py: the largest deviation over all samples of a case.  H: |H - H_ref| / max(1, |m_ref|), m = E[ln\n"
                "p(path)], bound 1e-4; grad: loss_scale 0, ent_scale 1, max |dLogits + dH_ref/dlogits| over the largest |entry| of the\n"
                "restatement (top) of the case, bound 1e-4 (f-logzero: no gradient, as for the loss).\n\n")
        if isinstance(p, dict) and "rows" in p:
            f.write("%-20s %7s %10s %10s %9s %10s %10s\n" % ("case", "samples", "H", "max |m|", "max H", "top", "grad"))
            for r in p["rows"]:
                f.write("%-20s %7d %10.2e %10.1f %9.3f %10.2e %10s\n" % (r["case"], r["samples"], r["H"], r["max_m"], r["max_H"], r["top"],
                                                                        "-" if r["grad"] is None else "%.2e" % r["grad"]))
        else:
            f.write("parity step: %s\n" % (p,))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="launches per timed window")
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
