#!/usr/bin/env python3
"""Cost of live recognition on the MI355X; writes profiles/live_timing.txt (--out: elsewhere).

The fusion network at the reference's sizes (H = 500 / 300 encoders, H = 100 fusion layer), chunk = 20, lookahead = 20 (windows of
40 frames), at S = 1 and S = 16 sessions, every slot with a whole window each step:

  step     one LiveSession.step(): host wall time around the whole call (it ends in the download of the event counts, a device
           synchronise), and inside it the device time of the window's kernels (HIP events around the enqueue); host = the rest
           (buffering, three small uploads per stream, the downloads).  To read the events the bench synchronises once behind the
           enqueue, which a step of its own does not: the step and host figures include that extra synchronise (the predict
           figure below has none), so they are upper bounds.  Median of `--steps` steps behind `--warmup`.
           The real-time budget: a step answers chunk x 50 ms = 1 s of signal; the bench ASSERTS step < budget and prints the ratio.
  scan     mgr_lstm_scan_window alone, the two H = 500 jobs (forward with state, reverse) of the audio encoder's first layer
           over the same window: device time per call (events around `--iters` calls, median of 5), and the bytes of Up one
           workgroup streams (steps x 4 H^2 x 4 bytes) over that time.
  predict  the only route without this feature: Engine(B = S, T = 40, inference_only=True).predict on the same window - stateless,
           so wrong for live use, but the cost a user paid before.  Host wall time, the same median.  No target.
Nothing here measures accuracy: whether a lookahead costs recognition rate needs ChaLearn data, which is not at hand.
Each S runs in a child process of its own under a time limit; one that fails or runs out of time is reported as such and ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mgr_amd  # noqa: E402,F401  (before numpy: _hostenv.py)
import numpy as np  # noqa: E402

EV0, EV1 = 10, 11
CHUNK, LOOK = 20, 20
FRAME_S = 0.05


def bench_sessions(dev, spec, w, S, a):
    from mgr_amd.engine import Engine
    Tw = CHUNK + LOOK
    eng = Engine(spec, S, Tw, 4, device=dev, inference_only=True)
    eng.set_weights(w)
    live = eng.open_live(S, CHUNK, LOOK)
    rng = np.random.default_rng(S)
    frames = lambda n: {s["name"]: rng.standard_normal((n, s["F"])).astype(np.float32) for s in spec.streams}
    dev_ms = []
    enqueue = live._enqueue

    def timed(nv, nk):
        dev.record(EV0)
        enqueue(nv, nk)
        dev.record(EV1)
        dev.sync()
        dev_ms.append(dev.elapsed_ms(EV0, EV1))
    live._enqueue = timed
    for slot in range(S):
        live.push(slot, frames(LOOK))
    wall = []
    for it in range(a.warmup + a.steps):
        for slot in range(S):
            live.push(slot, frames(CHUNK))
        t0 = time.perf_counter()
        res = live.step()
        wall.append((time.perf_counter() - t0) * 1e3)
        assert all(r.n_keep == CHUNK for r in res)
    wall, dms = wall[a.warmup:], dev_ms[a.warmup:]
    step_ms, device_ms = statistics.median(wall), statistics.median(dms)
    live._enqueue = enqueue

    # the H = 500 window scan alone, on the session's own buffers
    from mgr_amd import _capi
    name = spec.streams[0]["name"]
    H = spec.streams[0]["layers"][0]["H"]
    jobs = []
    for di, d in enumerate(("fwd", "bwd")):
        L = eng.dirs["%s/l0/%s" % (name, d)]
        jobs.append(dict(Z=live.Z[name][di], Up=L.Up, Y=live.Y1[name].view(di * H, (1,)), ldy=2 * H, H=H, reverse=L.reverse,
                         state=0 if L.reverse else live.state["%s/l0" % name]))
    arr = _capi.make_live_jobs(jobs)
    call = lambda: dev.call("mgr_lstm_scan_window", 2, arr, S, Tw, live.n_valid, live.n_keep, 0, 0)
    for _ in range(3):
        call()
    dev.sync()
    scan = []
    for _ in range(5):
        dev.record(EV0)
        for _ in range(a.iters):
            call()
        dev.record(EV1)
        dev.sync()
        scan.append(dev.elapsed_ms(EV0, EV1) / a.iters)
    scan_ms = statistics.median(scan)
    up_bytes = Tw * 4 * H * H * 4
    live.close()

    # the stateless route: predict on the same window
    x = {k: np.stack([frames(Tw)[k] for _ in range(S)]) for k in frames(1)}
    pred = []
    for it in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        eng.predict(x)
        pred.append((time.perf_counter() - t0) * 1e3)
    predict_ms = statistics.median(pred[a.warmup:])
    eng.close()
    budget_ms = CHUNK * FRAME_S * 1e3
    lines = ["S = %2d  step %8.3f ms (device %7.3f, host %6.3f; min %.3f max %.3f)  budget %.0f ms: %.4f of it, %5.0fx real time"
             % (S, step_ms, device_ms, step_ms - device_ms, min(wall), max(wall), budget_ms, step_ms / budget_ms, budget_ms / step_ms),
             "        scan  H = %d, 2 jobs, %d steps: %7.3f ms per call (%.1f us per step), %d workgroups; Up per workgroup %.1f MB per call = %.1f GB/s"
             % (H, Tw, scan_ms, scan_ms * 1e3 / Tw, 2 * ((S + 3) // 4), up_bytes / 1e6, up_bytes / (scan_ms * 1e-3) / 1e9),
             "        predict (Engine(B = %d, T = %d, inference_only).predict, stateless): %8.3f ms" % (S, Tw, predict_ms)]
    return lines, step_ms < budget_ms


def child(a):
    from mgr_amd import _capi
    from mgr_amd.configs import fusion_spec
    from mgr_amd.synthetic import synthetic_weights
    dev = _capi.Device(0)
    spec = fusion_spec()
    lines, within = bench_sessions(dev, spec, synthetic_weights(spec, 20131900), a.part, a)
    print("RESULT " + json.dumps(dict(lines=lines, within=within, name=dev.name, cus=dev.cu_count)))
    dev.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds per child process")
    ap.add_argument("--part", type=int, default=0, help="(internal) run the measurements of this many sessions in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_timing.txt"))
    a = ap.parse_args()
    if a.part:
        return child(a)
    out, ok, head = [], True, None
    for S in (1, 16):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", str(S), "--steps", str(a.steps), "--warmup", str(a.warmup), "--iters", str(a.iters)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.limit)
            res = [ln for ln in r.stdout.decode(errors="replace").splitlines() if ln.startswith("RESULT ")]
        except subprocess.TimeoutExpired:
            r, res = None, []
        if r is None or r.returncode != 0 or not res:
            out.append("S = %2d  FAILED (%s)" % (S, "time limit of %d s" % a.limit if r is None else "exit status %d" % r.returncode))
            if r is not None:
                sys.stderr.write(r.stdout.decode(errors="replace")[-2000:])
            ok = False
            break       # (nothing more is started on the device behind a child that failed or hung)
        d = json.loads(res[-1][len("RESULT "):])
        head = head or ["live recognition, fusion network at the reference's sizes, chunk = %d, lookahead = %d (tools/live_bench.py) on %s, %d CUs"
                        % (CHUNK, LOOK, d["name"], d["cus"]),
                        "medians of %d steps behind %d warm-up steps; scan: median of 5 windows of %d calls; step and host include one extra "
                        "synchronise behind the enqueue" % (a.steps, a.warmup, a.iters)]
        out += d["lines"]
        ok = ok and d["within"]
    out = (head or []) + out + ["accuracy against lookahead: not measured (no ChaLearn data at hand)"]
    text = "\n".join(out) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)
    assert ok, "a live step failed, or takes longer than the signal it answers"


if __name__ == "__main__":
    main()
