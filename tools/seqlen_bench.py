#!/usr/bin/env python3
"""Cost and parity of per-sample sequence lengths; writes profiles/seqlen_timing.txt and profiles/seqlen_parity.txt
(--out-dir: elsewhere).  Config F, B = 64, T = 1900, lengths uniform in [1000, 1900] under a fixed seed.

  fills    the mgr_seq_zero_tail calls of ONE training step, recorded from the engine and replayed on its buffers: device time
           (HIP events around `iters` repetitions, median of 5 windows), the bytes they zero, and the rate against mgr_memset
           (hipMemsetAsync) of the same number of bytes in the same windows.  No target was set.
  step     a pipelined training step with the lengths on (input_length = len - 2) against off (the batch without the key,
           input_length = T - 2: the calls an engine made before lengths existed), alternating window by window in one process
           (a window = `steps` pipelined steps between device syncs, host wall time).
  parity   the worst deviations of tests/test_gpu_seqlen_step.py's steps from the truncated fp64 oracle, with and without the
           lengths, and the kernel families tests/test_gpu_seqlen_scan.py ran.
Each step runs in a child process of its own under a time limit; a step that fails or runs out of time is reported as such."""
import argparse
import contextlib
import io
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
LEN_LO, LEN_SEED = 1000, 20131900


def _engine_f():
    from mgr_amd import _capi
    from mgr_amd.configs import baseline_config
    from mgr_amd.engine import Engine
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    dev = _capi.Device(0)
    spec, B, T, Lmax = baseline_config("F")
    eng = Engine(spec, B, T, Lmax, device=dev, seed=1000)
    eng.set_weights(synthetic_weights(spec, 20131900 + 3))
    xs, labels, il, ll = synthetic_arrays(spec, B, T, Lmax, 20131900 + 3)
    lens = np.random.default_rng(LEN_SEED).integers(LEN_LO, T + 1, size=B).astype(np.int32)
    return dev, eng, (xs, labels, il, ll), lens


def step_fills(a):
    from mgr_amd import _capi
    dev, eng, (xs, labels, il, ll), lens = _engine_f()
    B, T = eng.B, eng.T
    recorded = []
    zero = eng._zero_tails

    def recording(ln, bufs):
        if ln is not None and bufs:
            recorded.append([(b if isinstance(b, int) else b.ptr, row, ld) for b, row, ld in bufs])
        return zero(ln, bufs)
    eng._zero_tails = recording
    eng.train_step(dict(xs, seq_length=lens), labels, np.maximum(0, lens - 2), ll, apply_update=False)
    eng._zero_tails = zero
    dev.sync()
    d_len = dev.array(lens)
    calls = [(len(bufs), _capi.make_seq_fill_jobs([(p, row, ld, B, T) for p, row, ld in bufs])) for bufs in recorded]
    tail_frames = int((T - lens).sum())
    nbytes = sum(tail_frames * row * 4 for bufs in recorded for _, row, _ in bufs)
    scratch = dev.bytes(nbytes)

    def fills():
        for n, arr in calls:
            dev.call("mgr_seq_zero_tail", n, arr, d_len)

    def memset():
        dev.call("mgr_memset", scratch, 0, nbytes)
    times = {"fills": [], "memset": []}
    for fn in (fills, memset):
        for _ in range(3):
            fn()
    dev.sync()
    for _ in range(WINDOWS):
        for k, fn in (("fills", fills), ("memset", memset)):
            dev.record(EV0)
            for _ in range(a.iters):
                fn()
            dev.record(EV1)
            dev.sync()
            times[k].append(dev.elapsed_ms(EV0, EV1) / a.iters)
    name = dev.name
    eng.close()
    dev.close()
    return {"device": name, "B": B, "T": T, "calls": [[(row, ld) for _, row, ld in bufs] for bufs in recorded], "bytes": nbytes,
            "tail_frames": tail_frames, "lens": [int(lens.min()), int(lens.max()), float(lens.mean())],
            "ms": {k: [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)] for k, v in times.items()}}


def step_step(a):
    dev, eng, (xs, labels, il, ll), lens = _engine_f()
    modes = {"off": (xs, il), "on": (dict(xs, seq_length=lens), np.maximum(0, lens - 2))}

    def window(mode, n):
        x, ilen = modes[mode]
        eng._upload_inputs(x, None, True)       # resident inputs: the lengths stay with the input set they were uploaded with
        eng._upload_labels(labels, ilen, ll)
        dev.sync()
        t0 = time.perf_counter()
        for i in range(n):
            eng.enqueue_train_step(None, None, None, None, rand=None, apply_update=True, upload=False, prefetch_next=i + 1 < n,
                                   prefetch_after_next=i + 2 < n)
            loss = eng.read_loss(local=True)
        dev.sync()
        return (time.perf_counter() - t0) * 1e3 / n, loss
    times, last = {"off": [], "on": []}, {}
    for mode in modes:
        window(mode, 3)
    for _ in range(WINDOWS):
        for mode in modes:
            ms, last[mode] = window(mode, a.steps)
            times[mode].append(ms)
    out = {"config": "F", "B": eng.B, "T": eng.T, "Lmax": eng.Lmax, "steps": a.steps, "last": last,
           "ms_per_step": {k: [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for k, v in times.items()}}
    eng.close()
    dev.close()
    return out


def step_parity(a):
    import test_gpu_seqlen_scan as tscan
    import test_gpu_seqlen_step as ts
    from mgr_amd import _capi
    from tests import rng_cases as rc
    from tests import seqlen_ref as sr
    dev = _capi.Device(0)
    rows = []
    for name in sr.NAMES:
        c, lens = rc.case(name), sr.LENS[name]
        ref = sr.truncated_step(name)
        for label, inputs in (("with lengths", ts.with_len(c["inputs"], lens)), ("without", c["inputs"])):
            eng = ts.make_engine(dev, c)
            f = ts.figures(ts.run_step(eng, c, inputs, lens), ref, lens)
            eng.close()
            rows.append([name, label, f["loss"], f["loss_b"], f["P"], min(f["g"].values()), max(f["g"].values())])
    families = io.StringIO()
    with contextlib.redirect_stdout(families):
        for H in (32, 100, 300):
            tscan.test_reverse_scan_holds_zero_state_through_the_tail_in_every_family(dev, H)
            tscan.test_bptt_over_zeroed_gate_tails_gives_zero_dz_there_in_every_form(dev, H)
    dev.close()
    return {"rows": rows, "families": families.getvalue().strip().splitlines()}


STEPS = {"fills": (step_fills, 240), "step": (step_step, 300), "parity": (step_parity, 240)}


def write_reports(res, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    fl, st, p = res.get("fills"), res.get("step"), res.get("parity")
    with open(os.path.join(out_dir, "seqlen_timing.txt"), "w") as f:
        f.write("Per-sample sequence lengths on one MI355X (python tools/seqlen_bench.py): config F, lengths uniform in [%d, T] under seed %d.\n"
                "No time target was set.\n\n" % (LEN_LO, LEN_SEED))
        if isinstance(fl, dict) and "ms" in fl:
            f.write("device: %s; B=%d T=%d; lengths min / max / mean %d / %d / %.1f: %d tail frames\n" % (fl["device"], fl["B"], fl["T"], *fl["lens"],
                                                                                                       fl["tail_frames"]))
            f.write("the mgr_seq_zero_tail calls of one training step, (row, ld) per job: %s\n" % (fl["calls"],))
            f.write("device time in ms, HIP events around %d repetitions, median (min .. max) of %d windows, the two interleaved:\n"
                    % (res["iters"], WINDOWS))
            for k, label in (("fills", "the step's %d fill calls" % len(fl["calls"])), ("memset", "mgr_memset of the same bytes, one call")):
                ms = fl["ms"][k]
                f.write("  %-40s %8.4f (%.4f .. %.4f)   %7.1f GB/s\n" % (label, *ms, fl["bytes"] / ms[0] / 1e6))
            f.write("  bytes zeroed: %.1f MB; fill rate / memset rate: %.2f\n" % (fl["bytes"] / 1e6, fl["ms"]["memset"][0] / fl["ms"]["fills"][0]))
        else:
            f.write("fills: %s\n" % (fl,))
        if isinstance(st, dict) and "ms_per_step" in st:
            off, on = st["ms_per_step"]["off"], st["ms_per_step"]["on"]
            f.write("\nconfig F training step (B=%d T=%d Lmax=%d; one engine, resident inputs, %d pipelined steps a window, host wall time per\n"
                    "step in ms, median (min .. max) of %d windows, the two modes alternating):\n"
                    "  without lengths, input_length = T - 2     %8.3f (%.3f .. %.3f)\n"
                    "  with lengths, input_length = len - 2      %8.3f (%.3f .. %.3f)\n"
                    "  ratio of the medians %.3f; last losses off / on: %s / %s\n"
                    % (st["B"], st["T"], st["Lmax"], st["steps"], WINDOWS, *off, *on, on[0] / off[0], st["last"]["off"], st["last"]["on"]))
        else:
            f.write("\nstep: %s\n" % (st,))
    with open(os.path.join(out_dir, "seqlen_parity.txt"), "w") as f:
        f.write("Training steps given per-sample lengths against the fp64 oracle run on every sample alone at its own length, on one MI355X\n"
                "(python tools/seqlen_bench.py; cases and lengths of tests/seqlen_ref.py, device RNG against the replayed randomness).\n"
                "Deviations relative to the oracle; gradients relative to each tensor's largest entry, best and worst tensor.  The tests\n"
                "bound the rows \"with lengths\" by 1e-4 (loss, loss_b, P at t < len) and 2e-4 (gradients); the rows \"without\" are the same\n"
                "step told only input_length = len - 2: the padded computation.\n\n")
        if isinstance(p, dict) and "rows" in p:
            f.write("%-14s %-13s %10s %10s %10s %12s %12s\n" % ("case", "", "loss", "loss_b", "P", "grad best", "grad worst"))
            for name, label, *e in p["rows"]:
                f.write("%-14s %-13s %10.2e %10.2e %10.2e %12.2e %12.2e\n" % (name, label, *e))
            f.write("\nkernel families (tests/test_gpu_seqlen_scan.py, B = 17, the same real rows embedded at T = 21 and T = 37, bit-equal at t < len):\n")
            for line in p["families"]:
                f.write("  %s\n" % line)
        else:
            f.write("parity: %s\n" % (p,))


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
