#!/usr/bin/env python3
"""Device time and parity of the posterior-extent and overlap calls; writes profiles/occupancy_timing.txt and
profiles/occupancy_parity.txt (--out-dir: elsewhere).

  timing   mgr_ctc_occupancy with and without gamma beside mgr_ctc_loss_grad (with and without its gradient kernel) and mgr_ctc_align,
           same process, calls interleaved window by window, at B = 64, T = 1900, C = 22, Lmax = 20 and 145; mgr_segment_overlap at
           64 samples x 256 x 256 segments beside the numpy restatement of tests/overlap_ref.py (host time).  HIP events around `iters`
           launches, the median of 5 windows.
  parity   the maxima behind the bounds of tests/test_gpu_occupancy.py: gamma, occ / max(occ), conf (absolute) and logp (relative)
           against the fp64 restatement of tests/occupancy_ref.py, seg against its float32 restatement, at the timing shapes (four
           samples each) and at small random shapes.
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
SKIP, EPS = 2, 1e-8
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


def _occupancy_buffers(dev, P, lab, ll, il=None):
    B, T, Cn = P.shape
    Lmax = lab.shape[1]
    il = np.full(B, T - SKIP, np.int32) if il is None else il
    ins = [dev.array(P), dev.array(lab), dev.array(il), dev.array(ll)]
    outs = [dev.empty((B, T - SKIP, 2 * Lmax + 1)), dev.empty((B, Lmax, 2), np.int32), dev.empty((B, Lmax)), dev.empty((B, Lmax)),
            dev.empty((B,), np.float64)]
    ws = dev.bytes(dev.lib.mgr_ctc_ws_bytes(B, T, Cn, Lmax))
    return ins, outs, ws


def _occupancy_call(dev, ins, outs, ws, shape, q, gamma=True):
    B, T, Cn, Lmax = shape
    dev.call("mgr_ctc_occupancy", *ins, B, T, Cn, Lmax, SKIP, Cn - 1, C.c_float(EPS), C.c_float(q), outs[0] if gamma else None, *outs[1:], ws,
             ws.nbytes)


def step_timing(a):
    from align_bench import peaky
    from mgr_amd import _capi
    dev = _capi.Device(0)
    res = {"device": dev.name, "shapes": []}
    for shape in SHAPES:
        B, T, Cn, Lmax = shape
        P, lab, ll = peaky(np.random.default_rng(Lmax), B, T, Cn, Lmax)
        ins, outs, ws = _occupancy_buffers(dev, P, lab, ll)
        loss, dlog = dev.empty((B,)), dev.empty((B, T, Cn))
        path, wsa = dev.empty((B, T - SKIP), np.int32), dev.bytes(dev.lib.mgr_ctc_align_ws_bytes(B, T, Cn, Lmax))
        tail = (B, T, Cn, Lmax, SKIP, Cn - 1, C.c_float(EPS))
        calls = {
            "occupancy": lambda: _occupancy_call(dev, ins, outs, ws, shape, 0.5),
            "occupancy_no_gamma": lambda: _occupancy_call(dev, ins, outs, ws, shape, 0.5, gamma=False),
            "ctc_loss_grad": lambda: dev.call("mgr_ctc_loss_grad", *ins, *tail, C.c_float(1.0), loss, dlog, ws, ws.nbytes),
            "ctc_loss_no_grad": lambda: dev.call("mgr_ctc_loss_grad", *ins, *tail, C.c_float(1.0), loss, 0, ws, ws.nbytes),
            "ctc_align": lambda: dev.call("mgr_ctc_align", *ins, *tail, path, outs[1], outs[2], outs[4], wsa, wsa.nbytes),
        }
        ms = _timed(dev, calls, a.iters)
        _occupancy_call(dev, ins, outs, ws, shape, 0.5)
        res["shapes"].append({"shape": shape, "mean_label_len": round(float(ll.mean()), 1), "ms": ms,
                              "all_feasible": bool(np.all(np.isfinite(outs[4].download())))})
        for x in ins + outs + [ws, loss, dlog, path, wsa]:
            x.free()
    dev.close()
    return res


def step_overlap(a):
    import overlap_ref as ov
    from mgr_amd import _capi, decoding
    dev = _capi.Device(0)
    rng = np.random.default_rng(0)
    B, S, Cn, n = 64, 256, 21, 1900

    def segs():
        first = rng.integers(0, n, (B, S))
        return [[(int(rng.integers(0, Cn)), int(f), int(f) + int(rng.integers(0, 40))) for f in row] for row in first]
    hyp, ref = segs(), segs()
    hl, hs = decoding.pack_segments(hyp)
    rl, rs = decoding.pack_segments(ref)
    ins = [dev.array(x) for x in (hl, hs, rl, rs, np.full(B, n, np.int32))]
    outs = [dev.empty((B, Cn), np.int32) for _ in range(4)]
    call = lambda: dev.call("mgr_segment_overlap", ins[0], ins[1], S, ins[2], ins[3], S, ins[4], B, Cn, 0, *outs)
    ms = _timed(dev, {"segment_overlap": call}, a.iters)
    host = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        want = ov.overlap(hyp, ref, Cn, n)
        host.append((time.perf_counter() - t0) * 1e3)
    got = [o.download() for o in outs]
    dev.close()
    return {"shape": [B, S, S, Cn, n], "ms": ms, "numpy_ms": [round(float(np.median(host)), 2), round(float(np.min(host)), 2)],
            "equal": bool(all(np.array_equal(g, w) for g, w in zip(got, want)))}


def step_parity(a):
    import occupancy_ref as oc
    from align_bench import peaky
    from mgr_amd import _capi
    dev = _capi.Device(0)
    rows = []
    cases = [("peaky B=4 T=1900 C=22 Lmax=%d" % L, peaky(np.random.default_rng(L), 4, 1900, 22, L)) for L in (20, 145)]
    for seed, (B, T, Cn, Lmax) in enumerate([(5, 40, 3, 4), (5, 259, 22, 65), (3, 131, 22, 100), (3, 67, 22, 200)]):
        rng = np.random.default_rng(seed)
        P = rng.dirichlet(np.full(Cn, 0.3), size=(B, T)).astype(np.float32)
        ll = rng.integers(1, min(Lmax, (T - SKIP) // 2) + 1, B).astype(np.int32)
        lab = -np.ones((B, Lmax), np.int32)
        for b in range(B):
            lab[b, :ll[b]] = rng.integers(0, Cn - 1, ll[b])
        cases.append(("dirichlet(0.3) B=%d T=%d C=%d Lmax=%d" % (B, T, Cn, Lmax), (P, lab, ll)))
    for name, (P, lab, ll) in cases:
        B, T, Cn = P.shape
        shape = (B, T, Cn, lab.shape[1])
        ins, outs, ws = _occupancy_buffers(dev, P, lab, ll)
        for q in (0.5, 0.05):
            _occupancy_call(dev, ins, outs, ws, shape, q)
            gamma, seg, occ, conf, logp = [o.download() for o in outs]
            w = dict(gamma=0.0, occ=0.0, conf=0.0, logp=0.0, seg_mismatch=0, seg_vs_fp64=0)
            for b in range(B):
                L = int(ll[b])
                ref = oc.occupancy(P[b], lab[b, :L], None, q, SKIP)
                w["gamma"] = max(w["gamma"], float(np.abs(gamma[b, :, :2 * L + 1] - ref["gamma"]).max()))
                w["occ"] = max(w["occ"], float(np.abs(occ[b, :L] - ref["occ"]).max() / ref["occ"].max()))
                w["conf"] = max(w["conf"], float(np.abs(conf[b, :L] - ref["conf"]).max()))
                w["logp"] = max(w["logp"], float(abs(logp[b] - ref["logp"]) / abs(ref["logp"])))
                mine = [tuple(r) for r in seg[b, :L]]
                w["seg_mismatch"] += sum(x != y for x, y in zip(mine, oc.extents_from_gamma(gamma[b], q, L, SKIP)))
                w["seg_vs_fp64"] += sum(x != y for x, y in zip(mine, ref["seg"]))
            rows.append({"case": name, "q": q, "labels": int(ll.sum()), **w})
        for x in ins + outs + [ws]:
            x.free()
    dev.close()
    return {"rows": rows}


STEPS = {"timing": (step_timing, 240), "overlap": (step_overlap, 120), "parity": (step_parity, 300)}


def write_reports(res, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    t, o, p = res.get("timing"), res.get("overlap"), res.get("parity")
    with open(os.path.join(out_dir, "occupancy_timing.txt"), "w") as f:
        f.write("mgr_ctc_occupancy / mgr_segment_overlap alone on one MI355X (python tools/occupancy_bench.py): device time per call in ms, HIP\n"
                "events around %d launches, median (min) of %d windows, the calls of a shape interleaved window by window in one process.\n"
                "Posteriors are run-structured and blank-dominated (tools/align_bench.py: peaky); every sample carries up to Lmax labels.\n"
                "No time target was set: the call shares the loss's emission and chain kernels and should cost about what the loss costs.\n\n"
                % (res["iters"], WINDOWS))
        if isinstance(t, dict) and "shapes" in t:
            f.write("device: %s\n" % t["device"])
            for s_ in t["shapes"]:
                ms = s_["ms"]
                f.write("\nB=%d T=%d C=%d Lmax=%d (mean label length %.1f, all feasible: %s)\n" % (*s_["shape"], s_["mean_label_len"], s_["all_feasible"]))
                for k, v in ms.items():
                    f.write("  %-20s %8.4f (%.4f)\n" % (k, v[0], v[1]))
                base, ng = ms["ctc_loss_grad"][0], ms["ctc_loss_no_grad"][0]
                f.write("  ratios of the medians: occupancy / loss+grad %.2f, occupancy without gamma / loss+grad %.2f, occupancy without gamma / "
                        "loss without grad %.2f, occupancy / align %.2f\n"
                        % (ms["occupancy"][0] / base, ms["occupancy_no_gamma"][0] / base, ms["occupancy_no_gamma"][0] / ng,
                           ms["occupancy"][0] / ms["ctc_align"][0]))
        else:
            f.write("timing step: %s\n" % (t,))
        if isinstance(o, dict) and "ms" in o:
            f.write("\nmgr_segment_overlap, B=%d samples x %d x %d segments, C=%d, %d frames: %.4f (%.4f) ms; the numpy restatement "
                    "(tests/overlap_ref.py, host time) %.2f (%.2f) ms: %.0f x; results equal: %s\n"
                    % (*o["shape"], *o["ms"]["segment_overlap"], *o["numpy_ms"], o["numpy_ms"][0] / o["ms"]["segment_overlap"][0], o["equal"]))
        else:
            f.write("\noverlap step: %s\n" % (o,))
    with open(os.path.join(out_dir, "occupancy_parity.txt"), "w") as f:
        f.write("mgr_ctc_occupancy against the fp64 restatement of tests/occupancy_ref.py on one MI355X (python tools/occupancy_bench.py): the\n"
                "largest deviation over all samples of a case.  gamma, conf: absolute; occ: absolute / max(occ) of the sample; logp: relative.\n"
                "The tests bound the first three by 1e-4 and logp by 1e-4.  seg_mismatch: labels whose extent differs from the float32\n"
                "sequential restatement applied to the kernel's own gamma (must be 0); seg_vs_fp64: labels whose extent differs from the fp64\n"
                "restatement's (allowed: a cumulative sum within rounding of the quantile).\n\n")
        if isinstance(p, dict) and "rows" in p:
            f.write("%-44s %5s %7s %10s %10s %10s %10s %12s %11s\n" % ("case", "q", "labels", "gamma", "occ", "conf", "logp", "seg_mismatch", "seg_vs_fp64"))
            for r in p["rows"]:
                f.write("%-44s %5g %7d %10.2e %10.2e %10.2e %10.2e %12d %11d\n"
                        % (r["case"], r["q"], r["labels"], r["gamma"], r["occ"], r["conf"], r["logp"], r["seg_mismatch"], r["seg_vs_fp64"]))
        else:
            f.write("parity step: %s\n" % (p,))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="launches per timed window")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process and print its JSON line")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(STEPS[a.step][0](a)))
        return
    res = {"iters": a.iters}
    for name, (_, limit) in STEPS.items():
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--iters", str(a.iters)], stdout=subprocess.PIPE,
                               timeout=limit)
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
