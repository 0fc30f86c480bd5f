#!/usr/bin/env python3
"""Device time of the expected-risk gradient (csrc/risk.hip) against the only way to the same gradient without it - mgr_ctc_rescore
for the K scores, then K calls of mgr_ctc_loss_grad with their gradients, one hypothesis column each; the host pass that forms the
weights from the scores and combines the K gradients is NOT in the composition's time - and the cost of the minimum-risk training
mode in a config-F training step.  Same process, the ways alternating window by window, HIP events around `iters` repetitions, median
(min) over `reps` windows; the training steps are wall-clock per step over `steps` steps behind a warm-up, mode off / on / off.
--part sample: the sampler mgr_ctc_sample_paths against the beam search mgr_ctc_beam_search_lm at equal B, T, C and K =
top_paths (8 and 32), timed the same way, and the config-F step with the mode off / source="beam" / source="sample" / off, into
--sample-out.  Recorded, with no target.  Prints one JSON line per part and writes the tables to --out / --sample-out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mgr_amd  # noqa: E402,F401  (before numpy: _hostenv.py)
import numpy as np  # noqa: E402
from mgr_amd import _capi, decoding  # noqa: E402
from rescore_bench import edits, peaky  # noqa: E402

EV0, EV1 = 10, 11
SKIP, EPS = 2, 1e-8


def kernel_part(dev, B, T, Cn, K, iters, reps):
    rng = np.random.default_rng(15)
    truths = [[int(g) for g in rng.integers(0, Cn - 1, int(rng.integers(8, 37)))] for _ in range(B)]
    P = np.stack([peaky(rng, T, Cn, t) for t in truths])
    paths = [edits(rng, t, Cn - 1, K, 40) for t in truths]
    hyp, hyp_len = decoding.pack_nbest(paths, K=K, width=T - SKIP)
    lab, lab_len = decoding.pack_nbest(paths, K=K)
    Lmax, Lcap = lab.shape[2], decoding.risk_label_cap(hyp, hyp_len)
    risks = rng.integers(0, 6, (B, K)).astype(np.int32)
    dP, dil, dh, dl, dr = dev.array(P), dev.array(np.full(B, T - SKIP, np.int32)), dev.array(hyp), dev.array(hyp_len), dev.array(risks)
    dlogp, dw, de, dg = dev.empty((B, K), np.float64), dev.empty((B, K), np.float32), dev.empty((B,), np.float32), dev.empty((B, T, Cn))
    ws_bytes = dev.lib.mgr_ctc_risk_ws_bytes(B, T, Cn, K, Lcap, 0, None)
    ws = dev.bytes(ws_bytes)
    cols = [(dev.array(np.ascontiguousarray(lab[:, k])), dev.array(np.ascontiguousarray(lab_len[:, k]))) for k in range(K)]
    dloss, dgk = dev.empty((B,), np.float32), [dev.empty((B, T, Cn)) for _ in range(K)]
    wsl = dev.bytes(max(dev.lib.mgr_ctc_ws_bytes(B, T, Cn, Lmax), dev.lib.mgr_ctc_rescore_ws_bytes(B, T, Cn, 0, None)))
    eps, one = C.c_float(EPS), C.c_float(1.0)

    def new():
        dev.call("mgr_ctc_risk_grad", dP, dil, B, T, Cn, SKIP, Cn - 1, eps, None, None, 0, dh, dl, K, T - SKIP, Lcap, dr, one, one, one, 0,
                 dlogp, dw, de, dg, ws, ws.nbytes)

    def old():
        dev.call("mgr_ctc_rescore", dP, dil, B, T, Cn, SKIP, Cn - 1, eps, None, None, 0, dh, dl, K, T - SKIP, dlogp, None, wsl, wsl.nbytes)
        for k in range(K):
            dev.call("mgr_ctc_loss_grad", dP, cols[k][0], dil, cols[k][1], B, T, Cn, Lmax, SKIP, Cn - 1, eps, one, dloss, dgk[k], wsl,
                     wsl.nbytes)

    calls = {"risk_grad": new, "composition": old}
    for fn in calls.values():
        for _ in range(3):
            fn()
    dev.sync()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            dev.record(EV0)
            for _ in range(iters):
                fn()
            dev.record(EV1)
            dev.sync()
            times[k].append(dev.elapsed_ms(EV0, EV1) / iters)
    for a in [dP, dil, dh, dl, dr, dlogp, dw, de, dg, ws, dloss, wsl] + dgk + [x for c in cols for x in c]:
        a.free()
    return {"B": B, "T": T, "C": Cn, "K": K, "Lcap": int(Lcap), "ws_bytes": int(ws_bytes),
            "ms_median": {k: round(float(np.median(v)), 4) for k, v in times.items()},
            "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()}}


def sample_kernel_part(dev, B, T, Cn, K, beam, iters, reps):
    """mgr_ctc_sample_paths against mgr_ctc_beam_search_lm (no tables, top_paths = K) on the same posteriors."""
    rng = np.random.default_rng(16)
    truths = [[int(g) for g in rng.integers(0, Cn - 1, int(rng.integers(8, 37)))] for _ in range(B)]
    P = np.stack([peaky(rng, T, Cn, t) for t in truths])
    dP, dil = dev.array(P), dev.array(np.full(B, T - SKIP, np.int32))
    out, out_len = dev.empty((B, K, T - SKIP), np.int32), dev.empty((B, K), np.int32)
    count, nu = dev.empty((B, K), np.int32), dev.empty((B,), np.int32)
    score, lctc, ext = dev.empty((B, K), np.float64), dev.empty((B, K), np.float64), dev.zeros((Cn + 1, Cn), np.float64)
    ws = dev.bytes(dev.lib.mgr_ctc_beam_lm_ws_bytes(B, T, Cn, beam, K))
    eps = C.c_float(EPS)
    seed = [0]

    def sample():
        seed[0] += 1
        dev.call("mgr_ctc_sample_paths", dP, dil, B, T, Cn, SKIP, Cn - 1, eps, C.c_uint64(seed[0]), K, out, out_len, count, nu, None)

    def search():
        dev.call("mgr_ctc_beam_search_lm", dP, dil, B, T, Cn, SKIP, Cn - 1, beam, eps, ext, None, K, out, out_len, score, lctc, ws, ws.nbytes)

    calls = {"sample_paths": sample, "beam_search_lm": search}
    for fn in calls.values():
        fn()
    dev.sync()
    unique = float(nu.download().mean())     # (of the sampler's last call: search ran after it, but into out / out_len only)
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            dev.record(EV0)
            for _ in range(iters):
                fn()
            dev.record(EV1)
            dev.sync()
            times[k].append(dev.elapsed_ms(EV0, EV1) / iters)
    for a in (dP, dil, out, out_len, count, nu, score, lctc, ext, ws):
        a.free()
    return {"B": B, "T": T, "C": Cn, "K": K, "beam_width": beam, "mean_unique": round(unique, 2),
            "ms_median": {k: round(float(np.median(v)), 4) for k, v in times.items()},
            "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()}}


def step_part(dev, steps, warmup, cfg, modes=None):
    from mgr_amd.configs import baseline_config
    from mgr_amd.engine import Engine
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    spec, B, T, Lmax = baseline_config("F")
    eng = Engine(spec, B, T, Lmax, device=dev, seed=1)
    eng.set_weights(synthetic_weights(spec, 3))
    xs, labels, il, ll = synthetic_arrays(spec, B, T, Lmax, 9)
    out = {"config": "F", "B": B, "T": T, "Lmax": Lmax, "cfg": {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, "ms_per_step": {}}
    for name, c in modes or (("off", None), ("on", cfg), ("off_again", None)):
        eng.set_risk(c)
        for _ in range(warmup):
            eng.train_step(xs, labels, il, ll, next_inputs=xs)
        dev.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.train_step(xs, labels, il, ll, next_inputs=xs)
        dev.sync()
        out["ms_per_step"][name] = round((time.perf_counter() - t0) * 1e3 / steps, 3)
        if c is not None:      # what the risk kernels had to work on in the last step: labels per present slot, share of slots scored
            n, lp = eng._risk["out_len"].download(), eng._risk["logp"].download()
            out.setdefault("slots", {})[name] = {"present": int((n >= 0).sum()), "mean_labels": round(float(n[n >= 0].mean()), 1),
                                                 "live": int(np.isfinite(lp).sum()), "of": int(n.size)}
    out["max_labels"] = min(255, max(2 * Lmax, 16)) if cfg.get("max_labels") is None else cfg["max_labels"]
    eng.close()
    return out


def sample_main(dev, a, cfg):
    ks = [sample_kernel_part(dev, a.batch, a.maxlen, 22, K, beam, a.iters, a.reps) for K, beam in ((8, 16), (32, 32))]
    modes = (("off", None), ("beam", dict(cfg, source="beam")), ("sample", dict(cfg, source="sample")), ("off_again", None))
    s = step_part(dev, a.steps, a.warmup, cfg, modes)
    res = {"metric": "ctc_sample_ms", "device": dev.name, "iters": a.iters, "reps": a.reps, "kernel": ks, "step": s}
    ms = s["ms_per_step"]
    lines = ["mgr_ctc_sample_paths against mgr_ctc_beam_search_lm (no tables, top_paths = K) on the same posteriors, one MI355X (%s):" % res["device"],
             "device time in ms, HIP events around %d repetitions, median (min) of %d windows, the two alternating; a new seed per call." % (
                 a.iters, a.reps), "",
             "%4s %5s %3s %3s %5s %8s  %-20s %-22s %8s" % ("B", "T", "C", "K", "beam", "unique", "sample_paths", "beam_search_lm", "ratio")]
    for k in ks:
        m, lo = k["ms_median"], k["ms_min"]
        lines.append("%4d %5d %3d %3d %5d %8.2f  %-20s %-22s %7.1fx" % (
            k["B"], k["T"], k["C"], k["K"], k["beam_width"], k["mean_unique"], "%.4f (%.4f)" % (m["sample_paths"], lo["sample_paths"]),
            "%.4f (%.4f)" % (m["beam_search_lm"], lo["beam_search_lm"]), m["beam_search_lm"] / m["sample_paths"]))
    lines += ["(unique: the mean number of unique labellings per sample among the K draws of one call)", "",
              "Config-F training step (B %d, T %d, Lmax %d), wall-clock ms per step over %d steps behind %d warm-up steps, the same batch, the"
              % (s["B"], s["T"], s["Lmax"], a.steps, a.warmup),
              "next batch announced, one engine, the modes in this order (%s):" % ", ".join("%s=%s" % kv for kv in s["cfg"].items()),
              "mode off %.3f | source=beam %.3f | source=sample %.3f | off again %.3f" % (ms["off"], ms["beam"], ms["sample"], ms["off_again"]),
              "The hypothesis slots of the last timed step (synthetic weights: the posteriors are near uniform, the labellings long):"]
    lines += ["  source=%-6s %d of %d slots present, %.1f labels each on average, %d live (scored: at most max_labels = %s labels)"
              % (k, v["present"], v["of"], v["mean_labels"], v["live"], s.get("max_labels")) for k, v in s["slots"].items()]
    lines += ["A slot that is not scored costs mgr_ctc_risk_grad no lattice; with every slot live the call takes the time of profiles/risk_timing.txt."]
    os.makedirs(os.path.dirname(os.path.abspath(a.sample_out)), exist_ok=True)
    with open(a.sample_out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--maxlen", type=int, default=1900)
    ap.add_argument("--hyps", type=int, default=8, help="hypotheses per sample (K)")
    ap.add_argument("--iters", type=int, default=5, help="repetitions per timed window")
    ap.add_argument("--reps", type=int, default=7, help="timed windows per way")
    ap.add_argument("--steps", type=int, default=20, help="timed training steps per mode")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "risk_timing.txt"))
    ap.add_argument("--part", choices=("risk", "sample", "all"), default="all")
    ap.add_argument("--sample-out", default=os.path.join(ROOT, "profiles", "risk_sample_timing.txt"))
    a = ap.parse_args()
    dev = _capi.Device(0)
    cfg = dict(top_paths=a.hyps, beam_width=16, ctc_weight=0.1, costs=(1, 1, 1), post_scale=1.0)
    if a.part in ("sample", "all"):
        sample_main(dev, a, cfg)
    if a.part == "sample":
        dev.close()
        return
    k = kernel_part(dev, a.batch, a.maxlen, 22, a.hyps, a.iters, a.reps)
    s = step_part(dev, a.steps, a.warmup, cfg)
    res = {"metric": "ctc_risk_ms", "device": dev.name, "iters": a.iters, "reps": a.reps, "kernel": k, "step": s}
    dev.close()
    m, lo = k["ms_median"], k["ms_min"]
    lines = ["mgr_ctc_risk_grad against mgr_ctc_rescore + K calls of mgr_ctc_loss_grad (with gradients) on the same posteriors, one MI355X (%s):"
             % res["device"],
             "device time in ms, HIP events around %d repetitions, median (min) of %d windows, the two ways alternating.  The composition's"
             % (a.iters, a.reps),
             "host pass (weights from the scores, the K gradients combined) is not in its time.", "",
             "%4s %5s %3s %3s %5s %10s  %-20s %-20s %7s" % ("B", "T", "C", "K", "Lcap", "ws MiB", "one call", "composition", "ratio"),
             "%4d %5d %3d %3d %5d %10.1f  %-20s %-20s %6.2fx" % (k["B"], k["T"], k["C"], k["K"], k["Lcap"], k["ws_bytes"] / 2.0 ** 20,
                                                                "%.4f (%.4f)" % (m["risk_grad"], lo["risk_grad"]),
                                                                "%.4f (%.4f)" % (m["composition"], lo["composition"]),
                                                                m["composition"] / m["risk_grad"]), "",
             "Config-F training step (B %d, T %d, Lmax %d), wall-clock ms per step over %d steps behind %d warm-up steps, the same batch, the"
             % (s["B"], s["T"], s["Lmax"], a.steps, a.warmup),
             "next batch announced: mode off %.3f | on (%s) %.3f | off again %.3f" % (
                 s["ms_per_step"]["off"], ", ".join("%s=%s" % kv for kv in s["cfg"].items()), s["ms_per_step"]["on"], s["ms_per_step"]["off_again"])]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
