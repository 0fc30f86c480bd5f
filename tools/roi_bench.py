#!/usr/bin/env python3
"""Upper-body crop front-end (csrc/roi.hip) throughput at the reference's shapes (640 x 480 BGR frames, img_dim 60):
  * kernel only: `frames` device-resident frames with skeleton-like boxes (about 390 x 360 crops), timed in HIP events;
  * end to end: a synthetic video of `frames` frames as a .npy stack and as a raw bgr24 AVI, through roi_extraction.extract_video
    (read, upload in chunks of CHUNK_FRAMES, launch, download), timed on the host with a warm device;
  * the numpy restatement tests/roi_ref.py on the CPU (a few frames, as a rate).
Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mgr_amd  # noqa: E402,F401
from mgr_amd import _capi  # noqa: E402
from mgr_amd.rgb_network import roi_extraction as roi  # noqa: E402

EV0, EV1 = 10, 11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--img-dim", type=int, default=60)
    ap.add_argument("--iters", type=int, default=50, help="launches per timed window")
    ap.add_argument("--reps", type=int, default=5, help="timed windows")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-reps", type=int, default=5)
    ap.add_argument("--ref-frames", type=int, default=8, help="frames run through the CPU restatement (0: skip)")
    a = ap.parse_args()
    n, D = a.frames, a.img_dim
    rng = np.random.RandomState(0)
    frames = rng.randint(0, 256, (n, roi.FRAME_H, roi.FRAME_W, 3)).astype(np.uint8)
    hx, hy, sy = rng.randint(280, 360, n), rng.randint(280, 320, n), rng.randint(120, 160, n)
    boxes = roi.crop_boxes(hx, hy, sy, n)
    dev = _capi.Device(0)
    d_fr, d_b, d_out = dev.array(frames), dev.array(boxes), dev.empty((n, D, D), np.uint8)
    args = (d_fr, n, roi.FRAME_H, roi.FRAME_W, d_b, D, d_out)
    for _ in range(a.warmup):
        dev.call("mgr_roi_crop", *args)
    dev.sync()
    times = []
    for _ in range(a.reps):       # each window: `iters` back-to-back launches
        dev.record(EV0)
        for _ in range(a.iters):
            dev.call("mgr_roi_crop", *args)
        dev.record(EV1)
        dev.sync()
        times.append(dev.elapsed_ms(EV0, EV1) / a.iters)
    ms = float(np.median(times))
    crop_px = float(((boxes[:, 1] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 2])).mean())
    # bytes the kernel must move: the dwords of the touched rows of each crop, the boxes and the output
    rd = 0
    for y0, y1, x0, x1 in boxes:
        ty = np.floor(((np.arange(D) + 0.5) * (1.0 / (D / (y1 - y0))) - 0.5).astype(np.float32)).astype(np.int64)
        rows = np.unique(np.clip(ty[:, None] - 1 + np.arange(4), 0, y1 - y0 - 1))
        rd += rows.size * 4 * (((3 * x1 + 3) >> 2) - ((3 * x0) >> 2))
    moved = rd + boxes.nbytes + n * D * D
    res = {"metric": "roi_frames_per_s", "frames": n, "img_dim": D, "mean_crop_px": round(crop_px),
           "kernel_ms_median": round(ms, 4), "kernel_ms_min": round(float(np.min(times)), 4),
           "kernel_frames_per_s": round(n / (ms * 1e-3)), "kernel_bytes": int(moved),
           "kernel_GB_s": round(moved / (ms * 1e-3) / 1e9, 1), "device": dev.name}
    for a_ in (d_fr, d_b, d_out):
        a_.free()
    import pandas as pd
    df = pd.DataFrame({"file_number": 1, "hipX": hx, "hipY": hy, "shcY": sy})
    with tempfile.TemporaryDirectory() as tmp:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from avi_writer import write_avi
        paths = {"npy": os.path.join(tmp, "Sample00001_color.npy"), "avi": os.path.join(tmp, "Sample00001_color.avi")}
        np.save(paths["npy"], frames)
        write_avi(paths["avi"], frames)
        roi.extract_video(df, paths["npy"], D, dev=dev)      # warm: library, attributes, allocator
        for kind, p in paths.items():
            best = None
            for _ in range(a.e2e_reps):
                t0 = time.perf_counter()
                out = roi.extract_video(df, p, D, dev=dev)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            assert out.shape == (n, D, D, 1)
            res["e2e_%s_frames_per_s" % kind] = round(n / best)
            res["e2e_%s_s" % kind] = round(best, 4)
    if a.ref_frames > 0:
        import roi_ref
        k = min(a.ref_frames, n)
        t0 = time.perf_counter()
        ref = roi_ref.extract(frames[:k], list(hx), list(hy), list(sy), D)
        res["cpu_ref_frames_per_s"] = round(k / (time.perf_counter() - t0), 1)
        res["cpu_ref_frames"] = k
        got = roi.roi_frames(frames[:k], boxes[:k], D, dev=dev)
        res["gpu_equals_ref"] = bool(np.array_equal(got, ref))
    dev.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
