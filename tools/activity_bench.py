#!/usr/bin/env python3
"""Skeletal activity step (csrc/activity.hip) at the data set's shape (about 470 files x 1,900 frames):
  * kernel only: the joints of `files` files device-resident, one launch, timed in HIP events;
  * end to end: the files as raw SampleNNNNN_data.csv joint files, through activity.extract_activity (parse, upload, launch,
    download, per-file tables) and activity.skeletal_tables (plus gather and the skeletal features), host clock, warm device;
    the parse alone (activity.import_data over the directory) for comparison.
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
from mgr_amd.skeletal_network import activity  # noqa: E402
from mgr_amd.skeletal_network import skeletal_feature_extraction as sfe  # noqa: E402

EV0, EV1 = 10, 11


def walk(rng, n):
    J = rng.integers(150, 450, (1, 20)) + np.cumsum(rng.integers(-4, 5, (n, 20)), axis=0)
    J = np.clip(J, 0, 639)
    J[:, 1::2] = np.minimum(J[:, 1::2], 479)
    return J.astype(np.int32)


def write_raw(path, J):
    cells = np.char.add(np.char.add(np.char.add('[', J[:, 0::2].astype(str)), np.char.add(' ', J[:, 1::2].astype(str))), ']')
    lines = [',' + ','.join(activity.RAW_COLS)] + ['%d,%s' % (i, ','.join(r)) for i, r in enumerate(cells)]
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=470)
    ap.add_argument("--frames", type=int, default=1900)
    ap.add_argument("--iters", type=int, default=20, help="launches per timed window")
    ap.add_argument("--reps", type=int, default=5, help="timed windows")
    ap.add_argument("--e2e-reps", type=int, default=2)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    J = [walk(rng, a.frames) for _ in range(a.files)]
    dev = _capi.Device(0)
    activity._DEV[0] = sfe._DEV[0] = dev
    offs = np.zeros(a.files + 1, np.int64)
    offs[1:] = np.cumsum([j.shape[0] for j in J])
    total = int(offs[-1])
    d_j, d_off = dev.array(np.concatenate(J)), dev.array(offs)
    d_rest, d_out, d_st = dev.empty((a.files, 16), np.int32), dev.empty((total, 5), np.int32), dev.empty((a.files,), np.int32)
    args = (d_j, d_off, a.files, total, 0, d_rest, d_out, d_st)
    for _ in range(3):
        dev.call("mgr_skeletal_activity", *args)
    dev.sync()
    times = []
    for _ in range(a.reps):
        dev.record(EV0)
        for _ in range(a.iters):
            dev.call("mgr_skeletal_activity", *args)
        dev.record(EV1)
        dev.sync()
        times.append(dev.elapsed_ms(EV0, EV1) / a.iters)
    ms = float(np.median(times))
    st = d_st.download()
    res = {"metric": "activity_kernel_ms", "files": a.files, "frames_per_file": a.frames, "frames": total,
           "kernel_ms_median": round(ms, 4), "kernel_ms_min": round(float(np.min(times)), 4),
           "kernel_M_frames_per_s": round(total / (ms * 1e-3) / 1e6, 1), "files_skipped": int((st != 0).sum()), "device": dev.name}
    for x in (d_j, d_off, d_rest, d_out, d_st):
        x.free()
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        for k, j in enumerate(J):
            write_raw(os.path.join(tmp, "Sample%05d_data.csv" % (k + 1)), j)
        res["write_raw_s"] = round(time.perf_counter() - t0, 2)
        names = activity.joint_files(tmp)
        t0 = time.perf_counter()
        for nme in names:
            activity.import_data(tmp, nme)
        res["parse_s"] = round(time.perf_counter() - t0, 3)
        for key, fn in (("extract_activity_s", lambda: activity.extract_activity(tmp, dev=dev)),
                        ("skeletal_tables_s", lambda: activity.skeletal_tables(tmp, dev=dev))):
            best = None
            for _ in range(a.e2e_reps):
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            res[key] = round(best, 3)
    dev.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
