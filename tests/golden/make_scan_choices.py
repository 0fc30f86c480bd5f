"""Writes tests/golden/scan_choices.json: what the multi-scan calls (mgr_lstm_scan_fwd_multi_ex, mgr_lstm_scan_bwd_multi_ex) of a
REFERENCE commit launch for a list of job shapes, launch forms and tune keys - observed on the GPU, since that commit exposes no
decision.  tests/test_cpu_scan_choice.py asserts that the decision functions of the tree (csrc/scan_choice.h, printed by
mgr_lstm_scan_fwd_describe / mgr_lstm_scan_bwd_describe) say the same - so the fixture is made from the library of the commit BEFORE a
change of the launchers, never from the code under test.

Two steps.  On a box with the GPU, ONE process under ONE time limit, the kernel trace on its own (no counters, no other tracing),
the program behind "--":

    rocprofv3 --kernel-trace -f csv -d <dir> -- python tests/golden/make_scan_choices.py record <raw.json>

Per case the recorder sets the tune keys (MGR_TUNE_SCAN_SYNC_CHECK = 1 throughout), asks the context-aware workspace query, makes the
call on zeroed operands, and notes: return code and error text, the bytes the query said, whether opts->seq_out got a launch number
(the launch entered the residency ledger) or MGR_SEQ_NONE, and the mgr_persist_stats delta.  A one-workgroup k_mean launch sits in
front of the first case and behind every case: it separates the cases in the trace.  The recorder stops at the first HIP failure or
nonzero scan status.  Then, anywhere:

    python tests/golden/make_scan_choices.py merge <raw.json> <..._kernel_trace.csv> <commit id> [<out.json>]

cuts the trace at the separators and writes, per case, the ordered launches as [kernel name without namespace and arguments, grid in
WORKGROUPS (the trace counts work-items: divided), workgroup size, LDS bytes as traced].  The LDS figure is what the profiler shows
(it may round): it is compared trace to trace only (profiles/scan_choice_parity.txt), never with the decision.

T is between 5 and 9 throughout: the launch geometry depends on B and H only, every case takes well under a second.
"""
import csv
import ctypes as C
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "scan_choices.json")

HS = [500, 300, 128, 100, 64, 32, 16, 12, 30]     # 30 is no multiple of 4: the simple kernel
BS = [16, 17, 64]
LDT = 32
# tune keys (include/mgr.h)
PATH, NO_XCD, FORM, LDS_IMAGE, SPLIT_ROLE, F32, BPTT_FORM, SINGLE_CU = 0, 3, 4, 7, 8, 14, 16, 19
AUTO, PLAIN, FUSED, FUSED_ANY = 0, 1, 3, 4


def fj(H, B, T=7, Y=1, YT=1, split=0):
    return dict(H=H, B=B, T=T, Y=Y, YT=YT, yt_split=split)


def bj(H, B, T=7, dzmax=1, dbsum=1):
    return dict(H=H, B=B, T=T, dzmax=dzmax, dbsum=dbsum)


def cases():
    out = []

    def fwd(jobs, form=AUTO, tune=None, ws="exact"):
        out.append(dict(dir="fwd", jobs=jobs, form=form, tune={str(k): v for k, v in (tune or {}).items()}, ws=ws))

    def bwd(jobs, form=0, tune=None):
        out.append(dict(dir="bwd", jobs=jobs, form=form, tune={str(k): v for k, v in (tune or {}).items()}))

    def layers(mk, hs, B, **kw):
        return [mk(H, B, **kw) for H in hs for _ in range(2)]

    # ---- forward
    for H in HS:
        for B in BS:
            fwd([fj(H, B, T=5 + (H + B) % 5)])                      # one job
            fwd(layers(fj, [H], B), PLAIN)                          # the two directions of a layer
    for H in (500, 300, 128, 100):
        for B in BS:
            for form in (FUSED, FUSED_ANY):
                fwd(layers(fj, [H], B), form)
    for hs in ((500, 300), (100, 300)):                             # two layers x two directions
        for B in BS:
            for form in (AUTO, PLAIN, FUSED, FUSED_ANY):
                fwd(layers(fj, hs, B), form)
    for jobs in (layers(fj, [500], 64), layers(fj, [100], 17), layers(fj, [500, 300], 64)):
        fwd(jobs, AUTO, {FORM: 3})
    for path in range(5):
        for H in (500, 100, 32, 30):
            fwd(layers(fj, [H], 17), AUTO, {PATH: path})
    for key in (LDS_IMAGE, F32, NO_XCD):
        for H in (500, 300, 128, 100):
            for B in (17, 64):
                for form in (PLAIN, FUSED_ANY):
                    fwd(layers(fj, [H], B), form, {key: 1})
    for H in (500, 100, 64, 30):                                    # with and without Y, YT, split rows
        for Y, YT, split in ((1, 0, 0), (1, 1, 1), (0, 1, 0), (0, 1, 1)):
            fwd(layers(fj, [H], 17, Y=Y, YT=YT, split=split), PLAIN)
    fwd(layers(fj, [100], 17, Y=0), PLAIN, {LDS_IMAGE: 1})          # a K-split shape on the LDS-image step: rows in scratch
    fwd(layers(fj, [100], 17, Y=0), FUSED_ANY, {F32: 1})
    fwd([fj(100, 17), fj(100, 17, Y=0), fj(64, 17, Y=0), fj(30, 17, Y=0)], PLAIN)
    fwd(layers(fj, [100], 17), PLAIN, ws="degrade")                 # a workspace of base_need - 256 bytes
    fwd(layers(fj, [500], 64), FUSED, ws="degrade")
    fwd(layers(fj, [100], 17, Y=0), PLAIN, ws="degrade")            # ... and no room for the rows either: refused
    # more workgroups than the chip holds at once: the plan leaves such a list to the other families (no host refusal is reachable:
    # the planner counts every job rounded up to 8 workgroups, the launcher's co-residency check never sees more than it accepts)
    fwd([fj(500, 64, T=5) for _ in range(8)], PLAIN)
    fwd([fj(300, 64, T=5) for _ in range(8)], PLAIN, {PATH: 3})
    # ---- backward
    for H in HS:
        for B in BS:
            bwd([bj(H, B, T=5 + (H + B) % 5)])
        for form in range(7):
            bwd(layers(bj, [H], 17), form)
    for H in (500, 300, 100):
        for form in range(7):
            bwd(layers(bj, [H], 64), form)
    for H in (500, 128, 100):
        for v in (0, 1, 2):
            bwd(layers(bj, [H], 17), 0, {BPTT_FORM: v})
    for H in (500, 300, 100, 16):
        for B in (17, 64):
            for v in (0, 1, 2):
                bwd(layers(bj, [H], B), 0, {SPLIT_ROLE: v})
    for H in (500, 128, 100, 64, 32):
        for v in (0, 1):
            bwd(layers(bj, [H], 17), 0, {SINGLE_CU: v})
    bwd(layers(bj, [100], 17), 0, {SINGLE_CU: 1, F32: 1})
    bwd(layers(bj, [100], 17), 6, {F32: 1})
    bwd(layers(bj, [100], 17), 6, {PATH: 1})
    bwd([bj(100, 17), bj(64, 17)], 6)                               # not the directions of ONE layer: the cluster kernels
    for path in (0, 1, 3):
        for H in (500, 100, 30, 12):
            bwd(layers(bj, [H], 17), 0, {PATH: path})
    for H in (500, 100, 64, 30):
        for dzmax, dbsum in ((0, 0), (1, 0), (0, 1)):
            bwd(layers(bj, [H], 17, dzmax=dzmax, dbsum=dbsum), 0)
    for key in (F32, NO_XCD):
        for H in (500, 100):
            for B in (17, 64):
                for form in (0, 2, 3, 4, 5):
                    bwd(layers(bj, [H], B), form, {key: 1})
    bwd(layers(bj, [500], 17), 0, {F32: 1, SPLIT_ROLE: 1})
    bwd(layers(bj, [100], 17), 0, {SPLIT_ROLE: 2})
    for hs in ((100, 300), (500, 300), (30, 100), (64, 100)):       # mixed shapes
        for form in (0, 4):
            bwd(layers(bj, hs, 17), form)
        bwd(layers(bj, hs, 64), 0)
    # left-over jobs.  Every width of HS with an instantiation of the single-CU MFMA kernel has a cluster instantiation too; H = 4 has
    # the former only, and MGR_TUNE_SCAN_PATH = 2 keeps every job off the cluster kernels
    bwd(layers(bj, [4], 17), 0)                                     # ... of one shape: ONE launch of the single-CU MFMA kernel
    bwd(layers(bj, [64], 64), 0, {PATH: 2})
    bwd([bj(64, 17), bj(32, 17)], 0, {PATH: 2})                     # ... of two shapes: one launch each
    bwd([bj(4, 17), bj(4, 17), bj(12, 17)], 0)                      # ... and the simple kernel where there is no instantiation
    bwd([bj(100, 17), bj(100, 17), bj(4, 16), bj(4, 16)], 4)        # ... behind a cluster launch
    bwd(layers(bj, [64], 17), 0, {PATH: 1})                         # MGR_TUNE_SCAN_PATH = 1: the simple kernel whatever the width
    bwd([bj(64, 17), bj(30, 17), bj(12, 17)], 0, {PATH: 1})
    bwd([bj(64, 17), bj(30, 17)], 0)                                # a cluster job beside a left-over one
    bwd([bj(100, 17), bj(100, 17), bj(30, 16), bj(30, 16)], 4)
    bwd([bj(500, 64, T=5) for _ in range(8)], 0)                    # more workgroups than the chip holds: no cluster launch
    return out


# ---- record (GPU)
def record(raw_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import mgr_amd  # noqa: F401
    from mgr_amd import _capi
    dev = _capi.Device(0)
    lib = dev.lib
    NS, BM, TM, HM = 4, 64, 9, 500
    pool = [dict(Z=dev.zeros((BM * TM * 4 * HM,)), Up=dev.zeros((HM * 4 * HM,)), Y=dev.zeros((BM * TM * HM,)), gates=dev.zeros((BM * TM * 4 * HM,)),
                 cs=dev.zeros((BM * TM * HM,)), YT=dev.zeros((BM * HM * LDT,)), dY=dev.zeros((BM * TM * HM,)), dZ=dev.zeros((BM * TM * 4 * HM,)),
                 dzmax=dev.zeros((BM * 4 * HM,)), dbsum=dev.zeros((BM * 4 * HM,))) for _ in range(NS)]
    ws = dev.zeros((40 << 20,))
    mean_out = dev.zeros((8,))
    seq = dev.pinned((4,), np.uint32)
    status = (C.c_uint * 4)()

    def separator():
        dev.call("mgr_mean", mean_out, 4, mean_out.ptr + 16)

    def stats():
        a, b = C.c_int(), C.c_int()
        _capi.check(lib.mgr_persist_stats(dev.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    dev.call("mgr_tune", 1, 1)
    dev.call("mgr_scan_status_clear")
    dev.sync()
    separator()
    res = []
    stopped = None
    for n, case in enumerate(cases()):
        for k, v in case["tune"].items():
            dev.call("mgr_tune", int(k), v)
        seq[0] = 0x12345678
        opts = _capi.make_launch_opts(case["form"], seq.ctypes.data)
        s0 = stats()
        nj = len(case["jobs"])
        if case["dir"] == "fwd":
            arr = _capi.make_scan_jobs([dict(Z=pool[i % NS]["Z"], Up=pool[i % NS]["Up"], Y=pool[i % NS]["Y"] if j["Y"] else 0, ldy=j["H"] if j["Y"] else 0,
                                             gates=pool[i % NS]["gates"], cs=pool[i % NS]["cs"], B=j["B"], T=j["T"], H=j["H"], reverse=i & 1,
                                             YT=pool[i % NS]["YT"] if j["YT"] else 0, ytb=j["H"] * LDT if j["YT"] else 0, ldt=LDT if j["YT"] else 0,
                                             yt_split=j["yt_split"]) for i, j in enumerate(case["jobs"])])
            need = lib.mgr_lstm_scan_fwd_multi_ws_bytes(dev.ctx, nj, arr, C.byref(opts))
            upper = lib.mgr_lstm_scan_multi_ws_bytes(nj, arr)
            give = need
            if case["ws"] == "degrade":     # header + exchange images less 256 bytes: what the upper bound says for the same jobs WITH rows
                full = _capi.make_scan_jobs([dict(Z=1 << 16, Up=1 << 16, Y=1 << 16, ldy=j["H"], B=j["B"], T=j["T"], H=j["H"]) for j in case["jobs"]])
                give = lib.mgr_lstm_scan_multi_ws_bytes(nj, full) - 256
            assert give <= ws.nbytes
            rc = lib.mgr_lstm_scan_fwd_multi_ex(dev.ctx, nj, arr, ws.ptr if give else None, give, C.byref(opts))
            rec = dict(need=need, upper=upper, ws_bytes=give)
        else:
            arr = _capi.make_scan_bwd_jobs([dict(dY=pool[i % NS]["dY"], gates=pool[i % NS]["gates"], cs=pool[i % NS]["cs"], Up=pool[i % NS]["Up"],
                                                 dZ=pool[i % NS]["dZ"], lddy=j["H"], B=j["B"], T=j["T"], H=j["H"], reverse=i & 1,
                                                 dzmax=pool[i % NS]["dzmax"] if j["dzmax"] else 0, dbsum=pool[i % NS]["dbsum"] if j["dbsum"] else 0)
                                            for i, j in enumerate(case["jobs"])])
            need = lib.mgr_lstm_scan_bwd_multi_ws_bytes(nj, arr)
            assert need <= ws.nbytes
            rc = lib.mgr_lstm_scan_bwd_multi_ex(dev.ctx, nj, arr, ws.ptr, need, C.byref(opts))
            rec = dict(need=need)
        err = lib.mgr_last_error().decode(errors="replace") if rc != 0 else ""
        if rc == 0 or rc == -1:
            dev.sync()
        s1 = stats()
        rec.update(rc=rc, err=err, ledger=int(seq[0] not in (0x12345678, _capi.SEQ_NONE)), seq_word="none" if seq[0] == _capi.SEQ_NONE else
                   ("kept" if seq[0] == 0x12345678 else "seq"), persist=[s1[0] - s0[0], s1[1] - s0[1]])
        res.append(dict(case, **rec))
        for k in case["tune"]:
            dev.call("mgr_tune", int(k), 0)
        if rc not in (0, -1):
            stopped = "case %d: rc %d: %s" % (n, rc, err)
            break
        dev.call("mgr_scan_status_ex", status)
        if status[0] != 0:
            stopped = "case %d: scan status %d" % (n, status[0])
            break
        separator()
        dev.sync()
    with open(raw_path, "w") as f:
        json.dump(dict(cu_count=dev.cu_count, device=dev.name, stopped=stopped, cases=res), f)
    print("recorded %d of %d cases on %s (%d CUs)%s" % (len(res), len(cases()), dev.name, dev.cu_count, "; STOPPED: " + stopped if stopped else ""))
    dev.close()
    return 1 if stopped else 0


# ---- merge (anywhere)
def short_name(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    name = re.sub(r"\(.*\)\s*(\[clone.*\])?$", "", name).strip()
    return re.sub(r"\.kd$", "", name)


def read_trace(path):
    """The launches of a rocprofv3 kernel trace in dispatch order, cut at the k_mean separators: a list (per case) of
    [name, grid in workgroups, workgroup size, LDS bytes]."""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))

    def dims(r, what):
        if what + "_X" in r:
            return [int(r[what + "_" + d]) for d in "XYZ"]
        return [int(r[what]), 1, 1]

    groups, cur = [], None
    for r in rows:
        name = short_name(r["Kernel_Name"])
        if name == "k_mean":
            if cur is not None:
                groups.append(cur)
            cur = []
            continue
        if cur is None:
            continue          # (fills and the like in front of the first separator)
        g, w = dims(r, "Grid_Size"), dims(r, "Workgroup_Size")
        wgs = 1
        for a, b in zip(g, w):
            assert a % b == 0, r
            wgs *= a // b
        cur.append([name, wgs, w[0] * w[1] * w[2], int(r.get("LDS_Block_Size", 0) or 0)])
    return groups


def merge(raw_path, trace_path, commit, out_path=OUT):
    raw = json.load(open(raw_path))
    assert not raw["stopped"], raw["stopped"]
    groups = read_trace(trace_path)
    assert len(groups) == len(raw["cases"]), (len(groups), len(raw["cases"]))
    for case, launches in zip(raw["cases"], groups):
        case["launches"] = launches
    doc = dict(commit=commit, device=raw["device"], cu_count=raw["cu_count"],
               note="recorded by tests/golden/make_scan_choices.py from the library of `commit`; launches: [kernel, workgroups, workgroup size, LDS as traced]",
               cases=raw["cases"])
    with open(out_path, "w") as f:
        f.write("{\n")
        for k in ("commit", "device", "cu_count", "note"):
            f.write(' "%s": %s,\n' % (k, json.dumps(doc[k])))
        f.write(' "cases": [\n')
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in doc["cases"]))
        f.write("\n ]\n}\n")
    print("wrote %s: %d cases" % (out_path, len(doc["cases"])))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "record":
        sys.exit(record(sys.argv[2]))
    elif len(sys.argv) >= 5 and sys.argv[1] == "merge":
        merge(*sys.argv[2:6])
    else:
        sys.exit(__doc__)
