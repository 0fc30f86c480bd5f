"""What a multi-scan call launches is decided by two pure host functions (csrc/scan_choice.h) that the library prints without a GPU:
mgr_lstm_scan_fwd_describe / mgr_lstm_scan_bwd_describe.

  * golden: tests/golden/scan_choices.json holds what the launchers of the commit BEFORE the decision became a value launched on the
    MI355X (tests/golden/make_scan_choices.py: return code, error text, workspace bytes, ledger entry, the traced launches).  At the
    fixture's CU count the described choice says the same: kernel, grid, workgroup size, ledger entry, bytes, refusal text, and the
    kernels of the jobs the cluster kernel does not take.  LDS bytes are not compared here (the profiler's figure is compared trace
    to trace, profiles/scan_choice_parity.txt).
  * invariants at CU counts nobody recorded (64, 104, 304), read off the launchers' text
  * a tensor beyond the 32-bit lane offsets of the K-split step
  * the header on its own, under AddressSanitizer + UBSan, in a stand-alone program (tests/scan_choice_walk.cpp)
"""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

from mgr_amd import _build, _capi

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = 0x10000      # a 16-byte aligned address nobody reads
LDT = 32
HDR = 4096          # kScanHdrBytes
FIX = json.load(open(os.path.join(HERE, "golden", "scan_choices.json")))
CASES = FIX["cases"]
CU = FIX["cu_count"]


def _jobs(case):
    if case["dir"] == "fwd":
        return [dict(Z=FAKE, Up=FAKE, Y=FAKE if j["Y"] else 0, ldy=j["H"] if j["Y"] else 0, gates=FAKE, cs=FAKE, B=j["B"], T=j["T"], H=j["H"],
                     reverse=i & 1, YT=FAKE if j["YT"] else 0, ytb=j["H"] * LDT if j["YT"] else 0, ldt=LDT if j["YT"] else 0,
                     yt_split=j["yt_split"]) for i, j in enumerate(case["jobs"])]
    return [dict(dY=FAKE, gates=FAKE, cs=FAKE, Up=FAKE, dZ=FAKE, lddy=j["H"], B=j["B"], T=j["T"], H=j["H"], reverse=i & 1,
                 dzmax=FAKE if j["dzmax"] else 0, dbsum=FAKE if j["dbsum"] else 0) for i, j in enumerate(case["jobs"])]


def _describe(case, cu=CU, ws_bytes=None):
    return _capi.describe_scan(case["dir"], cu, case["tune"], _jobs(case), case["form"], ws_bytes)


def _scan_launches(case):
    """The traced launches of the scan kernels proper (fills, copies, transposes and the row-maximum pass left out)."""
    return [l[:3] for l in case["launches"] if l[0].startswith("k_scan_")]


def _expected_launches(case, ch):
    """The same list from a choice: [name, workgroups, workgroup size]; the simple kernels by name only (their grid is their own)."""
    jobs, out = case["jobs"], []
    nbg = lambda j: (j["B"] + 15) // 16
    if case["dir"] == "fwd":
        if ch.kernel:
            out.append([_capi.SCAN_FWD_KERNELS[ch.kernel], ch.grid, ch.block])
        out += [["k_scan_fwd_simple", None, 256] for i in range(ch.njobs) if not ch.job[i].cluster]
        return out
    if ch.single_cu:
        return [["k_scan_bwd_cu16<%d>" % jobs[0]["H"], ch.grid, ch.block]]
    if ch.kernel:
        out.append([_capi.SCAN_BWD_KERNELS[ch.kernel], ch.grid, ch.block])
    joint = [j for i, j in enumerate(jobs) if ch.job[i].fallback == _capi.SCAN_FALLBACK_MFMA_JOINT]
    if joint:
        out.append(["k_scan_bwd_mfma<%d>" % joint[0]["H"], nbg(joint[0]) * len(joint), 512])
    for i, j in enumerate(jobs):
        if ch.job[i].fallback == _capi.SCAN_FALLBACK_MFMA:
            out.append(["k_scan_bwd_mfma<%d>" % j["H"], nbg(j), 512])
        elif ch.job[i].fallback == _capi.SCAN_FALLBACK_SIMPLE:
            out.append(["k_scan_bwd_simple", None, 256])
    return out


def _same_launches(traced, expected):
    if len(traced) != len(expected):
        return False
    for t, e in zip(traced, expected):
        if e[1] is None:      # a simple kernel: k_scan_fwd_simple<4, 1>, ...
            if re.sub(r"<.*>$", "", t[0]) != e[0] or t[2] != e[2]:
                return False
        elif t != e:
            return False
    return True


def test_fixture_covers_every_kernel_and_every_tune_value():
    assert len(CASES) >= 150 and CU == 256
    traced = set(l[0] for c in CASES for l in c["launches"])
    for name in _capi.SCAN_FWD_KERNELS[1:] + _capi.SCAN_BWD_KERNELS[1:]:
        assert name in traced, name
    assert any(n.startswith("k_scan_bwd_mfma") for n in traced) and any(n.startswith("k_scan_bwd_simple") for n in traced)
    assert any(n.startswith("k_scan_bwd_cu16") for n in traced) and any(n.startswith("k_scan_fwd_simple") for n in traced)
    described = {"fwd": set(), "bwd": set()}
    for c in CASES:
        if c["rc"] == 0:
            described[c["dir"]].add(_describe(c, ws_bytes=c.get("ws_bytes")).kernel)
    assert described["fwd"] == set(range(7)) and described["bwd"] == set(range(11))
    # every tune key the two decisions read, at every value they tell apart (0 is every other case)
    seen = {(c["dir"], int(k), v) for c in CASES for k, v in c["tune"].items()}
    T = _capi
    for key, vals in ((T.TUNE_SCAN_PATH, (1, 2, 3, 4)), (T.TUNE_SCAN_FORM, (3,)), (T.TUNE_SCAN_LDS_IMAGE, (1,)), (T.TUNE_SCAN_F32_MFMA, (1,)),
                      (T.TUNE_SCAN_NO_XCD_LOCAL, (1,))):
        assert all(("fwd", key, v) in seen for v in vals), key
    for key, vals in ((T.TUNE_SCAN_PATH, (1, 2, 3)), (T.TUNE_BPTT_FORM, (1, 2)), (T.TUNE_BPTT_SPLIT_ROLE, (1, 2)), (T.TUNE_BPTT_SINGLE_CU, (1,)),
                      (T.TUNE_SCAN_F32_MFMA, (1,)), (T.TUNE_SCAN_NO_XCD_LOCAL, (1,))):
        assert all(("bwd", key, v) in seen for v in vals), key
    assert {c["form"] for c in CASES if c["dir"] == "fwd"} == {0, 1, 3, 4} and {c["form"] for c in CASES if c["dir"] == "bwd"} == set(range(7))
    assert any(c.get("ws") == "degrade" for c in CASES)


def test_described_choice_is_what_the_recorded_launchers_did():
    bad = []
    for n, c in enumerate(CASES):
        fwd = c["dir"] == "fwd"
        if fwd:     # the workspace query: planned with a workspace that is large enough
            q = _describe(c)
            if q.need != c["need"]:
                bad.append((n, "need", q.need, c["need"]))
            hdr_images = _capi.load_library().mgr_lstm_scan_multi_ws_bytes(len(c["jobs"]), _capi.make_scan_jobs(
                [dict(j, Y=FAKE, ldy=j["H"]) for j in _jobs(c)]))
            assert q.base_need == hdr_images and q.need <= c["upper"]
        try:
            ch = _describe(c, ws_bytes=c["ws_bytes"] if fwd else None)
        except _capi.MgrError as e:
            if c["rc"] == 0 or c["err"] not in str(e):
                bad.append((n, "refusal", str(e), c["err"]))
            if [l for l in c["launches"] if not l[0].startswith("__amd_rocclr_")]:      # (the recorder's own status read-back is a copy)
                bad.append((n, "a refused call launched", c["launches"]))
            continue
        if c["rc"] != 0:
            bad.append((n, "not refused", c["err"]))
            continue
        if not fwd and ch.need != c["need"]:
            bad.append((n, "need", ch.need, c["need"]))
        if not _same_launches(_scan_launches(c), _expected_launches(c, ch)):
            bad.append((n, "launches", _scan_launches(c), _expected_launches(c, ch)))
        if ch.ledger != c["ledger"] or c["persist"][0] != ch.ledger:
            bad.append((n, "ledger", ch.ledger, c["ledger"], c["persist"]))
        if fwd and c.get("ws") == "degrade" and not ch.degraded:
            bad.append((n, "not degraded"))
        # transposes behind the scans: one per job with a YT that the kernel does not write itself
        if fwd:
            behind = sum(1 for l in c["launches"] if l[0] in ("k_transpose_bt", "k_transpose_split", "k_transpose_bt_split"))
            want = sum(1 for i, j in enumerate(c["jobs"]) if j["YT"] and not ch.job[i].yt_in_kernel)
            if behind != want:
                bad.append((n, "transposes", behind, want))
    assert not bad, bad[:8]


def _check_invariants(c, ch, cu):
    J = [ch.job[i] for i in range(ch.njobs)]
    cl = [j for j in J if j.cluster]
    assert bool(ch.kernel) == bool(cl) and (ch.kernel or not ch.ledger)
    if ch.exchange:      # every spinning workgroup is co-resident
        assert ch.live <= ch.per_cu * cu, (c, cu)
    if ch.fused:
        assert ch.xcd_local and ch.per_cu == 1 and ch.waves == 8
    if ch.xcd_local:
        assert ch.grid * 4 <= HDR - 256
    assert ch.live <= ch.grid and (not ch.kernel or ch.block == 64 * ch.waves)
    for j in cl:
        assert j.cls_begin % 8 == 0 and 0 <= j.cls_cluster0 and j.cls_cluster0 + j.nbg <= j.cls_nclusters
        per = (j.cls_nclusters + 7) // 8 * 8 if ch.xcd_local else j.cls_nclusters
        assert j.cls_begin + j.members * per <= ch.grid and (ch.xcd_local or j.cls_rot == 0)
        assert j.members == ((j.G + 1) // 2 if ch.fused else j.G)
    if c["dir"] == "fwd":
        def images(j):     # (tests/test_cpu_scan_no_rows.py: the independent statement of the sizes)
            return ((j["B"] + 15) // 16 * 2 * ((j["H"] // 4 + 7) // 8) * 512 * 4 + 255) // 256 * 256

        def scratch(j):
            return (j["B"] * j["T"] * j["H"] * 4 + 255) // 256 * 256

        rows = [i for i, j in enumerate(c["jobs"]) if not j["Y"] and not J[i].yt_in_kernel]
        assert [i for i in range(ch.njobs) if J[i].rows_in_scratch] == rows
        assert ch.base_need == HDR + sum(images(j) for j in c["jobs"])
        assert ch.need == ch.base_need + sum(scratch(c["jobs"][i]) for i in rows)
        at = ch.base_need
        for i in rows:
            assert J[i].rows_off == at
            at += scratch(c["jobs"][i])
        assert ch.zero_bytes == (HDR + sum(images(j) for i, j in enumerate(c["jobs"]) if J[i].cluster) if ch.kernel else 0)
        assert all(not J[i].yt_in_kernel or (J[i].cluster and c["jobs"][i]["YT"]) for i in range(ch.njobs))
    else:
        assert ch.need == ch.base_need and (not ch.kernel or ch.zero_bytes == ch.need)
        assert not ch.split or (ch.grid <= cu and not ch.fused)


@pytest.mark.parametrize("cu", [64, 104, 256, 304])
def test_invariants_hold_at_cu_counts_nobody_recorded(cu):
    for c in CASES:
        _check_invariants(c, _describe(c, cu), cu)


def test_a_tensor_beyond_32_bit_lane_offsets_takes_the_lds_image_step():
    """B T 4H 4 >= 2^32 cannot be recorded on the GPU in seconds.  The launcher's rule: the K-split step addresses Z with 32-bit byte
    offsets per lane, a launch with a larger tensor takes the LDS-image step - which writes no YT."""
    H, B = 500, 64
    T = (1 << 32) // (B * 4 * H * 4) + 1
    ldt = (T + 31) // 32 * 32
    job = dict(Z=FAKE, Up=FAKE, Y=FAKE, ldy=H, B=B, T=T, H=H, YT=FAKE, ytb=H * ldt, ldt=ldt)
    big = _capi.describe_scan("fwd", CU, {}, [job, job], _capi.SCAN_FORM_FUSED_ANY)
    assert B * T * 4 * H * 4 >= 1 << 32 and not big.ksplit and big.kernel == _capi.SCAN_FWD_KERNELS.index("k_scan_cluster")
    assert not big.xcd_local and not big.fused and not any(big.job[i].yt_in_kernel for i in range(2))
    near = _capi.describe_scan("fwd", CU, {}, [dict(job, T=T - 1)] * 2, _capi.SCAN_FORM_PLAIN)
    assert near.ksplit and near.kernel == _capi.SCAN_FWD_KERNELS.index("k_scan_cluster_k16") and near.job[0].yt_in_kernel
    # the BPTT's saved state: B T H 16 bytes
    bj = dict(dY=FAKE, gates=FAKE, cs=FAKE, Up=FAKE, dZ=FAKE, lddy=H, B=B, T=T, H=H, reverse=0)
    assert not _capi.describe_scan("bwd", CU, {}, [bj, bj]).kernel and _capi.describe_scan("bwd", CU, {}, [dict(bj, T=T - 1)] * 2).kernel


def test_describe_checks_the_job_list_like_the_calls():
    job = dict(Z=FAKE, Up=FAKE, Y=0, YT=0, B=17, T=9, H=100)
    with pytest.raises(_capi.MgrError, match="neither Y nor YT"):
        _capi.describe_scan("fwd", CU, {}, [job])
    with pytest.raises(_capi.MgrError, match="bad shape"):
        _capi.describe_scan("fwd", CU, {}, [dict(job, Y=FAKE, ldy=99)])
    with pytest.raises(_capi.MgrError, match="retired"):
        _capi.describe_scan("fwd", CU, {}, [dict(job, Y=FAKE, ldy=100)], form=2)
    with pytest.raises(_capi.MgrError, match="unknown BPTT form"):
        _capi.describe_scan("bwd", CU, {}, [dict(dY=FAKE, gates=FAKE, cs=FAKE, Up=FAKE, dZ=FAKE, lddy=100, B=17, T=9, H=100, reverse=0)], form=7)
    out = _capi.ScanChoice()      # (struct_size not set)
    arr = _capi.make_scan_jobs([dict(job, Y=FAKE, ldy=100)])
    assert _capi.load_library().mgr_lstm_scan_fwd_describe(CU, None, 0, 1, arr, None, 0, C.byref(out)) != 0


def _cxx():
    for cand in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("clang++"),
                 os.path.join(os.path.dirname(os.path.realpath(_build._hipcc())), "..", "llvm", "bin", "clang++")):
        if cand and (os.path.exists(cand) or shutil.which(cand)):
            return cand
    raise RuntimeError("no host C++ compiler")


def test_header_alone_under_asan_and_ubsan_says_what_the_library_says(tmp_path):
    """The stand-alone program includes csrc/scan_choice.h and nothing of HIP: built with -fsanitize=address,undefined and run on the
    CPU over every fixture shape at four CU counts, plus eight-job lists (the largest plan search: 4^8 combinations)."""
    exe = str(tmp_path / "scan_choice_walk")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(HERE, "scan_choice_walk.cpp")], check=True)
    eight = [dict(dir="fwd", form=1, tune={}, jobs=[dict(H=h, B=17, T=7, Y=1, YT=1, yt_split=0) for h in (100, 100, 128, 128, 64, 64, 32, 30)]),
             dict(dir="fwd", form=4, tune={}, jobs=[dict(H=100, B=b, T=7, Y=0, YT=1, yt_split=0) for b in (16, 17, 33, 64, 1, 15, 48, 100)]),
             dict(dir="bwd", form=4, tune={}, jobs=[dict(H=h, B=17, T=7, dzmax=0, dbsum=0) for h in (100, 100, 128, 128, 64, 64, 32, 30)])]
    lines, want = [], []
    for cu in (64, 104, 256, 304):
        for c in CASES + eight:
            fwd = c["dir"] == "fwd"
            ws = c.get("ws_bytes", -1) if fwd else None
            try:
                ch = _describe(c, cu, ws_bytes=None if ws in (None, -1) else ws)
            except _capi.MgrError:
                continue      # (a refusal is the library's, behind the decision)
            pairs = " ".join("%s %d" % kv for kv in c["tune"].items())
            head = "%s %d %d %s%d %s %d" % (c["dir"], cu, c["form"], "%d " % ws if fwd else "", len(c["tune"]), pairs, len(c["jobs"]))
            lines.append(head + " " + " ".join(("%d %d %d %d %d" % (j["H"], j["B"], j["T"], j["Y"], j["YT"])) if fwd else
                                               ("%d %d %d" % (j["H"], j["B"], j["T"])) for j in c["jobs"]))
            want.append(" ".join(str(v) for v in [ch.kernel, ch.grid, ch.block, ch.lds_bytes, ch.waves, ch.per_cu, ch.live, ch.xcd_local, ch.fused,
                                                  ch.ledger, ch.need] + [x for i in range(ch.njobs) for x in
                                                                        (ch.job[i].cluster, ch.job[i].fallback, ch.job[i].cls_begin)]))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    got = r.stdout.strip().split("\n")
    assert len(got) == len(want)
    assert [(a, b) for a, b in zip(got, want) if a != b][:5] == []
