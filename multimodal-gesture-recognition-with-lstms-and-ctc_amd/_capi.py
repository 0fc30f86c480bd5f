"""ctypes binding of include/mgr.h (libmgr.so).  No CPU fallback: a missing library raises."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmgr.so")

c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)
vp = C.c_void_p
sz = C.c_size_t
u64 = C.c_uint64
i32 = C.c_int

# name -> (restype, argtypes).  Must list every symbol include/mgr.h declares (tests check this).
SIGNATURES = {
    "mgr_version": (i32, []),
    "mgr_last_error": (C.c_char_p, []),
    "mgr_device_count": (i32, [C.POINTER(i32)]),
    "mgr_ctx_create": (i32, [i32, C.POINTER(vp)]),
    "mgr_ctx_destroy": (i32, [vp]),
    "mgr_device_info": (i32, [vp, C.POINTER(i32), C.POINTER(sz), C.c_char_p, i32]),
    "mgr_alloc": (i32, [vp, sz, C.POINTER(vp)]),
    "mgr_free": (i32, [vp, vp]),
    "mgr_memset": (i32, [vp, vp, i32, sz]),
    "mgr_h2d": (i32, [vp, vp, vp, sz]),
    "mgr_d2h": (i32, [vp, vp, vp, sz]),
    "mgr_d2d": (i32, [vp, vp, vp, sz]),
    "mgr_d2h_async": (i32, [vp, vp, vp, sz]),
    "mgr_event_sync": (i32, [vp, i32]),
    "mgr_sync": (i32, [vp]),
    "mgr_stream_set": (i32, [vp, i32]),
    "mgr_stream_wait": (i32, [vp, i32, i32]),
    "mgr_stream_set_priority": (i32, [vp, i32, i32]),
    "mgr_event_record": (i32, [vp, i32]),
    "mgr_stream_wait_event": (i32, [vp, i32, i32]),
    "mgr_event_elapsed_ms": (i32, [vp, i32, i32, C.POINTER(C.c_float)]),
    "mgr_prof_enable": (i32, [vp, i32]),
    "mgr_prof_get": (i32, [vp, i32, C.POINTER(i32), C.POINTER(C.c_float)]),
    "mgr_prof_reset": (i32, [vp]),
    "mgr_add_gaussian_noise": (i32, [vp, vp, vp, sz, C.c_float, u64]),
    "mgr_dropout_mask": (i32, [vp, vp, sz, C.c_float, u64]),
    "mgr_augment_plan_len": (i32, [i32, i32, i32, i32]),
    "mgr_augment_plan": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, vp, C.c_uint32, u64, vp]),
    "mgr_augment_apply": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, C.c_float, C.c_float, u64]),
    "mgr_seq_zero_tail": (i32, [vp, i32, vp, vp]),
    "mgr_lstm_pack": (i32, [vp, vp, vp, i32, i32, i32]),
    "mgr_transpose": (i32, [vp, vp, vp, i32, i32]),
    "mgr_lstm_input_proj": (i32, [vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32]),
    "mgr_lstm_input_proj_dropout_ws_bytes": (sz, [i32, i32, i32]),
    "mgr_lstm_input_proj_dropout": (i32, [vp, vp, i32, vp, C.c_float, vp, vp, vp, i32, i32, i32, i32, vp, sz]),
    "mgr_lstm_input_proj_dropout_wants_transposed": (i32, [vp, C.c_float, i32]),
    "mgr_lstm_input_proj_dropout_t": (i32, [vp, vp, i32, vp, C.c_float, vp, vp, vp, i32, i32, i32, i32, vp, sz, C.c_float]),
    "mgr_transpose_bt": (i32, [vp, vp, i32, vp, i32, i32, i32, i32]),
    "mgr_lstm_input_proj_dropout_ts_ws_bytes": (sz, [i32, i32, i32]),
    "mgr_lstm_input_proj_dropout_ts": (i32, [vp, vp, i32, vp, C.c_float, vp, vp, vp, i32, i32, i32, i32, vp, sz]),
    "mgr_transpose_bt_split": (i32, [vp, vp, i32, vp, i32, i32, i32, i32]),
    "mgr_transpose_bt_split_shift": (i32, [vp, vp, i32, vp, i32, i32, i32, i32, i32]),
    "mgr_weight_planes_cache": (i32, [vp, vp, i32]),
    "mgr_lstm_input_proj_pair": (i32, [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32]),
    "mgr_lstm_scan_ws_bytes": (sz, [i32, i32, i32]),
    "mgr_lstm_scan_fwd": (i32, [vp, vp, vp, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, vp, sz]),
    "mgr_lstm_scan_multi_ws_bytes": (sz, [i32, vp]),
    "mgr_lstm_scan_fwd_multi": (i32, [vp, i32, vp, vp, sz]),
    "mgr_lstm_scan_fwd_multi_ex": (i32, [vp, i32, vp, vp, sz, vp]),
    "mgr_lstm_scan_fwd_multi_ws_bytes": (sz, [vp, i32, vp, vp]),
    "mgr_abi_struct_sizes": (i32, [vp]),
    "mgr_tune": (i32, [vp, i32, i32]),
    "mgr_tune_get": (i32, [vp, i32, C.POINTER(i32)]),
    "mgr_probe_xcc": (i32, [vp, i32, i32, i32, vp]),
    "mgr_stream_delay": (i32, [vp, i32]),
    "mgr_probe_guest": (i32, [vp, i32, i32, i32, i32, vp]),
    "mgr_host_alloc": (i32, [vp, sz, C.POINTER(vp)]),
    "mgr_host_free": (i32, [vp, vp]),
    "mgr_h2d_async": (i32, [vp, vp, vp, sz]),
    "mgr_scan_status": (i32, [vp, vp]),
    "mgr_scan_status_clear": (i32, [vp]),
    "mgr_scan_status_ex": (i32, [vp, vp]),
    "mgr_scan_status_bind": (i32, [vp, vp]),
    "mgr_scan_status_inject": (i32, [vp, C.c_uint]),
    "mgr_update_gate_eval": (i32, [vp, C.c_uint, vp]),
    "mgr_update_gate_set": (i32, [vp, vp]),
    "mgr_stream_wait_next_resident": (i32, [vp, i32]),
    "mgr_stream_wait_resident": (i32, [vp, C.c_uint, i32]),
    "mgr_stream_wait_resident_word": (i32, [vp, vp, i32]),
    "mgr_resident_wait_stats": (i32, [vp, vp]),
    "mgr_persist_stats": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
    "mgr_skeletal_features": (i32, [vp, vp, sz, vp]),
    "mgr_skeletal_activity": (i32, [vp, vp, vp, i32, C.c_longlong, i32, vp, vp, vp]),
    "mgr_mfcc_ws_bytes": (sz, [i32, C.c_longlong, i32, i32, i32, i32]),
    "mgr_mfcc": (i32, [vp, vp, vp, i32, C.c_longlong, i32, i32, i32, i32, i32, i32, C.c_double, i32, i32, i32, vp, vp, vp, vp, vp,
                       sz]),
    "mgr_lstm_scan_bwd_multi_ws_bytes": (sz, [i32, vp]),
    "mgr_lstm_scan_bwd_multi": (i32, [vp, i32, vp, vp, sz]),
    "mgr_lstm_scan_bwd_multi_ex": (i32, [vp, i32, vp, vp, sz, vp]),
    "mgr_lstm_scan_bwd": (i32, [vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp, sz]),
    "mgr_lstm_scan_fwd_describe": (i32, [i32, vp, i32, i32, vp, vp, sz, vp]),
    "mgr_lstm_scan_bwd_describe": (i32, [i32, vp, i32, i32, vp, vp, vp]),
    "mgr_lstm_param_grads_ws_bytes": (sz, [i32, i32, i32, i32]),
    "mgr_lstm_param_grads": (i32, [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, sz]),
    "mgr_lstm_param_grads_dropout_ws_bytes": (sz, [i32, i32, i32, i32]),
    "mgr_lstm_param_grads_dropout": (i32, [vp, vp, i32, vp, C.c_float, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, sz]),
    "mgr_lstm_param_grads_dropout_wants_transposed": (i32, [vp, C.c_float, i32]),
    "mgr_lstm_param_grads_dropout_t_ws_bytes": (sz, [i32, i32, i32, i32, i32]),
    "mgr_lstm_param_grads_dropout_t": (i32, [vp, vp, i32, vp, C.c_float, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, C.c_float]),
    "mgr_lstm_param_grads_dropout_ts_ws_bytes": (sz, [i32, i32, i32, i32, i32]),
    "mgr_lstm_param_grads_dropout_ts": (i32, [vp, vp, i32, vp, C.c_float, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp, vp, vp, vp]),
    "mgr_lstm_input_grad": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32]),
    "mgr_dense_softmax_fwd": (i32, [vp, vp, i32, vp, C.c_float, u64, vp, vp, vp, i32, i32, i32, i32]),
    "mgr_dense_bwd_ws_bytes": (sz, [i32, i32, i32, i32]),
    "mgr_dense_bwd": (i32, [vp, vp, i32, vp, C.c_float, u64, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, sz]),
    "mgr_head_ws_bytes": (sz, [i32, i32, i32, i32, i32]),
    "mgr_head_fwd_bwd": (i32, [vp, vp, i32, vp, C.c_float, u64, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, C.c_float, C.c_float,
                               vp, vp, vp, vp, vp, vp, vp, i32, vp, sz]),
    "mgr_ctc_ws_bytes": (sz, [i32, i32, i32, i32]),
    "mgr_ctc_loss_grad": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, C.c_float, C.c_float, vp, vp, vp, sz]),
    "mgr_ctc_entropy_grad": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, vp, vp, vp, vp, sz]),
    "mgr_adam_step": (i32, [vp, vp, vp, vp, vp, sz, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    "mgr_maxnorm_cols": (i32, [vp, vp, i32, i32, C.c_float, C.c_float]),
    "mgr_add2d": (i32, [vp, vp, i32, vp, i32, vp, i32, sz, i32]),
    "mgr_mean": (i32, [vp, vp, i32, vp]),
    "mgr_comm_unique_id": (i32, [C.c_char_p]),
    "mgr_comm_init_rank": (i32, [vp, i32, i32, C.c_char_p, C.POINTER(vp)]),
    "mgr_allreduce_sum": (i32, [vp, vp, sz]),
    "mgr_allreduce_max": (i32, [vp, vp, sz]),
    "mgr_comm_destroy": (i32, [vp]),
    "mgr_comm_count": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
    "mgr_frame_argmax": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
    "mgr_ctc_beam_ws_bytes": (sz, [i32, i32, i32, i32]),
    "mgr_ctc_beam_search": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, C.c_float, i32, vp, vp, vp, vp, sz]),
    "mgr_ctc_beam_lm_ws_bytes": (sz, [i32, i32, i32, i32, i32]),
    "mgr_ctc_beam_search_lm": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, C.c_float, vp, vp, i32, vp, vp, vp, vp, vp, sz]),
    "mgr_ctc_align_ws_bytes": (sz, [i32, i32, i32, i32]),
    "mgr_ctc_align": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, C.c_float, vp, vp, vp, vp, vp, sz]),
    "mgr_greedy_segments": (i32, [vp, vp, i32, i32, i32, i32, C.c_float, i32, vp, vp, vp, vp]),
    "mgr_ctc_occupancy": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp, sz]),
    "mgr_segment_overlap": (i32, [vp, vp, vp, i32, vp, vp, i32, vp, i32, i32, u64, vp, vp, vp, vp]),
    "mgr_ctc_lexicon_ws_bytes": (sz, [i32, i32, i32, i32, vp]),
    "mgr_ctc_lexicon_decode": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, C.c_float, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp,
                                     sz]),
    "mgr_ctc_rescore_ws_bytes": (sz, [i32, i32, i32, i32, vp]),
    "mgr_ctc_rescore": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, C.c_float, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, sz]),
    "mgr_ctc_joint_ws_bytes": (sz, [i32, i32, vp, i32, i32, i32, i32]),
    "mgr_ctc_joint_decode": (i32, [vp, i32, i32, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz]),
    "mgr_ctc_risk_ws_bytes": (sz, [i32, i32, i32, i32, i32, i32, vp]),
    "mgr_ctc_risk_grad": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, C.c_float, vp, vp, i32, vp, vp, i32, i32, i32, vp, C.c_float, C.c_float,
                                C.c_float, i32, vp, vp, vp, vp, vp, sz]),
    "mgr_ctc_sample_paths": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, C.c_float, u64, i32, vp, vp, vp, vp, vp]),
    "mgr_edit_distance_ws_bytes": (sz, [i32, i32, i32, i32]),
    "mgr_edit_distance": (i32, [vp, vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, u64, vp, vp, vp, vp, vp, vp, sz]),
    "mgr_conv_pool_fwd": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp]),
    "mgr_conv_pool_bwd_data": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "mgr_conv_pool_bwd_weights_ws_bytes": (sz, [i32, i32, i32, i32, i32, i32]),
    "mgr_conv_pool_bwd_weights": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, sz]),
    "mgr_roi_crop": (i32, [vp, vp, i32, i32, i32, vp, i32, vp]),
    "mgr_lstm_scan_window": (i32, [vp, i32, vp, i32, i32, vp, vp, vp, vp]),
    "mgr_live_greedy": (i32, [vp, vp, i32, i32, i32, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp]),
}

SCAN_GAVE_UP, SCAN_NONFINITE = 1, 8   # enum in include/mgr.h (mgr_scan_status)

(K_GEMM_NN, K_GEMM_TN, K_GEMM_NT, K_SCAN_FWD, K_SCAN_BWD, K_DENSE_FWD, K_DENSE_BWD, K_CTC, K_ADAM, K_MISC, K_ALLREDUCE, K_SCAN_FWD_NARROW) = range(12)
KERNEL_FAMILIES = ["gemm_nn", "gemm_tn", "gemm_nt", "scan_fwd", "scan_bwd", "dense_fwd", "dense_bwd", "ctc", "adam", "misc", "allreduce",
                   "scan_fwd_narrow"]



class ScanJob(C.Structure):
    """struct mgr_scan_job"""
    _fields_ = [("Z", vp), ("Up", vp), ("Y", vp), ("R", vp), ("gates", vp), ("cs", vp),
                ("ldy", i32), ("ldr", i32), ("B", i32), ("T", i32), ("H", i32), ("reverse", i32),
                ("YT", vp), ("ytb", C.c_longlong), ("ldt", i32), ("yt_split", i32)]


class ScanBwdJob(C.Structure):
    """struct mgr_scan_bwd_job"""
    _fields_ = [("dY", vp), ("gates", vp), ("cs", vp), ("Up", vp), ("dZ", vp),
                ("lddy", i32), ("B", i32), ("T", i32), ("H", i32), ("reverse", i32), ("dzmax", vp), ("dbsum", vp)]


class ScanLaunchOpts(C.Structure):
    """struct mgr_scan_launch_opts"""
    _fields_ = [("struct_size", C.c_uint), ("form", i32), ("seq_out", vp)]


class ScanChoiceJob(C.Structure):
    """struct mgr_scan_choice_job"""
    _fields_ = [(n, i32) for n in ("cluster", "fallback", "nw", "tpw", "G", "nbg", "members", "cls_begin", "cls_nclusters", "cls_cluster0",
                                   "cls_rot", "yt_in_kernel", "rows_in_scratch", "reserved")] + [("xbuf_off", u64), ("rows_off", u64)]


class ScanChoice(C.Structure):
    """struct mgr_scan_choice: what a multi-scan call launches (csrc/scan_choice.h)"""
    _fields_ = ([("struct_size", C.c_uint)] +
                [(n, i32) for n in ("njobs", "kernel", "grid", "block", "lds_bytes", "waves", "per_cu", "live", "xcd_local", "fused", "exchange",
                                    "ksplit", "split16", "split", "single_cu", "ledger", "degraded")] +
                [("base_need", u64), ("need", u64), ("zero_bytes", u64), ("job", ScanChoiceJob * 8)])

    def to_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("struct_size", "job")}
        d["job"] = [{n: getattr(self.job[i], n) for n, _ in ScanChoiceJob._fields_ if n != "reserved"} for i in range(self.njobs)]
        return d


# mgr_scan_choice.kernel -> kernel name (MGR_SCAN_FWD_* / MGR_SCAN_BWD_* of include/mgr.h); job[i].fallback (MGR_SCAN_FALLBACK_*)
SCAN_FWD_KERNELS = ["", "k_scan_cluster", "k_scan_cluster_ks", "k_scan_cluster_ks_s", "k_scan_cluster_k16", "k_scan_cluster_k16_s",
                    "k_scan_cluster_k16fs"]
SCAN_BWD_KERNELS = ["", "k_scan_cluster_bwd", "k_scan_cluster_bwd_s", "k_scan_cluster_bwd_split", "k_scan_cluster_bwd16", "k_scan_cluster_bwd16_s",
                    "k_scan_cluster_bwd16_sl", "k_scan_cluster_bwd16_sd", "k_scan_cluster_bwd16_split", "k_scan_cluster_bwd16_f",
                    "k_scan_cluster_bwd16_fd"]
SCAN_FALLBACK_NONE, SCAN_FALLBACK_SIMPLE, SCAN_FALLBACK_MFMA, SCAN_FALLBACK_MFMA_JOINT, SCAN_FALLBACK_CU16 = range(5)


def describe_scan(direction, cu_count, tune, jobs, form=0, ws_bytes=None):
    """The decision of a multi-scan call as a ScanChoice - no context, no GPU.  direction "fwd" / "bwd"; tune: {key: value}; jobs: what
    make_scan_jobs / make_scan_bwd_jobs take (pointers may be any aligned non-zero numbers: they are never followed); ws_bytes (forward):
    the workspace the call would get, None = as much as it takes.  Raises MgrError with the call's own refusal text.
        print(_capi.describe_scan("fwd", 256, {}, [dict(Z=4096, Up=4096, Y=4096, ldy=500, B=64, T=8, H=500)] * 2).to_dict())"""
    lib = load_library()
    t = (i32 * TUNE_COUNT)()
    for k, v in tune.items():
        t[int(k)] = int(v)
    out = ScanChoice()
    out.struct_size = C.sizeof(ScanChoice)
    opts = make_launch_opts(form, 0)
    if direction == "fwd":
        arr = make_scan_jobs(jobs)
        rc = lib.mgr_lstm_scan_fwd_describe(cu_count, t, TUNE_COUNT, len(jobs), arr, C.byref(opts), sz(-1).value if ws_bytes is None else ws_bytes,
                                            C.byref(out))
    else:
        arr = make_scan_bwd_jobs(jobs)
        rc = lib.mgr_lstm_scan_bwd_describe(cu_count, t, TUNE_COUNT, len(jobs), arr, C.byref(opts), C.byref(out))
    check(rc, lib)
    return out


class LiveJob(C.Structure):
    """struct mgr_live_job (K20)"""
    _fields_ = [("Z", vp), ("Up", vp), ("Y", vp), ("R", vp), ("state", vp), ("ldy", i32), ("ldr", i32), ("H", i32), ("reverse", i32)]


LIVE_MAX_H, LIVE_MAX_JOBS, LIVE_STATE_WORDS = 1024, 8, 8     # MGR_LIVE_* of include/mgr.h


def make_live_jobs(jobs):
    """jobs: list of dicts with the mgr_live_job fields (DeviceArray or int pointers; R / state may be absent)."""
    arr = (LiveJob * max(len(jobs), 1))()
    for a, j in zip(arr, jobs):
        for k in ("Z", "Up", "Y", "R", "state"):
            v = j.get(k, 0)
            setattr(a, k, v.ptr if isinstance(v, DeviceArray) else (v or 0))
        for k in ("ldy", "ldr", "H", "reverse"):
            setattr(a, k, int(j.get(k, 0)))
    return arr


class SeqFillJob(C.Structure):
    """struct mgr_seq_fill_job (K1c)"""
    _fields_ = [("buf", vp), ("row", i32), ("ld", i32), ("B", i32), ("T", i32)]


def make_seq_fill_jobs(jobs):
    """jobs: list of (buf, row, ld, B, T) - buf a DeviceArray or a device address."""
    arr = (SeqFillJob * max(len(jobs), 1))()
    for a, (buf, row, ld, B, T) in zip(arr, jobs):
        a.buf = buf.ptr if isinstance(buf, DeviceArray) else (buf or None)
        a.row, a.ld, a.B, a.T = int(row), int(ld), int(B), int(T)
    return arr


class JointStream(C.Structure):
    """struct mgr_joint_stream (K19): struct_size is checked by mgr_ctc_joint_decode; phrase_off / phrase_words are HOST pointers or 0"""
    _fields_ = [("struct_size", C.c_uint), ("T", i32), ("C", i32), ("skip", i32), ("blank", i32), ("eps", C.c_float), ("weight", C.c_double),
                ("P", vp), ("input_len", vp), ("phrase_off", vp), ("phrase_words", vp)]


JOINT_MAX_STREAMS, JOINT_MAX_PHRASE_WORDS = 4, 8       # MGR_JOINT_MAX_* of include/mgr.h
AUGMENT_MAX_SEGMENTS, AUGMENT_MAX_STREAMS, AUGMENT_MAX_MASKS, AUGMENT_MAX_T, AUGMENT_STREAM_COLS = 16, 8, 8, 32767, 5   # MGR_AUGMENT_*


def make_joint_streams(streams):
    """streams: list of dicts with the mgr_joint_stream fields - P / input_len DeviceArrays (or device addresses), phrase_off /
    phrase_words host int32 arrays or None (the caller keeps them alive for the call)."""
    arr = (JointStream * len(streams))()
    for a, s in zip(arr, streams):
        a.struct_size = C.sizeof(JointStream)
        for k in ("T", "C", "skip", "blank"):
            setattr(a, k, int(s[k]))
        a.eps, a.weight = float(s["eps"]), float(s["weight"])
        for k in ("P", "input_len"):
            v = s[k]
            setattr(a, k, v.ptr if isinstance(v, DeviceArray) else (v or None))
        for k in ("phrase_off", "phrase_words"):
            v = s.get(k)
            setattr(a, k, None if v is None else v.ctypes.data)
    return arr


# enums of include/mgr.h (mgr_scan_launch_opts.form)
SCAN_FORM_AUTO, SCAN_FORM_PLAIN, SCAN_FORM_FUSED, SCAN_FORM_FUSED_ANY = 0, 1, 3, 4
BPTT_FORM_AUTO, BPTT_FORM_TRIMMED, BPTT_FORM_YIELDING, BPTT_FORM_DIRECT, BPTT_FORM_FUSED, BPTT_FORM_FUSED_DIRECT, BPTT_FORM_SINGLE_CU = range(7)
SEQ_NONE = 0xFFFFFFFF
ABI_REVISION = 7
# tune keys of include/mgr.h (mgr_tune / mgr_tune_get)
TUNE_SCAN_PATH = 0
TUNE_SCAN_SYNC_CHECK = 1
TUNE_SCAN_PRINT_PLAN = 2
TUNE_SCAN_NO_XCD_LOCAL = 3
TUNE_SCAN_FORM = 4
TUNE_SCAN_LDS_IMAGE = 7
TUNE_BPTT_SPLIT_ROLE = 8
TUNE_PROJ_DENSE = 9
TUNE_PROJ_DENSE16_MASKED = 10
TUNE_PROJ_WIDE_TILES = 11
TUNE_PROJ_TS_TILE = 12
TUNE_DENSE_VALU = 13
TUNE_SCAN_F32_MFMA = 14
TUNE_GEMM_F32 = 15
TUNE_BPTT_FORM = 16
TUNE_CTC_ONE_SAMPLE = 18
TUNE_BPTT_SINGLE_CU = 19
TUNE_CTC_CHAIN_LDS_KIB = 20
TUNE_CTC_FRAME_LDS_KIB = 21
TUNE_COUNT = 24


def make_launch_opts(form=0, seq_out=0):
    """seq_out: address of a host word (e.g. element of a Device.pinned() array: arr.ctypes.data + 4 * i) or 0."""
    o = ScanLaunchOpts()
    o.struct_size = C.sizeof(ScanLaunchOpts)
    o.form = int(form)
    o.seq_out = int(seq_out) or None
    return o


def make_scan_bwd_jobs(jobs):
    arr = (ScanBwdJob * len(jobs))()
    for a, j in zip(arr, jobs):
        for k in ("dY", "gates", "cs", "Up", "dZ", "dzmax", "dbsum"):
            v = j.get(k, 0)
            setattr(a, k, v.ptr if isinstance(v, DeviceArray) else (v or 0))
        for k in ("lddy", "B", "T", "H", "reverse"):
            setattr(a, k, int(j[k]))
    return arr


def make_scan_jobs(jobs):
    """jobs: list of dicts with the mgr_scan_job fields (DeviceArray or int pointers)."""
    arr = (ScanJob * len(jobs))()
    for a, j in zip(arr, jobs):
        for k in ("Z", "Up", "Y", "R", "gates", "cs", "YT"):
            v = j.get(k, 0)
            setattr(a, k, v.ptr if isinstance(v, DeviceArray) else (v or 0))
        for k in ("ldy", "ldr", "B", "T", "H", "reverse", "ytb", "ldt", "yt_split"):
            setattr(a, k, int(j.get(k, 0)))
    return arr


_lib = None


class MgrError(RuntimeError):
    pass


def load_library(build_if_missing=True):
    """dlopen libmgr.so (building it with hipcc first if absent).  Raises if neither is possible."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH) and build_if_missing:
        from . import _build
        _build.build(verbose=False)
    if not os.path.exists(LIB_PATH):
        raise MgrError("libmgr.so is missing (%s) and could not be built; there is no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    # ABI guard: this binding fills the job structs field by field - the library must have been built from the same header
    sizes = (C.c_uint * 4)()
    if lib.mgr_abi_struct_sizes(sizes) != 0 or tuple(sizes) != (C.sizeof(ScanJob), C.sizeof(ScanBwdJob), C.sizeof(ScanLaunchOpts), ABI_REVISION):
        raise MgrError("libmgr.so was built from another include/mgr.h than this binding (struct sizes / revision %s, expected %s): rebuild it"
                       % (tuple(sizes), (C.sizeof(ScanJob), C.sizeof(ScanBwdJob), C.sizeof(ScanLaunchOpts), ABI_REVISION)))
    _lib = lib
    return lib


def check(rc, lib=None):
    if rc != 0:
        lib = lib or load_library()
        raise MgrError("libmgr error %d: %s" % (rc, lib.mgr_last_error().decode(errors="replace")))


class DeviceArray:
    """A typed view of device memory owned by a Device."""

    __slots__ = ("dev", "ptr", "shape", "dtype", "nbytes", "_own")

    def __init__(self, dev, ptr, shape, dtype, own=True):
        self.dev = dev
        self.ptr = ptr
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self._own = own

    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def view(self, offset_elems, shape):
        """Non-owning sub-view starting offset_elems elements in."""
        return DeviceArray(self.dev, self.ptr + offset_elems * self.dtype.itemsize, shape, self.dtype, own=False)

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        if host.size != self.size:
            raise ValueError("upload size mismatch: host %s vs device %s" % (host.shape, self.shape))
        check(self.dev.lib.mgr_h2d(self.dev.ctx, self.ptr, host.ctypes.data, self.nbytes))
        return self

    def download(self):
        out = np.empty(self.shape, self.dtype)
        check(self.dev.lib.mgr_d2h(self.dev.ctx, out.ctypes.data, self.ptr, self.nbytes))
        return out

    def zero(self):
        check(self.dev.lib.mgr_memset(self.dev.ctx, self.ptr, 0, self.nbytes))
        return self

    def free(self):
        if self._own and self.ptr:
            self.dev.lib.mgr_free(self.dev.ctx, self.ptr)
            self.ptr = 0


class Device:
    """One mgr_ctx (one GPU).  Fails loudly when no GPU / no library is available."""

    def __init__(self, index=0):
        self.lib = load_library()
        ctx = vp()
        check(self.lib.mgr_ctx_create(int(index), C.byref(ctx)), self.lib)
        self.ctx = ctx
        self.index = index
        cu = i32()
        hbm = sz()
        name = C.create_string_buffer(64)
        check(self.lib.mgr_device_info(self.ctx, C.byref(cu), C.byref(hbm), name, 64))
        self.cu_count = cu.value
        self.hbm_bytes = hbm.value
        self.name = name.value.decode()
        self._arrays = []
        self._pinned = []

    # -- memory ------------------------------------------------------------------------------------
    def empty(self, shape, dtype=np.float32):
        if isinstance(shape, int):
            shape = (shape,)
        n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        p = vp()
        check(self.lib.mgr_alloc(self.ctx, max(n, 16), C.byref(p)))
        a = DeviceArray(self, p.value, shape, dtype)
        self._arrays.append(a)
        return a

    def pinned(self, shape, dtype=np.float32):
        """Page-locked host array (numpy view) for mgr_h2d_async; freed with the Device."""
        n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        p = vp()
        check(self.lib.mgr_host_alloc(self.ctx, max(n, 16), C.byref(p)))
        self._pinned.append(p.value)
        buf = (C.c_char * n).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def h2d_async(self, darr, host_pinned):
        """Enqueue a copy from a pinned() array on the current stream; does not block the host."""
        check(self.lib.mgr_h2d_async(self.ctx, darr.ptr, host_pinned.ctypes.data, host_pinned.nbytes))

    def d2h_async(self, host_pinned, darr):
        """Enqueue a copy into a pinned() array on the current stream; valid after an event recorded behind it (event_sync)."""
        check(self.lib.mgr_d2h_async(self.ctx, host_pinned.ctypes.data, darr.ptr, min(host_pinned.nbytes, darr.nbytes)))

    def event_sync(self, ev):
        check(self.lib.mgr_event_sync(self.ctx, ev))

    def zeros(self, shape, dtype=np.float32):
        return self.empty(shape, dtype).zero()

    def array(self, host, dtype=None):
        host = np.asarray(host)
        dtype = dtype or host.dtype
        return self.empty(host.shape, dtype).upload(host)

    def bytes(self, nbytes):
        return self.empty((int(nbytes + 3) // 4,), np.float32)

    def free(self, *arrays):
        """Free some of this Device's arrays before the rest (temporaries of a call on a Device that lives on)."""
        dead = set(id(a) for a in arrays)
        for a in arrays:
            a.free()
        self._arrays = [a for a in self._arrays if id(a) not in dead]

    # -- streams / timing ------------------------------------------------------------------------
    def sync(self):
        check(self.lib.mgr_sync(self.ctx))

    def stream(self, idx):
        check(self.lib.mgr_stream_set(self.ctx, idx))

    def wait(self, waiter, waited):
        check(self.lib.mgr_stream_wait(self.ctx, waiter, waited))

    def record(self, ev):
        check(self.lib.mgr_event_record(self.ctx, ev))

    def wait_event(self, waiter, ev):
        check(self.lib.mgr_stream_wait_event(self.ctx, waiter, ev))

    def elapsed_ms(self, ev0, ev1):
        ms = C.c_float()
        check(self.lib.mgr_event_elapsed_ms(self.ctx, ev0, ev1, C.byref(ms)))
        return ms.value

    def prof_enable(self, mask):
        check(self.lib.mgr_prof_enable(self.ctx, mask))

    def prof_reset(self):
        check(self.lib.mgr_prof_reset(self.ctx))

    def prof_get(self, family):
        n = i32()
        ms = C.c_float()
        check(self.lib.mgr_prof_get(self.ctx, family, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def call(self, name, *args):
        """Invoke a C-ABI function with the ctx prepended; DeviceArrays are passed by pointer."""
        conv = [a.ptr if isinstance(a, DeviceArray) else a for a in args]
        check(getattr(self.lib, name)(self.ctx, *conv))

    def close(self):
        if self.ctx:
            for a in self._arrays:
                a.free()
            self._arrays = []
            for p in self._pinned:
                self.lib.mgr_host_free(self.ctx, p)
            self._pinned = []
            self.lib.mgr_ctx_destroy(self.ctx)
            self.ctx = None


def device_count():
    lib = load_library()
    n = i32()
    rc = lib.mgr_device_count(C.byref(n))
    return n.value if rc == 0 else 0
