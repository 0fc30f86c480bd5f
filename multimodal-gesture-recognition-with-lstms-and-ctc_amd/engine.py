"""Device engine: runs one network of the reference's family on one MI355X through the libmgr C ABI.

It owns the device-resident weights (packed layouts), the activation workspaces sized for a fixed
(B, T, Lmax), and sequences the HIP kernels for predict / train steps over the ctx's streams (the two
directions of every Bidirectional layer and the modality encoders run concurrently).  This is what
Keras' ``train_on_batch`` / ``predict_on_batch`` do for the reference (multimodal_fusion/multimodal.py:264,
multimodal_fusion/sequence_decoding.py:121); there is no CPU fallback.
"""
import collections
import ctypes as C
import itertools
import math

import numpy as np

from . import _capi, decoding
from . import augment as augment_mod
from . import seqlen
from ._capi import Device, DeviceArray
from .spec import frontend_layers, input_width


def _pad4(n):
    return (n + 3) // 4 * 4


class _Arena:
    """Allocations that live and die with one Engine (the Device itself may be shared)."""

    def __init__(self, dev):
        self.dev = dev
        self.arrays = []

    def _keep(self, a):
        self.arrays.append(a)
        return a

    def empty(self, shape, dtype=np.float32):
        return self._keep(self.dev.empty(shape, dtype))

    def zeros(self, shape, dtype=np.float32):
        return self._keep(self.dev.zeros(shape, dtype))

    def bytes(self, nbytes):
        return self._keep(self.dev.bytes(nbytes))

    def pinned(self, shape, dtype=np.float32):
        return self.dev.pinned(shape, dtype)   # (tiny; released with the Device)

    def release(self, arrays):
        """Free some of this arena's arrays before the rest."""
        dead = set(id(a) for a in arrays)
        for a in arrays:
            a.free()
        self.arrays = [a for a in self.arrays if id(a) not in dead]
        self.dev._arrays = [a for a in self.dev._arrays if id(a) not in dead]

    def free_all(self):
        dead = set(id(a) for a in self.arrays)
        for a in self.arrays:
            a.free()
        self.dev._arrays = [a for a in self.dev._arrays if id(a) not in dead]
        self.arrays = []


class _LstmDir:
    """Device state of one direction of one Bidirectional(LSTM) layer."""

    def __init__(self, prefix, d, fin, H, trainable):
        self.prefix = prefix
        self.d = d  # "fwd" | "bwd"
        self.reverse = 1 if d == "bwd" else 0
        self.fin = fin
        self.H = H
        self.trainable = trainable
        self.Wp = self.Up = self.bp = None
        self.gWp = self.gUp = self.gbp = None
        self.mask = None       # device [4,B,fin] when input dropout is active
        self.Z = None
        self.gates = self.cs = self.dZ = self.dzmax = self.dbsum = None
        self.ws_scan = self.ws_pg = self.ws_sp = None
        self.lists_mask = 0     # the mask whose kept lists the projection of this step left in ws_sp (0: none)
        self.HsT = None         # [B][H][ldt] split rows of h_prev (the recurrent weight gradient as a product along time; first use)
        self.hst_ready = False  # ... already written for the step in flight (Engine._prep_hst)


class Schedule:
    """How one training step is laid out over the context's streams.  The default is the schedule bench.py
    and fit_generator run; the switches exist so that tests can show every layout computes the same step.

    pipeline            with frozen encoders, the encoder pass of step n+1 runs on a second stream beside step n's
                        fusion layer / CTC / BPTT / optimizer
    defer_param_grads   step n's dW / dU / db GEMMs and the optimizer are held back until the deepest projection GEMMs of
                        step n+1 are done and then run beside its deepest encoder scan (GEMM beside GEMM gains nothing)
    encoders_run_ahead  the encoder stream does not wait for the previous step as a whole: only the scan that overwrites
                        the FEAT buffer that step's dW GEMMs read waits for it
    transposed_inputs   keep a transposed copy of the inputs of the wide dropout layers for the dropout-aware projection GEMMs
    resident_wait_us    upper bound of the device-side wait that lets the deepest encoder scan become resident before the
                        deferred GEMMs are released (mgr_stream_wait_next_resident); 0 = no wait
    encoders_two_ahead  (round 5; needs bptt_beside_deepest_scan) a caller that announces TWO batches ahead (enqueue_train_step's
                        prefetch_after_next) gets the first part of the batch-after-next's encoder pass enqueued at the end of a
                        step instead of at the start of the next call, which has to wait for the step's loss
    deepest_scan_after_fusion_proj  (round 5) the next batch's deepest encoder scan is launched behind this step's fusion projections
                        instead of at the same instant
    depth1_proj_ahead   (round 5; needs encoders_two_ahead) the depth-1 projections of the batch after next are enqueued on the encoder
                        stream IN FRONT of the next batch's deepest scan - into gate pre-activation buffers of their own - and run while
                        that stream would wait for this step's fusion projections (a store-bound f32 GEMM beside a staging-bound one)
    bptt_yields_beside_scans  (round 5) a narrow layer's BPTT that the schedule puts beside the next batch's encoder scans takes the form
                        that yields to them (mgr.h, MGR_TUNE_BPTT_FORM) instead of the one trimmed along its dependent chain (faster alone,
                        costs the step 0.1 - 0.2 ms there); bit-identical either way
    bptt_direct_when_alone  (round 5; measured, not the default) beside fused encoder scans the fusion layer's BPTT takes the direct-gather
                        form (mgr.h, MGR_TUNE_BPTT_FORM = 2: one barrier per step, the fastest form alone) - 16.64 - 16.72 against 16.60 - 16.61 ms
    fused_wide_tiles    (round 5) with fused encoder scans no GEMM shares a CU with a scan workgroup: the fusion layer's pre-split
                        products take the library's own tile choice instead of the 4-wave forms
    fused_encoder_scans (round 5; needs encoders_two_ahead) the encoder scans take the FUSED form (mgr.h, MGR_SCAN_FORM_FUSED: 8-wave
                        workgroups that hold a CU each, 208 instead of 408) and leave 48 CUs to the fusion layer's recurrences, which
                        are started once the encoder scan they run beside is resident.  Round 6: the form is an argument of each
                        launch and the launch number each wait is for is HANDED OVER by the launch itself (a page-locked word the
                        wait kernel polls, mgr_stream_wait_resident_word) - no context-wide tune key, no predicted numbers; a wait
                        that runs into its bound is counted (Engine.resident_wait_stats)
    fusion_scan_fused   (round 6; with fused_encoder_scans) the fusion layer's own forward scan takes the fused form as well
                        (MGR_SCAN_FORM_FUSED_ANY: H = 100 -> 4 eight-wave workgroups per cluster, 32 workgroups that hold a CU each,
                        instead of 56 four-wave workgroups on the 48 CUs the encoder scans leave, eight of which carry two).  The scan
                        itself is no faster (3.6 against 3.4 ms in the step); the 16 CUs it leaves free are what the head's Dense
                        kernels get (dense_bwd 0.85 -> 0.21 ms): 16.2 - 16.3 -> 15.9 - 16.0 ms per step (profiles/r06_schedule_probes.txt)
    bptt_fused          (round 6; with fused_encoder_scans) the fusion layer's BPTT takes the fused form too (MGR_BPTT_FORM_FUSED /
                        _FUSED_DIRECT with bptt_direct_when_alone: 32 eight-wave workgroups, a CU each, instead of 56 four-wave ones)
    chain_stream_priority  (round 6) dispatch priority of stream 0 against the encoder stream: 1 = stream 0 (the step's dependent chain)
                        high, -1 = the encoder stream low, 0 = equal (rounds 1 - 5).  Round 5 measured it zero-sum while both streams were
                        equally long; with the shared gather the encoder stream has slack
    param_grads_two_streams  (round 6) the dW / dU / db chains of the two directions of a Bidirectional layer run on two streams (the
                        second one: PG_STREAM) instead of one behind the other: the short kernels of one chain (lists, row maxima,
                        transposes, reductions) run under the long ones of the other
    first_pass_on_encoder_stream  (round 6; with fused_encoder_scans) a pipelined step that finds no prefetched encoder pass - the first step
                        of a run, the step after a validation pass - runs its own pass on the ENCODER stream in the fused forms and is a
                        steady-state call from there on (the next batch's pass follows at once, fused, its scans paired with this step's
                        recurrences through their launch numbers); round 5: in line on stream 0 in the plain forms, the next pass behind
                        a stream-wide wait, the fused forms only from the third step of a run on
    bptt_single_cu      (round 6; measured, not the default) narrow trainable layers (H in {32, 64, 100}) run their BPTT on ONE CU per
                        (direction, 16-sample group) without an inter-CU exchange (MGR_BPTT_FORM_SINGLE_CU, lstm_cu_bwd.hip) - in every
                        schedule (its results equal the multi-CU forms' to rounding, not bit for bit)
    du_split            (round 6) the recurrent weight gradient dU of a layer whose dW runs on pre-split rows is formed the same way - the
                        split rows of h_prev along time (one transposing pass over the layer's outputs) against the dZ^T rows the dW
                        product reads anyway - instead of by the f32 split-K product and its slab reduction
    feat_rows_when_unread  the deepest encoder scans write the row-major FEAT rows even in a pass in which every reader of the encoder
                        output takes the transposed copy FEAT^T (Engine._feat_rows_unread: a fusion layer whose projection and
                        weight-gradient calls read FEAT^T, no trainable stream).  Default: such a pass hands its scans Y = 0 (mgr.h,
                        mgr_scan_job) and the K-split scan step drops one 4-byte store per lane; bit-identical either way
    split_rows          (round 5) the transposed copies are written in the split row format (f16 hi / lo pairs) and the wide products
                        run as loader / matrix pipelines on pre-split operands (gemm_split.hip); False: f32 rows, converted by
                        every product that reads them (round 4's kernels)
    bptt_beside_deepest_scan  (round 4; needs the three switches above) the trainable layer's BPTT is held back together with its
                        GEMMs: recurrence beside recurrence, GEMM beside GEMM.  The encoder stream then runs free - the next batch's
                        encoder pass up to its deepest projections is enqueued BEFORE this step's fusion work, and its depth-1
                        projections no longer wait for this step's fusion projections
    """

    def __init__(self, pipeline=True, defer_param_grads=True, encoders_run_ahead=True, resident_wait_us=2000,
                 transposed_inputs=True, bptt_beside_deepest_scan=True, split_rows=True, encoders_two_ahead=True,
                 deepest_scan_after_fusion_proj=True, depth1_proj_ahead=True, bptt_yields_beside_scans=True,
                 fused_encoder_scans=True, fused_wide_tiles=True, bptt_direct_when_alone=False, fusion_scan_fused=True,
                 bptt_fused=False, chain_stream_priority=0, param_grads_two_streams=False, first_pass_on_encoder_stream=True,
                 bptt_single_cu=False, du_split=True, feat_rows_when_unread=False):
        self.feat_rows_when_unread = bool(feat_rows_when_unread)
        self.bptt_single_cu = bool(bptt_single_cu)
        self.du_split = bool(du_split)
        self.first_pass_on_encoder_stream = bool(first_pass_on_encoder_stream)
        self.param_grads_two_streams = bool(param_grads_two_streams)
        self.chain_stream_priority = int(chain_stream_priority)
        self.bptt_fused = bool(bptt_fused)
        self.fusion_scan_fused = bool(fusion_scan_fused)
        self.bptt_direct_when_alone = bool(bptt_direct_when_alone)
        self.fused_wide_tiles = bool(fused_wide_tiles)
        self.fused_encoder_scans = bool(fused_encoder_scans)
        self.bptt_yields_beside_scans = bool(bptt_yields_beside_scans)
        self.depth1_proj_ahead = bool(depth1_proj_ahead)
        self.deepest_scan_after_fusion_proj = bool(deepest_scan_after_fusion_proj)
        self.encoders_two_ahead = bool(encoders_two_ahead)
        self.split_rows = bool(split_rows)
        self.bptt_beside_deepest_scan = bool(bptt_beside_deepest_scan)
        self.transposed_inputs = bool(transposed_inputs)
        self.pipeline = bool(pipeline)
        self.defer_param_grads = bool(defer_param_grads)
        self.encoders_run_ahead = bool(encoders_run_ahead)
        self.resident_wait_us = int(resident_wait_us)


class StepLayout(collections.namedtuple("StepLayout", "beside_scans wide_ok enc_scan_form fusion_scan_form gate_fusion gate_bptt")):
    """What the launches of ONE training step look like.  enqueue_train_step builds it once and hands it to whatever
    enqueues for the step; closures that run later capture it.
    beside_scans      the fusion layer's GEMMs run beside encoder scans of the next batch (a pipelined step)
    wide_ok           ... of FUSED encoder scans, which share no CU with a GEMM: the library's own tile choice (Schedule.fused_wide_tiles)
    enc_scan_form     form of the encoder scan launches (mgr.h MGR_SCAN_FORM_*; AUTO: the context's MGR_TUNE_SCAN_FORM)
    fusion_scan_form  form of the fusion layer's scan launch
    gate_fusion / gate_bptt  fused encoder scans: the host words through which the launches the fusion scan / the BPTT of the step
                      wait for hand over their launch numbers (None: no wait)"""
    __slots__ = ()

    @property
    def fused(self):
        """A step of the fused schedule: one of its recurrences waits for an encoder scan to become resident."""
        return self.gate_fusion is not None or self.gate_bptt is not None


# everything that is not a pipelined training step: predict, loss_on_batch, predict_stream, a step on the plain schedule
PLAIN = StepLayout(False, False, _capi.SCAN_FORM_AUTO, _capi.SCAN_FORM_AUTO, None, None)


class Engine:
    closed = False      # set by close(): what shares this engine's buffers (live.LiveSession) checks it

    def __init__(self, spec, B, T, Lmax, device=0, seed=1234, comm=None, world=1, inference_only=False, schedule=None):
        self.spec = spec
        self.B, self.T, self.Lmax = int(B), int(T), int(Lmax)
        cdev = getattr(comm, "dev", None)
        if cdev is not None:
            # the all-reduce is enqueued on the communicator's context: it must be THIS engine's context, or it would not be
            # ordered against the gradient kernels and the optimizer
            if isinstance(device, Device) and device is not cdev:
                raise ValueError("the communicator was created on another Device than the engine's")
            device = cdev
        self._own_dev = not isinstance(device, Device)
        self.dev = device if isinstance(device, Device) else Device(device)
        self.schedule = schedule or Schedule()
        self.mem = _Arena(self.dev)           # device buffers owned by this engine
        self.lib = self.dev.lib
        self.seed = int(seed)
        self.comm = comm
        self.world = int(world)
        self.inference_only = inference_only
        if self.schedule.chain_stream_priority:
            # (a property of the CONTEXT's streams: engines that share a Device share it; the call waits for the stream to be idle)
            if self.schedule.chain_stream_priority > 0:
                self.dev.call("mgr_stream_set_priority", 0, 1)
            else:
                self.dev.call("mgr_stream_set_priority", self.ES, -1)
        self._adam_calls = 0  # optimizer steps enqueued; `iterations` (Keras) = those the update gate did not skip
        self.rng_step = 0     # advances per forward pass that draws randomness
        self._risk = None     # set_risk: the minimum-risk training mode's settings and buffers
        self._entropy = None  # set_entropy: the entropy-regularised training mode's weight and buffers
        self._augment = None  # set_augment: the train-time input augmentation's settings and buffers
        self._build()

    # ------------------------------------------------------------------------------------------ build
    def _build(self):
        sp, dev, B, T = self.spec, self.mem, self.B, self.T
        table = sp.weight_table()
        # flat trainable buffer layout (every segment padded to 4 floats)
        self.seg = {}
        off = 0
        for name, shape, tr, kind in table:
            n = int(np.prod(shape))
            if tr:
                self.seg[name] = (off, n, shape, kind)
                off += _pad4(n)
        self.n_train = off
        self.params = dev.zeros((max(off, 4),))
        # this engine's own scan-status block (several engines may share one Device): [0] status bits, [2] skipped updates
        self.status = dev.zeros((16,), np.uint32)
        # inference passes (predict / loss_on_batch / predict_stream) report into a block of their OWN per pass (two: batches of a
        # pipelined run alternate), so that one batch with a NaN input marks ITS samples and nothing else (words [8, 16): mgr.h)
        self._pass_status = [dev.zeros((16,), np.uint32) for _ in range(2)]
        self.loss_host = dev.pinned((4,), np.float32)
        self.status_host = dev.pinned((4,), np.uint32)
        # launch numbers handed from a persistent scan launch to the residency wait that was enqueued before it (page-locked: the
        # wait kernel polls the word; mgr_stream_wait_resident_word).  A ring: two words per step, reused eight steps later.
        self._seq_words = dev.pinned((16,), np.uint32)
        self._seq_words[...] = 0
        self._seq_next = 0
        # (diagnostic, bounded) per fused step: (step id, kind, the words its two residency waits poll) - tools/startup_probe.py
        self._gate_log = collections.deque(maxlen=16)
        # data parallel: [gate flag, sum over ranks of the local mean losses, -, -] of step s in slot s & 1, copied from behind the
        # all-reduced gradient buffer (apply_gradients); read by read_global_loss
        self.gloss_host = [dev.pinned((4,), np.float32) for _ in range(2)]
        self._gloss_step = [-1, -1]
        if not self.inference_only:
            # the 4 floats behind the gradients ride through the gradient all-reduce (apply_gradients): [0] the update-gate flag,
            # [1] this rank's mean loss of the step ("piggy-backed as one extra float")
            self.grads = dev.zeros((max(off, 4) + 4,))
            self.gate_flag = self.grads.view(max(off, 4), (4,))
            self.loss_slot = self.grads.view(max(off, 4) + 1, (1,))
            self.m = dev.zeros((max(off, 4),))
            self.v = dev.zeros((max(off, 4),))
        self.frozen = {}
        for name, shape, tr, kind in table:
            if not tr:
                self.frozen[name] = dev.zeros((_pad4(int(np.prod(shape))),))
        self.kinds = {name: kind for name, _, _, kind in table}
        self.shapes = {name: shape for name, shape, _, _ in table}

        # LSTM layer-direction objects
        self.dirs = {}
        train = not self.inference_only
        for prefix, fin, H, p, tr in sp.lstm_layers():
            for d in ("fwd", "bwd"):
                L = _LstmDir(prefix, d, fin, H, tr)
                base = "%s/%s" % (prefix, d)
                L.Wp, L.Up, L.bp = (self._wview(base + "/W"), self._wview(base + "/U"), self._wview(base + "/b"))
                if tr and train:
                    L.gWp, L.gUp, L.gbp = (self._gview(base + "/W"), self._gview(base + "/U"), self._gview(base + "/b"))
                    L.gates = dev.empty((B, T, H, 4))
                    L.cs = dev.empty((B, T, H))
                    L.dZ = dev.empty((B, T, 4 * H))
                    L.dzmax = dev.zeros((B, 4 * H), np.uint32)   # row maxima of dZ^T, left by the BPTT (mgr_scan_bwd_job.dzmax)
                    L.dbsum = dev.zeros((B, 4 * H))              # and its sums of dZ over time: db without a pass over dZ
                    L.ws_scan = dev.bytes(self.lib.mgr_lstm_scan_ws_bytes(B, T, H))
                    need = (self.lib.mgr_lstm_param_grads_dropout_ws_bytes(B, T, fin, H) if p > 0
                            else self.lib.mgr_lstm_param_grads_ws_bytes(B, T, fin, H))
                    if p > 0 and self.schedule.transposed_inputs:
                        # (+ the transposed dZ of the dropout-aware dW from the transposed activation copy: sized here, not by a
                        # hipMalloc in the middle of the first training step)
                        need = max(need, self.lib.mgr_lstm_param_grads_dropout_t_ws_bytes(B, T, fin, H, (T + 127) // 128 * 128))
                        if self._ts_shape(fin):
                            need = max(need, self.lib.mgr_lstm_param_grads_dropout_ts_ws_bytes(B, T, fin, H, (T + 127) // 128 * 128))
                    L.ws_pg = dev.bytes(need)
                if p > 0:
                    L.mask = dev.empty((4, B, fin))
                    need = self.lib.mgr_lstm_input_proj_dropout_ws_bytes(B, fin, H)                 # kept-feature lists, weight copies
                    if self._ts_shape(fin):
                        need = max(need, self.lib.mgr_lstm_input_proj_dropout_ts_ws_bytes(B, fin, H))
                    L.ws_sp = dev.bytes(need)
                L.p = p
                self.dirs[base] = L

        # activations
        W = sp.concat_width
        self.X = {}
        self.Y1 = {}
        self.Y2 = {}
        self.dY1 = {}
        self.Zbuf = {}
        self.Z1buf = {}
        self._xcur = {}
        # host batches arrive through a dedicated copy stream into two alternating input / label buffer sets, so an upload
        # never has to wait for (or stall the host behind) whatever the compute streams still have queued
        self._xin_ring = [{}, {}]
        self._xin_slot = 0
        self._xin_pin = None
        self._xin_user = [-1, -1]      # id of the last step that reads input set 0 / 1 (see _upload_inputs)
        self._xin_copied = [False, False]   # EV_XIN_COPIED / EV_LAB_COPIED of set 0 / 1 have been recorded
        self._lab_copied = [False, False]
        self._lab_user = [-1, -1]
        # per-sample sequence lengths (seqlen.KEY of an input dict): the device array of the batch in input set 0 / 1 (None:
        # that batch came without lengths), and per FEAT buffer that of the batch whose encoder pass filled it last - what the fusion
        # layer, the head and the backward pass of the step that consumes the buffer use, whichever call ran the encoder pass
        self._xin_len = [None, None]
        self._feat_len = {}
        self._len_ring = None          # (allocated with the first batch that carries lengths)
        self._len_next = 0
        self._step_id = 0              # training steps enqueued so far
        self._synced_step = -1         # the host has seen the loss of this step (everything before its CTC is complete)
        self.fe = {}       # stream name -> its CNN front-end: per conv layer (shape dict, pooled output, pool routing codes[, dX])
        for s in sp.streams:
            for ring in self._xin_ring:
                ring[s["name"]] = dev.empty((B, T, input_width(s)))
            if s.get("frontend"):
                self._build_frontend(s, train)
            if s["noise"] > 0:
                self.X[s["name"]] = dev.empty((B, T, s["F"]))
            self.Xin = self._xin_ring[0]
            Hs = [lay["H"] for lay in s["layers"]]
            zf = dev.empty((B, T, 4 * max(Hs)))
            zb = dev.empty((B, T, 4 * max(Hs)))
            self.Zbuf[s["name"]] = (zf, zb)
            if train and self.can_pipeline and self.schedule.depth1_proj_ahead and len(Hs) == 2:
                # (Schedule.depth1_proj_ahead: the depth-1 projections of a batch are written while the previous batch's deepest scan
                #  still reads the shared buffers)
                self.Z1buf[s["name"]] = (dev.empty((B, T, 4 * Hs[0])), dev.empty((B, T, 4 * Hs[0])))
            if len(Hs) == 2:
                self.Y1[s["name"]] = dev.empty((B, T, 2 * Hs[0]))
                if s["trainable"] and train:
                    if s["residual"]:
                        self.Y2[s["name"]] = dev.empty((B, T, 2 * Hs[1]))
                    self.dY1[s["name"]] = dev.empty((B, T, 2 * Hs[0]))
        self.FEAT = dev.empty((B, T, W))
        self._feat_ring = [self.FEAT]
        if (train and self.can_pipeline) or self.inference_only:
            # second FEAT buffer: cross-step pipelining of training (frozen encoders) / batch pipelining of inference
            self._feat_ring.append(dev.empty((B, T, W)))
        # Transposed copies [B, features, T padded to 128] of the inputs of the WIDE dropout layers (depth-2 encoder layers, the
        # fusion layer): the dropout-aware projection gathers kept FEATURES, which are contiguous rows there (gemm.hip,
        # k_gemm_nn_sparse<.., true>).  Row-major stays what everything else reads (dW GEMMs, residual adds, dense layer).
        self.ldt = (T + 127) // 128 * 128
        self.Y1T = {}
        self._featT = {}
        self._featT_ready = {}   # FEAT buffer -> its transposed copy was written by the scans of the current pass
        self._feat_rows = {}     # FEAT buffer -> the current pass wrote its row-major contents (False: only FEAT^T, _feat_rows_unread)
        self._xt_split = {}      # transposed copy (device pointer) -> its rows are in the split row format (as last written)
        if self.schedule.transposed_inputs:   # (training: dropout-aware GEMMs; inference: the dense split-f16 projection reads it too)
            want = lambda p, F: bool(self.lib.mgr_lstm_input_proj_dropout_wants_transposed(self.dev.ctx, C.c_float(float(p)), int(F)))
            for s in sp.streams:
                if len(s["layers"]) == 2 and want(s["layers"][1]["dropout"], 2 * s["layers"][0]["H"]):
                    self.Y1T[s["name"]] = dev.zeros((B, 2 * s["layers"][0]["H"], self.ldt))
            if sp.fusion and want(sp.fusion["dropout"], W):
                for fb in self._feat_ring:
                    self._featT[fb.ptr] = dev.zeros((B, W, self.ldt))
        self._feat_idx = 0
        self._prefetched = None
        self._prefetched_for = None
        self._masks = {}
        any_tr_stream = any(s["trainable"] for s in sp.streams)
        if sp.fusion:
            Hf = sp.fusion["H"]
            self.ZF = (dev.empty((B, T, 4 * Hf)), dev.empty((B, T, 4 * Hf)))
            self.YF = dev.empty((B, T, 2 * Hf))
            if train:
                self.dYF = dev.empty((B, T, 2 * Hf))
        if train and any_tr_stream:
            self.dFEAT = dev.empty((B, T, W))
        D, Cn = sp.head_width, sp.num_classes
        self.P = dev.empty((B, T, Cn))
        self.head_mask = None
        if train:
            self.dLogits = dev.empty((B, T, Cn))
            self.loss_b = dev.empty((B,))
            self.loss_mean = dev.empty((4,))
            self._lab_ring = [(dev.empty((B, self.Lmax), np.int32), dev.empty((B,), np.int32), dev.empty((B,), np.int32))
                              for _ in range(2)]
            self._lab_slot = 0
            self.labels_d, self.ilen_d, self.llen_d = self._lab_ring[0]
            # page-locked staging for the (tiny) label arrays: their copies are enqueued without blocking the host
            self._lab_pin = [(dev.pinned((B, self.Lmax), np.int32), dev.pinned((B,), np.int32), dev.pinned((B,), np.int32))
                             for _ in range(2)]
            self.ws_ctc = dev.bytes(self.lib.mgr_ctc_ws_bytes(B, T, Cn, self.Lmax))
            self.ws_dense = dev.bytes(self.lib.mgr_dense_bwd_ws_bytes(B, T, D, Cn))
            self.ws_head = dev.bytes(self.lib.mgr_head_ws_bytes(B, T, D, Cn, self.Lmax))
        # The schedule, resolved once: what Schedule's switches, the spec and the communicator allow a step of this engine (each name
        # narrows an earlier one; enqueue_train_step adds what only a call knows)
        sch = self.schedule
        self.depth = max(len(s["layers"]) for s in sp.streams)
        self.frozen_fusion = self.can_pipeline and sch.pipeline      # steps announced ahead are pipelined
        self.can_defer = self.frozen_fusion and sch.defer_param_grads and self.depth >= 2    # ... their dW / dU / db GEMMs held back
        self.can_hold_bptt = self.can_defer and sch.bptt_beside_deepest_scan                  # ... and the fusion layer's BPTT with them
        self.can_run_ahead = self.can_defer and sch.encoders_run_ahead      # the encoder stream waits for one scan's buffer, not a step
        self.can_run_free = self.can_hold_bptt and self.can_run_ahead       # ... and takes the next pass before the step's fusion work
        # (fused: not with a host-blocking all-reduce - HostComm holds the host inside finish(), the depth-1 scan the BPTT's wait is for
        #  would only be enqueued after it, the wait would always run into its bound; such runs share a GPU and use small batches anyway)
        self.can_fuse = self.can_run_free and sch.fused_encoder_scans and not getattr(self.comm, "host_blocking", False)
        self.dev.sync()

    def _build_frontend(self, s, train):
        """Buffers of a stream's CNN front-end: per conv layer the pooled output [B*T frames][Hp][Wp][Cout] (the last one is the
        stream's LSTM input [B, T, F]) and its pool routing codes; for training the gradient w.r.t. each layer's input but the
        first's (the data), the LSTM's dX into the last pooled map and the weight-gradient workspace."""
        dev, N = self.mem, self.B * self.T
        layers = []
        for i, c in enumerate(frontend_layers(s["frontend"])):
            lay = dict(c, Y=dev.empty((self.B, self.T, c["F"])), code=dev.empty((N * c["F"],), np.uint8), dX=None)
            if train and s["trainable"] and i > 0:
                lay["dX"] = dev.empty((N * c["Hin"] * c["Win"] * c["Cin"],))
            layers.append(lay)
        ws = None
        if train and s["trainable"]:
            ws = dev.bytes(max(self.lib.mgr_conv_pool_bwd_weights_ws_bytes(N, c["Hin"], c["Win"], c["Cin"], c["ks"], c["Cout"])
                               for c in layers))
        self.fe[s["name"]] = dict(layers=layers, ws=ws, dF=dev.empty((self.B, self.T, s["F"])) if ws is not None else None)

    def _frontend_fwd(self, name, X):
        """The front-end's forward on the current stream: conv + bias + ReLU + pool per layer (one launch each); returns the last
        pooled map, the stream's LSTM input."""
        N = self.B * self.T
        self.fe[name]["X0"] = X           # (read again by the first layer's weight gradient)
        for c in self.fe[name]["layers"]:
            pre = "%s/%s/" % (name, c["name"])
            self.dev.call("mgr_conv_pool_fwd", X, N, c["Hin"], c["Win"], c["Cin"], self._wview(pre + "W"), self._wview(pre + "b"),
                          c["ks"], c["Cout"], c["Y"], c["code"])
            X = c["Y"]
        return X

    def _frontend_bwd(self, name):
        """The front-end's backward on the current stream, from the gradient the first LSTM layer left in fe["dF"]: per layer, last
        first, dW / db and (but for the first layer) the gradient w.r.t. its input, which is the pooled map of the layer below."""
        fe, N = self.fe[name], self.B * self.T
        layers = fe["layers"]
        dY = fe["dF"]
        for i in range(len(layers) - 1, -1, -1):
            c = layers[i]
            X = layers[i - 1]["Y"] if i > 0 else fe["X0"]
            pre = "%s/%s/" % (name, c["name"])
            self.dev.call("mgr_conv_pool_bwd_weights", X, dY, c["code"], N, c["Hin"], c["Win"], c["Cin"], c["ks"], c["Cout"],
                          self._gview(pre + "W"), self._gview(pre + "b"), fe["ws"], fe["ws"].nbytes)
            if i > 0:
                self.dev.call("mgr_conv_pool_bwd_data", dY, c["code"], self._wview(pre + "W"), N, c["Hin"], c["Win"], c["Cin"], c["ks"],
                              c["Cout"], c["dX"])
                dY = c["dX"]

    def _wview(self, name):
        if name in self.seg:
            off, n, shape, _ = self.seg[name]
            return self.params.view(off, (n,))
        return self.frozen[name]

    def _gview(self, name):
        off, n, shape, _ = self.seg[name]
        return self.grads.view(off, (n,))

    # ------------------------------------------------------------------------------------------ weights
    def _bind(self, block=None):
        """Scans enqueued from here on report into THIS engine's status block (the Device may be shared) - or into `block`."""
        self.dev.call("mgr_scan_status_bind", self.status if block is None else block)

    def _begin_pass(self, slot=0):
        """An inference pass gets a zeroed status block of its own (current stream): what its scans report - a give-up, WHICH
        samples met a non-finite state - belongs to this pass only, whatever earlier passes or the training loop recorded."""
        blk = self._pass_status[slot]
        blk.zero()
        self._bind(blk)
        return blk

    def _end_pass(self, blk_words, out, what="inference pass"):
        """blk_words: the 16 words of the pass's status block on the host (read behind the pass).  Raises on a give-up; returns
        `out` with NaN in the rows of exactly the samples whose hidden state went NaN / Inf in THIS pass (the multi-CU exchange
        feeds 0 back for such a state, so other units of the sample may look finite where the reference's whole sample is NaN)."""
        self._bind()
        bits = int(blk_words[0])
        if bits & ~_capi.SCAN_NONFINITE:
            raise _capi.MgrError("a persistent scan of this %s gave up on a bounded spin (status %d): its outputs are invalid" % (what, bits))
        if not bits & _capi.SCAN_NONFINITE:
            return out
        field = np.asarray(blk_words[8:16], np.uint32)
        bad = np.array([bool((int(field[(b & 255) >> 5]) >> (b & 31)) & 1) for b in range(self.B)])
        return self._nan_rows(out, bad)

    def _nan_rows(self, out, bad):
        """NaN (floats) / -1 (integer label outputs) / empty paths in the rows of the samples marked in `bad`."""
        if isinstance(out, tuple):
            return tuple(self._nan_rows(o, bad) for o in out)
        if isinstance(out, list) and len(out) == len(bad):            # decoded label sequences: no labels for an invalid sample
            return [[] if bad[b] else o for b, o in enumerate(out)]
        if isinstance(out, np.ndarray) and out.shape[:1] == bad.shape:
            out = out.copy()
            out[bad] = np.nan if out.dtype.kind == "f" else -1
        return out

    def set_weights(self, weights):
        """weights: dict name -> numpy array in Keras layout (see NetworkSpec.weight_table).  Fresh weights start with a clean
        scan status: a NaN / give-up recorded under the old ones (diverged run) must not haunt a restored checkpoint."""
        dev = self.dev
        dev.stream(0)
        self.clear_scan_status()
        for name, shape, tr, kind in self.spec.weight_table():
            if name not in weights:
                continue
            w = np.ascontiguousarray(np.asarray(weights[name], dtype=np.float32))
            if tuple(w.shape) != tuple(shape):
                raise ValueError("weight %s: expected shape %s, got %s" % (name, shape, w.shape))
            dst = self._wview(name)
            if kind in ("kernel", "recurrent", "bias"):
                H = shape[-1] // 4
                rows = 1 if kind == "bias" else shape[0]
                tmp = dev.array(w.reshape(-1))
                dev.call("mgr_lstm_pack", tmp, dst, rows, H, 0)
                dev.sync()
                tmp.free()
            else:
                dst.view(0, (w.size,)).upload(w.reshape(-1))
        dev.sync()
        self._freeze_planes()

    def _freeze_planes(self):
        """The input weights of FROZEN layers (the encoders of the fusion network) are rewritten by set_weights only: the library may
        keep their split (hi, lo) planes in the projection workspaces from call to call (mgr_weight_planes_cache; every call drops
        what was kept, so this runs after every rewrite)."""
        for L in self.dirs.values():
            if L.ws_sp is not None and (L.prefix + "/" + L.d + "/W") in self.frozen:
                self.dev.call("mgr_weight_planes_cache", L.Wp, 1)

    def get_weights(self):
        dev = self.dev
        dev.stream(0)
        out = {}
        for name, shape, tr, kind in self.spec.weight_table():
            n = int(np.prod(shape))
            src = self._wview(name)
            if kind in ("kernel", "recurrent", "bias"):
                H = shape[-1] // 4
                rows = 1 if kind == "bias" else shape[0]
                tmp = dev.empty((n,))
                dev.call("mgr_lstm_pack", src, tmp, rows, H, 1)
                out[name] = tmp.download().reshape(shape)
                tmp.free()
            else:
                out[name] = src.view(0, (n,)).download().reshape(shape)
        return out

    def get_grads(self):
        """Trainable gradients of the last train step's backward pass, Keras layouts (tests / debugging)."""
        dev = self.dev
        dev.stream(0)
        out = {}
        for name, (off, n, shape, kind) in self.seg.items():
            src = self.grads.view(off, (n,))
            if kind in ("kernel", "recurrent", "bias"):
                H = shape[-1] // 4
                rows = 1 if kind == "bias" else shape[0]
                tmp = dev.empty((n,))
                dev.call("mgr_lstm_pack", src, tmp, rows, H, 1)
                out[name] = tmp.download().reshape(shape)
                tmp.free()
            else:
                out[name] = src.download().reshape(shape)
        return out

    def reset_optimizer(self):
        self.m.zero()
        self.v.zero()
        self.clear_scan_status()
        self.iterations = 0

    # ------------------------------------------------------------------------------------------ helpers
    def _seed(self, slot, step):
        """The kernel seed of random stream `slot` in the pass that draws at step counter `step`."""
        return (self.seed * 1000003 + step * 131 + slot) & 0xFFFFFFFFFFFFFFFF

    SAMPLE_SLOT = 998     # the stream constant of the risk mode's sampled hypothesis sets (the head dropout's is 999)
    _head_step = 0        # rng_step of the head pass enqueued last

    def _sample_seed(self, base):
        """_seed's derivation at the step counter the head pass enqueued last drew its dropout seed at, from `base` in the engine
        seed's place (None: the engine's seed)."""
        return ((self.seed if base is None else int(base)) * 1000003 + self._head_step * 131 + self.SAMPLE_SLOT) & 0xFFFFFFFFFFFFFFFF

    COPY_STREAM = 7
    EV_IN = (41, 42)     # last reader of input buffer set 0 / 1
    EV_LAB = (43, 44)    # last reader of label buffer set 0 / 1
    EV_XIN_COPIED = (59, 60)   # the host-to-device copies out of input staging set 0 / 1 are done (the HOST waits for it before it
    EV_LAB_COPIED = (61, 62)   # refills that page-locked set; ... label staging set 0 / 1)

    def _upload_inputs(self, inputs, rand, train, stream=0):
        """Host batch -> the input buffer set that is NOT the one read last, on the copy stream; `stream` (where the
        encoder pass that reads it will be enqueued) waits for the copies."""
        dev = self.dev
        lens = seqlen.of(inputs, self.B, self.T)     # (refused before anything is enqueued)
        slot = self._xin_slot ^ 1
        dev.stream(self.COPY_STREAM)
        # the set was last read by step _xin_user[slot]; once the host has read a loss at or after that step the readers
        # are known to be complete (stream order) and no device-side wait is needed; otherwise wait for the readers' event
        if self._xin_user[slot] > self._synced_step:
            dev.wait_event(self.COPY_STREAM, self.EV_IN[slot])
        if self._xin_pin is None:   # page-locked staging, allocated at the first host batch (resident-input runs never need it)
            self._xin_pin = [{s["name"]: dev.pinned((self.B, self.T, input_width(s)), np.float32) for s in self.spec.streams}
                             for _ in range(2)]
        # The page-locked staging set is refilled by the HOST: the copies enqueued out of it last time must be done.  (Round 6: a call
        # of the two-calls-ahead schedule that also runs its own encoder pass uploads THREE batches - its own, the next, the one after
        # next - and the third refill met the first copy still in flight: a few input values of the step changed, a loss moved by 1e-6,
        # one run in three.  Found by tests/test_gpu_schedule_contract.py.)
        if self._xin_copied[slot]:
            dev.event_sync(self.EV_XIN_COPIED[slot])
        for s in self.spec.streams:
            x = np.asarray(inputs[s["name"]])
            if s.get("frontend"):
                # (B, T, h, w, c) frames of a CNN front-end; they travel as rows of h * w * c
                want = (self.B, self.T) + tuple(int(v) for v in s["frontend"]["input_shape"])
                if x.shape != want:
                    raise ValueError("input %s: expected %s got %s" % (s["name"], want, x.shape))
                x = x.reshape(self.B, self.T, -1)
            elif x.shape != (self.B, self.T, s["F"]):
                raise ValueError("input %s: expected %s got %s" % (s["name"], (self.B, self.T, s["F"]), x.shape))
            stage = self._xin_pin[slot][s["name"]]
            np.copyto(stage, x, casting="unsafe")          # float64 batch -> float32 staging in one pass
            nz = rand.get(s["name"] + "/noise") if rand else None
            if train and nz is not None:
                stage += np.asarray(nz, dtype=np.float32)
            dev.h2d_async(self._xin_ring[slot][s["name"]], stage)   # the host does not wait for the copy
        self._xin_len[slot] = None if lens is None else self._upload_lengths(lens)
        dev.record(self.EV_XIN_COPIED[slot])
        self._xin_copied[slot] = True
        dev.wait(stream, self.COPY_STREAM)
        self._xin_slot = slot
        self._xin_user[slot] = 1 << 60     # set by the step that consumes it (enqueue_train_step)
        self.Xin = self._xin_ring[slot]
        dev.stream(stream)

    LEN_RING = 8

    def _upload_lengths(self, lens):
        """The lengths of the batch being uploaded -> the next of LEN_RING small device arrays, on the current (copy) stream, through
        page-locked staging of its own.  Not one per input set: the fusion layer and the backward pass of the step that consumes a
        batch still read its lengths when the input set is refilled two uploads later (its encoder pass is all that reads the
        inputs); eight uploads later every reader is behind a loss the host has read or an event an upload has waited for."""
        if self._len_ring is None:
            self._len_ring = [(self.dev.pinned((self.B,), np.int32), self.mem.empty((self.B,), np.int32)) for _ in range(self.LEN_RING)]
        pin, d = self._len_ring[self._len_next]
        self._len_next = (self._len_next + 1) % self.LEN_RING
        pin[...] = lens
        self.dev.h2d_async(d, pin)
        return d

    def _zero_tails(self, lens, bufs):
        """One mgr_seq_zero_tail on the current stream over bufs = [(buffer, row, ld)], each [B, T, row]; nothing without lengths."""
        if lens is None or not bufs:
            return
        arr = _capi.make_seq_fill_jobs([(b, row, ld, self.B, self.T) for b, row, ld in bufs])
        self.dev.call("mgr_seq_zero_tail", len(bufs), arr, lens)

    def _check_lengths(self, inputs, input_length=None, augment=False):
        """seqlen.check_batch for this engine: raises ValueError before anything is enqueued; the lengths (host) or None."""
        return seqlen.check_batch(inputs, self.B, self.T, int(self.spec.ctc["skip"]), input_length, data_parallel=self.comm is not None,
                                  frontend=bool(self.fe), augment=augment)

    # Bound on the transposed activation copies the engine keeps (Y1T, FEAT^T), in the convention of mgr.h's x_absmax: NEGATIVE =
    # guaranteed by the producer, not checked.  Every such copy holds outputs of LSTM layers of this library - h = o * tanh(c) with
    # o in [0, 1], so |h| <= 1 - or the residual sum of two of them (encoder stacks, multimodal.py:111,117): <= 2 by construction,
    # whether the scans wrote the copy themselves or mgr_transpose_bt made it from such a buffer.  A diverged state is NaN, not large.
    XT_BOUND = -2.0

    @staticmethod
    def _ts_shape(fin):
        """Layer widths the pre-split products handle (mgr_lstm_input_proj_dropout_ts / mgr_lstm_param_grads_dropout_ts)."""
        return 128 <= fin <= 2048

    def _split_rows_wanted(self, train):
        """The format a pass of learning phase `train` writes new transposed activation copies in: split rows (f16 hi / lo pairs,
        mgr.h) for the pre-split products on the f16 matrix pipe - unless MGR_TUNE_GEMM_F32 keeps the GEMMs on their f32 MFMA kernels
        (bench.py's second leg)."""
        if not self.schedule.split_rows or self.inference_only or not train:
            # (learning phase 0 has no dropout mask: ONE dense K loop stages the A tile once for the four gates - k_gemm_nn_dense16 on
            #  f32 rows; the pre-split kernel would stage it once per gate: 20.3 against 19.4 ms per pipelined batch.  By PHASE, not by
            #  engine: predict on a training engine and on an inference engine give the same bits)
            return False
        v = C.c_int()
        self.dev.call("mgr_tune_get", _capi.TUNE_GEMM_F32, C.byref(v))
        return v.value == 0

    def _make_xt(self, X, ldx, XT, B, T, fin, train):
        """Transposed copy of a row-major activation buffer the scans did not write themselves, in the format its pass wants."""
        split = self._split_rows_wanted(train) and self._ts_shape(fin)
        self.dev.call("mgr_transpose_bt_split" if split else "mgr_transpose_bt", X, ldx, XT, self.ldt, B, T, fin)
        self._xt_split[XT.ptr] = split

    def _project_pair(self, X, ldx, pair, Ls, B, T, fin, H, train, XT=None, xt_ready=False, x_rows=True):
        """Input projections of the two directions of one Bidirectional layer (pair = [mask, Wp, bp, Z] x 2).  With input
        dropout active the library runs each direction's K loops over the kept features only (from p >= 0.3 on) - from the
        transposed copy XT of the input where the engine keeps one (pre-split rows: the loader / matrix pipeline of gemm_split.hip;
        f32 rows: the kernels of gemm.hip); otherwise both directions go through one call that fuses them into one GEMM where that
        saves tiles.  x_rows=False: the row-major X was not written (_feat_rows_unread) - a path that would read it is an error."""
        masked, unmasked_wide = self._proj_kind(pair[0], XT, fin, Ls[0])
        if not x_rows and (XT is None or not (masked or unmasked_wide) or not xt_ready):
            raise RuntimeError("this projection reads row-major input the encoder pass left out")
        if XT is not None and (masked or unmasked_wide) and not xt_ready:   # (xt_ready: the scans that produced X wrote XT themselves, mgr_scan_job.YT)
            self._make_xt(X, ldx, XT, B, T, fin, train)
        split = XT is not None and self._xt_split.get(XT.ptr, False)
        if masked or unmasked_wide:
            # (no dropout - inference - on a wide layer whose input the engine keeps transposed: the same kernels without a mask)
            for d in range(2):
                m, Wp, bp, Z = pair[4 * d:4 * d + 4]
                ws = Ls[d].ws_sp
                p = float(Ls[d].p) if masked else 0.0
                if split:
                    self.dev.call("mgr_lstm_input_proj_dropout_ts", XT, self.ldt, m, p, Wp, bp, Z, B, T, fin, H, ws, ws.nbytes)
                    Ls[d].lists_mask = m if masked else 0     # (the kept lists of this mask now sit in ws: the dW product of the step reuses them)
                elif XT is not None:
                    self.dev.call("mgr_lstm_input_proj_dropout_t", XT, self.ldt, m, p, Wp, bp, Z, B, T, fin, H, ws, ws.nbytes, self.XT_BOUND)
                else:
                    self.dev.call("mgr_lstm_input_proj_dropout", X, ldx, m, p, Wp, bp, Z, B, T, fin, H, ws, ws.nbytes)
        else:
            self.dev.call("mgr_lstm_input_proj_pair", X, ldx, *pair, B, T, fin, H)

    def _prep_mask(self, L, train, rand, slot, step):
        """Returns the device pointer (or 0) of the [4,B,fin] input-dropout mask for this pass (drawn at step counter `step`)."""
        if not self._mask_drawn(L, train, rand):
            return 0  # (also: explicit randomness given but no mask for this layer: no dropout)
        if rand is not None:
            L.mask.upload(np.asarray(rand["%s/%s/mask" % (L.prefix, L.d)], dtype=np.float32))
            return L.mask.ptr
        self.dev.call("mgr_dropout_mask", L.mask, L.mask.size, float(L.p), C.c_uint64(self._seed(slot, step)))
        return L.mask.ptr

    @staticmethod
    def _mask_drawn(L, train, rand):
        """Whether a pass with this learning phase and this explicit randomness applies an input-dropout mask to direction L."""
        if not train or L.p <= 0:
            return False
        key = "%s/%s/mask" % (L.prefix, L.d)
        return rand is None or (key in rand and rand[key] is not None)

    # What the products of a Bidirectional layer read their input from - decided HERE, for the calls that make them (_project_pair,
    # _bilstm_backward) and for the encoder pass that leaves out the row-major FEAT nobody reads (_feat_rows_unread) alike.
    @staticmethod
    def _proj_kind(has_mask, XT, fin, L):
        """(masked, unmasked_wide) of a projection: either one with a transposed copy XT reads XT, anything else the rows."""
        masked = bool(has_mask) and L.ws_sp is not None
        unmasked_wide = not has_mask and XT is not None and 128 <= fin <= 2048 and L.ws_sp is not None
        return masked, unmasked_wide

    def _pgrad_kind(self, has_mask, XinT, split, p, fin):
        """The weight-gradient call of one direction: "ts" (pre-split rows of XinT), "t" (f32 rows of XinT) or "rows" (row-major)."""
        if has_mask and XinT is not None and split:
            return "ts"
        if has_mask and XinT is not None and self.lib.mgr_lstm_param_grads_dropout_wants_transposed(
                self.dev.ctx, C.c_float(float(p)), int(fin)):
            return "t"
        return "rows"

    def _feat_rows_unread(self, train, rand, feat_buf, feat_split):
        """True when nothing reads the row-major FEAT a pass with this learning phase / randomness writes into feat_buf, its scans
        writing FEAT^T in the format feat_split says: the fusion projection and - in a pass that keeps state for a backward pass - the
        fusion layer's weight-gradient calls take the transposed copy, and no stream is trainable (no residual add into FEAT, no
        encoder backward over it, no dFEAT).  The deepest scans then get Y = 0 (mgr.h).  Schedule.feat_rows_when_unread keeps the rows."""
        sp = self.spec
        XT = self._featT.get(feat_buf.ptr)
        if self.schedule.feat_rows_when_unread or not sp.fusion or XT is None or any(s["trainable"] for s in sp.streams):
            return False
        W = sp.concat_width
        Ls = [self.dirs["fusion/fwd"], self.dirs["fusion/bwd"]]
        drawn = [self._mask_drawn(L, train, rand) for L in Ls]
        if not any(self._proj_kind(drawn[0], XT, W, Ls[0])):      # (_project_pair branches on the first direction's mask)
            return False
        if train and not self.inference_only:
            return all(self._pgrad_kind(m, XT, feat_split, L.p, W) != "rows" for m, L in zip(drawn, Ls))
        return True

    # ------------------------------------------------------------------------------------------ forward
    def _forward(self, train, rand):
        """Encoders + fusion + head, all on stream 0 (predict / parity / non-pipelined training)."""
        if self._prefetched is not None:   # a pipelined encoder pass is in flight: let it finish, then discard it
            self.dev.wait(0, self.ES)
            self._prefetched = None
        self._enqueue_encoders(train, rand, self.FEAT, 0, self.rng_step)
        self._enqueue_fusion_head(train, rand, self.FEAT, self.rng_step)
        if train:
            self.rng_step += 1

    def _enqueue_encoders(self, train, rand, feat_buf, es, rng_step, hold_scans_for=None, augment=False, scan_form=_capi.SCAN_FORM_AUTO):
        """Noise + every encoder depth (input-projection GEMMs, then all recurrences of the depth in one multi-scan
        call), written into feat_buf.  Everything is enqueued on stream `es`.  augment, scan_form: _encoder_phases'."""
        for tag, k in self._encoder_phases(train, rand, feat_buf, es, rng_step, augment=augment, scan_form=scan_form):
            if tag != "projected":
                continue
            if hold_scans_for is not None and k >= 1:
                # pipelined with another stream: a persistent cluster launch that starts while chip-filling GEMMs of the
                # other stream are draining gets a lopsided workgroup placement for its whole life (measured 23 ms
                # instead of 11 ms), so the deep scans wait for that stream's queued work first
                self.dev.stream(es)
                self.dev.wait(es, hold_scans_for)

    def _encoder_phases(self, train, rand, feat_buf, es, rng_step, first_stream=None, z_first=None, seq_words=None, augment=False,
                        scan_form=_capi.SCAN_FORM_AUTO):
        """Generator form of the encoder pass: yields ("projected", k) after the projection GEMMs of depth k are enqueued
        (before its scan) and ("scanned", k) after its multi-scan launch, so that a caller can interleave work of another
        stream at those points.  Re-selects stream `es` after every resume; the pass draws its randomness at step counter
        `rng_step`, whatever self.rng_step is by the time a part of it is enqueued.
        first_stream / z_first (pipelined inference): the noise kernels and the depth-1 projections are enqueued on stream
        `first_stream` instead, into the gate pre-activation buffers z_first[name] = (fwd, bwd) instead of the stream's shared
        Zbuf - the caller orders `es` behind them before it resumes the generator.
        seq_words: dict {depth k: address of a host word} - the scan launch of depth k hands its launch number to that word (looked
        up when the launch is enqueued, so a caller may fill the dict while the generator is suspended).  scan_form: the form of
        the pass's scan launches (MGR_SCAN_FORM_*: StepLayout.enc_scan_form of the step that starts the pass).
        augment: this is the pass of a TRAINING STEP (only enqueue_train_step's passes say so: the train-phase passes of
        loss_on_batch / forward_train_phase stay what they are) - with set_augment on, the plan of THIS pass's rng_step is drawn and
        every stream goes through mgr_augment_apply, its noise included, in mgr_add_gaussian_noise's place."""
        sp, dev, B, T = self.spec, self.dev, self.B, self.T
        W = sp.concat_width
        save = train and not self.inference_only
        slot = 0
        cols = {}
        col = 0
        for s in sp.streams:
            cols[s["name"]] = col
            col += sp.stream_width(s)
        dev.stream(es if first_stream is None else first_stream)
        # the lengths of the batch this pass reads (None: none) stay with the FEAT buffer it fills
        lens = self._feat_len[feat_buf.ptr] = self._xin_len[self._xin_slot]
        aug = self._augment if (augment and train and rand is None) else None
        if aug is not None:
            # one plan per pass, from the pass's own step counter: a prefetched pass draws the plan of the step that consumes it, and
            # a stale pass that is redone draws the same plan again
            augment_mod.enqueue_plan(dev, aug["cfg"], aug["table"], B, T, self._seed(augment_mod.PLAN_SLOT, rng_step), aug["plan"])
        # GaussianNoise (K1) per stream
        for si, s in enumerate(sp.streams):
            name = s["name"]
            X = self.Xin[name]
            if aug is not None:
                # warp, masks, dropped stream and the stream's noise in one pass; the resident input stays pristine
                augment_mod.enqueue_apply(dev, aug["cfg"], si, X, self.X[name], aug["plan"], B, T, float(s["noise"]), self._seed(900 + si, rng_step))
                X = self.X[name]
            elif train and rand is None and s["noise"] > 0:
                # on device; the resident input stays pristine for the next step
                dev.call("mgr_add_gaussian_noise", X, self.X[name], X.size, float(s["noise"]),
                         C.c_uint64(self._seed(900 + si, rng_step)))
                X = self.X[name]
            if name in self.fe:
                X = self._frontend_fwd(name, X)     # (where the other networks apply GaussianNoise: the CNN front-end)
            self._xcur[name] = X
        depth = max(len(s["layers"]) for s in sp.streams)
        feat_by_scans = True     # every stream's last layer writes FEAT (and its transposed copy) from its scan
        split_now = self._split_rows_wanted(train)   # the format of the transposed copies this pass's scans write
        feat_split = bool(split_now and self._ts_shape(W))
        # every reader of this pass's encoder output takes FEAT^T: the scans that write both leave the row-major copy out
        no_rows = self._feat_rows_unread(train, rand, feat_buf, feat_split)
        self._feat_rows[feat_buf.ptr] = not no_rows
        for k in range(depth):
            jobs = []
            for si, s in enumerate(sp.streams):
                nl = len(s["layers"])
                if k >= nl:
                    continue
                name = s["name"]
                H = s["layers"][k]["H"]
                last = k == nl - 1
                col = cols[name]
                if k == 0:
                    cur, ldcur, fin = self._xcur[name], s["F"], s["F"]
                else:
                    Hp = s["layers"][k - 1]["H"]
                    cur, ldcur, fin = self.Y1[name], 2 * Hp, 2 * Hp
                pair, Ls_pair = [], []
                for di, dname in enumerate(("fwd", "bwd")):
                    L = self.dirs["%s/l%d/%s" % (name, k, dname)]
                    Ls_pair.append(L)
                    slot += 1   # (every projection GEMM fills the chip: one stream keeps their timings honest)
                    mptr = self._prep_mask(L, train, rand, slot, rng_step)
                    self._masks[(L.prefix, L.d)] = mptr
                    zb = z_first[name] if (k == 0 and z_first is not None) else self.Zbuf[name]
                    pair += [mptr, L.Wp, L.bp, zb[di]]
                self._project_pair(cur, ldcur, pair, Ls_pair, B, T, fin, H, train, XT=self.Y1T.get(name) if k == 1 else None,
                                   xt_ready=True)
                for di, dname in enumerate(("fwd", "bwd")):
                    L = self.dirs["%s/l%d/%s" % (name, k, dname)]
                    Z = (z_first[name] if (k == 0 and z_first is not None) else self.Zbuf[name])[di]
                    R, ldr = 0, 0
                    YT, ytb = 0, 0      # transposed copy written by the scan itself (what the next dropout layer's GEMMs read)
                    yt_fmt = 0
                    if not last:
                        Y, ldy = self.Y1[name].view(di * H, (1,)), 2 * H
                        if name in self.Y1T:
                            YT, ytb = self.Y1T[name].ptr + di * H * self.ldt * 4, 2 * H * self.ldt
                            yt_fmt = int(split_now and self._ts_shape(2 * H))
                            self._xt_split[self.Y1T[name].ptr] = bool(yt_fmt)
                    elif nl == 2 and s["residual"] and name in self.Y2 and save:
                        Y, ldy = self.Y2[name].view(di * H, (1,)), 2 * H
                        feat_by_scans = False
                    else:
                        Y, ldy = feat_buf.view(col + di * H, (1,)), W
                        if nl == 2 and s["residual"]:
                            R, ldr = self.Y1[name].view(di * H, (1,)), 2 * H
                        if feat_buf.ptr in self._featT:
                            YT, ytb = self._featT[feat_buf.ptr].ptr + (col + di * H) * self.ldt * 4, W * self.ldt
                            yt_fmt = int(feat_split)
                            self._xt_split[self._featT[feat_buf.ptr].ptr] = bool(yt_fmt)
                            if no_rows:
                                Y, ldy = 0, 0
                    keep = save and L.trainable
                    jobs.append(dict(Z=Z, Up=L.Up, Y=Y, ldy=ldy, R=R, ldr=ldr, gates=L.gates if keep else 0,
                                     cs=L.cs if keep else 0, B=B, T=T, H=H, reverse=L.reverse, YT=YT, ytb=ytb,
                                     ldt=self.ldt if YT else 0, yt_split=yt_fmt))
            # (lengths: a reverse recurrence meets zero gate pre-activations in a sample's tail and keeps h = c = 0 through it)
            self._zero_tails(lens, [(j["Z"], 4 * j["H"], 4 * j["H"]) for j in jobs if j["reverse"]])
            if k == 0:
                dev.record(self.EV_IN[self._xin_slot])   # the inputs have been read (noise kernel / depth-1 projections)
            yield ("projected", k)
            dev.stream(es)
            # all recurrences of this depth in ONE call (one persistent multi-CU launch when H is large)
            self._scan_multi(jobs, "_ws_multi", form=scan_form, seq_word=(seq_words or {}).get(k, 0))
            # (... and its saved gates are zeroed there: the BPTT's dZ is exactly 0 in the tail)
            self._zero_tails(lens, [(j["gates"], 4 * j["H"], 4 * j["H"]) for j in jobs if j["reverse"] and j["gates"]])
            yield ("scanned", k)
            dev.stream(es)
        self._featT_ready[feat_buf.ptr] = feat_by_scans
        for si, s in enumerate(sp.streams):
            name = s["name"]
            if len(s["layers"]) == 2 and s["residual"] and name in self.Y2 and save:
                H = s["layers"][-1]["H"]
                dev.call("mgr_add2d", self.Y1[name], 2 * H, self.Y2[name], 2 * H, feat_buf.view(cols[name], (1,)), W,
                         B * T, 2 * H)

    def _enqueue_fusion_head(self, train, rand, feat_buf, rng_step, dense=True, lay=PLAIN):
        """Fusion BiLSTM (projection GEMMs + recurrences) and Dropout/Dense/softmax on stream 0 (dense=False: the caller runs
        the Dense layer itself - the training step's mgr_head_fwd_bwd).  lay: the StepLayout of the training step this is part of."""
        sp, dev, B, T = self.spec, self.dev, self.B, self.T
        W = sp.concat_width
        save = train and not self.inference_only
        dev.stream(0)
        feat, ldf = feat_buf, W
        self._featin = feat_buf
        lens = self._feat_len.get(feat_buf.ptr)     # (of the batch whose encoder pass filled feat_buf)
        if sp.fusion:
            Hf = sp.fusion["H"]
            jobs = []
            pair, Ls_pair = [], []
            for di, dname in enumerate(("fwd", "bwd")):
                L = self.dirs["fusion/%s" % dname]
                Ls_pair.append(L)
                mptr = self._prep_mask(L, train, rand, 500 + di, rng_step)
                self._masks[(L.prefix, L.d)] = mptr
                pair += [mptr, L.Wp, L.bp, self.ZF[di]]
            # (pipelined training: these GEMMs run while the next batch's deepest encoder scan holds the chip - the forms of the
            # pre-split products that fit on a CU beside a scan workgroup, not the 8-wave ones that wait for the scan to end)
            with self._narrow_tiles(lay.beside_scans and not lay.wide_ok):
                self._project_pair(feat_buf, W, pair, Ls_pair, B, T, W, Hf, train, XT=self._featT.get(feat_buf.ptr),
                                   xt_ready=self._featT_ready.get(feat_buf.ptr, False), x_rows=self._feat_rows.get(feat_buf.ptr, True))
            self._zero_tails(lens, [(self.ZF[1], 4 * Hf, 4 * Hf)])
            dev.record(self.EV_FPROJ)   # (the next step's depth-1 scan is launched after these GEMMs, _enqueue_next_encoders)
            if lay.gate_fusion is not None:
                # (Schedule.fused_encoder_scans: the fusion scan's 56 workgroups must land on the CUs the next batch's deepest encoder
                #  scan - 208 whole CUs, released by the same event - leaves free, not on 56 CUs of their own.  That scan is enqueued
                #  LATER in this call: it hands its launch number to the word this wait polls)
                dev.call("mgr_stream_wait_resident_word", int(lay.gate_fusion), int(self.schedule.resident_wait_us))
            for di, dname in enumerate(("fwd", "bwd")):
                L = self.dirs["fusion/%s" % dname]
                jobs.append(dict(Z=self.ZF[di], Up=L.Up, Y=self.YF.view(di * Hf, (1,)), ldy=2 * Hf, R=0, ldr=0,
                                 gates=L.gates if save else 0, cs=L.cs if save else 0, B=B, T=T, H=Hf,
                                 reverse=L.reverse))
            self._scan_multi(jobs, "_ws_multi_f", form=lay.fusion_scan_form)
            self._zero_tails(lens, [(j["gates"], 4 * Hf, 4 * Hf) for j in jobs if j["reverse"] and j["gates"]])
            feat, ldf = self.YF, 2 * Hf
        # head
        D, Cn = sp.head_width, sp.num_classes
        p_head = float(sp.head["dropout"]) if train else 0.0
        hm = 0
        self._head_seed = 0
        if train and rand is not None:
            p_head = 0.0
            if rand.get("head/mask") is not None:
                if self.head_mask is None:
                    self.head_mask = self.mem.empty((B, T, D))
                self.head_mask.upload(np.asarray(rand["head/mask"], dtype=np.float32))
                hm = self.head_mask.ptr
        elif train and p_head > 0:
            self._head_seed = self._seed(999, rng_step)
        self._head_args = (hm, p_head, self._head_seed)
        self._head_step = rng_step      # (the counter this pass draws at: _sample_seed)
        if dense:
            dev.call("mgr_dense_softmax_fwd", feat, ldf, hm, p_head, C.c_uint64(self._head_seed),
                     self._wview("dense/W"), self._wview("dense/b"), self.P, B, T, D, Cn)
            self._zero_tails(lens, [(self.P, Cn, Cn)])      # (what a caller gets does not depend on the padding anywhere)
        self._feat = (feat, ldf)

    _early_words = None      # seq_words dict of the generator in _early_gen
    _since_fresh = 0         # pipelined calls since the last one that started the next batch's pass itself (0 in such a call)
    _early_for = None        # the inputs the generator started last was announced for
    _early_gen = None        # _next_encoders_free generator of the batch after next, its first part already enqueued

    def _tuned(self, on, keys, keep_set=False):
        """Context manager: the library calls enqueued inside run with the tune keys `keys` ({key: value}, mgr.h); a caller's own
        settings - bench.py --tune ... - come back afterwards (keep_set: and are not overridden where they are non-zero)."""
        eng = self

        class _Ctx:
            def __enter__(self_):
                self_.old = {}
                if on:
                    for k, val in keys.items():
                        v = C.c_int()
                        eng.dev.call("mgr_tune_get", k, C.byref(v))
                        if keep_set and v.value != 0:
                            continue
                        self_.old[k] = v.value
                        eng.dev.call("mgr_tune", k, val)

            def __exit__(self_, *exc):
                for k, val in self_.old.items():
                    eng.dev.call("mgr_tune", k, val)
                return False
        return _Ctx()

    def _narrow_tiles(self, on):
        """Context manager: the pre-split products enqueued inside take their 4-wave forms (MGR_TUNE_PROJ_TS_TILE = 1, mgr.h)."""
        return self._tuned(on, {_capi.TUNE_PROJ_TS_TILE: 1})

    def _new_seq_word(self):
        """Address of a zeroed page-locked word: a launch number on its way from the launch (mgr_scan_launch_opts.seq_out) to the
        wait that was enqueued before it (mgr_stream_wait_resident_word)."""
        i = self._seq_next
        self._seq_next = (i + 1) % self._seq_words.size
        self._seq_words[i] = 0
        return self._seq_words.ctypes.data + 4 * i

    def _scan_multi(self, jobs, wsname, form=_capi.SCAN_FORM_AUTO, seq_word=0):
        """One multi-scan call on the current stream; `wsname` keeps the encoder and fusion workspaces apart (they may
        be in flight at the same time when steps are pipelined).  form: mgr.h MGR_SCAN_FORM_* (AUTO: the context's MGR_TUNE_SCAN_FORM);
        seq_word: address of the host word that receives the launch number (0: not wanted)."""
        arr = _capi.make_scan_jobs(jobs)
        opts = _capi.make_launch_opts(form, seq_word)
        # (what THIS launch needs: a job without Y gets row scratch only where its kernel does not write the transposed copy itself)
        need = self.lib.mgr_lstm_scan_fwd_multi_ws_bytes(self.dev.ctx, len(jobs), arr, C.byref(opts))
        if need == 0:
            _capi.check(-1, self.lib)
        ws = getattr(self, wsname, None)
        if ws is None or ws.nbytes < need:
            ws = self.mem.bytes(need)
            setattr(self, wsname, ws)
        _capi.check(self.lib.mgr_lstm_scan_fwd_multi_ex(self.dev.ctx, len(jobs), arr, ws.ptr, ws.nbytes, C.byref(opts)))

    def resident_wait_stats(self):
        """(residency waits of this engine's context that have ended, those that ran into their bound) - mgr_resident_wait_stats.
        A wait at its bound costs Schedule.resident_wait_us of its stream and means the schedule's hand-over failed."""
        out = (C.c_uint * 4)()
        self.dev.call("mgr_resident_wait_stats", out)
        return int(out[0]), int(out[1])

    # ------------------------------------------------------------------------------------------ public
    def scan_health(self, snapshot=None):
        """(status bits, optimizer updates skipped by the update gate) of THIS engine since the last clear_scan_status(),
        read on the current stream (or taken from `snapshot`, the words a step copied to the host with its loss); never raises."""
        st = (C.c_uint * 4)()
        if snapshot is not None:
            st[0], st[2] = int(snapshot[0]), int(snapshot[2])
        else:
            self._bind()
            self.dev.call("mgr_scan_status_ex", st)
        self.updates_skipped = int(st[2])
        if st[0] & _capi.SCAN_NONFINITE:
            self.nonfinite_seen = True
        return int(st[0]), int(st[2])

    def _check_scans(self, step=None, snapshot=None):
        """Raises if a persistent scan of this engine gave up on a bounded spin (its outputs are garbage; the update gate keeps
        that step's gradients away from the weights, apply_gradients); a non-finite hidden state is not an error of the
        engine - the outputs / loss carry the NaN like the reference's would - and is remembered in `nonfinite_seen` until
        clear_scan_status().  `updates_skipped` counts the optimizer steps the gate has dropped since then."""
        bits, skipped = self.scan_health(snapshot)
        if bits & ~_capi.SCAN_NONFINITE:
            where = "" if step is None else " (noticed with the loss of training step %d)" % step
            raise _capi.MgrError("a persistent scan gave up on a bounded spin (status %d)%s: the outputs of that pass are invalid and "
                                 "its optimizer update is skipped on the device (the weights stay as they were) - "
                                 "clear_scan_status() to continue" % (bits, where))

    nonfinite_seen = False
    updates_skipped = 0

    @property
    def iterations(self):
        """Optimizer updates APPLIED so far (Keras `iterations`: learning-rate decay, Adam bias correction): the steps enqueued
        minus those the update gate skipped on the device, as far as the host knows (updates_skipped is refreshed with every
        loss read-back and by scan_health())."""
        return max(0, self._adam_calls - int(self.updates_skipped))

    @iterations.setter
    def iterations(self, value):
        self._adam_calls = int(value) + int(self.updates_skipped)

    def clear_scan_status(self):
        """Forget recorded scan status bits (after recovering from a diverged run / a give-up)."""
        self.scan_health()             # (the device's skipped-update count restarts at 0: fold it into the host's counter first)
        applied = self.iterations
        self.dev.call("mgr_scan_status_clear")
        self.nonfinite_seen = False
        self.updates_skipped = 0
        self._adam_calls = applied

    def predict(self, inputs):
        """Softmax output (B,T,C) with learning phase 0 (sequence_decoding.py:81)."""
        self._check_lengths(inputs)
        self._upload_inputs(inputs, None, False)
        blk = self._begin_pass()
        self._forward(False, None)
        P = self.P.download()
        return self._end_pass(blk.download(), P)

    def open_live(self, sessions, chunk, lookahead, cap=None):
        """A live.LiveSession over this engine's device weights: `sessions` slots fed frame by frame (push / end / reset / step),
        the BiLSTMs in windows of chunk + lookahead frames with the forward states carried.  Works on any engine,
        inference_only included; the session has its own buffers and touches none of this engine's."""
        from . import live
        return live.LiveSession(self, sessions, chunk, lookahead, cap=cap)

    def forward_train_phase(self, inputs, rand=None):
        """Softmax output with learning phase 1 (dropout / noise active) - no gradient."""
        self._check_lengths(inputs)
        self._upload_inputs(inputs, rand, True)
        blk = self._begin_pass()
        self._forward(True, rand)
        P = self.P.download()
        return self._end_pass(blk.download(), P)

    # ------------------------------------------------------------------------------------------ pipelined inference / validation
    EV_ENC = (46, 47)     # the encoder pass into FEAT buffer 0 / 1 is complete
    EV_FUSED = (48, 49)   # the fusion / head pass that read FEAT buffer 0 / 1 (and whatever decodes its output) is complete
    EV_OUT = (50, 51)     # the result of the batch in output slot 0 / 1 has reached its pinned host buffer
    EV_D1P = (55, 56)     # the depth-1 projections into depth-1 Z set 0 / 1 are done (stream 0)
    EV_D1S = (57, 58)     # the depth-1 scans that read depth-1 Z set 0 / 1 are done (stream ES)
    LABELLED = ("loss", "align", "occupancy", "score")     # the predict_stream outputs whose batches come with labels (a training engine)
    ALIGNED = ("align", "occupancy")     # ... whose kernel runs on stream 0 on the batch's own labels and lengths, like the loss

    def decode_ops(self, beam_width=10, merge_repeated=True, threshold=None, top_paths=1, lexicon=None, draws=8, sample_seed=0, quantile=0.5,
                   **lm_args):
        """predict_stream's decode outputs: name -> what builds decoding's description of its kernel with this engine's classes, frames
        and eps (nothing is validated before that is called).  Room for T - skip runs / phrases per sample, the most there can be: the
        count the kernel reports never exceeds what is downloaded."""
        Cn, skip, eps = self.spec.num_classes, int(self.spec.ctc["skip"]), float(self.spec.ctc["eps"])
        room = self.T - skip
        return {"argmax": lambda: decoding.argmax_op(Cn, skip),
                "segments": lambda: decoding.segments_op(Cn, skip, threshold, room),
                "beam": lambda: decoding.beam_op(Cn, skip, beam_width, merge_repeated, eps=eps),
                "beam_lm": lambda: decoding.beam_lm_op(Cn, skip, beam_width=beam_width, top_paths=top_paths, eps=eps, **lm_args),
                "lexicon": lambda: decoding.lexicon_op(Cn, skip, lexicon, cap=room, eps=eps, **lm_args),
                "sample": lambda: decoding.sample_op(Cn, skip, draws, sample_seed, eps=eps),
                "align": lambda: decoding.align_op(Cn, skip, return_path=True, eps=eps),
                "occupancy": lambda: decoding.occupancy_op(Cn, skip, quantile, eps=eps)}

    def predict_stream(self, batches, output="posteriors", train_phase=False, beam_width=10, merge_repeated=True, threshold=None,
                       lm=None, lm_end=None, alpha=1.0, beta=0.0, top_paths=1, decode="greedy", ignore=None, costs=(1, 1, 1), lexicon=None,
                       draws=8, sample_seed=0, quantile=0.5):
        """Batches of an inference / validation run are independent of each other: this generator keeps two of them in flight.
        Batch n + 1 is uploaded (copy stream) and runs its encoder pass (stream ES, into the other FEAT buffer) beside batch n's
        fusion layer / head / decode kernels (stream 0) and beside the download of batch n - 1's result (its own stream, into
        pinned host memory); the host only ever waits for the result it is about to hand out.  What the reference does with
        predict_generator over the whole set (sequence_decoding.py:118-127) and with the validation loop of every epoch
        (multimodal.py:264-269), one blocking batch at a time.

        batches: iterable of input dicts {stream name: (B, T, F)} - for output="loss", "align", "occupancy" and "score" of tuples (inputs, labels,
        input_length, label_length).  Yields, in order, per batch:
          "posteriors"  P (B, T, C) float32                  (learning phase 0 unless train_phase)
          "argmax"      (best (B, T - skip) int32, prob (B, T - skip) float32): mgr_frame_argmax on the device, the (B, T, C)
                        posteriors never travel to the host (decoding.confidence_filter_collapse does the rest)
          "beam"        (paths: list of B label lists, log-probabilities (B,) float64): mgr_ctc_beam_search on the device
          "beam_lm"     (paths, score (B,) or (B, top_paths) float64, logp_ctc likewise): mgr_ctc_beam_search_lm on the device - the
                        beam search with the label bigram lm / lm_end (weights alpha, beta) and top_paths hypotheses per sample, shaped
                        as decoding.beam_search_lm_decode returns them; the two tables are uploaded once per call, not per batch
          "lexicon"     (segments: list of B lists of (phrase, first_frame, last_frame, confidence), score (B,) float64, logp (B,)
                        float64): mgr_ctc_lexicon_decode on the device - the best phrase sequence over `lexicon` (whatever
                        decoding.compile_lexicon takes) with the phrase bigram lm (G + 1, G) / lm_end (G + 1,) weighted alpha, beta,
                        shaped as decoding.lexicon_decode returns them; the tables are uploaded once per call, and the per-sample
                        result arrays are all that travels back
          "loss"        per-sample CTC losses (B,) float32  (a training engine; learning phase as train_phase)
          "segments"    list of B lists of (label, first_frame, last_frame, confidence): mgr_greedy_segments(threshold) on the device
                        where "argmax" runs mgr_frame_argmax - the greedy decode with its frame positions (decoding.greedy_segments)
          "align"       (segments: list of B lists of (label, first_frame, last_frame, confidence), logp (B,) float64, path
                        (B, T - skip) int32): mgr_ctc_align of each sample's labels to its posteriors (a training engine, like "loss")
          "occupancy"   (segments: list of B lists of (label, first_frame, last_frame, confidence, occupancy), logp (B,) float64):
                        mgr_ctc_occupancy at `quantile` where "align" runs mgr_ctc_align - the posterior extents of each sample's labels
                        (decoding.posterior_align of the posteriors), in the engine's CTC workspace
          "score"       (loss (B,) float32, dist (B,) int32, counts (B, 4) int32 = (H, S, D, I), lens (B, 2) int32 = (m, n)): the CTC
                        loss exactly as "loss" computes it and, on the output stream, the decode kernel of decode = "greedy"
                        (mgr_greedy_segments with threshold) | "beam" | "beam_lm" (beam_width, lm, ... as above, one path) followed
                        by mgr_edit_distance of its device output against the batch's labels with costs = (sub, del, ins), both
                        sides without the labels in ignore (None: the blank, which the greedy decode keeps).  36 bytes per sample
                        travel to the host, no label sequence does (a training engine, like "loss")
          "rescore"     (logp (B, K) float64, n_lab (B, K) int32): mgr_ctc_rescore on the device - the CTC log-likelihood, summed over all
                        alignments, of K hypotheses per sample (decoding.ctc_scores of the posteriors).  Batches are tuples
                        (inputs, hyp (B, K, Lh) int32 padded -1, hyp_len (B, K) int32, -1 = no hypothesis) as decoding.pack_nbest lays
                        them out - with `lexicon` the entries are phrase ids -; K and Lh are those of the first batch.  The hypothesis
                        arrays go up through pinned double buffers on the output stream; an inference-only engine will do
          "sample"      (paths: per sample the list of its unique sampled labellings in order of first occurrence, counts: per sample
                        the number of draws that gave each): mgr_ctc_sample_paths on the device - `draws` (1 .. 32) alignments per
                        sample drawn from the posteriors, collapsed and merged (decoding.sample_hypotheses of the
                        posteriors).  The i-th batch of the stream draws with seed (sample_seed + i) mod 2^64; an inference-only
                        engine will do
        Results are bit-identical to the one-batch-at-a-time calls (predict / loss_on_batch): same kernels, same order per batch.
        A batch whose input dict carries "seq_length"  is computed as each sample alone at its own length: its posteriors
        are zero at t >= len, the outputs that take an input length decode len - skip frames (the labelled ones the input_length
        given, checked against that), "argmax" marks the frames past it -1 / 0, and "segments" / "score" with the greedy decode -
        whose kernel takes no length - refuse it."""
        sp, dev, B, T = self.spec, self.dev, self.B, self.T
        Cn, skip, eps = sp.num_classes, int(sp.ctc["skip"]), float(sp.ctc["eps"])
        # ("score" decodes one path; top_paths is read for "beam_lm" alone)
        ops = self.decode_ops(beam_width, merge_repeated, threshold, top_paths if output == "beam_lm" else 1, lexicon, draws, sample_seed,
                               quantile, lm=lm, lm_end=lm_end, alpha=alpha, beta=beta)
        if output not in ("posteriors", "loss", "score", "rescore") + tuple(ops):
            raise ValueError("unknown output %r" % (output,))
        labelled = output in self.LABELLED
        hypo = output == "rescore"
        if hypo:      # (K and the row width size the buffers below: the first batch is looked at before anything is enqueued)
            rest = iter(batches)
            head = next(rest, None)
            if head is None:
                return
            batches = itertools.chain([head], rest)
            hshape = tuple(int(v) for v in np.shape(head[1]))
            if len(hshape) != 3 or hshape[0] != B or np.shape(head[2]) != hshape[:2]:
                raise ValueError("output='rescore' takes batches (inputs, hyp (%d, K, Lh), hyp_len (%d, K)), got hyp %s / hyp_len %s"
                                 % (B, B, hshape, np.shape(head[2])))
        if labelled and self.inference_only:
            raise ValueError("output=%r needs a training engine (labels%s)" % (output, "" if output == "align" else ", CTC workspace"))
        self._bind()
        if self._prefetched is not None:     # a pipelined training encoder pass is in flight: let it finish, then discard it
            dev.wait(0, self.ES)
            self._prefetched = None
        dev.sync()                           # (nothing of an earlier call may still use the buffers the pipeline cycles through)
        ring = self._feat_ring
        ES, OUT = (self.ES if len(ring) > 1 else 0), self.LOSS_STREAM
        st = self.__dict__.setdefault("_stream_bufs", {})

        def bufs(key, make):
            if key not in st:
                st[key] = make()
            return st[key]

        def sets(n, make, shapes):
            return [tuple(make(*s) for s in shapes) for _ in range(n)]

        # two P buffers: the decode kernels / the download of batch n read one on their own stream while the head of batch n + 1
        # writes the other
        pring = bufs("pring", lambda: [self.P, self.mem.empty((B, T, Cn))])
        name = {"greedy": "segments", "beam": "beam", "beam_lm": "beam_lm"}.get(decode) if output == "score" else output
        if output == "score":
            if name is None:
                raise ValueError("unknown decode %r for output='score'" % (decode,))
            if T - skip > decoding.EDIT_MAX_LEN or self.Lmax > decoding.EDIT_MAX_LEN:
                raise ValueError("T - skip = %d or Lmax = %d above the %d labels mgr_edit_distance compares"
                                 % (T - skip, self.Lmax, decoding.EDIT_MAX_LEN))
            ecosts = decoding.check_costs(costs)
            emask = decoding.ignore_mask((Cn - 1,) if ignore is None else ignore)
        elif output == "beam_lm" and not 1 <= int(top_paths) <= int(beam_width):          # (before anything is allocated for it; the library checks again)
            raise ValueError("top_paths %d out of [1, beam_width = %d]" % (int(top_paths), int(beam_width)))
        elif output == "lexicon" and lexicon is None:
            raise ValueError("output='lexicon' needs a lexicon")
        op, host_labels, dil = None, {}, None
        if hypo:
            op = decoding.rescore_op(Cn, skip, lexicon, eps)
        elif name in ops:
            op = ops[name]()
        if op is not None:
            # The op's device outputs, workspace and tables, each cached under what sizes it - so "segments" and "score" with the greedy
            # decode, or "beam_lm" and "score" at one path, share them.  One set of outputs: decode, comparison and copies of a batch are
            # consecutive on the output stream - but two for "align" / "occupancy", which run on stream 0: one per output slot, like the losses below
            Lq = hshape[1] if hypo else self.Lmax       # ("rescore": K travels where the labelled ops get Lmax)
            shapes = op.outputs(B, T, Lq)
            dring = bufs((name, "out", shapes), lambda: [tuple(sh if sh is None else self.mem.empty(*sh) for sh in shapes)
                                                        for _ in range(2 if name in self.ALIGNED else 1)])
            nbytes = op.ws_bytes(self.lib, B, T, Lq) if op.ws_bytes else None
            if name == "occupancy":     # (the loss's layout, on the loss's stream: the engine's CTC workspace serves it)
                ws = self.ws_ctc
            else:
                ws = None if nbytes is None else bufs((name, "ws", nbytes), lambda: self.mem.bytes(nbytes))
            # (the tables are uploaded once per call, not per batch)
            tables = [t if t is None else bufs((name, "table", k, t.shape), lambda: self.mem.empty(t.shape, t.dtype)).upload(t)
                      for k, t in enumerate(op.tables)]
            dil = None          # ("align" / "occupancy" read the lengths that came with the labels)
            if op.uses_len and name not in self.ALIGNED:
                dil = bufs("dil", lambda: self.mem.empty((B,), np.int32)).upload(np.full(B, T - skip, np.int32))
            if hypo:      # one device set (upload and kernel of a batch are consecutive on the output stream), two pinned ones
                hspec = [(hshape, np.int32), (hshape[:2], np.int32)]
                dhyp = bufs(("rescore", "hyp", hshape), lambda: sets(1, self.mem.empty, hspec))[0]
                phyp = bufs(("rescore", "hyp pinned", hshape), lambda: sets(2, dev.pinned, hspec))
        # per output slot o: the pinned arrays a result arrives in, and the device arrays src(o) they are copied from
        if output == "posteriors":
            pins, src = bufs("P", lambda: sets(2, dev.pinned, [((B, T, Cn), np.float32)])), lambda o: (pring[o],)
        elif output in ("loss", "score"):
            # one device buffer per output slot, like pring: batch i's copy (its own stream, behind EV_FUSED only) must not find
            # batch i + 1's losses in the buffer - stream 0 waits for EV_OUT[o] of batch i - 2 before it reuses slot o
            lring = bufs("lring", lambda: [self.loss_b, self.mem.empty((B,))])
            dscore = ()
            if output == "score":
                dscore = bufs("dscore", lambda: sets(1, self.mem.empty, [((B,), np.int32), ((B, 4), np.int32), ((B, 2), np.int32)]))[0]
            pins = bufs(output, lambda: sets(2, dev.pinned, [((B,), np.float32)] + [(d.shape, d.dtype) for d in dscore]))
            src = lambda o: (lring[o],) + dscore
        else:
            pins = bufs((name, "pinned", shapes), lambda: sets(2, dev.pinned, [sh for sh in shapes if sh is not None]))
            src = lambda o: [d for d in dring[o % len(dring)] if d is not None]     # (the one set, or the set of slot o)

        spin = bufs("status16", lambda: [dev.pinned((16,), np.uint32) for _ in range(2)])

        # per-sample lengths: batch i -> its lengths on the host, from its upload until its result is handed out
        host_lens = {}
        greedy = name == "segments"       # (mgr_greedy_segments takes no input length, and its confidence filter is not local in time)

        def collect(i):
            o = i & 1
            dev.event_sync(self.EV_OUT[o])
            if output in ops or hypo:
                r = op.result(*pins[o], *host_labels.pop(i, ()))
            else:
                r = pins[o] if output == "score" else pins[o][0]
            bl = host_lens.pop(i, None)
            if bl is not None and output == "argmax":
                # (the frame argmax takes no input length: the frames past len - skip, the argmax of zero rows, are marked absent)
                best, prob = (m.copy() for m in r)
                for b, nfr in enumerate(seqlen.frames(bl, skip)):
                    best[b, nfr:], prob[b, nfr:] = -1, 0.0
                r = (best, prob)
            # the pinned buffers are reused two batches later: every array handed out is a copy (the lists hold Python numbers)
            own = lambda m: m.copy() if isinstance(m, np.ndarray) else m
            r = tuple(own(m) for m in r) if isinstance(r, tuple) else own(r)
            # the status block of THIS batch's pass travels with its result (no extra synchronisation): the samples whose hidden
            # state went NaN / Inf in it get NaN scores and no labels - not plausible numbers, and not every later batch
            return self._end_pass(spin[o].copy(), r, what="batch %d of the pipelined run" % i)

        # Depth-1 projections of the NEXT batch on stream 0 (round 4).  The cycle of the pipeline is the encoder stream's chain
        # (depth-1 projections 4.4 | depth-1 scans 8.2 | depth-2 projections 11.0 | depth-2 scans 8.3 ms at config F) while stream 0
        # idles two thirds of it; with two sets of depth-1 gate pre-activation buffers the projections of batch i + 1 are enqueued
        # on stream 0 in front of batch i's fusion pass - they run beside batch i's encoder scans - and the encoder stream's chain
        # loses them.  Same kernels, same inputs per batch: results stay bit-identical to the one-batch-at-a-time calls.
        two_stage = len(ring) > 1 and max(len(s_["layers"]) for s_ in sp.streams) >= 2
        z1 = None
        if two_stage:
            z1 = bufs("z1", lambda: [{s_["name"]: (self.mem.empty((B, T, 4 * s_["layers"][0]["H"])), self.mem.empty((B, T, 4 * s_["layers"][0]["H"])))
                                      for s_ in sp.streams} for _ in range(2)])

        started = [0]
        # launch numbers of the depth-1 / depth-2 scan launches of the batch in Z set 0 / 1, as the launches themselves report them
        # (mgr_scan_launch_opts.seq_out: round 5 predicted them from the context's counter, which another engine on the same Device or
        # a launch that does not enter the ledger made wrong - and every wait then ran into its bound)
        scan_seq = np.zeros((2, 2), np.uint32)

        def wait_resident(seq, us):
            if int(seq) not in (0, _capi.SEQ_NONE):     # (no persistent launch: nothing to wait for)
                dev.call("mgr_stream_wait_resident", C.c_uint(int(seq)), int(us))

        def start_encoders(i, item):
            """Upload batch i and enqueue its noise / depth-1 projections on stream 0 (two_stage), or nothing yet; returns the
            generator that enqueues the rest of its encoder pass on ES."""
            inputs = item[0] if labelled or hypo else item
            bl = self._check_lengths(inputs, item[2] if labelled else None)      # (raises before anything of this batch is enqueued)
            if bl is not None:
                if greedy:
                    raise ValueError("the greedy segment decode takes no input length (its confidence filter counts frames over the "
                                     "whole sequence): with %s use the argmax, beam or lexicon outputs" % seqlen.KEY)
                host_lens[i] = bl
            f = i % len(ring)
            first = 0 if two_stage else ES
            self._upload_inputs(inputs, None, train_phase, stream=first)
            self._xin_user[self._xin_slot] = 1 << 60       # (its readers are known by event, not by a loss read-back)
            scan_seq[i & 1, :] = 0
            gen = self._encoder_phases(train_phase, None, ring[f], ES, self.rng_step + (i - started[0]),
                                       first_stream=0 if two_stage else None, z_first=z1[i & 1] if two_stage else None,
                                       seq_words={k: scan_seq.ctypes.data + 4 * (2 * (i & 1) + k) for k in range(2)})
            if two_stage:
                dev.stream(0)
                dev.wait_event(0, self.EV_D1S[i & 1])       # the depth-1 scans that read this Z set two batches ago
                if i >= 1 and self.schedule.resident_wait_us > 0:
                    # ... and not beside the previous batch's depth-2 projection GEMMs on ES (GEMM beside GEMM: the sum of both), but
                    # beside its depth-2 SCANS, whose launch follows its depth-1 scan launch (bounded wait: placement only)
                    wait_resident(scan_seq[(i - 1) & 1, 1], 5 * self.schedule.resident_wait_us)
                tag = next(gen)                             # noise + depth-1 projections -> stream 0
                assert tag == ("projected", 0)
                dev.stream(0)
                dev.record(self.EV_D1P[i & 1])
            return gen

        def finish_encoders(i, gen):
            f = i % len(ring)
            dev.stream(ES)
            dev.wait_event(ES, self.EV_FUSED[f])            # the fusion pass that read this FEAT buffer two batches ago
            dev.wait_event(ES, self.EV_OUT[i & 1])          # ... and the copy of that batch's status block: this batch's pass
            self._begin_pass(i & 1)                         # zeroes it (stream ES) and reports into it from here on
            if two_stage:
                dev.wait_event(ES, self.EV_D1P[i & 1])
            for tag in gen:
                if two_stage and tag == ("scanned", 0):
                    dev.stream(ES)
                    dev.record(self.EV_D1S[i & 1])
            dev.stream(ES)
            dev.record(self.EV_ENC[f])

        n = 0
        try:
            it = iter(batches)
            nxt_item = next(it, None)
            if nxt_item is not None:
                gen = start_encoders(0, nxt_item)
                if two_stage:
                    finish_encoders(0, gen)
            i = -1
            while nxt_item is not None:
                i += 1
                item = nxt_item
                o, f = i & 1, i % len(ring)
                if not two_stage:
                    # ---- batch i's encoder pass (stream ES), beside what stream 0 still does for batch i - 1
                    finish_encoders(i, gen)
                nxt_item = next(it, None)
                if two_stage:
                    # ---- batch i + 1: upload, depth-1 projections on stream 0 (in front of batch i's fusion pass), and the REST of its
                    # encoder pass on ES right away - so that the fusion pass below can be ordered behind the residency of that pass's
                    # first scan launch
                    if nxt_item is not None:
                        finish_encoders(i + 1, start_encoders(i + 1, nxt_item))
                elif nxt_item is not None:
                    gen = start_encoders(i + 1, nxt_item)
                # ---- fusion layer, head, decode / loss kernels of batch i (stream 0)
                dev.stream(0)
                dev.wait_event(0, self.EV_ENC[f])
                if two_stage and nxt_item is not None and self.schedule.resident_wait_us > 0:
                    # Batch i's encoder pass ends and batch i + 1's depth-1 scans start at the same instant on ES: fusion projection
                    # GEMMs released at that instant race the scan's workgroups for the CUs and the scan runs at half speed for its
                    # whole life (13.1 instead of 8.3 ms: profiles/r04_predict_timeline.txt) - they wait until it is resident
                    wait_resident(scan_seq[(i + 1) & 1, 0], self.schedule.resident_wait_us)
                dev.wait_event(0, self.EV_OUT[o])               # batch i - 2's decode / download read the P buffer this pass overwrites
                if labelled:
                    self._upload_labels(item[1], item[2], item[3])
                if output in self.ALIGNED:
                    host_labels[i] = (self._lab_pin[self._lab_slot][0].copy(), np.asarray(item[3]).reshape(B).astype(np.int32))
                self.P = pring[o]
                self._bind(self._pass_status[o])        # (batch i + 1's encoder pass, enqueued above, bound the other block)
                self._enqueue_fusion_head(train_phase, None, ring[f], self.rng_step + (i - started[0]))
                dev.stream(0)
                if output in self.ALIGNED:
                    op.launch(dev, self.P, self.ilen_d, dring[o], tables, ws, self.labels_d, self.llen_d)
                elif labelled:
                    dev.call("mgr_ctc_loss_grad", self.P, self.labels_d, self.ilen_d, self.llen_d, B, T, Cn, self.Lmax, skip, Cn - 1,
                             eps, 1.0, lring[o], 0, self.ws_ctc, self.ws_ctc.nbytes)
                if output in ("loss",) + self.ALIGNED:       # ("score" reads the labels again on the output stream below)
                    dev.record(self.EV_LAB[self._lab_slot])
                    self._lab_user[self._lab_slot] = 1 << 60
                dev.record(self.EV_FUSED[f])
                # ---- decode kernels and the way back to pinned host memory: their own stream, beside batch i + 1's fusion layer
                dev.stream(OUT)
                dev.wait_event(OUT, self.EV_FUSED[f])
                dil_i = dil
                if dil is not None and i in host_lens:
                    # this batch's own input lengths, len - skip (pinned set o: read last by batch i - 2's copy, like phyp below; one
                    # device array: upload and kernel of a batch are consecutive on this stream)
                    dlen = bufs("dil seq", lambda: self.mem.empty((B,), np.int32))
                    plen = bufs("dil seq pinned", lambda: [dev.pinned((B,), np.int32) for _ in range(2)])
                    plen[o][...] = seqlen.frames(host_lens[i], skip)
                    dev.h2d_async(dlen, plen[o])
                    dil_i = dlen
                if hypo:
                    # (pinned set o was last read by batch i - 2's copies, behind EV_OUT[o], which collect(i - 2) has waited for)
                    if np.shape(item[1]) != hshape or np.shape(item[2]) != hshape[:2]:
                        raise ValueError("batch %d: hyp %s / hyp_len %s, the first batch had %s" % (i, np.shape(item[1]), np.shape(item[2]), hshape))
                    for pin, d, a in zip(phyp[o], dhyp, item[1:3]):
                        pin[...] = a
                        dev.h2d_async(d, pin)
                    host_labels[i] = (None, None)
                    op.launch(dev, pring[o], dil_i, dring[0], tables, ws, *dhyp)
                elif output == "sample":
                    op.launch(dev, pring[o], dil_i, dring[0], tables, ws, seed=int(sample_seed) + i)
                elif op is not None and output not in self.ALIGNED:
                    op.launch(dev, pring[o], dil_i, dring[0], tables, ws)
                if output == "score":
                    dev.call("mgr_edit_distance", dring[0][op.hyp[0]], dring[0][op.hyp[1]], B, T - skip, self.labels_d, self.llen_d, B, self.Lmax,
                             None, None, B, ecosts[0], ecosts[1], ecosts[2], emask, dscore[0], dscore[1], dscore[2], None, None, None, 0)
                    dev.record(self.EV_LAB[self._lab_slot])        # the labels' last reader of this batch is on this stream
                    self._lab_user[self._lab_slot] = 1 << 60
                for pin, d in zip(pins[o], src(o)):
                    dev.d2h_async(pin, d)
                dev.d2h_async(spin[o], self._pass_status[o])
                dev.record(self.EV_OUT[o])
                dev.stream(0)
                n = i + 1
                if i >= 1:
                    yield collect(i - 1)
            if n >= 1:
                yield collect(n - 1)
        finally:
            self.P = pring[0]
            if train_phase:
                self.rng_step += n          # (one draw of randomness per batch, as the one-batch-at-a-time calls)
            dev.stream(0)
            dev.sync()
            self._bind()

    def _upload_labels(self, labels, input_length, label_length):
        lab = np.asarray(labels)
        lab = np.where(np.isfinite(lab), lab, -1).astype(np.int32).reshape(self.B, -1)
        if lab.shape[1] != self.Lmax:
            if lab.shape[1] > self.Lmax:
                raise ValueError("label rows longer (%d) than Lmax=%d" % (lab.shape[1], self.Lmax))
            lab = np.concatenate([lab, -np.ones((self.B, self.Lmax - lab.shape[1]), np.int32)], axis=1)
        dev = self.dev
        slot = self._lab_slot ^ 1
        dev.stream(self.COPY_STREAM)
        if self._lab_user[slot] > self._synced_step:       # see _upload_inputs
            dev.wait_event(self.COPY_STREAM, self.EV_LAB[slot])
        labels_d, ilen_d, llen_d = self._lab_ring[slot]
        plab, pil, pll = self._lab_pin[slot]    # (the staging set is reused together with the device set: same ordering)
        if self._lab_copied[slot]:              # (... and refilled by the host only once its last copies are done: _upload_inputs)
            dev.event_sync(self.EV_LAB_COPIED[slot])
        plab[...] = lab
        pil[...] = np.asarray(input_length).reshape(self.B)
        pll[...] = np.asarray(label_length).reshape(self.B)
        dev.h2d_async(labels_d, plab)
        dev.h2d_async(ilen_d, pil)
        dev.h2d_async(llen_d, pll)
        dev.record(self.EV_LAB_COPIED[slot])
        self._lab_copied[slot] = True
        dev.wait(0, self.COPY_STREAM)          # the CTC kernel runs on stream 0
        self._lab_slot = slot
        self._lab_user[slot] = 1 << 60
        self.labels_d, self.ilen_d, self.llen_d = labels_d, ilen_d, llen_d
        dev.stream(0)

    def loss_on_batch(self, inputs, labels, input_length, label_length, rand=None, train_phase=True):
        """Per-sample CTC loss (validation inside fit_generator: learning phase stays 1, multimodal.py:66)."""
        self._check_lengths(inputs, input_length)
        self._upload_inputs(inputs, rand, train_phase)
        self._upload_labels(labels, input_length, label_length)
        blk = self._begin_pass()
        self._forward(train_phase, rand)
        sp = self.spec
        self.dev.call("mgr_ctc_loss_grad", self.P, self.labels_d, self.ilen_d, self.llen_d, self.B, self.T,
                      sp.num_classes, self.Lmax, int(sp.ctc["skip"]), sp.num_classes - 1, float(sp.ctc["eps"]),
                      1.0, self.loss_b, 0, self.ws_ctc, self.ws_ctc.nbytes)
        lb = self.loss_b.download()
        return self._end_pass(blk.download(), lb)

    def train_step(self, inputs, labels, input_length, label_length, rand=None, apply_update=True, next_inputs=None,
                   after_next_inputs=None):
        """One optimizer step (Keras train_on_batch).  Returns the mean CTC loss of the local batch.
        next_inputs (optional): the inputs of the FOLLOWING call; when the encoders are frozen their pass for that batch
        is overlapped with this step's fusion / BPTT / Adam work (bit-identical results); after_next_inputs: those of the call
        after that (the encoder stream gets the first part of its pass a call early).
        inputs["seq_length"] ((B,) or (B, 1) integers in [0, T]), in any of the three dicts: the batch's per-sample frame
        counts - the step computes what each sample gives alone at its own length, whatever the padding holds.  Needs
        input_length[b] <= max(0, seq_length[b] - skip); ValueError before anything is enqueued otherwise (seqlen.check_batch)."""
        self.enqueue_train_step(inputs, labels, input_length, label_length, rand, apply_update,
                                prefetch_next=next_inputs is not None, next_inputs=next_inputs,
                                prefetch_after_next=next_inputs is not None and after_next_inputs is not None,
                                after_next_inputs=after_next_inputs)
        return self.read_loss()

    LOSS_STREAM = 6   # (pipelined inference: decode / result copies)
    PG_STREAM = 4     # (Schedule.param_grads_two_streams: the second direction's parameter-gradient chain)
    EV_LOSS = 52      # the loss and the scan status of the step enqueued last have reached their page-locked host words

    def read_loss(self, local=False):
        """Mean CTC loss of the step enqueued last: waits for the event behind the loss kernels and their read-back - not for
        the gradient GEMMs / optimizer queued behind them - so the host can enqueue the next step early.
        Data parallel (world > 1): the mean over the GLOBAL batch, the same number on every rank - it arrives with the gradient
        all-reduce, i.e. at the END of the step (read_global_loss); local=True returns this rank's own mean without that wait
        (a training loop that wants to keep the host ahead of the device reads the global loss one step late)."""
        dev = self.dev
        dev.event_sync(self.EV_LOSS)
        v = float(self.loss_host[0])
        self.last_risk = self.last_ctc_loss = self.last_entropy = None
        if isinstance(self._loss_parts, tuple):      # an entropy-regularised step: [0] the mean CTC loss, [1] the mean entropy
            self.last_ctc_loss, self.last_entropy = v, float(self.loss_host[1])
            v = self.last_ctc_loss - self._loss_parts[1] * self.last_entropy
        elif self._loss_parts is not None:    # a minimum-risk step: [0] the mean CTC loss (0 where it was not computed), [1] the mean risk
            self.last_ctc_loss, self.last_risk = v, float(self.loss_host[1])
            v = self.last_risk + self._loss_parts * self.last_ctc_loss
        step = self._step_id - 1
        self._synced_step = step
        self._check_scans(step=step, snapshot=self.status_host)   # raises if a persistent scan gave up: results would be garbage
        if not local and self.world > 1 and self._gloss_step[step & 1] == step:
            return self.read_global_loss(step)
        if self.nonfinite_seen:
            # a hidden state went NaN / Inf: in the reference every later op propagates the NaN into the loss.  Here a NaN
            # feature that input dropout happens to drop is SKIPPED by the dropout-aware kernels (no 0 x NaN), so the number
            # the device computed may look finite - report what the reference would report
            return float("nan")
        return v

    EV_GLOSS = (53, 54)   # the all-reduced (gate flag, loss sum) of step s has reached gloss_host[s & 1]

    def read_global_loss(self, step=None):
        """Mean CTC loss over the global batch of training step `step` (default: the one enqueued last), identical on every
        rank: (sum over ranks of the local means) / world, carried by the gradient all-reduce of that step.  NaN on EVERY rank
        when any rank's scans reported a non-finite state or gave up in that step (the all-reduced update-gate flag)."""
        step = self._step_id - 1 if step is None else int(step)
        slot = step & 1
        if self._gloss_step[slot] != step:
            raise ValueError("no all-reduced loss for step %d (not a data-parallel step, its update was not applied, or two "
                             "later steps have been enqueued since)" % step)
        self.dev.event_sync(self.EV_GLOSS[slot])
        flag, total = float(self.gloss_host[slot][0]), float(self.gloss_host[slot][1])
        return float("nan") if flag != 0.0 else total / self.world

    @property
    def can_pipeline(self):
        """Frozen encoders do not depend on the weights the step updates, so the encoder pass of step n+1 may run
        while step n's fusion layer / CTC / BPTT / Adam are in flight (the fusion config of the reference)."""
        sp = self.spec
        return bool(sp.fusion) and not any(s["trainable"] for s in sp.streams) and not self.inference_only

    ES = 5          # encoder stream when steps are pipelined
    EV_PREV = 40    # end of the previous step's fusion phase on stream 0 (its dW GEMMs read the other FEAT buffer)
    EV_FPROJ = 45   # this step's fusion projection GEMMs are done

    def enqueue_train_step(self, inputs, labels, input_length, label_length, rand=None, apply_update=True,
                           upload=True, prefetch_next=False, next_inputs=None, prefetch_after_next=False, after_next_inputs=None):
        """Enqueue one training step.  With prefetch_next (device-RNG training of a network whose encoders are frozen)
        the NEXT step's encoder pass is enqueued on a second stream into the other FEAT buffer right after this step's
        fusion work, and this step consumes the encoder pass enqueued by the previous call (Schedule).
        prefetch_after_next (round 5; the caller promises that the call after the next one comes, with prefetch_next, for
        after_next_inputs): the encoder stream also gets the first part of THAT batch's pass - up to its deepest projections - at
        the end of this call instead of at the start of the next one.  The next call can only be made once the host has this step's
        loss (the CTC kernel, half-way through the step): the encoder stream used to sit idle from the end of its deepest scan
        until then (0.9 - 3.9 ms per step in the traces of round 5)."""
        dev, sch, ES, depth = self.dev, self.schedule, self.ES, self.depth
        if self._augment is not None and rand is not None:
            raise ValueError("a training step with set_augment on was given `rand`: host-supplied randomness has no augmentation plan "
                             "(set_augment(None) first)")
        if upload:
            self._check_lengths(inputs, input_length, augment=self._augment is not None)
        for ahead_inputs in (next_inputs, after_next_inputs):
            self._check_lengths(ahead_inputs, augment=self._augment is not None)
        self._bind()
        pipelined = bool(prefetch_next and rand is None and self.frozen_fusion)
        # ---- 1. this step's encoder pass: the one the previous call prefetched, or its own
        have = self._prefetched
        if have is not None:
            stale = rand is not None or not self.can_pipeline
            if upload and self._prefetched_for is not None and inputs is not self._prefetched_for:
                stale = True   # the caller did not come back with the batch it announced
            if stale:
                dev.wait(0, ES)
                have = None
        self._prefetched = None
        # What the encoder stream was handed a call early (the first part of the pass of the batch after this one) is settled BEFORE
        # this step's FEAT buffer is chosen: when the caller did not come back as announced - another batch, a predict /
        # loss_on_batch in between that discarded the prefetched pass - the early generator is dropped and its claim on the other FEAT
        # buffer with it; choosing `cur` first put the NEXT batch's deepest scan on top of the buffer this step's deferred dW GEMMs read.
        # (A step without a prefetched pass always drops it: its own pass uses the encoder buffers the early part has written.)
        early, self._early_gen = self._early_gen, None
        early_words, self._early_words = self._early_words, None
        keep_early = have is not None and pipelined and self.can_run_free and (not upload or next_inputs is self._early_for)
        if early is not None and not keep_early:
            dev.wait(0, ES)
            self._feat_idx ^= 1        # (the generator toggled it when it was started; nothing of its pass has touched a FEAT buffer yet)
            early.close()
            early = None
        # ---- the layout of this call: what _build resolved (can_*), narrowed by what only the call knows
        # Round 6: a pipelined step WITHOUT a prefetched pass (the first step of a run, the step after a validation pass) runs its own
        # encoder pass on the ENCODER stream, in the fused forms - nothing of this step can run beside it anyway, and from here on the
        # call is a steady-state call: the next batch's pass follows on that stream at once, beside this step's trainable part, instead
        # of behind a whole in-line pass in the plain forms and a stream-wide wait.  The step itself is what it was: same kernels'
        # results, same order of randomness.
        own_on_es = have is None and pipelined and self.can_fuse and sch.first_pass_on_encoder_stream
        # (a call that runs its own encoder pass in line on stream 0 starts nothing ahead: that pass uses the encoder buffers)
        has_pass = have is not None or own_on_es
        defer = pipelined and self.can_defer
        ahead = pipelined and self.can_run_ahead and has_pass
        # Free-running encoder stream (Schedule.bptt_beside_deepest_scan): the next batch's encoder pass up to its deepest projections
        # is handed to the encoder stream BEFORE this step's fusion work is enqueued - it depends on nothing of this step, and the
        # host needs ~1-2 ms to enqueue the fusion layer and the head, during which that stream would sit idle
        runs_free = pipelined and self.can_run_free and has_pass     # (a kept early generator implies it)
        fresh = runs_free and early is None                          # ... and this call starts the next batch's pass itself
        # The fused forms of the encoder scans belong to every pass the encoder stream runs for a pipelined step (round 6: also the
        # passes of the first steps of a run, which round 5 ran in the plain form until a step had been announced two calls ahead)
        fused = pipelined and self.can_fuse and has_pass
        two = bool(runs_free and prefetch_after_next and sch.encoders_two_ahead)
        self._since_fresh = 0 if (fresh or not runs_free) else self._since_fresh + 1
        free_words = early_words if early is not None else {}     # depth k -> the word the next pass's scan of depth k reports into
        new_words = {}                                            # ... of the pass of the batch after next
        lay = PLAIN._replace(beside_scans=pipelined)
        if fused:
            # Persistent launches of this call, in host order: fusion scan, BPTT, the next batch's deepest scan and - when the batch
            # after next is announced - its depth-1 scan.  The encoder scans take the FUSED form (an argument of their launch), and
            # each hands its launch number to the word the residency wait of the recurrence that runs BESIDE it polls (the waits are
            # enqueued first).  Steady state: the fusion scan beside the next batch's deepest scan, the BPTT beside the depth-1 scan
            # of the batch after next.  A call that starts the next batch's pass itself (fresh: the first steps of a run): the
            # fusion scan beside that pass's depth-1 scan, the BPTT beside its deepest scan.
            if fresh:
                free_words[0] = self._new_seq_word()
            wx = free_words[depth - 1] = self._new_seq_word()
            wy = None
            if two:
                wy = new_words[0] = self._new_seq_word()
            # (the call right after a fresh one: the encoder stream is still a phase behind - the deepest scan this call enqueues
            #  starts milliseconds after the fusion scan is ready, and the wait for it ran into its bound, once per run: no wait)
            late = (not fresh) and self._since_fresh == 1
            gates = (free_words[0], wx) if fresh else ((None, wy) if late else (wx, wy))
            lay = StepLayout(True, sch.fused_wide_tiles, _capi.SCAN_FORM_FUSED,
                             _capi.SCAN_FORM_FUSED_ANY if sch.fusion_scan_fused else _capi.SCAN_FORM_AUTO, *gates)
            self._gate_log.append((self._step_id, "fresh" if fresh else "steady", gates))
        if have is not None:
            cur = have
            # this step's encoder pass (enqueued by the previous call) must be complete: the event behind its deepest scan - not
            # everything the encoder stream has been handed since (round 5 waited for the whole stream: in steady state the first part of
            # the NEXT batch's pass, queued behind it, is done by then anyway; in the first steps of a run it is not, and the second step
            # started 7 ms late)
            dev.wait_event(0, self.EV_ENC[self._feat_ring.index(cur)])
        elif own_on_es:
            dev.wait(ES, 0)        # (the encoder buffers / this FEAT buffer may still be read by what stream 0 has queued)
            if upload:
                self._upload_inputs(inputs, None, True, stream=ES)
                self._xin_user[self._xin_slot] = self._step_id     # (this step reads them; frozen encoders: in this pass only)
            cur = self._feat_ring[self._feat_idx]
            self._enqueue_encoders(True, None, cur, ES, self.rng_step, augment=True, scan_form=lay.enc_scan_form)
            dev.wait(0, ES)
        else:
            if upload:
                self._upload_inputs(inputs, rand, True)
            cur = self._feat_ring[self._feat_idx]
            self._enqueue_encoders(True, rand, cur, 0, self.rng_step, augment=True, scan_form=lay.enc_scan_form)
        if upload:
            self._upload_labels(labels, input_length, label_length)
        if pipelined:
            # the other FEAT buffer was last read by the previous step's fusion phase (its dW GEMMs, queued on stream 0)
            if ahead:
                dev.stream(0)
                dev.record(self.EV_PREV)   # only the launch that WRITES that buffer (the deepest scan) has to wait for it
            else:
                dev.wait(ES, 0)
        free_gen = early      # (its first part was enqueued at the end of the previous call)
        if fresh:
            free_gen = self._next_encoders_free(next_inputs, self.rng_step + 1, self._step_id + 1, lay.enc_scan_form, seq_words=free_words)
            next(free_gen)
        # ---- 2., 3. fusion layer, head, CTC, loss read-back point, backward
        finish = self._enqueue_trainable_part(cur, rand, lay, defer, pipelined and self.can_hold_bptt, not has_pass, apply_update)

        # ---- 4. parameter gradients + optimizer, and (pipelined) the next step's encoder pass
        if not pipelined:
            finish()
        elif free_gen is None:
            self._enqueue_next_encoders(next_inputs, finish, defer, ahead, lay.enc_scan_form)
        else:
            def start_after_next(**kw):
                # the first part of the pass of the batch AFTER the next one (rng_step / _step_id were advanced above)
                self._early_gen = self._next_encoders_free(after_next_inputs, self.rng_step + 1, self._step_id + 1, lay.enc_scan_form,
                                                           seq_words=new_words, **kw)
                self._early_words = new_words
                next(self._early_gen)
            if two and self.Z1buf:
                # (Schedule.depth1_proj_ahead, which Z1buf exists for) its depth-1 projections in front of the next batch's deepest
                # scan, the rest of its first part at the end of this call
                free_gen.send((finish, lambda: start_after_next(split_first=True)))
                next(self._early_gen)
            else:
                free_gen.send(finish)
                if two:
                    start_after_next()
        dev.stream(0)

    def _mode_cfg(self, setter, cfg, what, what_parallel, kind=None, defaults=None):
        """What set_risk / set_entropy / set_augment refuse alike, before anything of the mode set before is touched (a cfg that is
        refused leaves the mode as it was): a communicator, an inference-only engine, keys that `defaults` does not have.  Returns
        cfg over defaults."""
        if self.comm is not None:
            raise NotImplementedError("%s is single-GPU: data-parallel %s is not implemented" % (what, what_parallel))
        if self.inference_only:
            raise ValueError("%s on an inference-only engine" % setter)
        if defaults is None:
            return cfg
        unknown = set(cfg) - set(defaults)
        if unknown:
            raise ValueError("unknown %s settings %s (known: %s)" % (kind, sorted(unknown), sorted(defaults)))
        return dict(defaults, **cfg)

    RISK_DEFAULTS = dict(top_paths=8, beam_width=16, ctc_weight=0.1, costs=(1, 1, 1), post_scale=1.0, max_labels=None, source="beam",
                         sample_seed=None)
    # the kernel seed of the sampled hypothesis set of the step enqueued last (source="sample"; None: no such step yet)
    last_sample_seed = None
    # set where a step is ENQUEUED, never by set_risk: the step enqueued last - the one whose loss read_loss reads, loss_host holds
    # no other - was a minimum-risk step with this ctc_weight (None: a plain step)
    _loss_parts = None
    last_risk = last_ctc_loss = None

    def set_risk(self, cfg):
        """Minimum-risk fine-tuning: with cfg - a dict over RISK_DEFAULTS - the head of a training step is the separate
        calls mgr_head_fwd_bwd equals, with the expected edit distance over the step's own N-best list added to the loss:
        loss = mean risk + ctc_weight * mean CTC loss.  The N-best list is mgr_ctc_beam_search_lm's (no tables, top_paths, beam_width)
        on the train-phase posteriors, its risks mgr_edit_distance's (costs) against the step's labels, the gradient
        mgr_ctc_risk_grad's (post_scale; hypotheses of more than max_labels labels - default min(255, max(2 Lmax, 16)) - are not
        scored; the risk workspace grows with it: B K T 2 (max_labels + 1) 8 bytes, 1.03 GiB at config F's default of 70).  read_loss
        returns the combined loss and leaves the parts in last_risk / last_ctc_loss.  None: back to the one mgr_head_fwd_bwd call; the
        mode's buffers are freed.  source="sample" (DESIGN 9o): the hypothesis set is not searched for but SAMPLED - mgr_ctc_sample_paths
        in the search's place, top_paths (1 .. 32) draws per sample, beam_width not read, no search workspace or tables held; the unique
        sampled labellings are the slots, weighted as the N-best list's are (the counts take no part).  The step's kernel seed comes from
        sample_seed (None: the engine's seed) and the step counter as the head dropout's does, with a stream constant of its own, and is
        left in last_sample_seed.  A cfg that is refused leaves the mode as it was.  The loss of a step
        enqueued before the call is still read as that step's.  Everything behind the head is the same either way."""
        if cfg is None:
            self._release_risk()
            return
        if self._entropy is not None:
            raise ValueError("set_risk with the entropy mode on: the two training modes are not combined (set_entropy(None) first)")
        cfg = self._mode_cfg("set_risk", cfg, "minimum-risk training", "risk training", "risk", self.RISK_DEFAULTS)
        sp, lib, B, T = self.spec, self.lib, self.B, self.T
        Cn, skip = sp.num_classes, int(sp.ctc["skip"])
        K, W = int(cfg["top_paths"]), int(cfg["beam_width"])
        sampled = cfg["source"] == "sample"
        if cfg["source"] not in ("beam", "sample"):
            raise ValueError("source = %r: 'beam' or 'sample'" % (cfg["source"],))
        if sampled:
            if not 1 <= K <= 32 or not 2 <= Cn <= 64:
                raise ValueError("top_paths = %d draws (1 .. 32) of %d classes (2 .. 64)" % (K, Cn))
            if cfg["sample_seed"] is not None:
                cfg["sample_seed"] = int(cfg["sample_seed"])
        elif not 1 <= K <= 32 or not K <= W <= 32:
            raise ValueError("top_paths = %d / beam_width = %d: 1 <= top_paths <= beam_width <= 32" % (K, W))
        cs, cd, ci = (int(v) for v in cfg["costs"])
        if min(cs, cd, ci) < 1 or max(cs, cd, ci) > 16384:
            raise ValueError("costs %r: three integers in [1, 16384]" % (cfg["costs"],))
        if not float(cfg["post_scale"]) > 0.0 or not float(cfg["ctc_weight"]) >= 0.0:
            raise ValueError("post_scale > 0 and ctc_weight >= 0, got %r / %r" % (cfg["post_scale"], cfg["ctc_weight"]))
        Lcap = min(255, max(2 * self.Lmax, 16)) if cfg["max_labels"] is None else int(cfg["max_labels"])
        if not 1 <= Lcap <= 255:
            raise ValueError("max_labels = %d: 1 .. 255" % Lcap)
        cfg.update(top_paths=K, beam_width=W, costs=(cs, cd, ci), max_labels=Lcap)
        self._release_risk()    # (the cfg is good: only now does the mode set before go)
        dev = self.mem          # (the engine's arena: freed with it, or at set_risk(None))
        r = dict(cfg=cfg, out=dev.empty((B, K, T - skip), np.int32), out_len=dev.empty((B, K), np.int32))
        if sampled:     # (the sampler needs no workspace: the counts and the number of unique labellings are all it adds)
            r.update(count=dev.empty((B, K), np.int32), n_unique=dev.empty((B,), np.int32))
        else:
            r.update(score=dev.empty((B, K), np.float64), lctc=dev.empty((B, K), np.float64), ext=dev.zeros((Cn + 1, Cn), np.float64),
                     ws_beam=dev.bytes(lib.mgr_ctc_beam_lm_ws_bytes(B, T, Cn, W, K)))
        r.update(pair_h=dev.empty((B * K,), np.int32).upload(np.arange(B * K)), pair_r=dev.empty((B * K,), np.int32).upload(np.repeat(np.arange(B), K)),
                 dist=dev.empty((B, K), np.int32), counts=dev.empty((B * K, 4), np.int32), lens=dev.empty((B * K, 2), np.int32),
                 logp=dev.empty((B, K), np.float64), weight=dev.empty((B, K), np.float32), exp_risk=dev.empty((B,), np.float32),
                 ws_risk=dev.bytes(lib.mgr_ctc_risk_ws_bytes(B, T, Cn, K, Lcap, 0, None)))
        r["bufs"] = [v for v in r.values() if isinstance(v, DeviceArray)]
        self._risk = r

    def _release_risk(self):
        if self._risk is not None:
            self.dev.sync()     # (a step that uses the buffers may be in flight)
            self.mem.release(self._risk["bufs"])
            self._risk = None

    def _enqueue_mode_head(self, feat, ldf, hm, p_head, hseed, dA, ldda, losses):
        """The head of a step of a training mode on the current stream, the separate calls mgr_head_fwd_bwd equals: Dropout / Dense /
        softmax, then losses() - the mode's loss and gradient kernels from P into dLogits; it returns the per-sample arrays of the two
        parts read_loss reports (the first None: not computed, reported as 0) -, their means, Dense backward."""
        sp, dev, B, T = self.spec, self.dev, self.B, self.T
        Cn, D = sp.num_classes, sp.head_width
        dev.call("mgr_dense_softmax_fwd", feat, ldf, hm, p_head, C.c_uint64(hseed), self._wview("dense/W"), self._wview("dense/b"), self.P,
                 B, T, D, Cn)
        first, second = losses()
        if first is not None:
            dev.call("mgr_mean", first, B, self.loss_mean)
        else:
            self.loss_mean.zero()
        dev.call("mgr_mean", second, B, self.loss_mean.view(1, (1,)))
        dev.call("mgr_dense_bwd", feat, ldf, hm, p_head, C.c_uint64(hseed), self.dLogits, self._wview("dense/W"), self._gview("dense/W"),
                 self._gview("dense/b"), dA, ldda, B, T, D, Cn, self.ws_dense, self.ws_dense.nbytes)

    def _risk_losses(self):
        """The middle of a minimum-risk step's head (set_risk): the CTC gradient scaled ctc_weight / B, the N-best list, its edit
        distances, the risk gradient ADDED with 1 / B."""
        sp, dev, B, T, r = self.spec, self.dev, self.B, self.T, self._risk
        cfg = r["cfg"]
        Cn, skip, eps = sp.num_classes, int(sp.ctc["skip"]), float(sp.ctc["eps"])
        K, cw = cfg["top_paths"], float(cfg["ctc_weight"])
        if cw != 0.0:
            dev.call("mgr_ctc_loss_grad", self.P, self.labels_d, self.ilen_d, self.llen_d, B, T, Cn, self.Lmax, skip, Cn - 1, eps, cw / B,
                     self.loss_b, self.dLogits, self.ws_ctc, self.ws_ctc.nbytes)
        if cfg["source"] == "sample":
            self.last_sample_seed = self._sample_seed(cfg["sample_seed"])
            dev.call("mgr_ctc_sample_paths", self.P, self.ilen_d, B, T, Cn, skip, Cn - 1, eps, C.c_uint64(self.last_sample_seed), K, r["out"],
                     r["out_len"], r["count"], r["n_unique"], None)
        else:
            dev.call("mgr_ctc_beam_search_lm", self.P, self.ilen_d, B, T, Cn, skip, Cn - 1, cfg["beam_width"], eps, r["ext"], None, K, r["out"],
                     r["out_len"], r["score"], r["lctc"], r["ws_beam"], r["ws_beam"].nbytes)
        dev.call("mgr_edit_distance", r["out"], r["out_len"], B * K, T - skip, self.labels_d, self.llen_d, B, self.Lmax, r["pair_h"],
                 r["pair_r"], B * K, *cfg["costs"], 0, r["dist"], r["counts"], r["lens"], None, None, None, 0)
        dev.call("mgr_ctc_risk_grad", self.P, self.ilen_d, B, T, Cn, skip, Cn - 1, eps, None, None, 0, r["out"], r["out_len"], K, T - skip,
                 cfg["max_labels"], r["dist"], 1.0, float(cfg["post_scale"]), 1.0 / B, 1 if cw != 0.0 else 0, r["logp"], r["weight"],
                 r["exp_risk"], self.dLogits, r["ws_risk"], r["ws_risk"].nbytes)
        return (self.loss_b if cw != 0.0 else None), r["exp_risk"]

    ENTROPY_DEFAULTS = dict(weight=0.2)
    last_entropy = None

    def set_entropy(self, cfg):
        """Entropy-regularised CTC training (Liu et al., NeurIPS 2018): with cfg - a dict over ENTROPY_DEFAULTS - the training
        loss is ctc - weight * H, H the entropy of the distribution over the alignments of each sample's labels, which keeps the network
        from putting all of p(labels | x) on one alignment.  The head of a step is then the separate calls mgr_head_fwd_bwd equals, with
        mgr_ctc_entropy_grad (scales 1 / B and weight / B) in the loss's place: mgr_dense_softmax_fwd, mgr_ctc_entropy_grad, the two means,
        mgr_dense_bwd.  read_loss returns the combined loss and leaves the parts in last_ctc_loss / last_entropy.  None: back to the one
        mgr_head_fwd_bwd call; the mode's buffers are freed.  Not combined with set_risk; single GPU.  A cfg that is refused leaves the
        mode as it was; the loss of a step enqueued before the call is still read as that step's."""
        if cfg is None:
            self._release_entropy()
            return
        if self._risk is not None:
            raise ValueError("set_entropy with the risk mode on: the two training modes are not combined (set_risk(None) first)")
        cfg = self._mode_cfg("set_entropy", cfg, "entropy-regularised training", "entropy training", "entropy", self.ENTROPY_DEFAULTS)
        weight = float(cfg["weight"])
        if not weight >= 0.0 or not np.isfinite(weight):
            raise ValueError("weight >= 0, got %r" % (cfg["weight"],))
        self._release_entropy()
        dev = self.mem          # (the engine's arena: freed with it, or at set_entropy(None))
        B, T, Cn = self.B, self.T, self.spec.num_classes
        e = dict(cfg=dict(weight=weight), H=dev.empty((B,), np.float32), ws=dev.bytes(2 * self.lib.mgr_ctc_ws_bytes(B, T, Cn, self.Lmax)))
        e["bufs"] = [v for v in e.values() if isinstance(v, DeviceArray)]
        self._entropy = e

    def _release_entropy(self):
        if self._entropy is not None:
            self.dev.sync()     # (a step that uses the buffers may be in flight)
            self.mem.release(self._entropy["bufs"])
            self._entropy = None

    def _entropy_losses(self):
        """The middle of an entropy-regularised step's head (set_entropy): the CTC loss and the alignment entropy with the gradient of
        (loss - weight H) / B."""
        sp, dev, B, T, e = self.spec, self.dev, self.B, self.T, self._entropy
        Cn, skip, eps = sp.num_classes, int(sp.ctc["skip"]), float(sp.ctc["eps"])
        dev.call("mgr_ctc_entropy_grad", self.P, self.labels_d, self.ilen_d, self.llen_d, B, T, Cn, self.Lmax, skip, Cn - 1, eps, 1.0 / B,
                 e["cfg"]["weight"] / B, self.loss_b, e["H"], self.dLogits, e["ws"], e["ws"].nbytes)
        return self.loss_b, e["H"]

    def set_augment(self, cfg):
        """Train-time input augmentation (augment.py): with cfg - a dict over augment.DEFAULTS - the encoder pass of every
        TRAINING STEP reads, in the place of the noised copy of its batch, Y = noise(mask(warp(X))): a length-preserving time warp
        shared by the streams of a sample, time / feature masks per stream, at most one blanked stream per sample, then the stream's
        GaussianNoise - one mgr_augment_plan per pass (seed slot 950 at the pass's step counter) and one mgr_augment_apply per stream
        in mgr_add_gaussian_noise's place (slot 900 + i as before).  The resident inputs stay pristine; labels and lengths are not
        touched (the warp keeps T).  loss_on_batch / forward_train_phase / predict / predict_stream are what they are without the
        mode.  Combines with set_risk / set_entropy.  A training step given `rand` is refused while the mode is on.  None: the mode's
        buffers are freed and a step makes exactly the calls it made before.  Single GPU; a cfg that is refused leaves the mode as
        it was."""
        if cfg is None:
            self._release_augment()
            return
        self._mode_cfg("set_augment", cfg, "input augmentation", "augmentation")     # (its keys: normalize_config)
        norm = augment_mod.normalize_config(cfg, self.spec, self.T)
        n = augment_mod.plan_len(norm)
        self._release_augment()     # (the cfg is good: only now does the mode set before go)
        self._drop_prefetched()     # (an encoder pass enqueued ahead of its step was made without the mode: it is redone under it)
        dev, B, T = self.mem, self.B, self.T
        a = dict(cfg=norm, table=augment_mod.stream_table(norm), plan=dev.empty((B, n), np.int32), own_x=[])
        for s in self.spec.streams:
            if s["name"] not in self.X:     # (a stream without GaussianNoise has had no copy to write into)
                self.X[s["name"]] = dev.empty((B, T, s["F"]))
                a["own_x"].append(s["name"])
        a["bufs"] = [a["plan"]] + [self.X[k] for k in a["own_x"]]
        self._augment = a

    def _release_augment(self):
        if self._augment is not None:
            self._drop_prefetched()     # (an encoder pass enqueued ahead was made under the mode that goes: it is redone, same randomness)
            self.dev.sync()     # (a step that uses the buffers may be in flight)
            for k in self._augment["own_x"]:
                del self.X[k]
            self.mem.release(self._augment["bufs"])
            self._augment = None

    def _drop_prefetched(self):
        """Forget the encoder pass a pipelined step enqueued for its successor: the next step runs its own (what a step does whose
        caller did not come back with the announced batch)."""
        if self._prefetched is not None:
            self.dev.wait(0, self.ES)
            self._prefetched = None

    def _enqueue_trainable_part(self, cur, rand, lay, defer, hold_bptt, own_inputs, apply_update):
        """Steps 2 and 3 of a training step of layout `lay` on stream 0 - fusion layer, head, CTC, the loss read-back point, the
        backward pass up to what `defer` (the dW / dU / db GEMMs) / `hold_bptt` (the fusion layer's BPTT with them) hold back - and the
        closure `finish(gate=None)` that enqueues the rest (held-back BPTT, dW / dU / db GEMMs, optimizer)."""
        sp, dev, B, T = self.spec, self.dev, self.B, self.T
        # ---- 2. fusion layer, head, CTC, loss read-back point
        self._enqueue_fusion_head(True, rand, cur, self.rng_step, dense=False, lay=lay)
        self.rng_step += 1
        Cn, D = sp.num_classes, sp.head_width
        dev.stream(0)
        feat, ldf = self._feat
        hm, p_head, hseed = self._head_args
        W = sp.concat_width
        any_tr_stream = any(s["trainable"] for s in sp.streams)
        if sp.fusion:
            dA, ldda = self.dYF, 2 * sp.fusion["H"]
        elif any_tr_stream:
            dA, ldda = self.dFEAT, W
        else:
            dA, ldda = 0, D
        # the whole head in one call (mgr.h): Dropout / Dense / softmax, CTC loss + gradient, the mean loss, Dense backward
        # (a step of the fused schedule: the head runs beside the next batch's deepest encoder scan - 208 whole CUs.  The CTC kernels ask
        #  for more LDS than a scan workgroup leaves on its CU - MGR_TUNE_CTC_CHAIN_LDS_KIB / _FRAME_LDS_KIB, mgr.h - so that the 32
        #  recurrence workgroups get one of the 48 other CUs each, and neither they nor the per-frame kernels share SIMDs with the scan,
        #  which is on the step's critical path)
        ctc_lds = {_capi.TUNE_CTC_CHAIN_LDS_KIB: 96, _capi.TUNE_CTC_FRAME_LDS_KIB: 64}
        with self._tuned(lay.fused, ctc_lds, keep_set=True):
            if self._risk is not None or self._entropy is not None:
                self._enqueue_mode_head(feat, ldf, hm, p_head, hseed, dA, ldda, self._risk_losses if self._risk is not None else self._entropy_losses)
            else:
                dev.call("mgr_head_fwd_bwd", feat, ldf, hm, p_head, C.c_uint64(hseed), self._wview("dense/W"), self._wview("dense/b"),
                         self.labels_d, self.ilen_d, self.llen_d, B, T, D, Cn, self.Lmax, int(sp.ctc["skip"]), Cn - 1, float(sp.ctc["eps"]),
                         1.0 / B, self.P, self.loss_b, self.loss_mean, self.dLogits, self._gview("dense/W"), self._gview("dense/b"),
                         dA, ldda, self.ws_head, self.ws_head.nbytes)
        self._loss_parts = None if self._risk is None else float(self._risk["cfg"]["ctc_weight"])
        if self._entropy is not None:      # (an entropy-regularised step; never together with the risk mode)
            self._loss_parts = ("entropy", float(self._entropy["cfg"]["weight"]))
        if self.comm is not None:
            dev.call("mgr_mean", self.loss_b, B, self.loss_slot)   # travels with the gradient all-reduce (apply_gradients)
        dev.record(self.EV_LAB[self._lab_slot])
        # The loss and this engine's scan status go to page-locked host words from THIS stream, an event behind them: the host
        # polls that event (read_loss) while the rest of the backward pass queued behind it runs.  Round 2 read them on a stream
        # of their own that waited for stream 0 - a copy on an otherwise idle hardware queue now and then started 20-45 ms after
        # the event it waited for (one step in ten of a 5 ms step; profiles/r03_loss_readback_stall.txt).
        dev.d2h_async(self.loss_host, self.loss_mean)
        dev.d2h_async(self.status_host, self.status)
        dev.record(self.EV_LOSS)
        this_step = self._step_id
        self._step_id += 1
        self._lab_user[self._lab_slot] = this_step
        if own_inputs:   # this step's own inputs (a prefetched set was tagged when it was uploaded)
            # trainable first layers read them again in their dW GEMMs, which only the NEXT step's loss read-back covers
            self._xin_user[self._xin_slot] = this_step + (1 if any_tr_stream else 0)
        # ---- 3. backward
        deferred = None
        late_bptt = None    # (Schedule.bptt_beside_deepest_scan) the fusion layer's BPTT itself is held back with its GEMMs
        if sp.fusion:
            Hf = sp.fusion["H"]
            bargs = ("fusion", self.dYF, 2 * Hf, self._featin, W, W, self.YF, 2 * Hf, self.dFEAT if any_tr_stream else None, W, lay)
            bkw = dict(defer_param_grads=defer, XinT=self._featT.get(self._featin.ptr), xin_rows=self._feat_rows.get(self._featin.ptr, True))
            if hold_bptt:
                late_bptt = lambda: self._bilstm_backward(*bargs, **bkw)
            else:
                deferred = self._bilstm_backward(*bargs, **bkw)
        if any_tr_stream:
            col = 0
            for s in sp.streams:
                if s["trainable"]:
                    self._stream_backward(s, col, lay)
                col += sp.stream_width(s)
            dev.stream(0)
            dev.record(self.EV_IN[self._xin_slot])   # trainable first layers read the inputs again in their dW GEMMs

        def finish(gate=None):
            """This step's (held-back) BPTT, its dW / dU / db GEMMs and the optimizer on stream 0.  gate: enqueues the device-side
            wait for the residency of the next persistent launch of the context - the deepest encoder scan the caller enqueues
            right after this returns.  It goes BEHIND the BPTT (a persistent launch itself: in front of it, "the next persistent
            launch" would be the BPTT queued behind the gate) and in FRONT of the chip-filling GEMMs, which are what
            must not be placed before the scan's workgroups: recurrence beside recurrence starts at once, GEMMs wait."""
            dev.stream(0)
            if lay.gate_bptt is not None and late_bptt is not None:
                # (as for the fusion scan: the depth-1 scan of the batch after next, enqueued at the end of this call, fills the word)
                dev.call("mgr_stream_wait_resident_word", int(lay.gate_bptt), int(self.schedule.resident_wait_us))
            d = late_bptt() if late_bptt is not None else deferred
            if gate is not None:
                gate()
            if d is not None:
                d()
            if apply_update:
                self.apply_gradients()
        return finish

    def _next_encoders_free(self, next_inputs, rng_step, consumer_step, scan_form, split_first=False, seq_words=None):
        """Schedule.bptt_beside_deepest_scan, as a generator.  Part 1 (before this step's fusion work is enqueued): the next
        batch's encoder pass on stream ES up to and including its deepest projection GEMMs.  Part 2 (after the loss read-back point,
        resumed with send(finish) or send((finish, pre))): stream 0 waits for those GEMMs, then - once the deepest scan launched behind
        them is resident - runs `finish` (this step's BPTT, dW / dU / db GEMMs, optimizer) beside that scan; `pre`, if given, is called
        with stream ES selected right in front of the deepest scan's waits.
        split_first (Schedule.depth1_proj_ahead): part 1 comes in two pieces - upload, noise and the depth-1 projections into the
        engine's second set of gate pre-activation buffers, then one more yield, then the rest - so that a caller can put the first
        piece in front of the PREVIOUS batch's deepest scan (its `pre`)."""
        dev, ES, depth = self.dev, self.ES, self.depth
        self._feat_idx ^= 1
        nxt = self._feat_ring[self._feat_idx]
        self._early_for = next_inputs          # (becomes _prefetched_for when the pass is complete: two announcements may be in flight)
        if next_inputs is not None:
            dev.stream(ES)
            self._upload_inputs(next_inputs, None, True, stream=ES)
            self._xin_user[self._xin_slot] = consumer_step
        split_first = bool(split_first and self.Z1buf)
        phases = self._encoder_phases(True, None, nxt, ES, rng_step, z_first=self.Z1buf if split_first else None, seq_words=seq_words,
                                      augment=True, scan_form=scan_form)
        for tag, k in phases:
            if tag == "projected" and k == 0 and split_first and depth > 1:
                dev.stream(0)
                yield "depth-1 projections"
                continue
            if tag == "projected" and k == depth - 1:
                break
        dev.stream(0)
        got = yield
        finish, pre = got if isinstance(got, tuple) else (got, None)
        dev.wait(0, ES)
        dev.stream(0)
        finish(self._resident_gate())
        if pre is not None:
            dev.stream(ES)
            pre()
            dev.stream(ES)
        dev.wait_event(ES, self.EV_PREV)   # (the deepest scan overwrites the FEAT buffer the previous step's dW GEMMs read)
        if self.schedule.deepest_scan_after_fusion_proj:
            # ... and it lets THIS step's fusion projections go first: both become ready at the same instant (the end of the previous
            # step's optimizer), and beside the scan's 408 workgroups the two GEMMs took 4.5 ms instead of 1.1 - on the chain of
            # the stream that sets the step time, while the encoder stream has ~3 ms to spare (profiles/r05_scan_probes.txt)
            dev.wait_event(ES, self.EV_FPROJ)
        for _ in phases:
            pass
        dev.stream(ES)
        dev.record(self.EV_ENC[self._feat_ring.index(nxt)])     # this pass is complete (what the step that consumes it waits for)
        self._prefetched = nxt
        self._prefetched_for = next_inputs
        dev.stream(0)
        yield

    def _resident_gate(self):
        """The device-side wait (current stream) until the persistent launch enqueued NEXT on this context - the deepest encoder scan -
        reports every workgroup resident, bounded by Schedule.resident_wait_us; None where it must not be used (switched off; in
        front of a host-blocking all-reduce: HostComm holds the host inside finish(), the scan the gate waits for would only be
        enqueued after it - the gate would always run into its bound)."""
        if self.schedule.resident_wait_us <= 0 or getattr(self.comm, "host_blocking", False):
            return None
        return lambda: self.dev.call("mgr_stream_wait_next_resident", self.schedule.resident_wait_us)

    def _enqueue_next_encoders(self, next_inputs, finish, defer, ahead, scan_form):
        """Encoder pass of the NEXT step on stream ES into the other FEAT buffer, concurrent with what enqueue_train_step
        has put on stream 0; `finish` (this step's parameter-gradient GEMMs + optimizer) is placed according to the schedule.
        (A step that may run the encoder stream free - `ahead` and the BPTT held back - goes through _next_encoders_free instead.)"""
        dev, ES, depth = self.dev, self.ES, self.depth
        self._feat_idx ^= 1
        nxt = self._feat_ring[self._feat_idx]
        self._prefetched_for = next_inputs
        if next_inputs is not None:
            dev.stream(ES)
            self._upload_inputs(next_inputs, None, True, stream=ES)
            self._xin_user[self._xin_slot] = self._step_id   # (already advanced: the step that will consume it)
        if not defer:
            finish()
            self._enqueue_encoders(True, None, nxt, ES, self.rng_step, hold_scans_for=0, augment=True, scan_form=scan_form)
        else:
            # The dW/dU GEMMs of THIS step and the optimizer are held back until the next step's deepest projection GEMMs are
            # done and then run beside its deepest encoder scan: GEMM next to GEMM gains nothing, whereas a big scan leaves
            # most of the MFMA issue slots free (tools/overlap_probe.py: scan x1.12, GEMM at 1/3 speed).
            # With `ahead` the encoder stream does not wait for this stream's previous step as a whole: its depth-1
            # projections start as soon as its own previous pass is done (beside the small kernels that end that step), the
            # depth-1 scan is launched after this step's fusion projections (a persistent launch placed among chip-filling
            # GEMMs gets a poor CU set), and only the deepest scan - the one that overwrites the FEAT buffer the previous
            # step's dW GEMMs read - waits for that step.
            for tag, k in self._encoder_phases(True, None, nxt, ES, self.rng_step, augment=True, scan_form=scan_form):
                if tag != "projected":
                    continue
                if ahead and k == 0:
                    dev.stream(ES)
                    dev.wait_event(ES, self.EV_FPROJ)
                if k == depth - 1:
                    dev.wait(0, ES)
                    dev.stream(0)
                    # Both streams become ready at the same instant.  The scan's workgroups must be placed first (one or
                    # two per CU): if GEMM waves get there first the scan's workgroups trickle in behind them and the
                    # whole scan runs at half speed (measured 22.7 vs 11.4 ms).  So the GEMMs wait - on the device - until
                    # the scan launched next on this context reports every workgroup resident.
                    # (not in front of a host-blocking all-reduce: HostComm holds the host inside finish(), the scan the gate waits
                    # for would only be enqueued after it - the gate would always run into its bound)
                    finish(self._resident_gate())
                    if ahead:
                        dev.wait_event(ES, self.EV_PREV)
        dev.stream(ES)
        dev.record(self.EV_ENC[self._feat_ring.index(nxt)])
        self._prefetched = nxt

    def _bilstm_backward(self, prefix, dY, lddy, Xin, ldx, fin, Hbuf, ldh, dX, lddx, lay, defer_param_grads=False, XinT=None, xin_rows=True):
        """BPTT + parameter grads of one Bidirectional layer (both directions in one persistent launch) in a step of layout `lay`.
        defer_param_grads: return the dW/dU/db GEMM launches as a closure instead of enqueuing them now.
        XinT: the transposed copy of Xin the forward projection was fed (same step), if the engine keeps one - the
        dropout-aware dW then reads both of its operands along time.
        xin_rows=False: the row-major Xin was not written (_feat_rows_unread) - a weight-gradient call that would read it is an error."""
        dev, B, T = self.dev, self.B, self.T
        jobs = []
        for di, dname in enumerate(("fwd", "bwd")):
            L = self.dirs["%s/%s" % (prefix, dname)]
            H = L.H
            dYv = dY.view(di * H, (1,)) if isinstance(dY, DeviceArray) else dY
            jobs.append(dict(dY=dYv, gates=L.gates, cs=L.cs, Up=L.Up, dZ=L.dZ, lddy=lddy, B=B, T=T, H=H,
                             reverse=L.reverse, dzmax=L.dzmax, dbsum=L.dbsum))
        dev.stream(0)
        arr = _capi.make_scan_bwd_jobs(jobs)   # both directions in ONE call (one persistent launch of CU clusters)
        need = self.lib.mgr_lstm_scan_bwd_multi_ws_bytes(len(jobs), arr)
        if getattr(self, "_ws_bwd_multi", None) is None or self._ws_bwd_multi.nbytes < need:
            self._ws_bwd_multi = self.mem.bytes(need)
        # The form of the narrow-layer BPTT is an argument of the launch (mgr.h MGR_BPTT_FORM_*; AUTO = the context's MGR_TUNE_BPTT_FORM):
        # beside the next batch's encoder scans the form that yields to them - or, beside FUSED encoder scans (CUs of its own) and if the
        # schedule asks for it, the direct gather with one barrier per step; a launch that has the chip to itself takes the context's.
        form = _capi.BPTT_FORM_AUTO
        if lay.beside_scans and self.schedule.bptt_yields_beside_scans:
            direct = (lay.wide_ok or lay.gate_bptt is not None) and self.schedule.bptt_direct_when_alone
            form = _capi.BPTT_FORM_DIRECT if direct else _capi.BPTT_FORM_YIELDING
            if lay.gate_fusion is not None and self.schedule.bptt_fused:     # (a step of the fused schedule)
                form = _capi.BPTT_FORM_FUSED_DIRECT if direct else _capi.BPTT_FORM_FUSED
        if self.schedule.bptt_single_cu and jobs[0]["H"] in (32, 64, 100):
            form = _capi.BPTT_FORM_SINGLE_CU       # (whatever the schedule puts beside it: the choice must not depend on the layout)
        opts = _capi.make_launch_opts(form, 0)
        _capi.check(self.lib.mgr_lstm_scan_bwd_multi_ex(dev.ctx, len(jobs), arr, self._ws_bwd_multi.ptr, self._ws_bwd_multi.nbytes,
                                                        C.byref(opts)))

        two = self.schedule.param_grads_two_streams

        def param_grads():
            if two:
                dev.stream(0)
                dev.wait(self.PG_STREAM, 0)     # (everything queued on stream 0 so far: the BPTT, the previous step's optimizer)
            for di, dname in enumerate(("fwd", "bwd")):
                L = self.dirs["%s/%s" % (prefix, dname)]
                H = L.H
                mptr = self._masks.get((L.prefix, L.d), 0)
                if two:
                    dev.stream(self.PG_STREAM if di == 1 else 0)
                kind = self._pgrad_kind(mptr, XinT, XinT is not None and self._xt_split.get(XinT.ptr, False), L.p, fin)
                if kind == "rows" and not xin_rows:
                    raise RuntimeError("this weight-gradient call reads row-major input the encoder pass left out")
                if kind == "ts":
                    # (the projection of this step left the kept lists of this very mask in its workspace: not built again)
                    pws = L.ws_sp if (L.ws_sp is not None and L.lists_mask == mptr) else 0
                    L.lists_mask = 0
                    # dU like dW: from the split rows of h_prev along time against the same dZ^T rows (Schedule.du_split)
                    hst = 0
                    if self.schedule.du_split and H >= 16:
                        self._prep_hst(L, Hbuf.view(di * H, (1,)), ldh)
                        hst, L.hst_ready = L.HsT, False
                    with self._narrow_tiles(lay.beside_scans and not lay.wide_ok):     # (the deferred GEMMs run beside the encoder scans as well)
                        dev.call("mgr_lstm_param_grads_dropout_ts", XinT, self.ldt, mptr, float(L.p), Hbuf.view(di * H, (1,)), ldh, L.dZ,
                                 L.gWp, L.gUp, L.gbp, B, T, fin, H, L.reverse, L.ws_pg, L.ws_pg.nbytes, L.dzmax, L.dbsum, pws, hst)
                elif kind == "t":
                    need = self.lib.mgr_lstm_param_grads_dropout_t_ws_bytes(B, T, fin, H, self.ldt)
                    if L.ws_pg.nbytes < need:          # (+ the transposed dZ; first use only)
                        L.ws_pg = self.mem.bytes(need)
                    dev.call("mgr_lstm_param_grads_dropout_t", XinT, self.ldt, mptr, float(L.p), Hbuf.view(di * H, (1,)), ldh, L.dZ,
                             L.gWp, L.gUp, L.gbp, B, T, fin, H, L.reverse, L.ws_pg, L.ws_pg.nbytes, self.XT_BOUND)
                elif mptr:   # input dropout was applied: dW only has rows for the kept features of each (gate, sample)
                    dev.call("mgr_lstm_param_grads_dropout", Xin, ldx, mptr, float(L.p), Hbuf.view(di * H, (1,)), ldh, L.dZ,
                             L.gWp, L.gUp, L.gbp, B, T, fin, H, L.reverse, L.ws_pg, L.ws_pg.nbytes)
                else:
                    dev.call("mgr_lstm_param_grads", Xin, ldx, mptr, Hbuf.view(di * H, (1,)), ldh, L.dZ, L.gWp, L.gUp,
                             L.gbp, B, T, fin, H, L.reverse, L.ws_pg, L.ws_pg.nbytes)
            if two:
                dev.stream(0)
                dev.wait(0, self.PG_STREAM)     # (the optimizer / the input-gradient GEMMs behind this need both chains)
        if not defer_param_grads:
            param_grads()
        if dX is not None:
            for di, dname in enumerate(("fwd", "bwd")):
                L = self.dirs["%s/%s" % (prefix, dname)]
                mptr = self._masks.get((L.prefix, L.d), 0)
                dev.call("mgr_lstm_input_grad", L.dZ, L.Wp, mptr, dX, lddx, 1 if di == 1 else 0, B, T, fin, L.H)
        return param_grads if defer_param_grads else None

    def _prep_hst(self, L, Hdir, ldh):
        """The split transposed copy of h_prev of direction L (rows h_{t-1} forward, h_{t+1} reverse) from its outputs Hdir, on the
        current stream, unless this step's copy exists already."""
        if L.hst_ready:
            return
        if L.HsT is None:
            L.HsT = self.dev.zeros((self.B, L.H, self.ldt))
        self.dev.call("mgr_transpose_bt_split_shift", Hdir, ldh, L.HsT, self.ldt, self.B, self.T, L.H, 1 if L.reverse else -1)
        L.hst_ready = True

    def _stream_backward(self, s, col, lay):
        sp, dev, B, T = self.spec, self.dev, self.B, self.T
        W = sp.concat_width
        name = s["name"]
        nl = len(s["layers"])
        dout = self.dFEAT.view(col, (1,))
        dF = self.fe[name]["dF"] if name in self.fe else None     # (the first layer's input gradient feeds the CNN front-end)
        if nl == 2:
            H1, H2 = s["layers"][0]["H"], s["layers"][1]["H"]
            if s["residual"]:
                Hbuf, ldh = self.Y2[name], 2 * H2
            else:
                Hbuf, ldh = self.FEAT.view(col, (1,)), W
            self._bilstm_backward("%s/l1" % name, dout, W, self.Y1[name], 2 * H1, 2 * H1, Hbuf, ldh,
                                  self.dY1[name], 2 * H1, lay, XinT=self.Y1T.get(name))
            if s["residual"]:
                dev.call("mgr_add2d", self.dY1[name], 2 * H1, dout, W, self.dY1[name], 2 * H1, B * T, 2 * H1)
            self._bilstm_backward("%s/l0" % name, self.dY1[name], 2 * H1, self._xcur[name], s["F"], s["F"],
                                  self.Y1[name], 2 * H1, dF, s["F"] if dF is not None else 0, lay)
        else:
            H1 = s["layers"][0]["H"]
            self._bilstm_backward("%s/l0" % name, dout, W, self._xcur[name], s["F"], s["F"],
                                  self.FEAT.view(col, (1,)), W, dF, s["F"] if dF is not None else 0, lay)
        if dF is not None:
            self._frontend_bwd(name)

    def apply_gradients(self):
        """all-reduce (if data parallel) -> clip -> Adam -> max-norm; identical on every replica."""
        dev, o = self.dev, self.spec.optimizer
        dev.stream(0)
        self._bind()
        # Update gate: a scan of this step that gave up (garbage gradients) or met a non-finite state must not reach the weights,
        # and the host only learns of it with the loss - after these kernels are queued.  So the decision is taken on the device:
        # the flag is evaluated here (stream order: behind every scan and GEMM of the step), rides behind the gradients through
        # the all-reduce (all replicas skip together) and closes Adam + max-norm; read_loss then raises with the weights intact.
        dev.call("mgr_update_gate_eval", _capi.SCAN_GAVE_UP | _capi.SCAN_NONFINITE, self.gate_flag)
        gscale = 1.0
        if self.comm is not None:   # (a 1-rank communicator is legal: the reduction is then the identity)
            self.comm.allreduce_sum(self.grads, max(self.n_train, 4) + 4)
            gscale = 1.0 / self.world
            step = self._step_id - 1
            dev.d2h_async(self.gloss_host[step & 1], self.gate_flag)      # [flag sum, loss sum]: read_global_loss
            dev.record(self.EV_GLOSS[step & 1])
            self._gloss_step[step & 1] = step
        # Keras' `iterations` counts APPLIED updates: what the gate skipped on the device (counted there; the host learns the
        # number with each loss read-back, i.e. one or two steps late) does not advance the learning-rate decay / bias correction
        k = self.iterations
        lr_k = o["lr"] * (1.0 / (1.0 + o["decay"] * k))
        t = k + 1
        # the bias correction takes the betas AS THE KERNEL GETS THEM (the C ABI's floats): v is built with 1 - 0.999f, which is
        # 1.3e-5 off 0.001, and a correction formed from the double 0.999 left every step 6.6e-6 too long (as float32 Keras does,
        # one beta for both keeps m / sqrt(v) free of the rounding)
        b1, b2 = float(np.float32(o["beta_1"])), float(np.float32(o["beta_2"]))
        lr_t = lr_k * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        dev.call("mgr_update_gate_set", self.gate_flag)
        try:
            dev.call("mgr_adam_step", self.params, self.grads, self.m, self.v, self.n_train, lr_t, b1, b2, o["epsilon"],
                     o["clipvalue"] or 0.0, gscale)
            for name, (off, n, shape, kind) in self.seg.items():
                if kind == "kernel":
                    mv = self.spec.kernel_maxnorm(name.rsplit("/", 2)[0])   # "<prefix>/<fwd|bwd>/W" -> "<prefix>"
                    if mv > 0:
                        dev.call("mgr_maxnorm_cols", self.params.view(off, (n,)), shape[0], shape[1], mv, 1e-7)
        finally:
            dev.call("mgr_update_gate_set", 0)      # (never leave the gate pointer installed in the context)
        self._adam_calls += 1

    def close(self):
        """Free this engine's device buffers; destroy the context only if the engine created it."""
        self.closed = True
        if self.dev.ctx is None:
            return
        self.dev.sync()
        if self._own_dev:
            self.dev.close()
            return
        self.dev.call("mgr_scan_status_bind", 0)      # (the context goes back to its own status block)
        self.mem.free_all()
