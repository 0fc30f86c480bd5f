"""A test double that records what an Engine enqueues: no GPU, no libmgr.so.

Engine takes a Device; RecordingDevice is a Device whose memory is a bump allocator over a fake heap and whose `lib` records every
call (name, arguments) and answers 0.  Unmodified engine code runs on it, and the recorded trace - one line per call - is the
engine's enqueue sequence: which call, in which order, on which stream, with which buffers, forms, seeds and gate words.  Nothing is
computed.  tests/test_cpu_enqueue_trace.py compares traces of a list of cases (enqueue_cases below) against goldens recorded from
the commit before the step layout became a value (tests/golden/make_enqueue_traces.py).

What the stand-in library answers (everything else: 0):
  *_ws_bytes                  WS_BYTES
  mgr_tune / mgr_tune_get     a dict per device
  *_wants_transposed          drop rate >= 0.3, F >= 128, tune key TUNE_PROJ_DENSE == 0.  This is a COPY of the rule in csrc/gemm.hip
                              (mgr_lstm_input_proj_dropout_wants_transposed / mgr_lstm_param_grads_dropout_wants_transposed).
  mgr_d2h                     zeroes the host destination: what is read back from the fake device is 0 (a clean scan status, a loss
                              of 0), not whatever np.empty held

Rendering: a device address is `d+<hex offset into the fake heap>`, an address inside the k-th pinned array `pin<k>+<hex offset>`, any
other host address `host`; ctypes structs, arrays and byref() arguments are expanded field by field, so the form and seq_out of every
scan launch and the Y / YT of every scan job are readable.  The text is identical across processes.
"""
import ctypes as C
import numbers

import numpy as np

from mgr_amd import _capi
from mgr_amd._capi import Device, DeviceArray

HEAP_BASE = 1 << 56        # (above every user-space host address)
ALIGN = 256
WS_BYTES = 4096
_BYREF = type(C.byref(C.c_int()))


class _Ctx:
    def __repr__(self):
        return "ctx"


class _Lib:
    """Stands in for the ctypes library object: every mgr_* attribute is a function that records its call."""

    def __init__(self, dev):
        self._dev = dev
        self.tune = {}

    def __getattr__(self, name):
        if not name.startswith("mgr_"):
            raise AttributeError(name)
        fn = lambda *args: self._call(name, args)
        self.__dict__[name] = fn
        return fn

    def _call(self, name, args):
        self._dev.trace.append("%s(%s)" % (name, ", ".join(self._dev.render(a) for a in args)))
        if name.endswith("_ws_bytes"):
            return WS_BYTES
        if name == "mgr_tune":
            self.tune[int(args[1])] = int(args[2])
        elif name == "mgr_tune_get":
            args[2]._obj.value = self.tune.get(int(args[1]), 0)
        elif name.endswith("_wants_transposed"):
            return int(args[1].value >= 0.3 and args[2] >= 128 and self.tune.get(_capi.TUNE_PROJ_DENSE, 0) == 0)
        elif name == "mgr_d2h":
            C.memset(args[1], 0, args[3])
        elif name == "mgr_last_error":
            return b""
        return 0


class RecordingDevice(Device):
    def __init__(self):
        self.trace = []
        self.lib = _Lib(self)
        self.ctx = _Ctx()
        self.index = 0
        self.cu_count, self.hbm_bytes, self.name = 256, 1 << 38, "recorder"
        self._arrays = []
        self._pinned = []     # the numpy arrays themselves
        self._top = 0

    def empty(self, shape, dtype=np.float32):
        if isinstance(shape, int):
            shape = (shape,)
        n = max(int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize, 16)
        a = DeviceArray(self, HEAP_BASE + self._top, shape, dtype)
        self.trace.append("alloc(%d) -> d+0x%x" % (n, self._top))
        self._top += (n + ALIGN - 1) // ALIGN * ALIGN
        self._arrays.append(a)
        return a

    def pinned(self, shape, dtype=np.float32):
        a = np.zeros(shape, dtype)
        self.trace.append("pinned(%d) -> pin%d" % (a.nbytes, len(self._pinned)))
        self._pinned.append(a)
        return a

    def close(self):
        self._arrays, self._pinned, self.ctx = [], [], None

    # -- rendering ---------------------------------------------------------------------------------
    def address(self, v):
        if v == 0:
            return "0"
        if HEAP_BASE <= v < HEAP_BASE + self._top:
            return "d+0x%x" % (v - HEAP_BASE)
        for k, a in enumerate(self._pinned):
            if 0 <= v - a.ctypes.data < max(a.nbytes, 1):
                return "pin%d+0x%x" % (k, v - a.ctypes.data)
        return "host"

    def render(self, a):
        if a is None:
            return "null"
        if isinstance(a, _Ctx):
            return "ctx"
        if isinstance(a, DeviceArray):
            return self.address(a.ptr)
        if isinstance(a, bool):
            return str(int(a))
        if isinstance(a, numbers.Integral):
            return self.address(int(a)) if a >= 1 << 32 else str(int(a))
        if isinstance(a, numbers.Real):
            return repr(float(a))
        if isinstance(a, _BYREF):
            return "&" + self.render(a._obj)
        if isinstance(a, C.Structure):
            return "{%s}" % ", ".join("%s=%s" % (f[0], self._field(f[1], getattr(a, f[0]))) for f in a._fields_)
        if isinstance(a, C.Array):
            return "[%s]" % ", ".join(self.render(e) for e in a)
        if isinstance(a, C.c_void_p):
            return self.address(a.value or 0)
        if isinstance(a, C._SimpleCData):      # c_int, c_uint, c_uint64 (seeds), c_float: the value, never an address
            v = a.value
            return "%s(%s)" % (type(a).__name__, repr(float(v)) if isinstance(v, float) else v)
        return repr(a)

    def _field(self, ctype, v):
        if ctype is C.c_void_p:
            return self.address(v or 0)
        return repr(float(v)) if isinstance(v, float) else str(v)

    def text(self):
        return "\n".join(self.trace) + "\n"


class StubComm:
    """A communicator that records its all-reduce (Engine reads dev, host_blocking, allreduce_sum)."""

    def __init__(self, dev, host_blocking):
        self.dev, self.host_blocking = dev, bool(host_blocking)

    def allreduce_sum(self, darr, n):
        self.dev.trace.append("comm.allreduce_sum(%s, %d)" % (self.dev.render(darr), n))


# ---------------------------------------------------------------------------------------------------- the cases
B, T, LMAX = 4, 32, 5       # the smallest shapes Engine._build takes; nothing is computed


def _batch(spec, seed=0):
    """(inputs, labels, input_length, label_length) of the engine's shapes: zeros, distinct objects per call."""
    from mgr_amd.spec import input_width
    xs = {}
    for s in spec.streams:
        fe = s.get("frontend")
        xs[s["name"]] = np.zeros((B, T) + (tuple(fe["input_shape"]) if fe else (input_width(s),)), np.float32)
    labels = np.full((B, LMAX), 1 + seed % 3, np.float64)
    return xs, labels, np.full((B, 1), T - 2, np.int64), np.full((B, 1), LMAX, np.int64)


def _engine(spec, dev=None, sched=None, **kw):
    from mgr_amd.engine import Engine, Schedule
    dev = dev or RecordingDevice()
    eng = Engine(spec, B, T, LMAX, device=dev, seed=5, schedule=Schedule(**(sched or {})), **kw)
    eng.set_weights({})      # (no weights travel; the frozen layers' planes are announced as after a real set_weights)
    return eng


def _fusion_spec():
    from mgr_amd.configs import baseline_config
    return baseline_config("F")[0]


def _resident_run(sched=None, steps=6, tune=None, modes=None, rand_at=None, comm=None):
    """tests/test_gpu_schedule_contract.py's _fusion_run: resident inputs, device RNG, steps announced two calls ahead."""
    spec = _fusion_spec()
    dev = RecordingDevice()
    for k, v in (tune or {}).items():
        dev.call("mgr_tune", k, v)
    kw = {}
    if comm is not None:
        kw = dict(comm=StubComm(dev, comm), world=2)
    eng = _engine(spec, dev, sched, **kw)
    for mode, cfg in (modes or []):
        getattr(eng, mode)(cfg)
    xs, labels, il, ll = _batch(spec)
    eng._upload_inputs(xs, None, True)
    eng._upload_labels(labels, il, ll)
    pipe = (sched or {}).get("pipeline", True)
    for i in range(steps):
        rand = None
        if i == rand_at:
            from oracle.network_ref import draw_rand
            rand = draw_rand(spec.to_dict(), B, T, np.random.default_rng(3), dtype=np.float32)
        eng.enqueue_train_step(None, None, None, None, rand=rand, apply_update=True, upload=False,
                               prefetch_next=pipe and i < steps - 1, prefetch_after_next=pipe and i < steps - 2)
        eng.read_loss()
    dev.sync()
    return dev.text()


AUGMENT = dict(segments=4, max_shift=1, time_masks=1, time_width=4, feature_masks=1, feature_width=3, stream_drop=0.2)


def _augment_run(modes):
    """set_augment asks the real library for the length of a plan row (augment.plan_len): here it gets a fixed one, as the workspace
    sizes are."""
    from mgr_amd import augment
    real, augment.plan_len = augment.plan_len, lambda norm: 64
    try:
        return _resident_run(steps=4, modes=modes)
    finally:
        augment.plan_len = real


def _drop_paths():
    """test_drop_paths_of_the_two_ahead_schedule_equal_the_plain_schedule's pipelined run: host batches, a mis-announcement at step
    2, a predict after step 5."""
    spec = _fusion_spec()
    eng = _engine(spec)
    data = [_batch(spec, k) for k in range(4)]
    order = [0, 1, 2, 3, 0, 2, 1, 3]
    for i, k in enumerate(order):
        xs, lab, il, ll = data[k]
        nxt = data[order[i + 1]][0] if i + 1 < len(order) else None
        nxt2 = data[order[i + 2]][0] if i + 2 < len(order) else None
        if i == 2:
            nxt, nxt2 = data[3][0], data[1][0]
        eng.train_step(xs, lab, il, ll, next_inputs=nxt, after_next_inputs=nxt2)
        if i == 5:
            eng.predict(data[0][0])
    eng.dev.sync()
    return eng.dev.text()


def _between_steps():
    """Config F, host batches: the other public passes between pipelined steps."""
    spec = _fusion_spec()
    eng = _engine(spec)
    data = [_batch(spec, k) for k in range(3)]
    between = {1: lambda: eng.loss_on_batch(*data[2]),
               2: lambda: eng.forward_train_phase(data[2][0]),
               3: lambda: eng.predict(data[2][0]),
               4: lambda: list(eng.predict_stream([d[0] for d in data], output="posteriors"))}
    for i in range(6):
        xs, lab, il, ll = data[i % 2]
        eng.train_step(xs, lab, il, ll, next_inputs=data[(i + 1) % 2][0], after_next_inputs=data[i % 2][0])
        if i in between:
            between[i]()
    eng.dev.sync()
    return eng.dev.text()


def _plain_network(spec, sched=None):
    """train_step with host batches three times, then loss_on_batch and predict."""
    eng = _engine(spec, sched=sched)
    data = [_batch(spec, k) for k in range(2)]
    for i in range(3):
        eng.train_step(*data[i % 2])
    eng.loss_on_batch(*data[1])
    eng.predict(data[0][0])
    eng.dev.sync()
    return eng.dev.text()


def _trainable_fusion_spec():
    from mgr_amd.spec import NetworkSpec
    d = _fusion_spec().to_dict()
    for s in d["streams"]:
        s["trainable"] = True
    return NetworkSpec.from_dict(d)


SWITCHES = ("pipeline", "defer_param_grads", "encoders_run_ahead", "transposed_inputs", "bptt_beside_deepest_scan", "split_rows",
            "encoders_two_ahead", "deepest_scan_after_fusion_proj", "depth1_proj_ahead", "bptt_yields_beside_scans", "fused_encoder_scans",
            "fused_wide_tiles", "bptt_direct_when_alone", "fusion_scan_fused", "bptt_fused", "param_grads_two_streams",
            "first_pass_on_encoder_stream", "bptt_single_cu", "du_split", "feat_rows_when_unread")


def enqueue_cases():
    """name -> callable that returns the trace text of the case."""
    from mgr_amd import configs
    from mgr_amd.engine import Schedule
    cases = {"default": lambda: _resident_run()}
    defaults = Schedule()
    for k in SWITCHES:
        cases["flip_" + k] = lambda k=k: _resident_run({k: not getattr(defaults, k)})
    cases["resident_wait_us_0"] = lambda: _resident_run(dict(resident_wait_us=0))
    cases["chain_priority_high"] = lambda: _resident_run(dict(chain_stream_priority=1))
    cases["chain_priority_low"] = lambda: _resident_run(dict(chain_stream_priority=-1))
    cases["pair_f32_rows_no_transposed"] = lambda: _resident_run(dict(split_rows=False, transposed_inputs=False))
    cases["pair_depth1_ahead_bptt_trimmed"] = lambda: _resident_run(dict(depth1_proj_ahead=True, bptt_yields_beside_scans=False))
    cases["pair_bptt_fused_direct"] = lambda: _resident_run(dict(bptt_fused=True, bptt_direct_when_alone=True))
    cases["tune_gemm_f32"] = lambda: _resident_run(tune={_capi.TUNE_GEMM_F32: 1})
    cases["drop_paths"] = _drop_paths
    cases["host_rand_mid_run"] = lambda: _resident_run(steps=5, rand_at=2)
    cases["passes_between_steps"] = _between_steps
    cases["risk_beam"] = lambda: _resident_run(steps=4, modes=[("set_risk", dict(source="beam"))])
    cases["risk_sample"] = lambda: _resident_run(steps=4, modes=[("set_risk", dict(source="sample"))])
    cases["entropy"] = lambda: _resident_run(steps=4, modes=[("set_entropy", dict())])
    cases["augment"] = lambda: _augment_run([("set_augment", AUGMENT)])
    cases["augment_risk"] = lambda: _augment_run([("set_augment", AUGMENT), ("set_risk", dict(source="beam"))])
    cases["spec_A"] = lambda: _plain_network(configs.baseline_config("A")[0])
    cases["spec_S"] = lambda: _plain_network(configs.baseline_config("S")[0])
    cases["spec_rgb"] = lambda: _plain_network(configs.rgb_spec())
    cases["fusion_all_trainable"] = lambda: _plain_network(_trainable_fusion_spec())
    cases["comm_host_blocking"] = lambda: _resident_run(comm=True)
    cases["comm_device"] = lambda: _resident_run(comm=False)
    return cases


FULL_TEXT = ("default", "flip_pipeline")      # the cases whose traces are committed in full (tests/golden/enqueue_trace_<name>.txt)
