"""Train-time sequence augmentation: the host side of mgr_augment_plan / mgr_augment_apply (csrc/augment.hip).

A length-preserving time warp shared by the streams of a sample (performer speed), SpecAugment's time and feature masks per stream
(Park et al., Interspeech 2019) and ModDrop's blanked stream (Neverova et al., PAMI 2016).  Settings, all off by default:

    segments        K: the time axis is cut into K pieces at a_j = j (T - 1) / K and the inner cuts move
    max_shift       D: each inner cut moves by a uniform integer in [-D, D]; 2 D must stay below the shortest piece
    time_masks      blocks of frames set to `fill`, each of a uniform width in [0, time_width] at a uniform start
    time_width
    feature_masks   blocks of features set to `fill`, each of a uniform width in [0, feature_width]
    feature_width
    fill            what a masked element / a dropped stream becomes (0: the padding value of the data generators)
    stream_drop     probability that ONE stream of a sample is blanked (never more than one)
    streams         {stream name: dict(time_masks=, time_width=, feature_masks=, feature_width=, fill=)} - overrides per stream

normalize_config needs no device.  augment_batch shows what a setting does to a batch; Engine.set_augment runs the same two calls at
the noise site of a training step's encoder pass."""
import ctypes as C

import numpy as np

from . import _capi

DEFAULTS = dict(segments=1, max_shift=0, time_masks=0, time_width=0, feature_masks=0, feature_width=0, fill=0.0, stream_drop=0.0,
                streams=None)
STREAM_KEYS = ("time_masks", "time_width", "feature_masks", "feature_width", "fill")
PLAN_SLOT = 950          # the seed slot of a pass's plan (Engine._seed); the noise of stream i keeps 900 + i


def _streams_of(spec):
    """[(name, F, noise, has front-end)] of a NetworkSpec, its dict form, or a plain list of stream dicts."""
    streams = getattr(spec, "streams", None)
    if streams is None:
        streams = spec["streams"] if isinstance(spec, dict) else spec
    return [(s["name"], int(s["F"]) if "F" in s else None, float(s.get("noise", 0.0)), bool(s.get("frontend"))) for s in streams]


def shortest_segment(T, K):
    """min_j (a_{j+1} - a_j) of the K source segments over T frames."""
    return min((j + 1) * (T - 1) // K - j * (T - 1) // K for j in range(K))


def _int(cfg, key, lo, hi=None):
    v = cfg[key]
    if isinstance(v, bool) or int(v) != v:
        raise ValueError("%s = %r: an integer" % (key, v))
    v = int(v)
    if v < lo or (hi is not None and v > hi):
        raise ValueError("%s = %d: %d .. %s" % (key, v, lo, "" if hi is None else hi))
    return v


def normalize_config(cfg, spec, T):
    """The settings with defaults applied and every stream's own values resolved: dict(segments, max_shift, stream_drop, drop_thresh,
    n_t, n_f, streams=[dict(name, F, time_masks, time_width, feature_masks, feature_width, fill)] in spec order).  n_t / n_f are the
    mask slots of a plan row (the largest count over the streams); drop_thresh is (uint32)(stream_drop 2^24), what the plan compares
    24 random bits against.  Raises ValueError naming the offending key; NotImplementedError for a stream with a CNN front-end.
    T=None checks everything that does not depend on the sequence length."""
    cfg = dict(cfg or {})
    unknown = set(cfg) - set(DEFAULTS)
    if unknown:
        raise ValueError("unknown augment settings %s (known: %s)" % (sorted(unknown), sorted(DEFAULTS)))
    full = dict(DEFAULTS, **cfg)
    streams = _streams_of(spec)
    S = len(streams)
    if not 1 <= S <= _capi.AUGMENT_MAX_STREAMS:
        raise ValueError("streams: %d of them (1 .. %d)" % (S, _capi.AUGMENT_MAX_STREAMS))
    for name, F, _, fe in streams:
        if fe:
            raise NotImplementedError("stream %s has a CNN front-end: its frames are not augmented (as they take no GaussianNoise)" % name)
    K = _int(full, "segments", 1)
    if K > _capi.AUGMENT_MAX_SEGMENTS:
        raise ValueError("segments = %d: at most %d" % (K, _capi.AUGMENT_MAX_SEGMENTS))
    D = _int(full, "max_shift", 0)
    if T is not None:
        T = int(T)
        if not 1 <= T <= _capi.AUGMENT_MAX_T:
            raise ValueError("T = %d: 1 .. %d" % (T, _capi.AUGMENT_MAX_T))
        if K > 1 and T - 1 < K:
            raise ValueError("segments = %d: more than the %d frame steps of T = %d" % (K, T - 1, T))
        if K > 1 and 2 * D >= shortest_segment(T, K):
            raise ValueError("max_shift = %d: 2 max_shift must stay below the shortest segment (%d frames at T = %d, segments = %d)"
                             % (D, shortest_segment(T, K), T, K))
    p = float(full["stream_drop"])
    if not 0.0 <= p < 1.0:
        raise ValueError("stream_drop = %r: a probability in [0, 1)" % (full["stream_drop"],))
    if p > 0 and S < 2:
        raise ValueError("stream_drop = %r on a network of one stream: there would be nothing left" % (full["stream_drop"],))
    over = dict(full["streams"] or {})
    names = [n for n, _, _, _ in streams]
    if set(over) - set(names):
        raise ValueError("streams: no stream named %s (streams: %s)" % (sorted(set(over) - set(names)), names))
    out = []
    for name, F, _, _ in streams:
        o = dict(over.get(name) or {})
        if set(o) - set(STREAM_KEYS):
            raise ValueError("streams[%r]: unknown settings %s (known: %s)" % (name, sorted(set(o) - set(STREAM_KEYS)), list(STREAM_KEYS)))
        st = {k: o.get(k, full[k]) for k in STREAM_KEYS}
        st["time_masks"] = _int(st, "time_masks", 0, _capi.AUGMENT_MAX_MASKS)
        st["feature_masks"] = _int(st, "feature_masks", 0, _capi.AUGMENT_MAX_MASKS)
        st["time_width"] = _int(st, "time_width", 0)
        st["feature_width"] = _int(st, "feature_width", 0)
        if T is not None and st["time_width"] > T:
            raise ValueError("time_width = %d of stream %s: wider than T = %d" % (st["time_width"], name, T))
        if F is not None and st["feature_width"] > F:
            raise ValueError("feature_width = %d of stream %s: wider than its F = %d" % (st["feature_width"], name, F))
        st["fill"] = float(st["fill"])
        st.update(name=name, F=F)
        out.append(st)
    return dict(segments=K, max_shift=D, stream_drop=p, drop_thresh=int(p * 16777216.0),
                n_t=max(s["time_masks"] for s in out), n_f=max(s["feature_masks"] for s in out), streams=out)


def plan_len(norm):
    """int32 entries of one sample's plan row (mgr.h: K + 2 + 2 S (n_t + n_f))."""
    n = _capi.load_library().mgr_augment_plan_len(len(norm["streams"]), norm["segments"], norm["n_t"], norm["n_f"])
    if n <= 0:
        raise ValueError("augment settings out of the library's range: %r" % (norm,))
    return int(n)


def stream_table(norm):
    """The host array mgr_augment_plan reads each stream's F and mask settings from (kept alive by the caller for the call)."""
    return np.ascontiguousarray([[s["F"], s["time_masks"], s["time_width"], s["feature_masks"], s["feature_width"]]
                                 for s in norm["streams"]], np.int32)


def enqueue_plan(dev, norm, table, B, T, seed, plan):
    """mgr_augment_plan on the device's current stream: the plan rows of B samples under `seed`."""
    dev.call("mgr_augment_plan", int(B), int(T), len(norm["streams"]), norm["segments"], norm["max_shift"], norm["n_t"], norm["n_f"],
             table.ctypes.data, norm["drop_thresh"], C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), plan)


def enqueue_apply(dev, norm, si, X, Y, plan, B, T, stddev=0.0, seed=0):
    """mgr_augment_apply for stream number si on the current stream: Y = noise(mask(warp(X)))."""
    s = norm["streams"][si]
    dev.call("mgr_augment_apply", X, Y, plan, int(B), int(T), s["F"], len(norm["streams"]), norm["segments"], norm["n_t"], norm["n_f"],
             int(si), float(s["fill"]), float(stddev), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF))


def augment_batch(inputs, cfg, seed, device=0):
    """What the settings `cfg` do to one batch under `seed`: inputs is {stream name: array [B, T, F]} (all streams of the samples, in
    the network's order); returns ({name: augmented float32 array}, plan) with plan the int32 rows the device drew (layout: mgr.h).
    No noise is added.  device: a GPU index or a _capi.Device."""
    names = list(inputs)
    arrs = {n: np.ascontiguousarray(inputs[n], np.float32) for n in names}
    B, T = arrs[names[0]].shape[:2]
    for n in names:
        if arrs[n].ndim != 3 or arrs[n].shape[:2] != (B, T):
            raise ValueError("input %s: expected (%d, %d, F), got %s" % (n, B, T, arrs[n].shape))
    norm = normalize_config(cfg, [dict(name=n, F=arrs[n].shape[2]) for n in names], T)
    own = not isinstance(device, _capi.Device)
    dev = _capi.Device(device) if own else device
    bufs = []
    try:
        plan = dev.empty((B, plan_len(norm)), np.int32)
        bufs.append(plan)
        table = stream_table(norm)
        enqueue_plan(dev, norm, table, B, T, seed, plan)
        out = {}
        for si, n in enumerate(names):
            X, Y = dev.array(arrs[n]), dev.empty(arrs[n].shape)
            bufs += [X, Y]
            enqueue_apply(dev, norm, si, X, Y, plan, B, T)
            out[n] = Y.download()
        return out, plan.download()
    finally:
        if own:
            dev.close()
        else:
            dev.free(*bufs)
