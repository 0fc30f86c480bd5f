"""Live recognition: the networks on sessions that are still producing frames.

A session is a sequence of frames 0, 1, 2, ... for every input stream of the spec, at the network rate.  The network sees it in
WINDOWS (the latency-controlled BiLSTM): window k starts at frame k * chunk and holds up to chunk + lookahead frames; the forward
direction of every Bidirectional layer starts from the state it had after the previous window's last KEPT frame, the reverse direction
starts from zero at the window's last frame.  The posteriors of a window's first `chunk` frames are the session's output; they reach
the caller chunk + lookahead frames late.  With chunk >= n_frames (one window), or with lookahead >= n_frames (every window reaches
the session's end), the result is the offline network's.

    live = engine.open_live(sessions=2, chunk=20, lookahead=20)
    live.push(0, {"the_input_audio": a, "the_input_skeletal": s})     # [n, F] network-rate feature frames, any n
    for slot, res in enumerate(live.step()):                           # one window for every slot that has one
        for label, first, last, conf in res.events: ...
    live.end(0)                                                        # the rest of slot 0 is its last windows; then the open run is flushed
"""
import collections
import ctypes as C

import numpy as np

from . import _capi

LiveResult = collections.namedtuple("LiveResult", "events posteriors n_keep")


def plan_windows(n_frames, chunk, lookahead):
    """The windows of a session of known length as (start, n_valid, n_keep): window k starts at k * chunk, holds n_valid =
    min(chunk + lookahead, n_frames - start) frames and answers the first n_keep = min(chunk, n_frames - start) of them.  Every
    frame is answered by exactly one window; the last window's lookahead is whatever is left, possibly 0."""
    n_frames, chunk, lookahead = int(n_frames), int(chunk), int(lookahead)
    if chunk < 1 or lookahead < 0 or n_frames < 0:
        raise ValueError("plan_windows: n_frames = %d, chunk = %d, lookahead = %d (chunk >= 1, the others >= 0)" % (n_frames, chunk, lookahead))
    for start in range(0, n_frames, chunk):
        left = n_frames - start
        yield start, min(chunk + lookahead, left), min(chunk, left)


class _Slot:
    """Host side of one session slot: the frames pushed and not yet kept by a window, per stream."""

    def __init__(self, widths):
        self.widths = widths
        self.clear()

    def clear(self):
        self.buf = {n: np.zeros((0, F), np.float32) for n, F in self.widths.items()}
        self.ending = False
        self.flushed = False

    @property
    def buffered(self):
        return next(iter(self.buf.values())).shape[0]


class LiveSession:
    """`sessions` independent session slots over one engine's weights.  The device weights are the ENGINE's (no copy: a later
    Engine.set_weights is seen by the next window); every other buffer - window inputs, gate pre-activations, layer outputs,
    posteriors, the carried (h, c) of every forward direction, the decode's open run, the event arrays - is this object's own, and
    none of the engine's step buffers is touched."""

    def __init__(self, engine, sessions, chunk, lookahead, cap=None):
        sp = engine.spec
        S, chunk, lookahead = int(sessions), int(chunk), int(lookahead)
        if S < 1 or chunk < 1 or lookahead < 0:
            raise ValueError("open_live: sessions = %d, chunk = %d, lookahead = %d (sessions, chunk >= 1, lookahead >= 0)" % (S, chunk, lookahead))
        for s in sp.streams:
            if s.get("frontend"):
                raise NotImplementedError("open_live: stream %s has a CNN front-end; live sessions take network-rate feature frames "
                                          "(push) and run the BiLSTM stacks only - CNN front-ends are not supported" % s["name"])
            if len(s["layers"]) > 2:
                raise NotImplementedError("open_live: stream %s has %d layers (1 or 2)" % (s["name"], len(s["layers"])))
            for lay in s["layers"]:
                if lay["H"] > _capi.LIVE_MAX_H:
                    raise ValueError("open_live: H = %d > %d" % (lay["H"], _capi.LIVE_MAX_H))
        self.engine, self.spec, self.dev = engine, sp, engine.dev
        self.S, self.chunk, self.lookahead, self.Tw = S, chunk, lookahead, chunk + lookahead
        # (a window keeps `chunk` frames: at most that many runs end inside it, plus the carried one and the flushed one)
        self.cap = chunk + 2 if cap is None else int(cap)
        if self.cap < chunk + 2:
            # (fewer would let a window finalise events that are lost AFTER the carried states have moved on)
            raise ValueError("open_live: cap = %d < chunk + 2 = %d, the most a window can finalise" % (self.cap, chunk + 2))
        self.skip = int(sp.ctc["skip"])
        self.blank = sp.num_classes - 1
        dev, Tw = engine.mem, self.Tw
        W = sp.concat_width
        self.cols, col = {}, 0
        for s in sp.streams:
            self.cols[s["name"]] = col
            col += sp.stream_width(s)
        self.widths = {s["name"]: int(s["F"]) for s in sp.streams}
        self.slots = [_Slot(self.widths) for _ in range(S)]
        self._own = []

        def keep(a):
            self._own.append(a)
            return a

        self.X = {n: keep(dev.zeros((S, Tw, F))) for n, F in self.widths.items()}
        self._xhost = {n: np.zeros((S, Tw, F), np.float32) for n, F in self.widths.items()}
        self.Z = {s["name"]: [keep(dev.zeros((S, Tw, 4 * max(lay["H"] for lay in s["layers"])))) for _ in range(2)] for s in sp.streams}
        self.Y1 = {s["name"]: keep(dev.zeros((S, Tw, 2 * s["layers"][0]["H"]))) for s in sp.streams if len(s["layers"]) == 2}
        self.FEAT = keep(dev.zeros((S, Tw, W)))
        if sp.fusion:
            Hf = sp.fusion["H"]
            self.ZF = [keep(dev.zeros((S, Tw, 4 * Hf))) for _ in range(2)]
            self.YF = keep(dev.zeros((S, Tw, 2 * Hf)))
        self.P = keep(dev.zeros((S, Tw, sp.num_classes)))
        # the carried (h, c) of every forward direction
        self.state = {prefix: keep(dev.zeros((S, 2, H))) for prefix, _, H, _, _ in sp.lstm_layers()}
        self.n_valid = keep(dev.zeros((S,), np.int32))
        self.n_keep = keep(dev.zeros((S,), np.int32))
        self.flush = keep(dev.zeros((S,), np.int32))
        self.dstate = keep(dev.zeros((S, _capi.LIVE_STATE_WORDS), np.int32))
        self.n_events = keep(dev.zeros((S,), np.int32))
        self.ev_lab = keep(dev.zeros((S, max(self.cap, 1)), np.int32))
        self.ev_seg = keep(dev.zeros((S, max(self.cap, 1), 2), np.int32))
        self.ev_conf = keep(dev.zeros((S, max(self.cap, 1))))
        self.windows = 0      # windows run so far (step() calls that reached the device)

    # ------------------------------------------------------------------------------------------ host buffering
    def _slot(self, slot):
        if not 0 <= int(slot) < self.S:
            raise IndexError("slot %s of %d" % (slot, self.S))
        return self.slots[int(slot)]

    def _alive(self):
        if self.engine.closed or not self._own:
            raise RuntimeError("this live session has ended: %s" % ("its engine was closed (a Model rebuilds its engine when a call comes with "
                               "another batch shape)" if self.engine.closed else "it was closed"))

    def push(self, slot, frames):
        """frames: {name: [n, F]} - the next n frames of the slot's session, the same n for every stream.  A stream is named by its
        own name or, where it reads several graph inputs concatenated on the feature axis (early fusion), by those inputs' names -
        what Model._split_inputs takes."""
        self._alive()
        sl = self._slot(slot)
        if sl.ending:
            raise ValueError("slot %d was ended: reset it before the next session" % slot)
        new, n = {}, None
        for s in self.spec.streams:
            name, F = s["name"], self.widths[s["name"]]
            if name in frames:
                x = np.asarray(frames[name], np.float32)
            elif s.get("inputs") and all(k in frames for k in s["inputs"]):
                parts = [np.asarray(frames[k], np.float32) for k in s["inputs"]]
                if any(q.ndim != 2 or q.shape[0] != parts[0].shape[0] for q in parts):
                    raise ValueError("push: the inputs %s of stream %s take [n, F] frames with one n, got %s" % (s["inputs"], name, [q.shape for q in parts]))
                x = np.concatenate(parts, axis=1)
            else:
                raise ValueError("push: no frames for stream %s%s" % (name, " (or its inputs %s)" % s["inputs"] if s.get("inputs") else ""))
            if x.ndim != 2 or x.shape[1] != F:
                raise ValueError("push: stream %s takes [n, %d] frames, got %s" % (name, F, x.shape))
            if n is not None and x.shape[0] != n:
                raise ValueError("push: %d frames for stream %s, %d for the others" % (x.shape[0], name, n))
            n = x.shape[0]
            new[name] = x
        for name, x in new.items():
            sl.buf[name] = np.concatenate([sl.buf[name], x], axis=0)

    def end(self, slot):
        """No more frames for the slot's session: its next windows take what is buffered (the lookahead shrinks to what is left) and
        the decode's open run is closed behind the last frame."""
        self._slot(slot).ending = True

    def reset(self, slot):
        """A new session in the slot: frames still buffered are dropped, the carried states and the decode state are zeroed."""
        self._alive()
        slot = int(slot)
        self._slot(slot).clear()
        self.dev.stream(0)
        for st in self.state.values():
            H = st.shape[2]
            st.view(slot * 2 * H, (2, H)).zero()
        self.dstate.view(slot * _capi.LIVE_STATE_WORDS, (_capi.LIVE_STATE_WORDS,)).zero()

    def pending(self, slot):
        """Frames of the slot pushed and not yet answered."""
        return self._slot(slot).buffered

    def done(self, slot):
        """The slot was ended and everything it held has been answered and flushed."""
        sl = self._slot(slot)
        return sl.ending and sl.flushed

    def _plan(self):
        """(n_valid, n_keep, flush) of the next window, per slot: a slot takes part when it has a whole window buffered, or is ending
        and has frames - or only its flush - left."""
        nv, nk, fl = (np.zeros(self.S, np.int32) for _ in range(3))
        for i, sl in enumerate(self.slots):
            n = sl.buffered
            if sl.ending and not sl.flushed:
                nv[i], nk[i] = min(self.Tw, n), min(self.chunk, n)
                fl[i] = int(nk[i] == n)
            elif not sl.ending and n >= self.Tw:
                nv[i], nk[i] = self.Tw, self.chunk
        return nv, nk, fl

    # ------------------------------------------------------------------------------------------ one window
    def step(self, posteriors=False):
        """One window for every slot that has one.  Returns per slot a LiveResult: events - the gestures finalised by this window as
        (label, first_frame, last_frame, confidence), frames counted from the session's start; posteriors - with posteriors=True
        the [n_keep, C] rows this window answers (else None); n_keep.  A slot without a window gets no events and n_keep = 0."""
        self._alive()
        nv, nk, fl = self._plan()
        if not (nv.any() or fl.any()):
            return [LiveResult([], np.zeros((0, self.spec.num_classes), np.float32) if posteriors else None, 0) for _ in range(self.S)]
        dev = self.dev
        dev.stream(0)
        for name, host in self._xhost.items():
            host[...] = 0
            for i, sl in enumerate(self.slots):
                host[i, :nv[i]] = sl.buf[name][:nv[i]]
            self.X[name].upload(host)
        self.n_valid.upload(nv)
        self.n_keep.upload(nk)
        self.flush.upload(fl)
        self._enqueue(nv, nk)
        n_ev = self.n_events.download()
        assert int(n_ev.max()) <= self.cap      # (cap >= chunk + 2: more cannot end in one window)
        lab = seg = conf = None
        if n_ev.any():
            lab, seg, conf = self.ev_lab.download(), self.ev_seg.download(), self.ev_conf.download()
        P = self.P.download() if posteriors else None
        out = []
        for i, sl in enumerate(self.slots):
            ev = [(int(lab[i, e]), int(seg[i, e, 0]), int(seg[i, e, 1]), float(conf[i, e])) for e in range(int(n_ev[i]))]
            out.append(LiveResult(ev, P[i, :nk[i]].copy() if posteriors else None, int(nk[i])))
            for name in sl.buf:
                sl.buf[name] = sl.buf[name][nk[i]:]
            if fl[i]:
                sl.flushed = True
        self.windows += 1
        return out

    def _enqueue(self, nv, nk):
        """The device calls of one window, on the current stream: per encoder depth the input projections of every stream and
        direction and ONE window scan; the fusion layer the same; Dense + softmax; the carried greedy decode."""
        sp, dev, eng, S, Tw = self.spec, self.dev, self.engine, self.S, self.Tw
        W = sp.concat_width
        h_nv, h_nk = nv.ctypes.data, nk.ctypes.data
        for k in range(max(len(s["layers"]) for s in sp.streams)):
            jobs = []
            for s in sp.streams:
                nl = len(s["layers"])
                if k >= nl:
                    continue
                name, H, col = s["name"], s["layers"][k]["H"], self.cols[s["name"]]
                if k == 0:
                    cur, fin = self.X[name], s["F"]
                else:
                    cur, fin = self.Y1[name], 2 * s["layers"][0]["H"]
                for di, dname in enumerate(("fwd", "bwd")):
                    L = eng.dirs["%s/l%d/%s" % (name, k, dname)]
                    Z = self.Z[name][di]
                    dev.call("mgr_lstm_input_proj", cur, fin, 0, L.Wp, L.bp, Z, S, Tw, fin, H)
                    R, ldr = 0, 0
                    if k < nl - 1:
                        Y, ldy = self.Y1[name].view(di * H, (1,)), 2 * H
                    else:
                        Y, ldy = self.FEAT.view(col + di * H, (1,)), W
                        if nl == 2 and s["residual"]:
                            R, ldr = self.Y1[name].view(di * H, (1,)), 2 * H
                    jobs.append(dict(Z=Z, Up=L.Up, Y=Y, ldy=ldy, R=R, ldr=ldr, H=H, reverse=L.reverse,
                                     state=0 if L.reverse else self.state["%s/l%d" % (name, k)]))
            self._scan(jobs, h_nv, h_nk)
        feat, ldf = self.FEAT, W
        if sp.fusion:
            Hf = sp.fusion["H"]
            jobs = []
            for di, dname in enumerate(("fwd", "bwd")):
                L = eng.dirs["fusion/%s" % dname]
                dev.call("mgr_lstm_input_proj", self.FEAT, W, 0, L.Wp, L.bp, self.ZF[di], S, Tw, W, Hf)
                jobs.append(dict(Z=self.ZF[di], Up=L.Up, Y=self.YF.view(di * Hf, (1,)), ldy=2 * Hf, H=Hf, reverse=L.reverse,
                                 state=0 if L.reverse else self.state["fusion"]))
            self._scan(jobs, h_nv, h_nk)
            feat, ldf = self.YF, 2 * Hf
        dev.call("mgr_dense_softmax_fwd", feat, ldf, 0, 0.0, C.c_uint64(0), eng._wview("dense/W"), eng._wview("dense/b"), self.P, S, Tw,
                 sp.head_width, sp.num_classes)
        dev.call("mgr_live_greedy", self.P, S, Tw, sp.num_classes, self.n_keep, self.blank, self.skip, self.dstate, self.flush, self.cap,
                 self.n_events, self.ev_lab, self.ev_seg, self.ev_conf)

    def _scan(self, jobs, h_nv, h_nk):
        for j0 in range(0, len(jobs), _capi.LIVE_MAX_JOBS):
            part = jobs[j0:j0 + _capi.LIVE_MAX_JOBS]
            self.dev.call("mgr_lstm_scan_window", len(part), _capi.make_live_jobs(part), self.S, self.Tw, self.n_valid, self.n_keep, h_nv, h_nk)

    def close(self):
        """Free this session's device buffers (the engine's stay)."""
        if self._own:
            self.engine.mem.release(self._own)
            self._own = []


def run_session(live, slot, frames_iter, posteriors=False):
    """Feed one session from an iterator of {stream: [n, F]} pieces into `slot` and yield every LiveResult with frames or events in it,
    as the windows complete; ends and flushes the session when the iterator is exhausted."""
    for frames in frames_iter:
        live.push(slot, frames)
        while live.pending(slot) >= live.Tw:
            yield live.step(posteriors)[slot]
    live.end(slot)
    while not live.done(slot):
        yield live.step(posteriors)[slot]


def decode_live(model, frames_iter, chunk, lookahead, map_gest):
    """The generator behind every decode module's decode_live: one live session over `model` (a keras_like.Model, or anything with
    open_live), fed from frames_iter; yields (name, first_frame, last_frame, confidence) as gestures are finalised - at most chunk +
    lookahead frames (decoding.FRAME_PERIOD_HTK each) after their last frame, the last one when the iterator ends."""
    live = model.open_live(1, chunk, lookahead)
    try:
        for res in run_session(live, 0, frames_iter):
            for label, first, last, conf in res.events:
                yield map_gest[label], first, last, conf
    finally:
        live.close()
