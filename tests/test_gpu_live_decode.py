"""-m gpu: mgr_live_greedy (include/mgr.h K21, csrc/live_decode.hip): `==` with the restatement in tests/live_ref.py and with the
non-blank runs of decoding.greedy_segments(thr=-1) on the concatenated posteriors, for sessions cut into windows of 1, 5 and 64+
frames, runs that straddle every window boundary, skip inside the first window(s), more events than cap, and flushes."""
import numpy as np
import pytest

import live_ref
from mgr_amd import _capi, decoding

pytestmark = pytest.mark.gpu

f32 = np.float32
W = _capi.LIVE_STATE_WORDS


def _planted(labels, C, rng):
    """Posteriors whose best class at frame t is labels[t], with distinct maxima."""
    n = len(labels)
    P = rng.uniform(0.0, 0.3, (n, C)).astype(f32)
    P[np.arange(n), labels] = rng.uniform(0.5, 1.0, n).astype(f32)
    return P


def _random(n, C, rng):
    """Few classes win (long and short runs), with exact ties among the columns of some frames (the first index wins)."""
    P = rng.uniform(0, 1, (n, C)).astype(f32)
    lab = np.repeat(rng.integers(0, C, n), rng.integers(1, 6, n))[:n]
    P[np.arange(n), lab] += f32(1)
    tie = rng.random(n) < 0.2
    P[tie, (lab[tie] + 1) % C] = P[tie, lab[tie]]
    return P


class Runner:
    """S sessions on the device, each fed its own window sizes."""

    def __init__(self, dev, S, Tw, C, blank, skip, cap):
        self.dev, self.S, self.Tw, self.C, self.blank, self.skip, self.cap = dev, S, Tw, C, blank, skip, cap
        self.P = dev.zeros((S, Tw, C))
        self.state = dev.zeros((S, W), np.int32)
        self.nk, self.flush, self.n_ev = (dev.zeros((S,), np.int32) for _ in range(3))
        self.lab, self.seg, self.conf = dev.zeros((S, max(cap, 1)), np.int32), dev.zeros((S, max(cap, 1), 2), np.int32), dev.zeros((S, max(cap, 1)))
        self.host = np.zeros((S, Tw, C), f32)

    def window(self, rows, flush):
        """rows[s]: (n, C) posteriors, n <= Tw; returns per session (true event count, the events that fit cap)."""
        self.host[...] = np.nan                                 # (rows behind n_keep are never read)
        for s, r in enumerate(rows):
            self.host[s, :len(r)] = r
        self.P.upload(self.host)
        self.nk.upload(np.int32([len(r) for r in rows]))
        self.flush.upload(np.int32(flush))
        self.dev.call("mgr_live_greedy", self.P, self.S, self.Tw, self.C, self.nk, self.blank, self.skip, self.state, self.flush, self.cap,
                      self.n_ev, self.lab, self.seg, self.conf)
        n, lab, seg, conf = self.n_ev.download(), self.lab.download(), self.seg.download(), self.conf.download()
        return [(int(n[s]), [(int(lab[s, e]), int(seg[s, e, 0]), int(seg[s, e, 1]), float(conf[s, e])) for e in range(min(int(n[s]), self.cap))])
                for s in range(self.S)]

    def free(self):
        self.dev.free(self.P, self.state, self.nk, self.flush, self.n_ev, self.lab, self.seg, self.conf)


def _session(dev, P, win, C, skip, cap=None, blank=None):
    """One session P (n, C) in windows of `win` frames, flushed with the last; returns (device events, restated events)."""
    n = P.shape[0]
    blank = C - 1 if blank is None else blank
    cap = win + 2 if cap is None else cap
    r = Runner(dev, 1, win, C, blank, skip, cap)
    ref = live_ref.GreedyState(blank, skip)
    got, want = [], []
    for s0 in range(0, n, win):
        rows, last = P[s0:s0 + win], s0 + win >= n
        cnt, ev = r.window([rows], [int(last)])[0]
        w = ref.window(rows, last)
        assert cnt == len(w)
        got += ev
        want += w[:cap]
    st = r.state.download()[0]
    assert st[0] == n and st[4] == 0                           # every frame consumed, no run left open behind the flush
    r.free()
    return got, want


def _offline(dev, P, skip, blank):
    return [e for e in decoding.greedy_segments(P[None], -1, skip=skip, dev=dev)[0] if e[0] != blank]


@pytest.mark.parametrize("C", [2, 22, 44, 64])
@pytest.mark.parametrize("win", [1, 5, 64, 70])
def test_random_sessions_equal_the_restatement_and_the_offline_decode(device, C, win):
    rng = np.random.default_rng(100 * C + win)
    P = _random(150, C, rng)
    for skip in (0, 2):
        got, want = _session(device, P, win, C, skip)
        assert got == want
        assert got == _offline(device, P, skip, C - 1)


@pytest.mark.parametrize("win", [1, 5, 64])
def test_runs_straddle_every_window_boundary(device, win):
    """Runs of a non-blank label across each boundary, one by one and all at once; blank runs across boundaries separate equal labels."""
    C, rng = 22, np.random.default_rng(win)
    n = 4 * win + 3
    cases = []
    for b in range(win, n, win):
        lab = np.full(n, C - 1)
        lab[max(b - 2, 0):b + 2] = 3                              # one run over boundary b
        cases.append(lab)
    lab = np.arange(n) // max(win, 2) % 3 + 1
    lab[win // 2::win] = 5
    cases.append(lab)                                             # label changes exactly at the boundaries as well
    lab = np.full(n, 7)
    lab[win - 1:win + 1] = C - 1                                  # the same label on both sides of a blank run over the boundary
    cases.append(lab)
    cases.append(np.full(n, 4))                                   # one run over the whole session
    cases.append(np.full(n, C - 1))                               # nothing but blank
    for lab in cases:
        P = _planted(lab, C, rng)
        got, want = _session(device, P, win, C, 0)
        assert got == want and got == _offline(device, P, 0, C - 1)
        assert [e[:3] for e in got] == live_ref.collapse_offline(lab, C - 1)


@pytest.mark.parametrize("win,skip", [(5, 3), (1, 2), (1, 1), (5, 5), (5, 7), (64, 66)])
def test_skip_inside_and_across_the_first_windows(device, win, skip):
    C, rng = 22, np.random.default_rng(skip)
    n = 2 * win + skip + 9
    lab = np.full(n, 2)
    lab[skip + 3:] = 6                                            # a run that starts below skip and goes on behind it
    P = _planted(lab, C, rng)
    got, want = _session(device, P, win, C, skip)
    assert got == want and got == _offline(device, P, skip, C - 1)
    assert got[0][:3] == (2, skip, skip + 2)


def test_more_events_than_cap(device):
    C, win, cap = 22, 64, 5
    lab = np.arange(130) % 2 * 3 + 1                              # a new run every frame
    P = _planted(lab, C, np.random.default_rng(3))
    got, want = _session(device, P, win, C, 0, cap=cap)           # (_session checks the TRUE count of every window)
    # (two windows of 64 one-frame runs give cap events each; the last holds two frames: the carried run, the first frame's, the flush)
    assert got == want and len(got) == 2 * cap + 3
    assert _session(device, P, win, C, 0, cap=0)[0] == []


def test_flush_with_and_without_an_open_run(device):
    C = 22
    rng = np.random.default_rng(4)
    r = Runner(device, 2, 8, C, C - 1, 0, 4)
    ref = [live_ref.GreedyState(C - 1, 0) for _ in range(2)]
    a, b = _planted(np.int64([1, 1, 2, 2, 2]), C, rng), _planted(np.int64([3, 21, 21]), C, rng)
    # session 0 keeps label 2 open; session 1 a blank run
    out = r.window([a, b], [0, 0])
    assert [o[1] for o in out] == [ref[0].window(a), ref[1].window(b)] and [o[0] for o in out] == [1, 1]
    st = r.state.download()
    assert tuple(st[0, :5]) == (5, 2, 2, 4, 3) and tuple(st[1, :5]) == (3, 21, 1, 2, 2)
    # a flush without frames: session 0's open run becomes an event, session 1's blank run does not; nothing is open afterwards
    e = np.zeros((0, C), f32)
    out = r.window([e, e], [1, 1])
    assert [o[1] for o in out] == [ref[0].window(e, True), ref[1].window(e, True)] and [o[0] for o in out] == [1, 0]
    assert out[0][1][0][:3] == (2, 2, 4)
    # a flush with no open run: no event; and an idle call changes nothing
    out = r.window([e, e], [1, 0])
    st = r.state.download()
    assert [o[0] for o in out] == [0, 0] and tuple(st[:, 0]) == (5, 3) and not st[:, 4].any()
    # the session goes on behind a flush: frame numbers continue
    out = r.window([a[:2], e], [1, 0])
    assert out[0][1] == ref[0].window(a[:2], True) and out[0][1][0][:3] == (1, 5, 6)
    r.free()


def test_several_sessions_with_different_window_sizes(device):
    """Sessions in one call are independent: each `==` its own restatement, whatever the others do (idle ones included)."""
    C, S, Tw = 44, 4, 70
    rng = np.random.default_rng(6)
    Ps = [_random(200, C, rng) for _ in range(S)]
    sizes = [70, 1, 33, 0]
    r = Runner(device, S, Tw, C, C - 1, 2, Tw + 2)
    ref = [live_ref.GreedyState(C - 1, 2) for _ in range(S)]
    pos = [0] * S
    for it in range(3):
        rows = [Ps[s][pos[s]:pos[s] + sizes[s]] for s in range(S)]
        pos = [pos[s] + sizes[s] for s in range(S)]
        out = r.window(rows, [it == 2] * S)
        for s in range(S):
            assert out[s][1] == ref[s].window(rows[s], it == 2)
    r.free()


def test_refusals(device):
    r = Runner(device, 1, 4, 5, 4, 0, 2)
    args = lambda **kw: [kw.get(k, v) for k, v in (("P", r.P), ("S", 1), ("Tw", 4), ("C", 5), ("nk", r.nk), ("blank", 4), ("skip", 0), ("state", r.state),
                                                   ("flush", r.flush), ("cap", 2), ("n", r.n_ev), ("lab", r.lab), ("seg", r.seg), ("conf", r.conf))]
    for bad in (dict(P=0), dict(state=0), dict(blank=5), dict(skip=-1), dict(cap=-1), dict(lab=0), dict(C=0), dict(S=0)):
        with pytest.raises(_capi.MgrError):
            device.call("mgr_live_greedy", *args(**bad))
    device.call("mgr_live_greedy", *args(flush=0))                # (no flush array: nobody is flushed)
    r.free()
