"""Live recognition on the host: the window plan, the fp64 restatement (tests/live_ref.py) against the independent
oracle, the carried-run collapse against the offline collapse, and LiveSession's buffering against a device that records calls."""
import itertools
import types

import numpy as np
import pytest

import live_ref
from enqueue_recorder import RecordingDevice
from mgr_amd import configs
from mgr_amd.engine import Engine
from mgr_amd.live import LiveSession, plan_windows
from oracle import keras_ref as kr
from oracle import network_ref as nr

SPECS = {
    "audio": lambda: configs.audio_spec(7, 5, h=6),
    "audio1": lambda: configs.audio_spec(7, 5, h=6, layers=1),
    "fusion": lambda: configs.fusion_spec(7, 4, 5, h_audio=6, h_skeletal=5, h_fusion=3),
}


def _case(name, n, seed=0):
    rng = np.random.default_rng(seed)
    sd = SPECS[name]().to_dict()
    w = nr.init_weights(sd, rng)
    for k in w:     # (biases and the Dense layer off their initial zeros)
        w[k] = w[k] + 0.1 * rng.standard_normal(w[k].shape)
    x = {s["name"]: rng.standard_normal((n, s["F"])) for s in sd["streams"]}
    return sd, w, x


# ---- the window plan ----------------------------------------------------------------------------------------------------------------
def test_plan_windows_covers_every_frame_once():
    for n, chunk, look in itertools.product(range(13), range(1, 6), range(6)):
        ws = list(plan_windows(n, chunk, look))
        kept = [t for s0, nv, nk in ws for t in range(s0, s0 + nk)]
        assert kept == list(range(n)), (n, chunk, look)
        for k, (s0, nv, nk) in enumerate(ws):
            assert s0 == k * chunk and nv == min(chunk + look, n - s0) and nk == min(chunk, n - s0) and 1 <= nk <= nv
        if ws:
            assert ws[-1][0] + ws[-1][1] == n     # the last window reaches the end of the session


def test_plan_windows_refuses_bad_arguments():
    for bad in ((5, 0, 1), (5, 2, -1), (-1, 2, 1)):
        with pytest.raises(ValueError):
            list(plan_windows(*bad))


# ---- the restatement against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
def test_scan_with_zero_state_is_the_oracles_lstm(reverse):
    rng = np.random.default_rng(1)
    T, F, H = 9, 4, 5
    x, W, U, b = rng.standard_normal((T, F)), rng.standard_normal((F, 4 * H)), rng.standard_normal((H, 4 * H)), rng.standard_normal(4 * H)
    y, _ = live_ref.scan(x @ W + b, U, None, None, reverse)
    ref, _ = kr.lstm_forward(x[None], W, U, b, reverse=reverse)
    assert np.abs(y - ref[0]).max() <= 1e-12


@pytest.mark.parametrize("name", sorted(SPECS))
def test_one_window_is_the_offline_network(name):
    """case (a): chunk >= n_frames - residual, concat and fusion layer included."""
    sd, w, x = _case(name, 11)
    ref, _ = nr.forward(sd, w, {k: v[None] for k, v in x.items()})
    for chunk, look in ((11, 0), (20, 3)):
        assert np.abs(live_ref.run_session(sd, w, x, chunk, look) - ref[0]).max() <= 1e-12


@pytest.mark.parametrize("name", sorted(SPECS))
@pytest.mark.parametrize("chunk", [1, 3, 5])
def test_full_lookahead_is_the_offline_network(name, chunk):
    """case (b): lookahead >= n_frames - every kept frame sees its whole future, the forward state is carried across windows."""
    sd, w, x = _case(name, 11, seed=2)
    ref, _ = nr.forward(sd, w, {k: v[None] for k, v in x.items()})
    assert np.abs(live_ref.run_session(sd, w, x, chunk, 11) - ref[0]).max() <= 1e-12


def test_a_short_lookahead_differs_and_a_carried_state_matters():
    """The restatement is not vacuous: a truncated future changes the result, and so does dropping the carried state."""
    sd, w, x = _case("audio", 11, seed=3)
    ref, _ = nr.forward(sd, w, {k: v[None] for k, v in x.items()})
    assert np.abs(live_ref.run_session(sd, w, x, 3, 1) - ref[0]).max() > 1e-6
    net = live_ref.Network(sd, w)
    net.window({k: v[:4] for k, v in x.items()}, 4)
    b = net.window({k: v[4:] for k, v in x.items()}, 7)
    fresh = live_ref.Network(sd, w).window({k: v[4:] for k, v in x.items()}, 7)
    assert np.abs(b - fresh).max() > 1e-6


# ---- the carried-run collapse -------------------------------------------------------------------------------------------------------
def test_carried_collapse_equals_offline_collapse_for_every_cut():
    blank = 2
    for n in range(7):
        for labels in itertools.product(range(3), repeat=n):
            want = live_ref.collapse_offline(labels, blank)
            for cuts in itertools.product((0, 1), repeat=max(n - 1, 0)):      # cuts[i]: a window ends behind frame i
                st, got, lo = live_ref.GreedyState(blank, 0), [], 0
                for i in range(n):
                    if i == n - 1 or cuts[i]:
                        got += st.labels(labels[lo:i + 1], [0.5] * (i + 1 - lo), flush=i == n - 1)
                        lo = i + 1
                assert [e[:3] for e in got] == want, (labels, cuts)


def test_carried_collapse_skip_and_confidence():
    st = live_ref.GreedyState(blank=3, skip=2)
    p = np.float32([0.9, 0.8, 0.7, 0.6, 0.5, 0.4])
    ev = st.labels([1, 1, 1, 1, 3, 0], p[:6][:6], flush=False)
    assert ev == [(1, 2, 3, float((np.float32(0.7) + np.float32(0.6)) / np.float32(2)))]
    assert st.labels([], [], flush=True) == [(0, 5, 5, float(np.float32(0.4)))]
    assert st.labels([], [], flush=True) == []


# ---- LiveSession's host side on a device that records calls -------------------------------------------------------------------------
def _recorded(spec, S, chunk, look):
    dev = RecordingDevice()
    eng = Engine(spec, 2, 8, 4, device=dev, inference_only=True)
    n0 = len(dev.trace)
    live = eng.open_live(S, chunk, look)
    return dev, eng, live, n0


def _calls(dev, since, name):
    return [ln for ln in dev.trace[since:] if ln.startswith(name + "(")]


def test_live_session_buffering_and_calls():
    spec = SPECS["fusion"]()
    dev, eng, live, _ = _recorded(spec, 3, 4, 2)
    fa, fs = (lambda n: {"the_input_audio": np.ones((n, 7)), "the_input_skeletal": np.ones((n, 4))}), None
    mark = len(dev.trace)
    # nothing buffered: no device call at all
    assert [r.n_keep for r in live.step()] == [0, 0, 0] and len(dev.trace) == mark
    live.push(0, fa(5))
    assert live.pending(0) == 5 and [r.n_keep for r in live.step()] == [0, 0, 0] and len(dev.trace) == mark     # less than a window
    live.push(0, fa(1))
    live.push(2, fa(3))
    live.end(2)
    res = live.step()
    assert [r.n_keep for r in res] == [4, 0, 3] and live.pending(0) == 2 and live.pending(2) == 0 and live.done(2)
    # one window: 3 depths (two encoder depths, the fusion layer) -> 3 window scans, 2 x 2 x 2 + 2 projections, one Dense, one decode
    assert len(_calls(dev, mark, "mgr_lstm_scan_window")) == 3
    assert len(_calls(dev, mark, "mgr_lstm_input_proj")) == 10
    assert len(_calls(dev, mark, "mgr_dense_softmax_fwd")) == 1 and len(_calls(dev, mark, "mgr_live_greedy")) == 1
    # none of the engine's own step calls
    assert not _calls(dev, mark, "mgr_lstm_scan_fwd_multi_ex") and not _calls(dev, mark, "mgr_lstm_scan_fwd_multi")
    # an ended slot takes no more frames and no more windows until it is reset
    with pytest.raises(ValueError):
        live.push(2, fa(1))
    mark = len(dev.trace)
    assert [r.n_keep for r in live.step()] == [0, 0, 0] and len(dev.trace) == mark
    live.reset(2)
    assert not live.done(2)
    live.push(2, fa(6))
    live.end(0)
    assert [r.n_keep for r in live.step()] == [2, 0, 4] and live.done(0) and live.pending(2) == 2
    # ending with nothing buffered still flushes the decode once
    live.reset(0)
    live.end(0)
    mark = len(dev.trace)
    assert [r.n_keep for r in live.step()] == [0, 0, 0] and len(_calls(dev, mark, "mgr_live_greedy")) == 1 and live.done(0)


def test_live_session_plan_follows_plan_windows():
    """A slot fed a whole session and ended runs exactly plan_windows' windows."""
    spec = SPECS["audio"]()
    for n, chunk, look in ((11, 3, 2), (4, 5, 5), (10, 5, 0), (1, 1, 0)):
        dev, eng, live, _ = _recorded(spec, 1, chunk, look)
        live.push(0, {"the_input": np.zeros((n, 7))})
        live.end(0)
        got = []
        while not live.done(0):
            nv, nk, fl = live._plan()
            got.append((n - live.pending(0), int(nv[0]), int(nk[0])))
            live.step()
        assert got == list(plan_windows(n, chunk, look)) and int(fl[0]) == 1


def test_live_session_refusals():
    spec = SPECS["fusion"]()
    dev, eng, live, _ = _recorded(spec, 2, 4, 2)
    with pytest.raises(ValueError):
        live.push(0, {"the_input_audio": np.ones((3, 7))})                                        # a stream is missing
    with pytest.raises(ValueError):
        live.push(0, {"the_input_audio": np.ones((3, 7)), "the_input_skeletal": np.ones((2, 4))})  # different frame counts
    with pytest.raises(ValueError):
        live.push(0, {"the_input_audio": np.ones((3, 6)), "the_input_skeletal": np.ones((3, 4))})  # wrong width
    with pytest.raises(IndexError):
        live.push(2, {})
    assert live.pending(0) == 0
    with pytest.raises(NotImplementedError, match="front-end"):
        LiveSession(types.SimpleNamespace(spec=configs.rgb_spec(h=4)), 1, 2, 1)      # (refused before the engine is looked at)
    with pytest.raises(ValueError):
        eng.open_live(0, 4, 2)


def test_opening_no_live_session_changes_nothing():
    """An engine that never opens a live session allocates and calls exactly what it did: open_live is the only entry."""
    spec = SPECS["fusion"]()
    a, b = RecordingDevice(), RecordingDevice()
    Engine(spec, 2, 8, 4, device=a, inference_only=True)
    eb = Engine(spec, 2, 8, 4, device=b, inference_only=True)
    assert a.trace == b.trace
    n = len(b.trace)
    eb.open_live(1, 4, 2)
    assert a.trace == b.trace[:n] and len(b.trace) > n


# ---- the facade: Model.open_live and the decode modules' decode_live ----------------------------------------------------------------
def _answering_device():
    """A RecordingDevice whose read-backs hold int32 ones: every window then reports ONE event, (label 1, frames 1 .. 1)."""
    import ctypes as C
    dev = RecordingDevice()
    call = dev.lib._call

    def answering(name, args):
        r = call(name, args)
        if name == "mgr_d2h":
            n = int(args[3]) // 4
            (C.c_int32 * n).from_address(int(args[1]))[:] = [1] * n
        return r
    dev.lib._call = answering
    return dev


def _facade_cases():
    from mgr_amd.audio_network import sequence_decoding as audio
    from mgr_amd.early_fusion import sequence_decoding as early
    from mgr_amd.multimodal_fusion import sequence_decoding as fusion
    return {"audio": (audio, configs.audio_spec(7, 44, h=6), {"the_input": 7}),
            "fusion": (fusion, configs.fusion_spec(7, 4, 22, h_audio=6, h_skeletal=5, h_fusion=3), {"the_input_audio": 7, "the_input_skeletal": 4}),
            "early": (early, configs.early_fusion_spec(7, 4, 22, h=6), {"the_input_audio": 7, "the_input_skeletal": 4})}


@pytest.mark.parametrize("name", ["audio", "fusion", "early"])
def test_model_open_live_and_decode_live_take_graph_input_names(name):
    from mgr_amd.keras_like import Model
    module, spec, inputs = _facade_cases()[name]
    n, chunk, look = 11, 4, 2
    rng = np.random.default_rng(0)
    x = {k: rng.standard_normal((n, F)).astype(np.float32) for k, F in inputs.items()}
    model = Model(spec, device=_answering_device())
    # Model.open_live: push is keyed by the graph's input names; a concatenated stream gets its inputs side by side, in order
    live = model.open_live(1, chunk, look)
    live.push(0, x)
    for s in spec.streams:
        want = np.concatenate([x[k] for k in s["inputs"]], axis=1) if s.get("inputs") else x[s["name"]]
        assert np.array_equal(live.slots[0].buf[s["name"]], want)
    live.close()
    with pytest.raises(RuntimeError, match="closed"):
        live.step()
    # decode_live: one (name, first, last, confidence) per event, names through the module's class map
    pieces = ({k: v[s0:s0 + 3] for k, v in x.items()} for s0 in range(0, n, 3))
    got = list(module.decode_live(model, pieces, chunk, look))
    assert [g[:3] for g in got] == [(module.map_gest[1], 1, 1)] * len(list(plan_windows(n, chunk, look)))
    # the session ends with its engine: another batch shape rebuilds it, and the next call says so
    live = model.open_live(1, chunk, look)
    model._ensure_engine(1, 5, 1, inference_only=True)       # (what predict_on_batch does for a batch of another shape)
    with pytest.raises(RuntimeError, match="engine was closed"):
        live.push(0, x)


def test_rgb_decode_live_refuses_the_front_end():
    from mgr_amd.keras_like import Model
    from mgr_amd.rgb_network import decode_rgb
    model = Model(configs.rgb_spec(h=4), device=RecordingDevice())
    with pytest.raises(NotImplementedError, match="front-end"):
        next(decode_rgb.decode_live(model, iter([{"the_input": np.zeros((2, 60, 60, 1))}]), 2, 1))


def test_a_cap_below_what_a_window_can_finalise_is_refused():
    dev, eng, live, _ = _recorded(SPECS["audio"](), 1, 4, 2)
    assert live.cap == 6 and eng.open_live(1, 4, 2, cap=9).cap == 9
    with pytest.raises(ValueError, match="cap"):
        eng.open_live(1, 4, 2, cap=5)
