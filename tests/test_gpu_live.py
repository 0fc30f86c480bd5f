"""-m gpu: live sessions through whole networks (Engine.open_live, mgr_amd/live.py): the two cases in which a live
session must give the offline network's posteriors, a short lookahead against the fp64 restatement, several sessions in one
LiveSession, the engine's own predict left alone, set_weights seen by the next window, the specs that are refused, and the facade:
Model.open_live and the decode modules' decode_live by the graph's input names (early fusion included)."""
import numpy as np
import pytest

import live_ref
from helpers import rel_err
from mgr_amd import configs, decoding
from mgr_amd.engine import Engine
from mgr_amd.live import run_session
from oracle import network_ref as nr

pytestmark = pytest.mark.gpu

f32 = np.float32
N = 37
SPECS = {
    "audio": lambda: configs.audio_spec(39, 22, h=32),
    "skeletal": lambda: configs.skeletal_spec(20, 22, h=24),
    "fusion": lambda: configs.fusion_spec(h_audio=32, h_skeletal=24, h_fusion=16),
}


def _weights(sd, rng):
    """The initialisation recipe with the biases and the Dense layer off their initial values and input kernels large enough for
    gates that move (pre-activations of order 1 at every width); the recurrent matrices stay orthogonal, so the fp32 and the fp64
    recursions do not drift apart over a session."""
    w = nr.init_weights(sd, rng, dtype=np.float32)
    for k in w:
        if k.endswith("/U"):
            continue
        scale = 0.1 if w[k].ndim == 1 else 1.0 / np.sqrt(w[k].shape[0])
        w[k] = (w[k] + scale * rng.standard_normal(w[k].shape)).astype(f32)
    return w


def _make(device, name, n=N, seed=0, spec=None):
    rng = np.random.default_rng(seed)
    spec = spec or SPECS[name]()
    sd = spec.to_dict()
    w = _weights(sd, rng)
    x = {s["name"]: rng.standard_normal((n, s["F"])).astype(f32) for s in sd["streams"]}
    eng = Engine(spec, 1, n, 4, device=device, inference_only=True)
    eng.set_weights(w)
    return eng, sd, w, x


def _pieces(x, sizes):
    """The session cut into pushes of the given sizes (cycled)."""
    n, s0, i = next(iter(x.values())).shape[0], 0, 0
    while s0 < n:
        k = sizes[i % len(sizes)]
        yield {name: v[s0:s0 + k] for name, v in x.items()}
        s0, i = s0 + k, i + 1


def _live(eng, x, chunk, look, sizes=(4, 1, 9), slot=0, sessions=1):
    """One session through a fresh LiveSession: (posteriors (n, C), events)."""
    live = eng.open_live(sessions, chunk, look)
    rows, events = [], []
    for res in run_session(live, slot, _pieces(x, sizes), posteriors=True):
        rows.append(res.posteriors)
        events += res.events
    live.close()
    return np.concatenate(rows), events


@pytest.fixture(scope="module", params=sorted(SPECS))
def net(request, device):
    eng, sd, w, x = _make(device, request.param)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    x64 = {k: v.astype(np.float64) for k, v in x.items()}
    ref, _ = nr.forward(sd, w64, {k: v[None] for k, v in x64.items()})
    yield dict(eng=eng, sd=sd, w=w, w64=w64, x=x, x64=x64, ref=ref[0])
    eng.close()


def test_one_window_is_the_offline_network(net):
    """case (a): chunk >= n_frames."""
    P, _ = _live(net["eng"], net["x"], N, 0)
    assert P.shape == net["ref"].shape and rel_err(P, net["ref"]) < 1e-4
    P, _ = _live(net["eng"], net["x"], N + 3, 2)
    assert rel_err(P, net["ref"]) < 1e-4


def test_full_lookahead_is_the_offline_network(net):
    """case (b): chunk = 5, lookahead >= n_frames - the carried forward states against the independent oracle."""
    P, _ = _live(net["eng"], net["x"], 5, N)
    assert P.shape == net["ref"].shape and rel_err(P, net["ref"]) < 1e-4


def test_short_lookahead_is_the_restatement(net):
    want = live_ref.run_session(net["sd"], net["w64"], net["x64"], 5, 3)
    P, events = _live(net["eng"], net["x"], 5, 3)
    assert rel_err(P, want) < 1e-4
    assert rel_err(want, net["ref"]) > 1e-3          # (the truncated future is visible: this is not the offline result again)
    # the events are the carried decode of exactly these posteriors
    C = P.shape[1]
    assert events == [e for e in decoding.greedy_segments(P[None], -1, skip=2, dev=net["eng"].dev)[0] if e[0] != C - 1]
    # however the frames are pushed, the windows - and so the bits - are the same
    P2, ev2 = _live(net["eng"], net["x"], 5, 3, sizes=(N,))
    assert np.array_equal(P, P2) and events == ev2


def test_predict_is_untouched_by_a_live_run(net):
    eng = net["eng"]
    batch = {k: v[None] for k, v in net["x"].items()}
    before = eng.predict(batch)
    _live(eng, net["x"], 5, 3)
    assert np.array_equal(eng.predict(batch), before)
    assert rel_err(before[0], net["ref"]) < 1e-4


def test_two_sessions_one_ending_and_a_new_one_in_the_freed_slot(net):
    """Sessions of different lengths side by side, one ending while the other goes on, then a new session in the freed slot after
    reset: each `==` its solo run in the same configuration (same number of slots, same slot)."""
    eng, x = net["eng"], net["x"]
    chunk, look = 5, 3
    xa = x
    xb = {k: v[:13] for k, v in x.items()}
    xc = {k: v[7:31][::-1].copy() for k, v in x.items()}
    solo = {key: _live(eng, xs, chunk, look, slot=slot, sessions=2) for key, xs, slot in (("a", xa, 0), ("b", xb, 1), ("c", xc, 1))}
    live = eng.open_live(2, chunk, look)
    rows, events = {k: [] for k in "abc"}, {k: [] for k in "abc"}

    def step(keys):
        for slot, res in enumerate(live.step(posteriors=True)):
            if res.n_keep or res.events:
                rows[keys[slot]].append(res.posteriors)
                events[keys[slot]] += res.events

    fed_a = 0
    live.push(1, xb)                       # b arrives at once and ends; a trickles in
    live.end(1)
    on1 = "b"
    while fed_a < N or not live.done(0):
        if fed_a < N:
            live.push(0, {k: v[fed_a:fed_a + 6] for k, v in xa.items()})
            fed_a += 6
            if fed_a >= N:
                live.end(0)
        step({0: "a", 1: on1})
        if on1 == "b" and live.done(1):     # the freed slot takes a new session while a goes on
            live.reset(1)
            live.push(1, xc)
            live.end(1)
            on1 = "c"
    while not live.done(1):
        step({0: "a", 1: on1})
    live.close()
    for key in "abc":
        assert np.array_equal(np.concatenate(rows[key]), solo[key][0]), key
        assert events[key] == solo[key][1], key


def test_set_weights_is_seen_by_the_next_session(device):
    eng, sd, w, x = _make(device, "audio", seed=5)
    live = eng.open_live(1, 5, 3)
    first = np.concatenate([r.posteriors for r in run_session(live, 0, _pieces(x, (7,)), posteriors=True)])
    w2 = _weights(sd, np.random.default_rng(77))
    eng.set_weights(w2)
    live.reset(0)
    second = np.concatenate([r.posteriors for r in run_session(live, 0, _pieces(x, (7,)), posteriors=True)])
    want = live_ref.run_session(sd, {k: v.astype(np.float64) for k, v in w2.items()}, {k: v.astype(np.float64) for k, v in x.items()}, 5, 3)
    assert rel_err(second, want) < 1e-4 and rel_err(first, want) > 1e-3
    eng.close()


def test_reference_sizes(device):
    """The fusion network at the reference's sizes (H = 500, 300, 100): 45 frames, chunk = 20, lookahead = 5."""
    eng, sd, w, x = _make(device, None, n=45, seed=9, spec=configs.fusion_spec())
    want = live_ref.run_session(sd, {k: v.astype(np.float64) for k, v in w.items()}, {k: v.astype(np.float64) for k, v in x.items()}, 20, 5)
    P, _ = _live(eng, x, 20, 5)
    assert P.shape == want.shape and rel_err(P, want) < 1e-4
    eng.close()


def test_refused_specs(device):
    eng = Engine(configs.rgb_spec(h=8), 1, 4, 2, device=device, inference_only=True)
    with pytest.raises(NotImplementedError, match="front-end"):
        eng.open_live(1, 2, 1)
    eng.close()


# ---- the facade: Model.open_live and the decode modules' decode_live ----------------------------------------------------------------
def _facade_cases():
    from mgr_amd.audio_network import sequence_decoding as audio
    from mgr_amd.early_fusion import sequence_decoding as early
    from mgr_amd.multimodal_fusion import sequence_decoding as fusion
    return {"audio": (audio, configs.audio_spec(39, 44, h=32)),
            "fusion": (fusion, configs.fusion_spec(h_audio=32, h_skeletal=24, h_fusion=16)),
            "early": (early, configs.early_fusion_spec(h=32))}


@pytest.mark.parametrize("name", ["audio", "fusion", "early"])
def test_decode_live_through_the_model(device, name):
    """The decode module's decode_live over a keras_like.Model, fed by the graph's input names (early fusion: the two inputs of the
    concatenated stream): the names and frames are those of a LiveSession on the model's engine run by stream name, through the
    module's class map; the posteriors behind them are the fp64 restatement's."""
    from mgr_amd.keras_like import Model
    module, spec = _facade_cases()[name]
    sd = spec.to_dict()
    rng = np.random.default_rng(11)
    w = _weights(sd, rng)
    names = [k for s in spec.streams for k in (s.get("inputs") or [s["name"]])]
    widths = dict(the_input=39, the_input_audio=39, the_input_skeletal=20)
    x = {k: rng.standard_normal((N, widths[k])).astype(f32) for k in names}
    by_stream = {s["name"]: (np.concatenate([x[k] for k in s["inputs"]], axis=1) if s.get("inputs") else x[s["name"]]) for s in spec.streams}
    model = Model(spec, device=device)
    model.set_weights_dict(w)
    got = list(module.decode_live(model, _pieces(x, (4, 1, 9)), 5, 3))
    P, events = _live(model._engine, by_stream, 5, 3)
    assert got == [(module.map_gest[lab], first, last, conf) for lab, first, last, conf in events]
    want = live_ref.run_session(sd, {k: v.astype(np.float64) for k, v in w.items()}, {k: v.astype(np.float64) for k, v in by_stream.items()}, 5, 3)
    assert rel_err(P, want) < 1e-4
    assert events                  # (the comparison above is about something)
    # Model.open_live itself, posteriors on request
    live = model.open_live(1, 5, 3)
    rows = [r.posteriors for r in run_session(live, 0, _pieces(x, (N,)), posteriors=True)]
    assert np.array_equal(np.concatenate(rows), P)
    model._engine.close()


def test_rgb_decode_live_refuses_the_front_end(device):
    from mgr_amd.keras_like import Model
    from mgr_amd.rgb_network import decode_rgb
    model = Model(configs.rgb_spec(h=8), device=device)
    with pytest.raises(NotImplementedError, match="front-end"):
        next(decode_rgb.decode_live(model, iter([{"the_input": np.zeros((2, 60, 60, 1), f32)}]), 2, 1))
    if model._engine is not None:
        model._engine.close()
