"""-m gpu: the minimum-risk training mode (Engine.set_risk / Model.set_risk) - one training step's dLogits, logged scalars
and Dense gradient against the fp64 restatement computed from the step's own downloaded posteriors; the mode off is the step it was."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as blr  # noqa: E402
import edit_ref as er  # noqa: E402
import rescore_cases as rc  # noqa: E402
import risk_ref as kr  # noqa: E402
from oracle import keras_ref as okr  # noqa: E402

pytestmark = pytest.mark.gpu

B, T, LMAX, REL = 3, 24, 6, 1e-4
CFG = dict(top_paths=4, beam_width=8, ctc_weight=0.3, costs=(3, 2, 2), post_scale=0.7)


def _spec(kind, head_dropout):
    from mgr_amd.configs import fusion_spec, skeletal_spec
    spec = fusion_spec(h_audio=8, h_skeletal=8, h_fusion=4) if kind == "fusion" else skeletal_spec(20, 22, h=8, layers=2)
    if not head_dropout:
        spec.head["dropout"] = 0.0
    assert head_dropout == (spec.head["dropout"] > 0)
    return spec


def _engine(device, spec, seed=5, **kw):
    from mgr_amd.engine import Engine
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    eng = Engine(spec, B, T, LMAX, device=device, seed=seed, **kw)
    w = synthetic_weights(spec, 3)
    w["dense/W"] = w["dense/W"] * 40.0        # (posteriors away from uniform: the N-best list is not decided by rounding)
    eng.set_weights(w)
    return eng, synthetic_arrays(spec, B, T, LMAX, 9, lmin=2, lmax=5)


def _restated(P, labels, il, ll, cfg, skip, eps):
    """From the step's posteriors: (dLogits, mean risk, mean CTC loss, the reference search's smallest deciding score gap)."""
    P64 = P.astype(np.float64)
    il, ll = np.asarray(il).reshape(-1), np.asarray(ll).reshape(-1)
    loss, dz = okr.ctc_loss_grad(P64, labels, il, ll, skip=skip, eps=np.float64(np.float32(eps)))
    K = cfg["top_paths"]
    seqs, _, _, gap = blr.beam_search_lm(P, il, beam_width=cfg["beam_width"], top_paths=K, skip=skip, eps=eps)
    hyp, hl = rc.pack([row + [None] * (K - len(row)) for row in seqs], K, T - skip)
    refs = [[int(v) for v in labels[b, :ll[b]]] for b in range(B)]
    risks = np.array([[er.align(seqs[b][k], refs[b], cfg["costs"])[0] if k < len(seqs[b]) else 0 for k in range(K)] for b in range(B)], np.int32)
    r = kr.expected_risk(P, hyp, hl, risks, skip=skip, eps=eps, input_len=il, Lcap=min(255, max(2 * LMAX, 16)), post_scale=cfg["post_scale"],
                         gscale=1.0 / B)
    return cfg["ctc_weight"] / B * dz + r["dlogits"], float(r["risk"].mean()), float(loss.mean()), gap, r


@pytest.mark.parametrize("kind", ["fusion", "trainable"])
@pytest.mark.parametrize("head_dropout", [False, True])
@pytest.mark.parametrize("ctc_weight", [0.3, 0.0])
def test_one_risk_step_against_the_restatement(device, kind, head_dropout, ctc_weight):
    spec = _spec(kind, head_dropout)
    eng, (xs, labels, il, ll) = _engine(device, spec)
    cfg = dict(CFG, ctc_weight=ctc_weight)
    try:
        eng.set_risk(cfg)
        loss = eng.train_step(xs, labels, il, ll, apply_update=False)
        eng.dev.sync()
        P, dL = eng.P.download(), eng.dLogits.download()
        skip, eps = int(spec.ctc["skip"]), float(spec.ctc["eps"])
        want, risk, ctc, gap, r = _restated(P, labels, il, ll, cfg, skip, eps)
        assert gap > 1e-6, gap                                   # (the premise: the reference search's N-best list is well decided)
        assert (r["live"].sum(axis=1) >= 2).all() and np.abs(r["dlogits"]).max() > 1e-5          # ... and the risk term shows
        top = np.abs(want).max()
        assert np.abs(dL - want).max() <= REL * top, (np.abs(dL - want).max(), top)
        assert abs(eng.last_risk - risk) <= REL * max(1.0, abs(risk))
        if ctc_weight:
            assert abs(eng.last_ctc_loss - ctc) <= REL * abs(ctc)
        else:
            assert eng.last_ctc_loss == 0.0                      # (not computed)
        assert abs(loss - (risk + ctc_weight * ctc)) <= REL * abs(risk + ctc_weight * ctc)
        # dense/W's gradient is mgr_dense_bwd of that dLogits (same activations, same dropout mask)
        D, Cn = spec.head_width, spec.num_classes
        feat, ldf = eng._feat
        hm, p_head, hseed = eng._head_args
        dW, db, dA = device.empty((D, Cn)), device.empty((Cn,)), device.empty((B, T, D))
        ws = device.bytes(device.lib.mgr_dense_bwd_ws_bytes(B, T, D, Cn))
        device.call("mgr_dense_bwd", feat, ldf, hm, p_head, C.c_uint64(hseed), eng.dLogits, eng._wview("dense/W"), dW, db, dA, D, B, T, D, Cn,
                    ws, ws.nbytes)
        assert np.array_equal(dW.download().reshape(-1), eng._gview("dense/W").download())
        assert np.array_equal(db.download().reshape(-1), eng._gview("dense/b").download())
        for a in (dW, db, dA, ws):
            a.free()
    finally:
        eng.close()


def test_the_mode_off_is_the_step_it_was(device):
    """set_risk(cfg), one risk step without an update, set_risk(None): the next step gives the bits of an engine that never had a cfg
    (which ran a plain step without an update in its place: the same draws of randomness)."""
    spec = _spec("fusion", True)
    out = []
    for with_cfg in (True, False):
        eng, (xs, labels, il, ll) = _engine(device, spec)
        try:
            if with_cfg:
                eng.set_risk(CFG)
            eng.train_step(xs, labels, il, ll, apply_update=False)
            eng.set_risk(None)
            assert eng._risk is None
            loss = eng.train_step(xs, labels, il, ll)
            assert eng.last_risk is None
            eng.dev.sync()
            out.append((loss, eng.dLogits.download(), eng.get_weights()))
        finally:
            eng.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
    for k, v in out[0][2].items():
        assert np.array_equal(v, out[1][2][k]), k


def test_a_loss_is_read_as_its_own_steps_whatever_the_mode_is_by_then(device):
    """The mode is switched between enqueueing a step and reading its loss: the loss and its parts are those of the step."""
    spec = _spec("fusion", False)
    eng, (xs, labels, il, ll) = _engine(device, spec)
    try:
        eng.set_risk(CFG)
        eng.enqueue_train_step(xs, labels, il, ll, None, False)
        eng.set_risk(None)                                       # (a risk step is enqueued and unread)
        loss = eng.read_loss()
        ctc, risk = float(eng.loss_host[0]), float(eng.loss_host[1])
        assert (eng.last_risk, eng.last_ctc_loss) == (risk, ctc) and loss == risk + CFG["ctc_weight"] * ctc and risk > 0 and ctc > 0
        eng.enqueue_train_step(xs, labels, il, ll, None, False)
        eng.set_risk(dict(CFG, ctc_weight=0.9))                  # (a plain step is enqueued and unread)
        assert eng.read_loss() == float(eng.loss_host[0]) and eng.last_risk is None and eng.last_ctc_loss is None
    finally:
        eng.close()


def test_a_communicator_with_a_risk_cfg_is_refused(device):
    from mgr_amd import keras_like as K

    class Comm:
        rank = 0

    eng, _ = _engine(device, _spec("fusion", False), comm=Comm())
    try:
        with pytest.raises(NotImplementedError):
            eng.set_risk(CFG)
        assert eng._risk is None
        eng.comm = None
        with pytest.raises(ValueError):
            eng.set_risk(dict(CFG, top_path=3))                  # an unknown setting
        with pytest.raises(ValueError):
            eng.set_risk(dict(CFG, top_paths=9))                 # more paths than the beam holds
        eng.set_risk(CFG)
        held = eng._risk
        with pytest.raises(ValueError):
            eng.set_risk(dict(CFG, top_paths=9))
        assert eng._risk is held and held["out"].ptr                  # a refused cfg leaves the mode, and its buffers, as they were
    finally:
        eng.close()
    m = K.Model(_spec("fusion", False), device=device)
    m.distribute(Comm(), 2)
    with pytest.raises(NotImplementedError):
        m.set_risk(CFG)
    m = K.Model(_spec("fusion", False), device=device)
    m.compile(optimizer=K.Adam(lr=1e-3), risk=CFG)
    with pytest.raises(NotImplementedError):
        m.distribute(Comm(), 2)


def test_the_mode_survives_a_rebuilt_engine_and_is_logged(device):
    from mgr_amd import keras_like as K
    from mgr_amd.synthetic import synthetic_arrays
    spec = _spec("fusion", True)
    m = K.Model(spec, device=device, seed=3)
    m.compile(loss={"ctc": lambda a, b: b}, optimizer=K.Adam(lr=1e-3, clipvalue=0.5), risk=CFG)

    def batch(t):
        xs, labels, il, ll = synthetic_arrays(spec, B, t, LMAX, 9, lmin=2, lmax=5)
        return dict(xs, the_labels=labels, input_length=il, label_length=ll)
    loss = m.train_on_batch(batch(T))
    first = m._engine
    assert first._risk is not None and set(m.last_logs) == {"loss", "risk", "ctc_loss"} and m.last_logs["loss"] == loss
    assert abs(loss - (m.last_logs["risk"] + CFG["ctc_weight"] * m.last_logs["ctc_loss"])) <= 1e-5 * abs(loss)
    m.train_on_batch(batch(T + 8))                              # another T: the engine is rebuilt
    assert m._engine is not first and m._engine._risk is not None and m._engine._risk["cfg"]["top_paths"] == CFG["top_paths"]
    assert "risk" in m.last_logs

    def gen():
        while True:
            yield batch(T + 8), None
    hist = m.fit_generator(gen(), steps_per_epoch=2, epochs=1, verbose=0)
    assert {"loss", "risk", "ctc_loss"} <= set(hist.history)
    m.set_risk(None)
    m.train_on_batch(batch(T + 8))
    assert set(m.last_logs) == {"loss"} and m._engine._risk is None
