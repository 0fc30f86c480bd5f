"""-m gpu: the entropy-regularised training mode (Engine.set_entropy / Model.set_entropy) - one training step's dLogits and
both loss parts against a direct mgr_ctc_entropy_grad call on the step's own downloaded posteriors, bit for bit; the logged scalars;
the mode off is the step it was; the refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

B, T, LMAX = 3, 24, 6
CFG = dict(weight=0.3)
RISK = dict(top_paths=4, beam_width=8)


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
    w["dense/W"] = w["dense/W"] * 40.0        # (posteriors away from uniform)
    eng.set_weights(w)
    return eng, synthetic_arrays(spec, B, T, LMAX, 9, lmin=2, lmax=5)


def _direct(device, P, labels, il, ll, skip, eps, loss_scale, ent_scale):
    """mgr_ctc_entropy_grad on host posteriors: (loss, H, dLogits)"""
    Bn, Tn, Cn = P.shape
    lab = np.ascontiguousarray(labels, np.int32)
    held = [device.array(np.ascontiguousarray(P, np.float32)), device.array(lab), device.array(np.asarray(il).reshape(-1).astype(np.int32)),
            device.array(np.asarray(ll).reshape(-1).astype(np.int32)), device.empty((Bn,)), device.empty((Bn,)), device.empty((Bn, Tn, Cn)),
            device.bytes(2 * device.lib.mgr_ctc_ws_bytes(Bn, Tn, Cn, lab.shape[1]))]
    try:
        device.call("mgr_ctc_entropy_grad", *held[:4], Bn, Tn, Cn, lab.shape[1], skip, Cn - 1, eps, loss_scale, ent_scale, *held[4:7], held[7],
                    held[7].nbytes)
        return held[4].download(), held[5].download(), held[6].download()
    finally:
        for a in held:
            a.free()


@pytest.mark.parametrize("kind", ["fusion", "trainable"])
@pytest.mark.parametrize("head_dropout", [False, True])
def test_one_entropy_step_against_a_direct_call(device, kind, head_dropout):
    spec = _spec(kind, head_dropout)
    eng, (xs, labels, il, ll) = _engine(device, spec)
    try:
        eng.set_entropy(CFG)
        loss = eng.train_step(xs, labels, il, ll, apply_update=False)
        eng.dev.sync()
        P, dL = eng.P.download(), eng.dLogits.download()
        skip, eps = int(spec.ctc["skip"]), float(spec.ctc["eps"])
        lab = np.where(np.isfinite(labels) & (np.asarray(labels) >= 0), labels, -1)
        lo, H, dz = _direct(device, P, lab, il, ll, skip, eps, 1.0 / B, CFG["weight"] / B)
        assert np.array_equal(dL.view(np.uint32), dz.view(np.uint32))
        assert np.array_equal(eng.loss_b.download().view(np.uint32), lo.view(np.uint32))
        assert np.array_equal(eng._entropy["H"].download().view(np.uint32), H.view(np.uint32))
        assert (H > 0).all() and np.isfinite(lo).all() and np.abs(dz).max() > 1e-4
        # the two means are float32 means of those arrays; the loss read is their combination
        assert abs(eng.last_ctc_loss - float(lo.astype(np.float64).mean())) <= 1e-5 * abs(eng.last_ctc_loss)
        assert abs(eng.last_entropy - float(H.astype(np.float64).mean())) <= 1e-5 * abs(eng.last_entropy)
        want = eng.last_ctc_loss - CFG["weight"] * eng.last_entropy
        assert abs(loss - want) <= 1e-5 * abs(want) and eng.last_risk is None
        # the entropy term shows in the gradient: it differs from the loss's own
        _, _, plain = _direct(device, P, lab, il, ll, skip, eps, 1.0 / B, 0.0)
        assert np.abs(dz - plain).max() > 1e-3 * np.abs(plain).max()
    finally:
        eng.close()


def test_the_mode_off_is_the_step_it_was(device):
    """set_entropy(cfg), one step without an update, set_entropy(None): the next step gives the bits of an engine that never had the mode
    (which ran a plain step without an update in its place: the same draws of randomness)."""
    spec = _spec("fusion", True)
    out = []
    for with_cfg in (True, False):
        eng, (xs, labels, il, ll) = _engine(device, spec)
        try:
            if with_cfg:
                eng.set_entropy(CFG)
            eng.train_step(xs, labels, il, ll, apply_update=False)
            eng.set_entropy(None)
            assert eng._entropy is None
            loss = eng.train_step(xs, labels, il, ll)
            assert eng.last_entropy is None and eng.last_ctc_loss is None
            eng.dev.sync()
            out.append((loss, eng.dLogits.download(), eng.get_weights()))
        finally:
            eng.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
    for k, v in out[0][2].items():
        assert np.array_equal(v, out[1][2][k]), k


def test_a_loss_is_read_as_its_own_steps_whatever_the_mode_is_by_then(device):
    spec = _spec("fusion", False)
    eng, (xs, labels, il, ll) = _engine(device, spec)
    try:
        eng.set_entropy(CFG)
        eng.enqueue_train_step(xs, labels, il, ll, None, False)
        eng.set_entropy(None)                                    # (an entropy step is enqueued and unread)
        loss = eng.read_loss()
        ctc, H = float(eng.loss_host[0]), float(eng.loss_host[1])
        assert (eng.last_ctc_loss, eng.last_entropy) == (ctc, H) and loss == ctc - CFG["weight"] * H and H > 0 and ctc > 0
        eng.enqueue_train_step(xs, labels, il, ll, None, False)
        eng.set_entropy(dict(weight=0.9))                        # (a plain step is enqueued and unread)
        assert eng.read_loss() == float(eng.loss_host[0]) and eng.last_entropy is None and eng.last_ctc_loss is None
    finally:
        eng.close()


def test_refusals(device):
    from mgr_amd import keras_like as K

    class Comm:
        rank = 0

    eng, _ = _engine(device, _spec("fusion", False), comm=Comm())
    try:
        with pytest.raises(NotImplementedError):
            eng.set_entropy(CFG)
        assert eng._entropy is None
        eng.comm = None
        with pytest.raises(ValueError):
            eng.set_entropy(dict(wieght=0.1))                    # an unknown setting
        with pytest.raises(ValueError):
            eng.set_entropy(dict(weight=-0.1))
        eng.set_entropy({})
        assert eng._entropy["cfg"]["weight"] == eng.ENTROPY_DEFAULTS["weight"] == 0.2
        held = eng._entropy
        with pytest.raises(ValueError):
            eng.set_entropy(dict(weight=-1.0))
        assert eng._entropy is held and held["ws"].ptr              # a refused cfg leaves the mode, and its buffers, as they were
        with pytest.raises(ValueError):
            eng.set_risk(RISK)                                   # not combined, in either order
        assert eng._risk is None
        eng.set_entropy(None)
        eng.set_risk(RISK)
        with pytest.raises(ValueError):
            eng.set_entropy(CFG)
        assert eng._entropy is None and eng._risk is not None
    finally:
        eng.close()
    inf, _ = _engine(device, _spec("fusion", False), inference_only=True)
    try:
        with pytest.raises(ValueError):
            inf.set_entropy(CFG)
    finally:
        inf.close()
    m = K.Model(_spec("fusion", False), device=device)
    m.distribute(Comm(), 2)
    with pytest.raises(NotImplementedError):
        m.set_entropy(CFG)
    m = K.Model(_spec("fusion", False), device=device)
    m.compile(optimizer=K.Adam(lr=1e-3), entropy=CFG)
    with pytest.raises(NotImplementedError):
        m.distribute(Comm(), 2)
    with pytest.raises(ValueError):
        m.set_risk(RISK)
    with pytest.raises(ValueError):
        K.Model(_spec("fusion", False), device=device).compile(optimizer=K.Adam(lr=1e-3), risk=RISK, entropy=CFG)


def test_the_mode_survives_a_rebuilt_engine_and_is_logged(device):
    from mgr_amd import keras_like as K
    from mgr_amd.synthetic import synthetic_arrays
    spec = _spec("fusion", True)
    m = K.Model(spec, device=device, seed=3)
    m.compile(loss={"ctc": lambda a, b: b}, optimizer=K.Adam(lr=1e-3, clipvalue=0.5), entropy=CFG)

    def batch(t):
        xs, labels, il, ll = synthetic_arrays(spec, B, t, LMAX, 9, lmin=2, lmax=5)
        return dict(xs, the_labels=labels, input_length=il, label_length=ll)
    loss = m.train_on_batch(batch(T))
    first = m._engine
    assert first._entropy is not None and set(m.last_logs) == {"loss", "ctc_loss", "entropy"} and m.last_logs["loss"] == loss
    assert abs(loss - (m.last_logs["ctc_loss"] - CFG["weight"] * m.last_logs["entropy"])) <= 1e-5 * abs(loss)
    m.train_on_batch(batch(T + 8))                              # another T: the engine is rebuilt
    assert m._engine is not first and m._engine._entropy is not None and m._engine._entropy["cfg"]["weight"] == CFG["weight"]
    assert "entropy" in m.last_logs

    def gen():
        while True:
            yield batch(T + 8), None
    hist = m.fit_generator(gen(), steps_per_epoch=2, epochs=1, verbose=0)
    assert {"loss", "ctc_loss", "entropy"} <= set(hist.history) and "risk" not in hist.history
    m.set_entropy(None)
    m.train_on_batch(batch(T + 8))
    assert set(m.last_logs) == {"loss"} and m._engine._entropy is None
