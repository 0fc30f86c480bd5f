"""-m gpu: the minimum-risk training mode with SAMPLED hypothesis sets (Engine.set_risk(source="sample")) - one training
step's hypothesis arrays `==` the restatement's (tests/sample_ref.py on the step's own downloaded posteriors and seed), its dLogits and
logged scalars against the fp64 restatement of the risk over that set; reproducibility, buffers, refusals, the mode off, the facade."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_ref as er  # noqa: E402
import risk_ref as kr  # noqa: E402
import sample_ref as sr  # noqa: E402
from oracle import keras_ref as okr  # noqa: E402

pytestmark = pytest.mark.gpu

B, T, LMAX, REL = 3, 24, 6, 1e-4
# (max_labels = T - skip: a sampled labelling can be as long as the frames, and every one of them is to be scored)
CFG = dict(source="sample", top_paths=6, ctc_weight=0.3, costs=(3, 2, 2), post_scale=0.7, max_labels=22)
WORST = [0.0]


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
    w["dense/W"] = w["dense/W"] * 40.0        # (posteriors away from uniform: draws agree often enough for the merge to show)
    eng.set_weights(w)
    return eng, synthetic_arrays(spec, B, T, LMAX, 9, lmin=2, lmax=5)


def _hyp_arrays(eng):
    r = eng._risk
    return tuple(r[k].download() for k in ("out", "out_len", "count", "n_unique"))


def _restated(P, labels, il, ll, cfg, skip, eps, seed):
    """From the step's posteriors and kernel seed: (dLogits, mean risk, mean CTC loss, the hypothesis arrays, risk_ref's dict)."""
    il, ll = np.asarray(il).reshape(-1), np.asarray(ll).reshape(-1)
    Cn, K = P.shape[2], cfg["top_paths"]
    loss, dz = okr.ctc_loss_grad(P.astype(np.float64), labels, il, ll, skip=skip, eps=np.float64(np.float32(eps)))
    hyp = sr.sample_paths(P, il, skip, Cn - 1, eps, seed, K)
    out, out_len = hyp[0], hyp[1]
    refs = [[int(v) for v in labels[b, :ll[b]]] for b in range(B)]
    risks = np.array([[er.align([int(v) for v in out[b, k, :max(out_len[b, k], 0)]], refs[b], cfg["costs"])[0] for k in range(K)]
                      for b in range(B)], np.int32)
    r = kr.expected_risk(P, out, out_len, risks, skip=skip, eps=eps, input_len=il, Lcap=cfg["max_labels"], post_scale=cfg["post_scale"],
                         gscale=1.0 / B)
    return cfg["ctc_weight"] / B * dz + r["dlogits"], float(r["risk"].mean()), float(loss.mean()), hyp, r


@pytest.mark.parametrize("kind", ["fusion", "trainable"])
@pytest.mark.parametrize("head_dropout", [False, True])
@pytest.mark.parametrize("ctc_weight", [0.3, 0.0])
def test_one_sampled_risk_step_against_the_restatement(device, kind, head_dropout, ctc_weight):
    spec = _spec(kind, head_dropout)
    eng, (xs, labels, il, ll) = _engine(device, spec)
    cfg = dict(CFG, ctc_weight=ctc_weight)
    try:
        assert eng.last_sample_seed is None
        eng.set_risk(cfg)
        loss = eng.train_step(xs, labels, il, ll, apply_update=False)
        eng.dev.sync()
        P, dL = eng.P.download(), eng.dLogits.download()
        skip, eps = int(spec.ctc["skip"]), float(spec.ctc["eps"])
        assert 0 <= eng.last_sample_seed < 2 ** 64
        want, risk, ctc, hyp, r = _restated(P, labels, il, ll, cfg, skip, eps, eng.last_sample_seed)
        for name, g, w in zip(("out", "out_len", "count", "n_unique"), _hyp_arrays(eng), hyp):
            assert np.array_equal(g, w), name
        print("unique labellings per sample", hyp[3], "live", r["live"].sum(axis=1))
        assert np.array_equal(r["live"], hyp[1] >= 0)                      # every sampled labelling is feasible and scored
        assert (r["live"].sum(axis=1) >= 2).any() and np.abs(r["dlogits"]).max() > 1e-5          # the risk term shows
        top = np.abs(want).max()
        dev_gap = np.abs(dL - want).max() / top
        WORST[0] = max(WORST[0], dev_gap)
        print("sampled risk step %s dropout=%s ctc_weight=%s: largest dLogits deviation %.3e of the largest entry (worst so far %.3e)"
              % (kind, head_dropout, ctc_weight, dev_gap, WORST[0]))
        assert np.abs(dL - want).max() <= REL * top, (np.abs(dL - want).max(), top)
        print("risk %.9g against %.9g (relative %.3e), ctc_loss %.9g against %.9g" % (eng.last_risk, risk, abs(eng.last_risk - risk) / abs(risk),
                                                                                    eng.last_ctc_loss, ctc))
        assert abs(eng.last_risk - risk) <= 1e-5 * abs(risk)
        if ctc_weight:
            assert abs(eng.last_ctc_loss - ctc) <= 1e-5 * abs(ctc)
        else:
            assert eng.last_ctc_loss == 0.0                                # (not computed)
        assert abs(loss - (risk + ctc_weight * ctc)) <= 1e-5 * abs(risk + ctc_weight * ctc)
    finally:
        eng.close()


def test_two_engines_alike_take_the_same_step_and_the_seed_changes_the_set(device):
    spec = _spec("fusion", True)
    got = []
    for sample_seed in (None, None, 77):
        eng, (xs, labels, il, ll) = _engine(device, spec)
        try:
            eng.set_risk(dict(CFG, sample_seed=sample_seed))
            eng.train_step(xs, labels, il, ll, apply_update=False)
            first_seed = eng.last_sample_seed
            eng.train_step(xs, labels, il, ll, apply_update=False)
            eng.dev.sync()
            assert eng.last_sample_seed != first_seed                      # the step counter is in the seed
            got.append((eng.last_sample_seed, eng.dLogits.download(), eng.P.download()) + _hyp_arrays(eng))
        finally:
            eng.close()
    assert got[0][0] == got[1][0] and all(np.array_equal(a, b) for a, b in zip(got[0][1:], got[1][1:]))
    assert got[2][0] != got[0][0] and np.array_equal(got[2][2], got[0][2])          # the same posteriors ...
    assert not all(np.array_equal(a, b) for a, b in zip(got[0][3:], got[2][3:]))    # ... another set


def test_buffers_refusals_and_large_top_paths(device):
    eng, (xs, labels, il, ll) = _engine(device, _spec("fusion", False))
    try:
        eng.set_risk(CFG)
        held = eng._risk
        assert not {"ws_beam", "ext", "score", "lctc"} & set(held) and {"count", "n_unique"} <= set(held)
        with pytest.raises(ValueError):
            eng.set_risk(dict(CFG, source="nbest"))
        with pytest.raises(ValueError):
            eng.set_risk(dict(CFG, top_paths=33))
        assert eng._risk is held and held["out"].ptr                       # a refused cfg leaves the mode, and its buffers, as they were
        eng.set_risk(dict(CFG, top_paths=20, beam_width=8))                # more draws than a beam of that width would hold
        assert eng._risk["cfg"]["top_paths"] == 20 and eng._risk["out"].shape == (B, 20, T - 2)
        loss = eng.train_step(xs, labels, il, ll, apply_update=False)
        assert np.isfinite(loss) and eng._risk["count"].download().sum(axis=1).tolist() == [20] * B
        eng.set_risk(dict(CFG, source="beam", top_paths=4, beam_width=8))  # the beam-sourced mode allocates what it did
        assert {"ws_beam", "ext", "score", "lctc"} <= set(eng._risk) and "count" not in eng._risk
        with pytest.raises(ValueError):
            eng.set_risk(dict(top_paths=9, beam_width=8))                  # ... and validates as it did
        eng.set_risk(None)
        assert eng._risk is None
    finally:
        eng.close()


def test_the_mode_off_is_the_step_it_was(device):
    spec = _spec("fusion", True)
    out = []
    for with_cfg in (True, False):
        eng, (xs, labels, il, ll) = _engine(device, spec)
        try:
            if with_cfg:
                eng.set_risk(CFG)
            eng.train_step(xs, labels, il, ll, apply_update=False)
            eng.set_risk(None)
            loss = eng.train_step(xs, labels, il, ll)
            assert eng.last_risk is None
            eng.dev.sync()
            out.append((loss, eng.dLogits.download(), eng.get_weights()))
        finally:
            eng.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
    for k, v in out[0][2].items():
        assert np.array_equal(v, out[1][2][k]), k


def test_through_the_facade(device):
    from mgr_amd import keras_like as K
    from mgr_amd.synthetic import synthetic_arrays
    spec = _spec("fusion", True)
    m = K.Model(spec, device=device, seed=3)
    m.compile(loss={"ctc": lambda a, b: b}, optimizer=K.Adam(lr=1e-3, clipvalue=0.5), risk=dict(CFG, sample_seed=11))
    xs, labels, il, ll = synthetic_arrays(spec, B, T, LMAX, 9, lmin=2, lmax=5)
    loss = m.train_on_batch(dict(xs, the_labels=labels, input_length=il, label_length=ll))
    assert set(m.last_logs) == {"loss", "risk", "ctc_loss"} and m.last_logs["loss"] == loss and np.isfinite(loss)
    assert m._engine._risk["cfg"]["source"] == "sample" and m._engine.last_sample_seed is not None
    assert abs(loss - (m.last_logs["risk"] + CFG["ctc_weight"] * m.last_logs["ctc_loss"])) <= 1e-5 * abs(loss)
    with pytest.raises(ValueError):
        m.set_risk(dict(CFG, source="nbest"))
