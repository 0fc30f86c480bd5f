"""The fp64 restatement of the expected-risk contract (tests/risk_ref.py) against its own definition - central finite differences of
Rbar w.r.t. the logits, logp by exhaustive path enumeration - and the case generator's promise (tests/risk_cases.py).  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rescore_cases as rc  # noqa: E402
import rescore_ref as rr  # noqa: E402
import risk_cases as kc  # noqa: E402
import risk_ref as kr  # noqa: E402

SMALL = [  # (T, C, skip, hypotheses of one sample (None: absent), risks, input_len, post_scale, risk_scale)
    (6, 4, 2, [[0], [1, 1], [], [2, 0]], [3, 0, 2, 1], None, 1.0, 1.0),
    (5, 3, 0, [[0, 1], [1], None, [0, 0, 0]], [0, 2, 9, 5], None, 0.5, 0.5),      # [0, 0, 0] fits exactly (5 frames); an absent slot
    (6, 4, 1, [[2], [0, 1, 2], [1, 1, 1, 1]], [1, 4, 0], [4], 2.0, 1.0),           # [1, 1, 1, 1] needs 7 frames: infeasible
    (4, 4, 0, [[2, -3], [1]], [2, 1], None, 1.0, 3.0),                             # a label clipped into the class range
]


def _rbar(z, hyp, hl, risks, skip, il, ps, rs, logp_fn=None):
    return kr.expected_risk(kr.softmax(z), hyp, hl, risks, skip=skip, input_len=il, post_scale=ps, risk_scale=rs, grad=False,
                            logp_fn=logp_fn)["risk"][0]


@pytest.mark.parametrize("case", range(len(SMALL)))
def test_gradient_is_the_finite_difference_of_the_expected_risk(case):
    T, Cn, skip, hyps, risks, il, ps, rs = SMALL[case]
    rng = np.random.default_rng(case)
    z = rng.standard_normal((1, T, Cn))
    hyp, hl = rc.pack([hyps], len(hyps), max(len(h) for h in hyps if h is not None))
    risks = np.asarray([risks])
    ref = kr.expected_risk(kr.softmax(z), hyp, hl, risks, skip=skip, input_len=il, post_scale=ps, risk_scale=rs)
    assert ref["live"].sum() >= 2 and np.abs(ref["dlogits"]).max() > 1e-3          # (a case that shows something)
    h = 1e-6
    fd = np.zeros_like(z)
    for t in range(T):
        for c in range(Cn):
            zp, zm = z.copy(), z.copy()
            zp[0, t, c] += h
            zm[0, t, c] -= h
            fd[0, t, c] = (_rbar(zp, hyp, hl, risks, skip, il, ps, rs) - _rbar(zm, hyp, hl, risks, skip, il, ps, rs)) / (2 * h)
    # central differences of a smooth fp64 function at h = 1e-6: truncation ~h^2, rounding ~1e-16 / h
    assert np.abs(fd - ref["dlogits"]).max() <= 1e-7 * max(1.0, np.abs(ref["dlogits"]).max())
    Tp = T - skip if il is None else il[0]
    assert np.all(ref["dlogits"][0, :skip] == 0) and np.all(ref["dlogits"][0, skip + Tp:] == 0)
    assert abs(ref["g"].sum()) <= 1e-12                                            # sum_k g_k = 0: the k-independent terms cancel


@pytest.mark.parametrize("case", range(len(SMALL)))
def test_expected_risk_with_logp_by_path_enumeration(case):
    T, Cn, skip, hyps, risks, il, ps, rs = SMALL[case]
    z = np.random.default_rng(10 + case).standard_normal((1, T, Cn))
    hyp, hl = rc.pack([hyps], len(hyps), max(len(h) for h in hyps if h is not None))
    a = _rbar(z, hyp, hl, np.asarray([risks]), skip, il, ps, rs)
    b = _rbar(z, hyp, hl, np.asarray([risks]), skip, il, ps, rs, logp_fn=rr.enumerate_logp)
    assert abs(a - b) <= 1e-12 * max(1.0, abs(b))


def test_slot_kinds_and_degenerate_samples():
    P = np.random.default_rng(3).dirichlet(np.full(4, 0.5), size=(1, 8)).astype(np.float32)
    hyp, hl = rc.pack([[[0], None, [1, 1, 1, 1, 1]]], 3, 5)                        # one live slot: absent, infeasible (9 frames)
    r = kr.expected_risk(P, hyp, hl, np.asarray([[2, 0, 1]]))
    assert r["live"].tolist() == [[True, False, False]] and r["risk"][0] == 2.0 and np.all(r["dlogits"] == 0) and np.all(r["g"] == 0)
    assert r["weight"].tolist() == [[1.0, 0.0, 0.0]]
    hyp, hl = rc.pack([[None, None]], 2, 1)                                        # no live slot
    r = kr.expected_risk(P, hyp, hl, np.asarray([[2, 5]]))
    assert r["risk"][0] == 0.0 and np.all(r["weight"] == 0) and np.all(r["dlogits"] == 0)
    hyp, hl = rc.pack([[[0], [1], [2, 0]]], 3, 2)                                  # equal risks everywhere
    r = kr.expected_risk(P, hyp, hl, np.asarray([[4, 4, 4]]))
    assert abs(r["risk"][0] - 4.0) < 1e-12 and np.abs(r["dlogits"]).max() < 1e-12
    r = kr.expected_risk(P, hyp, hl, np.asarray([[1, 2, 3]]), Lcap=1)              # longer than Lcap: not scored
    assert np.isnan(r["logp"][0, 2]) and r["live"].tolist() == [[True, True, False]]
    lex = [[0, 1], [2]]
    hyp, hl = rc.pack([[[0, 1], [1, 2], [1]]], 3, 2)                               # a phrase id outside the lexicon
    r = kr.expected_risk(P, hyp, hl, np.asarray([[1, 2, 3]]), lexicon=lex)
    assert np.isnan(r["logp"][0, 1]) and r["live"].tolist() == [[True, False, True]]
    words, wl = rc.pack([[[0, 1, 2], [2]]], 2, 3)
    e = kr.expected_risk(P, words, wl, np.asarray([[1, 3]]))
    assert np.array_equal(e["dlogits"], r["dlogits"]) and e["risk"][0] == r["risk"][0]


def test_every_random_case_has_a_gradient_to_show():
    for case in kc.random_cases():
        ref = kr.expected_risk(case["P"], case["hyp"], case["hl"], case["risks"], skip=case["skip"], eps=kc.EPS, input_len=case["il"],
                               post_scale=case["post_scale"], risk_scale=case["risk_scale"])
        assert kc.informative(case, ref["logp"]) >= 0.9, case["name"]
        assert np.abs(ref["dlogits"]).max() > 1e-4, case["name"]


def test_every_decode_module_exposes_expected_risk(monkeypatch):
    """Beside decode_score: the module's class map decides what is dropped from both sides ("sil"), HResults' costs by default."""
    from mgr_amd import decoding
    from mgr_amd.audio_network import sequence_decoding as audio
    from mgr_amd.early_fusion import sequence_decoding as early
    from mgr_amd.multimodal_fusion import sequence_decoding as fusion
    from mgr_amd.rgb_network import decode_rgb as rgb
    seen = []
    monkeypatch.setattr(decoding, "expected_risk", lambda *a, **kw: seen.append((a, kw)) or "out")
    for mod, sil in ((audio, 43), (early, 21), (fusion, 21), (rgb, 21)):
        assert mod.expected_risk("P", "paths", "refs", post_scale=0.5) == "out"
        a, kw = seen[-1]
        assert a == ("P", "paths") and kw["refs"] == "refs" and kw["costs"] == decoding.HTK_COSTS and kw["post_scale"] == 0.5
        assert list(kw["ignore"]) == [sil]
