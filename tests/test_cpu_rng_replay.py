"""tests/rng_replay.py on its own, and what the GPU comparison of tests/test_gpu_rng_replay.py can see: keys and shapes against
oracle.network_ref.draw_rand, the masks' kept fractions, that no two sites of a run share a seed, that neighbouring masks are
independent - and, on the fp64 oracle alone, that a replay off by one step, with a layer's two masks swapped or without the
head mask moves the loss and every gradient by at least ten times the tolerance the GPU file compares at."""
import math

import numpy as np
import pytest

from oracle import network_ref as nr
from tests import rng_cases as rc
from tests import rng_replay as rr
from tests import update_cases as uc
from tests import update_ref as ur
from tests.helpers import rel_err

# what tests/test_gpu_rng_replay.py compares at (tests/test_gpu_network.py::test_loss_grads_match_golden's figures)
TOL_LOSS, TOL_GRAD = 1e-4, 2e-4


def _five_sigma(frac, q, n):
    return abs(frac - q) <= 5 * math.sqrt(q * (1 - q) / n)


def _masks(c, step=0):
    return {k: v for k, v in c["rands"][step].items() if k.endswith("/mask")}


@pytest.mark.parametrize("name", rc.NAMES)
def test_keys_and_shapes_are_draw_rands(name):
    c = rc.case(name)
    ref = nr.draw_rand(c["spec"], c["B"], c["T"], np.random.default_rng(0))
    for r in c["rands"]:
        assert set(r) == set(ref)
        for k in ref:
            assert r[k].shape == ref[k].shape and r[k].dtype == ref[k].dtype, k
    assert nr.draw_rand(c["spec"], c["B"], c["T"], np.random.default_rng(0), train=False) == {}


def test_the_cases_cover_what_they_claim():
    f, u, w, n = (rc.covered(rc.case(k)) for k in rc.NAMES)
    assert {"audio/noise", "fusion/fwd/mask", "fusion/bwd/mask", "head/mask", "audio/l1/bwd/mask", "skeletal/l0/fwd/mask"} <= f
    assert "skeletal/noise" not in f           # (stream 1 has no noise and keeps slot 901 all the same)
    assert not any(s["trainable"] for s in rc.case("fusion_tiny")["spec"]["streams"])
    for cov in (u, w, n):
        assert {"the_input/noise", "the_input/l0/fwd/mask", "the_input/l1/bwd/mask", "head/mask"} <= cov
    for k, lo, hi in (("split_wide", 128, 2048), ("split_narrow", 1, 127)):
        s = rc.case(k)["spec"]["streams"][0]
        assert s["trainable"] and lo <= 2 * s["layers"][0]["H"] <= hi and s["layers"][1]["dropout"] >= 0.3
    assert rc.SEEDS["unimodal_tiny"] > 2 ** 62 and rc.SEEDS["unimodal_tiny"] * rr.SEED_MUL >= 2 ** 64


def test_the_rgb_network_draws_nothing():
    """Every rate of the RGB network is 0 and it has no noise (a CNN front-end takes none): a device-RNG step of it consumes no
    randomness, and tests/test_gpu_rgb.py's rand={} steps already are its device-RNG steps.  Should a rate appear, this fails and
    the GPU file needs an RGB case."""
    from mgr_amd import configs
    sd = configs.rgb_spec(h=64).to_dict()
    assert rr.replay(sd, 2, 8, 3, 0) == {} and nr.draw_rand(sd, 2, 8, np.random.default_rng(0)) == {}


def test_slot_order():
    """The order written down in tests/rng_replay.py, on a spec whose streams differ in depth and whose first layer has p = 0."""
    spec = {"streams": [{"name": "a", "F": 3, "noise": 0.0, "layers": [{"H": 2, "dropout": 0.0}, {"H": 2, "dropout": 0.5}]},
                        {"name": "b", "F": 4, "noise": 0.3, "layers": [{"H": 5, "dropout": 0.5}]}],
            "fusion": {"H": 3, "dropout": 0.2}, "head": {"dropout": 0.1, "C": 4}}
    got = {k: (slot, shape) for k, slot, shape, _, _ in rr.sites(spec, 2, 6)}
    assert got == {"a/noise": (900, (2, 6, 3)), "b/noise": (901, (2, 6, 4)),
                   "a/l0/fwd/mask": (1, (4, 2, 3)), "a/l0/bwd/mask": (2, (4, 2, 3)),
                   "b/l0/fwd/mask": (3, (4, 2, 4)), "b/l0/bwd/mask": (4, (4, 2, 4)),
                   "a/l1/fwd/mask": (5, (4, 2, 4)), "a/l1/bwd/mask": (6, (4, 2, 4)),
                   "fusion/fwd/mask": (500, (4, 2, 14)), "fusion/bwd/mask": (501, (4, 2, 14)), "head/mask": (999, (2, 6, 6))}
    r = rr.replay(spec, 2, 6, 7, 3)
    assert set(r) == set(nr.draw_rand(spec, 2, 6, np.random.default_rng(0))) and "a/l0/fwd/mask" not in r and "a/noise" not in r
    sd = rr.site_seed(7, 3, 5)
    assert sd == 7 * 1000003 + 3 * 131 + 5
    assert np.array_equal(r["a/l1/fwd/mask"].reshape(-1), ur.drop_scale(sd, np.arange(32, dtype=np.uint64), 0.5))
    assert np.array_equal(r["b/noise"].reshape(-1), ur.noise_ref(np.zeros(48), 48, 0.3, rr.site_seed(7, 3, 901)))
    assert rr.site_seed(2 ** 63 + 9, 1, 2) == ((2 ** 63 + 9) * 1000003 + 133) % 2 ** 64 < (2 ** 63 + 9) * 1000003


@pytest.mark.parametrize("name", rc.NAMES)
def test_kept_fraction(name):
    c = rc.case(name)
    rates = {k: p for k, _, _, p, kind in rr.sites(c["spec"], c["B"], c["T"]) if kind == "mask"}
    for r in c["rands"]:
        for k, m in ((k, v) for k, v in r.items() if k.endswith("/mask")):
            p = rates[k]
            assert p > 0 and set(np.unique(m)) <= {0.0, float(ur.inv_keep(p))}, k
            assert _five_sigma((m != 0).mean(), 1.0 - p, m.size), (k, (m != 0).mean(), p, m.size)


@pytest.mark.parametrize("name", rc.NAMES)
def test_no_two_sites_share_a_seed_in_10000_steps(name):
    c = rc.case(name)
    slots = [slot for _, slot, _, _, _ in rr.sites(c["spec"], c["B"], c["T"])]
    assert len(set(slots)) == len(slots)
    seeds = {rr.site_seed(c["seed"], step, slot) for step in range(10000) for slot in slots}
    assert len(seeds) == 10000 * len(slots)


@pytest.mark.parametrize("name", rc.NAMES)
def test_masks_of_a_layer_and_of_consecutive_steps_differ(name):
    """Two independent masks of rate p differ where exactly one of them keeps: a fraction 2 p (1 - p) of the positions."""
    c = rc.case(name)
    rates = {k: p for k, _, _, p, _ in rr.sites(c["spec"], c["B"], c["T"])}
    m0, m1 = _masks(c, 0), _masks(c, 1)
    pairs = [(k, m0[k], m0[k.replace("/fwd/", "/bwd/")]) for k in m0 if "/fwd/" in k] + [(k, m0[k], m1[k]) for k in m0]
    assert len(pairs) == len(m0) + (len(m0) - 1) // 2
    for k, a, b in pairs:
        q = 2 * rates[k] * (1 - rates[k])
        assert _five_sigma((a != b).mean(), q, a.size), (k, (a != b).mean(), q, a.size)


def _swapped(r):
    out = dict(r)
    for k in r:
        if "/fwd/" in k:
            out[k], out[k.replace("/fwd/", "/bwd/")] = r[k.replace("/fwd/", "/bwd/")], r[k]
    return out


@pytest.mark.parametrize("name", rc.NAMES)
@pytest.mark.parametrize("step", [0, 1, 2])
def test_the_oracle_tells_a_wrong_replay_from_the_right_one(name, step):
    """Negative control, oracle only: at every step the GPU file compares at, the replay of the NEXT step, the right step's
    replay with each layer's fwd and bwd masks swapped, and the right replay without the head mask each move the loss, a per-
    sample loss, the posteriors and every gradient by at least 10 x the tolerance of the GPU comparison.  A condition on the
    chosen batches and seeds (tests/rng_cases.py), which is why it is asserted: without it the GPU test would pass with such a
    mistake in the engine."""
    c = rc.case(name)
    loss, lb, g, P = rc.oracle_step(name, step)
    right = c["rands"][step]
    wrong = {"next step": c["rands"][step + 1], "swapped": _swapped(right), "no head mask": {k: v for k, v in right.items() if k != "head/mask"}}
    assert "head/mask" in right and any("/fwd/" in k for k in right)
    for what, r in wrong.items():
        loss2, lb2, g2, P2 = nr.loss_and_grads(c["spec"], c["w0"], c["inputs"], c["labels"], c["il"], c["ll"], r)
        assert abs(loss2 - loss) >= 10 * TOL_LOSS * abs(loss), (what, loss, loss2)
        assert (np.abs(lb2 - lb) / np.abs(lb)).max() >= 10 * TOL_LOSS, what
        assert rel_err(P2, P) >= 10 * TOL_LOSS, what
        assert set(g2) == set(g)
        for k in g:
            assert rel_err(g2[k], g[k]) >= 10 * TOL_GRAD, (what, k, rel_err(g2[k], g[k]))


MOVE_CASES = [(name, 3) for name in rc.NAMES] + [("fusion_tiny", 4)]


@pytest.mark.parametrize("name,n", MOVE_CASES)
def test_movement_error_model(name, n):
    """The float64-vs-float32 movement figures of these cases in tests/update_cases.py, re-measured the way
    tests/test_cpu_update_ref.py::test_movement_error_model measures the others; an update scaled by 0.8 fails."""
    c = rc.steps(rc.case(name), n)
    w0, wf, _ = rc.oracle_trajectory(name, n)
    s0, sf, _, _ = uc.run_trainer(c, np.float32)
    case_name = rc.move_name(name, n)
    worst = uc.assert_movement(case_name, c["spec"], sf, s0, wf, w0)
    assert set(worst) == set(uc.MOVE_MEASURED[case_name])
    for kind in worst:                                # far below the 0.2 of an update wrong by 20 %
        assert uc.move_tol(case_name, kind) < 0.2 / 20, kind
    bad = {k: w0[k] + 0.8 * (wf[k] - w0[k]) for k in wf}
    with pytest.raises(AssertionError):
        uc.assert_movement(case_name, c["spec"], bad, w0, wf, w0)
