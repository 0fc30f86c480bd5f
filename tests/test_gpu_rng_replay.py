"""-m gpu: training steps under the DEVICE RNG (rand=None - the mode every real run, fit_generator and bench.py train in) against
the fp64 oracle.  tests/rng_replay.py rebuilds on the CPU the masks and the noise such a step consumes from (engine seed, step
counter); the oracle is given them as its `rand`.  A mask drawn at another counter or slot in one part of the step than in
another, the kept-feature lists of another mask, one mask for both directions, noise added twice or a head seed that differs
between forward and backward all move the result by far more than the tolerances here (tests/test_cpu_rng_replay.py shows
it on the oracle alone).  The cases are tests/rng_cases.py's; the RGB network draws nothing (same CPU file) and has no case.

Tolerances: 1e-4 for loss, loss_b and P, 2e-4 for gradients (test_gpu_network.py::test_loss_grads_match_golden's); 1e-4 for
losses and final weights of a trajectory (::test_training_trajectory_matches_golden's); the movement through
update_cases.assert_movement (4 x the CPU-measured float64-vs-float32 figure of each case); the noise kernel's bound of
tests/test_gpu_update_kernels.py; 5 binomial standard deviations where masks are counted."""
import math

import numpy as np
import pytest

from oracle import network_ref as nr
from tests import rng_cases as rc
from tests import rng_replay as rr
from tests import update_cases as uc
from tests import update_ref as ur
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _engine(device, c, seed=None):
    from mgr_amd.engine import Engine
    from mgr_amd.spec import NetworkSpec
    eng = Engine(NetworkSpec.from_dict(c["spec"]), c["B"], c["T"], c["Lmax"], device=device, seed=c["seed"] if seed is None else seed)
    eng.set_weights(c["w0"])
    return eng


def _step(eng, c, rand=None):
    """One step without update; everything it computed."""
    eng.enqueue_train_step(c["inputs"], c["labels"], c["il"], c["ll"], rand=rand, apply_update=False)
    loss = eng.read_loss()
    return dict(loss=loss, loss_b=eng.loss_b.download(), P=eng.P.download(), g=eng.get_grads())


def _assert_step(got, ref, what):
    loss, lb, g, P = ref
    err = {k: rel_err(got["g"][k], g[k]) for k in g}
    print("%s: loss %.3e  loss_b %.3e  P %.3e  worst gradient %.3e (%s)" % (
        what, abs(got["loss"] - loss) / abs(loss), float((np.abs(got["loss_b"] - lb) / np.abs(lb)).max()), rel_err(got["P"], P),
        max(err.values()), max(err, key=err.get)))
    assert abs(got["loss"] - loss) <= 1e-4 * abs(loss), (what, got["loss"], loss)
    assert np.allclose(got["loss_b"], lb, rtol=1e-4), what
    assert rel_err(got["P"], P) < 1e-4, what
    assert set(got["g"]) == set(g)
    bad = {k: e for k, e in err.items() if not e < 2e-4}
    assert not bad, (what, bad)


def _assert_covers(c):
    """The sites a case claims to cover are drawn from: noise, every encoder layer, the fusion layer if there is one, the head."""
    sp = c["spec"]
    assert sp["head"]["dropout"] > 0 and any(s["noise"] > 0 for s in sp["streams"])
    assert all(lay["dropout"] > 0 for s in sp["streams"] for lay in s["layers"])
    assert not sp["fusion"] or sp["fusion"]["dropout"] > 0


class _Calls:
    """Records the library calls an engine makes through its Device (name, arguments) while it is installed."""

    def __init__(self, monkeypatch, device):
        self.seen = []
        call = device.call

        def recording(name, *args):
            self.seen.append((name, args))
            return call(name, *args)
        monkeypatch.setattr(device, "call", recording)

    def count(self, name):
        return sum(1 for n, _ in self.seen if n == name)

    def args(self, name):
        return [a for n, a in self.seen if n == name]


# --------------------------------------------------------------------------------------------------------------- a. one step
@pytest.mark.parametrize("name", rc.NAMES)
def test_first_step_matches_fp64_under_the_replayed_randomness(device, monkeypatch, name):
    """A fresh engine's first device-RNG step against the oracle under replay(seed, 0).  The split cases also show which products
    ran: 128 masked inputs - the transposed split-row projection, whose kept-feature lists the weight-gradient product is handed
    (the lists of the very mask the backward pass reads); 64 - the row-major dropout-aware calls."""
    c = rc.case(name)
    _assert_covers(c)
    if name == "fusion_tiny":
        assert c["spec"]["fusion"] and not any(s["trainable"] for s in c["spec"]["streams"])
    else:
        assert all(s["trainable"] and len(s["layers"]) == 2 for s in c["spec"]["streams"])
    eng = _engine(device, c)
    calls = _Calls(monkeypatch, device)
    try:
        got = _step(eng, c)
        monkeypatch.undo()
        _assert_step(got, rc.oracle_step(name, 0), name)
        assert eng.rng_step == 1
        if name.startswith("split"):
            sname = c["spec"]["streams"][0]["name"]
            L1 = [eng.dirs["%s/l1/%s" % (sname, d)] for d in ("fwd", "bwd")]
            fin = L1[0].fin
            assert all(L.p >= 0.3 and L.mask is not None and L.ws_sp is not None for L in L1)
            if name == "split_wide":
                assert 128 <= fin <= 2048 and eng._xt_split.get(eng.Y1T[sname].ptr)
                assert calls.count("mgr_lstm_input_proj_dropout_ts") == 2 and calls.count("mgr_lstm_input_proj_dropout") == 2
                pg = calls.args("mgr_lstm_param_grads_dropout_ts")
                assert len(pg) == 2 and calls.count("mgr_lstm_param_grads_dropout") == 2
                for L, a in zip(L1, pg):
                    assert a[2] == L.mask.ptr and a[-2] is L.ws_sp, "the dW product was not handed the projection's kept lists"
                    assert L.lists_mask == 0
            else:
                assert fin < 128 and sname not in eng.Y1T
                assert calls.count("mgr_lstm_input_proj_dropout") == 4 and calls.count("mgr_lstm_param_grads_dropout") == 4
                assert not any(n.endswith(("_ts", "_t")) for n, _ in calls.seen)
    finally:
        monkeypatch.undo()
        eng.close()


# ------------------------------------------------------------------------------------- b. the same bits as the explicit path
@pytest.mark.parametrize("name", rc.NAMES)
def test_device_rng_step_is_bit_identical_to_the_step_given_the_replay(device, name):
    """Without GaussianNoise (the one thing the two modes compute differently: the explicit mode adds host noise in the staging
    buffer) a device-RNG step and a step given rand=replay(...) run the same kernels on the same numbers: mgr_dropout_mask fills
    the buffer the upload fills, and the Dense kernels' drop_factor returns the same float from a mask as from a seed.  Two
    steps each, so that the second replay is told from the first.  unimodal_tiny's seed is above 2^62: the seed product wraps."""
    c = rc.without_noise(rc.case(name))
    assert all(s["noise"] == 0 for s in c["spec"]["streams"]) and not any(k.endswith("/noise") for k in c["rands"][0])
    assert name != "unimodal_tiny" or c["seed"] * rr.SEED_MUL >= 2 ** 64
    dev_eng, exp_eng = _engine(device, c), _engine(device, c)
    try:
        for step in range(2):
            a, b = _step(dev_eng, c), _step(exp_eng, c, rand=c["rands"][step])
            assert a["loss"] == b["loss"], (step, a["loss"], b["loss"])
            assert np.array_equal(bits(a["loss_b"]), bits(b["loss_b"])) and np.array_equal(bits(a["P"]), bits(b["P"])), step
            for k in a["g"]:
                assert np.array_equal(bits(a["g"][k]), bits(b["g"][k])), (step, k)
        assert dev_eng.rng_step == 2 and exp_eng.rng_step == 2
    finally:
        dev_eng.close()
        exp_eng.close()


@pytest.mark.parametrize("name", rc.NAMES)
def test_noise_goes_into_the_copy_once_and_the_resident_input_stays(device, name):
    """The engine's noised copy of the input after a step is the resident input plus noise_ref at slot 900 + stream index, within
    the noise kernel's bound (tests/test_gpu_update_kernels.py::test_noise_elementwise: 1e-5 stddev + 2^-23 |Y|); the resident
    buffer holds the float32 input, bit for bit, after two steps."""
    c = rc.case(name)
    eng = _engine(device, c)
    try:
        for step in range(2):
            _step(eng, c)
            for i, s in enumerate(c["spec"]["streams"]):
                x32 = np.asarray(c["inputs"][s["name"]], np.float32)
                assert np.array_equal(bits(eng.Xin[s["name"]].download()), bits(x32)), (step, s["name"])
                if s["noise"] > 0:
                    Y = eng.X[s["name"]].download().reshape(-1)
                    ref = ur.noise_ref(x32, x32.size, s["noise"], rr.site_seed(c["seed"], step, rr.NOISE_SLOT + i))
                    err = np.abs(Y.astype(np.float64) - ref)
                    bound = 1e-5 * s["noise"] + 2.0 ** -23 * np.abs(Y)
                    assert np.all(err <= bound), (step, s["name"], float((err / bound).max()))
                else:
                    assert s["name"] not in eng.X
        assert any(s["noise"] > 0 for s in c["spec"]["streams"])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------- c. the step counter
def _assert_trajectory(name, n, losses, start, end):
    c = rc.case(name)
    r0, rf, rlosses = rc.oracle_trajectory(name, n)
    print("%s losses %s oracle %s" % (name, losses, rlosses))
    assert np.allclose(losses, rlosses, rtol=1e-4), (losses, rlosses)
    for k in rf:
        assert rel_err(end[k], rf[k]) < 1e-4, k
    for wname, _, tr, _ in nr.weight_names(c["spec"]):
        if not tr:
            assert np.array_equal(end[wname], start[wname]), wname
    uc.assert_movement(rc.move_name(name, n), c["spec"], end, start, rf, r0)


@pytest.mark.parametrize("name", rc.NAMES)
def test_three_updating_steps_match_the_fp64_trainer_over_replays_0_1_2(device, name):
    c = rc.case(name)
    _assert_covers(c)
    eng = _engine(device, c)
    try:
        start = eng.get_weights()
        losses = [eng.train_step(c["inputs"], c["labels"], c["il"], c["ll"]) for _ in range(3)]
        assert eng.rng_step == 3 and eng.iterations == 3 and eng.updates_skipped == 0
        _assert_trajectory(name, 3, losses, start, eng.get_weights())
    finally:
        eng.close()


# --------------------------------------------------------------------------------------------------------- d. calls in between
@pytest.mark.parametrize("name", rc.NAMES)
def test_predict_draws_nothing_and_a_training_phase_loss_takes_one_step_of_randomness(device, name):
    """step; predict; loss_on_batch(train_phase=True); step - without updates, so that every pass is the oracle's at the start
    weights: replay 0, no randomness, replay 1 (forward only), replay 2."""
    c = rc.case(name)
    _assert_covers(c)
    eng = _engine(device, c)
    try:
        _assert_step(_step(eng, c), rc.oracle_step(name, 0), name + " step 0")
        P = eng.predict(c["inputs"])
        assert eng.rng_step == 1
        assert rel_err(P, rc.oracle_step(name, 0, train=False)[3]) < 1e-4
        lb = eng.loss_on_batch(c["inputs"], c["labels"], c["il"], c["ll"], train_phase=True)
        ref_lb = rc.oracle_step(name, 1)[1]
        print("%s loss_on_batch %.3e" % (name, float((np.abs(lb - ref_lb) / np.abs(ref_lb)).max())))
        assert np.allclose(lb, ref_lb, rtol=1e-4), (lb, ref_lb)
        assert rel_err(eng.P.download(), rc.oracle_step(name, 1)[3]) < 1e-4
        _assert_step(_step(eng, c), rc.oracle_step(name, 2), name + " step 2")
        assert eng.rng_step == 3
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------- e. the pipelined schedule
@pytest.mark.parametrize("two_ahead", [False, True], ids=["next", "next_and_after_next"])
def test_pipelined_steps_match_the_fp64_trainer_over_replays_0_to_3(device, two_ahead):
    """The frozen-encoder fusion network on resident inputs, each step's encoder pass enqueued by the call before it (and, two
    ahead, its first part by the call before that): the pass of step n draws at counter n whichever call enqueues it."""
    name = "fusion_tiny"
    c = rc.case(name)
    _assert_covers(c)
    eng = _engine(device, c)
    try:
        assert eng.can_pipeline and eng.schedule.pipeline
        start = eng.get_weights()
        eng._upload_inputs(c["inputs"], None, True)
        eng._upload_labels(c["labels"], c["il"], c["ll"])
        losses = []
        for i in range(4):
            eng.enqueue_train_step(None, None, None, None, upload=False, prefetch_next=i < 3, prefetch_after_next=two_ahead and i < 2)
            losses.append(eng.read_loss())
        device.sync()
        assert eng.rng_step == 4 and eng.iterations == 4
        _assert_trajectory(name, 4, losses, start, eng.get_weights())
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ f. seeds
def test_same_seed_same_bits_and_the_next_seed_an_independent_mask(device):
    name = "fusion_tiny"
    c = rc.case(name)
    p = c["spec"]["fusion"]["dropout"]
    assert p > 0
    out, masks = [], []
    for seed in (c["seed"], c["seed"], c["seed"] + 1):
        eng = _engine(device, c, seed=seed)
        try:
            out.append(_step(eng, c))
            masks.append({d: eng.dirs["fusion/" + d].mask.download() for d in ("fwd", "bwd")})
        finally:
            eng.close()
    a, b, other = out
    assert a["loss"] == b["loss"] and np.array_equal(bits(a["loss_b"]), bits(b["loss_b"])) and np.array_equal(bits(a["P"]), bits(b["P"]))
    for k in a["g"]:
        assert np.array_equal(bits(a["g"][k]), bits(b["g"][k])), k
    assert other["loss"] != a["loss"]
    q = 2 * p * (1 - p)
    for d in ("fwd", "bwd"):
        # what the engine drew IS the replay (so a failure of the oracle comparison above can be told from a wrong mask) ...
        assert np.array_equal(bits(masks[0][d]), bits(c["rands"][0]["fusion/%s/mask" % d])), d
        assert np.array_equal(bits(masks[0][d]), bits(masks[1][d]))
        # ... and the next seed's mask differs from it where exactly one of two independent masks keeps
        n = masks[0][d].size
        frac = float((masks[0][d] != masks[2][d]).mean())
        assert abs(frac - q) <= 5 * math.sqrt(q * (1 - q) / n), (d, frac, q, n)
    fb = float((masks[0]["fwd"] != masks[0]["bwd"]).mean())
    assert abs(fb - q) <= 5 * math.sqrt(q * (1 - q) / masks[0]["fwd"].size), fb
