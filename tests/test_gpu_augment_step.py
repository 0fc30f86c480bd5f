"""-m gpu: training steps with Engine.set_augment on, against the fp64 oracle fed the RESTATED augmentation (tests/augment_ref.py)
of the step's batch and the replayed randomness of the step's counter (tests/rng_replay.py; the plan's seed slot is 950).  The
cases are tests/rng_cases.py's, unchanged.  A plan drawn at another counter, applied to another batch of the pipelined schedule,
or applied by a pass that is no training step moves the results far beyond the tolerances (test_gpu_rng_replay.py's: 1e-4 on
loss / loss_b / P, 2e-4 on gradients) or breaks the bit comparisons."""
import copy

import numpy as np
import pytest

from mgr_amd import augment
from oracle import network_ref as nr
from tests import augment_ref as ar
from tests import rng_cases as rc
from tests import rng_replay as rr
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

PLAN_SLOT = 950
CFGS = {
    "fusion_tiny": dict(segments=2, max_shift=1, time_masks=1, time_width=3, feature_masks=1, feature_width=2, stream_drop=0.5,
                        streams={"skeletal": dict(feature_width=1, fill=0.25)}),
    "split_wide": dict(segments=3, max_shift=2, time_masks=2, time_width=5, feature_masks=1, feature_width=3),
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_engine(device, c, seed, schedule=None):
    from mgr_amd.engine import Engine
    from mgr_amd.spec import NetworkSpec
    eng = Engine(NetworkSpec.from_dict(c["spec"]), c["B"], c["T"], c["Lmax"], device=device, seed=seed, schedule=schedule)
    eng.set_weights(c["w0"])
    return eng


def _norm(c, name):
    return augment.normalize_config(CFGS[name], c["spec"], c["T"])


def restated(c, name, inputs, seed, step):
    """(augmented float32 inputs, plan) of the training-step pass engine `seed` runs at counter `step`."""
    x32 = {k: np.asarray(v, np.float32) for k, v in inputs.items()}
    return ar.augment_ref(x32, _norm(c, name), rr.site_seed(seed, step, PLAN_SLOT))


def seed_with_a_dropped_and_an_undropped_sample(c, name):
    K = CFGS[name]["segments"]
    for seed in range(rc.SEEDS[name], rc.SEEDS[name] + 64):
        drop = restated(c, name, c["inputs"], seed, 0)[1][:, K + 1]
        if (drop >= 0).any() and (drop < 0).any():
            return seed
    raise AssertionError("no seed found")


def batches_of(c, n):
    """n distinct batches of the case's shapes (the first is the case's own)."""
    out = [(c["inputs"], c["labels"], c["il"], c["ll"])]
    rng = np.random.default_rng(2014)
    for _ in range(n - 1):
        out.append(nr.synthetic_batch(c["spec"], c["B"], c["T"], c["Lmax"], rng, lmin=1, lmax=4))
    return out


def oracle(c, name, batch, seed, step):
    inputs, labels, il, ll = batch
    xa, plan = restated(c, name, inputs, seed, step)
    rand = rr.replay(c["spec"], c["B"], c["T"], seed, step)
    return nr.loss_and_grads(c["spec"], c["w0"], {k: v.astype(np.float64) for k, v in xa.items()}, labels, il, ll, rand), xa, plan


def run_step(eng, batch, **kw):
    inputs, labels, il, ll = batch
    loss = eng.train_step(inputs, labels, il, ll, apply_update=False, **kw)
    return dict(loss=loss, loss_b=eng.loss_b.download(), P=eng.P.download(), g=eng.get_grads())


def assert_step(got, ref, what):
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


class _Calls:
    """Records the library calls an engine makes through its Device (name, arguments) while it is installed."""

    def __init__(self, monkeypatch, device):
        self.seen = []
        call = device.call

        def recording(name, *args):
            self.seen.append((name, args))
            return call(name, *args)
        monkeypatch.setattr(device, "call", recording)

    def names(self):
        return [n for n, _ in self.seen]

    def args(self, name):
        return [a for n, a in self.seen if n == name]


# ---------------------------------------------------------------------------------------------------------------- a. one step
@pytest.mark.parametrize("name", list(CFGS))
def test_first_step_matches_fp64_under_the_restated_augmentation(device, monkeypatch, name):
    c = rc.case(name)
    seed = seed_with_a_dropped_and_an_undropped_sample(c, name) if name == "fusion_tiny" else rc.SEEDS[name]
    batch = (c["inputs"], c["labels"], c["il"], c["ll"])
    ref, xa, plan = oracle(c, name, batch, seed, 0)
    K = CFGS[name]["segments"]
    assert np.any(plan[:, 1:K] != ar.sources(c["T"], K)[1:K]), "the warp of this seed is the identity"
    if name == "fusion_tiny":
        assert (plan[:, K + 1] >= 0).any() and (plan[:, K + 1] < 0).any()
    assert any(not np.array_equal(bits(xa[k]), bits(np.asarray(c["inputs"][k], np.float32))) for k in xa)
    plain = nr.loss_and_grads(c["spec"], c["w0"], c["inputs"], c["labels"], c["il"], c["ll"], rr.replay(c["spec"], c["B"], c["T"], seed, 0))
    assert abs(plain[0] - ref[0]) > 1e-3 * abs(ref[0]), "the comparison could not tell an augmented step from a plain one"
    eng = make_engine(device, c, seed)
    calls = _Calls(monkeypatch, device)
    try:
        eng.set_augment(CFGS[name])
        got = run_step(eng, batch)
        monkeypatch.undo()
        assert_step(got, ref, name)
        assert eng.rng_step == 1
        S = len(c["spec"]["streams"])
        names = calls.names()
        assert names.count("mgr_augment_plan") == 1 and names.count("mgr_augment_apply") == S and "mgr_add_gaussian_noise" not in names
        # what the encoders read IS the restated batch plus the replayed noise (and the resident input is pristine)
        for i, s in enumerate(c["spec"]["streams"]):
            Y = eng.X[s["name"]].download()
            if s["noise"] > 0:
                assert not np.array_equal(bits(Y), bits(xa[s["name"]]))
            else:
                assert np.array_equal(bits(Y), bits(xa[s["name"]])), s["name"]
            assert np.array_equal(bits(eng.Xin[s["name"]].download()), bits(np.asarray(c["inputs"][s["name"]], np.float32)))
        with pytest.raises(ValueError, match="rand"):
            eng.train_step(*batch, rand=rr.replay(c["spec"], c["B"], c["T"], seed, 1), apply_update=False)
        assert eng.rng_step == 1
    finally:
        monkeypatch.undo()
        eng.close()


# --------------------------------------------------------------------------------------------------------- b. the step counter
@pytest.mark.parametrize("name", list(CFGS))
def test_three_steps_in_a_row_each_under_the_plan_of_its_counter(device, name):
    c = rc.case(name)
    seed = rc.SEEDS[name]
    batches = batches_of(c, 3)
    eng = make_engine(device, c, seed)
    try:
        eng.set_augment(CFGS[name])
        plans = []
        for k in range(3):
            ref, _, plan = oracle(c, name, batches[k], seed, k)
            plans.append(plan)
            assert_step(run_step(eng, batches[k]), ref, "%s step %d" % (name, k))
        assert eng.rng_step == 3
        assert not np.array_equal(plans[0], plans[1]) and not np.array_equal(plans[1], plans[2])
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------------------- c. the pipelined schedule
def test_pipelined_steps_equal_unpipelined_steps_bit_for_bit(device):
    name = "fusion_tiny"
    c = rc.case(name)
    seed = rc.SEEDS[name]
    batches = batches_of(c, 4)
    out = []
    for pipelined in (True, False):
        eng = make_engine(device, c, seed)
        try:
            assert eng.can_pipeline and eng.schedule.pipeline
            eng.set_augment(CFGS[name])
            losses = []
            for i, (inputs, labels, il, ll) in enumerate(batches):
                kw = {}
                if pipelined and i + 1 < 4:
                    kw["next_inputs"] = batches[i + 1][0]
                    if i + 2 < 4:
                        kw["after_next_inputs"] = batches[i + 2][0]
                losses.append(eng.train_step(inputs, labels, il, ll, **kw))
            device.sync()
            assert eng.rng_step == 4 and eng.iterations == 4
            out.append((losses, eng.get_weights()))
        finally:
            eng.close()
    (la, wa), (lb, wb) = out
    assert la == lb, (la, lb)
    for k in wa:
        assert np.array_equal(bits(wa[k]), bits(wb[k])), k
    # ... and they are the augmented steps: the first loss is the oracle's under plan 0
    ref, _, _ = oracle(c, name, batches[0], seed, 0)
    assert abs(la[0] - ref[0]) <= 1e-4 * abs(ref[0])


# ----------------------------------------------------------------------------------------------------------- d. other passes
def test_passes_that_are_no_training_step_are_untouched(device):
    name = "fusion_tiny"
    c = rc.case(name)
    seed = rc.SEEDS[name]
    on, off = make_engine(device, c, seed), make_engine(device, c, seed)
    try:
        on.set_augment(CFGS[name])
        for eng in (on, off):
            eng.train_step(c["inputs"], c["labels"], c["il"], c["ll"], apply_update=False)       # (rng_step 1 on both)
        a = on.loss_on_batch(c["inputs"], c["labels"], c["il"], c["ll"], train_phase=True)
        b = off.loss_on_batch(c["inputs"], c["labels"], c["il"], c["ll"], train_phase=True)
        assert np.array_equal(bits(a), bits(b)) and on.rng_step == off.rng_step == 2
        a, b = on.forward_train_phase(c["inputs"]), off.forward_train_phase(c["inputs"])
        assert np.array_equal(bits(a), bits(b)) and on.rng_step == off.rng_step == 3
        a, b = on.predict(c["inputs"]), off.predict(c["inputs"])
        assert np.array_equal(bits(a), bits(b)) and on.rng_step == off.rng_step == 3
    finally:
        on.close()
        off.close()


# ------------------------------------------------------------------------------------------------------------- e. mode off
def _noise_args(calls):
    return [(a[2], a[3], a[4].value) for a in calls.args("mgr_add_gaussian_noise")]


@pytest.mark.parametrize("name", list(CFGS))
def test_mode_off_makes_the_calls_of_an_engine_that_never_had_it(device, monkeypatch, name):
    c = rc.case(name)
    seed = rc.SEEDS[name]
    batch = (c["inputs"], c["labels"], c["il"], c["ll"])
    seen = []
    for cycle in (False, True):
        eng = make_engine(device, c, seed)
        try:
            before = set(eng.X)
            if cycle:
                eng.set_augment(CFGS[name])
                assert set(eng.X) == {s["name"] for s in c["spec"]["streams"]}
                eng.set_augment(None)
            assert eng._augment is None and set(eng.X) == before
            calls = _Calls(monkeypatch, device)
            got = run_step(eng, batch)
            monkeypatch.undo()
            seen.append((calls.names(), _noise_args(calls), got))
        finally:
            monkeypatch.undo()
            eng.close()
    (na, za, ga), (nb, zb, gb) = seen
    assert na == nb and za == zb
    assert not any(n.startswith("mgr_augment") for n in na) and "mgr_add_gaussian_noise" in na
    assert ga["loss"] == gb["loss"] and np.array_equal(bits(ga["P"]), bits(gb["P"]))


# --------------------------------------------------------------------------------------------------------------- f. the facade
def test_engine_refusals_leave_the_mode_as_it_was(device):
    name = "fusion_tiny"
    c = rc.case(name)
    eng = make_engine(device, c, 1)
    try:
        eng.set_augment(CFGS[name])
        kept = eng._augment
        for bad in (dict(segments=17), dict(segments=2, max_shift=3), dict(time_masks=1, time_width=c["T"] + 1), dict(nonsense=1),
                    dict(stream_drop=1.0)):
            with pytest.raises(ValueError):
                eng.set_augment(bad)
            assert eng._augment is kept
        eng.set_entropy(dict(weight=0.1))        # (combines with the other training modes: it only changes what the encoders read)
        assert np.isfinite(eng.train_step(c["inputs"], c["labels"], c["il"], c["ll"]))
        eng.set_entropy(None)
    finally:
        eng.close()
    from mgr_amd.engine import Engine
    from mgr_amd.spec import NetworkSpec
    inf = Engine(NetworkSpec.from_dict(c["spec"]), c["B"], c["T"], c["Lmax"], device=device, inference_only=True)
    try:
        with pytest.raises(ValueError, match="inference"):
            inf.set_augment(CFGS[name])
    finally:
        inf.close()


def test_facade_compile_fit_and_switch_off(device):
    from mgr_amd import keras_like as K
    from mgr_amd.spec import NetworkSpec
    from mgr_amd.synthetic import synthetic_arrays
    name = "fusion_tiny"
    c = rc.case(name)
    spec = NetworkSpec.from_dict(copy.deepcopy(c["spec"]))
    B, T, Lmax = c["B"], c["T"], c["Lmax"]
    m = K.Model(spec, device=device, seed=3)
    m.compile(loss={"ctc": lambda a, b: b}, optimizer=K.Adam(lr=1e-3, clipvalue=0.5), augment=CFGS[name])

    def batch():
        xs, labels, il, ll = synthetic_arrays(spec, B, T, Lmax, 9, lmin=1, lmax=4)
        return dict(xs, the_labels=labels, input_length=il, label_length=ll)

    def gen():
        while True:
            yield batch(), None
    hist = m.fit_generator(gen(), steps_per_epoch=2, epochs=1, verbose=0)
    assert np.all(np.isfinite(hist.history["loss"]))
    eng = m._engine
    assert eng._augment is not None and eng._augment["cfg"]["segments"] == CFGS[name]["segments"] and eng.rng_step >= 2
    with pytest.raises(ValueError, match="segments"):
        m.set_augment(dict(segments=17))
    assert eng._augment is not None and m._augment == CFGS[name]         # (the refused config left the previous one in force)
    m.set_augment(None)
    assert eng._augment is None and m._augment is None and "skeletal" not in eng.X
    assert np.isfinite(m.train_on_batch(batch()))
