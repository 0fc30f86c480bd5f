"""-m gpu: engines given per-sample sequence lengths (inputs["seq_length"]) against the fp64 oracle run on every sample
ALONE at its own length (tests/seqlen_ref.py::truncated), under the replayed randomness of tests/rng_cases.py.  The cases are cut
to seqlen_ref.LENS; input_length = len - 2 throughout.

Bounds are tests/test_gpu_rng_replay.py's: 1e-4 on loss, loss_b and P[b, :len], 2e-4 of a gradient tensor's largest entry.  The
same step WITHOUT the lengths (same input_length) is the padded computation and misses them by one to two orders of magnitude
(tests/test_cpu_seqlen.py's negative control): that is what every comparison here can see.  Padding invariance, the pipelined
schedule and "no key, no call" are compared on bits."""
import copy

import numpy as np
import pytest

from mgr_amd import decoding
from tests import rng_cases as rc
from tests import seqlen_ref as sr
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_engine(device, c, seed=None, **kw):
    from mgr_amd.engine import Engine
    from mgr_amd.spec import NetworkSpec
    eng = Engine(NetworkSpec.from_dict(c["spec"]), c["B"], c["T"], c["Lmax"], device=device, seed=c["seed"] if seed is None else seed, **kw)
    eng.set_weights(c["w0"])
    return eng


def with_len(inputs, lens):
    return dict(inputs, seq_length=np.asarray(lens, np.int32))


def run_step(eng, c, inputs, lens, rand=None):
    """One step without update at input_length = len - 2; everything it computed."""
    eng.enqueue_train_step(inputs, c["labels"], sr.il_of(lens), c["ll"], rand=rand, apply_update=False)
    loss = eng.read_loss()
    return dict(loss=loss, loss_b=eng.loss_b.download(), P=eng.P.download(), g=eng.get_grads())


def figures(got, ref, lens):
    """Deviations of a step from the truncated oracle: mean loss, worst loss_b, worst P[b, :len] (each relative), per gradient tensor."""
    loss, lb, g, Ps = ref
    return dict(loss=abs(got["loss"] - loss) / abs(loss), loss_b=float((np.abs(got["loss_b"] - lb) / np.abs(lb)).max()),
                P=max(rel_err(got["P"][b, :n], Ps[b]) for b, n in enumerate(lens)), g=sr.worst(got["g"], g))


def assert_truncated(got, ref, lens, what):
    f = figures(got, ref, lens)
    print("%s: loss %.3e  loss_b %.3e  P %.3e  worst gradient %.3e (%s)" % (what, f["loss"], f["loss_b"], f["P"], max(f["g"].values()),
                                                                            max(f["g"], key=f["g"].get)))
    assert set(got["g"]) == set(ref[2])
    assert f["loss"] <= 1e-4 and f["loss_b"] <= 1e-4 and f["P"] < 1e-4, (what, f)
    bad = {k: e for k, e in f["g"].items() if not e < 2e-4}
    assert not bad, (what, bad)
    return f


def same_bits(a, b, lens, what):
    assert a["loss"] == b["loss"], (what, a["loss"], b["loss"])
    assert np.array_equal(bits(a["loss_b"]), bits(b["loss_b"])), what
    for i, n in enumerate(lens):
        assert np.array_equal(bits(a["P"][i, :n]), bits(b["P"][i, :n])), (what, i)
    for k in a["g"]:
        assert np.array_equal(bits(a["g"][k]), bits(b["g"][k])), (what, k)


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


# ------------------------------------------------------------------------------------------------------------ a. one step
@pytest.mark.parametrize("mode", ["replay_given", "device_rng"])
@pytest.mark.parametrize("name", sr.NAMES)
def test_step_with_lengths_is_the_truncated_computation_and_without_them_is_not(device, name, mode):
    """replay_given: the step is handed rand = replay(seed, 0); device_rng: it draws on the device (rand=None) what the replay
    restates.  Either way the oracle is each sample alone at its length under that randomness cut to the sample."""
    c, lens = rc.case(name), sr.LENS[name]
    ref = sr.truncated_step(name)
    assert np.all(np.isfinite(ref[1])) and min(lens) < c["T"] == max(lens)
    rand = c["rands"][0] if mode == "replay_given" else None
    eng = make_engine(device, c)
    try:
        assert_truncated(run_step(eng, c, with_len(c["inputs"], lens), lens, rand), ref, lens, "%s %s with lengths" % (name, mode))
        assert eng.rng_step == 1
    finally:
        eng.close()
    eng = make_engine(device, c)
    try:
        f = figures(run_step(eng, c, c["inputs"], lens, rand), ref, lens)
        print("%s %s WITHOUT lengths: loss_b %.3e  gradients %.3e .. %.3e" % (name, mode, f["loss_b"], min(f["g"].values()), max(f["g"].values())))
        assert f["loss_b"] > 1e-3 and min(f["g"].values()) > 2e-3, "the comparison could not tell the padded computation from the truncated one"
    finally:
        eng.close()


# --------------------------------------------------------------------------------------------------- b. padding invariance
@pytest.mark.parametrize("name", sr.NAMES)
def test_results_do_not_depend_on_what_the_padding_holds(device, name):
    c, lens = rc.case(name), sr.LENS[name]
    zero, rep = sr.repeated_tails(c, lens)
    assert any(not np.array_equal(zero[k], rep[k]) for k in zero)
    out = {}
    for key, inputs, ln in (("zero", zero, lens), ("rep", rep, lens), ("zero_plain", zero, None), ("rep_plain", rep, None),
                            ("full", zero, (c["T"],) * c["B"])):
        eng = make_engine(device, c)
        try:
            if key == "full":       # (every length T: input_length stays the case's T - 2, as in the plain step below)
                eng.enqueue_train_step(with_len(inputs, ln), c["labels"], c["il"], c["ll"], apply_update=False)
                out[key] = dict(loss=eng.read_loss(), loss_b=eng.loss_b.download(), P=eng.P.download(), g=eng.get_grads())
                eng2 = make_engine(device, c)
                try:
                    eng2.enqueue_train_step(inputs, c["labels"], c["il"], c["ll"], apply_update=False)
                    out["none"] = dict(loss=eng2.read_loss(), loss_b=eng2.loss_b.download(), P=eng2.P.download(), g=eng2.get_grads())
                finally:
                    eng2.close()
            else:
                out[key] = run_step(eng, c, inputs if ln is None else with_len(inputs, ln), lens)
        finally:
            eng.close()
    same_bits(out["zero"], out["rep"], lens, name + ": zero tails against repeated frames")
    assert np.all(np.isfinite(out["zero"]["loss_b"]))
    # without the lengths the two paddings are two batches
    assert out["zero_plain"]["loss"] != out["rep_plain"]["loss"]
    assert not np.array_equal(bits(out["zero_plain"]["loss_b"]), bits(out["rep_plain"]["loss_b"]))
    # every length T: the bits of a step without lengths
    same_bits(out["full"], out["none"], (c["T"],) * c["B"], name + ": seq_length = T against no seq_length")


# ------------------------------------------------------------------------------------------------ c. the pipelined schedule
PIPE_LENS = [(12, 8, 6), (7, 12, 5), (9, 6, 12), (12, 12, 3)]


def test_pipelined_steps_equal_unpipelined_steps_and_each_pass_uses_its_own_lengths(device):
    name = "fusion_tiny"
    c = rc.case(name)
    assert PIPE_LENS[0] == sr.LENS[name] and all(np.all(sr.il_of(ln).reshape(-1) >= np.asarray(c["ll"]).reshape(-1)) for ln in PIPE_LENS)
    batches = [with_len(c["inputs"], ln) for ln in PIPE_LENS]        # (distinct dicts: a prefetched pass is matched by identity)
    out = []
    for pipelined in (True, False):
        eng = make_engine(device, c)
        try:
            assert eng.can_pipeline and eng.schedule.pipeline
            losses = []
            for i, (x, ln) in enumerate(zip(batches, PIPE_LENS)):
                kw = {}
                if pipelined and i + 1 < 4:
                    kw["next_inputs"] = batches[i + 1]
                    if i + 2 < 4:
                        kw["after_next_inputs"] = batches[i + 2]
                losses.append(eng.train_step(x, c["labels"], sr.il_of(ln), c["ll"], **kw))
            device.sync()
            assert eng.rng_step == 4 and eng.iterations == 4
            out.append((losses, eng.get_weights()))
        finally:
            eng.close()
    (la, wa), (lb, wb) = out
    print("pipelined %s unpipelined %s" % (la, lb))
    assert la == lb and np.all(np.isfinite(la)), (la, lb)
    for k in wa:
        assert np.array_equal(bits(wa[k]), bits(wb[k])), k
    ref = sr.truncated_step(name)
    assert abs(la[0] - ref[0]) <= 1e-4 * abs(ref[0]), (la[0], ref[0])
    # (the four batches differ in nothing but their lengths: steps of one batch's lengths applied to another's pass would show here)
    assert len(set(la)) == 4


# ------------------------------------------------------------------------------------------------------------ d. calls made
def _count_scans(monkeypatch, eng):
    """[(jobs, reverse jobs that keep their gates)] per multi-scan call of the engine."""
    seen = []
    scan = eng._scan_multi

    def counting(jobs, *a, **kw):
        seen.append((len(jobs), sum(1 for j in jobs if j["reverse"] and j["gates"])))
        return scan(jobs, *a, **kw)
    monkeypatch.setattr(eng, "_scan_multi", counting)
    return seen


@pytest.mark.parametrize("name", ["fusion_tiny", "unimodal_tiny"])
def test_without_the_key_no_fill_is_enqueued_before_or_after_batches_with_lengths(device, monkeypatch, name):
    c, lens = rc.case(name), sr.LENS[name]
    seen = []
    for had_lengths in (False, True):
        eng = make_engine(device, c)
        try:
            if had_lengths:
                scans = _count_scans(monkeypatch, eng)
                calls = _Calls(monkeypatch, device)
                run_step(eng, c, with_len(c["inputs"], lens), lens)
                monkeypatch.undo()
                fills = calls.names().count("mgr_seq_zero_tail")
                # one fill per scan call for Z, one more per scan call that keeps reverse gates
                assert len(scans) >= 2 and fills == len(scans) + sum(1 for _, kept in scans if kept), (fills, scans)
                # fusion_tiny: 2 frozen encoder depths + the fusion layer, which keeps its gates; unimodal_tiny: 2 trainable depths
                assert fills == 4
                eng.predict(with_len(c["inputs"], lens))
                eng.rng_step = 0        # (the step below draws what the other engine's first step draws)
            calls = _Calls(monkeypatch, device)
            got = run_step(eng, c, c["inputs"], lens)
            monkeypatch.undo()
            seen.append((calls.names(), got))
        finally:
            monkeypatch.undo()
            eng.close()
    (na, ga), (nb, gb) = seen
    assert "mgr_seq_zero_tail" not in na and na == nb
    same_bits(ga, gb, (c["T"],) * c["B"], name)


# ------------------------------------------------------------------------------------------------------------- e. inference
@pytest.mark.parametrize("name", sr.NAMES)
def test_predict_and_the_loss_passes_honour_the_lengths(device, name):
    c, lens = rc.case(name), sr.LENS[name]
    x = with_len(c["inputs"], lens)
    eng = make_engine(device, c)
    try:
        P = eng.predict(x)
        for b, (n, ref) in enumerate(zip(lens, sr.forward_truncated(c, lens))):
            assert rel_err(P[b, :n], ref) < 1e-4, (name, b)
            assert np.array_equal(bits(P[b, n:]), np.zeros_like(bits(P[b, n:]))), (name, b)
        assert eng.rng_step == 0
        # learning phase 0, no randomness: each sample's loss alone at its length
        lb = eng.loss_on_batch(x, c["labels"], sr.il_of(lens), c["ll"], train_phase=False)
        ref_lb = sr.truncated(c, None, lens)[1]
        assert np.allclose(lb, ref_lb, rtol=1e-4), (lb, ref_lb)
        plain = eng.loss_on_batch(c["inputs"], c["labels"], sr.il_of(lens), c["ll"], train_phase=False)
        assert float((np.abs(plain - ref_lb) / np.abs(ref_lb)).max()) > 1e-3
        # learning phase 1 under the replay of step 0
        Pt = eng.forward_train_phase(x, rand=c["rands"][0])
        for b, (n, ref) in enumerate(zip(lens, sr.truncated_step(name)[3])):
            assert rel_err(Pt[b, :n], ref) < 1e-4, (name, b)
            assert not Pt[b, n:].any()
    finally:
        eng.close()


def test_predict_stream_decodes_what_the_truncated_posteriors_decode_to(device):
    name = "fusion_tiny"
    c = rc.case(name)
    skip = int(c["spec"]["ctc"]["skip"])
    lens_by_batch = [sr.LENS[name], (5, 12, 9), (12, 12, 12)]
    eng = make_engine(device, c)
    try:
        Ps = [eng.predict(with_len(c["inputs"], ln)) for ln in lens_by_batch]
        post = list(eng.predict_stream([with_len(c["inputs"], ln) for ln in lens_by_batch]))
        for P, Q in zip(Ps, post):
            assert np.array_equal(bits(P), bits(Q))
        greedy = list(eng.predict_stream([with_len(c["inputs"], ln) for ln in lens_by_batch], output="argmax"))
        beam = list(eng.predict_stream([with_len(c["inputs"], ln) for ln in lens_by_batch], output="beam", beam_width=4))
        for P, ln, (best, prob), (paths, logp) in zip(Ps, lens_by_batch, greedy, beam):
            for b, n in enumerate(ln):
                cut = np.ascontiguousarray(P[b:b + 1, :n])          # the sample's posteriors alone, n frames
                rbest, rprob = decoding.frame_argmax(cut, skip=skip, dev=device)
                assert np.array_equal(best[b, :n - skip], rbest[0]) and np.array_equal(bits(prob[b, :n - skip]), bits(rprob[0])), (ln, b)
                assert np.all(best[b, n - skip:] == -1) and not prob[b, n - skip:].any()
                rpaths, rlogp = decoding.beam_search_decode(cut, beam_width=4, skip=skip, dev=device)
                assert paths[b] == rpaths[0] and logp[b] == rlogp[0], (ln, b, paths[b], rpaths[0])
        # a batch without lengths in the same stream decodes all T - skip frames, as before
        mixed = list(eng.predict_stream([with_len(c["inputs"], lens_by_batch[0]), c["inputs"]], output="beam", beam_width=4))
        plain = list(eng.predict_stream([c["inputs"]], output="beam", beam_width=4))
        assert mixed[0][0] == beam[0][0] and mixed[1][0] == plain[0][0] and np.array_equal(mixed[1][1], plain[0][1])
        with pytest.raises(ValueError, match="greedy segment"):
            list(eng.predict_stream([with_len(c["inputs"], lens_by_batch[0])], output="segments"))
        assert np.array_equal(bits(eng.predict(with_len(c["inputs"], lens_by_batch[0]))), bits(Ps[0]))      # (still usable)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------- f. combinations, refusals
def test_entropy_mode_with_lengths_is_finite_and_padding_invariant(device):
    name = "fusion_tiny"
    c, lens = rc.case(name), sr.LENS[name]
    zero, rep = sr.repeated_tails(c, lens)
    out = []
    for inputs in (zero, rep):
        eng = make_engine(device, c)
        try:
            eng.set_entropy(dict(weight=0.1))
            got = run_step(eng, c, with_len(inputs, lens), lens)
            got["entropy"] = eng.last_entropy
            out.append(got)
        finally:
            eng.close()
    a, b = out
    assert np.isfinite(a["loss"]) and np.isfinite(a["entropy"]) and all(np.all(np.isfinite(v)) for v in a["g"].values())
    same_bits(a, b, lens, "entropy mode")
    assert a["entropy"] == b["entropy"]


def test_refusals_raise_before_anything_is_enqueued_and_leave_the_engine_usable(device, monkeypatch):
    name = "fusion_tiny"
    c, lens = rc.case(name), sr.LENS[name]
    x = with_len(c["inputs"], lens)
    ref = sr.truncated_step(name)
    eng = make_engine(device, c)
    try:
        calls = _Calls(monkeypatch, device)
        too_long = sr.il_of(lens).copy()
        too_long[1, 0] += 1
        with pytest.raises(ValueError, match="input_length"):
            eng.train_step(x, c["labels"], too_long, c["ll"], apply_update=False)
        with pytest.raises(ValueError, match="input_length"):         # (the case's own T - 2 is above len - 2 of the shortened samples)
            eng.loss_on_batch(x, c["labels"], c["il"], c["ll"])
        with pytest.raises(ValueError, match="outside"):
            eng.train_step(with_len(c["inputs"], (c["T"] + 1,) + tuple(lens[1:])), c["labels"], sr.il_of(lens), c["ll"], apply_update=False)
        with pytest.raises(ValueError, match="outside"):
            eng.train_step(c["inputs"], c["labels"], c["il"], c["ll"], apply_update=False, next_inputs=with_len(c["inputs"], (-1, 3, 3)))
        with pytest.raises(ValueError, match="shape"):
            eng.predict(with_len(c["inputs"], lens[:2]))
        eng.set_augment(dict(segments=2, max_shift=1))
        with pytest.raises(ValueError, match="set_augment"):
            eng.train_step(x, c["labels"], sr.il_of(lens), c["ll"], apply_update=False)
        eng.set_augment(None)
        monkeypatch.undo()
        work = ("mgr_lstm", "mgr_seq", "mgr_head", "mgr_dense", "mgr_ctc", "mgr_add", "mgr_dropout", "mgr_transpose")
        assert not [n for n in calls.names() if n.startswith(work)] and eng.rng_step == 0 and eng._step_id == 0, calls.names()
        assert_truncated(run_step(eng, c, x, lens), ref, lens, "after the refusals")
    finally:
        monkeypatch.undo()
        eng.close()


# --------------------------------------------------------------------------------------------------------------- g. the facade
def test_facade_fits_from_a_true_lengths_generator_and_takes_batches_with_and_without_the_key(device):
    from mgr_amd import keras_like as K
    from mgr_amd.datagen import BaseDataGenerator, SyntheticStore
    from mgr_amd.spec import NetworkSpec
    name = "fusion_tiny"
    c = rc.case(name)
    spec = NetworkSpec.from_dict(copy.deepcopy(c["spec"]))
    B, T, Lmax = c["B"], c["T"], c["Lmax"]
    Fa, Fs = (s["F"] for s in c["spec"]["streams"])

    class Gen(BaseDataGenerator):
        streams = (("audio", "audio", "fa"), ("skeletal", "skeletal", "fs"))

        def __init__(self, true_lengths):
            self.fa, self.fs = Fa, Fs
            store = SyntheticStore(4 * B, {"audio": (Fa, 3.0), "skeletal": (Fs, 1.0)}, T, c["spec"]["head"]["C"], lmin=1, lmax=2)
            self._setup(B, T, c["spec"]["head"]["C"], "val", 0.0, Lmax, store, true_lengths=true_lengths)

    gen = Gen(True)
    first = gen.get_batch(False)[0]
    assert first["seq_length"].shape == (B, 1) and first["seq_length"].min() < T and np.all(first["input_length"] == first["seq_length"] - 2)
    m = K.Model(spec, device=device, seed=3)
    m.compile(loss={"ctc": lambda a, b: b}, optimizer=K.Adam(lr=1e-3, clipvalue=0.5))
    hist = m.fit_generator(gen.next_val(), steps_per_epoch=2, epochs=1, verbose=0)
    assert len(hist.history["loss"]) == 1 and np.all(np.isfinite(hist.history["loss"]))
    with_key = Gen(True).get_batch(False)[0]
    without = Gen(False).get_batch(False)[0]
    assert "seq_length" not in without
    la, lb, lc = m.train_on_batch(with_key), m.train_on_batch(without), m.train_on_batch(with_key)
    assert np.all(np.isfinite([la, lb, lc]))
    assert np.isfinite(m.test_on_batch(with_key)) and np.isfinite(m.test_on_batch(without))
    P = m.predict_on_batch(with_key)
    for b, n in enumerate(with_key["seq_length"].reshape(-1)):
        assert not P[b, n:].any() and P[b, :n].all()
