"""Per-sample sequence lengths on the CPU: the mechanism the engine uses - zero gate pre-activations and zero saved
gates in the tails of the reverse directions, nothing else - restated in fp64 (tests/seqlen_ref.py) equals the per-sample
truncated computation whatever the tails hold, while the padded computation an engine without lengths makes does not; the
checks the engine makes on a batch's lengths; and the data generators' true_lengths batches.

Bounds: 1e-10 for fp64 restatement against fp64 truncation (measured 1.7e-14: the same operations, summed over other batch
shapes); the negative control's floors are 1e-3 (some sample's loss) and 1e-2 (every gradient tensor), measured 3.5e-3 and 1.4e-2."""
import numpy as np
import pytest

import mgr_amd  # noqa: F401
from mgr_amd import seqlen
from mgr_amd.multimodal_fusion.data_generator import DataGenerator
from tests import rng_cases as rc
from tests import seqlen_ref as sr


def _against_truncated(got, ref):
    """(worst relative per-sample loss deviation, {tensor: deviation relative to its largest entry}, worst P deviation at t < len)."""
    _, lb, g, P = got
    _, rlb, rg, rPs = ref
    dl = np.abs(np.asarray(lb).reshape(-1) - rlb) / np.abs(rlb)
    dP = max(float(np.abs(P[b, :len(rP)] - rP).max()) for b, rP in enumerate(rPs))
    return dl, sr.worst(g, rg), dP


@pytest.mark.parametrize("name", sr.NAMES)
def test_every_truncated_loss_is_finite(name):
    _, lb, g, Ps = sr.truncated_step(name)
    assert np.all(np.isfinite(lb)) and all(np.all(np.isfinite(v)) for v in g.values())
    assert [P.shape[0] for P in Ps] == list(sr.LENS[name])


@pytest.mark.parametrize("name", sr.NAMES)
def test_mechanism_equals_truncation_whatever_the_tails_hold(name):
    c, lens = rc.case(name), sr.LENS[name]
    rng = np.random.default_rng(97)
    inputs, rand = sr.with_tails(c, c["rands"][0], lens, lambda shape: 3.0 * rng.standard_normal(shape))
    for b, n in enumerate(lens):      # (the tails really are not what the case had)
        assert n == c["T"] or any(not np.array_equal(inputs[k][b, n:], np.asarray(c["inputs"][k], np.float64)[b, n:]) for k in inputs)
    dl, dg, dP = _against_truncated(sr.mechanism(c, rand, lens, inputs), sr.truncated_step(name))
    print("%s: loss_b %.2e  gradients %.2e  P %.2e" % (name, dl.max(), max(dg.values()), dP))
    assert dl.max() < 1e-10 and max(dg.values()) < 1e-10 and dP < 1e-10


@pytest.mark.parametrize("name", sr.NAMES)
def test_full_lengths_are_the_plain_oracle(name):
    c = rc.case(name)
    loss, lb, g, P = sr.mechanism(c, c["rands"][0], (c["T"],) * c["B"])
    rloss, rlb, rg, rP = sr.padded(c, c["rands"][0], (c["T"],) * c["B"])
    assert loss == rloss and np.array_equal(lb, rlb) and np.array_equal(P, rP)
    for k in rg:
        assert np.array_equal(g[k], rg[k]), k
    # (... and that is the case's own step: T - 2 frames each)
    assert np.array_equal(sr.il_of((c["T"],) * c["B"]).reshape(-1), np.asarray(c["il"]).reshape(-1))


@pytest.mark.parametrize("name", sr.NAMES)
def test_negative_control_the_padded_computation_is_another_model(name):
    c, lens = rc.case(name), sr.LENS[name]
    dl, dg, _ = _against_truncated(sr.padded(c, c["rands"][0], lens), sr.truncated_step(name))
    print("%s: padded vs truncated: loss_b %s  gradients %.2e .. %.2e" % (name, dl, min(dg.values()), max(dg.values())))
    assert dl.max() > 1e-3, dl
    assert min(dg.values()) > 1e-2, dg
    for b, n in enumerate(lens):      # (a sample at its full length is untouched by the others' padding)
        if n == c["T"]:
            assert dl[b] < 1e-10


# ------------------------------------------------------------------------------------------------------------- the checks
def test_normalize_accepts_vectors_and_columns_of_integers():
    for a in ([3, 0, 5], np.array([[3], [0], [5]]), np.array([3.0, 0.0, 5.0]), np.array([3, 0, 5], np.int64)):
        out = seqlen.normalize(a, 3, 5)
        assert out.dtype == np.int32 and out.shape == (3,) and out.tolist() == [3, 0, 5]


@pytest.mark.parametrize("bad", [[3, 4], [[3, 4, 5]], np.zeros((3, 2), int), [3.5, 1, 1], [np.nan, 1, 1], [6, 1, 1], [-1, 1, 1],
                                 [True, False, True], ["a", "b", "c"]])
def test_normalize_refuses(bad):
    with pytest.raises(ValueError):
        seqlen.normalize(bad, 3, 5)


def test_check_batch():
    B, T, skip = 3, 12, 2
    x = {"a": np.zeros((B, T, 2))}
    assert seqlen.check_batch(x, B, T, skip) is None and seqlen.check_batch(None, B, T, skip) is None
    # (without the key nothing else is looked at: such a batch is what it was)
    assert seqlen.check_batch(x, B, T, skip, input_length=[99] * B, data_parallel=True, frontend=True, augment=True) is None
    xl = dict(x, seq_length=[12, 8, 1])
    assert seqlen.check_batch(xl, B, T, skip, input_length=[[10], [6], [0]]).tolist() == [12, 8, 1]
    assert seqlen.frames([12, 8, 1, 0], skip).tolist() == [10, 6, 0, 0]
    for kw in (dict(input_length=[10, 7, 0]), dict(input_length=[10, 6, 1]), dict(input_length=[10, 6]), dict(data_parallel=True),
               dict(frontend=True), dict(augment=True)):
        with pytest.raises(ValueError):
            seqlen.check_batch(xl, B, T, skip, **kw)
    with pytest.raises(ValueError):
        seqlen.check_batch(dict(x, seq_length=[12, 8, 13]), B, T, skip)


# ------------------------------------------------------------------------------------------------------------ the generators
class _Store:
    """Four files: 1 longer than maxlen (truncated), 2 with streams of unequal lengths, 3 without a label row, 4 short."""
    FRAMES = {1: (15, 15), 2: (7, 9), 3: (5, 5), 4: (4, 3)}      # (audio, skeletal)

    def file_ids(self):
        return sorted(self.FRAMES)

    def features(self, fid, modality):
        n = self.FRAMES[fid][0 if modality == "audio" else 1]
        F = 3 if modality == "audio" else 2
        return np.random.default_rng([fid, F]).standard_normal((n, F))

    def labels(self, fid):
        return np.zeros((0,), np.float32) if fid == 3 else np.array([1, 2], np.float32)


def _gen(true_lengths):
    return DataGenerator(4, 2, 3, 10, 6, "val", absolute_max_sequence_len=5, store=_Store(), true_lengths=true_lengths)


def test_true_lengths_off_is_todays_batch():
    plain = DataGenerator(4, 2, 3, 10, 6, "val", absolute_max_sequence_len=5, store=_Store()).get_batch(False)
    off = _gen(False).get_batch(False)
    assert set(plain[0]) == set(off[0]) and "seq_length" not in off[0]
    for k in plain[0]:
        assert plain[0][k].dtype == off[0][k].dtype and np.array_equal(plain[0][k], off[0][k]), k
    assert np.all(off[0]["input_length"] == 8)


def test_true_lengths_on_adds_the_lengths_and_changes_nothing_else():
    off, on = _gen(False).get_batch(False)[0], _gen(True).get_batch(False)[0]
    assert set(on) == set(off) | {"seq_length"}
    for k in off:
        if k != "input_length":
            assert np.array_equal(on[k], off[k]), k
    # truncated file: maxlen; unequal streams: the longer; no label row (all-ones inputs): maxlen; short file: its frames
    assert on["seq_length"].shape == (4, 1) and on["seq_length"].reshape(-1).tolist() == [10, 9, 10, 4]
    assert on["input_length"].shape == (4, 1) and on["input_length"].reshape(-1).tolist() == [8, 7, 8, 2]
    assert np.all(on["the_input_audio"][2] == 1.0) and np.all(on["the_input_audio"][1, 7:] == 0.0)
    seqlen.check_batch({"seq_length": on["seq_length"]}, 4, 10, 2, on["input_length"])
