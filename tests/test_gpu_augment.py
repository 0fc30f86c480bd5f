"""-m gpu: mgr_augment_plan / mgr_augment_apply (csrc/augment.hip) against the numpy restatement tests/augment_ref.py.  Every
comparison is == on bits: the plan is integers, the warp's interpolation is four float32 operations rounded one by one on both
sides, and the noise is the device function mgr_add_gaussian_noise uses, so apply(stddev) is held to that call over apply(0)."""
import ctypes as C

import numpy as np
import pytest

from mgr_amd import augment
from tests import augment_ref as ar

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def streams(*Fs):
    return [dict(name="s%d" % i, F=F) for i, F in enumerate(Fs)]


def table(norm):
    return [(s["F"], s["time_masks"], s["time_width"], s["feature_masks"], s["feature_width"]) for s in norm["streams"]]


def device_plan(device, norm, B, T, seed):
    plan = device.empty((B, augment.plan_len(norm)), np.int32)
    try:
        augment.enqueue_plan(device, norm, augment.stream_table(norm), B, T, seed, plan)
        return plan.download()
    finally:
        device.free(plan)


def device_apply(device, norm, x, plan, si=0, stddev=0.0, seed=0):
    """mgr_augment_apply of stream si over host array x under the host plan rows `plan`."""
    B, T, F = x.shape
    X, Y, P = device.array(np.ascontiguousarray(x, np.float32)), device.empty((B, T, F)), device.array(np.ascontiguousarray(plan, np.int32))
    try:
        Y.upload(np.full((B, T, F), 7.25, np.float32))       # (every element must be written)
        augment.enqueue_apply(device, norm, si, X, Y, P, B, T, stddev, seed)
        return Y.download()
    finally:
        device.free(X, Y, P)


def ref_plan(norm, B, T, seed):
    return ar.plan_ref(B, T, table(norm), norm["segments"], norm["max_shift"], norm["n_t"], norm["n_f"], norm["drop_thresh"], seed)


def ref_apply(norm, x, plan, si=0):
    return ar.apply_ref(x, plan, norm["segments"], norm["n_t"], norm["n_f"], len(norm["streams"]), si, norm["streams"][si]["fill"])


def batch(rng, B, T, F):
    return rng.standard_normal((B, T, F)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------- the plan
PLAN_CFG = dict(segments=3, max_shift=2, time_masks=2, time_width=5, feature_masks=1, feature_width=3, stream_drop=0.5)


@pytest.mark.parametrize("seed", [0, 5, (1 << 62) + 20131901], ids=["0", "5", "above_2_62"])
def test_plan_matches_the_restatement(device, seed):
    B, T = 5, 23
    norm = augment.normalize_config(PLAN_CFG, streams(7, 4), T)
    assert augment.plan_len(norm) == ar.plan_len(2, 3, 2, 1) == 17
    assert seed < (1 << 62) or seed * 0xD1342543DE82EF95 >= 2 ** 64       # (the seed product wraps)
    got, ref = device_plan(device, norm, B, T, seed), ref_plan(norm, B, T, seed)
    assert got.dtype == np.int32 and np.array_equal(got, ref), (got, ref)
    assert np.any(ref[:, 1:3] != ar.sources(T, 3)[1:3])


def test_plan_matches_at_the_flagship_shape_and_with_per_stream_settings(device):
    B, T = 64, 1900
    cfg = dict(segments=16, max_shift=40, time_masks=2, time_width=100, feature_masks=2, feature_width=8, stream_drop=0.2,
               streams={"s1": dict(time_masks=1, feature_masks=0)})
    norm = augment.normalize_config(cfg, streams(39, 20), T)
    got, ref = device_plan(device, norm, B, T, 1234), ref_plan(norm, B, T, 1234)
    assert np.array_equal(got, ref)
    assert len(set(ref[:, 17].tolist())) == 3       # (no stream, the first, the second)


# ------------------------------------------------------------------------------------------------------ apply, without noise
APPLY_CASES = {
    # name: (B, T, Fs, cfg)
    "b3_t12_f39_f20": (3, 12, (39, 20), dict(segments=2, max_shift=2, time_masks=2, time_width=4, feature_masks=1, feature_width=5,
                                             stream_drop=0.5, streams={"s1": dict(fill=-2.5)})),
    "b5_t23_f7_odd": (5, 23, (7,), dict(segments=3, max_shift=2, time_masks=2, time_width=5, feature_masks=1, feature_width=3)),
    "b2_t257_f1": (2, 257, (1,), dict(segments=16, max_shift=7, time_masks=1, time_width=30)),
    "k1": (5, 23, (7,), dict(segments=1, time_masks=2, time_width=5, feature_masks=1, feature_width=3)),
    "d0": (5, 23, (7,), dict(segments=3, max_shift=0, time_masks=1, time_width=5)),
    "blocks_2": (40, 23, (7,), dict(segments=3, max_shift=3)),       # 6440 elements: more than one workgroup
    # several frame ranges per sample (a workgroup takes 4096 / F frames, at most 255): 105 + 105 + 20 frames at F 39, and 99 + 12
    # at F 41 with T F odd - the last noise pair of a range reaches into the next range, the last of a sample into the next sample
    "ranges_3": (2, 230, (39,), dict(segments=16, max_shift=6, time_masks=2, time_width=40, feature_masks=2, feature_width=8)),
    "ranges_2_odd": (3, 111, (41, 3), dict(segments=5, max_shift=10, time_masks=1, time_width=30, feature_masks=1, feature_width=2,
                                           stream_drop=0.5)),
}


def case_inputs(name):
    """{stream name: float32 [B, T, F]} of an apply case, in stream order."""
    B, T, Fs, cfg = APPLY_CASES[name]
    rng = np.random.default_rng(len(name))
    return {"s%d" % i: batch(rng, B, T, F) for i, F in enumerate(Fs)}


@pytest.mark.parametrize("name", list(APPLY_CASES))
def test_apply_matches_the_restatement(device, name):
    """Through the public call: augment.augment_batch on the shared Device draws the plan and applies it to every stream."""
    B, T, Fs, cfg = APPLY_CASES[name]
    norm = augment.normalize_config(cfg, streams(*Fs), T)
    x = case_inputs(name)
    held = len(device._arrays)
    got, plan = augment.augment_batch(x, cfg, 77, device=device)
    assert len(device._arrays) == held, "augment_batch left arrays on the caller's Device"
    ref, rplan = ar.augment_ref(x, norm, 77)
    assert plan.dtype == np.int32 and np.array_equal(plan, rplan)
    K = norm["segments"]
    if norm["max_shift"] > 0:
        assert np.any(plan[:, :K + 1] != ar.sources(T, K))
    assert list(got) == list(x)
    for k in x:
        assert got[k].dtype == np.float32 and np.array_equal(bits(got[k]), bits(ref[k])), (name, k, int((bits(got[k]) != bits(ref[k])).sum()))
        if norm["max_shift"] == 0 and norm["n_t"] == 0 and norm["n_f"] == 0:
            assert np.array_equal(bits(got[k]), bits(x[k]))


def test_augment_batch_on_a_device_of_its_own_and_on_the_callers(device):
    """Two streams with stream_drop: given a GPU index the call opens and closes its own Device, given a Device it uses that one and
    leaves nothing on it; both give the restatement's bits and each other's.  float64 inputs are taken as float32; the streams are
    those of the dict, in its order; arrays that disagree on (B, T) are refused."""
    B, T = 6, 23
    cfg = dict(PLAN_CFG, streams={"skeletal": dict(fill=-1.0, time_masks=1)})
    rng = np.random.default_rng(42)
    x = {"audio": rng.standard_normal((B, T, 7)), "skeletal": rng.standard_normal((B, T, 4))}       # (float64, as generators yield)
    norm = augment.normalize_config(cfg, [dict(name="audio", F=7), dict(name="skeletal", F=4)], T)
    x32 = {k: v.astype(np.float32) for k, v in x.items()}
    ref, rplan = ar.augment_ref(x32, norm, 2015)
    drop = rplan[:, norm["segments"] + 1]
    assert {-1, 0, 1} == set(drop.tolist()), "the case must hold an undropped sample and one dropped sample per stream"
    held = len(device._arrays)
    mine, mplan = augment.augment_batch(x, cfg, 2015, device=device)
    assert len(device._arrays) == held
    own, oplan = augment.augment_batch(x, cfg, 2015, device=0)
    for got, plan in ((mine, mplan), (own, oplan)):
        assert np.array_equal(plan, rplan) and list(got) == ["audio", "skeletal"]
        for k in ref:
            assert np.array_equal(bits(got[k]), bits(ref[k])), k
    for b in range(B):
        if drop[b] == 0:
            assert np.all(mine["audio"][b] == 0.0)
        if drop[b] == 1:
            assert np.all(mine["skeletal"][b] == -1.0)
    # the streams' order is the dict's: the other order is another plan layout (F 4 first) and drops the other stream
    swapped, splan = augment.augment_batch({"skeletal": x["skeletal"], "audio": x["audio"]}, dict(PLAN_CFG), 2015, device=device)
    snorm = augment.normalize_config(PLAN_CFG, [dict(name="skeletal", F=4), dict(name="audio", F=7)], T)
    sref, srplan = ar.augment_ref({"skeletal": x32["skeletal"], "audio": x32["audio"]}, snorm, 2015)
    assert np.array_equal(splan, srplan) and all(np.array_equal(bits(swapped[k]), bits(sref[k])) for k in sref)
    with pytest.raises(ValueError, match="skeletal"):
        augment.augment_batch({"audio": x["audio"], "skeletal": x["skeletal"][:, :T - 1]}, cfg, 2015, device=device)
    with pytest.raises(ValueError, match="feature_width"):
        augment.augment_batch({"audio": x["audio"][:, :, :2]}, dict(feature_masks=1, feature_width=3), 0, device=device)
    assert len(device._arrays) == held


def test_apply_with_the_last_segment_at_its_narrowest(device):
    """Every inner target at +D: the last segment spans den = a_K - a_{K-1} - D target frames, its frames step fastest through the
    source and the last frame is the source's last, copied."""
    B, T, F, K, D = 3, 23, 7, 3, 3
    norm = augment.normalize_config(dict(segments=K, max_shift=D), streams(F), T)
    a = ar.sources(T, K)
    plan = ref_plan(norm, B, T, 1)
    plan[:, 1:K] = a[1:K] + D
    i0, rem, den = ar.frames(plan[0], T, K)
    assert den[T - 1] == a[K] - a[K - 1] - D and i0[T - 1] == T - 1 and rem[T - 1] == 0
    x = batch(np.random.default_rng(3), B, T, F)
    got = device_apply(device, norm, x, plan)
    assert np.array_equal(bits(got), bits(ref_apply(norm, x, plan)))
    assert np.array_equal(bits(got[:, T - 1]), bits(x[:, T - 1])) and np.array_equal(bits(got[:, 0]), bits(x[:, 0]))


def test_apply_with_a_whole_sample_masked(device):
    B, T, F = 3, 12, 5
    norm = augment.normalize_config(dict(segments=2, max_shift=1, time_masks=1, time_width=T, fill=0.5), streams(F), T)
    plan = ref_plan(norm, B, T, 4)
    plan[1, 2 + 2:2 + 4] = (0, T)         # sample 1: one mask over all T frames
    plan[0, 2 + 2:2 + 4] = (T, 0)         # sample 0: an empty mask at the far end
    x = batch(np.random.default_rng(8), B, T, F)
    got = device_apply(device, norm, x, plan)
    assert np.array_equal(bits(got), bits(ref_apply(norm, x, plan)))
    assert np.all(got[1] == 0.5) and not np.any(got[0] == 0.5)


def test_apply_copies_negative_zero_nan_payloads_and_denormals(device):
    B, T, F, K = 2, 23, 7, 3
    x = batch(np.random.default_rng(9), B, T, F)
    x[:, ::2] = -0.0
    x.view(np.uint32)[0, 1, 3] = 0x7FC01234
    x[1, 3, 2] = np.float32(1e-42)
    ident = augment.normalize_config(dict(segments=K, max_shift=0), streams(F), T)
    got = device_apply(device, ident, x, ref_plan(ident, B, T, 2))
    assert np.array_equal(bits(got), bits(x))
    warped = augment.normalize_config(dict(segments=K, max_shift=3), streams(F), T)
    plan = ref_plan(warped, B, T, 2)
    got, ref = device_apply(device, warped, x, plan), ref_apply(warped, x, plan)
    assert np.array_equal(bits(got), bits(ref))
    copied = [ar.frames(plan[b], T, K)[1] == 0 for b in range(B)]
    assert all(np.array_equal(bits(got[b, c]), bits(x[b, ar.frames(plan[b], T, K)[0][c]])) for b, c in enumerate(copied))
    assert (bits(got) == 0x80000000).any()


# ------------------------------------------------------------------------------------------------------------------- noise
def device_noise(device, x, stddev, seed):
    X, Y = device.array(np.ascontiguousarray(x, np.float32)), device.empty(x.shape)
    try:
        device.call("mgr_add_gaussian_noise", X, Y, X.size, float(stddev), C.c_uint64(seed))
        return Y.download()
    finally:
        device.free(X, Y)


@pytest.mark.parametrize("B, T, F", [(5, 23, 7), (3, 111, 41)], ids=["b5_t23_f7", "b3_t111_f41_ranges"])
def test_apply_with_noise_is_the_noise_call_over_apply_without(device, B, T, F):
    """T F is odd (161; 4551), so every other sample starts on the second element of a noise pair - the pair straddles two samples,
    two plan rows; at T 111, F 41 a sample is also two frame ranges of the kernel (99 + 12 frames)."""
    assert (T * F) % 2 == 1
    x = batch(np.random.default_rng(11), B, T, F)
    seed = (1 << 63) + 12345
    norm = augment.normalize_config(PLAN_CFG, streams(F, 4), T)
    plan = ref_plan(norm, B, T, 6)
    clean = device_apply(device, norm, x, plan)
    assert np.array_equal(bits(clean), bits(ref_apply(norm, x, plan)))
    noisy = device_apply(device, norm, x, plan, stddev=0.5, seed=seed)
    assert np.array_equal(bits(noisy), bits(device_noise(device, clean, 0.5, seed)))
    assert not np.array_equal(bits(noisy), bits(clean))
    ident = augment.normalize_config({}, streams(F, 4), T)
    got = device_apply(device, ident, x, ref_plan(ident, B, T, 6), stddev=0.5, seed=seed)
    assert np.array_equal(bits(got), bits(device_noise(device, x, 0.5, seed)))


# ------------------------------------------------------------------------------------------------- nothing behind the buffer
def test_the_last_frame_does_not_depend_on_what_follows_the_buffer(device):
    """X is the first B T F floats of ONE allocation and `after` the T F floats right behind it - where row T of the last sample would
    be - holding huge values in one run and NaN in the other.  The last frame (and every other) is exact both times, under the
    identity and under a warped plan: the row behind i0 = T - 1 takes no part, not even multiplied by a zero weight (0 x NaN)."""
    B, T, F, K = 2, 12, 5, 2
    x = batch(np.random.default_rng(13), B, T, F)
    whole = device.empty((B * T * F + T * F,))
    X, after = whole.view(0, (B, T, F)), whole.view(B * T * F, (T, F))
    Y = device.empty((B, T, F))
    try:
        assert after.ptr == X.ptr + B * T * F * 4
        X.upload(x)
        for cfg in (dict(segments=K, max_shift=0), dict(segments=K, max_shift=2)):
            norm = augment.normalize_config(cfg, streams(F), T)
            plan = ref_plan(norm, B, T, 21)
            P = device.array(plan)
            ref = ref_apply(norm, x, plan)
            for junk in (np.float32(3e38), np.float32(np.nan)):
                after.upload(np.full((T, F), junk, np.float32))
                augment.enqueue_apply(device, norm, 0, X, Y, P, B, T)
                got = Y.download()
                assert np.array_equal(bits(got[:, T - 1]), bits(x[:, T - 1])), (cfg, junk)
                assert np.array_equal(bits(got), bits(ref)), (cfg, junk)
            device.free(P)
    finally:
        device.free(whole, Y)


def test_apply_refuses_what_it_cannot_do(device):
    from mgr_amd._capi import MgrError
    norm = augment.normalize_config(dict(segments=2, max_shift=1), streams(5), 12)
    X = device.zeros((2, 12, 5))
    P = device.array(ref_plan(norm, 2, 12, 0))
    try:
        with pytest.raises(MgrError, match="in place"):
            augment.enqueue_apply(device, norm, 0, X, X, P, 2, 12)
        with pytest.raises(MgrError, match="shortest"):
            device.call("mgr_augment_plan", 2, 12, 1, 2, 3, 0, 0, augment.stream_table(norm).ctypes.data, 0, C.c_uint64(0), P)
    finally:
        device.free(X, P)
