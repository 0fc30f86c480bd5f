"""CPU suite (no GPU): the augmentation plan's invariants on the numpy restatement (tests/augment_ref.py), the restated apply
step's exact cases, and every refusal of mgr_amd.augment.normalize_config.  tests/test_gpu_augment.py holds the kernels to the
restatement bit for bit; what is shown here is that the restatement itself is a valid, in-range, length-preserving augmentation."""
import math

import numpy as np
import pytest

import mgr_amd  # noqa: F401
from mgr_amd import augment, configs
from tests import augment_ref as ar

SEEDS = 1000
TS, KS = (12, 23, 1900), (1, 2, 3, 16)


def _streams(*Fs):
    return [dict(name="s%d" % i, F=F) for i, F in enumerate(Fs)]


def _max_shift(T, K):
    """The largest D with 2 D < the shortest segment (0 for K = 1: no inner cut)."""
    return 0 if K == 1 else (augment.shortest_segment(T, K) - 1) // 2


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("K", KS)
def test_plan_invariants_over_1000_seeds(T, K):
    """Targets strictly increasing with fixed endpoints, every source row inside [0, T - 1], no read of row i0 + 1 behind the last
    frame, masks inside their axis, at most one dropped stream - at the LARGEST shift the settings allow."""
    if T - 1 < K:
        with pytest.raises(ValueError, match="segments"):
            augment.normalize_config(dict(segments=K), _streams(7, 4), T)
        return
    D = _max_shift(T, K)
    Fs = (7, 4)
    Wt, Wf = min(T, 5), 3
    norm = augment.normalize_config(dict(segments=K, max_shift=D, time_masks=2, time_width=Wt, feature_masks=1, feature_width=Wf,
                                         stream_drop=0.5), _streams(*Fs), T)
    table = [(F, 2, Wt, 1, Wf) for F in Fs]
    B = 2
    moved = 0
    for seed in range(SEEDS):
        plan = ar.plan_ref(B, T, table, K, D, norm["n_t"], norm["n_f"], norm["drop_thresh"], seed * 7919 + 1)
        q = plan[:, :K + 1].astype(np.int64)
        assert np.all(q[:, 0] == 0) and np.all(q[:, K] == T - 1)
        assert np.all(np.diff(q, axis=1) > 0), (seed, q)
        assert np.all(np.abs(q - ar.sources(T, K)) <= D)
        moved += int(np.any(q != ar.sources(T, K)))
        for b in range(B):
            i0, rem, den = ar.frames(plan[b], T, K)
            assert i0.min() >= 0 and i0.max() <= T - 1
            assert np.all(i0[rem != 0] + 1 <= T - 1)
            assert np.all(den > 0) and np.all((rem >= 0) & (rem < den))
            assert i0[0] == 0 and i0[T - 1] == T - 1 and rem[T - 1] == 0
            assert np.all(np.diff(i0) >= 0)             # (the warp is monotone)
        assert np.all((plan[:, K + 1] >= -1) & (plan[:, K + 1] < len(Fs)))
        p = K + 2
        for F in Fs:
            for m in range(3):
                axis, wmax = (T, Wt) if m < 2 else (F, Wf)
                st, w = plan[:, p], plan[:, p + 1]
                assert np.all((w >= 0) & (w <= wmax) & (st >= 0) & (st + w <= axis)), (seed, F, m)
                p += 2
        assert p == plan.shape[1] == ar.plan_len(2, K, 2, 1)
    assert (moved > 0) == (D > 0)


def test_dropped_share_and_each_streams_share():
    """Within 5 binomial standard deviations (the project's mask-count bound) of stream_drop and of stream_drop / S."""
    S, B, T, K = 3, 20000, 12, 2
    for p in (0.5, 0.1):
        thresh = ar.drop_thresh(p)
        plan = ar.plan_ref(B, T, [(4, 0, 0, 0, 0)] * S, K, 0, 0, 0, thresh, 2014)
        drop = plan[:, K + 1]
        share = float((drop >= 0).mean())
        assert abs(share - p) <= 5 * math.sqrt(p * (1 - p) / B), (p, share)
        for s in range(S):
            ps = p / S
            assert abs(float((drop == s).mean()) - ps) <= 5 * math.sqrt(ps * (1 - ps) / B), (p, s)
    assert np.all(ar.plan_ref(64, T, [(4, 0, 0, 0, 0)] * S, K, 0, 0, 0, 0, 2014)[:, K + 1] == -1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_identity_config_returns_the_inputs_bits():
    rng = np.random.default_rng(5)
    B, T, F = 3, 12, 5
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    x[0, 3, 1] = -0.0
    x[1, T - 1, 4] = -0.0
    x.view(np.uint32)[2, 5, 0] = 0x7FC01234          # a NaN with a payload
    x[2, 6, 2] = np.float32(1e-42)                   # a denormal
    for cfg in ({}, dict(segments=1, max_shift=0), dict(segments=3, max_shift=0)):
        norm = augment.normalize_config(cfg, _streams(F), T)
        out, plan = ar.augment_ref({"s0": x}, norm, 17)
        assert np.array_equal(_bits(out["s0"]), _bits(x)), cfg
        assert np.all(plan[:, norm["segments"] + 1] == -1)


def test_ramp_warps_to_the_source_position_and_a_constant_to_itself():
    T, K, D, B = 23, 3, 2, 64
    norm = augment.normalize_config(dict(segments=K, max_shift=D), _streams(1), T)
    ramp = np.broadcast_to(np.arange(T, dtype=np.float32)[None, :, None], (B, T, 1))
    out, plan = ar.augment_ref({"s0": ramp}, norm, 3)
    assert np.any(plan[:, 1:K] != ar.sources(T, K)[1:K])
    for b in range(B):
        i0, rem, den = ar.frames(plan[b], T, K)
        pos = i0 + rem / den                              # the source position, float64
        ulp = np.spacing(np.maximum(pos, 1.0).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(out["s0"][b, :, 0].astype(np.float64) - pos) <= ulp), b
    const = np.full((B, T, 1), np.float32(0.3))
    out, _ = ar.augment_ref({"s0": const}, norm, 3)
    assert np.array_equal(_bits(out["s0"]), _bits(const))


def test_masks_and_the_dropped_stream_become_fill():
    T, B = 12, 16
    cfg = dict(time_masks=1, time_width=T, feature_masks=1, feature_width=2, stream_drop=0.5,
               streams={"s1": dict(fill=-1.5, time_masks=0)})
    norm = augment.normalize_config(cfg, _streams(5, 4), T)
    assert [s["fill"] for s in norm["streams"]] == [0.0, -1.5] and [s["time_masks"] for s in norm["streams"]] == [1, 0]
    x = {"s0": np.ones((B, T, 5), np.float32), "s1": np.ones((B, T, 4), np.float32)}
    out, plan = ar.augment_ref(x, norm, 9)
    K = 1
    drop = plan[:, K + 1]
    assert set(drop.tolist()) == {-1, 0, 1}
    off1 = K + 2 + 2 * (norm["n_t"] + norm["n_f"])
    assert np.all(plan[:, off1:off1 + 2] == 0)            # (the stream that uses no time mask leaves its slot empty)
    for b in range(B):
        if drop[b] == 1:
            assert np.all(out["s1"][b] == -1.5)
        fs, fw = plan[b, off1 + 2], plan[b, off1 + 3]
        assert np.all(out["s1"][b][:, fs:fs + fw] == -1.5)
        st, w = plan[b, K + 2], plan[b, K + 3]
        assert np.all(out["s0"][b, st:st + w] == 0.0)
        if drop[b] == 0:
            assert np.all(out["s0"][b] == 0.0)
        assert set(np.unique(out["s0"][b]).tolist()) <= {0.0, 1.0} and set(np.unique(out["s1"][b]).tolist()) <= {-1.5, 1.0}


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_normalize_config_defaults_are_off():
    norm = augment.normalize_config(None, _streams(7, 4), 23)
    assert norm["segments"] == 1 and norm["max_shift"] == 0 and norm["drop_thresh"] == 0 and norm["n_t"] == 0 and norm["n_f"] == 0
    assert [s["name"] for s in norm["streams"]] == ["s0", "s1"]
    spec, B, T, Lmax = configs.baseline_config("F")
    norm = augment.normalize_config(dict(segments=16, max_shift=20, stream_drop=0.25), spec, T)
    assert norm["drop_thresh"] == 1 << 22 and [s["F"] for s in norm["streams"]] == [39, 20]


@pytest.mark.parametrize("cfg, key", [
    (dict(warp=2), "warp"),
    (dict(segments=17), "segments"),
    (dict(segments=0), "segments"),
    (dict(segments=3, max_shift=4), "max_shift"),          # T 23: a_j = 0, 7, 14, 22 - the shortest segment is 7 frames, 2 D = 8
    (dict(segments=2, max_shift=-1), "max_shift"),
    (dict(time_masks=1, time_width=24), "time_width"),
    (dict(feature_masks=1, feature_width=5), "feature_width"),     # wider than the second stream's F = 4
    (dict(streams={"s1": dict(feature_width=5)}), "feature_width"),
    (dict(time_masks=9), "time_masks"),
    (dict(stream_drop=1.0), "stream_drop"),
    (dict(stream_drop=-0.1), "stream_drop"),
    (dict(streams={"nobody": {}}), "nobody"),
    (dict(streams={"s0": dict(segments=2)}), "segments"),
])
def test_normalize_config_refuses(cfg, key):
    with pytest.raises(ValueError, match=key):
        augment.normalize_config(cfg, _streams(7, 4), 23)


def test_normalize_config_accepts_the_edges_of_the_refusals():
    augment.normalize_config(dict(segments=3, max_shift=3, time_masks=8, time_width=23, feature_masks=1, feature_width=4,
                                  stream_drop=0.999), _streams(7, 4), 23)
    augment.normalize_config(dict(segments=16), _streams(7), 17)


def test_stream_drop_needs_two_streams_and_a_cnn_front_end_is_refused():
    with pytest.raises(ValueError, match="stream_drop"):
        augment.normalize_config(dict(stream_drop=0.5), _streams(7), 23)
    with pytest.raises(NotImplementedError, match="front-end"):
        augment.normalize_config(dict(time_masks=1, time_width=2), configs.rgb_spec(), 23)
    with pytest.raises(NotImplementedError, match="front-end"):
        augment.normalize_config({}, [dict(name="the_input", F=64, frontend=dict(layers=[]))], 23)
