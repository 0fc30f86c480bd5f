"""-m gpu: mgr_ctc_sample_paths (K16) - hypothesis sets by sampling alignments - `==` on all five outputs against the numpy
restatement (tests/sample_ref.py) at the smallest shapes where each stage can go wrong: the chunk and wave edges of the draw kernel,
every class count's row stride, one to 32 draws, merges with and without duplicates; the device output fed to mgr_ctc_rescore; the host
API down to predict_stream."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rescore_cases as rc  # noqa: E402
import rescore_ref as rr  # noqa: E402
import sample_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-8
NAMES = ("out", "out_len", "count", "n_unique", "path")


def _sample(device, P, il, skip, blank, eps, seed, K, want_path=True, keep=False):
    """mgr_ctc_sample_paths through the C ABI -> the five host arrays (path None if not asked for)[, the device arrays, to be freed]."""
    P = np.ascontiguousarray(P, np.float32)
    B, T, Cn = P.shape
    To = T - skip
    il = np.full(B, To, np.int32) if il is None else np.asarray(il, np.int32)
    ins = [device.array(P), device.array(il)]
    outs = [device.empty((B, K, To), np.int32), device.empty((B, K), np.int32), device.empty((B, K), np.int32), device.empty((B,), np.int32),
            device.empty((B, K, To), np.int32) if want_path else None]
    try:
        device.call("mgr_ctc_sample_paths", ins[0], ins[1], B, T, Cn, skip, blank, C.c_float(eps), C.c_uint64(seed), K, *outs)
        host = tuple(None if o is None else o.download() for o in outs)
    except Exception:
        keep = False
        raise
    finally:
        for a in ins + ([] if keep else [o for o in outs if o is not None]):
            a.free()
    return (host, outs) if keep else host


def _posteriors(kind, B, T, Cn, seed, scale=40.0):
    rng = np.random.default_rng(seed)
    if kind == "flat":
        P = rng.random((B, T, Cn)) + 0.5
    else:                                   # peaked: logits scaled, as the step tests scale dense/W
        z = rng.standard_normal((B, T, Cn)) * scale
        P = np.exp(z - z.max(axis=2, keepdims=True))
    return (P / P.sum(axis=2, keepdims=True)).astype(np.float32)


def _check(device, P, il, skip, blank, eps, seed, K, where=None):
    got = _sample(device, P, il, skip, blank, eps, seed, K)
    want = sr.sample_paths(P, il, skip, blank, eps, seed, K)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, where)
    return want


@pytest.mark.parametrize("To", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_frame_counts_through_T(device, To):
    """T - skip at the wave (64), chunk (128) and merge-stride (256) edges, a clipped input_len and a shorter neighbour in the batch."""
    skip, Cn, K = 2, 22, 8
    for kind in ("flat", "peaked"):
        P = _posteriors(kind, 3, To + skip, Cn, 100 + To)
        _check(device, P, [To, To + 9, To // 2], skip, Cn - 1, EPS, 7 + To, K, kind)


def test_frame_counts_through_input_len(device):
    lens = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025, 5000, -3]
    skip, Cn = 2, 22
    P = _posteriors("peaked", len(lens), 1027 + skip, Cn, 3, scale=6.0)
    out, out_len, count, nu, path = _check(device, P, lens, skip, Cn - 1, EPS, 99, 2)
    assert nu[0] == 1 and out_len[0, 0] == 0 and count[0, 0] == 2 and nu[11] == 1         # Tp = 0: the empty labelling, all draws
    assert (path[10] >= 0).all() and (path[9, :, 1025:] == -1).all()                      # clipped to T - skip; -1 from Tp on


@pytest.mark.parametrize("skip", [0, 2])
@pytest.mark.parametrize("Cn", [2, 22, 44, 64])
def test_shape_parameters(device, skip, Cn):
    T = 70
    for K in (1, 2, 8, 32):
        for B in (1, 3):
            for blank in (Cn - 1, 0):
                P = _posteriors("peaked" if K > 2 else "flat", B, T, Cn, K * 10 + B, scale=60.0)
                _check(device, P, None if B == 1 else [T - skip, 40, 66], skip, blank, EPS, 1000 * K + B, K, (K, B, blank))


def test_full_length(device):
    B, T, Cn, K, skip = 2, 1900, 22, 8, 2
    P = np.concatenate([_posteriors("flat", 1, T, Cn, 1), _posteriors("peaked", 1, T, Cn, 2, scale=30.0)])
    out, out_len, count, nu, _ = _check(device, P, [T - skip, 1500], skip, Cn - 1, EPS, 2026, K)
    assert nu[0] == K and out_len[0].min() > 1000          # flat: every draw unique, long labellings


def test_flat_draws_are_unique_and_peaked_draws_merge(device):
    skip, Cn, K, T = 2, 22, 32, 26
    flat = _check(device, _posteriors("flat", 3, T, Cn, 5), None, skip, Cn - 1, EPS, 1, K)
    assert (flat[3] == K).all() and (flat[2] == 1).all()
    peaked = _check(device, _posteriors("peaked", 3, T, Cn, 6, scale=48.0), None, skip, Cn - 1, EPS, 1, K)
    assert (peaked[3] < K).all() and (peaked[3] > 1).all() and peaked[2].max() > 2 and (peaked[2].sum(axis=1) == K).all()


@pytest.mark.parametrize("blank", [21, 0])
def test_exact_zeros_and_all_zero_rows(device, blank):
    skip, Cn, K, T = 2, 22, 8, 40
    P = _posteriors("flat", 2, T, Cn, 8)
    P[:, :, [0, 7, 21]] = 0.0             # first, middle, last class: never drawn with eps = 0
    P[0, 10] = 0.0                        # an all-zero row: S = 0, the blank
    P[1, skip] = 0.0
    path = _check(device, P, None, skip, blank, 0.0, 4, K)[4]
    drawn = np.delete(path[0], 10 - skip, axis=1)
    assert not np.isin(drawn, [0, 7, 21]).any() and (path[0][:, 10 - skip] == blank).all() and (path[1][:, 0] == blank).all()


def test_path_is_optional_seeds_differ_and_repeat(device):
    skip, Cn, K = 2, 22, 8
    P = _posteriors("peaked", 3, 130, Cn, 12, scale=8.0)
    il = [128, 64, 100]
    a = _sample(device, P, il, skip, Cn - 1, EPS, 5, K)
    b = _sample(device, P, il, skip, Cn - 1, EPS, 5, K, want_path=False)
    assert b[4] is None and all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))
    again = _sample(device, P, il, skip, Cn - 1, EPS, 5, K)
    assert all(np.array_equal(x, y) for x, y in zip(a, again))
    other = _sample(device, P, il, skip, Cn - 1, EPS, 6, K)
    assert not np.array_equal(a[4], other[4])
    big = _check(device, P, il, skip, Cn - 1, EPS, 2 ** 64 - 1, K)          # the seed is 64 bits wide
    assert not np.array_equal(a[4], big[4])


def test_a_sample_does_not_depend_on_its_neighbours(device):
    skip, Cn, K, T = 2, 22, 8, 90
    P = _posteriors("peaked", 3, T, Cn, 20, scale=8.0)
    il = np.array([88, 70, 33], np.int32)
    base = _check(device, P, il, skip, Cn - 1, EPS, 17, K)
    Q = P.copy()
    Q[0], Q[2] = _posteriors("flat", 2, T, Cn, 21)
    other = _sample(device, Q, [5, 70, 88], skip, Cn - 1, EPS, 17, K)
    for name, x, y in zip(NAMES, base, other):
        assert np.array_equal(x[1], y[1]), name          # row 1 of (b = 1, K, T): the same whatever stands beside it


def test_bad_arguments_are_refused(device):
    from mgr_amd import decoding
    from mgr_amd._capi import MgrError
    P = _posteriors("flat", 1, 10, 22, 0)
    for K in (0, 33):
        with pytest.raises(MgrError):
            _sample(device, P, None, 2, 21, EPS, 1, K)
        with pytest.raises(ValueError):
            decoding.sample_hypotheses(P, draws=K, dev=device)
    with pytest.raises(MgrError):
        _sample(device, np.full((1, 8, 65), 1 / 65, np.float32), None, 2, 64, EPS, 1, 4)
    with pytest.raises(MgrError):
        _sample(device, P, None, 2, 22, EPS, 1, 4)           # blank outside the classes


def test_the_device_output_feeds_mgr_ctc_rescore(device):
    """out / out_len as the kernel left them on the device, absent slots included, into K14: the scores of the restatement's lists."""
    skip, Cn, K, T = 2, 22, 8, 30
    P = _posteriors("peaked", 3, T, Cn, 30)
    il = np.array([28, 20, 0], np.int32)
    host, outs = _sample(device, P, il, skip, Cn - 1, EPS, 3, K, keep=True)
    want = sr.sample_paths(P, il, skip, Cn - 1, EPS, 3, K)
    assert (want[3] < K).any() and (want[3] > 1).any()          # (absent slots and several live ones)
    dP, dil = device.array(P), device.array(il)
    dlogp = device.empty((3, K), np.float64)
    ws = device.bytes(device.lib.mgr_ctc_rescore_ws_bytes(3, T, Cn, 0, None))
    try:
        device.call("mgr_ctc_rescore", dP, dil, 3, T, Cn, skip, Cn - 1, C.c_float(EPS), None, None, 0, outs[0], outs[1], K, T - skip, dlogp,
                    None, ws, ws.nbytes)
        logp = dlogp.download()
    finally:
        for a in [dP, dil, dlogp, ws] + outs:
            a.free()
    ref, _ = rr.score_batch(P, want[0], want[1], Cn - 1, skip, EPS, il)
    assert np.array_equal(logp == -np.inf, ref == -np.inf) and np.array_equal(ref == -np.inf, want[1] < 0)
    fin = np.isfinite(ref)
    gap = np.abs(logp[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1e-300)
    print("sampled sets into mgr_ctc_rescore: %d scores, largest gap %.3e" % (fin.sum(), gap.max()))
    assert gap.max() <= rc.REL == 1e-4


def test_host_api(device):
    from mgr_amd import decoding
    from mgr_amd.multimodal_fusion import sequence_decoding as sd
    skip, Cn, T = 2, 22, 40
    P = _posteriors("peaked", 3, T, Cn, 40)
    il = [38, 25, 10]
    want = sr.sample_paths(P, il, skip, Cn - 1, EPS, 77, 16)
    paths, counts = sr.lists(*want[:3])
    got = decoding.sample_hypotheses(P, draws=16, seed=77, input_length=il, dev=device)
    assert got == (paths, counts) and all(sum(c) == 16 for c in counts)
    got3 = decoding.sample_hypotheses(P, draws=16, seed=77, input_length=il, dev=device, return_path=True)
    assert got3[:2] == (paths, counts) and np.array_equal(got3[2], want[4])
    # the lists go where the beam search's go
    logp = decoding.ctc_scores(P, paths, input_length=il, dev=device)
    assert all(np.isfinite(logp[b, :len(paths[b])]).all() for b in range(3))
    full = sr.sample_paths(P, None, skip, Cn - 1, EPS, 5, 8)
    decoding._DEV[0] = device
    names, cnt = sd.decode_samples(P, [1, 2, 3], draws=8, seed=5)
    fp, fc = sr.lists(*full[:3])
    assert names == [[[sd.map_gest[i] for i in h] for h in hyps] for hyps in fp] and cnt == fc
    assert sd.decode_samples((fp, fc), [1, 2, 3])[0] == names


def test_predict_stream_draws_per_batch(device):
    """output="sample" piped over 3 batches equals three single-batch streams with sample_seed + i, and the restatement on the
    posteriors - on an inference-only engine and on a training engine."""
    from mgr_amd.configs import fusion_spec
    from mgr_amd.engine import Engine
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    spec = fusion_spec(h_audio=8, h_skeletal=8, h_fusion=4)
    B, T, skip, Cn = 2, 24, int(spec.ctc["skip"]), spec.num_classes
    w = synthetic_weights(spec, 3)
    w["dense/W"] = w["dense/W"] * 40.0
    data = [synthetic_arrays(spec, B, T, 4, 50 + i, lmin=2, lmax=4)[0] for i in range(3)]
    for inference_only in (True, False):
        eng = Engine(spec, B, T, 4, device=device, seed=5, inference_only=inference_only)
        try:
            eng.set_weights(w)
            P = list(eng.predict_stream(iter(data)))
            piped = list(eng.predict_stream(iter(data), output="sample", draws=8, sample_seed=2 ** 64 - 2))
            for i in range(3):
                seed = (2 ** 64 - 2 + i) % 2 ** 64
                single = list(eng.predict_stream([data[i]], output="sample", draws=8, sample_seed=seed))[0]
                want = sr.lists(*sr.sample_paths(P[i], None, skip, Cn - 1, float(spec.ctc["eps"]), seed, 8)[:3])
                assert piped[i] == single == want, (inference_only, i)
            assert piped[0] != list(eng.predict_stream([data[0]], output="sample", draws=8, sample_seed=0))[0]
            assert np.array_equal(P[0], list(eng.predict_stream([data[0]]))[0])          # the other outputs are as they were
        finally:
            eng.close()
