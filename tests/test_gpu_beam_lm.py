"""-m gpu: the beam search with a label bigram and an N-best list (mgr_ctc_beam_search_lm) against the plain entry point
(zero tables: bit for bit), the fp64 reference tests/beam_lm_ref.py, exhaustive enumeration, and through the facade.

Sequences are compared for equality only after the reference has shown that no decision of the search hangs on a score difference
below 1e-9 (its `gap`); scores to 1e-12 relative, the project's bound for the plain beam search."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as br  # noqa: E402
from test_cpu_beam_lm import TINY, check_tiny_inputs, tiny_case  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(4, 50, 22, 10), (2, 30, 44, 16), (3, 150, 5, 10), (3, 400, 3, 4)]     # (N, T, C, W); the last: prefixes re-enter the beam
AUDIO = (2, 120, 44, 10)


def posteriors(N, T, Cn, seed):
    """Posteriors between flat and peaky, ragged input lengths with one sample of length 0 (N >= 3) - computed once per shape."""
    rng = np.random.default_rng(seed)
    P = rng.dirichlet(0.3 * np.ones(Cn), size=(N, T)).astype(np.float32)
    il = np.array([T - 2] + [int(v) for v in rng.integers(T // 2, T - 2, N - 1)])
    if N >= 3:
        il[N - 1] = 0
    return P, il


def tables(Cn, seed, frac_inf):
    rng = np.random.default_rng(seed)
    ext = rng.standard_normal((Cn + 1, Cn))
    if frac_inf:
        ext[rng.random((Cn + 1, Cn)) < frac_inf] = -np.inf
    return ext, rng.standard_normal(Cn + 1)


_CASES = {}


def case(shape):
    if shape not in _CASES:
        _CASES[shape] = posteriors(shape[0], shape[1], shape[2], 1000 + shape[1])
    return _CASES[shape]


def run_nbest(device, P, il, ext, fin, W, NP, skip=2, eps=1e-8, blank=None):
    """The C call itself: the raw (out, out_len, score, logp_ctc) arrays.  blank: None = the last class."""
    N, T, Cn = P.shape
    blank = Cn - 1 if blank is None else blank
    arrs = [device.array(np.ascontiguousarray(P, np.float32)), device.array(np.asarray(il, np.int32)),
            device.array(np.ascontiguousarray(ext, np.float64))]
    dfin = None
    if fin is not None:
        arrs.append(device.array(np.ascontiguousarray(fin, np.float64)))
        dfin = arrs[-1]
    outs = [device.empty((N, NP, T - skip), np.int32), device.empty((N, NP), np.int32), device.empty((N, NP), np.float64),
            device.empty((N, NP), np.float64)]
    ws = device.bytes(device.lib.mgr_ctc_beam_lm_ws_bytes(N, T, Cn, W, NP))
    try:
        device.call("mgr_ctc_beam_search_lm", arrs[0], arrs[1], N, T, Cn, skip, blank, W, C.c_float(eps), arrs[2], dfin, NP, *outs, ws,
                    ws.nbytes)
        return [o.download() for o in outs]
    finally:
        for a in arrs + outs + [ws]:
            a.free()


def assert_matches_reference(got, ref, NP, To):
    out, olen, score, logp = got
    seqs, rscore, rlogp, gap = ref
    assert gap > 1e-9, gap
    for b in range(len(seqs)):
        n = len(seqs[b])
        assert olen[b].tolist() == [len(s) for s in seqs[b]] + [-1] * (NP - n)
        for k in range(NP):
            want = seqs[b][k] if k < n else []
            assert out[b, k].tolist() == want + [-1] * (To - len(want))
        assert np.allclose(score[b, :n], rscore[b], rtol=1e-12, atol=0) and np.allclose(logp[b, :n], rlogp[b], rtol=1e-12, atol=0)
        assert np.all(np.isneginf(score[b, n:])) and np.all(np.isneginf(logp[b, n:]))


@pytest.mark.parametrize("shape", SHAPES)
def test_zero_tables_equal_the_existing_beam_kernel_bit_for_bit(device, shape):
    """Zero tables against the plain entry point: the LM = true and LM = false instantiations of the one k_beam body."""
    from mgr_amd import decoding
    N, T, Cn, W = shape
    P, il = case(shape)
    assert (il == 0).sum() == (1 if N >= 3 else 0) and len(set(il.tolist())) > 1
    want, wsc = decoding.beam_search_decode(P, il, beam_width=W, merge_repeated=False, dev=device)
    for lm, lm_end in ((None, None), (np.zeros((Cn + 1, Cn)), np.zeros(Cn + 1))):
        paths, score, logp = decoding.beam_search_lm_decode(P, lm, lm_end, input_length=il, beam_width=W, dev=device)
        assert paths == want
        assert score.shape == (N,) and score.dtype == np.float64 and np.array_equal(score, wsc) and np.array_equal(logp, score)
    assert sum(len(p) for p in want) > 0
    for b in np.flatnonzero(il == 0):
        assert want[b] == [] and score[b] == 0.0


@pytest.mark.parametrize("frac_inf", [0.0, 0.2])
@pytest.mark.parametrize("shape", SHAPES + [AUDIO])
def test_random_tables_equal_the_reference(device, shape, frac_inf):
    N, T, Cn, W = shape
    P, il = case(shape)
    ext, fin = tables(Cn, 50 + Cn, frac_inf)
    for NP in sorted({1, 3, W}):
        ref = br.beam_search_lm(P, il, ext, fin, beam_width=W, top_paths=NP)
        got = run_nbest(device, P, il, ext, fin, W, NP)
        assert_matches_reference(got, ref, NP, T - 2)
        if frac_inf:
            banned = {(int(p) - 1, int(c)) for p, c in zip(*np.nonzero(np.isneginf(ext)))}
            assert not any((a, b) in banned for hyps in ref[0] for s in hyps for a, b in zip([-1] + s, s))
    # without fin the score is the network's part plus the ext bonuses of the path
    ref = br.beam_search_lm(P, il, ext, None, beam_width=W, top_paths=3)
    got = run_nbest(device, P, il, ext, None, W, 3)
    assert_matches_reference(got, ref, 3, T - 2)
    out, olen, score, logp = got
    for b in range(N):
        for k in range(3):
            if olen[b, k] >= 0:
                s = out[b, k, :olen[b, k]].tolist()
                bonus = sum(ext[p + 1, c] for p, c in zip([-1] + s, s))
                assert abs(score[b, k] - (logp[b, k] + bonus)) <= 1e-12 * abs(score[b, k]) + 1e-12


@pytest.mark.parametrize("frac_inf", [0.0, 0.2])
@pytest.mark.parametrize("shape", [(2, 30, 44, 32), (2, 24, 64, 20)])
def test_more_than_12_candidates_per_lane_equal_the_reference(device, shape, frac_inf):
    """beam * (C + 1) > 768: the 34-candidates-per-lane form with the bigram terms, the instantiation that spills the most to scratch.
    The posteriors of test_gpu_decode.py::test_beam_search_with_more_than_12_candidates_per_lane: 44 classes at the beam limit of 32,
    and the class limit of 64."""
    N, T, Cn, W = shape
    assert W * (Cn + 1) > 768
    rng = np.random.default_rng(N * 100 + Cn + W)
    P = rng.random((N, T, Cn)) ** 6
    P = (P / P.sum(-1, keepdims=True)).astype(np.float32)
    il = np.full(N, T - 2)
    il[0] = (T - 2) // 2
    ext, fin = tables(Cn, 50 + Cn, frac_inf)
    for NP in sorted({1, 3, W}):
        ref = br.beam_search_lm(P, il, ext, fin, beam_width=W, top_paths=NP)
        got = run_nbest(device, P, il, ext, fin, W, NP)
        assert_matches_reference(got, ref, NP, T - 2)


@pytest.mark.parametrize("frac_inf", [0.0, 0.2])
def test_merge_mask_bit_63_equal_the_reference(device, frac_inf):
    """64 classes with blank = 0 (the inputs of test_gpu_decode.py::test_beam_search_merge_mask_bit_63): class 63 is a label, and an
    extension by it that lands on a live beam sets bit 63 of the merge mask.  The table never bans an extension by 5 or 63, so 63
    stays reachable and occurs in what is returned."""
    N, T, Cn, W, skip, blank = 2, 24, 64, 20, 2, 0
    rng = np.random.default_rng(63)
    P = rng.random((N, T, Cn)) ** 6 * 1e-3
    P[:, :, [0, 5, 63]] = rng.random((N, T, 3)) + 0.2
    P = (P / P.sum(-1, keepdims=True)).astype(np.float32)
    il = np.array([T - skip, T - skip - 3])
    ext, fin = tables(Cn, 50 + Cn, frac_inf)
    for c in (5, 63):
        ext[np.isneginf(ext[:, c]), c] = 0.0
    for NP in sorted({1, 3, W}):
        ref = br.beam_search_lm(P, il, ext, fin, beam_width=W, top_paths=NP, skip=skip, blank=blank)
        assert any(63 in s for hyps in ref[0] for s in hyps)
        got = run_nbest(device, P, il, ext, fin, W, NP, skip=skip, blank=blank)
        assert_matches_reference(got, ref, NP, T - skip)
        assert any(63 in got[0][b, k, :got[1][b, k]].tolist() for b in range(N) for k in range(NP) if got[1][b, k] >= 0)


@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("Cn,Tp", TINY)
def test_equals_exhaustive_enumeration(device, Cn, Tp, with_inf):
    """A beam of 32 holds every prefix before the last frame of these shapes: the kernel must return the truly best labellings."""
    P, ext, fin = tiny_case(Cn, Tp, 100 * Cn + 10 * Tp, with_inf)
    ranked, pruned_order = br.enumerate_labellings(P, ext, fin)
    check_tiny_inputs(ranked, pruned_order)
    out, olen, score, logp = run_nbest(device, P[None], [Tp], ext, fin, 32, 8, skip=0, eps=0.0)
    n = min(8, len(ranked))
    assert [tuple(out[0, k, :olen[0, k]].tolist()) for k in range(n)] == [e[0] for e in ranked[:n]]
    assert np.allclose(score[0, :n], [e[1] for e in ranked[:n]], rtol=1e-12, atol=0)
    assert np.allclose(logp[0, :n], [e[2] for e in ranked[:n]], rtol=1e-12, atol=0)


def spikes():
    """T = 42, C = 6 (blank 5): a blank floor, spikes of label 0 at t = 8, label 1 at t = 20, label 2 at t = 32; label 3 sits 0.1 logit
    below label 1 at t = 20."""
    z = np.zeros((1, 42, 6))
    z[:, :, 5] = 6.0
    z[0, 8, 0] = z[0, 20, 1] = z[0, 32, 2] = 12.0
    z[0, 20, 3] = 11.9
    P = np.exp(z - z.max(-1, keepdims=True))
    return (P / P.sum(-1, keepdims=True)).astype(np.float32)


def test_the_bonus_does_what_it_says(device):
    from mgr_amd import decoding
    P = spikes()
    nbest = lambda **kw: decoding.beam_search_lm_decode(P, beam_width=10, top_paths=4, dev=device, **kw)
    paths, score, logp = nbest()
    assert paths[0][:2] == [[0, 1, 2], [0, 3, 2]] and np.array_equal(score, logp) and score[0, 0] > score[0, 1]
    lm = np.zeros((7, 6))
    lm[0 + 1, 1], lm[0 + 1, 3] = -2.0, -0.1
    p2, s2, l2 = nbest(lm=lm)
    assert p2[0][:2] == [[0, 3, 2], [0, 1, 2]]
    assert np.isclose(s2[0, 0], l2[0, 0] - 0.1, rtol=1e-12) and np.isclose(s2[0, 1], l2[0, 1] - 2.0, rtol=1e-12)
    lm[0 + 1, 1] = -np.inf
    p3, s3, _ = nbest(lm=lm)
    assert len(p3[0]) == 4 and p3[0][0] == [0, 3, 2]
    assert not any((a, b) == (0, 1) for s in p3[0] for a, b in zip(s, s[1:]))
    # alpha scales the table: at alpha = 0.01 the bonuses are too small to swap the order
    p4, _, _ = nbest(lm=np.where(np.isneginf(lm), -2.0, lm), alpha=0.01)
    assert p4[0][:2] == [[0, 1, 2], [0, 3, 2]]
    # lm_end is added once at the end and takes no part in the pruning: every beam that survives the spike at t = 32 ends with label 2,
    # so a penalty on ending there lowers every score and changes nothing else - and a ban leaves no hypothesis at all
    lm_end = np.zeros(7)
    lm_end[2 + 1] = -5.0
    p5, s5, l5 = nbest(lm_end=lm_end)
    assert p5 == paths and np.array_equal(l5, logp) and np.array_equal(s5, logp + -5.0)
    lm_end[2 + 1] = -np.inf
    p6, s6, l6 = nbest(lm_end=lm_end)
    assert p6 == [[]] and np.all(np.isneginf(s6)) and np.all(np.isneginf(l6)) and s6.shape == (1, 4)
    # a larger bonus per label never shortens the 1-best
    rng = np.random.default_rng(3)
    Pn = rng.dirichlet(0.5 * np.ones(6), size=(3, 42)).astype(np.float32)
    prev = [0, 0, 0]
    for beta in (-2.0, -0.5, 0.0, 0.5, 2.0, 6.0):
        paths, _, _ = decoding.beam_search_lm_decode(Pn, beta=beta, beam_width=10, dev=device)
        lens = [len(p) for p in paths]
        assert all(a >= b for a, b in zip(lens, prev)), (beta, lens, prev)
        prev = lens
    assert prev[0] > 10


def test_independence_and_bounds(device):
    from mgr_amd import _capi, decoding
    shape = SHAPES[0]
    N, T, Cn, W = shape
    P, il = case(shape)
    ext, fin = tables(Cn, 9, 0.2)
    base = run_nbest(device, P, il, ext, fin, W, 3)
    perm = np.array([2, 0, 3, 1])
    for a, b in zip(base, run_nbest(device, P[perm], il[perm], ext, fin, W, 3)):
        assert np.array_equal(a[perm], b)
    # a sample alone, and beside other neighbours
    other = np.random.default_rng(1).dirichlet(np.ones(Cn), size=(2, T)).astype(np.float32)
    for a, b, c in zip(base, run_nbest(device, P[1:2], il[1:2], ext, fin, W, 3),
                       run_nbest(device, np.concatenate([other, P[1:2]]), [T - 2, 5, il[1]], ext, fin, W, 3)):
        assert np.array_equal(a[1], b[0]) and np.array_equal(a[1], c[2])
    # refusals
    with pytest.raises(_capi.MgrError, match="top_paths"):
        run_nbest(device, P, il, ext, fin, 4, 5)
    with pytest.raises(_capi.MgrError, match="top_paths"):
        run_nbest(device, P, il, ext, fin, 4, 0)
    with pytest.raises(_capi.MgrError, match="beam width"):
        run_nbest(device, P, il, ext, fin, 33, 1)
    P65 = np.full((1, 8, 65), 1 / 65, np.float32)
    with pytest.raises(_capi.MgrError, match="C <= 64"):
        run_nbest(device, P65, [6], np.zeros((66, 65)), None, 4, 1)
    bad = ext.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        decoding.beam_search_lm_decode(P, lm=bad, dev=device)
    badfin = fin.copy()
    badfin[0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        decoding.beam_search_lm_decode(P, lm=ext, lm_end=badfin, dev=device)
    with pytest.raises(ValueError, match="shape"):
        decoding.beam_search_lm_decode(P, lm=ext[:, :-1], dev=device)


def test_through_the_facade(device, tmp_path):
    """predict_generator(decode="beam_lm") equals beam_search_lm_decode of predict_generator()'s posteriors - pipelined and one batch
    per stream; decode_beam writes an MLF that read_mlf reads back to the 1-best names."""
    from mgr_amd import decoding, keras_like as K
    from mgr_amd.configs import fusion_spec
    from mgr_amd.keras_like import Model
    from mgr_amd.multimodal_fusion import sequence_decoding as sd
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    K.set_learning_phase(0)
    decoding._DEV[0] = device
    spec = fusion_spec()
    B, T, Cn = 2, 48, spec.num_classes
    data = [synthetic_arrays(spec, B, T, 4, 700 + i, lmin=2, lmax=4)[0] for i in range(3)]
    m = Model(spec, device=device)
    m.set_weights_dict(synthetic_weights(spec, 11))
    P = m.predict_generator(iter(data), steps=3)
    rng = np.random.default_rng(5)
    lm, lm_end = decoding.bigram_lm([list(rng.integers(0, Cn - 1, 6)) for _ in range(40)], Cn, add_k=0.5)
    kw = dict(lm=lm, lm_end=lm_end, alpha=0.7, beta=0.3, beam_width=8)
    eps = float(spec.ctc["eps"])
    assert eps == 1e-8          # (what beam_search_lm_decode passes)
    for NP in (1, 3):
        want = decoding.beam_search_lm_decode(P, top_paths=NP, dev=device, **kw)
        got = m.predict_generator(iter(data), steps=3, decode="beam_lm", top_paths=NP, **kw)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert got[1].shape == ((3 * B,) if NP == 1 else (3 * B, NP))
        # one batch per stream: nothing in flight beside it
        eng = m._engine
        single = [list(eng.predict_stream([d], output="beam_lm", top_paths=NP, **kw))[0] for d in data]
        assert [p for r in single for p in r[0]] == want[0]
        assert np.array_equal(np.concatenate([r[1] for r in single]), want[1])
        assert np.array_equal(np.concatenate([r[2] for r in single]), want[2])
    assert sum(len(h) for h in want[0]) == 3 * B * 3 and sum(len(s) for h in want[0] for s in h) > 0
    # the table changes something on these posteriors, and the plain beam mode still gives what it gave
    plain = decoding.beam_search_lm_decode(P, top_paths=3, beam_width=8, dev=device)
    assert not np.array_equal(plain[1], want[1])
    bm = m.predict_generator(iter(data), steps=3, decode="beam", beam_width=8)
    p1 = decoding.beam_search_decode(P, beam_width=8, dev=device)
    assert bm[0] == p1[0] and np.array_equal(bm[1], p1[1])
    with pytest.raises(ValueError, match="top_paths"):
        m.predict_generator(iter(data), steps=3, decode="beam_lm", top_paths=9, beam_width=8)
    # the module: 1-best names into the MLF, the N-best lists returned - from posteriors and from the device's result
    f_list = list(range(1, 3 * B + 1))
    names, nbest = sd.decode_beam(P, f_list, top_paths=3, out_file=str(tmp_path / "a.mlf"), **kw)
    names2, nbest2 = sd.decode_beam(got, f_list, out_file=str(tmp_path / "b.mlf"))
    assert names == names2 == [[sd.map_gest[i] for i in h[0]] for h in want[0]]
    assert nbest[0] == want[0] and np.array_equal(nbest[1], want[1]) and nbest2 is got
    assert open(tmp_path / "a.mlf").read() == open(tmp_path / "b.mlf").read()
    back = decoding.read_mlf(str(tmp_path / "a.mlf"))
    assert [back["Sample%05d" % f] for f in f_list] == names
