"""-m gpu: mgr_ctc_joint_decode (K19) - the label-synchronous prefix search over several CTC streams - against the fp64 restatement of
tests/joint_ref.py on the cases of tests/joint_cases.py (tests/test_cpu_joint.py has shown their decision margins, so sequences and
round counts are asked to be EQUAL on every sample), against mgr_ctc_rescore on the returned hypotheses, on the planted case that
re-ranking a pool cannot solve, on arguments it has to refuse, and through decoding.joint_decode / rescoring.decode_joint."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_cases as jc  # noqa: E402
import joint_ref as jr  # noqa: E402

pytestmark = pytest.mark.gpu

NEG = float("-inf")
_want = {}


def want(case):
    """The restatement's arrays of a case, computed once."""
    if case["name"] not in _want:
        _want[case["name"]] = jr.decode_case(case)
    return _want[case["name"]]


def _raw(device, case, rows=None, ws_short=0, with_rounds=True):
    """mgr_ctc_joint_decode through the C ABI on a case (rows: a subset of its samples).  The outputs are pre-filled, so that a
    refused call can be shown to have written nothing: returns (out, out_len, score, logp, rounds, ws_bytes), and on MgrError
    raises it with the downloaded outputs attached as .outputs."""
    from mgr_amd import _capi, decoding
    M, G, W, NP, L = len(case["streams"]), case["G"], case["beam"], case["top_paths"], case["max_len"]
    own, descs, alive = [], [], []

    def keep(a):
        own.append(a)
        return a
    try:
        for s in case["streams"]:
            P = s["P"] if rows is None else np.ascontiguousarray(s["P"][rows])
            B, T, Cn = P.shape
            il = np.full(B, T - s["skip"], np.int32) if s["il"] is None else (s["il"] if rows is None else s["il"][rows]).astype(np.int32)
            off = words = None
            if s["lexicon"] is not None:
                off, words = decoding.compile_lexicon(s["lexicon"], Cn, s["blank"])
                alive += [off, words]
            descs.append(dict(T=T, C=Cn, skip=s["skip"], blank=s["blank"], eps=s["eps"], weight=s["weight"], P=keep(device.array(P)),
                              input_len=keep(device.array(il)), phrase_off=off, phrase_words=words))
        arr = _capi.make_joint_streams(descs)
        ext = np.zeros((G + 1, G)) if case["ext"] is None else np.asarray(case["ext"], np.float64)
        dext = keep(device.array(ext))
        dfin = None if case["fin"] is None else keep(device.array(np.asarray(case["fin"], np.float64)))
        fill = [np.full((B, NP, L), -7, np.int32), np.full((B, NP), -7, np.int32), np.full((B, NP), 123.0), np.full((B, NP, M), 123.0),
                np.full((B,), -7, np.int32)]
        outs = [keep(device.array(a)) for a in fill]
        nbytes = device.lib.mgr_ctc_joint_ws_bytes(B, M, arr, G, W, NP, L)
        ws = keep(device.bytes(max(nbytes - ws_short, 16)))
        try:
            device.call("mgr_ctc_joint_decode", B, M, arr, G, dext, dfin, W, NP, L, outs[0], outs[1], outs[2], outs[3],
                        outs[4] if with_rounds else None, ws, ws.nbytes)
        except _capi.MgrError as e:
            e.outputs, e.fill = [o.download() for o in outs], fill
            raise
        return tuple(o.download() for o in outs) + (nbytes,)
    finally:
        for a in own:
            a.free()


def rel_gap(got, want_):
    """-inf where -inf; the largest relative gap over the finite entries."""
    got, want_ = np.asarray(got, np.float64), np.asarray(want_, np.float64)
    assert got.shape == want_.shape and not np.isnan(got).any()
    assert np.array_equal(got == NEG, want_ == NEG), (got, want_)
    fin = np.isfinite(want_)
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - want_[fin]) / np.maximum(np.abs(want_[fin]), 1e-300)))


def check_equal(case, got, rel, rows=None):
    out, out_len, score, logp, rounds = got[:5]
    w = [a if rows is None else a[rows] for a in want(case)[:5]]
    assert np.array_equal(out_len, w[1]), (case["name"], out_len, w[1])
    assert np.array_equal(out, w[0]), (case["name"], out, w[0])
    assert np.array_equal(rounds, w[4]), (case["name"], rounds, w[4])
    gs, gl = rel_gap(score, w[2]), rel_gap(logp, w[3])
    print("joint parity: %-16s %3d finite scores   largest gap to the fp64 restatement: score %.3e  logp %.3e" %
          (case["name"], int(np.isfinite(w[2]).sum()), gs, gl))
    assert gs <= rel and gl <= rel, (case["name"], gs, gl)


@pytest.mark.parametrize("case", jc.shape_cases(), ids=lambda c: c["name"])
def test_equals_the_restatement(device, case):
    """out, out_len and rounds ==, score and logp within 1e-12 relative, on every sample of every shape case."""
    got = _raw(device, case)
    check_equal(case, got, jc.REL)
    B = got[0].shape[0]
    if case["name"] == "m1_ragged":             # Tp = 0: the empty hypothesis alone, ln p = 0; and a row does not depend on the batch
        assert got[1][1].tolist() == [0, -1, -1] and got[2][1, 0] == 0.0 and got[4][1] == 1
        for b in range(B):
            one = _raw(device, case, rows=[b])
            for a, c in zip(one[:5], got[:5]):
                assert np.array_equal(a[0], c[b])
        assert all(np.array_equal(a, c) for a, c in zip(_raw(device, case, with_rounds=False)[:4], got[:4]))
    if case["name"] == "nothing_finite":
        assert (got[1] == -1).all() and (got[0] == -1).all() and (got[2] == NEG).all() and (got[3] == NEG).all()
    if case["name"] == "one_frame":
        assert (got[1][0] >= 0).sum() == 4       # fewer survivors than top_paths


def test_tie_rule(device):
    """Duplicated class columns: two candidates are the same operations on the same numbers, and the smaller gesture wins - on the
    device as in the restatement."""
    case = jc.tie_case()
    got = _raw(device, case)
    check_equal(case, got, jc.REL)
    score, out_len = got[2], got[1]
    assert any(score[b, k] == score[b, k + 1] for b in range(score.shape[0]) for k in range(score.shape[1] - 1) if out_len[b, k + 1] >= 0)


def _rescore(device, s, hyp, hyp_len):
    """mgr_ctc_rescore of one stream on hypothesis arrays."""
    import ctypes as C
    from mgr_amd import decoding
    P = s["P"]
    B, T, Cn = P.shape
    off = words = None
    G = 0
    if s["lexicon"] is not None:
        off, words = decoding.compile_lexicon(s["lexicon"], Cn, s["blank"])
        G = len(off) - 1
    host = lambda a: None if a is None else a.ctypes.data
    il = np.full(B, T - s["skip"], np.int32) if s["il"] is None else s["il"].astype(np.int32)
    own = [device.array(P), device.array(il), device.array(hyp), device.array(hyp_len), device.empty(hyp_len.shape, np.float64)]
    own.append(device.bytes(device.lib.mgr_ctc_rescore_ws_bytes(B, T, Cn, G, host(off))))
    try:
        device.call("mgr_ctc_rescore", own[0], own[1], B, T, Cn, s["skip"], s["blank"], C.c_float(s["eps"]), host(off), host(words), G, own[2],
                    own[3], hyp.shape[1], hyp.shape[2], own[4], None, own[5], own[5].nbytes)
        return own[4].download()
    finally:
        for a in own:
            a.free()


@pytest.mark.parametrize("name", ["m2_lexicon", "m3_tables", "gestures21"])
def test_against_the_shipped_kernels(device, name):
    """logp[..., m] is mgr_ctc_rescore's logp of the returned hypotheses (f32 recursion: REL_SHIPPED), with and without a lexicon;
    score is logp . w plus the table terms, recomputed on the host, to 1e-12."""
    case = [c for c in jc.shape_cases() if c["name"] == name][0]
    out, out_len, score, logp = _raw(device, case)[:4]
    assert (out_len >= 0).sum() >= out_len.shape[0]
    gap = 0.0
    for m, s in enumerate(case["streams"]):
        ref = _rescore(device, s, out, out_len)
        g = rel_gap(logp[:, :, m], ref)
        gap = max(gap, g)
        assert g <= jc.REL_SHIPPED, (name, m, g)
    print("joint parity: %-16s against mgr_ctc_rescore, largest gap %.3e" % (name, gap))
    w = np.array([s["weight"] for s in case["streams"]])
    for b in range(out.shape[0]):
        for k in range(out.shape[1]):
            if out_len[b, k] >= 0:
                t = float(np.dot(w, logp[b, k])) + jr.table_terms([int(g) for g in out[b, k, :out_len[b, k]]], case["G"], case["ext"], case["fin"])
                assert abs(score[b, k] - t) <= 1e-12 * abs(t), (b, k, score[b, k], t)


def test_long_chain(device):
    """B = 2, T = 1900 on both streams, C = 22 / 44 through the reference's lexicon, ten planted gestures, beam 10, top_paths 4:
    sequences ==, scores within 1e-9 relative (at most 3 x 1900 x 40 rounded fp64 operations per score at about 1e-15 relative each:
    2.3e-10 in the worst case)."""
    case = jc.long_case()
    got = _raw(device, case)
    print("joint: long chain workspace %d bytes, rounds %s" % (got[5], got[4].tolist()))
    check_equal(case, got, jc.REL_LONG)
    assert [list(got[0][b, 0, :got[1][b, 0]]) for b in range(2)] == case["truth"]


def test_pool_miss(device, tmp_path):
    """Three gestures; the skeletal stream prefers a wrong third one, the audio stream a wrong first one.  decode_rescoring's pool at
    top_paths = 2 does not hold the truth (tests/test_cpu_joint.py shows it on the restatements), so it returns a wrong sequence;
    the joint decode with equal weights returns the truth."""
    from mgr_amd import decoding
    from mgr_amd.multimodal_fusion import rescoring
    from mgr_amd.multimodal_fusion.sequence_decoding import map_gest
    decoding._DEV[0] = device
    case = jc.pool_miss_case()
    sk, au = case["streams"][0]["P"], case["streams"][1]["P"]
    names, (ranked, total, _) = rescoring.decode_rescoring(sk, au, [1], top_paths=2, beam_width=10, out_file=None)
    assert case["truth"] not in ranked[0] and ranked[0][0] in (case["sk_wrong"], case["sk_wrong2"], case["au_wrong"])
    jnames, (jranked, jtotal, _) = rescoring.decode_joint(sk, au, [1], top_paths=2, beam_width=10, out_file=str(tmp_path / "j.mlf"))
    assert jranked[0][0] == case["truth"] and jnames == [[map_gest[g] for g in case["truth"]]]
    assert decoding.read_mlf(str(tmp_path / "j.mlf")) == {"Sample00001": jnames[0]}
    rescoring.decode_joint(sk, au, [228], out_file=str(tmp_path / "i.mlf"))          # a file number of the ignore list is left out
    assert decoding.read_mlf(str(tmp_path / "i.mlf")) == {}
    assert jtotal[0, 0] > total[0, 0]
    check_equal(case, _raw(device, case), jc.REL)


def test_errors_are_refused_and_nothing_is_written(device):
    from mgr_amd._capi import MgrError
    rng = np.random.default_rng(5)
    P = jc.dirichlet(rng, 2, 12, 6)
    good = jc.case("good", [jc.stream(P), jc.stream(P, jc.SMALL_LEXICON)], 5, 4, 2, 4)
    assert (_raw(device, good)[1][:, 0] >= 0).all()
    nine = [[0, 1, 0, 1, 0, 1, 0, 1, 0]] + jc.SMALL_LEXICON[1:]
    bad = [(jc.case("long_phrase", [jc.stream(P), jc.stream(P, nine)], 5, 4, 2, 4), "words"),
           (jc.case("g_above_c", [jc.stream(P)], 7, 4, 2, 4), "without a lexicon"),
           (jc.case("top_above_beam", good["streams"], 5, 4, 5, 4), "top_paths"),
           (jc.case("zero_weight", [jc.stream(P), jc.stream(P, jc.SMALL_LEXICON, weight=0.0)], 5, 4, 2, 4), "weight"),
           (jc.case("negative_weight", [jc.stream(P, weight=-1.0)], 5, 4, 2, 4), "weight")]
    for case, msg in bad:
        with pytest.raises(MgrError, match=msg) as e:
            _raw(device, case)
        assert all(np.array_equal(a, f) for a, f in zip(e.value.outputs, e.value.fill)), case["name"]
    with pytest.raises(MgrError, match="workspace too small") as e:
        _raw(device, good, ws_short=256)
    assert all(np.array_equal(a, f) for a, f in zip(e.value.outputs, e.value.fill))


def test_facade(device):
    """decoding.joint_decode returns what the raw call returns - from host arrays and from DeviceArrays -, and its output feeds
    ctc_scores and mbr_decode without conversion."""
    from mgr_amd import decoding
    decoding._DEV[0] = device
    case = [c for c in jc.shape_cases() if c["name"] == "gestures21"][0]
    out, out_len, score, logp, rounds = _raw(device, case)[:5]
    streams = [(s["P"], {"lexicon": s["lexicon"]}) for s in case["streams"]]
    paths, total, parts, r = decoding.joint_decode(streams, beam_width=case["beam"], top_paths=case["top_paths"], max_len=case["max_len"],
                                                   dev=device, return_rounds=True)
    assert paths == decoding.joint_from_arrays(out, out_len, score, logp)[0]
    assert np.array_equal(total, score) and np.array_equal(parts, logp) and np.array_equal(r, rounds)
    dP = [device.array(s["P"]) for s in case["streams"]]
    again = decoding.joint_decode([(dP[0], None), (dP[1], {"lexicon": case["streams"][1]["lexicon"]})], G=21, beam_width=case["beam"],
                                  top_paths=case["top_paths"], max_len=case["max_len"], dev=device)
    for a in dP:
        a.free()
    assert again[0] == paths and np.array_equal(again[1], total)
    # the shapes the N-best consumers take
    sk = decoding.ctc_scores(case["streams"][0]["P"], paths, dev=device)
    fin = np.isfinite(total)
    assert sk.shape == total.shape and rel_gap(sk[fin], parts[:, :, 0][fin]) <= jc.REL_SHIPPED
    picks, ranks, _ = decoding.mbr_decode(paths, total, dev=device)
    assert len(picks) == len(paths) and np.all(ranks >= 0)
    dist, rank, _ = decoding.nbest_attainable(paths, [[3, 17, 8], [11, 11, 0]], dev=device)
    assert np.all(dist == 0) and np.all(rank == 0)
    with pytest.raises(ValueError):
        decoding.joint_decode(streams, weights=(1.0, 0.0), dev=device)
    with pytest.raises(ValueError):
        decoding.joint_decode(streams, beam_width=4, top_paths=5, dev=device)
