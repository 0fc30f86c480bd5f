"""The fp64 restatements of tests/align_ref.py against first principles, the segment restatement against the shipped host decode, and the
timed MLF (no GPU)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as ar  # noqa: E402

from mgr_amd import decoding  # noqa: E402


@pytest.mark.parametrize("labels", [[], [0], [2], [0, 1], [1, 1], [2, 0, 2], [1, 1, 1], [0, 0, 2], [2, 1, 0]])
@pytest.mark.parametrize("seed", [0, 1])
def test_viterbi_equals_exhaustive_enumeration(labels, seed):
    rng = np.random.default_rng(100 * seed + len(labels))
    T, Cn, blank = 6, 4, 3
    P = rng.dirichlet(np.full(Cn, 0.5), size=T).astype(np.float32)
    logy = ar.log_emissions(P, skip=0)
    score, states = ar.viterbi(logy, labels, blank)
    brute = ar.brute_force_best(logy, labels, blank)
    assert np.isfinite(brute)        # (the longest case, [1, 1, 1], needs 5 of the 6 frames)
    assert abs(score - brute) <= 1e-12 * max(1.0, abs(brute))
    path = ar.states_to_path(states, labels, blank)
    assert ar.collapse(path, blank) == labels
    assert abs(ar.path_score(logy, path) - score) <= 1e-12 * max(1.0, abs(score))
    assert np.all(np.diff(states) >= 0) and np.all(np.diff(states) <= 2)


def test_viterbi_infeasible_exactly():
    logy = ar.log_emissions(np.full((3, 4), 0.25, np.float32), skip=0)
    s, st = ar.viterbi(logy, [1, 1], 3)
    assert np.isfinite(s) and list(st) == [1, 2, 3]              # label, blank, label fits three frames exactly
    assert ar.viterbi(logy[:2], [1, 1], 3) == (-np.inf, None)    # ... and not two


def test_tie_rule_on_uniform_posteriors():
    """Every alignment has the same score.  A back-pointer tie takes the smallest step, so a state points at itself whenever it was
    reachable a frame earlier; the final tie takes the last blank.  Read forwards the path therefore climbs as early as reachability
    allows - state s is first reachable at frame ceil(s / 2) where every step of two is allowed, one frame later per forbidden one -
    and then waits in the last blank."""
    Cn, blank = 5, 4
    logy = ar.log_emissions(np.full((10, Cn), 1.0 / Cn, np.float32), skip=0)
    s, st = ar.viterbi(logy, [0, 1], blank)
    assert list(st) == [1, 3, 4, 4, 4, 4, 4, 4, 4, 4]      # label 0, straight over the blank onto label 1, the last blank
    assert abs(s - 10 * np.log(1.0 / Cn)) < 1e-12
    s, st = ar.viterbi(logy, [2, 2], blank)
    assert list(st) == [1, 2, 3, 4, 4, 4, 4, 4, 4, 4]      # a repeated label: the blank between cannot be stepped over
    s, st = ar.viterbi(logy, [], blank)
    assert list(st) == [0] * 10 and abs(s - 10 * np.log(1.0 / Cn)) < 1e-12
    s, st = ar.viterbi(logy[:3], [2, 2], blank)
    assert list(st) == [1, 2, 3]                           # the last blank is out of reach: the last label ends the path
    s, st = ar.viterbi(logy[:2], [0, 1], blank)
    assert list(st) == [1, 3]


def _filter_case(rng, T, Cn, thr):
    """Posteriors whose frame maxima lie on both sides of thr, in runs, with labels whose first occurrences get dropped."""
    P = np.zeros((T, Cn), np.float32)
    t = 0
    while t < T:
        n = int(rng.integers(1, 6))
        lab = int(rng.integers(0, Cn))
        for u in range(t, min(T, t + n)):
            hi = float(rng.uniform(max(thr - 0.3, 1.0 / Cn + 0.05), min(thr + 0.3, 0.999)))
            P[u] = (1.0 - hi) / (Cn - 1)
            P[u, lab] = hi
        t += n
    return P


@pytest.mark.parametrize("thr", [0.5, 0.75, 0.97, None])
def test_segment_restatement_gives_the_labels_of_the_host_decode(thr):
    rng = np.random.default_rng(7)
    dropped = empty = 0
    for case in range(40):
        T, Cn = int(rng.integers(3, 80)), int(rng.integers(3, 23))
        P = _filter_case(rng, T, Cn, 0.5 if thr is None else thr)
        if case % 8 == 0 and thr is not None:      # every frame below the threshold: nothing survives
            P = np.full((T, Cn), 1.0 / Cn, np.float32)
            P[:, 1] += 1e-3
        best, prob = P[2:].argmax(axis=1), P[2:].max(axis=1)
        want = decoding.confidence_filter_collapse(best, prob, thr)
        segs = ar.greedy_segments(P, thr, skip=2)
        assert [s[0] for s in segs] == want
        empty += not want
        for lab, f, l, cf in segs:
            assert 2 <= f <= l < T and best[f - 2] == lab and best[l - 2] == lab
            assert prob.min() - 1e-7 <= cf <= prob.max() + 1e-7
        assert all(a[2] < b[1] for a, b in zip(segs, segs[1:]))
        if thr is not None:
            dropped += int((prob < thr).sum()) > 0 and len(segs) > 0
    if thr is not None:
        assert dropped >= 10 and empty >= 3


def _write_pair(tmp_path, names, segs, f_list, ignore):
    a, b = str(tmp_path / "plain.mlf"), str(tmp_path / "timed.mlf")
    decoding.write_mlf(a, names, f_list, ignore, "Sample%05d")
    decoding.write_mlf(b, names, f_list, ignore, "Sample%05d", segments=segs)
    return a, b


def test_timed_mlf_round_trip_and_score(tmp_path):
    names = [["sil", "VA", "sil", "OK"], [], ["CP"], ["sil"]]
    segs = [[(21, 2, 9, .9), (1, 10, 10, .8), (21, 11, 40, .99), (11, 41, 45, .7)], [], [(5, 2, 2, .6)], [(21, 2, 50, 1.0)]]
    f_list, ignore = [1, 2, 3, 228], [228]
    plain, timed = _write_pair(tmp_path, names, segs, f_list, ignore)
    text = open(timed).read().split("\n")
    assert text[0] == "#!MLF!#" and text[1] == '"*/Sample00001.rec"'
    assert text[2] == "1000000 5000000 sil" and text[3] == "5000000 5500000 VA" and text[5] == "20500000 23000000 OK"
    assert decoding.read_mlf(timed) == decoding.read_mlf(plain) == {"Sample00001": names[0], "Sample00002": [], "Sample00003": ["CP"]}
    # a reference file the recognition differs from: the timed file scores exactly like its untimed twin
    ref = str(tmp_path / "ref.mlf")
    decoding.write_mlf(ref, [["VA", "OK", "CP"], ["FU"], ["CP"], []], f_list, ignore)
    assert decoding.score_mlf(ref, timed) == decoding.score_mlf(ref, plain)
    assert decoding.score_mlf(ref, timed)[1] == 3 and decoding.score_mlf(ref, timed)[0] > 0
    # another frame period
    decoding.write_mlf(timed, names, f_list, ignore, segments=segs, frame_period=100000)
    assert open(timed).read().split("\n")[3] == "1000000 1100000 VA"
    with pytest.raises(ValueError):
        decoding.write_mlf(timed, names, f_list, ignore, segments=[[], [], [], []])


def test_untimed_mlf_is_unchanged_byte_for_byte(tmp_path):
    names = [["sil", "VA", "sil"], ["oov"], []]
    p = str(tmp_path / "a.mlf")
    decoding.write_mlf(p, names, [17, 228, 5], [228], "Sample%05d_audio")
    assert open(p, "rb").read() == b'#!MLF!#\n"*/Sample00017_audio.rec"\nsil\nVA\nsil\n.\n"*/Sample00005_audio.rec"\n.\n'
    decoding.write_mlf(p, names, [17, 228, 5], [228], "Sample%05d_audio", segments=None)
    assert open(p, "rb").read() == b'#!MLF!#\n"*/Sample00017_audio.rec"\nsil\nVA\nsil\n.\n"*/Sample00005_audio.rec"\n.\n'


def test_pack_labels_accepts_padded_arrays_and_lists():
    lab, ll = decoding.pack_labels(np.array([[3, 4, -1, -1], [1, np.nan, np.nan, np.nan]]))
    assert lab.dtype == np.int32 and lab.tolist() == [[3, 4, -1, -1], [1, -1, -1, -1]] and ll.tolist() == [2, 1]
    lab, ll = decoding.pack_labels([[3, 4], [], [1, 2, 3]])
    assert lab.tolist() == [[3, 4, -1], [-1, -1, -1], [1, 2, 3]] and ll.tolist() == [2, 0, 3]
    lab, ll = decoding.pack_labels([[], []])
    assert lab.shape == (2, 1) and ll.tolist() == [0, 0]
    lab, ll = decoding.pack_labels(np.array([[3, 4, 5]]), label_length=[2])
    assert ll.tolist() == [2]


def test_decode_segments_of_every_module_writes_the_timed_mlf_from_given_segments(tmp_path):
    """Segments computed elsewhere (Model.predict_generator(decode="segments")) go through each module's own class map, ignore list and
    file-name pattern without touching the GPU."""
    from mgr_amd.audio_network import sequence_decoding as adec
    from mgr_amd.early_fusion import sequence_decoding as edec
    from mgr_amd.multimodal_fusion import sequence_decoding as fdec
    from mgr_amd.rgb_network import decode_rgb as rdec
    segs = [[(21, 2, 30, 0.99), (3, 31, 33, 0.8), (21, 34, 60, 0.97)], [(5, 2, 4, 0.7)], []]
    for mod, rec in ((fdec, "Sample00017.rec"), (edec, "Sample00017.rec"), (rdec, "Sample00017.rec"), (adec, "Sample00017_audio.rec")):
        out = str(tmp_path / "t.mlf")
        names, back = mod.decode_segments(segs, [17, 228, 5], out_file=out)
        assert back is segs and names == [[mod.map_gest[s[0]] for s in sg] for sg in segs]
        text = open(out).read().split("\n")
        assert text[1] == '"*/%s"' % rec and text[2] == "1000000 15500000 %s" % mod.map_gest[21]
        assert text[3] == "15500000 17000000 %s" % mod.map_gest[3]
        assert not any("Sample00228" in l for l in text)           # on the ignore list
        assert decoding.read_mlf(out)[rec.split(".")[0]] == names[0]
