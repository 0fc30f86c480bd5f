"""-m gpu: locating gestures in time - mgr_ctc_align (Viterbi forced alignment) and mgr_greedy_segments (the greedy decode with its frame
positions) against the fp64 restatements of tests/align_ref.py, against the shipped loss / decode, and through the facade."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-8
REL = 1e-4          # the project's bound for the CTC loss (README, north_star)


def _align_raw(device, P, lab, il, ll, skip=2, eps=EPS):
    """mgr_ctc_align through the C ABI: (path, seg, conf, logp)."""
    P = np.ascontiguousarray(P, np.float32)
    B, T, Cn = P.shape
    lab = np.ascontiguousarray(lab, np.int32)
    Lmax = lab.shape[1]
    arrs = [device.array(P), device.array(lab), device.array(np.asarray(il, np.int32)), device.array(np.asarray(ll, np.int32))]
    outs = [device.empty((B, T - skip), np.int32), device.empty((B, Lmax, 2), np.int32), device.empty((B, Lmax), np.float32),
            device.empty((B,), np.float64)]
    ws = device.bytes(device.lib.mgr_ctc_align_ws_bytes(B, T, Cn, Lmax))
    device.call("mgr_ctc_align", *arrs, B, T, Cn, Lmax, skip, Cn - 1, C.c_float(eps), *outs, ws, ws.nbytes)
    res = tuple(o.download() for o in outs)
    for a in arrs + outs + [ws]:
        a.free()
    return res


def _loss_raw(device, P, lab, il, ll, skip=2, eps=EPS):
    P = np.ascontiguousarray(P, np.float32)
    B, T, Cn = P.shape
    lab = np.ascontiguousarray(lab, np.int32)
    Lmax = lab.shape[1]
    arrs = [device.array(P), device.array(lab), device.array(np.asarray(il, np.int32)), device.array(np.asarray(ll, np.int32))]
    loss = device.empty((B,), np.float32)
    ws = device.bytes(device.lib.mgr_ctc_ws_bytes(B, T, Cn, Lmax))
    device.call("mgr_ctc_loss_grad", *arrs, B, T, Cn, Lmax, skip, Cn - 1, C.c_float(eps), C.c_float(1.0), loss, 0, ws, ws.nbytes)
    out = loss.download()
    for a in arrs + [loss, ws]:
        a.free()
    return out


def _random_labels(rng, L, Cn, p_repeat=0.25):
    out = []
    for k in range(L):
        if k and rng.random() < p_repeat:
            out.append(out[-1])
        else:
            out.append(int(rng.integers(0, Cn - 1)))
    return out


def _pad(label_lists, Lmax):
    lab = -np.ones((len(label_lists), Lmax), np.int32)
    for i, l in enumerate(label_lists):
        lab[i, :len(l)] = l
    return lab


@pytest.mark.parametrize("B,T,Cn,Lmax,mixed", [(64, 1900, 22, 35, False), (8, 1900, 44, 150, False), (8, 200, 44, 150, False),
                                                (17, 1000, 22, 35, True)])
def test_planted_alignments_are_recovered_exactly(device, B, T, Cn, Lmax, mixed):
    """P = 0.9 on the class of a randomly drawn valid alignment and 0.1 / (C - 1) elsewhere: any other valid alignment loses at least
    log(0.9 (C - 1) / 0.1) per differing frame, so the planted one is the unique optimum by a wide margin - path and seg equal it."""
    rng = np.random.default_rng(B * 1000 + T)
    skip, blank = 2, Cn - 1
    To = T - skip
    labels, il, states = [], [], []
    P = np.full((B, T, Cn), 1.0 / Cn, np.float32)
    for b in range(B):
        if mixed:
            L = [0, 1, Lmax, 20][b] if b < 4 else int(rng.integers(0, Lmax + 1))
            Tp = To if b % 3 == 0 else int(rng.integers(2 * L + 1, To + 1))
        else:
            L, Tp = Lmax, To
        lab = _random_labels(rng, L, Cn)
        if T == 200:        # the tight fit: 150 labels in 198 frames leave room for few repeats
            lab = _random_labels(rng, L, Cn, p_repeat=0.1)
            while L + sum(a == b_ for a, b_ in zip(lab, lab[1:])) > Tp:
                lab = _random_labels(rng, L, Cn, p_repeat=0.1)
        st = ar.planted_alignment(rng, Tp, lab, blank)
        P[b, :Tp + skip] = ar.planted_posteriors(st, lab, blank, Cn, skip)
        labels.append(lab)
        il.append(Tp)
        states.append(st)
    path, seg, conf, logp = _align_raw(device, P, _pad(labels, Lmax), il, [len(l) for l in labels])
    for b in range(B):
        want = ar.states_to_path(states[b], labels[b], blank)
        assert np.array_equal(path[b, :il[b]], want), b
        assert np.all(path[b, il[b]:] == -1)
        L = len(labels[b])
        assert [tuple(s) for s in seg[b, :L]] == ar.states_to_segments(states[b], L, skip), b
        assert np.all(seg[b, L:] == -1) and np.all(conf[b, L:] == 0)
        for k in range(L):
            n = seg[b, k, 1] - seg[b, k, 0] + 1
            assert abs(float(conf[b, k]) - float(np.float32(0.9))) <= (n + 1) * 2.0 ** -24 * 0.9
        score = ar.path_score(ar.log_emissions(P[b, :il[b] + skip], skip, EPS), want)
        assert abs(logp[b] - score) <= REL * abs(score)


def _unfriendly(rng, kind, T, Cn):
    if kind == "dirichlet":
        return rng.dirichlet(np.full(Cn, 0.3), size=T).astype(np.float32)
    if kind == "near_uniform":
        P = np.full((T, Cn), 1.0 / Cn) + rng.uniform(-1e-4, 1e-4, size=(T, Cn))
        return (P / P.sum(axis=1, keepdims=True)).astype(np.float32)
    P = rng.dirichlet(np.full(Cn, 0.3), size=T)                # exact zeros: eps decides
    P[rng.random((T, Cn)) < 0.5] = 0.0
    P[np.arange(T), rng.integers(0, Cn, T)] += 0.05
    return (P / P.sum(axis=1, keepdims=True)).astype(np.float32)


def test_optimal_score_on_unfriendly_posteriors(device):
    """The returned path is valid and its score, re-evaluated here in fp64, is within 1e-4 relative of the fp64 optimum; the returned
    logp is within the same bound of that score; conf is the fp64 mean of P over the label's frames to within (n + 1) 2^-24 relative
    (the worst case of any f32 summation order of n non-negative terms, plus the division).  Exact path equality is not asserted:
    near-ties may break differently in f32.  Measured (MI355X): see profiles/align_parity.txt."""
    rng = np.random.default_rng(11)
    skip = 2
    lines = []
    for (B, T, Cn, Lmax) in [(6, 1900, 22, 35), (3, 1900, 44, 150), (5, 333, 22, 35), (4, 320, 44, 150)]:
        for kind in ("dirichlet", "near_uniform", "zeros"):
            blank, To = Cn - 1, T - skip
            P = np.stack([_unfriendly(rng, kind, T, Cn) for _ in range(B)])
            labels, il = [], []
            for b in range(B):
                L = Lmax if b == 0 else int(rng.integers(0, min(Lmax, (To - 1) // 2) + 1))
                L = min(L, (To - 1) // 2)
                labels.append(_random_labels(rng, L, Cn))
                il.append(To if b < 2 else int(rng.integers(2 * L + 1, To + 1)))
            path, seg, conf, logp = _align_raw(device, P, _pad(labels, Lmax), il, [len(l) for l in labels])
            gap_opt = gap_logp = gap_conf = 0.0
            same = 0
            for b in range(B):
                logy = ar.log_emissions(P[b, :il[b] + skip], skip, EPS)
                opt, states = ar.viterbi(logy, labels[b], blank)
                pb = path[b, :il[b]]
                assert np.all(path[b, il[b]:] == -1) and pb.min() >= 0
                assert ar.collapse(pb, blank) == labels[b]
                L = len(labels[b])
                runs = ar.path_segments(pb, blank, skip)
                assert [(l, int(seg[b, k, 0]), int(seg[b, k, 1])) for k, l in enumerate(labels[b])] == runs
                assert np.all(seg[b, L:] == -1)
                score = ar.path_score(logy, pb)
                g1, g2 = abs(score - opt) / abs(opt), abs(logp[b] - score) / abs(score)
                gap_opt, gap_logp = max(gap_opt, g1), max(gap_logp, g2)
                same += bool(np.array_equal(ar.states_to_path(states, labels[b], blank), pb))
                assert score <= opt + 1e-9 * abs(opt)
                assert g1 <= REL and g2 <= REL, (kind, b, score, opt, logp[b])
                for k, (l, f, la) in enumerate(runs):
                    n = la - f + 1
                    want = P[b, f:la + 1, l].astype(np.float64).mean()
                    g3 = abs(float(conf[b, k]) - want) / want if want > 0 else abs(float(conf[b, k]))
                    gap_conf = max(gap_conf, g3 / ((n + 1) * 2.0 ** -24))
                    assert g3 <= (n + 1) * 2.0 ** -24, (kind, b, k, conf[b, k], want, n)
            lines.append("B=%d T=%d C=%d Lmax=%d %-12s  score vs fp64 optimum %.3e  logp vs fp64 score of the path %.3e  "
                         "conf error / bound %.3f  paths equal to the fp64 path %d/%d" % (B, T, Cn, Lmax, kind, gap_opt, gap_logp, gap_conf, same, B))
    print("\n".join(lines))
    out = os.environ.get("MGR_ALIGN_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            f.write("mgr_ctc_align against the fp64 restatement (tests/test_gpu_align.py): largest relative gaps per shape and kind of "
                    "posteriors; bound 1e-4\n" + "\n".join(lines) + "\n")


def test_logp_is_bounded_by_the_loss_and_infeasible_samples_stand_alone(device):
    """A single alignment cannot be more probable than all of them: logp <= -loss of mgr_ctc_loss_grad on the same inputs (1e-4
    relative slack).  A sample whose labels do not fit gives -inf where the loss gives +inf, and the other samples of its batch get,
    bit for bit, what a batch without it gives.  Label values outside the class range go through both calls alike."""
    rng = np.random.default_rng(5)
    B, T, Cn, Lmax, skip = 9, 120, 22, 35, 2
    To = T - skip
    P = rng.dirichlet(np.full(Cn, 0.5), size=(B, T)).astype(np.float32)
    labels = [_random_labels(rng, int(rng.integers(0, 30)), Cn) for _ in range(B)]
    labels[2] = [3] * 35                       # 35 labels + 34 repeats = 69 frames
    labels[4] = [-5, 99, 7, 7, 40]             # out of range: clipped to 0 / C - 1, as the loss clips them
    il = [To] * B
    il[2] = 68                                 # ... do not fit 68
    il[6] = 0                                  # no frames at all
    ll = [len(l) for l in labels]
    lab = _pad(labels, Lmax)
    path, seg, conf, logp = _align_raw(device, P, lab, il, ll)
    loss = _loss_raw(device, P, lab, il, ll)
    for b in range(B):
        if b in (2, 6):
            assert loss[b] == np.inf and logp[b] == -np.inf
            assert np.all(path[b] == -1) and np.all(seg[b] == -1) and np.all(conf[b] == 0)
        else:
            assert np.isfinite(loss[b]) and np.isfinite(logp[b])
            assert logp[b] <= -float(loss[b]) + REL * abs(float(loss[b])), (b, logp[b], loss[b])
    il[2] = 69                                 # exactly enough: feasible, one alignment only - the path IS the sum
    path2, seg2, conf2, logp2 = _align_raw(device, P, lab, il, ll)
    loss2 = _loss_raw(device, P, lab, il, ll)
    assert np.isfinite(logp2[2]) and abs(logp2[2] + float(loss2[2])) <= REL * abs(float(loss2[2]))
    assert list(path2[2, :69]) == [3 if t % 2 == 0 else Cn - 1 for t in range(69)]
    keep = [b for b in range(B) if b not in (2, 6)]
    sub = _align_raw(device, P[keep], lab[keep], [il[b] for b in keep], [ll[b] for b in keep])
    for full, part in zip((path, seg, conf, logp), sub):
        assert np.array_equal(full[keep], part)


@pytest.mark.parametrize("T,Cn,Lmax", [(64, 22, 35), (400, 44, 150), (1900, 22, 35)])
def test_tie_rule_on_uniform_posteriors(device, T, Cn, Lmax):
    """Every alignment has exactly the same score (every sum is a sum of identical numbers, in f32 too): the path is decided by the
    tie rule alone and equals the restatement's."""
    rng = np.random.default_rng(T)
    skip, blank, B = 2, Cn - 1, 6
    To = T - skip
    P = np.full((B, T, Cn), 1.0 / Cn, np.float32)
    labels = [[], [4], _random_labels(rng, min(Lmax, (To - 1) // 2), Cn), [2, 2, 2], _random_labels(rng, min(Lmax, To // 3), Cn, 0.5),
              _random_labels(rng, min(Lmax, 10), Cn)]
    il = [To, To, To, To, To - 7, max(21, To // 2)]
    path, seg, conf, logp = _align_raw(device, P, _pad(labels, Lmax), il, [len(l) for l in labels])
    for b in range(B):
        logy = ar.log_emissions(P[b, :il[b] + skip], skip, EPS)
        score, states = ar.viterbi(logy, labels[b], blank)
        assert np.array_equal(path[b, :il[b]], ar.states_to_path(states, labels[b], blank)), b
        assert [tuple(s) for s in seg[b, :len(labels[b])]] == ar.states_to_segments(states, len(labels[b]), skip)
        assert abs(logp[b] - score) <= REL * abs(score)


def test_forced_align_python_surface(device):
    from mgr_amd import decoding
    rng = np.random.default_rng(3)
    Cn, T, skip = 22, 90, 2
    labels = [[1, 2, 2, 5], [], [7]]
    states = [ar.planted_alignment(rng, T - skip, l, Cn - 1) for l in labels]
    P = np.stack([ar.planted_posteriors(s, l, Cn - 1, Cn, skip) for s, l in zip(states, labels)])
    segs, logp, path = decoding.forced_align(P, labels, dev=device, return_path=True)
    for b, l in enumerate(labels):
        want = ar.states_to_segments(states[b], len(l), skip)
        assert [(s[0], s[1], s[2]) for s in segs[b]] == [(c, f, e) for c, (f, e) in zip(l, want)]
        assert all(abs(s[3] - 0.9) < 1e-6 for s in segs[b])
        assert np.array_equal(path[b], ar.states_to_path(states[b], l, Cn - 1))
    padded = np.array([[1, 2, 2, 5], [np.nan] * 4, [7, np.nan, np.nan, np.nan]])
    segs2, logp2 = decoding.forced_align(P, padded, dev=device)
    assert segs2 == segs and np.array_equal(logp, logp2)
    # labels that do not fit: -inf and no segments, the others untouched
    segs3, logp3 = decoding.forced_align(P, labels, input_length=[T - skip, T - skip, 0], dev=device)
    assert segs3[:2] == segs[:2] and segs3[2] == [] and logp3[2] == -np.inf and np.array_equal(logp3[:2], logp[:2])


def _straddling(rng, N, T, Cn, thr):
    """Frame maxima on both sides of thr, in runs of a few frames: the filter drops first occurrences and changes the collapse."""
    P = np.zeros((N, T, Cn), np.float32)
    for n in range(N):
        t = 0
        while t < T:
            k, lab = int(rng.integers(1, 7)), int(rng.integers(0, Cn))
            for u in range(t, min(T, t + k)):
                hi = float(rng.uniform(max(thr - 0.3, 1.0 / Cn + 0.05), min(thr + 0.3, 0.9995)))
                P[n, u] = (1.0 - hi) / (Cn - 1)
                P[n, u, lab] = hi
            t += k
    return P


def _check_segments(segs, P, thr, skip=2):
    for n in range(P.shape[0]):
        want = ar.greedy_segments(P[n], thr, skip, with_count=True)
        assert [s[:3] for s in segs[n]] == [w[:3] for w in want], n
        for s, w in zip(segs[n], want):      # (the bound of any f32 summation order of w[4] non-negative terms, plus the division)
            assert abs(s[3] - w[3]) <= (w[4] + 1) * 2.0 ** -24 * w[3], (n, s, w)


@pytest.mark.parametrize("thr", [0.5, 0.75, 0.97, None])
@pytest.mark.parametrize("N,T,Cn", [(7, 90, 22), (3, 1900, 44), (64, 333, 22)])
def test_greedy_segments_equal_greedy_decode_and_the_restatement(device, thr, N, T, Cn):
    from mgr_amd import decoding
    from oracle.keras_ref import greedy_decode_quirk
    rng = np.random.default_rng(N + T)
    P = _straddling(rng, N, T, Cn, 0.5 if thr is None else thr)
    if thr is not None:
        P[0, :, :] = 1.0 / Cn                  # nothing survives: an empty result
        P[0, :, 2] += 1e-3
    segs = decoding.greedy_segments(P, thr, dev=device)
    labels = [[s[0] for s in sg] for sg in segs]
    assert labels == decoding.greedy_decode(P, thr, dev=device)
    if thr is not None:
        assert labels[0] == []
        if T <= 333:
            assert labels == greedy_decode_quirk(P, thr)      # the literal restatement of the reference's loop
    _check_segments(segs, P, thr)


def test_greedy_segments_on_the_golden_posteriors(device):
    from mgr_amd import decoding
    z = np.load(GOLDEN + "/decode_small.npz")
    unpad = lambda a: [[int(v) for v in r if v >= 0] for r in a]
    for thr, key in ((0.5, "greedy_thr05"), (0.75, "greedy_thr075")):
        segs = decoding.greedy_segments(z["P"], thr, dev=device)
        assert [[s[0] for s in sg] for sg in segs] == unpad(z[key])
        _check_segments(segs, z["P"], thr)


def test_greedy_segments_overflow_is_reported(device):
    """More runs than the output holds: the device reports the TRUE count and fills what fits; the Python layer runs again with room
    for every frame (decoding.greedy_segments) or raises (segments_from_arrays)."""
    from mgr_amd import decoding
    N, T, Cn, skip, cap = 3, 700, 22, 2, 16
    P = np.full((N, T, Cn), 0.01, np.float32)
    for n in range(N):
        for t in range(T):
            P[n, t, (t // (n + 1)) % 5] = 0.79             # sample n: a new run every n + 1 frames
    want = [ar.greedy_segments(P[n], None, skip) for n in range(N)]
    counts = [len(w) for w in want]
    assert counts[0] == T - skip and min(counts) > 200       # (every frame a run of its own in sample 0: the most there can be)
    dP = device.array(P)
    dn, dl, ds, dc = device.empty((N,), np.int32), device.empty((N, cap), np.int32), device.empty((N, cap, 2), np.int32), device.empty((N, cap))
    device.call("mgr_greedy_segments", dP, N, T, Cn, skip, C.c_float(-1.0), cap, dn, dl, ds, dc)
    n, lab, seg, conf = dn.download(), dl.download(), ds.download(), dc.download()
    assert n.tolist() == counts
    for b in range(N):
        assert [(int(lab[b, r]), int(seg[b, r, 0]), int(seg[b, r, 1])) for r in range(cap)] == [w[:3] for w in want[b][:cap]]
    with pytest.raises(OverflowError):
        decoding.segments_from_arrays(n, lab, seg, conf)
    for a in (dP, dn, dl, ds, dc):
        a.free()
    segs = decoding.greedy_segments(P, None, dev=device)        # default capacity 256 < 698: falls back, nothing is lost
    assert [[s[:3] for s in sg] for sg in segs] == [[w[:3] for w in ws_] for ws_ in want]
    assert [len(sg) for sg in decoding.greedy_segments(P, None, dev=device, max_segments=1000)] == counts


def _batches(spec, B, T, Lmax, n, seed0=300):
    from mgr_amd.synthetic import synthetic_arrays
    return [synthetic_arrays(spec, B, T, Lmax, seed0 + i, lmin=2, lmax=5) for i in range(n)]


def test_facade_segments_and_align(device, tmp_path):
    """predict_generator(decode="segments") equals greedy_segments of predict_generator(decode=None), with a short last batch; the
    other modes give what they gave before the new modes first ran in the process; align_generator equals forced_align of the
    posteriors; the module's decode_segments writes a timed MLF that scores like the untimed one."""
    from mgr_amd import decoding, keras_like as K
    from mgr_amd.configs import fusion_spec
    from mgr_amd.keras_like import Model
    from mgr_amd.multimodal_fusion import sequence_decoding as sd
    from mgr_amd.synthetic import synthetic_weights
    K.set_learning_phase(0)
    decoding._DEV[0] = device
    spec = fusion_spec()
    B, T, Lmax = 8, 64, 4
    full = _batches(spec, B, T, Lmax, 5, seed0=400)
    data = [b[0] for b in full]
    data[-1] = {k: v[:3] for k, v in data[-1].items()}                 # a short last batch
    m = Model(spec, device=device)
    m.set_weights_dict(synthetic_weights(spec, 11))
    P = m.predict_generator(iter(data), steps=5)
    am = m.predict_generator(iter(data), steps=5, decode="argmax")
    bm = m.predict_generator(iter(data), steps=5, decode="beam", beam_width=10)
    thr_mid = float(np.median(P[:, 2:].max(axis=2)))      # (untrained posteriors are flat: the threshold that straddles them)
    for thr in (None, thr_mid, sd.THRESHOLD):
        segs = m.predict_generator(iter(data), steps=5, decode="segments", threshold=thr)
        assert len(segs) == 4 * B + 3
        assert segs == decoding.greedy_segments(P, thr, dev=device)
        assert [[s[0] for s in sg] for sg in segs] == decoding.greedy_decode(P, thr, dev=device)
        if thr != sd.THRESHOLD:
            assert sum(len(sg) > 1 for sg in segs) >= B
    assert np.array_equal(P, m.predict_generator(iter(data), steps=5))
    am2 = m.predict_generator(iter(data), steps=5, decode="argmax")
    assert np.array_equal(am[0], am2[0]) and np.array_equal(am[1], am2[1])
    bm2 = m.predict_generator(iter(data), steps=5, decode="beam", beam_width=10)
    assert bm[0] == bm2[0] and np.array_equal(bm[1], bm2[1])
    # the module: names as decode_batch, a timed MLF
    f_list = list(range(1, P.shape[0] + 1))
    names = sd.decode_batch(P, f_list, out_file=str(tmp_path / "a.mlf"))
    names2, segs2 = sd.decode_segments(P, f_list, out_file=str(tmp_path / "b.mlf"))
    names3, _ = sd.decode_segments(segs, f_list, out_file=str(tmp_path / "c.mlf"))
    assert names == names2 == names3
    assert open(tmp_path / "b.mlf").read() == open(tmp_path / "c.mlf").read()
    assert decoding.read_mlf(str(tmp_path / "a.mlf")) == decoding.read_mlf(str(tmp_path / "b.mlf"))
    assert decoding.score_mlf(str(tmp_path / "a.mlf"), str(tmp_path / "b.mlf"))[0] == 0.0
    # ... and on posteriors that survive the module's threshold: every line carries its segment's times
    Ps = _straddling(np.random.default_rng(1), 6, 80, 22, sd.THRESHOLD)
    na = sd.decode_batch(Ps, f_list[:6], out_file=str(tmp_path / "d.mlf"))
    nb, sb = sd.decode_segments(Ps, f_list[:6], out_file=str(tmp_path / "e.mlf"))
    assert na == nb and sum(len(x) for x in na) > 30
    assert decoding.read_mlf(str(tmp_path / "d.mlf")) == decoding.read_mlf(str(tmp_path / "e.mlf"))
    timed = [l.split() for l in open(tmp_path / "e.mlf").read().split("\n") if l[:1].isdigit()]
    flat = [(s_, n_) for sg, ns in zip(sb, nb) for s_, n_ in zip(sg, ns)]
    assert len(timed) == len(flat)
    for (start, end, name), (s_, n_) in zip(timed, flat):
        assert (int(start), int(end), name) == (s_[1] * 500000, (s_[2] + 1) * 500000, n_)
    # alignment of each sample's own labels, through a training engine (short last batch again)
    def gen():
        for i, (xs, lab, il, ll) in enumerate(full):
            n = 3 if i == 4 else B
            x = {k: v[:n] for k, v in xs.items()}
            x.update(the_labels=lab[:n], input_length=il[:n], label_length=ll[:n])
            yield x, None
    asegs, alogp, apath = m.align_generator(gen(), steps=5, return_path=True)
    P2 = m.predict_generator(iter(data), steps=5)     # (from the training engine the alignment built)
    lab = np.concatenate([b[1][:(3 if i == 4 else B)] for i, b in enumerate(full)])
    ll = np.concatenate([b[3][:(3 if i == 4 else B)] for i, b in enumerate(full)]).reshape(-1)
    fsegs, flogp, fpath = decoding.forced_align(P2, lab, label_length=ll, dev=device, return_path=True, eps=float(spec.ctc["eps"]))
    assert asegs == fsegs and np.array_equal(alogp, flogp) and np.array_equal(apath, fpath)
    assert all(len(sg) == n for sg, n in zip(asegs, ll)) and np.all(np.isfinite(alogp))


def test_pipelined_segments_and_align_equal_one_batch_at_a_time(device):
    from mgr_amd.configs import fusion_spec
    from mgr_amd.engine import Engine
    from mgr_amd.synthetic import synthetic_weights
    spec = fusion_spec()
    B, T, Lmax = 16, 72, 6
    data = _batches(spec, B, T, Lmax, 4)
    eng = Engine(spec, B, T, Lmax, device=device, seed=5)
    eng.set_weights(synthetic_weights(spec, 11))
    pipe = list(eng.predict_stream((b[0] for b in data), output="segments"))
    single = [list(eng.predict_stream([b[0]], output="segments"))[0] for b in data]
    assert pipe == single and pipe[0] != pipe[1]
    pipe = list(eng.predict_stream(iter(data), output="align"))
    single = [list(eng.predict_stream([b], output="align"))[0] for b in data]
    for a, b in zip(pipe, single):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert not np.array_equal(pipe[0][2], pipe[1][2])
    eng.close()
    inf = Engine(spec, B, T, Lmax, device=device, seed=5, inference_only=True)
    with pytest.raises(ValueError):
        list(inf.predict_stream(iter(data), output="align"))
    inf.close()
