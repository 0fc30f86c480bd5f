"""-m gpu: mgr_ctc_occupancy - forward-backward state posteriors and quantile extents - against the fp64 restatement of
tests/occupancy_ref.py, against the float32 restatement of its pinned extent arithmetic, against the shipped loss and aligner, and
through decoding.posterior_align.

Shapes: the kernel walks a sample in tiles of FT frames, FT = 256, 128 or 64 - the largest whose LDS rows (2 Lmax + 3 floats of states
and C | 1 floats of posteriors a frame) fit 160 KiB: 256 up to Lmax = 67 at C = 22, 128 up to Lmax = 147, 64 above.  Each FT is met one
frame below, at and one above a tile, the lattice at one pair per lane (Lmax + 1 <= 64) and two (Lmax = 64, 65: the loss's own edge)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as ar  # noqa: E402
import occupancy_ref as oc  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-8
ABS = 1e-4          # gamma, occ / max(occ), conf: entries are at most 1 - the project's bound for the same quantity inside the CTC gradient
REL = 1e-4          # logp: the loss's bound
SKIP = 2


def _occupancy_raw(device, P, lab, il, ll, q=0.5, want_gamma=True, skip=SKIP, eps=EPS):
    """mgr_ctc_occupancy through the C ABI: (gamma or None, seg, occ, conf, logp)."""
    P = np.ascontiguousarray(P, np.float32)
    B, T, Cn = P.shape
    lab = np.ascontiguousarray(lab, np.int32)
    Lmax = lab.shape[1]
    arrs = [device.array(P), device.array(lab), device.array(np.asarray(il, np.int32)), device.array(np.asarray(ll, np.int32))]
    gamma = device.empty((B, T - skip, 2 * Lmax + 1), np.float32) if want_gamma else None
    outs = [device.empty((B, Lmax, 2), np.int32), device.empty((B, Lmax), np.float32), device.empty((B, Lmax), np.float32),
            device.empty((B,), np.float64)]
    ws = device.bytes(device.lib.mgr_ctc_ws_bytes(B, T, Cn, Lmax))
    device.call("mgr_ctc_occupancy", *arrs, B, T, Cn, Lmax, skip, Cn - 1, C.c_float(eps), C.c_float(q), gamma, *outs, ws, ws.nbytes)
    res = (gamma.download() if want_gamma else None,) + tuple(o.download() for o in outs)
    for a in arrs + outs + [ws] + ([gamma] if want_gamma else []):
        a.free()
    return res


def _loss_raw(device, P, lab, il, ll, skip=SKIP, eps=EPS):
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


def _align_seg(device, P, lab, il, ll, skip=SKIP, eps=EPS):
    P = np.ascontiguousarray(P, np.float32)
    B, T, Cn = P.shape
    lab = np.ascontiguousarray(lab, np.int32)
    Lmax = lab.shape[1]
    arrs = [device.array(P), device.array(lab), device.array(np.asarray(il, np.int32)), device.array(np.asarray(ll, np.int32))]
    outs = [device.empty((B, T - skip), np.int32), device.empty((B, Lmax, 2), np.int32), device.empty((B, Lmax), np.float32),
            device.empty((B,), np.float64)]
    ws = device.bytes(device.lib.mgr_ctc_align_ws_bytes(B, T, Cn, Lmax))
    device.call("mgr_ctc_align", *arrs, B, T, Cn, Lmax, skip, Cn - 1, C.c_float(eps), *outs, ws, ws.nbytes)
    seg = outs[1].download()
    for a in arrs + outs + [ws]:
        a.free()
    return seg


def _labels(rng, L, Cn, p_repeat):
    out = []
    for k in range(L):
        out.append(out[-1] if k and rng.random() < p_repeat else int(rng.integers(0, Cn - 1)))
    return out


def _case(seed, B, To, Lmax, Cn, third):
    """Sample 0: the whole input, as many labels as always fit.  Sample 1: a shorter input, repeated neighbours, one label value outside
    the class range.  Sample 2: `third` - "empty" (label_len 0), "noinput" (input_len 0) or "nofit" (more labels than frames)."""
    rng = np.random.default_rng(seed)
    P = rng.dirichlet(np.full(Cn, 0.3), size=(B, To + SKIP)).astype(np.float32)
    lab = -np.ones((B, Lmax), np.int32)
    il, ll = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        if b == 0:
            il[b], L, rep = To, min(Lmax, (To + 1) // 2), 0.25
        elif b == 1:
            il[b] = max(1, To - 3)
            L, rep = min(Lmax, max(1, il[b] // 4)), 0.5
        else:
            il[b], L, rep = To, min(Lmax, max(1, To // 5)), 0.25
            if third == "empty":
                L = 0
            elif third == "noinput":
                il[b] = 0
            elif L >= 2:
                il[b] = L - 1          # "nofit"
            else:
                L = 0
        row = _labels(rng, L, Cn, rep)
        if b == 1 and L:
            row[L // 2] = Cn + 3
        lab[b, :L] = row
        ll[b] = L
    return P, lab, il, ll


#        B  To   Lmax C   third
CASES = [(1, 1, 1, 3, None), (3, 2, 1, 3, "empty"), (3, 2, 3, 22, "noinput"),
         (3, 255, 3, 22, "nofit"), (1, 256, 3, 3, None), (3, 257, 3, 3, "empty"),               # FT = 256
         (3, 257, 64, 22, "nofit"), (1, 256, 65, 22, None), (3, 255, 65, 3, "noinput"),         # two pairs a lane
         (3, 127, 100, 22, "empty"), (1, 128, 100, 3, None), (3, 129, 100, 22, "nofit"),        # FT = 128
         (3, 63, 200, 22, "noinput"), (1, 64, 200, 22, None), (3, 65, 200, 3, "nofit"), (1, 130, 200, 22, None)]   # FT = 64


@pytest.mark.parametrize("q", [0.5, 0.05])
@pytest.mark.parametrize("case", CASES, ids=["B%d-To%d-L%d-C%d-%s" % c for c in CASES])
def test_occupancy_against_fp64(device, case, q):
    B, To, Lmax, Cn, third = case
    P, lab, il, ll = _case(1000 * To + Lmax + B, B, To, Lmax, Cn, third)
    gamma, seg, occ, conf, logp = _occupancy_raw(device, P, lab, il, ll, q)
    _, seg0, occ0, conf0, logp0 = _occupancy_raw(device, P, lab, il, ll, q, want_gamma=False)
    loss = _loss_raw(device, P, lab, il, ll)
    # the same with and without gamma; logp is the loss's own
    assert np.array_equal(seg, seg0) and np.array_equal(occ, occ0) and np.array_equal(conf, conf0) and np.array_equal(logp, logp0)
    assert np.array_equal(logp, -loss.astype(np.float64))
    worst = dict(gamma=0.0, occ=0.0, conf=0.0, logp=0.0)
    for b in range(B):
        L = int(ll[b])
        ref = oc.occupancy(P[b], lab[b, :L], il[b], q, SKIP)
        assert np.all(seg[b, L:] == -1) and not occ[b, L:].any() and not conf[b, L:].any()
        assert not gamma[b, :, 2 * L + 1:].any() and not gamma[b, il[b]:].any()
        if not np.isfinite(ref["logp"]):
            assert logp[b] == -np.inf and np.all(seg[b] == -1) and not occ[b].any() and not conf[b].any() and not gamma[b].any()
            continue
        worst["logp"] = max(worst["logp"], abs(logp[b] - ref["logp"]) / abs(ref["logp"]))
        worst["gamma"] = max(worst["gamma"], np.abs(gamma[b, :, :2 * L + 1] - ref["gamma"]).max())
        # the pinned arithmetic: seg from the kernel's own float32 gamma, no exception allowed
        assert [tuple(r) for r in seg[b, :L]] == oc.extents_from_gamma(gamma[b, :il[b]], q, L, SKIP)
        if L:
            worst["occ"] = max(worst["occ"], np.abs(occ[b, :L] - ref["occ"]).max() / ref["occ"].max())
            worst["conf"] = max(worst["conf"], np.abs(conf[b, :L] - ref["conf"]).max())
        else:
            assert np.all(gamma[b, :il[b], 0] == 1.0)
    print("occupancy %s q=%g worst %s" % (case, q, worst))
    assert worst["gamma"] <= ABS and worst["occ"] <= ABS and worst["conf"] <= ABS and worst["logp"] <= REL


def test_planted_extents_equal_viterbi(device):
    rng = np.random.default_rng(11)
    Cn, blank, To = 6, 5, 60
    rows = [[0], [3, 3, 1], [4, 0, 1, 1, 1, 3]]
    Lmax = max(len(r) for r in rows)
    lab = -np.ones((len(rows), Lmax), np.int32)
    P, planted = [], []
    for b, r in enumerate(rows):
        lab[b, :len(r)] = r
        states = ar.planted_alignment(rng, To, r, blank)
        P.append(ar.planted_posteriors(states, r, blank, Cn, skip=SKIP, hi=0.999))
        planted.append(ar.states_to_segments(states, len(r), SKIP))
    P = np.stack(P)
    il, ll = np.full(len(rows), To, np.int32), np.asarray([len(r) for r in rows], np.int32)
    _, seg, occ, conf, logp = _occupancy_raw(device, P, lab, il, ll, 0.5)
    vit = _align_seg(device, P, lab, il, ll)
    for b, r in enumerate(rows):
        assert [tuple(x) for x in seg[b, :len(r)]] == planted[b] == [tuple(x) for x in vit[b, :len(r)]]
        # an alignment that differs from the planted one in k frames weighs (0.0002 / 0.999)^k of it: a boundary moves with weight 2e-4
        dwell = np.asarray([l - f + 1 for f, l in planted[b]])
        assert np.abs(occ[b, :len(r)] - dwell).max() <= 0.05 and np.all(conf[b, :len(r)] > 0.99)


def test_sample_is_independent_of_its_batch(device):
    P, lab, il, ll = _case(77, 3, 129, 100, 22, "nofit")
    whole = _occupancy_raw(device, P, lab, il, ll, 0.2)
    for b in (0, 1):
        alone = _occupancy_raw(device, P[b:b + 1], lab[b:b + 1], il[b:b + 1], ll[b:b + 1], 0.2)
        for x, y in zip(whole, alone):
            assert np.array_equal(x[b:b + 1], y)
    again = _occupancy_raw(device, P, lab, il, ll, 0.2)
    assert all(np.array_equal(x, y) for x, y in zip(whole, again))          # deterministic


def test_bad_arguments_are_refused(device):
    from mgr_amd._capi import MgrError
    P, lab, il, ll = _case(1, 1, 8, 2, 3, None)
    for q in (0.0, 0.6):
        with pytest.raises(MgrError):
            _occupancy_raw(device, P, lab, il, ll, q)


def test_posterior_align_facade(device):
    from mgr_amd import decoding
    P, lab, il, ll = _case(5, 3, 65, 4, 22, "nofit")
    gamma, seg, occ, conf, logp = _occupancy_raw(device, P, lab, il, ll, 0.2)
    segs, lp, g = decoding.posterior_align(P, lab, ll, il, quantile=0.2, skip=SKIP, dev=device, return_gamma=True)
    assert np.array_equal(lp, logp) and np.array_equal(g, gamma)
    clipped = np.clip(lab, 0, 21)
    for b in range(3):
        n = int(ll[b]) if np.isfinite(logp[b]) else 0
        assert segs[b] == [(int(clipped[b, k]), int(seg[b, k, 0]), int(seg[b, k, 1]), float(conf[b, k]), float(occ[b, k])) for k in range(n)]
    assert segs[2] == [] and lp[2] == -np.inf
    segs2, lp2 = decoding.posterior_align(P, [list(r[:n]) for r, n in zip(lab, ll)], input_length=il, quantile=0.2, skip=SKIP, dev=device)
    assert segs2 == segs and np.array_equal(lp2, lp)


def test_align_generator_posterior_mode(device):
    """align_generator(mode="posterior") equals posterior_align of predict_generator's posteriors bit for bit (a short last batch); the
    default mode returns what it returned; the pipelined pass equals one batch at a time."""
    from mgr_amd import decoding, keras_like as K
    from mgr_amd.configs import fusion_spec
    from mgr_amd.keras_like import Model
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    K.set_learning_phase(0)
    spec = fusion_spec()
    B, T, Lmax, steps = 8, 64, 4, 3
    full = [synthetic_arrays(spec, B, T, Lmax, 400 + i, lmin=2, lmax=4) for i in range(steps)]
    size = lambda i: 3 if i == steps - 1 else B

    def gen():
        for i, (xs, lab, il, ll) in enumerate(full):
            x = {k: v[:size(i)] for k, v in xs.items()}
            x.update(the_labels=lab[:size(i)], input_length=il[:size(i)], label_length=ll[:size(i)])
            yield x, None
    m = Model(spec, device=device)
    m.set_weights_dict(synthetic_weights(spec, 11))
    vsegs, vlogp = m.align_generator(gen(), steps=steps)
    psegs, plogp = m.align_generator(gen(), steps=steps, mode="posterior", quantile=0.2)
    P = m.predict_generator(({k: v[:size(i)] for k, v in b[0].items()} for i, b in enumerate(full)), steps=steps)
    lab = np.concatenate([b[1][:size(i)] for i, b in enumerate(full)])
    ll = np.concatenate([b[3][:size(i)] for i, b in enumerate(full)]).reshape(-1)
    il = np.concatenate([b[2][:size(i)] for i, b in enumerate(full)]).reshape(-1)
    eps = float(spec.ctc["eps"])
    fsegs, flogp = decoding.posterior_align(P, lab, ll, il, quantile=0.2, dev=device, eps=eps)
    assert psegs == fsegs and np.array_equal(plogp, flogp)
    assert all(len(sg) == n and all(len(s) == 5 for s in sg) for sg, n in zip(psegs, ll)) and np.all(np.isfinite(plogp))
    wsegs, wlogp = decoding.forced_align(P, lab, ll, il, dev=device, eps=eps)
    assert vsegs == wsegs and np.array_equal(vlogp, wlogp)            # the default mode: what it was
    assert np.all(plogp >= vlogp)                                     # all alignments weigh at least what the best one does
    with pytest.raises(ValueError):
        m.align_generator(gen(), steps=steps, mode="median")
    with pytest.raises(ValueError):
        m.align_generator(gen(), steps=steps, mode="posterior", return_path=True)


def test_decode_extents_of_the_modules(device, tmp_path):
    from mgr_amd import decoding
    from mgr_amd.audio_network import sequence_decoding as asd
    from mgr_amd.multimodal_fusion import sequence_decoding as sd
    decoding._DEV[0] = device
    rng = np.random.default_rng(2)
    Cn, blank, To = 22, 21, 70
    rows = [[3, 3, 7], [20], [1, 2, 3, 4]]
    P = np.stack([ar.planted_posteriors(ar.planted_alignment(rng, To, r, blank), r, blank, Cn, skip=SKIP, hi=0.99) for r in rows])
    f_list = [1, 2, 3]
    names, segs = sd.decode_extents(P, f_list, out_file=str(tmp_path / "ext.mlf"))
    _, spikes = sd.decode_segments(P, f_list, out_file=None)
    assert names == [[sd.map_gest[k] for k in r] for r in rows]
    assert [[s[:3] for s in sg] for sg in segs] == [[s[:3] for s in sg if s[0] != blank] for sg in spikes]
    back = decoding.read_mlf_segments(str(tmp_path / "ext.mlf"))
    assert back["Sample00001"] == [(n, s[1], s[2]) for n, s in zip(names[0], segs[0])]
    wide = sd.decode_extents(P, f_list, quantile=0.01, out_file=None)[1]
    assert all(w[1] <= s[1] and w[2] >= s[2] for ws, sg in zip(wide, segs) for w, s in zip(ws, sg))
    r = decoding.jaccard_index(segs, spikes, Cn, To + SKIP, ignore=(blank,), dev=device)
    assert r["jaccard"] == 1.0
    # the audio network: word posteriors, gesture extents
    lex = asd.GESTURE_LEXICON
    gest = [[1, 3], [5]]
    Ca = 44
    words = [[int(w) for g in seq for w in lex[g]] for seq in gest]
    Pa = np.stack([ar.planted_posteriors(ar.planted_alignment(rng, To, w, Ca - 1), w, Ca - 1, Ca, skip=SKIP, hi=0.99) for w in words])
    gn, gs = asd.decode_extents(Pa, [1, 2], out_file=str(tmp_path / "gext.mlf"))
    ln, ls = asd.decode_lexicon(Pa, [1, 2], out_file=None)
    assert gn == ln == [[asd.gesture_names[g] for g in seq] for seq in gest]
    assert [[s[:3] for s in sg] for sg in gs] == [[s[:3] for s in sg] for sg in ls]
