"""-m gpu: mgr_ctc_rescore - log p(hypothesis | posteriors) summed over all CTC alignments, K hypotheses per sample in one launch -
against the fp64 restatement of tests/rescore_ref.py, against the shipped loss / aligner / beam kernels on the same inputs, through
the lexicon, through decoding.rescore_nbest on the planted cases of tests/rescore_cases.py, and through the facade."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rescore_cases as rc  # noqa: E402
import rescore_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

SKIP, EPS, REL = rc.SKIP, rc.EPS, rc.REL


def _raw(device, P, hyp, hyp_len, il=None, skip=SKIP, blank=None, eps=EPS, lexicon=None, want_nlab=True, lex_arrays=None):
    """mgr_ctc_rescore through the C ABI; hyp / hyp_len may be host arrays or device arrays.  Returns (logp, n_lab or None)."""
    from mgr_amd import decoding
    from mgr_amd._capi import DeviceArray
    P = np.ascontiguousarray(P, np.float32)
    B, T, Cn = P.shape
    blank = Cn - 1 if blank is None else blank
    off = words = None
    G = 0
    if lex_arrays is not None:
        off, words, G = lex_arrays
    elif lexicon is not None:
        off, words = decoding.compile_lexicon(lexicon, Cn, blank)
        G = len(off) - 1
    il = np.full(B, T - skip, np.int32) if il is None else np.asarray(il, np.int32)
    own = [device.array(P), device.array(il)]
    dh = hyp if isinstance(hyp, DeviceArray) else device.array(np.ascontiguousarray(hyp, np.int32))
    dl = hyp_len if isinstance(hyp_len, DeviceArray) else device.array(np.ascontiguousarray(hyp_len, np.int32))
    own += [a for a, src in ((dh, hyp), (dl, hyp_len)) if a is not src]
    K, Lh = dh.shape[1], dh.shape[2]
    dlogp = device.empty((B, K), np.float64)
    dn = device.empty((B, K), np.int32) if want_nlab else None
    host = lambda a: None if a is None else a.ctypes.data
    ws = device.bytes(device.lib.mgr_ctc_rescore_ws_bytes(B, T, Cn, G, host(off)))
    own += [dlogp, ws] + ([dn] if want_nlab else [])
    try:
        device.call("mgr_ctc_rescore", own[0], own[1], B, T, Cn, skip, blank, C.c_float(eps), host(off), host(words), G, dh, dl, K, Lh,
                    dlogp, dn, ws, ws.nbytes)
        return dlogp.download(), (dn.download() if want_nlab else None)
    finally:
        for a in own:
            a.free()


class Gap:
    """The largest measured relative gap of a test (printed: profiles/rescore_parity.txt records them)."""

    def __init__(self, what):
        self.what, self.gap, self.n = what, 0.0, 0

    def check(self, got, want, where=None):
        """Arrays of logp: NaN where NaN, -inf where -inf, within REL where finite."""
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape
        assert np.array_equal(np.isnan(got), np.isnan(want)), (self.what, where, got, want)
        assert np.array_equal(got == -np.inf, want == -np.inf), (self.what, where, got, want)
        fin = np.isfinite(want)
        assert np.all(np.isfinite(got[fin]))
        if fin.any():
            g = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)
            g = np.where(want[fin] == 0, np.abs(got[fin]), g)
            self.gap, self.n = max(self.gap, float(g.max())), self.n + int(fin.sum())
            assert g.max() <= REL, (self.what, where, got, want)

    def done(self):
        print("rescore parity: %-44s %5d finite scores   largest gap to the fp64 restatement %.3e" % (self.what, self.n, self.gap))


def _against_ref(device, gap, P, hyps, K, Lh, where=None, **kw):
    hyp, hl = rc.pack(hyps, K, Lh)
    logp, n_lab = _raw(device, P, hyp, hl, **kw)
    Cn = P.shape[2]
    blank = Cn - 1 if kw.get("blank") is None else kw["blank"]
    wl, wn = rr.score_batch(P, hyp, hl, blank, kw.get("skip", SKIP), kw.get("eps", EPS), kw.get("il"), kw.get("lexicon"))
    gap.check(logp, wl, where)
    assert np.array_equal(n_lab, wn), (where, n_lab, wn)
    return logp, n_lab


def _labels(rng, Cn, L):
    return [int(v) for v in rng.integers(0, Cn - 1, L)]


def test_every_lattice_width(device):
    """Expanded lengths at every edge of the pairs-per-lane instantiations, with T - skip just above what each needs; narrow and
    wide hypotheses share a sample (a wave picks its width from its own hypothesis); 256 labels are not scored."""
    gap = Gap("lattice widths 0 .. 255")
    Cn, B, K = 5, 2, 4
    for L in (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255):
        rng = np.random.default_rng(L)
        hyps = [[_labels(rng, Cn, L), _labels(rng, Cn, min(3, L)), _labels(rng, Cn, L), _labels(rng, Cn, max(L - 1, 0))] for _ in range(B)]
        To = max(rr.needs(h) for row in hyps for h in row) + 3
        P = rng.dirichlet(np.full(Cn, 0.5), size=(B, To + SKIP)).astype(np.float32)
        logp, _ = _against_ref(device, gap, P, hyps, K, max(L, 1), where=L)
        assert np.all(np.isfinite(logp))
    rng = np.random.default_rng(256)
    hyps = [[_labels(rng, Cn, 256), _labels(rng, Cn, 255), [], _labels(rng, Cn, 7)] for _ in range(B)]
    P = rng.dirichlet(np.full(Cn, 0.5), size=(B, 600)).astype(np.float32)
    logp, n_lab = _against_ref(device, gap, P, hyps, K, 256, where=256)
    assert np.all(np.isnan(logp[:, 0])) and np.all(n_lab[:, 0] == 256) and np.all(np.isfinite(logp[:, 1:]))
    gap.done()


def test_frames_and_input_lengths(device):
    """Every renormalisation (16 frames) and prefetch-chunk (8 frames) edge as a ragged input_len within ONE batch, lengths above
    T - skip and below 0, repeated labels that fit only with their forced blanks and the same one frame short."""
    gap = Gap("frames: ragged input_len")
    Cn, To = 6, 257
    il = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 40, 257, 100000, -5, 7, 6]
    B = len(il)
    rng = np.random.default_rng(11)
    P = rng.dirichlet(np.full(Cn, 0.5), size=(B, To + SKIP)).astype(np.float32)
    P[12] = P[11]
    hyps = [[[], [1], [2, 2], [0, 1, 2, 1], [3, 3, 3, 3]] for _ in range(B)]        # [3, 3, 3, 3] needs 7 frames
    logp, n_lab = _against_ref(device, gap, P, hyps, 5, 4, il=il)
    assert logp[0, 0] == 0.0 and np.all(logp[0, 1:] == -np.inf)                   # Tp = 0
    assert logp[2, 2] == -np.inf and np.isfinite(logp[3, 2])                      # [2, 2]: 2 frames, 3 frames
    assert logp[15, 4] == -np.inf and np.isfinite(logp[14, 4])                    # [3, 3, 3, 3]: 6 frames, 7 frames
    assert np.array_equal(logp[12], logp[11]) and np.array_equal(logp[13], logp[0])     # clipped to T - skip, and to 0
    assert np.all(n_lab == [0, 1, 2, 4, 4])
    gap.done()


def test_slots(device):
    """K at and around the four hypotheses of a workgroup; absent slots first, in the middle, a sample without any; rows of 1898
    entries holding ten labels or fewer; n_lab NULL."""
    gap = Gap("slots: K, absent, Lh = 1898")
    Cn = 7
    for K in (1, 2, 5, 33):
        rng = np.random.default_rng(K)
        B = 3
        P = rng.dirichlet(np.full(Cn, 0.5), size=(B, 30)).astype(np.float32)
        hyps = rc.random_hyps(rng, Cn - 1, B, K, 10, p_absent=0.3)
        hyps[0][0] = None
        if K > 1:
            hyps[0][-1] = [1, 2]
        hyps[1] = [None] * K
        hyps[2][K // 2] = None
        Lh = 1898 if K == 5 else 10
        logp, n_lab = _against_ref(device, gap, P, hyps, K, Lh, where=K)
        assert np.all(logp[1] == -np.inf) and np.all(n_lab[1] == -1) and logp[0, 0] == -np.inf
        hyp, hl = rc.pack(hyps, K, Lh)
        assert np.array_equal(_raw(device, P, hyp, hl, want_nlab=False)[0], logp)
    gap.done()


def test_conventions(device):
    """skip, the blank's position, eps - 0 with exact zeros in P gives -inf where the labels need a zero and never NaN -, and
    out-of-range labels clipped as the loss clips them."""
    gap = Gap("conventions: skip, blank, eps, clipping")
    Cn, B, K = 6, 3, 6
    rng = np.random.default_rng(21)
    P = rng.dirichlet(np.full(Cn, 0.5), size=(B, 24)).astype(np.float32)
    for skip in (0, 1, 2, 5):
        for blank in (0, 3, Cn - 1):
            hyps = [[[c for c in h if c != blank] for h in row] for row in rc.random_hyps(rng, Cn, B, K, 6)]
            _against_ref(device, gap, P, hyps, K, 6, where=(skip, blank), skip=skip, blank=blank)
    _against_ref(device, gap, P, rc.random_hyps(rng, Cn - 1, B, K, 6), K, 6, where="eps", eps=1e-3)
    Pz = P.copy()
    Pz[:, :, 3] = 0.0
    Pz[1, 10, :] = [0, 0, 1, 0, 0, 0]                   # a one-hot frame
    Pz /= Pz.sum(axis=2, keepdims=True)
    hyps = [[[3], [0, 3, 1], [0, 1], [], [2], [1, 2, 4]] for _ in range(B)]
    logp, _ = _against_ref(device, gap, Pz, hyps, K, 6, where="eps 0", eps=0.0)
    assert not np.isnan(logp).any() and np.all(logp[:, :2] == -np.inf) and np.all(np.isfinite(logp[[0, 2], 2:]))
    assert logp[1, 3] == -np.inf                       # the empty hypothesis needs the blank at the one-hot frame
    clip = [[[7, -2, 100], [5, 0, 5], [-1], [6, 6], [2, -7, 3], [1]] for _ in range(B)]
    logp, n_lab = _against_ref(device, gap, P, clip, K, 6, where="clip")
    want = _raw(device, P, *rc.pack([[[5, 0, 5], [5, 0, 5], [0], [5, 5], [2, 0, 3], [1]] for _ in range(B)], K, 6))[0]
    assert np.array_equal(logp, want)
    gap.done()


def test_against_the_loss_and_the_aligner(device):
    """On the same inputs: minus mgr_ctc_loss_grad's loss, called once per hypothesis column, within REL; at least mgr_ctc_align's
    logp (one alignment against the sum over all)."""
    Cn, B, K, Lmax, T = 7, 4, 3, 8, 40
    rng = np.random.default_rng(31)
    P = rng.dirichlet(np.full(Cn, 0.4), size=(B, T)).astype(np.float32)
    il = np.array([38, 30, 9, 38], np.int32)
    hyps = rc.random_hyps(rng, Cn - 1, B, K, Lmax)
    hyps[0][0] = []
    hyps[2][1] = [1, 1, 1, 1, 1, 2]                    # does not fit 9 frames
    hyp, hl = rc.pack(hyps, K, Lmax)
    logp, _ = _raw(device, P, hyp, hl, il=il)
    dP, dil = device.array(P), device.array(il)
    ws = device.bytes(max(device.lib.mgr_ctc_ws_bytes(B, T, Cn, Lmax), device.lib.mgr_ctc_align_ws_bytes(B, T, Cn, Lmax)))
    dloss, dalp = device.empty((B,), np.float32), device.empty((B,), np.float64)
    dpath, dseg, dconf = device.empty((B, T - SKIP), np.int32), device.empty((B, Lmax, 2), np.int32), device.empty((B, Lmax), np.float32)
    g_loss = 0.0
    for k in range(K):
        dlab, dll = device.array(np.ascontiguousarray(hyp[:, k])), device.array(np.ascontiguousarray(hl[:, k]))
        device.call("mgr_ctc_loss_grad", dP, dlab, dil, dll, B, T, Cn, Lmax, SKIP, Cn - 1, C.c_float(EPS), C.c_float(1.0), dloss, None, ws,
                    ws.nbytes)
        loss = dloss.download().astype(np.float64)
        device.call("mgr_ctc_align", dP, dlab, dil, dll, B, T, Cn, Lmax, SKIP, Cn - 1, C.c_float(EPS), dpath, dseg, dconf, dalp, ws, ws.nbytes)
        alp = dalp.download()
        for b in range(B):
            if np.isinf(loss[b]):
                assert logp[b, k] == -np.inf and alp[b] == -np.inf
                continue
            g_loss = max(g_loss, abs(logp[b, k] + loss[b]) / abs(loss[b]))
            assert abs(logp[b, k] + loss[b]) <= REL * abs(loss[b]), (b, k, logp[b, k], loss[b])
            assert logp[b, k] >= alp[b] - REL * abs(alp[b]), (b, k, logp[b, k], alp[b])
        dlab.free()
        dll.free()
    assert logp[2, 1] == -np.inf
    for a in (dP, dil, ws, dloss, dalp, dpath, dseg, dconf):
        a.free()
    print("rescore parity: against -mgr_ctc_loss_grad (f32 loss)            largest gap %.3e" % g_loss)


def _beam_lm(device, P, il, beam, top_paths, eps):
    """mgr_ctc_beam_search_lm with zero tables; returns the DEVICE arrays out, out_len and the downloaded logp_ctc, plus what to free."""
    B, T, Cn = P.shape
    dP, dil = device.array(P), device.array(np.asarray(il, np.int32))
    ext = device.array(np.zeros((Cn + 1, Cn), np.float64))
    out, out_len = device.empty((B, top_paths, T - SKIP), np.int32), device.empty((B, top_paths), np.int32)
    score, lctc = device.empty((B, top_paths), np.float64), device.empty((B, top_paths), np.float64)
    ws = device.bytes(device.lib.mgr_ctc_beam_lm_ws_bytes(B, T, Cn, beam, top_paths))
    device.call("mgr_ctc_beam_search_lm", dP, dil, B, T, Cn, SKIP, Cn - 1, beam, C.c_float(eps), ext, None, top_paths, out, out_len, score, lctc,
                ws, ws.nbytes)
    return out, out_len, lctc.download(), [dP, dil, ext, out, out_len, score, lctc, ws]


def test_hypotheses_straight_from_the_beam_search(device):
    """The device outputs of mgr_ctc_beam_search_lm (top_paths = 4) feed the call unchanged.  A pruned search sees part of the
    alignments: the full sum is at least its logp_ctc.  At T - skip = 6, C = 3 the two are equal: label 1 has probability exactly 0 in
    the last three frames (eps = 0), so at most 31 prefixes have a non-zero probability before the last frame and the beam of 32 -
    the kernel's widest - holds every one of them; the last frame's candidates are computed from all of them before the final cut."""
    rng = np.random.default_rng(41)
    B, T, Cn = 5, 25, 6
    P = rng.dirichlet(np.full(Cn, 0.3), size=(B, T)).astype(np.float32)
    il = [23, 23, 12, 0, 23]
    out, out_len, lctc, held = _beam_lm(device, P, il, 8, 4, EPS)
    logp, n_lab = _raw(device, P, out, out_len, il=il)
    hl = out_len.download()
    for a in held:
        a.free()
    assert (hl >= 0).sum() >= 13 and np.array_equal(n_lab, hl)
    assert np.all(logp[hl < 0] == -np.inf) and np.all(np.isfinite(logp[hl >= 0]))
    assert np.all(logp[hl >= 0] >= lctc[hl >= 0] - REL * np.abs(lctc[hl >= 0]))
    assert logp[3, 0] == 0.0 and lctc[3, 0] == 0.0

    B, T, Cn = 6, 6 + SKIP, 3
    P = rng.dirichlet(np.full(Cn, 1.0), size=(B, T)).astype(np.float32)
    P[:, -3:, 1] = 0.0
    P /= P.sum(axis=2, keepdims=True)
    out, out_len, lctc, held = _beam_lm(device, P, [6] * B, 32, 4, 0.0)
    logp, _ = _raw(device, P, out, out_len, eps=0.0)
    hl, hyp = out_len.download(), out.download()
    for a in held:
        a.free()
    assert np.all(hl >= 0)
    g = np.abs(logp - lctc) / np.abs(lctc)
    print("rescore parity: against an exhaustive beam search's logp_ctc        largest gap %.3e" % g.max())
    assert g.max() <= REL, (logp, lctc)
    gap = Gap("beam hypotheses, T - skip = 6")
    gap.check(logp, rr.score_batch(P, hyp, hl, Cn - 1, SKIP, 0.0)[0])
    gap.done()


def _phrase_hyps(rng, G, B, K, max_phrases):
    return rc.random_hyps(rng, G, B, K, max_phrases, p_absent=0.1)


@pytest.mark.parametrize("which", ["reference", "shared"])
def test_lexicon_is_the_host_expansion_bit_for_bit(device, which):
    """Phrase hypotheses through the lexicon against the host-expanded word rows without one: the same bits.  A phrase id of G or -2
    makes that slot NaN and no other."""
    lexicon, Cn, To = (rc.reference_lexicon(), 44, 90) if which == "reference" else (rc.SHARED_LEXICON, 8, 60)
    G, B, K = len(lexicon), 3, 6
    rng = np.random.default_rng(51 + G)
    P = rng.dirichlet(np.full(Cn, 0.3), size=(B, To + SKIP)).astype(np.float32)
    hyps = _phrase_hyps(rng, G, B, K, 9)
    hyps[0][0] = [1, 1, 2, 2, 4, 4, 0, 3] if which == "shared" else [1, 1, 3, 3, 5, 6, 19, 7, 13]      # equal words meet across phrases
    gap = Gap("lexicon: %s" % which)
    logp, n_lab = _against_ref(device, gap, P, hyps, K, 9, lexicon=lexicon)
    words = [[None if h is None else rr.expand(h, lexicon) for h in row] for row in hyps]
    wl, wn = _raw(device, P, *rc.pack(words, K, max(len(w) for row in words for w in row if w is not None)))
    assert np.array_equal(logp, wl) and np.array_equal(n_lab, wn)
    assert np.isfinite(logp).sum() >= 10
    bad = [list(row) for row in hyps]
    bad[1][2], bad[2][0] = [0, G, 1], [-2]
    bl, bn = _against_ref(device, gap, P, bad, K, 9, lexicon=lexicon)
    assert np.isnan(bl[1, 2]) and np.isnan(bl[2, 0]) and bn[1, 2] == -1 and bn[2, 0] == -1
    keep = np.ones((B, K), bool)
    keep[1, 2] = keep[2, 0] = False
    assert np.array_equal(bl[keep], logp[keep]) and not np.isnan(bl[keep]).any()
    gap.done()


def test_lexicon_arrays_that_break_the_rules_are_refused(device):
    from mgr_amd._capi import MgrError
    P = np.full((1, 10, 5), 0.2, np.float32)
    hyp, hl = rc.pack([[[0]]], 1, 1)
    i32 = lambda *v: np.asarray(v, np.int32)
    for off, words, G, msg in ((i32(1, 2), i32(0, 1), 1, "phrase_off[0]"), (i32(0, 0), i32(0), 1, "is empty"), (i32(0, 1), i32(4), 1, "non-blank class"),
                               (i32(0, 1), i32(5), 1, "non-blank class"), (i32(0, 1), i32(-1), 1, "non-blank class"),
                               (i32(0, 256), np.zeros(256, np.int32), 1, "more than 255 words"), (i32(0, 1), i32(0), 65, "phrases out of")):
        with pytest.raises(MgrError, match=msg.replace("[", r"\[").replace("]", r"\]")):
            _raw(device, P, hyp, hl, lex_arrays=(off if G < 65 else np.arange(66, dtype=np.int32), words if G < 65 else np.zeros(65, np.int32), G))
    with pytest.raises(MgrError, match="too large"):
        _raw(device, np.full((1, 10, 65), 1 / 65, np.float32), hyp, hl, lex_arrays=(i32(0, 1), i32(0), 1))
    assert np.isfinite(_raw(device, P, hyp, hl, lex_arrays=(i32(0, 1), i32(0), 1))[0]).all()


def test_a_row_does_not_depend_on_the_batch(device):
    Cn, B, K, To = 9, 5, 6, 50
    rng = np.random.default_rng(61)
    P = rng.dirichlet(np.full(Cn, 0.4), size=(B, To + SKIP)).astype(np.float32)
    il = [50, 33, 7, 50, 16]
    hyps = rc.random_hyps(rng, Cn - 1, B, K, 12, p_absent=0.15)
    hyp, hl = rc.pack(hyps, K, 12)
    logp, n_lab = _raw(device, P, hyp, hl, il=il)
    for b in range(B):
        one, n1 = _raw(device, P[b:b + 1], hyp[b:b + 1], hl[b:b + 1], il=il[b:b + 1])
        assert np.array_equal(one[0], logp[b], equal_nan=True) and np.array_equal(n1[0], n_lab[b])


def test_full_length(device):
    """The audio network's frames: T = 1900, C = 44, hypotheses of 150 words through the reference lexicon."""
    lexicon = rc.reference_lexicon()
    B, K, T, Cn = 2, 4, 1900, 44
    rng = np.random.default_rng(71)
    P = rng.dirichlet(np.full(Cn, 0.3), size=(B, T)).astype(np.float32)
    hyps = []
    for b in range(B):
        row = []
        for k in range(K):
            h = []
            while len(rr.expand(h, lexicon)) < 150:
                h.append(int(rng.integers(0, len(lexicon))))
            while len(rr.expand(h, lexicon)) > 150:
                h.pop()
            while len(rr.expand(h, lexicon)) < 150:
                h.append(0)            # (a one-word phrase)
            row.append(h)
        hyps.append(row)
    gap = Gap("full length: T = 1900, 150 words")
    logp, n_lab = _against_ref(device, gap, P, hyps, K, T - SKIP, lexicon=lexicon, il=[1898, 1500])
    assert np.all(n_lab == 150) and np.all(np.isfinite(logp))
    gap.done()


def test_ranking_end_to_end(device):
    """rescore_nbest on the planted two-stream cases (T = 40 / 23, C = 22 / 44 with the lexicon): the returned order is the
    restatement's on every sample - no allowance: tests/test_cpu_rescore.py has shown the margins -, the truth comes first although each
    stream alone prefers a wrong hypothesis on one sample, and what the bigram forbids comes last."""
    from mgr_amd import decoding
    gap = Gap("ranking cases: parts")
    for case in rc.ranking_cases():
        streams = [(s["P"], {"lexicon": s["lexicon"], "skip": SKIP, "eps": EPS}) for s in case["streams"]]
        ranked, total, parts, order = decoding.rescore_nbest(streams, case["paths"], case["weights"], case["lm"], case["lm_end"],
                                                              case["alpha"], case["beta"], dev=device)
        worder, wtotal, wparts = rc.reference_ranking(case)
        assert np.array_equal(order, worder), case["name"]
        gap.check(parts, np.take_along_axis(wparts, worder[:, :, None], axis=1), case["name"])
        gap.check(total, wtotal, case["name"])
        for b, hyps in enumerate(case["paths"]):
            t = case["truth"][b]
            assert ranked[b] == [hyps[k] for k in order[b]]
            if rr.lm_term(hyps[t], case["lm"], case["lm_end"]) == -np.inf:
                assert total[b, list(order[b]).index(t)] == -np.inf and list(order[b]).index(t) >= np.isfinite(total[b]).sum()
            else:
                assert order[b, 0] == t
            for m, wb in enumerate(case["wrong"]):
                alone = int(order[b, np.nanargmax(parts[b, :, m])])
                assert alone == (case["sub"][b] if b == wb else t)
        # the shapes mbr_decode and nbest_attainable take
        picks, ranks, _ = decoding.mbr_decode(ranked, total, dev=device)
        dist, rank, _ = decoding.nbest_attainable(ranked, [hyps[t] for hyps, t in zip(case["paths"], case["truth"])], dev=device)
        assert len(picks) == len(ranked) and np.all(dist == 0) and np.all(ranks >= 0)
        assert np.all(rank[[b for b in range(len(ranked)) if order[b, 0] == case["truth"][b]]] == 0)
    gap.done()


def test_ctc_scores_takes_lists_and_arrays(device):
    from mgr_amd import decoding
    rng = np.random.default_rng(81)
    P = rng.dirichlet(np.full(6, 0.5), size=(3, 20)).astype(np.float32)
    paths = [[[1, 2], [0]], [[]], [[4, 4, 1], [2], [3]]]
    a = decoding.ctc_scores(P, paths, dev=device)
    b, n = decoding.ctc_scores(P, decoding.pack_nbest(paths, K=3, width=18), dev=device, return_counts=True)
    assert a.dtype == np.float64 and a.shape == (3, 3) and np.array_equal(a, b)
    assert n.tolist() == [[2, 1, -1], [0, -1, -1], [3, 1, 1]]
    gap = Gap("ctc_scores")
    gap.check(a, rr.score_paths(P, paths, 5, 3))
    gap.check(decoding.ctc_scores(P, paths, input_length=[5, 0, 18], skip=1, dev=device), rr.score_paths(P, paths, 5, 3, 1, EPS, [5, 0, 18]))
    gap.done()


def test_facade_rescore_generator(device):
    """Model.rescore_generator over 3 batches with a short last one - on a fresh model, so on an inference-only engine - equals
    ctc_scores of predict_generator's posteriors bit for bit, through the lexicon and without; pipelined equals one batch at a time;
    predict_generator has no hypotheses to give and keeps refusing decode="rescore"."""
    from mgr_amd import decoding, keras_like as K
    from mgr_amd.audio_network.sequence_decoding import GESTURE_LEXICON
    from mgr_amd.configs import audio_spec
    from mgr_amd.keras_like import Model
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    K.set_learning_phase(0)
    decoding._DEV[0] = device
    spec = audio_spec(h=16)
    B, T = 4, 40
    data = [synthetic_arrays(spec, B, T, 4, 700 + i, lmin=2, lmax=4)[0] for i in range(3)]
    data[-1] = {k: v[:2] for k, v in data[-1].items()}
    N = 2 * B + 2
    rng = np.random.default_rng(91)
    phrases = [[h for h in row if h is not None] for row in rc.random_hyps(rng, len(GESTURE_LEXICON), N, 5, 4, p_absent=0.3)]
    phrases[0] = [[5], [6, 7], [1, 1], [], [10, 15, 1]]
    words = [[h for h in row if h is not None] for row in rc.random_hyps(rng, 43, N, 3, 6, p_absent=0.2)]
    m = Model(spec, device=device)
    m.set_weights_dict(synthetic_weights(spec, 17))
    got, counts = m.rescore_generator(iter(data), 3, phrases, lexicon=GESTURE_LEXICON, return_counts=True)
    assert m._engine.inference_only
    P = m.predict_generator(iter(data), steps=3)
    eps = float(spec.ctc["eps"])
    want, wcounts = decoding.ctc_scores(P, phrases, lexicon=GESTURE_LEXICON, dev=device, eps=eps, return_counts=True)
    assert got.dtype == np.float64 and got.shape == (N, 5) and np.array_equal(got, want) and np.array_equal(counts, wcounts)
    assert np.isfinite(got).sum() >= N
    gap = Gap("facade: rescore_generator")
    gap.check(got, rr.score_paths(P, phrases, 43, 5, SKIP, eps, None, GESTURE_LEXICON))
    gap.done()
    arrays = decoding.pack_nbest(words, K=4, width=9)
    assert np.array_equal(m.rescore_generator(iter(data), 3, arrays), decoding.ctc_scores(P, arrays, dev=device, eps=eps))
    e = m._engine
    full = [(d,) + tuple(a[i * B:(i + 1) * B] for a in arrays) for i, d in enumerate(data[:2])]
    pipe = list(e.predict_stream(iter(full), output="rescore"))
    single = [list(e.predict_stream([f], output="rescore"))[0] for f in full]
    for a, b in zip(pipe, single):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert list(e.predict_stream(iter([]), output="rescore")) == []
    with pytest.raises(ValueError):
        list(e.predict_stream([(full[0][0], arrays[0][:B - 1], arrays[1][:B - 1])], output="rescore"))
    with pytest.raises(KeyError):
        m.predict_generator(iter(data), steps=3, decode="rescore")
    assert np.array_equal(P, m.predict_generator(iter(data), steps=3))          # the other modes are as they were


def test_decode_rescoring_writes_the_predicted_mlf(device, tmp_path):
    """multimodal_fusion.rescoring.decode_rescoring on a planted two-stream case: the pool is the skeletal 4-best plus the audio
    lexicon 1-best, and the MLF holds, per sample, the names of the hypothesis the restatement ranks first on that pool (its margin
    is asserted first); a file number of the ignore list is left out; scores computed elsewhere give the same file."""
    from mgr_amd import decoding
    from mgr_amd.multimodal_fusion import rescoring
    from mgr_amd.multimodal_fusion.sequence_decoding import map_gest
    decoding._DEV[0] = device
    case = next(iter(rc.ranking_cases()))
    sk, au = case["streams"][0]["P"], case["streams"][1]["P"]
    lex = case["streams"][1]["lexicon"]
    f_list = [1, 228, 3]
    names, (ranked, total, parts) = rescoring.decode_rescoring(sk, au, f_list, top_paths=4, beam_width=8, weights=(1.0, 0.8),
                                                               out_file=str(tmp_path / "r.mlf"))
    pool = [sorted(r) for r in ranked]
    K = total.shape[1]
    assert all(4 <= len(p) <= 5 for p in pool) and parts.shape == (3, K, 2)
    wparts = np.stack([rr.score_paths(sk, pool, 21, K), rr.score_paths(au, pool, 43, K, lexicon=lex)], axis=2)
    worder, wtotal = rr.combine(wparts, pool, (1.0, 0.8))
    assert np.all(wtotal[:, 0] - wtotal[:, 1] >= rc.MARGIN * np.abs(wtotal[:, 0]))
    best = [pool[b][worder[b, 0]] for b in range(3)]
    assert [r[0] for r in ranked] == best == [case["paths"][b][case["truth"][b]] for b in range(3)]
    assert names == [[map_gest[g] for g in h] for h in best]
    gap = Gap("decode_rescoring: totals")
    gap.check(total[:, 0], wtotal[:, 0])
    gap.done()
    assert decoding.read_mlf(str(tmp_path / "r.mlf")) == {"Sample00001": names[0], "Sample00003": names[2]}
    want = "#!MLF!#\n" + "".join('"*/Sample%05d.rec"\n%s.\n' % (f, "".join(n + "\n" for n in names[b])) for b, f in enumerate(f_list) if f != 228)
    assert open(tmp_path / "r.mlf").read() == want
    # the same from scores computed elsewhere, for the same pool
    upool = [list(r) for r in ranked]
    s_sk, s_au = decoding.ctc_scores(sk, upool, dev=device), decoding.ctc_scores(au, upool, lexicon=lex, dev=device)
    names2, (ranked2, total2, _) = rescoring.decode_rescoring(s_sk, s_au, f_list, weights=(1.0, 0.8), out_file=str(tmp_path / "r2.mlf"),
                                                              paths=upool)
    assert names2 == names and ranked2 == ranked and np.array_equal(total2, total)
    assert open(tmp_path / "r2.mlf").read() == want
    with pytest.raises(ValueError):
        rescoring.decode_rescoring(s_sk, au, f_list, out_file=None)
