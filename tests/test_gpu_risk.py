"""-m gpu: mgr_ctc_risk_grad - the expected risk over an N-best list and its gradient w.r.t. the Dense logits, K hypotheses per
sample in one call - against the fp64 restatement of tests/risk_ref.py at the smallest shapes at which it can go wrong, against the
K-call composition of mgr_ctc_loss_grad and mgr_ctc_rescore it replaces, through the lexicon, and through decoding.expected_risk."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_ref as er  # noqa: E402
import rescore_cases as rc  # noqa: E402
import rescore_ref as rr  # noqa: E402
import risk_cases as kc  # noqa: E402
import risk_ref as kr  # noqa: E402

pytestmark = pytest.mark.gpu

EPS, REL = kc.EPS, kc.REL
_host = lambda a: None if a is None else a.ctypes.data


def _raw(device, P, hyp, hl, risks, il=None, skip=2, eps=EPS, lexicon=None, lex_arrays=None, Lcap=None, risk_scale=1.0, post_scale=1.0,
         gscale=1.0, onto=None, grad=True, want_weight=True, K=None):
    """mgr_ctc_risk_grad through the C ABI.  onto: a host buffer (B, T, C) the gradient is ACCUMULATED onto.  Returns dict(logp,
    weight, risk, dlogits)."""
    from mgr_amd import decoding
    P = np.ascontiguousarray(P, np.float32)
    B, T, Cn = P.shape
    hyp, hl = np.ascontiguousarray(hyp, np.int32), np.ascontiguousarray(hl, np.int32)
    K, Lh = hl.shape[1] if K is None else K, hyp.shape[2]
    off = words = None
    G = 0
    if lex_arrays is not None:
        off, words, G = lex_arrays
    elif lexicon is not None:
        off, words = decoding.compile_lexicon(lexicon, Cn)
        G = len(off) - 1
    Lcap = decoding.risk_label_cap(hyp, hl, off) if Lcap is None else Lcap
    il = np.full(B, T - skip, np.int32) if il is None else np.asarray(il, np.int32)
    own = [device.array(P), device.array(il), device.array(hyp), device.array(hl), device.array(np.ascontiguousarray(risks, np.int32)),
           device.empty((B, hl.shape[1]), np.float64), device.empty((B, hl.shape[1]), np.float32), device.empty((B,), np.float32)]
    dg = None
    if grad:
        dg = device.array(np.ascontiguousarray(onto, np.float32)) if onto is not None else device.empty((B, T, Cn), np.float32)
        own.append(dg)
    try:
        ws = device.bytes(device.lib.mgr_ctc_risk_ws_bytes(B, T, Cn, K, Lcap, G, _host(off)))
        own.append(ws)
        device.call("mgr_ctc_risk_grad", own[0], own[1], B, T, Cn, skip, Cn - 1, C.c_float(eps), _host(off), _host(words), G, own[2], own[3],
                    K, Lh, Lcap, own[4], C.c_float(risk_scale), C.c_float(post_scale), C.c_float(gscale), 1 if onto is not None else 0,
                    own[5], own[6] if want_weight else None, own[7], dg, ws, ws.nbytes)
        return {"logp": own[5].download(), "weight": own[6].download() if want_weight else None, "risk": own[7].download(),
                "dlogits": dg.download() if grad else None}
    finally:
        for a in own:
            a.free()


def _ref(P, hyp, hl, risks, **kw):
    return kr.expected_risk(P, hyp, hl, risks, skip=kw.get("skip", 2), eps=kw.get("eps", EPS), input_len=kw.get("il"),
                            lexicon=kw.get("lexicon"), Lcap=kw.get("Lcap") or rr.MAX_LABELS, risk_scale=kw.get("risk_scale", 1.0),
                            post_scale=kw.get("post_scale", 1.0), gscale=kw.get("gscale", 1.0))


def _compare(got, want, where):
    """logp: NaN where NaN, -inf where -inf, within REL relative where finite (K14's bound); weight and exp_risk within REL (of 1 and
    of the largest risk in play); dLogits within REL of the restatement's largest entry; exact zeros where the restatement has a whole
    zero frame (skipped, behind the input length, fewer than two live slots).  Returns the measured gradient gap."""
    gl, wl = got["logp"], want["logp"]
    assert np.array_equal(np.isnan(gl), np.isnan(wl)) and np.array_equal(gl == -np.inf, wl == -np.inf), (where, gl, wl)
    fin = np.isfinite(wl)
    if fin.any():
        rel = np.where(wl[fin] == 0, np.abs(gl[fin]), np.abs(gl[fin] - wl[fin]) / np.maximum(np.abs(wl[fin]), 1e-300))
        assert rel.max() <= REL, (where, gl, wl)
    if got["weight"] is not None:
        assert np.abs(got["weight"] - want["weight"]).max() <= REL, (where, got["weight"], want["weight"])
    assert np.abs(got["risk"] - want["risk"]).max() <= REL * max(1.0, np.abs(want["risk"]).max()), (where, got["risk"], want["risk"])
    top = np.abs(want["dlogits"]).max()
    gap = np.abs(got["dlogits"] - want["dlogits"]).max()
    assert gap <= REL * top, (where, gap, top)
    trivial = want["live"].sum(axis=1) < 2
    assert np.all(got["dlogits"][trivial] == 0), where
    zero_frames = np.all(want["dlogits"] == 0, axis=2) & ~np.all(want["g"] == 0, axis=1)[:, None]      # skipped / out-of-length frames
    assert np.all(got["dlogits"][zero_frames] == 0), where
    return gap / top if top > 0 else 0.0


@pytest.mark.parametrize("idx", range(len(kc.random_cases())))
def test_random_cases_against_the_restatement(device, idx):
    """Frame counts at the chunk and renormalisation edges, skip 0 and 2, C 4 / 22 / 64, K 3 .. 32, ragged input lengths, rows as wide
    as the input; the same call twice gives the same bits; accumulate = 1 onto a random buffer adds to one f32 rounding."""
    case = kc.random_cases()[idx]
    kw = dict(il=case["il"], skip=case["skip"], post_scale=case["post_scale"], risk_scale=case["risk_scale"], gscale=0.5)
    got = _raw(device, case["P"], case["hyp"], case["hl"], case["risks"], **kw)
    want = _ref(case["P"], case["hyp"], case["hl"], case["risks"], **kw)
    assert kc.informative(case, want["logp"]) >= 0.9
    gap = _compare(got, want, case["name"])
    print("risk parity: %-44s gradient gap / largest entry %.3e" % (case["name"], gap))
    again = _raw(device, case["P"], case["hyp"], case["hl"], case["risks"], **kw)
    for key in ("logp", "weight", "risk", "dlogits"):
        assert np.array_equal(got[key], again[key], equal_nan=True), key
    X = np.random.default_rng(idx).standard_normal(got["dlogits"].shape).astype(np.float32)
    acc = _raw(device, case["P"], case["hyp"], case["hl"], case["risks"], onto=X, **kw)["dlogits"]
    assert np.array_equal(acc, X + got["dlogits"])           # (one f32 addition of the same f32 value)


@pytest.mark.parametrize("L", kc.WIDTH_EDGES + (200,))
def test_every_lattice_width(device, L):
    """Expanded lengths at every pairs-per-lane switch, narrow and wide hypotheses in one sample (a wave picks its width from its own
    hypothesis), repeated labels that force blanks, Lcap exactly the longest hypothesis."""
    Cn, B, K = 5, 2, 4
    rng = np.random.default_rng(L)
    lab = lambda n: [int(v) for v in rng.integers(0, Cn - 1, n)]
    hyps = [[lab(L), lab(min(3, max(L, 1))), lab(L), lab(max(L - 1, 0))] for _ in range(B)]
    if L >= 3:
        hyps[0][2][1] = hyps[0][2][0]          # a repeat
    To = max(rr.needs(h) for row in hyps for h in row) + 3
    P = rng.dirichlet(np.full(Cn, 0.5), size=(B, To + 2)).astype(np.float32)
    hyp, hl = rc.pack(hyps, K, max(L, 1))
    risks = np.array([[0, 3, 1, 2]] * B, np.int32)
    # (long label sequences over random posteriors differ by many nats: a flat posterior scale keeps more than one slot in play)
    kw = dict(post_scale=0.05 if L > 3 else 1.0, Lcap=max(L, 1))
    want = _ref(P, hyp, hl, risks, **kw)
    assert np.all(want["live"]) and np.abs(want["dlogits"]).max() > 1e-4
    _compare(_raw(device, P, hyp, hl, risks, **kw), want, L)


def test_one_slot_per_sample(device):
    """K = 1: a grid of (1, B) workgroups whose second hypothesis' waves have nothing to run, and a prologue with at most one live slot
    - weight 1, exp_risk = r_0 risk_scale, the gradient exactly zero, a buffer accumulated onto left as it was; the same bits twice
    and for a sample alone."""
    Cn, B = 22, 4
    rng = np.random.default_rng(1)
    P = rng.dirichlet(np.full(Cn, 0.5), size=(B, 19)).astype(np.float32)
    hyp, hl = rc.pack([[[3, 3, 7]], [[]], [None], [[1, 2, 3, 4, 5, 6, 7, 8, 9]]], 1, 9)       # the last needs 9 of its 8 frames
    risks = np.array([[3], [5], [2], [4]], np.int32)
    kw = dict(il=[17, 17, 17, 8], risk_scale=0.5, post_scale=0.7, gscale=0.5)
    got = _raw(device, P, hyp, hl, risks, **kw)
    want = _ref(P, hyp, hl, risks, **kw)
    _compare(got, want, "K = 1")
    assert got["weight"].tolist() == [[1.0], [1.0], [0.0], [0.0]] and got["risk"].tolist() == [1.5, 2.5, 0.0, 0.0]
    assert np.all(got["dlogits"] == 0) and got["logp"][2, 0] == -np.inf and got["logp"][3, 0] == -np.inf
    again = _raw(device, P, hyp, hl, risks, **kw)
    for key in ("logp", "weight", "risk", "dlogits"):
        assert np.array_equal(got[key], again[key]), key
    X = rng.standard_normal(got["dlogits"].shape).astype(np.float32)
    assert np.array_equal(_raw(device, P, hyp, hl, risks, onto=X, **kw)["dlogits"], X)
    full = _raw(device, P, hyp, hl, risks, **dict(kw, Lcap=9))
    for b in range(B):
        one = _raw(device, P[b:b + 1], hyp[b:b + 1], hl[b:b + 1], risks[b:b + 1], **dict(kw, il=kw["il"][b:b + 1], Lcap=9))
        for key in ("logp", "weight", "risk", "dlogits"):
            assert np.array_equal(one[key][0], full[key][b]), (b, key)


def test_slot_kinds(device):
    """Absent slots, infeasible slots, a slot longer than Lcap, a sample without any slot, one live slot, equal risks everywhere,
    input_len 0 and shorter than T; weight NULL and dLogits NULL."""
    Cn, K = 6, 5
    rng = np.random.default_rng(7)
    P = rng.dirichlet(np.full(Cn, 0.5), size=(7, 20)).astype(np.float32)
    hyps = [[None, [1, 2], [0], None, [3, 3]],                       # absent first and in the middle
            [[1, 1, 1, 1, 1, 1, 1, 1, 1, 1], [2], [0, 1], [], [4]],  # [1] * 10 needs 19 frames: infeasible
            [[0, 1, 2, 3, 4], [1], [2, 2], [0], [3]],                # five labels: longer than Lcap = 4
            [None] * K,                                              # no slot at all
            [None, [2, 1], None, None, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]],   # one live slot
            [[0], [1], [2], [3], [4]],                               # equal risks (below)
            [[0], [1], [], [2, 2], [1, 0]]]                          # input_len 0: only the empty hypothesis fits
    hyp, hl = rc.pack(hyps, K, 10)
    risks = np.array([[1, 0, 2, 9, 3], [0, 1, 2, 3, 4], [0, 2, 1, 1, 0], [1, 2, 3, 4, 5], [7, 3, 1, 1, 0], [2, 2, 2, 2, 2], [1, 0, 3, 2, 2]], np.int32)
    il = [18, 18, 18, 18, 18, 11, 0]
    # samples 1 and 4 hold ten labels: with Lcap = 4 they are "not scored" (NaN), with Lcap = 10 infeasible (-inf): both kinds are run
    for kw in (dict(il=il, Lcap=4), dict(il=il, Lcap=10)):
        got = _raw(device, P, hyp, hl, risks, **kw)
        want = _ref(P, hyp, hl, risks, **kw)
        _compare(got, want, kw["Lcap"])
        assert np.isnan(got["logp"][2, 0]) == (kw["Lcap"] == 4) and np.isnan(got["logp"][1, 0]) == (kw["Lcap"] == 4)
        assert np.all(got["dlogits"][[3, 4, 6]] == 0) and got["risk"][3] == 0 and got["risk"][4] == 3 and np.all(got["weight"][3] == 0)
        assert np.abs(got["dlogits"][5]).max() <= 1e-6 and abs(got["risk"][5] - 2) <= 1e-6          # equal risks: g = a w (r - Rbar) ~ 0
        assert np.all(got["dlogits"][5, 13:] == 0) and np.all(got["dlogits"][:, :2] == 0)
        assert got["weight"][6].tolist() == [0, 0, 1, 0, 0] and got["logp"][6, 2] == 0.0
    bare = _raw(device, P, hyp, hl, risks, grad=False, want_weight=False, **kw)
    assert np.array_equal(bare["logp"], got["logp"], equal_nan=True) and np.array_equal(bare["risk"], got["risk"])


def test_lexicon(device):
    """Phrase ids through the lexicon - an id outside [0, G) is not scored - give the bits of the call on the expanded words."""
    lex = rc.SHARED_LEXICON
    Cn, K, B = 8, 4, 3
    rng = np.random.default_rng(17)
    P = rng.dirichlet(np.full(Cn, 0.5), size=(B, 30)).astype(np.float32)
    phr = [[[0, 2], [1], [4, 4, 0], [3, 5]], [[2, 2], [6, 1], [0], []], [[5], [1, 0], [-1], None]]      # ids 6 and -1: outside the lexicon
    hyp, hl = rc.pack(phr, K, 3)
    risks = np.array([[2, 0, 3, 1], [1, 5, 0, 2], [0, 1, 4, 4]], np.int32)
    kw = dict(post_scale=0.3)
    got = _raw(device, P, hyp, hl, risks, lexicon=lex, **kw)
    want = _ref(P, hyp, hl, risks, lexicon=lex, **kw)
    _compare(got, want, "lexicon")
    assert np.isnan(got["logp"][1, 1]) and np.isnan(got["logp"][2, 2]) and got["weight"][1, 1] == 0
    # the same slots as words: the bad-id slots become absent ones with the same (zero) weight
    words = [[None if h is None or rr.expand(h, lex) is None else rr.expand(h, lex) for h in row] for row in phr]
    whyp, whl = rc.pack(words, K, 12)
    plain = _raw(device, P, whyp, whl, risks, **kw)
    assert np.array_equal(plain["dlogits"], got["dlogits"]) and np.array_equal(plain["risk"], got["risk"])
    assert np.array_equal(plain["weight"], got["weight"])
    assert np.array_equal(plain["logp"][np.isfinite(got["logp"])], got["logp"][np.isfinite(got["logp"])])


def test_a_sample_does_not_depend_on_its_batch(device):
    case = kc.random_case(300, 5, 33, 22, 5)
    full = _raw(device, case["P"], case["hyp"], case["hl"], case["risks"], Lcap=case["Lcap"])
    for b in (0, 3):
        one = _raw(device, case["P"][b:b + 1], case["hyp"][b:b + 1], case["hl"][b:b + 1], case["risks"][b:b + 1], Lcap=case["Lcap"])
        for key in ("logp", "weight", "risk", "dlogits"):
            assert np.array_equal(one[key][0], full[key][b]), (b, key)


def _composition(device, P, hyp, hl, risks, il=None, skip=2, eps=EPS, post_scale=1.0, risk_scale=1.0, gscale=1.0):
    """What the library offered before this call: mgr_ctc_rescore for logp, K calls of mgr_ctc_loss_grad (one label column each) for
    the per-hypothesis gradients, weights and combination on the host in fp64.  Returns (logp, dlogits float64)."""
    P = np.ascontiguousarray(P, np.float32)
    B, T, Cn = P.shape
    K, Lh = hl.shape[1], hyp.shape[2]
    il = np.full(B, T - skip, np.int32) if il is None else np.asarray(il, np.int32)
    dP, dil, dh, dl = device.array(P), device.array(il), device.array(hyp), device.array(hl)
    dlogp = device.empty((B, K), np.float64)
    ws = device.bytes(max(device.lib.mgr_ctc_rescore_ws_bytes(B, T, Cn, 0, None), device.lib.mgr_ctc_ws_bytes(B, T, Cn, Lh)))
    dloss, dg = device.empty((B,), np.float32), device.empty((B, T, Cn), np.float32)
    held = [dP, dil, dh, dl, dlogp, ws, dloss, dg]
    try:
        device.call("mgr_ctc_rescore", dP, dil, B, T, Cn, skip, Cn - 1, C.c_float(eps), None, None, 0, dh, dl, K, Lh, dlogp, None, ws, ws.nbytes)
        logp = dlogp.download()
        g = np.stack([kr.weights(logp[b], risks[b], risk_scale, post_scale)[2] for b in range(B)])
        total = np.zeros((B, T, Cn))
        for k in range(K):
            dlab, dll = device.array(np.ascontiguousarray(hyp[:, k])), device.array(np.ascontiguousarray(np.maximum(hl[:, k], 0)))
            held += [dlab, dll]
            device.call("mgr_ctc_loss_grad", dP, dlab, dil, dll, B, T, Cn, Lh, skip, Cn - 1, C.c_float(eps), C.c_float(1.0), dloss, dg, ws,
                        ws.nbytes)
            total -= gscale * g[:, k, None, None] * dg.download().astype(np.float64)
        return logp, total
    finally:
        for a in held:
            a.free()


def test_against_the_composition_it_replaces(device):
    case = kc.random_case(310, 4, 33, 22, 4, max_len=6)
    got = _raw(device, case["P"], case["hyp"], case["hl"], case["risks"])
    logp, comp = _composition(device, case["P"], case["hyp"], case["hl"], case["risks"])
    assert np.array_equal(logp, got["logp"])                 # (the alpha recursion is mgr_ctc_rescore's)
    top = np.abs(comp).max()
    assert top > 1e-4 and np.abs(got["dlogits"] - comp).max() <= REL * top


def test_decoding_expected_risk_with_references(device):
    """decoding.expected_risk(refs=...): the risks are mgr_edit_distance's - pair (b K + k) against reference b, ignored labels dropped
    from both sides, an absent slot the empty hypothesis - and everything else the restatement fed with those distances."""
    from mgr_amd import decoding
    case = kc.random_case(320, 4, 24, 22, 4, p_absent=0.15)
    rng = np.random.default_rng(321)
    refs = [[int(v) for v in rng.integers(0, 21, int(rng.integers(1, 5)))] for _ in range(4)]
    refs[1] = list(case["hyp"][1, 0, :max(case["hl"][1, 0], 0)])         # one list holds its truth
    costs, ignore = (3, 2, 2), (0,)
    mask = 1
    want_r = np.array([[er.align(er.filter_row(case["hyp"][b, k], case["hl"][b, k], mask), er.filter_row(refs[b], None, mask), costs)[0]
                        for k in range(4)] for b in range(4)], np.int32)
    paths = [[[int(v) for v in case["hyp"][b, k, :case["hl"][b, k]]] for k in range(4) if case["hl"][b, k] >= 0] for b in range(4)]
    for hyps in ((case["hyp"], case["hl"]), paths):
        risk, w, logp, risks, dl = decoding.expected_risk(case["P"], hyps, refs=refs, costs=costs, ignore=ignore, risk_scale=0.5,
                                                          post_scale=0.7, dev=device)
        if isinstance(hyps, tuple):
            assert np.array_equal(risks, want_r)
            want = _ref(case["P"], case["hyp"], case["hl"], want_r, risk_scale=0.5, post_scale=0.7)
            _compare({"logp": logp, "weight": w, "risk": risk, "dlogits": dl}, want, "refs")
            first = (risk, dl)
        else:       # lists: absent slots are packed behind the present ones - the same sums
            assert np.abs(risk - first[0]).max() <= 1e-6 and np.abs(dl - first[1]).max() <= 1e-6 * max(1.0, np.abs(first[1]).max())
    r2 = decoding.expected_risk(case["P"], (case["hyp"], case["hl"]), risks=want_r, risk_scale=0.5, post_scale=0.7, grad=False, dev=device)
    assert len(r2) == 4 and np.array_equal(r2[0], first[0])
    with pytest.raises(ValueError):
        decoding.expected_risk(case["P"], paths, dev=device)
    with pytest.raises(ValueError):
        decoding.expected_risk(case["P"], paths, refs=refs, risks=want_r, dev=device)


def test_argument_errors_are_reported(device):
    from mgr_amd._capi import MgrError
    case = kc.random_case(330, 2, 8, 4, 3)
    for bad in (dict(K=33), dict(Lcap=256), dict(Lcap=0), dict(post_scale=0.0), dict(post_scale=float("nan"))):
        with pytest.raises(MgrError):
            _raw(device, case["P"], case["hyp"], case["hl"], case["risks"], **bad)


def test_the_long_case_against_fp64_and_the_composition(device):
    """T = 1900, K = 8, B = 2, C = 22: the error of logp feeds the weights through exp, so no bound is fixed in advance - the call's
    gradient error against fp64 may be at most the larger of REL of the largest entry and twice the error of the K-call composition
    (the same f32 recursions in another summation order).  Both figures are printed: profiles/risk_parity.txt records them.
    Measured on an MI355X: the call 5.6e-5, the composition 5.5e-5 of the largest entry."""
    B, T, Cn, K = 2, 1900, 22, 8
    rng = np.random.default_rng(1900)
    truth = [[int(v) for v in rng.integers(0, Cn - 1, 18)] for _ in range(B)]
    P = np.stack([rc._planted(T - 2, t, Cn - 1, Cn, 0.6) for t in truth])
    hyps = []
    for b in range(B):
        row = [list(truth[b])]
        for k in range(1, K):          # substitutions, deletions and insertions of the truth: hypotheses a beam would return together
            h = list(truth[b])
            i = int(rng.integers(0, len(h)))
            if k % 3 == 0:
                h[i] = (h[i] + 1 + int(rng.integers(0, Cn - 2))) % (Cn - 1)
            elif k % 3 == 1:
                del h[i]
            else:
                h.insert(i, int(rng.integers(0, Cn - 1)))
            row.append(h)
        hyps.append(row)
    hyp, hl = rc.pack(hyps, K, 20)
    risks = np.array([[er.align(h, truth[b], (1, 1, 1))[0] for h in hyps[b]] for b in range(B)], np.int32)
    kw = dict(post_scale=0.02)           # (hypotheses one edit apart differ by tens of nats at this length)
    want = _ref(P, hyp, hl, risks, **kw)
    top = np.abs(want["dlogits"]).max()
    assert np.all(want["live"]) and top > 1e-6 and (want["weight"] > 0.01).sum() >= 3 * B
    got = _raw(device, P, hyp, hl, risks, **kw)
    _, comp = _composition(device, P, hyp, hl, risks, **kw)
    e_call, e_comp = np.abs(got["dlogits"] - want["dlogits"]).max() / top, np.abs(comp - want["dlogits"]).max() / top
    print("risk parity: T 1900 K 8 B 2 C 22   gradient error / largest entry: the call %.3e   the K-call composition %.3e" % (e_call, e_comp))
    assert e_call <= max(REL, 2 * e_comp), (e_call, e_comp)
