"""-m gpu: mgr_edit_distance (csrc/edit.hip) against tests/edit_ref.py with == on every output, its input conventions,
independence and refusals; decoding.nbest_attainable / mbr_decode against their fp64 restatements; Model.score_generator and
fit_generator(val_score=...) against the two-pass route they replace.

Every call here goes through run_edit, which puts guard words behind every output and a page of sentinel bytes behind the workspace
and checks them after the call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_ref as er  # noqa: E402
from test_cpu_edit import ASYM, MBR_SCALES, NBEST_SHAPE, nbest_case  # noqa: E402

pytestmark = pytest.mark.gpu

COSTS = er.COST_SETS + [ASYM]
REF_LENS = [0, 1, 15, 16, 63, 64, 65, 150, 257]      # lane and chunk boundaries of the column split
HYP_LENS = [0, 1, 2, 64, 65, 300]
GUARD = 16
SENTINEL = 0x5A


def run_edit(device, hyp, hyp_len, ref, ref_len, pair_h, pair_r, costs, mask=0, want_ops=True, ws_bytes=None, n_pairs=None):
    """The C call itself on host arrays: (dist, counts, lens, n_ops, ops), the last two None without want_ops."""
    hyp, ref = np.ascontiguousarray(hyp, np.int32), np.ascontiguousarray(ref, np.int32)
    (n_hyp, Lh), (n_ref, Lr) = hyp.shape, ref.shape
    P = n_pairs if n_pairs is not None else (n_hyp if pair_h is None else len(pair_h))
    opt = lambda a: None if a is None else device.array(np.ascontiguousarray(a, np.int32))
    ins = [device.array(hyp), opt(hyp_len), device.array(ref), opt(ref_len), opt(pair_h), opt(pair_r)]
    shapes = [((P,), np.int32), ((P, 4), np.int32), ((P, 2), np.int32)] + ([((P,), np.int32), ((P, Lh + Lr), np.int8)] if want_ops else [])
    outs = []
    for shp, dt in shapes:      # every output with GUARD words of a sentinel behind it
        n = int(np.prod(shp))
        outs.append(device.array(np.full(n + GUARD, SENTINEL, dt)))
    need = device.lib.mgr_edit_distance_ws_bytes(P, Lh, Lr, 1 if want_ops else 0)
    assert need == 0 or want_ops
    nws = need if ws_bytes is None else ws_bytes
    ws = device.array(np.full(nws + 4096, SENTINEL, np.uint8)) if want_ops else None
    try:
        device.call("mgr_edit_distance", ins[0], ins[1], n_hyp, Lh, ins[2], ins[3], n_ref, Lr, ins[4], ins[5], P, costs[0], costs[1],
                    costs[2], mask, outs[0], outs[1], outs[2], outs[4] if want_ops else None, outs[3] if want_ops else None, ws, nws)
        res = []
        for (shp, dt), o in zip(shapes, outs):
            a = o.download()
            n = int(np.prod(shp))
            assert np.all(a[n:] == SENTINEL), "guard words behind an output were written"
            res.append(a[:n].reshape(shp))
        if want_ops:
            assert np.all(ws.download()[nws:] == SENTINEL), "bytes behind the workspace were written"
        return tuple(res) if want_ops else (res[0], res[1], res[2], None, None)
    finally:
        for a in ins + outs + [ws]:
            if a is not None:
                a.free()


def assert_equal_ref(got, want):
    for name, g, w in zip(("dist", "counts", "lens", "n_ops", "ops"), got, want):
        if g is not None:
            assert np.array_equal(g, w), (name, np.argwhere(np.asarray(g) != np.asarray(w))[:5])


def padded(rows, width):
    """Rows of labels -> (len(rows), width) int32 padded with -1."""
    a = -np.ones((len(rows), width), np.int32)
    for i, r in enumerate(rows):
        a[i, :len(r)] = r
    return a


@pytest.mark.parametrize("A", [2, 5, 44])
@pytest.mark.parametrize("n", REF_LENS)
def test_kernel_equals_reference(device, n, A):
    """One ref length, every hyp length, the four cost sets; with and without ops."""
    rng = np.random.default_rng(1000 * A + n)
    hyps = [[int(v) for v in rng.integers(0, A, m)] for m in HYP_LENS] * 2
    refs = [[int(v) for v in rng.integers(0, A, n)] for _ in range(len(hyps))]
    if n >= 2:      # near-copies: long hit runs with a few edits, where the three steps tie
        for k in range(len(HYP_LENS), len(hyps)):
            src = list(hyps[k])
            refs[k] = (src + refs[k])[:n]
    hyp, ref = padded(hyps, 303), padded(refs, n + 3)
    for costs in COSTS:
        want = er.kernel_ref(hyp, None, ref, None, None, None, costs)
        got = run_edit(device, hyp, None, ref, None, None, None, costs)
        assert_equal_ref(got, want)
        plain = run_edit(device, hyp, None, ref, None, None, None, costs, want_ops=False)
        assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1]) and np.array_equal(plain[2], got[2])


@pytest.mark.parametrize("Lr", [700, 1500, 4095])
def test_wide_rows(device, Lr):
    """Rows of up to MGR_EDIT_MAX_LEN labels: the kernels with 16, 32 and 64 columns per lane, the back-pointers in the workspace."""
    rng = np.random.default_rng(Lr)
    Lh = {700: 40, 1500: 1000, 4095: 4095}[Lr]      # (the last two: more back-pointers than LDS holds)
    hyps = [[int(v) for v in rng.integers(0, 5, m)] for m in (24, 0, 7, min(Lh, 33))]
    refs = [[int(v) for v in rng.integers(0, 5, n)] for n in (Lr, Lr - 1, 65, 0)]
    hyp, ref = padded(hyps, Lh), padded(refs, Lr)
    for costs in ((10, 7, 7), ASYM):
        assert_equal_ref(run_edit(device, hyp, None, ref, None, None, None, costs), er.kernel_ref(hyp, None, ref, None, None, None, costs))
    # the largest costs at the full width: cost near 2^27
    big = (16384, 16384, 16384)
    got = run_edit(device, hyp, None, ref, None, [1, 0], [0, 3], big, want_ops=False)
    assert got[0].tolist() == [16384 * Lr, 16384 * 24] and got[1].tolist() == [[0, 0, Lr, 0], [0, 0, 0, 24]]


def test_input_conventions(device):
    Cn = 22
    rng = np.random.default_rng(7)
    hyp = rng.integers(0, Cn, (6, 37)).astype(np.int32)
    ref = rng.integers(0, Cn, (5, 70)).astype(np.int32)
    hyp[rng.random(hyp.shape) < 0.2] = -1      # -1 in the middle of rows
    ref[rng.random(ref.shape) < 0.2] = -1
    hyp[4] = -1
    hlen, rlen = [37, 0, 500, -4, 12, 36], [70, 71, 0, 33, 64]
    mask = (1 << 0) | (1 << (Cn - 1))
    ph, pr = [0, 0, 0, 0, 0, 3, 3, 5, 1, 2, 4, 2], [0, 1, 2, 3, 4, 1, 1, 0, 4, 3, 2, 3]      # repeats, one hyp against every ref
    for hl, rl, mk in ((None, None, 0), (hlen, rlen, 0), (hlen, None, mask), (None, rlen, mask)):
        want = er.kernel_ref(hyp, hl, ref, rl, ph, pr, (4, 3, 3), mk)
        assert_equal_ref(run_edit(device, hyp, hl, ref, rl, ph, pr, (4, 3, 3), mk), want)
    assert np.any(want[2] == 0) and len(set(want[0].tolist())) > 4
    # the NULL / NULL form: pair p is (p, p)
    sq = ref[:, :30].copy()
    want = er.kernel_ref(hyp[:5], hlen[:5], sq, None, None, None, ASYM, mask)
    assert_equal_ref(run_edit(device, hyp[:5], hlen[:5], sq, None, None, None, ASYM, mask), want)
    # bits of labels that do not occur, and of labels >= 64 (there are no such bits), change nothing
    h64 = hyp.copy()
    h64[0, :3] = [64, 100, 2 ** 31 - 1]
    want = er.kernel_ref(h64, None, ref, None, ph, pr, (1, 1, 1), 1 << 63)
    assert_equal_ref(run_edit(device, h64, None, ref, None, ph, pr, (1, 1, 1), 1 << 63), want)


def test_pairs_are_independent(device):
    rng = np.random.default_rng(3)
    hyps = [[int(v) for v in rng.integers(0, 3, int(rng.integers(0, 90)))] for _ in range(40)]
    refs = [[int(v) for v in rng.integers(0, 3, int(rng.integers(0, 140)))] for _ in range(40)]
    hyp, ref = padded(hyps, 90), padded(refs, 140)
    ph, pr = rng.integers(0, 40, 64), rng.integers(0, 40, 64)
    base = run_edit(device, hyp, None, ref, None, ph, pr, (10, 7, 7))
    assert_equal_ref(base, er.kernel_ref(hyp, None, ref, None, ph, pr, (10, 7, 7)))
    perm = rng.permutation(64)
    for a, b in zip(base, run_edit(device, hyp, None, ref, None, ph[perm], pr[perm], (10, 7, 7))):
        assert np.array_equal(a[perm], b)
    # a pair alone, and among other rows
    for p in (0, 17, 63):
        alone = run_edit(device, hyp[ph[p]:ph[p] + 1], None, ref[pr[p]:pr[p] + 1], None, [0], [0], (10, 7, 7))
        for a, b in zip(base, alone):
            assert np.array_equal(a[p], b[0])
    # twice the same call: the same bits
    for a, b in zip(base, run_edit(device, hyp, None, ref, None, ph, pr, (10, 7, 7))):
        assert np.array_equal(a, b)


def test_workspace_sizes(device):
    q = device.lib.mgr_edit_distance_ws_bytes
    assert q(64, 300, 257, 0) == 0 and q(1, 1, 1, 1) > 0
    assert q(64, 300, 257, 1) >= 64 * 300 * 258 * 2 // 8          # 2 bits per cell
    assert q(64, 300, 257, 1) <= 2 * 64 * 300 * 320 * 2 // 8        # ... and no more than the padding of a row to 64 columns explains
    assert q(2, 4095, 4095, 1) >= 2 * 4095 * 4096 * 2 // 8


def test_refusals(device):
    """Through the host checks and the library's argument checks only: nothing here reaches a kernel."""
    from mgr_amd import _capi, decoding
    hyp, ref = padded([[1, 2]], 4), padded([[1]], 3)
    with pytest.raises(_capi.MgrError, match="above 4095"):
        run_edit(device, np.zeros((1, 4096), np.int32), None, ref, None, None, None, (1, 1, 1), want_ops=False)
    with pytest.raises(_capi.MgrError, match="above 4095"):
        run_edit(device, hyp, None, np.zeros((1, 4096), np.int32), None, None, None, (1, 1, 1), want_ops=False)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (16385, 1, 1), (1, 16385, 1), (1, 1, 16385), (-1, 1, 1)):
        with pytest.raises(_capi.MgrError, match="costs"):
            run_edit(device, hyp, None, ref, None, None, None, bad, want_ops=False)
    need = device.lib.mgr_edit_distance_ws_bytes(1, 4, 3, 1)
    with pytest.raises(_capi.MgrError, match="workspace too small"):
        run_edit(device, hyp, None, ref, None, None, None, (1, 1, 1), ws_bytes=need - 1)
    with pytest.raises(_capi.MgrError, match="both"):
        run_edit(device, hyp, None, ref, None, [0], None, (1, 1, 1), want_ops=False)
    with pytest.raises(_capi.MgrError, match="n_hyp = n_ref = n_pairs"):
        run_edit(device, padded([[1], [2]], 2), None, ref, None, None, None, (1, 1, 1), want_ops=False)
    with pytest.raises(_capi.MgrError, match="bad shape"):
        run_edit(device, hyp, None, ref, None, None, None, (1, 1, 1), want_ops=False, n_pairs=0)
    # the host wrapper: indices, costs, labels to ignore, widths
    with pytest.raises(IndexError):
        decoding.edit_distances([[1]], [[1]], pairs=[(1, 0)], dev=device)
    with pytest.raises(IndexError):
        decoding.edit_distances([[1]], [[1]], pairs=[(0, -1)], dev=device)
    with pytest.raises(ValueError):
        decoding.edit_distances([[1]], [[1]], costs=(1, 2), dev=device)
    with pytest.raises(ValueError):
        decoding.edit_distances([[1]], [[1]], costs=(1, 1, 1.5), dev=device)
    with pytest.raises(ValueError):
        decoding.edit_distances([[1]], [[1]], ignore=(-1,), dev=device)
    with pytest.raises(ValueError):
        decoding.edit_distances(np.zeros((1, 4096)), [[1]], dev=device)
    # ... and after all of them the library still answers
    assert decoding.edit_distances([[1, 2]], [[1]], dev=device)[0].tolist() == [1]


def test_host_wrappers_equal_the_reference(device):
    from mgr_amd import decoding
    rng = np.random.default_rng(21)
    hyps = [[int(v) for v in rng.integers(0, 6, int(rng.integers(0, 12)))] for _ in range(30)]
    refs = [[int(v) for v in rng.integers(0, 6, int(rng.integers(0, 12)))] for _ in range(30)]
    dist, counts, lens, ops = decoding.edit_distances(hyps, refs, costs=decoding.HTK_COSTS, ignore=(5,), return_ops=True, dev=device)
    strip = lambda s: [v for v in s if v != 5]
    conf = np.zeros((7, 7), np.int64)
    for p, (h, r) in enumerate(zip(hyps, refs)):
        c, cnt, o = er.align(strip(h), strip(r), (10, 7, 7))
        assert (int(dist[p]), tuple(counts[p]), list(ops[p])) == (c, cnt, o) and lens[p].tolist() == [len(strip(h)), len(strip(r))]
        assert er.replay(strip(h), strip(r), ops[p], (10, 7, 7)) == (True, c, cnt)
        i = j = 0
        for op in o:
            conf[strip(r)[j] if op != er.INS else 6, strip(h)[i] if op != er.DEL else 6] += 1
            i, j = i + (op != er.DEL), j + (op != er.INS)
    s = decoding.score_sequences(hyps, refs, costs=decoding.HTK_COSTS, ignore=(5,), confusion=True, n_classes=6, dev=device)
    assert np.array_equal(s["confusion"], conf) and s["S"] == conf[:6, :6].sum() - np.trace(conf[:6, :6]) and s["H"] == np.trace(conf[:6, :6])
    assert (s["D"], s["I"]) == (conf[:6, 6].sum(), conf[6, :6].sum()) and s["N"] == sum(len(strip(r)) for r in refs)
    unit = decoding.score_sequences(hyps, refs, dev=device)
    assert unit["ler"] == decoding.label_error_rate(hyps, refs) and unit["dist_sum"] == unit["S"] + unit["D"] + unit["I"]


def test_nbest_attainable_and_mbr_equal_their_restatements(device):
    """On the N-best lists of the beam search with a bigram table at (N, T, C, W, top_paths) = (4, 50, 22, 10, 10): distances ==,
    risks to 1e-12 relative (fp64 sums of at most 32 terms), picks == (tests/test_cpu_edit.py has shown that no sample's two
    smallest reference risks are within 1e-9: none is excused)."""
    from mgr_amd import decoding
    case = nbest_case()
    N, T, Cn, W, NP = NBEST_SHAPE
    seqs, score, logp, gap = case["nbest"]
    paths, sc, _ = decoding.beam_search_lm_decode(case["P"], lm=case["ext"], lm_end=case["fin"], input_length=case["il"], beam_width=W,
                                                  top_paths=NP, dev=device)
    assert paths == seqs and np.allclose(sc, np.asarray(score), rtol=1e-12, atol=0)
    for costs in ((1, 1, 1), (10, 7, 7)):
        d, r, ler = decoding.nbest_attainable(paths, case["refs"], costs=costs, dev=device)
        wd, wr, wler = er.nbest_attainable_ref(seqs, case["refs"], costs)
        assert np.array_equal(d, wd) and np.array_equal(r, wr) and ler == wler
        for scale in MBR_SCALES:
            picks, ranks, risk = decoding.mbr_decode(paths, sc, scale=scale, costs=costs, dev=device)
            wp, wranks, wrisk, gaps = er.mbr_ref(seqs, sc, scale, costs)
            print("mbr", costs, scale, "max rel risk err", np.max(np.abs(risk - wrisk) / wrisk), "ranks", ranks, "min gap", gaps.min())
            assert np.all(np.abs(risk - wrisk) <= 1e-12 * np.abs(wrisk))
            excused = gaps <= 1e-9
            assert excused.sum() * 20 <= N
            assert np.array_equal(ranks[~excused], wranks[~excused]) and [p for p, e in zip(picks, excused) if not e] == \
                [p for p, e in zip(wp, excused) if not e]
    # K = 1 returns the 1-best
    one = decoding.mbr_decode([p[:1] for p in paths], sc[:, :1], dev=device)
    assert one[0] == [p[0] for p in paths] and one[1].tolist() == [0] * N and np.all(one[2] == 0.0)


# ---- through the facade, on the tiny fusion model tests/test_gpu_beam_lm.py builds -------------------------------------------------
def _facade(device):
    from mgr_amd import decoding, keras_like as K
    from mgr_amd.configs import fusion_spec
    from mgr_amd.keras_like import Model
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    K.set_learning_phase(0)
    decoding._DEV[0] = device
    spec = fusion_spec()
    B, T = 2, 48
    full = [synthetic_arrays(spec, B, T, 4, 700 + i, lmin=2, lmax=4) for i in range(3)]
    m = Model(spec, device=device)
    m.set_weights_dict(synthetic_weights(spec, 11))
    return spec, m, full, B


def _labelled(full, B, short_last):
    for i, (xs, lab, il, ll) in enumerate(full):
        n = 1 if (short_last and i == len(full) - 1) else B
        x = {k: v[:n] for k, v in xs.items()}
        x.update(the_labels=lab[:n], input_length=il[:n], label_length=ll[:n])
        yield x, None


def test_score_generator_equals_decode_then_score(device):
    from mgr_amd import decoding
    from mgr_amd.keras_like import Adam
    spec, m, full, B = _facade(device)
    m.compile(optimizer=Adam(lr=1e-3))
    Cn = spec.num_classes
    rng = np.random.default_rng(5)
    lm, lm_end = decoding.bigram_lm([list(rng.integers(0, Cn - 1, 6)) for _ in range(40)], Cn, add_k=0.5)
    modes = [("greedy", {}), ("greedy", dict(threshold=0.06)), ("beam", dict(beam_width=8)),
             ("beam_lm", dict(beam_width=8, lm=lm, lm_end=lm_end, alpha=0.7, beta=0.3))]
    loss_full = m.evaluate_generator(_labelled(full, B, False), steps=3)
    seen = set()
    for short in (False, True):
        rows = [(1 if (short and i == 2) else B) for i in range(3)]
        data = [{k: v[:n] for k, v in b[0].items()} for b, n in zip(full, rows)]
        refs = np.concatenate([b[1][:n] for b, n in zip(full, rows)])
        for decode, kw in modes:
            got = m.score_generator(_labelled(full, B, short), steps=3, decode=decode, **kw)
            if decode == "greedy":
                segs = m.predict_generator(iter(data), steps=3, decode="segments", threshold=kw.get("threshold"))
                hyps = [[s[0] for s in sg] for sg in segs]
            else:
                hyps = m.predict_generator(iter(data), steps=3, decode=decode, **kw)[0]
            want = decoding.score_sequences(hyps, refs, ignore=(Cn - 1,), dev=device)
            for k in ("H", "S", "D", "I", "N", "ler", "corr", "acc"):
                assert got[k] == want[k], (decode, kw, k)
            for k in ("dist", "counts", "lens"):
                assert np.array_equal(got["per_sample"][k], want["per_sample"][k])
            assert got["per_sample"]["loss"].shape == (sum(rows),) and got["N"] == int((refs >= 0).sum())
            if not short:
                assert got["loss"] == loss_full      # bit for bit
            seen.add((got["H"], got["S"], got["D"], got["I"]))
    assert len(seen) > 1        # (the modes do not all decode the same thing)
    # other costs reach the kernel: the weighted distance of the same decode
    hyps = m.predict_generator(iter([b[0] for b in full]), steps=3, decode="beam", beam_width=8)[0]
    refs = np.concatenate([b[1] for b in full])
    got = m.score_generator(_labelled(full, B, False), steps=3, decode="beam", beam_width=8, costs=decoding.HTK_COSTS)
    want = decoding.score_sequences(hyps, refs, costs=decoding.HTK_COSTS, dev=device)
    assert np.array_equal(got["per_sample"]["dist"], want["per_sample"]["dist"]) and got["S"] == want["S"]
    with pytest.raises(ValueError):
        m.score_generator(_labelled(full, B, False), steps=3, decode="argmax")
    # under a communicator the integer sums and the loss are all-reduced: two ranks with the same shard double every count
    class TwoEqualRanks:
        rank = 0

        def allreduce_sum_scalar(self, v):
            return float(np.float32(v) + np.float32(v))      # (the communicators sum float32)

    one = m.score_generator(_labelled(full, B, False), steps=3)
    m.comm, m.world = TwoEqualRanks(), 2
    try:
        two = m.score_generator(_labelled(full, B, False), steps=3)
    finally:
        m.comm, m.world = None, 1
    assert [two[k] for k in "HSDIN"] == [2 * one[k] for k in "HSDIN"] and two["ler"] == one["ler"]
    assert two["loss"] == float(np.float32(one["loss"]) + np.float32(one["loss"])) / 2
    # the existing outputs give what they gave beside it
    assert m.evaluate_generator(_labelled(full, B, False), steps=3) == loss_full


def test_fit_generator_with_val_score_changes_nothing_else(device):
    from mgr_amd.keras_like import Adam, Callback
    runs = {}
    for key, vs in (("plain", None), ("scored", dict(decode="beam", beam_width=8))):
        spec, m, full, B = _facade(device)
        m.compile(optimizer=Adam(lr=1e-3))
        after = []

        class Rescore(Callback):
            def on_epoch_end(self, epoch, logs=None):
                if vs is not None:
                    after.append(self.model.score_generator(_labelled(full[2:], B, False), steps=1, **vs))

        def train():
            while True:
                for b in _labelled(full[:2], B, False):
                    yield b

        def val():
            while True:
                for b in _labelled(full[2:], B, False):
                    yield b

        h = m.fit_generator(train(), steps_per_epoch=2, epochs=2, verbose=0, validation_data=val(), validation_steps=1, val_score=vs,
                            callbacks=[Rescore()])
        runs[key] = (h.history, m.get_weights_dict(), after)
    hp, wp, _ = runs["plain"]
    hs, ws, after = runs["scored"]
    assert "val_ler" not in hp and set(hs) == set(hp) | {"val_ler", "val_corr", "val_acc"}
    assert hp["val_loss"] == hs["val_loss"] and hp["loss"] == hs["loss"]      # bit for bit
    assert set(wp) == set(ws) and all(wp[k].tobytes() == ws[k].tobytes() for k in wp)
    assert hs["val_ler"] == [a["ler"] for a in after] and hs["val_acc"] == [a["acc"] for a in after] and len(after) == 2
    assert hs["val_loss"] == [a["loss"] for a in after]


def test_pipelined_score_equals_one_batch_at_a_time(device):
    """Four batches in flight two at a time (both output slots reused) against one batch per stream, every decode mode; the loss slot
    is output="loss"'s bit for bit; an inference engine refuses."""
    from mgr_amd.configs import fusion_spec
    from mgr_amd.engine import Engine
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    spec = fusion_spec()
    B, T, Lmax = 16, 72, 6
    data = [synthetic_arrays(spec, B, T, Lmax, 900 + i, lmin=2, lmax=6) for i in range(4)]
    eng = Engine(spec, B, T, Lmax, device=device, seed=5)
    eng.set_weights(synthetic_weights(spec, 11))
    losses = list(eng.predict_stream(iter(data), output="loss"))
    for kw in (dict(decode="greedy"), dict(decode="greedy", threshold=0.05), dict(decode="beam", beam_width=6),
               dict(decode="beam_lm", beam_width=6, beta=0.2), dict(decode="greedy", costs=(10, 7, 7), ignore=(0, 21))):
        pipe = list(eng.predict_stream(iter(data), output="score", **kw))
        single = [list(eng.predict_stream([b], output="score", **kw))[0] for b in data]
        for a, b, l, d in zip(pipe, single, losses, data):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[0], l)
            assert a[1].shape == (B,) and a[2].shape == (B, 4) and a[3].shape == (B, 2) and a[1].dtype == np.int32
            if "ignore" not in kw:
                assert np.array_equal(a[3][:, 1], (d[1] >= 0).sum(axis=1))
        assert not np.array_equal(pipe[0][1], pipe[1][1])
    with pytest.raises(ValueError):
        list(eng.predict_stream(iter(data), output="score", decode="best"))
    with pytest.raises(ValueError):
        list(eng.predict_stream(iter(data), output="score", costs=(1, 0, 1)))
    eng.close()
    inf = Engine(spec, B, T, Lmax, device=device, seed=5, inference_only=True)
    with pytest.raises(ValueError):
        list(inf.predict_stream(iter(data), output="score"))
    inf.close()
