"""-m gpu: mgr_ctc_loss_grad (csrc/ctc.hip) at every lattice width and length edge, against oracle.keras_ref.ctc_loss_grad in fp64.

The cases are built in tests/ctc_cases.py (their premises are checked without a GPU in tests/test_cpu_ctc_edges.py).  Every case
goes through _check: loss 1e-4 relative (the project's bound), +inf exactly where the reference is, the gradient PER SAMPLE
(max |dz_b - ref_b| <= bound * max |ref_b|), exact +0.0 on dropped frames, and the same bits without a gradient, with one sample per
workgroup, and with a workspace full of 0xFF (NaN) instead of 0x00.  Every case prints one line with its measured errors
(pytest -s; profiles/ctc_edges.txt keeps a run's lines).

Gradient bound: 5e-4 per sample.  The kernel renormalises every 16 steps and stays far below what the float32 oracle gives (1e-4 ...
1.2e-3 per sample on these inputs); the measured figures are in profiles/ctc_edges.txt."""
import numpy as np
import pytest

from tests import ctc_cases as cc

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-4
GRAD_BOUND = 5e-4


def _run(dev, c, gscale=1.0, need_grad=True, ws_fill=0x00):
    """mgr_ctc_loss_grad on a case.  loss and dLogits start as 0xFF bytes (NaN), the workspace as `ws_fill` bytes."""
    B, T, Cn = c.P.shape
    Lmax = c.labels.shape[1]
    held = [dev.array(c.P), dev.array(c.labels.astype(np.int32)), dev.array(c.il.astype(np.int32)), dev.array(c.ll.astype(np.int32)),
            dev.empty((B,)), dev.empty((B, T, Cn)), dev.bytes(dev.lib.mgr_ctc_ws_bytes(B, T, Cn, Lmax))]
    dP, dl, dil, dll, loss, dz, ws = held
    try:
        dev.call("mgr_memset", loss, 0xFF, loss.nbytes)
        dev.call("mgr_memset", dz, 0xFF, dz.nbytes)
        dev.call("mgr_memset", ws, ws_fill, ws.nbytes)
        dev.call("mgr_ctc_loss_grad", dP, dl, dil, dll, B, T, Cn, Lmax, c.skip, c.blank, c.eps, gscale, loss, dz if need_grad else 0,
                 ws, ws.nbytes)
        return loss.download(), (dz.download() if need_grad else None)
    finally:
        for a in held:
            a.free()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _dropped_frames_are_plus_zero(c, dz):
    T = c.P.shape[1]
    for b in range(len(c.il)):
        Tp = int(np.clip(c.il[b], 0, T - c.skip))
        assert not _bits(dz[b, :c.skip]).any() and not _bits(dz[b, c.skip + Tp:]).any(), (c.name, b)


def _loss_errors(c, loss, ref_loss):
    """+inf exactly where the reference is (asserted); the relative error of every finite sample"""
    inf = np.isposinf(ref_loss)
    assert np.array_equal(np.isposinf(loss), inf), (c.name, loss, ref_loss)
    assert np.isfinite(loss[~inf]).all(), (c.name, loss)
    return np.abs(loss[~inf].astype(np.float64) - ref_loss[~inf]) / np.abs(ref_loss[~inf])


def _grad_errors(c, dz, ref_loss, ref_dz):
    """per sample max |dz_b - ref_b| / max |ref_b|; a sample with +inf loss has an all-zero gradient (asserted; its entry is 0)"""
    assert np.isfinite(dz).all(), c.name
    errs = np.zeros(len(ref_loss))
    for b in range(len(ref_loss)):
        if np.isposinf(ref_loss[b]):
            assert not _bits(dz[b]).any(), (c.name, b)
        else:
            errs[b] = np.abs(dz[b].astype(np.float64) - ref_dz[b]).max() / np.abs(ref_dz[b]).max()
    return errs


def _report(name, loss_err, grad_err, bound):
    print("ctc_edges %-18s loss err %.2e (bound %.0e)  grad err per sample %s (bound %s)"
          % (name, loss_err, LOSS_RTOL, "-" if grad_err is None else "%.2e" % grad_err, "-" if bound is None else "%.0e" % bound))


def _same_bits_every_way(dev, c, loss, dz):
    """need_grad = False, one sample per workgroup (tune key 18), a dirty workspace: the same bits"""
    loss_ng, _ = _run(dev, c, need_grad=False)
    assert _same_bits(loss, loss_ng), (c.name, "need_grad=False")
    dev.call("mgr_tune", 18, 1)
    try:
        loss1, dz1 = _run(dev, c, need_grad=dz is not None)
    finally:
        dev.call("mgr_tune", 18, 0)
    assert _same_bits(loss, loss1), (c.name, "one sample per workgroup: loss")
    loss_d, dz_d = _run(dev, c, need_grad=dz is not None, ws_fill=0xFF)
    assert _same_bits(loss, loss_d), (c.name, "dirty workspace: loss")
    if dz is not None:
        assert _same_bits(dz, dz1), (c.name, "one sample per workgroup: gradient")
        assert _same_bits(dz, dz_d), (c.name, "dirty workspace: gradient")


def _check(dev, name, bound=GRAD_BOUND):
    c = cc.case(name)
    ref_loss, ref_dz = cc.reference(name)
    loss, dz = _run(dev, c)
    le = _loss_errors(c, loss, ref_loss)
    ge = _grad_errors(c, dz, ref_loss, ref_dz)
    _report(name, le.max(), ge.max(), bound)
    assert (le <= LOSS_RTOL).all(), (name, "loss", loss, ref_loss)
    assert (ge <= bound).all(), (name, "gradient per sample", ge, bound)
    _dropped_frames_are_plus_zero(c, dz)
    _same_bits_every_way(dev, c, loss, dz)
    return loss, dz


@pytest.mark.parametrize("name", cc.A_NAMES)
def test_every_pairs_per_lane_width_with_states_on_the_lane_boundaries(device, name):
    """(a) Lmax 63 ... 255: k_ctc_chains<1 .. 4, *>, label lengths Lmax (states on the last lane), Lmax - 1, just past a multiple of
    64, and 1; repeated labels at the first pair of a lane."""
    _check(device, name)


@pytest.mark.parametrize("name", cc.B_NAMES)
def test_single_alignment_lattices_match_their_closed_form(device, name):
    """(b) one alignment only, so a wrong carry between lanes loses ALL of the probability: loss = - sum_t log y_t(path_t); one frame
    less gives +inf and a zero gradient, and the neighbour in the workgroup stays exact."""
    c = cc.case(name)
    loss, dz = _check(device, name)
    assert abs(loss[0] - c.closed[0]) <= LOSS_RTOL * abs(c.closed[0]), (name, loss[0], c.closed[0])
    assert np.isposinf(loss[1]) and not _bits(dz[1]).any()


@pytest.mark.parametrize("name", cc.C_NAMES)
def test_sweep_over_input_lengths_in_one_launch(device, name):
    """(c) T' = 1 ... 40 and around 256 and 512 in one batch (ppl = 1, chunks of 8), T' = 1 ... 20 at ppl = 3 (chunks of 4)"""
    _check(device, name)


@pytest.mark.parametrize("name", cc.D_NAMES)
def test_skip_blank_and_eps_are_honoured(device, name):
    """(d) skip 0 / 1 / 5, blank 0 / C // 2, eps 0 / 1e-3"""
    _check(device, name)


@pytest.mark.parametrize("gscale", [0.25, -2.0, 1.0 / 64])
def test_gscale_scales_the_gradient_exactly(device, gscale):
    """(d) a power-of-two gscale: dz = gscale * (the gscale = 1 gradient) bit for bit on the live frames, +0.0 on the dropped ones,
    and the loss does not move"""
    c = cc.case("d-base")
    loss1, dz1 = _run(device, c)
    loss, dz = _run(device, c, gscale=gscale)
    assert _same_bits(loss, loss1)
    _dropped_frames_are_plus_zero(c, dz)
    for b in range(len(c.il)):
        live = slice(c.skip, c.skip + int(c.il[b]))
        assert dz1[b, live].any() and _same_bits(dz[b, live], dz1[b, live] * np.float32(gscale)), (gscale, b)
    ref_loss, ref_dz = cc.reference("d-base")
    ge = _grad_errors(c, dz, ref_loss, ref_dz * gscale)
    _report("d-base gscale %g" % gscale, _loss_errors(c, loss, ref_loss).max(), ge.max(), GRAD_BOUND)
    assert (ge <= GRAD_BOUND).all(), (gscale, ge)


def test_out_of_range_arguments_are_clipped(device):
    """(e) input_len into [0, T - skip], label_len into [0, Lmax], label values into [0, C - 1] (include/mgr.h, K6): the same bits
    as the call with the arguments clipped beforehand; input_len 0 gives +inf and a zero gradient."""
    raw, clipped = cc.case("e-raw"), cc.case("e-clipped")
    loss_c, dz_c = _check(device, "e-clipped")
    loss_r, dz_r = _check(device, "e-raw")
    assert _same_bits(loss_r, loss_c) and _same_bits(dz_r, dz_c)
    for b in np.nonzero(clipped.il == 0)[0]:
        assert np.isposinf(loss_r[b]) and not _bits(dz_r[b]).any()
    assert (raw.il[np.nonzero(clipped.il == 0)[0]] <= 0).all()


def test_log_zero(device):
    """(f) eps = 0 and exact zeros in P, no gradient asked for: kLseFloor's path.  +inf where a label's class is never possible,
    the reference's finite loss where the zeros only close part of the lattice."""
    c = cc.case("f-logzero")
    ref_loss, _ = cc.reference("f-logzero")
    loss, _ = _run(device, c, need_grad=False)
    le = _loss_errors(c, loss, ref_loss)
    _report(c.name, le.max(), None, None)
    assert (le <= LOSS_RTOL).all(), (loss, ref_loss)
    assert np.isposinf(loss[0]) and np.isfinite(loss[1:]).all()
    _same_bits_every_way(device, c, loss, None)


def test_peaked_posteriors(device):
    """(g) a trained network's near-one-hot output (logit + 12 along one alignment): states hundreds of log-units apart inside one
    renormalisation window"""
    _check(device, "g-peaked12")


def test_chains_that_drift_100_log2_units_per_frame(device):
    """(h) posteriors that contradict the labels for 1900 frames: what the renormalisation every 16 steps is for.  The bound is the
    5e-4 of every case; a float32 lattice renormalised every 64 steps instead misses it on this input (1.0e-3 on sample 2 in a numpy
    model of the recursions, 1.5e-4 at 16 steps)."""
    _check(device, "h-drift")


def test_saturated_posteriors(device):
    """(g) logit + 25, eps = 1e-6: the loss (about 3e-3) is eps * C per frame and the gradient tiny, so: finite, zero frames, and
    |loss - ref| <= 1e-4 |ref| + a, a = 4 x the absolute loss error of the float32 oracle on the same float32 P (the kernel's 1-ulp
    raw exp / log against numpy's half ulp, and one more rounding of the emissions)."""
    c = cc.case("g-peaked25")
    ref_loss, _ = cc.reference(c.name)
    loss32, _ = cc.oracle(c, np.float32)
    a = 4.0 * np.abs(loss32.astype(np.float64) - ref_loss)
    loss, dz = _run(device, c)
    _loss_errors(c, loss, ref_loss)
    err = np.abs(loss.astype(np.float64) - ref_loss)
    print("ctc_edges %-18s loss abs err %s  bound 1e-4 |ref| + a, a = %s, ref = %s" % (c.name, err, a, ref_loss))
    assert (err <= LOSS_RTOL * np.abs(ref_loss) + a).all()
    assert np.isfinite(dz).all()
    _dropped_frames_are_plus_zero(c, dz)
    _same_bits_every_way(device, c, loss, dz)
