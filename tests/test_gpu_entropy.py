"""-m gpu: mgr_ctc_entropy_grad (csrc/ctc.hip) - the CTC loss with the entropy of the labels' alignments and the gradient of
loss_scale * loss - ent_scale * H - at every lattice width and length edge the loss is tested at (tests/ctc_cases.py), against the
shipped loss bit for bit and against the fp64 restatement of tests/entropy_ref.py.

Per case: loss == mgr_ctc_loss_grad's bits; with ent_scale = 0 dLogits == its bits; two calls and a call without dLogits give equal
bits; with loss_scale = 0, ent_scale = 1 dLogits is within 1e-4 of the restatement's largest entry of the case (the project's gradient
bound); |H - H_ref| <= 1e-4 max(1, |m_ref|) per sample (H = ln Z - m is a difference of two quantities of the loss's size, each held
to the loss's 1e-4 relative); what does not fit gives +inf / 0 / a zero gradient.  The workspace starts as 0xFF bytes (NaN) before
every call.  Every case prints one line with its measured maxima (pytest -s; tools/entropy_bench.py writes the same figures to profiles/entropy_parity.txt).
f-logzero (eps = 0 and exact zeros in P) is checked without a gradient, as the loss is: the chain through log(P + eps) is 0 / 0 there.

Measured on an MI355X: the error of H is at most 5.2e-6 and the gradient's 5.0e-5 (b-i-L193; h-drift 4.6e-5), against bounds of 1e-4."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import entropy_ref as en  # noqa: E402
from tests import ctc_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

GRAD_BOUND = 1e-4
H_BOUND = 1e-4
# (no case is marked slow: the fp64 restatement of the longest, h-drift, takes under two seconds, all of them together eight)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _arrays(dev, c):
    B, T, Cn = c.P.shape
    Lmax = c.labels.shape[1]
    return [dev.array(c.P), dev.array(c.labels.astype(np.int32)), dev.array(c.il.astype(np.int32)), dev.array(c.ll.astype(np.int32))], (B, T, Cn, Lmax)


def _entropy(dev, c, loss_scale, ent_scale, need_grad=True, ws_bytes=None):
    """mgr_ctc_entropy_grad on a case: (loss, H, dLogits or None).  The outputs and the workspace start as 0xFF bytes (NaN)."""
    ins, (B, T, Cn, Lmax) = _arrays(dev, c)
    n = 2 * dev.lib.mgr_ctc_ws_bytes(B, T, Cn, Lmax) if ws_bytes is None else ws_bytes
    held = ins + [dev.empty((B,)), dev.empty((B,)), dev.empty((B, T, Cn)), dev.bytes(n)]
    loss, H, dz, ws = held[4:]
    try:
        for a in (loss, H, dz, ws):
            dev.call("mgr_memset", a, 0xFF, a.nbytes)
        dev.call("mgr_ctc_entropy_grad", *ins, B, T, Cn, Lmax, c.skip, c.blank, c.eps, loss_scale, ent_scale, loss, H, dz if need_grad else 0,
                 ws, ws.nbytes)
        return loss.download(), H.download(), (dz.download() if need_grad else None)
    finally:
        for a in held:
            a.free()


def _loss(dev, c, gscale, need_grad=True):
    """the shipped mgr_ctc_loss_grad on the same case"""
    ins, (B, T, Cn, Lmax) = _arrays(dev, c)
    held = ins + [dev.empty((B,)), dev.empty((B, T, Cn)), dev.bytes(dev.lib.mgr_ctc_ws_bytes(B, T, Cn, Lmax))]
    loss, dz, ws = held[4:]
    try:
        for a in (loss, dz, ws):
            dev.call("mgr_memset", a, 0xFF, a.nbytes)
        dev.call("mgr_ctc_loss_grad", *ins, B, T, Cn, Lmax, c.skip, c.blank, c.eps, gscale, loss, dz if need_grad else 0, ws, ws.nbytes)
        return loss.download(), (dz.download() if need_grad else None)
    finally:
        for a in held:
            a.free()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(H, m, dH/dlogits, logp) of a case in fp64 (of the clipped twin for e-raw), read-only"""
    c = cc.case("e-clipped" if name == "e-raw" else name)
    out = en.batch(c.P, c.labels, c.il, c.ll, c.skip, c.blank, c.eps)
    for a in out:
        a.flags.writeable = False
    return out


def _check(dev, name):
    c = cc.case(name)
    with_grad = name != "f-logzero"
    H_ref, m_ref, dH_ref, logp_ref = _reference(name)
    loss, H, dz = _entropy(dev, c, 0.0, 1.0, need_grad=with_grad)
    # the loss is the shipped loss's bits, with and without its gradient scale; ent_scale = 0 is its gradient too
    loss0, dz0 = _loss(dev, c, 0.25, need_grad=with_grad)
    loss_l, H_l, dz_l = _entropy(dev, c, 0.25, 0.0, need_grad=with_grad)
    assert _same_bits(loss, loss0) and _same_bits(loss_l, loss0), (name, "loss bits")
    assert _same_bits(H_l, H), (name, "H with ent_scale = 0")
    # again, and without dLogits: equal bits
    loss2, H2, dz2 = _entropy(dev, c, 0.0, 1.0, need_grad=with_grad)
    loss_n, H_n, _ = _entropy(dev, c, 0.0, 1.0, need_grad=False)
    assert _same_bits(loss2, loss) and _same_bits(H2, H) and _same_bits(loss_n, loss) and _same_bits(H_n, H), (name, "repeat / no dLogits")
    # what does not fit: +inf, 0, a zero gradient - exactly where the restatement has no alignment
    dead = np.isneginf(logp_ref)
    assert np.array_equal(np.isposinf(loss), dead) and set(c.inf) <= set(np.flatnonzero(dead)), (name, loss, logp_ref)
    assert not _bits(H[dead]).any() and np.isfinite(H).all() and (H >= 0).all(), (name, H)
    assert not _bits(H[np.clip(c.ll, 0, None) == 0]).any(), (name, "no labels: H = 0")
    h_err = np.abs(H.astype(np.float64) - H_ref) / np.maximum(1.0, np.abs(m_ref))
    g_err = None
    if with_grad:
        assert _same_bits(dz_l, dz0), (name, "ent_scale = 0: the loss's gradient bits")
        assert _same_bits(dz2, dz), (name, "repeat: gradient")
        assert np.isfinite(dz).all(), name
        T = c.P.shape[1]
        for b in range(len(c.il)):
            Tp = int(np.clip(c.il[b], 0, T - c.skip))
            assert not _bits(dz[b, :c.skip]).any() and not _bits(dz[b, c.skip + Tp:]).any(), (name, b, "dropped frames")
            if dead[b]:
                assert not _bits(dz[b]).any(), (name, b)
        top = np.abs(dH_ref).max()
        g_err = np.abs(dz.astype(np.float64) + dH_ref).max() / top if top > 0 else np.abs(dz).max()      # (dLogits = -ent_scale dH/dlogits)
    print("entropy_parity %-18s H err / max(1, |m|) %.2e (bound %.0e)  max |m| %.1f  max H %.3f  grad err / largest entry %s (bound %.0e)"
          % (name, h_err.max(), H_BOUND, np.abs(m_ref).max(), H_ref.max(), "-" if g_err is None else "%.2e" % g_err, GRAD_BOUND))
    assert (h_err <= H_BOUND).all(), (name, "H", H, H_ref, m_ref)
    if with_grad:
        assert g_err <= GRAD_BOUND, (name, "gradient", g_err)
    return loss, H, dz


@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_every_ctc_edge_case(device, name):
    _check(device, name)


def test_out_of_range_arguments_are_clipped(device):
    """e-raw gives the bits of e-clipped, gradient included"""
    raw, clipped = cc.case("e-raw"), cc.case("e-clipped")
    for scales in ((0.0, 1.0), (0.5, 0.125)):
        a, b = _entropy(device, raw, *scales), _entropy(device, clipped, *scales)
        assert all(_same_bits(x, y) for x, y in zip(a, b)), scales
    loss, H, dz = a
    for b in np.flatnonzero(clipped.il == 0):
        assert np.isposinf(loss[b]) and H[b] == 0.0 and not _bits(dz[b]).any()


def _sub(c, rows, P=None):
    import types
    rows = list(rows)
    return types.SimpleNamespace(name=c.name, P=np.ascontiguousarray((c.P if P is None else P)[rows]), labels=c.labels[rows], il=c.il[rows],
                                 ll=c.ll[rows], skip=c.skip, blank=c.blank, eps=c.eps, inf=())


@pytest.mark.parametrize("name", ["a-Lmax64", "b-ii-L65", "c-sweep-ppl3"])
def test_samples_are_independent_of_their_neighbours(device, name):
    """A sample alone, beside other neighbours (the infeasible and empty ones among them), and with one sample per workgroup: the same
    bits for the sample."""
    c = cc.case(name)
    B = c.P.shape[0]
    whole = _entropy(device, c, 0.5, 0.25)
    for b in (0, B - 1):
        alone = _entropy(device, _sub(c, [b]), 0.5, 0.25)
        assert all(_same_bits(x[b:b + 1], y) for x, y in zip(whole, alone)), (name, b, "alone")
    rng = np.random.default_rng(3)
    P2 = np.array(c.P)
    P2[1:] = cc.rand_probs(rng, B - 1, c.P.shape[1], c.P.shape[2])
    other = _entropy(device, _sub(c, range(B), P2), 0.5, 0.25)
    assert all(_same_bits(x[0], y[0]) for x, y in zip(whole, other)), (name, "other neighbours")
    device.call("mgr_tune", 18, 1)
    try:
        one = _entropy(device, c, 0.5, 0.25)
    finally:
        device.call("mgr_tune", 18, 0)
    assert all(_same_bits(x, y) for x, y in zip(whole, one)), (name, "one sample per workgroup")


def test_both_terms_add_up(device):
    """loss_scale dloss - ent_scale dH against the two pure gradients, to float32 rounding of the sum (d-base)"""
    c = cc.case("d-base")
    _, _, gl = _entropy(device, c, 1.0, 0.0)
    _, _, ge = _entropy(device, c, 0.0, 1.0)
    _, _, both = _entropy(device, c, 0.5, 2.0)
    want = 0.5 * gl.astype(np.float64) + 2.0 * ge.astype(np.float64)
    assert np.abs(both - want).max() <= 1e-5 * np.abs(want).max()


def test_ascent_on_the_kernels_own_gradient_raises_its_own_entropy(device):
    """z + lr dH/dz with the kernel's pure-entropy gradient raises the kernel's H on every sample with a gradient (the inputs and lr of
    tests/test_cpu_entropy.py); the others keep theirs."""
    import types
    z, lab, il, ll = en.ascent_inputs()
    mk = lambda zz: types.SimpleNamespace(P=en.softmax(zz).astype(np.float32), labels=lab, il=il, ll=ll, skip=en.ASCENT_SKIP,
                                          blank=z.shape[2] - 1, eps=en.ASCENT_EPS)
    loss, H, dz = _entropy(device, mk(z), 0.0, -1.0)          # (dLogits = + dH/dlogits)
    moving = np.abs(dz).reshape(len(H), -1).max(axis=1) > 0
    assert list(moving) == [True, True, False, False, True]
    _, H2, _ = _entropy(device, mk(z + en.ASCENT_LR * dz.astype(np.float64)), 0.0, -1.0)
    print("entropy ascent: H %s -> %s" % (H, H2))
    assert (H2[moving] > H[moving]).all(), (H, H2)
    assert _same_bits(H2[~moving], H[~moving]) and not H[~moving].any()


def test_alignment_entropy_facade(device):
    from mgr_amd import decoding
    c = cc.case("d-base")
    loss, H, dz = _entropy(device, c, 0.0, -1.0)
    rows = [list(r[:n]) for r, n in zip(c.labels, c.ll)]
    H1, logp1, g1 = decoding.alignment_entropy(c.P, rows, input_length=c.il, skip=c.skip, eps=c.eps, grad=True, dev=device)
    assert _same_bits(H1, H) and np.array_equal(logp1, -loss.astype(np.float64)) and _same_bits(g1, dz)
    H2, logp2 = decoding.alignment_entropy(c.P, c.labels, c.ll, c.il, skip=c.skip, eps=c.eps, dev=device)
    assert _same_bits(H2, H) and np.array_equal(logp2, logp1)


def test_a_workspace_of_the_losss_size_is_refused(device):
    from mgr_amd._capi import MgrError
    c = cc.case("d-base")
    B, T, Cn = c.P.shape
    with pytest.raises(MgrError):
        _entropy(device, c, 1.0, 1.0, ws_bytes=device.lib.mgr_ctc_ws_bytes(B, T, Cn, c.labels.shape[1]))
