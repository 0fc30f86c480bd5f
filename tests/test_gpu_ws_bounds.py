"""-m gpu: every entry point that carves a caller's workspace stays inside the bytes its own mgr_*_ws_bytes query asked for.

A case runs its entry point once on `need` bytes that lie between two guard bands of 4096 bytes, the whole buffer filled with 0xFF,
and once on a roomy workspace of 2 * need bytes at its own base.  Both guard bands must still be all 0xFF, and the outputs of the two
runs must agree: bit for bit where an existing test of that entry point already asserts equal bits between two calls, else both
within that test's tolerance of its fp64 reference.  The shapes are odd, so that blocks end off the 256-byte grid and a dropped or
doubled padding moves a pointer: B = 3, T = 40, H = 20, F = 130 (72 for the row-major dropout projection, which then takes the
generic kernel), drop rate 0.5, ldt = 128, C = 21, Lmax = 7, beam 10, D = 2 H."""
import ctypes as C

import numpy as np
import pytest

from oracle import keras_ref as kr
from tests import ctc_cases as cc
from tests.helpers import rel_err
from tests.test_gpu_membound_passes import _grads_ref, _ints, _narrow_mask
from tests.test_gpu_split_gemm import _proj_ref

pytestmark = pytest.mark.gpu
f32 = np.float32

GUARD = 4096
B, T, H, F_WIDE, F_ROW, P_DROP, LDT = 3, 40, 20, 130, 72, 0.5, 128
CN, LMAX, BEAM, D, SKIP = 21, 7, 10, 2 * 20, 2
N = 4 * H


def _both(dev, need, run):
    """run(ws) -> list of device outputs, on the guarded and on the roomy workspace; the downloaded outputs of the two runs"""
    need = int(need)
    assert need > 0
    buf = dev.empty((GUARD + need + GUARD,), np.uint8)
    dev.call("mgr_memset", buf, 0xFF, buf.nbytes)
    guarded = [o.download() for o in run(buf.view(GUARD, (need,)))]
    raw = buf.download()
    buf.free()
    assert (raw[:GUARD] == 0xFF).all(), "the call wrote in front of its workspace"
    assert (raw[GUARD + need:] == 0xFF).all(), "the call wrote behind the %d bytes its query asked for" % need
    big = dev.empty((2 * need,), np.uint8)
    dev.call("mgr_memset", big, 0xFF, big.nbytes)
    roomy = [o.download() for o in run(big)]
    big.free()
    return guarded, roomy


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _nan(dev, shape, dtype=f32):
    a = dev.empty(shape, dtype)
    dev.call("mgr_memset", a, 0xFF, a.nbytes)
    return a


# ------------------------------------------------------------------------------------------------ projections
def _proj_inputs(dev, F):
    rng = np.random.default_rng(F)
    X = rng.standard_normal((B, T, F)).astype(f32)
    W = (rng.standard_normal((F, N)) * 0.1).astype(f32)
    bias = rng.standard_normal(N).astype(f32)
    M = _narrow_mask(rng, B, F, P_DROP)
    return X, W, bias, M, [dev.array(a) for a in (X, W, bias, M)]


def test_input_proj_dropout_row_major(device):
    dev = device
    X, W, bias, M, (dX, dW, db, dM) = _proj_inputs(dev, F_ROW)

    def run(ws):
        Z = _nan(dev, (B, T, N))
        dev.call("mgr_lstm_input_proj_dropout", dX, F_ROW, dM, P_DROP, dW, db, Z, B, T, F_ROW, H, ws, ws.nbytes)
        return [Z]

    (g,), (r,) = _both(dev, dev.lib.mgr_lstm_input_proj_dropout_ws_bytes(B, F_ROW, H), run)
    assert np.isfinite(g).all() and _same_bits(g, r)      # (test_narrow_projection_equals_generic_kernel_and_fp64: equal bits)


def test_input_proj_dropout_transposed(device):
    dev = device
    X, W, bias, M, (dX, dW, db, dM) = _proj_inputs(dev, F_WIDE)
    XT = dev.zeros((B, F_WIDE, LDT))
    dev.call("mgr_transpose_bt", dX, F_WIDE, XT, LDT, B, T, F_WIDE)

    def run(ws):      # (a stated bound on |X|: the split-f16 kernel, which uses the word block too)
        Z = _nan(dev, (B, T, N))
        dev.call("mgr_lstm_input_proj_dropout_t", XT, LDT, dM, P_DROP, dW, db, Z, B, T, F_WIDE, H, ws, ws.nbytes, float(np.abs(X).max()))
        return [Z]

    (g,), (r,) = _both(dev, dev.lib.mgr_lstm_input_proj_dropout_ws_bytes(B, F_WIDE, H), run)
    assert np.isfinite(g).all() and _same_bits(g, r)      # (test_input_proj_dropout_sparse_equals_dense: equal bits between calls)


def test_input_proj_dropout_split_rows(device):
    dev = device
    X, W, bias, M, (dX, dW, db, dM) = _proj_inputs(dev, F_WIDE)
    XS = dev.zeros((B, F_WIDE, LDT))
    dev.call("mgr_transpose_bt_split", dX, F_WIDE, XS, LDT, B, T, F_WIDE)

    def run(ws):
        Z = _nan(dev, (B, T, N))
        dev.call("mgr_lstm_input_proj_dropout_ts", XS, LDT, dM, P_DROP, dW, db, Z, B, T, F_WIDE, H, ws, ws.nbytes)
        return [Z]

    (g,), (r,) = _both(dev, dev.lib.mgr_lstm_input_proj_dropout_ts_ws_bytes(B, F_WIDE, H), run)
    assert _same_bits(g, r)                               # (test_projection_from_split_rows: equal bits between calls)
    ref = _proj_ref(X, M, W, bias)
    assert np.abs(g - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())


# ------------------------------------------------------------------------------------------------ parameter gradients
_GRADS = {}


def _grad_inputs(dev):
    """exact inputs (tests/test_gpu_membound_passes.py): every sum is exact in f32, the integer result is the fp64 reference"""
    if dev not in _GRADS:
        rng = np.random.default_rng(B * 977 + T + F_WIDE + H)
        X, Hs, dZ = _ints(rng, (B, T, F_WIDE)), _ints(rng, (B, T, H)), _ints(rng, (B, T, N), zero_share=0.3)
        M = ((rng.random((4, B, F_WIDE)) < 0.5) * f32(2.0)).astype(f32)
        dX, dH, dM, ddZ = dev.array(X), dev.array(Hs), dev.array(M), dev.array(dZ)
        XT, XS, HsT = dev.zeros((B, F_WIDE, LDT)), dev.zeros((B, F_WIDE, LDT)), dev.zeros((B, H, LDT))
        dev.call("mgr_transpose_bt", dX, F_WIDE, XT, LDT, B, T, F_WIDE)
        dev.call("mgr_transpose_bt_split", dX, F_WIDE, XS, LDT, B, T, F_WIDE)
        dev.call("mgr_transpose_bt_split_shift", dH, H, HsT, LDT, B, T, H, -1)
        ref = [a.astype(np.float64) for a in _grads_ref(X, M, Hs, dZ, 0)]
        _GRADS[dev] = dict(dX=dX, dH=dH, dM=dM, ddZ=ddZ, XT=XT, XS=XS, HsT=HsT, ref=ref, M=M)
    return _GRADS[dev]


def _grad_outs(dev):
    return [_nan(dev, (F_WIDE, N)), _nan(dev, (H, N)), _nan(dev, (N,))]


def _check_grads(guarded, roomy, ref, per_column=False):
    """dU / db: equal bits (test_param_grads_dropout_sparse_equals_dense asserts them between calls).  dW: both runs within 3e-5 of
    the fp64 reference - of its maximum, or per column for the split-f16 kernel: that test's bounds"""
    assert _same_bits(guarded[1], roomy[1]) and _same_bits(guarded[2], roomy[2])
    for got in (guarded, roomy):
        assert all(np.isfinite(a).all() for a in got)
        scale = np.maximum(np.abs(ref[0]).max(axis=0, keepdims=True), 1e-30) if per_column else max(1.0, np.abs(ref[0]).max())
        err = (np.abs(got[0] - ref[0]) / scale).max()
        print("dW: max err %.3e (bound 3e-5)" % err)
        assert err <= 3e-5


def test_param_grads(device):
    dev, g = device, _grad_inputs(device)

    def run(ws):
        o = _grad_outs(dev)
        dev.call("mgr_lstm_param_grads", g["dX"], F_WIDE, g["dM"], g["dH"], H, g["ddZ"], *o, B, T, F_WIDE, H, 0, ws, ws.nbytes)
        return o

    _check_grads(*_both(dev, dev.lib.mgr_lstm_param_grads_ws_bytes(B, T, F_WIDE, H), run), g["ref"])


def test_param_grads_dropout(device):
    dev, g = device, _grad_inputs(device)

    def run(ws):
        o = _grad_outs(dev)
        dev.call("mgr_lstm_param_grads_dropout", g["dX"], F_WIDE, g["dM"], P_DROP, g["dH"], H, g["ddZ"], *o, B, T, F_WIDE, H, 0, ws, ws.nbytes)
        return o

    _check_grads(*_both(dev, dev.lib.mgr_lstm_param_grads_dropout_ws_bytes(B, T, F_WIDE, H), run), g["ref"])


def test_param_grads_dropout_transposed(device):
    dev, g = device, _grad_inputs(device)

    def run(ws):      # (a stated bound on |X|: the split-f16 kernel, which uses the row maxima and the bound-violation word)
        o = _grad_outs(dev)
        dev.call("mgr_lstm_param_grads_dropout_t", g["XT"], LDT, g["dM"], P_DROP, g["dH"], H, g["ddZ"], *o, B, T, F_WIDE, H, 0, ws, ws.nbytes, 1.0)
        return o

    _check_grads(*_both(dev, dev.lib.mgr_lstm_param_grads_dropout_t_ws_bytes(B, T, F_WIDE, H, LDT), run), g["ref"], per_column=True)


@pytest.mark.parametrize("use_proj_ws,use_hst", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_param_grads_dropout_split_rows(device, use_proj_ws, use_hst):
    dev, g = device, _grad_inputs(device)
    pws = 0
    if use_proj_ws:      # the projection of the same mask leaves its kept lists behind
        pws = dev.bytes(dev.lib.mgr_lstm_input_proj_dropout_ts_ws_bytes(B, F_WIDE, H))
        dev.call("mgr_memset", pws, 0xFF, pws.nbytes)
        Wp_, bp_, Z_ = dev.array(_ints(np.random.default_rng(1), (F_WIDE, N))), dev.zeros((N,)), dev.empty((B, T, N))
        dev.call("mgr_lstm_input_proj_dropout_ts", g["XS"], LDT, g["dM"], P_DROP, Wp_, bp_, Z_, B, T, F_WIDE, H, pws, pws.nbytes)

    def run(ws):
        o = _grad_outs(dev)
        dev.call("mgr_lstm_param_grads_dropout_ts", g["XS"], LDT, g["dM"], P_DROP, g["dH"], H, g["ddZ"], *o, B, T, F_WIDE, H, 0, ws, ws.nbytes,
                 0, 0, pws, g["HsT"] if use_hst else 0)
        return o

    guarded, roomy = _both(dev, dev.lib.mgr_lstm_param_grads_dropout_ts_ws_bytes(B, T, F_WIDE, H, LDT), run)
    for a, b, ref in zip(guarded, roomy, g["ref"]):      # (test_weight_gradients_are_exact_on_exact_inputs: the integer result, bit for bit)
        assert _same_bits(a, b) and _same_bits(a, (ref + 0.0).astype(f32))


# ------------------------------------------------------------------------------------------------ CTC, head, decodes
def _ctc_inputs(dev):
    rng = np.random.default_rng(CN * 100 + LMAX)
    P = cc.rand_probs(rng, B, T, CN)
    ll = np.array([LMAX, 3, 1])
    lab = cc._labels(rng, B, LMAX, ll, CN, CN - 1)
    il = np.array([T - SKIP, T - SKIP - 1, 9])
    return P, lab, il, ll, [dev.array(P), dev.array(lab.astype(np.int32)), dev.array(il.astype(np.int32)), dev.array(ll.astype(np.int32))]


def test_ctc_loss_grad(device):
    dev = device
    P, lab, il, ll, arrs = _ctc_inputs(dev)

    def run(ws):
        loss, dz = _nan(dev, (B,)), _nan(dev, (B, T, CN))
        dev.call("mgr_ctc_loss_grad", *arrs, B, T, CN, LMAX, SKIP, CN - 1, 1e-8, 1.0, loss, dz, ws, ws.nbytes)
        return [loss, dz]

    guarded, roomy = _both(dev, dev.lib.mgr_ctc_ws_bytes(B, T, CN, LMAX), run)
    assert np.isfinite(guarded[0]).all() and np.isfinite(guarded[1]).all()
    assert all(_same_bits(a, b) for a, b in zip(guarded, roomy))      # (tests/test_gpu_ctc_edges.py, _same_bits_every_way)


def _dense_inputs(dev):
    rng = np.random.default_rng(B * 7 + D)
    A = rng.standard_normal((B, T, D)).astype(f32)
    Wd = (rng.standard_normal((D, CN)) * (2.0 / np.sqrt(D))).astype(f32)
    bd = (rng.standard_normal(CN) * 0.1).astype(f32)
    return A, Wd, bd, [dev.array(A), dev.array(Wd), dev.array(bd)]


def test_head_fwd_bwd(device):
    dev = device
    P_, lab, il, ll, (_, dlab, dil, dll) = _ctc_inputs(dev)
    A, Wd, bd, (dA_, dW_, db_) = _dense_inputs(dev)

    def run(ws):
        o = [_nan(dev, (B, T, CN)), _nan(dev, (B,)), _nan(dev, (B, T, CN)), _nan(dev, (D, CN)), _nan(dev, (CN,)), _nan(dev, (B, T, D))]
        dev.call("mgr_head_fwd_bwd", dA_, D, 0, 0.0, C.c_uint64(0), dW_, db_, dlab, dil, dll, B, T, D, CN, LMAX, SKIP, CN - 1, 1e-8, 1.0 / B,
                 o[0], o[1], 0, o[2], o[3], o[4], o[5], D, ws, ws.nbytes)
        return o

    guarded, roomy = _both(dev, dev.lib.mgr_head_ws_bytes(B, T, D, CN, LMAX), run)
    # P, loss, dLogits: equal bits (test_head_fwd_bwd_at_two_pairs_per_lane_equals_its_parts); dWd, dbd, dA: that test's bound
    # against the fp64 oracle
    assert all(_same_bits(a, b) for a, b in zip(guarded[:3], roomy[:3]))
    Pref, cache = kr.dense_softmax_forward(A.astype(np.float64), None, Wd.astype(np.float64), bd.astype(np.float64))
    ref_loss, ref_dz = kr.ctc_loss_grad(Pref, lab, il, ll, skip=SKIP, eps=1e-8)
    dAref, dWref, dbref = kr.dense_backward(ref_dz / B, cache)
    for got in (guarded, roomy):
        assert np.allclose(got[1], ref_loss, rtol=1e-4)
        for name, a, b in (("dWd", got[3], dWref), ("dbd", got[4], dbref), ("dA", got[5], dAref)):
            assert rel_err(a, b) < 5e-4, (name, rel_err(a, b))


def test_dense_bwd(device):
    dev = device
    A, Wd, bd, (dA_, dW_, db_) = _dense_inputs(dev)
    dL = np.random.default_rng(D).standard_normal((B, T, CN)).astype(f32)
    ddL = dev.array(dL)

    def run(ws):
        o = [_nan(dev, (D, CN)), _nan(dev, (CN,)), _nan(dev, (B, T, D))]
        dev.call("mgr_dense_bwd", dA_, D, 0, 0.0, C.c_uint64(0), ddL, dW_, o[0], o[1], o[2], D, B, T, D, CN, ws, ws.nbytes)
        return o

    guarded, roomy = _both(dev, dev.lib.mgr_dense_bwd_ws_bytes(B, T, D, CN), run)
    _, cache = kr.dense_softmax_forward(A.astype(np.float64), None, Wd.astype(np.float64), bd.astype(np.float64))
    dAref, dWref, dbref = kr.dense_backward(dL.astype(np.float64), cache)
    for got in (guarded, roomy):      # (test_dense_softmax_fwd_bwd's bound against the fp64 oracle)
        for name, a, b in (("dWd", got[0], dWref), ("dbd", got[1], dbref), ("dA", got[2], dAref)):
            assert rel_err(a, b) < 1e-5, (name, rel_err(a, b))


def test_ctc_align(device):
    dev = device
    P, lab, il, ll, arrs = _ctc_inputs(dev)

    def run(ws):
        o = [_nan(dev, (B, T - SKIP), np.int32), _nan(dev, (B, LMAX, 2), np.int32), _nan(dev, (B, LMAX)), _nan(dev, (B,), np.float64)]
        dev.call("mgr_ctc_align", *arrs, B, T, CN, LMAX, SKIP, CN - 1, C.c_float(1e-8), *o, ws, ws.nbytes)
        return o

    guarded, roomy = _both(dev, dev.lib.mgr_ctc_align_ws_bytes(B, T, CN, LMAX), run)
    assert np.isfinite(guarded[3]).all() and (guarded[1][0] >= 0).all()
    assert all(_same_bits(a, b) for a, b in zip(guarded, roomy))      # (test_forced_align_python_surface: equal between calls)


def test_ctc_beam_search(device):
    dev = device
    P, lab, il, ll, arrs = _ctc_inputs(dev)

    def run(ws):
        o = [_nan(dev, (B, T - SKIP), np.int32), _nan(dev, (B,), np.int32), _nan(dev, (B,), np.float64)]
        dev.call("mgr_ctc_beam_search", arrs[0], arrs[2], B, T, CN, SKIP, CN - 1, BEAM, C.c_float(1e-8), 0, *o, ws, ws.nbytes)
        return o

    guarded, roomy = _both(dev, dev.lib.mgr_ctc_beam_ws_bytes(B, T, CN, BEAM), run)
    assert (guarded[1] >= 0).all() and np.isfinite(guarded[2]).all()
    assert all(_same_bits(a, b) for a, b in zip(guarded, roomy))      # (tests/test_gpu_beam_lm.py: bit for bit between calls)


def test_ctc_beam_search_lm(device):
    dev = device
    P, lab, il, ll, arrs = _ctc_inputs(dev)
    NP = 3
    ext, fin = dev.zeros((CN + 1, CN), np.float64), dev.zeros((CN + 1,), np.float64)

    def run(ws):
        o = [_nan(dev, (B, NP, T - SKIP), np.int32), _nan(dev, (B, NP), np.int32), _nan(dev, (B, NP), np.float64), _nan(dev, (B, NP), np.float64)]
        dev.call("mgr_ctc_beam_search_lm", arrs[0], arrs[2], B, T, CN, SKIP, CN - 1, BEAM, C.c_float(1e-8), ext, fin, NP, *o, ws, ws.nbytes)
        return o

    guarded, roomy = _both(dev, dev.lib.mgr_ctc_beam_lm_ws_bytes(B, T, CN, BEAM, NP), run)
    assert (guarded[1][:, 0] >= 0).all() and np.isfinite(guarded[2][:, 0]).all()
    assert all(_same_bits(a, b) for a, b in zip(guarded, roomy))      # (tests/test_gpu_beam_lm.py: bit for bit between calls)
