"""-m gpu: the memory-bound passes of the training step's GEMM phase, through the C ABI - the narrow (depth-1) dropout-aware input
projection (gemm.hip), the two passes that write split rows along time and the gather of the per-sample weight-gradient tiles
(gemm_split.hip).  The passes move bytes; what they compute is small enough to be stated exactly: the split row format is compared
byte for byte with its numpy statement, and the weight gradients are formed from inputs on which f32 and split-f16 arithmetic are
exact in any order (small integers times powers of two), so dW / dU / db must equal the integer numpy result byte for byte - a
dropped, doubled or misplaced sample or time step cannot hide."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32


# ------------------------------------------------------------------------------------------------ narrow projection
def _proj_ref(X, M, W, bias):
    """fp64: Z[b, t, 4u + g] = (X[b, t] * M[g, b]) . W[:, 4u + g] + bias[4u + g]"""
    B, T, F = X.shape
    N = W.shape[1]
    gate = np.arange(N) % 4
    ref = np.empty((B, T, N))
    for g in range(4):
        ref[:, :, gate == g] = (X.astype(np.float64) * M[g][:, None, :]) @ W[:, gate == g].astype(np.float64) + bias[gate == g]
    return ref


def _narrow_mask(rng, B, F, p):
    c = f32(1.0 / (1.0 - p))
    M = ((rng.random((4, B, F)) >= p) * c).astype(f32)
    M[1, 0, :] = 0.0        # a (gate, sample) that keeps nothing
    M[2, B - 1, :] = c      # ... and one that keeps everything
    return M


@pytest.mark.parametrize("F,H,p,T", list(itertools.product((16, 20, 39, 59, 64), (100, 300, 500), (0.4, 0.6), (1900, 130))))
def test_narrow_projection_equals_generic_kernel_and_fp64(device, F, H, p, T):
    """mgr_lstm_input_proj_dropout on a row-major input with 16 <= F <= 64: Z byte-equal to the same call with tune key 11
    (MGR_TUNE_PROJ_WIDE_TILES) = 2, the generic kernel with 128-unit tiles, and within 2e-5 max(1, max |ref|) of the fp64 product."""
    dev = device
    B, N = 3, 4 * H
    rng = np.random.default_rng(F * 7919 + H * 31 + T + int(p * 10))
    X = rng.standard_normal((B, T, F)).astype(f32)
    W = (rng.standard_normal((F, N)) * 0.1).astype(f32)
    bias = rng.standard_normal(N).astype(f32)
    M = _narrow_mask(rng, B, F, p)
    dX, dW, db, dM = dev.array(X), dev.array(W), dev.array(bias), dev.array(M)
    ws = dev.bytes(dev.lib.mgr_lstm_input_proj_dropout_ws_bytes(B, F, H))
    dev.call("mgr_memset", ws, 0xFF, ws.nbytes)      # the workspace arrives dirty
    Z = dev.empty((B, T, N))
    outs = []
    try:
        for wide in (0, 2):
            dev.call("mgr_tune", 11, wide)
            Z.upload(np.full((B, T, N), np.nan, f32))
            dev.call("mgr_lstm_input_proj_dropout", dX, F, dM, p, dW, db, Z, B, T, F, H, ws, ws.nbytes)
            outs.append(Z.download())
    finally:
        dev.call("mgr_tune", 11, 0)
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    ref = _proj_ref(X, M, W, bias)
    err, tol = np.abs(outs[0] - ref).max(), 2e-5 * max(1.0, np.abs(ref).max())
    print("narrow projection F=%d H=%d p=%.1f T=%d: max |err| %.3e (bound %.3e)" % (F, H, p, T, err, tol))
    assert np.all(np.isfinite(outs[0])) and err <= tol
    # the (gate, sample) that keeps nothing is the bias alone
    assert np.array_equal(outs[0][0, :, 1::4], np.broadcast_to(bias[1::4], (T, H)))
    for a in (dX, dW, db, dM, ws, Z):
        a.free()


@pytest.mark.parametrize("F,H", [(39, 500), (20, 300), (59, 100)])
def test_narrow_projection_with_frozen_weights_follows_a_rewrite(device, F, H):
    """Weights declared frozen (mgr_weight_planes_cache(Wp, 1)) may be kept in any prepared form between calls; after
    mgr_weight_planes_cache(Wp, 0) and a rewrite the next call computes with the NEW weights - no stale copy."""
    dev = device
    B, T, p, N = 3, 130, 0.4, 4 * H
    rng = np.random.default_rng(F + H)
    X = rng.standard_normal((B, T, F)).astype(f32)
    W1 = (rng.standard_normal((F, N)) * 0.1).astype(f32)
    W2 = (rng.standard_normal((F, N)) * 0.3).astype(f32)
    bias = rng.standard_normal(N).astype(f32)
    M = _narrow_mask(rng, B, F, p)
    dX, dW, db, dM = dev.array(X), dev.array(W1), dev.array(bias), dev.array(M)
    ws = dev.bytes(dev.lib.mgr_lstm_input_proj_dropout_ws_bytes(B, F, H))
    Z = dev.empty((B, T, N))

    def proj():
        Z.upload(np.full((B, T, N), np.nan, f32))
        dev.call("mgr_lstm_input_proj_dropout", dX, F, dM, p, dW, db, Z, B, T, F, H, ws, ws.nbytes)
        return Z.download()

    z1 = proj()
    dev.call("mgr_weight_planes_cache", dW, 1)
    try:
        assert np.array_equal(proj(), z1) and np.array_equal(proj(), z1)
    finally:
        dev.call("mgr_weight_planes_cache", dW, 0)
    dW.upload(W2)
    z2 = proj()
    ref2 = _proj_ref(X, M, W2, bias)
    assert np.abs(z2 - ref2).max() <= 2e-5 * max(1.0, np.abs(ref2).max())
    dev.call("mgr_weight_planes_cache", dW, 1)          # ... and declared frozen again with the new weights: still theirs
    try:
        assert np.array_equal(proj(), z2) and np.array_equal(proj(), z2)
    finally:
        dev.call("mgr_weight_planes_cache", dW, 0)
    dW.upload(W1)
    assert np.array_equal(proj(), z1)
    for a in (dX, dW, db, dM, ws, Z):
        a.free()


# ------------------------------------------------------------------------------------------------ split rows along time
def _shifted(X, tshift):
    """entry t = X[:, t + tshift], zero where that step does not exist"""
    Xs = np.zeros_like(X)
    T = X.shape[1]
    if tshift == 0:
        Xs[:] = X
    elif tshift > 0:
        Xs[:, :T - tshift] = X[:, tshift:]
    else:
        Xs[:, -tshift:] = X[:, :T + tshift]
    return Xs


def _split_rows(X, ldt):
    """numpy statement of the split row format: row (b, f) = ldt f16 hi(t) | ldt f16 lo(t), hi = float16(x s), lo = float16(x s -
    float32(hi)), s = 2^13, round-to-nearest-even; zero in [T, ldt)"""
    B, T, F = X.shape
    xs = np.zeros((B, F, 2, ldt), np.float16)
    s = (X.transpose(0, 2, 1) * f32(8192.0)).astype(f32)
    hi = s.astype(np.float16)
    lo = (s - hi.astype(f32)).astype(np.float16)
    xs[:, :, 0, :T] = hi
    xs[:, :, 1, :T] = lo
    return xs.reshape(B, F, 2 * ldt).view(np.uint32)


@pytest.mark.parametrize("T,F,tshift", list(itertools.product((1, 7, 64, 130, 1900), (1, 63, 100, 200), (-1, 0, 1))))
def test_split_rows_along_time_match_the_row_format(device, T, F, tshift):
    """mgr_transpose_bt_split / mgr_transpose_bt_split_shift into a buffer full of NaN: byte-equal to the numpy statement of the
    format.  ldt takes values that are multiples of 8 only, of 128, and ones that leave a ragged last tile; F = 63 reads a padded
    input (ldx = 64)."""
    dev = device
    B = 2
    rng = np.random.default_rng(T * 131 + F * 7 + tshift + 1)
    ldx = 64 if F == 63 else F
    ldt = (T + 7) // 8 * 8 + 8 * (F % 3) if F != 100 else (T + 127) // 128 * 128
    Xp = rng.uniform(-7.9, 7.9, (B, T, ldx)).astype(f32)
    Xp.reshape(-1)[::5] = rng.integers(-8, 9, Xp.reshape(-1)[::5].shape).astype(f32) * f32(0.125)     # exact in f16: lo = 0
    Xp.reshape(-1)[::11] = (rng.standard_normal(Xp.reshape(-1)[::11].shape) * 1e-6).astype(f32)       # tiny: hi subnormal or zero
    Xp.reshape(-1)[::17] = f32(-0.0)
    X = np.ascontiguousarray(Xp[:, :, :F])
    dX = dev.array(Xp)
    XS = dev.empty((B, F, ldt))
    want = _split_rows(_shifted(X, tshift), ldt)
    calls = [("mgr_transpose_bt_split_shift", (tshift,))] + ([("mgr_transpose_bt_split", ())] if tshift == 0 else [])
    for name, extra in calls:
        XS.upload(np.full((B, F, ldt), np.nan, f32))
        dev.call(name, dX, ldx, XS, ldt, B, T, F, *extra)
        got = XS.download().view(np.uint32)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
    dX.free()
    XS.free()


# ------------------------------------------------------------------------------------------------ weight gradients, exactly
def _ints(rng, shape, zero_share=0.0):
    """k 2^-3 with |k| <= 8"""
    v = rng.integers(-8, 9, shape).astype(f32) * f32(0.125)
    if zero_share:
        v[rng.random(shape) < zero_share] = 0.0
    return v


def _grads_ref(X, M, Hs, dZ, reverse):
    """the integer result: dW[f, 4u + g] = sum_b M[g, b, f] sum_t X[b, t, f] dZ[b, t, 4u + g], dU[k] = sum_(b, t) h_prev[b, t, k] dZ[b, t],
    db = sum_(b, t) dZ[b, t] - every term a multiple of 2^-6 (times the mask's power of two), every sum exact in fp64 AND in f32"""
    N = dZ.shape[2]
    gate = np.arange(N) % 4
    dW = np.empty((X.shape[2], N))
    for g in range(4):
        dW[:, gate == g] = np.einsum("btf,btn->fn", X.astype(np.float64) * M[g][:, None, :], dZ[:, :, gate == g].astype(np.float64))
    hp = _shifted(Hs, 1 if reverse else -1).astype(np.float64)
    dU = np.einsum("btk,btn->kn", hp, dZ.astype(np.float64))
    db = dZ.astype(np.float64).sum(axis=(0, 1))
    for a in (dW, dU, db):
        assert np.array_equal(a.astype(f32).astype(np.float64), a)      # (the premise: representable in f32)
    # (+ 0.0: a sum that is zero is +0, as a sum of f32 adds that starts from +0 is, whatever order numpy took)
    return (dW + 0.0).astype(f32), (dU + 0.0).astype(f32), (db + 0.0).astype(f32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


@pytest.mark.parametrize("B,T,F,H,keep,factor,reverse", [(1, 130, 40, 20, 1.0, 1.0, 0), (1, 65, 64, 36, 0.5, 2.0, 1), (5, 77, 70, 100, 0.5, 4.0, 0),
                                                         (5, 130, 200, 17, 0.03, 0.5, 1), (64, 33, 32, 36, 0.5, 2.0, 1),
                                                         (64, 40, 130, 100, 0.03, 2.0, 0), (64, 9, 48, 20, 1.0, 0.25, 0)])
def test_weight_gradients_are_exact_on_exact_inputs(device, B, T, F, H, keep, factor, reverse):
    """mgr_lstm_param_grads_dropout_ts with every combination of dzmax / dbsum / proj_ws / HsT given or NULL: dW, dU and db equal the
    integer numpy result byte for byte.  The scaled split rows of dZ and the gather of the per-sample tiles are internal to the call;
    samples, time steps and kept features that went missing, came twice or landed elsewhere change an exact sum."""
    dev = device
    N = 4 * H
    rng = np.random.default_rng(B * 977 + T + F + H)
    X, Hs = _ints(rng, (B, T, F)), _ints(rng, (B, T, H))
    dZ = _ints(rng, (B, T, N), zero_share=0.3)
    dZ[0, :, 5] = 0.0                       # rows of dZ that are all zero: their scale comes from a maximum of 0
    dZ[B - 1, :, N - 1] = 0.0
    dZ[:, :, 8:12] = 0.0
    M = ((rng.random((4, B, F)) < keep) * f32(factor)).astype(f32)
    if keep == 1.0:
        M[:] = factor
    M[3, B // 2, :] = 0.0                   # a (gate, sample) that keeps nothing
    ldt = (T + 127) // 128 * 128
    dX, dH, dM, ddZ = dev.array(X), dev.array(Hs), dev.array(M), dev.array(dZ)
    XS, HsT = dev.empty((B, F, ldt)), dev.empty((B, H, ldt))
    dev.call("mgr_transpose_bt_split", dX, F, XS, ldt, B, T, F)
    dev.call("mgr_transpose_bt_split_shift", dH, H, HsT, ldt, B, T, H, 1 if reverse else -1)
    zmx = dev.array(np.abs(dZ).max(axis=1).astype(f32).view(np.uint32))
    zsm = dev.array(dZ.astype(np.float64).sum(axis=1).astype(f32))
    ws = dev.bytes(dev.lib.mgr_lstm_param_grads_dropout_ts_ws_bytes(B, T, F, H, ldt))
    # the projection of the same mask leaves its kept lists behind (proj_ws)
    pws = dev.bytes(dev.lib.mgr_lstm_input_proj_dropout_ts_ws_bytes(B, F, H))
    dev.call("mgr_memset", pws, 0xFF, pws.nbytes)
    Wp_, bp_, Z_ = dev.array(_ints(rng, (F, N))), dev.zeros((N,)), dev.empty((B, T, N))
    dev.call("mgr_lstm_input_proj_dropout_ts", XS, ldt, dM, 0.5, Wp_, bp_, Z_, B, T, F, H, pws, pws.nbytes)
    rW, rU, rb = _grads_ref(X, M, Hs, dZ, reverse)
    gW, gU, gb = dev.empty((F, N)), dev.empty((H, N)), dev.empty((N,))
    for use_max, use_sum, use_pws, use_hst in itertools.product((0, 1), repeat=4):
        for g in (gW, gU, gb):
            g.upload(np.full(g.shape, np.nan, f32))
        dev.call("mgr_memset", ws, 0xFF, ws.nbytes)          # the workspace arrives dirty
        dev.call("mgr_lstm_param_grads_dropout_ts", XS, ldt, dM, 0.5, dH, H, ddZ, gW, gU, gb, B, T, F, H, reverse, ws, ws.nbytes,
                 zmx if use_max else 0, zsm if use_sum else 0, pws if use_pws else 0, HsT if use_hst else 0)
        which = (use_max, use_sum, use_pws, use_hst)
        assert np.array_equal(_bits(gW.download()), _bits(rW)), ("dW", which)
        assert np.array_equal(_bits(gU.download()), _bits(rU)), ("dU", which)
        assert np.array_equal(_bits(gb.download()), _bits(rb)), ("db", which)
    for a in (dX, dH, dM, ddZ, XS, HsT, zmx, zsm, ws, pws, Wp_, bp_, Z_, gW, gU, gb):
        a.free()


def test_an_infinite_gate_gradient_stays_visible(device):
    """One Inf in dZ (gemm_split.hip, dw_zscale: the scale of such a row is NaN): the column of that (sample, unit, gate) is not
    finite in dU and db and in dW for every feature the sample kept for that gate; every other column is the exact result."""
    dev = device
    B, T, F, H, reverse = 5, 77, 70, 36, 0
    N = 4 * H
    rng = np.random.default_rng(77)
    X, Hs, dZ = _ints(rng, (B, T, F)), _ints(rng, (B, T, H)), _ints(rng, (B, T, N))
    X[X == 0] = f32(0.125)
    M = ((rng.random((4, B, F)) < 0.5) * f32(2.0)).astype(f32)
    b_inf, t_inf, col = 2, 40, 4 * 7 + 1
    clean = dZ.copy()
    dZ[b_inf, t_inf, col] = np.inf
    ldt = 128
    dX, dH, dM, ddZ = dev.array(X), dev.array(Hs), dev.array(M), dev.array(dZ)
    XS, HsT = dev.empty((B, F, ldt)), dev.empty((B, H, ldt))
    dev.call("mgr_transpose_bt_split", dX, F, XS, ldt, B, T, F)
    dev.call("mgr_transpose_bt_split_shift", dH, H, HsT, ldt, B, T, H, -1)
    ws = dev.bytes(dev.lib.mgr_lstm_param_grads_dropout_ts_ws_bytes(B, T, F, H, ldt))
    rW, rU, rb = _grads_ref(X, M, Hs, clean, reverse)
    other = np.arange(N) != col
    kept = M[1, b_inf] != 0
    gW, gU, gb = dev.empty((F, N)), dev.empty((H, N)), dev.empty((N,))
    for use_hst in (0, 1):
        dev.call("mgr_memset", ws, 0xFF, ws.nbytes)
        dev.call("mgr_lstm_param_grads_dropout_ts", XS, ldt, dM, 0.5, dH, H, ddZ, gW, gU, gb, B, T, F, H, reverse, ws, ws.nbytes, 0, 0, 0,
                 HsT if use_hst else 0)
        w, u, bb = gW.download(), gU.download(), gb.download()
        assert not np.isfinite(w[kept, col]).any() and not np.isfinite(u[:, col]).any() and not np.isfinite(bb[col])
        assert np.array_equal(_bits(w[~kept, col]), _bits(rW[~kept, col]))
        assert np.array_equal(_bits(w[:, other]), _bits(rW[:, other]))
        assert np.array_equal(_bits(u[:, other]), _bits(rU[:, other])) and np.array_equal(_bits(bb[other]), _bits(rb[other]))
    for a in (dX, dH, dM, ddZ, XS, HsT, ws, gW, gU, gb):
        a.free()
