"""-m gpu parity tests: every C-ABI kernel against the fp64 oracle on seeded inputs.
Tolerances: fp32 kernels vs fp64 oracle.  CTC loss 1e-4 relative (BASELINE.json north_star)."""
import ctypes as C

import numpy as np
import pytest

from oracle import keras_ref as kr
from tests.helpers import GOLDEN, rel_err

pytestmark = pytest.mark.gpu


def _rand_probs(rng, B, T, Cn, scale=2.0):
    z = rng.standard_normal((B, T, Cn)) * scale
    P = np.exp(z - z.max(-1, keepdims=True))
    return (P / P.sum(-1, keepdims=True)).astype(np.float32)


def _run_ctc(dev, P, labels, il, ll, skip=2, gscale=1.0, need_grad=True):
    B, T, Cn = P.shape
    Lmax = labels.shape[1]
    dP = dev.array(P)
    dl = dev.array(labels.astype(np.int32))
    dil = dev.array(np.asarray(il).reshape(B).astype(np.int32))
    dll = dev.array(np.asarray(ll).reshape(B).astype(np.int32))
    loss = dev.empty((B,))
    dz = dev.empty((B, T, Cn))
    wsb = dev.lib.mgr_ctc_ws_bytes(B, T, Cn, Lmax)
    ws = dev.bytes(wsb)
    dev.call("mgr_ctc_loss_grad", dP, dl, dil, dll, B, T, Cn, Lmax, skip, Cn - 1, 1e-8, gscale, loss,
             dz if need_grad else 0, ws, ws.nbytes)
    out = loss.download(), dz.download()
    for a in (dP, dl, dil, dll, loss, dz, ws):
        a.free()
    return out


def test_ctc_golden(device):
    z = np.load(GOLDEN + "/ctc_small.npz")
    loss, dz = _run_ctc(device, z["P"].astype(np.float32), z["labels"], z["input_length"], z["label_length"])
    assert np.allclose(loss, z["loss"], rtol=1e-5), (loss, z["loss"])
    assert rel_err(dz, z["dlogits"]) < 2e-4


@pytest.mark.parametrize("B,T,Cn,Lmax,lo,hi", [(4, 50, 22, 35, 1, 12), (3, 400, 22, 35, 8, 20), (2, 330, 44, 150, 100, 150),
                                               (2, 70, 22, 28, 1, 28), (1, 3, 5, 4, 1, 1)])
def test_ctc_random(device, B, T, Cn, Lmax, lo, hi):
    rng = np.random.default_rng(B * 1000 + T)
    P = _rand_probs(rng, B, T, Cn)
    labels = -np.ones((B, Lmax))
    ll = np.zeros(B, np.int64)
    for b in range(B):
        L = int(rng.integers(lo, hi + 1))
        L = min(L, (T - 2) // 2) if T > 4 else 1
        labels[b, :L] = rng.integers(0, Cn - 1, size=L)
        ll[b] = L
    il = np.full(B, T - 2)
    if B > 1:
        il[1] = max(2 * int(ll[1]) + 1, (T - 2) // 2)
    ref_loss, ref_dz = kr.ctc_loss_grad(P.astype(np.float64), labels, il, ll)
    loss, dz = _run_ctc(device, P, labels, il, ll)
    assert np.allclose(loss, ref_loss, rtol=1e-4), (loss, ref_loss)
    assert rel_err(dz, ref_dz) < 5e-4
    loss2, _ = _run_ctc(device, P, labels, il, ll, need_grad=False)
    assert np.array_equal(loss, loss2)
    # round 6: two samples per workgroup (one alpha / beta chain per SIMD; an odd batch leaves the last workgroup one sample) - tune key
    # 18 = 1 brings the one-sample workgroups back: the same arithmetic per sample, the same bits
    device.call("mgr_tune", 18, 1)
    try:
        loss1, dz1 = _run_ctc(device, P, labels, il, ll)
    finally:
        device.call("mgr_tune", 18, 0)
    assert np.array_equal(loss, loss1) and np.array_equal(dz, dz1)


def test_ctc_empty_label_sequence(device):
    """A sample without labels (TF's ctc_loss accepts it; the reference's generator never emits one): the single state is the
    blank, loss = - sum_t log y_t(blank) in closed form, and its neighbours in the batch are not disturbed."""
    rng = np.random.default_rng(11)
    for B, T, Cn, Lmax in ((3, 12, 6, 4), (2, 300, 22, 35)):
        P = _rand_probs(rng, B, T, Cn)
        labels = -np.ones((B, Lmax))
        labels[1, :2] = [1, 3]
        ll = np.zeros(B, np.int64)
        ll[1] = 2
        il = np.full(B, T - 2)
        ref_loss, ref_dz = kr.ctc_loss_grad(P.astype(np.float64), labels, il, ll)
        u = P[0, 2:2 + il[0]].astype(np.float64) + 1e-8
        closed = -np.log(u[:, Cn - 1] / u.sum(-1)).sum()
        assert abs(ref_loss[0] - closed) < 1e-9 * closed
        loss, dz = _run_ctc(device, P, labels, il, ll)
        assert np.allclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
        assert np.isfinite(dz).all() and rel_err(dz, ref_dz) < 5e-4


def test_ctc_label_sequence_that_does_not_fit_its_input(device):
    """tf.nn.ctc_loss raises for it; here (mgr.h) the sample's loss is +inf, its gradient zero, and its neighbour exact."""
    rng = np.random.default_rng(12)
    B, T, Cn, Lmax = 2, 6, 6, 4
    P = _rand_probs(rng, B, T, Cn)
    labels = -np.ones((B, Lmax))
    labels[0, :3] = [1, 1, 1]          # needs 5 frames, has T - 2 = 4
    labels[1, :2] = [1, 3]
    ll, il = np.array([3, 2]), np.full(B, T - 2)
    ref_loss, ref_dz = kr.ctc_loss_grad(P.astype(np.float64), labels, il, ll)
    loss, dz = _run_ctc(device, P, labels, il, ll)
    assert np.isinf(loss[0]) and loss[0] > 0 and np.isinf(ref_loss[0])
    assert np.isfinite(dz).all() and not dz[0].any()
    assert np.allclose(loss[1], ref_loss[1], rtol=1e-5) and rel_err(dz[1], ref_dz[1]) < 5e-4


def test_ctc_long_T_relative(device):
    """BASELINE shape T=1900 (B reduced): loss ~ thousands, must match 1e-4 relative."""
    rng = np.random.default_rng(5)
    B, T, Cn, Lmax = 2, 1900, 22, 35
    P = _rand_probs(rng, B, T, Cn, scale=1.0)
    labels = -np.ones((B, Lmax))
    ll = np.array([20, 8])
    for b in range(B):
        labels[b, :ll[b]] = rng.integers(0, Cn - 1, size=ll[b])
    il = np.full(B, T - 2)
    ref_loss, ref_dz = kr.ctc_loss_grad(P.astype(np.float64), labels, il, ll)
    loss, dz = _run_ctc(device, P, labels, il, ll)
    assert np.allclose(loss, ref_loss, rtol=1e-4), (loss, ref_loss)
    assert rel_err(dz, ref_dz) < 2e-3


@pytest.mark.parametrize("B,T,D,Cn,p", [(3, 37, 200, 22, 0.5), (2, 65, 1000, 44, 0.0), (1, 5, 8, 6, 0.5)])
def test_dense_softmax_fwd_bwd(device, B, T, D, Cn, p):
    dev = device
    rng = np.random.default_rng(D)
    A = rng.standard_normal((B, T, D)).astype(np.float32)
    Wd = (rng.standard_normal((D, Cn)) * 0.1).astype(np.float32)
    bd = rng.standard_normal(Cn).astype(np.float32)
    dm = ((rng.random((B, T, D)) >= p) / (1 - p)).astype(np.float32) if p > 0 else None
    dL = rng.standard_normal((B, T, Cn)).astype(np.float32)
    Pref, cache = kr.dense_softmax_forward(A.astype(np.float64), None if dm is None else dm.astype(np.float64),
                                           Wd.astype(np.float64), bd.astype(np.float64))
    dAref, dWref, dbref = kr.dense_backward(dL.astype(np.float64), cache)
    dA_, dW_, db_, dP_ = dev.array(A), dev.array(Wd), dev.array(bd), dev.empty((B, T, Cn))
    dmask = dev.array(dm) if dm is not None else 0
    dev.call("mgr_dense_softmax_fwd", dA_, D, dmask, 0.0, C.c_uint64(0), dW_, db_, dP_, B, T, D, Cn)
    assert rel_err(dP_.download(), Pref) < 1e-5
    gW, gb, gA, ddL = dev.empty((D, Cn)), dev.empty((Cn,)), dev.empty((B, T, D)), dev.array(dL)
    ws = dev.bytes(dev.lib.mgr_dense_bwd_ws_bytes(B, T, D, Cn))
    dev.call("mgr_dense_bwd", dA_, D, dmask, 0.0, C.c_uint64(0), ddL, dW_, gW, gb, gA, D, B, T, D, Cn, ws, ws.nbytes)
    assert rel_err(gW.download(), dWref) < 1e-5
    assert rel_err(gb.download(), dbref) < 1e-5
    assert rel_err(gA.download(), dAref) < 1e-5


def test_dense_device_rng_mask_consistent(device):
    """In-kernel dropout (seed) must equal mgr_dropout_mask's mask, in forward and backward."""
    dev = device
    B, T, D, Cn, p, seed = 2, 33, 200, 22, 0.5, 77
    rng = np.random.default_rng(1)
    A = rng.standard_normal((B, T, D)).astype(np.float32)
    Wd = (rng.standard_normal((D, Cn)) * 0.1).astype(np.float32)
    bd = np.zeros(Cn, np.float32)
    m = dev.empty((B, T, D))
    dev.call("mgr_dropout_mask", m, m.size, p, C.c_uint64(seed))
    mh = m.download()
    assert set(np.unique(mh)) <= {0.0, 2.0} and 0.4 < (mh > 0).mean() < 0.6
    dA_, dW_, db_ = dev.array(A), dev.array(Wd), dev.array(bd)
    P1, P2 = dev.empty((B, T, Cn)), dev.empty((B, T, Cn))
    dev.call("mgr_dense_softmax_fwd", dA_, D, m, 0.0, C.c_uint64(0), dW_, db_, P1, B, T, D, Cn)
    dev.call("mgr_dense_softmax_fwd", dA_, D, 0, p, C.c_uint64(seed), dW_, db_, P2, B, T, D, Cn)
    assert np.array_equal(P1.download(), P2.download())


def _lstm_case(rng, B, T, F, H, p):
    x = rng.standard_normal((B, T, F))
    W = rng.uniform(-0.3, 0.3, (F, 4 * H))
    U = rng.uniform(-0.4, 0.4, (H, 4 * H))
    b = rng.uniform(-0.2, 0.2, 4 * H)
    mask = ((rng.random((4, B, F)) >= p) / (1 - p)) if p > 0 else None
    return x, W, U, b, mask


@pytest.mark.parametrize("B,T,F,H,p", [(3, 12, 5, 8, 0.4), (17, 9, 39, 32, 0.5), (5, 21, 20, 100, 0.0), (2, 7, 1600, 100, 0.5),
                                       (3, 6, 30, 128, 0.5), (5, 8, 13, 12, 0.5), (2, 5, 600, 300, 0.6), (2, 4, 64, 500, 0.4)])
@pytest.mark.parametrize("reverse", [0, 1])
def test_lstm_direction_fwd_bwd(device, B, T, F, H, p, reverse):
    """input projection (MFMA GEMM) + scan fwd + scan bwd + parameter / input grads for one direction."""
    dev = device
    rng = np.random.default_rng(B * 100 + T * 10 + H + reverse)
    x, W, U, b, mask = _lstm_case(rng, B, T, F, H, p)
    y_ref, cache = kr.lstm_forward(x, W, U, b, mask, bool(reverse))
    dy = rng.standard_normal((B, T, H))
    dx_ref, dW_ref, dU_ref, db_ref = kr.lstm_backward(dy, cache, need_dx=True)

    f32 = np.float32
    dX = dev.array(x.astype(f32))
    dmask = dev.array(mask.astype(f32)) if mask is not None else 0
    Wk, Uk, bk = dev.array(W.astype(f32)), dev.array(U.astype(f32)), dev.array(b.astype(f32))
    Wp, Up, bp = dev.empty((F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
    dev.call("mgr_lstm_pack", Wk, Wp, F, H, 0)
    dev.call("mgr_lstm_pack", Uk, Up, H, H, 0)
    dev.call("mgr_lstm_pack", bk, bp, 1, H, 0)
    Z = dev.empty((B, T, 4 * H))
    dev.call("mgr_lstm_input_proj", dX, F, dmask, Wp, bp, Z, B, T, F, H)
    Y, G, Cs = dev.empty((B, T, H)), dev.empty((B, T, H, 4)), dev.empty((B, T, H))
    ws0 = dev.bytes(dev.lib.mgr_lstm_scan_ws_bytes(B, T, H)); dev.call("mgr_lstm_scan_fwd", Z, Up, Y, H, 0, 0, G, Cs, B, T, H, reverse, ws0, ws0.nbytes)
    y = Y.download()
    assert rel_err(y, y_ref) < 2e-5, rel_err(y, y_ref)
    assert rel_err(Cs.download(), cache["c"]) < 2e-5
    g = G.download()
    assert rel_err(g[..., 0], cache["i"]) < 2e-5 and rel_err(g[..., 2], cache["g"]) < 2e-5

    ddY, dZ = dev.array(dy.astype(f32)), dev.empty((B, T, 4 * H))
    ws = dev.bytes(dev.lib.mgr_lstm_scan_ws_bytes(B, T, H))
    dev.call("mgr_lstm_scan_bwd", ddY, H, G, Cs, Up, dZ, B, T, H, reverse, ws, ws.nbytes)
    gW, gU, gb = dev.empty((F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
    ws2 = dev.bytes(dev.lib.mgr_lstm_param_grads_ws_bytes(B, T, F, H))
    dev.call("mgr_lstm_param_grads", dX, F, dmask, Y, H, dZ, gW, gU, gb, B, T, F, H, reverse, ws2, ws2.nbytes)
    gWk, gUk, gbk = dev.empty((F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
    dev.call("mgr_lstm_pack", gW, gWk, F, H, 1)
    dev.call("mgr_lstm_pack", gU, gUk, H, H, 1)
    dev.call("mgr_lstm_pack", gb, gbk, 1, H, 1)
    assert rel_err(gWk.download(), dW_ref) < 1e-4
    assert rel_err(gUk.download(), dU_ref) < 1e-4
    assert rel_err(gbk.download(), db_ref) < 1e-4
    gX = dev.empty((B, T, F))
    dev.call("mgr_lstm_input_grad", dZ, Wp, dmask, gX, F, 0, B, T, F, H)
    assert rel_err(gX.download(), dx_ref) < 1e-4
    dev.call("mgr_lstm_input_grad", dZ, Wp, dmask, gX, F, 1, B, T, F, H)
    assert rel_err(gX.download(), 2 * dx_ref) < 1e-4


def test_scan_residual_and_strides(device):
    """Y written with a row stride / column offset and a residual source (multimodal.py:111,155)."""
    dev = device
    rng = np.random.default_rng(3)
    B, T, F, H = 3, 7, 6, 8
    x, W, U, b, _ = _lstm_case(rng, B, T, F, H, 0.0)
    y_ref, _ = kr.lstm_forward(x, W, U, b, None, False)
    R = rng.standard_normal((B, T, 2 * H)).astype(np.float32)
    f32 = np.float32
    Wp, Up, bp = dev.empty((F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
    dev.call("mgr_lstm_pack", dev.array(W.astype(f32)), Wp, F, H, 0)
    dev.call("mgr_lstm_pack", dev.array(U.astype(f32)), Up, H, H, 0)
    dev.call("mgr_lstm_pack", dev.array(b.astype(f32)), bp, 1, H, 0)
    Z = dev.empty((B, T, 4 * H))
    dev.call("mgr_lstm_input_proj", dev.array(x.astype(f32)), F, 0, Wp, bp, Z, B, T, F, H)
    ld = 3 * H + 4
    OUT = dev.zeros((B, T, ld))
    dR = dev.array(R)
    ws0 = dev.bytes(dev.lib.mgr_lstm_scan_ws_bytes(B, T, H)); dev.call("mgr_lstm_scan_fwd", Z, Up, OUT.view(H, (1,)), ld, dR.view(H, (1,)), 2 * H, 0, 0, B, T, H, 0, ws0, ws0.nbytes)
    out = OUT.download()
    assert rel_err(out[:, :, H:2 * H], y_ref + R[:, :, H:]) < 2e-5
    assert np.all(out[:, :, :H] == 0) and np.all(out[:, :, 2 * H:] == 0)


def test_adam_maxnorm_noise_argmax(device):
    dev = device
    rng = np.random.default_rng(9)
    n = 1003
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 2).astype(np.float32)
    m = rng.standard_normal(n).astype(np.float32) * 0.1
    v = rng.random(n).astype(np.float32) * 0.1
    pr, mr, vr = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    lr_t = kr.adam_lr_t(1e-4, 1e-5, 7)
    kr.adam_step(pr, g.astype(np.float64), mr, vr, lr_t, clipvalue=0.5, gscale=0.5)
    dp, dg, dm, dv = dev.array(p), dev.array(g), dev.array(m), dev.array(v)
    dev.call("mgr_adam_step", dp, dg, dm, dv, n, lr_t, 0.9, 0.999, 1e-7, 0.5, 0.5)
    assert rel_err(dp.download(), pr) < 1e-6 and rel_err(dm.download(), mr) < 1e-6 and rel_err(dv.download(), vr) < 1e-6
    W = (rng.standard_normal((37, 45)) * 1.2).astype(np.float32)
    Wr = W.astype(np.float64)
    kr.maxnorm_cols(Wr, 3.0)
    dW = dev.array(W)
    dev.call("mgr_maxnorm_cols", dW, 37, 45, 3.0, 1e-7)
    assert rel_err(dW.download(), Wr) < 1e-6
    x = np.zeros(200001, np.float32)
    dx, dyv = dev.array(x), dev.empty((200001,))
    dev.call("mgr_add_gaussian_noise", dx, dyv, x.size, 0.5, C.c_uint64(5))
    yv = dyv.download()
    assert abs(yv.mean()) < 0.01 and abs(yv.std() - 0.5) < 0.01
    P = _rand_probs(rng, 3, 17, 22)
    P[0, 5, 3] = P[0, 5, 7] = 0.9  # tie: first index wins
    best, prob = dev.empty((3, 15), np.int32), dev.empty((3, 15))
    dev.call("mgr_frame_argmax", dev.array(P), 3, 17, 22, 2, best, prob)
    assert np.array_equal(best.download(), P[:, 2:].argmax(-1)) and np.array_equal(prob.download(), P[:, 2:].max(-1))


@pytest.mark.parametrize("B,T,H,path", [(5, 9, 32, 3), (33, 6, 32, 3), (17, 7, 100, 3), (17, 7, 100, 4), (20, 5, 300, 0), (40, 7, 32, 5), (64, 6, 100, 5), (33, 5, 500, 5), (64, 4, 300, 5),
                                        (18, 5, 500, 0), (64, 4, 500, 3), (3, 6, 12, 3),
                                        (5, 1, 100, 0), (17, 2, 500, 0), (33, 1, 300, 0), (64, 2, 128, 0), (16, 1, 500, 0)])   # T = 1, 2: no / one hand-off
def test_cluster_scan_matches_oracle(device, B, T, H, path):
    """Persistent multi-CU scan (per-step sc1 hand-off between workgroups) vs the oracle, both directions in ONE launch."""
    from mgr_amd import _capi
    dev = device
    rng = np.random.default_rng(H + B)
    F = 6
    f32 = np.float32
    jobs, refs, outs, keep = [], [], [], []
    for reverse in (0, 1):
        x, W, U, b, _ = _lstm_case(rng, B, T, F, H, 0.0)
        U = U * (0.1 if H >= 300 else 1.0)
        y_ref, cache = kr.lstm_forward(x, W, U, b, None, bool(reverse))
        Wp, Up, bp = dev.empty((F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
        dev.call("mgr_lstm_pack", dev.array(W.astype(f32)), Wp, F, H, 0)
        dev.call("mgr_lstm_pack", dev.array(U.astype(f32)), Up, H, H, 0)
        dev.call("mgr_lstm_pack", dev.array(b.astype(f32)), bp, 1, H, 0)
        Z = dev.empty((B, T, 4 * H))
        dev.call("mgr_lstm_input_proj", dev.array(x.astype(f32)), F, 0, Wp, bp, Z, B, T, F, H)
        Y, G, Cs = dev.empty((B, T, H)), dev.empty((B, T, H, 4)), dev.empty((B, T, H))
        jobs.append(dict(Z=Z, Up=Up, Y=Y, ldy=H, R=0, ldr=0, gates=G, cs=Cs, B=B, T=T, H=H, reverse=reverse))
        refs.append((y_ref, cache))
        outs.append((Y, G, Cs))
        keep += [Wp, Up, bp, Z]
    dev.call("mgr_tune", 0, path)
    dev.call("mgr_tune", 1, 1)  # synchronous give-up check
    try:
        arr = _capi.make_scan_jobs(jobs)
        ws = dev.bytes(dev.lib.mgr_lstm_scan_multi_ws_bytes(2, arr))
        for rep in range(2):  # second launch re-uses the (re-zeroed) flags
            _capi.check(dev.lib.mgr_lstm_scan_fwd_multi(dev.ctx, 2, arr, ws.ptr, ws.nbytes))
            for (Y, G, Cs), (y_ref, cache) in zip(outs, refs):
                assert rel_err(Y.download(), y_ref) < 3e-5
                assert rel_err(Cs.download(), cache["c"]) < 3e-5
                assert rel_err(G.download()[..., 3], cache["o"]) < 3e-5
    finally:
        dev.call("mgr_tune", 0, 0)
        dev.call("mgr_tune", 1, 0)


@pytest.mark.parametrize("H,B,T", [(100, 17, 40), (300, 33, 25), (500, 64, 30)])
def test_cluster_step_variants_agree(device, H, B, T):
    """One-tile-per-wave clusters: the K-split step (default: blocks gathered straight into registers) and the LDS-image step
    (mgr_tune key 7) compute the same recurrence; both against the oracle, over enough steps to cycle the epoch parity many times."""
    from mgr_amd import _capi
    dev = device
    rng = np.random.default_rng(H)
    F = 5
    f32 = np.float32
    x, W, U, b, _ = _lstm_case(rng, B, T, F, H, 0.0)
    U = U * (0.1 if H >= 300 else 1.0)
    got = {}
    y_ref, _ = kr.lstm_forward(x, W, U, b, None, False)
    Wp, Up, bp = dev.empty((F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
    dev.call("mgr_lstm_pack", dev.array(W.astype(f32)), Wp, F, H, 0)
    dev.call("mgr_lstm_pack", dev.array(U.astype(f32)), Up, H, H, 0)
    dev.call("mgr_lstm_pack", dev.array(b.astype(f32)), bp, 1, H, 0)
    Z = dev.empty((B, T, 4 * H))
    dev.call("mgr_lstm_input_proj", dev.array(x.astype(f32)), F, 0, Wp, bp, Z, B, T, F, H)
    ws = dev.bytes(dev.lib.mgr_lstm_scan_ws_bytes(B, T, H))
    dev.call("mgr_tune", 0, 3)
    dev.call("mgr_tune", 1, 1)
    try:
        for variant in (0, 1):
            dev.call("mgr_tune", 7, variant)
            Y = dev.zeros((B, T, H))
            dev.call("mgr_lstm_scan_fwd", Z, Up, Y, H, 0, 0, 0, 0, B, T, H, 0, ws, ws.nbytes)
            got[variant] = Y.download()
            assert rel_err(got[variant], y_ref) < 3e-5, variant
        assert rel_err(got[0], got[1]) < 1e-5
        import ctypes
        st = ctypes.c_uint(7)
        dev.call("mgr_scan_status", ctypes.byref(st))     # no persistent scan of this context ever gave up
        assert st.value == 0
    finally:
        dev.call("mgr_tune", 7, 0)
        dev.call("mgr_tune", 0, 0)
        dev.call("mgr_tune", 1, 0)


@pytest.mark.parametrize("path", [1, 2, 3])
def test_scan_paths_agree(device, path):
    """fallback (1), single-CU (2) and 4-tile clusters (3) give the same recurrence (tolerance: fp32 summation order)."""
    dev = device
    rng = np.random.default_rng(11)
    B, T, F, H = 19, 11, 7, 100
    x, W, U, b, _ = _lstm_case(rng, B, T, F, H, 0.0)
    y_ref, _ = kr.lstm_forward(x, W, U, b, None, True)
    f32 = np.float32
    Wp, Up, bp = dev.empty((F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
    dev.call("mgr_lstm_pack", dev.array(W.astype(f32)), Wp, F, H, 0)
    dev.call("mgr_lstm_pack", dev.array(U.astype(f32)), Up, H, H, 0)
    dev.call("mgr_lstm_pack", dev.array(b.astype(f32)), bp, 1, H, 0)
    Z = dev.empty((B, T, 4 * H))
    dev.call("mgr_lstm_input_proj", dev.array(x.astype(f32)), F, 0, Wp, bp, Z, B, T, F, H)
    Y = dev.zeros((B, T, H))
    ws = dev.bytes(dev.lib.mgr_lstm_scan_ws_bytes(B, T, H))
    dev.call("mgr_tune", 0, path)
    dev.call("mgr_tune", 1, 1)
    try:
        dev.call("mgr_lstm_scan_fwd", Z, Up, Y, H, 0, 0, 0, 0, B, T, H, 1, ws, ws.nbytes)
        assert rel_err(Y.download(), y_ref) < 3e-5
    finally:
        dev.call("mgr_tune", 0, 0)
        dev.call("mgr_tune", 1, 0)


@pytest.mark.parametrize("B,T,H,path", [(5, 9, 32, 0), (33, 6, 100, 0), (17, 7, 128, 0), (20, 5, 16, 0), (3, 6, 8, 0), (19, 8, 100, 2), (18, 5, 300, 0), (33, 4, 500, 0),
                                        (7, 1, 100, 0), (20, 2, 500, 0), (33, 1, 300, 0), (64, 2, 128, 0)])   # T = 1, 2
@pytest.mark.parametrize("f32_mfma", [0, 1])
def test_bwd_multi_matches_oracle(device, B, T, H, path, f32_mfma):
    """BPTT of both directions in one call (multi-CU clusters exchanging dz_t when path == 0) vs the oracle - with the partial
    products on the f16 matrix pipe (split-f16 operands, the default) and on the f32 matrix instruction (tune key 14 = 1)."""
    from mgr_amd import _capi
    dev = device
    rng = np.random.default_rng(H * 7 + B)
    F = 5
    f32 = np.float32
    jobs, refs, outs = [], [], []
    for reverse in (0, 1):
        x, W, U, b, _ = _lstm_case(rng, B, T, F, H, 0.0)
        y_ref, cache = kr.lstm_forward(x, W, U, b, None, bool(reverse))
        dy = rng.standard_normal((B, T, 2 * H))[:, :, reverse * H:(reverse + 1) * H]
        # reference dZ in packed order: recompute from the oracle's backward internals via dW = x^T dz ... use dx instead
        dx_ref, dW_ref, dU_ref, db_ref = kr.lstm_backward(np.ascontiguousarray(dy), cache, need_dx=True)
        Wp, Up, bp = dev.empty((F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
        dev.call("mgr_lstm_pack", dev.array(W.astype(f32)), Wp, F, H, 0)
        dev.call("mgr_lstm_pack", dev.array(U.astype(f32)), Up, H, H, 0)
        dev.call("mgr_lstm_pack", dev.array(b.astype(f32)), bp, 1, H, 0)
        dX = dev.array(x.astype(f32))
        Z = dev.empty((B, T, 4 * H))
        dev.call("mgr_lstm_input_proj", dX, F, 0, Wp, bp, Z, B, T, F, H)
        Y, G, Cs = dev.empty((B, T, H)), dev.empty((B, T, H, 4)), dev.empty((B, T, H))
        ws0 = dev.bytes(dev.lib.mgr_lstm_scan_ws_bytes(B, T, H))
        dev.call("mgr_lstm_scan_fwd", Z, Up, Y, H, 0, 0, G, Cs, B, T, H, reverse, ws0, ws0.nbytes)
        dYd = dev.array(np.ascontiguousarray(dy).astype(f32))
        dZ = dev.empty((B, T, 4 * H))
        zm = dev.array(np.full((B, 4 * H), 0xFFFFFFFF, np.uint32))     # dirty: the call must write every word
        zs = dev.array(np.full((B, 4 * H), np.nan, f32))
        jobs.append(dict(dY=dYd, gates=G, cs=Cs, Up=Up, dZ=dZ, lddy=H, B=B, T=T, H=H, reverse=reverse, dzmax=zm, dbsum=zs))
        refs.append((dx_ref, dW_ref, dU_ref, db_ref))
        outs.append((dX, Y, dZ, Wp))
    dev.call("mgr_tune", 0, path)
    dev.call("mgr_tune", 1, 1)
    dev.call("mgr_tune", 14, f32_mfma)
    try:
        arr = _capi.make_scan_bwd_jobs(jobs)
        ws = dev.bytes(dev.lib.mgr_lstm_scan_bwd_multi_ws_bytes(2, arr))
        for rep in range(2):
            _capi.check(dev.lib.mgr_lstm_scan_bwd_multi(dev.ctx, 2, arr, ws.ptr, ws.nbytes))
            for reverse, ((dX, Y, dZ, Wp), (dx_ref, dW_ref, dU_ref, db_ref)) in enumerate(zip(outs, refs)):
                # mgr_scan_bwd_job.dzmax: the largest |dZ| over time per (sample, gate column), whatever kernel family ran
                zm = jobs[reverse]["dzmax"].download().view(np.float32)
                assert np.array_equal(zm, np.abs(dZ.download()).max(axis=1))
                # mgr_scan_bwd_job.dbsum: the sums of dZ over time (the bias gradient per sample), f32 sums in the kernel's own order
                dz64 = dZ.download().astype(np.float64)
                zs = jobs[reverse]["dbsum"].download()
                assert np.all(np.abs(zs - dz64.sum(axis=1)) <= 1e-6 * np.abs(dz64).sum(axis=1) + 1e-30)
                gW, gU, gb = dev.empty((F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
                ws2 = dev.bytes(dev.lib.mgr_lstm_param_grads_ws_bytes(B, T, F, H))
                dev.call("mgr_lstm_param_grads", dX, F, 0, Y, H, dZ, gW, gU, gb, B, T, F, H, reverse, ws2, ws2.nbytes)
                gUk = dev.empty((H, 4 * H))
                dev.call("mgr_lstm_pack", gU, gUk, H, H, 1)
                assert rel_err(gUk.download(), dU_ref) < 1e-4
                gX = dev.empty((B, T, F))
                dev.call("mgr_lstm_input_grad", dZ, Wp, 0, gX, F, 0, B, T, F, H)
                assert rel_err(gX.download(), dx_ref) < 1e-4
        if f32_mfma == 0 and path == 0 and 16 < H <= 128:
            # narrow layers have three forms of the split-f16 step (mgr.h, tune key 16): the one trimmed along its dependent chain (what ran
            # above) and the one the engine asks for beside other persistent launches - same results bit for bit
            lean = [(o[2].download(), np.concatenate([j["dzmax"].download(), j["dbsum"].download().view(np.uint32)])) for o, j in zip(outs, jobs)]
            both = lambda j: np.concatenate([j["dzmax"].download(), j["dbsum"].download().view(np.uint32)])
            for form in (1, 2):      # 1: the form that yields to co-resident scans, 2: the direct gather (one barrier per step)
                dev.call("mgr_tune", 16, form)
                _capi.check(dev.lib.mgr_lstm_scan_bwd_multi(dev.ctx, 2, arr, ws.ptr, ws.nbytes))
                for (dz0, zm0), o, j in zip(lean, outs, jobs):
                    assert np.array_equal(o[2].download(), dz0) and np.array_equal(both(j), zm0), form
            dev.call("mgr_tune", 16, 0)
            # round 6: the form as an ARGUMENT of the launch (mgr_scan_launch_opts) - every named form, and the FUSED forms (8-wave
            # workgroups that run two unit groups of their cluster, a CU each; an odd group count leaves a half that only keeps the
            # barrier count): the same bits again
            import ctypes
            n0 = ctypes.c_int()
            for form in (_capi.BPTT_FORM_TRIMMED, _capi.BPTT_FORM_YIELDING, _capi.BPTT_FORM_DIRECT, _capi.BPTT_FORM_FUSED, _capi.BPTT_FORM_FUSED_DIRECT):
                for o in outs:
                    o[2].zero()
                seq = ctypes.c_uint(0)
                opts = _capi.make_launch_opts(form, ctypes.addressof(seq))
                _capi.check(dev.lib.mgr_lstm_scan_bwd_multi_ex(dev.ctx, 2, arr, ws.ptr, ws.nbytes, ctypes.byref(opts)))
                dev.call("mgr_persist_stats", ctypes.byref(n0), None)
                assert seq.value == n0.value          # (the launch number the call reports is the context's newest)
                for (dz0, zm0), o, j in zip(lean, outs, jobs):
                    assert np.array_equal(o[2].download(), dz0) and np.array_equal(both(j), zm0), form
            # the SINGLE-CU form (lstm_cu_bwd.hip: one workgroup per (direction, 16-sample group), no inter-CU exchange): the same
            # arithmetic in another summation order - equal to the multi-CU forms to rounding, its row maxima exact for ITS dZ
            if H in (32, 64, 100):
                for o in outs:
                    o[2].zero()
                seq = ctypes.c_uint(0)
                opts = _capi.make_launch_opts(_capi.BPTT_FORM_SINGLE_CU, ctypes.addressof(seq))
                _capi.check(dev.lib.mgr_lstm_scan_bwd_multi_ex(dev.ctx, 2, arr, ws.ptr, ws.nbytes, ctypes.byref(opts)))
                assert seq.value == _capi.SEQ_NONE          # (no exchange: nothing enters the residency ledger)
                for (dz0, zm0), o, j in zip(lean, outs, jobs):
                    dz1 = o[2].download()
                    assert np.isfinite(dz1).all() and rel_err(dz1, dz0) < 2e-5, rel_err(dz1, dz0)
                    assert np.array_equal(j["dzmax"].download().view(np.float32), np.abs(dz1).max(axis=1))
                    d64 = dz1.astype(np.float64)
                    assert np.all(np.abs(j["dbsum"].download() - d64.sum(axis=1)) <= 1e-6 * np.abs(d64).sum(axis=1) + 1e-30)
    finally:
        dev.call("mgr_tune", 16, 0)
        dev.call("mgr_tune", 14, 0)
        dev.call("mgr_tune", 0, 0)
        dev.call("mgr_tune", 1, 0)


@pytest.mark.parametrize("H,B,T", [(100, 17, 12), (300, 33, 8)])
def test_contiguous_cluster_ids_match_oracle_and_the_octet_layout(device, H, B, T):
    """Tune key 3 = 1: the clusters of the K-split scans and of the multi-CU BPTT sit on CONTIGUOUS workgroup ids (what a batch beyond
    256 takes as well) instead of XCD-local octets - the other branch of every kernel's walk over the job table.  Both directions in one
    forward call with the states saved, BPTT over them: against the oracle, and bit for bit what the octet layout gives (placement is
    speed, never arithmetic).  H = 100: seven unit groups, an odd count."""
    import ctypes
    from mgr_amd import _capi
    dev = device
    rng = np.random.default_rng(H * 3 + B)
    F = 5
    f32 = np.float32
    fj, bj, refs, keep = [], [], [], []
    for reverse in (0, 1):
        x, W, U, b, _ = _lstm_case(rng, B, T, F, H, 0.0)
        U = U * (0.1 if H >= 300 else 1.0)
        y_ref, cache = kr.lstm_forward(x, W, U, b, None, bool(reverse))
        dy = np.ascontiguousarray(rng.standard_normal((B, T, H)))
        dx_ref, dW_ref, dU_ref, db_ref = kr.lstm_backward(dy, cache, need_dx=True)
        Wp, Up, bp = dev.empty((F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
        dev.call("mgr_lstm_pack", dev.array(W.astype(f32)), Wp, F, H, 0)
        dev.call("mgr_lstm_pack", dev.array(U.astype(f32)), Up, H, H, 0)
        dev.call("mgr_lstm_pack", dev.array(b.astype(f32)), bp, 1, H, 0)
        dX = dev.array(x.astype(f32))
        Z = dev.empty((B, T, 4 * H))
        dev.call("mgr_lstm_input_proj", dX, F, 0, Wp, bp, Z, B, T, F, H)
        Y, G, Cs, dZ = dev.empty((B, T, H)), dev.empty((B, T, H, 4)), dev.empty((B, T, H)), dev.empty((B, T, 4 * H))
        fj.append(dict(Z=Z, Up=Up, Y=Y, ldy=H, R=0, ldr=0, gates=G, cs=Cs, B=B, T=T, H=H, reverse=reverse))
        bj.append(dict(dY=dev.array(dy.astype(f32)), gates=G, cs=Cs, Up=Up, dZ=dZ, lddy=H, B=B, T=T, H=H, reverse=reverse))
        refs.append((y_ref, cache, dx_ref, dU_ref))
        keep += [Wp, bp, dX]
    farr, barr = _capi.make_scan_jobs(fj), _capi.make_scan_bwd_jobs(bj)
    fws = dev.bytes(dev.lib.mgr_lstm_scan_multi_ws_bytes(2, farr))
    bws = dev.bytes(dev.lib.mgr_lstm_scan_bwd_multi_ws_bytes(2, barr))
    nan = np.full((B, T, 4 * H), np.nan, f32)
    got = {}
    dev.call("mgr_tune", 1, 1)  # synchronous give-up check
    try:
        for contiguous in (0, 1):
            dev.call("mgr_tune", 3, contiguous)
            for f, bw in zip(fj, bj):      # dirty outputs: each layout must write every word itself
                f["Y"].upload(nan[:, :, :H]), f["gates"].upload(nan), f["cs"].upload(nan[:, :, :H]), bw["dZ"].upload(nan)
            _capi.check(dev.lib.mgr_lstm_scan_fwd_multi(dev.ctx, 2, farr, fws.ptr, fws.nbytes))
            _capi.check(dev.lib.mgr_lstm_scan_bwd_multi(dev.ctx, 2, barr, bws.ptr, bws.nbytes))
            got[contiguous] = [(f["Y"].download(), f["gates"].download(), f["cs"].download(), bw["dZ"].download()) for f, bw in zip(fj, bj)]
    finally:
        dev.call("mgr_tune", 3, 0)
        dev.call("mgr_tune", 1, 0)
    for reverse, ((Yh, Gh, Ch, dZh), (y_ref, cache, dx_ref, dU_ref)) in enumerate(zip(got[1], refs)):
        assert rel_err(Yh, y_ref) < 3e-5
        assert rel_err(Ch, cache["c"]) < 3e-5
        assert rel_err(Gh[..., 3], cache["o"]) < 3e-5
        dZ = bj[reverse]["dZ"]     # (holds the contiguous layout's result: it ran last)
        gW, gU, gb = dev.empty((F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
        ws2 = dev.bytes(dev.lib.mgr_lstm_param_grads_ws_bytes(B, T, F, H))
        dev.call("mgr_lstm_param_grads", keep[3 * reverse + 2], F, 0, fj[reverse]["Y"], H, dZ, gW, gU, gb, B, T, F, H, reverse, ws2, ws2.nbytes)
        gUk = dev.empty((H, 4 * H))
        dev.call("mgr_lstm_pack", gU, gUk, H, H, 1)
        assert rel_err(gUk.download(), dU_ref) < 1e-4
        gX = dev.empty((B, T, F))
        dev.call("mgr_lstm_input_grad", dZ, keep[3 * reverse], 0, gX, F, 0, B, T, F, H)
        assert rel_err(gX.download(), dx_ref) < 1e-4
        for a, o in zip(got[1][reverse], got[0][reverse]):
            assert np.array_equal(a, o)
    st = ctypes.c_uint(7)
    dev.call("mgr_scan_status", ctypes.byref(st))     # no persistent scan of this context ever gave up
    assert st.value == 0


@pytest.mark.parametrize("H,B,T", [(100, 20, 24), (300, 18, 16), (500, 33, 12)])
@pytest.mark.parametrize("scale", [1e-4, 1.0, 1.5])
def test_split_f16_scan_over_weight_scales(device, H, B, T, scale):
    """The split-f16 recurrence (operands as f16 (hi, lo) pairs of scaled f32 values) picks its weight scale from the
    weights it finds: tiny, ordinary and large recurrent weights give the f32 MFMA step's accuracy against the fp64 oracle, and
    both steps agree to rounding.  (Much larger weights make the recurrence chaotic: at 6 x the f32 step itself leaves the fp64
    trajectory at H = 100, at 3 x still.)"""
    dev = device
    rng = np.random.default_rng(H + int(scale * 7))
    F, f32 = 5, np.float32
    x, W, U, b, _ = _lstm_case(rng, B, T, F, H, 0.0)
    U = U * (0.1 if H >= 300 else 1.0) * scale
    y_ref, cache = kr.lstm_forward(x, W, U, b, None, False)
    Wp, Up, bp = dev.empty((F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
    dev.call("mgr_lstm_pack", dev.array(W.astype(f32)), Wp, F, H, 0)
    dev.call("mgr_lstm_pack", dev.array(U.astype(f32)), Up, H, H, 0)
    dev.call("mgr_lstm_pack", dev.array(b.astype(f32)), bp, 1, H, 0)
    Z = dev.empty((B, T, 4 * H))
    dev.call("mgr_lstm_input_proj", dev.array(x.astype(f32)), F, 0, Wp, bp, Z, B, T, F, H)
    ws = dev.bytes(dev.lib.mgr_lstm_scan_ws_bytes(B, T, H))
    got = {}
    dev.call("mgr_tune", 0, 3)   # clusters with an exchange at every H (the K-split step)
    dev.call("mgr_tune", 1, 1)
    try:
        for f32_mfma in (0, 1):
            dev.call("mgr_tune", 14, f32_mfma)
            Y, Cs = dev.zeros((B, T, H)), dev.zeros((B, T, H))
            dev.call("mgr_lstm_scan_fwd", Z, Up, Y, H, 0, 0, 0, Cs, B, T, H, 0, ws, ws.nbytes)
            got[f32_mfma] = (Y.download(), Cs.download())
        for f32_mfma in (0, 1):
            assert rel_err(got[f32_mfma][0], y_ref) < 3e-5
            assert rel_err(got[f32_mfma][1], cache["c"]) < 3e-5
        assert rel_err(got[0][0], got[1][0]) < 1e-5
    finally:
        dev.call("mgr_tune", 14, 0)
        dev.call("mgr_tune", 0, 0)
        dev.call("mgr_tune", 1, 0)


@pytest.mark.parametrize("H,B,T", [(100, 20, 12), (300, 18, 9)])
def test_split_f16_bptt_is_homogeneous_over_80_binary_orders_of_magnitude(device, H, B, T):
    """The multi-CU BPTT on the f16 pipe scales the gate gradients per wave and step by a power of two: scaling dY by
    2^k scales every dZ by exactly 2^k - bit for bit - for k from -40 to +40, i.e. no gradient magnitude is special."""
    dev = device
    rng = np.random.default_rng(H)
    F, f32 = 5, np.float32
    x, W, U, b, _ = _lstm_case(rng, B, T, F, H, 0.0)
    U = U * (0.1 if H >= 300 else 1.0)
    Wp, Up, bp = dev.empty((F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
    dev.call("mgr_lstm_pack", dev.array(W.astype(f32)), Wp, F, H, 0)
    dev.call("mgr_lstm_pack", dev.array(U.astype(f32)), Up, H, H, 0)
    dev.call("mgr_lstm_pack", dev.array(b.astype(f32)), bp, 1, H, 0)
    Z = dev.empty((B, T, 4 * H))
    dev.call("mgr_lstm_input_proj", dev.array(x.astype(f32)), F, 0, Wp, bp, Z, B, T, F, H)
    Y, G, Cs = dev.empty((B, T, H)), dev.empty((B, T, H, 4)), dev.empty((B, T, H))
    ws = dev.bytes(dev.lib.mgr_lstm_scan_ws_bytes(B, T, H))
    dev.call("mgr_lstm_scan_fwd", Z, Up, Y, H, 0, 0, G, Cs, B, T, H, 0, ws, ws.nbytes)
    dy = rng.standard_normal((B, T, H)).astype(f32)
    base = None
    for k in (0, -40, 40):
        dYd = dev.array((dy * f32(2.0 ** k)).astype(f32))
        dZ = dev.zeros((B, T, 4 * H))
        dev.call("mgr_lstm_scan_bwd", dYd, H, G, Cs, Up, dZ, B, T, H, 0, ws, ws.nbytes)
        out = dZ.download()
        assert np.all(np.isfinite(out)) and np.abs(out).max() > 0
        if base is None:
            base = out
        else:
            assert np.array_equal(out, base * f32(2.0 ** k)), k


@pytest.mark.parametrize("B,T,F,H,masked", [(3, 130, 64, 100, True), (2, 257, 1600, 100, True), (2, 100, 32, 25, False),
                                            (1, 128, 48, 300, True), (2, 90, 16, 20, True)])
def test_input_proj_pair_equals_two_calls(device, B, T, F, H, masked):
    """mgr_lstm_input_proj_pair (both directions of a Bidirectional layer as one GEMM over 8H columns where that saves
    column tiles: 4H = 400 -> 7 tiles instead of 8) writes exactly what two mgr_lstm_input_proj calls write, and that
    matches numpy fp64."""
    dev = device
    rng = np.random.default_rng(B * 1000 + T + F + H)
    f32 = np.float32
    N = 4 * H
    X = rng.standard_normal((B, T, F)).astype(f32)
    W = [(rng.standard_normal((F, N)) * 0.1).astype(f32) for _ in range(2)]
    bias = [rng.standard_normal(N).astype(f32) for _ in range(2)]
    M = [((rng.random((4, B, F)) > 0.5) * 2.0).astype(f32) if masked else None for _ in range(2)]
    dX = dev.array(X)
    dW, db = [dev.array(w) for w in W], [dev.array(b) for b in bias]
    dM = [dev.array(m) if masked else 0 for m in M]
    single = [dev.empty((B, T, N)) for _ in range(2)]
    for d in range(2):
        dev.call("mgr_lstm_input_proj", dX, F, dM[d], dW[d], db[d], single[d], B, T, F, H)
    both = [dev.empty((B, T, N)) for _ in range(2)]
    dev.call("mgr_lstm_input_proj_pair", dX, F, dM[0], dW[0], db[0], both[0], dM[1], dW[1], db[1], both[1], B, T, F, H)
    gate = np.arange(N) % 4
    for d in range(2):
        got = both[d].download()
        assert np.array_equal(got, single[d].download())
        ref = np.empty((B, T, N))
        for g in range(4):
            xg = X.astype(np.float64) * (M[d][g][:, None, :] if masked else 1.0)
            ref[:, :, gate == g] = xg @ W[d][:, gate == g].astype(np.float64) + bias[d][gate == g]
        assert np.abs(got - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("B,T,F,H,p", [(3, 130, 128, 100, 0.5), (2, 300, 1600, 100, 0.5), (2, 257, 1000, 500, 0.5),
                                       (2, 140, 600, 300, 0.6), (1, 64, 250, 64, 0.4), (2, 100, 131, 20, 0.9),
                                       (2, 50, 144, 33, 0.0), (2, 64, 160, 40, 1.0), (3, 200, 39, 500, 0.4), (2, 129, 20, 300, 0.6), (2, 40, 16, 8, 0.5)])
def test_input_proj_dropout_sparse_equals_dense(device, B, T, F, H, p):
    """mgr_lstm_input_proj_dropout (per-gate K loops over the kept features only) against mgr_lstm_input_proj and numpy fp64:
    the same sums with the zero terms left out.  Includes all-kept and all-dropped masks and unit counts that do not fill a tile."""
    dev = device
    rng = np.random.default_rng(B * 1000 + T + F + H)
    f32 = np.float32
    N = 4 * H
    X = rng.standard_normal((B, T, F)).astype(f32)
    W = (rng.standard_normal((F, N)) * 0.1).astype(f32)
    bias = rng.standard_normal(N).astype(f32)
    scale = 1.0 / (1.0 - p) if p < 1.0 else 1.0
    M = ((rng.random((4, B, F)) >= p) * scale).astype(f32)
    dX, dW, db, dM = dev.array(X), dev.array(W), dev.array(bias), dev.array(M)
    dense, sparse = dev.empty((B, T, N)), dev.empty((B, T, N))
    dev.call("mgr_lstm_input_proj", dX, F, dM, dW, db, dense, B, T, F, H)
    ws = dev.bytes(dev.lib.mgr_lstm_input_proj_dropout_ws_bytes(B, F, H))
    dev.call("mgr_lstm_input_proj_dropout", dX, F, dM, 0.5, dW, db, sparse, B, T, F, H, ws, ws.nbytes)
    gate = np.arange(N) % 4
    ref = np.empty((B, T, N))
    for g in range(4):
        ref[:, :, gate == g] = (X.astype(np.float64) * M[g][:, None, :]) @ W[:, gate == g].astype(np.float64) + bias[gate == g]
    tol = 2e-5 * max(1.0, np.abs(ref).max())
    assert np.abs(sparse.download() - ref).max() <= tol
    assert np.abs(sparse.download() - dense.download()).max() <= tol
    # the same kernel fed from the TRANSPOSED copy of X (rows of 128 time steps instead of gathered columns): mgr_transpose_bt
    # writes XT[b][f][t] padded to whole row tiles; the LDS images - hence every sum - are the same, bit for bit
    if 0.3 <= p and 16 <= F:
        ldt = (T + 127) // 128 * 128
        XT = dev.empty((B, F, ldt))
        XT.upload(np.full((B, F, ldt), np.nan, f32))     # the transpose must write the padding too
        dev.call("mgr_transpose_bt", dX, F, XT, ldt, B, T, F)
        xt = XT.download()
        assert np.array_equal(xt[:, :, :T], X.transpose(0, 2, 1)) and np.all(xt[:, :, T:] == 0)
        tr = dev.empty((B, T, N))
        dev.call("mgr_lstm_input_proj_dropout_t", XT, ldt, dM, 0.5, dW, db, tr, B, T, F, H, ws, ws.nbytes, 0.0)
        assert np.array_equal(tr.download(), sparse.download())      # (no bound on |X| stated: the f32 MFMA kernel)
        # with a bound on |X| the products run as split-f16 pairs on the f16 matrix pipe (k_gemm_nn_sparse16): the same tolerance
        # against fp64 as the f32 kernels; a looser bound only moves the scale
        # (tune key 10: 0 = per-gate K loops over the kept features, 2 = one dense K loop with the mask as a factor of the weight tiles)
        for kernel in (0, 2):
            dev.call("mgr_tune", 10, kernel)
            for bound in (float(np.abs(X).max()), 4.0 * float(np.abs(X).max())):
                tr.upload(np.full((B, T, N), np.nan, f32))
                dev.call("mgr_lstm_input_proj_dropout_t", XT, ldt, dM, p if p < 0.99 else 0.5, dW, db, tr, B, T, F, H, ws, ws.nbytes, bound)
                assert np.abs(tr.download() - ref).max() <= tol
        dev.call("mgr_tune", 10, 0)
        # no mask at all (inference): the dense kernel is the plain projection
        plain = dev.empty((B, T, N))
        dev.call("mgr_lstm_input_proj", dX, F, 0, dW, db, plain, B, T, F, H)
        tr.upload(np.full((B, T, N), np.nan, f32))
        dev.call("mgr_lstm_input_proj_dropout_t", XT, ldt, 0, 0.0, dW, db, tr, B, T, F, H, ws, ws.nbytes, float(np.abs(X).max()))
        ref0 = X.astype(np.float64) @ W.astype(np.float64) + bias
        assert np.abs(tr.download() - ref0).max() <= 2e-5 * max(1.0, np.abs(ref0).max())
        assert np.abs(tr.download() - plain.download()).max() <= 2e-5 * max(1.0, np.abs(ref0).max())
        # an input beyond the STATED bound (x_absmax > 0) is found on the device and the call falls back to the f32 MFMA kernel: the
        # result is the f32 kernel's, bit for bit - never Inf / NaN; a bound GUARANTEED by the producer (x_absmax < 0) is not checked:
        # there the violation overflows f16 and shows
        if p < 0.99:
            wrong = float(np.abs(X).max()) / 1024.0
            tr.upload(np.zeros((B, T, N), f32))
            dev.call("mgr_lstm_input_proj_dropout_t", XT, ldt, dM, p, dW, db, tr, B, T, F, H, ws, ws.nbytes, wrong)
            assert np.array_equal(tr.download(), sparse.download())
            dev.call("mgr_lstm_input_proj_dropout_t", XT, ldt, 0, 0.0, dW, db, tr, B, T, F, H, ws, ws.nbytes, wrong)      # no mask
            assert np.abs(tr.download() - ref0).max() <= 2e-5 * max(1.0, np.abs(ref0).max())
            dev.call("mgr_lstm_input_proj_dropout_t", XT, ldt, dM, p, dW, db, tr, B, T, F, H, ws, ws.nbytes, -wrong)
            assert not np.all(np.isfinite(tr.download()))
            # ... and a guaranteed bound that holds gives the checked call's result bit for bit (the same kernel, no gate)
            okb = float(np.abs(X).max())
            dev.call("mgr_lstm_input_proj_dropout_t", XT, ldt, dM, p, dW, db, tr, B, T, F, H, ws, ws.nbytes, okb)
            a = tr.download()
            dev.call("mgr_lstm_input_proj_dropout_t", XT, ldt, dM, p, dW, db, tr, B, T, F, H, ws, ws.nbytes, -okb)
            assert np.array_equal(tr.download(), a)
        # no mask and no bound (or tune key 15 = 1 - the f32 A/B switch - in an inference pass): the f32 kernel over all features
        tr.upload(np.full((B, T, N), np.nan, f32))
        dev.call("mgr_lstm_input_proj_dropout_t", XT, ldt, 0, 0.0, dW, db, tr, B, T, F, H, ws, ws.nbytes, 0.0)
        assert np.abs(tr.download() - ref0).max() <= 2e-5 * max(1.0, np.abs(ref0).max())
    assert dev.lib.mgr_lstm_input_proj_dropout_wants_transposed(dev.ctx, 0.5, 1000) == 1
    assert dev.lib.mgr_lstm_input_proj_dropout_wants_transposed(dev.ctx, 0.5, 39) == 0
    assert dev.lib.mgr_lstm_input_proj_dropout_wants_transposed(dev.ctx, 0.1, 1000) == 0


@pytest.mark.parametrize("B,T,F,H,p,reverse", [(3, 130, 128, 100, 0.5, 0), (2, 300, 1600, 100, 0.5, 1), (2, 77, 1000, 130, 0.5, 0),
                                               (2, 140, 600, 300, 0.6, 1), (2, 100, 131, 20, 0.9, 0), (2, 50, 144, 33, 0.0, 1),
                                               (2, 64, 160, 40, 1.0, 0)])
def test_param_grads_dropout_sparse_equals_dense(device, B, T, F, H, p, reverse):
    """mgr_lstm_param_grads_dropout (dW rows of the kept features only, per (gate, sample), gathered in sample order) against
    mgr_lstm_param_grads and numpy fp64; dU and db are the shared path."""
    dev = device
    rng = np.random.default_rng(B * 977 + T + F + H)
    f32 = np.float32
    N = 4 * H
    X = rng.standard_normal((B, T, F)).astype(f32)
    Hs = rng.standard_normal((B, T, H)).astype(f32)
    dZ = (rng.standard_normal((B, T, N)) * 0.3).astype(f32)
    scale = 1.0 / (1.0 - p) if p < 1.0 else 1.0
    M = ((rng.random((4, B, F)) >= p) * scale).astype(f32)
    dX, dH, ddZ, dM = dev.array(X), dev.array(Hs), dev.array(dZ), dev.array(M)
    outs = []
    for sparse in (False, True):
        gW, gU, gb = dev.empty((F, N)), dev.empty((H, N)), dev.empty((N,))
        if sparse:
            ws = dev.bytes(dev.lib.mgr_lstm_param_grads_dropout_ws_bytes(B, T, F, H))
            dev.call("mgr_lstm_param_grads_dropout", dX, F, dM, 0.5, dH, H, ddZ, gW, gU, gb, B, T, F, H, reverse, ws, ws.nbytes)
        else:
            ws = dev.bytes(dev.lib.mgr_lstm_param_grads_ws_bytes(B, T, F, H))
            dev.call("mgr_lstm_param_grads", dX, F, dM, dH, H, ddZ, gW, gU, gb, B, T, F, H, reverse, ws, ws.nbytes)
        outs.append((gW.download(), gU.download(), gb.download()))
    gate = np.arange(N) % 4
    ref = np.empty((F, N))
    for g in range(4):
        ref[:, gate == g] = np.einsum("btf,btn->fn", X.astype(np.float64) * M[g][:, None, :], dZ[:, :, gate == g].astype(np.float64))
    tol = 3e-5 * max(1.0, np.abs(ref).max())
    assert np.abs(outs[1][0] - ref).max() <= tol
    assert np.abs(outs[1][0] - outs[0][0]).max() <= tol
    assert np.array_equal(outs[1][1], outs[0][1]) and np.array_equal(outs[1][2], outs[0][2])
    # both operands from transposed copies (time is the K dimension of dW): bit-identical to the gathered form
    if dev.lib.mgr_lstm_param_grads_dropout_wants_transposed(dev.ctx, 0.5, F):
        for ldt in ((T + 15) // 16 * 16, (T + 127) // 128 * 128):
            XT = dev.zeros((B, F, ldt))
            dev.call("mgr_transpose_bt", dX, F, XT, ldt, B, T, F)
            ws = dev.bytes(dev.lib.mgr_lstm_param_grads_dropout_t_ws_bytes(B, T, F, H, ldt))
            dev.call("mgr_memset", ws, 0xFF, ws.nbytes)        # the workspace arrives dirty (all-ones words are NaNs)
            gW, gU, gb = dev.empty((F, N)), dev.empty((H, N)), dev.empty((N,))
            dev.call("mgr_lstm_param_grads_dropout_t", XT, ldt, dM, 0.5, dH, H, ddZ, gW, gU, gb, B, T, F, H, reverse, ws, ws.nbytes, 0.0)
            assert np.array_equal(gW.download(), outs[1][0])
            assert np.array_equal(gU.download(), outs[1][1]) and np.array_equal(gb.download(), outs[1][2])
            # with a bound on |X|: split-f16 operands on the f16 matrix pipe (rows padded to 32 steps), dZ scaled per (sample, gate
            # column) - here with dZ rows spread over 24 orders of magnitude; the same tolerance against fp64 as the f32 kernels
            if ldt % 32 == 0:
                spread = (10.0 ** rng.uniform(-12, 12, size=(B, 1, N))).astype(f32)
                dZw = dZ * spread
                refw = np.empty((F, N))
                for g in range(4):
                    refw[:, gate == g] = np.einsum("btf,btn->fn", X.astype(np.float64) * M[g][:, None, :], dZw[:, :, gate == g].astype(np.float64))
                for zz, rr in ((dZ, ref), (dZw, refw)):
                    dzz = dev.array(zz)
                    dev.call("mgr_memset", ws, 0xFF, ws.nbytes)
                    gW.upload(np.full((F, N), np.nan, f32))
                    dev.call("mgr_lstm_param_grads_dropout_t", XT, ldt, dM, 0.5, dH, H, dzz, gW, gU, gb, B, T, F, H, reverse, ws, ws.nbytes,
                             float(np.abs(X).max()))
                    got = gW.download()
                    colscale = np.maximum(np.abs(rr).max(axis=0, keepdims=True), 1e-30)   # per column: the spread is per column
                    assert np.all(np.isfinite(got)) and (np.abs(got - rr) / colscale).max() <= 3e-5
                # a stated bound the data violate: found on the device, the f32 MFMA kernel's result bit for bit
                dev.call("mgr_memset", ws, 0xFF, ws.nbytes)
                gW.upload(np.full((F, N), np.nan, f32))
                dev.call("mgr_lstm_param_grads_dropout_t", XT, ldt, dM, 0.5, dH, H, ddZ, gW, gU, gb, B, T, F, H, reverse, ws, ws.nbytes,
                         float(np.abs(X).max()) / 1024.0)
                assert np.array_equal(gW.download(), outs[1][0])


@pytest.mark.parametrize("H,B,T,path", [(300, 20, 75, 0), (500, 33, 70, 0), (100, 16, 64, 0), (128, 5, 33, 0), (300, 20, 75, 1),
                                        (60, 7, 40, 0), (300, 18, 50, 7)])
def test_scan_writes_the_transposed_output_itself(device, H, B, T, path):
    """mgr_scan_job.YT: the scans leave YT[b][col0 + u][t] = Y[b, t, u] (+ residual) with zeros behind T up to the row
    length ldt, two directions into column ranges of ONE wider copy - from inside the K-split multi-CU kernel (LDS-staged rows) or,
    for every other kernel family (path 1: fallback kernels; 7: LDS-image cluster step; small H), through the transpose
    the call appends.  Y itself is unchanged by the option."""
    from mgr_amd import _capi
    dev = device
    rng = np.random.default_rng(H + B + T)
    ldt = (T + 127) // 128 * 128
    W = 2 * H
    Y = dev.zeros((B, T, W))
    R = dev.array(rng.standard_normal((B, T, W)).astype(np.float32))
    YT = dev.array(np.full((B, W, ldt), 7.0, np.float32))        # dirty: what is not written must be recognisable
    jobs, keep = [], []
    for d in range(2):
        Z = dev.array((rng.standard_normal((B, T, 4 * H)) * 0.5).astype(np.float32))
        U = dev.array((rng.standard_normal((H, 4 * H)) * 0.1 / np.sqrt(H)).astype(np.float32))
        Up = dev.empty((H, 4 * H))
        dev.call("mgr_lstm_pack", U, Up, H, H, 0)
        keep += [Z, U, Up]
        jobs.append(dict(Z=Z, Up=Up, Y=Y.view(d * H, (1,)), ldy=W, R=R.view(d * H, (1,)), ldr=W, gates=0, cs=0, B=B, T=T, H=H,
                         reverse=d, YT=YT.ptr + d * H * ldt * 4, ytb=W * ldt, ldt=ldt))
    if path == 7:
        dev.call("mgr_tune", 7, 1)
    else:
        dev.call("mgr_tune", 0, path)
    try:
        arr = _capi.make_scan_jobs(jobs)
        ws = dev.bytes(dev.lib.mgr_lstm_scan_multi_ws_bytes(len(jobs), arr))
        _capi.check(dev.lib.mgr_lstm_scan_fwd_multi(dev.ctx, len(jobs), arr, ws.ptr, ws.nbytes))
        y, yt = Y.download(), YT.download()
        # the same scans without the option give the same Y
        Y2 = dev.zeros((B, T, W))
        for d, j in enumerate(jobs):
            j.update(Y=Y2.view(d * H, (1,)), YT=0, ytb=0, ldt=0)
        arr2 = _capi.make_scan_jobs(jobs)
        _capi.check(dev.lib.mgr_lstm_scan_fwd_multi(dev.ctx, len(jobs), arr2, ws.ptr, ws.nbytes))
        assert np.array_equal(Y2.download(), y)
    finally:
        dev.call("mgr_tune", 0, 0)
        dev.call("mgr_tune", 7, 0)
    assert np.array_equal(yt[:, :, :T], y.transpose(0, 2, 1))
    assert not yt[:, :, T:].any()          # zeros behind T up to the row length, whatever the buffer held (mgr.h)


@pytest.mark.parametrize("B,T,D,Cn,Lmax,p", [(64, 1900, 200, 22, 35, 0.5), (8, 200, 256, 22, 35, 0.5), (3, 37, 200, 22, 10, 0.0),
                                             (2, 50, 600, 22, 12, 0.5)])
def test_head_fwd_bwd_matches_the_oracle(device, B, T, D, Cn, Lmax, p):
    """mgr_head_fwd_bwd (Dropout -> Dense -> softmax -> CTC loss + gradient -> Dense backward behind ONE entry point - a host-side
    sequence of four launches, not a fused kernel; reference multimodal_fusion/multimodal.py:171-179, losses.py:4-15) against the
    fp64 oracle: P 1e-5, losses 1e-4 (north_star's bound), dLogits and dA / dWd / dbd 5e-4 of the tensor's maximum (the existing
    bound of the CTC gradient).  (64, 1900, 200, 22) is the bench shape, (8, 200, 256, 22) BASELINE configs[0]'s;
    D = 600 takes the vector-ALU kernels (the matrix-core forms hold Wd in registers / LDS up to D = 256)."""
    dev = device
    rng = np.random.default_rng(B * 7 + D)
    A = rng.standard_normal((B, T, D)).astype(np.float32)
    Wd = (rng.standard_normal((D, Cn)) * (2.0 / np.sqrt(D))).astype(np.float32)
    bd = (rng.standard_normal(Cn) * 0.1).astype(np.float32)
    dm = ((rng.random((B, T, D)) >= p) / (1 - p)).astype(np.float32) if p > 0 else None
    skip, eps, blank = 2, 1e-8, Cn - 1
    labels = -np.ones((B, Lmax))
    ll = np.zeros(B, np.int64)
    for b in range(B):
        L = int(rng.integers(1, min(Lmax, (T - skip) // 2) + 1))
        labels[b, :L] = rng.integers(0, Cn - 1, size=L)
        ll[b] = L
    il = np.full(B, T - skip)
    dA_, dW_, db_ = dev.array(A), dev.array(Wd), dev.array(bd)
    dmask = dev.array(dm) if dm is not None else 0
    dlab = dev.array(np.where(labels >= 0, labels, -1).astype(np.int32))
    dil, dll = dev.array(il.astype(np.int32)), dev.array(ll.astype(np.int32))

    def outs():
        return dict(P=dev.empty((B, T, Cn)), loss=dev.empty((B,)), mean=dev.empty((4,)), dL=dev.empty((B, T, Cn)),
                    gW=dev.empty((D, Cn)), gb=dev.empty((Cn,)), gA=dev.empty((B, T, D)))

    f = outs()
    ws = dev.bytes(dev.lib.mgr_head_ws_bytes(B, T, D, Cn, Lmax))
    dev.call("mgr_head_fwd_bwd", dA_, D, dmask, 0.0, C.c_uint64(0), dW_, db_, dlab, dil, dll, B, T, D, Cn, Lmax, skip, blank, eps,
             1.0 / B, f["P"], f["loss"], f["mean"], f["dL"], f["gW"], f["gb"], f["gA"], D, ws, ws.nbytes)
    got = {k: v.download() for k, v in f.items()}
    # the oracle: dense + softmax, CTC on its own (fp64) softmax output, dense backward of its own gradient
    A64, dm64 = A.astype(np.float64), None if dm is None else dm.astype(np.float64)
    Pref, cache = kr.dense_softmax_forward(A64, dm64, Wd.astype(np.float64), bd.astype(np.float64))
    ref_loss, ref_dz = kr.ctc_loss_grad(Pref, labels, il, ll, skip=skip, eps=eps)
    dAref, dWref, dbref = kr.dense_backward(ref_dz / B, cache)
    assert rel_err(got["P"], Pref) < 1e-5
    assert np.allclose(got["loss"], ref_loss, rtol=1e-4), np.abs(got["loss"] / ref_loss - 1).max()
    assert abs(got["mean"][0] / ref_loss.mean() - 1) < 1e-4
    assert rel_err(got["dL"], ref_dz / B) < 5e-4
    for name, a, b in (("dA", got["gA"], dAref), ("dWd", got["gW"], dWref), ("dbd", got["gb"], dbref)):
        assert rel_err(a, b) < 5e-4, (name, rel_err(a, b))     # (the bound of the CTC gradient they are products of)


def test_head_fwd_bwd_at_two_pairs_per_lane_equals_its_parts(device):
    """mgr_head_fwd_bwd at Lmax = 70 (the CTC recursions hold two (blank, label) pairs per lane; one sample has all 70 labels, its
    states cross the lane boundaries): the bounds of test_head_fwd_bwd_matches_the_oracle against the fp64 oracle, and the header's
    promise - bit for bit the results of mgr_dense_softmax_fwd followed by mgr_ctc_loss_grad with the same arguments."""
    dev = device
    B, T, D, Cn, Lmax = 3, 150, 64, 22, 70
    rng = np.random.default_rng(B * 7 + D + Lmax)
    A = rng.standard_normal((B, T, D)).astype(np.float32)
    Wd = (rng.standard_normal((D, Cn)) * (2.0 / np.sqrt(D))).astype(np.float32)
    bd = (rng.standard_normal(Cn) * 0.1).astype(np.float32)
    skip, eps, blank = 2, 1e-8, Cn - 1
    ll = np.array([70, 33, 5])
    labels = -np.ones((B, Lmax), np.int64)
    for b in range(B):
        labels[b, :ll[b]] = rng.integers(0, Cn - 1, size=ll[b])
    il = np.array([T - skip, T - skip - 1, 40])
    dA_, dW_, db_ = dev.array(A), dev.array(Wd), dev.array(bd)
    dlab, dil, dll = dev.array(labels.astype(np.int32)), dev.array(il.astype(np.int32)), dev.array(ll.astype(np.int32))
    f = dict(P=dev.empty((B, T, Cn)), loss=dev.empty((B,)), mean=dev.empty((4,)), dL=dev.empty((B, T, Cn)),
             gW=dev.empty((D, Cn)), gb=dev.empty((Cn,)), gA=dev.empty((B, T, D)))
    ws = dev.bytes(dev.lib.mgr_head_ws_bytes(B, T, D, Cn, Lmax))
    dev.call("mgr_head_fwd_bwd", dA_, D, 0, 0.0, C.c_uint64(0), dW_, db_, dlab, dil, dll, B, T, D, Cn, Lmax, skip, blank, eps,
             1.0 / B, f["P"], f["loss"], f["mean"], f["dL"], f["gW"], f["gb"], f["gA"], D, ws, ws.nbytes)
    got = {k: v.download() for k, v in f.items()}
    Pref, cache = kr.dense_softmax_forward(A.astype(np.float64), None, Wd.astype(np.float64), bd.astype(np.float64))
    ref_loss, ref_dz = kr.ctc_loss_grad(Pref, labels, il, ll, skip=skip, eps=eps)
    dAref, dWref, dbref = kr.dense_backward(ref_dz / B, cache)
    assert np.isfinite(ref_loss).all()
    assert rel_err(got["P"], Pref) < 1e-5
    assert np.allclose(got["loss"], ref_loss, rtol=1e-4), np.abs(got["loss"] / ref_loss - 1).max()
    assert abs(got["mean"][0] / ref_loss.mean() - 1) < 1e-4
    assert rel_err(got["dL"], ref_dz / B) < 5e-4
    for name, a, b in (("dA", got["gA"], dAref), ("dWd", got["gW"], dWref), ("dbd", got["gb"], dbref)):
        assert rel_err(a, b) < 5e-4, (name, rel_err(a, b))
    # the parts, on their own buffers
    P2, loss2, dL2 = dev.empty((B, T, Cn)), dev.empty((B,)), dev.empty((B, T, Cn))
    ws2 = dev.bytes(dev.lib.mgr_ctc_ws_bytes(B, T, Cn, Lmax))
    dev.call("mgr_dense_softmax_fwd", dA_, D, 0, 0.0, C.c_uint64(0), dW_, db_, P2, B, T, D, Cn)
    dev.call("mgr_ctc_loss_grad", P2, dlab, dil, dll, B, T, Cn, Lmax, skip, blank, eps, 1.0 / B, loss2, dL2, ws2, ws2.nbytes)
    for name, a, b in (("P", got["P"], P2.download()), ("loss", got["loss"], loss2.download()), ("dLogits", got["dL"], dL2.download())):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    for a in (dA_, dW_, db_, dlab, dil, dll, ws, P2, loss2, dL2, ws2) + tuple(f.values()):
        a.free()
