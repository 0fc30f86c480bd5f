"""-m gpu: a scan job may omit its row-major output (mgr_scan_job.Y == NULL with a YT, include/mgr.h), and the engine omits it
for the deepest encoder scans of a pass in which every reader of the encoder output takes the transposed copy FEAT^T
(Engine._feat_rows_unread, Schedule.feat_rows_when_unread).

  * library: the transposed copy of a call without Y equals, bit for bit and including the zeroed tail, the copy of the same call
    with Y - K-split kernels (plain, fused, f32 MFMA step: no row scratch in the workspace the call asks for) and a kernel family
    that transposes behind the scan (rows in scratch); a workspace without room for that scratch is refused before anything runs
  * engine: pipelined training steps with and without the rows give the same losses and weights; without them the FEAT buffers
    keep the pattern they were filled with; a schedule whose fusion GEMMs read row-major FEAT keeps writing it; a validation pass
    between pipelined steps changes nothing
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
B_LIB, LDT = 17, 128      # two 16-sample groups, the second with one sample


def _status(dev):
    st = (C.c_uint * 4)()
    dev.call("mgr_scan_status_ex", st)
    return int(st[0])


def _layer(dev, H, T, seed):
    """Both directions of a random layer of width H: per direction (Z, packed U), and a residual input [B, T, 2H]."""
    rng = np.random.default_rng(seed)
    dirs = []
    for _ in range(2):
        Z = dev.array((rng.standard_normal((B_LIB, T, 4 * H)) * 0.5).astype(f32))
        U = dev.array((rng.standard_normal((H, 4 * H)) * 0.1 / np.sqrt(H)).astype(f32))
        Up = dev.empty((H, 4 * H))
        dev.call("mgr_lstm_pack", U, Up, H, H, 0)
        dirs.append((Z, Up, U))
    R = dev.array(rng.uniform(-1, 1, (B_LIB, T, 2 * H)).astype(f32))
    return dirs, R


def _scan(dev, dirs, R, H, T, with_y, split, form, ws_bytes=None):
    """One multi-scan call over both directions into a dirty YT; returns (return code, YT, Y or None, exact workspace bytes, the
    bytes the same jobs need WITH rows)."""
    from mgr_amd import _capi
    W = 2 * H
    Y = dev.zeros((B_LIB, T, W)) if with_y else None
    YT = dev.array(np.full((B_LIB, W, LDT), 7.0, f32))

    def jobs_(rows):
        return [dict(Z=dirs[d][0], Up=dirs[d][1], Y=rows.view(d * H, (1,)) if rows is not None else 0, ldy=W if rows is not None else 0,
                     R=R.view(d * H, (1,)) if R is not None else 0, ldr=W if R is not None else 0, B=B_LIB, T=T, H=H, reverse=d,
                     YT=YT.ptr + d * H * LDT * 4, ytb=W * LDT, ldt=LDT, yt_split=int(split)) for d in range(2)]

    arr = _capi.make_scan_jobs(jobs_(Y))
    opts = _capi.make_launch_opts(form, 0)
    exact = dev.lib.mgr_lstm_scan_fwd_multi_ws_bytes(dev.ctx, 2, arr, C.byref(opts))
    upper = dev.lib.mgr_lstm_scan_multi_ws_bytes(2, arr)
    probe = dev.empty((B_LIB, T, W))
    with_rows = dev.lib.mgr_lstm_scan_multi_ws_bytes(2, _capi.make_scan_jobs(jobs_(probe)))
    probe.free()
    assert 0 < with_rows <= exact <= upper
    ws = dev.bytes(exact if ws_bytes is None else ws_bytes(exact, with_rows))
    dev.call("mgr_tune", 1, 1)      # the call checks its launch's give-up word synchronously
    try:
        rc = dev.lib.mgr_lstm_scan_fwd_multi_ex(dev.ctx, 2, arr, ws.ptr, ws.nbytes, C.byref(opts))
    finally:
        dev.call("mgr_tune", 1, 0)
    dev.sync()
    out = (rc, YT.download(), None if Y is None else Y.download(), exact, with_rows)
    for a in (Y, YT, ws):
        if a is not None:
            a.free()
    return out


def _tail_is_zero(yt, T, split):
    if split:
        return not yt.view(np.float16).reshape(yt.shape[0], yt.shape[1], 2, LDT)[..., T:].any()
    return not yt[:, :, T:].any()


@pytest.mark.parametrize("form", ["plain", "fused_any", "f32_mfma"])
@pytest.mark.parametrize("H", [100, 300, 500])
def test_transposed_copy_without_rows_is_bit_identical(device, H, form):
    """K-split kernels: cluster_run_k16 as k_scan_cluster_k16[_s] (plain) and as the two halves of k_scan_cluster_k16fs
    (MGR_SCAN_FORM_FUSED_ANY; H = 100 and H = 300 have an odd unit-group count: a fused member without valid cells), cluster_run_ks
    (tune 14 = 1).  T = 7 / 8 / 9 / 17: shorter than, equal to and one over the 8-step staging chunk, a partial last chunk."""
    from mgr_amd import _capi
    dev = device
    dev.call("mgr_scan_status_clear")
    opt_form = _capi.SCAN_FORM_FUSED_ANY if form == "fused_any" else _capi.SCAN_FORM_PLAIN
    dev.call("mgr_tune", 14, 1 if form == "f32_mfma" else 0)
    try:
        for T in (7, 8, 9, 17):
            dirs, R = _layer(dev, H, T, 1000 * H + T)
            for res in (R, None):
                for split in (0, 1):
                    rc0, yt0, y0, _, _ = _scan(dev, dirs, res, H, T, True, split, opt_form)
                    assert rc0 == 0 and _status(dev) == 0
                    rc1, yt1, _, exact, with_rows = _scan(dev, dirs, res, H, T, False, split, opt_form)
                    assert rc1 == 0 and _status(dev) == 0
                    # (the K-split kernel wrote YT itself: the call asked for no row scratch)
                    assert exact == with_rows, (H, form, T)
                    assert np.isfinite(y0).all() and np.abs(y0).max() > 0.05
                    assert np.array_equal(yt0.view(np.uint32), yt1.view(np.uint32)), (H, form, T, res is not None, split)
                    assert _tail_is_zero(yt1, T, split)
                    if not split:
                        assert np.array_equal(yt1[:, :, :T], y0.transpose(0, 2, 1))
            for Z, Up, U in dirs:
                Z.free(), Up.free(), U.free()
            R.free()
    finally:
        dev.call("mgr_tune", 14, 0)


@pytest.mark.parametrize("H,lds_image", [(64, 0), (100, 1)])
def test_kernels_that_transpose_behind_the_scan_take_rows_from_scratch(device, H, lds_image):
    """H = 64 has no K-split instantiation; H = 100 with tune 7 = 1 takes the LDS-image step: the transposed copy comes from a
    transpose behind the scan, which reads rows - scratch from the workspace when the job gave no Y.  Same YT; the call asks for
    exactly the scratch on top; a workspace without it is refused before anything is enqueued (YT keeps its fill)."""
    from mgr_amd import _capi
    dev = device
    dev.call("mgr_scan_status_clear")
    T = 9
    dirs, R = _layer(dev, H, T, 77 + H)
    rows_bytes = 2 * ((B_LIB * T * H * 4 + 255) // 256 * 256)
    dev.call("mgr_tune", 7, lds_image)
    try:
        for split in (0, 1):
            rc0, yt0, y0, _, _ = _scan(dev, dirs, R, H, T, True, split, _capi.SCAN_FORM_AUTO)
            rc1, yt1, _, exact, with_rows = _scan(dev, dirs, R, H, T, False, split, _capi.SCAN_FORM_AUTO)
            assert rc0 == 0 and rc1 == 0 and _status(dev) == 0
            assert exact == with_rows + rows_bytes
            assert np.array_equal(yt0.view(np.uint32), yt1.view(np.uint32)) and _tail_is_zero(yt1, T, split)
        rc, yt, _, _, _ = _scan(dev, dirs, R, H, T, False, 0, _capi.SCAN_FORM_AUTO, ws_bytes=lambda exact, with_rows: with_rows)
        assert rc != 0 and b"workspace" in dev.lib.mgr_last_error()
        assert (yt == 7.0).all() and _status(dev) == 0
    finally:
        dev.call("mgr_tune", 7, 0)


# ---------------------------------------------------------------------------------------------------------------- engine
B, T, LMAX, STEPS = 17, 40, 8, 3


def _train(device, sched, predict_between=False):
    """STEPS pipelined device-RNG training steps (announced two calls ahead, as bench.py does) of a small fusion network with frozen
    two-layer residual encoders (H = 64: depth-2 fin = 128, FEAT width 256 - the pre-split path) and a fusion layer of H = 100, the
    FEAT buffers filled with NaN first.  Returns (losses, weights after each step, FEAT buffers at the end, validation outputs)."""
    from mgr_amd.configs import fusion_spec
    from mgr_amd.engine import Engine, Schedule
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    spec = fusion_spec(h_audio=64, h_skeletal=64, h_fusion=100)
    eng = Engine(spec, B, T, LMAX, device=device, seed=7, schedule=Schedule(**sched))
    eng.set_weights(synthetic_weights(spec, 3))
    xs, labels, il, ll = synthetic_arrays(spec, B, T, LMAX, 11)
    eng._upload_inputs(xs, None, True)
    eng._upload_labels(labels, il, ll)
    W = spec.concat_width
    for fb in eng._feat_ring:
        fb.upload(np.full((B, T, W), np.nan, f32))
    assert len(eng._feat_ring) == 2
    trainable = [n for n, _, tr, _ in spec.weight_table() if tr]
    losses, weights, seen = [], [], []
    for i in range(STEPS):
        eng.enqueue_train_step(None, None, None, None, rand=None, apply_update=True, upload=False,
                               prefetch_next=i < STEPS - 1, prefetch_after_next=i < STEPS - 2)
        losses.append(eng.read_loss())
        w = eng.get_weights()
        weights.append({k: w[k].copy() for k in trainable})
        if predict_between and i < STEPS - 1:
            seen.append([p.copy() for p in eng.predict_stream([xs], output="posteriors")])
    device.sync()
    assert eng.scan_health()[0] == 0
    feats = [fb.download() for fb in eng._feat_ring]
    eng.close()
    return losses, weights, feats, seen


def _same(a, b):
    la, wa = a[0], a[1]
    lb, wb = b[0], b[1]
    assert la == lb
    for x, y in zip(wa, wb):
        assert x.keys() == y.keys() and len(x) > 0
        for k in x:
            assert np.array_equal(x[k], y[k]), k


@pytest.fixture(scope="module")
def with_rows(device):
    return _train(device, dict(feat_rows_when_unread=True))


def test_pipelined_steps_without_feat_rows_are_bit_identical_and_leave_feat_alone(device, with_rows):
    got = _train(device, {})
    assert all(np.isfinite(got[0]))
    _same(got, with_rows)
    # the store is gone and nobody read what it used to write: the NaN fill is still there - and it is gone where the rows are kept
    assert all(np.isnan(f).all() for f in got[2])
    assert not any(np.isnan(f).any() for f in with_rows[2])


def test_a_schedule_whose_fusion_gemms_read_rows_keeps_writing_them(device):
    """Schedule(split_rows=False, transposed_inputs=False): no FEAT^T at all, the fusion projection and dW read row-major FEAT - the
    predicate is false and the pass is what it was: the same bits as with feat_rows_when_unread=True, both with FEAT written."""
    base = dict(split_rows=False, transposed_inputs=False)
    got = _train(device, base)
    ref = _train(device, dict(base, feat_rows_when_unread=True))
    _same(got, ref)
    assert all(np.isfinite(got[0]))
    assert not any(np.isnan(f).any() for f in got[2]) and not any(np.isnan(f).any() for f in ref[2])


def test_a_validation_pass_between_pipelined_steps_changes_nothing(device, with_rows):
    """predict_stream between announced steps discards the prefetched encoder pass (its own passes leave the rows out as well:
    the inference projection reads FEAT^T); the training losses and weights stay those of the undisturbed run, and the validation
    outputs those of the engine that writes the rows."""
    got = _train(device, {}, predict_between=True)
    _same(got, with_rows)
    ref = _train(device, dict(feat_rows_when_unread=True), predict_between=True)
    assert len(got[3]) == STEPS - 1
    for a, b in zip(got[3], ref[3]):
        assert len(a) == 1 and np.isfinite(a[0]).all() and np.array_equal(a[0], b[0])
