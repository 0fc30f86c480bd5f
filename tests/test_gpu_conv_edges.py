"""-m gpu: the CNN front-end kernels (csrc/conv.hip) through the C ABI against torch fp64 at every dispatch branch and shape edge.
The cases are built in tests/conv_cases.py (their premises are checked without a GPU in tests/test_cpu_conv_cases.py) and run
through tests/conv_harness.py: guarded, poisoned outputs and a NaN-filled weight-gradient workspace.  Then every refusal of the three
entry points, and one whole train step through the engine on a colour, non-square front-end that is none of the reference's.

What these cases found: k_conv_pool_bwd_w_mfma formed the bias gradient with one thread per channel of a 256-thread block, so for
Cout = 272 the partial sums of channels 256 .. 271 were never written and db[256:] came back NaN from the 0xFF-filled workspace
(mfma4-cout272; fixed by a loop over the channels).  A frame of exactly 64 KiB launches (lds-limit); its data gradient would stage
62 x 62 x 4 pooled gradients and codes, 76 880 bytes, and is refused like any other over 64 KiB - that case checks the refusal
where the others check dX."""
import numpy as np
import pytest

from mgr_amd import _capi
from tests import conv_cases as cc
from tests.conv_harness import Guarded, fill_workspace, run_layer
from tests.helpers import rel_err
from tests.rgb_ref import conv_layer_routed

pytestmark = pytest.mark.gpu

POOLED_REFUSAL = "does not fit the LDS stage"


def _last_error(device):
    return device.lib.mgr_last_error().decode(errors="replace")


def _check_case(device, name, off=0):
    c = cc.case(name)
    d = cc.dims(c.Hin, c.Win, c.Cin, c.ks, c.Cout)
    fits = d.pooled_bytes <= cc.MAX_LDS           # (the data gradient stages the pooled gradient: lds-limit's does not fit)
    Y, dX, gW, gb, code, rep = run_layer(device, c.x, c.W, c.b, c.dY, c.ks, off=off, data_gradient=fits)
    rY, pre = cc.reference(name)
    print("%s: Y %.2e" % (name, rel_err(Y, rY)))
    assert rel_err(Y, rY) < 1e-5
    # routing: the f32 forward's window choice is the fp64 one wherever the two largest values are apart by more than f32 rounding
    code = code.reshape(Y.shape)
    rcode, clear, dead = cc.routing_premise(pre)
    assert set(np.unique(code)) <= {0, 1, 2, 3, 255}
    assert np.array_equal(code[clear], rcode[clear])
    assert (code[dead] == 255).all()
    assert (clear | dead).mean() > 0.99 or c.constant
    assert np.array_equal(code == 255, Y == 0)                  # a window routes nothing exactly when its output is a ReLU zero
    # gradients through that routing
    pre2, rdX, rW, rb = conv_layer_routed(c.x, c.W, c.b, c.dY, code)
    assert np.array_equal(pre2, pre)
    print("%s: dX %s dW %.2e db %.2e" % (name, "%.2e" % rel_err(dX, rdX) if fits else "refused", rel_err(gW, rW), rel_err(gb, rb)))
    if fits:
        assert rel_err(dX, rdX) < 1e-5
    assert rel_err(gW, rW) < 1e-5, rel_err(gW, rW)
    assert rel_err(gb, rb) < 1e-5, rel_err(gb, rb)
    assert np.array_equal(gW.view(np.uint32), rep.view(np.uint32))   # deterministic: a second launch gives the same bits
    if c.constant:
        assert set(np.unique(code)) <= {0, 255}        # ties go to the first position; ReLU-zero windows route nothing
        assert (code == 0).any() and (code == 255).any()
    return c, d


@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_conv_case_matches_fp64(device, name):
    c, d = _check_case(device, name)
    if d.pooled_bytes > cc.MAX_LDS:
        # its forward and weight gradient ran at the LDS limit; the data gradient of such a frame is refused, and says why
        x = Guarded(device, c.x.size, salt=20)
        g = Guarded(device, c.dY.size, salt=21, fill=c.dY)
        code = Guarded(device, c.dY.size, item=1, salt=22, fill=np.zeros(c.dY.size, np.uint8))
        W = device.array(c.W.reshape(-1))
        try:
            with pytest.raises(_capi.MgrError):
                device.call("mgr_conv_pool_bwd_data", g.ptr, code.ptr, W, c.N, c.Hin, c.Win, c.Cin, c.ks, c.Cout, x.ptr)
            assert POOLED_REFUSAL in _last_error(device) and "pooled gradient" in _last_error(device)
            device.sync()
            assert x.untouched()
        finally:
            for a in (x, g, code):
                a.free()
            device.free(W)


def test_conv_case_one_element_into_its_allocations(device):
    """X, dY, Y and dX one float, code one byte into their allocations: only W of the forward has an alignment contract."""
    _check_case(device, cc.OFFSET_CASE, off=1)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
ALL3 = ("fwd", "data", "weights")
# what -> (N, Hin, Win, Cin, ks, Cout, entry points that must refuse, fragment of the message)
REFUSALS = {
    "cout-6": (3, 10, 10, 1, 5, 6, ALL3, "Cout must be a multiple of 4"),
    "ks-3": (3, 10, 10, 1, 3, 8, ALL3, "kernel size 3"),
    "ks-6": (3, 10, 10, 1, 6, 8, ALL3, "kernel size 6"),
    "hin-equals-ks": (3, 5, 10, 1, 5, 8, ALL3, "too small"),
    "win-equals-ks": (3, 10, 4, 1, 4, 8, ALL3, "too small"),
    "frame-over-lds": (1, 129, 128, 1, 5, 4, ("fwd", "weights"), "129x128x1 frame does not fit the LDS stage"),
    "pooled-over-lds": (1, 70, 70, 1, 5, 16, ("data",), "pooled gradient of a frame (33x33x16) does not fit the LDS stage"),
    "w-misaligned": (3, 10, 10, 1, 5, 8, ("fwd",), "W must be 16-byte aligned"),
    "workspace-short": (3, 10, 10, 1, 5, 8, ("weights",), "weight-gradient workspace"),
    "no-frames": (0, 10, 10, 1, 5, 8, ALL3, "bad shape (N 0"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_change_nothing(device, what):
    """Every refusal returns before any launch: the error names the reason and every output keeps its bits.  The buffers are as
    large as the refused shape would need (one frame at least)."""
    N, Hin, Win, Cin, ks, Cout, entries, fragment = REFUSALS[what]
    n1 = max(N, 1)
    Hp, Wp = max((Hin - ks + 1) // 2, 1), max((Win - ks + 1) // 2, 1)
    rng = np.random.RandomState(5)
    nx, npool, nw = n1 * Hin * Win * Cin, n1 * Hp * Wp * Cout, ks * ks * Cin * Cout
    X = Guarded(device, nx, salt=1, fill=rng.uniform(0, 1, nx).astype(np.float32))
    G = Guarded(device, npool, salt=2, fill=rng.standard_normal(npool).astype(np.float32))
    cin = Guarded(device, npool, item=1, salt=3, fill=np.zeros(npool, np.uint8))
    W = Guarded(device, nw + 1, salt=4, fill=rng.uniform(-0.05, 0.05, nw + 1).astype(np.float32))
    b = device.array(rng.uniform(-0.02, 0.02, Cout).astype(np.float32))
    Y, code, dX, gW, gb = (Guarded(device, n, item=i, salt=10 + k)
                           for k, (n, i) in enumerate(((npool, 4), (npool, 1), (nx, 4), (nw, 4), (Cout, 4))))
    need = max(int(device.lib.mgr_conv_pool_bwd_weights_ws_bytes(n1, Hin, Win, Cin, ks, Cout)), 16)
    ws = device.bytes(need)
    w_ptr = W.ptr + (4 if what == "w-misaligned" else 0)
    ws_bytes = need - 1 if what == "workspace-short" else need
    calls = {"fwd": ("mgr_conv_pool_fwd", X.ptr, N, Hin, Win, Cin, w_ptr, b, ks, Cout, Y.ptr, code.ptr),
             "data": ("mgr_conv_pool_bwd_data", G.ptr, cin.ptr, w_ptr, N, Hin, Win, Cin, ks, Cout, dX.ptr),
             "weights": ("mgr_conv_pool_bwd_weights", X.ptr, G.ptr, cin.ptr, N, Hin, Win, Cin, ks, Cout, gW.ptr, gb.ptr, ws, ws_bytes)}
    try:
        assert W.ptr % 16 == 0 and need % 8 == 0
        fill_workspace(device, ws)
        for e in entries:
            with pytest.raises(_capi.MgrError) as err:
                device.call(*calls[e])
            assert fragment in _last_error(device) and fragment in str(err.value), (e, _last_error(device))
        device.sync()
        for a in (Y, code, dX, gW, gb, X, G, cin, W):
            assert a.untouched()
        if what == "workspace-short":
            assert (ws.download().view(np.uint8) == 0xFF).all()
        if what == "pooled-over-lds":               # its forward is accepted (and leaves the context usable)
            device.call(*calls["fwd"])
            Y.body("Y"), code.body("code")
    finally:
        for a in (X, G, cin, W, Y, code, dX, gW, gb):
            a.free()
        device.free(b, ws)


# ---- one whole train step on a front-end that is none of the reference's ------------------------------------------------------------
def test_colour_nonsquare_frontend_train_step_matches_fp64(device):
    """input_shape [26, 21, 3]; conv_a 16 filters 5x5 (K = 75: partial<5,8>; Ho x Wo = 22 x 17 pooled to 11 x 8, a dropped
    column); conv_b 20 filters 4x4 (K = 256, Cout = 20: partial<4,8>; its data gradient at Ho x Wo = 8 x 5, pooled to 4 x 2);
    F = 160 into two residual BiLSTM(32) layers."""
    from mgr_amd.spec import NetworkSpec, frontend_layers
    from tests.test_gpu_rgb import _batch, _check_step, _train_engine
    fe = {"input_shape": [26, 21, 3], "layers": [{"name": "conv_a", "filters": 16, "kernel_size": 5},
                                                 {"name": "conv_b", "filters": 20, "kernel_size": 4}]}
    lay = frontend_layers(fe)
    assert [(c["Ho"], c["Wo"], c["Hp"], c["Wp"]) for c in lay] == [(22, 17, 11, 8), (8, 5, 4, 2)] and lay[-1]["F"] == 160
    assert [cc.branch_of(c["Cin"], c["ks"], c["Cout"]) for c in lay] == ["partial<5,8>", "partial<4,8>"]
    spec = NetworkSpec(
        streams=[{"name": "the_input", "noise": 0.0, "residual": True, "trainable": True, "frontend": fe,
                  "layers": [{"H": 32, "dropout": 0.0, "name": "blstm_1"}, {"H": 32, "dropout": 0.0, "name": "blstm_2"}]}],
        fusion=None, head={"dropout": 0.0, "C": 22, "dropout_name": "drop_4"},
        optimizer={"lr": 1e-4, "decay": 0.0, "clipvalue": 0.5, "maxnorm": 3.0}, name="rgb_colour_nonsquare")
    B, T, Lmax = 2, 24, 6
    eng, w = _train_engine(device, spec, B, T, Lmax)
    try:
        _check_step(eng, spec, *_batch(spec, B, T, Lmax, 13), w)
    finally:
        eng.close()
