"""-m gpu: mgr_lstm_scan_window (include/mgr.h K20, csrc/lstm_live.hip) against tests/live_ref.py: parity with the fp64 restatement,
bit equality of a session however it is cut into windows and wherever it sits among the sessions, idle sessions untouched, zero
tails, NaN behind n_valid never read, the residual, and the refusals."""
import os

import numpy as np
import pytest

import live_ref
from helpers import rel_err
from mgr_amd import _capi

pytestmark = pytest.mark.gpu

f32 = np.float32
T = 23
HS = [3, 64, 100, 257, 500, 512, 1024]     # (from 513 on the k range is not split: no LDS reduction, idle waves)
CANARY = f32(-77.25)
_worst = {}


def _data(H, S=1, seed=0):
    """Z (S, T, 4H) and U (H, 4H) in Keras layout, float32; U scaled so that the states stay in the cell's active range."""
    rng = np.random.default_rng(1000 * H + seed)
    Z = rng.standard_normal((S, T, 4 * H)).astype(f32)
    U = (rng.standard_normal((H, 4 * H)) / np.sqrt(H)).astype(f32)
    return Z, U


def _window(dev, Zw, Up_d, H, nv, nk, reverse, state=None, R=None, Yfill=None, h_check=True):
    """One call on Zw (S, Tw, 4H) in Keras layout; returns Y (S, Tw, H) and the state array (S, 2, H) after the call."""
    S, Tw = Zw.shape[:2]
    Zd = dev.array(live_ref.pack(Zw, H))
    Yd = dev.array(np.full((S, Tw, H), 0 if Yfill is None else Yfill, f32))
    st = None if reverse else dev.array(np.zeros((S, 2, H), f32) if state is None else state)
    Rd = None if R is None else dev.array(R)
    nv, nk = np.asarray(nv, np.int32), np.asarray(nk, np.int32)
    nvd, nkd = dev.array(nv), dev.array(nk)
    jobs = _capi.make_live_jobs([dict(Z=Zd, Up=Up_d, Y=Yd, ldy=H, R=Rd or 0, ldr=H if R is not None else 0, state=st or 0, H=H, reverse=int(reverse))])
    dev.call("mgr_lstm_scan_window", 1, jobs, S, Tw, nvd, nkd, nv.ctypes.data if h_check else 0, nk.ctypes.data if h_check else 0)
    Y = Yd.download()
    out = None if st is None else st.download()
    dev.free(*[a for a in (Zd, Yd, st, Rd, nvd, nkd) if a is not None])
    return Y, out


@pytest.fixture(scope="module", params=HS)
def case(request, device):
    H = request.param
    Z, U = _data(H)
    Up = device.array(live_ref.pack(U, H))
    Yf, st = _window(device, Z, Up, H, [T], [T], False)
    Yr, _ = _window(device, Z, Up, H, [T], [T], True)
    yield dict(H=H, Z=Z, U=U, Up=Up, Yf=Yf[0], Yr=Yr[0], st=st[0])
    device.free(Up)


def test_parity_with_the_fp64_restatement(case):
    """rel_err < 1e-4 (the project's bound for a forward pass), both directions and the final state (the measured values:
    profiles/live_parity.txt)."""
    Z64, U64 = case["Z"][0].astype(np.float64), case["U"].astype(np.float64)
    yf, (h, c) = live_ref.scan(Z64, U64, None, T, False)
    yr, _ = live_ref.scan(Z64, U64, None, None, True)
    errs = dict(fwd=rel_err(case["Yf"], yf), rev=rel_err(case["Yr"], yr), h=rel_err(case["st"][0], h), c=rel_err(case["st"][1], c))
    _worst[case["H"]] = errs
    print("H=%d" % case["H"], errs)
    assert max(errs.values()) < 1e-4, errs


@pytest.fixture(scope="module", autouse=True)
def _parity_profile():
    """Behind the module's tests: what the parity cases measured, printed - and written to the file MGR_LIVE_PARITY_OUT names
    (that is how profiles/live_parity.txt is made)."""
    yield
    if not _worst:
        return
    lines = ["mgr_lstm_scan_window against the fp64 restatement (tests/live_ref.py), %d frames, rel_err = max|a-b| / max|b|; bound 1e-4" % T]
    for H in sorted(_worst):
        lines.append("H=%4d  " % H + "  ".join("%s %.3e" % kv for kv in sorted(_worst[H].items())))
    lines.append("worst %.3e" % max(max(e.values()) for e in _worst.values()))
    print("\n".join(lines))
    out = os.environ.get("MGR_LIVE_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("cut", ["7", "1", "5+3"])
def test_windows_give_the_same_bits(case, device, cut):
    """A forward job as windows of 7, of 1, and of 5 kept + 3 lookahead == the one window of 23: kept frames and final state."""
    H, Z, Up = case["H"], case["Z"], case["Up"]
    chunk, look = {"7": (7, 0), "1": (1, 0), "5+3": (5, 3)}[cut]
    state, rows = np.zeros((1, 2, H), f32), []
    for s0, nv, nk in live_ref.plan_windows(T, chunk, look):
        Zw = np.full((1, chunk + look, 4 * H), np.nan, f32)
        Zw[0, :nv] = Z[0, s0:s0 + nv]
        Y, state = _window(device, Zw, Up, H, [nv], [nk], False, state=state)
        rows.append(Y[0, :nk])
        assert not Y[0, nv:].any()
    assert np.array_equal(np.concatenate(rows), case["Yf"])
    assert np.array_equal(state[0], case["st"])


def test_mixed_lengths_idle_sessions_and_tails(case, device):
    H, Up = case["H"], case["Up"]
    S = 5
    nv, nk = [0, 1, T, 3, T - 1], [0, 0, T, 2, T - 1]
    Z, _ = _data(H, S, seed=1)
    st0 = np.random.default_rng(5).uniform(-0.5, 0.5, (S, 2, H)).astype(f32)
    st0[0] = CANARY
    for reverse in (False, True):
        Y, st = _window(device, Z, Up, H, nv, nk, reverse, state=st0, Yfill=CANARY)
        assert (Y[0] == CANARY).all()                                   # the idle session's rows hold their canary
        for s in range(1, S):
            assert np.isfinite(Y[s, :nv[s]]).all() and (Y[s, :nv[s]] != CANARY).all()
            assert not Y[s, nv[s]:].any()                                # the tails are zero
            y64, s64 = live_ref.scan(Z[s, :nv[s]].astype(np.float64), case["U"].astype(np.float64),
                                     None if reverse else st0[s].astype(np.float64), nk[s], reverse)
            assert rel_err(Y[s, :nv[s]], y64) < 1e-4
            if not reverse and nk[s]:
                assert rel_err(st[s], np.stack(s64)) < 1e-4
        if not reverse:
            assert (st[0] == CANARY).all()                               # ... and so does its state
            assert np.array_equal(st[1], st0[1])                         # n_keep = 0 with n_valid > 0: the state is unchanged
            assert not np.array_equal(st[3], st0[3])


def test_reverse_never_reads_behind_n_valid(case, device):
    H, Up = case["H"], case["Up"]
    nv = 9
    Z0 = case["Z"].copy()
    Z0[0, nv:] = 0
    Zn = Z0.copy()
    Zn[0, nv:] = np.nan
    a, _ = _window(device, Z0, Up, H, [nv], [nv], True)
    b, _ = _window(device, Zn, Up, H, [nv], [nv], True)
    assert np.isfinite(b).all() and np.array_equal(a, b)
    y64, _ = live_ref.scan(Z0[0, :nv].astype(np.float64), case["U"].astype(np.float64), None, None, True)
    assert rel_err(b[0, :nv], y64) < 1e-4


def test_residual_is_added(case, device):
    H, Up = case["H"], case["Up"]
    R = np.random.default_rng(9).standard_normal((1, T, H)).astype(f32)
    Y, _ = _window(device, case["Z"], Up, H, [T], [T], False, R=R)
    assert np.array_equal(Y[0], case["Yf"] + R[0])


def test_a_sessions_bits_do_not_depend_on_its_slot(case, device):
    H, Up = case["H"], case["Up"]
    S = 5
    Z = np.full((S, T, 4 * H), np.nan, f32)
    for slot in (0, 3):
        Zs = Z.copy()
        Zs[slot] = case["Z"][0]
        nv = np.zeros(S, np.int32)
        nv[slot] = T
        Y, st = _window(device, Zs, Up, H, nv, nv, False)
        assert np.array_equal(Y[slot], case["Yf"]) and np.array_equal(st[slot], case["st"])
    # ... nor on the company: every slot busy, in the second workgroup as well
    Zs, _ = _data(H, S, seed=2)
    Zs[4] = case["Z"][0]
    Y, st = _window(device, Zs, Up, H, [T] * S, [T] * S, False)
    assert np.array_equal(Y[4], case["Yf"]) and np.array_equal(st[4], case["st"])


def test_refusals_enqueue_nothing(device):
    H = 8
    Z, U = _data(H)
    Up, Zd = device.array(live_ref.pack(U, H)), device.array(live_ref.pack(Z, H))
    Yd, st = device.array(np.full((1, T, H), CANARY, f32)), device.array(np.full((1, 2, H), CANARY, f32))
    one = device.array(np.int32([1]))
    good = dict(Z=Zd, Up=Up, Y=Yd, ldy=H, state=st, H=H, reverse=0)
    nv, nk = np.int32([5]), np.int32([6])
    with pytest.raises(_capi.MgrError, match="n_keep"):                                  # n_keep > n_valid on the host copies
        device.call("mgr_lstm_scan_window", 1, _capi.make_live_jobs([good]), 1, T, one, one, nv.ctypes.data, nk.ctypes.data)
    for change in (dict(H=1025, ldy=1025),        # H above the bound
                   dict(H=0),
                   dict(state=0),                  # a forward job without a state
                   dict(reverse=1),                # a reverse job with one
                   dict(Y=0),
                   dict(Z=Zd.ptr + 4),             # misaligned
                   dict(ldy=H - 1)):
        with pytest.raises(_capi.MgrError):
            device.call("mgr_lstm_scan_window", 1, _capi.make_live_jobs([dict(good, **change)]), 1, T, one, one, 0, 0)
    with pytest.raises(_capi.MgrError):
        device.call("mgr_lstm_scan_window", 9, _capi.make_live_jobs([good] * 9), 1, T, one, one, 0, 0)
    device.sync()
    assert (Yd.download() == CANARY).all() and (st.download() == CANARY).all()           # nothing was enqueued
    device.free(Up, Zd, Yd, st, one)
