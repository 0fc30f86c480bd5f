"""-m gpu, library level: what Engine's per-sample lengths rest on, per kernel family.

Forward: a REVERSE recurrence whose gate pre-activations are zero in a sample's tail (mgr_seq_zero_tail) keeps c = 0 and h = 0
through it - mgr_tanh(0) == 0 and 0 * U == 0 on every matrix pipe - so its outputs at t < len are, bit for bit, those of the same
real rows embedded in a shorter or longer T; a forward job is causal and agrees at t < len whatever its tail holds.
"h = 0" needs one qualification, read in csrc/lstm_cluster.hip: the kernels whose workgroups exchange h_t between CUs carry the
hand-off's epoch parity in the mantissa LSB of every h they publish, and Y and the recurrence use that same word - there a zero
state is the bit pattern 0 or 1 (0 or 2^-149), alternating every two steps.  2^-149 times any |U| < 0.5 rounds to zero, so c and
everything at t < len are exact all the same: asserted here for every family as bits(Y) <= 1 in the tail, c == 0 on bits, and the
bit comparison of the real rows; the families without an exchange are held to bits(Y) == 0, and which family gave which is printed.
(The two embeddings differ by 16 steps, a multiple of the parity's period of 4: the real rows carry the same parity in both.)
Backward: with the reverse job's saved gates zeroed in the tail and dY zero there, dZ is 0 in the tail and dZ at t < len, dbsum
and dzmax do not depend on the embedding; without the gate fill dZ in the tail is an ordinary gradient (the control).  The
same qualification, read in csrc/lstm_cluster_bwd.hip: the multi-CU BPTT forms exchange dz_t with the epoch parity in the mantissa
LSB, so an exact zero travels as 0 or 2^-149 and the tail of either direction holds zeros and multiples of 2^-149 that went
through a few products with |U| < 1.  Measured on an MI355X: up to 1e-44.  Any normal number absorbs them exactly; only results
that are themselves zero (a saturated gate's column, the sample of length 0) show them.  So "zero" is asserted as |x| below the
smallest normal float32 (2^-126: a factor 2^23 above what one parity bit is), and "equal between the embeddings" as equal bits
wherever either value is a normal number and a difference below 2^-126 elsewhere; the control's tail gradient must exceed 1e-6.
The forms whose tails came out as exact zeros are printed.

B = 17 (two 16-sample groups, the second with one sample), lengths spread over [0, 21] with 0, 1 and 21, embedded at T = 21 and 37."""
import ctypes as C

import numpy as np
import pytest

from mgr_amd import _capi

pytestmark = pytest.mark.gpu
f32 = np.float32
B = 17
LENS = np.array([0, 1, 21, 20, 2, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 10, 4], np.int32)
TS = (21, 37)
assert LENS.size == B and LENS.max() == TS[0]

# (tune key 0 = MGR_TUNE_SCAN_PATH, key 14 = MGR_TUNE_SCAN_F32_MFMA, launch form): the settings existing tests run at these widths
FWD_VARIANTS = {
    32: [(0, 0, "plain"), (3, 0, "plain"), (0, 1, "plain"), (0, 0, "fused_any")],
    100: [(0, 0, "plain"), (1, 0, "plain"), (2, 0, "plain"), (3, 0, "plain"), (4, 0, "plain"), (0, 1, "plain"), (0, 0, "fused_any")],
    300: [(0, 0, "plain"), (1, 0, "plain"), (3, 0, "plain"), (0, 1, "plain"), (0, 0, "fused_any")],
}
BPTT_FORMS = {
    32: ["AUTO", "TRIMMED", "YIELDING", "DIRECT", "FUSED", "FUSED_DIRECT", "SINGLE_CU"],
    100: ["AUTO", "TRIMMED", "YIELDING", "DIRECT", "FUSED", "FUSED_DIRECT", "SINGLE_CU"],
    300: ["AUTO"],
}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _status(dev):
    st = (C.c_uint * 4)()
    dev.call("mgr_scan_status_ex", st)
    return int(st[0])


class Layer:
    """Both directions of a random layer of width H: packed U per direction and the REAL rows of Z and dY per sample."""

    def __init__(self, dev, H, seed):
        rng = np.random.default_rng(seed)
        self.dev, self.H = dev, H
        self.Up = []
        for _ in range(2):
            U = dev.array((rng.standard_normal((H, 4 * H)) * 0.1 / np.sqrt(H)).astype(f32))
            Up = dev.empty((H, 4 * H))
            dev.call("mgr_lstm_pack", U, Up, H, H, 0)
            dev.free(U)
            self.Up.append(Up)
        self.z_real = [(rng.standard_normal((B, TS[0], 4 * H)) * 0.5).astype(f32) for _ in range(2)]
        self.dy_real = [rng.standard_normal((B, TS[0], H)).astype(f32) for _ in range(2)]
        self.lens = dev.array(LENS)

    def embed(self, real, T, junk_seed, zero_tail):
        """The real rows of every sample at t < len inside [B, T, row]; the tails hold junk (or zeros)."""
        rng = np.random.default_rng(junk_seed)
        out = np.zeros((B, T, real.shape[2]), f32) if zero_tail else (rng.standard_normal((B, T, real.shape[2])) * 2.0).astype(f32)
        for b, n in enumerate(LENS):
            out[b, :n] = real[b, :n]
        return out

    def close(self):
        self.dev.free(*self.Up, self.lens)


def forward(dev, lay, T, path=0, f32_mfma=0, form="plain", fill=True):
    """One multi-scan call over (forward job, reverse job) with the states kept; the reverse job's Z tails zeroed by mgr_seq_zero_tail
    first (fill).  Returns per direction dict(Y, gates, cs) on the host, and the device gates / cs for a BPTT."""
    H = lay.H
    Z = [dev.array(lay.embed(lay.z_real[d], T, 100 * T + d, zero_tail=False)) for d in range(2)]
    Y = [dev.array(np.full((B, T, H), 7.0, f32)) for _ in range(2)]
    G = [dev.array(np.full((B, T, H, 4), 7.0, f32)) for _ in range(2)]
    Cs = [dev.array(np.full((B, T, H), 7.0, f32)) for _ in range(2)]
    if fill:
        dev.call("mgr_seq_zero_tail", 1, _capi.make_seq_fill_jobs([(Z[1], 4 * H, 4 * H, B, T)]), lay.lens)
    jobs = [dict(Z=Z[d], Up=lay.Up[d], Y=Y[d], ldy=H, R=0, ldr=0, gates=G[d], cs=Cs[d], B=B, T=T, H=H, reverse=d) for d in range(2)]
    arr = _capi.make_scan_jobs(jobs)
    opts = _capi.make_launch_opts(_capi.SCAN_FORM_FUSED_ANY if form == "fused_any" else _capi.SCAN_FORM_PLAIN, 0)
    dev.call("mgr_tune", _capi.TUNE_SCAN_PATH, path)
    dev.call("mgr_tune", _capi.TUNE_SCAN_F32_MFMA, f32_mfma)
    dev.call("mgr_tune", _capi.TUNE_SCAN_SYNC_CHECK, 1)
    try:
        need = dev.lib.mgr_lstm_scan_fwd_multi_ws_bytes(dev.ctx, 2, arr, C.byref(opts))
        assert need > 0
        ws = dev.bytes(need)
        _capi.check(dev.lib.mgr_lstm_scan_fwd_multi_ex(dev.ctx, 2, arr, ws.ptr, ws.nbytes, C.byref(opts)))
    finally:
        dev.call("mgr_tune", _capi.TUNE_SCAN_PATH, 0)
        dev.call("mgr_tune", _capi.TUNE_SCAN_F32_MFMA, 0)
        dev.call("mgr_tune", _capi.TUNE_SCAN_SYNC_CHECK, 0)
    dev.sync()
    host = [dict(Y=Y[d].download(), gates=G[d].download(), cs=Cs[d].download()) for d in range(2)]
    dev.free(*Z, *Y, ws)
    return host, G, Cs


def real_part_equal(a, b, what):
    """a, b: [B, T, ...] arrays of two embeddings: the rows t < len hold the same bits."""
    for i, n in enumerate(LENS):
        assert np.array_equal(bits(a[i, :n]), bits(b[i, :n])), (what, i, int(n))


TINY = float(np.finfo(f32).tiny)        # 2^-126, the smallest normal float32


def equal_above_the_denormals(a, b, what):
    """Equal bits wherever either value is a normal number; elsewhere both are zeros or denormals."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    normal = (np.abs(a) >= TINY) | (np.abs(b) >= TINY)
    assert np.array_equal(bits(a)[normal], bits(b)[normal]), what
    assert np.all(np.abs(a.astype(np.float64) - b.astype(np.float64))[~normal] < TINY), what


@pytest.mark.parametrize("H", [32, 100, 300])
def test_reverse_scan_holds_zero_state_through_the_tail_in_every_family(device, H):
    dev = device
    dev.call("mgr_scan_status_clear")
    lay = Layer(dev, H, 5 + H)
    ran = []
    try:
        for path, mfma, form in FWD_VARIANTS[H]:
            out = {}
            # one workgroup holds the whole recurrent matrix of its batch group: the plain narrow kernel, or forced (path 2)
            no_exchange = path == 2 or (path == 0 and H == 32 and form == "plain")
            tail_bits = 0
            for T in TS:
                host, G, Cs = forward(dev, lay, T, path, mfma, form)
                dev.free(*G, *Cs)
                assert _status(dev) == 0, (H, path, mfma, form, T)
                out[T] = host
                rev = host[1]
                worst_bits = 0
                for b, n in enumerate(LENS):
                    # c is exactly zero through the tail (bits: not -0.0 either); h is zero, or zero with the hand-off's parity bit
                    assert not bits(rev["cs"][b, n:]).any(), (H, path, mfma, form, T, b)
                    if n < T:
                        worst_bits = max(worst_bits, int(bits(rev["Y"][b, n:]).max()))
                assert worst_bits <= 1, (H, path, mfma, form, T, worst_bits)
                if no_exchange:
                    assert worst_bits == 0, (H, path, mfma, form, T)
                tail_bits = max(tail_bits, worst_bits)
                assert np.isfinite(rev["Y"]).all() and np.abs(rev["Y"]).max() > 0.02
                assert np.isfinite(host[0]["Y"]).all()
            for d, dname in enumerate(("forward job", "reverse job")):
                for k in ("Y", "gates", "cs"):
                    real_part_equal(out[TS[0]][d][k], out[TS[1]][d][k], (H, path, mfma, form, dname, k))
            ran.append("path %d, f32_mfma %d, %s: tail h %s" % (path, mfma, form, "== 0" if tail_bits == 0 else "0 or 2^-149"))
        print("H = %d: zero state held and embeddings bit-equal under: %s" % (H, "; ".join(ran)))
    finally:
        lay.close()


def bptt(dev, lay, T, G, Cs, form):
    """BPTT over (forward job, reverse job) from the kept states, dY = the real rows with ZERO tails.  Returns per direction
    dict(dZ, dzmax, dbsum) on the host."""
    H = lay.H
    dY = [dev.array(lay.embed(lay.dy_real[d], T, 0, zero_tail=True)) for d in range(2)]
    dZ = [dev.array(np.full((B, T, 4 * H), 7.0, f32)) for _ in range(2)]
    zm = [dev.array(np.full((B, 4 * H), 0xFFFFFFFF, np.uint32)) for _ in range(2)]
    zs = [dev.array(np.full((B, 4 * H), np.nan, f32)) for _ in range(2)]
    jobs = [dict(dY=dY[d], gates=G[d], cs=Cs[d], Up=lay.Up[d], dZ=dZ[d], lddy=H, B=B, T=T, H=H, reverse=d, dzmax=zm[d], dbsum=zs[d])
            for d in range(2)]
    arr = _capi.make_scan_bwd_jobs(jobs)
    ws = dev.bytes(dev.lib.mgr_lstm_scan_bwd_multi_ws_bytes(2, arr))
    opts = _capi.make_launch_opts(getattr(_capi, "BPTT_FORM_" + form), 0)
    dev.call("mgr_tune", _capi.TUNE_SCAN_SYNC_CHECK, 1)
    try:
        _capi.check(dev.lib.mgr_lstm_scan_bwd_multi_ex(dev.ctx, 2, arr, ws.ptr, ws.nbytes, C.byref(opts)))
    finally:
        dev.call("mgr_tune", _capi.TUNE_SCAN_SYNC_CHECK, 0)
    dev.sync()
    host = [dict(dZ=dZ[d].download(), dzmax=zm[d].download(), dbsum=zs[d].download()) for d in range(2)]
    dev.free(*dY, *dZ, *zm, *zs, ws)
    return host


@pytest.mark.parametrize("H", [32, 100, 300])
def test_bptt_over_zeroed_gate_tails_gives_zero_dz_there_in_every_form(device, H):
    dev = device
    dev.call("mgr_scan_status_clear")
    lay = Layer(dev, H, 9 + H)
    kept = {}
    try:
        for T in TS:
            _, G, Cs = forward(dev, lay, T)
            kept[T] = (G, Cs)
        # the control first, on the gates as the scan left them: hard_sigmoid(0) = 0.5 lies inside (0, 1), the tail steps pass gradient on
        ctrl = bptt(dev, lay, TS[1], *kept[TS[1]], "AUTO")[1]["dZ"]
        assert all(np.abs(ctrl[b, n:]).max() > 1e-6 for b, n in enumerate(LENS) if 0 < n < TS[1]), "no gradient in the tail without the fill: the control is blind"
        for T in TS:
            G = kept[T][0]
            dev.call("mgr_seq_zero_tail", 1, _capi.make_seq_fill_jobs([(G[1], 4 * H, 4 * H, B, T)]), lay.lens)
        ran = []
        for form in BPTT_FORMS[H]:
            out = {T: bptt(dev, lay, T, *kept[T], form) for T in TS}
            assert _status(dev) == 0, (H, form)
            worst = 0.0
            for T in TS:
                for d in range(2):
                    dz = out[T][d]["dZ"]
                    assert np.isfinite(dz).all()
                    for b, n in enumerate(LENS):
                        if n < T:
                            worst = max(worst, float(np.abs(dz[b, n:]).max()))
                    assert worst < TINY, (H, form, T, d, worst)         # zero in the tail (to the exchange's parity bit), both directions
                assert np.abs(out[T][1]["dZ"]).max() > 1e-3
            for d, dname in enumerate(("forward job", "reverse job")):
                a, b = out[TS[0]][d], out[TS[1]][d]
                for i, n in enumerate(LENS):
                    equal_above_the_denormals(a["dZ"][i, :n], b["dZ"][i, :n], (H, form, dname, "dZ", i))
                equal_above_the_denormals(a["dzmax"].view(f32), b["dzmax"].view(f32), (H, form, dname, "dzmax"))
                equal_above_the_denormals(a["dbsum"], b["dbsum"], (H, form, dname, "dbsum"))
            ran.append("%s (tail dZ %s)" % (form, "== 0" if worst == 0 else "<= %.1e" % worst))
        print("H = %d: BPTT forms %s" % (H, ", ".join(ran)))
    finally:
        for G, Cs in kept.values():
            dev.free(*G, *Cs)
        lay.close()
