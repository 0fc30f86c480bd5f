"""-m gpu: the split weight planes that mgr_lstm_input_proj_dropout_ts keeps in a projection workspace for FROZEN weights
(mgr_weight_planes_cache, gemm_split.hip) at every call order mgr.h allows: several weights, batch sizes and unit counts on one
workspace, the workspace rewritten by other library calls or through a view into it, more weights than the table holds, freed and
reallocated buffers, a hit on another stream.  A stale hit is silent - finite, plausible numbers from the wrong weights - so every
projection here is checked bit for bit against an UNCACHED call (a private copy of the weights, never declared frozen, and a fresh
workspace full of 0xFF) and against numpy fp64.  Each scenario ends by proving the cache is still on: weights rewritten behind the
promise still give the old weights' result.  MGR_FUZZ_PLANES sets the number of random sequences (default 6)."""
import hashlib
import os

import numpy as np
import pytest

from tests.test_gpu_split_gemm import _proj_ref, _split_rows

pytestmark = pytest.mark.gpu
f32 = np.float32
T = 130
LDT = 256       # T padded to whole row tiles of 128


def _plane_offset(B, F):
    """Byte offset of the largest-|W| word block inside a projection workspace (gemm_split.hip: lists [4B][Fp32] | counts [4B] |
    words (256 bytes) | weight planes | list positions); the planes follow 256 bytes later."""
    fp32 = (F + 31) // 32 * 32
    up = lambda x: (x + 255) // 256 * 256    # noqa: E731
    return up(4 * B * fp32 * 4) + up(4 * B * 4)


class Rig:
    """Inputs of one (F, Hmax, Bmax) family: X [Bmax, T, F] (the split copy of its first B samples is a prefix of one buffer), a
    bias for Hmax (its prefix is a bias for any H), masks per (B, name); projections, uncached projections and fp64 references."""

    def __init__(self, dev, seed, F, Hmax, Bmax, p=0.5):
        self.dev, self.F, self.Hmax, self.Bmax, self.p = dev, F, Hmax, Bmax, p
        self.rng = np.random.default_rng(seed)
        self.X = self.rng.uniform(-2, 2, (Bmax, T, F)).astype(f32)
        self.XS = dev.array(_split_rows(self.X, LDT))
        self.bias = self.rng.standard_normal(4 * Hmax).astype(f32)
        self.db = dev.array(self.bias)
        self.masks = {}
        self._memo = {}

    def weights(self, H=None, scale=0.1):
        return (self.rng.standard_normal((self.F, 4 * (H or self.Hmax))) * scale).astype(f32)

    def mask(self, B, name="a", factor=2.0, empty_gate=False):
        """[4, B, F] Keras dropout mask (entries 0 or factor), one per (B, name); empty_gate: gate 2 of sample 0 keeps nothing."""
        key = (B, name, factor, empty_gate)
        if key not in self.masks:
            M = ((self.rng.random((4, B, self.F)) >= self.p) * f32(factor)).astype(f32)
            if empty_gate:
                M[2, 0, :] = 0.0
            self.masks[key] = (M, self.dev.array(M))
        return self.masks[key]

    def ws_bytes(self, B=None, H=None):
        return self.dev.lib.mgr_lstm_input_proj_dropout_ts_ws_bytes(B or self.Bmax, self.F, H or self.Hmax)

    def proj(self, Wp, ws, B, H, mask):
        """One projection on the current stream; mask = (host, device) or None."""
        dev = self.dev
        Z = dev.empty((B, T, 4 * H))
        Z.upload(np.full((B, T, 4 * H), np.nan, f32))
        dev.call("mgr_lstm_input_proj_dropout_ts", self.XS, LDT, mask[1] if mask else 0, self.p, Wp, self.db, Z, B, T, self.F, H, ws, ws.nbytes)
        z = Z.download()
        Z.free()
        return z

    def expect(self, W, B, H, mask):
        """(uncached result, fp64 reference, bound) for weights W [F][4H] (host) at (B, mask), memoised by content."""
        key = (hashlib.sha1(W.tobytes()).hexdigest(), W.shape, B, H, None if mask is None else id(mask[0]))
        if key not in self._memo:
            dev = self.dev
            Wc = dev.array(np.ascontiguousarray(W))
            dev.call("mgr_weight_planes_cache", Wc, 0)      # (never a promise: rebuilt by this call whatever the tables say)
            ws = dev.bytes(self.ws_bytes(B, H))
            dev.call("mgr_memset", ws, 0xFF, ws.nbytes)
            z = self.proj(Wc, ws, B, H, mask)
            Wc.free()
            ws.free()
            ref = _proj_ref(self.X[:B], None if mask is None else mask[0], W, self.bias[:4 * H])
            self._memo[key] = (z, ref, 2e-5 * max(1.0, np.abs(ref).max()))
        return self._memo[key]

    def check(self, z, W, B, H, mask, what=""):
        u, ref, tol = self.expect(W, B, H, mask)
        assert np.array_equal(z.view(np.uint32), u.view(np.uint32)), "differs from the uncached call by up to %s: %s" % (
            np.nanmax(np.abs(z - u)), what)
        assert np.all(np.isfinite(z)) and np.abs(z - ref).max() <= tol, "differs from fp64 by %s > %s: %s" % (np.abs(z - ref).max(), tol, what)

    def still_cached(self, dW, W, ws, B, H, mask):
        """The same key once more: a hit.  Weights rewritten BEHIND the promise must still give W's result (the kept planes really are
        reused - the fix must not turn the cache off); afterwards W is restored and declared again."""
        self.check(self.proj(dW, ws, B, H, mask), W, B, H, mask, "repeat of the last key")
        dW.view(0, (W.size,)).upload(self.weights(W.shape[1] // 4, 0.3).reshape(-1))
        self.check(self.proj(dW, ws, B, H, mask), W, B, H, mask, "weights rewritten behind the promise")
        dW.view(0, (W.size,)).upload(W.reshape(-1))
        self.dev.call("mgr_weight_planes_cache", dW, 1)


@pytest.mark.parametrize("b_frozen", [True, False])
def test_two_weights_alternate_on_one_workspace(device, b_frozen):
    """proj(A, ws), proj(B, ws), proj(A, ws): the third call must not find A's planes in ws - B's are there now (ADVICE: a rebuild
    left the other entries naming the same workspace in place, frozen B or not)."""
    dev = device
    r = Rig(dev, 11, F=600, Hmax=300, Bmax=2)
    B, H = 2, 300
    m = r.mask(B)
    WA, WB = r.weights(), r.weights(scale=0.2)
    dA, dB = dev.array(WA), dev.array(WB)
    ws = dev.bytes(r.ws_bytes())
    dev.call("mgr_memset", ws, 0xFF, ws.nbytes)
    dev.call("mgr_weight_planes_cache", dA, 1)
    dev.call("mgr_weight_planes_cache", dB, 1 if b_frozen else 0)
    for i, (dW, W) in enumerate(((dA, WA), (dB, WB), (dA, WA), (dB, WB), (dA, WA))):
        r.check(r.proj(dW, ws, B, H, m), W, B, H, m, "call %d" % i)
    r.still_cached(dA, WA, ws, B, H, m)
    for a in (dA, dB, ws):
        a.free()


def test_batch_size_is_part_of_the_key(device):
    """The planes start 4 B Fp32 words (+ counts) into the workspace: the same (Wp, ws, F, H) at another B reads them from another
    offset, and the lists of the larger B cover part of the smaller B's planes.  Then B = 1 and B = 5 with a gate of a sample that
    keeps no feature at all."""
    dev = device
    r = Rig(dev, 12, F=300, Hmax=200, Bmax=5)
    H = 200
    W = r.weights()
    dW = dev.array(W)
    ws = dev.bytes(r.ws_bytes())
    dev.call("mgr_memset", ws, 0xFF, ws.nbytes)
    dev.call("mgr_weight_planes_cache", dW, 1)
    for B, empty in ((2, False), (3, False), (2, False), (1, True), (5, True), (2, False)):
        m = r.mask(B, empty_gate=empty)
        r.check(r.proj(dW, ws, B, H, m), W, B, H, m, "B = %d" % B)
    r.still_cached(dW, W, ws, 2, H, r.mask(2))
    for a in (dW, ws):
        a.free()


def test_same_weight_and_workspace_two_unit_counts(device):
    """One Wp buffer (sized for the larger H) and one workspace at two H: each call reads the [F][4H] matrix at the start of the
    buffer, and the planes of one H are not those of the other."""
    dev = device
    r = Rig(dev, 13, F=256, Hmax=300, Bmax=2)
    B = 2
    m = r.mask(B)
    Wbig = r.weights(300)
    flat = Wbig.reshape(-1)
    dW = dev.array(Wbig)
    ws = dev.bytes(r.ws_bytes())
    dev.call("mgr_memset", ws, 0xFF, ws.nbytes)
    dev.call("mgr_weight_planes_cache", dW, 1)
    for H in (300, 100, 300, 100):
        W = flat[:r.F * 4 * H].reshape(r.F, 4 * H)
        r.check(r.proj(dW, ws, B, H, m), W, B, H, m, "H = %d" % H)
    r.still_cached(dW, flat[:r.F * 400].reshape(r.F, 400), ws, B, 100, m)
    for a in (dW, ws):
        a.free()


@pytest.mark.parametrize("how", ["memset", "d2d", "h2d", "h2d_async", "param_grads", "memset_view"])
def test_workspace_rewritten_by_the_library_between_two_hits(device, how):
    """A kept entry, then a library call that writes the workspace (or part of it, through a pointer INTO it that reaches the plane
    region), then the same key: the planes must be rebuilt, not read back from what the other call left."""
    dev = device
    r = Rig(dev, 14, F=200, Hmax=100, Bmax=3)
    B, H = 3, 100
    m = r.mask(B)
    W = r.weights()
    dW = dev.array(W)
    need = r.ws_bytes()
    if how == "param_grads":
        need = max(need, dev.lib.mgr_lstm_param_grads_dropout_ts_ws_bytes(B, T, r.F, H, LDT))
    ws = dev.bytes(need)
    dev.call("mgr_memset", ws, 0xFF, ws.nbytes)
    dev.call("mgr_weight_planes_cache", dW, 1)
    r.check(r.proj(dW, ws, B, H, m), W, B, H, m, "build")
    r.check(r.proj(dW, ws, B, H, m), W, B, H, m, "hit")
    junk = r.rng.standard_normal(ws.size).astype(f32)
    if how == "memset":
        dev.call("mgr_memset", ws, 0xFF, ws.nbytes)
    elif how == "d2d":
        src = dev.array(junk)
        dev.call("mgr_d2d", ws, src, ws.nbytes)
        src.free()
    elif how == "h2d":
        ws.upload(junk)
    elif how == "h2d_async":
        pin = dev.pinned(junk.shape)
        pin[:] = junk
        dev.h2d_async(ws, pin)
    elif how == "param_grads":
        Hs = dev.array(r.rng.standard_normal((B, T, H)).astype(f32))
        dZ = dev.array((r.rng.standard_normal((B, T, 4 * H)) * 0.3).astype(f32))
        gW, gU, gb = dev.empty((r.F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
        dev.call("mgr_lstm_param_grads_dropout_ts", r.XS, LDT, m[1], r.p, Hs, H, dZ, gW, gU, gb, B, T, r.F, H, 0, ws, ws.nbytes, 0, 0, 0, 0)
        for a in (Hs, dZ, gW, gU, gb):
            a.free()
    else:
        start = _plane_offset(B, r.F) - 512             # 512 bytes in front of the word block, ending 4 KiB into the planes
        dev.call("mgr_memset", ws.ptr + start, 0xFF, 512 + 256 + 4096)
    r.check(r.proj(dW, ws, B, H, m), W, B, H, m, "after " + how)
    r.still_cached(dW, W, ws, B, H, m)
    for a in (dW, ws):
        a.free()


def test_more_frozen_weights_than_the_tables_hold(device):
    """40 frozen weights (the tables hold MGR_MAX_FROZEN = 32), each with its own workspace, projected round-robin three times:
    whatever is forgotten is rebuilt, nothing is mixed up."""
    dev = device
    r = Rig(dev, 15, F=128, Hmax=64, Bmax=2)
    B, H = 2, 64
    m = r.mask(B)
    Ws = [r.weights() for _ in range(40)]
    dWs = [dev.array(W) for W in Ws]
    wss = [dev.bytes(r.ws_bytes()) for _ in range(40)]
    for dW in dWs:
        dev.call("mgr_weight_planes_cache", dW, 1)
    for rnd in range(3):
        for i in range(40):
            r.check(r.proj(dWs[i], wss[i], B, H, m), Ws[i], B, H, m, "round %d weight %d" % (rnd, i))
    r.still_cached(dWs[39], Ws[39], wss[39], B, H, m)
    for a in dWs + wss:
        a.free()


def test_freed_and_reallocated_buffers(device):
    """Wp and ws are views 4 KiB into larger buffers.  After the buffers are freed, neither the promise nor the planes may outlive
    them: a new buffer the allocator hands out at the same address holds new weights, which are projected first WITHOUT a promise
    and then with one.  (The case has teeth only when the allocator returns the same addresses; the test says which way it went.)"""
    dev = device
    r = Rig(dev, 16, F=256, Hmax=128, Bmax=2)
    B, H = 2, 128
    m = r.mask(B)
    off = 1024                                           # floats: 4 KiB
    W1, W2 = r.weights(), r.weights(scale=0.25)
    wblob, sblob = dev.empty((off + W1.size,)), dev.bytes(4 * off + r.ws_bytes())
    dW, ws = wblob.view(off, W1.shape), sblob.view(off, (r.ws_bytes() // 4,))
    dW.upload(W1)
    dev.call("mgr_weight_planes_cache", dW, 1)
    r.check(r.proj(dW, ws, B, H, m), W1, B, H, m, "build")
    r.check(r.proj(dW, ws, B, H, m), W1, B, H, m, "hit")
    old = (wblob.ptr, sblob.ptr)
    wblob.free()
    sblob.free()
    wblob, sblob = dev.empty((off + W1.size,)), dev.bytes(4 * off + r.ws_bytes())
    reused = (wblob.ptr, sblob.ptr) == old
    print("freed and reallocated: the allocator %s the same addresses" % ("returned" if reused else "did NOT return"))
    dW, ws = wblob.view(off, W1.shape), sblob.view(off, (r.ws_bytes() // 4,))
    dW.upload(W2)
    r.check(r.proj(dW, ws, B, H, m), W2, B, H, m, "new buffers, no promise (same addresses: %s)" % reused)
    dev.call("mgr_weight_planes_cache", dW, 1)
    r.check(r.proj(dW, ws, B, H, m), W2, B, H, m, "new buffers, frozen (same addresses: %s)" % reused)
    r.still_cached(dW, W2, ws, B, H, m)
    wblob.free()
    sblob.free()


def test_hit_on_another_stream_ordered_by_an_event(device):
    """The legal cross-stream reuse (mgr.h): the building call on stream 1 behind a 20 ms delay, an event, stream 2 waits for it
    and hits - the hit must read the planes the build wrote, not what was in the workspace before."""
    dev = device
    r = Rig(dev, 17, F=400, Hmax=256, Bmax=2)
    B, H = 2, 256
    m = r.mask(B)
    W = r.weights()
    dW = dev.array(W)
    ws = dev.bytes(r.ws_bytes())
    dev.call("mgr_memset", ws, 0xFF, ws.nbytes)
    dev.call("mgr_weight_planes_cache", dW, 1)
    Z1, Z2 = dev.array(np.full((B, T, 4 * H), np.nan, f32)), dev.array(np.full((B, T, 4 * H), np.nan, f32))
    dev.sync()
    try:
        dev.stream(1)
        dev.call("mgr_stream_delay", 20000)
        dev.call("mgr_lstm_input_proj_dropout_ts", r.XS, LDT, m[1], r.p, dW, r.db, Z1, B, T, r.F, H, ws, ws.nbytes)
        dev.record(5)
        dev.stream(2)
        dev.wait_event(2, 5)
        dev.call("mgr_lstm_input_proj_dropout_ts", r.XS, LDT, m[1], r.p, dW, r.db, Z2, B, T, r.F, H, ws, ws.nbytes)
        z1, z2 = Z1.download(), Z2.download()
        dev.sync()
    finally:
        dev.stream(0)
    r.check(z1, W, B, H, m, "build on stream 1")
    r.check(z2, W, B, H, m, "hit on stream 2")
    r.still_cached(dW, W, ws, B, H, m)
    for a in (dW, ws, Z1, Z2):
        a.free()


def test_kept_lists_after_a_hit_feed_the_weight_gradient(device):
    """mgr_lstm_param_grads_dropout_ts reading its lists, counts and mask factor from the workspace of a projection that HIT the
    cache (proj_ws): the same dW bits as the call that builds its own - a hit still writes this call's lists and factor (the build
    before it ran with another mask and another factor)."""
    dev = device
    r = Rig(dev, 18, F=300, Hmax=128, Bmax=3)
    B, H = 3, 128
    m1, m2 = r.mask(B, "one", 2.0), r.mask(B, "two", 2.5)
    W = r.weights()
    dW = dev.array(W)
    ws = dev.bytes(r.ws_bytes())
    dev.call("mgr_weight_planes_cache", dW, 1)
    r.check(r.proj(dW, ws, B, H, m2), W, B, H, m2, "build, mask two")
    r.check(r.proj(dW, ws, B, H, m1), W, B, H, m1, "hit, mask one")
    Hs = dev.array(r.rng.standard_normal((B, T, H)).astype(f32))
    dZ = dev.array((r.rng.standard_normal((B, T, 4 * H)) * 0.3).astype(f32))
    pg = dev.bytes(dev.lib.mgr_lstm_param_grads_dropout_ts_ws_bytes(B, T, r.F, H, LDT))
    outs = []
    for pws in (0, ws):
        gW, gU, gb = dev.empty((r.F, 4 * H)), dev.empty((H, 4 * H)), dev.empty((4 * H,))
        gW.upload(np.full((r.F, 4 * H), np.nan, f32))
        dev.call("mgr_memset", pg, 0xFF, pg.nbytes)
        dev.call("mgr_lstm_param_grads_dropout_ts", r.XS, LDT, m1[1], r.p, Hs, H, dZ, gW, gU, gb, B, T, r.F, H, 0, pg, pg.nbytes, 0, 0, pws, 0)
        outs.append(gW.download())
        for a in (gW, gU, gb):
            a.free()
    assert np.all(np.isfinite(outs[0])) and np.array_equal(outs[0], outs[1])
    r.still_cached(dW, W, ws, B, H, m1)
    for a in (dW, ws, Hs, dZ, pg):
        a.free()


@pytest.mark.parametrize("case", range(int(os.environ.get("MGR_FUZZ_PLANES", "6"))))
def test_random_plane_cache_sequences(device, case):
    """Seeded random sequences over 3 weights, 2 workspaces and a view into one of them, B in {2, 3}, two masks and none, streams 0
    and 1 (an event between them at every switch): promises made and withdrawn, projections, weights rewritten and declared again,
    workspaces memset, freed and allocated again.  Every projection bit for bit that of the uncached call."""
    dev = device
    rng = np.random.default_rng(8100 + case)
    F, H = int(rng.choice([128, 200, 333])), int(rng.choice([64, 100, 160]))
    r = Rig(dev, 8200 + case, F=F, Hmax=H, Bmax=3)
    view_off = 4096                                      # bytes
    wsb = r.ws_bytes()
    host = [r.weights() for _ in range(3)]
    dws = [dev.array(W) for W in host]
    frozen = [False] * 3
    wss = [dev.bytes(wsb + view_off), dev.bytes(wsb)]

    def space(i):
        return wss[0].view(view_off // 4, (wsb // 4,)) if i == 2 else wss[i]

    ops, cur = [], 0
    try:
        for step in range(40):
            x = rng.random()
            if x < 0.15:
                i, fz = int(rng.integers(3)), bool(rng.integers(2))
                ops.append(("declare", i, fz))
                dev.call("mgr_weight_planes_cache", dws[i], int(fz))
                frozen[i] = fz
            elif x < 0.25:
                i = int(rng.integers(3))
                ops.append(("rewrite", i))
                host[i] = r.weights()
                dws[i].upload(host[i])
                dev.call("mgr_weight_planes_cache", dws[i], int(frozen[i]))
            elif x < 0.32:
                i = int(rng.integers(2))
                ops.append(("memset", i))
                dev.call("mgr_memset", wss[i], 0xFF, wss[i].nbytes)
            elif x < 0.38:
                i = int(rng.integers(2))
                ops.append(("realloc", i))
                n = wss[i].size
                wss[i].free()
                wss[i] = dev.bytes(4 * n)
            else:
                s = int(rng.integers(2))
                if s != cur:
                    ops.append(("stream", s))
                    dev.record(7)
                    dev.stream(s)
                    dev.wait_event(s, 7)
                    cur = s
                i, w, B, mk = int(rng.integers(3)), int(rng.integers(3)), int(rng.choice([2, 3])), int(rng.integers(3))
                m = None if mk == 2 else r.mask(B, "ab"[mk])
                ops.append(("proj", i, w, B, mk))
                z = r.proj(dws[i], space(w), B, H, m)
                dev.stream(0)
                try:
                    r.check(z, host[i], B, H, m, "operations " + ", ".join(map(str, ops)))
                finally:
                    dev.stream(cur)
    finally:
        dev.sync()
        dev.stream(0)
        for a in dws + wss:
            a.free()
