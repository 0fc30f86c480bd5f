"""One CNN front-end layer through the C ABI (mgr_conv_pool_fwd, _bwd_data, _bwd_weights of csrc/conv.hip), shared by
tests/test_gpu_rgb.py and tests/test_gpu_conv_edges.py.  Every output sits between guard words that must come back unchanged, over
a poison that no result can equal - an element the kernels did not write shows -, and the weight-gradient workspace is filled with
0xFF bytes before each call: a partial sum nobody wrote reads as NaN, not as whatever the allocator left."""
import numpy as np

GUARD_BYTES = 32                       # on either side of a body; a multiple of 16, so a body without offset stays 16-byte aligned
POISON = {4: 0x7FC0DEAD, 1: 0x5A}      # by item size: a NaN with a payload no arithmetic produces; a byte that is no routing code


def _guard(n, salt):
    i = np.arange(n, dtype=np.uint64)
    return ((i * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503) + np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


class Guarded:
    """n float32 (item = 4) or uint8 (item = 1) elements, `off` elements into a 16-byte aligned allocation, guards on both sides
    (the `off` elements count as guard).  host: the bits uploaded."""

    def __init__(self, device, n, item=4, off=0, salt=0, fill=None):
        self.device, self.n, self.item = device, int(n), item
        bits = np.uint32 if item == 4 else np.uint8
        self.lead = GUARD_BYTES // item + off
        tail = GUARD_BYTES // item
        host = np.full(self.lead + self.n + tail, POISON[item], bits)
        host[:self.lead] = _guard(self.lead, salt).astype(bits)
        host[self.lead + self.n:] = _guard(tail, salt + 1).astype(bits)
        if fill is not None:       # an input: its values instead of the poison
            host[self.lead:self.lead + self.n] = np.ascontiguousarray(fill).reshape(-1).view(bits)
        self.host = host
        self.dev = device.array(host)
        self.ptr = self.dev.ptr + item * self.lead

    def bits(self):
        return self.dev.download()

    def body(self, what):
        """The body after a call that must have written all of it: guards intact, no element left as it was."""
        got = self.bits()
        lo, hi = self.lead, self.lead + self.n
        assert np.array_equal(got[:lo], self.host[:lo]) and np.array_equal(got[hi:], self.host[hi:]), "%s: a guard word was written" % what
        out = got[lo:hi]
        left = np.flatnonzero(out == POISON[self.item])
        assert left.size == 0, "%s: %d of %d elements never written, the first at %s" % (what, left.size, self.n, left[:8])
        return out.view(np.float32) if self.item == 4 else out

    def untouched(self):
        return np.array_equal(self.bits(), self.host)

    def free(self):
        self.device.free(self.dev)


def fill_workspace(device, ws):
    device.call("mgr_memset", ws, 0xFF, ws.nbytes)      # (f64 NaNs)


def run_layer(device, x, W, b, dY, ks, off=0, data_gradient=True):
    """Forward, data gradient, weight gradient and the weight gradient a second time.  Returns (Y (N, Hp, Wp, Cout), dX like x, dW like
    W, db, code flat uint8, the second launch's dW).  off = 1 passes X, dY, Y and dX one float and code one byte into their
    allocations (W of the forward alone has an alignment contract).  data_gradient = False leaves the data gradient out (dX None)."""
    N, Hin, Win, Cin = x.shape
    Cout = W.shape[-1]
    Hp, Wp = (Hin - ks + 1) // 2, (Win - ks + 1) // 2
    npool = N * Hp * Wp * Cout
    X = Guarded(device, x.size, off=off, salt=1, fill=x)
    G = Guarded(device, npool, off=off, salt=2, fill=dY)
    dW_, db_ = device.array(W.reshape(-1)), device.array(b)
    Y = Guarded(device, npool, off=off, salt=3)
    code = Guarded(device, npool, item=1, off=off, salt=4)
    dX = Guarded(device, x.size, off=off, salt=5)
    gW, gb, rW, rb = (Guarded(device, n, salt=6 + i) for i, n in enumerate((W.size, b.size, W.size, b.size)))
    ws = device.bytes(device.lib.mgr_conv_pool_bwd_weights_ws_bytes(N, Hin, Win, Cin, ks, Cout))
    try:
        assert dW_.ptr % 16 == 0 and (X.ptr % 16 == 0) == (off == 0)
        device.call("mgr_conv_pool_fwd", X.ptr, N, Hin, Win, Cin, dW_, db_, ks, Cout, Y.ptr, code.ptr)
        if data_gradient:
            device.call("mgr_conv_pool_bwd_data", G.ptr, code.ptr, dW_, N, Hin, Win, Cin, ks, Cout, dX.ptr)
        for w_out, b_out in ((gW, gb), (rW, rb)):
            fill_workspace(device, ws)
            device.call("mgr_conv_pool_bwd_weights", X.ptr, G.ptr, code.ptr, N, Hin, Win, Cin, ks, Cout, w_out.ptr, b_out.ptr, ws, ws.nbytes)
        assert X.untouched() and G.untouched(), "an input was written"
        out = (Y.body("Y").reshape(N, Hp, Wp, Cout), dX.body("dX").reshape(x.shape) if data_gradient else None,
               gW.body("dW").reshape(W.shape), gb.body("db"), code.body("code"), rW.body("dW again").reshape(W.shape))
        assert np.array_equal(out[3].view(np.uint32), rb.body("db again").view(np.uint32))     # the bias gradient is deterministic too
        return out
    finally:
        for g in (X, G, Y, code, dX, gW, gb, rW, rb):
            g.free()
        device.free(dW_, db_, ws)
