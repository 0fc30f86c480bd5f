"""-m gpu: mgr_seq_zero_tail (csrc/seqlen.hip) against numpy, on bits.  Every buffer is pre-filled with a pattern that holds NaN and
Inf bit patterns - an element the kernel should have left alone, and one it multiplied by zero instead of storing zero, both
show - and sits between guard words that must come back unchanged, as must the ld - row floats between rows."""
import numpy as np
import pytest

from mgr_amd import _capi

pytestmark = pytest.mark.gpu

GUARD = 8
SPECIAL = np.array([0x7FC00001, 0x7F800000, 0xFF800000, 0xFFC12345, 0x80000000, 0x00000001, 0x3F800000, 0xDEADBEEF], np.uint32)


def pattern(n, salt):
    i = np.arange(n, dtype=np.uint64)
    p = ((i * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    p[::3] = SPECIAL[(np.arange(p[::3].size) + salt) % SPECIAL.size]
    p[p == 0] = 0xDEADBEEF       # (no element is zero before the call)
    return p


class Buf:
    """One [B, T, row] buffer with row stride ld, `off` floats into a 16-byte aligned allocation, guard words on both sides."""

    def __init__(self, device, B, T, row, ld, off, salt):
        self.B, self.T, self.row, self.ld, self.off = B, T, row, ld, off
        self.n = B * T * ld
        self.host = pattern(GUARD + off + self.n + GUARD, salt)
        self.dev = device.array(self.host)
        self.ptr = self.dev.ptr + 4 * (GUARD + off)

    def job(self):
        return (self.ptr, self.row, self.ld, self.B, self.T)

    def expect(self, lens):
        out = self.host.copy()
        body = out[GUARD + self.off:GUARD + self.off + self.n].reshape(self.B, self.T, self.ld)
        for b in range(self.B):
            body[b, min(max(int(lens[b]), 0), self.T):, :self.row] = 0
        return out


def run(device, bufs, lens):
    d_len = device.array(np.asarray(lens, np.int32))
    try:
        device.call("mgr_seq_zero_tail", len(bufs), _capi.make_seq_fill_jobs([b.job() for b in bufs]), d_len)
        return [b.dev.download() for b in bufs]
    finally:
        device.free(d_len)


def len_sets(B, T):
    edge = [0, 1, T - 1, T, T + 7, -3]
    return [[v] for v in edge] if B == 1 else [edge[:3], edge[3:]]


LAYOUTS = {"packed": (0, 0), "strided": (4, 0), "odd_stride": (3, 0), "unaligned": (0, 1)}      # (ld - row, base offset in floats)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("row", [4, 6, 400, 1200])
def test_tail_rows_are_zeroed_and_nothing_else_is_written(device, row, layout):
    gap, off = LAYOUTS[layout]
    vector_path = row % 4 == 0 and gap % 4 == 0 and off == 0
    assert vector_path == (layout in ("packed", "strided") and row != 6)
    for B in (1, 3):
        for T in (1, 5, 33):
            for lens in len_sets(B, T):
                buf = Buf(device, B, T, row, row + gap, off, salt=row + T)
                try:
                    assert (buf.ptr % 16 == 0) == (off == 0)
                    got, = run(device, [buf], lens)
                    ref = buf.expect(lens)
                    assert np.array_equal(got, ref), (B, T, lens, np.flatnonzero(got != ref)[:8])
                    assert np.array_equal(got[:GUARD + off], buf.host[:GUARD + off]) and np.array_equal(got[-GUARD:], buf.host[-GUARD:])
                    tail = sum(T - min(max(v, 0), T) for v in lens) * row
                    assert int((got == 0).sum()) == tail      # (zero BITS: not -0.0, not NaN)
                finally:
                    device.free(buf.dev)


def test_three_jobs_of_different_rows_in_one_call(device):
    B, T = 3, 33
    lens = [0, 17, 40]
    bufs = [Buf(device, B, T, 400, 400, 0, 1), Buf(device, B, T, 6, 9, 0, 2), Buf(device, B, 5, 1200, 1204, 1, 3)]
    try:
        for got, b in zip(run(device, bufs, lens), bufs):
            assert np.array_equal(got, b.expect(lens)), (b.row, b.T)
        assert bufs[2].T == 5      # (T differs between the jobs: the lengths are clipped per job)
    finally:
        device.free(*[b.dev for b in bufs])


def test_more_jobs_than_one_launch_takes(device):
    B, T = 2, 5
    lens = [2, 5]
    bufs = [Buf(device, B, T, 4 + 2 * j, 4 + 2 * j, 0, j) for j in range(19)]
    try:
        for got, b in zip(run(device, bufs, lens), bufs):
            assert np.array_equal(got, b.expect(lens)), b.row
    finally:
        device.free(*[b.dev for b in bufs])


def test_nothing_to_do_succeeds(device):
    buf = Buf(device, 3, 5, 8, 8, 0, 7)
    d_len = device.array(np.array([1, 2, 3], np.int32))
    try:
        device.call("mgr_seq_zero_tail", 0, None, None)
        device.call("mgr_seq_zero_tail", 0, _capi.make_seq_fill_jobs([buf.job()]), d_len)
        device.call("mgr_seq_zero_tail", 1, _capi.make_seq_fill_jobs([(buf.ptr, 8, 8, 0, 5)]), d_len)        # B == 0
        device.call("mgr_seq_zero_tail", 1, _capi.make_seq_fill_jobs([(buf.ptr, 8, 8, 3, 0)]), d_len)        # T == 0
        assert np.array_equal(buf.dev.download(), buf.host)
    finally:
        device.free(buf.dev, d_len)


@pytest.mark.parametrize("what", ["null_buffer", "null_lengths", "null_jobs", "row_zero", "row_negative", "ld_below_row", "other_B", "negative_njobs"])
def test_refusals_change_nothing(device, what):
    good = Buf(device, 3, 5, 8, 8, 0, 11)
    d_len = device.array(np.array([1, 2, 3], np.int32))
    bad = {"null_buffer": (0, 8, 8, 3, 5), "row_zero": (good.ptr, 0, 8, 3, 5), "row_negative": (good.ptr, -4, 8, 3, 5),
           "ld_below_row": (good.ptr, 8, 7, 3, 5), "other_B": (good.ptr, 8, 8, 2, 5)}
    try:
        with pytest.raises(_capi.MgrError):
            if what == "null_lengths":
                device.call("mgr_seq_zero_tail", 1, _capi.make_seq_fill_jobs([good.job()]), None)
            elif what == "null_jobs":
                device.call("mgr_seq_zero_tail", 1, None, d_len)
            elif what == "negative_njobs":
                device.call("mgr_seq_zero_tail", -1, _capi.make_seq_fill_jobs([good.job()]), d_len)
            else:
                # (the good job comes first: a refusal after it has been enqueued would show in its buffer)
                device.call("mgr_seq_zero_tail", 2, _capi.make_seq_fill_jobs([good.job(), bad[what]]), d_len)
        device.sync()
        assert np.array_equal(good.dev.download(), good.host)
        got, = run(device, [good], [1, 2, 3])       # (the context is still usable)
        assert np.array_equal(got, good.expect([1, 2, 3]))
    finally:
        device.free(good.dev, d_len)
