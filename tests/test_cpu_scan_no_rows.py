"""Host side of "a scan job may omit its row-major output" (mgr_scan_job.Y == NULL with a YT, include/mgr.h).  A kernel that stores
through a NULL row pointer faults the device; what keeps such a launch from being enqueued is the launcher's checks of the job
list, and they are plain host code: they run, and are tested, without a GPU (the job list is checked before the context is looked
at).  The pointers below are never dereferenced."""
import ctypes as C

import pytest

from mgr_amd import _capi

FAKE = 0x10000      # a 16-byte aligned address nobody reads


def _job(H=100, B=17, T=9, **kw):
    j = dict(Z=FAKE, Up=FAKE, Y=FAKE, ldy=H, B=B, T=T, H=H, reverse=0, YT=FAKE, ytb=H * 128, ldt=128, yt_split=0)
    j.update(kw)
    return j


def _call(lib, jobs):
    arr = _capi.make_scan_jobs(jobs)
    opts = _capi.make_launch_opts(_capi.SCAN_FORM_AUTO, 0)
    rc = lib.mgr_lstm_scan_fwd_multi_ex(None, len(jobs), arr, None, 0, C.byref(opts))
    return rc, lib.mgr_last_error().decode()


def test_a_job_without_rows_and_without_a_transposed_copy_is_refused():
    lib = _capi.load_library()
    rc, msg = _call(lib, [_job(), _job(Y=0, ldy=0, YT=0, ytb=0, ldt=0)])
    assert rc != 0 and "job 1" in msg and "neither Y nor YT" in msg
    # the same through the entry points that forward to it, and through the exact workspace query (0 = refused)
    arr = _capi.make_scan_jobs([_job(Y=0, YT=0, ytb=0, ldt=0)])
    assert lib.mgr_lstm_scan_fwd_multi(None, 1, arr, None, 0) != 0 and "neither Y nor YT" in lib.mgr_last_error().decode()
    assert lib.mgr_lstm_scan_fwd_multi_ws_bytes(None, 1, arr, None) == 0
    assert lib.mgr_lstm_scan_fwd(None, FAKE, FAKE, None, 100, None, 0, None, None, 17, 9, 100, 0, None, 0) != 0
    assert "neither Y nor YT" in lib.mgr_last_error().decode()


@pytest.mark.parametrize("H", [100, 64, 30])
def test_a_job_without_rows_passes_the_job_checks_whatever_kernel_it_will_take(H):
    """Y == NULL with a YT is a legal job for every kernel family (K-split widths skip the store, the others get scratch): the call
    gets as far as the context, which a box without a GPU does not have - and ldy is not looked at."""
    lib = _capi.load_library()
    rc, msg = _call(lib, [_job(H=H, Y=0, ldy=0, ytb=H * 128)])
    assert rc != 0 and msg == "null context"
    rc, msg = _call(lib, [_job(H=H, ldy=H - 1, ytb=H * 128)])      # (with rows the row stride is still checked)
    assert rc != 0 and "bad shape" in msg


def test_workspace_query_counts_row_scratch_only_for_jobs_without_rows():
    """mgr_lstm_scan_multi_ws_bytes needs no context: with Y it says what it always said (header + exchange images), without Y it adds
    B T H floats per such job, rounded up to 256 bytes - an upper bound; mgr_lstm_scan_fwd_multi_ws_bytes is the exact figure."""
    lib = _capi.load_library()
    B, T = 17, 9

    def query(jobs):
        return lib.mgr_lstm_scan_multi_ws_bytes(len(jobs), _capi.make_scan_jobs(jobs))

    def images(H):     # lstm.hip job_ws: two exchange images per 16-sample group, 1 KiB per 16 units in whole K-blocks of 32
        return ((B + 15) // 16 * 2 * ((H // 4 + 7) // 8) * 512 * 4 + 255) // 256 * 256

    def scratch(H):
        return (B * T * H * 4 + 255) // 256 * 256

    hdr = query([_job(H=100)]) - images(100)
    assert hdr > 0 and hdr % 256 == 0
    for hs in ((100,), (500, 300), (64, 100, 100)):
        with_rows = [_job(H=H, B=B, T=T, ytb=H * 128) for H in hs]
        assert query(with_rows) == hdr + sum(images(H) for H in hs)
        assert query([dict(j, YT=0, ytb=0, ldt=0) for j in with_rows]) == query(with_rows)
        none = [dict(j, Y=0, ldy=0) for j in with_rows]
        assert query(none) == query(with_rows) + sum(scratch(H) for H in hs)
        mixed = [with_rows[0]] + none[1:]
        assert query(mixed) == query(with_rows) + sum(scratch(H) for H in hs[1:])


def test_struct_sizes_and_revision_are_what_they_were():
    """No member was added for this: the sizes the library reports are those of the binding's structs, the revision stays 7."""
    lib = _capi.load_library()
    sizes = (C.c_uint * 4)()
    assert lib.mgr_abi_struct_sizes(sizes) == 0
    assert tuple(sizes) == (C.sizeof(_capi.ScanJob), C.sizeof(_capi.ScanBwdJob), C.sizeof(_capi.ScanLaunchOpts), _capi.ABI_REVISION)
    assert tuple(sizes) == (96, 80, 16, 7)
