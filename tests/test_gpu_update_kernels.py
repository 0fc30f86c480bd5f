"""-m gpu: the update, RNG and small elementwise kernels of csrc/elementwise.hip against the restatements of tests/update_ref.py,
element by element, at the sizes where their grids, tails and branches change: a second and third grid-stride trip (the grids
are capped at 2048 x 256 threads), ragged tails, one row, one column, multiples of the 32-wide tiles and their neighbours.
Every bound is derived from float32 arithmetic (tests/update_ref.py: adam_bounds; the docstrings here), none is measured.
Each buffer a kernel writes has guard words on both sides, which must come back unchanged."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from oracle import keras_ref as kr
from tests import update_ref as ur

pytestmark = pytest.mark.gpu

U = ur.U
SEEDS = [0, 5, 2 ** 63 + 1]
GUARD = 64
PATTERN = {np.dtype(np.float32): np.float32(-12345.678), np.dtype(np.int32): np.int32(-0x5A5A5A5)}


class Guarded:
    """Device buffer [lo guard words | payload | hi guard words] and the view of the payload that a kernel is given."""

    def __init__(self, dev, host, lo=GUARD, hi=GUARD):
        host = np.ascontiguousarray(host)
        self.pat = PATTERN[host.dtype]
        self.lo, self.n, self.shape = lo, host.size, host.shape
        full = np.full(lo + host.size + hi, self.pat, host.dtype)
        full[lo:lo + host.size] = host.reshape(-1)
        self.buf = dev.array(full)
        self.view = self.buf.view(lo, (host.size,))
        self.ptr = self.view.ptr

    def read(self):
        """The payload, after checking that no guard word changed."""
        full = self.buf.download()
        assert np.all(full[:self.lo] == self.pat), "words in front of the buffer were written"
        assert np.all(full[self.lo + self.n:] == self.pat), "words behind the buffer were written"
        return full[self.lo:self.lo + self.n].reshape(self.shape)

    def free(self):
        self.buf.free()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound elementwise; reports the worst element as a multiple of its bound."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = err > bound
    if bad.any():
        i = int(np.argmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        raise AssertionError("%s: %d of %d elements beyond their bound; worst at %d: got %r, reference %r, error %.3e, bound %.3e"
                             % (what, int(bad.sum()), err.size, i, np.ravel(got)[i], np.ravel(ref)[i], np.ravel(err)[i], np.ravel(bound)[i]))


# ---------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------
ADAM_N = [1, 255, 256, 257, 524287, 524288, 524289, 1310723]      # 524288 = 2048 x 256 threads: one trip; the last: three, ragged
B1, B2, EPS = 0.9, 0.999, 1e-7
CLIP = np.float32(0.5)
GSCALES = [1.0, 0.5, 1.0 / 3.0]


def _ulp_neighbours(x):
    x = np.float32(x)
    return [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(0))]


def _adam_patch():
    """Gradients on, and one float32 ulp either side of, +-clip - as they are and as g gscale lands there for each gscale -, then
    0, 0, +-1e-20 (g g is subnormal), +-1e4 (far beyond the clip; 1e8 in v with clipping off)."""
    vals = []
    for gs in GSCALES:
        for x in _ulp_neighbours(CLIP / np.float32(gs)):
            vals += [x, -x]
    return np.array(vals + [0.0, 0.0, 1e-20, -1e-20, 1e4, -1e4], np.float32)


@functools.lru_cache(maxsize=1)
def _adam_data(n):
    rng = np.random.default_rng(1000 + n)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 2).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = (rng.random(n) * 0.1).astype(np.float32)
    patch = _adam_patch()
    # a stretch where m opposes g so that b1 m + (1 - b1) g cancels to rounding level (for the unclipped, unscaled g)
    s0, s1 = min(n, patch.size), min(n, patch.size + 40)
    m[s0:s1] = (-(1.0 - B1) / B1 * g[s0:s1].astype(np.float64) * (1 + 1e-6 * rng.standard_normal(s1 - s0))).astype(np.float32)
    exact = np.zeros(n, bool)
    starts = [0] + ([n - patch.size] if n >= 4 * patch.size else []) + ([524288 - 12] if n > 524288 + patch.size else [])
    for st in starts:                                    # at the head, at the ragged tail, across the end of the first trip
        k = min(n - st, patch.size)
        g[st:st + k] = patch[:k]
        zero = np.flatnonzero(patch[:k] == 0) + st
        v[zero] = 0                                      # 0 / (0 + eps): v carries zeros where g = 0 ...
        m[zero[:1]] = 0                                  # ... and at the first of them m too: nothing may move there
        exact[zero[:1]] = True
    for a in (p, g, m, v):
        a.setflags(write=False)
    return p, g, m, v, exact


@pytest.mark.parametrize("n,clip,gscale", list(itertools.product(ADAM_N, [0.5, 0.0], GSCALES)))
def test_adam_elementwise(device, n, clip, gscale):
    dev = device
    p, g, m, v, exact = _adam_data(n)
    lr_t = kr.adam_lr_t(1e-4, 1e-5, 7)
    pn, mn, vn, mags = ur.adam_ref(p, g, m, v, lr_t, B1, B2, EPS, clip, gscale)
    bp, bm, bv = ur.adam_bounds(mags)
    dp, dg, dm, dv = (Guarded(dev, a) for a in (p, g, m, v))
    try:
        dev.call("mgr_adam_step", dp.view, dg.view, dm.view, dv.view, n, lr_t, B1, B2, EPS, clip, gscale)
        P, G, M, V = dp.read(), dg.read(), dm.read(), dv.read()
    finally:
        for a in (dp, dg, dm, dv):
            a.free()
    assert np.array_equal(bits(G), bits(g))
    assert_within(M, mn, bm, "m")
    assert_within(V, vn, bv, "v")
    assert_within(P, pn, bp, "p")
    # g = 0 on m = v = 0: 0 / (0 + eps), nothing moves, to the bit
    assert exact.any() or n < 255
    assert np.array_equal(bits(P[exact]), bits(p[exact])) and np.array_equal(bits(M[exact]), bits(m[exact])) \
        and np.array_equal(bits(V[exact]), bits(v[exact]))
    # the bounds can see the step: on most elements they are below a twentieth of it
    assert n < 255 or np.mean(bp < 0.05 * np.abs(pn - p)) > 0.5


@pytest.mark.parametrize("n", [1003, 524289])
def test_adam_ten_steps(device, n):
    """Ten consecutive steps from m = v = 0 with fresh gradients and Keras' lr_t of each iteration; the MOVEMENT p_k - p_0 after
    every step against the float64 trajectory, per element within the sum of the per-step bounds (an error of m or v made in one
    step decays in the next ones, so the sum of what each step can add covers what is carried)."""
    dev = device
    rng = np.random.default_rng(n)
    p0 = rng.standard_normal(n).astype(np.float32)
    idle = np.arange(n) % 97 == 5                          # parameters that never see a gradient: they must never move
    dp, dm, dv = Guarded(dev, p0), Guarded(dev, np.zeros(n, np.float32)), Guarded(dev, np.zeros(n, np.float32))
    pr, mr, vr = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    sp, sm, sv = np.zeros(n), np.zeros(n), np.zeros(n)
    try:
        for k in range(10):
            g = (rng.standard_normal(n) * np.where(np.arange(n) % 2, 2.0, 1e-3)).astype(np.float32)
            g[idle] = 0
            lr_t = kr.adam_lr_t(1e-4, 1e-5, k)
            dg = Guarded(dev, g)
            dev.call("mgr_adam_step", dp.view, dg.view, dm.view, dv.view, n, lr_t, B1, B2, EPS, 0.5, 1.0)
            dg.free()
            pr, mr, vr, mags = ur.adam_ref(pr, g, mr, vr, lr_t, B1, B2, EPS, 0.5, 1.0)
            bp, bm, bv = ur.adam_bounds(mags)
            sp, sm, sv = sp + bp, sm + bm, sv + bv
            P = dp.read()
            assert_within(P.astype(np.float64) - p0, pr - p0, sp, "movement after step %d" % (k + 1))
            assert np.array_equal(bits(P[idle]), bits(p0[idle]))
        assert_within(dm.read(), mr, sm, "m after ten steps")
        assert_within(dv.read(), vr, sv, "v after ten steps")
        # ten steps of about lr each: the summed bound is still a small fraction of the movement
        assert np.median(sp[~idle] / np.abs(pr - p0)[~idle]) < 0.01
    finally:
        for a in (dp, dm, dv):
            a.free()


# ---------------------------------------------------------------------------------------------------------------------------
# max-norm
# ---------------------------------------------------------------------------------------------------------------------------
MAXV, MN_EPS = 3.0, 1e-7
MN_SHAPES = [(r, c) for r in (1, 31, 32, 33, 64, 1600) for c in (1, 31, 32, 33, 64, 400) if (r, c) != (1600, 400)]
SMALL, BELOW, ABOVE, BIG, ZERO, SINGLE = range(6)


def _maxnorm_matrix(rows, cols):
    """Columns, shuffled: norm 0.1 maxv; maxv (1 -+ 1e-7), i.e. the bound to within a float32 ulp from either side; 3 maxv; all
    zeros; one non-zero entry in the LAST row (2 maxv or 0.5 maxv).  Returns float32 W and each column's class."""
    rng = np.random.default_rng(rows * 1000 + cols)
    cls = rng.permutation((np.arange(cols) + rows + cols) % 6)
    W = rng.standard_normal((rows, cols))
    W /= np.sqrt((W * W).sum(0, keepdims=True))
    W *= np.choose(cls, [0.1 * MAXV, MAXV * (1 - 1e-7), MAXV * (1 + 1e-7), 3 * MAXV, 0.0, 0.0])
    W[:, (cls == ZERO) | (cls == SINGLE)] = 0.0                      # (+0, not the -0 of a negative entry times 0)
    single = np.flatnonzero(cls == SINGLE)
    W[-1, single] = np.where(single % 2, 2.0, -0.5) * MAXV
    return W.astype(np.float32), cls


def _check_maxnorm(W, out, cls):
    rows = W.shape[0]
    ref = ur.maxnorm_ref(W, MAXV, MN_EPS)
    assert np.isfinite(out).all()
    # against the reference: the float32 sum of squares is off by at most rows U relative if summed sequentially (the kernel's
    # 32-way split is within that), the root halves it; the sum with eps, the quotient and the product round once each
    assert_within(out, ref, (rows + 4) * U * np.abs(ref), "max-norm vs reference")
    nin, nout = np.sqrt((W.astype(np.float64) ** 2).sum(0)), np.sqrt((out.astype(np.float64) ** 2).sum(0))
    assert np.all(nout <= MAXV * (1 + 1e-6))
    # below the bound - what every real step takes - the column comes back at nrm / (eps + nrm) of itself: the exact shift
    # eps / (eps + nrm) (3.3e-7 at norm 0.3; Keras' formula makes it, so does the reference) and 2.5 U of rounding (the sum with
    # eps at most U, the quotient in [0.5, 1) at most U / 2, the product at most U)
    low = nin < 0.9 * MAXV
    shift = MN_EPS / (MN_EPS + np.where(low, nin, 1.0))
    assert_within(out[:, low], W[:, low].astype(np.float64) * (1 - shift[low]), 2.5 * U * np.abs(W[:, low]), "columns below the bound")
    assert set(cls[low]) <= {SMALL, ZERO, SINGLE} and np.all(low[cls == SMALL])
    # at and above it the norm comes back as the bound
    clipped = (cls == BELOW) | (cls == ABOVE) | (cls == BIG) | ((cls == SINGLE) & (nin > MAXV))
    assert np.all(np.abs(nout[clipped] - MAXV) <= 1e-6 * MAXV)
    # 0 / eps: zero columns stay zero, to the bit
    assert not bits(out[:, cls == ZERO]).any()
    # a lone entry in the last row is found (a reduction that drops the tail rows leaves it unclipped)
    hi = (cls == SINGLE) & (nin > MAXV)
    assert np.all(np.abs(np.abs(out[-1, hi]) - MAXV) <= 1e-6 * MAXV)


@pytest.mark.parametrize("rows,cols", MN_SHAPES)
def test_maxnorm_cols(device, rows, cols):
    W, cls = _maxnorm_matrix(rows, cols)
    d = Guarded(device, W)
    try:
        device.call("mgr_maxnorm_cols", d.view, rows, cols, MAXV, MN_EPS)
        out = d.read()
    finally:
        d.free()
    _check_maxnorm(W, out, cls)


@pytest.mark.parametrize("rows,cols", [(33, 33), (24, 16), (1600, 64)])
def test_maxnorm_on_a_view_at_an_odd_offset(device, rows, cols):
    """As Engine.apply_gradients calls it: on a kernel's segment somewhere inside the flat parameter buffer."""
    W, cls = _maxnorm_matrix(rows, cols)
    d = Guarded(device, W, lo=3, hi=5)
    try:
        device.call("mgr_maxnorm_cols", d.view, rows, cols, MAXV, MN_EPS)
        out = d.read()
    finally:
        d.free()
    _check_maxnorm(W, out, cls)


# ---------------------------------------------------------------------------------------------------------------------------
# Gaussian noise
# ---------------------------------------------------------------------------------------------------------------------------
NOISE_N = [1, 2, 3, 511, 512, 513, 1048577, 2097155]     # pairs: 1048576 = 2 x (2048 x 256) fill one trip; the last takes three


@pytest.mark.parametrize("n,seed", list(itertools.product(NOISE_N, SEEDS)))
def test_noise_elementwise(device, n, seed):
    """|Y - ref| <= 1e-5 stddev + 2^-23 |Y|: the radius is at most 5.77 stddev, the float32 angle 2 pi u2 is off by at most
    7.5e-7, logf, sqrtf and sincosf add a few ulp - together about 4.5e-6 stddev, doubled; the sum X + noise rounds once."""
    dev = device
    sd = 0.5
    X = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    ref = ur.noise_ref(X, n, sd, seed)
    dx = dev.array(X)
    dy, dy0, dip = Guarded(dev, np.zeros(n, np.float32)), Guarded(dev, np.zeros(n, np.float32)), Guarded(dev, X)
    try:
        dev.call("mgr_add_gaussian_noise", dx, dy.view, n, sd, seed)
        Y = dy.read()                                     # (the guard behind Y[n - 1]: an odd n must not write its pair's second half)
        assert_within(Y, ref, 1e-5 * sd + 2.0 ** -23 * np.abs(Y), "noise")
        assert n <= 3 or np.mean(Y != X) > 0.999          # (the noise is there: the reference holds X + noise, the buffer held 0)
        dev.call("mgr_add_gaussian_noise", dx, dy.view, n, sd, seed)
        assert np.array_equal(bits(dy.read()), bits(Y))   # stateless: the same call, the same bits
        dev.call("mgr_add_gaussian_noise", dip.view, dip.view, n, sd, seed)
        assert np.array_equal(bits(dip.read()), bits(Y))  # in place
        dev.call("mgr_add_gaussian_noise", dx, dy0.view, n, 0.0, seed)
        assert np.array_equal(bits(dy0.read()), bits(X))  # stddev 0: X, bit for bit
        assert np.array_equal(bits(dx.download()), bits(X))
        if n > 3:
            dev.call("mgr_add_gaussian_noise", dx, dy.view, n, sd, seed + 1)
            assert np.mean(dy.read() != Y) > 0.99         # another seed, another stream
    finally:
        for a in (dx, dy, dy0, dip):
            a.free()


# ---------------------------------------------------------------------------------------------------------------------------
# dropout mask
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", list(itertools.product([1, 257, 524289], SEEDS)))
def test_dropout_mask_bit_exact(device, n, seed):
    idx = np.arange(n, dtype=np.uint64)
    for p in (0.0, 0.1, 0.5, 0.9):
        d = Guarded(device, np.full(n, 7.0, np.float32))
        try:
            device.call("mgr_dropout_mask", d.view, n, p, seed)
            got = d.read()
        finally:
            d.free()
        assert np.array_equal(bits(got), bits(ur.drop_scale(seed, idx, p))), p


def test_dropout_mask_refuses_bad_rates(device):
    dev = device
    d = Guarded(dev, np.full(100, 7.0, np.float32))
    try:
        for p in (1.0, -0.25, 1.5):
            assert dev.lib.mgr_dropout_mask(dev.ctx, d.ptr, 100, p, 3) != 0
            assert b"dropout rate" in dev.lib.mgr_last_error()
        assert np.all(d.read() == 7.0)
    finally:
        d.free()


# ---------------------------------------------------------------------------------------------------------------------------
# small kernels: all exact
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", list(itertools.product([1, 31, 32, 33, 100], [1, 31, 32, 33, 257])))
def test_transpose(device, rows, cols):
    src = np.random.default_rng(rows * 300 + cols).standard_normal((rows, cols)).astype(np.float32)
    ds, dd = device.array(src), Guarded(device, np.zeros((cols, rows), np.float32))
    try:
        device.call("mgr_transpose", ds, dd.view, rows, cols)
        assert np.array_equal(bits(dd.read()), bits(np.ascontiguousarray(src.T)))
    finally:
        ds.free()
        dd.free()


@pytest.mark.parametrize("rows,H", list(itertools.product([1, 5, 1600], [1, 8, 100, 500])))
def test_lstm_pack_both_directions(device, rows, H):
    """packed[:, u * 4 + g] = keras[:, g * H + u], each direction on its own input against the index formula (a round trip
    would let a wrong pack cancel against its inverse)."""
    rng = np.random.default_rng(rows + H)
    c = np.arange(4 * H)
    for to_keras in (0, 1):
        src = rng.standard_normal((rows, 4 * H)).astype(np.float32)
        if to_keras:
            g, u = c // H, c % H                          # destination column g * H + u  <-  packed column u * 4 + g
            want = src[:, u * 4 + g]
        else:
            u, g = c // 4, c % 4                          # destination column u * 4 + g  <-  keras column g * H + u
            want = src[:, g * H + u]
        ds, dd = device.array(src), Guarded(device, np.zeros((rows, 4 * H), np.float32))
        try:
            device.call("mgr_lstm_pack", ds, dd.view, rows, H, to_keras)
            assert np.array_equal(bits(dd.read()), bits(np.ascontiguousarray(want))), to_keras
        finally:
            ds.free()
            dd.free()


ADD2D_SHAPES = [(7, 5), (33, 200), (1900, 64)]


def _strided(rng, rows, ld):
    return rng.standard_normal((rows, ld)).astype(np.float32)


@pytest.mark.parametrize("rows,cols", ADD2D_SHAPES)
def test_add2d_three_strides(device, rows, cols):
    rng = np.random.default_rng(rows)
    lda, ldb, ldo = cols + 3, cols + 8, cols + 1
    A, Bm, O = _strided(rng, rows, lda), _strided(rng, rows, ldb), _strided(rng, rows, ldo)
    da, db, do = device.array(A), device.array(Bm), Guarded(device, O)
    try:
        device.call("mgr_add2d", da, lda, db, ldb, do.view, ldo, rows, cols)
        want = O.copy()
        want[:, :cols] = A[:, :cols] + Bm[:, :cols]       # (the padding columns of Out keep what they held)
        assert np.array_equal(bits(do.read()), bits(want))
    finally:
        for a in (da, db, do):
            a.free()


@pytest.mark.parametrize("rows,cols", ADD2D_SHAPES)
def test_add2d_in_place(device, rows, cols):
    """Out == A with another stride for B: the residual add of the backward pass (dY1 += its slice of the wider dout)."""
    rng = np.random.default_rng(rows + 1)
    lda, ldb = cols + 2, 3 * cols + 5
    A, Bm = _strided(rng, rows, lda), _strided(rng, rows, ldb)
    off = cols + 1                                        # B starts at a column offset inside its rows, like dout's slice
    da, db = Guarded(device, A), device.array(Bm)
    try:
        device.call("mgr_add2d", da.view, lda, db.view(off, (1,)), ldb, da.view, lda, rows, cols)
        want = A.copy()
        want[:, :cols] = A[:, :cols] + Bm[:, off:off + cols]
        assert np.array_equal(bits(da.read()), bits(want))
        assert np.array_equal(bits(db.download()), bits(Bm))
    finally:
        da.free()
        db.free()


@pytest.mark.parametrize("rows,cols", ADD2D_SHAPES)
def test_add2d_into_a_column_window(device, rows, cols):
    """Contiguous A and B summed into a column window of a wider zeroed buffer: the residual add into the concatenated features."""
    rng = np.random.default_rng(rows + 2)
    A, Bm = _strided(rng, rows, cols), _strided(rng, rows, cols)
    wide, off = 2 * cols + 7, cols + 3
    da, db, do = device.array(A), device.array(Bm), Guarded(device, np.zeros((rows, wide), np.float32))
    try:
        device.call("mgr_add2d", da, cols, db, cols, do.buf.view(do.lo + off, (1,)), wide, rows, cols)
        want = np.zeros((rows, wide), np.float32)
        want[:, off:off + cols] = A + Bm
        assert np.array_equal(bits(do.read()), bits(want))
    finally:
        for a in (da, db, do):
            a.free()


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1900, 100003])
def test_mean(device, n):
    """Values of 1e-3 beside values of 1e4: the result is the float64 mean rounded to float32, to within one float32 ulp - which
    a float32 accumulator misses by far."""
    rng = np.random.default_rng(n)
    x = (np.where(rng.random(n) < 0.5, 1e-3, 1e4) * (1 + 0.1 * rng.random(n))).astype(np.float32)
    x[0] = 1e4
    want = np.float32(np.mean(x.astype(np.float64)))
    dx, do = device.array(x), Guarded(device, np.zeros(1, np.float32))
    try:
        device.call("mgr_mean", dx, n, do.view)
        got = do.read()[0]
    finally:
        dx.free()
        do.free()
    assert abs(float(got) - float(want)) <= float(np.spacing(want)), (got, want)
    if n == 100003:   # the data can tell: a sequential float32 sum of it is off by many ulp
        assert abs(float(np.add.accumulate(x, dtype=np.float32)[-1] / np.float32(n)) - float(want)) > 16 * float(np.spacing(want))


def _argmax(dev, P, skip):
    B, T, Cn = P.shape
    dP = dev.array(P)
    best, prob = Guarded(dev, np.zeros((B, T - skip), np.int32)), Guarded(dev, np.zeros((B, T - skip), np.float32))
    try:
        dev.call("mgr_frame_argmax", dP, B, T, Cn, skip, best.view, prob.view)
        return best.read(), prob.read()
    finally:
        for a in (dP, best, prob):
            a.free()


@pytest.mark.parametrize("B,T,Cn,skip", [(3, 17, 22, 0), (3, 17, 22, 16), (2, 9, 1, 0), (2, 9, 1, 8), (5, 6, 2, 3),
                                         (3, 174764, 3, 1)])           # the last: 3 x 174763 = 524289 frames, a second trip
def test_frame_argmax(device, B, T, Cn, skip):
    rng = np.random.default_rng(T + Cn)
    P = rng.random((B, T, Cn)).astype(np.float32)
    t = T - 1                                            # a frame that every skip here keeps
    P[0, t, :] = 0.25                                    # all equal: index 0
    if B > 1:
        P[1, t, :] = 0.1
        P[1, t, 0] = P[1, t, -1] = 0.9                   # first and last class tie: the first wins
    if B > 2:
        P[2, t, :] = 0.1
        P[2, t, -1] = 0.9                                # the maximum in the last class
    best, prob = _argmax(device, P, skip)
    assert best.shape == (B, T - skip)
    assert np.array_equal(best, P[:, skip:].argmax(-1)) and np.array_equal(bits(prob), bits(np.ascontiguousarray(P[:, skip:].max(-1))))
    assert best[0, -1] == 0 and (B < 2 or best[1, -1] == 0) and (B < 3 or best[2, -1] == Cn - 1)
