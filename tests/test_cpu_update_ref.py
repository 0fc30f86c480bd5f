"""The restatements of tests/update_ref.py against the oracle, and the design of the device generator (csrc/common.h) through
them: keep rates and scales of the dropout decision, moments and correlations of the Box-Muller noise.  The GPU tests
(tests/test_gpu_update_kernels.py) prove the kernels EQUAL these restatements; what the restatements are worth is checked here."""
import math

import numpy as np
import pytest

from oracle import keras_ref as kr
from tests import update_cases as uc
from tests import update_ref as ur

SEEDS = [0, 5, 2 ** 63 + 1]
N = 1 << 22


def test_mix64_is_splitmix64():
    """The first outputs of splitmix64 seeded with 0 (the published test vector of the generator): state k * golden, finalised."""
    golden = 0x9E3779B97F4A7C15
    got = ur.mix64(np.array([(k * golden) % 2 ** 64 for k in range(3)], np.uint64))
    assert [int(x) for x in got] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    # and in plain Python integers, for a few awkward states
    def plain(z):
        z = (z + golden) % 2 ** 64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
        return z ^ (z >> 31)
    zs = [0, 1, 2 ** 63, 2 ** 64 - 1, 0xD1342543DE82EF95, 12345678901234567890]
    assert [int(x) for x in ur.mix64(np.array(zs, np.uint64))] == [plain(z) for z in zs]
    assert [int(x) for x in ur.rand_u32(2 ** 63 + 1, np.array([7], np.uint64))] == \
        [plain(((2 ** 63 + 1) * 0xD1342543DE82EF95 + 7) % 2 ** 64) >> 32]


def test_adam_ref_equals_oracle():
    rng = np.random.default_rng(1)
    n = 501
    p, g = rng.standard_normal(n), rng.standard_normal(n) * 2
    m, v = rng.standard_normal(n) * 0.1, rng.random(n) * 0.1
    for clip, gscale in ((0.5, 1.0), (0.0, 0.5), (0.5, 1.0 / 3.0)):
        lr_t = kr.adam_lr_t(1e-4, 1e-5, 3)
        pr, mr, vr = p.copy(), m.copy(), v.copy()
        kr.adam_step(pr, g, mr, vr, lr_t, 0.9, 0.999, 1e-7, clip, gscale)
        pn, mn, vn, mags = ur.adam_ref(p, g, m, v, lr_t, 0.9, 0.999, 1e-7, clip, gscale, round_scalars=False)
        assert np.array_equal(pn, pr) and np.array_equal(mn, mr) and np.array_equal(vn, vr)
        assert np.all(mags["m"] >= np.abs(mn)) and np.all(mags["v"] >= vn * (1 - 1e-15)) and np.all(mags["step"] >= np.abs(pn - p) * (1 - 1e-9))
        # the float32-rounded scalars are the kernel's contract: they move the result by 1e-5 of the step, not more
        pn32, mn32, vn32, _ = ur.adam_ref(p, g, m, v, lr_t, 0.9, 0.999, 1e-7, clip, gscale)
        assert 0 < np.abs(vn32 - vn).max() <= 2e-5 * np.abs(vn).max()
        assert np.abs((pn32 - p) - (pn - p)).max() <= 2e-5 * np.abs(pn - p).max()


def test_maxnorm_ref_equals_oracle():
    rng = np.random.default_rng(2)
    W = rng.standard_normal((37, 45)) * np.where(np.arange(45) % 2, 1.2, 0.05)     # columns above and below the bound
    W[:, 7] = 0
    Wr = W.copy()
    kr.maxnorm_cols(Wr, 3.0)
    assert np.array_equal(ur.maxnorm_ref(W, 3.0, round_scalars=False), Wr)
    n = np.sqrt((Wr * Wr).sum(0))
    assert n.max() <= 3.0 and n.min() == 0 and (n < 1).any() and np.isfinite(Wr).all()
    assert np.abs(ur.maxnorm_ref(W, 3.0) - Wr).max() <= 1e-14


@pytest.mark.parametrize("seed", SEEDS)
def test_dropout_keep_rate_and_scale(seed):
    idx = np.arange(N, dtype=np.uint64)
    m0 = ur.drop_scale(seed, idx, 0.0)
    assert m0.dtype == np.float32 and np.all(m0 == 1.0)                       # p = 0 keeps everything, unscaled
    for p in (0.1, 0.5, 0.9):
        m = ur.drop_scale(seed, idx, p)
        kept = m != 0
        # the rate reaches the C ABI as a float: the scale is the correctly rounded 1 / (1 - float32(p)), 9.999998 at p = 0.9f =
        # 0.89999998, which makes keep rate x scale = 1; forming it in float32 like mgr_dropout_mask rounds to the same
        assert np.all(m[kept] == np.float32(1.0 / (1.0 - float(np.float32(p))))), p
        # the decision is u >= float32(p) on a 24-bit uniform: P(keep) = 1 - ceil(p 2^24) / 2^24
        q = 1.0 - math.ceil(float(np.float32(p)) * 2 ** 24) / 2 ** 24
        assert abs(int(kept.sum()) - N * q) <= 5 * math.sqrt(N * q * (1 - q)), (p, kept.mean())
    # another seed is another mask
    assert (ur.drop_scale(seed, idx[:4096], 0.5) != ur.drop_scale(seed + 1, idx[:4096], 0.5)).mean() > 0.4


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("seed", SEEDS)
def test_noise_statistics(seed):
    """Moments of n = 2^22 noise samples at X = 0 against a normal sample's analytic standard errors:
    mean sigma / sqrt(n), variance sigma^2 sqrt(2 / n), skewness sqrt(6 / n), excess kurtosis sqrt(24 / n); a correlation
    coefficient of k independent pairs has standard error 1 / sqrt(k).  Every bound is 5 standard errors."""
    sd = 0.5
    z = ur.noise_ref(np.zeros(N), N, sd, seed)
    assert z.shape == (N,) and z.dtype == np.float64
    mu, var = z.mean(), z.var()
    c = (z - mu) / math.sqrt(var)
    assert abs(mu) <= 5 * sd / math.sqrt(N)
    assert abs(var - sd * sd) <= 5 * sd * sd * math.sqrt(2.0 / N)
    assert abs((c ** 3).mean()) <= 5 * math.sqrt(6.0 / N)
    assert abs((c ** 4).mean() - 3.0) <= 5 * math.sqrt(24.0 / N)
    # the cosine and sine halves of a pair, neighbours of the same half, and another seed's stream
    assert abs(_corr(z[0::2], z[1::2])) <= 5 / math.sqrt(N // 2)
    assert abs(_corr(z[:-2], z[2:])) <= 5 / math.sqrt(N - 2)
    other = ur.noise_ref(np.zeros(N), N, sd, SEEDS[(SEEDS.index(seed) + 1) % 3])
    assert abs(_corr(z, other)) <= 5 / math.sqrt(N)
    # each half alone has the moments too (a transform that wrote the cosine twice would pass the pooled test)
    for half in (z[0::2], z[1::2]):
        assert abs(half.mean()) <= 5 * sd / math.sqrt(N // 2) and abs(half.var() - sd * sd) <= 5 * sd * sd * math.sqrt(2.0 / (N // 2))
    assert abs(_corr(np.abs(z[0::2]), np.abs(z[1::2]))) <= 5 / math.sqrt(N // 2)     # (independent, not merely uncorrelated in sign)
    # tail cut: u1 >= 2^-24 bounds the radius, so no sample lies beyond sqrt(2 ln 2^24) = 5.768 sigma (a true normal sample of
    # this size has none beyond it either with probability 0.97); nothing degenerate on the way there
    assert np.abs(z).max() / sd <= math.sqrt(2 * math.log(2.0 ** 24)) and np.abs(z).max() / sd > 4.5


def test_noise_ref_adds_x_and_handles_odd_n():
    rng = np.random.default_rng(3)
    X = rng.standard_normal(11)
    full = ur.noise_ref(np.zeros(12), 12, 0.5, 5)
    for n in (1, 2, 3, 11):
        y = ur.noise_ref(X, n, 0.5, 5)
        assert y.shape == (n,) and np.array_equal(y, X[:n] + full[:n])
    assert np.array_equal(ur.noise_ref(X, 11, 0.0, 5), X)
    u1, u2 = ur.noise_uniforms(N, 0)
    assert u1.dtype == np.float32 and u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1


@pytest.mark.parametrize("make", [lambda: uc.golden_case("fusion_tiny"), lambda: uc.golden_case("unimodal_tiny"), uc.fusion_bite_case,
                                  uc.unimodal_layer_bound_case], ids=["fusion_tiny", "unimodal_tiny", "fusion_bite", "unimodal_layer_bound"])
def test_movement_error_model(make):
    """What the movement assertion of tests/test_gpu_network.py lets through and what it catches, from the oracle alone: the
    numpy float32 trainer (the error model the tolerances of tests/update_cases.py were measured on) passes it, an update
    scaled by 0.8 - and no update at all - fails it for every weight kind."""
    c = make()
    w0, wf, losses, norms = uc.run_trainer(c, np.float64)
    if c["wfinal"] is not None:                       # the golden end state IS this float64 run
        assert all(np.array_equal(wf[k], c["wfinal"][k]) for k in wf)
    s0, sf, _, _ = uc.run_trainer(c, np.float32)
    assert all(v.dtype == np.float32 for v in sf.values())
    worst = uc.assert_movement(c["name"], c["spec"], sf, s0, wf, w0)
    assert set(worst) == set(uc.MOVE_MEASURED[c["name"]])
    for kind in worst:                                # far below the 0.2 of an update wrong by 20 %
        assert uc.move_tol(c["name"], kind) < 0.2 / 40, kind
    for scale in (0.8, 0.0):
        bad = {k: w0[k] + scale * (wf[k] - w0[k]) for k in wf}
        errs = uc.movement_errors(c["spec"], bad, w0, wf, w0)
        for kind, (e, _) in errs.items():
            assert abs(e - (1 - scale)) < 1e-9 and e > uc.move_tol(c["name"], kind), (kind, e)
        with pytest.raises(AssertionError):
            uc.assert_movement(c["name"], c["spec"], bad, w0, wf, w0)
    # the bounds bite where the case says so
    if c["name"] == "fusion_bite":
        for n in uc.kernel_names(c["spec"]):
            start = uc.col_norms(w0[n])
            assert (start > 0.25).sum() > (start < 0.25).sum() > 0
            assert all(step[n].max() <= 0.25 * (1 + 1e-12) for step in norms) and (norms[-1][n] < 0.2).any()
    if c["name"] == "unimodal_layer_bound":
        for n in uc.kernel_names(c["spec"]):
            free = "/l0/" in n
            assert (uc.col_norms(w0[n]) > 0.2).any()
            assert (norms[-1][n].max() > 0.3) if free else (norms[-1][n].max() <= 0.2 * (1 + 1e-12))
