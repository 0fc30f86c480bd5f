"""Plain numpy restatements of the update, RNG and noise kernels of csrc/elementwise.hip (test infrastructure, NOT product code).

The generator of csrc/common.h is stateless - one splitmix64 finaliser of (seed, element index) - so it is restated here bit for
bit on np.uint64 arrays; the dropout decision stays in float32 like the kernel's, the Box-Muller transform and the Adam
arithmetic are float64.  tests/test_cpu_update_ref.py checks these restatements (against the oracle, and the generator's
statistics); tests/test_gpu_update_kernels.py then only has to show that the kernels equal them."""
import numpy as np

from oracle import keras_ref as kr

U64 = np.uint64
_GOLDEN, _M1, _M2 = U64(0x9E3779B97F4A7C15), U64(0xBF58476D1CE4E5B9), U64(0x94D049BB133111EB)
_SEED_MUL = U64(0xD1342543DE82EF95)
_INV24 = np.float32(1.0 / 16777216.0)
U = 2.0 ** -24          # float32 unit roundoff (half an ulp, relative)
TINY = 2.0 ** -149      # float32 subnormal spacing


def mix64(z):
    """mgr_mix64: the splitmix64 finaliser, modulo 2^64, on an array of np.uint64."""
    z = np.asarray(z, U64)
    with np.errstate(over="ignore"):
        z = z + _GOLDEN
        z = (z ^ (z >> U64(30))) * _M1
        z = (z ^ (z >> U64(27))) * _M2
        return z ^ (z >> U64(31))


def _stream(seed, idx):
    with np.errstate(over="ignore"):
        return mix64(np.asarray([int(seed) & (2 ** 64 - 1)], U64) * _SEED_MUL + np.asarray(idx, U64))


def rand_u32(seed, idx):
    """mgr_rand_u32: the top 32 bits of the mix of seed * K + idx."""
    return (_stream(seed, idx) >> U64(32)).astype(np.uint32)


def inv_keep(p):
    """What mgr_dropout_mask hands its kernel: 1.0f / (1.0f - p), every operation in float32."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def drop_scale(seed, idx, p):
    """mgr_drop_scale: float32 uniform in [0, 1) from the top 24 bits, kept (u >= p) elements scaled by 1 / (1 - p)."""
    u = (rand_u32(seed, idx) >> np.uint32(8)).astype(np.float32) * _INV24      # (exact: 24 bits times a power of two)
    return np.where(u >= np.float32(p), inv_keep(p), np.float32(0.0)).astype(np.float32)


def noise_uniforms(n, seed):
    """The two 24-bit uniforms k_add_noise takes per PAIR of elements, exact in float32: u1 in (0, 1], u2 in [0, 1)."""
    r = _stream(seed, np.arange((n + 1) // 2, dtype=U64))
    u1 = ((r >> U64(40)).astype(np.float32) + np.float32(1.0)) * _INV24
    u2 = ((r >> U64(8)) & U64(0xFFFFFF)).astype(np.float32) * _INV24
    return u1, u2


def noise_ref(X, n, stddev, seed):
    """X + Gaussian noise as k_add_noise draws it: element 2i takes the cosine, 2i+1 the sine half of pair i's Box-Muller
    transform, here in float64 from the same uniforms.  The radius is at most sqrt(2 ln 2^24) ~ 5.77 stddev (u1 >= 2^-24)."""
    u1, u2 = noise_uniforms(n, seed)
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * float(np.float32(stddev))
    ang = 2.0 * np.pi * u2.astype(np.float64)
    z = np.empty(2 * u1.size, np.float64)
    z[0::2] = rad * np.cos(ang)
    z[1::2] = rad * np.sin(ang)
    return np.asarray(X, np.float64).reshape(-1)[:n] + z[:n]


def adam_ref(p, g, m, v, lr_t, b1=0.9, b2=0.999, eps=1e-7, clip=0.5, gscale=1.0, round_scalars=True):
    """One k_adam step in float64.  The C ABI takes its scalars as float, so each is first rounded to float32 (1 - 0.999f is not
    0.001): that is the kernel's contract.  Returns the new (p, m, v) and a dict of per-element magnitudes for error bounds:
      "m": |b1 m| + |(1 - b1) g|          the sum of the magnitudes of m's terms (g scaled and clipped),
      "v": |b2 v| + |(1 - b2) g g|        the same for v,
      "p": |p|                            the parameter before the step,
      "step": lr_t "m" / (sqrt(v) + eps)  the step with m's term magnitudes in place of m: |step| where m's terms do not
                                          cancel, and what a relative error of m's terms can move the step by where they do."""
    if round_scalars:
        lr_t, b1, b2, eps, clip, gscale = (float(np.float32(s)) for s in (lr_t, b1, b2, eps, clip, gscale))
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    g = g * gscale
    if clip > 0:
        g = np.clip(g, -clip, clip)
    mn = b1 * m + (1.0 - b1) * g
    vn = b2 * v + (1.0 - b2) * g * g
    den = np.sqrt(vn) + eps
    pn = p - lr_t * mn / den
    m_mag = np.abs(b1 * m) + np.abs((1.0 - b1) * g)
    mags = {"m": m_mag, "v": np.abs(b2 * v) + np.abs((1.0 - b2) * g * g), "p": np.abs(p), "step": lr_t * m_mag / den}
    return pn, mn, vn, mags


def adam_bounds(mags):
    """Largest float32-vs-float64 distance of one k_adam step from adam_ref, per element, for (p, m, v).
    m: the product g gscale, the product of each term and the sum are at most 4 roundings of at most U relative to the terms'
    magnitudes (3 with the FMA the compiler contracts the sum into); (1 - b) is exact in float32 for b in [0.5, 1].
    v: g gscale enters twice (2 U, none for gscale = 1 or 0.5), two more products and the sum: 4 U with the FMA, and 5 U only
    if all five roundings of an uncontracted sum were extreme with one sign.  A result below the normal range is also off by
    up to the subnormal spacing (g = 1e-20 squares to 1e-40).
    p: the final subtraction rounds by U |p_new| <= U (|p| + step); the step carries m's 4 U, half of v's 4 U through the
    root, and a rounding each of sqrtf, the sum with eps, the product with lr_t and the (correctly rounded) quotient: 10 U."""
    return U * mags["p"] + 16 * U * mags["step"], 4 * U * mags["m"] + TINY, 4 * U * mags["v"] + TINY


def maxnorm_ref(W, maxv=3.0, eps=1e-7, round_scalars=True):
    """oracle.keras_ref.maxnorm_cols in float64 on a copy (maxv and eps rounded to float32 like the C ABI's arguments)."""
    if round_scalars:
        maxv, eps = float(np.float32(maxv)), float(np.float32(eps))
    out = np.array(W, np.float64)
    kr.maxnorm_cols(out, maxv, eps)
    return out
