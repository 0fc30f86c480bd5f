"""Input builders of the CNN front-end edge tests (tests/test_gpu_conv_edges.py runs them through mgr_conv_pool_fwd / _bwd_data /
_bwd_weights, tests/test_cpu_conv_cases.py checks their premises with the fp64 reference alone).  A case is a namespace: name, N, Hin,
Win, Cin, ks, Cout, `branch` - the weight-gradient kernel csrc/conv.hip picks for it -, `constant` (constant frames: every window
ties or is a ReLU zero), `why` and the arrays x (N, Hin, Win, Cin), W (ks, ks, Cin, Cout), b (Cout,), dY (N, Hp, Wp, Cout), all
float32 and read-only.  case(name) and reference(name) build once per process.

csrc/conv.hip stages one frame per workgroup in LDS (at most 64 KiB), walks the frames with a grid of at most 8192 workgroups,
sums the weight gradient over at most 256 frame chunks, and picks the weight-gradient kernel from K = ks * ks * Cin, Cout and
nE = K * Cout + Cout: the implicit GEMM on the f32 MFMA when K and Cout are multiples of 16, else the vector form with two
elements per thread for nE <= 1024 and eight above.  The shapes below sit on those boundaries."""
import functools
import types
import zlib

import numpy as np

from tests import rgb_ref

MAX_LDS = 64 * 1024       # kMaxLds: the frame (forward, weight gradient) or the pooled gradient and its codes (data gradient) in LDS
GRID_CAP = 8192           # frame_grid
CHUNKS = 256              # kChunks
VECTOR_SMALL = 1024       # nE up to which the vector weight gradient takes two elements per thread
TILES_PER_GROUP = 16      # 16x16 output tiles per workgroup of the MFMA weight gradient (4 waves x kTpw)

BRANCHES = ("mfma<4>", "mfma<5>", "partial<4,2>", "partial<4,8>", "partial<5,2>", "partial<5,8>")

# (name, N, Hin, Win, Cin, ks, Cout, branch, what it reaches)
_TABLE = (
    ("colour-13x10", 40, 13, 10, 3, 5, 16, "partial<5,8>", "colour frames (K = 75), Hin > Win, odd conv rows only (Ho = 9, Wo = 6)"),
    ("over-1024", 40, 10, 13, 1, 5, 40, "partial<5,8>", "nE = 1040: just over the two / eight element boundary, Hin < Win"),
    ("under-1024", 40, 10, 13, 1, 5, 36, "partial<5,2>", "nE = 936: just under it"),
    ("tiny-ks4", 40, 9, 12, 1, 4, 4, "partial<4,2>", "nE = 68, a dropped conv column only (Ho = 6, Wo = 9)"),
    ("vector-ks4-k128", 40, 9, 12, 8, 4, 12, "partial<4,8>", "K = 128 but Cout = 12: the eight-element form at ks = 4"),
    ("mfma4-straddle", 40, 9, 12, 3, 4, 16, "mfma<4>", "Cin = 3: every 16-row tile straddles filter taps; ntiles = 3, most waves own nothing"),
    ("mfma5-11x8", 40, 11, 8, 16, 5, 16, "mfma<5>", "Hin > Win, odd conv rows only (Ho = 7, Wo = 4)"),
    ("mfma4-cout256", 24, 7, 6, 1, 4, 256, "mfma<4>", "Cout = 256: the last width one pass of the block over the bias covers"),
    ("mfma4-cout272", 24, 7, 6, 1, 4, 272, "mfma<4>", "Cout = 272 > the 256 threads of the block: db[256:] needs a second pass"),
    ("stride-vector", 8200, 6, 7, 1, 5, 4, "partial<5,2>", "N > 8192: grid-stride over frames; 33 frames per chunk, one short chunk, empty chunks"),
    ("stride-mfma", 8200, 5, 6, 1, 4, 16, "mfma<4>", "the same on the MFMA form"),
    ("smallest-ks5", 1, 6, 6, 1, 5, 4, "partial<5,2>", "the smallest legal input, one frame: Hp = Wp = 1"),
    ("smallest-ks4", 1, 5, 5, 2, 4, 16, "mfma<4>", "the same at ks = 4 on the MFMA form (Cin = 2: tiles straddle taps)"),
    ("chunks-255", 255, 6, 7, 2, 5, 8, "partial<5,2>", "one frame per chunk, 255 chunks"),
    ("chunks-256", 256, 6, 7, 2, 5, 8, "partial<5,2>", "one frame per chunk, every chunk used"),
    ("chunks-257", 257, 6, 7, 2, 5, 8, "partial<5,2>", "two frames per chunk: 128 full chunks, one half-full, 127 empty"),
    ("lds-limit", 1, 128, 128, 1, 5, 4, "partial<5,2>", "a frame of exactly 64 KiB in LDS"),
)
# constant frames of one non-square vector and one non-square MFMA case: ties and ReLU zeros routed at Hp != Wp
_CONSTANT_OF = {"colour-13x10-constant": "colour-13x10", "mfma5-11x8-constant": "mfma5-11x8"}

RANDOM_NAMES = tuple(r[0] for r in _TABLE)
ALL_NAMES = RANDOM_NAMES + tuple(_CONSTANT_OF)
OFFSET_CASE = "colour-13x10"       # the case that also runs with X, dY, Y, dX one float and code one byte into their allocations


def dims(Hin, Win, Cin, ks, Cout):
    """The sizes csrc/conv.hip derives from a layer's shape."""
    Ho, Wo = Hin - ks + 1, Win - ks + 1
    K = ks * ks * Cin
    return types.SimpleNamespace(Ho=Ho, Wo=Wo, Hp=Ho // 2, Wp=Wo // 2, K=K, nE=K * Cout + Cout,
                                 ntiles=(K // 16) * (Cout // 16) if K % 16 == 0 and Cout % 16 == 0 else 0,
                                 frame_bytes=Hin * Win * Cin * 4, pooled_bytes=(Ho // 2) * (Wo // 2) * Cout * 5)


def branch_of(Cin, ks, Cout):
    """The weight-gradient kernel mgr_conv_pool_bwd_weights launches."""
    K = ks * ks * Cin
    if K % 16 == 0 and Cout % 16 == 0:
        return "mfma<%d>" % ks
    return "partial<%d,%d>" % (ks, 2 if K * Cout + Cout <= VECTOR_SMALL else 8)


def chunking(N):
    """(chunks launched, frames per chunk, chunks that hold a frame, frames in the last of those)"""
    nchunk = min(N, CHUNKS)
    per = -(-N // nchunk)
    used = -(-N // per)
    return nchunk, per, used, N - (used - 1) * per


def make_inputs(rng, N, Hin, Win, Cin, ks, Cout, constant=False):
    """x uniform in [0, 1) ([-0.5, 1) for Cin = 1: some ReLU zeros), W uniform +-0.05, b uniform +-0.02, dY standard normal - the
    distributions of the reference-layer test (tests/test_gpu_rgb.py)."""
    if constant:
        x = np.repeat(rng.uniform(0, 1, (N, 1, 1, Cin)), Hin, 1).repeat(Win, 2).astype(np.float32)
    else:
        x = rng.uniform(0 if Cin > 1 else -0.5, 1, (N, Hin, Win, Cin)).astype(np.float32)
    W = rng.uniform(-0.05, 0.05, (ks, ks, Cin, Cout)).astype(np.float32)
    b = rng.uniform(-0.02, 0.02, Cout).astype(np.float32)
    dY = rng.standard_normal((N, (Hin - ks + 1) // 2, (Win - ks + 1) // 2, Cout)).astype(np.float32)
    return x, W, b, dY


@functools.lru_cache(maxsize=None)
def case(name):
    constant = name in _CONSTANT_OF
    row = next(r for r in _TABLE if r[0] == _CONSTANT_OF.get(name, name))
    _, N, Hin, Win, Cin, ks, Cout, branch, why = row
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)      # seeded per case
    x, W, b, dY = make_inputs(rng, N, Hin, Win, Cin, ks, Cout, constant)
    for a in (x, W, b, dY):
        a.flags.writeable = False
    return types.SimpleNamespace(name=name, N=N, Hin=Hin, Win=Win, Cin=Cin, ks=ks, Cout=Cout, branch=branch, constant=constant,
                                 why=why, x=x, W=W, b=b, dY=dY)


def routing_premise(pre):
    """(fp64 routing codes, clear, dead) of pre-activation windows (N, Hp, Wp, Cout, 4).  clear: the two largest ReLU values of the
    window are further apart than f32 rounding (1e-5 of the largest |pre|), so an f32 forward must route like fp64; dead: every
    value is a ReLU zero by that margin, so it must route nothing."""
    rcode, gap = rgb_ref.reference_code(pre)
    tol = 1e-5 * np.abs(pre).max()
    return rcode, gap > tol, pre.max(-1) < -tol


@functools.lru_cache(maxsize=None)
def reference(name):
    """fp64, read-only: (pooled output Y (N, Hp, Wp, Cout), pre-activation windows (N, Hp, Wp, Cout, 4))"""
    c = case(name)
    pre = rgb_ref.conv_windows(c.x, c.W, c.b)
    Y = np.maximum(pre, 0.0).max(-1)
    pre.flags.writeable = False
    Y.flags.writeable = False
    return Y, pre
