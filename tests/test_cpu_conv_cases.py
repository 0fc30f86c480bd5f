"""The premises of the CNN front-end edge cases (tests/conv_cases.py), checked with the fp64 reference alone: every case lands on the
branch of csrc/conv.hip it is named for, the table covers every weight-gradient instantiation and every shape edge, and the
routing of all but a sliver of the pooling windows is decided beyond f32 rounding - what tests/test_gpu_conv_edges.py assumes
about its inputs holds before any kernel runs."""
import numpy as np
import pytest

from tests import conv_cases as cc
from tests import rgb_ref

# name -> the figures that put it where its row says (checked against the formulas of csrc/conv.hip below)
FIGURES = {
    "colour-13x10": dict(K=75, nE=1216, Ho=9, Wo=6),
    "over-1024": dict(K=25, nE=1040),
    "under-1024": dict(K=25, nE=936),
    "tiny-ks4": dict(K=16, nE=68, Ho=6, Wo=9),
    "vector-ks4-k128": dict(K=128, nE=1548),
    "mfma4-straddle": dict(K=48, ntiles=3),
    "mfma5-11x8": dict(K=400, ntiles=25, Ho=7, Wo=4),
    "mfma4-cout256": dict(K=16, ntiles=16),
    "mfma4-cout272": dict(K=16, ntiles=17),
    "stride-vector": dict(nE=104, Hp=1, Wp=1),
    "stride-mfma": dict(K=16, ntiles=1, Hp=1, Wp=1),
    "smallest-ks5": dict(Ho=2, Wo=2, Hp=1, Wp=1),
    "smallest-ks4": dict(Ho=2, Wo=2, Hp=1, Wp=1, K=32, ntiles=2),
    "lds-limit": dict(frame_bytes=65536),
}
# name -> (chunks launched, frames per chunk, chunks that hold a frame, frames in the last of those)
CHUNKING = {"stride-vector": (256, 33, 249, 16), "stride-mfma": (256, 33, 249, 16), "chunks-255": (255, 1, 255, 1),
            "chunks-256": (256, 1, 256, 1), "chunks-257": (256, 2, 129, 1), "smallest-ks5": (1, 1, 1, 1)}


@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_case_lands_on_its_named_branch(name):
    c = cc.case(name)
    d = cc.dims(c.Hin, c.Win, c.Cin, c.ks, c.Cout)
    assert c.branch in cc.BRANCHES and cc.branch_of(c.Cin, c.ks, c.Cout) == c.branch
    gemm = d.K % 16 == 0 and c.Cout % 16 == 0
    assert c.branch.startswith("mfma") == gemm and c.branch[c.branch.index("<") + 1] == str(c.ks)
    if not gemm:
        assert c.branch.endswith(",2>") == (d.nE <= 1024)
    for k, v in FIGURES.get(name, {}).items():
        assert getattr(d, k) == v, (k, getattr(d, k), v)
    if name in CHUNKING:
        assert cc.chunking(c.N) == CHUNKING[name]
    # what every entry point accepts
    assert c.N > 0 and c.Cout % 4 == 0 and c.ks in (4, 5) and min(c.Hin, c.Win) >= c.ks + 1 and d.frame_bytes <= cc.MAX_LDS
    assert c.x.shape == (c.N, c.Hin, c.Win, c.Cin) and c.W.shape == (c.ks, c.ks, c.Cin, c.Cout) and c.b.shape == (c.Cout,)
    assert c.dY.shape == (c.N, d.Hp, d.Wp, c.Cout) and all(a.dtype == np.float32 for a in (c.x, c.W, c.b, c.dY))
    # the data gradient stages the pooled gradient and its codes: only the 128 x 128 frame's does not fit (62 x 62 x 4 x 5 bytes)
    assert (d.pooled_bytes > cc.MAX_LDS) == (name == "lds-limit")


def test_table_covers_every_weight_gradient_instantiation_and_shape_edge():
    cases = [cc.case(n) for n in cc.ALL_NAMES]
    assert {c.branch for c in cases} == set(cc.BRANCHES)
    ds = [(c, cc.dims(c.Hin, c.Win, c.Cin, c.ks, c.Cout)) for c in cases]
    assert any(c.Hin > c.Win for c in cases) and any(c.Hin < c.Win for c in cases)
    assert any(d.Ho % 2 == 1 and d.Wo % 2 == 0 for _, d in ds) and any(d.Ho % 2 == 0 and d.Wo % 2 == 1 for _, d in ds)
    assert any(d.Ho % 2 == 1 and c.ks == 5 for c, d in ds) and any(d.Wo % 2 == 1 and c.ks == 4 for c, d in ds)
    # the two-element / eight-element boundary from both sides, as near as Cout % 4 == 0 allows at K = 25 (26 elements per channel)
    nE = sorted(d.nE for c, d in ds if not c.branch.startswith("mfma"))
    assert max(v for v in nE if v <= 1024) + 4 * 26 > 1024 >= min(v for v in nE if v > 1024) - 4 * 26
    # frames beyond the grid cap on both weight-gradient families, chunk counts around 256, one frame alone
    for fam in ("mfma", "partial"):
        assert any(c.N > cc.GRID_CAP and c.branch.startswith(fam) for c in cases)
        assert any(c.N == 1 and c.branch.startswith(fam) for c in cases)
    assert {255, 256, 257} <= {c.N for c in cases}
    # MFMA tiles: fewer than one workgroup's 16, exactly 16, more (a second tile group), and rows that straddle filter taps
    nt = {d.ntiles for c, d in ds if c.branch.startswith("mfma")}
    assert min(nt) < cc.TILES_PER_GROUP and cc.TILES_PER_GROUP in nt and max(nt) > cc.TILES_PER_GROUP
    assert any(c.branch.startswith("mfma") and 16 % c.Cin != 0 for c in cases)            # (Cin = 3: k / Cin, k % Cin in full)
    assert any(c.branch.startswith("mfma") and c.Cout > 256 for c in cases) and any(c.Cout == 256 for c in cases)
    assert any(d.frame_bytes == cc.MAX_LDS for _, d in ds)
    # constant frames at Hp != Wp on both families
    for fam in ("mfma", "partial"):
        assert any(c.constant and c.branch.startswith(fam) and d.Hp != d.Wp for c, d in ds)
    assert cc.OFFSET_CASE in cc.RANDOM_NAMES


def test_cases_are_seeded_per_case_and_read_only():
    seen = {}
    for n in cc.ALL_NAMES:
        c = cc.case(n)
        assert not any(a.flags.writeable for a in (c.x, c.W, c.b, c.dY))
        assert cc.case(n) is c
        seen.setdefault(c.W.tobytes()[:64], []).append(n)
    assert all(len(v) == 1 for v in seen.values()), seen
    for n in cc.RANDOM_NAMES:
        c = cc.case(n)
        lo = -0.5 if c.Cin == 1 else 0.0
        assert lo <= c.x.min() and c.x.max() < 1 and np.abs(c.W).max() <= 0.05 and np.abs(c.b).max() <= 0.02
        assert (c.x.min() < 0) == (c.Cin == 1)


@pytest.mark.parametrize("name", cc.RANDOM_NAMES)
def test_routing_is_decided_beyond_f32_rounding(name):
    """Clearly routed (the two largest ReLU values of the window apart by more than 1e-5 of the largest |pre|) or dead (every
    pre-activation below minus that): more than 0.99 of the windows, the cap the GPU test may leave unchecked."""
    c = cc.case(name)
    Y, pre = cc.reference(name)
    rcode, clear, dead = cc.routing_premise(pre)
    share = float((clear | dead).mean())
    print("%s: clear or dead %.5f (dead %.4f) of %d windows" % (name, share, float(dead.mean()), clear.size))
    assert share > 0.99, share
    assert not (clear & dead).any()
    assert set(np.unique(rcode)) <= {0, 1, 2, 3, 255} and (rcode[dead] == 255).all() and (rcode[clear] != 255).all()


@pytest.mark.parametrize("name", sorted(cc._CONSTANT_OF))
def test_constant_frames_tie_or_die(name):
    c = cc.case(name)
    _, pre = cc.reference(name)
    assert (c.x == c.x[:, :1, :1, :]).all()
    assert np.abs(pre - pre[..., :1]).max() <= 1e-12 * np.abs(pre).max()             # the four values of a window are one value
    live = pre[..., 0] > 1e-5 * np.abs(pre).max()
    assert live.any() and (~live).any()                                              # both ties and ReLU zeros occur


@pytest.mark.parametrize("name", ["colour-13x10", "mfma4-straddle", "tiny-ks4"])
def test_windows_agree_with_the_autograd_reference(name):
    """conv_windows is the forward of conv_layer / conv_layer_routed: same pooled output, same windows."""
    c = cc.case(name)
    Y, pre = cc.reference(name)
    assert np.array_equal(Y, rgb_ref.conv_layer(c.x, c.W, c.b, c.dY)[0])
    rcode = rgb_ref.reference_code(pre)[0]
    assert np.array_equal(pre, rgb_ref.conv_layer_routed(c.x, c.W, c.b, c.dY, rcode.astype(np.uint8))[0])
