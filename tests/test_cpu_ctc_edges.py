"""The premises of the CTC edge cases (tests/ctc_cases.py), checked with the fp64 oracle alone: what tests/test_gpu_ctc_edges.py
assumes about its inputs holds before any kernel runs."""
import numpy as np
import pytest

from tests import ctc_cases as cc


@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_only_the_designated_samples_have_an_infinite_reference_loss(name):
    c = cc.case(name)
    loss, dz = cc.reference(name)
    assert not np.isnan(loss).any() and not np.isneginf(loss).any()
    assert tuple(np.nonzero(np.isposinf(loss))[0]) == tuple(sorted(cc.case("e-clipped" if name == "e-raw" else name).inf)) == tuple(sorted(c.inf))
    assert (loss[np.isfinite(loss)] > 0).all()
    if name != "f-logzero":                       # (log 0: only the loss is specified)
        assert np.isfinite(dz).all()
        for b in range(len(loss)):
            assert dz[b].any() == bool(np.isfinite(loss[b]))
    live = np.asarray(c.labels)[np.arange(c.labels.shape[1])[None, :] < np.clip(c.ll, 0, None)[:, None]]
    if name != "e-raw":
        assert (live >= 0).all() and (live < c.P.shape[2]).all() and (live != c.blank).all()
    if c.eps == 0.0 and name != "f-logzero":
        assert (c.P > 0).all() and (c.P >= np.finfo(np.float32).tiny).all()


@pytest.mark.parametrize("name", cc.B_NAMES)
def test_closed_forms_equal_the_oracle(name):
    """one alignment: loss = - sum_t log y_t(path_t); and its path collapses to the labels in exactly the frames it has"""
    c = cc.case(name)
    loss, _ = cc.reference(name)
    assert abs(loss[0] - c.closed[0]) <= 1e-12 * abs(c.closed[0]), (loss[0], c.closed[0])
    form, L = name.split("-")[1], int(c.ll[0])
    path = cc.closed_form_path(form, L, c.blank, c.labels[0, :L])
    assert len(path) == c.il[0] and np.array_equal(cc.collapse(path, c.blank), c.labels[0, :L])
    assert c.il[1] == c.il[0] - 1 and np.array_equal(c.P[1], c.P[0]) and np.array_equal(c.labels[1], c.labels[0])
    # form (i) never may skip, form (ii) always: every lane boundary is crossed by the one transition the form is about
    lab = c.labels[0, :L]
    assert (lab[1:] == lab[:-1]).all() if form == "i" else (lab[1:] != lab[:-1]).all()


def test_closed_form_cases_cover_the_lane_boundaries():
    got = {(n.split("-")[1], int(cc.case(n).ll[0])) for n in cc.B_NAMES if "Lmax" not in n}
    assert got == {(f, L) for f in ("i", "ii") for L in (63, 64, 65, 127, 128, 129, 191, 192, 193, 255)}
    for n in cc.B_NAMES:
        c = cc.case(n)
        assert (c.labels.shape[1] > c.ll[0]) == ("Lmax" in n)
    assert sum("Lmax" in n for n in cc.B_NAMES) == 2


@pytest.mark.parametrize("Lmax", cc.A_LMAX)
def test_width_cases_map_to_the_intended_pairs_per_lane(Lmax):
    c = cc.case("a-Lmax%d" % Lmax)
    ppl = cc.ppl_of(c.labels.shape[1])
    assert c.labels.shape[1] == Lmax and ppl == cc.A_PPL[Lmax]
    assert len(c.il) % 2 == 1                                     # the last two-sample workgroup holds one sample
    ll = set(int(v) for v in c.ll)
    assert {Lmax, Lmax - 1, 1} <= ll and ll & {33, 65, 129, 193}
    T, skip = c.P.shape[1], c.skip
    assert T <= 2 * Lmax + 74 and {T - skip, T - skip - 1} <= set(int(v) for v in c.il) and c.il[1] == 2 * c.ll[1] + 3
    # can_skip is false at the FIRST pair of a lane (p = lane * ppl, p >= 1) in sample 0 or sample 4, and true at others
    first = np.arange(1, (Lmax - 1) // ppl + 1) * ppl
    rep = [(c.labels[b, first] == c.labels[b, first - 1]) for b in (0, 4)]
    assert (rep[0] | rep[1]).sum() >= len(first) // 2 and not (rep[0] & rep[1]).all()
    assert (c.labels[0, 1:Lmax:2] == c.labels[0, 0:Lmax - 1:2]).all()


def test_pairs_per_lane_of_every_case():
    """all four widths of k_ctc_chains are launched, and 63 / 255 fill the 64 lanes exactly"""
    assert {cc.ppl_of(cc.case(n).labels.shape[1]) for n in cc.ALL_NAMES} == {1, 2, 3, 4}
    assert (63 + 1) == 64 * cc.ppl_of(63) and (255 + 1) == 64 * cc.ppl_of(255)
    assert [cc.ppl_of(n) for n in (63, 64, 127, 128, 191, 192, 255)] == [1, 2, 2, 3, 3, 4, 4]


def test_length_sweeps_contain_every_class_of_length():
    c = cc.case("c-sweep")
    tps = set(int(v) for v in c.il)
    assert len(c.il) == 47 and tps == set(range(1, 41)) | {255, 256, 257, 258, 511, 512, 513}
    assert {t % 16 for t in tps} == set(range(16)) and {t % 8 for t in tps} == set(range(8)) and {t % 2 for t in tps} == {0, 1}
    assert {1, 2} <= tps and max(tps) == c.P.shape[1] - c.skip
    assert any(t <= 256 for t in tps if t > 200) and any(t > 256 for t in tps)
    assert (2 * c.ll - 1 <= c.il).all() and set(int(v) for v in c.ll) == {1, 2, 3}
    # lengths differ inside the two-sample workgroups
    assert (c.il[0:46:2] != c.il[1:46:2]).all()
    c3 = cc.case("c-sweep-ppl3")
    assert cc.ppl_of(c3.labels.shape[1]) == 3 and sorted(int(v) for v in c3.il) == list(range(1, 21)) and (c3.ll == 2).all()
    assert (c3.labels[:, 0] != c3.labels[:, 1]).all()


@pytest.mark.parametrize("s", [12, 25])
def test_peaked_alignments_are_valid(s):
    c = cc.case("g-peaked%d" % s)
    paths = cc.peaked_alignments(s)
    for b, path in enumerate(paths):
        L = int(c.ll[b])
        assert len(path) == c.il[b]
        assert np.array_equal(cc.collapse(path, c.blank), c.labels[b, :L])
        # the raised class is the frame's most probable one by far
        rows = c.P[b, c.skip + np.arange(len(path))]
        assert (rows.argmax(-1) == path).all() and rows[np.arange(len(path)), path].min() > 0.5
    loss, dz = cc.reference(c.name)
    assert (loss < 1.0).all()                     # (nats over ~135 frames: the raised alignment carries nearly all the mass)


def test_argument_cases_vary_what_they_say():
    base = cc.case("d-base")
    assert (base.skip, base.blank, base.eps) == (2, base.P.shape[2] - 1, 1e-8)
    assert [cc.case(n).skip for n in ("d-skip0", "d-skip1", "d-skip5")] == [0, 1, 5]
    assert [cc.case(n).blank for n in ("d-blank0", "d-blankmid")] == [0, base.P.shape[2] // 2]
    assert [cc.case(n).eps for n in ("d-eps0", "d-eps1e-3")] == [0.0, 1e-3]
    raw, cl = cc.case("e-raw"), cc.case("e-clipped")
    T, Lmax, Cn = raw.P.shape[1], raw.labels.shape[1], raw.P.shape[2]
    assert (raw.il > T - raw.skip).any() and (raw.il < 0).any() and (raw.il == 0).any()
    assert (raw.ll > Lmax).any() and (raw.ll < 0).any() and (raw.labels >= Cn).any() and (raw.labels[0] < 0).any()
    assert np.array_equal(cl.il, np.clip(raw.il, 0, T - raw.skip)) and np.array_equal(cl.ll, np.clip(raw.ll, 0, Lmax))
    f = cc.case("f-logzero")
    assert f.eps == 0.0 and (f.P[0, :, 2] == 0).all() and (f.P[1, 10:26, 4] == 0).all() and (f.P[2, 10:26, 2] == 0).all()
    assert 4 not in f.labels and 2 in f.labels


def test_drift_case_loads_the_renormalisation():
    """every lattice class loses 85 ... 115 log2 units in every frame, the garbage class holds the mass and is in no label
    sequence; the saturated case's float32 error is far below its loss"""
    c = cc.case("h-drift")
    Cn = c.P.shape[2]
    lattice = np.delete(c.P, Cn - 2, axis=2)
    assert c.eps == 0.0 and c.blank == Cn - 1 and (Cn - 2) not in c.labels
    assert (np.log2(lattice) < -85).all() and (np.log2(lattice) > -115).all() and (c.P[:, :, Cn - 2] > 0.999).all()
    assert 16 * 85 > 1024 and 64 * 85 > 4096          # float32 ulp 1.2e-4 at 16 steps, 4.9e-4 at 64
    s = cc.case("g-peaked25")
    ref, _ = cc.reference(s.name)
    l32, _ = cc.oracle(s, np.float32)
    assert (4 * np.abs(l32 - ref) < 0.05 * ref).all(), (l32, ref)
