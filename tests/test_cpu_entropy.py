"""The fp64 restatement of the alignment entropy (tests/entropy_ref.py) against the definition - every alignment enumerated -
and against central differences of its own H through both softmaxes; the invariants it rests on; and the ascent step's size, fixed
here for tests/test_gpu_entropy.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as ar  # noqa: E402
import entropy_ref as en  # noqa: E402

#        name              labels     C  blank  T'  eps   zero class
CASES = [("two-labels",    [0, 1],    3, 2,     6,  1e-8, None),
         ("repeated",      [0, 0],    3, 2,     6,  1e-8, None),
         ("three-of-four", [0, 2, 2], 4, 3,     6,  1e-8, None),
         ("one-label",     [1],       3, 2,     6,  1e-8, None),
         ("no-label",      [],        3, 2,     6,  1e-8, None),
         ("blank-first",   [1, 2],    3, 0,     6,  1e-8, None),
         ("blank-middle",  [0, 3],    4, 1,     5,  1e-8, None),
         ("zero-label",    [0, 1],    3, 2,     6,  0.0,  1),      # a label's class is impossible in some frames: part of the lattice is closed
         ("zero-other",    [0, 1],    4, 3,     6,  0.0,  2),      # a class outside the labels
         ("one-way",       [0, 0, 1], 3, 2,     4,  1e-8, None)]   # label, blank, label, label: the only alignment


def _posteriors(name, Cn, Tp, zero):
    rng = np.random.default_rng(sum(map(ord, name)))
    P = rng.dirichlet(np.ones(Cn), size=Tp + 2)
    if zero is not None:
        P[3:5, zero] = 0.0
        P /= P.sum(axis=1, keepdims=True)
    return P.astype(np.float32)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_enumeration(case):
    name, labels, Cn, blank, Tp, eps, zero = case
    P = _posteriors(name, Cn, Tp, zero)
    logy = ar.log_emissions(P, 2, eps)
    ref = en.enumerate_paths(logy, labels, blank)
    got = en.lattice(logy, labels, blank)
    assert abs(got["H"] - ref["H"]) <= 1e-12 and abs(got["logp"] - ref["logp"]) <= 1e-12 and abs(got["m"] - ref["m"]) <= 1e-12
    assert np.isfinite(got["dHdu"]).all() and np.abs(got["dHdu"] - ref["dHdu"]).max() <= 1e-12
    # m_t is the same at every frame; the rows sum to zero; 0 <= H <= ln(number of alignments)
    assert np.abs(got["mt"] - got["m"]).max() <= 1e-12
    assert np.abs(got["dHdu"].sum(axis=1)).max() <= 1e-12
    assert -1e-12 <= got["H"] <= np.log(ref["n"]) + 1e-12
    if name in ("no-label", "one-way"):
        assert ref["n"] == 1 and abs(got["H"]) <= 1e-12 and np.abs(got["dHdu"]).max() <= 1e-12
    else:
        assert got["H"] > 0.1 and np.abs(got["dHdu"]).max() > 1e-2
    if zero is not None:
        assert np.isneginf(logy).any()


def test_what_does_not_fit_has_no_entropy():
    P = _posteriors("nofit", 3, 2, None)
    assert en.enumerate_paths(ar.log_emissions(P, 2, 1e-8), [0, 0], 2) is None and en.lattice(ar.log_emissions(P, 2, 1e-8), [0, 0], 2) is None
    r = en.entropy(P, [0, 0])
    assert r["H"] == 0.0 and r["logp"] == -np.inf and not r["dlogits"].any()
    r = en.entropy(P, [0], input_len=0)
    assert r["H"] == 0.0 and r["logp"] == -np.inf and not r["dlogits"].any()


@pytest.mark.parametrize("labels,Cn,blank,eps", [([0, 1, 1], 4, 3, 1e-8), ([2], 4, 1, 1e-3), ([], 3, 2, 1e-8)])
def test_logit_gradient_equals_central_differences(labels, Cn, blank, eps):
    """dH/dlogits through y = softmax(log(P + eps)) and P = softmax(logits), against (H(z + h) - H(z - h)) / 2h of the restatement's own
    H (fp64 posteriors, h = 1e-6: truncation h^2, rounding 1e-16 / h)."""
    rng = np.random.default_rng(5 + len(labels))
    T = 9
    z = rng.standard_normal((T, Cn))
    H = lambda zz: en.entropy(en.softmax(zz), labels, T - 3, 2, blank, eps)["H"]
    got = en.entropy(en.softmax(z), labels, T - 3, 2, blank, eps)["dlogits"]
    num = np.zeros_like(z)
    h = 1e-6
    for t in range(T):
        for k in range(Cn):
            d = np.zeros_like(z)
            d[t, k] = h
            num[t, k] = (H(z + d) - H(z - d)) / (2 * h)
    assert np.abs(got - num).max() <= 1e-8, np.abs(got - num).max()
    assert not got[:2].any() and not got[-1:].any() and np.abs(got.sum(axis=1)).max() <= 1e-12
    if labels:
        assert np.abs(got).max() > 1e-3


def test_ascent_step_raises_the_entropy():
    """The planted inputs and the step size of the GPU ascent test: H(z + lr dH/dz) > H(z) on every sample with a gradient, by far more
    than float32 resolves (the kernel's H is held to 1e-4 max(1, |m|): below 1e-3 here)."""
    z, lab, il, ll = en.ascent_inputs()
    P = en.softmax(z).astype(np.float32)
    H, m, dz, logp = en.batch(P, lab, il, ll, en.ASCENT_SKIP, None, en.ASCENT_EPS)
    H2 = en.batch(en.softmax(z + en.ASCENT_LR * dz).astype(np.float32), lab, il, ll, en.ASCENT_SKIP, None, en.ASCENT_EPS)[0]
    moving = np.abs(dz).reshape(len(H), -1).max(axis=1) > 0
    assert list(moving) == [True, True, False, False, True] and np.isneginf(logp[3]) and H[2] == 0.0 and H[3] == 0.0
    assert np.abs(m).max() < 10.0
    assert (H2[moving] - H[moving] > 0.05).all(), (H, H2)
    assert np.array_equal(H2[~moving], H[~moving])
