"""CPU (no GPU): the restatement of mgr_ctc_sample_paths the GPU tests compare with bit for bit (tests/sample_ref.py) - its collapse and
merge against loops written out by hand, the edges of the draw, and the distribution of the sampled labellings against the exact one."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_ref as sr  # noqa: E402


def _collapse_loop(path, blank):
    out, prev = [], None
    for v in path:
        if v != prev and v != blank:
            out.append(int(v))
        prev = v
    return out


@pytest.mark.parametrize("path, blank, want", [
    ([2, 2, 2, 2], 2, []),                            # all blank
    ([0, 1, 0, 1], 2, [0, 1, 0, 1]),                  # no blank
    ([0, 0, 2, 0, 1, 1, 2, 2, 1], 2, [0, 0, 1, 1]),   # repeats across a blank survive, repeats without one do not
    ([], 2, []),                                      # length 0
    ([1], 2, [1]), ([2], 2, []),                      # length 1
    ([0, 0, 1, 0], 0, [1]),                           # the blank need not be the last class
])
def test_collapse_is_the_three_line_loop(path, blank, want):
    assert sr.collapse(np.asarray(path, np.int32), blank) == want == _collapse_loop(path, blank)


def test_collapse_on_random_paths():
    rng = np.random.default_rng(0)
    for _ in range(200):
        C = int(rng.integers(2, 5))
        path = rng.integers(0, C, int(rng.integers(0, 12)))
        blank = int(rng.integers(0, C))
        assert sr.collapse(path, blank) == _collapse_loop(list(path), blank)


def test_merge_counts_order_and_absent_slots():
    assert sr.merge([[1], [0, 1], [1], [], [0, 1], [1]]) == ([[1], [0, 1], []], [3, 2, 1])
    rng = np.random.default_rng(1)
    B, T, C, K, skip = 3, 9, 3, 8, 2
    P = rng.random((B, T, C)).astype(np.float32) ** 8          # (peaked: duplicates)
    P /= P.sum(axis=2, keepdims=True)
    il = np.array([7, 3, 0], np.int32)
    out, out_len, count, nu, path = sr.sample_paths(P, il, skip, C - 1, 1e-8, 11, K)
    assert (count.sum(axis=1) == K).all() and (nu >= 1).all() and nu[2] == 1 and out_len[2, 0] == 0 and count[2, 0] == K
    assert (nu < K).any()                                       # (the premise: something was merged)
    for b in range(B):
        labs = [sr.collapse(path[b, k, :sr.clip_len(il[b], T - skip)], C - 1) for k in range(K)]
        first = [lab for i, lab in enumerate(labs) if lab not in labs[:i]]
        assert [[int(v) for v in out[b, j, :out_len[b, j]]] for j in range(nu[b])] == first       # order of first occurrence
        assert [int(count[b, j]) for j in range(nu[b])] == [labs.count(lab) for lab in first]
        assert (out_len[b, nu[b]:] == -1).all() and (count[b, nu[b]:] == 0).all() and (out[b, nu[b]:] == -1).all()
        for j in range(nu[b]):
            assert (out[b, j, out_len[b, j]:] == -1).all()
        assert (path[b, :, sr.clip_len(il[b], T - skip):] == -1).all()
    paths, counts = sr.lists(out, out_len, count)
    assert [len(p) for p in paths] == list(nu) and [sum(c) for c in counts] == [K] * B


@pytest.mark.parametrize("blank", [0, 2])
def test_an_all_zero_row_gives_the_blank(blank):
    P = np.zeros((1, 6, 3), np.float32)
    P[0, 3] = [0.2, 0.5, 0.3]
    out, out_len, count, nu, path = sr.sample_paths(P, None, 0, blank, 0.0, 3, 4)
    assert (path[0][:, [0, 1, 2, 4, 5]] == blank).all()


@pytest.mark.parametrize("zero", [0, 1, 2])
def test_a_class_of_weight_zero_is_never_drawn(zero):
    rng = np.random.default_rng(zero)
    P = rng.random((2, 40, 3)).astype(np.float32)
    P[:, :, zero] = 0.0
    path = sr.sample_paths(P, None, 0, 2, 0.0, 5, 32)[4]
    assert (path != zero).all() and (path >= 0).all()
    assert all((path == c).any() for c in range(3) if c != zero)


def _exact_labelling_probabilities(P, blank, eps):
    y = (P.astype(np.float64) + np.float64(np.float32(eps)))
    y /= y.sum(axis=1, keepdims=True)
    T, C = y.shape
    prob = {}
    for pi in itertools.product(range(C), repeat=T):
        lab = tuple(sr.collapse(np.asarray(pi), blank))
        prob[lab] = prob.get(lab, 0.0) + float(np.prod(y[np.arange(T), pi]))
    return prob


@pytest.mark.parametrize("seed", [1, 20261019, 2 ** 63 + 5])
def test_sampled_labellings_follow_the_exact_distribution(seed):
    T, C, N = 5, 3, 4096
    P = np.random.default_rng(7).random((1, T, C)).astype(np.float32)
    P /= P.sum(axis=2, keepdims=True)
    prob = _exact_labelling_probabilities(P[0], C - 1, 1e-8)
    assert abs(sum(prob.values()) - 1.0) < 1e-12
    out, out_len, count, nu, _ = sr.sample_paths(P, None, 0, C - 1, 1e-8, seed, N)          # (one restatement call with K = 4096)
    seen = {tuple(int(v) for v in out[0, j, :out_len[0, j]]): int(count[0, j]) for j in range(nu[0])}
    assert sum(seen.values()) == N and set(seen) <= set(prob)
    checked, worst = 0, 0.0
    for lab, p in prob.items():
        if N * p >= 5:
            f = seen.get(lab, 0) / N
            sigma = np.sqrt(p * (1 - p) / N)
            worst = max(worst, abs(f - p) / sigma)
            assert abs(f - p) <= 5 * sigma, (lab, f, p)
            checked += 1
    print("labellings checked %d, largest deviation %.2f sigma" % (checked, worst))
    assert checked >= 20
