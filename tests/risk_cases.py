"""Seeded inputs shared by tests/test_cpu_risk.py and tests/test_gpu_risk.py.  A random case is only worth a GPU run if its gradient
is not trivially zero: at least 90 % of its samples must have two live slots with different risks - the CPU test checks that on every
case listed here, so the GPU tests skip no sample."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rescore_cases as rc  # noqa: E402
import rescore_ref as rr  # noqa: E402

EPS = 1e-8
REL = 1e-4            # K14's bound for logp, the project's bound for a gradient (relative to its largest entry)

# T - skip at the chunk (8 frames) and renormalisation (16 frames) edges
FRAME_EDGES = (1, 7, 8, 15, 16, 17, 33, 70)
# expanded lengths at the pairs-per-lane switches
WIDTH_EDGES = (0, 1, 63, 64, 65, 127, 128)


def fitting_hyps(rng, n_ids, K, To, max_len, p_absent=0.0):
    """K different hypotheses (None: an absent slot) of ids below n_ids that fit To frames with their forced blanks."""
    out, seen = [], []
    for _ in range(K):
        if rng.random() < p_absent:
            out.append(None)
            continue
        for _try in range(200):
            h = [int(v) for v in rng.integers(0, n_ids, int(rng.integers(0, max_len + 1)))]
            if rr.needs(h) <= To and h not in seen:
                break
        else:
            h = []
        seen.append(h)
        out.append(h)
    return out


def random_case(seed, B, To, Cn, K, skip=2, max_len=6, p_absent=0.0, Lh=None, il=None, post_scale=1.0, risk_scale=1.0, max_risk=6,
                conc=0.5):
    """Dirichlet posteriors, K fitting hypotheses per sample, risks drawn in [0, max_risk] (a permutation-like spread: the first two
    present slots get different risks)."""
    rng = np.random.default_rng(seed)
    P = rng.dirichlet(np.full(Cn, conc), size=(B, To + skip)).astype(np.float32)
    il = None if il is None else np.asarray(il, np.int32)
    hyps = []
    for b in range(B):
        Tp = To if il is None else max(0, min(int(il[b]), To))
        hyps.append(fitting_hyps(rng, Cn - 1, K, Tp, min(max_len, max(Tp, 0)), p_absent))
    longest = max([len(h) for row in hyps for h in row if h is not None] + [1])
    hyp, hl = rc.pack(hyps, K, longest if Lh is None else Lh)
    risks = rng.integers(0, max_risk + 1, size=(B, K)).astype(np.int32)
    for b in range(B):
        present = [k for k in range(K) if hyps[b][k] is not None]
        if len(present) >= 2 and risks[b, present[0]] == risks[b, present[1]]:
            risks[b, present[1]] += 1
    return {"name": "seed %d: B %d To %d C %d K %d skip %d" % (seed, B, To, Cn, K, skip), "P": P, "hyp": hyp, "hl": hl, "risks": risks,
            "skip": skip, "il": il, "post_scale": post_scale, "risk_scale": risk_scale, "lexicon": None, "Lcap": max(1, longest)}


def random_cases():
    """The random cases of the GPU tests (every one must pass informative())."""
    cases = []
    for i, To in enumerate(FRAME_EDGES):                       # frame edges, both skips, all C, most K
        cases.append(random_case(100 + i, 3, To, (4, 22, 64)[i % 3], (3, 4, 5, 8)[i % 4], skip=(0, 2)[i % 2], post_scale=(1.0, 0.5)[i % 2]))
    cases.append(random_case(120, 2, 33, 22, 32, max_len=8, post_scale=0.3))                     # K = 32
    cases.append(random_case(121, 3, 17, 4, 4, Lh=17, risk_scale=0.25))                          # rows T - skip wide
    cases.append(random_case(122, 12, 40, 22, 5, il=[40, 39, 33, 32, 31, 17, 16, 15, 9, 8, 7, 100], p_absent=0.1))   # ragged lengths
    return cases


def informative(case, logp):
    """Fraction of the case's samples with at least two live slots (finite logp (N, K) of the restatement) of different risks."""
    ok = 0
    for b in range(logp.shape[0]):
        live = np.isfinite(logp[b])
        ok += len(set(int(v) for v in case["risks"][b][live])) >= 2
    return ok / logp.shape[0]
