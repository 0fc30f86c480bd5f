"""fp64 restatement the expected-risk tests compare against (plain numpy, no GPU): the contract of mgr_ctc_risk_grad in
include/mgr.h, each part stated on its own - logp per slot by rescore_ref.forward, the live slots, the weights, the expected risk,
g_k = dRbar / dlogp_k, and the gradient w.r.t. the Dense logits as the oracle's CTC gradient per hypothesis, combined linearly."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import rescore_ref as rr  # noqa: E402
from oracle import keras_ref as kr  # noqa: E402

NEG_INF = -np.inf


def log_emissions(P, skip, eps, Tp):
    """ln softmax(log(P[skip:skip + Tp] + eps)) in fp64 from P of ANY float dtype (align_ref.log_emissions without its float32 view:
    the finite-difference test moves P in fp64); eps is the kernel's float32 value."""
    u = np.asarray(P, np.float64)[skip:skip + Tp] + np.float64(np.float32(eps))
    with np.errstate(divide="ignore"):
        return np.log(u) - np.log(u.sum(axis=1, keepdims=True))


def slot_labels(entries, Cn, lexicon=None, Lcap=rr.MAX_LABELS):
    """(labels, logp of a slot that is not scored): (None, -inf) absent, (None, NaN) a phrase id outside the lexicon or more than
    Lcap labels, else (the expanded / clipped labels, None)."""
    if entries is None:
        return None, NEG_INF
    if lexicon is not None:
        labels = rr.expand(entries, lexicon)
        if labels is None:
            return None, np.nan
    else:
        labels = [min(max(int(v), 0), Cn - 1) for v in entries]
    if len(labels) > Lcap:
        return None, np.nan
    return labels, None


def sample_slots(hyp_b, hl_b, Cn, lexicon=None, Lcap=rr.MAX_LABELS):
    out = []
    for k in range(len(hl_b)):
        n = int(hl_b[k])
        out.append(slot_labels(None if n < 0 else [int(v) for v in hyp_b[k, :min(n, hyp_b.shape[1])]], Cn, lexicon, Lcap))
    return out


def weights(logp, risks, risk_scale=1.0, post_scale=1.0):
    """One sample: logp (K,) with -inf / NaN for slots that are not live, risks (K,) -> (w (K,), Rbar, g (K,), live (K,) bool)."""
    logp, r = np.asarray(logp, np.float64), np.asarray(risks, np.float64) * float(risk_scale)
    live = np.isfinite(logp)
    w, g = np.zeros(len(logp)), np.zeros(len(logp))
    if not live.any():
        return w, 0.0, g, live
    z = float(post_scale) * logp[live]
    e = np.exp(z - z.max())
    w[live] = e / e.sum()
    rbar = float((w[live] * r[live]).sum())
    if live.sum() >= 2:
        g[live] = float(post_scale) * w[live] * (r[live] - rbar)
    return w, rbar, g, live


def sample_logp(P_b, slots, blank, skip, eps, Tp, logp_fn=None):
    """logp (K,) of one sample's slots over its Tp frames; logp_fn (logy, labels, blank): rescore_ref.forward by default."""
    logy = log_emissions(P_b, skip, eps, Tp)
    fn = logp_fn or rr.forward
    return np.array([fn(logy, lab, blank) if lab is not None else miss for lab, miss in slots], np.float64)


def dlogp_dlogits(P_b, labels, blank, skip, eps, Tp):
    """d logp(labels) / d logits (T, C) of one sample, P_b = softmax(logits): minus the oracle's CTC gradient for that label row."""
    P1 = np.asarray(P_b, np.float64)[None]
    lab = np.asarray(labels, np.int64).reshape(1, -1) if len(labels) else -np.ones((1, 1), np.int64)
    _, dz = kr.ctc_loss_grad(P1, lab, [Tp], [len(labels)], skip=skip, blank=blank, eps=np.float64(np.float32(eps)))
    return -dz[0]


def expected_risk(P, hyp, hyp_len, risks, blank=None, skip=2, eps=1e-8, input_len=None, lexicon=None, Lcap=rr.MAX_LABELS, risk_scale=1.0,
                  post_scale=1.0, gscale=1.0, grad=True, logp_fn=None):
    """The whole contract on a batch: dict(logp (N, K), weight (N, K), risk (N,), g (N, K), live (N, K), dlogits (N, T, C))."""
    P = np.asarray(P)
    N, T, Cn = P.shape
    K = hyp_len.shape[1]
    blank = Cn - 1 if blank is None else blank
    out = {"logp": np.zeros((N, K)), "weight": np.zeros((N, K)), "risk": np.zeros(N), "g": np.zeros((N, K)),
           "live": np.zeros((N, K), bool), "dlogits": np.zeros((N, T, Cn)) if grad else None}
    for b in range(N):
        Tp = T - skip if input_len is None else max(0, min(int(input_len[b]), T - skip))
        slots = sample_slots(hyp[b], hyp_len[b], Cn, lexicon, Lcap)
        out["logp"][b] = sample_logp(P[b], slots, blank, skip, eps, Tp, logp_fn)
        out["weight"][b], out["risk"][b], out["g"][b], out["live"][b] = weights(out["logp"][b], risks[b], risk_scale, post_scale)
        if grad and Tp > 0:
            for k in range(K):
                if out["g"][b, k] != 0.0:
                    out["dlogits"][b] += gscale * out["g"][b, k] * dlogp_dlogits(P[b], slots[k][0], blank, skip, eps, Tp)
    return out


def softmax(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)
