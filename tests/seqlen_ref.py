"""fp64 references for per-sample sequence lengths, shared by tests/test_cpu_seqlen.py and the GPU tests.

  truncated(c, rand, lens)   the oracle run on every sample ALONE at its own length: what a length-aware engine must compute
  mechanism(c, rand, lens)   the engine's mechanism restated on the padded batch: a copy of oracle.keras_ref.lstm_forward that,
                             in a reverse direction, takes zero gate pre-activations in a sample's tail and caches zero gates there;
                             everything else is oracle.network_ref.loss_and_grads as it stands
  padded(c, rand, lens)      the plain oracle on the padded batch with input_length = len - 2: what an engine without lengths computes

The cases are tests/rng_cases.py's (replayed device randomness); LENS are the lengths the three of them are cut to."""
import contextlib
import functools

import numpy as np

from oracle import keras_ref as kr
from oracle import network_ref as nr
from tests import rng_cases as rc

LENS = {"fusion_tiny": (12, 8, 6), "unimodal_tiny": (12, 9, 6), "split_wide": (23, 17, 12, 9, 7)}
NAMES = list(LENS)


def il_of(lens):
    """The CTC input lengths that go with sequence lengths: max(0, len - 2), shaped like the batches' input_length."""
    return np.maximum(0, np.asarray(lens, np.int64) - 2).reshape(-1, 1)


def f64(d):
    return {k: np.asarray(v, np.float64) for k, v in d.items()}


def cut_rand(rand, b, n):
    """The randomness of sample b alone at n frames: per-frame tensors cut to [:n], the (4, B, F) input masks by sample."""
    out = {}
    for k, v in (rand or {}).items():
        v = np.asarray(v, np.float64)
        out[k] = v[b:b + 1, :n] if (k.endswith("/noise") or k == "head/mask") else v[:, b:b + 1]
    return out


def truncated(c, rand, lens, inputs=None):
    """(mean loss, loss_b (B,), gradients of the batch mean, [P_b (len_b, C)]): every sample alone at its own length, il = len - 2,
    the gradients summed over the samples as g / B."""
    inputs = f64(inputs or c["inputs"])
    w = f64(c["w0"])
    B = c["B"]
    lb, Ps, grads = np.zeros(B), [], None
    for b, n in enumerate(lens):
        assert n >= 1
        x = {k: v[b:b + 1, :n] for k, v in inputs.items()}
        _, l1, g, P = nr.loss_and_grads(c["spec"], w, x, c["labels"][b:b + 1], il_of([n]), c["ll"][b:b + 1], cut_rand(rand, b, n) if rand else None)
        lb[b] = float(l1[0])
        Ps.append(P[0])
        grads = {k: v / B for k, v in g.items()} if grads is None else {k: grads[k] + g[k] / B for k in g}
    return float(lb.mean()), lb, grads, Ps


def forward_truncated(c, lens, inputs=None):
    """[P_b (len_b, C)] of the learning phase 0 forward of every sample alone at its own length."""
    inputs = f64(inputs or c["inputs"])
    w = f64(c["w0"])
    return [nr.forward(c["spec"], w, {k: v[b:b + 1, :n] for k, v in inputs.items()})[0][0] for b, n in enumerate(lens)]


def _lstm_forward_lens(lens):
    lens = np.asarray(lens)

    def lstm_forward(x, W, U, b, mask4=None, reverse=False):
        """oracle.keras_ref.lstm_forward with the fill: reverse directions take Z = 0 at t >= len and cache i = f = g = o = 0 there."""
        dt = x.dtype
        B, T, F = x.shape
        H = U.shape[0]
        h = np.zeros((B, H), dt)
        c = np.zeros((B, H), dt)
        y = np.empty((B, T, H), dt)
        gi, gf, gg, go, cs = (np.empty((B, T, H), dt) for _ in range(5))
        Wg = [W[:, k * H:(k + 1) * H] for k in range(4)]
        Ug = [U[:, k * H:(k + 1) * H] for k in range(4)]
        bg = [b[k * H:(k + 1) * H] for k in range(4)]
        for t in (range(T - 1, -1, -1) if reverse else range(T)):
            xt = x[:, t, :]
            xs = [xt, xt, xt, xt] if mask4 is None else [xt * mask4[k] for k in range(4)]
            tail = (t >= lens)[:, None] if reverse else np.zeros((B, 1), bool)
            # (the projection's Z, bias included, is what the fill overwrites; h is exactly 0 there, so h @ U adds nothing)
            z = [np.where(tail, 0.0, xs[k] @ Wg[k] + bg[k]) + h @ Ug[k] for k in range(4)]
            i, f, g, o = kr.hard_sigmoid(z[0]), kr.hard_sigmoid(z[1]), np.tanh(z[2]), kr.hard_sigmoid(z[3])
            c = f * c + i * g
            h = o * np.tanh(c)
            y[:, t, :] = h
            cs[:, t, :] = c
            for buf, v in ((gi, i), (gf, f), (gg, g), (go, o)):
                buf[:, t, :] = np.where(tail, 0.0, v)          # the saved gates of the tail are zeroed behind the scan
        return y, dict(x=x, W=W, U=U, mask4=mask4, reverse=reverse, y=y, i=gi, f=gf, g=gg, o=go, c=cs)
    return lstm_forward


@contextlib.contextmanager
def _filled(lens):
    keep = kr.lstm_forward
    kr.lstm_forward = _lstm_forward_lens(lens)
    try:
        yield
    finally:
        kr.lstm_forward = keep


def mechanism(c, rand, lens, inputs=None):
    """network_ref.loss_and_grads on the padded batch with the fill restated inside the LSTM forward: (loss, loss_b, grads, P)."""
    with _filled(lens):
        return nr.loss_and_grads(c["spec"], f64(c["w0"]), f64(inputs or c["inputs"]), c["labels"], il_of(lens), c["ll"],
                                 f64(rand) if rand else None)


def padded(c, rand, lens, inputs=None):
    """The plain oracle on the padded batch, told only input_length = len - 2."""
    return nr.loss_and_grads(c["spec"], f64(c["w0"]), f64(inputs or c["inputs"]), c["labels"], il_of(lens), c["ll"], f64(rand) if rand else None)


def with_tails(c, rand, lens, fill):
    """(inputs, rand) with every tail - of the inputs, the noise and the head mask - replaced: fill(shape) -> values.  The input
    masks are per sample and have no tail."""
    inputs, rand = f64(c["inputs"]), {k: np.array(v, np.float64) for k, v in (rand or {}).items()}
    for d, keys in ((inputs, list(inputs)), (rand, [k for k in rand if k.endswith("/noise") or k == "head/mask"])):
        for k in keys:
            d[k] = d[k].copy()
            for b, n in enumerate(lens):
                d[k][b, n:] = fill(d[k][b, n:].shape)
    return inputs, rand


def repeated_tails(c, lens):
    """The case's inputs with zero tails and with tails that repeat the sample's own real frames (two paddings of the same samples)."""
    zero, rep = f64(c["inputs"]), f64(c["inputs"])
    for k in zero:
        zero[k], rep[k] = zero[k].copy(), rep[k].copy()
        for b, n in enumerate(lens):
            zero[k][b, n:] = 0.0
            T = rep[k].shape[1]
            rep[k][b, n:] = rep[k][b, np.arange(n, T) % n]
    return zero, rep


def worst(a, b):
    """Largest deviation of gradient dicts a from b, each tensor relative to its largest entry in b: {name: error}."""
    return {k: float(np.abs(np.asarray(a[k], np.float64) - b[k]).max() / max(1e-300, np.abs(b[k]).max())) for k in b}


@functools.lru_cache(maxsize=None)
def truncated_step(name, step=0):
    """truncated() of a case under the replay of `step`, computed once per session."""
    c = rc.case(name)
    return truncated(c, c["rands"][step], LENS[name])
