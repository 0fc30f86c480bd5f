"""Live recognition restated on the host (include/mgr.h K20 / K21): test infrastructure, no GPU.

The network side is fp64 numpy with its OWN LSTM step that takes and returns a state (oracle/keras_ref.py starts every direction from
zero): scan() is one direction over one window from gate pre-activations (what mgr_lstm_scan_window computes), Network runs a
whole spec window by window with the forward states carried, run_session cuts a session of known length into live.plan_windows'
windows.  The decode side is integers and float32: GreedyState.window() is mgr_live_greedy for one session, one operation at a
time in the kernel's order, so the GPU tests ask for `==`.  Weights and Z are in Keras layout (gate column blocks i, f, c, o)."""
import numpy as np

from mgr_amd.live import plan_windows


def hard_sigmoid(z):
    return np.clip(0.2 * z + 0.5, 0.0, 1.0)


def lstm_step(z, h, c, U):
    """One cell step from the input part z (4H,) of the pre-activation and the state (h, c): returns the new (h, c)."""
    H = h.shape[0]
    a = z + h @ U
    i, f, g, o = hard_sigmoid(a[:H]), hard_sigmoid(a[H:2 * H]), np.tanh(a[2 * H:3 * H]), hard_sigmoid(a[3 * H:])
    c = f * c + i * g
    return o * np.tanh(c), c


def scan(Z, U, state=None, n_keep=None, reverse=False):
    """One direction over one window of one session.  Z (n_valid, 4H): x . W + b.  Forward: starts from state = (h, c) (None: zero),
    returns y (n_valid, H) and the state after frame n_keep - 1 (the state given when n_keep == 0).  Reverse: starts from zero at
    the last frame; the state returned is None."""
    n, H = Z.shape[0], U.shape[0]
    y = np.zeros((n, H), Z.dtype)
    if reverse:
        h, c = np.zeros(H, Z.dtype), np.zeros(H, Z.dtype)
        for t in range(n - 1, -1, -1):
            h, c = lstm_step(Z[t], h, c, U)
            y[t] = h
        return y, None
    h, c = (np.zeros(H, Z.dtype), np.zeros(H, Z.dtype)) if state is None else (state[0].copy(), state[1].copy())
    n_keep = n if n_keep is None else n_keep
    out = (h, c)
    for t in range(n):
        h, c = lstm_step(Z[t], h, c, U)
        y[t] = h
        if t == n_keep - 1:
            out = (h, c)
    return y, out


def bilstm_window(x, wf, wb, state, n_keep):
    """Bidirectional layer over one window x (n_valid, F): wf / wb = (W, U, b); returns y (n_valid, 2H) and the forward state."""
    yf, st = scan(x @ wf[0] + wf[2], wf[1], state, n_keep, False)
    yb, _ = scan(x @ wb[0] + wb[2], wb[1], None, None, True)
    return np.concatenate([yf, yb], axis=1), st


def _wb(w, p):
    return (w[p + "/W"], w[p + "/U"], w[p + "/b"])


class Network:
    """One session of a spec (dict as NetworkSpec.to_dict()) with fp64 weights in Keras layout: window() runs one window and carries
    the forward state of every Bidirectional layer."""

    def __init__(self, spec, w):
        self.spec, self.w = spec, {k: np.asarray(v, np.float64) for k, v in w.items()}
        self.state = {}

    def _layer(self, prefix, x, n_keep):
        y, self.state[prefix] = bilstm_window(x, _wb(self.w, prefix + "/fwd"), _wb(self.w, prefix + "/bwd"), self.state.get(prefix), n_keep)
        return y

    def window(self, inputs, n_keep):
        """inputs {stream: (n_valid, F)}; returns the posteriors (n_keep, C) this window answers."""
        outs = []
        for s in self.spec["streams"]:
            cur, ys = np.asarray(inputs[s["name"]], np.float64), []
            for k in range(len(s["layers"])):
                cur = self._layer("%s/l%d" % (s["name"], k), cur, n_keep)
                ys.append(cur)
            outs.append(ys[0] + ys[1] if (s.get("residual") and len(ys) == 2) else ys[-1])
        feat = np.concatenate(outs, axis=1)
        if self.spec.get("fusion"):
            feat = self._layer("fusion", feat, n_keep)
        z = feat @ self.w["dense/W"] + self.w["dense/b"]
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return (e / e.sum(axis=1, keepdims=True))[:n_keep]


def run_session(spec, w, inputs, chunk, lookahead):
    """A whole session {stream: (n, F)} through plan_windows' windows: the posteriors (n, C) a live session gives."""
    net = Network(spec, w)
    n = next(iter(inputs.values())).shape[0]
    rows = [net.window({k: v[s0:s0 + nv] for k, v in inputs.items()}, nk) for s0, nv, nk in plan_windows(n, chunk, lookahead)]
    return np.concatenate(rows, axis=0)


# ---- the carried greedy decode ------------------------------------------------------------------------------------------------------
class GreedyState:
    """mgr_live_greedy for one session: the open run (label, first, last, count, float32 sum) carried from window to window."""

    def __init__(self, blank, skip):
        self.blank, self.skip = blank, skip
        self.consumed = 0
        self.open = None     # [label, first, last, count, sum]

    def _close(self, events):
        if self.open is not None and self.open[0] != self.blank:
            lab, first, last, cnt, s = self.open
            events.append((lab, first, last, float(np.float32(s) / np.float32(cnt))))
        self.open = None

    def labels(self, best, prob, flush=False):
        """The next frames of the session as (best label, its probability) per frame; returns the events this call finalises."""
        events = []
        for b, p in zip(best, prob):
            g = self.consumed
            self.consumed += 1
            if g < self.skip:
                continue
            if self.open is not None and self.open[0] == int(b):
                self.open[2] = g
                self.open[3] += 1
                self.open[4] = np.float32(self.open[4] + np.float32(p))
            else:
                self._close(events)
                self.open = [int(b), g, g, 1, np.float32(np.float32(0) + np.float32(p))]
        if flush:
            self._close(events)
        return events

    def window(self, P, flush=False):
        """P (n_keep, C) float32 posteriors: argmax with the first index on ties, then labels()."""
        P = np.asarray(P, np.float32).reshape(-1, P.shape[-1])
        return self.labels(P.argmax(axis=1), P.max(axis=1), flush)


def collapse_offline(labels, blank, skip=0):
    """The non-blank runs of a whole label string as (label, first, last) - the offline collapse, written without any state."""
    out, t, n = [], skip, len(labels)
    while t < n:
        e = t
        while e + 1 < n and labels[e + 1] == labels[t]:
            e += 1
        if labels[t] != blank:
            out.append((int(labels[t]), t, e))
        t = e + 1
    return out


# ---- layouts ------------------------------------------------------------------------------------------------------------------------
def pack(M, H):
    """Keras column order (g * H + u) -> the packed order of the C ABI (u * 4 + g) on the last axis."""
    M = np.asarray(M)
    return np.ascontiguousarray(M.reshape(M.shape[:-1] + (4, H)).swapaxes(-1, -2).reshape(M.shape))
