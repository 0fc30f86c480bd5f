"""Input builders of the CTC edge tests (tests/test_gpu_ctc_edges.py runs them through mgr_ctc_loss_grad, tests/test_cpu_ctc_edges.py
checks their premises with the oracle alone).  A case is a namespace: P (B, T, C) float32, labels (B, Lmax) int64 padded -1, il / ll
(B,), skip, blank, eps, `inf` - the samples the case DESIGNATES to have loss = +inf - and, for the closed forms, `closed` {sample:
loss}.  case(name) and reference(name) build once per process and hand out read-only arrays.

csrc/ctc.hip lays the lattice across one wave as (blank, label) pairs, ppl = ceil((Lmax + 1) / 64) pairs per lane, stores rows two
time steps at a time, prefetches emissions in chunks of 8 (ppl <= 2) or 4 steps, and renormalises every 16 steps: the shapes below
sit on those boundaries."""
import functools
import types

import numpy as np

from oracle import keras_ref as kr

A_LMAX = (63, 64, 126, 127, 128, 191, 192, 255)
A_PPL = dict(zip(A_LMAX, (1, 2, 2, 2, 3, 3, 4, 4)))
B_L = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255)
B_WIDER = {"i": (65, 100), "ii": (129, 200)}          # form -> (L, Lmax > L)
C_TPS = tuple(range(1, 41)) + (255, 256, 257, 258, 511, 512, 513)

A_NAMES = tuple("a-Lmax%d" % n for n in A_LMAX)
B_NAMES = tuple("b-%s-L%d" % (f, n) for f in ("i", "ii") for n in B_L) + tuple("b-%s-L%d-Lmax%d" % ((f,) + B_WIDER[f]) for f in ("i", "ii"))
C_NAMES = ("c-sweep", "c-sweep-ppl3")
D_NAMES = ("d-base", "d-skip0", "d-skip1", "d-skip5", "d-blank0", "d-blankmid", "d-eps0", "d-eps1e-3")
G_NAMES = ("g-peaked12", "g-peaked25")
ALL_NAMES = A_NAMES + B_NAMES + C_NAMES + D_NAMES + ("e-raw", "e-clipped", "f-logzero") + G_NAMES + ("h-drift",)


def ppl_of(Lmax):
    """pairs per lane the host picks (mgr_ctc_loss_grad)"""
    return (Lmax + 1 + 63) // 64


def softmax32(z):
    P = np.exp(z - z.max(-1, keepdims=True))
    return (P / P.sum(-1, keepdims=True)).astype(np.float32)


def rand_probs(rng, B, T, Cn, scale=2.0):
    return softmax32(rng.standard_normal((B, T, Cn)) * scale)


def _make(name, P, labels, il, ll, skip=2, blank=None, eps=1e-8, inf=(), closed=None):
    c = types.SimpleNamespace(name=name, P=np.ascontiguousarray(P, np.float32), labels=np.asarray(labels, np.int64),
                              il=np.asarray(il, np.int64), ll=np.asarray(ll, np.int64), skip=int(skip),
                              blank=P.shape[2] - 1 if blank is None else int(blank), eps=float(eps), inf=tuple(inf), closed=closed)
    for a in (c.P, c.labels, c.il, c.ll):
        a.flags.writeable = False
    return c


def _labels(rng, B, Lmax, ll, Cn, blank):
    """random labels from the non-blank classes, padded -1"""
    classes = np.array([k for k in range(Cn) if k != blank])
    lab = -np.ones((B, Lmax), np.int64)
    for b in range(B):
        lab[b, :ll[b]] = classes[rng.integers(0, len(classes), size=ll[b])]
    return lab


# ---- (a) every pairs-per-lane instantiation, states on the lane boundaries -------------------------------------------------------
def _case_a(Lmax):
    """B = 5 (the four label lengths asked for do not fit into three samples; odd, so the last two-sample workgroup holds one).
    Sample 0: L = Lmax, label 2k + 1 repeats label 2k (can_skip false at the odd pairs - the first pair of every second lane at
    ppl = 1).  Sample 4: L = Lmax, label 2k repeats label 2k - 1 (can_skip false at the even pairs - the first pair of EVERY lane at
    ppl = 2 and 4).  Sample 1: L = Lmax - 1 in barely more than 2 L + 1 frames.  Sample 2: a length just past a multiple of 64.
    Sample 3: one label in 5 frames."""
    rng = np.random.default_rng(1000 + Lmax)
    Cn = 44 if Lmax == 255 else 22
    B, skip, T = 5, 2, min(2 * Lmax + 74, 560)
    past = max(v for v in (33, 65, 129, 193) if v < Lmax - 1)
    ll = np.array([Lmax, Lmax - 1, past, 1, Lmax])
    lab = _labels(rng, B, Lmax, ll, Cn, Cn - 1)
    lab[0, 1:Lmax:2] = lab[0, 0:Lmax - 1:2]
    lab[4, 2:Lmax:2] = lab[4, 1:Lmax - 1:2]
    il = np.array([T - skip, 2 * ll[1] + 3, T - skip - 1, 5, T - skip - 1])
    return _make("a-Lmax%d" % Lmax, rand_probs(rng, B, T, Cn), lab, il, ll, skip=skip)


# ---- (b) single-alignment lattices with a closed form ----------------------------------------------------------------------------
def closed_form_path(form, L, blank, lab):
    """the ONE alignment of form (i) (L equal labels in 2 L - 1 frames: label, blank, label, ...) or (ii) (labels alternating
    between two classes in L frames: a label per frame)"""
    if form == "i":
        path = np.full(2 * L - 1, blank, np.int64)
        path[0::2] = lab
        return path
    return np.asarray(lab, np.int64).copy()


def _case_b(form, L, Lmax):
    """Sample 0: the single-alignment lattice.  Sample 1: the same inputs one frame shorter - nothing fits, +inf.  Sample 2: the
    same inputs one frame longer (many alignments; oracle only)."""
    rng = np.random.default_rng((7000 if form == "i" else 9000) + L + 3 * Lmax)
    B, Cn, skip = 3, 6, 2
    blank = Cn - 1
    Tp = 2 * L - 1 if form == "i" else L
    T = Tp + skip + 2
    P = rand_probs(rng, B, T, Cn)
    P[1] = P[0]
    P[2] = P[0]
    lab = -np.ones((B, Lmax), np.int64)
    lab[:, :L] = 2 if form == "i" else np.where(np.arange(L) % 2 == 0, 1, 3)
    path = closed_form_path(form, L, blank, lab[0, :L])
    u = P[0, skip:skip + Tp].astype(np.float64) + 1e-8
    y = u / u.sum(-1, keepdims=True)
    closed = {0: float(-np.log(y[np.arange(Tp), path]).sum())}
    name = "b-%s-L%d" % (form, L) + ("" if Lmax == L else "-Lmax%d" % Lmax)
    return _make(name, P, lab, [Tp, Tp - 1, Tp + 1], [L, L, L], skip=skip, inf=(1,), closed=closed)


# ---- (c) a sweep over lengths in one launch --------------------------------------------------------------------------------------
def _case_c(ppl3):
    """Per-sample input lengths inside one batch: both parities, T' = 1 and 2, every residue mod 8 and mod 16, both sides of the
    256-frame step of the per-frame kernels' grid.  L = min(3, (T' + 1) // 2): 2 L - 1 <= T', so any labels fit.  The ppl = 3
    sweep (chunks of 4 steps) has L = 2 distinct labels and T' = 1 ... 20: T' = 1 cannot hold them and is designated +inf."""
    if ppl3:
        rng = np.random.default_rng(31)
        tps = rng.permutation(np.arange(1, 21))
        B, T, Cn, Lmax = 20, 23, 6, 150
        ll = np.full(B, 2)
        lab = -np.ones((B, Lmax), np.int64)
        for b in range(B):
            lab[b, :2] = rng.permutation(Cn - 1)[:2]
        return _make("c-sweep-ppl3", rand_probs(rng, B, T, Cn), lab, tps, ll, inf=tuple(np.nonzero(tps == 1)[0]))
    rng = np.random.default_rng(30)
    tps = rng.permutation(np.array(C_TPS))
    B, T, Cn, Lmax = 47, 515, 6, 5
    ll = np.minimum(3, (tps + 1) // 2)
    return _make("c-sweep", rand_probs(rng, B, T, Cn), _labels(rng, B, Lmax, ll, Cn, Cn - 1), tps, ll)


# ---- (d) arguments never varied ---------------------------------------------------------------------------------------------------
def _case_d(name):
    kw = {"d-base": {}, "d-skip0": dict(skip=0), "d-skip1": dict(skip=1), "d-skip5": dict(skip=5), "d-blank0": dict(blank=0),
          "d-blankmid": dict(blank=3), "d-eps0": dict(eps=0.0), "d-eps1e-3": dict(eps=1e-3)}[name]
    rng = np.random.default_rng(40 + D_NAMES.index(name))
    B, T, Cn, Lmax = 3, 60, 7, 9
    skip, blank = kw.get("skip", 2), kw.get("blank", Cn - 1)
    ll = np.array([9, 4, 1])
    il = np.array([T - skip, T - skip - 7, 20])
    return _make(name, rand_probs(rng, B, T, Cn), _labels(rng, B, Lmax, ll, Cn, blank), il, ll, skip=skip, blank=blank,
                 eps=kw.get("eps", 1e-8))


# ---- (e) out-of-range arguments ---------------------------------------------------------------------------------------------------
def _case_e(clipped):
    """input_len beyond T - skip and below 0, label_len beyond Lmax and below 0, label values beyond the class range: the kernels
    clip them (include/mgr.h, K6).  The clipped twin must give the same bits.  blank = C // 2, so the clipped label values 0 and
    C - 1 are ordinary classes.  input_len <= 0: +inf and a zero gradient."""
    rng = np.random.default_rng(50)
    B, T, Cn, Lmax, skip, blank = 5, 30, 7, 6, 2, 3
    P = rand_probs(rng, B, T, Cn)
    il = np.array([T + 5, -3, 0, 17, T - skip])
    ll = np.array([Lmax + 4, 2, 3, -2, 3])
    lab = -np.ones((B, Lmax), np.int64)
    lab[0] = [1, 99, -7, 2, 4, 5]
    lab[1, :2] = [0, 1]
    lab[2, :3] = [4, 5, 6]
    lab[3, :2] = [2, 2]            # (label_len -2: not read)
    lab[4, :3] = [6, 250, -1]
    if clipped:
        il = np.clip(il, 0, T - skip)
        ll = np.clip(ll, 0, Lmax)
        lab = np.where(np.arange(Lmax)[None, :] < ll[:, None], np.clip(lab, 0, Cn - 1), -1)
    return _make("e-clipped" if clipped else "e-raw", P, lab, il, ll, skip=skip, blank=blank, inf=(1, 2))


# ---- (f) log 0 --------------------------------------------------------------------------------------------------------------------
def _case_f():
    """eps = 0 and exact zeros in P (the loss alone: the reference's gradient is 0 / 0 on such rows).  Sample 0: a label's class is
    zero in every frame - +inf.  Sample 1: a class outside the label sequence is zero for a stretch.  Sample 2: a label's class is
    zero for a stretch only."""
    rng = np.random.default_rng(60)
    B, T, Cn, Lmax = 3, 40, 6, 3
    P = rand_probs(rng, B, T, Cn).astype(np.float64)
    P[0, :, 2] = 0.0
    P[1, 10:26, 4] = 0.0
    P[2, 10:26, 2] = 0.0
    P = (P / P.sum(-1, keepdims=True)).astype(np.float32)
    lab = np.tile(np.array([1, 2, 3]), (B, 1))
    return _make("f-logzero", P, lab, np.full(B, T - 2), np.full(B, 3), eps=0.0, inf=(0,))


# ---- (g) peaked posteriors --------------------------------------------------------------------------------------------------------
def random_alignment(rng, lab, Tp, blank):
    """a valid CTC alignment of the labels `lab` over Tp frames, frame by frame: every label at least one frame, a blank between
    equal neighbours, the spare frames spread at random over labels and blank slots"""
    L = len(lab)
    seg_class, seg_min = [], []
    for i in range(L + 1):
        seg_class.append(blank)
        seg_min.append(1 if 0 < i < L and lab[i - 1] == lab[i] else 0)
        if i < L:
            seg_class.append(int(lab[i]))
            seg_min.append(1)
    seg_min = np.array(seg_min)
    spare = Tp - int(seg_min.sum())
    assert spare >= 0
    dur = seg_min + rng.multinomial(spare, np.full(len(seg_min), 1.0 / len(seg_min)))
    return np.repeat(np.array(seg_class), dur)


def collapse(path, blank):
    """CTC's many-to-one map: merge repeats, drop blanks"""
    path = np.asarray(path)
    keep = np.ones(len(path), bool)
    keep[1:] = path[1:] != path[:-1]
    out = path[keep]
    return out[out != blank]


def peaked_alignments(s):
    """the alignments _case_g raises, per sample (the same random stream as _case_g)"""
    return _peaked(s)[1]


def _peaked(s):
    rng = np.random.default_rng(70)
    B, T, Cn, Lmax, skip = 3, 140, 22, 63, 2
    ll = np.array([63, 40, 63])
    il = np.array([T - skip, T - skip, T - skip - 8])
    lab = _labels(rng, B, Lmax, ll, Cn, Cn - 1)
    z = rng.standard_normal((B, T, Cn))
    paths = []
    for b in range(B):
        path = random_alignment(rng, lab[b, :ll[b]], int(il[b]), Cn - 1)
        z[b, skip + np.arange(il[b]), path] += s
        paths.append(path)
    # the saturated variant's loss is eps * C per frame: eps = 1e-6 puts it at about 3e-3, far above float32's error on it
    return _make("g-peaked%d" % s, softmax32(z), lab, il, ll, skip=skip, eps=1e-8 if s < 20 else 1e-6), paths


# ---- (h) posteriors that contradict the labels: the chains drift ~100 log2 units per frame -----------------------------------------
def _case_h():
    """Near-one-hot posteriors on a class that is neither a label nor the blank, for the whole input (eps = 0): every lattice state
    loses about 100 log2 units per frame, so between two renormalisations 16 steps apart the chains reach -1600, and would reach
    -6400 (float32 ulp 5e-4) with 64 steps between them.  The lattice classes' probabilities are 1e-30 x a log-normal factor, so the
    alignments still compete and the gradient (about - occupancy on those classes) is O(1)."""
    rng = np.random.default_rng(0)
    B, T, Cn, Lmax, L = 6, 1900, 8, 35, 20
    P = 1e-30 * np.exp(rng.standard_normal((B, T, Cn)) * 2.0)
    P[:, :, Cn - 2] = 1.0
    P = (P / P.sum(-1, keepdims=True)).astype(np.float32)
    ll = np.full(B, L)
    return _make("h-drift", P, _labels(rng, B, Lmax, ll, Cn - 2, -1), np.full(B, T - 2), ll, eps=0.0)


# ---- registry ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    kind = name.split("-")[0]
    if kind == "a":
        return _case_a(int(name[len("a-Lmax"):]))
    if kind == "b":
        parts = name.split("-")
        L = int(parts[2][1:])
        return _case_b(parts[1], L, int(parts[3][4:]) if len(parts) > 3 else L)
    if kind == "c":
        return _case_c(name.endswith("ppl3"))
    if kind == "d":
        return _case_d(name)
    if kind == "e":
        return _case_e(name == "e-clipped")
    if kind == "f":
        return _case_f()
    if kind == "g":
        return _peaked(int(name[len("g-peaked"):]))[0]
    if kind == "h":
        return _case_h()
    raise KeyError(name)


def oracle(c, dtype=np.float64):
    """oracle.keras_ref.ctc_loss_grad on P.astype(dtype), sample by sample; the arguments must be in range.  A sample without frames
    (the oracle has no row 0 to start from) has loss +inf; a sample with loss +inf has the ZERO gradient include/mgr.h promises
    (the oracle's own is meaningless there)."""
    B, T, Cn = c.P.shape
    assert (c.il >= 0).all() and (c.il <= T - c.skip).all() and (c.ll >= 0).all() and (c.ll <= c.labels.shape[1]).all(), c.name
    loss = np.full(B, np.inf, dtype)
    dz = np.zeros((B, T, Cn), dtype)
    live = np.nonzero(c.il > 0)[0]
    with np.errstate(all="ignore"):
        lo, dl = kr.ctc_loss_grad(c.P[live].astype(dtype), c.labels[live], c.il[live], c.ll[live], skip=c.skip, blank=c.blank, eps=c.eps)
    loss[live] = lo
    dz[live] = np.where(np.isposinf(lo)[:, None, None], 0.0, dl)
    return loss, dz


@functools.lru_cache(maxsize=None)
def reference(name):
    """the fp64 reference of a case (of the clipped twin for e-raw): (loss (B,), dz (B, T, C)), read-only"""
    loss, dz = oracle(case("e-clipped" if name == "e-raw" else name))
    loss.flags.writeable = False
    dz.flags.writeable = False
    return loss, dz
