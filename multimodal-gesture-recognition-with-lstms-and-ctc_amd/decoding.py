"""Decode helpers shared by the three sequence_decoding modules (K9).

Frame-wise max / argmax runs on the GPU (mgr_frame_argmax); the reference's confidence filter and the
repeat collapse run on the host (greedy_decode) or, with the frame positions kept, on the GPU (greedy_segments).  The filter reproduces the NET EFFECT of the reference's Python-2 loop
(multimodal_fusion/sequence_decoding.py:45-48: ``list.remove`` deletes the first element equal to the value,
not the visited one): for every label s, the first k_s occurrences of s are dropped, where k_s is the number
of frames whose best label is s with probability below the threshold.  Blanks are kept (they decode to "sil").
"""
import ctypes as C

import numpy as np

from . import _capi

_DEV = [None]


def default_device():
    if _DEV[0] is None:
        _DEV[0] = _capi.Device(0)
    return _DEV[0]


def frame_argmax(pred_out, skip=2, dev=None):
    """(N,T,C) float32 softmax -> best (N,T-skip) int32, prob (N,T-skip) float32, computed on the GPU."""
    dev = dev or default_device()
    P = np.ascontiguousarray(pred_out, dtype=np.float32)
    N, T, Cn = P.shape
    dP = dev.array(P)
    best = dev.empty((N, T - skip), np.int32)
    prob = dev.empty((N, T - skip), np.float32)
    dev.call("mgr_frame_argmax", dP, N, T, Cn, skip, best, prob)
    out = best.download(), prob.download()
    for a in (dP, best, prob):
        a.free()
    return out


def confidence_filter_collapse(best, prob, thr):
    """One sample: best/prob 1-D arrays over frames.  Returns the collapsed label-id list."""
    best = np.asarray(best)
    if thr is not None:
        low = np.asarray(prob) < thr          # float32 value vs Python float, as in the reference
        nlab = int(best.max()) + 1 if best.size else 0
        k = np.bincount(best[low], minlength=nlab)
        # occurrence index of every frame among the frames with the same label
        order = np.argsort(best, kind="stable")
        sorted_lab = best[order]
        starts = np.r_[0, np.flatnonzero(np.diff(sorted_lab)) + 1]
        group_start = np.repeat(starts, np.diff(np.r_[starts, best.size]))
        rank = np.empty(best.size, np.int64)
        rank[order] = np.arange(best.size) - group_start
        best = best[rank >= k[best]]
    if best.size == 0:
        return []
    keep = np.r_[True, best[1:] != best[:-1]]
    return [int(v) for v in best[keep]]


def greedy_decode(pred_out, thr, skip=2, dev=None):
    best, prob = frame_argmax(pred_out, skip, dev)
    return [confidence_filter_collapse(best[j], prob[j], thr) for j in range(best.shape[0])]


def greedy_decode_argmax(best, prob, thr):
    """The same from per-frame (best label, its probability) arrays - what Model.predict_generator(decode="argmax") returns
    straight from the device, without the (N, T, C) posteriors crossing PCIe."""
    best, prob = np.asarray(best), np.asarray(prob)
    return [confidence_filter_collapse(best[j], prob[j], thr) for j in range(best.shape[0])]


# HTK label times are in 100 ns units.  One network frame is 50 ms in every modality: the skeletal stream is Kinect's 20 frames / s, and
# the audio stream is 10 ms MFCC frames of which every data_generator of the reference takes every fifth (iloc[::5]).
FRAME_PERIOD_HTK = 500000


def write_mlf(path, decoded_names, f_list, ignore_list, name_fmt="Sample%05d", segments=None, frame_period=FRAME_PERIOD_HTK):
    """HTK master label file in the reference's layout (sequence_decoding.py:35-36,57-65).
    segments (optional): per sample one (label, first_frame, last_frame, confidence) tuple per name - what greedy_segments /
    forced_align return; each line then reads "start end name" in HTK's 100 ns units, start = first_frame * frame_period and end =
    (last_frame + 1) * frame_period (the end of the last frame).  Without segments the file is the reference's, byte for byte."""
    with open(path, "w") as of:
        of.write("#!MLF!#\n")
        for j, (names, f_num) in enumerate(zip(decoded_names, f_list)):
            if int(f_num) in ignore_list:
                continue
            of.write('"*/%s.rec"\n' % (name_fmt % int(f_num)))
            if segments is None:
                for cl in names:
                    of.write("%s\n" % cl)
            else:
                if len(segments[j]) != len(names):
                    raise ValueError("sample %d: %d segments for %d names" % (j, len(segments[j]), len(names)))
                for cl, sg in zip(names, segments[j]):
                    of.write("%d %d %s\n" % (int(sg[1]) * int(frame_period), (int(sg[2]) + 1) * int(frame_period), cl))
            of.write(".\n")


def greedy_segments(pred_out, thr, skip=2, dev=None, max_segments=256):
    """greedy_decode with the frame positions it discards, all on the GPU (mgr_greedy_segments): per sample a list of
    (label, first_frame, last_frame, confidence) - the run's label (blanks kept), the indices in the ORIGINAL sequence (t + skip) of its
    first and last surviving frame, and the mean of the frame maxima over its surviving frames.  The labels are those of
    greedy_decode(pred_out, thr, skip).  max_segments sizes the first download; a sample with more runs (the device always reports the
    true count) makes the call run again with room for T - skip."""
    dev = dev or default_device()
    P = np.ascontiguousarray(pred_out, dtype=np.float32)
    N, T, Cn = P.shape
    dP = dev.array(P)
    dn = dev.empty((N,), np.int32)
    try:
        cap = max(1, min(T - skip, int(max_segments)))
        while True:
            dl, ds, dc = dev.empty((N, cap), np.int32), dev.empty((N, cap, 2), np.int32), dev.empty((N, cap), np.float32)
            dev.call("mgr_greedy_segments", dP, N, T, Cn, skip, C.c_float(-1.0 if thr is None else float(thr)), cap, dn, dl, ds, dc)
            n = dn.download()
            if int(n.max()) <= cap:
                lab, seg, conf = dl.download(), ds.download(), dc.download()
            for a in (dl, ds, dc):
                a.free()
            if int(n.max()) <= cap:
                break
            cap = T - skip
    finally:
        dP.free()
        dn.free()
    return segments_from_arrays(n, lab, seg, conf)


def segments_from_arrays(n, lab, seg, conf):
    """The (count, label, [first, last], confidence) arrays of mgr_greedy_segments -> per sample a list of tuples.  Raises when a
    sample has more runs than the arrays hold."""
    cap = lab.shape[1]
    if len(n) and int(np.max(n)) > cap:
        raise OverflowError("a sample has %d runs, the output holds %d per sample" % (int(np.max(n)), cap))
    return [[(int(lab[b, r]), int(seg[b, r, 0]), int(seg[b, r, 1]), float(conf[b, r])) for r in range(int(n[b]))] for b in range(len(n))]


def pack_labels(labels, label_length=None):
    """A padded array (-1 or NaN padding, as the generators' the_labels) or a list of label lists -> (int32 (N, Lmax) padded -1,
    int32 (N,) lengths)."""
    if isinstance(labels, np.ndarray) or (len(labels) and np.ndim(labels[0]) == 0):
        lab = np.atleast_2d(np.asarray(labels, dtype=np.float64))
        lab = np.where(np.isfinite(lab) & (lab >= 0), lab, -1).astype(np.int32)
    else:
        Lmax = max([len(r) for r in labels] + [1])
        lab = -np.ones((len(labels), Lmax), np.int32)
        for i, r in enumerate(labels):
            lab[i, :len(r)] = np.asarray(r, np.int32)
    if lab.shape[1] == 0:
        lab = -np.ones((lab.shape[0], 1), np.int32)
    ll = (lab >= 0).sum(axis=1).astype(np.int32) if label_length is None else np.asarray(label_length).reshape(-1).astype(np.int32)
    return np.ascontiguousarray(lab), ll


def alignment_from_arrays(lab, ll, seg, conf, logp):
    """mgr_ctc_align's seg / conf arrays -> per sample a list of (label, first_frame, last_frame, confidence); a sample whose
    labels do not fit its input (logp = -inf) has no segments."""
    out = []
    for b in range(lab.shape[0]):
        n = 0 if not np.isfinite(logp[b]) else min(int(ll[b]), lab.shape[1])
        out.append([(int(lab[b, k]), int(seg[b, k, 0]), int(seg[b, k, 1]), float(conf[b, k])) for k in range(n)])
    return out


def forced_align(pred_out, labels, label_length=None, input_length=None, skip=2, dev=None, return_path=False, eps=1e-8):
    """Viterbi forced alignment on the GPU (mgr_ctc_align): the single most probable CTC alignment of each sample's label sequence to
    its posteriors, under the loss's conventions (frames skip .., y = softmax(log(P + eps)), blank = C - 1).
    Returns (segments, logp[, path]): per sample a list of (label, first_frame, last_frame, confidence) - the frames, as indices of the
    ORIGINAL sequence, at which the path emits the label, and the mean of P[t, label] over them; logp (N,) float64, the natural-log
    probability of the path (-inf and no segments where the labels do not fit the input length); path (N, T - skip) int32, the class
    emitted at every frame (-1 past the input length).  A CTC-trained network emits short spikes: the frames are where the network
    commits to the gesture, not the extent of the movement."""
    dev = dev or default_device()
    P = np.ascontiguousarray(pred_out, dtype=np.float32)
    N, T, Cn = P.shape
    lab, ll = pack_labels(labels, label_length)
    if lab.shape[0] != N:
        raise ValueError("%d label rows for %d samples" % (lab.shape[0], N))
    il = np.full(N, T - skip, np.int32) if input_length is None else np.asarray(input_length).reshape(N).astype(np.int32)
    Lmax = lab.shape[1]
    dP, dlab, dil, dll = dev.array(P), dev.array(lab), dev.array(il), dev.array(ll)
    dpath, dseg = dev.empty((N, T - skip), np.int32), dev.empty((N, Lmax, 2), np.int32)
    dconf, dlogp = dev.empty((N, Lmax), np.float32), dev.empty((N,), np.float64)
    ws = dev.bytes(dev.lib.mgr_ctc_align_ws_bytes(N, T, Cn, Lmax))
    try:
        dev.call("mgr_ctc_align", dP, dlab, dil, dll, N, T, Cn, Lmax, skip, Cn - 1, C.c_float(eps), dpath, dseg, dconf, dlogp, ws, ws.nbytes)
        seg, conf, logp = dseg.download(), dconf.download(), dlogp.download()
        path = dpath.download() if return_path else None
    finally:
        for a in (dP, dlab, dil, dll, dpath, dseg, dconf, dlogp, ws):
            a.free()
    clipped = np.clip(lab, 0, Cn - 1)     # (what the kernels align: out-of-range values clipped into the class range, as the loss)
    segs = alignment_from_arrays(clipped, ll, seg, conf, logp)
    return (segs, logp, path) if return_path else (segs, logp)


def beam_search_decode(pred_out, input_length=None, beam_width=10, skip=2, merge_repeated=True, dev=None):
    """K.ctc_decode(greedy=False, beam_width) equivalent on the GPU (BASELINE.json config 5)."""
    dev = dev or default_device()
    P = np.ascontiguousarray(pred_out, dtype=np.float32)
    N, T, Cn = P.shape
    if input_length is None:
        input_length = np.full(N, T - skip)
    il = np.asarray(input_length).reshape(N).astype(np.int32)
    dP, dil = dev.array(P), dev.array(il)
    out = dev.empty((N, T - skip), np.int32)
    olen = dev.empty((N,), np.int32)
    logp = dev.empty((N,), np.float64)
    ws = dev.bytes(dev.lib.mgr_ctc_beam_ws_bytes(N, T, Cn, beam_width))
    dev.call("mgr_ctc_beam_search", dP, dil, N, T, Cn, skip, Cn - 1, int(beam_width), C.c_float(1e-8),
             1 if merge_repeated else 0, out, olen, logp, ws, ws.nbytes)
    o, l, s = out.download(), olen.download(), logp.download()
    for a in (dP, dil, out, olen, logp, ws):
        a.free()
    return [[int(v) for v in o[i, :l[i]]] for i in range(N)], s


def bigram_lm(label_seqs, n_classes, blank=None, add_k=1.0):
    """A bigram over labels from counts (host, numpy): label_seqs is whatever pack_labels takes - an iterable of label lists or a
    padded array.  Returns (lm (C + 1, C) float64, lm_end (C + 1,) float64), natural-log conditional probabilities: lm[p + 1, c] =
    log p(c | previous label p), row 0 = start of sequence, lm_end[p + 1] = log p(end | p) - "end of sequence" is one more outcome of
    every row.  Smoothing is add-k over the non-blank classes plus end; the blank never follows anything (its column is -inf, and the
    decoder never reads it).  With add_k = 0 unseen transitions are -inf - a hard grammar - and a row without counts is all -inf."""
    Cn = int(n_classes)
    blank = Cn - 1 if blank is None else int(blank)
    label_seqs = label_seqs if isinstance(label_seqs, np.ndarray) else list(label_seqs)
    counts, ends = np.zeros((Cn + 1, Cn), np.float64), np.zeros(Cn + 1, np.float64)
    if len(label_seqs):
        lab, _ = pack_labels(label_seqs)
        for row in lab:
            prev = 0
            for v in row[row >= 0]:
                if v >= Cn or v == blank:
                    raise ValueError("label %d is not one of the %d non-blank classes" % (int(v), Cn - 1))
                counts[prev, v] += 1.0
                prev = int(v) + 1
            ends[prev] += 1.0
    k = float(add_k)
    smooth = np.full(Cn, k)
    smooth[blank] = 0.0
    num, num_end = counts + smooth, ends + k
    den = num.sum(axis=1) + num_end
    with np.errstate(divide="ignore", invalid="ignore"):
        lm = np.where(num > 0, np.log(num / den[:, None]), -np.inf)
        lm_end = np.where(num_end > 0, np.log(num_end / den), -np.inf)
    return lm, lm_end


def lm_tables(n_classes, lm=None, lm_end=None, alpha=1.0, beta=0.0):
    """The two tables mgr_ctc_beam_search_lm reads, in fp64: ext (C + 1, C) = alpha * lm + beta (lm=None: zeros) and fin (C + 1,) =
    alpha * lm_end, or None.  -inf stays -inf whatever alpha is; NaN and +inf are refused here - the kernel reads device memory and
    cannot say so."""
    Cn = int(n_classes)

    def scaled(t, shape, shift, what):
        t = np.asarray(t, np.float64)
        if t.shape != shape:
            raise ValueError("%s has shape %s, the decoder needs %s" % (what, t.shape, shape))
        if np.isnan(t).any() or np.isposinf(t).any():
            raise ValueError("%s holds NaN or +inf: entries must be finite or -inf" % what)
        ninf = np.isneginf(t)
        out = np.where(ninf, -np.inf, float(alpha) * np.where(ninf, 0.0, t) + shift)
        if not np.all(np.isfinite(out) | ninf):
            raise ValueError("alpha / beta make %s NaN or infinite" % what)
        return np.ascontiguousarray(out)

    ext = scaled(np.zeros((Cn + 1, Cn)) if lm is None else lm, (Cn + 1, Cn), float(beta), "lm")
    fin = None if lm_end is None else scaled(lm_end, (Cn + 1,), 0.0, "lm_end")
    return ext, fin


def nbest_from_arrays(out, out_len, score, logp_ctc, top_paths):
    """mgr_ctc_beam_search_lm's arrays ((B, top_paths, T - skip), (B, top_paths) x 3) -> (paths, score, logp_ctc).  top_paths = 1:
    the shapes beam_search_decode returns (a label list per sample, (B,) arrays); otherwise per sample the ranked list of its
    surviving hypotheses (at most top_paths) and (B, top_paths) arrays with -inf where there is none."""
    B = out.shape[0]
    paths = [[[int(v) for v in out[b, k, :out_len[b, k]]] for k in range(top_paths) if out_len[b, k] >= 0] for b in range(B)]
    if top_paths == 1:
        return [p[0] if p else [] for p in paths], score[:, 0].copy(), logp_ctc[:, 0].copy()
    return paths, score.copy(), logp_ctc.copy()


def beam_search_lm_decode(pred_out, lm=None, lm_end=None, alpha=1.0, beta=0.0, input_length=None, beam_width=10, top_paths=1, skip=2,
                          dev=None):
    """CTC prefix beam search with a label bigram and an N-best list on the GPU (mgr_ctc_beam_search_lm): beam_search_decode
    (merge_repeated=False) in which a hypothesis ranks by log p_ctc + alpha * (sum of lm over its label pairs) + beta * (its length),
    plus alpha * lm_end[last label + 1] once at the end (no part in the pruning).  lm (C + 1, C), lm_end (C + 1,) as bigram_lm returns
    them; -inf entries forbid a transition.  Returns (paths, score, logp_ctc): with top_paths = 1 a label list per sample and two (N,)
    float64 arrays - the ranking score and the network's part of it -, otherwise per sample the ranked list of its at most top_paths
    hypotheses and (N, top_paths) arrays, -inf where fewer survive."""
    dev = dev or default_device()
    P = np.ascontiguousarray(pred_out, dtype=np.float32)
    N, T, Cn = P.shape
    ext, fin = lm_tables(Cn, lm, lm_end, alpha, beta)
    W, NP = int(beam_width), int(top_paths)
    il = np.full(N, T - skip, np.int32) if input_length is None else np.asarray(input_length).reshape(N).astype(np.int32)
    bufs = [dev.array(P), dev.array(il), dev.array(ext)]
    try:
        if fin is not None:
            bufs.append(dev.array(fin))
        dfin = bufs[3] if fin is not None else None
        out, olen = dev.empty((N, NP, T - skip), np.int32), dev.empty((N, NP), np.int32)
        score, logp = dev.empty((N, NP), np.float64), dev.empty((N, NP), np.float64)
        bufs += [out, olen, score, logp]
        ws = dev.bytes(dev.lib.mgr_ctc_beam_lm_ws_bytes(N, T, Cn, W, NP))
        bufs.append(ws)
        dev.call("mgr_ctc_beam_search_lm", bufs[0], bufs[1], N, T, Cn, skip, Cn - 1, W, C.c_float(1e-8), bufs[2], dfin, NP, out, olen,
                 score, logp, ws, ws.nbytes)
        res = nbest_from_arrays(out.download(), olen.download(), score.download(), logp.download(), NP)
    finally:
        for a in bufs:
            a.free()
    return res


def decode_beam_mlf(pred_out, f_list, map_gest, ignore_list, name_fmt, out_file, top_paths=1, **kwargs):
    """What the networks' decode_beam share: pred_out (N, T, C) softmax - decoded with beam_search_lm_decode(**kwargs) - or the
    (paths, score, logp_ctc) that Model.predict_generator(decode="beam_lm", top_paths=top_paths) computed on the device.  The 1-best
    path of every sample goes through the class map into the unchanged write_mlf; returns (1-best name lists, (paths, score,
    logp_ctc))."""
    nbest = pred_out if isinstance(pred_out, tuple) else beam_search_lm_decode(np.asarray(pred_out), top_paths=top_paths, **kwargs)
    best = nbest[0] if np.ndim(nbest[1]) == 1 else [p[0] if p else [] for p in nbest[0]]      # ((N,) scores: one path per sample)
    ret = [[map_gest[i] for i in seq] for seq in best]
    if out_file is not None:
        write_mlf(out_file, ret, f_list, ignore_list, name_fmt)
    return ret, nbest


def edit_distance(a, b):
    la, lb = len(a), len(b)
    d = list(range(lb + 1))
    for i in range(1, la + 1):
        prev, d[0] = d[0], i
        for j in range(1, lb + 1):
            cur = d[j]
            d[j] = min(d[j] + 1, d[j - 1] + 1, prev + (a[i - 1] != b[j - 1]))
            prev = cur
    return d[lb]


def label_error_rate(hyps, refs):
    """sum of edit distances / sum of reference lengths (what HTK HResults reports as 100 - Acc)."""
    num = sum(edit_distance(h, r) for h, r in zip(hyps, refs))
    den = sum(len(r) for r in refs)
    return num / max(1, den)


def read_mlf(path):
    """HTK master label file -> {sample name: [labels]} (the layout write_mlf produces: '"*/Sample00001.rec"' lines,
    one label per line, '.' terminator).  '.lab' and '.rec' entries are keyed by the bare sample name."""
    out, cur = {}, None
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line == "#!MLF!#":
                continue
            if line.startswith('"'):
                name = line.strip('"').split("/")[-1]
                cur = out.setdefault(name.rsplit(".", 1)[0], [])
            elif line == ".":
                cur = None
            elif cur is not None:
                cur.append(line.split()[-1] if len(line.split()) > 1 and line.split()[0].isdigit() else line.split()[0])
    return out


def score_mlf(ref_path, rec_path, ignore=("sil",)):
    """Label error rate of a recognition MLF against a reference MLF, over the samples present in both
    (HResults-style: (S + D + I) / N after removing the `ignore` labels).  Returns (ler, n_samples)."""
    ref, rec = read_mlf(ref_path), read_mlf(rec_path)
    names = sorted(set(ref) & set(rec))
    strip = lambda seq: [x for x in seq if x not in ignore]
    return label_error_rate([strip(rec[n]) for n in names], [strip(ref[n]) for n in names]), len(names)
