"""Decode helpers shared by the three sequence_decoding modules (K9).

Frame-wise max / argmax runs on the GPU (mgr_frame_argmax); the reference's confidence filter and the
repeat collapse run on the host (greedy_decode) or, with the frame positions kept, on the GPU (greedy_segments).  The filter reproduces the NET EFFECT of the reference's Python-2 loop
(multimodal_fusion/sequence_decoding.py:45-48: ``list.remove`` deletes the first element equal to the value,
not the visited one): for every label s, the first k_s occurrences of s are dropped, where k_s is the number
of frames whose best label is s with probability below the threshold.  Blanks are kept (they decode to "sil").
"""
import collections
import ctypes as C

import numpy as np

from . import _capi

_DEV = [None]


def default_device():
    if _DEV[0] is None:
        _DEV[0] = _capi.Device(0)
    return _DEV[0]


# ---- one description per device decode: what the host wrappers below and Engine.predict_stream both read --------------
DecodeOp = collections.namedtuple("DecodeOp", "name outputs launch result tables ws_bytes hyp uses_len", defaults=((), None, None, False))
DecodeOp.__doc__ = """What there is to know about one decode kernel with its parameters set (built by the *_op factories, which validate):
  outputs   (N, T, Lmax=None) -> one (shape, dtype) per device output, in the kernel's order; None = not asked for (null pointer)
  launch    (dev, P, input_len, outs, tables, ws[, labels, label_len]): the one place the entry point's argument list is written;
            arguments that are HOST memory (the lexicon's phrase_off / phrase_words) are kept by the op
  result    (the outputs that are not None, as host arrays[, labels, label_len]) -> what the public function returns; it may hand an
            array through as it came (Engine.predict_stream, which passes pinned buffers it reuses, copies every array it gets back)
  tables    host arrays to upload once, in the kernel's order; None = absent, the kernel gets a null pointer
  ws_bytes  (lib, N, T, Lmax=None) -> bytes of workspace, or None: the kernel takes none
  hyp       (index of the output with the hypothesis labels [N, width] padded -1, index of their lengths), what mgr_edit_distance
            takes from it for output="score" - or None
  uses_len  whether the kernel reads input_len (launch gets None where it does not)
Buffers are cached under what sizes them: the op's name with these shapes and byte counts."""


def _i32(*shape):
    return shape, np.int32


def _f32(*shape):
    return shape, np.float32


def _f64(*shape):
    return shape, np.float64


def argmax_op(n_classes, skip):
    Cn = int(n_classes)

    def launch(dev, P, input_len, outs, tables, ws):
        dev.call("mgr_frame_argmax", P, P.shape[0], P.shape[1], Cn, skip, *outs)
    return DecodeOp("argmax", lambda N, T, Lmax=None: (_i32(N, T - skip), _f32(N, T - skip)), launch, lambda best, prob: (best, prob))


def segments_op(n_classes, skip, threshold, cap):
    Cn, thr, cap = int(n_classes), C.c_float(-1.0 if threshold is None else float(threshold)), int(cap)

    def launch(dev, P, input_len, outs, tables, ws):
        dev.call("mgr_greedy_segments", P, P.shape[0], P.shape[1], Cn, skip, thr, cap, *outs)
    return DecodeOp("segments", lambda N, T, Lmax=None: (_i32(N), _i32(N, cap), _i32(N, cap, 2), _f32(N, cap)), launch,
                    segments_from_arrays, hyp=(1, 0))


def beam_op(n_classes, skip, beam_width=10, merge_repeated=True, blank=None, eps=1e-8):
    Cn, W = int(n_classes), int(beam_width)
    blank = Cn - 1 if blank is None else int(blank)

    def launch(dev, P, input_len, outs, tables, ws):
        dev.call("mgr_ctc_beam_search", P, input_len, P.shape[0], P.shape[1], Cn, skip, blank, W, C.c_float(eps),
                 1 if merge_repeated else 0, *outs, ws, ws.nbytes)

    def result(out, out_len, logp):
        return [[int(v) for v in out[i, :out_len[i]]] for i in range(len(out_len))], logp
    return DecodeOp("beam", lambda N, T, Lmax=None: (_i32(N, T - skip), _i32(N), _f64(N)), launch, result,
                    ws_bytes=lambda lib, N, T, Lmax=None: lib.mgr_ctc_beam_ws_bytes(N, T, Cn, W), hyp=(0, 1), uses_len=True)


def beam_lm_op(n_classes, skip, lm=None, lm_end=None, alpha=1.0, beta=0.0, beam_width=10, top_paths=1, eps=1e-8):
    Cn, W, NP = int(n_classes), int(beam_width), int(top_paths)

    def launch(dev, P, input_len, outs, tables, ws):
        dev.call("mgr_ctc_beam_search_lm", P, input_len, P.shape[0], P.shape[1], Cn, skip, Cn - 1, W, C.c_float(eps), tables[0], tables[1],
                 NP, *outs, ws, ws.nbytes)
    return DecodeOp("beam_lm", lambda N, T, Lmax=None: (_i32(N, NP, T - skip), _i32(N, NP), _f64(N, NP), _f64(N, NP)), launch,
                    lambda *arrays: nbest_from_arrays(*arrays, NP), tables=lm_tables(Cn, lm, lm_end, alpha, beta),
                    ws_bytes=lambda lib, N, T, Lmax=None: lib.mgr_ctc_beam_lm_ws_bytes(N, T, Cn, W, NP),
                    hyp=(0, 1), uses_len=True)         # (a length of -1 - no hypothesis - counts as 0 in mgr_edit_distance)


def sample_op(n_classes, skip, draws, seed, return_path=False, eps=1e-8):
    """mgr_ctc_sample_paths (K16): `draws` frame paths per sample, collapsed, merged and counted.  launch takes one more keyword,
    seed=: a caller that draws again for every batch (Engine.predict_stream) passes it there, the op's own seed is the default."""
    Cn, K, seed0 = int(n_classes), int(draws), int(seed) & (2 ** 64 - 1)
    if not 2 <= Cn <= SAMPLE_MAX_CLASSES or not 1 <= K <= SAMPLE_MAX_DRAWS:
        raise ValueError("n_classes = %d (2 .. %d) / draws = %d (1 .. %d)" % (Cn, SAMPLE_MAX_CLASSES, K, SAMPLE_MAX_DRAWS))

    def outputs(N, T, Lmax=None):
        return (_i32(N, K, T - skip), _i32(N, K), _i32(N, K), _i32(N), _i32(N, K, T - skip) if return_path else None)

    def launch(dev, P, input_len, outs, tables, ws, seed=None):
        dev.call("mgr_ctc_sample_paths", P, input_len, P.shape[0], P.shape[1], Cn, skip, Cn - 1, C.c_float(eps),
                 C.c_uint64(seed0 if seed is None else int(seed) & (2 ** 64 - 1)), K, *outs)

    def result(out, out_len, count, n_unique, *path):
        return samples_from_arrays(out, out_len, count) + path
    return DecodeOp("sample", outputs, launch, result, hyp=(0, 1), uses_len=True)


def lexicon_op(n_classes, skip, lexicon, lm=None, lm_end=None, alpha=1.0, beta=0.0, cap=256, return_path=False, eps=1e-8):
    Cn, cap = int(n_classes), int(cap)
    off, words = compile_lexicon(lexicon, Cn)        # (host arrays: the library reads and checks them at every call)
    G = len(off) - 1

    def outputs(N, T, Lmax=None):
        return (_i32(N), _i32(N, cap), _i32(N, cap, 2), _f32(N, cap), _i32(N, T - skip) if return_path else None, _f64(N), _f64(N))

    def launch(dev, P, input_len, outs, tables, ws):
        dev.call("mgr_ctc_lexicon_decode", P, input_len, P.shape[0], P.shape[1], Cn, skip, Cn - 1, C.c_float(eps), off.ctypes.data,
                 words.ctypes.data, G, tables[0], tables[1], cap, *outs, ws, ws.nbytes)

    def result(n, phr, seg, conf, *rest):           # (rest: [path, ]score, logp)
        return (lexicon_from_arrays(n, phr, seg, conf), rest[-2], rest[-1]) + rest[:-2]
    return DecodeOp("lexicon", outputs, launch, result, tables=phrase_lm_tables(G, lm, lm_end, alpha, beta),
                    ws_bytes=lambda lib, N, T, Lmax=None: lib.mgr_ctc_lexicon_ws_bytes(N, T, Cn, G, off.ctypes.data), uses_len=True)


def align_op(n_classes, skip, return_path=False, eps=1e-8):
    Cn = int(n_classes)

    def launch(dev, P, input_len, outs, tables, ws, labels, label_len):
        dev.call("mgr_ctc_align", P, labels, input_len, label_len, P.shape[0], P.shape[1], Cn, labels.shape[1], skip, Cn - 1, C.c_float(eps),
                 *outs, ws, ws.nbytes)

    def result(path, seg, conf, logp, lab, ll):
        clipped = np.clip(lab, 0, Cn - 1)     # (what the kernels align: out-of-range values clipped into the class range, as the loss)
        return (alignment_from_arrays(clipped, ll, seg, conf, logp), logp) + ((path,) if return_path else ())
    return DecodeOp("align", lambda N, T, Lmax: (_i32(N, T - skip), _i32(N, Lmax, 2), _f32(N, Lmax), _f64(N)), launch, result,
                    ws_bytes=lambda lib, N, T, Lmax: lib.mgr_ctc_align_ws_bytes(N, T, Cn, Lmax), uses_len=True)


def occupancy_op(n_classes, skip, quantile=0.5, return_gamma=False, eps=1e-8):
    """mgr_ctc_occupancy (K17): state posteriors and quantile extents of given labels; it runs in the loss's workspace."""
    Cn, q = int(n_classes), float(quantile)
    if not 0.0 < q <= 0.5:
        raise ValueError("quantile %r is not in (0, 0.5]" % (quantile,))

    def outputs(N, T, Lmax):
        return (_f32(N, T - skip, 2 * Lmax + 1) if return_gamma else None, _i32(N, Lmax, 2), _f32(N, Lmax), _f32(N, Lmax), _f64(N))

    def launch(dev, P, input_len, outs, tables, ws, labels, label_len):
        dev.call("mgr_ctc_occupancy", P, labels, input_len, label_len, P.shape[0], P.shape[1], Cn, labels.shape[1], skip, Cn - 1, C.c_float(eps),
                 C.c_float(q), *outs, ws, ws.nbytes)

    def result(*arrays):
        lab, ll = arrays[-2:]
        seg, occ, conf, logp = arrays[-6:-2]
        clipped = np.clip(lab, 0, Cn - 1)     # (what the kernels align: out-of-range values clipped into the class range, as the loss)
        return (extents_from_arrays(clipped, ll, seg, conf, occ, logp), logp) + ((arrays[0],) if return_gamma else ())
    return DecodeOp("occupancy", outputs, launch, result, ws_bytes=lambda lib, N, T, Lmax: lib.mgr_ctc_ws_bytes(N, T, Cn, Lmax), uses_len=True)


def entropy_op(n_classes, skip, grad=False, eps=1e-8):
    """mgr_ctc_entropy_grad as a measurement: the entropy of the labels' alignments and logp, with grad also dH/dlogits
    (loss_scale 0, ent_scale -1: the call writes loss_scale dloss - ent_scale dH).  Its workspace is twice the loss's."""
    Cn = int(n_classes)

    def outputs(N, T, Lmax):
        return (_f32(N), _f32(N), _f32(N, T, Cn) if grad else None)

    def launch(dev, P, input_len, outs, tables, ws, labels, label_len):
        dev.call("mgr_ctc_entropy_grad", P, labels, input_len, label_len, P.shape[0], P.shape[1], Cn, labels.shape[1], skip, Cn - 1,
                 C.c_float(eps), C.c_float(0.0), C.c_float(-1.0), *outs, ws, ws.nbytes)

    def result(*arrays):
        loss, H = arrays[0], arrays[1]
        return (H, -loss.astype(np.float64)) + ((arrays[2],) if grad else ())
    return DecodeOp("entropy", outputs, launch, result, ws_bytes=lambda lib, N, T, Lmax: 2 * lib.mgr_ctc_ws_bytes(N, T, Cn, Lmax), uses_len=True)


def rescore_op(n_classes, skip, lexicon=None, eps=1e-8):
    """mgr_ctc_rescore (K14): the hypothesis arrays (hyp (N, K, Lh), hyp_len (N, K)) travel where align passes its labels, so the
    `Lmax` the description's functions get is K."""
    Cn = int(n_classes)
    off, words = compile_lexicon(lexicon, Cn) if lexicon is not None else (None, None)     # (host arrays, checked again at every call)
    G = 0 if off is None else len(off) - 1
    host = lambda a: None if a is None else a.ctypes.data

    def launch(dev, P, input_len, outs, tables, ws, hyp, hyp_len):
        dev.call("mgr_ctc_rescore", P, input_len, P.shape[0], P.shape[1], Cn, skip, Cn - 1, C.c_float(eps), host(off), host(words), G,
                 hyp, hyp_len, hyp.shape[1], hyp.shape[2], *outs, ws, ws.nbytes)
    return DecodeOp("rescore", lambda N, T, K: (_f64(N, K), _i32(N, K)), launch, lambda logp, n_lab, hyp, hyp_len: (logp, n_lab),
                    ws_bytes=lambda lib, N, T, K=None: lib.mgr_ctc_rescore_ws_bytes(N, T, Cn, G, host(off)), uses_len=True)


def _posteriors(pred_out):
    return np.ascontiguousarray(pred_out, dtype=np.float32)


def _run(op, P, skip, dev, input_length=None, labels=()):
    """One decode op on host posteriors P (N, T, C) float32: upload, allocate what the description says, launch, download, shape -
    and free all of it, whatever happens.  labels: () or the (labels (N, Lmax), lengths (N,)) of pack_labels."""
    dev = dev or default_device()
    N, T = P.shape[:2]
    Lmax = labels[0].shape[1] if labels else None
    held = []

    def keep(a):
        held.append(a)
        return a
    try:
        dP, dil = keep(dev.array(P)), None
        if op.uses_len:
            dil = keep(dev.array(np.full(N, T - skip, np.int32) if input_length is None else np.asarray(input_length).reshape(N).astype(np.int32)))
        dlab = [keep(dev.array(a)) for a in labels]
        tables = [t if t is None else keep(dev.array(t)) for t in op.tables]
        outs = [o if o is None else keep(dev.empty(*o)) for o in op.outputs(N, T, Lmax)]
        ws = keep(dev.bytes(op.ws_bytes(dev.lib, N, T, Lmax))) if op.ws_bytes else None
        op.launch(dev, dP, dil, outs, tables, ws, *dlab)
        return op.result(*[o.download() for o in outs if o is not None], *labels)
    finally:
        for a in held:
            a.free()


def _run_with_room(make_op, first, P, skip, dev, **kwargs):
    """_run of make_op(cap) with room for `first` entries per sample, and again with room for T - skip - the most there can be - when a
    sample has more: the device always reports the true count, and the op's *_from_arrays refuses it with OverflowError (any OverflowError
    out of _run is taken for that one; what the second run raises is raised).  The second run is a whole _run - P uploaded, the lexicon
    compiled, every buffer allocated again: more than reallocating the outputs would cost, but rare (more than `first` in a sample)."""
    room = P.shape[1] - skip
    cap = max(1, min(room, int(first)))
    try:
        return _run(make_op(cap), P, skip, dev, **kwargs)
    except OverflowError:
        if cap >= room:
            raise
        return _run(make_op(room), P, skip, dev, **kwargs)


def frame_argmax(pred_out, skip=2, dev=None):
    """(N,T,C) float32 softmax -> best (N,T-skip) int32, prob (N,T-skip) float32, computed on the GPU."""
    P = _posteriors(pred_out)
    return _run(argmax_op(P.shape[2], skip), P, skip, dev)


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
    P = _posteriors(pred_out)
    return _run_with_room(lambda cap: segments_op(P.shape[2], skip, thr, cap), max_segments, P, skip, dev)


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
    P = _posteriors(pred_out)
    lab, ll = pack_labels(labels, label_length)
    if lab.shape[0] != P.shape[0]:
        raise ValueError("%d label rows for %d samples" % (lab.shape[0], P.shape[0]))
    return _run(align_op(P.shape[2], skip, return_path, eps), P, skip, dev, input_length, (lab, ll))


def extents_from_arrays(lab, ll, seg, conf, occ, logp):
    """mgr_ctc_occupancy's seg / conf / occ arrays -> per sample a list of (label, first_frame, last_frame, confidence, occupancy); a
    sample whose labels do not fit its input (logp = -inf) has no segments."""
    out = []
    for b in range(lab.shape[0]):
        n = 0 if not np.isfinite(logp[b]) else min(int(ll[b]), lab.shape[1])
        out.append([(int(lab[b, k]), int(seg[b, k, 0]), int(seg[b, k, 1]), float(conf[b, k]), float(occ[b, k])) for k in range(n)])
    return out


def posterior_align(pred_out, labels, label_length=None, input_length=None, quantile=0.5, skip=2, dev=None, return_gamma=False, eps=1e-8):
    """Posterior extents on the GPU (mgr_ctc_occupancy): where forced_align reports the frames of the single best alignment, this weighs
    every CTC alignment of the labels.  gamma(t, s) is the posterior of lattice state s (l' = [blank, l_1, blank, ..., l_L, blank]) at
    frame t; label i's extent runs from the first frame at which it has begun with probability >= quantile to the last frame at which it
    has not ended with probability >= quantile.  quantile = 0.5 is the median extent, a smaller one a wider credible extent (neighbouring
    extents may then overlap); first <= last and the firsts increase for every quantile in (0, 0.5].
    Returns (segments, logp[, gamma]): per sample a list of (label, first_frame, last_frame, confidence, occupancy) - frames as indices
    of the ORIGINAL sequence, inclusive; confidence the posterior-weighted mean of P[t, label]; occupancy the expected number of frames
    spent in the label -, logp (N,) float64 = -loss (-inf and no segments where the labels do not fit), gamma (N, T - skip, 2 Lmax + 1)
    float32.  A CTC network's posteriors stay peaky: the median extent sits near the Viterbi spikes, smaller quantiles widen it."""
    P = _posteriors(pred_out)
    lab, ll = pack_labels(labels, label_length)
    if lab.shape[0] != P.shape[0]:
        raise ValueError("%d label rows for %d samples" % (lab.shape[0], P.shape[0]))
    return _run(occupancy_op(P.shape[2], skip, quantile, return_gamma, eps), P, skip, dev, input_length, (lab, ll))


def alignment_entropy(pred_out, labels, label_length=None, input_length=None, skip=2, eps=1e-8, grad=False, dev=None):
    """The entropy of the distribution over the CTC alignments of each sample's labels, on the GPU (mgr_ctc_entropy_grad):
    H = - sum_pi q(pi) ln q(pi) in nats, q(pi) = p(pi) / p(labels | posteriors) over the feasible alignments pi, under the loss's
    conventions (frames skip .., y = softmax(log(P + eps)), blank = C - 1).  It is the quantity entropy-regularised CTC training
    (Engine.set_entropy) raises, and a per-sample measure of how far posterior_align's extents can be trusted: H near 0 means one
    alignment holds all of p(labels | x) - the posteriors are peaky and every quantile gives the Viterbi spikes -, a larger H that the
    extents average over alignments that really differ.
    Returns (H, logp[, dH/dlogits]): H (N,) float32 (0 without labels, and where the labels do not fit), logp (N,) float64 = -loss
    (-inf where they do not fit), dH/dlogits (N, T, C) float32 with respect to the logits behind the posteriors (grad=True; zero on
    dropped and out-of-length frames)."""
    P = _posteriors(pred_out)
    lab, ll = pack_labels(labels, label_length)
    if lab.shape[0] != P.shape[0]:
        raise ValueError("%d label rows for %d samples" % (lab.shape[0], P.shape[0]))
    return _run(entropy_op(P.shape[2], skip, grad, eps), P, skip, dev, input_length, (lab, ll))


def beam_search_decode(pred_out, input_length=None, beam_width=10, skip=2, merge_repeated=True, dev=None, blank=None):
    """K.ctc_decode(greedy=False, beam_width) equivalent on the GPU (BASELINE.json config 5).  blank: the blank's class, the last
    one (Keras') by default."""
    P = _posteriors(pred_out)
    return _run(beam_op(P.shape[2], skip, beam_width, merge_repeated, blank), P, skip, dev, input_length)


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
    ext = _scaled_table(np.zeros((Cn + 1, Cn)) if lm is None else lm, (Cn + 1, Cn), alpha, float(beta), "lm")
    fin = None if lm_end is None else _scaled_table(lm_end, (Cn + 1,), alpha, 0.0, "lm_end")
    return ext, fin


def _scaled_table(t, shape, alpha, shift, what, f32_range=False):
    """alpha * t + shift in fp64 with -inf kept, or ValueError: a wrong shape, NaN, +inf, or a weight that makes an entry so.
    f32_range: also refuse a finite result beyond the float32 range (for a kernel that searches on the tables rounded to f32)."""
    t = np.asarray(t, np.float64)
    if t.shape != shape:
        raise ValueError("%s has shape %s, the decoder needs %s" % (what, t.shape, shape))
    if np.isnan(t).any() or np.isposinf(t).any():
        raise ValueError("%s holds NaN or +inf: entries must be finite or -inf" % what)
    ninf = np.isneginf(t)
    out = np.where(ninf, -np.inf, float(alpha) * np.where(ninf, 0.0, t) + shift)
    if not np.all(np.isfinite(out) | ninf):
        raise ValueError("alpha / beta make %s NaN or infinite" % what)
    if f32_range and np.any(np.abs(out[~ninf]) > np.finfo(np.float32).max):
        raise ValueError("%s holds a finite entry beyond the float32 range: the decoder searches on the table rounded to float32" % what)
    return np.ascontiguousarray(out)


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
    P = _posteriors(pred_out)
    return _run(beam_lm_op(P.shape[2], skip, lm, lm_end, alpha, beta, beam_width, top_paths), P, skip, dev, input_length)


# ---- lexicon-constrained decode (K13): phrase sequences from word posteriors -----------------------------------------
LEXICON_MAX_PHRASES, LEXICON_MAX_WORDS, LEXICON_MAX_CLASSES = 64, 255, 64       # MGR_LEXICON_MAX_* of include/mgr.h, and its C <= 64


def compile_lexicon(lexicon, n_classes, blank=None):
    """A phrase lexicon - a list of word lists, or a dict with the keys 0 .. G - 1 - in the layout mgr_ctc_lexicon_decode reads:
    (phrase_off (G + 1,) int32, phrase_words (n_words,) int32), phrase g = phrase_words[phrase_off[g]:phrase_off[g + 1]].  Refuses an
    empty lexicon or phrase, the blank (default: the last class) as a word, a word outside [0, n_classes) and a lexicon above the
    kernel's limits (64 phrases, 255 words, 64 classes).  Phrases may share words and need not be uniquely decodable."""
    Cn = int(n_classes)
    blank = Cn - 1 if blank is None else int(blank)
    if isinstance(lexicon, dict):
        if sorted(lexicon) != list(range(len(lexicon))):
            raise ValueError("a lexicon dict needs the keys 0 .. G - 1, got %r" % (sorted(lexicon),))
        lexicon = [lexicon[g] for g in range(len(lexicon))]
    lexicon = [[int(w) for w in p] for p in lexicon]
    if not 1 <= len(lexicon) <= LEXICON_MAX_PHRASES:
        raise ValueError("%d phrases: the decoder takes 1 .. %d" % (len(lexicon), LEXICON_MAX_PHRASES))
    if not 2 <= Cn <= LEXICON_MAX_CLASSES or not 0 <= blank < Cn:
        raise ValueError("n_classes = %d (2 .. %d) / blank = %d" % (Cn, LEXICON_MAX_CLASSES, blank))
    for g, p in enumerate(lexicon):
        if not p:
            raise ValueError("phrase %d is empty" % g)
        for w in p:
            if w == blank:
                raise ValueError("phrase %d holds the blank (%d) as a word" % (g, blank))
            if not 0 <= w < Cn:
                raise ValueError("phrase %d: word %d is outside [0, %d)" % (g, w, Cn))
    off = np.concatenate([[0], np.cumsum([len(p) for p in lexicon])]).astype(np.int32)
    if int(off[-1]) > LEXICON_MAX_WORDS:
        raise ValueError("%d words in the lexicon: the decoder takes %d" % (int(off[-1]), LEXICON_MAX_WORDS))
    return np.ascontiguousarray(off), np.ascontiguousarray(np.asarray([w for p in lexicon for w in p], np.int32))


def phrase_lm_tables(G, lm=None, lm_end=None, alpha=1.0, beta=0.0):
    """lm_tables for a prior over PHRASES - the two tables mgr_ctc_lexicon_decode reads, without a blank column: ext (G + 1, G) =
    alpha * lm + beta (lm=None: zeros; row 0 = start of sequence) and fin (G + 1,) = alpha * lm_end (index 0 = the empty sequence), or
    None.  -inf stays -inf; NaN, +inf and finite entries beyond the float32 range (the kernel searches on the tables rounded to
    float32: -1e300 would become "forbidden") are refused.  bigram_lm counts the right thing when the phrase ids stand in for its labels
    and one more id for its blank: lm, lm_end = bigram_lm(gesture_seqs, G + 1, blank=G) gives (G + 2, G + 1) / (G + 2,), of which the
    decoder's tables are lm[:G + 1, :G] and lm_end[:G + 1] (the last row is "after the blank", the last column the blank's: neither
    ever holds a count).  Pass those slices here."""
    G = int(G)
    if not 1 <= G <= LEXICON_MAX_PHRASES:
        raise ValueError("G = %d phrases: the decoder takes 1 .. %d" % (G, LEXICON_MAX_PHRASES))
    ext = _scaled_table(np.zeros((G + 1, G)) if lm is None else lm, (G + 1, G), alpha, float(beta), "lm", f32_range=True)
    fin = None if lm_end is None else _scaled_table(lm_end, (G + 1,), alpha, 0.0, "lm_end", f32_range=True)
    return ext, fin


def lexicon_from_arrays(n, phr, seg, conf):
    """mgr_ctc_lexicon_decode's (count, phrase, [first, last], confidence) arrays -> per sample a list of (phrase, first, last, conf);
    a sample without a finite-scoring sequence (count -1) has none.  Raises when a sample has more phrases than the arrays hold."""
    return segments_from_arrays(np.maximum(np.asarray(n), 0), phr, seg, conf)


def lexicon_decode(pred_out, lexicon, lm=None, lm_end=None, alpha=1.0, beta=0.0, input_length=None, skip=2, dev=None, return_path=False,
                   eps=1e-8, max_phrases=256):
    """Lexicon-constrained CTC decode on the GPU (mgr_ctc_lexicon_decode): the best PHRASE sequence whose word expansion
    the word posteriors pred_out (N, T, C) support - one Viterbi pass over the lexicon composed with the CTC topology (blank = C - 1),
    with an optional phrase bigram lm (G + 1, G) / lm_end (G + 1,) weighted alpha, plus beta per phrase (phrase_lm_tables; -inf
    forbids a transition).  lexicon: whatever compile_lexicon takes.
    Returns (segments, score, logp[, path]): per sample a list of (phrase, first_frame, last_frame, confidence) - what write_mlf's
    segments= takes; the frames, indices of the ORIGINAL sequence, run from the first frame of the phrase's first word to the last frame
    of its last word, the confidence is the mean of P[t, emitted word] over its non-blank frames -, score (N,) float64 = logp + the
    table terms, logp (N,) float64 the network's part, path (N, T - skip) int32 the class emitted per frame (-1 past input_length).
    A sample for which no sequence has a finite score has no segments and -inf scores.  max_phrases sizes the first download; a sample
    with more phrases (the device reports the true count) makes the call run again with room for T - skip."""
    P = _posteriors(pred_out)
    make = lambda cap: lexicon_op(P.shape[2], skip, lexicon, lm, lm_end, alpha, beta, cap, return_path, eps)
    return _run_with_room(make, max_phrases, P, skip, dev, input_length=input_length)


def decode_lexicon_mlf(pred_out, f_list, lexicon, names, ignore_list, name_fmt, out_file, **kwargs):
    """What a network's decode_lexicon does: pred_out (N, T, C) softmax - decoded with lexicon_decode(lexicon, **kwargs) - or the
    (segments, score, logp) that Model.predict_generator(decode="lexicon", ...) computed on the device.  The phrases go through `names`
    into the unchanged write_mlf with their times; returns (phrase-name lists, segments)."""
    segs = pred_out[0] if isinstance(pred_out, tuple) else lexicon_decode(np.asarray(pred_out), lexicon, **kwargs)[0]
    ret = [[names[s[0]] for s in sg] for sg in segs]
    if out_file is not None:
        write_mlf(out_file, ret, f_list, ignore_list, name_fmt, segments=segs)
    return ret, segs


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


# ---- sampled hypothesis sets (K16): frame paths drawn from the posteriors, collapsed, merged and counted ----------------
SAMPLE_MAX_DRAWS, SAMPLE_MAX_CLASSES = 32, 64       # MGR_SAMPLE_MAX_DRAWS of include/mgr.h, and its C <= 64


def samples_from_arrays(out, out_len, count):
    """mgr_ctc_sample_paths' arrays ((B, K, T - skip), (B, K), (B, K)) -> (paths: per sample its unique labellings as label lists in
    order of first occurrence, counts: per sample the number of draws that gave each)."""
    B, K = out_len.shape
    live = [[j for j in range(K) if out_len[b, j] >= 0] for b in range(B)]
    return ([[[int(v) for v in out[b, j, :out_len[b, j]]] for j in live[b]] for b in range(B)],
            [[int(count[b, j]) for j in live[b]] for b in range(B)])


def sample_hypotheses(pred_out, draws=8, seed=0, input_length=None, skip=2, dev=None, return_path=False, eps=1e-8):
    """A hypothesis set per sample by SAMPLING on the GPU (mgr_ctc_sample_paths): `draws` (1 .. 32) frame paths per sample
    drawn from the per-frame distribution (P + eps) / sum (P + eps) - the loss's -, each collapsed to its labelling (blank = C - 1),
    equal labellings merged.  A pure function of (pred_out, seed): the same call gives the same set.
    Returns (paths, counts[, frame_paths]): paths[b] the unique labellings in order of first occurrence - what ctc_scores,
    pool_hypotheses, nbest_attainable and expected_risk take as they take the beam search's lists -, counts[b] the number of draws that
    gave each (they sum to `draws`; np.log(counts / draws) serves mbr_decode as scores, counts[b][j] / draws is the share of draws
    that agree with labelling j), frame_paths (N, draws, T - skip) int32 the class drawn at every frame, in draw order, -1 past the
    input length."""
    P = _posteriors(pred_out)
    return _run(sample_op(P.shape[2], skip, draws, seed, return_path, eps), P, skip, dev, input_length)


def decode_samples_map(pred_out, f_list, map_gest, **kwargs):
    """What the networks' decode_samples share: pred_out (N, T, C) softmax - sampled with sample_hypotheses(**kwargs) - or the (paths,
    counts) that Model.predict_generator(decode="sample", ...) drew on the device.  Returns (per file the name lists of its unique
    sampled labellings through the class map, as decode_beam returns its N-best lists; counts)."""
    if len(f_list) != (len(pred_out[0]) if isinstance(pred_out, tuple) else len(pred_out)):
        raise ValueError("%d files for %d samples" % (len(f_list), len(pred_out[0]) if isinstance(pred_out, tuple) else len(pred_out)))
    paths, counts = pred_out[:2] if isinstance(pred_out, tuple) else sample_hypotheses(np.asarray(pred_out), **kwargs)[:2]
    return [[[map_gest[i] for i in seq] for seq in hyps] for hyps in paths], counts


# ---- rescoring N-best lists across modalities (K14): CTC scores of pooled hypotheses, combined and re-ranked -----------
RESCORE_MAX_LABELS, RESCORE_MAX_WIDTH = 255, 65536       # MGR_RESCORE_MAX_* of include/mgr.h


def pack_nbest(paths, K=None, width=None):
    """Per sample a list of label lists (what beam_search_lm_decode(top_paths > 1) or pool_hypotheses return) -> the arrays
    mgr_ctc_rescore reads, in the layout mgr_ctc_beam_search_lm writes: (hyp (N, K, Lh) int32 padded -1, hyp_len (N, K) int32, -1 =
    no hypothesis in the slot).  K / width default to the largest list / longest hypothesis (at least 1); smaller ones are refused."""
    paths = [[[int(v) for v in h] for h in hyps] for hyps in paths]
    most = max([len(h) for h in paths] + [1])
    longest = max([len(h) for hyps in paths for h in hyps] + [1])
    K, Lh = most if K is None else int(K), longest if width is None else int(width)
    if K < most or Lh < longest:
        raise ValueError("K = %d / width = %d: the lists hold up to %d hypotheses of up to %d labels" % (K, Lh, most, longest))
    if Lh > RESCORE_MAX_WIDTH:
        raise ValueError("width = %d: rows of at most %d entries" % (Lh, RESCORE_MAX_WIDTH))
    hyp, hyp_len = -np.ones((len(paths), K, Lh), np.int32), -np.ones((len(paths), K), np.int32)
    for b, hyps in enumerate(paths):
        for k, h in enumerate(hyps):
            hyp[b, k, :len(h)] = h
            hyp_len[b, k] = len(h)
    return hyp, hyp_len


def ctc_scores(pred_out, paths_or_arrays, lexicon=None, input_length=None, skip=2, dev=None, eps=1e-8, return_counts=False):
    """log p(hypothesis | posteriors) for many hypotheses per sample in one launch (mgr_ctc_rescore): the sum over ALL CTC
    alignments, under the loss's conventions (frames skip .., y = softmax(log(P + eps)), blank = C - 1) - for a label row the loss
    takes, minus the loss.  pred_out (N, T, C); paths_or_arrays: per sample a list of label lists, or the (hyp (N, K, Lh), hyp_len
    (N, K)) of pack_nbest / of the beam decoder's device output.  With a lexicon (whatever compile_lexicon takes) the entries are
    PHRASE ids and their word expansion is scored, expanded on the device.
    Returns logp (N, K) float64: -inf for an absent slot or a hypothesis that does not fit the input length, NaN ("not scored") for
    one with a phrase id outside the lexicon or more than 255 expanded labels[, n_lab (N, K) int32: the expanded label counts]."""
    P = _posteriors(pred_out)
    arrays = isinstance(paths_or_arrays, tuple) and len(paths_or_arrays) == 2 and np.ndim(paths_or_arrays[0]) == 3
    hyp, hyp_len = paths_or_arrays if arrays else pack_nbest(paths_or_arrays)
    hyp, hyp_len = np.ascontiguousarray(hyp, np.int32), np.ascontiguousarray(hyp_len, np.int32)
    if hyp.shape[0] != P.shape[0] or hyp_len.shape != hyp.shape[:2]:
        raise ValueError("hypotheses %s / lengths %s for %d samples" % (hyp.shape, hyp_len.shape, P.shape[0]))
    logp, n_lab = _run(rescore_op(P.shape[2], skip, lexicon, eps), P, skip, dev, input_length, (hyp, hyp_len))
    return (logp, n_lab) if return_counts else logp


def pool_hypotheses(*nbest_lists, cap=None):
    """The hypotheses every stream scores: per sample the ordered union without duplicates of its lists - the first list's order, then
    what each further list adds, in its order; cap truncates.  Each argument is per sample a list of label lists."""
    if not nbest_lists:
        return []
    N = len(nbest_lists[0])
    if any(len(l) != N for l in nbest_lists):
        raise ValueError("lists for %s samples" % ([len(l) for l in nbest_lists],))
    pool = []
    for b in range(N):
        seen, out = set(), []
        for lst in nbest_lists:
            for h in lst[b]:
                key = tuple(int(v) for v in h)
                if key not in seen:
                    seen.add(key)
                    out.append(list(key))
        pool.append(out if cap is None else out[:int(cap)])
    return pool


def combine_scores(parts, paths, weights=None, lm=None, lm_end=None, alpha=1.0, beta=0.0):
    """Stream-weighted totals of pooled hypotheses and their ranking (host, fp64).  parts (N, K, M): the score of hypothesis k of
    sample b in stream m (ctc_scores); paths: the pool, per sample at most K label lists over one gesture alphabet.
        total = sum_m weights[m] * parts[.., m] + alpha * (lm[prev + 1, g] over the hypothesis + lm_end[last + 1]) + beta * len
    with the tables of phrase_lm_tables (row / index 0 = start of sequence / the empty sequence; -inf forbids; lm_end may be None).
    A zero weight leaves its stream out, whatever the stream holds.  Returns (order (N, K) int64: slot indices, best first; total
    (N, K) float64 in that order).  Ties go to pool order; hypotheses whose total is -inf or NaN and absent slots (total -inf) come
    last, in pool order."""
    parts = np.asarray(parts, np.float64)
    if parts.ndim != 3 or parts.shape[0] != len(paths):
        raise ValueError("parts %s for %d samples" % (parts.shape, len(paths)))
    N, K, M = parts.shape
    w = np.ones(M) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    if w.shape != (M,) or not np.all(np.isfinite(w)):
        raise ValueError("weights %r for %d streams" % (weights, M))
    ext = fin = None
    if lm is not None or lm_end is not None:
        G = np.shape(lm)[1] if lm is not None else len(lm_end) - 1
        ext, fin = phrase_lm_tables(G, lm, lm_end, alpha, 0.0)
    total = np.zeros((N, K))
    for m in range(M):
        if w[m] != 0.0:
            total += w[m] * parts[:, :, m]
    order = np.zeros((N, K), np.int64)
    for b, hyps in enumerate(paths):
        if len(hyps) > K:
            raise ValueError("sample %d has %d hypotheses, parts hold %d" % (b, len(hyps), K))
        for k, h in enumerate(hyps):
            t, prev = float(beta) * len(h), 0
            for g in h:
                if ext is not None:
                    if not 0 <= int(g) < ext.shape[1]:
                        raise ValueError("sample %d: label %d is outside the tables' %d" % (b, int(g), ext.shape[1]))
                    t += ext[prev, int(g)]
                    prev = int(g) + 1
            if fin is not None:
                t += fin[prev if h else 0]
            total[b, k] += t
        total[b, len(hyps):] = -np.inf
        good = np.isfinite(total[b])
        first = np.flatnonzero(good)
        first = first[np.argsort(-total[b, first], kind="stable")]
        order[b] = np.concatenate([first, np.flatnonzero(~good)])
    return order, np.take_along_axis(total, order, axis=1)


def rescore_nbest(streams, paths, weights=None, lm=None, lm_end=None, alpha=1.0, beta=0.0, dev=None):
    """Multiple-hypotheses rescoring: every stream scores the same pool, the scores are combined (combine_scores) and
    the pool is re-ranked.  streams: a list of (pred_out (N, T, C), dict(lexicon=, input_length=, skip=, eps=)) - T and C may differ
    from stream to stream, a stream with a lexicon reads the pool's labels as phrase ids - or of ((N, K) scores computed elsewhere,
    e.g. by Model.rescore_generator, anything).  paths: the pool (pool_hypotheses).
    Returns (ranked paths: per sample its hypotheses best first, total (N, K), parts (N, K, M) in ranked order, order (N, K)) - paths
    and total are what mbr_decode(paths, scores) and nbest_attainable(paths, refs) take."""
    hyp, hyp_len = pack_nbest(paths)
    cols = []
    for pred_out, opts in streams:
        if np.ndim(pred_out) == 2:
            s = np.asarray(pred_out, np.float64)
            if s.shape != hyp_len.shape:
                raise ValueError("scores %s for a pool of %s" % (s.shape, hyp_len.shape))
        else:
            s = ctc_scores(pred_out, (hyp, hyp_len), dev=dev, **(opts or {}))
        cols.append(s)
    parts = np.stack(cols, axis=2)
    order, total = combine_scores(parts, paths, weights, lm, lm_end, alpha, beta)
    ranked = [[list(paths[b][k]) for k in order[b] if k < len(paths[b])] for b in range(len(paths))]
    return ranked, total, np.take_along_axis(parts, order[:, :, None], axis=1), order


# ---- joint decode over several streams (K19): a label-synchronous prefix search that every stream scores ---------------
JOINT_MAX_STREAMS, JOINT_MAX_PHRASE_WORDS, JOINT_MAX_BEAM = 4, 8, 32       # MGR_JOINT_MAX_* of include/mgr.h, and its beam <= 32


def joint_from_arrays(out, out_len, score, logp):
    """mgr_ctc_joint_decode's arrays ((B, K, max_len), (B, K), (B, K), (B, K, M)) -> (paths: per sample its hypotheses best first,
    score (B, K), parts (B, K, M)) - rescore_nbest's ranked shapes."""
    B, K = out_len.shape
    paths = [[[int(v) for v in out[b, k, :out_len[b, k]]] for k in range(K) if out_len[b, k] >= 0] for b in range(B)]
    return paths, score.copy(), logp.copy()


def joint_decode(streams, G=None, weights=None, lm=None, lm_end=None, alpha=1.0, beta=0.0, beam_width=10, top_paths=1, max_len=None,
                 input_lengths=None, skip=2, dev=None, return_rounds=False):
    """Joint decode over several CTC streams on the GPU (mgr_ctc_joint_decode): a prefix search over GESTURE sequences in
    which every stream scores every extension with its CTC prefix probability - unlike rescore_nbest it can return a sequence that no
    stream proposed on its own.  streams: a list of (posteriors (N, T, C) - a host array or a float32 DeviceArray -, dict(lexicon=,
    input_length=, skip=, eps=) or None), the pairs rescore_nbest takes; T, C and the frame rate may differ from stream to stream, the
    blank is each stream's last class.  A stream with a lexicon (whatever compile_lexicon takes, phrases of at most 8 words) reads
    gesture g as its phrase's words, one without reads it as class g.  G: the number of gestures (default: the lexicons' phrase count,
    without a lexicon the first stream's C - 1).  A hypothesis ranks by
        sum_m weights[m] * ln p_m + alpha * (lm over its gesture pairs + lm_end[last + 1]) + beta * len
    with the tables of phrase_lm_tables.  beam_width <= 32 prefixes are kept per round, top_paths <= beam_width hypotheses returned;
    max_len (default: the shortest stream's frames, at most 255) bounds the gestures per hypothesis.  input_lengths: per stream None or
    (N,) lengths (a stream's dict may hold its own).
    Returns (paths: per sample its at most top_paths hypotheses best first, score (N, top_paths) float64 with -inf in empty slots,
    parts (N, top_paths, M): each stream's ln p, unweighted) - what pool_hypotheses, mbr_decode, nbest_attainable, ctc_scores and
    expected_risk take from rescore_nbest[, rounds (N,): the rounds each sample's search ran]."""
    dev = dev or default_device()
    M = len(streams)
    if not 1 <= M <= JOINT_MAX_STREAMS:
        raise ValueError("%d streams: the decoder takes 1 .. %d" % (M, JOINT_MAX_STREAMS))
    w = np.ones(M) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    if w.shape != (M,) or not np.all(np.isfinite(w)) or not np.all(w > 0):
        raise ValueError("weights %r for %d streams: positive finite numbers" % (weights, M))
    if input_lengths is not None and len(input_lengths) != M:
        raise ValueError("input_lengths for %d streams, not %d" % (M, len(input_lengths)))
    held, keep_alive, descs = [], [], []

    def keep(a):
        held.append(a)
        return a
    try:
        N = None
        for m, (post, opts) in enumerate(streams):
            opts = dict(opts or {})
            dP = post if isinstance(post, _capi.DeviceArray) else keep(dev.array(_posteriors(post)))
            if len(dP.shape) != 3 or dP.dtype != np.float32:
                raise ValueError("stream %d: posteriors %s %s, not (N, T, C) float32" % (m, dP.shape, dP.dtype))
            n, T, Cn = dP.shape
            if N is not None and n != N:
                raise ValueError("stream %d holds %d samples, stream 0 %d" % (m, n, N))
            N = n
            sk = int(opts.get("skip", skip))
            il = opts.get("input_length", None if input_lengths is None else input_lengths[m])
            il = np.full(N, T - sk, np.int32) if il is None else np.asarray(il).reshape(N).astype(np.int32)
            off = words = None
            if opts.get("lexicon") is not None:
                off, words = compile_lexicon(opts["lexicon"], Cn)
                if int(np.diff(off).max()) > JOINT_MAX_PHRASE_WORDS:
                    raise ValueError("stream %d: a phrase of %d words, the joint decoder takes %d" % (m, int(np.diff(off).max()), JOINT_MAX_PHRASE_WORDS))
                keep_alive += [off, words]
            descs.append(dict(T=T, C=Cn, skip=sk, blank=Cn - 1, eps=opts.get("eps", 1e-8), weight=w[m], P=dP, input_len=keep(dev.array(il)),
                              phrase_off=off, phrase_words=words))
        counts = set(len(d["phrase_off"]) - 1 for d in descs if d["phrase_off"] is not None)
        if len(counts) > 1:
            raise ValueError("the streams' lexicons hold %s phrases" % sorted(counts))
        G = int(G) if G is not None else (counts.pop() if counts else descs[0]["C"] - 1)
        if counts and G not in counts:
            raise ValueError("G = %d for lexicons of %s phrases" % (G, sorted(counts)))
        for m, d in enumerate(descs):
            if d["phrase_off"] is None and G > d["C"]:
                raise ValueError("stream %d: G = %d gestures for %d classes without a lexicon" % (m, G, d["C"]))
        W, NP = int(beam_width), int(top_paths)
        if not 1 <= NP <= W <= JOINT_MAX_BEAM:
            raise ValueError("top_paths = %d / beam_width = %d: 1 <= top_paths <= beam_width <= %d" % (NP, W, JOINT_MAX_BEAM))
        Lmax = min(RESCORE_MAX_LABELS, min(d["T"] - d["skip"] for d in descs)) if max_len is None else int(max_len)
        if not 1 <= Lmax <= RESCORE_MAX_LABELS:
            raise ValueError("max_len = %d: 1 .. %d" % (Lmax, RESCORE_MAX_LABELS))
        ext, fin = phrase_lm_tables(G, lm, lm_end, alpha, beta)
        arr = _capi.make_joint_streams(descs)
        dext, dfin = keep(dev.array(ext)), None if fin is None else keep(dev.array(fin))
        out, out_len = keep(dev.empty((N, NP, Lmax), np.int32)), keep(dev.empty((N, NP), np.int32))
        score, logp, rounds = keep(dev.empty((N, NP), np.float64)), keep(dev.empty((N, NP, M), np.float64)), keep(dev.empty((N,), np.int32))
        ws = keep(dev.bytes(dev.lib.mgr_ctc_joint_ws_bytes(N, M, arr, G, W, NP, Lmax)))
        dev.call("mgr_ctc_joint_decode", N, M, arr, G, dext, dfin, W, NP, Lmax, out, out_len, score, logp, rounds, ws, ws.nbytes)
        res = joint_from_arrays(out.download(), out_len.download(), score.download(), logp.download())
        return res + ((rounds.download(),) if return_rounds else ())
    finally:
        for a in held:
            a.free()


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


# ---- scoring on the device (K12): mgr_edit_distance and what is built on it -----------------------------------------
HTK_COSTS = (10, 7, 7)      # (substitution, deletion, insertion) of HTK's HResults (HTK book, 17.4 of the 3.4 edition)
NIST_COSTS = (4, 3, 3)      # ... of its -n switch, the NIST scoring package's alignment
EDIT_MAX_LEN, EDIT_MAX_COST = 4095, 16384       # MGR_EDIT_MAX_LEN / MGR_EDIT_MAX_COST of include/mgr.h


def check_costs(costs):
    """(sub, del, ins) as three ints in [1, EDIT_MAX_COST], or ValueError."""
    c = tuple(costs)
    if len(c) != 3 or any(int(v) != v for v in c) or not all(1 <= int(v) <= EDIT_MAX_COST for v in c):
        raise ValueError("costs %r: three integers (sub, del, ins) in [1, %d]" % (costs, EDIT_MAX_COST))
    return tuple(int(v) for v in c)


def ignore_mask(ignore):
    """Label ids (each in [0, 64)) -> the bit mask mgr_edit_distance takes."""
    mask = 0
    for v in ignore or ():
        if not 0 <= int(v) < 64:
            raise ValueError("ignored label %r is not in [0, 64)" % (v,))
        mask |= 1 << int(v)
    return mask


def edit_distances(hyps, refs, pairs=None, costs=(1, 1, 1), ignore=(), return_ops=False, dev=None):
    """Weighted edit distances of many pairs in one launch (mgr_edit_distance).  hyps / refs: whatever pack_labels takes (a padded
    array or a list of label lists); pairs: None - pair p is (hyps[p], refs[p]) - or a (P, 2) array of (hyp row, ref row) indices,
    range-checked here; costs = (sub, del, ins); ignore: label ids in [0, 64) that both sides lose before the comparison.
    Returns dist (P,) int32, counts (P, 4) int32 = (H, S, D, I), lens (P, 2) int32 = (m, n) after the filter[, ops: a list of P int8
    arrays, the alignment in forward order: 0 hit, 1 substitution, 2 deletion, 3 insertion].  The tuple (cost, S, D, I) is the
    lexicographically smallest over all alignments (include/mgr.h)."""
    cs, cd, ci = check_costs(costs)
    mask = ignore_mask(ignore)
    h, _ = pack_labels(hyps)
    r, _ = pack_labels(refs)
    if pairs is None:
        if h.shape[0] != r.shape[0]:
            raise ValueError("%d hypotheses for %d references" % (h.shape[0], r.shape[0]))
        P, pr = h.shape[0], None
    else:
        pr = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2))
        P = pr.shape[0]
        if P and (pr.min() < 0 or pr[:, 0].max() >= h.shape[0] or pr[:, 1].max() >= r.shape[0]):
            raise IndexError("pair index out of range (%d hypotheses, %d references)" % (h.shape[0], r.shape[0]))
    if h.shape[1] > EDIT_MAX_LEN or r.shape[1] > EDIT_MAX_LEN:
        raise ValueError("rows of %d / %d labels: at most %d" % (h.shape[1], r.shape[1], EDIT_MAX_LEN))
    if P == 0:
        z = np.zeros((0,), np.int32), np.zeros((0, 4), np.int32), np.zeros((0, 2), np.int32)
        return z + ([],) if return_ops else z
    dev = dev or default_device()
    Lh, Lr = h.shape[1], r.shape[1]
    bufs = [dev.array(h), dev.array(r)]
    try:
        dph = dpr = None
        if pr is not None:
            bufs += [dev.array(pr[:, 0].astype(np.int32)), dev.array(pr[:, 1].astype(np.int32))]
            dph, dpr = bufs[2], bufs[3]
        ddist, dcnt, dlen = dev.empty((P,), np.int32), dev.empty((P, 4), np.int32), dev.empty((P, 2), np.int32)
        bufs += [ddist, dcnt, dlen]
        dops = dnops = ws = None
        if return_ops:
            dops, dnops = dev.empty((P, Lh + Lr), np.int8), dev.empty((P,), np.int32)
            ws = dev.bytes(dev.lib.mgr_edit_distance_ws_bytes(P, Lh, Lr, 1))
            bufs += [dops, dnops, ws]
        dev.call("mgr_edit_distance", bufs[0], None, h.shape[0], Lh, bufs[1], None, r.shape[0], Lr, dph, dpr, P, cs, cd, ci, mask,
                 ddist, dcnt, dlen, dops, dnops, ws, ws.nbytes if ws is not None else 0)
        res = (ddist.download(), dcnt.download(), dlen.download())
        if return_ops:
            o, k = dops.download(), dnops.download()
            res += ([o[p, :k[p]].copy() for p in range(P)],)
    finally:
        for a in bufs:
            a.free()
    return res


def score_from_counts(counts, lens, loss=None):
    """Sums of per-sample (H, S, D, I) / (m, n) -> the figures HResults prints: ler = (S + D + I) / N, corr = H / N, acc = (H - I) / N
    (N = the number of reference labels; 0 -> N taken as 1)."""
    counts = np.asarray(counts, np.int64).reshape(-1, 4)
    H, S, D, I = (int(v) for v in counts.sum(axis=0))
    N = int(np.asarray(lens, np.int64).reshape(-1, 2)[:, 1].sum())
    den = max(1, N)
    return {"H": H, "S": S, "D": D, "I": I, "N": N, "ler": (S + D + I) / den, "corr": H / den, "acc": (H - I) / den}


def confusion_from_ops(hyps, refs, ops, n_classes, ignore=()):
    """(C + 1, C + 1) int64 [ref label or C for "inserted", hyp label or C for "deleted"] from the alignments of edit_distances."""
    Cn = int(n_classes)
    conf = np.zeros((Cn + 1, Cn + 1), np.int64)
    h, _ = pack_labels(hyps)
    r, _ = pack_labels(refs)
    drop = set(int(v) for v in ignore)
    for p, o in enumerate(ops):
        hs = [int(v) for v in h[p] if v >= 0 and int(v) not in drop]
        rs = [int(v) for v in r[p] if v >= 0 and int(v) not in drop]
        o = np.asarray(o)
        if int((o != 2).sum()) != len(hs) or int((o != 3).sum()) != len(rs):
            raise ValueError("pair %d: the alignment does not consume its %d / %d labels" % (p, len(hs), len(rs)))
        # every step but a deletion consumes the next hyp label, every step but an insertion the next ref label
        hl = np.where(o != 2, np.asarray(hs + [Cn], np.int64)[np.clip(np.cumsum(o != 2) - 1, 0, len(hs))], Cn)
        rl = np.where(o != 3, np.asarray(rs + [Cn], np.int64)[np.clip(np.cumsum(o != 3) - 1, 0, len(rs))], Cn)
        if hl.size and (hl.max() > Cn or rl.max() > Cn):
            raise ValueError("a label is not below n_classes = %d" % Cn)
        np.add.at(conf, (rl, hl), 1)
    return conf


def score_sequences(hyps, refs, costs=(1, 1, 1), ignore=(), confusion=False, n_classes=None, dev=None):
    """Score hypotheses against references on the device: a dict with the summed H, S, D, I and N (reference labels), ler = (S + D +
    I) / max(1, N), HResults' two figures corr = H / N and acc = (H - I) / N, dist_sum, per_sample = {"dist", "counts", "lens"} and,
    with confusion, "confusion": a (C + 1, C + 1) int64 matrix [ref label or C for "inserted", hyp label or C for "deleted"] formed
    from the alignments with numpy (n_classes = C; default: the largest label + 1)."""
    res = edit_distances(hyps, refs, costs=costs, ignore=ignore, return_ops=confusion, dev=dev)
    dist, counts, lens = res[:3]
    out = score_from_counts(counts, lens)
    out["dist_sum"] = int(dist.astype(np.int64).sum())
    out["per_sample"] = {"dist": dist, "counts": counts, "lens": lens}
    if confusion:
        if n_classes is None:
            h, _ = pack_labels(hyps)
            r, _ = pack_labels(refs)
            n_classes = int(max(h.max(initial=-1), r.max(initial=-1))) + 1
        out["confusion"] = confusion_from_ops(hyps, refs, res[3], n_classes, ignore)
    return out


def score_mlf_counts(ref_path, rec_path, ignore=("sil",), costs=HTK_COSTS, dev=None):
    """score_sequences over two HTK master label files, over the samples present in both: label names are mapped to ids (sorted names
    of both files, the ignored ones left out beforehand).  The alignment costs default to HResults' (10, 7, 7), so H / S / D / I, corr
    and acc are HResults' quantities by construction; parity with the HResults BINARY is unpinned - HTK is not available to this
    project, no output of it has been compared.  Returns the score_sequences dict plus "n_samples" and "names" (id -> label name)."""
    ref, rec = read_mlf(ref_path), read_mlf(rec_path)
    names = sorted(set(ref) & set(rec))
    strip = lambda seq: [x for x in seq if x not in ignore]
    hyps, refs = [strip(rec[n]) for n in names], [strip(ref[n]) for n in names]
    vocab = sorted(set(x for s in hyps + refs for x in s))
    ids = {x: i for i, x in enumerate(vocab)}
    out = score_sequences([[ids[x] for x in s] for s in hyps], [[ids[x] for x in s] for s in refs], costs=costs, dev=dev)
    out["n_samples"], out["names"] = len(names), vocab
    return out


def _flatten_nbest(paths):
    """Per sample a ranked list of label lists -> (flat list of hypotheses, first flat index per sample (N + 1,))."""
    flat, off = [], [0]
    for hyps in paths:
        flat.extend(list(h) for h in hyps)
        off.append(len(flat))
    return flat, np.asarray(off, np.int64)


def nbest_attainable(paths, refs, costs=(1, 1, 1), ignore=(), dev=None):
    """What the best choice from N-best lists would score - the best attainable error rate of the lists, the bound a rescoring pass
    is measured against: per sample the smallest distance to its reference over its hypotheses
    (what beam_search_lm_decode returns with top_paths > 1) and the rank that attains it (ties: the better rank; no hypothesis: the
    distance of the empty one, rank -1), in ONE launch over all pairs.  Returns (dist (N,) int64, rank (N,) int64, ler = sum dist /
    max(1, sum n)) - with unit costs the label error rate no rescoring pass over these lists can beat."""
    flat, off = _flatten_nbest(paths)
    N = len(paths)
    rlab, _ = pack_labels(refs)
    if rlab.shape[0] != N:
        raise ValueError("%d references for %d samples" % (rlab.shape[0], N))
    flat.append([])                                     # the empty hypothesis: its distance stands in where a sample has none
    pairs = [(k, b) for b in range(N) for k in range(off[b], off[b + 1])] + [(len(flat) - 1, b) for b in range(N)]
    dist, _, lens = edit_distances(flat, rlab, pairs=pairs, costs=costs, ignore=ignore, dev=dev)
    npairs = int(off[-1])
    best, rank = dist[npairs:].astype(np.int64), -np.ones(N, np.int64)
    for b in range(N):
        if off[b + 1] > off[b]:
            d = dist[off[b]:off[b + 1]]
            rank[b] = int(np.argmin(d))                 # (the first minimum: ties go to the better rank)
            best[b] = int(d[rank[b]])
    return best, rank, float(best.sum()) / max(1, int(lens[npairs:, 1].sum()))


def mbr_decode(paths, scores, scale=1.0, costs=(1, 1, 1), dev=None):
    """Minimum-Bayes-risk pick from N-best lists: per sample with K surviving hypotheses, w = softmax(scale * score) over them (fp64,
    host), risk_k = sum_j w_j * dist(hyp = h_k, ref = h_j), and the pick is the smallest risk, ties to the better rank.  All K x K
    distances of all samples go to the device in one launch.  paths / scores as beam_search_lm_decode(top_paths > 1) returns them.
    Returns (picked paths: a label list per sample, [] where none survives; picked ranks (N,) int64, -1 likewise; risk (N,
    top_paths) float64, +inf where there is no hypothesis).  K = 1 returns the 1-best.  Whether this lowers an error rate on real
    data is not measured here."""
    flat, off = _flatten_nbest(paths)
    N = len(paths)
    scores = np.asarray(scores, np.float64).reshape(N, -1)
    NP = scores.shape[1]
    pairs = [(k, j) for b in range(N) for k in range(off[b], off[b + 1]) for j in range(off[b], off[b + 1])]
    dist = edit_distances(flat, flat, pairs=pairs, costs=costs, dev=dev)[0] if pairs else np.zeros(0, np.int32)
    risk = np.full((N, NP), np.inf)
    picks, ranks, q = [], -np.ones(N, np.int64), 0
    for b in range(N):
        K = int(off[b + 1] - off[b])
        if K == 0:
            picks.append([])
            continue
        if K > NP:
            raise ValueError("sample %d has %d hypotheses, scores hold %d" % (b, K, NP))
        z = float(scale) * scores[b, :K]
        w = np.exp(z - z.max())
        w /= w.sum()
        d = dist[q:q + K * K].reshape(K, K).astype(np.float64)
        q += K * K
        risk[b, :K] = d @ w
        ranks[b] = int(np.argmin(risk[b, :K]))
        picks.append(list(paths[b][ranks[b]]))
    return picks, ranks, risk


# ---- minimum-risk training (K15): the expected edit distance over an N-best list and its gradient ----------------------
RISK_MAX_SLOTS = 32       # MGR_RISK_MAX_SLOTS of include/mgr.h


def risk_label_cap(hyp, hyp_len, lex_off=None):
    """Lcap for mgr_ctc_risk_grad: the longest hypothesis of (hyp (N, K, Lh), hyp_len (N, K)) after expansion through the lexicon
    offsets (None: labels), within the kernel's [1, RESCORE_MAX_LABELS] - a longer one is then "not scored", as in ctc_scores."""
    n = np.clip(hyp_len, 0, hyp.shape[2])
    if lex_off is None:
        longest = int(n.max()) if n.size else 0
    else:
        G = len(lex_off) - 1
        inside = (np.arange(hyp.shape[2])[None, None, :] < n[:, :, None]) & (hyp >= 0) & (hyp < G)
        words = np.diff(lex_off)[np.clip(hyp, 0, G - 1)]
        longest = int(np.where(inside, words, 0).sum(axis=2).max()) if n.size else 0
    return max(1, min(RESCORE_MAX_LABELS, longest))


def expected_risk(pred_out, paths_or_arrays, refs=None, risks=None, costs=(1, 1, 1), ignore=(), risk_scale=1.0, post_scale=1.0,
                  lexicon=None, input_length=None, skip=2, eps=1e-8, grad=True, dev=None):
    """The expected risk of N-best lists under the network's own CTC posterior over them, and its gradient w.r.t. the Dense logits
    (mgr_ctc_risk_grad) - the loss of sequence-level minimum-risk training: per sample, over the live hypotheses (present,
    scored, feasible), w = softmax(post_scale * logp), risk = sum_k w_k * risks_k * risk_scale, with logp what ctc_scores returns.
    pred_out (N, T, C); paths_or_arrays / lexicon as ctc_scores takes them (at most 32 hypotheses per sample).  Exactly one of
    refs - whatever pack_labels takes, one reference per sample: the risks are the edit distances (costs, ignore as edit_distances) of
    hypothesis k of sample b to reference b, formed on the device (an absent slot counts as the empty hypothesis; with a lexicon the
    references are phrase ids, as the hypotheses) - and risks - an integer array (N, K).
    Returns (risk (N,) float32, weights (N, K) float32, logp (N, K) float64, risks (N, K) int32[, dlogits (N, T, C) float32 - the
    gradient of sum_b risk_b; zero on the skipped frames, behind the input length, and where fewer than two hypotheses are live])."""
    if (refs is None) == (risks is None):
        raise ValueError("exactly one of refs and risks")
    if not float(post_scale) > 0.0 or not np.isfinite(post_scale):
        raise ValueError("post_scale = %r: a positive number" % (post_scale,))
    P = _posteriors(pred_out)
    N, T, Cn = P.shape
    arrays = isinstance(paths_or_arrays, tuple) and len(paths_or_arrays) == 2 and np.ndim(paths_or_arrays[0]) == 3
    hyp, hyp_len = paths_or_arrays if arrays else pack_nbest(paths_or_arrays)
    hyp, hyp_len = np.ascontiguousarray(hyp, np.int32), np.ascontiguousarray(hyp_len, np.int32)
    if hyp.shape[0] != N or hyp_len.shape != hyp.shape[:2]:
        raise ValueError("hypotheses %s / lengths %s for %d samples" % (hyp.shape, hyp_len.shape, N))
    K, Lh = hyp.shape[1], hyp.shape[2]
    if not 1 <= K <= RISK_MAX_SLOTS:
        raise ValueError("%d hypotheses per sample: 1 .. %d" % (K, RISK_MAX_SLOTS))
    off, words = compile_lexicon(lexicon, Cn) if lexicon is not None else (None, None)
    G = 0 if off is None else len(off) - 1
    host = lambda a: None if a is None else a.ctypes.data
    Lcap = risk_label_cap(hyp, hyp_len, off)
    if refs is not None:
        cs, cd, ci = check_costs(costs)
        mask = ignore_mask(ignore)
        rlab, _ = pack_labels(refs)
        if rlab.shape[0] != N:
            raise ValueError("%d references for %d samples" % (rlab.shape[0], N))
    else:
        r = np.asarray(risks)
        if r.shape != (N, K) or not np.all(r == np.round(r)):
            raise ValueError("risks %s: integers (%d, %d)" % (r.shape, N, K))
        r = np.ascontiguousarray(r, np.int32)
    dev = dev or default_device()
    held = []

    def keep(a):
        held.append(a)
        return a
    try:
        dP = keep(dev.array(P))
        dil = keep(dev.array(np.full(N, T - skip, np.int32) if input_length is None else np.asarray(input_length).reshape(N).astype(np.int32)))
        dh, dl = keep(dev.array(hyp)), keep(dev.array(hyp_len))
        if refs is not None:
            dref = keep(dev.array(rlab))
            dph = keep(dev.array(np.arange(N * K, dtype=np.int32)))
            dpr = keep(dev.array(np.repeat(np.arange(N, dtype=np.int32), K)))
            drisk, dcnt, dlen = keep(dev.empty((N, K), np.int32)), keep(dev.empty((N * K, 4), np.int32)), keep(dev.empty((N * K, 2), np.int32))
            dev.call("mgr_edit_distance", dh, dl, N * K, Lh, dref, None, N, rlab.shape[1], dph, dpr, N * K, cs, cd, ci, mask, drisk, dcnt,
                     dlen, None, None, None, 0)
        else:
            drisk = keep(dev.array(r))
        dlogp, dw, dr = keep(dev.empty((N, K), np.float64)), keep(dev.empty((N, K), np.float32)), keep(dev.empty((N,), np.float32))
        dg = keep(dev.empty((N, T, Cn), np.float32)) if grad else None
        ws = keep(dev.bytes(dev.lib.mgr_ctc_risk_ws_bytes(N, T, Cn, K, Lcap, G, host(off))))
        dev.call("mgr_ctc_risk_grad", dP, dil, N, T, Cn, skip, Cn - 1, C.c_float(eps), host(off), host(words), G, dh, dl, K, Lh, Lcap, drisk,
                 C.c_float(risk_scale), C.c_float(post_scale), C.c_float(1.0), 0, dlogp, dw, dr, dg, ws, ws.nbytes)
        res = (dr.download(), dw.download(), dlogp.download(), drisk.download())
        return res + ((dg.download(),) if grad else ())
    finally:
        for a in held:
            a.free()


def expected_risk_map(pred_out, paths_or_arrays, refs, map_gest, costs=HTK_COSTS, **kwargs):
    """What the networks' expected_risk share: expected_risk against reference label ids with the distance decode_score_map scores by -
    every id whose name is "sil" dropped from both sides, the alignment costs HResults' by default (kwargs: expected_risk's)."""
    sil = [k for k, v in map_gest.items() if v == "sil" and k >= 0]
    return expected_risk(pred_out, paths_or_arrays, refs=refs, costs=costs, ignore=sil, **kwargs)


def decode_score_map(hyp_ids, ref_ids, map_gest, costs=HTK_COSTS, confusion=True, dev=None):
    """What the networks' decode_score share: score_sequences of label-id sequences (what greedy_decode / the beam decoders return,
    blank runs included) over a module's class map - every id whose name is "sil" is dropped from both sides, the confusion matrix
    covers the map's classes, the alignment costs default to HResults'."""
    sil = [k for k, v in map_gest.items() if v == "sil" and k >= 0]
    return score_sequences(hyp_ids, ref_ids, costs=costs, ignore=sil, confusion=confusion, n_classes=1 + max(map_gest), dev=dev)


# ---- frame overlap of segment sets (K18): mgr_segment_overlap and the Jaccard index built on its counts -------------------
def pack_segments(segments):
    """Per sample a list of (label, first, last, ...) tuples -> (int32 (N, S) labels padded -1, int32 (N, S, 2) extents padded -1)."""
    S = max([len(r) for r in segments] + [1])
    lab = -np.ones((len(segments), S), np.int32)
    seg = -np.ones((len(segments), S, 2), np.int32)
    for i, r in enumerate(segments):
        for k, sg in enumerate(r):
            lab[i, k], seg[i, k, 0], seg[i, k, 1] = int(sg[0]), int(sg[1]), int(sg[2])
    return lab, seg


def segment_overlap(hyp_segments, ref_segments, n_classes, n_frames, ignore=(), dev=None):
    """Per sample and class the frames covered by both segment sets, by either, and by each (mgr_segment_overlap): four int32 (N,
    n_classes) arrays (inter, union, hyp_frames, ref_frames), exact.  hyp_segments / ref_segments: per sample a list of (label, first,
    last, ...) with inclusive frames - what forced_align, posterior_align, greedy_segments and lexicon_decode return; n_frames: an int or
    one per sample, extents are clipped to [0, n_frames); ignore: label ids in [0, 64) dropped on both sides.  Segments of one class on
    one side are united; a label outside [0, n_classes) or a negative first frame skips the segment."""
    Cn = int(n_classes)
    if not 1 <= Cn <= 64:
        raise ValueError("n_classes = %d is not in [1, 64]" % Cn)
    N = len(hyp_segments)
    if len(ref_segments) != N:
        raise ValueError("%d hypothesis samples for %d reference samples" % (N, len(ref_segments)))
    mask = ignore_mask(ignore)
    if N == 0:
        return tuple(np.zeros((0, Cn), np.int32) for _ in range(4))
    nf = np.ascontiguousarray(np.broadcast_to(np.asarray(n_frames, np.int64), (N,)).astype(np.int32))
    hl, hs = pack_segments(hyp_segments)
    rl, rs = pack_segments(ref_segments)
    dev = dev or default_device()
    bufs = []
    try:
        bufs += [dev.array(a) for a in (hl, hs, rl, rs, nf)]
        outs = [dev.empty((N, Cn), np.int32) for _ in range(4)]
        bufs += outs
        dev.call("mgr_segment_overlap", bufs[0], bufs[1], hl.shape[1], bufs[2], bufs[3], rl.shape[1], bufs[4], N, Cn, mask, *outs)
        return tuple(o.download() for o in outs)
    finally:
        for a in bufs:
            a.free()


def jaccard_from_counts(inter, union, hyp_frames, ref_frames, false_positives=True):
    """The Jaccard index from mgr_segment_overlap's counts, in float64 on the host.  Per sample: the mean of inter / union over the
    classes present in the reference (false_positives=False) or on either side (True: a class only the hypothesis has scores 0 and
    counts - the penalty as the ChaLearn 2014 challenge's text states it).  A sample with no class to average over is NaN and left out of
    the mean.  Returns {"jaccard", "per_sample" (N,), "per_class" (C,) - over the samples in which the class counts, NaN where none -,
    "inter", "union"}."""
    inter, union = np.asarray(inter, np.int64), np.asarray(union, np.int64)
    present = (np.asarray(ref_frames) > 0) | ((np.asarray(hyp_frames) > 0) if false_positives else False)
    ratio = np.where(present, inter / np.maximum(union, 1).astype(np.float64), 0.0)
    n_s, n_c = present.sum(axis=1), present.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_sample = np.where(n_s > 0, ratio.sum(axis=1) / n_s, np.nan)
        per_class = np.where(n_c > 0, ratio.sum(axis=0) / n_c, np.nan)
    ok = n_s > 0
    return {"jaccard": float(per_sample[ok].mean()) if ok.any() else float("nan"), "per_sample": per_sample, "per_class": per_class,
            "inter": inter, "union": union}


def jaccard_index(hyp_segments, ref_segments, n_classes, n_frames, ignore=(), false_positives=True, dev=None):
    """segment_overlap on the GPU, then jaccard_from_counts.  Parity with the ChaLearn challenge's own evaluation script is unpinned: the
    script is not available to this project."""
    return jaccard_from_counts(*segment_overlap(hyp_segments, ref_segments, n_classes, n_frames, ignore, dev), false_positives=false_positives)


def read_mlf_segments(path, frame_period=FRAME_PERIOD_HTK):
    """The timed lines write_mlf(..., segments=) writes -> {sample name: [(label name, first_frame, last_frame)]}: first = start /
    frame_period, last = end / frame_period - 1 (the end is the end of the last frame).  Lines without times are refused."""
    out, cur = {}, None
    fp = int(frame_period)
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
                w = line.split()
                if len(w) < 3 or not (w[0].isdigit() and w[1].isdigit()):
                    raise ValueError("%s: %r is not a 'start end label' line" % (path, line))
                cur.append((w[2], int(w[0]) // fp, int(w[1]) // fp - 1))
    return out


def score_mlf_overlap(ref_path, rec_path, names, ignore=("sil",), n_frames=None, **kw):
    """The Jaccard index of two timed MLF files over the samples present in both.  names: the label names, a name's index is its class
    id (at most 64; a label not in names is skipped); ignore: label NAMES dropped on both sides; n_frames: {sample name: frames}, an int,
    or None = up to the last frame any segment of the sample reaches.  kw: frame_period, false_positives, dev.  Returns jaccard_index's
    dict plus "n_samples" and "samples" (the sample names, in the order of per_sample)."""
    fp = kw.pop("frame_period", FRAME_PERIOD_HTK)
    ref, rec = read_mlf_segments(ref_path, fp), read_mlf_segments(rec_path, fp)
    samples = sorted(set(ref) & set(rec))
    ids = {n: i for i, n in enumerate(names)}
    conv = lambda segs: [(ids.get(l, -1), a, b) for l, a, b in segs]
    hyp, refs = [conv(rec[n]) for n in samples], [conv(ref[n]) for n in samples]
    if n_frames is None:
        nf = [max([b + 1 for _, _, b in h + r] + [0]) for h, r in zip(hyp, refs)]
    elif isinstance(n_frames, dict):
        nf = [int(n_frames[n]) for n in samples]
    else:
        nf = int(n_frames)
    out = jaccard_index(hyp, refs, len(names), nf, ignore=[ids[n] for n in ignore if n in ids], **kw)
    out["n_samples"], out["samples"] = len(samples), samples
    return out


def decode_extents_mlf(pred_out, f_list, map_gest, ignore_list, name_fmt, out_file, threshold, quantile=0.5, skip=2, dev=None):
    """What the modules' decode_extents share: the greedy decode (threshold, as decode_batch) gives each file's label sequence - blank
    runs dropped -, posterior_align its extents at `quantile`, the class map the names; every MLF line reads "start end name".  Returns
    (label-name lists, segment lists of (label, first_frame, last_frame, confidence, occupancy))."""
    P = _posteriors(pred_out)
    blank = P.shape[2] - 1
    ids = [[i for i in seq if i != blank] for seq in greedy_decode(P, threshold, skip=skip, dev=dev)]
    segs, _ = posterior_align(P, ids, quantile=quantile, skip=skip, dev=dev)
    ret = [[map_gest[s[0]] for s in sg] for sg in segs]
    if out_file is not None:
        write_mlf(out_file, ret, f_list, ignore_list, name_fmt, segments=segs)
    return ret, segs


def group_word_extents(word_segments, phrases, lexicon):
    """Word extents of posterior_align -> one extent per phrase: from its first word's first frame to its last word's last frame; the
    confidence is the occupancy-weighted mean of its words' confidences, the occupancy their sum.  phrases: the phrase ids whose word
    expansion (over lexicon) the words are, in order."""
    out, k = [], 0
    for g in phrases:
        ws = word_segments[k:k + len(lexicon[g])]
        k += len(lexicon[g])
        if len(ws) < len(lexicon[g]):
            break               # (the words did not fit the input: no segments came back)
        occ = sum(w[4] for w in ws)
        out.append((int(g), ws[0][1], ws[-1][2], sum(w[3] * w[4] for w in ws) / occ if occ > 0 else 0.0, occ))
    return out


def decode_extents_lexicon_mlf(pred_out, f_list, lexicon, names, ignore_list, name_fmt, out_file, quantile=0.5, skip=2, dev=None, **kwargs):
    """decode_extents for a network whose classes are words: lexicon_decode (kwargs: its lm, lm_end, alpha, beta) gives each file's
    phrases, posterior_align the extents of their word expansion, group_word_extents - on the host - one extent per phrase."""
    P = _posteriors(pred_out)
    phr, _, _ = lexicon_decode(P, lexicon, skip=skip, dev=dev, **kwargs)
    ids = [[s[0] for s in sg] for sg in phr]
    words = [[int(w) for g in seq for w in lexicon[g]] for seq in ids]
    wsegs, _ = posterior_align(P, words, quantile=quantile, skip=skip, dev=dev)
    segs = [group_word_extents(ws, seq, lexicon) for ws, seq in zip(wsegs, ids)]
    ret = [[names[s[0]] for s in sg] for sg in segs]
    if out_file is not None:
        write_mlf(out_file, ret, f_list, ignore_list, name_fmt, segments=segs)
    return ret, segs
