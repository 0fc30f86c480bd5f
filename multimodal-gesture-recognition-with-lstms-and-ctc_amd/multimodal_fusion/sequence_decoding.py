"""Decode for the fusion network (reference multimodal_fusion/sequence_decoding.py:21-69)."""
import numpy as np

from ..decoding import HTK_COSTS, decode_beam_mlf, decode_extents_mlf, decode_samples_map, decode_score_map, expected_risk_map, greedy_decode, greedy_decode_argmax, greedy_segments, write_mlf

# gesture code -> class name; the blank (21) is emitted as "sil" (reference :26-29)
map_gest = {0: "oov", 1: "VA", 2: "VQ", 3: "PF", 4: "FU", 5: "CP", 6: "CV", 7: "DC", 8: "SP", 9: "CN", 10: "FN",
            11: "OK", 12: "CF", 13: "BS", 14: "PR", 15: "NU", 16: "FM", 17: "TT", 18: "BN", 19: "MC", 20: "ST",
            21: "sil"}
# files the reference skips when writing the MLF (:32)
ignore_list = [228, 298, 299, 300, 303, 304, 334, 343, 373, 375]
THRESHOLD = 0.5


def decode_batch(pred_out, f_list, out_file="final_ctc_recout.mlf"):
    """pred_out (N,T,C) softmax, f_list file numbers.  Writes the MLF and returns the label-name lists
    (ignored files included in the return value, as in the reference)."""
    ids = greedy_decode(np.asarray(pred_out), THRESHOLD, skip=2)
    ret = [[map_gest[i] for i in seq] for seq in ids]
    write_mlf(out_file, ret, f_list, ignore_list, "Sample%05d")
    return ret


def decode_argmax(best, prob, f_list, out_file=None):
    """decode_batch from the per-frame (best label, probability) pairs that Model.predict_generator(decode="argmax") computes
    on the device: same filter, same collapse, same MLF."""
    ids = greedy_decode_argmax(best, prob, THRESHOLD)
    ret = [[map_gest[i] for i in seq] for seq in ids]
    if out_file is not None:
        write_mlf(out_file, ret, f_list, ignore_list, "Sample%05d")
    return ret


def decode_live(model, frames_iter, chunk=20, lookahead=20):
    """decode_segments for a session that is still producing frames (live.decode_live): frames_iter yields {input name:
    [n, F]} pieces at the network rate; yields (name, first_frame, last_frame, confidence) as gestures are finalised, chunk +
    lookahead frames behind the signal.  No confidence filter (it counts over a whole recording)."""
    from ..live import decode_live as _decode_live
    return _decode_live(model, frames_iter, chunk, lookahead, map_gest)


def decode_segments(pred_out, f_list, out_file="final_ctc_recout_timed.mlf"):
    """decode_batch with start and end times: pred_out (N, T, C) softmax - or the per-sample segment lists that
    Model.predict_generator(decode="segments", threshold=THRESHOLD) computed on the device.  The same filter, collapse, class map and
    ignore list; every MLF line reads "start end name" in HTK's 100 ns units (50 ms per frame).  The times are the frames at which the
    network commits to the class, not the extent of the movement.  Returns (label-name lists, segment lists)."""
    segs = pred_out if isinstance(pred_out, list) else greedy_segments(np.asarray(pred_out), THRESHOLD, skip=2)
    ret = [[map_gest[s[0]] for s in sg] for sg in segs]
    if out_file is not None:
        write_mlf(out_file, ret, f_list, ignore_list, "Sample%05d", segments=segs)
    return ret, segs


def decode_extents(pred_out, f_list, quantile=0.5, out_file="final_ctc_recout_extents.mlf"):
    """decode_segments with extents in place of spikes: the greedy decode gives each file's gesture sequence (blank runs
    dropped), decoding.posterior_align its posterior extents - at quantile 0.5 the median extent, near the frames decode_segments
    reports; a smaller quantile widens them to credible extents, which may overlap.  Returns (label-name lists, segment lists of
    (label, first_frame, last_frame, confidence, occupancy))."""
    return decode_extents_mlf(pred_out, f_list, map_gest, ignore_list, "Sample%05d", out_file, THRESHOLD, quantile=quantile)


def decode_beam(pred_out, f_list, lm=None, lm_end=None, alpha=1.0, beta=0.0, beam_width=10, top_paths=1, out_file="final_ctc_recout_beam.mlf"):
    """Beam search with a label bigram and an N-best list (decoding.beam_search_lm_decode): pred_out (N, T, C) softmax - or the
    (paths, score, logp_ctc) that Model.predict_generator(decode="beam_lm", top_paths=top_paths, ...) computed on the device.  lm /
    lm_end as decoding.bigram_lm returns them (None: no prior), weighted alpha, beta per label.  The 1-best path goes through the class
    map into the MLF; returns (1-best name lists, (paths, score, logp_ctc)) - with top_paths > 1 the ranked N-best lists."""
    return decode_beam_mlf(pred_out, f_list, map_gest, ignore_list, "Sample%05d", out_file, top_paths=top_paths, lm=lm, lm_end=lm_end,
                           alpha=alpha, beta=beta, beam_width=beam_width)


def decode_samples(pred_out, f_list, draws=8, seed=0, **kwargs):
    """A sampled hypothesis set per file (decoding.sample_hypotheses): pred_out (N, T, C) softmax - or the (paths, counts)
    that Model.predict_generator(decode="sample", draws=draws, ...) drew on the device.  Returns (per file the name lists of its unique
    sampled labellings in order of first occurrence, through the class map as decode_beam's N-best lists; per file the number of the
    `draws` draws that gave each).  No MLF: a sampled set is no transcription (kwargs: sample_hypotheses')."""
    return decode_samples_map(pred_out, f_list, map_gest, draws=draws, seed=seed, **kwargs)


def decode_score(hyp_ids, ref_ids, costs=HTK_COSTS, confusion=True):
    """HResults-style counts (H, S, D, I, corr, acc, confusion matrix) of decoded label ids against reference label ids on the device,
    "sil" dropped from both (decoding.decode_score_map with this module's class map)."""
    return decode_score_map(hyp_ids, ref_ids, map_gest, costs=costs, confusion=confusion)


def expected_risk(pred_out, paths_or_arrays, ref_ids, costs=HTK_COSTS, **kwargs):
    """The expected edit distance of N-best lists to the reference label ids under the network's own posterior over them, and its
    gradient w.r.t. the Dense logits - the loss of minimum-risk fine-tuning (decoding.expected_risk_map with this module's class map:
    "sil" dropped from both sides, HResults' costs)."""
    return expected_risk_map(pred_out, paths_or_arrays, ref_ids, map_gest, costs=costs, **kwargs)
