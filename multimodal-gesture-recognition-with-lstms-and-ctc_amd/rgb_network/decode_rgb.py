"""Decode for the RGB network (reference rgb_network/decode_rgb.py): plain best-path decoding of out[j, 2:] with repeats collapsed -
the reference's confidence threshold is commented out, so none applies - over the 22 gesture names (index 21 = "sil", kept), and the
MLF writer with the ten-file ignore list."""
import numpy as np

from ..decoding import HTK_COSTS, confidence_filter_collapse, decode_beam_mlf, decode_extents_mlf, decode_samples_map, decode_score_map, expected_risk_map, greedy_segments, write_mlf
from ..keras_like import Model
from ..multimodal_fusion.sequence_decoding import ignore_list, map_gest  # noqa: F401  (the same 22 names and ignore list)
from .cnn_lstm import load_model as _load_model


def load_model(json_path="rgb_ctc_lstm_model.json", weights_path="rgb_ctc_lstm_weights_best.h5", device=0):
    """The trained model and its softmax view (decode_rgb.py: Model(inputs=loaded.input, outputs=loaded.get_layer('softmax').output))."""
    return prediction_model(_load_model(json_path, weights_path, device))


def prediction_model(model):
    return Model(inputs=model.input, outputs=model.get_layer('softmax').output)


def decode_batch(pred_out, f_list, out_file="ctc_recout.mlf"):
    """pred_out (N, T, C) posteriors -> per file the collapsed best-path gesture names of frames 2 ...; writes the MLF."""
    P = np.asarray(pred_out)[:, 2:, :]
    best = P.argmax(axis=2)           # (first index on ties, as mgr_frame_argmax)
    ret = [[map_gest[int(i)] for i in confidence_filter_collapse(best[j], None, None)] for j in range(P.shape[0])]
    nums = [int(str(f)[6:11]) if not isinstance(f, (int, np.integer)) else int(f) for f in f_list]
    write_mlf(out_file, ret, nums, ignore_list, "Sample%05d")
    return ret


def decode_live(model, frames_iter, chunk=20, lookahead=20):
    """decode_segments for a session that is still producing frames (live.decode_live): frames_iter yields {input name:
    [n, F]} pieces at the network rate; yields (name, first_frame, last_frame, confidence) as gestures are finalised, chunk +
    lookahead frames behind the signal.  No confidence filter (it counts over a whole recording).  The RGB network has a CNN front-end, which live sessions do not
    run: open_live refuses it with that message."""
    from ..live import decode_live as _decode_live
    return _decode_live(model, frames_iter, chunk, lookahead, map_gest)


def decode_segments(pred_out, f_list, out_file="ctc_recout_timed.mlf"):
    """decode_batch with start and end times: pred_out (N, T, C) softmax - or the per-sample segment lists that
    Model.predict_generator(decode="segments") computed on the device.  No confidence filter (as decode_batch here); the same
    collapse, class map and ignore list; every MLF line reads "start end name" in HTK's 100 ns units (50 ms per frame).  The times are
    the frames at which the network commits to the class, not the extent of the movement.  Returns (label-name lists, segment lists)."""
    nums = [int(str(f)[6:11]) if not isinstance(f, (int, np.integer)) else int(f) for f in f_list]
    segs = pred_out if isinstance(pred_out, list) else greedy_segments(np.asarray(pred_out), None, skip=2)
    ret = [[map_gest[s[0]] for s in sg] for sg in segs]
    if out_file is not None:
        write_mlf(out_file, ret, nums, ignore_list, "Sample%05d", segments=segs)
    return ret, segs


def decode_extents(pred_out, f_list, quantile=0.5, out_file="ctc_recout_extents.mlf"):
    """decode_segments with extents in place of spikes: the best-path decode (no confidence filter, as decode_batch here)
    gives each file's gesture sequence (blank runs dropped), decoding.posterior_align its posterior extents - at quantile 0.5 the
    median extent, near the frames decode_segments reports; a smaller quantile widens them to credible extents, which may overlap.
    Returns (label-name lists, segment lists of (label, first_frame, last_frame, confidence, occupancy))."""
    nums = [int(str(f)[6:11]) if not isinstance(f, (int, np.integer)) else int(f) for f in f_list]
    return decode_extents_mlf(pred_out, nums, map_gest, ignore_list, "Sample%05d", out_file, None, quantile=quantile)


def decode_beam(pred_out, f_list, lm=None, lm_end=None, alpha=1.0, beta=0.0, beam_width=10, top_paths=1, out_file="ctc_recout_beam.mlf"):
    """Beam search with a label bigram and an N-best list (decoding.beam_search_lm_decode): pred_out (N, T, C) softmax - or the
    (paths, score, logp_ctc) that Model.predict_generator(decode="beam_lm", top_paths=top_paths, ...) computed on the device.  lm /
    lm_end as decoding.bigram_lm returns them (None: no prior), weighted alpha, beta per label.  The 1-best path goes through the class
    map into the MLF; returns (1-best name lists, (paths, score, logp_ctc)) - with top_paths > 1 the ranked N-best lists."""
    f_list = [int(str(f)[6:11]) if not isinstance(f, (int, np.integer)) else int(f) for f in f_list]
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
