"""Decode for the audio network (reference audio_network/sequence_decoding.py:19-69): word-level classes, thr .75."""
import numpy as np

from ..decoding import (HTK_COSTS, decode_beam_mlf, decode_extents_lexicon_mlf, decode_lexicon_mlf, decode_samples_map, decode_score_map, expected_risk_map, greedy_decode,
                        greedy_decode_argmax, greedy_segments, write_mlf)
from .data_generator import class_2_words

_words = ["oov", "Vattene", "Vieni", "qui", "Perfetto", "E'", "un", "furbo", "Che", "due", "palle", "vuoi", "Vanno",
          "d'accordo", "Sei", "Pazzo", "Cos'hai", "combinato", "Non", "me", "ne", "frega", "niente", "ok", "Cosa", "ti",
          "farei", "Basta", "Le", "prendere", "ce", "n'e", "piu", "Ho", "fame", "Tanto", "tempo", "fa", "Buonissimo",
          "Si", "sono", "messi", "stufo", "sil"]
map_gest = dict(enumerate(_words))
map_gest[-1] = "sil"
ignore_list = [228, 298, 299, 300, 303, 304, 334, 343, 373, 375]
THRESHOLD = 0.75
# The gestures behind the words: gesture class g is spoken as the words GESTURE_LEXICON[g] (what DataGenerator.sent_2_words expands
# the labels with); class 21 is the blank itself and no phrase.  Names: the ChaLearn 2013 gesture codes listed in the reference
# (audio_network/data_generator.py:126-128).
GESTURE_LEXICON = [list(class_2_words[g]) for g in range(21)]
gesture_names = ["oov", "VA", "VQ", "PF", "FU", "CP", "CV", "DC", "SP", "CN", "FN", "OK", "CF", "BS", "PR", "NU", "FM", "TT", "BN", "MC", "ST"]


def decode_batch(pred_out, f_list, out_file="ctc_recout.mlf"):
    ids = greedy_decode(np.asarray(pred_out), THRESHOLD, skip=2)
    ret = [[map_gest[i] for i in seq] for seq in ids]
    write_mlf(out_file, ret, f_list, ignore_list, "Sample%05d_audio")
    return ret


def decode_argmax(best, prob, f_list, out_file=None):
    """decode_batch from the per-frame (best label, probability) pairs that Model.predict_generator(decode="argmax") computes
    on the device: same filter, same collapse, same MLF."""
    ids = greedy_decode_argmax(best, prob, THRESHOLD)
    ret = [[map_gest[i] for i in seq] for seq in ids]
    if out_file is not None:
        write_mlf(out_file, ret, f_list, ignore_list, "Sample%05d_audio")
    return ret


def decode_live(model, frames_iter, chunk=20, lookahead=20):
    """decode_segments for a session that is still producing frames (live.decode_live): frames_iter yields {input name:
    [n, F]} pieces at the network rate; yields (name, first_frame, last_frame, confidence) as gestures are finalised, chunk +
    lookahead frames behind the signal.  No confidence filter (it counts over a whole recording)."""
    from ..live import decode_live as _decode_live
    return _decode_live(model, frames_iter, chunk, lookahead, map_gest)


def decode_segments(pred_out, f_list, out_file="ctc_recout_timed.mlf"):
    """decode_batch with start and end times: pred_out (N, T, C) softmax - or the per-sample segment lists that
    Model.predict_generator(decode="segments", threshold=THRESHOLD) computed on the device.  The same filter, collapse, class map and
    ignore list; every MLF line reads "start end name" in HTK's 100 ns units (50 ms per frame).  The times are the frames at which the
    network commits to the class, not the extent of the movement.  Returns (label-name lists, segment lists)."""
    segs = pred_out if isinstance(pred_out, list) else greedy_segments(np.asarray(pred_out), THRESHOLD, skip=2)
    ret = [[map_gest[s[0]] for s in sg] for sg in segs]
    if out_file is not None:
        write_mlf(out_file, ret, f_list, ignore_list, "Sample%05d_audio", segments=segs)
    return ret, segs


def decode_beam(pred_out, f_list, lm=None, lm_end=None, alpha=1.0, beta=0.0, beam_width=10, top_paths=1, out_file="ctc_recout_beam.mlf"):
    """Beam search with a label bigram and an N-best list (decoding.beam_search_lm_decode): pred_out (N, T, C) softmax - or the
    (paths, score, logp_ctc) that Model.predict_generator(decode="beam_lm", top_paths=top_paths, ...) computed on the device.  lm /
    lm_end as decoding.bigram_lm returns them (None: no prior), weighted alpha, beta per label.  The 1-best path goes through the class
    map into the MLF; returns (1-best name lists, (paths, score, logp_ctc)) - with top_paths > 1 the ranked N-best lists."""
    return decode_beam_mlf(pred_out, f_list, map_gest, ignore_list, "Sample%05d_audio", out_file, top_paths=top_paths, lm=lm, lm_end=lm_end,
                           alpha=alpha, beta=beta, beam_width=beam_width)


def decode_lexicon(pred_out, f_list, lm=None, lm_end=None, alpha=1.0, beta=0.0, out_file="ctc_recout_gestures.mlf"):
    """Gestures from the word posteriors (decoding.lexicon_decode over GESTURE_LEXICON): pred_out (N, T, C) softmax - or the
    (segments, score, logp) that Model.predict_generator(decode="lexicon", lexicon=GESTURE_LEXICON, ...) computed on the device.  lm /
    lm_end: a bigram over gestures as decoding.phrase_lm_tables takes it (None: no prior).  Every MLF line reads "start end gesture" in
    HTK's 100 ns units, from the first frame of the gesture's first word to the last frame of its last word.  Returns (gesture-name
    lists, segment lists of (gesture id, first_frame, last_frame, confidence))."""
    return decode_lexicon_mlf(pred_out, f_list, GESTURE_LEXICON, gesture_names, ignore_list, "Sample%05d_audio", out_file, lm=lm,
                              lm_end=lm_end, alpha=alpha, beta=beta)


def decode_extents(pred_out, f_list, quantile=0.5, out_file="ctc_recout_gesture_extents.mlf", lm=None, lm_end=None, alpha=1.0, beta=0.0):
    """decode_lexicon with extents in place of the Viterbi path's frames: decode_lexicon's phrases give each file's gesture
    sequence, decoding.posterior_align the posterior extents of their word expansion at `quantile`; a gesture's extent runs from its
    first word's first frame to its last word's last frame (grouped on the host).  Returns (gesture-name lists, segment lists of
    (gesture id, first_frame, last_frame, confidence, occupancy))."""
    return decode_extents_lexicon_mlf(pred_out, f_list, GESTURE_LEXICON, gesture_names, ignore_list, "Sample%05d_audio", out_file,
                                      quantile=quantile, lm=lm, lm_end=lm_end, alpha=alpha, beta=beta)


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
