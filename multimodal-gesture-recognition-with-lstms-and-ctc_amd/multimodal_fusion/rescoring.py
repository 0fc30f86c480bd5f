"""Late fusion by multiple-hypotheses rescoring (not present in the reference, whose one multimodal result is the fusion
network): the skeletal network's N-best gesture sequences and the audio network's lexicon 1-best are pooled, every pooled hypothesis
is scored by BOTH networks - the audio network through its gesture lexicon -, the scores are combined with stream weights and a
gesture bigram, and the pool is re-ranked.  The CTC likelihood sums over all alignments, so the two streams need neither a common
frame rate nor synchronous gestures."""
import numpy as np

from ..audio_network.sequence_decoding import GESTURE_LEXICON
from ..decoding import beam_search_lm_decode, joint_decode, lexicon_decode, pool_hypotheses, rescore_nbest, write_mlf
from .sequence_decoding import ignore_list, map_gest


def decode_rescoring(skeletal_post, audio_post, f_list, top_paths=10, beam_width=10, weights=(1.0, 1.0), lm=None, lm_end=None, alpha=1.0,
                     beta=0.0, out_file="ctc_recout_rescored.mlf", paths=None):
    """skeletal_post (N, T, 22) gesture posteriors and audio_post (N, T', 44) word posteriors of the same N samples.  The pool per
    sample: the skeletal beam search's top_paths hypotheses (no prior: the bigram enters once, in the combination), then the audio
    network's lexicon 1-best if it is not among them.  lm (22, 21) / lm_end (22,): a bigram over gestures as decoding.phrase_lm_tables
    takes it, weighted alpha; beta per gesture.  The 1-best goes through the fusion module's class map and ignore list into the MLF.
    Either posterior argument may instead be the (N, K) scores Model.rescore_generator computed on the device for the pool `paths`,
    which then has to be given (with both as scores nothing is decoded here).
    Returns (1-best name lists, (ranked paths, total, parts in ranked order))."""
    is_scores = [np.ndim(skeletal_post) == 2, np.ndim(audio_post) == 2]
    if paths is None:
        if any(is_scores):
            raise ValueError("scores computed elsewhere belong to a pool: pass it as paths=")
        nbest = beam_search_lm_decode(np.asarray(skeletal_post), beam_width=max(int(beam_width), int(top_paths)), top_paths=int(top_paths))[0]
        if int(top_paths) == 1:
            nbest = [[p] for p in nbest]
        segs = lexicon_decode(np.asarray(audio_post), GESTURE_LEXICON)[0]
        paths = pool_hypotheses(nbest, [[[s[0] for s in sg]] for sg in segs])
    streams = [(skeletal_post, {}), (audio_post, {"lexicon": GESTURE_LEXICON})]
    ranked, total, parts, _ = rescore_nbest(streams, paths, weights, lm, lm_end, alpha, beta)
    ret = [[map_gest[g] for g in (r[0] if r else [])] for r in ranked]
    if out_file is not None:
        write_mlf(out_file, ret, f_list, ignore_list, "Sample%05d")
    return ret, (ranked, total, parts)


def decode_joint(skeletal_post, audio_post, f_list, top_paths=1, beam_width=10, weights=(1.0, 1.0), lm=None, lm_end=None, alpha=1.0, beta=0.0,
                 max_len=None, out_file="ctc_recout_joint.mlf"):
    """Late fusion by JOINT decoding: one prefix search over gesture sequences in which both networks score every
    extension - the skeletal network gesture g as its class g, the audio network as the words of GESTURE_LEXICON[g] -, so the result
    need not be a sequence either network proposed on its own (decode_rescoring can only re-rank such a pool).  Arguments as
    decode_rescoring's; the same class map, ignore list and MLF writing.
    Returns (1-best name lists, (ranked paths, total, parts))."""
    streams = [(skeletal_post, {}), (audio_post, {"lexicon": GESTURE_LEXICON})]
    ranked, total, parts = joint_decode(streams, len(GESTURE_LEXICON), weights, lm, lm_end, alpha, beta, beam_width, top_paths, max_len)
    ret = [[map_gest[g] for g in (r[0] if r else [])] for r in ranked]
    if out_file is not None:
        write_mlf(out_file, ret, f_list, ignore_list, "Sample%05d")
    return ret, (ranked, total, parts)
