"""Planted and seeded inputs of the joint-decode tests (mgr_ctc_joint_decode, K19).  A case is a dict: name, streams (list of dict(P
(B, T, C) float32, il (B,) or None, skip, blank, eps, lexicon or None, weight)), G, ext / fin (or None), beam, top_paths, max_len.
tests/test_cpu_joint.py asserts that every case of gpu_cases() but the tie case has a decision margin of at least MARGIN under the
fp64 restatement; a seed that fails it is replaced HERE."""
import numpy as np

SKIP, EPS = 2, 1e-8
MARGIN = 1e-6
REL = 1e-12           # score / logp against the restatement: tests/test_gpu_beam_lm.py's bound for the fp64 search
REL_LONG = 1e-9       # at T = 1900: at most 3 x 1900 x 40 rounded fp64 operations per score at 1e-15 each is 2.3e-10
REL_SHIPPED = 1e-4    # against mgr_ctc_rescore (f32 recursion): tests/rescore_cases.py's REL
TIE = "tie"

# the reference's gestures as word phrases (audio_network/data_generator.py: class_2_words), as the product states them
def gesture_lexicon():
    from mgr_amd.audio_network.sequence_decoding import GESTURE_LEXICON
    return [list(p) for p in GESTURE_LEXICON]


def stream(P, lexicon=None, il=None, skip=SKIP, blank=None, eps=EPS, weight=1.0):
    P = np.ascontiguousarray(P, np.float32)
    return dict(P=P, il=None if il is None else np.asarray(il, np.int32), skip=skip, blank=P.shape[2] - 1 if blank is None else blank, eps=eps,
                lexicon=lexicon, weight=weight)


def dirichlet(rng, B, T, Cn, conc=0.4):
    return rng.dirichlet(np.full(Cn, conc), size=(B, T)).astype(np.float32)


def peaky(rng, T, Cn, blank, classes, skip=SKIP, hi=3.0, lo=0.02, jitter=True):
    """(T, C) posteriors with the classes planted at even distances (two frames each, a blank frame before a repeat), blank elsewhere."""
    P = np.full((T, Cn), lo)
    P[:, blank] = 1.0
    To = T - skip
    if classes:
        pos = np.linspace(1, To - 3, len(classes)).astype(int) + skip
        for p, c in zip(pos, classes):
            P[p, c], P[p + 1, c] = hi, 0.67 * hi
    if jitter:
        P = P * rng.uniform(0.5, 1.5, P.shape)
    return (P / P.sum(axis=1, keepdims=True)).astype(np.float32)


def expand(seq, lexicon):
    return [w for g in seq for w in lexicon[g]]


SMALL_LEXICON = [[0, 1], [1, 1], [2, 0], [2, 3], [4]]         # a repeated word inside a phrase; boundary words that meet: 0|0, 1|1, 2|2


def case(name, streams, G, beam, top_paths, max_len, ext=None, fin=None):
    return dict(name=name, streams=streams, G=G, beam=beam, top_paths=top_paths, max_len=max_len, ext=ext, fin=fin)


def tables(rng, G, p_forbid=0.15, with_fin=True, shift=-0.5):
    """A soft bigram with some entries -inf and some positive (the stop's bound U_n is then not zero)."""
    ext = rng.normal(shift, 1.0, size=(G + 1, G))
    ext[rng.random((G + 1, G)) < p_forbid] = -np.inf
    fin = None
    if with_fin:
        fin = rng.normal(shift, 1.0, size=G + 1)
        fin[rng.random(G + 1) < p_forbid] = -np.inf
    return ext, fin


def shape_cases():
    """The shape cases of the equality test, T <= 64."""
    out = []
    rng = np.random.default_rng(1920)         # (1901: the Tp = 2 sample's best live prefix fills both frames, so its pre IS the list's
    #                                            worst score - an exact tie in the stop test; replaced)
    # one stream, no lexicon, ragged lengths with Tp = 0, 1, 2 (and a length above T - skip), B = 5
    out.append(case("m1_ragged", [stream(dirichlet(rng, 5, 22, 6), il=[20, 0, 1, 2, 1000])], 5, 4, 3, 6))
    # two streams: G < C - 1 without a lexicon and a blank inside the gesture range (gesture 2 has probability 0 there), own skips
    rng = np.random.default_rng(1902)
    out.append(case("m2_lexicon", [stream(dirichlet(rng, 3, 19, 8), skip=1, blank=2),
                                   stream(dirichlet(rng, 3, 27, 6), SMALL_LEXICON, il=[25, 11, 25], weight=0.7)], 5, 5, 5, 4))
    # three streams, two lexicons, weights, tables with -inf and positive entries
    rng = np.random.default_rng(1903)
    ext, fin = tables(rng, 5)
    out.append(case("m3_tables", [stream(dirichlet(rng, 2, 16, 6)), stream(dirichlet(rng, 2, 24, 6), SMALL_LEXICON, weight=0.7),
                                  stream(dirichlet(rng, 2, 12, 7, 0.6), [[0], [1], [2], [3], [5]], skip=0, weight=0.5)], 5, 3, 2, 5, ext, fin))
    # G = 1, beam 1 and 2
    rng = np.random.default_rng(1904)
    out.append(case("g1_beam1", [stream(dirichlet(rng, 2, 9, 3, 1.0))], 1, 1, 1, 5))
    out.append(case("g1_beam2", [stream(dirichlet(rng, 2, 9, 3, 1.0))], 1, 2, 2, 5))
    # T - skip = 1: the empty hypothesis and single gestures are all there is - fewer survivors than top_paths
    rng = np.random.default_rng(1905)
    out.append(case("one_frame", [stream(dirichlet(rng, 1, 3, 5)), stream(dirichlet(rng, 1, 4, 5), il=[1], skip=3)], 3, 8, 8, 4))
    # the reference's 21 gestures on 22 / 44 classes, three planted, B = 2
    rng = np.random.default_rng(1906)
    lex = gesture_lexicon()
    truth = [[3, 17, 8], [11, 11, 0]]
    sk = np.stack([peaky(rng, 40, 22, 21, t, lo=1e-3) for t in truth])
    au = np.stack([peaky(rng, 64, 44, 43, expand(t, lex), lo=1e-3) for t in truth])
    out.append(case("gestures21", [stream(sk), stream(au, lex)], 21, 10, 4, 8))
    # the widest beam, top_paths 8; and max_len reached before the stop
    rng = np.random.default_rng(1907)
    out.append(case("beam32", [stream(dirichlet(rng, 2, 14, 6)), stream(dirichlet(rng, 2, 20, 6), SMALL_LEXICON)], 5, 32, 8, 3))
    rng = np.random.default_rng(1908)
    out.append(case("max_len", [stream(np.stack([peaky(rng, 30, 5, 4, [0, 1, 2, 3, 0, 1])]))], 4, 3, 2, 3))
    # a bigram that forbids most transitions: fewer finite hypotheses than top_paths; a sample with none (fin forbids everything)
    rng = np.random.default_rng(1909)
    ext = np.full((4, 3), -np.inf)
    ext[0, 1], ext[2, 0], ext[1, 2] = -0.3, 0.4, -1.0
    out.append(case("hard_grammar", [stream(dirichlet(rng, 2, 12, 4))], 3, 4, 4, 5, ext, np.array([-0.2, 0.1, -np.inf, 0.3])))
    out.append(case("nothing_finite", [stream(dirichlet(rng, 2, 8, 4))], 3, 2, 2, 3, None, np.full(4, -np.inf)))
    return out


def tie_case():
    """Classes 0 and 1 are the same column: extending by gesture 0 and by gesture 1 is the same arithmetic on the same numbers.  The
    smaller gesture wins every cut."""
    rng = np.random.default_rng(1910)
    P = dirichlet(rng, 2, 14, 5)
    P[:, :, 1] = P[:, :, 0]
    return case(TIE, [stream(P)], 4, 3, 3, 4)


def long_case():
    """T = 1900 on both streams, 22 / 44 classes, the reference's lexicon, ten planted gestures, B = 2."""
    rng = np.random.default_rng(1911)
    lex = gesture_lexicon()
    truth = [[int(v) for v in rng.integers(0, 21, 10)] for _ in range(2)]
    sk = np.stack([peaky(rng, 1900, 22, 21, t, lo=1e-6) for t in truth])
    au = np.stack([peaky(rng, 1900, 44, 43, expand(t, lex), lo=1e-6) for t in truth])
    c = case("long", [stream(sk), stream(au, lex)], 21, 10, 4, 12)
    c["truth"] = truth
    return c


def slots(rng, T, Cn, blank, options, skip=SKIP, lo=2e-4):
    """(T, C) posteriors: the frames behind skip in len(options) equal slots, in each the words of every (words, height) option
    planted at even distances (two frames a word), blank elsewhere."""
    P = np.full((T, Cn), lo)
    P[:, blank] = 1.0
    n = (T - skip) // len(options)
    for i, opts in enumerate(options):
        for words, height in opts:
            for p, c in zip(np.linspace(1, n - 3, len(words)).astype(int) + skip + i * n, words):
                P[p, c] += height
                P[p + 1, c] += 0.67 * height
    P = P * rng.uniform(0.9, 1.1, P.shape)          # (no two columns alike: no exact ties)
    return (P / P.sum(axis=1, keepdims=True)).astype(np.float32)


def pool_miss_case():
    """Three gestures.  The skeletal stream is sure of gestures 1 and 2 and prefers two wrong third ones; the audio stream is sure of 2
    and 3 and prefers a wrong first one.  Neither stream's short list holds the truth; the sum of the two streams does."""
    lex = gesture_lexicon()
    truth, sk_wrong, sk_wrong2, au_wrong = [4, 9, 14], [4, 9, 2], [4, 9, 6], [7, 9, 14]
    rng = np.random.default_rng(1912)
    sk = slots(rng, 40, 22, 21, [[([4], 3.0)], [([9], 3.0)], [([2], 3.0), ([6], 2.4), ([14], 1.5)]])[None]
    au = slots(rng, 64, 44, 43, [[(lex[7], 3.0), (lex[4], 1.5)], [(lex[9], 3.0)], [(lex[14], 3.0)]])[None]
    c = case("pool_miss", [stream(sk), stream(au, lex)], 21, 10, 2, 6)
    c.update(truth=truth, sk_wrong=sk_wrong, sk_wrong2=sk_wrong2, au_wrong=au_wrong)
    return c


def gpu_cases():
    return shape_cases() + [tie_case(), long_case(), pool_miss_case()]
