"""Seeded inputs shared by tests/test_cpu_lexicon.py and tests/test_gpu_lexicon.py: the GPU tests decode them, the CPU test checks
on the same inputs that near ties (a search in f32 against one in fp64) are as rare as the GPU tests' allowance assumes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lexicon_ref as lr  # noqa: E402

SKIP = 2
EPS = 1e-8
REF_TOS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 300)      # T - skip of the reference-lexicon cases
TABLE_KINDS = ("zero", "bigram", "grammar")
SMALL_TO = 89                                              # "small T" of the near-tie test


def reference_lexicon():
    from mgr_amd.audio_network.sequence_decoding import GESTURE_LEXICON
    return [list(p) for p in GESTURE_LEXICON]


def tables(rng, G, kind):
    """zero: no tables; bigram: a soft bigram with about 15 % of its entries forbidden; grammar: 0 / -inf entries, half of them
    forbidden, two phrases after which nothing may follow (whole rows -inf) and a fin that forbids ending after a quarter of them."""
    if kind == "zero":
        return None, None
    if kind == "bigram":
        return lr.random_tables(rng, G)
    ext = np.where(rng.random((G + 1, G)) < 0.5, -np.inf, 0.0)
    ext[1 + rng.choice(G, size=min(2, G), replace=False)] = -np.inf
    ext[0, rng.integers(0, G)] = 0.0                        # (some sequence can start)
    fin = np.where(rng.random(G + 1) < 0.25, -np.inf, 0.0)
    return ext, fin


def random_sequence(rng, lexicon, To, max_phrases, ext=None, fin=None):
    """A random phrase sequence whose word expansion fits To frames and which the tables allow (a walk over their finite entries);
    the empty one if no walk ends well.  A planted input must plant a sequence the tables allow: posteriors planted on a forbidden
    one leave the optimum to a many-way exact tie of equally wrong alternatives."""
    G = len(lexicon)
    for _ in range(300):
        m = int(rng.integers(1, max_phrases + 1))
        seq, prev = [], -1
        for _ in range(m):
            allowed = [g for g in range(G) if ext is None or np.isfinite(ext[prev + 1, g])]
            if not allowed:
                break
            prev = int(rng.choice(allowed))
            seq.append(prev)
        if seq and lr.fits(seq, lexicon, To) and (fin is None or np.isfinite(fin[prev + 1])):
            return seq
    assert fin is None or np.isfinite(fin[0]), "the tables allow no sequence that fits"
    return []


def batch(rng, lexicon, Cn, To, B, planted, alpha=0.1, ext=None, fin=None):
    """(P (B, To + SKIP, C) float32, planted sequences or None)."""
    blank = Cn - 1
    if not planted:
        return rng.dirichlet(np.full(Cn, alpha), size=(B, To + SKIP)).astype(np.float32), None
    seqs = [random_sequence(rng, lexicon, To, max(1, min(8, To // 4)), ext, fin) for _ in range(B)]
    return np.stack([lr.planted_case(rng, To, q, lexicon, blank, Cn, SKIP)[0] for q in seqs]), seqs


def reference_cases(tos=REF_TOS, B=5):
    """The reference-lexicon cases: per T - skip, kind of posteriors and kind of tables one batch.  Yields dicts."""
    lex = reference_lexicon()
    Cn = 44
    for To in tos:
        for planted in (True, False):
            for ki, kind in enumerate(TABLE_KINDS):
                rng = np.random.default_rng(1000 * To + 10 * ki + int(planted))
                ext, fin = tables(rng, len(lex), kind)
                P, seqs = batch(rng, lex, Cn, To, B, planted, ext=ext, fin=fin)
                yield {"name": "To=%d %s %s" % (To, "planted" if planted else "dirichlet", kind), "lexicon": lex, "C": Cn, "To": To,
                       "planted": planted, "kind": kind, "P": P, "seqs": seqs, "ext": ext, "fin": fin}


def topology_lexicons():
    """name -> (lexicon, planted sequence or None, table kinds); C = 8, blank = 7."""
    rng = np.random.default_rng(77)
    return {
        "one_word": ([[3]], [0, 0, 0], ("zero", "bigram")),
        # 64 single-word phrases over 7 words: equal phrases tie exactly without a table, so this one runs with a bigram only
        "64_single": ([[int(w)] for w in rng.integers(0, 7, 64)], None, ("bigram",)),
        "16_words_repeat": ([[0, 1, 2, 2, 3, 4, 5, 6, 0, 1, 1, 2, 3, 4, 5, 6]], [0], ("zero", "bigram")),       # a blank inside is mandatory
        "last_equals_first": ([[2, 5, 2], [4]], [0, 0, 1], ("zero", "bigram")),                                  # ... between the phrases
        "prefix": ([[1, 2], [1, 2, 3], [3, 0]], [0, 1, 0, 2], ("zero", "bigram")),
    }


def topology_cases(To=40, B=4):
    Cn = 8
    for i, (name, (lex, seq, kinds)) in enumerate(topology_lexicons().items()):
        for planted in (True, False):
            for ki, kind in enumerate(kinds):
                rng = np.random.default_rng(5000 + 100 * i + 10 * ki + int(planted))
                ext, fin = tables(rng, len(lex), kind)
                if planted:
                    if seq is not None and kind == "bigram":       # the fixed sequences must stay allowed
                        ext, fin = np.where(np.isfinite(ext), ext, -3.0), np.where(np.isfinite(fin), fin, -3.0)
                    seqs = [seq if seq is not None else random_sequence(rng, lex, To, 8, ext, fin) for _ in range(B)]
                    P = np.stack([lr.planted_case(rng, To, q, lex, Cn - 1, Cn, SKIP)[0] for q in seqs])
                else:
                    P, seqs = batch(rng, lex, Cn, To, B, False, alpha=0.3)
                yield {"name": "%s %s %s" % (name, "planted" if planted else "dirichlet", kind), "lexicon": lex, "C": Cn, "To": To,
                       "planted": planted, "kind": kind, "P": P, "seqs": seqs, "ext": ext, "fin": fin}


def capacity_lexicon():
    """255 words in 64 phrases (511 states) over the 63 non-blank classes of C = 64."""
    rng = np.random.default_rng(91)
    return [[int(w) for w in rng.integers(0, 63, 4 if g < 63 else 3)] for g in range(64)]


def capacity_cases(To=40, B=3):
    lex, Cn = capacity_lexicon(), 64
    for planted in (True, False):
        for ki, kind in enumerate(("zero", "bigram")):
            rng = np.random.default_rng(9000 + 10 * ki + int(planted))
            ext, fin = tables(rng, len(lex), kind)
            P, seqs = batch(rng, lex, Cn, To, B, planted, ext=ext, fin=fin)
            yield {"name": "capacity To=%d %s %s" % (To, "planted" if planted else "dirichlet", kind), "lexicon": lex, "C": Cn, "To": To,
                   "planted": planted, "kind": kind, "P": P, "seqs": seqs, "ext": ext, "fin": fin}


def small_cases():
    """Every case above with T - skip <= SMALL_TO."""
    for c in reference_cases(tuple(t for t in REF_TOS if t <= SMALL_TO)):
        yield c
    for c in topology_cases():
        yield c
    for c in capacity_cases():
        yield c
