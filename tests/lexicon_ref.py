"""The lexicon-constrained CTC decode restated in numpy (fp64 by default, no GPU): include/mgr.h's mgr_ctc_lexicon_decode.

token_pass is one Viterbi pass over the state graph of the header, in the kernel's state numbering: with the lexicon's words numbered
j = 0 .. n_words - 1 in phrase order, state 0 = INIT, state 2j + 1 = word j, state 2j + 2 = the blank behind it (B(g, k) inside a
phrase, Z(g) behind its last word).  Back-pointer codes and tie rule are the kernel's: the first maximum of (stay, from s - 1, from
s - 2), for a phrase entry of (stay, INIT, Z(0), last word of 0, Z(1), ...), and the first of the equal final states.
sequence_score scores a GIVEN phrase sequence by the definition: align_ref.viterbi on its word expansion plus the table terms.
"""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as ar  # noqa: E402

NEG_INF = -np.inf


def as_lists(lexicon):
    if isinstance(lexicon, dict):
        lexicon = [lexicon[g] for g in range(len(lexicon))]
    return [[int(w) for w in p] for p in lexicon]


def expand(seq, lexicon):
    lex = as_lists(lexicon)
    return [w for g in seq for w in lex[g]]


def table_terms(seq, G, ext=None, fin=None):
    """sum_i ext[prev_i + 1][g_i] + fin[g_m + 1] in fp64 (0 for a table that is None)."""
    tot, prev = 0.0, -1
    for g in seq:
        if ext is not None:
            tot += float(np.asarray(ext, np.float64)[prev + 1, g])
        prev = g
    if fin is not None:
        tot += float(np.asarray(fin, np.float64)[prev + 1])
    return tot


def sequence_score(logy, seq, lexicon, blank, ext=None, fin=None, cache=None):
    """score(Q) of the header for one phrase sequence; logy (T, C) fp64.  T = 0: only the empty sequence has a score.  cache: a dict
    shared between calls on the same logy (many phrase sequences have the same words)."""
    words = tuple(expand(seq, lexicon))
    if cache is not None and words in cache:
        a = cache[words]
    else:
        if logy.shape[0] == 0:
            a = 0.0 if not words else NEG_INF
        else:
            a = ar.viterbi(logy, list(words), blank)[0]
        if cache is not None:
            cache[words] = a
    t = table_terms(seq, len(as_lists(lexicon)), ext, fin)
    return a + t if a != NEG_INF and t != NEG_INF else NEG_INF


def enumerate_best(logy, lexicon, blank, ext=None, fin=None, max_len=None):
    """The optimum over ALL phrase sequences of at most max_len (default: T) phrases - tiny shapes only."""
    G = len(as_lists(lexicon))
    T = logy.shape[0]
    max_len = T if max_len is None else max_len
    best, cache = NEG_INF, {}
    for m in range(max_len + 1):
        for seq in itertools.product(range(G), repeat=m):
            best = max(best, sequence_score(logy, seq, lexicon, blank, ext, fin, cache))
    return best


class Graph:
    def __init__(self, lexicon, blank):
        lex = as_lists(lexicon)
        self.lex, self.G, self.blank = lex, len(lex), int(blank)
        self.off = np.concatenate([[0], np.cumsum([len(p) for p in lex])]).astype(np.int64)
        words = np.asarray([w for p in lex for w in p], np.int64)
        nw = len(words)
        self.N = N = 1 + 2 * nw
        self.cls = np.full(N, blank, np.int64)
        self.cls[1::2] = words
        phrase_of_word = np.repeat(np.arange(self.G), np.diff(self.off))
        k = np.arange(nw) - self.off[phrase_of_word]
        self.entry_state = 1 + 2 * self.off[:-1]                  # W(g, 0)
        self.wl_state = 2 * self.off[1:] - 1                      # W(g, n_g - 1)
        self.z_state = 2 * self.off[1:]                           # Z(g)
        self.ent = np.full(N, -1, np.int64)
        self.ent[self.entry_state] = np.arange(self.G)
        self.has1 = np.ones(N, bool)
        self.has1[0] = False
        self.has1[self.entry_state] = False
        self.has2 = np.zeros(N, bool)
        inner = np.flatnonzero(k > 0)
        self.has2[1 + 2 * inner] = words[inner] != words[inner - 1]
        self.diff = words[self.off[1:] - 1][:, None] != words[self.off[:-1]][None, :]      # [g', g]: last word of g' != first of g
        self.fin_state = np.concatenate([[0], np.stack([self.wl_state, self.z_state], 1).reshape(-1)])
        self.fin_index = np.concatenate([[0], np.repeat(np.arange(self.G) + 1, 2)])
        order = np.argsort(self.fin_state, kind="stable")         # final states in state order: the first maximum wins
        self.fin_state, self.fin_index = self.fin_state[order], self.fin_index[order]


def token_pass(logy, lexicon, blank, ext=None, fin=None, dtype=np.float64):
    """logy (T, C).  Returns (score, phrase sequence, states (T,)) - score includes the table terms, in dtype arithmetic - or
    (-inf, None, None) when no sequence has a finite score."""
    gr = lexicon if isinstance(lexicon, Graph) else Graph(lexicon, blank)
    G, N = gr.G, gr.N
    logy = np.asarray(logy, dtype)
    T = logy.shape[0]
    ext = np.zeros((G + 1, G), dtype) if ext is None else np.asarray(ext).astype(dtype)
    fin = np.zeros(G + 1, dtype) if fin is None else np.asarray(fin).astype(dtype)
    v = np.full(N, NEG_INF, dtype)
    bp = np.zeros((T, N), np.int16)
    idx = np.arange(N)
    with np.errstate(invalid="ignore"):
        if T == 0:
            v[0] = 0.0
        else:
            v[0] = logy[0, gr.blank]
            v[gr.entry_state] = ext[0] + logy[0, gr.cls[gr.entry_state]]
        for t in range(1, T):
            c = np.full((3, N), NEG_INF, dtype)
            c[0] = v
            c[1, 1:] = np.where(gr.has1[1:], v[:-1], NEG_INF)
            c[2, 2:] = np.where(gr.has2[2:], v[:-2], NEG_INF)
            step = np.argmax(c, axis=0)
            m = c[step, idx]
            # phrase entries: [stay, INIT, Z(0), Wl(0), Z(1), Wl(1), ...] per entered phrase g (columns)
            ce = np.full((2 + 2 * G, G), NEG_INF, dtype)
            ce[0] = v[gr.entry_state]
            ce[1] = v[0] + ext[0]
            ce[2::2] = v[gr.z_state][:, None] + ext[1:]
            ce[3::2] = np.where(gr.diff, v[gr.wl_state][:, None] + ext[1:], NEG_INF)
            es = np.argmax(ce, axis=0)
            step[gr.entry_state] = es
            m[gr.entry_state] = ce[es, np.arange(G)]
            bp[t] = step
            v = (m + logy[t, gr.cls]).astype(dtype)
        f = v[gr.fin_state] + fin[gr.fin_index]
    if np.isnan(f).any():
        f = np.where(np.isnan(f), NEG_INF, f)
    q = int(np.argmax(f))
    if f[q] == NEG_INF:
        return NEG_INF, None, None
    s = int(gr.fin_state[q])
    states = np.zeros(T, np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        code = int(bp[t, s])
        if gr.ent[s] < 0:
            s -= code
        elif code == 1:
            s = 0
        elif code >= 2:
            gp = (code - 2) >> 1
            s = int(gr.wl_state[gp] if code & 1 else gr.z_state[gp])
    return float(f[q]), states_to_phrases(states, gr), states


def states_to_phrases(states, gr):
    seq = []
    for t, s in enumerate(states):
        if gr.ent[s] >= 0 and (t == 0 or states[t - 1] != s):
            seq.append(int(gr.ent[s]))
    return seq


def states_to_path(states, gr):
    return gr.cls[states]


def path_phrase_segments(path, seq, lexicon, blank, skip=2):
    """(first, last) original frame indices of each phrase of seq in a frame path whose collapse is seq's word expansion: the first
    frame of the phrase's first word, the last frame of its last word."""
    lex = as_lists(lexicon)
    runs = ar.path_segments(path, blank, skip)                 # one (label, first, last) per word
    out, i = [], 0
    for g in seq:
        n = len(lex[g])
        assert [r[0] for r in runs[i:i + n]] == lex[g]
        out.append((runs[i][1], runs[i + n - 1][2]))
        i += n
    assert i == len(runs)
    return out


def phrase_conf(P, path, segs, blank, skip=2):
    """fp64 mean of P[t, emitted word] over the non-blank frames of each (first, last) segment."""
    P = np.asarray(P, np.float64)
    out = []
    for f, l in segs:
        ts = [t for t in range(f, l + 1) if path[t - skip] != blank]
        out.append(float(np.mean([P[t, path[t - skip]] for t in ts])))
    return out


def decode(P, lexicon, blank, ext=None, fin=None, skip=2, eps=1e-8, input_len=None, dtype=np.float64):
    """One sample, P (T, C) float32: the restatement end to end.  Returns a dict: seq (None when infeasible), score, logp, path,
    seg, conf - score and logp re-evaluated in fp64 along the returned path, whatever dtype the search ran in."""
    gr = Graph(lexicon, blank)
    To = P.shape[0] - skip
    Tp = To if input_len is None else max(0, min(int(input_len), To))
    logy = ar.log_emissions(P[:Tp + skip], skip, eps)
    sc, seq, states = token_pass(logy, gr, blank, ext, fin, dtype)
    if seq is None:
        return {"seq": None, "score": NEG_INF, "logp": NEG_INF, "path": None, "seg": [], "conf": []}
    path = states_to_path(states, gr)
    logp = ar.path_score(logy, path) if Tp else 0.0
    segs = path_phrase_segments(path, seq, lexicon, blank, skip)
    return {"seq": seq, "score": logp + table_terms(seq, gr.G, ext, fin), "logp": logp, "path": path, "seg": segs,
            "conf": phrase_conf(P, path, segs, blank, skip), "search_score": sc}


def random_tables(rng, G, p_forbid=0.15, with_fin=True):
    """A random soft bigram with about p_forbid of its entries -inf."""
    ext = rng.normal(-2.0, 1.5, size=(G + 1, G))
    ext[rng.random((G + 1, G)) < p_forbid] = NEG_INF
    fin = None
    if with_fin:
        fin = rng.normal(-2.0, 1.5, size=G + 1)
        fin[rng.random(G + 1) < p_forbid] = NEG_INF
    return ext, fin


def planted_case(rng, To, seq, lexicon, blank, Cn, skip=2, hi=0.9):
    """Posteriors with hi on a randomly drawn valid alignment of seq's word expansion.  Returns (P (To + skip, C) float32, states of
    align_ref's extended label sequence)."""
    words = expand(seq, lexicon)
    st = ar.planted_alignment(rng, To, words, blank)
    return ar.planted_posteriors(st, words, blank, Cn, skip, hi), st


def fits(seq, lexicon, To):
    """Frames the word expansion needs: one per word plus a blank between equal neighbours."""
    w = expand(seq, lexicon)
    return len(w) + sum(a == b for a, b in zip(w, w[1:])) <= To
