// K19: joint decode over several CTC streams (not present in the reference): a label-synchronous prefix search over gesture
// sequences that every stream scores at every step - Graves' prefix search with the CTC prefix score (include/mgr.h states the
// recursion and the search).  The streams share nothing but the gesture alphabet: frame counts, class sets, blanks, skips differ.
//
// Two kernels.  k_joint_emissions, once per stream: class-major ln y rows per sample in fp64.  k_joint: ONE WORKGROUP per sample that
// loops over the rounds.  A round of `live` prefixes is live * G * M independent chains of Tp_m dependent steps, three fp64
// log-sum-exp per word and step: latency, not throughput.
//   pass A   a thread per (stream, prefix r, gesture g) - the streams on whole waves (a wave walks one stream's frames), inside a wave
//            the G gestures of a prefix side by side, so the parent's gn / gb loads are broadcasts.  A gesture's words advance in one
//            loop over t with the t - 1 values in registers (word j at t needs word j - 1 at t - 1: updated from the last word down).
//            Emissions and the parent's values are fetched a step ahead.  Kept: ln psi and ln p, in the workspace.
//   select   pre = sum_m w_m ln psi_m + the table terms in LDS; `beam` rounds of wave arg-max by wave 0, ties to the smaller
//            candidate index r * G + g (k_beam's loop).
//   pass B   the <= beam kept chains run again, a wave per stream, and store their gn / gb into the other half of the ping-pong
//            buffer: the arrays of all live * G candidates are never stored.  Skipped when the round is the last.
// The empty prefix needs no arrays: its gb is the running sum of ln y(blank), which the chain carries anyway.
// The result list (<= top_paths entries) lives in LDS, unordered with an arrival number; an entry replaces the worst when it is
// strictly better; ranked at the end by (score, arrival).  Everything a decision reads is fp64.
#include "ctc_lattice.h"
#include "wave_f64.h"

namespace {

constexpr int MAXW = 32;                             // beam width limit
constexpr int MAXG = MGR_LEXICON_MAX_PHRASES;
constexpr int MAXM = MGR_JOINT_MAX_STREAMS;
constexpr int MAXLEN = MGR_RESCORE_MAX_LABELS + 1;   // bytes per stored sequence
constexpr int JNT = 512;                             // threads of k_joint: 8 waves, two per SIMD

static_assert(MAXM == kJointMaxStreams, "ws_layout.h");
static_assert(MAXG <= 256 && MGR_LEXICON_MAX_WORDS <= 255, "gesture ids and lexicon offsets are kept as bytes");

struct JtStream {
  const double* E;   // [B][C][row]
  double* A;         // [B][2][beam][2][row]
  const int32_t* input_len;
  double w;
  int T, C, skip, blank, lex, nwmax;
};
struct JtArgs {
  JtStream s[MAXM];
  LexArg lex[MAXM];
};

// ln y(t, c) = ln(P + eps) - ln(sum_c (P + eps)) in fp64, class-major rows of length TS; zeros from the sample's length on
__global__ __launch_bounds__(256) void k_joint_emissions(const float* __restrict__ P, const int32_t* __restrict__ input_len, int T, int C, int skip,
                                                         float eps, size_t TS, double* __restrict__ E) {
  const int b = blockIdx.y, To = T - skip;
  const int Tp = clip_len(input_len[b], To);
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= TS) return;
  double* Eb = E + (size_t)b * C * TS;
  if (t >= (size_t)Tp) {
    for (int c = 0; c < C; ++c) Eb[(size_t)c * TS + t] = 0.0;
    return;
  }
  const float* row = P + ((size_t)b * T + skip + t) * C;
  double s = 0.0;
  for (int c = 0; c < C; ++c) s += (double)row[c] + (double)eps;
  const double ls = log(s);
  for (int c = 0; c < C; ++c) Eb[(size_t)c * TS + t] = log((double)row[c] + (double)eps) - ls;
}

struct Chain { double psi, lp; };

// One gesture (n <= NW words: wd[0 .. n - 1], or the class g where wd is null) appended to a prefix, over the Tp frames of one stream
// of one sample.  Eb: the sample's emission rows; plast: the prefix' last class, -1 for the empty prefix; pgn / pgb: the prefix'
// arrays (null: the empty prefix); STORE: the gesture's arrays go to ogn / ogb.  Rows hold one entry behind Tp (fetched, not used).
template <int NW, bool STORE>
__device__ __forceinline__ Chain jt_chain(const double* __restrict__ Eb, size_t TS, int Tp, int blank, const unsigned char* wd, int g, int n,
                                          int plast, const double* __restrict__ pgn, const double* __restrict__ pgb, double* __restrict__ ogn,
                                          double* __restrict__ ogb) {
  Chain r;
  r.psi = r.lp = kNegInfD;
  if (Tp <= 0) return r;
  const double* er[NW];
  bool same[NW];   // word j equals the class before it (j = 0: the prefix' last): no step over the blank
  {
    int prev = plast;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const int c = j < n ? (wd ? (int)wd[j] : g) : blank;
      er[j] = Eb + (size_t)c * TS;
      same[j] = c == prev;
      prev = c;
    }
  }
  const double* ebr = Eb + (size_t)blank * TS;
  const bool pe = pgn == nullptr;
  double hn[NW], hb[NW], en[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) hn[j] = hb[j] = kNegInfD;
  // t = 0
  hn[0] = pe ? er[0][0] : kNegInfD;
  double psi = n == 1 ? hn[0] : kNegInfD;
  double cumb = ebr[0];   // the empty prefix' gb
  if (STORE) {
    ogn[0] = psi;
    ogb[0] = kNegInfD;
  }
  double pn = pe ? kNegInfD : pgn[0], pb = pe ? kNegInfD : pgb[0];   // the prefix at t - 1
  double ebn = ebr[1];
#pragma unroll
  for (int j = 0; j < NW; ++j) en[j] = er[j][1];
  for (int t = 1; t < Tp; ++t) {
    const double eb = ebn;
    double e[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) e[j] = en[j];
    double pnn = kNegInfD, pbn = kNegInfD;
    if (!pe) {
      pnn = pgn[t];
      pbn = pgb[t];
    }
    ebn = ebr[t + 1];
#pragma unroll
    for (int j = 0; j < NW; ++j) en[j] = er[j][t + 1];
    const double phi0 = pe ? cumb : lse64(pb, same[0] ? kNegInfD : pn);
#pragma unroll
    for (int j = NW - 1; j >= 0; --j) {
      if (j < n) {
        const double phi = j == 0 ? phi0 : lse64(hb[j > 0 ? j - 1 : 0], same[j] ? kNegInfD : hn[j > 0 ? j - 1 : 0]);
        const double nn = lse64(hn[j], phi) + e[j];
        const double nb = lse64(hb[j], hn[j]) + eb;
        if (j == n - 1) {
          psi = lse64(psi, phi + e[j]);
          if (STORE) {
            ogn[t] = nn;
            ogb[t] = nb;
          }
        }
        hn[j] = nn;
        hb[j] = nb;
      }
    }
    cumb += eb;
    pn = pnn;
    pb = pbn;
  }
  double fn = kNegInfD, fb = kNegInfD;
#pragma unroll
  for (int j = 0; j < NW; ++j)
    if (j == n - 1) {
      fn = hn[j];
      fb = hb[j];
    }
  r.psi = psi;
  r.lp = lse64(fn, fb);
  return r;
}

template <bool STORE>
__device__ __forceinline__ Chain jt_run(int nwmax, const double* Eb, size_t TS, int Tp, int blank, const unsigned char* wd, int g, int n, int plast,
                                        const double* pgn, const double* pgb, double* ogn, double* ogb) {
  if (nwmax <= 1) return jt_chain<1, STORE>(Eb, TS, Tp, blank, wd, g, n, plast, pgn, pgb, ogn, ogb);
  if (nwmax <= 2) return jt_chain<2, STORE>(Eb, TS, Tp, blank, wd, g, n, plast, pgn, pgb, ogn, ogb);
  if (nwmax <= 4) return jt_chain<4, STORE>(Eb, TS, Tp, blank, wd, g, n, plast, pgn, pgb, ogn, ogb);
  return jt_chain<MGR_JOINT_MAX_PHRASE_WORDS, STORE>(Eb, TS, Tp, blank, wd, g, n, plast, pgn, pgb, ogn, ogb);
}

// grid B, JNT threads; dynamic LDS: ext [(G + 1) * G] and the candidates' pre [beam * G], doubles
__global__ __launch_bounds__(JNT) void k_joint(const JtArgs a, int M, int G, const double* __restrict__ ext, const double* __restrict__ fin, int beam,
                                               int NP, int max_len, double* __restrict__ PSI, double* __restrict__ LP, int32_t* __restrict__ out,
                                               int32_t* __restrict__ out_len, double* __restrict__ score, double* __restrict__ logp,
                                               int32_t* __restrict__ rounds) {
  extern __shared__ double s_dyn[];
  double* s_ext = s_dyn;
  double* s_cpre = s_dyn + (size_t)(G + 1) * G;
  __shared__ JtStream s_st[MAXM];
  __shared__ unsigned char s_off[MAXM][MAXG + 1], s_words[MAXM][MGR_LEXICON_MAX_WORDS + 1];
  __shared__ unsigned char s_seq[2][MAXW][MAXLEN], s_rseq[MAXW][MAXLEN];
  __shared__ double s_lm[2][MAXW], s_lpre[MAXW], s_fl[MAXW], s_flp[MAXW][MAXM], s_rscore[MAXW], s_rlp[MAXW][MAXM], s_selpre[MAXW];
  __shared__ double s_red[JNT], s_u[3];   // s_u: max(0, largest ext), max(0, largest fin), the list's worst score
  __shared__ int s_last[2][MAXW], s_sel[MAXW], s_rlen[MAXW], s_rord[MAXW], s_src[MAXW], s_tp[MAXM];
  __shared__ int s_nsel, s_cnt;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t NCmax = (size_t)beam * G;
  double* PSIb = PSI + (size_t)b * M * NCmax;
  double* LPb = LP + (size_t)b * M * NCmax;

  // ---- streams, lexicons and tables into LDS
#pragma unroll
  for (int m = 0; m < MAXM; ++m) {
    if (m < M) {
      if (tid == m) s_st[m] = a.s[m];
      if (a.s[m].lex) {
        for (int i = tid; i <= G; i += JNT) s_off[m][i] = a.lex[m].off[i];
        for (int i = tid; i <= MGR_LEXICON_MAX_WORDS; i += JNT) s_words[m][i] = a.lex[m].words[i];
      }
    }
  }
  double mx = kNegInfD;
  for (int i = tid; i < (G + 1) * G; i += JNT) {
    const double e = ext[i];
    s_ext[i] = e;
    mx = e > mx ? e : mx;
  }
  s_red[tid] = mx;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < JNT; ++i) mx = s_red[i] > mx ? s_red[i] : mx;
    s_u[0] = mx > 0.0 ? mx : 0.0;
    double fm = 0.0;
    if (fin)
      for (int i = 0; i <= G; ++i) fm = fin[i] > fm ? fin[i] : fm;
    s_u[1] = fm;
  }
  // ---- round 0: the empty prefix is live; the empty hypothesis' ln p per stream is the sum of ln y(blank)
  if (tid < M) {
    const JtStream st = s_st[tid];
    const int To = st.T - st.skip;
    const int Tp = clip_len(st.input_len[b], To);
    s_tp[tid] = Tp;
    const double* eb = st.E + ((size_t)b * st.C + st.blank) * mgr_joint_row(To);
    double c = 0.0;
    for (int t = 0; t < Tp; ++t) c += eb[t];
    s_flp[0][tid] = c;
  }
  __syncthreads();
  if (tid == 0) {
    double sc = 0.0;
    for (int m = 0; m < M; ++m) sc += s_st[m].w * s_flp[0][m];
    sc += 0.0;
    if (fin) sc += fin[0];
    int cnt = 0;
    if (sc > kNegInfD) {
      s_rscore[0] = sc;
      s_rlen[0] = 0;
      s_rord[0] = 0;
      for (int m = 0; m < M; ++m) s_rlp[0][m] = s_flp[0][m];
      cnt = 1;
    }
    s_cnt = cnt;
    s_u[2] = (cnt == NP) ? sc : kNegInfD;
    s_lm[0][0] = 0.0;
    s_last[0][0] = -1;
  }
  __syncthreads();
  const double umax_ext = s_u[0], umax_fin = s_u[1];

  int live = 1, cur = 0, n_run = 0;
  int ord = 1;   // arrival numbers (thread 0 alone uses it)
  for (int n = 1; n <= max_len; ++n) {
    n_run = n;
    const int nxt = cur ^ 1;
    const int NC = live * G, NCp = (NC + 63) & ~63;
    // ---- pass A: every candidate's chain in every stream
    for (int i = tid; i < M * NCp; i += JNT) {
      const int m = i / NCp, cand = i - m * NCp;   // (m is wave-uniform: NCp is whole waves)
      if (cand >= NC) continue;
      const int r = cand / G, g = cand - r * G;
      const int lastg = s_last[cur][r];
      Chain ch;
      ch.psi = ch.lp = kNegInfD;
      const JtStream st = s_st[m];
      if (s_ext[(lastg + 1) * G + g] != kNegInfD && (st.lex || g != st.blank)) {
        const size_t TS = mgr_joint_row(st.T - st.skip);
        const double* Eb = st.E + (size_t)b * st.C * TS;
        const unsigned char* wd = st.lex ? &s_words[m][s_off[m][g]] : nullptr;
        const int nw = st.lex ? (int)s_off[m][g + 1] - (int)s_off[m][g] : 1;
        const int plast = lastg < 0 ? -1 : (st.lex ? (int)s_words[m][s_off[m][lastg + 1] - 1] : lastg);
        const double* pgn = n == 1 ? nullptr : st.A + (((size_t)b * 2 + cur) * beam + r) * 2 * TS;
        ch = jt_run<false>(st.nwmax, Eb, TS, s_tp[m], st.blank, wd, g, nw, plast, pgn, pgn ? pgn + TS : nullptr, nullptr, nullptr);
      }
      PSIb[(size_t)m * NCmax + cand] = ch.psi;
      LPb[(size_t)m * NCmax + cand] = ch.lp;
    }
    __syncthreads();
    // ---- every candidate's pre
    for (int cand = tid; cand < NC; cand += JNT) {
      const int r = cand / G, g = cand - r * G;
      const double e = s_ext[(s_last[cur][r] + 1) * G + g];
      double pre = kNegInfD;
      if (e != kNegInfD) {
        pre = 0.0;
        for (int m = 0; m < M; ++m) pre += s_st[m].w * PSIb[(size_t)m * NCmax + cand];
        pre += s_lm[cur][r] + e;
      }
      s_cpre[cand] = pre;
    }
    __syncthreads();
    // ---- the beam best, by wave 0: ties to the smaller candidate index
    if (wave == 0) {
      int nsel = 0;
      for (int w = 0; w < beam; ++w) {
        double best = kNegInfD;
        int bidx = 0x7fffffff;
        for (int idx = lane; idx < NC; idx += 64) {   // (ascending: the first of equal values stays)
          const double v = s_cpre[idx];
          if (v > best) {
            best = v;
            bidx = idx;
          }
        }
        for (int o = 32; o > 0; o >>= 1) {
          const ScoreIdx q = wave_argmax_step_d(best, bidx, o);
          best = q.v;
          bidx = q.i;
        }
        if (best == kNegInfD) break;   // wave-uniform
        if (lane == (bidx & 63)) s_cpre[bidx] = kNegInfD;   // the owning lane retires the candidate
        if (lane == 0) {
          s_sel[nsel] = bidx;
          s_selpre[nsel] = best;
        }
        ++nsel;
      }
      if (lane == 0) s_nsel = nsel;
    }
    __syncthreads();
    const int nsel = s_nsel;
    // ---- the new live set and the kept candidates' complete scores
    if (tid < nsel) {
      const int cand = s_sel[tid];
      const int r = cand / G, g = cand - r * G;
      const double lm = s_lm[cur][r] + s_ext[(s_last[cur][r] + 1) * G + g];
      double fl = 0.0;
      for (int m = 0; m < M; ++m) {
        const double lp = LPb[(size_t)m * NCmax + cand];
        s_flp[tid][m] = lp;
        fl += s_st[m].w * lp;
      }
      fl += lm;
      if (fin) fl += fin[g + 1];
      s_fl[tid] = fl;
      s_lm[nxt][tid] = lm;
      s_last[nxt][tid] = g;
      s_lpre[tid] = s_selpre[tid];
    }
    for (int i = tid; i < nsel * n; i += JNT) {
      const int k = i / n, j = i - k * n;
      const int cand = s_sel[k];
      const int r = cand / G;
      s_seq[nxt][k][j] = j < n - 1 ? s_seq[cur][r][j] : (unsigned char)(cand - r * G);
    }
    if (tid < MAXW) s_src[tid] = -1;
    __syncthreads();
    // ---- the result list: thread 0 decides in rank order, every thread copies behind it
    if (tid == 0) {
      int cnt = s_cnt;
      for (int k = 0; k < nsel; ++k) {
        const double f = s_fl[k];
        if (!(f > kNegInfD)) continue;
        int slot = -1;
        if (cnt < NP) {
          slot = cnt++;
        } else {
          int wi = 0;
          for (int i = 1; i < NP; ++i)
            if (s_rscore[i] < s_rscore[wi] || (s_rscore[i] == s_rscore[wi] && s_rord[i] > s_rord[wi])) wi = i;
          if (f > s_rscore[wi]) slot = wi;
        }
        if (slot >= 0) {
          s_rscore[slot] = f;
          s_rlen[slot] = n;
          s_rord[slot] = ord;
          s_src[slot] = k;
          for (int m = 0; m < M; ++m) s_rlp[slot][m] = s_flp[k][m];
        }
        ++ord;
      }
      s_cnt = cnt;
      double worst = kNegInfD;
      if (cnt == NP) {
        worst = s_rscore[0];
        for (int i = 1; i < NP; ++i) worst = s_rscore[i] < worst ? s_rscore[i] : worst;
      }
      s_u[2] = worst;
    }
    __syncthreads();
    for (int i = tid; i < NP * n; i += JNT) {
      const int slot = i / n, j = i - slot * n;
      const int k = s_src[slot];
      if (k >= 0) s_rseq[slot][j] = s_seq[nxt][k][j];
    }
    // ---- stop? (the same values in every thread)
    const double un = (double)(max_len - n) * umax_ext + umax_fin;
    const bool stop = nsel == 0 || n == max_len || (s_cnt == NP && s_lpre[0] + un < s_u[2]);
    if (stop) break;
    // ---- pass B: the kept chains again, a wave per stream, their arrays into the other half
    if (wave < M && lane < nsel) {
      const int m = wave;
      const int cand = s_sel[lane];
      const int r = cand / G, g = cand - r * G;
      const int lastg = s_last[cur][r];
      const JtStream st = s_st[m];
      const size_t TS = mgr_joint_row(st.T - st.skip);
      const double* Eb = st.E + (size_t)b * st.C * TS;
      const unsigned char* wd = st.lex ? &s_words[m][s_off[m][g]] : nullptr;
      const int nw = st.lex ? (int)s_off[m][g + 1] - (int)s_off[m][g] : 1;
      const int plast = lastg < 0 ? -1 : (st.lex ? (int)s_words[m][s_off[m][lastg + 1] - 1] : lastg);
      const double* pgn = n == 1 ? nullptr : st.A + (((size_t)b * 2 + cur) * beam + r) * 2 * TS;
      double* ogn = st.A + (((size_t)b * 2 + nxt) * beam + lane) * 2 * TS;
      jt_run<true>(st.nwmax, Eb, TS, s_tp[m], st.blank, wd, g, nw, plast, pgn, pgn ? pgn + TS : nullptr, ogn, ogn + TS);
    }
    __syncthreads();
    cur = nxt;
    live = nsel;
  }
  __syncthreads();

  // ---- the list in order: by score, ties to the earlier arrival
  const int cnt = s_cnt;
  if (tid < NP) {
    int rank = tid;
    if (tid < cnt) {
      rank = 0;
      for (int i = 0; i < cnt; ++i)
        rank += (s_rscore[i] > s_rscore[tid] || (s_rscore[i] == s_rscore[tid] && s_rord[i] < s_rord[tid])) ? 1 : 0;
    }
    const size_t slot = (size_t)b * NP + rank;
    const int len = tid < cnt ? s_rlen[tid] : 0;
    int32_t* o = out + slot * max_len;
    for (int j = 0; j < len; ++j) o[j] = s_rseq[tid][j];
    for (int j = len; j < max_len; ++j) o[j] = -1;
    out_len[slot] = tid < cnt ? len : -1;
    score[slot] = tid < cnt ? s_rscore[tid] : kNegInfD;
    for (int m = 0; m < M; ++m) logp[slot * M + m] = tid < cnt ? s_rlp[tid][m] : kNegInfD;
  }
  if (rounds && tid == 0) rounds[b] = n_run;
}

}  // namespace

extern "C" {

size_t mgr_ctc_joint_ws_bytes(int B, int M, const mgr_joint_stream* streams, int G, int beam, int top_paths, int max_len) {
  (void)top_paths;   // (the list lives in LDS)
  (void)max_len;
  int T[MAXM], C[MAXM];
  M = M < 1 ? 1 : (M > MAXM ? MAXM : M);
  for (int m = 0; m < M; ++m) {
    T[m] = (streams && streams[m].T > 0) ? streams[m].T : 1;
    C[m] = (streams && streams[m].C > 0) ? streams[m].C : 1;
  }
  return mgr_joint_ws_layout(nullptr, B > 0 ? B : 1, M, T, C, G > 0 ? G : 1, beam > 0 ? beam : 1).bytes;
}

int mgr_ctc_joint_decode(mgr_ctx* c, int B, int M, const mgr_joint_stream* streams, int G, const double* ext, const double* fin, int beam,
                         int top_paths, int max_len, int32_t* out, int32_t* out_len, double* score, double* logp, int32_t* rounds, void* ws,
                         size_t ws_bytes) {
  MGR_REQUIRE(c && streams && ext && out && out_len && score && logp, "null argument");
  mgr_planes_forget_range(c, ws, ws_bytes);   // (this call writes its workspace: kept weight planes in it are gone)
  MGR_REQUIRE(M >= 1 && M <= MAXM, "M = %d streams out of [1, %d]", M, MAXM);
  MGR_REQUIRE(B > 0 && B <= 65535, "B = %d out of [1, 65535]", B);
  MGR_REQUIRE(G >= 1 && G <= MAXG, "G = %d gestures out of [1, %d]", G, MAXG);
  MGR_REQUIRE(beam >= 1 && beam <= MAXW, "beam width %d out of [1, %d]", beam, MAXW);
  MGR_REQUIRE(top_paths >= 1 && top_paths <= beam, "top_paths %d out of [1, beam = %d]", top_paths, beam);
  MGR_REQUIRE(max_len >= 1 && max_len <= MGR_RESCORE_MAX_LABELS, "max_len %d out of [1, %d]", max_len, MGR_RESCORE_MAX_LABELS);
  JtArgs a;
  memset(&a, 0, sizeof(a));
  int T[MAXM], C[MAXM];
  for (int m = 0; m < M; ++m) {
    const mgr_joint_stream& s = streams[m];
    MGR_REQUIRE(s.struct_size == sizeof(mgr_joint_stream), "stream %d: struct_size %u, this library's is %u", m, s.struct_size,
                (unsigned)sizeof(mgr_joint_stream));
    MGR_REQUIRE(s.P && s.input_len, "stream %d: null argument", m);
    MGR_REQUIRE(s.T > s.skip && s.skip >= 0 && s.C > 1, "stream %d: bad shape T=%d C=%d skip=%d", m, s.T, s.C, s.skip);
    MGR_REQUIRE(s.blank >= 0 && s.blank < s.C, "stream %d: blank %d out of range", m, s.blank);
    MGR_REQUIRE(s.weight > 0.0 && s.weight <= 1.79e308, "stream %d: weight %g is not a positive finite number", m, s.weight);
    MGR_REQUIRE(s.eps >= 0.f && s.eps <= 3.4e38f, "stream %d: eps %g", m, (double)s.eps);
    const bool with_lex = s.phrase_off || s.phrase_words;
    int nwmax = 1;
    if (with_lex) {   // (mgr_ctc_lexicon_decode's rules)
      MGR_REQUIRE(s.phrase_off && s.phrase_words, "stream %d: null argument", m);
      MGR_REQUIRE(s.C <= 64, "stream %d: C = %d too large (max 64)", m, s.C);
      if (const int rc = lex_arg_pack(&a.lex[m], s.phrase_off, s.phrase_words, G, s.C, s.blank)) return rc;
      for (int g = 0; g < G; ++g) {
        const int nw = s.phrase_off[g + 1] - s.phrase_off[g];
        MGR_REQUIRE(nw <= MGR_JOINT_MAX_PHRASE_WORDS, "stream %d: phrase %d has %d words (max %d)", m, g, nw, MGR_JOINT_MAX_PHRASE_WORDS);
        nwmax = nw > nwmax ? nw : nwmax;
      }
    } else {
      MGR_REQUIRE(G <= s.C, "stream %d: G = %d gestures for C = %d classes without a lexicon", m, G, s.C);
    }
    T[m] = s.T;
    C[m] = s.C;
    a.s[m].input_len = s.input_len;
    a.s[m].w = s.weight;
    a.s[m].T = s.T;
    a.s[m].C = s.C;
    a.s[m].skip = s.skip;
    a.s[m].blank = s.blank;
    a.s[m].lex = with_lex ? 1 : 0;
    a.s[m].nwmax = nwmax;
  }
  MGR_REQUIRE(ws && ws_bytes >= mgr_ctc_joint_ws_bytes(B, M, streams, G, beam, top_paths, max_len), "workspace too small");
  const mgr_joint_ws W = mgr_joint_ws_layout(ws, B, M, T, C, G, beam);
  const size_t lds = ((size_t)(G + 1) * G + (size_t)beam * G) * sizeof(double);
  if (!(c->attr_done & MGR_ATTR_JOINT)) {
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_joint), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(((size_t)(MAXG + 1) * MAXG + (size_t)MAXW * MAXG) * sizeof(double))));
    c->attr_done |= MGR_ATTR_JOINT;
  }
  hipStream_t s = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_MISC);
  for (int m = 0; m < M; ++m) {
    a.s[m].E = W.E[m];
    a.s[m].A = W.A[m];
    const size_t TS = mgr_joint_row(T[m] - streams[m].skip);
    hipLaunchKernelGGL(k_joint_emissions, dim3((unsigned)((TS + 255) / 256), B), dim3(256), 0, s, streams[m].P, streams[m].input_len, T[m], C[m],
                       streams[m].skip, streams[m].eps, TS, W.E[m]);
  }
  hipLaunchKernelGGL(k_joint, dim3(B), dim3(JNT), lds, s, a, M, G, ext, fin, beam, top_paths, max_len, W.PSI, W.LP, out, out_len, score, logp,
                     rounds);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}

}  // extern "C"
