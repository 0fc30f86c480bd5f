// K13: lexicon-constrained CTC decode (not present in the reference): the best PHRASE sequence whose word expansion the
// posteriors support - a Viterbi token pass over the phrase lexicon composed with the CTC topology, with a phrase bigram.  The audio
// network's classes are words; its gestures are phrases of one to five words (audio_network/data_generator.py: class_2_words).
//
// State graph (include/mgr.h states the semantics): with the lexicon's words numbered j = 0 .. n_words - 1 in phrase order,
//   state 0 = INIT (blank before any phrase), state 2j + 1 = the word j, state 2j + 2 = the blank behind word j: B(g, k) inside a
//   phrase, Z(g) behind its last word - the extended label sequence of ctc.hip / align.hip over the concatenated lexicon, in which
//   the step onto a phrase's FIRST word does not come from the neighbouring states but from INIT, every Z(g') and every last word.
// Two kernels: emissions (k_lattice_emissions of ctc_lattice.h in natural-log units: class-major rows), then ONE WORKGROUP per sample
// with a state per thread (64 .. 512 threads).  A frame is one barrier: every thread reads its two neighbours' values of the previous
// frame from LDS (two buffers, swapped per frame), a phrase-entry thread also the G pairs (Z(g'), last word of g') - kept beside the
// state values as one 8-byte entry per phrase, a broadcast read - and its column of ext (f32, LDS, consecutive lanes consecutive
// words; kept twice, the second copy with -inf where the last word of g' equals the first word of g): G^2 candidates per frame spread
// over the G entry threads.  Emissions are fetched four frames at a time with 16-byte loads, a chunk ahead.
// Back-pointers: 2 bits per frame for every state but the phrase entries (stay, from s - 1, from s - 2), sixteen frames to a word:
// ceil(To / 16) * N words; a byte per frame for a phrase entry (0 stay, 1 INIT, 2 + 2g' from Z(g'), 3 + 2g' from the last word of g'),
// four frames to a word: ceil(To / 4) * G words - 46 KB + 40 KB at the reference's lexicon (97 states, 21 phrases) and 1898 frames.
// They live in LDS when everything fits 160 KB and in the workspace otherwise (align.hip's rule).  The backtrace is a chain of
// dependent reads run by wave 0 with wave-uniform values (scalar instructions); a state that stays takes the rest of its 16-frame
// word in one step.  Behind it, parallel passes over the frames turn the state path into classes, phrase starts (a block-wide prefix
// sum), segments and confidences.
// Numerics: natural-log units.  The search runs on f32 values kept O(10) by subtracting the workgroup maximum every 16 frames; the
// search decides, it does not report: logp is summed again in fp64 over the emissions of the path found and the table terms over its
// phrases from the fp64 tables, so what was subtracted needs no fp64 sum of its own (as align.hip keeps one) and logp of a
// 1900-frame path does not sit where an f32 ulp is 5e-4.
// Ties: the smaller back-pointer code wins (stay, then one state, then two; for a phrase entry stay, INIT, then the phrases in
// order, Z(g') before the last word of g'); among the final states the smallest state index.
#include "ctc_lattice.h"
#include "wave_f64.h"

namespace {

constexpr int MAXG = MGR_LEXICON_MAX_PHRASES;
constexpr size_t kLdsMax = 160 * 1024;

// row length of the class-major emissions: To + the over-read of the chunk fetched ahead, a multiple of 4 floats
__host__ __device__ inline size_t lex_ts(int To) { return ((size_t)To + 8 + 3) / 4 * 4; }
__host__ __device__ inline int lex_nb16(int To) { return (To + 15) / 16; }
__host__ __device__ inline int lex_nb4(int To) { return (To + 3) / 4; }
__host__ __device__ inline int lex_gp(int G) { return (G + 3) & ~3; }   // phrases rounded up to the entry loop's four per turn

// LDS of the decode kernel, in 32-bit words
struct LexLds { size_t red, x, vb, ext, scan, wred, off, cls, ent, state, starts, bp2, bpe, words; };
__host__ __device__ inline LexLds lex_lds(int NT, int G, int N, int To, bool with_bp) {
  LexLds L;
  size_t o = 0;
  L.red = o;    o += 2 * (size_t)NT;                 // double per thread (first: 8-byte aligned)
  L.x = o;      o += 2 * 2 * (size_t)MAXG;           // float2 per phrase, two buffers
  L.vb = o;     o += 2 * (size_t)NT;                 // float per state, two buffers
  L.ext = o;    o += 2 * (size_t)(lex_gp(G) + 1) * G;   // float: ext, and ext where the last word of g' differs from the first of g
  L.scan = o;   o += (size_t)NT;                     // int per thread
  L.wred = o;   o += 16;                             // per-wave value and index
  L.off = o;    o += MAXG + 2;                       // int per phrase + 1
  L.cls = o;    o += (size_t)(NT + 1) / 2;           // int16 per state: the class it emits
  L.ent = o;    o += (size_t)(NT + 1) / 2;           // int16 per state: the phrase it enters, or -1
  L.state = o;  o += (size_t)(To + 64 + 1) / 2;      // uint16 per frame: the path's state
  L.starts = o; o += (size_t)(To + 1) / 2;           // uint16 per phrase of the path: its first frame
  L.bp2 = o;    o += with_bp ? (size_t)lex_nb16(To) * N : 0;
  L.bpe = o;    o += with_bp ? (size_t)lex_nb4(To) * G : 0;
  L.words = o;
  return L;
}

// sum of one double per thread over the workgroup, in a fixed order (wave butterflies, then the waves in order); every thread gets it
__device__ __forceinline__ double block_sum_d(double v, double* red, int tid, int nwaves) {
  for (int o = 32; o > 0; o >>= 1) v += shfl_xor_d(v, o);
  __syncthreads();   // (red may still be read from an earlier sum)
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < nwaves; ++w) s += red[w];
  return s;
}

// One workgroup per sample, thread s = state s (blockDim.x = the states rounded up to whole waves).
template <bool LDS_BP>
__global__ __launch_bounds__(512) void k_lexicon_decode(const float* __restrict__ P, const int32_t* __restrict__ input_len, int T, int C, int skip,
                                                        int blank, const LexArg lex, int G, int nw, const double* __restrict__ ext,
                                                        const double* __restrict__ fin, int cap, const float* __restrict__ E,
                                                        uint32_t* __restrict__ BP2g, uint32_t* __restrict__ BPEg, int32_t* __restrict__ n_phr,
                                                        int32_t* __restrict__ phr, int32_t* __restrict__ seg, float* __restrict__ conf,
                                                        int32_t* __restrict__ path, double* __restrict__ score, double* __restrict__ logp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6, NW = NT >> 6;
  const int To = T - skip, N = 1 + 2 * nw, NB16 = lex_nb16(To), NB4 = lex_nb4(To);
  const size_t TS = lex_ts(To);
  const int Tp = clip_len(input_len[b], To);
  const LexLds L = lex_lds(NT, G, N, To, LDS_BP);
  double* s_red = reinterpret_cast<double*>(smem + L.red);
  float* s_x = reinterpret_cast<float*>(smem + L.x);       // [2][MAXG][2]: (Z(g), last word of g)
  float* s_vb = reinterpret_cast<float*>(smem + L.vb);     // [2][NT]
  const int Gp = lex_gp(G);
  float* s_ext = reinterpret_cast<float*>(smem + L.ext);   // [(Gp + 1) * G]: ext, rows behind G + 1 are -inf
  float* s_extw = s_ext + (size_t)(Gp + 1) * G;            // the same with -inf where phrase g may not follow g' without a blank
  int* s_scan = reinterpret_cast<int*>(smem + L.scan);
  float* s_wval = reinterpret_cast<float*>(smem + L.wred);
  int* s_widx = reinterpret_cast<int*>(smem + L.wred + 8);
  int* s_off = reinterpret_cast<int*>(smem + L.off);
  int16_t* s_cls = reinterpret_cast<int16_t*>(smem + L.cls);
  int16_t* s_ent = reinterpret_cast<int16_t*>(smem + L.ent);
  uint16_t* s_state = reinterpret_cast<uint16_t*>(smem + L.state);
  uint16_t* s_starts = reinterpret_cast<uint16_t*>(smem + L.starts);
  uint32_t* bp2 = LDS_BP ? smem + L.bp2 : BP2g + (size_t)b * NB16 * N;
  uint32_t* bpe = LDS_BP ? smem + L.bpe : BPEg + (size_t)b * NB4 * G;
  const float* Eb = E + (size_t)b * C * TS;

  for (int i = tid; i <= G; i += NT) s_off[i] = lex.off[i];
  for (int i = tid; i < 2 * 2 * MAXG; i += NT) s_x[i] = kNegInf;   // (the entries behind G stay -inf: the entry loop reads them)
  __syncthreads();
  for (int i = tid; i < (Gp + 1) * G; i += NT) {
    const int row = i / G, col = i - row * G;
    const float e = row <= G ? (float)ext[i] : kNegInf;
    s_ext[i] = e;
    // the last word of phrase row - 1 against the first word of phrase col
    s_extw[i] = (row >= 1 && row <= G && lex.words[s_off[row] - 1] != lex.words[s_off[col]]) ? e : kNegInf;
  }
  __syncthreads();

  // ---- what this thread's state is
  const int s = tid;
  const bool valid = s < N;
  int j = 0, g = 0, k = 0, cls = blank;
  bool isword = false, islast = false;
  if (valid && s > 0) {
    j = (s - 1) >> 1;
    while (g < G - 1 && s_off[g + 1] <= j) ++g;
    k = j - s_off[g];
    isword = (s & 1) != 0;
    islast = j == s_off[g + 1] - 1;
    if (isword) cls = lex.words[j];
  }
  const bool entry = isword && k == 0;
  const bool has1 = valid && s >= 1 && !entry;                                  // a word behind its blank, a blank behind its word
  const bool has2 = isword && k > 0 && (int)lex.words[j - 1] != cls;           // the step over the blank: different words only
  const bool isZ = valid && s > 0 && !isword && islast, isWl = isword && islast;
  const int finidx = !valid ? -1 : (s == 0 ? 0 : ((isZ || isWl) ? g + 1 : -1));
  s_cls[s] = (int16_t)cls;
  s_ent[s] = (int16_t)(entry ? g : -1);
  const float e0 = entry ? s_ext[g] : kNegInf;
  const float* Er = Eb + (size_t)cls * TS;

  // ---- the token pass
  float v = kNegInf;
  if (Tp == 0) {
    if (s == 0) v = 0.f;
  } else {
    if (s == 0) v = Er[0];
    if (entry) v = e0 + Er[0];
    int cur = 0;
    s_vb[s] = v;
    if (isZ) s_x[2 * g] = v;
    if (isWl) s_x[2 * g + 1] = v;
    __syncthreads();
    float4 ec = *reinterpret_cast<const float4*>(Er), en;
    uint32_t bits = 0u;
    int since = 0;
    for (int t0 = 0; t0 < Tp; t0 += 4) {
      en = *reinterpret_cast<const float4*>(Er + t0 + 4);   // (t0 a multiple of 4: 16-byte aligned; the over-read stays in the row)
      const float em[4] = {ec.x, ec.y, ec.z, ec.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int t = t0 + q;
        if (t >= 1 && t < Tp) {   // (uniform over the workgroup)
          const float* vb = s_vb + cur * NT;
          float m = v;
          uint32_t code = 0u;
          if (!entry) {
            const float p1 = has1 ? vb[s - 1] : kNegInf;
            const float p2 = has2 ? vb[s - 2] : kNegInf;
            if (p1 > m) { m = p1; code = 1u; }
            if (p2 > m) { m = p2; code = 2u; }
            bits |= code << (2 * (t & 15));
          } else {
            const float2* xs = reinterpret_cast<const float2*>(s_x + cur * 2 * MAXG);
            float c = vb[0] + e0;
            if (c > m) { m = c; code = 1u; }
            // The G^2 candidates of a frame, G per entry lane: a lone wave pays several cycles of issue per instruction, so what
            // counts is the instruction count per phrase (about a tenth of the call at G = 21).  Per phrase g': one maximum of (Z(g'), last word of
            // g') - the second through the table that already holds -inf where the two words are equal - and one comparison; which
            // of the two it was is looked up once, for the winner.  Four phrases per turn, their twelve LDS reads in flight together.
            int bq = -1;
            for (int q0 = 0; q0 < Gp; q0 += 4) {
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                const int q2 = q0 + u;
                const float2 x = xs[q2];
                c = fmaxf(x.x + s_ext[(q2 + 1) * G + g], x.y + s_extw[(q2 + 1) * G + g]);
                if (c > m) { m = c; bq = q2; }
              }
            }
            if (bq >= 0) code = (xs[bq].x + s_ext[(bq + 1) * G + g] == m) ? 2u + 2u * bq : 3u + 2u * bq;   // (Z(g') wins their tie)
            bits |= code << (8 * (t & 3));
          }
          v = valid ? m + em[q] : kNegInf;
          cur ^= 1;
          s_vb[cur * NT + s] = v;
          if (isZ) s_x[cur * 2 * MAXG + 2 * g] = v;
          if (isWl) s_x[cur * 2 * MAXG + 2 * g + 1] = v;
          __syncthreads();
        }
      }
      // back-pointer words: a phrase entry completes one per chunk, the other states one per sixteen frames (or at the last ones)
      if (entry) {
        bpe[(size_t)(t0 >> 2) * G + g] = bits;
        bits = 0u;
      } else if (((t0 + 4) & 15) == 0 || t0 + 4 >= Tp) {
        if (valid) bp2[(size_t)(t0 >> 4) * N + s] = bits;
        bits = 0u;
      }
      ec = en;
      since += 4;
      if (since >= 16 && t0 + 4 < Tp) {   // renormalise: keep the running values O(10)
        since = 0;
        float m = v;
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) s_wval[wave] = m;
        __syncthreads();
        m = s_wval[0];
        for (int w = 1; w < NW; ++w) m = fmaxf(m, s_wval[w]);
        if (m != kNegInf) {
          v -= m;
          s_vb[cur * NT + s] = v;
          if (isZ) s_x[cur * 2 * MAXG + 2 * g] = v;
          if (isWl) s_x[cur * 2 * MAXG + 2 * g + 1] = v;
        }
        __syncthreads();
      }
    }
  }

  // ---- the best final state: INIT + fin[0], or a phrase's last word / its Z + fin[g + 1]; a tie takes the smallest state
  float f = kNegInf;
  if (finidx >= 0) f = v + (fin ? (float)fin[finidx] : 0.f);
  int fs = s;
  for (int o = 32; o > 0; o >>= 1) {
    const float of = __shfl_xor(f, o);
    const int os = __shfl_xor(fs, o);
    if (of > f || (of == f && os < fs)) { f = of; fs = os; }
  }
  __syncthreads();
  if (lane == 0) { s_wval[wave] = f; s_widx[wave] = fs; }
  __syncthreads();   // (also: the back-pointer words of every thread are in place)
  f = s_wval[0];
  fs = s_widx[0];
  for (int w = 1; w < NW; ++w)
    if (s_wval[w] > f) { f = s_wval[w]; fs = s_widx[w]; }   // (waves in order: the smaller state wins a tie)
  const bool feasible = f != kNegInf;

  if (!feasible) {
    if (tid == 0) {
      n_phr[b] = -1;
      score[b] = -(double)__builtin_huge_valf();
      logp[b] = -(double)__builtin_huge_valf();
    }
    for (int i = tid; i < cap; i += NT) {
      phr[(size_t)b * cap + i] = -1;
      seg[((size_t)b * cap + i) * 2] = -1;
      seg[((size_t)b * cap + i) * 2 + 1] = -1;
      conf[(size_t)b * cap + i] = 0.f;
    }
    if (path)
      for (int t = tid; t < To; t += NT) path[(size_t)b * To + t] = -1;
    return;
  }

  // ---- backtrace: wave 0, wave-uniform values (see the head of the file)
  if (tid < 64) {
    int st = __builtin_amdgcn_readfirstlane(fs);
    int t = Tp - 1;
    while (t >= 0) {
      const int eg = __builtin_amdgcn_readfirstlane((int)s_ent[st]);
      if (eg < 0) {
        const int kk = t & 15;
        const uint32_t w = __builtin_amdgcn_readfirstlane(bp2[(size_t)(t >> 4) * N + st]);
        // this state's pointers at frames t - kk .. t of the word (frame 0's are zero: nothing points out of it)
        if ((w & (0xFFFFFFFFu >> (30 - 2 * kk))) == 0u) {
          if (lane <= kk) s_state[t - kk + lane] = (uint16_t)st;
          t -= kk + 1;
        } else {
          if (lane == 0) s_state[t] = (uint16_t)st;
          st -= (int)((w >> (2 * kk)) & 3u);
          if (st < 0) st = 0;   // (cannot happen with pointers this kernel wrote; keeps the LDS reads in range whatever they hold)
          t -= 1;
        }
      } else {
        const uint32_t w = __builtin_amdgcn_readfirstlane(bpe[(size_t)(t >> 2) * G + eg]);
        const int code = (int)((w >> (8 * (t & 3))) & 255u);
        if (lane == 0) s_state[t] = (uint16_t)st;
        if (code == 1) {
          st = 0;
        } else if (code >= 2) {
          int q = (code - 2) >> 1;
          if (q >= G) q = G - 1;   // (likewise)
          const int z = 2 * __builtin_amdgcn_readfirstlane(s_off[q + 1]);
          st = (code & 1) ? z - 1 : z;
        }
        t -= 1;
      }
    }
  }
  __syncthreads();

  // ---- states -> classes, logp, phrase starts (a phrase starts where its entry state is entered)
  const int chunk = (Tp + NT - 1) / NT;
  const int ta = min(tid * chunk, Tp), tb = min(ta + chunk, Tp);
  double lp = 0.0;
  int cnt = 0;
  for (int t = ta; t < tb; ++t) {
    const int st = s_state[t], c = s_cls[st];
    if (path) path[(size_t)b * To + t] = c;
    lp += (double)Eb[(size_t)c * TS + t];
    cnt += (s_ent[st] >= 0 && (t == 0 || s_state[t - 1] != st)) ? 1 : 0;
  }
  if (path)
    for (int t = Tp + tid; t < To; t += NT) path[(size_t)b * To + t] = -1;
  s_scan[tid] = cnt;
  __syncthreads();
  for (int o = 1; o < NT; o <<= 1) {
    const int x = tid >= o ? s_scan[tid - o] : 0;
    __syncthreads();
    s_scan[tid] += x;
    __syncthreads();
  }
  const int n = s_scan[NT - 1];
  {
    int o = s_scan[tid] - cnt;
    for (int t = ta; t < tb; ++t) {
      const int st = s_state[t];
      if (s_ent[st] >= 0 && (t == 0 || s_state[t - 1] != st)) s_starts[o++] = (uint16_t)t;
    }
  }
  __syncthreads();

  // ---- per phrase: its table term (fp64, from the tables themselves), and for the first cap of them the outputs
  double tbl = 0.0;
  for (int i = tid; i < n; i += NT) {
    const int ti = s_starts[i];
    const int gi = s_ent[s_state[ti]];
    const int gp = i > 0 ? (int)s_ent[s_state[s_starts[i - 1]]] : -1;
    tbl += ext[(size_t)(gp + 1) * G + gi];
    if (i == n - 1 && fin) tbl += fin[gi + 1];
    if (i < cap) {
      int end = (i + 1 < n ? (int)s_starts[i + 1] : Tp) - 1;
      while (end > ti && !(s_state[end] & 1)) --end;   // the last frame of the phrase's last word
      double sum = 0.0;
      int nf = 0;
      for (int t = ti; t <= end; ++t) {
        const int st = s_state[t];
        if (st & 1) {
          sum += (double)P[((size_t)b * T + skip + t) * C + s_cls[st]];
          ++nf;
        }
      }
      phr[(size_t)b * cap + i] = gi;
      seg[((size_t)b * cap + i) * 2] = ti + skip;
      seg[((size_t)b * cap + i) * 2 + 1] = end + skip;
      conf[(size_t)b * cap + i] = (float)(sum / (double)nf);
    }
  }
  if (n == 0 && tid == 0 && fin) tbl += fin[0];
  for (int i = min(n, cap) + tid; i < cap; i += NT) {
    phr[(size_t)b * cap + i] = -1;
    seg[((size_t)b * cap + i) * 2] = -1;
    seg[((size_t)b * cap + i) * 2 + 1] = -1;
    conf[(size_t)b * cap + i] = 0.f;
  }
  lp = block_sum_d(lp, s_red, tid, NW);
  tbl = block_sum_d(tbl, s_red, tid, NW);
  if (tid == 0) {
    n_phr[b] = n;   // the TRUE count, whatever the capacity
    logp[b] = lp;
    score[b] = lp + tbl;
  }
}

}  // namespace

extern "C" {

// emissions | 2-bit back-pointer words | phrase-entry back-pointer words; laid out for T frames (the kernels use rows of T - skip:
// both fit) to keep the query simple
struct LexWs { float* E; uint32_t *bp2, *bpe; size_t bytes; };
static LexWs lex_ws_layout(void* ws, int B, int T, int C, int G, int nw) {
  mgr_ws_carver w(ws);
  return {w.take<float>((size_t)B * C * lex_ts(T)), w.take<uint32_t>((size_t)B * lex_nb16(T) * (1 + 2 * (size_t)nw)),
          w.take<uint32_t>((size_t)B * lex_nb4(T) * G), w.off};
}
// (the words are counted from the lexicon itself, host memory: a count passed beside it could disagree with it)
size_t mgr_ctc_lexicon_ws_bytes(int B, int T, int C, int G, const int32_t* phrase_off) {
  const int nw = (phrase_off && G > 0 && phrase_off[G] > 0) ? phrase_off[G] : 1;
  return lex_ws_layout(nullptr, B > 0 ? B : 1, T > 0 ? T : 1, C > 0 ? C : 1, G > 0 ? G : 1, nw).bytes;
}

int mgr_ctc_lexicon_decode(mgr_ctx* c, const float* P, const int32_t* input_len, int B, int T, int C, int skip, int blank, float eps,
                           const int32_t* phrase_off, const int32_t* phrase_words, int G, const double* ext, const double* fin, int cap,
                           int32_t* n_phr, int32_t* phr, int32_t* seg, float* conf, int32_t* path, double* score, double* logp, void* ws,
                           size_t ws_bytes) {
  MGR_REQUIRE(c && P && input_len && phrase_off && phrase_words && ext && n_phr && phr && seg && conf && score && logp, "null argument");
  mgr_planes_forget_range(c, ws, ws_bytes);   // (this call writes its workspace: kept weight planes in it are gone)
  MGR_REQUIRE(B > 0 && T > skip && skip >= 0 && C > 1 && cap > 0, "bad shape B=%d T=%d C=%d skip=%d cap=%d", B, T, C, skip, cap);
  MGR_REQUIRE(C <= 64, "C = %d too large (max 64)", C);
  MGR_REQUIRE(blank >= 0 && blank < C, "blank %d out of range", blank);
  MGR_REQUIRE(G >= 1 && G <= MGR_LEXICON_MAX_PHRASES, "G = %d phrases out of [1, %d]", G, MGR_LEXICON_MAX_PHRASES);
  MGR_REQUIRE(T - skip <= MGR_SEGMENTS_MAX_FRAMES, "T - skip = %d too large (max %d)", T - skip, MGR_SEGMENTS_MAX_FRAMES);
  LexArg lex;
  memset(&lex, 0, sizeof(lex));
  if (const int rc = lex_arg_pack(&lex, phrase_off, phrase_words, G, C, blank)) return rc;
  const int nw = phrase_off[G];
  MGR_REQUIRE(ws && ws_bytes >= mgr_ctc_lexicon_ws_bytes(B, T, C, G, phrase_off), "workspace too small");
  const int To = T - skip, N = 1 + 2 * nw, NT = (N + 63) / 64 * 64;
  const LexWs W = lex_ws_layout(ws, B, T, C, G, nw);
  const size_t lds_small = lex_lds(NT, G, N, To, false).words * sizeof(uint32_t);
  const size_t lds_full = lex_lds(NT, G, N, To, true).words * sizeof(uint32_t);
  const bool in_lds = lds_full <= kLdsMax;
  MGR_REQUIRE(lds_small <= kLdsMax, "T - skip = %d too large for the LDS frame states", To);
  if (!(c->attr_done & MGR_ATTR_LEXICON)) {
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_lexicon_decode<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_lexicon_decode<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    c->attr_done |= MGR_ATTR_LEXICON;
  }
  hipStream_t s = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_MISC);
  hipLaunchKernelGGL(k_lattice_emissions<false>, dim3((unsigned)((lex_ts(To) + 255) / 256), B), dim3(256), 0, s, P, input_len, T, C, skip, eps, lex_ts(To),
                     W.E);
  if (in_lds)
    hipLaunchKernelGGL(k_lexicon_decode<true>, dim3(B), dim3(NT), lds_full, s, P, input_len, T, C, skip, blank, lex, G, nw, ext, fin, cap, W.E,
                       W.bp2, W.bpe, n_phr, phr, seg, conf, path, score, logp);
  else
    hipLaunchKernelGGL(k_lexicon_decode<false>, dim3(B), dim3(NT), lds_small, s, P, input_len, T, C, skip, blank, lex, G, nw, ext, fin, cap, W.E,
                       W.bp2, W.bpe, n_phr, phr, seg, conf, path, score, logp);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}

}  // extern "C"
