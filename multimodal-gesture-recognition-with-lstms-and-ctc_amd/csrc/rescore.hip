// K14: CTC hypothesis scoring (not present in the reference): logp[b, k] = ln sum over all CTC alignments of hypothesis k
// of sample b - what rescoring an N-best list needs from every modality: the loss's alpha recursion for K label sequences per sample
// in one launch, without beta, without a stored lattice, with the posteriors read once.
//
// Two kernels.  k_rescore_emissions: class-major log2 y rows per sample (ctc.hip's emissions restated with rows that start at t = 0,
// as lexicon.hip restated the aligner's), written once and read by the sample's K hypotheses out of L2.  k_rescore: ONE WAVE per
// hypothesis, four hypotheses of a sample per workgroup - the hardware deals a workgroup's waves round over the CU's four SIMDs, so the
// four chains do not share one (ctc.hip, round 6: chains on one SIMD slow each other down).
// Prologue: the wave expands its hypothesis into LDS - without a lexicon the labels themselves (clipped into the class range as the loss
// clips them), with one the words of its phrases: sixty-four entries at a time, a prefix sum of the phrase lengths across the wave.
// Recursion: ctc.hip's alpha.  The extended sequence lies across the lanes as (blank, label) pairs, PPL pairs per lane; the wave picks
// PPL from its OWN expanded length (a wave-uniform branch: gesture hypotheses always run PPL = 1); the neighbour's label state arrives
// through DPP wave_shr:1; base-2 units on the raw exp / log instructions; the wave maximum is subtracted every 16 frames and summed
// into an fp64 offset; emissions are fetched a chunk (8 frames, 4 from PPL = 3 on) ahead with 16-byte loads.  The recursion starts
// from a virtual frame -1 (state 0 holds log 1), so the chunks start at t = 0 and an empty input needs no case of its own.  Nothing is
// stored per frame: the two final states and the offset are the result.
#include "common.h"

namespace {

constexpr float kNegInf = -__builtin_huge_valf();
constexpr float kLseFloor = -3.0e38f;   // (ctc.hip: all-(-inf) inputs of a log-sum-exp)
constexpr double kLn2 = 0.693147180559945309417232121458;
constexpr int MAXG = MGR_LEXICON_MAX_PHRASES;
constexpr int MAXL = MGR_RESCORE_MAX_LABELS;   // 255 labels: 256 pairs, four per lane
constexpr int WPB = 4;                         // waves (hypotheses) per workgroup

// the lexicon travels as a kernel argument: word ids are below 64, offsets at most 255
struct LexArg {
  uint8_t off[MAXG + 1];
  uint8_t words[MGR_LEXICON_MAX_WORDS + 1];
};

__device__ __forceinline__ float exp2_raw(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float log2_raw(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(fmaxf(a, b), kLseFloor);
  return m + log2_raw(exp2_raw(a - m) + exp2_raw(b - m));
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(fmaxf(a, b), c), kLseFloor);
  return m + log2_raw(exp2_raw(a - m) + exp2_raw(b - m) + exp2_raw(c - m));
}

// (ctc.hip) wave_shr:1 moves a value to the next lane of the whole wave, lanes without a source receive `fill`; row_shr:n within rows
constexpr int DPP_WAVE_SHR1 = 0x138;
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v, float fill) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_max_f32(float m) {
  m = fmaxf(m, dpp_f32<0x111>(m, m));
  m = fmaxf(m, dpp_f32<0x112>(m, m));
  m = fmaxf(m, dpp_f32<0x114>(m, m));
  m = fmaxf(m, dpp_f32<0x118>(m, m));   // lane 15 of a row holds the row's maximum
  const int i = __float_as_int(m);
  return fmaxf(fmaxf(__int_as_float(__builtin_amdgcn_readlane(i, 15)), __int_as_float(__builtin_amdgcn_readlane(i, 31))),
               fmaxf(__int_as_float(__builtin_amdgcn_readlane(i, 47)), __int_as_float(__builtin_amdgcn_readlane(i, 63))));
}

// row length of the class-major emissions: To + the over-read of the chunk fetched ahead (at most 15 floats behind the last frame),
// a multiple of 4 floats
__host__ __device__ inline size_t rs_ts(int To) { return ((size_t)To + 16 + 3) / 4 * 4; }
__device__ __forceinline__ int clip_len(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// emissions log2 y(t, c) = log2(P + eps) - log2(sum_c (P + eps)), class-major: E[b][c][TS].  One frame per thread; the frames of a
// row behind the sample's length (the prefetch reads them and uses none) are zeros.
__global__ __launch_bounds__(256) void k_rescore_emissions(const float* __restrict__ P, const int32_t* __restrict__ input_len, int T, int C,
                                                           int skip, float eps, float* __restrict__ E) {
  const int b = blockIdx.y, To = T - skip;
  const size_t TS = rs_ts(To);
  const int Tp = clip_len(input_len[b], To);
  const int t = blockIdx.x * 256 + threadIdx.x;
  if ((size_t)t >= TS) return;
  float* Eb = E + (size_t)b * C * TS;
  if (t >= Tp) {
    for (int c = 0; c < C; ++c) Eb[(size_t)c * TS + t] = 0.f;
    return;
  }
  const float* row = P + ((size_t)b * T + skip + t) * C;
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += row[c] + eps;
  const float ls = log2f(s);
  for (int c = 0; c < C; ++c) Eb[(size_t)c * TS + t] = log2f(row[c] + eps) - ls;
}

template <int PPL>
struct Chunk {
  static constexpr int CH = PPL <= 2 ? 8 : 4;   // frames per prefetched chunk (a multiple of 4: float4 loads along time)
  float eb[CH];
  float el[CH][PPL];
};

// alpha over the Tp frames of one sample for the L labels in s_lab, by one wave: log2 p(l | x), -inf where no alignment fits
template <int PPL>
__device__ __forceinline__ double rs_alpha(const float* __restrict__ Eb, size_t TS, const int* s_lab, int L, int Tp, int blank, int lane) {
  constexpr int CH = Chunk<PPL>::CH;
  int lab[PPL];
  bool vl[PPL], vb[PPL], cs[PPL];
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    const int p = lane * PPL + j;
    vl[j] = p < L;
    vb[j] = p <= L;
    lab[j] = vl[j] ? s_lab[p] : blank;
  }
  {
    const int prev_last = __shfl_up(lab[PPL - 1], 1);
    const bool prev_vl = __shfl_up((int)vl[PPL - 1], 1) != 0;
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int p = lane * PPL + j;
      const int pl = (j > 0) ? lab[j - 1] : prev_last;
      const bool pv = (j > 0) ? vl[j - 1] : (lane > 0 && prev_vl);
      cs[j] = vl[j] && p >= 1 && pv && lab[j] != blank && lab[j] != pl;   // the step over a blank: onto a different label only
    }
  }
  float ab[PPL], al[PPL];   // the virtual frame -1: only state 0 is alive
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    ab[j] = (lane * PPL + j == 0) ? 0.f : kNegInf;
    al[j] = kNegInf;
  }
  Chunk<PPL> cur, nxt;
  auto load = [&](Chunk<PPL>& ch, int t0) {   // frames t0 .. t0 + CH - 1 (t0 a multiple of CH: 16-byte aligned; the over-read stays in the row)
    const float* rb = Eb + (size_t)blank * TS + t0;
#pragma unroll
    for (int q = 0; q < CH / 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(rb + 4 * q);
      ch.eb[4 * q] = v.x; ch.eb[4 * q + 1] = v.y; ch.eb[4 * q + 2] = v.z; ch.eb[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const float* rl = Eb + (size_t)lab[j] * TS + t0;
#pragma unroll
      for (int q = 0; q < CH / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(rl + 4 * q);
        ch.el[4 * q][j] = v.x; ch.el[4 * q + 1][j] = v.y; ch.el[4 * q + 2][j] = v.z; ch.el[4 * q + 3][j] = v.w;
      }
    }
  };
  load(cur, 0);
  double coff = 0.0;
  int since = 0;
  for (int t0 = 0; t0 < Tp; t0 += CH) {
    load(nxt, t0 + CH);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      if (t0 + k < Tp) {
        const float carry = dpp_f32<DPP_WAVE_SHR1>(al[PPL - 1], kNegInf);   // (lane 0: log 0)
        float nb[PPL], nl[PPL];
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
          const float up = (j > 0) ? al[j - 1] : carry;
          nb[j] = vb[j] ? cur.eb[k] + lse2(ab[j], up) : kNegInf;
          nl[j] = vl[j] ? cur.el[k][j] + lse3(al[j], ab[j], cs[j] ? up : kNegInf) : kNegInf;
        }
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
          ab[j] = nb[j];
          al[j] = nl[j];
        }
      }
    }
    cur = nxt;
    since += CH;
    if (since >= 16) {   // renormalise: keep the running log-values O(10)
      since = 0;
      float m = kNegInf;
#pragma unroll
      for (int j = 0; j < PPL; ++j) m = fmaxf(m, fmaxf(ab[j], al[j]));
      m = wave_max_f32(m);
      if (m != kNegInf) {
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
          ab[j] -= m;
          al[j] -= m;
        }
        coff += (double)m;
      }
    }
  }
  // log2 p(l | x) = lse(alpha(2L), alpha(2L - 1)) at the last frame + what was subtracted
  float fb = kNegInf, fl = kNegInf;
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    const int p = lane * PPL + j;
    if (p == L) fb = ab[j];
    if (p == L - 1) fl = al[j];
  }
  for (int o = 32; o > 0; o >>= 1) {   // (exactly one lane holds each)
    fb = fmaxf(fb, __shfl_xor(fb, o));
    fl = fmaxf(fl, __shfl_xor(fl, o));
  }
  const float lfin = lse2(fb, fl);
  return lfin == kNegInf ? -(double)__builtin_huge_valf() : (double)lfin + coff;
}

// grid (ceil(K / 4), B), 256 threads: wave w scores hypothesis blockIdx.x * 4 + w of sample blockIdx.y
__global__ __launch_bounds__(64 * WPB) void k_rescore(const float* __restrict__ E, const int32_t* __restrict__ input_len, int T, int C, int skip,
                                                      int blank, const LexArg lex, int G, const int32_t* __restrict__ hyp,
                                                      const int32_t* __restrict__ hyp_len, int K, int Lh, double* __restrict__ logp,
                                                      int32_t* __restrict__ n_lab) {
  __shared__ int s_off[MAXG + 1];
  __shared__ int s_words[MGR_LEXICON_MAX_WORDS + 1];
  __shared__ int s_lab[WPB][MAXL + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, k = blockIdx.x * WPB + wave;
  const int To = T - skip;
  const size_t TS = rs_ts(To);
  if (G > 0) {
    for (int i = tid; i <= G; i += 64 * WPB) s_off[i] = lex.off[i];
    for (int i = tid; i <= MGR_LEXICON_MAX_WORDS; i += 64 * WPB) s_words[i] = lex.words[i];
  }
  __syncthreads();

  // ---- expansion: the hypothesis' entries (phrase ids with a lexicon, labels without) -> its labels in s_lab[wave], 64 entries a turn
  const bool active = k < K;
  int n = active ? hyp_len[(size_t)b * K + k] : -1;
  if (n > Lh) n = Lh;
  int L = 0;          // the expanded count (wave-uniform)
  bool bad = false;   // a phrase id outside [0, G)
  if (n > 0) {
    const int32_t* row = hyp + ((size_t)b * K + k) * Lh;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      int v = i < n ? row[i] : 0, len = 0, w0 = 0;
      bool badl = false;
      if (i < n) {
        if (G > 0) {
          if (v < 0 || v >= G) badl = true;
          else { w0 = s_off[v]; len = s_off[v + 1] - w0; }
        } else {
          v = v < 0 ? 0 : (v >= C ? C - 1 : v);   // (clipped into the class range, as the loss)
          len = 1;
        }
      }
      int x = len;   // inclusive prefix sum of the lengths over the wave
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
      }
      const int start = L + x - len;
      for (int q = 0; q < len; ++q)
        if (start + q <= MAXL) s_lab[wave][start + q] = G > 0 ? s_words[w0 + q] : v;
      L += __shfl(x, 63);
      bad = bad || __any(badl ? 1 : 0);
    }
  }
  __syncthreads();   // (every wave arrives: nothing above returns)
  if (!active) return;

  const double ninf = -(double)__builtin_huge_valf();
  double r;
  int nl;
  if (n < 0) {                       // no hypothesis in this slot
    r = ninf;
    nl = -1;
  } else if (bad) {                  // not scored
    r = __builtin_nan("");
    nl = -1;
  } else if (L > MAXL) {
    r = __builtin_nan("");
    nl = L;
  } else {
    const int Tp = clip_len(input_len[b], To);
    const float* Eb = E + (size_t)b * C * TS;
    const int ppl = __builtin_amdgcn_readfirstlane((L + 1 + 63) / 64);
    double l2;
    switch (ppl) {
      case 1: l2 = rs_alpha<1>(Eb, TS, s_lab[wave], L, Tp, blank, lane); break;
      case 2: l2 = rs_alpha<2>(Eb, TS, s_lab[wave], L, Tp, blank, lane); break;
      case 3: l2 = rs_alpha<3>(Eb, TS, s_lab[wave], L, Tp, blank, lane); break;
      default: l2 = rs_alpha<4>(Eb, TS, s_lab[wave], L, Tp, blank, lane); break;
    }
    r = l2 == ninf ? ninf : l2 * kLn2;
    nl = L;
  }
  if (lane == 0) {
    logp[(size_t)b * K + k] = r;
    if (n_lab) n_lab[(size_t)b * K + k] = nl;
  }
}

}  // namespace

extern "C" {

// the emission rows only; laid out for T frames (the kernels use rows of T - skip: they fit) to keep the query simple.  The lexicon
// changes nothing about it: hypotheses are expanded in LDS.
struct RescoreWs { float* E; size_t bytes; };
static RescoreWs rescore_ws_layout(void* ws, int B, int T, int C) {
  mgr_ws_carver w(ws);
  return {w.take<float>((size_t)B * C * rs_ts(T)), w.off};
}
size_t mgr_ctc_rescore_ws_bytes(int B, int T, int C, int G, const int32_t* phrase_off) {
  (void)G;
  (void)phrase_off;
  return rescore_ws_layout(nullptr, B > 0 ? B : 1, T > 0 ? T : 1, C > 0 ? C : 1).bytes;
}

int mgr_ctc_rescore(mgr_ctx* c, const float* P, const int32_t* input_len, int B, int T, int C, int skip, int blank, float eps,
                    const int32_t* phrase_off, const int32_t* phrase_words, int G, const int32_t* hyp, const int32_t* hyp_len, int K, int Lh,
                    double* logp, int32_t* n_lab, void* ws, size_t ws_bytes) {
  MGR_REQUIRE(c && P && input_len && hyp && hyp_len && logp, "null argument");
  mgr_planes_forget_range(c, ws, ws_bytes);   // (this call writes its workspace: kept weight planes in it are gone)
  MGR_REQUIRE(B > 0 && T > skip && skip >= 0 && C > 1 && K > 0 && Lh > 0, "bad shape B=%d T=%d C=%d skip=%d K=%d Lh=%d", B, T, C, skip, K, Lh);
  MGR_REQUIRE(B <= 65535, "B = %d too large (max 65535)", B);
  MGR_REQUIRE(Lh <= MGR_RESCORE_MAX_WIDTH, "Lh = %d too large (max %d)", Lh, MGR_RESCORE_MAX_WIDTH);
  MGR_REQUIRE(blank >= 0 && blank < C, "blank %d out of range", blank);
  LexArg lex;
  memset(&lex, 0, sizeof(lex));
  const bool with_lex = phrase_off || phrase_words || G != 0;
  if (with_lex) {
    // the lexicon is host memory: checked here, entry by entry (mgr_ctc_lexicon_decode's rules)
    MGR_REQUIRE(phrase_off && phrase_words, "null argument");
    MGR_REQUIRE(C <= 64, "C = %d too large (max 64)", C);
    MGR_REQUIRE(G >= 1 && G <= MGR_LEXICON_MAX_PHRASES, "G = %d phrases out of [1, %d]", G, MGR_LEXICON_MAX_PHRASES);
    MGR_REQUIRE(phrase_off[0] == 0, "phrase_off[0] = %d, not 0", phrase_off[0]);
    for (int g = 0; g < G; ++g) {
      MGR_REQUIRE(phrase_off[g + 1] > phrase_off[g], "phrase %d is empty", g);
      MGR_REQUIRE(phrase_off[g + 1] <= MGR_LEXICON_MAX_WORDS, "the lexicon has more than %d words", MGR_LEXICON_MAX_WORDS);
      lex.off[g + 1] = (uint8_t)phrase_off[g + 1];
    }
    const int nw = phrase_off[G];
    for (int j = 0; j < nw; ++j) {
      MGR_REQUIRE(phrase_words[j] >= 0 && phrase_words[j] < C && phrase_words[j] != blank, "word %d of the lexicon is %d: not a non-blank class", j,
                  phrase_words[j]);
      lex.words[j] = (uint8_t)phrase_words[j];
    }
  }
  MGR_REQUIRE(ws && ws_bytes >= mgr_ctc_rescore_ws_bytes(B, T, C, G, phrase_off), "workspace too small");
  const int To = T - skip;
  const RescoreWs W = rescore_ws_layout(ws, B, T, C);
  hipStream_t s = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_MISC);
  hipLaunchKernelGGL(k_rescore_emissions, dim3((unsigned)((rs_ts(To) + 255) / 256), B), dim3(256), 0, s, P, input_len, T, C, skip, eps, W.E);
  hipLaunchKernelGGL(k_rescore, dim3((unsigned)((K + WPB - 1) / WPB), B), dim3(64 * WPB), 0, s, W.E, input_len, T, C, skip, blank, lex,
                     with_lex ? G : 0, hyp, hyp_len, K, Lh, logp, n_lab);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}

}  // extern "C"
