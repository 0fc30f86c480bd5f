// K14: CTC hypothesis scoring (not present in the reference): logp[b, k] = ln sum over all CTC alignments of hypothesis k
// of sample b - what rescoring an N-best list needs from every modality: the loss's alpha recursion for K label sequences per sample
// in one launch, without beta, without a stored lattice, with the posteriors read once.
//
// Two kernels.  k_lattice_emissions<base 2> (ctc_lattice.h): class-major log2 y rows per sample, rows that start at t = 0, written once
// and read by the sample's K hypotheses out of L2.  k_rescore: ONE WAVE per hypothesis, four hypotheses of a sample per workgroup - the
// hardware deals a workgroup's waves round over the CU's four SIMDs, so the four chains do not share one (ctc.hip, round 6: chains on
// one SIMD slow each other down).
// Prologue: the wave expands its hypothesis into LDS (hyp_expand of ctc_lattice.h, shared with risk.hip) - without a lexicon the labels
// themselves, with one the words of its phrases.
// Recursion: the loss's alpha, from the pieces of ctc_lattice.h - the (blank, label) pairs across the lanes, PPL pairs per lane, the
// alpha step in base-2 units on the raw exp / log instructions, the renormalisation, emissions fetched a chunk (8 frames, 4 from
// PPL = 3 on) ahead with 16-byte loads.  The wave picks PPL from its OWN expanded length (a wave-uniform branch: gesture hypotheses
// always run PPL = 1).  This file's own loop: the wave maximum is subtracted every 16 frames and summed into an fp64 offset, and the
// recursion starts from a virtual frame -1 (state 0 holds log 1), so the chunks start at t = 0 and an empty input needs no case of its
// own.  Nothing is stored per frame: the two final states and the offset are the result.
#include "ctc_lattice.h"

namespace {

constexpr int MAXG = MGR_LEXICON_MAX_PHRASES;
constexpr int MAXL = MGR_RESCORE_MAX_LABELS;   // 255 labels: 256 pairs, four per lane
constexpr int WPB = 4;                         // waves (hypotheses) per workgroup

// row length of the class-major emissions: To + the over-read of the chunk fetched ahead (at most 15 floats behind the last frame),
// a multiple of 4 floats
__host__ __device__ inline size_t rs_ts(int To) { return ((size_t)To + 16 + 3) / 4 * 4; }

// alpha over the Tp frames of one sample for the L labels in s_lab, by one wave: log2 p(l | x), -inf where no alignment fits
template <int PPL>
__device__ __forceinline__ double rs_alpha(const float* __restrict__ Eb, size_t TS, const int* s_lab, int L, int Tp, int blank, int lane) {
  constexpr int CH = Chunk<PPL>::CH;
  const Pairs<PPL> pr(s_lab, L, blank, lane);
  float ab[PPL], al[PPL];   // the virtual frame -1: only state 0 is alive
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    ab[j] = (lane * PPL + j == 0) ? 0.f : kNegInf;
    al[j] = kNegInf;
  }
  Chunk<PPL> cur, nxt;   // frames t0 .. t0 + CH - 1, t0 a multiple of CH: 16-byte aligned
  cur.load(Eb, TS, blank, pr.lab, 0);
  double coff = 0.0;
  int since = 0;
  for (int t0 = 0; t0 < Tp; t0 += CH) {
    nxt.load(Eb, TS, blank, pr.lab, t0 + CH);
#pragma unroll
    for (int k = 0; k < CH; ++k)
      if (t0 + k < Tp) alpha_step(pr, ab, al, cur.eb[k], cur.el[k]);
    cur = nxt;
    since += CH;
    if (since >= 16) {   // renormalise: keep the running log-values O(10)
      since = 0;
      coff += (double)renorm(ab, al);
    }
  }
  // log2 p(l | x) = lse(alpha(2L), alpha(2L - 1)) at the last frame + what was subtracted
  const float2 f = final_states(ab, al, L, lane);
  const float lfin = lse2(f.x, f.y);
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
  lex_to_lds(lex, G, s_off, s_words, tid, 64 * WPB);
  __syncthreads();

  // ---- expansion: the hypothesis' entries (phrase ids with a lexicon, labels without) -> its labels in s_lab[wave]
  const bool active = k < K;
  const HypLabels h = hyp_expand(hyp + ((size_t)b * K + (active ? k : 0)) * Lh, active ? hyp_len[(size_t)b * K + k] : -1, Lh, G, s_off,
                                 s_words, C, s_lab[wave], MAXL, lane);
  const int n = h.n, L = h.L;
  const bool bad = h.bad;
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
  if (with_lex) {   // (mgr_ctc_lexicon_decode's rules)
    MGR_REQUIRE(phrase_off && phrase_words, "null argument");
    MGR_REQUIRE(C <= 64, "C = %d too large (max 64)", C);
    MGR_REQUIRE(G >= 1 && G <= MGR_LEXICON_MAX_PHRASES, "G = %d phrases out of [1, %d]", G, MGR_LEXICON_MAX_PHRASES);
    if (const int rc = lex_arg_pack(&lex, phrase_off, phrase_words, G, C, blank)) return rc;
  }
  MGR_REQUIRE(ws && ws_bytes >= mgr_ctc_rescore_ws_bytes(B, T, C, G, phrase_off), "workspace too small");
  const int To = T - skip;
  const RescoreWs W = rescore_ws_layout(ws, B, T, C);
  hipStream_t s = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_MISC);
  hipLaunchKernelGGL(k_lattice_emissions<true>, dim3((unsigned)((rs_ts(To) + 255) / 256), B), dim3(256), 0, s, P, input_len, T, C, skip, eps, rs_ts(To),
                     W.E);
  hipLaunchKernelGGL(k_rescore, dim3((unsigned)((K + WPB - 1) / WPB), B), dim3(64 * WPB), 0, s, W.E, input_len, T, C, skip, blank, lex,
                     with_lex ? G : 0, hyp, hyp_len, K, Lh, logp, n_lab);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}

}  // extern "C"
