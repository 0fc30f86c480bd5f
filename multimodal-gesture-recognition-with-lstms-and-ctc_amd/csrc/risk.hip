// K15: expected risk over an N-best list and its gradient w.r.t. the Dense logits (not present in the reference): what
// sequence-level minimum-risk training needs beside the beam decoder, the edit distance and the hypothesis scores - the gradient of
//     Rbar = sum_k w_k r_k,   w = softmax over the live slots of post_scale * logp_k
// through the K CTC likelihoods of a sample, in one call.  With g_k = dRbar / dlogp_k = a w_k (r_k - Rbar), sum_k g_k = 0: every term of
// dlogp_k / dlogits that does not depend on k (the frame's own softmax term of the loss gradient) cancels, and what is left is the g_k -
// weighted sum of the hypotheses' per-class state occupancies, chained through y = softmax(log(P + eps)) and the network's softmax as
// k_ctc_grad chains them.
//
// Three kernels, the loss's form (ctc.hip).  k_lattice_emissions<base 2> (ctc_lattice.h): the class-major log2 y rows, once per sample,
// read by its K hypotheses out of L2.  k_risk_chains: TWO WAVES per hypothesis - alpha forward, beta backward - and two hypotheses
// per workgroup: four chains, one per SIMD (ctc.hip, round 6: chains on one SIMD slow each other down).  The alpha wave expands the slot
// (hyp_expand, shared with rescore.hip), leaves the labels in the workspace for the third kernel, and is rescore.hip's recursion - the
// virtual frame -1, chunks from t = 0, the wave maximum subtracted every 16 frames into an fp64 offset: logp is mgr_ctc_rescore's - with
// a row of (blank, label) state pairs stored per frame.  The beta wave walks the SAME forward emission rows from the last chunk down
// (a chunk is fetched whole and used back to front), renormalised every 16 frames with no offset kept: the third kernel normalises each
// frame's occupancies by their own sum.  k_risk_grad: a thread per frame; thread 0 of a workgroup forms w_k, g_k of its sample from the
// K fp64 logp values (fp64, slot order: every workgroup of a sample gets the same bits), then every thread sums the K weighted
// occupancies of its frame in slot order through two LDS rows.  No atomics anywhere.
//
// Workspace: emissions [B][C][TS] | alpha, beta [B][K][T][2 (Lcap + 1)] f32 each | labels [B][K][Lcap + 1] | counts [B][K]: with the
// lattices stored that is about B K T 2 (Lcap + 1) 8 bytes - 0.6 GB at B = 64, K = 8, T = 1900, Lcap = 40 (computed, not measured).
#include "ctc_lattice.h"

namespace {

constexpr int MAXG = MGR_LEXICON_MAX_PHRASES;
constexpr int MAXL = MGR_RESCORE_MAX_LABELS;
constexpr int HPB = 2;      // hypotheses per workgroup of k_risk_chains: 2 x (alpha, beta) = one chain per SIMD
constexpr int FPB = 128;    // frames (threads) per workgroup of k_risk_grad: two LDS rows of C + 1 floats each

// row length of the class-major emissions: rescore.hip's (To + the over-read of the chunk fetched ahead, a multiple of 4 floats)
__host__ __device__ inline size_t rk_ts(int To) { return ((size_t)To + 16 + 3) / 4 * 4; }

// alpha over the Tp frames for the L labels in s_lab, by one wave: log2 p(l | x), -inf where no alignment fits (rescore.hip's loop).
// A: the hypothesis' alpha rows - row t holds the float2 (blank 2p, label 2p + 1) of pair p <= L at t * S2 + 2 p - or null.
template <int PPL>
__device__ __forceinline__ double rk_alpha(const float* __restrict__ Eb, size_t TS, const int* s_lab, int L, int Tp, int blank, int lane,
                                           float* __restrict__ A, int S2) {
  constexpr int CH = Chunk<PPL>::CH;
  const Pairs<PPL> pr(s_lab, L, blank, lane);
  float ab[PPL], al[PPL];   // the virtual frame -1: only state 0 is alive
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    ab[j] = (lane * PPL + j == 0) ? 0.f : kNegInf;
    al[j] = kNegInf;
  }
  Chunk<PPL> cur, nxt;
  cur.load(Eb, TS, blank, pr.lab, 0);
  double coff = 0.0;
  int since = 0;
  for (int t0 = 0; t0 < Tp; t0 += CH) {
    nxt.load(Eb, TS, blank, pr.lab, t0 + CH);
#pragma unroll
    for (int k = 0; k < CH; ++k)
      if (t0 + k < Tp) {
        alpha_step(pr, ab, al, cur.eb[k], cur.el[k]);
        if (A) {
#pragma unroll
          for (int j = 0; j < PPL; ++j) {
            const int p = lane * PPL + j;
            if (p <= L) *reinterpret_cast<float2*>(A + (size_t)(t0 + k) * S2 + 2 * p) = make_float2(ab[j], al[j]);
          }
        }
      }
    cur = nxt;
    since += CH;
    if (since >= 16) {
      since = 0;
      coff += (double)renorm(ab, al);
    }
  }
  const float2 f = final_states(ab, al, L, lane);
  const float lfin = lse2(f.x, f.y);
  return lfin == kNegInf ? -(double)__builtin_huge_valf() : (double)lfin + coff;
}

// What the beta step needs beside the pairs: the step over the blank INTO pair p + 1's label, seen from pair p.
template <int PPL>
struct BetaSkips {
  bool csn[PPL];
  __device__ __forceinline__ BetaSkips(const Pairs<PPL>& pr, int lane) {
    const int nfirst = __shfl_down((int)pr.cs[0], 1);   // (once per kernel: not on the chain)
#pragma unroll
    for (int j = 0; j < PPL; ++j) csn[j] = (j < PPL - 1) ? pr.cs[j + 1] : (lane < 63 && nfirst != 0);
  }
};

// One time step of beta, from t + 1 down to t: eb / el the emissions of step t + 1 (beta excludes its own step's emission, so that
// alpha + beta is the log-probability of all alignments through a state).
template <int PPL>
__device__ __forceinline__ void beta_step(const Pairs<PPL>& pr, const BetaSkips<PPL>& sk, float (&bb)[PPL], float (&bl)[PPL], float eb,
                                          const float (&el)[PPL]) {
  float xb[PPL], xl[PPL];   // beta(., t + 1) + emission(., t + 1)
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    xb[j] = pr.vb[j] ? bb[j] + eb : kNegInf;
    xl[j] = pr.vl[j] ? bl[j] + el[j] : kNegInf;
  }
  const float nxb = dpp_f32<DPP_WAVE_SHL1>(xb[0], kNegInf);   // (lane 63: log 0)
  const float nxl = dpp_f32<DPP_WAVE_SHL1>(xl[0], kNegInf);
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    const float b1 = (j < PPL - 1) ? xb[j + 1] : nxb;   // blank of pair p + 1 (state u + 1 for the label state)
    const float l1 = (j < PPL - 1) ? xl[j + 1] : nxl;   // label of pair p + 1 (state u + 2)
    bb[j] = pr.vb[j] ? lse2(xb[j], xl[j]) : kNegInf;
    bl[j] = pr.vl[j] ? lse3(xl[j], b1, sk.csn[j] ? l1 : kNegInf) : kNegInf;
  }
}

// beta over the same frames, from Tp - 1 down to 0, rows laid out as alpha's.  Step s -> s - 1 uses the emissions of frame s: the
// chunk [t0, t0 + CH) of the forward rows (t0 a multiple of CH: aligned) is used from its last frame to its first.
template <int PPL>
__device__ __forceinline__ void rk_beta(const float* __restrict__ Eb, size_t TS, const int* s_lab, int L, int Tp, int blank, int lane,
                                        float* __restrict__ Bt, int S2) {
  constexpr int CH = Chunk<PPL>::CH;
  if (Tp <= 0) return;
  const Pairs<PPL> pr(s_lab, L, blank, lane);
  const BetaSkips<PPL> sk(pr, lane);
  float bb[PPL], bl[PPL];
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    const int p = lane * PPL + j;
    bb[j] = (p == L) ? 0.f : kNegInf;
    bl[j] = (p == L - 1) ? 0.f : kNegInf;
    if (p <= L) *reinterpret_cast<float2*>(Bt + (size_t)(Tp - 1) * S2 + 2 * p) = make_float2(bb[j], bl[j]);
  }
  const int tl = (Tp - 1) / CH * CH;
  Chunk<PPL> cur, nxt;
  cur.load(Eb, TS, blank, pr.lab, tl);
  int since = 0;
  for (int t0 = tl; t0 >= 0; t0 -= CH) {
    nxt.load(Eb, TS, blank, pr.lab, t0 >= CH ? t0 - CH : 0);
#pragma unroll
    for (int k = CH - 1; k >= 0; --k) {
      const int s = t0 + k;
      if (s < Tp && s >= 1) {
        beta_step(pr, sk, bb, bl, cur.eb[k], cur.el[k]);
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
          const int p = lane * PPL + j;
          if (p <= L) *reinterpret_cast<float2*>(Bt + (size_t)(s - 1) * S2 + 2 * p) = make_float2(bb[j], bl[j]);
        }
      }
    }
    cur = nxt;
    since += CH;
    if (since >= 16) {
      since = 0;
      renorm(bb, bl);   // (no offset kept: k_risk_grad normalises every frame by its own sum)
    }
  }
}

// grid (ceil(K / 2), B), 256 threads: waves 2 h, 2 h + 1 run alpha, beta of hypothesis blockIdx.x * 2 + h of sample blockIdx.y.
// store = 0: alpha only and nothing stored (no gradient asked for).
__global__ __launch_bounds__(128 * HPB) void k_risk_chains(const float* __restrict__ E, const int32_t* __restrict__ input_len, int T, int C,
                                                           int skip, int blank, const LexArg lex, int G, const int32_t* __restrict__ hyp,
                                                           const int32_t* __restrict__ hyp_len, int K, int Lh, int Lcap, int store,
                                                           double* __restrict__ logp, float* __restrict__ AL, float* __restrict__ BE,
                                                           int32_t* __restrict__ labs, int32_t* __restrict__ nlab) {
  __shared__ int s_off[MAXG + 1];
  __shared__ int s_words[MGR_LEXICON_MAX_WORDS + 1];
  __shared__ int s_lab[HPB][MAXL + 1];
  __shared__ int s_n[HPB], s_L[HPB], s_bad[HPB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = wave >> 1, role = wave & 1;
  const int b = blockIdx.y, k = blockIdx.x * HPB + h;
  const int To = T - skip, S2 = 2 * (Lcap + 1);
  const size_t TS = rk_ts(To);
  lex_to_lds(lex, G, s_off, s_words, tid, 128 * HPB);
  __syncthreads();
  const bool active = k < K;
  const size_t slot = (size_t)b * K + (active ? k : 0);
  if (role == 0) {   // the alpha wave expands the slot for both
    const HypLabels e = hyp_expand(hyp + slot * Lh, active ? hyp_len[slot] : -1, Lh, G, s_off, s_words, C, s_lab[h], MAXL, lane);
    if (lane == 0) {
      s_n[h] = e.n;
      s_L[h] = e.L;
      s_bad[h] = e.bad ? 1 : 0;
    }
  }
  __syncthreads();   // (every wave arrives: nothing above returns)
  if (!active) return;
  const int n = s_n[h], L = s_L[h];
  if (n < 0 || s_bad[h] || L > Lcap) {   // absent / not scored: no lattice, no part in the weights
    if (role == 0 && lane == 0) {
      logp[slot] = n < 0 ? -(double)__builtin_huge_valf() : __builtin_nan("");
      nlab[slot] = -1;
    }
    return;
  }
  const int Tp = clip_len(input_len[b], To);
  const float* Eb = E + (size_t)b * C * TS;
  float* A = store ? AL + slot * (size_t)T * S2 : nullptr;
  float* Bt = store ? BE + slot * (size_t)T * S2 : nullptr;
  const int ppl = __builtin_amdgcn_readfirstlane((L + 1 + 63) / 64);
  if (role == 0) {
    double l2;
    switch (ppl) {
      case 1: l2 = rk_alpha<1>(Eb, TS, s_lab[h], L, Tp, blank, lane, A, S2); break;
      case 2: l2 = rk_alpha<2>(Eb, TS, s_lab[h], L, Tp, blank, lane, A, S2); break;
      case 3: l2 = rk_alpha<3>(Eb, TS, s_lab[h], L, Tp, blank, lane, A, S2); break;
      default: l2 = rk_alpha<4>(Eb, TS, s_lab[h], L, Tp, blank, lane, A, S2); break;
    }
    const double ninf = -(double)__builtin_huge_valf();
    for (int i = lane; i < L; i += 64) labs[slot * (Lcap + 1) + i] = s_lab[h][i];
    if (lane == 0) {
      logp[slot] = l2 == ninf ? ninf : l2 * kLn2;
      nlab[slot] = L;
    }
  } else if (store) {
    switch (ppl) {
      case 1: rk_beta<1>(Eb, TS, s_lab[h], L, Tp, blank, lane, Bt, S2); break;
      case 2: rk_beta<2>(Eb, TS, s_lab[h], L, Tp, blank, lane, Bt, S2); break;
      case 3: rk_beta<3>(Eb, TS, s_lab[h], L, Tp, blank, lane, Bt, S2); break;
      default: rk_beta<4>(Eb, TS, s_lab[h], L, Tp, blank, lane, Bt, S2); break;
    }
  }
}

// grid (ceil(T / 128), B), 128 threads (dLogits null: grid (1, B), the prologue only).
__global__ __launch_bounds__(FPB) void k_risk_grad(const float* __restrict__ P, const int32_t* __restrict__ input_len, int T, int C, int skip,
                                                   int blank, float eps, int K, int Lcap, const int32_t* __restrict__ risk, float risk_scale,
                                                   float post_scale, float gscale, int accumulate, const double* __restrict__ logp,
                                                   const float* __restrict__ AL, const float* __restrict__ BE,
                                                   const int32_t* __restrict__ labs, const int32_t* __restrict__ nlab,
                                                   float* __restrict__ weight, float* __restrict__ exp_risk, float* __restrict__ dLogits) {
  // g [32] | L [32]: the label count of a live slot, -1 otherwise | e [32] fp64: exp(a logp - max) | [FPB][C + 1] weighted occupancies |
  // [FPB][C + 1] one hypothesis' own (all of it dynamic: the limit set for the kernel is the whole 160 KiB)
  extern __shared__ __attribute__((aligned(16))) float smem_all[];
  float* s_g = smem_all;
  int* s_L = reinterpret_cast<int*>(smem_all + MGR_RISK_MAX_SLOTS);
  double* s_e = reinterpret_cast<double*>(smem_all + 2 * MGR_RISK_MAX_SLOTS);
  float* smem = smem_all + 4 * MGR_RISK_MAX_SLOTS;
  const int tid = threadIdx.x, b = blockIdx.y;
  const size_t slot0 = (size_t)b * K;
  if (tid == 0) {   // w, Rbar, g of the sample: fp64, slot order
    const double a = (double)post_scale, rs = (double)risk_scale, ninf = -(double)__builtin_huge_valf();
    double m = ninf;
    int live = 0;
    for (int k = 0; k < K; ++k) {
      const double lp = logp[slot0 + k];
      const bool lv = nlab[slot0 + k] >= 0 && lp > ninf;   // (NaN compares false)
      s_L[k] = lv ? nlab[slot0 + k] : -1;
      if (lv) {
        ++live;
        if (a * lp > m) m = a * lp;
      }
    }
    double sum = 0.0, rbar = 0.0;
    for (int k = 0; k < K; ++k) {   // exp(a logp_k - m), once per slot
      s_e[k] = s_L[k] >= 0 ? exp(a * logp[slot0 + k] - m) : 0.0;
      sum += s_e[k];
    }
    for (int k = 0; k < K; ++k)
      if (s_L[k] >= 0) rbar += s_e[k] / sum * ((double)risk[slot0 + k] * rs);
    for (int k = 0; k < K; ++k) {
      const double w = s_L[k] >= 0 ? s_e[k] / sum : 0.0;
      s_g[k] = (live >= 2 && s_L[k] >= 0) ? (float)(a * w * ((double)risk[slot0 + k] * rs - rbar)) : 0.f;
      if (blockIdx.x == 0 && weight) weight[slot0 + k] = (float)w;
    }
    if (blockIdx.x == 0) exp_risk[b] = (float)rbar;
  }
  __syncthreads();
  const int f = blockIdx.x * FPB + tid;
  if (!dLogits || f >= T) return;
  float* out = dLogits + ((size_t)b * T + f) * C;
  const int tt = f - skip, Tp = clip_len(input_len[b], T - skip);
  if (tt < 0 || tt >= Tp) {   // skipped and out-of-length frames: zero, as k_ctc_grad
    if (!accumulate)
      for (int c = 0; c < C; ++c) out[c] = 0.f;
    return;
  }
  float* occ = smem + (size_t)tid * (C + 1);
  float* own = smem + (size_t)(FPB + tid) * (C + 1);
  for (int c = 0; c < C; ++c) occ[c] = 0.f;
  const int S2 = 2 * (Lcap + 1);
  for (int k = 0; k < K; ++k) {
    const int L = s_L[k];
    const float g = s_g[k];
    if (L < 0 || g == 0.f) continue;
    const float* ar = AL + ((slot0 + k) * (size_t)T + tt) * S2;
    const float* br = BE + ((slot0 + k) * (size_t)T + tt) * S2;
    const int32_t* lab = labs + (slot0 + k) * (Lcap + 1);
    for (int c = 0; c < C; ++c) own[c] = 0.f;
    float vmax = kNegInf;
    for (int p = 0; p <= L; ++p) {
      const float2 al = *reinterpret_cast<const float2*>(ar + 2 * p);
      const float2 be = *reinterpret_cast<const float2*>(br + 2 * p);
      vmax = fmaxf(vmax, al.x + be.x);
      if (p < L) vmax = fmaxf(vmax, al.y + be.y);
    }
    float den = 0.f;
    for (int p = 0; p <= L; ++p) {
      const float2 al = *reinterpret_cast<const float2*>(ar + 2 * p);
      const float2 be = *reinterpret_cast<const float2*>(br + 2 * p);
      const float wb = exp2_raw(al.x + be.x - vmax);
      own[blank] += wb;
      den += wb;
      if (p < L) {
        const float wl = exp2_raw(al.y + be.y - vmax);
        own[lab[p]] += wl;
        den += wl;
      }
    }
    const float sc = g / den;   // sum_u alpha beta = p(l | x) at every t: the frame's own sum normalises
    for (int c = 0; c < C; ++c) occ[c] += own[c] * sc;
  }
  const float* row = P + ((size_t)b * T + f) * C;
  float dot = 0.f;
  for (int c = 0; c < C; ++c) {
    const float gp = occ[c] / (row[c] + eps);
    occ[c] = gp;
    dot += row[c] * gp;
  }
  for (int c = 0; c < C; ++c) {
    const float v = row[c] * (occ[c] - dot) * gscale;
    out[c] = accumulate ? out[c] + v : v;
  }
}

}  // namespace

extern "C" {

// emissions | alpha | beta | the expanded labels | their counts; rows laid out for T frames (the kernels use T - skip: they fit), as
// K14's.  The lexicon changes nothing about it: hypotheses are expanded in LDS, Lcap bounds what is kept.
struct RiskWs { float *E, *AL, *BE; int32_t *labs, *nlab; size_t bytes; };
static RiskWs risk_ws_layout(void* ws, int B, int T, int C, int K, int Lcap) {
  mgr_ws_carver w(ws);
  const size_t ab = (size_t)B * K * T * 2 * (Lcap + 1);
  return {w.take<float>((size_t)B * C * rk_ts(T)), w.take<float>(ab), w.take<float>(ab), w.take<int32_t>((size_t)B * K * (Lcap + 1)),
          w.take<int32_t>((size_t)B * K), w.off};
}
size_t mgr_ctc_risk_ws_bytes(int B, int T, int C, int K, int Lcap, int G, const int32_t* phrase_off) {
  (void)G;
  (void)phrase_off;
  return risk_ws_layout(nullptr, B > 0 ? B : 1, T > 0 ? T : 1, C > 0 ? C : 1, K > 0 ? K : 1, Lcap > 0 ? Lcap : 1).bytes;
}

int mgr_ctc_risk_grad(mgr_ctx* c, const float* P, const int32_t* input_len, int B, int T, int C, int skip, int blank, float eps,
                      const int32_t* phrase_off, const int32_t* phrase_words, int G, const int32_t* hyp, const int32_t* hyp_len, int K, int Lh,
                      int Lcap, const int32_t* risk, float risk_scale, float post_scale, float gscale, int accumulate, double* logp,
                      float* weight, float* exp_risk, float* dLogits, void* ws, size_t ws_bytes) {
  MGR_REQUIRE(c && P && input_len && hyp && hyp_len && risk && logp && exp_risk, "null argument");
  mgr_planes_forget_range(c, ws, ws_bytes);   // (this call writes its workspace: kept weight planes in it are gone)
  MGR_REQUIRE(B > 0 && T > skip && skip >= 0 && C > 1 && Lh > 0, "bad shape B=%d T=%d C=%d skip=%d Lh=%d", B, T, C, skip, Lh);
  MGR_REQUIRE(K >= 1 && K <= MGR_RISK_MAX_SLOTS, "K = %d out of [1, %d]", K, MGR_RISK_MAX_SLOTS);
  MGR_REQUIRE(Lcap >= 1 && Lcap <= MGR_RESCORE_MAX_LABELS, "Lcap = %d out of [1, %d]", Lcap, MGR_RESCORE_MAX_LABELS);
  MGR_REQUIRE(B <= 65535, "B = %d too large (max 65535)", B);
  MGR_REQUIRE(Lh <= MGR_RESCORE_MAX_WIDTH, "Lh = %d too large (max %d)", Lh, MGR_RESCORE_MAX_WIDTH);
  MGR_REQUIRE(blank >= 0 && blank < C, "blank %d out of range", blank);
  MGR_REQUIRE(post_scale > 0.f && post_scale <= 3.0e38f, "post_scale %g is not a positive finite number", (double)post_scale);
  LexArg lex;
  memset(&lex, 0, sizeof(lex));
  const bool with_lex = phrase_off || phrase_words || G != 0;
  if (with_lex) {   // (mgr_ctc_lexicon_decode's rules)
    MGR_REQUIRE(phrase_off && phrase_words, "null argument");
    MGR_REQUIRE(C <= 64, "C = %d too large (max 64)", C);
    MGR_REQUIRE(G >= 1 && G <= MGR_LEXICON_MAX_PHRASES, "G = %d phrases out of [1, %d]", G, MGR_LEXICON_MAX_PHRASES);
    if (const int rc = lex_arg_pack(&lex, phrase_off, phrase_words, G, C, blank)) return rc;
  }
  MGR_REQUIRE(ws && ws_bytes >= mgr_ctc_risk_ws_bytes(B, T, C, K, Lcap, G, phrase_off), "workspace too small");
  const size_t lds = ((size_t)2 * FPB * (C + 1) + 4 * MGR_RISK_MAX_SLOTS) * sizeof(float);
  MGR_REQUIRE(lds <= 160 * 1024, "C=%d too large for the LDS occupancy rows", C);
  if (!(c->attr_done & MGR_ATTR_RISK)) {
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_risk_grad), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    c->attr_done |= MGR_ATTR_RISK;
  }
  const int To = T - skip;
  const RiskWs W = risk_ws_layout(ws, B, T, C, K, Lcap);
  hipStream_t s = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_CTC);
  hipLaunchKernelGGL(k_lattice_emissions<true>, dim3((unsigned)((rk_ts(To) + 255) / 256), B), dim3(256), 0, s, P, input_len, T, C, skip, eps, rk_ts(To),
                     W.E);
  hipLaunchKernelGGL(k_risk_chains, dim3((unsigned)((K + HPB - 1) / HPB), B), dim3(128 * HPB), 0, s, W.E, input_len, T, C, skip, blank, lex,
                     with_lex ? G : 0, hyp, hyp_len, K, Lh, Lcap, dLogits ? 1 : 0, logp, W.AL, W.BE, W.labs, W.nlab);
  hipLaunchKernelGGL(k_risk_grad, dim3(dLogits ? (unsigned)((T + FPB - 1) / FPB) : 1u, B), dim3(FPB), lds, s, P, input_len, T, C, skip, blank, eps, K,
                     Lcap, risk, risk_scale, post_scale, gscale, accumulate, logp, W.AL, W.BE, W.labs, W.nlab, weight, exp_risk, dLogits);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_CTC);
  return 0;
}

}  // extern "C"
