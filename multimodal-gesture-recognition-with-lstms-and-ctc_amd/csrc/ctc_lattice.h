// The CTC lattice, once: what every kernel that walks the extended label sequence l' = [blank, l1, blank, ..., lL, blank] shares - the
// loss (ctc.hip), forced alignment (align.hip), hypothesis scoring (rescore.hip), the expected-risk gradient (risk.hip) - and the
// smaller pieces the lexicon decode (lexicon.hip) and the edit distance (edit.hip) take from the same place.  Every numerics decision of the loss lives here: base-2 raw
// exp / log, the -3e38 floor, DPP in place of ds_bpermute, the renormalisation, the skip onto a different label only.
//
// Form: the extended sequence lies across the lanes of ONE WAVE as (blank, label) PAIRS - pair p = lane * PPL + j holds states 2p (blank)
// and 2p + 1 (label p), PPL = 1 .. 4 pairs per lane - so the only cross-lane traffic of a time step is one shift-by-one of the
// neighbouring pair's label state.  Emissions are class-major rows (a row per class, time along the row), fetched a chunk of time steps
// ahead of the recursion with 16-byte loads, so the serial chain per step is shift -> combine -> add.
//
// What is here is pieces, not a recursion: each kernel keeps its own loop - its chunk origin, its renormalisation cadence, what it stores
// per step - because those decide the bits of its result.  The max / back-pointer step (align.hip) and the beta steps (ctc.hip, whose
// step is interleaved with its two-steps-a-time stores, and risk.hip) have one user each and live there.  Everything is force-inlined
// into its caller: a translation unit pays for what it uses.
#pragma once
#include "common.h"

namespace {

// ---- numerics ------------------------------------------------------------------------------------------------------------------

constexpr float kNegInf = -__builtin_huge_valf();

// The recursions run in BASE-2 log units (round 6): log2 y emissions, log2 alpha / beta, so that a log-sum-exp is v_exp_f32 / v_log_f32
// on their own - no log2(e) / ln 2 multiplications, and none of logf's denormal-range and last-ulp fix-ups either: the argument of the
// logarithm lies in [1, 3] (the largest term contributes exactly 1), where the raw instruction's 1 ulp is 1e-7 absolute on values that
// are added to numbers of size O(10).  That was 30 of the 95 instructions of a step of the serial chain (12 for each logf).
// All-(-inf) inputs (log 0): the maximum is floored at a huge finite negative number, x - floor stays -inf, 2^-inf = 0, log2 0 = -inf.
constexpr float kLseFloor = -3.0e38f;
constexpr double kLn2 = 0.693147180559945309417232121458;
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

// ---- wave operations -----------------------------------------------------------------------------------------------------------

// Cross-lane traffic of the recursions through DPP (one v_mov_b32_dpp, a few cycles) instead of __shfl_* (a ds_bpermute round trip
// through the LDS crossbar, ~100 cycles, on the serial chain of every time step): wave_shr:1 / wave_shl:1 move a value to the
// next / previous lane of the whole wave, row_shr:n to the n-th next lane inside a row of 16 lanes; lanes without a source receive
// `fill`.
constexpr int DPP_WAVE_SHR1 = 0x138, DPP_WAVE_SHL1 = 0x130;
constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118;
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v, float fill) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// wave-wide maximum: DPP within the rows of 16 lanes, then the four row results through v_readlane (uniform)
__device__ __forceinline__ float wave_max_f32(float m) {
  m = fmaxf(m, dpp_f32<DPP_ROW_SHR1>(m, m));   // (lanes without a source keep their own value)
  m = fmaxf(m, dpp_f32<DPP_ROW_SHR2>(m, m));
  m = fmaxf(m, dpp_f32<DPP_ROW_SHR4>(m, m));
  m = fmaxf(m, dpp_f32<DPP_ROW_SHR8>(m, m));   // lane 15 of a row holds the row's maximum
  const int i = __float_as_int(m);
  return fmaxf(fmaxf(__int_as_float(__builtin_amdgcn_readlane(i, 15)), __int_as_float(__builtin_amdgcn_readlane(i, 31))),
               fmaxf(__int_as_float(__builtin_amdgcn_readlane(i, 47)), __int_as_float(__builtin_amdgcn_readlane(i, 63))));
}

// lengths and indices are device data: into [0, hi]
__device__ __forceinline__ int clip_len(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// a label into the class range [0, C), as the loss clips it: every lattice kernel reads the rows of the class it gets here
__device__ __forceinline__ int clip_label(int v, int C) { return v < 0 ? 0 : (v >= C ? C - 1 : v); }

// ---- the lattice across the lanes ------------------------------------------------------------------------------------------------

// What a lane knows about its PPL pairs, from the L labels of a row in LDS (already clipped into the class range).
template <int PPL>
struct Pairs {
  int lab[PPL];    // the pair's label (the blank where the pair has none: its row is fetched and not used)
  bool vl[PPL];    // the label state 2p + 1 exists: p < L
  bool vb[PPL];    // the blank state 2p exists: p <= L
  bool cs[PPL];    // the step over the blank, from label p - 1 straight to label p: onto a different label only
  __device__ __forceinline__ Pairs(const int* s_lab, int L, int blank, int lane) {
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int p = lane * PPL + j;
      vl[j] = p < L;
      vb[j] = p <= L;
      lab[j] = vl[j] ? s_lab[p] : blank;
    }
    const int prev_last = __shfl_up(lab[PPL - 1], 1);   // (once per kernel: not on the chain)
    const bool prev_vl = __shfl_up((int)vl[PPL - 1], 1) != 0;
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int p = lane * PPL + j;
      const int pl = (j > 0) ? lab[j - 1] : prev_last;
      const bool pv = (j > 0) ? vl[j - 1] : (lane > 0 && prev_vl);
      cs[j] = vl[j] && p >= 1 && pv && lab[j] != blank && lab[j] != pl;
    }
  }
};

// A prefetched chunk of emissions: CH time steps of the blank's row and of the rows of the lane's PPL labels.
template <int PPL>
struct Chunk {
  static constexpr int CH = PPL <= 2 ? 8 : 4;   // time steps per prefetched chunk (a multiple of 4: float4 loads along time)
  float eb[CH];
  float el[CH][PPL];
  // steps t0 .. t0 + CH - 1 of class-major rows of length TS; E: where step 0 of class 0 lies.  E + t0 is 16-byte aligned (the
  // callers' chunk origins and row offsets see to that) and the over-read behind a sample's last step stays inside the row.
  __device__ __forceinline__ void load(const float* E, size_t TS, int blank, const int (&lab)[PPL], int t0) {
    const float* rb = E + (size_t)blank * TS + t0;
#pragma unroll
    for (int q = 0; q < CH / 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(rb + 4 * q);
      eb[4 * q] = v.x; eb[4 * q + 1] = v.y; eb[4 * q + 2] = v.z; eb[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const float* rl = E + (size_t)lab[j] * TS + t0;
#pragma unroll
      for (int q = 0; q < CH / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(rl + 4 * q);
        el[4 * q][j] = v.x; el[4 * q + 1][j] = v.y; el[4 * q + 2][j] = v.z; el[4 * q + 3][j] = v.w;
      }
    }
  }
};

// Renormalise: the wave-wide maximum of the running values is subtracted, so that they stay O(10) instead of O(-5000) at T = 1900, where
// an fp32 ulp is 5e-4.  Returns what was subtracted, for the caller's fp64 offset (beta needs none: the gradient normalises each frame
// by its own sum); 0 where every state is dead (log 0) and nothing was.
template <int PPL>
__device__ __forceinline__ float renorm(float (&ab)[PPL], float (&al)[PPL]) {
  float m = kNegInf;
#pragma unroll
  for (int j = 0; j < PPL; ++j) m = fmaxf(m, fmaxf(ab[j], al[j]));
  m = wave_max_f32(m);
  if (m == kNegInf) return 0.f;
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    ab[j] -= m;
    al[j] -= m;
  }
  return m;
}

// The two states a complete alignment ends in, on every lane: x = the last blank 2L, y = the last label 2L - 1 (-inf without labels).
template <int PPL>
__device__ __forceinline__ float2 final_states(const float (&ab)[PPL], const float (&al)[PPL], int L, int lane) {
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
  return make_float2(fb, fl);
}

// One time step of alpha: eb / el the step's emissions of the blank and of the lane's labels.
template <int PPL>
__device__ __forceinline__ void alpha_step(const Pairs<PPL>& pr, float (&ab)[PPL], float (&al)[PPL], float eb, const float (&el)[PPL]) {
  const float carry = dpp_f32<DPP_WAVE_SHR1>(al[PPL - 1], kNegInf);   // (lane 0: log 0)
  float nb[PPL], nl[PPL];
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    const float up = (j > 0) ? al[j - 1] : carry;
    nb[j] = pr.vb[j] ? eb + lse2(ab[j], up) : kNegInf;
    nl[j] = pr.vl[j] ? el[j] + lse3(al[j], ab[j], pr.cs[j] ? up : kNegInf) : kNegInf;
  }
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    ab[j] = nb[j];
    al[j] = nl[j];
  }
}

// ---- the entropy of the paths into a state, carried beside alpha / beta -------------------------------------------------

// lse2 / lse3 that also hand out their maximum, their terms 2^(x - m), the terms' sum and its logarithm: the operations of lse2 / lse3
// in their order, so the same bits.
__device__ __forceinline__ float lse2_terms(float a, float b, float& m, float& ea, float& eb, float& s, float& lg) {
  m = fmaxf(fmaxf(a, b), kLseFloor);
  ea = exp2_raw(a - m);
  eb = exp2_raw(b - m);
  s = ea + eb;
  lg = log2_raw(s);
  return m + lg;
}
__device__ __forceinline__ float lse3_terms(float a, float b, float c, float& m, float& ea, float& eb, float& ec, float& s, float& lg) {
  m = fmaxf(fmaxf(fmaxf(a, b), c), kLseFloor);
  ea = exp2_raw(a - m);
  eb = exp2_raw(b - m);
  ec = exp2_raw(c - m);
  s = ea + eb + ec;
  lg = log2_raw(s);
  return m + lg;
}
// The chain rule of the entropy over one log-sum-exp: with predecessors r of log-weight x_r, w_r = 2^(x_r - m) / s, and h_r the entropy
// (base 2) of the paths into r,  h = sum_r w_r h_r - sum_r w_r log2 w_r = log2 s + sum_r w_r (h_r - (x_r - m)).  A predecessor of
// weight 0 (log 0) is left out by SELECTION: its x_r - m is -inf, and 0 * -inf is not 0.  s = 0 (every predecessor dead): the caller selects the result away.
// With d_r what the float32 recursion has rounded away from x_r (below), the weights that belong to the exact recursion are those of
// x_r + d_r: to first order w_r (1 + ln 2 (d_r - D)), D = sum_r w_r d_r, with log2 of their normaliser log2 s + D.  The chain rule is
// taken over THOSE weights - at |alpha| = 1600 neighbouring d differ by 1e-4, and weights off by that much leave as much in h at every
// step.  D: the caller's sum_r w_r d_r.
__device__ __forceinline__ float ent_term(float e, float h, float x, float m, float d, float D) {
  return e > 0.f ? e * (1.f + (float)kLn2 * (d - D)) * ((h - d) - (x - m)) : 0.f;
}
__device__ __forceinline__ float ent_chain2(float m, float s, float lg, float D, float ea, float ha, float xa, float da, float eb, float hb,
                                            float xb, float db) {
  return (lg + D) + (ent_term(ea, ha, xa, m, da, D) + ent_term(eb, hb, xb, m, db, D)) * __builtin_amdgcn_rcpf(s);
}
__device__ __forceinline__ float ent_chain3(float m, float s, float lg, float D, float ea, float ha, float xa, float da, float eb, float hb,
                                            float xb, float db, float ec, float hc, float xc, float dc) {
  return (lg + D) + (ent_term(ea, ha, xa, m, da, D) + ent_term(eb, hb, xb, m, db, D) + ent_term(ec, hc, xc, m, dc, D)) * __builtin_amdgcn_rcpf(s);
}
// (a + b) - fl(a + b) exactly (Knuth's two-sum; s = fl(a + b)).  Not finite where an operand is not: the callers select such results away.
__device__ __forceinline__ float add_err(float a, float b, float s) {
  const float bv = s - a;
  return (a - (s - bv)) + (b - bv);
}
// sum_r (e_r / s) x_r, a term of weight 0 left out by selection (its x_r may not be finite)
__device__ __forceinline__ float wsel(float e, float x) { return e > 0.f ? e * x : 0.f; }

// alpha_step with two more values per state:
//   h(t, s)  the entropy of the distribution over the prefixes that end in s at t, i.e. log2 alpha(t, s) minus the expected
//            log2-probability of such a prefix (the chain rule above).  h >= 0 grows by what the alignments add, not per frame: it needs
//            no renormalisation and no offset;
//   d(t, s)  what the float32 additions of the alpha recursion have rounded away on the way into s: alpha + d is, to first order, the
//            recursion's value had its additions been exact - d = sum_r w_r d_r + the two-sum errors of the step's own two additions.
// alpha's own operations are alpha_step's (the same bits); a dead state (alpha = log 0) keeps h = d = 0, so every stored value is finite.
template <int PPL>
__device__ __forceinline__ void alpha_step_ent(const Pairs<PPL>& pr, float (&ab)[PPL], float (&al)[PPL], float (&hb)[PPL], float (&hl)[PPL],
                                               float (&db)[PPL], float (&dl)[PPL], float eb, const float (&el)[PPL]) {
  const float carry = dpp_f32<DPP_WAVE_SHR1>(al[PPL - 1], kNegInf);   // (lane 0: log 0)
  const float hcarry = dpp_f32<DPP_WAVE_SHR1>(hl[PPL - 1], 0.f);
  const float dcarry = dpp_f32<DPP_WAVE_SHR1>(dl[PPL - 1], 0.f);
  float nb[PPL], nl[PPL], nhb[PPL], nhl[PPL], ndb[PPL], ndl[PPL];
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    const float up = (j > 0) ? al[j - 1] : carry;
    const float hup = (j > 0) ? hl[j - 1] : hcarry;
    const float dup = (j > 0) ? dl[j - 1] : dcarry;
    const float skp = pr.cs[j] ? up : kNegInf;
    float m, e0, e1, e2, s, lg;
    {
      const float lb = lse2_terms(ab[j], up, m, e0, e1, s, lg);
      const float v = eb + lb;
      nb[j] = pr.vb[j] ? v : kNegInf;
      const bool dead = nb[j] == kNegInf;
      const float D = (wsel(e0, db[j]) + wsel(e1, dup)) * __builtin_amdgcn_rcpf(s);
      nhb[j] = dead ? 0.f : ent_chain2(m, s, lg, D, e0, hb[j], ab[j], db[j], e1, hup, up, dup);
      ndb[j] = dead ? 0.f : D + (add_err(m, lg, lb) + add_err(eb, lb, v));
    }
    {
      const float ll = lse3_terms(al[j], ab[j], skp, m, e0, e1, e2, s, lg);
      const float v = el[j] + ll;
      nl[j] = pr.vl[j] ? v : kNegInf;
      const bool dead = nl[j] == kNegInf;
      const float D = (wsel(e0, dl[j]) + wsel(e1, db[j]) + wsel(e2, dup)) * __builtin_amdgcn_rcpf(s);
      nhl[j] = dead ? 0.f : ent_chain3(m, s, lg, D, e0, hl[j], al[j], dl[j], e1, hb[j], ab[j], db[j], e2, hup, skp, dup);
      ndl[j] = dead ? 0.f : D + (add_err(m, lg, ll) + add_err(el[j], ll, v));
    }
  }
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    ab[j] = nb[j];
    al[j] = nl[j];
    hb[j] = nhb[j];
    hl[j] = nhl[j];
    db[j] = ndb[j];
    dl[j] = ndl[j];
  }
}

// renorm that also adds what its subtraction rounds away to d (nothing on dead states): the same wave-wide maximum, the same
// subtraction, the same bits in ab / al.
template <int PPL>
__device__ __forceinline__ float renorm_ent(float (&ab)[PPL], float (&al)[PPL], float (&db)[PPL], float (&dl)[PPL]) {
  float m = kNegInf;
#pragma unroll
  for (int j = 0; j < PPL; ++j) m = fmaxf(m, fmaxf(ab[j], al[j]));
  m = wave_max_f32(m);
  if (m == kNegInf) return 0.f;
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    const float vb = ab[j] - m, vl = al[j] - m;
    if (ab[j] != kNegInf) db[j] += add_err(ab[j], -m, vb);
    if (al[j] != kNegInf) dl[j] += add_err(al[j], -m, vl);
    ab[j] = vb;
    al[j] = vl;
  }
  return m;
}

// What the entropy's gradient kernel reads in alpha's (beta's) rows when rel is set (wave-uniform): the state's value relative to the
// step's wave-wide maximum with d put back, (v - max) + d - small for every state that matters, so that neither its own float32
// rounding nor the recursion's is left in it.  A constant of the frame is of no account there: occupancies are normalised per frame,
// and only differences between states enter the entropy's gradient.  rel off: v itself, the loss's rows.
template <int PPL>
__device__ __forceinline__ void ent_rows(bool rel, const float (&vb)[PPL], const float (&vl)[PPL], const float (&db)[PPL], const float (&dl)[PPL],
                                         float (&sb)[PPL], float (&sl)[PPL]) {
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    sb[j] = vb[j];
    sl[j] = vl[j];
  }
  if (!rel) return;
  float m = kNegInf;
#pragma unroll
  for (int j = 0; j < PPL; ++j) m = fmaxf(m, fmaxf(vb[j], vl[j]));
  m = wave_max_f32(m);
  if (m == kNegInf) return;
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    sb[j] = (vb[j] - m) + db[j];   // (a dead state: -inf + 0)
    sl[j] = (vl[j] - m) + dl[j];
  }
}

// ---- emissions -------------------------------------------------------------------------------------------------------------------

template <bool BASE2>
__device__ __forceinline__ float emission_log(float x) { return BASE2 ? log2f(x) : logf(x); }
// the frame's normaliser log(sum_c (P + eps)): the emissions are y = softmax(log(P + eps)), as the reference's loss forms them
template <bool BASE2>
__device__ __forceinline__ float frame_log_norm(const float* __restrict__ row, int C, float eps) {
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += row[c] + eps;
  return emission_log<BASE2>(s);
}

// emissions log y(t, c) = log(P + eps) - log(sum_c (P + eps)), class-major: E[b][c][TS], in base-2 (BASE2) or natural-log units.  One
// frame per thread, grid (ceil(TS / 256), B); the frames of a row behind the sample's length (the recursions' prefetch reads them and
// uses none) are zeros.  row_len: the caller's row length TS (To + its own over-read, a multiple of 4 floats).
template <bool BASE2>
__global__ __launch_bounds__(256) void k_lattice_emissions(const float* __restrict__ P, const int32_t* __restrict__ input_len, int T, int C,
                                                           int skip, float eps, size_t row_len, float* __restrict__ E) {
  // (a multiple of 4 already; formed so that the compiler knows it: given a stride that might be 1 it keeps its unrolled store loop for
  // that case alone and writes the rows one class per trip)
  const size_t TS = row_len / 4 * 4;
  const int b = blockIdx.y, To = T - skip;
  const int Tp = clip_len(input_len[b], To);
  const int t = blockIdx.x * 256 + threadIdx.x;
  if ((size_t)t >= TS) return;
  float* Eb = E + (size_t)b * C * TS;
  if (t >= Tp) {
    for (int c = 0; c < C; ++c) Eb[(size_t)c * TS + t] = 0.f;
    return;
  }
  const float* row = P + ((size_t)b * T + skip + t) * C;
  const float ls = frame_log_norm<BASE2>(row, C, eps);
  for (int c = 0; c < C; ++c) Eb[(size_t)c * TS + t] = emission_log<BASE2>(row[c] + eps) - ls;
}

// ---- the phrase lexicon as a kernel argument -------------------------------------------------------------------------------------

// the lexicon travels as a kernel argument: word ids are below 64, offsets at most 255
struct LexArg {
  uint8_t off[MGR_LEXICON_MAX_PHRASES + 1];
  uint8_t words[MGR_LEXICON_MAX_WORDS + 1];
};

// The lexicon is host memory: checked here, entry by entry, and packed into *lex (zeroed by the caller, who has also checked G against
// [1, MGR_LEXICON_MAX_PHRASES] and C against 64).  Returns 0, or the error code with mgr_last_error set.
static inline int lex_arg_pack(LexArg* lex, const int32_t* phrase_off, const int32_t* phrase_words, int G, int C, int blank) {
  MGR_REQUIRE(phrase_off[0] == 0, "phrase_off[0] = %d, not 0", phrase_off[0]);
  for (int g = 0; g < G; ++g) {
    MGR_REQUIRE(phrase_off[g + 1] > phrase_off[g], "phrase %d is empty", g);
    MGR_REQUIRE(phrase_off[g + 1] <= MGR_LEXICON_MAX_WORDS, "the lexicon has more than %d words", MGR_LEXICON_MAX_WORDS);
    lex->off[g + 1] = (uint8_t)phrase_off[g + 1];
  }
  const int nw = phrase_off[G];
  for (int j = 0; j < nw; ++j) {
    MGR_REQUIRE(phrase_words[j] >= 0 && phrase_words[j] < C && phrase_words[j] != blank, "word %d of the lexicon is %d: not a non-blank class", j,
                phrase_words[j]);
    lex->words[j] = (uint8_t)phrase_words[j];
  }
  return 0;
}

// the lexicon argument into the workgroup's LDS: s_off [MGR_LEXICON_MAX_PHRASES + 1], s_words [MGR_LEXICON_MAX_WORDS + 1] (the caller
// synchronises)
__device__ __forceinline__ void lex_to_lds(const LexArg& lex, int G, int* s_off, int* s_words, int tid, int nthreads) {
  if (G <= 0) return;
  for (int i = tid; i <= G; i += nthreads) s_off[i] = lex.off[i];
  for (int i = tid; i <= MGR_LEXICON_MAX_WORDS; i += nthreads) s_words[i] = lex.words[i];
}

// One slot of an N-best list (hyp [.., Lh] / hyp_len as mgr_ctc_beam_search_lm writes out / out_len), expanded by ONE WAVE into the
// labels the lattice runs over: without a lexicon (G = 0) the entries themselves, clipped into the class range as the loss clips them,
// with one the words of its phrases - sixty-four entries a turn, a prefix sum of the phrase lengths across the wave.  s_lab holds
// cap + 1 labels; what lies behind is counted and not written.  All members are wave-uniform.
struct HypLabels {
  int n;      // the slot's entries (clipped to Lh); < 0: no hypothesis in this slot
  int L;      // the expanded count
  bool bad;   // a phrase id outside [0, G)
};
__device__ __forceinline__ HypLabels hyp_expand(const int32_t* __restrict__ row, int n, int Lh, int G, const int* s_off, const int* s_words,
                                                int C, int* s_lab, int cap, int lane) {
  HypLabels h;
  h.n = n > Lh ? Lh : n;
  h.L = 0;
  h.bad = false;
  for (int base = 0; base < h.n; base += 64) {
    const int i = base + lane;
    int v = i < h.n ? row[i] : 0, len = 0, w0 = 0;
    bool badl = false;
    if (i < h.n) {
      if (G > 0) {
        if (v < 0 || v >= G) badl = true;
        else { w0 = s_off[v]; len = s_off[v + 1] - w0; }
      } else {
        v = clip_label(v, C);   // (as the loss)
        len = 1;
      }
    }
    int x = len;   // inclusive prefix sum of the lengths over the wave
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    const int start = h.L + x - len;
    for (int q = 0; q < len; ++q)
      if (start + q <= cap) s_lab[start + q] = G > 0 ? s_words[w0 + q] : v;
    h.L += __shfl(x, 63);
    h.bad = h.bad || __any(badl ? 1 : 0);
  }
  return h;
}

}  // namespace
