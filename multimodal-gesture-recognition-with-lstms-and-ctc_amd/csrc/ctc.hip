// K6: CTC loss + gradient w.r.t. the Dense logits: three kernels - emissions (a thread per frame), the alpha / beta recursions (two
// waves per sample), gradient (a thread per frame).
//
// Restates K.ctc_batch_cost -> tf.nn.ctc_loss as called by ctc_lambda_func
// (reference multimodal_fusion/losses.py:4-15): y = softmax(log(P[:,skip:]+eps)), blank = C-1,
// log-space alpha/beta DP over l' = [blank,l1,blank,...,lL,blank].
//
// Recursions: one wave runs alpha forward in time, one runs beta backward in time, concurrently.  The
// extended label sequence lives across the lanes of the wave as (blank,label) PAIRS: lane*PPL+j holds
// states 2p (blank) and 2p+1 (label p), so the only cross-lane traffic per time step is one
// shift-by-one of the neighbouring pair's label state; the three-way log-sum-exp is max-shifted fp32.
// Emissions log2 y(t,.) are precomputed (k_ctc_emissions) and software-prefetched a chunk of time
// steps ahead of the recursion, so the serial chain per step is shift -> lse -> add.
// Numerics: alpha and beta are RENORMALISED every 16 time steps (the wave-wide max is subtracted and summed
// into an fp64 scalar), so the stored log-values stay O(10) instead of O(-5000) at T=1900, where an fp32 ulp is
// 5e-4 and would put percent-level noise on the gradient.  The loss adds the fp64 offset back; the gradient
// needs no offsets at all because sum_u alpha(t,u)beta(t,u) = p(l|x) at every t, so each frame's occupancies
// are normalised by their own sum.
// The gradient (k_ctc_grad) combines alpha+beta into per-class occupancies through an LDS row per thread and
// chains through softmax(log(P+eps)) and the network's own softmax to dLogits.
// The lattice's pieces - the base-2 log-sum-exp, the DPP shift and wave maximum, the pairs across the lanes, the chunked emission fetch,
// the alpha step, the renormalisation, the final states - are in ctc_lattice.h, shared with align.hip and rescore.hip; the loops (alpha's
// chunks start at t = 1 with the 3-float row offset; rows stored two steps at a time) and the beta step are this file's.
// Vector-memory instructions of the serial chain (round 4; a wave that is alone with its chain pays 60-130 cycles of issue for
// each): the emissions are stored CLASS-MAJOR, forward in time for alpha and reversed for beta, so that a lane fetches eight
// steps of its label's (and the blank's) emissions with two 16-byte loads instead of 16 four-byte ones, and alpha / beta rows
// are stored two time steps at a time (one 16-byte store per lane and pair of steps): ~1 instead of ~3 per step.
// mgr_ctc_entropy_grad is the same three kernels with a template flag on the last two: the chains also carry the entropy of
// the prefixes into (suffixes out of) every state, the gradient kernel turns them into the gradient of the alignment entropy.
#include "ctc_lattice.h"

namespace {

// row length of the class-major emission copies: T' + the over-read of two chunks + the 3-float offset that puts t = 1 on a
// 16-byte boundary (alpha's chunks start at t = 1, 9, 17, ...)
__host__ __device__ inline size_t ctc_ts(int To) { return ((size_t)To + 24 + 3) / 4 * 4; }
// alpha / beta rows, two time steps per block: element (t, state 2p + e) at  (t >> 1) * 2 S2 + 4 p + 2 (t & 1) + e
__device__ __forceinline__ size_t ab_off(int t, int S2) { return (size_t)(t >> 1) * (2 * S2) + 2 * (t & 1); }

// One sample's three phases as functions (the recurrence kernel runs ONE or TWO samples per workgroup).
// Per-sample state: which sample, its clipped lengths, its slices of the workspace, its labels in the workgroup's LDS.
struct CtcSample {
  int b, Tp, L;
  float *LYTb, *LYRb, *ALb, *BEb;
  int* s_lab;
  float *XAb, *XBb;   // the entropy call's rows: the entropy of the prefixes into / the suffixes out of a state, in ALb / BEb's format
};

// the sample's labels into the workgroup's LDS (clipped into the class range)
__device__ __forceinline__ void ctc_labels(const CtcSample& cs_, int tid, int nthreads, const int32_t* __restrict__ labels, int C, int Lmax) {
  for (int i = tid; i < Lmax; i += nthreads) {
    cs_.s_lab[i] = clip_label((i < cs_.L) ? labels[(size_t)cs_.b * Lmax + i] : -1, C);
  }
}
// ---- phase 0: emissions log2 y(t,c) = log2(P+eps) - log2(sum_c (P+eps)), class-major, forward and reversed in time.  One frame per
// thread: workgroup `blk` of the sample's ceil(To / 256) (workgroup 0 also writes the rows' zero tails)
__device__ __forceinline__ void ctc_phase0(const CtcSample& cs_, int tid, int blk, const float* __restrict__ P, int T, int C, int skip, float eps,
                                           size_t TS) {
  const int b = cs_.b, Tp = cs_.Tp;
  float *LYTb = cs_.LYTb, *LYRb = cs_.LYRb;
  const int t = blk * 256 + tid;
  if (t < Tp) {
    const float* row = P + ((size_t)b * T + skip + t) * C;
    const float ls = frame_log_norm<true>(row, C, eps);
    for (int c = 0; c < C; ++c) {
      const float v = emission_log<true>(row[c] + eps) - ls;   // (base-2 units, as everything the recursions touch)
      LYTb[(size_t)c * TS + t + 3] = v;
      LYRb[(size_t)c * TS + (Tp - 1 - t)] = v;
    }
  }
  if (blk != 0) return;
  // the two-chunks-ahead prefetch of the recursions reads up to 2 CH + 2 = 18 floats behind the last emission of a row (values it
  // never uses): they are zeros, not whatever the workspace held (forward rows: [Tp + 3, Tp + 24), reversed rows: [Tp, Tp + 21);
  // TS >= To + 24 holds both)
  for (int i = tid; i < C * 21; i += 256) {
    const int c = i / 21, k = i % 21;
    LYTb[(size_t)c * TS + Tp + 3 + k] = 0.f;
    LYRb[(size_t)c * TS + Tp + k] = 0.f;
  }
}

// ---- phase 1 (one wave per role): role 0 runs alpha forward in time, role 1 beta backward
// ENT (mgr_ctc_entropy_grad): the alpha wave also carries ha(t, s) = log2 alpha(t, s) - E[log2 p(pi_0..t) | the prefix ends in
// s at t], the entropy of the prefixes into s, the beta wave hb(t, s) = log2 beta(t, s) - E[log2 p(pi_t+1..) | the suffix starts in s at
// t] (like this file's beta, without frame t's own emission).  Both follow the chain rule of the entropy over the log-sum-exp the step
// forms anyway (ent_chain2 / 3), take no emission and stay >= 0 and small: no renormalisation, no offset.  They are stored in rows of
// alpha's format; the gradient kernel forms E[log2 p(pi) | pi passes s at t] as (alpha + beta) - (ha + hb).  The alpha wave writes H,
// the chain rule once more over the two final states.  alpha and beta themselves are computed by the same operations either way.
// rel (the entropy's gradient kernel will read the rows): each wave also carries d, what its recursion's float32 additions have rounded
// away per state, and the rows AL / BE hold (alpha - the step's wave-wide maximum) + d instead of alpha (ent_rows) - at |alpha| = 1600
// alpha's own rounding is 1.2e-4 a step, state by state, and the entropy's gradient multiplies it by a few nats.  rel off: the loss's rows.
template <int PPL, bool ENT>
__device__ __forceinline__ void ctc_phase1(const CtcSample& cs_, int role, int lane, int blank, int Lmax, int S2, size_t TS,
                                           float* __restrict__ loss, float* __restrict__ entropy, bool rel) {
  constexpr int CH = Chunk<PPL>::CH;
  const int b = cs_.b, Tp = cs_.Tp, L = cs_.L;
  float *LYTb = cs_.LYTb, *LYRb = cs_.LYRb, *ALb = cs_.ALb, *BEb = cs_.BEb;
  float *XAb = cs_.XAb, *XBb = cs_.XBb;
  int* s_lab = cs_.s_lab;
  if (role < 2 && Tp > 0) {
    const Pairs<PPL> pr(s_lab, L, blank, lane);
    if (role == 0) {
      float ab[PPL], al[PPL];
      float hb[PPL], hl[PPL];   // the even step of the pair in flight (rows are stored two steps at a time)
      float xb[PPL], xl[PPL], gb[PPL], gl[PPL];   // (ENT) ha beside alpha, and its even step in flight
      float db[PPL], dl[PPL], sb[PPL], sl[PPL];   // (ENT) d, and what goes into alpha's rows (ent_rows)
      const float (&wb)[PPL] = ENT ? sb : ab;     // what is stored: alpha itself without ENT
      const float (&wl)[PPL] = ENT ? sl : al;
#pragma unroll
      for (int j = 0; j < PPL; ++j) {
        int p = lane * PPL + j;
        ab[j] = (p == 0) ? LYTb[(size_t)blank * TS + 3] : kNegInf;
        al[j] = (p == 0 && pr.vl[j]) ? LYTb[(size_t)pr.lab[j] * TS + 3] : kNegInf;
        hb[j] = ab[j];
        hl[j] = al[j];
        if (Tp == 1 && p <= Lmax) *reinterpret_cast<float2*>(ALb + 4 * p) = make_float2(ab[j], al[j]);
        if constexpr (ENT) {   // (one prefix of one frame into a start state: no entropy)
          xb[j] = xl[j] = gb[j] = gl[j] = db[j] = dl[j] = 0.f;
          if (Tp == 1 && p <= Lmax) *reinterpret_cast<float2*>(XAb + 4 * p) = make_float2(0.f, 0.f);
        }
      }
      if constexpr (ENT) {   // (the first row as ent_rows has it)
        ent_rows(rel, ab, al, db, dl, sb, sl);
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
          int p = lane * PPL + j;
          hb[j] = sb[j];
          hl[j] = sl[j];
          if (Tp == 1 && p <= Lmax) *reinterpret_cast<float2*>(ALb + 4 * p) = make_float2(sb[j], sl[j]);
        }
      }
      Chunk<PPL> cur, nxt;   // steps t0 .. t0 + CH - 1, t0 = 1 mod CH: with the rows' 3-float offset 16-byte aligned
      cur.load(LYTb + 3, TS, blank, pr.lab, 1);
      double coff = 0.0;
      int since = 0;
      for (int t0 = 1; t0 < Tp; t0 += CH) {
        nxt.load(LYTb + 3, TS, blank, pr.lab, t0 + CH);
#pragma unroll
        for (int k = 0; k < CH; ++k) {
          int t = t0 + k;
          if (t < Tp) {
            if constexpr (ENT) {
              alpha_step_ent(pr, ab, al, xb, xl, db, dl, cur.eb[k], cur.el[k]);
              ent_rows(rel, ab, al, db, dl, sb, sl);
            } else {
              alpha_step(pr, ab, al, cur.eb[k], cur.el[k]);
            }
#pragma unroll
            for (int j = 0; j < PPL; ++j) {
              int p = lane * PPL + j;
              if (t & 1) {          // the pair (t - 1, t) is complete: one 16-byte store
                if (p <= Lmax) *reinterpret_cast<float4*>(ALb + ab_off(t - 1, S2) + 4 * p) = make_float4(hb[j], hl[j], wb[j], wl[j]);
                if constexpr (ENT)
                  if (p <= Lmax) *reinterpret_cast<float4*>(XAb + ab_off(t - 1, S2) + 4 * p) = make_float4(gb[j], gl[j], xb[j], xl[j]);
              } else {
                hb[j] = wb[j];
                hl[j] = wl[j];
                if (t == Tp - 1 && p <= Lmax) *reinterpret_cast<float2*>(ALb + ab_off(t, S2) + 4 * p) = make_float2(wb[j], wl[j]);
                if constexpr (ENT) {
                  gb[j] = xb[j];
                  gl[j] = xl[j];
                  if (t == Tp - 1 && p <= Lmax) *reinterpret_cast<float2*>(XAb + ab_off(t, S2) + 4 * p) = make_float2(xb[j], xl[j]);
                }
              }
            }
          }
        }
        cur = nxt;
        since += CH;
        if (since >= 16) {  // renormalise: keep the running log-values O(10)
          since = 0;
          if constexpr (ENT) coff += (double)renorm_ent(ab, al, db, dl);
          else coff += (double)renorm(ab, al);
        }
      }
      // log p(l|x) = lse(alpha(2L, Tp-1), alpha(2L-1, Tp-1)) + accumulated offset
      const float2 f = final_states(ab, al, L, lane);
      float lfin = lse2(f.x, f.y);
      if (lane == 0) {
        // (+inf: no alignment fits - what k_ctc_grad reads as "no gradient")
        loss[b] = (lfin == kNegInf) ? __builtin_huge_valf() : (float)(-((double)lfin + coff) * kLn2);
      }
      if constexpr (ENT) {
        // H: the chain rule over the two final states, weighed as lfin weighs their alpha (-inf from final_states: no such state - weight 0)
        const float2 fx = final_states(xb, xl, L, lane), fd = final_states(db, dl, L, lane);
        float m, e0, e1, s, lg;
        lse2_terms(f.x, f.y, m, e0, e1, s, lg);
        const float D = (wsel(e0, fd.x) + wsel(e1, fd.y)) * __builtin_amdgcn_rcpf(s);
        const float h = ent_chain2(m, s, lg, D, e0, fx.x, f.x, fd.x, e1, fx.y, f.y, fd.y);
        if (lane == 0) entropy[b] = (lfin == kNegInf || !(h > 0.f)) ? 0.f : (float)((double)h * kLn2);
      }
    } else {
      float bb[PPL], bl[PPL];
      bool csn[PPL];  // can_skip of pair p+1
      {
        int nfirst = __shfl_down((int)pr.cs[0], 1);
#pragma unroll
        for (int j = 0; j < PPL; ++j) csn[j] = (j < PPL - 1) ? pr.cs[j + 1] : (lane < 63 && nfirst != 0);
      }
      float hb[PPL], hl[PPL];   // the odd step of the pair in flight (beta walks down: t + 1 comes before t)
      float yb[PPL], yl[PPL], gb[PPL], gl[PPL];   // (ENT) hb beside beta, and its odd step in flight
      float qb[PPL], ql[PPL], sb[PPL], sl[PPL];   // (ENT) d, and what goes into beta's rows (ent_rows)
#pragma unroll
      for (int j = 0; j < PPL; ++j) {
        int p = lane * PPL + j;
        bb[j] = (p == L) ? 0.f : kNegInf;
        bl[j] = (p == L - 1) ? 0.f : kNegInf;
        hb[j] = bb[j];
        hl[j] = bl[j];
        // t = Tp - 1: an even t is a pair's first half and nothing pairs with it from above - stored on its own
        if (((Tp - 1) & 1) == 0 && p <= Lmax) *reinterpret_cast<float2*>(BEb + ab_off(Tp - 1, S2) + 4 * p) = make_float2(bb[j], bl[j]);
        if constexpr (ENT) {   // (nothing lies behind the last frame: no entropy)
          yb[j] = yl[j] = gb[j] = gl[j] = qb[j] = ql[j] = 0.f;
          if (((Tp - 1) & 1) == 0 && p <= Lmax) *reinterpret_cast<float2*>(XBb + ab_off(Tp - 1, S2) + 4 * p) = make_float2(0.f, 0.f);
        }
      }
      if constexpr (ENT) {   // (the last row as ent_rows has it)
        ent_rows(rel, bb, bl, qb, ql, sb, sl);
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
          int p = lane * PPL + j;
          hb[j] = sb[j];
          hl[j] = sl[j];
          if (((Tp - 1) & 1) == 0 && p <= Lmax) *reinterpret_cast<float2*>(BEb + ab_off(Tp - 1, S2) + 4 * p) = make_float2(sb[j], sl[j]);
        }
      }
      Chunk<PPL> cur, nxt;
      // step index n = 0.. walks t = Tp-2-n; uses emissions at t+1 = Tp-1-n = reversed index n: a chunk is the reversed steps
      // n0 .. n0 + CH - 1 (n0 = 0 mod CH: aligned)
      cur.load(LYRb, TS, blank, pr.lab, 0);
      const int nsteps = Tp - 1;
      int since = 0;
      for (int n0 = 0; n0 < nsteps; n0 += CH) {
        nxt.load(LYRb, TS, blank, pr.lab, n0 + CH);
#pragma unroll
        for (int k = 0; k < CH; ++k) {
          int n = n0 + k;
          if (n < nsteps) {
            int t = Tp - 2 - n;
            float xb[PPL], xl[PPL];  // beta(.,t+1) + emission(.,t+1)
#pragma unroll
            for (int j = 0; j < PPL; ++j) {
              xb[j] = pr.vb[j] ? bb[j] + cur.eb[k] : kNegInf;
              xl[j] = pr.vl[j] ? bl[j] + cur.el[k][j] : kNegInf;
            }
            const float nxb = dpp_f32<DPP_WAVE_SHL1>(xb[0], kNegInf);   // (lane 63: log 0)
            const float nxl = dpp_f32<DPP_WAVE_SHL1>(xl[0], kNegInf);
            // (ENT) hb(., t + 1) of the next lane's first pair; d(., t + 1) with what beta + emission rounds away (not finite on a dead
            // state: weight 0, selected away), and the next lane's first pair's
            float nyb = 0.f, nyl = 0.f, zb[PPL], zl[PPL], nzb = 0.f, nzl = 0.f;
            if constexpr (ENT) {
              nyb = dpp_f32<DPP_WAVE_SHL1>(yb[0], 0.f);
              nyl = dpp_f32<DPP_WAVE_SHL1>(yl[0], 0.f);
#pragma unroll
              for (int j = 0; j < PPL; ++j) {
                zb[j] = qb[j] + add_err(bb[j], cur.eb[k], xb[j]);
                zl[j] = ql[j] + add_err(bl[j], cur.el[k][j], xl[j]);
              }
              nzb = dpp_f32<DPP_WAVE_SHL1>(zb[0], 0.f);
              nzl = dpp_f32<DPP_WAVE_SHL1>(zl[0], 0.f);
            }
#pragma unroll
            for (int j = 0; j < PPL; ++j) {
              float b1 = (j < PPL - 1) ? xb[j + 1] : nxb;  // blank of pair p+1 (state u+1 for the label state)
              float l1 = (j < PPL - 1) ? xl[j + 1] : nxl;  // label of pair p+1 (state u+2)
              if constexpr (ENT) {   // (lse2 / lse3 with their terms handed out: the same bits)
                const float yb1 = (j < PPL - 1) ? yb[j + 1] : nyb, yl1 = (j < PPL - 1) ? yl[j + 1] : nyl;   // (pair j + 1 is updated after pair j)
                const float zb1 = (j < PPL - 1) ? zb[j + 1] : nzb, zl1 = (j < PPL - 1) ? zl[j + 1] : nzl;
                const float l2 = csn[j] ? l1 : kNegInf;
                float m, e0, e1, e2, s, lg;
                const float vb = lse2_terms(xb[j], xl[j], m, e0, e1, s, lg);
                bb[j] = pr.vb[j] ? vb : kNegInf;
                const float Db = (wsel(e0, zb[j]) + wsel(e1, zl[j])) * __builtin_amdgcn_rcpf(s);
                const float nyb_j = (bb[j] == kNegInf) ? 0.f : ent_chain2(m, s, lg, Db, e0, yb[j], xb[j], zb[j], e1, yl[j], xl[j], zl[j]);
                qb[j] = (bb[j] == kNegInf) ? 0.f : Db + add_err(m, lg, vb);
                const float vl = lse3_terms(xl[j], b1, l2, m, e0, e1, e2, s, lg);
                bl[j] = pr.vl[j] ? vl : kNegInf;
                const float Dl = (wsel(e0, zl[j]) + wsel(e1, zb1) + wsel(e2, zl1)) * __builtin_amdgcn_rcpf(s);
                yl[j] = (bl[j] == kNegInf) ? 0.f : ent_chain3(m, s, lg, Dl, e0, yl[j], xl[j], zl[j], e1, yb1, b1, zb1, e2, yl1, l2, zl1);
                ql[j] = (bl[j] == kNegInf) ? 0.f : Dl + add_err(m, lg, vl);
                yb[j] = nyb_j;
              } else {
                bb[j] = pr.vb[j] ? lse2(xb[j], xl[j]) : kNegInf;
                bl[j] = pr.vl[j] ? lse3(xl[j], b1, csn[j] ? l1 : kNegInf) : kNegInf;
              }
              if constexpr (!ENT) {
                int p = lane * PPL + j;
                if (t & 1) {          // first half of the pair (t - 1, t) to arrive: keep it (or store it alone at t = ... never: t >= 0 even ends)
                  hb[j] = bb[j];
                  hl[j] = bl[j];
                } else {              // the pair (t, t + 1) is complete (t + 1 was held, or is the initial row when Tp - 1 is odd)
                  if (p <= Lmax) *reinterpret_cast<float4*>(BEb + ab_off(t, S2) + 4 * p) = make_float4(bb[j], bl[j], hb[j], hl[j]);
                }
              }
            }
            if constexpr (ENT) {   // (the same stores, of what ent_rows makes of the step's whole row)
              ent_rows(rel, bb, bl, qb, ql, sb, sl);
#pragma unroll
              for (int j = 0; j < PPL; ++j) {
                int p = lane * PPL + j;
                if (t & 1) {
                  hb[j] = sb[j];
                  hl[j] = sl[j];
                  gb[j] = yb[j];
                  gl[j] = yl[j];
                } else if (p <= Lmax) {
                  *reinterpret_cast<float4*>(BEb + ab_off(t, S2) + 4 * p) = make_float4(sb[j], sl[j], hb[j], hl[j]);
                  *reinterpret_cast<float4*>(XBb + ab_off(t, S2) + 4 * p) = make_float4(yb[j], yl[j], gb[j], gl[j]);
                }
              }
            }
          }
        }
        cur = nxt;
        since += CH;
        if (since >= 16) {
          since = 0;
          if constexpr (ENT) renorm_ent(bb, bl, qb, ql);
          else renorm(bb, bl);   // (no offset kept: the gradient normalises every frame by its own sum)
        }
      }
    }
  }
}

// ---- phase 2 (one frame per thread): gradient w.r.t. the Dense logits
__device__ __forceinline__ void ctc_phase2(const CtcSample& cs_, int tid, int blk, float* smem, const float* __restrict__ P, int T, int C, int skip,
                                           int blank, float eps, float gscale, int S2, bool dead, float* __restrict__ dLogits) {
  const int b = cs_.b, Tp = cs_.Tp, L = cs_.L;
  float *ALb = cs_.ALb, *BEb = cs_.BEb;
  int* s_lab = cs_.s_lab;
  float* occ = smem + (size_t)tid * (C + 1);
  const int f = blk * 256 + tid;
  if (f >= T) return;
  float* out = dLogits + ((size_t)b * T + f) * C;
  const int tt = f - skip;
  if (tt < 0 || tt >= Tp || dead) {   // (dead: p(l|x) = 0 - no alignment fits - or no frames at all: the loss is +inf, the gradient zero)
    for (int c = 0; c < C; ++c) out[c] = 0.f;
    return;
  }
  for (int c = 0; c < C; ++c) occ[c] = 0.f;
  const float* ar = ALb + ab_off(tt, S2);
  const float* br = BEb + ab_off(tt, S2);
  float vmax = kNegInf;
  for (int p = 0; p <= L; ++p) {
    float2 a = *reinterpret_cast<const float2*>(ar + 4 * p);
    float2 be = *reinterpret_cast<const float2*>(br + 4 * p);
    vmax = fmaxf(vmax, a.x + be.x);
    if (p < L) vmax = fmaxf(vmax, a.y + be.y);
  }
  float den = 0.f;
  for (int p = 0; p <= L; ++p) {
    float2 a = *reinterpret_cast<const float2*>(ar + 4 * p);
    float2 be = *reinterpret_cast<const float2*>(br + 4 * p);
    float wb = exp2_raw(a.x + be.x - vmax);
    occ[blank] += wb;
    den += wb;
    if (p < L) {
      float wl = exp2_raw(a.y + be.y - vmax);
      occ[s_lab[p]] += wl;
      den += wl;
    }
  }
  const float iden = 1.f / den;  // sum_u alpha*beta = p(l|x) for every t: normalise by the frame's own sum
  const float* row = P + ((size_t)b * T + f) * C;
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += row[c] + eps;
  float inv = 1.f / s;
  float dot = 0.f;
  for (int c = 0; c < C; ++c) {
    float u = row[c] + eps;
    float gp = (u * inv - occ[c] * iden) / u;
    occ[c] = gp;
    dot += row[c] * gp;
  }
  for (int c = 0; c < C; ++c) out[c] = row[c] * (occ[c] - dot) * gscale;
}

// ---- phase 2 of mgr_ctc_entropy_grad (one frame per thread): loss_scale * dloss/dlogits - ent_scale * dH/dlogits.  With
// c(t, s) = E[log2 p(pi) | pi passes s at t] and gamma the frame's normalised occupancies, dH/du(t, k) = -ln 2 (sum_{s: l'_s = k} gamma c
// - gamma_k m_t), m_t = sum_s gamma c: a row that sums to zero over k, put where the loss puts y_k - gamma_k.  Only c - m_t enters, so c
// is taken up to a constant of the frame: c(t, s) = (log2 alpha + log2 beta)(t, s) - (ha + hb)(t, s) (this file's beta leaves frame t's
// emission out, so nothing is subtracted; ha, hb: the chains' rows, the prefixes' and suffixes' entropy), and the first bracket is
// log2 gamma(t, s) up to such a constant - the exponent the occupancy is formed from.  occ / gc: the thread's two LDS rows.
__device__ __forceinline__ void ctc_phase2_ent(const CtcSample& cs_, int f, float* occ, float* gc, const float* __restrict__ P, int T, int C,
                                               int skip, int blank, float eps, float lscale, float escale, int S2, bool dead,
                                               float* __restrict__ dLogits) {
  const int b = cs_.b, Tp = cs_.Tp, L = cs_.L;
  const int* s_lab = cs_.s_lab;
  if (f >= T) return;
  float* out = dLogits + ((size_t)b * T + f) * C;
  const int tt = f - skip;
  if (tt < 0 || tt >= Tp || dead) {
    for (int c = 0; c < C; ++c) out[c] = 0.f;
    return;
  }
  for (int c = 0; c < C; ++c) occ[c] = gc[c] = 0.f;
  const float* ar = cs_.ALb + ab_off(tt, S2);
  const float* br = cs_.BEb + ab_off(tt, S2);
  const float* xar = cs_.XAb + ab_off(tt, S2);
  const float* xbr = cs_.XBb + ab_off(tt, S2);
  // (log2 alpha + log2 beta is summed in fp64 here: at |alpha| = 1600 the float32 sum alone rounds at 2.4e-4, state by state, and that
  // rounding is multiplied by |c - m_t| in what follows)
  double vmax = -__builtin_huge_val();
  int iref = 0;   // the frame's most probable state: c is taken relative to ITS c, which is then exactly 0 (peaked posteriors: gamma = 1
                  // - 1e-4 there, and sum gamma c - gamma_k m_t would cancel to its last digits otherwise)
  for (int p = 0; p <= L; ++p) {
    const float2 a = *reinterpret_cast<const float2*>(ar + 4 * p), be = *reinterpret_cast<const float2*>(br + 4 * p);
    if ((double)a.x + (double)be.x > vmax) {
      vmax = (double)a.x + (double)be.x;
      iref = 4 * p;
    }
    if (p < L && (double)a.y + (double)be.y > vmax) {
      vmax = (double)a.y + (double)be.y;
      iref = 4 * p + 1;
    }
  }
  const float kref = xar[iref] + xbr[iref];
  float den = 0.f, msum = 0.f;
  for (int p = 0; p <= L; ++p) {
    const float2 a = *reinterpret_cast<const float2*>(ar + 4 * p), be = *reinterpret_cast<const float2*>(br + 4 * p);
    const float2 xa = *reinterpret_cast<const float2*>(xar + 4 * p), xb = *reinterpret_cast<const float2*>(xbr + 4 * p);
    const float vb = (float)(((double)a.x + (double)be.x) - vmax);
    const float wb = exp2_raw(vb);
    const float cb = wb > 0.f ? wb * (vb - ((xa.x + xb.x) - kref)) : 0.f;   // (a dead state: weight 0 and exponent -inf - left out by selection)
    occ[blank] += wb;
    gc[blank] += cb;
    den += wb;
    msum += cb;
    if (p < L) {
      const float vl = (float)(((double)a.y + (double)be.y) - vmax);
      const float wl = exp2_raw(vl);
      const float cl = wl > 0.f ? wl * (vl - ((xa.y + xb.y) - kref)) : 0.f;
      occ[s_lab[p]] += wl;
      gc[s_lab[p]] += cl;
      den += wl;
      msum += cl;
    }
  }
  const float iden = 1.f / den;
  const float mt = msum * iden;
  const float* row = P + ((size_t)b * T + f) * C;
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += row[c] + eps;
  const float inv = 1.f / s;
  // P_c (gp_c - sum_j P_j gp_j) as the loss forms it, with gp taken relative to its value g0 at the frame's most probable class (sum_j
  // P_j = 1): saturated posteriors have P = 1 there, and gp_c - dot would cancel to its last digits on that class
  int cmax = 0;
  for (int c = 0; c < C; ++c) {
    const float u = row[c] + eps;
    const float g = occ[c] * iden;
    const float r = -(float)kLn2 * (gc[c] * iden - g * mt);   // dH/du(t, c), nats
    occ[c] = (lscale * (u * inv - g) - escale * r) / u;
    if (row[c] > row[cmax]) cmax = c;
  }
  const float g0 = occ[cmax];
  float dot = 0.f;
  for (int c = 0; c < C; ++c) dot += row[c] * (occ[c] - g0);
  for (int c = 0; c < C; ++c) out[c] = row[c] * ((occ[c] - g0) - dot);
}

// One sample's slices of the workspace and its clipped lengths.  s_lab: the sample's label row in the workgroup's LDS (or null).
__device__ __forceinline__ CtcSample ctc_sample(int b, int B, const int32_t* __restrict__ input_len, const int32_t* __restrict__ label_len, int To,
                                                int C, int Lmax, float* LY, float* AL, float* BE, int* s_lab) {
  CtcSample s_;
  s_.b = b < B ? b : -1;
  const int bc = b < B ? b : B - 1;
  const int S2 = 2 * (Lmax + 1);
  const size_t TS = ctc_ts(To);
  int Tp = input_len[bc];
  s_.Tp = Tp < 0 ? 0 : (Tp > To ? To : Tp);
  int L = label_len[bc];
  s_.L = L < 0 ? 0 : (L > Lmax ? Lmax : L);
  s_.LYTb = LY + (size_t)bc * 2 * C * TS;           // [C][TS]: y(t, c) at c * TS + t + 3
  s_.LYRb = s_.LYTb + (size_t)C * TS;               // [C][TS]: y(Tp - 1 - r, c) at c * TS + r
  s_.ALb = AL + (size_t)bc * (To + 1) * S2;
  s_.BEb = BE + (size_t)bc * (To + 1) * S2;
  s_.s_lab = s_lab;
  s_.XAb = s_.XBb = nullptr;
  return s_;
}
// ... and its slices of the entropy call's two extra rows (XA, XB: [B][To + 1][S2] each, as AL and BE)
__device__ __forceinline__ void ctc_sample_ent(CtcSample& s_, int B, int To, int Lmax, float* XA, float* XB) {
  const int bc = s_.b >= 0 ? s_.b : B - 1;
  const size_t rows = (size_t)bc * (To + 1) * (2 * (Lmax + 1));
  s_.XAb = XA + rows;
  s_.XBb = XB + rows;
}

// Three kernels (round 6; one kernel with three phases before): the emissions and the gradient are one independent piece of work per
// FRAME - 121,600 of them at config F's shape - and ran on the 256 threads of the workgroup that owns the sample's two chains, one sample
// after the other: 0.09 + 0.20 ms of the kernel's 0.56, for microseconds of work once every frame has a thread of its own.
//
// k_ctc_emissions: grid (ceil(To / 256), B) - phase 0.
__global__ __launch_bounds__(256) void k_ctc_emissions(const float* __restrict__ P, const int32_t* __restrict__ input_len,
                                                       const int32_t* __restrict__ label_len, int B, int T, int C, int Lmax, int skip, float eps,
                                                       float* __restrict__ LY, float* __restrict__ AL, float* __restrict__ BE) {
  const CtcSample s_ = ctc_sample((int)blockIdx.y, B, input_len, label_len, T - skip, C, Lmax, LY, AL, BE, nullptr);
  ctc_phase0(s_, threadIdx.x, (int)blockIdx.x, P, T, C, skip, eps, ctc_ts(T - skip));
}

// k_ctc_chains - phase 1.  SPW = samples per workgroup.  1: wave 0 = alpha, wave 1 = beta of the workgroup's sample (128 threads).  2: waves
// 0, 1 run the chains of sample 2 j, waves 2, 3 those of sample 2 j + 1 - one chain per SIMD.  In the training step the kernel runs on
// the 48 CUs the fused encoder scans leave: 64 one-sample workgroups there put two on 16 CUs, whose alpha (beta) waves then SHARE a SIMD,
// and every chain of the launch waits for those (0.97 ms in the step for 0.55 alone); 32 two-sample workgroups have a CU each.
// ENT: the chains of mgr_ctc_entropy_grad (ctc_phase1) - entropy [B] and the rows XA, XB are read and written only then.
template <int PPL, int SPW, bool ENT>
__global__ __launch_bounds__(128 * SPW) void k_ctc_chains(const int32_t* __restrict__ labels, const int32_t* __restrict__ input_len,
                                                          const int32_t* __restrict__ label_len, int B, int T, int C, int Lmax, int skip, int blank,
                                                          float* __restrict__ loss, float* __restrict__ LY, float* __restrict__ AL,
                                                          float* __restrict__ BE, float* __restrict__ entropy, float* __restrict__ XA,
                                                          float* __restrict__ XB, int rel) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // SPW label rows
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int To = T - skip;
  const int S2 = 2 * (Lmax + 1);
  const size_t TS = ctc_ts(To);
  auto sample = [&](int si) {
    CtcSample s_ = ctc_sample((int)blockIdx.x * SPW + si, B, input_len, label_len, To, C, Lmax, LY, AL, BE,
                              reinterpret_cast<int*>(smem) + si * (Lmax + 1));
    if constexpr (ENT) ctc_sample_ent(s_, B, To, Lmax, XA, XB);
    return s_;
  };
  {
    const CtcSample s_ = sample(wave >> 1);
    if (s_.b >= 0) ctc_labels(s_, tid & 127, 128, labels, C, Lmax);
  }
  __syncthreads();
  {
    const CtcSample s_ = sample(wave >> 1);
    if (s_.b >= 0) ctc_phase1<PPL, ENT>(s_, wave & 1, lane, blank, Lmax, S2, TS, loss, entropy, rel != 0);
    if (s_.b >= 0 && s_.Tp == 0 && (tid & 127) == 0) {
      loss[s_.b] = __builtin_huge_valf();
      if constexpr (ENT) entropy[s_.b] = 0.f;
    }
  }
}

// k_ctc_grad: grid (ceil(T / 256), B) - phase 2.
// ENT (mgr_ctc_entropy_grad): grid (ceil(T / FT), B) of FT = blockDim.x threads, a SECOND LDS row per thread for sum gamma c per class;
// gscale is the loss's scale, escale the entropy's.
template <bool ENT>
__global__ __launch_bounds__(256) void k_ctc_grad(const float* __restrict__ P, const int32_t* __restrict__ labels,
                                                  const int32_t* __restrict__ input_len, const int32_t* __restrict__ label_len, int B, int T, int C,
                                                  int Lmax, int skip, int blank, float eps, float gscale, const float* __restrict__ loss,
                                                  float* __restrict__ dLogits, float* __restrict__ LY, float* __restrict__ AL,
                                                  float* __restrict__ BE, float escale, float* __restrict__ XA, float* __restrict__ XB) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [256][C+1] occupancy rows, then the label row
  if constexpr (ENT) {   // [FT][C+1] occupancy rows, [FT][C+1] rows of sum gamma c, then the label row
    const int FT = (int)blockDim.x, tid = (int)threadIdx.x;
    CtcSample s_ = ctc_sample((int)blockIdx.y, B, input_len, label_len, T - skip, C, Lmax, LY, AL, BE,
                              reinterpret_cast<int*>(smem + (size_t)2 * FT * (C + 1)));
    ctc_sample_ent(s_, B, T - skip, Lmax, XA, XB);
    ctc_labels(s_, tid, FT, labels, C, Lmax);
    __syncthreads();
    const bool dead = loss[s_.b] == __builtin_huge_valf();
    ctc_phase2_ent(s_, (int)blockIdx.x * FT + tid, smem + (size_t)tid * (C + 1), smem + (size_t)(FT + tid) * (C + 1), P, T, C, skip, blank, eps,
                   gscale, escale, 2 * (Lmax + 1), dead, dLogits);
    return;
  }
  const CtcSample s_ = ctc_sample((int)blockIdx.y, B, input_len, label_len, T - skip, C, Lmax, LY, AL, BE,
                                  reinterpret_cast<int*>(smem + 256 * (C + 1)));
  ctc_labels(s_, threadIdx.x, 256, labels, C, Lmax);
  __syncthreads();
  const bool dead = loss[s_.b] == __builtin_huge_valf();
  ctc_phase2(s_, threadIdx.x, (int)blockIdx.x, smem, P, T, C, skip, blank, eps, gscale, 2 * (Lmax + 1), dead, dLogits);
}

// ---- K17: state posteriors and quantile extents.  gamma(t, s) = alpha(t, s) beta(t, s) / sum_s', from the loss's own chains.
//
// k_ctc_occupancy: one workgroup per sample, looping over tiles of FT frames (FT = 256, 128 or 64: what fits the LDS), three phases a tile:
//   fill   the tile's alpha and beta rows are ONE contiguous stretch of the workspace each (rows lie two time steps a block): all 256
//          threads read it front to back with 8-byte loads and put log2 alpha + log2 beta into an LDS row per FRAME of odd length
//          2 (Lmax + 1) + 1, so that the walk below - a thread per frame, every lane at the same state - meets no bank twice; the
//          frames' posteriors P go into a second tile (odd row length again) for conf;
//   walk   a thread per frame: the row's maximum, the weights 2^(x - max) and their sum in ascending state order (k_ctc_grad's order),
//          then from the last state down gamma = w * (1 / sum) and the running sum cum - one rounded multiplication and one rounded
//          addition per state, never a fused one: seg is a function of the float32 gamma alone, which a sequential float32 sum on the
//          host restates bit for bit.  gamma >= 0, so its sign bit carries the state's flag to the next phase: for a label state
//          2i + 1 "cum >= q" (label i has begun), for the blank behind it 2i + 2 "cum <= 1 - q" (label i has not ended);
//   labels a thread per label, over the tile's frames in ascending order: the first frame with the label state's flag, the last with the
//          blank's, the sums of gamma and gamma * P[t, l_i] - no atomics, one fixed order.
// gamma leaves the tile with contiguous stores.  Nothing here depends on whether gamma is asked for but those stores.
constexpr int kOccLdsMax = 160 * 1024;
__host__ __device__ inline int occ_row(int Lmax) { return 2 * (Lmax + 1) + 1; }
static size_t occ_lds_bytes(int ft, int C, int Lmax) { return ((size_t)ft * (occ_row(Lmax) + (C | 1)) + (Lmax + 1)) * sizeof(float); }
static int occ_frame_tile(int C, int Lmax) {
  for (int ft = 256; ft >= 64; ft >>= 1)
    if (occ_lds_bytes(ft, C, Lmax) <= (size_t)kOccLdsMax) return ft;
  return 0;
}

// logp = -loss, the loss's float widened
__global__ __launch_bounds__(256) void k_occ_logp(const float* __restrict__ loss, int B, double* __restrict__ logp) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) logp[b] = -(double)loss[b];
}

__global__ __launch_bounds__(256) void k_ctc_occupancy(const float* __restrict__ P, const int32_t* __restrict__ labels,
                                                       const int32_t* __restrict__ input_len, const int32_t* __restrict__ label_len, int B, int T,
                                                       int C, int Lmax, int skip, int FT, float q, const double* __restrict__ logp,
                                                       float* __restrict__ gamma, int32_t* __restrict__ seg, float* __restrict__ occ,
                                                       float* __restrict__ conf, float* LY, float* AL, float* BE) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [FT][RS] alpha + beta -> weights -> gamma | [FT][Cp] P | the label row
  const int tid = threadIdx.x, b = blockIdx.x;
  const int To = T - skip, S2 = 2 * (Lmax + 1), RS = occ_row(Lmax), Cp = C | 1, S = 2 * Lmax + 1;
  float* tile = smem;
  float* ptile = tile + (size_t)FT * RS;
  const CtcSample s_ = ctc_sample(b, B, input_len, label_len, To, C, Lmax, LY, AL, BE, reinterpret_cast<int*>(ptile + (size_t)FT * Cp));
  ctc_labels(s_, tid, 256, labels, C, Lmax);
  const bool dead = !(logp[b] > -__builtin_huge_val());   // (no alignment fits, or no frames at all)
  const int Tp = dead ? 0 : s_.Tp, L = s_.L;
  const float omq = 1.0f - q;
  int first = -1, last = -1;    // of label `tid`, in frames of P[:, skip:]
  float so = 0.f, sc = 0.f;
  for (int t0 = 0; t0 < To; t0 += FT) {
    const int nf = Tp - t0 < 0 ? 0 : (Tp - t0 > FT ? FT : Tp - t0);
    __syncthreads();   // (the labels; the tile's readers of the round before)
    if (nf > 0) {
      // frames t0 .. t0 + nf - 1 (t0 is even): blocks t0 / 2 .. of two rows each, S2 float2 a block - (p, step) at float2 2 p + step
      const float2* a2 = reinterpret_cast<const float2*>(s_.ALb + (size_t)t0 * S2);
      const float2* b2 = reinterpret_cast<const float2*>(s_.BEb + (size_t)t0 * S2);
      const int n2 = ((nf + 1) >> 1) * S2;   // (an odd nf reads the half block behind it - inside the sample's rows - into a row nobody walks)
      for (int i = tid; i < n2; i += 256) {
        const int blk = i / S2, r = i - blk * S2;
        const float2 a = a2[i], be = b2[i];
        float* d = tile + (size_t)(2 * blk + (r & 1)) * RS + (r >> 1) * 2;
        d[0] = a.x + be.x;
        d[1] = a.y + be.y;
      }
      const float* prow = P + ((size_t)b * T + skip + t0) * C;
      for (int i = tid; i < nf * C; i += 256) {
        const int f = i / C;
        ptile[(size_t)f * Cp + (i - f * C)] = prow[i];
      }
    }
    __syncthreads();
    if (tid < nf) {
      float* row = tile + (size_t)tid * RS;
      const int ns = 2 * L + 1;
      // (each pass takes eight states at a time, the LDS reads first: a wave that is alone on its SIMD has nothing else to hide their
      // latency behind.  The order of every sum is that of the plain loops.)
      float vmax = kNegInf;
      int s = 0;
      for (; s + 8 <= ns; s += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = row[s + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) vmax = fmaxf(vmax, v[k]);
      }
      for (; s < ns; ++s) vmax = fmaxf(vmax, row[s]);
      float den = 0.f;
      for (s = 0; s + 8 <= ns; s += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = exp2_raw(row[s + k] - vmax);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          row[s + k] = v[k];
          den += v[k];
        }
      }
      for (; s < ns; ++s) {
        const float w = exp2_raw(row[s] - vmax);
        row[s] = w;
        den += w;
      }
      const float iden = 1.f / den;   // sum_s alpha beta = p(l|x) at every t: each frame is normalised by its own sum
      float cum = 0.f;
      auto state = [&](int st, float w) {
        const float g = __fmul_rn(w, iden);
        cum = __fadd_rn(cum, g);
        const bool flag = (st & 1) ? (cum >= q) : (st >= 2 && cum <= omq);
        return flag ? __uint_as_float(__float_as_uint(g) | 0x80000000u) : g;
      };
      for (s = ns - 1; s >= 7; s -= 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = row[s - k];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = state(s - k, v[k]);
#pragma unroll
        for (int k = 0; k < 8; ++k) row[s - k] = v[k];
      }
      for (; s >= 0; --s) row[s] = state(s, row[s]);
    }
    __syncthreads();
    if (tid < L) {
      const int lab = s_.s_lab[tid];
      auto frame = [&](int f, float v, float u, float pl) {
        if ((__float_as_uint(v) >> 31) && first < 0) first = t0 + f;
        if (__float_as_uint(u) >> 31) last = t0 + f;
        const float g = fabsf(v);
        so += g;
        sc += g * pl;
      };
      const float* col = tile + 2 * tid + 1;
      int f = 0;
      for (; f + 4 <= nf; f += 4) {
        float v[4], u[4], pl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[k] = col[(size_t)(f + k) * RS];
          u[k] = col[(size_t)(f + k) * RS + 1];
          pl[k] = ptile[(size_t)(f + k) * Cp + lab];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) frame(f + k, v[k], u[k], pl[k]);
      }
      for (; f < nf; ++f) frame(f, col[(size_t)f * RS], col[(size_t)f * RS + 1], ptile[(size_t)f * Cp + lab]);
    }
    if (gamma) {
      const int nfa = To - t0 > FT ? FT : To - t0;
      float* out = gamma + ((size_t)b * To + t0) * S;
      for (int i = tid; i < nfa * S; i += 256) {
        const int f = i / S, s = i - f * S;
        out[i] = (f < nf && s <= 2 * L) ? fabsf(tile[(size_t)f * RS + s]) : 0.f;
      }
    }
  }
  if (tid < Lmax) {
    const bool ok = tid < L && Tp > 0;
    const size_t o = (size_t)b * Lmax + tid;
    seg[2 * o] = (ok && first >= 0) ? first + skip : -1;
    seg[2 * o + 1] = (ok && last >= 0) ? last + skip : -1;
    occ[o] = ok ? so : 0.f;
    conf[o] = (ok && so > 0.f) ? sc / so : 0.f;
  }
}

}  // namespace

extern "C" {

// class-major emissions (forward + reversed) | alpha | beta; sized with T (>= T - skip) to keep the query simple
struct CtcWs { float *LY, *AL, *BE; size_t bytes; };
static CtcWs ctc_ws_layout(void* ws, int B, size_t To, int C, int Lmax) {
  mgr_ws_carver w(ws);
  const size_t ab = (size_t)B * (To + 1) * 2 * (Lmax + 1);
  return {w.take<float>((size_t)B * 2 * C * ctc_ts((int)To)), w.take<float>(ab), w.take<float>(ab), w.off};
}
size_t mgr_ctc_ws_bytes(int B, int T, int C, int Lmax) { return ctc_ws_layout(nullptr, B, (size_t)(T > 0 ? T : 1), C, Lmax).bytes; }

// The argument checks the loss and the occupancies share.
static int ctc_check_args(mgr_ctx* c, const float* P, const int32_t* labels, const int32_t* input_len, const int32_t* label_len, int B, int T, int C,
                          int Lmax, int skip, int blank, void* ws, size_t ws_bytes) {
  MGR_REQUIRE(c && P && labels && input_len && label_len, "null argument");
  mgr_planes_forget_range(c, ws, ws_bytes);   // (this call writes its workspace: kept weight planes in it are gone)
  MGR_REQUIRE(B > 0 && T > skip && skip >= 0 && C > 1 && Lmax > 0, "bad shape B=%d T=%d C=%d Lmax=%d skip=%d", B, T, C, Lmax, skip);
  MGR_REQUIRE(blank >= 0 && blank < C, "blank %d out of range", blank);
  MGR_REQUIRE(Lmax + 1 <= 256, "Lmax %d too large (max 255)", Lmax);
  MGR_REQUIRE(ws && ws_bytes >= mgr_ctc_ws_bytes(B, T, C, Lmax), "workspace too small");
  return 0;
}

// The emissions and the two chains of every sample: what mgr_ctc_loss_grad and mgr_ctc_occupancy both start with (the caller has opened
// the profile family).  frame_kib > 0: the LDS the emission kernel asks for, see below.
// The rows the entropy call adds to the loss's workspace: E[log2 p(prefix)] beside alpha, E[log2 p(suffix)] beside beta, in their row
// format.  They are carved from the SECOND half of a workspace of 2 * mgr_ctc_ws_bytes (which holds two such rows and the emissions):
// the first half is ctc_ws_layout's, untouched.
struct CtcEntWs { float *XA, *XB; size_t bytes; };
static CtcEntWs ctc_ent_ws_layout(void* ws, int B, size_t To, int C, int Lmax) {
  mgr_ws_carver w(ws, ctc_ws_layout(nullptr, B, To, C, Lmax).bytes);
  const size_t ab = (size_t)B * (To + 1) * 2 * (Lmax + 1);
  return {w.take<float>(ab), w.take<float>(ab), w.off};
}

// ent: null for the loss's own chains; the entropy call's rows, with `entropy` [B] for H.
static int ctc_launch_chains(mgr_ctx* c, const float* P, const int32_t* labels, const int32_t* input_len, const int32_t* label_len, int B, int T,
                             int C, int Lmax, int skip, int blank, float eps, float* loss, const CtcWs& L, const CtcEntWs* ent = nullptr,
                             float* entropy = nullptr, int rel = 0) {
  const size_t To = (size_t)T;
  float *LY = L.LY, *AL = L.AL, *BE = L.BE;
  // two samples per workgroup (one chain per SIMD) from B = 2 on; MGR_TUNE_CTC_ONE_SAMPLE = 1: one sample per workgroup (rounds 1 - 5)
  const int spw = (B >= 2 && c->tune[MGR_TUNE_CTC_ONE_SAMPLE] == 0) ? 2 : 1;
  size_t lds_chains = (size_t)spw * (Lmax + 1) * sizeof(int) + 16, lds_emis = 0;
  // KiB of LDS the recurrence / the per-frame kernels ask for at least.  Placement: a workgroup that asks for more than a persistent
  // scan workgroup leaves on its CU can only land on a CU without one (the engine sets them for the steps of its fused schedule,
  // where this call runs beside 208 whole-CU scan workgroups: 96 KiB = the 32 recurrence workgroups on a CU each)
  const int chain_kib = c->tune[MGR_TUNE_CTC_CHAIN_LDS_KIB], frame_kib = c->tune[MGR_TUNE_CTC_FRAME_LDS_KIB];
  if (chain_kib > 0 && lds_chains < (size_t)chain_kib * 1024) lds_chains = (size_t)chain_kib * 1024;
  if (frame_kib > 0) lds_emis = (size_t)frame_kib * 1024;
  if (!(c->attr_done & MGR_ATTR_CTC)) {
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_emissions), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_grad<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_occupancy), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<1, 1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<1, 2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<2, 1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<2, 2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<3, 1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<3, 2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<4, 1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<4, 2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    c->attr_done |= MGR_ATTR_CTC;
  }
  if (ent && !(c->attr_done & MGR_ATTR_CTC_ENT)) {
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_grad<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<1, 1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<1, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<2, 1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<2, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<3, 1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<3, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<4, 1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_chains<4, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    c->attr_done |= MGR_ATTR_CTC_ENT;
  }
  float *XA = ent ? ent->XA : nullptr, *XB = ent ? ent->XB : nullptr;
  int npairs = Lmax + 1;
  int ppl = (npairs + 63) / 64;
  hipStream_t s = mgr_stream(c);
  hipLaunchKernelGGL(k_ctc_emissions, dim3((unsigned)((To + 255) / 256), B), dim3(256), lds_emis, s, P, input_len, label_len, B, T, C, Lmax, skip, eps, LY, AL, BE);
#define MGR_CTC_LAUNCH_E(N, E)                                                                                                         \
  do {                                                                                                                                 \
    if (spw == 2)                                                                                                                      \
      hipLaunchKernelGGL((k_ctc_chains<N, 2, E>), dim3((B + 1) / 2), dim3(256), lds_chains, s, labels, input_len, label_len, B, T, C,  \
                         Lmax, skip, blank, loss, LY, AL, BE, entropy, XA, XB, rel);                                                   \
    else                                                                                                                               \
      hipLaunchKernelGGL((k_ctc_chains<N, 1, E>), dim3(B), dim3(128), lds_chains, s, labels, input_len, label_len, B, T, C, Lmax,      \
                         skip, blank, loss, LY, AL, BE, entropy, XA, XB, rel);                                                         \
  } while (0)
#define MGR_CTC_LAUNCH(N)                \
  do {                                   \
    if (ent) MGR_CTC_LAUNCH_E(N, true);  \
    else MGR_CTC_LAUNCH_E(N, false);     \
  } while (0)
  switch (ppl) {
    case 1: MGR_CTC_LAUNCH(1); break;
    case 2: MGR_CTC_LAUNCH(2); break;
    case 3: MGR_CTC_LAUNCH(3); break;
    default: MGR_CTC_LAUNCH(4); break;
  }
#undef MGR_CTC_LAUNCH
#undef MGR_CTC_LAUNCH_E
  return 0;
}

int mgr_ctc_loss_grad(mgr_ctx* c, const float* P, const int32_t* labels, const int32_t* input_len,
                      const int32_t* label_len, int B, int T, int C, int Lmax, int skip, int blank, float eps,
                      float gscale, float* loss, float* dLogits, void* ws, size_t ws_bytes) {
  MGR_REQUIRE(loss, "null argument");
  if (int rc = ctc_check_args(c, P, labels, input_len, label_len, B, T, C, Lmax, skip, blank, ws, ws_bytes)) return rc;
  const CtcWs L = ctc_ws_layout(ws, B, (size_t)T, C, Lmax);
  size_t lds_grad = (size_t)256 * (C + 1) * sizeof(float) + (size_t)(Lmax + 1) * sizeof(int);
  MGR_REQUIRE(lds_grad <= 160 * 1024, "C=%d too large for the LDS occupancy tile", C);
  const int frame_kib = c->tune[MGR_TUNE_CTC_FRAME_LDS_KIB];
  if (frame_kib > 0 && lds_grad < (size_t)frame_kib * 1024) lds_grad = (size_t)frame_kib * 1024;
  hipStream_t s = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_CTC);
  if (int rc = ctc_launch_chains(c, P, labels, input_len, label_len, B, T, C, Lmax, skip, blank, eps, loss, L)) return rc;
  if (dLogits)
    hipLaunchKernelGGL(k_ctc_grad<false>, dim3((unsigned)((T + 255) / 256), B), dim3(256), lds_grad, s, P, labels, input_len, label_len, B, T, C, Lmax,
                       skip, blank, eps, gscale, loss, dLogits, L.LY, L.AL, L.BE, 0.f, nullptr, nullptr);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_CTC);
  return 0;
}

// frames a workgroup of the entropy gradient kernel: the largest of 256, 128, 64 whose two LDS rows a frame fit (0: none does)
static size_t ent_lds_bytes(int ft, int C, int Lmax) { return ((size_t)2 * ft * (C + 1) + (Lmax + 1)) * sizeof(float); }
static int ent_frame_tile(int C, int Lmax) {
  for (int ft = 256; ft >= 64; ft >>= 1)
    if (ent_lds_bytes(ft, C, Lmax) <= (size_t)kOccLdsMax) return ft;
  return 0;
}

int mgr_ctc_entropy_grad(mgr_ctx* c, const float* P, const int32_t* labels, const int32_t* input_len, const int32_t* label_len, int B, int T,
                         int C, int Lmax, int skip, int blank, float eps, float loss_scale, float ent_scale, float* loss, float* entropy,
                         float* dLogits, void* ws, size_t ws_bytes) {
  MGR_REQUIRE(loss && entropy, "null argument");
  if (int rc = ctc_check_args(c, P, labels, input_len, label_len, B, T, C, Lmax, skip, blank, ws, ws_bytes)) return rc;
  MGR_REQUIRE(ws_bytes >= 2 * mgr_ctc_ws_bytes(B, T, C, Lmax), "workspace too small (2 * mgr_ctc_ws_bytes)");
  const CtcWs L = ctc_ws_layout(ws, B, (size_t)T, C, Lmax);
  const CtcEntWs E = ctc_ent_ws_layout(ws, B, (size_t)T, C, Lmax);
  const bool with_ent = ent_scale != 0.f;   // (ent_scale 0: the loss's own gradient kernel, the loss's bits)
  const int ft = with_ent ? ent_frame_tile(C, Lmax) : 256;
  size_t lds_grad = with_ent ? ent_lds_bytes(ft, C, Lmax) : (size_t)256 * (C + 1) * sizeof(float) + (size_t)(Lmax + 1) * sizeof(int);
  MGR_REQUIRE(!dLogits || (ft > 0 && lds_grad <= 160 * 1024), "C=%d too large for the LDS occupancy tile", C);
  const int frame_kib = c->tune[MGR_TUNE_CTC_FRAME_LDS_KIB];
  if (frame_kib > 0 && lds_grad < (size_t)frame_kib * 1024) lds_grad = (size_t)frame_kib * 1024;
  hipStream_t s = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_CTC);
  if (int rc = ctc_launch_chains(c, P, labels, input_len, label_len, B, T, C, Lmax, skip, blank, eps, loss, L, &E, entropy,
                                 (dLogits && with_ent) ? 1 : 0))   // (the rows the entropy's gradient kernel reads: ent_rows)
    return rc;
  if (dLogits && with_ent)
    hipLaunchKernelGGL(k_ctc_grad<true>, dim3((unsigned)((T + ft - 1) / ft), B), dim3(ft), lds_grad, s, P, labels, input_len, label_len, B, T, C, Lmax,
                       skip, blank, eps, loss_scale, loss, dLogits, L.LY, L.AL, L.BE, ent_scale, E.XA, E.XB);
  else if (dLogits)
    hipLaunchKernelGGL(k_ctc_grad<false>, dim3((unsigned)((T + 255) / 256), B), dim3(256), lds_grad, s, P, labels, input_len, label_len, B, T, C, Lmax,
                       skip, blank, eps, loss_scale, loss, dLogits, L.LY, L.AL, L.BE, 0.f, nullptr, nullptr);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_CTC);
  return 0;
}

int mgr_ctc_occupancy(mgr_ctx* c, const float* P, const int32_t* labels, const int32_t* input_len, const int32_t* label_len, int B, int T,
                      int C, int Lmax, int skip, int blank, float eps, float quantile, float* gamma, int32_t* seg, float* occ, float* conf,
                      double* logp, void* ws, size_t ws_bytes) {
  MGR_REQUIRE(seg && occ && conf && logp, "null argument");
  if (int rc = ctc_check_args(c, P, labels, input_len, label_len, B, T, C, Lmax, skip, blank, ws, ws_bytes)) return rc;
  MGR_REQUIRE(quantile > 0.f && quantile <= 0.5f, "quantile %g outside (0, 0.5]", (double)quantile);
  const int ft = occ_frame_tile(C, Lmax);
  MGR_REQUIRE(ft > 0, "C=%d too large for the LDS tiles at Lmax=%d", C, Lmax);
  const CtcWs L = ctc_ws_layout(ws, B, (size_t)T, C, Lmax);
  hipStream_t s = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_CTC);
  // the chains write the loss as B floats: into the head of conf (B * Lmax >= B floats, all of them rewritten by k_ctc_occupancy)
  if (int rc = ctc_launch_chains(c, P, labels, input_len, label_len, B, T, C, Lmax, skip, blank, eps, conf, L)) return rc;
  hipLaunchKernelGGL(k_occ_logp, dim3((B + 255) / 256), dim3(256), 0, s, conf, B, logp);
  hipLaunchKernelGGL(k_ctc_occupancy, dim3(B), dim3(256), occ_lds_bytes(ft, C, Lmax), s, P, labels, input_len, label_len, B, T, C, Lmax, skip, ft,
                     quantile, logp, gamma, seg, occ, conf, L.LY, L.AL, L.BE);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_CTC);
  return 0;
}

}  // extern "C"
