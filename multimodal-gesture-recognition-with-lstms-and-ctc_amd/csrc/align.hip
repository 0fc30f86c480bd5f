// K11: locating gestures in time.  Two device operations:
//
// mgr_ctc_align - Viterbi forced alignment: the alpha recursion of ctc.hip with max in place of log-sum-exp, a 2-bit back-pointer per
// frame and state, and a backtrace.  Two kernels: emissions (k_lattice_emissions in natural-log units: a thread per frame, class-major
// rows), then one WAVE per sample over the lattice as ctc_lattice.h lays it across the lanes: (blank, label) pairs, lane * PPL + j holds
// states 2p and 2p + 1, the only cross-lane traffic of a step is one DPP shift of the neighbouring pair's label value, and a lane
// fetches CH steps of its label's and the blank's emissions with 16-byte loads, a chunk ahead of the recursion.  The pairs, the chunks,
// the renormalisation and the pick of the final states come from that header; the max step, the back-pointer packing and the backtrace
// are this file's.
// Back-pointers: a pair's two pointers are one nibble per frame; a lane collects eight frames of a pair in one register and stores one
// word per pair and eight frames: (Lmax + 1) * ceil(To / 8) words, 143 KB at 301 states and 1898 frames, 34 KB at 71 states.  They live
// in the workgroup's LDS when they fit 160 KB (every shape the networks have) and in the workspace otherwise: the backtrace is a chain
// of dependent reads (one per eight frames while the path stays in a state, one per frame while it climbs), ~100 cycles each from
// LDS, about a microsecond each from global memory.  The chain runs on the scalar unit; turning states into classes and segments is
// a parallel pass over the frames behind it.
// Numerics: natural-log units, f32 running values kept O(10) by subtracting the wave maximum every 16 frames and summing it in fp64
// (as alpha is in ctc.hip), so log p of a 1900-frame path (10^3 .. 10^4) does not sit where an f32 ulp is 5e-4.
// Ties: the smaller step wins a back-pointer tie (stay, one state, two states), the last blank wins a tie of the two final states.
//
// mgr_greedy_segments - the greedy decode of K9 with its frame positions: frame argmax, the reference's confidence filter in its net
// effect (for every label s the first k_s frames whose best label is s are dropped, k_s = the number of such frames below the
// threshold), the collapse of repeats, and per run its label, first / last surviving frame and mean probability.  One workgroup per
// sample, everything per frame in LDS: per-label counts by LDS atomics, the frame of a label's k_s-th occurrence by a ballot scan (one
// wave per label), survivors and run starts by two block-wide prefix sums.
#include "ctc_lattice.h"

namespace {

// row length of the class-major emissions: To + the over-read of two chunks of 8 steps, a multiple of 4 floats
__host__ __device__ inline size_t align_ts(int To) { return ((size_t)To + 16 + 3) / 4 * 4; }
__host__ __device__ inline int align_nb(int To) { return (To + 7) / 8; }   // back-pointer blocks of eight frames
__host__ __device__ inline int align_state_words(int To) { return (To + 63) / 64 * 32; }   // uint16 per frame, whole blocks of 64 frames
// One wave per sample.  LDS: the label row, first / last frame per label, the path's state per frame, then (LDS_BP) the back-pointer words.
template <int PPL, bool LDS_BP>
__global__ __launch_bounds__(64) void k_ctc_align(const float* __restrict__ P, const int32_t* __restrict__ labels,
                                                  const int32_t* __restrict__ input_len, const int32_t* __restrict__ label_len, int T, int C,
                                                  int Lmax, int skip, int blank, const float* __restrict__ E, uint32_t* __restrict__ BPg,
                                                  int32_t* __restrict__ path, int32_t* __restrict__ seg, float* __restrict__ conf,
                                                  double* __restrict__ logp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  constexpr int CH = Chunk<PPL>::CH;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int To = T - skip, NP = Lmax + 1, NB = align_nb(To);
  const size_t TS = align_ts(To);
  const int Tp = clip_len(input_len[b], To), L = clip_len(label_len[b], Lmax);
  int* s_lab = reinterpret_cast<int*>(smem);
  int* s_first = s_lab + NP;
  int* s_last = s_first + NP;
  uint16_t* s_state = reinterpret_cast<uint16_t*>(s_last + NP);   // the path's state per frame: align_state_words(To) words
  uint32_t* bp = LDS_BP ? smem + 3 * NP + align_state_words(To) : BPg + (size_t)b * NB * NP;
  const float* Eb = E + (size_t)b * C * TS;
  for (int i = lane; i < NP; i += 64) {   // labels clipped into the class range, as ctc.hip's ctc_labels
    s_lab[i] = clip_label((i < L) ? labels[(size_t)b * Lmax + i] : -1, C);
    s_first[i] = -1;
    s_last[i] = -1;
  }
  __syncthreads();

  const Pairs<PPL> pr(s_lab, L, blank, lane);   // (cs: the skip of two states, as in the loss)

  float ab[PPL], al[PPL];
  double coff = 0.0;
  if (Tp > 0) {
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int p = lane * PPL + j;
      ab[j] = (p == 0) ? Eb[(size_t)blank * TS] : kNegInf;
      al[j] = (p == 0 && pr.vl[j]) ? Eb[(size_t)pr.lab[j] * TS] : kNegInf;
    }
    Chunk<PPL> cur, nxt;   // steps t0 .. t0 + CH - 1, t0 a multiple of 4: 16-byte aligned
    cur.load(Eb, TS, blank, pr.lab, 0);
    uint32_t bits[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) bits[j] = 0u;
    int since = 0;
    for (int t0 = 0; t0 < Tp; t0 += CH) {
      nxt.load(Eb, TS, blank, pr.lab, t0 + CH);
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        const int t = t0 + k;
        if (t >= 1 && t < Tp) {
          const float carry = dpp_f32<DPP_WAVE_SHR1>(al[PPL - 1], kNegInf);   // (lane 0: log 0)
          float nb[PPL], nl[PPL];
          const int sh = 4 * (t & 7);
#pragma unroll
          for (int j = 0; j < PPL; ++j) {
            const float up = (j > 0) ? al[j - 1] : carry;
            // blank state 2p: stay (0), or from label p - 1 (1); a tie stays
            const bool b1 = up > ab[j];
            nb[j] = pr.vb[j] ? cur.eb[k] + (b1 ? up : ab[j]) : kNegInf;
            // label state 2p + 1: stay (0), from its blank (1), from label p - 1 where the skip is allowed (2); a tie takes the smaller step
            float m = al[j];
            uint32_t s = 0u;
            if (ab[j] > m) { m = ab[j]; s = 1u; }
            const float u2 = pr.cs[j] ? up : kNegInf;
            if (u2 > m) { m = u2; s = 2u; }
            nl[j] = pr.vl[j] ? cur.el[k][j] + m : kNegInf;
            bits[j] |= ((b1 ? 1u : 0u) | (s << 2)) << sh;
          }
#pragma unroll
          for (int j = 0; j < PPL; ++j) {
            ab[j] = nb[j];
            al[j] = nl[j];
          }
        }
      }
      if (((t0 + CH) & 7) == 0 || t0 + CH >= Tp) {   // eight frames of back-pointers (or the last ones) are complete: one word per pair
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
          const int p = lane * PPL + j;
          if (p <= Lmax) bp[(size_t)(t0 >> 3) * NP + p] = bits[j];
          bits[j] = 0u;
        }
      }
      cur = nxt;
      since += CH;
      if (since >= 16) {   // renormalise: keep the running values O(10)
        since = 0;
        coff += (double)renorm(ab, al);
      }
    }
  }
  // the two final states: the last blank 2L and the last label 2L - 1; a tie takes the blank
  const float2 f = Tp > 0 ? final_states(ab, al, L, lane) : make_float2(kNegInf, kNegInf);   // (Tp is uniform over the wave)
  const float fb = f.x, fl = f.y;
  const float fin = fmaxf(fb, fl);
  const bool feasible = fin != kNegInf;
  __syncthreads();   // the back-pointer words of every lane are in place
  if (lane == 0) logp[b] = feasible ? (double)fin + coff : -(double)__builtin_huge_valf();
  if (feasible) {
    // The backtrace is a chain of Tp dependent steps.  Every lane runs it with wave-uniform values, so the chain itself is scalar
    // instructions (a one-lane vector loop pays the full vector issue latency for each of its ~40 instructions per frame: 0.27 of
    // the first version's 0.42 ms at the fusion shape).  The back-pointer word in hand covers eight frames of one pair: a path that
    // stays in its state reads LDS once per eight frames and takes them in one step.  Lane t % 64 keeps the state of frame t; 64
    // frames are stored at a time.
    int s = __builtin_amdgcn_readfirstlane((fb >= fl) ? 2 * L : 2 * L - 1);
    uint32_t w = 0u;
    int wkey = -1, mine = 0;
    int t = Tp - 1;
    while (t >= 0) {
      const int k = t & 7, q = t & 63;
      const int key = (t >> 3) * NP + (s >> 1);
      if (key != wkey) {
        w = __builtin_amdgcn_readfirstlane(bp[key]);
        wkey = key;
      }
      // this state's pointers at frames t - k .. t of the block (frame 0's nibble is zero: nothing points out of it)
      const uint32_t stay = w & ((s & 1) ? 0xCCCCCCCCu : 0x33333333u) & (0xFFFFFFFFu >> (28 - 4 * k));
      if (stay == 0u) {   // all "stay": the rest of the block in one step (a trained network's paths wait in blanks most of the time)
        if ((lane >> 3) == (q >> 3) && (lane & 7) <= k) mine = s;
        if ((q - k) == 0) s_state[t - k + lane] = (uint16_t)mine;   // frames t - k .. t - k + 63 (those from Tp on are not read)
        t -= k + 1;
      } else {
        if (q == lane) mine = s;
        if (q == 0) s_state[t + lane] = (uint16_t)mine;
        const uint32_t nib = (w >> (4 * k)) & 15u;
        s -= (s & 1) ? (int)(nib >> 2) : (int)(nib & 3u);
        if (s < 0) s = 0;   // (cannot happen with pointers this kernel wrote; keeps the LDS reads in range whatever they hold)
        t -= 1;
      }
    }
  }
  __syncthreads();
  // states -> classes, and the first / last frame of every label state (each has exactly one writer)
  if (feasible) {
    for (int t = lane; t < Tp; t += 64) {
      const int st = s_state[t], p = st >> 1;
      path[(size_t)b * To + t] = (st & 1) ? s_lab[p] : blank;
      if (st & 1) {
        if (t == 0 || s_state[t - 1] != st) s_first[p] = t;
        if (t == Tp - 1 || s_state[t + 1] != st) s_last[p] = t;
      }
    }
  }
  __syncthreads();
  for (int t = (feasible ? Tp : 0) + lane; t < To; t += 64) path[(size_t)b * To + t] = -1;
  for (int k = lane; k < Lmax; k += 64) {
    int f = -1, l = -1;
    float cf = 0.f;
    if (feasible && k < L) {
      f = s_first[k];
      l = s_last[k];
      const float* col = P + ((size_t)b * T + skip) * C + s_lab[k];
      float sum = 0.f;
      for (int t = f; t <= l; ++t) sum += col[(size_t)t * C];
      cf = sum / (float)(l - f + 1);
      f += skip;
      l += skip;
    }
    seg[((size_t)b * Lmax + k) * 2] = f;
    seg[((size_t)b * Lmax + k) * 2 + 1] = l;
    conf[(size_t)b * Lmax + k] = cf;
  }
}

// exclusive prefix sum of one int per thread over the 256 threads of a workgroup; *total = the sum
__device__ __forceinline__ int block_excl_scan256(int v, int* sh, int tid, int* total) {
  sh[tid] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int x = tid >= o ? sh[tid - o] : 0;
    __syncthreads();
    sh[tid] += x;
    __syncthreads();
  }
  const int incl = sh[tid];
  *total = sh[255];
  __syncthreads();
  return incl - v;
}

// One workgroup per sample.  LDS: best, prob, idx (surviving frames in order), rs (position of each run's first frame in idx) [To]
// each; cnt, cut [C]; the scan's 256 words.
__global__ __launch_bounds__(256) void k_greedy_segments(const float* __restrict__ P, int T, int C, int skip, float thr, int cap,
                                                         int32_t* __restrict__ n_runs, int32_t* __restrict__ rlab, int32_t* __restrict__ rseg,
                                                         float* __restrict__ rconf) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int To = T - skip;
  int* best = reinterpret_cast<int*>(smem);
  float* prob = reinterpret_cast<float*>(best + To);
  int* idx = reinterpret_cast<int*>(prob + To);
  int* rs = idx + To;
  int* cnt = rs + To;
  int* cut = cnt + C;
  int* sh = cut + C;
  for (int c = tid; c < C; c += 256) {
    cnt[c] = 0;
    cut[c] = -1;
  }
  __syncthreads();
  // frame argmax (first index on ties, as mgr_frame_argmax) and the per-label count of frames below the threshold
  for (int t = tid; t < To; t += 256) {
    const float* row = P + ((size_t)b * T + skip + t) * C;
    float mx = row[0];
    int am = 0;
    for (int c = 1; c < C; ++c) {
      const float v = row[c];
      if (v > mx) {
        mx = v;
        am = c;
      }
    }
    best[t] = am;
    prob[t] = mx;
    if (mx < thr) atomicAdd(&cnt[am], 1);
  }
  __syncthreads();
  // cut[s] = the frame of the k_s-th occurrence of label s (the last one the filter drops), one wave per label
  for (int s = wave; s < C; s += 4) {
    const int k = cnt[s];
    if (k == 0) continue;
    int seen = 0;
    for (int base = 0; base < To; base += 64) {
      const int t = base + lane;
      const bool hit = t < To && best[t] == s;
      const unsigned long long m = __ballot(hit);
      const int n = __popcll(m);
      if (seen + n >= k) {
        if (hit && seen + __popcll(m & ((1ull << lane) - 1ull)) == k - 1) cut[s] = t;
        break;
      }
      seen += n;
    }
  }
  __syncthreads();
  // surviving frames, in order
  const int chunk = (To + 255) / 256;
  int nsurv, nruns;
  {
    const int t0 = tid * chunk, t1 = min(t0 + chunk, To);
    int n = 0;
    for (int t = t0; t < t1; ++t) n += t > cut[best[t]];
    int o = block_excl_scan256(n, sh, tid, &nsurv);
    for (int t = t0; t < t1; ++t)
      if (t > cut[best[t]]) idx[o++] = t;
  }
  __syncthreads();
  // run starts among the survivors
  {
    const int chunk2 = (nsurv + 255) / 256;
    const int i0 = tid * chunk2, i1 = min(i0 + chunk2, nsurv);
    int n = 0;
    for (int i = i0; i < i1; ++i) n += (i == 0 || best[idx[i]] != best[idx[i - 1]]);
    int o = block_excl_scan256(n, sh, tid, &nruns);
    for (int i = i0; i < i1; ++i)
      if (i == 0 || best[idx[i]] != best[idx[i - 1]]) rs[o++] = i;
  }
  __syncthreads();
  if (tid == 0) n_runs[b] = nruns;   // the TRUE count, whatever the capacity
  for (int r = tid; r < cap; r += 256) {
    int lb = -1, f = -1, l = -1;
    float cf = 0.f;
    if (r < nruns) {
      const int i0 = rs[r], i1 = (r + 1 < nruns) ? rs[r + 1] : nsurv;
      lb = best[idx[i0]];
      f = idx[i0] + skip;
      l = idx[i1 - 1] + skip;
      float sum = 0.f;
      for (int i = i0; i < i1; ++i) sum += prob[idx[i]];
      cf = sum / (float)(i1 - i0);
    }
    rlab[(size_t)b * cap + r] = lb;
    rseg[((size_t)b * cap + r) * 2] = f;
    rseg[((size_t)b * cap + r) * 2 + 1] = l;
    rconf[(size_t)b * cap + r] = cf;
  }
}

constexpr size_t kLdsMax = 160 * 1024;

}  // namespace

extern "C" {

// emissions | back-pointer words; laid out for T frames (the kernels use rows of T - skip: both fit) to keep the query simple
struct AlignWs { float* E; uint32_t* BPg; size_t bytes; };
static AlignWs align_ws_layout(void* ws, int B, int T, int C, int Lmax) {
  mgr_ws_carver w(ws);
  return {w.take<float>((size_t)B * C * align_ts(T)), w.take<uint32_t>((size_t)B * align_nb(T) * (Lmax + 1)), w.off};
}
size_t mgr_ctc_align_ws_bytes(int B, int T, int C, int Lmax) { return align_ws_layout(nullptr, B, T > 0 ? T : 1, C, Lmax).bytes; }

int mgr_ctc_align(mgr_ctx* c, const float* P, const int32_t* labels, const int32_t* input_len, const int32_t* label_len, int B, int T, int C,
                  int Lmax, int skip, int blank, float eps, int32_t* path, int32_t* seg, float* conf, double* logp, void* ws, size_t ws_bytes) {
  MGR_REQUIRE(c && P && labels && input_len && label_len && path && seg && conf && logp, "null argument");
  mgr_planes_forget_range(c, ws, ws_bytes);   // (this call writes its workspace: kept weight planes in it are gone)
  MGR_REQUIRE(B > 0 && T > skip && skip >= 0 && C > 1 && Lmax > 0, "bad shape B=%d T=%d C=%d Lmax=%d skip=%d", B, T, C, Lmax, skip);
  MGR_REQUIRE(blank >= 0 && blank < C, "blank %d out of range", blank);
  MGR_REQUIRE(Lmax + 1 <= 256, "Lmax %d too large (max 255)", Lmax);
  MGR_REQUIRE(ws && ws_bytes >= mgr_ctc_align_ws_bytes(B, T, C, Lmax), "workspace too small");
  const int To = T - skip, NP = Lmax + 1;
  const AlignWs L = align_ws_layout(ws, B, T, C, Lmax);
  const size_t lds_small = ((size_t)3 * NP + align_state_words(To)) * sizeof(int);
  const size_t lds_full = lds_small + (size_t)align_nb(To) * NP * sizeof(uint32_t);
  const bool in_lds = lds_full <= kLdsMax;
  MGR_REQUIRE(lds_small <= kLdsMax, "T - skip = %d too large for the LDS frame states", To);
  if (!(c->attr_done & MGR_ATTR_ALIGN)) {
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_align<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_align<2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_align<3, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_align<4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_align<1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_align<2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_align<3, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ctc_align<4, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    c->attr_done |= MGR_ATTR_ALIGN;
  }
  const int ppl = (NP + 63) / 64;
  hipStream_t s = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_CTC);
  hipLaunchKernelGGL(k_lattice_emissions<false>, dim3((unsigned)((align_ts(To) + 255) / 256), B), dim3(256), 0, s, P, input_len, T, C, skip, eps,
                     align_ts(To), L.E);
#define MGR_ALIGN_LAUNCH(N)                                                                                                                \
  do {                                                                                                                                     \
    if (in_lds)                                                                                                                            \
      hipLaunchKernelGGL((k_ctc_align<N, true>), dim3(B), dim3(64), lds_full, s, P, labels, input_len, label_len, T, C, Lmax, skip, blank, \
                         L.E, L.BPg, path, seg, conf, logp);                                                                               \
    else                                                                                                                                   \
      hipLaunchKernelGGL((k_ctc_align<N, false>), dim3(B), dim3(64), lds_small, s, P, labels, input_len, label_len, T, C, Lmax, skip,      \
                         blank, L.E, L.BPg, path, seg, conf, logp);                                                                        \
  } while (0)
  switch (ppl) {
    case 1: MGR_ALIGN_LAUNCH(1); break;
    case 2: MGR_ALIGN_LAUNCH(2); break;
    case 3: MGR_ALIGN_LAUNCH(3); break;
    default: MGR_ALIGN_LAUNCH(4); break;
  }
#undef MGR_ALIGN_LAUNCH
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_CTC);
  return 0;
}

int mgr_greedy_segments(mgr_ctx* c, const float* P, int B, int T, int C, int skip, float thr, int cap, int32_t* n_runs, int32_t* lab,
                        int32_t* seg, float* conf) {
  MGR_REQUIRE(c && P && n_runs && lab && seg && conf, "null argument");
  MGR_REQUIRE(B > 0 && T > skip && skip >= 0 && C > 0 && cap > 0, "bad shape B=%d T=%d C=%d skip=%d cap=%d", B, T, C, skip, cap);
  MGR_REQUIRE(T - skip <= MGR_SEGMENTS_MAX_FRAMES && C <= 1024, "T - skip = %d (max %d) or C = %d (max 1024) too large for the LDS frame arrays",
              T - skip, MGR_SEGMENTS_MAX_FRAMES, C);
  const size_t lds = ((size_t)4 * (T - skip) + 2 * (size_t)C + 256) * sizeof(int);
  if (!(c->attr_done & MGR_ATTR_SEGMENTS)) {
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_greedy_segments), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    c->attr_done |= MGR_ATTR_SEGMENTS;
  }
  mgr_prof_begin(c, MGR_K_MISC);
  hipLaunchKernelGGL(k_greedy_segments, dim3(B), dim3(256), lds, mgr_stream(c), P, T, C, skip, thr, cap, n_runs, lab, seg, conf);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}

}  // extern "C"
