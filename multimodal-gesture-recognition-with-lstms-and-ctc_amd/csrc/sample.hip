// K16: CTC hypotheses by sampling alignments (not present in the reference): K frame paths per sample drawn from the
// network's own per-frame distribution y = (P + eps) / sum_c (P + eps), collapsed to labellings, equal labellings merged and counted.
// What the beam search serialises over the frames is here one independent draw per (sample, draw, frame); the set is a pure function of
// (posteriors, seed) and is restated bit for bit on the host (tests/sample_ref.py): every float operation below is one IEEE f32 add,
// multiply or compare in the order include/mgr.h states.  There is no multiply next to an add that could be fused; contraction is
// switched off for the file all the same, and nothing here is compiled with a fast-math flag that would let the sums be reordered.
//
// Two kernels.  k_sample_draw, grid (K, B), 128 threads: the workgroup of draw k of sample b walks the Tp frames in chunks of 128.  A
// chunk's posterior rows are one contiguous piece of P: it is read coalesced into LDS (row stride C | 1 dwords: odd, so that a thread
// per frame reading its own row hits every bank once), then a thread per frame sums its C weights in class order (S), forms thr = u S
// and sums again to the first class whose running sum exceeds thr - the same adds, the same bits.  The collapse is a flag per frame
// (class != blank and != the class of the frame before) and its prefix sum: the flag is one bit, so the sum within a wave is a ballot
// and a population count below the lane, across the two waves one LDS word, across chunks a carried offset; every kept class is
// written to its final place in row k of out.  k_sample_merge, grid B, 256 threads: the K rows of a sample in draw order, each compared
// EXACTLY (lengths first, then every label; no hash) with the unique rows found so far; a new one moves down to the next free slot of
// out - unique rows only ever move to lower slots, whose former content has been compared already - so the kernel needs no workspace.
// No atomics anywhere; a sample's rows depend on its own posteriors, seed, b, K and T alone.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int FR = 128;   // frames (threads) per chunk of k_sample_draw
constexpr int MT = 256;   // threads of k_sample_merge

__device__ __forceinline__ int sm_clip_len(int len, int To) { return len < 0 ? 0 : (len > To ? To : len); }

// grid (K, B), FR threads; dynamic LDS: FR * (C | 1) floats
__global__ __launch_bounds__(FR) void k_sample_draw(const float* __restrict__ P, const int32_t* __restrict__ input_len, int T, int C, int skip,
                                                    int blank, float eps, uint64_t seed, int K, int32_t* __restrict__ out,
                                                    int32_t* __restrict__ out_len, int32_t* __restrict__ path) {
  extern __shared__ __attribute__((aligned(16))) float s_rows[];
  __shared__ int s_cls[FR];
  __shared__ int s_tot[FR / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = blockIdx.x, b = blockIdx.y;
  const int To = T - skip, RS = C | 1;
  const int Tp = sm_clip_len(input_len[b], To);
  const size_t row = (size_t)b * K + k;
  int32_t* orow = out + row * To;
  int32_t* prow = path ? path + row * To : nullptr;
  const float* Pb = P + ((size_t)b * T + skip) * C;
  int off = 0;         // labels written so far (uniform)
  int last = -1;       // class of the frame before the chunk (uniform); -1: no frame yet
  for (int t0 = 0; t0 < Tp; t0 += FR) {
    const int n = Tp - t0 < FR ? Tp - t0 : FR;
    const float* src = Pb + (size_t)t0 * C;
    for (int i = tid; i < n * C; i += FR) {
      const int r = i / C;
      s_rows[r * RS + (i - r * C)] = src[i];
    }
    __syncthreads();
    int cls = -1;
    if (tid < n) {
      const float* w = s_rows + tid * RS;
      float S = 0.f;
      for (int c = 0; c < C; ++c) S += w[c] + eps;
      const int t = skip + t0 + tid;
      const float u = (float)(mgr_rand_u32(seed, (uint64_t)row * (uint64_t)T + (uint64_t)t) >> 8) * (1.0f / 16777216.0f);
      const float thr = u * S;
      cls = blank;
      float cum = 0.f;
      for (int c = 0; c < C; ++c) {
        cum += w[c] + eps;
        if (cum > thr) {
          cls = c;
          break;
        }
      }
      if (prow) prow[t0 + tid] = cls;
    }
    s_cls[tid] = cls;
    __syncthreads();
    const int prev = tid == 0 ? last : s_cls[tid - 1];
    const bool keep = tid < n && cls != blank && cls != prev;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_tot[wave] = __popcll(m);
    __syncthreads();
    int pos = off + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += s_tot[w];
    if (keep) orow[pos] = cls;     // (pos < the number of frames seen so far <= Tp <= To)
    for (int w = 0; w < FR / 64; ++w) off += s_tot[w];
    last = s_cls[n - 1];
    __syncthreads();               // (s_rows, s_cls and s_tot are rewritten by the next chunk)
  }
  for (int i = off + tid; i < To; i += FR) orow[i] = -1;
  if (prow)
    for (int i = Tp + tid; i < To; i += FR) prow[i] = -1;
  if (tid == 0) out_len[row] = off;     // (draw order: k_sample_merge turns it into slot order)
}

// grid B, MT threads: rows of out / out_len in draw order -> unique rows in order of first occurrence, counts, absent slots
__global__ __launch_bounds__(MT) void k_sample_merge(int To, int K, int32_t* out, int32_t* out_len, int32_t* __restrict__ count,
                                                     int32_t* __restrict__ n_unique) {
  __shared__ int s_len[MGR_SAMPLE_MAX_DRAWS];    // length of draw k
  __shared__ int s_ulen[MGR_SAMPLE_MAX_DRAWS];   // length of unique slot j
  __shared__ int s_cnt[MGR_SAMPLE_MAX_DRAWS];
  const int tid = threadIdx.x, b = blockIdx.x;
  int32_t* ob = out + (size_t)b * K * To;
  if (tid < K) s_len[tid] = out_len[(size_t)b * K + tid];
  __syncthreads();
  int nu = 0;   // (uniform)
  for (int k = 0; k < K; ++k) {
    const int Lk = s_len[k];
    const int32_t* rk = ob + (size_t)k * To;
    int match = -1;
    for (int j = 0; j < nu; ++j) {
      if (s_ulen[j] != Lk) continue;     // (uniform: every thread skips or none)
      const int32_t* rj = ob + (size_t)j * To;
      int diff = 0;
      for (int i = tid; i < Lk; i += MT) diff |= rk[i] != rj[i];
      if (!__syncthreads_or(diff)) {
        match = j;
        break;
      }
    }
    if (match >= 0) {
      if (tid == 0) s_cnt[match] += 1;
    } else {
      if (nu != k) {                     // slot nu < k: its former row was a duplicate or has moved further down
        int32_t* rn = ob + (size_t)nu * To;
        for (int i = tid; i < To; i += MT) rn[i] = rk[i];
      }
      if (tid == 0) {
        s_ulen[nu] = Lk;
        s_cnt[nu] = 1;
      }
      ++nu;
    }
    __syncthreads();   // the moved row and the slot's length and count, before the next draw is compared with them
  }
  for (int j = nu; j < K; ++j) {
    int32_t* rj = ob + (size_t)j * To;
    for (int i = tid; i < To; i += MT) rj[i] = -1;
  }
  if (tid < K) {
    out_len[(size_t)b * K + tid] = tid < nu ? s_ulen[tid] : -1;
    count[(size_t)b * K + tid] = tid < nu ? s_cnt[tid] : 0;
  }
  if (tid == 0) n_unique[b] = nu;
}

}  // namespace

extern "C" {

int mgr_ctc_sample_paths(mgr_ctx* c, const float* P, const int32_t* input_len, int B, int T, int C, int skip, int blank, float eps,
                         uint64_t seed, int K, int32_t* out, int32_t* out_len, int32_t* count, int32_t* n_unique, int32_t* path) {
  MGR_REQUIRE(c && P && input_len && out && out_len && count && n_unique, "null argument");
  MGR_REQUIRE(B > 0 && T > skip && skip >= 0, "bad shape B=%d T=%d skip=%d", B, T, skip);
  MGR_REQUIRE(C >= 2 && C <= 64, "C = %d out of [2, 64]", C);
  MGR_REQUIRE(K >= 1 && K <= MGR_SAMPLE_MAX_DRAWS, "K = %d out of [1, %d]", K, MGR_SAMPLE_MAX_DRAWS);
  MGR_REQUIRE(B <= 65535, "B = %d too large (max 65535)", B);
  MGR_REQUIRE(blank >= 0 && blank < C, "blank %d out of range", blank);
  const int To = T - skip;
  const size_t lds = (size_t)FR * (C | 1) * sizeof(float);   // <= 33 280 bytes: below the limit a kernel has without asking
  hipStream_t s = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_CTC);
  hipLaunchKernelGGL(k_sample_draw, dim3(K, B), dim3(FR), lds, s, P, input_len, T, C, skip, blank, eps, seed, K, out, out_len, path);
  hipLaunchKernelGGL(k_sample_merge, dim3(B), dim3(MT), 0, s, To, K, out, out_len, count, n_unique);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_CTC);
  return 0;
}

}  // extern "C"
