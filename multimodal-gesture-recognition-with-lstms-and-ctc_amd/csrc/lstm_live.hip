// Live recognition: mgr_lstm_scan_window - one direction of one layer over a WINDOW of a session that is still being
// produced, with the forward direction's (h, c) carried from window to window.  Inference only.
//
// One 16-wave workgroup per (job, group of kNB sessions); no workgroup talks to or waits for another.  Per step the workgroup forms
// z = Z[t] + h_{t-1} . Up for all H units of its sessions:
//   - h_{t-1} lives in LDS, double-buffered, as [k][kNB] so that one 16-byte read gives the kNB sessions' h_k;
//   - c lives in registers of the thread that owns the unit;
//   - Up (packed: the four gates of unit u at row k are 16 contiguous bytes) is streamed from L2 every step.  The waves form a
//     (units x k) grid: nuw = ceil(H / 64) waves along the units, ks = min(8, 16 / nuw) along k, each k part a contiguous range of
//     kc = ceil(H / ks) rows.  A wave's load of one row is one 1 KiB line run; ks parts of a unit column are in flight at once.
//   - parts 1 .. ks-1 leave their partial sums in LDS; part 0 adds them IN PART ORDER to its own (which began with Z[t]) and runs
//     the cell.  nuw, ks and kc depend on H alone, and a session's arithmetic does not involve its slot in the group: the bits
//     of a step are a function of (Z[t], h, c, Up, H) only.
// Sessions of a group may have different lengths: every session starts at step 0 (a reverse one at its own last frame) and drops
// out when its n_valid frames are done.
#include "lstm_common.h"

namespace {

constexpr int kNB = 4;          // sessions per workgroup (as lstm_simple.hip's NB)
constexpr int kWaves = 16;
constexpr int kThreads = kWaves * 64;
constexpr int kMaxKs = 8;

struct LiveJobs {
  const float* Z[MGR_LIVE_MAX_JOBS];
  const float* Up[MGR_LIVE_MAX_JOBS];
  float* Y[MGR_LIVE_MAX_JOBS];
  const float* R[MGR_LIVE_MAX_JOBS];
  float* state[MGR_LIVE_MAX_JOBS];
  int ldy[MGR_LIVE_MAX_JOBS], ldr[MGR_LIVE_MAX_JOBS], H[MGR_LIVE_MAX_JOBS], reverse[MGR_LIVE_MAX_JOBS];
};

// the wave grid of a layer width: a function of H alone (the host sizes the LDS with the same numbers)
__host__ __device__ static inline void live_grid(int H, int* nuw, int* ks, int* kc) {
  *nuw = (H + 63) / 64;
  int s = kWaves / *nuw;
  *ks = s > kMaxKs ? kMaxKs : s;
  *kc = (H + *ks - 1) / *ks;
}
static inline size_t live_lds_bytes(int H) {
  int nuw, ks, kc;
  live_grid(H, &nuw, &ks, &kc);
  return ((size_t)2 * H * kNB + (size_t)(ks - 1) * kNB * nuw * 64 * 4) * sizeof(float);
}

__global__ __launch_bounds__(kThreads) void k_scan_window(LiveJobs J, int S, int Tw, const int32_t* __restrict__ n_valid,
                                                           const int32_t* __restrict__ n_keep) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int j = blockIdx.y, s0 = blockIdx.x * kNB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = J.H[j], N = 4 * H, reverse = J.reverse[j];
  const float* __restrict__ Z = J.Z[j];
  const float* __restrict__ Up = J.Up[j];
  const float* __restrict__ R = J.R[j];
  float* __restrict__ Y = J.Y[j];
  float* __restrict__ state = J.state[j];
  const int ldy = J.ldy[j], ldr = J.ldr[j];
  int nuw, ks, kc;
  live_grid(H, &nuw, &ks, &kc);
  const int NU = nuw * 64;
  float* hs = lds;                                                        // [2][H][kNB]
  float4* red = reinterpret_cast<float4*>(lds + (size_t)2 * H * kNB);     // [ks - 1][kNB][NU]

  // lengths of this group's sessions (uniform over the workgroup)
  int nv[kNB], nk[kNB], steps = 0;
#pragma unroll
  for (int s = 0; s < kNB; ++s) {
    int v = 0, k = 0;
    if (s0 + s < S) {
      v = n_valid[s0 + s];
      v = v < 0 ? 0 : (v > Tw ? Tw : v);
      k = n_keep[s0 + s];
      k = k < 0 ? 0 : (k > v ? v : k);
    }
    nv[s] = v, nk[s] = k;
    steps = v > steps ? v : steps;
  }
  if (steps == 0) return;   // every session of the group is idle: nothing is read, nothing is written

  const int part = wave / nuw, uw = wave - part * nuw;
  const int u = uw * 64 + lane;
  const bool in_grid = wave < nuw * ks;
  const bool owner = in_grid && part == 0 && u < H;      // runs the cell of unit u
  const bool worker = in_grid && u < H;                  // streams a k range of unit u's column
  const int k0 = part * kc, k1 = (k0 + kc) < H ? (k0 + kc) : H;

  float c[kNB];
#pragma unroll
  for (int s = 0; s < kNB; ++s) {
    c[s] = 0.f;
    if (owner && state && nv[s] > 0) c[s] = state[((size_t)(s0 + s) * 2 + 1) * H + u];
  }
  for (int i = tid; i < H * kNB; i += kThreads) {
    const int k = i / kNB, s = i - k * kNB;
    float h0 = 0.f;
    if (state && nv[s] > 0) h0 = state[(size_t)(s0 + s) * 2 * H + k];
    hs[i] = h0;
    hs[H * kNB + i] = 0.f;
  }
  __syncthreads();

  int cur = 0;
  for (int step = 0; step < steps; ++step) {
    float4 acc[kNB];
#pragma unroll
    for (int s = 0; s < kNB; ++s) {
      acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (owner && step < nv[s]) {
        const int t = reverse ? nv[s] - 1 - step : step;
        acc[s] = *reinterpret_cast<const float4*>(Z + ((size_t)(s0 + s) * Tw + t) * N + u * 4);
      }
    }
    const float4* hc = reinterpret_cast<const float4*>(hs + (size_t)cur * H * kNB);
    if (worker) {
      const float* up = Up + (size_t)u * 4;
#pragma unroll 8
      for (int k = k0; k < k1; ++k) {
        const float4 uv = *reinterpret_cast<const float4*>(up + (size_t)k * N);
        const float4 h4 = hc[k];
        const float hk[kNB] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
        for (int s = 0; s < kNB; ++s) {
          acc[s].x += hk[s] * uv.x;
          acc[s].y += hk[s] * uv.y;
          acc[s].z += hk[s] * uv.z;
          acc[s].w += hk[s] * uv.w;
        }
      }
      if (part > 0) {
#pragma unroll
        for (int s = 0; s < kNB; ++s) red[((size_t)(part - 1) * kNB + s) * NU + u] = acc[s];
      }
    }
    __syncthreads();
    float* hn = hs + (size_t)(cur ^ 1) * H * kNB;
    if (owner) {
      for (int p = 1; p < ks; ++p) {
#pragma unroll
        for (int s = 0; s < kNB; ++s) {
          const float4 r = red[((size_t)(p - 1) * kNB + s) * NU + u];
          acc[s].x += r.x;
          acc[s].y += r.y;
          acc[s].z += r.z;
          acc[s].w += r.w;
        }
      }
      float hv[kNB];
#pragma unroll
      for (int s = 0; s < kNB; ++s) {
        hv[s] = 0.f;
        if (step < nv[s]) {
          const int t = reverse ? nv[s] - 1 - step : step;
          float4 g4;
          const float h = mgr_cell_fwd(acc[s].x, acc[s].y, acc[s].z, acc[s].w, c[s], g4);
          hv[s] = h;
          const size_t row = (size_t)(s0 + s) * Tw + t;
          float yo = h;
          if (R) yo += R[row * ldr + u];
          Y[row * ldy + u] = yo;
          if (state && step == nk[s] - 1) {   // (forward jobs only: the state the next window starts from)
            state[(size_t)(s0 + s) * 2 * H + u] = h;
            state[((size_t)(s0 + s) * 2 + 1) * H + u] = c[s];
          }
        }
      }
      *reinterpret_cast<float4*>(hn + (size_t)u * kNB) = make_float4(hv[0], hv[1], hv[2], hv[3]);
    }
    __syncthreads();
    cur ^= 1;
  }
  // the tail of every session that is not idle: rows n_valid .. Tw - 1, columns 0 .. H - 1
#pragma unroll
  for (int s = 0; s < kNB; ++s) {
    if (nv[s] == 0) continue;
    const int n = (Tw - nv[s]) * H;
    for (int i = tid; i < n; i += kThreads) {
      const int r = i / H, col = i - r * H;
      Y[((size_t)(s0 + s) * Tw + nv[s] + r) * ldy + col] = 0.f;
    }
  }
}

}  // namespace

extern "C" {

int mgr_lstm_scan_window(mgr_ctx* c, int njobs, const mgr_live_job* jobs, int S, int Tw, const int32_t* n_valid, const int32_t* n_keep,
                         const int32_t* h_n_valid, const int32_t* h_n_keep) {
  MGR_REQUIRE(jobs, "null job list");
  MGR_REQUIRE(njobs >= 1 && njobs <= MGR_LIVE_MAX_JOBS, "njobs = %d (1 .. %d)", njobs, MGR_LIVE_MAX_JOBS);
  MGR_REQUIRE(S >= 1 && Tw >= 1, "bad shape S=%d Tw=%d", S, Tw);
  MGR_REQUIRE(n_valid && n_keep, "null n_valid / n_keep");
  MGR_REQUIRE(((uintptr_t)n_valid & 3) == 0 && ((uintptr_t)n_keep & 3) == 0, "n_valid / n_keep must be 4-byte aligned");
  MGR_REQUIRE((h_n_valid == nullptr) == (h_n_keep == nullptr), "h_n_valid and h_n_keep go together");
  LiveJobs J;
  memset(&J, 0, sizeof J);
  size_t lds = 0;
  for (int j = 0; j < njobs; ++j) {
    const mgr_live_job& q = jobs[j];
    MGR_REQUIRE(q.H >= 1 && q.H <= MGR_LIVE_MAX_H, "job %d: H = %d (1 .. %d)", j, q.H, MGR_LIVE_MAX_H);
    MGR_REQUIRE(q.Z && q.Up && q.Y, "job %d: null Z / Up / Y", j);
    MGR_REQUIRE(((uintptr_t)q.Z & 15) == 0 && ((uintptr_t)q.Up & 15) == 0, "job %d: Z and Up must be 16-byte aligned", j);
    MGR_REQUIRE(((uintptr_t)q.Y & 3) == 0 && ((uintptr_t)q.R & 3) == 0 && ((uintptr_t)q.state & 3) == 0, "job %d: misaligned Y / R / state", j);
    MGR_REQUIRE(q.ldy >= q.H, "job %d: ldy = %d < H = %d", j, q.ldy, q.H);
    MGR_REQUIRE(!q.R || q.ldr >= q.H, "job %d: ldr = %d < H = %d", j, q.ldr, q.H);
    MGR_REQUIRE(q.reverse ? q.state == nullptr : q.state != nullptr, "job %d: a forward job carries a state, a reverse job has none", j);
    J.Z[j] = q.Z, J.Up[j] = q.Up, J.Y[j] = q.Y, J.R[j] = q.R, J.state[j] = q.state;
    J.ldy[j] = q.ldy, J.ldr[j] = q.ldr, J.H[j] = q.H, J.reverse[j] = q.reverse != 0;
    const size_t need = live_lds_bytes(q.H);
    lds = need > lds ? need : lds;
  }
  if (h_n_valid)
    for (int s = 0; s < S; ++s)
      MGR_REQUIRE(h_n_keep[s] >= 0 && h_n_keep[s] <= h_n_valid[s] && h_n_valid[s] <= Tw, "session %d: n_keep = %d, n_valid = %d, Tw = %d (0 <= n_keep <= n_valid <= Tw)",
                  s, h_n_keep[s], h_n_valid[s], Tw);
  MGR_REQUIRE(c, "null context");
  MGR_REQUIRE(lds <= 64 * 1024, "internal: %zu bytes of LDS", lds);
  mgr_prof_begin(c, MGR_K_SCAN_FWD);
  hipLaunchKernelGGL(k_scan_window, dim3((unsigned)((S + kNB - 1) / kNB), (unsigned)njobs), dim3(kThreads), lds, mgr_stream(c), J, S, Tw, n_valid,
                     n_keep);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_SCAN_FWD);
  return 0;
}

}  // extern "C"
