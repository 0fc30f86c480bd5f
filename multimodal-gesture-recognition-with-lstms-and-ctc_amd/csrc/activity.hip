// Activity features of the skeletal network's raw joint files (reference skeletal_network/velocity.py, r_position.py):
// per file the hand velocities, the low-velocity mask, the hand rest position and each hand's distance from it.  Every output is an
// integer or a boolean, and every one is exact: integer radicands, floor(sqrt) corrected in integers, integer sums and counts.
//
// One workgroup (4 waves) per file of a ragged batch; thread t owns the file's frames t, t + 256, ... in every pass, so it reads back
// only what it stored itself:
//   1. lh_v / rh_v = floor(|cur - prev|) of the hand joints (rows 0..3 of the file: 0) and their int64 sums (wave shuffles, LDS);
//   2. low = lh_v n < sum(lh_v) && rh_v n < sum(rh_v) (the reference's v < mean, exactly) and its count; then the 16 rest-position
//      medians of the low frames by an exact radix select on order-preserving uint32 keys: 4 passes of 8-bit digits, one 256-bin LDS
//      histogram per (column, order statistic) - 16 columns, two statistics when the count is even;
//   3. lh_dist_rp / rh_dist_rp = floor(|rest hand - cur hand|) (rows 0..3: 0).
// No LDS buffer grows with the frame count, no global atomics: repeated launches give identical bytes.
#include "common.h"

namespace {

constexpr int ACT_THREADS = 256;
constexpr int ACT_WAVES = ACT_THREADS / 64;
constexpr int ACT_COLS = MGR_ACTIVITY_JOINT_COLS;   // hipX hipY shcX shcY | lsX lsY leX leY lwX lwY lhX lhY rsX rsY reX reY rwX rwY rhX rhY
constexpr int ACT_RP = MGR_ACTIVITY_REST_COLS;      // the rest position: columns 4..19
constexpr int ACT_OUT = MGR_ACTIVITY_OUT_COLS;      // lh_v rh_v low lh_dist_rp rh_dist_rp
constexpr int ACT_SEL = 2 * ACT_RP;                 // (column, lower / upper middle order statistic)
constexpr int LH = 10, RH = 18;                     // lhX, rhX
constexpr int RP_LH = LH - 4, RP_RH = RH - 4;

// floor(sqrt(n)) of an exact integer n < 2^53: the device sqrt may be an ulp low (sqrt(25) -> 4.999...), so the floor is corrected
__device__ __forceinline__ int isqrt_exact(long long n) {
  long long r = (long long)sqrt((double)n);
  while (r * r > n) --r;
  while ((r + 1) * (r + 1) <= n) ++r;
  return (int)r;
}

// int(scipy pdist euclidean) of two integer points (coordinates within +-2^20: the radicand is exact)
__device__ __forceinline__ int dist_floor(int ax, int ay, int bx, int by) {
  const long long dx = (long long)ax - bx, dy = (long long)ay - by;
  return isqrt_exact(dx * dx + dy * dy);
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// the workgroup's total of v (every thread gets it; the same summation order in all of them)
__device__ __forceinline__ long long block_sum(long long v, long long* red) {
  v = wave_sum(v);
  __syncthreads();   // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = 0;
#pragma unroll
  for (int w = 0; w < ACT_WAVES; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(ACT_THREADS) void k_activity(const int* __restrict__ J, const long long* __restrict__ offsets,
                                                          long long n_frames, int rest_given, int* __restrict__ rest,
                                                          int* __restrict__ out, int* __restrict__ status) {
  __shared__ unsigned hist[ACT_SEL][256];   // 32 KiB
  __shared__ unsigned prefix[ACT_SEL];
  __shared__ long long rank[ACT_SEL];
  __shared__ long long red[ACT_WAVES];
  __shared__ int rp[ACT_RP];

  const int f = blockIdx.x, tid = threadIdx.x;
  const long long o0 = offsets[f], o1 = offsets[f + 1];
  if (o0 < 0 || o1 < o0 || o1 > n_frames) {   // the host never sends such offsets; the file is reported, nothing is written
    if (tid == 0) status[f] = 2;
    return;
  }
  const long long n = o1 - o0;
  const int* Jf = J + o0 * ACT_COLS;
  int* Of = out + o0 * ACT_OUT;

  // 1. velocities and their sums
  long long sl = 0, sr = 0;
  for (long long i = tid; i < n; i += ACT_THREADS) {
    int vl = 0, vr = 0;
    if (i >= 4) {
      const int* p = Jf + i * ACT_COLS;
      const int* q = p - ACT_COLS;
      vl = dist_floor(p[LH], p[LH + 1], q[LH], q[LH + 1]);
      vr = dist_floor(p[RH], p[RH + 1], q[RH], q[RH + 1]);
    }
    Of[i * ACT_OUT] = vl;
    Of[i * ACT_OUT + 1] = vr;
    sl += vl;
    sr += vr;
  }
  sl = block_sum(sl, red);
  sr = block_sum(sr, red);

  // 2. the low-velocity mask (v < sum / n  <=>  v n < sum for integers, sums < 2^53) and its count
  long long cnt = 0;
  for (long long i = tid; i < n; i += ACT_THREADS) {
    const long long vl = Of[i * ACT_OUT], vr = Of[i * ACT_OUT + 1];   // this thread's own stores
    const int low = vl * n < sl && vr * n < sr;
    Of[i * ACT_OUT + 2] = low;
    cnt += low;
  }
  cnt = block_sum(cnt, red);
  const int st = cnt == 0 ? 1 : 0;

  if (rest_given) {
    if (tid < ACT_RP) rp[tid] = rest[(size_t)f * ACT_RP + tid];
  } else if (st) {
    if (tid < ACT_RP) rest[(size_t)f * ACT_RP + tid] = 0;
  } else {
    // radix select of the order statistics (cnt - 1) / 2 and cnt / 2 of every column over the low frames
    const int nsel = (cnt & 1) ? ACT_RP : ACT_SEL;
    if (tid < ACT_SEL) {
      prefix[tid] = 0;
      rank[tid] = tid < ACT_RP ? (cnt - 1) / 2 : cnt / 2;
    }
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      for (int e = tid; e < ACT_SEL * 256; e += ACT_THREADS) (&hist[0][0])[e] = 0;
      __syncthreads();
      for (long long i = tid; i < n; i += ACT_THREADS) {
        if (!Of[i * ACT_OUT + 2]) continue;
        const int* p = Jf + i * ACT_COLS + 4;
        for (int c = 0; c < ACT_RP; ++c) {
          const unsigned key = (unsigned)p[c] ^ 0x80000000u;
          for (int s = c; s < nsel; s += ACT_RP)
            if (pass == 0 || (key >> (shift + 8)) == (prefix[s] >> (shift + 8))) atomicAdd(&hist[s][(key >> shift) & 255u], 1u);
        }
      }
      __syncthreads();
      if (tid < nsel) {
        const long long k = rank[tid];
        long long cum = 0;
        int d = 0;
        for (; d < 255; ++d) {
          const long long h = hist[tid][d];
          if (cum + h > k) break;
          cum += h;
        }
        rank[tid] = k - cum;
        prefix[tid] |= (unsigned)d << shift;
      }
      __syncthreads();
    }
    if (tid < ACT_RP) {
      const long long a = (int)(prefix[tid] ^ 0x80000000u);
      const long long b = nsel == ACT_SEL ? (int)(prefix[tid + ACT_RP] ^ 0x80000000u) : a;
      const int m = (int)((a + b) / 2);   // pandas' median of an even count, then int(): truncated toward zero
      rp[tid] = m;
      rest[(size_t)f * ACT_RP + tid] = m;
    }
  }
  __syncthreads();

  // 3. distances from the rest position (zeros for a file without one)
  const bool have = rest_given || !st;
  for (long long i = tid; i < n; i += ACT_THREADS) {
    int dl = 0, dr = 0;
    if (have && i >= 4) {
      const int* p = Jf + i * ACT_COLS;
      dl = dist_floor(rp[RP_LH], rp[RP_LH + 1], p[LH], p[LH + 1]);
      dr = dist_floor(rp[RP_RH], rp[RP_RH + 1], p[RH], p[RH + 1]);
    }
    Of[i * ACT_OUT + 3] = dl;
    Of[i * ACT_OUT + 4] = dr;
  }
  if (tid == 0) status[f] = st;
}

}  // namespace

extern "C" int mgr_skeletal_activity(mgr_ctx* c, const int32_t* joints, const int64_t* offsets, int n_files, long long n_frames,
                                     int rest_given, int32_t* rest, int32_t* out, int32_t* status) {
  MGR_REQUIRE(c, "null argument");
  MGR_REQUIRE(n_files >= 0 && n_files <= MGR_ACTIVITY_MAX_FILES, "n_files must be in [0, %d]", MGR_ACTIVITY_MAX_FILES);
  MGR_REQUIRE(n_frames >= 0 && n_frames <= MGR_ACTIVITY_MAX_FRAMES, "n_frames must be in [0, %lld]", (long long)MGR_ACTIVITY_MAX_FRAMES);
  if (n_files == 0) return 0;
  MGR_REQUIRE(offsets && rest && status && (n_frames == 0 || (joints && out)), "null argument");
  hipStream_t st = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_MISC);
  hipLaunchKernelGGL(k_activity, dim3((unsigned)n_files), dim3(ACT_THREADS), 0, st, (const int*)joints, (const long long*)offsets,
                     n_frames, rest_given ? 1 : 0, (int*)rest, (int*)out, (int*)status);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}
