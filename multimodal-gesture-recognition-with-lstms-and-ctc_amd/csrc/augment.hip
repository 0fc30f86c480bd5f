// Train-time sequence augmentation: a length-preserving piecewise-linear time warp shared by the streams of a sample,
// time / feature masks per stream (SpecAugment), at most one blanked stream per sample (ModDrop), and the GaussianNoise of
// k_add_noise, in ONE pass over a stream's [B, T, F] input: Y = noise(mask(warp(X))).
//   mgr_augment_plan   one thread per sample: the int32 plan row (layout and draw order: mgr.h).  Integers only.
//   mgr_augment_apply  one workgroup per (sample, range of frames): the frames are resolved once each into a small LDS table (source
//                      row, interpolation weight, blanked or not), then one thread per PAIR of flat output elements (the noise
//                      pairing) walks the range - a wave stores 512 contiguous bytes, its loads are one or two rows of X per
//                      warped frame.
// Neither call uses atomics or a workspace.
#include "common.h"
#include "noise.h"

namespace {

constexpr int kBlock = 256;

struct StreamCfg {
  int F[MGR_AUGMENT_MAX_STREAMS], nt[MGR_AUGMENT_MAX_STREAMS], wt[MGR_AUGMENT_MAX_STREAMS], nf[MGR_AUGMENT_MAX_STREAMS],
      wf[MGR_AUGMENT_MAX_STREAMS];
};

// integer in [lo, hi] from one 32-bit draw
__device__ static inline int draw_int(uint32_t u, int lo, int hi) {
  return lo + (int)(((uint64_t)u * (uint64_t)(uint32_t)(hi - lo + 1)) >> 32);
}

__global__ void k_augment_plan(int B, int T, int S, int K, int D, int n_t, int n_f, StreamCfg cfg, uint32_t drop_thresh, uint64_t seed,
                               int len, int32_t* __restrict__ plan) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int32_t* row = plan + (size_t)b * len;
  const uint64_t base = (uint64_t)b * (uint64_t)len;     // entry p of the row draws at index base + p
  // warp targets q_0 .. q_K
  for (int j = 0; j <= K; ++j) {
    int q = (int)((long long)j * (T - 1) / K);
    if (j > 0 && j < K && D > 0) q += draw_int(mgr_rand_u32(seed, base + j), -D, D);
    row[j] = q;
  }
  // the dropped stream
  int drop = -1;
  if (drop_thresh > 0) {
    const uint32_t r = mgr_rand_u32(seed, base + K + 1) >> 8;
    if (r < drop_thresh) drop = (int)(((uint64_t)r * (uint64_t)S) / drop_thresh);
  }
  row[K + 1] = drop;
  // masks: per stream n_t (start, width) pairs along time, then n_f along the features; a stream with fewer masks than the row has
  // slots leaves the rest empty (width 0) and their draws unused
  int p = K + 2;
  for (int s = 0; s < S; ++s) {
    for (int m = 0; m < n_t + n_f; ++m, p += 2) {
      const bool time = m < n_t;
      const int used = time ? cfg.nt[s] : cfg.nf[s];
      const int wmax = time ? cfg.wt[s] : cfg.wf[s];
      const int axis = time ? T : cfg.F[s];
      int start = 0, width = 0;
      if ((time ? m : m - n_t) < used) {
        width = draw_int(mgr_rand_u32(seed, base + p + 1), 0, wmax);
        start = draw_int(mgr_rand_u32(seed, base + p), 0, axis - width);
      }
      row[p] = start;
      row[p + 1] = width;
    }
  }
}

// what frame (b, t) of a stream's output is made of: source rows i0 (and i0 + 1 when rem != 0) of X, and whether the frame is blanked
struct Frame {
  int i0, rem, den;
  bool blank;
};

__device__ static inline Frame resolve_frame(const int32_t* __restrict__ row, int t, int T, int K, int n_t, int n_f, int stream) {
  Frame fr;
  // the first segment with t <= q_{j+1}: the targets increase, so j is the number of inner targets below t (independent loads,
  // no loop-carried exit; whatever the row holds, j stays below K)
  int j = 0;
  for (int m = 1; m < K; ++m) j += row[m] < t;
  const int q0 = row[j], q1 = row[j + 1];
  const int a0 = j * (T - 1) / K, a1 = (j + 1) * (T - 1) / K;     // (K <= 16, T < 2^15: 32 bits)
  fr.den = q1 - q0;
  if (fr.den > 0) {
    const int num = (t - q0) * (a1 - a0);
    fr.i0 = a0 + num / fr.den;
    fr.rem = num % fr.den;
  } else {                                      // (T == 1: the one frame is itself)
    fr.i0 = a0;
    fr.rem = 0;
  }
  // (a row mgr_augment_plan wrote never gets here out of range; a row that is not one must not send a read outside X)
  if (fr.i0 < 0) fr.i0 = 0;
  if (fr.i0 >= T - 1) fr.i0 = T - 1, fr.rem = 0;
  fr.blank = row[K + 1] == stream;
  const int32_t* tm = row + K + 2 + stream * 2 * (n_t + n_f);
  for (int m = 0; m < n_t; ++m) {
    const int st = tm[2 * m], w = tm[2 * m + 1];
    fr.blank = fr.blank || (t >= st && t < st + w);
  }
  return fr;
}

// x0 + (rem / den) (x1 - x0) in four roundings: numpy float32 gives the same bits.  __fmul_rn / __fadd_rn do not pin that here:
// the headers define them as the plain operators, inlined they are a multiply and an add like any other, which the compiler may
// fuse.  So the operators are written out where contraction is OFF.
__device__ static inline float lerp_unfused(float x0, float x1, int rem, int den) {
#pragma clang fp contract(off)
  const float frac = __fdiv_rn((float)rem, (float)den);     // (correctly rounded)
  const float d = x1 - x0;
  const float p = frac * d;
  return x0 + p;
}

// What the elements of one output frame need, resolved ONCE per frame by a thread of the workgroup that owns the frame, kept in LDS
struct FrameEntry {
  size_t src;      // flat index of X[b, i0, 0]
  int rem, den;    // rem != 0: interpolate towards row i0 + 1 with weight rem / den
  int blank;       // the whole frame becomes `fill` (time mask / dropped stream)
  int next;        // 1: the frame belongs to the NEXT sample (its feature masks are the second set)
};

constexpr int kFramesMax = 255;     // frames per workgroup (plus the one frame behind them that a noise pair may reach into)

// One workgroup per (sample b, range of frames [t0, t1)): the flat elements [(b T + t0) F, (b T + t1) F).  It owns the noise pairs
// whose FIRST element lies in that range - so the second element of its last pair may be the first element of frame t1, or of
// frame 0 of sample b + 1 (T F odd), which is entry t1 - t0 of its table - and every element has exactly one owner.  The segment
// search, the integer division for i0 and the time masks happen once per frame; an element pays one division by F per pair, its
// feature masks out of LDS, one or two loads of X, its noise and a store.
__global__ __launch_bounds__(kBlock) void k_augment_apply(const float* __restrict__ X, float* __restrict__ Y, const int32_t* __restrict__ plan,
                                                          size_t n, int B, int T, int F, int FR, int nchunk, int len, int K, int n_t,
                                                          int n_f, int stream, float fill, float stddev, uint64_t seed) {
  __shared__ FrameEntry fe[kFramesMax + 1];
  __shared__ int fmask[2][2 * MGR_AUGMENT_MAX_MASKS];
  const int b = blockIdx.x / nchunk, t0 = (blockIdx.x % nchunk) * FR;
  const int t1 = min(t0 + FR, T);
  const int nfr = t1 - t0;                                          // <= kFramesMax
  const size_t s = ((size_t)b * T + t0) * (size_t)F, e_end = s + (size_t)nfr * F;
  const bool has_next = e_end < n;                                   // there is a frame behind the range (this sample's or the next's)
  for (int k = threadIdx.x; k < nfr + (has_next ? 1 : 0); k += blockDim.x) {
    int tt = t0 + k, bb = b;
    if (tt == T) tt = 0, ++bb;                                       // (only k == nfr, only with has_next: bb < B)
    const int32_t* row = plan + (size_t)bb * len;
    const Frame fr = resolve_frame(row, tt, T, K, n_t, n_f, stream);
    FrameEntry en;
    en.src = ((size_t)bb * T + (size_t)fr.i0) * (size_t)F;
    en.rem = fr.rem, en.den = fr.den, en.blank = fr.blank, en.next = bb - b;
    fe[k] = en;
  }
  for (int k = threadIdx.x; k < 2 * 2 * n_f; k += blockDim.x) {
    const int which = k / (2 * n_f), m = k % (2 * n_f);
    const int bb = b + which;
    fmask[which][m] = bb < B ? plan[(size_t)bb * len + K + 2 + stream * 2 * (n_t + n_f) + 2 * n_t + m] : 0;
  }
  __syncthreads();
  auto value = [&](int k, int f) -> float {
    const FrameEntry en = fe[k];
    bool blank = en.blank != 0;
    const int* fm = fmask[en.next];
    for (int m = 0; m < n_f; ++m) blank = blank || (f >= fm[2 * m] && f < fm[2 * m] + fm[2 * m + 1]);
    if (blank) return fill;
    const float* x = X + en.src + f;
    const float x0 = x[0];
    if (en.rem == 0) return x0;                   // verbatim: the row behind i0 is not read (at t = T - 1 there is none)
    return lerp_unfused(x0, x[F], en.rem, en.den);
  };
  const size_t i_lo = (s + 1) / 2, i_hi = (e_end + 1) / 2;           // pairs whose first element 2i lies in [s, e_end)
  for (size_t i = i_lo + threadIdx.x; i < i_hi; i += blockDim.x) {
    const size_t e = 2 * i;
    const unsigned l = (unsigned)(e - s);                            // < nfr F <= 2^31
    int k = (int)(l / (unsigned)F), f = (int)(l - (unsigned)k * (unsigned)F);
    float v0 = value(k, f), v1 = 0.f;
    const bool two = e + 1 < n;
    if (two) {
      if (++f == F) f = 0, ++k;                                      // (k == nfr: the frame behind the range; it exists, e + 1 < n)
      v1 = value(k, f);
    }
    if (stddev > 0.f) {
      float rad, sn, cs;
      mgr_noise_pair(seed, i, stddev, &rad, &cs, &sn);
      v0 = mgr_noise_add(v0, rad, cs);
      v1 = mgr_noise_add(v1, rad, sn);
    }
    Y[e] = v0;
    if (two) Y[e + 1] = v1;
  }
}

static int check_shape(int S, int K, int n_t, int n_f) {
  return S >= 1 && S <= MGR_AUGMENT_MAX_STREAMS && K >= 1 && K <= MGR_AUGMENT_MAX_SEGMENTS && n_t >= 0 && n_t <= MGR_AUGMENT_MAX_MASKS &&
         n_f >= 0 && n_f <= MGR_AUGMENT_MAX_MASKS;
}

}  // namespace

extern "C" {

int mgr_augment_plan_len(int S, int K, int n_t, int n_f) {
  if (!check_shape(S, K, n_t, n_f)) return 0;
  return K + 2 + S * 2 * (n_t + n_f);
}

int mgr_augment_plan(mgr_ctx* c, int B, int T, int S, int K, int D, int n_t, int n_f, const int32_t* stream_cfg, uint32_t drop_thresh,
                     uint64_t seed, int32_t* plan) {
  MGR_REQUIRE(c && stream_cfg && plan, "null argument");
  MGR_REQUIRE(check_shape(S, K, n_t, n_f), "S = %d (1 .. %d), K = %d (1 .. %d), masks %d / %d (0 .. %d)", S, MGR_AUGMENT_MAX_STREAMS, K,
              MGR_AUGMENT_MAX_SEGMENTS, n_t, n_f, MGR_AUGMENT_MAX_MASKS);
  MGR_REQUIRE(B > 0 && T > 0 && T <= MGR_AUGMENT_MAX_T, "bad shape B=%d T=%d (T <= %d)", B, T, MGR_AUGMENT_MAX_T);
  MGR_REQUIRE(D >= 0, "max_shift = %d", D);
  if (K > 1 && D > 0) {
    int shortest = T;
    for (int j = 0; j < K; ++j) {
      const int seg = (int)((long long)(j + 1) * (T - 1) / K - (long long)j * (T - 1) / K);
      if (seg < shortest) shortest = seg;
    }
    MGR_REQUIRE(2 * D < shortest, "max_shift = %d: 2 D must stay below the shortest segment (%d frames)", D, shortest);
  } else if (K > 1) {
    MGR_REQUIRE(T - 1 >= K, "K = %d segments over T = %d frames", K, T);
  }
  MGR_REQUIRE(drop_thresh < (1u << 24), "drop_thresh = %u: below 2^24 (stream_drop < 1)", drop_thresh);
  MGR_REQUIRE(drop_thresh == 0 || S > 1, "a stream is dropped only where there are several");
  StreamCfg cfg;
  memset(&cfg, 0, sizeof cfg);
  for (int s = 0; s < S; ++s) {
    const int32_t* r = stream_cfg + s * MGR_AUGMENT_STREAM_COLS;
    MGR_REQUIRE(r[0] >= 1 && r[1] >= 0 && r[1] <= n_t && r[3] >= 0 && r[3] <= n_f, "stream %d: F = %d, masks %d / %d of %d / %d slots", s,
                r[0], r[1], r[3], n_t, n_f);
    MGR_REQUIRE(r[2] >= 0 && r[2] <= T && r[4] >= 0 && r[4] <= r[0], "stream %d: mask widths %d / %d beyond T = %d / F = %d", s, r[2], r[4],
                T, r[0]);
    cfg.F[s] = r[0], cfg.nt[s] = r[1], cfg.wt[s] = r[2], cfg.nf[s] = r[3], cfg.wf[s] = r[4];
  }
  const int len = mgr_augment_plan_len(S, K, n_t, n_f);
  mgr_prof_begin(c, MGR_K_MISC);
  hipLaunchKernelGGL(k_augment_plan, dim3((B + 63) / 64), dim3(64), 0, mgr_stream(c), B, T, S, K, D, n_t, n_f, cfg, drop_thresh, seed, len,
                     plan);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}

int mgr_augment_apply(mgr_ctx* c, const float* X, float* Y, const int32_t* plan, int B, int T, int F, int S, int K, int n_t, int n_f,
                      int stream, float fill, float stddev, uint64_t seed) {
  MGR_REQUIRE(c && X && Y && plan, "null argument");
  MGR_REQUIRE(X != Y, "in place: a warped frame reads rows other elements overwrite");
  MGR_REQUIRE(check_shape(S, K, n_t, n_f), "S = %d (1 .. %d), K = %d (1 .. %d), masks %d / %d (0 .. %d)", S, MGR_AUGMENT_MAX_STREAMS, K,
              MGR_AUGMENT_MAX_SEGMENTS, n_t, n_f, MGR_AUGMENT_MAX_MASKS);
  MGR_REQUIRE(B > 0 && T > 0 && T <= MGR_AUGMENT_MAX_T && F > 0, "bad shape B=%d T=%d F=%d (T <= %d)", B, T, F, MGR_AUGMENT_MAX_T);
  MGR_REQUIRE((long long)T * F < (1LL << 31), "T F = %lld: below 2^31", (long long)T * F);
  MGR_REQUIRE(K == 1 || T - 1 >= K, "K = %d segments over T = %d frames", K, T);
  MGR_REQUIRE(stream >= 0 && stream < S, "stream %d of %d", stream, S);
  MGR_REQUIRE(stddev >= 0.f, "stddev = %f", stddev);
  const size_t n = (size_t)B * T * F;
  // frames per workgroup: about 4096 elements (16 per thread), at least one frame, at most the table's
  int FR = 4096 / F;
  FR = FR < 1 ? 1 : (FR > kFramesMax ? kFramesMax : FR);
  const int nchunk = (T + FR - 1) / FR;
  MGR_REQUIRE((long long)B * nchunk < (1LL << 31), "B = %d x %d frame ranges: too many workgroups", B, nchunk);
  mgr_prof_begin(c, MGR_K_MISC);
  hipLaunchKernelGGL(k_augment_apply, dim3((unsigned)(B * nchunk)), dim3(kBlock), 0, mgr_stream(c), X, Y, plan, n, B, T, F, FR, nchunk,
                     mgr_augment_plan_len(S, K, n_t, n_f), K, n_t, n_f, stream, fill, stddev, seed);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}

}  // extern "C"
