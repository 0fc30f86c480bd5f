// TimeDistributed CNN front-end of the RGB network (rgb_network/cnn_lstm.py): per frame, valid Conv2D + bias + ReLU + 2x2 / stride 2
// floor max-pool, channels-last.  Forward, backward data (through the pool, the ReLU and the transposed convolution) and backward
// weights / bias, all in exact f32.  The weight gradient is deterministic: fixed-order per-chunk partial sums (f64) in a
// workspace, then a fixed-order pass over the chunks - no atomics.  The weight gradient of the GEMM-shaped layers (conv_3, conv_5) runs
// as an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact f32); the forward and the data gradient are direct f32 kernels on the vector ALUs.
//
// Layouts (Keras, channels-last): X [N][Hin][Win][Cin], W [ks][ks][Cin][Cout], b [Cout], pooled Y / dY [N][Hp][Wp][Cout] with
// Hp = (Hin - ks + 1) / 2 (floor: a last odd conv row / column is dropped), code [N][Hp][Wp][Cout] (uint8): the window position
// (dy * 2 + dx) of the first maximum in row-major order, or MGR_CONV_NO_GRAD when that maximum is a ReLU zero.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kCpt = 4;              // output channels per thread in the forward kernel
constexpr int kChunks = 256;         // frame chunks of the weight gradient (its partial sums: kChunks x (K * Cout + Cout) doubles)
constexpr size_t kMaxLds = 64 * 1024;
constexpr uint8_t kNoGrad = 0xFF;

struct Shape {
  int N, Hin, Win, Cin, Cout, Hp, Wp;
};

static inline int frame_grid(int N) { return N < 8192 ? N : 8192; }

// One workgroup per frame (grid-stride over frames): the frame is staged in LDS, each thread forms the four conv outputs of one
// pooling window for kCpt consecutive channels (weights read as float4 rows of W, L1/L2-resident), then bias, ReLU, max.
template <int KS>
__global__ void __launch_bounds__(kBlock) k_conv_pool_fwd(const float* __restrict__ X, const float* __restrict__ Wt, const float* __restrict__ bias,
                                                          Shape s, float* __restrict__ Y, uint8_t* __restrict__ code) {
  extern __shared__ float xs[];
  const int fsz = s.Hin * s.Win * s.Cin;
  const int cg = s.Cout / kCpt;
  const int nout = s.Hp * s.Wp * cg;
  const int rowx = s.Win * s.Cin;
  for (int n = blockIdx.x; n < s.N; n += gridDim.x) {
    const float* xf = X + (size_t)n * fsz;
    __syncthreads();
    for (int i = threadIdx.x; i < fsz; i += blockDim.x) xs[i] = xf[i];
    __syncthreads();
    for (int o = threadIdx.x; o < nout; o += blockDim.x) {
      const int c0 = (o % cg) * kCpt;
      const int p = o / cg;
      const int pi = p / s.Wp, pj = p % s.Wp;
      float acc[4][kCpt];
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int q = 0; q < kCpt; ++q) acc[d][q] = 0.0f;
      const float* x0 = xs + (2 * pi) * rowx + (2 * pj) * s.Cin;
#pragma unroll
      for (int kh = 0; kh < KS; ++kh) {
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
          const float* xk = x0 + kh * rowx + kw * s.Cin;
          const float* wk = Wt + ((size_t)(kh * KS + kw) * s.Cin) * s.Cout + c0;
          for (int ci = 0; ci < s.Cin; ++ci) {
            const float4 w = *reinterpret_cast<const float4*>(wk + (size_t)ci * s.Cout);
            const float xv[4] = {xk[ci], xk[s.Cin + ci], xk[rowx + ci], xk[rowx + s.Cin + ci]};
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              acc[d][0] = fmaf(xv[d], w.x, acc[d][0]);
              acc[d][1] = fmaf(xv[d], w.y, acc[d][1]);
              acc[d][2] = fmaf(xv[d], w.z, acc[d][2]);
              acc[d][3] = fmaf(xv[d], w.w, acc[d][3]);
            }
          }
        }
      }
      const size_t ob = ((size_t)n * s.Hp * s.Wp + p) * s.Cout + c0;
#pragma unroll
      for (int q = 0; q < kCpt; ++q) {
        const float bq = bias[c0 + q];
        float best = fmaxf(acc[0][q] + bq, 0.0f);
        int arg = 0;
#pragma unroll
        for (int d = 1; d < 4; ++d) {
          const float v = fmaxf(acc[d][q] + bq, 0.0f);
          if (v > best) {       // strictly greater: the first maximum in row-major window order wins a tie
            best = v;
            arg = d;
          }
        }
        Y[ob + q] = best;
        code[ob + q] = best > 0.0f ? (uint8_t)arg : kNoGrad;   // a ReLU zero passes no gradient to any position of its window
      }
    }
  }
}

// dX[n][y][x][ci] = sum over (kh, kw, co) of dPre[n][y - kh][x - kw][co] * W[kh][kw][ci][co], where dPre (the gradient of the conv
// pre-activation) is the pooled gradient at the window position its code names and zero elsewhere.  One workgroup per frame: the
// frame's pooled gradient and codes are staged in LDS.
template <int KS>
__global__ void __launch_bounds__(kBlock) k_conv_pool_bwd_data(const float* __restrict__ dY, const uint8_t* __restrict__ code,
                                                               const float* __restrict__ Wt, Shape s, float* __restrict__ dX) {
  extern __shared__ float gs[];
  const int psz = s.Hp * s.Wp * s.Cout;
  uint8_t* cs = reinterpret_cast<uint8_t*>(gs + psz);
  const int fsz = s.Hin * s.Win * s.Cin;
  for (int n = blockIdx.x; n < s.N; n += gridDim.x) {
    __syncthreads();
    for (int i = threadIdx.x; i < psz; i += blockDim.x) {
      gs[i] = dY[(size_t)n * psz + i];
      cs[i] = code[(size_t)n * psz + i];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < fsz; e += blockDim.x) {
      const int ci = e % s.Cin;
      const int pix = e / s.Cin;
      const int y = pix / s.Win, x = pix % s.Win;
      float acc = 0.0f;
#pragma unroll
      for (int kh = 0; kh < KS; ++kh) {
        const int oy = y - kh;
        if (oy < 0 || oy >= 2 * s.Hp) continue;
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
          const int ox = x - kw;
          if (ox < 0 || ox >= 2 * s.Wp) continue;
          const uint8_t want = (uint8_t)((oy & 1) * 2 + (ox & 1));
          const int pb = ((oy >> 1) * s.Wp + (ox >> 1)) * s.Cout;
          const float* wk = Wt + ((size_t)(kh * KS + kw) * s.Cin + ci) * s.Cout;
          for (int co = 0; co < s.Cout; ++co)
            if (cs[pb + co] == want) acc = fmaf(gs[pb + co], wk[co], acc);
        }
      }
      dX[(size_t)n * fsz + e] = acc;
    }
  }
}

// Partial weight / bias gradients of frame chunk blockIdx.x: element e < K * Cout (K = ks * ks * Cin) is W[k][co] with k = e / Cout,
// e >= K * Cout is b[e - K * Cout].  Each thread owns EP elements of tile blockIdx.y and sums them over the chunk's frames (frames in
// order, each frame's pooled positions in order, per-frame sums in f32 folded into f64): a fixed order whatever the launch timing.
template <int KS, int EP>
__global__ void __launch_bounds__(kBlock) k_conv_pool_bwd_w_partial(const float* __restrict__ X, const float* __restrict__ dY,
                                                                    const uint8_t* __restrict__ code, Shape s, int per_chunk,
                                                                    double* __restrict__ part) {
  extern __shared__ float xs[];
  const int K = KS * KS * s.Cin;
  const int nE = K * s.Cout + s.Cout;
  const int fsz = s.Hin * s.Win * s.Cin;
  const int psz = s.Hp * s.Wp * s.Cout;
  const int rowx = s.Win * s.Cin;
  const int n0 = blockIdx.x * per_chunk;
  const int n1 = min(s.N, n0 + per_chunk);
  int co[EP], xoff[EP];
  bool isb[EP], live[EP];
  double tot[EP];
#pragma unroll
  for (int j = 0; j < EP; ++j) {
    const int e = (blockIdx.y * EP + j) * kBlock + threadIdx.x;
    live[j] = e < nE;
    isb[j] = e >= K * s.Cout;
    const int k = isb[j] ? 0 : e / s.Cout;
    co[j] = isb[j] ? e - K * s.Cout : e % s.Cout;
    if (!live[j]) co[j] = 0;
    const int ci = k % s.Cin, kk = k / s.Cin;
    xoff[j] = (kk / KS) * rowx + (kk % KS) * s.Cin + ci;
    tot[j] = 0.0;
  }
  for (int n = n0; n < n1; ++n) {
    __syncthreads();
    for (int i = threadIdx.x; i < fsz; i += blockDim.x) xs[i] = X[(size_t)n * fsz + i];
    __syncthreads();
    const float* g = dY + (size_t)n * psz;
    const uint8_t* cd = code + (size_t)n * psz;
    float acc[EP];
#pragma unroll
    for (int j = 0; j < EP; ++j) acc[j] = 0.0f;
    for (int p = 0; p < s.Hp * s.Wp; ++p) {
      const int pi = p / s.Wp, pj = p % s.Wp;
#pragma unroll
      for (int j = 0; j < EP; ++j) {
        const uint8_t c = cd[p * s.Cout + co[j]];
        if (!live[j] || c == kNoGrad) continue;
        const float gv = g[p * s.Cout + co[j]];
        const int oy = 2 * pi + (c >> 1), ox = 2 * pj + (c & 1);
        const float xv = isb[j] ? 1.0f : xs[oy * rowx + ox * s.Cin + xoff[j]];
        acc[j] = fmaf(xv, gv, acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < EP; ++j) tot[j] += (double)acc[j];
  }
#pragma unroll
  for (int j = 0; j < EP; ++j) {
    const int e = (blockIdx.y * EP + j) * kBlock + threadIdx.x;
    if (e < nE) part[(size_t)blockIdx.x * nE + e] = tot[j];
  }
}

typedef float mgr_conv_f4 __attribute__((ext_vector_type(4)));
constexpr int kTpw = 4;   // 16x16 output tiles per wave of the MFMA weight gradient

// The weight gradient of a GEMM-shaped layer (K = ks*ks*Cin and Cout multiples of 16: conv_3, conv_5) as an implicit GEMM on
// v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation): dW[k][co] = sum over m of A[k][m] * B[m][co], m = (pooled position p,
// window position d), A[k][m] = the input under tap k at conv output (p, d) (the frame staged in LDS), B[m][co] = the pooled gradient
// where code routes it to d, else 0.  Each wave owns kTpw output tiles of tile group blockIdx.y; per frame the accumulators are folded
// into f64 sums - frames in order, m in order: the same fixed order whatever the launch timing.  blockIdx.y == 0 also forms db.
template <int KS>
__global__ void __launch_bounds__(kBlock) k_conv_pool_bwd_w_mfma(const float* __restrict__ X, const float* __restrict__ dY,
                                                                 const uint8_t* __restrict__ code, Shape s, int per_chunk,
                                                                 double* __restrict__ part) {
  extern __shared__ float xs[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = KS * KS * s.Cin;
  const int nkt = K / 16, ntiles = nkt * (s.Cout / 16);
  const int nE = K * s.Cout + s.Cout;
  const int fsz = s.Hin * s.Win * s.Cin;
  const int psz = s.Hp * s.Wp * s.Cout;
  const int rowx = s.Win * s.Cin;
  const int M = 4 * s.Hp * s.Wp;
  const int n0 = blockIdx.x * per_chunk;
  const int n1 = min(s.N, n0 + per_chunk);
  const int tile0 = (blockIdx.y * (kBlock / 64) + wave) * kTpw;     // (wave-uniform: so is every tile test below)
  int xo[kTpw], co[kTpw];
  double tot[kTpw][4];
#pragma unroll
  for (int t = 0; t < kTpw; ++t) {
    const int tile = min(tile0 + t, ntiles - 1);
    const int k = (tile % nkt) * 16 + (lane & 15);                  // A row of this lane
    const int kk = k / s.Cin;
    xo[t] = (kk / KS) * rowx + (kk % KS) * s.Cin + k % s.Cin;
    co[t] = (tile / nkt) * 16 + (lane & 15);                        // B / D column of this lane
#pragma unroll
    for (int r = 0; r < 4; ++r) tot[t][r] = 0.0;
  }
  for (int n = n0; n < n1; ++n) {
    __syncthreads();
    for (int i = threadIdx.x; i < fsz; i += blockDim.x) xs[i] = X[(size_t)n * fsz + i];
    __syncthreads();
    const float* g = dY + (size_t)n * psz;
    const uint8_t* cd = code + (size_t)n * psz;
    mgr_conv_f4 acc[kTpw];
#pragma unroll
    for (int t = 0; t < kTpw; ++t) acc[t] = mgr_conv_f4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int m0 = 0; m0 < M; m0 += 4) {
      const int mm = m0 + (lane >> 4);
      const int p = mm >> 2, d = mm & 3;
      const int base = (2 * (p / s.Wp) + (d >> 1)) * rowx + (2 * (p % s.Wp) + (d & 1)) * s.Cin;
#pragma unroll
      for (int t = 0; t < kTpw; ++t) {
        if (tile0 + t >= ntiles) break;
        const float a = xs[base + xo[t]];
        const int gi = p * s.Cout + co[t];
        const float b = cd[gi] == (uint8_t)d ? g[gi] : 0.0f;
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < kTpw; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) tot[t][r] += (double)acc[t][r];
  }
#pragma unroll
  for (int t = 0; t < kTpw; ++t) {
    const int tile = tile0 + t;
    if (tile >= ntiles) break;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = (tile % nkt) * 16 + (lane >> 4) * 4 + r;         // D row of this lane
      part[(size_t)blockIdx.x * nE + (size_t)k * s.Cout + co[t]] = tot[t][r];
    }
  }
  if (blockIdx.y != 0) return;
  for (int c = threadIdx.x; c < s.Cout; c += kBlock) {   // (Cout may exceed the block: every channel gets its partial sum)
    double tb = 0.0;
    for (int n = n0; n < n1; ++n) {
      float a = 0.0f;
      for (int p = 0; p < s.Hp * s.Wp; ++p)
        if (code[(size_t)n * psz + p * s.Cout + c] != kNoGrad) a += dY[(size_t)n * psz + p * s.Cout + c];
      tb += (double)a;
    }
    part[(size_t)blockIdx.x * nE + (size_t)K * s.Cout + c] = tb;
  }
}

// dW / db = the chunks' partial sums added in chunk order.
__global__ void k_conv_pool_bwd_w_final(const double* __restrict__ part, int nchunk, int K, int Cout, float* __restrict__ dW,
                                        float* __restrict__ db) {
  const int nE = K * Cout + Cout;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nE; e += gridDim.x * blockDim.x) {
    double t = 0.0;
    for (int c = 0; c < nchunk; ++c) t += part[(size_t)c * nE + e];
    if (e < K * Cout)
      dW[e] = (float)t;
    else
      db[e - K * Cout] = (float)t;
  }
}

int check_shape(int N, int Hin, int Win, int Cin, int ks, int Cout, Shape* s) {
  MGR_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && Cout % kCpt == 0, "conv: bad shape (N %d, Cin %d, Cout %d: Cout must be a multiple of %d)", N, Cin,
              Cout, kCpt);
  MGR_REQUIRE(ks == 4 || ks == 5, "conv: kernel size %d (4 or 5 are built)", ks);
  MGR_REQUIRE(Hin >= ks + 1 && Win >= ks + 1, "conv: input %dx%d too small for a %dx%d kernel and a 2x2 pool", Hin, Win, ks, ks);
  *s = Shape{N, Hin, Win, Cin, Cout, (Hin - ks + 1) / 2, (Win - ks + 1) / 2};
  return 0;
}

int chunks_of(int N) { return N < kChunks ? N : kChunks; }

}  // namespace

extern "C" {

int mgr_conv_pool_fwd(mgr_ctx* c, const float* X, int N, int Hin, int Win, int Cin, const float* W, const float* b, int ks, int Cout, float* Y,
                      uint8_t* code) {
  MGR_REQUIRE(c && X && W && b && Y && code, "null argument");
  MGR_REQUIRE(((uintptr_t)W & 15) == 0, "conv: W must be 16-byte aligned");
  Shape s;
  if (int r = check_shape(N, Hin, Win, Cin, ks, Cout, &s)) return r;
  const size_t lds = (size_t)Hin * Win * Cin * sizeof(float);
  MGR_REQUIRE(lds <= kMaxLds, "conv: a %dx%dx%d frame does not fit the LDS stage", Hin, Win, Cin);
  if (ks == 4)
    hipLaunchKernelGGL(k_conv_pool_fwd<4>, dim3(frame_grid(N)), dim3(kBlock), lds, mgr_stream(c), X, W, b, s, Y, code);
  else
    hipLaunchKernelGGL(k_conv_pool_fwd<5>, dim3(frame_grid(N)), dim3(kBlock), lds, mgr_stream(c), X, W, b, s, Y, code);
  MGR_LAUNCH_CHECK();
  return 0;
}

int mgr_conv_pool_bwd_data(mgr_ctx* c, const float* dY, const uint8_t* code, const float* W, int N, int Hin, int Win, int Cin, int ks,
                           int Cout, float* dX) {
  MGR_REQUIRE(c && dY && code && W && dX, "null argument");
  Shape s;
  if (int r = check_shape(N, Hin, Win, Cin, ks, Cout, &s)) return r;
  const size_t lds = (size_t)s.Hp * s.Wp * Cout * (sizeof(float) + 1);
  MGR_REQUIRE(lds <= kMaxLds, "conv: the pooled gradient of a frame (%dx%dx%d) does not fit the LDS stage", s.Hp, s.Wp, Cout);
  if (ks == 4)
    hipLaunchKernelGGL(k_conv_pool_bwd_data<4>, dim3(frame_grid(N)), dim3(kBlock), lds, mgr_stream(c), dY, code, W, s, dX);
  else
    hipLaunchKernelGGL(k_conv_pool_bwd_data<5>, dim3(frame_grid(N)), dim3(kBlock), lds, mgr_stream(c), dY, code, W, s, dX);
  MGR_LAUNCH_CHECK();
  return 0;
}

size_t mgr_conv_pool_bwd_weights_ws_bytes(int N, int Hin, int Win, int Cin, int ks, int Cout) {
  if (N <= 0 || Cin <= 0 || Cout <= 0 || ks <= 0) return 0;
  const size_t nE = (size_t)ks * ks * Cin * Cout + Cout;
  return (size_t)chunks_of(N) * nE * sizeof(double);
}

int mgr_conv_pool_bwd_weights(mgr_ctx* c, const float* X, const float* dY, const uint8_t* code, int N, int Hin, int Win, int Cin, int ks,
                              int Cout, float* dW, float* db, void* ws, size_t ws_bytes) {
  MGR_REQUIRE(c && X && dY && code && dW && db && ws, "null argument");
  mgr_planes_forget_range(c, ws, ws_bytes);   // (this call writes its workspace: kept weight planes in it are gone)
  Shape s;
  if (int r = check_shape(N, Hin, Win, Cin, ks, Cout, &s)) return r;
  const size_t need = mgr_conv_pool_bwd_weights_ws_bytes(N, Hin, Win, Cin, ks, Cout);
  MGR_REQUIRE(ws_bytes >= need, "conv: weight-gradient workspace of %zu bytes, %zu needed", ws_bytes, need);
  const size_t lds = (size_t)Hin * Win * Cin * sizeof(float);
  MGR_REQUIRE(lds <= kMaxLds, "conv: a %dx%dx%d frame does not fit the LDS stage", Hin, Win, Cin);
  const int K = ks * ks * Cin;
  const int nE = K * Cout + Cout;
  const int nchunk = chunks_of(N);
  const int per = (N + nchunk - 1) / nchunk;
  double* part = static_cast<double*>(ws);
  if (K % 16 == 0 && Cout % 16 == 0) {
    // GEMM-shaped layers (conv_3, conv_5): implicit GEMM on the f32 MFMA, 16 output tiles per workgroup
    const int ntiles = (K / 16) * (Cout / 16);
    dim3 grid(nchunk, (ntiles + 4 * kTpw - 1) / (4 * kTpw));
    if (ks == 4)
      hipLaunchKernelGGL(k_conv_pool_bwd_w_mfma<4>, grid, dim3(kBlock), lds, mgr_stream(c), X, dY, code, s, per, part);
    else
      hipLaunchKernelGGL(k_conv_pool_bwd_w_mfma<5>, grid, dim3(kBlock), lds, mgr_stream(c), X, dY, code, s, per, part);
  } else if (nE <= 2 * kBlock * 2) {
    // (the small first layer, K = 25: the vector form, two elements per thread)
    dim3 grid(nchunk, (nE + 2 * kBlock - 1) / (2 * kBlock));
    if (ks == 4)
      hipLaunchKernelGGL((k_conv_pool_bwd_w_partial<4, 2>), grid, dim3(kBlock), lds, mgr_stream(c), X, dY, code, s, per, part);
    else
      hipLaunchKernelGGL((k_conv_pool_bwd_w_partial<5, 2>), grid, dim3(kBlock), lds, mgr_stream(c), X, dY, code, s, per, part);
  } else {
    dim3 grid(nchunk, (nE + 8 * kBlock - 1) / (8 * kBlock));
    if (ks == 4)
      hipLaunchKernelGGL((k_conv_pool_bwd_w_partial<4, 8>), grid, dim3(kBlock), lds, mgr_stream(c), X, dY, code, s, per, part);
    else
      hipLaunchKernelGGL((k_conv_pool_bwd_w_partial<5, 8>), grid, dim3(kBlock), lds, mgr_stream(c), X, dY, code, s, per, part);
  }
  MGR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_conv_pool_bwd_w_final, dim3((nE + kBlock - 1) / kBlock), dim3(kBlock), 0, mgr_stream(c), part, nchunk, K, Cout, dW, db);
  MGR_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
