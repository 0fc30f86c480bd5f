// The split-f16 arithmetic, once: an f32 product as THREE f16 matrix products.  Every f32 operand becomes an f16 (hi, lo)
// pair of its scaled value - x s = hi + lo to 22+ bits, s a power of two, so scaling is exact - and a 32 x 32 block takes
// hi hi + lo hi + hi lo into one f32 accumulator (the dropped lo lo term is 2^-22 of the product).  What the projection and
// weight-gradient GEMMs (gemm.hip, gemm_split.hip) and the persistent scans (lstm_cluster.hip, lstm_cluster_bwd.hip, lstm_cu_bwd.hip)
// share of it lives here: the vector types, the split with its value pin, the exponent of a scale, and - for the GEMMs only - the
// MFMA tile pieces: the accumulator map, the three-MFMA product, the XCD-aware tile decode and the four-gate Z epilogue.
//
// What is here is pieces, not a kernel: every kernel keeps its stage loop, its LDS layout, the floor of its exponent and what it does
// with a non-finite maximum, because those decide its bits and its speed.  The scans take the types, the split and the exponent and
// nothing else (their machine code is held identical across changes of this file).  Everything is force-inlined into its caller and
// sits at global scope like lstm_common.h, which takes its f32x4 from here.
#pragma once
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---- the (hi, lo) split ------------------------------------------------------------------------------------------------------------

// x = hi + lo, both f16: hi = rn(x), lo = rn(x - hi), x an f32 VALUE.  The empty asm pins that value: without it hipcc contracts a
// product that feeds x into the subtraction (v_fma_mix: exact product - hi') AND takes that hi' by rounding the exact product to
// f16 in one step, while the hi it stores was rounded from the f32 product - two different roundings of x now and then, i.e. a lo
// that belongs to another hi: one operand in a few hundred with 11 instead of 22 bits (seen with the mask factor 2.5; a power-of-two
// factor makes the product exact and hides it).
__device__ __forceinline__ _Float16 split_hi(float& x) {   // pins x, returns hi
  asm volatile("" : "+v"(x));
  return (_Float16)x;
}
__device__ __forceinline__ _Float16 split_lo(float x, _Float16 hi) { return (_Float16)(x - (float)hi); }   // x as split_hi left it
__device__ __forceinline__ void split_f16(float x, _Float16& hi, _Float16& lo) {
  hi = split_hi(x);
  lo = split_lo(x, hi);
}
// Into two f16 vectors (V = f16x4 / f16x8), in the two statement orders the open-coded copies had.  The results are the same; hipcc's
// instruction schedule follows the order, and each user keeps the one its machine code was measured with:
//   split_f16_lane: lane e, its hi in place before its lo is taken (the scans);
//   split_f16_vec:  N values, each lane's (hi, lo) formed first and then put in place (the GEMMs).
template <typename V>
__device__ __forceinline__ void split_f16_lane(float x, V& hi, V& lo, int e) {
  const _Float16 h = split_hi(x);
  hi[e] = h;
  lo[e] = split_lo(x, h);
}
template <int N, typename V>
__device__ __forceinline__ void split_f16_vec(const float (&xs)[N], V& hi, V& lo) {
#pragma unroll
  for (int e = 0; e < N; ++e) {
    _Float16 h, l;
    split_f16(xs[e], h, l);
    hi[e] = h;
    lo[e] = l;
  }
}

// ---- the scale ---------------------------------------------------------------------------------------------------------------------

// ex with m = f 2^ex, f in [0.5, 1), not below `floor`; a maximum that is zero, Inf or NaN gives 0.  The scale of an operand whose
// largest magnitude is m is 2^(15 - ex): the largest scaled magnitude lies in [2^14, 2^15).  The floor keeps that power of two (and the
// inverses a kernel builds from ex) finite for tiny maxima: -60 for weights, -100 for gradients, SPLIT_NO_FLOOR for a bound the host
// has checked to be an ordinary number.
constexpr int SPLIT_NO_FLOOR = -200;
__host__ __device__ __forceinline__ int split_exponent(float m, int floor) {
  int ex = 0;
  if (m > 0.f && m < 3.0e38f) (void)frexpf(m, &ex);
  return ex < floor ? floor : ex;
}
// What a non-finite maximum (m >= 3e38, NaN) does to the scale - each call site names its policy:
//   SPLIT_NONFINITE_ZERO  scale 0: the caller's inverse becomes NaN and so does its whole output (weights: an Inf weight stays visible)
//   SPLIT_NONFINITE_NAN   quiet NaN: the row's products are NaN (dZ rows: an Inf / NaN gradient stays visible)
//   SPLIT_NONFINITE_NONE  no special case, 2^15 (a maximum checked beforehand)
enum SplitNonFinite { SPLIT_NONFINITE_ZERO, SPLIT_NONFINITE_NAN, SPLIT_NONFINITE_NONE };
template <SplitNonFinite P>
__host__ __device__ __forceinline__ float split_scale(float m, int floor) {
  const float s = ldexpf(1.f, 15 - split_exponent(m, floor));
  if (P == SPLIT_NONFINITE_NONE) return s;
  return m < 3.0e38f ? s : (P == SPLIT_NONFINITE_ZERO ? 0.f : __builtin_nanf(""));
}
// num / (sw sx), what an accumulator of (A sx) (B sw) is multiplied with; sw = 0 (SPLIT_NONFINITE_ZERO): quiet NaN
__device__ __forceinline__ float split_unscale(float num, float sw, float sx) { return sw > 0.f ? num / (sw * sx) : __builtin_nanf(""); }

// ---- MFMA 32 x 32 tile pieces (the GEMMs) --------------------------------------------------------------------------------------------

// accumulator register reg (0 .. 15) of a lane -> (row, column), for the 32 x 32 block whose first row / column is row0 / col0.  The
// lane enters as the kernel's own l31 = lane & 31 and lh = lane >> 5 (every kernel has them for its fragment reads), and the row is one
// sum from left to right with the origin first: given `lane`, or another order, hipcc forms other common subexpressions in the
// unrolled epilogues and allocates the registers of the whole kernel differently.
__device__ __forceinline__ int acc_row(int row0, int reg, int lh) { return row0 + (reg & 3) + 8 * (reg >> 2) + 4 * lh; }
__device__ __forceinline__ int acc_col(int col0, int l31) { return col0 + l31; }

template <int A, int B>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[A][B]) {
#pragma unroll
  for (int i = 0; i < A; ++i)
#pragma unroll
    for (int j = 0; j < B; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// one 32 x 32 block, 16 k: hi hi + lo hi + hi lo, in this order (a kernel that issues the terms in another order keeps its own code)
__device__ __forceinline__ void mfma3_split(const f16x8& ah, const f16x8& al, const f16x8& bh, const f16x8& bl, f32x16& acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
}

// Workgroup -> tile, XCD-aware: consecutive workgroup ids go round-robin over the 8 XCDs (each with its own L2), so the `per_group`
// workgroups that share operands - the column tiles of one (sample, row tile) of X, all tiles of one sample of a weight gradient - are
// the ids x, x + 8, x + 16, ...: they meet in ONE L2 instead of pulling the same rows into all eight.  The grid holds the groups padded
// to a multiple of 8; a group beyond the last one returns at once (the caller's check).
struct XcdTile {
  int group, item;   // which group, which of its per_group workgroups
};
__device__ __forceinline__ XcdTile xcd_tile(unsigned wg, int per_group) {   // (wg = blockIdx.x; unsigned: jj is known not to be negative)
  const int x = wg & 7, jj = wg >> 3;
  return {(jj / per_group) * 8 + x, jj % per_group};
}

// The Z epilogue of a four-gate projection tile: Z[b, row, 4 unit + g] = acc[g] inv + bias.g for the 2 x 16 rows this lane holds of
// its unit, rows >= T left out, the four gates of a (row, unit) as ONE 16-byte store in the packed order the scans read.  rows0: the
// first row of the wave's 64, lh = lane >> 5.  NonTemporal: Z is read once, by a scan, milliseconds later - it need not displace what concurrent
// products keep in L2.  Each kernel keeps the store kind it was measured with: k_gemm_nn_sparse, k_proj_narrow and k_proj_split store
// non-temporally, k_gemm_nn_sparse16 and k_gemm_nn_dense16 plainly; making them uniform is a change of behaviour, not of form.
template <bool NonTemporal>
__device__ __forceinline__ void store_z_tile(const f32x16 (&acc)[4][2], float inv, const float4& bias, float* __restrict__ Z, int b, int T, int N,
                                             int rows0, int unit, int lh) {
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = acc_row(rows0 + mt * 32, reg, lh);
      if (row < T) {
        float* z = Z + ((size_t)b * T + row) * N + unit * 4;
        if constexpr (NonTemporal) {
          const f32x4 v = {fmaf(acc[0][mt][reg], inv, bias.x), fmaf(acc[1][mt][reg], inv, bias.y), fmaf(acc[2][mt][reg], inv, bias.z),
                           fmaf(acc[3][mt][reg], inv, bias.w)};
          __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(z));
        } else {
          *reinterpret_cast<float4*>(z) = make_float4(fmaf(acc[0][mt][reg], inv, bias.x), fmaf(acc[1][mt][reg], inv, bias.y),
                                                      fmaf(acc[2][mt][reg], inv, bias.z), fmaf(acc[3][mt][reg], inv, bias.w));
        }
      }
    }
}
