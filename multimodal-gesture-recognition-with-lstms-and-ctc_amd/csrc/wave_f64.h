// The fp64 pieces that the one-wave searches share: the prefix beam search (beam.hip), the select of the joint decode (joint.hip) and
// the fixed-order sums of the lexicon decode (lexicon.hip).  Scores are doubles there because a decision hangs on them; a double
// crosses the lanes as its two halves.  Everything is force-inlined into its caller: a translation unit pays for what it uses.
#pragma once
#include "common.h"

namespace {

constexpr double kNegInfD = -__builtin_huge_val();

__device__ __forceinline__ double lse64(double a, double b) {
  if (a == kNegInfD) return b;
  if (b == kNegInfD) return a;
  double m = a > b ? a : b;
  return m + log1p(exp(-fabs(a - b)));
}

__device__ __forceinline__ double shfl_xor_d(double v, int o) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __shfl_xor(lo, o);
  hi = __shfl_xor(hi, o);
  return __hiloint2double(hi, lo);
}

// One step of the butterfly that turns every lane's (score, index) into the wave's - the larger score, ties to the smaller index:
//   for (int o = 32; o > 0; o >>= 1) { const ScoreIdx q = wave_argmax_step_d(best, bidx, o); best = q.v; bidx = q.i; }
// By value, and the loop with the caller: with the loop in here, or the pair passed by reference, the compiler orders the callers'
// registers differently, and the 34-per-lane beam search, which has none to spare, spills 8 bytes more.
struct ScoreIdx {
  double v;
  int i;
};
__device__ __forceinline__ ScoreIdx wave_argmax_step_d(double best, int bidx, int o) {
  double ob = shfl_xor_d(best, o);
  int oi = __shfl_xor(bidx, o);
  if (ob > best || (ob == best && oi < bidx)) {
    best = ob;
    bidx = oi;
  }
  return {best, bidx};
}

}  // namespace
