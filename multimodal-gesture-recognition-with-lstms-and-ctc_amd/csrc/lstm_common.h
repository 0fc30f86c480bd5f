// Device helpers shared by the LSTM scan kernels: the cell functions, forward and BPTT, and the DPP move (Keras LSTMCell
// semantics; reference call sites
// multimodal_fusion/multimodal.py:159-168: activation='tanh', recurrent_activation='hard_sigmoid').
#pragma once
#include "common.h"
#include "split_f16.h"   // (f32x4)

__device__ __forceinline__ float mgr_hsig(float z) { return fminf(fmaxf(0.2f * z + 0.5f, 0.f), 1.f); }
// tanh via one v_exp_f32 + one v_rcp_f32 (1 ulp; __frcp_rn would be the ten-instruction IEEE division sequence, and vector
// instructions are step time in the scans: they do not overlap with the SIMD's MFMAs): |abs err| ~1e-7, saturates cleanly to +-1
__device__ __forceinline__ float mgr_tanh(float x) {
  float e = __expf(2.f * x);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}
__device__ __forceinline__ float mgr_hsig_grad(float a) { return (a > 0.f && a < 1.f) ? 0.2f : 0.f; }

// One LSTM cell step on activated pre-activations z (i,f,c,o); returns h, updates c, emits activated gates.
__device__ __forceinline__ float mgr_cell_fwd(const float zi, const float zf, const float zc, const float zo, float& c,
                                              float4& gates) {
  float i = mgr_hsig(zi), f = mgr_hsig(zf), g = mgr_tanh(zc), o = mgr_hsig(zo);
  c = f * c + i * g;
  gates = make_float4(i, f, g, o);
  return o * mgr_tanh(c);
}

// One BPTT cell step. dh: total dL/dh_t; dc_carry: dL/dc_t arriving from step t+1 (in/out).
__device__ __forceinline__ float4 mgr_cell_bwd(float dh, float4 g4, float c, float c_prev, float& dc_carry) {
  float i = g4.x, f = g4.y, g = g4.z, o = g4.w;
  float tc = mgr_tanh(c);
  float dO = dh * tc;
  float dc = dh * o * (1.f - tc * tc) + dc_carry;
  float di = dc * g, df = dc * c_prev, dg = dc * i;
  dc_carry = dc * f;
  return make_float4(di * mgr_hsig_grad(i), df * mgr_hsig_grad(f), dg * (1.f - g * g), dO * mgr_hsig_grad(o));
}
// mgr_cell_bwd with tanh(c) given: every split-f16 form of the BPTT step (lstm_cluster_bwd.hip: cluster_bwd_run, cluster_bwd_run16;
// lstm_cu_bwd.hip) goes through THIS function with an opaque tc, so that hipcc contracts the cell arithmetic the same way in all of
// them (the multi-CU forms are compared bit for bit)
__device__ __forceinline__ float4 mgr_cell_bwd_tc(float dh, float4 g4, float tc, float c_prev, float& dc_carry) {
#pragma clang fp contract(off)   // (every fused operation below is written out: no context-dependent contraction)
  const float i = g4.x, f = g4.y, g = g4.z, o = g4.w;
  const float dO = dh * tc;
  const float dc = __builtin_fmaf(dh * o, __builtin_fmaf(-tc, tc, 1.f), dc_carry);
  const float di = dc * g, df = dc * c_prev, dg = dc * i;
  dc_carry = dc * f;
  return make_float4(di * mgr_hsig_grad(i), df * mgr_hsig_grad(f), dg * __builtin_fmaf(-g, g, 1.f), dO * mgr_hsig_grad(o));
}

// DPP with the lane's own value where a row has no source (ctc_lattice.h has the same for the lattices, dpp_f32)
template <int CTRL>
__device__ __forceinline__ float mgr_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xf, 0xf, false));
}
