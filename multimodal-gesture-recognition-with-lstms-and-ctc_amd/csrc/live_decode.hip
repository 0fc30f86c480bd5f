// Live recognition: mgr_live_greedy - the greedy CTC decode of a session that arrives window by window.  The run that is
// open at the end of a window (label, first and last frame, frame count, float32 sum of the frame maxima) stays on the device in
// the session's state block and is continued by the next call, so the posteriors never leave the device.
//
// One wave per session, 64 frames at a time, a lane per frame: the lane finds its frame's best class (first index on ties, as
// mgr_frame_argmax), a ballot marks the lanes whose best class differs from the frame before (lane 0: from the carried run), and the
// lane at the start of a run owns it: it adds the run's frame maxima one at a time, in frame order, from LDS.  A run that another
// start follows inside the batch is final; the last one stays open and is handed to the next batch / the next call.
#include "common.h"

namespace {

struct LiveRun {
  int lab, first, last, cnt;
  float sum;
};

__device__ __forceinline__ void emit(int32_t* __restrict__ lab, int32_t* __restrict__ seg, float* __restrict__ conf, size_t row, int cap, int e,
                                     const LiveRun& r) {
  if (e >= cap) return;
  lab[row * cap + e] = r.lab;
  seg[(row * cap + e) * 2] = r.first;
  seg[(row * cap + e) * 2 + 1] = r.last;
  conf[row * cap + e] = r.sum / (float)r.cnt;
}

__global__ __launch_bounds__(64) void k_live_greedy(const float* __restrict__ P, int Tw, int C, const int32_t* __restrict__ n_keep, int blank,
                                                    int skip, int32_t* __restrict__ state, const int32_t* __restrict__ flush, int cap,
                                                    int32_t* __restrict__ n_events, int32_t* __restrict__ lab, int32_t* __restrict__ seg,
                                                    float* __restrict__ conf) {
  __shared__ float prob[64];
  const int s = blockIdx.x, lane = threadIdx.x;
  int nk = n_keep[s];
  nk = nk < 0 ? 0 : (nk > Tw ? Tw : nk);
  int32_t* st = state + (size_t)s * MGR_LIVE_STATE_WORDS;
  const int consumed = st[0];
  LiveRun open = {st[1], st[2], st[3], st[4], __int_as_float(st[5])};   // (uniform over the wave)
  if (open.cnt <= 0) open = LiveRun{-1, 0, 0, 0, 0.f};
  int nev = 0;
  for (int base = 0; base < nk; base += 64) {
    const int i = base + lane, g = consumed + i;
    const bool valid = i < nk && g >= skip;
    int b = -1;
    float mx = 0.f;
    if (valid) {
      const float* row = P + ((size_t)s * Tw + i) * C;
      mx = row[0];
      b = 0;
      for (int c = 1; c < C; ++c) {
        const float v = row[c];
        if (v > mx) {
          mx = v;
          b = c;
        }
      }
    }
    prob[lane] = mx;
    __syncthreads();
    const unsigned long long vmask = __ballot(valid);
    if (vmask != 0) {
      // the frames below skip are a prefix of the session and the frames past n_keep a suffix of the batch: valid lanes are [lo, hi)
      const int lo = __ffsll((long long)vmask) - 1, hi = 64 - __clzll((long long)vmask);
      int prevb = __shfl_up(b, 1);
      if (lane == lo) prevb = open.lab;
      const bool start = valid && b != prevb;
      const unsigned long long smask = __ballot(start);
      if (open.cnt > 0 && ((smask >> lo) & 1ull)) {    // the carried run ends where this batch begins
        if (open.lab != blank) {
          if (lane == 0) emit(lab, seg, conf, s, cap, nev, open);
          ++nev;
        }
        open.cnt = 0;
      }
      const bool own = start || (valid && lane == lo);   // (lane lo without a start continues the carried run)
      const unsigned long long above = smask & ~((2ull << lane) - 1ull);
      const int end = above ? __ffsll((long long)above) - 1 : hi;
      const bool closed = own && above != 0;
      LiveRun r = {b, g, 0, 0, 0.f};
      if (own) {
        if (!start) r.first = open.first, r.cnt = open.cnt, r.sum = open.sum;
        for (int q = lane; q < end; ++q) r.sum += prob[q];
        r.cnt += end - lane;
        r.last = consumed + base + end - 1;
      }
      const bool ev = closed && b != blank;
      const unsigned long long emask = __ballot(ev);
      if (ev) emit(lab, seg, conf, s, cap, nev + __popcll(emask & ((1ull << lane) - 1ull)), r);
      nev += __popcll(emask);
      const int src = __ffsll((long long)__ballot(own && !closed)) - 1;   // the run that stays open: exactly one lane
      open.lab = __shfl(r.lab, src);
      open.first = __shfl(r.first, src);
      open.last = __shfl(r.last, src);
      open.cnt = __shfl(r.cnt, src);
      open.sum = __shfl(r.sum, src);
    }
    __syncthreads();
  }
  if (flush && flush[s] && open.cnt > 0) {
    if (open.lab != blank) {
      if (lane == 0) emit(lab, seg, conf, s, cap, nev, open);
      ++nev;
    }
    open = LiveRun{-1, 0, 0, 0, 0.f};
  }
  if (lane == 0) {
    st[0] = consumed + nk;
    st[1] = open.lab, st[2] = open.first, st[3] = open.last, st[4] = open.cnt, st[5] = __float_as_int(open.sum);
    n_events[s] = nev;
  }
}

}  // namespace

extern "C" {

int mgr_live_greedy(mgr_ctx* c, const float* P, int S, int Tw, int C, const int32_t* n_keep, int blank, int skip, int32_t* state,
                    const int32_t* flush, int cap, int32_t* n_events, int32_t* lab, int32_t* seg, float* conf) {
  MGR_REQUIRE(S >= 1 && Tw >= 1 && C >= 1, "bad shape S=%d Tw=%d C=%d", S, Tw, C);
  MGR_REQUIRE(blank < C && skip >= 0 && cap >= 0, "blank = %d (< C = %d), skip = %d, cap = %d", blank, C, skip, cap);
  MGR_REQUIRE(P && n_keep && state && n_events, "null P / n_keep / state / n_events");
  MGR_REQUIRE(cap == 0 || (lab && seg && conf), "null event arrays with cap = %d", cap);
  MGR_REQUIRE((((uintptr_t)P | (uintptr_t)n_keep | (uintptr_t)state | (uintptr_t)flush | (uintptr_t)n_events | (uintptr_t)lab | (uintptr_t)seg |
                (uintptr_t)conf) & 3) == 0, "misaligned pointer");
  MGR_REQUIRE(c, "null context");
  mgr_prof_begin(c, MGR_K_MISC);
  hipLaunchKernelGGL(k_live_greedy, dim3((unsigned)S), dim3(64), 0, mgr_stream(c), P, Tw, C, n_keep, blank, skip, state, flush, cap, n_events, lab,
                     seg, conf);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}

}  // extern "C"
