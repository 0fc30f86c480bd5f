// K18: frame overlap of two segment sets per class - what the Jaccard index of gesture spotting is made of.
//
// One workgroup per sample.  The sample's segments (label, first, last - inclusive frames), filtered and clipped once, lie in LDS; a
// thread per frame, in tiles of 256 frames, walks them and builds the frame's two 64-bit class masks: bit c of `mh` = some hypothesis
// segment of class c covers the frame, the same for `mr` and the reference - so segments of one class on one side are united and segments
// of different classes may overlap.  Per class the four counts of a tile are wave ballots and population counts (lane c of a wave keeps
// class c's), summed over the four waves through LDS in wave order.  Everything is integers: the results are exact.
#include "common.h"

namespace {

constexpr int kOverlapMaxSegs = 4096;   // per side: 2 * 4096 * 12 bytes = 96 KiB of LDS

struct OvSeg { int lab, first, last; };

// one side's segments into LDS: lab = -1 marks what is skipped (a label outside [0, C), an ignored one, first < 0, nothing left after
// the clip to [0, n))
__device__ __forceinline__ void ov_load(OvSeg* dst, const int32_t* __restrict__ lab, const int32_t* __restrict__ seg, int b, int S, int C,
                                        uint64_t ignore, int n, int tid) {
  for (int i = tid; i < S; i += 256) {
    const size_t o = (size_t)b * S + i;
    const int l = lab[o], f = seg[2 * o];
    int e = seg[2 * o + 1];
    e = e > n - 1 ? n - 1 : e;
    const bool ok = l >= 0 && l < C && !((ignore >> (l & 63)) & 1) && f >= 0 && f <= e;
    dst[i].lab = ok ? l : -1;
    dst[i].first = f;
    dst[i].last = e;
  }
}

__device__ __forceinline__ uint64_t ov_mask(const OvSeg* s, int S, int t) {
  uint64_t m = 0;
  for (int i = 0; i < S; ++i) {
    const OvSeg g = s[i];
    if (g.lab >= 0 && g.first <= t && t <= g.last) m |= 1ull << g.lab;
  }
  return m;
}

__global__ __launch_bounds__(256) void k_segment_overlap(const int32_t* __restrict__ hyp_lab, const int32_t* __restrict__ hyp_seg, int Sh,
                                                         const int32_t* __restrict__ ref_lab, const int32_t* __restrict__ ref_seg, int Sr,
                                                         const int32_t* __restrict__ n_frames, int C, uint64_t ignore,
                                                         int32_t* __restrict__ inter, int32_t* __restrict__ uni,
                                                         int32_t* __restrict__ hyp_frames, int32_t* __restrict__ ref_frames) {
  extern __shared__ __attribute__((aligned(16))) int smem_i[];   // [4 waves][4 counts][64 classes] | hyp segments | ref segments
  int* s_cnt = smem_i;
  OvSeg* s_h = reinterpret_cast<OvSeg*>(smem_i + 4 * 4 * 64);
  OvSeg* s_r = s_h + Sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int n = n_frames[b] < 0 ? 0 : n_frames[b];
  ov_load(s_h, hyp_lab, hyp_seg, b, Sh, C, ignore, n, tid);
  ov_load(s_r, ref_lab, ref_seg, b, Sr, C, ignore, n, tid);
  __syncthreads();
  int ci = 0, cu = 0, ch = 0, cr = 0;   // class `lane`, this wave's frames
  for (int t0 = 0; t0 < n; t0 += 256) {
    const int t = t0 + tid;
    uint64_t mh = 0, mr = 0;
    if (t < n) {
      mh = ov_mask(s_h, Sh, t);
      mr = ov_mask(s_r, Sr, t);
    }
    if (!__any((mh | mr) != 0)) continue;   // (wave-uniform)
    for (int c = 0; c < C; ++c) {
      const int h = (int)((mh >> c) & 1), r = (int)((mr >> c) & 1);
      const int ni = __popcll(__ballot(h & r)), nu = __popcll(__ballot(h | r)), nh = __popcll(__ballot(h)), nr = __popcll(__ballot(r));
      if (lane == c) {
        ci += ni;
        cu += nu;
        ch += nh;
        cr += nr;
      }
    }
  }
  s_cnt[(wave * 4 + 0) * 64 + lane] = ci;
  s_cnt[(wave * 4 + 1) * 64 + lane] = cu;
  s_cnt[(wave * 4 + 2) * 64 + lane] = ch;
  s_cnt[(wave * 4 + 3) * 64 + lane] = cr;
  __syncthreads();
  if (tid < C) {
    int v[4];
    for (int k = 0; k < 4; ++k) v[k] = s_cnt[(0 * 4 + k) * 64 + tid] + s_cnt[(1 * 4 + k) * 64 + tid] + s_cnt[(2 * 4 + k) * 64 + tid] + s_cnt[(3 * 4 + k) * 64 + tid];
    const size_t o = (size_t)b * C + tid;
    inter[o] = v[0];
    uni[o] = v[1];
    hyp_frames[o] = v[2];
    ref_frames[o] = v[3];
  }
}

}  // namespace

extern "C" {

int mgr_segment_overlap(mgr_ctx* c, const int32_t* hyp_lab, const int32_t* hyp_seg, int Sh, const int32_t* ref_lab, const int32_t* ref_seg, int Sr,
                        const int32_t* n_frames, int B, int C, uint64_t ignore_mask, int32_t* inter, int32_t* uni, int32_t* hyp_frames,
                        int32_t* ref_frames) {
  MGR_REQUIRE(c && hyp_lab && hyp_seg && ref_lab && ref_seg && n_frames && inter && uni && hyp_frames && ref_frames, "null argument");
  MGR_REQUIRE(B > 0 && Sh > 0 && Sr > 0, "bad shape B=%d Sh=%d Sr=%d", B, Sh, Sr);
  MGR_REQUIRE(C >= 1 && C <= 64, "C=%d outside [1, 64]", C);
  MGR_REQUIRE(Sh <= kOverlapMaxSegs && Sr <= kOverlapMaxSegs, "Sh=%d Sr=%d above %d segments a side", Sh, Sr, kOverlapMaxSegs);
  const size_t lds = (size_t)4 * 4 * 64 * sizeof(int) + (size_t)(Sh + Sr) * sizeof(OvSeg);
  if (!(c->attr_done & MGR_ATTR_OVERLAP)) {
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_segment_overlap), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    c->attr_done |= MGR_ATTR_OVERLAP;
  }
  mgr_prof_begin(c, MGR_K_MISC);
  hipLaunchKernelGGL(k_segment_overlap, dim3(B), dim3(256), lds, mgr_stream(c), hyp_lab, hyp_seg, Sh, ref_lab, ref_seg, Sr, n_frames, C, ignore_mask,
                     inter, uni, hyp_frames, ref_frames);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}

}  // extern "C"
