// Upper-body crops of the RGB network's frames (reference rgb_network/roi_extraction.py:18-80): OpenCV's 8-bit BGR2GRAY, the crop
// [y0, y1) x [x0, x1) of the gray frame, and OpenCV's generic 8-bit fixed-point INTER_CUBIC resize to img_dim x img_dim.  DESIGN 9d
// restates the arithmetic; rgb_network/roi_extraction.py builds the boxes (clamps, slicing, fallback) and uploads the frames.
//
// One workgroup (4 waves) per frame:
//   1. per output column / row: source offset and the four Q11 cubic weights (float32 as OpenCV's interpolateCubic, fp contraction
//      off, rounded half to even), and the ascending list of the crop rows the vertical taps touch (at most min(4 img_dim, crop
//      height)) with each vertical tap's index into it;
//   2. per step every wave stages one touched source row as aligned dwords in LDS, and its lane dx forms the gray values of output
//      column dx's four horizontal taps (clamped to the crop) and their int32 weighted sum -> int32 tile [touched row][img_dim];
//   3. the vertical pass: 4 taps x 4 Q11 weights in int32, (v + 2^21) >> 22 saturated to 0..255, into an LDS byte image that is
//      stored with dword stores (the frame's unaligned head and tail bytes singly).
// Integer arithmetic past the weight tables and every byte written by one thread (no atomics): repeated launches are bit-identical.
#include "common.h"

namespace {

constexpr int ROI_MAX_DIM = 64;
constexpr int ROI_MAX_W = 4096;
constexpr int ROI_THREADS = 256;
constexpr int ROI_WAVES = ROI_THREADS / 64;   // source rows staged per step: one per wave

__host__ __device__ inline int roi_raw_dwords(int W) { return (3 * W) / 4 + 1; }   // a crop row's dwords: [3 x0 / 4, (3 x1 + 3) / 4)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// OpenCV resize(): scale = 1 / (dsize / ssize) in double, fx = (float)((d + 0.5) scale - 0.5), sx = floor(fx), fx -= sx, then
// interpolateCubic(fx) with A = -0.75 in float32 and saturate_cast<short>(c * 2048) (round half to even).  No fused multiply-add
// anywhere here: a contraction changes fx and the weights.
__device__ void cubic_tab(int d, int dst, int src, int* ofs, int* w) {
#pragma clang fp contract(off)
  const double scale = 1.0 / ((double)dst / (double)src);
  float fx = (float)(((double)d + 0.5) * scale - 0.5);
  const int sx = (int)floorf(fx);
  fx -= (float)sx;
  const float A = -0.75f;
  const float x1 = fx + 1.f, y = 1.f - fx;
  const float c0 = ((A * x1 - 5.f * A) * x1 + 8.f * A) * x1 - 4.f * A;
  const float c1 = ((A + 2.f) * fx - (A + 3.f)) * fx * fx + 1.f;
  const float c2 = ((A + 2.f) * y - (A + 3.f)) * y * y + 1.f;
  const float c3 = 1.f - c0 - c1 - c2;
  *ofs = sx;
  w[0] = (int)rintf(c0 * 2048.f);
  w[1] = (int)rintf(c1 * 2048.f);
  w[2] = (int)rintf(c2 * 2048.f);
  w[3] = (int)rintf(c3 * 2048.f);
}

// dynamic LDS: int32 tile [4 * D][D] (the touched rows' horizontal sums), then ROI_WAVES staged source rows of roi_raw_dwords(W)
__global__ __launch_bounds__(ROI_THREADS) void k_roi_crop(const uint32_t* __restrict__ frames, int H, int W, const int* __restrict__ boxes,
                                                          int D, uint8_t* __restrict__ out) {
  extern __shared__ int lds[];
  __shared__ int xofs[ROI_MAX_DIM], xw[ROI_MAX_DIM * 4];
  __shared__ int yofs[ROI_MAX_DIM], yw[ROI_MAX_DIM * 4], vidx[ROI_MAX_DIM * 4];
  __shared__ int ylo[ROI_MAX_DIM], ycnt[ROI_MAX_DIM], rowlist[ROI_MAX_DIM * 4];
  __shared__ int n_rows;
  __shared__ uint32_t obuf[(ROI_MAX_DIM * ROI_MAX_DIM + 4) / 4 + 1];
  int* tile = lds;
  uint32_t* raw_all = (uint32_t*)(lds + 4 * D * D);
  const int rawn = roi_raw_dwords(W);
  uint8_t* ob = (uint8_t*)obuf;

  const int f = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int DD = D * D;
  const size_t gb = (size_t)f * (size_t)DD;   // first output byte of this frame
  const int mis = (int)(gb & 3);               // obuf byte mis + e holds output byte e: obuf's dwords are the aligned global ones
  const int y0 = boxes[4 * f], y1 = boxes[4 * f + 1], x0 = boxes[4 * f + 2], x1 = boxes[4 * f + 3];
  const int ch = y1 - y0, cw = x1 - x0;
  const bool valid = y0 >= 0 && y1 <= H && ch > 0 && x0 >= 0 && x1 <= W && cw > 0;   // uniform over the workgroup

  if (!valid) {   // the host never sends such a box; the frame's output is zeros rather than a read outside the frame
    for (int e = tid; e < DD; e += ROI_THREADS) ob[mis + e] = 0;
  } else {
    // 1. tables
    if (tid < D) {
      cubic_tab(tid, D, cw, &xofs[tid], &xw[4 * tid]);
    } else if (tid >= 64 && tid < 64 + D) {
      cubic_tab(tid - 64, D, ch, &yofs[tid - 64], &yw[4 * (tid - 64)]);
    }
    __syncthreads();
    // touched rows: taps of output row dy are [lo, hi] = clamp([sy - 1, sy + 2]); sy ascends with dy, so the rows new at dy are
    // [max(lo, hi of dy - 1 + 1), hi], listed in ascending order, and every tap's index is base + row - (first new row)
    if (tid < D) {
      const int sy = yofs[tid];
      const int lo = clampi(sy - 1, 0, ch - 1), hi = clampi(sy + 2, 0, ch - 1);
      const int prev = tid > 0 ? clampi(yofs[tid - 1] + 2, 0, ch - 1) : -1;
      const int nlo = lo > prev + 1 ? lo : prev + 1;
      ylo[tid] = nlo;
      ycnt[tid] = hi >= nlo ? hi - nlo + 1 : 0;
    }
    __syncthreads();
    if (tid < D) {
      int base = 0;
      for (int i = 0; i < tid; ++i) base += ycnt[i];
      const int nlo = ylo[tid], cnt = ycnt[tid], sy = yofs[tid];
      for (int i = 0; i < cnt; ++i) rowlist[base + i] = nlo + i;
      for (int k = 0; k < 4; ++k) vidx[4 * tid + k] = base + clampi(sy - 1 + k, 0, ch - 1) - nlo;
      if (tid == D - 1) n_rows = base + cnt;
    }
    __syncthreads();
    const int R = n_rows;

    // 2. horizontal pass, one staged source row per wave and step
    const int d0 = (3 * x0) >> 2, nd = ((3 * x1 + 3) >> 2) - d0;   // within the row: 3 W is a multiple of 4
    const int boff = 3 * x0 - 4 * d0;                                // crop column 0's byte in the staged row
    uint32_t* raw = raw_all + wave * rawn;
    const uint8_t* raw8 = (const uint8_t*)raw;
    const size_t frame_dw = (size_t)H * (size_t)(3 * W / 4);
    int sx = 0, w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    if (lane < D) {
      sx = xofs[lane];
      w0 = xw[4 * lane];
      w1 = xw[4 * lane + 1];
      w2 = xw[4 * lane + 2];
      w3 = xw[4 * lane + 3];
    }
    for (int j0 = 0; j0 < R; j0 += ROI_WAVES) {
      const int j = j0 + wave;
      if (j < R) {
        const uint32_t* src = frames + (size_t)f * frame_dw + (size_t)(y0 + rowlist[j]) * (size_t)(3 * W / 4) + d0;
        for (int i = lane; i < nd; i += 64) raw[i] = src[i];
      }
      __syncthreads();
      if (j < R && lane < D) {
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int b = boff + 3 * clampi(sx - 1 + k, 0, cw - 1);
          const int g = (1868 * (int)raw8[b] + 9617 * (int)raw8[b + 1] + 4899 * (int)raw8[b + 2] + 8192) >> 14;
          acc += g * (k == 0 ? w0 : (k == 1 ? w1 : (k == 2 ? w2 : w3)));
        }
        tile[j * D + lane] = acc;
      }
      __syncthreads();
    }

    // 3. vertical pass: consecutive lanes read consecutive dwords of a tile row
    for (int e = tid; e < DD; e += ROI_THREADS) {
      const int dy = e / D, dx = e - dy * D;
      int v = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) v += yw[4 * dy + k] * tile[vidx[4 * dy + k] * D + dx];
      v = (v + (1 << 21)) >> 22;
      ob[mis + e] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
  }
  __syncthreads();

  // store: the dwords wholly inside the frame as dwords, the head and tail bytes singly
  const int q0 = mis ? 1 : 0, q1 = (mis + DD) >> 2;
  uint32_t* out32 = (uint32_t*)(out + (gb - mis));
  for (int q = q0 + tid; q < q1; q += ROI_THREADS) out32[q] = obuf[q];
  const int head = 4 * q0 - mis < DD ? 4 * q0 - mis : DD;
  const int tail = 4 * q1 - mis > head ? 4 * q1 - mis : head;
  if (tid < head) out[gb + tid] = ob[mis + tid];
  if (tail + tid < DD) out[gb + tail + tid] = ob[mis + tail + tid];
}

}  // namespace

extern "C" int mgr_roi_crop(mgr_ctx* c, const uint8_t* frames, int n, int H, int W, const int32_t* boxes, int img_dim, uint8_t* out) {
  MGR_REQUIRE(c, "null argument");
  MGR_REQUIRE(n >= 0, "n must be >= 0");
  MGR_REQUIRE(H >= 1 && W >= 1 && W <= ROI_MAX_W && (3 * W) % 4 == 0, "need H >= 1 and 1 <= W <= 4096 with 3 W a multiple of 4");
  MGR_REQUIRE(img_dim >= 1 && img_dim <= ROI_MAX_DIM, "img_dim must be in [1, 64]");
  if (n == 0) return 0;
  MGR_REQUIRE(frames && boxes && out, "null argument");
  MGR_REQUIRE(((uintptr_t)frames & 3) == 0 && ((uintptr_t)out & 3) == 0, "frames and out must be 4-byte aligned");
  const size_t lds = sizeof(int) * (size_t)(4 * img_dim * img_dim) + sizeof(uint32_t) * (size_t)(ROI_WAVES * roi_raw_dwords(W));
  if (!(c->attr_done & MGR_ATTR_ROI)) {
    MGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_roi_crop), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    c->attr_done |= MGR_ATTR_ROI;
  }
  hipStream_t st = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_MISC);
  hipLaunchKernelGGL(k_roi_crop, dim3((unsigned)n), dim3(ROI_THREADS), lds, st, (const uint32_t*)frames, H, W, (const int*)boxes, img_dim,
                     out);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}
