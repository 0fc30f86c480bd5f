// Per-sample sequence lengths: mgr_seq_zero_tail zeroes the rows [b, t >= len[b], 0:row) of one or several [B, T, row]
// float32 buffers - the gate pre-activations of a reverse recurrence before its scan, its saved gates after it, the posteriors a
// caller gets - and writes nothing else.  The lengths live on the device, so the grid is sized from T: a fixed number of
// workgroups per (job, sample) stride over that sample's tail and leave at once where there is none.  16-byte stores where row, ld
// and the pointer allow, one float per store otherwise.  No atomics, no workspace.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxSlices = 32;                 // workgroups per (job, sample)
constexpr size_t kSliceFloats = 16 * 1024;     // ... one per this many floats of a whole sample, up to kMaxSlices

struct SeqJobs {
  float* buf[MGR_SEQ_MAX_JOBS];
  int row[MGR_SEQ_MAX_JOBS], ld[MGR_SEQ_MAX_JOBS], T[MGR_SEQ_MAX_JOBS], vec[MGR_SEQ_MAX_JOBS];
};

// The tail of a sample is nrows rows of `w` units (float4 or float) `ld` floats apart; with ld == row it is ONE row of the whole tail.
template <typename V>
__device__ static inline void zero_rows(float* base, size_t nrows, size_t w, size_t ld) {
  const size_t n = nrows * w, step = (size_t)gridDim.x * kBlock;
  constexpr size_t per = sizeof(V) / sizeof(float);
  V zero;
  memset(&zero, 0, sizeof zero);
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
    size_t r = 0, c = i;
    if (nrows > 1) r = i / w, c = i - r * w;
    *reinterpret_cast<V*>(base + r * ld + c * per) = zero;
  }
}

__global__ __launch_bounds__(kBlock) void k_seq_zero_tail(SeqJobs J, const int32_t* __restrict__ seq_len) {
  const int j = blockIdx.z, b = blockIdx.y;
  const int T = J.T[j];
  int len = seq_len[b];
  len = len < 0 ? 0 : (len > T ? T : len);
  if (len == T) return;
  const size_t row = (size_t)J.row[j], ld = (size_t)J.ld[j];
  float* base = J.buf[j] + ((size_t)b * T + len) * ld;
  size_t nrows = (size_t)(T - len), w = row;
  if (ld == row) w *= nrows, nrows = 1;
  if (J.vec[j])
    zero_rows<float4>(base, nrows, w / 4, ld);
  else
    zero_rows<float>(base, nrows, w, ld);
}

}  // namespace

extern "C" {

int mgr_seq_zero_tail(mgr_ctx* c, int njobs, const mgr_seq_fill_job* jobs, const int32_t* seq_len) {
  MGR_REQUIRE(c, "null context");
  MGR_REQUIRE(njobs >= 0, "njobs = %d", njobs);
  if (njobs == 0) return 0;
  MGR_REQUIRE(jobs && seq_len, "null job list or seq_len");
  const int B = jobs[0].B;
  for (int j = 0; j < njobs; ++j) {
    const mgr_seq_fill_job& q = jobs[j];
    MGR_REQUIRE(q.buf, "job %d: null buffer", j);
    MGR_REQUIRE(q.row > 0 && q.ld >= q.row, "job %d: row = %d, ld = %d (0 < row <= ld)", j, q.row, q.ld);
    MGR_REQUIRE(q.B >= 0 && q.T >= 0 && q.B <= 65535, "job %d: bad shape B=%d T=%d (B <= 65535)", j, q.B, q.T);
    MGR_REQUIRE(q.B == B, "job %d: B = %d, job 0 has %d (one seq_len per call)", j, q.B, B);
  }
  if (B == 0) return 0;
  mgr_prof_begin(c, MGR_K_MISC);
  for (int j0 = 0; j0 < njobs; j0 += MGR_SEQ_MAX_JOBS) {
    SeqJobs J;
    memset(&J, 0, sizeof J);
    const int n = njobs - j0 < MGR_SEQ_MAX_JOBS ? njobs - j0 : MGR_SEQ_MAX_JOBS;
    size_t most = 0;
    int live = 0;
    for (int j = 0; j < n; ++j) {
      const mgr_seq_fill_job& q = jobs[j0 + j];
      if (q.T == 0) continue;       // (no frames: nothing to zero)
      J.buf[live] = q.buf, J.row[live] = q.row, J.ld[live] = q.ld, J.T[live] = q.T;
      J.vec[live] = q.row % 4 == 0 && q.ld % 4 == 0 && ((uintptr_t)q.buf & 15) == 0;
      const size_t fl = (size_t)q.T * q.row;
      if (fl > most) most = fl;
      ++live;
    }
    if (!live) continue;
    size_t slices = (most + kSliceFloats - 1) / kSliceFloats;
    slices = slices < 1 ? 1 : (slices > kMaxSlices ? kMaxSlices : slices);
    hipLaunchKernelGGL(k_seq_zero_tail, dim3((unsigned)slices, (unsigned)B, (unsigned)live), dim3(kBlock), 0, mgr_stream(c), J, seq_len);
    MGR_LAUNCH_CHECK();
  }
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}

}  // extern "C"
