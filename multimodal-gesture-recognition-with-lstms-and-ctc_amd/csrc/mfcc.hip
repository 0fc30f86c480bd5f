// HTK HCopy-compatible MFCC_0[_D[_A]] front-end of the audio network (the reference's README: 13 MFCCs + first and second order
// derivatives, extracted with HTK's HCopy and its config_HCopy).  DESIGN 9c restates the algorithm; audio_network/
// feature_extraction.py parses the config and the WAV files and builds the filterbank table.
//
// A batch is a list of ragged utterances (int16 samples, sample_offsets[n_utts + 1]).  Three launches on the ctx stream:
//   k_mfcc_setup     one workgroup: per-utterance frame offsets, per-channel bin ranges, Hamming window, FFT twiddles, DCT matrix
//                    into the workspace;
//   k_mfcc_spectral  one workgroup per frame: pre-emphasis, window, real FFT of size fftN (a complex fftN/2 Stockham radix-2
//                    FFT in LDS plus the split step), magnitude, mel filterbank, log, DCT, lifter -> numCeps + 1 fp64 statics
//                    in the workspace (C1..C_numCeps, C0);
//   k_mfcc_deltas    one thread per output element: statics, deltas and accelerations (+-2 frame regression windows, edge
//                    frames replicated, never across an utterance) rounded to f32, every out_stride-th frame, into the rows
//                    [out_offsets[u], out_offsets[u + 1]) of utterance u; rows past the utterance's last frame are zeroed.
// All arithmetic is fp64; each output is written by one thread in a fixed order (no atomics), so launches are bit-identical.
#include "common.h"

namespace {

constexpr int MFCC_MAX_CHANS = 128;
constexpr int MFCC_MAX_STATICS = 64;
constexpr int MFCC_MIN_FFT = 256;
constexpr int MFCC_MAX_FFT = 2048;   // LDS per workgroup: (2 fftN + numChans) doubles, 33 KiB at most

struct MfccWs {
  long long* frame_off;   // [n_utts + 1]
  int* chan_lo;           // [numChans + 1], bins [chan_lo[c], chan_hi[c]) feed channel c (1-based)
  int* chan_hi;
  double* window;         // [frameSize]
  double* tw_re;          // [fftN / 2]: exp(-2 pi i k / fftN)
  double* tw_im;
  double* dct;            // [numCeps + 1][numChans]: row j < numCeps is cepstrum j + 1, row numCeps is C0
  double* statics;        // [n_frames][numCeps + 1]
};

__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

__host__ __device__ inline size_t carve(MfccWs* w, char* base, int n_utts, long long n_frames, int frameSize, int fftN, int numChans,
                                        int numCeps) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += align256(bytes);
    return p;
  };
  const int half = fftN / 2, ns = numCeps + 1;
  MfccWs t;
  t.frame_off = (long long*)take(sizeof(long long) * (size_t)(n_utts + 1));
  t.chan_lo = (int*)take(sizeof(int) * (size_t)(numChans + 1));
  t.chan_hi = (int*)take(sizeof(int) * (size_t)(numChans + 1));
  t.window = (double*)take(sizeof(double) * (size_t)frameSize);
  t.tw_re = (double*)take(sizeof(double) * (size_t)half);
  t.tw_im = (double*)take(sizeof(double) * (size_t)half);
  t.dct = (double*)take(sizeof(double) * (size_t)ns * numChans);
  t.statics = (double*)take(sizeof(double) * (size_t)ns * (size_t)(n_frames > 0 ? n_frames : 1));
  if (w) *w = t;
  return o;
}

__global__ __launch_bounds__(256) void k_mfcc_setup(MfccWs w, const long long* __restrict__ sample_offsets, int n_utts, int frameSize,
                                                    int frameRate, int fftN, int numChans, int numCeps, const int* __restrict__ loChan) {
  const int tid = threadIdx.x, half = fftN / 2;
  if (tid == 0) {
    long long acc = 0;
    w.frame_off[0] = 0;
    for (int u = 0; u < n_utts; ++u) {
      long long n = sample_offsets[u + 1] - sample_offsets[u];
      acc += n >= frameSize ? (n - frameSize) / frameRate + 1 : 0;
      w.frame_off[u + 1] = acc;
    }
  }
  if (tid == 32) {   // another wave: bin k with loChan[k] = c feeds channel c (weight loWt) and c + 1 (weight 1 - loWt)
    for (int c = 0; c <= numChans; ++c) {
      w.chan_lo[c] = half;
      w.chan_hi[c] = 0;
    }
    for (int k = 0; k < half; ++k) {
      const int c = loChan[k];
      if (c < 0 || c > numChans) continue;
      if (c >= 1) {
        w.chan_lo[c] = min(w.chan_lo[c], k);
        w.chan_hi[c] = k + 1;
      }
      if (c + 1 <= numChans) {
        w.chan_lo[c + 1] = min(w.chan_lo[c + 1], k);
        w.chan_hi[c + 1] = k + 1;
      }
    }
  }
  for (int i = tid; i < frameSize; i += blockDim.x) w.window[i] = 0.54 - 0.46 * cospi(2.0 * i / (double)(frameSize - 1));
  for (int k = tid; k < half; k += blockDim.x) {
    double s, c;
    sincospi(-2.0 * k / (double)fftN, &s, &c);
    w.tw_re[k] = c;
    w.tw_im[k] = s;
  }
  const int ns = numCeps + 1;
  for (int e = tid; e < ns * numChans; e += blockDim.x) {
    const int j = e / numChans, k = e % numChans;
    w.dct[e] = j < numCeps ? cospi((double)(j + 1) * (k + 0.5) / (double)numChans) : 1.0;
  }
}

// LDS swizzle of the FFT buffers.  A Stockham stage of span ns < 16 writes its two outputs to runs of ns elements spaced 2 ns apart,
// so the 16 lanes of a ds_write_b64 group would land on 32 consecutive doubles, two to a bank (bank = (a/4) mod 32).  The stage stores
// element i at i ^ ((i & 16) ? ns : 0) instead: the upper half of each 32-element window moves onto the banks the lower half leaves
// free, and the next stage's contiguous reads (ds_read_b64, 32 lanes over 64 banks) stay within the same 32 doubles.
__device__ __forceinline__ int swz(int i, int key) { return (i & 16) ? (i ^ key) : i; }

__global__ __launch_bounds__(256) void k_mfcc_spectral(MfccWs w, const short* __restrict__ samples,
                                                       const long long* __restrict__ sample_offsets, int n_utts, long long n_frames,
                                                       int frameSize, int frameRate, int fftN, int numChans, int numCeps, int cepLifter,
                                                       double preemph, const int* __restrict__ loChan, const double* __restrict__ loWt) {
  extern __shared__ double lds[];   // re[2][M], im[2][M], fb[numChans]: (4 M + numChans) doubles
  const long long f = blockIdx.x;
  if (f >= n_frames || f >= w.frame_off[n_utts]) return;
  int lo = 0, hi = n_utts;   // utterance u with frame_off[u] <= f < frame_off[u + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (w.frame_off[mid] <= f) lo = mid;
    else hi = mid;
  }
  const int u = lo;
  const short* s = samples + sample_offsets[u] + (f - w.frame_off[u]) * frameRate;
  const int M = fftN / 2, tid = threadIdx.x, nt = blockDim.x;
  double* re[2] = {lds, lds + M};
  double* im[2] = {lds + 2 * M, lds + 3 * M};
  double* fb = lds + 4 * M;

  // pre-emphasis (HTK: s[i] -= k s[i-1] for i = N..2, s[1] *= 1 - k), Hamming window, zero pad; pack the real frame x as the complex
  // sequence z[n] = x[2n] + i x[2n+1]
  for (int n = tid; n < M; n += nt) {
    double v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = 2 * n + h;
      double x = 0.0;
      if (i < frameSize) {
        const double cur = (double)s[i];
        x = (i == 0 ? cur * (1.0 - preemph) : cur - preemph * (double)s[i - 1]) * w.window[i];
      }
      v[h] = x;
    }
    re[0][n] = v[0];
    im[0][n] = v[1];
  }
  __syncthreads();

  // complex FFT of size M, radix-2 Stockham (natural order in and out), ping-pong between the two LDS buffers
  int src = 0, key_in = 0;
  for (int ns = 1; ns < M; ns <<= 1) {
    const int key_out = ns < 16 ? ns : 0;
    const int step = fftN / (2 * ns);   // exp(-2 pi i k / (2 ns)) = tw[k * step]
    for (int j = tid; j < M / 2; j += nt) {
      const int k = j & (ns - 1);
      const double ar = re[src][swz(j, key_in)], ai = im[src][swz(j, key_in)];
      const double br0 = re[src][swz(j + M / 2, key_in)], bi0 = im[src][swz(j + M / 2, key_in)];
      const double wr = w.tw_re[k * step], wi = w.tw_im[k * step];
      const double br = br0 * wr - bi0 * wi, bi = br0 * wi + bi0 * wr;
      const int o = (j - k) * 2 + k;
      re[src ^ 1][swz(o, key_out)] = ar + br;
      im[src ^ 1][swz(o, key_out)] = ai + bi;
      re[src ^ 1][swz(o + ns, key_out)] = ar - br;
      im[src ^ 1][swz(o + ns, key_out)] = ai - bi;
    }
    src ^= 1;
    key_in = key_out;
    __syncthreads();
  }

  // split step: X[k] = (Z[k] + conj Z[M-k]) / 2 - i/2 exp(-2 pi i k / fftN) (Z[k] - conj Z[M-k]), k = 0..M-1 (the Nyquist bin is
  // not used); |X[k]| goes to the other buffer (M >= 128 > 16: the last stage wrote unswizzled)
  for (int k = tid; k < M; k += nt) {
    const int m = k ? M - k : 0;
    const double zr = re[src][k], zi = im[src][k], cr = re[src][m], ci = -im[src][m];
    const double er = 0.5 * (zr + cr), ei = 0.5 * (zi + ci);
    const double dr = zr - cr, di = zi - ci;               // X = E - i/2 W D
    const double wr = w.tw_re[k], wi = w.tw_im[k];
    const double pr = wr * dr - wi * di, pi = wr * di + wi * dr;
    const double xr = er + 0.5 * pi, xi = ei - 0.5 * pr;
    re[src ^ 1][k] = sqrt(xr * xr + xi * xi);
  }
  __syncthreads();
  const double* mag = re[src ^ 1];

  // mel filterbank in ascending bin order per channel, then the log with HTK's floor of 1.0
  for (int c = 1 + tid; c <= numChans; c += nt) {
    double acc = 0.0;
    for (int k = w.chan_lo[c]; k < w.chan_hi[c]; ++k) {
      const int lc = loChan[k];
      if (lc == c) acc += loWt[k] * mag[k];
      else if (lc == c - 1) acc += (1.0 - loWt[k]) * mag[k];
    }
    fb[c - 1] = log(acc < 1.0 ? 1.0 : acc);
  }
  __syncthreads();

  // DCT-II with HTK's sqrt(2 / numChans) scale, lifter on the cepstra (not on C0)
  const int ns_ = numCeps + 1;
  const double norm = sqrt(2.0 / numChans);
  for (int j = tid; j < ns_; j += nt) {
    const double* row = w.dct + (size_t)j * numChans;
    double acc = 0.0;
    for (int k = 0; k < numChans; ++k) acc += fb[k] * row[k];
    double v = acc * norm;
    if (j < numCeps && cepLifter > 0) v *= 1.0 + 0.5 * cepLifter * sinpi((double)(j + 1) / (double)cepLifter);
    w.statics[f * ns_ + j] = v;
  }
}

// statics of frame t of an utterance of n frames at st (edge frames replicated)
__device__ __forceinline__ double stat_at(const double* st, int ns, long long t, long long n, int j) {
  t = t < 0 ? 0 : (t >= n ? n - 1 : t);
  return st[t * ns + j];
}

__device__ __forceinline__ double delta_at(const double* st, int ns, long long t, long long n, int j) {
  return (1.0 * (stat_at(st, ns, t + 1, n, j) - stat_at(st, ns, t - 1, n, j)) +
          2.0 * (stat_at(st, ns, t + 2, n, j) - stat_at(st, ns, t - 2, n, j))) / 10.0;
}

__global__ __launch_bounds__(256) void k_mfcc_deltas(MfccWs w, int n_utts, long long n_frames, int numCeps, int deltas, int accs,
                                                     int out_stride, float* __restrict__ out, const long long* __restrict__ out_offsets) {
  const int u = blockIdx.y;
  const int ns = numCeps + 1, ncols = ns * (1 + deltas + accs);
  const long long f0 = w.frame_off[u], f1 = min(w.frame_off[u + 1], n_frames);
  const long long n = f1 > f0 ? f1 - f0 : 0;
  const long long r0 = out_offsets[u], rows = out_offsets[u + 1] - r0;
  const double* st = w.statics + f0 * ns;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < rows * ncols; e += (long long)gridDim.x * blockDim.x) {
    const long long r = e / ncols;
    const int col = (int)(e - r * ncols), part = col / ns, j = col - part * ns;
    const long long t = r * out_stride;
    double v = 0.0;
    if (t < n) {
      if (part == 0) {
        v = st[t * ns + j];
      } else if (part == 1) {
        v = delta_at(st, ns, t, n, j);
      } else {
        v = (1.0 * (delta_at(st, ns, t + 1 < n ? t + 1 : n - 1, n, j) - delta_at(st, ns, t - 1 > 0 ? t - 1 : 0, n, j)) +
             2.0 * (delta_at(st, ns, t + 2 < n ? t + 2 : n - 1, n, j) - delta_at(st, ns, t - 2 > 0 ? t - 2 : 0, n, j))) / 10.0;
      }
    }
    out[(r0 + r) * ncols + col] = (float)v;
  }
}

}  // namespace

extern "C" size_t mgr_mfcc_ws_bytes(int n_utts, long long n_frames, int frameSize, int fftN, int numChans, int numCeps) {
  if (n_utts < 0 || n_frames < 0 || frameSize < 1 || fftN < 2 || numChans < 1 || numCeps < 0) return 0;
  return carve(nullptr, nullptr, n_utts, n_frames, frameSize, fftN, numChans, numCeps);
}

extern "C" int mgr_mfcc(mgr_ctx* c, const int16_t* samples, const int64_t* sample_offsets, int n_utts, long long n_frames, int frameSize,
                        int frameRate, int fftN, int numChans, int numCeps, int cepLifter, double preemph, int deltas, int accs,
                        int out_stride, const int32_t* loChan, const double* loWt, float* out, const int64_t* out_offsets, void* ws,
                        size_t ws_bytes) {
  MGR_REQUIRE(c && sample_offsets && loChan && loWt && out_offsets && ws, "null argument");
  mgr_planes_forget_range(c, ws, ws_bytes);   // (this call writes its workspace: kept weight planes in it are gone)
  MGR_REQUIRE(n_utts >= 1 && n_utts <= 65535, "n_utts must be in [1, 65535]");
  MGR_REQUIRE(n_frames >= 0 && n_frames < (1ll << 40), "bad n_frames");
  MGR_REQUIRE(fftN >= MFCC_MIN_FFT && fftN <= MFCC_MAX_FFT && (fftN & (fftN - 1)) == 0, "fftN must be a power of two in [256, 2048]");
  MGR_REQUIRE(frameSize >= 2 && frameSize <= fftN && frameRate >= 1, "need 2 <= frameSize <= fftN and frameRate >= 1");
  MGR_REQUIRE(numChans >= 2 && numChans <= MFCC_MAX_CHANS, "numChans must be in [2, 128]");
  MGR_REQUIRE(numCeps >= 1 && numCeps < MFCC_MAX_STATICS && numCeps <= numChans, "numCeps must be in [1, min(numChans, 63)]");
  MGR_REQUIRE(cepLifter >= 0 && preemph >= 0.0 && preemph < 1.0, "bad cepLifter / preemph");
  MGR_REQUIRE((deltas == 0 || deltas == 1) && (accs == 0 || accs == 1) && (accs <= deltas), "accelerations need deltas");
  MGR_REQUIRE(out_stride >= 1, "out_stride must be >= 1");
  MGR_REQUIRE(ws_bytes >= carve(nullptr, nullptr, n_utts, n_frames, frameSize, fftN, numChans, numCeps), "workspace too small");
  MGR_REQUIRE(n_frames == 0 || samples, "null samples");
  MfccWs w;
  carve(&w, (char*)ws, n_utts, n_frames, frameSize, fftN, numChans, numCeps);
  hipStream_t st = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_MISC);
  hipLaunchKernelGGL(k_mfcc_setup, dim3(1), dim3(256), 0, st, w, (const long long*)sample_offsets, n_utts, frameSize, frameRate, fftN,
                     numChans, numCeps, (const int*)loChan);
  MGR_LAUNCH_CHECK();
  if (n_frames > 0) {
    const int threads = fftN / 4 < 64 ? 64 : (fftN / 4 > 256 ? 256 : fftN / 4);   // one butterfly per thread per stage up to fftN 1024
    const size_t lds = sizeof(double) * (size_t)(2 * fftN + numChans);
    hipLaunchKernelGGL(k_mfcc_spectral, dim3((unsigned)n_frames), dim3(threads), lds, st, w, (const short*)samples,
                       (const long long*)sample_offsets, n_utts, n_frames, frameSize, frameRate, fftN, numChans, numCeps, cepLifter,
                       preemph, (const int*)loChan, loWt);
    MGR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_mfcc_deltas, dim3(16, (unsigned)n_utts), dim3(256), 0, st, w, n_utts, n_frames, numCeps, deltas, accs, out_stride,
                     out, (const long long*)out_offsets);
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}
