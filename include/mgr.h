/*
 * mgr.h - C ABI of libmgr.so: the MI355X (gfx950) BiLSTM + CTC training / decode hot path.
 *
 * The reference (AlexGidiotis/Multimodal-Gesture-Recognition-with-LSTMs-and-CTC) has NO native or FFI
 * interface: its hot path is whatever Keras 2.1.4 / TensorFlow 1.12.1 execute for the Python call sites
 * cited on each entry point below (paths relative to the reference root).  This header is therefore the
 * boundary the build defines: plain pointers and sizes, no framework types.  The Python host
 * (mgr_amd/_capi.py) binds it with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; mgr_last_error() (thread-local) explains.
 *   - all tensors are row-major fp32 unless stated; integer inputs are int32.
 *   - device pointers come from mgr_alloc(); the caller owns every buffer; the library keeps no caller
 *     pointer past the call.  Scratch is passed explicitly (ws, ws_bytes) - see the *_ws_bytes queries.
 *   - one mgr_ctx per device; calls on a ctx are serialised by the caller.  Kernels are enqueued on the
 *     ctx's CURRENT stream (mgr_stream_set, 8 streams); mgr_sync() waits for all of them.
 *   - LSTM weights use the "packed" gate-interleaved layout: column u*4+g of a packed matrix is column
 *     g*H+u of the Keras matrix (g in i,f,c,o).  mgr_lstm_pack converts both ways.  Z / dZ (gate
 *     pre-activations and their gradients) use the same interleaved column order.
 */
#ifndef MGR_H_
#define MGR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgr_ctx mgr_ctx;
typedef struct mgr_comm mgr_comm;

#define MGR_NUM_STREAMS 8
#define MGR_NUM_EVENTS 64
#define MGR_UNIQUE_ID_BYTES 128

/* ---- library / context ------------------------------------------------------------------------------ */
int mgr_version(void);
const char* mgr_last_error(void);
int mgr_device_count(int* n);
int mgr_ctx_create(int device, mgr_ctx** out);
int mgr_ctx_destroy(mgr_ctx* ctx);
/* name may be NULL */
int mgr_device_info(mgr_ctx* ctx, int* cu_count, size_t* hbm_bytes, char* name, int name_len);

/* ---- memory / streams / events ---------------------------------------------------------------------- */
int mgr_alloc(mgr_ctx* ctx, size_t bytes, void** dptr);
int mgr_free(mgr_ctx* ctx, void* dptr);
int mgr_memset(mgr_ctx* ctx, void* d, int byte, size_t n);
/* Keras feeds numpy arrays through feed_dict (multimodal_fusion/multimodal.py:264); these are that copy. */
int mgr_h2d(mgr_ctx* ctx, void* d, const void* h, size_t n);
/* Pinned host memory + a copy that does NOT synchronise: the host returns at once and the copy is ordered on the current
 * stream.  (mgr_h2d on pageable memory blocks the host, and on this runtime for as long as OTHER streams have work queued.) */
int mgr_host_alloc(mgr_ctx* ctx, size_t bytes, void** out);
int mgr_host_free(mgr_ctx* ctx, void* p);
int mgr_h2d_async(mgr_ctx* ctx, void* d, const void* h_pinned, size_t n);
int mgr_d2h(mgr_ctx* ctx, void* h, const void* d, size_t n);
/* The way back without a host stall: device -> pinned host memory (mgr_host_alloc), ordered on the current stream; the bytes are
 * valid once an event recorded behind the call has completed (mgr_event_record + mgr_event_sync).  What predict_generator's
 * pipeline downloads posteriors / decoded paths with while the next batch is computed (sequence_decoding.py:118-127). */
int mgr_d2h_async(mgr_ctx* ctx, void* h_pinned, const void* d, size_t n);
int mgr_event_sync(mgr_ctx* ctx, int ev);                 /* the host waits for event ev as last recorded */
int mgr_d2d(mgr_ctx* ctx, void* dst, const void* src, size_t n);
int mgr_sync(mgr_ctx* ctx);
int mgr_stream_set(mgr_ctx* ctx, int idx);
int mgr_stream_wait(mgr_ctx* ctx, int waiter, int waited); /* waiter waits for everything queued on waited */
/* Dispatch priority of stream idx: level 1 high, 0 default, -1 low (hipStreamCreateWithPriority).  The stream is recreated: it must be
 * idle (the call waits for it) and is best set before first use.  What it buys: when two streams have chip-filling GEMMs ready at the same
 * time, the workgroups of the higher-priority stream are placed first - the engine gives the stream that carries a training step's
 * dependent chain (fusion projections -> scan -> CTC -> BPTT -> dW -> Adam) the chip when the encoder stream has slack
 * (Schedule.chain_stream_priority). */
int mgr_stream_set_priority(mgr_ctx* ctx, int idx, int level);
int mgr_event_record(mgr_ctx* ctx, int ev);               /* on the current stream */
int mgr_stream_wait_event(mgr_ctx* ctx, int waiter, int ev); /* stream `waiter` waits for event ev as last recorded */
int mgr_event_elapsed_ms(mgr_ctx* ctx, int ev0, int ev1, float* ms);
/* Per-kernel-family device timing (HIP events around each launch, on the launch stream).
 * family ids: MGR_K_*.  mgr_prof_get syncs the device and returns accumulated launches / milliseconds. */
enum {
  MGR_K_GEMM_NN = 0, MGR_K_GEMM_TN = 1, MGR_K_GEMM_NT = 2, MGR_K_SCAN_FWD = 3, MGR_K_SCAN_BWD = 4,
  MGR_K_DENSE_FWD = 5, MGR_K_DENSE_BWD = 6, MGR_K_CTC = 7, MGR_K_ADAM = 8, MGR_K_MISC = 9, MGR_K_ALLREDUCE = 10,
  /* (round 6) multi-scan calls whose widest layer has H <= 128 - the fusion layer's own scan - are counted apart from the encoder
   * depths (MGR_K_SCAN_FWD): a roofline figure of the dominant kernel must not average it with a launch of 3 % of its FLOP */
  MGR_K_SCAN_FWD_NARROW = 11, MGR_K_COUNT = 12
};
int mgr_prof_enable(mgr_ctx* ctx, int family_mask);
int mgr_prof_get(mgr_ctx* ctx, int family, int* launches, float* ms);
int mgr_prof_reset(mgr_ctx* ctx);

/* ---- K1: GaussianNoise (multimodal_fusion/multimodal.py:103-106) ------------------------------------ */
/* Y = X + stddev * N(0,1), counter-based RNG keyed by (seed, element index).  X may equal Y. */
int mgr_add_gaussian_noise(mgr_ctx* ctx, const float* X, float* Y, size_t n, float stddev, uint64_t seed);
/* mask[i] = (uniform(seed,i) >= p) ? 1/(1-p) : 0  - Keras dropout mask (inverted dropout) */
int mgr_dropout_mask(mgr_ctx* ctx, float* mask, size_t n, float p, uint64_t seed);

/* ---- K1b: train-time sequence augmentation: a length-preserving time warp shared by the S streams of a sample, time /
 * feature masks per stream (SpecAugment), at most one blanked stream per sample (ModDrop), and K1's noise, in one pass per stream.
 * Both calls are deterministic functions of their arguments: no atomics, no workspace.
 *
 * The PLAN is one int32 row of len = K + 2 + 2 S (n_t + n_f) per sample (that is what the _plan_len call returns; 0 for counts out
 * of range):
 *   [0 .. K]                        q_0 .. q_K, the warp's target boundaries.  The source boundaries are a_j = j (T - 1) / K (integer
 *                                   division) and are not stored; q_j = a_j + d_j, d_j in [-D, D] for 0 < j < K, q_0 = 0, q_K = T - 1.
 *                                   2 D < min_j (a_{j+1} - a_j) is required (targets strictly increasing); K = 1 or D = 0: identity.
 *   [K + 1]                         the dropped stream's index, or -1
 *   [K + 2 + 2 (n_t + n_f) s ...]   stream s: n_t (start, width) pairs of time masks, then n_f pairs of feature masks.  A stream
 *                                   that uses fewer masks than the row has slots leaves the others at (0, 0).
 * DRAW ORDER: entry p of sample b's row is drawn from the 32-bit output u of the stateless generator of K1 (top half of the 64-bit
 * mix, as the dropout masks) at index b len + p under `seed`; entries that are not drawn (q_0, q_K, unused slots) leave their index
 * unused.  An integer in [lo, hi] is lo + ((uint64) u (hi - lo + 1) >> 32).  d_j: [-D, D] at p = j.  A mask's width: [0, W] at its
 * width entry; its start: [0, axis - width] at its start entry (axis T or the stream's F).  The dropped stream: r = u >> 8 at
 * p = K + 1; dropped when r < drop_thresh = (uint32) (stream_drop 2^24), the stream (r S) / drop_thresh from the same r.  No float
 * enters the plan.
 * stream_cfg: HOST array [S][MGR_AUGMENT_STREAM_COLS] = F, time masks used (<= n_t), Wt (<= T), feature masks used (<= n_f),
 * Wf (<= F) of each stream.  drop_thresh < 2^24, and 0 when S = 1.  T <= MGR_AUGMENT_MAX_T.
 *
 * The APPLY call, once per stream: Y[b, t, f] = noise(mask(warp(X))) over [B, T, F]; X != Y.  Frame t lies in the first segment j
 * with t <= q_{j+1}: num = (t - q_j) (a_{j+1} - a_j), den = q_{j+1} - q_j, i0 = a_j + num / den, rem = num % den.  rem == 0: the
 * value is X[b, i0, f] copied verbatim (-0.0, NaN payloads and denormals stay; row i0 + 1 is not read - at t = T - 1 there is none).
 * Otherwise frac = (float) rem / (float) den and the value is x0 + frac * (x1 - x0), each of the four operations rounded to float32
 * on its own (no fused multiply-add: a float32 restatement gives the same bits).  A frame inside a time mask of this stream, a
 * feature inside a feature mask, or every element when this stream is the sample's dropped one, becomes `fill`.  stddev > 0 adds
 * K1's noise under `seed`, keyed by the flat element index (b T + t) F + f with K1's pairing of elements 2i, 2i + 1 - each element of
 * a pair resolves its own (b, t, f) - so apply at stddev is bit for bit K1 over apply at stddev 0; stddev == 0 adds nothing.
 * T F < 2^31.  Device time of both calls: profiling family MGR_K_MISC. */
#define MGR_AUGMENT_MAX_SEGMENTS 16
#define MGR_AUGMENT_MAX_STREAMS 8
#define MGR_AUGMENT_MAX_MASKS 8
#define MGR_AUGMENT_MAX_T 32767
#define MGR_AUGMENT_STREAM_COLS 5
int mgr_augment_plan_len(int S, int K, int n_t, int n_f);
int mgr_augment_plan(mgr_ctx* ctx, int B, int T, int S, int K, int D, int n_t, int n_f, const int32_t* stream_cfg, uint32_t drop_thresh,
                     uint64_t seed, int32_t* plan);
int mgr_augment_apply(mgr_ctx* ctx, const float* X, float* Y, const int32_t* plan, int B, int T, int F, int S, int K, int n_t, int n_f,
                      int stream, float fill, float stddev, uint64_t seed);

/* ---- K1c: per-sample sequence lengths.  Zeroes buf[b, t, 0:row) for every t >= clip(seq_len[b], 0, T) of each job's
 * [B, T, row] float32 buffer (consecutive frames ld >= row floats apart; the ld - row floats between rows are not written) and
 * writes nothing else.  One launch per MGR_SEQ_MAX_JOBS jobs; its work is that of the tails: a sample with seq_len[b] >= T costs
 * the read of its length.  16-byte stores where row % 4 == 0, ld % 4 == 0 and buf is 16-byte aligned, single floats otherwise.
 * seq_len: DEVICE array of B int32, one for the call - every job has the same B (<= 65535); T may differ between jobs.
 * njobs == 0, B == 0 and T == 0 enqueue nothing.  A NULL buf or seq_len, row <= 0, ld < row or differing B are refused before
 * anything is enqueued.  What it is for: a reverse recurrence whose gate pre-activations Z [B, T, 4H] are zero in a sample's tail
 * keeps h = c = 0 through it and starts the real frames as if the sequence ended there; with its saved gates [B, T, H, 4] zeroed
 * there as well, the BPTT's dZ is exactly 0 in the tail.  No atomics, no workspace.  Profiling family MGR_K_MISC. */
#define MGR_SEQ_MAX_JOBS 16
typedef struct mgr_seq_fill_job {
  float* buf;
  int row, ld, B, T;
} mgr_seq_fill_job;
int mgr_seq_zero_tail(mgr_ctx* ctx, int njobs, const mgr_seq_fill_job* jobs, const int32_t* seq_len);

/* ---- K2/K3/K7: Bidirectional(LSTM) (multimodal_fusion/multimodal.py:109-118,159-168;
 *      audio_network/speech_lstm_ctc_words.py:56-77; skeletal_network/skeletal_lstm_ctc.py:309-335) ---- */
/* Keras layout <-> packed layout for a [rows, 4H] matrix (W: rows=F, U: rows=H, b: rows=1). */
int mgr_lstm_pack(mgr_ctx* ctx, const float* src, float* dst, int rows, int H, int to_keras);
/* dst[c][r] = src[r][c] */
int mgr_transpose(mgr_ctx* ctx, const float* src, float* dst, int rows, int cols);
/* Gate pre-activations for all T:  Z[b,t,:] = (X[b,t,:F] (.) mask4[g,b,:]) . Wp + bp   (f32 MFMA GEMM).
 * X has row stride ldx floats (>= F).  mask4 [4,B,F] may be NULL (no input dropout).  Z is [B,T,4H] packed order. */
int mgr_lstm_input_proj(mgr_ctx* ctx, const float* X, int ldx, const float* mask4, const float* Wp,
                        const float* bp, float* Z, int B, int T, int F, int H);
/* The same for BOTH directions of a Bidirectional layer (multimodal.py:159-168: two LSTMs over the same input, each with
 * its own kernel, bias and dropout masks) as one GEMM over 8H columns when that saves column tiles (4H = 400: 7 instead
 * of 2 x 4); otherwise it is two mgr_lstm_input_proj calls.  Results are identical to the two calls. */
int mgr_lstm_input_proj_pair(mgr_ctx* ctx, const float* X, int ldx, const float* mask4_fwd, const float* Wp_fwd,
                             const float* bp_fwd, float* Z_fwd, const float* mask4_rev, const float* Wp_rev,
                             const float* bp_rev, float* Z_rev, int B, int T, int F, int H);
/* The same projection for a layer with Keras input dropout at rate drop_rate (the rate only selects the kernel; mask4
 * holds the actual factors, 0 or 1/(1-p)): from drop_rate >= 0.3 on (and 16 <= F <= 2048) the K loop runs per gate
 * over the kept features only (gemm.hip, k_gemm_nn_sparse) - the same sums with the zero terms left out, i.e. equal to
 * mgr_lstm_input_proj up to fp32 summation order.  ws from mgr_lstm_input_proj_dropout_ws_bytes (index lists, rebuilt by
 * every call).  MGR_TUNE_PROJ_DENSE = 1 keeps the dense kernel. */
size_t mgr_lstm_input_proj_dropout_ws_bytes(int B, int F, int H);
int mgr_lstm_input_proj_dropout(mgr_ctx* ctx, const float* X, int ldx, const float* mask4, float drop_rate,
                                const float* Wp, const float* bp, float* Z, int B, int T, int F, int H, void* ws,
                                size_t ws_bytes);
/* The same projection from a TRANSPOSED copy of the layer input, XT[b][f][t] with row stride ldt (T padded to a multiple of
 * 128, zeros behind T; mgr_transpose_bt writes it): a kept feature is then a contiguous row, and the kernel's A operand is
 * staged with coalesced 16-byte loads instead of one scattered 4-byte load per element.  Only for shapes the dropout-aware
 * kernel handles - mgr_lstm_input_proj_dropout_wants_transposed says whether a copy is worth making for (drop_rate, F).
 * x_absmax: a bound on |XT|, or 0 if there is none.  With a bound the products run on the f16 matrix pipe with every f32 operand
 * split into an f16 (hi, lo) pair of its scaled value and f32 accumulation (22+ significant bits per operand: gemm.hip,
 * k_gemm_nn_sparse16; the representation error is below the rounding an f32 accumulation of the same length commits).
 *   x_absmax > 0: a bound the CALLER states.  It is checked on the device in front of the product (k_absmax_gate: one pass over
 *     XT); data that would leave the f16 range at the scale the bound implies make the call fall back - on the device, without a
 *     host round trip - to the f32 MFMA kernel, so a wrong bound costs time, never Inf / NaN in Z.
 *   x_absmax < 0: |x_absmax| is a bound the PRODUCER of XT guarantees by construction - the transposed copies the scans of this
 *     library write (mgr_scan_job.YT) hold h = o * tanh(c), |h| <= 1, or the sum of two of them (residual input), <= 2 - and no
 *     check is made.  This is what the engine passes for the buffers its own scans fill.
 *   0, or MGR_TUNE_GEMM_F32 = 1: v_mfma_f32_32x32x2_f32.
 * mask4 may be NULL (no dropout: inference): with a bound the plain dense projection on the f16 pipe (k_gemm_nn_dense16: one
 * K loop over all features, the A tile staged once for the four gates; MGR_TUNE_PROJ_DENSE16_MASKED = 2 takes it with a mask as
 * well, the mask factors folded into the weight tiles), without one the f32 kernel over all features. */
int mgr_lstm_input_proj_dropout_wants_transposed(mgr_ctx* ctx, float drop_rate, int F);
int mgr_lstm_input_proj_dropout_t(mgr_ctx* ctx, const float* XT, int ldt, const float* mask4, float drop_rate,
                                  const float* Wp, const float* bp, float* Z, int B, int T, int F, int H, void* ws,
                                  size_t ws_bytes, float x_absmax);
int mgr_transpose_bt(mgr_ctx* ctx, const float* X, int ldx, float* XT, int ldt, int B, int T, int F);
/* The same projection from a PRE-SPLIT transposed copy (round 5; gemm_split.hip).  XS has the shape and strides of XT - [B][F][ldt]
 * floats' worth of bytes - but the 4 ldt bytes of row (b, f) hold ldt f16 values hi(t) followed by ldt f16 values lo(t) with
 * x 2^13 = hi + lo, hi = rn_f16(x 2^13), lo = rn_f16(x 2^13 - hi): the split-f16 operand pair of the f16 matrix pipe, made ONCE by
 * whoever produces the activations instead of by every product that reads them.  Producers: the scans (mgr_scan_job.yt_split - their
 * outputs are bounded by construction: |h| <= 1, with a residual sum <= 2) and mgr_transpose_bt_split (any row-major tensor with
 * |x| < 7.99; a larger value overflows the f16 range and shows as Inf / NaN).  ldt % 128 == 0, zero behind T.
 * The kernel is a loader + matrix pipeline: both operands travel HBM -> LDS by LDS-DMA through a three-stage ring (no register
 * staging, no conversion), fragments come out of LDS with transposed reads, the waves issue nothing but those and MFMAs.
 * mask4: entries 0 or ONE common factor c (what mgr_dropout_mask and Keras' Dropout produce: c = 1 / (1 - rate)); checked on the
 * device - two different factors in one call make Z NaN (the factor is applied once, in the epilogue).  NULL: no dropout.
 * drop_rate is informative only.  16 <= F <= 2048. */
size_t mgr_lstm_input_proj_dropout_ts_ws_bytes(int B, int F, int H);
int mgr_lstm_input_proj_dropout_ts(mgr_ctx* ctx, const float* XS, int ldt, const float* mask4, float drop_rate,
                                   const float* Wp, const float* bp, float* Z, int B, int T, int F, int H, void* ws,
                                   size_t ws_bytes);
/* XS[b][f] = the split row (above) of X[b][0..T)[f], zero for t in [T, ldt); ldt % 8 == 0. */
int mgr_transpose_bt_split(mgr_ctx* ctx, const float* X, int ldx, float* XS, int ldt, int B, int T, int F);
/* the same with entry t of a row = X[b, t + tshift, f] (tshift in {-1, 0, 1}; zero where that step does not exist) */
int mgr_transpose_bt_split_shift(mgr_ctx* ctx, const float* X, int ldx, float* XS, int ldt, int B, int T, int F, int tshift);
/* Frozen weights: frozen != 0 promises that the contents of Wp (a packed input-weight matrix passed to mgr_lstm_input_proj_dropout_ts) do
 * not change until the next call of this function for the same pointer; the (hi, lo) weight planes and the largest |W| that
 * mgr_lstm_input_proj_dropout_ts leaves in its workspace are then reused by later calls with the same (Wp, workspace, B, F, H) instead of
 * being rebuilt (the frozen encoders of the fusion network, multimodal_fusion/multimodal.py:118-130: 4 of the 6 conversions of a step).
 * Every call (either value) drops what was kept for Wp - call it again after rewriting the weights.  Host-side state only.
 *   Kept planes are forgotten (the next call with that key rebuilds them) by every library call that writes bytes they lie in:
 *   mgr_memset, mgr_h2d, mgr_h2d_async and mgr_d2d into that range (a pointer into the workspace included), every entry point given
 *   that workspace (or a range over it) as its own ws, and mgr_lstm_input_proj_dropout_ts with another key on it.  mgr_free of a buffer
 *   ends the promise of every weight inside it and forgets every plane kept in it.  Copies into Wp itself do not forget: a rewrite
 *   behind the promise goes unnoticed.  proj_ws of mgr_lstm_param_grads_dropout_ts is only read.  Writes the library cannot see - an
 *   output argument of another call pointing into the workspace, the caller's own kernels - must not touch a workspace with kept planes.
 *   Ordering is the caller's, as for any reuse of a workspace (every call rewrites its lists and mask-factor word): a call on another
 *   stream that reuses kept planes must be ordered after the call that built them (an event, mgr_stream_wait). */
int mgr_weight_planes_cache(mgr_ctx* ctx, const float* Wp, int frozen);
/* Recurrence. reverse=1 walks t = T-1..0 and writes outputs at their original t (Bidirectional backward
 * sub-layer).  Y[b,t,0:H] with row stride ldy gets h_t (+ R[b,t,0:H] with stride ldr when R != NULL: the
 * residual add / concat fusion of multimodal.py:111,117,155).  gates [B,T,H,4] (i,f,g,o after activation) and
 * cs [B,T,H] are saved for BPTT when non-NULL.  ws from mgr_lstm_scan_ws_bytes (may be 0/NULL). */
size_t mgr_lstm_scan_ws_bytes(int B, int T, int H);
int mgr_lstm_scan_fwd(mgr_ctx* ctx, const float* Z, const float* Up, float* Y, int ldy, const float* R,
                      int ldr, float* gates, float* cs, int B, int T, int H, int reverse, void* ws,
                      size_t ws_bytes);
/* Several independent recurrences (e.g. audio fwd/rev + skeletal fwd/rev of one encoder depth) in ONE call.
 * Layers whose recurrent matrix does not fit one CU (H = 300, 500) run as a single persistent multi-CU launch
 * (clusters of CUs exchanging h_t each step, lstm_cluster.hip); sharing the launch keeps every spinning
 * workgroup co-resident.  Fields as in mgr_lstm_scan_fwd.  ws from mgr_lstm_scan_multi_ws_bytes. */
typedef struct mgr_scan_job {
  const float* Z;
  const float* Up;
  /* NULL together with a YT: write ONLY the transposed copy (a caller whose every reader takes YT - the pre-split / transposed
   * projection and weight-gradient products - saves the scan a store stream of B T H floats in 16-byte pieces).  The K-split multi-CU
   * kernels then skip their row store; every other kernel family still writes rows, because the transpose behind it reads them: into
   * scratch from ws (mgr_lstm_scan_fwd_multi_ws_bytes counts it for exactly those jobs, mgr_lstm_scan_multi_ws_bytes for every job
   * without Y).  ldy is not looked at.  Y == NULL and YT == NULL is an error; so is a workspace without room for the scratch - both
   * are refused before anything is enqueued. */
  float* Y;
  const float* R;
  float* gates;
  float* cs;
  int ldy, ldr, B, T, H, reverse;
  /* optional transposed copy of the output, written by the scan itself (the K-split multi-CU kernel stages 32 steps per lane
   * in LDS and stores 128-byte row segments; any other kernel family is followed by a transpose inside the call):
   * YT[b * ytb + u * ldt + t] = what Y[b, t, u] gets, u < H; t in [T, ldt) is written as zero (the buffer may arrive dirty).
   * ldt % 4 == 0, ldt >= T rounded up to 32.  NULL: none.  This is the layout mgr_lstm_input_proj_dropout_t / mgr_lstm_param_grads_dropout_t
   * read; with ytb > H * ldt several jobs fill column ranges of one wider [B][F][ldt] copy. */
  float* YT;
  long long ytb;
  int ldt;
  /* yt_split != 0: the rows of YT are written in the SPLIT ROW FORMAT of mgr_lstm_input_proj_dropout_ts - row (b, u) holds ldt f16
   * values hi(t) followed by ldt f16 values lo(t) of y 2^13 - instead of ldt floats: what the pre-split products read without
   * converting anything (the scan's outputs are bounded by construction: |h| <= 1, with a residual input <= 2).  ldt % 8 == 0. */
  int yt_split;
} mgr_scan_job;
size_t mgr_lstm_scan_multi_ws_bytes(int njobs, const mgr_scan_job* jobs);
int mgr_lstm_scan_fwd_multi(mgr_ctx* ctx, int njobs, const mgr_scan_job* jobs, void* ws, size_t ws_bytes);
/* Explicit launch options of the two multi-scan calls (round 6; the same calls, with the choices a scheduler makes PER CALL passed
 * as arguments instead of through context-wide tune keys, and with the launch number handed back).
 *   struct_size  sizeof(mgr_scan_launch_opts) of the CALLER's header: members beyond it are taken as zero, so the struct can grow.
 *   form         forward call: MGR_SCAN_FORM_*; backward call: MGR_BPTT_FORM_*.  AUTO (0) = what MGR_TUNE_SCAN_FORM /
 *                MGR_TUNE_BPTT_FORM say.
 *   seq_out      host word (ordinary or page-locked memory; NULL: not wanted) that receives, BEFORE the call returns, the launch
 *                number of the persistent multi-CU launch this call enqueued - what mgr_stream_wait_resident takes - or MGR_SEQ_NONE
 *                when the call enqueued no launch that enters the residency ledger (single-CU kernels, fallbacks).  With a word from
 *                mgr_host_alloc this is the hand-over for a wait that was enqueued BEFORE the launch it waits for
 *                (mgr_stream_wait_resident_word). */
enum { MGR_SCAN_FORM_AUTO = 0, MGR_SCAN_FORM_PLAIN = 1, MGR_SCAN_FORM_FUSED = 3,
       MGR_SCAN_FORM_FUSED_ANY = 4 };   /* FUSED: launches that do not fit one workgroup per CU as they are; FUSED_ANY: every launch the
                                         * fused kernel can run (a narrow layer then holds ceil(G / 2) whole CUs per cluster).  2 (the
                                         * retired pair form) is refused. */
enum { MGR_BPTT_FORM_AUTO = 0, MGR_BPTT_FORM_TRIMMED = 1, MGR_BPTT_FORM_YIELDING = 2, MGR_BPTT_FORM_DIRECT = 3,   /* MGR_TUNE_BPTT_FORM = 0 / 1 / 2 */
       /* round 6, narrow layers (16 < H <= 128) with an exchange: 8-wave workgroups that run TWO unit groups of their cluster, a CU each
        * (H = 100: 32 workgroups instead of 56), with the trimmed step / the direct gather inside; the same bits as every other form.  A
        * launch that does not qualify takes the trimmed / direct form. */
       MGR_BPTT_FORM_FUSED = 4, MGR_BPTT_FORM_FUSED_DIRECT = 5,
       /* round 6, the directions of ONE narrow layer (same shape, H in {32, 64, 100}): one 8-wave workgroup per (direction, 16-sample
        * group) that holds the whole recurrent matrix as f16 (hi, lo) fragments and keeps dh in registers - NO inter-CU exchange, so its
        * step does not depend on what the rest of the chip does to the L2 / fabric (lstm_cu_bwd.hip).  Same arithmetic as the multi-CU
        * forms with another summation order: equal to them to rounding, not bit for bit.  A call that does not qualify takes the
        * trimmed multi-CU form.  mgr_scan_bwd_job.dzmax is filled by a reduction pass behind the kernel. */
       MGR_BPTT_FORM_SINGLE_CU = 6 };
#define MGR_SEQ_NONE 0xFFFFFFFFu
typedef struct mgr_scan_launch_opts {
  unsigned struct_size;
  int form;
  unsigned* seq_out;
} mgr_scan_launch_opts;
int mgr_lstm_scan_fwd_multi_ex(mgr_ctx* ctx, int njobs, const mgr_scan_job* jobs, void* ws, size_t ws_bytes,
                               const mgr_scan_launch_opts* opts);
/* The workspace mgr_lstm_scan_fwd_multi_ex needs for exactly this call in this context (its tune keys, opts->form): what
 * mgr_lstm_scan_multi_ws_bytes says, less the row scratch of the jobs without Y whose kernel writes YT itself.  Plans the call with
 * the launcher's own code and enqueues nothing.  0: a bad job list (mgr_last_error). */
size_t mgr_lstm_scan_fwd_multi_ws_bytes(mgr_ctx* ctx, int njobs, const mgr_scan_job* jobs, const mgr_scan_launch_opts* opts);
/* ABI guard for bindings that fill mgr_scan_job / mgr_scan_bwd_job / mgr_scan_launch_opts field by field: the sizes the LIBRARY was
 * built with (round 5 appended mgr_scan_bwd_job.dzmax and turned mgr_scan_job's reserved word into yt_split; revision 7 appended
 * mgr_scan_bwd_job.dbsum and the dbsum / proj_ws / HsT arguments of mgr_lstm_param_grads_dropout_ts - a caller built against
 * an older header must not pass its structs to this library).  out[0..2] = sizeof of the three structs, out[3] =
 * MGR_ABI_REVISION. */
#define MGR_ABI_REVISION 7
int mgr_abi_struct_sizes(unsigned out[4]);
/* Tuning / test hooks: context-wide keys set with mgr_tune, 0 by default.  Keys 5, 6, 17, 22 and 23 are unused; mgr_tune refuses
 * the settings of retired forms (key 4 = 2, key 17 != 0) rather than run the default under their name. */
enum {
  /* 0 auto, 1 force the L2-streaming fallback kernels, 2 force one workgroup per batch group (no inter-CU exchange) where it fits,
   * 3 force clusters with 4 tiles per workgroup, 4 same with 8 tiles per workgroup. */
  MGR_TUNE_SCAN_PATH = 0,
  MGR_TUNE_SCAN_SYNC_CHECK = 1,     /* != 0: the multi-scan calls check the give-up word synchronously */
  MGR_TUNE_SCAN_PRINT_PLAN = 2,     /* != 0: print the forward scan plan */
  /* 1 = K-split scan launches keep contiguous cluster ids and write-through publishes (no XCD-local exchange). */
  MGR_TUNE_SCAN_NO_XCD_LOCAL = 3,
  /* form of the split-f16 K-split scan launches (mgr_lstm_scan_fwd_multi[_ex] with form AUTO): 3 = launches that do not fit ONE
   * workgroup per CU as they are (config F's encoder depths: 408 workgroups) take the FUSED form: 8-wave workgroups that run two unit
   * groups of their cluster, a CU each (208), bit-identical; the CUs they leave free are what 4-wave persistent launches of other
   * streams get - the admission ledger then counts those by the CUs they need two to a CU, and their caller starts them once the
   * fused launch is resident (mgr_stream_wait_resident) so that they do land there.  Any other value: the plain form. */
  MGR_TUNE_SCAN_FORM = 4,
  MGR_TUNE_SCAN_LDS_IMAGE = 7,      /* one-tile-per-wave clusters: 0 = K-split step (register-direct gather), 1 = LDS-image step */
  /* 1 = the multi-CU BPTT keeps its 4-wave kernel instead of the split-role (4 compute + 4 gather waves) one, 2 = always split. */
  MGR_TUNE_BPTT_SPLIT_ROLE = 8,
  MGR_TUNE_PROJ_DENSE = 9,          /* 1 = mgr_lstm_input_proj_dropout always takes the dense kernel */
  /* 2 = mgr_lstm_input_proj_dropout_t with a bound on |XT| takes the dense-K split-f16 kernel with a mask as well. */
  MGR_TUNE_PROJ_DENSE16_MASKED = 10,
  /* 2 = mgr_lstm_input_proj_dropout from row-major X takes 128-unit tiles instead of 64: faster alone, slower in the training step
   * (its 512-thread workgroups need two free wave slots on all four SIMDs of a CU at once). */
  MGR_TUNE_PROJ_WIDE_TILES = 11,
  /* mgr_lstm_input_proj_dropout_ts tile: 0 = the library's choice, 1 = 128 x 64 (4 waves, two workgroups per CU), 2 = 128 x 128
   * (8 waves). */
  MGR_TUNE_PROJ_TS_TILE = 12,
  /* 1 = mgr_dense_softmax_fwd / mgr_dense_bwd keep their LDS-tiled vector-ALU kernels where the matrix-core forms would run. */
  MGR_TUNE_DENSE_VALU = 13,
  /* K-split scan step: 0 = recurrent product on the f16 matrix pipe with every f32 operand split into an f16 (hi, lo) pair and f32
   * accumulation (22+ significant bits per operand; lstm_cluster.hip cluster_run_k16), 1 = v_mfma_f32_16x16x4_f32. */
  MGR_TUNE_SCAN_F32_MFMA = 14,
  /* 1 = the transposed-input projection / parameter-gradient GEMMs keep their f32 MFMA kernels whatever bound the caller states. */
  MGR_TUNE_GEMM_F32 = 15,
  /* form of the narrow-layer (H <= 128) BPTT with form AUTO.  1 = the BPTT launched next runs BESIDE persistent scans of another
   * stream: it takes the form that yields to them (two barriers, partial sums through LDS) instead of the one trimmed along its
   * dependent chain, which is faster alone (H = 100: 1.77 against 2.29 us per step) and costs the step beside them; same results bit
   * for bit.  The engine sets it from its schedule (a deterministic choice: it never depends on what happens to be running).
   * 2 = the direct gather: every wave fetches the words of its own cells from all sources, no partial sums through LDS, one barrier
   * per step - the fastest form alone (1.58 us per step), 4.7 x the texture-path traffic: for launches that have CUs of their own
   * (beside fused encoder scans).  All three forms give the same bits. */
  MGR_TUNE_BPTT_FORM = 16,
  /* 1 = mgr_ctc_loss_grad runs one sample per workgroup (rounds 1 - 5); 0 = two (from B = 2 on: the alpha / beta chains of a
   * workgroup's two samples on its four SIMDs - 32 workgroups for config F's 64 samples, which the 48 CUs beside fused encoder scans
   * hold one per CU); the same bits. */
  MGR_TUNE_CTC_ONE_SAMPLE = 18,
  /* 1 = mgr_lstm_scan_bwd_multi[_ex] with form AUTO takes MGR_BPTT_FORM_SINGLE_CU where it qualifies (A/B of whole runs). */
  MGR_TUNE_BPTT_SINGLE_CU = 19,
  /* KiB of LDS the CTC recurrence kernel (20) / the CTC per-frame kernels (21) ask for at least (0: what they use).  A placement hint
   * for callers that run mgr_ctc_loss_grad / mgr_head_fwd_bwd beside persistent scan launches of another stream: a workgroup that
   * asks for more LDS than a scan workgroup leaves on its CU lands on a CU without one (engine.py sets 96 / 64 for such steps). */
  MGR_TUNE_CTC_CHAIN_LDS_KIB = 20,
  MGR_TUNE_CTC_FRAME_LDS_KIB = 21,
  MGR_TUNE_COUNT = 24
};
int mgr_tune(mgr_ctx* ctx, int key, int value);
int mgr_tune_get(mgr_ctx* ctx, int key, int* value);   /* what a key is set to (a host of the library that lays out buffers by it) */
/* Health of the persistent multi-CU scans launched on this context since the last mgr_scan_status_clear: *out receives the OR
 * of their status bits.  MGR_SCAN_GAVE_UP: a bounded spin expired (a dead-locked or lost peer) - the launch returned promptly
 * but its outputs are garbage; the call FAILS (mgr_last_error).  MGR_SCAN_NONFINITE: a hidden state became NaN / Inf (diverged
 * weights, bad checkpoint): the output Y of that (sample, unit) is NaN from that time step on (the multi-CU exchange feeds 0 back
 * in its place - a NaN word cannot travel through the hand-off - so the OTHER units of the sample stay finite where the
 * reference's would turn NaN one step later; whoever consumes the outputs must treat the whole pass as NaN, as Engine.read_loss
 * does); the call succeeds.  Ordered on the current stream; cheap (one 4-byte read back) - call it where results are consumed,
 * e.g. with the loss. */
enum { MGR_SCAN_GAVE_UP = 1, MGR_SCAN_NONFINITE = 8 };
int mgr_scan_status(mgr_ctx* ctx, unsigned* out);
/* The same read without the failure: out[0] = status bits, out[2] = optimizer updates skipped by the update gate (below) since
 * the last clear, out[1] = out[3] = 0. */
int mgr_scan_status_ex(mgr_ctx* ctx, unsigned out[4]);
/* Forget the recorded status bits and the skipped-update count (enqueued on the current stream), e.g. after restoring a good
 * checkpoint. */
int mgr_scan_status_clear(mgr_ctx* ctx);
/* Several engines may share one context: each binds its OWN status block (>= 64 zeroed bytes from mgr_alloc, 16-byte aligned)
 * before it enqueues work; scans launched while a block is bound report into it and mgr_scan_status* / the update gate read
 * it.  NULL binds the context's own block again.  Host-side state only (no stream order).
 * Words of a block: [0] status bits, [2] skipped updates, [8, 16) WHICH samples met a non-finite hidden state - bit (b mod 256) of
 * the 256-bit field is set together with MGR_SCAN_NONFINITE by the scan that saw sample b of its job go NaN / Inf, so that a
 * consumer can hand out NaN for exactly those samples (Engine.predict: a block of its own per inference pass). */
int mgr_scan_status_bind(mgr_ctx* ctx, void* block);
/* Test hook: OR `bits` into the bound status block on the current stream, as a scan that gave up would. */
int mgr_scan_status_inject(mgr_ctx* ctx, unsigned bits);
/* Update gate: keeps a bad step away from the weights WITHOUT a host round trip (the host reads the status with the loss, by
 * which time the optimizer kernels of the same step are already queued).  mgr_update_gate_eval writes flag[0] = 1.0f if
 * (status bits & mask) else 0.0f on the current stream - put flag behind the gradient buffer and it travels with the gradient
 * all-reduce, so that every replica takes the same decision (sum > 0 on all ranks if any rank raised it).  While a flag is set
 * with mgr_update_gate_set (host-side state; NULL = gate open), mgr_adam_step and mgr_maxnorm_cols read it on the device and
 * leave parameters and moments untouched when it is non-zero; each skipped mgr_adam_step is counted (mgr_scan_status_ex). */
int mgr_update_gate_eval(mgr_ctx* ctx, unsigned mask, float* flag);
int mgr_update_gate_set(mgr_ctx* ctx, const float* flag);
/* Placement aid (never a correctness dependency): the current stream waits, on the device, until every workgroup of the NEXT
 * persistent scan launched on this context (on any stream) has started, or timeout_us (<= 100000) has passed.  Chip-filling
 * GEMMs enqueued behind it therefore arrive when the scan is resident instead of racing its workgroups for the CUs. */
int mgr_stream_wait_next_resident(mgr_ctx* ctx, int timeout_us);
/* The same for ONE given launch: `seq` is the context's count of persistent launches (mgr_persist_stats: `launches`) read right
 * before that launch was enqueued, plus one.  Lets a stream wait for a launch that is already enqueued on another stream. */
int mgr_stream_wait_resident(mgr_ctx* ctx, unsigned seq, int timeout_us);
/* The same when the wait has to be enqueued BEFORE the launch it is for (the launch sits later in the host's order, on another
 * stream): `seq_word` is a word of page-locked host memory (mgr_host_alloc) that the caller sets to 0 before this call and that the
 * launch's call fills in (mgr_scan_launch_opts.seq_out = seq_word).  The wait kernel polls the word until it is non-zero, then waits
 * for that launch's residency as mgr_stream_wait_resident does; MGR_SEQ_NONE releases it at once.  Bounded like the others. */
int mgr_stream_wait_resident_word(mgr_ctx* ctx, const unsigned* seq_word, int timeout_us);
/* Counters of the residency waits of this context since it was created (read on the current stream, a 16-byte read-back):
 * out[0] = waits enqueued that have finished, out[1] = those that ran into their timeout (a wait whose launch never came, came too
 * late, or could not become resident while the wait held its stream: each costs its full bound - silently, which is why this exists),
 * out[2], out[3] = diagnostics of the LAST wait that expired: the launch number it was for (0: its word was never filled) and the low
 * 32 bits of the address of the word it polled (0: a wait for a known number). */
int mgr_resident_wait_stats(mgr_ctx* ctx, unsigned out[4]);
/* Persistent launches on different streams are admitted against the chip's workgroup slots; one that would not fit beside the
 * launches still in flight is ordered behind them (co-residency by construction).  Counters: launches so far, and how many of
 * them had to be serialised that way. */
int mgr_persist_stats(mgr_ctx* ctx, int* launches, int* serialised);
/* Diagnostic: out[b] = XCC (XCD) id the workgroup b of a (nblocks, threads, lds_bytes) launch ran on. */
int mgr_probe_xcc(mgr_ctx* ctx, int nblocks, int threads, int lds_bytes, int32_t* out);
/* Diagnostic: what a guest kernel of the shape of a collective (RCCL all-reduce: a few workgroups, tens of KiB of LDS, ~100 us)
 * experiences on the current stream, e.g. beside resident persistent scans: a 1-block marker launch followed by the guest
 * (nblocks x threads, lds_bytes of dynamic LDS, every block busy for ~us microseconds).  out[0], out[1] = the marker's start /
 * end, out[2 + 2b], out[3 + 2b] = start / end of guest block b, all in ticks of the 100 MHz device wall clock.  out: device,
 * 2 + 2 * nblocks int64. */
int mgr_probe_guest(mgr_ctx* ctx, int nblocks, int threads, int lds_bytes, int us, int64_t* out);
/* Diagnostic (tools/overlap_probe.py): hold the current stream for ~us microseconds on the device (bounded; 0 <= us <= 100000). */
int mgr_stream_delay(mgr_ctx* ctx, int us);
/* BPTT: dY[b,t,0:H] (row stride lddy) is dLoss/dh_t from above; Y (stride ldy) is the layer's own output as
 * written by scan_fwd WITHOUT residual (needed only through gates/cs here).  Produces dZ [B,T,4H] packed. */
int mgr_lstm_scan_bwd(mgr_ctx* ctx, const float* dY, int lddy, const float* gates, const float* cs,
                      const float* Up, float* dZ, int B, int T, int H, int reverse, void* ws, size_t ws_bytes);
/* Several BPTT recurrences (both directions of a Bidirectional layer) in ONE call; layers with a multi-CU
 * instantiation run as a single persistent launch of CU clusters exchanging dz_t each step (lstm_cluster_bwd.hip). */
typedef struct mgr_scan_bwd_job {
  const float* dY;
  const float* gates;
  const float* cs;
  const float* Up;
  float* dZ;
  int lddy, B, T, H, reverse;
  /* optional: dzmax[b * 4H + col] = the largest |dZ[b, t, col]| over t as float bits - what mgr_lstm_param_grads_dropout_ts scales
   * the rows of dZ^T by.  The multi-CU kernel keeps it in four registers of the thread that owns a (sample, unit) for all T steps
   * (free); any other kernel family is followed by a reduction pass inside the call.  NULL: not wanted. */
  unsigned* dzmax;
  /* optional: dbsum[b * 4H + col] = sum over t of dZ[b, t, col], added in step order - the bias gradient's per-sample partial sums
   * (mgr_lstm_param_grads_dropout_ts takes them in place of its own pass over dZ).  Kept by the multi-CU kernels like dzmax, in four
   * more registers; any other kernel family: the same reduction pass.  NULL: not wanted. */
  float* dbsum;
} mgr_scan_bwd_job;
size_t mgr_lstm_scan_bwd_multi_ws_bytes(int njobs, const mgr_scan_bwd_job* jobs);
int mgr_lstm_scan_bwd_multi(mgr_ctx* ctx, int njobs, const mgr_scan_bwd_job* jobs, void* ws, size_t ws_bytes);
int mgr_lstm_scan_bwd_multi_ex(mgr_ctx* ctx, int njobs, const mgr_scan_bwd_job* jobs, void* ws, size_t ws_bytes,
                               const mgr_scan_launch_opts* opts);   /* opts->form: MGR_BPTT_FORM_* */
/* What a multi-scan call launches, as a value: the decision the two *_multi_ex calls carry out (csrc/scan_choice.h), made by pure
 * host functions of the CU count, the tune keys (tune[0 .. ntune), keys beyond ntune read as 0), the job list and opts->form.  The
 * describe calls need no context and no GPU and enqueue nothing; they check the job list and the form like the calls themselves
 * (same return code, same mgr_last_error) and fill *out, whose struct_size the caller has set to sizeof *out.  Pointers of the jobs
 * are looked at (NULL or not, alignment), never followed.
 *   kernel     forward MGR_SCAN_FWD_*, backward MGR_SCAN_BWD_*: the persistent cluster kernel of the call; NONE (0): no such launch
 *   grid, block, lds_bytes   its launch; waves per workgroup, workgroups per_cu, live workgroups (forward: those that run a cluster)
 *   ledger     the launch takes a place in the residency ledger (opts->seq_out gets its number; else MGR_SEQ_NONE)
 *   need       workspace bytes of exactly this call; base_need: header + exchange images; zero_bytes: what is zeroed ahead of the launch
 *   degraded   forward: ws_bytes < base_need kept the jobs off the cluster kernels
 *   single_cu  backward: the call is ONE launch of the single-CU split-f16 kernel (fallback CU16 for every job)
 *   job[i]     cluster: runs in the cluster kernel, as nbg clusters of G unit groups on `members` workgroups each, laid out by cls_*;
 *              else fallback MGR_SCAN_FALLBACK_*.  yt_in_kernel: the kernel writes the transposed copy (else a transpose follows);
 *              rows_in_scratch: the job gave no Y and its rows go to the workspace at rows_off; xbuf_off: its exchange images. */
enum { MGR_SCAN_CHOICE_MAX_JOBS = 8 };
enum { MGR_SCAN_FWD_NONE = 0, MGR_SCAN_FWD_IMAGE = 1, MGR_SCAN_FWD_KS = 2, MGR_SCAN_FWD_KS_S = 3, MGR_SCAN_FWD_K16 = 4, MGR_SCAN_FWD_K16_S = 5,
       MGR_SCAN_FWD_K16_FUSED = 6 };
enum { MGR_SCAN_BWD_NONE = 0, MGR_SCAN_BWD = 1, MGR_SCAN_BWD_S = 2, MGR_SCAN_BWD_SPLIT = 3, MGR_SCAN_BWD_16 = 4, MGR_SCAN_BWD_16_S = 5,
       MGR_SCAN_BWD_16_SL = 6, MGR_SCAN_BWD_16_SD = 7, MGR_SCAN_BWD_16_SPLIT = 8, MGR_SCAN_BWD_16_F = 9, MGR_SCAN_BWD_16_FD = 10 };
enum { MGR_SCAN_FALLBACK_NONE = 0, MGR_SCAN_FALLBACK_SIMPLE = 1, MGR_SCAN_FALLBACK_MFMA = 2, MGR_SCAN_FALLBACK_MFMA_JOINT = 3,
       MGR_SCAN_FALLBACK_CU16 = 4 };
typedef struct mgr_scan_choice_job {
  int cluster, fallback, nw, tpw, G, nbg, members, cls_begin, cls_nclusters, cls_cluster0, cls_rot, yt_in_kernel, rows_in_scratch, reserved;
  unsigned long long xbuf_off, rows_off;
} mgr_scan_choice_job;
typedef struct mgr_scan_choice {
  unsigned struct_size;
  int njobs, kernel, grid, block, lds_bytes, waves, per_cu, live, xcd_local, fused, exchange, ksplit, split16, split, single_cu, ledger, degraded;
  unsigned long long base_need, need, zero_bytes;
  mgr_scan_choice_job job[MGR_SCAN_CHOICE_MAX_JOBS];
} mgr_scan_choice;
/* ws_bytes: the workspace the call would be given ((size_t)-1: as much as it takes - then need is what
 * mgr_lstm_scan_fwd_multi_ws_bytes says in a context with these tune keys) */
int mgr_lstm_scan_fwd_describe(int cu_count, const int* tune, int ntune, int njobs, const mgr_scan_job* jobs,
                               const mgr_scan_launch_opts* opts, size_t ws_bytes, mgr_scan_choice* out);
int mgr_lstm_scan_bwd_describe(int cu_count, const int* tune, int ntune, int njobs, const mgr_scan_bwd_job* jobs,
                               const mgr_scan_launch_opts* opts, mgr_scan_choice* out);
/* Parameter gradients from dZ (all packed layouts, f32 MFMA split-K GEMMs, deterministic slab reduce):
 *   dWp[F,4H] = sum_rows (X (.) mask4)^T dZ ;  dUp[H,4H] = sum_rows hprev^T dZ ;  dbp[4H] = sum_rows dZ
 * Hs is the layer's own un-residualed output h (row stride ldh); hprev is its time-shifted view. */
size_t mgr_lstm_param_grads_ws_bytes(int B, int T, int F, int H);
int mgr_lstm_param_grads(mgr_ctx* ctx, const float* X, int ldx, const float* mask4, const float* Hs, int ldh,
                         const float* dZ, float* dWp, float* dUp, float* dbp, int B, int T, int F, int H,
                         int reverse, void* ws, size_t ws_bytes);
/* The same with Keras input dropout at rate drop_rate on X (mask4 holds the factors): from drop_rate >= 0.3 and F >= 128 on,
 * dW is computed per (gate, sample) over the rows of the kept features only and gathered in sample order (gemm.hip,
 * k_gemm_tn_sparse / k_dw_gather); dU and db as in mgr_lstm_param_grads.  Equal to it up to fp32 summation order. */
size_t mgr_lstm_param_grads_dropout_ws_bytes(int B, int T, int F, int H);
int mgr_lstm_param_grads_dropout(mgr_ctx* ctx, const float* X, int ldx, const float* mask4, float drop_rate,
                                 const float* Hs, int ldh, const float* dZ, float* dWp, float* dUp, float* dbp, int B,
                                 int T, int F, int H, int reverse, void* ws, size_t ws_bytes);
/* The dropout-aware dW from the TRANSPOSED activation copy XT[b][f][0..ldt) (mgr_transpose_bt - the copy the forward
 * projection mgr_lstm_input_proj_dropout_t was fed): the K dimension of dW is time, so both operands (XT rows of the kept
 * features; dZ transposed into the workspace by this call) are read as contiguous float4 along t.  Results bit-identical
 * to mgr_lstm_param_grads_dropout.  Only for shapes where ..._wants_transposed() says 1; ldt % 4 == 0, ldt >= T rounded
 * up to 16, the pad zero.
 * x_absmax: as for mgr_lstm_input_proj_dropout_t - with a bound on |XT| (and ldt >= T rounded up to 32) the dW product runs on the
 * f16 matrix pipe with split-f16 (hi, lo) operands and f32 accumulation (k_gemm_tn_sparse16; dZ is scaled per (sample, gate
 * column) by its own largest magnitude, so its dynamic range costs nothing); then equal to mgr_lstm_param_grads_dropout to the
 * f32 tolerance instead of bit for bit.  > 0: checked on the device, f32 MFMA kernel if violated; < 0: guaranteed by the producer of
 * XT, unchecked; 0, or MGR_TUNE_GEMM_F32 = 1: the f32 MFMA kernel. */
int mgr_lstm_param_grads_dropout_wants_transposed(mgr_ctx* ctx, float drop_rate, int F);
size_t mgr_lstm_param_grads_dropout_t_ws_bytes(int B, int T, int F, int H, int ldt);
int mgr_lstm_param_grads_dropout_t(mgr_ctx* ctx, const float* XT, int ldt, const float* mask4, float drop_rate,
                                   const float* Hs, int ldh, const float* dZ, float* dWp, float* dUp, float* dbp, int B,
                                   int T, int F, int H, int reverse, void* ws, size_t ws_bytes, float x_absmax);
/* The same from a PRE-SPLIT transposed copy XS (the format of mgr_lstm_input_proj_dropout_ts, ldt % 32 == 0): dW on the f16 matrix pipe
 * as a loader + matrix pipeline (gemm_split.hip, k_dw_split) - dZ is transposed into the workspace as split rows scaled per (sample,
 * gate column) by that row's own largest magnitude.  mask4: entries 0 or ONE common factor (checked on the device; else dW is NaN).
 * 16 <= F <= 2048.  dU / db as in mgr_lstm_param_grads. */
size_t mgr_lstm_param_grads_dropout_ts_ws_bytes(int B, int T, int F, int H, int ldt);
int mgr_lstm_param_grads_dropout_ts(mgr_ctx* ctx, const float* XS, int ldt, const float* mask4, float drop_rate,
                                    const float* Hs, int ldh, const float* dZ, float* dWp, float* dUp, float* dbp, int B,
                                    int T, int F, int H, int reverse, void* ws, size_t ws_bytes, const unsigned* dzmax,
                                    const float* dbsum, const void* proj_ws, const float* HsT);
/* (dzmax: the row maxima of dZ if the BPTT left them - mgr_scan_bwd_job.dzmax - or NULL: this call finds them with one more pass.
 *  dbsum: the per-sample sums of dZ over time if the BPTT left them - mgr_scan_bwd_job.dbsum - then db = their sum over the samples in
 *  sample order; or NULL: db from a pass over dZ, as in mgr_lstm_param_grads.
 *  proj_ws: the workspace of the mgr_lstm_input_proj_dropout_ts call that projected with the SAME mask4 (same B, F, H), untouched since -
 *  its kept lists are used instead of being built again; or NULL.
 *  HsT: the rows h_prev in the split row format - mgr_transpose_bt_split_shift of this direction's outputs Hs with tshift = -1 (forward) /
 *  +1 (reverse), [B][H][ldt] - then dU is formed like dW, on the f16 matrix pipe against the same dZ^T rows (16 <= H); or NULL: the f32
 *  product of mgr_lstm_param_grads.) */
/* dX[b,t,0:F] (stride lddx) (+)= sum_g mask4[g] (.) (dZ_g . W_g^T); accumulate=1 adds into dX. */
int mgr_lstm_input_grad(mgr_ctx* ctx, const float* dZ, const float* Wp, const float* mask4, float* dX,
                        int lddx, int accumulate, int B, int T, int F, int H);

/* ---- K5: Dropout -> Dense -> softmax (multimodal_fusion/multimodal.py:171-179) ---------------------- */
/* P[B,T,C] = softmax((A (.) dm) . Wd + bd).  A has row stride lda.  The dropout mask dm is either the
 * explicit array dmask[B,T,D] (parity runs) or, when dmask==NULL and p>0, generated in-kernel from
 * (seed, element index) exactly as mgr_dropout_mask would; p==0 & dmask==NULL means no dropout. */
int mgr_dense_softmax_fwd(mgr_ctx* ctx, const float* A, int lda, const float* dmask, float p, uint64_t seed,
                          const float* Wd, const float* bd, float* P, int B, int T, int D, int C);
size_t mgr_dense_bwd_ws_bytes(int B, int T, int D, int C);
/* dWd[D,C], dbd[C], dA[B,T,D] (stride ldda) from dLogits[B,T,C]. */
int mgr_dense_bwd(mgr_ctx* ctx, const float* A, int lda, const float* dmask, float p, uint64_t seed,
                  const float* dLogits, const float* Wd, float* dWd, float* dbd, float* dA, int ldda, int B,
                  int T, int D, int C, void* ws, size_t ws_bytes);
/* The whole head of a training step behind ONE entry point - a host-side sequence of four launches on the context's stream
 * (k_dense_softmax_fwd*, k_ctc, k_mean, k_dense_bwd*), NOT a fused kernel: Dropout -> Dense -> softmax (P written), CTC loss +
 * gradient, Dense backward, and the mean loss if loss_mean != NULL (written between the CTC kernel and the Dense backward, so a
 * read-back of it does not wait for the backward).  Reference: multimodal_fusion/multimodal.py:171-179 (Dropout / Dense / Activation('softmax')), losses.py:4-15
 * (ctc_lambda_func) and Keras' backward pass through them.  Bit for bit the results of mgr_dense_softmax_fwd + mgr_ctc_loss_grad
 * (+ mgr_mean) + mgr_dense_bwd with the same arguments; dLogits [B,T,C] is a required scratch / output; ws >= mgr_head_ws_bytes. */
size_t mgr_head_ws_bytes(int B, int T, int D, int C, int Lmax);
int mgr_head_fwd_bwd(mgr_ctx* ctx, const float* A, int lda, const float* dmask, float p, uint64_t seed, const float* Wd, const float* bd,
                     const int32_t* labels, const int32_t* input_len, const int32_t* label_len, int B, int T, int D, int C, int Lmax,
                     int skip, int blank, float eps, float gscale, float* P, float* loss, float* loss_mean, float* dLogits, float* dWd,
                     float* dbd, float* dA, int ldda, void* ws, size_t ws_bytes);

/* ---- K6: ctc_lambda_func (multimodal_fusion/losses.py:4-15 -> K.ctc_batch_cost -> tf.nn.ctc_loss) ---- */
/* CTC on P[:, skip:, :] with y = softmax(log(P+eps)); labels int32 [B,Lmax] padded -1; blank = C-1 in the
 * reference.  loss[B] = -log p(l|x).  dLogits[B,T,C] (may be NULL) = gscale * dloss_b/d(Dense logits),
 * zero on dropped / out-of-length frames.  Edge cases: label_len 0 is accepted (the single state is the blank, as in
 * tf.nn.ctc_loss); a label sequence that does not fit its input length (tf.nn.ctc_loss raises "Not enough time for target
 * transition sequence") yields loss = +inf and a ZERO gradient for that sample, the other samples of the batch are unaffected.
 * Out-of-range arguments are clipped, not rejected: input_len into [0, T - skip], label_len into [0, Lmax], label values into
 * [0, C - 1]; the results are those of the call with the clipped arguments, bit for bit.  input_len 0 (no frames) yields loss = +inf
 * and a zero gradient as well. */
size_t mgr_ctc_ws_bytes(int B, int T, int C, int Lmax);
int mgr_ctc_loss_grad(mgr_ctx* ctx, const float* P, const int32_t* labels, const int32_t* input_len,
                      const int32_t* label_len, int B, int T, int C, int Lmax, int skip, int blank, float eps,
                      float gscale, float* loss, float* dLogits, void* ws, size_t ws_bytes);
/* Entropy-regularised CTC (Liu et al., NeurIPS 2018): the loss and, beside it, the entropy H_b = -sum_pi q(pi) ln q(pi) of the
 * distribution q(pi) = p(pi) / p(labels | x) over the feasible alignments pi of sample b's labels, in nats, with the gradient of
 * loss_scale * loss - ent_scale * H.  Conventions, clipping of out-of-range arguments and edge cases are K6's, argument for argument.
 *   loss    [B]: the bits mgr_ctc_loss_grad writes.
 *   entropy [B]: H = ln p(labels | x) - E_q[ln p(pi)] >= 0; 0 for label_len 0 (one alignment).
 *   dLogits [B,T,C] (may be NULL: the two values only) = loss_scale * dloss_b/dlogits - ent_scale * dH_b/dlogits, overwritten, zero on
 *           dropped / out-of-length frames.  ent_scale == 0 skips the entropy term: dLogits is then mgr_ctc_loss_grad's with gscale =
 *           loss_scale, bit for bit (entropy is still written).
 * A label sequence that does not fit its input, or an input length of 0: loss = +inf, entropy = 0 and a zero gradient for that sample
 * alone.  Lmax <= 255.  Deterministic; samples are independent of each other; no atomics.
 * Workspace: ws_bytes >= 2 * mgr_ctc_ws_bytes(B, T, C, Lmax) - there is no query of its own.  The first half is the loss's layout
 * (emissions, alpha, beta); the second half holds two more rows of alpha's size and format, the entropy of the prefixes into a state
 * beside alpha and of the suffixes out of it beside beta.  With dLogits == NULL or ent_scale == 0 the first half is left as
 * mgr_ctc_loss_grad leaves it; otherwise its alpha and beta rows hold each state's value relative to the frame's largest, with what the
 * float32 recursion rounded away put back - the same occupancies, more digits of them.  Device time: profiling family MGR_K_CTC. */
int mgr_ctc_entropy_grad(mgr_ctx* ctx, const float* P, const int32_t* labels, const int32_t* input_len, const int32_t* label_len, int B,
                         int T, int C, int Lmax, int skip, int blank, float eps, float loss_scale, float ent_scale, float* loss,
                         float* entropy, float* dLogits, void* ws, size_t ws_bytes);

/* ---- K7: Adam(clipvalue) + maxnorm (multimodal_fusion/multimodal.py:159-168,206-213) ---------------- */
/* g' = clip(g*gscale, +-clipvalue) (clipvalue<=0: no clip); m,v,p Keras-Adam update with step size lr_t. */
int mgr_adam_step(mgr_ctx* ctx, float* p, const float* g, float* m, float* v, size_t n, float lr_t, float b1,
                  float b2, float eps, float clipvalue, float gscale);
/* per column j of W[rows,cols]: W[:,j] *= clip(n_j,0,maxv)/(eps+n_j), n_j = ||W[:,j]||_2 */
int mgr_maxnorm_cols(mgr_ctx* ctx, float* W, int rows, int cols, float maxv, float eps);
/* Out[r, 0:cols] = A[r, 0:cols] + Bm[r, 0:cols] with independent row strides (layers.add, multimodal.py:111) */
int mgr_add2d(mgr_ctx* ctx, const float* A, int lda, const float* Bm, int ldb, float* Out, int ldo, size_t rows,
              int cols);
/* out[0] = mean(x[0:n]) */
int mgr_mean(mgr_ctx* ctx, const float* x, int n, float* out);

/* ---- K8: data parallel gradient all-reduce (not in the reference; BASELINE.json config 4) ----------- */
int mgr_comm_unique_id(uint8_t id[MGR_UNIQUE_ID_BYTES]);
int mgr_comm_init_rank(mgr_ctx* ctx, int nranks, int rank, const uint8_t id[MGR_UNIQUE_ID_BYTES], mgr_comm** out);
int mgr_allreduce_sum(mgr_comm* comm, float* dbuf, size_t n); /* in place, on the ctx's current stream */
int mgr_allreduce_max(mgr_comm* comm, float* dbuf, size_t n);
int mgr_comm_destroy(mgr_comm* comm);
/* What RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank), not what the caller passed to
 * mgr_comm_init_rank: bench.py prints it, so that a multi-GPU line proves from the library's side that N ranks met.
 * The gradient all-reduce's device time is profiling family MGR_K_ALLREDUCE (events on the stream it is enqueued on). */
int mgr_comm_count(mgr_comm* comm, int* nranks_seen, int* rank_seen);

/* ---- K9: decode (multimodal_fusion/sequence_decoding.py:38-53; audio_network/sequence_decoding.py:38-53) */
/* best[b,t-skip] = argmax_c P[b,t,c] (first index on ties, numpy semantics), prob = that max. */
int mgr_frame_argmax(mgr_ctx* ctx, const float* P, int B, int T, int C, int skip, int32_t* best, float* prob);
/* CTC prefix beam search (K.ctc_decode(greedy=False, beam_width) semantics; BASELINE.json config 5).
 * out[B,T-skip] padded -1 holds the best path (after merge_repeated collapse when merge_repeated!=0). */
size_t mgr_ctc_beam_ws_bytes(int B, int T, int C, int beam);
int mgr_ctc_beam_search(mgr_ctx* ctx, const float* P, const int32_t* input_len, int B, int T, int C, int skip,
                        int blank, int beam, float eps, int merge_repeated, int32_t* out, int32_t* out_len,
                        double* logp, void* ws, size_t ws_bytes);
/* The same search with a label bigram and an N-best list.  The semantics are those of mgr_ctc_beam_search with
 * merge_repeated = 0 (a prefix is the labelling), plus:
 *   ext [(C+1)*C] double (device): the bonus for appending label c after label p is ext[(p+1)*C + c]; row 0 is the empty prefix, the
 *                  column `blank` is never read.  Every live beam carries the sum of ext over its prefix and a candidate ranks by
 *                  lse(p_blank, p_nonblank) + that sum; an extension whose entry is -inf is no candidate (a hard grammar).  Ties and
 *                  -inf candidates as in mgr_ctc_beam_search.  Entries must be finite or -inf: the caller checks, the tables are
 *                  device memory.
 *   fin [C+1] double (device) or NULL: added once after the last frame, indexed by last label + 1 (0 = empty prefix).  It takes no
 *                  part in the pruning: the at most `beam` live beams are ranked again by total + fin (ties to the better rank
 *                  before; a beam whose sum is -inf is dropped) and the first top_paths are written.
 *   out [B,top_paths,T-skip] padded -1; out_len [B,top_paths], -1 where fewer than top_paths hypotheses survive; score [B,top_paths]
 *   = the network's log-probability + the bonuses, -inf where out_len = -1; logp_ctc [B,top_paths] the network's part alone.
 * input_len 0 gives the empty prefix with logp_ctc = 0 and score = fin[0].  beam <= 32, C <= 64, 1 <= top_paths <= beam.  With
 * all-zero tables the hypotheses and scores are those of mgr_ctc_beam_search bit for bit.  Deterministic; samples are independent. */
size_t mgr_ctc_beam_lm_ws_bytes(int B, int T, int C, int beam, int top_paths);
int mgr_ctc_beam_search_lm(mgr_ctx* ctx, const float* P, const int32_t* input_len, int B, int T, int C, int skip, int blank, int beam,
                           float eps, const double* ext, const double* fin, int top_paths, int32_t* out, int32_t* out_len,
                           double* score, double* logp_ctc, void* ws, size_t ws_bytes);

/* ---- K11: locating gestures in time.  The reference "spots and classifies gestures from two continuous streams" and keeps
 * only the label sequence (sequence_decoding.py:38-53 of each network); these two calls keep the frame positions as well. ---- */
/* Viterbi forced alignment: the single most probable CTC alignment of each sample's label sequence.  Conventions are those of
 * mgr_ctc_loss_grad, argument for argument: P[:, skip:, :], y = softmax(log(P+eps)), labels int32 [B,Lmax] padded -1 (values outside
 * the class range are clipped into it, as there), blank = C-1 in the reference, ws >= mgr_ctc_align_ws_bytes.
 *   path [B,T-skip] int32: the class emitted at each frame (a label or blank); -1 from input_len on.
 *   seg  [B,Lmax,2] int32: first and last frame (inclusive, indices of the ORIGINAL sequence: t + skip) at which label k is
 *                          emitted; -1 for k >= label_len.  Blank stretches are not reported.
 *   conf [B,Lmax] float:   mean of P[b,t,l_k] (the raw softmax, what the reference's threshold looks at) over those frames; 0 for
 *                          k >= label_len.
 *   logp [B] double:       natural-log probability of the path under y.
 * Ties: a back-pointer tie takes the smallest step (stay, one state, two states), a tie of the two final states the last blank; the
 * step over two states is allowed only onto a label that differs from the previous one, as in the loss.  Edge cases: label_len 0
 * gives an all-blank path and no segments; a label sequence that does not fit its input length (where the loss is +inf), or an
 * input length of 0, gives logp = -inf, path and seg -1, conf 0 for that sample, the other samples of the batch are unaffected.
 * Deterministic; samples are independent of each other (a sample's result does not depend on the rest of the batch). */
size_t mgr_ctc_align_ws_bytes(int B, int T, int C, int Lmax);
int mgr_ctc_align(mgr_ctx* ctx, const float* P, const int32_t* labels, const int32_t* input_len, const int32_t* label_len, int B, int T,
                  int C, int Lmax, int skip, int blank, float eps, int32_t* path, int32_t* seg, float* conf, double* logp, void* ws,
                  size_t ws_bytes);
/* The greedy decode of K9 with its frame positions, all on the device: frame argmax (first index on ties), the reference's confidence
 * filter in its net effect (sequence_decoding.py:45-48: for every label s the first k_s frames whose best label is s are dropped, k_s
 * = the number of frames whose best label is s with probability < thr, compared in float32; thr < 0: no filter), then the collapse of
 * equal neighbours among the surviving frames.  Per sample: n_runs [B] = the number of runs - the TRUE count, also when it exceeds cap -
 * and for run r < min(n_runs, cap): lab [B,cap] its label (blank runs are kept), seg [B,cap,2] the original indices (t + skip) of its
 * first and last surviving frame, conf [B,cap] the mean of the frame maxima over its surviving frames; rows n_runs <= r < cap hold
 * -1, -1, 0.  n_runs can reach T - skip.  Needs no workspace (the per-frame arrays live in LDS): T - skip <= MGR_SEGMENTS_MAX_FRAMES. */
#define MGR_SEGMENTS_MAX_FRAMES 8192
int mgr_greedy_segments(mgr_ctx* ctx, const float* P, int B, int T, int C, int skip, float thr, int cap, int32_t* n_runs, int32_t* lab,
                        int32_t* seg, float* conf);

/* ---- K17 / K18: posterior gesture extents and the frame-overlap (Jaccard) counts. ---- */
/* Forward-backward state posteriors of each sample's label sequence and extents read off them at a quantile: where mgr_ctc_align reports
 * the frames of the single best alignment, this call weighs every alignment.  Conventions are those of mgr_ctc_loss_grad and
 * mgr_ctc_align, argument for argument (P[:, skip:, :], y = softmax(log(P+eps)), labels [B,Lmax] padded -1 and clipped into the class
 * range, input_len / label_len clipped), and alpha, beta and logp are the loss's own: the call runs the loss's emission and chain
 * kernels inside the loss's workspace, ws >= mgr_ctc_ws_bytes(B, T, C, Lmax).  States are l' = [blank, l_1, blank, ..., l_L, blank],
 * S = 2 * Lmax + 1 columns; gamma(t, s) = P(state s at frame t | labels, posteriors), each frame normalised by its own sum.
 *   gamma [B,T-skip,S] float or NULL: 0 from input_len on and for states >= 2 * label_len + 1.
 *   seg   [B,Lmax,2] int32: with cum(t, s) = sum_{s' >= s} gamma(t, s'), first_i = min{t : cum(t, 2i+1) >= q} (label i has begun with
 *                           probability >= q) and last_i = max{t : cum(t, 2i+2) <= 1 - q} (it has not ended with probability >= q), as
 *                           indices of the ORIGINAL sequence (t + skip), inclusive; q = quantile in (0, 0.5].  first_i <= last_i and
 *                           first_i < first_{i+1}; below q = 0.5 neighbouring extents may overlap (they are credible intervals).
 *                           cum is formed from the float32 values that go to gamma, added one at a time in float32 from state S - 1
 *                           downwards and compared with (float)q and 1.0f - (float)q: seg is a function of gamma alone, and the same
 *                           whether gamma is asked for or not.  -1 for i >= label_len.
 *   occ   [B,Lmax] float:   sum_t gamma(t, 2i+1), the expected number of frames in label i, summed in ascending t; 0 for i >= label_len.
 *   conf  [B,Lmax] float:   sum_t gamma(t, 2i+1) P[b,t+skip,l_i] / occ_i - mgr_ctc_align's conf weighted by the posterior.
 *   logp  [B] double:       ln p(labels | posteriors) = -loss of mgr_ctc_loss_grad.
 * Edge cases as mgr_ctc_align: label_len 0 gives no segments and all of gamma in state 0; a label sequence that does not fit its input,
 * or an input length of 0, gives logp = -inf, seg -1, occ, conf and gamma 0 for that sample alone.  Deterministic; samples are
 * independent of each other.  Lmax <= 255. */
int mgr_ctc_occupancy(mgr_ctx* ctx, const float* P, const int32_t* labels, const int32_t* input_len, const int32_t* label_len, int B, int T,
                      int C, int Lmax, int skip, int blank, float eps, float quantile, float* gamma, int32_t* seg, float* occ, float* conf,
                      double* logp, void* ws, size_t ws_bytes);
/* Per sample and class, the number of frames covered by the hypothesis segments and the reference segments of that class: their
 * intersection, their union and each side's own count (all [B,C] int32, exact) - inter / uni is the Jaccard index of the class.
 * hyp_lab [B,Sh], hyp_seg [B,Sh,2], ref_lab [B,Sr], ref_seg [B,Sr,2] (first and last frame, inclusive), n_frames [B], all device memory.
 * A segment with a label outside [0, C), a label in ignore_mask (bit l = class l, as mgr_edit_distance's) or first < 0 is skipped;
 * extents are clipped to [0, n_frames); segments of one class on one side are united, segments of different classes may overlap.
 * C <= 64, Sh and Sr <= 4096.  Needs no workspace. */
int mgr_segment_overlap(mgr_ctx* ctx, const int32_t* hyp_lab, const int32_t* hyp_seg, int Sh, const int32_t* ref_lab, const int32_t* ref_seg,
                        int Sr, const int32_t* n_frames, int B, int C, uint64_t ignore_mask, int32_t* inter, int32_t* uni,
                        int32_t* hyp_frames, int32_t* ref_frames);

/* ---- K13: lexicon-constrained CTC decode: the best PHRASE sequence whose word expansion the posteriors support - HTK
 * HVite's token pass over a phrase lexicon composed with the CTC topology, with an optional prior over phrase sequences.  The audio
 * network's classes are words, its gestures phrases of words (audio_network/data_generator.py: class_2_words).
 * The lexicon is G phrases; phrase g is the word sequence phrase_words[phrase_off[g] .. phrase_off[g+1]-1] (n_g >= 1 words, each a class
 * in [0, C) other than blank).  phrase_off [G+1] and phrase_words [phrase_off[G]] are HOST memory - the one pair of pointers of this
 * call that is: they are checked entry by entry on every call and travel to the kernel as arguments.  Everything else is device memory.
 * Emissions are the loss's and the aligner's: frames skip .., ln y = ln softmax(log(P + eps)).  For a phrase sequence Q = (g_1 .. g_m),
 * m = 0 allowed,
 *     score(Q) = A(words(Q)) + sum_i ext[prev_i + 1][g_i] + fin[g_m + 1]
 * where A is the Viterbi forced-alignment log-probability of the concatenated words - exactly mgr_ctc_align's logp: the step over a
 * blank only between different words, within and across phrases -, ext [(G+1)*G] double has row 0 = "start of sequence" (prev_1 = -1),
 * fin [G+1] double or NULL has index 0 = "empty sequence" (g_0 = -1).  The table conventions are mgr_ctc_beam_search_lm's: entries are
 * finite or -inf, -inf forbids the transition (a hard grammar and a soft bigram are the same table), THE CALLER refuses NaN and +inf.
 * The call returns argmax_Q score(Q), computed exactly as one Viterbi pass over this state graph:
 *   INIT     blank, before any phrase          W(g,k)   emits word k of phrase g
 *   B(g,k)   k < n_g - 1: blank inside g       Z(g)     blank behind phrase g (per phrase: a bigram keeps its history)
 * Into frame t every state may stay; W(g,k>0) is entered from B(g,k-1), and from W(g,k-1) if the two words differ; B(g,k) from W(g,k);
 * Z(g) from W(g,n_g-1); W(g,0) from INIT + ext[0][g] (also applied at t = 0), from Z(g') + ext[g'+1][g], and from W(g',n_g'-1) +
 * ext[g'+1][g] if that word differs from w[g][0].  The final score is the maximum of INIT + fin[0], W(g,n_g-1) + fin[g+1] and Z(g) +
 * fin[g+1].  1 + 2 * n_words states; the lexicon need not be uniquely decodable.  The search compares f32 values (the tables rounded
 * to f32); what it reports is summed again in fp64 over the path and the fp64 tables.  Finite table entries must therefore lie within
 * the f32 range, |x| <= FLT_MAX: a larger negative one would round to -inf and forbid what the definition allows, a larger positive
 * one to +inf.  THE CALLER checks that too (decoding.phrase_lm_tables does).
 * Outputs: n_phr [B] the TRUE number of phrases, also when it exceeds cap (as mgr_greedy_segments); phr [B,cap] padded -1; seg
 * [B,cap,2] the original frame indices (t + skip) of the phrase's first word's first frame and its last word's last frame; conf [B,cap]
 * the mean of P[t, emitted word] over the phrase's non-blank frames (0 where phr = -1); path [B,T-skip] or NULL: the class emitted per
 * frame, -1 from input_len on; logp [B] the network's part of the score (the fp64 sum of ln y over the path), score [B] = logp + the
 * table terms.  input_len 0 gives the empty sequence, logp = 0, score = fin[0] (0 without fin).  A sample for which no sequence has a
 * finite score gets n_phr = -1, score = logp = -inf, phr / seg / path rows -1, conf 0; the other samples are unaffected.
 * Ties: the smaller back-pointer wins - stay, then from the state before, then the step over a blank; for W(g,0): stay, INIT, then the
 * phrases g' in order, Z(g') before W(g',n_g'-1) - and among equal final scores the first state in lexicon order (INIT, then per word
 * the word before its blank).  Deterministic; a sample's result does not depend on the rest of the batch.
 * G <= MGR_LEXICON_MAX_PHRASES, n_words <= MGR_LEXICON_MAX_WORDS (511 states), C <= 64, T - skip <= MGR_SEGMENTS_MAX_FRAMES, cap >= 1.
 * Parity with HVite itself is unpinned: HTK is not available to this project. */
#define MGR_LEXICON_MAX_PHRASES 64
#define MGR_LEXICON_MAX_WORDS   255
/* The workspace for a lexicon of G phrases: phrase_off [G+1] is the HOST array the decode call takes (its last entry is n_words). */
size_t mgr_ctc_lexicon_ws_bytes(int B, int T, int C, int G, const int32_t* phrase_off);
int mgr_ctc_lexicon_decode(mgr_ctx* ctx, const float* P, const int32_t* input_len, int B, int T, int C, int skip, int blank, float eps,
                           const int32_t* phrase_off, const int32_t* phrase_words, int G, const double* ext, const double* fin, int cap,
                           int32_t* n_phr, int32_t* phr, int32_t* seg, float* conf, int32_t* path, double* score, double* logp, void* ws,
                           size_t ws_bytes);

/* ---- K14: CTC hypothesis scoring: what rescoring N-best lists across modalities needs from each of them - the CTC
 * likelihood of K label sequences per sample in one launch.
 *     logp[b,k] = ln sum over all CTC alignments pi of hypothesis k of prod_t y[t, pi_t]
 * over the frames skip .. skip + Tp - 1, Tp = input_len[b] clipped into [0, T - skip], y = (P + eps) / sum_c (P + eps): blank, skip,
 * eps and - without a lexicon - the clipping of labels into the class range are those of mgr_ctc_loss_grad / mgr_ctc_align, and for a
 * hypothesis a label row of the loss could hold logp is -loss.  fp64, natural-log units (the recursion runs on renormalised f32
 * values in base-2 units, what it subtracted is summed in fp64).
 * hyp [B,K,Lh] int32 / hyp_len [B,K] int32 (device) are laid out as mgr_ctc_beam_search_lm writes out / out_len: rows of any width Lh
 * <= MGR_RESCORE_MAX_WIDTH, only the first hyp_len entries of a row are read (a length above Lh counts as Lh), a length < 0 means "no
 * hypothesis in this slot".
 * Lexicon: phrase_off [G+1] / phrase_words (HOST memory, as in K13; checked entry by entry at every call by K13's rules; C <= 64) or
 * NULL, NULL, 0.  With a lexicon the entries of hyp are PHRASE ids and the hypothesis is the concatenation of its phrases' words - a
 * blank is forced only between equal neighbouring words, within and across phrases; the expansion happens on the device.
 * Results: logp [B,K] double, n_lab [B,K] int32 or NULL = the number of labels after expansion.
 *   absent slot                                   logp -inf, n_lab -1
 *   labels + forced blanks > Tp (also Tp = 0)     logp -inf, n_lab the expanded count
 *   a phrase id outside [0, G)                    logp NaN ("not scored"), n_lab -1
 *   more than MGR_RESCORE_MAX_LABELS labels       logp NaN, n_lab the expanded count
 *   the empty hypothesis                          logp = sum_t ln y[t, blank] (0 at Tp = 0), n_lab 0
 * The workspace holds the class-major emissions, computed once per sample and shared by its hypotheses; its size does not depend on
 * the lexicon (the query takes it for symmetry with the call).  No atomics: deterministic, and a sample's row does not depend on the
 * rest of the batch.  B <= 65535. */
#define MGR_RESCORE_MAX_LABELS 255
#define MGR_RESCORE_MAX_WIDTH  65536
size_t mgr_ctc_rescore_ws_bytes(int B, int T, int C, int G, const int32_t* phrase_off);
int mgr_ctc_rescore(mgr_ctx* ctx, const float* P, const int32_t* input_len, int B, int T, int C, int skip, int blank, float eps,
                    const int32_t* phrase_off, const int32_t* phrase_words, int G, const int32_t* hyp, const int32_t* hyp_len, int K,
                    int Lh, double* logp, int32_t* n_lab, void* ws, size_t ws_bytes);

/* ---- K19: joint decode over several CTC streams: a LABEL-synchronous prefix search - Graves' prefix search with the CTC
 * prefix score - over gesture sequences that every stream scores at every step.  Streams may differ in frame count, frame rate and
 * class set; nothing is frame-synchronous.
 * Streams: 1 <= M <= MGR_JOINT_MAX_STREAMS entries of the struct below.  Stream m has posteriors P [B,T,C] float32 and input_len [B]
 * (device), skip, blank, eps, a weight w_m > 0, and an optional lexicon phrase_off [G+1] / phrase_words (HOST memory, K13's rules, C <=
 * 64; both NULL: none).  Hypotheses are sequences over G gesture ids, G <= MGR_LEXICON_MAX_PHRASES.  In a stream with a lexicon
 * gesture g is its phrase's words (at most MGR_JOINT_MAX_PHRASE_WORDS of them: a longer phrase is refused, for the whole call); in a
 * stream without one gesture g is class g, which needs G <= C, and g == blank is an extension of probability 0 in that stream.
 * Emissions are K14's: frames skip .. skip + Tp - 1, Tp = input_len[b] clipped into [0, T - skip], ln y = ln((P + eps) / sum_c (P + eps)),
 * formed in fp64.  struct_size = sizeof of the struct in the CALLER's header: the call refuses any other value.
 * Score of a hypothesis Q = (g_1 .. g_n), n = 0 allowed:
 *     score(Q) = sum_m w_m ln p_m(Q) + sum_i ext[(g_{i-1} + 1) * G + g_i] + fin[g_n + 1]
 * ln p_m(Q) is K14's logp (all alignments, words expanded through the lexicon); ext [(G+1)*G] and fin [G+1] (or NULL) are doubles in
 * device memory with K13's conventions: row / index 0 = start / empty, entries finite or -inf, THE CALLER refuses NaN and +inf.
 * Prefix score: pre(Q) = the same sum with ln psi_m(Q) in place of ln p_m(Q) and without fin, psi_m(Q) the probability under stream m
 * that the labelling BEGINS with the expansion of Q.
 * Recursion per stream, natural-log fp64, lse(a, b) = max + log1p(exp(-|a - b|)) with lse(-inf, x) = x.  A prefix g has gn(t), gb(t):
 * the log-probability of emitting exactly g over frames 0 .. t, ending in a label / in blank; the empty prefix has gn = -inf, gb(t) =
 * sum_{tau <= t} ln y_tau(blank).  Extension h = g . c by a class c of the stream (never blank):
 *     t = 0:  gn_h(0) = ln y_0(c) if g is empty, else -inf;  gb_h(0) = -inf;  psi = gn_h(0)
 *     t >= 1: phi = lse(gb_g(t-1), last(g) != c ? gn_g(t-1) : -inf)            (the empty prefix: gb_g(t-1))
 *             gn_h(t) = lse(gn_h(t-1), phi) + ln y_t(c);   gb_h(t) = lse(gb_h(t-1), gn_h(t-1)) + ln y_t(blank)
 *             psi = lse(psi, phi + ln y_t(c))
 *     ln p(h) = lse(gn_h(Tp-1), gb_h(Tp-1));  at Tp = 0 every non-empty h has psi = p = 0 (-inf) and the empty hypothesis ln p = 0
 * A gesture of n_g words is n_g chained extensions; only the last word's gn, gb and psi are the gesture's.
 * The search, per sample:
 *   round 0        the live set is the empty prefix; the result list receives the empty hypothesis if its score is finite.
 *   round n >= 1   candidates are (live prefix of rank r, gesture g) with finite ext; a candidate ranks by pre, pre = -inf is dropped;
 *                  the `beam` best are kept, ties to the smaller r, then the smaller g; each kept candidate whose score is finite
 *                  enters the result list, in rank order.
 *   result list    the top_paths best scores; ties go to the entry found earlier (lower round, then better rank in the round).
 *   stop           after round n when nothing is live, or n == max_len, or the list holds top_paths entries and the best live prefix
 *                  has pre + U_n < the list's worst score, U_n = (max_len - n) * max(0, largest ext) + max(0, largest fin).
 * Since psi_m(Q) >= p_m(Q') for every extension Q' of Q and the comparison is strict, the stop never changes the output: it equals
 * the search that always runs max_len rounds.
 * Outputs (device): out [B,top_paths,max_len] int32 padded -1; out_len [B,top_paths], -1 for an empty slot; score [B,top_paths] double,
 * -inf for an empty slot; logp [B,top_paths,M] double, each stream's ln p_m unweighted (-inf in an empty slot); rounds [B] int32 or
 * NULL: the rounds the sample ran.  A sample without a finite hypothesis gets all slots empty.
 * 1 <= top_paths <= beam <= 32, 1 <= max_len <= MGR_RESCORE_MAX_LABELS, B <= 65535.  The workspace holds per stream the fp64 class-major
 * emissions and two sets of `beam` prefix arrays (the kept candidates' chains are run again to store theirs: the arrays of all
 * beam * G candidates are never stored), and the candidates' psi / ln p.  No atomics: deterministic, and a sample's rows do not
 * depend on the rest of the batch.  An error is reported before anything is written. */
#define MGR_JOINT_MAX_STREAMS 4
#define MGR_JOINT_MAX_PHRASE_WORDS 8
typedef struct mgr_joint_stream {
  unsigned struct_size;
  int T;
  int C;
  int skip;
  int blank;
  float eps;
  double weight;
  const float* P;
  const int32_t* input_len;
  const int32_t* phrase_off;
  const int32_t* phrase_words;
} mgr_joint_stream;
size_t mgr_ctc_joint_ws_bytes(int B, int M, const mgr_joint_stream* streams, int G, int beam, int top_paths, int max_len);
int mgr_ctc_joint_decode(mgr_ctx* ctx, int B, int M, const mgr_joint_stream* streams, int G, const double* ext, const double* fin, int beam,
                         int top_paths, int max_len, int32_t* out, int32_t* out_len, double* score, double* logp, int32_t* rounds,
                         void* ws, size_t ws_bytes);

/* ---- K15: expected risk over an N-best list and its gradient: what sequence-level minimum-risk training (MWER / minimum
 * expected error) needs beside K11's N-best lists, K12's edit distances and K14's scores - the gradient through all K likelihoods of a
 * sample in one call.  Per sample: K hypothesis slots (hyp / hyp_len / the lexicon exactly as K14 takes them) and one integer risk
 * r_k per slot (risk [B,K] int32, device: what mgr_edit_distance writes as dist for pair b * K + k).  logp_k is K14's logp: the same
 * frames, skip, eps, blank, label clipping and expansion.  A slot is LIVE if it is present (hyp_len >= 0), scored (no phrase id outside
 * [0, G), at most Lcap labels after expansion) and feasible (logp_k > -inf).  Over the live slots, with a = post_scale > 0:
 *     w_k      = exp(a logp_k) / sum_j exp(a logp_j)          (differences taken in fp64)
 *     Rbar     = sum_k w_k r_k risk_scale                      -> exp_risk[b]
 *     g_k      = a w_k (r_k risk_scale - Rbar)                 = dRbar / dlogp_k
 *     dLogits  = gscale sum_k g_k dlogp_k/dlogits
 * where dlogp_k/dlogits is minus what mgr_ctc_loss_grad writes into dLogits for the label row = hypothesis k at gscale = 1: the
 * gradient w.r.t. the Dense logits (P = softmax(logits)), the eps handling and the zeros on the skipped frames and on the frames from
 * skip + Tp on are k_ctc_grad's, applied linearly.  Since sum_k g_k = 0 the k-independent term of the loss gradient cancels; the
 * kernel sums only the g_k-weighted state occupancies.  Non-live slots have w_k = 0; with fewer than two live slots the gradient is
 * zero, with none exp_risk is 0.
 * Outputs (device): logp [B,K] double (K14's table, and NaN for a slot with more than Lcap labels), weight [B,K] or NULL, exp_risk
 * [B], dLogits [B,T,C] or NULL (then no lattice is stored).  accumulate != 0: dLogits += instead of =, so a caller that has the CTC
 * gradient in dLogits needs no add pass (frames that get zero are then left as they are).
 * 1 <= K <= MGR_RISK_MAX_SLOTS; 1 <= Lcap <= MGR_RESCORE_MAX_LABELS is the longest expanded hypothesis the workspace holds.  The
 * workspace keeps the class-major emissions and alpha and beta of every slot: B K T 2 (Lcap + 1) 8 bytes beside the small blocks -
 * about 0.6 GB at B = 64, K = 8, T = 1900, Lcap = 40 (computed).  Its size does not depend on the lexicon (the query takes it for
 * symmetry with the call, as K13 / K14).  No atomics: deterministic, and a sample's rows do not depend on the rest of the batch.
 * B <= 65535. */
#define MGR_RISK_MAX_SLOTS 32
size_t mgr_ctc_risk_ws_bytes(int B, int T, int C, int K, int Lcap, int G, const int32_t* phrase_off);
int mgr_ctc_risk_grad(mgr_ctx* ctx, const float* P, const int32_t* input_len, int B, int T, int C, int skip, int blank, float eps,
                      const int32_t* phrase_off, const int32_t* phrase_words, int G, const int32_t* hyp, const int32_t* hyp_len, int K,
                      int Lh, int Lcap, const int32_t* risk, float risk_scale, float post_scale, float gscale, int accumulate,
                      double* logp, float* weight, float* exp_risk, float* dLogits, void* ws, size_t ws_bytes);

/* ---- K16: CTC hypotheses by sampling alignments: a second filler for "a list of hypotheses per sample" beside the beam
 * search - K frame paths per sample drawn from the network's own per-frame distribution, collapsed, equal labellings merged and
 * counted.  One independent draw per (sample, draw, frame): nothing is serial over the frames.  P [B,T,C] float32 and input_len [B]
 * (required) as every decode kernel takes them: Tp = input_len[b] clipped into [0, T - skip].
 * The draw of sample b, draw k, frame t in [skip, skip + Tp) - every operation a single IEEE float32 operation, in this order:
 *     w_c   = P[b,t,c] + eps
 *     cum_c = cum_{c-1} + w_c   (cum_{-1} = 0; class order), S = cum_{C-1}
 *     u     = (float)(r >> 8) * 2^-24,   r = the library's counter-based 32-bit generator (mgr_rand_u32 in csrc/common.h) at
 *             seed and index (uint64_t)(b * K + k) * T + t
 *     thr   = u * S
 *     class = the first c with cum_c > thr; `blank` if there is none (S = 0)
 * That is the distribution y = (P + eps) / sum_c (P + eps) of mgr_ctc_loss_grad, mgr_ctc_rescore and mgr_ctc_risk_grad; a class of
 * weight 0 is never drawn; NaN input is unspecified.
 * The labelling of a draw is the CTC collapse of its frame path: a frame equal to its predecessor is dropped, then the blanks are; its
 * length lies in [0, Tp].  The UNIQUE labellings of a sample are written in order of first occurrence over k = 0 .. K - 1 (labellings
 * are compared exactly, label by label): out [B,K,T-skip] int32 padded -1 (the beam kernels' layout), out_len [B,K] the labelling's
 * length, count [B,K] the number of draws that collapsed to it, n_unique [B].  Slots j >= n_unique[b] are absent slots as K12, K14
 * and K15 understand them: out_len -1, count 0, a row of -1.  sum_j count[b,j] = K always; Tp = 0 gives one labelling, the empty one,
 * with count K.  path [B,K,T-skip] int32 or NULL: the class drawn at every frame in DRAW order (row k = draw k), -1 from Tp on.
 * 2 <= C <= 64, 1 <= K <= MGR_SAMPLE_MAX_DRAWS, B <= 65535.  No workspace: the unique rows are compacted in out itself.  No atomics:
 * deterministic - row b depends on its own posteriors, seed, b, K and T alone. */
#define MGR_SAMPLE_MAX_DRAWS 32
int mgr_ctc_sample_paths(mgr_ctx* ctx, const float* P, const int32_t* input_len, int B, int T, int C, int skip, int blank, float eps,
                         uint64_t seed, int K, int32_t* out, int32_t* out_len, int32_t* count, int32_t* n_unique, int32_t* path);

/* ---- K12: scoring decodes: the weighted edit distance of n_pairs pairs of label sequences, with the substitution /
 * deletion / insertion split of HTK's HResults, in one launch.  All pointers are device memory.
 * hyp [n_hyp,Lh], ref [n_ref,Lr] int32, rows padded with -1; hyp_len [n_hyp] / ref_len [n_ref] int32 or NULL: NULL = the whole row,
 * otherwise clipped into [0, width].  Before comparing, a row loses every entry < 0 and every entry v < 64 whose bit is set in
 * ignore_mask (so the -1 padded lab rows of mgr_greedy_segments and the out rows of the beam kernels feed it unchanged, and the
 * blank / "sil" is stripped here); what remains is h with m labels and r with n labels.  Pair p compares h of row pair_h[p] with r of
 * row pair_r[p]; both arrays NULL: pair p is (p, p) and n_hyp == n_ref == n_pairs.  The indices are device data: THE CALLER must
 * keep them in [0, n_hyp) / [0, n_ref) (the kernel clamps what it reads, it cannot report).
 * Result, whatever the traversal order: over all monotone alignments of h to r - a hit pairs equal labels at cost 0; a substitution
 * pairs unequal labels, cost_sub, S + 1; a deletion is a ref label without partner, cost_del, D + 1; an insertion is a hyp label
 * without partner, cost_ins, I + 1 - the lexicographically smallest tuple (cost, S, D, I).  dist [n_pairs] = cost, counts
 * [n_pairs,4] = (H, S, D, I) with H = n - S - D, lens [n_pairs,2] = (m, n).  (Lexicographic order is compatible with addition, so
 * the DP over tuples is exact.)
 * ops [n_pairs,Lh+Lr] int8 and n_ops [n_pairs] may be NULL.  ops holds one alignment that attains the tuple, in forward order: 0 hit,
 * 1 substitution, 2 deletion, 3 insertion, -1 behind the n_ops = H + S + D + I entries.  It is the walk back from (m, n) that takes
 * at each cell the first of diagonal, deletion, insertion whose predecessor tuple plus the step's tuple equals the cell's tuple.
 * The walk needs 2 bits per cell: ws >= the size query with want_ops = 1 when ops is given (written only then); without ops the
 * query is 0 and ws may be NULL.
 * Lh, Lr <= MGR_EDIT_MAX_LEN; costs in [1, MGR_EDIT_MAX_COST] (the cost stays below 2^27).  Integer arithmetic, no atomics:
 * deterministic, and a pair's result does not depend on the other pairs. */
#define MGR_EDIT_MAX_LEN  4095
#define MGR_EDIT_MAX_COST 16384
size_t mgr_edit_distance_ws_bytes(int n_pairs, int Lh, int Lr, int want_ops);
int mgr_edit_distance(mgr_ctx* ctx, const int32_t* hyp, const int32_t* hyp_len, int n_hyp, int Lh, const int32_t* ref,
                      const int32_t* ref_len, int n_ref, int Lr, const int32_t* pair_h, const int32_t* pair_r, int n_pairs, int cost_sub,
                      int cost_del, int cost_ins, uint64_t ignore_mask, int32_t* dist, int32_t* counts, int32_t* lens, int8_t* ops,
                      int32_t* n_ops, void* ws, size_t ws_bytes);

/* ---- K10: TimeDistributed CNN front-end of the RGB network (rgb_network/cnn_lstm.py: conv_1 / conv_3 / conv_5, each followed by
 * MaxPooling2D) ------------------------------------------------------------------------------------------------------------------
 * Per frame of N = B*T frames, channels-last: X [N][Hin][Win][Cin] -> valid Conv2D (W [ks][ks][Cin][Cout], b [Cout]) -> ReLU ->
 * 2x2 / stride 2 max-pool with floor -> Y [N][Hp][Wp][Cout], Hp = (Hin - ks + 1) / 2, Wp likewise.  ks is 4 or 5, Cout a multiple of
 * 4, W 16-byte aligned; a frame (Hin*Win*Cin floats) and a frame's pooled gradient (Hp*Wp*Cout floats + bytes) must fit 64 KiB.
 * code [N][Hp][Wp][Cout] (uint8) routes the gradient through the pool: the window position dy*2+dx of the FIRST maximum in row-major
 * window order, or MGR_CONV_NO_GRAD when the maximum is a ReLU zero (no position of that window gets a gradient).  Exact f32.
 * mgr_conv_pool_bwd_data: dX [N][Hin][Win][Cin] (overwritten) from the pooled gradient dY through pool, ReLU and the transposed conv.
 * mgr_conv_pool_bwd_weights: dW, db (overwritten), deterministic: fixed-order partial sums over frame chunks in ws
 * (mgr_conv_pool_bwd_weights_ws_bytes), then a fixed-order pass over the chunks; no atomics.  The forward and data-gradient calls
 * need no workspace. */
#define MGR_CONV_NO_GRAD 0xFF
int mgr_conv_pool_fwd(mgr_ctx* ctx, const float* X, int N, int Hin, int Win, int Cin, const float* W, const float* b, int ks, int Cout,
                      float* Y, uint8_t* code);
int mgr_conv_pool_bwd_data(mgr_ctx* ctx, const float* dY, const uint8_t* code, const float* W, int N, int Hin, int Win, int Cin, int ks,
                           int Cout, float* dX);
size_t mgr_conv_pool_bwd_weights_ws_bytes(int N, int Hin, int Win, int Cin, int ks, int Cout);
int mgr_conv_pool_bwd_weights(mgr_ctx* ctx, const float* X, const float* dY, const uint8_t* code, int N, int Hin, int Win, int Cin, int ks,
                              int Cout, float* dW, float* db, void* ws, size_t ws_bytes);

/* ---- skeletal feature extraction (skeletal_network/skeletal_feature_extraction.py:24-215), fp64 like the original.
 * joints[n_frames][12] = lhX lhY rhX rhY leX leY reX reY hipX hipY shcX shcY of the WHOLE frame table in file order;
 * out[n_frames][23] = lh_v rh_v le_v re_v | lh_a rh_a le_a re_a | hands_d | lh,rh,le,re _hip_d | lh,rh,le,re _shc_d |
 * lh_hip_ang rh_hip_ang lh_shc_ang rh_shc_ang lh_el_ang rh_el_ang.  Velocities / accelerations of rows 0..4 are 0. */
#define MGR_SKELETAL_JOINT_COLS 12
#define MGR_SKELETAL_FEATURE_COLS 23
int mgr_skeletal_features(mgr_ctx* ctx, const double* joints, size_t n_frames, double* out);

/* ---- activity features of the raw joint files (skeletal_network/velocity.py, r_position.py of the reference), integer
 * exact.  A ragged batch of n_files files: file f's frames are [offsets[f], offsets[f + 1]) of joints[n_frames][20] = hipX hipY
 * shcX shcY lsX lsY leX leY lwX lwY lhX lhY rsX rsY reX reY rwX rwY rhX rhY (int32, clamped, within +-2^20; offsets int64 with
 * offsets[n_files] <= n_frames).  Per file: out[.][5] = lh_v rh_v low lh_dist_rp rh_dist_rp, with lh_v / rh_v = floor of the hand's
 * Euclidean step from the previous frame (0 in the file's rows 0..3), low = lh_v < mean(lh_v) && rh_v < mean(rh_v) over the file,
 * rest[f][16] = the truncated medians of lsX .. rhY over the low frames (an even count: (a + b) / 2 of the two middle values,
 * truncated toward zero), and the distances floor(|rest hand - hand|) (0 in rows 0..3).  rest_given: rest is read instead of
 * estimated.  status[f] = 0, or 1 when the file has no low-velocity frame (then, unless rest_given, its rest and distances are 0).
 * One launch, one workgroup per file; deterministic (no atomics on global memory). */
#define MGR_ACTIVITY_JOINT_COLS 20
#define MGR_ACTIVITY_REST_COLS 16
#define MGR_ACTIVITY_OUT_COLS 5
#define MGR_ACTIVITY_MAX_FILES 65536
#define MGR_ACTIVITY_MAX_FRAMES (1LL << 26)
int mgr_skeletal_activity(mgr_ctx* ctx, const int32_t* joints, const int64_t* offsets, int n_files, long long n_frames, int rest_given,
                          int32_t* rest, int32_t* out, int32_t* status);

/* ---- HTK HCopy-compatible MFCC_0[_D[_A]] front-end of the audio network (README.md: 13 MFCCs + deltas + accelerations, made with
 * HTK's HCopy from config_HCopy; algorithm restated in DESIGN 9c).  A batch of n_utts ragged utterances: samples (raw int16, no
 * scaling) of utterance u are [sample_offsets[u], sample_offsets[u + 1]); it has (N - frameSize) / frameRate + 1 frames when
 * N >= frameSize, else 0, and n_frames is their sum over the batch.  fftN is a power of two in [256, 2048] with frameSize <= fftN;
 * numChans <= 128, numCeps <= min(numChans, 63); cepLifter 0 disables the lifter; accs needs deltas.  loChan (int32) / loWt (fp64)
 * [fftN / 2] are HTK's filterbank table per bin (bin 0 = DC; loChan -1 = unused bin).  Each output row holds numCeps + 1 statics
 * (C1..C_numCeps, C0), then as many deltas if deltas, then as many accelerations if accs, as f32.  Utterance u's rows are
 * [out_offsets[u], out_offsets[u + 1]) (out_offsets has n_utts + 1 entries): row r holds frame r * out_stride, or zeros past the
 * utterance's last frame, so the rows can be packed or a padded (B, T, cols) batch.  fp64 arithmetic; deterministic (no atomics).
 * ws >= mgr_mfcc_ws_bytes(n_utts, n_frames, frameSize, fftN, numChans, numCeps). */
size_t mgr_mfcc_ws_bytes(int n_utts, long long n_frames, int frameSize, int fftN, int numChans, int numCeps);
int mgr_mfcc(mgr_ctx* ctx, const int16_t* samples, const int64_t* sample_offsets, int n_utts, long long n_frames, int frameSize,
             int frameRate, int fftN, int numChans, int numCeps, int cepLifter, double preemph, int deltas, int accs, int out_stride,
             const int32_t* loChan, const double* loWt, float* out, const int64_t* out_offsets, void* ws, size_t ws_bytes);

/* ---- upper-body crops of the RGB network's frames (rgb_network/roi_extraction.py:18-80 of the reference).  frames are
 * n BGR uint8 frames (n, H, W, 3), 4-byte aligned, 3 W a multiple of 4, W <= 4096; boxes int32 (n, 4) = [y0, y1, x0, x1) with
 * 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W (the host has applied the reference's clamps, slicing and fallback; a frame whose box is
 * outside these bounds gets zeros); 1 <= img_dim <= 64.  out (n, img_dim, img_dim) uint8, 4-byte aligned: OpenCV's 8-bit BGR2GRAY
 * Y = (1868 B + 9617 G + 4899 R + 8192) >> 14 of the crop, resized with OpenCV's generic fixed-point INTER_CUBIC path: per axis
 * scale = 1 / (img_dim / size) (double), fx = (float)((d + 0.5) scale - 0.5), sx = floor(fx), fx -= sx, cubic weights (A = -0.75)
 * in float32, the fourth 1 - c0 - c1 - c2, each rounded half to even to c * 2048; taps sx - 1 .. sx + 2 clamped to the crop;
 * int32 horizontal sums, int32 vertical sums of 4 taps x 4 weights, (v + 2^21) >> 22 saturated to 0..255.  Bit-exact contract;
 * deterministic (no atomics). */
int mgr_roi_crop(mgr_ctx* ctx, const uint8_t* frames, int n, int H, int W, const int32_t* boxes, int img_dim, uint8_t* out);

/* ---- K20 / K21: live recognition - chunked BiLSTM inference with carried state.  Inference only. ----
 * A session is a stream of frames that is still being produced; the network sees it in WINDOWS of Tw frames.  Per window and
 * session s, n_valid[s] <= Tw frames are present and the first n_keep[s] <= n_valid[s] of them are answered by this window (the
 * rest is lookahead, seen again by the next window).  One job of the call below is ONE direction of ONE layer for S sessions:
 *   Z [S,Tw,4H] and Up [H,4H] packed, Y with row stride ldy, R (or NULL) with row stride ldr: as in the scan jobs above.
 *   reverse == 0: the recurrence starts from state [S,2,H] = (h, c) of each session, walks t = 0 .. n_valid[s] - 1 and overwrites
 *                 the state with (h, c) after frame n_keep[s] - 1; with n_keep[s] == 0 the state is left as it was.
 *   reverse != 0: starts from zero at t = n_valid[s] - 1 and walks down to 0; state must be NULL.
 * n_valid, n_keep: device int32 [S], shared by the jobs of the call.  n_valid[s] == 0: the session is idle - nothing of it is read
 * and no byte of its Y rows or its state is written.  Otherwise rows n_valid[s] <= t < Tw of Y (columns 0:H) are written as zero,
 * and rows t >= n_valid[s] of Z are never read (they may hold NaN).  The device clips n_valid into [0, Tw] and n_keep into
 * [0, n_valid].  h_n_valid / h_n_keep: the same values on the HOST, or both NULL; when given they are checked (0 <= n_keep <=
 * n_valid <= Tw) before anything is enqueued.
 * Kernel: one 16-wave workgroup per (job, group of 4 sessions); no workgroup waits for another, so the call cannot hang on
 * residency and needs no workspace.  The recurrent matrix is streamed from L2 every step, the k range of the product split over
 * the waves and reduced through LDS in a fixed order: the summation order of a pre-activation is a function of H alone - not of the
 * step's place in the window, of Tw, or of the session's slot - so a session cut into windows differently gives the same bits.
 * 1 <= H <= MGR_LIVE_MAX_H, 1 <= njobs <= MGR_LIVE_MAX_JOBS, all jobs with the same S and Tw; pointers 16-byte aligned. */
#define MGR_LIVE_MAX_H 1024
#define MGR_LIVE_MAX_JOBS 8
typedef struct mgr_live_job {
  const float* Z;
  const float* Up;
  float* Y;
  const float* R;
  float* state;
  int ldy, ldr, H, reverse;
} mgr_live_job;
int mgr_lstm_scan_window(mgr_ctx* ctx, int njobs, const mgr_live_job* jobs, int S, int Tw, const int32_t* n_valid, const int32_t* n_keep,
                         const int32_t* h_n_valid, const int32_t* h_n_keep);
/* Greedy CTC decode that carries its open run from call to call: P [S,Tw,C] are the posteriors of a window, of which the first
 * n_keep[s] rows (device int32 [S], clipped into [0, Tw]) are the session's next frames.  state: device int32 [S, MGR_LIVE_STATE_WORDS]
 * = {frames consumed so far, the open run's label (-1: none), its first frame, its last frame, its frame count, the float32 sum of
 * its frame maxima (as bits), 0, 0}; all zero except label = -1 is a fresh session - and so is all zero: a run counts only with a
 * frame count > 0.  Frames are numbered from the session's start; frames below skip are ignored.  Per frame the best class is the argmax
 * with the first index on ties; equal neighbouring best classes form a run; a run is FINAL when a frame with another best class
 * follows it or when flush[s] != 0 (device int32 [S] or NULL: the open run is closed behind this call's frames).  Final runs whose
 * label is not blank are this call's events, in order: n_events [S] = their TRUE count, also beyond cap, and for e < min(n_events,
 * cap): lab [S,cap], seg [S,cap,2] = (first, last) frame, conf [S,cap] = the sum of the run's frame maxima, added one at a time in
 * float32 in frame order, divided by its frame count.  Entries from n_events on are not written.  The confidence filter of the
 * offline decode counts over a whole recording and is not causal: this is its thr < 0 form.  One wave per session.
 * 1 <= C, 0 <= blank < C or blank < 0 (no blank), cap >= 0, skip >= 0. */
#define MGR_LIVE_STATE_WORDS 8
int mgr_live_greedy(mgr_ctx* ctx, const float* P, int S, int Tw, int C, const int32_t* n_keep, int blank, int skip, int32_t* state,
                    const int32_t* flush, int cap, int32_t* n_events, int32_t* lab, int32_t* seg, float* conf);

#ifdef __cplusplus
}
#endif
#endif /* MGR_H_ */
