// C-ABI entry points of the LSTM recurrence (K3, K7-scan): pick the kernel family for each shape.
//   forward:  H/4 with an instantiation (H = 100, 128, 300, 500 and test sizes) -> lstm_cluster.hip: persistent
//             weight-stationary MFMA kernel, one CU per batch group (H <= 128) or clusters of CUs exchanging h_t
//   backward: H <= 128 -> lstm_mfma.hip (single-CU weight-stationary MFMA)
//   anything else (H <= 1024) -> lstm_simple.hip (U streamed from L2; correctness fallback)
// WHAT a call launches is decided once per call, by the pure host functions of scan_choice.h (mgr_scan_fwd_decide / mgr_scan_bwd_decide);
// the entry points here validate, decide, and carry the choice out.
#include <algorithm>
#include <cstddef>

#include "common.h"
#include "lstm_cluster.h"

int mgr_scan_fwd_simple(mgr_ctx*, const float*, const float*, float*, int, const float*, int, float*, float*, int, int, int, int);
int mgr_scan_bwd_simple(mgr_ctx*, const float*, int, const float*, const float*, const float*, float*, int, int, int, int);
int mgr_scan_bwd_mfma_multi(mgr_ctx*, int, const mgr_scan_bwd_job*);
int mgr_scan_bwd_cu16_multi(mgr_ctx*, int, const mgr_scan_bwd_job*, const mgr_scan_choice&);   // lstm_cu_bwd.hip: one CU per (direction, 16-sample group), split-f16

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

static int check_launch_status(mgr_ctx* c, unsigned* status, const char* what) {
  unsigned st = 0;   // MGR_TUNE_SCAN_SYNC_CHECK: synchronous give-up check (tests)
  MGR_HIP(hipMemcpyAsync(&st, status, sizeof(st), hipMemcpyDeviceToHost, mgr_stream(c)));
  MGR_HIP(hipStreamSynchronize(mgr_stream(c)));
  MGR_REQUIRE(st == 0, "%s: a bounded spin gave up (status %u)", what, st);
  return 0;
}

extern "C" {

int mgr_tune(mgr_ctx* c, int key, int value) {
  MGR_REQUIRE(c && key >= 0 && key < MGR_TUNE_COUNT, "bad tune key");
  MGR_REQUIRE(!(key == MGR_TUNE_SCAN_FORM && value == 2), "tune key %d = 2: the pair form of the scan is retired", key);
  MGR_REQUIRE(key != 17 || value == 0, "tune key 17 = %d: the fused scan form whose halves gather alone is retired", value);
  c->tune[key] = value;
  return 0;
}

int mgr_tune_get(mgr_ctx* c, int key, int* value) {
  MGR_REQUIRE(c && value && key >= 0 && key < MGR_TUNE_COUNT, "bad tune key");
  *value = c->tune[key];
  return 0;
}

// the workspace queries that need no context: the layout functions of scan_choice.h, which yield offsets only
size_t mgr_lstm_scan_bwd_multi_ws_bytes(int njobs, const mgr_scan_bwd_job* jobs) { return mgr_scan_bwd_ws_layout(njobs, jobs).bytes; }

size_t mgr_lstm_scan_ws_bytes(int B, int T, int H) {
  (void)T;
  mgr_scan_job j;
  memset(&j, 0, sizeof(j));
  j.B = B;
  j.H = H;
  mgr_scan_bwd_job bj;
  memset(&bj, 0, sizeof(bj));
  bj.B = B;
  bj.H = H;
  // (the backward figure holds U^T for the fallback backward kernel)
  return std::max(mgr_scan_fwd_ws_layout(1, &j, nullptr, nullptr).bytes, mgr_scan_bwd_ws_layout(1, &bj).bytes);
}

// (an upper bound: row scratch for EVERY job without Y; mgr_lstm_scan_fwd_multi_ws_bytes leaves out the jobs whose kernel writes the
// transposed copy itself)
size_t mgr_lstm_scan_multi_ws_bytes(int njobs, const mgr_scan_job* jobs) { return mgr_scan_fwd_ws_layout(njobs, jobs, nullptr, nullptr).bytes; }

// what a mgr_scan_launch_opts says, read through its own struct_size (members beyond it are zero)
static void read_opts(const mgr_scan_launch_opts* o, int* form, unsigned** seq_out) {
  *form = 0;
  *seq_out = nullptr;
  if (!o) return;
  if (o->struct_size >= offsetof(mgr_scan_launch_opts, form) + sizeof(o->form)) *form = o->form;
  if (o->struct_size >= offsetof(mgr_scan_launch_opts, seq_out) + sizeof(o->seq_out)) *seq_out = o->seq_out;
}

int mgr_abi_struct_sizes(unsigned out[4]) {
  MGR_REQUIRE(out, "null argument");
  out[0] = (unsigned)sizeof(mgr_scan_job);
  out[1] = (unsigned)sizeof(mgr_scan_bwd_job);
  out[2] = (unsigned)sizeof(mgr_scan_launch_opts);
  out[3] = MGR_ABI_REVISION;
  return 0;
}

int mgr_lstm_scan_fwd_multi(mgr_ctx* c, int njobs, const mgr_scan_job* jobs, void* ws, size_t ws_bytes) {
  return mgr_lstm_scan_fwd_multi_ex(c, njobs, jobs, ws, ws_bytes, nullptr);
}

// The checks of a forward call that are plain host code, shared by the call, its workspace query and mgr_lstm_scan_fwd_describe.
// (The job list is checked before the context: these checks are what keeps a store through a NULL row pointer off the device, and a
//  box without a GPU can run them - tests/test_cpu_scan_no_rows.py)
static int check_fwd_jobs(int njobs, const mgr_scan_job* jobs) {
  MGR_REQUIRE(jobs && njobs > 0 && njobs <= MGR_MAX_SCAN_JOBS, "bad job list");
  for (int i = 0; i < njobs; ++i) {
    const mgr_scan_job& j = jobs[i];
    MGR_REQUIRE(j.Z && j.Up, "job %d: null argument", i);
    MGR_REQUIRE(j.Y || j.YT, "job %d: neither Y nor YT - a scan job writes its rows, the transposed copy, or both", i);
    MGR_REQUIRE(j.B > 0 && j.T > 0 && j.H > 0 && (!j.Y || j.ldy >= j.H) && (!j.R || j.ldr >= j.H), "job %d: bad shape", i);
    MGR_REQUIRE(aligned16(j.Z) && aligned16(j.Up) && (!j.gates || aligned16(j.gates)), "job %d: Z/Up/gates must be 16-byte aligned", i);
    MGR_REQUIRE(!j.YT || (aligned16(j.YT) && j.ldt % 4 == 0 && j.ldt >= (j.T + 31) / 32 * 32 && j.ytb % 4 == 0 && j.ytb >= (long long)j.H * j.ldt),
                "job %d: transposed output needs a 16-byte aligned YT, ldt %% 4 == 0, ldt >= T rounded up to 32, ytb >= H * ldt", i);
    MGR_REQUIRE(!j.YT || !j.yt_split || j.ldt % 8 == 0, "job %d: split rows need ldt %% 8 == 0", i);
  }
  return 0;
}
static int check_fwd_form(int form) {
  MGR_REQUIRE(form >= MGR_SCAN_FORM_AUTO && form <= MGR_SCAN_FORM_FUSED_ANY, "unknown scan form %d", form);
  MGR_REQUIRE(form != 2, "scan form 2 (the pair form) is retired");
  return 0;
}
// Rows in scratch were decided, and the workspace is checked against them, BEFORE anything is enqueued: a kernel that stores through a
// NULL row pointer faults the device.
static int check_fwd_ws(const mgr_scan_choice& C, size_t ws_avail) {
  MGR_REQUIRE(C.need == C.base_need || ws_avail >= C.need,
              "jobs without Y whose kernel does not write YT itself need %zu bytes of workspace for their rows (mgr_lstm_scan_fwd_multi_ws_bytes)",
              (size_t)C.need);
  return 0;
}

// The forward multi-scan call: validate -> decide (scan_choice.h) -> carry the choice out.
int mgr_lstm_scan_fwd_multi_ex(mgr_ctx* c, int njobs, const mgr_scan_job* jobs, void* ws, size_t ws_bytes,
                               const mgr_scan_launch_opts* opts) {
  int r = check_fwd_jobs(njobs, jobs);
  if (r) return r;
  MGR_REQUIRE(c, "null context");
  mgr_planes_forget_range(c, ws, ws_bytes);   // (this call writes its workspace: kept weight planes in it are gone)
  int form;
  unsigned* seq_out;
  read_opts(opts, &form, &seq_out);
  r = check_fwd_form(form);
  if (r) return r;
  if (seq_out) *seq_out = MGR_SEQ_NONE;   // (until a launch of this call enters the residency ledger)
  int hmax = 0;
  for (int i = 0; i < njobs; ++i) hmax = jobs[i].H > hmax ? jobs[i].H : hmax;
  const int family = hmax > 128 ? MGR_K_SCAN_FWD : MGR_K_SCAN_FWD_NARROW;
  r = mgr_prof_begin(c, family);
  if (r) return r;
  const size_t ws_avail = ws ? ws_bytes : 0;
  const mgr_scan_choice C = mgr_scan_fwd_decide(c->cu_count, c->tune, njobs, jobs, form, ws_avail);
  r = check_fwd_ws(C, ws_avail);
  if (r) return r;
  char* base = reinterpret_cast<char*>(ws);
  unsigned* status = nullptr;
  float* rows[MGR_MAX_SCAN_JOBS];   // where each job's rows go: its Y, or scratch (a K-split job without Y keeps its NULL)
  int ldrows[MGR_MAX_SCAN_JOBS];
  for (int i = 0; i < njobs; ++i) {
    const bool scratch = C.job[i].rows_in_scratch;
    rows[i] = scratch ? reinterpret_cast<float*>(base + C.job[i].rows_off) : jobs[i].Y;
    ldrows[i] = scratch ? jobs[i].H : jobs[i].ldy;
  }
  if (C.kernel != MGR_SCAN_FWD_NONE) {
    ClusterLaunch L;
    memset(&L, 0, sizeof(L));
    status = reinterpret_cast<unsigned*>(base);
    const bool writes_yt = C.kernel != MGR_SCAN_FWD_IMAGE;   // (the K-split kernels honour ClusterJob::YT)
    for (int i = 0; i < njobs; ++i) {
      const mgr_scan_choice_job& q = C.job[i];
      if (!q.cluster) continue;
      const mgr_scan_job& j = jobs[i];
      ClusterJob& cj = L.job[L.njobs++];
      cj.Z = j.Z; cj.Up = j.Up; cj.Y = rows[i]; cj.R = j.R; cj.G = j.gates; cj.Cs = j.cs;
      cj.ldy = ldrows[i]; cj.ldr = j.ldr; cj.B = j.B; cj.T = j.T; cj.H = j.H; cj.reverse = j.reverse;
      cj.ks = j.H / 4; cj.tpw = q.tpw; cj.nw = q.nw;
      cj.G_ = q.G; cj.nbg = q.nbg;
      cj.cls_begin = q.cls_begin; cj.cls_nclusters = q.cls_nclusters; cj.cls_cluster0 = q.cls_cluster0; cj.cls_rot = q.cls_rot;
      cj.xbuf = reinterpret_cast<float*>(base + q.xbuf_off);
      if (writes_yt) {
        cj.YT = j.YT; cj.ytb = j.ytb; cj.ldt = j.ldt; cj.yt_split = j.yt_split;
      }
      MGR_REQUIRE(cj.Y || (q.yt_in_kernel && cj.YT), "job %d: no rows to write to", i);
    }
    L.xcd_local = C.xcd_local;
    L.fused = C.fused;
    L.live_wgs = C.live;
    L.ksplit = C.ksplit;
    L.split16 = C.split16;
    if (c->tune[MGR_TUNE_SCAN_PRINT_PLAN]) {
      for (int i = 0; i < L.njobs; ++i)
        fprintf(stderr, "[mgr scan plan] job %d: H=%d ks=%d nw=%d tpw=%d G=%d nbg=%d wg_begin=%d\n", i, L.job[i].H,
                L.job[i].ks, L.job[i].nw, L.job[i].tpw, L.job[i].G_, L.job[i].nbg, L.job[i].cls_begin);
      fprintf(stderr, "[mgr scan plan] total %d workgroups, exchange=%d\n", C.grid, C.exchange);
    }
    L.cm.status = status;
    L.cm.sticky = mgr_status_block(c);
    L.cm.resident = c->sticky_status + 1;
    L.cm.total_wgs = C.grid;
    // The ledger counts the forward launch by its LIVE workgroups (the octet layout leaves empty ids that count themselves in and
    // return), the BPTT launch by its grid (mgr_lstm_scan_bwd_multi_ex): an asymmetry as old as the two layouts, kept as it is.
    if (C.ledger) {
      r = mgr_persist_admit(c, C.live, C.waves, C.per_cu, C.fused, &L.cm.seq);
      if (r) return r;
      if (seq_out) *seq_out = L.cm.seq;
    }
    // exchange slots + status must be zero at every launch (epochs count from 1 within the call)
    MGR_HIP(hipMemsetAsync(base, 0, C.zero_bytes, mgr_stream(c)));
    r = mgr_cluster_launch(c, L, C);
    if (r) return r;
    if (C.ledger) {
      r = mgr_persist_commit(c, C.live, C.waves, C.per_cu, C.fused);
      if (r) return r;
    }
  }
  for (int i = 0; i < njobs; ++i) {
    if (C.job[i].cluster) continue;
    const mgr_scan_job& j = jobs[i];
    r = mgr_scan_fwd_simple(c, j.Z, j.Up, rows[i], ldrows[i], j.R, j.ldr, j.gates, j.cs, j.B, j.T, j.H, j.reverse);
    if (r < 0) return r;
  }
  for (int i = 0; i < njobs; ++i) {   // transposed outputs the scan kernel did not write itself
    const mgr_scan_job& j = jobs[i];
    if (!j.YT || C.job[i].yt_in_kernel) continue;
    r = j.yt_split ? mgr_transpose_bt_split_strided(c, rows[i], ldrows[i], j.YT, j.ldt, j.ytb, j.ldt, j.B, j.T, j.H)
                   : mgr_transpose_bt_strided(c, rows[i], ldrows[i], j.YT, j.ldt, j.ytb, j.ldt, j.B, j.T, j.H);
    if (r) return r;
  }
  r = mgr_prof_end(c, family);
  if (r) return r;
  if (status && c->tune[MGR_TUNE_SCAN_SYNC_CHECK]) return check_launch_status(c, status, "cluster scan");
  return 0;
}

// (0: a bad job list, no context or an unknown form - mgr_last_error)
size_t mgr_lstm_scan_fwd_multi_ws_bytes(mgr_ctx* c, int njobs, const mgr_scan_job* jobs, const mgr_scan_launch_opts* opts) {
  if (check_fwd_jobs(njobs, jobs) != 0) return 0;
  if (!c) {
    mgr_fail(-1, "null context");
    return 0;
  }
  mgr_scan_choice C;
  C.struct_size = (unsigned)sizeof(C);
  return mgr_lstm_scan_fwd_describe(c->cu_count, c->tune, MGR_TUNE_COUNT, njobs, jobs, opts, (size_t)-1, &C) == 0 ? (size_t)C.need : 0;
}

// tune keys of a describe call: tune[0 .. ntune), the rest 0
static void read_tune(const int* tune, int ntune, int* out) {
  for (int k = 0; k < MGR_TUNE_COUNT; ++k) out[k] = tune && k < ntune ? tune[k] : 0;
}

int mgr_lstm_scan_fwd_describe(int cu_count, const int* tune, int ntune, int njobs, const mgr_scan_job* jobs, const mgr_scan_launch_opts* opts,
                               size_t ws_bytes, mgr_scan_choice* out) {
  int r = check_fwd_jobs(njobs, jobs);
  if (r) return r;
  MGR_REQUIRE(out && out->struct_size == sizeof(*out) && cu_count > 0, "describe: out->struct_size must be sizeof(mgr_scan_choice), cu_count > 0");
  int form, t[MGR_TUNE_COUNT];
  unsigned* seq_out;
  read_opts(opts, &form, &seq_out);
  r = check_fwd_form(form);
  if (r) return r;
  read_tune(tune, ntune, t);
  *out = mgr_scan_fwd_decide(cu_count, t, njobs, jobs, form, ws_bytes);
  return check_fwd_ws(*out, ws_bytes);
}

int mgr_lstm_scan_fwd(mgr_ctx* c, const float* Z, const float* Up, float* Y, int ldy, const float* R, int ldr,
                      float* gates, float* cs, int B, int T, int H, int reverse, void* ws, size_t ws_bytes) {
  mgr_scan_job j;
  memset(&j, 0, sizeof(j));
  j.Z = Z; j.Up = Up; j.Y = Y; j.R = R; j.gates = gates; j.cs = cs;
  j.ldy = ldy; j.ldr = ldr; j.B = B; j.T = T; j.H = H; j.reverse = reverse;
  return mgr_lstm_scan_fwd_multi(c, 1, &j, ws, ws_bytes);
}

int mgr_lstm_scan_bwd_multi(mgr_ctx* c, int njobs, const mgr_scan_bwd_job* jobs, void* ws, size_t ws_bytes) {
  return mgr_lstm_scan_bwd_multi_ex(c, njobs, jobs, ws, ws_bytes, nullptr);
}

static int check_bwd_form(int form) {
  MGR_REQUIRE(form >= MGR_BPTT_FORM_AUTO && form <= MGR_BPTT_FORM_SINGLE_CU, "unknown BPTT form %d", form);
  return 0;
}
static int check_bwd_jobs(int njobs, const mgr_scan_bwd_job* jobs) {
  for (int i = 0; i < njobs; ++i) {
    const mgr_scan_bwd_job& j = jobs[i];
    MGR_REQUIRE(j.dY && j.gates && j.cs && j.Up && j.dZ, "job %d: null argument", i);
    MGR_REQUIRE(j.B > 0 && j.T > 0 && j.H > 0 && j.lddy >= j.H, "job %d: bad shape", i);
    MGR_REQUIRE(aligned16(j.gates) && aligned16(j.Up) && aligned16(j.dZ), "job %d: gates/Up/dZ must be 16-byte aligned", i);
  }
  return 0;
}

// The BPTT multi-scan call: validate -> decide (scan_choice.h) -> carry the choice out.
int mgr_lstm_scan_bwd_multi_ex(mgr_ctx* c, int njobs, const mgr_scan_bwd_job* jobs, void* ws, size_t ws_bytes,
                               const mgr_scan_launch_opts* opts) {
  MGR_REQUIRE(c && jobs && njobs > 0 && njobs <= MGR_MAX_SCAN_JOBS, "bad job list");
  mgr_planes_forget_range(c, ws, ws_bytes);   // (this call writes its workspace: kept weight planes in it are gone)
  int form;
  unsigned* seq_out;
  read_opts(opts, &form, &seq_out);
  int r = check_bwd_form(form);
  if (r) return r;
  if (seq_out) *seq_out = MGR_SEQ_NONE;
  MGR_REQUIRE(ws && ws_bytes >= mgr_lstm_scan_bwd_multi_ws_bytes(njobs, jobs), "workspace too small");
  r = check_bwd_jobs(njobs, jobs);
  if (r) return r;
  r = mgr_prof_begin(c, MGR_K_SCAN_BWD);
  if (r) return r;
  const mgr_scan_choice C = mgr_scan_bwd_decide(c->cu_count, c->tune, njobs, jobs, form);
  char* base = reinterpret_cast<char*>(ws);
  unsigned* status = reinterpret_cast<unsigned*>(base);
  if (C.single_cu) {
    r = mgr_scan_bwd_cu16_multi(c, njobs, jobs, C);
    if (r) return r;
  }
  if (C.kernel != MGR_SCAN_BWD_NONE) {
    ClusterBwdLaunch L;
    memset(&L, 0, sizeof(L));
    L.xcd_local = C.xcd_local;
    L.fused = C.fused;
    for (int i = 0; i < njobs; ++i) {
      const mgr_scan_choice_job& q = C.job[i];
      if (!q.cluster) continue;
      const mgr_scan_bwd_job& j = jobs[i];
      ClusterBwdJob& cj = L.job[L.njobs++];
      cj.dY = j.dY; cj.gates = j.gates; cj.cs = j.cs; cj.Up = j.Up; cj.dZ = j.dZ; cj.dzmax = j.dzmax; cj.dbsum = j.dbsum;
      cj.lddy = j.lddy; cj.B = j.B; cj.T = j.T; cj.H = j.H; cj.reverse = j.reverse;
      cj.G_ = q.G; cj.nbg = q.nbg;
      cj.cls_begin = q.cls_begin; cj.cls_nclusters = q.cls_nclusters; cj.cls_cluster0 = q.cls_cluster0; cj.cls_rot = q.cls_rot;
      cj.xbuf = reinterpret_cast<float*>(base + q.xbuf_off);
    }
    L.cm.status = status;
    L.cm.sticky = mgr_status_block(c);
    L.cm.resident = c->sticky_status + 1;
    L.cm.total_wgs = C.grid;
    // (the ledger counts this launch by its GRID, the forward launch by its live workgroups: mgr_lstm_scan_fwd_multi_ex)
    r = mgr_persist_admit(c, C.grid, C.waves, C.per_cu, C.fused, &L.cm.seq);
    if (r) return r;
    if (seq_out) *seq_out = L.cm.seq;
    MGR_HIP(hipMemsetAsync(base, 0, C.zero_bytes, mgr_stream(c)));
    r = mgr_cluster_bwd_launch(c, L, C);
    if (r) return r;
    r = mgr_persist_commit(c, C.grid, C.waves, C.per_cu, C.fused);
    if (r) return r;
  }
  // the jobs that are left: the single-CU MFMA kernel - ONE launch for all of them when they share a shape - or the simple kernel
  mgr_scan_bwd_job joint[MGR_MAX_SCAN_JOBS];
  int njoint = 0;
  for (int i = 0; i < njobs; ++i)
    if (C.job[i].fallback == MGR_SCAN_FALLBACK_MFMA_JOINT) joint[njoint++] = jobs[i];
  if (njoint > 0) {
    r = mgr_scan_bwd_mfma_multi(c, njoint, joint);
    if (r < 0) return r;
  }
  for (int i = 0; i < njobs; ++i) {
    const mgr_scan_bwd_job& j = jobs[i];
    r = 0;
    if (C.job[i].fallback == MGR_SCAN_FALLBACK_MFMA) {
      r = mgr_scan_bwd_mfma_multi(c, 1, &j);
    } else if (C.job[i].fallback == MGR_SCAN_FALLBACK_SIMPLE) {
      float* UpT = reinterpret_cast<float*>(base + C.job[i].xbuf_off);
      r = mgr_transpose(c, j.Up, UpT, j.H, 4 * j.H);
      if (r) return r;
      r = mgr_scan_bwd_simple(c, j.dY, j.lddy, j.gates, j.cs, UpT, j.dZ, j.B, j.T, j.H, j.reverse);
    }
    if (r < 0) return r;
  }
  for (int i = 0; i < njobs; ++i) {   // the row maxima / sums of dZ where the kernel that ran did not leave them itself
    const mgr_scan_bwd_job& j = jobs[i];
    if ((!j.dzmax && !j.dbsum) || C.job[i].cluster) continue;
    r = mgr_rowmax_bt(c, j.dZ, 4 * j.H, j.T, j.B, j.dzmax, j.dbsum);
    if (r) return r;
  }
  r = mgr_prof_end(c, MGR_K_SCAN_BWD);
  if (r) return r;
  if (C.kernel != MGR_SCAN_BWD_NONE && c->tune[MGR_TUNE_SCAN_SYNC_CHECK]) return check_launch_status(c, status, "cluster BPTT");
  return 0;
}

int mgr_lstm_scan_bwd_describe(int cu_count, const int* tune, int ntune, int njobs, const mgr_scan_bwd_job* jobs, const mgr_scan_launch_opts* opts,
                               mgr_scan_choice* out) {
  MGR_REQUIRE(jobs && njobs > 0 && njobs <= MGR_MAX_SCAN_JOBS, "bad job list");
  MGR_REQUIRE(out && out->struct_size == sizeof(*out) && cu_count > 0, "describe: out->struct_size must be sizeof(mgr_scan_choice), cu_count > 0");
  int form, t[MGR_TUNE_COUNT];
  unsigned* seq_out;
  read_opts(opts, &form, &seq_out);
  int r = check_bwd_form(form);
  if (r) return r;
  r = check_bwd_jobs(njobs, jobs);
  if (r) return r;
  read_tune(tune, ntune, t);
  *out = mgr_scan_bwd_decide(cu_count, t, njobs, jobs, form);
  return 0;
}

int mgr_lstm_scan_bwd(mgr_ctx* c, const float* dY, int lddy, const float* gates, const float* cs, const float* Up,
                      float* dZ, int B, int T, int H, int reverse, void* ws, size_t ws_bytes) {
  mgr_scan_bwd_job j;
  j.dY = dY; j.gates = gates; j.cs = cs; j.Up = Up; j.dZ = dZ;
  j.lddy = lddy; j.B = B; j.T = T; j.H = H; j.reverse = reverse;
  j.dzmax = nullptr; j.dbsum = nullptr;
  return mgr_lstm_scan_bwd_multi(c, 1, &j, ws, ws_bytes);
}

}  // extern "C"

// ---- admission of persistent launches -----------------------------------------------------------------------------------
// A persistent scan's workgroups spin on their peers, so ALL of them must be resident at once.  Inside one launch the grid is
// checked against the chip (mgr_cluster_launch).  Across the streams of a context (the encoder scans of step n+1 beside the
// fusion scan / BPTT of step n, engine.py) this ledger does the same: every persistent launch records (workgroups, waves per
// workgroup, workgroups per CU) and an event behind its kernel; a new launch that would not fit beside the launches that may
// still be running is ORDERED BEHIND them (hipStreamWaitEvent) instead of being allowed to dead-lock with them.  Capacity:
// a CU holds two 4-wave or one 8-wave workgroup of these kernels (they use > 128 VGPRs); as soon as any launch needs a CU of its
// own, every workgroup in flight is counted as a whole CU (4-wave workgroups are dealt one per CU first, so each may block one).
// Kernels that are not persistent (GEMMs, ...) leave on their own and need no entry.
int mgr_persist_admit(mgr_ctx* c, int wgs, int waves_per_wg, int per_cu, int fused, unsigned* seq_out) {
  (void)waves_per_wg;
  bool ordered[MGR_MAX_PERSIST] = {};   // launches this one has been put behind
  for (;;) {
    // launches of ONE stream run one after the other: a stream can hold at most its largest launch on the chip at a time
    int per_stream[MGR_NUM_STREAMS] = {}, cus_stream[MGR_NUM_STREAMS] = {};
    int any_excl = per_cu == 1 ? 1 : 0, any_fused = fused ? 1 : 0, oldest = -1;
    for (int i = 0; i < MGR_MAX_PERSIST; ++i) {
      mgr_ctx::Persist& e = c->persist[i];
      if (!e.active || ordered[i] || e.stream == c->cur) continue;   // (same stream: ordered before this launch anyway)
      if (hipEventQuery(e.done) == hipSuccess) {
        e.active = 0;
        continue;
      }
      per_stream[e.stream] = e.wgs > per_stream[e.stream] ? e.wgs : per_stream[e.stream];
      const int cus = (e.wgs + e.per_cu - 1) / e.per_cu;
      cus_stream[e.stream] = cus > cus_stream[e.stream] ? cus : cus_stream[e.stream];
      any_excl |= e.per_cu == 1;
      any_fused |= e.fused;
      if (oldest < 0 || e.seq < c->persist[oldest].seq) oldest = i;
    }
    int shared = wgs, cus = (wgs + per_cu - 1) / per_cu;
    for (int s = 0; s < MGR_NUM_STREAMS; ++s) {
      shared += per_stream[s];
      cus += cus_stream[s];
    }
    // fused scans (8-wave workgroups that fill a CU's register file - this launch, or one in flight): beside them the 4-wave launches are
    // counted by the CUs they need two to a CU - their caller (the engine) starts them once the exclusive launch is resident, so that
    // they do land there.  (A property of the LAUNCHES in the ledger since round 6, not of a tune key that happens to be set.)
    const bool by_cus = any_excl && any_fused;
    const int capacity = any_excl ? c->cu_count : 2 * c->cu_count;
    if (oldest < 0 || (by_cus ? cus : shared) <= capacity) break;
    // does not fit beside what may still be running: run behind the oldest of them, then look again
    MGR_HIP(hipStreamWaitEvent(mgr_stream(c), c->persist[oldest].done, 0));
    ordered[oldest] = true;
    c->persist_serialised += 1;
  }
  *seq_out = ++c->persist_seq;
  return 0;
}

int mgr_persist_commit(mgr_ctx* c, int wgs, int waves_per_wg, int per_cu, int fused) {
  int slot = -1;
  for (int i = 0; i < MGR_MAX_PERSIST && slot < 0; ++i)
    if (!c->persist[i].active) slot = i;
  if (slot < 0) {   // every entry still marked active: retire those that have finished, else reuse the oldest after waiting for it
    int oldest = 0;
    for (int i = 0; i < MGR_MAX_PERSIST; ++i) {
      if (hipEventQuery(c->persist[i].done) == hipSuccess) slot = i;
      if (c->persist[i].seq < c->persist[oldest].seq) oldest = i;
    }
    if (slot < 0) {
      MGR_HIP(hipEventSynchronize(c->persist[oldest].done));
      slot = oldest;
    }
  }
  mgr_ctx::Persist& e = c->persist[slot];
  if (!e.done) MGR_HIP(hipEventCreateWithFlags(&e.done, hipEventDisableTiming));
  MGR_HIP(hipEventRecord(e.done, mgr_stream(c)));
  e.active = 1;
  e.stream = c->cur;
  e.wgs = wgs;
  e.waves = waves_per_wg;
  e.per_cu = per_cu;
  e.fused = fused ? 1 : 0;
  e.seq = c->persist_seq;
  return 0;
}

namespace {
// One lane polls the context's residency words until the launch with sequence number `seq` has all its workgroups on the chip.
// seq_word != nullptr: the number is not known yet when the wait is enqueued - it arrives in a word of page-locked host memory
// that the launch's call fills in (mgr_scan_launch_opts.seq_out); MGR_SEQ_NONE there = no such launch: nothing to wait for.
// counters[0] counts the waits that have ended, counters[1] those that ended by their timeout (mgr_resident_wait_stats).
__global__ void k_wait_resident(const unsigned* resident, const unsigned* ring, const unsigned* seq_word, unsigned seq, unsigned timeout_us,
                                unsigned* counters) {
  const unsigned long long t0 = wall_clock64();   // 100 MHz
  bool expired = false;
  for (;;) {
    if (seq_word && seq == 0u) seq = __hip_atomic_load(seq_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (seq == MGR_SEQ_NONE) break;
    if (seq != 0u) {
      const unsigned* w = ring ? ring + (seq & 15u) : resident;
      if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= seq) break;
    }
    __builtin_amdgcn_s_sleep(32);
    if (wall_clock64() - t0 > 100ull * timeout_us) {   // placement hint only: never a correctness dependency
      expired = true;
      break;
    }
  }
  __hip_atomic_fetch_add(counters, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (expired) {
    __hip_atomic_fetch_add(counters + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    counters[2] = seq;                                             // diagnostics of the LAST expired wait: the launch number it was for (0: never
    counters[3] = (unsigned)reinterpret_cast<uintptr_t>(seq_word); // learnt) and the low 32 bits of the word it polled (0: a known-number wait)
  }
}
constexpr int kWaitCounters = 32;   // words [32, 34) of the context's own status block
}  // namespace

extern "C" {

int mgr_stream_wait_next_resident(mgr_ctx* c, int timeout_us) {
  MGR_REQUIRE(c && timeout_us >= 0 && timeout_us <= 100000, "timeout_us must be in [0, 100000]");
  hipLaunchKernelGGL(k_wait_resident, dim3(1), dim3(1), 0, mgr_stream(c), c->sticky_status + 1, nullptr, nullptr, c->persist_seq + 1,
                     (unsigned)timeout_us, c->sticky_status + kWaitCounters);
  MGR_LAUNCH_CHECK();
  return 0;
}

int mgr_stream_wait_resident(mgr_ctx* c, unsigned seq, int timeout_us) {
  MGR_REQUIRE(c && timeout_us >= 0 && timeout_us <= 100000, "timeout_us must be in [0, 100000]");
  MGR_REQUIRE(seq != 0u, "launch numbers start at 1");
  hipLaunchKernelGGL(k_wait_resident, dim3(1), dim3(1), 0, mgr_stream(c), c->sticky_status + 1, c->sticky_status + 16, nullptr, seq,
                     (unsigned)timeout_us, c->sticky_status + kWaitCounters);
  MGR_LAUNCH_CHECK();
  return 0;
}

int mgr_stream_wait_resident_word(mgr_ctx* c, const unsigned* seq_word, int timeout_us) {
  MGR_REQUIRE(c && seq_word && timeout_us >= 0 && timeout_us <= 100000, "null word / timeout_us must be in [0, 100000]");
  hipLaunchKernelGGL(k_wait_resident, dim3(1), dim3(1), 0, mgr_stream(c), c->sticky_status + 1, c->sticky_status + 16, seq_word, 0u,
                     (unsigned)timeout_us, c->sticky_status + kWaitCounters);
  MGR_LAUNCH_CHECK();
  return 0;
}

int mgr_resident_wait_stats(mgr_ctx* c, unsigned out[4]) {
  MGR_REQUIRE(c && out, "null argument");
  MGR_HIP(hipMemcpyAsync(out, c->sticky_status + kWaitCounters, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, mgr_stream(c)));
  MGR_HIP(hipStreamSynchronize(mgr_stream(c)));
  return 0;
}

int mgr_persist_stats(mgr_ctx* c, int* launches, int* serialised) {
  MGR_REQUIRE(c, "null ctx");
  if (launches) *launches = (int)c->persist_seq;
  if (serialised) *serialised = c->persist_serialised;
  return 0;
}

}  // extern "C"
