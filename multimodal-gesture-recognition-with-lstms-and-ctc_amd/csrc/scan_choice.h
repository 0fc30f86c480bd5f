// What a multi-scan call launches (plain host C++17, no HIP types, no context): which shapes have an instantiation, and ONE pure
// function per direction that decides, for a job list, the launch options and the tune keys, everything the launchers of lstm.hip /
// lstm_cluster.hip / lstm_cluster_bwd.hip then only carry out - kernel, grid, LDS, ledger entry, class layout, workspace offsets,
// fallbacks.  Every quantity is computed once, here.  The value is mgr_scan_choice (include/mgr.h): mgr_lstm_scan_fwd_describe /
// mgr_lstm_scan_bwd_describe print it without a GPU (tests/test_cpu_scan_choice.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/mgr.h"
#include "ws_layout.h"

constexpr int MGR_MAX_SCAN_JOBS = MGR_SCAN_CHOICE_MAX_JOBS;
constexpr size_t kScanHdrBytes = 4096;   // header of every persistent launch's workspace (lstm_cluster.h)

// ---- the instantiation lists: the single statement of which shapes exist (the .hip files expand them from here)
// forward LDS-image step, cluster_run<KS, TPW>: (k-steps = H / 4, tiles per wave)
#define CL_FOREACH(X) \
  X(125, 1) X(75, 1) X(75, 2) X(32, 1) X(32, 2) X(32, 4) X(25, 1) X(25, 2) X(25, 4) X(16, 1) X(16, 2) X(8, 1) X(8, 2) \
  X(4, 1) X(3, 1) X(2, 1) X(1, 1)
// forward K-split steps, cluster_run_ks<KS> / cluster_run_k16: k-steps, by layer width (two kernels: lstm_cluster.hip)
#define CLKS_LARGE(X) X(125) X(75)
#define CLKS_SMALL(X) X(32) X(25)
#define CLKS_FOREACH(X) CLKS_LARGE(X) CLKS_SMALL(X)
// BPTT cluster kernels, cluster_bwd_run<H> / cluster_bwd_run16<H>: H, by layer width
#define BW_SMALL(X) X(8) X(16) X(32) X(64) X(100) X(128)
#define BW_LARGE(X) X(300) X(500)
#define BW_FOREACH(X) BW_SMALL(X) BW_LARGE(X)
// single-CU split-f16 BPTT, k_scan_bwd_cu16<H> (H = 128: eight tiles - image + rings would need 160.1 KiB of LDS; it keeps the multi-CU forms)
#define CB_FOREACH(X) X(32) X(64) X(100)
// single-CU f32 MFMA BPTT, k_scan_bwd_mfma<H>
#define BWD_MFMA_FOREACH(X) X(4) X(8) X(16) X(32) X(64) X(100) X(128)

#define MGR_CASE1_(V) \
  if (v == V) return true;
#define MGR_CASE2_(A, B) \
  if (a == A && b == B) return true;
inline bool mgr_cluster_supported(int a, int b) { CL_FOREACH(MGR_CASE2_) return false; }   // (ks, tpw)
inline bool mgr_cluster_ks_supported(int v) { CLKS_FOREACH(MGR_CASE1_) return false; }    // ks
inline bool mgr_cluster_bwd_supported(int v) { BW_FOREACH(MGR_CASE1_) return false; }     // H
inline bool mgr_scan_bwd_cu16_supported(int v) { CB_FOREACH(MGR_CASE1_) return false; }   // H
inline bool mgr_scan_bwd_mfma_supported(int v) { BWD_MFMA_FOREACH(MGR_CASE1_) return false; }   // H
#undef MGR_CASE1_
#undef MGR_CASE2_

// ---- dynamic LDS of the kernels, in bytes (each .hip file asserts these against the layout its kernels use)
constexpr size_t kScanLdsKs = 51200;                 // k_scan_cluster_ks[_s]
constexpr size_t kScanLdsK16 = 52288;                // k_scan_cluster_k16[_s]
constexpr size_t kScanLdsK16Fused = 2 * kScanLdsK16 + 4 * 4 * 2 * 256 * sizeof(float);   // k_scan_cluster_k16fs: two halves + their exchange
constexpr size_t kScanLdsBwdA = 27712;               // cluster_bwd_run
constexpr size_t kScanLdsBwdB = 36928;               // cluster_bwd_run16
constexpr size_t kScanLdsAlone = 84 * 1024;          // a request of this size keeps a workgroup alone on its CU
constexpr size_t mgr_scan_bwd_cu16_lds(int H) {      // k_scan_bwd_cu16<H>: two dz images, the factors, per tile two ring slots + four cell slots
  return ((size_t)2 * (2 * ((H + 15) / 16)) * 2 * 64 * 4 + 32 + (size_t)((H + 15) / 16) * (2 * (4 + 1) * 64 * 4 + 4 * 64 * 4)) * sizeof(float);
}
// floats of BPTT exchange memory per batch group and slot: [dest G][src G][256]
inline size_t mgr_cluster_bwd_img_floats(int H) {
  size_t g = (size_t)(H + 15) / 16;
  return g * g * 256;
}

// ---- kernel names, by mgr_scan_choice::kernel
inline const char* mgr_scan_fwd_kernel_name(int k) {
  static const char* const n[] = {"", "k_scan_cluster", "k_scan_cluster_ks", "k_scan_cluster_ks_s", "k_scan_cluster_k16", "k_scan_cluster_k16_s",
                                  "k_scan_cluster_k16fs"};
  return k >= 0 && k <= MGR_SCAN_FWD_K16_FUSED ? n[k] : "?";
}
inline const char* mgr_scan_bwd_kernel_name(int k) {
  static const char* const n[] = {"", "k_scan_cluster_bwd", "k_scan_cluster_bwd_s", "k_scan_cluster_bwd_split", "k_scan_cluster_bwd16",
                                  "k_scan_cluster_bwd16_s", "k_scan_cluster_bwd16_sl", "k_scan_cluster_bwd16_sd", "k_scan_cluster_bwd16_split",
                                  "k_scan_cluster_bwd16_f", "k_scan_cluster_bwd16_fd"};
  return k >= 0 && k <= MGR_SCAN_BWD_16_FD ? n[k] : "?";
}

// ---- class layout.  Jobs with identical geometry (the two directions of a layer) form a class that shares one contiguous range of
// workgroups; every class starts on a multiple of 8 (the XCD round-robin).  octets: a class takes whole octets of clusters (XCD-local
// layout) and its first cluster the lane after the previous class's last.  Fills cls_* of the jobs in use; returns the grid size.
template <class SameFn, class SizeFn>
inline int mgr_scan_layout_classes(int njobs, mgr_scan_choice_job* job, SameFn same, SizeFn members_of, bool octets) {
  int cls_of[MGR_MAX_SCAN_JOBS], ncls = 0, cls_first[MGR_MAX_SCAN_JOBS], cls_clusters[MGR_MAX_SCAN_JOBS];
  for (int i = 0; i < njobs; ++i) {
    if (!job[i].cluster) continue;
    int found = -1;
    for (int k = 0; k < ncls; ++k)
      if (same(cls_first[k], i)) found = k;
    if (found < 0) {
      found = ncls++;
      cls_first[found] = i;
      cls_clusters[found] = 0;
    }
    cls_of[i] = found;
    cls_clusters[found] += job[i].nbg;
  }
  int cls_begin[MGR_MAX_SCAN_JOBS], cls_next[MGR_MAX_SCAN_JOBS], cls_rot[MGR_MAX_SCAN_JOBS], begin = 0, lanes = 0;
  for (int k = 0; k < ncls; ++k) {
    begin = (begin + 7) / 8 * 8;
    cls_begin[k] = begin;
    cls_next[k] = 0;
    cls_rot[k] = lanes & 7;   // (XCD-local layout) this class's first cluster takes the lane after the previous class's last
    lanes += cls_clusters[k];
    begin += members_of(cls_first[k]) * (octets ? (cls_clusters[k] + 7) / 8 * 8 : cls_clusters[k]);
  }
  for (int i = 0; i < njobs; ++i) {
    if (!job[i].cluster) continue;
    const int k = cls_of[i];
    job[i].cls_begin = cls_begin[k];
    job[i].cls_nclusters = cls_clusters[k];
    job[i].cls_cluster0 = cls_next[k];
    job[i].cls_rot = octets ? cls_rot[k] : 0;
    cls_next[k] += job[i].nbg;
  }
  return begin;
}
inline bool mgr_scan_xcd_table_fits(int grid) { return (size_t)grid * sizeof(unsigned) <= kScanHdrBytes - 256; }   // (the header's table of XCD ids)

// ---- workspace layouts (ws_layout.h: one function per workspace, offsets only - the launchers add their base)
// forward: header | exchange images of the jobs in `images` (null: every job), packed in job order | ... up to base = header + the
// images of EVERY job | row scratch, packed [B][T][H], of the jobs in `scratch` (null: every job without Y that has a YT)
struct mgr_scan_fwd_ws { size_t xbuf[MGR_MAX_SCAN_JOBS], rows[MGR_MAX_SCAN_JOBS], zero_bytes, base_bytes, bytes; };
inline size_t mgr_scan_fwd_image_floats(const mgr_scan_job& j) {
  // two images per 16-sample group; 1 KiB per 16 units, in whole K-blocks of 32 (the split-f16 step's image)
  return (size_t)((j.B + 15) / 16) * 2 * ((size_t)((j.H / 4 + 7) / 8) * 512);
}
inline mgr_scan_fwd_ws mgr_scan_fwd_ws_layout(int njobs, const mgr_scan_job* jobs, const mgr_scan_choice_job* images, const mgr_scan_choice_job* scratch) {
  mgr_scan_fwd_ws L = {};
  mgr_ws_carver w(nullptr), all(nullptr);
  w.take<char>(kScanHdrBytes);
  all.take<char>(kScanHdrBytes);
  for (int i = 0; i < njobs; ++i) {
    all.take<float>(mgr_scan_fwd_image_floats(jobs[i]));
    if (i >= MGR_MAX_SCAN_JOBS || (images && !images[i].cluster)) continue;   // (the context-free queries take any job count)
    L.xbuf[i] = w.off;
    w.take<float>(mgr_scan_fwd_image_floats(jobs[i]));
  }
  L.zero_bytes = w.off;   // (exchange slots + header: zero at every launch)
  L.base_bytes = all.off;
  for (int i = 0; i < njobs; ++i) {
    if (scratch ? !scratch[i].rows_in_scratch : !(!jobs[i].Y && jobs[i].YT)) continue;
    if (i < MGR_MAX_SCAN_JOBS) L.rows[i] = all.off;
    all.take<float>((size_t)jobs[i].B * jobs[i].T * jobs[i].H);
  }
  L.bytes = all.off;
  return L;
}
// backward: header | per job the larger of the cluster kernel's exchange images and U^T of the simple kernel
struct mgr_scan_bwd_ws { size_t job[MGR_MAX_SCAN_JOBS], bytes; };
inline mgr_scan_bwd_ws mgr_scan_bwd_ws_layout(int njobs, const mgr_scan_bwd_job* jobs) {
  mgr_scan_bwd_ws L = {};
  mgr_ws_carver w(nullptr);
  w.take<char>(kScanHdrBytes);
  for (int i = 0; i < njobs; ++i) {
    if (i < MGR_MAX_SCAN_JOBS) L.job[i] = w.off;
    const mgr_scan_bwd_job& j = jobs[i];
    w.take<float>(std::max((size_t)((j.B + 15) / 16) * 2 * mgr_cluster_bwd_img_floats(j.H), (size_t)4 * j.H * j.H));
  }
  L.bytes = w.off;
  return L;
}

// ---- forward.  form: MGR_SCAN_FORM_* (checked by the caller); ws_avail: bytes of workspace the call was given ((size_t)-1: as much
// as it takes - the workspace query); jobs: checked by the caller (H, B, T > 0, Y or YT).
inline mgr_scan_choice mgr_scan_fwd_decide(int cu_count, const int* tune, int njobs, const mgr_scan_job* jobs, int form, size_t ws_avail) {
  struct Cfg { int nw, tpw; };
  constexpr int NCFG = 4;   // candidate (active waves, tiles per wave) configurations
  const Cfg kCfgs[NCFG] = {{4, 1}, {8, 1}, {8, 2}, {8, 4}};
  mgr_scan_choice C = {};
  C.struct_size = (unsigned)sizeof(C);
  C.njobs = njobs;
  mgr_scan_choice_job* J = C.job;
  const int path = tune[MGR_TUNE_SCAN_PATH];
  // the form of the split-f16 K-split launches: the caller's, or MGR_TUNE_SCAN_FORM (3 fused, anything else plain)
  const bool want_fused = form == MGR_SCAN_FORM_AUTO ? tune[MGR_TUNE_SCAN_FORM] == MGR_SCAN_FORM_FUSED : form >= MGR_SCAN_FORM_FUSED;
  const bool fused_any = form == MGR_SCAN_FORM_FUSED_ANY;

  // -- the plan: per-job configurations that minimise the slowest job's per-step MFMA time subject to all workgroups being co-resident
  // (sum <= CUs).  Jobs that cannot run on the cluster kernel are left to the other families.
  int idx[MGR_MAX_SCAN_JOBS], n = 0;
  for (int i = 0; i < njobs; ++i) {
    const int H = jobs[i].H, ks = H / 4;
    bool ok = false;
    for (int k = 0; k < NCFG && H % 4 == 0; ++k) ok = ok || mgr_cluster_supported(ks, kCfgs[k].tpw);
    if (path == 1) ok = false;
    J[i].nbg = (jobs[i].B + 15) / 16;
    if (ok) idx[n++] = i;
  }
  // what a (job, configuration) pair contributes, whatever the other jobs take: computed once per pair, not once per combination
  struct Cand { bool ok, exch; int wgs8; long t, t_shared; } cand[MGR_MAX_SCAN_JOBS][NCFG];
  int maxks = 0;
  for (int k = 0; k < n; ++k) {
    const int ks = jobs[idx[k]].H / 4;
    maxks = std::max(maxks, ks);
    for (int q = 0; q < NCFG; ++q) {
      const Cfg f = kCfgs[q];
      const int tiles = f.nw * f.tpw, G = (ks + tiles - 1) / tiles;
      Cand& d = cand[k][q];
      d.ok = mgr_cluster_supported(ks, f.tpw) && !(path == 3 && q != 0) && !(path == 4 && q != 1) &&
             !(path == 2 && tiles < ks) &&   // (path 2: force single-CU, no exchange)
             G <= 64;
      d.exch = G > 1;
      // (classes of jobs are laid out on workgroup ranges rounded up to a multiple of 8 - the XCD count - at launch; count
      // every job rounded up so that a plan accepted here always passes the launcher's co-residency check)
      d.wgs8 = (G * J[idx[k]].nbg + 7) / 8 * 8;
      // per-step estimate in cycles: MFMA chain per SIMD (+15% issue overhead) + cell update + exchange / barrier
      const int per_simd = (std::min(tiles, ks) + 3) / 4;
      d.t = (long)per_simd * ks * 37 + 700 + (G > 1 ? 3300 : 400);
      d.t_shared = (long)per_simd * ks * 12;   // a second workgroup on the CU competes for the MFMA pipe part of the time
    }
  }
  int best[MGR_MAX_SCAN_JOBS], cur[MGR_MAX_SCAN_JOBS];
  long best_cost = -1;
  int combos = 1;
  for (int k = 0; k < n; ++k) combos *= NCFG;
  for (int code = 0; code < combos && n > 0; ++code) {
    int x = code, total = 0;
    long worst = 0, sum = 0;
    bool feas = true, exch = false, all4 = true;
    for (int k = 0; k < n && feas; ++k) {
      cur[k] = x % NCFG;
      x /= NCFG;
      const Cand& d = cand[k][cur[k]];
      feas = d.ok;
      exch = exch || d.exch;
      all4 = all4 && kCfgs[cur[k]].nw == 4;
      total += d.wgs8;
      const long t = d.t + (total > cu_count ? d.t_shared : 0);
      worst = std::max(worst, t);
      sum += t;
    }
    // capacity: one 8-wave workgroup per CU, or two 4-wave workgroups (<= 80 KiB LDS each) per CU
    const size_t lds2 = (size_t)2 * ((maxks + 3) / 4) * 1024;
    const int capacity = (all4 && lds2 <= 80 * 1024) ? 2 * cu_count : cu_count;
    if (!feas || (exch && total > capacity)) continue;
    long cost = worst * 1000 + sum / n;
    if (best_cost < 0 || cost < best_cost) {
      best_cost = cost;
      for (int k = 0; k < n; ++k) best[k] = cur[k];
    }
  }
  C.base_need = mgr_scan_fwd_ws_layout(njobs, jobs, nullptr, nullptr).base_bytes;
  // (does not fit: these jobs go to the fallback; so do all when there is no workspace for the exchange - the degrade rule)
  const bool any = best_cost >= 0 && ws_avail >= C.base_need;
  C.degraded = best_cost >= 0 && !any;
  bool all_ks_shape = true, small = true;   // every cluster job a 4-wave, one-tile-per-wave cluster with an exchange and a K-split instantiation
  int maxnw = 0, unfused = 0;
  size_t image_lds = 0;
  for (int k = 0; k < n && any; ++k) {
    const int i = idx[k], ks = jobs[i].H / 4;
    J[i].cluster = 1;
    J[i].nw = kCfgs[best[k]].nw;
    J[i].tpw = kCfgs[best[k]].tpw;
    J[i].G = (ks + J[i].nw * J[i].tpw - 1) / (J[i].nw * J[i].tpw);
    if (J[i].G > 1) C.exchange = 1;
    all_ks_shape = all_ks_shape && J[i].nw == 4 && J[i].tpw == 1 && J[i].G > 1 && mgr_cluster_ks_supported(ks);
    small = small && ks <= 32;
    maxnw = std::max(maxnw, J[i].nw);
    unfused += J[i].G * J[i].nbg;
    image_lds = std::max(image_lds, 2 * (size_t)((ks + 3) / 4) * 256 * sizeof(float));
  }
  for (int i = 0; i < njobs; ++i) J[i].fallback = J[i].cluster ? MGR_SCAN_FALLBACK_NONE : MGR_SCAN_FALLBACK_SIMPLE;
  if (any) {
    // the K-split step addresses Z and the residual input with 32-bit byte offsets per lane (LDS-DMA prefetch): launches with a
    // larger tensor take the LDS-image step
    bool ks_ok = tune[MGR_TUNE_SCAN_LDS_IMAGE] == 0;
    for (int i = 0; i < njobs && ks_ok; ++i) {
      if (!J[i].cluster) continue;
      const mgr_scan_job& j = jobs[i];
      const size_t zb = (size_t)j.B * j.T * 4 * j.H * sizeof(float), rb = j.R ? (size_t)j.B * j.T * j.ldr * sizeof(float) : 0;
      ks_ok = zb < ((size_t)1 << 32) && rb < ((size_t)1 << 32);
    }
    C.ksplit = ks_ok;
    C.split16 = tune[MGR_TUNE_SCAN_F32_MFMA] == 0;
    // THE eligibility for the K-split kernels (which honour YT, and understand the XCD-local layout)
    const bool ks = ks_ok && C.exchange && all_ks_shape;
    // Fused form (k_scan_cluster_k16fs): 8-wave workgroups that run TWO unit groups of their cluster, one workgroup per CU (config F's
    // encoder depths: 208 workgroups on 208 CUs, 48 CUs left to the other stream) - only launches that do not fit one workgroup per CU
    // as they are (the fusion layer's 56 workgroups stay what they are), unless asked for ANY
    const bool fused_wanted = ks && C.split16 && want_fused && tune[MGR_TUNE_SCAN_NO_XCD_LOCAL] == 0 && (fused_any || unfused > cu_count);
    // K-split launches lay their clusters out XCD-locally (MGR_TUNE_SCAN_NO_XCD_LOCAL = 1 turns that off): octets of clusters - the
    // grid may grow; it must still fit the chip and the header's table
    bool xcd = ks && tune[MGR_TUNE_SCAN_NO_XCD_LOCAL] == 0;
    if (xcd) {
      int tot = 0, live_x = 0;
      for (int i = 0; i < njobs; ++i) {
        if (!J[i].cluster) continue;
        bool seen = false;
        for (int k = 0; k < i; ++k) seen = seen || (J[k].cluster && jobs[k].H == jobs[i].H);
        if (seen) continue;
        int clusters = 0;
        for (int k = i; k < njobs; ++k)
          if (J[k].cluster && jobs[k].H == jobs[i].H) clusters += J[k].nbg;
        const int m = fused_wanted ? (J[i].G + 1) / 2 : J[i].G;
        tot += m * ((clusters + 7) / 8 * 8);
        live_x += m * clusters;
      }
      xcd = live_x <= (fused_wanted ? 1 : 2) * cu_count && tot <= 2 * cu_count && mgr_scan_xcd_table_fits(tot);
    }
    C.xcd_local = xcd;
    C.fused = fused_wanted && xcd;   // (the fused kernel understands the octet layout only)
    // workgroups that really run (a class laid out in octets of clusters has empty ids when its cluster count is no multiple of 8:
    // those workgroups count themselves in and return): what co-residency and the admission ledger are about
    for (int i = 0; i < njobs; ++i) {
      if (!J[i].cluster) continue;
      J[i].members = C.fused ? (J[i].G + 1) / 2 : J[i].G;
      C.live += J[i].members * J[i].nbg;
    }
    C.grid = mgr_scan_layout_classes(
        njobs, J, [&](int a, int b) { return jobs[a].H == jobs[b].H && J[a].nw == J[b].nw && J[a].tpw == J[b].tpw; },
        [&](int a) { return J[a].members; }, xcd);
    // geometry: 4-wave workgroups with <= 80 KiB of LDS fit two per CU (8 waves, <= 256 VGPRs each); anything else sits alone on its CU
    C.waves = maxnw <= 4 ? 4 : 8;
    C.per_cu = (C.waves == 4 && (ks || image_lds <= 80 * 1024)) ? 2 : 1;
    if (C.fused) {   // (8 waves, 134 KiB, a CU of its own)
      C.kernel = MGR_SCAN_FWD_K16_FUSED;
      C.waves = 8;
      C.per_cu = 1;
      C.lds_bytes = (int)kScanLdsK16Fused;
    } else if (ks) {
      // partial-sum exchange, staging tiles of the transposed output, Z / R rings (no h image): 50 KiB, two workgroups per CU
      C.kernel = C.split16 ? (small ? MGR_SCAN_FWD_K16_S : MGR_SCAN_FWD_K16) : (small ? MGR_SCAN_FWD_KS_S : MGR_SCAN_FWD_KS);
      C.lds_bytes = (int)(C.split16 ? kScanLdsK16 : kScanLdsKs);
    } else {
      C.kernel = MGR_SCAN_FWD_IMAGE;
      // (a workgroup that must sit alone on its CU beside peers it spins on says so through its LDS request)
      C.lds_bytes = (int)(C.exchange && C.per_cu == 1 ? std::max(image_lds, kScanLdsAlone) : image_lds);
    }
    C.block = C.waves * 64;
    // (a launch without an exchange spins on nobody: it needs no place in the ledger and is never ordered behind one)
    C.ledger = C.exchange;
    // transposed outputs: the K-split kernels write them themselves; everything else gets a transpose behind the scans
    for (int i = 0; i < njobs; ++i) J[i].yt_in_kernel = J[i].cluster && ks && jobs[i].YT != nullptr;
  }
  // Where each job's rows go: its Y - or, for a job that gave none and whose kernel does not write the transposed copy itself (the
  // transpose behind the scans reads rows), scratch behind the exchange images.  (A K-split job without Y keeps its NULL: the kernel
  // skips the row store.)
  for (int i = 0; i < njobs; ++i) J[i].rows_in_scratch = !jobs[i].Y && !J[i].yt_in_kernel;
  const mgr_scan_fwd_ws W = mgr_scan_fwd_ws_layout(njobs, jobs, J, J);
  for (int i = 0; i < njobs; ++i) {
    J[i].xbuf_off = W.xbuf[i];
    J[i].rows_off = W.rows[i];
  }
  C.zero_bytes = any ? W.zero_bytes : 0;
  C.need = W.bytes;
  return C;
}

// ---- backward.  form: MGR_BPTT_FORM_* (checked by the caller); jobs: checked by the caller.
inline mgr_scan_choice mgr_scan_bwd_decide(int cu_count, const int* tune, int njobs, const mgr_scan_bwd_job* jobs, int form) {
  mgr_scan_choice C = {};
  C.struct_size = (unsigned)sizeof(C);
  C.njobs = njobs;
  mgr_scan_choice_job* J = C.job;
  const int path = tune[MGR_TUNE_SCAN_PATH];
  const bool f16 = tune[MGR_TUNE_SCAN_F32_MFMA] == 0;   // split-f16 operands (MGR_TUNE_SCAN_F32_MFMA = 1: f32 MFMA)
  const bool cluster_path = path == 0 || path == 3;
  const bool want_fused = form == MGR_BPTT_FORM_FUSED || form == MGR_BPTT_FORM_FUSED_DIRECT;
  // 0 trimmed, 1 yielding, 2 direct gather (the fused forms: the trimmed step / the direct gather)
  const int form16 = form == MGR_BPTT_FORM_AUTO ? tune[MGR_TUNE_BPTT_FORM]
                     : (form == MGR_BPTT_FORM_FUSED || form == MGR_BPTT_FORM_SINGLE_CU) ? 0 : form == MGR_BPTT_FORM_FUSED_DIRECT ? 2 : form - 1;
  const mgr_scan_bwd_ws W = mgr_scan_bwd_ws_layout(njobs, jobs);
  C.base_need = C.need = W.bytes;
  for (int i = 0; i < njobs; ++i) {
    J[i].nbg = (jobs[i].B + 15) / 16;
    J[i].G = J[i].members = (jobs[i].H + 15) / 16;
    J[i].xbuf_off = W.job[i];   // (the simple kernel's U^T takes the same block)
  }
  // the 32-bit byte offsets per lane of the LDS-DMA prefetch (cluster kernels, single-CU split-f16 form)
  auto small = [&](const mgr_scan_bwd_job& j) {
    return (size_t)j.B * j.T * j.H * 16 < ((size_t)1 << 32) && (size_t)j.B * j.T * j.lddy * 4 < ((size_t)1 << 32);
  };
  // The single-CU split-f16 form (lstm_cu_bwd.hip): asked for by the caller (or MGR_TUNE_BPTT_SINGLE_CU = 1), taken when the jobs are
  // the directions of ONE narrow layer (same shape, an instantiation, operands laid out for the 16-byte LDS-DMA rows) and the f16
  // matrix pipe is in use; (B + 15) / 16 x njobs workgroups, a CU each; no inter-CU exchange, no ledger entry
  bool single = (form == MGR_BPTT_FORM_SINGLE_CU || (form == MGR_BPTT_FORM_AUTO && tune[MGR_TUNE_BPTT_SINGLE_CU] == 1)) && f16 && cluster_path &&
                mgr_scan_bwd_cu16_supported(jobs[0].H) && jobs[0].lddy % 4 == 0 && small(jobs[0]);
  for (int i = 0; i < njobs && single; ++i)
    single = jobs[i].B == jobs[0].B && jobs[i].T == jobs[0].T && jobs[i].H == jobs[0].H && jobs[i].lddy == jobs[0].lddy &&
             !(reinterpret_cast<uintptr_t>(jobs[i].dY) & 15) && !(reinterpret_cast<uintptr_t>(jobs[i].cs) & 15);
  if (single) {
    C.single_cu = 1;
    C.grid = C.live = J[0].nbg * njobs;
    C.waves = 8;
    C.per_cu = 1;
    C.block = 512;
    C.lds_bytes = (int)mgr_scan_bwd_cu16_lds(jobs[0].H);
    for (int i = 0; i < njobs; ++i) J[i].fallback = MGR_SCAN_FALLBACK_CU16;
    return C;
  }
  // cluster kernel when instantiated and the whole launch is co-resident (two 4-wave workgroups per CU)
  int total = 0;
  for (int i = 0; i < njobs; ++i) {
    J[i].cluster = cluster_path && mgr_cluster_bwd_supported(jobs[i].H) && small(jobs[i]);
    if (J[i].cluster) total += J[i].G * J[i].nbg;
  }
  if (total + 8 * njobs > 2 * cu_count)
    for (int i = 0; i < njobs; ++i) J[i].cluster = 0;
  int ncluster = 0, maxH = 0;
  bool narrow = true, all_small = true;   // narrow: what the fused form runs (16 < H <= 128); all_small: the kernels of the narrow layers
  for (int i = 0; i < njobs; ++i) {
    if (!J[i].cluster) continue;
    ++ncluster;
    maxH = std::max(maxH, jobs[i].H);
    C.exchange = C.exchange || J[i].G > 1;
    narrow = narrow && jobs[i].H > 16 && jobs[i].H <= 128;
    all_small = all_small && jobs[i].H <= 128;
  }
  if (ncluster > 0) {
    auto same_h = [&](int a, int b) { return jobs[a].H == jobs[b].H; };
    auto fits = [&](int grid, int per_cu) { return grid <= per_cu * cu_count && mgr_scan_xcd_table_fits(grid); };
    // Candidate layouts, each computed once.  XCD-local (octets of clusters) where the padded grid still fits the chip and the header's
    // table (MGR_TUNE_SCAN_NO_XCD_LOCAL = 1: off).  Fused form (k_scan_cluster_bwd16_f / _fd): asked for by the caller, taken when
    // EVERY job of the call qualifies - the same clusters with ceil(G / 2) eight-wave members, a CU each, in octets
    mgr_scan_choice octet = C, fused = C;
    const int grid_plain = mgr_scan_layout_classes(njobs, J, same_h, [&](int a) { return J[a].G; }, false);
    const int grid_octet = mgr_scan_layout_classes(njobs, octet.job, same_h, [&](int a) { return J[a].G; }, true);
    const int grid_fused = mgr_scan_layout_classes(njobs, fused.job, same_h, [&](int a) { return (J[a].G + 1) / 2; }, true);
    C.grid = grid_plain;
    if (tune[MGR_TUNE_SCAN_NO_XCD_LOCAL] == 0 && fits(grid_octet, 2)) {
      C.xcd_local = 1;
      C.grid = grid_octet;
      C.fused = want_fused && f16 && narrow && ncluster == njobs && fits(grid_fused, 1);
      if (C.fused) C.grid = grid_fused;
      const mgr_scan_choice& from = C.fused ? fused : octet;
      for (int i = 0; i < njobs; ++i) {
        J[i] = from.job[i];
        if (C.fused) J[i].members = (J[i].G + 1) / 2;
      }
    }
    C.live = C.grid;
    // split roles (8 waves, > 80 KiB of LDS requested so that exactly one workgroup sits on a CU) whenever the launch fits one
    // workgroup per CU, has an exchange at all and the layers are wide: at H = 100 (7 workgroups per cluster, two 16-byte stores
    // per lane and step) the store acknowledgement is 0.35 of 2.2 us and the 8-wave workgroups cost config F 0.7 % end to end,
    // at H = 300 / 500 they save a third of the step (E: 60 -> 48 ms/step, S_ref 24 -> 21).  MGR_TUNE_BPTT_SPLIT_ROLE: 1 = never, 2 = always.
    const int key = tune[MGR_TUNE_BPTT_SPLIT_ROLE];
    C.split = !C.fused && C.exchange && (maxH >= 200 || key == 2) && C.grid <= cu_count && key != 1;
    C.split16 = f16;
    C.waves = C.fused || C.split ? 8 : 4;
    C.per_cu = C.fused || C.split ? 1 : 2;
    C.block = C.waves * 64;
    if (C.fused) {   // (>= 84 KiB requested: the workgroup sits alone on its CU whatever its registers would allow)
      C.kernel = form16 == 2 ? MGR_SCAN_BWD_16_FD : MGR_SCAN_BWD_16_F;
      C.lds_bytes = (int)std::max(2 * kScanLdsBwdB, kScanLdsAlone);
    } else if (C.split) {
      C.kernel = f16 ? MGR_SCAN_BWD_16_SPLIT : MGR_SCAN_BWD_SPLIT;
      C.lds_bytes = (int)kScanLdsAlone;
    } else {
      C.kernel = all_small && f16 ? (form16 == 2 ? MGR_SCAN_BWD_16_SD : form16 == 0 ? MGR_SCAN_BWD_16_SL : MGR_SCAN_BWD_16_S)
                 : all_small ? MGR_SCAN_BWD_S : f16 ? MGR_SCAN_BWD_16 : MGR_SCAN_BWD;
      C.lds_bytes = (int)(C.kernel == MGR_SCAN_BWD_16_SD || C.kernel == MGR_SCAN_BWD_16_SL ? kScanLdsBwdB : kScanLdsBwdA);
    }
    C.ledger = 1;   // (every BPTT cluster launch takes its place in the ledger, exchange or not)
    C.zero_bytes = W.bytes;
  }
  // the single-CU MFMA kernel takes every job that is left in ONE launch when they share a shape (the two directions of a layer); else
  // one launch each where the width has an instantiation; else the simple kernel (MGR_TUNE_SCAN_PATH = 1: always)
  int first = -1;
  bool same = true;
  for (int i = 0; i < njobs; ++i) {
    if (J[i].cluster) continue;
    if (first < 0) first = i;
    same = same && jobs[i].B == jobs[first].B && jobs[i].T == jobs[first].T && jobs[i].H == jobs[first].H && jobs[i].lddy == jobs[first].lddy;
  }
  for (int i = 0; i < njobs; ++i) {
    if (J[i].cluster) continue;
    J[i].fallback = path == 1 || !mgr_scan_bwd_mfma_supported(jobs[i].H) ? MGR_SCAN_FALLBACK_SIMPLE
                    : same ? MGR_SCAN_FALLBACK_MFMA_JOINT : MGR_SCAN_FALLBACK_MFMA;
  }
  return C;
}
