// Stand-alone host program (its own main, no HIP, no GPU): walks job shapes through the two decision functions of csrc/scan_choice.h
// and prints each choice.  tests/test_cpu_scan_choice.py builds it with -fsanitize=address,undefined and feeds it the shapes of
// tests/golden/scan_choices.json at several CU counts: the fixed-size [MGR_MAX_SCAN_JOBS] arrays and the 4^n plan search are where an
// index could run off.  One case per line on stdin:
//   fwd <cu_count> <form> <ws_bytes | -1> <n pairs> {<key> <value>} <njobs> {<H> <B> <T> <Y> <YT>}
//   bwd <cu_count> <form> <n pairs> {<key> <value>} <njobs> {<H> <B> <T>}
// and one line out: kernel grid block lds waves per_cu live xcd_local fused ledger need, then per job cluster fallback cls_begin.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>

#include "../multimodal-gesture-recognition-with-lstms-and-ctc_amd/csrc/scan_choice.h"

int main() {
  std::string dir;
  float* const fake = reinterpret_cast<float*>(0x10000);   // a 16-byte aligned address nobody reads
  long lines = 0;
  while (std::cin >> dir) {
    int cu, form, npairs, njobs, tune[MGR_TUNE_COUNT] = {};
    long long ws = -1;
    std::cin >> cu >> form;
    if (dir == "fwd") std::cin >> ws;
    std::cin >> npairs;
    for (int k = 0; k < npairs; ++k) {
      int key, value;
      std::cin >> key >> value;
      if (key < 0 || key >= MGR_TUNE_COUNT) return 2;
      tune[key] = value;
    }
    std::cin >> njobs;
    if (!std::cin || njobs < 1 || njobs > MGR_MAX_SCAN_JOBS) return 2;
    mgr_scan_choice C;
    if (dir == "fwd") {
      mgr_scan_job jobs[MGR_MAX_SCAN_JOBS];
      memset(jobs, 0, sizeof(jobs));
      for (int i = 0; i < njobs; ++i) {
        int y, yt;
        std::cin >> jobs[i].H >> jobs[i].B >> jobs[i].T >> y >> yt;
        jobs[i].Z = jobs[i].Up = fake;
        jobs[i].Y = y ? fake : nullptr;
        jobs[i].YT = yt ? fake : nullptr;
        jobs[i].ldy = jobs[i].H;
      }
      C = mgr_scan_fwd_decide(cu, tune, njobs, jobs, form, ws < 0 ? (size_t)-1 : (size_t)ws);
    } else {
      mgr_scan_bwd_job jobs[MGR_MAX_SCAN_JOBS];
      memset(jobs, 0, sizeof(jobs));
      for (int i = 0; i < njobs; ++i) {
        std::cin >> jobs[i].H >> jobs[i].B >> jobs[i].T;
        jobs[i].dY = jobs[i].gates = jobs[i].cs = jobs[i].Up = fake;
        jobs[i].dZ = fake;
        jobs[i].lddy = jobs[i].H;
      }
      C = mgr_scan_bwd_decide(cu, tune, njobs, jobs, form);
    }
    if (!std::cin) return 2;
    printf("%d %d %d %d %d %d %d %d %d %d %llu", C.kernel, C.grid, C.block, C.lds_bytes, C.waves, C.per_cu, C.live, C.xcd_local, C.fused, C.ledger,
           C.need);
    for (int i = 0; i < njobs; ++i) printf(" %d %d %d", C.job[i].cluster, C.job[i].fallback, C.job[i].cls_begin);
    printf("\n");
    ++lines;
  }
  return lines > 0 ? 0 : 2;
}
