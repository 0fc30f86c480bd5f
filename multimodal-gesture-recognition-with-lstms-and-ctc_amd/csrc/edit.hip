// K12: scoring decodes on the device.  mgr_edit_distance - weighted edit distance of many short label sequences, with
// the substitution / deletion / insertion split HResults prints and, on request, the alignment itself.
//
// One WAVE per pair.  Both rows are filtered (entries < 0, entries in ignore_mask) into LDS, m hyp labels and n ref labels remain.
// The DP runs over the hyp labels (rows); the n + 1 columns are split over the lanes in contiguous runs of cpl = ceil((n + 1) / 64),
// one row of keys lives in registers.  A cell is the lexicographically smallest tuple (cost, S, D, I), packed into one int64 as
// cost << 36 | S << 24 | D << 12 | I: no field can overflow (S, D <= n, I <= m <= 4095, cost < 2^27), so the lexicographic min is
// an integer min and every step adds a constant (K_sub, K_del, K_ins).
// The registers hold e[j] = d[i][j] - j * K_del.  In that form the in-row dependency d[i][j - 1] + K_del is "e[j - 1]": a row is
//   c[j] = min(e'[j] + K_ins, e'[j - 1] - K_del + (K_sub or 0)),  e[j] = min over k <= j of c[k],
// a prefix minimum: a pass over the lane's own columns, one DPP scan of the lane minima over the wave, a second pass over the lane's
// columns that forms the final keys (and the back-pointers).  No step depends on n.
// Back-pointers: 2 bits per cell - 0 hit, 1 substitution, 2 deletion, 3 insertion, the first of diagonal / deletion / insertion whose
// predecessor plus the step equals the cell - as two bit planes per (row, column-within-lane): the two wave ballots, stored by one
// lane as 16 bytes.  They live in LDS when they fit beside the rows and in the workspace otherwise.  The backtrace from (m, n) is a
// chain of m + n dependent steps at most: every lane runs it with wave-uniform values (scalar instructions, see align.hip), the
// ops land in LDS back to front (their number, n + I, is known from the final key) and leave with one parallel copy.
#include "ctc_lattice.h"

namespace {

typedef long long i64;
constexpr i64 kInf = 0x7fffffffffffffffLL;

// cross-lane traffic through DPP (the control codes and the reasons: ctc_lattice.h), here for 64-bit keys: two v_mov_b32_dpp
template <int CTRL>
__device__ __forceinline__ i64 dpp_i64(i64 v, i64 fill) {   // lanes without a source get fill
  const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)(fill & 0xffffffffLL), (int)(unsigned)(v & 0xffffffffLL), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(fill >> 32), (int)(v >> 32), CTRL, 0xf, 0xf, false);
  return ((i64)hi << 32) | (i64)(unsigned)lo;
}
__device__ __forceinline__ i64 min_i64(i64 a, i64 b) { return a < b ? a : b; }
__device__ __forceinline__ i64 readlane_i64(i64 v, int l) {
  const int lo = __builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffLL), l);
  const int hi = __builtin_amdgcn_readlane((int)(v >> 32), l);
  return ((i64)hi << 32) | (i64)(unsigned)lo;
}
// EXCLUSIVE prefix minimum over the wave (lane 0: kInf): row_shr 1, 2, 4, 8 inside the rows of 16 lanes, the three row totals
// through v_readlane, one wave_shr:1
__device__ __forceinline__ i64 wave_excl_min(i64 x, int lane) {
  x = min_i64(x, dpp_i64<DPP_ROW_SHR1>(x, x));
  x = min_i64(x, dpp_i64<DPP_ROW_SHR2>(x, x));
  x = min_i64(x, dpp_i64<DPP_ROW_SHR4>(x, x));
  x = min_i64(x, dpp_i64<DPP_ROW_SHR8>(x, x));
  const i64 t0 = readlane_i64(x, 15);
  const i64 t1 = min_i64(t0, readlane_i64(x, 31));
  const i64 t2 = min_i64(t1, readlane_i64(x, 47));
  const int row = lane >> 4;
  const i64 pre = row == 0 ? kInf : (row == 1 ? t0 : (row == 2 ? t1 : t2));
  x = min_i64(x, pre);
  return dpp_i64<DPP_WAVE_SHR1>(x, kInf);
}

__host__ __device__ inline int edit_cpl(int n) { return (n + 1 + 63) / 64; }   // columns per lane for n ref labels
// back-pointer bytes of one pair at the widths (Lh rows of cpl(Lr) x 16 bytes)
__host__ __device__ inline size_t edit_bp_bytes(int Lh, int Lr) { return (size_t)Lh * edit_cpl(Lr) * 16; }

// a row -> its surviving labels, in order, in LDS; returns their number (wave-uniform)
__device__ __forceinline__ int edit_filter(const int32_t* __restrict__ row, int len, uint64_t ignore_mask, int* dst, int lane) {
  int cnt = 0;
  for (int base = 0; base < len; base += 64) {
    const int t = base + lane;
    const int v = t < len ? row[t] : -1;
    const bool keep = v >= 0 && !(v < 64 && ((ignore_mask >> v) & 1ull));
    const unsigned long long b = __ballot(keep);
    if (keep) dst[cnt + __popcll(b & ((1ull << lane) - 1ull))] = v;
    cnt += __popcll(b);
  }
  return cnt;
}

template <int CPL>
__global__ __launch_bounds__(64) void k_edit_distance(const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len, int n_hyp, int Lh,
                                                      const int32_t* __restrict__ ref, const int32_t* __restrict__ ref_len, int n_ref, int Lr,
                                                      const int32_t* __restrict__ pair_h, const int32_t* __restrict__ pair_r, int cost_sub,
                                                      int cost_del, int cost_ins, uint64_t ignore_mask, int32_t* __restrict__ dist,
                                                      int32_t* __restrict__ counts, int32_t* __restrict__ lens, int8_t* __restrict__ ops,
                                                      int32_t* __restrict__ n_ops, ulonglong2* bp_g, size_t bp_pair_words, int bp_in_lds) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int p = blockIdx.x, lane = threadIdx.x;
  int* s_h = reinterpret_cast<int*>(smem);
  int* s_r = s_h + Lh;
  // (with ops) the ops of the walk, then the back-pointers when they fit: both 16-byte aligned behind the rows
  const size_t rows16 = ((size_t)(Lh + Lr) * 4 + 15) / 16 * 16;
  int8_t* s_ops = reinterpret_cast<int8_t*>(smem) + rows16;
  ulonglong2* bp = bp_in_lds ? reinterpret_cast<ulonglong2*>(reinterpret_cast<char*>(smem) + rows16 + ((size_t)(Lh + Lr) + 15) / 16 * 16)
                             : bp_g + (size_t)p * bp_pair_words;
  // the indices are device data: clamped, so that whatever they hold the reads stay inside the two arrays
  int ih = pair_h ? pair_h[p] : p, ir = pair_r ? pair_r[p] : p;
  ih = clip_len(ih, n_hyp - 1);
  ir = clip_len(ir, n_ref - 1);
  const int lh = hyp_len ? clip_len(hyp_len[ih], Lh) : Lh;
  const int lr = ref_len ? clip_len(ref_len[ir], Lr) : Lr;
  const int m = edit_filter(hyp + (size_t)ih * Lh, lh, ignore_mask, s_h, lane);
  const int n = edit_filter(ref + (size_t)ir * Lr, lr, ignore_mask, s_r, lane);
  __syncthreads();

  const int cpl = edit_cpl(n);   // <= CPL
  const i64 Ksub = ((i64)cost_sub << 36) | (1LL << 24), Kdel = ((i64)cost_del << 36) | (1LL << 12), Kins = ((i64)cost_ins << 36) | 1LL;
  const bool want = ops != nullptr;
  i64 e[CPL];
  int rl[CPL];   // the ref label of column j (the one a diagonal step into column j consumes: r[j - 1]); none: -2
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int j = lane * cpl + k;
    e[k] = 0;   // row 0: d[0][j] = j * K_del
    rl[k] = (k < cpl && j >= 1 && j <= n) ? s_r[j - 1] : -2;
  }
  for (int i = 1; i <= m; ++i) {
    const int hi = s_h[i - 1];
    // e'[j - 1] of the lane's first column: the previous lane's last column
    i64 last = e[0];
#pragma unroll
    for (int k = 1; k < CPL; ++k)
      if (k < cpl) last = e[k];
    const i64 left0 = dpp_i64<DPP_WAVE_SHR1>(last, kInf);
    // pass 1: the minimum of the lane's own c[j]
    i64 loc = kInf, left = left0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      if (k < cpl) {
        const i64 old = e[k];
        const i64 cd = (lane == 0 && k == 0) ? kInf : left - Kdel + (rl[k] == hi ? 0 : Ksub);
        loc = min_i64(loc, min_i64(cd, old + Kins));
        left = old;
      }
    }
    i64 run = wave_excl_min(loc, lane);   // the final key of the column left of the lane's first one (lane 0: none)
    // pass 2: the final keys, and which step each cell took
    left = left0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      if (k < cpl) {   // (wave-uniform: the ballots below see all 64 lanes)
        const i64 old = e[k];
        const bool eq = rl[k] == hi;
        const i64 cd = (lane == 0 && k == 0) ? kInf : left - Kdel + (eq ? 0 : Ksub);
        const i64 v = min_i64(min_i64(cd, old + Kins), run);
        if (want) {
          const int op = (cd == v) ? (eq ? 0 : 1) : (run == v ? 2 : 3);
          const unsigned long long b0 = __ballot(op & 1), b1 = __ballot(op & 2);
          if (lane == 0) bp[(size_t)(i - 1) * cpl + k] = make_ulonglong2(b0, b1);
        }
        e[k] = v;
        run = v;
        left = old;
      }
    }
  }
  // d[m][n] = e[n] + n * K_del, held by lane n / cpl at k = n % cpl
  const int ln = n / cpl, kn = n - ln * cpl;
  i64 mine = 0;
#pragma unroll
  for (int k = 0; k < CPL; ++k)
    if (k == kn) mine = e[k];
  const i64 d = readlane_i64(mine, __builtin_amdgcn_readfirstlane(ln)) + (i64)n * Kdel;
  const int cost = (int)(d >> 36), S = (int)((d >> 24) & 4095), D = (int)((d >> 12) & 4095), I = (int)(d & 4095);
  if (lane == 0) {
    dist[p] = cost;
    counts[(size_t)p * 4] = n - S - D;
    counts[(size_t)p * 4 + 1] = S;
    counts[(size_t)p * 4 + 2] = D;
    counts[(size_t)p * 4 + 3] = I;
    lens[(size_t)p * 2] = m;
    lens[(size_t)p * 2 + 1] = n;
    if (n_ops) n_ops[p] = n + I;
  }
  if (!want) return;
  __syncthreads();   // the back-pointer words are in place
  {
    int i = m, j = n, lj = ln, kj = kn, pos = n + I - 1;
    while ((i > 0 || j > 0) && pos >= 0) {   // (pos cannot run out with pointers this kernel wrote; keeps the LDS writes in range)
      int op;
      if (i == 0) op = 2;
      else if (j == 0) op = 3;
      else {
        const ulonglong2 w = bp[(size_t)(i - 1) * cpl + kj];
        const unsigned sh = (unsigned)lj & 63u;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)((w.x >> sh) & 1ull));
        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((w.y >> sh) & 1ull));
        op = (int)(lo | (hi << 1));
      }
      if (lane == 0) s_ops[pos] = (int8_t)op;
      --pos;
      if (op != 2) --i;
      if (op != 3) {
        --j;
        if (--kj < 0) {
          kj = cpl - 1;
          --lj;
        }
      }
    }
  }
  __syncthreads();
  const int W = Lh + Lr, no = n + I;
  for (int q = lane; q < W; q += 64) ops[(size_t)p * W + q] = q < no ? s_ops[q] : (int8_t)-1;
}

constexpr size_t kEditLdsMax = 64 * 1024;

}  // namespace

extern "C" {

size_t mgr_edit_distance_ws_bytes(int n_pairs, int Lh, int Lr, int want_ops) {
  if (!want_ops || n_pairs <= 0 || Lh <= 0 || Lr <= 0) return 0;
  return mgr_align_up((size_t)n_pairs * edit_bp_bytes(Lh, Lr), 256);
}

int mgr_edit_distance(mgr_ctx* c, const int32_t* hyp, const int32_t* hyp_len, int n_hyp, int Lh, const int32_t* ref, const int32_t* ref_len,
                      int n_ref, int Lr, const int32_t* pair_h, const int32_t* pair_r, int n_pairs, int cost_sub, int cost_del, int cost_ins,
                      uint64_t ignore_mask, int32_t* dist, int32_t* counts, int32_t* lens, int8_t* ops, int32_t* n_ops, void* ws,
                      size_t ws_bytes) {
  MGR_REQUIRE(c && hyp && ref && dist && counts && lens, "null argument");
  MGR_REQUIRE(n_pairs > 0 && n_hyp > 0 && n_ref > 0 && Lh > 0 && Lr > 0, "bad shape n_pairs=%d n_hyp=%d Lh=%d n_ref=%d Lr=%d", n_pairs, n_hyp,
              Lh, n_ref, Lr);
  MGR_REQUIRE(Lh <= MGR_EDIT_MAX_LEN && Lr <= MGR_EDIT_MAX_LEN, "row width Lh=%d Lr=%d above %d", Lh, Lr, MGR_EDIT_MAX_LEN);
  MGR_REQUIRE(cost_sub >= 1 && cost_sub <= MGR_EDIT_MAX_COST && cost_del >= 1 && cost_del <= MGR_EDIT_MAX_COST && cost_ins >= 1 &&
                  cost_ins <= MGR_EDIT_MAX_COST,
              "costs (%d, %d, %d) out of [1, %d]", cost_sub, cost_del, cost_ins, MGR_EDIT_MAX_COST);
  MGR_REQUIRE((pair_h == nullptr) == (pair_r == nullptr), "pair_h and pair_r must both be given or both be null");
  MGR_REQUIRE(pair_h || (n_hyp == n_pairs && n_ref == n_pairs), "without pair arrays n_hyp = n_ref = n_pairs (%d, %d, %d)", n_hyp, n_ref,
              n_pairs);
  const size_t need = mgr_edit_distance_ws_bytes(n_pairs, Lh, Lr, ops != nullptr);
  MGR_REQUIRE(!ops || (ws && ws_bytes >= need), "workspace too small (%zu bytes, ops need %zu)", ws_bytes, need);
  size_t lds = ((size_t)(Lh + Lr) * 4 + 15) / 16 * 16;
  int in_lds = 0;
  if (ops) {
    lds += ((size_t)(Lh + Lr) + 15) / 16 * 16;
    if (lds + edit_bp_bytes(Lh, Lr) <= kEditLdsMax) {
      in_lds = 1;
      lds += edit_bp_bytes(Lh, Lr);
    } else {
      mgr_planes_forget_range(c, ws, need);   // (this call writes its workspace: kept weight planes in it are gone)
    }
  }
  const int cpl = edit_cpl(Lr);
  ulonglong2* bpg = reinterpret_cast<ulonglong2*>(ws);
  const size_t bpw = edit_bp_bytes(Lh, Lr) / 16;
  hipStream_t s = mgr_stream(c);
  mgr_prof_begin(c, MGR_K_MISC);
#define MGR_EDIT_LAUNCH(N)                                                                                                                  \
  hipLaunchKernelGGL((k_edit_distance<N>), dim3(n_pairs), dim3(64), lds, s, hyp, hyp_len, n_hyp, Lh, ref, ref_len, n_ref, Lr, pair_h, pair_r, \
                     cost_sub, cost_del, cost_ins, ignore_mask, dist, counts, lens, ops, n_ops, bpg, bpw, in_lds)
  if (cpl <= 1) MGR_EDIT_LAUNCH(1);
  else if (cpl <= 2) MGR_EDIT_LAUNCH(2);
  else if (cpl <= 4) MGR_EDIT_LAUNCH(4);
  else if (cpl <= 8) MGR_EDIT_LAUNCH(8);
  else if (cpl <= 16) MGR_EDIT_LAUNCH(16);
  else if (cpl <= 32) MGR_EDIT_LAUNCH(32);
  else MGR_EDIT_LAUNCH(64);
#undef MGR_EDIT_LAUNCH
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}

}  // extern "C"
