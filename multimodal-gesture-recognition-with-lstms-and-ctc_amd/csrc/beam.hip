// K9 / K12: CTC prefix beam search, one body with two entry points.  One wave per sequence, fp64 scores.
//   mgr_ctc_beam_search     (k_beam<KM, false>)  K.ctc_decode(greedy=False, beam_width=W, top_paths=1) semantics; BASELINE.json
//                                                config 5 - not present in the reference
//   mgr_ctc_beam_search_lm  (k_beam<KM, true>)   the same search with a label bigram and an N-best list (not present in
//                                                the reference either); a prefix IS the labelling, as with merge_repeated = 0
//
// Per time step (strictly sequential over t, parallel over the <= W*(C+1) candidates across the 64 lanes):
//   1. log y(c) = log(P+eps) - log(sum_c (P+eps))                               (lanes over classes)
//   2. every live beam r yields a "stay" candidate (blank, or repeat of its last label)        idx r*(C+1)
//      and an "extend by c" candidate for every non-blank c                                      idx r*(C+1)+1+c
//      an extension that reproduces the prefix of another live beam r2 (its trie parent is beam r and its last
//      label is c) is merged into r2's stay candidate instead (stay term first, then the extension)
//   3. the W best candidates by lse(p_blank, p_nonblank) - ties to the smaller idx, -inf dropped - are picked by W
//      rounds of a wave-wide (score, idx) arg-max with lane shuffles; extensions take their trie node (parent, label)
//      from a per-sequence hash table, so that a prefix which fell out of the beam and is found again keeps its node
//      id: "same node" is then exactly "same prefix", which the merge rule of step 2 relies on (a prefix p can die
//      while p+c lives; when p comes back, p+c must still be recognised as its child).
// The winner's prefix is read back through the parent links.  Scores are fp64 because fp32 scores near -5000 have
// an ulp of 5e-4 and the beam cut would then depend on libm rounding; the CPU oracle uses the same formulas.
//
// LM = true adds three things, each behind `if constexpr (LM)`:
//   * every live beam r carries lm_r, the sum of ext over its prefix; a candidate ranks by lse(p_blank, p_nonblank) + lm, where an
//     extension of beam r by c has lm = lm_r + ext[(last_r + 1) * C + c] (row 0: the empty prefix).  An extension whose ext entry is
//     -inf ranks -inf and is dropped like every -inf candidate.  An extension that lands on a live beam merges its network mass into
//     that beam as before: it is the same prefix, hence the same bonus.
//   * after the last frame the live beams are ranked again by total + fin[last + 1] (ties to the better rank before, -inf dropped);
//     fin takes no part in the pruning.
//   * the first top_paths of them are written, each read back through the trie by a lane of its own.
// ext lives in LDS: the kernel is a chain of T dependent steps of one wave, so what counts is the latency of a candidate's lookup
// (an LDS read beside the reads of s_pb / s_tot / s_logy it already does), not bandwidth; a read through the cache would put a
// global-memory round trip on every frame's critical path.  Only the (C + 1) * C doubles in use are staged (dynamic LDS, at most
// 65 * 64 * 8 = 33,280 bytes): the copy costs one pass of at most 65 loads per lane against T frames of work.  The plain
// instantiations take no dynamic LDS and none of the LM arrays.
// With all-zero tables every candidate's rank is its network score + 0.0, i.e. the same double: the search, the sequences and the
// scores of the LM entry point are then those of the plain one bit for bit.
#include "wave_f64.h"

namespace {

constexpr int MAXW = 32;   // beam width limit
constexpr int MAXC = 64;   // classes limit
constexpr int KMAX = 34;   // candidates per lane at the limits: ceil(MAXW*(MAXC+1)/64); the kernel is instantiated for 4 / 12 / 34

// KM = candidate ranks a lane keeps in registers (64 * KM >= W * (C + 1)).  One size for every shape (34) used 256 VGPRs and
// spilled 92 bytes of them to scratch memory - also for the reference's own shape (beam 10, 22 classes: 230 candidates, 4 per lane).
// LM = false reads merge_repeated and writes one path per sequence: out [B][To], out_len [B], logp [B]; ext, fin, NP, score unused.
// LM = true reads ext, fin and writes NP paths per sequence: out [B][NP][To], out_len / score / logp [B][NP]; merge_repeated unused.
// s_ext, s_lm, s_sellm and s_hyp are declared for both forms, since a declaration cannot sit inside an `if constexpr` and be used in
// the next one; every use is behind `if constexpr (LM)`, so the plain instantiations allocate none of them (3584 bytes of LDS, no
// dynamic LDS).  merge_repeated comes last: the arguments before it lie where the bigram form's registers were tuned for.
template <int KM, bool LM>
__global__ __launch_bounds__(64) void k_beam(const float* __restrict__ P, const int32_t* __restrict__ input_len, int T, int C,
                                             int skip, int blank, int W, float eps, const double* __restrict__ ext,
                                             const double* __restrict__ fin, int NP, int32_t* __restrict__ out,
                                             int32_t* __restrict__ out_len, double* __restrict__ score,
                                             double* __restrict__ logp, int32_t* __restrict__ node_parent,
                                             int32_t* __restrict__ node_label, int nodes_per_seq,
                                             unsigned long long* __restrict__ table, int table_bits, int merge_repeated) {
  extern __shared__ double s_ext[];   // LM: [(C+1)*C]
  __shared__ double s_logy[MAXC];
  __shared__ double s_pb[MAXW], s_pnb[MAXW], s_tot[MAXW];
  __shared__ double s_npb[MAXW], s_npnb[MAXW];   // stay candidates (after merging)
  __shared__ int s_node[MAXW], s_pnode[MAXW], s_last[MAXW], s_len[MAXW];
  __shared__ unsigned long long s_mmask[MAXW];   // classes whose extension of beam r was merged into another beam
  __shared__ double s_selb[MAXW], s_selnb[MAXW];
  __shared__ int s_selnode[MAXW], s_selpnode[MAXW], s_sellast[MAXW], s_sellen[MAXW];
  __shared__ double s_lm[MAXW], s_sellm[MAXW];   // LM: the bonus a beam carries
  __shared__ int s_hyp[MAXW];                    // LM: final rank k -> beam, -1 = none
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int To = T - skip;
  int Tp = input_len[b];
  Tp = Tp < 0 ? 0 : (Tp > To ? To : Tp);
  int32_t* par = node_parent + (size_t)b * nodes_per_seq;
  int32_t* lab = node_label + (size_t)b * nodes_per_seq;
  // (parent, label) -> node: open addressing, one 64-bit word per entry = (key + 1) << 32 | node, 0 = empty
  unsigned long long* tab = table + ((size_t)b << table_bits);
  const unsigned tmask = (1u << table_bits) - 1u;
  for (unsigned i = lane; i <= tmask; i += 64) tab[i] = 0ull;
  if constexpr (LM)
    for (int i = lane; i < (C + 1) * C; i += 64) s_ext[i] = ext[i];
  __threadfence();
  int nb = 1;          // live beams
  int nnodes = 1;      // node 0 = empty prefix
  if (lane == 0) {
    par[0] = -1;
    lab[0] = -1;
    s_pb[0] = 0.0;
    s_pnb[0] = kNegInfD;
    if constexpr (LM) s_lm[0] = 0.0;
    s_node[0] = 0;
    s_pnode[0] = -1;
    s_last[0] = -1;
    s_len[0] = 0;
  }
  __syncthreads();
  const int CP1 = C + 1;
  for (int t = 0; t < Tp; ++t) {
    // ---- 1. frame log-probabilities
    const float* row = P + ((size_t)b * T + skip + t) * C;
    double u = (lane < C) ? (double)row[lane] + (double)eps : 0.0;
    double s = u;
    for (int o = 32; o > 0; o >>= 1) s += shfl_xor_d(s, o);
    if (lane < C) s_logy[lane] = log(u) - log(s);
    __syncthreads();
    // ---- 2a. stay candidates
    if (lane < nb) {
      double pb = s_pb[lane], pnb = s_pnb[lane];
      double tot = lse64(pb, pnb);
      s_tot[lane] = tot;
      s_npb[lane] = tot + s_logy[blank];
      s_npnb[lane] = (s_len[lane] > 0) ? pnb + s_logy[s_last[lane]] : kNegInfD;
      s_mmask[lane] = 0ull;
    }
    __syncthreads();
    // ---- 2b. merge extensions that land on a live beam (lane = r2; at most one (r, c) per r2)
    if (lane < nb && s_len[lane] > 0) {
      int pnode = s_pnode[lane];
      int c = s_last[lane];
      for (int r = 0; r < nb; ++r) {
        if (s_node[r] == pnode) {
          double val = ((s_len[r] > 0 && c == s_last[r]) ? s_pb[r] : s_tot[r]) + s_logy[c];
          s_npnb[lane] = lse64(s_npnb[lane], val);
          atomicOr(&s_mmask[r], 1ull << c);
          break;
        }
      }
    }
    __syncthreads();
    // ---- 3. candidate ranks (this lane's slice) and W rounds of arg-max
    double cs[KM];
    const int ncand = nb * CP1;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      int idx = lane + 64 * k;
      double sc = kNegInfD;
      if (idx < ncand) {
        int r = idx / CP1, slot = idx - r * CP1;
        if (slot == 0) {
          if constexpr (LM)
            sc = lse64(s_npb[r], s_npnb[r]) + s_lm[r];
          else
            sc = lse64(s_npb[r], s_npnb[r]);
        } else {
          int c = slot - 1;
          if (c != blank && !((s_mmask[r] >> c) & 1ull)) {
            if constexpr (LM)
              sc = (((s_len[r] > 0 && c == s_last[r]) ? s_pb[r] : s_tot[r]) + s_logy[c]) + (s_lm[r] + s_ext[(s_last[r] + 1) * C + c]);
            else
              sc = ((s_len[r] > 0 && c == s_last[r]) ? s_pb[r] : s_tot[r]) + s_logy[c];
          }
        }
      }
      cs[k] = sc;
    }
    int nsel = 0;
    const int kused = (ncand + 63) / 64;
    for (int w = 0; w < W; ++w) {
      double best = kNegInfD;
      int bidx = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < KM; ++k) {
        if (k < kused) {
          int idx = lane + 64 * k;
          if (cs[k] > best || (cs[k] == best && cs[k] != kNegInfD && idx < bidx)) {
            best = cs[k];
            bidx = idx;
          }
        }
      }
      for (int o = 32; o > 0; o >>= 1) {
        const ScoreIdx q = wave_argmax_step_d(best, bidx, o);
        best = q.v;
        bidx = q.i;
      }
      if (best == kNegInfD) break;  // wave-uniform
      // the owning lane retires the candidate
#pragma unroll
      for (int k = 0; k < KM; ++k)
        if (lane + 64 * k == bidx) cs[k] = kNegInfD;
      if (lane == 0) {
        int r = bidx / CP1, slot = bidx - r * CP1;
        if (slot == 0) {
          s_selb[nsel] = s_npb[r];
          s_selnb[nsel] = s_npnb[r];
          if constexpr (LM) s_sellm[nsel] = s_lm[r];
          s_selnode[nsel] = s_node[r];
          s_selpnode[nsel] = s_pnode[r];
          s_sellast[nsel] = s_last[r];
          s_sellen[nsel] = s_len[r];
        } else {
          int c = slot - 1;
          s_selb[nsel] = kNegInfD;
          s_selnb[nsel] = ((s_len[r] > 0 && c == s_last[r]) ? s_pb[r] : s_tot[r]) + s_logy[c];
          if constexpr (LM) s_sellm[nsel] = s_lm[r] + s_ext[(s_last[r] + 1) * C + c];
          s_selnode[nsel] = -1;  // resolved below, all selections in parallel
          s_selpnode[nsel] = s_node[r];
          s_sellast[nsel] = c;
          s_sellen[nsel] = s_len[r] + 1;
        }
      }
      ++nsel;
    }
    __syncthreads();
    if (lane < nsel) {
      int node = s_selnode[lane];
      if (node < 0) {
        // find-or-insert (parent, label); the selected extensions are distinct prefixes, hence distinct keys
        const int pn = s_selpnode[lane], c = s_sellast[lane];
        const unsigned key = (unsigned)pn * 64u + (unsigned)c + 1u;
        const int fresh = nnodes + lane;  // only used if the prefix is new; gaps in the pool are harmless
        unsigned h = (key * 0x9E3779B1u) >> (32 - table_bits);
        for (;;) {
          unsigned long long e = __hip_atomic_load(tab + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (e == 0ull) {
            unsigned long long mine = ((unsigned long long)key << 32) | (unsigned)fresh;
            if (atomicCAS(tab + h, 0ull, mine) == 0ull) {
              par[fresh] = pn;
              lab[fresh] = c;
              node = fresh;
              break;
            }
            continue;  // another lane took the slot: look at it again
          }
          if ((unsigned)(e >> 32) == key) {
            node = (int)(unsigned)e;
            break;
          }
          h = (h + 1u) & tmask;
        }
      }
      s_pb[lane] = s_selb[lane];
      s_pnb[lane] = s_selnb[lane];
      if constexpr (LM) s_lm[lane] = s_sellm[lane];
      s_node[lane] = node;
      s_pnode[lane] = s_selpnode[lane];
      s_last[lane] = s_sellast[lane];
      s_len[lane] = s_sellen[lane];
    }
    nb = nsel;
    nnodes += W;
    __syncthreads();
  }
  __threadfence();
  if constexpr (!LM) {
    // ---- read the winner back
    if (lane == 0) {
      int32_t* o = out + (size_t)b * To;
      int n = 0;
      if (nb > 0) {
        int len = s_len[0];
        int node = s_node[0];
        // write reversed into the tail, then compact forward
        for (int i = len - 1; i >= 0; --i) {  // (nodes were written by other lanes: read them past the L1)
          o[i] = __hip_atomic_load(lab + node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          node = __hip_atomic_load(par + node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (merge_repeated) {
          for (int i = 0; i < len; ++i)
            if (i == 0 || o[i] != o[i - 1]) o[n++] = o[i];
        } else {
          n = len;
        }
        logp[b] = lse64(s_pb[0], s_pnb[0]);
      } else {
        logp[b] = kNegInfD;
      }
      for (int i = n; i < To; ++i) o[i] = -1;
      out_len[b] = n;
    }
  } else {
    // ---- final ranking: total + fin[last + 1], ties to the better rank before, -inf dropped
    double net = kNegInfD, f = kNegInfD;
    if (lane < nb) {
      net = lse64(s_pb[lane], s_pnb[lane]);
      f = net + s_lm[lane];
      if (fin) f = f + fin[s_last[lane] + 1];
      s_npb[lane] = f;
    }
    if (lane < MAXW) s_hyp[lane] = -1;
    __syncthreads();
    if (lane < nb && f != kNegInfD) {
      int k = 0;
      for (int r = 0; r < nb; ++r) {
        double g = s_npb[r];
        k += (g > f || (g == f && r < lane)) ? 1 : 0;
      }
      s_hyp[k] = lane;   // (the beams with a finite score take the ranks 0 .. their count - 1, each exactly one)
    }
    __syncthreads();
    // ---- the first NP of them: the padding by all lanes, hypothesis k's labels by lane k through the parent links
    for (int k = 0; k < NP; ++k) {
      const int r = s_hyp[k];
      const int len = r >= 0 ? s_len[r] : 0;
      int32_t* o = out + ((size_t)b * NP + k) * To;
      for (int i = len + lane; i < To; i += 64) o[i] = -1;
    }
    if (lane < NP) {
      const int r = s_hyp[lane];
      const size_t slot = (size_t)b * NP + lane;
      if (r >= 0) {
        int32_t* o = out + slot * To;
        int node = s_node[r];
        for (int i = s_len[r] - 1; i >= 0; --i) {  // (nodes were written by other lanes: read them past the L1)
          o[i] = __hip_atomic_load(lab + node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          node = __hip_atomic_load(par + node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        out_len[slot] = s_len[r];
        score[slot] = s_npb[r];
        logp[slot] = lse64(s_pb[r], s_pnb[r]);
      } else {
        out_len[slot] = -1;
        score[slot] = kNegInfD;
        logp[slot] = kNegInfD;
      }
    }
  }
}

// the argument checks of both entry points (the plain one has top_paths = 1)
int beam_check(mgr_ctx* c, int B, int T, int C, int skip, int blank, int beam, int top_paths, void* ws, size_t ws_bytes) {
  mgr_planes_forget_range(c, ws, ws_bytes);   // (this call writes its workspace: kept weight planes in it are gone)
  MGR_REQUIRE(B > 0 && T > skip && skip >= 0 && C > 1 && C <= MAXC, "bad shape (C <= %d)", MAXC);
  MGR_REQUIRE(beam >= 1 && beam <= MAXW, "beam width %d out of [1,%d]", beam, MAXW);
  MGR_REQUIRE(top_paths >= 1 && top_paths <= beam, "top_paths %d out of [1, beam = %d]", top_paths, beam);
  MGR_REQUIRE(beam * (C + 1) <= 64 * KMAX, "beam*(C+1) too large");
  MGR_REQUIRE(blank >= 0 && blank < C, "blank out of range");
  MGR_REQUIRE(ws && ws_bytes >= mgr_ctc_beam_ws_bytes(B, T, C, beam), "workspace too small");
  MGR_REQUIRE((size_t)(T * beam + 2) < ((size_t)1 << 25), "T*beam too large for the prefix table");
  return 0;
}

// carves the workspace, picks KM by the candidates per lane and launches
template <bool LM>
int beam_launch(mgr_ctx* c, const float* P, const int32_t* input_len, int B, int T, int C, int skip, int blank, int beam, float eps,
                int merge_repeated, const double* ext, const double* fin, int top_paths, int32_t* out, int32_t* out_len,
                double* score, double* logp, void* ws) {
  const int nodes = T * beam + 2;
  const mgr_beam_ws L = mgr_beam_ws_layout(ws, B, (size_t)nodes);
  const size_t lds = LM ? (size_t)(C + 1) * C * sizeof(double) : 0;
  mgr_prof_begin(c, MGR_K_MISC);
  const int per_lane = (beam * (C + 1) + 63) / 64;
#define MGR_BEAM_LAUNCH(KM)                                                                                                    \
  hipLaunchKernelGGL((k_beam<KM, LM>), dim3(B), dim3(64), lds, mgr_stream(c), P, input_len, T, C, skip, blank, beam, eps, ext,  \
                     fin, top_paths, out, out_len, score, logp, L.parent, L.label, nodes, L.table, L.bits, merge_repeated)
  if (per_lane <= 4)
    MGR_BEAM_LAUNCH(4);
  else if (per_lane <= 12)
    MGR_BEAM_LAUNCH(12);
  else
    MGR_BEAM_LAUNCH(KMAX);
#undef MGR_BEAM_LAUNCH
  MGR_LAUNCH_CHECK();
  mgr_prof_end(c, MGR_K_MISC);
  return 0;
}

}  // namespace

extern "C" {

size_t mgr_ctc_beam_ws_bytes(int B, int T, int C, int beam) {
  (void)C;
  return mgr_beam_ws_layout(nullptr, B, (size_t)T * (beam > 0 ? beam : 1) + 2).bytes;
}

size_t mgr_ctc_beam_lm_ws_bytes(int B, int T, int C, int beam, int top_paths) {
  (void)top_paths;   // (the hypotheses are read out of the trie the search keeps anyway)
  return mgr_ctc_beam_ws_bytes(B, T, C, beam);
}

int mgr_ctc_beam_search(mgr_ctx* c, const float* P, const int32_t* input_len, int B, int T, int C, int skip, int blank,
                        int beam, float eps, int merge_repeated, int32_t* out, int32_t* out_len, double* logp, void* ws,
                        size_t ws_bytes) {
  MGR_REQUIRE(c && P && input_len && out && out_len && logp, "null argument");
  if (int e = beam_check(c, B, T, C, skip, blank, beam, 1, ws, ws_bytes)) return e;
  return beam_launch<false>(c, P, input_len, B, T, C, skip, blank, beam, eps, merge_repeated, nullptr, nullptr, 1, out, out_len,
                            nullptr, logp, ws);
}

int mgr_ctc_beam_search_lm(mgr_ctx* c, const float* P, const int32_t* input_len, int B, int T, int C, int skip, int blank, int beam,
                           float eps, const double* ext, const double* fin, int top_paths, int32_t* out, int32_t* out_len,
                           double* score, double* logp_ctc, void* ws, size_t ws_bytes) {
  MGR_REQUIRE(c && P && input_len && ext && out && out_len && score && logp_ctc, "null argument");
  if (int e = beam_check(c, B, T, C, skip, blank, beam, top_paths, ws, ws_bytes)) return e;
  return beam_launch<true>(c, P, input_len, B, T, C, skip, blank, beam, eps, 0, ext, fin, top_paths, out, out_len, score, logp_ctc,
                           ws);
}

}  // extern "C"
