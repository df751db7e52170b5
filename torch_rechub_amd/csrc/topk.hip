// Streaming exact top-K of score[i][j] = q_i . x_j (+ bias[j]) over an item table, without the (M, V) score matrix
// (rh_topk_*; replaces Annoy / torch.topk at the end of the reference's matching, session and generative examples).
//
// Scan kernel: a workgroup owns RB query rows (64 at K <= 128, 32 above: the K-lists of its rows fill at most 64 KiB of
// LDS) and one of nsplit contiguous column ranges [V s / nsplit, V (s + 1) / nsplit), which it walks in tiles of 64
// columns.  The 64 x 64 score tile comes from the shared MFMA tile of mfma_tile.h (exact f32 products, k-ordered
// accumulation from zero, bias added once at the end), so one score depends on q_i, x_j and D alone.  Per row the
// workgroup keeps the K best (score, id) so far in LDS, sorted by (score descending, id ascending); the K-th score is the
// row's threshold.  After each tile the wavefront that owns a row ballots the 64 scores against the threshold; only the
// hits are looked up in the row's exclude list and the invalid list (global memory, scanned by the wavefront) and
// inserted cooperatively.  Columns arrive in ascending id, so a candidate enters behind every entry of equal score and
// an equal score never displaces the K-th: the list is the range's top K under the total order.
// Merge kernel: one wavefront per row merges the nsplit sorted lists under the same total order.  Every range's top K
// under a total order holds the global top K's members of that range, so the result does not depend on nsplit.
// No atomics; every element of the partials is written (unused tail: -inf, -1).
// The scan of one workgroup (topk_scan_tiles), its K-list (threshold, ballot, cooperative insert) and the merge of one row
// live in topk_list.h, shared with ivf.hip: topk_scan_kernel only names its column range and, in FlatRule, its rows
// (topk_rules.h, which topk_half.hip runs under the half-table scan body).
#include "topk_rules.h"

namespace {

__global__ __launch_bounds__(RH_BLOCK) void topk_scan_kernel(const TopkArgs a) {
  extern __shared__ __align__(16) float lds[];
  int64_t lo, hi;
  const FlatRule rule = topk_flat_rule(a, lo, hi);
  topk_scan_tiles(a.s, rule, lo, hi, lds);
}

}  // namespace

extern "C" int rh_topk_supported(int D, int K, int S, int* supported) {
  RH_REQUIRE(supported != nullptr, RH_E_BADARG, "rh_topk_supported: null pointer");
  *supported = topk_shape_ok(D, K, S) ? 1 : 0;
  return 0;
}

extern "C" int rh_topk_plan(int M, int V, int K, int* nsplit, int64_t* workspace_bytes) {
  RH_REQUIRE(nsplit != nullptr && workspace_bytes != nullptr, RH_E_BADARG, "rh_topk_plan: null pointer");
  RH_REQUIRE(M >= 0 && V >= 1, RH_E_BADARG, "rh_topk_plan: M=%d V=%d (M >= 0, V >= 1)", M, V);
  RH_REQUIRE(K >= 1 && K <= kTopkMaxK, RH_E_UNSUPPORTED, "rh_topk_plan: K=%d unsupported (1 <= K <= %d)", K, kTopkMaxK);
  *nsplit = topk_default_split(M, V, topk_rows(K));
  *workspace_bytes = (int64_t)M * *nsplit * K * 8;
  return 0;
}

extern "C" int rh_topk_fwd(const float* q, int64_t ldq, const float* x, const float* bias, const int64_t* exclude, int S,
                           const int64_t* invalid, int n_inv, int M, int D, int V, int K, int nsplit, void* workspace,
                           int64_t* ids, float* scores, void* stream) {
  TopkArgs a{};
  bool go;
  if (int rc = topk_flat_args("rh_topk_fwd", &a, &go, q, ldq, x, bias, exclude, S, invalid, n_inv, M, D, V, K, nsplit,
                              workspace, ids, scores))
    return rc;
  if (!go) return 0;
  static RhLdsReserved reserved;
  if (int rc = rh_reserve_lds(reserved, topk_scan_kernel, topk_lds_bytes(128), "rh_topk_fwd")) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t nrt = ((int64_t)M + a.s.RB - 1) / a.s.RB;
  hipLaunchKernelGGL(topk_scan_kernel, dim3((unsigned)nrt, nsplit), dim3(RH_BLOCK), topk_lds_bytes(K), st, a);
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)M), dim3(RH_WAVE), 0, st, a.s);
  RH_LAUNCH_CHECK("rh_topk_fwd");
  return 0;
}
