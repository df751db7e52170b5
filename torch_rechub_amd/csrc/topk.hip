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
// live in topk_list.h, shared with ivf.hip: topk_scan_kernel only names its column range and, in FlatRule, its rows.
#include "topk_list.h"

namespace {

struct TopkArgs {
  TopkScanArgs s;          // nlist = nsplit
  const int64_t* invalid;  // (n_inv,) or null
  int n_inv;
};

// tile row r is query row r0 + r where r < rows, a column's id is its index, range `split` is the query's list `split`
struct FlatRule {
  int64_t r0;
  int rows, nsplit, split, K;
  const int64_t* invalid;
  int n_inv;
  __device__ __forceinline__ bool has_row(int r) const { return r < rows; }
  __device__ __forceinline__ int64_t query_row(int r) const { return r0 + r; }
  __device__ __forceinline__ int64_t id_of(int64_t c) const { return c; }
  __device__ __forceinline__ int64_t list_offset(int r) const { return ((r0 + r) * nsplit + split) * K; }
};

__global__ __launch_bounds__(RH_BLOCK) void topk_scan_kernel(const TopkArgs a) {
  extern __shared__ __align__(16) float lds[];
  const TopkScanArgs& s = a.s;
  const int split = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * s.RB;
  const FlatRule rule{r0, (int)(s.M - r0 < s.RB ? s.M - r0 : s.RB), s.nlist, split, s.K, a.invalid, a.n_inv};
  topk_scan_tiles(s, rule, (int64_t)s.V * split / s.nlist, (int64_t)s.V * (split + 1) / s.nlist, lds);
}

// one wavefront per row
__global__ __launch_bounds__(RH_WAVE) void topk_merge_kernel(const TopkArgs a) {
  __shared__ int hp[kTopkMaxSplit];
  const int64_t row = blockIdx.x;
  const TopkScanArgs& s = a.s;
  topk_merge_row(s.part_s + row * s.nlist * s.K, s.part_i + row * s.nlist * s.K, s.nlist, s.K, s.ids + row * s.K,
                 s.scores + row * s.K, hp, threadIdx.x);
}

// default ranges: enough workgroups for one round over the chip's 256 compute units, ranges of at least 4096 columns (the
// lists of a range cost about K (1 + ln(range / K)) insertions per row whatever its length, so short ranges only add work)
int topk_default_split(int M, int V, int K) {
  const int64_t nrt = ((int64_t)M + topk_rows(K) - 1) / topk_rows(K);
  int64_t s = nrt > 0 ? (256 + nrt - 1) / nrt : 1;
  const int64_t cap = V / 4096;
  if (s > cap) s = cap;
  if (s > kTopkMaxSplit) s = kTopkMaxSplit;
  if (s < 1) s = 1;
  return (int)s;
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
  *nsplit = topk_default_split(M, V, K);
  *workspace_bytes = (int64_t)M * *nsplit * K * 8;
  return 0;
}

extern "C" int rh_topk_fwd(const float* q, int64_t ldq, const float* x, const float* bias, const int64_t* exclude, int S,
                           const int64_t* invalid, int n_inv, int M, int D, int V, int K, int nsplit, void* workspace,
                           int64_t* ids, float* scores, void* stream) {
  RH_REQUIRE(topk_shape_ok(D, K, S), RH_E_UNSUPPORTED,
             "rh_topk_fwd: D=%d K=%d S=%d unsupported (1 <= D <= %d, 1 <= K <= %d, 0 <= S <= %d)", D, K, S, kTopkMaxD,
             kTopkMaxK, kTopkMaxS);
  if (int rc = topk_scan_sizes("rh_topk_fwd", M, V, "n_inv", n_inv, n_inv >= 0, ldq, D)) return rc;
  RH_REQUIRE(nsplit >= 1 && nsplit <= kTopkMaxSplit && nsplit <= V, RH_E_BADARG,
             "rh_topk_fwd: nsplit=%d outside [1, min(V, %d)]", nsplit, kTopkMaxSplit);
  if (M == 0) return 0;
  TopkArgs a{};
  if (int rc = topk_scan_args("rh_topk_fwd", &a.s, q, ldq, x, bias, exclude, S, M, D, V, K, nsplit, workspace, ids, scores))
    return rc;
  RH_REQUIRE(n_inv == 0 || invalid, RH_E_BADARG, "rh_topk_fwd: null pointer");
  a.invalid = invalid;
  a.n_inv = n_inv;
  static RhLdsReserved reserved;
  if (int rc = rh_reserve_lds(reserved, topk_scan_kernel, topk_lds_bytes(128), "rh_topk_fwd")) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t nrt = ((int64_t)M + a.s.RB - 1) / a.s.RB;
  hipLaunchKernelGGL(topk_scan_kernel, dim3((unsigned)nrt, nsplit), dim3(RH_BLOCK), topk_lds_bytes(K), st, a);
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)M), dim3(RH_WAVE), 0, st, a);
  RH_LAUNCH_CHECK("rh_topk_fwd");
  return 0;
}
