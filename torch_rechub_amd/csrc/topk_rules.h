// The rules (see the head of topk_list.h) and the kernel arguments of the flat scan (topk.hip) and the list scan (ivf.hip),
// and how a list-scan workgroup finds its tile.  None of this knows the table's type: topk_half.hip runs the same rules
// under the half scan body of topk_half_tile.h.
#pragma once

#include "topk_list.h"

constexpr int kIvfMaxProbe = RH_IVF_MAX_NPROBE;

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

// the flat scan's workgroup: RB rows from blockIdx.x, the column range blockIdx.y of s.nlist
static __device__ __forceinline__ FlatRule topk_flat_rule(const TopkArgs& a, int64_t& lo, int64_t& hi) {
  const TopkScanArgs& s = a.s;
  const int split = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * s.RB;
  lo = (int64_t)s.V * split / s.nlist;
  hi = (int64_t)s.V * (split + 1) / s.nlist;
  return FlatRule{r0, (int)(s.M - r0 < s.RB ? s.M - r0 : s.RB), s.nlist, split, s.K, a.invalid, a.n_inv};
}

struct IvfArgs {
  TopkScanArgs s;           // x, bias = the rows grouped by list; exclude = original ids; nlist = nprobe
  const int32_t* row_id;    // (V,) original ids
  const int32_t* list_off;  // (nlists + 1,)
  const int32_t* pair;      // (M nprobe,) pair indices grouped by list
  const int32_t* pair_off;  // (nlists + 2,)
  const int32_t* tile_off;  // (nlists + 2,)
  int nlists;
};

// tile row r holds the pair prs[r] = query nprobe + slot (-1: no row), whose list in the partials is the pair's; the id
// of a grouped row is row_id's
struct IvfRule {
  const int* prs;  // [64] in LDS
  const int32_t* row_id;
  int nprobe, K;
  static constexpr const int64_t* invalid = nullptr;
  static constexpr int n_inv = 0;
  __device__ __forceinline__ bool has_row(int r) const { return prs[r] >= 0; }
  __device__ __forceinline__ int64_t query_row(int r) const { return prs[r] / nprobe; }
  __device__ __forceinline__ int64_t id_of(int64_t c) const { return row_id[c]; }
  __device__ __forceinline__ int64_t list_offset(int r) const { return (int64_t)prs[r] * K; }
};

// The tile of list-scan workgroup blockIdx.x: its pairs' indices into prs[64] (LDS; -1 = no row), its list's rows
// [lo, hi) (none for group 0).  false: the workgroup is past tile_off's end and leaves.  Ends in a barrier.
static __device__ __forceinline__ bool ivf_tile(const IvfArgs& a, int* prs, int64_t& lo, int64_t& hi) {
  const TopkScanArgs& s = a.s;
  const int tid = threadIdx.x, RB = s.RB;
  const int b = blockIdx.x;
  if (b >= a.tile_off[a.nlists + 1]) return false;
  int g = 0;  // the last group with tile_off[g] <= b: tile_off[g + 1] > b, so the group has the tile
  for (int hi_g = a.nlists; g < hi_g;) {
    const int mid = (g + hi_g + 1) / 2;
    if (a.tile_off[mid] <= b) g = mid; else hi_g = mid - 1;
  }
  const int64_t p0 = (int64_t)a.pair_off[g] + (int64_t)(b - a.tile_off[g]) * RB, p1 = a.pair_off[g + 1];
  const int64_t npair = (int64_t)s.M * s.nlist;
  lo = 0, hi = 0;  // group 0: no list
  if (g > 0) {
    lo = a.list_off[g - 1];
    hi = a.list_off[g];
    if (lo < 0) lo = 0;
    if (hi > s.V) hi = s.V;
  }
  if (tid < kT) {
    int p = -1;
    if (tid < RB && p0 >= 0 && p0 + tid < p1 && p0 + tid < npair) {
      p = a.pair[p0 + tid];
      if (p < 0 || p >= npair) p = -1;
    }
    prs[tid] = p;
  }
  __syncthreads();
  return true;
}

inline bool ivf_shape_ok(int D, int K, int S, int nprobe) {
  return topk_shape_ok(D, K, S) && nprobe >= 1 && nprobe <= kIvfMaxProbe;
}

// Everything of a flat-scan entry point (`who`) up to the launch, whatever the table's type: the limits, the sizes, the
// pointers, the arguments.  *go = there is something to launch (M > 0).
inline int topk_flat_args(const char* who, TopkArgs* a, bool* go, const float* q, int64_t ldq, const void* x,
                          const float* bias, const int64_t* exclude, int S, const int64_t* invalid, int n_inv, int M, int D,
                          int V, int K, int nsplit, void* workspace, int64_t* ids, float* scores) {
  *go = false;
  RH_REQUIRE(topk_shape_ok(D, K, S), RH_E_UNSUPPORTED,
             "%s: D=%d K=%d S=%d unsupported (1 <= D <= %d, 1 <= K <= %d, 0 <= S <= %d)", who, D, K, S, kTopkMaxD,
             kTopkMaxK, kTopkMaxS);
  if (int rc = topk_scan_sizes(who, M, V, "n_inv", n_inv, n_inv >= 0, ldq, D)) return rc;
  RH_REQUIRE(nsplit >= 1 && nsplit <= kTopkMaxSplit && nsplit <= V, RH_E_BADARG, "%s: nsplit=%d outside [1, min(V, %d)]",
             who, nsplit, kTopkMaxSplit);
  if (M == 0) return 0;
  if (int rc = topk_scan_args(who, &a->s, q, ldq, x, bias, exclude, S, M, D, V, K, nsplit, workspace, ids, scores))
    return rc;
  RH_REQUIRE(n_inv == 0 || invalid, RH_E_BADARG, "%s: null pointer", who);
  a->invalid = invalid;
  a->n_inv = n_inv;
  *go = true;
  return 0;
}

// The same for a list-scan entry point; *grid = its fixed grid bound.
inline int ivf_scan_args(const char* who, IvfArgs* a, bool* go, int64_t* grid, const float* q, int64_t ldq, const void* xs,
                         const float* bias_s, const int32_t* row_id, const int32_t* list_off, int nlists,
                         const int32_t* pair, const int32_t* pair_off, const int32_t* tile_off, const int64_t* exclude,
                         int S, int M, int D, int V, int K, int nprobe, void* partials, int64_t* ids, float* scores) {
  *go = false;
  RH_REQUIRE(ivf_shape_ok(D, K, S, nprobe), RH_E_UNSUPPORTED,
             "%s: D=%d K=%d S=%d nprobe=%d unsupported (1 <= D <= %d, 1 <= K <= %d, 0 <= S <= %d, 1 <= nprobe <= %d)", who,
             D, K, S, nprobe, kTopkMaxD, kTopkMaxK, kTopkMaxS, kIvfMaxProbe);
  if (int rc = topk_scan_sizes(who, M, V, "nlists", nlists, nlists >= 1, ldq, D)) return rc;
  const int RB = topk_rows(K);
  const int64_t npair = (int64_t)M * nprobe;
  *grid = (npair + RB - 1) / RB + nlists + 1;
  RH_REQUIRE(*grid < ((int64_t)1 << 31), RH_E_UNSUPPORTED, "%s: M nprobe = %lld pairs are too many", who, (long long)npair);
  if (M == 0) return 0;
  if (int rc = topk_scan_args(who, &a->s, q, ldq, xs, bias_s, exclude, S, M, D, V, K, nprobe, partials, ids, scores)) return rc;
  RH_REQUIRE(row_id && list_off && pair && pair_off && tile_off, RH_E_BADARG, "%s: null pointer", who);
  a->row_id = row_id;
  a->list_off = list_off;
  a->pair = pair;
  a->pair_off = pair_off;
  a->tile_off = tile_off;
  a->nlists = nlists;
  *go = true;
  return 0;
}
