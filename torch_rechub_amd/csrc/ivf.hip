// Inverted-file index on the flat scan's tile (rh_ivf_*; replaces faiss's IVF{nlists},Flat index with nprobe of the
// reference's serving/faiss.py).  The table's rows are grouped by list (xs, bias_s, row_id = the original ids, ascending
// inside a list; list_off = the lists' offsets); query i probes the lists probe[i][0 .. nprobe) (-1 = none).
//
// Scan kernel, list-centric: the M nprobe (query, slot) pairs arrive grouped by list (pair = the pair indices
// i nprobe + slot in list order, group 0 = the pairs with no list, group l + 1 = list l; pair_off = the groups' offsets;
// tile_off = the prefix sum of ceil(group size / RB)).  The grid is the fixed upper bound of the tile count; a workgroup
// finds its (group, tile of RB pairs) by binary search in tile_off and leaves if there is none.  It puts its pairs'
// indices into LDS and hands its list's rows to topk_scan_tiles of topk_list.h, the one scan body that topk_scan_kernel
// runs over a column range (the score tile of mfma_tile.h: one score depends on q_i, x_j and D alone; the K-lists),
// under IvfRule: tile row r is the query of pair r, row_id[c] is the id of column c, the list goes to the pair's place
// in the partials.  Ids ascend inside a list, so the list is the top K of the probed list under (score
// descending, id ascending).  Every pair belongs to exactly one tile, which writes the pair's list to the partials at
// (query, slot) (unused tail: -inf, -1) -- also where the list is empty or absent: every element the merge reads is
// written.  Merge kernel: topk_merge_row with one list per slot.  The union of the probed lists' top K holds the top K
// of the union, so with every list probed the result is rh_topk_fwd's, bit for bit.  No atomics.
//
// List mean (the update step of k-means): one workgroup per list; wavefront w adds the rows w, w + 4, ... of the list in
// order, the four partial sums are added as (0 + 1) + (2 + 3) and divided by the count.  An empty list keeps `previous`.
#include "topk_list.h"

namespace {

constexpr int kIvfMaxProbe = RH_IVF_MAX_NPROBE;

struct IvfArgs {
  TopkScanArgs s;           // x, bias = the rows grouped by list; exclude = original ids; nlist = nprobe
  const int32_t* row_id;    // (V,) original ids
  const int32_t* list_off;  // (nlists + 1,)
  const int32_t* pair;      // (M nprobe,) pair indices grouped by list
  const int32_t* pair_off;  // (nlists + 2,)
  const int32_t* tile_off;  // (nlists + 2,)
  int nlists;
};

size_t ivf_lds_bytes(int K) { return topk_lds_bytes(K) + (size_t)kT * 4; }

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

__global__ __launch_bounds__(RH_BLOCK) void ivf_scan_kernel(const IvfArgs a) {
  extern __shared__ __align__(16) float lds[];
  const TopkScanArgs& s = a.s;
  int* prs = reinterpret_cast<int*>(lds + topk_lds_bytes(s.K) / sizeof(float));  // [64] pair index of the row, -1 = no row
  const int tid = threadIdx.x, RB = s.RB;
  const int b = blockIdx.x;
  if (b >= a.tile_off[a.nlists + 1]) return;
  int g = 0;  // the last group with tile_off[g] <= b: tile_off[g + 1] > b, so the group has the tile
  for (int hi_g = a.nlists; g < hi_g;) {
    const int mid = (g + hi_g + 1) / 2;
    if (a.tile_off[mid] <= b) g = mid; else hi_g = mid - 1;
  }
  const int64_t p0 = (int64_t)a.pair_off[g] + (int64_t)(b - a.tile_off[g]) * RB, p1 = a.pair_off[g + 1];
  const int64_t npair = (int64_t)s.M * s.nlist;
  int64_t lo = 0, hi = 0;  // group 0: no list
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
  topk_scan_tiles(s, IvfRule{prs, a.row_id, s.nlist, s.K}, lo, hi, lds);
}

// one wavefront per query: one list per slot
__global__ __launch_bounds__(RH_WAVE) void ivf_merge_kernel(const IvfArgs a) {
  __shared__ int hp[kIvfMaxProbe];
  const int64_t row = blockIdx.x;
  const TopkScanArgs& s = a.s;
  topk_merge_row(s.part_s + row * s.nlist * s.K, s.part_i + row * s.nlist * s.K, s.nlist, s.K, s.ids + row * s.K,
                 s.scores + row * s.K, hp, threadIdx.x);
}

__global__ __launch_bounds__(RH_BLOCK) void ivf_list_mean_kernel(const float* __restrict__ xs,
                                                                 const int32_t* __restrict__ list_off,
                                                                 const float* __restrict__ previous, int V, int D,
                                                                 float* __restrict__ out) {
  __shared__ float red[4][RH_WAVE];
  const int l = blockIdx.x, lane = threadIdx.x % RH_WAVE, w = threadIdx.x / RH_WAVE;
  int64_t lo = list_off[l], hi = list_off[l + 1];
  if (lo < 0) lo = 0;
  if (hi > V) hi = V;
  const int64_t n = hi - lo;
  for (int d0 = 0; d0 < D; d0 += RH_WAVE) {
    const int d = d0 + lane;
    float s = 0.f;
    if (d < D)
      for (int64_t r = lo + w; r < hi; r += 4) s += xs[r * D + d];
    __syncthreads();  // (the previous chunk is done with red)
    red[w][lane] = s;
    __syncthreads();
    if (w == 0 && d < D) {
      const float tot = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
      out[(int64_t)l * D + d] = n > 0 ? __fdiv_rn(tot, (float)n) : previous[(int64_t)l * D + d];
    }
  }
}

bool ivf_shape_ok(int D, int K, int S, int nprobe) {
  return topk_shape_ok(D, K, S) && nprobe >= 1 && nprobe <= kIvfMaxProbe;
}

}  // namespace

extern "C" int rh_ivf_supported(int D, int K, int S, int nprobe, int* supported) {
  RH_REQUIRE(supported != nullptr, RH_E_BADARG, "rh_ivf_supported: null pointer");
  *supported = ivf_shape_ok(D, K, S, nprobe) ? 1 : 0;
  return 0;
}

extern "C" int rh_ivf_plan(int M, int nlists, int nprobe, int K, int* rows_per_tile, int64_t* grid,
                           int64_t* workspace_bytes) {
  RH_REQUIRE(rows_per_tile != nullptr && grid != nullptr && workspace_bytes != nullptr, RH_E_BADARG,
             "rh_ivf_plan: null pointer");
  RH_REQUIRE(M >= 0 && nlists >= 1, RH_E_BADARG, "rh_ivf_plan: M=%d nlists=%d (M >= 0, nlists >= 1)", M, nlists);
  RH_REQUIRE(K >= 1 && K <= kTopkMaxK && nprobe >= 1 && nprobe <= kIvfMaxProbe, RH_E_UNSUPPORTED,
             "rh_ivf_plan: K=%d nprobe=%d unsupported (1 <= K <= %d, 1 <= nprobe <= %d)", K, nprobe, kTopkMaxK,
             kIvfMaxProbe);
  const int64_t npair = (int64_t)M * nprobe;
  *rows_per_tile = topk_rows(K);
  *grid = (npair + *rows_per_tile - 1) / *rows_per_tile + nlists + 1;
  *workspace_bytes = npair * K * 8 + npair * 4 + (int64_t)(nlists + 2) * 8;
  return 0;
}

extern "C" int rh_ivf_scan(const float* q, int64_t ldq, const float* xs, const float* bias_s, const int32_t* row_id,
                           const int32_t* list_off, int nlists, const int32_t* pair, const int32_t* pair_off,
                           const int32_t* tile_off, const int64_t* exclude, int S, int M, int D, int V, int K, int nprobe,
                           void* partials, int64_t* ids, float* scores, void* stream) {
  RH_REQUIRE(ivf_shape_ok(D, K, S, nprobe), RH_E_UNSUPPORTED,
             "rh_ivf_scan: D=%d K=%d S=%d nprobe=%d unsupported (1 <= D <= %d, 1 <= K <= %d, 0 <= S <= %d, "
             "1 <= nprobe <= %d)", D, K, S, nprobe, kTopkMaxD, kTopkMaxK, kTopkMaxS, kIvfMaxProbe);
  if (int rc = topk_scan_sizes("rh_ivf_scan", M, V, "nlists", nlists, nlists >= 1, ldq, D)) return rc;
  const int RB = topk_rows(K);
  const int64_t npair = (int64_t)M * nprobe, grid = (npair + RB - 1) / RB + nlists + 1;
  RH_REQUIRE(grid < ((int64_t)1 << 31), RH_E_UNSUPPORTED, "rh_ivf_scan: M nprobe = %lld pairs are too many",
             (long long)npair);
  if (M == 0) return 0;
  IvfArgs a{};
  if (int rc = topk_scan_args("rh_ivf_scan", &a.s, q, ldq, xs, bias_s, exclude, S, M, D, V, K, nprobe, partials, ids, scores))
    return rc;
  RH_REQUIRE(row_id && list_off && pair && pair_off && tile_off, RH_E_BADARG, "rh_ivf_scan: null pointer");
  a.row_id = row_id;
  a.list_off = list_off;
  a.pair = pair;
  a.pair_off = pair_off;
  a.tile_off = tile_off;
  a.nlists = nlists;
  static RhLdsReserved reserved;
  if (int rc = rh_reserve_lds(reserved, ivf_scan_kernel, ivf_lds_bytes(128), "rh_ivf_scan")) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ivf_scan_kernel, dim3((unsigned)grid), dim3(RH_BLOCK), ivf_lds_bytes(K), st, a);
  hipLaunchKernelGGL(ivf_merge_kernel, dim3((unsigned)M), dim3(RH_WAVE), 0, st, a);
  RH_LAUNCH_CHECK("rh_ivf_scan");
  return 0;
}

extern "C" int rh_ivf_list_mean(const float* xs, const int32_t* list_off, const float* previous, int V, int D, int nlists,
                                float* centroids, void* stream) {
  RH_REQUIRE(V >= 0 && D >= 1 && nlists >= 1, RH_E_BADARG, "rh_ivf_list_mean: V=%d D=%d nlists=%d", V, D, nlists);
  RH_REQUIRE(list_off && previous && centroids && (V == 0 || xs), RH_E_BADARG, "rh_ivf_list_mean: null pointer");
  hipLaunchKernelGGL(ivf_list_mean_kernel, dim3((unsigned)nlists), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream),
                     xs, list_off, previous, V, D, centroids);
  RH_LAUNCH_CHECK("rh_ivf_list_mean");
  return 0;
}
