// Inverted-file index on the flat scan's tile (rh_ivf_*; replaces faiss's IVF{nlists},Flat index with nprobe of the
// reference's serving/faiss.py).  The table's rows are grouped by list (xs, bias_s, row_id = the original ids, ascending
// inside a list; list_off = the lists' offsets); query i probes the lists probe[i][0 .. nprobe) (-1 = none).
//
// Scan kernel, list-centric: the M nprobe (query, slot) pairs arrive grouped by list (pair = the pair indices
// i nprobe + slot in list order, group 0 = the pairs with no list, group l + 1 = list l; pair_off = the groups' offsets;
// tile_off = the prefix sum of ceil(group size / RB)).  The grid is the fixed upper bound of the tile count; a workgroup
// finds its (group, tile of RB pairs) by binary search in tile_off and leaves if there is none.  It gathers its pairs'
// query rows into the q half of LDS and walks its list's rows in tiles of 64 exactly as topk_scan_kernel walks a column
// range: the score tile of mfma_tile.h (one score depends on q_i, x_j and D alone), the K-lists of topk_list.h with
// row_id[c] as the id of column c.  Ids ascend inside a list, so the list is the top K of the probed list under (score
// descending, id ascending).  Every pair belongs to exactly one tile, which writes the pair's list to the partials at
// (query, slot) (unused tail: -inf, -1) -- also where the list is empty or absent: every element the merge reads is
// written.  Merge kernel: topk_merge_row with one list per slot.  The union of the probed lists' top K holds the top K
// of the union, so with every list probed the result is rh_topk_fwd's, bit for bit.  No atomics.
//
// List mean (the update step of k-means): one workgroup per list; wavefront w adds the rows w, w + 4, ... of the list in
// order, the four partial sums are added as (0 + 1) + (2 + 3) and divided by the count.  An empty list keeps `previous`.
#include "topk_list.h"

namespace {

constexpr int kIvfMaxProbe = 256;

struct IvfArgs {
  const float* q;           // (M, D), row stride ldq
  int64_t ldq;
  const float* xs;          // (V, D) contiguous, grouped by list
  const float* bias;        // (V,) or null, grouped alike
  const int32_t* row_id;    // (V,) original ids
  const int32_t* list_off;  // (nlists + 1,)
  const int64_t* exclude;   // (M, S) or null, original ids
  const int32_t* pair;      // (M nprobe,) pair indices grouped by list
  const int32_t* pair_off;  // (nlists + 2,)
  const int32_t* tile_off;  // (nlists + 2,)
  int S, M, D, V, K, nprobe, nlists;
  int RB;                   // pairs per workgroup
  float* part_s;            // (M, nprobe, K)
  int32_t* part_i;          // (M, nprobe, K) original ids, -1 = no entry
  int64_t* ids;             // (M, K)
  float* scores;            // (M, K)
};

size_t ivf_lds_bytes(int K) { return topk_lds_bytes(K) + (size_t)kT * 4; }

__global__ __launch_bounds__(RH_BLOCK) void ivf_scan_kernel(const IvfArgs a) {
  extern __shared__ __align__(16) float lds[];
  float* ws = lds;                  // x chunk (64 columns x 64 k), then the score tile [row][column]
  float* hs = ws + kT * kLd;        // q chunk (64 rows x 64 k)
  float* ls = hs + kT * kLd;        // [RB][K] list scores
  int* li = reinterpret_cast<int*>(ls + a.RB * a.K);   // [RB][K] list ids
  float* thr = reinterpret_cast<float*>(li + a.RB * a.K);  // [64] K-th score of a full list
  int* cnt = reinterpret_cast<int*>(thr + kT);         // [64] entries of the list
  int* prs = cnt + kT;                                 // [64] pair index of the row, -1 = no row
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int l32 = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int K = a.K, RB = a.RB;
  const int b = blockIdx.x;
  if (b >= a.tile_off[a.nlists + 1]) return;
  int g = 0;  // the last group with tile_off[g] <= b: tile_off[g + 1] > b, so the group has the tile
  for (int hi_g = a.nlists; g < hi_g;) {
    const int mid = (g + hi_g + 1) / 2;
    if (a.tile_off[mid] <= b) g = mid; else hi_g = mid - 1;
  }
  const int64_t p0 = (int64_t)a.pair_off[g] + (int64_t)(b - a.tile_off[g]) * RB, p1 = a.pair_off[g + 1];
  const int64_t npair = (int64_t)a.M * a.nprobe;
  int64_t lo = 0, hi = 0;  // group 0: no list
  if (g > 0) {
    lo = a.list_off[g - 1];
    hi = a.list_off[g];
    if (lo < 0) lo = 0;
    if (hi > a.V) hi = a.V;
  }
  const int nkc = (a.D + kT - 1) / kT;
  const bool work = wm * 32 < RB;   // RB = 32: the lower row half of the tile is empty
  const int rpw = RB / 4;           // list rows per wavefront
  const int nch = (K + RH_WAVE - 1) / RH_WAVE;
  if (tid < kT) {
    thr[tid] = -INFINITY;
    cnt[tid] = 0;
    int p = -1;
    if (tid < RB && p0 >= 0 && p0 + tid < p1 && p0 + tid < npair) {
      p = a.pair[p0 + tid];
      if (p < 0 || p >= npair) p = -1;
    }
    prs[tid] = p;
  }
  __syncthreads();
  if (nkc == 1) {  // one k chunk: the q tile is loaded once
    for (int e = tid; e < kT * kT; e += RH_BLOCK) {
      const int r = e / kT, c = e % kT;
      const int p = prs[r];
      hs[r * kLd + c] = (p >= 0 && c < a.D) ? a.q[(int64_t)(p / a.nprobe) * a.ldq + c] : 0.f;
    }
  }
  for (int64_t c0 = lo; c0 < hi; c0 += kT) {
    v16f acc = zero16();
    for (int k0 = 0; k0 < a.D; k0 += kT) {
      __syncthreads();
      for (int e = tid; e < kT * kT; e += RH_BLOCK) {
        const int r = e / kT, c = e % kT, k = k0 + c;
        ws[r * kLd + c] = (c0 + r < hi && k < a.D) ? a.xs[(c0 + r) * a.D + k] : 0.f;
        if (nkc > 1) {
          const int p = prs[r];
          hs[r * kLd + c] = (p >= 0 && k < a.D) ? a.q[(int64_t)(p / a.nprobe) * a.ldq + k] : 0.f;
        }
      }
      __syncthreads();
      const int kc = a.D - k0 < kT ? a.D - k0 : kT;
      if (work) acc = mma_lds(acc, hs + wm * 32 * kLd, kLd, 1, ws + wn * 32 * kLd, 1, kLd, (kc + 1) & ~1, l32, kk);
    }
    __syncthreads();
    if (work) {
      const int64_t c = c0 + wn * 32 + l32;
      const float bv = (a.bias != nullptr && c < hi) ? a.bias[c] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        ws[(wm * 32 + acc_row(r, kk)) * kLd + wn * 32 + l32] = a.bias != nullptr ? acc[r] + bv : acc[r];
    }
    __syncthreads();
    for (int i = 0; i < rpw; ++i) {
      const int row = w * rpw + i;
      const int p = prs[row];
      if (p < 0) continue;
      const float s = ws[row * kLd + lane];
      int n = cnt[row];
      float t = thr[row];
      const uint64_t m = __ballot(c0 + lane < hi && (n < K || s > t));
      if (m == 0) continue;
      const int64_t* ex = a.S > 0 ? a.exclude + (int64_t)(p / a.nprobe) * a.S : nullptr;
      topk_row_hits(m, s, ls + row * K, li + row * K, n, t, K, nch, ex, a.S, nullptr, 0, lane,
                    [&](int j) { return (int64_t)a.row_id[c0 + j]; });
      if (lane == 0) {
        cnt[row] = n;
        thr[row] = t;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < RB * K; e += RH_BLOCK) {
    const int row = e / K, k = e % K;
    const int p = prs[row];
    if (p < 0) continue;
    const bool have = k < cnt[row];
    const int64_t o = (int64_t)p * K + k;
    a.part_s[o] = have ? ls[e] : -INFINITY;
    a.part_i[o] = have ? li[e] : -1;
  }
}

// one wavefront per query: one list per slot
__global__ __launch_bounds__(RH_WAVE) void ivf_merge_kernel(const IvfArgs a) {
  __shared__ int hp[kIvfMaxProbe];
  const int64_t row = blockIdx.x;
  topk_merge_row(a.part_s + row * a.nprobe * a.K, a.part_i + row * a.nprobe * a.K, a.nprobe, a.K, a.ids + row * a.K,
                 a.scores + row * a.K, hp, threadIdx.x);
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
  return D >= 1 && D <= kTopkMaxD && K >= 1 && K <= kTopkMaxK && S >= 0 && S <= kTopkMaxS && nprobe >= 1 &&
         nprobe <= kIvfMaxProbe;
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
  RH_REQUIRE(M >= 0 && V >= 1 && nlists >= 1 && ldq >= D, RH_E_BADARG, "rh_ivf_scan: M=%d V=%d nlists=%d ldq=%lld D=%d", M,
             V, nlists, (long long)ldq, D);
  const int RB = topk_rows(K);
  const int64_t npair = (int64_t)M * nprobe, grid = (npair + RB - 1) / RB + nlists + 1;
  RH_REQUIRE(grid < ((int64_t)1 << 31), RH_E_UNSUPPORTED, "rh_ivf_scan: M nprobe = %lld pairs are too many",
             (long long)npair);
  if (M == 0) return 0;
  RH_REQUIRE(q && xs && row_id && list_off && pair && pair_off && tile_off && partials && ids && scores &&
                 (S == 0 || exclude), RH_E_BADARG, "rh_ivf_scan: null pointer");
  IvfArgs a{};
  a.q = q;
  a.ldq = ldq;
  a.xs = xs;
  a.bias = bias_s;
  a.row_id = row_id;
  a.list_off = list_off;
  a.exclude = exclude;
  a.pair = pair;
  a.pair_off = pair_off;
  a.tile_off = tile_off;
  a.S = S;
  a.M = M;
  a.D = D;
  a.V = V;
  a.K = K;
  a.nprobe = nprobe;
  a.nlists = nlists;
  a.RB = RB;
  a.part_s = static_cast<float*>(partials);
  a.part_i = reinterpret_cast<int32_t*>(a.part_s + npair * K);
  a.ids = ids;
  a.scores = scores;
  // the attribute belongs to the function on ONE device: once per device this process launches on
  static bool attr_set[64] = {};
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  RH_REQUIRE(e == hipSuccess, (int)e, "rh_ivf_scan: no current device: %s", hipGetErrorString(e));
  if (device < 0 || device >= 64 || !attr_set[device]) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(ivf_scan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)ivf_lds_bytes(128));
    RH_REQUIRE(e == hipSuccess, (int)e, "rh_ivf_scan: cannot reserve LDS: %s", hipGetErrorString(e));
    if (device >= 0 && device < 64) attr_set[device] = true;
  }
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
