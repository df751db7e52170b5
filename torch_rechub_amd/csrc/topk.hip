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
// The K-list (threshold, ballot, cooperative insert) and the merge of one row live in topk_list.h, shared with ivf.hip.
#include "topk_list.h"

namespace {

struct TopkArgs {
  const float* q;          // (M, D), row stride ldq
  int64_t ldq;
  const float* x;          // (V, D) contiguous
  const float* bias;       // (V,) or null
  const int64_t* exclude;  // (M, S) or null
  const int64_t* invalid;  // (n_inv,) or null
  int S, n_inv;
  int M, D, V, K, nsplit;
  int RB;                  // query rows per workgroup
  float* part_s;           // (M, nsplit, K) scores of the per-range lists
  int32_t* part_i;         // (M, nsplit, K) their ids, -1 = no entry
  int64_t* ids;            // (M, K)
  float* scores;           // (M, K)
};

__global__ __launch_bounds__(RH_BLOCK) void topk_scan_kernel(const TopkArgs a) {
  extern __shared__ __align__(16) float lds[];
  float* ws = lds;                  // x chunk (64 columns x 64 k), then the score tile [row][column]
  float* hs = ws + kT * kLd;        // q chunk (64 rows x 64 k)
  float* ls = hs + kT * kLd;        // [RB][K] list scores
  int* li = reinterpret_cast<int*>(ls + a.RB * a.K);   // [RB][K] list ids
  float* thr = reinterpret_cast<float*>(li + a.RB * a.K);  // [64] K-th score of a full list
  int* cnt = reinterpret_cast<int*>(thr + kT);         // [64] entries of the list
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int l32 = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int K = a.K, RB = a.RB;
  const int64_t r0 = (int64_t)blockIdx.x * RB;
  const int split = blockIdx.y;
  const int64_t lo = (int64_t)a.V * split / a.nsplit, hi = (int64_t)a.V * (split + 1) / a.nsplit;
  const int nkc = (a.D + kT - 1) / kT;
  const bool work = wm * 32 < RB;   // RB = 32: the lower row half of the tile is empty
  const int rpw = RB / 4;           // list rows per wavefront
  const int nch = (K + RH_WAVE - 1) / RH_WAVE;
  if (tid < kT) {
    thr[tid] = -INFINITY;
    cnt[tid] = 0;
  }
  if (nkc == 1) {  // one k chunk: the q tile is loaded once
    for (int e = tid; e < kT * kT; e += RH_BLOCK) {
      const int r = e / kT, c = e % kT;
      hs[r * kLd + c] = (r < RB && r0 + r < a.M && c < a.D) ? a.q[(r0 + r) * a.ldq + c] : 0.f;
    }
  }
  for (int64_t c0 = lo; c0 < hi; c0 += kT) {
    v16f acc = zero16();
    for (int k0 = 0; k0 < a.D; k0 += kT) {
      __syncthreads();
      for (int e = tid; e < kT * kT; e += RH_BLOCK) {
        const int r = e / kT, c = e % kT, k = k0 + c;
        ws[r * kLd + c] = (c0 + r < hi && k < a.D) ? a.x[(c0 + r) * a.D + k] : 0.f;
        if (nkc > 1) hs[r * kLd + c] = (r < RB && r0 + r < a.M && k < a.D) ? a.q[(r0 + r) * a.ldq + k] : 0.f;
      }
      __syncthreads();
      const int kc = a.D - k0 < kT ? a.D - k0 : kT;
      if (work) acc = mma_lds(acc, hs + wm * 32 * kLd, kLd, 1, ws + wn * 32 * kLd, 1, kLd, (kc + 1) & ~1, l32, kk);
    }
    __syncthreads();
    if (work) {
      const int64_t c = c0 + wn * 32 + l32;
      const float b = (a.bias != nullptr && c < hi) ? a.bias[c] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        ws[(wm * 32 + acc_row(r, kk)) * kLd + wn * 32 + l32] = a.bias != nullptr ? acc[r] + b : acc[r];
    }
    __syncthreads();
    for (int i = 0; i < rpw; ++i) {
      const int row = w * rpw + i;
      if (r0 + row >= a.M) break;
      const float s = ws[row * kLd + lane];
      int n = cnt[row];
      float t = thr[row];
      const uint64_t m = __ballot(c0 + lane < hi && (n < K || s > t));
      if (m == 0) continue;
      const int64_t* ex = a.S > 0 ? a.exclude + (r0 + row) * a.S : nullptr;
      topk_row_hits(m, s, ls + row * K, li + row * K, n, t, K, nch, ex, a.S, a.invalid, a.n_inv, lane,
                    [&](int j) { return c0 + j; });
      if (lane == 0) {
        cnt[row] = n;
        thr[row] = t;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < RB * K; e += RH_BLOCK) {
    const int row = e / K, k = e % K;
    if (r0 + row >= a.M) break;
    const bool have = k < cnt[row];
    const int64_t o = ((r0 + row) * a.nsplit + split) * K + k;
    a.part_s[o] = have ? ls[e] : -INFINITY;
    a.part_i[o] = have ? li[e] : -1;
  }
}

// one wavefront per row
__global__ __launch_bounds__(RH_WAVE) void topk_merge_kernel(const TopkArgs a) {
  __shared__ int hp[kTopkMaxSplit];
  const int64_t row = blockIdx.x;
  topk_merge_row(a.part_s + row * a.nsplit * a.K, a.part_i + row * a.nsplit * a.K, a.nsplit, a.K, a.ids + row * a.K,
                 a.scores + row * a.K, hp, threadIdx.x);
}

bool topk_shape_ok(int D, int K, int S) {
  return D >= 1 && D <= kTopkMaxD && K >= 1 && K <= kTopkMaxK && S >= 0 && S <= kTopkMaxS;
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
  RH_REQUIRE(M >= 0 && V >= 1 && n_inv >= 0 && ldq >= D, RH_E_BADARG, "rh_topk_fwd: M=%d V=%d n_inv=%d ldq=%lld D=%d", M, V,
             n_inv, (long long)ldq, D);
  RH_REQUIRE(nsplit >= 1 && nsplit <= kTopkMaxSplit && nsplit <= V, RH_E_BADARG,
             "rh_topk_fwd: nsplit=%d outside [1, min(V, %d)]", nsplit, kTopkMaxSplit);
  if (M == 0) return 0;
  RH_REQUIRE(q && x && workspace && ids && scores && (S == 0 || exclude) && (n_inv == 0 || invalid), RH_E_BADARG,
             "rh_topk_fwd: null pointer");
  TopkArgs a{};
  a.q = q;
  a.ldq = ldq;
  a.x = x;
  a.bias = bias;
  a.exclude = exclude;
  a.invalid = invalid;
  a.S = S;
  a.n_inv = n_inv;
  a.M = M;
  a.D = D;
  a.V = V;
  a.K = K;
  a.nsplit = nsplit;
  a.RB = topk_rows(K);
  a.part_s = static_cast<float*>(workspace);
  a.part_i = reinterpret_cast<int32_t*>(a.part_s + (int64_t)M * nsplit * K);
  a.ids = ids;
  a.scores = scores;
  // the attribute belongs to the function on ONE device: once per device this process launches on
  static bool attr_set[64] = {};
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  RH_REQUIRE(e == hipSuccess, (int)e, "rh_topk_fwd: no current device: %s", hipGetErrorString(e));
  if (device < 0 || device >= 64 || !attr_set[device]) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(topk_scan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)topk_lds_bytes(128));
    RH_REQUIRE(e == hipSuccess, (int)e, "rh_topk_fwd: cannot reserve LDS: %s", hipGetErrorString(e));
    if (device >= 0 && device < 64) attr_set[device] = true;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t nrt = ((int64_t)M + a.RB - 1) / a.RB;
  hipLaunchKernelGGL(topk_scan_kernel, dim3((unsigned)nrt, nsplit), dim3(RH_BLOCK), topk_lds_bytes(K), st, a);
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)M), dim3(RH_WAVE), 0, st, a);
  RH_LAUNCH_CHECK("rh_topk_fwd");
  return 0;
}
