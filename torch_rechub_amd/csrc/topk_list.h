// The per-row K-list of the streaming top-K kernels (topk.hip: the flat scan; ivf.hip: the list scan) and the merge of
// several such lists.  A list holds the K best (score, id) seen so far in LDS, sorted by (score descending, id
// ascending); the K-th score of a full list is the row's threshold.  The wavefront that owns a row ballots the 64 scores
// of a tile against the threshold; only the hits are looked up in the exclude / invalid lists and inserted
// cooperatively.  Candidates must arrive in ascending id among equal scores (both kernels walk ids in ascending order
// inside what one list covers): a candidate enters behind every entry of equal score and an equal score never displaces
// the K-th, so the list is the top K of what it has seen under the total order.
//
// The scan of one workgroup, topk_scan_tiles, is here too: up to RB query rows against the rows [lo, hi) of x in tiles of
// 64 -- the score tile of mfma_tile.h (exact f32 products, k-ordered accumulation from zero, bias added once at the end),
// the ballot, the insert, and the write-out of the rows' lists to the partials (unused tail: -inf, -1; every element the
// merge reads is written).  What differs between the two kernels is a rule R, a small struct the kernel fills:
//   has_row(r)      whether tile row r holds a query; the list of a row that does not is neither kept nor written
//   query_row(r)    the row of q and of exclude that tile row r holds
//   id_of(c)        the id of row c of x
//   list_offset(r)  where tile row r's list of K entries starts in part_s / part_i
//   invalid, n_inv  ids dropped for every row (null, 0: none)
// query_row and list_offset are asked only where has_row holds.  has_row is asked for every row after every tile, so it
// has to be cheap; query_row is asked at the q loads and when a row has hits, list_offset at the write-out.
#pragma once

#include <math.h>

#include "mfma_tile.h"

constexpr int kTopkMaxD = RH_TOPK_MAX_D, kTopkMaxK = RH_TOPK_MAX_K, kTopkMaxS = RH_TOPK_MAX_S, kTopkMaxSplit = RH_TOPK_MAX_SPLIT;
constexpr int kTopkListBytes = 64 * 1024;  // LDS of the K-lists of one workgroup

__host__ __device__ inline int topk_rows(int K) { return K * 64 * 8 <= kTopkListBytes ? 64 : 32; }

// the x / q chunks, the K-lists of topk_rows(K) rows, the thresholds and the counts: what topk_scan_tiles carves up
__host__ __device__ inline size_t topk_lds_bytes(int K) {
  return (size_t)2 * kT * kLd * sizeof(float) + (size_t)topk_rows(K) * K * 8 + (size_t)2 * kT * 4;
}

inline bool topk_shape_ok(int D, int K, int S) {
  return D >= 1 && D <= kTopkMaxD && K >= 1 && K <= kTopkMaxK && S >= 0 && S <= kTopkMaxS;
}

// what the flat and the list scan (and their merges) are given alike
struct TopkScanArgs {
  const float* q;          // (M, D), row stride ldq
  int64_t ldq;
  const float* x;          // (V, D) contiguous
  const float* bias;       // (V,) or null
  const int64_t* exclude;  // (M, S) or null
  int S, M, D, V, K;
  int nlist;               // lists per query in the partials
  int RB;                  // tile rows per workgroup
  float* part_s;           // (M, nlist, K) scores of the partial lists
  int32_t* part_i;         // (M, nlist, K) their ids, -1 = no entry
  int64_t* ids;            // (M, K)
  float* scores;           // (M, K)
};

// The parts of rh_topk_fwd and rh_ivf_scan that are the same.  The sizes: `count` (n_inv / nlists) is the entry point's
// own, named in the message.
inline int topk_scan_sizes(const char* who, int M, int V, const char* count, int n, bool n_ok, int64_t ldq, int D) {
  RH_REQUIRE(M >= 0 && V >= 1 && n_ok && ldq >= D, RH_E_BADARG, "%s: M=%d V=%d %s=%d ldq=%lld D=%d", who, M, V, count, n,
             (long long)ldq, D);
  return 0;
}

// For M > 0: the null pointers, the arguments and the split of the workspace into scores and ids.
inline int topk_scan_args(const char* who, TopkScanArgs* a, const float* q, int64_t ldq, const float* x, const float* bias,
                          const int64_t* exclude, int S, int M, int D, int V, int K, int nlist, void* workspace,
                          int64_t* ids, float* scores) {
  RH_REQUIRE(q && x && workspace && ids && scores && (S == 0 || exclude), RH_E_BADARG, "%s: null pointer", who);
  float* part_s = static_cast<float*>(workspace);
  *a = TopkScanArgs{q, ldq, x, bias, exclude, S, M, D, V, K, nlist, topk_rows(K), part_s,
                    reinterpret_cast<int32_t*>(part_s + (int64_t)M * nlist * K), ids, scores};
  return 0;
}

// orders the LDS accesses of the lanes of one wavefront (the hardware runs them in program order)
static __device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One row's hits of one tile, by the wavefront that owns the row: lane j holds the score s of the tile's column j and m is
// the ballot of the hits (the column exists and n < K or s > t; the caller leaves early when there is none).  id_of(j) is
// the id of column j (wavefront-uniform j).  rs / ri = the row's list (K entries), n its length and t its threshold
// (registers of the caller, uniform over the wavefront).  ex = the row's S excluded ids, invalid = n_inv ids excluded for
// every row.
template <typename IdOf>
static __device__ __forceinline__ void topk_row_hits(uint64_t m, float s, float* rs, int* ri, int& n, float& t, int K, int nch,
                                                     const int64_t* ex, int S, const int64_t* invalid, int n_inv, int lane,
                                                     IdOf id_of) {
  while (m != 0) {
    const int j = __ffsll((unsigned long long)m) - 1;
    m &= m - 1;
    const float sj = __shfl(s, j, RH_WAVE);
    if (n >= K && !(sj > t)) continue;
    const int64_t id = id_of(j);
    bool drop = false;
    for (int e = lane; e < S; e += RH_WAVE) drop |= ex[e] == id;
    for (int e = lane; e < n_inv; e += RH_WAVE) drop |= invalid[e] == id;
    if (__ballot(drop) != 0) continue;
    // p = entries that stay in front (score >= sj: every entry has a lower id); entries [p, n) move one place back
    int p = 0;
    for (int u = 0; u < nch; ++u) {
      const int e = u * RH_WAVE + lane;
      p += __popcll(__ballot(e < n && rs[e] >= sj));
    }
    float os[kTopkMaxK / RH_WAVE];
    int oi[kTopkMaxK / RH_WAVE];
#pragma unroll
    for (int u = 0; u < kTopkMaxK / RH_WAVE; ++u) {
      const int e = u * RH_WAVE + lane;
      const bool mv = e > p && e <= n && e < K;
      os[u] = mv ? rs[e - 1] : 0.f;
      oi[u] = mv ? ri[e - 1] : 0;
    }
    wave_sync();
#pragma unroll
    for (int u = 0; u < kTopkMaxK / RH_WAVE; ++u) {
      const int e = u * RH_WAVE + lane;
      if (e > p && e <= n && e < K) {
        rs[e] = os[u];
        ri[e] = oi[u];
      }
    }
    if (lane == (p & (RH_WAVE - 1))) {  // p < K: a full list takes only sj > t
      rs[p] = sj;
      ri[p] = (int)id;
    }
    wave_sync();
    if (n < K) ++n;
    if (n == K) t = rs[K - 1];
  }
}

// The scan of one workgroup of RH_BLOCK threads under the rule R (see the head of this file): the rows [lo, hi) of a.x
// against the tile rows the rule names.  lds = topk_lds_bytes(a.K) bytes of dynamic LDS.  Every thread of the workgroup
// calls this; whatever the rule reads from LDS is written, and a barrier passed, before the call.
template <typename R>
static __device__ __forceinline__ void topk_scan_tiles(const TopkScanArgs& a, const R& rule, int64_t lo, int64_t hi,
                                                       float* lds) {
  float* ws = lds;                  // x chunk (64 columns x 64 k), then the score tile [row][column]
  float* hs = ws + kT * kLd;        // q chunk (64 rows x 64 k)
  float* ls = hs + kT * kLd;        // [RB][K] list scores
  int* li = reinterpret_cast<int*>(ls + a.RB * a.K);   // [RB][K] list ids
  float* thr = reinterpret_cast<float*>(li + a.RB * a.K);  // [64] K-th score of a full list
  int* cnt = reinterpret_cast<int*>(thr + kT);         // [64] entries of the list
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int l32 = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int K = a.K, RB = a.RB;
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
      hs[r * kLd + c] = (r < RB && rule.has_row(r) && c < a.D) ? a.q[rule.query_row(r) * a.ldq + c] : 0.f;
    }
  }
  for (int64_t c0 = lo; c0 < hi; c0 += kT) {
    v16f acc = zero16();
    for (int k0 = 0; k0 < a.D; k0 += kT) {
      __syncthreads();
      for (int e = tid; e < kT * kT; e += RH_BLOCK) {
        const int r = e / kT, c = e % kT, k = k0 + c;
        ws[r * kLd + c] = (c0 + r < hi && k < a.D) ? a.x[(c0 + r) * a.D + k] : 0.f;
        if (nkc > 1) {
          const int64_t qr = (r < RB && rule.has_row(r)) ? rule.query_row(r) : -1;
          hs[r * kLd + c] = (qr >= 0 && k < a.D) ? a.q[qr * a.ldq + k] : 0.f;
        }
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
      if (!rule.has_row(row)) continue;
      const float s = ws[row * kLd + lane];
      int n = cnt[row];
      float t = thr[row];
      const uint64_t m = __ballot(c0 + lane < hi && (n < K || s > t));
      if (m == 0) continue;
      const int64_t* ex = a.S > 0 ? a.exclude + rule.query_row(row) * a.S : nullptr;
      topk_row_hits(m, s, ls + row * K, li + row * K, n, t, K, nch, ex, a.S, rule.invalid, rule.n_inv, lane,
                    [&](int j) { return rule.id_of(c0 + j); });
      if (lane == 0) {
        cnt[row] = n;
        thr[row] = t;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < RB * K; e += RH_BLOCK) {
    const int row = e / K, k = e % K;
    if (!rule.has_row(row)) continue;
    const int64_t o = rule.list_offset(row);
    const bool have = k < cnt[row];
    a.part_s[o + k] = have ? ls[e] : -INFINITY;
    a.part_i[o + k] = have ? li[e] : -1;
  }
}

// (s, id) ahead of (bs, bi) in (score descending, id ascending); id < 0 = no entry, behind everything
static __device__ __forceinline__ bool topk_ahead(float s, int id, float bs, int bi) {
  return id >= 0 && (bi < 0 || s > bs || (s == bs && id < bi));
}

// One wavefront merges the nlist sorted lists ps / pi (nlist, K) of one row into ids / scores (K,) under the same total
// order; lane l owns the lists l, l + 64, ... and keeps the best of their heads.  hp = nlist ints of LDS (the head of each
// list; touched by its owner lane only).  Ids are distinct over the lists.  Unused tail: id -1, score -inf.
static __device__ __forceinline__ void topk_merge_row(const float* ps, const int32_t* pi, int nlist, int K, int64_t* ids,
                                                      float* scores, int* hp, int lane) {
  for (int l = lane; l < nlist; l += RH_WAVE) hp[l] = 0;
  float bs;
  int bi, bl;
  auto rescan = [&]() {
    bs = -INFINITY;
    bi = -1;
    bl = -1;
    for (int l = lane; l < nlist; l += RH_WAVE) {
      const int h = hp[l];
      if (h >= K) continue;
      const float s = ps[(int64_t)l * K + h];
      const int id = pi[(int64_t)l * K + h];
      if (topk_ahead(s, id, bs, bi)) {
        bs = s;
        bi = id;
        bl = l;
      }
    }
  };
  rescan();
  int k = 0;
  for (; k < K; ++k) {
    float s = bs;
    int id = bi, l = bl;
#pragma unroll
    for (int m = RH_WAVE / 2; m >= 1; m >>= 1) {
      const float s2 = __shfl_xor(s, m, RH_WAVE);
      const int id2 = __shfl_xor(id, m, RH_WAVE), l2 = __shfl_xor(l, m, RH_WAVE);
      if (topk_ahead(s2, id2, s, id)) {
        s = s2;
        id = id2;
        l = l2;
      }
    }
    if (id < 0) break;  // every list is used up (wavefront-uniform: ids are distinct, every lane holds the same winner)
    if (lane == 0) {
      ids[k] = id;
      scores[k] = s;
    }
    if (lane == (l & (RH_WAVE - 1))) {
      hp[l] += 1;
      rescan();
    }
  }
  for (int e = k + lane; e < K; e += RH_WAVE) {
    ids[e] = -1;
    scores[e] = -INFINITY;
  }
}
