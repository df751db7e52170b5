// The per-row K-list of the streaming top-K kernels (topk.hip: the flat scan; ivf.hip: the list scan) and the merge of
// several such lists.  A list holds the K best (score, id) seen so far in LDS, sorted by (score descending, id
// ascending); the K-th score of a full list is the row's threshold.  The wavefront that owns a row ballots the 64 scores
// of a tile against the threshold; only the hits are looked up in the exclude / invalid lists and inserted
// cooperatively.  Candidates must arrive in ascending id among equal scores (both kernels walk ids in ascending order
// inside what one list covers): a candidate enters behind every entry of equal score and an equal score never displaces
// the K-th, so the list is the top K of what it has seen under the total order.
#pragma once

#include <math.h>

#include "mfma_tile.h"

constexpr int kTopkMaxD = 1024, kTopkMaxK = 256, kTopkMaxS = 1024, kTopkMaxSplit = 1024;
constexpr int kTopkListBytes = 64 * 1024;  // LDS of the K-lists of one workgroup

__host__ __device__ inline int topk_rows(int K) { return K * 64 * 8 <= kTopkListBytes ? 64 : 32; }

// the x / q chunks, the K-lists of topk_rows(K) rows, the thresholds and the counts
static inline size_t topk_lds_bytes(int K) {
  return (size_t)2 * kT * kLd * sizeof(float) + (size_t)topk_rows(K) * K * 8 + (size_t)2 * kT * 4;
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
