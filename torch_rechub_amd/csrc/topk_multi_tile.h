// The scan of one workgroup for multi-interest queries (topk_multi.hip): q is (M, I, D), one vector per interest of a
// user, and a user gets ONE K-list, the top K of
//   t(u,i,j)  = dot(q[u,i,:], x[j,:])      the score tile of the flat scans, bit for bit what they give row (u, i)
//   t'(u,i,j) = t + qbias[u,i]             one f32 addition; skipped without qbias
//   s(u,j)    = max_i t'(u,i,j)
//   score     = s + bias[j]                one f32 addition after the fold; skipped without bias
// which is the merged, de-duplicated union of the I per-interest top-K lists: an item of the top K of s reaches its maximum
// under some interest i*, and K items ahead of it there would each have s >= their score under i*, so it is in i*'s top K.
// Adding bias after the fold gives the bits of adding it before: round-to-nearest addition of one b is monotone in its other
// operand, so max_i (t'_i + b) = (max_i t'_i) + b.  qbias[u,i] = -inf marks an absent interest; a user without any interest
// has no candidates and gets the (-1, -inf) tail.
//
// Tile rows: a user occupies Ip = 2^sh consecutive rows of the 64-row MFMA tile, Ip the next power of two >= I; a workgroup
// holds U = min(64 / Ip, topk_rows(K)) users.  Slot rows i >= I, users past M and absent interests feed zeros and fold as
// -inf.  With Ip >= 2 the lists of U <= 32 users fit 64 KiB at every K, so the whole 64-row tile is used at every K.
// Fold in registers: a lane of mfma_tile.h's map holds C[4 kk + (r & 3) + 8 (r >> 2)][li], four consecutive rows per group
// of four accumulator registers.  Ip = 2: a maximum inside the group; 4: across the group; 8: and one exchange between lane
// l and lane l ^ 32 (the other kk: a cross-lane move, no LDS); 16: and the maximum of two groups.  Only the folded (U x 64)
// tile goes to LDS, and the list stage (ballot against the threshold, topk_row_hits) runs once per user.
//
// The producer P of the 32 x 32 accumulators is a template parameter: MultiTileF32 (v_mfma_f32_32x32x2_f32 through mma_lds,
// x and q chunks in LDS as topk_scan_tiles has them) and MultiTileHalf<T> (v_mfma_f32_32x32x16_f16 / _bf16 with the
// operand helpers and the LDS geometry of topk_half_tile.h: q in registers, the item tile double-buffered, barriers A / B).
//   P(s, rows, stage, lo, hi, vec)  loads what the whole walk needs; ends in a barrier
//   mma(c0)                         the accumulators of the tile at column c0 (every k chunk)
//   score()                         where the folded tile of this tile goes (64 rows of stride kLd)
//   before_score()                  the barrier after which score() may be written
//   after_score()                   what the producer stores between the folded tile and the barrier before the list stage
#pragma once

#include "topk_half_tile.h"
#include "topk_rules.h"

struct TopkMultiArgs {
  TopkArgs f;          // s.q = the M I interest rows (row stride ldq), s.M = users, s.exclude per user, s.RB = U, nlist = nsplit
  const float* qbias;  // (M, I) or null
  int I, sh;           // interests per user, log2 Ip
};

__host__ __device__ inline int topk_multi_shift(int I) {
  int sh = 0;
  while ((1 << sh) < I) ++sh;
  return sh;
}

__host__ __device__ inline int topk_multi_users(int I, int K) {
  const int u = kT >> topk_multi_shift(I);
  return u < topk_rows(K) ? u : topk_rows(K);
}

// which interest row a tile row holds
struct MultiRows {
  int64_t u0;  // the workgroup's first user
  int M, I, sh, rows;  // rows = U Ip tile rows in use
  const float* qbias;
  __device__ __forceinline__ int64_t user(int r) const { return u0 + (r >> sh); }
  __device__ __forceinline__ int64_t q_row(int r) const { return user(r) * I + (r & ((1 << sh) - 1)); }
  // -inf: tile row r holds no interest (a padded slot, a user past M, an absent interest); else its qbias, 0 without one
  __device__ __forceinline__ float row_bias(int r) const {
    if (r >= rows || (r & ((1 << sh) - 1)) >= I || user(r) >= M) return -INFINITY;
    return qbias != nullptr ? qbias[q_row(r)] : 0.f;
  }
};

struct MultiTileF32 {
  static constexpr int kStage = 2 * kT * kLd * (int)sizeof(float);
  static constexpr int kWaves = 4;  // wavefronts per SIMD the kernel is held to (128 registers: no scratch)
  const TopkScanArgs& a;
  const MultiRows& rows;
  float *ws, *hs;  // x chunk (64 columns x 64 k), then the folded tile; q chunk (64 rows x 64 k)
  int64_t hi;
  int tid, l32, kk, wm, wn, nkc;
  bool work;
  uint32_t live;  // bit j: tile row tid / 64 + 4 j, the j-th row this thread loads, holds an interest

  __device__ __forceinline__ MultiTileF32(const TopkScanArgs& a_, const MultiRows& rows_, float* stage, int64_t lo,
                                          int64_t hi_, int)
      : a(a_), rows(rows_), ws(stage), hs(stage + kT * kLd), hi(hi_) {
    tid = threadIdx.x;
    const int lane = tid % RH_WAVE, w = tid / RH_WAVE;
    l32 = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
    nkc = (a.D + kT - 1) / kT;
    work = wm * 32 < rows.rows;
    live = 0;
#pragma unroll
    for (int j = 0; j < kT * kT / RH_BLOCK; ++j)
      if (rows.row_bias(tid / kT + 4 * j) != -INFINITY) live |= 1u << j;
    if (nkc == 1) load_q(0);  // one k chunk: the q tile is loaded once
  }
  __device__ __forceinline__ void load_q(int k0) {
#pragma unroll
    for (int j = 0; j < kT * kT / RH_BLOCK; ++j) {
      const int r = tid / kT + 4 * j, c = tid % kT, k = k0 + c;
      hs[r * kLd + c] = (((live >> j) & 1u) != 0 && k < a.D) ? a.q[rows.q_row(r) * a.ldq + k] : 0.f;
    }
  }
  __device__ __forceinline__ v16f mma(int64_t c0) {
    v16f acc = zero16();
    for (int k0 = 0; k0 < a.D; k0 += kT) {
      __syncthreads();
      for (int e = tid; e < kT * kT; e += RH_BLOCK) {
        const int r = e / kT, c = e % kT, k = k0 + c;
        ws[r * kLd + c] = (c0 + r < hi && k < a.D) ? a.x[(c0 + r) * a.D + k] : 0.f;
      }
      if (nkc > 1) load_q(k0);
      __syncthreads();
      const int kc = a.D - k0 < kT ? a.D - k0 : kT;
      if (work) acc = mma_lds(acc, hs + wm * 32 * kLd, kLd, 1, ws + wn * 32 * kLd, 1, kLd, (kc + 1) & ~1, l32, kk);
    }
    return acc;
  }
  __device__ __forceinline__ float* score() const { return ws; }
  __device__ __forceinline__ void before_score() const { __syncthreads(); }
  __device__ __forceinline__ void after_score() const {}
};

template <typename T>
struct MultiTileHalf {
  static constexpr int kStage = kHStage;  // [buf0][E][buf1] of topk_half_tile.h
  static constexpr int kWaves = 3;        // the sixteen qbias registers on top of the half body's 122 do not fit 128
  const TopkScanArgs& a;
  char* stage;
  const uint16_t* x;
  const float* qrow;  // this lane's row of q (null: its tile row holds no interest)
  int64_t hi;
  int tid, l32, kk, wm, wn, nkc, par;  // par: the buffer this stage reads, buf0 at 0, buf1 at kHScore
  bool work, xvec, qvec, more;
  v4u qf[4], qn[4], pre[2];

  __device__ __forceinline__ MultiTileHalf(const TopkScanArgs& a_, const MultiRows& rows, float* stage_, int64_t lo,
                                           int64_t hi_, int vec)
      : a(a_), stage(reinterpret_cast<char*>(stage_)), x(reinterpret_cast<const uint16_t*>(a_.x)), hi(hi_) {
    tid = threadIdx.x;
    const int lane = tid % RH_WAVE, w = tid / RH_WAVE;
    l32 = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
    nkc = (a.D + kT - 1) / kT;
    work = wm * 32 < rows.rows;
    xvec = (vec & 1) != 0, qvec = (vec & 2) != 0;
    const int qt = wm * 32 + l32;
    qrow = (work && rows.row_bias(qt) != -INFINITY) ? a.q + rows.q_row(qt) * a.ldq : nullptr;
    par = 0;
    more = false;
    if (lo < hi) {
      load_x(lo, 0);
      store_x(stage);
      load_q(0, qf);
    }
    __syncthreads();
  }
  __device__ __forceinline__ void load_q(int k0, v4u (&f)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) f[s] = half_q8<T>(qrow, k0 + 16 * s + 8 * kk, a.D, qvec);
  }
  // the item tile of one stage: 512 pieces of 8 halves, two per thread (piece e: column e / 8, halves 8 (e % 8) .. + 8)
  __device__ __forceinline__ void load_x(int64_t c0, int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + i * RH_BLOCK;
      const int64_t col = c0 + (e >> 3);
      const int k = k0 + 8 * (e & 7);
      v4u v = {0u, 0u, 0u, 0u};
      if (col < hi && k < a.D) {
        const uint16_t* p = x + col * a.D + k;
        if (xvec) {
          v = *reinterpret_cast<const v4u*>(p);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (k + j < a.D) v[j >> 1] |= (uint32_t)p[j] << (16 * (j & 1));
        }
      }
      pre[i] = v;
    }
  }
  __device__ __forceinline__ void store_x(char* buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + i * RH_BLOCK;
      *reinterpret_cast<v4u*>(buf + (e >> 3) * kHLdB + 16 * (e & 7)) = pre[i];
    }
  }
  __device__ __forceinline__ void take_next() {
    if (!more) return;
    store_x(stage + (par ? 0 : kHScore));
    if (nkc > 1) {
#pragma unroll
      for (int s = 0; s < 4; ++s) qf[s] = qn[s];
    }
  }
  // Returns before barrier A of the tile's last stage, with the next tile's first stage in flight (pre, qn).
  __device__ __forceinline__ v16f mma(int64_t c0) {
    v16f acc = zero16();
    for (int c = 0;; ++c, par ^= 1) {
      const int k0 = c * kT;
      const bool last = c == nkc - 1;
      const int64_t nc0 = last ? c0 + kT : c0;
      const int nk0 = last ? 0 : k0 + kT;
      more = nc0 < hi;
      if (more) {
        load_x(nc0, nk0);
        if (nkc > 1) load_q(nk0, qn);
      }
      if (work) {
        const char* b = stage + (par ? kHScore : 0) + (wn * 32 + l32) * kHLdB + 16 * kk;
        const int steps = ((a.D - k0 < kT ? a.D - k0 : kT) + 15) / 16;
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (s < steps) acc = T::mfma(qf[s], *reinterpret_cast<const v4u*>(b + 32 * s), acc);
      }
      if (last) return acc;
      if (c == 0) __syncthreads();  // A: the list stage of the previous tile is done with its folded tile
      take_next();
      __syncthreads();  // B
    }
  }
  // a stage that read buf0 has its tile on buf0 + E, one that read buf1 on E + buf1: never where the prefetch goes
  __device__ __forceinline__ float* score() const { return reinterpret_cast<float*>(stage + (par ? kHBuf : 0)); }
  __device__ __forceinline__ void before_score() const { __syncthreads(); }  // A
  __device__ __forceinline__ void after_score() {
    take_next();
    par ^= 1;
  }
};

static __device__ __forceinline__ float max4(const float* v) { return fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])); }

// Every thread of a workgroup of RH_BLOCK threads calls this: users [blockIdx.x U, + U) against the column range
// blockIdx.y of a.f.s.nlist.  lds = P::kStage + 8 U K + 512 bytes of dynamic LDS, 16-byte aligned.
template <typename P>
static __device__ __forceinline__ void topk_multi_scan_tiles(const TopkMultiArgs& a, float* lds, int vec) {
  const TopkScanArgs& s = a.f.s;
  const int K = s.K, U = s.RB, sh = a.sh, split = blockIdx.y;
  const int64_t lo = (int64_t)s.V * split / s.nlist, hi = (int64_t)s.V * (split + 1) / s.nlist;
  const MultiRows rows{(int64_t)blockIdx.x * U, s.M, a.I, sh, U << sh, a.qbias};
  float* ls = lds + P::kStage / sizeof(float);           // [U][K] list scores
  int* li = reinterpret_cast<int*>(ls + U * K);          // [U][K] list ids
  float* thr = reinterpret_cast<float*>(li + U * K);     // [64] K-th score of a full list
  int* cnt = reinterpret_cast<int*>(thr + kT);           // [64] entries of the list; -1: the user has no interest
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int l32 = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int rpw = U / 4;  // users per wavefront (U is 4, 8, 16, 32 or 64)
  const int nch = (K + RH_WAVE - 1) / RH_WAVE;
  const bool work = wm * 32 < rows.rows, has_qb = a.qbias != nullptr;
  if (tid < kT) {
    bool any = false;
    if (tid < U)
      for (int i = 0; i < a.I; ++i) any |= rows.row_bias((tid << sh) + i) != -INFINITY;
    thr[tid] = -INFINITY;
    cnt[tid] = any ? 0 : -1;
  }
  float qb[16];  // row_bias of this lane's sixteen accumulator rows
#pragma unroll
  for (int r = 0; r < 16; ++r) qb[r] = rows.row_bias(wm * 32 + acc_row(r, kk));
  P prod(s, rows, lds, lo, hi, vec);
  for (int64_t c0 = lo; c0 < hi; c0 += kT) {
    const v16f acc = prod.mma(c0);
    float* fs = prod.score();  // the folded tile [user][column]
    prod.before_score();
    if (work) {
      const int64_t c = c0 + wn * 32 + l32;
      const float b = (s.bias != nullptr && c < hi) ? s.bias[c] : 0.f;
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = qb[r] == -INFINITY ? -INFINITY : (has_qb ? acc[r] + qb[r] : acc[r]);
      float* f = fs + wn * 32 + l32;
      const int ub = (wm * 32) >> sh;  // the first user of this quadrant
      auto put = [&](int user, float m) { f[user * kLd] = s.bias != nullptr ? m + b : m; };
      if (sh == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) put(ub + acc_row(r, kk), v[r]);
      } else if (sh == 1) {  // rows 8 g + 4 kk + {0, 1} and + {2, 3}: users 4 g + 2 kk and + 1 of the quadrant
#pragma unroll
        for (int p = 0; p < 8; ++p) put(ub + 4 * (p >> 1) + 2 * kk + (p & 1), fmaxf(v[2 * p], v[2 * p + 1]));
      } else if (sh == 2) {  // rows 8 g + 4 kk .. + 4: user 2 g + kk
#pragma unroll
        for (int g = 0; g < 4; ++g) put(ub + 2 * g + kk, max4(v + 4 * g));
      } else if (sh == 3) {  // rows 8 g .. + 8, half of them in lane l ^ 32: user g
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float m = max4(v + 4 * g);
          m = fmaxf(m, __shfl_xor(m, 32, RH_WAVE));
          if (kk == 0) put(ub + g, m);
        }
      } else {  // rows 16 h .. + 16: groups 2 h and 2 h + 1 of both lanes
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float m = fmaxf(max4(v + 8 * h), max4(v + 8 * h + 4));
          m = fmaxf(m, __shfl_xor(m, 32, RH_WAVE));
          if (kk == 0) put(ub + h, m);
        }
      }
    }
    prod.after_score();
    __syncthreads();  // B: the folded tile (and the producer's next stage) is visible
    for (int i = 0; i < rpw; ++i) {
      const int u = w * rpw + i;
      int n = cnt[u];
      if (n < 0) continue;
      const float sc = fs[u * kLd + lane];
      float t = thr[u];
      const uint64_t m = __ballot(c0 + lane < hi && (n < K || sc > t));
      if (m == 0) continue;
      const int64_t* ex = s.S > 0 ? s.exclude + (rows.u0 + u) * s.S : nullptr;
      topk_row_hits(m, sc, ls + u * K, li + u * K, n, t, K, nch, ex, s.S, a.f.invalid, a.f.n_inv, lane,
                    [&](int j) { return c0 + j; });
      if (lane == 0) {
        cnt[u] = n;
        thr[u] = t;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < U * K; e += RH_BLOCK) {
    const int u = e / K, k = e % K;
    if (rows.u0 + u >= s.M) continue;
    const int64_t o = ((rows.u0 + u) * s.nlist + split) * K;
    const bool have = k < cnt[u];
    s.part_s[o + k] = have ? ls[e] : -INFINITY;
    s.part_i[o + k] = have ? li[e] : -1;
  }
}
