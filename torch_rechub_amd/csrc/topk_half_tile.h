// The scan of one workgroup over an fp16 or bf16 item table: topk_scan_tiles of topk_list.h with the score tile on
// v_mfma_f32_32x32x16_f16 / _bf16, under the same rule struct R, the same K-lists (topk_row_hits), partials and merge.
//
//   score[i][j] = sum_k T(q[i][k]) * x[j][k] (+ bias[j])
// q is fp32 in memory and rounded to T (nearest even) when a lane loads its operand; a product of two T values is exact
// in f32 (22 / 16 significand bits); the sum is f32 from zero over k in steps of 16 (one MFMA each, ascending, the table
// and the query zero-padded to the step; the order inside one instruction is the hardware's); the bias is one f32 add at
// the end.  Nothing else enters a score, so it depends on q_i, x_j and D alone, as the f32 scan's does.
//
// Work split: as the f32 scan -- RB rows x a column range in tiles of 64 columns, four wavefronts with one 32 x 32
// accumulator quadrant each (wm = w & 1 rows, wn = w >> 1 columns).  What moves differently:
//   * q never goes through LDS.  Lane (l32, kk) feeds A[l32][16 s + 8 kk .. + 8) of its row to step s, so a chunk of 64 k
//     is four 8-half operands = 16 VGPRs per lane.  With D <= 64 they are loaded and rounded once for the whole walk;
//     otherwise the next chunk's are fetched (from L1 / L2) while the MFMAs of the current chunk run.
//   * the item tile (64 columns x 64 k of halves, row stride 72 halves = 144 B) is double-buffered: the global loads of the
//     next stage (16 bytes = 8 halves per lane and load when D % 8 == 0 and the table is 16-byte aligned, single halves
//     otherwise) are issued before the MFMAs of this stage and stored to the other buffer after them.  Lane (l32, kk) reads
//     its B operand for step s as ONE 16-byte LDS read at row * 144 + 32 s + 16 kk: sixteen consecutive lanes start 36
//     dwords apart and cover the 64 banks exactly once.
//   * LDS: [buf0 9216][E 7424][buf1 9216]; the f32 score tile (64 x 65 floats, 16 640 B) of a stage that read buf0 lies
//     on buf0 + E, of one that read buf1 on E + buf1 -- never on the buffer the prefetch is filling.  Barriers per stage:
//     A (every wavefront is done with the MFMAs of this stage and the ballots of the previous tile; then the score tile
//     and the prefetched tile are stored) and B (both are visible; then the ballots).  A stage in the middle of a tile's
//     k chunks has no score tile and needs only B.
//   25 856 B of staging against the f32 scan's 33 280: the workgroups-per-CU bands of the f32 scan hold or improve.
#pragma once

#include "half_mfma.h"
#include "topk_list.h"

constexpr int kHLdB = (kT + 8) * 2;                   // bytes of one row of an item buffer
constexpr int kHBuf = kT * kHLdB;                     // one item buffer
constexpr int kHScore = kT * kLd * 4;                 // the score tile
constexpr int kHStage = kHScore + kHBuf;              // [buf0][E][buf1]
static_assert(kHScore >= kHBuf && kHScore % 16 == 0 && kHBuf % 16 == 0, "the score tile starts on either buffer");

__host__ __device__ inline size_t topk_half_lds_bytes(int K) {
  return (size_t)kHStage + (size_t)topk_rows(K) * K * 8 + (size_t)2 * kT * 4;
}
// with [64] ints behind them: the pair indices of a list-scan workgroup (IvfRule::prs)
inline size_t ivf_half_lds_bytes(int K) { return topk_half_lds_bytes(K) + (size_t)kT * 4; }

// the `vec` of a half-table scan kernel: bit 0 = 16-byte loads of the table are legal (a row is a multiple of 16 bytes,
// the base aligned), bit 1 = of q
inline int vec_flags(const TopkScanArgs& s) {
  const bool xvec = s.D % 8 == 0 && reinterpret_cast<uintptr_t>(s.x) % 16 == 0;
  const bool qvec = s.ldq % 4 == 0 && reinterpret_cast<uintptr_t>(s.q) % 16 == 0;
  return (xvec ? 1 : 0) | (qvec ? 2 : 0);
}

// the two table types, TableF16 and TableBf16, are half_mfma.h's

// q[row][k .. k + 8) rounded to T, zero from D on (row = null: a tile row without a query); vec: 16-byte loads are legal
template <typename T>
static __device__ __forceinline__ v4u half_q8(const float* row, int k, int D, bool vec) {
  float f[8];
  if (row != nullptr && vec && k + 8 <= D) {
    const float4 u = *reinterpret_cast<const float4*>(row + k), v = *reinterpret_cast<const float4*>(row + k + 4);
    f[0] = u.x, f[1] = u.y, f[2] = u.z, f[3] = u.w, f[4] = v.x, f[5] = v.y, f[6] = v.z, f[7] = v.w;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (row != nullptr && k + i < D) ? row[k + i] : 0.f;
  }
  v4u r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = T::round(f[2 * j]) | (T::round(f[2 * j + 1]) << 16);
  return r;
}

// The scan of one workgroup of RH_BLOCK threads under the rule R: the rows [lo, hi) of the T table a.x against the tile
// rows the rule names.  lds = topk_half_lds_bytes(a.K) bytes of dynamic LDS, 16-byte aligned.  xvec / qvec: 16-byte
// global loads of the table (D % 8 == 0, aligned) / of q (ldq % 4 == 0, aligned) are legal.  Every thread calls this;
// whatever the rule reads from LDS is written, and a barrier passed, before the call.
template <typename T, typename R>
static __device__ __forceinline__ void topk_half_scan_tiles(const TopkScanArgs& a, const R& rule, int64_t lo, int64_t hi,
                                                            float* lds, bool xvec, bool qvec) {
  char* stage = reinterpret_cast<char*>(lds);
  float* ls = reinterpret_cast<float*>(stage + kHStage);   // [RB][K] list scores
  int* li = reinterpret_cast<int*>(ls + a.RB * a.K);       // [RB][K] list ids
  float* thr = reinterpret_cast<float*>(li + a.RB * a.K);  // [64] K-th score of a full list
  int* cnt = reinterpret_cast<int*>(thr + kT);             // [64] entries of the list
  const uint16_t* x = reinterpret_cast<const uint16_t*>(a.x);
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int l32 = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int K = a.K, RB = a.RB, D = a.D;
  const int nkc = (D + kT - 1) / kT;
  const bool work = wm * 32 < RB;   // RB = 32: the lower row half of the tile is empty
  const int rpw = RB / 4;           // list rows per wavefront
  const int nch = (K + RH_WAVE - 1) / RH_WAVE;
  if (tid < kT) {
    thr[tid] = -INFINITY;
    cnt[tid] = 0;
  }
  // this lane's row of q (null: none) and its A operands of one k chunk
  const int qt = wm * 32 + l32;
  const float* qrow = (work && qt < RB && rule.has_row(qt)) ? a.q + rule.query_row(qt) * a.ldq : nullptr;
  v4u qf[4], qn[4], pre[2];
  auto load_q = [&](int k0, v4u (&f)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) f[s] = half_q8<T>(qrow, k0 + 16 * s + 8 * kk, D, qvec);
  };
  // the item tile of one stage: 512 pieces of 8 halves, two per thread (piece e: column e / 8, halves 8 (e % 8) .. + 8)
  auto load_x = [&](int64_t c0, int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + i * RH_BLOCK;
      const int64_t col = c0 + (e >> 3);
      const int k = k0 + 8 * (e & 7);
      v4u v = {0u, 0u, 0u, 0u};
      if (col < hi && k < D) {
        const uint16_t* p = x + col * D + k;
        if (xvec) {
          v = *reinterpret_cast<const v4u*>(p);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (k + j < D) v[j >> 1] |= (uint32_t)p[j] << (16 * (j & 1));
        }
      }
      pre[i] = v;
    }
  };
  auto store_x = [&](char* buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + i * RH_BLOCK;
      *reinterpret_cast<v4u*>(buf + (e >> 3) * kHLdB + 16 * (e & 7)) = pre[i];
    }
  };
  if (lo < hi) {
    load_x(lo, 0);
    store_x(stage);
    load_q(0, qf);
  }
  __syncthreads();
  int par = 0;  // the buffer this stage reads: buf0 at 0, buf1 at kHScore
  for (int64_t c0 = lo; c0 < hi; c0 += kT) {
    v16f acc = zero16();
    for (int c = 0; c < nkc; ++c, par ^= 1) {
      const int k0 = c * kT;
      const bool last = c == nkc - 1;
      const int64_t nc0 = last ? c0 + kT : c0;
      const int nk0 = last ? 0 : k0 + kT;
      const bool more = nc0 < hi;
      if (more) {
        load_x(nc0, nk0);
        if (nkc > 1) load_q(nk0, qn);
      }
      if (work) {
        const char* b = stage + (par ? kHScore : 0) + (wn * 32 + l32) * kHLdB + 16 * kk;
        const int steps = ((D - k0 < kT ? D - k0 : kT) + 15) / 16;
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (s < steps) acc = T::mfma(qf[s], *reinterpret_cast<const v4u*>(b + 32 * s), acc);
      }
      float* ws = reinterpret_cast<float*>(stage + (par ? kHBuf : 0));  // the score tile [row][column] of this stage
      if (last || c == 0) __syncthreads();  // A
      if (last && work) {
        const int64_t col = c0 + wn * 32 + l32;
        const float bv = (a.bias != nullptr && col < hi) ? a.bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          ws[(wm * 32 + acc_row(r, kk)) * kLd + wn * 32 + l32] = a.bias != nullptr ? acc[r] + bv : acc[r];
      }
      if (more) {
        store_x(stage + (par ? 0 : kHScore));
        if (nkc > 1) {
#pragma unroll
          for (int s = 0; s < 4; ++s) qf[s] = qn[s];
        }
      }
      __syncthreads();  // B
      if (!last) continue;
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
