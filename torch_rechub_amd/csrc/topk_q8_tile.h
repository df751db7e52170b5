// The scan of one workgroup over an int8 item table (SQ8: one code per dimension, one f32 scale per row), the third scan
// body beside topk_scan_tiles (topk_list.h) and topk_half_scan_tiles (topk_half_tile.h): the score tile on
// v_mfma_i32_32x32x32_i8 under the same rule struct R, the same K-lists (topk_row_hits), partials and merge.
//
//   score[i][j] = ((float)(sum_k qc[i][k] * xc[j][k]) * qs[i]) * xs[j] (+ bias[j])
// The sum is i32 and exact in any order (127^2 D < 2^24 for D <= RH_TOPK_MAX_D, so its conversion to f32 is exact too);
// then two f32 multiplications and one f32 addition in exactly that order, each rounded on its own (q8_score: nothing
// contracts to an FMA).  Nothing else enters a score, so it depends on q_i, x_j and D alone.
//
// Work split: as the other scans -- RB rows x a column range in tiles of 64 columns, four wavefronts with one 32 x 32
// accumulator quadrant each (wm = w & 1 rows, wn = w >> 1 columns), the accumulator a v16i.  How the data moves:
//   * a k chunk is 128 codes = 128 bytes; an MFMA takes 32 k, so a chunk is up to four steps and only
//     ceil(min(128, rest) / 32) of them run.  Lane (l32, kk) feeds step s the 16 codes at byte 32 s + 16 kk of its row, for
//     A and for B alike: which k of the instruction a byte lands on is the hardware's, and the same for both operands,
//     which is all an exact integer sum needs.
//   * the query codes never go through LDS.  The quantise launch leaves them with a row stride that is a multiple of 16,
//     16-byte aligned, so an A operand is always ONE 16-byte global load; there is no scalar path for q.  With D <= 128 a
//     lane's four operands are loaded once for the whole walk, otherwise the next chunk's are fetched while the MFMAs of
//     this chunk run.  Bytes of q from D on meet zeros of the table tile, so what they hold does not matter.
//   * the item tile of a stage is 64 columns x 128 B with row stride 144 B: byte for byte the LDS geometry of the half
//     tile, [buf0 9216][E 7424][buf1 9216] with the f32 score tile on buf0 + E or E + buf1, the same double buffering
//     (global loads of the next stage before this stage's MFMAs, their LDS stores after them) and the same barriers A and
//     B (topk_half_tile.h).  A B operand is ONE 16-byte LDS read at row * 144 + 32 s + 16 kk.  The table is loaded 16 bytes
//     at a time when D % 16 == 0 and it is 16-byte aligned, else byte by byte into dwords formed in registers: LDS only
//     ever sees 16-byte stores.
//   * the epilogue of a tile's last chunk: a lane converts its 16 sums, multiplies by qs of their rows (16 registers,
//     fetched once per workgroup), by xs[column], adds bias[column] and writes the f32 score tile.  From there on
//     everything is the shared code.
#pragma once

#include "topk_half_tile.h"

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kQ8Chunk = 128;  // codes (= bytes) of one k chunk: the 128 payload bytes of an item buffer's row
static_assert(kQ8Chunk + 16 == kHLdB, "an item buffer's row is one chunk plus the pad");

// The rows of the two operands' scales: what an int8 scan is given beyond TopkScanArgs, whose q and x hold the codes.
struct Q8Scales {
  const float* qs;  // (M,) scale of every query row
  const float* xs;  // (V,) scale of every table row (grouped as the table is)
};

// One score from its exact sum: two f32 multiplications and one f32 addition, each rounded on its own.  The pragma is what
// keeps them apart: HIP's __fmul_rn / __fadd_rn are plain * and +, which the default contraction fuses into an FMA.
static __device__ __forceinline__ float q8_score(int sum, float qs, float xs, float bias, bool with_bias) {
#pragma clang fp contract(off)
  const float s = ((float)sum * qs) * xs;
  return with_bias ? s + bias : s;
}

// The scan of one workgroup of RH_BLOCK threads under the rule R: the rows [lo, hi) of the int8 table a.x against the
// tile rows the rule names.  a.q = the query codes with row stride a.ldq bytes (a multiple of 16, 16-byte aligned).
// lds = topk_half_lds_bytes(a.K) bytes of dynamic LDS, 16-byte aligned.  xvec: 16-byte global loads of the table are
// legal.  kOneChunk: D <= 128, so the lane's A operands are loaded once and the registers of the prefetched ones are
// not needed (the caller picks the instantiation; one chunk costs 16 VGPRs less, which is one more wavefront per SIMD).
// Every thread calls this; whatever the rule reads from LDS is written, and a barrier passed, before the call.
template <bool kOneChunk, typename R>
static __device__ __forceinline__ void topk_q8_scan_tiles(const TopkScanArgs& a, const Q8Scales& sc, const R& rule,
                                                          int64_t lo, int64_t hi, float* lds, bool xvec) {
  char* stage = reinterpret_cast<char*>(lds);
  float* ls = reinterpret_cast<float*>(stage + kHStage);   // [RB][K] list scores
  int* li = reinterpret_cast<int*>(ls + a.RB * a.K);       // [RB][K] list ids
  float* thr = reinterpret_cast<float*>(li + a.RB * a.K);  // [64] K-th score of a full list
  int* cnt = reinterpret_cast<int*>(thr + kT);             // [64] entries of the list
  const uint8_t* x = reinterpret_cast<const uint8_t*>(a.x);
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int l32 = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int K = a.K, RB = a.RB, D = a.D;
  const int nkc = kOneChunk ? 1 : (D + kQ8Chunk - 1) / kQ8Chunk;
  const bool work = wm * 32 < RB;   // RB = 32: the lower row half of the tile is empty
  const int rpw = RB / 4;           // list rows per wavefront
  const int nch = (K + RH_WAVE - 1) / RH_WAVE;
  if (tid < kT) {
    thr[tid] = -INFINITY;
    cnt[tid] = 0;
  }
  // this lane's row of query codes (null: none), its A operands of one k chunk, the scales of its 16 accumulator rows
  const int qt = wm * 32 + l32;
  const char* qrow = (work && qt < RB && rule.has_row(qt))
                         ? reinterpret_cast<const char*>(a.q) + rule.query_row(qt) * a.ldq : nullptr;
  v4u qf[4], qn[4], pre[2];
  auto load_q = [&](int k0, v4u (&f)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + 32 * s + 16 * kk;  // k < D <= ldq and both multiples of 16: the 16 bytes lie inside the row
      f[s] = (qrow != nullptr && k < D) ? *reinterpret_cast<const v4u*>(qrow + k) : v4u{0u, 0u, 0u, 0u};
    }
  };
  float qsr[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = wm * 32 + acc_row(r, kk);
    qsr[r] = (work && row < RB && rule.has_row(row)) ? sc.qs[rule.query_row(row)] : 0.f;
  }
  // the item tile of one stage: 512 pieces of 16 codes, two per thread (piece e: column e / 8, bytes 16 (e % 8) .. + 16)
  auto load_x = [&](int64_t c0, int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + i * RH_BLOCK;
      const int64_t col = c0 + (e >> 3);
      const int k = k0 + 16 * (e & 7);
      v4u v = {0u, 0u, 0u, 0u};
      if (col < hi && k < D) {
        const uint8_t* p = x + col * D + k;
        if (xvec) {
          v = *reinterpret_cast<const v4u*>(p);
        } else {
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (k + j < D) v[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
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
    v16i acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
    for (int c = 0; c < nkc; ++c, par ^= 1) {
      const int k0 = c * kQ8Chunk;
      const bool last = c == nkc - 1;
      const int64_t nc0 = last ? c0 + kT : c0;
      const int nk0 = last ? 0 : k0 + kQ8Chunk;
      const bool more = nc0 < hi;
      if (more) {
        load_x(nc0, nk0);
        if (!kOneChunk) load_q(nk0, qn);
      }
      if (work) {
        const char* b = stage + (par ? kHScore : 0) + (wn * 32 + l32) * kHLdB + 16 * kk;
        const int steps = ((D - k0 < kQ8Chunk ? D - k0 : kQ8Chunk) + 31) / 32;
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (s < steps)
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(v4i, qf[s]),
                                                        *reinterpret_cast<const v4i*>(b + 32 * s), acc, 0, 0, 0);
      }
      float* ws = reinterpret_cast<float*>(stage + (par ? kHBuf : 0));  // the score tile [row][column] of this stage
      if (last || c == 0) __syncthreads();  // A
      if (last && work) {
        const int64_t col = c0 + wn * 32 + l32;
        const bool have = col < hi;
        const float xv = have ? sc.xs[col] : 0.f;
        const float bv = (a.bias != nullptr && have) ? a.bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          ws[(wm * 32 + acc_row(r, kk)) * kLd + wn * 32 + l32] = q8_score(acc[r], qsr[r], xv, bv, a.bias != nullptr);
      }
      if (more) {
        store_x(stage + (par ? 0 : kHScore));
        if (!kOneChunk) {
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
