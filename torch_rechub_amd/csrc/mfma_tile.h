// The 64 x 64 workgroup tile on v_mfma_f32_32x32x2_f32 (exact f32 products, k-ordered accumulation) shared by the
// attention kernels (hstu.hip; softmax_attn_tile.h, the flash-style body of hllm.hip and t5attn.hip), the streaming cross
// entropy (stream_ce.hip), the top-k scores (topk.hip, ivf.hip) and SASRec's row-tile GEMM stages (sasrec.hip).  Helpers only: a
// kernel family that is more than the tile has its own header on top of this one, as softmax_attn_tile.h is.
//
// Lane map: four wavefronts per workgroup; wavefront w owns the 32 x 32 accumulator of quadrant (wm = w & 1, wn = w >> 1);
// lane (li = lane % 32, kk = lane / 32) feeds A[li][k + kk] and B[k + kk][li], and holds C[4 kk + (r & 3) + 8 (r >> 2)][li]
// in acc[r].  Tiles in LDS are 64 rows of stride kLd.
#pragma once

#include "common.h"

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kT = 64;          // tile edge (queries, keys, V columns, rows) and LDS column chunk
constexpr int kLd = kT + 1;     // padded LDS row stride

static __device__ __forceinline__ int acc_row(int r, int kk) { return 4 * kk + (r & 3) + 8 * (r >> 2); }

static __device__ __forceinline__ v16f zero16() {
  v16f z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// acc += A (32 x K) B (K x 32) with A[i][k] = a[i * ai + k * ak], B[k][j] = b[k * bk + j * bj] (LDS), K even
static __device__ __forceinline__ v16f mma_lds(v16f acc, const float* a, int ai, int ak, const float* b, int bk, int bj,
                                               int K, int li, int kk) {
  for (int k = 0; k < K; k += 2) {
    const float av = a[li * ai + (k + kk) * ak];
    const float bv = b[(k + kk) * bk + li * bj];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
  }
  return acc;
}

// rows [r0, r0 + 64) x columns [c0, c0 + 64) of one head (column offset col) of sample b into s[64][kLd]; zero outside
// L / d
static __device__ __forceinline__ void load_tile(float* s, const float* base, int64_t ld, int col, int c0, int r0, int L,
                                                 int d, int b, int tid) {
  for (int e = tid; e < kT * kT; e += RH_BLOCK) {
    const int r = e / kT, c = e % kT;
    const int row = r0 + r;
    float v = 0.f;
    if (row < L && c0 + c < d) v = base[((int64_t)b * L + row) * ld + col + c0 + c];
    s[r * kLd + c] = v;
  }
}
