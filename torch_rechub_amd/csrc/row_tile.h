// The row tile of the transformer-block kernels (sasrec.hip, encoder.hip): a workgroup of four wavefronts owns TR rows
// padded to DP columns (D <= 64: DP = 64, TR = 64, wavefronts 2 x 2; D <= 128: DP = 128, TR = 32, wavefronts 1 x 4), so
// every wavefront holds ONE 32 x 32 accumulator of v_mfma_f32_32x32x2_f32 (mfma_tile.h) per (TR, DP) product.  A tile in LDS
// has row stride DP + 1; rows beyond M and columns beyond D are held as zeros, so the products need no edge cases (an odd
// width meets a zero in the second half of its last 2-wide MFMA step).  A weight matrix passes through LDS kKC reduction
// steps at a time (kKC x (DP + 1) floats), never whole.
#pragma once

#include "mfma_tile.h"

constexpr int kKC = 32;    // reduction steps of a weight matrix held in LDS at a time

template <int DP>
struct Tile {
  static constexpr int TR = DP == 64 ? 64 : 32;   // rows of a workgroup
  static constexpr int LD = DP + 1;               // LDS row stride
};

struct Lane {
  int tid, lane, w, li, kk, wm, wn;
};

template <int DP>
__device__ __forceinline__ Lane lane_of() {
  Lane t;
  t.tid = threadIdx.x;
  t.lane = t.tid % RH_WAVE;
  t.w = t.tid / RH_WAVE;
  t.li = t.lane % 32;
  t.kk = t.lane / 32;
  t.wm = DP == 64 ? (t.w & 1) : 0;
  t.wn = DP == 64 ? (t.w >> 1) : t.w;
  return t;
}

// rows [r0, r0 + TR) of src (M, D) with row stride ld into s; zero beyond M and D
template <int DP>
__device__ __forceinline__ void load_rows(float* s, const float* src, int64_t ld, int r0, int M, int D, int tid) {
  constexpr int TR = Tile<DP>::TR, LD = Tile<DP>::LD;
  for (int e = tid; e < TR * DP; e += RH_BLOCK) {
    const int r = e / DP, c = e % DP;
    float v = 0.f;
    if (r0 + r < M && c < D) v = src[(int64_t)(r0 + r) * ld + c];
    s[r * LD + c] = v;
  }
}

// acc += A B over K reduction steps: A = the LDS tile (TR x DP, zero beyond K), B[k][n] = W[n ldw + k] (WT: y = A W^T with
// W (N, K) row-major) or W[k ldw + n] (g A = G W with W (K, N) row-major); B is staged kKC steps at a time in wl, zero
// beyond K and N.  Every thread of the workgroup calls this; it synchronises before it reads A.
template <int DP, bool WT>
__device__ __forceinline__ v16f tile_gemm(v16f acc, const float* A, const float* W, int64_t ldw, int K, int N, float* wl,
                                          const Lane& t) {
  constexpr int LD = Tile<DP>::LD;
  for (int k0 = 0; k0 < K; k0 += kKC) {
    __syncthreads();
    for (int e = t.tid; e < kKC * DP; e += RH_BLOCK) {
      int kc, n;
      float v = 0.f;
      if (WT) {
        kc = e % kKC;
        n = e / kKC;
        if (k0 + kc < K && n < N) v = W[(int64_t)n * ldw + k0 + kc];
      } else {
        n = e % DP;
        kc = e / DP;
        if (k0 + kc < K && n < N) v = W[(int64_t)(k0 + kc) * ldw + n];
      }
      wl[kc * LD + n] = v;
    }
    __syncthreads();
    acc = mma_lds(acc, A + 32 * t.wm * LD + k0, LD, 1, wl + 32 * t.wn, LD, 1, kKC, t.li, t.kk);
  }
  return acc;
}

// f(row in the tile, column, value) over this wavefront's 32 x 32 block
template <typename F>
__device__ __forceinline__ void for_acc(const v16f& acc, const Lane& t, F f) {
#pragma unroll
  for (int r = 0; r < 16; ++r) f(32 * t.wm + acc_row(r, t.kk), 32 * t.wn + t.li, acc[r]);
}

// LayerNorm of the rows of `in` into `out` (both LDS tiles; zero in the padding); wavefront w owns rows w, w + 4, ...
// dst (M, D) or null: the rows in HBM as well.
template <int DP>
__device__ __forceinline__ void ln_rows(const float* in, float* out, const float* gamma, const float* beta, float eps, int r0,
                                        int M, int D, float* dst, float* stats, const Lane& t) {
  constexpr int TR = Tile<DP>::TR, LD = Tile<DP>::LD;
  const int c0 = t.lane, c1 = t.lane + 64;
  const bool k0 = c0 < D, k1 = c1 < D;
  const float g0 = k0 ? gamma[c0] : 0.f, g1 = k1 ? gamma[c1] : 0.f;
  const float b0 = k0 ? beta[c0] : 0.f, b1 = k1 ? beta[c1] : 0.f;
  const float inv = 1.f / (float)D;
  for (int r = t.w; r < TR; r += 4) {
    const int row = r0 + r;
    const float v0 = k0 ? in[r * LD + c0] : 0.f, v1 = k1 ? in[r * LD + c1] : 0.f;
    const float mean = wave_sum(v0 + v1) * inv;
    const float d0 = k0 ? v0 - mean : 0.f, d1 = k1 ? v1 - mean : 0.f;
    const float var = wave_sum(d0 * d0 + d1 * d1) * inv;
    const float rstd = 1.f / sqrtf(var + eps);
    const bool live = row < M;
    const float o0 = (k0 && live) ? fmaf(d0 * rstd, g0, b0) : 0.f, o1 = (k1 && live) ? fmaf(d1 * rstd, g1, b1) : 0.f;
    if (c0 < DP) out[r * LD + c0] = o0;
    if (c1 < DP) out[r * LD + c1] = o1;
    if (live) {
      if (dst) {
        if (k0) dst[(int64_t)row * D + c0] = o0;
        if (k1) dst[(int64_t)row * D + c1] = o1;
      }
      if (t.lane == 0) {
        stats[2 * (int64_t)row] = mean;
        stats[2 * (int64_t)row + 1] = rstd;
      }
    }
  }
}

// the rows' (mean, rstd) into LDS (0, 0 beyond M)
template <int TR>
__device__ __forceinline__ void load_stats(float* sm, float* sr, const float* stats, int r0, int M, int tid) {
  if (tid < TR) {
    const bool live = r0 + tid < M;
    sm[tid] = live ? stats[2 * (int64_t)(r0 + tid)] : 0.f;
    sr[tid] = live ? stats[2 * (int64_t)(r0 + tid) + 1] : 0.f;
  }
}

// part[0][c] = sum_r g[r][c] xhat[r][c], part[1][c] = sum_r g[r][c] over the tile's rows in ascending order; g an LDS tile of
// stride LD, xhat from the LayerNorm's input x (M, D) and the rows' statistics in LDS
static __device__ __forceinline__ void col_partials(const float* g, int LD, int TR, const float* x, const float* sm, const float* sr,
                                             int r0, int M, int D, float* part, int tid) {
  if (tid < D) {
    float gg = 0.f, gb = 0.f;
    for (int r = 0; r < TR && r0 + r < M; ++r) {
      const float gv = g[r * LD + tid];
      const float xh = (x[(int64_t)(r0 + r) * D + tid] - sm[r]) * sr[r];
      gg = fmaf(gv, xh, gg);
      gb += gv;
    }
    part[tid] = gg;
    part[D + tid] = gb;
  }
}

// LayerNorm backward of the rows: g (LDS tile, the gradient of the LayerNorm's output) -> out (LDS tile, the gradient of its
// input; zero in the padding).  g and out may be the same tile.
template <int DP>
__device__ __forceinline__ void ln_bwd_rows(const float* g, float* out, const float* x, const float* gamma, const float* sm,
                                            const float* sr, int r0, int M, int D, const Lane& t) {
  constexpr int TR = Tile<DP>::TR, LD = Tile<DP>::LD;
  const int c0 = t.lane, c1 = t.lane + 64;
  const bool k0 = c0 < D, k1 = c1 < D;
  const float g0 = k0 ? gamma[c0] : 0.f, g1 = k1 ? gamma[c1] : 0.f;
  const float inv = 1.f / (float)D;
  for (int r = t.w; r < TR; r += 4) {
    const int row = r0 + r;
    const bool live = row < M;
    const float mean = sm[r], rstd = sr[r];
    const float h0 = (k0 && live) ? (x[(int64_t)row * D + c0] - mean) * rstd : 0.f;
    const float h1 = (k1 && live) ? (x[(int64_t)row * D + c1] - mean) * rstd : 0.f;
    const float a0 = k0 ? g[r * LD + c0] * g0 : 0.f, a1 = k1 ? g[r * LD + c1] * g1 : 0.f;
    const float m1 = wave_sum(a0 + a1) * inv;
    const float m2 = wave_sum(a0 * h0 + a1 * h1) * inv;
    const float o0 = (k0 && live) ? rstd * (a0 - m1 - h0 * m2) : 0.f;
    const float o1 = (k1 && live) ? rstd * (a1 - m1 - h1 * m2) : 0.f;
    if (c0 < DP) out[r * LD + c0] = o0;
    if (c1 < DP) out[r * LD + c1] = o1;
  }
}
