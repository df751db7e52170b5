// SASRec's transformer block around the causal attention (include/rechub_hip.h, "SASRec"): the input stage, LayerNorm +
// in-projection, out-projection + LayerNorm + point-wise FFN, and the final LayerNorm with the two logit products.
//
// The two GEMM stages work on row tiles: a workgroup of four wavefronts owns TR rows padded to DP columns (D <= 64:
// DP = 64, TR = 64, wavefronts 2 x 2; D <= 128: DP = 128, TR = 32, wavefronts 1 x 4), so every wavefront holds ONE 32 x 32
// accumulator of v_mfma_f32_32x32x2_f32 (mfma_tile.h).  The activations of a tile stay in two LDS tiles (stride DP + 1)
// from the first product to the last; a weight matrix passes through LDS 32 reduction steps at a time (32 x (DP + 1)
// floats), never whole.  LDS per workgroup: DP = 64: 2 x 16.3 KiB + 8.1 KiB + statistics = 41 KiB; DP = 128: 2 x 16.1 KiB +
// 16.1 KiB = 49 KiB.  Rows beyond M and columns beyond D are held as zeros, so the products need no edge cases (an odd D
// meets a zero in the second half of its last 2-wide MFMA step).
//
// Reductions over rows ((g_gamma, g_beta) of the LayerNorms) are one partial per workgroup, summed over the tile's rows in
// ascending order by one thread per column; the host sums the partials with rh_colsum.  The D x D weight gradients are not
// formed here: the backward kernels emit their operands and rh_linear_wgrad (split-batch MFMA, fixed-order reduction)
// forms them.
#include "mfma_tile.h"

namespace {

constexpr int kMaxD = RH_SASREC_MAX_D;
constexpr int kKC = 32;    // reduction steps of a weight matrix held in LDS at a time
constexpr int kHR = 64;    // rows per workgroup of the head's backward

// ---------------------------------------------------------------------------------------------------------------------
// input stage
struct InArgs {
  const int64_t* seq;
  const float* e;
  int64_t e_bs, e_rs;
  const float* P;
  const float* g_x0;
  const int64_t* rng;
  int64_t* saved_ctr;
  float* x0;
  float* g_e;
  float* g_P;
  int B, L, D, max_len;
  float scale, p;
};

__global__ __launch_bounds__(RH_BLOCK) void input_fwd_kernel(const InArgs a) {
  const DropKey dk = drop_key(a.p, a.rng, a.saved_ctr, 1);
  if (a.p > 0.f && blockIdx.x == 0 && threadIdx.x == 0) a.saved_ctr[0] = (int64_t)dk.ctr;
  const int64_t n = (int64_t)a.B * a.L * a.D;
  for (int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * RH_BLOCK) {
    const int64_t row = i / a.D;
    const int d = (int)(i % a.D), l = (int)(row % a.L);
    const int64_t b = row / a.L;
    float v = 0.f;
    if (a.seq[row] != 0) v = (a.e[b * a.e_bs + l * a.e_rs + d] * a.scale + a.P[l * a.D + d]) * drop_mul(a.p, dk, i);
    a.x0[i] = v;
  }
}

// one thread per (l, d) of the position table walks the samples in ascending order
__global__ __launch_bounds__(RH_BLOCK) void input_bwd_kernel(const InArgs a) {
  const DropKey dk = drop_key(a.p, a.rng, a.saved_ctr, 0);
  const int n = a.max_len * a.D;
  for (int i = blockIdx.x * RH_BLOCK + threadIdx.x; i < n; i += gridDim.x * RH_BLOCK) {
    const int l = i / a.D, d = i % a.D;
    float sum = 0.f;
    if (l < a.L) {
      for (int b = 0; b < a.B; ++b) {
        const int64_t row = (int64_t)b * a.L + l, idx = row * a.D + d;
        float g = 0.f;
        if (a.seq[row] != 0) g = a.g_x0[idx] * drop_mul(a.p, dk, idx);
        a.g_e[idx] = g * a.scale;
        sum += g;
      }
    }
    a.g_P[i] = sum;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// tile helpers
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
__device__ __forceinline__ v16f tile_gemm(v16f acc, const float* A, const float* W, int ldw, int K, int N, float* wl,
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
      if (k0) dst[(int64_t)row * D + c0] = o0;
      if (k1) dst[(int64_t)row * D + c1] = o1;
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
__device__ __forceinline__ void col_partials(const float* g, int LD, int TR, const float* x, const float* sm, const float* sr,
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

// ---------------------------------------------------------------------------------------------------------------------
// LayerNorm + in-projection
struct AttnArgs {
  const float* x;
  const float* gamma;
  const float* beta;
  const float* w;
  const float* b;
  const float* stats_in;
  const float* g_qkv;
  const float* g_Q;
  float* Q;
  float* qkv;
  float* stats;
  float* g_x;
  float* part;
  int M, D;
  float eps;
};

template <int DP>
__global__ __launch_bounds__(RH_BLOCK) void attn_in_fwd_kernel(const AttnArgs a) {
  constexpr int TR = Tile<DP>::TR, LD = Tile<DP>::LD;
  __shared__ float s0[TR * LD], s1[TR * LD], wl[kKC * LD];
  const Lane t = lane_of<DP>();
  const int r0 = blockIdx.x * TR, M = a.M, D = a.D;
  load_rows<DP>(s0, a.x, D, r0, M, D, t.tid);
  __syncthreads();
  ln_rows<DP>(s0, s1, a.gamma, a.beta, a.eps, r0, M, D, a.Q, a.stats, t);
  for (int j = 0; j < 3; ++j) {
    const v16f acc = tile_gemm<DP, true>(zero16(), j == 0 ? s1 : s0, a.w + (int64_t)j * D * D, D, D, D, wl, t);
    for_acc(acc, t, [&](int r, int c, float v) {
      if (r0 + r < M && c < D) a.qkv[(int64_t)(r0 + r) * 3 * D + j * D + c] = v + a.b[j * D + c];
    });
  }
}

template <int DP>
__global__ __launch_bounds__(RH_BLOCK) void attn_in_bwd_kernel(const AttnArgs a) {
  constexpr int TR = Tile<DP>::TR, LD = Tile<DP>::LD;
  __shared__ float s0[TR * LD], s1[TR * LD], wl[kKC * LD], sm[TR], sr[TR];
  const Lane t = lane_of<DP>();
  const int r0 = blockIdx.x * TR, M = a.M, D = a.D;
  load_stats<TR>(sm, sr, a.stats_in, r0, M, t.tid);
  load_rows<DP>(s0, a.g_qkv, 3 * D, r0, M, D, t.tid);
  // g of the LayerNorm's output: the residual's plus g_q Wq
  v16f acc = tile_gemm<DP, false>(zero16(), s0, a.w, D, D, D, wl, t);
  for_acc(acc, t, [&](int r, int c, float v) {
    s1[r * LD + c] = (r0 + r < M && c < D) ? v + a.g_Q[(int64_t)(r0 + r) * D + c] : 0.f;
  });
  __syncthreads();
  col_partials(s1, LD, TR, a.x, sm, sr, r0, M, D, a.part + (int64_t)blockIdx.x * 2 * D, t.tid);
  __syncthreads();
  ln_bwd_rows<DP>(s1, s1, a.x, a.gamma, sm, sr, r0, M, D, t);
  // + g_k Wk + g_v Wv
  acc = zero16();
  for (int j = 1; j < 3; ++j) {
    __syncthreads();  // (the previous product has read s0)
    load_rows<DP>(s0, a.g_qkv + j * D, 3 * D, r0, M, D, t.tid);
    acc = tile_gemm<DP, false>(acc, s0, a.w + (int64_t)j * D * D, D, D, D, wl, t);
  }
  for_acc(acc, t, [&](int r, int c, float v) {
    if (r0 + r < M && c < D) a.g_x[(int64_t)(r0 + r) * D + c] = v + s1[r * LD + c];
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// out-projection + residual + LayerNorm + point-wise FFN + mask
struct FfnArgs {
  const float* attn;
  const float* Q;
  const int64_t* seq;
  const float* wo;
  const float* bo;
  const float* gamma;
  const float* beta;
  const float* w1;
  const float* b1;
  const float* w2;
  const float* b2;
  const int64_t* rng;
  int64_t* saved_ctr;
  float* y;
  float* z;
  float* a;
  float* stats;
  float* out;
  const float* g_out;
  float* g_f;
  float* g_h;
  float* g_Q;
  float* g_attn;
  float* part;
  int M, D;
  float eps, p;
};

template <int DP>
__global__ __launch_bounds__(RH_BLOCK) void ffn_fwd_kernel(const FfnArgs a) {
  constexpr int TR = Tile<DP>::TR, LD = Tile<DP>::LD;
  __shared__ float s0[TR * LD], s1[TR * LD], wl[kKC * LD];
  const Lane t = lane_of<DP>();
  const int r0 = blockIdx.x * TR, M = a.M, D = a.D;
  const int64_t MD = (int64_t)M * D;
  const DropKey dk = drop_key(a.p, a.rng, a.saved_ctr, 1);
  if (a.p > 0.f && blockIdx.x == 0 && t.tid == 0) a.saved_ctr[0] = (int64_t)dk.ctr;
  load_rows<DP>(s0, a.attn, D, r0, M, D, t.tid);
  v16f acc = tile_gemm<DP, true>(zero16(), s0, a.wo, D, D, D, wl, t);
  for_acc(acc, t, [&](int r, int c, float v) {
    const bool ok = r0 + r < M && c < D;
    const int64_t i = (int64_t)(r0 + r) * D + c;
    const float yv = ok ? v + a.bo[c] + a.Q[i] : 0.f;
    s1[r * LD + c] = yv;
    if (ok) a.y[i] = yv;
  });
  __syncthreads();
  ln_rows<DP>(s1, s0, a.gamma, a.beta, a.eps, r0, M, D, a.z, a.stats, t);  // (the first product is done with s0)
  acc = tile_gemm<DP, true>(zero16(), s0, a.w1, D, D, D, wl, t);
  for_acc(acc, t, [&](int r, int c, float v) {
    const bool ok = r0 + r < M && c < D;
    const int64_t i = (int64_t)(r0 + r) * D + c;
    const float av = ok ? fmaxf((v + a.b1[c]) * drop_mul(a.p, dk, (uint64_t)i), 0.f) : 0.f;
    s1[r * LD + c] = av;
    if (ok) a.a[i] = av;
  });
  acc = tile_gemm<DP, true>(zero16(), s1, a.w2, D, D, D, wl, t);
  for_acc(acc, t, [&](int r, int c, float v) {
    if (r0 + r < M && c < D) {
      const int64_t i = (int64_t)(r0 + r) * D + c;
      const float f = (v + a.b2[c]) * drop_mul(a.p, dk, (uint64_t)(MD + i));
      a.out[i] = a.seq[r0 + r] != 0 ? s0[r * LD + c] + f : 0.f;
    }
  });
}

template <int DP>
__global__ __launch_bounds__(RH_BLOCK) void ffn_bwd_kernel(const FfnArgs a) {
  constexpr int TR = Tile<DP>::TR, LD = Tile<DP>::LD;
  __shared__ float s0[TR * LD], s1[TR * LD], wl[kKC * LD], sm[TR], sr[TR];
  const Lane t = lane_of<DP>();
  const int r0 = blockIdx.x * TR, M = a.M, D = a.D;
  const int64_t MD = (int64_t)M * D;
  const DropKey dk = drop_key(a.p, a.rng, a.saved_ctr, 0);
  load_stats<TR>(sm, sr, a.stats, r0, M, t.tid);
  // g_f = the gradient of a W2^T + b2: mask, dropout2
  for (int e = t.tid; e < TR * DP; e += RH_BLOCK) {
    const int r = e / DP, c = e % DP;
    float v = 0.f;
    if (r0 + r < M && c < D) {
      const int64_t i = (int64_t)(r0 + r) * D + c;
      if (a.seq[r0 + r] != 0) v = a.g_out[i] * drop_mul(a.p, dk, (uint64_t)(MD + i));
      a.g_f[i] = v;
    }
    s0[r * LD + c] = v;
  }
  // g_h = the gradient of z W1^T + b1: g_f W2 through the ReLU and dropout1 (a > 0 exactly where both let it pass)
  v16f acc = tile_gemm<DP, false>(zero16(), s0, a.w2, D, D, D, wl, t);
  for_acc(acc, t, [&](int r, int c, float v) {
    const bool ok = r0 + r < M && c < D;
    const int64_t i = (int64_t)(r0 + r) * D + c;
    const float gh = (ok && a.a[i] > 0.f) ? v * dk.keep : 0.f;
    s1[r * LD + c] = gh;
    if (ok) a.g_h[i] = gh;
  });
  // g_z = g_h W1 + the residual's (the masked g_out)
  acc = tile_gemm<DP, false>(zero16(), s1, a.w1, D, D, D, wl, t);
  for_acc(acc, t, [&](int r, int c, float v) {
    const bool ok = r0 + r < M && c < D;
    float gz = 0.f;
    if (ok) gz = v + (a.seq[r0 + r] != 0 ? a.g_out[(int64_t)(r0 + r) * D + c] : 0.f);
    s0[r * LD + c] = gz;
  });
  __syncthreads();
  col_partials(s0, LD, TR, a.y, sm, sr, r0, M, D, a.part + (int64_t)blockIdx.x * 2 * D, t.tid);
  ln_bwd_rows<DP>(s0, s1, a.y, a.gamma, sm, sr, r0, M, D, t);  // g_y (the second product is done with s1)
  __syncthreads();
  for (int e = t.tid; e < TR * D; e += RH_BLOCK) {
    const int r = e / D, c = e % D;
    if (r0 + r < M) a.g_Q[(int64_t)(r0 + r) * D + c] = s1[r * LD + c];
  }
  acc = tile_gemm<DP, false>(zero16(), s1, a.wo, D, D, D, wl, t);
  for_acc(acc, t, [&](int r, int c, float v) {
    if (r0 + r < M && c < D) a.g_attn[(int64_t)(r0 + r) * D + c] = v;
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// final LayerNorm + the two logit products
struct HeadArgs {
  const float* x;
  const float* gamma;
  const float* beta;
  const float* pos_e;
  const float* neg_e;
  int64_t pos_bs, neg_bs, e_rs;
  const float* stats_in;
  const float* g_s;
  const float* g_pos;
  const float* g_neg;
  float* s;
  float* pos_logit;
  float* neg_logit;
  float* stats;
  float* g_x;
  float* g_pos_e;
  float* g_neg_e;
  float* part;
  int B, L, D;
  float eps;
};

// one wavefront per row
__global__ __launch_bounds__(RH_BLOCK) void head_fwd_kernel(const HeadArgs a) {
  const int lane = threadIdx.x % RH_WAVE, w = threadIdx.x / RH_WAVE, D = a.D;
  const int64_t M = (int64_t)a.B * a.L, row = (int64_t)blockIdx.x * 4 + w;
  if (row >= M) return;
  const int c0 = lane, c1 = lane + 64;
  const bool k0 = c0 < D, k1 = c1 < D;
  const float inv = 1.f / (float)D;
  const float v0 = k0 ? a.x[row * D + c0] : 0.f, v1 = k1 ? a.x[row * D + c1] : 0.f;
  const float mean = wave_sum(v0 + v1) * inv;
  const float d0 = k0 ? v0 - mean : 0.f, d1 = k1 ? v1 - mean : 0.f;
  const float var = wave_sum(d0 * d0 + d1 * d1) * inv;
  const float rstd = 1.f / sqrtf(var + a.eps);
  const float o0 = k0 ? fmaf(d0 * rstd, a.gamma[c0], a.beta[c0]) : 0.f;
  const float o1 = k1 ? fmaf(d1 * rstd, a.gamma[c1], a.beta[c1]) : 0.f;
  if (a.s) {
    if (k0) a.s[row * D + c0] = o0;
    if (k1) a.s[row * D + c1] = o1;
  }
  if (lane == 0) {
    a.stats[2 * row] = mean;
    a.stats[2 * row + 1] = rstd;
  }
  if (a.pos_e) {
    const int64_t b = row / a.L, off = (row % a.L) * a.e_rs;
    const float* pe = a.pos_e + b * a.pos_bs + off;
    const float* ne = a.neg_e + b * a.neg_bs + off;
    const float ps = wave_sum((k0 ? o0 * pe[c0] : 0.f) + (k1 ? o1 * pe[c1] : 0.f));
    const float ns = wave_sum((k0 ? o0 * ne[c0] : 0.f) + (k1 ? o1 * ne[c1] : 0.f));
    if (lane == 0) {
      a.pos_logit[row] = ps;
      a.neg_logit[row] = ns;
    }
  }
}

// kHR rows per workgroup, wavefront w owns rows w, w + 4, ...
__global__ __launch_bounds__(RH_BLOCK) void head_bwd_kernel(const HeadArgs a) {
  constexpr int LD = kMaxD + 1;
  __shared__ float gs[kHR * LD], sm[kHR], sr[kHR];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE, D = a.D;
  const int64_t M = (int64_t)a.B * a.L, r0 = (int64_t)blockIdx.x * kHR;
  const int c0 = lane, c1 = lane + 64;
  const bool k0 = c0 < D, k1 = c1 < D;
  const float inv = 1.f / (float)D;
  const float ga0 = k0 ? a.gamma[c0] : 0.f, ga1 = k1 ? a.gamma[c1] : 0.f;
  const float be0 = k0 ? a.beta[c0] : 0.f, be1 = k1 ? a.beta[c1] : 0.f;
  for (int r = w; r < kHR; r += 4) {
    const int64_t row = r0 + r;
    if (row >= M) break;  // (wavefront-uniform)
    const float mean = a.stats_in[2 * row], rstd = a.stats_in[2 * row + 1];
    const float h0 = k0 ? (a.x[row * D + c0] - mean) * rstd : 0.f, h1 = k1 ? (a.x[row * D + c1] - mean) * rstd : 0.f;
    float g0 = 0.f, g1 = 0.f;
    if (a.g_s) {
      g0 = k0 ? a.g_s[row * D + c0] : 0.f;
      g1 = k1 ? a.g_s[row * D + c1] : 0.f;
    }
    if (a.pos_e) {
      const int64_t b = row / a.L, off = (row % a.L) * a.e_rs;
      const float* pe = a.pos_e + b * a.pos_bs + off;
      const float* ne = a.neg_e + b * a.neg_bs + off;
      const float gp = a.g_pos[row], gn = a.g_neg[row];
      const float s0 = fmaf(h0, ga0, be0), s1 = fmaf(h1, ga1, be1);
      if (k0) {
        g0 += gp * pe[c0] + gn * ne[c0];
        a.g_pos_e[row * D + c0] = gp * s0;
        a.g_neg_e[row * D + c0] = gn * s0;
      }
      if (k1) {
        g1 += gp * pe[c1] + gn * ne[c1];
        a.g_pos_e[row * D + c1] = gp * s1;
        a.g_neg_e[row * D + c1] = gn * s1;
      }
    }
    const float a0 = g0 * ga0, a1 = g1 * ga1;
    const float m1 = wave_sum(a0 + a1) * inv;
    const float m2 = wave_sum(a0 * h0 + a1 * h1) * inv;
    if (k0) a.g_x[row * D + c0] = rstd * (a0 - m1 - h0 * m2);
    if (k1) a.g_x[row * D + c1] = rstd * (a1 - m1 - h1 * m2);
    if (k0) gs[r * LD + c0] = g0;
    if (k1) gs[r * LD + c1] = g1;
    if (lane == 0) {
      sm[r] = mean;
      sr[r] = rstd;
    }
  }
  __syncthreads();
  const int rows = (int)(M - r0 < kHR ? M - r0 : kHR);
  col_partials(gs, LD, rows, a.x + r0 * D, sm, sr, 0, rows, D, a.part + (int64_t)blockIdx.x * 2 * D, tid);
}

int check_md(const char* name, int64_t M, int D) {
  RH_REQUIRE(D >= 1 && D <= kMaxD, RH_E_UNSUPPORTED, "%s: width %d unsupported (1 <= D <= %d)", name, D, kMaxD);
  RH_REQUIRE(M >= 0 && M <= 0x7FFFFFFF - 64, RH_E_UNSUPPORTED, "%s: %lld rows unsupported", name, (long long)M);
  return 0;
}

int check_drop(const char* name, float p, const void* rng, const void* saved_ctr) {
  RH_REQUIRE(p >= 0.f && p < 1.f, RH_E_BADARG, "%s: dropout p=%g outside [0, 1)", name, (double)p);
  RH_REQUIRE(p == 0.f || (rng && saved_ctr), RH_E_BADARG, "%s: dropout without its (seed, counter) state", name);
  return 0;
}

int tiles_of(int M, int D) { return D <= 64 ? (M + 63) / 64 : (M + 31) / 32; }

}  // namespace

#define RH_SASREC_LAUNCH(kernel, D, grid, st, args)                                         \
  do {                                                                                      \
    if ((D) <= 64)                                                                          \
      hipLaunchKernelGGL(kernel<64>, dim3(grid), dim3(RH_BLOCK), 0, st, args);              \
    else                                                                                    \
      hipLaunchKernelGGL(kernel<128>, dim3(grid), dim3(RH_BLOCK), 0, st, args);             \
  } while (0)

extern "C" int rh_sasrec_ntiles(int M, int D, int* ntiles) {
  RH_REQUIRE(ntiles, RH_E_BADARG, "rh_sasrec_ntiles: null pointer");
  if (int rc = check_md("rh_sasrec_ntiles", M, D)) return rc;
  *ntiles = tiles_of(M, D);
  return 0;
}

extern "C" int rh_sasrec_input_fwd(const int64_t* seq, const float* e, int64_t e_bstride, int64_t e_rstride, const float* P,
                                   int B, int L, int D, int max_len, float scale, float p_drop, int64_t* rng, int64_t* saved_ctr, float* x0,
                                   void* stream) {
  RH_REQUIRE(B >= 0 && L >= 0, RH_E_BADARG, "rh_sasrec_input_fwd: negative size");
  if (int rc = check_md("rh_sasrec_input_fwd", (int64_t)B * L, D)) return rc;
  RH_REQUIRE(L <= max_len, RH_E_UNSUPPORTED, "rh_sasrec_input_fwd: L=%d exceeds max_len=%d", L, max_len);
  if (int rc = check_drop("rh_sasrec_input_fwd", p_drop, rng, saved_ctr)) return rc;
  RH_REQUIRE(seq && e && P && x0, RH_E_BADARG, "rh_sasrec_input_fwd: null pointer");
  RH_REQUIRE(e_rstride >= D && e_bstride >= (int64_t)L * e_rstride, RH_E_BADARG,
             "rh_sasrec_input_fwd: strides %lld, %lld too small", (long long)e_bstride, (long long)e_rstride);
  if ((int64_t)B * L == 0) return 0;
  InArgs a{};
  a.seq = seq;
  a.e = e;
  a.e_bs = e_bstride;
  a.e_rs = e_rstride;
  a.P = P;
  a.rng = rng;
  a.saved_ctr = saved_ctr;
  a.x0 = x0;
  a.B = B;
  a.L = L;
  a.D = D;
  a.max_len = max_len;
  a.scale = scale;
  a.p = p_drop;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)B * L * D;
  int64_t grid = (n + RH_BLOCK - 1) / RH_BLOCK;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(input_fwd_kernel, dim3((unsigned)grid), dim3(RH_BLOCK), 0, st, a);
  if (p_drop > 0.f) hipLaunchKernelGGL(drop_advance_kernel, dim3(1), dim3(1), 0, st, rng);
  RH_LAUNCH_CHECK("rh_sasrec_input_fwd");
  return 0;
}

extern "C" int rh_sasrec_input_bwd(const int64_t* seq, const float* g_x0, int B, int L, int D, int max_len, float scale,
                                   float p_drop, const int64_t* rng, const int64_t* saved_ctr, float* g_e, float* g_P,
                                   void* stream) {
  RH_REQUIRE(B >= 0 && L >= 0 && max_len >= 1, RH_E_BADARG, "rh_sasrec_input_bwd: bad size");
  if (int rc = check_md("rh_sasrec_input_bwd", (int64_t)B * L, D)) return rc;
  RH_REQUIRE(L <= max_len, RH_E_UNSUPPORTED, "rh_sasrec_input_bwd: L=%d exceeds max_len=%d", L, max_len);
  if (int rc = check_drop("rh_sasrec_input_bwd", p_drop, rng, saved_ctr)) return rc;
  RH_REQUIRE(seq && g_x0 && g_e && g_P, RH_E_BADARG, "rh_sasrec_input_bwd: null pointer");
  InArgs a{};
  a.seq = seq;
  a.g_x0 = g_x0;
  a.rng = rng;
  a.saved_ctr = const_cast<int64_t*>(saved_ctr);
  a.g_e = g_e;
  a.g_P = g_P;
  a.B = B;
  a.L = L;
  a.D = D;
  a.max_len = max_len;
  a.scale = scale;
  a.p = p_drop;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int n = max_len * D;
  hipLaunchKernelGGL(input_bwd_kernel, dim3((n + RH_BLOCK - 1) / RH_BLOCK), dim3(RH_BLOCK), 0, st, a);
  RH_LAUNCH_CHECK("rh_sasrec_input_bwd");
  return 0;
}

extern "C" int rh_sasrec_attn_in_fwd(const float* x, const float* gamma, const float* beta, float eps, const float* w,
                                     const float* b, int M, int D, float* Q, float* qkv, float* stats, void* stream) {
  if (int rc = check_md("rh_sasrec_attn_in_fwd", M, D)) return rc;
  RH_REQUIRE(x && gamma && beta && w && b && Q && qkv && stats, RH_E_BADARG, "rh_sasrec_attn_in_fwd: null pointer");
  if (M == 0) return 0;
  AttnArgs a{};
  a.x = x;
  a.gamma = gamma;
  a.beta = beta;
  a.w = w;
  a.b = b;
  a.Q = Q;
  a.qkv = qkv;
  a.stats = stats;
  a.M = M;
  a.D = D;
  a.eps = eps;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  RH_SASREC_LAUNCH(attn_in_fwd_kernel, D, tiles_of(M, D), st, a);
  RH_LAUNCH_CHECK("rh_sasrec_attn_in_fwd");
  return 0;
}

extern "C" int rh_sasrec_attn_in_bwd(const float* x, const float* gamma, const float* w, const float* stats,
                                     const float* g_qkv, const float* g_Q, int M, int D, float* g_x, float* part,
                                     void* stream) {
  if (int rc = check_md("rh_sasrec_attn_in_bwd", M, D)) return rc;
  RH_REQUIRE(x && gamma && w && stats && g_qkv && g_Q && g_x && part, RH_E_BADARG, "rh_sasrec_attn_in_bwd: null pointer");
  if (M == 0) return 0;
  AttnArgs a{};
  a.x = x;
  a.gamma = gamma;
  a.w = w;
  a.stats_in = stats;
  a.g_qkv = g_qkv;
  a.g_Q = g_Q;
  a.g_x = g_x;
  a.part = part;
  a.M = M;
  a.D = D;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  RH_SASREC_LAUNCH(attn_in_bwd_kernel, D, tiles_of(M, D), st, a);
  RH_LAUNCH_CHECK("rh_sasrec_attn_in_bwd");
  return 0;
}

extern "C" int rh_sasrec_ffn_fwd(const float* attn, const float* Q, const int64_t* seq, const float* wo, const float* bo,
                                 const float* gamma, const float* beta, float eps, const float* w1, const float* b1,
                                 const float* w2, const float* b2, int M, int D, float p_drop, int64_t* rng,
                                 int64_t* saved_ctr, float* y, float* z, float* a_out, float* stats, float* out,
                                 void* stream) {
  if (int rc = check_md("rh_sasrec_ffn_fwd", M, D)) return rc;
  if (int rc = check_drop("rh_sasrec_ffn_fwd", p_drop, rng, saved_ctr)) return rc;
  RH_REQUIRE(attn && Q && seq && wo && bo && gamma && beta && w1 && b1 && w2 && b2 && y && z && a_out && stats && out,
             RH_E_BADARG, "rh_sasrec_ffn_fwd: null pointer");
  if (M == 0) return 0;
  FfnArgs a{};
  a.attn = attn;
  a.Q = Q;
  a.seq = seq;
  a.wo = wo;
  a.bo = bo;
  a.gamma = gamma;
  a.beta = beta;
  a.w1 = w1;
  a.b1 = b1;
  a.w2 = w2;
  a.b2 = b2;
  a.rng = rng;
  a.saved_ctr = saved_ctr;
  a.y = y;
  a.z = z;
  a.a = a_out;
  a.stats = stats;
  a.out = out;
  a.M = M;
  a.D = D;
  a.eps = eps;
  a.p = p_drop;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  RH_SASREC_LAUNCH(ffn_fwd_kernel, D, tiles_of(M, D), st, a);
  if (p_drop > 0.f) hipLaunchKernelGGL(drop_advance_kernel, dim3(1), dim3(1), 0, st, rng);
  RH_LAUNCH_CHECK("rh_sasrec_ffn_fwd");
  return 0;
}

extern "C" int rh_sasrec_ffn_bwd(const int64_t* seq, const float* wo, const float* gamma, const float* w1, const float* w2,
                                 const float* y, const float* a_in, const float* stats, const float* g_out, int M, int D,
                                 float p_drop, const int64_t* rng, const int64_t* saved_ctr, float* g_f, float* g_h,
                                 float* g_Q, float* g_attn, float* part, void* stream) {
  if (int rc = check_md("rh_sasrec_ffn_bwd", M, D)) return rc;
  if (int rc = check_drop("rh_sasrec_ffn_bwd", p_drop, rng, saved_ctr)) return rc;
  RH_REQUIRE(seq && wo && gamma && w1 && w2 && y && a_in && stats && g_out && g_f && g_h && g_Q && g_attn && part,
             RH_E_BADARG, "rh_sasrec_ffn_bwd: null pointer");
  if (M == 0) return 0;
  FfnArgs a{};
  a.seq = seq;
  a.wo = wo;
  a.gamma = gamma;
  a.w1 = w1;
  a.w2 = w2;
  a.rng = rng;
  a.saved_ctr = const_cast<int64_t*>(saved_ctr);
  a.y = const_cast<float*>(y);
  a.a = const_cast<float*>(a_in);
  a.stats = const_cast<float*>(stats);
  a.g_out = g_out;
  a.g_f = g_f;
  a.g_h = g_h;
  a.g_Q = g_Q;
  a.g_attn = g_attn;
  a.part = part;
  a.M = M;
  a.D = D;
  a.p = p_drop;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  RH_SASREC_LAUNCH(ffn_bwd_kernel, D, tiles_of(M, D), st, a);
  RH_LAUNCH_CHECK("rh_sasrec_ffn_bwd");
  return 0;
}

namespace {
int head_check(const char* name, int B, int L, int D, const void* pos_e, int64_t pos_bs, const void* neg_e, int64_t neg_bs,
               int64_t rs) {
  RH_REQUIRE(B >= 0 && L >= 0, RH_E_BADARG, "%s: negative size", name);
  if (int rc = check_md(name, (int64_t)B * L, D)) return rc;
  RH_REQUIRE((pos_e == nullptr) == (neg_e == nullptr), RH_E_BADARG, "%s: pos_e and neg_e come together", name);
  RH_REQUIRE(!pos_e || (rs >= D && pos_bs >= (int64_t)L * rs && neg_bs >= (int64_t)L * rs), RH_E_BADARG,
             "%s: strides too small", name);
  return 0;
}
}  // namespace

extern "C" int rh_sasrec_head_fwd(const float* x, const float* gamma, const float* beta, float eps, const float* pos_e,
                                  int64_t pos_bstride, const float* neg_e, int64_t neg_bstride, int64_t e_rstride, int B, int L,
                                  int D, float* s, float* pos_logit, float* neg_logit, float* stats, void* stream) {
  if (int rc = head_check("rh_sasrec_head_fwd", B, L, D, pos_e, pos_bstride, neg_e, neg_bstride, e_rstride)) return rc;
  RH_REQUIRE(x && gamma && beta && stats && (pos_e ? (pos_logit && neg_logit) : s != nullptr), RH_E_BADARG,
             "rh_sasrec_head_fwd: null pointer");
  const int64_t M = (int64_t)B * L;
  if (M == 0) return 0;
  HeadArgs a{};
  a.x = x;
  a.gamma = gamma;
  a.beta = beta;
  a.pos_e = pos_e;
  a.neg_e = neg_e;
  a.pos_bs = pos_bstride;
  a.neg_bs = neg_bstride;
  a.e_rs = e_rstride;
  a.s = s;
  a.pos_logit = pos_logit;
  a.neg_logit = neg_logit;
  a.stats = stats;
  a.B = B;
  a.L = L;
  a.D = D;
  a.eps = eps;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(head_fwd_kernel, dim3((unsigned)((M + 3) / 4)), dim3(RH_BLOCK), 0, st, a);
  RH_LAUNCH_CHECK("rh_sasrec_head_fwd");
  return 0;
}

extern "C" int rh_sasrec_head_bwd(const float* x, const float* gamma, const float* beta, const float* stats,
                                  const float* pos_e, int64_t pos_bstride, const float* neg_e, int64_t neg_bstride,
                                  int64_t e_rstride, const float* g_s, const float* g_pos, const float* g_neg, int B, int L,
                                  int D, float* g_x, float* g_pos_e, float* g_neg_e, float* part, void* stream) {
  if (int rc = head_check("rh_sasrec_head_bwd", B, L, D, pos_e, pos_bstride, neg_e, neg_bstride, e_rstride)) return rc;
  RH_REQUIRE(x && gamma && beta && stats && g_x && part && (pos_e ? (g_pos && g_neg && g_pos_e && g_neg_e) : g_s != nullptr),
             RH_E_BADARG, "rh_sasrec_head_bwd: null pointer");
  const int64_t M = (int64_t)B * L;
  if (M == 0) return 0;
  HeadArgs a{};
  a.x = x;
  a.gamma = gamma;
  a.beta = beta;
  a.stats_in = stats;
  a.pos_e = pos_e;
  a.neg_e = neg_e;
  a.pos_bs = pos_bstride;
  a.neg_bs = neg_bstride;
  a.e_rs = e_rstride;
  a.g_s = g_s;
  a.g_pos = g_pos;
  a.g_neg = g_neg;
  a.g_x = g_x;
  a.g_pos_e = g_pos_e;
  a.g_neg_e = g_neg_e;
  a.part = part;
  a.B = B;
  a.L = L;
  a.D = D;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(head_bwd_kernel, dim3((unsigned)((M + kHR - 1) / kHR)), dim3(RH_BLOCK), 0, st, a);
  RH_LAUNCH_CHECK("rh_sasrec_head_bwd");
  return 0;
}
