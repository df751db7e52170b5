// The post-norm transformer encoder block after attention (include/rechub_hip.h, "encoder block"): out-projection +
// residual + LayerNorm + a WIDE feed-forward (hidden width F >> D) + residual + LayerNorm.
//
// The hidden never reaches HBM.  A workgroup owns one row tile (row_tile.h: TR x DP) and walks F in chunks of DP columns:
// one MFMA product forms the chunk of u = x1 W1^T from the x1 tile in LDS, bias, LeakyReLU and dropout are applied to the
// accumulator in registers, the chunk of a goes to a second LDS tile, and a second product adds its contribution
// a_chunk W2_chunk^T to the (TR, DP) accumulator of the feed-forward's output, which stays in registers across the loop.
// The weight chunks pass through LDS kKC reduction steps at a time.  Dynamic LDS per workgroup (DP = 64 | 128):
//   forward          2 tiles + the weight stage                     41 | 49 KiB
//   backward, rows   3 tiles + the weight stage + statistics        58 | 66 KiB
//   backward, weights 4 tiles + the weight stage + statistics       75 | 82 KiB
// so two workgroups share a CU's 160 KiB everywhere but in the weight kernel at D > 64.
//
// The backward recomputes the hidden, chunk by chunk, twice: enc_bwd_rows_kernel (one workgroup per row tile, all chunks)
// for the gradients that are sums over F, enc_bwd_weights_kernel (one workgroup per (chunk, row split), the split's row
// tiles in ascending order) for the gradients that are sums over rows, held in registers across the tiles and written
// once as the split's partial.  No atomics anywhere.
#include "row_tile.h"

namespace {

constexpr int kMaxD = RH_SASREC_MAX_D;   // the row tile's widest form
constexpr int kWeightGrid = 256;         // workgroups the weight kernel aims for: one per CU

struct EncArgs {
  const float* attn;
  const float* x;
  int64_t ldx;
  const float* wo;
  const float* bo;
  const float* gamma1;
  const float* beta1;
  const float* w1;
  const float* b1;
  const float* w2;
  const float* b2;
  const float* gamma2;
  const float* beta2;
  const int64_t* rng;
  int64_t* saved_ctr;
  float* y1;
  float* y2;
  float* stats1;
  float* stats2;
  float* out;
  const float* g_out;
  float* g_f;
  float* g_o;
  float* g_x;
  float* g_attn;
  float* part;
  float* wpart;
  int M, D, F, tiles_per_split;
  float eps1, eps2, slope, p;
};

template <int DP>
constexpr size_t lds_bytes(int tiles, int stat_vectors) {
  return sizeof(float) * (size_t)(tiles * Tile<DP>::TR * Tile<DP>::LD + kKC * Tile<DP>::LD + stat_vectors * Tile<DP>::TR);
}

// x1 = LN1(y1) of the tile's rows from the saved statistics, with the forward's own operations (hence its bits)
template <int DP>
__device__ __forceinline__ void recompute_x1(float* s, const EncArgs& a, const float* sm, const float* sr, int r0, int tid) {
  constexpr int TR = Tile<DP>::TR, LD = Tile<DP>::LD;
  for (int e = tid; e < TR * DP; e += RH_BLOCK) {
    const int r = e / DP, c = e % DP;
    float v = 0.f;
    if (r0 + r < a.M && c < a.D)
      v = fmaf((a.y1[(int64_t)(r0 + r) * a.D + c] - sm[r]) * sr[r], a.gamma1[c], a.beta1[c]);
    s[r * LD + c] = v;
  }
}

template <int DP>
__global__ __launch_bounds__(RH_BLOCK) void enc_fwd_kernel(const EncArgs a) {
  constexpr int TR = Tile<DP>::TR, LD = Tile<DP>::LD;
  extern __shared__ float lds[];
  float* s0 = lds;
  float* s1 = s0 + TR * LD;
  float* wl = s1 + TR * LD;
  const Lane t = lane_of<DP>();
  const int r0 = blockIdx.x * TR, M = a.M, D = a.D, F = a.F;
  const uint64_t MD = (uint64_t)M * D, MF = (uint64_t)M * F;
  const DropKey dk = drop_key(a.p, a.rng, a.saved_ctr, 1);
  if (a.p > 0.f && blockIdx.x == 0 && t.tid == 0) a.saved_ctr[0] = (int64_t)dk.ctr;
  // y1 = x + drop_o(attn Wo^T + bo)
  load_rows<DP>(s0, a.attn, D, r0, M, D, t.tid);
  v16f acc = tile_gemm<DP, true>(zero16(), s0, a.wo, D, D, D, wl, t);
  for_acc(acc, t, [&](int r, int c, float v) {
    const int64_t row = r0 + r;
    float yv = 0.f;
    if (row < M && c < D) {
      yv = a.x[row * a.ldx + c] + (v + a.bo[c]) * drop_mul(a.p, dk, (uint64_t)(row * D + c));
      a.y1[row * D + c] = yv;
    }
    s1[r * LD + c] = yv;
  });
  __syncthreads();
  ln_rows<DP>(s1, s0, a.gamma1, a.beta1, a.eps1, r0, M, D, nullptr, a.stats1, t);  // x1 (the first product is done with s0)
  // f = a W2^T over the chunks of the hidden; a chunk of a lives in s1 between its two products
  v16f accf = zero16();
  for (int f0 = 0; f0 < F; f0 += DP) {
    const int fc = F - f0 < DP ? F - f0 : DP;
    const v16f u = tile_gemm<DP, true>(zero16(), s0, a.w1 + (int64_t)f0 * D, D, D, fc, wl, t);
    // (every wavefront has passed a barrier of that product since it last read s1)
    for_acc(u, t, [&](int r, int c, float v) {
      const int64_t row = r0 + r;
      float av = 0.f;
      if (row < M && c < fc) {
        const float uv = v + a.b1[f0 + c];
        av = (uv > 0.f ? uv : uv * a.slope) * drop_mul(a.p, dk, MD + (uint64_t)row * F + f0 + c);
      }
      s1[r * LD + c] = av;
    });
    accf = tile_gemm<DP, true>(accf, s1, a.w2 + f0, F, fc, D, wl, t);
  }
  __syncthreads();  // (the last product has read s1)
  // y2 = x1 + drop_f(f + b2), out = LN2(y2)
  for_acc(accf, t, [&](int r, int c, float v) {
    const int64_t row = r0 + r;
    float yv = 0.f;
    if (row < M && c < D) {
      yv = s0[r * LD + c] + (v + a.b2[c]) * drop_mul(a.p, dk, MD + MF + (uint64_t)(row * D + c));
      a.y2[row * D + c] = yv;
    }
    s1[r * LD + c] = yv;
  });
  __syncthreads();
  ln_rows<DP>(s1, s1, a.gamma2, a.beta2, a.eps2, r0, M, D, a.out, a.stats2, t);  // (a wavefront reads a row, then writes it)
}

// part (ntiles, 5, D) = per-tile [g_gamma2 | g_beta2 | g_gamma1 | g_beta1 | g_b2]
template <int DP>
__global__ __launch_bounds__(RH_BLOCK) void enc_bwd_rows_kernel(const EncArgs a) {
  constexpr int TR = Tile<DP>::TR, LD = Tile<DP>::LD;
  extern __shared__ float lds[];
  float* s0 = lds;
  float* s1 = s0 + TR * LD;
  float* s2 = s1 + TR * LD;
  float* wl = s2 + TR * LD;
  float* sm1 = wl + kKC * LD;
  float* sr1 = sm1 + TR;
  float* sm2 = sr1 + TR;
  float* sr2 = sm2 + TR;
  const Lane t = lane_of<DP>();
  const int r0 = blockIdx.x * TR, M = a.M, D = a.D, F = a.F;
  const uint64_t MD = (uint64_t)M * D, MF = (uint64_t)M * F;
  const DropKey dk = drop_key(a.p, a.rng, a.saved_ctr, 0);
  float* part = a.part + (int64_t)blockIdx.x * 5 * D;
  load_stats<TR>(sm1, sr1, a.stats1, r0, M, t.tid);
  load_stats<TR>(sm2, sr2, a.stats2, r0, M, t.tid);
  load_rows<DP>(s1, a.g_out, D, r0, M, D, t.tid);
  __syncthreads();
  recompute_x1<DP>(s0, a, sm1, sr1, r0, t.tid);
  col_partials(s1, LD, TR, a.y2, sm2, sr2, r0, M, D, part, t.tid);
  __syncthreads();
  ln_bwd_rows<DP>(s1, s1, a.y2, a.gamma2, sm2, sr2, r0, M, D, t);  // g_y2 (a wavefront reads a row, then writes it)
  __syncthreads();
  // g_y2 stays in registers as the residual's share of g_x1; the tile becomes g_f = drop_f(g_y2).  A wavefront's
  // accumulator positions cover the tile once, so every element has one owner.
  v16f res;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rr = 32 * t.wm + acc_row(r, t.kk), c = 32 * t.wn + t.li;
    const int64_t row = r0 + rr;
    res[r] = s1[rr * LD + c];
    if (row < M && c < D) {
      const float gf = res[r] * drop_mul(a.p, dk, MD + MF + (uint64_t)(row * D + c));
      s1[rr * LD + c] = gf;
      a.g_f[row * D + c] = gf;
    }
  }
  __syncthreads();
  if (t.tid < D) {
    float gb = 0.f;
    for (int r = 0; r < TR && r0 + r < M; ++r) gb += s1[r * LD + t.tid];
    part[4 * D + t.tid] = gb;
  }
  // g_x1 = g_y2 + sum over the chunks of g_u W1_chunk, g_u = (g_f W2_chunk) leaky'(u) drop_h with u recomputed
  v16f accx = zero16();
  for (int f0 = 0; f0 < F; f0 += DP) {
    const int fc = F - f0 < DP ? F - f0 : DP;
    const v16f u = tile_gemm<DP, true>(zero16(), s0, a.w1 + (int64_t)f0 * D, D, D, fc, wl, t);
    const v16f ga = tile_gemm<DP, false>(zero16(), s1, a.w2 + f0, F, D, fc, wl, t);
    // (every wavefront has passed a barrier of those products since it last read s2)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = 32 * t.wm + acc_row(r, t.kk), c = 32 * t.wn + t.li;
      const int64_t row = r0 + rr;
      float gu = 0.f;
      if (row < M && c < fc) {
        const float uv = u[r] + a.b1[f0 + c];
        gu = ga[r] * (uv > 0.f ? 1.f : a.slope) * drop_mul(a.p, dk, MD + (uint64_t)row * F + f0 + c);
      }
      s2[rr * LD + c] = gu;
    }
    accx = tile_gemm<DP, false>(accx, s2, a.w1 + (int64_t)f0 * D, D, fc, D, wl, t);
  }
  // (the first product of the last chunk was the last reader of s0, two barriers ago)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rr = 32 * t.wm + acc_row(r, t.kk), c = 32 * t.wn + t.li;
    s0[rr * LD + c] = (r0 + rr < M && c < D) ? accx[r] + res[r] : 0.f;
  }
  __syncthreads();  // (and the last product has read s2)
  col_partials(s0, LD, TR, a.y1, sm1, sr1, r0, M, D, part + 2 * D, t.tid);
  ln_bwd_rows<DP>(s0, s2, a.y1, a.gamma1, sm1, sr1, r0, M, D, t);  // g_y1 = g_x
  __syncthreads();
  for (int e = t.tid; e < TR * DP; e += RH_BLOCK) {
    const int r = e / DP, c = e % DP;
    const int64_t row = r0 + r;
    if (row < M && c < D) {
      const float gy = s2[r * LD + c];
      const float go = gy * drop_mul(a.p, dk, (uint64_t)(row * D + c));
      a.g_x[row * D + c] = gy;
      a.g_o[row * D + c] = go;
      s2[r * LD + c] = go;
    }
  }
  const v16f gat = tile_gemm<DP, false>(zero16(), s2, a.wo, D, D, D, wl, t);
  for_acc(gat, t, [&](int r, int c, float v) {
    if (r0 + r < M && c < D) a.g_attn[(int64_t)(r0 + r) * D + c] = v;
  });
}

// wpart (nsplits, (2 D + 1) F) = per-split [g_W1 (F, D) | g_W2 (D, F) | g_b1 (F)]; workgroup (chunk, split) writes the
// chunk's columns of its split's row, every element of them
template <int DP>
__global__ __launch_bounds__(RH_BLOCK) void enc_bwd_weights_kernel(const EncArgs a) {
  constexpr int TR = Tile<DP>::TR, LD = Tile<DP>::LD;
  constexpr int NB = DP == 64 ? 1 : 4;  // 32 x 32 blocks of a (DP, DP) weight-gradient chunk per wavefront
  extern __shared__ float lds[];
  float* s0 = lds;
  float* s1 = s0 + TR * LD;
  float* s2 = s1 + TR * LD;
  float* s3 = s2 + TR * LD;
  float* wl = s3 + TR * LD;
  float* sm1 = wl + kKC * LD;
  float* sr1 = sm1 + TR;
  const Lane t = lane_of<DP>();
  const int M = a.M, D = a.D, F = a.F;
  const int f0 = blockIdx.x * DP, fc = F - f0 < DP ? F - f0 : DP;
  const int ntiles = (M + TR - 1) / TR;
  const int tile0 = blockIdx.y * a.tiles_per_split;
  const int tile1 = tile0 + a.tiles_per_split < ntiles ? tile0 + a.tiles_per_split : ntiles;
  const uint64_t MD = (uint64_t)M * D;
  const DropKey dk = drop_key(a.p, a.rng, a.saved_ctr, 0);
  v16f gw1[NB], gw2[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) gw1[q] = gw2[q] = zero16();
  float gb1 = 0.f;
  for (int tile = tile0; tile < tile1; ++tile) {
    const int r0 = tile * TR;
    __syncthreads();  // (the products of the tile before have read all four tiles)
    load_stats<TR>(sm1, sr1, a.stats1, r0, M, t.tid);
    load_rows<DP>(s1, a.g_f, D, r0, M, D, t.tid);
    __syncthreads();
    recompute_x1<DP>(s0, a, sm1, sr1, r0, t.tid);
    const v16f u = tile_gemm<DP, true>(zero16(), s0, a.w1 + (int64_t)f0 * D, D, D, fc, wl, t);
    const v16f ga = tile_gemm<DP, false>(zero16(), s1, a.w2 + f0, F, D, fc, wl, t);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = 32 * t.wm + acc_row(r, t.kk), c = 32 * t.wn + t.li;
      const int64_t row = r0 + rr;
      float av = 0.f, gu = 0.f;
      if (row < M && c < fc) {
        const float uv = u[r] + a.b1[f0 + c];
        const float m = drop_mul(a.p, dk, MD + (uint64_t)row * F + f0 + c);
        av = (uv > 0.f ? uv : uv * a.slope) * m;
        gu = ga[r] * (uv > 0.f ? 1.f : a.slope) * m;
      }
      s2[rr * LD + c] = av;
      s3[rr * LD + c] = gu;
    }
    __syncthreads();
    if (t.tid < fc)
      for (int r = 0; r < TR; ++r) gb1 += s3[r * LD + t.tid];
    // g_W2[d][j] += sum_r g_f[r][d] a[r][j];  g_W1[j][d] += sum_r g_u[r][j] x1[r][d]  (rows beyond M are zero in both)
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const int bi = DP == 64 ? (t.w & 1) : q, bj = DP == 64 ? (t.w >> 1) : t.w;
      gw2[q] = mma_lds(gw2[q], s1 + 32 * bi, 1, LD, s2 + 32 * bj, LD, 1, TR, t.li, t.kk);
      gw1[q] = mma_lds(gw1[q], s3 + 32 * bi, 1, LD, s0 + 32 * bj, LD, 1, TR, t.li, t.kk);
    }
  }
  float* out = a.wpart + (int64_t)blockIdx.y * (2 * D + 1) * F;
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int bi = DP == 64 ? (t.w & 1) : q, bj = DP == 64 ? (t.w >> 1) : t.w;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = 32 * bi + acc_row(r, t.kk), j = 32 * bj + t.li;
      if (i < fc && j < D) out[(int64_t)(f0 + i) * D + j] = gw1[q][r];
      if (i < D && j < fc) out[(int64_t)F * D + (int64_t)i * F + f0 + j] = gw2[q][r];
    }
  }
  if (t.tid < fc) out[2 * (int64_t)F * D + f0 + t.tid] = gb1;
}

int tiles_of(int M, int D) { return D <= 64 ? (M + 63) / 64 : (M + 31) / 32; }
int chunks_of(int F, int D) { return D <= 64 ? (F + 63) / 64 : (F + 127) / 128; }

// row splits of the weight kernel: chunks x splits fills the chip once, whatever M; no split is empty
void splits_of(int M, int D, int F, int* tiles_per_split, int* nsplits) {
  const int ntiles = tiles_of(M, D), nchunks = chunks_of(F, D);
  int s = kWeightGrid / nchunks;
  if (s < 1) s = 1;
  if (s > ntiles) s = ntiles;
  *tiles_per_split = (ntiles + s - 1) / s;
  *nsplits = (ntiles + *tiles_per_split - 1) / *tiles_per_split;
}

int check_shape(const char* name, int M, int D, int F) {
  RH_REQUIRE(D >= 1 && D <= kMaxD, RH_E_UNSUPPORTED, "%s: width %d unsupported (1 <= D <= %d)", name, D, kMaxD);
  RH_REQUIRE(F >= 1 && F <= 0x7FFFFFFF / (2 * kMaxD + 1), RH_E_UNSUPPORTED, "%s: hidden width %d unsupported (F >= 1)",
             name, F);
  RH_REQUIRE(M >= 0 && M <= 0x7FFFFFFF - 64, RH_E_UNSUPPORTED, "%s: %d rows unsupported", name, M);
  return 0;
}

int check_drop(const char* name, float p, const void* rng, const void* saved_ctr) {
  RH_REQUIRE(p >= 0.f && p < 1.f, RH_E_BADARG, "%s: dropout p=%g outside [0, 1)", name, (double)p);
  RH_REQUIRE(p == 0.f || (rng && saved_ctr), RH_E_BADARG, "%s: dropout without its (seed, counter) state", name);
  return 0;
}

template <typename Kernel>
int launch(Kernel* kernel, size_t lds, dim3 grid, hipStream_t st, const EncArgs& a, RhLdsReserved& reserved, const char* who) {
  if (int rc = rh_reserve_lds(reserved, kernel, lds, who)) return rc;
  hipLaunchKernelGGL(kernel, grid, dim3(RH_BLOCK), lds, st, a);
  return 0;
}

}  // namespace

// one `static RhLdsReserved` per kernel instantiation
#define RH_ENC_LAUNCH(kernel, tiles, stat_vectors, grid, st, a, who)                                               \
  do {                                                                                                             \
    int rc_;                                                                                                       \
    if ((a).D <= 64) {                                                                                             \
      static RhLdsReserved r64;                                                                                    \
      rc_ = launch(kernel<64>, lds_bytes<64>(tiles, stat_vectors), grid, st, a, r64, who);                         \
    } else {                                                                                                       \
      static RhLdsReserved r128;                                                                                   \
      rc_ = launch(kernel<128>, lds_bytes<128>(tiles, stat_vectors), grid, st, a, r128, who);                      \
    }                                                                                                              \
    if (rc_) return rc_;                                                                                           \
  } while (0)

extern "C" int rh_enc_nsplits(int M, int D, int F, int* ntiles, int* nsplits) {
  RH_REQUIRE(ntiles && nsplits, RH_E_BADARG, "rh_enc_nsplits: null pointer");
  if (int rc = check_shape("rh_enc_nsplits", M, D, F)) return rc;
  int tps = 0;
  *ntiles = tiles_of(M, D);
  *nsplits = 0;
  if (M > 0) splits_of(M, D, F, &tps, nsplits);
  return 0;
}

extern "C" int rh_enc_block_fwd(const float* attn, const float* x, int64_t ldx, const float* wo, const float* bo,
                                const float* gamma1, const float* beta1, float eps1, const float* w1, const float* b1,
                                const float* w2, const float* b2, const float* gamma2, const float* beta2, float eps2,
                                float slope, int M, int D, int F, float p_drop, int64_t* rng, int64_t* saved_ctr, float* y1,
                                float* y2, float* stats1, float* stats2, float* out, void* stream) {
  if (int rc = check_shape("rh_enc_block_fwd", M, D, F)) return rc;
  if (int rc = check_drop("rh_enc_block_fwd", p_drop, rng, saved_ctr)) return rc;
  RH_REQUIRE(attn && x && wo && bo && gamma1 && beta1 && w1 && b1 && w2 && b2 && gamma2 && beta2 && y1 && y2 && stats1 &&
                 stats2 && out, RH_E_BADARG, "rh_enc_block_fwd: null pointer");
  RH_REQUIRE(ldx >= D, RH_E_BADARG, "rh_enc_block_fwd: row stride %lld below the width %d", (long long)ldx, D);
  if (M == 0) return 0;
  EncArgs a{};
  a.attn = attn, a.x = x, a.ldx = ldx, a.wo = wo, a.bo = bo, a.gamma1 = gamma1, a.beta1 = beta1, a.w1 = w1, a.b1 = b1;
  a.w2 = w2, a.b2 = b2, a.gamma2 = gamma2, a.beta2 = beta2, a.rng = rng, a.saved_ctr = saved_ctr;
  a.y1 = y1, a.y2 = y2, a.stats1 = stats1, a.stats2 = stats2, a.out = out;
  a.M = M, a.D = D, a.F = F, a.eps1 = eps1, a.eps2 = eps2, a.slope = slope, a.p = p_drop;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  RH_ENC_LAUNCH(enc_fwd_kernel, 2, 0, dim3(tiles_of(M, D)), st, a, "rh_enc_block_fwd");
  if (p_drop > 0.f) hipLaunchKernelGGL(drop_advance_kernel, dim3(1), dim3(1), 0, st, rng);
  RH_LAUNCH_CHECK("rh_enc_block_fwd");
  return 0;
}

namespace {
// what both backward kernels take: the recomputation's inputs
int bwd_args(const char* name, EncArgs& a, const float* gamma1, const float* beta1, const float* w1, const float* b1,
             const float* w2, const float* y1, const float* stats1, float slope, int M, int D, int F, float p_drop,
             const int64_t* rng, const int64_t* saved_ctr, float* g_f) {
  if (int rc = check_shape(name, M, D, F)) return rc;
  if (int rc = check_drop(name, p_drop, rng, saved_ctr)) return rc;
  RH_REQUIRE(gamma1 && beta1 && w1 && b1 && w2 && y1 && stats1 && g_f, RH_E_BADARG, "%s: null pointer", name);
  a.gamma1 = gamma1, a.beta1 = beta1, a.w1 = w1, a.b1 = b1, a.w2 = w2;
  a.y1 = const_cast<float*>(y1), a.stats1 = const_cast<float*>(stats1), a.g_f = g_f;
  a.rng = rng, a.saved_ctr = const_cast<int64_t*>(saved_ctr);
  a.M = M, a.D = D, a.F = F, a.slope = slope, a.p = p_drop;
  return 0;
}
}  // namespace

extern "C" int rh_enc_block_bwd_rows(const float* wo, const float* gamma1, const float* beta1, const float* w1,
                                     const float* b1, const float* w2, const float* gamma2, const float* y1, const float* y2,
                                     const float* stats1, const float* stats2, const float* g_out, float slope, int M, int D,
                                     int F, float p_drop, const int64_t* rng, const int64_t* saved_ctr, float* g_f,
                                     float* g_o, float* g_x, float* g_attn, float* part, void* stream) {
  EncArgs a{};
  if (int rc = bwd_args("rh_enc_block_bwd_rows", a, gamma1, beta1, w1, b1, w2, y1, stats1, slope, M, D, F, p_drop, rng,
                        saved_ctr, g_f))
    return rc;
  RH_REQUIRE(wo && gamma2 && y2 && stats2 && g_out && g_o && g_x && g_attn && part, RH_E_BADARG,
             "rh_enc_block_bwd_rows: null pointer");
  if (M == 0) return 0;
  a.wo = wo, a.gamma2 = gamma2, a.y2 = const_cast<float*>(y2), a.stats2 = const_cast<float*>(stats2), a.g_out = g_out;
  a.g_o = g_o, a.g_x = g_x, a.g_attn = g_attn, a.part = part;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  RH_ENC_LAUNCH(enc_bwd_rows_kernel, 3, 4, dim3(tiles_of(M, D)), st, a, "rh_enc_block_bwd_rows");
  RH_LAUNCH_CHECK("rh_enc_block_bwd_rows");
  return 0;
}

extern "C" int rh_enc_block_bwd_weights(const float* gamma1, const float* beta1, const float* w1, const float* b1,
                                        const float* w2, const float* y1, const float* stats1, const float* g_f, float slope,
                                        int M, int D, int F, float p_drop, const int64_t* rng, const int64_t* saved_ctr,
                                        float* wpart, void* stream) {
  EncArgs a{};
  if (int rc = bwd_args("rh_enc_block_bwd_weights", a, gamma1, beta1, w1, b1, w2, y1, stats1, slope, M, D, F, p_drop, rng,
                        saved_ctr, const_cast<float*>(g_f)))
    return rc;
  RH_REQUIRE(wpart, RH_E_BADARG, "rh_enc_block_bwd_weights: null pointer");
  if (M == 0) return 0;
  a.wpart = wpart;
  int nsplits = 0;
  splits_of(M, D, F, &a.tiles_per_split, &nsplits);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  RH_ENC_LAUNCH(enc_bwd_weights_kernel, 4, 2, dim3(chunks_of(F, D), nsplits), st, a, "rh_enc_block_bwd_weights");
  RH_LAUNCH_CHECK("rh_enc_block_bwd_weights");
  return 0;
}
