// Compressed Interaction Network (the interaction of xDeepFM), one layer, for gfx950.
//
// Reference op chain replaced (paths relative to the reference package):
//   CIN.forward   torch_rechub/basic/layers.py:359-362   z = x0.unsqueeze(2) * h.unsqueeze(1) -> view (B, F Hp, D) ->
//                                                          Conv1d(F Hp, Ho, 1) -> relu, and its autograd (z kept for backward)
//
// The layer is ONE GEMM whose A operand is a product of two small tiles and never exists in HBM:
//   rows m = (b, d), M = B D;  K = F Hp, channel c = f Hp + h;  N = Ho;
//   A[m][c] = x0[b, f, d] h[b, h, d],   y[b, o, d] = relu(bias[o] + sum_c A[m][c] W[o][c]).
// All three kernels run the 64 x 64 workgroup tile of mfma_tile.h (v_mfma_f32_32x32x2_f32: exact f32 products, k-ordered
// accumulation).  Every staging loop lets consecutive lanes take consecutive rows m -- consecutive d of one sample, the
// contiguous direction of x0, h, y and g_y -- and LDS rows have an odd stride, so both sides are conflict-free.
//
//   forward  grid (row tiles <= kRowGrid, looping; Ho tiles).  LDS: the tile's x0 (64 x F) and h (64 x Hp) once per row tile;
//            per K chunk of 64 channels a 64 x 64 chunk of W and the A tile, each element x0[row][f] * h[row][hh], the product
//            of two LDS reads ((f, hh) of a column are wavefront-uniform scalars).  An odd K ends in a zero-filled step.
//   bwd      grid (row tiles <= kRowGrid, looping).  A workgroup owns its 64 rows for all of K: per 64-channel chunk,
//            gz = gp W[:, chunk] (gp = g_y where y > 0) accumulates over Ho on the MFMA tile, is dumped to LDS and folded, per
//            field of the chunk in ascending order, into the LDS accumulators g_x0[row][f] += sum_j gz[row][j] h[row][hh(j)],
//            g_h[row][hh(j)] += gz[row][j] x0[row][f].  Each accumulator element belongs to ONE thread (row = tid % 64, f or
//            hh = tid / 64 mod 4): no atomics, a fixed order, every output element written exactly once.
//   wgrad    grid (Ho tiles x K tiles, M chunks <= kMaxChunks).  g_W tile = sum over the chunk's rows of gp^T z, z re-formed
//            while staging; the K tile 0 workgroups also sum gp's columns (g_bias).  Per-chunk partials (chunks, Ho K + Ho)
//            are added in chunk order by rh_colsum: two runs give the same bits.
// All three fetch the operands of the NEXT MFMA pass into registers before they run the current one (single LDS buffer,
// the global latency hidden behind the 32 MFMA steps of a pass).
//
// Roofline: the fp32 MFMA rate (2 M K Ho flop forward, 4 M K Ho backward); HBM traffic is the operands only.
#include "mfma_tile.h"

namespace {

constexpr int kMaxF = RH_CIN_MAX_F;
constexpr int kMaxHp = RH_CIN_MAX_HP;
constexpr int kMaxHo = RH_CIN_MAX_HO;
constexpr int kMaxD = RH_CIN_MAX_D;
constexpr int kRowGrid = 1024;   // row tiles per launch; a workgroup loops over the rest
constexpr int kMaxChunks = 16;   // wgrad: M chunks (rows of the partial workspace)
constexpr int kFillTiles = 512;  // wgrad: workgroups aimed for (2 per CU)
constexpr int kQ = RH_BLOCK / kT;  // staging: row = tid % 64, column = tid / 64 + kQ i

struct CinArgs {
  const float* x0;  // (B, F, D): sample stride xs, field stride xf
  int64_t xs, xf;
  const float* h;   // (B, Hp, D): sample stride hs, field stride D
  int64_t hs;
  const float* w;   // (Ho, K)
  const float* bias;
  const float* y;   // backward: the forward's output (B, Ho, D) and its gradient, both contiguous
  const float* g;
  float* out;       // forward: y
  float* gx0;       // bwd: (B, F, D) contiguous or null
  float* gh;        // bwd: (B, Hp, D) contiguous or null
  float* part;      // wgrad: (chunks, Ho K + Ho)
  int64_t M, rpc;   // rows; rows per wgrad chunk (a multiple of 64)
  int D, F, Hp, Ho, K;
};

__device__ __forceinline__ int odd(int n) { return n | 1; }

__global__ __launch_bounds__(RH_BLOCK) void cin_fwd_kernel(const CinArgs a) {
  extern __shared__ float lds[];
  const int F = a.F, Hp = a.Hp, Ho = a.Ho, K = a.K, D = a.D;
  const int ldx = odd(F), ldh = odd(Hp);
  float* sX = lds;             // [64][ldx]
  float* sH = sX + kT * ldx;   // [64][ldh]
  float* sW = sH + kT * ldh;   // [64 k][kLd]: W[o0 + j][c0 + k]; then the output tile [64 o][kLd]
  float* sA = sW + kT * kLd;   // [64 rows][kLd]: x0[row][f(c0 + k)] h[row][hh(c0 + k)]
  const int tid = threadIdx.x, lane = tid % RH_WAVE, wv = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = wv & 1, wn = wv >> 1;
  const int rl = tid % kT, q = tid / kT;
  const int o0 = blockIdx.y * kT;
  const int64_t ntile = (a.M + kT - 1) / kT;
  // the next chunk of W travels in registers while the MFMA loop of this one runs
  float rw[kT / kQ];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int i = 0; i < kT / kQ; ++i) {
      const int e = tid + RH_BLOCK * i, k = e % kT, j = e / kT;
      rw[i] = (c0 + k < K && o0 + j < Ho) ? a.w[(int64_t)(o0 + j) * K + c0 + k] : 0.f;
    }
  };
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int64_t m = t * kT + rl;
    const bool ok = m < a.M;
    const int64_t b = ok ? m / D : 0;
    const int d = ok ? (int)(m - b * D) : 0;
    const float* xr = a.x0 + b * a.xs + d;
    const float* hr = a.h + b * a.hs + d;
    __syncthreads();  // (the previous tile is done with the LDS)
    for (int f = q; f < F; f += kQ) sX[rl * ldx + f] = ok ? xr[f * a.xf] : 0.f;
    for (int hh = q; hh < Hp; hh += kQ) sH[rl * ldh + hh] = ok ? hr[(int64_t)hh * D] : 0.f;
    fetch(0);
    v16f acc = zero16();
    for (int c0 = 0; c0 < K; c0 += kT) {
      __syncthreads();  // (the previous chunk is done with sW / sA; first trip: sX / sH are written)
#pragma unroll
      for (int i = 0; i < kT / kQ; ++i) {
        const int e = tid + RH_BLOCK * i;
        sW[(e % kT) * kLd + e / kT] = rw[i];
        const int j = q + kQ * i, c = c0 + j < K ? c0 + j : 0, f = c / Hp;  // (wavefront-uniform: scalar arithmetic)
        sA[rl * kLd + j] = c0 + j < K ? sX[rl * ldx + f] * sH[rl * ldh + c - f * Hp] : 0.f;  // K's tail is zero-filled
      }
      __syncthreads();
      if (c0 + kT < K) fetch(c0 + kT);
      acc = mma_lds(acc, sA + 32 * wm * kLd, kLd, 1, sW + 32 * wn, kLd, 1, kT, li, kk);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) sW[(32 * wn + li) * kLd + 32 * wm + acc_row(r, kk)] = acc[r];
    __syncthreads();
    if (ok) {
      for (int j = q; j < kT && o0 + j < Ho; j += kQ)
        a.out[(b * Ho + o0 + j) * D + d] = fmaxf(sW[j * kLd + rl] + a.bias[o0 + j], 0.f);
    }
  }
}

__global__ __launch_bounds__(RH_BLOCK) void cin_bwd_kernel(const CinArgs a) {
  extern __shared__ float lds[];
  const int F = a.F, Hp = a.Hp, Ho = a.Ho, K = a.K, D = a.D;
  const int ldx = odd(F), ldh = odd(Hp);
  float* aX = lds;             // [64][ldx] g_x0 accumulators
  float* aH = aX + kT * ldx;   // [64][ldh] g_h accumulators
  float* sG = aH + kT * ldh;   // [64 rows][kLd]: gp[row][o0 + k]; then gz[row][c0 + j]
  float* sW = sG + kT * kLd;   // [64 k][kLd]: W[o0 + k][c0 + j]; then h[row][hh(c0 + j)]
  const int tid = threadIdx.x, lane = tid % RH_WAVE, wv = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = wv & 1, wn = wv >> 1;
  const int rl = tid % kT, q = tid / kT;
  const int64_t ntile = (a.M + kT - 1) / kT;
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int64_t m = t * kT + rl;
    const bool ok = m < a.M;
    const int64_t b = ok ? m / D : 0;
    const int d = ok ? (int)(m - b * D) : 0;
    const float* xr = a.x0 + b * a.xs + d;
    const float* hr = a.h + b * a.hs + d;
    const int64_t yb = b * Ho * D + d;
    // the accumulators of (rl, f = q mod kQ) and (rl, hh = q mod kQ) are this thread's alone: no barrier guards them
    for (int f = q; f < F; f += kQ) aX[rl * ldx + f] = 0.f;
    for (int hh = q; hh < Hp; hh += kQ) aH[rl * ldh + hh] = 0.f;
    // operands of the NEXT pass travel in registers while the MFMA loop of this one runs
    float ry[kT / kQ], rg[kT / kQ], rw[kT / kQ], rh[kT / kQ];
    auto fetch = [&](int c0, int o0) {
#pragma unroll
      for (int i = 0; i < kT / kQ; ++i) {
        const int j = q + kQ * i;
        const bool in = ok && o0 + j < Ho;
        const int64_t at = in ? yb + (int64_t)(o0 + j) * D : 0;
        ry[i] = in ? a.y[at] : 0.f;
        rg[i] = in ? a.g[at] : 0.f;
        const int e = tid + RH_BLOCK * i, jc = e % kT, k = e / kT;
        const bool inw = c0 + jc < K && o0 + k < Ho;
        rw[i] = inw ? a.w[(int64_t)(o0 + k) * K + c0 + jc] : 0.f;
      }
    };
    fetch(0, 0);
    for (int c0 = 0; c0 < K; c0 += kT) {
      const int kc = K - c0 < kT ? K - c0 : kT;
      const int f_lo = c0 / Hp, f_hi = (c0 + kc - 1) / Hp;
#pragma unroll
      for (int i = 0; i < kT / kQ; ++i) {  // h[row][hh(c0 + j)] for the fold below
        const int j = q + kQ * i;
        const bool in = ok && j < kc;
        rh[i] = in ? hr[(int64_t)((c0 + j) % Hp) * D] : 0.f;
      }
      const float xv0 = ok ? xr[f_lo * a.xf] : 0.f;
      const float xv1 = ok ? xr[(f_lo + 1 < F ? f_lo + 1 : F - 1) * a.xf] : 0.f;
      v16f acc = zero16();
      for (int o0 = 0; o0 < Ho; o0 += kT) {
        __syncthreads();  // (the previous pass is done with sG / sW, the previous chunk with its fold)
#pragma unroll
        for (int i = 0; i < kT / kQ; ++i) {
          sG[rl * kLd + q + kQ * i] = ry[i] > 0.f ? rg[i] : 0.f;
          const int e = tid + RH_BLOCK * i;
          sW[(e / kT) * kLd + e % kT] = rw[i];
        }
        __syncthreads();
        int o1 = o0 + kT, c1 = c0;
        if (o1 >= Ho) {
          o1 = 0;
          c1 = c0 + kT;
        }
        if (c1 < K) fetch(c1, o1);
        acc = mma_lds(acc, sG + 32 * wm * kLd, kLd, 1, sW + 32 * wn, kLd, 1, kT, li, kk);
      }
      __syncthreads();  // (every wavefront has read sG / sW)
#pragma unroll
      for (int r = 0; r < 16; ++r) sG[(32 * wm + acc_row(r, kk)) * kLd + 32 * wn + li] = acc[r];
#pragma unroll
      for (int i = 0; i < kT / kQ; ++i) sW[rl * kLd + q + kQ * i] = rh[i];
      __syncthreads();
      // the fold, per field of the chunk in ascending order; a thread reads its own row of gz and h only
      const float* gz = sG + rl * kLd;
      const float* hz = sW + rl * kLd;
      for (int f = f_lo; f <= f_hi; ++f) {
        const int j0 = f * Hp > c0 ? f * Hp - c0 : 0;
        const int j1 = (f + 1) * Hp - c0 < kc ? (f + 1) * Hp - c0 : kc;
        if (a.gx0 != nullptr && (f % kQ) == q) {  // g_x0[row][f] += sum_j gz[row][j] h[row][hh(j)]
          float s = 0.f;
#pragma unroll 8
          for (int j = j0; j < j1; ++j) s = fmaf(gz[j], hz[j], s);
          aX[rl * ldx + f] += s;
        }
        if (a.gh != nullptr) {  // g_h[row][hh(j)] += gz[row][j] x0[row][f] for the hh = q mod kQ
          const float xv = f == f_lo ? xv0 : (f == f_lo + 1 ? xv1 : (ok ? xr[f * a.xf] : 0.f));
          const int hh0 = c0 + j0 - f * Hp;  // hh of column j0
          float* ah = aH + rl * ldh + hh0 - j0;  // ah[j] = the accumulator of column j
          for (int j = j0 + ((q - hh0 % kQ) + kQ) % kQ; j < j1; j += 4 * kQ) {
            float av[4], zv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int ju = j + u * kQ;
              av[u] = ju < j1 ? ah[ju] : 0.f;
              zv[u] = ju < j1 ? gz[ju] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int ju = j + u * kQ;
              if (ju < j1) ah[ju] = fmaf(zv[u], xv, av[u]);
            }
          }
        }
      }
    }
    if (ok) {
      if (a.gx0 != nullptr)
        for (int f = q; f < F; f += kQ) a.gx0[(b * F + f) * D + d] = aX[rl * ldx + f];
      if (a.gh != nullptr)
        for (int hh = q; hh < Hp; hh += kQ) a.gh[(b * Hp + hh) * D + d] = aH[rl * ldh + hh];
    }
  }
}

__global__ __launch_bounds__(RH_BLOCK) void cin_wgrad_kernel(const CinArgs a) {
  __shared__ float sG[kT * kLd];  // [64 rows][kLd]: gp[row][o0 + i]
  __shared__ float sZ[kT * kLd];  // [64 rows][kLd]: z[row][c0 + j]
  const int Hp = a.Hp, Ho = a.Ho, K = a.K, D = a.D;
  const int tid = threadIdx.x, lane = tid % RH_WAVE, wv = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = wv & 1, wn = wv >> 1;
  const int rl = tid % kT, q = tid / kT;
  const int nct = (K + kT - 1) / kT;
  const int ot = blockIdx.x / nct, ct = blockIdx.x - ot * nct;
  const int o0 = ot * kT, c0 = ct * kT;
  const int64_t r0 = (int64_t)blockIdx.y * a.rpc;
  const int64_t r1 = r0 + a.rpc < a.M ? r0 + a.rpc : a.M;
  // the next block of rows travels in registers while the MFMA loop of this one runs
  float ry[kT / kQ], rg[kT / kQ], rx[kT / kQ], rh[kT / kQ];
  auto fetch = [&](int64_t mb) {
    const int64_t m = mb + rl;
    const bool ok = m < r1;
    const int64_t b = ok ? m / D : 0;
    const int d = ok ? (int)(m - b * D) : 0;
    const float* xr = a.x0 + b * a.xs + d;
    const float* hr = a.h + b * a.hs + d;
    const int64_t yb = b * Ho * D + d;
#pragma unroll
    for (int i = 0; i < kT / kQ; ++i) {
      const int j = q + kQ * i;
      const bool in = ok && o0 + j < Ho;
      const int64_t at = in ? yb + (int64_t)(o0 + j) * D : 0;
      ry[i] = in ? a.y[at] : 0.f;
      rg[i] = in ? a.g[at] : 0.f;
      const bool inz = ok && c0 + j < K;
      const int c = inz ? c0 + j : 0, f = c / Hp;  // (q, hence j and c, is wavefront-uniform: scalar arithmetic)
      rx[i] = inz ? xr[f * a.xf] : 0.f;
      rh[i] = inz ? hr[(int64_t)(c - f * Hp) * D] : 0.f;
    }
  };
  v16f acc = zero16();
  float bsum = 0.f;
  if (r0 < r1) fetch(r0);
  for (int64_t mb = r0; mb < r1; mb += kT) {
    __syncthreads();  // (the previous block of rows is done with sG / sZ)
#pragma unroll
    for (int i = 0; i < kT / kQ; ++i) {
      sG[rl * kLd + q + kQ * i] = ry[i] > 0.f ? rg[i] : 0.f;
      sZ[rl * kLd + q + kQ * i] = rx[i] * rh[i];
    }
    __syncthreads();
    if (mb + kT < r1) fetch(mb + kT);
    acc = mma_lds(acc, sG + 32 * wm, 1, kLd, sZ + 32 * wn, kLd, 1, kT, li, kk);
    if (ct == 0 && tid < kT) {
      for (int k = 0; k < kT; ++k) bsum += sG[k * kLd + tid];
    }
  }
  float* part = a.part + (int64_t)blockIdx.y * ((int64_t)Ho * K + Ho);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = o0 + 32 * wm + acc_row(r, kk), c = c0 + 32 * wn + li;
    if (o < Ho && c < K) part[(int64_t)o * K + c] = acc[r];
  }
  if (ct == 0 && tid < kT && o0 + tid < Ho) part[(int64_t)Ho * K + o0 + tid] = bsum;
}

int check_shape(const char* who, int B, int D, int F, int Hp, int Ho) {
  RH_REQUIRE(B >= 0, RH_E_BADARG, "%s: bad batch size %d", who, B);
  RH_REQUIRE(D >= 1 && D <= kMaxD, RH_E_UNSUPPORTED, "%s: embed_dim %d unsupported (1 .. %d)", who, D, kMaxD);
  RH_REQUIRE(F >= 1 && F <= kMaxF, RH_E_UNSUPPORTED, "%s: num_fields %d unsupported (1 .. %d)", who, F, kMaxF);
  RH_REQUIRE(Hp >= 1 && Hp <= kMaxHp, RH_E_UNSUPPORTED, "%s: input channels %d unsupported (1 .. %d)", who, Hp, kMaxHp);
  RH_REQUIRE(Ho >= 1 && Ho <= kMaxHo, RH_E_UNSUPPORTED, "%s: output channels %d unsupported (1 .. %d)", who, Ho, kMaxHo);
  return 0;
}

CinArgs make_args(const float* x0, int64_t xs, int64_t xf, const float* h, int64_t hs, int B, int D, int F, int Hp, int Ho) {
  CinArgs a{};
  a.x0 = x0;
  a.xs = xs;
  a.xf = xf;
  a.h = h;
  a.hs = hs;
  a.M = (int64_t)B * D;
  a.D = D;
  a.F = F;
  a.Hp = Hp;
  a.Ho = Ho;
  a.K = F * Hp;
  return a;
}

// chunks of the wgrad's M split and the rows of one: enough workgroups to fill the chip, at most kMaxChunks
int wgrad_chunks(int64_t M, int Ho, int K, int64_t* rpc) {
  const int64_t rt = (M + kT - 1) / kT;
  const int64_t tiles = (int64_t)((Ho + kT - 1) / kT) * ((K + kT - 1) / kT);
  int64_t n = (kFillTiles + tiles - 1) / tiles;
  if (n > kMaxChunks) n = kMaxChunks;
  if (n > rt) n = rt;
  if (n < 1) n = 1;
  const int64_t per = (rt + n - 1) / n;
  *rpc = (per < 1 ? 1 : per) * kT;
  return M <= 0 ? 0 : (int)((M + *rpc - 1) / *rpc);
}

size_t fwd_lds(int F, int Hp) { return sizeof(float) * (size_t)(kT * ((F | 1) + (Hp | 1)) + 2 * kT * kLd); }
size_t bwd_lds(int F, int Hp) { return sizeof(float) * (size_t)(kT * ((F | 1) + (Hp | 1)) + 2 * kT * kLd); }

// both kernels at their largest, whichever entry point comes first
int reserve_lds(const char* who) {
  static RhLdsReserved fwd, bwd;
  if (int rc = rh_reserve_lds(fwd, cin_fwd_kernel, fwd_lds(kMaxF, kMaxHp), who)) return rc;
  return rh_reserve_lds(bwd, cin_bwd_kernel, bwd_lds(kMaxF, kMaxHp), who);
}

unsigned row_grid(int64_t M) {
  const int64_t t = (M + kT - 1) / kT;
  return (unsigned)(t < kRowGrid ? t : kRowGrid);
}

}  // namespace

extern "C" int rh_cin_wgrad_chunks(int B, int D, int F, int Hp, int Ho, int* nchunks) {
  RH_REQUIRE(nchunks != nullptr, RH_E_BADARG, "rh_cin_wgrad_chunks: null pointer");
  if (int rc = check_shape("rh_cin_wgrad_chunks", B, D, F, Hp, Ho)) return rc;
  int64_t rpc = 0;
  *nchunks = wgrad_chunks((int64_t)B * D, Ho, F * Hp, &rpc);
  return 0;
}

extern "C" int rh_cin_fwd(const float* x0, int64_t x0_sample_stride, int64_t x0_field_stride, const float* h,
                          int64_t h_sample_stride, const float* w, const float* bias, int B, int D, int F, int Hp, int Ho,
                          float* y, void* stream) {
  RH_REQUIRE(x0 && h && w && bias && y, RH_E_BADARG, "rh_cin_fwd: null argument");
  if (int rc = check_shape("rh_cin_fwd", B, D, F, Hp, Ho)) return rc;
  RH_REQUIRE(x0_field_stride >= D && x0_sample_stride >= 0 && h_sample_stride >= 0, RH_E_BADARG,
             "rh_cin_fwd: bad strides");
  if (B == 0) return 0;
  if (int rc = reserve_lds("rh_cin_fwd")) return rc;
  CinArgs a = make_args(x0, x0_sample_stride, x0_field_stride, h, h_sample_stride, B, D, F, Hp, Ho);
  a.w = w;
  a.bias = bias;
  a.out = y;
  hipLaunchKernelGGL(cin_fwd_kernel, dim3(row_grid(a.M), (unsigned)((Ho + kT - 1) / kT)), dim3(RH_BLOCK), fwd_lds(F, Hp),
                     reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_cin_fwd");
  return 0;
}

extern "C" int rh_cin_bwd(const float* x0, int64_t x0_sample_stride, int64_t x0_field_stride, const float* h,
                          int64_t h_sample_stride, const float* w, const float* y, const float* g_y, int B, int D, int F,
                          int Hp, int Ho, float* g_x0, float* g_h, void* stream) {
  RH_REQUIRE(x0 && h && w && y && g_y && (g_x0 || g_h), RH_E_BADARG, "rh_cin_bwd: null argument");
  if (int rc = check_shape("rh_cin_bwd", B, D, F, Hp, Ho)) return rc;
  RH_REQUIRE(x0_field_stride >= D && x0_sample_stride >= 0 && h_sample_stride >= 0, RH_E_BADARG,
             "rh_cin_bwd: bad strides");
  if (B == 0) return 0;
  if (int rc = reserve_lds("rh_cin_bwd")) return rc;
  CinArgs a = make_args(x0, x0_sample_stride, x0_field_stride, h, h_sample_stride, B, D, F, Hp, Ho);
  a.w = w;
  a.y = y;
  a.g = g_y;
  a.gx0 = g_x0;
  a.gh = g_h;
  hipLaunchKernelGGL(cin_bwd_kernel, dim3(row_grid(a.M)), dim3(RH_BLOCK), bwd_lds(F, Hp),
                     reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_cin_bwd");
  return 0;
}

extern "C" int rh_cin_wgrad(const float* x0, int64_t x0_sample_stride, int64_t x0_field_stride, const float* h,
                            int64_t h_sample_stride, const float* y, const float* g_y, int B, int D, int F, int Hp, int Ho,
                            float* partial, void* stream) {
  RH_REQUIRE(x0 && h && y && g_y && partial, RH_E_BADARG, "rh_cin_wgrad: null argument");
  if (int rc = check_shape("rh_cin_wgrad", B, D, F, Hp, Ho)) return rc;
  RH_REQUIRE(x0_field_stride >= D && x0_sample_stride >= 0 && h_sample_stride >= 0, RH_E_BADARG,
             "rh_cin_wgrad: bad strides");
  if (B == 0) return 0;
  CinArgs a = make_args(x0, x0_sample_stride, x0_field_stride, h, h_sample_stride, B, D, F, Hp, Ho);
  a.y = y;
  a.g = g_y;
  a.part = partial;
  const int nch = wgrad_chunks(a.M, Ho, a.K, &a.rpc);
  const unsigned tiles = (unsigned)(((Ho + kT - 1) / kT) * ((a.K + kT - 1) / kT));
  hipLaunchKernelGGL(cin_wgrad_kernel, dim3(tiles, (unsigned)nch), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream),
                     a);
  RH_LAUNCH_CHECK("rh_cin_wgrad");
  return 0;
}
