// AutoInt's interacting layer -- multi-head self-attention over the F fields of a sample, a projected residual, a ReLU --
// as one launch each way, for gfx950.
//
// Reference op chain replaced (paths relative to the reference package):
//   InteractingLayer.forward   torch_rechub/basic/layers.py:1006-1044   W_Q / W_K / W_V / W_Res products, the (B, H, F, F)
//                                                                        scores, softmax, w @ v, transposes, add, relu, and its
//                                                                        autograd (projections, scores and softmax kept)
//
// The whole problem of a sample fits in LDS, so nothing but x, y and the row log-sum-exp ever exists in HBM.  One 64-row
// tile of mfma_tile.h (four wavefronts, v_mfma_f32_32x32x2_f32: exact f32 products) holds G = 64 / F whole samples, row
// r = g F + f; the rows of a tile are consecutive rows of the (B F, D) view of x, so every global access is a contiguous
// block.  Workgroups are persistent (tile t = blockIdx.x, += gridDim.x).
//
//   forward  per tile: X (64 x D) -> LDS; Q, K, V, R = X W^T for ALL heads at once (N = D, not dh: four products, each weight
//            staged transposed in the scores' buffer) -> LDS; per head S = scale Q_h K_h^T as one 64 x 64 tile -> LDS, row
//            softmax by four lanes per row over the F keys of the row's own sample (everything else of the row is written
//            as 0: the tile is block diagonal), lse -> HBM; O_h = P V_h (K = 64), y = relu(O_h + R_h) from the accumulators.
//   backward per tile: X and gO = g_y [y > 0] -> LDS; Q, K, V as above; per head S and gP = gO_h V_h^T -> LDS, the row pass
//            P = exp(S - lse) / its row sum, gS = scale P (gP - sum_row(gP P)); gV_h = P^T gO_h, gK_h = gS^T Q_h, gQ_h = gS K_h overwrite
//            V_h, K_h, Q_h in place.  After the heads the four (64 x D) gradients [gQ | gK | gV | gO] give
//            g_x = sum_p G_p W_p (K = D) and, in accumulator registers kept across all of the workgroup's tiles,
//            g_W_p += G_p^T X (K = 64); those 4 D D sums are written once, as the workgroup's row of `part`.
//
// A product whose K is odd ends in a step whose upper half-wavefront feeds zeros; lanes past a product's M or N read a
// clamped row / column (their results are not stored), wavefronts whose quadrant lies outside do nothing.  Dead rows (past
// G F, or of samples past B) hold X = gO = 0 and P = 0: finite everywhere, no contribution.  No atomics.
#include "mfma_tile.h"

namespace {

constexpr int kMaxF = RH_CIN_MAX_F;  // fields of a (B, F, D) block
constexpr int kMaxD = RH_SA_MAX_D;   // self-attention width
static_assert(kMaxF == kT, "a tile holds at least one whole sample");
static_assert(kMaxD == kT, "a projection is one tile wide and the 4 D D weight gradients are 64 accumulators per lane");
constexpr int kFwdGrid = 512;  // persistent workgroups: two per CU, which registers and LDS allow up to D = 32
constexpr int kBwdGrid = 256;  // one per CU, all that the backward's registers allow; also the rows of `part`

struct IaArgs {
  const float* x;     // (B, F, D)
  const float* w[4];  // (D, D) each: W_Q, W_K, W_V, W_Res (null: no residual)
  const float* y;     // backward: the forward's output, its lse and the upstream gradient
  const float* lse_in;
  const float* gy;
  float* out;         // forward: y and lse (B, H, F)
  float* lse;
  float* gx;          // backward: (B, F, D) or null
  float* part;        // backward: (gridDim.x, 4 D D) or null
  float scale;
  int B, F, D, H, G, ntiles;
};

struct Lane {
  int li, kk, wm, wn;
};

__device__ __forceinline__ Lane lane_of(int tid) {
  const int lane = tid % RH_WAVE, wv = tid / RH_WAVE;
  return Lane{lane % 32, lane / 32, wv & 1, wv >> 1};
}

// acc += A (M x K) B (K x N) on the workgroup tile, A[i][k] = a[i * ai + k * ak], B[k][j] = b[k * bk + j * bj] (LDS);
// M, N <= 64, any K
__device__ __forceinline__ v16f tile_mma(v16f acc, const float* a, int ai, int ak, const float* b, int bk, int bj, int K, int M,
                                         int N, const Lane& l) {
  if (32 * l.wm >= M || 32 * l.wn >= N) return acc;  // (wavefront-uniform)
  const float* ap = a + min(32 * l.wm + l.li, M - 1) * ai;
  const float* bp = b + min(32 * l.wn + l.li, N - 1) * bj;
  acc = mma_lds(acc, ap, 0, ak, bp, bk, 0, K & ~1, l.li, l.kk);
  if (K & 1) {
    const float av = l.kk == 0 ? ap[(K - 1) * ak] : 0.f;
    const float bv = l.kk == 0 ? bp[(K - 1) * bk] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
  }
  return acc;
}

// dst[row * ld + col] = mul * C[row][col] for row < M, col < N
__device__ __forceinline__ void tile_store(const v16f& acc, float* dst, int ld, int M, int N, const Lane& l, float mul = 1.f) {
  const int col = 32 * l.wn + l.li;
  if (32 * l.wm >= M || col >= N) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = 32 * l.wm + acc_row(r, l.kk);
    if (row < M) dst[row * ld + col] = mul * acc[r];
  }
}

// s[k * kLd + j] = w[k * D + j] (transposed: s[j * kLd + k])
__device__ __forceinline__ void stage_weight(float* s, const float* w, int D, bool transposed, int tid) {
  for (int e = tid; e < D * D; e += RH_BLOCK) {
    const int k = e / D, j = e - k * D;
    s[transposed ? j * kLd + k : k * kLd + j] = w[e];
  }
}

__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 1, RH_WAVE);
  return v + __shfl_xor(v, 2, RH_WAVE);
}

__global__ __launch_bounds__(RH_BLOCK) void interact_fwd_kernel(const IaArgs a) {
  extern __shared__ float lds[];
  const int F = a.F, D = a.D, dh = D / a.H, ldx = D | 1, GF = a.G * F;
  float* sX = lds;                  // [64][ldx]
  float* sQ = sX + kT * ldx;        // [4][64][ldx]: Q, K, V, R of all heads
  float* sK = sQ + kT * ldx;
  float* sV = sK + kT * ldx;
  float* sR = sV + kT * ldx;
  float* sP = sR + kT * ldx;        // [64][kLd]: a weight, transposed; then the scores / softmax of one head
  const int tid = threadIdx.x;
  const Lane l = lane_of(tid);
  const int nproj = a.w[3] != nullptr ? 4 : 3;
  const int r4 = tid >> 2, q4 = tid & 3;  // softmax: four lanes per row
  const int g4 = r4 / F, k0 = g4 * F;     // the row's sample and its first key
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int64_t row0 = (int64_t)t * GF;
    const int64_t left = (int64_t)a.B * F - row0;
    const int nv = left < GF ? (int)left : GF;  // rows of the tile that exist
    __syncthreads();  // (the previous tile is done with the LDS)
    for (int e = tid; e < kT * ldx; e += RH_BLOCK) {
      const int r = e / ldx, c = e - r * ldx;
      sX[e] = (r < nv && c < D) ? a.x[(row0 + r) * D + c] : 0.f;
    }
    for (int p = 0; p < nproj; ++p) {
      __syncthreads();  // (sX is written; the previous product is done with sP)
      stage_weight(sP, a.w[p], D, true, tid);
      __syncthreads();
      const v16f acc = tile_mma(zero16(), sX, ldx, 1, sP, kLd, 1, D, kT, D, l);
      tile_store(acc, sQ + p * kT * ldx, ldx, kT, D, l);
    }
    for (int h = 0; h < a.H; ++h) {
      const int c0 = h * dh;
      __syncthreads();  // (Q, K, V, R are written; the previous head is done with sP)
      const v16f s = tile_mma(zero16(), sQ + c0, ldx, 1, sK + c0, 1, ldx, dh, kT, kT, l);
      tile_store(s, sP, kLd, kT, kT, l, a.scale);
      __syncthreads();
      {
        float* pr = sP + r4 * kLd;
        const bool live = r4 < GF;
        float m = -INFINITY;
        if (live)
          for (int c = k0 + q4; c < k0 + F; c += 4) m = fmaxf(m, pr[c]);
        m = fmaxf(m, __shfl_xor(m, 1, RH_WAVE));
        m = fmaxf(m, __shfl_xor(m, 2, RH_WAVE));
        float sum = 0.f;
        if (live)
          for (int c = k0 + q4; c < k0 + F; c += 4) sum += expf(pr[c] - m);
        sum = quad_sum(sum);
        const float inv = live ? 1.f / sum : 0.f;
        for (int c = q4; c < kT; c += 4) {
          const bool in = live && c >= k0 && c < k0 + F;
          pr[c] = in ? expf(pr[c] - m) * inv : 0.f;
        }
        if (q4 == 0 && r4 < nv) a.lse[(((int64_t)t * a.G + g4) * a.H + h) * F + (r4 - k0)] = m + logf(sum);
      }
      __syncthreads();
      const v16f o = tile_mma(zero16(), sP, kLd, 1, sV + c0, ldx, 1, kT, kT, dh, l);
      const int col = 32 * l.wn + l.li;
      if (col < dh) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * l.wm + acc_row(r, l.kk);
          if (row < nv) {
            const float res = nproj == 4 ? sR[row * ldx + c0 + col] : 0.f;
            a.out[(row0 + row) * D + c0 + col] = fmaxf(o[r] + res, 0.f);
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(RH_BLOCK) void interact_bwd_kernel(const IaArgs a) {
  extern __shared__ float lds[];
  const int F = a.F, D = a.D, dh = D / a.H, ldx = D | 1, GF = a.G * F;
  float* sX = lds;                  // [64][ldx]
  float* sQ = sX + kT * ldx;        // [4][64][ldx]: Q, K, V of all heads, then gQ, gK, gV; gO = g_y [y > 0]
  float* sK = sQ + kT * ldx;
  float* sV = sK + kT * ldx;
  float* sG = sV + kT * ldx;
  float* sP = sG + kT * ldx;        // [64][kLd]: the scores, then P, of one head
  float* sT = sP + kT * kLd;        // [64][kLd]: a weight; gP, then gS, of one head
  const int tid = threadIdx.x;
  const Lane l = lane_of(tid);
  const int nproj = a.w[3] != nullptr ? 4 : 3;
  const int r4 = tid >> 2, q4 = tid & 3;
  const int g4 = r4 / F, k0 = g4 * F;
  v16f wacc[4];  // the workgroup's sums of g_W_p = G_p^T X over its tiles
#pragma unroll
  for (int p = 0; p < 4; ++p) wacc[p] = zero16();
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int64_t row0 = (int64_t)t * GF;
    const int64_t left = (int64_t)a.B * F - row0;
    const int nv = left < GF ? (int)left : GF;
    __syncthreads();  // (the previous tile is done with the LDS)
    for (int e = tid; e < kT * ldx; e += RH_BLOCK) {
      const int r = e / ldx, c = e - r * ldx;
      const bool in = r < nv && c < D;
      const int64_t at = in ? (row0 + r) * D + c : 0;
      sX[e] = in ? a.x[at] : 0.f;
      sG[e] = (in && a.y[at] > 0.f) ? a.gy[at] : 0.f;
    }
    for (int p = 0; p < 3; ++p) {
      __syncthreads();  // (sX is written; the previous product is done with sT)
      stage_weight(sT, a.w[p], D, true, tid);
      __syncthreads();
      const v16f acc = tile_mma(zero16(), sX, ldx, 1, sT, kLd, 1, D, kT, D, l);
      tile_store(acc, sQ + p * kT * ldx, ldx, kT, D, l);
    }
    for (int h = 0; h < a.H; ++h) {
      const int c0 = h * dh;
      __syncthreads();  // (Q, K, V are written; the previous head is done with sP and sT)
      const v16f s = tile_mma(zero16(), sQ + c0, ldx, 1, sK + c0, 1, ldx, dh, kT, kT, l);
      const v16f gp = tile_mma(zero16(), sG + c0, ldx, 1, sV + c0, 1, ldx, dh, kT, kT, l);
      tile_store(s, sP, kLd, kT, kT, l, a.scale);
      tile_store(gp, sT, kLd, kT, kT, l);
      __syncthreads();
      {
        float* pr = sP + r4 * kLd;
        float* tr = sT + r4 * kLd;
        const bool live = r4 < nv;  // (a sample past B has no lse: its rows are dead)
        const float lse = live ? a.lse_in[(((int64_t)t * a.G + g4) * a.H + h) * F + (r4 - k0)] : 0.f;
        // lse is rounded at its own magnitude (6e-5 at 1e3), which scales the whole row by e^eps: harmless in the forward,
        // but gS sums to zero over a row only when P sums to one, so the row is renormalised (z = 1 to that rounding)
        float dot = 0.f, z = 0.f;
        if (live)
          for (int c = k0 + q4; c < k0 + F; c += 4) {
            const float e = expf(pr[c] - lse);
            z += e;
            dot = fmaf(e, tr[c], dot);
          }
        z = quad_sum(z);
        const float inv = live ? 1.f / z : 0.f;
        dot = quad_sum(dot) * inv;
        for (int c = q4; c < kT; c += 4) {
          const bool in = live && c >= k0 && c < k0 + F;
          const float pv = in ? expf(pr[c] - lse) * inv : 0.f;
          pr[c] = pv;
          tr[c] = in ? a.scale * pv * (tr[c] - dot) : 0.f;
        }
      }
      __syncthreads();
      const v16f gv = tile_mma(zero16(), sP, 1, kLd, sG + c0, ldx, 1, kT, kT, dh, l);  // P^T gO_h
      const v16f gk = tile_mma(zero16(), sT, 1, kLd, sQ + c0, ldx, 1, kT, kT, dh, l);  // gS^T Q_h
      const v16f gq = tile_mma(zero16(), sT, kLd, 1, sK + c0, ldx, 1, kT, kT, dh, l);  // gS K_h
      __syncthreads();  // (every wavefront has read Q_h and K_h)
      tile_store(gq, sQ + c0, ldx, kT, dh, l);
      tile_store(gk, sK + c0, ldx, kT, dh, l);
      tile_store(gv, sV + c0, ldx, kT, dh, l);
    }
    if (a.gx != nullptr) {
      v16f gx = zero16();
      for (int p = 0; p < nproj; ++p) {
        __syncthreads();  // (gQ, gK, gV are written; the previous product is done with sT)
        stage_weight(sT, a.w[p], D, false, tid);
        __syncthreads();
        gx = tile_mma(gx, sQ + p * kT * ldx, ldx, 1, sT, kLd, 1, D, kT, D, l);
      }
      const int col = 32 * l.wn + l.li;
      if (col < D) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * l.wm + acc_row(r, l.kk);
          if (row < nv) a.gx[(row0 + row) * D + col] = gx[r];
        }
      }
    }
    if (a.part != nullptr) {
      __syncthreads();  // (gQ, gK, gV are written)
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (p < nproj) wacc[p] = tile_mma(wacc[p], sQ + p * kT * ldx, 1, ldx, sX, ldx, 1, kT, D, D, l);
    }
  }
  if (a.part != nullptr) {
    float* part = a.part + (int64_t)blockIdx.x * 4 * D * D;
#pragma unroll
    for (int p = 0; p < 4; ++p) tile_store(wacc[p], part + p * D * D, D, D, D, l);
  }
}

int check_shape(const char* who, int B, int F, int D, int H) {
  RH_REQUIRE(B >= 0, RH_E_BADARG, "%s: bad batch size %d", who, B);
  RH_REQUIRE(F >= 1 && F <= kMaxF, RH_E_UNSUPPORTED, "%s: num_fields %d unsupported (1 .. %d)", who, F, kMaxF);
  RH_REQUIRE(D >= 1 && D <= kMaxD, RH_E_UNSUPPORTED, "%s: embed_dim %d unsupported (1 .. %d)", who, D, kMaxD);
  RH_REQUIRE(H >= 1, RH_E_UNSUPPORTED, "%s: num_heads %d unsupported (>= 1)", who, H);
  RH_REQUIRE(D % H == 0, RH_E_BADARG, "%s: embed_dim %d is not a multiple of num_heads %d", who, D, H);
  return 0;
}

int tiles_of(int B, int F) {
  const int G = kT / F;
  return (int)(((int64_t)B + G - 1) / G);
}

size_t fwd_lds(int D) { return sizeof(float) * (size_t)(5 * kT * (D | 1) + kT * kLd); }
size_t bwd_lds(int D) { return sizeof(float) * (size_t)(5 * kT * (D | 1) + 2 * kT * kLd); }

IaArgs make_args(const float* x, const float* w_q, const float* w_k, const float* w_v, const float* w_res, float scale, int B,
                 int F, int D, int H) {
  IaArgs a{};
  a.x = x;
  a.w[0] = w_q;
  a.w[1] = w_k;
  a.w[2] = w_v;
  a.w[3] = w_res;
  a.scale = scale;
  a.B = B;
  a.F = F;
  a.D = D;
  a.H = H;
  a.G = kT / F;
  a.ntiles = tiles_of(B, F);
  return a;
}

}  // namespace

extern "C" int rh_interact_plan(int B, int F, int D, int H, int* ntiles, int* nblocks) {
  RH_REQUIRE(ntiles != nullptr && nblocks != nullptr, RH_E_BADARG, "rh_interact_plan: null pointer");
  if (int rc = check_shape("rh_interact_plan", B, F, D, H)) return rc;
  *ntiles = tiles_of(B, F);
  *nblocks = *ntiles < kBwdGrid ? *ntiles : kBwdGrid;
  return 0;
}

extern "C" int rh_interact_fwd(const float* x, const float* w_q, const float* w_k, const float* w_v, const float* w_res,
                               float scale, int B, int F, int D, int H, float* y, float* lse, void* stream) {
  RH_REQUIRE(x && w_q && w_k && w_v && y && lse, RH_E_BADARG, "rh_interact_fwd: null argument");
  if (int rc = check_shape("rh_interact_fwd", B, F, D, H)) return rc;
  if (B == 0) return 0;
  static RhLdsReserved reserved;
  if (int rc = rh_reserve_lds(reserved, interact_fwd_kernel, fwd_lds(kMaxD), "rh_interact_fwd")) return rc;
  IaArgs a = make_args(x, w_q, w_k, w_v, w_res, scale, B, F, D, H);
  a.out = y;
  a.lse = lse;
  const unsigned grid = (unsigned)(a.ntiles < kFwdGrid ? a.ntiles : kFwdGrid);
  hipLaunchKernelGGL(interact_fwd_kernel, dim3(grid), dim3(RH_BLOCK), fwd_lds(D), reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_interact_fwd");
  return 0;
}

extern "C" int rh_interact_bwd(const float* x, const float* w_q, const float* w_k, const float* w_v, const float* w_res,
                               float scale, const float* y, const float* lse, const float* g_y, int B, int F, int D, int H,
                               float* g_x, float* part, void* stream) {
  RH_REQUIRE(x && w_q && w_k && w_v && y && lse && g_y && (g_x || part), RH_E_BADARG, "rh_interact_bwd: null argument");
  if (int rc = check_shape("rh_interact_bwd", B, F, D, H)) return rc;
  if (B == 0) return 0;
  static RhLdsReserved reserved;
  if (int rc = rh_reserve_lds(reserved, interact_bwd_kernel, bwd_lds(kMaxD), "rh_interact_bwd")) return rc;
  IaArgs a = make_args(x, w_q, w_k, w_v, w_res, scale, B, F, D, H);
  a.y = y;
  a.lse_in = lse;
  a.gy = g_y;
  a.gx = g_x;
  a.part = part;
  const unsigned grid = (unsigned)(a.ntiles < kBwdGrid ? a.ntiles : kBwdGrid);
  hipLaunchKernelGGL(interact_bwd_kernel, dim3(grid), dim3(RH_BLOCK), bwd_lds(D), reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_interact_bwd");
  return 0;
}
