// Score tails and the field gate of the remaining two-tower models, one launch each way.
//
// (a) rh_band_logits_*: YoutubeSBC.forward, torch_rechub/models/matching/youtube_sbc.py:61-80
//       pred = torch.cosine_similarity(u.unsqueeze(1), v, dim=2)      # (B, B): every pair
//       scores = (pred - log(w))[index0, index1] / T                   # 1 + n_neg entries per row, on a fixed band
//     index1[i, k] = (i + k) mod B, so only B (1 + n_neg) D of the B^2 D multiply-adds are ever read.  Here the band is
//     computed straight from the tower outputs (one wavefront per row, as csrc/match.hip's in-batch logits), and because
//     every item row r is used by exactly the user rows (r - k) mod B, the item gradient is a GATHER in ascending k: no
//     atomics, no zeroed buffer, the same bits on every run.
// (b) rh_pair_cosine_*: FaceBookDSSM's three F.normalize calls and two multiply-sum reductions
//     (torch_rechub/models/matching/dssm_facebook.py:52-53,64,75-76) and their autograd.
// (c) rh_senet_*: SENETLayer.forward (torch_rechub/basic/layers.py:525-529: mean, Linear, ReLU, Linear, ReLU, scale) over the
//     (B, F, D) field block, the two weight matrices staged in LDS; the weight gradients leave as one partial per workgroup
//     (summed in a fixed order by rh_colsum): no float atomics.
// Same numbers as the reference up to the summation order of a D-term (F-term) sum.  Latency- and gather-bound.  Measured
// (profiles/twotower_bench.txt; tail forward + backward through autograd, one MI355X): band logits at B = 4096,
// D = 64, n_neg = 3: 85 us against 56 ms for the torch formulation, 0.09 MiB against 12.5 GiB of peak forward memory; pair
// cosine 110-126 us against 327-352 us; SENET gate 97-101 us against 223-228 us.  The fused figures are host launch cost;
// the kernels' own times are unmeasured.
#include "common.h"

namespace {

constexpr int kWaves = RH_BLOCK / RH_WAVE;
constexpr int kMaxPerLane = 16;
static_assert(RH_WAVE * kMaxPerLane == RH_TWOTOWER_MAX_D, "a row's D values are dealt over one wavefront");
constexpr int kGridCap = 1024;   // workgroups; more rows than kGridCap * kWaves take further trips of the row loop

int grid_for(int B) {
  int64_t grid = ((int64_t)B + kWaves - 1) / kWaves;
  return (int)(grid > kGridCap ? kGridCap : grid);
}

#define RH_PL_DISPATCH(KERNEL, D, grid, s, args)                                                                   \
  do {                                                                                                             \
    const int pl_ = ((D) + RH_WAVE - 1) / RH_WAVE;                                                                 \
    const dim3 g_((unsigned)(grid)), b_(RH_BLOCK);                                                                 \
    if (pl_ <= 1) hipLaunchKernelGGL((KERNEL<1>), g_, b_, 0, s, args);                                             \
    else if (pl_ <= 2) hipLaunchKernelGGL((KERNEL<2>), g_, b_, 0, s, args);                                        \
    else if (pl_ <= 4) hipLaunchKernelGGL((KERNEL<4>), g_, b_, 0, s, args);                                        \
    else if (pl_ <= 8) hipLaunchKernelGGL((KERNEL<8>), g_, b_, 0, s, args);                                        \
    else hipLaunchKernelGGL((KERNEL<kMaxPerLane>), g_, b_, 0, s, args);                                            \
  } while (0)

template <int PL>
static __device__ __forceinline__ void load_row(const float* __restrict__ p, int D, int lane, float (&r)[PL]) {
#pragma unroll
  for (int e = 0; e < PL; ++e) {
    const int d = lane + e * RH_WAVE;
    r[e] = d < D ? p[d] : 0.f;
  }
}

template <int PL>
static __device__ __forceinline__ float row_dot(const float (&a)[PL], const float (&b)[PL]) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < PL; ++e) s = fmaf(a[e], b[e], s);
  return wave_sum(s);
}

// ---- (a) band logits ---------------------------------------------------------------------------------------------------
struct BandArgs {
  const float* u;  // (B, D), row stride ldu
  int64_t ldu;
  const float* v;  // (B, D), row stride ldv
  int64_t ldv;
  const float* w;   // (B,) sample weights            forward
  const float* nu;  // (B,) ||u_i||                   written by the forward, read by the backward
  const float* nv;  // (B,) ||v_j||
  const float* g;   // (B, K1)                        backward
  float* logits;    // (B, K1)                        forward
  float* nu_out;
  float* nv_out;
  float* g_u;  // (B, D)                              backward
  float* g_v;  // (B, D)
  int B, D, K1;
  float inv_t, eps;
};

template <int PL>
__global__ __launch_bounds__(RH_BLOCK) void band_fwd_kernel(const BandArgs a) {
  RH_CHAIN_PRIO();
  const int lane = threadIdx.x % RH_WAVE, wave = threadIdx.x / RH_WAVE;
  for (int64_t i = (int64_t)blockIdx.x * kWaves + wave; i < a.B; i += (int64_t)gridDim.x * kWaves) {
    float ur[PL], vr[PL];
    load_row<PL>(a.u + i * a.ldu, a.D, lane, ur);
    const float nu = sqrtf(row_dot<PL>(ur, ur));
    const float inv_nu = 1.f / fmaxf(nu, a.eps);
    if (lane == 0) a.nu_out[i] = nu;
    for (int k = 0; k < a.K1; ++k) {  // wavefront-uniform
      int64_t j = i + k;
      if (j >= a.B) j -= a.B;  // K1 <= B: one wrap at most
      load_row<PL>(a.v + j * a.ldv, a.D, lane, vr);
      const float nv = sqrtf(row_dot<PL>(vr, vr));
      const float dot = row_dot<PL>(ur, vr);
      if (lane == 0) {
        if (k == 0) a.nv_out[i] = nv;  // j == i: every item row's norm is written by the wavefront of its own row
        a.logits[i * a.K1 + k] = (dot * inv_nu * (1.f / fmaxf(nv, a.eps)) - logf(a.w[j])) * a.inv_t;
      }
    }
  }
}

// With c = u^ . v^, u^ = u / Nu, v^ = v / Nv, Nu = max(||u||, eps).  ATen's cosine_similarity clamps the two norms in
// place OUTSIDE autograd, so its gradient treats Nu as ||u|| even where eps replaced it (checked against the recorded
// gradients of tests/golden/twotower_layers.npz; F.normalize's clamp_min, a constant denominator there, differs):
//   dc/du = (v^ - c u / ||u||) / Nu = (v^ - (Nu / ||u||) c u^) / Nu,   and v^ / Nu for a zero row (the norm's gradient at 0 is 0)
// so g_u[r] = (A - (Nu / ||u||) (u^ . A) u^) / Nu with A = sum_k s[r, k] v^_(r + k), s = g / T, and the same for g_v[r] over
// the rows (r - k) mod B: one wavefront reduction per output row.
template <int PL>
__global__ __launch_bounds__(RH_BLOCK) void band_bwd_kernel(const BandArgs a) {
  RH_CHAIN_PRIO();
  const int lane = threadIdx.x % RH_WAVE, wave = threadIdx.x / RH_WAVE;
  for (int64_t r = (int64_t)blockIdx.x * kWaves + wave; r < a.B; r += (int64_t)gridDim.x * kWaves) {
    float own[PL], other[PL], acc[PL];
    {  // g_u[r]
      load_row<PL>(a.u + r * a.ldu, a.D, lane, own);
      const float n = a.nu[r];
      const float inv = 1.f / fmaxf(n, a.eps);
#pragma unroll
      for (int e = 0; e < PL; ++e) {
        own[e] /= fmaxf(n, a.eps);
        acc[e] = 0.f;
      }
      for (int k = 0; k < a.K1; ++k) {
        int64_t j = r + k;
        if (j >= a.B) j -= a.B;
        load_row<PL>(a.v + j * a.ldv, a.D, lane, other);
        const float s = a.g[r * a.K1 + k] * a.inv_t * (1.f / fmaxf(a.nv[j], a.eps));
#pragma unroll
        for (int e = 0; e < PL; ++e) acc[e] = fmaf(s, other[e], acc[e]);
      }
      const float proj = n > 0.f ? row_dot<PL>(own, acc) * (fmaxf(n, a.eps) / n) : 0.f;
#pragma unroll
      for (int e = 0; e < PL; ++e) {
        const int d = lane + e * RH_WAVE;
        if (d < a.D) a.g_u[r * a.D + d] = fmaf(-proj, own[e], acc[e]) * inv;
      }
    }
    {  // g_v[r]: the user rows (r - k) mod B, ascending k
      load_row<PL>(a.v + r * a.ldv, a.D, lane, own);
      const float n = a.nv[r];
      const float inv = 1.f / fmaxf(n, a.eps);
#pragma unroll
      for (int e = 0; e < PL; ++e) {
        own[e] /= fmaxf(n, a.eps);
        acc[e] = 0.f;
      }
      for (int k = 0; k < a.K1; ++k) {
        int64_t i = r - k;
        if (i < 0) i += a.B;
        load_row<PL>(a.u + i * a.ldu, a.D, lane, other);
        const float s = a.g[i * a.K1 + k] * a.inv_t * (1.f / fmaxf(a.nu[i], a.eps));
#pragma unroll
        for (int e = 0; e < PL; ++e) acc[e] = fmaf(s, other[e], acc[e]);
      }
      const float proj = n > 0.f ? row_dot<PL>(own, acc) * (fmaxf(n, a.eps) / n) : 0.f;
#pragma unroll
      for (int e = 0; e < PL; ++e) {
        const int d = lane + e * RH_WAVE;
        if (d < a.D) a.g_v[r * a.D + d] = fmaf(-proj, own[e], acc[e]) * inv;
      }
    }
  }
}

int band_check(const char* who, int B, int D, int K1, float temperature, float eps) {
  RH_REQUIRE(B >= 1 && K1 >= 1 && temperature != 0.f && eps >= 0.f, RH_E_BADARG, "%s: bad shape B=%d K1=%d temperature=%g eps=%g",
             who, B, K1, (double)temperature, (double)eps);
  RH_REQUIRE(K1 <= B, RH_E_UNSUPPORTED, "%s: 1 + n_neg = %d columns from a batch of %d rows (the band wraps once at most)", who,
             K1, B);
  RH_REQUIRE(D >= 1 && D <= RH_WAVE * kMaxPerLane, RH_E_UNSUPPORTED, "%s: embedding width %d unsupported (max %d)", who, D,
             RH_WAVE * kMaxPerLane);
  return 0;
}

// ---- (b) pair cosine ---------------------------------------------------------------------------------------------------
struct PairArgs {
  const float* hu;
  int64_t ldu;
  const float* hp;
  int64_t ldp;
  const float* hn;
  int64_t ldn;
  const float* nrm;    // (3, B): ||hu||, ||hp||, ||hn||    backward
  const float* g_pos;  // (B,)
  const float* g_neg;  // (B,)
  float* pos;          // (B,)                              forward
  float* neg;          // (B,)
  float* nrm_out;      // (3, B)
  float* g_hu;         // (B, D) each                       backward
  float* g_hp;
  float* g_hn;
  int B, D;
  float eps;
};

template <int PL>
__global__ __launch_bounds__(RH_BLOCK) void pair_fwd_kernel(const PairArgs a) {
  RH_CHAIN_PRIO();
  const int lane = threadIdx.x % RH_WAVE, wave = threadIdx.x / RH_WAVE;
  for (int64_t i = (int64_t)blockIdx.x * kWaves + wave; i < a.B; i += (int64_t)gridDim.x * kWaves) {
    float u[PL], p[PL];
    load_row<PL>(a.hu + i * a.ldu, a.D, lane, u);
    const float nu = sqrtf(row_dot<PL>(u, u));
    const float inv_u = 1.f / fmaxf(nu, a.eps);
    load_row<PL>(a.hp + i * a.ldp, a.D, lane, p);
    const float np_ = sqrtf(row_dot<PL>(p, p));
    const float pos = row_dot<PL>(u, p) * inv_u * (1.f / fmaxf(np_, a.eps));
    load_row<PL>(a.hn + i * a.ldn, a.D, lane, p);  // the same instruction sequence: hp == hn gives pos == neg bitwise
    const float nn = sqrtf(row_dot<PL>(p, p));
    const float neg = row_dot<PL>(u, p) * inv_u * (1.f / fmaxf(nn, a.eps));
    if (lane == 0) {
      a.pos[i] = pos;
      a.neg[i] = neg;
      a.nrm_out[i] = nu;
      a.nrm_out[(int64_t)a.B + i] = np_;
      a.nrm_out[2 * (int64_t)a.B + i] = nn;
    }
  }
}

template <int PL>
__global__ __launch_bounds__(RH_BLOCK) void pair_bwd_kernel(const PairArgs a) {
  RH_CHAIN_PRIO();
  const int lane = threadIdx.x % RH_WAVE, wave = threadIdx.x / RH_WAVE;
  for (int64_t i = (int64_t)blockIdx.x * kWaves + wave; i < a.B; i += (int64_t)gridDim.x * kWaves) {
    float u[PL], p[PL], n[PL];
    const float nu = a.nrm[i], np_ = a.nrm[(int64_t)a.B + i], nn = a.nrm[2 * (int64_t)a.B + i];
    const float du = fmaxf(nu, a.eps), dp = fmaxf(np_, a.eps), dn = fmaxf(nn, a.eps);
    const float inv_u = 1.f / du, inv_p = 1.f / dp, inv_n = 1.f / dn;
    load_row<PL>(a.hu + i * a.ldu, a.D, lane, u);
    load_row<PL>(a.hp + i * a.ldp, a.D, lane, p);
    load_row<PL>(a.hn + i * a.ldn, a.D, lane, n);
#pragma unroll
    for (int e = 0; e < PL; ++e) {
      u[e] /= du;  // (a true division: a row of width 1 normalises to exactly +-1, so its gradient is exactly 0)
      p[e] /= dp;
      n[e] /= dn;
    }
    const float pos = row_dot<PL>(u, p), neg = row_dot<PL>(u, n);
    const float gp = a.g_pos[i], gn = a.g_neg[i];
    const float cu = nu > a.eps ? fmaf(gp, pos, gn * neg) : 0.f;
    const float cp = np_ > a.eps ? pos : 0.f, cn = nn > a.eps ? neg : 0.f;
#pragma unroll
    for (int e = 0; e < PL; ++e) {
      const int d = lane + e * RH_WAVE;
      if (d < a.D) {
        a.g_hu[i * a.D + d] = (fmaf(gp, p[e], gn * n[e]) - cu * u[e]) * inv_u;
        a.g_hp[i * a.D + d] = gp * fmaf(-cp, p[e], u[e]) * inv_p;
        a.g_hn[i * a.D + d] = gn * fmaf(-cn, n[e], u[e]) * inv_n;
      }
    }
  }
}

int pair_check(const char* who, int B, int D, float eps) {
  RH_REQUIRE(B >= 1 && eps >= 0.f, RH_E_BADARG, "%s: bad shape B=%d eps=%g", who, B, (double)eps);
  RH_REQUIRE(D >= 1 && D <= RH_WAVE * kMaxPerLane, RH_E_UNSUPPORTED, "%s: embedding width %d unsupported (max %d)", who, D,
             RH_WAVE * kMaxPerLane);
  return 0;
}

// ---- (c) SENET gate ----------------------------------------------------------------------------------------------------
constexpr int kMaxFields = RH_SENET_MAX_F;
constexpr int kMaxFieldDim = RH_SENET_MAX_D;
constexpr int kWeightRegs = kMaxFields * kMaxFields / RH_BLOCK;  // weight-gradient elements per thread

struct SenetArgs {
  const float* x;  // (B, F, D): sample stride ldx, a sample's F D values contiguous
  int64_t ldx;
  const float* w1;  // (R, F)
  const float* w2;  // (F, R)
  const float* z;   // (B, F)   written by the forward, read by the backward
  const float* h;   // (B, R)
  const float* a;   // (B, F)
  const float* g;   // (B, F, D), sample stride ldg       backward
  int64_t ldg;
  float* y;  // (B, F D)                                   forward
  float* z_out;
  float* h_out;
  float* a_out;
  float* g_x;      // (B, F D)                             backward
  float* partial;  // (gridDim.x, 2 R F): [g_W1 (R, F) | g_W2 (F, R)] per workgroup
  int B, F, R, D;
};

// G = lanes per field (the power of two >= min(D, 64)), 64 / G fields per pass of the wavefront over a sample
static __device__ __forceinline__ int lanes_per_field(int D) {
  int G = 1;
  while (G < D && G < RH_WAVE) G <<= 1;
  return G;
}

__global__ __launch_bounds__(RH_BLOCK) void senet_fwd_kernel(const SenetArgs p) {
  RH_CHAIN_PRIO();
  __shared__ float w1t[kMaxFields * kMaxFields];  // [f * R + r]
  __shared__ float w2t[kMaxFields * kMaxFields];  // [r * F + f]
  __shared__ float zs[kWaves][kMaxFields], hs[kWaves][kMaxFields], as[kWaves][kMaxFields];
  const int lane = threadIdx.x % RH_WAVE, wave = threadIdx.x / RH_WAVE;
  const int F = p.F, R = p.R, D = p.D;
  for (int e = threadIdx.x; e < R * F; e += RH_BLOCK) {
    w1t[(e % F) * R + e / F] = p.w1[e];  // w1[r, f], e = r F + f
    w2t[(e % R) * F + e / R] = p.w2[e];  // w2[f, r], e = f R + r
  }
  const int G = lanes_per_field(D), per_pass = RH_WAVE / G, q = lane % G, slot = lane / G;
  const float inv_d = 1.f / (float)D;
  for (int64_t b0 = (int64_t)blockIdx.x * kWaves; b0 < p.B; b0 += (int64_t)gridDim.x * kWaves) {  // uniform per workgroup
    const int64_t b = b0 + wave;
    const bool live = b < p.B;
    const float* xr = p.x + (live ? b : 0) * p.ldx;
    for (int f0 = 0; f0 < F; f0 += per_pass) {
      const int f = f0 + slot;
      float s = 0.f;
      if (live && f < F)
        for (int d = q; d < D; d += G) s += xr[f * D + d];
      for (int m = 1; m < G; m <<= 1) s += __shfl_xor(s, m, RH_WAVE);
      if (q == 0 && f < F) zs[wave][f] = s * inv_d;
    }
    __syncthreads();  // (also: the staged weights, on the first trip)
    if (lane < R) {
      float s = 0.f;
      for (int f = 0; f < F; ++f) s = fmaf(w1t[f * R + lane], zs[wave][f], s);
      hs[wave][lane] = fmaxf(s, 0.f);
    }
    __syncthreads();
    if (lane < F) {
      float s = 0.f;
      for (int r = 0; r < R; ++r) s = fmaf(w2t[r * F + lane], hs[wave][r], s);
      as[wave][lane] = fmaxf(s, 0.f);
    }
    __syncthreads();
    if (live) {
      if (lane < F) {
        p.z_out[b * F + lane] = zs[wave][lane];
        p.a_out[b * F + lane] = as[wave][lane];
      }
      if (lane < R) p.h_out[b * R + lane] = hs[wave][lane];
      float* yr = p.y + b * (int64_t)F * D;
      for (int f0 = 0; f0 < F; f0 += per_pass) {
        const int f = f0 + slot;
        if (f < F) {
          const float gate = as[wave][f];
          for (int d = q; d < D; d += G) yr[f * D + d] = xr[f * D + d] * gate;
        }
      }
    }
    __syncthreads();  // the next trip overwrites zs / hs / as
  }
}

// y = x a:  g_a[f] = sum_d g[f, d] x[f, d],  g_x[f, d] = g[f, d] a[f] + g_z[f] / D;  through the two ReLU layers (derivative 0
// at 0) g_a -> g_h -> g_z.  g_W2[f, r] = sum_b g_a'[b, f] h[b, r], g_W1[r, f] = sum_b g_h'[b, r] z[b, f]: every thread keeps
// its elements of both in registers over the workgroup's samples (ascending b) and writes them once.
__global__ __launch_bounds__(RH_BLOCK) void senet_bwd_kernel(const SenetArgs p) {
  RH_CHAIN_PRIO();
  __shared__ float w1s[kMaxFields * kMaxFields];  // [r * F + f]
  __shared__ float w2s[kMaxFields * kMaxFields];  // [f * R + r]
  __shared__ float zs[kWaves][kMaxFields], hs[kWaves][kMaxFields], gas[kWaves][kMaxFields], ghs[kWaves][kMaxFields],
      gzs[kWaves][kMaxFields];
  const int lane = threadIdx.x % RH_WAVE, wave = threadIdx.x / RH_WAVE;
  const int F = p.F, R = p.R, D = p.D, RF = R * F;
  for (int e = threadIdx.x; e < RF; e += RH_BLOCK) {
    w1s[e] = p.w1[e];
    w2s[e] = p.w2[e];
  }
  float acc1[kWeightRegs], acc2[kWeightRegs];
#pragma unroll
  for (int t = 0; t < kWeightRegs; ++t) acc1[t] = acc2[t] = 0.f;
  const int G = lanes_per_field(D), per_pass = RH_WAVE / G, q = lane % G, slot = lane / G;
  const float inv_d = 1.f / (float)D;
  for (int64_t b0 = (int64_t)blockIdx.x * kWaves; b0 < p.B; b0 += (int64_t)gridDim.x * kWaves) {  // uniform per workgroup
    const int64_t b = b0 + wave;
    const bool live = b < p.B;
    const float* xr = p.x + (live ? b : 0) * p.ldx;
    const float* gr = p.g + (live ? b : 0) * p.ldg;
    if (lane < F) zs[wave][lane] = live ? p.z[b * F + lane] : 0.f;
    if (lane < R) hs[wave][lane] = live ? p.h[b * R + lane] : 0.f;
    for (int f0 = 0; f0 < F; f0 += per_pass) {
      const int f = f0 + slot;
      float s = 0.f;
      if (live && f < F)
        for (int d = q; d < D; d += G) s = fmaf(gr[f * D + d], xr[f * D + d], s);
      for (int m = 1; m < G; m <<= 1) s += __shfl_xor(s, m, RH_WAVE);
      if (q == 0 && f < F) gas[wave][f] = (live && p.a[b * F + f] > 0.f) ? s : 0.f;  // through the outer ReLU
    }
    __syncthreads();  // (also: the staged weights, on the first trip)
    if (lane < R) {
      float s = 0.f;
      for (int f = 0; f < F; ++f) s = fmaf(w2s[f * R + lane], gas[wave][f], s);
      ghs[wave][lane] = hs[wave][lane] > 0.f ? s : 0.f;  // through the inner ReLU
    }
    __syncthreads();
    if (lane < F) {
      float s = 0.f;
      for (int r = 0; r < R; ++r) s = fmaf(w1s[r * F + lane], ghs[wave][r], s);
      gzs[wave][lane] = s * inv_d;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kWeightRegs; ++t) {
      const int e = threadIdx.x + t * RH_BLOCK;
      if (e < RF) {
        const int r1 = e / F, f1 = e - r1 * F;  // g_W1[r1, f1]
        const int f2 = e / R, r2 = e - f2 * R;  // g_W2[f2, r2]
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {  // the workgroup's samples in ascending order (dead ones hold zeros)
          acc1[t] = fmaf(ghs[w][r1], zs[w][f1], acc1[t]);
          acc2[t] = fmaf(gas[w][f2], hs[w][r2], acc2[t]);
        }
      }
    }
    if (live) {
      float* gx = p.g_x + b * (int64_t)F * D;
      for (int f0 = 0; f0 < F; f0 += per_pass) {
        const int f = f0 + slot;
        if (f < F) {
          const float gate = p.a[b * F + f], gz = gzs[wave][f];
          for (int d = q; d < D; d += G) gx[f * D + d] = fmaf(gr[f * D + d], gate, gz);
        }
      }
    }
    __syncthreads();  // the next trip overwrites the per-sample rows
  }
  float* out = p.partial + (int64_t)blockIdx.x * 2 * RF;
#pragma unroll
  for (int t = 0; t < kWeightRegs; ++t) {
    const int e = threadIdx.x + t * RH_BLOCK;
    if (e < RF) {
      out[e] = acc1[t];
      out[RF + e] = acc2[t];
    }
  }
}

int senet_check(const char* who, int B, int F, int R, int D, int64_t ld) {
  RH_REQUIRE(B >= 1, RH_E_BADARG, "%s: bad batch B=%d", who, B);
  RH_REQUIRE(F >= 1 && F <= kMaxFields && R >= 1 && R <= F && D >= 1 && D <= kMaxFieldDim, RH_E_UNSUPPORTED,
             "%s: F=%d R=%d D=%d unsupported (1 <= R <= F <= %d, 1 <= D <= %d)", who, F, R, D, kMaxFields, kMaxFieldDim);
  RH_REQUIRE(ld >= (int64_t)F * D, RH_E_BADARG, "%s: sample stride %lld shorter than F D = %d", who, (long long)ld, F * D);
  return 0;
}

}  // namespace

extern "C" int rh_twotower_nblocks(int B, int* nblocks) {
  RH_REQUIRE(nblocks != nullptr && B >= 0, RH_E_BADARG, "rh_twotower_nblocks: bad arguments");
  *nblocks = B < 1 ? 0 : grid_for(B);
  return 0;
}

extern "C" int rh_band_logits_fwd(const float* u, int64_t ldu, const float* v, int64_t ldv, const float* w, int B, int D, int K1,
                                  float temperature, float eps, float* logits, float* nu, float* nv, void* stream) {
  RH_REQUIRE(u && v && w && logits && nu && nv, RH_E_BADARG, "rh_band_logits_fwd: null pointer");
  if (int rc = band_check("rh_band_logits_fwd", B, D, K1, temperature, eps)) return rc;
  RH_REQUIRE(ldu >= D && ldv >= D, RH_E_BADARG, "rh_band_logits_fwd: row stride shorter than D");
  BandArgs a{u, ldu, v, ldv, w, nullptr, nullptr, nullptr, logits, nu, nv, nullptr, nullptr, B, D, K1, 1.f / temperature, eps};
  RH_PL_DISPATCH(band_fwd_kernel, D, grid_for(B), reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_band_logits_fwd");
  return 0;
}

extern "C" int rh_band_logits_bwd(const float* u, int64_t ldu, const float* v, int64_t ldv, const float* nu, const float* nv,
                                  const float* g, int B, int D, int K1, float temperature, float eps, float* g_u, float* g_v,
                                  void* stream) {
  RH_REQUIRE(u && v && nu && nv && g && g_u && g_v, RH_E_BADARG, "rh_band_logits_bwd: null pointer");
  if (int rc = band_check("rh_band_logits_bwd", B, D, K1, temperature, eps)) return rc;
  RH_REQUIRE(ldu >= D && ldv >= D, RH_E_BADARG, "rh_band_logits_bwd: row stride shorter than D");
  BandArgs a{u, ldu, v, ldv, nullptr, nu, nv, g, nullptr, nullptr, nullptr, g_u, g_v, B, D, K1, 1.f / temperature, eps};
  RH_PL_DISPATCH(band_bwd_kernel, D, grid_for(B), reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_band_logits_bwd");
  return 0;
}

extern "C" int rh_pair_cosine_fwd(const float* hu, int64_t ldu, const float* hp, int64_t ldp, const float* hn, int64_t ldn, int B,
                                  int D, float eps, float* pos, float* neg, float* nrm, void* stream) {
  RH_REQUIRE(hu && hp && hn && pos && neg && nrm, RH_E_BADARG, "rh_pair_cosine_fwd: null pointer");
  if (int rc = pair_check("rh_pair_cosine_fwd", B, D, eps)) return rc;
  RH_REQUIRE(ldu >= D && ldp >= D && ldn >= D, RH_E_BADARG, "rh_pair_cosine_fwd: row stride shorter than D");
  PairArgs a{hu, ldu, hp, ldp, hn, ldn, nullptr, nullptr, nullptr, pos, neg, nrm, nullptr, nullptr, nullptr, B, D, eps};
  RH_PL_DISPATCH(pair_fwd_kernel, D, grid_for(B), reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_pair_cosine_fwd");
  return 0;
}

extern "C" int rh_pair_cosine_bwd(const float* hu, int64_t ldu, const float* hp, int64_t ldp, const float* hn, int64_t ldn,
                                  const float* nrm, const float* g_pos, const float* g_neg, int B, int D, float eps, float* g_hu,
                                  float* g_hp, float* g_hn, void* stream) {
  RH_REQUIRE(hu && hp && hn && nrm && g_pos && g_neg && g_hu && g_hp && g_hn, RH_E_BADARG, "rh_pair_cosine_bwd: null pointer");
  if (int rc = pair_check("rh_pair_cosine_bwd", B, D, eps)) return rc;
  RH_REQUIRE(ldu >= D && ldp >= D && ldn >= D, RH_E_BADARG, "rh_pair_cosine_bwd: row stride shorter than D");
  PairArgs a{hu, ldu, hp, ldp, hn, ldn, nrm, g_pos, g_neg, nullptr, nullptr, nullptr, g_hu, g_hp, g_hn, B, D, eps};
  RH_PL_DISPATCH(pair_bwd_kernel, D, grid_for(B), reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_pair_cosine_bwd");
  return 0;
}

extern "C" int rh_senet_fwd(const float* x, int64_t ldx, const float* w1, const float* w2, int B, int F, int R, int D, float* y,
                            float* z, float* h, float* a, void* stream) {
  RH_REQUIRE(x && w1 && w2 && y && z && h && a, RH_E_BADARG, "rh_senet_fwd: null pointer");
  if (int rc = senet_check("rh_senet_fwd", B, F, R, D, ldx)) return rc;
  SenetArgs p{x, ldx, w1, w2, nullptr, nullptr, nullptr, nullptr, 0, y, z, h, a, nullptr, nullptr, B, F, R, D};
  hipLaunchKernelGGL(senet_fwd_kernel, dim3((unsigned)grid_for(B)), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), p);
  RH_LAUNCH_CHECK("rh_senet_fwd");
  return 0;
}

extern "C" int rh_senet_bwd(const float* x, int64_t ldx, const float* w1, const float* w2, const float* z, const float* h,
                            const float* a, const float* g, int64_t ldg, int B, int F, int R, int D, float* g_x, float* w_partial,
                            void* stream) {
  RH_REQUIRE(x && w1 && w2 && z && h && a && g && g_x && w_partial, RH_E_BADARG, "rh_senet_bwd: null pointer");
  if (int rc = senet_check("rh_senet_bwd", B, F, R, D, ldx)) return rc;
  RH_REQUIRE(ldg >= (int64_t)F * D, RH_E_BADARG, "rh_senet_bwd: gradient stride shorter than F D");
  SenetArgs p{x, ldx, w1, w2, z, h, a, g, ldg, nullptr, nullptr, nullptr, nullptr, g_x, w_partial, B, F, R, D};
  hipLaunchKernelGGL(senet_bwd_kernel, dim3((unsigned)grid_for(B)), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), p);
  RH_LAUNCH_CHECK("rh_senet_bwd");
  return 0;
}
