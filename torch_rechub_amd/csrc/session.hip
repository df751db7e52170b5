// Session-based retrieval (NARM, STAMP, GRU4Rec): a general GRU recurrence and the additive attention pooling, for gfx950.
//
// GRU (reference nn.GRU as used by narm.py:40 / gru4rec.py:37; PyTorch's cell, gate order r, z, n):
//     r = sigmoid(x_r + h W_hr^T + b_hr)    z = sigmoid(x_z + h W_hz^T + b_hz)    n = tanh(x_n + r * (h W_hn^T + b_hn))
//     h' = (1 - z) n + z h
// The input halves x = x W_ih^T + b_ih of all steps are ONE ops.linear product done by the caller (xw, (B, T, 3H)); the
// kernels run the T-step recurrence inside one launch from the zero state.  Any 1 <= H <= 128.
//
// Layout.  A workgroup owns S <= 8 samples and has 3 HP threads (HP = H rounded up to 32, 64 or 128): thread (part, i)
// owns gate column j = part H + i.  The state weights do not fit an LDS at H = 128 (3 H^2 * 4 B = 192 KiB > 160 KiB), and
// splitting them over several workgroups would need a grid-wide barrier per step.  So they live in VGPRs: in the forward
// thread j keeps ROW j of W_hh (HP floats) and forms the S state products of its column with the states read from LDS
// as broadcasts; in the backward thread (part, k) keeps COLUMN k of W_hh's gate block `part` and forms its share of
// dh_{t-1}[k] = sum_j d_s[j] W_hh[j][k]; the three shares are added in a fixed order.  The states, the state products
// and the gate gradients of the S samples go through LDS (< 32 KiB) with two or three barriers per step.
// The forward also stores the state products hu = h_{t-1} W_hh^T + b_hh (B, T, 3H): the backward then needs only the
// transposed product (one weight orientation in registers, not two).  It writes the input-side pre-activation gradients
// d_xw = [d r_pre | d z_pre | d n_pre] and the state-side ones d_s = [d r_pre | d z_pre | d hu_n]; the weight gradients
// are split-batch products over those (ops.linear_wgrad), as DIEN's.
// Bound: a latency chain of T dependent steps; per step a thread does S HP FMAs from LDS broadcasts.
//
// Additive attention pooling (NARM narm.py:60-63, STAMP stamp.py:66-67):
//     s_l = sum_h w0_h sigmoid(P_lh + r_h)    e_l = exp(s_l) mask_l    a_l = e_l / den    out = sum_l a_l X_l (+ add)
// den = sum_l e_l (NARM) or max(sum_l e_l, 1e-12) (STAMP's F.normalize(p=1)); no max subtraction, as the reference.
// One workgroup per sample; only e (B, L) and (sum, den) (B, 2) are kept for the backward, which recomputes the sigmoids.
// d w0 is per-sample partials (B, H) summed over samples in a fixed order by a second launch: no float atomics.
#include <math.h>

#include "common.h"

namespace {

constexpr int kS = 8;          // samples per GRU workgroup at most
constexpr int kMaxH = RH_GRU_MAX_H;
constexpr int kMaxL = RH_ATTN_POOL_MAX_L;    // attention pooling: positions per row
constexpr int kMaxW = RH_ATTN_POOL_MAX_W;    // attention pooling: H, Dx

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

struct GruArgs {
  const float* xw;    // (B, T, 3H)
  const float* W;     // (3H, H) weight_hh, rows r | z | n
  const float* bias;  // (3H,) bias_hh or null
  const float* h_all; // bwd: (B, T, H)
  const float* hu;    // bwd: (B, T, 3H)
  const float* g;     // bwd: (B, T, H)
  float* out_h;       // fwd: (B, T, H)
  float* out_hu;      // fwd: (B, T, 3H)
  float* d_xw;        // bwd: (B, T, 3H)
  float* d_s;         // bwd: (B, T, 3H)
  int B, T, H, S;
};

template <int HP>
__global__ __launch_bounds__(3 * HP) void gru_fwd_kernel(const GruArgs a) {
  __shared__ __attribute__((aligned(16))) float hs[kS][HP];
  __shared__ float gs[kS][3 * HP];
  const int tid = threadIdx.x, part = tid / HP, i = tid % HP;
  const int H = a.H, H3 = 3 * a.H, T = a.T;
  const bool col = i < H;
  const int j = part * H + i;
  float w[HP];
#pragma unroll
  for (int k = 0; k < HP; ++k) w[k] = (col && k < H) ? a.W[(int64_t)j * H + k] : 0.f;
  const float bj = (col && a.bias != nullptr) ? a.bias[j] : 0.f;
  const int64_t b0 = (int64_t)blockIdx.x * a.S;
  for (int e = tid; e < kS * HP; e += 3 * HP) hs[e / HP][e % HP] = 0.f;
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    float acc[kS];
#pragma unroll
    for (int s = 0; s < kS; ++s) acc[s] = bj;
#pragma unroll
    for (int k = 0; k < HP; k += 4) {
#pragma unroll
      for (int s = 0; s < kS; ++s) {
        if (s < a.S) {
          const float4 hv = *reinterpret_cast<const float4*>(&hs[s][k]);
          acc[s] = fmaf(hv.x, w[k], acc[s]);
          acc[s] = fmaf(hv.y, w[k + 1], acc[s]);
          acc[s] = fmaf(hv.z, w[k + 2], acc[s]);
          acc[s] = fmaf(hv.w, w[k + 3], acc[s]);
        }
      }
    }
    if (col) {
#pragma unroll
      for (int s = 0; s < kS; ++s)
        if (s < a.S) gs[s][part * HP + i] = acc[s];
    }
    __syncthreads();
    for (int e = tid; e < a.S * HP; e += 3 * HP) {
      const int s = e / HP, ii = e % HP;
      const int64_t b = b0 + s;
      if (ii >= H || b >= a.B) continue;
      const int64_t row = b * T + t;
      const float* x = a.xw + row * H3;
      const float hr = gs[s][ii], hz = gs[s][HP + ii], hn = gs[s][2 * HP + ii];
      const float r = sigm(x[ii] + hr);
      const float z = sigm(x[H + ii] + hz);
      const float n = tanhf(x[2 * H + ii] + r * hn);
      const float hnew = (1.f - z) * n + z * hs[s][ii];
      hs[s][ii] = hnew;
      a.out_h[row * H + ii] = hnew;
      float* u = a.out_hu + row * H3;
      u[ii] = hr, u[H + ii] = hz, u[2 * H + ii] = hn;
    }
    __syncthreads();
  }
}

template <int HP>
__global__ __launch_bounds__(3 * HP) void gru_bwd_kernel(const GruArgs a) {
  __shared__ float dh[kS][HP];
  __shared__ __attribute__((aligned(16))) float ds[kS][3 * HP];
  __shared__ float pp[3][kS][HP];
  const int tid = threadIdx.x, part = tid / HP, k = tid % HP;
  const int H = a.H, H3 = 3 * a.H, T = a.T;
  const bool col = k < H;
  float w[HP];  // w[i] = W_hh[part H + i][k]
#pragma unroll
  for (int i = 0; i < HP; ++i) w[i] = (col && i < H) ? a.W[(int64_t)(part * H + i) * H + k] : 0.f;
  const int64_t b0 = (int64_t)blockIdx.x * a.S;
  for (int e = tid; e < kS * HP; e += 3 * HP) dh[e / HP][e % HP] = 0.f;
  for (int e = tid; e < kS * 3 * HP; e += 3 * HP) ds[e / (3 * HP)][e % (3 * HP)] = 0.f;
  __syncthreads();
  for (int t = T - 1; t >= 0; --t) {
    for (int e = tid; e < a.S * HP; e += 3 * HP) {
      const int s = e / HP, ii = e % HP;
      const int64_t b = b0 + s;
      if (ii >= H || b >= a.B) continue;
      const int64_t row = b * T + t;
      const float d = dh[s][ii] + a.g[row * H + ii];
      const float hp = t > 0 ? a.h_all[(row - 1) * H + ii] : 0.f;
      const float* x = a.xw + row * H3;
      const float* u = a.hu + row * H3;
      const float hn = u[2 * H + ii];
      const float r = sigm(x[ii] + u[ii]);
      const float z = sigm(x[H + ii] + u[H + ii]);
      const float n = tanhf(x[2 * H + ii] + r * hn);
      const float an = d * (1.f - z) * (1.f - n * n);
      const float dpz = d * (hp - n) * z * (1.f - z);
      const float dpr = an * hn * r * (1.f - r);
      const float dhn = an * r;
      float* dx = a.d_xw + row * H3;
      float* dsg = a.d_s + row * H3;
      dx[ii] = dpr, dx[H + ii] = dpz, dx[2 * H + ii] = an;
      dsg[ii] = dpr, dsg[H + ii] = dpz, dsg[2 * H + ii] = dhn;
      ds[s][ii] = dpr, ds[s][HP + ii] = dpz, ds[s][2 * HP + ii] = dhn;
      dh[s][ii] = d * z;  // the direct path to h_{t-1}; the paths through W_hh are added below
    }
    __syncthreads();
    if (col) {
#pragma unroll
      for (int s = 0; s < kS; ++s) {
        if (s < a.S) {
          float p = 0.f;
#pragma unroll
          for (int i = 0; i < HP; i += 4) {
            const float4 v = *reinterpret_cast<const float4*>(&ds[s][part * HP + i]);
            p = fmaf(v.x, w[i], p);
            p = fmaf(v.y, w[i + 1], p);
            p = fmaf(v.z, w[i + 2], p);
            p = fmaf(v.w, w[i + 3], p);
          }
          pp[part][s][k] = p;
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < a.S * HP; e += 3 * HP) {
      const int s = e / HP, kk = e % HP;
      if (kk < H) dh[s][kk] = ((dh[s][kk] + pp[0][s][kk]) + pp[1][s][kk]) + pp[2][s][kk];
    }
    __syncthreads();
  }
}

int gru_hp(int H) { return H <= 32 ? 32 : (H <= 64 ? 64 : 128); }

int gru_samples(int B) {
  const int s = (B + 511) / 512;
  return s < 1 ? 1 : (s > kS ? kS : s);
}

int gru_launch(bool fwd, const GruArgs& a, hipStream_t st) {
  const int hp = gru_hp(a.H);
  const dim3 grid((unsigned)((a.B + a.S - 1) / a.S)), block(3 * hp);
  if (fwd) {
    if (hp == 32) hipLaunchKernelGGL(gru_fwd_kernel<32>, grid, block, 0, st, a);
    else if (hp == 64) hipLaunchKernelGGL(gru_fwd_kernel<64>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(gru_fwd_kernel<128>, grid, block, 0, st, a);
  } else {
    if (hp == 32) hipLaunchKernelGGL(gru_bwd_kernel<32>, grid, block, 0, st, a);
    else if (hp == 64) hipLaunchKernelGGL(gru_bwd_kernel<64>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(gru_bwd_kernel<128>, grid, block, 0, st, a);
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
struct PoolArgs {
  const float* P;     // (B, L, H)
  const float* r;     // (B, H)
  const float* w0;    // (H,)
  const float* mask;  // (B, L) 0 / 1
  const float* X;     // (B, L, Dx)
  const float* add;   // (B, Dx) or null
  float* out;         // (B, Dx)
  float* e;           // (B, L)
  float* sums;        // (B, 2): sum_l e_l, den
  const float* g;     // (B, Dx)
  float* dP;          // (B, L, H)
  float* dr;          // (B, H)
  float* dw0_part;    // (B, H)
  float* dw0;         // (H,)
  float* dX;          // (B, L, Dx)
  int B, L, H, Dx, floor_;
};

constexpr float kNormEps = 1e-12f;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < RH_WAVE; m <<= 1) v += __shfl_xor(v, m, RH_WAVE);
  return v;
}

// fixed-order sum of v over the workgroup (every thread gets it)
__device__ __forceinline__ float block_sum(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = RH_BLOCK / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(RH_BLOCK) void pool_fwd_kernel(const PoolArgs a) {
  __shared__ float ev[kMaxL];
  __shared__ float red[RH_BLOCK];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, wv = tid / RH_WAVE;
  const int64_t b = blockIdx.x;
  const int L = a.L, H = a.H, Dx = a.Dx;
  for (int l = wv; l < L; l += RH_BLOCK / RH_WAVE) {
    const float* p = a.P + (b * L + l) * H;
    float s = 0.f;
    for (int h = lane; h < H; h += RH_WAVE) s = fmaf(a.w0[h], sigm(p[h] + a.r[b * H + h]), s);
    s = wave_sum(s);
    if (lane == 0) ev[l] = expf(s) * a.mask[b * L + l];
  }
  __syncthreads();
  float part = 0.f;
  for (int l = tid; l < L; l += RH_BLOCK) part += ev[l];
  const float sum = block_sum(part, red);
  const float den = a.floor_ ? fmaxf(sum, kNormEps) : sum;
  for (int l = tid; l < L; l += RH_BLOCK) a.e[b * L + l] = ev[l];
  if (tid == 0) a.sums[2 * b] = sum, a.sums[2 * b + 1] = den;
  for (int d = tid; d < Dx; d += RH_BLOCK) {
    float acc = 0.f;
    for (int l = 0; l < L; ++l) acc = fmaf(ev[l] / den, a.X[(b * L + l) * Dx + d], acc);
    if (a.add != nullptr) acc += a.add[b * Dx + d];
    a.out[b * Dx + d] = acc;
  }
}

__global__ __launch_bounds__(RH_BLOCK) void pool_bwd_kernel(const PoolArgs a) {
  __shared__ float al[kMaxL], dl[kMaxL];
  __shared__ float red[RH_BLOCK];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, wv = tid / RH_WAVE;
  const int64_t b = blockIdx.x;
  const int L = a.L, H = a.H, Dx = a.Dx;
  const float sum = a.sums[2 * b], den = a.sums[2 * b + 1];
  const float* gb = a.g + b * Dx;
  // da_l = g . X_l, dX_l = a_l g
  for (int l = wv; l < L; l += RH_BLOCK / RH_WAVE) {
    const float al_ = a.e[b * L + l] / den;
    const float* x = a.X + (b * L + l) * Dx;
    float* dx = a.dX + (b * L + l) * Dx;
    float s = 0.f;
    for (int d = lane; d < Dx; d += RH_WAVE) {
      const float gv = gb[d];
      s = fmaf(gv, x[d], s);
      dx[d] = al_ * gv;
    }
    s = wave_sum(s);
    if (lane == 0) al[l] = al_, dl[l] = s;
  }
  __syncthreads();
  float part = 0.f;
  for (int l = tid; l < L; l += RH_BLOCK) part = fmaf(al[l], dl[l], part);
  const float c = block_sum(part, red);
  // the floor of F.normalize holds the denominator constant (no gradient through the sum)
  const bool floored = a.floor_ && !(sum >= kNormEps);
  for (int l = tid; l < L; l += RH_BLOCK) {
    const float de = floored ? dl[l] / den : (dl[l] - c) / den;
    dl[l] = a.e[b * L + l] * de;  // d s_l
  }
  __syncthreads();
  for (int h = tid; h < H; h += RH_BLOCK) {
    const float rr = a.r[b * H + h], w = a.w0[h];
    float drh = 0.f, dwh = 0.f;
    for (int l = 0; l < L; ++l) {
      const int64_t i = (b * L + l) * H + h;
      const float sg = sigm(a.P[i] + rr);
      const float dp = dl[l] * w * sg * (1.f - sg);
      a.dP[i] = dp;
      drh += dp;
      dwh = fmaf(dl[l], sg, dwh);
    }
    a.dr[b * H + h] = drh;
    a.dw0_part[b * H + h] = dwh;
  }
}

// dw0[h] = sum over samples of dw0_part[:, h], thread t taking samples t, t + 256, ... then a fixed tree
__global__ __launch_bounds__(RH_BLOCK) void pool_dw0_kernel(const PoolArgs a) {
  __shared__ float red[RH_BLOCK];
  const int h = blockIdx.x, tid = threadIdx.x;
  float s = 0.f;
  for (int64_t b = tid; b < a.B; b += RH_BLOCK) s += a.dw0_part[b * a.H + h];
  s = block_sum(s, red);
  if (tid == 0) a.dw0[h] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// Dropout with the project's counter hash (common.h rh_drop_hash); the mask is recomputed in the backward from ctr.
__global__ __launch_bounds__(RH_BLOCK) void dropout_kernel(const float* x, int64_t n, float p, const int64_t* rng,
                                                           int64_t* saved_ctr, float* y) {
  const uint64_t seed = (uint64_t)rng[0];
  const uint64_t ctr = (uint64_t)rng[1];
  if (blockIdx.x == 0 && threadIdx.x == 0) saved_ctr[0] = (int64_t)ctr;
  const uint32_t thr = (uint32_t)(p * 4294967296.0);
  const float keep = 1.f / (1.f - p);
  for (int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * RH_BLOCK)
    y[i] = rh_drop_hash(seed, ctr, (uint64_t)i) >= thr ? x[i] * keep : 0.f;
}

__global__ void dropout_advance_kernel(int64_t* rng) { rng[1] += 1; }

__global__ __launch_bounds__(RH_BLOCK) void dropout_bwd_kernel(const float* g, int64_t n, float p, const int64_t* rng,
                                                               const int64_t* saved_ctr, float* dx) {
  const uint64_t seed = (uint64_t)rng[0], ctr = (uint64_t)saved_ctr[0];
  const uint32_t thr = (uint32_t)(p * 4294967296.0);
  const float keep = 1.f / (1.f - p);
  for (int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * RH_BLOCK)
    dx[i] = rh_drop_hash(seed, ctr, (uint64_t)i) >= thr ? g[i] * keep : 0.f;
}

// Session lengths: counts[b] = #(seq[b, :] != 0); ORs RH_FLAG_SESSION_EMPTY into *err for a row without items and, with
// check_full, RH_FLAG_SESSION_SHORT when no row reaches L (the inputs pack_padded_sequence / NARM's broadcast reject).
// One workgroup: rows strided over the threads, a fixed-order max.
__global__ __launch_bounds__(RH_BLOCK) void session_lengths_kernel(const int64_t* seq, int B, int L, int check_full,
                                                                   int64_t* counts, int32_t* err) {
  __shared__ int red[RH_BLOCK];
  const int tid = threadIdx.x;
  int mx = 0, empty = 0;
  for (int b = tid; b < B; b += RH_BLOCK) {
    int c = 0;
    for (int l = 0; l < L; ++l) c += seq[(int64_t)b * L + l] != 0;
    counts[b] = c;
    mx = c > mx ? c : mx;
    empty |= c == 0;
  }
  red[tid] = mx;
  __syncthreads();
  for (int o = RH_BLOCK / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = red[tid + o] > red[tid] ? red[tid + o] : red[tid];
    __syncthreads();
  }
  if (empty) atomicOr(err, RH_FLAG_SESSION_EMPTY);
  if (tid == 0 && check_full && red[0] < L) atomicOr(err, RH_FLAG_SESSION_SHORT);
}

int grid_for(int64_t n) {
  int64_t g = (n + RH_BLOCK - 1) / RH_BLOCK;
  if (g > 8192) g = 8192;
  return (int)(g < 1 ? 1 : g);
}

}  // namespace

extern "C" int rh_gru_fwd(const float* xw, const float* w_hh, const float* b_hh, int B, int T, int H, float* h_all, float* hu,
                          void* stream) {
  RH_REQUIRE(B >= 0 && T >= 1, RH_E_BADARG, "rh_gru_fwd: bad shape B=%d T=%d", B, T);
  RH_REQUIRE(H >= 1 && H <= kMaxH, RH_E_UNSUPPORTED, "rh_gru_fwd: hidden size %d unsupported (1 <= H <= %d)", H, kMaxH);
  if (B == 0) return 0;
  RH_REQUIRE(xw && w_hh && h_all && hu, RH_E_BADARG, "rh_gru_fwd: null pointer");
  GruArgs a{};
  a.xw = xw, a.W = w_hh, a.bias = b_hh, a.out_h = h_all, a.out_hu = hu;
  a.B = B, a.T = T, a.H = H, a.S = gru_samples(B);
  gru_launch(true, a, reinterpret_cast<hipStream_t>(stream));
  RH_LAUNCH_CHECK("rh_gru_fwd");
  return 0;
}

extern "C" int rh_gru_bwd(const float* xw, const float* w_hh, const float* h_all, const float* hu, const float* g, int B, int T,
                          int H, float* d_xw, float* d_s, void* stream) {
  RH_REQUIRE(B >= 0 && T >= 1, RH_E_BADARG, "rh_gru_bwd: bad shape B=%d T=%d", B, T);
  RH_REQUIRE(H >= 1 && H <= kMaxH, RH_E_UNSUPPORTED, "rh_gru_bwd: hidden size %d unsupported (1 <= H <= %d)", H, kMaxH);
  if (B == 0) return 0;
  RH_REQUIRE(xw && w_hh && h_all && hu && g && d_xw && d_s, RH_E_BADARG, "rh_gru_bwd: null pointer");
  GruArgs a{};
  a.xw = xw, a.W = w_hh, a.h_all = h_all, a.hu = hu, a.g = g, a.d_xw = d_xw, a.d_s = d_s;
  a.B = B, a.T = T, a.H = H, a.S = gru_samples(B);
  gru_launch(false, a, reinterpret_cast<hipStream_t>(stream));
  RH_LAUNCH_CHECK("rh_gru_bwd");
  return 0;
}

static int pool_check(const char* name, int B, int L, int H, int Dx) {
  RH_REQUIRE(B >= 0, RH_E_BADARG, "%s: bad batch %d", name, B);
  RH_REQUIRE(L >= 1 && L <= kMaxL && H >= 1 && H <= kMaxW && Dx >= 1 && Dx <= kMaxW, RH_E_UNSUPPORTED,
             "%s: L=%d H=%d Dx=%d unsupported (1 <= L <= %d, 1 <= H, Dx <= %d)", name, L, H, Dx, kMaxL, kMaxW);
  return 0;
}

extern "C" int rh_attn_pool_fwd(const float* P, const float* r, const float* w0, const float* mask, const float* X,
                                const float* add, int B, int L, int H, int Dx, int floor_, float* out, float* e, float* sums,
                                void* stream) {
  if (int rc = pool_check("rh_attn_pool_fwd", B, L, H, Dx)) return rc;
  if (B == 0) return 0;
  RH_REQUIRE(P && r && w0 && mask && X && out && e && sums, RH_E_BADARG, "rh_attn_pool_fwd: null pointer");
  PoolArgs a{};
  a.P = P, a.r = r, a.w0 = w0, a.mask = mask, a.X = X, a.add = add, a.out = out, a.e = e, a.sums = sums;
  a.B = B, a.L = L, a.H = H, a.Dx = Dx, a.floor_ = floor_ != 0;
  hipLaunchKernelGGL(pool_fwd_kernel, dim3(B), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_attn_pool_fwd");
  return 0;
}

extern "C" int rh_attn_pool_bwd(const float* P, const float* r, const float* w0, const float* X, const float* e,
                                const float* sums, const float* g, int B, int L, int H, int Dx, int floor_, float* dP, float* dr,
                                float* dw0_part, float* dw0, float* dX, void* stream) {
  if (int rc = pool_check("rh_attn_pool_bwd", B, L, H, Dx)) return rc;
  RH_REQUIRE(P && r && w0 && X && e && sums && g && dP && dr && dw0_part && dw0 && dX, RH_E_BADARG,
             "rh_attn_pool_bwd: null pointer");
  PoolArgs a{};
  a.P = P, a.r = r, a.w0 = w0, a.X = X, a.e = const_cast<float*>(e), a.sums = const_cast<float*>(sums), a.g = g;
  a.dP = dP, a.dr = dr, a.dw0_part = dw0_part, a.dw0 = dw0, a.dX = dX;
  a.B = B, a.L = L, a.H = H, a.Dx = Dx, a.floor_ = floor_ != 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // d w0 (H,) does not depend on B: an empty batch still writes it (the sum over no sample, zero)
  if (B > 0) hipLaunchKernelGGL(pool_bwd_kernel, dim3(B), dim3(RH_BLOCK), 0, st, a);
  hipLaunchKernelGGL(pool_dw0_kernel, dim3(H), dim3(RH_BLOCK), 0, st, a);
  RH_LAUNCH_CHECK("rh_attn_pool_bwd");
  return 0;
}

extern "C" int rh_session_dropout_fwd(const float* x, int64_t n, float p, int64_t* rng, int64_t* saved_ctr, float* y,
                                      void* stream) {
  RH_REQUIRE(n >= 0 && p > 0.f && p < 1.f, RH_E_BADARG, "rh_session_dropout_fwd: n=%lld p=%g", (long long)n, (double)p);
  RH_REQUIRE(x && rng && saved_ctr && y, RH_E_BADARG, "rh_session_dropout_fwd: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dropout_kernel, dim3(grid_for(n)), dim3(RH_BLOCK), 0, st, x, n, p, rng, saved_ctr, y);
  hipLaunchKernelGGL(dropout_advance_kernel, dim3(1), dim3(1), 0, st, rng);
  RH_LAUNCH_CHECK("rh_session_dropout_fwd");
  return 0;
}

extern "C" int rh_session_dropout_bwd(const float* g, int64_t n, float p, const int64_t* rng, const int64_t* saved_ctr,
                                      float* dx, void* stream) {
  RH_REQUIRE(n >= 0 && p > 0.f && p < 1.f, RH_E_BADARG, "rh_session_dropout_bwd: n=%lld p=%g", (long long)n, (double)p);
  RH_REQUIRE(g && rng && saved_ctr && dx, RH_E_BADARG, "rh_session_dropout_bwd: null pointer");
  hipLaunchKernelGGL(dropout_bwd_kernel, dim3(grid_for(n)), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), g, n,
                     p, rng, saved_ctr, dx);
  RH_LAUNCH_CHECK("rh_session_dropout_bwd");
  return 0;
}

extern "C" int rh_session_lengths(const int64_t* seq, int B, int L, int check_full, int64_t* counts, int32_t* err,
                                  void* stream) {
  RH_REQUIRE(B >= 0 && L >= 1, RH_E_BADARG, "rh_session_lengths: bad shape B=%d L=%d", B, L);
  if (B == 0) return 0;
  RH_REQUIRE(seq && counts && err, RH_E_BADARG, "rh_session_lengths: null pointer");
  hipLaunchKernelGGL(session_lengths_kernel, dim3(1), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), seq, B, L,
                     check_full, counts, err);
  RH_LAUNCH_CHECK("rh_session_lengths");
  return 0;
}
