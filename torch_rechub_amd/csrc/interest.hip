// Multi-interest user towers and list-wise scoring of the retrieval models (YoutubeDNN, MIND, ComiRec-DR / -SA).
//
// Capsule routing (reference CapsuleNetwork.forward, torch_rechub/basic/layers.py:657-712).  The reference forms the
// projections u_hat (B, L, I, D) -- for ComiRec-DR (bilinear type 2) through `w[:, :L] * u` summed over the last axis, a
// (B, L, I*D, D) product: 839 MB at B = 4096, L = 50, I = 4, D = 16, and as much again in its backward -- then runs
// `routing_times` iterations of softmax / weighted sum / squash / logit update with ~15 ATen launches each.  Here one
// workgroup routes S samples with their u_hat in LDS: types 0 / 1 read the (B, L, Iu*D) output of the Linear in front of
// it (Iu = 1 for MIND's shared projection, repeated over the I interests by indexing), type 2 forms u_hat from w[l]
// staged in LDS once per tile of S samples.  Gradient flows only through the last iteration (iterations < 2 use the
// detached u_hat, the logits never carry gradient): d_s = squash'(s) d_cap, d_u_hat[l, i] = softmax_weight[i, l] d_s[i].
// The type-2 weight gradient sum_b d_u_hat[b, l] (x) e[b, l] is a second kernel over (l, chunk of samples) whose per-chunk
// partials the caller sums in a fixed order (rh_colsum): bitwise reproducible, no atomics.
//
// Self-attentive pooling (reference MultiInterestSA.forward, layers.py:599-609 after H W2): softmax over L of
// A + (-1e9)(1 - mask), formed as the reference forms it (a fully padded row comes out uniform), then A^T E.  One
// wavefront per sample each way.
//
// List-wise scoring (reference YoutubeDNN / MIND / ComiRec forward + item_tower): L2-normalises the positive and the K
// negative item rows (F.normalize, eps 1e-12), picks the interest with the largest dot product with the positive (first
// maximum, as torch.argmax), and writes the (B, 1 + K) logits, without the (B, 1 + K, D) concatenation.
#include "common.h"

namespace {

constexpr int kMaxLdsFloats = 16384;  // 64 KB of dynamic LDS per workgroup
constexpr float kSquashEps = 1e-9f;

struct CapsGeom {
  int B, L, I, D, type, iters, S;
};

// samples per workgroup: S * I * D <= 256 (one thread per capsule element), LDS within kMaxLdsFloats
int caps_samples_per_block(int L, int I, int D, int type) {
  const int ID = I * D;
  int S = RH_BLOCK / ID;
  if (S > 4) S = 4;
  const int fixed = type == 2 ? ID * D : 0;
  while (S >= 1 && S * (L * ID + 2 * I * L + 2 * ID) + fixed > kMaxLdsFloats) --S;
  return S;
}

size_t caps_lds_bytes(const CapsGeom& g) {
  const int ID = g.I * g.D;
  return sizeof(float) * ((size_t)g.S * (g.L * ID + 2 * g.I * g.L + 2 * ID) + (g.type == 2 ? (size_t)ID * g.D : 0));
}

// the masked softmax over L of each (sample, interest) row of lg into sw; lanes per row a power of two <= 64
__device__ __forceinline__ void caps_softmax(const float* lg, float* sw, const int32_t* __restrict__ mask, int b0, int B, int S,
                                             int I, int L) {
  const int R = S * I;
  int lpr = 64;
  while (lpr > 1 && lpr * R > RH_BLOCK) lpr >>= 1;
  const int row = threadIdx.x / lpr, q = threadIdx.x % lpr;
  const int rr = row < R ? row : R - 1;  // (every lane takes part in the shuffles)
  const float* x = lg + rr * L;
  float m = -INFINITY;
  for (int l = q; l < L; l += lpr) m = fmaxf(m, x[l]);
  for (int o = 1; o < lpr; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, RH_WAVE));
  float sum = 0.f;
  for (int l = q; l < L; l += lpr) sum += expf(x[l] - m);
  for (int o = 1; o < lpr; o <<= 1) sum += __shfl_xor(sum, o, RH_WAVE);
  if (row < R) {
    const int s = row / I;
    const int64_t b = (int64_t)b0 + s;
    for (int l = q; l < L; l += lpr) {
      const bool keep = b < B && mask[b * L + l] != 0;
      sw[row * L + l] = keep ? expf(x[l] - m) / sum : 0.f;
    }
  }
}

__global__ __launch_bounds__(RH_BLOCK) void capsule_fwd_kernel(const float* __restrict__ U, const float* __restrict__ E,
                                                               const float* __restrict__ W, const int32_t* __restrict__ mask,
                                                               const float* __restrict__ init, const CapsGeom g,
                                                               float* __restrict__ cap, float* __restrict__ sw_out,
                                                               float* __restrict__ s_out) {
  RH_CHAIN_PRIO();
  extern __shared__ float lds[];
  const int L = g.L, I = g.I, D = g.D, S = g.S, ID = I * D, LID = L * ID;
  float* uh = lds;                  // [S][L][I][D]
  float* lg = uh + S * LID;         // [S][I][L] routing logits
  float* sw = lg + S * I * L;       // [S][I][L] masked softmax weights
  float* cs = sw + S * I * L;       // [S][I][D] weighted sums s
  float* cc = cs + S * ID;          // [S][I][D] squashed capsules
  float* wl = cc + S * ID;          // [I*D][D] w[l] (type 2)
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * S;
  if (g.type == 2) {
    for (int l = 0; l < L; ++l) {
      __syncthreads();
      for (int e = tid; e < ID * D; e += RH_BLOCK) wl[e] = W[(int64_t)l * ID * D + e];
      __syncthreads();
      for (int e = tid; e < S * ID; e += RH_BLOCK) {
        const int s = e / ID, j = e % ID;
        const int64_t b = (int64_t)b0 + s;
        float acc = 0.f;
        if (b < g.B) {
          const float* er = E + (b * L + l) * D;
          for (int k = 0; k < D; ++k) acc = fmaf(wl[j * D + k], er[k], acc);
        }
        uh[s * LID + l * ID + j] = acc;
      }
    }
  } else {
    const int Iu = g.type == 0 ? 1 : I;
    for (int e = tid; e < S * LID; e += RH_BLOCK) {
      const int s = e / LID, r = e % LID;
      const int l = r / ID, j = r % ID;
      const int64_t b = (int64_t)b0 + s;
      uh[e] = b < g.B ? U[(b * L + l) * Iu * D + (g.type == 0 ? j % D : j)] : 0.f;
    }
  }
  for (int e = tid; e < S * I * L; e += RH_BLOCK) {
    const int64_t b = (int64_t)b0 + e / (I * L);
    lg[e] = (init != nullptr && b < g.B) ? init[b * I * L + e % (I * L)] : 0.f;
  }
  __syncthreads();
  for (int it = 0; it < g.iters; ++it) {
    caps_softmax(lg, sw, mask, b0, g.B, S, I, L);
    __syncthreads();
    if (tid < S * ID) {  // s[i, d] = sum_l sw[i, l] u_hat[l, i, d]
      const int s = tid / ID, j = tid % ID, i = j / D;
      const float* wrow = sw + (s * I + i) * L;
      const float* u = uh + s * LID + j;
      float acc = 0.f;
      for (int l = 0; l < L; ++l) acc = fmaf(wrow[l], u[l * ID], acc);
      cs[tid] = acc;
    }
    __syncthreads();
    if (tid < S * ID) {  // squash: n / (1 + n) / sqrt(n + 1e-9) * s
      const int base = tid - tid % D;
      float n = 0.f;
      for (int d = 0; d < D; ++d) n = fmaf(cs[base + d], cs[base + d], n);
      cc[tid] = n / (1.f + n) / sqrtf(n + kSquashEps) * cs[tid];
    }
    __syncthreads();
    if (it < 2 && it + 1 < g.iters) {  // logits += u_hat . capsule (iterations 0 and 1 only)
      for (int e = tid; e < S * I * L; e += RH_BLOCK) {
        const int s = e / (I * L), i = (e / L) % I, l = e % L;
        const float* u = uh + s * LID + l * ID + i * D;
        const float* c = cc + (s * I + i) * D;
        float acc = 0.f;
        for (int d = 0; d < D; ++d) acc = fmaf(u[d], c[d], acc);
        lg[e] += acc;
      }
      __syncthreads();
    }
  }
  for (int e = tid; e < S * ID; e += RH_BLOCK) {
    const int64_t b = (int64_t)b0 + e / ID;
    if (b < g.B) {
      cap[b * ID + e % ID] = cc[e];
      if (s_out != nullptr) s_out[b * ID + e % ID] = cs[e];
    }
  }
  if (sw_out != nullptr) {
    for (int e = tid; e < S * I * L; e += RH_BLOCK) {
      const int64_t b = (int64_t)b0 + e / (I * L);
      if (b < g.B) sw_out[b * I * L + e % (I * L)] = sw[e];
    }
  }
}

// d_s = f(n) d_cap + 2 f'(n) (s . d_cap) s,  f(n) = n / (1 + n) / sqrt(n + eps)
__device__ __forceinline__ float squash_bwd(const float* s, const float* gc, int D, int d) {
  float n = 0.f, sg = 0.f;
  for (int k = 0; k < D; ++k) {
    n = fmaf(s[k], s[k], n);
    sg = fmaf(s[k], gc[k], sg);
  }
  const float r = sqrtf(n + kSquashEps);
  const float f = n / (1.f + n) / r;
  const float fp = 1.f / ((1.f + n) * (1.f + n) * r) - 0.5f * n / ((1.f + n) * (n + kSquashEps) * r);
  return f * gc[d] + 2.f * fp * sg * s[d];
}

// per S samples: d_s (B, I, D) -> types 0 / 1: d_U (B, L, Iu*D);  type 2: d_E (B, L, D) and d_s to global (wgrad kernel)
__global__ __launch_bounds__(RH_BLOCK) void capsule_bwd_kernel(const float* __restrict__ g_cap, const float* __restrict__ s_in,
                                                               const float* __restrict__ sw_in, const float* __restrict__ W,
                                                               const CapsGeom g, float* __restrict__ g_u,
                                                               float* __restrict__ g_e, float* __restrict__ gs_out) {
  RH_CHAIN_PRIO();
  extern __shared__ float lds[];
  const int L = g.L, I = g.I, D = g.D, S = g.S, ID = I * D;
  float* sw = lds;             // [S][I][L]
  float* gs = sw + S * I * L;  // [S][I][D]
  float* wl = gs + S * ID;     // [I*D][D] (type 2)
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * S;
  for (int e = tid; e < S * I * L; e += RH_BLOCK) {
    const int64_t b = (int64_t)b0 + e / (I * L);
    sw[e] = b < g.B ? sw_in[b * I * L + e % (I * L)] : 0.f;
  }
  if (tid < S * ID) {
    const int64_t b = (int64_t)b0 + tid / ID;
    float v = 0.f;
    if (b < g.B) {
      const int j = tid % ID;
      v = squash_bwd(s_in + (b * ID + (j - j % D)), g_cap + (b * ID + (j - j % D)), D, j % D);
      if (gs_out != nullptr) gs_out[b * ID + j] = v;
    }
    gs[tid] = v;
  }
  __syncthreads();
  if (g.type != 2) {
    const int Iu = g.type == 0 ? 1 : I;
    const int W_ = Iu * D;
    for (int e = tid; e < S * L * W_; e += RH_BLOCK) {
      const int s = e / (L * W_), r = e % (L * W_);
      const int l = r / W_, j = r % W_;
      const int64_t b = (int64_t)b0 + s;
      if (b >= g.B) continue;
      float acc;
      if (g.type == 0) {  // the shared projection: the I interests' gradients summed (in interest order)
        acc = 0.f;
        for (int i = 0; i < I; ++i) acc = fmaf(sw[(s * I + i) * L + l], gs[(s * I + i) * D + j], acc);
      } else {
        const int i = j / D;
        acc = sw[(s * I + i) * L + l] * gs[s * ID + j];
      }
      g_u[(b * L + l) * W_ + j] = acc;
    }
    return;
  }
  for (int l = 0; l < L; ++l) {
    __syncthreads();
    for (int e = tid; e < ID * D; e += RH_BLOCK) wl[e] = W[(int64_t)l * ID * D + e];
    __syncthreads();
    for (int e = tid; e < S * D; e += RH_BLOCK) {  // d_e[l, k] = sum_j w[l, j, k] sw[i(j), l] d_s[j]
      const int s = e / D, k = e % D;
      const int64_t b = (int64_t)b0 + s;
      if (b >= g.B) continue;
      float acc = 0.f;
      for (int j = 0; j < ID; ++j) acc = fmaf(wl[j * D + k], sw[(s * I + j / D) * L + l] * gs[s * ID + j], acc);
      g_e[(b * L + l) * D + k] = acc;
    }
  }
}

constexpr int kWgradChunks = 32;
constexpr int kWgradTile = 16;        // samples staged in LDS at a time
constexpr int kWgradMaxPerThread = 16;
static_assert(RH_BLOCK == RH_CAPSULE_MAX_ID && RH_BLOCK * kWgradMaxPerThread == RH_CAPSULE_MAX_IDD,
              "one thread per capsule element, kWgradMaxPerThread weight gradients each");

// partial[c, l, j, k] = sum over the samples b of chunk c (in order) of sw[b, j/D, l] d_s[b, j] e[b, l, k]
__global__ __launch_bounds__(RH_BLOCK) void capsule_wgrad_kernel(const float* __restrict__ gs, const float* __restrict__ sw,
                                                                 const float* __restrict__ E, const CapsGeom g, int chunk,
                                                                 float* __restrict__ partial) {
  RH_CHAIN_PRIO();
  __shared__ float gu[kWgradTile * 256];
  __shared__ float ev[kWgradTile * 64];
  const int L = g.L, I = g.I, D = g.D, ID = I * D, N = ID * D;
  const int l = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int64_t lo = (int64_t)c * chunk;
  int64_t hi = lo + chunk;
  if (hi > g.B) hi = g.B;
  float acc[kWgradMaxPerThread];
#pragma unroll
  for (int r = 0; r < kWgradMaxPerThread; ++r) acc[r] = 0.f;
  for (int64_t t0 = lo; t0 < hi; t0 += kWgradTile) {
    const int n = (int)((hi - t0) < kWgradTile ? (hi - t0) : kWgradTile);
    __syncthreads();
    for (int e = tid; e < n * ID; e += RH_BLOCK) {
      const int64_t b = t0 + e / ID;
      const int j = e % ID;
      gu[e] = sw[(b * I + j / D) * L + l] * gs[b * ID + j];
    }
    for (int e = tid; e < n * D; e += RH_BLOCK) {
      const int64_t b = t0 + e / D;
      ev[e] = E[(b * L + l) * D + e % D];
    }
    __syncthreads();
    for (int t = 0; t < n; ++t) {
#pragma unroll
      for (int r = 0; r < kWgradMaxPerThread; ++r) {
        const int e = tid + r * RH_BLOCK;
        if (e < N) acc[r] = fmaf(gu[t * ID + e / D], ev[t * D + e % D], acc[r]);
      }
    }
  }
  float* out = partial + ((int64_t)c * L + l) * N;
#pragma unroll
  for (int r = 0; r < kWgradMaxPerThread; ++r) {
    const int e = tid + r * RH_BLOCK;
    if (e < N) out[e] = acc[r];
  }
}

int caps_check(const char* who, const CapsGeom& g) {
  RH_REQUIRE(g.B >= 0 && g.L >= 1 && g.I >= 1 && g.D >= 1 && g.type >= 0 && g.type <= 2 && g.iters >= 1, RH_E_BADARG,
             "%s: bad shape B=%d L=%d I=%d D=%d type=%d routing_times=%d", who, g.B, g.L, g.I, g.D, g.type, g.iters);
  RH_REQUIRE(g.D <= RH_CAPSULE_MAX_D && g.I * g.D <= RH_CAPSULE_MAX_ID && g.S >= 1 && (g.type != 2 || g.I * g.D * g.D <= RH_CAPSULE_MAX_IDD),
             RH_E_UNSUPPORTED,
             "%s: L=%d I=%d D=%d (type %d) has no HIP kernel (D <= %d, I*D <= %d, I*D*D <= %d for type 2, "
             "the routing state of one sample within 64 KB of LDS)", who, g.L, g.I, g.D, g.type, RH_CAPSULE_MAX_D, RH_CAPSULE_MAX_ID,
             RH_CAPSULE_MAX_IDD);
  return 0;
}

}  // namespace

extern "C" int rh_capsule_supported(int L, int I, int D, int type) {
  if (L < 1 || I < 1 || D < 1 || D > RH_CAPSULE_MAX_D || I * D > RH_CAPSULE_MAX_ID || type < 0 || type > 2) return 0;
  if (type == 2 && I * D * D > RH_CAPSULE_MAX_IDD) return 0;
  return caps_samples_per_block(L, I, D, type) >= 1;
}

extern "C" int rh_capsule_fwd(const float* U, const float* E, const float* W, const int32_t* mask, const float* init, int B,
                              int L, int I, int D, int type, int routing_times, float* cap, float* sw, float* s,
                              void* stream) {
  CapsGeom g{B, L, I, D, type, routing_times, 0};
  if (D >= 1 && I >= 1 && L >= 1 && I * D <= RH_CAPSULE_MAX_ID) g.S = caps_samples_per_block(L, I, D, type);
  if (int rc = caps_check("rh_capsule_fwd", g)) return rc;
  RH_REQUIRE(mask && cap && (type == 2 ? (E && W) : U != nullptr), RH_E_BADARG, "rh_capsule_fwd: null pointer");
  if (B == 0) return 0;
  const unsigned grid = (unsigned)((B + g.S - 1) / g.S);
  hipLaunchKernelGGL(capsule_fwd_kernel, dim3(grid), dim3(RH_BLOCK), caps_lds_bytes(g), reinterpret_cast<hipStream_t>(stream),
                     U, E, W, mask, init, g, cap, sw, s);
  RH_LAUNCH_CHECK("rh_capsule_fwd");
  return 0;
}

extern "C" int rh_capsule_bwd(const float* g_cap, const float* s, const float* sw, const float* W, int B, int L, int I, int D,
                              int type, float* g_u, float* g_e, float* g_s, void* stream) {
  CapsGeom g{B, L, I, D, type, 3, 0};
  if (D >= 1 && I >= 1 && L >= 1 && I * D <= RH_CAPSULE_MAX_ID) g.S = caps_samples_per_block(L, I, D, type);
  if (int rc = caps_check("rh_capsule_bwd", g)) return rc;
  RH_REQUIRE(g_cap && s && sw && (type == 2 ? (W && g_e && g_s) : g_u != nullptr), RH_E_BADARG,
             "rh_capsule_bwd: null pointer");
  if (B == 0) return 0;
  const int ID = I * D;
  const size_t lds = sizeof(float) * ((size_t)g.S * (I * L + ID) + (type == 2 ? (size_t)ID * D : 0));
  const unsigned grid = (unsigned)((B + g.S - 1) / g.S);
  hipLaunchKernelGGL(capsule_bwd_kernel, dim3(grid), dim3(RH_BLOCK), lds, reinterpret_cast<hipStream_t>(stream), g_cap, s, sw,
                     W, g, g_u, g_e, g_s);
  RH_LAUNCH_CHECK("rh_capsule_bwd");
  return 0;
}

extern "C" int rh_capsule_wgrad_nchunks(int B) { return B < 1 ? 1 : (B < kWgradChunks ? B : kWgradChunks); }

extern "C" int rh_capsule_wgrad(const float* g_s, const float* sw, const float* E, int B, int L, int I, int D, float* partial,
                                void* stream) {
  RH_REQUIRE(g_s && sw && E && partial, RH_E_BADARG, "rh_capsule_wgrad: null pointer");
  RH_REQUIRE(B >= 1 && L >= 1 && I >= 1 && D >= 1 && D <= RH_CAPSULE_MAX_D && I * D <= RH_CAPSULE_MAX_ID &&
                 I * D * D <= RH_CAPSULE_MAX_IDD,
             RH_E_UNSUPPORTED,
             "rh_capsule_wgrad: B=%d L=%d I=%d D=%d unsupported", B, L, I, D);
  CapsGeom g{B, L, I, D, 2, 3, 1};
  const int nch = rh_capsule_wgrad_nchunks(B);
  const int chunk = (B + nch - 1) / nch;
  hipLaunchKernelGGL(capsule_wgrad_kernel, dim3((unsigned)L, (unsigned)nch), dim3(RH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), g_s, sw, E, g, chunk, partial);
  RH_LAUNCH_CHECK("rh_capsule_wgrad");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Self-attentive multi-interest pooling: one wavefront per sample.
namespace {

constexpr int kLwWaves = RH_BLOCK / RH_WAVE;
constexpr int kSaMaxLI = RH_SA_MAX_LI;
static_assert(RH_SA_MAX_ID == kSaMaxLI, "gk holds a sample's I * D gradients in an array of the same size");  // L * I per sample (the softmax weights of one sample in LDS)

__global__ __launch_bounds__(RH_WAVE) void sa_fwd_kernel(const float* __restrict__ A, const float* __restrict__ E,
                                                          const int32_t* __restrict__ mask, int B, int L, int I, int D,
                                                          float* __restrict__ P, float* __restrict__ out) {
  RH_CHAIN_PRIO();
  __shared__ float p[kSaMaxLI];
  const int lane = threadIdx.x;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    for (int k = 0; k < I; ++k) {
      // A + -1e9 * (1 - mask) as the reference forms it: a fully padded row is -1e9 everywhere (uniform after softmax)
      float m = -INFINITY;
      for (int l = lane; l < L; l += RH_WAVE) {
        float v = A[(b * L + l) * I + k];
        if (mask != nullptr) v = v + -1.e9f * (1.f - (float)mask[b * L + l]);
        p[l * I + k] = v;
        m = fmaxf(m, v);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, RH_WAVE));
      float sum = 0.f;
      for (int l = lane; l < L; l += RH_WAVE) sum += expf(p[l * I + k] - m);
      sum = wave_sum(sum);
      for (int l = lane; l < L; l += RH_WAVE) {
        const float w = expf(p[l * I + k] - m) / sum;
        p[l * I + k] = w;
        P[(b * L + l) * I + k] = w;
      }
    }
    __syncthreads();
    if (lane < D) {
      for (int k = 0; k < I; ++k) {
        float acc = 0.f;
        for (int l = 0; l < L; ++l) acc = fmaf(p[l * I + k], E[(b * L + l) * D + lane], acc);
        out[(b * I + k) * D + lane] = acc;
      }
    }
    __syncthreads();
  }
}

// gP[l, k] = g_k . e_l;  gA[l, k] = P[l, k] (gP[l, k] - sum_l' P[l', k] gP[l', k]);  gE[l] = sum_k P[l, k] g_k
__global__ __launch_bounds__(RH_WAVE) void sa_bwd_kernel(const float* __restrict__ P, const float* __restrict__ E,
                                                          const float* __restrict__ G, int B, int L, int I, int D,
                                                          float* __restrict__ gA, float* __restrict__ gE) {
  RH_CHAIN_PRIO();
  __shared__ float gk[kSaMaxLI];
  const int lane = threadIdx.x;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    for (int e = lane; e < I * D; e += RH_WAVE) gk[e] = G[b * I * D + e];
    __syncthreads();
    for (int k = 0; k < I; ++k) {
      float dot = 0.f;
      for (int l = lane; l < L; l += RH_WAVE) {
        const float* er = E + (b * L + l) * D;
        float gp = 0.f;
        for (int d = 0; d < D; ++d) gp = fmaf(gk[k * D + d], er[d], gp);
        dot = fmaf(P[(b * L + l) * I + k], gp, dot);
      }
      dot = wave_sum(dot);
      for (int l = lane; l < L; l += RH_WAVE) {
        const float* er = E + (b * L + l) * D;
        float gp = 0.f;
        for (int d = 0; d < D; ++d) gp = fmaf(gk[k * D + d], er[d], gp);
        gA[(b * L + l) * I + k] = P[(b * L + l) * I + k] * (gp - dot);
      }
    }
    for (int l = lane; l < L; l += RH_WAVE) {
      for (int d = 0; d < D; ++d) {
        float acc = 0.f;
        for (int k = 0; k < I; ++k) acc = fmaf(P[(b * L + l) * I + k], gk[k * D + d], acc);
        gE[(b * L + l) * D + d] = acc;
      }
    }
    __syncthreads();
  }
}

unsigned sa_grid(int B) { return (unsigned)(B < 65536 ? B : 65536); }

unsigned lw_grid(int B) {
  int64_t grid = ((int64_t)B + kLwWaves - 1) / kLwWaves;
  if (grid > 8192) grid = 8192;
  return (unsigned)grid;
}

}  // namespace

extern "C" int rh_sa_supported(int L, int I, int D) { return L >= 1 && I >= 1 && D >= 1 && D <= RH_SA_MAX_D && L * I <= kSaMaxLI && I * D <= RH_SA_MAX_ID; }

extern "C" int rh_sa_pool_fwd(const float* A, const float* E, const int32_t* mask, int B, int L, int I, int D, float* P,
                              float* out, void* stream) {
  RH_REQUIRE(A && E && P && out, RH_E_BADARG, "rh_sa_pool_fwd: null pointer");
  RH_REQUIRE(B >= 0 && rh_sa_supported(L, I, D), RH_E_UNSUPPORTED,
             "rh_sa_pool_fwd: L=%d I=%d D=%d has no HIP kernel (D <= %d, L*I <= %d)", L, I, D, RH_SA_MAX_D, kSaMaxLI);
  if (B == 0) return 0;
  hipLaunchKernelGGL(sa_fwd_kernel, dim3(sa_grid(B)), dim3(RH_WAVE), 0, reinterpret_cast<hipStream_t>(stream), A, E, mask, B,
                     L, I, D, P, out);
  RH_LAUNCH_CHECK("rh_sa_pool_fwd");
  return 0;
}

extern "C" int rh_sa_pool_bwd(const float* P, const float* E, const float* g, int B, int L, int I, int D, float* gA, float* gE,
                              void* stream) {
  RH_REQUIRE(P && E && g && gA && gE, RH_E_BADARG, "rh_sa_pool_bwd: null pointer");
  RH_REQUIRE(B >= 0 && rh_sa_supported(L, I, D), RH_E_UNSUPPORTED, "rh_sa_pool_bwd: L=%d I=%d D=%d unsupported", L, I, D);
  if (B == 0) return 0;
  hipLaunchKernelGGL(sa_bwd_kernel, dim3(sa_grid(B)), dim3(RH_WAVE), 0, reinterpret_cast<hipStream_t>(stream), P, E, g, B, L,
                     I, D, gA, gE);
  RH_LAUNCH_CHECK("rh_sa_pool_bwd");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// List-wise scoring: one wavefront per sample, lane = embedding column (D <= 64).
namespace {

constexpr int kMaxInterests = RH_LISTWISE_MAX_I;
static_assert(RH_WAVE == RH_LISTWISE_MAX_D, "lane = embedding column");
constexpr float kNormEps = 1e-12f;

struct ListwiseArgs {
  const float* u;    // (B, I, D) contiguous
  const float* pos;  // (B, D), row stride ldp
  int64_t ldp;
  const float* neg;  // (B, K, D) contiguous
  const float* g;    // (B, 1 + K)  backward
  const int32_t* best_in;
  const float* nrm_in;
  float* logits;     // (B, 1 + K)  forward
  int32_t* best;     // (B,)
  float* nrm;        // (B, 1 + K) row norms
  float* g_u;        // (B, I, D)   backward
  float* g_pos;      // (B, D)
  float* g_neg;      // (B, K, D)
  int B, I, D, K;
  float temperature;
};

__device__ __forceinline__ const float* lw_row(const ListwiseArgs& a, int64_t b, int k) {
  return k == 0 ? a.pos + b * a.ldp : a.neg + (b * a.K + (k - 1)) * a.D;
}

template <bool BWD>
__global__ __launch_bounds__(RH_BLOCK) void listwise_kernel(const ListwiseArgs a) {
  RH_CHAIN_PRIO();
  const int lane = threadIdx.x % RH_WAVE, wave = threadIdx.x / RH_WAVE;
  const bool on = lane < a.D;
  const int K1 = a.K + 1;
  for (int64_t b = (int64_t)blockIdx.x * kLwWaves + wave; b < a.B; b += (int64_t)gridDim.x * kLwWaves) {
    if (!BWD) {
      const float pv = on ? lw_row(a, b, 0)[lane] : 0.f;
      const float n0 = sqrtf(wave_sum(pv * pv));
      const float ph = pv / fmaxf(n0, kNormEps);
      int bi = 0;
      float bd = 0.f;
      for (int i = 0; i < a.I; ++i) {
        const float d = wave_sum(on ? a.u[(b * a.I + i) * a.D + lane] * ph : 0.f);
        if (i == 0 || d > bd) {  // first maximum (NaN never wins, as in torch.argmax only for finite inputs)
          bd = d;
          bi = i;
        }
      }
      const float ub = on ? a.u[(b * a.I + bi) * a.D + lane] : 0.f;
      if (lane == 0) {
        a.best[b] = bi;
        a.nrm[b * K1] = n0;
        a.logits[b * K1] = bd / a.temperature;
      }
      for (int k = 1; k < K1; ++k) {
        const float v = on ? lw_row(a, b, k)[lane] : 0.f;
        const float n = sqrtf(wave_sum(v * v));
        const float d = wave_sum(ub * (v / fmaxf(n, kNormEps)));
        if (lane == 0) {
          a.nrm[b * K1 + k] = n;
          a.logits[b * K1 + k] = d / a.temperature;
        }
      }
    } else {
      const int bi = a.best_in[b];
      const float ub = on ? a.u[(b * a.I + bi) * a.D + lane] : 0.f;
      float gu = 0.f;
      for (int k = 0; k < K1; ++k) {
        const float v = on ? lw_row(a, b, k)[lane] : 0.f;
        const float n = a.nrm_in[b * K1 + k];
        const float inv = 1.f / fmaxf(n, kNormEps);
        const float vh = v * inv;
        const float gk = a.g[b * K1 + k] / a.temperature;
        gu = fmaf(gk, vh, gu);
        const float gvh = gk * ub;
        float dot = wave_sum(gvh * vh);
        if (!(n > kNormEps)) dot = 0.f;
        const float gv = (gvh - vh * dot) * inv;
        if (on) {
          if (k == 0) a.g_pos[b * a.D + lane] = gv;
          else a.g_neg[(b * a.K + (k - 1)) * a.D + lane] = gv;
        }
      }
      if (on) {
        for (int i = 0; i < a.I; ++i) a.g_u[(b * a.I + i) * a.D + lane] = i == bi ? gu : 0.f;
      }
    }
  }
}

}  // namespace

extern "C" int rh_listwise_fwd(const float* u, const float* pos, int64_t ldp, const float* neg, int B, int I, int D, int K,
                               float temperature, float* logits, int32_t* best, float* nrm, void* stream) {
  RH_REQUIRE(u && pos && logits && best && nrm && (neg || K == 0) && ldp >= D, RH_E_BADARG, "rh_listwise_fwd: bad arguments");
  RH_REQUIRE(B >= 0 && I >= 1 && I <= kMaxInterests && D >= 1 && D <= RH_LISTWISE_MAX_D && K >= 0 && K <= RH_LISTWISE_MAX_K, RH_E_UNSUPPORTED,
             "rh_listwise_fwd: I=%d D=%d K=%d has no HIP kernel (I <= %d, D <= %d, K <= %d)", I, D, K, kMaxInterests,
             RH_LISTWISE_MAX_D, RH_LISTWISE_MAX_K);
  if (B == 0) return 0;
  ListwiseArgs a{u, pos, ldp, neg, nullptr, nullptr, nullptr, logits, best, nrm, nullptr, nullptr, nullptr, B, I, D, K,
                 temperature};
  hipLaunchKernelGGL(listwise_kernel<false>, dim3(lw_grid(B)), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_listwise_fwd");
  return 0;
}

extern "C" int rh_listwise_bwd(const float* u, const float* pos, int64_t ldp, const float* neg, const int32_t* best,
                               const float* nrm, const float* g, int B, int I, int D, int K, float temperature, float* g_u,
                               float* g_pos, float* g_neg, void* stream) {
  RH_REQUIRE(u && pos && best && nrm && g && g_u && g_pos && (K == 0 || (neg && g_neg)) && ldp >= D, RH_E_BADARG,
             "rh_listwise_bwd: bad arguments");
  RH_REQUIRE(B >= 0 && I >= 1 && I <= kMaxInterests && D >= 1 && D <= RH_LISTWISE_MAX_D && K >= 0 && K <= RH_LISTWISE_MAX_K, RH_E_UNSUPPORTED,
             "rh_listwise_bwd: I=%d D=%d K=%d unsupported", I, D, K);
  if (B == 0) return 0;
  ListwiseArgs a{u, pos, ldp, neg, g, best, nrm, nullptr, nullptr, nullptr, g_u, g_pos, g_neg, B, I, D, K, temperature};
  hipLaunchKernelGGL(listwise_kernel<true>, dim3(lw_grid(B)), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_listwise_bwd");
  return 0;
}
