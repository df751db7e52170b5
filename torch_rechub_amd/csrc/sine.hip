// SINE's sparse-interest chain (reference torch_rechub/models/matching/sine.py:94-128) between its GEMMs.
//
// The reference runs ~30 ATen launches over (B, S, E) and (B, K, S) tensors per user tower: a masked softmax over the S
// positions, the virtual concept vector z_u and its scores against the T concept prototypes, torch.topk, the sigmoid-gated
// prototype gather, two row normalisations, a softmax over the K intentions, K more masked softmaxes over S, and three
// small contractions; then, behind the w_4 / w_5 GEMM, one more masked softmax, a normalisation, a softmax over K and
// the final mix.  Here that is two kernels each way:
//
//   rh_sine_interest_*   (sine.py:94-118) one workgroup per sample, X[b] staged in LDS once, Y[b] streamed once a row per
//                        wavefront.  The per-sample products are K <= 8 rows against (S, E): VALU work, no MFMA shape.
//   rh_sine_aggregate_*  (sine.py:122-128) one wavefront per sample, lane = embedding column (two per lane up to E = 128),
//                        in fp64 inside (see there).
//
// The forward saves the three softmaxes (P1 (B, S), P2 (B, K, S), PU (B, K, S)) and the chosen concepts; the backward
// recomputes z_u, the gates, c_u and the row norms from them.  The concept table's gradient touches K rows per sample:
// the per-sample kernel writes those rows (B, K, E) and a second kernel adds them into per-chunk (T, E) tables in LDS in
// sample order; the caller sums the chunks with rh_colsum.  No atomics anywhere: two runs give the same bits.
#include "common.h"

namespace {

constexpr int kMaxS = RH_SINE_MAX_S;   // positions: one lane per position in the softmaxes over S
constexpr int kMaxE = RH_SINE_MAX_E;  // embedding columns: two per lane
constexpr int kMaxT = RH_SINE_MAX_T;   // concepts: one lane per concept in the top-k
constexpr int kMaxK = RH_SINE_MAX_K;    // intentions: per-row scores in registers
constexpr int kChunks = 64;
constexpr int kWaves = RH_BLOCK / RH_WAVE;
constexpr float kNormEps = 1e-12f;

struct SineGeom {
  int B, S, E, T, K;
};

__host__ __device__ inline bool sine_shape_ok(int S, int E, int T, int K) {
  return S >= 1 && S <= kMaxS && E >= 1 && E <= kMaxE && T >= 1 && T <= kMaxT && K >= 1 && K <= kMaxK && K <= T;
}

// LDS floats.  At the largest shape (S 64, E 128, K 8): forward 11 728 (46 KB), backward 15 848 (62 KB) -- within the
// 64 KB a workgroup may take without an opt-in, two (three) workgroups per CU at the limits and four at the example's
// 50 / 128 / 10 / 2 (33 KB).
size_t sine_fwd_lds(const SineGeom& g) {
  return sizeof(float) * ((size_t)g.S * g.E + 2 * g.K * g.E + 2 * g.K * g.S + g.S + g.E + g.T + 2 * kMaxK);
}
size_t sine_bwd_lds(const SineGeom& g) {
  return sizeof(float) * ((size_t)g.S * g.E + 5 * g.K * g.E + 4 * g.K * g.S + 3 * g.S + 2 * g.E + 5 * kMaxK);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, RH_WAVE));
  return v;
}

// softmax over the S <= 64 positions of a[s * stride] + -1e9 (1 - mask[s]), lane = position: the mask term is added in
// fp32 as the reference adds it, so a fully padded row is -1e9 everywhere and comes out uniform.  Lanes >= S return 0.
__device__ __forceinline__ float masked_softmax_lane(const float* __restrict__ a, int stride, const int32_t* __restrict__ mask,
                                                     int S, int lane) {
  float v = -INFINITY;
  if (lane < S) v = a[(int64_t)lane * stride] + -1.e9f * (1.f - (float)mask[lane]);
  const float m = wave_max(v);
  const float ex = lane < S ? expf(v - m) : 0.f;
  return ex / wave_sum(ex);
}

// n contiguous floats global -> LDS; dwordx4 when n is a multiple of four.  Only dst (LDS, offset 0 of a 16-byte aligned
// array) needs the alignment: gload<float4> reads through common.h's 4-byte aligned vector type, so src may sit at any
// dword (a view with an odd storage offset included)
__device__ __forceinline__ void stage_rows(float* dst, const float* __restrict__ src, int n, int tid) {
  if ((n & 3) == 0) {
    for (int i = tid * 4; i < n; i += RH_BLOCK * 4) *reinterpret_cast<float4*>(dst + i) = gload<float4>(src + i);
  } else {
    for (int i = tid; i < n; i += RH_BLOCK) dst[i] = src[i];
  }
}

// the gated prototypes of one sample: c_u[k] = gate[k] C[sel[k]] into cu, c_u[k] / max(|c_u[k]|, eps) into ch,
// 1 / max(|c_u[k]|, eps) into ninv (and whether the norm was above eps into nlive, when asked)
__device__ __forceinline__ void gated_prototypes(const float* __restrict__ C, const int* sel, const float* gate, int E, int K,
                                                 float* cu, float* ch, float* ninv, float* nlive) {
  const int lane = threadIdx.x % RH_WAVE, wave = threadIdx.x / RH_WAVE;
  const bool on0 = lane < E, on1 = lane + RH_WAVE < E;
  for (int k = wave; k < K; k += kWaves) {
    const float* c = C + (int64_t)sel[k] * E;
    const float c0 = on0 ? gate[k] * c[lane] : 0.f, c1 = on1 ? gate[k] * c[lane + RH_WAVE] : 0.f;
    const float n = sqrtf(wave_sum(fmaf(c0, c0, c1 * c1)));
    const float inv = 1.f / fmaxf(n, kNormEps);
    if (on0) {
      cu[k * E + lane] = c0;
      ch[k * E + lane] = c0 * inv;
    }
    if (on1) {
      cu[k * E + lane + RH_WAVE] = c1;
      ch[k * E + lane + RH_WAVE] = c1 * inv;
    }
    if (lane == 0) {
      ninv[k] = inv;
      if (nlive != nullptr) nlive[k] = n > kNormEps ? 1.f : 0.f;
    }
  }
}

__global__ __launch_bounds__(RH_BLOCK) void sine_interest_fwd_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ a1, const float* __restrict__ a2,
    const int32_t* __restrict__ mask, const float* __restrict__ C, const SineGeom g, int32_t* __restrict__ idx_out,
    float* __restrict__ phi, float* __restrict__ xhat, float* __restrict__ P1o, float* __restrict__ P2o,
    float* __restrict__ PUo) {
  RH_CHAIN_PRIO();
  extern __shared__ __align__(16) float lds[];
  const int S = g.S, E = g.E, T = g.T, K = g.K;
  float* xs = lds;            // [S][E]
  float* cu = xs + S * E;     // [K][E] gated prototypes
  float* ch = cu + K * E;     // [K][E] ... normalised
  float* p2 = ch + K * E;     // [K][S] softmax over S of a2[:, k]
  float* pu = p2 + K * S;     // [K][S] softmax over K of yh[s] . ch[k]
  float* p1 = pu + K * S;     // [S]
  float* zu = p1 + S;         // [E]
  float* su = zu + E;         // [T]
  float* gate = su + T;       // [kMaxK]
  int* sel = reinterpret_cast<int*>(gate + kMaxK);  // [kMaxK]
  const int tid = threadIdx.x, lane = tid % RH_WAVE, wave = tid / RH_WAVE;
  const bool on0 = lane < E, on1 = lane + RH_WAVE < E;
  const int64_t b = blockIdx.x;
  const int32_t* mb = mask + b * S;
  stage_rows(xs, X + b * S * E, S * E, tid);
  for (int j = wave; j <= K; j += kWaves) {  // column 0: a1; column 1 + k: a2[:, k]
    if (j == 0) {
      const float p = masked_softmax_lane(a1 + b * S, 1, mb, S, lane);
      if (lane < S) {
        p1[lane] = p;
        P1o[b * S + lane] = p;
      }
    } else {
      const float p = masked_softmax_lane(a2 + b * S * K + (j - 1), K, mb, S, lane);
      if (lane < S) {
        p2[(j - 1) * S + lane] = p;
        P2o[(b * K + (j - 1)) * S + lane] = p;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < E; e += RH_BLOCK) {  // z_u = P1^T X
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc = fmaf(p1[s], xs[s * E + e], acc);
    zu[e] = acc;
  }
  __syncthreads();
  for (int t = wave; t < T; t += kWaves) {  // s_u = z_u C^T
    const float* c = C + (int64_t)t * E;
    float d = on0 ? zu[lane] * c[lane] : 0.f;
    if (on1) d = fmaf(zu[lane + RH_WAVE], c[lane + RH_WAVE], d);
    d = wave_sum(d);
    if (lane == 0) su[t] = d;
  }
  __syncthreads();
  if (wave == 0) {  // the K largest scores in descending order, ties to the lower index (torch.topk, sorted)
    float v = lane < T ? su[lane] : -INFINITY;
    int key = lane < T ? lane : RH_WAVE + lane;  // a taken lane sorts behind every live one
    for (int k = 0; k < K; ++k) {
      float bv = v;
      int bi = key;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(bv, o, RH_WAVE);
        const int oi = __shfl_xor(bi, o, RH_WAVE);
        if (ov > bv || (ov == bv && oi < bi)) {
          bv = ov;
          bi = oi;
        }
      }
      int r = bi & (RH_WAVE - 1);
      if (r >= T) r = T - 1;  // (only reachable with NaN scores: keep the gather in bounds)
      if (lane == 0) {
        sel[k] = r;
        gate[k] = 1.f / (1.f + expf(-bv));
        idx_out[b * K + k] = r;
      }
      if (lane == r) {
        v = -INFINITY;
        key = RH_WAVE + lane;
      }
    }
  }
  __syncthreads();
  gated_prototypes(C, sel, gate, E, K, cu, ch, su /* 1 / norm: s_u is done with */, nullptr);
  __syncthreads();
  const float* Yb = Y + b * S * E;
  for (int s = wave; s < S; s += kWaves) {  // p_u[:, s] = softmax over k of normalize(Y[s]) . normalize(c_u[k])
    const float y0 = on0 ? Yb[s * E + lane] : 0.f, y1 = on1 ? Yb[s * E + lane + RH_WAVE] : 0.f;
    const float inv = 1.f / fmaxf(sqrtf(wave_sum(fmaf(y0, y0, y1 * y1))), kNormEps);
    float d[kMaxK];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      d[k] = -INFINITY;
      if (k < K) {
        float t = on0 ? y0 * ch[k * E + lane] : 0.f;
        if (on1) t = fmaf(y1, ch[k * E + lane + RH_WAVE], t);
        d[k] = wave_sum(t) * inv;
        m = fmaxf(m, d[k]);
      }
    }
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      d[k] = k < K ? expf(d[k] - m) : 0.f;
      sum += d[k];
    }
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      if (k < K && lane == k) {
        const float p = d[k] / sum;
        pu[k * S + s] = p;
        PUo[(b * K + k) * S + s] = p;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < K * E; i += RH_BLOCK) {  // phi[k] = sum_s p_u[k, s] P2[s, k] X[s]
    const int k = i / E, e = i % E;
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc = fmaf(pu[k * S + s] * p2[k * S + s], xs[s * E + e], acc);
    phi[b * K * E + i] = acc;
  }
  for (int i = tid; i < S * E; i += RH_BLOCK) {  // xhat[s] = sum_k p_u[k, s] c_u[k]
    const int s = i / E, e = i % E;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(pu[k * S + s], cu[k * E + e], acc);
    xhat[b * S * E + i] = acc;
  }
}

// One workgroup per sample.  With w = p_u P2, yh / ch the normalised rows and d = yh ch^T:
//   g_w[k, s] = g_phi[k] . X[s];  g_pu = g_w P2 + g_xhat[s] . c_u[k];  g_P2 = g_w p_u;  g_d = softmax'(g_pu) over k;
//   g_Y[s] = normalize'(sum_k g_d[k, s] ch[k]);  g_cu[k] = sum_s p_u[k, s] g_xhat[s] + normalize'(sum_s g_d[k, s] yh[s]);
//   g_gate[k] = g_cu[k] . C[idx[k]];  g_st[k] = g_gate[k] gate (1 - gate);  g_C[idx[k]] = gate g_cu[k] + g_st[k] z_u;
//   g_z = sum_k g_st[k] C[idx[k]];  g_P1[s] = g_z . X[s];  g_X[s] = sum_k w[k, s] g_phi[k] + P1[s] g_z;
//   g_a1 = softmax'(g_P1) over s;  g_a2[:, k] = softmax'(g_P2[:, k]) over s.
__global__ __launch_bounds__(RH_BLOCK) void sine_interest_bwd_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ C, const int32_t* __restrict__ idx,
    const float* __restrict__ P1, const float* __restrict__ P2, const float* __restrict__ PU,
    const float* __restrict__ g_phi, const float* __restrict__ g_xhat, const SineGeom g, float* __restrict__ g_X,
    float* __restrict__ g_Y, float* __restrict__ g_a1, float* __restrict__ g_a2, float* __restrict__ g_crow) {
  RH_CHAIN_PRIO();
  extern __shared__ __align__(16) float lds[];
  const int S = g.S, E = g.E, T = g.T, K = g.K;
  float* xs = lds;             // [S][E]
  float* gph = xs + S * E;     // [K][E] g_phi
  float* cu = gph + K * E;     // [K][E]
  float* ch = cu + K * E;      // [K][E]
  float* gcu = ch + K * E;     // [K][E] sum_s p_u g_xhat
  float* gch = gcu + K * E;    // [K][E] sum_s g_d yh, then g_st[k] C[idx[k]]
  float* p2 = gch + K * E;     // [K][S]
  float* pu = p2 + K * S;      // [K][S]
  float* gp2 = pu + K * S;     // [K][S]
  float* gd = gp2 + K * S;     // [K][S]
  float* p1 = gd + K * S;      // [S]
  float* gp1 = p1 + S;         // [S]
  float* invy = gp1 + S;       // [S] 1 / max(|Y[s]|, eps)
  float* zu = invy + S;        // [E]
  float* gz = zu + E;          // [E]
  float* gate = gz + E;        // [kMaxK]
  float* ninv = gate + kMaxK;  // [kMaxK]
  float* nlive = ninv + kMaxK;  // [kMaxK]
  float* st = nlive + kMaxK;   // [kMaxK]
  int* sel = reinterpret_cast<int*>(st + kMaxK);  // [kMaxK]
  const int tid = threadIdx.x, lane = tid % RH_WAVE, wave = tid / RH_WAVE;
  const bool on0 = lane < E, on1 = lane + RH_WAVE < E;
  const int64_t b = blockIdx.x;
  stage_rows(xs, X + b * S * E, S * E, tid);
  for (int i = tid; i < K * E; i += RH_BLOCK) gph[i] = g_phi[b * K * E + i];
  for (int i = tid; i < K * S; i += RH_BLOCK) {
    p2[i] = P2[b * K * S + i];
    pu[i] = PU[b * K * S + i];
  }
  for (int i = tid; i < S; i += RH_BLOCK) p1[i] = P1[b * S + i];
  if (tid < K) {
    int r = idx[b * K + tid];
    sel[tid] = r < 0 ? 0 : (r >= T ? T - 1 : r);
  }
  __syncthreads();
  for (int e = tid; e < E; e += RH_BLOCK) {
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc = fmaf(p1[s], xs[s * E + e], acc);
    zu[e] = acc;
  }
  __syncthreads();
  for (int k = wave; k < K; k += kWaves) {  // the chosen scores and their gates, as the forward formed them
    const float* c = C + (int64_t)sel[k] * E;
    float d = on0 ? zu[lane] * c[lane] : 0.f;
    if (on1) d = fmaf(zu[lane + RH_WAVE], c[lane + RH_WAVE], d);
    d = wave_sum(d);
    if (lane == 0) {
      st[k] = d;
      gate[k] = 1.f / (1.f + expf(-d));
    }
  }
  __syncthreads();
  gated_prototypes(C, sel, gate, E, K, cu, ch, ninv, nlive);
  __syncthreads();
  const float* Yb = Y + b * S * E;
  const float* Gb = g_xhat + b * S * E;
  for (int s = wave; s < S; s += kWaves) {
    const float x0 = on0 ? xs[s * E + lane] : 0.f, x1 = on1 ? xs[s * E + lane + RH_WAVE] : 0.f;
    const float y0 = on0 ? Yb[s * E + lane] : 0.f, y1 = on1 ? Yb[s * E + lane + RH_WAVE] : 0.f;
    const float q0 = on0 ? Gb[s * E + lane] : 0.f, q1 = on1 ? Gb[s * E + lane + RH_WAVE] : 0.f;
    const float ny = sqrtf(wave_sum(fmaf(y0, y0, y1 * y1)));
    const float inv = 1.f / fmaxf(ny, kNormEps);
    const float yh0 = y0 * inv, yh1 = y1 * inv;
    float gpu_[kMaxK];
    float dotp = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      gpu_[k] = 0.f;
      if (k < K) {
        float t = on0 ? gph[k * E + lane] * x0 : 0.f;
        if (on1) t = fmaf(gph[k * E + lane + RH_WAVE], x1, t);
        const float gw = wave_sum(t);
        float u = on0 ? cu[k * E + lane] * q0 : 0.f;
        if (on1) u = fmaf(cu[k * E + lane + RH_WAVE], q1, u);
        const float gxc = wave_sum(u);
        const float pk = pu[k * S + s];
        gpu_[k] = fmaf(gw, p2[k * S + s], gxc);
        dotp = fmaf(pk, gpu_[k], dotp);
        if (lane == 0) gp2[k * S + s] = gw * pk;
      }
    }
    float gy0 = 0.f, gy1 = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      if (k < K) {
        const float gdk = pu[k * S + s] * (gpu_[k] - dotp);
        if (lane == 0) gd[k * S + s] = gdk;
        if (on0) gy0 = fmaf(gdk, ch[k * E + lane], gy0);
        if (on1) gy1 = fmaf(gdk, ch[k * E + lane + RH_WAVE], gy1);
      }
    }
    float dot = wave_sum(fmaf(gy0, yh0, gy1 * yh1));
    if (!(ny > kNormEps)) dot = 0.f;  // the clamped norm is a constant
    if (on0) g_Y[b * S * E + s * E + lane] = (gy0 - yh0 * dot) * inv;
    if (on1) g_Y[b * S * E + s * E + lane + RH_WAVE] = (gy1 - yh1 * dot) * inv;
    if (lane == 0) invy[s] = inv;
  }
  __syncthreads();
  for (int i = tid; i < K * E; i += RH_BLOCK) {
    const int k = i / E, e = i % E;
    float a = 0.f, c = 0.f;
    for (int s = 0; s < S; ++s) {
      a = fmaf(pu[k * S + s], Gb[s * E + e], a);
      c = fmaf(gd[k * S + s] * invy[s], Yb[s * E + e], c);
    }
    gcu[i] = a;
    gch[i] = c;
  }
  __syncthreads();
  for (int k = wave; k < K; k += kWaves) {
    const float* c = C + (int64_t)sel[k] * E;
    const float h0 = on0 ? ch[k * E + lane] : 0.f, h1 = on1 ? ch[k * E + lane + RH_WAVE] : 0.f;
    const float a0 = on0 ? gch[k * E + lane] : 0.f, a1_ = on1 ? gch[k * E + lane + RH_WAVE] : 0.f;
    float dot = wave_sum(fmaf(h0, a0, h1 * a1_));
    if (nlive[k] == 0.f) dot = 0.f;
    const float t0 = (on0 ? gcu[k * E + lane] : 0.f) + (a0 - h0 * dot) * ninv[k];
    const float t1 = (on1 ? gcu[k * E + lane + RH_WAVE] : 0.f) + (a1_ - h1 * dot) * ninv[k];
    const float c0 = on0 ? c[lane] : 0.f, c1 = on1 ? c[lane + RH_WAVE] : 0.f;
    const float gt = gate[k];
    const float gst = wave_sum(fmaf(t0, c0, t1 * c1)) * gt * (1.f - gt);
    float* row = g_crow + (b * K + k) * E;
    if (on0) {
      row[lane] = fmaf(gt, t0, gst * zu[lane]);
      gch[k * E + lane] = gst * c0;
    }
    if (on1) {
      row[lane + RH_WAVE] = fmaf(gt, t1, gst * zu[lane + RH_WAVE]);
      gch[k * E + lane + RH_WAVE] = gst * c1;
    }
  }
  __syncthreads();
  for (int e = tid; e < E; e += RH_BLOCK) {
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc += gch[k * E + e];
    gz[e] = acc;
  }
  __syncthreads();
  for (int s = wave; s < S; s += kWaves) {
    float d = on0 ? gz[lane] * xs[s * E + lane] : 0.f;
    if (on1) d = fmaf(gz[lane + RH_WAVE], xs[s * E + lane + RH_WAVE], d);
    d = wave_sum(d);
    if (lane == 0) gp1[s] = d;
  }
  __syncthreads();
  for (int j = wave; j <= K; j += kWaves) {  // the softmaxes over S, backward
    const float p = lane < S ? (j == 0 ? p1[lane] : p2[(j - 1) * S + lane]) : 0.f;
    const float gp = lane < S ? (j == 0 ? gp1[lane] : gp2[(j - 1) * S + lane]) : 0.f;
    const float dot = wave_sum(p * gp);
    if (lane < S) {
      if (j == 0) g_a1[b * S + lane] = p * (gp - dot);
      else g_a2[(b * S + lane) * K + (j - 1)] = p * (gp - dot);
    }
  }
  for (int i = tid; i < S * E; i += RH_BLOCK) {
    const int s = i / E, e = i % E;
    float acc = p1[s] * gz[e];
    for (int k = 0; k < K; ++k) acc = fmaf(pu[k * S + s] * p2[k * S + s], gph[k * E + e], acc);
    g_X[b * S * E + i] = acc;
  }
}

// partial[c] (T, E) = the rows g_crow[b, k] of the samples b of chunk c added into row idx[b, k], in (b, k) order; a thread
// owns its columns of every row, so there is nothing to synchronise but the start
__global__ __launch_bounds__(kMaxE) void sine_cgrad_kernel(const float* __restrict__ g_crow, const int32_t* __restrict__ idx,
                                                           const SineGeom g, int chunk, float* __restrict__ partial) {
  extern __shared__ __align__(16) float lds[];
  const int E = g.E, T = g.T, K = g.K, tid = threadIdx.x;
  for (int i = tid; i < T * E; i += kMaxE) lds[i] = 0.f;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  int64_t hi = lo + chunk;
  if (hi > g.B) hi = g.B;
  if (tid < E) {
    for (int64_t b = lo; b < hi; ++b) {
      for (int k = 0; k < K; ++k) {
        int r = idx[b * K + k];
        r = r < 0 ? 0 : (r >= T ? T - 1 : r);
        lds[r * E + tid] += g_crow[(b * K + k) * E + tid];
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < T * E; i += kMaxE) partial[(int64_t)blockIdx.x * T * E + i] = lds[i];
}

// ---------------------------------------------------------------------------------------------------------------------
// Interest aggregation.  sine.py:122 calls F.normalize(m, -1), whose second positional argument is the norm's ORDER p (the
// axis stays at its default, 1, the last one of a (B, E) tensor): the reference divides the adapted intention m by its
// p = -1 "norm" n = 1 / sum_e 1 / |m_e|, not by its length.  n is about the smallest |m_e|, a coordinate where the sum over
// the positions nearly cancels, so in fp32 its relative error is eps |xhat| / min_e |m_e| (1e-3 for the unluckiest row of a
// batch), and it scales every logit and, through dn / dm_e = n^2 / m_e^2, the largest entries of the gradient.  These two
// kernels therefore carry the softmax over S, m, n, the K logits and their softmax in fp64 (S E fused multiply-adds per
// sample: the kernels stay bound by reading xhat), and the backward recomputes them from the inputs instead of reading
// fp32 copies: outputs are exact to their fp32 rounding.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, RH_WAVE);
  return v;
}

struct AggState {
  double p;           // P3[lane] (0 for lanes >= S)
  double m0, m1;      // m = P3^T xhat, columns lane and lane + 64
  double n, inv;      // |m|_{-1} and 1 / max(n, eps)
  double e[kMaxK];    // softmax_k(c . phi[k] / t), c = m inv
  float f0[kMaxK], f1[kMaxK];  // phi[k], columns lane and lane + 64
};

// one wavefront: the forward chain of sample b (every lane of the wavefront must be active)
__device__ __forceinline__ void aggregate_state(const float* __restrict__ xh, const float* __restrict__ a3,
                                                const int32_t* __restrict__ mask, const float* __restrict__ ph, double inv_t,
                                                int S, int E, int K, int lane, AggState& st) {
  const bool on0 = lane < E, on1 = lane + RH_WAVE < E;
  // a3 + -1e9 (1 - mask) in fp32 as the reference forms it (a fully padded row is -1e9 everywhere: uniform), then fp64
  float vf = -INFINITY;
  if (lane < S) vf = a3[lane] + -1.e9f * (1.f - (float)mask[lane]);
  const float mx = wave_max(vf);
  const double ex = lane < S ? exp((double)vf - (double)mx) : 0.0;
  st.p = ex / wave_sum_f64(ex);
  st.m0 = st.m1 = 0.0;
  for (int s = 0; s < S; ++s) {
    const double ps = __shfl(st.p, s, RH_WAVE);
    if (on0) st.m0 = fma(ps, (double)xh[s * E + lane], st.m0);
    if (on1) st.m1 = fma(ps, (double)xh[s * E + lane + RH_WAVE], st.m1);
  }
  st.n = 1.0 / wave_sum_f64((on0 ? 1.0 / fabs(st.m0) : 0.0) + (on1 ? 1.0 / fabs(st.m1) : 0.0));
  st.inv = 1.0 / fmax(st.n, (double)kNormEps);
  const double c0 = st.m0 * st.inv, c1 = st.m1 * st.inv;
  double mxl = -INFINITY;
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) {
    st.f0[k] = st.f1[k] = 0.f;
    st.e[k] = -INFINITY;
    if (k < K) {
      if (on0) st.f0[k] = ph[k * E + lane];
      if (on1) st.f1[k] = ph[k * E + lane + RH_WAVE];
      st.e[k] = wave_sum_f64(c0 * (double)st.f0[k] + c1 * (double)st.f1[k]) * inv_t;
      mxl = fmax(mxl, st.e[k]);
    }
  }
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) {
    st.e[k] = k < K ? exp(st.e[k] - mxl) : 0.0;
    sum += st.e[k];
  }
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) st.e[k] /= sum;
}

// One wavefront per sample: P3 = masked softmax of a3 over S, m = P3^T xhat, c = m / max(|m|_{-1}, eps),
// e = softmax_k(c . phi[k] / t), v = sum_k e[k] phi[k].
__global__ __launch_bounds__(RH_BLOCK) void sine_aggregate_fwd_kernel(const float* __restrict__ xhat, const float* __restrict__ a3,
                                                                      const int32_t* __restrict__ mask,
                                                                      const float* __restrict__ phi, float inv_t,
                                                                      const SineGeom g, float* __restrict__ v) {
  RH_CHAIN_PRIO();
  const int S = g.S, E = g.E, K = g.K;
  const int lane = threadIdx.x % RH_WAVE, wave = threadIdx.x / RH_WAVE;
  for (int64_t b = (int64_t)blockIdx.x * kWaves + wave; b < g.B; b += (int64_t)gridDim.x * kWaves) {
    AggState st;
    aggregate_state(xhat + b * S * E, a3 + b * S, mask + b * S, phi + b * K * E, (double)inv_t, S, E, K, lane, st);
    double v0 = 0.0, v1 = 0.0;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      if (k < K) {
        v0 = fma(st.e[k], (double)st.f0[k], v0);
        v1 = fma(st.e[k], (double)st.f1[k], v1);
      }
    }
    if (lane < E) v[b * E + lane] = (float)v0;
    if (lane + RH_WAVE < E) v[b * E + lane + RH_WAVE] = (float)v1;
  }
}

//   g_e[k] = g_v . phi[k];  g_l = softmax'(g_e) / t;  g_c = sum_k g_l[k] phi[k];  g_phi[k] = e[k] g_v + g_l[k] c;
//   g_m = g_c / n - (c . g_c) n sign(m) / m^2 (n = |m|_{-1} > eps; the clamped norm is a constant);
//   g_P3[s] = g_m . xhat[s];  g_xhat[s] = P3[s] g_m;  g_a3 = softmax'(g_P3) over s.
__global__ __launch_bounds__(RH_BLOCK) void sine_aggregate_bwd_kernel(const float* __restrict__ xhat, const float* __restrict__ a3,
                                                                      const int32_t* __restrict__ mask,
                                                                      const float* __restrict__ phi, const float* __restrict__ g_v,
                                                                      float inv_t, const SineGeom g, float* __restrict__ g_xhat,
                                                                      float* __restrict__ g_a3, float* __restrict__ g_phi) {
  RH_CHAIN_PRIO();
  const int S = g.S, E = g.E, K = g.K;
  const int lane = threadIdx.x % RH_WAVE, wave = threadIdx.x / RH_WAVE;
  const bool on0 = lane < E, on1 = lane + RH_WAVE < E;
  for (int64_t b = (int64_t)blockIdx.x * kWaves + wave; b < g.B; b += (int64_t)gridDim.x * kWaves) {
    const float* xh = xhat + b * S * E;
    AggState st;
    aggregate_state(xh, a3 + b * S, mask + b * S, phi + b * K * E, (double)inv_t, S, E, K, lane, st);
    const double q0 = on0 ? (double)g_v[b * E + lane] : 0.0, q1 = on1 ? (double)g_v[b * E + lane + RH_WAVE] : 0.0;
    const double c0 = st.m0 * st.inv, c1 = st.m1 * st.inv;
    double ge[kMaxK];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      ge[k] = 0.0;
      if (k < K) {
        ge[k] = wave_sum_f64(q0 * (double)st.f0[k] + q1 * (double)st.f1[k]);
      }
    }
    double gc0 = 0.0, gc1 = 0.0;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      if (k < K) {
        // e_k (g_e[k] - sum_j e_j g_e[j]) as e_k sum_j e_j (g_e[k] - g_e[j]): with a saturated softmax (logits of hundreds) the
        // first form cancels to nothing but rounding
        double gl = 0.0;
#pragma unroll
        for (int j = 0; j < kMaxK; ++j) {
          if (j < K) gl = fma(st.e[j], ge[k] - ge[j], gl);
        }
        gl *= st.e[k] * (double)inv_t;
        gc0 = fma(gl, (double)st.f0[k], gc0);
        gc1 = fma(gl, (double)st.f1[k], gc1);
        if (on0) g_phi[(b * K + k) * E + lane] = (float)fma(st.e[k], q0, gl * c0);
        if (on1) g_phi[(b * K + k) * E + lane + RH_WAVE] = (float)fma(st.e[k], q1, gl * c1);
      }
    }
    const double dc = wave_sum_f64(gc0 * c0 + gc1 * c1);
    const bool live = st.n > (double)kNormEps;
    const double gm0 = gc0 * st.inv - (live && on0 ? dc * st.n / (st.m0 * fabs(st.m0)) : 0.0);
    const double gm1 = gc1 * st.inv - (live && on1 ? dc * st.n / (st.m1 * fabs(st.m1)) : 0.0);
    double gp = 0.0;
    for (int s = 0; s < S; ++s) {
      const double ps = __shfl(st.p, s, RH_WAVE);
      double d = on0 ? gm0 * (double)xh[s * E + lane] : 0.0;
      if (on1) d = fma(gm1, (double)xh[s * E + lane + RH_WAVE], d);
      d = wave_sum_f64(d);
      if (lane == s) gp = d;
      if (on0) g_xhat[b * S * E + s * E + lane] = (float)(ps * gm0);
      if (on1) g_xhat[b * S * E + s * E + lane + RH_WAVE] = (float)(ps * gm1);
    }
    const double dp = wave_sum_f64(st.p * gp);
    if (lane < S) g_a3[b * S + lane] = (float)(st.p * (gp - dp));
  }
}

int sine_check(const char* who, int B, int S, int E, int T, int K) {
  RH_REQUIRE(B >= 0, RH_E_BADARG, "%s: B=%d", who, B);
  RH_REQUIRE(sine_shape_ok(S, E, T, K), RH_E_UNSUPPORTED,
             "%s: S=%d E=%d T=%d K=%d has no HIP kernel (1 <= S <= %d, 1 <= E <= %d, 1 <= T <= %d, 1 <= K <= min(T, %d))", who,
             S, E, T, K, kMaxS, kMaxE, kMaxT, kMaxK);
  return 0;
}

unsigned wave_grid(int B) {
  int64_t grid = ((int64_t)B + kWaves - 1) / kWaves;
  if (grid > 16384) grid = 16384;
  return (unsigned)grid;
}

}  // namespace

static int sine_nchunks(int B) { return B < 1 ? 1 : (B < kChunks ? B : kChunks); }

extern "C" int rh_sine_supported(int S, int E, int T, int K, int* supported) {
  RH_REQUIRE(supported != nullptr, RH_E_BADARG, "rh_sine_supported: null pointer");
  *supported = sine_shape_ok(S, E, T, K) ? 1 : 0;
  return 0;
}

extern "C" int rh_sine_nchunks(int B, int* nchunks) {
  RH_REQUIRE(nchunks != nullptr, RH_E_BADARG, "rh_sine_nchunks: null pointer");
  *nchunks = sine_nchunks(B);
  return 0;
}

extern "C" int rh_sine_interest_fwd(const float* X, const float* Y, const float* a1, const float* a2, const int32_t* mask,
                                    const float* C, int B, int S, int E, int T, int K, int32_t* idx, float* phi, float* xhat,
                                    float* P1, float* P2, float* PU, void* stream) {
  if (int rc = sine_check("rh_sine_interest_fwd", B, S, E, T, K)) return rc;
  RH_REQUIRE(X && Y && a1 && a2 && mask && C && idx && phi && xhat && P1 && P2 && PU, RH_E_BADARG,
             "rh_sine_interest_fwd: null pointer");
  if (B == 0) return 0;
  const SineGeom g{B, S, E, T, K};
  hipLaunchKernelGGL(sine_interest_fwd_kernel, dim3((unsigned)B), dim3(RH_BLOCK), sine_fwd_lds(g),
                     reinterpret_cast<hipStream_t>(stream), X, Y, a1, a2, mask, C, g, idx, phi, xhat, P1, P2, PU);
  RH_LAUNCH_CHECK("rh_sine_interest_fwd");
  return 0;
}

extern "C" int rh_sine_interest_bwd(const float* X, const float* Y, const float* C, const int32_t* idx, const float* P1,
                                    const float* P2, const float* PU, const float* g_phi, const float* g_xhat, int B, int S,
                                    int E, int T, int K, float* g_X, float* g_Y, float* g_a1, float* g_a2, float* g_crow,
                                    float* c_partial, void* stream) {
  if (int rc = sine_check("rh_sine_interest_bwd", B, S, E, T, K)) return rc;
  RH_REQUIRE(X && Y && C && idx && P1 && P2 && PU && g_phi && g_xhat && g_X && g_Y && g_a1 && g_a2 && g_crow && c_partial,
             RH_E_BADARG, "rh_sine_interest_bwd: null pointer");
  if (B == 0) return 0;
  const SineGeom g{B, S, E, T, K};
  hipLaunchKernelGGL(sine_interest_bwd_kernel, dim3((unsigned)B), dim3(RH_BLOCK), sine_bwd_lds(g),
                     reinterpret_cast<hipStream_t>(stream), X, Y, C, idx, P1, P2, PU, g_phi, g_xhat, g, g_X, g_Y, g_a1, g_a2,
                     g_crow);
  RH_LAUNCH_CHECK("rh_sine_interest_bwd");
  const int nch = sine_nchunks(B);
  const int chunk = (B + nch - 1) / nch;
  hipLaunchKernelGGL(sine_cgrad_kernel, dim3((unsigned)nch), dim3(kMaxE), sizeof(float) * (size_t)T * E,
                     reinterpret_cast<hipStream_t>(stream), g_crow, idx, g, chunk, c_partial);
  RH_LAUNCH_CHECK("rh_sine_interest_bwd (concept gradient)");
  return 0;
}

extern "C" int rh_sine_aggregate_fwd(const float* xhat, const float* a3, const int32_t* mask, const float* phi,
                                     float inv_temperature, int B, int S, int E, int K, float* v, void* stream) {
  if (int rc = sine_check("rh_sine_aggregate_fwd", B, S, E, kMaxT, K)) return rc;
  RH_REQUIRE(xhat && a3 && mask && phi && v, RH_E_BADARG, "rh_sine_aggregate_fwd: null pointer");
  if (B == 0) return 0;
  const SineGeom g{B, S, E, 0, K};
  hipLaunchKernelGGL(sine_aggregate_fwd_kernel, dim3(wave_grid(B)), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream),
                     xhat, a3, mask, phi, inv_temperature, g, v);
  RH_LAUNCH_CHECK("rh_sine_aggregate_fwd");
  return 0;
}

extern "C" int rh_sine_aggregate_bwd(const float* xhat, const float* a3, const int32_t* mask, const float* phi,
                                     const float* g_v, float inv_temperature, int B, int S, int E, int K, float* g_xhat,
                                     float* g_a3, float* g_phi, void* stream) {
  if (int rc = sine_check("rh_sine_aggregate_bwd", B, S, E, kMaxT, K)) return rc;
  RH_REQUIRE(xhat && a3 && mask && phi && g_v && g_xhat && g_a3 && g_phi, RH_E_BADARG, "rh_sine_aggregate_bwd: null pointer");
  if (B == 0) return 0;
  const SineGeom g{B, S, E, 0, K};
  hipLaunchKernelGGL(sine_aggregate_bwd_kernel, dim3(wave_grid(B)), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream),
                     xhat, a3, mask, phi, g_v, inv_temperature, g, g_xhat, g_a3, g_phi);
  RH_LAUNCH_CHECK("rh_sine_aggregate_bwd");
  return 0;
}
