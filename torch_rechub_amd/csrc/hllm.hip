// HLLM (generative next-item model): causal softmax multi-head attention with an additive per-head bucketed
// relative-position bias and dropout on the attention weights, forward and backward.
//
// Reference HLLMTransformerBlock.forward torch_rechub/models/generative/hllm.py:69-88 with RelPosBias.forward
// utils/hstu_utils.py:54-68:
//   S[i, j] = scale q_i . k_j + table[bucket(i, j), h]  for j <= i,  -inf above the diagonal,
//   bucket(i, j) = min(|i - j|, N) * (nb - 1) / N  (integers),  P = softmax_j S,  O = dropout(P) V.
// The reference materialises the (B, H, L, L) scores, the masked scores, the softmax, the dropout mask and its product
// in fp32 and keeps them for autograd.  Here one workgroup owns a 64-query tile of one (sample, head) and walks the key
// tiles up to the diagonal with a running (max, sum) per row (online softmax); only O and the per-row log-sum-exp
// leave the chip.  The backward recomputes P tile by tile from Q, K, the bias and the log-sum-exp (FlashAttention-2
// layout, no float atomics): one kernel per key tile owns dK and dV and walks the query tiles below it, one kernel per
// query tile owns dQ and this tile's per-diagonal sums of dS; the bias table's gradient is those partials summed in
// workgroup order, then by diagonal in ascending order (the bucket depends on i - j only).  Bitwise reproducible.
//
// Head widths up to 128: the fragments that stay fixed for a workgroup (Q and dO rows of a query tile; K and V rows of a
// key tile) live in registers, dh / 2 values per lane; the tiles that stream (K, V; Q, dO) pass through 64 x 64 LDS
// buffers in column chunks of 64, so the LDS plan (three 64 x 65 buffers) is that of the dh <= 64 HSTU kernels and a
// wider head costs a second pass over the chunk loop, not a larger footprint.  Columns past dh are zero in LDS.
//
// Dropout: the project's counter hash (common.h rh_drop_hash) over element ((b H + h) L + i) L + j of the call whose
// counter the forward reads from the device-resident (seed, counter) and then advances; the backward re-derives the mask
// from the saved counter.  p = 0 takes a path with no hash.
//
// The products run on the 64 x 64 MFMA tile of mfma_tile.h.
#include <math.h>

#include "mfma_tile.h"

namespace {

constexpr int kMaxDh = 128;
constexpr int kNC = kMaxDh / kT;  // column chunks of a head
constexpr int kMaxL = 1024;

struct SArgs {
  const float* q;        // (B, L, H, dh) views, row stride ld
  const float* k;
  const float* v;
  int64_t ld;
  const float* bias;     // (nb, H) or null
  const int64_t* rng;    // (seed, counter) or null (p_drop == 0)
  int64_t* saved_ctr;    // (1,) forward: written; backward: read
  float* out;            // (B, L, H dh)
  float* lse;            // (B, H, L)
  const float* g_out;    // (B, L, H dh)
  float* delta;          // (B, H, L) backward workspace: g_out . out per row
  float* g_q;            // (B, L, H, dh) views, row stride ldg
  float* g_k;
  float* g_v;
  int64_t ldg;
  float* part;           // (B H nqt + H, L) per-workgroup diagonal sums of dS, then their per-head totals
  float* g_bias;         // (nb, H)
  int B, L, H, dh, N, nb, fwd;
  float scale, p_drop;
};

__device__ __forceinline__ float bias_of(const SArgs& a, int i, int j, int h) {
  int d = i - j;
  d = d < a.N ? d : a.N;
  const int bucket = (int)((int64_t)d * (a.nb - 1) / a.N);
  return a.bias[(int64_t)bucket * a.H + h];
}

// the row's fragment for the A / B operand of a product over the head's columns: element s = column 2 s + kk
__device__ __forceinline__ void load_frag(float* f, const float* base, int64_t ld, int col, int row, int L, int d, int b,
                                          int kk) {
#pragma unroll
  for (int s = 0; s < kMaxDh / 2; ++s) {
    const int c = 2 * s + kk;
    f[s] = (row < L && c < d) ? base[((int64_t)b * L + row) * ld + col + c] : 0.f;
  }
}

struct DropKey {
  uint64_t seed, ctr;
  uint32_t thr;
  float keep;
};

__device__ __forceinline__ DropKey drop_key(const SArgs& a) {
  DropKey d{};
  d.keep = 1.f;
  if (a.p_drop > 0.f) {
    d.seed = (uint64_t)a.rng[0];
    d.ctr = a.fwd ? (uint64_t)a.rng[1] : (uint64_t)a.saved_ctr[0];
    d.thr = (uint32_t)(a.p_drop * 4294967296.0);
    d.keep = 1.f / (1.f - a.p_drop);
  }
  return d;
}

// 1 / (1 - p) for a kept weight, 0 for a dropped one
__device__ __forceinline__ float drop_mul(const SArgs& a, const DropKey& d, int bh, int i, int j) {
  if (a.p_drop <= 0.f) return 1.f;
  const uint64_t idx = ((uint64_t)bh * a.L + i) * a.L + j;
  return rh_drop_hash(d.seed, d.ctr, idx) >= d.thr ? d.keep : 0.f;
}

__global__ __launch_bounds__(RH_BLOCK) void softmax_attn_fwd_kernel(const SArgs a) {
  __shared__ float ks[kT * kLd], vs[kT * kLd], ps[kT * kLd];
  __shared__ float fac[kT];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int qt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int i0 = qt * kT, dh = a.dh, L = a.L, col = h * dh;
  const int nc = (dh + kT - 1) / kT, dh2 = (dh + 1) & ~1;
  const DropKey dk = drop_key(a);
  if (a.p_drop > 0.f && bh == 0 && qt == 0 && tid == 0) a.saved_ctr[0] = (int64_t)dk.ctr;
  float qf[kMaxDh / 2];
  load_frag(qf, a.q, a.ld, col, i0 + wm * 32 + li, L, dh, b, kk);
  v16f o[kNC];
#pragma unroll
  for (int c = 0; c < kNC; ++c) o[c] = zero16();
  // running (max, sum) of row tid / 4; its four lanes agree
  const int row = tid / 4, part = tid % 4;
  float rm = -INFINITY, rl = 0.f;
  for (int kt = 0; kt <= qt; ++kt) {
    const int j0 = kt * kT;
    v16f s = zero16();
#pragma unroll
    for (int c = 0; c < kNC; ++c) {
      if (c >= nc) continue;
      __syncthreads();
      load_tile(ks, a.k, a.ld, col, c * kT, j0, L, dh, b, tid);
      if (c == 0) load_tile(vs, a.v, a.ld, col, 0, j0, L, dh, b, tid);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kT; k += 2)
        if (c * kT + k < dh2)
          s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[c * (kT / 2) + k / 2], ks[(wn * 32 + li) * kLd + k + kk], s, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int il = wm * 32 + acc_row(r, kk), jl = wn * 32 + li;
      const int i = i0 + il, j = j0 + jl;
      float x = -INFINITY;
      if (i < L && j <= i) {
        x = s[r] * a.scale;
        if (a.bias) x += bias_of(a, i, j, h);
      }
      ps[il * kLd + jl] = x;
    }
    __syncthreads();
    {
      float m = -INFINITY;
      for (int q = 0; q < 16; ++q) m = fmaxf(m, ps[row * kLd + part * 16 + q]);
      m = fmaxf(m, __shfl_xor(m, 1, RH_WAVE));
      m = fmaxf(m, __shfl_xor(m, 2, RH_WAVE));
      const float nm = fmaxf(rm, m);
      float f = 1.f, sum = 0.f;
      if (nm > -INFINITY) {
        f = expf(rm - nm);  // 0 on the row's first tile (rm = -inf)
        for (int q = 0; q < 16; ++q) {
          const int jl = part * 16 + q;
          const float x = ps[row * kLd + jl];
          const float p = x > -INFINITY ? expf(x - nm) : 0.f;
          sum += p;
          ps[row * kLd + jl] = p > 0.f ? p * drop_mul(a, dk, bh, i0 + row, j0 + jl) : 0.f;
        }
        sum += __shfl_xor(sum, 1, RH_WAVE);
        sum += __shfl_xor(sum, 2, RH_WAVE);
      } else {
        for (int q = 0; q < 16; ++q) ps[row * kLd + part * 16 + q] = 0.f;
      }
      rl = rl * f + sum;
      rm = nm;
      if (part == 0) fac[row] = f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float f = fac[wm * 32 + acc_row(r, kk)];
#pragma unroll
      for (int c = 0; c < kNC; ++c) o[c][r] *= f;
    }
#pragma unroll
    for (int c = 0; c < kNC; ++c) {
      if (c >= nc) continue;
      if (c > 0) {
        __syncthreads();
        load_tile(vs, a.v, a.ld, col, c * kT, j0, L, dh, b, tid);
        __syncthreads();
      }
      // O quadrant: rows wm * 32, columns c * 64 + wn * 32;  O += P (64 x 64 keys) V (64 keys x 64 columns)
      if (c * kT + wn * 32 < dh) o[c] = mma_lds(o[c], ps + wm * 32 * kLd, kLd, 1, vs + wn * 32, kLd, 1, kT, li, kk);
    }
  }
  __syncthreads();
  if (part == 0) {
    fac[row] = rl > 0.f ? 1.f / rl : 0.f;
    if (i0 + row < L) a.lse[(int64_t)bh * L + i0 + row] = rm + logf(rl);
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kNC; ++c) {
    const int cc = c * kT + wn * 32 + li;
    if (cc >= dh) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int il = wm * 32 + acc_row(r, kk), i = i0 + il;
      if (i < L) a.out[((int64_t)b * L + i) * ((int64_t)a.H * dh) + col + cc] = o[c][r] * fac[il];
    }
  }
}

__global__ void drop_advance_kernel(int64_t* rng) { rng[1] += 1; }

// delta[b, h, i] = g_out[b, i, h, :] . out[b, i, h, :]
__global__ __launch_bounds__(RH_BLOCK) void softmax_attn_delta_kernel(const SArgs a) {
  const int64_t n = (int64_t)a.B * a.H * a.L;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    const int i = (int)(e % a.L);
    const int64_t bh = e / a.L;
    const int h = (int)(bh % a.H);
    const int64_t b = bh / a.H;
    const int64_t off = (b * a.L + i) * ((int64_t)a.H * a.dh) + (int64_t)h * a.dh;
    float s = 0.f;
    for (int c = 0; c < a.dh; ++c) s = fmaf(a.g_out[off + c], a.out[off + c], s);
    a.delta[e] = s;
  }
}

// dK, dV of one key tile: walks the query tiles at and below the diagonal.
__global__ __launch_bounds__(RH_BLOCK) void softmax_attn_dkv_kernel(const SArgs a) {
  __shared__ float qs[kT * kLd], gs[kT * kLd], xs[kT * kLd];
  __shared__ float lses[kT], dels[kT];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int kt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int j0 = kt * kT, dh = a.dh, L = a.L, col = h * dh;
  const int nc = (dh + kT - 1) / kT, dh2 = (dh + 1) & ~1;
  const int64_t ldo = (int64_t)a.H * dh;
  const int nqt = (L + kT - 1) / kT;
  const DropKey dk = drop_key(a);
  // K and V rows of the wavefront's key half as B fragments (B[k][j] = K[j][k]), in registers
  float kf[kMaxDh / 2], vf[kMaxDh / 2];
  load_frag(kf, a.k, a.ld, col, j0 + wn * 32 + li, L, dh, b, kk);
  load_frag(vf, a.v, a.ld, col, j0 + wn * 32 + li, L, dh, b, kk);
  v16f dkacc[kNC], dvacc[kNC];
#pragma unroll
  for (int c = 0; c < kNC; ++c) {
    dkacc[c] = zero16();
    dvacc[c] = zero16();
  }
  for (int qt = kt; qt < nqt; ++qt) {
    const int i0 = qt * kT;
    v16f s = zero16(), da = zero16();
#pragma unroll
    for (int c = 0; c < kNC; ++c) {
      if (c >= nc) continue;
      __syncthreads();
      load_tile(qs, a.q, a.ld, col, c * kT, i0, L, dh, b, tid);
      load_tile(gs, a.g_out, ldo, col, c * kT, i0, L, dh, b, tid);
      if (c == 0 && tid < kT) {
        const int i = i0 + tid;
        lses[tid] = i < L ? a.lse[(int64_t)bh * L + i] : 0.f;
        dels[tid] = i < L ? a.delta[(int64_t)bh * L + i] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kT; k += 2) {
        if (c * kT + k >= dh2) continue;
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(qs[(wm * 32 + li) * kLd + k + kk], kf[c * (kT / 2) + k / 2], s, 0, 0, 0);
        da = __builtin_amdgcn_mfma_f32_32x32x2f32(gs[(wm * 32 + li) * kLd + k + kk], vf[c * (kT / 2) + k / 2], da, 0, 0, 0);
      }
    }
    float pd[16], ds[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int il = wm * 32 + acc_row(r, kk), jl = wn * 32 + li;
      const int i = i0 + il, j = j0 + jl;
      pd[r] = 0.f;
      ds[r] = 0.f;
      if (i < L && j <= i) {
        float x = s[r] * a.scale;
        if (a.bias) x += bias_of(a, i, j, h);
        const float p = expf(x - lses[il]);
        const float m = drop_mul(a, dk, bh, i, j);
        pd[r] = p * m;
        ds[r] = p * (da[r] * m - dels[il]);
      }
    }
    // gs / qs hold the head's last chunk: walk the chunks downwards, reloading the earlier one
#pragma unroll
    for (int r = 0; r < 16; ++r) xs[(wm * 32 + acc_row(r, kk)) * kLd + wn * 32 + li] = pd[r];
#pragma unroll
    for (int cc = 0; cc < kNC; ++cc) {
      const int c = kNC - 1 - cc;
      if (c >= nc) continue;
      if (c != nc - 1) {
        __syncthreads();
        load_tile(gs, a.g_out, ldo, col, c * kT, i0, L, dh, b, tid);
      }
      __syncthreads();
      // dV quadrant: keys wm * 32, columns c * 64 + wn * 32;  dV += P^T dO  (A[key][i] = xs[i][key])
      if (c * kT + wn * 32 < dh) dvacc[c] = mma_lds(dvacc[c], xs + wm * 32, 1, kLd, gs + wn * 32, kLd, 1, kT, li, kk);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) xs[(wm * 32 + acc_row(r, kk)) * kLd + wn * 32 + li] = ds[r];
#pragma unroll
    for (int cc = 0; cc < kNC; ++cc) {
      const int c = kNC - 1 - cc;
      if (c >= nc) continue;
      if (c != nc - 1) {
        __syncthreads();
        load_tile(qs, a.q, a.ld, col, c * kT, i0, L, dh, b, tid);
      }
      __syncthreads();
      // dK quadrant: keys wm * 32, columns c * 64 + wn * 32;  dK += dS^T Q
      if (c * kT + wn * 32 < dh) dkacc[c] = mma_lds(dkacc[c], xs + wm * 32, 1, kLd, qs + wn * 32, kLd, 1, kT, li, kk);
    }
  }
#pragma unroll
  for (int c = 0; c < kNC; ++c) {
    const int cc = c * kT + wn * 32 + li;
    if (cc >= dh) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = j0 + wm * 32 + acc_row(r, kk);
      if (j >= L) continue;
      const int64_t off = ((int64_t)b * L + j) * a.ldg + col + cc;
      a.g_k[off] = dkacc[c][r] * a.scale;
      a.g_v[off] = dvacc[c][r];
    }
  }
}

// dQ of one query tile, and this tile's sums of dS by diagonal i - j (the bias bucket depends on it alone).
__global__ __launch_bounds__(RH_BLOCK) void softmax_attn_dq_kernel(const SArgs a) {
  __shared__ float ks[kT * kLd], vs[kT * kLd], xs[kT * kLd];
  __shared__ float pacc[kMaxL];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int qt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int i0 = qt * kT, dh = a.dh, L = a.L, col = h * dh;
  const int nc = (dh + kT - 1) / kT, dh2 = (dh + 1) & ~1;
  const int64_t ldo = (int64_t)a.H * dh;
  const DropKey dk = drop_key(a);
  // Q and dO rows of the wavefront's query half as A fragments, in registers
  float qf[kMaxDh / 2], gf[kMaxDh / 2];
  load_frag(qf, a.q, a.ld, col, i0 + wm * 32 + li, L, dh, b, kk);
  load_frag(gf, a.g_out, ldo, col, i0 + wm * 32 + li, L, dh, b, kk);
  float lser[16], delr[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = i0 + wm * 32 + acc_row(r, kk);
    lser[r] = i < L ? a.lse[(int64_t)bh * L + i] : 0.f;
    delr[r] = i < L ? a.delta[(int64_t)bh * L + i] : 0.f;
  }
  if (a.bias)
    for (int e = tid; e < L; e += RH_BLOCK) pacc[e] = 0.f;
  v16f dq[kNC];
#pragma unroll
  for (int c = 0; c < kNC; ++c) dq[c] = zero16();
  for (int kt = 0; kt <= qt; ++kt) {
    const int j0 = kt * kT;
    v16f s = zero16(), da = zero16();
#pragma unroll
    for (int c = 0; c < kNC; ++c) {
      if (c >= nc) continue;
      __syncthreads();
      load_tile(ks, a.k, a.ld, col, c * kT, j0, L, dh, b, tid);
      load_tile(vs, a.v, a.ld, col, c * kT, j0, L, dh, b, tid);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kT; k += 2) {
        if (c * kT + k >= dh2) continue;
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[c * (kT / 2) + k / 2], ks[(wn * 32 + li) * kLd + k + kk], s, 0, 0, 0);
        da = __builtin_amdgcn_mfma_f32_32x32x2f32(gf[c * (kT / 2) + k / 2], vs[(wn * 32 + li) * kLd + k + kk], da, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int il = wm * 32 + acc_row(r, kk), jl = wn * 32 + li;
      const int i = i0 + il, j = j0 + jl;
      float d = 0.f;
      if (i < L && j <= i) {
        float x = s[r] * a.scale;
        if (a.bias) x += bias_of(a, i, j, h);
        const float p = expf(x - lser[r]);
        d = p * (da[r] * drop_mul(a, dk, bh, i, j) - delr[r]);
      }
      xs[il * kLd + jl] = d;
    }
#pragma unroll
    for (int cc = 0; cc < kNC; ++cc) {
      const int c = kNC - 1 - cc;
      if (c >= nc) continue;
      if (c != nc - 1) {
        __syncthreads();
        load_tile(ks, a.k, a.ld, col, c * kT, j0, L, dh, b, tid);
      }
      __syncthreads();
      // dQ quadrant: queries wm * 32, columns c * 64 + wn * 32;  dQ += dS K
      if (c * kT + wn * 32 < dh) dq[c] = mma_lds(dq[c], xs + wm * 32 * kLd, kLd, 1, ks + wn * 32, kLd, 1, kT, li, kk);
    }
    // lane t < 127 owns the tile diagonal il - jl = t - 63, i.e. i - j = i0 - j0 + t - 63
    if (a.bias && tid < 2 * kT - 1) {
      const int e = tid - (kT - 1);
      const int d = i0 - j0 + e;
      if (d >= 0 && d < L) {
        float sum = 0.f;
        for (int il = e > 0 ? e : 0; il < kT && il - e < kT; ++il) sum += xs[il * kLd + il - e];
        pacc[d] += sum;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < kNC; ++c) {
    const int cc = c * kT + wn * 32 + li;
    if (cc >= dh) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + wm * 32 + acc_row(r, kk);
      if (i < L) a.g_q[((int64_t)b * L + i) * a.ldg + col + cc] = dq[c][r] * a.scale;
    }
  }
  if (a.bias) {
    __syncthreads();
    const int64_t p = (int64_t)bh * gridDim.y + qt;
    for (int e = tid; e < L; e += RH_BLOCK) a.part[p * L + e] = pacc[e];
  }
}

// per-head totals by diagonal: part[(B H nqt + h), d] = sum over (b, query tile) in that order
__global__ __launch_bounds__(RH_BLOCK) void softmax_attn_diag_kernel(const SArgs a, int nqt) {
  const int64_t n = (int64_t)a.H * a.L;
  float* tot = a.part + (int64_t)a.B * a.H * nqt * a.L;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    const int d = (int)(e % a.L), h = (int)(e / a.L);
    float sum = 0.f;
    for (int b = 0; b < a.B; ++b)
      for (int q = 0; q < nqt; ++q) sum += a.part[(((int64_t)b * a.H + h) * nqt + q) * a.L + d];
    tot[e] = sum;
  }
}

// g_bias[c, h] = sum over the diagonals of bucket c in ascending order
__global__ __launch_bounds__(RH_BLOCK) void softmax_attn_bias_kernel(const SArgs a, int nqt) {
  const int64_t n = (int64_t)a.nb * a.H;
  const float* tot = a.part + (int64_t)a.B * a.H * nqt * a.L;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    const int h = (int)(e % a.H), c = (int)(e / a.H);
    float sum = 0.f;
    for (int d = 0; d < a.L; ++d) {
      const int dd = d < a.N ? d : a.N;
      if ((int)((int64_t)dd * (a.nb - 1) / a.N) == c) sum += tot[(int64_t)h * a.L + d];
    }
    a.g_bias[e] = sum;
  }
}

int sattn_check(const char* name, const SArgs& a) {
  RH_REQUIRE(a.q && a.k && a.v, RH_E_BADARG, "%s: null pointer", name);
  RH_REQUIRE(a.B >= 0 && a.H >= 1 && a.N >= 1 && a.L >= 1 && a.L <= kMaxL && a.L <= a.N, RH_E_UNSUPPORTED,
             "%s: L=%d H=%d unsupported (1 <= L <= min(max_seq_len=%d, %d), H >= 1)", name, a.L, a.H, a.N, kMaxL);
  RH_REQUIRE(a.dh >= 1 && a.dh <= kMaxDh, RH_E_UNSUPPORTED, "%s: head width %d unsupported (1 <= dh <= %d)", name, a.dh,
             kMaxDh);
  RH_REQUIRE(!a.bias || a.nb >= 1, RH_E_UNSUPPORTED, "%s: num_buckets=%d unsupported (>= 1)", name, a.nb);
  RH_REQUIRE((int64_t)a.B * a.H <= 0x7FFFFFFF, RH_E_UNSUPPORTED, "%s: B * H = %lld exceeds the grid", name,
             (long long)a.B * a.H);
  RH_REQUIRE(a.ld >= (int64_t)a.H * a.dh, RH_E_BADARG, "%s: row stride %lld too small", name, (long long)a.ld);
  RH_REQUIRE(a.p_drop >= 0.f && a.p_drop < 1.f, RH_E_BADARG, "%s: dropout p=%g outside [0, 1)", name, (double)a.p_drop);
  RH_REQUIRE(a.p_drop == 0.f || (a.rng && a.saved_ctr), RH_E_BADARG, "%s: dropout without its (seed, counter) state", name);
  return 0;
}

SArgs sattn_args(const float* q, const float* k, const float* v, int64_t ld, int B, int L, int H, int dh, const float* bias,
                 int N, int nb, float scale, float p_drop, const int64_t* rng, const int64_t* saved_ctr, const float* out,
                 const float* lse) {
  SArgs a{};
  a.q = q;
  a.k = k;
  a.v = v;
  a.ld = ld;
  a.bias = bias;
  a.rng = rng;
  a.saved_ctr = const_cast<int64_t*>(saved_ctr);
  a.out = const_cast<float*>(out);
  a.lse = const_cast<float*>(lse);
  a.B = B;
  a.L = L;
  a.H = H;
  a.dh = dh;
  a.N = N;
  a.nb = nb;
  a.scale = scale;
  a.p_drop = p_drop;
  return a;
}

}  // namespace

extern "C" int rh_softmax_attn_nparts(int B, int L, int H) { return B * H * ((L + kT - 1) / kT) + H; }

extern "C" int rh_softmax_attn_fwd(const float* q, const float* k, const float* v, int64_t ld, int B, int L, int H, int dh,
                                   const float* bias, int N, int nb, float scale, float p_drop, int64_t* rng,
                                   int64_t* saved_ctr, float* out, float* lse, void* stream) {
  SArgs a = sattn_args(q, k, v, ld, B, L, H, dh, bias, N, nb, scale, p_drop, rng, saved_ctr, out, lse);
  a.fwd = 1;
  if (int rc = sattn_check("rh_softmax_attn_fwd", a)) return rc;
  RH_REQUIRE(out && lse, RH_E_BADARG, "rh_softmax_attn_fwd: null output");
  if (B == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nqt = (L + kT - 1) / kT;
  hipLaunchKernelGGL(softmax_attn_fwd_kernel, dim3(B * H, nqt), dim3(RH_BLOCK), 0, st, a);
  if (p_drop > 0.f) hipLaunchKernelGGL(drop_advance_kernel, dim3(1), dim3(1), 0, st, rng);
  RH_LAUNCH_CHECK("rh_softmax_attn_fwd");
  return 0;
}

extern "C" int rh_softmax_attn_bwd(const float* q, const float* k, const float* v, int64_t ld, int B, int L, int H, int dh,
                                   const float* bias, int N, int nb, float scale, float p_drop, const int64_t* rng,
                                   const int64_t* saved_ctr, const float* out, const float* lse, const float* g_out,
                                   float* delta, float* g_q, float* g_k, float* g_v, int64_t ldg, float* part,
                                   float* g_bias, void* stream) {
  SArgs a = sattn_args(q, k, v, ld, B, L, H, dh, bias, N, nb, scale, p_drop, rng, saved_ctr, out, lse);
  a.g_out = g_out;
  a.delta = delta;
  a.g_q = g_q;
  a.g_k = g_k;
  a.g_v = g_v;
  a.ldg = ldg;
  a.part = part;
  a.g_bias = g_bias;
  if (int rc = sattn_check("rh_softmax_attn_bwd", a)) return rc;
  RH_REQUIRE(out && lse && g_out && delta && g_q && g_k && g_v && (!bias || (part && g_bias)), RH_E_BADARG,
             "rh_softmax_attn_bwd: null pointer");
  RH_REQUIRE(ldg >= (int64_t)H * dh, RH_E_BADARG, "rh_softmax_attn_bwd: gradient row stride %lld too small", (long long)ldg);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nqt = (L + kT - 1) / kT;
  if (B > 0) {
    const int64_t n = (int64_t)B * H * L;
    int grid = (int)((n + RH_BLOCK - 1) / RH_BLOCK);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(softmax_attn_delta_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a);
    hipLaunchKernelGGL(softmax_attn_dkv_kernel, dim3(B * H, nqt), dim3(RH_BLOCK), 0, st, a);
    hipLaunchKernelGGL(softmax_attn_dq_kernel, dim3(B * H, nqt), dim3(RH_BLOCK), 0, st, a);
  }
  if (bias) {
    const int64_t n1 = (int64_t)H * L, n2 = (int64_t)nb * H;
    hipLaunchKernelGGL(softmax_attn_diag_kernel, dim3((int)((n1 + RH_BLOCK - 1) / RH_BLOCK)), dim3(RH_BLOCK), 0, st, a, nqt);
    hipLaunchKernelGGL(softmax_attn_bias_kernel, dim3((int)((n2 + RH_BLOCK - 1) / RH_BLOCK)), dim3(RH_BLOCK), 0, st, a, nqt);
  }
  RH_LAUNCH_CHECK("rh_softmax_attn_bwd");
  return 0;
}
