// TIGER's T5 stack: softmax multi-head attention in the three forms T5 uses, forward and backward, and the RMS norm with
// the residual add.
//
//   encoder self-attention  bidirectional, Lq = Lk, key-padding mask, bucketed relative-position bias
//   decoder self-attention  causal, Lq = Lk, one-sided buckets
//   cross attention         Lq != Lk (a handful of decoder positions against the encoded history), key-padding mask, no bias
//
// S[i, j] = q_i . k_j (no scale) + bias[bucket[(j - i) + (Lq - 1)], h]; an excluded (i, j) -- key masked out, or j > i
// when causal -- has S = -FLT_MAX, which is what the reference's additive finfo.min mask rounds to in fp32.  So a row with
// some key left gives the excluded ones weight exp(-FLT_MAX - max) = 0 exactly, and a row with no key left gives every
// key of the Lk weight 1 / Lk.  The forward marks such a row with lse = +inf, and the backward, which recomputes the
// weights from lse, reads the mark (-FLT_MAX + log Lk is not representable).  The gradient of such a row flows into
// q, k and the bias as autograd's does through the reference's additive mask.  The bucket table is the host's (T5's
// integer / float rule, ops.t5_relative_buckets): no logarithm is evaluated here.
//
// Two paths.  Lq > 8: hllm.hip's plan generalised -- one workgroup per 64-query tile of a (sample, head) walks the key
// tiles with an online softmax on the 64 x 64 MFMA tile of mfma_tile.h; the backward has one kernel per key tile (dK, dV)
// and one per query tile (dQ and the tile's sums of dS by diagonal j - i).  Lq <= 8 (TIGER's decoder: n_levels + 1
// tokens): a 64-row MFMA tile would be 7/8 padding or more (15/16 at four queries), so one WAVEFRONT owns a (sample, head), four to a workgroup; a lane
// owns a key of the current 64-key chunk and the dot products of its row with all (<= 8) queries, the chunk's weights pass
// through 2 KB of LDS per wavefront and lanes turn to the head's columns for P V (and dS K).  Same online softmax, same
// -FLT_MAX rule, same dropout element index, so the two paths agree wherever both could run.
//
// g_bias: per-workgroup (per-wavefront on the narrow path) sums of dS by diagonal, summed over (sample, query tile) in
// that order, then over the diagonals of a bucket in ascending order.  No atomics: bitwise reproducible.
#include <float.h>
#include <math.h>

#include "mfma_tile.h"

namespace {

constexpr int kMaxDh = 128;
constexpr int kNC = kMaxDh / kT;  // column chunks of a head
constexpr int kMaxL = 1024;
constexpr int kSmallQ = 8;        // queries a wavefront of the narrow path carries
constexpr int kWG = RH_BLOCK / RH_WAVE;

struct TArgs {
  const float* q;         // (B, Lq, H, dh) view, row stride ldq
  int64_t ldq;
  const float* k;         // (B, Lk, H, dh) views, row stride ldkv
  const float* v;
  int64_t ldkv;
  const uint8_t* mask;    // (B, Lk) or null
  const float* bias;      // (nb, H) or null
  const int32_t* bucket;  // (Lq + Lk - 1,)
  const int64_t* rng;     // (seed, counter) or null (p_drop == 0)
  int64_t* saved_ctr;     // (1,) forward: written; backward: read
  float* out;             // (B, Lq, H dh)
  float* lse;             // (B, H, Lq)
  const float* g_out;     // (B, Lq, H dh)
  float* delta;           // (B, H, Lq) backward workspace: g_out . out per row
  float* g_q;             // (B, Lq, H, dh) view, row stride ldgq
  int64_t ldgq;
  float* g_k;             // (B, Lk, H, dh) views, row stride ldgkv
  float* g_v;
  int64_t ldgkv;
  float* part;            // (B H nqt + H, nd) per-workgroup diagonal sums of dS, then their per-head totals
  float* g_bias;          // (nb, H)
  int B, Lq, Lk, H, dh, nb, causal, fwd, nd;
  float p_drop;
};

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

__device__ __forceinline__ DropKey drop_key(const TArgs& a) {
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
__device__ __forceinline__ float drop_mul(const TArgs& a, const DropKey& d, int64_t bh, int i, int j) {
  if (a.p_drop <= 0.f) return 1.f;
  const uint64_t idx = ((uint64_t)bh * a.Lq + i) * a.Lk + j;
  return rh_drop_hash(d.seed, d.ctr, idx) >= d.thr ? d.keep : 0.f;
}

__device__ __forceinline__ bool key_ok(const TArgs& a, int b, int j) {
  return j < a.Lk && (!a.mask || a.mask[(int64_t)b * a.Lk + j] != 0);
}

// the bias of the 127 diagonals jl - il = e - 63 of the tile pair (i0, j0)
__device__ __forceinline__ void load_diag_bias(float* bd, const TArgs& a, int i0, int j0, int h, int tid) {
  if (a.bias && tid < 2 * kT - 1) {
    const int d = (j0 - i0) + (tid - (kT - 1)) + (a.Lq - 1);
    bd[tid] = (d >= 0 && d < a.nd) ? a.bias[(int64_t)a.bucket[d] * a.H + h] : 0.f;
  }
}

// Key tiles that hold no valid key may be passed over when the row still has a valid key elsewhere: their weights are
// exp(-FLT_MAX - max) = 0 exactly, so the result is the same to the bit.  Not under the causal rule (a row's own valid set is
// then smaller than the sample's) and not for a sample with no valid key at all (every key then weighs 1 / Lk).
// tv[t] = key tile t has a valid key; returns whether empty tiles may be skipped.  All threads call it.
__device__ __forceinline__ bool scan_key_tiles(int* tv, const TArgs& a, int b, int tid) {
  if (!a.mask || a.causal) return false;
  if (tid < kMaxL / kT) tv[tid] = 0;
  __syncthreads();
  for (int j = tid; j < a.Lk; j += RH_BLOCK)
    if (a.mask[(int64_t)b * a.Lk + j] != 0) tv[j / kT] = 1;
  __syncthreads();
  int any = 0;
  for (int t = 0; t < (a.Lk + kT - 1) / kT; ++t) any |= tv[t];
  return any != 0;
}

// Causal WITHOUT a mask: every row keeps its own key, so the key tiles past the diagonal weigh 0 and are not visited.
// Causal WITH a mask, a row whose keys j <= i are all masked (a left-padded sample) has no key left and weighs ALL Lk
// keys 1 / Lk, those past the diagonal included: every key tile is visited then, as the narrow path does.
__device__ __forceinline__ bool stop_at_diagonal(const TArgs& a) { return a.causal && !a.mask; }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, RH_WAVE));
  return v;
}

// ------------------------------------------------------------------------------------------------------------------
// Lq > 8: the 64 x 64 MFMA tile
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RH_BLOCK, 2) void t5_attn_fwd_kernel(const TArgs a) {
  __shared__ float ks[kT * kLd], vs[kT * kLd], ps[kT * kLd];
  __shared__ float fac[kT], bd[2 * kT];
  __shared__ int tv[kMaxL / kT];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int qt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int i0 = qt * kT, dh = a.dh, Lq = a.Lq, Lk = a.Lk, col = h * dh;
  const int nc = (dh + kT - 1) / kT, dh2 = (dh + 1) & ~1;
  const int nkt = stop_at_diagonal(a) ? qt + 1 : (Lk + kT - 1) / kT;
  const DropKey dk = drop_key(a);
  if (a.p_drop > 0.f && bh == 0 && qt == 0 && tid == 0) a.saved_ctr[0] = (int64_t)dk.ctr;
  const bool skip = scan_key_tiles(tv, a, b, tid);
  float qf[kMaxDh / 2];
  load_frag(qf, a.q, a.ldq, col, i0 + wm * 32 + li, Lq, dh, b, kk);
  v16f o[kNC];
#pragma unroll
  for (int c = 0; c < kNC; ++c) o[c] = zero16();
  // running (max, sum) of row tid / 4; its four lanes agree
  const int row = tid / 4, part = tid % 4;
  float rm = -INFINITY, rl = 0.f;
  for (int kt = 0; kt < nkt; ++kt) {
    if (skip && !tv[kt]) continue;
    const int j0 = kt * kT;
    v16f s = zero16();
#pragma unroll
    for (int c = 0; c < kNC; ++c) {
      if (c >= nc) continue;
      __syncthreads();
      load_tile(ks, a.k, a.ldkv, col, c * kT, j0, Lk, dh, b, tid);
      if (c == 0) {
        load_tile(vs, a.v, a.ldkv, col, 0, j0, Lk, dh, b, tid);
        load_diag_bias(bd, a, i0, j0, h, tid);
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kT; k += 2)
        if (c * kT + k < dh2)
          s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[c * (kT / 2) + k / 2], ks[(wn * 32 + li) * kLd + k + kk], s, 0, 0, 0);
    }
    {
      const int jl = wn * 32 + li, j = j0 + jl;
      const bool kok = key_ok(a, b, j);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int il = wm * 32 + acc_row(r, kk), i = i0 + il;
        float x = -INFINITY;
        if (i < Lq && j < Lk) {
          x = -FLT_MAX;
          if (kok && (!a.causal || j <= i)) x = a.bias ? s[r] + bd[jl - il + kT - 1] : s[r];
        }
        ps[il * kLd + jl] = x;
      }
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
        f = expf(rm - nm);  // 0 on the row's first tile (rm = -inf), and when only excluded keys came before
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
        load_tile(vs, a.v, a.ldkv, col, c * kT, j0, Lk, dh, b, tid);
        __syncthreads();
      }
      if (c * kT + wn * 32 < dh) o[c] = mma_lds(o[c], ps + wm * 32 * kLd, kLd, 1, vs + wn * 32, kLd, 1, kT, li, kk);
    }
  }
  __syncthreads();
  if (part == 0) {
    fac[row] = rl > 0.f ? 1.f / rl : 0.f;
    if (i0 + row < Lq) a.lse[(int64_t)bh * Lq + i0 + row] = rm == -FLT_MAX ? INFINITY : rm + logf(rl);
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kNC; ++c) {
    const int cc = c * kT + wn * 32 + li;
    if (cc >= dh) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int il = wm * 32 + acc_row(r, kk), i = i0 + il;
      if (i < Lq) a.out[((int64_t)b * Lq + i) * ((int64_t)a.H * dh) + col + cc] = o[c][r] * fac[il];
    }
  }
}

__global__ void t5_drop_advance_kernel(int64_t* rng) { rng[1] += 1; }

// delta[b, h, i] = g_out[b, i, h, :] . out[b, i, h, :]
__global__ __launch_bounds__(RH_BLOCK) void t5_attn_delta_kernel(const TArgs a) {
  const int64_t n = (int64_t)a.B * a.H * a.Lq;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    const int i = (int)(e % a.Lq);
    const int64_t bh = e / a.Lq;
    const int h = (int)(bh % a.H);
    const int64_t b = bh / a.H;
    const int64_t off = (b * a.Lq + i) * ((int64_t)a.H * a.dh) + (int64_t)h * a.dh;
    float s = 0.f;
    for (int c = 0; c < a.dh; ++c) s = fmaf(a.g_out[off + c], a.out[off + c], s);
    a.delta[e] = s;
  }
}

// the weight of (i, j) recomputed from the row's lse, i < Lq and j < Lk
__device__ __forceinline__ float weight_of(const TArgs& a, float s, float bias, float lse, bool ok, float inv_lk) {
  if (lse == INFINITY) return inv_lk;  // no key left: uniform
  return ok ? expf(s + bias - lse) : 0.f;
}

// dK, dV of one key tile: walks the query tiles (from the diagonal down when causal).
__global__ __launch_bounds__(RH_BLOCK) void t5_attn_dkv_kernel(const TArgs a) {
  __shared__ float qs[kT * kLd], gs[kT * kLd], xs[kT * kLd];
  __shared__ float lses[kT], dels[kT], bd[2 * kT];
  __shared__ int tv[kMaxL / kT];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int kt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int j0 = kt * kT, dh = a.dh, Lq = a.Lq, Lk = a.Lk, col = h * dh;
  const int nc = (dh + kT - 1) / kT, dh2 = (dh + 1) & ~1;
  const int64_t ldo = (int64_t)a.H * dh;
  const int nqt = (Lq + kT - 1) / kT;
  const float inv_lk = 1.f / (float)Lk;
  const DropKey dk = drop_key(a);
  float kf[kMaxDh / 2], vf[kMaxDh / 2];
  load_frag(kf, a.k, a.ldkv, col, j0 + wn * 32 + li, Lk, dh, b, kk);
  load_frag(vf, a.v, a.ldkv, col, j0 + wn * 32 + li, Lk, dh, b, kk);
  const bool kok = key_ok(a, b, j0 + wn * 32 + li);
  v16f dkacc[kNC], dvacc[kNC];
#pragma unroll
  for (int c = 0; c < kNC; ++c) {
    dkacc[c] = zero16();
    dvacc[c] = zero16();
  }
  // a key tile without a valid key in a sample that has one elsewhere: dK = dV = 0, written below
  const bool dead = scan_key_tiles(tv, a, b, tid) && !tv[kt];
  for (int qt = stop_at_diagonal(a) ? kt : 0; qt < (dead ? 0 : nqt); ++qt) {
    const int i0 = qt * kT;
    v16f s = zero16(), da = zero16();
#pragma unroll
    for (int c = 0; c < kNC; ++c) {
      if (c >= nc) continue;
      __syncthreads();
      load_tile(qs, a.q, a.ldq, col, c * kT, i0, Lq, dh, b, tid);
      load_tile(gs, a.g_out, ldo, col, c * kT, i0, Lq, dh, b, tid);
      if (c == 0) {
        if (tid < kT) {
          const int i = i0 + tid;
          lses[tid] = i < Lq ? a.lse[(int64_t)bh * Lq + i] : 0.f;
          dels[tid] = i < Lq ? a.delta[(int64_t)bh * Lq + i] : 0.f;
        }
        load_diag_bias(bd, a, i0, j0, h, tid);
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
      if (i < Lq && j < Lk) {
        const float p = weight_of(a, s[r], a.bias ? bd[jl - il + kT - 1] : 0.f, lses[il], kok && (!a.causal || j <= i), inv_lk);
        if (p > 0.f) {
          const float m = drop_mul(a, dk, bh, i, j);
          pd[r] = p * m;
          ds[r] = p * (da[r] * m - dels[il]);
        }
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
        load_tile(gs, a.g_out, ldo, col, c * kT, i0, Lq, dh, b, tid);
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
        load_tile(qs, a.q, a.ldq, col, c * kT, i0, Lq, dh, b, tid);
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
      if (j >= Lk) continue;
      const int64_t off = ((int64_t)b * Lk + j) * a.ldgkv + col + cc;
      a.g_k[off] = dkacc[c][r];
      a.g_v[off] = dvacc[c][r];
    }
  }
}

// dQ of one query tile, and this tile's sums of dS by diagonal (j - i) + (Lq - 1) (the bias bucket depends on it alone).
__global__ __launch_bounds__(RH_BLOCK) void t5_attn_dq_kernel(const TArgs a) {
  __shared__ float ks[kT * kLd], vs[kT * kLd], xs[kT * kLd];
  __shared__ float pacc[2 * kMaxL], bd[2 * kT];
  __shared__ int tv[kMaxL / kT];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int qt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int i0 = qt * kT, dh = a.dh, Lq = a.Lq, Lk = a.Lk, col = h * dh, nd = a.nd;
  const int nc = (dh + kT - 1) / kT, dh2 = (dh + 1) & ~1;
  const int64_t ldo = (int64_t)a.H * dh;
  const int nkt = stop_at_diagonal(a) ? qt + 1 : (Lk + kT - 1) / kT;
  const float inv_lk = 1.f / (float)Lk;
  const DropKey dk = drop_key(a);
  float qf[kMaxDh / 2], gf[kMaxDh / 2];
  load_frag(qf, a.q, a.ldq, col, i0 + wm * 32 + li, Lq, dh, b, kk);
  load_frag(gf, a.g_out, ldo, col, i0 + wm * 32 + li, Lq, dh, b, kk);
  float lser[16], delr[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = i0 + wm * 32 + acc_row(r, kk);
    lser[r] = i < Lq ? a.lse[(int64_t)bh * Lq + i] : 0.f;
    delr[r] = i < Lq ? a.delta[(int64_t)bh * Lq + i] : 0.f;
  }
  if (a.bias)
    for (int e = tid; e < nd; e += RH_BLOCK) pacc[e] = 0.f;
  v16f dq[kNC];
#pragma unroll
  for (int c = 0; c < kNC; ++c) dq[c] = zero16();
  const bool skip = scan_key_tiles(tv, a, b, tid);
  for (int kt = 0; kt < nkt; ++kt) {
    if (skip && !tv[kt]) continue;
    const int j0 = kt * kT;
    v16f s = zero16(), da = zero16();
#pragma unroll
    for (int c = 0; c < kNC; ++c) {
      if (c >= nc) continue;
      __syncthreads();
      load_tile(ks, a.k, a.ldkv, col, c * kT, j0, Lk, dh, b, tid);
      load_tile(vs, a.v, a.ldkv, col, c * kT, j0, Lk, dh, b, tid);
      if (c == 0) load_diag_bias(bd, a, i0, j0, h, tid);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kT; k += 2) {
        if (c * kT + k >= dh2) continue;
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[c * (kT / 2) + k / 2], ks[(wn * 32 + li) * kLd + k + kk], s, 0, 0, 0);
        da = __builtin_amdgcn_mfma_f32_32x32x2f32(gf[c * (kT / 2) + k / 2], vs[(wn * 32 + li) * kLd + k + kk], da, 0, 0, 0);
      }
    }
    {
      const int jl = wn * 32 + li, j = j0 + jl;
      const bool kok = key_ok(a, b, j);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int il = wm * 32 + acc_row(r, kk), i = i0 + il;
        float d = 0.f;
        if (i < Lq && j < Lk) {
          const float p = weight_of(a, s[r], a.bias ? bd[jl - il + kT - 1] : 0.f, lser[r], kok && (!a.causal || j <= i), inv_lk);
          if (p > 0.f) d = p * (da[r] * drop_mul(a, dk, bh, i, j) - delr[r]);
        }
        xs[il * kLd + jl] = d;
      }
    }
#pragma unroll
    for (int cc = 0; cc < kNC; ++cc) {
      const int c = kNC - 1 - cc;
      if (c >= nc) continue;
      if (c != nc - 1) {
        __syncthreads();
        load_tile(ks, a.k, a.ldkv, col, c * kT, j0, Lk, dh, b, tid);
      }
      __syncthreads();
      // dQ quadrant: queries wm * 32, columns c * 64 + wn * 32;  dQ += dS K
      if (c * kT + wn * 32 < dh) dq[c] = mma_lds(dq[c], xs + wm * 32 * kLd, kLd, 1, ks + wn * 32, kLd, 1, kT, li, kk);
    }
    // thread t < 127 owns the tile diagonal jl - il = t - 63, i.e. index (j0 - i0) + t - 63 + (Lq - 1)
    if (a.bias && tid < 2 * kT - 1) {
      const int e = tid - (kT - 1);
      const int d = (j0 - i0) + e + (Lq - 1);
      if (d >= 0 && d < nd) {
        float sum = 0.f;
        for (int il = e < 0 ? -e : 0; il < kT && il + e < kT; ++il) sum += xs[il * kLd + il + e];
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
      if (i < Lq) a.g_q[((int64_t)b * Lq + i) * a.ldgq + col + cc] = dq[c][r];
    }
  }
  if (a.bias) {
    __syncthreads();
    const int64_t p = (int64_t)bh * gridDim.y + qt;
    for (int e = tid; e < nd; e += RH_BLOCK) a.part[p * nd + e] = pacc[e];
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Lq <= 8: one wavefront per (sample, head), a lane per key of the 64-key chunk
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RH_BLOCK) void t5_attn_small_fwd_kernel(const TArgs a) {
  __shared__ float qs_[kWG][kSmallQ * kMaxDh];
  __shared__ float pc_[kWG][kSmallQ * RH_WAVE];
  const int lane = threadIdx.x % RH_WAVE, w = threadIdx.x / RH_WAVE;
  float* qs = qs_[w];
  float* pc = pc_[w];
  const int64_t nbh = (int64_t)a.B * a.H;
  int64_t bh = (int64_t)blockIdx.x * kWG + w;
  const bool live = bh < nbh;  // a wavefront past the end computes the last pair again and stores nothing
  if (!live) bh = nbh - 1;
  const int b = (int)(bh / a.H), h = (int)(bh % a.H);
  const int dh = a.dh, Lq = a.Lq, Lk = a.Lk, col = h * dh;
  const DropKey dk = drop_key(a);
  if (a.p_drop > 0.f && blockIdx.x == 0 && threadIdx.x == 0) a.saved_ctr[0] = (int64_t)dk.ctr;
  for (int e = lane; e < kSmallQ * dh; e += RH_WAVE) {
    const int i = e / dh, c = e % dh;
    qs[i * kMaxDh + c] = i < Lq ? a.q[((int64_t)b * Lq + i) * a.ldq + col + c] : 0.f;
  }
  __syncthreads();
  float rm[kSmallQ], rl[kSmallQ], o[kSmallQ][kNC];
#pragma unroll
  for (int i = 0; i < kSmallQ; ++i) {
    rm[i] = -INFINITY;
    rl[i] = 0.f;
#pragma unroll
    for (int c = 0; c < kNC; ++c) o[i][c] = 0.f;
  }
  for (int j0 = 0; j0 < Lk; j0 += RH_WAVE) {
    const int j = j0 + lane;
    const bool inb = j < Lk;
    float s[kSmallQ];
#pragma unroll
    for (int i = 0; i < kSmallQ; ++i) s[i] = 0.f;
    if (inb) {
      const float* kr = a.k + ((int64_t)b * Lk + j) * a.ldkv + col;
      for (int c = 0; c < dh; ++c) {
        const float kv = kr[c];
#pragma unroll
        for (int i = 0; i < kSmallQ; ++i) s[i] = fmaf(qs[i * kMaxDh + c], kv, s[i]);
      }
    }
    const bool kok = key_ok(a, b, j);
#pragma unroll
    for (int i = 0; i < kSmallQ; ++i) {
      float p = 0.f;
      if (i < Lq) {  // uniform
        float x = -INFINITY;
        if (inb) {
          x = -FLT_MAX;
          if (kok && (!a.causal || j <= i))
            x = a.bias ? s[i] + a.bias[(int64_t)a.bucket[j - i + Lq - 1] * a.H + h] : s[i];
        }
        const float nm = fmaxf(rm[i], wave_max(x));  // finite: every chunk has a key j < Lk
        const float f = expf(rm[i] - nm);
        p = x > -INFINITY ? expf(x - nm) : 0.f;
        rl[i] = rl[i] * f + wave_sum(p);
        rm[i] = nm;
#pragma unroll
        for (int c = 0; c < kNC; ++c) o[i][c] *= f;
        if (p > 0.f) p *= drop_mul(a, dk, bh, i, j);
      }
      pc[i * RH_WAVE + lane] = p;
    }
    __syncthreads();
    const int nj = Lk - j0 < RH_WAVE ? Lk - j0 : RH_WAVE;
    for (int jl = 0; jl < nj; ++jl) {
      const float* vr = a.v + ((int64_t)b * Lk + j0 + jl) * a.ldkv + col;
#pragma unroll
      for (int c = 0; c < kNC; ++c) {
        const int cc = c * RH_WAVE + lane;
        if (cc < dh) {
          const float vv = vr[cc];
#pragma unroll
          for (int i = 0; i < kSmallQ; ++i) o[i][c] = fmaf(pc[i * RH_WAVE + jl], vv, o[i][c]);
        }
      }
    }
    __syncthreads();
  }
  if (!live) return;
#pragma unroll
  for (int i = 0; i < kSmallQ; ++i) {
    if (i >= Lq) continue;
    const float inv = 1.f / rl[i];
#pragma unroll
    for (int c = 0; c < kNC; ++c) {
      const int cc = c * RH_WAVE + lane;
      if (cc < dh) a.out[((int64_t)b * Lq + i) * ((int64_t)a.H * dh) + col + cc] = o[i][c] * inv;
    }
    if (lane == 0) a.lse[bh * Lq + i] = rm[i] == -FLT_MAX ? INFINITY : rm[i] + logf(rl[i]);
  }
}

__global__ __launch_bounds__(RH_BLOCK) void t5_attn_small_bwd_kernel(const TArgs a) {
  __shared__ float qs_[kWG][kSmallQ * kMaxDh];
  __shared__ float gs_[kWG][kSmallQ * kMaxDh];
  __shared__ float dc_[kWG][kSmallQ * RH_WAVE];
  const int lane = threadIdx.x % RH_WAVE, w = threadIdx.x / RH_WAVE;
  float* qs = qs_[w];
  float* gs = gs_[w];
  float* dc = dc_[w];
  const int64_t nbh = (int64_t)a.B * a.H;
  int64_t bh = (int64_t)blockIdx.x * kWG + w;
  const bool live = bh < nbh;
  if (!live) bh = nbh - 1;
  const int b = (int)(bh / a.H), h = (int)(bh % a.H);
  const int dh = a.dh, Lq = a.Lq, Lk = a.Lk, col = h * dh, nd = a.nd;
  const int64_t ldo = (int64_t)a.H * dh;
  const float inv_lk = 1.f / (float)Lk;
  const DropKey dk = drop_key(a);
  for (int e = lane; e < kSmallQ * dh; e += RH_WAVE) {
    const int i = e / dh, c = e % dh;
    qs[i * kMaxDh + c] = i < Lq ? a.q[((int64_t)b * Lq + i) * a.ldq + col + c] : 0.f;
    gs[i * kMaxDh + c] = i < Lq ? a.g_out[((int64_t)b * Lq + i) * ldo + col + c] : 0.f;
  }
  float lser[kSmallQ], delr[kSmallQ], dq[kSmallQ][kNC];
#pragma unroll
  for (int i = 0; i < kSmallQ; ++i) {
    lser[i] = i < Lq ? a.lse[bh * Lq + i] : 0.f;
    delr[i] = i < Lq ? a.delta[bh * Lq + i] : 0.f;
#pragma unroll
    for (int c = 0; c < kNC; ++c) dq[i][c] = 0.f;
  }
  __syncthreads();
  float carry = 0.f;  // lane t < Lq - 1: the part of diagonal j0 + 64 + t that the chunk before j0 + 64 holds
  int j0 = 0;
  for (; j0 < Lk; j0 += RH_WAVE) {
    const int j = j0 + lane;
    const bool inb = j < Lk;
    float s[kSmallQ], da[kSmallQ];
#pragma unroll
    for (int i = 0; i < kSmallQ; ++i) {
      s[i] = 0.f;
      da[i] = 0.f;
    }
    if (inb) {
      const float* kr = a.k + ((int64_t)b * Lk + j) * a.ldkv + col;
      const float* vr = a.v + ((int64_t)b * Lk + j) * a.ldkv + col;
      for (int c = 0; c < dh; ++c) {
        const float kv = kr[c], vv = vr[c];
#pragma unroll
        for (int i = 0; i < kSmallQ; ++i) {
          s[i] = fmaf(qs[i * kMaxDh + c], kv, s[i]);
          da[i] = fmaf(gs[i * kMaxDh + c], vv, da[i]);
        }
      }
    }
    const bool kok = key_ok(a, b, j);
    float pd[kSmallQ], ds[kSmallQ];
#pragma unroll
    for (int i = 0; i < kSmallQ; ++i) {
      pd[i] = 0.f;
      ds[i] = 0.f;
      if (i < Lq && inb) {
        const bool ok = kok && (!a.causal || j <= i);
        const float bv = (a.bias && ok) ? a.bias[(int64_t)a.bucket[j - i + Lq - 1] * a.H + h] : 0.f;
        const float p = weight_of(a, s[i], bv, lser[i], ok, inv_lk);
        if (p > 0.f) {
          const float m = drop_mul(a, dk, bh, i, j);
          pd[i] = p * m;
          ds[i] = p * (da[i] * m - delr[i]);
        }
      }
      dc[i * RH_WAVE + lane] = ds[i];
    }
    if (inb && live) {
      float* gk = a.g_k + ((int64_t)b * Lk + j) * a.ldgkv + col;
      float* gv = a.g_v + ((int64_t)b * Lk + j) * a.ldgkv + col;
      for (int c = 0; c < dh; ++c) {
        float dkc = 0.f, dvc = 0.f;
#pragma unroll
        for (int i = 0; i < kSmallQ; ++i) {
          dkc = fmaf(ds[i], qs[i * kMaxDh + c], dkc);
          dvc = fmaf(pd[i], gs[i * kMaxDh + c], dvc);
        }
        gk[c] = dkc;
        gv[c] = dvc;
      }
    }
    __syncthreads();
    const int nj = Lk - j0 < RH_WAVE ? Lk - j0 : RH_WAVE;
    for (int jl = 0; jl < nj; ++jl) {
      const float* kr = a.k + ((int64_t)b * Lk + j0 + jl) * a.ldkv + col;
#pragma unroll
      for (int c = 0; c < kNC; ++c) {
        const int cc = c * RH_WAVE + lane;
        if (cc < dh) {
          const float kv = kr[cc];
#pragma unroll
          for (int i = 0; i < kSmallQ; ++i) dq[i][c] = fmaf(dc[i * RH_WAVE + jl], kv, dq[i][c]);
        }
      }
    }
    if (a.bias) {
      // diagonal index d = (j - i) + (Lq - 1); lane t finishes d = j0 + t: this chunk's keys jl = t + i - (Lq - 1) plus
      // the carry from the chunk before
      float t = carry, nxt = 0.f;
      for (int i = 0; i < Lq; ++i) {
        const int jl = lane + i - (Lq - 1);
        if (jl >= 0) t += dc[i * RH_WAVE + jl];
        const int jn = jl + RH_WAVE;
        if (jn < RH_WAVE) nxt += dc[i * RH_WAVE + jn];
      }
      const int d = j0 + lane;
      if (live && d < nd) a.part[bh * nd + d] = t;
      carry = nxt;
    }
    __syncthreads();
  }
  if (!live) return;
  if (a.bias && lane < Lq - 1 && j0 + lane < nd) a.part[bh * nd + j0 + lane] = carry;
#pragma unroll
  for (int i = 0; i < kSmallQ; ++i) {
    if (i >= Lq) continue;
#pragma unroll
    for (int c = 0; c < kNC; ++c) {
      const int cc = c * RH_WAVE + lane;
      if (cc < dh) a.g_q[((int64_t)b * Lq + i) * a.ldgq + col + cc] = dq[i][c];
    }
  }
}

// per-head totals by diagonal: part[(B H nqt + h), d] = sum over (b, query tile) in that order
__global__ __launch_bounds__(RH_BLOCK) void t5_attn_diag_kernel(const TArgs a, int nqt) {
  const int64_t n = (int64_t)a.H * a.nd;
  float* tot = a.part + (int64_t)a.B * a.H * nqt * a.nd;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    const int d = (int)(e % a.nd), h = (int)(e / a.nd);
    float sum = 0.f;
    for (int b = 0; b < a.B; ++b)
      for (int q = 0; q < nqt; ++q) sum += a.part[(((int64_t)b * a.H + h) * nqt + q) * a.nd + d];
    tot[e] = sum;
  }
}

// g_bias[c, h] = sum over the diagonals of bucket c in ascending order
__global__ __launch_bounds__(RH_BLOCK) void t5_attn_bias_kernel(const TArgs a, int nqt) {
  const int64_t n = (int64_t)a.nb * a.H;
  const float* tot = a.part + (int64_t)a.B * a.H * nqt * a.nd;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    const int h = (int)(e % a.H), c = (int)(e / a.H);
    float sum = 0.f;
    for (int d = 0; d < a.nd; ++d)
      if (a.bucket[d] == c) sum += tot[(int64_t)h * a.nd + d];
    a.g_bias[e] = sum;
  }
}

int t5_nqt(int Lq) { return Lq <= kSmallQ ? 1 : (Lq + kT - 1) / kT; }

int t5_check(const char* name, const TArgs& a) {
  RH_REQUIRE(a.q && a.k && a.v, RH_E_BADARG, "%s: null pointer", name);
  RH_REQUIRE(a.B >= 0 && a.H >= 1 && a.Lq >= 1 && a.Lq <= kMaxL && a.Lk >= 1 && a.Lk <= kMaxL, RH_E_UNSUPPORTED,
             "%s: Lq=%d Lk=%d H=%d unsupported (1 <= Lq, Lk <= %d, H >= 1)", name, a.Lq, a.Lk, a.H, kMaxL);
  RH_REQUIRE(!a.causal || a.Lq == a.Lk, RH_E_UNSUPPORTED, "%s: causal attention needs Lq == Lk (got %d, %d)", name, a.Lq,
             a.Lk);
  RH_REQUIRE(a.dh >= 1 && a.dh <= kMaxDh, RH_E_UNSUPPORTED, "%s: head width %d unsupported (1 <= dh <= %d)", name, a.dh,
             kMaxDh);
  RH_REQUIRE(!a.bias || a.nb >= 1, RH_E_UNSUPPORTED, "%s: num_buckets=%d unsupported (>= 1)", name, a.nb);
  RH_REQUIRE(!a.bias || a.bucket, RH_E_BADARG, "%s: a bias table without its bucket table", name);
  RH_REQUIRE((int64_t)a.B * a.H <= 0x7FFFFFFF, RH_E_UNSUPPORTED, "%s: B * H = %lld exceeds the grid", name,
             (long long)a.B * a.H);
  RH_REQUIRE(a.ldq >= (int64_t)a.H * a.dh && a.ldkv >= (int64_t)a.H * a.dh, RH_E_BADARG, "%s: row stride %lld / %lld too small",
             name, (long long)a.ldq, (long long)a.ldkv);
  RH_REQUIRE(a.p_drop >= 0.f && a.p_drop < 1.f, RH_E_BADARG, "%s: dropout p=%g outside [0, 1)", name, (double)a.p_drop);
  RH_REQUIRE(a.p_drop == 0.f || (a.rng && a.saved_ctr), RH_E_BADARG, "%s: dropout without its (seed, counter) state", name);
  return 0;
}

TArgs t5_args(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, int B, int Lq, int Lk, int H, int dh,
              const uint8_t* mask, int causal, const float* bias, const int32_t* bucket, int nb, float p_drop,
              const int64_t* rng, const int64_t* saved_ctr, const float* out, const float* lse) {
  TArgs a{};
  a.q = q;
  a.ldq = ldq;
  a.k = k;
  a.v = v;
  a.ldkv = ldkv;
  a.mask = mask;
  a.bias = bias;
  a.bucket = bucket;
  a.rng = rng;
  a.saved_ctr = const_cast<int64_t*>(saved_ctr);
  a.out = const_cast<float*>(out);
  a.lse = const_cast<float*>(lse);
  a.B = B;
  a.Lq = Lq;
  a.Lk = Lk;
  a.H = H;
  a.dh = dh;
  a.nb = nb;
  a.causal = causal ? 1 : 0;
  a.nd = Lq + Lk - 1;
  a.p_drop = p_drop;
  return a;
}

// ------------------------------------------------------------------------------------------------------------------
// RMS norm with the residual add: one wavefront per row, the row's D <= 1024 values in 16 registers per lane
// ------------------------------------------------------------------------------------------------------------------
constexpr int kRmsMaxD = 1024;
constexpr int kRmsPer = kRmsMaxD / RH_WAVE;
constexpr int kRmsGrid = 512;  // workgroups of a launch at most; each walks rows blockIdx.x * 4 + wave, + 4 * grid, ...

__global__ __launch_bounds__(RH_BLOCK) void add_rms_norm_fwd_kernel(const float* h, const float* delta, const float* w,
                                                                     float eps, int M, int D, float* hn, float* y,
                                                                     float* rstd) {
  const int lane = threadIdx.x % RH_WAVE, wv = threadIdx.x / RH_WAVE;
  for (int64_t row = (int64_t)blockIdx.x * kWG + wv; row < M; row += (int64_t)gridDim.x * kWG) {
    float x[kRmsPer];
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < kRmsPer; ++t) {
      const int c = t * RH_WAVE + lane;
      x[t] = 0.f;
      if (c < D) {
        x[t] = h[row * D + c];
        if (delta) x[t] += delta[row * D + c];
      }
      ss = fmaf(x[t], x[t], ss);
    }
    ss = wave_sum(ss);
    const float r = rsqrtf(ss / (float)D + eps);
#pragma unroll
    for (int t = 0; t < kRmsPer; ++t) {
      const int c = t * RH_WAVE + lane;
      if (c < D) {
        if (hn) hn[row * D + c] = x[t];
        y[row * D + c] = x[t] * r * w[c];
      }
    }
    if (lane == 0) rstd[row] = r;
  }
}

__global__ __launch_bounds__(RH_BLOCK) void add_rms_norm_bwd_kernel(const float* hn, const float* w, const float* rstd,
                                                                     const float* g_y, const float* g_res, int M, int D,
                                                                     float* g_h, float* part) {
  __shared__ float red[kWG][kRmsMaxD];
  const int lane = threadIdx.x % RH_WAVE, wv = threadIdx.x / RH_WAVE;
  float gw[kRmsPer];
#pragma unroll
  for (int t = 0; t < kRmsPer; ++t) gw[t] = 0.f;
  for (int64_t row = (int64_t)blockIdx.x * kWG + wv; row < M; row += (int64_t)gridDim.x * kWG) {
    const float r = rstd[row];
    float x[kRmsPer], g[kRmsPer];
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < kRmsPer; ++t) {
      const int c = t * RH_WAVE + lane;
      x[t] = 0.f;
      g[t] = 0.f;
      if (c < D) {
        x[t] = hn[row * D + c];
        const float gy = g_y[row * D + c];
        g[t] = gy * w[c];
        gw[t] = fmaf(gy, x[t] * r, gw[t]);
      }
      dot = fmaf(g[t], x[t], dot);
    }
    dot = wave_sum(dot);
    const float coef = dot * r * r * r / (float)D;
#pragma unroll
    for (int t = 0; t < kRmsPer; ++t) {
      const int c = t * RH_WAVE + lane;
      if (c < D) {
        float v = r * g[t] - x[t] * coef;
        if (g_res) v += g_res[row * D + c];
        g_h[row * D + c] = v;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < kRmsPer; ++t) red[wv][t * RH_WAVE + lane] = gw[t];
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += RH_BLOCK) part[(int64_t)blockIdx.x * D + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

int rms_grid(int M) {
  const int g = (M + kWG - 1) / kWG;
  return g < 1 ? 1 : (g > kRmsGrid ? kRmsGrid : g);
}

}  // namespace

extern "C" int rh_t5_attn_nparts(int B, int Lq, int H, int* nparts) {
  RH_REQUIRE(nparts, RH_E_BADARG, "rh_t5_attn_nparts: null pointer");
  RH_REQUIRE(B >= 0 && H >= 1 && Lq >= 1 && Lq <= kMaxL && (int64_t)B * H * t5_nqt(Lq) + H <= 0x7FFFFFFF, RH_E_UNSUPPORTED,
             "rh_t5_attn_nparts: B=%d Lq=%d H=%d unsupported", B, Lq, H);
  *nparts = B * H * t5_nqt(Lq) + H;
  return 0;
}

extern "C" int rh_t5_attn_fwd(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, int B, int Lq, int Lk,
                              int H, int dh, const uint8_t* key_mask, int causal, const float* bias, const int32_t* bucket,
                              int nb, float p_drop, int64_t* rng, int64_t* saved_ctr, float* out, float* lse, void* stream) {
  TArgs a = t5_args(q, ldq, k, v, ldkv, B, Lq, Lk, H, dh, key_mask, causal, bias, bucket, nb, p_drop, rng, saved_ctr, out, lse);
  a.fwd = 1;
  if (int rc = t5_check("rh_t5_attn_fwd", a)) return rc;
  RH_REQUIRE(out && lse, RH_E_BADARG, "rh_t5_attn_fwd: null output");
  if (B == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (Lq <= kSmallQ) {
    const int grid = (int)(((int64_t)B * H + kWG - 1) / kWG);
    hipLaunchKernelGGL(t5_attn_small_fwd_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a);
  } else {
    hipLaunchKernelGGL(t5_attn_fwd_kernel, dim3(B * H, t5_nqt(Lq)), dim3(RH_BLOCK), 0, st, a);
  }
  if (p_drop > 0.f) hipLaunchKernelGGL(t5_drop_advance_kernel, dim3(1), dim3(1), 0, st, rng);
  RH_LAUNCH_CHECK("rh_t5_attn_fwd");
  return 0;
}

extern "C" int rh_t5_attn_bwd(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, int B, int Lq, int Lk,
                              int H, int dh, const uint8_t* key_mask, int causal, const float* bias, const int32_t* bucket,
                              int nb, float p_drop, const int64_t* rng, const int64_t* saved_ctr, const float* out,
                              const float* lse, const float* g_out, float* delta, float* g_q, int64_t ldgq, float* g_k,
                              float* g_v, int64_t ldgkv, float* part, float* g_bias, void* stream) {
  TArgs a = t5_args(q, ldq, k, v, ldkv, B, Lq, Lk, H, dh, key_mask, causal, bias, bucket, nb, p_drop, rng, saved_ctr, out, lse);
  a.g_out = g_out;
  a.delta = delta;
  a.g_q = g_q;
  a.ldgq = ldgq;
  a.g_k = g_k;
  a.g_v = g_v;
  a.ldgkv = ldgkv;
  a.part = part;
  a.g_bias = g_bias;
  if (int rc = t5_check("rh_t5_attn_bwd", a)) return rc;
  RH_REQUIRE(out && lse && g_out && delta && g_q && g_k && g_v && (!bias || (part && g_bias)), RH_E_BADARG,
             "rh_t5_attn_bwd: null pointer");
  RH_REQUIRE(ldgq >= (int64_t)H * dh && ldgkv >= (int64_t)H * dh, RH_E_BADARG,
             "rh_t5_attn_bwd: gradient row stride %lld / %lld too small", (long long)ldgq, (long long)ldgkv);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nqt = t5_nqt(Lq);
  if (B > 0) {
    const int64_t n = (int64_t)B * H * Lq;
    int grid = (int)((n + RH_BLOCK - 1) / RH_BLOCK);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(t5_attn_delta_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a);
    if (Lq <= kSmallQ) {
      const int g2 = (int)(((int64_t)B * H + kWG - 1) / kWG);
      hipLaunchKernelGGL(t5_attn_small_bwd_kernel, dim3(g2), dim3(RH_BLOCK), 0, st, a);
    } else {
      hipLaunchKernelGGL(t5_attn_dkv_kernel, dim3(B * H, (Lk + kT - 1) / kT), dim3(RH_BLOCK), 0, st, a);
      hipLaunchKernelGGL(t5_attn_dq_kernel, dim3(B * H, nqt), dim3(RH_BLOCK), 0, st, a);
    }
  }
  if (bias) {
    const int64_t n1 = (int64_t)H * a.nd, n2 = (int64_t)nb * H;
    hipLaunchKernelGGL(t5_attn_diag_kernel, dim3((int)((n1 + RH_BLOCK - 1) / RH_BLOCK)), dim3(RH_BLOCK), 0, st, a, nqt);
    hipLaunchKernelGGL(t5_attn_bias_kernel, dim3((int)((n2 + RH_BLOCK - 1) / RH_BLOCK)), dim3(RH_BLOCK), 0, st, a, nqt);
  }
  RH_LAUNCH_CHECK("rh_t5_attn_bwd");
  return 0;
}

extern "C" int rh_add_rms_norm_nparts(int M, int* nparts) {
  RH_REQUIRE(nparts && M >= 0, RH_E_BADARG, "rh_add_rms_norm_nparts: bad argument");
  *nparts = rms_grid(M);
  return 0;
}

extern "C" int rh_add_rms_norm_fwd(const float* h, const float* delta, const float* w, float eps, int M, int D, float* h_new,
                                   float* y, float* rstd, void* stream) {
  RH_REQUIRE(h && w && y && rstd && (!delta || h_new), RH_E_BADARG, "rh_add_rms_norm_fwd: null pointer");
  RH_REQUIRE(M >= 0 && D >= 1 && D <= kRmsMaxD, RH_E_UNSUPPORTED, "rh_add_rms_norm_fwd: D=%d unsupported (1 <= D <= %d)", D,
             kRmsMaxD);
  if (M == 0) return 0;
  hipLaunchKernelGGL(add_rms_norm_fwd_kernel, dim3(rms_grid(M)), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), h,
                     delta, w, eps, M, D, h_new, y, rstd);
  RH_LAUNCH_CHECK("rh_add_rms_norm_fwd");
  return 0;
}

extern "C" int rh_add_rms_norm_bwd(const float* h_new, const float* w, const float* rstd, const float* g_y, const float* g_res,
                                   int M, int D, float* g_h, float* part, void* stream) {
  RH_REQUIRE(h_new && w && rstd && g_y && g_h && part, RH_E_BADARG, "rh_add_rms_norm_bwd: null pointer");
  RH_REQUIRE(M >= 0 && D >= 1 && D <= kRmsMaxD, RH_E_UNSUPPORTED, "rh_add_rms_norm_bwd: D=%d unsupported (1 <= D <= %d)", D,
             kRmsMaxD);
  if (M == 0) return 0;
  hipLaunchKernelGGL(add_rms_norm_bwd_kernel, dim3(rms_grid(M)), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream),
                     h_new, w, rstd, g_y, g_res, M, D, g_h, part);
  RH_LAUNCH_CHECK("rh_add_rms_norm_bwd");
  return 0;
}
