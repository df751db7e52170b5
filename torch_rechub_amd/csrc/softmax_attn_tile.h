// The flash-style softmax attention tile, forward and backward, shared by the two attention families that use it: HLLM's
// causal attention with a scale and linear buckets (hllm.hip) and T5's three forms (t5attn.hip, Lq > 8).
//
// One workgroup owns a 64-query tile of one (sample, head) and walks the key tiles with a running (max, sum) per row
// (online softmax); only O and the per-row log-sum-exp leave the chip.  The backward recomputes P tile by tile from Q, K,
// the bias and the log-sum-exp (FlashAttention-2 layout, no float atomics): one kernel per key tile owns dK and dV and
// walks the query tiles, one kernel per query tile owns dQ and this tile's per-diagonal sums of dS; the bias table's
// gradient is those partials summed over (sample, query tile) in that order, then over the diagonals of a bucket in
// ascending index.  Bitwise reproducible.
//
// Head widths up to 128: the fragments that stay fixed for a workgroup (Q and dO rows of a query tile; K and V rows of a
// key tile) live in registers, dh / 2 values per lane; the tiles that stream (K, V; Q, dO) pass through 64 x 64 LDS
// buffers in column chunks of 64 (three 64 x 65 buffers), so a wider head costs a second pass over the chunk loop, not
// a larger footprint.  Columns past dh are zero in LDS.  The products run on the 64 x 64 MFMA tile of mfma_tile.h.
//
// Dropout: common.h's key over element ((b H + h) Lq + i) Lk + j; the forward saves the counter it drew, the backward
// re-derives the mask from it.
//
// What differs between the families is a compile-time rule R, a struct of static functions and constants:
//   kFwdWaves            second argument of the forward's __launch_bounds__ (0: none)
//   kMaxDiag             diagonals a query tile's sums of dS may span (LDS floats of the dQ kernel)
//   Lds                  what the rule stages in LDS per workgroup (empty: none)
//   key_tiles(a, qt)     key tiles [0, n) a query tile visits
//   first_query_tile(a, kt)  query tiles [first, nqt) a key tile visits
//   scan_keys(lds, a, b, tid), has_key(lds, kt)  whether key tiles may be passed over, and which; all threads call scan_keys
//   stage_bias(lds, a, i0, j0, h, tid)           per tile pair, before the barrier that precedes the scores
//   key_ok(a, b, j)      the key column's own state
//   score(lds, a, kok, s, i, j, il, jl, h)       the forward's score of (i, j) from the product s; -inf outside the tile's range
//   lse(rm, rl)          the row's saved log-sum-exp
//   uniform_weight(a), with_weight(lds, a, kok, uw, s, i, j, il, jl, h, lse, use)  the backward's weight p of (i, j)
//                        recomputed from the row's lse: calls use(p) where (i, j) contributes, else nothing
//   grad_scale(a)        factor of g_q and g_k at the store
//   diag(a, j - i)       index of a diagonal in pacc / part (extent a.nd)
//   bucket(a, d)         bias bucket of diagonal index d
#pragma once

#include <float.h>
#include <math.h>

#include "mfma_tile.h"

constexpr int kMaxDh = RH_ATTN_MAX_DH;
constexpr int kNC = kMaxDh / kT;  // column chunks of a head
constexpr int kMaxL = RH_ATTN_MAX_L;

struct AttnArgs {
  const float* q;         // (B, Lq, H, dh) view, row stride ldq
  int64_t ldq;
  const float* k;         // (B, Lk, H, dh) views, row stride ldkv
  const float* v;
  int64_t ldkv;
  const uint8_t* mask;    // (B, Lk) or null
  const float* bias;      // (nb, H) or null
  const int32_t* bucket;  // (nd,) or null (linear buckets)
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
  int B, Lq, Lk, H, dh, nb, causal, fwd, nd, N;
  float p_drop, scale;
};

// the row's fragment for the A / B operand of a product over the head's columns: element s = column 2 s + kk
static __device__ __forceinline__ void load_frag(float* f, const float* base, int64_t ld, int col, int row, int L, int d,
                                                 int b, int kk) {
#pragma unroll
  for (int s = 0; s < kMaxDh / 2; ++s) {
    const int c = 2 * s + kk;
    f[s] = (row < L && c < d) ? base[((int64_t)b * L + row) * ld + col + c] : 0.f;
  }
}

static __device__ __forceinline__ float attn_drop_mul(const AttnArgs& a, const DropKey& d, int64_t bh, int i, int j) {
  return drop_mul(a.p_drop, d, ((uint64_t)bh * a.Lq + i) * a.Lk + j);
}

template <class R>
__global__ __launch_bounds__(RH_BLOCK, R::kFwdWaves) void softmax_attn_fwd_kernel(const AttnArgs a) {
  __shared__ float ks[kT * kLd], vs[kT * kLd], ps[kT * kLd];
  __shared__ float fac[kT];
  __shared__ typename R::Lds rs;
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int qt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int i0 = qt * kT, dh = a.dh, Lq = a.Lq, Lk = a.Lk, col = h * dh;
  const int nc = (dh + kT - 1) / kT, dh2 = (dh + 1) & ~1;
  const int nkt = R::key_tiles(a, qt);
  const DropKey dk = drop_key(a.p_drop, a.rng, a.saved_ctr, a.fwd);
  if (a.p_drop > 0.f && bh == 0 && qt == 0 && tid == 0) a.saved_ctr[0] = (int64_t)dk.ctr;
  const bool skip = R::scan_keys(rs, a, b, tid);
  float qf[kMaxDh / 2];
  load_frag(qf, a.q, a.ldq, col, i0 + wm * 32 + li, Lq, dh, b, kk);
  v16f o[kNC];
#pragma unroll
  for (int c = 0; c < kNC; ++c) o[c] = zero16();
  // running (max, sum) of row tid / 4; its four lanes agree
  const int row = tid / 4, part = tid % 4;
  float rm = -INFINITY, rl = 0.f;
  for (int kt = 0; kt < nkt; ++kt) {
    if (skip && !R::has_key(rs, kt)) continue;
    const int j0 = kt * kT;
    v16f s = zero16();
#pragma unroll
    for (int c = 0; c < kNC; ++c) {
      if (c >= nc) continue;
      __syncthreads();
      load_tile(ks, a.k, a.ldkv, col, c * kT, j0, Lk, dh, b, tid);
      if (c == 0) {
        load_tile(vs, a.v, a.ldkv, col, 0, j0, Lk, dh, b, tid);
        R::stage_bias(rs, a, i0, j0, h, tid);
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kT; k += 2)
        if (c * kT + k < dh2)
          s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[c * (kT / 2) + k / 2], ks[(wn * 32 + li) * kLd + k + kk], s, 0, 0, 0);
    }
    {
      const int jl = wn * 32 + li, j = j0 + jl;
      const bool kok = R::key_ok(a, b, j);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int il = wm * 32 + acc_row(r, kk), i = i0 + il;
        ps[il * kLd + jl] = R::score(rs, a, kok, s[r], i, j, il, jl, h);
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
          ps[row * kLd + jl] = p > 0.f ? p * attn_drop_mul(a, dk, bh, i0 + row, j0 + jl) : 0.f;
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
      // O quadrant: rows wm * 32, columns c * 64 + wn * 32;  O += P (64 x 64 keys) V (64 keys x 64 columns)
      if (c * kT + wn * 32 < dh) o[c] = mma_lds(o[c], ps + wm * 32 * kLd, kLd, 1, vs + wn * 32, kLd, 1, kT, li, kk);
    }
  }
  __syncthreads();
  if (part == 0) {
    fac[row] = rl > 0.f ? 1.f / rl : 0.f;
    if (i0 + row < Lq) a.lse[(int64_t)bh * Lq + i0 + row] = R::lse(rm, rl);
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

// delta[b, h, i] = g_out[b, i, h, :] . out[b, i, h, :]
static __global__ __launch_bounds__(RH_BLOCK) void softmax_attn_delta_kernel(const AttnArgs a) {
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

// dK, dV of one key tile: walks the query tiles that see it.
template <class R>
__global__ __launch_bounds__(RH_BLOCK) void softmax_attn_dkv_kernel(const AttnArgs a) {
  __shared__ float qs[kT * kLd], gs[kT * kLd], xs[kT * kLd];
  __shared__ float lses[kT], dels[kT];
  __shared__ typename R::Lds rs;
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int kt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int j0 = kt * kT, dh = a.dh, Lq = a.Lq, Lk = a.Lk, col = h * dh;
  const int nc = (dh + kT - 1) / kT, dh2 = (dh + 1) & ~1;
  const int64_t ldo = (int64_t)a.H * dh;
  const int nqt = (Lq + kT - 1) / kT;
  const float uw = R::uniform_weight(a);
  const DropKey dk = drop_key(a.p_drop, a.rng, a.saved_ctr, a.fwd);
  // K and V rows of the wavefront's key half as B fragments (B[k][j] = K[j][k]), in registers
  float kf[kMaxDh / 2], vf[kMaxDh / 2];
  load_frag(kf, a.k, a.ldkv, col, j0 + wn * 32 + li, Lk, dh, b, kk);
  load_frag(vf, a.v, a.ldkv, col, j0 + wn * 32 + li, Lk, dh, b, kk);
  const bool kok = R::key_ok(a, b, j0 + wn * 32 + li);
  v16f dkacc[kNC], dvacc[kNC];
#pragma unroll
  for (int c = 0; c < kNC; ++c) {
    dkacc[c] = zero16();
    dvacc[c] = zero16();
  }
  // a key tile without a valid key in a sample that has one elsewhere: dK = dV = 0, written below
  const bool dead = R::scan_keys(rs, a, b, tid) && !R::has_key(rs, kt);
  for (int qt = R::first_query_tile(a, kt); qt < (dead ? 0 : nqt); ++qt) {
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
        R::stage_bias(rs, a, i0, j0, h, tid);
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
      R::with_weight(rs, a, kok, uw, s[r], i, j, il, jl, h, lses[il], [&](float p) {
        const float m = attn_drop_mul(a, dk, bh, i, j);
        pd[r] = p * m;
        ds[r] = p * (da[r] * m - dels[il]);
      });
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
  const float gscale = R::grad_scale(a);
#pragma unroll
  for (int c = 0; c < kNC; ++c) {
    const int cc = c * kT + wn * 32 + li;
    if (cc >= dh) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = j0 + wm * 32 + acc_row(r, kk);
      if (j >= Lk) continue;
      const int64_t off = ((int64_t)b * Lk + j) * a.ldgkv + col + cc;
      a.g_k[off] = dkacc[c][r] * gscale;
      a.g_v[off] = dvacc[c][r];
    }
  }
}

// dQ of one query tile, and this tile's sums of dS by diagonal (the bias bucket depends on j - i alone).
template <class R>
__global__ __launch_bounds__(RH_BLOCK) void softmax_attn_dq_kernel(const AttnArgs a) {
  __shared__ float ks[kT * kLd], vs[kT * kLd], xs[kT * kLd];
  __shared__ float pacc[R::kMaxDiag];
  __shared__ typename R::Lds rs;
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int qt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int i0 = qt * kT, dh = a.dh, Lq = a.Lq, Lk = a.Lk, col = h * dh, nd = a.nd;
  const int nc = (dh + kT - 1) / kT, dh2 = (dh + 1) & ~1;
  const int64_t ldo = (int64_t)a.H * dh;
  const int nkt = R::key_tiles(a, qt);
  const float uw = R::uniform_weight(a);
  const DropKey dk = drop_key(a.p_drop, a.rng, a.saved_ctr, a.fwd);
  // Q and dO rows of the wavefront's query half as A fragments, in registers
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
  const bool skip = R::scan_keys(rs, a, b, tid);
  for (int kt = 0; kt < nkt; ++kt) {
    if (skip && !R::has_key(rs, kt)) continue;
    const int j0 = kt * kT;
    v16f s = zero16(), da = zero16();
#pragma unroll
    for (int c = 0; c < kNC; ++c) {
      if (c >= nc) continue;
      __syncthreads();
      load_tile(ks, a.k, a.ldkv, col, c * kT, j0, Lk, dh, b, tid);
      load_tile(vs, a.v, a.ldkv, col, c * kT, j0, Lk, dh, b, tid);
      if (c == 0) R::stage_bias(rs, a, i0, j0, h, tid);
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
      const bool kok = R::key_ok(a, b, j);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int il = wm * 32 + acc_row(r, kk), i = i0 + il;
        float d = 0.f;
        R::with_weight(rs, a, kok, uw, s[r], i, j, il, jl, h, lser[r],
                       [&](float p) { d = p * (da[r] * attn_drop_mul(a, dk, bh, i, j) - delr[r]); });
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
    // thread t < 127 owns the tile diagonal jl - il = t - 63 and sums it over il ascending
    if (a.bias && tid < 2 * kT - 1) {
      const int e = tid - (kT - 1);
      const int d = R::diag(a, (j0 - i0) + e);
      if (d >= 0 && d < nd) {
        float sum = 0.f;
        for (int il = e < 0 ? -e : 0; il < kT && il + e < kT; ++il) sum += xs[il * kLd + il + e];
        pacc[d] += sum;
      }
    }
  }
  const float gscale = R::grad_scale(a);
#pragma unroll
  for (int c = 0; c < kNC; ++c) {
    const int cc = c * kT + wn * 32 + li;
    if (cc >= dh) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + wm * 32 + acc_row(r, kk);
      if (i < Lq) a.g_q[((int64_t)b * Lq + i) * a.ldgq + col + cc] = dq[c][r] * gscale;
    }
  }
  if (a.bias) {
    __syncthreads();
    const int64_t p = (int64_t)bh * gridDim.y + qt;
    for (int e = tid; e < nd; e += RH_BLOCK) a.part[p * nd + e] = pacc[e];
  }
}

// per-head totals by diagonal: part[(B H nqt + h), d] = sum over (b, query tile) in that order
static __global__ __launch_bounds__(RH_BLOCK) void softmax_attn_diag_kernel(const AttnArgs a, int nqt) {
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

// g_bias[c, h] = sum over the diagonals of bucket c in ascending order of the family's own diagonal index
template <class R>
__global__ __launch_bounds__(RH_BLOCK) void softmax_attn_bias_kernel(const AttnArgs a, int nqt) {
  const int64_t n = (int64_t)a.nb * a.H;
  const float* tot = a.part + (int64_t)a.B * a.H * nqt * a.nd;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    const int h = (int)(e % a.H), c = (int)(e / a.H);
    float sum = 0.f;
    for (int d = 0; d < a.nd; ++d)
      if (R::bucket(a, d) == c) sum += tot[(int64_t)h * a.nd + d];
    a.g_bias[e] = sum;
  }
}

// the conditions both families share; the caller adds those on its own lengths, strides and tables
static int attn_check(const char* name, const AttnArgs& a) {
  RH_REQUIRE(a.q && a.k && a.v, RH_E_BADARG, "%s: null pointer", name);
  RH_REQUIRE(a.dh >= 1 && a.dh <= kMaxDh, RH_E_UNSUPPORTED, "%s: head width %d unsupported (1 <= dh <= %d)", name, a.dh,
             kMaxDh);
  RH_REQUIRE(!a.bias || a.nb >= 1, RH_E_UNSUPPORTED, "%s: num_buckets=%d unsupported (>= 1)", name, a.nb);
  RH_REQUIRE((int64_t)a.B * a.H <= 0x7FFFFFFF, RH_E_UNSUPPORTED, "%s: B * H = %lld exceeds the grid", name,
             (long long)a.B * a.H);
  RH_REQUIRE(a.p_drop >= 0.f && a.p_drop < 1.f, RH_E_BADARG, "%s: dropout p=%g outside [0, 1)", name, (double)a.p_drop);
  RH_REQUIRE(a.p_drop == 0.f || (a.rng && a.saved_ctr), RH_E_BADARG, "%s: dropout without its (seed, counter) state", name);
  return 0;
}

static AttnArgs attn_args(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, int B, int Lq, int Lk,
                          int H, int dh, const float* bias, int nb, int nd, float p_drop, const int64_t* rng,
                          const int64_t* saved_ctr, const float* out, const float* lse) {
  AttnArgs a{};
  a.q = q;
  a.ldq = ldq;
  a.k = k;
  a.v = v;
  a.ldkv = ldkv;
  a.bias = bias;
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
  a.nd = nd;
  a.p_drop = p_drop;
  return a;
}

static void attn_bwd_args(AttnArgs& a, const float* g_out, float* delta, float* g_q, int64_t ldgq, float* g_k, float* g_v,
                          int64_t ldgkv, float* part, float* g_bias) {
  a.g_out = g_out;
  a.delta = delta;
  a.g_q = g_q;
  a.ldgq = ldgq;
  a.g_k = g_k;
  a.g_v = g_v;
  a.ldgkv = ldgkv;
  a.part = part;
  a.g_bias = g_bias;
}
