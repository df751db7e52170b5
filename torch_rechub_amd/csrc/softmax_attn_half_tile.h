// The flash-style softmax attention tile of softmax_attn_tile.h for fp16 / bf16 operands: the same plan (64 queries x 64
// keys per workgroup, four wavefronts with one 32 x 32 accumulator quadrant each, online softmax, FlashAttention-2 backward,
// no atomics, bitwise reproducible), the same rule struct R and the same AttnArgs, whose q, k, v, out, g_out, g_q, g_k, g_v
// point at T elements here (strides count elements).  The five products run on v_mfma_f32_32x32x16_f16 / _bf16 (half_mfma.h).
//
// Numerics: q, k, v, g_out and the saved out are T; scores, bias, max, sum, lse, delta and g_bias are f32; the row sum adds
// the f32 weights before they are rounded; P (after the dropout multiplier) and dS are rounded to T, nearest even, when they
// are written as MFMA operands; out, g_q, g_k, g_v are rounded once at the store.  The dropout element index and key are
// those of the f32 body.  The per-diagonal partials, softmax_attn_diag_kernel and softmax_attn_bias_kernel are the f32 body's.
//
// How the operands move.  One MFMA step takes 16 k; lane (l32, kk) feeds eight consecutive k of row / column l32 as ONE
// 16-byte operand, so every operand must lie k-contiguous for its lane:
//   * the fragments fixed for a workgroup (Q and dO rows of a query tile; K and V rows of a key tile) are rows of memory
//     along the head's columns: loaded once from global memory into dh / 4 VGPRs of packed halves (zero past dh and L);
//   * S = Q K^T and dA = dO V^T contract over the head's columns, which is how the streaming rows lie in memory too.  The
//     forward stages K row-major ([64][128 + 8] halves, 17 408 B: rows 68 dwords apart, so 16 lanes' 16-byte reads cover
//     the 64 banks once); the two backward kernels load the streaming rows of their lane straight from global memory into
//     registers (issued before the tile's staging, so they fly during it) and keep LDS for the transposed copies;
//   * O += P V, dQ += dS K, dV += P^T dO, dK += dS^T Q contract over keys or queries, the row index of V, K, dO, Q in
//     memory.  Those tiles are staged TRANSPOSED ([128 columns][64 + 8] halves, 18 432 B) by a transposing store: a thread
//     loads the same 8 columns of two neighbouring rows (16 bytes each) and writes eight dwords (row r, row r + 1) down the
//     columns; a wavefront's 64 dwords of one store land in 64 banks.  The inner loops then read 16 bytes per lane, rows 36
//     dwords apart -- no 2-byte gathers;
//   * P and dS leave the accumulators, where a lane holds four consecutive ROWS of one column per register group.  The dK/dV
//     kernel needs them transposed ([key][query]), which is exactly that: one 8-byte store per group.  The dQ kernel needs
//     dS as [query][key]; it computes the TRANSPOSED scores S^T = K Q^T and dA^T = V dO^T (K, V rows as A from global memory,
//     the fixed Q, dO fragments as B -- the same registers either way), so again four consecutive keys of one query per
//     group.  The forward's P passes through the f32 score tile for the row maximum and sum anyway; the thread that owns a
//     quarter row writes its 16 weights as two 16-byte stores.
// Widths: the staged width is dh rounded up to 32 (the O / dQ / dK / dV quadrants are 32 columns wide), the score products
// take ceil(dh / 16) steps; no 64-column chunk loop and no reloads.  `vec`: bit 0 = 16-byte global loads of q, k, v are legal
// (dh % 8 == 0, 16-byte aligned bases and row stride), bit 1 = of out / g_out; single halves otherwise.
#pragma once

#include "half_mfma.h"
#include "softmax_attn_tile.h"

constexpr int kHS = kMaxDh / 16;  // MFMA steps over a head's columns
constexpr int kRLd = kMaxDh + 8;  // halves per row of a row-major tile [64][kRLd]
constexpr int kTLd = kT + 8;      // halves per row of a transposed tile [kMaxDh][kTLd] and of a P / dS tile [64][kTLd]

// row[k .. k + 8) as packed halves, zero from d on (row = null: a row past L)
static __device__ __forceinline__ v4u half_load8(const uint16_t* row, int k, int d, bool vec) {
  v4u v = {0u, 0u, 0u, 0u};
  if (row == nullptr || k >= d) return v;
  if (vec) return *reinterpret_cast<const v4u*>(row + k);  // d % 8 == 0: the piece is whole
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (k + j < d) v[j >> 1] |= (uint32_t)row[k + j] << (16 * (j & 1));
  return v;
}

static __device__ __forceinline__ const uint16_t* half_row(const uint16_t* base, int64_t ld, int col, int row, int L, int b) {
  return row < L ? base + ((int64_t)b * L + row) * ld + col : nullptr;
}

// the row's operands for the products over the head's columns: f[s] = row[16 s + 8 kk .. + 8)
static __device__ __forceinline__ void load_half_frag(v4u* f, const uint16_t* base, int64_t ld, int col, int row, int L,
                                                      int d, int b, int kk, bool vec) {
  const uint16_t* p = half_row(base, ld, col, row, L, b);
#pragma unroll
  for (int s = 0; s < kHS; ++s) f[s] = half_load8(p, 16 * s + 8 * kk, d, vec);
}

// rows [r0, r0 + 64) x columns [0, 8 np) of one head into s[64][kRLd]; zero outside L / d
static __device__ __forceinline__ void stage_half_rows(uint16_t* s, const uint16_t* base, int64_t ld, int col, int r0, int L,
                                                       int d, int np, int b, int tid, bool vec) {
#pragma unroll
  for (int e = tid; e < kT * (kMaxDh / 8); e += RH_BLOCK) {
    const int r = e / (kMaxDh / 8), p = e % (kMaxDh / 8);
    if (p >= np) continue;
    *reinterpret_cast<v4u*>(s + r * kRLd + 8 * p) = half_load8(half_row(base, ld, col, r0 + r, L, b), 8 * p, d, vec);
  }
}

// the same rows transposed into t[8 np][kTLd]: thread (rp = tid % 32, pg = tid / 32) takes rows 2 rp, 2 rp + 1 of the pieces
// pg, pg + 8 and writes one dword (both rows) per column
static __device__ __forceinline__ void stage_half_cols(uint16_t* t, const uint16_t* base, int64_t ld, int col, int r0, int L,
                                                       int d, int np, int b, int tid, bool vec) {
  const int rp = tid % 32, pg = tid / 32;
  const uint16_t* ra = half_row(base, ld, col, r0 + 2 * rp, L, b);
  const uint16_t* rb = half_row(base, ld, col, r0 + 2 * rp + 1, L, b);
#pragma unroll
  for (int p = pg; p < kMaxDh / 8; p += RH_BLOCK / 32) {
    if (p >= np) continue;
    const v4u x = half_load8(ra, 8 * p, d, vec), y = half_load8(rb, 8 * p, d, vec);
    uint32_t* o = reinterpret_cast<uint32_t*>(t + 8 * p * kTLd + 2 * rp);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int sh = 16 * (i & 1);
      o[i * (kTLd / 2)] = ((x[i >> 1] >> sh) & 0xffffu) | (((y[i >> 1] >> sh) & 0xffffu) << 16);
    }
  }
}

// acc += A (32 x 64) B (64 x 32): lane (li, kk) reads a[li][16 s + 8 kk .. + 8) and b[li][16 s + 8 kk .. + 8), rows kTLd apart
template <class T>
static __device__ __forceinline__ v16f mma_half_lds(v16f acc, const uint16_t* a, const uint16_t* b, int li, int kk) {
  const uint16_t* pa = a + li * kTLd + 8 * kk;
  const uint16_t* pb = b + li * kTLd + 8 * kk;
#pragma unroll
  for (int s = 0; s < kT / 16; ++s)
    acc = T::mfma(*reinterpret_cast<const v4u*>(pa + 16 * s), *reinterpret_cast<const v4u*>(pb + 16 * s), acc);
  return acc;
}

// the accumulator's register group g (rows 8 g + 4 kk .. + 4 of column li) rounded to T: four halves, one 8-byte store
template <class T>
static __device__ __forceinline__ v2u pack_group(const float* x, int g) {
  v2u r;
  r[0] = T::round(x[4 * g]) | (T::round(x[4 * g + 1]) << 16);
  r[1] = T::round(x[4 * g + 2]) | (T::round(x[4 * g + 3]) << 16);
  return r;
}

template <class T, class R>
__global__ __launch_bounds__(RH_BLOCK) void softmax_attn_half_fwd_kernel(const AttnArgs a, const int vec) {
  __shared__ __attribute__((aligned(16))) uint16_t ks[kT * kRLd], vt[kMaxDh * kTLd], ph[kT * kTLd];
  __shared__ float ps[kT * kLd];
  __shared__ float fac[kT];
  __shared__ typename R::Lds rs;
  const uint16_t* gq = reinterpret_cast<const uint16_t*>(a.q);
  const uint16_t* gk = reinterpret_cast<const uint16_t*>(a.k);
  const uint16_t* gv = reinterpret_cast<const uint16_t*>(a.v);
  uint16_t* gout = reinterpret_cast<uint16_t*>(a.out);
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int qt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int i0 = qt * kT, dh = a.dh, Lq = a.Lq, Lk = a.Lk, col = h * dh;
  const int ns = (dh + 15) / 16, np = (dh + 31) / 32 * 4;
  const bool v1 = vec & 1;
  const int nkt = R::key_tiles(a, qt);
  const DropKey dk = drop_key(a.p_drop, a.rng, a.saved_ctr, a.fwd);
  if (a.p_drop > 0.f && bh == 0 && qt == 0 && tid == 0) a.saved_ctr[0] = (int64_t)dk.ctr;
  const bool skip = R::scan_keys(rs, a, b, tid);
  v4u qf[kHS];
  load_half_frag(qf, gq, a.ldq, col, i0 + wm * 32 + li, Lq, dh, b, kk, v1);
  v16f o[kNC];
#pragma unroll
  for (int c = 0; c < kNC; ++c) o[c] = zero16();
  // running (max, sum) of row tid / 4; its four lanes agree
  const int row = tid / 4, part = tid % 4;
  float rm = -INFINITY, rl = 0.f;
  for (int kt = 0; kt < nkt; ++kt) {
    if (skip && !R::has_key(rs, kt)) continue;
    const int j0 = kt * kT;
    __syncthreads();
    stage_half_rows(ks, gk, a.ldkv, col, j0, Lk, dh, np, b, tid, v1);
    stage_half_cols(vt, gv, a.ldkv, col, j0, Lk, dh, np, b, tid, v1);
    R::stage_bias(rs, a, i0, j0, h, tid);
    __syncthreads();
    v16f s = zero16();
    {
      const uint16_t* kb = ks + (wn * 32 + li) * kRLd + 8 * kk;
#pragma unroll
      for (int t = 0; t < kHS; ++t)
        if (t < ns) s = T::mfma(qf[t], *reinterpret_cast<const v4u*>(kb + 16 * t), s);
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
      v4u pk[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
      if (nm > -INFINITY) {
        f = expf(rm - nm);  // 0 on the row's first tile (rm = -inf), and when only excluded keys came before
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int jl = part * 16 + q;
          const float x = ps[row * kLd + jl];
          const float p = x > -INFINITY ? expf(x - nm) : 0.f;
          sum += p;
          const float pd = p > 0.f ? p * attn_drop_mul(a, dk, bh, i0 + row, j0 + jl) : 0.f;
          pk[q >> 3][(q & 7) >> 1] |= T::round(pd) << (16 * (q & 1));
        }
        sum += __shfl_xor(sum, 1, RH_WAVE);
        sum += __shfl_xor(sum, 2, RH_WAVE);
      }
      *reinterpret_cast<v4u*>(ph + row * kTLd + part * 16) = pk[0];
      *reinterpret_cast<v4u*>(ph + row * kTLd + part * 16 + 8) = pk[1];
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
    // O quadrant: rows wm * 32, columns c * 64 + wn * 32;  O += P (64 x 64 keys) V (64 keys x 32 columns)
#pragma unroll
    for (int c = 0; c < kNC; ++c)
      if (c * kT + wn * 32 < dh) o[c] = mma_half_lds<T>(o[c], ph + wm * 32 * kTLd, vt + (c * kT + wn * 32) * kTLd, li, kk);
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
      if (i < Lq) gout[((int64_t)b * Lq + i) * ((int64_t)a.H * dh) + col + cc] = (uint16_t)T::round(o[c][r] * fac[il]);
    }
  }
}

// delta[b, h, i] = g_out[b, i, h, :] . out[b, i, h, :], both T, summed in f32 over ascending columns
template <class T>
__global__ __launch_bounds__(RH_BLOCK) void softmax_attn_half_delta_kernel(const AttnArgs a, const int vec) {
  const uint16_t* go = reinterpret_cast<const uint16_t*>(a.g_out);
  const uint16_t* out = reinterpret_cast<const uint16_t*>(a.out);
  const bool v2 = vec & 2;
  const int64_t n = (int64_t)a.B * a.H * a.Lq;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    const int i = (int)(e % a.Lq);
    const int64_t bh = e / a.Lq;
    const int h = (int)(bh % a.H);
    const int64_t b = bh / a.H;
    const int64_t off = (b * a.Lq + i) * ((int64_t)a.H * a.dh) + (int64_t)h * a.dh;
    float s = 0.f;
    for (int c = 0; c < a.dh; c += 8) {
      const v4u x = half_load8(go + off, c, a.dh, v2), y = half_load8(out + off, c, a.dh, v2);
#pragma unroll
      for (int j = 0; j < 8; ++j)  // the halves past dh are zero
        s = fmaf(T::value((uint16_t)(x[j >> 1] >> (16 * (j & 1)))), T::value((uint16_t)(y[j >> 1] >> (16 * (j & 1)))), s);
    }
    a.delta[e] = s;
  }
}

// dK, dV of one key tile: walks the query tiles that see it.
template <class T, class R>
__global__ __launch_bounds__(RH_BLOCK) void softmax_attn_half_dkv_kernel(const AttnArgs a, const int vec) {
  // Q and dO transposed ([column][query]); P^T and dS^T ([key][query])
  __shared__ __attribute__((aligned(16))) uint16_t qs[kMaxDh * kTLd], gs[kMaxDh * kTLd], xp[kT * kTLd], xd[kT * kTLd];
  __shared__ float lses[kT], dels[kT];
  __shared__ typename R::Lds rs;
  const uint16_t* gq = reinterpret_cast<const uint16_t*>(a.q);
  const uint16_t* gk = reinterpret_cast<const uint16_t*>(a.k);
  const uint16_t* gv = reinterpret_cast<const uint16_t*>(a.v);
  const uint16_t* ggo = reinterpret_cast<const uint16_t*>(a.g_out);
  uint16_t* ggk = reinterpret_cast<uint16_t*>(a.g_k);
  uint16_t* ggv = reinterpret_cast<uint16_t*>(a.g_v);
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int kt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int j0 = kt * kT, dh = a.dh, Lq = a.Lq, Lk = a.Lk, col = h * dh;
  const int ns = (dh + 15) / 16, np = (dh + 31) / 32 * 4;
  const bool v1 = vec & 1, v2 = vec & 2;
  const int64_t ldo = (int64_t)a.H * dh;
  const int nqt = (Lq + kT - 1) / kT;
  const float uw = R::uniform_weight(a);
  const DropKey dk = drop_key(a.p_drop, a.rng, a.saved_ctr, a.fwd);
  // K and V rows of the wavefront's key half as B operands (B[k][j] = K[j][k]), in registers
  v4u kf[kHS], vf[kHS];
  load_half_frag(kf, gk, a.ldkv, col, j0 + wn * 32 + li, Lk, dh, b, kk, v1);
  load_half_frag(vf, gv, a.ldkv, col, j0 + wn * 32 + li, Lk, dh, b, kk, v1);
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
    // this lane's Q and dO rows as A operands, from global memory: issued ahead of the staging
    v4u qa[kHS], ga[kHS];
    load_half_frag(qa, gq, a.ldq, col, i0 + wm * 32 + li, Lq, dh, b, kk, v1);
    load_half_frag(ga, ggo, ldo, col, i0 + wm * 32 + li, Lq, dh, b, kk, v2);
    __syncthreads();
    stage_half_cols(qs, gq, a.ldq, col, i0, Lq, dh, np, b, tid, v1);
    stage_half_cols(gs, ggo, ldo, col, i0, Lq, dh, np, b, tid, v2);
    if (tid < kT) {
      const int i = i0 + tid;
      lses[tid] = i < Lq ? a.lse[(int64_t)bh * Lq + i] : 0.f;
      dels[tid] = i < Lq ? a.delta[(int64_t)bh * Lq + i] : 0.f;
    }
    R::stage_bias(rs, a, i0, j0, h, tid);
    __syncthreads();
    v16f s = zero16(), da = zero16();
#pragma unroll
    for (int t = 0; t < kHS; ++t) {
      if (t >= ns) continue;
      s = T::mfma(qa[t], kf[t], s);
      da = T::mfma(ga[t], vf[t], da);
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
    // register group g holds queries wm * 32 + 8 g + 4 kk .. + 4 of key wn * 32 + li: the transposed tiles' own layout
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int e = (wn * 32 + li) * kTLd + wm * 32 + 8 * g + 4 * kk;
      *reinterpret_cast<v2u*>(xp + e) = pack_group<T>(pd, g);
      *reinterpret_cast<v2u*>(xd + e) = pack_group<T>(ds, g);
    }
    __syncthreads();
    // quadrants: keys wm * 32, columns c * 64 + wn * 32;  dV += P^T dO, dK += dS^T Q
#pragma unroll
    for (int c = 0; c < kNC; ++c) {
      if (c * kT + wn * 32 >= dh) continue;
      dvacc[c] = mma_half_lds<T>(dvacc[c], xp + wm * 32 * kTLd, gs + (c * kT + wn * 32) * kTLd, li, kk);
      dkacc[c] = mma_half_lds<T>(dkacc[c], xd + wm * 32 * kTLd, qs + (c * kT + wn * 32) * kTLd, li, kk);
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
      ggk[off] = (uint16_t)T::round(dkacc[c][r] * gscale);
      ggv[off] = (uint16_t)T::round(dvacc[c][r]);
    }
  }
}

// dQ of one query tile, and this tile's sums of dS by diagonal (the bias bucket depends on j - i alone).  The scores are
// computed transposed: wavefront (wm, wn) holds keys wm * 32 + acc_row x query wn * 32 + li.
template <class T, class R>
__global__ __launch_bounds__(RH_BLOCK) void softmax_attn_half_dq_kernel(const AttnArgs a, const int vec) {
  // K transposed ([column][key]); dS ([query][key]) as T, and as f32 for the diagonal sums.  xs and pacc are reserved
  // whether or not there is a bias table (static LDS); without one they are neither written nor read.
  __shared__ __attribute__((aligned(16))) uint16_t ks[kMaxDh * kTLd], xh[kT * kTLd];
  __shared__ float xs[kT * kLd];
  __shared__ float pacc[R::kMaxDiag];
  __shared__ typename R::Lds rs;
  const uint16_t* gq = reinterpret_cast<const uint16_t*>(a.q);
  const uint16_t* gk = reinterpret_cast<const uint16_t*>(a.k);
  const uint16_t* gv = reinterpret_cast<const uint16_t*>(a.v);
  const uint16_t* ggo = reinterpret_cast<const uint16_t*>(a.g_out);
  uint16_t* ggq = reinterpret_cast<uint16_t*>(a.g_q);
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int qt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int i0 = qt * kT, dh = a.dh, Lq = a.Lq, Lk = a.Lk, col = h * dh, nd = a.nd;
  const int ns = (dh + 15) / 16, np = (dh + 31) / 32 * 4;
  const bool v1 = vec & 1, v2 = vec & 2;
  const int64_t ldo = (int64_t)a.H * dh;
  const int nkt = R::key_tiles(a, qt);
  const float uw = R::uniform_weight(a);
  const DropKey dk = drop_key(a.p_drop, a.rng, a.saved_ctr, a.fwd);
  // Q and dO rows of the wavefront's query half as B operands (B[k][i] = Q[i][k]), in registers; the lane's query
  const int il = wn * 32 + li, i = i0 + il;
  v4u qf[kHS], gf[kHS];
  load_half_frag(qf, gq, a.ldq, col, i, Lq, dh, b, kk, v1);
  load_half_frag(gf, ggo, ldo, col, i, Lq, dh, b, kk, v2);
  const float lsei = i < Lq ? a.lse[(int64_t)bh * Lq + i] : 0.f;
  const float deli = i < Lq ? a.delta[(int64_t)bh * Lq + i] : 0.f;
  if (a.bias)
    for (int e = tid; e < nd; e += RH_BLOCK) pacc[e] = 0.f;
  v16f dq[kNC];
#pragma unroll
  for (int c = 0; c < kNC; ++c) dq[c] = zero16();
  const bool skip = R::scan_keys(rs, a, b, tid);
  for (int kt = 0; kt < nkt; ++kt) {
    if (skip && !R::has_key(rs, kt)) continue;
    const int j0 = kt * kT;
    // this lane's K and V rows as A operands, from global memory: issued ahead of the staging
    v4u ka[kHS], va[kHS];
    load_half_frag(ka, gk, a.ldkv, col, j0 + wm * 32 + li, Lk, dh, b, kk, v1);
    load_half_frag(va, gv, a.ldkv, col, j0 + wm * 32 + li, Lk, dh, b, kk, v1);
    __syncthreads();
    stage_half_cols(ks, gk, a.ldkv, col, j0, Lk, dh, np, b, tid, v1);
    R::stage_bias(rs, a, i0, j0, h, tid);
    v16f s = zero16(), da = zero16();
#pragma unroll
    for (int t = 0; t < kHS; ++t) {
      if (t >= ns) continue;
      s = T::mfma(ka[t], qf[t], s);
      da = T::mfma(va[t], gf[t], da);
    }
    __syncthreads();
    float ds[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jl = wm * 32 + acc_row(r, kk), j = j0 + jl;
      const bool kok = R::key_ok(a, b, j);
      float d = 0.f;
      R::with_weight(rs, a, kok, uw, s[r], i, j, il, jl, h, lsei,
                     [&](float p) { d = p * (da[r] * attn_drop_mul(a, dk, bh, i, j) - deli); });
      ds[r] = d;
      if (a.bias) xs[il * kLd + jl] = d;
    }
    // register group g holds keys wm * 32 + 8 g + 4 kk .. + 4 of query il: one 8-byte store
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<v2u*>(xh + il * kTLd + wm * 32 + 8 * g + 4 * kk) = pack_group<T>(ds, g);
    __syncthreads();
    // dQ quadrant: queries wm * 32, columns c * 64 + wn * 32;  dQ += dS K
#pragma unroll
    for (int c = 0; c < kNC; ++c)
      if (c * kT + wn * 32 < dh) dq[c] = mma_half_lds<T>(dq[c], xh + wm * 32 * kTLd, ks + (c * kT + wn * 32) * kTLd, li, kk);
    // thread t < 127 owns the tile diagonal jl - il = t - 63 and sums it over il ascending
    if (a.bias && tid < 2 * kT - 1) {
      const int e = tid - (kT - 1);
      const int d = R::diag(a, (j0 - i0) + e);
      if (d >= 0 && d < nd) {
        float sum = 0.f;
        for (int r = e < 0 ? -e : 0; r < kT && r + e < kT; ++r) sum += xs[r * kLd + r + e];
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
      const int iq = i0 + wm * 32 + acc_row(r, kk);
      if (iq < Lq) ggq[((int64_t)b * Lq + iq) * a.ldgq + col + cc] = (uint16_t)T::round(dq[c][r] * gscale);
    }
  }
  if (a.bias) {
    __syncthreads();
    const int64_t p = (int64_t)bh * gridDim.y + qt;
    for (int e = tid; e < nd; e += RH_BLOCK) a.part[p * nd + e] = pacc[e];
  }
}

// whether 16-byte loads of rows of `p` with row stride ld (elements) and heads dh wide are legal
static inline bool half_rows_vec(const void* p, int64_t ld, int dh) {
  return dh % 8 == 0 && ld % 8 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0;
}
