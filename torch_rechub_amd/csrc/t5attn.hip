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
// Two paths.  Lq > 8: the flash-style tile kernels of softmax_attn_tile.h, the body hllm.hip runs too, under this file's
// rule T5Rule -- two lengths, the -FLT_MAX exclusion with the key mask and the causal test, key tiles without a valid key
// passed over, the bias of a tile pair's 127 diagonals staged in LDS from the host's bucket table, the lse = +inf mark,
// diagonals indexed (j - i) + (Lq - 1), and two waves per SIMD asked of the forward.  Lq <= 8 (TIGER's decoder:
// n_levels + 1 tokens): a 64-row MFMA tile would be 7/8 padding or more (15/16 at four queries), so one WAVEFRONT owns a
// (sample, head), four to a workgroup; a lane
// owns a key of the current 64-key chunk and the dot products of its row with all (<= 8) queries, the chunk's weights pass
// through 2 KB of LDS per wavefront and lanes turn to the head's columns for P V (and dS K).  Same online softmax, same
// -FLT_MAX rule, same dropout element index, so the two paths agree wherever both could run.
//
// g_bias: per-workgroup (per-wavefront on the narrow path) sums of dS by diagonal, summed over (sample, query tile) in
// that order, then over the diagonals of a bucket in ascending order.  No atomics: bitwise reproducible.
#include "softmax_attn_tile.h"

namespace {

constexpr int kSmallQ = 8;        // queries a wavefront of the narrow path carries
constexpr int kWG = RH_BLOCK / RH_WAVE;

struct T5Rule {
  static constexpr int kFwdWaves = 2;  // without it: 228 + 32 registers, one wave per SIMD (build figures)
  static constexpr int kMaxDiag = 2 * kMaxL;
  struct alignas(16) Lds {  // aligned as a __shared__ array of its own: a lane's four consecutive bd[] are one 128-bit read
    float bd[2 * kT];      // the bias of the 127 diagonals jl - il = e - 63 of the current tile pair
    int tv[kMaxL / kT];    // tv[t] = key tile t has a valid key
  };

  // Causal WITHOUT a mask: every row keeps its own key, so the key tiles past the diagonal weigh 0 and are not visited.
  // Causal WITH a mask, a row whose keys j <= i are all masked (a left-padded sample) has no key left and weighs ALL Lk
  // keys 1 / Lk, those past the diagonal included: every key tile is visited then, as the narrow path does.
  static __device__ __forceinline__ bool stop_at_diagonal(const AttnArgs& a) { return a.causal && !a.mask; }
  static __device__ __forceinline__ int key_tiles(const AttnArgs& a, int qt) {
    return stop_at_diagonal(a) ? qt + 1 : (a.Lk + kT - 1) / kT;
  }
  static __device__ __forceinline__ int first_query_tile(const AttnArgs& a, int kt) { return stop_at_diagonal(a) ? kt : 0; }

  // Key tiles that hold no valid key may be passed over when the row still has a valid key elsewhere: their weights are
  // exp(-FLT_MAX - max) = 0 exactly, so the result is the same to the bit.  Not under the causal rule (a row's own valid set is
  // then smaller than the sample's) and not for a sample with no valid key at all (every key then weighs 1 / Lk).
  // Returns whether empty tiles may be skipped.
  static __device__ __forceinline__ bool scan_keys(Lds& l, const AttnArgs& a, int b, int tid) {
    if (!a.mask || a.causal) return false;
    if (tid < kMaxL / kT) l.tv[tid] = 0;
    __syncthreads();
    for (int j = tid; j < a.Lk; j += RH_BLOCK)
      if (a.mask[(int64_t)b * a.Lk + j] != 0) l.tv[j / kT] = 1;
    __syncthreads();
    int any = 0;
    for (int t = 0; t < (a.Lk + kT - 1) / kT; ++t) any |= l.tv[t];
    return any != 0;
  }
  static __device__ __forceinline__ bool has_key(const Lds& l, int kt) { return l.tv[kt] != 0; }

  static __device__ __forceinline__ int diag(const AttnArgs& a, int dji) { return dji + (a.Lq - 1); }
  static __device__ __forceinline__ int bucket(const AttnArgs& a, int d) { return a.bucket[d]; }
  static __device__ __forceinline__ void stage_bias(Lds& l, const AttnArgs& a, int i0, int j0, int h, int tid) {
    if (a.bias && tid < 2 * kT - 1) {
      const int d = diag(a, (j0 - i0) + (tid - (kT - 1)));
      l.bd[tid] = (d >= 0 && d < a.nd) ? a.bias[(int64_t)a.bucket[d] * a.H + h] : 0.f;
    }
  }
  static __device__ __forceinline__ bool key_ok(const AttnArgs& a, int b, int j) {
    return j < a.Lk && (!a.mask || a.mask[(int64_t)b * a.Lk + j] != 0);
  }
  static __device__ __forceinline__ float score(const Lds& l, const AttnArgs& a, bool kok, float s, int i, int j, int il,
                                                int jl, int) {
    float x = -INFINITY;
    if (i < a.Lq && j < a.Lk) {
      x = -FLT_MAX;
      if (kok && (!a.causal || j <= i)) x = a.bias ? s + l.bd[jl - il + kT - 1] : s;
    }
    return x;
  }
  static __device__ __forceinline__ float lse(float rm, float rl) { return rm == -FLT_MAX ? INFINITY : rm + logf(rl); }
  // the weight of (i, j) recomputed from the row's lse, i < Lq and j < Lk
  static __device__ __forceinline__ float weight_of(float s, float bias, float lse, bool ok, float inv_lk) {
    if (lse == INFINITY) return inv_lk;  // no key left: uniform
    return ok ? expf(s + bias - lse) : 0.f;
  }
  static __device__ __forceinline__ float uniform_weight(const AttnArgs& a) { return 1.f / (float)a.Lk; }
  template <class F>
  static __device__ __forceinline__ void with_weight(const Lds& l, const AttnArgs& a, bool kok, float uw, float s, int i,
                                                     int j, int il, int jl, int, float lse, F use) {
    if (i < a.Lq && j < a.Lk) {
      const float p = weight_of(s, a.bias ? l.bd[jl - il + kT - 1] : 0.f, lse, kok && (!a.causal || j <= i), uw);
      if (p > 0.f) use(p);
    }
  }
  static __device__ __forceinline__ float grad_scale(const AttnArgs&) { return 1.f; }
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, RH_WAVE));
  return v;
}

// ------------------------------------------------------------------------------------------------------------------
// Lq <= 8: one wavefront per (sample, head), a lane per key of the 64-key chunk
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RH_BLOCK) void t5_attn_small_fwd_kernel(const AttnArgs a) {
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
  const DropKey dk = drop_key(a.p_drop, a.rng, a.saved_ctr, a.fwd);
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
    const bool kok = T5Rule::key_ok(a, b, j);
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
        if (p > 0.f) p *= attn_drop_mul(a, dk, bh, i, j);
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

__global__ __launch_bounds__(RH_BLOCK) void t5_attn_small_bwd_kernel(const AttnArgs a) {
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
  const DropKey dk = drop_key(a.p_drop, a.rng, a.saved_ctr, a.fwd);
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
    const bool kok = T5Rule::key_ok(a, b, j);
    float pd[kSmallQ], ds[kSmallQ];
#pragma unroll
    for (int i = 0; i < kSmallQ; ++i) {
      pd[i] = 0.f;
      ds[i] = 0.f;
      if (i < Lq && inb) {
        const bool ok = kok && (!a.causal || j <= i);
        const float bv = (a.bias && ok) ? a.bias[(int64_t)a.bucket[j - i + Lq - 1] * a.H + h] : 0.f;
        const float p = T5Rule::weight_of(s[i], bv, lser[i], ok, inv_lk);
        if (p > 0.f) {
          const float m = attn_drop_mul(a, dk, bh, i, j);
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

int t5_nqt(int Lq) { return Lq <= kSmallQ ? 1 : (Lq + kT - 1) / kT; }

int t5_check(const char* name, const AttnArgs& a) {
  if (int rc = attn_check(name, a)) return rc;
  RH_REQUIRE(a.B >= 0 && a.H >= 1 && a.Lq >= 1 && a.Lq <= kMaxL && a.Lk >= 1 && a.Lk <= kMaxL, RH_E_UNSUPPORTED,
             "%s: Lq=%d Lk=%d H=%d unsupported (1 <= Lq, Lk <= %d, H >= 1)", name, a.Lq, a.Lk, a.H, kMaxL);
  RH_REQUIRE(!a.causal || a.Lq == a.Lk, RH_E_UNSUPPORTED, "%s: causal attention needs Lq == Lk (got %d, %d)", name, a.Lq,
             a.Lk);
  RH_REQUIRE(!a.bias || a.bucket, RH_E_BADARG, "%s: a bias table without its bucket table", name);
  RH_REQUIRE(a.ldq >= (int64_t)a.H * a.dh && a.ldkv >= (int64_t)a.H * a.dh, RH_E_BADARG, "%s: row stride %lld / %lld too small",
             name, (long long)a.ldq, (long long)a.ldkv);
  return 0;
}

AttnArgs t5_args(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, int B, int Lq, int Lk, int H,
                 int dh, const uint8_t* mask, int causal, const float* bias, const int32_t* bucket, int nb, float p_drop,
                 const int64_t* rng, const int64_t* saved_ctr, const float* out, const float* lse) {
  AttnArgs a = attn_args(q, ldq, k, v, ldkv, B, Lq, Lk, H, dh, bias, nb, Lq + Lk - 1, p_drop, rng, saved_ctr, out, lse);
  a.mask = mask;
  a.bucket = bucket;
  a.causal = causal ? 1 : 0;
  return a;
}

// ------------------------------------------------------------------------------------------------------------------
// RMS norm with the residual add: one wavefront per row, the row's D <= 1024 values in 16 registers per lane
// ------------------------------------------------------------------------------------------------------------------
constexpr int kRmsMaxD = RH_RMS_NORM_MAX_D;
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
  AttnArgs a = t5_args(q, ldq, k, v, ldkv, B, Lq, Lk, H, dh, key_mask, causal, bias, bucket, nb, p_drop, rng, saved_ctr, out, lse);
  a.fwd = 1;
  if (int rc = t5_check("rh_t5_attn_fwd", a)) return rc;
  RH_REQUIRE(out && lse, RH_E_BADARG, "rh_t5_attn_fwd: null output");
  if (B == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (Lq <= kSmallQ) {
    const int grid = (int)(((int64_t)B * H + kWG - 1) / kWG);
    hipLaunchKernelGGL(t5_attn_small_fwd_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a);
  } else {
    hipLaunchKernelGGL(softmax_attn_fwd_kernel<T5Rule>, dim3(B * H, t5_nqt(Lq)), dim3(RH_BLOCK), 0, st, a);
  }
  if (p_drop > 0.f) hipLaunchKernelGGL(drop_advance_kernel, dim3(1), dim3(1), 0, st, rng);
  RH_LAUNCH_CHECK("rh_t5_attn_fwd");
  return 0;
}

extern "C" int rh_t5_attn_bwd(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, int B, int Lq, int Lk,
                              int H, int dh, const uint8_t* key_mask, int causal, const float* bias, const int32_t* bucket,
                              int nb, float p_drop, const int64_t* rng, const int64_t* saved_ctr, const float* out,
                              const float* lse, const float* g_out, float* delta, float* g_q, int64_t ldgq, float* g_k,
                              float* g_v, int64_t ldgkv, float* part, float* g_bias, void* stream) {
  AttnArgs a = t5_args(q, ldq, k, v, ldkv, B, Lq, Lk, H, dh, key_mask, causal, bias, bucket, nb, p_drop, rng, saved_ctr, out, lse);
  attn_bwd_args(a, g_out, delta, g_q, ldgq, g_k, g_v, ldgkv, part, g_bias);
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
    hipLaunchKernelGGL(softmax_attn_delta_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a);
    if (Lq <= kSmallQ) {
      const int g2 = (int)(((int64_t)B * H + kWG - 1) / kWG);
      hipLaunchKernelGGL(t5_attn_small_bwd_kernel, dim3(g2), dim3(RH_BLOCK), 0, st, a);
    } else {
      hipLaunchKernelGGL(softmax_attn_dkv_kernel<T5Rule>, dim3(B * H, (Lk + kT - 1) / kT), dim3(RH_BLOCK), 0, st, a);
      hipLaunchKernelGGL(softmax_attn_dq_kernel<T5Rule>, dim3(B * H, nqt), dim3(RH_BLOCK), 0, st, a);
    }
  }
  if (bias) {
    const int64_t n1 = (int64_t)H * a.nd, n2 = (int64_t)nb * H;
    hipLaunchKernelGGL(softmax_attn_diag_kernel, dim3((int)((n1 + RH_BLOCK - 1) / RH_BLOCK)), dim3(RH_BLOCK), 0, st, a, nqt);
    hipLaunchKernelGGL(softmax_attn_bias_kernel<T5Rule>, dim3((int)((n2 + RH_BLOCK - 1) / RH_BLOCK)), dim3(RH_BLOCK), 0, st, a, nqt);
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
