// HSTU (generative next-item model): pointwise attention with the relative (position, time-bucket) bias, and the
// next-token cross entropy over the item table.
//
// Attention (reference HSTULayer.forward torch_rechub/basic/layers.py:908-933 with
// RelativeBucketedTimeAndPositionBias.forward utils/hstu_utils.py:150-185):
//   A[i, j] = silu(alpha q_i . k_j + pos_w[j - i + N - 1] + ts_w[bucket(t_i - t_j)]) / N   for j <= i and key j kept,
//   A[i, j] = 0 otherwise (the reference's masked entries are silu(-1e4) / N = -0.0),     O = A V.
// The reference materialises the (B, H, L, L) scores, the position gather, the (B, L, L) bucket arithmetic, the
// (B, L, L, H) time-bias gather, the mask, silu and /N in fp32, and again in the backward.  Here one workgroup owns a
// 64-query tile of one (sample, head) and walks the key tiles up to the diagonal (tiles above it are all masked), with
// S, A and the bias formed in registers / LDS only.  No softmax: no running max, no renormalisation.
// Backward (FlashAttention-2 layout, no float atomics): one kernel per key tile owns dK and dV and walks the query
// tiles below it; one kernel per query tile owns dQ and walks the key tiles up to it and also reduces the two bias
// gradients of its tile -- the position gradient by diagonal (lane t owns diagonal t - 63 of each 64 x 64 tile), the
// time-bucket gradient by bucket (lane t owns buckets t, t + 256, ... and scans the tile in order) -- into per-workgroup
// partials that a third kernel sums in workgroup order.  Every output is bitwise reproducible.
// The time bucket is the reference's CPU arithmetic in fp32: (float)(t_i - t_j) -> abs -> [/ 60] -> max(., 1e-6) ->
// sqrt | log -> / divisor -> clamp [0, nb] -> truncate; IEEE division and sqrt, log correctly rounded through double.
//
// Next-token cross entropy (reference HSTUModel.forward hstu.py:257-271 + SeqTrainer._compute_next_token_loss
// trainers/seq_trainer.py:177-194 + nn.CrossEntropyLoss / NCELoss): z = ((h . w_c + b_c) / t1) / t2 over the item table,
// column 0 excluded (the reference's logits[..., 0] = -1e9), mean over rows whose label is not 0.  The forward streams V
// tiles per row tile and keeps (max, sum exp) per row and V split; the backward recomputes the logits tile by tile, once
// per row tile for dh and once per (V tile, row range) for dW / d_bias (partials summed in a fixed order).  The (M, V)
// logits never exist.
//
// All GEMM-shaped work is on v_mfma_f32_32x32x2_f32 (exact f32 products, k-ordered accumulation): a wavefront owns one
// 32 x 32 accumulator; lane (li = lane % 32, kk = lane / 32) feeds A[li][k + kk] and B[k + kk][li], and holds
// C[4 kk + (r & 3) + 8 (r >> 2)][li] in acc[r].
#include <math.h>

#include "common.h"

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kT = 64;          // tile edge (queries, keys, V columns, rows)
constexpr int kLd = kT + 1;     // padded LDS row stride
constexpr int kMaxDh = 64;      // dqk, dv <= 64
constexpr int kMaxL = 1024;
constexpr int kMaxBuckets = 1024;  // num_time_buckets + 1
constexpr int kHeadDc = 256;    // dh / dW columns per workgroup

__device__ __forceinline__ int acc_row(int r, int kk) { return 4 * kk + (r & 3) + 8 * (r >> 2); }

__device__ __forceinline__ v16f zero16() {
  v16f z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// acc += A (32 x K) B (K x 32) with A[i][k] = a[i * ai + k * ak], B[k][j] = b[k * bk + j * bj] (LDS), K even
__device__ __forceinline__ v16f mma_lds(v16f acc, const float* a, int ai, int ak, const float* b, int bk, int bj, int K,
                                        int li, int kk) {
  for (int k = 0; k < K; k += 2) {
    const float av = a[li * ai + (k + kk) * ak];
    const float bv = b[(k + kk) * bk + li * bj];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
  }
  return acc;
}

__device__ __forceinline__ float silu_f(float x) { return x / (1.f + expf(-x)); }
__device__ __forceinline__ float dsilu_f(float x) {
  const float s = 1.f / (1.f + expf(-x));
  return s * (1.f + x * (1.f - s));
}

struct AttnArgs {
  const float* proj;    // (B, L, ld): q at h * dqk, k at H * dqk + h * dqk, v at 2 H dqk + H dv + h * dv
  int64_t ld;
  const int64_t* td;    // (B, L) or null
  const int32_t* kmask; // (B, L) nonzero = kept, or null
  const float* pos_w;   // (2 N - 1, H)
  const float* ts_w;    // (nb + 1, H)
  const float* g_out;   // (B, L, H dv)  backward
  float* out;           // (B, L, H dv)  forward
  float* g_proj;        // (B, L, ld)    backward: q / k / v columns
  float* pos_part;      // (B H nqt, L)  backward
  float* ts_part;       // (B H nqt, nb + 1)
  int B, L, H, dqk, dv, N, nb, fn_log, minutes;
  float divisor, alpha;
};

__device__ __forceinline__ int time_bucket(int64_t ti, int64_t tj, const AttnArgs& a) {
  float dt = fabsf((float)(ti - tj));
  if (a.minutes) dt = dt / 60.0f;
  dt = fmaxf(dt, 1e-6f);
  float v = a.fn_log ? (float)log((double)dt) : sqrtf(dt);
  v = v / a.divisor;
  v = fminf(fmaxf(v, 0.f), (float)a.nb);
  return (int)v;
}

// the bias term of score (i, j), both in range
__device__ __forceinline__ float attn_bias(int i, int j, int h, int64_t ti, int64_t tj, const AttnArgs& a) {
  const float p = a.pos_w[(int64_t)(j - i + a.N - 1) * a.H + h];
  if (!a.td) return p;
  return p + a.ts_w[(int64_t)time_bucket(ti, tj, a) * a.H + h];
}

// loads rows [r0, r0 + 64) x cols [0, d) of one head's slice (column offset col) into s[64][kLd], zero padded to kT
__device__ __forceinline__ void load_tile(float* s, const float* base, int64_t ld, int col, int r0, int L, int d, int b,
                                          int tid) {
  for (int e = tid; e < kT * kT; e += RH_BLOCK) {
    const int r = e / kT, c = e % kT;
    const int row = r0 + r;
    float v = 0.f;
    if (row < L && c < d) v = base[((int64_t)b * L + row) * ld + col + c];
    s[r * kLd + c] = v;
  }
}

__device__ __forceinline__ void load_keys(int64_t* tds, int* kept, const AttnArgs& a, int b, int j0, int tid) {
  if (tid < kT) {
    const int j = j0 + tid;
    tds[tid] = (a.td && j < a.L) ? a.td[(int64_t)b * a.L + j] : 0;
    kept[tid] = j < a.L && (!a.kmask || a.kmask[(int64_t)b * a.L + j] != 0);
  }
}

__global__ __launch_bounds__(RH_BLOCK) void hstu_attn_fwd_kernel(const AttnArgs a) {
  __shared__ float qs[kT * kLd], ks[kT * kLd], vs[kT * kLd];
  __shared__ int64_t tq[kT], tk[kT];
  __shared__ int kept[kT];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int qt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int i0 = qt * kT, H = a.H, dqk = a.dqk, dv = a.dv;
  const int dqk2 = (dqk + 1) & ~1;
  const int qcol = h * dqk, kcol = H * dqk + h * dqk, vcol = 2 * H * dqk + H * dv + h * dv;
  load_tile(qs, a.proj, a.ld, qcol, i0, a.L, dqk, b, tid);
  if (tid < kT) tq[tid] = (a.td && i0 + tid < a.L) ? a.td[(int64_t)b * a.L + i0 + tid] : 0;
  v16f o = zero16();
  const float nf = (float)a.N;
  for (int kt = 0; kt <= qt; ++kt) {
    const int j0 = kt * kT;
    __syncthreads();
    load_tile(ks, a.proj, a.ld, kcol, j0, a.L, dqk, b, tid);
    load_tile(vs, a.proj, a.ld, vcol, j0, a.L, dv, b, tid);
    load_keys(tk, kept, a, b, j0, tid);
    __syncthreads();
    // S quadrant: rows wm * 32 (queries), cols wn * 32 (keys)
    v16f s = mma_lds(zero16(), qs + wm * 32 * kLd, kLd, 1, ks + wn * 32 * kLd, 1, kLd, dqk2, li, kk);
    float p[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int il = wm * 32 + acc_row(r, kk), jl = wn * 32 + li;
      const int i = i0 + il, j = j0 + jl;
      p[r] = 0.f;
      if (i < a.L && j <= i && kept[jl]) {
        const float x = s[r] * a.alpha + attn_bias(i, j, h, tq[il], tk[jl], a);
        p[r] = silu_f(x) / nf;
      }
    }
    __syncthreads();  // every wavefront is done reading ks
#pragma unroll
    for (int r = 0; r < 16; ++r) ks[(wm * 32 + acc_row(r, kk)) * kLd + wn * 32 + li] = p[r];
    __syncthreads();
    // O quadrant: rows wm * 32, dv cols wn * 32;  O += P (64 x 64 keys) V (64 keys x dv)
    if (wn * 32 < dv) o = mma_lds(o, ks + wm * 32 * kLd, kLd, 1, vs + wn * 32, kLd, 1, kT, li, kk);
  }
  const int c = wn * 32 + li;
  if (c < dv) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + wm * 32 + acc_row(r, kk);
      if (i < a.L) a.out[((int64_t)b * a.L + i) * (H * dv) + h * dv + c] = o[r];
    }
  }
}

// dK, dV of one key tile: walks the query tiles at and below the diagonal.
__global__ __launch_bounds__(RH_BLOCK) void hstu_attn_dkv_kernel(const AttnArgs a) {
  __shared__ float qs[kT * kLd], gs[kT * kLd], xs[kT * kLd];
  __shared__ int64_t tq[kT], tk[kT];
  __shared__ int kept[kT];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int kt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int j0 = kt * kT, H = a.H, dqk = a.dqk, dv = a.dv, L = a.L;
  const int dqk2 = (dqk + 1) & ~1, dv2 = (dv + 1) & ~1;
  const int qcol = h * dqk, kcol = H * dqk + h * dqk, vcol = 2 * H * dqk + H * dv + h * dv;
  const int64_t ldo = (int64_t)H * dv;
  const int nqt = (L + kT - 1) / kT;
  // K and V of this tile as B fragments (B[k][j] = K[j][k]) of the wavefront's key half wn, kept in registers
  load_tile(qs, a.proj, a.ld, kcol, j0, L, dqk, b, tid);
  load_tile(gs, a.proj, a.ld, vcol, j0, L, dv, b, tid);
  load_keys(tk, kept, a, b, j0, tid);
  __syncthreads();
  float kf[kMaxDh / 2], vf[kMaxDh / 2];
#pragma unroll
  for (int s = 0; s < kMaxDh / 2; ++s) {
    kf[s] = qs[(wn * 32 + li) * kLd + 2 * s + kk];
    vf[s] = gs[(wn * 32 + li) * kLd + 2 * s + kk];
  }
  v16f dk = zero16(), dvacc = zero16();
  const float nf = (float)a.N;
  for (int qt = kt; qt < nqt; ++qt) {
    const int i0 = qt * kT;
    __syncthreads();
    load_tile(qs, a.proj, a.ld, qcol, i0, L, dqk, b, tid);
    load_tile(gs, a.g_out, ldo, h * dv, i0, L, dv, b, tid);
    if (tid < kT) tq[tid] = (a.td && i0 + tid < L) ? a.td[(int64_t)b * L + i0 + tid] : 0;
    __syncthreads();
    v16f s = zero16(), da = zero16();
#pragma unroll
    for (int k = 0; k < kMaxDh; k += 2)
      if (k < dqk2) s = __builtin_amdgcn_mfma_f32_32x32x2f32(qs[(wm * 32 + li) * kLd + k + kk], kf[k / 2], s, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < kMaxDh; k += 2)
      if (k < dv2) da = __builtin_amdgcn_mfma_f32_32x32x2f32(gs[(wm * 32 + li) * kLd + k + kk], vf[k / 2], da, 0, 0, 0);
    float p[16], ds[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int il = wm * 32 + acc_row(r, kk), jl = wn * 32 + li;
      const int i = i0 + il, j = j0 + jl;
      p[r] = 0.f;
      ds[r] = 0.f;
      if (i < L && j <= i && kept[jl]) {
        const float x = s[r] * a.alpha + attn_bias(i, j, h, tq[il], tk[jl], a);
        p[r] = silu_f(x) / nf;
        ds[r] = da[r] * dsilu_f(x) / nf;
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) xs[(wm * 32 + acc_row(r, kk)) * kLd + wn * 32 + li] = p[r];
    __syncthreads();
    // dV quadrant: keys wm * 32, dv cols wn * 32;  dV += P^T dO  (A[key][i] = xs[i][key])
    if (wn * 32 < dv) dvacc = mma_lds(dvacc, xs + wm * 32, 1, kLd, gs + wn * 32, kLd, 1, kT, li, kk);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) xs[(wm * 32 + acc_row(r, kk)) * kLd + wn * 32 + li] = ds[r];
    __syncthreads();
    // dK quadrant: keys wm * 32, dqk cols wn * 32;  dK += dS^T Q
    if (wn * 32 < dqk) dk = mma_lds(dk, xs + wm * 32, 1, kLd, qs + wn * 32, kLd, 1, kT, li, kk);
  }
  const int c = wn * 32 + li;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int j = j0 + wm * 32 + acc_row(r, kk);
    if (j >= L) continue;
    float* row = a.g_proj + ((int64_t)b * L + j) * a.ld;
    if (c < dqk) row[kcol + c] = dk[r] * a.alpha;
    if (c < dv) row[vcol + c] = dvacc[r];
  }
}

// dQ of one query tile, and this tile's partial sums of the two bias gradients.
__global__ __launch_bounds__(RH_BLOCK) void hstu_attn_dq_kernel(const AttnArgs a) {
  __shared__ float ks[kT * kLd], vs[kT * kLd], xs[kT * kLd];
  __shared__ float pacc[kMaxL], tacc[kMaxBuckets];
  __shared__ int64_t tk[kT];
  __shared__ int kept[kT];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int qt = blockIdx.y, bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int i0 = qt * kT, H = a.H, dqk = a.dqk, dv = a.dv, L = a.L;
  const int dqk2 = (dqk + 1) & ~1, dv2 = (dv + 1) & ~1;
  const int qcol = h * dqk, kcol = H * dqk + h * dqk, vcol = 2 * H * dqk + H * dv + h * dv;
  const int64_t ldo = (int64_t)H * dv;
  const int nb1 = a.nb + 1;
  // Q and dO rows of the wavefront's query half as A fragments, in registers
  float qf[kMaxDh / 2], gf[kMaxDh / 2];
  {
    const int i = i0 + wm * 32 + li;
#pragma unroll
    for (int s = 0; s < kMaxDh / 2; ++s) {
      const int c = 2 * s + kk;
      qf[s] = (i < L && c < dqk) ? a.proj[((int64_t)b * L + i) * a.ld + qcol + c] : 0.f;
      gf[s] = (i < L && c < dv) ? a.g_out[((int64_t)b * L + i) * ldo + h * dv + c] : 0.f;
    }
  }
  // the query times of the accumulator rows this lane holds
  int64_t tqr[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = i0 + wm * 32 + acc_row(r, kk);
    tqr[r] = (a.td && i < L) ? a.td[(int64_t)b * L + i] : 0;
  }
  for (int e = tid; e < L; e += RH_BLOCK) pacc[e] = 0.f;
  if (a.td)
    for (int e = tid; e < nb1; e += RH_BLOCK) tacc[e] = 0.f;
  int* bk = reinterpret_cast<int*>(vs);  // the tile's buckets, once V is consumed
  v16f dq = zero16();
  const float nf = (float)a.N;
  for (int kt = 0; kt <= qt; ++kt) {
    const int j0 = kt * kT;
    __syncthreads();
    load_tile(ks, a.proj, a.ld, kcol, j0, L, dqk, b, tid);
    load_tile(vs, a.proj, a.ld, vcol, j0, L, dv, b, tid);
    load_keys(tk, kept, a, b, j0, tid);
    __syncthreads();
    v16f s = zero16(), da = zero16();
#pragma unroll
    for (int k = 0; k < kMaxDh; k += 2)
      if (k < dqk2) s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[k / 2], ks[(wn * 32 + li) * kLd + k + kk], s, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < kMaxDh; k += 2)
      if (k < dv2) da = __builtin_amdgcn_mfma_f32_32x32x2f32(gf[k / 2], vs[(wn * 32 + li) * kLd + k + kk], da, 0, 0, 0);
    float ds[16];
    int bkt[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int il = wm * 32 + acc_row(r, kk), jl = wn * 32 + li;
      const int i = i0 + il, j = j0 + jl;
      ds[r] = 0.f;
      bkt[r] = -1;
      if (i < L && j <= i && kept[jl]) {
        float bias = a.pos_w[(int64_t)(j - i + a.N - 1) * H + h];
        if (a.td) {
          bkt[r] = time_bucket(tqr[r], tk[jl], a);
          bias += a.ts_w[(int64_t)bkt[r] * H + h];
        }
        const float x = s[r] * a.alpha + bias;
        ds[r] = da[r] * dsilu_f(x) / nf;
      }
    }
    __syncthreads();  // every wavefront is done reading vs
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int e = (wm * 32 + acc_row(r, kk)) * kLd + wn * 32 + li;
      xs[e] = ds[r];
      bk[e] = bkt[r];
    }
    __syncthreads();
    // dQ quadrant: queries wm * 32, dqk cols wn * 32;  dQ += dS K
    if (wn * 32 < dqk) dq = mma_lds(dq, xs + wm * 32 * kLd, kLd, 1, ks + wn * 32, kLd, 1, kT, li, kk);
    // position gradient: lane t < 127 owns the tile diagonal il - jl = t - 63, i.e. i - j = i0 - j0 + t - 63
    if (tid < 2 * kT - 1) {
      const int e = tid - (kT - 1);
      const int d = i0 - j0 + e;
      if (d >= 0 && d < L) {
        float sum = 0.f;
        for (int il = e > 0 ? e : 0; il < kT && il - e < kT; ++il) sum += xs[il * kLd + il - e];
        pacc[d] += sum;
      }
    }
    // time-bucket gradient: lane t owns buckets t, t + 256, ... and scans the tile in row-major order
    if (a.td) {
      for (int c = tid; c < nb1; c += RH_BLOCK) {
        float sum = 0.f;
        for (int il = 0; il < kT; ++il)
          for (int jl = 0; jl < kT; ++jl)
            if (bk[il * kLd + jl] == c) sum += xs[il * kLd + jl];
        tacc[c] += sum;
      }
    }
  }
  const int c = wn * 32 + li;
  if (c < dqk) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + wm * 32 + acc_row(r, kk);
      if (i < L) a.g_proj[((int64_t)b * L + i) * a.ld + qcol + c] = dq[r] * a.alpha;
    }
  }
  __syncthreads();
  const int64_t part = (int64_t)bh * gridDim.y + qt;
  for (int e = tid; e < L; e += RH_BLOCK) a.pos_part[part * L + e] = pacc[e];
  if (a.td)
    for (int e = tid; e < nb1; e += RH_BLOCK) a.ts_part[part * nb1 + e] = tacc[e];
}

// d pos_w[(N - 1 - d), h] = sum over (b, query tile) of the diagonal-d partials of head h; d ts_w[c, h] likewise
__global__ __launch_bounds__(RH_BLOCK) void hstu_bias_reduce_kernel(const AttnArgs a, int nqt, float* g_pos, float* g_ts) {
  const int npos = 2 * a.N - 1, nb1 = a.nb + 1;
  const int64_t total = (int64_t)(npos + nb1) * a.H;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * RH_BLOCK) {
    const int h = (int)(e % a.H);
    const int64_t row = e / a.H;
    float sum = 0.f;
    if (row < npos) {
      const int d = a.N - 1 - (int)row;
      if (d >= 0 && d < a.L)
        for (int b = 0; b < a.B; ++b)
          for (int q = 0; q < nqt; ++q) sum += a.pos_part[(((int64_t)b * a.H + h) * nqt + q) * a.L + d];
      g_pos[row * a.H + h] = sum;
    } else {
      const int c = (int)(row - npos);
      if (a.td)
        for (int b = 0; b < a.B; ++b)
          for (int q = 0; q < nqt; ++q) sum += a.ts_part[(((int64_t)b * a.H + h) * nqt + q) * nb1 + c];
      g_ts[(int64_t)c * a.H + h] = sum;
    }
  }
}

}  // namespace

static int attn_check(const char* name, const AttnArgs& a) {
  RH_REQUIRE(a.proj && a.pos_w && a.ts_w, RH_E_BADARG, "%s: null pointer", name);
  RH_REQUIRE(a.B >= 0 && a.H >= 1 && a.L >= 1 && a.L <= kMaxL && a.L <= a.N, RH_E_UNSUPPORTED,
             "%s: L=%d unsupported (1 <= L <= min(max_seq_len=%d, %d))", name, a.L, a.N, kMaxL);
  RH_REQUIRE(a.dqk >= 1 && a.dqk <= kMaxDh && a.dv >= 1 && a.dv <= kMaxDh, RH_E_UNSUPPORTED,
             "%s: dqk=%d dv=%d unsupported (each in [1, %d])", name, a.dqk, a.dv, kMaxDh);
  RH_REQUIRE(a.nb >= 0 && a.nb + 1 <= kMaxBuckets, RH_E_UNSUPPORTED, "%s: num_time_buckets=%d unsupported (<= %d)", name,
             a.nb, kMaxBuckets - 1);
  RH_REQUIRE(a.ld >= 2 * (int64_t)a.H * (a.dqk + a.dv), RH_E_BADARG, "%s: row stride %lld too small", name, (long long)a.ld);
  RH_REQUIRE(a.divisor != 0.f, RH_E_BADARG, "%s: time_bucket_divisor must be nonzero", name);
  return 0;
}

static AttnArgs attn_args(const float* proj, int64_t ld, int B, int L, int H, int dqk, int dv, const int64_t* td,
                          const int32_t* kmask, const float* pos_w, const float* ts_w, int N, int nb, int fn_log, int minutes,
                          float divisor, float alpha) {
  AttnArgs a{};
  a.proj = proj;
  a.ld = ld;
  a.td = td;
  a.kmask = kmask;
  a.pos_w = pos_w;
  a.ts_w = ts_w;
  a.B = B;
  a.L = L;
  a.H = H;
  a.dqk = dqk;
  a.dv = dv;
  a.N = N;
  a.nb = nb;
  a.fn_log = fn_log;
  a.minutes = minutes;
  a.divisor = divisor;
  a.alpha = alpha;
  return a;
}

extern "C" int rh_hstu_attn_nparts(int B, int L, int H) { return B * H * ((L + kT - 1) / kT); }

extern "C" int rh_hstu_attn_fwd(const float* proj, int64_t ld, int B, int L, int H, int dqk, int dv, const int64_t* td,
                                const int32_t* kmask, const float* pos_w, const float* ts_w, int N, int nb, int fn_log,
                                int minutes, float divisor, float alpha, float* out, void* stream) {
  AttnArgs a = attn_args(proj, ld, B, L, H, dqk, dv, td, kmask, pos_w, ts_w, N, nb, fn_log, minutes, divisor, alpha);
  a.out = out;
  if (int rc = attn_check("rh_hstu_attn_fwd", a)) return rc;
  RH_REQUIRE(out, RH_E_BADARG, "rh_hstu_attn_fwd: null output");
  if (B == 0) return 0;
  const int nqt = (L + kT - 1) / kT;
  hipLaunchKernelGGL(hstu_attn_fwd_kernel, dim3(B * H, nqt), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_hstu_attn_fwd");
  return 0;
}

extern "C" int rh_hstu_attn_bwd(const float* proj, int64_t ld, int B, int L, int H, int dqk, int dv, const int64_t* td,
                                const int32_t* kmask, const float* pos_w, const float* ts_w, int N, int nb, int fn_log,
                                int minutes, float divisor, float alpha, const float* g_out, float* g_proj, float* pos_part,
                                float* ts_part, float* g_pos_w, float* g_ts_w, void* stream) {
  AttnArgs a = attn_args(proj, ld, B, L, H, dqk, dv, td, kmask, pos_w, ts_w, N, nb, fn_log, minutes, divisor, alpha);
  a.g_out = g_out;
  a.g_proj = g_proj;
  a.pos_part = pos_part;
  a.ts_part = ts_part;
  if (int rc = attn_check("rh_hstu_attn_bwd", a)) return rc;
  RH_REQUIRE(g_out && g_proj && pos_part && g_pos_w && g_ts_w && (!td || ts_part), RH_E_BADARG,
             "rh_hstu_attn_bwd: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nqt = (L + kT - 1) / kT;
  if (B > 0) {
    hipLaunchKernelGGL(hstu_attn_dkv_kernel, dim3(B * H, nqt), dim3(RH_BLOCK), 0, st, a);
    hipLaunchKernelGGL(hstu_attn_dq_kernel, dim3(B * H, nqt), dim3(RH_BLOCK), 0, st, a);
  }
  const int64_t total = (int64_t)(2 * N - 1 + nb + 1) * H;
  int grid = (int)((total + RH_BLOCK - 1) / RH_BLOCK);
  hipLaunchKernelGGL(hstu_bias_reduce_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a, nqt, g_pos_w, g_ts_w);
  RH_LAUNCH_CHECK("rh_hstu_attn_bwd");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Next-token cross entropy over the item table.
namespace {

struct HeadArgs {
  const float* h;        // (M, D) contiguous
  const float* W;        // (V, D) contiguous
  const float* bias;     // (V,) or null
  const int64_t* labels; // (M,)
  float* part;           // fwd: (M, nsplit, 2) per-split (max, sum exp); bwd: (R, V, D + 1) dW / d_bias partials
  float* zlab;           // (M,) the label's logit
  float* lse;            // (M,)
  float* wrow;           // (M,) gradient weight of the row in the mean
  float* loss;           // (1,)
  int32_t* err;          // (1,) error word or null
  const float* g_loss;   // (1,) device
  float* g_h;            // (M, D)
  float* g_W;            // (V, D)
  float* g_bias;         // (V,) or null
  int M, D, V, nsplit, nce, R;
  float t1, t2;
  int c_lo;              // first column that counts: 1 (HSTU: column 0 excluded) or 0 (catalogue: every column)
  int all_rows;          // 1: every row counts (catalogue); 0: rows labelled 0 are ignored (HSTU)
  int Sv;                // dh: V ranges per row tile; > 1 writes per-range partials to part_h
  float* part_h;         // (Sv, M, D) dh partials or null
};

// z tile (64 rows r0.. x 64 columns c0..) of the wavefront's quadrant; hs / ws are (64 x 64 + pad) LDS staging
__device__ __forceinline__ v16f head_logits(const HeadArgs& a, int r0, int c0, float* hs, float* ws, int tid, int li, int kk,
                                            int wm, int wn) {
  v16f acc = zero16();
  for (int k0 = 0; k0 < a.D; k0 += kT) {
    __syncthreads();
    for (int e = tid; e < kT * kT; e += RH_BLOCK) {
      const int r = e / kT, c = e % kT, k = k0 + c;
      hs[r * kLd + c] = (r0 + r < a.M && k < a.D) ? a.h[(int64_t)(r0 + r) * a.D + k] : 0.f;
      ws[r * kLd + c] = (c0 + r < a.V && k < a.D) ? a.W[(int64_t)(c0 + r) * a.D + k] : 0.f;
    }
    __syncthreads();
    acc = mma_lds(acc, hs + wm * 32 * kLd, kLd, 1, ws + wn * 32 * kLd, 1, kLd, kT, li, kk);
  }
  return acc;
}

__device__ __forceinline__ float head_z(const HeadArgs& a, float acc, int c) {
  const float b = a.bias ? a.bias[c] : 0.f;
  return ((acc + b) / a.t1) / a.t2;
}

__global__ __launch_bounds__(RH_BLOCK) void head_fwd_kernel(const HeadArgs a) {
  __shared__ float hs[kT * kLd], ws[kT * kLd];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int r0 = blockIdx.x * kT, split = blockIdx.y;
  const int nvt = (a.V + kT - 1) / kT;
  const int t_lo = (int)((int64_t)nvt * split / a.nsplit), t_hi = (int)((int64_t)nvt * (split + 1) / a.nsplit);
  // running (max, sum) of row tid / 4 over its 16-column quarter of every tile; the 4 lanes of a row agree after combining
  const int row = tid / 4, part = tid % 4;
  const int64_t grow = (int64_t)r0 + row;
  const int64_t lab = grow < a.M ? a.labels[grow] : 0;
  if (part == 0 && (lab < 0 || lab >= a.V) && a.err != nullptr) atomicOr(a.err, RH_FLAG_TARGET_OOB);
  float rm = -INFINITY, rs = 0.f;
  for (int t = t_lo; t < t_hi; ++t) {
    const int c0 = t * kT;
    v16f acc = head_logits(a, r0, c0, hs, ws, tid, li, kk, wm, wn);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = c0 + wn * 32 + li;
      hs[(wm * 32 + acc_row(r, kk)) * kLd + wn * 32 + li] = (c >= a.c_lo && c < a.V) ? head_z(a, acc[r], c) : -INFINITY;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int q = 0; q < 16; ++q) m = fmaxf(m, hs[row * kLd + part * 16 + q]);
    m = fmaxf(m, __shfl_xor(m, 1, RH_WAVE));
    m = fmaxf(m, __shfl_xor(m, 2, RH_WAVE));
    if (m > -INFINITY) {
      float s = 0.f;
      for (int q = 0; q < 16; ++q) s += expf(hs[row * kLd + part * 16 + q] - m);
      s += __shfl_xor(s, 1, RH_WAVE);
      s += __shfl_xor(s, 2, RH_WAVE);
      const float nm = fmaxf(rm, m);
      rs = rs * expf(rm - nm) + s * expf(m - nm);
      rm = nm;
    }
    if (lab >= c0 + part * 16 && lab < c0 + part * 16 + 16 && lab >= a.c_lo && lab < a.V && grow < a.M)
      a.zlab[grow] = hs[row * kLd + (int)(lab - c0)];
  }
  if (part == 0 && grow < a.M) {
    a.part[(grow * a.nsplit + split) * 2 + 0] = rm;
    a.part[(grow * a.nsplit + split) * 2 + 1] = rs;
  }
}

// one workgroup: per-row log-sum-exp, row weights and the mean loss, in a fixed order
__global__ __launch_bounds__(RH_BLOCK) void head_combine_kernel(const HeadArgs a) {
  __shared__ float red_l[RH_BLOCK], red_a[RH_BLOCK];
  __shared__ int red_n[RH_BLOCK];
  const int tid = threadIdx.x;
  const float z0 = -1e9f / a.t2;
  float sl = 0.f, sa = 0.f;
  int n = 0;
  for (int r = tid; r < a.M; r += RH_BLOCK) {
    float m = -INFINITY;
    for (int s = 0; s < a.nsplit; ++s) m = fmaxf(m, a.part[((int64_t)r * a.nsplit + s) * 2]);
    float sum = 0.f;
    for (int s = 0; s < a.nsplit; ++s) {
      const float ms = a.part[((int64_t)r * a.nsplit + s) * 2];
      if (ms > -INFINITY) sum += a.part[((int64_t)r * a.nsplit + s) * 2 + 1] * expf(ms - m);
    }
    const float l = m + logf(sum);
    a.lse[r] = l;
    const int64_t lab = a.labels[r];
    if (a.all_rows || lab != 0) {
      sl += l - a.zlab[r];
      ++n;
    }
    sa += l - z0;
  }
  red_l[tid] = sl;
  red_a[tid] = sa;
  red_n[tid] = n;
  __syncthreads();
  for (int o = RH_BLOCK / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red_l[tid] += red_l[tid + o];
      red_a[tid] += red_a[tid + o];
      red_n[tid] += red_n[tid + o];
    }
    __syncthreads();
  }
  const int cnt = red_n[0];
  // nn.CrossEntropyLoss: 0 / 0 = NaN with every row ignored; NCELoss: then the mean over every row
  const bool all_rows = cnt == 0 && a.nce;
  for (int r = tid; r < a.M; r += RH_BLOCK)
    a.wrow[r] = all_rows ? 1.f / (float)a.M : ((a.all_rows || a.labels[r] != 0) ? 1.f / (float)cnt : 0.f);
  if (tid == 0) a.loss[0] = all_rows ? red_a[0] / (float)a.M : red_l[0] / (float)cnt;
}

// d logit (before the temperatures) of the wavefront's quadrant: g w_r (softmax - onehot) / t2 / t1, column 0 zero
__device__ __forceinline__ void head_dz(const HeadArgs& a, const v16f& acc, int r0, int c0, int wm, int wn, int li, int kk,
                                        float g, float* out) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = (int64_t)r0 + wm * 32 + acc_row(r, kk);
    const int c = c0 + wn * 32 + li;
    float d = 0.f;
    if (row < a.M && c >= a.c_lo && c < a.V) {
      const float p = expf(head_z(a, acc[r], c) - a.lse[row]);
      const float y = a.labels[row] == c ? 1.f : 0.f;
      d = ((g * a.wrow[row] * (p - y)) / a.t2) / a.t1;
    }
    out[r] = d;
  }
}

// dh for rows [r0, r0 + 64) and columns [d0, d0 + kHeadDc): wavefront w owns quadrants (w & 1, w >> 1 + 2 q)
__global__ __launch_bounds__(RH_BLOCK) void head_dh_kernel(const HeadArgs a) {
  __shared__ float hs[kT * kLd], ws[kT * kLd], gz[kT * kLd];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int r0 = blockIdx.x * kT, d0 = blockIdx.y * kHeadDc;
  const float g = a.g_loss[0];
  v16f acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = zero16();
  const int nvt = (a.V + kT - 1) / kT;
  const int vs = blockIdx.z;
  const int t_lo = a.Sv > 1 ? (int)((int64_t)nvt * vs / a.Sv) : 0;
  const int t_hi = a.Sv > 1 ? (int)((int64_t)nvt * (vs + 1) / a.Sv) : nvt;
  for (int t = t_lo; t < t_hi; ++t) {
    const int c0 = t * kT;
    v16f z = head_logits(a, r0, c0, hs, ws, tid, li, kk, wm, wn);
    float d[16];
    head_dz(a, z, r0, c0, wm, wn, li, kk, g, d);
#pragma unroll
    for (int r = 0; r < 16; ++r) gz[(wm * 32 + acc_row(r, kk)) * kLd + wn * 32 + li] = d[r];
    // dh[:, d0 + 64 j + ...] += dz (64 x 64 items) W[c0.., d0 + 64 j ..]: W chunks of 64 columns through ws
#pragma unroll
    for (int j = 0; j < kHeadDc / kT; ++j) {
      if (d0 + j * kT >= a.D) break;
      __syncthreads();
      for (int e = tid; e < kT * kT; e += RH_BLOCK) {
        const int r = e / kT, c = e % kT, k = d0 + j * kT + c;
        ws[r * kLd + c] = (c0 + r < a.V && k < a.D) ? a.W[(int64_t)(c0 + r) * a.D + k] : 0.f;
      }
      __syncthreads();
      // quadrant (wm, 2 j + wn'): wavefront w handles column half wn of chunk j
      acc[j] = mma_lds(acc[j], gz + wm * 32 * kLd, kLd, 1, ws + wn * 32, kLd, 1, kT, li, kk);
    }
  }
#pragma unroll
  for (int j = 0; j < kHeadDc / kT; ++j) {
    const int c = d0 + j * kT + wn * 32 + li;
    if (c >= a.D) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = (int64_t)r0 + wm * 32 + acc_row(r, kk);
      if (row < a.M) {
        if (a.Sv > 1) a.part_h[((int64_t)vs * a.M + row) * a.D + c] = acc[j][r];
        else a.g_h[row * a.D + c] = acc[j][r];
      }
    }
  }
}

// dW / d_bias partials for item columns [c0, c0 + 64), hidden columns [d0, d0 + kHeadDc), rows of range blockIdx.z
__global__ __launch_bounds__(RH_BLOCK) void head_dw_kernel(const HeadArgs a) {
  __shared__ float hs[kT * kLd], ws[kT * kLd], gz[kT * kLd];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int li = lane % 32, kk = lane / 32, wm = w & 1, wn = w >> 1;
  const int c0 = blockIdx.x * kT, d0 = blockIdx.y * kHeadDc, rr = blockIdx.z;
  const float g = a.g_loss[0];
  const int nrt = (a.M + kT - 1) / kT;
  const int t_lo = (int)((int64_t)nrt * rr / a.R), t_hi = (int)((int64_t)nrt * (rr + 1) / a.R);
  v16f acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = zero16();
  float bsum = 0.f;  // lane tid < 64: column c0 + tid of d_bias
  for (int t = t_lo; t < t_hi; ++t) {
    const int r0 = t * kT;
    v16f z = head_logits(a, r0, c0, hs, ws, tid, li, kk, wm, wn);
    float d[16];
    head_dz(a, z, r0, c0, wm, wn, li, kk, g, d);
#pragma unroll
    for (int r = 0; r < 16; ++r) gz[(wm * 32 + acc_row(r, kk)) * kLd + wn * 32 + li] = d[r];
    __syncthreads();
    if (tid < kT)
      for (int r = 0; r < kT; ++r) bsum += gz[r * kLd + tid];
#pragma unroll
    for (int j = 0; j < kHeadDc / kT; ++j) {
      if (d0 + j * kT >= a.D) break;
      __syncthreads();
      for (int e = tid; e < kT * kT; e += RH_BLOCK) {
        const int r = e / kT, c = e % kT, k = d0 + j * kT + c;
        hs[r * kLd + c] = (r0 + r < a.M && k < a.D) ? a.h[(int64_t)(r0 + r) * a.D + k] : 0.f;
      }
      __syncthreads();
      // dW quadrant (items wm * 32, hidden wn * 32 of chunk j) += dz^T h   (A[item][row] = gz[row][item])
      acc[j] = mma_lds(acc[j], gz + wm * 32, 1, kLd, hs + wn * 32, kLd, 1, kT, li, kk);
    }
  }
  // R == 1: straight into dW / d_bias; else partial slab rr (V, D + 1), d_bias in the last column
  const bool direct = a.R == 1;
  float* slab = a.part + (int64_t)rr * a.V * (a.D + 1);
  const int64_t lds = direct ? a.D : a.D + 1;
  float* dst = direct ? a.g_W : slab;
#pragma unroll
  for (int j = 0; j < kHeadDc / kT; ++j) {
    const int c = d0 + j * kT + wn * 32 + li;
    if (c >= a.D) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int item = c0 + wm * 32 + acc_row(r, kk);
      if (item < a.V) dst[(int64_t)item * lds + c] = acc[j][r];
    }
  }
  if (blockIdx.y == 0 && tid < kT && c0 + tid < a.V) {
    if (!direct) slab[(int64_t)(c0 + tid) * (a.D + 1) + a.D] = bsum;
    else if (a.g_bias) a.g_bias[c0 + tid] = bsum;
  }
}

// dW, d_bias = sum of the R slabs in slab order
__global__ __launch_bounds__(RH_BLOCK) void head_dw_reduce_kernel(const HeadArgs a) {
  const int64_t n = (int64_t)a.V * (a.D + 1);
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    float s = 0.f;
    for (int r = 0; r < a.R; ++r) s += a.part[(int64_t)r * n + e];
    const int64_t item = e / (a.D + 1);
    const int c = (int)(e % (a.D + 1));
    if (c < a.D) a.g_W[item * a.D + c] = s;
    else if (a.g_bias) a.g_bias[item] = s;
  }
}

// dh = sum of the Sv per-range partials in range order
__global__ __launch_bounds__(RH_BLOCK) void head_dh_reduce_kernel(const HeadArgs a) {
  const int64_t n = (int64_t)a.M * a.D;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    float s = 0.f;
    for (int v = 0; v < a.Sv; ++v) s += a.part_h[(int64_t)v * n + e];
    a.g_h[e] = s;
  }
}

int head_check(const char* name, const HeadArgs& a) {
  RH_REQUIRE(a.h && a.W && a.labels, RH_E_BADARG, "%s: null pointer", name);
  RH_REQUIRE(a.M >= 1 && a.D >= 1 && a.V >= 2 && a.t1 > 0.f && a.t2 > 0.f, RH_E_BADARG,
             "%s: M=%d D=%d V=%d t1=%g t2=%g unsupported (M >= 1, D >= 1, V >= 2, temperatures > 0)", name, a.M, a.D, a.V,
             (double)a.t1, (double)a.t2);
  return 0;
}

}  // namespace

extern "C" int rh_hstu_head_nsplit(int M, int V) {
  const int nrt = (M + kT - 1) / kT, nvt = (V + kT - 1) / kT;
  int s = 1;
  while (nrt * s < 1024 && s * 2 <= nvt && s < 64) s *= 2;
  return s;
}

extern "C" int rh_hstu_head_rsplit(int M, int D, int V) {
  const int nrt = (M + kT - 1) / kT, nvt = (V + kT - 1) / kT, ndc = (D + kHeadDc - 1) / kHeadDc;
  int r = 1;
  while (nvt * ndc * r < 1024 && r * 2 <= nrt && r < 32) r *= 2;
  return r;
}

extern "C" int rh_hstu_head_fwd(const float* h, const float* W, const float* bias, const int64_t* labels, int M, int D, int V,
                                float t1, float t2, int nce, float* part, float* zlab, float* lse, float* wrow, float* loss,
                                int32_t* err, void* stream) {
  HeadArgs a{};
  a.h = h;
  a.W = W;
  a.bias = bias;
  a.labels = labels;
  a.part = part;
  a.zlab = zlab;
  a.lse = lse;
  a.wrow = wrow;
  a.loss = loss;
  a.err = err;
  a.M = M;
  a.D = D;
  a.V = V;
  a.t1 = t1;
  a.t2 = t2;
  a.nce = nce;
  a.c_lo = 1;
  a.nsplit = rh_hstu_head_nsplit(M, V);
  if (int rc = head_check("rh_hstu_head_fwd", a)) return rc;
  RH_REQUIRE(part && zlab && lse && wrow && loss, RH_E_BADARG, "rh_hstu_head_fwd: null output");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(head_fwd_kernel, dim3((M + kT - 1) / kT, a.nsplit), dim3(RH_BLOCK), 0, st, a);
  hipLaunchKernelGGL(head_combine_kernel, dim3(1), dim3(RH_BLOCK), 0, st, a);
  RH_LAUNCH_CHECK("rh_hstu_head_fwd");
  return 0;
}

extern "C" int rh_hstu_head_bwd(const float* h, const float* W, const float* bias, const int64_t* labels, const float* lse,
                                const float* wrow, const float* g_loss, int M, int D, int V, float t1, float t2, float* part,
                                float* g_h, float* g_W, float* g_bias, void* stream) {
  HeadArgs a{};
  a.h = h;
  a.W = W;
  a.bias = bias;
  a.labels = labels;
  a.lse = const_cast<float*>(lse);
  a.wrow = const_cast<float*>(wrow);
  a.g_loss = g_loss;
  a.part = part;
  a.g_h = g_h;
  a.g_W = g_W;
  a.g_bias = g_bias;
  a.M = M;
  a.D = D;
  a.V = V;
  a.t1 = t1;
  a.t2 = t2;
  a.R = rh_hstu_head_rsplit(M, D, V);
  a.c_lo = 1;
  a.Sv = 1;
  if (int rc = head_check("rh_hstu_head_bwd", a)) return rc;
  // g_W null: a frozen item table (HLLM) -- no dW kernel runs and no workspace is read
  RH_REQUIRE(lse && wrow && g_loss && g_h && (g_W ? part != nullptr : g_bias == nullptr), RH_E_BADARG,
             "rh_hstu_head_bwd: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nrt = (M + kT - 1) / kT, nvt = (V + kT - 1) / kT, ndc = (D + kHeadDc - 1) / kHeadDc;
  hipLaunchKernelGGL(head_dh_kernel, dim3(nrt, ndc), dim3(RH_BLOCK), 0, st, a);
  if (g_W) hipLaunchKernelGGL(head_dw_kernel, dim3(nvt, ndc, a.R), dim3(RH_BLOCK), 0, st, a);
  if (g_W && a.R > 1) {
    const int64_t n = (int64_t)V * (D + 1);
    int grid = (int)((n + RH_BLOCK - 1) / RH_BLOCK);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(head_dw_reduce_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a);
  }
  RH_LAUNCH_CHECK("rh_hstu_head_bwd");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Full-catalogue cross entropy (NARM / STAMP with MatchTrainer(mode=2): nn.CrossEntropyLoss over u E^T, reference
// examples/matching/run_sbr.py): the same streaming head with every column and every row counted, no bias, no
// temperature.  The backward splits the item range of each row tile over Sv workgroups (B is small next to V here) and
// sums their dh partials in range order.

extern "C" int rh_catalogue_ce_vsplit(int B, int D, int V) {
  const int nrt = (B + kT - 1) / kT, nvt = (V + kT - 1) / kT, ndc = (D + kHeadDc - 1) / kHeadDc;
  int s = 1;
  while (nrt * ndc * s < 1024 && s * 2 <= nvt && s < 256) s *= 2;
  return s;
}

extern "C" int rh_catalogue_ce_fwd(const float* u, const float* E, const int64_t* labels, int B, int D, int V, float* part,
                                   float* zlab, float* lse, float* wrow, float* loss, int32_t* err, void* stream) {
  HeadArgs a{};
  a.h = u;
  a.W = E;
  a.labels = labels;
  a.part = part;
  a.zlab = zlab;
  a.lse = lse;
  a.wrow = wrow;
  a.loss = loss;
  a.err = err;
  a.M = B;
  a.D = D;
  a.V = V;
  a.t1 = 1.f;
  a.t2 = 1.f;
  a.c_lo = 0;
  a.all_rows = 1;
  a.nsplit = rh_hstu_head_nsplit(B, V);
  RH_REQUIRE(V >= 1 && V <= (1 << 30), RH_E_UNSUPPORTED, "rh_catalogue_ce_fwd: V=%d unsupported (1 <= V <= 2^30)", V);
  if (int rc = head_check("rh_catalogue_ce_fwd", a)) return rc;
  RH_REQUIRE(part && zlab && lse && wrow && loss, RH_E_BADARG, "rh_catalogue_ce_fwd: null output");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(head_fwd_kernel, dim3((B + kT - 1) / kT, a.nsplit), dim3(RH_BLOCK), 0, st, a);
  hipLaunchKernelGGL(head_combine_kernel, dim3(1), dim3(RH_BLOCK), 0, st, a);
  RH_LAUNCH_CHECK("rh_catalogue_ce_fwd");
  return 0;
}

extern "C" int rh_catalogue_ce_bwd(const float* u, const float* E, const int64_t* labels, const float* lse, const float* wrow,
                                   const float* g_loss, int B, int D, int V, float* part, float* part_h, float* g_u, float* g_E,
                                   void* stream) {
  HeadArgs a{};
  a.h = u;
  a.W = E;
  a.labels = labels;
  a.lse = const_cast<float*>(lse);
  a.wrow = const_cast<float*>(wrow);
  a.g_loss = g_loss;
  a.part = part;
  a.part_h = part_h;
  a.g_h = g_u;
  a.g_W = g_E;
  a.M = B;
  a.D = D;
  a.V = V;
  a.t1 = 1.f;
  a.t2 = 1.f;
  a.c_lo = 0;
  a.all_rows = 1;
  a.R = rh_hstu_head_rsplit(B, D, V);
  a.Sv = rh_catalogue_ce_vsplit(B, D, V);
  RH_REQUIRE(V >= 1 && V <= (1 << 30), RH_E_UNSUPPORTED, "rh_catalogue_ce_bwd: V=%d unsupported (1 <= V <= 2^30)", V);
  if (int rc = head_check("rh_catalogue_ce_bwd", a)) return rc;
  RH_REQUIRE(lse && wrow && g_loss && part && g_u && g_E && (a.Sv == 1 || part_h), RH_E_BADARG,
             "rh_catalogue_ce_bwd: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nrt = (B + kT - 1) / kT, nvt = (V + kT - 1) / kT, ndc = (D + kHeadDc - 1) / kHeadDc;
  hipLaunchKernelGGL(head_dh_kernel, dim3(nrt, ndc, a.Sv), dim3(RH_BLOCK), 0, st, a);
  if (a.Sv > 1) {
    const int64_t n = (int64_t)B * D;
    int grid = (int)((n + RH_BLOCK - 1) / RH_BLOCK);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(head_dh_reduce_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a);
  }
  hipLaunchKernelGGL(head_dw_kernel, dim3(nvt, ndc, a.R), dim3(RH_BLOCK), 0, st, a);
  if (a.R > 1) {
    const int64_t n = (int64_t)V * (D + 1);
    int grid = (int)((n + RH_BLOCK - 1) / RH_BLOCK);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(head_dw_reduce_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a);
  }
  RH_LAUNCH_CHECK("rh_catalogue_ce_bwd");
  return 0;
}
