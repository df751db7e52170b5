// HSTU (generative next-item model): pointwise attention with the relative (position, time-bucket) bias.  The model's
// next-token cross entropy is stream_ce.hip.
//
// Reference HSTULayer.forward torch_rechub/basic/layers.py:908-933 with RelativeBucketedTimeAndPositionBias.forward
// utils/hstu_utils.py:150-185:
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
// The products run on the 64 x 64 MFMA tile of mfma_tile.h.
#include <math.h>

#include "mfma_tile.h"

namespace {

constexpr int kMaxDh = RH_HSTU_MAX_DH;  // dqk, dv
constexpr int kMaxL = RH_HSTU_MAX_L;
constexpr int kMaxBuckets = 1024;  // num_time_buckets + 1
static_assert(kMaxBuckets - 1 == RH_HSTU_MAX_BUCKETS, "the table has num_time_buckets + 1 rows");

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
  load_tile(qs, a.proj, a.ld, qcol, 0, i0, a.L, dqk, b, tid);
  if (tid < kT) tq[tid] = (a.td && i0 + tid < a.L) ? a.td[(int64_t)b * a.L + i0 + tid] : 0;
  v16f o = zero16();
  const float nf = (float)a.N;
  for (int kt = 0; kt <= qt; ++kt) {
    const int j0 = kt * kT;
    __syncthreads();
    load_tile(ks, a.proj, a.ld, kcol, 0, j0, a.L, dqk, b, tid);
    load_tile(vs, a.proj, a.ld, vcol, 0, j0, a.L, dv, b, tid);
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
  load_tile(qs, a.proj, a.ld, kcol, 0, j0, L, dqk, b, tid);
  load_tile(gs, a.proj, a.ld, vcol, 0, j0, L, dv, b, tid);
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
    load_tile(qs, a.proj, a.ld, qcol, 0, i0, L, dqk, b, tid);
    load_tile(gs, a.g_out, ldo, h * dv, 0, i0, L, dv, b, tid);
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
    load_tile(ks, a.proj, a.ld, kcol, 0, j0, L, dqk, b, tid);
    load_tile(vs, a.proj, a.ld, vcol, 0, j0, L, dv, b, tid);
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
