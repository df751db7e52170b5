// Streaming cross entropy over an item table ("the head"): loss, dh, dW and d_bias of z = ((h W^T + b) / t1) / t2 without
// the (M, V) logits.  Two users set its fields:
// - the next-token loss of HSTU and HLLM (rh_hstu_head_*; reference HSTUModel.forward hstu.py:257-271 +
//   SeqTrainer._compute_next_token_loss trainers/seq_trainer.py:177-194 + nn.CrossEntropyLoss / NCELoss): column 0
//   excluded (the reference's logits[..., 0] = -1e9), mean over rows whose label is not 0; a null g_W (HLLM's frozen item
//   table) runs no dW kernel;
// - the full-catalogue cross entropy of NARM / STAMP (rh_catalogue_ce_*; nn.CrossEntropyLoss over u E^T with
//   MatchTrainer(mode=2), reference examples/matching/run_sbr.py): every column and every row counted, no bias, no
//   temperature; B is small next to V there, so the dh kernel splits the item range of each row tile over Sv workgroups.
// The forward streams V tiles per row tile and keeps (max, sum exp) per row and V split; the backward recomputes the
// logits tile by tile, once per (row tile, V range) for dh and once per (V tile, row range) for dW / d_bias.  Partials
// are summed in a fixed order: bitwise reproducible.  The products run on the 64 x 64 MFMA tile of mfma_tile.h.
#include <math.h>

#include "mfma_tile.h"

namespace {

constexpr int kHeadDc = 256;    // dh / dW columns per workgroup

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

// the fields both directions share; catalogue: every column and every row counts (else column 0 and rows labelled 0 do not)
HeadArgs head_args(const float* h, const float* W, const float* bias, const int64_t* labels, int M, int D, int V, float t1,
                   float t2, int catalogue) {
  HeadArgs a{};
  a.h = h;
  a.W = W;
  a.bias = bias;
  a.labels = labels;
  a.M = M;
  a.D = D;
  a.V = V;
  a.t1 = t1;
  a.t2 = t2;
  a.c_lo = catalogue ? 0 : 1;
  a.all_rows = catalogue;
  a.Sv = 1;
  return a;
}

int reduce_grid(int64_t n) {
  const int64_t grid = (n + RH_BLOCK - 1) / RH_BLOCK;
  return grid > 4096 ? 4096 : (int)grid;
}

int head_fwd(const char* name, HeadArgs a, float* part, float* zlab, float* lse, float* wrow, float* loss, int32_t* err,
             void* stream) {
  a.part = part;
  a.zlab = zlab;
  a.lse = lse;
  a.wrow = wrow;
  a.loss = loss;
  a.err = err;
  a.nsplit = rh_hstu_head_nsplit(a.M, a.V);
  if (int rc = head_check(name, a)) return rc;
  RH_REQUIRE(part && zlab && lse && wrow && loss, RH_E_BADARG, "%s: null output", name);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(head_fwd_kernel, dim3((a.M + kT - 1) / kT, a.nsplit), dim3(RH_BLOCK), 0, st, a);
  hipLaunchKernelGGL(head_combine_kernel, dim3(1), dim3(RH_BLOCK), 0, st, a);
  RH_LAUNCH_CHECK(name);
  return 0;
}

// dh over Sv item ranges (summed when Sv > 1), then, unless the table is frozen (null g_W), dW / d_bias over R row ranges
// (summed when R > 1)
int head_bwd(const char* name, const HeadArgs& a, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nrt = (a.M + kT - 1) / kT, nvt = (a.V + kT - 1) / kT, ndc = (a.D + kHeadDc - 1) / kHeadDc;
  hipLaunchKernelGGL(head_dh_kernel, dim3(nrt, ndc, a.Sv), dim3(RH_BLOCK), 0, st, a);
  if (a.Sv > 1)
    hipLaunchKernelGGL(head_dh_reduce_kernel, dim3(reduce_grid((int64_t)a.M * a.D)), dim3(RH_BLOCK), 0, st, a);
  if (a.g_W) hipLaunchKernelGGL(head_dw_kernel, dim3(nvt, ndc, a.R), dim3(RH_BLOCK), 0, st, a);
  if (a.g_W && a.R > 1)
    hipLaunchKernelGGL(head_dw_reduce_kernel, dim3(reduce_grid((int64_t)a.V * (a.D + 1))), dim3(RH_BLOCK), 0, st, a);
  RH_LAUNCH_CHECK(name);
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

extern "C" int rh_catalogue_ce_vsplit(int B, int D, int V) {
  const int nrt = (B + kT - 1) / kT, nvt = (V + kT - 1) / kT, ndc = (D + kHeadDc - 1) / kHeadDc;
  int s = 1;
  while (nrt * ndc * s < 1024 && s * 2 <= nvt && s < 256) s *= 2;
  return s;
}

extern "C" int rh_hstu_head_fwd(const float* h, const float* W, const float* bias, const int64_t* labels, int M, int D, int V,
                                float t1, float t2, int nce, float* part, float* zlab, float* lse, float* wrow, float* loss,
                                int32_t* err, void* stream) {
  HeadArgs a = head_args(h, W, bias, labels, M, D, V, t1, t2, 0);
  a.nce = nce;
  return head_fwd("rh_hstu_head_fwd", a, part, zlab, lse, wrow, loss, err, stream);
}

extern "C" int rh_catalogue_ce_fwd(const float* u, const float* E, const int64_t* labels, int B, int D, int V, float* part,
                                   float* zlab, float* lse, float* wrow, float* loss, int32_t* err, void* stream) {
  RH_REQUIRE(V >= 1 && V <= (1 << 30), RH_E_UNSUPPORTED, "rh_catalogue_ce_fwd: V=%d unsupported (1 <= V <= 2^30)", V);
  return head_fwd("rh_catalogue_ce_fwd", head_args(u, E, nullptr, labels, B, D, V, 1.f, 1.f, 1), part, zlab, lse, wrow, loss,
                  err, stream);
}

extern "C" int rh_hstu_head_bwd(const float* h, const float* W, const float* bias, const int64_t* labels, const float* lse,
                                const float* wrow, const float* g_loss, int M, int D, int V, float t1, float t2, float* part,
                                float* g_h, float* g_W, float* g_bias, void* stream) {
  HeadArgs a = head_args(h, W, bias, labels, M, D, V, t1, t2, 0);
  a.lse = const_cast<float*>(lse);
  a.wrow = const_cast<float*>(wrow);
  a.g_loss = g_loss;
  a.part = part;
  a.g_h = g_h;
  a.g_W = g_W;
  a.g_bias = g_bias;
  a.R = rh_hstu_head_rsplit(M, D, V);
  if (int rc = head_check("rh_hstu_head_bwd", a)) return rc;
  // g_W null: a frozen item table (HLLM) -- no dW kernel runs and no workspace is read
  RH_REQUIRE(lse && wrow && g_loss && g_h && (g_W ? part != nullptr : g_bias == nullptr), RH_E_BADARG,
             "rh_hstu_head_bwd: null pointer");
  return head_bwd("rh_hstu_head_bwd", a, stream);
}

extern "C" int rh_catalogue_ce_bwd(const float* u, const float* E, const int64_t* labels, const float* lse, const float* wrow,
                                   const float* g_loss, int B, int D, int V, float* part, float* part_h, float* g_u, float* g_E,
                                   void* stream) {
  HeadArgs a = head_args(u, E, nullptr, labels, B, D, V, 1.f, 1.f, 1);
  a.lse = const_cast<float*>(lse);
  a.wrow = const_cast<float*>(wrow);
  a.g_loss = g_loss;
  a.part = part;
  a.part_h = part_h;
  a.g_h = g_u;
  a.g_W = g_E;
  a.R = rh_hstu_head_rsplit(B, D, V);
  a.Sv = rh_catalogue_ce_vsplit(B, D, V);
  RH_REQUIRE(V >= 1 && V <= (1 << 30), RH_E_UNSUPPORTED, "rh_catalogue_ce_bwd: V=%d unsupported (1 <= V <= 2^30)", V);
  if (int rc = head_check("rh_catalogue_ce_bwd", a)) return rc;
  RH_REQUIRE(lse && wrow && g_loss && part && g_u && g_E && (a.Sv == 1 || part_h), RH_E_BADARG,
             "rh_catalogue_ce_bwd: null pointer");
  return head_bwd("rh_catalogue_ce_bwd", a, stream);
}
