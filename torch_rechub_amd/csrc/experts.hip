// Expert banks of the multi-task models (MMOE, PLE's CGC levels): G same-depth [Linear, BatchNorm1d, ReLU, Dropout] stacks
// and the softmax gates (Linear, BatchNorm1d, Softmax) that read the same input streams, all over the batch dimension M.
// A bank layer lives in ONE wide (M, C) buffer, C = sum N_g: group g owns the column block [col0_g, col0_g + N_g), so no
// stack / cat is ever formed and every pass below is one launch for all groups.
//
//   forward   experts_fwd_kernel   grouped GEMM z[:, block g] = x_s(g) W_g^T + b_g, 128 x 32 tiles on v_mfma_f32_32x32x2_f32,
//                                  + per-slab (sum, M2) of every wide column
//             bn_fwd_kernel        slabs -> stat (mean, rstd, gamma, beta, kind per wide column), running statistics
//             act_fwd_kernel       hidden layers: a = dropout(relu(bn(z)))
//             mix_fwd_kernel       out_o = sum_e softmax(bn(zgate_o))[e] dropout(relu(bn(z_sel_o[e]))), applied on load
//   backward  mix_bwd_kernel       -> gradient w.r.t. every BatchNorm output (experts: summed over the outputs in output
//                                  order; gates: softmax backward) + per-16-row-slab (sum g, sum g xhat)
//             act_bwd_kernel       hidden layers: ReLU / mask on the dgrad's output, in place, + the same slab sums
//             bn_bwd_fin / _apply  slab sums -> (dgamma, dbeta); buffer -> gradient w.r.t. z, in place
//             experts_dgrad_kernel gx_s = sum_{g of stream s} gz[:, block g] W_g, the sum over the groups carried in the
//                                  accumulator (fixed order)
// fp32 throughout, no atomics, every sum in a fixed order: two runs give the same bits.  Group descriptors travel by value
// in the kernel arguments (a captured graph replays them).  Loads are scalar: no alignment is asked of widths or strides.
#include "mfma_tile.h"

namespace {

constexpr int kMaxG = 32;      // groups (experts + gates) per bank layer
constexpr int kMaxW = 1024;    // K_g, N_g
constexpr int kMaxSel = 32;    // experts per gate
constexpr int kMaxOut = 8;     // mixed outputs per bank
constexpr int kTM = 128, kTN = 32, kTK = 32, kLdT = kTK + 1;  // GEMM tile: four wavefronts stacked over the rows
constexpr int kGemmRowBlocks = 256;                           // grid cap over row tiles (further trips beyond)
constexpr int kBR = 16;        // rows of a backward slab = rows of a mixture workgroup
constexpr int kRowBlocks = 2048;  // grid cap over 16-row chunks

struct Grp {
  const float* x;     // forward: this group's input rows; dgrad: unused
  const float* w;     // (N, K) row-major, nn.Linear.weight
  const float* bias;  // (N,) or null
  int64_t ldx;
  int K, N, col0, pad;
};

// forward: a RUN is a maximal range of consecutive groups that read the same rows (x, ldx, K): its wide columns form one GEMM
// whose B operand gathers rows of several W_g, so 32-wide column tiles pack across narrow groups (N_g = 16, gates of 2 or 3).
// dgrad: a run is an input stream; its tiles walk the stream's K output columns.
struct GemmArgs {
  Grp g[kMaxG];
  int run_g0[kMaxG], run_g1[kMaxG], run_tile0[kMaxG + 1];
  float* run_out[kMaxG];   // dgrad: gx of the stream
  int64_t run_ld[kMaxG];   // dgrad: its row stride
  int nruns, M, C, slab_rows;
  float* z;            // forward: (M, C) out; dgrad: gz in
  float* stats;        // forward: (ceil(M / slab_rows), 2, C)
};

__device__ __forceinline__ int find_run(const GemmArgs& a, int tile) {
  int r = 0;
  while (r + 1 < a.nruns && tile >= a.run_tile0[r + 1]) ++r;
  return r;
}

__global__ __launch_bounds__(RH_BLOCK) void experts_fwd_kernel(const GemmArgs a) {
  __shared__ float As[kTM * kLdT];
  __shared__ float Bs[kTK * kLdT];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE, li = lane % 32, kk = lane / 32;
  const int run = find_run(a, blockIdx.y);
  const int g0 = a.run_g0[run], g1 = a.run_g1[run];
  const int c_end = a.g[g1 - 1].col0 + a.g[g1 - 1].N;
  const int c0 = a.g[g0].col0 + kTN * ((int)blockIdx.y - a.run_tile0[run]);
  const float* x = a.g[g0].x;
  const int64_t ldx = a.g[g0].ldx;
  const int K = a.g[g0].K;
  // the four B columns this thread stages (j = tid / 32 + 8 i) and the column this lane owns in the epilogue (li)
  const float* wrow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + tid / 32 + 8 * i;
    wrow[i] = nullptr;
    if (c < c_end) {
      int g = g0;
      while (c >= a.g[g].col0 + a.g[g].N) ++g;
      wrow[i] = a.g[g].w + (int64_t)(c - a.g[g].col0) * K;
    }
  }
  const int cl = c0 + li;
  float bias = 0.f;
  if (cl < c_end) {
    int g = g0;
    while (cl >= a.g[g].col0 + a.g[g].N) ++g;
    if (a.g[g].bias) bias = a.g[g].bias[cl - a.g[g].col0];
  }
  const int R = a.slab_rows;
  const int ntile = (a.M + kTM - 1) / kTM;
  for (int rt = blockIdx.x; rt < ntile; rt += gridDim.x) {
    const int r0 = rt * kTM;
    v16f acc = zero16();
    for (int k0 = 0; k0 < K; k0 += kTK) {
      __syncthreads();
      for (int e = tid; e < kTM * kTK; e += RH_BLOCK) {
        const int r = e / kTK, kc = e % kTK;
        float v = 0.f;
        if (r0 + r < a.M && k0 + kc < K) v = x[(int64_t)(r0 + r) * ldx + k0 + kc];
        As[r * kLdT + kc] = v;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kc = tid % 32, j = tid / 32 + 8 * i;
        Bs[kc * kLdT + j] = (wrow[i] != nullptr && k0 + kc < K) ? wrow[i][k0 + kc] : 0.f;
      }
      __syncthreads();
      acc = mma_lds(acc, As + 32 * w * kLdT, kLdT, 1, Bs, kLdT, 1, kTK, li, kk);
    }
    __syncthreads();  // As is the output tile from here
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = 32 * w + acc_row(r, kk);
      const float v = acc[r] + bias;
      As[rl * kLdT + li] = v;
      if (r0 + rl < a.M && cl < c_end) a.z[(int64_t)(r0 + rl) * a.C + cl] = v;
    }
    __syncthreads();
    // per-slab (sum, M2 about the slab mean) of the tile's columns, rows in ascending order
    if (tid < (kTM / R) * kTN) {
      const int s = tid / kTN, j = tid % kTN;
      const int rb = r0 + s * R;
      const int n = min(R, a.M - rb);
      if (n > 0 && c0 + j < c_end) {
        float sum = 0.f;
        for (int r = 0; r < n; ++r) sum += As[(s * R + r) * kLdT + j];
        const float mean = sum / (float)n;
        float m2 = 0.f;
        for (int r = 0; r < n; ++r) {
          const float d = As[(s * R + r) * kLdT + j] - mean;
          m2 = fmaf(d, d, m2);
        }
        const int64_t slab = rb / R;
        a.stats[(slab * 2 + 0) * a.C + c0 + j] = sum;
        a.stats[(slab * 2 + 1) * a.C + c0 + j] = m2;
      }
    }
  }
}

// gx_s (M, K_s) tile of 128 rows x 32 columns: the reduction runs over the wide columns of every group of the stream
__global__ __launch_bounds__(RH_BLOCK) void experts_dgrad_kernel(const GemmArgs a) {
  __shared__ float As[kTM * kLdT];
  __shared__ float Bs[kTK * kLdT];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE, li = lane % 32, kk = lane / 32;
  const int run = find_run(a, blockIdx.y);
  const int g0 = a.run_g0[run], g1 = a.run_g1[run];
  const int K = a.g[g0].K;
  const int c0 = kTN * ((int)blockIdx.y - a.run_tile0[run]);
  float* out = a.run_out[run];
  const int64_t ldo = a.run_ld[run];
  const int ntile = (a.M + kTM - 1) / kTM;
  for (int rt = blockIdx.x; rt < ntile; rt += gridDim.x) {
    const int r0 = rt * kTM;
    v16f acc = zero16();
    for (int g = g0; g < g1; ++g) {
      const int N = a.g[g].N, col0 = a.g[g].col0;
      const float* W = a.g[g].w;
      for (int n0 = 0; n0 < N; n0 += kTK) {
        __syncthreads();
        for (int e = tid; e < kTM * kTK; e += RH_BLOCK) {
          const int r = e / kTK, kc = e % kTK;
          float v = 0.f;
          if (r0 + r < a.M && n0 + kc < N) v = a.z[(int64_t)(r0 + r) * a.C + col0 + n0 + kc];
          As[r * kLdT + kc] = v;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = tid % 32, kc = tid / 32 + 8 * i;
          Bs[kc * kLdT + j] = (n0 + kc < N && c0 + j < K) ? W[(int64_t)(n0 + kc) * K + c0 + j] : 0.f;
        }
        __syncthreads();
        acc = mma_lds(acc, As + 32 * w * kLdT, kLdT, 1, Bs, kLdT, 1, kTK, li, kk);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = r0 + 32 * w + acc_row(r, kk);
      if (row < a.M && c0 + li < K) out[(int64_t)row * ldo + c0 + li] = acc[r];
    }
  }
}

// ---- BatchNorm of a bank layer ---------------------------------------------------------------------------------------
// stat (5, C): mean, rstd, gamma, beta, kind (1 = expert column: ReLU + dropout follow; 0 = gate column)
struct BnArgs {
  const float* gamma[kMaxG];
  const float* beta[kMaxG];
  float* rmean[kMaxG];
  float* rvar[kMaxG];
  int64_t* batches[kMaxG];
  float momentum[kMaxG], eps[kMaxG];
  int col0[kMaxG + 1];
  int kind[kMaxG];
  int G, M, C, slab_rows, training;
  const float* stats;
  int64_t* rng;
  int64_t* saved_ctr;
  float* stat;
};

__global__ __launch_bounds__(RH_BLOCK) void bn_fwd_kernel(const BnArgs a) {
  const int c = blockIdx.x * RH_BLOCK + threadIdx.x;
  if (c == 0 && a.training) {  // the layer's dropout counter
    a.saved_ctr[0] = a.rng[1];
    a.rng[1] += 1;
  }
  if (c >= a.C) return;
  int g = 0;
  while (c >= a.col0[g + 1]) ++g;
  const int lc = c - a.col0[g];
  float mean, rstd;
  if (a.training) {
    // Chan's combination of the slabs in slab order, about the mean of slab 0 (rh_combine_slabs' arithmetic)
    const int R = a.slab_rows, nslab = (a.M + R - 1) / R;
    const float full = (float)R, tail = (float)(a.M - (nslab - 1) * R);
    const float shift = a.stats[c] / (nslab == 1 ? tail : full);
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < nslab; ++k) {
      const float n = k == nslab - 1 ? tail : full;
      const float d = a.stats[((int64_t)k * 2 + 0) * a.C + c] / n - shift;
      s1 = fmaf(n, d, s1);
      s2 += fmaf(n * d, d, a.stats[((int64_t)k * 2 + 1) * a.C + c]);
    }
    const float dm = s1 / (float)a.M;
    mean = shift + dm;
    const float var = fmaxf((s2 - s1 * dm) / (float)a.M, 0.f);
    rstd = rsqrtf(var + a.eps[g]);
    const float n = (float)a.M;
    const float unbiased = a.M > 1 ? var * (n / (n - 1.f)) : var;
    float* rm = a.rmean[g] + lc;
    float* rv = a.rvar[g] + lc;
    *rm = fmaf(a.momentum[g], mean - *rm, *rm);
    *rv = fmaf(a.momentum[g], unbiased - *rv, *rv);
    if (lc == 0 && a.batches[g] != nullptr) a.batches[g][0] += 1;
  } else {
    mean = a.rmean[g][lc];
    rstd = rsqrtf(a.rvar[g][lc] + a.eps[g]);
  }
  a.stat[c] = mean;
  a.stat[a.C + c] = rstd;
  a.stat[2 * a.C + c] = a.gamma[g][lc];
  a.stat[3 * a.C + c] = a.beta[g][lc];
  a.stat[4 * a.C + c] = (float)a.kind[g];
}

struct ColStat {
  float mean, rstd, gamma, beta;
};
__device__ __forceinline__ ColStat col_stat(const float* stat, int C, int c) {
  return ColStat{stat[c], stat[C + c], stat[2 * C + c], stat[3 * C + c]};
}

__global__ __launch_bounds__(RH_BLOCK) void act_fwd_kernel(const float* z, const float* stat, int M, int C, float p,
                                                           const int64_t* rng, const int64_t* ctr, float* out) {
  const DropKey dk = drop_key(p, rng, ctr, 0);
  const int64_t n = (int64_t)M * C;
  for (int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * RH_BLOCK) {
    const int c = (int)(i % C);
    float y = 0.f;
    if (stat[4 * C + c] != 0.f) {
      const ColStat s = col_stat(stat, C, c);
      const float bn = fmaf((z[i] - s.mean) * s.rstd, s.gamma, s.beta);
      y = bn > 0.f ? bn * drop_mul(p, dk, (uint64_t)i) : 0.f;
    }
    out[i] = y;
  }
}

// ---- gated mixture ---------------------------------------------------------------------------------------------------
struct MixArgs {
  int gate_col[kMaxOut], n_sel[kMaxOut];
  int sel_col[kMaxOut][kMaxSel];
  float* out[kMaxOut];          // forward: out_o (M, H); backward: g_out_o
  int exp_col[kMaxG];           // backward: the expert groups' first columns ...
  signed char pos[kMaxOut][kMaxG];  // ... and each one's place in sel_o, or -1
  int n_out, n_exp, H, M, Cg, Ce;
  const float* zg;      // the buffer that holds the gates' logits (the first layer's) and its stat
  const float* statg;
  const float* ze;      // the experts' last layer and its stat
  const float* state;
  float p;
  const int64_t* rng;
  const int64_t* ctr;
  float* gg;            // backward: gradient buffers of the two layers (the same one for a one-layer bank)
  float* ge;
  float* partg;         // (ceil(M / 16), 2, C) slab sums of the two layers
  float* parte;
};

// softmax(bn(zgate_o)) of rows [r0, r0 + 16) into P[r][e]; every thread of the workgroup calls this
__device__ __forceinline__ void gate_probs(const MixArgs& a, int o, int r0, float* P, int tid) {
  const int E = a.n_sel[o], gc = a.gate_col[o];
  for (int t = tid; t < kBR * E; t += RH_BLOCK) {
    const int r = t / E, e = t % E;
    float l = 0.f;
    if (r0 + r < a.M) {
      const ColStat s = col_stat(a.statg, a.Cg, gc + e);
      l = fmaf((a.zg[(int64_t)(r0 + r) * a.Cg + gc + e] - s.mean) * s.rstd, s.gamma, s.beta);
    }
    P[r * kMaxSel + e] = l;
  }
  __syncthreads();
  if (tid < kBR) {
    float* row = P + tid * kMaxSel;
    float mx = row[0];
    for (int e = 1; e < E; ++e) mx = fmaxf(mx, row[e]);
    float sum = 0.f;
    for (int e = 0; e < E; ++e) {
      row[e] = expf(row[e] - mx);
      sum += row[e];
    }
    const float inv = 1.f / sum;
    for (int e = 0; e < E; ++e) row[e] *= inv;
  }
  __syncthreads();
}

// dropout(relu(bn(z))) of element (row, c) of the experts' last layer
__device__ __forceinline__ float expert_act(const MixArgs& a, const DropKey& dk, int row, int c) {
  const ColStat s = col_stat(a.state, a.Ce, c);
  const int64_t i = (int64_t)row * a.Ce + c;
  const float bn = fmaf((a.ze[i] - s.mean) * s.rstd, s.gamma, s.beta);
  return bn > 0.f ? bn * drop_mul(a.p, dk, (uint64_t)i) : 0.f;
}

__global__ __launch_bounds__(RH_BLOCK) void mix_fwd_kernel(const MixArgs a) {
  __shared__ float P[kBR * kMaxSel];
  const int tid = threadIdx.x, o = blockIdx.y;
  const DropKey dk = drop_key(a.p, a.rng, a.ctr, 0);
  const int E = a.n_sel[o], H = a.H;
  const int nchunk = (a.M + kBR - 1) / kBR;
  for (int ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const int r0 = ch * kBR;
    __syncthreads();
    gate_probs(a, o, r0, P, tid);
    for (int idx = tid; idx < kBR * H; idx += RH_BLOCK) {
      const int r = idx / H, h = idx % H;
      if (r0 + r >= a.M) break;
      float acc = 0.f;
      for (int e = 0; e < E; ++e) acc = fmaf(P[r * kMaxSel + e], expert_act(a, dk, r0 + r, a.sel_col[o][e] + h), acc);
      a.out[o][(int64_t)(r0 + r) * H + h] = acc;
    }
  }
}

__global__ __launch_bounds__(RH_BLOCK) void mix_bwd_kernel(const MixArgs a) {
  __shared__ float P[kMaxOut][kBR * kMaxSel];   // gate weights
  __shared__ float D[kMaxOut][kBR * kMaxSel];   // d_e = g_out . act_e, then the gates' gradient
  const int tid = threadIdx.x, H = a.H;
  const DropKey dk = drop_key(a.p, a.rng, a.ctr, 0);
  const int nchunk = (a.M + kBR - 1) / kBR;
  for (int ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const int r0 = ch * kBR;
    __syncthreads();
    for (int o = 0; o < a.n_out; ++o) gate_probs(a, o, r0, P[o], tid);
    // d[o][r][e] = sum_h g_out_o[r][h] act_sel_o[e][r][h]: eight lanes per item, h strided, an xor tree inside the eight
    const int sub = tid % 8;
    for (int o = 0; o < a.n_out; ++o) {
      const int E = a.n_sel[o], items = kBR * E;
      for (int base = 0; base < items; base += RH_BLOCK / 8) {
        const int it = base + tid / 8;
        const int r = it / E, e = it % E;
        float d = 0.f;
        if (it < items && r0 + r < a.M) {
          const float* go = a.out[o] + (int64_t)(r0 + r) * H;
          for (int h = sub; h < H; h += 8) d = fmaf(go[h], expert_act(a, dk, r0 + r, a.sel_col[o][e] + h), d);
        }
        d += __shfl_xor(d, 4, RH_WAVE);
        d += __shfl_xor(d, 2, RH_WAVE);
        d += __shfl_xor(d, 1, RH_WAVE);
        if (it < items && sub == 0) D[o][r * kMaxSel + e] = d;
      }
    }
    __syncthreads();
    // softmax backward of every gate row: dlogit_e = p_e (d_e - sum_e' p_e' d_e'); one thread per (output, row)
    for (int t = tid; t < a.n_out * kBR; t += RH_BLOCK) {
      const int o = t / kBR, r = t % kBR, E = a.n_sel[o];
      float* d = D[o] + r * kMaxSel;
      const float* p = P[o] + r * kMaxSel;
      float dot = 0.f;
      for (int e = 0; e < E; ++e) dot = fmaf(p[e], d[e], dot);
      for (int e = 0; e < E; ++e) {
        const float g1 = r0 + r < a.M ? p[e] * (d[e] - dot) : 0.f;
        d[e] = g1;
        if (r0 + r < a.M) a.gg[(int64_t)(r0 + r) * a.Cg + a.gate_col[o] + e] = g1;
      }
    }
    __syncthreads();
    // slab sums of the gate columns, rows in ascending order
    for (int t = tid; t < a.n_out * kMaxSel; t += RH_BLOCK) {
      const int o = t / kMaxSel, e = t % kMaxSel;
      if (e >= a.n_sel[o]) continue;
      const int c = a.gate_col[o] + e;
      const ColStat s = col_stat(a.statg, a.Cg, c);
      float s1 = 0.f, s2 = 0.f;
      for (int r = 0; r < kBR && r0 + r < a.M; ++r) {
        const float g1 = D[o][r * kMaxSel + e];
        s1 += g1;
        s2 = fmaf(g1, (a.zg[(int64_t)(r0 + r) * a.Cg + c] - s.mean) * s.rstd, s2);
      }
      a.partg[((int64_t)ch * 2 + 0) * a.Cg + c] = s1;
      a.partg[((int64_t)ch * 2 + 1) * a.Cg + c] = s2;
    }
    // expert columns: a thread owns a column for the slab's rows, so its two sums stay in registers
    for (int idx = tid; idx < a.n_exp * H; idx += RH_BLOCK) {
      const int j = idx / H, h = idx % H, c = a.exp_col[j] + h;
      const ColStat s = col_stat(a.state, a.Ce, c);
      float s1 = 0.f, s2 = 0.f;
      for (int r = 0; r < kBR && r0 + r < a.M; ++r) {
        const int64_t i = (int64_t)(r0 + r) * a.Ce + c;
        const float xhat = (a.ze[i] - s.mean) * s.rstd;
        const float bn = fmaf(xhat, s.gamma, s.beta);
        float gs = 0.f;
        for (int o = 0; o < a.n_out; ++o) {
          const int e = a.pos[o][j];
          if (e >= 0) gs = fmaf(P[o][r * kMaxSel + e], a.out[o][(int64_t)(r0 + r) * H + h], gs);
        }
        const float g1 = bn > 0.f ? gs * drop_mul(a.p, dk, (uint64_t)i) : 0.f;
        a.ge[i] = g1;
        s1 += g1;
        s2 = fmaf(g1, xhat, s2);
      }
      a.parte[((int64_t)ch * 2 + 0) * a.Ce + c] = s1;
      a.parte[((int64_t)ch * 2 + 1) * a.Ce + c] = s2;
    }
  }
}

// hidden layer: g (the grouped dgrad's output, the gradient of a = dropout(relu(bn(z)))) -> the gradient of bn(z), in place,
// and its slab sums.  Gate columns (kind 0) were finished by mix_bwd_kernel and are left alone.
__global__ __launch_bounds__(RH_BLOCK) void act_bwd_kernel(const float* z, const float* stat, int M, int C, float p,
                                                           const int64_t* rng, const int64_t* ctr, float* g, float* part) {
  const DropKey dk = drop_key(p, rng, ctr, 0);
  const int nchunk = (M + kBR - 1) / kBR;
  for (int ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const int r0 = ch * kBR;
    for (int c = threadIdx.x; c < C; c += RH_BLOCK) {
      if (stat[4 * C + c] == 0.f) continue;
      const ColStat s = col_stat(stat, C, c);
      float s1 = 0.f, s2 = 0.f;
      for (int r = 0; r < kBR && r0 + r < M; ++r) {
        const int64_t i = (int64_t)(r0 + r) * C + c;
        const float xhat = (z[i] - s.mean) * s.rstd;
        const float bn = fmaf(xhat, s.gamma, s.beta);
        const float g1 = bn > 0.f ? g[i] * drop_mul(p, dk, (uint64_t)i) : 0.f;
        g[i] = g1;
        s1 += g1;
        s2 = fmaf(g1, xhat, s2);
      }
      part[((int64_t)ch * 2 + 0) * C + c] = s1;
      part[((int64_t)ch * 2 + 1) * C + c] = s2;
    }
  }
}

// dgb (2, C) = (dgamma, dbeta): the slab sums added in slab order
__global__ __launch_bounds__(RH_BLOCK) void bn_bwd_fin_kernel(const float* part, int nchunk, int C, float* dgb) {
  const int c = blockIdx.x * RH_BLOCK + threadIdx.x;
  if (c >= C) return;
  float s1 = 0.f, s2 = 0.f;
  for (int k = 0; k < nchunk; ++k) {
    s1 += part[((int64_t)k * 2 + 0) * C + c];
    s2 += part[((int64_t)k * 2 + 1) * C + c];
  }
  dgb[c] = s2;
  dgb[C + c] = s1;
}

__global__ __launch_bounds__(RH_BLOCK) void bn_bwd_apply_kernel(const float* z, const float* stat, const float* dgb, int M,
                                                                int C, float* g) {
  const int64_t n = (int64_t)M * C;
  const float inv_n = 1.f / (float)M;
  for (int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * RH_BLOCK) {
    const int c = (int)(i % C);
    const ColStat s = col_stat(stat, C, c);
    const float xhat = (z[i] - s.mean) * s.rstd;
    g[i] = s.gamma * s.rstd * (g[i] - dgb[C + c] * inv_n - xhat * (dgb[c] * inv_n));
  }
}

int elementwise_grid(int64_t n) {
  const int64_t b = (n + RH_BLOCK - 1) / RH_BLOCK;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
int chunk_grid(int M) {
  const int b = (M + kBR - 1) / kBR;
  return b < 1 ? 1 : (b > kRowBlocks ? kRowBlocks : b);
}
int gemm_row_grid(int M) {
  const int b = (M + kTM - 1) / kTM;
  return b < 1 ? 1 : (b > kGemmRowBlocks ? kGemmRowBlocks : b);
}

bool widths_ok(int G, const int* K, const int* N) {
  if (G < 1 || G > kMaxG || !K || !N) return false;
  for (int g = 0; g < G; ++g)
    if (K[g] < 1 || K[g] > kMaxW || N[g] < 1 || N[g] > kMaxW) return false;
  return true;
}

// col0 of every group (prefix sums of N) and the total width
int fill_cols(int G, const int* N, int* col0) {
  int c = 0;
  for (int g = 0; g < G; ++g) {
    col0[g] = c;
    c += N[g];
  }
  col0[G] = c;
  return c;
}

}  // namespace

extern "C" int rh_experts_limits(int* max_groups, int* max_width, int* max_sel, int* max_out) {
  RH_REQUIRE(max_groups && max_width && max_sel && max_out, RH_E_BADARG, "rh_experts_limits: null pointer");
  *max_groups = kMaxG, *max_width = kMaxW, *max_sel = kMaxSel, *max_out = kMaxOut;
  return 0;
}

extern "C" int rh_experts_supported(int G, const int* K, const int* N, int n_out, int max_sel, int H, int* ok) {
  RH_REQUIRE(ok != nullptr, RH_E_BADARG, "rh_experts_supported: null pointer");
  *ok = widths_ok(G, K, N) && n_out >= 0 && n_out <= kMaxOut && max_sel >= 0 && max_sel <= kMaxSel && H >= 0 && H <= kMaxW;
  return 0;
}

extern "C" int rh_experts_blocks(int M, int* gemm_row_blocks, int* gemm_rows, int* chunk_blocks, int* chunk_rows) {
  RH_REQUIRE(gemm_row_blocks && gemm_rows && chunk_blocks && chunk_rows, RH_E_BADARG, "rh_experts_blocks: null pointer");
  *gemm_row_blocks = gemm_row_grid(M), *gemm_rows = kTM, *chunk_blocks = chunk_grid(M), *chunk_rows = kBR;
  return 0;
}

extern "C" int rh_experts_fwd(int G, const float* const* x, const int64_t* ldx, const float* const* w,
                              const float* const* bias, const int* K, const int* N, int M, float* z, float* stats,
                              void* stream) {
  RH_REQUIRE(x && ldx && w && bias && z, RH_E_BADARG, "rh_experts_fwd: null pointer");
  RH_REQUIRE(widths_ok(G, K, N), RH_E_UNSUPPORTED, "rh_experts_fwd: G=%d or a width outside 1..%d", G, kMaxW);
  RH_REQUIRE(M >= 0, RH_E_BADARG, "rh_experts_fwd: M=%d", M);
  if (M == 0) return 0;
  GemmArgs a{};
  int col0[kMaxG + 1];
  a.C = fill_cols(G, N, col0);
  a.M = M;
  a.slab_rows = rh_gemm_chain_stats_rows(M);
  a.z = z;
  a.stats = stats;
  RH_REQUIRE(stats != nullptr, RH_E_BADARG, "rh_experts_fwd: null pointer");
  int tiles = 0;
  for (int g = 0; g < G; ++g) {
    RH_REQUIRE(x[g] && w[g] && ldx[g] >= K[g], RH_E_BADARG, "rh_experts_fwd: group %d: null pointer or ldx < K", g);
    a.g[g] = Grp{x[g], w[g], bias[g], ldx[g], K[g], N[g], col0[g], 0};
    if (g == 0 || x[g] != x[g - 1] || ldx[g] != ldx[g - 1] || K[g] != K[g - 1]) {
      if (a.nruns > 0) {
        a.run_g1[a.nruns - 1] = g;
        tiles += (col0[g] - col0[a.run_g0[a.nruns - 1]] + kTN - 1) / kTN;
      }
      a.run_g0[a.nruns] = g;
      a.run_tile0[a.nruns] = tiles;
      ++a.nruns;
    }
  }
  a.run_g1[a.nruns - 1] = G;
  tiles += (col0[G] - col0[a.run_g0[a.nruns - 1]] + kTN - 1) / kTN;
  a.run_tile0[a.nruns] = tiles;
  hipLaunchKernelGGL(experts_fwd_kernel, dim3(gemm_row_grid(M), tiles), dim3(RH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_experts_fwd");
  return 0;
}

extern "C" int rh_experts_dgrad(int S, float* const* gx, const int64_t* ldgx, const int* g_begin, const int* g_end, int G,
                                const float* const* w, const int* K, const int* N, const float* gz, int M, void* stream) {
  RH_REQUIRE(gx && ldgx && g_begin && g_end && w && gz, RH_E_BADARG, "rh_experts_dgrad: null pointer");
  RH_REQUIRE(widths_ok(G, K, N) && S >= 1 && S <= G, RH_E_UNSUPPORTED, "rh_experts_dgrad: G=%d S=%d or a width outside 1..%d",
             G, S, kMaxW);
  RH_REQUIRE(M >= 0, RH_E_BADARG, "rh_experts_dgrad: M=%d", M);
  if (M == 0) return 0;
  GemmArgs a{};
  int col0[kMaxG + 1];
  a.C = fill_cols(G, N, col0);
  a.M = M;
  a.z = const_cast<float*>(gz);
  for (int g = 0; g < G; ++g) {
    RH_REQUIRE(w[g] != nullptr, RH_E_BADARG, "rh_experts_dgrad: group %d: null pointer", g);
    a.g[g] = Grp{nullptr, w[g], nullptr, 0, K[g], N[g], col0[g], 0};
  }
  int tiles = 0;
  for (int s = 0; s < S; ++s) {
    RH_REQUIRE(gx[s] && 0 <= g_begin[s] && g_begin[s] < g_end[s] && g_end[s] <= G, RH_E_BADARG,
               "rh_experts_dgrad: stream %d: null pointer or an empty group range", s);
    const int Ks = K[g_begin[s]];
    for (int g = g_begin[s]; g < g_end[s]; ++g)
      RH_REQUIRE(K[g] == Ks, RH_E_BADARG, "rh_experts_dgrad: stream %d: group %d has K=%d, not %d", s, g, K[g], Ks);
    RH_REQUIRE(ldgx[s] >= Ks, RH_E_BADARG, "rh_experts_dgrad: stream %d: ldgx < K", s);
    a.run_g0[s] = g_begin[s], a.run_g1[s] = g_end[s];
    a.run_out[s] = gx[s], a.run_ld[s] = ldgx[s];
    a.run_tile0[s] = tiles;
    tiles += (Ks + kTN - 1) / kTN;
  }
  a.nruns = S;
  a.run_tile0[S] = tiles;
  hipLaunchKernelGGL(experts_dgrad_kernel, dim3(gemm_row_grid(M), tiles), dim3(RH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_experts_dgrad");
  return 0;
}

extern "C" int rh_experts_bn_fwd(int G, const int* N, const int* kind, const float* const* gamma, const float* const* beta,
                                 float* const* running_mean, float* const* running_var, int64_t* const* batches,
                                 const float* momentum, const float* eps, int M, const float* stats, int training,
                                 int64_t* rng, int64_t* saved_ctr, float* stat, void* stream) {
  RH_REQUIRE(N && kind && gamma && beta && running_mean && running_var && batches && momentum && eps && stat, RH_E_BADARG,
             "rh_experts_bn_fwd: null pointer");
  RH_REQUIRE(G >= 1 && G <= kMaxG, RH_E_UNSUPPORTED, "rh_experts_bn_fwd: G=%d", G);
  RH_REQUIRE(!training || (stats && rng && saved_ctr && M >= 2), RH_E_BADARG,
             "rh_experts_bn_fwd: training needs the slab statistics, the dropout state and M >= 2");
  BnArgs a{};
  for (int g = 0; g < G; ++g) {
    RH_REQUIRE(N[g] >= 1 && gamma[g] && beta[g] && running_mean[g] && running_var[g], RH_E_BADARG,
               "rh_experts_bn_fwd: group %d: null pointer", g);
    a.gamma[g] = gamma[g], a.beta[g] = beta[g], a.rmean[g] = running_mean[g], a.rvar[g] = running_var[g];
    a.batches[g] = batches[g], a.momentum[g] = momentum[g], a.eps[g] = eps[g], a.kind[g] = kind[g];
  }
  a.C = fill_cols(G, N, a.col0);
  a.G = G, a.M = M, a.slab_rows = rh_gemm_chain_stats_rows(M), a.training = training;
  a.stats = stats, a.rng = rng, a.saved_ctr = saved_ctr, a.stat = stat;
  hipLaunchKernelGGL(bn_fwd_kernel, dim3((a.C + RH_BLOCK - 1) / RH_BLOCK), dim3(RH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_experts_bn_fwd");
  return 0;
}

extern "C" int rh_experts_act_fwd(const float* z, const float* stat, int M, int C, float p_drop, const int64_t* rng,
                                  const int64_t* ctr, float* a, void* stream) {
  RH_REQUIRE(z && stat && a && (p_drop <= 0.f || (rng && ctr)), RH_E_BADARG, "rh_experts_act_fwd: null pointer");
  RH_REQUIRE(M >= 0 && C >= 1 && p_drop >= 0.f && p_drop < 1.f, RH_E_BADARG, "rh_experts_act_fwd: M=%d C=%d p=%g", M, C, p_drop);
  if (M == 0) return 0;
  hipLaunchKernelGGL(act_fwd_kernel, dim3(elementwise_grid((int64_t)M * C)), dim3(RH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), z, stat, M, C, p_drop, rng, ctr, a);
  RH_LAUNCH_CHECK("rh_experts_act_fwd");
  return 0;
}

static int mix_fill(MixArgs& a, const char* who, int n_out, const int* gate_col, const int* n_sel, const int* sel_col, int H,
                    float* const* out, const float* zg, const float* statg, int Cg, const float* ze, const float* state,
                    int Ce, int M, float p_drop, const int64_t* rng, const int64_t* ctr) {
  RH_REQUIRE(gate_col && n_sel && sel_col && out && zg && statg && ze && state && (p_drop <= 0.f || (rng && ctr)), RH_E_BADARG,
             "%s: null pointer", who);
  RH_REQUIRE(n_out >= 1 && n_out <= kMaxOut && H >= 1 && H <= kMaxW, RH_E_UNSUPPORTED, "%s: n_out=%d H=%d", who, n_out, H);
  RH_REQUIRE(M >= 0 && p_drop >= 0.f && p_drop < 1.f, RH_E_BADARG, "%s: M=%d p=%g", who, M, p_drop);
  for (int o = 0; o < n_out; ++o) {
    RH_REQUIRE(n_sel[o] >= 1 && n_sel[o] <= kMaxSel, RH_E_UNSUPPORTED, "%s: output %d mixes %d experts (1..%d)", who, o,
               n_sel[o], kMaxSel);
    RH_REQUIRE(out[o] && gate_col[o] >= 0 && gate_col[o] + n_sel[o] <= Cg, RH_E_BADARG, "%s: output %d: bad gate block", who, o);
    a.gate_col[o] = gate_col[o], a.n_sel[o] = n_sel[o], a.out[o] = out[o];
    for (int e = 0; e < n_sel[o]; ++e) {
      const int c = sel_col[o * kMaxSel + e];
      RH_REQUIRE(c >= 0 && c + H <= Ce, RH_E_BADARG, "%s: output %d: expert block %d outside the buffer", who, o, e);
      a.sel_col[o][e] = c;
    }
  }
  a.n_out = n_out, a.H = H, a.M = M, a.Cg = Cg, a.Ce = Ce;
  a.zg = zg, a.statg = statg, a.ze = ze, a.state = state, a.p = p_drop, a.rng = rng, a.ctr = ctr;
  return 0;
}

extern "C" int rh_experts_mix_fwd(int n_out, const int* gate_col, const int* n_sel, const int* sel_col, int H,
                                  const float* zg, const float* statg, int Cg, const float* ze, const float* state, int Ce,
                                  int M, float p_drop, const int64_t* rng, const int64_t* ctr, float* const* out,
                                  void* stream) {
  MixArgs a{};
  const int rc = mix_fill(a, "rh_experts_mix_fwd", n_out, gate_col, n_sel, sel_col, H, out, zg, statg, Cg, ze, state, Ce, M,
                          p_drop, rng, ctr);
  if (rc != 0 || M == 0) return rc;
  hipLaunchKernelGGL(mix_fwd_kernel, dim3(chunk_grid(M), n_out), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_experts_mix_fwd");
  return 0;
}

extern "C" int rh_experts_mix_bwd(int n_out, const int* gate_col, const int* n_sel, const int* sel_col, int H, int n_exp,
                                  const int* exp_col, const float* zg, const float* statg, int Cg, const float* ze,
                                  const float* state, int Ce, int M, float p_drop, const int64_t* rng, const int64_t* ctr,
                                  float* const* g_out, float* gg, float* partg, float* ge, float* parte, void* stream) {
  MixArgs a{};
  const int rc = mix_fill(a, "rh_experts_mix_bwd", n_out, gate_col, n_sel, sel_col, H, g_out, zg, statg, Cg, ze, state, Ce,
                          M, p_drop, rng, ctr);
  if (rc != 0) return rc;
  RH_REQUIRE(exp_col && gg && partg && ge && parte, RH_E_BADARG, "rh_experts_mix_bwd: null pointer");
  RH_REQUIRE(n_exp >= 1 && n_exp <= kMaxG, RH_E_UNSUPPORTED, "rh_experts_mix_bwd: n_exp=%d", n_exp);
  for (int j = 0; j < n_exp; ++j) {
    RH_REQUIRE(exp_col[j] >= 0 && exp_col[j] + H <= Ce, RH_E_BADARG, "rh_experts_mix_bwd: expert block %d outside the buffer", j);
    a.exp_col[j] = exp_col[j];
    for (int o = 0; o < n_out; ++o) {
      a.pos[o][j] = -1;
      for (int e = 0; e < n_sel[o]; ++e)
        if (a.sel_col[o][e] == exp_col[j]) a.pos[o][j] = (signed char)e;
    }
  }
  a.n_exp = n_exp, a.gg = gg, a.ge = ge, a.partg = partg, a.parte = parte;
  if (M == 0) return 0;
  hipLaunchKernelGGL(mix_bwd_kernel, dim3(chunk_grid(M)), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_experts_mix_bwd");
  return 0;
}

extern "C" int rh_experts_act_bwd(const float* z, const float* stat, int M, int C, float p_drop, const int64_t* rng,
                                  const int64_t* ctr, float* g, float* partial, void* stream) {
  RH_REQUIRE(z && stat && g && partial && (p_drop <= 0.f || (rng && ctr)), RH_E_BADARG, "rh_experts_act_bwd: null pointer");
  RH_REQUIRE(M >= 0 && C >= 1 && p_drop >= 0.f && p_drop < 1.f, RH_E_BADARG, "rh_experts_act_bwd: M=%d C=%d p=%g", M, C, p_drop);
  if (M == 0) return 0;
  hipLaunchKernelGGL(act_bwd_kernel, dim3(chunk_grid(M)), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), z, stat, M,
                     C, p_drop, rng, ctr, g, partial);
  RH_LAUNCH_CHECK("rh_experts_act_bwd");
  return 0;
}

extern "C" int rh_experts_bn_bwd(const float* z, const float* stat, int M, int C, const float* partial, float* g, float* dgb,
                                 void* stream) {
  RH_REQUIRE(z && stat && partial && g && dgb, RH_E_BADARG, "rh_experts_bn_bwd: null pointer");
  RH_REQUIRE(M >= 1 && C >= 1, RH_E_BADARG, "rh_experts_bn_bwd: M=%d C=%d", M, C);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(bn_bwd_fin_kernel, dim3((C + RH_BLOCK - 1) / RH_BLOCK), dim3(RH_BLOCK), 0, s, partial,
                     (M + kBR - 1) / kBR, C, dgb);
  RH_LAUNCH_CHECK("rh_experts_bn_bwd");
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(elementwise_grid((int64_t)M * C)), dim3(RH_BLOCK), 0, s, z, stat, dgb, M, C, g);
  RH_LAUNCH_CHECK("rh_experts_bn_bwd");
  return 0;
}
