// FiBiNET's bilinear interaction -- out[b, (i, j), :] = (W_ij x_i) * x_j for every field pair i < j, and the same on the
// SENET-gated fields -- as fused kernels for gfx950: nothing of size (B, P, D) but the result itself reaches HBM.
//
// Reference op chain replaced (paths relative to the reference package):
//   BiLinearInteractionLayer.forward   torch_rechub/basic/layers.py:557-565   the per-pair Linear calls and Hadamard
//                                                                              products, run twice by FiBiNet.forward (raw and
//                                                                              gated) and concatenated, and their autograd
//
// A sample is one row of C = F D flat columns, c = j D + d.  For a left field i the pairs (i, i + 1 .. F - 1) are
// contiguous in out, and out[b, off_i D + c - (i + 1) D] = U_i[b, c] x[b, c] for c >= (i + 1) D, where
// U_i = x_i Wcat_i^T is one GEMM with K = D whose B operand row for column c is row d of weight widx(i, j) (the pair, i,
// or 0).  The 32-wide column blocks of v_mfma_f32_32x32x2_f32 are aligned to c, so a lane's column is the same (j, d)
// for every i.  Gating the operands scales a pair by a_i a_j: (W (a_i x_i)) * (a_j x_j) = a_i a_j (W x_i) * x_j, so the
// gated half of out is the raw half times one scalar per (sample, pair) and one product serves both.
//
//   forward  a workgroup owns (a 32-row tile, a group of left fields of about equal pair count); the x tile (and the gate)
//            sit in LDS: 4 (32 (C|1) + 32 (F|1)) bytes, 139520 at the limits, so the tile always fits.  Wavefront w
//            takes the column blocks cb = first + w, + 4, ...; A = x_i from LDS, B = the lane's own weight row, read
//            once into registers; the epilogue multiplies by x_j (and a_i a_j) and stores along c.
//   backward (inputs, gate): a workgroup owns (a 64-row tile, a slice of 128 flat columns) and walks i.  Per i it
//            stages x_i and the slice's weight rows in LDS, recomputes U_i, and with Gc = G_raw + a_i a_j G_gated keeps
//            S1 += G_raw U_i and S2 += a_i G_gated U_i in accumulator registers that stay with the lane's column over
//            the whole loop (right role: g_x[b, c] = S1 + a_j S2, g_gate[b, j] = sum_d x[b, c] S2).  gU = Gc x_j goes
//            through LDS into the left-role product g_x_i += gU Wcat_i (K = the slice's columns), whose result is the
//            slice's partial; G_gated U_i x_j a_j is row-summed through LDS into g_gate[b, i].  A second, elementwise
//            launch adds the slices' partials in slice order.
//   wgrad    g_w[n] = sum_b gU^T x_i with gU formed straight from G, the gate and x_j in the operand load (no U).  A
//            workgroup owns (a 32 x 32 block of one stacked weight, a row split); its four wavefronts take 16 rows each
//            of every 64-row tile, walk the pairs that share the weight and the split's tiles with the accumulator in
//            registers, and are added in wavefront order into one row of `part` (g_w = rh_colsum of it).
//
// An odd D ends in a step whose upper half-wavefront feeds zeros.  Lanes whose column lies outside a product read zeros
// or a clamped address and store nothing.  No atomics anywhere: every sum has a fixed order.
#include "mfma_tile.h"

namespace {

constexpr int kMaxF = RH_CIN_MAX_F;        // fields of a (B, F, D) block
constexpr int kMaxD = RH_SA_MAX_D;         // width of one field: K of the product
constexpr int kMaxC = RH_TWOTOWER_MAX_D;   // width of a sample's flattened row
constexpr int kFwdRows = 32;               // rows of a forward tile
constexpr int kFwdGrid = 1024;             // persistent forward workgroups
constexpr int kFwdTarget = 512;            // forward units wanted before the left fields stop being split
constexpr int kMaxGroups = 8;              // left-field groups per row tile, at most
constexpr int kBwdRows = 64;               // rows of a backward tile
constexpr int kSlice = 128;                // flat columns of a backward workgroup: two column blocks per wavefront
constexpr int kLdS = kSlice + 1;
constexpr int kWgTarget = 1024;            // weight-gradient workgroups wanted
constexpr int kWgMaxSplits = 256;          // rows of `part`, at most
static_assert(kBwdRows == kT && kMaxD <= kT && kMaxF <= kT, "the backward tiles are the 64-row tile of mfma_tile.h");

struct BlArgs {
  const float* x;     // (B, F, D), sample stride xs
  const float* w;     // (NW, D, D)
  const float* gate;  // (B, F) or null
  const float* g;     // backward: the gradient of out, contiguous
  float* out;
  float* gx;          // (B, F, D) contiguous, or null
  float* ggate;       // (B, F) or null
  float* ws;          // backward: (S, B, C) left-role partials, then (S, B, F) gate partials
  float* part;        // wgrad: (splits, NW D D)
  int64_t xs;
  int B, F, D, C, P, NW, kind;
  int ngroups, units, ibeg[kMaxGroups + 1];  // forward
  int S;                                     // backward
  int splits, tps, nt;                       // wgrad: row splits, 64-row tiles per split, tiles
};

__device__ __forceinline__ int pair_off(int i, int F) { return i * (2 * F - i - 1) / 2; }
__device__ __forceinline__ int widx(int kind, int i, int j, int F) {
  return kind == 2 ? pair_off(i, F) + j - i - 1 : kind == 1 ? i : 0;
}

__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 1, RH_WAVE);
  return v + __shfl_xor(v, 2, RH_WAVE);
}

// acc = A (32 x D) B (D x 32): A[li][k] = ap[k] (the lane's row, LDS), B[k][li] = wrow[k] (the lane's weight row, global,
// each element read by exactly one lane)
__device__ __forceinline__ v16f u_block_global(const float* ap, const float* wrow, int D, int kk) {
  float bw[kMaxD / 2];
#pragma unroll
  for (int s = 0; s < kMaxD / 2; ++s) {
    bw[s] = 0.f;
    if (2 * s < D) {  // (wavefront-uniform)
      const int k = 2 * s + kk;
      bw[s] = k < D ? wrow[k] : 0.f;
    }
  }
  v16f acc = zero16();
#pragma unroll
  for (int s = 0; s < kMaxD / 2; ++s) {
    if (2 * s < D) {
      const int k = 2 * s + kk;
      const float av = k < D ? ap[k] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bw[s], acc, 0, 0, 0);
    }
  }
  return acc;
}

// acc += A (32 x K) B (K x 32) from LDS, any K: A[li][k] = ap[k * ak], B[k][li] = bp[k * bk] (the lane's own row and column)
__device__ __forceinline__ v16f mma_any(v16f acc, const float* ap, int ak, const float* bp, int bk, int K, int kk) {
  for (int k = 0; k < (K & ~1); k += 2)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[(k + kk) * ak], bp[(k + kk) * bk], acc, 0, 0, 0);
  if (K & 1) {
    const float av = kk == 0 ? ap[(K - 1) * ak] : 0.f;
    const float bv = kk == 0 ? bp[(K - 1) * bk] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
  }
  return acc;
}

__global__ __launch_bounds__(RH_BLOCK) void bilinear_fwd_kernel(const BlArgs a) {
  extern __shared__ float lds[];
  const int F = a.F, D = a.D, C = a.C, ldx = C | 1, ldg = F | 1;
  float* sX = lds;                  // [32][ldx]
  float* sA = sX + kFwdRows * ldx;  // [32][ldg]: the gate
  const int tid = threadIdx.x, lane = tid % RH_WAVE, wv = tid / RH_WAVE, li = lane % 32, kk = lane / 32;
  const int NB = (C + 31) / 32;
  const bool gated = a.gate != nullptr;
  const int64_t PD = (int64_t)a.P * D, os = gated ? 2 * PD : PD;
  for (int u = blockIdx.x; u < a.units; u += gridDim.x) {
    const int t = u / a.ngroups, grp = u - t * a.ngroups;
    const int64_t row0 = (int64_t)t * kFwdRows;
    const int64_t left = (int64_t)a.B - row0;
    const int nv = left < kFwdRows ? (int)left : kFwdRows;  // rows of the tile that exist
    __syncthreads();  // (the previous unit is done with the LDS)
    for (int e = tid; e < kFwdRows * C; e += RH_BLOCK) {
      const int r = e / C, c = e - r * C;
      sX[r * ldx + c] = r < nv ? a.x[(row0 + r) * a.xs + c] : 0.f;
    }
    if (gated)
      for (int e = tid; e < kFwdRows * F; e += RH_BLOCK) {
        const int r = e / F, f = e - r * F;
        sA[r * ldg + f] = r < nv ? a.gate[(row0 + r) * F + f] : 0.f;
      }
    __syncthreads();
    for (int i = a.ibeg[grp]; i < a.ibeg[grp + 1]; ++i) {
      const int c0 = (i + 1) * D;
      const int64_t obase = (int64_t)pair_off(i, F) * D - c0;
      for (int cb = c0 / 32 + wv; cb < NB; cb += 4) {
        const int c = 32 * cb + li;
        const bool valid = c >= c0 && c < C;
        const int cc = min(max(c, c0), C - 1);  // a lane outside reads a column inside; its result is not stored
        const int j = cc / D, d = cc - j * D;
        const float* wrow = a.w + ((int64_t)widx(a.kind, i, j, F) * D + d) * D;
        const v16f acc = u_block_global(sX + li * ldx + i * D, wrow, D, kk);
        if (valid) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, kk);
            if (row < nv) {
              const float v = acc[r] * sX[row * ldx + c];
              float* o = a.out + (row0 + row) * os + obase + c;
              o[0] = v;
              if (gated) o[PD] = v * (sA[row * ldg + i] * sA[row * ldg + j]);
            }
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(RH_BLOCK) void bilinear_bwd_kernel(const BlArgs a) {
  extern __shared__ float lds[];
  const int F = a.F, D = a.D, C = a.C, ldd = D | 1, ldg = F | 1;
  const bool gated = a.gate != nullptr;
  float* sXi = lds;                   // [64][ldd]: x_i
  float* sW = sXi + kT * ldd;         // [128][ldd]: the weight row of each of the slice's columns, for this i
  float* sGU = sW + kSlice * ldd;     // [64][129]: gU = Gc x_j
  float* sA = sGU + kT * kLdS;        // gated only: [64][ldg] the gate, [64][ldg] the slice's g_gate,
  float* sGG = sA + kT * ldg;         //             [64][129] the per-column gate terms
  float* sGL = sGG + kT * ldg;
  const int tid = threadIdx.x, lane = tid % RH_WAVE, wv = tid / RH_WAVE, li = lane % 32, kk = lane / 32;
  const int wm = wv & 1, wn = wv >> 1;
  const int t = blockIdx.x / a.S, s = blockIdx.x - t * a.S;
  const int64_t row0 = (int64_t)t * kT;
  const int64_t left = (int64_t)a.B - row0;
  const int nv = left < kT ? (int)left : kT;
  const int cbeg = s * kSlice, cend = min(cbeg + kSlice, C);
  const int nlb = (cend - cbeg + 31) / 32;  // column blocks of the slice
  const int64_t PD = (int64_t)a.P * D, gs = gated ? 2 * PD : PD;
  const int r4 = tid >> 2, q4 = tid & 3;  // row sums: four lanes per row

  // the lane's two columns: x_j stays in registers, S1 and S2 are the right-role sums
  float xj[2][16];
  v16f S1[2], S2[2];
  int jc[2];
#pragma unroll
  for (int tb = 0; tb < 2; ++tb) {
    const int c = cbeg + 32 * (wn + 2 * tb) + li;
    jc[tb] = min(c, C - 1) / D;
    S1[tb] = zero16();
    S2[tb] = zero16();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * wm + acc_row(r, kk);
      xj[tb][r] = (c < cend && row < nv) ? a.x[(row0 + row) * a.xs + c] : 0.f;
    }
  }
  if (gated)
    for (int e = tid; e < kT * F; e += RH_BLOCK) {
      const int r = e / F, f = e - r * F;
      sA[r * ldg + f] = r < nv ? a.gate[(row0 + r) * F + f] : 0.f;
      sGG[r * ldg + f] = 0.f;
    }

  for (int i = 0; (i + 1) * D < cend; ++i) {
    const int c0 = (i + 1) * D;
    const int64_t obase = (int64_t)pair_off(i, F) * D - c0;
    const int lb0 = max(c0 - cbeg, 0) / 32;  // first column block with a pair of i
    __syncthreads();  // (the previous i is done with sXi, sW, sGU, sGL)
    for (int e = tid; e < kT * D; e += RH_BLOCK) {
      const int r = e / D, k = e - r * D;
      sXi[r * ldd + k] = r < nv ? a.x[(row0 + r) * a.xs + i * D + k] : 0.f;
    }
    for (int e = tid; e < kSlice * D; e += RH_BLOCK) {
      const int cc = e / D, n = e - cc * D;
      const int c = cbeg + cc;
      float v = 0.f;
      if (c >= c0 && c < cend) {
        const int j = c / D, d = c - j * D;
        v = a.w[((int64_t)widx(a.kind, i, j, F) * D + d) * D + n];
      }
      sW[cc * ldd + n] = v;
    }
    __syncthreads();
#pragma unroll
    for (int tb = 0; tb < 2; ++tb) {
      const int cbl = wn + 2 * tb;
      if (cbl >= lb0 && cbl < nlb) {  // (wavefront-uniform)
        const int cl = 32 * cbl + li, c = cbeg + cl;
        const bool valid = c >= c0 && c < cend;
        const v16f U = mma_any(zero16(), sXi + (32 * wm + li) * ldd, 1, sW + cl * ldd, 1, D, kk);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * wm + acc_row(r, kk);
          const bool live = valid && row < nv;
          const int64_t at = live ? (row0 + row) * gs + obase + c : 0;
          const float Gr = live ? a.g[at] : 0.f;
          float Gg = 0.f, ai = 0.f, aj = 0.f;
          if (gated) {
            Gg = live ? a.g[at + PD] : 0.f;
            ai = sA[row * ldg + i];
            aj = sA[row * ldg + jc[tb]];
          }
          S1[tb][r] = fmaf(Gr, U[r], S1[tb][r]);
          S2[tb][r] = fmaf(ai * Gg, U[r], S2[tb][r]);
          sGU[row * kLdS + cl] = (Gr + ai * aj * Gg) * xj[tb][r];
          if (gated) sGL[row * kLdS + cl] = Gg * U[r] * xj[tb][r] * aj;
        }
      }
    }
    __syncthreads();
    if (a.gx != nullptr && 32 * wn < D) {  // left role: g_x_i (64 x D) = gU (64 x K) Wcat (K x D) over the slice's columns
      const int n = 32 * wn + li;
      const v16f acc = mma_any(zero16(), sGU + (32 * wm + li) * kLdS + 32 * lb0, 1, sW + 32 * lb0 * ldd + min(n, D - 1), ldd,
                               32 * (nlb - lb0), kk);
      if (n < D) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * wm + acc_row(r, kk);
          if (row < nv) a.ws[((int64_t)s * a.B + row0 + row) * C + i * D + n] = acc[r];
        }
      }
    }
    if (gated && a.ggate != nullptr) {  // left role of the gate: a row sum in a fixed order
      float v = 0.f;
      for (int k = 32 * lb0 + q4; k < 32 * nlb; k += 4) v += sGL[r4 * kLdS + k];
      v = quad_sum(v);
      if (q4 == 0) sGG[r4 * ldg + i] = v;
    }
  }

  __syncthreads();  // (the last i is done with sGL; sGG is written)
#pragma unroll
  for (int tb = 0; tb < 2; ++tb) {
    const int cl = 32 * (wn + 2 * tb) + li, c = cbeg + cl;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * wm + acc_row(r, kk);
      const bool live = c < cend && row < nv;
      const float aj = gated ? sA[row * ldg + jc[tb]] : 0.f;
      if (live && a.gx != nullptr) a.gx[(row0 + row) * C + c] = fmaf(aj, S2[tb][r], S1[tb][r]);
      if (gated) sGL[row * kLdS + cl] = live ? xj[tb][r] * S2[tb][r] : 0.f;
    }
  }
  if (gated && a.ggate != nullptr) {
    __syncthreads();
    float* wsg = a.ws + (int64_t)a.S * a.B * C;
    for (int e = tid; e < kT * F; e += RH_BLOCK) {
      const int r = e / F, f = e - r * F;
      float v = sGG[r * ldg + f];
      for (int c = max(f * D, cbeg); c < min(f * D + D, cend); ++c) v += sGL[r * kLdS + c - cbeg];
      if (r < nv) wsg[((int64_t)s * a.B + row0 + r) * F + f] = v;
    }
  }
}

// g_x += the slices' left-role partials, g_gate = the slices' gate partials, in slice order
__global__ __launch_bounds__(RH_BLOCK) void bilinear_combine_kernel(const BlArgs a) {
  const int64_t nx = a.gx != nullptr ? (int64_t)a.B * a.C : 0;
  const int64_t ng = a.ggate != nullptr ? (int64_t)a.B * a.F : 0;
  const float* wsg = a.ws + (int64_t)a.S * a.B * a.C;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < nx + ng; e += (int64_t)gridDim.x * RH_BLOCK) {
    if (e < nx) {
      const int64_t b = e / a.C;
      const int c = (int)(e - b * a.C), i = c / a.D;
      if (i < a.F - 1) {  // slice s holds a pair of i when (i + 1) D < its last column + 1
        float v = a.gx[e];
        for (int s = (i + 1) * a.D / kSlice; s < a.S; ++s) v += a.ws[((int64_t)s * a.B + b) * a.C + c];
        a.gx[e] = v;
      }
    } else {
      const int64_t q = e - nx;
      float v = 0.f;
      for (int s = 0; s < a.S; ++s) v += wsg[(int64_t)s * a.B * a.F + q];
      a.ggate[q] = v;
    }
  }
}

__global__ __launch_bounds__(RH_BLOCK) void bilinear_wgrad_kernel(const BlArgs a) {
  __shared__ float red[4][16][RH_WAVE];
  const int F = a.F, D = a.D;
  const bool gated = a.gate != nullptr;
  const int tid = threadIdx.x, lane = tid % RH_WAVE, wv = tid / RH_WAVE, li = lane % 32, kk = lane / 32;
  const int nblk = (D + 31) / 32;
  const int n = blockIdx.x / (nblk * nblk), rem = blockIdx.x - n * nblk * nblk;
  const int dl = 32 * (rem / nblk) + li;  // the lane's weight row as an A lane
  const int kc = 32 * (rem % nblk) + li;  // the lane's weight column as a B lane
  const int64_t PD = (int64_t)a.P * D, gs = gated ? 2 * PD : PD;
  // the pairs that share weight n: one (kind 2), those of left field n (kind 1), all (kind 0)
  int i_lo = 0, i_hi = F - 1;
  if (a.kind == 1) {
    i_lo = n;
    i_hi = min(n + 1, F - 1);
  } else if (a.kind == 2) {
    while (pair_off(i_lo + 1, F) <= n) ++i_lo;
    i_hi = i_lo + 1;
  }
  const int t_lo = blockIdx.y * a.tps, t_hi = min(t_lo + a.tps, a.nt);
  v16f acc = zero16();
  for (int i = i_lo; i < i_hi; ++i) {
    const int j_lo = a.kind == 2 ? i + 1 + n - pair_off(i, F) : i + 1;
    const int j_hi = a.kind == 2 ? j_lo + 1 : F;
    for (int j = j_lo; j < j_hi; ++j) {
      const int64_t gcol = (int64_t)(pair_off(i, F) + j - i - 1) * D + dl;
      for (int t = t_lo; t < t_hi; ++t) {
        const int64_t base = (int64_t)t * kT + 16 * wv;
        float av[8], bv[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const int64_t b = base + 2 * s + kk;
          const bool okb = b < a.B;
          const bool oka = okb && dl < D;
          float gc = oka ? a.g[b * gs + gcol] : 0.f;
          if (gated && oka) gc = fmaf(a.gate[b * F + i] * a.gate[b * F + j], a.g[b * gs + PD + gcol], gc);
          av[s] = oka ? gc * a.x[b * a.xs + j * D + dl] : 0.f;
          bv[s] = (okb && kc < D) ? a.x[b * a.xs + i * D + kc] : 0.f;
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) red[wv][r][lane] = acc[r];
  __syncthreads();
  if (wv == 0 && kc < D) {
    float* part = a.part + ((int64_t)blockIdx.y * a.NW + n) * D * D;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = 32 * (rem / nblk) + acc_row(r, kk);
      if (d < D) part[d * D + kc] = ((red[0][r][lane] + red[1][r][lane]) + red[2][r][lane]) + red[3][r][lane];
    }
  }
}

int check_shape(const char* who, int B, int F, int D, int kind) {
  RH_REQUIRE(B >= 0, RH_E_BADARG, "%s: bad batch size %d", who, B);
  RH_REQUIRE(kind >= 0 && kind <= 2, RH_E_BADARG, "%s: bad kind %d (0 field_all, 1 field_each, 2 field_interaction)", who, kind);
  RH_REQUIRE(F >= 2 && F <= kMaxF, RH_E_UNSUPPORTED, "%s: num_fields %d unsupported (2 .. %d)", who, F, kMaxF);
  RH_REQUIRE(D >= 1 && D <= kMaxD, RH_E_UNSUPPORTED, "%s: embed_dim %d unsupported (1 .. %d)", who, D, kMaxD);
  RH_REQUIRE(F * D <= kMaxC, RH_E_UNSUPPORTED, "%s: num_fields * embed_dim %d unsupported (<= %d)", who, F * D, kMaxC);
  return 0;
}

size_t fwd_lds(int F, int D) { return sizeof(float) * (size_t)(kFwdRows * ((F * D) | 1) + kFwdRows * (F | 1)); }
size_t bwd_lds(int F, int D, bool gated) {
  size_t n = (size_t)(kT + kSlice) * (D | 1) + (size_t)kT * kLdS;
  if (gated) n += (size_t)2 * kT * (F | 1) + (size_t)kT * kLdS;
  return sizeof(float) * n;
}
constexpr size_t kFwdLdsMax = sizeof(float) * (size_t)(kFwdRows * (kMaxC | 1) + kFwdRows * (kMaxF | 1));
// above every backward shape (the largest, D = 64 with F = 16 and a gate, needs 124672)
constexpr size_t kBwdLdsMax = sizeof(float) * (size_t)((kT + kSlice) * (kMaxD | 1) + 2 * kT * kLdS + 2 * kT * (kMaxF | 1));

BlArgs make_args(const float* x, int64_t xs, const float* w, const float* gate, int B, int F, int D, int kind) {
  BlArgs a{};
  a.x = x;
  a.xs = xs;
  a.w = w;
  a.gate = gate;
  a.B = B;
  a.F = F;
  a.D = D;
  a.C = F * D;
  a.P = F * (F - 1) / 2;
  a.NW = kind == 2 ? a.P : kind == 1 ? F : 1;
  a.kind = kind;
  // forward: split the left fields of a row tile into groups of about equal pair count while the tiles alone are few
  const int64_t ft = ((int64_t)B + kFwdRows - 1) / kFwdRows;
  int64_t want = ft > 0 ? (kFwdTarget + ft - 1) / ft : 1;
  const int cap = F - 1 < kMaxGroups ? F - 1 : kMaxGroups;
  a.ngroups = (int)(want < 1 ? 1 : want > cap ? cap : want);
  a.units = (int)(ft * a.ngroups);
  for (int g = 0, i = 0; g <= a.ngroups; ++g) {
    while (i < F - 1 && (int64_t)(i * (2 * F - i - 1) / 2) * a.ngroups < (int64_t)g * a.P) ++i;
    a.ibeg[g] = g == a.ngroups ? F - 1 : i;
  }
  a.S = (a.C + kSlice - 1) / kSlice;
  // wgrad: row splits so that about kWgTarget workgroups exist, each with at least one tile
  const int nblk = (D + 31) / 32;
  const int wunits = a.NW * nblk * nblk;
  a.nt = (int)(((int64_t)B + kT - 1) / kT);
  int ws = (kWgTarget + wunits - 1) / wunits;
  ws = ws > kWgMaxSplits ? kWgMaxSplits : ws;
  ws = ws > a.nt ? a.nt : ws;
  a.tps = ws > 0 ? (a.nt + ws - 1) / ws : 0;
  a.splits = a.tps > 0 ? (a.nt + a.tps - 1) / a.tps : 0;
  return a;
}

}  // namespace

extern "C" int rh_bilinear_plan(int B, int F, int D, int kind, int* fwd_units, int* fwd_grid, int* bwd_slices,
                                int* wgrad_splits, int* wgrad_tiles, int64_t* bwd_floats, int64_t* wgrad_floats) {
  RH_REQUIRE(fwd_units && fwd_grid && bwd_slices && wgrad_splits && wgrad_tiles && bwd_floats && wgrad_floats, RH_E_BADARG,
             "rh_bilinear_plan: null pointer");
  if (int rc = check_shape("rh_bilinear_plan", B, F, D, kind)) return rc;
  const BlArgs a = make_args(nullptr, 0, nullptr, nullptr, B, F, D, kind);
  *fwd_units = a.units;
  *fwd_grid = a.units < kFwdGrid ? a.units : kFwdGrid;
  *bwd_slices = a.S;
  *wgrad_splits = a.splits;
  *wgrad_tiles = a.tps;
  *bwd_floats = (int64_t)a.S * B * (a.C + F);
  *wgrad_floats = (int64_t)a.splits * a.NW * D * D;
  return 0;
}

extern "C" int rh_bilinear_fwd(const float* x, int64_t x_stride, const float* w, const float* gate, int B, int F, int D,
                               int kind, float* out, void* stream) {
  RH_REQUIRE(x && w && out, RH_E_BADARG, "rh_bilinear_fwd: null argument");
  if (int rc = check_shape("rh_bilinear_fwd", B, F, D, kind)) return rc;
  RH_REQUIRE(x_stride >= (int64_t)F * D, RH_E_BADARG, "rh_bilinear_fwd: sample stride %lld below F D", (long long)x_stride);
  if (B == 0) return 0;
  static RhLdsReserved reserved;
  if (int rc = rh_reserve_lds(reserved, bilinear_fwd_kernel, kFwdLdsMax, "rh_bilinear_fwd")) return rc;
  BlArgs a = make_args(x, x_stride, w, gate, B, F, D, kind);
  a.out = out;
  const unsigned grid = (unsigned)(a.units < kFwdGrid ? a.units : kFwdGrid);
  hipLaunchKernelGGL(bilinear_fwd_kernel, dim3(grid), dim3(RH_BLOCK), fwd_lds(F, D), reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_bilinear_fwd");
  return 0;
}

extern "C" int rh_bilinear_bwd(const float* x, int64_t x_stride, const float* w, const float* gate, const float* g_out, int B,
                               int F, int D, int kind, float* g_x, float* g_gate, float* workspace, void* stream) {
  RH_REQUIRE(x && w && g_out && workspace && (g_x || g_gate), RH_E_BADARG, "rh_bilinear_bwd: null argument");
  RH_REQUIRE(g_gate == nullptr || gate != nullptr, RH_E_BADARG, "rh_bilinear_bwd: g_gate without a gate");
  if (int rc = check_shape("rh_bilinear_bwd", B, F, D, kind)) return rc;
  RH_REQUIRE(x_stride >= (int64_t)F * D, RH_E_BADARG, "rh_bilinear_bwd: sample stride %lld below F D", (long long)x_stride);
  if (B == 0) return 0;
  static RhLdsReserved reserved;
  if (int rc = rh_reserve_lds(reserved, bilinear_bwd_kernel, kBwdLdsMax, "rh_bilinear_bwd")) return rc;
  BlArgs a = make_args(x, x_stride, w, gate, B, F, D, kind);
  a.g = g_out;
  a.gx = g_x;
  a.ggate = g_gate;
  a.ws = workspace;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(bilinear_bwd_kernel, dim3((unsigned)a.nt * a.S), dim3(RH_BLOCK), bwd_lds(F, D, gate != nullptr), st, a);
  RH_LAUNCH_CHECK("rh_bilinear_bwd");
  const int64_t n = (int64_t)B * (a.C + F);
  const int64_t blocks = (n + RH_BLOCK - 1) / RH_BLOCK;
  hipLaunchKernelGGL(bilinear_combine_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(RH_BLOCK), 0, st, a);
  RH_LAUNCH_CHECK("rh_bilinear_bwd");
  return 0;
}

extern "C" int rh_bilinear_wgrad(const float* x, int64_t x_stride, const float* gate, const float* g_out, int B, int F, int D,
                                 int kind, float* part, void* stream) {
  RH_REQUIRE(x && g_out && part, RH_E_BADARG, "rh_bilinear_wgrad: null argument");
  if (int rc = check_shape("rh_bilinear_wgrad", B, F, D, kind)) return rc;
  RH_REQUIRE(x_stride >= (int64_t)F * D, RH_E_BADARG, "rh_bilinear_wgrad: sample stride %lld below F D", (long long)x_stride);
  if (B == 0) return 0;
  BlArgs a = make_args(x, x_stride, nullptr, gate, B, F, D, kind);
  a.g = g_out;
  a.part = part;
  const int nblk = (D + 31) / 32;
  hipLaunchKernelGGL(bilinear_wgrad_kernel, dim3((unsigned)(a.NW * nblk * nblk), (unsigned)a.splits), dim3(RH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_bilinear_wgrad");
  return 0;
}
