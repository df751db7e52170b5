// Field-aware FM (DeepFFM / FAT-DeepFFM) interaction and the CEN field attention, for gfx950.
//
// Reference op chains replaced (paths relative to the reference package):
//   DeepFFM.forward      torch_rechub/models/ranking/deepffm.py:57-62   x * F + fields_offset -> (B, F, F, D) lookup -> FFM
//   FFM.forward          torch_rechub/basic/layers.py:736-746           F(F-1)/2 slice products + torch.stack (+ sum)
//   CEN.forward          torch_rechub/basic/layers.py:777-786           d = relu(sum_d u * em), aem = s * em
//
// Names: F fields, P = F(F-1)/2 pairs in the reference's order (i outer, j > i inner), D logical width, Dp physical row
// width (PaddedEmbedding stores D = 10 as 16 floats).  Pair side (i, j) reads row x_i * F + j of field i's table, so
// em[b, p(i,j), :D] = T_i[x_i F + j] * T_j[x_j F + i]: 2P of the F^2 rows of a sample are read (never the diagonal) and
// nothing of size (B, F, F, D) is materialised.  The dense mode reads the same rows from a (B, F, F, D) tensor
// (the layer-level FFM a patched reference model calls).
//
// Roofline: HBM.  Forward: 2 P D reads (whole 64-byte rows at D = 10 / Dp = 16) and P D writes per sample.  Backward:
// 2 P D float atomics per sample into the tables' gradient buffers (memory-side, ~1.3 TB/s chip-wide) or, in sink mode,
// 2 P Dp plain stores of gradient rows for the data-parallel exchange.  One workgroup walks one sample at a time:
// consecutive lanes own consecutive (pair, column) elements, so a wavefront reads ~6 pairs' rows as contiguous runs.
#include "common.h"

namespace {

constexpr int kMaxF = RH_FFM_MAX_F;
constexpr int kMaxP = kMaxF * (kMaxF - 1) / 2;
constexpr int kMaxD = RH_FFM_MAX_D;
constexpr int kCenRows = 64;  // samples per partial row of the CEN u gradient

struct FfmArgs {
  const int64_t* fdesc;  // table mode (fdesc / idesc layouts of include/rechub_hip.h), else null
  const int64_t* idesc;
  const float* x;        // dense mode: (B, F, F, D), sample stride xs
  int64_t xs;
  int B, F, D, Dp, reduce;
  float* out;            // forward: em (B, P*D) or (B, P) when reduce, row stride ld_out
  int64_t ld_out;
  const float* g;        // backward: g_em, row stride ld_g
  int64_t ld_g;
  float* gx;             // backward, dense mode: dX (B, F, F, D), sample stride ld_gx
  int64_t ld_gx;
  int sink;              // backward, table mode: 1 = rows (B, F(F-1), Dp) instead of the gradient buffers
  float* rows;
  int* err;
};

// Per-workgroup staging: the pair table once, the F row bases of the current sample per sample.
struct FfmShared {
  uint8_t pi[kMaxP], pj[kMaxP];
  const float* tab[kMaxF];
  float* grad[kMaxF];
  int64_t voc[kMaxF], pad[kMaxF], base[kMaxF];
};

template <bool TABLE>
__device__ __forceinline__ void stage_pairs(const FfmArgs& a, FfmShared& s) {
  const int F = a.F;
  for (int i = threadIdx.x; i < F - 1; i += RH_BLOCK) {
    int p = i * (2 * F - i - 1) / 2;  // first pair of row i
    for (int j = i + 1; j < F; ++j, ++p) {
      s.pi[p] = (uint8_t)i;
      s.pj[p] = (uint8_t)j;
    }
  }
  if (TABLE) {
    for (int f = threadIdx.x; f < F; f += RH_BLOCK) {
      s.tab[f] = reinterpret_cast<const float*>(a.fdesc[f]);
      s.grad[f] = reinterpret_cast<float*>(a.fdesc[F + f]);
      s.voc[f] = a.fdesc[2 * F + f];
      s.pad[f] = a.fdesc[3 * F + f];
    }
  }
}

// base[f] = x_f * F (or -1 for a negative index) of sample b
template <typename IdxT>
__device__ __forceinline__ void stage_sample(const FfmArgs& a, FfmShared& s, int64_t b) {
  for (int f = threadIdx.x; f < a.F; f += RH_BLOCK) {
    const IdxT* ip = reinterpret_cast<const IdxT*>(a.idesc[f]);
    const int64_t x = (int64_t)ip[b * a.idesc[a.F + f]];
    s.base[f] = x < 0 ? -1 : x * a.F;
  }
}

// row of pair side (i, j) of the current sample: valid -> table row, else row 0 (read) and ok = false
__device__ __forceinline__ int64_t side_row(const FfmShared& s, int i, int j, bool& ok) {
  const int64_t r = s.base[i] + j;
  ok = s.base[i] >= 0 && r < s.voc[i];
  return ok ? r : 0;
}

template <bool TABLE, typename IdxT>
__global__ __launch_bounds__(RH_BLOCK) void ffm_fwd_kernel(const FfmArgs a) {
  __shared__ FfmShared s;
  stage_pairs<TABLE>(a, s);
  const int F = a.F, D = a.D, Dp = a.Dp;
  const int P = F * (F - 1) / 2;
  bool oob = false;
  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    __syncthreads();  // (the previous sample is done with base[])
    if (TABLE) stage_sample<IdxT>(a, s, b);
    __syncthreads();
    const float* xb = TABLE ? nullptr : a.x + b * a.xs;
    float* ob = a.out + b * a.ld_out;
    if (a.reduce) {  // one lane per pair, sum over d (reference: torch.sum(dim=-1) of the products)
      for (int p = threadIdx.x; p < P; p += RH_BLOCK) {
        const int i = s.pi[p], j = s.pj[p];
        const float *ra, *rc;
        if (TABLE) {
          bool oka, okc;
          ra = s.tab[i] + side_row(s, i, j, oka) * Dp;
          rc = s.tab[j] + side_row(s, j, i, okc) * Dp;
          oob |= !(oka && okc);
        } else {
          ra = xb + (int64_t)(i * F + j) * D;
          rc = xb + (int64_t)(j * F + i) * D;
        }
        float t = 0.f;
        for (int d = 0; d < D; ++d) t = fmaf(ra[d], rc[d], t);
        ob[p] = t;
      }
      continue;
    }
    for (int e = threadIdx.x; e < P * D; e += RH_BLOCK) {
      const int p = e / D, d = e - p * D;
      const int i = s.pi[p], j = s.pj[p];
      float va, vc;
      if (TABLE) {
        bool oka, okc;
        va = s.tab[i][side_row(s, i, j, oka) * Dp + d];
        vc = s.tab[j][side_row(s, j, i, okc) * Dp + d];
        oob |= !(oka && okc);
      } else {
        va = xb[(int64_t)(i * F + j) * D + d];
        vc = xb[(int64_t)(j * F + i) * D + d];
      }
      ob[e] = va * vc;  // one product per element: bit-exact against float32 numpy
    }
  }
  if (oob && a.err != nullptr) atomicOr(a.err, RH_FLAG_INDEX_OOB);
}

// d em[b,p,d] / d T_i[x_i F + j, d] = T_j[x_j F + i, d] (and the roles swapped); dense mode: dX[b,i,j] / dX[b,j,i],
// the diagonal zero.  Table mode: float atomics on the logical columns only (PaddedEmbedding's padding stays 0), rows
// at padding_idx dropped; every row gets exactly ONE contribution per sample.  Sink mode: plain stores of whole Dp rows.
template <bool TABLE, typename IdxT>
__global__ __launch_bounds__(RH_BLOCK) void ffm_bwd_kernel(const FfmArgs a) {
  __shared__ FfmShared s;
  stage_pairs<TABLE>(a, s);
  const int F = a.F, D = a.D, Dp = a.Dp;
  const int P = F * (F - 1) / 2;
  const int V = F * (F - 1);
  const int W = (TABLE && a.sink) ? Dp : D;  // columns walked per pair
  bool oob = false;
  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    __syncthreads();
    if (TABLE) stage_sample<IdxT>(a, s, b);
    __syncthreads();
    const float* xb = TABLE ? nullptr : a.x + b * a.xs;
    const float* gb = a.g + b * a.ld_g;
    for (int e = threadIdx.x; e < P * W; e += RH_BLOCK) {
      const int p = e / W, d = e - p * W;
      const int i = s.pi[p], j = s.pj[p];
      const bool live = d < D;
      const float g = live ? (a.reduce ? gb[p] : gb[p * D + d]) : 0.f;
      if (TABLE) {
        bool oka, okc;
        const int64_t ra = side_row(s, i, j, oka), rc = side_row(s, j, i, okc);
        oob |= !(oka && okc);
        const float va = live ? s.tab[i][ra * Dp + d] : 0.f;
        const float vc = live ? s.tab[j][rc * Dp + d] : 0.f;
        if (a.sink) {
          a.rows[(b * V + i * (F - 1) + j - 1) * Dp + d] = g * vc;  // v(i, j), j > i
          a.rows[(b * V + j * (F - 1) + i) * Dp + d] = g * va;      // v(j, i), i < j
        } else {
          if (oka && ra != s.pad[i] && s.grad[i] != nullptr) gatomic_add_f32(s.grad[i] + ra * Dp + d, g * vc);
          if (okc && rc != s.pad[j] && s.grad[j] != nullptr) gatomic_add_f32(s.grad[j] + rc * Dp + d, g * va);
        }
      } else {
        const int64_t oa = (int64_t)(i * F + j) * D + d, oc = (int64_t)(j * F + i) * D + d;
        float* gxb = a.gx + b * a.ld_gx;
        gxb[oa] = g * xb[oc];
        gxb[oc] = g * xb[oa];
      }
    }
    if (!TABLE) {
      float* gxb = a.gx + b * a.ld_gx;
      for (int e = threadIdx.x; e < F * D; e += RH_BLOCK) {
        const int f = e / D, d = e - f * D;
        gxb[(int64_t)(f * F + f) * D + d] = 0.f;
      }
    }
  }
  if (oob && a.err != nullptr) atomicOr(a.err, RH_FLAG_INDEX_OOB);
}

// xv[b, v(i,j)] = x_i * F + j for the F(F-1) virtual fields, v(i,j) = i (F-1) + (j < i ? j : j - 1)
template <typename IdxT>
__global__ __launch_bounds__(RH_BLOCK) void ffm_expand_kernel(const int64_t* __restrict__ idesc, int B, int F,
                                                              IdxT* __restrict__ xv) {
  const int V = F * (F - 1);
  const int64_t n = (int64_t)B * V;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    const int64_t b = e / V;
    const int v = (int)(e - b * V);
    const int i = v / (F - 1), r = v - i * (F - 1);
    const int j = r < i ? r : r + 1;
    const IdxT* ip = reinterpret_cast<const IdxT*>(idesc[i]);
    xv[e] = (IdxT)(ip[b * idesc[F + i]] * (IdxT)F + (IdxT)j);
  }
}

// ---- CEN ------------------------------------------------------------------------------------------------------------
// d[b,p] = relu(sum_d u[p,d] em[b,p,d])
__global__ __launch_bounds__(RH_BLOCK) void cen_desc_fwd_kernel(const float* __restrict__ em, int64_t ld,
                                                                const float* __restrict__ u, int B, int P, int D,
                                                                float* __restrict__ dout) {
  const int64_t n = (int64_t)B * P;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    const int64_t b = e / P;
    const int p = (int)(e - b * P);
    const float* r = em + b * ld + (int64_t)p * D;
    const float* w = u + (int64_t)p * D;
    float t = 0.f;
    for (int d = 0; d < D; ++d) t = fmaf(w[d], r[d], t);
    dout[e] = fmaxf(t, 0.f);
  }
}

// g_em[b,c] = relu'(d[b,p]) g_d[b,p] u[c]  (c = p*D + d), and per chunk of kCenRows samples the partial
// u_partial[chunk, c] = sum over the chunk's samples IN ORDER of relu'(d) g_d em[b,c]: deterministic, no atomics.
__global__ __launch_bounds__(RH_BLOCK) void cen_desc_bwd_kernel(const float* __restrict__ em, int64_t ld,
                                                                const float* __restrict__ u,
                                                                const float* __restrict__ dv,
                                                                const float* __restrict__ gd, int B, int P, int D,
                                                                float* __restrict__ g_em,
                                                                float* __restrict__ u_partial) {
  const int C = P * D;
  const int c = blockIdx.y * RH_BLOCK + threadIdx.x;
  if (c >= C) return;
  const int p = c / D;
  const float uc = u[c];
  const int64_t b0 = (int64_t)blockIdx.x * kCenRows;
  const int64_t b1 = b0 + kCenRows < B ? b0 + kCenRows : B;
  float acc = 0.f;
  for (int64_t b = b0; b < b1; ++b) {
    const float gg = dv[b * P + p] > 0.f ? gd[b * P + p] : 0.f;
    g_em[b * C + c] = gg * uc;
    acc = fmaf(gg, em[b * ld + c], acc);
  }
  u_partial[(int64_t)blockIdx.x * C + c] = acc;
}

// aem[b, p*D + d] = s[b,p] em[b, p*D + d]
__global__ __launch_bounds__(RH_BLOCK) void cen_rescale_fwd_kernel(const float* __restrict__ em, int64_t ld,
                                                                   const float* __restrict__ sv, int B, int P, int D,
                                                                   float* __restrict__ out) {
  const int C = P * D;
  const int64_t n = (int64_t)B * C;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    const int64_t b = e / C;
    const int c = (int)(e - b * C);
    out[e] = sv[b * P + c / D] * em[b * ld + c];
  }
}

// g_em = s g ; g_s[b,p] = sum_d g em   (one lane per (b, p))
__global__ __launch_bounds__(RH_BLOCK) void cen_rescale_bwd_kernel(const float* __restrict__ em, int64_t ld,
                                                                   const float* __restrict__ sv,
                                                                   const float* __restrict__ g, int64_t ldg, int B,
                                                                   int P, int D, float* __restrict__ g_em,
                                                                   float* __restrict__ g_s) {
  const int64_t n = (int64_t)B * P;
  const int C = P * D;
  for (int64_t e = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * RH_BLOCK) {
    const int64_t b = e / P;
    const int p = (int)(e - b * P);
    const float* r = em + b * ld + (int64_t)p * D;
    const float* gr = g + b * ldg + (int64_t)p * D;
    float* o = g_em + b * C + (int64_t)p * D;
    const float s = sv[e];
    float t = 0.f;
    for (int d = 0; d < D; ++d) {
      const float gv = gr[d];
      o[d] = s * gv;
      t = fmaf(gv, r[d], t);
    }
    g_s[e] = t;
  }
}

unsigned grid_for(int64_t n) {
  int64_t g = (n + RH_BLOCK - 1) / RH_BLOCK;
  if (g > 8192) g = 8192;
  return (unsigned)(g < 1 ? 1 : g);
}

unsigned sample_grid(int B) { return (unsigned)(B < 4096 ? B : 4096); }

int check_shape(const char* who, int B, int F, int D, int Dp) {
  RH_REQUIRE(B >= 0, RH_E_BADARG, "%s: bad batch size %d", who, B);
  RH_REQUIRE(F >= 2 && F <= kMaxF, RH_E_UNSUPPORTED, "%s: num_fields %d unsupported (2 .. %d)", who, F, kMaxF);
  RH_REQUIRE(D >= 1 && D <= kMaxD, RH_E_UNSUPPORTED, "%s: embed_dim %d unsupported (1 .. %d)", who, D, kMaxD);
  RH_REQUIRE(Dp >= D && Dp <= kMaxD, RH_E_UNSUPPORTED, "%s: row width %d unsupported (embed_dim .. %d)", who, Dp, kMaxD);
  return 0;
}

}  // namespace

extern "C" int rh_ffm_expand_index(const int64_t* idesc, int idx_is_i64, int B, int F, void* out, void* stream) {
  RH_REQUIRE(idesc && out, RH_E_BADARG, "rh_ffm_expand_index: null argument");
  if (int rc = check_shape("rh_ffm_expand_index", B, F, 1, 1)) return rc;
  if (B == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((int64_t)B * F * (F - 1));
  if (idx_is_i64)
    hipLaunchKernelGGL(ffm_expand_kernel<int64_t>, dim3(grid), dim3(RH_BLOCK), 0, st, idesc, B, F, (int64_t*)out);
  else
    hipLaunchKernelGGL(ffm_expand_kernel<int32_t>, dim3(grid), dim3(RH_BLOCK), 0, st, idesc, B, F, (int32_t*)out);
  RH_LAUNCH_CHECK("rh_ffm_expand_index");
  return 0;
}

extern "C" int rh_ffm_fwd(const int64_t* fdesc, const int64_t* idesc, int idx_is_i64, const float* x, int64_t x_stride,
                          int B, int F, int D, int Dp, int reduce_sum, float* out, int64_t out_stride, int32_t* err_flag,
                          void* stream) {
  const bool table = fdesc != nullptr;
  RH_REQUIRE(out && (table ? (idesc != nullptr && x == nullptr) : (x != nullptr && idesc == nullptr)), RH_E_BADARG,
             "rh_ffm_fwd: pass either (fdesc, idesc) or x");
  if (int rc = check_shape("rh_ffm_fwd", B, F, D, table ? Dp : D)) return rc;
  if (B == 0) return 0;
  FfmArgs a{fdesc, idesc, x, x_stride, B, F, D, table ? Dp : D, reduce_sum ? 1 : 0, out, out_stride,
            nullptr, 0, nullptr, 0, 0, nullptr, err_flag};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = sample_grid(B);
  if (!table)
    hipLaunchKernelGGL((ffm_fwd_kernel<false, int64_t>), dim3(grid), dim3(RH_BLOCK), 0, st, a);
  else if (idx_is_i64)
    hipLaunchKernelGGL((ffm_fwd_kernel<true, int64_t>), dim3(grid), dim3(RH_BLOCK), 0, st, a);
  else
    hipLaunchKernelGGL((ffm_fwd_kernel<true, int32_t>), dim3(grid), dim3(RH_BLOCK), 0, st, a);
  RH_LAUNCH_CHECK("rh_ffm_fwd");
  return 0;
}

extern "C" int rh_ffm_bwd(const int64_t* fdesc, const int64_t* idesc, int idx_is_i64, const float* x, int64_t x_stride,
                          int B, int F, int D, int Dp, int reduce_sum, const float* g, int64_t g_stride, float* g_x,
                          int64_t gx_stride, int sink, float* rows, int32_t* err_flag, void* stream) {
  const bool table = fdesc != nullptr;
  RH_REQUIRE(g && (table ? (idesc != nullptr && x == nullptr && (!sink || rows)) : (x != nullptr && g_x != nullptr)),
             RH_E_BADARG, "rh_ffm_bwd: pass either (fdesc, idesc[, rows]) or (x, g_x)");
  if (int rc = check_shape("rh_ffm_bwd", B, F, D, table ? Dp : D)) return rc;
  if (B == 0) return 0;
  FfmArgs a{fdesc, idesc, x, x_stride, B, F, D, table ? Dp : D, reduce_sum ? 1 : 0, nullptr, 0,
            g, g_stride, g_x, gx_stride, table && sink ? 1 : 0, rows, err_flag};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = sample_grid(B);
  if (!table)
    hipLaunchKernelGGL((ffm_bwd_kernel<false, int64_t>), dim3(grid), dim3(RH_BLOCK), 0, st, a);
  else if (idx_is_i64)
    hipLaunchKernelGGL((ffm_bwd_kernel<true, int64_t>), dim3(grid), dim3(RH_BLOCK), 0, st, a);
  else
    hipLaunchKernelGGL((ffm_bwd_kernel<true, int32_t>), dim3(grid), dim3(RH_BLOCK), 0, st, a);
  RH_LAUNCH_CHECK("rh_ffm_bwd");
  return 0;
}

extern "C" int rh_cen_nchunks(int B) { return B <= 0 ? 0 : (B + kCenRows - 1) / kCenRows; }

extern "C" int rh_cen_desc_fwd(const float* em, int64_t ld, const float* u, int B, int P, int D, float* d_out,
                               void* stream) {
  RH_REQUIRE(em && u && d_out && B >= 0 && P >= 1 && D >= 1 && D <= kMaxD, RH_E_BADARG, "rh_cen_desc_fwd: bad arguments");
  if (B == 0) return 0;
  hipLaunchKernelGGL(cen_desc_fwd_kernel, dim3(grid_for((int64_t)B * P)), dim3(RH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), em, ld, u, B, P, D, d_out);
  RH_LAUNCH_CHECK("rh_cen_desc_fwd");
  return 0;
}

extern "C" int rh_cen_desc_bwd(const float* em, int64_t ld, const float* u, const float* d, const float* g_d, int B,
                               int P, int D, float* g_em, float* u_partial, void* stream) {
  RH_REQUIRE(em && u && d && g_d && g_em && u_partial && B >= 0 && P >= 1 && D >= 1 && D <= kMaxD, RH_E_BADARG,
             "rh_cen_desc_bwd: bad arguments");
  if (B == 0) return 0;
  const dim3 grid((unsigned)rh_cen_nchunks(B), (unsigned)((P * D + RH_BLOCK - 1) / RH_BLOCK));
  hipLaunchKernelGGL(cen_desc_bwd_kernel, grid, dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), em, ld, u, d,
                     g_d, B, P, D, g_em, u_partial);
  RH_LAUNCH_CHECK("rh_cen_desc_bwd");
  return 0;
}

extern "C" int rh_cen_rescale_fwd(const float* em, int64_t ld, const float* s, int B, int P, int D, float* out,
                                  void* stream) {
  RH_REQUIRE(em && s && out && B >= 0 && P >= 1 && D >= 1, RH_E_BADARG, "rh_cen_rescale_fwd: bad arguments");
  if (B == 0) return 0;
  hipLaunchKernelGGL(cen_rescale_fwd_kernel, dim3(grid_for((int64_t)B * P * D)), dim3(RH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), em, ld, s, B, P, D, out);
  RH_LAUNCH_CHECK("rh_cen_rescale_fwd");
  return 0;
}

extern "C" int rh_cen_rescale_bwd(const float* em, int64_t ld, const float* s, const float* g, int64_t ldg, int B, int P,
                                  int D, float* g_em, float* g_s, void* stream) {
  RH_REQUIRE(em && s && g && g_em && g_s && B >= 0 && P >= 1 && D >= 1, RH_E_BADARG, "rh_cen_rescale_bwd: bad arguments");
  if (B == 0) return 0;
  hipLaunchKernelGGL(cen_rescale_bwd_kernel, dim3(grid_for((int64_t)B * P)), dim3(RH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), em, ld, s, g, ldg, B, P, D, g_em, g_s);
  RH_LAUNCH_CHECK("rh_cen_rescale_bwd");
  return 0;
}
