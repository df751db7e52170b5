// int8 item tables (SQ8) for the flat top-K scan and the inverted-file list scan (rh_topk_q8_fwd, rh_ivf_scan_q8), and the
// one quantisation rule that builds the table and quantises every batch of queries (rh_quantize_rows_q8): a quarter of
// the fp32 bytes per item.  The scan kernels are topk_scan_kernel / ivf_scan_kernel with the scan body of topk_q8_tile.h
// (v_mfma_i32_32x32x32_i8, the query codes in registers, the item tile double-buffered in LDS) under the same rules
// (topk_rules.h), the same K-lists and partials, and topk_merge_row for the merge.  The integer sum is exact, the two
// scale multiplications and the bias addition are single rounded f32 operations in a fixed order: a score depends on
// q_i, x_j and D alone, so the result does not depend on nsplit, M, V or the tile position, and with every list probed
// the list scan equals the flat scan bit for bit.  No atomics, no scratch: two runs give the same bits.
#include "topk_q8_tile.h"
#include "topk_rules.h"

namespace {

static_assert(kTopkMaxSplit >= kIvfMaxProbe, "one merge kernel holds the heads of either scan's lists");
static_assert(127 * 127 * kTopkMaxD < (1 << 24), "the i32 sum of a score converts to f32 exactly");

// One wavefront per row: m = max |x|, scale = m / 127 (1 for a zero row), code = clamp(rint(x / scale), -127, 127), both
// divisions correctly rounded, columns [D, ldc) zero.  Four columns per lane and trip: xvec = 16-byte loads of x are
// legal (ldx % 4 == 0, aligned), cvec = dword stores of the codes are (ldc % 4 == 0, aligned).
__global__ __launch_bounds__(RH_BLOCK) void quantize_rows_q8_kernel(const float* x, int64_t ldx, int M, int D, int8_t* codes,
                                                                    int64_t ldc, float* scale, int xvec, int cvec) {
  const int lane = threadIdx.x % RH_WAVE;
  const int64_t row = (int64_t)blockIdx.x * (RH_BLOCK / RH_WAVE) + threadIdx.x / RH_WAVE;
  if (row >= M) return;
  const float* xr = x + row * ldx;
  auto load4 = [&](int k, float (&f)[4]) {
    if (xvec && k + 4 <= D) {
      const float4 u = *reinterpret_cast<const float4*>(xr + k);
      f[0] = u.x, f[1] = u.y, f[2] = u.z, f[3] = u.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = k + j < D ? xr[k + j] : 0.f;
    }
  };
  float m = 0.f;
  for (int k = 4 * lane; k < D; k += 4 * RH_WAVE) {
    float f[4];
    load4(k, f);
#pragma unroll
    for (int j = 0; j < 4; ++j) m = fmaxf(m, fabsf(f[j]));
  }
#pragma unroll
  for (int s = RH_WAVE / 2; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, RH_WAVE));
  const float sc = m == 0.f ? 1.f : __fdiv_rn(m, 127.f);
  if (lane == 0) scale[row] = sc;
  int8_t* cr = codes + row * ldc;
  for (int64_t k = 4 * lane; k < ldc; k += 4 * RH_WAVE) {
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if (k < D) load4((int)k, f);
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = (int)fminf(fmaxf(rintf(__fdiv_rn(f[j], sc)), -127.f), 127.f);
      packed |= (uint32_t)(c & 0xff) << (8 * j);
    }
    if (cvec) {
      *reinterpret_cast<uint32_t*>(cr + k) = packed;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (k + j < ldc) cr[k + j] = (int8_t)(packed >> (8 * j));
    }
  }
}

template <bool kOneChunk>
__global__ __launch_bounds__(RH_BLOCK) void topk_q8_scan_kernel(const TopkArgs a, const Q8Scales sc, int xvec) {
  extern __shared__ __align__(16) float lds[];
  int64_t lo, hi;
  const FlatRule rule = topk_flat_rule(a, lo, hi);
  topk_q8_scan_tiles<kOneChunk>(a.s, sc, rule, lo, hi, lds, xvec != 0);
}

template <bool kOneChunk>
__global__ __launch_bounds__(RH_BLOCK) void ivf_q8_scan_kernel(const IvfArgs a, const Q8Scales sc, int xvec) {
  extern __shared__ __align__(16) float lds[];
  const TopkScanArgs& s = a.s;
  int* prs = reinterpret_cast<int*>(lds + topk_half_lds_bytes(s.K) / sizeof(float));  // [64] pair index of the row
  int64_t lo, hi;
  if (!ivf_tile(a, prs, lo, hi)) return;
  topk_q8_scan_tiles<kOneChunk>(s, sc, IvfRule{prs, a.row_id, s.nlist, s.K}, lo, hi, lds, xvec != 0);
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// the query codes as the scan body loads them, and the two scale pointers
int q8_operands(const char* who, const int8_t* qc, int64_t ldqc, const float* qs, const float* xs, int M) {
  RH_REQUIRE(ldqc % 16 == 0 && aligned16(qc), RH_E_BADARG,
             "%s: the query codes need a row stride that is a multiple of 16 (ldqc=%lld) and a 16-byte aligned base", who,
             (long long)ldqc);
  RH_REQUIRE(M <= 0 || (qs && xs), RH_E_BADARG, "%s: null pointer", who);
  return 0;
}

int xvec_flag(const TopkScanArgs& s) { return s.D % 16 == 0 && aligned16(s.x) ? 1 : 0; }

// kOneChunk: D <= 128 (topk_q8_tile.h)
template <bool kOneChunk>
int launch_flat(const TopkArgs& a, const Q8Scales& sc, hipStream_t st) {
  static RhLdsReserved reserved;
  if (int rc = rh_reserve_lds(reserved, topk_q8_scan_kernel<kOneChunk>, topk_half_lds_bytes(128), "rh_topk_q8_fwd")) return rc;
  const int64_t nrt = ((int64_t)a.s.M + a.s.RB - 1) / a.s.RB;
  hipLaunchKernelGGL(topk_q8_scan_kernel<kOneChunk>, dim3((unsigned)nrt, a.s.nlist), dim3(RH_BLOCK),
                     topk_half_lds_bytes(a.s.K), st, a, sc, xvec_flag(a.s));
  return 0;
}

template <bool kOneChunk>
int launch_ivf(const IvfArgs& a, const Q8Scales& sc, int64_t grid, hipStream_t st) {
  static RhLdsReserved reserved;
  if (int rc = rh_reserve_lds(reserved, ivf_q8_scan_kernel<kOneChunk>, ivf_half_lds_bytes(128), "rh_ivf_scan_q8")) return rc;
  hipLaunchKernelGGL(ivf_q8_scan_kernel<kOneChunk>, dim3((unsigned)grid), dim3(RH_BLOCK), ivf_half_lds_bytes(a.s.K), st, a, sc,
                     xvec_flag(a.s));
  return 0;
}

}  // namespace

extern "C" int rh_quantize_rows_q8(const float* x, int64_t ldx, int M, int D, int8_t* codes, int64_t ldc, float* scale,
                                   void* stream) {
  RH_REQUIRE(M >= 0 && D >= 1 && ldx >= D && ldc >= D, RH_E_BADARG, "rh_quantize_rows_q8: M=%d D=%d ldx=%lld ldc=%lld", M, D,
             (long long)ldx, (long long)ldc);
  if (M == 0) return 0;
  RH_REQUIRE(x && codes && scale, RH_E_BADARG, "rh_quantize_rows_q8: null pointer");
  const int per = RH_BLOCK / RH_WAVE;
  const int xvec = ldx % 4 == 0 && aligned16(x) ? 1 : 0;
  const int cvec = ldc % 4 == 0 && reinterpret_cast<uintptr_t>(codes) % 4 == 0 ? 1 : 0;
  hipLaunchKernelGGL(quantize_rows_q8_kernel, dim3((unsigned)((M + per - 1) / per)), dim3(RH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), x, ldx, M, D, codes, ldc, scale, xvec, cvec);
  RH_LAUNCH_CHECK("rh_quantize_rows_q8");
  return 0;
}

extern "C" int rh_topk_q8_supported(int D, int K, int S, int* supported) {
  RH_REQUIRE(supported != nullptr, RH_E_BADARG, "rh_topk_q8_supported: null pointer");
  *supported = topk_shape_ok(D, K, S) ? 1 : 0;
  return 0;
}

extern "C" int rh_topk_q8_fwd(const int8_t* qc, int64_t ldqc, const float* qs, const int8_t* xc, const float* xs,
                              const float* bias, const int64_t* exclude, int S, const int64_t* invalid, int n_inv, int M,
                              int D, int V, int K, int nsplit, void* workspace, int64_t* ids, float* scores, void* stream) {
  TopkArgs a{};
  bool go;
  if (int rc = topk_flat_args("rh_topk_q8_fwd", &a, &go, reinterpret_cast<const float*>(qc), ldqc, xc, bias, exclude, S,
                              invalid, n_inv, M, D, V, K, nsplit, workspace, ids, scores))
    return rc;
  if (int rc = q8_operands("rh_topk_q8_fwd", qc, ldqc, qs, xs, M)) return rc;
  if (!go) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const Q8Scales sc{qs, xs};
  if (int rc = D <= kQ8Chunk ? launch_flat<true>(a, sc, st) : launch_flat<false>(a, sc, st)) return rc;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)M), dim3(RH_WAVE), 0, st, a.s);
  RH_LAUNCH_CHECK("rh_topk_q8_fwd");
  return 0;
}

extern "C" int rh_ivf_scan_q8(const int8_t* qc, int64_t ldqc, const float* qs, const int8_t* xc_s, const float* xs_s,
                              const float* bias_s, const int32_t* row_id, const int32_t* list_off, int nlists,
                              const int32_t* pair, const int32_t* pair_off, const int32_t* tile_off, const int64_t* exclude,
                              int S, int M, int D, int V, int K, int nprobe, void* partials, int64_t* ids, float* scores,
                              void* stream) {
  IvfArgs a{};
  bool go;
  int64_t grid;
  if (int rc = ivf_scan_args("rh_ivf_scan_q8", &a, &go, &grid, reinterpret_cast<const float*>(qc), ldqc, xc_s, bias_s,
                             row_id, list_off, nlists, pair, pair_off, tile_off, exclude, S, M, D, V, K, nprobe, partials,
                             ids, scores))
    return rc;
  if (int rc = q8_operands("rh_ivf_scan_q8", qc, ldqc, qs, xs_s, M)) return rc;
  if (!go) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const Q8Scales sc{qs, xs_s};
  if (int rc = D <= kQ8Chunk ? launch_ivf<true>(a, sc, grid, st) : launch_ivf<false>(a, sc, grid, st)) return rc;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)M), dim3(RH_WAVE), 0, st, a.s);
  RH_LAUNCH_CHECK("rh_ivf_scan_q8");
  return 0;
}
