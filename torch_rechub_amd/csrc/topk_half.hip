// The flat top-K scan and the inverted-file list scan over an fp16 or bf16 item table (rh_topk_half_fwd,
// rh_ivf_scan_half): half the bytes per item, so twice the catalogue beside a resident model.  The kernels are
// topk_scan_kernel / ivf_scan_kernel with the scan body of topk_half_tile.h (v_mfma_f32_32x32x16_f16 / _bf16, q rounded
// to the table's type in registers, the item tile double-buffered in LDS) under the same rules (topk_rules.h), the same
// K-lists and partials, and topk_merge_row for the merge.  A score depends on q_i, x_j and D alone, so the result does
// not depend on nsplit, M, V or the tile position, and with every list probed the list scan equals the flat scan bit for
// bit, exactly as for the f32 table.  No atomics, no scratch: two runs give the same bits.
#include "topk_half_tile.h"
#include "topk_rules.h"

namespace {

static_assert(kTopkMaxSplit >= kIvfMaxProbe, "one merge kernel holds the heads of either scan's lists");

// vec: bit 0 = 16-byte loads of the table are legal, bit 1 = of q
template <typename T>
__global__ __launch_bounds__(RH_BLOCK) void topk_half_scan_kernel(const TopkArgs a, int vec) {
  extern __shared__ __align__(16) float lds[];
  int64_t lo, hi;
  const FlatRule rule = topk_flat_rule(a, lo, hi);
  topk_half_scan_tiles<T>(a.s, rule, lo, hi, lds, (vec & 1) != 0, (vec & 2) != 0);
}

template <typename T>
__global__ __launch_bounds__(RH_BLOCK) void ivf_half_scan_kernel(const IvfArgs a, int vec) {
  extern __shared__ __align__(16) float lds[];
  const TopkScanArgs& s = a.s;
  int* prs = reinterpret_cast<int*>(lds + topk_half_lds_bytes(s.K) / sizeof(float));  // [64] pair index of the row
  int64_t lo, hi;
  if (!ivf_tile(a, prs, lo, hi)) return;
  topk_half_scan_tiles<T>(s, IvfRule{prs, a.row_id, s.nlist, s.K}, lo, hi, lds, (vec & 1) != 0, (vec & 2) != 0);
}

template <typename T>
int launch_flat(const TopkArgs& a, hipStream_t st) {
  static RhLdsReserved reserved;
  if (int rc = rh_reserve_lds(reserved, topk_half_scan_kernel<T>, topk_half_lds_bytes(128), "rh_topk_half_fwd")) return rc;
  const int64_t nrt = ((int64_t)a.s.M + a.s.RB - 1) / a.s.RB;
  hipLaunchKernelGGL(topk_half_scan_kernel<T>, dim3((unsigned)nrt, a.s.nlist), dim3(RH_BLOCK), topk_half_lds_bytes(a.s.K),
                     st, a, vec_flags(a.s));
  return 0;
}

template <typename T>
int launch_ivf(const IvfArgs& a, int64_t grid, hipStream_t st) {
  static RhLdsReserved reserved;
  if (int rc = rh_reserve_lds(reserved, ivf_half_scan_kernel<T>, ivf_half_lds_bytes(128), "rh_ivf_scan_half")) return rc;
  hipLaunchKernelGGL(ivf_half_scan_kernel<T>, dim3((unsigned)grid), dim3(RH_BLOCK), ivf_half_lds_bytes(a.s.K), st, a,
                     vec_flags(a.s));
  return 0;
}

bool table_type_ok(int is_bf16) { return is_bf16 == 0 || is_bf16 == 1; }

}  // namespace

extern "C" int rh_topk_half_supported(int D, int K, int S, int is_bf16, int* supported) {
  RH_REQUIRE(supported != nullptr, RH_E_BADARG, "rh_topk_half_supported: null pointer");
  *supported = topk_shape_ok(D, K, S) && table_type_ok(is_bf16) ? 1 : 0;
  return 0;
}

extern "C" int rh_topk_half_fwd(const float* q, int64_t ldq, const void* x, int is_bf16, const float* bias,
                                const int64_t* exclude, int S, const int64_t* invalid, int n_inv, int M, int D, int V, int K,
                                int nsplit, void* workspace, int64_t* ids, float* scores, void* stream) {
  RH_REQUIRE(table_type_ok(is_bf16), RH_E_UNSUPPORTED, "rh_topk_half_fwd: is_bf16=%d is neither 0 (fp16) nor 1 (bf16)",
             is_bf16);
  TopkArgs a{};
  bool go;
  if (int rc = topk_flat_args("rh_topk_half_fwd", &a, &go, q, ldq, x, bias, exclude, S, invalid, n_inv, M, D, V, K, nsplit,
                              workspace, ids, scores))
    return rc;
  if (!go) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = is_bf16 == 0 ? launch_flat<TableF16>(a, st) : launch_flat<TableBf16>(a, st)) return rc;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)M), dim3(RH_WAVE), 0, st, a.s);
  RH_LAUNCH_CHECK("rh_topk_half_fwd");
  return 0;
}

extern "C" int rh_ivf_scan_half(const float* q, int64_t ldq, const void* xs, int is_bf16, const float* bias_s,
                                const int32_t* row_id, const int32_t* list_off, int nlists, const int32_t* pair,
                                const int32_t* pair_off, const int32_t* tile_off, const int64_t* exclude, int S, int M, int D,
                                int V, int K, int nprobe, void* partials, int64_t* ids, float* scores, void* stream) {
  RH_REQUIRE(table_type_ok(is_bf16), RH_E_UNSUPPORTED, "rh_ivf_scan_half: is_bf16=%d is neither 0 (fp16) nor 1 (bf16)",
             is_bf16);
  IvfArgs a{};
  bool go;
  int64_t grid;
  if (int rc = ivf_scan_args("rh_ivf_scan_half", &a, &go, &grid, q, ldq, xs, bias_s, row_id, list_off, nlists, pair,
                             pair_off, tile_off, exclude, S, M, D, V, K, nprobe, partials, ids, scores))
    return rc;
  if (!go) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = is_bf16 == 0 ? launch_ivf<TableF16>(a, grid, st) : launch_ivf<TableBf16>(a, grid, st)) return rc;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)M), dim3(RH_WAVE), 0, st, a.s);
  RH_LAUNCH_CHECK("rh_ivf_scan_half");
  return 0;
}
