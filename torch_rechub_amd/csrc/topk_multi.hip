// Multi-interest top-K retrieval (rh_topk_multi_*): q (M, I, D) holds one vector per interest of a user, as MIND,
// ComiRec-DR / -SA and SINE return them, and every user gets ONE K-list: the top K of max_i (q[u,i] . x_j + qbias[u,i])
// + bias[j] -- the merged, de-duplicated union of the I per-interest lists, which the reference's evaluation forms on the
// host with a sort per user (the definition, the equivalence and why the bias may follow the fold: topk_multi_tile.h).
// Scan kernel: a workgroup owns U = min(64 / Ip, topk_rows(K)) users (Ip = the next power of two >= I tile rows each) and
// one of nsplit column ranges; the 64 x 64 score tile is folded over the interests in the accumulator registers, only the
// (U x 64) folded tile goes to LDS, and the K-list stage of topk_list.h runs once per user.  Partials are (M, nsplit, K)
// per USER; the merge is topk_merge_row.  fp32 tables run on v_mfma_f32_32x32x2_f32, fp16 / bf16 tables on
// v_mfma_f32_32x32x16_f16 / _bf16 (q rounded to the table's type as topk_half.hip rounds it).  The order, the tie rule,
// exclude (per user), invalid, the (-1, -inf) tail and the independence of nsplit are rh_topk_fwd's.  No atomics, no
// scratch: two runs give the same bits.
#include "topk_multi_tile.h"

namespace {

static_assert(RH_LISTWISE_MAX_I == 16, "the fold covers Ip = 1, 2, 4, 8, 16: at most half a 32-row accumulator quadrant");
constexpr int kMultiMaxI = RH_LISTWISE_MAX_I;

template <typename P>
size_t multi_lds_bytes(int U, int K) { return (size_t)P::kStage + (size_t)U * K * 8 + (size_t)2 * kT * 4; }

// vec (the half producers): bit 0 = 16-byte loads of the table are legal, bit 1 = of q
template <typename P>
__global__ __launch_bounds__(RH_BLOCK, P::kWaves) void topk_multi_scan_kernel(const TopkMultiArgs a, int vec) {
  extern __shared__ __align__(16) float lds[];
  topk_multi_scan_tiles<P>(a, lds, vec);
}

bool multi_shape_ok(int D, int K, int S, int I) { return topk_shape_ok(D, K, S) && I >= 1 && I <= kMultiMaxI; }

// Everything up to the launch, whatever the table's type.  *go = there is something to launch (M > 0).
int multi_args(const char* who, TopkMultiArgs* a, bool* go, const float* q, int64_t ldq, int I, const float* qbias,
               const void* x, const float* bias, const int64_t* exclude, int S, const int64_t* invalid, int n_inv, int M,
               int D, int V, int K, int nsplit, void* workspace, int64_t* ids, float* scores) {
  *go = false;
  RH_REQUIRE(I >= 1 && I <= kMultiMaxI, RH_E_UNSUPPORTED, "%s: I=%d unsupported (1 <= I <= %d)", who, I, kMultiMaxI);
  RH_REQUIRE((int64_t)M * I < ((int64_t)1 << 31), RH_E_UNSUPPORTED, "%s: M I = %lld interest rows are too many", who,
             (long long)M * I);
  if (int rc = topk_flat_args(who, &a->f, go, q, ldq, x, bias, exclude, S, invalid, n_inv, M, D, V, K, nsplit, workspace,
                              ids, scores))
    return rc;
  a->f.s.RB = topk_multi_users(I, K);
  a->qbias = qbias;
  a->I = I;
  a->sh = topk_multi_shift(I);
  return 0;
}

template <typename P>
int launch(const TopkMultiArgs& a, int vec, const char* who, hipStream_t st) {
  const TopkScanArgs& s = a.f.s;
  static RhLdsReserved reserved;
  if (int rc = rh_reserve_lds(reserved, topk_multi_scan_kernel<P>, multi_lds_bytes<P>(kT, 128), who)) return rc;
  const int64_t nrt = ((int64_t)s.M + s.RB - 1) / s.RB;
  hipLaunchKernelGGL(topk_multi_scan_kernel<P>, dim3((unsigned)nrt, s.nlist), dim3(RH_BLOCK), multi_lds_bytes<P>(s.RB, s.K),
                     st, a, vec);
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)s.M), dim3(RH_WAVE), 0, st, s);
  return 0;
}

}  // namespace

extern "C" int rh_topk_multi_supported(int D, int K, int S, int I, int* supported) {
  RH_REQUIRE(supported != nullptr, RH_E_BADARG, "rh_topk_multi_supported: null pointer");
  *supported = multi_shape_ok(D, K, S, I) ? 1 : 0;
  return 0;
}

extern "C" int rh_topk_multi_plan(int M, int I, int V, int K, int* nsplit, int64_t* workspace_bytes) {
  RH_REQUIRE(nsplit != nullptr && workspace_bytes != nullptr, RH_E_BADARG, "rh_topk_multi_plan: null pointer");
  RH_REQUIRE(M >= 0 && V >= 1, RH_E_BADARG, "rh_topk_multi_plan: M=%d V=%d (M >= 0, V >= 1)", M, V);
  RH_REQUIRE(K >= 1 && K <= kTopkMaxK && I >= 1 && I <= kMultiMaxI, RH_E_UNSUPPORTED,
             "rh_topk_multi_plan: K=%d I=%d unsupported (1 <= K <= %d, 1 <= I <= %d)", K, I, kTopkMaxK, kMultiMaxI);
  *nsplit = topk_default_split(M, V, topk_multi_users(I, K));
  *workspace_bytes = (int64_t)M * *nsplit * K * 8;
  return 0;
}

extern "C" int rh_topk_multi_fwd(const float* q, int64_t ldq, int I, const float* qbias, const float* x, const float* bias,
                                 const int64_t* exclude, int S, const int64_t* invalid, int n_inv, int M, int D, int V,
                                 int K, int nsplit, void* workspace, int64_t* ids, float* scores, void* stream) {
  TopkMultiArgs a{};
  bool go;
  if (int rc = multi_args("rh_topk_multi_fwd", &a, &go, q, ldq, I, qbias, x, bias, exclude, S, invalid, n_inv, M, D, V, K,
                          nsplit, workspace, ids, scores))
    return rc;
  if (!go) return 0;
  if (int rc = launch<MultiTileF32>(a, 0, "rh_topk_multi_fwd", reinterpret_cast<hipStream_t>(stream))) return rc;
  RH_LAUNCH_CHECK("rh_topk_multi_fwd");
  return 0;
}

extern "C" int rh_topk_multi_half_fwd(const float* q, int64_t ldq, int I, const float* qbias, const void* x, int is_bf16,
                                      const float* bias, const int64_t* exclude, int S, const int64_t* invalid, int n_inv,
                                      int M, int D, int V, int K, int nsplit, void* workspace, int64_t* ids, float* scores,
                                      void* stream) {
  RH_REQUIRE(is_bf16 == 0 || is_bf16 == 1, RH_E_UNSUPPORTED,
             "rh_topk_multi_half_fwd: is_bf16=%d is neither 0 (fp16) nor 1 (bf16)", is_bf16);
  TopkMultiArgs a{};
  bool go;
  if (int rc = multi_args("rh_topk_multi_half_fwd", &a, &go, q, ldq, I, qbias, x, bias, exclude, S, invalid, n_inv, M, D, V,
                          K, nsplit, workspace, ids, scores))
    return rc;
  if (!go) return 0;
  const TopkScanArgs& s = a.f.s;
  const int vec = vec_flags(s);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = is_bf16 == 0 ? launch<MultiTileHalf<TableF16>>(a, vec, "rh_topk_multi_half_fwd", st)
                            : launch<MultiTileHalf<TableBf16>>(a, vec, "rh_topk_multi_half_fwd", st))
    return rc;
  RH_LAUNCH_CHECK("rh_topk_multi_half_fwd");
  return 0;
}
