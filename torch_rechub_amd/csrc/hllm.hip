// HLLM (generative next-item model): causal softmax multi-head attention with an additive per-head bucketed
// relative-position bias and dropout on the attention weights, forward and backward.
//
// Reference HLLMTransformerBlock.forward torch_rechub/models/generative/hllm.py:69-88 with RelPosBias.forward
// utils/hstu_utils.py:54-68:
//   S[i, j] = scale q_i . k_j + table[bucket(i, j), h]  for j <= i,  -inf above the diagonal,
//   bucket(i, j) = min(|i - j|, N) * (nb - 1) / N  (integers),  P = softmax_j S,  O = dropout(P) V.
// The reference materialises the (B, H, L, L) scores, the masked scores, the softmax, the dropout mask and its product
// in fp32 and keeps them for autograd.  Here the flash-style tile kernels of softmax_attn_tile.h do it (the plan, the
// head widths, the dropout and the bias reduction are described there); this file supplies their rule for HLLM -- one
// length, the key tiles up to the diagonal and the query tiles from it down, the scale, the linear buckets evaluated in
// place, diagonals indexed i - j -- and the entry points with their checks and launches.  No mask test, no key-tile scan
// and no LDS beyond the tiles: the rule's Lds is empty.
#include "softmax_attn_tile.h"

namespace {

struct HllmRule {
  static constexpr int kFwdWaves = 0;
  static constexpr int kMaxDiag = kMaxL;
  struct Lds {};

  static __device__ __forceinline__ int key_tiles(const AttnArgs&, int qt) { return qt + 1; }
  static __device__ __forceinline__ int first_query_tile(const AttnArgs&, int kt) { return kt; }
  static __device__ __forceinline__ bool scan_keys(Lds&, const AttnArgs&, int, int) { return false; }
  static __device__ __forceinline__ bool has_key(const Lds&, int) { return true; }
  static __device__ __forceinline__ void stage_bias(Lds&, const AttnArgs&, int, int, int, int) {}
  static __device__ __forceinline__ bool key_ok(const AttnArgs&, int, int) { return true; }

  static __device__ __forceinline__ int diag(const AttnArgs&, int dji) { return -dji; }
  static __device__ __forceinline__ int bucket(const AttnArgs& a, int d) {
    d = d < a.N ? d : a.N;
    return (int)((int64_t)d * (a.nb - 1) / a.N);
  }
  // scale q_i . k_j + bias, for j <= i < L
  static __device__ __forceinline__ float logit(const AttnArgs& a, float s, int i, int j, int h) {
    float x = s * a.scale;
    if (a.bias) x += a.bias[(int64_t)bucket(a, i - j) * a.H + h];
    return x;
  }
  static __device__ __forceinline__ float score(const Lds&, const AttnArgs& a, bool, float s, int i, int j, int, int, int h) {
    return (i < a.Lq && j <= i) ? logit(a, s, i, j, h) : -INFINITY;
  }
  static __device__ __forceinline__ float lse(float rm, float rl) { return rm + logf(rl); }
  static __device__ __forceinline__ float uniform_weight(const AttnArgs&) { return 0.f; }
  template <class F>
  static __device__ __forceinline__ void with_weight(const Lds&, const AttnArgs& a, bool, float, float s, int i, int j, int,
                                                     int, int h, float lse, F use) {
    if (i < a.Lq && j <= i) use(expf(logit(a, s, i, j, h) - lse));
  }
  static __device__ __forceinline__ float grad_scale(const AttnArgs& a) { return a.scale; }
};

int sattn_check(const char* name, const AttnArgs& a) {
  if (int rc = attn_check(name, a)) return rc;
  RH_REQUIRE(a.B >= 0 && a.H >= 1 && a.N >= 1 && a.Lq >= 1 && a.Lq <= kMaxL && a.Lq <= a.N, RH_E_UNSUPPORTED,
             "%s: L=%d H=%d unsupported (1 <= L <= min(max_seq_len=%d, %d), H >= 1)", name, a.Lq, a.H, a.N, kMaxL);
  RH_REQUIRE(a.ldq >= (int64_t)a.H * a.dh, RH_E_BADARG, "%s: row stride %lld too small", name, (long long)a.ldq);
  return 0;
}

AttnArgs sattn_args(const float* q, const float* k, const float* v, int64_t ld, int B, int L, int H, int dh,
                    const float* bias, int N, int nb, float scale, float p_drop, const int64_t* rng,
                    const int64_t* saved_ctr, const float* out, const float* lse) {
  AttnArgs a = attn_args(q, ld, k, v, ld, B, L, L, H, dh, bias, nb, L, p_drop, rng, saved_ctr, out, lse);
  a.N = N;
  a.scale = scale;
  return a;
}

}  // namespace

extern "C" int rh_softmax_attn_nparts(int B, int L, int H) { return B * H * ((L + kT - 1) / kT) + H; }

extern "C" int rh_softmax_attn_fwd(const float* q, const float* k, const float* v, int64_t ld, int B, int L, int H, int dh,
                                   const float* bias, int N, int nb, float scale, float p_drop, int64_t* rng,
                                   int64_t* saved_ctr, float* out, float* lse, void* stream) {
  AttnArgs a = sattn_args(q, k, v, ld, B, L, H, dh, bias, N, nb, scale, p_drop, rng, saved_ctr, out, lse);
  a.fwd = 1;
  if (int rc = sattn_check("rh_softmax_attn_fwd", a)) return rc;
  RH_REQUIRE(out && lse, RH_E_BADARG, "rh_softmax_attn_fwd: null output");
  if (B == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nqt = (L + kT - 1) / kT;
  hipLaunchKernelGGL(softmax_attn_fwd_kernel<HllmRule>, dim3(B * H, nqt), dim3(RH_BLOCK), 0, st, a);
  if (p_drop > 0.f) hipLaunchKernelGGL(drop_advance_kernel, dim3(1), dim3(1), 0, st, rng);
  RH_LAUNCH_CHECK("rh_softmax_attn_fwd");
  return 0;
}

extern "C" int rh_softmax_attn_bwd(const float* q, const float* k, const float* v, int64_t ld, int B, int L, int H, int dh,
                                   const float* bias, int N, int nb, float scale, float p_drop, const int64_t* rng,
                                   const int64_t* saved_ctr, const float* out, const float* lse, const float* g_out,
                                   float* delta, float* g_q, float* g_k, float* g_v, int64_t ldg, float* part,
                                   float* g_bias, void* stream) {
  AttnArgs a = sattn_args(q, k, v, ld, B, L, H, dh, bias, N, nb, scale, p_drop, rng, saved_ctr, out, lse);
  attn_bwd_args(a, g_out, delta, g_q, ldg, g_k, g_v, ldg, part, g_bias);
  if (int rc = sattn_check("rh_softmax_attn_bwd", a)) return rc;
  RH_REQUIRE(out && lse && g_out && delta && g_q && g_k && g_v && (!bias || (part && g_bias)), RH_E_BADARG,
             "rh_softmax_attn_bwd: null pointer");
  RH_REQUIRE(ldg >= (int64_t)H * dh, RH_E_BADARG, "rh_softmax_attn_bwd: gradient row stride %lld too small", (long long)ldg);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nqt = (L + kT - 1) / kT;
  if (B > 0) {
    const int64_t n = (int64_t)B * H * L;
    int grid = (int)((n + RH_BLOCK - 1) / RH_BLOCK);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(softmax_attn_delta_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a);
    hipLaunchKernelGGL(softmax_attn_dkv_kernel<HllmRule>, dim3(B * H, nqt), dim3(RH_BLOCK), 0, st, a);
    hipLaunchKernelGGL(softmax_attn_dq_kernel<HllmRule>, dim3(B * H, nqt), dim3(RH_BLOCK), 0, st, a);
  }
  if (bias) {
    const int64_t n1 = (int64_t)H * L, n2 = (int64_t)nb * H;
    hipLaunchKernelGGL(softmax_attn_diag_kernel, dim3((int)((n1 + RH_BLOCK - 1) / RH_BLOCK)), dim3(RH_BLOCK), 0, st, a, nqt);
    hipLaunchKernelGGL(softmax_attn_bias_kernel<HllmRule>, dim3((int)((n2 + RH_BLOCK - 1) / RH_BLOCK)), dim3(RH_BLOCK), 0, st, a,
                       nqt);
  }
  RH_LAUNCH_CHECK("rh_softmax_attn_bwd");
  return 0;
}
