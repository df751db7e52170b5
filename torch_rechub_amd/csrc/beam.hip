// One step of TIGER's constrained beam search over a flat trie (rh_beam_step; replaces, per decoding step of
// TIGERModel.generate, the host walk of the constraint callback, the dense (B K, V) mask, the log-softmax over it and
// torch.topk over (B, K V)).
//
// One workgroup of 256 threads per query, one launch per step, no workspace.
// Phase 1, the rows' log-sum-exp: the four wavefronts take the query's K logits rows round-robin.  Lane l owns the
// elements of the float4 groups l, l + 64, ... (dword-aligned 16-byte loads: a row's alignment changes nothing) and then
// the elements l, l + 64, ... of the last V % 256; it takes their maximum, the wavefront the maximum of the lanes, and in
// a second walk (the row is 4 V bytes, read again from the cache) every lane adds expf(x - max) over its elements in that
// same order and the wavefront adds the lanes in the butterfly's fixed order.  Which lane holds which element follows from
// the index in the row and V alone, so (max, log(sum)) depends on the row's V values and on nothing else -- not on the
// query, the beam, B or the stride.  expf / logf are the accurate ones: the selection depends on these values.  A dead
// beam's row is not read.
// Phase 2, the candidates, by wavefront 0 with the K-list of topk_list.h in LDS: beams in ascending order, the edges of a
// beam's node in ascending order (= ascending token), 64 edges at a time; lane j holds the score running + ((logit - max)
// - log(sum)) of edge j, the ballot against the list's K-th score picks the hits and topk_row_hits inserts them.  The
// walk is in ascending (beam, token), so an equal score goes behind and never displaces the K-th: the list is the top K
// under (score descending, beam ascending, token ascending).  A list entry's id packs (beam, offset of the edge in its
// node); the write-out turns it back into (parent, token, child node).
// LDS: 2 x 64 floats of (max, log(sum)) and 64 (score, id) pairs: 1 KiB.  No atomics: two runs give the same bits.
#include "topk_list.h"

namespace {

constexpr int kBeamMaxK = RH_BEAM_MAX_K;     // one list chunk per wavefront; a beam index takes 6 bits of an id
constexpr int kBeamEdgeBits = 25; // the offset of an edge inside its node takes the other 25 (distinct tokens: < V)

struct BeamArgs {
  const float* logits;
  int64_t ld;
  const float* running;
  const int32_t* node;
  const int32_t* child_off;
  const int32_t* child_tok;
  const int32_t* child_node;
  int n_nodes, K, V;
  float* running_out;
  int32_t* parent_out;
  int32_t* tok_out;
  int32_t* node_out;
  int32_t* short_out;
};

static __device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, RH_WAVE));
  return v;
}

__global__ __launch_bounds__(RH_BLOCK) void beam_step_kernel(const BeamArgs a) {
  __shared__ float row_max[kBeamMaxK], row_log[kBeamMaxK];
  __shared__ float ls[kBeamMaxK];
  __shared__ int li[kBeamMaxK];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int K = a.K, V = a.V;
  const int64_t q0 = (int64_t)blockIdx.x * K;  // the query's first beam row
  const int nv = V / (4 * RH_WAVE);            // float4 sweeps of the wavefront
  for (int k = w; k < K; k += RH_BLOCK / RH_WAVE) {
    const int nd = a.node[q0 + k];
    if (nd < 0 || nd >= a.n_nodes) continue;  // (wavefront-uniform)
    const float* row = a.logits + (q0 + k) * a.ld;
    float m = -INFINITY;
    for (int i = 0; i < nv; ++i) {
      const float4 x = gload<float4>(row + ((int64_t)i * RH_WAVE + lane) * 4);
      m = fmaxf(fmaxf(m, fmaxf(x.x, x.y)), fmaxf(x.z, x.w));
    }
    for (int c = nv * 4 * RH_WAVE + lane; c < V; c += RH_WAVE) m = fmaxf(m, row[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int i = 0; i < nv; ++i) {
      const float4 x = gload<float4>(row + ((int64_t)i * RH_WAVE + lane) * 4);
      s += expf(x.x - m);
      s += expf(x.y - m);
      s += expf(x.z - m);
      s += expf(x.w - m);
    }
    for (int c = nv * 4 * RH_WAVE + lane; c < V; c += RH_WAVE) s += expf(row[c] - m);
    s = wave_sum(s);
    if (lane == 0) {
      row_max[k] = m;
      row_log[k] = logf(s);
    }
  }
  __syncthreads();
  if (w != 0) return;
  int n = 0;
  float t = -INFINITY;
  for (int k = 0; k < K; ++k) {
    const int nd = a.node[q0 + k];
    if (nd < 0 || nd >= a.n_nodes) continue;
    const int lo = a.child_off[nd];
    int hi = a.child_off[nd + 1];
    if (hi - lo > (1 << kBeamEdgeBits)) hi = lo + (1 << kBeamEdgeBits);  // (unreachable with distinct tokens below V)
    const float* row = a.logits + (q0 + k) * a.ld;
    const float r = a.running[q0 + k], m = row_max[k], lg = row_log[k];
    for (int e0 = lo; e0 < hi; e0 += RH_WAVE) {
      const int e = e0 + lane;
      const int tok = e < hi ? a.child_tok[e] : -1;
      const bool ok = (unsigned)tok < (unsigned)V;  // a token outside the row is no candidate (and is not read)
      const float s = ok ? r + ((row[tok] - m) - lg) : -INFINITY;
      const uint64_t hits = __ballot(ok && s > -INFINITY && (n < K || s > t));
      if (hits == 0) continue;
      topk_row_hits(hits, s, ls, li, n, t, K, 1, nullptr, 0, nullptr, 0, lane,
                    [&](int j) { return (int64_t)((k << kBeamEdgeBits) | (e0 - lo + j)); });
    }
  }
  wave_sync();
  if (lane < K) {
    float s = -INFINITY;
    int parent = -1, tok = -1, child = -1;
    if (lane < n) {
      const int id = li[lane];
      parent = id >> kBeamEdgeBits;
      const int e = a.child_off[a.node[q0 + parent]] + (id & ((1 << kBeamEdgeBits) - 1));
      s = ls[lane];
      tok = a.child_tok[e];
      child = a.child_node[e];
    }
    a.running_out[q0 + lane] = s;
    a.parent_out[q0 + lane] = parent;
    a.tok_out[q0 + lane] = tok;
    a.node_out[q0 + lane] = child;
  }
  if (lane == 0) a.short_out[blockIdx.x] = n < K ? 1 : 0;
}

// [p, p + n) and [q, q + m) share a byte
bool beam_overlap(const void* p, int64_t n, const void* q, int64_t m) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)m && b < a + (uintptr_t)n;
}

}  // namespace

extern "C" int rh_beam_step(const float* logits, int64_t ld, const float* running, const int32_t* node,
                            const int32_t* child_off, const int32_t* child_tok, const int32_t* child_node, int n_nodes, int B,
                            int K, int V, float* running_out, int32_t* parent_out, int32_t* tok_out, int32_t* node_out,
                            int32_t* short_out, void* stream) {
  RH_REQUIRE(K >= 1 && K <= kBeamMaxK && V >= 1 && V <= (1 << kBeamEdgeBits) && B >= 0 && n_nodes >= 1 &&
                 (int64_t)B * K <= INT32_MAX,
             RH_E_BADARG, "rh_beam_step: B=%d K=%d V=%d n_nodes=%d (1 <= K <= %d, 1 <= V <= 2^%d, n_nodes >= 1, B K < 2^31)", B,
             K, V, n_nodes, kBeamMaxK, kBeamEdgeBits);
  RH_REQUIRE(ld >= V, RH_E_BADARG, "rh_beam_step: row stride ld=%lld below V=%d", (long long)ld, V);
  RH_REQUIRE(logits && running && node && child_off && child_tok && child_node && running_out && parent_out && tok_out &&
                 node_out && short_out,
             RH_E_BADARG, "rh_beam_step: null pointer");
  if (B == 0) return 0;
  const int64_t rows = (int64_t)B * K;
  const void* outs[5] = {running_out, parent_out, tok_out, node_out, short_out};
  for (int i = 0; i < 5; ++i) {
    const int64_t bytes = 4 * (i < 4 ? rows : (int64_t)B);
    RH_REQUIRE(!beam_overlap(outs[i], bytes, logits, 4 * ((rows - 1) * ld + V)) && !beam_overlap(outs[i], bytes, running, 4 * rows) &&
                   !beam_overlap(outs[i], bytes, node, 4 * rows),
               RH_E_BADARG, "rh_beam_step: an output aliases an input");
  }
  const BeamArgs a{logits, ld, running, node, child_off, child_tok, child_node, n_nodes, K, V,
                   running_out, parent_out, tok_out, node_out, short_out};
  hipLaunchKernelGGL(beam_step_kernel, dim3((unsigned)B), dim3(RH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
  RH_LAUNCH_CHECK("rh_beam_step");
  return 0;
}
