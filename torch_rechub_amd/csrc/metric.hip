// Evaluation metrics on the device (rh_auc_*, rh_gauc_reduce, rh_log_loss, rh_rank_metrics; replaces the host loops of the
// reference's basic/metric.py: roc_auc_score, the per-user dict of gauc_score, the quadruple loop of topk_metrics).  The
// beyond-accuracy metrics (rh_ild, rh_coverage, rh_novelty) have their own section at the end of the file.
//
// Rank statistic.  The caller sorts (group, prediction) ascending (torch.sort over the int64 keys of rh_auc_keys: plumbing)
// and hands the permutation `order` over.  With Npre[k] = the negatives among the first k sorted elements, a positive i of
// group g adds   2 #{neg of g below i} + #{neg of g tied with i} = Npre[start of i's tie run] + Npre[end of i's tie run]
//                                                                  - 2 Npre[start of g]
// to U2_g: three prefix counts, all integers.  A chunk of 1024 sorted elements is one trip of a workgroup; its elements
// become four 64-bit ballot masks per wavefront (negative, positive, "starts a tie run", "starts a group"), so every
// position lookup is a bit search and every prefix count a popcount over LDS.  Runs and groups that cross chunk borders:
//   launch 1 (auc_agg_kernel)   per chunk: negatives, the negatives ahead of its first run border and of its last run /
//                               group border, whether it is one run / one group, whether it opens with a border;
//   launch 2 (auc_scan_kernel)  ONE workgroup, fixed order: the chunks' exclusive prefix P[c], and three carried values --
//                               Npre at the start of the run / group that reaches INTO chunk c, Npre at the end of the run
//                               that reaches OUT of it -- each a copy-scan "take your own value at a border, else your
//                               neighbour's", forwards twice and backwards once;
//   launch 3 (auc_emit_kernel)  per chunk again: the positives' terms, an int64 scan over the chunk, and for every group
//                               segment of the chunk one 64-bit integer atomic each into P_g, N_g, U2_g.
// Integer sums do not depend on the order of arrival: two runs give the same bits.  No float atomics anywhere.
//
// rh_gauc_reduce / rh_log_loss: double terms, one partial per workgroup over a grid that depends on the size alone, the
// partials added in index order by one workgroup: bit-reproducible.
//
// rh_rank_metrics: one wavefront per user, lane l owns the positions l, l + 64, l + 128, l + 192 of the K <= 256
// recommended ids.  The user's truth list goes through LDS kRankStage ids at a time; every lane compares its ids with the
// staged ones (one LDS address per step for the whole wavefront: a broadcast).  Per cut-off the hits are four ballot
// masks; dcg is their bits walked low to high, adding gain[j] in double -- the reference's own order of additions.  A
// wavefront's running sums over its users sit in LDS (in registers they cost 80 per lane and a third of the occupancy).
#include <math.h>

#include "common.h"

namespace {

constexpr int kAucChunk = 1024, kAucWords = kAucChunk / 64, kAucItems = kAucChunk / RH_BLOCK, kAucMaxGrid = 2048;
constexpr int kAucAgg = 5;    // int32 per chunk: neg, head_n, tail_run, tail_grp, flags
constexpr int kAucCarry = 4;  // int64 per chunk: P, run_in, grp_in, run_out
constexpr int kFullRun = 1, kFullGrp = 2, kOpensRun = 4, kOpensGrp = 8;
// rechub_hip.h documents the `partial` of rh_gauc_reduce as 3072 doubles and that of rh_log_loss as 1024, and callers
// allocate exactly that; the kernels write 3 and 1 doubles per workgroup of a grid of at most kReduceMaxGrid
constexpr int kReduceMaxGrid = 1024;
static_assert(3 * kReduceMaxGrid <= 3072, "rh_gauc_reduce writes past the 3072 doubles its contract gives it");
static_assert(kReduceMaxGrid <= 1024, "rh_log_loss writes past the 1024 doubles its contract gives it");
// the list kernels (rank metrics, ild, novelty): one wavefront per user, at most kListMaxCut cut-offs over K <= kListMaxK
constexpr int kListUsers = RH_BLOCK / RH_WAVE, kListMaxK = RH_RANK_MAX_K, kListMaxCut = RH_RANK_MAX_CUTOFFS, kListPer = kListMaxK / RH_WAVE;
constexpr int kListMaxGrid = 2048;  // ild, novelty
constexpr int kRankStage = 256, kRankMaxGrid = 1024, kRankSums = 4;
constexpr int kSumParts = 32;

typedef unsigned long long u64;

// workgroups for `count` items at `per` a workgroup: at least one, at most `cap` (what is left over is further trips)
int grid_for(int64_t count, int per, int cap) {
  const int64_t b = (count + per - 1) / per;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

struct AucArgs {
  const uint32_t* pred;  // float32 bit patterns, element stride ps
  int64_t ps;
  const void* label;
  int ldt;               // 0 float32, 1 float64, 2 int64, 3 uint8 / bool
  const int64_t* g;      // dense group ids or null (one group)
  const int64_t* order;
  int64_t n, G, nchunks;
  int32_t* agg;          // (nchunks, kAucAgg)
  int64_t* carry;        // (nchunks, kAucCarry)
  u64* out;              // (3, G): P, N, U2
  u64* bad;              // (2,): non-finite predictions, labels that are neither 0 nor 1 (and group ids outside [0, G))
};

struct AucLds {
  uint64_t neg[kAucWords], pos[kAucWords], runb[kAucWords], grpb[kAucWords];
  int negpre[kAucWords + 1], pospre[kAucWords + 1];
  int64_t wpre[kAucWords + 1];
  int64_t u2pre[kAucChunk + 1];
};

// value equality: -0.0 and +0.0 are one value, every other bit pattern (denormals included) is its own
__device__ __forceinline__ uint32_t canon(uint32_t b) { return (b << 1) == 0 ? 0u : b; }

// 1 = positive, 0 = negative, -1 = neither
__device__ __forceinline__ int label_class(const void* p, int dt, int64_t i) {
  switch (dt) {
    case 0: {
      const float v = static_cast<const float*>(p)[i];
      return v == 1.f ? 1 : (v == 0.f ? 0 : -1);
    }
    case 1: {
      const double v = static_cast<const double*>(p)[i];
      return v == 1.0 ? 1 : (v == 0.0 ? 0 : -1);
    }
    case 2: {
      const int64_t v = static_cast<const int64_t*>(p)[i];
      return v == 1 ? 1 : (v == 0 ? 0 : -1);
    }
    default: {
      const uint8_t v = static_cast<const uint8_t*>(p)[i];
      return v == 1 ? 1 : (v == 0 ? 0 : -1);
    }
  }
}

// highest set bit at a position <= t, or -1
__device__ __forceinline__ int last_set_le(const uint64_t* m, int t) {
  int w = t >> 6;
  uint64_t x = m[w] & (~0ull >> (63 - (t & 63)));
  while (true) {
    if (x != 0) return w * 64 + 63 - __clzll((long long)x);
    if (--w < 0) return -1;
    x = m[w];
  }
}

// lowest set bit at a position > t, or -1
__device__ __forceinline__ int first_set_gt(const uint64_t* m, int t) {
  const int p = t + 1;
  if (p >= kAucChunk) return -1;
  int w = p >> 6;
  uint64_t x = m[w] & (~0ull << (p & 63));
  while (true) {
    if (x != 0) return w * 64 + __ffsll((unsigned long long)x) - 1;
    if (++w >= kAucWords) return -1;
    x = m[w];
  }
}

// set bits at positions < p, 0 <= p <= kAucChunk
__device__ __forceinline__ int count_below(const int* pre, const uint64_t* m, int p) {
  const int w = p >> 6;
  if (w >= kAucWords) return pre[kAucWords];
  return pre[w] + __popcll(m[w] & ((1ull << (p & 63)) - 1));
}

// The chunk's four masks and the word prefix counts, in LDS.  gsel[j] = the group of the thread's j-th element (-1: none to
// write to).  Ends with a workgroup barrier; the caller puts another one before the next chunk overwrites the masks.
template <bool COUNT>
__device__ __forceinline__ void auc_load_chunk(const AucArgs& a, int64_t c, AucLds& L, int64_t gsel[kAucItems], u64& nbad0,
                                               u64& nbad1) {
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int64_t base = c * kAucChunk;
#pragma unroll
  for (int j = 0; j < kAucItems; ++j) {
    const int64_t i = base + j * RH_BLOCK + tid;
    const bool valid = i < a.n;
    uint32_t pb = 0;
    int64_t gg = -1;
    int cls = 0;
    bool oob = false;
    if (valid) {
      int64_t o = a.order[i];
      if ((u64)o >= (u64)a.n) {
        o = 0;
        oob = true;
      }
      pb = a.pred[o * a.ps];
      gg = a.g != nullptr ? a.g[o] : 0;
      cls = label_class(a.label, a.ldt, o);
      oob |= gg < 0 || gg >= a.G;
    }
    const bool nonfinite = valid && (pb & 0x7f800000u) == 0x7f800000u;
    pb = canon(pb);
    uint32_t ppb = __shfl_up(pb, 1, RH_WAVE);
    int64_t pg = __shfl_up(gg, 1, RH_WAVE);
    if (lane == 0 && valid && i > 0) {  // the element before the wavefront's first
      int64_t o = a.order[i - 1];
      if ((u64)o >= (u64)a.n) o = 0;
      ppb = canon(a.pred[o * a.ps]);
      pg = a.g != nullptr ? a.g[o] : 0;
    }
    const bool gb = valid && (i == 0 || gg != pg);
    const bool rb = gb || (valid && pb != ppb);
    const uint64_t m_pos = __ballot(valid && cls == 1), m_neg = __ballot(valid && cls != 1);
    const uint64_t m_run = __ballot(rb), m_grp = __ballot(gb);
    if (COUNT) {
      nbad0 += __popcll(__ballot(nonfinite));
      nbad1 += __popcll(__ballot(valid && (cls < 0 || oob)));
    }
    if (lane == 0) {
      const int word = j * (RH_BLOCK / RH_WAVE) + w;
      L.pos[word] = m_pos;
      L.neg[word] = m_neg;
      L.runb[word] = m_run;
      L.grpb[word] = m_grp;
    }
    gsel[j] = (valid && !oob) ? gg : -1;
  }
  __syncthreads();
  if (tid == 0) {
    int sn = 0, sp = 0;
    for (int k = 0; k < kAucWords; ++k) {
      L.negpre[k] = sn;
      L.pospre[k] = sp;
      sn += __popcll(L.neg[k]);
      sp += __popcll(L.pos[k]);
    }
    L.negpre[kAucWords] = sn;
    L.pospre[kAucWords] = sp;
  }
  __syncthreads();
}

__global__ __launch_bounds__(RH_BLOCK) void auc_agg_kernel(const AucArgs a) {
  __shared__ AucLds L;
  u64 nbad0 = 0, nbad1 = 0;
  int64_t gsel[kAucItems];
  for (int64_t c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    auc_load_chunk<true>(a, c, L, gsel, nbad0, nbad1);
    if (threadIdx.x == 0) {
      const int64_t left = a.n - c * kAucChunk;
      const int len = left < kAucChunk ? (int)left : kAucChunk;
      const int neg = L.negpre[kAucWords];
      const int fb = first_set_gt(L.runb, 0), lb = last_set_le(L.runb, len - 1);
      const int fg = first_set_gt(L.grpb, 0), lg = last_set_le(L.grpb, len - 1);
      int32_t* ag = a.agg + c * kAucAgg;
      ag[0] = neg;
      ag[1] = fb < 0 ? neg : count_below(L.negpre, L.neg, fb);   // negatives of the chunk's leading run
      ag[2] = lb >= 1 ? count_below(L.negpre, L.neg, lb) : 0;     // negatives ahead of its trailing run
      ag[3] = lg >= 1 ? count_below(L.negpre, L.neg, lg) : 0;     // negatives ahead of its trailing group
      ag[4] = (fb < 0 ? kFullRun : 0) | (fg < 0 ? kFullGrp : 0) | ((L.runb[0] & 1) ? kOpensRun : 0) |
              ((L.grpb[0] & 1) ? kOpensGrp : 0);
    }
    __syncthreads();
  }
  if (threadIdx.x % RH_WAVE == 0) {  // the ballots made the counts wavefront-uniform
    if (nbad0 != 0) atomicAdd(a.bad + 0, nbad0);
    if (nbad1 != 0) atomicAdd(a.bad + 1, nbad1);
  }
}

// ONE workgroup.  Thread k owns the chunks [k per, (k + 1) per); every scan is: a walk over the own range, thread 0 chaining
// the RH_BLOCK range results in index order, a second walk that writes.
__global__ __launch_bounds__(RH_BLOCK) void auc_scan_kernel(const AucArgs a) {
  __shared__ int64_t s0[RH_BLOCK + 1], s1[RH_BLOCK + 1];
  __shared__ int h0[RH_BLOCK], h1[RH_BLOCK];
  const int tid = threadIdx.x;
  const int64_t per = (a.nchunks + RH_BLOCK - 1) / RH_BLOCK;
  const int64_t lo = tid * per < a.nchunks ? tid * per : a.nchunks;
  const int64_t hi = lo + per < a.nchunks ? lo + per : a.nchunks;
  // P[c]: negatives ahead of chunk c
  int64_t sum = 0;
  for (int64_t c = lo; c < hi; ++c) sum += a.agg[c * kAucAgg];
  s0[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int k = 0; k < RH_BLOCK; ++k) {
      const int64_t v = s0[k];
      s0[k] = run;
      run += v;
    }
  }
  __syncthreads();
  sum = s0[tid];
  for (int64_t c = lo; c < hi; ++c) {
    a.carry[c * kAucCarry] = sum;
    sum += a.agg[c * kAucAgg];
  }
  __syncthreads();
  // forwards: S[c] = Npre at the start of chunk c's trailing run (group) = its own border's, or S[c - 1] when the chunk is
  // one run (group) that does not open with a border.  run_in[c] = S_run[c - 1], grp_in[c] = S_grp[c - 1].
  int64_t vr = 0, vg = 0;
  int hr = 0, hg = 0;
  for (int64_t c = lo; c < hi; ++c) {
    const int32_t* ag = a.agg + c * kAucAgg;
    const int f = ag[4];
    const int64_t P = a.carry[c * kAucCarry];
    if (!((f & kFullRun) && !(f & kOpensRun))) {
      vr = P + ag[2];
      hr = 1;
    }
    if (!((f & kFullGrp) && !(f & kOpensGrp))) {
      vg = P + ag[3];
      hg = 1;
    }
  }
  s0[tid + 1] = vr;
  s1[tid + 1] = vg;
  h0[tid] = hr;
  h1[tid] = hg;
  __syncthreads();
  if (tid == 0) {
    s0[0] = 0;
    s1[0] = 0;
    for (int k = 0; k < RH_BLOCK; ++k) {  // s[k + 1] = the value behind range k, s[k] the one that enters it
      if (!h0[k]) s0[k + 1] = s0[k];
      if (!h1[k]) s1[k + 1] = s1[k];
    }
  }
  __syncthreads();
  vr = s0[tid];
  vg = s1[tid];
  for (int64_t c = lo; c < hi; ++c) {
    const int32_t* ag = a.agg + c * kAucAgg;
    const int f = ag[4];
    const int64_t P = a.carry[c * kAucCarry];
    a.carry[c * kAucCarry + 1] = vr;
    a.carry[c * kAucCarry + 2] = vg;
    if (!((f & kFullRun) && !(f & kOpensRun))) vr = P + ag[2];
    if (!((f & kFullGrp) && !(f & kOpensGrp))) vg = P + ag[3];
  }
  __syncthreads();
  // backwards: E[c] = Npre at the end of chunk c's leading run = its own border's, or E[c + 1] when the chunk is one run and
  // chunk c + 1 does not open with a border.  run_out[c] = E[c + 1].
  vr = 0;
  hr = 0;
  for (int64_t c = hi - 1; c >= lo; --c) {
    const int32_t* ag = a.agg + c * kAucAgg;
    const bool through = (ag[4] & kFullRun) && c + 1 < a.nchunks && !(a.agg[(c + 1) * kAucAgg + 4] & kOpensRun);
    if (!through) {
      vr = a.carry[c * kAucCarry] + ag[1];
      hr = 1;
    }
  }
  s0[tid] = vr;
  h0[tid] = hr;
  __syncthreads();
  if (tid == 0) {
    s0[RH_BLOCK] = 0;
    for (int k = RH_BLOCK - 1; k >= 0; --k)  // s[k] = the value in front of range k, s[k + 1] the one that enters it from behind
      if (!h0[k]) s0[k] = s0[k + 1];
  }
  __syncthreads();
  vr = s0[tid + 1];
  for (int64_t c = hi - 1; c >= lo; --c) {
    const int32_t* ag = a.agg + c * kAucAgg;
    const bool through = (ag[4] & kFullRun) && c + 1 < a.nchunks && !(a.agg[(c + 1) * kAucAgg + 4] & kOpensRun);
    a.carry[c * kAucCarry + 3] = vr;
    if (!through) vr = a.carry[c * kAucCarry] + ag[1];
  }
}

__global__ __launch_bounds__(RH_BLOCK) void auc_emit_kernel(const AucArgs a) {
  __shared__ AucLds L;
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  u64 unused0 = 0, unused1 = 0;
  int64_t gsel[kAucItems];
  for (int64_t c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    auc_load_chunk<false>(a, c, L, gsel, unused0, unused1);
    const int64_t left = a.n - c * kAucChunk;
    const int len = left < kAucChunk ? (int)left : kAucChunk;
    const int64_t P = a.carry[c * kAucCarry], run_in = a.carry[c * kAucCarry + 1], grp_in = a.carry[c * kAucCarry + 2];
    const int64_t run_out = a.carry[c * kAucCarry + 3];
    const bool next_joins = c + 1 < a.nchunks && !(a.agg[(c + 1) * kAucAgg + 4] & kOpensRun);
    const int64_t chunk_end = P + L.negpre[kAucWords];
    int64_t incl[kAucItems], own[kAucItems];
#pragma unroll
    for (int j = 0; j < kAucItems; ++j) {
      const int word = j * (RH_BLOCK / RH_WAVE) + w, t = word * 64 + lane;
      int64_t u2 = 0;
      if ((L.pos[word] >> lane) & 1) {
        const int rs = last_set_le(L.runb, t), nb = first_set_gt(L.runb, t), gs = last_set_le(L.grpb, t);
        const int64_t n_rs = rs >= 0 ? P + count_below(L.negpre, L.neg, rs) : run_in;
        const int64_t n_re = nb >= 0 ? P + count_below(L.negpre, L.neg, nb) : (next_joins ? run_out : chunk_end);
        const int64_t n_gs = gs >= 0 ? P + count_below(L.negpre, L.neg, gs) : grp_in;
        u2 = n_rs + n_re - 2 * n_gs;
      }
      own[j] = u2;
#pragma unroll
      for (int d = 1; d < RH_WAVE; d <<= 1) {
        const int64_t o = __shfl_up(u2, d, RH_WAVE);
        if (lane >= d) u2 += o;
      }
      incl[j] = u2;
      if (lane == RH_WAVE - 1) L.wpre[word + 1] = u2;
    }
    __syncthreads();
    if (tid == 0) {
      L.wpre[0] = 0;
      for (int k = 0; k < kAucWords; ++k) L.wpre[k + 1] += L.wpre[k];
      L.u2pre[kAucChunk] = L.wpre[kAucWords];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kAucItems; ++j) {
      const int word = j * (RH_BLOCK / RH_WAVE) + w;
      L.u2pre[word * 64 + lane] = L.wpre[word] + incl[j] - own[j];
    }
    __syncthreads();
    // the last element of every group segment of the chunk adds the segment's three sums to its group
#pragma unroll
    for (int j = 0; j < kAucItems; ++j) {
      const int word = j * (RH_BLOCK / RH_WAVE) + w, t = word * 64 + lane;
      if (t >= len || gsel[j] < 0) continue;
      const bool ends = t == len - 1 || ((L.grpb[(t + 1) >> 6] >> ((t + 1) & 63)) & 1);
      if (!ends) continue;
      const int gs0 = last_set_le(L.grpb, t), gs = gs0 < 0 ? 0 : gs0;
      const int64_t sp = count_below(L.pospre, L.pos, t + 1) - count_below(L.pospre, L.pos, gs);
      const int64_t sn = count_below(L.negpre, L.neg, t + 1) - count_below(L.negpre, L.neg, gs);
      const int64_t su = L.u2pre[t + 1] - L.u2pre[gs];
      if (sp != 0) atomicAdd(a.out + gsel[j], (u64)sp);
      if (sn != 0) atomicAdd(a.out + a.G + gsel[j], (u64)sn);
      if (su != 0) atomicAdd(a.out + 2 * a.G + gsel[j], (u64)su);
    }
    __syncthreads();
  }
}

// sort key of (group, prediction): the group in the high word, below it the prediction's bit pattern made monotone
// (negative values: every bit flipped; others: the sign bit set), -0.0 and +0.0 sharing a key
__global__ __launch_bounds__(RH_BLOCK) void auc_keys_kernel(const uint32_t* pred, int64_t ps, const int64_t* g, int64_t n,
                                                            int64_t* keys) {
  for (int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * RH_BLOCK) {
    const uint32_t b = canon(pred[i * ps]);
    const uint32_t m = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    const int64_t gg = g != nullptr ? g[i] : 0;
    keys[i] = (int64_t)(((u64)gg << 32) | m);
  }
}

// sum of v over the workgroup, in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = RH_BLOCK / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(RH_BLOCK) void gauc_partial_kernel(const int64_t* stats, const double* weights, int64_t G,
                                                                double* partial) {
  __shared__ double red[RH_BLOCK];
  double num = 0.0, den = 0.0, single = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; i < G; i += (int64_t)gridDim.x * RH_BLOCK) {
    const int64_t P = stats[i], N = stats[G + i], U2 = stats[2 * G + i];
    const double wgt = weights != nullptr ? weights[i] : (double)(P + N);
    if (P == 0 || N == 0) {
      single += 1.0;
    } else {
      num += wgt * ((double)U2 / (2.0 * (double)P * (double)N));
      den += wgt;
    }
  }
  num = block_sum(num, red);
  den = block_sum(den, red);
  single = block_sum(single, red);
  if (threadIdx.x == 0) {
    partial[blockIdx.x * 3 + 0] = num;
    partial[blockIdx.x * 3 + 1] = den;
    partial[blockIdx.x * 3 + 2] = single;
  }
}

// ONE workgroup: the NV values of every per-workgroup partial, thread-strided adds in ascending index and then the
// block_sum tree; thread 0 hands the NV totals to `done`
template <int NV, typename Done>
__global__ __launch_bounds__(RH_BLOCK) void tree_final_kernel(const double* partial, int nblocks, const Done done) {
  __shared__ double red[RH_BLOCK];
  double v[NV];
  for (int k = 0; k < NV; ++k) v[k] = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += RH_BLOCK)
    for (int k = 0; k < NV; ++k) v[k] += partial[b * NV + k];
  for (int k = 0; k < NV; ++k) v[k] = block_sum(v[k], red);
  if (threadIdx.x == 0) done(v);
}

struct GaucDone {
  double* result;
  int64_t* single_class;
  __device__ void operator()(const double* v) const {
    result[0] = v[0];
    result[1] = v[1];
    single_class[0] = (int64_t)v[2];
  }
};

struct LogLossDone {
  double* result;
  int64_t n;
  __device__ void operator()(const double* v) const { result[0] = -v[0] / (double)n; }
};

__device__ __forceinline__ double label_value(const void* p, int dt, int64_t i) {
  switch (dt) {
    case 0: return (double)static_cast<const float*>(p)[i];
    case 1: return static_cast<const double*>(p)[i];
    case 2: return (double)static_cast<const int64_t*>(p)[i];
    default: return (double)static_cast<const uint8_t*>(p)[i];
  }
}

__global__ __launch_bounds__(RH_BLOCK) void log_loss_partial_kernel(const float* pred, int64_t ps, const void* label, int ldt,
                                                                    int64_t n, double* partial) {
  __shared__ double red[RH_BLOCK];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * RH_BLOCK) {
    const double p = (double)pred[i * ps], y = label_value(label, ldt, i);
    s += y * log(p) + (1.0 - y) * log(1.0 - p);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

struct ListCuts {
  int n_k;
  int cut[kListMaxCut];   // in the caller's order, or ascending (rh_ild)
  int slot[kListMaxCut];  // the position of cut[q] in the caller's list
};

struct RankArgs {
  const int64_t* pred;
  int64_t ld;
  int M, K;
  ListCuts c;  // in the caller's order
  const int64_t* off;
  const int64_t* ids;
  int64_t n_truth;
  const double* gain;   // (K,)
  const double* ideal;  // (K + 1,)
  double* partial;      // (gridDim.x, n_k, 4)
  u64* hits;            // (n_k,)
  u64* gts;             // (1,)
  double* per_user;     // (M, n_k, 5) or null
};

__device__ __forceinline__ void rank_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// butterfly sum over the 64 lanes, masks ascending: every lane gets the total through the same order of additions
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 1; m < RH_WAVE; m <<= 1) v += __shfl_xor(v, m, RH_WAVE);
  return v;
}

// A wavefront's running sums over its users, in two LDS arrays that the kernel declares: NS = W / kListMaxCut doubles per
// cut-off (wsum[w][q * NS + t]) and one exact count (wcnt[w][q]).
//   wave_acc_zero  the low lanes zero their wavefront's row; the caller syncs the wavefront (or the workgroup) behind it
//   wave_acc_add   called by ONE lane per user and cut-off, so that a wavefront adds user after user: a fixed order
//   wave_acc_tail  called by the whole workgroup: the counts leave as integer atomics, the wavefronts' sums are added in
//                  index order into the workgroup's partial (n_k * NS doubles)
template <int W>
__device__ __forceinline__ void wave_acc_zero(double (&wsum)[kListUsers][W], u64 (&wcnt)[kListUsers][kListMaxCut], int w,
                                              int lane) {
  if (lane < W) wsum[w][lane] = 0.0;
  if (lane < kListMaxCut) wcnt[w][lane] = 0;
}

template <int W>
__device__ __forceinline__ void wave_acc_add(double (&wsum)[kListUsers][W], u64 (&wcnt)[kListUsers][kListMaxCut], int w,
                                             int q, const double* v, u64 n) {
  constexpr int NS = W / kListMaxCut;
  wcnt[w][q] += n;
  for (int t = 0; t < NS; ++t) wsum[w][q * NS + t] += v[t];
}

template <int W>
__device__ __forceinline__ void wave_acc_tail(double (&wsum)[kListUsers][W], u64 (&wcnt)[kListUsers][kListMaxCut], int n_k,
                                              u64* counts, double* partial) {
  constexpr int NS = W / kListMaxCut;
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  rank_wave_sync();
  if (lane < n_k && wcnt[w][lane] != 0) atomicAdd(counts + lane, wcnt[w][lane]);
  __syncthreads();
  if (tid < n_k * NS) {
    double s = wsum[0][tid];
    for (int ww = 1; ww < kListUsers; ++ww) s += wsum[ww][tid];
    partial[(int64_t)blockIdx.x * n_k * NS + tid] = s;
  }
}

__global__ __launch_bounds__(RH_BLOCK) void rank_metrics_kernel(const RankArgs a) {
  __shared__ int64_t stage[kListUsers][kRankStage];
  // the wavefront's running sums live in LDS (lane 0 adds user after user: a fixed order), not in 80 registers per lane
  __shared__ double wsum[kListUsers][kListMaxCut * kRankSums];
  __shared__ u64 whit[kListUsers][kListMaxCut];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  wave_acc_zero(wsum, whit, w, lane);
  rank_wave_sync();
  u64 gts = 0;
  for (int64_t u = (int64_t)blockIdx.x * kListUsers + w; u < a.M; u += (int64_t)gridDim.x * kListUsers) {
    int64_t lo = a.off[u], hi = a.off[u + 1];
    lo = lo < 0 ? 0 : (lo > a.n_truth ? a.n_truth : lo);
    hi = hi < lo ? lo : (hi > a.n_truth ? a.n_truth : hi);
    const int64_t len = hi - lo;
    int64_t id[kListPer];
    bool hit[kListPer];
#pragma unroll
    for (int r = 0; r < kListPer; ++r) {
      const int j = r * RH_WAVE + lane;
      id[r] = j < a.K ? a.pred[u * a.ld + j] : 0;
      hit[r] = false;
    }
    for (int64_t s0 = 0; s0 < len; s0 += kRankStage) {
      const int cnt = len - s0 < kRankStage ? (int)(len - s0) : kRankStage;
      rank_wave_sync();  // the previous stage has been read
      for (int e = lane; e < cnt; e += RH_WAVE) stage[w][e] = a.ids[lo + s0 + e];
      rank_wave_sync();
      for (int e = 0; e < cnt; ++e) {
        const int64_t t = stage[w][e];
#pragma unroll
        for (int r = 0; r < kListPer; ++r) hit[r] |= id[r] == t;
      }
    }
    if (len > 0) gts += (u64)len;
#pragma unroll
    for (int q = 0; q < kListMaxCut; ++q) {
      if (q >= a.c.n_k) break;
      const int k = a.c.cut[q];
      uint64_t m[kListPer];
      int nhit = 0;
#pragma unroll
      for (int r = 0; r < kListPer; ++r) {
        m[r] = __ballot(hit[r] && r * RH_WAVE + lane < k && r * RH_WAVE + lane < a.K);
        nhit += __popcll(m[r]);
      }
      double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      if (len > 0) {
        double dcg = 0.0;
        int first = -1;
#pragma unroll
        for (int r = 0; r < kListPer; ++r) {
          uint64_t x = m[r];
          while (x != 0) {  // ascending positions: the order in which the reference adds
            const int j = r * RH_WAVE + __ffsll((unsigned long long)x) - 1;
            x &= x - 1;
            if (first < 0) first = j;
            dcg += a.gain[j];
          }
        }
        const int64_t il = len < k ? len : k;
        v[0] = (double)nhit;
        v[1] = first >= 0 ? 1.0 / (double)(1 + first) : 0.0;
        v[2] = (double)nhit / (double)len;
        v[3] = (double)nhit / (double)k;
        v[4] = dcg / a.ideal[il];
        if (lane == 0) wave_acc_add(wsum, whit, w, q, v + 1, (u64)nhit);
      }
      if (a.per_user != nullptr && lane < 5) {
        double o = v[0];
        for (int t = 1; t < 5; ++t) o = lane == t ? v[t] : o;
        a.per_user[(u * a.c.n_k + q) * 5 + lane] = o;
      }
    }
  }
  if (lane == 0 && gts != 0) atomicAdd(a.gts, gts);
  wave_acc_tail(wsum, whit, a.c.n_k, a.hits, a.partial);
}

// ONE workgroup of kSumParts x WIDTH threads over partials of n <= WIDTH sums each: thread (part, e) adds the partials
// b = part, part + kSumParts, ... of sum e in ascending b, then thread e adds the parts in ascending order: a fixed order
template <int WIDTH>
__global__ __launch_bounds__(kSumParts * WIDTH) void final_sum_kernel(const double* partial, int nblocks, int n,
                                                                      double* sums) {
  __shared__ double part_sum[kSumParts][WIDTH];
  const int e = threadIdx.x % WIDTH, part = threadIdx.x / WIDTH;
  double s = 0.0;
  if (e < n)
    for (int b = part; b < nblocks; b += kSumParts) s += partial[(int64_t)b * n + e];
  part_sum[part][e] = s;
  __syncthreads();
  if (part == 0 && e < n) {
    s = part_sum[0][e];
    for (int q = 1; q < kSumParts; ++q) s += part_sum[q][e];
    sums[e] = s;
  }
}

template <int WIDTH>
void final_sum_launch(const double* partial, int nblocks, int n, double* sums, hipStream_t st) {
  hipLaunchKernelGGL((final_sum_kernel<WIDTH>), dim3(1), dim3(kSumParts * WIDTH), 0, st, partial, nblocks, n, sums);
}

// what the plans of the list kernels answer: `width` doubles per workgroup of a grid of at most `cap`
int list_plan(const char* who, int M, int cap, int width, int* users_per_workgroup, int* max_grid, int64_t* partial_doubles) {
  RH_REQUIRE(users_per_workgroup && max_grid && partial_doubles, RH_E_BADARG, "%s: null pointer", who);
  RH_REQUIRE(M >= 0, RH_E_BADARG, "%s: M=%d", who, M);
  *users_per_workgroup = kListUsers;
  *max_grid = cap;
  *partial_doubles = (int64_t)grid_for(M, kListUsers, cap) * width;
  return 0;
}

// the checks the list entries share; the cut-offs in the caller's order
int list_check(const char* who, int64_t ld, int M, int K, const int* cutoffs, int n_k, ListCuts* c) {
  RH_REQUIRE(K >= 1 && K <= kListMaxK, RH_E_UNSUPPORTED, "%s: K=%d unsupported (1 <= K <= %d)", who, K, kListMaxK);
  RH_REQUIRE(n_k >= 1 && n_k <= kListMaxCut, RH_E_UNSUPPORTED, "%s: %d cut-offs (1 <= n_k <= %d)", who, n_k, kListMaxCut);
  RH_REQUIRE(M >= 1 && ld >= K, RH_E_BADARG, "%s: M=%d ld=%lld K=%d", who, M, (long long)ld, K);
  RH_REQUIRE(cutoffs != nullptr, RH_E_BADARG, "%s: null pointer", who);
  c->n_k = n_k;
  for (int q = 0; q < kListMaxCut; ++q) {
    c->cut[q] = 0;
    c->slot[q] = 0;
  }
  for (int q = 0; q < n_k; ++q) {
    RH_REQUIRE(cutoffs[q] >= 1 && cutoffs[q] <= K, RH_E_BADARG, "%s: cut-off %d outside [1, K=%d]", who, cutoffs[q], K);
    c->cut[q] = cutoffs[q];
    c->slot[q] = q;
  }
  return 0;
}

}  // namespace

extern "C" int rh_auc_plan(int64_t n, int* chunk, int* max_grid, int64_t* workspace_bytes) {
  RH_REQUIRE(chunk && max_grid && workspace_bytes, RH_E_BADARG, "rh_auc_plan: null pointer");
  RH_REQUIRE(n >= 0 && n < (1ll << 31), RH_E_UNSUPPORTED, "rh_auc_plan: n=%lld outside [0, 2^31)", (long long)n);
  const int64_t nchunks = (n + kAucChunk - 1) / kAucChunk;
  *chunk = kAucChunk;
  *max_grid = kAucMaxGrid;
  *workspace_bytes = nchunks * (kAucCarry * 8 + kAucAgg * 4) + 8;
  return 0;
}

extern "C" int rh_auc_keys(const float* pred, int64_t pred_stride, const int64_t* g, int64_t n, int64_t* keys,
                           void* stream) {
  RH_REQUIRE(n >= 0 && n < (1ll << 31), RH_E_UNSUPPORTED, "rh_auc_keys: n=%lld outside [0, 2^31)", (long long)n);
  if (n == 0) return 0;
  RH_REQUIRE(pred && keys, RH_E_BADARG, "rh_auc_keys: null pointer");
  const int64_t b = (n + RH_BLOCK - 1) / RH_BLOCK;
  hipLaunchKernelGGL(auc_keys_kernel, dim3((unsigned)(b > 4096 ? 4096 : b)), dim3(RH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const uint32_t*>(pred), pred_stride, g, n, keys);
  RH_LAUNCH_CHECK("rh_auc_keys");
  return 0;
}

extern "C" int rh_auc_groups(const float* pred, int64_t pred_stride, const void* label, int label_dtype, const int64_t* g,
                             const int64_t* order, int64_t n, int64_t G, void* workspace, int64_t* out, int64_t* bad,
                             void* stream) {
  RH_REQUIRE(n >= 1 && n < (1ll << 31), RH_E_UNSUPPORTED, "rh_auc_groups: n=%lld outside [1, 2^31)", (long long)n);
  RH_REQUIRE(G >= 1 && G < (1ll << 31) && (g != nullptr || G == 1), RH_E_BADARG,
             "rh_auc_groups: G=%lld (1 <= G < 2^31; 1 without ids)", (long long)G);
  RH_REQUIRE(label_dtype >= 0 && label_dtype <= 3, RH_E_BADARG, "rh_auc_groups: label_dtype=%d outside [0, 3]", label_dtype);
  RH_REQUIRE(pred && label && order && workspace && out && bad, RH_E_BADARG, "rh_auc_groups: null pointer");
  AucArgs a{};
  a.pred = reinterpret_cast<const uint32_t*>(pred);
  a.ps = pred_stride;
  a.label = label;
  a.ldt = label_dtype;
  a.g = g;
  a.order = order;
  a.n = n;
  a.G = G;
  a.nchunks = (n + kAucChunk - 1) / kAucChunk;
  a.carry = static_cast<int64_t*>(workspace);
  a.agg = reinterpret_cast<int32_t*>(a.carry + a.nchunks * kAucCarry);
  a.out = reinterpret_cast<u64*>(out);
  a.bad = reinterpret_cast<u64*>(bad);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(out, 0, (size_t)G * 3 * 8, st);
  if (e == hipSuccess) e = hipMemsetAsync(bad, 0, 16, st);
  RH_REQUIRE(e == hipSuccess, (int)e, "rh_auc_groups: memset failed: %s", hipGetErrorString(e));
  const unsigned grid = (unsigned)(a.nchunks < kAucMaxGrid ? a.nchunks : kAucMaxGrid);
  hipLaunchKernelGGL(auc_agg_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a);
  hipLaunchKernelGGL(auc_scan_kernel, dim3(1), dim3(RH_BLOCK), 0, st, a);
  hipLaunchKernelGGL(auc_emit_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a);
  RH_LAUNCH_CHECK("rh_auc_groups");
  return 0;
}

extern "C" int rh_gauc_reduce(const int64_t* stats, const double* weights, int64_t G, double* partial, double* result,
                              int64_t* single_class, void* stream) {
  RH_REQUIRE(G >= 1 && G < (1ll << 31), RH_E_BADARG, "rh_gauc_reduce: G=%lld outside [1, 2^31)", (long long)G);
  RH_REQUIRE(stats && partial && result && single_class, RH_E_BADARG, "rh_gauc_reduce: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_for(G, RH_BLOCK, kReduceMaxGrid);
  hipLaunchKernelGGL(gauc_partial_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, stats, weights, G, partial);
  hipLaunchKernelGGL((tree_final_kernel<3, GaucDone>), dim3(1), dim3(RH_BLOCK), 0, st, partial, grid,
                     GaucDone{result, single_class});
  RH_LAUNCH_CHECK("rh_gauc_reduce");
  return 0;
}

extern "C" int rh_log_loss(const float* pred, int64_t pred_stride, const void* label, int label_dtype, int64_t n,
                           double* partial, double* result, void* stream) {
  RH_REQUIRE(n >= 1 && n < (1ll << 31), RH_E_UNSUPPORTED, "rh_log_loss: n=%lld outside [1, 2^31)", (long long)n);
  RH_REQUIRE(label_dtype >= 0 && label_dtype <= 3, RH_E_BADARG, "rh_log_loss: label_dtype=%d outside [0, 3]", label_dtype);
  RH_REQUIRE(pred && label && partial && result, RH_E_BADARG, "rh_log_loss: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_for(n, RH_BLOCK, kReduceMaxGrid);
  hipLaunchKernelGGL(log_loss_partial_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, pred, pred_stride, label, label_dtype, n,
                     partial);
  hipLaunchKernelGGL((tree_final_kernel<1, LogLossDone>), dim3(1), dim3(RH_BLOCK), 0, st, partial, grid,
                     LogLossDone{result, n});
  RH_LAUNCH_CHECK("rh_log_loss");
  return 0;
}

extern "C" int rh_rank_metrics_plan(int M, int* stage, int* users_per_workgroup, int* max_grid, int64_t* partial_doubles) {
  RH_REQUIRE(stage != nullptr, RH_E_BADARG, "rh_rank_metrics_plan: null pointer");
  if (int rc = list_plan("rh_rank_metrics_plan", M, kRankMaxGrid, kListMaxCut * kRankSums, users_per_workgroup, max_grid,
                         partial_doubles))
    return rc;
  *stage = kRankStage;
  return 0;
}

extern "C" int rh_rank_metrics(const int64_t* pred, int64_t ld, int M, int K, const int64_t* truth_off,
                               const int64_t* truth_ids, int64_t n_truth, const int* cutoffs, int n_k, const double* gain,
                               const double* ideal, double* partial, int64_t* hits, int64_t* gts, double* sums,
                               double* per_user, void* stream) {
  RankArgs a{};
  if (int rc = list_check("rh_rank_metrics", ld, M, K, cutoffs, n_k, &a.c)) return rc;
  RH_REQUIRE(n_truth >= 0, RH_E_BADARG, "rh_rank_metrics: n_truth=%lld", (long long)n_truth);
  RH_REQUIRE(pred && truth_off && truth_ids && gain && ideal && partial && hits && gts && sums, RH_E_BADARG,
             "rh_rank_metrics: null pointer");
  a.pred = pred;
  a.ld = ld;
  a.M = M;
  a.K = K;
  a.off = truth_off;
  a.ids = truth_ids;
  a.n_truth = n_truth;
  a.gain = gain;
  a.ideal = ideal;
  a.partial = partial;
  a.hits = reinterpret_cast<u64*>(hits);
  a.gts = reinterpret_cast<u64*>(gts);
  a.per_user = per_user;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(hits, 0, (size_t)n_k * 8, st);
  if (e == hipSuccess) e = hipMemsetAsync(gts, 0, 8, st);
  RH_REQUIRE(e == hipSuccess, (int)e, "rh_rank_metrics: memset failed: %s", hipGetErrorString(e));
  const int grid = grid_for(M, kListUsers, kRankMaxGrid);
  hipLaunchKernelGGL(rank_metrics_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a);
  final_sum_launch<kListMaxCut * kRankSums>(partial, grid, n_k * kRankSums, sums, st);
  RH_LAUNCH_CHECK("rh_rank_metrics");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Beyond-accuracy metrics (rh_ild, rh_coverage, rh_novelty; replaces the per-user loops of diversity_score,
// coverage_score and novelty_score).  An id below 0 is an absent position: the user's list is shorter there.
//
// rh_ild: one wavefront per user.  sum_{i<j} u_i . u_j = (||sum u_i||^2 - sum ||u_i||^2) / 2, so a user costs O(k D): the
// wavefront keeps S = sum u_i (D doubles spread over the lanes) and Q = sum ||u_i||^2 while it walks the positions in
// ascending order, and emits 1 - (||S||^2 - Q) / (n (n - 1)) at every cut-off.  LPI lanes share an item (VEC floats each,
// NCH times), so a trip of the wavefront takes 64 / LPI items; every lane group keeps the S, Q and n of its own items and
// the groups are added at the cut-offs by a butterfly (a fixed order).  The cut-offs arrive sorted and cut the walk into
// segments, so that a trip never holds an item beyond the cut-off it is followed by.  The user's ids go to LDS once, as
// table rows or -1 (the next user's ids are already on their way); the rows of the next kIldTrips trips are loaded
// before the current ones are reduced, so two steps of row gathers are in flight per wavefront.
//
// rh_novelty: one wavefront per user, lane l owns the positions l, l + 64, ...; per cut-off a masked butterfly sum.
// Both add a wavefront's users in LDS (lane 0, user after user), the workgroup's wavefronts in index order into one
// partial per workgroup, and the partials in index order: no float atomics, the same bits every time.  That is
// final_sum_kernel and, in novelty_kernel, the wave_acc_* functions of the rank metrics above, with one sum per cut-off
// where those carry four.  ild_kernel writes the same steps out: on the shared functions its D = 64 instantiation measured
// 1 - 1.5 % slower at M = 1 M (profiles/metric_tail_ab.txt), so it keeps its own copy of the tail.
//
// rh_coverage: first[id] = the lowest column at which id appears (integer atomicMin, skipped when a plain read already
// shows a value that low); a second pass counts per cut-off the slots with first < k.  Integers: exact in any order.
namespace {

constexpr int kIldMaxD = RH_ILD_MAX_D, kIldTrips = 2;
constexpr int kCovRows = 256, kCovMaxGrid = 2048;

struct IldArgs {
  const int64_t* pred;
  int64_t ld;
  int M, K;
  const float* table;
  int64_t lt, V;
  int D;
  ListCuts c;       // ascending
  double* partial;  // (gridDim.x, n_k)
  u64* counts;      // (n_k,)
  double* per_user; // (M, n_k) or null
};

template <int VEC, int LPI, int NCH>
__global__ __launch_bounds__(RH_BLOCK) void ild_kernel(const IldArgs a) {
  constexpr int IPT = RH_WAVE / LPI, NE = NCH * VEC, STEP = IPT * kIldTrips;
  __shared__ int64_t row[kListUsers][kListMaxK];
  __shared__ double wsum[kListUsers][kListMaxCut];
  __shared__ u64 wcnt[kListUsers][kListMaxCut];
  __shared__ int scut[kListMaxCut], sslot[kListMaxCut];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int g = lane / LPI, sub = lane % LPI;
#pragma unroll
  for (int q = 0; q < kListMaxCut; ++q) {
    if (tid == q) {
      scut[q] = a.c.cut[q];
      sslot[q] = a.c.slot[q];
    }
    if (lane == q) {
      wsum[w][q] = 0.0;
      wcnt[w][q] = 0;
    }
  }
  __syncthreads();
  const int n_k = a.c.n_k, kmax = scut[n_k - 1];
  const int64_t ustep = (int64_t)gridDim.x * kListUsers;
  int64_t u = (int64_t)blockIdx.x * kListUsers + w;
  int64_t idn[kListPer];
#pragma unroll
  for (int r = 0; r < kListPer; ++r) {
    const int j = r * RH_WAVE + lane;
    idn[r] = (u < a.M && j < kmax) ? a.pred[u * a.ld + j] : -1;
  }
  for (; u < a.M; u += ustep) {
    rank_wave_sync();  // the previous user's rows have been read
#pragma unroll
    for (int r = 0; r < kListPer; ++r) row[w][r * RH_WAVE + lane] = (idn[r] >= 0 && idn[r] < a.V) ? idn[r] : -1;
    rank_wave_sync();
#pragma unroll
    for (int r = 0; r < kListPer; ++r) {  // the next user's ids travel while this one's rows do
      const int j = r * RH_WAVE + lane;
      idn[r] = (u + ustep < a.M && j < kmax) ? a.pred[(u + ustep) * a.ld + j] : -1;
    }
    float cur[kIldTrips][NE], nxt[kIldTrips][NE];
    bool cok[kIldTrips], nok[kIldTrips];
    // the rows of the positions p0 + t IPT + g, t < kIldTrips, of which the first cnt exist
    auto load = [&](float (&e)[kIldTrips][NE], bool (&ok)[kIldTrips], int p0, int cnt) {
#pragma unroll
      for (int t = 0; t < kIldTrips; ++t) {
        const int o = t * IPT + g;
        const int64_t id = o < cnt ? row[w][p0 + o] : -1;
        ok[t] = id >= 0;
        const float* src = a.table + (ok[t] ? id : 0) * a.lt;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int col = (c * LPI + sub) * VEC;
          const bool in = ok[t] && col < a.D;
          if constexpr (VEC == 4) {
            const float4 v = in ? gload<float4>(src + col) : f4_zero();
            e[t][c * 4 + 0] = v.x;
            e[t][c * 4 + 1] = v.y;
            e[t][c * 4 + 2] = v.z;
            e[t][c * 4 + 3] = v.w;
          } else {
            e[t][c] = in ? gload<float>(src + col) : 0.f;
          }
        }
      }
    };
    double S[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) S[i] = 0.0;
    double Q = 0.0;
    int n = 0, p = 0, q = 0;
    load(cur, cok, 0, min(STEP, scut[0]));
    while (p < kmax) {
      const int cnt = min(STEP, scut[q] - p), pn = p + cnt;
      int qn = q;
      while (qn < n_k && scut[qn] <= pn) ++qn;
      if (pn < kmax) load(nxt, nok, pn, min(STEP, scut[qn] - pn));
#pragma unroll
      for (int t = 0; t < kIldTrips; ++t) {
        double ss = 0.0;
#pragma unroll
        for (int i = 0; i < NE; ++i) ss = fma((double)cur[t][i], (double)cur[t][i], ss);
#pragma unroll
        for (int m = 1; m < LPI; m <<= 1) ss += __shfl_xor(ss, m, RH_WAVE);
        // 1 / max(||e||, 1e-10); rsqrt, not sqrt and a division: the kernel is bound by its double arithmetic
        const double inv = cok[t] ? (ss >= 1e-20 ? rsqrt(ss) : 1e10) : 0.0;
#pragma unroll
        for (int i = 0; i < NE; ++i) S[i] = fma((double)cur[t][i], inv, S[i]);
        Q += ss * inv * inv;
        n += cok[t] ? 1 : 0;
      }
      if (qn > q) {  // pn is a cut-off: the lane groups' sums are added, the running ones stay as they are
        double nrm2 = 0.0;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
          double T = S[i];
#pragma unroll
          for (int m = LPI; m < RH_WAVE; m <<= 1) T += __shfl_xor(T, m, RH_WAVE);
          nrm2 = fma(T, T, nrm2);
        }
#pragma unroll
        for (int m = 1; m < LPI; m <<= 1) nrm2 += __shfl_xor(nrm2, m, RH_WAVE);
        double Qt = Q;
        int nt = n;
#pragma unroll
        for (int m = LPI; m < RH_WAVE; m <<= 1) {
          Qt += __shfl_xor(Qt, m, RH_WAVE);
          nt += __shfl_xor(nt, m, RH_WAVE);
        }
        const double value = nt >= 2 ? 1.0 - (nrm2 - Qt) / ((double)nt * (double)(nt - 1)) : (double)NAN;
        if (lane == 0) {
          for (int qq = q; qq < qn; ++qq) {
            const int s = sslot[qq];
            if (nt >= 2) {
              wsum[w][s] += value;
              wcnt[w][s] += 1;
            }
            if (a.per_user != nullptr) a.per_user[u * n_k + s] = value;
          }
        }
      }
      if (pn < kmax) {
#pragma unroll
        for (int t = 0; t < kIldTrips; ++t) {
          cok[t] = nok[t];
#pragma unroll
          for (int i = 0; i < NE; ++i) cur[t][i] = nxt[t][i];
        }
      }
      p = pn;
      q = qn;
    }
  }
  rank_wave_sync();
  if (lane < n_k && wcnt[w][lane] != 0) atomicAdd(a.counts + lane, wcnt[w][lane]);
  __syncthreads();
  if (tid < n_k) {
    double s = wsum[0][tid];
    for (int ww = 1; ww < kListUsers; ++ww) s += wsum[ww][tid];
    a.partial[(int64_t)blockIdx.x * n_k + tid] = s;
  }
}

struct NoveltyArgs {
  const int64_t* pred;
  int64_t ld;
  int M, K;
  const void* pop;
  int pdt;  // 0 float32, 1 float64
  int64_t V;
  ListCuts c;  // in the caller's order
  double* partial;
  u64* counts;
  double* per_user;
};

__global__ __launch_bounds__(RH_BLOCK) void novelty_kernel(const NoveltyArgs a) {
  __shared__ double wsum[kListUsers][kListMaxCut];
  __shared__ u64 wcnt[kListUsers][kListMaxCut];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int n_k = a.c.n_k;
  wave_acc_zero(wsum, wcnt, w, lane);
  rank_wave_sync();
  for (int64_t u = (int64_t)blockIdx.x * kListUsers + w; u < a.M; u += (int64_t)gridDim.x * kListUsers) {
    double term[kListPer];
    bool have[kListPer];
#pragma unroll
    for (int r = 0; r < kListPer; ++r) {
      const int j = r * RH_WAVE + lane;
      const int64_t id = j < a.K ? a.pred[u * a.ld + j] : -1;
      have[r] = id >= 0;
      double p = 1e-10;  // an id beyond the table: the reference's .get(item, 1e-10)
      if (have[r] && id < a.V) p = a.pdt == 0 ? (double)static_cast<const float*>(a.pop)[id] : static_cast<const double*>(a.pop)[id];
      term[r] = have[r] ? -log2(fmax(p, 1e-10)) : 0.0;
    }
#pragma unroll
    for (int q = 0; q < kListMaxCut; ++q) {
      if (q >= n_k) break;
      const int k = a.c.cut[q];
      double s = 0.0;
      int cnt = 0;
#pragma unroll
      for (int r = 0; r < kListPer; ++r) {
        const bool in = have[r] && r * RH_WAVE + lane < k;
        s += in ? term[r] : 0.0;
        cnt += __popcll(__ballot(in));
      }
      s = wave_sum_f64(s);
      const double value = cnt > 0 ? s / (double)cnt : (double)NAN;
      if (lane == 0) {
        if (cnt > 0) wave_acc_add(wsum, wcnt, w, q, &value, 1);
        if (a.per_user != nullptr) a.per_user[u * n_k + q] = value;
      }
    }
  }
  wave_acc_tail(wsum, wcnt, n_k, a.counts, a.partial);
}

// a workgroup takes kCovRows rows per trip and walks their first kmax columns as one flat range: coalesced for any K
__global__ __launch_bounds__(RH_BLOCK) void coverage_mark_kernel(const int64_t* pred, int64_t ld, int M, int kmax,
                                                                 int64_t n_slots, int32_t* first) {
  for (int64_t r0 = (int64_t)blockIdx.x * kCovRows; r0 < M; r0 += (int64_t)gridDim.x * kCovRows) {
    const int rows = M - r0 < kCovRows ? (int)(M - r0) : kCovRows;
    const int total = rows * kmax;
    for (int e = threadIdx.x; e < total; e += RH_BLOCK) {
      const int ul = e / kmax, j = e - ul * kmax;
      const int64_t id = pred[(r0 + ul) * ld + j];
      if (id < 0 || id >= n_slots) continue;
      if (first[id] > j) atomicMin(first + id, j);  // a popular item is settled by the read: no atomic
    }
  }
}

__global__ __launch_bounds__(RH_BLOCK) void coverage_count_kernel(const int32_t* first, int64_t n_slots, const ListCuts c,
                                                                  u64* counts) {
  __shared__ int64_t wc[kListUsers][kListMaxCut];
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  int64_t cnt[kListMaxCut];
#pragma unroll
  for (int q = 0; q < kListMaxCut; ++q) cnt[q] = 0;
  for (int64_t base = (int64_t)blockIdx.x * RH_BLOCK; base < n_slots; base += (int64_t)gridDim.x * RH_BLOCK) {
    const int64_t i = base + tid;
    const int f = i < n_slots ? first[i] : 0x7fffffff;
#pragma unroll
    for (int q = 0; q < kListMaxCut; ++q)
      if (q < c.n_k) cnt[q] += __popcll(__ballot(f < c.cut[q]));
  }
#pragma unroll
  for (int q = 0; q < kListMaxCut; ++q)
    if (lane == 0) wc[w][q] = cnt[q];
  __syncthreads();
  if (tid < c.n_k) {
    int64_t s = 0;
    for (int ww = 0; ww < kListUsers; ++ww) s += wc[ww][tid];
    if (s != 0) atomicAdd(counts + tid, (u64)s);
  }
}

template <int VEC, int LPI, int NCH>
void ild_launch(const IldArgs& a, int grid, hipStream_t st) {
  hipLaunchKernelGGL((ild_kernel<VEC, LPI, NCH>), dim3(grid), dim3(RH_BLOCK), 0, st, a);
}

}  // namespace

extern "C" int rh_ild_plan(int M, int* users_per_workgroup, int* max_grid, int64_t* partial_doubles) {
  return list_plan("rh_ild_plan", M, kListMaxGrid, kListMaxCut, users_per_workgroup, max_grid, partial_doubles);
}

extern "C" int rh_ild(const int64_t* pred, int64_t ld, int M, int K, const float* table, int64_t table_stride, int64_t V,
                      int D, const int* cutoffs, int n_k, double* partial, double* sums, int64_t* counts, double* per_user,
                      void* stream) {
  IldArgs a{};
  if (int rc = list_check("rh_ild", ld, M, K, cutoffs, n_k, &a.c)) return rc;
  RH_REQUIRE(D >= 1 && D <= kIldMaxD, RH_E_UNSUPPORTED, "rh_ild: D=%d unsupported (1 <= D <= %d)", D, kIldMaxD);
  RH_REQUIRE(V >= 1 && table_stride >= D, RH_E_BADARG, "rh_ild: V=%lld table_stride=%lld D=%d", (long long)V,
             (long long)table_stride, D);
  RH_REQUIRE(pred && table && partial && sums && counts, RH_E_BADARG, "rh_ild: null pointer");
  for (int q = 1; q < n_k; ++q)  // ascending, every cut-off with its place in the caller's list
    for (int r = q; r > 0 && a.c.cut[r - 1] > a.c.cut[r]; --r) {
      const int c = a.c.cut[r], s = a.c.slot[r];
      a.c.cut[r] = a.c.cut[r - 1];
      a.c.slot[r] = a.c.slot[r - 1];
      a.c.cut[r - 1] = c;
      a.c.slot[r - 1] = s;
    }
  a.pred = pred;
  a.ld = ld;
  a.M = M;
  a.K = K;
  a.table = table;
  a.lt = table_stride;
  a.V = V;
  a.D = D;
  a.partial = partial;
  a.counts = reinterpret_cast<u64*>(counts);
  a.per_user = per_user;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_k * 8, st);
  RH_REQUIRE(e == hipSuccess, (int)e, "rh_ild: memset failed: %s", hipGetErrorString(e));
  const int grid = grid_for(M, kListUsers, kListMaxGrid);
  if (D % 4 == 0) {  // a float4 per lane: 4 to 64 lanes per item
    if (D <= 16) ild_launch<4, 4, 1>(a, grid, st);
    else if (D <= 32) ild_launch<4, 8, 1>(a, grid, st);
    else if (D <= 64) ild_launch<4, 16, 1>(a, grid, st);
    else if (D <= 128) ild_launch<4, 32, 1>(a, grid, st);
    else if (D <= 256) ild_launch<4, 64, 1>(a, grid, st);
    else if (D <= 512) ild_launch<4, 64, 2>(a, grid, st);
    else ild_launch<4, 64, 4>(a, grid, st);
  } else {  // a float per lane
    if (D <= 16) ild_launch<1, 16, 1>(a, grid, st);
    else if (D <= 32) ild_launch<1, 32, 1>(a, grid, st);
    else if (D <= 64) ild_launch<1, 64, 1>(a, grid, st);
    else if (D <= 128) ild_launch<1, 64, 2>(a, grid, st);
    else if (D <= 256) ild_launch<1, 64, 4>(a, grid, st);
    else if (D <= 512) ild_launch<1, 64, 8>(a, grid, st);
    else ild_launch<1, 64, 16>(a, grid, st);
  }
  final_sum_launch<kListMaxCut>(partial, grid, n_k, sums, st);
  RH_LAUNCH_CHECK("rh_ild");
  return 0;
}

extern "C" int rh_coverage_plan(int64_t n_slots, int* rows_per_workgroup, int* max_grid, int64_t* workspace_bytes) {
  RH_REQUIRE(rows_per_workgroup && max_grid && workspace_bytes, RH_E_BADARG, "rh_coverage_plan: null pointer");
  RH_REQUIRE(n_slots >= 1 && n_slots < (1ll << 31), RH_E_UNSUPPORTED, "rh_coverage_plan: n_slots=%lld outside [1, 2^31)",
             (long long)n_slots);
  *rows_per_workgroup = kCovRows;
  *max_grid = kCovMaxGrid;
  *workspace_bytes = n_slots * 4;
  return 0;
}

extern "C" int rh_coverage(const int64_t* pred, int64_t ld, int M, int K, int64_t n_slots, const int* cutoffs, int n_k,
                           int32_t* first, int64_t* counts, void* stream) {
  ListCuts c{};
  if (int rc = list_check("rh_coverage", ld, M, K, cutoffs, n_k, &c)) return rc;
  RH_REQUIRE(n_slots >= 1 && n_slots < (1ll << 31), RH_E_UNSUPPORTED, "rh_coverage: n_slots=%lld outside [1, 2^31)",
             (long long)n_slots);
  RH_REQUIRE(pred && first && counts, RH_E_BADARG, "rh_coverage: null pointer");
  int kmax = 0;
  for (int q = 0; q < n_k; ++q) kmax = c.cut[q] > kmax ? c.cut[q] : kmax;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(first), K, (size_t)n_slots, st);
  if (e == hipSuccess) e = hipMemsetAsync(counts, 0, (size_t)n_k * 8, st);
  RH_REQUIRE(e == hipSuccess, (int)e, "rh_coverage: memset failed: %s", hipGetErrorString(e));
  const int64_t mark = ((int64_t)M + kCovRows - 1) / kCovRows, count = (n_slots + RH_BLOCK - 1) / RH_BLOCK;
  hipLaunchKernelGGL(coverage_mark_kernel, dim3((unsigned)(mark > kCovMaxGrid ? kCovMaxGrid : mark)), dim3(RH_BLOCK), 0, st,
                     pred, ld, M, kmax, n_slots, first);
  hipLaunchKernelGGL(coverage_count_kernel, dim3((unsigned)(count > kCovMaxGrid ? kCovMaxGrid : count)), dim3(RH_BLOCK), 0,
                     st, first, n_slots, c, reinterpret_cast<u64*>(counts));
  RH_LAUNCH_CHECK("rh_coverage");
  return 0;
}

extern "C" int rh_novelty_plan(int M, int* users_per_workgroup, int* max_grid, int64_t* partial_doubles) {
  return list_plan("rh_novelty_plan", M, kListMaxGrid, kListMaxCut, users_per_workgroup, max_grid, partial_doubles);
}

extern "C" int rh_novelty(const int64_t* pred, int64_t ld, int M, int K, const void* pop, int pop_dtype, int64_t V,
                          const int* cutoffs, int n_k, double* partial, double* sums, int64_t* counts, double* per_user,
                          void* stream) {
  NoveltyArgs a{};
  if (int rc = list_check("rh_novelty", ld, M, K, cutoffs, n_k, &a.c)) return rc;
  RH_REQUIRE(pop_dtype == 0 || pop_dtype == 1, RH_E_BADARG, "rh_novelty: pop_dtype=%d outside [0, 1]", pop_dtype);
  RH_REQUIRE(V >= 1, RH_E_BADARG, "rh_novelty: V=%lld", (long long)V);
  RH_REQUIRE(pred && pop && partial && sums && counts, RH_E_BADARG, "rh_novelty: null pointer");
  a.pred = pred;
  a.ld = ld;
  a.M = M;
  a.K = K;
  a.pop = pop;
  a.pdt = pop_dtype;
  a.V = V;
  a.partial = partial;
  a.counts = reinterpret_cast<u64*>(counts);
  a.per_user = per_user;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_k * 8, st);
  RH_REQUIRE(e == hipSuccess, (int)e, "rh_novelty: memset failed: %s", hipGetErrorString(e));
  const int grid = grid_for(M, kListUsers, kListMaxGrid);
  hipLaunchKernelGGL(novelty_kernel, dim3(grid), dim3(RH_BLOCK), 0, st, a);
  final_sum_launch<kListMaxCut>(partial, grid, n_k, sums, st);
  RH_LAUNCH_CHECK("rh_novelty");
  return 0;
}
