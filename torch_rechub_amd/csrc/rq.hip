// Residual quantizer of the RQ-VAE (reference torch_rechub/models/generative/rqvae.py:241-274 per level, :382-398 across
// levels), fp32, gfx950.  Rows x (N, E), L codebooks C_l (n_e[l], E); 1 <= E <= 128, 1 <= n_e[l] <= 1024, 1 <= L <= 8.
//
// Forward, ONE launch for all levels of a range [l0, l1): a workgroup of four wavefronts owns 16 consecutive rows (and strides
// over the row groups when there are more than kMaxFwdBlocks of them); their residuals live in LDS, transposed (e, row), for the
// whole launch.  Per level the codebook passes through LDS in tiles of up to 256 codes (row stride E | 1: a lane per code reads
// without bank conflicts); a wavefront takes four rows, a lane one code at a time: per column one code value and one
// broadcast float4 of the four residuals feed four direct-form accumulators sum (r - c)^2 (no ||r||^2 + ||c||^2 - 2 r.c: it
// cancels).  A lane keeps its best (distance, index) per row over its codes in ascending index order, one butterfly per row
// and level ends the arg-min; ties go to the lower index (torch.argmin).  Then r <- r - C_l[idx] in LDS, and the level's
// sum of (C_l[idx] - r)^2 (which is the new residual squared) goes into a per-workgroup partial; rh_colsum adds the partials
// in a fixed order.  No (N, K) array exists.  A level whose bit is set in `given` takes its index from idx instead.
//
// Backward, from x, the codebooks, idx, g_xq and the device scalar g_loss (s = g_loss 2 / (L N E)):
//   g_x   = g_xq + s beta (x - C_0[idx_0])                  (elementwise kernel; the commitment terms of the levels >= 1
//                                                            cancel through the straight-through estimator)
//   g_C_l[k] = s sum over rows with idx_l = k of (C_l[k] - r_l)
// The second as a gather: a thread owns one element (k, e) of one level's table for one chunk of consecutive rows, walks
// the chunk's indices in row order and, on a match, rebuilds r_l[e] from x and the earlier levels' codes.  Every element of
// the (chunks, sum_l n_e[l] E) partial is written, rows nobody chose get exactly 0, and rh_colsum adds the chunks.
// No atomics anywhere: two runs give the same bits.
#include "common.h"

namespace {

constexpr int kMaxE = RH_RQ_MAX_E, kMaxCodes = RH_RQ_MAX_CODES, kMaxL = RH_RQ_MAX_L;
constexpr int kRowsPerWave = 4, kWaves = RH_BLOCK / RH_WAVE, kRows = kRowsPerWave * kWaves;  // 16 rows per workgroup
constexpr int kColsPerStep = 4;
constexpr int kTileFloats = 12288, kMaxTileCodes = 256;                                    // 48 KB of codes in LDS
constexpr int kMaxFwdBlocks = 2048, kMaxChunks = 64, kChunkRows = 16;

struct RqArgs {
  const float* C[kMaxL];
  int ne[kMaxL];
  int N, E, L;
};

bool rq_shape_ok(int E, int L, const int* ne) {
  if (E < 1 || E > kMaxE || L < 1 || L > kMaxL) return false;
  for (int l = 0; l < L; ++l) {
    if (ne[l] < 1 || ne[l] > kMaxCodes) return false;
  }
  return true;
}

__host__ __device__ inline int rq_stride(int E) { return E | 1; }
__host__ __device__ inline int rq_tile_codes(int E) {
  const int t = (kTileFloats / rq_stride(E)) / RH_WAVE * RH_WAVE;
  return t > kMaxTileCodes ? kMaxTileCodes : t;  // 64 at E = 128, 256 up to E = 47
}
size_t rq_fwd_lds(int E) { return sizeof(float) * ((size_t)E * kRows + (size_t)rq_tile_codes(E) * rq_stride(E) + kMaxL * kWaves); }

int rq_fwd_blocks(int N) {
  const int64_t groups = ((int64_t)N + kRows - 1) / kRows;
  return groups < 1 ? 1 : (groups > kMaxFwdBlocks ? kMaxFwdBlocks : (int)groups);
}
int rq_bwd_chunks(int N) {
  const int64_t c = ((int64_t)N + kChunkRows - 1) / kChunkRows;
  return c < 1 ? 1 : (c > kMaxChunks ? kMaxChunks : (int)c);
}

__global__ __launch_bounds__(RH_BLOCK) void rq_fwd_kernel(const float* __restrict__ r_in, RqArgs a, int l0, int l1, int given,
                                                          int32_t* __restrict__ idx, float* __restrict__ r_out,
                                                          float* __restrict__ x_q, float* __restrict__ sse_partial) {
  extern __shared__ float lds[];
  const int E = a.E, L = a.L, N = a.N, ES = rq_stride(E), TK = rq_tile_codes(E);
  float* rT = lds;                     // (E, 16): the residuals, transposed
  float* tile = rT + E * kRows;        // (TK, ES)
  float* red = tile + TK * ES;         // (kMaxL, kWaves)
  const int tid = threadIdx.x, lane = tid % RH_WAVE, w = tid / RH_WAVE;
  const int groups = (N + kRows - 1) / kRows;
  float sse[kMaxL];
#pragma unroll
  for (int l = 0; l < kMaxL; ++l) sse[l] = 0.f;

  for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {  // uniform per workgroup
    const int64_t row0 = (int64_t)grp * kRows;
    __syncthreads();  // (the previous group's write-out is done with rT)
    for (int i = tid; i < kRows * E; i += RH_BLOCK) {
      const int rl = i / E, e = i - rl * E;
      rT[e * kRows + rl] = row0 + rl < N ? r_in[(row0 + rl) * E + e] : 0.f;
    }
#pragma unroll
    for (int l = 0; l < kMaxL; ++l) {
      if (l < l0 || l >= l1) continue;  // uniform
      const float* __restrict__ Cl = a.C[l];
      const int K = a.ne[l];
      int pick[kRowsPerWave];
      if (!((given >> l) & 1)) {
        float bd[kRowsPerWave];
#pragma unroll
        for (int q = 0; q < kRowsPerWave; ++q) bd[q] = INFINITY, pick[q] = 0;
        for (int t0 = 0; t0 < K; t0 += TK) {
          const int tk = K - t0 < TK ? K - t0 : TK;
          __syncthreads();  // rT is loaded / the previous tile has been read
          for (int i = tid; i < tk * E; i += RH_BLOCK) {
            const int k = i / E, e = i - k * E;
            tile[k * ES + e] = Cl[(int64_t)t0 * E + i];
          }
          __syncthreads();
          for (int kk = lane; kk < tk; kk += RH_WAVE) {
            const float* __restrict__ c = tile + kk * ES;
            float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
            // four columns' LDS reads are issued before their arithmetic (one wait per four columns, not per column);
            // every accumulator still adds its columns in ascending order
            int e = 0;
            for (; e + kColsPerStep <= E; e += kColsPerStep) {
              float cv[kColsPerStep];
              float4 r[kColsPerStep];
#pragma unroll
              for (int u = 0; u < kColsPerStep; ++u) {
                cv[u] = c[e + u];
                r[u] = *reinterpret_cast<const float4*>(rT + (e + u) * kRows + w * kRowsPerWave);
              }
#pragma unroll
              for (int u = 0; u < kColsPerStep; ++u) {
                const float t0_ = r[u].x - cv[u], t1_ = r[u].y - cv[u], t2_ = r[u].z - cv[u], t3_ = r[u].w - cv[u];
                d0 = fmaf(t0_, t0_, d0), d1 = fmaf(t1_, t1_, d1), d2 = fmaf(t2_, t2_, d2), d3 = fmaf(t3_, t3_, d3);
              }
            }
            for (; e < E; ++e) {
              const float cv = c[e];
              const float4 r = *reinterpret_cast<const float4*>(rT + e * kRows + w * kRowsPerWave);
              const float t0_ = r.x - cv, t1_ = r.y - cv, t2_ = r.z - cv, t3_ = r.w - cv;
              d0 = fmaf(t0_, t0_, d0), d1 = fmaf(t1_, t1_, d1), d2 = fmaf(t2_, t2_, d2), d3 = fmaf(t3_, t3_, d3);
            }
            const float d[kRowsPerWave] = {d0, d1, d2, d3};
#pragma unroll
            for (int q = 0; q < kRowsPerWave; ++q) {
              if (d[q] < bd[q]) bd[q] = d[q], pick[q] = t0 + kk;  // ascending index per lane: the lower index stays on a tie
            }
          }
        }
#pragma unroll
        for (int q = 0; q < kRowsPerWave; ++q) {
#pragma unroll
          for (int m = 32; m >= 1; m >>= 1) {
            const float od = __shfl_xor(bd[q], m, RH_WAVE);
            const int ok = __shfl_xor(pick[q], m, RH_WAVE);
            if (od < bd[q] || (od == bd[q] && ok < pick[q])) bd[q] = od, pick[q] = ok;
          }
          if (lane == 0 && row0 + w * kRowsPerWave + q < N) idx[(row0 + w * kRowsPerWave + q) * L + l] = pick[q];
        }
      } else {
#pragma unroll
        for (int q = 0; q < kRowsPerWave; ++q) {
          const int64_t row = row0 + w * kRowsPerWave + q;
          int k = row < N ? idx[row * L + l] : 0;
          pick[q] = k < 0 ? 0 : (k >= K ? K - 1 : k);
        }
        __syncthreads();  // rT is loaded (the searched path passes a barrier of its own)
      }
      // r <- r - C_l[idx]; the rows are this wavefront's own, nobody else touches their columns of rT
      float acc = 0.f;
#pragma unroll
      for (int q = 0; q < kRowsPerWave; ++q) {
        const bool live = row0 + w * kRowsPerWave + q < N;
        for (int e = lane; e < E; e += RH_WAVE) {
          float* p = rT + e * kRows + w * kRowsPerWave + q;
          const float rn = *p - Cl[(int64_t)pick[q] * E + e];
          *p = rn;
          if (live) acc = fmaf(rn, rn, acc);
        }
      }
      sse[l] += wave_sum(acc);
    }
    __syncthreads();
    for (int i = tid; i < kRows * E; i += RH_BLOCK) {
      const int rl = i / E, e = i - rl * E;
      if (row0 + rl < N) {
        const float r = rT[e * kRows + rl];
        r_out[(row0 + rl) * E + e] = r;
        x_q[(row0 + rl) * E + e] = r_in[(row0 + rl) * E + e] - r;
      }
    }
  }
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int l = 0; l < kMaxL; ++l) red[l * kWaves + w] = sse[l];
  }
  __syncthreads();
  if (tid < l1 - l0) {
    const float* p = red + (l0 + tid) * kWaves;
    sse_partial[(int64_t)blockIdx.x * (l1 - l0) + tid] = ((p[0] + p[1]) + p[2]) + p[3];
  }
}

__global__ __launch_bounds__(RH_BLOCK) void rq_gx_kernel(const float* __restrict__ x, const float* __restrict__ C0, int K0,
                                                         const int32_t* __restrict__ idx, const float* __restrict__ g_xq,
                                                         const float* __restrict__ g_loss, float coef, int64_t total, int E,
                                                         int L, float* __restrict__ g_x) {
  const float s = g_loss[0] * coef;
  for (int64_t i = (int64_t)blockIdx.x * RH_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * RH_BLOCK) {
    const int64_t row = i / E;
    const int e = (int)(i - row * E);
    int k = idx[row * L];
    k = k < 0 ? 0 : (k >= K0 ? K0 - 1 : k);
    g_x[i] = fmaf(s, x[i] - C0[(int64_t)k * E + e], g_xq[i]);
  }
}

// grid (ceil(max_l n_e[l] E / 256), chunks, L)
__global__ __launch_bounds__(RH_BLOCK) void rq_cgrad_kernel(const float* __restrict__ x, RqArgs a,
                                                            const int32_t* __restrict__ idx, const float* __restrict__ g_loss,
                                                            float coef, int chunk, int64_t total,
                                                            float* __restrict__ c_partial) {
  const int l = blockIdx.z, E = a.E, L = a.L, K = a.ne[l];
  const int j = blockIdx.x * RH_BLOCK + threadIdx.x;
  if (j >= K * E) return;
  int64_t off = 0;
  for (int q = 0; q < l; ++q) off += (int64_t)a.ne[q] * E;
  const int k = j / E, e = j - k * E;
  const float ck = a.C[l][j];
  const int64_t r0 = (int64_t)blockIdx.y * chunk;
  const int64_t r1 = r0 + chunk < a.N ? r0 + chunk : a.N;
  float acc = 0.f;
  bool hit = false;
  for (int64_t row = r0; row < r1; ++row) {
    int kl = idx[row * L + l];
    kl = kl < 0 ? 0 : (kl >= K ? K - 1 : kl);  // clamped as the forward and g_x clamp a given index
    if (kl != k) continue;
    float r = x[row * E + e];
    for (int q = 0; q < l; ++q) {
      int kq = idx[row * L + q];
      kq = kq < 0 ? 0 : (kq >= a.ne[q] ? a.ne[q] - 1 : kq);
      r -= a.C[q][(int64_t)kq * E + e];
    }
    acc += ck - r;
    hit = true;
  }
  c_partial[(int64_t)blockIdx.y * total + off + j] = hit ? acc * (g_loss[0] * coef) : 0.f;
}

int rq_check(const char* who, int N, int E, int L, const int* ne) {
  RH_REQUIRE(ne != nullptr, RH_E_BADARG, "%s: null pointer", who);
  RH_REQUIRE(N >= 0, RH_E_BADARG, "%s: N=%d", who, N);
  RH_REQUIRE(rq_shape_ok(E, L, ne), RH_E_UNSUPPORTED,
             "%s: E=%d with %d codebooks has no HIP kernel (1 <= E <= %d, 1 <= n_e <= %d, 1 <= L <= %d)", who, E, L, kMaxE,
             kMaxCodes, kMaxL);
  return 0;
}

}  // namespace

extern "C" int rh_rq_supported(int E, int L, const int* n_e, int* supported) {
  RH_REQUIRE(supported != nullptr && (n_e != nullptr || L < 1 || L > kMaxL), RH_E_BADARG, "rh_rq_supported: null pointer");
  *supported = rq_shape_ok(E, L, n_e) ? 1 : 0;
  return 0;
}

extern "C" int rh_rq_nchunks(int N, int* fwd_blocks, int* bwd_chunks) {
  RH_REQUIRE(fwd_blocks != nullptr && bwd_chunks != nullptr, RH_E_BADARG, "rh_rq_nchunks: null pointer");
  *fwd_blocks = rq_fwd_blocks(N);
  *bwd_chunks = rq_bwd_chunks(N);
  return 0;
}

extern "C" int rh_rq_fwd(const float* r_in, const float* const* C, const int* n_e, int N, int E, int L, int l0, int l1,
                         int given, int32_t* idx, float* r_out, float* x_q, float* sse_partial, float* sse, void* stream) {
  RH_REQUIRE(C != nullptr, RH_E_BADARG, "rh_rq_fwd: null pointer");
  if (int rc = rq_check("rh_rq_fwd", N, E, L, n_e)) return rc;
  RH_REQUIRE(0 <= l0 && l0 < l1 && l1 <= L, RH_E_BADARG, "rh_rq_fwd: level range [%d, %d) of %d", l0, l1, L);
  RH_REQUIRE(r_in && idx && r_out && x_q && sse_partial && sse, RH_E_BADARG, "rh_rq_fwd: null pointer");
  if (N == 0) return 0;
  RqArgs a{};
  for (int l = 0; l < L; ++l) {
    RH_REQUIRE(C[l] != nullptr, RH_E_BADARG, "rh_rq_fwd: null codebook %d", l);
    a.C[l] = C[l], a.ne[l] = n_e[l];
  }
  a.N = N, a.E = E, a.L = L;
  const int blocks = rq_fwd_blocks(N);
  hipLaunchKernelGGL(rq_fwd_kernel, dim3((unsigned)blocks), dim3(RH_BLOCK), rq_fwd_lds(E),
                     reinterpret_cast<hipStream_t>(stream), r_in, a, l0, l1, given, idx, r_out, x_q, sse_partial);
  RH_LAUNCH_CHECK("rh_rq_fwd");
  return rh_colsum(sse_partial, blocks, l1 - l0, sse + l0, nullptr, 0, nullptr, stream);
}

extern "C" int rh_rq_bwd(const float* x, const float* const* C, const int* n_e, const int32_t* idx, const float* g_xq,
                         const float* g_loss, float beta, int N, int E, int L, float* g_x, float* c_partial, float* g_C,
                         void* stream) {
  RH_REQUIRE(C != nullptr, RH_E_BADARG, "rh_rq_bwd: null pointer");
  if (int rc = rq_check("rh_rq_bwd", N, E, L, n_e)) return rc;
  RH_REQUIRE(x && idx && g_xq && g_loss && g_x && c_partial && g_C, RH_E_BADARG, "rh_rq_bwd: null pointer");
  if (N == 0) return 0;
  RqArgs a{};
  int64_t total = 0;
  int widest = 0;
  for (int l = 0; l < L; ++l) {
    RH_REQUIRE(C[l] != nullptr, RH_E_BADARG, "rh_rq_bwd: null codebook %d", l);
    a.C[l] = C[l], a.ne[l] = n_e[l];
    total += (int64_t)n_e[l] * E;
    if (n_e[l] * E > widest) widest = n_e[l] * E;
  }
  a.N = N, a.E = E, a.L = L;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float coef = (float)(2.0 / ((double)L * (double)N * (double)E));
  const int64_t ne = (int64_t)N * E;
  int64_t grid = (ne + RH_BLOCK - 1) / RH_BLOCK;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(rq_gx_kernel, dim3((unsigned)grid), dim3(RH_BLOCK), 0, st, x, a.C[0], a.ne[0], idx, g_xq, g_loss,
                     coef * beta, ne, E, L, g_x);
  RH_LAUNCH_CHECK("rh_rq_bwd (g_x)");
  const int nch = rq_bwd_chunks(N);
  const int chunk = (N + nch - 1) / nch;
  hipLaunchKernelGGL(rq_cgrad_kernel, dim3((unsigned)((widest + RH_BLOCK - 1) / RH_BLOCK), (unsigned)nch, (unsigned)L),
                     dim3(RH_BLOCK), 0, st, x, a, idx, g_loss, coef, chunk, total, c_partial);
  RH_LAUNCH_CHECK("rh_rq_bwd (codebook gradient)");
  return rh_colsum(c_partial, nch, (int)total, g_C, nullptr, 0, nullptr, stream);
}
