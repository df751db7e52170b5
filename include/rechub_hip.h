/*
 * rechub_hip.h — C ABI of librechub_hip.so, the MI355X (gfx950) CTR-training hot path.
 *
 * Every entry point replaces an ATen op chain of the reference (datawhalechina/torch-rechub
 * v0.8.0, 100 % Python on eager PyTorch — there is no FFI in the reference, so the
 * "interface replaced" is the Python call site cited per function, paths relative to
 * /root/reference).  Signatures carry plain pointers and sizes only: no torch types.
 *
 * Conventions
 *   - all data pointers are DEVICE pointers unless the name starts with h_;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - return value 0 = success, >0 = hipError_t of a failed launch, <0 = RH_E_* argument error
 *     (rh_last_error() returns a human-readable message for the calling thread);
 *   - kernels are asynchronous; nothing here synchronises, allocates or frees device memory,
 *     so every call may be captured into a hipGraph;
 *   - `err_flag` (device int32, may be NULL) is OR-ed with RH_FLAG_* bits by kernels that
 *     validate indices; the host reads it at its own sync points.
 *   - a shape limit (a bound answered with RH_E_UNSUPPORTED, or the size of a fixed LDS / register array) is an integer macro
 *     RH_<FAMILY>_MAX_<DIM> (or _MIN_) beside the family's declarations: the kernels take it from here, Python reads it
 *     as _lib.H.RH_..., tests/test_abi.py holds the values in one table.
 *
 * Field descriptor tables (device int64 arrays, struct-of-arrays, F = number of fields):
 *   fdesc[0*F + f] = const float* table base of field f        (vocab_f x D, row-major, fp32)
 *   fdesc[1*F + f] = float*       dense gradient buffer of that table (same shape) or 0
 *   fdesc[2*F + f] = int64        vocab_f (rows)
 *   fdesc[3*F + f] = int64        padding_idx of field f, or -1 (rows whose gradient is dropped,
 *                                 nn.Embedding(padding_idx=...) semantics, basic/initializers.py:16-21)
 *   idesc[0*F + f] = const idx_t* index column of field f (one index per sample)
 *   idesc[1*F + f] = int64        stride between consecutive samples, in elements
 *   idesc[2*F + f] = int64        output slot of field f: its D values live at columns
 *                                 [slot*D, slot*D + D) of out / g_out / emb (slot = f unless sequence
 *                                 features are interleaved with sparse ones, basic/layers.py:80-99)
 * Two fields may name the same table (SparseFeature.shared_with, basic/layers.py:85,99).
 *
 * Keep this file plain C: torch_rechub_amd/_header.py parses it for the ctypes signatures and refuses what it cannot map
 * (scalars other than int / int64_t / float by value, structs by value, function pointers, non-integer RH_* macros).
 */
#ifndef RECHUB_HIP_H
#define RECHUB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RH_ABI_VERSION 1

/* argument errors */
#define RH_E_BADARG (-1)
#define RH_E_UNSUPPORTED (-2)

/* err_flag bits */
#define RH_FLAG_INDEX_OOB 1 /* an index was <0 or >= vocab (reference: IndexError / device assert) */
#define RH_FLAG_TARGET_OOB 2 /* a class label was < 0 or >= the class count (reference: IndexError) */
#define RH_FLAG_SESSION_EMPTY 128 /* a session row holds no item (reference: pack_padded_sequence raises) */
#define RH_FLAG_SESSION_SHORT 256 /* no session row reaches the padded length L (reference NARM: broadcast error) */

int rh_abi_version(void);
const char* rh_last_error(void);

/* tuning knobs (process-wide; defaults are the measured winners).  Keys 1, 3, 4, 5, 6, 10, 11, 14, 15 and 16 selected experiments
 * that were measured and rejected (DESIGN.md keeps the numbers); they are removed with the variants behind them, and
 * rh_set_tuning fails for them as for any unknown key. */
#define RH_TUNE_SWEEP_GRID 2   /* workgroups of rh_adam_lazy_sweep (0 = default 8192) */
#define RH_TUNE_DEFERRED_GRID 8 /* persistent workgroups of a DEFERRED sweep (default 512 = 2 per CU; 0 = as RH_TUNE_SWEEP_GRID):
                                  the residency cap that lets the step's chain keep its wave slots and issue cycles */
#define RH_TUNE_SWEEP_STAGGER_NS 12 /* rh_adam_sweep_stagger: hold-back in nanoseconds (default 15000; 0 = no launch) */
#define RH_TUNE_SWEEP_GATE_NS 13 /* rh_adam_sweep_gate(fallback_ns = 0): hold-back behind the opening, ns (default 32000) */
#define RH_TUNE_WGRAD_BLOCKS 9 /* workgroups rh_linear_wgrad aims for when the reduction is >= 32768 rows (default 1024) */
#define RH_TUNE_FWD_PATH 7      /* rh_embed_fwd: 0 auto (by batch size), 1 lane-split kernel only, 2 field-uniform kernel only;
                                   any other value fails */
int rh_set_tuning(int key, int value);

/* ---------------------------------------------------------------------------------------------
 * K1+K2+K3  fused multi-field gather + FM second order + LR first order (+ dense concat)
 * replaces: EmbeddingLayer.forward  torch_rechub/basic/layers.py:77-127  (26x nn.Embedding + cat)
 *           FM.forward              torch_rechub/basic/layers.py:313-319
 *           LR.forward              torch_rechub/basic/layers.py:185-189 on the flattened embeddings
 *           as composed by DeepFM.forward torch_rechub/models/ranking/deepfm.py:34-43
 * out   : (B, out_stride) fp32, rows only 4-byte aligned (e.g. a contiguous (B, 429) tensor); field f
 *         at columns [slot_f*D, slot_f*D + D), dense values at [dense_col, dense_col + n_dense)
 *         (sparse block first, dense last: layers.py:120), other columns untouched.
 * ddesc : device int64 [2*n_dense]: const float* column, sample stride (elements); NULL if n_dense = 0
 * lr_w  : (F*D,) indexed by FIELD (needs slot_f == f) or NULL; lr_b: (1,) or NULL;
 *         lr_out (B,) = emb . lr_w + lr_b
 * fm_out: (B,) or NULL = 0.5 * sum_d[(sum_f v)^2 - sum_f v^2]
 * s_out : (B, D) or NULL = sum_f v  (saved for the backward)
 * D must be a multiple of 4 and <= RH_EMBED_MAX_D (16-byte lanes); idx_is_i64: 1 = int64 indices, 0 = int32.
 * lr_out needs F * D <= RH_EMBED_MAX_LR_FD (the LR weights are kept in LDS).
 * field_split: 0 = auto, else 1/2/4/8 lanes-groups per sample (tuning knob).
 */
#define RH_EMBED_MAX_D 128
#define RH_EMBED_MAX_LR_FD 12288
int rh_embed_fwd(const int64_t* fdesc, const int64_t* idesc, int idx_is_i64, int B, int F, int D,
                 const int64_t* ddesc, int n_dense, int dense_col, float* out, int64_t out_stride,
                 const float* lr_w, const float* lr_b, float* lr_out, float* fm_out, float* s_out,
                 int field_split, int32_t* err_flag, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K4  fused backward of the above
 * replaces: autograd of the chain above (embedding_dense_backward x F, FM/LR backward),
 *           driven by loss.backward() at torch_rechub/trainers/ctr_trainer.py:97-98
 * per lookup (b,f):  g = scale * ( g_out[b, f*D:(f+1)*D] + g_lr[b]*lr_w[f*D:(f+1)*D]
 *                                  + g_fm[b] * (s_sum[b,:] - emb[b, f*D:(f+1)*D]) )
 * sink = 0: scatter-add g into the dense gradient buffer fdesc[1*F+f] (skipping padding_idx rows);
 * sink = 1: write g to rows_out (B, F, D) for the data-parallel exchange.
 * Any of g_out / g_fm / g_lr may be NULL (term dropped).  emb/s_sum are required when g_fm != NULL,
 * emb when lr_wgrad != NULL.
 * lr_wgrad : (nchunks, F*D) partial sums of g_lr[b]*emb[b,:] per sample chunk, nchunks =
 *            ceil(B / samples_per_block); the caller reduces over dim 0 (deterministic). NULL to skip.
 * samples_per_block: multiple of 64, 0 = auto (256).
 */
int rh_embed_bwd(const int64_t* fdesc, const int64_t* idesc, int idx_is_i64, int B, int F, int D,
                 const float* g_out, int64_t g_stride, const float* emb, int64_t emb_stride,
                 const float* s_sum, const float* g_fm, const float* g_lr, const float* lr_w,
                 float* lr_wgrad, float scale, int sink, float* rows_out, int samples_per_block,
                 int32_t* err_flag, void* stream);

/* number of sample chunks (= rows of lr_wgrad) rh_embed_bwd uses for this B / samples_per_block */
int rh_embed_bwd_nchunks(int B, int samples_per_block);

/* scatter-add precomputed gradient rows (B, F, D) (e.g. all-gathered from the other ranks)
 * into the dense gradient buffers.  Same padding_idx and small-vocab LDS aggregation as above. */
int rh_embed_scatter_rows(const int64_t* fdesc, const int64_t* idesc, int idx_is_i64, int B, int F,
                          int D, const float* rows, float scale, int samples_per_block,
                          int32_t* err_flag, void* stream);

/* ---------------------------------------------------------------------------------------------
 * FM on an arbitrary (B, F, D) tensor (row stride x_stride floats per sample, fields contiguous)
 * replaces: FM.forward torch_rechub/basic/layers.py:313-319 and its autograd
 * reduce_sum = 1 -> out (B,) ; 0 -> out (B, D)
 */
int rh_fm_fwd(const float* x, int64_t x_stride, int B, int F, int D, int reduce_sum, float* out,
              void* stream);
int rh_fm_bwd(const float* x, int64_t x_stride, int B, int F, int D, int reduce_sum,
              const float* g_out, float* g_x, int64_t gx_stride, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sequence features: gather + masked pooling
 * replaces: InputMask.forward basic/layers.py:148-161 + Sum/Average/ConcatPooling :204-251
 *           as called from EmbeddingLayer.forward basic/layers.py:86-99
 * idx (B, L) with sample stride idx_stride_b and position stride idx_stride_l (elements)
 * mode 0 = sum, 1 = mean (divide by count + 1e-16), 2 = concat (no mask, out (B, L, D))
 * mask_sentinel = padding_idx if set else -1 (positions equal to it are excluded from sum/mean)
 * out row b at out + b*out_stride (D floats, or L*D floats for concat).  D a power-of-two multiple of 4, <= RH_SEQ_POOL_MAX_D.
 */
#define RH_SEQ_POOL_MAX_D 128
int rh_seq_pool_fwd(const float* table, int64_t vocab, const void* idx, int idx_is_i64,
                    int64_t idx_stride_b, int64_t idx_stride_l, int B, int L, int D, int mode,
                    int64_t mask_sentinel, float* out, int64_t out_stride, int32_t* err_flag,
                    void* stream);
/* backward: scatter-add into grad_table; rows equal to padding_idx (or -1 = none) get no gradient */
int rh_seq_pool_bwd(float* grad_table, int64_t vocab, const void* idx, int idx_is_i64,
                    int64_t idx_stride_b, int64_t idx_stride_l, int B, int L, int D, int mode,
                    int64_t mask_sentinel, int64_t padding_idx, const float* g_out,
                    int64_t g_stride, float scale, int32_t* err_flag, void* stream);
/* Reports the lane split both launches above use for rows of D floats and L positions (HOST ints, launches nothing; the
 * function the launches themselves call): *lanes_per_row = D / 4 lanes on one table row, *pos_groups = the interleaved
 * position groups LS a sample's positions are dealt over (lane group ls takes l = j LS + ls), *trips = the passes of a lane
 * group's gather loop, 8 positions each: ceil(ceil(L / LS) / 8). */
int rh_seq_pool_split(int D, int L, int* lanes_per_row, int* pos_groups, int* trips);

/* ---------------------------------------------------------------------------------------------
 * K5  CrossNetwork  x_{l+1} = x0 * (w_l . x_l) + b_l + x_l
 * replaces: CrossNetwork.forward torch_rechub/basic/layers.py:412-420 and its autograd
 * x0, x : (B, d) with row strides; w, b : (L, d) contiguous; L <= 4 per call (chain calls for more,
 * passing the original x0).  One wavefront per sample, d <= RH_CROSS_MAX_D.
 * bwd: g_x0 / g_x may alias-sum: if sum_into_gx != 0 the x0-gradient is added into g_x and g_x0 is
 * ignored (the x0 == x case of the first segment).
 * wb_partials: (nblocks, 2, L, d) per-block partial sums of (dW, dB); nblocks is returned by
 * rh_cross_bwd_nblocks(B); the caller reduces over dim 0.
 */
#define RH_CROSS_MAX_D 2048
int rh_cross_fwd(const float* x0, int64_t x0_stride, const float* x, int64_t x_stride,
                 const float* w, const float* b, int B, int d, int L, float* out,
                 int64_t out_stride, void* stream);
int rh_cross_bwd_nblocks(int B);
/* *nblocks (a HOST int) = the workgroups rh_cross_fwd launches for B rows (four rows each per trip of its grid-stride loop) */
int rh_cross_fwd_nblocks(int B, int* nblocks);
int rh_cross_max_layers(int d); /* layers one call can take for width d (4 for d <= 512) */
int rh_cross_bwd(const float* x0, int64_t x0_stride, const float* x, int64_t x_stride,
                 const float* w, const float* b, int B, int d, int L, const float* g_out,
                 int64_t g_stride, float* g_x0, float* g_x, int64_t gx_stride, int sum_into_gx,
                 float* wb_partials, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DCN-v2 cross layers: the streaming epilogues around the library GEMMs (all tensors contiguous fp32)
 * rh_cross_v2_epilogue_* replaces: `x0 * self.w[i](x) + self.b[i] + x` of CrossNetV2.forward basic/layers.py:442-443
 *   fwd: out = x0*y + b + x   (y = W_l x from the GEMM);  bwd: g_x0 = g*y, g_y = g*x0  (g_x = g, g_b = colsum(g))
 * rh_cross_mix_epilogue_* replaces: the expert loop tail of CrossNetMix.forward basic/layers.py:491-503
 *   fwd: out = sum_e gate[b,e] * x0 * (uv[e,b,:] + bias) + xl     uv (E,B,d) = U_e v_e from the batched GEMM,
 *        gate (B,E) = softmax of the gating scores;
 *   bwd: g_x0 = g * sum_e gate_e (uv_e + bias), g_uv[e] = g * gate_e * x0, g_gate[b,e] = sum_d g*x0*(uv_e + bias)
 *        (g_xl = g, g_bias = colsum(g * x0 * sum_e gate_e) are the caller's).  d <= RH_CROSS_MIX_MAX_D,
 *        E <= RH_CROSS_MIX_MAX_E.
 */
#define RH_CROSS_MIX_MAX_D 2048
#define RH_CROSS_MIX_MAX_E 16
int rh_cross_v2_epilogue_fwd(const float* x0, const float* y, const float* b, const float* x, int B, int d, float* out,
                             void* stream);
int rh_cross_v2_epilogue_bwd(const float* x0, const float* y, const float* g, int B, int d, float* g_x0, float* g_y,
                             void* stream);
int rh_cross_mix_epilogue_fwd(const float* x0, const float* xl, const float* uv, const float* gate, const float* bias,
                              int B, int d, int E, float* out, void* stream);
int rh_cross_mix_epilogue_bwd(const float* x0, const float* uv, const float* gate, const float* bias, const float* g,
                              int B, int d, int E, float* g_x0, float* g_uv, float* g_gate, void* stream);
/* *nblocks (a HOST int) = the workgroups of either rh_cross_v2_epilogue_* launch (256 elements each per trip) */
int rh_cross_v2_epilogue_nblocks(int B, int d, int* nblocks);
/* the same, also emitting the bias gradient as rh_cross_mix_nblocks(B) x d per-block partial rows (summed by the caller);
 * rh_cross_mix_nblocks(B) is the grid of all three rh_cross_mix_epilogue_* launches (four rows each per trip) */
int rh_cross_mix_nblocks(int B);
int rh_cross_mix_epilogue_bwd_b(const float* x0, const float* uv, const float* gate, const float* bias, const float* g, int B,
                                int d, int E, float* g_x0, float* g_uv, float* g_gate, float* g_bias_partial, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CrossNetMix (DCN-v2 mixture of low-rank experts) as two dense products per layer (csrc/moe.hip)
 * replaces: the layer x expert loops of CrossNetMix.forward torch_rechub/basic/layers.py:470-506 and their autograd.
 *   KP = rh_cross_moe_kp(E, r) = E r + E rounded up to a multiple of 4.  Per layer l:
 *     PG (B, KP) = x_l VgT_l^T;  mid pass: v1 = tanh(PG[:, :E r]), v2_e = tanh(C_e v1_e), gate = softmax(PG[:, E r:E r+E]),
 *     wp (B, KP) = [gate_e v2_e | sum_e gate_e | 0];  Y (B, d) = wp UTb_l^T;  x_{l+1} = x0 * Y + x_l.
 *   rh_cross_moe_pack: VgT (L, KP, d) rows e r + k = V_l[e][:, k], rows E r + e = gating_e.weight;
 *                      UTb (L, d, KP) columns e r + k = U_l[e][:, k], column E r = bias_l.  U / V / bias / Wg: HOST arrays
 *                      of device pointers (L, L, L, E entries).
 *   rh_cross_moe_mid_fwd / _bwd: the pass between the two products; the backward takes g_wp (B, KP), writes g_PG (B, KP)
 *                      and rh_cross_moe_mid_blocks(B, E, r) partial rows (E r r) of g_C.
 *   rh_cross_moe_res_bwd: g_Y = g * x0, acc = ((mode & 1) ? 0 : acc) + g * Y + ((mode & 2) ? g : 0)  (acc: running gradient of
 *                      x0; g, x0 with row strides; bit 0 = first layer of the backward, bit 1 = last: acc also takes the residual
 *                      path's gradient, the caller's closing product accumulates into it).
 *   rh_cross_moe_unpack: sums the weight-gradient slabs of the two products (rh_linear_wgrad_partial: slabV_l = S1_l slabs
 *                      (KP, d) of g_PG^T x_l, slabU_l = S2_l slabs (d, KP) of g_Y^T wp) and the g_C partials into g_U, g_V
 *                      (E, d, r), g_bias (d,), g_C (E, r, r) per layer and g_Wg (d,) per expert (summed over the layers).
 *   Supported: L <= RH_CROSS_MOE_MAX_L, E <= RH_CROSS_MOE_MAX_E, r in {4, 8, 16, 32, 64} (RH_CROSS_MOE_MAX_R), E r <=
 *   RH_CROSS_MOE_MAX_ER (rh_cross_moe_supported); anything else runs the batched-GEMM formulation with rh_cross_mix_epilogue_*.
 */
#define RH_CROSS_MOE_MAX_L 8
#define RH_CROSS_MOE_MAX_E 16
#define RH_CROSS_MOE_MAX_R 64
#define RH_CROSS_MOE_MAX_ER 256
int rh_cross_moe_kp(int E, int r);
int rh_cross_moe_supported(int L, int E, int d, int r);
int rh_cross_moe_mid_blocks(int B, int E, int r);
/* The grids of the other launches, each answered through HOST ints by the function the launch itself calls:
 *   rh_cross_moe_mid_fwd_blocks: workgroups of rh_cross_moe_mid_fwd, each taking 256 / (E r) samples per trip;
 *   rh_cross_moe_res_blocks:     workgroups of rh_cross_moe_res_bwd, 256 of the B d elements each per trip;
 *   rh_cross_moe_pack_blocks:    workgroups of rh_cross_moe_pack, 256 of the 2 L KP d elements each per trip;
 *   rh_cross_moe_unpack_blocks:  *blocks = the workgroups of rh_cross_moe_unpack that walk the L (2 E d r + d) + E d outputs of
 *                                g_U / g_V / g_bias / g_Wg (256 each per trip), *c_blocks = the ones in front of them that sum
 *                                the g_C partials (64 outputs each, no loop over outputs). */
int rh_cross_moe_mid_fwd_blocks(int B, int E, int r, int* blocks);
int rh_cross_moe_res_blocks(int B, int d, int* blocks);
int rh_cross_moe_pack_blocks(int L, int E, int d, int r, int* blocks);
int rh_cross_moe_unpack_blocks(int L, int E, int d, int r, int* blocks, int* c_blocks);
int rh_cross_moe_pack(const float* const* U, const float* const* V, const float* const* bias, const float* const* Wg, int L,
                      int E, int d, int r, float* VgT, float* UTb, void* stream);
int rh_cross_moe_mid_fwd(const float* PG, const float* C, int B, int E, int r, float* v1, float* v2, float* gate, float* wp,
                         void* stream);
int rh_cross_moe_mid_bwd(const float* g_wp, const float* v1, const float* v2, const float* gate, const float* C, int B, int E,
                         int r, float* g_PG, float* gC_partial, void* stream);
int rh_cross_moe_res_bwd(const float* g, int64_t ldg, const float* x0, int64_t ldx0, const float* Y, int B, int d, int mode,
                         float* g_Y, float* acc, void* stream);
int rh_cross_moe_unpack(const float* const* slabV, const int* S1, const float* const* slabU, const int* S2,
                        const float* const* gC, const int* NB, int L, int E, int d, int r, float* const* g_U,
                        float* const* g_V, float* const* g_bias, float* const* g_C, float* const* g_Wg, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DIN: Dice activation and the memory-bound ends of the ActivationUnit
 * rh_dice_fwd/bwd replaces: Dice.forward torch_rechub/basic/activation.py:15-25 (row-wise statistics over the neurons)
 *   x (N, C) contiguous, alpha (1,), eps; bwd writes gx (N, C) and per-block partial sums of d/d alpha into
 *   alpha_partial (rh_dice_nblocks(N),) which the caller sums.
 * rh_din_att_input_fwd/bwd replaces: cat[t, h, t-h, t*h] of ActivationUnit.forward, models/ranking/din.py:80-81
 *   hist (B, L, D) with batch stride hist_stride (positions contiguous), tgt (B, D) with batch stride tgt_stride,
 *   out (B*L, 4D);  bwd: g (B*L, 4D) -> g_hist (B, L, D) contiguous, g_tgt (B, D)
 * rh_din_pool_fwd/bwd replaces: (att_weight.unsqueeze(-1) * history).sum(dim=1), models/ranking/din.py:92
 *   w (B, L) contiguous -> out (B, D);  bwd: g (B, D) -> g_hist (B, L, D), g_w (B, L)
 * Dice takes C <= RH_DICE_MAX_C neurons, the BatchNorm-folded passes C <= RH_BN_DICE_MAX_C; the attention ends take D a
 * power-of-two multiple of 4 up to RH_DIN_ATT_MAX_D.
 */
#define RH_DICE_MAX_C 2048
#define RH_BN_DICE_MAX_C 512
#define RH_DIN_ATT_MAX_D 128
int rh_dice_nblocks(int64_t N);
int rh_dice_fwd(const float* x, const float* alpha, float eps, int64_t N, int C, const float* bn_scale,
                const float* bn_shift, float* out, void* stream);
int rh_dice_bwd(const float* x, const float* g, const float* alpha, float eps, int64_t N, int C, float* gx,
                float* alpha_partial, void* stream);
/* BatchNorm1d -> Dice of the ActivationUnit's MLP (basic/layers.py:281-287 with activation "dice"), the normalisation
 * folded into the Dice passes so that the normalised tensor is never materialised:
 *   forward : rh_bn_stats_fwd (batch statistics -> stat (6, C): mean, rstd, -, -, scale, shift; running stats,
 *             num_batches_tracked; eval: from the running statistics) then rh_dice_fwd(h, ..., stat + 4C, stat + 5C, out)
 *   backward: rh_bn_dice_bwd_stats (g = dL/d out -> per-block (sum g_x, sum g_x * xhat) rows, col_partial
 *             (rh_bn_dice_stats_blocks(N), 2, C), and alpha partial sums (same number of blocks)),
 *             rh_bn_finalize_bwd (-> stat rows 2, 3, dgamma, dbeta), rh_bn_dice_bwd_apply (-> dh).   C <= RH_BN_DICE_MAX_C. */
int rh_bn_stats_fwd(const float* h, int B, int C, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, int64_t* num_batches_tracked, float momentum, float eps, int training,
                    float* partial, float* stat, void* stream);
int rh_bn_finalize_bwd(float* partial, int rows, int C, float* stat, float* dgamma, float* dbeta, void* stream);
/* ... and, in the same launch, the other per-block partials of the statistics pass: extra (rows, C) -> extra_out (C) (the
 * attention head's weight gradient; null = none) and nscal <= 8 scalar rows scal (nscal, rows) -> scal_out (nscal) (Dice's alpha,
 * the head's bias; 0 = none).  Replaces torch_rechub/basic/activation.py:15-25's autograd sums over the (B L)-row tensors.
 * Fixed summation order. */
int rh_bn_finalize_bwd_tail(float* partial, int rows, int C, float* stat, float* dgamma, float* dbeta, const float* extra,
                            float* extra_out, const float* scal, int nscal, float* scal_out, void* stream);
int rh_bn_dice_stats_blocks(int64_t N);
int rh_bn_dice_bwd_stats(const float* h, const float* g, const float* alpha, float eps, int64_t N, int C,
                         const float* stat, const float* gamma, float* col_partial, float* alpha_partial, void* stream);
int rh_bn_dice_bwd_apply(const float* h, const float* g, const float* alpha, float eps, int64_t N, int C,
                         const float* stat, const float* gamma, float* dh, void* stream);
/* BatchNorm1d -> Dice -> [Dropout(0)] -> Linear(C, 1): the tail of the ActivationUnit's MLP (basic/layers.py:281-288, the
 * output layer of MLP(4 * emb_dim, dims=...), models/ranking/din.py:74).  The Dice output has ONE consumer, a C -> 1 dot
 * product, so it is never written: forward out (N,) = Dice(bn(h)) . head_w + head_b; backward g (N,) = dL/d out, the
 * gradient of the Dice output is g[r] * head_w[c] in registers.  rh_bn_dice_head_bwd_stats writes, besides col_partial
 * (blocks, 2, C), alpha_partial (2, blocks) = [d alpha partials | dL/d head_b partials] and head_partial (blocks, C) =
 * partial dL/d head_w (Dice output recomputed); blocks = rh_bn_dice_stats_blocks(N); the caller sums over blocks. */
int rh_bn_dice_head_fwd(const float* h, const float* alpha, float eps, int64_t N, int C, const float* bn_scale,
                        const float* bn_shift, const float* head_w, const float* head_b, float* out, void* stream);
int rh_bn_dice_head_bwd_stats(const float* h, const float* g, const float* alpha, float eps, int64_t N, int C,
                              const float* stat, const float* gamma, const float* head_w, float* col_partial,
                              float* alpha_partial, float* head_partial, void* stream);
int rh_bn_dice_head_bwd_apply(const float* h, const float* g, const float* alpha, float eps, int64_t N, int C,
                              const float* stat, const float* gamma, const float* head_w, float* dh, void* stream);
int rh_din_att_input_fwd(const float* hist, int64_t hist_stride, const float* tgt, int64_t tgt_stride, int B, int L,
                         int D, float* out, void* stream);
int rh_din_att_input_bwd(const float* hist, int64_t hist_stride, const float* tgt, int64_t tgt_stride, const float* g,
                         int B, int L, int D, float* g_hist, float* g_tgt, void* stream);
int rh_din_pool_fwd(const float* hist, int64_t hist_stride, const float* w, int B, int L, int D, float* out,
                    void* stream);
int rh_din_pool_bwd(const float* hist, int64_t hist_stride, const float* w, const float* g, int B, int L, int D,
                    float* g_hist, float* g_w, void* stream);
/* Reports the lane split the four launches above use for a history of L rows of D floats (HOST ints, launches nothing; the
 * function the launches themselves call): *lanes_per_row = D / 4, *pos_groups = the position groups LS (1, 4 or 16) a
 * sample's rows are dealt over. */
int rh_din_att_split(int D, int L, int* lanes_per_row, int* pos_groups);
/* First layer of the ActivationUnit's MLP with the operand built in registers (csrc/dinmlp.hip); replaces
 * models/ranking/din.py:81-85 (expand + cat + view) and the Linear(4 D, N) of basic/layers.py:279 on it:
 *   z (B L, N) = [t, h, t - h, t * h] W^T + bias;  the (B L, 4 D) operand never exists in memory.
 *   partial (optional): ceil(B L / rh_din_att_l1_chunk_rows(B L)) x 2 x N per-chunk (sum, M2 about the chunk mean) of z --
 *   the BatchNorm statistics, combined by rh_bn_stats_from_partial (no pass over z).
 *   Supported (rh_din_att_l1_supported): D in {4, 8, 16} (RH_DIN_ATT_L1_MAX_D), N a multiple of 64 up to
 *   RH_DIN_ATT_L1_MAX_N. */
#define RH_DIN_ATT_L1_MAX_D 16
#define RH_DIN_ATT_L1_MAX_N 256
/* nn.PReLU() with one slope (activation_layer("prelu"), torch_rechub/basic/activation.py:40-41; the DSSM towers): x contiguous,
 * n elements; bwd writes gx and rh_prelu_nblocks(n) per-block partial sums of d / d slope. */
int rh_prelu_nblocks(int64_t n);
int rh_prelu_fwd(const float* x, const float* slope, int64_t n, float* out, void* stream);
int rh_prelu_bwd(const float* x, const float* g, const float* slope, int64_t n, float* gx, float* partial, void* stream);
/* In-batch negatives without the (B, C) score matrix (csrc/match.hip); replaces, for RANDOM negatives,
 * `scores = user @ item.T` + `gather_inbatch_logits(scores, neg_indices)` of trainers/match_trainer.py:118-138 /
 * utils/match.py:148-153 and their autograd:  logits[i, 0] = u_i . v_(row0 + i),  logits[i, 1 + k] = u_i . v_neg[i, k];
 * bwd: g_u (B, D) written, g_v (C, D) accumulated with float atomics into a buffer the caller zeroed.  D <= RH_INBATCH_MAX_D. */
#define RH_INBATCH_MAX_D 1024
int rh_inbatch_logits_fwd(const float* u, int64_t ldu, const float* v, int64_t ldv, const int64_t* neg, int B, int C, int D,
                          int K, int row0, float* logits, int32_t* err_flag, void* stream);
int rh_inbatch_logits_bwd(const float* u, int64_t ldu, const float* v, int64_t ldv, const int64_t* neg, const float* g, int B,
                          int C, int D, int K, int row0, float* g_u, float* g_v, void* stream);

/* Two-tower glue as single launches.
 * rh_l2norm_fwd/bwd: F.normalize(x, p=2, dim=1) of the towers' outputs (torch_rechub/models/matching/dssm.py:56,66):
 *   y = x / max(||x||_2, eps) row-wise, nrm (B,) = ||x|| saved; gx = (g - y (g . y)) / ||x||, or g / eps where the norm was
 *   clamped.  x / g row stride ldx / ldg (multiples of 4), d % 4 == 0, RH_L2NORM_MIN_D <= d <= RH_L2NORM_MAX_D; y, gx contiguous (B, d).
 * rh_ce_fwd/bwd: torch.nn.CrossEntropyLoss() (mean) over the (B, C) in-batch logits (trainers/match_trainer.py:60,136;
 *   target int64 (B,), null = class 0 for every row as the trainer's zero targets): lse (B,) = logsumexp per row, loss_partial
 *   (rh_ce_nblocks(B),) per-block sums of lse - x[target] (the caller sums them and divides by B: rh_colsum);
 *   g_logits = g_loss[0] / B * (softmax - onehot), the softmax taken from the logits again as exp((x - max) - log sum): the
 *   backward requires lse but does not read it (its rounding would be the error of p - 1 at the target).  C <= RH_CE_MAX_C; an
 *   out-of-range target sets RH_FLAG_INDEX_OOB. */
#define RH_L2NORM_MIN_D 4
#define RH_L2NORM_MAX_D 4096
#define RH_CE_MAX_C 1024
int rh_l2norm_fwd(const float* x, int64_t ldx, int B, int d, float eps, float* y, float* nrm, void* stream);
int rh_l2norm_bwd(const float* y, const float* nrm, const float* g, int64_t ldg, int B, int d, float eps, float* gx, void* stream);
int rh_ce_nblocks(int B);
int rh_ce_fwd(const float* logits, const int64_t* target, int B, int C, float* lse, float* loss_partial, int32_t* err_flag,
              void* stream);
int rh_ce_bwd(const float* logits, const int64_t* target, const float* lse, const float* g_loss, int B, int C, float* g_logits,
              void* stream);
int rh_din_att_l1_supported(int D, int N);
int rh_din_att_l1_chunk_rows(int64_t rows);
int rh_din_att_l1_fwd(const float* hist, int64_t hist_stride, const float* tgt, int64_t tgt_stride, const float* W,
                      const float* bias, int B, int L, int D, int N, float* z, float* partial, void* stream);
/* rh_bn_stats_fwd (training) from per-chunk partials that a producer already emitted: finalize only. */
int rh_bn_stats_from_partial(const float* partial, int rows_per_chunk, int B, int C, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                             float eps, float* stat, void* stream);

/* ---------------------------------------------------------------------------------------------
 * MLP Linear weight gradient, the (., 1) output head and the BCE loss (csrc/linear.hip)
 * rh_linear_wgrad replaces: the weight/bias gradient of every nn.Linear of MLP, torch_rechub/basic/layers.py:279,290
 *   (autograd's mm(g^T, x) + sum(g, 0)):  dW (N, K) = g^T x,  db (N,) = column sums of g (db may be NULL)
 *   g (B, N) row stride ldg, x (B, K) row stride ldx; batch split over blocks, f32 MFMA, partial tiles summed in split
 *   order by a second small launch (deterministic).  partial: rh_linear_wgrad_workspace(B, N, K) floats.
 * rh_head_fwd/bwd replaces: MLP's output Linear(K, 1) + `y_linear + y_fm + y_deep` + torch.sigmoid(y.squeeze(1)),
 *   models/ranking/deepfm.py:39-43, widedeep.py:35-39:  y (B,) = sigmoid(h w^T + bias + e0 + e1)  (bias, e0, e1 optional)
 *   bwd: g_z = g_y y (1 - y) (also the gradient of e0 / e1), g_h (B, K) = g_z w, g_w (K,) = g_z^T h, g_b = sum g_z.
 *   1 <= K <= RH_HEAD_MAX_K (rows of h may be only 4-byte aligned).  partial: rh_head_nblocks(B) * (K + 1) floats.
 * rh_bce_fwd/bwd replaces: torch.nn.BCELoss() (mean) of trainers/ctr_trainer.py:62,:93-95: log terms clamped at -100;
 *   loss (1,), g_loss (1,) device scalars.
 */
#define RH_HEAD_MAX_K 1024
/* rh_linear_fwd / rh_linear_dgrad replace: the forward y = x W^T + b and the input gradient g_x = g W of the same
 *   nn.Linear modules (aten::addmm / mm) at CTR batch sizes, where one 64x64 f32-MFMA tile per workgroup fills the chip
 *   exactly once (csrc/gemm.hip).  x (M, K) row stride ldx, w (N, K) row stride ldw, bias (N,) or NULL, y (M, N).
 *   stats (NULL or (ceil(M / R), 2, N) floats, R = rh_gemm_stats_rows(M, N) = 64 or 32): per R-row slab of y and
 *   column, the slab sum and M2 = sum (y - slab mean)^2 -- the input rh_bn_relu_dropout_fwd takes with partial_rows = R.
 *   bn_rng / bn_saved_ctr / bn_batches (optional, with stats): the consuming rh_bn_relu_dropout_fwd call's dropout
 *   state (rng[1] = call counter) and num_batches_tracked; the GEMM then performs that call's bookkeeping
 *   (saved_ctr = rng[1]++, batches += 1) and rh_bn_relu_dropout_fwd (partial_rows > 0) then advances nothing.
 *   rh_linear_dgrad: g (M, N), w (N, K) -> gx (M, K).  Exact f32 (MFMA f32 == fmaf chain); summation order over k is
 *   permuted inside each 32-wide K tile. */
int rh_gemm_stats_rows(int M, int N);
int rh_gemm_chain_stats_rows(int M); /* slab height of the `stats` rh_linear_bnact_fwd writes (64, or 32 when M <= 32) */
int rh_linear_fwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, int M, int N, int K,
                  float* y, int64_t ldy, float* stats, int64_t* bn_rng, int64_t* bn_saved_ctr, int64_t* bn_batches,
                  void* stream);
/* rh_linear_fwd that also counts a CHAIN START in the deferred sweep's gate words (chain_gate[2], RH_GATE_WORDS below) when its
 * last workgroup starts, i.e. when every workgroup of the launch has been placed: captured as the first own GEMM of a step's
 * hipGraph it releases the optimizer's sweep of the step before (rh_adam_sweep_gate) beside a chain that is already running. */
int rh_linear_fwd_gate(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, int M, int N, int K,
                       float* y, int64_t ldy, float* stats, int64_t* bn_rng, int64_t* bn_saved_ctr, int64_t* bn_batches,
                       int64_t* chain_gate, void* stream);
int rh_linear_dgrad(const float* g, int64_t ldg, const float* w, int64_t ldw, int M, int N, int K, float* gx,
                    int64_t ldgx, void* stream);
/* One CrossNetV2 layer (torch_rechub/basic/layers.py:440-444: x <- x0 * (W_l x) + b_l + x) on the tile GEMM with the Hadamard +
 * bias + residual as its epilogue (round 5; rounds 1-4: library GEMM + rh_cross_v2_epilogue_fwd as a second pass).
 * rh_cross_v2_fwd: x0, x (M, d), w (d, d) row-major as nn.Linear.weight, b (d,) -> y (M, d) = x w^T (kept for the backward) and
 * out (M, d) = x0 * y + b + x.  rh_cross_v2_dgrad: gx (M, d) = g_y w + g with g_y = g * x0 (rh_cross_v2_epilogue_bwd forms g_y
 * and g_x0 = g * y): the layer's gradient with respect to x, residual path included.  Every operand contiguous (row stride d);
 * 1 <= M <= RH_CROSS_V2_MAX_M, 1 <= d <= RH_CROSS_V2_MAX_D, else RH_E_UNSUPPORTED. */
#define RH_CROSS_V2_MAX_M 16384
#define RH_CROSS_V2_MAX_D 1024
int rh_cross_v2_fwd(const float* x0, const float* x, const float* w, const float* b, int M, int d, float* y, float* out,
                    void* stream);
int rh_cross_v2_dgrad(const float* g_y, const float* w, const float* g, int M, int d, float* gx, void* stream);
/* The fused MLP chain (round 4): the reference's hidden-layer tail  BatchNorm1d -> ReLU -> Dropout
 * (torch_rechub/basic/layers.py:283-286) is never run as a pass of its own -- it is applied where its output is consumed.
 * rh_linear_bnact_fwd: layer l + 1 as ONE launch, y = dropout(relu(batch_norm(h))) W^T + b with h (M, K) the PRE-BatchNorm
 *   output of layer l.  pro_stats (ceil(M / pro_rows), 2, K): the per-slab (sum, M2) the producing GEMM wrote as `stats`
 *   (pro_rows = rh_gemm_stats_rows(M, K)); gamma / beta / running_* / momentum / eps: layer l's nn.BatchNorm1d; p_drop, rng,
 *   ctr: its nn.Dropout and the counter the producing GEMM drew for it (that call's bn_saved_ctr).  Written besides y:
 *   stat_out (>= 2, K) = mean, rstd of layer l; its running statistics; act_out (M, K) or NULL = the activations (this
 *   layer's weight gradient reads them); stats / bn_rng / bn_saved_ctr / bn_batches: as rh_linear_fwd, for y and the NEXT
 *   BatchNorm.  K % 4 == 0, K <= RH_LINEAR_BNACT_MAX_K, ldh % 4 == 0.  Same per-element arithmetic as rh_bn_relu_dropout_fwd.
 * rh_linear_dgrad_bnbwd: rh_linear_dgrad whose epilogue also forms the BatchNorm-backward column sums of the hidden layer
 *   that produced this Linear's input: gx (M, K) = gradient of a = dropout(relu(batch_norm(h))), h (M, K) that layer's
 *   pre-BatchNorm activations, stat (>= 2, K) its mean / rstd, ctr its dropout counter.  bwd_partial (ceil(M / R), 2, K),
 *   R = rh_gemm_stats_rows(M, K): per R-row slab (sum g1, sum g1 * xhat) -- rh_bn_relu_dropout_bwd_pre's `partial` with
 *   nchunks_pre = ceil(M / R) (replaces the statistics launch of the BatchNorm backward).
 * rh_head_bnact_fwd: the output head of such a chain, y = sigmoid(dropout(relu(batch_norm(z))) . w + b + e0 + e1), z (B, K)
 *   pre-BatchNorm, stats / stats_rows / ctr as above; t / loss_partial as rh_head_loss_fwd (both NULL: no loss terms).
 *   K % 4 == 0, K <= RH_HEAD_BN_MAX_K.  Its backward is rh_head_bwd_bn with h = NULL (the head's input is recomputed from z). */
#define RH_LINEAR_BNACT_MAX_K 1024
#define RH_HEAD_BN_MAX_K 256
int rh_linear_bnact_fwd(const float* h, int64_t ldh, int M, int K, const float* pro_stats, int pro_rows, const float* gamma,
                        const float* beta, float* running_mean, float* running_var, float momentum, float eps, float p_drop,
                        const int64_t* rng, const int64_t* ctr, float* stat_out, float* act_out, const float* w, int64_t ldw,
                        const float* bias, int N, float* y, int64_t ldy, float* stats, int64_t* bn_rng, int64_t* bn_saved_ctr,
                        int64_t* bn_batches, void* stream);
int rh_linear_dgrad_bnbwd(const float* g, int64_t ldg, const float* w, int64_t ldw, int M, int N, int K, float* gx,
                          int64_t ldgx, const float* h, int64_t ldh, const float* stat, const float* gamma, const float* beta,
                          float p_drop, const int64_t* rng, const int64_t* ctr, float* bwd_partial, void* stream);
int rh_head_bnact_fwd(const float* z, int64_t ldz, const float* stats, int stats_rows, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float momentum, float eps, float p_drop, const int64_t* rng,
                      const int64_t* ctr, float* stat_out, const float* w, const float* bias, const float* e0, const float* e1,
                      int B, int K, float* y, const float* t, float* loss_partial, void* stream);
int64_t rh_linear_wgrad_workspace(int B, int N, int K);
int rh_linear_wgrad_tiles(int N, int K);
int rh_linear_wgrad(const float* g, int64_t ldg, const float* x, int64_t ldx, int B, int N, int K, float* dW, float* db,
                    float* partial, void* stream);
/* The same without the reduction launch: partial = S slabs (N, K) followed by S slabs (N,), S = rh_linear_wgrad_splits;
 * the caller sums them (rh_pack_grads folds that into the packing of the step's dense gradients). */
int rh_linear_wgrad_splits(int B, int N, int K);
int rh_linear_wgrad_partial(const float* g, int64_t ldg, const float* x, int64_t ldx, int B, int N, int K, float* partial,
                            void* stream);
/* n <= 8 independent rh_linear_wgrad_partial problems as ONE launch (the two weight gradients per layer of CrossNetMix's
 * backward, torch_rechub/basic/layers.py:470-506: nothing else in that backward waits for them).  Host arrays of n entries.
 * Every B[i] < RH_WGRAD_LONG_MIN_B: a reduction of that many rows or more is a long one and takes the single call. */
#define RH_WGRAD_LONG_MIN_B 32768
int rh_linear_wgrad_partial_group(int n, const float* const* g, const int64_t* ldg, const float* const* x, const int64_t* ldx,
                                  const int* B, const int* N, const int* K, float* const* partial, void* stream);
int rh_head_nblocks(int B);
int rh_head_fwd(const float* h, int64_t ldh, const float* w, const float* bias, const float* e0, const float* e1, int B,
                int K, float* y, void* stream);
int rh_head_bwd(const float* h, int64_t ldh, const float* w, const float* y, const float* g_y, int B, int K, float* g_h,
                float* g_z, float* g_w, float* g_b, float* partial, void* stream);
/* Column sums of the per-block partial buffers the backward kernels emit (replaces the trailing `.sum(0)` / `.sum()`
 * launches of autograd): out (cols,) = sum over rows of a (rows, cols); optionally vsum (1,) = sum of v (n,). */
int rh_colsum(const float* a, int rows, int cols, float* out, const float* v, int64_t n, float* vsum, void* stream);
/* Fused head + loss for the trainer's step (models/ranking/deepfm.py:39-43 + torch.nn.BCELoss trainers/ctr_trainer.py:62,88):
 * rh_head_loss_fwd = rh_head_fwd that also emits, per block, the sum of the BCE terms of its rows against the labels t
 *   (loss_partial: rh_head_loss_nblocks(B) floats; the mean is finished by rh_step_scalars);
 * rh_head_loss_bwd = rh_bce_bwd + rh_head_bwd in one pass: g_y = g_loss[0] / B * (y - t) / max((1 - y) y, 1e-12) is
 *   formed per row with the arithmetic of rh_bce_bwd (bit-identical to the two separate launches).
 *   rh_head_bwd_ex / rh_head_bwd_bn take g_y, (t, g_loss) or both (a prediction with a second consumer besides the
 *   loss: the inline BCE gradient and g_y add per row).
 * rh_step_scalars: the scalar work of one training step in ONE single-block launch (each part optional, null = skip):
 *   loss[0] = sum(loss_partial[0..n_partial)) / B;  the bias corrections of the next Adam step (== rh_adam_prepare);
 *   two device counters c = (c + inc) % mod (mod 0 = no wrap): the batch position of the device loader (==
 *   rh_batch_advance), the call counter of the in-batch sampler. */
int rh_head_bwd_ex(const float* h, int64_t ldh, const float* w, const float* y, const float* g_y, const float* t,
                   const float* g_loss, int B, int K, float* g_h, float* g_z, float* g_w, float* g_b, float* partial,
                   int reduce, void* stream);
/* rh_head_bwd_ex + the BatchNorm-backward column sums of the hidden layer below the head, when h = dropout(relu(bn(bn_z)))
 * and the head is its only consumer: bn_partial (rh_head_nblocks(B), 2, K) per-block (sum g1, sum g1 * xhat) with the mask
 * arithmetic of rh_bn_relu_dropout_bwd; rh_bn_relu_dropout_bwd_pre then needs no statistics pass.  K % 4 == 0, K <= RH_HEAD_BN_MAX_K. */
int rh_head_bwd_bn(const float* h, int64_t ldh, const float* w, const float* y, const float* g_y, const float* t,
                   const float* g_loss, int B, int K, float* g_h, float* g_z, float* g_w, float* g_b, float* partial,
                   int reduce, const float* bn_z, const float* bn_stat, const float* bn_gamma, const float* bn_beta,
                   float bn_p, const int64_t* bn_rng, const int64_t* bn_ctr, int bn_relu, float* bn_partial, void* stream);
/* rh_head_bwd_bn + rh_step_scalars as ONE launch (one extra workgroup does the scalar work; arguments as rh_step_scalars):
 * nothing between the head's forward and its backward reads the loss mean / Adam corrections / device counters. */
int rh_head_bwd_bn_scalars(const float* h, int64_t ldh, const float* w, const float* y, const float* g_y, const float* t,
                           const float* g_loss, int B, int K, float* g_h, float* g_z, float* g_w, float* g_b, float* partial,
                           int reduce, const float* bn_z, const float* bn_stat, const float* bn_gamma, const float* bn_beta,
                           float bn_p, const int64_t* bn_rng, const int64_t* bn_ctr, int bn_relu, float* bn_partial,
                           const float* loss_partial, int n_partial, float* loss, double* hyper, int64_t* step, float* ring,
                           int ring_size, int64_t* c0, int64_t inc0, int64_t mod0, int64_t* c1, int64_t inc1, int64_t mod1,
                           void* stream);
int rh_head_loss_nblocks(int B);
int rh_head_loss_fwd(const float* h, int64_t ldh, const float* w, const float* bias, const float* e0, const float* e1, int B,
                     int K, float* y, const float* t, float* loss_partial, void* stream);
int rh_head_loss_bwd(const float* h, int64_t ldh, const float* w, const float* y, const float* t, const float* g_loss, int B,
                     int K, float* g_h, float* g_z, float* g_w, float* g_b, float* partial, void* stream);
int rh_step_scalars(const float* loss_partial, int n_partial, int64_t B, float* loss, double* hyper, int64_t* step,
                    float* ring, int ring_size, int64_t* c0, int64_t inc0, int64_t mod0, int64_t* c1, int64_t inc1,
                    int64_t mod1, void* stream);
int rh_bce_fwd(const float* y, const float* t, int64_t B, float* loss, void* stream);
int rh_bce_bwd(const float* y, const float* t, const float* g_loss, int64_t B, float* g_y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * MLP hidden-layer epilogue: BatchNorm1d + ReLU + Dropout fused (the Linear in front stays a library GEMM)
 * replaces: nn.BatchNorm1d -> ReLU -> nn.Dropout of MLP, torch_rechub/basic/layers.py:281-287, and their autograd
 * relu = 1: the MLP hidden layer BatchNorm1d -> ReLU -> Dropout; relu = 0: BatchNorm1d (-> Dropout) only, for the layers
 * whose activation is Dice / PReLU / ... (MLP of DIN's ActivationUnit, the DSSM towers).
 * h (B,C) pre-BN activations; training: batch statistics (biased variance), running stats updated with `momentum`
 * (unbiased variance), num_batches_tracked += 1; eval: running statistics, no dropout.
 * rng (device int64 [4]): seed, call counter (bumped by the forward), block ticket (zero on entry / exit), spare;
 * saved_ctr (device int64 [1]): the counter this call used — the backward recomputes the same dropout mask from it
 * (nothing is stored).  B <= 8192: two launches per direction (partial sums; finalize folded into apply), else three.
 * partial: (rh_bn_act_nchunks(B), 2, C) floats; stat: (4, C) floats (mean, rstd kept for the backward).
 * partial_rows > 0 (forward): `partial` ALREADY holds, per partial_rows-row slab and column, the slab's sum and its
 * M2 = sum (h - slab mean)^2 -- rh_linear_fwd writes exactly that (64- or 32-row slabs) from its accumulators, so the
 * statistics pass over h disappears; the slabs are combined with Chan's parallel-variance formula in slab order.
 * rng / num_batches_tracked were then already advanced by rh_linear_fwd (it was given the same pointers): this call
 * reads saved_ctr and advances nothing.
 */
int rh_bn_act_nchunks(int B);
/* *nblocks (a HOST int) = the workgroups of the apply launch of the three-launch path over n = B * C elements, either
 * direction, and of the eval-mode forward (1024 elements each per trip) */
int rh_bn_apply_nblocks(int64_t n, int* nblocks);
int rh_bn_relu_dropout_fwd(const float* h, int B, int C, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float p_drop,
                           int training, int64_t* rng, int64_t* saved_ctr, float* partial, int partial_rows, float* stat,
                           float* out, int relu, void* stream);
/* the same with the column sums already formed by the producer of dy (rh_head_bwd_bn): nchunks_pre <= RH_BN_PRE_MAX_CHUNKS
 * partial rows */
#define RH_BN_PRE_MAX_CHUNKS 128
int rh_bn_relu_dropout_bwd_pre(const float* h, const float* dy, int B, int C, const float* gamma, const float* beta,
                               float p_drop, const int64_t* rng, const int64_t* saved_ctr, const float* partial,
                               int nchunks_pre, float* stat, float* dx, float* dgamma, float* dbeta, int relu, void* stream);
int rh_bn_relu_dropout_bwd(const float* h, const float* dy, int B, int C, const float* gamma, const float* beta,
                           float p_drop, const int64_t* rng, const int64_t* saved_ctr, float* partial, float* stat,
                           float* dx, float* dgamma, float* dbeta, int relu, void* stream);
/* The same two passes with nn.PReLU() (ONE slope) in place of the ReLU: Linear -> BatchNorm1d -> PReLU -> Dropout of the
 * two-tower MLPs (reference MLP(activation="prelu"), examples/matching/run_ml_dssm.py:69-80; basic/layers.py:276-292).
 * y = bn > 0 ? bn : slope[0] * bn.  The backward also writes slope_partial (rh_bn_prelu_nblocks(B, C) floats): per-workgroup
 * sums of dy * min(bn, 0), whose total is the slope's gradient.  Training mode only (eval: BatchNorm pass + rh_prelu_fwd). */
int rh_bn_prelu_dropout_fwd(const float* h, int B, int C, const float* gamma, const float* beta, float* running_mean,
                            float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float p_drop,
                            int training, int64_t* rng, int64_t* saved_ctr, float* partial, int partial_rows, float* stat,
                            float* out, const float* slope, void* stream);
int rh_bn_prelu_nblocks(int B, int C);
int rh_bn_prelu_dropout_bwd(const float* h, const float* dy, int B, int C, const float* gamma, const float* beta, float p_drop,
                            const int64_t* rng, const int64_t* saved_ctr, float* partial, float* stat, float* dx,
                            float* dgamma, float* dbeta, const float* slope, float* slope_partial, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense Adam with coupled L2, torch.optim.Adam semantics over every row of every table
 * replaces: optimizer.step() torch_rechub/trainers/ctr_trainer.py:59-61,99 for embedding tables
 * tdesc (device int64 [5*T]): p, g, m, v pointers and numel per tensor (T <= RH_ADAM_MAX_TENSORS)
 * h_numel (HOST int64 [T]): the same numel values (multiples of 4), used to size the launch
 * hyper (device double [16]): inputs  [0]=lr [1]=beta1 [2]=beta2 [3]=eps [4]=weight_decay
 *                             derived [8]=step_size=lr/(1-beta1^t) [9]=sqrt(1-beta2^t)
 *                                     [10]=1-beta1 [11]=1-beta2 [12]=t
 * rh_adam_prepare increments *step (device int64) and fills hyper[8..12] on the device in fp64
 * (as torch does on the host), so prepare + dense can be replayed from a hipGraph.
 * per element (fp32): g' = g + wd*p; m += (1-b1)*(g'-m); v = v*b2 + (1-b2)*g'^2;
 *                     p -= step_size * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * zero_grad != 0: g <- 0 where it was non-zero (replaces model.zero_grad(), ctr_trainer.py:97)
 */
#define RH_ADAM_MAX_TENSORS 128
int rh_adam_prepare(double* hyper, int64_t* step, float* ring, int ring_size, void* stream);
int rh_adam_dense(const int64_t* tdesc, int T, const int64_t* h_numel, const double* hyper,
                  int zero_grad, void* stream);

/* Adam for the small dense parameters (MLP / LR / cross weights) in one launch; gradients are read from the packed
 * flat bucket (the buffer the RCCL all-reduce runs on).  Any numel, 4-byte alignment.  Uses hyper[] of rh_adam_prepare.
 * sdesc (device int64 [5*T]): p, m, v pointers, numel, offset of the parameter's gradient inside flat_g (T <= RH_ADAM_MAX_TENSORS).
 * replaces: optimizer.step() for the non-embedding parameters, trainers/ctr_trainer.py:99 */
int rh_adam_small(const int64_t* sdesc, int T, const int64_t* h_numel, const float* flat_g, const double* hyper,
                  void* stream);

/* Pack the dense gradients of one step into the flat bucket (replaces: torch.cat over the parameter gradients + the
 * trailing partial-sum launch of every backward kernel; autograd's `.sum(0)` / accumulate kernels in the reference,
 * trainers/ctr_trainer.py:97-98):  flat[dst_offset + i] = sum_{r < nparts} src[r * stride + i] (+ add[i]),  i < numel,
 * summed in the fixed order r = 0, 1, ... (deterministic).  nparts == 0 writes zeros.  `items` is a HOST array; its
 * entries travel by value in the kernel arguments (hipGraph-capturable although the slabs are temporaries). */
typedef struct RhPackItem {
  uint64_t src;       /* device pointer to the partial rows (float) */
  uint64_t add;       /* device pointer to a plain (numel,) term added on top, or 0 */
  int64_t nparts;     /* rows to sum */
  int64_t stride;     /* floats between consecutive rows */
  int64_t numel;      /* elements of the parameter */
  int64_t dst_offset; /* offset of the parameter inside flat */
} RhPackItem;
int rh_pack_grads(const RhPackItem* items, int n, float* flat, void* stream);
/* the same + the Adam step of every packed parameter on the element just summed (= rh_pack_grads then rh_adam_small over the
 * same n parameters, sdesc in rh_adam_small's layout, hyper already holding this step's scalars): one launch */
int rh_pack_grads_adam(const RhPackItem* items, int n, float* flat, const int64_t* sdesc, const double* hyper, void* stream);
/* rh_pack_grads_adam whose launch also counts an opening of `gate` (as rh_adam_sweep_gate_open) when it STARTS: captured
 * behind the end-of-step table launch it announces that launch's end without a launch of its own.  gate may be NULL. */
int rh_pack_grads_adam_gate(const RhPackItem* items, int n, float* flat, const int64_t* sdesc, const double* hyper,
                            int64_t* gate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Blocked-lazy EXACT Adam (same arithmetic as rh_adam_dense, bit-identical results, ~1/K of its HBM traffic)
 * replaces: the same optimizer.step() (trainers/ctr_trainer.py:99).  Adam is element-wise and a row that is not in
 * the batch has the known gradient wd*p, so rows are brought up to date lazily by replaying the skipped steps in
 * registers; every row is refreshed at least every K steps (sweep window) and immediately when the batch touches it.
 * ring  (device float [2*ring_size], ring_size a power of two > K and <= RH_ADAM_MAX_RING): per-step (A_t, E_t) written by rh_adam_prepare
 *       (hyper[13] = A_t = step_size*sqrt(1-b2^t), hyper[14] = E_t = eps*sqrt(1-b2^t))
 * ldesc (device int64 [8*T]): p, g, m, v, last (int32 per row: step the row is up to date with) pointers,
 *       rows, K_t (1 = dense table, stepped with its gradient by the sweep), window rows w_t = ceil(rows/K_t)
 * rh_adam_lazy_touched: for every lookup of the batch (index columns in idesc, as rh_embed_bwd) claim the row,
 *       replay it to step t-1, apply step t with its gradient row, re-zero the gradient row.
 *       field_table (device int64 [2*F]): table index of field f (-1 = skip), padding_idx (-1 = none)
 *       refresh != 0: the pre-gather pass (rows about to be READ are brought to the hyper step; their gradient rows
 *       are zero by construction and are neither read nor written)
 * rh_adam_lazy_sweep: bring window (t-1) mod K_t of every table up to date.  mode: RH_SWEEP_WINDOW = every table,
 *       RH_SWEEP_FLUSH = all rows of every table, RH_SWEEP_LAZY_TABLES = windows of the K_t > 1 tables only,
 *       RH_SWEEP_DENSE_TABLES = the K_t == 1 tables only (these take their gradient in the sweep).
 * Call order per step: rh_adam_prepare, rh_adam_lazy_touched (once per index batch), rh_adam_lazy_sweep.
 * t_value < 0: the sweep belongs to the step in hyper (in line, before the next rh_adam_prepare).  t_value = s >= 0:
 * deferred sweep of step s, step number by value and (A_s, E_s) from the ring -- it only touches rows that are NOT at
 * step >= s, so it may run on another stream concurrently with the whole of step s + 1 (its rh_adam_prepare,
 * forward, backward, rh_adam_lazy_touched), PROVIDED step s + 1 brought its own rows up to step s before the sweep
 * was launched (rh_adam_lazy_touched under the hyper of step s = the pre-gather refresh) and the sweep has finished
 * before step s + 2 refreshes its rows.
 */
#define RH_ADAM_MAX_RING 1024
#define RH_SWEEP_WINDOW 0
#define RH_SWEEP_FLUSH 1
#define RH_SWEEP_LAZY_TABLES 2
#define RH_SWEEP_DENSE_TABLES 3
/* A one-lane launch that occupies `stream` for RH_TUNE_SWEEP_STAGGER_NS: placed in front of a deferred sweep whose release
 * coincides with a kernel launch of the step's chain, so that the two are not dispatched together (csrc/optim.hip). */
int rh_adam_sweep_stagger(void* stream);
/* The sweep's release by device words instead of an event.  gate: RH_GATE_WORDS int64, zero-initialised by the caller:
 * [0] count of openings, [1] wall clock of the last one, [2] count of chain starts (rh_linear_fwd_gate), [4 + 2 (i & 3)],
 * [5 + 2 (i & 3)] chain-start count and wall clock at opening i.  rh_adam_sweep_gate_open: a one-lane launch that counts an
 * opening -- captured as the last launch of a step's hipGraph it announces on every replay that the step has finished.
 * rh_adam_sweep_gate occupies `stream` until the count has reached `expected` AND a chain start has been counted since that
 * opening (the next step's first own GEMM has placed its workgroups) -- or, failing that, fallback_ns (0: RH_TUNE_SWEEP_GATE_NS)
 * have passed since the opening (round 4: that hold-back WAS the release; it still is for graphs that count no chain start).  A gate not opened within 2 s gives up and sets bit
 * RH_ERR_GATE_TIMEOUT of *err_flag (the error word of rh_embed_fwd). */
#define RH_GATE_WORDS 16
#define RH_ERR_GATE_TIMEOUT 64
int rh_adam_sweep_gate(const int64_t* gate, int64_t expected, int64_t fallback_ns, int32_t* err_flag, void* stream);
/* rh_adam_sweep_gate that first stores done_value into *done_host -- the DEVICE address (rh_host_device_pointer) of a word of
 * pinned, mapped host memory: by stream order "everything enqueued on `stream` before this launch has completed", i.e. the
 * caller's count of finished deferred sweeps, readable by the host without an event record between the sweeps (round 6). */
int rh_adam_sweep_gate_done(const int64_t* gate, int64_t expected, int64_t fallback_ns, int32_t* err_flag, int64_t* done_host,
                            int64_t done_value, void* stream);
int rh_host_device_pointer(void* host, void** device);
int rh_adam_sweep_gate_open(int64_t* gate, void* stream);
/* Releases a deferred sweep that rh_adam_sweep_gate holds back for the NEXT step's chain start when the host knows that no
 * further step follows the ones it has enqueued (end of an epoch, a synchronisation): counts one chain start in gate[2], so the
 * sweep starts at once instead of after its fallback (round 6; enqueue on the stream the step's graph was launched on). */
int rh_adam_sweep_release(int64_t* gate, void* stream);
int rh_adam_lazy_touched(const int64_t* ldesc, int T, const int64_t* field_table, const int64_t* idesc,
                         int idx_is_i64, int B, int F, int D, const double* hyper, const float* ring,
                         int ring_size, int samples_per_block, int refresh, int32_t* err_flag, void* stream);
/* n <= 4 rh_adam_lazy_touched passes over ONE table group as one launch (round 6): the refreshes in front of the first gather of a
 * step with several gathers (two-tower / sequence models: user, item, history lookups; reference: one nn.Embedding call each,
 * basic/layers.py:83-99), or the touched-rows steps at its end.  field_table / idesc: HOST arrays of n device pointers;
 * idx_is_i64, B, F: host arrays of n entries. */
int rh_adam_lazy_touched_group(const int64_t* ldesc, int T, int n, const int64_t* const* field_table, const int64_t* const* idesc,
                               const int* idx_is_i64, const int* B, const int* F, int D, const double* hyper, const float* ring,
                               int ring_size, int samples_per_block, int refresh, int32_t* err_flag, void* stream);
/* rh_adam_lazy_touched, refresh argument: 0 = the touched-rows step (rows take their gradient); 1 = pre-gather refresh of
 * every row of the batch (no gradient traffic). */
/* rh_batch_gather + rh_adam_lazy_touched (refresh = 1, int64 indices) as ONE launch (round 4): the batch is assembled into the
 * static buffers (sparse_out (B, Fd), dense_out (B, ND), label_out (B)) from dataset rows perm[(pos + b) mod N] -- exactly
 * rh_batch_gather's arguments -- while the refresh part reads the same indices straight from the dataset.  idesc must
 * describe index columns INSIDE sparse_out (pointer = sparse_out + column, stride = Fd): the gather that follows reads them.
 * lookahead != 0: further workgroups also refresh those lookups of the NEXT batch (dataset rows perm[(pos + B + b) mod N],
 * b < B) whose table rows lie in the window ((t - 1) mod K) * w .. + w of the coming deferred sweep (t = hyper[12]): that sweep
 * then skips every row the next batch reads, so the next call of this function may run while it is still in flight. */
int rh_adam_lazy_refresh_assemble(const int64_t* ldesc, int T, const int64_t* field_table, const int64_t* idesc, int B, int F,
                                  int D, const double* hyper, const float* ring, int ring_size, int samples_per_block,
                                  int32_t* err_flag, const int64_t* perm, const int64_t* pos, int64_t N, const int64_t* sparse,
                                  int Fd, const float* dense, int ND, const float* label, int64_t* sparse_out, float* dense_out,
                                  float* label_out, int lookahead, void* stream);
/* The end of step t and the head of step t + 1 as ONE launch (round 4): rh_adam_lazy_step_mode(RH_SWEEP_DENSE_TABLES) of the
 * batch just trained on + rh_adam_lazy_refresh_assemble of the NEXT batch (arguments as there; B is the size of both; *pos
 * must already point at the next batch, i.e. the step's scalar launch has advanced it -- the finished batch is read back
 * from dataset positions pos - B ..; look_depth = batches after the next one whose lookups inside the coming deferred sweep's
 * window are refreshed too, 0..4).  Every part claims a row with atomicMax on its last-step word and the claimant applies the
 * row's gradient, so a row both batches look up is stepped exactly once.  The caller's hipGraph of a step then starts with
 * the gather; optim.TableAdam ("step ahead") keeps the bookkeeping. */
int rh_adam_lazy_step_ahead(const int64_t* ldesc, int T, const int64_t* h_rows, const int64_t* h_window, int D,
                            const double* hyper, const float* ring, int ring_size, const int64_t* field_table,
                            const int64_t* idesc, int B, int F, int32_t* err_flag, const int64_t* perm, const int64_t* pos,
                            int64_t N, const int64_t* sparse, int Fd, const float* dense, int ND, const float* label,
                            int64_t* sparse_out, float* dense_out, float* label_out, int look_depth, void* stream);
/* rh_adam_lazy_step_ahead whose touched-rows part walks touched_B rows of ANOTHER int64 index matrix (touched_idesc: F column
 * pointers, then F strides) instead of the batch before the one it assembles: the GATHERED lookups of every rank's batch under
 * data parallelism with replicated tables (round 6; reference: nn.DataParallel applies the global batch's update on every
 * replica, trainers/ctr_trainer.py:53-55, optimizer.step() :99).  The refresh / assembly / look-ahead parts work on the LOCAL
 * batch as before; a row both index sets hold is claimed by one of the two passes, as in rh_adam_lazy_step_ahead. */
int rh_adam_lazy_step_ahead_touched(const int64_t* ldesc, int T, const int64_t* h_rows, const int64_t* h_window, int D,
                                    const double* hyper, const float* ring, int ring_size, const int64_t* field_table,
                                    const int64_t* idesc, int B, int F, int32_t* err_flag, const int64_t* perm,
                                    const int64_t* pos, int64_t N, const int64_t* sparse, int Fd, const float* dense, int ND,
                                    const float* label, int64_t* sparse_out, float* dense_out, float* label_out, int look_depth,
                                    const int64_t* touched_idesc, int touched_B, void* stream);
/* rh_adam_lazy_step_ahead whose launch ALSO carries the weight gradients of the step's nn.Linear layers (round 6; reference:
 * the Linear backward inside loss.backward(), trainers/ctr_trainer.py:98, dW = g^T x of basic/layers.py:279,290): wn <= 8
 * problems, arrays of wn host entries as rh_linear_wgrad_partial_group (problem i writes its split slabs to wpartial[i],
 * rh_linear_wgrad_workspace floats, for rh_pack_grads).  Nothing between the last input-gradient GEMM of the backward and
 * the packing launch behind the optimizer reads those slabs, so they leave the step's critical chain: their MFMA workgroups
 * run beside the replay arithmetic of the optimizer's parts.  Same workgroup body and split plan as the grouped launch --
 * the same slabs bit for bit. */
int rh_adam_lazy_step_ahead_wgrad(const int64_t* ldesc, int T, const int64_t* h_rows, const int64_t* h_window, int D,
                                  const double* hyper, const float* ring, int ring_size, const int64_t* field_table,
                                  const int64_t* idesc, int B, int F, int32_t* err_flag, const int64_t* perm, const int64_t* pos,
                                  int64_t N, const int64_t* sparse, int Fd, const float* dense, int ND, const float* label,
                                  int64_t* sparse_out, float* dense_out, float* label_out, int look_depth, int wn,
                                  const float* const* wg, const int64_t* wldg, const float* const* wx, const int64_t* wldx,
                                  const int* wB, const int* wN, const int* wK, float* const* wpartial, void* stream);
/* rh_adam_lazy_touched (refresh = 0, int64 indices) + rh_adam_lazy_sweep (RH_SWEEP_WINDOW) of the same step as ONE launch:
 * both parts claim a lazy row with atomicMax on its last-step word and the claimant applies the row's gradient. */
int rh_adam_lazy_step(const int64_t* ldesc, int T, const int64_t* h_rows, const int64_t* h_window, int D,
                      const double* hyper, const float* ring, int ring_size, const int64_t* field_table,
                      const int64_t* idesc, int B, int F, int samples_per_block, int32_t* err_flag, void* stream);
/* rh_adam_lazy_step with the sweep part restricted as rh_adam_lazy_sweep's `mode` (RH_SWEEP_WINDOW or RH_SWEEP_DENSE_TABLES:
 * touched rows + the dense K = 1 tables only, for a step whose lazy-table window sweep is deferred to a side stream). */
int rh_adam_lazy_step_mode(const int64_t* ldesc, int T, const int64_t* h_rows, const int64_t* h_window, int D,
                           const double* hyper, const float* ring, int ring_size, const int64_t* field_table,
                           const int64_t* idesc, int B, int F, int samples_per_block, int32_t* err_flag, int sweep_mode,
                           void* stream);
/* ... for int32 or int64 index columns (idx_is_i64 as rh_adam_lazy_touched): the row-sharded step's localised indices are int32
 * (round 6: its touched-rows step and the dense tables' step as one launch). */
int rh_adam_lazy_step_mode_idx(const int64_t* ldesc, int T, const int64_t* h_rows, const int64_t* h_window, int D,
                               const double* hyper, const float* ring, int ring_size, const int64_t* field_table,
                               const int64_t* idesc, int idx_is_i64, int B, int F, int samples_per_block, int32_t* err_flag,
                               int sweep_mode, void* stream);
int rh_adam_lazy_sweep(const int64_t* ldesc, int T, const int64_t* h_rows, const int64_t* h_window, int D,
                       const double* hyper, const float* ring, int ring_size, int mode, int64_t t_value, void* stream);
/* The launch plan of a window sweep, from the function rh_adam_lazy_sweep and the merged rh_adam_lazy_step* launches take their
 * grid from (host arrays and HOST outputs, nothing is launched).  touch_blocks = touched-rows workgroups of a merged launch
 * (64-sample chunks x fields; mode RH_SWEEP_WINDOW or RH_SWEEP_DENSE_TABLES, t_value < 0), 0 = a plain rh_adam_lazy_sweep.
 * *total_vblocks = work units (256 / (D / 4) rows each; twice that when *wide), *grid = sweep workgroups after the cap
 * (RH_TUNE_SWEEP_GRID, RH_TUNE_DEFERRED_GRID for a sweep by value; a merged launch adds touch_blocks to them; 0 = no launch),
 * *touch_period = every how-many-th workgroup of a merged launch is a touched-rows one, *wide = the two-float4-per-lane kernel
 * of the deferred sweep is taken. */
int rh_adam_lazy_sweep_plan(int T, const int64_t* h_rows, const int64_t* h_window, int D, int mode, int64_t t_value,
                            int touch_blocks, int64_t* total_vblocks, int* grid, int* touch_period, int* wide);

/* ---------------------------------------------------------------------------------------------
 * Device-resident minibatch assembly (columnar dataset already in HBM)
 * replaces: TorchDataset.__getitem__ + default_collate  torch_rechub/utils/data.py:14-25,61-83
 *           and the 39 host->device copies at trainers/ctr_trainer.py:84-85
 * perm (N,) int64 sample order; *pos (device int64) = first position of this batch;
 * gathers rows perm[(pos + b) % N], b < B, of sparse (N,F) int64, dense (N,ND) fp32, label (N,) fp32
 * into the static batch buffers.  rh_batch_advance sets *pos = (*pos + B) % N (separate launch so
 * that every reader of *pos has finished).
 */
int rh_batch_gather(const int64_t* perm, const int64_t* pos, int64_t N, int B, const int64_t* sparse,
                    int F, const float* dense, int ND, const float* label, int64_t* sparse_out,
                    float* dense_out, float* label_out, void* stream);
int rh_batch_advance(int64_t* pos, int64_t B, int64_t N, void* stream);

/* In-batch negative sampling: out (B, K) int64, row i = K distinct columns drawn uniformly from {0..B-1} \ {i}.
 * replaces: the per-row randperm loop of inbatch_negative_sampling, torch_rechub/utils/match.py:136-145
 * rng (device int64 [2]): seed, call counter; bump the counter after the call with rh_batch_advance(rng + 1, 1, 0). */
int rh_inbatch_sample(const int64_t* rng, int B, int K, int64_t* out, void* stream);

/* The same draw for rows [row0, row0 + B) of a (cols x cols) problem: out (B, K), row r = K distinct columns from
 * {0..cols-1} \ {row0 + r}.  The random stream is keyed by the global row, so ranks holding slices of one global batch
 * (cross-rank in-batch negatives: their item embeddings all-gathered into `cols` candidates) draw what one process
 * would draw.  rh_inbatch_sample(rng, B, K, ...) == rh_inbatch_sample_rows(rng, B, B, 0, K, ...).
 * replaces: torch_rechub/utils/match.py:136-145 on the single-device branch of match_trainer.py:118-138 */
int rh_inbatch_sample_rows(const int64_t* rng, int B, int cols, int row0, int K, int64_t* out, void* stream);

/* ---- gated recurrences of DIEN: AUGRU (interest evolving) and GRU (interest extractor) ------------------------------
 * replaces: the per-step Python loop of AUGRU.forward over AUGRU_Cell.forward, torch_rechub/models/ranking/dien.py:30-36,
 *           60-66 (6 matmuls + ~12 elementwise kernels per step and as many again under autograd); and the
 *           nn.GRU(batch_first=True) of the interest extractor, dien.py:101,138-143.
 * xw   (B, T, 3D): input halves of the three gates for every step, x_t [Wu | Wr | Wh] + [bu | br | bh] (one GEMM by
 *                  the caller)
 * attn (B, T) or null: the step's attention weight a_t (0 on padded steps); null = 1 everywhere
 * U    (D, 3D):    [Uu | Ur | Uh];   state_bias (3D) or null: added to h U (nn.GRU's bias_hh)
 * forward, h_0 = 0:  s = h U + state_bias;  u = sigmoid(xw_u + s_u), r = sigmoid(xw_r + s_r), c = tanh(xw_h + r * s_h),
 *                    h_t = (1 - a_t u) h_{t-1} + a_t u c;   h_all (B, T, D) receives every h_t.
 *   nn.GRU is this with a = 1, u = 1 - z (negate the z rows of weight_ih / weight_hh / both biases) and r, n as r, c.
 * backward: g_hall (B, T, D) = upstream gradient of every h_t (may be null: zeros);
 *           d_xw (B, T, 3D) = gradient of xw;  d_huh (B, T, D) = gradient of s_h (so that
 *           dU = [h_0 .. h_{T-1}]^T [d_xw_u | d_xw_r | d_huh] is one GEMM by the caller and d state_bias its column sum);
 *           d_attn (B, T) (may be null when attn is).
 * D in {4, 8, 16, 32} (the largest is RH_AUGRU_MAX_D); D / 4 lanes per sample, state in registers, U in LDS. */
#define RH_AUGRU_MAX_D 32
int rh_augru_fwd(const float* xw, const float* attn, const float* U, const float* state_bias, int B, int T, int D,
                 float* h_all, void* stream);
int rh_augru_bwd(const float* xw, const float* attn, const float* U, const float* state_bias, const float* h_all,
                 const float* g_hall, int B, int T, int D, float* d_xw, float* d_huh, float* d_attn, void* stream);

/* ---- field-aware FM (DeepFFM / FAT-DeepFFM) ------------------------------------------------------------------------
 * F fields (2 .. RH_FFM_MAX_F), P = F(F-1)/2 pairs in the reference's order (i outer, j > i inner), D logical width
 * (1 .. RH_FFM_MAX_D), Dp physical row width of the tables (D <= Dp <= RH_FFM_MAX_D: PaddedEmbedding).  Pair side (i, j) is row x_i * F + j of field
 * i's table.  Two row-addressing modes, one kernel each way:
 *   table mode (fdesc, idesc as above, x = null): the raw (B,) index columns of the F fields;
 *   dense mode (fdesc = idesc = null, x (B, F, F, D) with sample stride x_stride): the layer-level FFM.
 * rh_ffm_fwd: out[b, p*D + d] = row(i,j)[d] * row(j,i)[d] (one product: bit-exact), or with reduce_sum out[b, p] = the sum
 *   over d; row stride out_stride.  An index whose row falls outside [0, vocab) sets RH_FLAG_INDEX_OOB.
 * rh_ffm_bwd: g (B, P*D) or (B, P) with reduce_sum, row stride g_stride.  Table mode: g * row(j,i) float-atomically added
 *   to row (i,j) of field i's gradient buffer (fdesc[F + i]; logical columns only, rows at padding_idx dropped), or with
 *   sink = 1 written to rows (B, F(F-1), Dp) at virtual field v(i,j) = i(F-1) + (j < i ? j : j - 1), padding columns 0.
 *   Dense mode: g_x (B, F, F, D), sample stride gx_stride, every element written once (diagonal 0).
 * rh_ffm_expand_index: out (B, F(F-1)) of the index dtype = x_i * F + j at v(i,j): the lookups of the table mode as
 *   ordinary index columns (optimizer touch records, the data-parallel exchange).
 * replaces: DeepFFM.forward torch_rechub/models/ranking/deepffm.py:57-62 (x * F + fields_offset, (B, F, F, D) lookup),
 *           FFM.forward torch_rechub/basic/layers.py:736-746 and their autograd. */
#define RH_FFM_MAX_F 64
#define RH_FFM_MAX_D 128
int rh_ffm_expand_index(const int64_t* idesc, int idx_is_i64, int B, int F, void* out, void* stream);
int rh_ffm_fwd(const int64_t* fdesc, const int64_t* idesc, int idx_is_i64, const float* x, int64_t x_stride, int B, int F,
               int D, int Dp, int reduce_sum, float* out, int64_t out_stride, int32_t* err_flag, void* stream);
int rh_ffm_bwd(const int64_t* fdesc, const int64_t* idesc, int idx_is_i64, const float* x, int64_t x_stride, int B, int F,
               int D, int Dp, int reduce_sum, const float* g, int64_t g_stride, float* g_x, int64_t gx_stride, int sink,
               float* rows, int32_t* err_flag, void* stream);
/* CEN field attention on em (B, P*D), row stride ld (FAT-DeepFFM).
 * rh_cen_desc_fwd: d (B, P) = relu(sum_d u[p,d] em[b,p,d]).
 * rh_cen_desc_bwd: g_em (B, P*D) contiguous = relu'(d) g_d u; u_partial (rh_cen_nchunks(B), P*D) per-chunk sums of
 *   relu'(d) g_d em over consecutive samples in a fixed order (g_u = rh_colsum of it: bitwise reproducible).
 * rh_cen_rescale_fwd: out (B, P*D) contiguous = s[b,p] em[b,p,:].
 * rh_cen_rescale_bwd: g_em (B, P*D) contiguous = s g; g_s (B, P) = sum_d g em.  g row stride ldg.
 * replaces: CEN.forward torch_rechub/basic/layers.py:777-786 (the attention MLP between d and s stays an MLP). */
int rh_cen_nchunks(int B);
int rh_cen_desc_fwd(const float* em, int64_t ld, const float* u, int B, int P, int D, float* d_out, void* stream);
int rh_cen_desc_bwd(const float* em, int64_t ld, const float* u, const float* d, const float* g_d, int B, int P, int D,
                    float* g_em, float* u_partial, void* stream);
int rh_cen_rescale_fwd(const float* em, int64_t ld, const float* s, int B, int P, int D, float* out, void* stream);
int rh_cen_rescale_bwd(const float* em, int64_t ld, const float* s, const float* g, int64_t ldg, int B, int P, int D,
                       float* g_em, float* g_s, void* stream);

/* ---- multi-interest user towers and list-wise scoring (YoutubeDNN / MIND / ComiRec) ----------------------------------
 * Capsule routing (CapsuleNetwork, bilinear types 0 / 1 / 2), B samples, L positions, I interests, width D (D <= RH_CAPSULE_MAX_D,
 * I*D <= RH_CAPSULE_MAX_ID; type 2 also I*D*D <= RH_CAPSULE_MAX_IDD).  mask (B, L) int32, nonzero = kept.  Types 0 / 1: U (B, L, Iu*D) the Linear's
 * output (Iu = 1 / I; type 0 repeats it over the interests); type 2: E (B, L, D) and W (L, I*D, D) (w[0, :L]).
 * init (B, I, L) the initial routing logits, or null for zeros.  Writes cap (B, I, D), and when not null the last
 * iteration's masked softmax weights sw (B, I, L) and pre-squash sums s (B, I, D) for the backward.
 * rh_capsule_bwd (through the last iteration only): types 0 / 1: g_u (B, L, Iu*D); type 2: g_e (B, L, D) and g_s (B, I, D).
 * rh_capsule_wgrad (type 2): partial (rh_capsule_wgrad_nchunks(B), L*I*D*D) per-chunk sums of the weight gradient in a
 *   fixed order (g_w = rh_colsum of it: bitwise reproducible).
 * replaces: CapsuleNetwork.forward torch_rechub/basic/layers.py:657-712 and its autograd. */
#define RH_CAPSULE_MAX_D 64
#define RH_CAPSULE_MAX_ID 256
#define RH_CAPSULE_MAX_IDD 4096
int rh_capsule_supported(int L, int I, int D, int type);
int rh_capsule_fwd(const float* U, const float* E, const float* W, const int32_t* mask, const float* init, int B, int L,
                   int I, int D, int type, int routing_times, float* cap, float* sw, float* s, void* stream);
int rh_capsule_bwd(const float* g_cap, const float* s, const float* sw, const float* W, int B, int L, int I, int D, int type,
                   float* g_u, float* g_e, float* g_s, void* stream);
int rh_capsule_wgrad_nchunks(int B);
int rh_capsule_wgrad(const float* g_s, const float* sw, const float* E, int B, int L, int I, int D, float* partial,
                     void* stream);
/* Self-attentive pooling (MultiInterestSA after A = tanh(E W1) W2): A (B, L, I), E (B, L, D), mask (B, L) int32 or null.
 * rh_sa_pool_fwd: P (B, L, I) = softmax over L of A + -1e9 (1 - mask); out (B, I, D) = P^T E.
 * rh_sa_pool_bwd: g (B, I, D) -> gA (B, L, I), gE (B, L, D).  D <= RH_SA_MAX_D, L*I <= RH_SA_MAX_LI, I*D <= RH_SA_MAX_ID.
 * replaces: MultiInterestSA.forward torch_rechub/basic/layers.py:601-609 (softmax, mask term, matmul) and its autograd. */
#define RH_SA_MAX_D 64
#define RH_SA_MAX_LI 1024
#define RH_SA_MAX_ID 1024
int rh_sa_supported(int L, int I, int D);
int rh_sa_pool_fwd(const float* A, const float* E, const int32_t* mask, int B, int L, int I, int D, float* P, float* out,
                   void* stream);
int rh_sa_pool_bwd(const float* P, const float* E, const float* g, int B, int L, int I, int D, float* gA, float* gE,
                   void* stream);
/* List-wise scoring: u (B, I, D) normalised user vectors (I <= RH_LISTWISE_MAX_I, D <= RH_LISTWISE_MAX_D), pos (B, D) row stride
 * ldp and neg (B, K, D) raw item rows (K <= RH_LISTWISE_MAX_K).  Rows are L2-normalised (F.normalize, eps 1e-12); best[b] = first argmax_i u_i . pos_hat;
 * logits (B, 1 + K) = u_best . [pos_hat, neg_hat] / temperature; nrm (B, 1 + K) the row norms for the backward.
 * rh_listwise_bwd: g (B, 1 + K) -> g_u (B, I, D) (zero but the chosen interest), g_pos (B, D), g_neg (B, K, D).
 * replaces: the item towers' F.normalize + torch.cat and the bmm / argmax / gather / mul-sum of YoutubeDNN, MIND,
 *           ComirecDR and ComirecSA.forward (torch_rechub/models/matching/youtube_dnn.py, mind.py, comirec.py). */
#define RH_LISTWISE_MAX_I 16
#define RH_LISTWISE_MAX_D 64
#define RH_LISTWISE_MAX_K 1023
int rh_listwise_fwd(const float* u, const float* pos, int64_t ldp, const float* neg, int B, int I, int D, int K,
                    float temperature, float* logits, int32_t* best, float* nrm, void* stream);
int rh_listwise_bwd(const float* u, const float* pos, int64_t ldp, const float* neg, const int32_t* best, const float* nrm,
                    const float* g, int B, int I, int D, int K, float temperature, float* g_u, float* g_pos, float* g_neg,
                    void* stream);

/* ---- SINE sparse-interest retrieval (csrc/sine.hip) ------------------------------------------------------------------
 * B samples, S = seq_max_len positions, width E, T concept prototypes, K intentions, one attention head.
 * 1 <= S <= RH_SINE_MAX_S, 1 <= E <= RH_SINE_MAX_E, 1 <= T <= RH_SINE_MAX_T, 1 <= K <= min(T, RH_SINE_MAX_K), else RH_E_UNSUPPORTED; B = 0 returns at once.
 * rh_sine_supported and rh_sine_nchunks answer through a HOST int (*supported = 0 / 1, *nchunks = the chunk count of a batch
 * of B) and return a status like every entry point that takes a pointer.  mask (B, S) int32, 1 = kept, any pattern; every softmax over S is of a + -1e9 (1 - mask) formed in
 * fp32 as the reference forms it (a fully padded row comes out uniform).  No atomics: two runs give the same bits.
 *
 * rh_sine_interest_fwd: X (B, S, E) = x_u, Y (B, S, E) = X w_3, a1 (B, S) = tanh(X w_1) w_2, a2 (B, S, K) =
 *   tanh(X w_k1) w_k2, C (T, E) the concept table.  Per sample: P1 = softmax_S(a1); z_u = P1^T X; s_u = z_u C^T; idx (B, K)
 *   = the K largest of s_u in descending order, ties to the lower index (torch.topk); c_u[k] = sigmoid(s_u[idx[k]])
 *   C[idx[k]]; PU[:, s] = softmax_k(normalize(Y[s]) . normalize(c_u[k])) (F.normalize, eps 1e-12); P2[k] =
 *   softmax_S(a2[:, k]); phi (B, K, E)[k] = sum_s PU[k, s] P2[k, s] X[s]; xhat (B, S, E)[s] = sum_k PU[k, s] c_u[k].
 *   Saves P1 (B, S), P2 (B, K, S) and PU (B, K, S) for the backward, which recomputes the rest.
 * rh_sine_interest_bwd: g_phi (B, K, E), g_xhat (B, S, E) -> g_X, g_Y (B, S, E), g_a1 (B, S), g_a2 (B, S, K).  The top-k
 *   passes gradient to the chosen scores only (through the gate and through s_u = z_u . C[idx] to z_u and C).  g_crow
 *   (B, K, E) is a workspace (the per-sample rows of the table's gradient); c_partial (rh_sine_nchunks(B), T*E) the
 *   per-chunk sums of those rows over consecutive samples in a fixed order (g_C = rh_colsum of it).
 * replaces: SINE.user_tower torch_rechub/models/matching/sine.py:94-118 (the softmaxes, einsums, topk, sigmoid gate,
 *           concept gather and F.normalize calls between the w_1 / w_k1 / w_3 products and h_3) and their autograd.
 *
 * rh_sine_aggregate_fwd: xhat (B, S, E), a3 (B, S) = tanh(xhat w_4) w_5, phi (B, K, E).  P3 = softmax_S(a3); m (B, E) =
 *   P3^T xhat; c_apt = m / max(|m|_p, 1e-12) with p = -1, |m|_p = 1 / sum_e 1 / |m_e| (sine.py:122 passes -1 as the ORDER
 *   of F.normalize, not as its axis); e (B, K) = softmax_k(c_apt . phi[k] * inv_temperature); v (B, E) = sum_k e[k] phi[k].
 *   |m|_p is about the smallest |m_e| and ill-conditioned in fp32: both kernels compute in fp64 inside and round their
 *   outputs once; the backward recomputes the chain from the inputs, nothing is saved.
 * rh_sine_aggregate_bwd: g_v (B, E) -> g_xhat (B, S, E), g_a3 (B, S), g_phi (B, K, E) (through e and directly).
 * replaces: sine.py:122-128 after h_3 w_5 (softmax, mask term, einsum, F.normalize, softmax over k, einsum) and their
 *           autograd. */
#define RH_SINE_MAX_S 64
#define RH_SINE_MAX_E 128
#define RH_SINE_MAX_T 64
#define RH_SINE_MAX_K 8
int rh_sine_supported(int S, int E, int T, int K, int* supported);
int rh_sine_nchunks(int B, int* nchunks);
int rh_sine_interest_fwd(const float* X, const float* Y, const float* a1, const float* a2, const int32_t* mask,
                         const float* C, int B, int S, int E, int T, int K, int32_t* idx, float* phi, float* xhat, float* P1,
                         float* P2, float* PU, void* stream);
int rh_sine_interest_bwd(const float* X, const float* Y, const float* C, const int32_t* idx, const float* P1, const float* P2,
                         const float* PU, const float* g_phi, const float* g_xhat, int B, int S, int E, int T, int K,
                         float* g_X, float* g_Y, float* g_a1, float* g_a2, float* g_crow, float* c_partial, void* stream);
int rh_sine_aggregate_fwd(const float* xhat, const float* a3, const int32_t* mask, const float* phi, float inv_temperature,
                          int B, int S, int E, int K, float* v, void* stream);
int rh_sine_aggregate_bwd(const float* xhat, const float* a3, const int32_t* mask, const float* phi, const float* g_v,
                          float inv_temperature, int B, int S, int E, int K, float* g_xhat, float* g_a3, float* g_phi,
                          void* stream);

/* ---- RQ-VAE residual quantizer (csrc/rq.hip) -----------------------------------------------------------------------------
 * Rows (N, E) fp32, L codebooks C_l (n_e[l], E).  C: HOST array of L device pointers, n_e: HOST array of L sizes (as
 * rh_cross_moe_pack takes its arrays).  1 <= E <= RH_RQ_MAX_E, 1 <= n_e[l] <= RH_RQ_MAX_CODES, 1 <= L <= RH_RQ_MAX_L, else RH_E_UNSUPPORTED; N = 0
 * returns at once.  rh_rq_supported and rh_rq_nchunks answer through HOST ints (*supported = 0 / 1; *fwd_blocks = the rows
 * of sse_partial, *bwd_chunks = the rows of c_partial for N rows) and return a status like every entry point that takes a
 * pointer.  No atomics: two runs give the same bits.
 *
 * rh_rq_fwd: the levels [l0, l1) on r_in (N, E), the residual entering level l0 (x when l0 = 0).  Per level l:
 *   idx[:, l] = argmin_k sum_e (r - C_l[k])^2 (direct form; an exact tie goes to the lower index, as torch.argmin), unless
 *   bit l of `given` is set: then idx[:, l] is read, not searched (clamped into [0, n_e[l])); r <- r - C_l[idx[:, l]];
 *   sse[l] = sum over rows and columns of (C_l[idx] - r_l)^2, through sse_partial (fwd_blocks, l1 - l0) summed in a fixed
 *   order.  idx (N, L) int32 (only the columns of the range are touched), r_out (N, E) the residual after level l1 - 1,
 *   x_q (N, E) = r_in - r_out.  sse (L,): only the entries of the range are written.  No (N, n_e) array is formed.
 *   The level's loss is (1 + beta) sse[l] / (N E) = codebook_loss + beta commitment_loss in value.
 * rh_rq_bwd: all L levels, from x (N, E), idx (N, L), g_xq (N, E) and the DEVICE scalar g_loss (gradient of the mean over
 *   levels of the level losses); s = g_loss 2 / (L N E):
 *   g_x (N, E) = g_xq + s beta (x - C_0[idx_0])   (the commitment terms of the levels >= 1 cancel: d r_{l+1} / d r_l = I - I
 *   through the straight-through estimator); g_C (sum_l n_e[l] E,) = the L tables' gradients one after the other,
 *   g_C_l[k] = s sum over rows with idx_l = k of (C_l[k] - r_l), the residuals recomputed from x and idx; rows of a table
 *   that no row chose get exactly 0.  c_partial (bwd_chunks, sum_l n_e[l] E): per-chunk sums over consecutive rows in row
 *   order, every element written, added by rh_colsum's kernel.
 * replaces: VectorQuantizer.forward torch_rechub/models/generative/rqvae.py:241-274 (distance matrix, argmin, embedding
 *           gather, the two mse_loss calls, the straight-through sum) and ResidualVectorQuantizer.forward :382-398 (the
 *           residual updates, the stacks and the mean), and their autograd. */
#define RH_RQ_MAX_E 128
#define RH_RQ_MAX_CODES 1024
#define RH_RQ_MAX_L 8
int rh_rq_supported(int E, int L, const int* n_e, int* supported);
int rh_rq_nchunks(int N, int* fwd_blocks, int* bwd_chunks);
int rh_rq_fwd(const float* r_in, const float* const* C, const int* n_e, int N, int E, int L, int l0, int l1, int given,
              int32_t* idx, float* r_out, float* x_q, float* sse_partial, float* sse, void* stream);
int rh_rq_bwd(const float* x, const float* const* C, const int* n_e, const int32_t* idx, const float* g_xq,
              const float* g_loss, float beta, int N, int E, int L, float* g_x, float* c_partial, float* g_C, void* stream);

/* ---- HSTU generative model: pointwise relative-bias attention (csrc/hstu.hip) and the next-token head ---------------
 * Attention of one HSTULayer on proj (B, L, ld) = silu(proj1(LN(x))) (row stride ld >= 2 H (dqk + dv)): per head h,
 * q at columns h dqk, k at H dqk + h dqk, v at 2 H dqk + H dv + h dv.  td (B, L) int64 seconds or null (position-only
 * bias), kmask (B, L) int32 nonzero = kept key or null.  pos_w (2 N - 1, H), ts_w (nb + 1, H) contiguous; N = max_seq_len,
 * nb = num_time_buckets, fn_log 0 sqrt / 1 log, minutes 0 / 1, alpha = 1 / sqrt(dqk).
 * rh_hstu_attn_fwd: out (B, L, H dv) = (silu(alpha q k^T + pos + ts) / N, masked to 0 above the diagonal and at dropped
 *   keys) v.  1 <= L <= min(N, RH_HSTU_MAX_L), dqk, dv <= RH_HSTU_MAX_DH, nb <= RH_HSTU_MAX_BUCKETS, else RH_E_UNSUPPORTED.
 * rh_hstu_attn_bwd: g_out (B, L, H dv) -> the q / k / v columns of g_proj (B, L, ld) (the other columns are not
 *   written), g_pos_w (2 N - 1, H) and g_ts_w (nb + 1, H), through per-workgroup partials pos_part
 *   (rh_hstu_attn_nparts(B, L, H), L) and ts_part (same rows, nb + 1; may be null when td is) summed in a fixed order.
 *   No atomics: bitwise reproducible.
 * replaces: HSTULayer.forward torch_rechub/basic/layers.py:916-933 (matmul, rab, tril, masked_fill, silu, /N, matmul) with
 *           RelativeBucketedTimeAndPositionBias.forward utils/hstu_utils.py:150-185, and their autograd. */
#define RH_HSTU_MAX_L 1024
#define RH_HSTU_MAX_DH 64
#define RH_HSTU_MAX_BUCKETS 1023
int rh_hstu_attn_nparts(int B, int L, int H);
int rh_hstu_attn_fwd(const float* proj, int64_t ld, int B, int L, int H, int dqk, int dv, const int64_t* td,
                     const int32_t* kmask, const float* pos_w, const float* ts_w, int N, int nb, int fn_log, int minutes,
                     float divisor, float alpha, float* out, void* stream);
int rh_hstu_attn_bwd(const float* proj, int64_t ld, int B, int L, int H, int dqk, int dv, const int64_t* td,
                     const int32_t* kmask, const float* pos_w, const float* ts_w, int N, int nb, int fn_log, int minutes,
                     float divisor, float alpha, const float* g_out, float* g_proj, float* pos_part, float* ts_part,
                     float* g_pos_w, float* g_ts_w, void* stream);
/* Next-token cross entropy over the item table (csrc/stream_ce.hip): h (M, D), W (V, D), bias (V,) or null, labels
 * (M,) int64 (0 = ignored, else in [1, V)).  z = ((h W^T + bias) / t1) / t2, column 0 excluded from the normaliser;
 * loss (1,) = mean over rows with a label of lse - z[label] (NaN when there is none; nce = 1: then the mean over every
 * row of lse + 1e9 / t2).
 * rh_hstu_head_fwd: part (M, rh_hstu_head_nsplit(M, V), 2) workspace; zlab, lse, wrow (M,) for the backward; a label
 *   outside [0, V) ORs RH_FLAG_TARGET_OOB into *err (when not null) and its row's loss is undefined.
 * rh_hstu_head_bwd: g_loss (1,) device scalar -> g_h (M, D), g_W (V, D), g_bias (V,) (null: not wanted); part
 *   (rh_hstu_head_rsplit(M, D, V), V, D + 1) workspace, unused when that count is 1.  Logits recomputed tile by tile;
 *   no atomics.  M >= 1, V >= 2, any D.  g_W null (a frozen table: then g_bias must be null too): only g_h is
 *   computed, no dW kernel runs and part is not read (may be null).
 * replaces: HSTUModel.forward's F.linear / temperature (models/generative/hstu.py:266-271), SeqTrainer's logits.clone()
 *           and CrossEntropyLoss / NCELoss (trainers/seq_trainer.py:177-194, basic/loss_func.py:141-175), and autograd. */
int rh_hstu_head_nsplit(int M, int V);
int rh_hstu_head_rsplit(int M, int D, int V);
int rh_hstu_head_fwd(const float* h, const float* W, const float* bias, const int64_t* labels, int M, int D, int V, float t1,
                     float t2, int nce, float* part, float* zlab, float* lse, float* wrow, float* loss, int32_t* err,
                     void* stream);
int rh_hstu_head_bwd(const float* h, const float* W, const float* bias, const int64_t* labels, const float* lse,
                     const float* wrow, const float* g_loss, int M, int D, int V, float t1, float t2, float* part, float* g_h,
                     float* g_W, float* g_bias, void* stream);

/* ---- HLLM: causal softmax multi-head attention with a bucketed relative-position bias and dropout -------------------
 * q, k, v: (B, L, H, dh) views sharing the row stride ld >= H dh (three separate (B L, H dh) projections with ld = H dh,
 * or three column blocks of one (B L, 3 H dh) product with ld = 3 H dh).  bias (nb, H) contiguous or null;
 * bucket(i, j) = min(|i - j|, N) * (nb - 1) / N in integers (N = max_seq_len), formed in the kernel.  Causal (j <= i),
 * no padding mask.  p_drop in [0, 1): dropout on the weights with the counter hash over element ((b H + h) L + i) L + j;
 * rng = the device (seed, counter) pair, saved_ctr (1,) receives the counter this call used; p_drop = 0: both may be
 * null and no hash is computed.
 * rh_softmax_attn_fwd: out (B, L, H dh) = dropout(softmax_j(scale q_i . k_j + bias)) v; lse (B, H, L) the rows'
 *   log-sum-exp for the backward.  The forward advances the counter on the device.
 * rh_softmax_attn_bwd: g_out (B, L, H dh) -> g_q, g_k, g_v ((B, L, H, dh) views, row stride ldg), g_bias (nb, H) when
 *   bias is given, through part (rh_softmax_attn_nparts(B, L, H), L) per-workgroup partials summed in a fixed order;
 *   delta (B, H, L) workspace.  Weights recomputed tile by tile; nothing of size L x L is written.  No atomics.
 * 1 <= L <= min(N, RH_ATTN_MAX_L), 1 <= dh <= RH_ATTN_MAX_DH (both shared with rh_t5_attn_*), H >= 1, nb >= 1 or no bias, else RH_E_UNSUPPORTED; B = 0 returns at once.
 * replaces: HLLMTransformerBlock.forward torch_rechub/models/generative/hllm.py:69-88 (view / transpose, matmul, tril,
 *           masked_fill, bias add, softmax, dropout, matmul, transpose / contiguous) with RelPosBias.forward
 *           utils/hstu_utils.py:54-68, and their autograd. */
#define RH_ATTN_MAX_L 1024
#define RH_ATTN_MAX_DH 128
int rh_softmax_attn_nparts(int B, int L, int H);
int rh_softmax_attn_fwd(const float* q, const float* k, const float* v, int64_t ld, int B, int L, int H, int dh,
                        const float* bias, int N, int nb, float scale, float p_drop, int64_t* rng, int64_t* saved_ctr,
                        float* out, float* lse, void* stream);
int rh_softmax_attn_bwd(const float* q, const float* k, const float* v, int64_t ld, int B, int L, int H, int dh,
                        const float* bias, int N, int nb, float scale, float p_drop, const int64_t* rng,
                        const int64_t* saved_ctr, const float* out, const float* lse, const float* g_out, float* delta,
                        float* g_q, float* g_k, float* g_v, int64_t ldg, float* part, float* g_bias, void* stream);

/* Full-catalogue cross entropy (csrc/stream_ce.hip: the same head, every column and row counted, no bias / temperature):
 * u (B, D), E (V, D), labels (B,) int64 in [0, V).  loss (1,) = mean over rows of lse(u E^T) - (u E^T)[label].
 * rh_catalogue_ce_fwd: part (B, rh_hstu_head_nsplit(B, V), 2) workspace; zlab, lse, wrow (B,) for the backward; a label
 *   outside [0, V) ORs RH_FLAG_TARGET_OOB into *err (when not null) and its row's loss is undefined.
 * rh_catalogue_ce_bwd: g_loss (1,) device scalar -> g_u (B, D), dense g_E (V, D); part (rh_hstu_head_rsplit(B, D, V), V,
 *   D + 1) workspace (unused when that count is 1), part_h (rh_catalogue_ce_vsplit(B, D, V), B, D) workspace (unused when 1).
 *   B >= 1, 2 <= V <= 2^30, any D; the (B, V) logits never exist; no atomics.
 * replaces: nn.CrossEntropyLoss over NARM / STAMP's (B, V) scores (models/matching/narm.py:111, stamp.py:99 with
 *           MatchTrainer(mode=2), examples/matching/run_sbr.py), and autograd. */
int rh_catalogue_ce_vsplit(int B, int D, int V);
int rh_catalogue_ce_fwd(const float* u, const float* E, const int64_t* labels, int B, int D, int V, float* part, float* zlab,
                        float* lse, float* wrow, float* loss, int32_t* err, void* stream);
int rh_catalogue_ce_bwd(const float* u, const float* E, const int64_t* labels, const float* lse, const float* wrow,
                        const float* g_loss, int B, int D, int V, float* part, float* part_h, float* g_u, float* g_E,
                        void* stream);

/* ---- exact top-K item retrieval (csrc/topk.hip) ---------------------------------------------------------------------
 * score[i][j] = q_i . x_j (+ bias[j]) over the whole table, the K best per query, without the (M, V) score matrix.
 * q (M, D) fp32 with row stride ldq, x (V, D) fp32 contiguous, bias (V,) or null.  exclude (M, S) int64 or null (S = 0):
 * the ids of row i that may not be returned to query i; entries outside [0, V) are ignored (pad with -1; a 0-padded
 * history also drops id 0).  invalid (n_inv,) int64 or null: ids dropped for every query.
 * ids (M, K) int64 and scores (M, K) fp32, sorted by (score descending, id ascending): an exact tie goes to the lower id,
 * as torch.topk.  Excluded and invalid ids never appear; with fewer than K candidates left the tail is id -1, score -inf
 * (K > V is legal).  Inputs are assumed finite (NaN is not checked).  The products are exact f32 accumulated in k order
 * from zero on the 64 x 64 MFMA tile, the bias is added last: one score depends on q_i, x_j and D only -- not on M, V,
 * the position in a tile or the split.  nsplit ranges [V s / nsplit, V (s + 1) / nsplit) are scanned by separate
 * workgroups and merged under the same total order: every nsplit in [1, min(V, RH_TOPK_MAX_SPLIT)] gives the same bits.  No atomics.
 * 1 <= D <= RH_TOPK_MAX_D, 1 <= K <= RH_TOPK_MAX_K, 0 <= S <= RH_TOPK_MAX_S, 1 <= V < 2^31, any M, else RH_E_UNSUPPORTED; M = 0 returns at once.
 * rh_topk_supported and rh_topk_plan answer through HOST pointers (*supported = 0 / 1; *nsplit = the default split,
 * *workspace_bytes = 8 M nsplit K for it -- a caller that passes another nsplit sizes the workspace by the same formula)
 * and return a status like every entry point that takes a pointer.
 * replaces: Annoy.fit / Annoy.query of examples/matching/movielens_utils.py:17-42, torch.topk over the (B, V) scores of
 *           examples/matching/run_sbr.py:53 and the masked torch.topk of examples/generative/run_hstu_movielens.py:109-114,
 *           the builders of torch_rechub/serving (annoy, faiss, milvus). */
#define RH_TOPK_MAX_D 1024
#define RH_TOPK_MAX_K 256
#define RH_TOPK_MAX_S 1024
#define RH_TOPK_MAX_SPLIT 1024
int rh_topk_supported(int D, int K, int S, int* supported);
int rh_topk_plan(int M, int V, int K, int* nsplit, int64_t* workspace_bytes);
int rh_topk_fwd(const float* q, int64_t ldq, const float* x, const float* bias, const int64_t* exclude, int S,
                const int64_t* invalid, int n_inv, int M, int D, int V, int K, int nsplit, void* workspace, int64_t* ids,
                float* scores, void* stream);

/* ---- inverted-file index (csrc/ivf.hip) ------------------------------------------------------------------------------
 * The top K of rh_topk_fwd's score over the UNION of the lists a query probes, without a host synchronisation.
 * xs (V, D) fp32 contiguous: the table with its rows grouped by list; bias_s (V,) or null, grouped alike; row_id (V,)
 * int32: the original id of every grouped row, ASCENDING inside each list; list_off (nlists + 1,) int32: list l is the rows
 * [list_off[l], list_off[l + 1]).  q (M, D) fp32 with row stride ldq.  exclude (M, S) int64 or null (S = 0): ORIGINAL ids
 * that may not be returned to query i (others are padding).
 * The (query, slot) pairs of probe (M, nprobe) arrive grouped by list, computed by the caller on the device: group 0 =
 * the pairs whose slot holds no list (-1), group l + 1 = the pairs that probe list l (the lists of one query are distinct);
 * pair (M nprobe,) int32 = the pair indices i nprobe + slot in group order (a permutation), pair_off (nlists + 2,) int32 =
 * the groups' offsets into it, tile_off (nlists + 2,) int32 = the prefix sum of ceil(group size / rows_per_tile).
 * One workgroup takes rows_per_tile pairs of one group and walks the WHOLE list (an over-long list is not split); the grid
 * is the fixed bound ceil(M nprobe / rows_per_tile) + nlists + 1, a workgroup past tile_off's end leaves.
 * partials: 8 M nprobe K bytes, every element written.  ids (M, K) int64 = original ids and scores (M, K) fp32, sorted by
 * (score descending, id ascending); with fewer than K candidates the tail is id -1, score -inf.  A score is computed
 * exactly as rh_topk_fwd computes it (it depends on q_i, x_j and D only), so with every list probed the result equals
 * rh_topk_fwd's on the un-grouped table bit for bit.  No atomics: two runs give the same bits.
 * 1 <= D <= RH_TOPK_MAX_D, 1 <= K <= RH_TOPK_MAX_K, 0 <= S <= RH_TOPK_MAX_S, 1 <= nprobe <= RH_IVF_MAX_NPROBE, 1 <= V < 2^31, else
 * RH_E_UNSUPPORTED; M = 0 returns
 * at once.  rh_ivf_supported and rh_ivf_plan answer through HOST pointers: *supported = 0 / 1; *rows_per_tile = 64 up to
 * K = 128, 32 above; *grid = the bound above; *workspace_bytes = 8 M nprobe K (partials) + 4 M nprobe (pair) +
 * 8 (nlists + 2) (pair_off, tile_off).
 * rh_ivf_list_mean: the update step of k-means.  centroids (nlists, D)[l] = the mean of the rows of list l of xs (V, D),
 * summed in a fixed order (bit-reproducible, no atomics) and divided once; an empty list keeps previous (nlists, D)[l].
 * replaces: FaissBuilder of torch_rechub/serving/faiss.py with index_type="IVF" (faiss's `IVF{nlists},Flat` with its
 *           k-means training, and `nprobe`). */
#define RH_IVF_MAX_NPROBE 256
int rh_ivf_supported(int D, int K, int S, int nprobe, int* supported);
int rh_ivf_plan(int M, int nlists, int nprobe, int K, int* rows_per_tile, int64_t* grid, int64_t* workspace_bytes);
int rh_ivf_scan(const float* q, int64_t ldq, const float* xs, const float* bias_s, const int32_t* row_id,
                const int32_t* list_off, int nlists, const int32_t* pair, const int32_t* pair_off, const int32_t* tile_off,
                const int64_t* exclude, int S, int M, int D, int V, int K, int nprobe, void* partials, int64_t* ids,
                float* scores, void* stream);
int rh_ivf_list_mean(const float* xs, const int32_t* list_off, const float* previous, int V, int D, int nlists,
                     float* centroids, void* stream);

/* ---- session-based retrieval (csrc/session.hip) ---------------------------------------------------------------------
 * GRU recurrence of nn.GRU (gate order r, z, n) from the zero state: xw (B, T, 3H) = x W_ih^T (+ b_ih) for every step,
 * w_hh (3H, H) = weight_hh, b_hh (3H,) or null.  1 <= H <= RH_GRU_MAX_H, else RH_E_UNSUPPORTED.
 * rh_gru_fwd: h_all (B, T, H) every state; hu (B, T, 3H) the state products h_{t-1} W_hh^T + b_hh (for the backward).
 * rh_gru_bwd: g (B, T, H) gradient of h_all -> d_xw (B, T, 3H) the input-side pre-activation gradients
 *   [r | z | n] and d_s (B, T, 3H) the state-side ones [r | z | hu_n] (weight gradients: d_s^T h_prev, d_xw^T x).
 * replaces: nn.GRU / pack_padded_sequence (models/matching/narm.py:55-57, gru4rec.py:60) and its autograd. */
#define RH_GRU_MAX_H 128
int rh_gru_fwd(const float* xw, const float* w_hh, const float* b_hh, int B, int T, int H, float* h_all, float* hu,
               void* stream);
int rh_gru_bwd(const float* xw, const float* w_hh, const float* h_all, const float* hu, const float* g, int B, int T, int H,
               float* d_xw, float* d_s, void* stream);
/* Additive attention pooling: s_l = sum_h w0_h sigmoid(P_lh + r_h), e_l = exp(s_l) mask_l, a_l = e_l / den with
 * den = sum_l e_l (floor = 0) or max(sum_l e_l, 1e-12) (floor = 1), out (B, Dx) = sum_l a_l X_l (+ add).  P (B, L, H),
 * r (B, H), w0 (H,), mask (B, L) float 0 / 1, X (B, L, Dx), add (B, Dx) or null.  1 <= L <= RH_ATTN_POOL_MAX_L, 1 <= H, Dx <= RH_ATTN_POOL_MAX_W.
 * rh_attn_pool_fwd: e (B, L), sums (B, 2) = (sum, den) for the backward.
 * rh_attn_pool_bwd: g (B, Dx) -> dP (B, L, H), dr (B, H), dw0 (H,) (per-sample partials dw0_part (B, H) summed in a
 *   fixed order; zero at B = 0), dX (B, L, Dx) the pooling term only.
 * replaces: NARM's q / alpha / c_l (models/matching/narm.py:60-63), STAMP's a / m_a (stamp.py:66-67), and autograd. */
#define RH_ATTN_POOL_MAX_L 1024
#define RH_ATTN_POOL_MAX_W 4096
int rh_attn_pool_fwd(const float* P, const float* r, const float* w0, const float* mask, const float* X, const float* add,
                     int B, int L, int H, int Dx, int floor_, float* out, float* e, float* sums, void* stream);
int rh_attn_pool_bwd(const float* P, const float* r, const float* w0, const float* X, const float* e, const float* sums,
                     const float* g, int B, int L, int H, int Dx, int floor_, float* dP, float* dr, float* dw0_part,
                     float* dw0, float* dX, void* stream);
/* Dropout (n elements, 0 < p < 1) with the counter hash of the fused MLP dropout: rng (device int64 [seed, counter, ..]);
 * the forward records the counter it used in saved_ctr and advances rng's; the backward recomputes the mask from it. */
/* counts (B,) int64 = the number of non-zero ids of each row of seq (B, L) int64; a row without any ORs
 * RH_FLAG_SESSION_EMPTY into *err, and with check_full a batch whose longest row is shorter than L ORs RH_FLAG_SESSION_SHORT.
 * replaces: value_mask.sum(1).to("cpu") and the errors of pack_padded_sequence / NARM's broadcast (narm.py:50-61),
 *           STAMP's gather at count - 1 (stamp.py:60). */
int rh_session_lengths(const int64_t* seq, int B, int L, int check_full, int64_t* counts, int32_t* err, void* stream);
int rh_session_dropout_fwd(const float* x, int64_t n, float p, int64_t* rng, int64_t* saved_ctr, float* y, void* stream);
int rh_session_dropout_bwd(const float* g, int64_t n, float p, const int64_t* rng, const int64_t* saved_ctr, float* dx,
                           void* stream);

/* ---- SASRec: the transformer block around the causal attention, fused per row tile (csrc/sasrec.hip) -----------------
 * fp32.  M = B L rows of width D, 1 <= D <= RH_SASREC_MAX_D, any M >= 1, else RH_E_UNSUPPORTED before any launch; M = 0 returns at
 * once.  seq (B, L) int64: the history ids, 0 = pad (m = seq != 0).  Every LayerNorm: mean, then the variance as the mean
 * of (x - mean)^2 (two passes), rstd = 1 / sqrt(var + eps), out = (x - mean) rstd gamma + beta; stats (M, 2) = the rows'
 * (mean, rstd).  An all-zero row gives exactly beta.  No atomics: every reduction over rows goes through one partial per
 * workgroup (rh_sasrec_ntiles(M, D) of them: a HOST int, like rh_sine_nchunks) summed in a fixed order by rh_colsum; a
 * backward run twice gives the same bits.  Dropout: rh_drop_hash over the device (seed, counter) pair rng, kept when
 * hash >= p 2^32, scaled by 1 / (1 - p), recomputed in the backward; an entry point draws ONE counter value, returns it in
 * saved_ctr (1,) and advances the device counter; p = 0 computes no hash and takes null rng / saved_ctr.  Element index
 * ranges of one call:  rh_sasrec_input_fwd  [0, M D): (b L + l) D + d;
 *                      rh_sasrec_ffn_fwd    dropout1 [0, M D): row D + c;  dropout2 [M D, 2 M D): M D + row D + c.
 *
 * rh_sasrec_input_fwd: e (B, L, D) with row (b, l) at e + b e_bstride + l e_rstride (a slice of the (B, 3, L, >= D) gather),
 *   P (max_len, D), L <= max_len.  x0 (B, L, D) = m dropout(e scale + P[l]) (scale = sqrt(D) as the caller rounds it).
 * rh_sasrec_input_bwd: g_x0 -> g_e (B, L, D) contiguous and g_P (max_len, D) = the sum over b in ascending order, rows
 *   l >= L written as zero.  The one exception to "M = 0 returns at once": with B L = 0 it still launches, because the sum
 *   over no samples is a result too -- g_P is written as all zero (g_e has no element).
 * replaces: SASRec.seq_forward torch_rechub/models/matching/sasrec.py:75-84 (scale, position lookup and add, dropout, mask).
 *
 * rh_sasrec_attn_in_fwd: x (M, D) -> Q (M, D) = LN(x; gamma, beta), qkv (M, 3 D) = [Q Wq^T + bq | x Wk^T + bk | x Wv^T + bv]
 *   with w (3 D, D) = in_proj_weight, b (3 D,) = in_proj_bias, stats (M, 2).
 * rh_sasrec_attn_in_bwd: g_qkv (M, 3 D), g_Q (M, D) (the residual's) -> g_x (M, D) and part (ntiles, 2, D) = per-tile
 *   (g_gamma, g_beta).  The weight and bias gradients are rh_linear_wgrad of (g_qkv[:, :D], Q) and (g_qkv[:, D:], x).
 * replaces: sasrec.py:90-91 (LayerNorm, the in-projection of nn.MultiheadAttention with query != key) and their autograd.
 *
 * rh_sasrec_ffn_fwd: attn (M, D) (the heads' output before out_proj), Q (M, D) -> y = Q + attn Wo^T + bo; z = LN(y);
 *   a = relu(dropout1(z W1^T + b1)); out = m (z + dropout2(a W2^T + b2)); ONE launch for the chain (the counter's advance
 *   is a one-thread launch behind it, as in rh_softmax_attn_fwd).  Saves y, z, a (M, D) and stats (M, 2).
 * rh_sasrec_ffn_bwd: g_out (M, D) -> g_attn, g_Q (M, D); g_f = g (a W2^T + b2) and g_h = g (z W1^T + b1) (M, D) are emitted
 *   as the operands of the weight gradients, formed by rh_linear_wgrad: (g_f, a) for W2 / b2, (g_h, z) for W1 / b1,
 *   (g_Q, attn) for Wo / bo (g_y = g_Q); part (ntiles, 2, D) = per-tile (g_gamma, g_beta).  ONE launch.
 * replaces: sasrec.py:91-98 (out_proj, residual, LayerNorm, PointWiseFeedForward sasrec.py:173-177, mask) and their
 *           autograd.
 *
 * rh_sasrec_head_fwd: s = LN(x) (M = B L rows); pos_logit, neg_logit (M,) = s . pos_e, s . neg_e with pos_e / neg_e
 *   (B, L, D) slices of the gather (row (b, l) at b *_bstride + l e_rstride).  pos_e = neg_e = null: LayerNorm only (s written; the logits
 *   may be null); s may be null when the logits are wanted.
 * rh_sasrec_head_bwd: g_s (M, D) or null, g_pos, g_neg (M,) or null -> g_x (M, D), g_pos_e, g_neg_e (B, L, D) contiguous,
 *   part (ceil(M / 64), 2, D) = per-workgroup (g_gamma, g_beta).
 * replaces: sasrec.py:100 (last_layernorm) and 156-157 (the two masked products and sums), torch.nn.LayerNorm of the
 *           selected rows in user_tower, and their autograd. */
#define RH_SASREC_MAX_D 128
int rh_sasrec_ntiles(int M, int D, int* ntiles);
int rh_sasrec_input_fwd(const int64_t* seq, const float* e, int64_t e_bstride, int64_t e_rstride, const float* P, int B, int L,
                        int D, int max_len, float scale, float p_drop, int64_t* rng, int64_t* saved_ctr, float* x0, void* stream);
int rh_sasrec_input_bwd(const int64_t* seq, const float* g_x0, int B, int L, int D, int max_len, float scale, float p_drop,
                        const int64_t* rng, const int64_t* saved_ctr, float* g_e, float* g_P, void* stream);
int rh_sasrec_attn_in_fwd(const float* x, const float* gamma, const float* beta, float eps, const float* w, const float* b,
                          int M, int D, float* Q, float* qkv, float* stats, void* stream);
int rh_sasrec_attn_in_bwd(const float* x, const float* gamma, const float* w, const float* stats, const float* g_qkv,
                          const float* g_Q, int M, int D, float* g_x, float* part, void* stream);
int rh_sasrec_ffn_fwd(const float* attn, const float* Q, const int64_t* seq, const float* wo, const float* bo,
                      const float* gamma, const float* beta, float eps, const float* w1, const float* b1, const float* w2,
                      const float* b2, int M, int D, float p_drop, int64_t* rng, int64_t* saved_ctr, float* y, float* z,
                      float* a, float* stats, float* out, void* stream);
int rh_sasrec_ffn_bwd(const int64_t* seq, const float* wo, const float* gamma, const float* w1, const float* w2,
                      const float* y, const float* a, const float* stats, const float* g_out, int M, int D, float p_drop,
                      const int64_t* rng, const int64_t* saved_ctr, float* g_f, float* g_h, float* g_Q, float* g_attn,
                      float* part, void* stream);
int rh_sasrec_head_fwd(const float* x, const float* gamma, const float* beta, float eps, const float* pos_e,
                       int64_t pos_bstride, const float* neg_e, int64_t neg_bstride, int64_t e_rstride, int B, int L, int D,
                       float* s, float* pos_logit, float* neg_logit, float* stats, void* stream);
int rh_sasrec_head_bwd(const float* x, const float* gamma, const float* beta, const float* stats, const float* pos_e,
                       int64_t pos_bstride, const float* neg_e, int64_t neg_bstride, int64_t e_rstride, const float* g_s,
                       const float* g_pos, const float* g_neg, int B, int L, int D, float* g_x, float* g_pos_e, float* g_neg_e, float* part,
                       void* stream);

/* ---- row-sharded tables (one shard per rank) -----------------------------------------------------------------------
 * Global row g of a table lives on rank g % world as local row g / world.  rh_shard_localize rewrites an index matrix
 * idx (n_rows, F) (int64 / int32, contiguous: the all-gathered indices of the global batch) for this rank's shards:
 *   local[i, f] = g / world   if g % world == rank and g != pad[f]
 *               = sink[f]     otherwise (the shard's all-zero row, passed to the gather / scatter / optimizer kernels as
 *                             the field's padding_idx: read as zeros, never updated)
 * desc (device int64 [3F]): vocab[F] | pad[F] (-1: none) | sink[F].  g outside [0, vocab) sets RH_FLAG_INDEX_OOB
 * (and maps to the sink row).  The gathers of all ranks over `local` sum to the reference's lookup, one non-zero
 * contributor per element.
 * replaces: nn.Embedding lookup on a replicated table, torch_rechub/basic/layers.py:83-99 under
 *           nn.DataParallel (trainers/ctr_trainer.py:53-55), which broadcasts every table every step. */
int rh_shard_localize(const void* idx, int idx_is_i64, int64_t n_rows, int F, const int64_t* desc, int world, int rank,
                      int32_t* local, int32_t* err_flag, void* stream);
/* The (n_rows, F) int64 index matrix (row stride ld) as contiguous int32 for the wire of the index all-gather, saturating (ids
 * beyond int32 stay out of range, below -1 -> -1); written into the caller's slice of the gather buffer (in-place collective). */
int rh_shard_narrow(const int64_t* idx, int64_t ld, int64_t n_rows, int F, int32_t* out, void* stream);

/* ---- two-tower score tails and the SENET field gate (csrc/twotower.hip) ---------------------------------------------
 * fp32, one wavefront per row, no atomics: every backward run twice gives the same bits.  A refusal (RH_E_*) returns
 * before any launch and touches nothing.  rh_twotower_nblocks answers through a HOST int, like rh_sine_nchunks: *nblocks = the
 * workgroups a launch over B rows uses (the rows of rh_senet_bwd's w_partial).
 * rh_band_logits_fwd: logits (B, K1)[i, k] = (u_i . v_j / (max(||u_i||, eps) max(||v_j||, eps)) - log w_j) / temperature,
 *   j = (i + k) mod B; nu (B,) = ||u_i||, nv (B,) = ||v_j|| saved.  u, v (B, D) with row strides ldu, ldv; w (B,).
 * rh_band_logits_bwd: g (B, K1) -> g_u (B, D), g_v (B, D), both contiguous and fully written by the wavefront of their row:
 *   g_u[r] over the item rows (r + k) mod B, g_v[r] over the user rows (r - k) mod B, ascending k.  As in ATen, the clamp
 *   takes no part in the gradient: dc/du = (v^ - c u / ||u||) / max(||u||, eps), and v^ / eps for a zero row.  w gets no
 *   gradient.
 *   1 <= D <= RH_TWOTOWER_MAX_D, 1 <= K1 <= B, else RH_E_UNSUPPORTED.
 * replaces: torch.cosine_similarity(u.unsqueeze(1), v, dim=2), the broadcast log-weight subtraction, the [index0, index1]
 *           gather and the division of YoutubeSBC.forward torch_rechub/models/matching/youtube_sbc.py:61-80, whose
 *           intermediates are (B, B) and (B, B, D).
 * rh_pair_cosine_fwd: pos (B,) = n(hu) . n(hp), neg (B,) = n(hu) . n(hn), n(x) = x / max(||x||, eps) row-wise; nrm (3, B) =
 *   the three norms saved.  rh_pair_cosine_bwd: g_pos, g_neg (B,) -> g_hu, g_hp, g_hn (B, D) contiguous.  1 <= D <= RH_TWOTOWER_MAX_D.
 * replaces: the three F.normalize calls and two multiply-sum reductions of FaceBookDSSM
 *           torch_rechub/models/matching/dssm_facebook.py:52-53,64,75-76.
 * rh_senet_fwd: x (B, F, D) with sample stride ldx (a sample's F D values contiguous), w1 (R, F), w2 (F, R) ->
 *   z (B, F) = mean_d x, h (B, R) = relu(w1 z), a (B, F) = relu(w2 h), y (B, F D) contiguous = x a[..., None].
 * rh_senet_bwd: g (B, F, D) with sample stride ldg -> g_x (B, F D) contiguous; w_partial (*nblocks of rh_twotower_nblocks, 2 R F) =
 *   per-workgroup sums [g_w1 (R, F) | g_w2 (F, R)] over the workgroup's samples in ascending order (g_w = rh_colsum of it).
 *   ReLU's derivative at 0 is 0.  1 <= R <= F <= RH_SENET_MAX_F, 1 <= D <= RH_SENET_MAX_D, else RH_E_UNSUPPORTED.
 * replaces: SENETLayer.forward torch_rechub/basic/layers.py:525-529 and its autograd. */
#define RH_TWOTOWER_MAX_D 1024
#define RH_SENET_MAX_F 64
#define RH_SENET_MAX_D 256
int rh_twotower_nblocks(int B, int* nblocks);
int rh_band_logits_fwd(const float* u, int64_t ldu, const float* v, int64_t ldv, const float* w, int B, int D, int K1,
                       float temperature, float eps, float* logits, float* nu, float* nv, void* stream);
int rh_band_logits_bwd(const float* u, int64_t ldu, const float* v, int64_t ldv, const float* nu, const float* nv, const float* g,
                       int B, int D, int K1, float temperature, float eps, float* g_u, float* g_v, void* stream);
int rh_pair_cosine_fwd(const float* hu, int64_t ldu, const float* hp, int64_t ldp, const float* hn, int64_t ldn, int B, int D,
                       float eps, float* pos, float* neg, float* nrm, void* stream);
int rh_pair_cosine_bwd(const float* hu, int64_t ldu, const float* hp, int64_t ldp, const float* hn, int64_t ldn, const float* nrm,
                       const float* g_pos, const float* g_neg, int B, int D, float eps, float* g_hu, float* g_hp, float* g_hn,
                       void* stream);
int rh_senet_fwd(const float* x, int64_t ldx, const float* w1, const float* w2, int B, int F, int R, int D, float* y, float* z,
                 float* h, float* a, void* stream);
int rh_senet_bwd(const float* x, int64_t ldx, const float* w1, const float* w2, const float* z, const float* h, const float* a,
                 const float* g, int64_t ldg, int B, int F, int R, int D, float* g_x, float* w_partial, void* stream);

/* ---- TIGER / T5: masked, biased, rectangular softmax attention and the residual RMS norm (csrc/t5attn.hip) ----------
 * q: (B, Lq, H, dh) view with row stride ldq; k, v: (B, Lk, H, dh) views sharing the row stride ldkv (separate projections,
 * or column blocks of one fused QKV / KV product).  No scale on q . k.  key_mask (B, Lk) uint8 or null: a key with 0 is
 * excluded; causal = 1 excludes j > i and needs Lq == Lk.  An excluded score is the most negative finite float, as the
 * reference's additive mask makes it: a row with no key left (under a mask and causal = 1 also a row whose keys j <= i are
 * all masked) gets weight 1 / Lk on every one of the Lk keys.  bias (nb, H) or null,
 * bucket (Lq + Lk - 1,) int32 built by the host: the score (i, j, h) gets bias[bucket[(j - i) + (Lq - 1)], h].  p_drop in
 * [0, 1): dropout on the weights with the counter hash over element ((b H + h) Lq + i) Lk + j; rng, saved_ctr as in
 * rh_softmax_attn_*.
 * rh_t5_attn_fwd: out (B, Lq, H dh); lse (B, H, Lq) the rows' log-sum-exp, +inf marking a row with no key left.
 * rh_t5_attn_bwd: g_out (B, Lq, H dh) -> g_q ((B, Lq, H, dh) view, row stride ldgq), g_k, g_v ((B, Lk, H, dh) views, row
 *   stride ldgkv), g_bias (nb, H) when bias is given, through part (*nparts of rh_t5_attn_nparts(B, Lq, H), Lq + Lk - 1) per-workgroup
 *   sums by diagonal, added in a fixed order; delta (B, H, Lq) workspace.  Weights recomputed tile by tile from lse; nothing
 *   of size Lq x Lk is written; no atomics.
 * The two nparts functions answer through a HOST int, like rh_twotower_nblocks.
 * Lq <= 8 (the decoder side) runs one wavefront per (sample, head), four to a workgroup; longer queries the 64 x 64 MFMA tile.
 * 1 <= Lq, Lk <= RH_ATTN_MAX_L, 1 <= dh <= RH_ATTN_MAX_DH, H >= 1, nb >= 1 or no bias, else RH_E_UNSUPPORTED before any launch; B = 0
 * returns at once.
 * replaces: T5Attention.forward (projection reshapes, matmul, compute_bias, the additive mask, softmax, dropout, matmul)
 *           of the T5 stack under torch_rechub/models/generative/tiger.py, and its autograd.
 * rh_add_rms_norm_fwd: h_new (M, D) = h + delta (delta null: h_new = h, and h_new may be null), y = h_new *
 *   rsqrt(mean(h_new^2) + eps) * w, rstd (M,) saved.  rh_add_rms_norm_bwd: g_y (M, D), g_res (M, D) or null (the gradient
 *   that reached h_new directly) -> g_h (M, D) (= g_delta); part (*nparts of rh_add_rms_norm_nparts(M), D) per-workgroup sums of g_w
 *   over rows in a fixed order (g_w = rh_colsum of it).  One wavefront per row, one pass.  1 <= D <= RH_RMS_NORM_MAX_D, else
 *   RH_E_UNSUPPORTED; M = 0 returns at once.
 * replaces: the residual add and T5LayerNorm.forward of every T5 sub-layer, and their autograd. */
#define RH_RMS_NORM_MAX_D 1024
int rh_t5_attn_nparts(int B, int Lq, int H, int* nparts);
int rh_t5_attn_fwd(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, int B, int Lq, int Lk, int H,
                   int dh, const uint8_t* key_mask, int causal, const float* bias, const int32_t* bucket, int nb, float p_drop,
                   int64_t* rng, int64_t* saved_ctr, float* out, float* lse, void* stream);
int rh_t5_attn_bwd(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, int B, int Lq, int Lk, int H,
                   int dh, const uint8_t* key_mask, int causal, const float* bias, const int32_t* bucket, int nb, float p_drop,
                   const int64_t* rng, const int64_t* saved_ctr, const float* out, const float* lse, const float* g_out,
                   float* delta, float* g_q, int64_t ldgq, float* g_k, float* g_v, int64_t ldgkv, float* part, float* g_bias,
                   void* stream);
int rh_add_rms_norm_nparts(int M, int* nparts);
int rh_add_rms_norm_fwd(const float* h, const float* delta, const float* w, float eps, int M, int D, float* h_new, float* y,
                        float* rstd, void* stream);
int rh_add_rms_norm_bwd(const float* h_new, const float* w, const float* rstd, const float* g_y, const float* g_res, int M,
                        int D, float* g_h, float* part, void* stream);

/* ---- TIGER: one step of the constrained beam search over a flat trie (csrc/beam.hip) --------------------------------
 * The constraint is a trie in CSR form: node 0 is the root, the edges of node n are [child_off[n], child_off[n + 1]) of
 * child_tok (ascending and distinct inside a node) and child_node; child_off (n_nodes + 1,), all int32.
 * logits (B K, V) fp32 with row stride ld >= V: row b K + k is beam k of query b.  running (B, K) fp32 the beams' scores,
 * node (B, K) int32 their trie nodes; a node outside [0, n_nodes) (-1) is a dead beam.
 * Per query: lse_k = max + log(sum exp(x - max)) over the V values of beam k's row, fp32, accurate expf / logf; it
 * depends on the row's values alone (not on b, k, B or ld).  The candidates are the edges (k, e) of every live beam's
 * node, score = running[b, k] + ((logits[row, tok_e] - max) - log(sum)) in fp32: the log-softmax runs over the whole
 * vocabulary and is not renormalised over the allowed tokens.  Slot j of running_out, parent_out, tok_out, node_out (B, K)
 * gets score, beam, token and child node of the j-th best candidate under (score descending, beam ascending, token
 * ascending).  A candidate whose score is -inf (an allowed token with a -inf logit) is never listed, as the dense
 * formulation cannot tell it from a masked token; a token outside [0, V) is no candidate.  With fewer than K candidates
 * above -inf the unused slots get (-inf, -1, -1, -1) and short_out (B,) int32 = 1, else 0.  Every output element is
 * written on every call.  A dead beam and a node without children add nothing and index no edge array; a dead beam's row
 * is not read.  No atomics, no workspace, one launch: two runs give the same bits.
 * Outside the contract: a row with a NaN or a +inf, or without a finite value (the row of a dead beam may hold anything).
 * 1 <= K <= RH_BEAM_MAX_K, 1 <= V <= 2^25, n_nodes >= 1, B K < 2^31; beyond that, on a null pointer, on ld < V or on an output that
 * overlaps logits, running or node: RH_E_BADARG before any launch.  B = 0 returns at once.
 * replaces: per decoding step of generate (models/generative/tiger.py), the prefix_allowed_tokens_fn calls of
 *           Trie.get (utils/data.py:798-886), the (B K, V) mask, log_softmax and torch.topk over (B, K V). */
#define RH_BEAM_MAX_K 64
int rh_beam_step(const float* logits, int64_t ld, const float* running, const int32_t* node, const int32_t* child_off,
                 const int32_t* child_tok, const int32_t* child_node, int n_nodes, int B, int K, int V, float* running_out,
                 int32_t* parent_out, int32_t* tok_out, int32_t* node_out, int32_t* short_out, void* stream);

/* Compressed Interaction Network, one layer (csrc/cin.hip): a GEMM over rows m = (b, d) and channels c = f Hp + h whose A
 * operand x0[b, f, d] h[b, h, d] is formed in registers from two LDS tiles; the (B, F Hp, D) product never exists in HBM.
 * fp32, the 64 x 64 tile on v_mfma_f32_32x32x2_f32, K = F Hp walked in chunks of 64 (an odd K ends in a zero-filled step).
 * x0 (B, F, D): sample stride x0_sample_stride, field stride x0_field_stride >= D, d contiguous (a view of the fused
 * gather's output is read in place).  h (B, Hp, D): sample stride h_sample_stride, a sample's Hp D values contiguous (the
 * second half of the previous layer's y is read in place).  w (Ho, F Hp) = conv.weight[:, :, 0], bias (Ho,).
 * rh_cin_fwd:   y (B, Ho, D) contiguous = relu(bias[o] + sum_c w[o, c] x0[b, f, d] h[b, h, d]).
 * rh_cin_bwd:   y, g_y (B, Ho, D) contiguous; gp = g_y where y > 0, else 0 -> g_x0 (B, F, D) and g_h (B, Hp, D), both
 *   contiguous, either may be null (not computed).  A workgroup owns 64 rows for all of K: no atomics, a fixed order,
 *   every element written exactly once.
 * rh_cin_wgrad: partial (*nchunks of rh_cin_wgrad_chunks, Ho F Hp + Ho) = per-chunk sums [g_w (Ho, F Hp) | g_bias (Ho,)]
 *   over consecutive rows in a fixed order ([g_w | g_bias] = rh_colsum of it: bitwise reproducible).  *nchunks <= 16,
 *   a HOST int, like rh_sine_nchunks.
 * B >= 0, 1 <= D <= RH_CIN_MAX_D, 1 <= F <= RH_CIN_MAX_F, 1 <= Hp <= RH_CIN_MAX_HP, 1 <= Ho <= RH_CIN_MAX_HO, else RH_E_UNSUPPORTED before any launch; B = 0
 * returns at once.  LDS: forward and bwd 4 (64 (F|1 + Hp|1) + 8320) bytes each (115712 at the limits), wgrad 33280.
 * replaces: CIN.forward torch_rechub/basic/layers.py:359-362 (broadcast product, view, Conv1d, relu) and its autograd. */
#define RH_CIN_MAX_D 128
#define RH_CIN_MAX_F 64
#define RH_CIN_MAX_HP 256
#define RH_CIN_MAX_HO 512
int rh_cin_wgrad_chunks(int B, int D, int F, int Hp, int Ho, int* nchunks);
int rh_cin_fwd(const float* x0, int64_t x0_sample_stride, int64_t x0_field_stride, const float* h, int64_t h_sample_stride,
               const float* w, const float* bias, int B, int D, int F, int Hp, int Ho, float* y, void* stream);
int rh_cin_bwd(const float* x0, int64_t x0_sample_stride, int64_t x0_field_stride, const float* h, int64_t h_sample_stride,
               const float* w, const float* y, const float* g_y, int B, int D, int F, int Hp, int Ho, float* g_x0, float* g_h,
               void* stream);
int rh_cin_wgrad(const float* x0, int64_t x0_sample_stride, int64_t x0_field_stride, const float* h, int64_t h_sample_stride,
                 const float* y, const float* g_y, int B, int D, int F, int Hp, int Ho, float* partial, void* stream);

/* ---- evaluation metrics (csrc/metric.hip) ---------------------------------------------------------------------------
 * Exact AUC / GAUC.  pred: n float32 values with element stride pred_stride; label: n contiguous values of label_dtype
 * (0 float32, 1 float64, 2 int64, 3 uint8 / bool), 1 = positive, 0 = negative; g: n dense group ids in [0, G) or null
 * (G = 1).  Two predictions are tied when their VALUES are equal: -0.0 == +0.0, every other bit pattern -- distinct
 * denormals included -- is its own value, whatever the FP denormal mode (bit patterns are compared).  1 <= n < 2^31.
 * rh_auc_keys: keys (n,) int64 = the group in the high word, below it the prediction's bit pattern made monotone; any
 *   ascending sort of the keys (torch.sort: plumbing, there is no hand-written sort here) gives the permutation `order`
 *   under which (g, pred) ascends.
 * rh_auc_groups: out (3, G) int64 = P_g (positives), N_g (negatives), U2_g = sum over the positives i of g of
 *   2 #{negatives of g with pred < pred_i} + #{negatives of g with pred == pred_i}   (AUC_g = U2_g / (2 P_g N_g)).
 *   Integer arithmetic throughout; tie runs and groups may span any number of workgroups (per-chunk aggregates, a scan by
 *   one workgroup, a second pass; 64-bit integer atomics into the group slots): two runs give the same bits.  bad (2,)
 *   int64 = the count of non-finite predictions and the count of labels that are neither 0 nor 1 (an `order` entry
 *   outside [0, n) or a group id outside [0, G) is counted with the latter and written nowhere); with either non-zero,
 *   out is undefined.  out and bad are zeroed by the call.  workspace: *workspace_bytes of rh_auc_plan.
 * rh_auc_plan answers through HOST pointers: *chunk = the sorted elements one workgroup takes per trip, *max_grid = the
 *   grid cap (more chunks than that: further trips).
 * rh_gauc_reduce: stats = out of rh_auc_groups; weights (G,) double or null (the group size P_g + N_g).  result (2,)
 *   double = sum_g w_g U2_g / (2 P_g N_g), sum_g w_g over the groups holding both classes; *single_class = the number of
 *   groups holding one class (left out of both sums).  partial: 3072 doubles of workspace.  Per-workgroup partials over a
 *   grid that depends on G alone, added in index order: bit-reproducible.
 * rh_log_loss: result (1,) double = -mean(y log p + (1 - y) log(1 - p)), p widened to double first; partial: 1024
 *   doubles; the same fixed order.  Non-finite terms propagate (p = 0 with y = 0 gives nan through 0 * -inf).
 * replaces: roc_auc_score behind auc_score torch_rechub/basic/metric.py:20-22, get_user_pred and the per-user loop of
 *           gauc_score metric.py:25-74, log_loss metric.py:198-200, and the per-batch .cpu() of the trainers' evaluate
 *           (trainers/ctr_trainer.py:157-172, match_trainer.py:225-236, mtl_trainer.py:238-252).
 *
 * List metrics.  pred (M, K) int64 with row stride ld >= K, 1 <= K <= RH_RANK_MAX_K; truth as CSR: truth_off (M + 1,) and truth_ids
 * (n_truth,) int64 (offsets are clamped into [0, n_truth]).  cutoffs: a HOST array of n_k <= RH_RANK_MAX_CUTOFFS ints in [1, K].  gain (K,)
 * double = 1 / log2(j + 2) and ideal (K + 1,) double = its sequential prefix sums, ideal[0] = 0, both built by the caller.
 * Membership is equality of ids; duplicates on either side count as the reference counts them.  Per user with a
 * non-empty list and cut-off k: hit = #{j < k: pred[j] in truth}, mrr = 1 / (1 + first hit), recall = hit / len,
 * precision = hit / k, ndcg = dcg / ideal[min(len, k)], dcg = the gains of the hit positions added in ascending j -- the
 * float64 reference's own operations in its own order, hence its bits.  A user with an empty list adds nothing.
 * hits (n_k,) int64, gts (1,) int64 = sum of len (both exact, zeroed by the call), sums (n_k, 4) double = mrr, recall,
 * precision, ndcg summed over users (per-workgroup partials added in index order), per_user (M, n_k, 5) double = hit, mrr,
 * recall, precision, ndcg, or null.  partial: *partial_doubles of rh_rank_metrics_plan, which also reports (HOST
 * pointers) *stage = the truth ids staged through LDS at a time, the users per workgroup and the grid cap.
 * replaces: the loops of topk_metrics torch_rechub/basic/metric.py:142-176. */
#define RH_RANK_MAX_K 256
#define RH_RANK_MAX_CUTOFFS 8
int rh_auc_plan(int64_t n, int* chunk, int* max_grid, int64_t* workspace_bytes);
int rh_auc_keys(const float* pred, int64_t pred_stride, const int64_t* g, int64_t n, int64_t* keys, void* stream);
int rh_auc_groups(const float* pred, int64_t pred_stride, const void* label, int label_dtype, const int64_t* g,
                  const int64_t* order, int64_t n, int64_t G, void* workspace, int64_t* out, int64_t* bad, void* stream);
int rh_gauc_reduce(const int64_t* stats, const double* weights, int64_t G, double* partial, double* result,
                   int64_t* single_class, void* stream);
int rh_log_loss(const float* pred, int64_t pred_stride, const void* label, int label_dtype, int64_t n, double* partial,
                double* result, void* stream);
int rh_rank_metrics_plan(int M, int* stage, int* users_per_workgroup, int* max_grid, int64_t* partial_doubles);
int rh_rank_metrics(const int64_t* pred, int64_t ld, int M, int K, const int64_t* truth_off, const int64_t* truth_ids,
                    int64_t n_truth, const int* cutoffs, int n_k, const double* gain, const double* ideal, double* partial,
                    int64_t* hits, int64_t* gts, double* sums, double* per_user, void* stream);

/* Beyond-accuracy metrics over the same pred (M, K) int64, row stride ld >= K, 1 <= K <= RH_RANK_MAX_K, M >= 1; cutoffs: a HOST
 * array of 1 <= n_k <= RH_RANK_MAX_CUTOFFS ints in [1, K], in any order, duplicates allowed; outputs are in the caller's order of cut-offs.
 * An id below 0 is an absent position (the -1 padding of rh_topk): the user's list is shorter there -- the reference run
 * on the rows with the negative entries removed.  K or n_k outside its range: RH_E_UNSUPPORTED before any launch; a
 * cut-off outside [1, K], ld < K, M < 1 or a null pointer: RH_E_BADARG before any launch.  No float atomics: a wavefront
 * adds its users one after the other, a workgroup its wavefronts in index order into one partial, one workgroup the
 * partials in index order -- two calls give the same bits, and a user's value does not depend on the other users.
 * rh_ild: intra-list diversity.  table (V, D) float32 with row stride table_stride >= D, V >= 1, 1 <= D <= RH_ILD_MAX_D (else
 *   RH_E_UNSUPPORTED before any launch).  Per user and cut-off k: the items are the entries among the first k with
 *   0 <= id < V (an id >= V is unknown and dropped; duplicates are separate entries); with n < 2 of them the user is left
 *   out; else, e_i the rows widened to double and u_i = e_i / max(||e_i||, 1e-10), the value is the mean over the pairs
 *   i < j of 1 - u_i . u_j, computed as 1 - (||sum u_i||^2 - sum ||u_i||^2) / (n (n - 1)) in double, O(k D) per user:
 *   nothing of size (M, K, D) or (M, K, K) is formed.  sums (n_k,) double = the values added over the users, counts (n_k,)
 *   int64 = the users that contributed (exact; zeroed by the call), per_user (M, n_k) double = the values, nan where the
 *   user was left out, or null.  partial: *partial_doubles of rh_ild_plan, which also reports (HOST pointers) the users per
 *   workgroup and the grid cap (more users than their product: further trips).
 * rh_coverage: counts (n_k,) int64 (zeroed by the call) = the distinct ids in [0, n_slots) among pred[:, :k], for every
 *   cut-off in one pass; ids outside are ignored.  first (n_slots,) int32 of workspace (*workspace_bytes of
 *   rh_coverage_plan), which the call sets to K and then lowers to the first column of every id by integer atomic minima:
 *   exact in any order of arrival.  1 <= n_slots < 2^31, else RH_E_UNSUPPORTED before any launch.  rh_coverage_plan also
 *   reports (HOST pointers) the rows a workgroup marks per trip and the grid cap of both passes (the counting pass takes
 *   256 slots per workgroup and trip).
 * rh_novelty: pop (V,) of pop_dtype (0 float32, 1 float64), V >= 1.  An id >= 0 adds -log2(max(p, 1e-10)) in double,
 *   p = pop[id] widened, p = 1e-10 for id >= V.  Per user and cut-off: the mean over the present positions among the first
 *   k, added in a fixed order; a user with none is left out.  sums, counts, per_user, partial and rh_novelty_plan: as for
 *   rh_ild.
 * replaces: the loops of diversity_score torch_rechub/basic/metric.py:203-251, coverage_score metric.py:254-277 and
 *           novelty_score metric.py:280-313. */
#define RH_ILD_MAX_D 1024
int rh_ild_plan(int M, int* users_per_workgroup, int* max_grid, int64_t* partial_doubles);
int rh_ild(const int64_t* pred, int64_t ld, int M, int K, const float* table, int64_t table_stride, int64_t V, int D,
           const int* cutoffs, int n_k, double* partial, double* sums, int64_t* counts, double* per_user, void* stream);
int rh_coverage_plan(int64_t n_slots, int* rows_per_workgroup, int* max_grid, int64_t* workspace_bytes);
int rh_coverage(const int64_t* pred, int64_t ld, int M, int K, int64_t n_slots, const int* cutoffs, int n_k, int32_t* first,
                int64_t* counts, void* stream);
int rh_novelty_plan(int M, int* users_per_workgroup, int* max_grid, int64_t* partial_doubles);
int rh_novelty(const int64_t* pred, int64_t ld, int M, int K, const void* pop, int pop_dtype, int64_t V, const int* cutoffs,
               int n_k, double* partial, double* sums, int64_t* counts, double* per_user, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RECHUB_HIP_H */
