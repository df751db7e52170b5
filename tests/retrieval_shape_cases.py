"""Case tables of tests/test_gpu_sine_rq_topk_shapes.py, importable without a GPU: the host tests of test_rqvae_host.py
and test_sine_host.py check from the float64 oracles alone how many rows each case excludes."""

# ---- the residual quantizer (csrc/rq.hip) -----------------------------------------------------------------------------
# The codebook passes through LDS in tiles of TK = rq_tile_codes(E) codes: 256 up to E = 47, 192 for E in 48..63, 128 at
# E = 64, 64 at E = 127 and 128.
#            N      E    sizes          seed
RQ_CASES = [(40, 16, [300], 70),            # TK 256: tiles of 256 + 44, the last narrower than a wavefront
            (40, 48, [200, 385], 71),       # TK 192: tiles 192 + 8 and 192 + 192 + 1
            (40, 64, [129, 128], 72),       # TK 128: 128 + 1, then exactly one tile
            (40, 127, [65], 73),            # TK 64: 64 + 1; LDS row stride = E; column tail of 3
            (19, 5, [2, 1, 3], 74),         # a one-code level; 16 + 3 rows
            (1, 3, [4], 75),                # N = 1
            (16, 128, [1024] * 8, 80),      # every upper limit at once; 1 048 576 gradient columns through rh_colsum
            (1030, 8, [6, 6], 77),          # 64 chunks of 17 rows; chunks 61..63 start past N and write zeros
            (32787, 33, [5, 3], 76)]        # 2050 row groups on 2048 workgroups, the last of 3 rows; 1 081 971 g_x elements
#                                             on 4096 workgroups; chunks of 513 rows


def rq_tile_codes(E):
    """csrc/rq.hip rq_tile_codes."""
    return min(256, (12288 // (E | 1)) // 64 * 64)


# ---- SINE (csrc/sine.hip) ------------------------------------------------------------------------------------------------
#              B    S   E   T   K  seed holes
SINE_CASES = [(5, 7, 21, 6, 6, 44, False),      # S E = 147: the scalar staging; K = T
              (3, 1, 1, 1, 1, 45, False),       # every lower limit
              (9, 64, 64, 64, 8, 46, False),    # E = 64: the lane + 64 half of the columns is empty
              (9, 33, 65, 9, 3, 47, True),      # E = 65: one column in that half; S E odd; holes
              (1, 5, 12, 4, 2, 48, False),      # B = 1, and that row is fully padded
              (200, 3, 4, 8, 8, 49, False)]     # K = T = 8; 64 concept-gradient chunks of 4 samples, the last 14 empty

# the aggregate kernels alone (only they have a capped grid): 16384 workgroups x 4 samples + 5
SINE_AGG_ONLY_CASE = (65541, 2, 3, 2, 2, 50, False)
SINE_TEMPERATURE, SINE_WARM_TEMPERATURE = 0.1, 50.0  # the example's, and one with logits of order one (at E >= 64)

MIN_GAP, MAX_EXCLUDED = 1e-4, 0.02  # of test_gpu_rq.py and test_gpu_sine.py

# ---- top-k (csrc/topk.hip) -------------------------------------------------------------------------------------------------
#                  M   D     V    K    bias
TOPK_INT_CASES = [(65, 64, 300, 128, True),     # the largest K with 64-row workgroups: all of topk_lds_bytes(128)
                  (33, 7, 300, 129, False),     # the first K with 32-row workgroups
                  (3, 7, 200, 63, False),       # K at both sides of one lane chunk of the list
                  (3, 7, 200, 65, True),
                  (3, 65, 130, 10, True),       # a second k chunk of one column (rounded up to two)
                  (2, 1023, 70, 10, False),
                  (2, 1024, 70, 64, True)]
