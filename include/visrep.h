/* libvisrep_hip.so — C ABI of the MI355X (gfx950) vision-representation scoring path.
 *
 * Drop-in boundary: the reference is pure Python on PyTorch; its hot path is a chain of stock
 * PyTorch calls.  Each entry point below replaces one such call chain and is what a ctypes binding inside the
 * reference would load.  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. torch tensor .data_ptr()) unless marked HOST
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); all work is enqueued
 *     asynchronously on it; nothing here synchronises, allocates or frees device memory
 *   - return value 0 = ok, negative = error (VISREP_ERR_*); visrep_last_error() gives the message; no C++
 *     exception crosses the boundary; no process-global mutable state: the error string and the A/B variant knobs are thread-local,
 *     caller-owned scratch is keyed by (device, stream), per-kernel LDS opt-ins and CU counts are cached per device
 *   - bf16 tensors are raw uint16 storage (torch.bfloat16), row-major, leading dimensions in ELEMENTS
 */
#ifndef VISREP_H
#define VISREP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VISREP_VERSION 650   /* 650: InternViT towers - visrep_vit_config grows trailing `norm` / `qk_norm`, visrep_vit_layer trailing `qn_g` / `kn_g` (struct changes), visrep_rmsnorm / visrep_rmsnorm_stats / visrep_qk_rmsnorm (+ _f32 / _cpu forms), visrep_gemm_bf16_resid_rms_stats, route ids 14 .. 18.  640: DINOv2-with-registers towers - visrep_vit_config grows a trailing `registers` (struct change), visrep_vit_weights::cls may be a [1 + registers, d] table, visrep_mhsa_prefix_fwd / visrep_mhsa_prefix_supported / visrep_prefix_rows, route id 13.  630: SwiGLU-FFN towers (DINOv2-giant) - VISREP_ACT_SWIGLU = 4 in visrep_vit_config::act (w1 / b1 / s1 then have 2 * mlp rows), VISREP_EPI_GATED, visrep_gemm_bf16_gated, visrep_swiglu, visrep_swiglu_f32, visrep_set_fuse_gate, visrep_debug_gated_refusal (new exports / newly accepted argument values; no struct layout change).  620: head widths other than 64 in the bf16 tower - visrep_vit_config grows head_dim / head_pad (struct change), visrep_mhsa_fwd takes head_dim 64 | 96 | 128, visrep_attention_fwd head_dim 96, route id 12; visrep_im2col and visrep_vit_forward_cpu no longer refuse an image side that is not a multiple of the patch - they floor the division as Conv2d does (newly accepted argument values).  610: visrep_cscore_transfer_packed2 / visrep_cscore_transfer2_cpu, the key-point transfer on two per-encoder banks (new exports only).  600 = round 6: reserved CUs, GEMM tile-walk knob, gemm variants 6-8, visrep_masked_nn_min_f32, window < 0 in the C-score transfers (new exports / newly accepted argument values only).  500 = round 5: device CU count, routing counters, MFMA probe, A-score reference arithmetic, host twins (new exports only).  410 = round 4: split-route `products`, stream-keyed scratch, per-thread knobs (changed signatures); 410: q_prescaled = 2, row-mapped GEMM, image-aligned / wide-head attention, conv + GroupNorm partials */

enum { VISREP_BF16 = 0, VISREP_F32 = 1 };
enum { VISREP_OK = 0, VISREP_ERR_ARG = -1, VISREP_ERR_SHAPE = -2, VISREP_ERR_LAUNCH = -3 };
/* GEMM epilogues */
enum {
    VISREP_EPI_BIAS = 0,   /* C = A W^T + bias                                   (nn.Linear)                    */
    VISREP_EPI_ACT = 1,    /* C = act(A W^T + bias)                              (Linear + QuickGELU/GELU)      */
    VISREP_EPI_RESID = 2,  /* C = resid + ls * (A W^T + bias)                    (Linear + LayerScale + add)    */
    VISREP_EPI_VT = 3,     /* V^T scatter for visrep_mhsa_fwd (see below)                                        */
    VISREP_EPI_PATCH = 4,  /* patch-embed: row remap past the CLS row + position add                             */
    VISREP_EPI_F32 = 5,    /* C(fp32) = A W^T + bias                                                             */
    VISREP_EPI_GATED = 7   /* C[m, 16 t + r] = silu(g) * u over N / 2 columns (visrep_gemm_bf16_gated only; 6 is internal) */
};
enum { VISREP_ACT_NONE = 0, VISREP_ACT_QUICK_GELU = 1, VISREP_ACT_GELU_ERF = 2, VISREP_ACT_GELU_TANH = 3,
       /* visrep_vit_config::act only (not an element-wise activation of the GEMM entry points): the tower's MLP is HF Dinov2SwiGLUFFN,
        * weights_out(silu(x1) * x2) with x1, x2 = weights_in(x).chunk(2).  `mlp` is then the (padded) hidden width h and w1 / b1 / s1 have 2 * mlp
        * rows: for visrep_vit_forward in the 16-row interleave of visrep_gemm_bf16_gated (or, with visrep_set_fuse_gate(0), in HF chunk order);
        * for the fp32 and host towers in HF chunk order (gate rows, then value rows).  w2 is [d, mlp]. */
       VISREP_ACT_SWIGLU = 4 };

int visrep_version(void);
/* copies the calling thread's last error message (NUL terminated) into buf; returns its length */
size_t visrep_last_error(char* buf, size_t n);

/* Kernel-variant knobs for A/B measurements.  They are PER-THREAD state (the calling thread's later launches only): there is no
 * process-global mutable state behind this ABI, and the defaults need no call at all.  Each returns the previous value.
 *
 * GEMM family used by every entry point below: 1 = 128x128 tiles, one barrier per K-tile (also: N % 256 != 0 shapes, tail rows, split-K,
 * implicit 3x3 convolution); 2 = 256x256 persistent ping-pong kernel, 64-byte LDS rows (runs when K % 64 != 0); 5 (default) = the same
 * structure with 128-byte LDS rows, a five-slot LDS-DMA ring and half the barriers (profiles/round2_gemm_v5.md).  2 and 5 need
 * N % 256 == 0.  Results are identical up to fp32 summation order.  (Variants 3 and 4 - measured dead ends, profiles/round2_gemm_v4.md -
 * exist only in the tools-only VISREP_EXPERIMENTS build.)  6 / 7 / 8 (round 6, A/B only: measured 20-30 % slower, profiles/round6_gemm.md) =
 * the "duo" kernel, two independent 4-wave workgroups per CU on 256 x 128 tiles (N % 128 == 0, K % 64 == 0, K >= 128; BIAS / ACT / RESID / VT
 * epilogues, everything else runs as variant 5): 6 = wherever it applies, 7 = for N <= 1024 only, 8 = its unpipelined first build.  Bitwise
 * equal to variant 5. */
int visrep_set_gemm_variant(int variant);
/* Attention forward at head width 64: 1 (default) = attn_fwd, the four-wave kernel that also serves head widths 128 / 192.  2 = attn_fwd_ab
 * (two 32-row query blocks per wave; measured equal-to-slower, profiles/round3_attention.md) exists only in the VISREP_EXPERIMENTS build;
 * the production library refuses it. */
int visrep_set_attn_variant(int variant);
/* Tile shape of the bf16 A-score Gram (visrep_ascore_maxcos*): 0 (default) = whichever launches the smaller tile area for (Nt, Nr);
 * 1 = one 128 x 128 tile per workgroup; 2 = persistent ping-pong tiles of 192 or 256 rows per operand (the GEMM default's structure;
 * 576 = 3 x 192, 256 = 1 x 256).  Results are identical up to fp32 summation order (none: both sum k in the same order per MFMA chain). */
int visrep_set_ascore_variant(int variant);
/* Timing-only ablation of GEMM variant 2 (bit 0: skip MFMAs, bit 1: skip the LDS-DMA loads, bit 2: skip the fragment reads):
 * results are WRONG for mask != 0; used by tools/gemm_ablate.py to attribute cycles.  Returns the previous mask. */
int visrep_debug_gemm_ablation(int mask);
/* Diagnostic builds (-DVISREP_GEMM_ABLATE) only: device buffer of 16 uint64 receiving per-segment cycle sums of variant 2
 * (wave 0 and wave 4 of block 0); ignored by production builds. */
int visrep_debug_gemm_timing_buffer(void* dev_u64x16);
/* Routing counters of the CALLING THREAD: how many launches each kernel family received since the last reset (host-side integers,
 * incremented by the dispatchers; HIP-graph replays do not pass through a dispatcher and are not counted).  Tests use them to assert
 * that a shape takes the route it was tuned for - e.g. that the 768-px diffusion tower's 256- / 512-channel convolutions run in the
 * persistent 256x256 kernel and its 128-channel ones in the 128x128 kernel with GroupNorm partials.  out: VISREP_ROUTE_COUNT longs
 * (NULL: only reset); reset != 0 clears the counters after the copy.  Returns VISREP_ROUTE_COUNT. */
enum {
    VISREP_ROUTE_GEMM_256 = 0,       /* persistent 256x256 kernel (variants 2 / 5), plain GEMM: head launch or whole problem */
    VISREP_ROUTE_GEMM_128 = 1,       /* 128x128 kernel, plain GEMM (N % 256 != 0, few tiles, variant 1) */
    VISREP_ROUTE_GEMM_TAIL = 2,      /* rows of a partial last tile round split off to the 128x128 kernel */
    VISREP_ROUTE_SPLITK = 3,         /* deterministic split-K pair (partials + reduce), GEMM or convolution */
    VISREP_ROUTE_CONV_256 = 4,       /* implicit 3x3 convolution in the persistent 256x256 kernel */
    VISREP_ROUTE_CONV_128 = 5,       /* implicit 3x3 convolution in the 128x128 kernel */
    VISREP_ROUTE_CONV_128_GN = 6,    /* ... that also emits GroupNorm partial sums */
    VISREP_ROUTE_ATTN = 7,           /* attn_fwd<ND> (head width 64 / 128 / 192) */
    VISREP_ROUTE_ATTN_WIDE = 8,      /* attn_fwd_wide (head width 512) */
    VISREP_ROUTE_ATTN_CLS = 9,       /* attn_fwd_cls (image-aligned CLS towers) */
    VISREP_ROUTE_CONV_HALO = 10,     /* conv3x3_halo: halo-resident 3x3 convolution with the input's GroupNorm + SiLU fused */
    VISREP_ROUTE_CONV_C8 = 11,       /* conv3x3_c8: the VAE's first convolution straight from 8-channel pixel tokens (no im2col) */
    VISREP_ROUTE_ATTN_96 = 12,       /* attn_fwd96 (head width 96: true widths 65 .. 96 zero-padded) */
    VISREP_ROUTE_ATTN_PREFIX = 13,   /* attn_fwd_prefix (image-aligned towers with CLS + register tokens) */
    VISREP_ROUTE_STATS_EPILOGUE = 14, /* row statistics of a residual GEMM from its epilogue's partial sums (ln_stats_finalize_rows / rms_stats_finalize_rows) */
    VISREP_ROUTE_STATS_REDUCE = 15,  /* ... written by the split-K reduction itself (N == 1024) */
    VISREP_ROUTE_STATS_ROWS = 16,    /* the read-only statistics pass over bf16 rows (visrep_layernorm_stats / visrep_rmsnorm_stats, called or fallen back to) */
    VISREP_ROUTE_RMS = 17,           /* any of the above, or a visrep_rmsnorm pass, in its RMS form */
    VISREP_ROUTE_QK_NORM = 18,       /* qk_rmsnorm_rows (visrep_qk_rmsnorm) */
    /* ConvNeXt towers (dwconv.hip).  New ids only: 0 .. 18 keep their meaning, and the version stays 650 - no struct or signature changed */
    VISREP_ROUTE_DWCONV_16 = 19,     /* dwconv7x7_stats_tile<16, 16>: the depthwise 7x7 convolution on 16 x 16 output tiles */
    VISREP_ROUTE_DWCONV_8 = 20,      /* dwconv7x7_stats_tile<8, 8>: the same on 8 x 8 tiles (small or ragged maps) */
    VISREP_ROUTE_DWCONV_FINALIZE = 21, /* the statistics finalize behind either (ln_stats_finalize_rows, or its odd-slot form) */
    VISREP_ROUTE_LN_S2D = 22,        /* ln_space_to_depth2_rows (visrep_ln_space_to_depth2) */
    /* SAM ViT towers (attention_relpos.hip).  New ids only, as above */
    VISREP_ROUTE_ATTN_RELPOS = 23,   /* attn_fwd_relpos (visrep_mhsa_relpos_fwd) */
    VISREP_ROUTE_RELPOS_TABLES = 24, /* relpos_tables_rows (visrep_relpos_tables) */
    VISREP_ROUTE_SAM_PARTITION = 25, /* sam_window_partition_qk + _vt (one count per visrep_sam_window_partition), sam_window_unpartition_rows */
    VISREP_ROUTE_SAM_NECK = 26,      /* the neck of visrep_sam_forward (one count per forward that reaches it: GEMM, LayerNorm, 3x3 convolution, LayerNorm) */
    VISREP_ROUTE_COUNT = 27
};
int visrep_debug_routes(long* out, int reset);
/* Matrix-pipe ceiling of THIS device under THIS process' conditions: `iters` bursts of 32 dependent-free v_mfma_f32_16x16x32_bf16 per wave,
 * 8 waves per CU, every CU, operands in registers (pseudo-random bf16 with |x| in [0.25, 4) when random != 0, small constants otherwise), no memory
 * traffic.  FLOP per launch = CUs * 8 * iters * 32 * 16384 (returned through *flop when non-NULL); the caller times the launch on
 * `stream`.  bench.py quotes the result beside the 2.5 PFLOP/s nominal peak: on random data the chip's power management holds a pure
 * MFMA stream near 1.9-2.0 PFLOP/s (DVFS), which is the practical roof every fraction on the line can also be read against.
 * sink: >= 24 bytes of 8-byte-aligned device memory: bytes [0, 4) are never written in practice; u64 [1] = shader-clock cycles (s_memtime) and
 * u64 [2] = 100-MHz ticks (s_memrealtime) of block 0's MFMA loop, i.e. the clock the stream ran at = [1] / ([2] * 10 ns) - the same pair of
 * counters, read in the tile-timing build of the GEMM (tools/gemm_tile_timing.py), gives the clock the GEMM runs at (profiles/round5_gemm.md). */
int visrep_debug_mfma_probe(int iters, int random, void* sink, double* flop, void* stream);
/* XCD-weighted tile split of the persistent 256x256 GEMM / convolution kernel (round 5).  The eight XCDs of an MI355X run at their own clocks
 * under the power limit (+-4 % around the mean inside one launch, measured with s_memtime / s_memrealtime: profiles/round5_gemm.md), so equal
 * shares of the tile list end when the slowest XCD does - and which XCD that is also depends on the kernel and its shape.  Per (kernel
 * instantiation, M, N, K) one launch in 8 records when each XCD finished; its last block leaves the time per round of tiles of each XCD in
 * pinned host memory; the following launches of that shape give every XCD whole rounds in proportion to its speed.  Results are bitwise
 * independent of the split.  OFF by default: a round of tiles is 2.8 % of a block's work at the headline shapes, as large as the effect, and
 * the same-box A/B measured +0.1 .. +0.3 % on the forward (profiles/round5_gemm.md section 3).  visrep_set_xcd_balance(1) (or
 * VISREP_XCD_BALANCE=1 in the environment) switches it on, process-wide; returns the previous setting.  Launches that are being CAPTURED into a
 * HIP graph always run with equal shares and are never measurements (a plan baked into a graph would be replayed with capture-time bounds forever):
 * the split serves eager launches only - the ViT / diffusion engines' graph replays are unaffected by it.  visrep_debug_xcd_balance: the smoothed relative time per round of each XCD (1 = mean; rel8 may
 * be NULL) of the shape launched most recently on the current device, and the number of measurements folded in so far; returns the setting. */
int visrep_set_xcd_balance(int on);
int visrep_debug_xcd_balance(float* rel8, unsigned* updates);
/* The split itself (pure host arithmetic, no device needed): rel8 = time per round of tiles of each XCD (any positive scale), grid = persistent
 * blocks (a multiple of 8), ntiles >= grid -> bounds9[x] .. bounds9[x + 1] = the tile indices of XCD x, bounds9[8] = ntiles; whole rounds of
 * grid / 8 tiles in proportion to speed, leftovers to the XCD that would finish first.  Returns 0, -1 for unusable arguments. */
int visrep_debug_xcd_split(const float* rel8, int grid, int ntiles, int* bounds9);

/* ---- optional device scratch owned by the caller (e.g. one torch tensor kept alive for the process).  With it,
 * visrep_gemm_bf16 splits the K loop of problems that have few output tiles but a deep reduction (the diffusion towers'
 * 3x3 convolutions at 12x12 / 24x24 resolution) across CUs and reduces the fp32 partial planes in slice order, i.e.
 * deterministically.  Registrations are keyed by (device, stream): visrep_set_scratch registers the buffer every stream of the CURRENT
 * device falls back to (enough when one stream per device runs GEMMs at a time); visrep_set_stream_scratch registers a buffer for ONE
 * stream of the current device and wins over the device-wide one - a caller that runs split-K GEMMs on several streams of a device
 * concurrently gives each stream its own (up to 8 per device).  (NULL, 0) detaches.  Both are thread-safe. */
int visrep_set_scratch(void* ptr, size_t bytes);
int visrep_set_stream_scratch(void* stream, void* ptr, size_t bytes);
/* Compute units of the CURRENT device as the dispatchers count them (cached per device; 256 on MI355X).  Callers that size launches for
 * whole tile rounds (engine.best_chunk, the sweep's launch plan) use it so that their arithmetic is the dispatcher's on any part. */
int visrep_device_cu_count(void);
/* CUs the persistent kernels leave free (round 6; multi-GPU insurance).  With world > 1 the sweep's C leg runs RCCL's all_to_all WHILE the next
 * tower launch's persistent GEMMs (grid = CU count) would own every CU (sweep.c_score_of; the reference has no counterpart: its feature dump,
 * llava/feature/extract.py:198-214, has no collective at all).  k (rounded down to a multiple of 8: the same number per XCD; ignored if fewer than
 * 64 CUs would remain) is subtracted from what visrep_device_cu_count() and every dispatcher see; 0 = off (default).  Process-wide;
 * VISREP_RESERVE_CUS=k in the environment is the same switch.  Set it before engines capture their HIP graphs.  Returns the previous value.
 * Unmeasured: no multi-GPU box was available in rounds 1-6; it exists so that the first one can A/B it. */
int visrep_set_reserved_cus(int k);
/* Tile order of the persistent 256x256 GEMM kernel (round 6 A/B knob, per thread; results do not depend on it).  0 = default: XCD-contiguous
 * chunks of the tile list, row-major, 4 x 8 windows for more than 8 column panels.  C = 1..255 (low byte): column-group-major - every XCD owns
 * whole row panels and walks them once per group of C column panels, so that the group's weight panels stay in that XCD's 4-MB L2 across rounds
 * (taken when the tile list splits into whole row panels per XCD and N / 256 is a multiple of C, else the default order).  Measured in
 * profiles/round6_gemm.md (FETCH_SIZE and time per window shape); the default stays 0.  Returns the previous value. */
int visrep_set_gemm_walk(int code);

/* ---- dense layers: replaces torch.nn.functional.linear (+ bias / activation / residual) inside
 * HF CLIPEncoderLayer / Dinov2Layer / SiglipEncoderLayer (transformers, called from
 * llava/model/multimodal_encoder/clip_encoder.py:48) and the mm_projector Sequential
 * (llava/model/multimodal_projector/builder.py:40-47).
 * A [M,K] bf16 (lda), W [N,K] bf16 (ldw, nn.Linear layout), bias [N] fp32 or NULL, C [M,N] bf16 (fp32 for EPI_F32).
 * N % 128 == 0, K % 64 == 0.  resid (bf16, same shape/ld as C, may alias C) and ls (fp32 [N] or NULL) are used by
 * EPI_RESID only.  C and resid must be 8-byte aligned (C 16-byte for EPI_F32) and ldc % 4 == 0 - a column window at a multiple of 4 elements
 * of an aligned buffer; anything less is refused before a launch, here and by the _ln, _rows and _resid_stats entries below.  16-byte aligned
 * C (and resid) with ldc % 8 == 0 selects the 16-byte store path. */
int visrep_gemm_bf16(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, int M, int N, int K,
                     int epilogue, int act, const void* resid, const float* ls, void* stream);

/* ---- LayerNorm over the last dim (torch.nn.LayerNorm in the HF blocks; CLIP pre_layrnorm).  x,y bf16 [rows,d];
 * gamma/beta fp32 [d]; fp32 statistics; y may alias x. */
int visrep_layernorm(const void* x, int ldx, const float* gamma, const float* beta, void* y, int ldy, int rows, int d, float eps,
                     void* stream);

/* ---- LayerNorm folded into a GEMM.  visrep_layernorm_stats only READS x and writes rt[row] = (rstd, -mean * rstd) (float2 per row;
 * allocate round_up(rows, 128) + 8 entries, zero past `rows`); visrep_gemm_bf16_ln then computes, for A = the RAW rows x and
 * W = gamma o W_orig,   C[m, n] = epilogue( rt[m].x * (A W^T)[m, n] + rt[m].y * ln_s[n] + bias[n] )
 * which equals Linear(LayerNorm(x)) when ln_s[n] = sum_k W[n, k] and bias = W_orig beta + b.  epilogue: VISREP_EPI_BIAS, _ACT or _VT.
 * The normalised activations are never written to HBM (the reference materialises them: HF nn.LayerNorm before every
 * attention / MLP block, e.g. modeling_clip.py CLIPEncoderLayer.forward). */
int visrep_layernorm_stats(const void* x, int ldx, void* rt, int rows, int d, float eps, void* stream);
int visrep_gemm_bf16_ln(const void* A, int lda, const void* W, int ldw, const float* bias, const void* ln_rt, const float* ln_s, void* C,
                        int ldc, int M, int N, int K, int epilogue, int act, void* stream);
/* Residual GEMM (VISREP_EPI_RESID of visrep_gemm_bf16) that ALSO leaves the LayerNorm statistics of its output rows in
 * rt[m] = (rstd, -mean * rstd) over the N columns — what the next block's visrep_gemm_bf16_ln consumes, so that LayerNorm never
 * reads the residual stream again (HF blocks: x = x + attn(ln1(x)); x = x + mlp(ln2(x))).  The 256x256 kernel emits per-row partial
 * sums of the bf16-rounded outputs from its epilogue (partial: scratch of M * N / 64 float2) which are reduced in a fixed order;
 * shapes routed elsewhere (split-K, 128x128 tail rows) run visrep_layernorm_stats on the rows they wrote.  N <= 2048. */
/* A GEMM over a periodic subset of A's rows: logical row r reads physical row (r / row_period) * row_stride + r % row_period + row_first
 * (e.g. the patch tokens of every image: period T - 1, stride T, first 1 - the reference's feature_select `[:, 1:]`,
 * clip_encoder.py:37-44 - or the CLS rows: period 1, stride T, first 0) without gathering them first.  ln_rt / ln_s (both or neither):
 * folded LayerNorm, statistics indexed by PHYSICAL row.  Epilogues BIAS, ACT, VT (row_period % 4 == 0), F32.  A folded VT reads the statistics
 * of four consecutive physical rows per 4-token group: when M % 4 != 0 the last group reads up to 3 entries past the last mapped row, so ln_rt
 * needs the same padding as for visrep_gemm_bf16_ln (round_up(physical rows, 128) + 8 entries; their values are never stored). */
int visrep_gemm_bf16_rows(const void* A, int lda, int row_period, int row_stride, int row_first, const void* W, int ldw, const float* bias,
                          const void* ln_rt, const float* ln_s, void* C, int ldc, int M, int N, int K, int epilogue, int act, void* stream);
int visrep_gemm_bf16_resid_stats(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, int M, int N, int K,
                                 const void* resid, const float* ls, void* rt, void* partial, float eps, void* stream);
/* ---- Gated (SwiGLU) GEMM: the GEMM has N = 2 mp columns, the output C [M, mp] (ldc >= mp) bf16:
 *   C[m, 16 t + r] = bf16( silu(g) * u ),  g = (A W^T + bias)[m, 32 t + r],  u = (A W^T + bias)[m, 32 t + 16 + r],  r < 16
 * (g and u in fp32, one rounding).  So row 32 t + r of W / bias / ln_s is the GATE row (HF x1) of hidden unit 16 t + r and row 32 t + 16 + r
 * its VALUE row (x2): the packer interleaves the two halves of Dinov2SwiGLUFFN.weights_in in blocks of 16 rows, which puts both operands of
 * an output element into the same lane of the MFMA accumulators.  ln_rt / ln_s (both or neither): LayerNorm folded as in visrep_gemm_bf16_ln.
 * N % 128 == 0 (mp % 64), K % 64 == 0.  No row map, convolution, row statistics or residual; few-tile problems are not split along K. */
int visrep_gemm_bf16_gated(const void* A, int lda, const void* W, int ldw, const float* bias, const void* ln_rt, const float* ln_s, void* C,
                           int ldc, int M, int N, int K, void* stream);
/* The unfused pair in HF chunk order: y[m, f] = silu(x[m, f]) * x[m, F + f], x [M, 2 F] (ldx), y [M, F] (ldy).  bf16: F, ldx, ldy % 8 == 0;
 * fp32: % 4 (libm expf, as the fp32 towers' activations).  What the fp32 towers and the A/B baseline of the gated epilogue run. */
int visrep_swiglu(const void* x, int ldx, void* y, int ldy, long M, int F, void* stream);
int visrep_swiglu_f32(const float* x, int ldx, float* y, int ldy, long M, int F, void* stream);
/* Per-thread A/B knob: 1 (default) = visrep_vit_forward runs a SwiGLU tower's fc1 as visrep_gemm_bf16_gated (interleaved w1); 0 = as a plain
 * GEMM + visrep_swiglu (w1 / b1 / s1 in HF chunk order; visrep_vit_workspace_bytes grows by the [M, 2 mlp] intermediate - query it with the
 * knob already set).  Returns the previous value. */
int visrep_set_fuse_gate(int on);
/* Tests: hands the GEMM dispatcher a gated problem combined with 1 = a convolution, 2 = an A row map, 3 = row statistics, 4 = GroupNorm
 * partials (placeholder pointers - every one of them must be refused before any launch) and returns the dispatcher's code. */
int visrep_debug_gated_refusal(int which);

/* ---- multi-head self-attention forward (HF CLIPAttention / Dinov2SelfAttention / SiglipAttention: softmax(QK^T
 * scale) V, fp32 softmax).  qk: [B*T, 2*H*head_dim] bf16 (Q | K, head-major columns: K starts at column H*head_dim); vt: V^T as written by
 * visrep_gemm_bf16(..., VISREP_EPI_VT): [H*head_dim, ldvt] with ldvt >= round_up(B*T, 64), % 64 == 0, columns beyond B*T
 * finite; out: [B*T, H*head_dim] bf16.  head_dim must be 64, 96 or 128 (the PADDED width of the buffers: a tower whose heads are 72 or 80
 * wide packs zero rows up to 96, one with 97 .. 128 up to 128; `scale` is the true width's).  scale <= 0 (head_dim 64 only): Q already
 * carries scale * log2(e) (folded into the Q projection by the caller): the kernel computes p = 2^(q.k - reference) with the reference
 * subtracted inside the matrix pipe (accumulator init). */
int visrep_mhsa_fwd(const void* qk, int ldqk, const void* vt, int ldvt, void* out, int ldo, int B, int T, int H, int head_dim,
                    float scale, void* stream);

/* ---- image-aligned self-attention of a CLS tower whose patch count is a multiple of 64 (T = 1 + 64 n: CLIP-L/14-336 577, the 224-px
 * L/14 towers 257), pre-scaled Q only.  qk as for visrep_mhsa_fwd; vt: V^T of the PATCH tokens only, [H*64, ldvt], column
 * b (T - 1) + t - 1 (perm16 inside 16-token blocks, as VISREP_EPI_VT writes it), ldvt >= B (T - 1); vcls: the V rows of the CLS tokens
 * [B, ldvc] row-major.  An image's keys are then whole 64-key tiles (no masks, one tile less per image than the global tiling of
 * visrep_mhsa_fwd) and the CLS key enters as the initial state of the online softmax (m = q.k_cls, l = 1, O = v_cls).
 * visrep_mhsa_cls_supported(T) says whether T qualifies.  Same semantics as visrep_mhsa_fwd(scale <= 0). */
int visrep_mhsa_cls_supported(int T);
int visrep_mhsa_cls_fwd(const void* qk, int ldqk, const void* vt, int ldvt, const void* vcls, int ldvc, void* out, int ldo, int B, int T,
                        int H, int head_dim, void* stream);

/* ---- image-aligned self-attention of a tower with a short PREFIX of NP non-patch tokens in front of 64 n patch tokens (DINOv2 with
 * registers: CLS + 4 registers, T = 5 + 64 n: 261 at 224 px, 581 at 336 px), pre-scaled Q only.  It is visrep_mhsa_cls_fwd with NP side
 * keys instead of one: qk as for visrep_mhsa_fwd; vt: V^T of the PATCH tokens only, [H*64, ldvt], column b (T - NP) + t - NP (perm16
 * inside 16-token blocks), ldvt >= B (T - NP); vpre: the V rows of the prefix tokens [B NP, ldvp] row-major (row b NP + i), ldvp >= H*64.
 * The prefix keys enter as the initial state of the online softmax: s_i = q.k_i, m = max_i s_i, p_i = 2^(s_i - m) kept in fp32, l = sum p_i,
 * O = sum p_i v_i; then (T - NP) / 64 whole key tiles.  With NP = 1 the result equals visrep_mhsa_cls_fwd's bit for bit.
 * visrep_mhsa_prefix_supported(T, NP): 1 <= NP <= 8, T - NP >= 64 and (T - NP) % 64 == 0.  qk and vt 16-byte aligned, vpre and out 8-byte
 * aligned, none null; anything else is refused before any launch. */
int visrep_mhsa_prefix_supported(int T, int NP);
int visrep_mhsa_prefix_fwd(const void* qk, int ldqk, const void* vt, int ldvt, const void* vpre, int ldvp, void* out, int ldo, int B, int T,
                           int NP, int H, int head_dim, void* stream);

/* ---- general multi-head attention forward for the diffusion towers' transformer blocks (vendored diffusers
 * attention_processor.py AttnProcessor2_0 / SlicedAttnProcessor called from attention.py:241-283 BasicTransformerBlock):
 * self-attention (k/vt built from the same tokens, Tk = Tq) and cross-attention to the prompt (Tk = text length).
 * q: [B*Tq, ldq] bf16, head h in columns [h*head_dim, (h+1)*head_dim); k: [B*Tk, ldk] likewise ([Tk, ldk] when
 * kv_shared = 1: one key/value sequence - the prompt - serves every batch item); vt: [H*head_dim, ldvt] as written by
 * VISREP_EPI_VT over the key rows, ldvt >= round_up(key rows, 64); out: [B*Tq, ldo].  head_dim in {64, 96, 128, 192}: the
 * weight packer zero-pads narrower heads (SD1.5: 40 / 80 / 160; SigLIP-so400m 72 and ViT-H/14 80 to 96), which changes nothing in
 * softmax(QK^T)V.  head_dim 96 (attn_fwd96) runs 18 MFMAs per 64-key tile where 128 runs 24 and needs scale > 0.  head_dim 512 (the single head of
 * the diffusion VAE's mid-block attention, AutoencoderKL: 9216 latent pixels at 768 px) runs a wide-head kernel that needs whole key tiles
 * (Tk % 64 == 0), causal = 0 and scale > 0.
 * causal = 1 masks keys after the query position (HF CLIPTextTransformer's causal mask: the prompt encoder behind
 * pipe.encode_prompt, dift_sd.py:258-263).  scale <= 0 (head_dim 64 only): pre-scaled Q, as for visrep_mhsa_fwd.
 * Pointers (all three attention entry points): none may be null; q / qk, k and vt must be 16-byte aligned, out and vcls 8-byte aligned -
 * anything else is refused with VISREP_ERR_ARG before any launch.  Output rows are written with 16-byte stores when ldo % 8 == 0 and out is
 * 16-byte aligned, with 8-byte stores otherwise; the results are bitwise the same.  Nothing outside [row, h * head_dim .. + head_dim) of the
 * B * Tq output rows is written; K rows past the last key row and q / k columns outside the heads are never read.
 * Non-finite data (tests/test_gpu_attention_contract.py): a masked key is not skipped, it enters P.V with weight exactly 0.  Masked SCORES
 * are overwritten, so a NaN / Inf in the Q or K of one image never reaches another image.  A NaN / Inf in image b's V does: where key tiles
 * are the global 64-key blocks (visrep_attention_fwd / visrep_mhsa_fwd with Tk % 64 != 0, keys not shared) the images that share a key
 * tile with the bad key - b - 1 and / or b + 1 - get 0 * NaN = NaN in that head's column, while softmax(QK^T)V keeps it inside image b.
 * Every other image, and every image when all data are finite, is bitwise independent of its neighbours.  V^T columns that belong to no
 * key must be finite for the same reason. */
int visrep_attention_fwd(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* out, int ldo, int B, int Tq,
                         int Tk, int H, int head_dim, int kv_shared, int causal, float scale, void* stream);

/* ---- patch embedding pieces (HF CLIPVisionEmbeddings / Dinov2Embeddings / SiglipVisionEmbeddings) */
/* visrep_im2col: cols [B * (Himg / patch) * (Wimg / patch), Kpad] bf16, k = c p p + i p + j.  The grid is floor(side / patch), as
 * Conv2d(kernel = stride = patch) gives it: the trailing Himg % patch rows and Wimg % patch columns are never read (384 / 14 = 27 patches,
 * 6 pixels unused).  Since 620; before, a side that was not a multiple of the patch was refused. */
int visrep_im2col(const void* pixels, int pixel_dtype, void* cols, int B, int Himg, int Wimg, int patch, int Kpad, void* stream);
int visrep_cls_rows(void* x, int ldx, const float* cls, const float* pos, int B, int T, int d, void* stream);
/* the same for a prefix of `prefix` non-patch rows per image: x[b T + r] = table[r] + pos[r], r < prefix (table: [prefix, d], see
 * visrep_vit_weights.cls).  prefix = 1 is visrep_cls_rows. */
int visrep_prefix_rows(void* x, int ldx, const float* table, const float* pos, int B, int T, int prefix, int d, void* stream);
int visrep_cast_f32_bf16(const float* src, void* dst, long n, void* stream);

/* ---- composed tower forward: replaces `self.vision_tower(images, output_hidden_states=True).hidden_states[k]`
 * (clip_encoder.py:48-49, dinov2_encoder.py:51-52, siglip_encoder.py:49-50). */
typedef struct {
    int image_size, patch, d, heads, mlp, layers, tokens, has_cls, pre_ln, act, kpad;
    float eps;
    /* 1: the Q rows of wqkv (and of bqkv) carry head_dim^-0.5 * log2(e) - folded in by the weight packer (the bf16 engine does it while it
     * folds LayerNorm: same single rounding of the fp32 product) - and the attention kernel exponentiates the raw scores (visrep_mhsa_fwd
     * with scale <= 0).  2: as 1, and towers with a CLS token and 64 n patches use the image-aligned kernel (visrep_mhsa_cls_fwd: V
     * projected by two row-mapped GEMMs, patch rows -> V^T, CLS rows -> [B, d]); other shapes behave as 1.  bf16 tower only; the fp32
     * towers ignore it. */
    int q_prescaled;
    /* bf16 tower only (the fp32 and host towers use d / heads).  head_dim: the true head width d / heads (0 = d / heads), what the softmax
     * scale head_dim^-0.5 is taken from.  head_pad: the width every head occupies in wqkv's q / k / v rows and in wo's columns, zero-padded
     * by the packer (0 = head_dim): 64, 96 or 128, >= head_dim.  wqkv is then [3 * heads * head_pad, d] (Q | K | V blocks of heads * head_pad
     * rows), bqkv / sqkv [3 * heads * head_pad], wo [d, heads * head_pad].  head_pad != 64 needs q_prescaled = 0.  `mlp` is the PADDED MLP
     * width the w1 / b1 / s1 / w2 arrays have (zero rows / columns past the true width), a multiple of 128. */
    int head_dim, head_pad;
    /* register tokens between the CLS row and the patch rows (HF Dinov2WithRegisters: num_register_tokens; needs has_cls).  tokens =
     * grid^2 + has_cls + registers; token rows of an image: CLS, the registers, the patches.  0 = every tower before 640, unchanged.
     * With q_prescaled == 2 and 64 n patches such a tower (prefix = 1 + registers <= 8) runs visrep_mhsa_prefix_fwd. */
    int registers;
    /* norm: the two pre-block norms - 0 = nn.LayerNorm (every tower before 650), 1 = RMSNorm (HF InternVLVisionRMSNorm: x * rsqrt(mean(x^2) + eps)
     * * ln*_g, no bias; ln*_b are ignored; d <= 4096; pre_ln is refused).  The folded route is the same GEMM epilogue fed with statistics
     * (rstd, 0).  qk_norm != 0: an RMSNorm over the WHOLE width (all heads, before the head split; eps VISREP_QK_NORM_EPS) is applied to the
     * Q and to the K projection's output with the layer's qn_g / kn_g (visrep_qk_rmsnorm between the Q|K GEMM and the attention kernel).  With
     * q_prescaled != 0 the packer folds head_dim^-0.5 * log2(e) into qn_g, NOT into the Q rows of wqkv / bqkv.  Both 0 = unchanged launches. */
    int norm, qk_norm;
} visrep_vit_config;
#define VISREP_QK_NORM_EPS 1e-6f   /* HF InternVLVisionAttention: q_norm / k_norm are built with the RMSNorm class default, not layer_norm_eps */
typedef struct {           /* device pointers; matrices bf16 [out,in], vectors fp32; ls1/ls2 NULL when no LayerScale */
    const float *ln1_g, *ln1_b; const void* wqkv; const float* bqkv; const void* wo; const float* bo; const float* ls1;
    const float *ln2_g, *ln2_b; const void* w1; const float* b1; const void* w2; const float* b2; const float* ls2;
    /* LayerNorm folded into the consuming GEMMs (both non-NULL to enable; ln*_g / ln*_b are then unused): wqkv = gamma1 o Wqkv and
     * bqkv = Wqkv beta1 + b (likewise w1 / b1 with LN2), sqkv[n] = sum_k wqkv[n, k] over the bf16-rounded rows [3d], s1 [mlp]. */
    const float *sqkv, *s1;
    /* qk_norm towers: the RMSNorm weights behind q_proj / k_proj.  bf16 tower: [heads * head_pad], zero in the padded columns; fp32 and host
     * towers: [d].  NULL otherwise. */
    const float *qn_g, *kn_g;
} visrep_vit_layer;
typedef struct {
    const void* patch_w;   /* bf16 [d, kpad], zero padded past 3*p*p */
    /* patch_b / cls / pre_ln_* may be NULL.  cls: [d], or for a tower with registers the table [1 + registers, d] of the non-patch rows (the
     * class token, then the register tokens); pos: [tokens, d] in token-row order - a register tower's rows 1 .. registers are ZERO (HF
     * adds the position embedding before it inserts the registers), so that row r of the embedding is cls[r] + pos[r] for every prefix row. */
    const float *patch_b, *cls, *pos, *pre_ln_g, *pre_ln_b;
    const visrep_vit_layer* layers;   /* HOST array of `layers` entries */
} visrep_vit_weights;
size_t visrep_vit_workspace_bytes(const visrep_vit_config* cfg, int B);
/* hidden: [B, tokens, d] bf16 — receives hidden_states[n_layers] (the residual stream lives in it). */
int visrep_vit_forward(const visrep_vit_config* cfg, const visrep_vit_weights* w, const void* pixels, int pixel_dtype, void* hidden,
                       int B, int n_layers, void* workspace, void* stream);

/* ---- RMSNorm (HF InternVLVisionRMSNorm; rowops.hip).  One wave per row, fp32 sum of squares, d % 8 == 0, d <= 4096, ldx / ldy % 8 == 0,
 * 16-byte aligned pointers (gamma included); refused before any launch otherwise.
 * visrep_rmsnorm: y = x * rsqrt(mean(x^2) + eps) * gamma, rounded once to bf16; y may alias x.
 * visrep_rmsnorm_stats: rt[row] = (rsqrt(mean(x^2) + eps), 0) - the (rstd, -mean * rstd) pair of visrep_layernorm_stats with an exact zero
 * second term, so that visrep_gemm_bf16_ln computes Linear(RMSNorm(x)) from W = gamma o W_orig unchanged (ln_s must be finite).
 * visrep_gemm_bf16_resid_rms_stats: visrep_gemm_bf16_resid_stats leaving that pair for its output rows (N <= 4096).
 * visrep_qk_rmsnorm: in place on qk [rows, ldqk] = the Q|K GEMM's output, Q in columns [0, width), K in [width, 2 width), width = heads *
 * head_pad <= 4096, % 8 == 0; ldqk % 8 == 0, >= 2 width.  Each half of each row: x * rsqrt(sum(x^2) / d_true + eps) * g[c] in fp32, one
 * rounding to bf16; g = qn_g for Q, kn_g for K ([width] fp32; zero in padded columns, which therefore stay zero).  d_true = heads * head_dim
 * (0 < d_true <= width): zero-padded columns add nothing to the sum and must not count in the mean.  Nothing outside the 2 width columns
 * of the `rows` rows is written.  Memory-bound: reads and writes 4 * rows * width bytes. */
int visrep_rmsnorm(const void* x, int ldx, const float* gamma, void* y, int ldy, int rows, int d, float eps, void* stream);
int visrep_rmsnorm_stats(const void* x, int ldx, void* rt, int rows, int d, float eps, void* stream);
int visrep_qk_rmsnorm(void* qk, int ldqk, int width, int d_true, const float* qn_g, const float* kn_g, int rows, float eps, void* stream);
int visrep_gemm_bf16_resid_rms_stats(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, int M, int N, int K,
                                     const void* resid, const float* ls, void* rt, void* partial, float eps, void* stream);
/* fp32 forms (device pointers, any d / width that is a multiple of 4) and host twins (HOST pointers, fp32, double-precision sums) */
int visrep_rmsnorm_f32(const float* x, int ldx, const float* gamma, float* y, int ldy, int rows, int d, float eps, void* stream);
int visrep_qk_rmsnorm_f32(float* qk, int ldqk, int width, int d_true, const float* qn_g, const float* kn_g, int rows, float eps, void* stream);
int visrep_rmsnorm_cpu(const float* x, int ldx, const float* gamma, float* y, int ldy, long rows, int d, float eps, int threads);
int visrep_rmsnorm_stats_cpu(const float* x, int ldx, float* rt, long rows, int d, float eps, int threads);
int visrep_qk_rmsnorm_cpu(float* qk, int ldqk, int width, int d_true, const float* qn_g, const float* kn_g, long rows, float eps, int threads);

/* ---- ConvNeXt towers (HF ConvNextModel; OpenCLIP's timm ConvNeXt trunks).  A block is
 *   x + ls * pwconv2(GELU(pwconv1(LayerNorm(dwconv7x7(x)))))
 * on channels-last token rows (row = (b H + y) W + x): visrep_dwconv7x7_stats, then visrep_gemm_bf16_ln (VISREP_EPI_ACT, VISREP_ACT_GELU_ERF)
 * on the raw convolution output with the statistics it left, then visrep_gemm_bf16 (VISREP_EPI_RESID, ls).  The normalised tensor is never written.
 *
 * visrep_dwconv7x7_stats: y[b, oy, ox, c] = bf16( bias[c] + sum_{ky, kx} wt[ky * 7 + kx, c] * x[b, oy + ky - 3, ox + kx - 3, c] ), zero outside the
 * image (padding 3), cross-correlation as nn.Conv2d(groups = C) computes it; fp32 fused multiply-adds in tap order starting from the bias, one
 * rounding.  x, y: [B, H, W, C] bf16 with leading dimensions ldx, ldy >= C (% 8 == 0; columns past C are neither read nor written); wt [49, C]
 * fp32, tap-major; bias [C] fp32.  The same pass writes, for every output row and every slab of 64 channels, (sum, sum of squares) of the
 * bf16-ROUNDED outputs into partial [B H W, C / 64] float2, and a second launch reduces them in slab order to rt[row] = (rstd, -mean * rstd)
 * with var = E[x^2] - mean^2 in fp32 - the pair visrep_gemm_bf16_ln consumes (allocate round_up(rows, 128) + 8 entries, zero past the rows).
 * C % 64 == 0; any H, W >= 1 (maps smaller than the window included), any B; a tile never reads across an image boundary.  y must not alias x.
 * x, wt, bias, y 16-byte aligned.  Anything else is refused before any launch (VISREP_ERR_SHAPE / VISREP_ERR_ARG).
 * visrep_ln_space_to_depth2: out[(b (H/2) + oy) (W/2) + ox, (i * 2 + j) * C + c] = bf16( LayerNorm(x[b, 2 oy + i, 2 ox + j, :])[c] ), the rows of
 * a 2x2 stride-2 convolution's GEMM (weight [Cout, 4 C] in the same k order).  x [B, H, W, C] bf16 (ldx >= C), gamma / beta [C] fp32, out bf16
 * (ldo >= 4 C).  H and W even; C % 8 == 0, C <= 4096; 16-byte aligned pointers; out must not alias x (x stays intact: it is a hidden state).
 * The _cpu forms are host twins with the same contract on HOST pointers (bf16 storage in and out, the same fmaf chain; sums of the statistics
 * in double) - threads <= 0: a default. */
int visrep_dwconv7x7_stats(const void* x, int ldx, const float* wt, const float* bias, void* y, int ldy, void* partial, void* rt, int B, int H,
                           int W, int C, float eps, void* stream);
int visrep_ln_space_to_depth2(const void* x, int ldx, const float* gamma, const float* beta, void* out, int ldo, int B, int H, int W, int C,
                              float eps, void* stream);
int visrep_dwconv7x7_stats_cpu(const void* x, int ldx, const float* wt, const float* bias, void* y, int ldy, float* rt, int B, int H, int W, int C,
                               float eps, int threads);
int visrep_ln_space_to_depth2_cpu(const void* x, int ldx, const float* gamma, const float* beta, void* out, int ldo, int B, int H, int W, int C,
                                  float eps, int threads);
/* Composed tower: hidden_states[n_stages] of HF ConvNextModel(output_hidden_states=True) - index 0 = the stem (4x4 stride-4 convolution +
 * LayerNorm), 1 .. 4 = the stage outputs - as token rows [B, H_s W_s, C_s] bf16 (H_s = image / 4 for index 0 and 1, halved per later stage).
 * widths[s] % 64 == 0; wp(s) = widths[s] rounded up to 128 is the width of the GEMM OUTPUTS (the residual stream's leading dimension): stem_w
 * [wp(0), kpad] (k = c 16 + i 4 + j, zero past 48), ds_w[s] [wp(s), 4 widths[s - 1]] (k = (i 2 + j) C + c), w2 [wp, 4 C], and stem_b / ds_b / b2 /
 * ls [wp], all zero in the padded rows; w1 [4 C, C] = gamma o W with s1[n] = its row sums and b1 = W beta + b (the block LayerNorm folded, as for
 * the ViT blocks); dw_w [49, C], dw_b [C].  ls may be NULL (no LayerScale).  ds_*[0] are unused.  image_size % 32 == 0.  bf16 only. */
typedef struct {
    int image_size, kpad;
    int depths[4], widths[4];
    float eps;
} visrep_convnext_config;
typedef struct {
    const float *dw_w, *dw_b; const void* w1; const float *b1, *s1; const void* w2; const float *b2, *ls;
} visrep_convnext_block;
typedef struct {
    const void* stem_w; const float *stem_b, *stem_ln_g, *stem_ln_b;
    const float *ds_ln_g[4], *ds_ln_b[4]; const void* ds_w[4]; const float* ds_b[4];
    const visrep_convnext_block* blocks;   /* HOST array of depths[0] + .. + depths[3] entries, stage by stage */
} visrep_convnext_weights;
size_t visrep_convnext_workspace_bytes(const visrep_convnext_config* cfg, int B);
int visrep_convnext_forward(const visrep_convnext_config* cfg, const visrep_convnext_weights* w, const void* pixels, int pixel_dtype, void* hidden,
                            int B, int n_stages, void* workspace, void* stream);

/* ---- SAM ViT towers (HF SamVisionModel / the Segment Anything image encoder, ViTDet style): attention whose logits carry the decomposed
 * relative-position term, over 14 x 14 windows of the patch grid in most layers and over the whole grid in a few.
 *
 * visrep_mhsa_relpos_fwd replaces SamVisionAttention.forward from `attn_weights = (query * self.scale) @ key.transpose(-2, -1)` through
 * add_decomposed_rel_pos's `attn + rel_h[:, :, :, :, None] + rel_w[:, :, :, None, :]`, the fp32 softmax and `attn_probs @ value`:
 *   out[g, q, h, :] = softmax_k( scale * Q[g,q,h,:] . K[g,k,h,:] + rel_h[g,h,q, k / S] + rel_w[g,h,q, k % S] ) V[g,k,h,:]
 * over NB independent S x S token grids (T = S S tokens each; NB = batch x windows, or the batch for a global layer).  qk [NB T, ldqk] bf16
 * (Q | K, head-major, K at column H 64), vt [H 64, ldvt] as VISREP_EPI_VT writes it over the NB T key rows (ldvt >= round_up(NB T, 64),
 * % 64 == 0, columns that belong to no key finite), out [NB T, ldo] bf16; rel_h, rel_w: fp32 [NB, H, T, S], taken as given (fp32 on purpose:
 * a bf16 table would put 2^-9 |bias| straight into the logits).  scale > 0 only: Q is the UNSCALED query (the position term uses it), so
 * there is no pre-scaled-Q form.  Rounding sequence per logit, all fp32: s = the MFMA's q.k; b = rel_h + rel_w; t = fma(s, scale log2 e,
 * b log2 e); p = exp2(t - m) with m the running reference (first tile's row maximum, moved when a later tile's exceeds it by more than 8);
 * the row sum adds the fp32 p, P.V takes p rounded to bf16, one bf16 rounding of O / l.  2 <= S <= 64, head_dim 64.  No scratch memory.
 * Pointers: none null; qk and vt 16-byte, out 8-byte, rel_h and rel_w 4-byte aligned; ldqk % 8, ldvt % 64, ldo % 4 - anything else is
 * refused (VISREP_ERR_ARG / VISREP_ERR_SHAPE) before any launch.  Nothing outside [row, h 64 .. + 64) of the NB T output rows is written;
 * K rows past the last key row, qk columns outside the heads and table entries of other (grid, head)s are never read.
 * Non-finite data, in the terms of the attention contract above: key tiles are the global 64-key blocks, so a key outside the grid is not
 * skipped - its score is overwritten with -inf and it enters P.V with weight exactly 0.  A NaN / Inf in the Q, K or tables of one grid never
 * reaches another grid (a table row belongs to one query); a NaN / Inf in grid g's V reaches the grids that share a key tile with the bad
 * key (g - 1 and / or g + 1: 0 * NaN) and no other.  With finite data every grid is bitwise independent of its neighbours' contents; its
 * result depends on its own data and on g T % 64 (where the tile boundaries fall inside it).
 *
 * visrep_relpos_tables replaces get_rel_pos + the two einsums of get_decomposed_rel_pos ("bhwc,hkc->bhwk", "bhwc,wkc->bhwk"):
 *   rel_h[g, h, q, kh] = sum_c Q[g T + q, h 64 + c] * Rh[q / S - kh + S - 1, c],   rel_w[g, h, q, kw] likewise with Rw and q % S - kw,
 * Q = the first H 64 columns of the rows of qk (bf16, ldqk % 8 == 0, 16-byte aligned), Rh / Rw fp32 [2 S - 1, 64] (16-byte aligned; a table
 * of another length is refused by the weight packer).  Summation order: ONE fp32 fmaf chain over c = 0, 1, .. 63
 * starting from +0 - the host twin runs the same chain and equals the kernel bit for bit.
 *
 * visrep_sam_window_partition / _unpartition replace window_partition / window_unpartition of SamVisionLayer together with the zero
 * padding in front of the QKV projection: the PROJECTED tokens are gathered.  Window row r = ((b nw + wy) nw + wx) w w + iy w + ix holds map
 * token (b, wy w + iy, wx w + ix), nw = ceil(g / w); a position past the map's bottom or right edge holds bf16(bias) - what qkv(0) is: bias
 * [3 d] fp32 is the RAW qkv bias (q | k | v), not the folded one.  qk [B g g, ldqk] -> qk_win [B nw nw w w, ldqw] (2 d columns), vt
 * [d, ldvt] -> vt_win [d, ldvw] (column perm16(row) on both sides).  unpartition copies the d columns of every map token's window row and
 * drops the pad rows.  d % 8 == 0; row pointers 16-byte aligned.
 * The _cpu forms are host twins on HOST pointers: plain C++ fp32 (float64 for the softmax sums), the same contract. */
int visrep_mhsa_relpos_fwd(const void* qk, int ldqk, const void* vt, int ldvt, const float* rel_h, const float* rel_w, void* out, int ldo, int NB,
                           int S, int H, int head_dim, float scale, void* stream);
int visrep_relpos_tables(const void* qk, int ldqk, const float* Rh, const float* Rw, float* rel_h, float* rel_w, int NB, int S, int H, int head_dim,
                         void* stream);
int visrep_sam_window_partition(const void* qk, int ldqk, const void* vt, int ldvt, const float* bias, void* qk_win, int ldqw, void* vt_win, int ldvw,
                                int B, int g, int window, int d, void* stream);
int visrep_sam_window_unpartition(const void* win, int ldw, void* out, int ldo, int B, int g, int window, int d, void* stream);
/* Host twins.  visrep_mhsa_relpos_cpu: q, k, v [NB T, ld*] fp32 ROW-major (v is not transposed), out fp32; the softmax of
 * scale q.k + rel_h + rel_w in fp32 logits and float64 sums, no bf16 rounding anywhere. */
int visrep_mhsa_relpos_cpu(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* rel_h, const float* rel_w, float* out,
                           int ldo, int NB, int S, int H, int head_dim, float scale, int threads);
int visrep_relpos_tables_cpu(const void* qk, int ldqk, const float* Rh, const float* Rw, float* rel_h, float* rel_w, int NB, int S, int H, int head_dim,
                             int threads);
/* Composed tower: state `n_state` of HF SamVisionModel(output_hidden_states=True) as token rows - 0 = patch embedding + absolute positions,
 * 1 .. layers = the block outputs [B, g g, d], layers + 1 = the neck output [B, g g, out_ch] (conv1x1 -> LayerNorm over channels -> conv3x3
 * -> LayerNorm over channels).  A block is x + attn(LN1(x)) then x + fc2(GELU(fc1(LN2(x)))); layer l attends over the whole grid when bit l
 * of global_mask is set, over window x window windows otherwise.  Composition: visrep_im2col + GEMM (EPI_PATCH); folded-LayerNorm Q | K and
 * V GEMMs over the UNPADDED tokens; windowed layers: visrep_sam_window_partition (pad rows = the raw bias bqkv_raw); visrep_relpos_tables +
 * visrep_mhsa_relpos_fwd in chunks of images such that each table stays within its 64 MiB of the workspace (as many images as fit, at
 * least one; a chunk is a range of grids of the same buffers, so the result does not depend on the chunk size); unpartition; the residual GEMMs with LayerNorm
 * statistics; fc1 with exact GELU; fc2.  The neck: plain
 * GEMM, visrep_layernorm, visrep_conv3x3_bf16, visrep_layernorm.  wqkv / bqkv / sqkv and w1 / b1 / s1 are the folded forms (as the ViT
 * blocks'); rel_h / rel_w fp32 [2 S - 1, 64] with S = window or g.  d, mlp % 128 == 0, out_ch % 64 == 0, heads 64 wide, kpad % 64 == 0. */
typedef struct {
    int image_size, patch, d, layers, heads, mlp, window, out_ch, kpad;
    unsigned long long global_mask;
    float eps, neck_eps;
} visrep_sam_config;
typedef struct {
    const void* wqkv; const float *bqkv, *sqkv, *bqkv_raw, *rel_h, *rel_w; const void* wo; const float* bo;
    const void* w1; const float *b1, *s1; const void* w2; const float* b2;
} visrep_sam_layer;
typedef struct {
    const void* patch_w; const float *patch_b, *pos;
    const void* neck_w1; const float *neck_ln1_g, *neck_ln1_b; const void* neck_w2; const float *neck_ln2_g, *neck_ln2_b;
    const visrep_sam_layer* layers;         /* HOST array of `layers` entries */
} visrep_sam_weights;
size_t visrep_sam_workspace_bytes(const visrep_sam_config* cfg, int B);
/* Tests: the per-table budget (bytes) the calling thread's visrep_sam_forward sizes its image chunks to, so that a small tower reaches the
 * chunked path; 0 = the default (64 MiB, also the most: the workspace holds that much).  Returns the previous value.  Results do not depend
 * on it. */
size_t visrep_debug_sam_table_bytes(size_t bytes);
int visrep_sam_forward(const visrep_sam_config* cfg, const visrep_sam_weights* w, const void* pixels, int pixel_dtype, void* hidden, int B,
                       int n_state, void* workspace, void* stream);

/* ---- reference-precision (fp32) tower path.  The reference builds the C-score CLIP / OpenCLIP / DINOv2 towers with no dtype cast and
 * fp32 pixels (C_score/extract_feature.py:36-45,49-50,80-87): every tensor and accumulation here is fp32 (v_mfma_f32_32x32x2_f32 = an
 * exact fmaf chain, 157 TFLOP/s peak), so images -> tower -> A / C scores can be held to the 1e-4 bar against the fp32 reference
 * chain.  A parity mode, ~1/20 of the bf16 engine's rate.
 * visrep_gemm_f32: C = epi(alpha * A W^T + bias); A [M,K] (lda), W [N,K] (w_kn = 0, nn.Linear) or [K,N] (w_kn = 1), all fp32, rows
 * 16-byte aligned (pointers, leading dimensions, batch strides % 4 floats); epilogue BIAS / ACT / RESID (C = resid + ls * (..), resid
 * may alias C).  Batched over nb1 x nb2 problems with element strides strides6 = {A1, A2, W1, W2, C1, C2} (NULL when nb1 = nb2 = 1):
 * replaces torch.matmul(q, k.transpose) / torch.matmul(attn, v) of HF's eager attention as well as F.linear. */
int visrep_gemm_f32(const float* A, int lda, const float* W, int ldw, int w_kn, const float* bias, float* C, int ldc, int M, int N, int K,
                    int epilogue, int act, const float* resid, const float* ls, float alpha, int nb1, int nb2, const long* strides6,
                    void* stream);
/* nn.LayerNorm in fp32 (two-pass variance); y may alias x */
int visrep_layernorm_f32(const float* x, int ldx, const float* g, const float* b, float* y, int ldy, int rows, int d, float eps, void* stream);
/* in-place softmax over the first `cols` entries of every row (ld >= cols) */
int visrep_softmax_rows_f32(float* x, int ld, long rows, int cols, void* stream);
/* composed fp32 forward = visrep_vit_forward with fp32 pixels, fp32 MATRICES in the weight struct (sqkv / s1 ignored) and an fp32
 * hidden [B, tokens, d]; any head width that is a multiple of 4. */
size_t visrep_vit_f32_workspace_bytes(const visrep_vit_config* cfg, int B);
int visrep_vit_forward_f32(const visrep_vit_config* cfg, const visrep_vit_weights* w, const float* pixels, float* hidden, int B, int n_layers,
                           void* workspace, void* stream);
/* ---- fp32 on the bf16 matrix pipe ("split-bf16"): an fp32 value x is carried as bf16 planes hi = bf16(x), mid = bf16(x - hi),
 * lo = bf16(x - hi - mid) (the subtractions are exact; two planes hold 16 significand bits, three hold 24) and a product sum runs over
 * `products` plane pairs, accumulated in fp32 by v_mfma_f32_16x16x32_bf16:
 *   6 = (hi,hi) (hi,mid) (hi,lo) (mid,hi) (mid,mid) (lo,hi): every term >= 2^-24 of the result; differs from the exact fp32 result by ~1e-7
 *       relative - below the rounding of an fp32 FMA chain - at 16/6 of the exact-fp32 MFMA rate;
 *   4 = the full product of two-plane operands; 3 = (hi,hi) (hi,mid) (mid,hi): terms below 2^-16 dropped, ~4e-6 relative per product sum
 *       (between TF32 and fp32), at 16/3 of the exact-fp32 rate; accuracy against A / PCK in profiles/round4_precision.md.
 * The reference-precision towers (C_score/extract_feature.py:36-45: CLIP / OpenCLIP / DINOv2 in fp32) run their projections this way;
 * tests/test_gpu_f32.py holds the route to the same bars as the exact-fp32 one. */
/* planes [rows, nplanes K] bf16 = hi | mid [| lo] of x fp32 [rows, K] (ldx floats per row); nplanes 2 | 3; K, ldx % 4 == 0 */
int visrep_split_bf16_planes(const float* x, int ldx, long rows, int K, int nplanes, void* planes, void* stream);
/* C [M, N] fp32 (ldc; may be NULL) and / or out_planes [M, npl N] (may be NULL) = epilogue(A W^T): v = act(A W^T + bias);
 * v = resid + ls * v when resid != NULL (resid fp32 [M, ldc], may alias C; ls [N] or NULL = 1).  products 3 | 4 | 6; npl = 3 for 6 products,
 * else 2; a_planes [M, npl K], w_planes [N, npl K] from visrep_split_bf16_planes; N % 256 == 0, K % 64 == 0; act = VISREP_ACT_* evaluated
 * with libm expf / erff / tanhf. */
int visrep_gemm_f32_split(const void* a_planes, const void* w_planes, int M, int N, int K, int products, const float* bias, int act,
                          const float* resid, const float* ls, float* C, int ldc, void* out_planes, void* stream);
/* 1 when visrep_vit_forward_f32_split takes this tower (d, mlp % 256 == 0, head width 64, norm == 0 and qk_norm == 0: RMSNorm / QK-norm towers
 * take the exact-fp32 route) */
int visrep_vit_f32_split_supported(const visrep_vit_config* cfg);
/* visrep_vit_forward_f32 with the projections and the attention as split-bf16 products.  w: the fp32 weights (vectors, patch matrix); wsplit:
 * same struct whose wqkv / wo / w1 / w2 point to the planes [N, npl K] of the fp32 matrices (other fields ignored); products as above.
 * Same workspace size. */
int visrep_vit_forward_f32_split(const visrep_vit_config* cfg, const visrep_vit_weights* w, const visrep_vit_weights* wsplit, int products,
                                 const float* pixels, float* hidden, int B, int n_layers, void* workspace, void* stream);
/* Per-thread diagnostic of the fp32 towers' attention (tests only): bit 0 = three-launch attention (batched Q K^T -> softmax rows -> P V
 * through HBM) on the exact route; bit 1 = exact-fp32 MFMA attention inside the split route.  Returns the previous mask. */
int visrep_debug_f32_attention(int mask);

/* ---- fp32 convolution-block primitives of the supervised C-score post-processor (C_score/model_utils/projection_network.py:15-125
 * AggregationNetwork = detectron2-style BottleneckBlocks, model_utils/resnet.py:174-286: 1x1 / 3x3 / 1x1 bias-free convolutions, each
 * followed by nn.GroupNorm, ReLU, projection shortcut).  Tokens are channels-last fp32 [B, H*W, C]; a 1x1 convolution is visrep_gemm_f32,
 * a 3x3 one visrep_im2col3x3_f32 (pad 1, stride 1; column order (ky, kx, c)) + visrep_gemm_f32 on weights repacked [Cout, 9 C];
 * visrep_groupnorm_f32: y = alpha * act(GN(x) * gamma + beta + resid) (+ y when accumulate), resid may be NULL, relu 0 / 1. */
int visrep_im2col3x3_f32(const float* x, float* cols, int B, int H, int W, int C, void* stream);
int visrep_groupnorm_f32(const float* x, const float* gamma, const float* beta, const float* resid, float* y, int B, int HW, int C, int groups,
                         float eps, int relu, float alpha, int accumulate, void* stream);

/* ---- ADAPT_FLIP support of the C score (C_score/pck_train.py:111-126 with MUTUAL_NN; utils/utils_correspondence.py:54-73
 * get_distance_mutual_nn): raw Gram matrices of image pairs from a position-major fp32 bank [n_images, PP, C] (gather by index),
 * normalize_feats' row factors r = 1 / (|x| + eps) (pck_train.py:24-29), and per pair the mean cdist of the mutual nearest neighbours
 * of the two L2-normalised descriptor sets: out[z] fp32 (nan when a pair has none, like torch's empty mean).  gram [n_pairs, PP, PP],
 * r1 / r2 [n_pairs, PP] (the factors of each pair's source / target map, eps = the epsilon they were built with), PP <= 4096
 * (60 x 60 maps). */
int visrep_gram_pairs_f32(const float* bank, const int* idx1, const int* idx2, int n_pairs, int PP, int C, float* gram, void* stream);
int visrep_row_rnorm_f32(const float* x, long rows, int C, float eps, float* r, void* stream);
int visrep_mutual_nn_distance(const float* gram, const float* r1, const float* r2, int n_pairs, int PP, float eps, float* out, void* stream);
/* ADAPT_FLIP WITHOUT MUTUAL_NN (C_score/pck_train.py:122-124 -> utils/utils_correspondence.py:22-52 get_distance, the mask-based flip
 * distance; round 6): the search of lines 41-50 - for every source cell (row of src [ns, C]: the cells inside the source mask) the squared
 * Euclidean distance to the nearest of the nt target cells (rows of tgt [nt, C]), difference first as the reference computes it (its operands
 * hold -100000 where a mask or an exact zero was), -> min_d2 [ns] fp32.  The resize / mask / substitution steps of lines 23-37 are the host
 * side's (cscore_ops.masked_nn_distance); the mean of sqrt(min_d2) is the reference's return value.  C % 4 == 0. */
int visrep_masked_nn_min_f32(const float* src, const float* tgt, int ns, int nt, int C, float* min_d2, void* stream);

/* ---- JPEG decode for the device input pipeline.  Replaces PIL's Image.open(path).convert('RGB') of the reference's
 * image loaders (C_score/extract_feature.py:65-66, llava/mm_utils.py:78-95, llava/feature/extract.py:198-214) bit for bit; what PIL runs
 * underneath is libjpeg-turbo's default decode (jidctint.c islow IDCT, jdsample.c fancy upsampling, jdcolor.c ycc_rgb_convert).
 * HOST: visrep_jpeg_info parses the headers (rc != 0: not a decodable JPEG stream; rc == 0 and info->unsupported != 0: a valid file this
 * decoder does not take - progressive, arithmetic, 12-bit, CMYK, multi-scan, unusual chroma layouts - visrep_last_error() says which; the
 * Python side lets PIL decode such a file).  visrep_jpeg_entropy_decode: baseline Huffman decode into QUANTISED coefficients, int16,
 * natural 8x8 order, component planes of whole MCUs one after the other (info->coef_count values), and the components' quantisation
 * tables qtab[ncomp][64] (natural order).  Both run on the calling host thread, thread-safe, no GPU needed.
 * DEVICE: visrep_jpeg_reconstruct turns a BATCH of decoded images into packed RGB u8 [H, W, 3] each: dequantisation + islow IDCT into
 * the `planes` scratch, then fancy chroma upsampling + YCbCr -> RGB.  desc: n_images x 32 int64 (device) - coefficient / plane offsets
 * per component, block grid, component and image sizes, offsets of the image's RGB output and quantisation tables
 * (law_of_vision_representation_in_mllms_amd/device_jpeg.py builds it); max_blocks / max_pixels: the largest image's. */
typedef struct VisrepJpegInfo {
    int width, height, ncomp;          /* ncomp 1 (grey) or 3 (YCbCr) */
    int hs[3], vs[3], hmax, vmax;      /* sampling factors */
    int mcus_w, mcus_h;
    int blocks_w[3], blocks_h[3];      /* block grid per component (whole MCUs) */
    int comp_w[3], comp_h[3];          /* real samples per component (jdmaster.c downsampled_width / height) */
    int restart_interval, progressive, unsupported;
    long coef_count;
} VisrepJpegInfo;
int visrep_jpeg_info(const void* data, size_t n, VisrepJpegInfo* info);
int visrep_jpeg_entropy_decode(const void* data, size_t n, int16_t* coef, uint16_t* qtab);
int visrep_jpeg_reconstruct(const void* coef, const void* qtab, const void* desc, int n_images, long max_blocks, long max_pixels,
                            void* planes, void* rgb, void* stream);

/* ---- A score (A_score/compute.py:12-15,54-72): scores[img] = mean_t max_s cos(other[img][t], ref[img][s]).
 * other [n_img,Nt,D], ref [n_img,Nr,D] contiguous, dtype VISREP_BF16 (D%16==0) or VISREP_F32 (D%8==0);
 * scores fp32 [n_img]; workspace of visrep_ascore_workspace_bytes(). */
size_t visrep_ascore_workspace_bytes(int n_img, int Nt, int Nr);
int visrep_ascore_maxcos(const void* other, const void* ref, int n_img, int Nt, int Nr, int D, int dtype, float* scores,
                         void* workspace, void* stream);
/* The per-row factor of the two normalisations (normalize_feat's 1/(|x|+1e-10) and F.cosine_similarity's eps clamp, compute.py:12-15,
 * 64-65), scale[rows] fp32 — and the score with factors computed earlier (NULL = compute here, as visrep_ascore_maxcos does).  The
 * reference re-normalises the clip336 / clip224 reference sets for every encoder and every encoder's tokens once per reference
 * (compute.py:54-56 inside the loops); computed once per tensor instead, the norm passes drop from 29 % of the A score's kernel time. */
int visrep_ascore_row_scale(const void* x, long rows, int D, int dtype, float* scale, void* stream);
int visrep_ascore_maxcos_scaled(const void* other, const void* ref, const float* other_scale, const float* ref_scale, int n_img, int Nt,
                                int Nr, int D, int dtype, float* scores, void* workspace, void* stream);

/* The A score in the REFERENCE'S OWN ARITHMETIC on bf16 tensors: A_score/compute.py:12-15,54-72 executed by torch on bf16 inputs rounds the
 * result of EVERY op to bf16 (norm, divide, the element-wise products inside F.cosine_similarity, their sum, the mean) - which is what the
 * published table holds (policy/ablations_t.csv: 1.0078125 for CLIP336 against itself).  other / ref: bf16 [n_img, Nt | Nr, D] contiguous,
 * any D; scores fp32 [n_img], each a bf16-representable value as `.item()` of the reference's bf16 scalar; workspace of
 * visrep_ascore_refarith_workspace_bytes().  VALU kernel (the rounded products are not a matrix product): a parity mode. */
size_t visrep_ascore_refarith_workspace_bytes(int n_img, int Nt, int Nr, int D);
int visrep_ascore_maxcos_refarith(const void* other, const void* ref, int n_img, int Nt, int Nr, int D, float* scores, void* workspace,
                                  void* stream);

/* ---- C score (C_score/utils/utils_correspondence.py:345-382 calculate_keypoint_transformation with get_flow,
 * C_score/pck_train.py:24-29 normalize_feats): feats = bank of [C, P*P] fp32 maps; per pair image indices, source
 * patch indices [n_pairs,kmax] (kmax <= 32), keypoint counts; lin = float32(np.linspace(-1,1,P)); xy [n_pairs,kmax,2].
 * split = 0: one encoder (pck_train.py); split = C1 > 0: channels [0,C1) and [C1,C) are two encoders normalised separately,
 * concatenated and normalised again (C_score/pck_train_two.py:24-36 normalize_feats).
 * layout = 0: maps are [C, P*P] (the reference's on-disk [1, C, P, P]); layout = 1: [P*P, C], the towers' own token layout - a
 * keypoint's descriptor is then one contiguous row (C and split multiples of 4).
 * window: > 0 the (2w+1)^2 window around the argmax (get_flow :301-320: entries outside are ZERO and stay in the softmax); 0 the plain
 * soft-argmax; < 0 (round 6) the Gaussian-kernel soft-argmax (:321-324 -> apply_gaussian_kernel :278-295, sigma = -window patches; the
 * reference hard-wires a 60 x 60 grid there, these kernels take their own P). */
int visrep_cscore_transfer(const float* feats, const int* img1, const int* img2, const int* patch_idx, const int* nkp,
                           const float* lin, float* xy, int n_pairs, int kmax, int P, int C, int split, int window, int soft_eval,
                           float beta, float anno_stride, float anno_half, int layout, void* stream);
/* The same transfer for position-major banks ([n_images, P*P, C]) with the key points of SEVERAL pairs packed into one 32-row MFMA tile:
 * a group = pairs that share a target image, at most 32 key points in total (the caller packs them: one pair alone fills 11.5 of 32 rows
 * on SPair-71k).  rows_tab int32 [n_groups, 32, 4] = (pair, key-point index, source image, source patch index) per tile row, pair < 0 for an
 * empty row, 16-byte aligned; tgt int32 [n_groups] = the group's target image; xy [n_pairs, kmax, 2] as above (rows of a group write their own
 * (pair, key point) slot).  Same arithmetic per row as visrep_cscore_transfer, bit for bit. */
int visrep_cscore_transfer_packed(const float* feats, const int* rows_tab, const int* tgt, const float* lin, float* xy, int n_groups, int kmax,
                                  int P, int C, int split, int window, int soft_eval, float beta, float anno_stride, float anno_half,
                                  void* stream);
/* The packed transfer on TWO position-major banks, one per encoder: feats_a [n_images, P*P, C_a] and feats_b [n_images, P*P, C_b], indexed by the
 * same image slots.  Replaces C_score/pck_train_two.py:24-51 without materialising the channel concatenation: the reference loads the two
 * per-encoder maps of an image (:38-51), normalises each, concatenates and normalises again (:24-36 normalize_feats).  Channel block [0, C_a)
 * is streamed from bank A, [C_a, C_a + C_b) from bank B; everything after the loads is visrep_cscore_transfer_packed's arithmetic in its order,
 * so xy equals that kernel's on cat(A, B) with split = C_a bit for bit.  rows_tab / tgt / lin / xy as above; C_a, C_b multiples of 4. */
int visrep_cscore_transfer_packed2(const float* feats_a, int C_a, const float* feats_b, int C_b, const int* rows_tab, const int* tgt, const float* lin,
                                   float* xy, int n_groups, int kmax, int P, int window, int soft_eval, float beta, float anno_stride,
                                   float anno_half, void* stream);
/* per-pair PCK hit counts (C_score/pck_train.py:101,149-163): kps1/kps2 [n_pairs,kmax,3] (x,y,vis) fp32, thresholds
 * fp64 [n_pairs], alphas3 = HOST pointer to 3 floats; counts int32 [n_pairs,4] = hits@a0,a1,a2, n_visible. */
int visrep_pck_count(const float* xy, const float* kps1, const float* kps2, const double* thresholds, const int* nkp, int n_pairs,
                     int kmax, const float* alphas3, int* counts, void* stream);

/* ==== HOST twins ("`*_cpu` twins with identical signatures minus stream back config 1"; BASELINE configs[0]: the CLIP-L/14 tower
 * on 32 images, CPU fp32, plumbing without a GPU).  Plain C++ on host threads, fp32, HOST pointers, `threads` <= 0 = min(hardware threads, 32).
 * An independent implementation (csrc/host_twins.hip): it shares no code with the device kernels and never runs unless the caller asks for
 * device "cpu" explicitly - the device entry points above still fail without a GPU.  Same semantics as their device counterparts:
 *   visrep_vit_forward_cpu: fp32 weights in the visrep_vit_weights struct (matrices fp32 [out, in], patch_w [d, kpad]; sqkv / s1 ignored),
 *   pixels fp32 [B, 3, S, S], hidden fp32 [B, tokens, d] = hidden_states[n_layers];
 *   visrep_ascore_maxcos_cpu: fp32 [n_img, Nt | Nr, D] -> scores fp32 [n_img];
 *   visrep_cscore_transfer_cpu / visrep_pck_count_cpu: arguments of visrep_cscore_transfer / visrep_pck_count;
 *   visrep_cscore_transfer2_cpu: visrep_cscore_transfer_cpu on two position-major per-encoder banks (C_score/pck_train_two.py:24-51; the channels
 *   of a position are gathered from both banks, then the same code runs: equal to the one-bank call on cat(A, B) with split = C_a bit for bit). */
int visrep_vit_forward_cpu(const visrep_vit_config* cfg, const visrep_vit_weights* w, const float* pixels, float* hidden, int B, int n_layers,
                           int threads);
int visrep_ascore_maxcos_cpu(const float* other, const float* ref, int n_img, int Nt, int Nr, int D, float* scores, int threads);
int visrep_cscore_transfer_cpu(const float* feats, const int* img1, const int* img2, const int* patch_idx, const int* nkp, const float* lin,
                               float* xy, int n_pairs, int kmax, int P, int C, int split, int window, int soft_eval, float beta,
                               float anno_stride, float anno_half, int layout, int threads);
int visrep_cscore_transfer2_cpu(const float* feats_a, int C_a, const float* feats_b, int C_b, const int* img1, const int* img2, const int* patch_idx,
                                const int* nkp, const float* lin, float* xy, int n_pairs, int kmax, int P, int window, int soft_eval, float beta,
                                float anno_stride, float anno_half, int threads);
int visrep_pck_count_cpu(const float* xy, const float* kps1, const float* kps2, const double* thresholds, const int* nkp, int n_pairs, int kmax,
                         const float* alphas3, int* counts);

/* ==== Convolutional-tower primitives (Stable-Diffusion feature towers) ==================================
 * All activations are channels-last token matrices: [B*H*W, C] bf16.  A 3x3 convolution = visrep_im2col3x3 +
 * visrep_gemm_bf16 with K = ld of the gathered matrix and weights repacked [Cout, (ky, kx, Cin)] (zero-padded to ld). */

/* torch.nn.GroupNorm (+ optional SiLU) as used by diffusers resnet.py:ResnetBlock2D.forward (norm1/norm2 + nonlinearity),
 * transformer_2d.py:141 and vae.py conv_norm_out.  x, y: [B*HW, C] bf16 (y may alias x); gamma/beta fp32 [C]; fp32
 * statistics over (HW, C/groups) per (image, group), summed in a fixed order (bit-reproducible run to run).
 * workspace: visrep_groupnorm_workspace_bytes(B, HW, groups). */
size_t visrep_groupnorm_workspace_bytes(int B, int HW, int groups);
int visrep_groupnorm(const void* x, const float* gamma, const float* beta, void* y, int B, int HW, int C, int groups, float eps,
                     int silu, void* workspace, void* stream);

/* 3x3 patch gather for nn.Conv2d(kernel 3): y[(b, oy, ox), (ky*3+kx)*C + c] = x[b, oy*stride+ky-pad, ox*stride+kx-pad, c]
 * (zero outside), columns [9C, ldy) zeroed.  pad_mode 0 = padding 1 on every side (resnet convs, UNet downsample
 * stride 2: downsampling.py Downsample2D padding=1); pad_mode 1 = F.pad(x, (0,1,0,1)) then no padding (VAE encoder
 * downsample, downsampling.py:130-133).  upsample = 1 reads the source through a nearest-neighbour 2x upsample
 * (upsampling.py Upsample2D: F.interpolate(scale_factor=2, mode="nearest") + conv) without materialising it. */
int visrep_im2col3x3(const void* x, void* y, int B, int H, int W, int C, int stride, int pad_mode, int upsample, int ldy, void* stream);

/* nn.Conv2d(kernel 3) as an IMPLICIT GEMM: the gather of visrep_im2col3x3 happens inside the GEMM's A-operand LDS-DMA
 * (per-lane source addresses, zero page for padded taps), so the 9x-expanded patch matrix never exists in HBM.
 * x: [B*H*W, C] bf16 channels-last, C % 64 == 0; Wt: [Cout (% 64 == 0), ldw >= 9*C] bf16 with K order (ky, kx, c);
 * out: [B*Ho*Wo, ldc] (fp32 for VISREP_EPI_F32); stride / pad_mode / upsample as visrep_im2col3x3; epilogue BIAS, RESID
 * (out = resid + conv + bias, resid [B*Ho*Wo, ldc]) or F32.  Few-tile problems use the split-K path when a scratch is set. */
int visrep_conv3x3_bf16(const void* x, int B, int H, int W, int C, const void* Wt, int ldw, const float* bias, void* out, int ldc, int Cout,
                        int stride, int pad_mode, int upsample, int epilogue, const void* resid, void* stream);

/* The same convolution (no upsampling, epilogue BIAS | RESID) that ALSO emits the GroupNorm statistics of its output - the norm1 / norm2 /
 * conv_norm_out that follows it in diffusers resnet.py:ResnetBlock2D / vae.py:Encoder - as partial sums from its epilogue:
 * gn_partial[((b * (Ho Wo / 64) + slot) * groups + g)] = (sum, sum of squares) of the fp32 outputs of image b, rows [64 slot, 64 slot + 64), group g
 * (visrep_conv_gn_partial_bytes(B, Ho Wo, groups) bytes, every entry written).  visrep_groupnorm_from_partials() then normalises without
 * reading the tensor for its statistics.  Supported when visrep_conv_gn_supported_epi(B, Ho Wo, Cout, groups, epilogue): Ho Wo % 128 == 0,
 * Cout % 64 == 0, Cout / groups in {4, 8, 16}, and a kernel that emits the sums without costing the convolution its route: the 128x128
 * kernel (both epilogues, from its epilogue's store loop) or - round 5 - the 256x256 ping-pong kernel for VISREP_EPI_BIAS (a packed-math pass
 * over the accumulators in front of its epilogue); a RESID convolution that the 256x256 kernel runs is answered 0 and keeps the separate
 * statistics pass.  visrep_conv_gn_supported() is the round-4 query without the epilogue (the answer that holds for both epilogues). */
int visrep_conv_gn_supported(int B, int HWo, int Cout, int groups);
int visrep_conv_gn_supported_epi(int B, int HWo, int Cout, int groups, int epilogue);
size_t visrep_conv_gn_partial_bytes(int B, int HWo, int groups);
int visrep_conv3x3_bf16_gn(const void* x, int B, int H, int W, int C, const void* Wt, int ldw, const float* bias, void* out, int ldc, int Cout,
                           int stride, int pad_mode, int epilogue, const void* resid, void* gn_partial, int groups, void* stream);
/* GroupNorm (+ SiLU) of x [B*HW, C] from such partial sums (HW % 64 == 0): finalize + apply.  workspace: >= B * groups * 8 bytes. */
int visrep_groupnorm_from_partials(const void* x, const float* gamma, const float* beta, void* y, int B, int HW, int C, int groups, float eps,
                                   int silu, const void* partial, void* workspace, void* stream);

/* ---- 3x3 convolution (stride 1, padding 1) with the INPUT's GroupNorm (+ SiLU) fused into its operand path, for the VAE encoder's
 * 128-channel layers (diffusers resnet.py ResnetBlock2D.forward: norm1 -> SiLU -> conv1 -> norm2 -> SiLU -> conv2 (+ shortcut); vae.py
 * Encoder at 768^2 / 384^2).  A workgroup owns a 16 x 16 output tile: its 18 x 18 x 128 input halo is fetched ONCE, normalised in registers
 * (gn_table[b, c] = (scale, shift) = (rstd gamma, beta - mean rstd gamma), then SiLU when silu != 0 - groupnorm_apply's arithmetic bit for
 * bit; NULL = use x as it is) and kept in LDS; the nine taps are shifted views of it, only W streams.  No normalised copy of the tensor
 * ever exists in HBM (the separate apply pass reads and re-writes 2 x 2.4 GB per layer at 768^2 x 16 images).  Results equal
 * visrep_conv3x3_bf16 on the normalised tensor bit for bit (same K order, same MFMA chains).
 * x [B H W, 128] bf16 channels-last; Wt [Cout, ldw >= 1152] with K order (ky, kx, c); out / resid [B H W, ldc]; epilogue BIAS | RESID.
 * gn_partial (may be NULL): GroupNorm partial sums of the OUTPUT for the norm that follows, layout of visrep_conv3x3_bf16_gn
 * (visrep_conv_gn_partial_bytes(B, H W, groups_out) bytes; slot = 64 pixels of a 16 x 4 patch; consumed by visrep_groupnorm_stats_from_partials
 * / visrep_groupnorm_from_partials).  Supported: C = 128, Cout in {128, 256}, H and W multiples of 16 (visrep_conv3x3_halo_supported). */
int visrep_conv3x3_halo_supported(int B, int H, int W, int C, int Cout);
/* Tile height of the Cout = 128 kernel: 16 (default; 16 x 16-pixel tiles, 8 waves, 147 KB of LDS: one workgroup per CU) or 8 (16 x 8 tiles, 4 waves,
 * 77 KB: two workgroups per CU, one's halo phase under the other's K loop - measured 3 % slower, kept as a tested variant).  Results are bitwise the
 * same.  Process-wide (also VISREP_HALO_TILE=8 in the environment); returns the previous value, < 0 for another argument. */
int visrep_set_conv_halo_tile(int rows);
int visrep_conv3x3_bf16_halo(const void* x, int B, int H, int W, int C, const void* Wt, int ldw, const float* bias, void* out, int ldc, int Cout,
                             int epilogue, const void* resid, const void* gn_table, int silu, void* gn_partial, int groups_out, void* stream);

/* ---- The VAE encoder's first convolution (diffusers vae.py Encoder.conv_in: Conv2d(3, 128, 3, padding = 1); dift_sd.py:172 vae.encode) without
 * im2col: x [B*H*W, 8] bf16 tokens (visrep_nchw_to_tokens with Cpad = 8), Wt [128, ldw >= 96] in K order (ky, kx, c8) with zero padding columns (the
 * packer's im2col layout), out [B*H*W, ldc].  The MFMA's pixel operand is read straight from the neighbour pixels' 16-byte tokens (one global load
 * per lane and k-step, zeros outside the image), nothing is staged; the epilogue is the GEMM kernels' (bias, 16-byte stores) and optionally leaves
 * the GroupNorm partial sums of the output (gn_partial as visrep_conv3x3_bf16_gn: visrep_conv_gn_partial_bytes(B, H W, groups) bytes; NULL = none).
 * Supported: Cout = 128, W % 16 == 0, H W % 64 == 0 (% 128 with partial sums).  Equals visrep_im2col3x3 + visrep_gemm_bf16 up to the order of
 * the fp32 sum inside an MFMA.  K is padded from 72 to 96: weight columns 72 .. 95 ARE read (against zero pixel operands) and must be zero - a
 * finite value there is not promised to leave the result unchanged, a NaN or Inf poisons it; columns >= 96 are never read.  ldw and ldc must be
 * multiples of 8 (refused otherwise); out may be 8-byte aligned only (narrow stores). */
int visrep_conv3x3_c8_supported(int B, int H, int W, int Cout);
int visrep_conv3x3_c8_bf16(const void* x, int B, int H, int W, const void* Wt, int ldw, const float* bias, void* out, int ldc, int Cout,
                           void* gn_partial, int groups, void* stream);
/* The statistics half of GroupNorm on its own: stats[b, g] = (mean, rstd) fp32 pairs [B, groups], from a read-only pass over x
 * (visrep_groupnorm_stats; workspace of visrep_groupnorm_workspace_bytes) or from a producing convolution's partial sums
 * (visrep_groupnorm_stats_from_partials, HW % 64 == 0) - and the per-(image, channel) (scale, shift) table the fused convolution
 * consumes: table [B, C] float2 (visrep_groupnorm_table_from_stats). */
int visrep_groupnorm_stats(const void* x, void* stats, int B, int HW, int C, int groups, float eps, void* workspace, void* stream);
int visrep_groupnorm_stats_from_partials(const void* partial, void* stats, int B, int HW, int C, int groups, float eps, void* stream);
int visrep_groupnorm_table_from_stats(const void* stats, const float* gamma, const float* beta, void* table, int B, int C, int groups, void* stream);

/* activations.py GEGLU: y[m, f] = x[m, f] * gelu_erf(x[m, F + f]); x [M, >= 2F] bf16, y [M, >= F] bf16. */
int visrep_geglu(const void* x, int ldx, void* y, int ldy, long M, int F, void* stream);

/* softmax(scale * scores) per row: fp32 scores [rows, lds] -> bf16 probabilities [rows, ldp], columns [n, ldp) zeroed.
 * Used by the single-head 512-wide VAE mid-block attention (attention_processor.py Attention, vae.py:UNetMidBlock2D). */
int visrep_softmax_rows(const float* scores, int lds, void* probs, int ldp, int rows, int n, float scale, void* stream);

/* [B, C, H, W] (dtype VISREP_BF16 | VISREP_F32) -> [B*H*W, Cpad] bf16, channels [C, Cpad) zero. */
int visrep_nchw_to_tokens(const void* x, int dtype, void* y, int B, int C, int H, int W, int Cpad, void* stream);

/* F.interpolate(x, size=(OH, OW), mode="bilinear") (align_corners=False, no antialias) over `planes` = B*C contiguous
 * [H, W] planes (dtype VISREP_BF16 | VISREP_F32) -> bf16 [planes, OH, OW].  The image-variation featurizer resizes the
 * input to 224x224 for its CLIP image encoder this way (dift_imsd.py:215-216). */
int visrep_resize_bilinear(const void* x, int dtype, void* y, int planes, int H, int W, int OH, int OW, void* stream);

/* dift_sd.py:172-176: latents = (mean + exp(0.5 * clamp(logvar, -30, 20)) * post_noise) * scaling_factor
 * (autoencoder_kl.py encode + vae.py DiagonalGaussianDistribution.sample), then the scheduler's add_noise as
 * y = coef_latent * latents + coef_noise * ddim_noise:  DDIMScheduler (scheduling_ddim.py:471-495) has
 * coef_latent = sqrt(alphas_cumprod[t]), coef_noise = sqrt(1 - alphas_cumprod[t]); the vendored
 * FlowMatchEulerDiscreteScheduler.add_noise used by the SD3 featurizer (scheduling_flow_match_euler_discrete.py:192-210,
 * dift_sd3.py:108-111) has coef_latent = t, coef_noise = 1 - t with the raw integer timestep.  moments: fp32 [B*HW, ldm] with
 * the mean in columns [0, Z) and the log-variance in [Z, 2Z); the two noise tensors are the reference's randn draws made
 * explicit, fp32 [B, Z, H, W]; y: [B*HW, Cpad] bf16, channels [Z, Cpad) zero. */
int visrep_sd_noisy_latents(const float* moments, int ldm, const float* post_noise, const float* ddim_noise, void* y, int B, int Z,
                            int HW, int Cpad, float scaling, float coef_latent, float coef_noise, void* stream);

/* dift_sd.py:275 ensemble mean: x [B, E, N] bf16 -> y [B, N] bf16 (fp32 accumulation). */
int visrep_mean_groups(const void* x, void* y, int B, int E, long N, void* stream);

/* ==== Device input pipeline: everything after JPEG decode ================================================
 * One axis of Pillow's 8-bit separable resampling (src/libImaging/Resample.c ImagingResampleHorizontal_8bpc /
 * Vertical_8bpc) - what `PIL.Image.resize` does inside the reference's pre-processing (C_score/extract_feature.py:65-66,
 * HF CLIPImageProcessor.resize, llava/mm_utils.py:64-95) - BIT-EXACT: out[line, xx, c] = clip8((2^21 + sum_x in[line,
 * xmin[xx] + x, c] * kk[xx][x]) >> 22) with bounds = (xmin, count) pairs and the 22-bit fixed-point coefficient table the
 * host builds like precompute_coeffs + normalize_coeffs_8bpc (device_preprocess.pil_coeffs).  Strides in bytes select the
 * axis: horizontal pass line = row, vertical pass line = column. */
int visrep_resample_u8(const void* in, void* out, long n_lines, int out_len, int channels, long in_line_stride, long in_elem_stride,
                       long out_line_stride, long out_elem_stride, const int* bounds, const int* kk, int ksize, void* stream);

/* crop + ToTensor + Normalize: out[c, y, x] = (in[y0+y, x0+x, c] / 255 - mean3[c]) / std3[c], IEEE fp32 (bit-identical to the
 * numpy expression of the CPU processors); in: uint8 [H, W, 3] on the device; mean3 / std3: HOST float[3];
 * out: [3, crop_h, crop_w] VISREP_F32 or VISREP_BF16. */
int visrep_u8hwc_to_chw_norm(const void* in, int H, int W, int x0, int y0, int crop_h, int crop_w, const float* mean3, const float* std3,
                             void* out, int dtype, void* stream);

/* Both resampling passes + crop + ToTensor + Normalize for a BATCH of images of different sizes in two launches - what
 * `processor.preprocess(expand2square(Image.open(p).convert('RGB')))` (llava/feature/extract.py:198-214, llava/mm_utils.py:78-95) and
 * `Image.open(p).convert('RGB').resize((s, s))` + `(x / 255 - 0.5) * 2` (C_score/extract_feature.py:65-70) do per image, bit for bit.
 * desc: DEVICE int64 [n_images][24]: 0 source pointer (uint8 [H, W, 3] on the device), 1 H, 2 W, 3-4 canvas height / width (= H, W, or
 * the padded square of expand2square), 5-6 row / column of the image inside the canvas, 7 background colour r | g << 8 | b << 16,
 * 8 mirror the image left-right (pck_train.py:112), 9 pointer to this image's scratch [rows, crop_w, 3] for the horizontal pass,
 * 10-11 first canvas row / row count of that scratch (the rows the vertical pass reads), 12-14 horizontal bounds pointer / coefficient
 * pointer / ksize (ksize 0: no horizontal resize), 15-17 the same for the vertical pass, 18-19 crop origin x0, y0 in the resized image.
 * max_mid_rows = max over images of field 11 with ksize != 0 (0: no image needs a horizontal pass).  out: [n_images, 3, crop_h, crop_w]. */
int visrep_preprocess_u8_batch(const void* desc, int n_images, long max_mid_rows, int crop_h, int crop_w, const float* mean3,
                               const float* std3, void* out, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
