/*
 * boxdreamer_hip.h -- C ABI of libboxdreamer_hip.so (gfx950 / MI355X only).
 *
 * The drop-in boundary for BoxDreamer's corner-heatmap inference path.  The reference is pure
 * Python: its "native" boundary is the set of library calls it makes into CUDA-only packages
 * and ATen.  Each entry point below cites the reference call it replaces
 * (paths relative to the reference repo root).
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked [host];
 *   - the caller (PyTorch) owns every input / output / workspace buffer; the library never allocates or frees device memory,
 *     never synchronises the device, and reads no environment variables: everything that affects numerics or scheduling is an
 *     argument;
 *   - library-owned state, all of it: (1) per host thread and device, the side streams and fork / join events of the sub-batch lanes
 *     (bd_*_forward_lanes, created on first use or by bd_lanes_prepare, never destroyed; see "Sub-batch lanes" for what that
 *     means for concurrent callers), (2) the optional launch trace at the end of this file (off by default), (2b) HOST state only: up to 15
 *     detached worker threads of bd_solve_pnp_host, parked on a condition variable between calls (one call at a time uses them; a forked
 *     child starts its own), (3) an immutable
 *     per-device cache of the compute-unit count, (4) a THREAD-LOCAL hint "this thread's bd_gemm launches run side by side with
 *     n - 1 others of the same shape" (1 outside the laned entry points, which set it for the duration of their enqueue and reset it
 *     before they return): it only biases the choice between kernel FORMS of a launch (large / small tiles) towards the CUs' share
 *     of one lane -- a row's bits never depend on the form, so the hint cannot change a result, only a duration;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) -- the laned entry points also
 *     on their side streams, forked from and joined back into `stream` inside the call;
 *   - return 0 on success, a negative BD_ERR_* for bad arguments, a positive hipError_t if a launch failed; no exceptions,
 *     no exit();
 *   - the plain entry points are re-entrant; one device per process in the multi-GPU sweep.
 *
 * Precision modes (`prec`): accumulation, the residual stream, LayerNorm / RMSNorm statistics, softmax and the logits are
 * fp32 in every mode; `prec` selects the MFMA operand format only (DESIGN.md section 3 has the measured logit errors):
 *   BD_PREC_F16C8_QK16  the package DEFAULT and the mode that meets north_star's 1e-3 bar with margin: one f16 MFMA pass +
 *                       one e4m3 correction pass per Linear (BD_PREC_F16C8), BETR's q, k columns one f16 pass
 *   BD_PREC_F16X3       split-f16, three passes: the class a PROMOTED Linear runs in; *_ATTN_X3 = the most precise GPU mode
 *   BD_PREC_BF16X3      split-bf16, three passes (round 1's strict mode)
 *   BD_PREC_BF16        one v_mfma_f32_32x32x16_bf16 pass: BASELINE.json's headline dtype, an explicit throughput opt-in --
 *                       4e-2 off the fp32 forward, like the reference's own bf16 autocast; does NOT meet the 1e-3 bar
 *   BD_PREC_F16         one v_mfma_f32_32x32x16_f16 pass (5e-3)
 *   BD_PREC_FP8         e4m3 Linears on the block-scaled MFMA (2x rate), bf16 attention: a THROUGHPUT DEMONSTRATION of
 *                       BASELINE configs[4] -- 3 mantissa bits are 0.6 max-abs / 0.13 rms off on the logits, the decoded
 *                       corners are not usable on noise-like heatmaps (tolerance restated)
 * In the split classes every 16-bit activation / weight tensor is stored as two planes (hi, then lo at +plane elements);
 * see DESIGN.md "data layout".
 */
#ifndef BOXDREAMER_HIP_H
#define BOXDREAMER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BD_ABI_VERSION 9

#define BD_DTYPE_BF16 0
#define BD_DTYPE_F16 1
#define BD_DTYPE_F32 2

#define BD_PREC_BF16 0
#define BD_PREC_F16 1
#define BD_PREC_BF16X3 2
#define BD_PREC_F16_OUT_BF16X3 3 /* bd_attention[_q] only: f16 qkv (one plane) in, one f16 MFMA pass, split-bf16 (hi, lo) planes out */
#define BD_PREC_FP8 4            /* OCP e4m3 operands for every Linear (v_mfma_scale_f32_32x32x64_f8f6f4, unit block scales,
                                    per-output-channel weight scale in the epilogue); attention stays bf16 (configs[4]) */
#define BD_PREC_BF16_OUT_FP8 5   /* bd_attention[_q] only: bf16 attention whose output is stored as e4m3 */
/* Whole-path entry points only (bd_encoder_forward / bd_decoder_forward / *_workspace_bytes): attention policy of the
 * strict family.  Operand layout and GEMMs are BD_PREC_BF16X3's; the unit operators do not accept these values.
 *   BD_PREC_BF16X3           f16 single-pass attention where q, k are RMS-normalised (BETR), split-bf16 attention in DINOv2
 *   BD_PREC_BF16X3_ATTN_X3   split-bf16 attention everywhere */
#define BD_PREC_BF16X3_ATTN_X3 6
/* (7, 11, 12: BD_PREC_BF16X3_ATTN_F16, BD_PREC_BF16X3_QKV16, BD_PREC_F16C8_QKV16 of ABI <= 6 -- measured dead ends, removed in ABI 7:
 * f16 attention on DINOv2's un-normalised q / k misses the bar (1.2e-3); BETR's whole QKV as one f16 pass is superseded by
 * BD_PREC_F16C8_QK16, which buys the same time with a 3x smaller error.  The values stay reserved.) */
/* f16 + e4m3 corrections (the strict operand class):  A.W ~= hi_A.hi_W (one f16 MFMA pass) + lo_A.q_W + q_A.lo_W (one e4m3
 * pass over a doubled K on the block-scaled MFMA): 2 pass-equivalents instead of BF16X3's 3, logits error 1.7e-4 at full depth.
 * Accepted by: bd_gemm, bd_layernorm, bd_im2col_images, bd_patchify_heatmaps, bd_gather_query_tokens and the whole-path entry
 * points.  NOT by bd_attention[_q] / bd_qk_rmsnorm (BD_ERR_DTYPE): attention runs on an f16 plane or on split-bf16 planes and
 * EMITS the class through BD_PREC_F16_OUT_F16C8 / BD_PREC_BF16X3_OUT_F16C8 below.
 * Storage of an operand [rows][K], K % 32 == 0, ld % 32 == 0; "plane" = 2-byte units between plane 0 and plane 1:
 *   plane 0                f16 hi = f16(x), row-major, 2 bytes per element (full f16 range; the e4m3 images below SATURATE at
 *                          +-448, so an element beyond 448 degrades towards single-f16-pass accuracy instead of being clipped).
 *   plane 1, ACTIVATIONS   lo8 = e4m3((x - hi) * 2^11): ONE byte per element, rows of `ld` BYTES packed into the first rows*ld
 *                          bytes of the plane (the rest of the plane's storage is unused); inside every 32-element block the
 *                          byte at 16 h + 8 a + j holds k = 16 a + 8 h + j (a, h < 2, j < 8).  q8 = e4m3(hi) is derived by the
 *                          GEMM in registers, nothing stored.
 *   plane 1, WEIGHTS       TWO bytes per element, rows of 2*ld bytes: per 32-element block 64 bytes = for each h < 2:
 *                          [ q8 x 16 | lo8 x 16 ] of the sixteen k = 16 a + 8 h + j in (a, j) order, with
 *                          q8 = e4m3(hi * 2^E), lo8 = e4m3((w - hi) * 2^(E + 11)); E = bd_linear.w_qexp / bd_gemm_args.w_qexp,
 *                          one exponent per weight tensor (the largest E with max|w| * 2^E <= 448).
 * boxdreamer_amd/hip_ops.py:f16c8_encode / f16c8_decode are the reference packers (torch ops, load time only). */
#define BD_PREC_F16C8 8
/*   BD_PREC_F16C8_QK16       whole-path only (round 3's default): BD_PREC_F16C8 Linears; in the blocks whose q, k are RMS-normalised
 *                            (BETR) the QKV Linear is split by output column: q, k (2/3 of the columns) as ONE f16 pass on the f16
 *                            plane of the F16C8 LayerNorm output, v as a full F16C8 product.  Column-wise sensitivity
 *                            (tools/policy_sim.py): the whole 5e-4 a single-pass QKV costs comes from the v columns; q, k -- normalised
 *                            right away and consumed through a softmax -- cost 2e-5.  1.33 pass-equivalents for that Linear
 *                            instead of 2 (F16C8), logits error 2.1e-4.  Needs bd_block_weights.qkv16. */
#define BD_PREC_F16C8_QK16 13
/* Split-f16 (round 4): hi = f16(x), lo = f16(x - hi), three f16 MFMA passes (hi*hi + hi*lo + lo*hi) like BD_PREC_BF16X3 but with
 * 11 + 11 mantissa bits instead of 8 + 8: products are fp32-faithful (~2^-22) for |x| up to f16's 65504 (conversions saturate), and
 * lose only absolute 6e-8 steps where a lo falls into f16's subnormals.  Measured / simulated 4x closer to the fp32 forward than
 * split-bf16 on trained-like outlier weights at the same cost (oracle/numerics_sim.py): it is the class the per-Linear PROMOTION
 * of the F16C8 family moves a Linear to (bd_block_weights.promote), and a whole-path mode of its own:
 *   BD_PREC_F16X3            Linears split-f16; attention as BD_PREC_BF16X3 (one f16 pass where q, k are RMS-normalised, split-bf16
 *                            elsewhere: probabilities and unnormalised q.k^T need bf16's range);
 *   BD_PREC_F16X3_ATTN_X3    whole-path only: split-bf16 attention everywhere -- the most precise GPU mode, the reference of the
 *                            load-time self-check.
 * Storage: two f16 planes (hi, then lo at +plane elements), exactly as BD_PREC_BF16X3.  Accepted by bd_gemm, bd_layernorm,
 * bd_im2col_images, bd_patchify_heatmaps, bd_gather_query_tokens and the whole-path entry points; attention EMITS the class through
 * BD_PREC_F16_OUT_F16X3 / BD_PREC_BF16X3_OUT_F16X3. */
#define BD_PREC_F16X3 14
#define BD_PREC_F16X3_ATTN_X3 15
#define BD_PREC_F16_OUT_F16X3 16    /* bd_attention[_q] only: f16 qkv (one plane) in, one f16 MFMA pass, split-f16 (hi, lo) planes out */
#define BD_PREC_BF16X3_OUT_F16X3 17 /* bd_attention[_q] only: split-bf16 qkv planes in, split-bf16 attention, split-f16 planes out */
#define BD_PREC_F16_OUT_F16C8 9     /* bd_attention[_q] only: f16 qkv (one plane) in, one f16 MFMA pass, F16C8 operand out */
#define BD_PREC_BF16X3_OUT_F16C8 10 /* bd_attention[_q] only: split-bf16 qkv planes in, split-bf16 attention, F16C8 operand out */

#define BD_OK 0
#define BD_ERR_SHAPE (-1)
#define BD_ERR_DTYPE (-2)
#define BD_ERR_ALIGN (-3)
#define BD_ERR_WORKSPACE (-4)
#define BD_ERR_NULL (-5)

#define BD_ACT_NONE 0
#define BD_ACT_GELU 1 /* exact erf GELU (timm Mlp / vggsfm Mlp / DINOv2 Mlp all use nn.GELU()) */

int bd_abi_version(void);
const char* bd_target_arch(void); /* "gfx950" */

/* ------------------------------------------------------------------------------------------
 * Unit operators (used directly by the parity tests and composed by the forward entry points)
 * ---------------------------------------------------------------------------------------- */

/* out[map(r), :] = act(A[r,:] . W^T + bias) + addtab[r % tab_rows, :] + resid[map(r), :]
 * Replaces every nn.Linear on the path (cuBLAS via ATen):
 *   src/models/modules/backbone/utils/blocks.py:229,233 (qkv, proj), timm Mlp fc1/fc2 (blocks.py:859-867),
 *   src/models/modules/backbone/betr.py:131-176 (bbox_emb, bbox_proj, input_transform),
 *   src/models/sources/DINOv2/layers/attention.py:51-53, layers/mlp.py:29-31,
 *   and the 14x14/s14 patch-embed conv as an im2col GEMM (layers/patch_embed.py:65,75).
 * A: [M, K] 16-bit row-major (lda elements); W: [N, K] 16-bit row-major (nn.Linear layout).
 * K must be a multiple of 64 (128 for BD_PREC_FP8; callers zero-pad); M, N arbitrary.
 * Leading dimensions may exceed the row length (rows inside a wider buffer, planes further apart than rows * ld) but never fall below
 * it: lda < K, ldw < K, ldo < N, ldr < N with a residual, or ln_op_ld < N with ln_op_out would make consecutive rows overlap and
 * return BD_ERR_SHAPE before any launch (a host check of the arguments; nothing is read from the device).
 * map(r) = r if rpg_in == 0 else (r / rpg_in) * rpg_out + r % rpg_in + row_off. */
typedef struct bd_gemm_args {
    const void* A; int64_t lda; int64_t a_plane;   /* a_plane: elements between hi/lo planes (BF16X3) */
    const void* W; int64_t ldw; int64_t w_plane;
    const float* bias;                             /* [N] or NULL */
    const float* wscale;                           /* [N] per-output-channel dequantisation scale (FP8) or NULL */
    const float* resid; int64_t ldr;               /* fp32 [*, N] indexed by the OUTPUT row, or NULL */
    const float* addtab; int tab_rows;             /* fp32 [tab_rows, N] or NULL */
    void* out; int64_t ldo; int64_t out_plane;     /* 16-bit (operand dtype of `prec`) or fp32 */
    int out_f32;                                   /* 0: operand-dtype output (planes per `prec`), 1: fp32, 2: f16 single plane,
                                                      3: bf16 single plane, 4: split-bf16 (hi, lo) planes at out_plane,
                                                      5: split-f16 (hi, lo) planes at out_plane */
    int M, N, K;
    int act;
    int rpg_in, rpg_out, row_off;
    int w_qexp;                                    /* BD_PREC_F16C8: exponent E of the weight's e4m3 planes */
    /* Fused q/k RMSNorm (LlamaRMSNorm on q and k after the head split, blocks.py:44-56,257) for a QKV Linear whose output
     * columns are [q | k | v] x heads x head_dim with head_dim == 96: q, k <- w * x * rsqrt(mean_96(x^2) + eps) on the fp32
     * accumulators, before the 16-bit store (no extra rounding, no separate pass over qkv).  Only where the launch uses 256 x 192
     * tiles (each wave tile is one head); bd_gemm returns BD_ERR_SHAPE otherwise -- ask bd_gemm_fuses_qk_rmsnorm first. */
    const float* rms_wq; const float* rms_wk; float rms_eps;
    int rms_parts;                                 /* with rms_wq: 0 or 3 = output columns are [q | k | v] (v untouched); 2 = [q | k] only
                                                      (a QKV Linear split into a q,k launch and a v launch, BD_PREC_F16C8_QK16) */
    /* LayerNorm folded into the neighbouring Linears (ABI 8; replaces the nn.LayerNorm launches between a residual Linear and the next
     * Linear: blocks.py:35-41, 876-886, DINOv2 layers/block.py:89-114).  LN(x) W^T + b = rstd (x (g . W)^T - mean s) + (beta W^T + b),
     * s[n] = sum_k (g . W)[n, k]: the weights are gain-folded at load time (bd_block_weights.qkv_f, fc1_f), the PRODUCER of x emits
     * what the consumer needs, the CONSUMER applies the row statistics to its fp32 accumulators.
     *   producer (an fp32-result Linear with a residual, BD_PREC_F16C8, N = 768): next to the fp32 rows it writes (a) their BD_PREC_F16C8
     *     operand copy -- the raw, un-normalised row -- at ln_op_out and (b) per 96-column wave tile the pair (mean, M2 = sum (x - mean)^2)
     *     of its 96 values at ln_stats_out[row][N / 96][2]: plain stores, one writer per element, no atomics -- deterministic;
     *   consumer (BD_PREC_F16C8, or BD_PREC_F16 with the fused q/k RMSNorm; K = 768): combines the row's K / 96 pairs in a fixed order
     *     (Chan), rstd = rsqrt(M2 / K + ln_eps), and forms rstd * acc + (-mean rstd) * ln_colsum[n] + bias[n] before anything else.
     * Ask bd_gemm_takes_ln_fold first: launches that would not run on a kernel form with these epilogues return BD_ERR_SHAPE. */
    float* ln_stats_out; void* ln_op_out; int64_t ln_op_plane; int64_t ln_op_ld;
    const float* ln_stats_in; const float* ln_colsum; float ln_eps;
    /* producer side, the 3-byte residual stream: 1 = the residual rows are READ from the operand copy at ln_op_out (x = hi + lo8 2^-11, exactly
     * what the consumer Linears multiply) instead of `resid` (which must be NULL), the sum is written back there in place, and the fp32 rows
     * at `out` are written only with out_f32 == 1 (out_f32 == 0: `out` is ignored -- nobody reads the stream as fp32 before the next residual
     * Linear).  Per residual Linear 3 + 3 bytes per element cross HBM instead of 4 + 7; the stream is rounded to the operand class (~2^-15
     * relative) once per residual add (tools/lnfold_sim.py RESID3=1: logits 2.2e-4 -> 2.6e-4 at full depth). */
    int ln_resid_in_op;
    /* Split-K for launches of a few tiles (ABI 9; BD_PREC_F16C8, the fp32-residual Linears proj / fc2 -- with or without the ln_* producer
     * fields -- at M <= BD_SPLITK_MAX_ROWS: one pose at a time, the reference demo's per-frame call src/demo/demo.py:1501-1514).
     * sk_ws != NULL lends the launch a scratch region of bd_gemm_splitk_workspace_bytes(M, N) bytes, 256-byte aligned, whose first
     * BD_SPLITK_FLAG_BYTES bytes are ZERO when the launch starts (every launch leaves them zero again, so launches on fewer rows may reuse
     * a region sized for more; the region must not be shared by launches that may run concurrently).  The library then MAY compute every 128 x 96 output tile with S = 2 .. 4 workgroups over
     * disjoint K ranges, summed in a fixed order: deterministic, but NOT bit-identical to the unsplit result (fp32 association differs,
     * ~1e-7 relative) -- the row-result-independent-of-the-launch-form property of the other forms does not hold across this switch,
     * which is why it is opt-in per launch.  sk_split: 0 = the library chooses (1 = no split where it does not pay), 2 .. 4 = forced. */
    void* sk_ws; int sk_split;
} bd_gemm_args;
#define BD_SPLITK_MAX_ROWS 4096
#define BD_SPLITK_FLAG_BYTES 16384
size_t bd_gemm_splitk_flag_bytes(int M, int N);            /* BD_SPLITK_FLAG_BYTES, or 0 when M, N have no split-K form */
size_t bd_gemm_splitk_workspace_bytes(int M, int N);      /* 0 when M, N have no split-K form (N % 96 != 0, M > BD_SPLITK_MAX_ROWS) */
int bd_gemm(const bd_gemm_args* args /*[host]*/, int prec, void* stream);
/* 1 if bd_gemm(args, prec) serves the ln_* fields that are set in args (producer and / or consumer side of the LayerNorm fold), else 0. */
int bd_gemm_takes_ln_fold(const bd_gemm_args* args /*[host]*/, int prec);
/* 1 if bd_gemm(args, prec) with args->rms_wq set would fuse the q/k RMSNorm (tile shape and head geometry fit), else 0. */
int bd_gemm_fuses_qk_rmsnorm(const bd_gemm_args* args /*[host]*/, int prec);

/* Which kernel instances bd_gemm(args, prec) launches, decided on the host (no GPU needed, nothing is launched or dereferenced; for
 * tests and tools -- nothing on the product path calls these).  bd_gemm plans with the same function and then launches the plan.
 * A launch names one row of its kernel family's instance table: `key` holds the instance's template arguments as integers, in
 * declaration order, unused entries 0:
 *   BD_GEMM_FAMILY_PC        gemm_kernel_pc        T (0 bf16, 1 f16, 2 e4m3), NS, BK, WM, WN, MI, NI, NPW, EP, OUTK, GELU, RING, LNF
 *   BD_GEMM_FAMILY_GLDS      gemm_kernel_glds      T, NS, BK, WM, WN, MI, NI, NSTG
 *   BD_GEMM_FAMILY_PC_F16C8  gemm_kernel_pc_f16c8  NSTAGE, EP, OUTK, GELU, WM, WN, NPW, LNF, SK
 * (a workgroup tile is WM MI 32 x WN NI 32; EP: 0 generic epilogue, 1 16-bit result, 2 fused q/k RMSNorm, 3 fp32 + residual, 4 / 5 the
 * LayerNorm-fold producers; LNF: LayerNorm-fold consumer; OUTK: a value of bd_gemm_args.out_f32).  The launches of a plan cover the
 * disjoint row ranges [row0, row0 + rows) of the problem; split_k is 1 or the split-K factor S the launch runs with. */
#define BD_GEMM_FAMILY_PC 1
#define BD_GEMM_FAMILY_GLDS 2
#define BD_GEMM_FAMILY_PC_F16C8 3
#define BD_GEMM_KEY_LEN 13
#define BD_GEMM_PLAN_MAX_LAUNCHES 3
typedef struct bd_gemm_launch {
    int family, row;                               /* row: index into the family's table (bd_gemm_instance) */
    int key[BD_GEMM_KEY_LEN];
    int grid, block;                               /* workgroups, threads per workgroup */
    int row0, rows;
    int split_k;
} bd_gemm_launch;
typedef struct bd_gemm_plan_t { int n_launches; bd_gemm_launch launch[BD_GEMM_PLAN_MAX_LAUNCHES]; } bd_gemm_plan_t;
/* Writes the plan bd_gemm(args, prec) would execute on a device of `cus` compute units (<= 0: the current device's count; 256 without
 * a device) while `concurrent_launches` launches of the same shape share it (<= 0: 1; the sub-batch lanes).  Returns BD_OK, or the
 * BD_ERR_* code with which bd_gemm refuses these arguments (out->n_launches = 0 then). */
int bd_gemm_plan(const bd_gemm_args* args /*[host]*/, int prec, int cus, int concurrent_launches, bd_gemm_plan_t* out /*[host]*/);
/* Row `index` of a family's instance table: writes its key (BD_GEMM_KEY_LEN ints) and returns 1; returns 0 past the end of the
 * table or for an unknown family.  The tables hold every instantiated GEMM kernel. */
int bd_gemm_instance(int family, int index, int* key /*[host]*/);

/* LayerNorm over the last dim (fp32 statistics), optional affine, fp32 input rows gathered by
 * in_row(r) = r if rpg_in == 0 else (r / rpg_in) * rpg_out + r % rpg_in + row_off.
 * Writes a 16-bit copy (next GEMM's A operand) and/or an fp32 copy.
 * Replaces blocks.py:35-41 (LayerNorm, eps hard-wired to 1e-5 by get_layernorm blocks.py:790-805),
 * betr.py:161,315 (adapter LayerNorm, no affine, eps 1e-6) and DINOv2 nn.LayerNorm eps 1e-6
 * (vision_transformer.py:95,263). */
int bd_layernorm(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                 void* out16, int64_t out16_plane, float* out32, int64_t ldo, int rows, int cols,
                 int rpg_in, int rpg_out, int row_off, int prec, void* stream);

/* In-place q/k RMSNorm on a packed qkv tensor [rows, 3, heads, head_dim] (16-bit):
 * q,k <- w * x * rsqrt(mean(x^2) + eps) in fp32.  Replaces LlamaRMSNorm, blocks.py:44-56,257. */
int bd_qk_rmsnorm(void* qkv, int64_t plane, const float* wq, const float* wk, float eps, int rows,
                  int heads, int head_dim, int prec, void* stream);

/* Multi-head self-attention softmax(scale * Q K^T) V on packed qkv [batch, seq, 3, heads, head_dim]
 * -> out [batch, seq, heads*head_dim] (16-bit).  head_dim in {64, 96}.  One sample's qkv rows (seq * 3 * heads * head_dim * 2 bytes)
 * must stay below 2 GiB (the kernels reach them through 32-bit buffer descriptors): BD_ERR_SHAPE otherwise.
 * Replaces flash_attn.flash_attn_func / F.scaled_dot_product_attention (blocks.py:259-285) and
 * xformers.ops.memory_efficient_attention / the naive softmax path (DINOv2 layers/attention.py:56-89). */
int bd_attention(const void* qkv, int64_t qkv_plane, void* out, int64_t out_plane, int batch, int seq,
                 int heads, int head_dim, float scale, int prec, void* stream);

/* Same, but only the rows [q_view[b]*q_len, +q_len) of every sequence act as queries (keys/values: all `seq` rows);
 * out is compact [batch, q_len, heads*head_dim].  Used for the LAST decoder block, whose output is consumed for the
 * query view only (betr.py:303).  q_view == NULL requires q_len == seq (plain attention). */
int bd_attention_q(const void* qkv, int64_t qkv_plane, void* out, int64_t out_plane, int batch, int seq,
                   int heads, int head_dim, float scale, const int32_t* q_view, int q_len, int prec, void* stream);

/* bd_attention for a sequence whose first n_prefix tokens are not patch tokens (DINOv2: cls + registers,
 * vision_transformer.py:219-230).  prefix_queries != 0: exactly bd_attention (one launch over all queries: measured faster than any
 * split, profiles/r4_attention.md).  prefix_queries == 0: only the seq - n_prefix patch queries are computed (all keys; exact query
 * tiles) and rows [0, n_prefix) of every sample in `out` are left untouched -- the LAST encoder block, whose prefix rows
 * x_norm_patchtokens drops (vision_transformer.py:263-267).  Patch rows are bit-identical between the two forms. */
int bd_attention_prefix(const void* qkv, int64_t qkv_plane, void* out, int64_t out_plane, int batch, int seq, int heads,
                        int head_dim, float scale, int n_prefix, int prefix_queries, int prec, void* stream);

/* Ragged batches: bd_attention / bd_attention_q for samples with DIFFERENT numbers of views, packed back to back -- the
 * flash_attn_varlen_func form of the boundary above (cu_seqlens), in units of views.  qkv: [n_views * tokens_per_view, 3, heads,
 * head_dim]; sample b owns the views [view_start[b], view_start[b + 1]), i.e. the token rows [view_start[b] * tokens_per_view,
 * view_start[b + 1] * tokens_per_view), and softmax(scale * Q K^T) V runs inside them: no padded views, nothing attends across samples.
 * view_start: DEVICE int32 [batch + 1], ascending, view_start[0] = 0, view_start[batch] = n_views.  n_views (their total) and max_views
 * (the largest per-sample count) are the HOST's copies of the same numbers: they size the grid and bound the per-sample buffer
 * descriptor, so the call never reads the offsets on the host and never synchronises.  A sample whose offsets disagree with them
 * (descending, more than max_views views, beyond n_views) is skipped by the kernel: its output rows are left untouched.
 *   q_view == NULL   every row is a query; out is packed like the input: [n_views * tokens_per_view, heads * head_dim].
 *   q_view != NULL   DEVICE int32 [batch], the view index INSIDE the sample (clamped to it): only that view's tokens_per_view rows are
 *                    queries and out is compact [batch * tokens_per_view, heads * head_dim] -- bd_attention_q's form, the last BETR block.
 * head_dim == 96 only (BETR; DINOv2's head_dim-64 sequences are per image and never ragged) and tokens_per_view % 128 == 0, so that every
 * sample is whole 64-key tiles and whole query blocks and no tail is masked (BETR: 256): BD_ERR_SHAPE otherwise.  The 2 GiB rule of
 * bd_attention applies per sample, to max_views * tokens_per_view rows.  Every `prec` bd_attention takes.
 * ONE launch: the work list (sample, head, query block) is implicit in the offsets -- the grid is exactly the batch's query blocks
 * (q_view: the batch's query views' blocks), never sized by the longest sample; a workgroup finds its sample with one ballot over the
 * offsets.  The same kernels as bd_attention, as their VL instances (which one, and the grid: bd_attention_plan), taking their base row
 * and key count per sample: a row's bits equal bd_attention[_q] run on that sample alone (batch = 1, seq = its rows).
 * Launch trace: one kind-1 record, N = max_views * tokens_per_view. */
int bd_attention_varlen(const void* qkv, int64_t qkv_plane, void* out, int64_t out_plane, const int32_t* view_start, int batch,
                        int n_views, int max_views, int tokens_per_view, int heads, int head_dim, float scale,
                        const int32_t* q_view, int prec, void* stream);

/* Which kernel instance an attention call launches, decided on the host (no GPU needed, nothing is launched or dereferenced; for tests
 * and tools -- nothing on the product path calls these).  The four entry points plan with the same function and then launch the plan.
 * A call is described by bd_attn_call: the entry point and its integer arguments (fields an entry point does not take are ignored),
 * whether q_view is given, and latency_forms -- the opt-in forms of bd_*_weights.latency_mode, which no public entry point can ask for
 * (they pass 0).  A launch names one row of its kernel family's instance table; `key` holds the template arguments as integers:
 *   BD_ATTN_FAMILY_TILED  attn_kernel     T (0 bf16, 1 f16), NS, HD, NW, OUTMODE, VL
 *   BD_ATTN_FAMILY_PP     attn_kernel_pp  T, HD, OUTMODE, VL
 * (NS: operand planes; HD: head_dim; NW: waves = 32-query blocks per workgroup, the ping-pong kernel has 8; OUTMODE: 0 operand class,
 * 1 split-bf16, 2 e4m3, 3 F16C8, 4 split-f16; VL: the ragged instance.)  q_len / q_off / out_rows: queries are the rows [q_off, q_off +
 * q_len) of a sample (of its query view with q_view), written to a sample's out_rows result rows from q_off. */
#define BD_ATTN_ENTRY_PLAIN 0                      /* bd_attention */
#define BD_ATTN_ENTRY_Q 1                          /* bd_attention_q */
#define BD_ATTN_ENTRY_PREFIX 2                     /* bd_attention_prefix */
#define BD_ATTN_ENTRY_VARLEN 3                     /* bd_attention_varlen */
#define BD_ATTN_FAMILY_TILED 1
#define BD_ATTN_FAMILY_PP 2
#define BD_ATTN_KEY_LEN 6
typedef struct bd_attn_call {
    int entry;
    int batch, seq, heads, head_dim;
    int has_q_view, q_len;                         /* bd_attention_q, bd_attention_varlen (has_q_view only) */
    int n_prefix, prefix_queries;                  /* bd_attention_prefix */
    int n_views, max_views, tokens_per_view;       /* bd_attention_varlen (which takes no seq) */
    int prec;
    int latency_forms;
} bd_attn_call;
typedef struct bd_attn_launch {
    int family, row;                               /* row: index into the family's table (bd_attention_instance) */
    int key[BD_ATTN_KEY_LEN];
    int grid, block;                               /* workgroups, threads per workgroup */
    int q_len, q_off, out_rows;
} bd_attn_launch;
typedef struct bd_attn_plan_t { int n_launches; bd_attn_launch launch[1]; } bd_attn_plan_t;
/* Writes the plan of `call` made with these pointers (device addresses, compared with NULL and checked for alignment only; view_start:
 * bd_attention_varlen).  Returns BD_OK, or the BD_ERR_* code with which the entry point refuses the call (out->n_launches = 0 then). */
int bd_attention_plan(const bd_attn_call* call /*[host]*/, const void* qkv, const void* out, const void* view_start,
                      bd_attn_plan_t* plan /*[host]*/);
/* Row `index` of a family's instance table: writes its key (BD_ATTN_KEY_LEN ints) and returns 1; returns 0 past the end of the
 * table or for an unknown family.  The tables hold every instantiated attention kernel. */
int bd_attention_instance(int family, int index, int* key /*[host]*/);

/* (x - mean_c) / std_c, then 14x14 patches -> A operand rows [n*grid*grid, kpad], k = c*p*p + py*p + px,
 * zero-padded to kpad.  Replaces encoder/dinov2.py:45-46,56 + the unfold inside the patch-embed conv. */
int bd_im2col_images(const void* images, int img_dtype, void* out16, int64_t out_plane, int n_images,
                     int size, int patch, int kpad, int prec, void* stream);

/* BETR.patchify (betr.py:211-228): [n, c, size, size] -> [n*grid*grid, kpad], feature (py*p+px)*c + ch. */
int bd_patchify_heatmaps(const void* heat, int in_dtype, void* out16, int64_t out_plane, int n_images,
                         int channels, int size, int patch, int kpad, int prec, void* stream);

/* Writes the n_prefix (cls+pos, registers) token rows of every image's token block
 * (vision_transformer.py:219-230).  prefix: fp32 [n_prefix, dim]. */
int bd_write_prefix_tokens(float* x, const float* prefix, int n_images, int tokens_per_image,
                           int n_prefix, int dim, void* stream);

/* Query-view substitution (betr.py:286-290 + :367-399): for every sample b the token rows of view
 * query_idx[b] become query_token + rgb + pos.  x, rgb: fp32 [B*T*P, dim]; pos: [P, dim]. */
int bd_query_substitute(float* x, const float* rgb, const float* pos, const float* query_token,
                        const int32_t* query_idx, int B, int T, int P, int dim, void* stream);

/* fp32 copy of the query view's P token rows per sample: x [B*T*P, dim] -> out [B*P, dim]. */
int bd_gather_query_rows_f32(const float* x, const int32_t* query_idx, float* out, int B, int T, int P, int dim,
                             void* stream);

/* Gathers the query view's P token rows per sample (betr.py:303) and casts to the operand dtype
 * (query_idx == NULL: view 0, i.e. a pure cast of an already compact [B*P, dim] tensor with T = 1). */
int bd_gather_query_tokens(const float* x, const int32_t* query_idx, void* out16, int64_t out_plane,
                           int B, int T, int P, int dim, int prec, void* stream);

/* The three query-view operators above for a ragged batch (bd_attention_varlen's packing): x, rgb are [n_views * P, dim], sample b's
 * query view is view view_start[b] + query_view[b] of the packed batch (query_view counts inside the sample and is clamped to it).
 * view_start: device int32 [B + 1]; query_view: device int32 [B]. */
int bd_query_substitute_varlen(float* x, const float* rgb, const float* pos, const float* query_token, const int32_t* view_start,
                               const int32_t* query_view, int B, int P, int dim, void* stream);
int bd_gather_query_rows_f32_varlen(const float* x, const int32_t* view_start, const int32_t* query_view, float* out, int B, int P,
                                    int dim, void* stream);
int bd_gather_query_tokens_varlen(const float* x, const int32_t* view_start, const int32_t* query_view, void* out16, int64_t out_plane,
                                  int B, int P, int dim, int prec, void* stream);

/* Segmented copy of whole views between operand tensors of ONE class: the decoder's feature operand of a batch (uniform or ragged),
 * assembled from a device-resident bank of cached reference views and the views the encoder produced in this forward -- in place of
 * re-encoding an object's references for every query (BoxDreamerModel.py:274-285).  Output view v is bank view s = src[v] when
 * s >= 0, fresh view -(s + 1) when s < 0 (src: device int32 [n_views]).  Per view: plane 0 (P * dim elements), and for the two-plane
 * classes plane 1 -- P * dim 16-bit elements (BF16X3, F16X3), or P * dim BYTES for F16C8, whose lo8 plane is packed row-wise at the
 * head of plane-1 storage: view v lives at byte v * P * dim of plane 1 in all three tensors, whatever their plane offsets.  *_plane:
 * offset of plane 1 in 16-bit elements (ignored by one-plane classes), a multiple of 8 and at least views * P * dim.  Classes:
 * BD_PREC_BF16, _F16, _FP8, _BF16X3, _F16X3, _F16C8 (BD_ERR_DTYPE otherwise).  bank32 / fresh32 / out32: optional fp32 copies
 * [views, P, dim] moved the same way; out32 == NULL: no fp32 traffic.  An entry of src outside its table (s >= bank_views,
 * -(s + 1) >= n_fresh) leaves that view's output bytes untouched and the others are copied (bd_attention_varlen's convention for
 * inconsistent device data).  Checked before any launch: NULL pointers (a table may be NULL when its view count is 0) BD_ERR_NULL;
 * negative counts, a plane 1 that starts inside plane 0, an out tensor whose bytes overlap bank's or fresh's BD_ERR_SHAPE; P * dim % 16 != 0, a pointer or a plane offset that is not
 * 16-byte aligned BD_ERR_ALIGN; n_views == 0 returns BD_OK without a launch.  One launch of 16-byte vector copies. */
int bd_gather_view_rows(const void* bank16, int64_t bank_plane, int bank_views, const void* fresh16, int64_t fresh_plane, int n_fresh,
                        const int32_t* src, void* out16, int64_t out_plane, int n_views, int P, int dim, int prec,
                        const float* bank32, const float* fresh32, float* out32, void* stream);

/* Assembles the decoder's ENTRY token rows of one batch (uniform or ragged) -- x = bbox_emb(patchify(bbox_feat)) + pos + adapter(feat),
 * betr.py:313-329 and :367-399 -- from a device-resident bank of finished reference rows (bd_decoder_entry_tokens) and the adapter
 * output of the views encoded in this forward, which are the query views: their rows are the query-token substitution of
 * bd_query_substitute (betr.py:286-290).  bank_x: fp32 [bank_views, P, dim]; rgb_fresh: fp32 [n_fresh, P, dim] (the adapter's
 * LayerNorm output); pos: fp32 [P, dim]; query_token: fp32 [dim]; src: device int32 [n_views]; x_out: fp32 [n_views, P, dim].
 * Output view v with s = src[v]:  s >= 0: x_out[v] = bank_x[s], moved as 16-byte vectors (NaN payloads pass through);
 * s < 0, f = -(s + 1): x_out[v][tok][d] = (query_token[d] + rgb_fresh[f][tok][d]) + pos[tok][d] -- bd_query_substitute's
 * association order, the same bits.  bd_gather_view_rows' src convention and its rule for inconsistent device data: an entry
 * s >= bank_views, or f >= n_fresh, leaves that view's output bytes untouched and the other views are written.
 * Checked before any launch: NULL pointers (bank_x / rgb_fresh may be NULL when their view count is 0) BD_ERR_NULL; negative counts,
 * P <= 0, dim <= 0, x_out overlapping an input BD_ERR_SHAPE; P * dim % 4 != 0 or a pointer that is not 16-byte aligned (src: 4-byte)
 * BD_ERR_ALIGN; n_views == 0 returns BD_OK without a launch.  One launch; the grid is sized by the batch's views. */
int bd_assemble_entry_tokens(const float* bank_x, int bank_views, const float* rgb_fresh, int n_fresh, const float* pos,
                             const float* query_token, const int32_t* src, float* x_out, int n_views, int P, int dim, void* stream);

/* BETR.unpatchify + 2*sigmoid-1 (betr.py:230-247, 432-435): proj fp32 [B*P, p*p*c] ->
 * logits, heat fp32 [B, c, size, size]. */
int bd_unpatchify_sigmoid(const float* proj, float* logits, float* heat, int B, int channels, int size,
                          int patch, void* stream);

/* Heatmap corner decode (box_utils.py:75-110): per (b, c): top-k of (heat+1)/2 over size*size
 * (ties: lower index first), corner = unweighted mean of the k integer (x, y).
 * kp_px, kp_norm: fp32 [B*C, 2]; topk_idx: int32 [B*C, k] in selection order (may be NULL). */
int bd_decode_topk(const float* heat, int n_maps, int height, int width, int k, float* kp_px,
                   float* kp_norm, int32_t* topk_idx, void* stream);

/* Corner heatmap rendering, the producer of `bbox_feat` one step BEFORE the path ("next" row f2):
 * make_bbox_features(type='heatmap'), src/datasets/utils/base/bbox_utils.py:263-303 (called per sample at
 * src/datasets/base.py:689-693).  corners: fp32 [n_groups*group, 8, 2] pixel (x, y); each consecutive run of `group`
 * views is one reference call (the per-corner max spans the run).  out: [n_groups*group, 8, height, width] in
 * out_dtype (BD_DTYPE_*). */
int bd_render_corner_heatmaps(const float* corners, int n_groups, int group, int height, int width,
                              void* out, int out_dtype, void* stream);

/* Pose from decoded corners on the GPU ("next" row f3): DLT + Levenberg-Marquardt PnP, one pose per thread in fp64,
 * the algorithm of cv2.solvePnP(SOLVEPNP_ITERATIVE) for non-planar points as restated in boxdreamer_amd/pnp.py
 * (replaces the per-sample host loop of src/models/utils/box_utils.py:139-199).  kp_px: fp32 [n_poses, n_points, 2] pixel
 * coordinates; pts3: fp32 [n_poses, n_points, 3]; K: fp32 [n_poses, 3, 3]; poses: fp32 [n_poses, 4, 4] = [R|t; 0 0 0 1],
 * all zeros where the solve fails -- a non-finite input, a degenerate DLT, or a pose that leaves a point at or behind the camera
 * plane, or an iteration that has not converged at its cap.  6 <= n_points <= 64.  iters >= 100 is a CAP on the LM iterations (the
 * callers pass 400): the iteration stops where the decrease its linearisation promises falls below 1e-12 of the error under weak damping
 * (about ten iterations on clean corners), and a solve that reaches the cap without that has no pose.  iters < 100 is a BUDGET: the
 * iterate is returned as it stands (0: the DLT start alone).
 * (One wavefront per pose instead of one thread: bd_solve_pnp_wave below.) */
int bd_solve_pnp(const float* kp_px, const float* pts3, const float* K, int n_poses, int n_points, int iters,
                 float* poses, void* stream);
/* The same solve with ONE WAVEFRONT per pose (grid = n_poses workgroups of 64 lanes, all state in LDS and registers, fp64, every sum
 * in a fixed order: a pose's bits do not depend on n_poses or on its place in the batch); replaces the same per-sample host loop of
 * src/models/utils/box_utils.py:139-199.  Same argument contract as bd_solve_pnp: 6 <= n_points <= 64, BD_ERR_NULL / BD_ERR_SHAPE
 * before any launch, an all-zero 4 x 4 where the solve fails.  It lands on the same minimum as bd_solve_pnp[_host], not on the same
 * bits (the 12 x 12 Jacobi runs in a round-robin order).  rms_px: fp32 [n_poses], may be NULL: root mean square over the n_points
 * points of the PIXEL reprojection error sqrt(sum((u - u^)^2 + (v - v^)^2) / n_points) of the returned pose, 0 where it fails. */
int bd_solve_pnp_wave(const float* kp_px, const float* pts3, const float* K, int n_poses, int n_points, int iters,
                      float* poses, float* rms_px /* may be NULL */, void* stream);
/* The same solver on the HOST (all pointers are host pointers, no GPU work): `n_threads` worker threads share the poses
 * (<= 0: one per 4 poses, at most 16).  The default pose solver of the facade when OpenCV is not importable -- the PnP post-solve
 * stays on the host CPU (north_star), without the per-sample Python loop of src/models/utils/box_utils.py:139-199. */
int bd_solve_pnp_host(const float* kp_px /*[host]*/, const float* pts3 /*[host]*/, const float* K /*[host]*/, int n_poses, int n_points,
                      int iters, float* poses /*[host]*/, int n_threads);

/* RANSAC PnP over the n_rounds x 8 corners of the dense multi-round mode, on the GPU (additive in ABI 9): replaces the
 * cv2.solvePnPRansac call, its ITERATIVE fall-back and the per-sample host loop around them, src/models/utils/box_utils.py:202-300.
 * Observation i of a sample is round i / 8, corner i % 8 (n_rounds * 8 <= 64).  Two launches on `stream`:
 *   pnp_ransac_hyp_kernel    n_samples * n_trials workgroups of one wavefront: the trial's 6 picked observations are solved with
 *                            bd_solve_pnp_wave's solver (hyp_iters LM iterations; the host scheme uses 5), every observation is scored by its
 *                            fp64 pixel error against reproj_err (a point behind the camera is never an inlier); per hypothesis the
 *                            workspace gets the inlier count (-1: solve failed), the inliers' error sum in index order and a 64-bit mask;
 *   pnp_ransac_final_kernel  one wavefront per sample: the selection of boxdreamer_amd/pnp.py solve_pnp_ransac in batches of 32 trials
 *                            (a batch's best = highest count, ties to the lowest index; it replaces the running best on a higher count
 *                            or an equal count with a lower error sum; need = ceil(log(1 - confidence) / log(max(1 - w^6, 1e-300)))
 *                            at inlier ratio w; stop at trials >= min(need, n_trials) or w >= 1), then the solve (final_iters, a cap; 400 in the
 *                            host scheme) of the best hypothesis' inliers compacted in index order -- of ALL observations when the best count
 *                            is below 6, the inliers cover fewer than 6 distinct corners, an observation is not finite, or that solve fails.
 * No atomics, no workgroup waits for another, every sum in index order: a sample's bits depend neither on n_samples nor on its row.
 * picks: DEVICE int32 [n_trials, 6] observation indices (boxdreamer_amd/pnp.py: ransac_picks); an entry outside [0, n_rounds * 8) is
 * clamped into it.  poses: fp32 [n_samples, 4, 4], zeros on failure; inliers: uint8 [n_samples, n_rounds * 8], the observations the pose was
 * solved on (all zero on failure); rms_px (may be NULL): fp32 [n_samples], pixel RMS of the pose over those observations, 0 on failure;
 * info (may be NULL): int32 [n_samples, 4] = trials used, index of the best hypothesis or -1, set entries of `inliers`, path
 * (0 = inliers, 1 = all observations, 2 = failed).  workspace: bd_solve_pnp_ransac_workspace_bytes(n_samples, n_trials) device bytes.
 * Before any launch: BD_ERR_NULL for a NULL pointer other than rms_px / info; BD_ERR_SHAPE for n_samples <= 0, n_rounds outside
 * [1, 8], n_trials <= 0, negative iteration counts, n_samples * n_trials above INT_MAX or a workspace that is too small.
 * Parity against OpenCV's solvePnPRansac (its own sampler and minimal solver) is un-pinned, like the host form's. */
size_t bd_solve_pnp_ransac_workspace_bytes(int n_samples, int n_trials);
int bd_solve_pnp_ransac_wave(const float* kp_px /* [n_samples, n_rounds, 8, 2] */, const float* bbox_3d /* [n_samples, 8, 3] */,
                             const float* K /* [n_samples, 3, 3] */, const int32_t* picks /* device [n_trials, 6] */, int n_samples,
                             int n_rounds, int n_trials, float reproj_err, float confidence, int hyp_iters, int final_iters, float* poses,
                             unsigned char* inliers /* [n_samples, n_rounds * 8] */, float* rms_px /* may be NULL */,
                             int32_t* info /* [n_samples, 4], may be NULL */, void* workspace, size_t workspace_bytes, void* stream);
/* The same two stages on the HOST (all pointers are host pointers, no GPU work, no workspace): the lanes of a wavefront run in a loop,
 * hypotheses and samples are dealt out to the worker threads of bd_solve_pnp_host (n_threads <= 0: 16).  Same checks, same outputs;
 * replaces the same lines of src/models/utils/box_utils.py:202-300.  Not the default host path of the dense mode
 * (pnp.solve_pnp_ransac is): the twin the device form is tested against. */
int bd_solve_pnp_ransac_host(const float* kp_px, const float* bbox_3d, const float* K, const int32_t* picks, int n_samples, int n_rounds,
                             int n_trials, float reproj_err, float confidence, int hyp_iters, int final_iters, float* poses,
                             unsigned char* inliers, float* rms_px /* may be NULL */, int32_t* info /* may be NULL */, int n_threads);

/* Dense-reference mode ("next" row f4): DINO-feature reference selection, src/models/utils/matching.py:64-174
 * (`dino_matching`, called from process_dense_input, src/models/utils/data_processing.py:179-225).
 * feats: fp32 [B, T, L, D] patch features of every view (the encoder output); images: [B, T, 3, H, W] RGB crops in [0, 1]
 * (img_dtype BD_DTYPE_*); query_view[b]: index of the query view.  scores: fp32 [B, T-1], one per reference in view order
 * = mean over the L x L patch pairs of the masked cosine similarity with the reference's -1e4 fill, evaluated in closed
 * form.  sums [B*T, D] and counts [B*T] are caller-provided scratch (per-view foreground feature sum / patch count). */
int bd_dino_match_scores(const float* feats, const void* images, int img_dtype, const int32_t* query_view, int B, int T,
                         int L, int D, int H, int W, float lum_threshold, float* sums, float* counts, float* scores,
                         void* stream);

/* Boolean top-k mask per row of scores [B, N] (matching.py:167-173): k largest, ties to the lower index. mask: uint8 [B, N].
 * Every row gets exactly k ones; -inf scores rank below every finite score (and among themselves by index).  NaN scores are
 * unordered and never selected: callers pass NaN-free rows (bd_dino_match_scores writes none). */
int bd_topk_mask(const float* scores, int B, int N, int k, unsigned char* mask, void* stream);

/* Dense-reference mode over a bank of cached views (cache.RefFeatureBank): a pair's score needs only each view's foreground feature
 * sum (D floats) and foreground patch count, so a view is summarised ONCE, when it enters the bank, and a forward scores, selects and
 * names its references without the views' features or crops.
 *
 * bd_match_view_sums: the per-view pass of bd_dino_match_scores (the same kernel) over V free-standing views.  feats: fp32 [V, L, D];
 * images: [V, 3, H, W] (img_dtype BD_DTYPE_*); sums: fp32 [V, D]; counts: fp32 [V].  A view's sums / counts are bit-identical to the
 * scratch bd_dino_match_scores fills for it.  The same checks as bd_dino_match_scores; V < 0 BD_ERR_SHAPE, V == 0 BD_OK without a
 * launch. */
int bd_match_view_sums(const float* feats, const void* images, int img_dtype, int V, int L, int D, int H, int W,
                       float lum_threshold, float* sums, float* counts, void* stream);

/* bd_match_select_rows: score, top-k and compaction in ONE launch, one workgroup per sample.  bank_sums [R, D] / bank_counts [R]: the
 * summaries of the bank's views; q_sums [B, D] / q_counts [B]: those of the B query views; rows: device int32 [B, N_max], the bank
 * row of every reference slot; n_refs: device int32 [B], k <= n_refs[b] <= N_max <= 1024 references per sample.
 * scores: fp32 [B, N_max], bit-identical to bd_dino_match_scores' score of the same pair (same summation order, zero-pairs rule and
 * nan_to_num); -inf for the slots n >= n_refs[b], which are never read through `rows` and never selected, and for a `rows` entry
 * outside [0, R).  sel: int32 [B, k], the selected slots in ascending order -- bd_topk_mask's rule: largest score, ties to the lower
 * slot, -inf an ordinary value.  src: int32 [B * (k + 1)], bd_gather_view_rows' source table of the (B, k + 1) batch: per sample the
 * selected bank rows in slot order, then -(b + 1), fresh view b (the query).
 * Inconsistent device data reads and writes nothing out of bounds: n_refs[b] is clamped into [0, N_max]; where that leaves fewer
 * than k slots the remaining entries of sel[b] are -1 and their src entries 0x7fffffff, which bd_gather_view_rows skips, as is the
 * src entry of a selected slot whose row is outside the bank.
 * Checked before any launch: NULL pointers BD_ERR_NULL; B <= 0, R < 0, N_max <= 0, N_max > 1024, k <= 0, k > N_max, L <= 0, D <= 0
 * BD_ERR_SHAPE. */
int bd_match_select_rows(const float* bank_sums, const float* bank_counts, int R, const float* q_sums, const float* q_counts,
                         const int32_t* rows, const int32_t* n_refs, int B, int N_max, int L, int D, int k,
                         float* scores, int32_t* sel, int32_t* src, void* stream);

/* Dense multi-round decode over a bank that keeps its views' poses (cache.RefFeatureBank(keep_poses=True)): the two tables the
 * facade needs between the selection above and the decoder, written on the device from what the device selected, so that nothing
 * waits for it.  Both run one workgroup per sample without atomics; a sample's outputs do not depend on the rest of the batch.
 * rows: device int32 [B, N_max] as above; cand: device int32 [B, k], bd_match_select_rows' `sel` (reference slots, ascending, -1:
 * none); R: the bank's views in use.  A candidate whose slot is outside [0, N_max), or whose row is outside [0, R), is invalid: its
 * src entry is 0x7fffffff, which bd_gather_view_rows and bd_assemble_entry_tokens skip, and `rows` is not read for it.
 *
 * bd_round_sources: the source table of the (B * rounds, sub + 1) batch, rounds = ceil(k / sub).  src / view: int32
 * [B * rounds * (sub + 1)].  Pseudo-sample q = b * rounds + r, position j < sub, c = r * sub + j: src = the bank row of candidate c
 * and view = c where c < k; src = zero_row (the bank's all-zero view, cache.RefFeatureBank.zero_row) and view = -1 where the last
 * round runs out.  Position sub is the query: view = k, src = -(q + 1) when per_round_query != 0 (bd_decoder_forward_entry wants one
 * fresh view per pseudo-sample, in order) and -(b + 1) otherwise (bd_gather_view_rows may name one fresh view `rounds` times).
 * `view` is a view position of the filtered (B, k + 1) batch: the facade re-packs bbox_feat / images with it by integer indexing.
 * Checked before any launch: NULL pointers BD_ERR_NULL; B <= 0, R < 0, N_max <= 0, k <= 0, k > 1024, sub <= 0, a table of more than
 * 2^31 - 1 entries, and k % sub != 0 with zero_row outside [0, R) BD_ERR_SHAPE (zero_row is not read when no round is padded). */
int bd_round_sources(const int32_t* rows, const int32_t* cand, int R, int B, int N_max, int k, int sub, int zero_row,
                     int per_round_query, int32_t* src, int32_t* view, void* stream);

/* bd_pose_select_rows: the fine level's choice (data_utils.py:97-135, fetch_neighbors_by_pose_similarity) among the k candidates, from
 * the bank's poses.  bank_poses: fp32 [>= R, 4, 4]; pred: fp32 [B, 4, 4], the coarse pose (bd_solve_pnp_ransac_wave's output, or the
 * host RANSAC's, uploaded); 1 <= fk <= k <= 1024.  Distance of candidate c, with P = pred[b], G = bank_poses[row of c]:
 *     d = acos(clamp((tr - 1) / 2, -1, 1)) + sqrt(ss)
 *     tr = trace(P_R G_R^T) = sum over i = 0..2, j = 0..2 (i outer) of P[i][j] * G[i][j]
 *     ss = sum over i = 0..2 of (P[i][3] - G[i][3])^2
 * evaluated in fp64 from the fp32 inputs, each sum sequential from 0.0 in the order written, every operation rounded on its own (no
 * contraction), the clamp by comparison (a NaN stays a NaN), and d rounded ONCE to fp32.  A failed coarse pose (all zeros) and
 * non-finite poses are ordinary inputs.
 * dist: fp32 [B, k], +inf for an invalid candidate.  fine_pos: int32 [B, fk], the positions in `cand` of the fk valid candidates
 * that rank first, in ascending position order (the order filter_by_neighbor_mask keeps).  Ranking is on the stored fp32 value:
 * smaller first, ties to the lower position, +inf an ordinary value, NaN after every number and among NaNs by position.  src: int32
 * [B * (fk + 1)]: per sample those candidates' bank rows, then -(b + 1), fresh view b (the query).  With fewer than fk valid
 * candidates the remaining entries of fine_pos[b] are -1 and their src entries 0x7fffffff.
 * Checked before any launch: NULL pointers BD_ERR_NULL; B <= 0, R < 0, N_max <= 0, k <= 0, k > 1024, fk <= 0, fk > k BD_ERR_SHAPE. */
int bd_pose_select_rows(const float* bank_poses, int R, const float* pred, const int32_t* rows, const int32_t* cand, int B,
                        int N_max, int k, int fk, float* dist, int32_t* fine_pos, int32_t* src, void* stream);

/* Eval-step pose metrics: the per-sample values of Metrics.compute_metrics, src/lightning/utils/metrics/metric_utils.py:97-128
 * (query_pose_error :162-211, process_single_bs_2d :255-306 with project_optimized :224-239, process_single_bs_add :331-424).
 * Per pose b (the query view, gathered by the caller): pred_poses / original_poses fp32 [n_poses, 4, 4], scale fp32 [n_poses, 3],
 * coordinate_transform fp32 [n_poses, 4, 4], original_intrinsics fp32 [n_poses, 3, 3].  The prediction is composed as the
 * reference does (:480-483, :282-283): pred[:3, 3] *= scale element-wise, then pred @ coordinate_transform.
 * points: fp32 [*, 3], one packed buffer of model points; pose b uses pt_count[b] points from row pt_offset[b] (int64 / int32
 * device arrays), so one batch can mix objects.  max_points >= every pt_count[b] (a pose with a count outside [1, max_points]
 * gets NaN point metrics).  t_scale: 0 = null, 1 = 'm' (t_err x 100), 2 = 'mm' (t_err / 10).
 * out: fp64 [n_poses, 6] = R_err (deg), t_err, inplane_R_err (deg), proj2d (px), add, adds -- ADD-S is the exact nearest-neighbour
 * mean (what scipy's cKDTree returns), by direct fp32 differences; the per-pose scalars and all sums are fp64.  Deterministic:
 * a pose's outputs are bit-identical whatever else is in the batch.  workspace: bd_pose_metrics_workspace_bytes(n_poses, max_points)
 * bytes, caller-owned scratch. */
size_t bd_pose_metrics_workspace_bytes(int n_poses, int max_points);
int bd_pose_metrics(const float* pred_poses, const float* original_poses, const float* scale, const float* coordinate_transform,
                    const float* original_intrinsics, const float* points, const int64_t* pt_offset, const int32_t* pt_count,
                    int n_poses, int max_points, int t_scale, void* workspace, size_t workspace_bytes, double* out, void* stream);

/* Crop + ToTensor + antialiased resize of raw frames: what the reference's dataset does per view on the host
 * (src/datasets/utils/preprocess.py:123-199 pad_and_resize_image, :202-274 _crop_image with bbox_obj, called from
 * src/datasets/base.py:541-566; the transform is ToTensor + Resize(img_size, antialias=True)).
 * frames: device uint8 [n_frames, H, W, 3] (HWC, RGB), row_stride / frame_stride in BYTES (row_stride >= 3 W; no alignment is
 * required of the base or the strides).  boxes: device int32 [n_crops, 4] = x0 y0 x1 y1, the integer crop window [x0, x1) x [y0, y1),
 * square (x1 - x0 == y1 - y0 >= 1); it may leave the frame on any side, pixels outside the frame are 0.  frame_idx: device int32
 * [n_crops], the frame each crop reads, or NULL (crop i reads frame i; then n_crops <= n_frames).  keep_boxes: device int32
 * [n_crops, 4] or NULL: pixels with x < kx0, x > kx1, y < ky0 or y > ky1 count as 0 (both edges inclusive: ImageDraw.rectangle).
 * The crop (side s) is resized to out_size x out_size as ATen's _upsample_bilinear2d_aa with align_corners = false does it:
 * separable triangle filter, scale = s / out_size, support = max(scale, 1), centre c_i = scale (i + 0.5), taps
 * [max(0, int(c_i - support + 0.5)), min(s, int(c_i + support + 0.5))), weight max(0, 1 - |j - c_i + 0.5| / support), normalised to
 * sum 1 per output sample; the window is clipped to the CROP (zero padding takes part in the filter).  Tap geometry and weights are
 * evaluated in fp64, sums are fp32.  The result is value / 255, clamped to [0, 1], rounded once to out_dtype (BD_DTYPE_F32 / F16 /
 * BF16) and stored CHW: out [n_crops, 3, out_size, out_size], contiguous.
 * Boxes are device data and cannot be rejected here: a crop whose box is not square, has a side < 1 or > 2^20, or whose frame index
 * lies outside [0, n_frames) is written as ZEROS.  out_size <= 512, n_crops <= 65535 (BD_ERR_SHAPE otherwise).  One launch, no
 * workspace, no synchronisation; a crop's bits do not depend on the other crops of the launch. */
int bd_crop_resize_frames(const uint8_t* frames, int n_frames, int H, int W, int64_t row_stride, int64_t frame_stride,
                          const int32_t* boxes, const int32_t* frame_idx, const int32_t* keep_boxes, int n_crops, int out_size,
                          void* out, int out_dtype, void* stream);

/* The same crop + resize on frames in the layout a camera, a compositor or a video decoder delivers.  bd_crop_resize_frames is
 * the BD_PIXEL_RGB case of this entry: the same kernel instance and launch.  Only the step that turns source bytes into pixels
 * differs per format (csrc/pixel_format.h, shared with bd_frames_to_rgb_host); the filter behind it sees the same pixels, so the
 * result is BIT FOR BIT bd_crop_resize_frames on the frame converted to packed RGB, and only pixels under a crop are converted.
 *   BD_PIXEL_RGB / _BGR    uint8 [n_frames, H, W, 3], row_stride >= 3 W
 *   BD_PIXEL_RGBA / _BGRA  uint8 [n_frames, H, W, 4], row_stride >= 4 W; the fourth byte is ignored
 *   BD_PIXEL_NV12          H and W even; H rows of W luma bytes from the frame's first byte, then, chroma_offset bytes from the
 *                          frame's first byte, H / 2 rows of W / 2 interleaved (U, V) pairs, both planes with row_stride >= W;
 *                          chroma_offset >= H * row_stride (a decoder that pads the luma plane's height is read in place).
 *                          Chroma is sampled nearest: pixel (x, y) uses pair (x >> 1, y >> 1).
 * No alignment is required of the base, the strides or chroma_offset.  chroma_offset and the coefficients are read for NV12 only.
 * NV12 -> RGB, int32, >> arithmetic:  y = Y - y_off, u = U - 128, v = V - 128,
 *   R = clamp((cy y + crv v + 32768) >> 16, 0, 255), G = clamp((cy y - cgu u - cgv v + 32768) >> 16, 0, 255),
 *   B = clamp((cy y + cbu u + 32768) >> 16, 0, 255)
 * with coefficients floor(x 65536 + 0.5) of cy = 255/219 | 1, crv = 2 (1 - Kr) s, cbu = 2 (1 - Kb) s, cgu = 2 Kb (1 - Kb) / Kg s,
 * cgv = 2 Kr (1 - Kr) / Kg s, s = 255/224 | 1 (limited | full range), Kg = 1 - Kr - Kb:
 *                   cy     crv    cgu    cgv    cbu  y_off
 *   BT.601 limited  76309 104597  25675  53279 132201  16        BT.601 full  65536  91881  22553  46802 116130  0
 *   BT.709 limited  76309 117489  13975  34925 138438  16        BT.709 full  65536 103206  12276  30679 121609  0
 * Before any launch, next to bd_crop_resize_frames' checks: an unknown format BD_ERR_DTYPE; row_stride below one row of the format,
 * NV12 with odd H or W, chroma_offset < H * row_stride, a coefficient outside [0, 2^20] or y_off outside [0, 255] BD_ERR_SHAPE. */
#define BD_PIXEL_RGB 0
#define BD_PIXEL_BGR 1
#define BD_PIXEL_RGBA 2
#define BD_PIXEL_BGRA 3
#define BD_PIXEL_NV12 4
int bd_crop_resize_frames_fmt(const uint8_t* frames, int n_frames, int H, int W, int64_t row_stride, int64_t frame_stride,
                              const int32_t* boxes, const int32_t* frame_idx, const int32_t* keep_boxes, int n_crops, int out_size,
                              void* out, int out_dtype, int format, int64_t chroma_offset, int cy, int crv, int cgu, int cgv,
                              int cbu, int y_off, void* stream);
/* A whole frame of any format to packed RGB on HOST pointers, in the calling thread, with the kernel's per-pixel text: out uint8
 * [n_frames, H, W, 3], contiguous.  The same layout checks and codes; needs no device. */
int bd_frames_to_rgb_host(const uint8_t* frames, int n_frames, int H, int W, int64_t row_stride, int64_t frame_stride, int format,
                          int64_t chroma_offset, int cy, int crv, int cgu, int cgv, int cbu, int y_off, uint8_t* out);

/* The two ends of a streaming pose step (boxdreamer_amd/stream.py), one launch each, so that a captured step holds two graph nodes
 * where the facade enqueues a few dozen small torch kernels per frame.  Each is ceil(n / 64) wavefronts, one sample per lane: no
 * workspace, no atomics, no synchronisation.  The *_host forms run the SAME arithmetic (written once, __host__ __device__) on host
 * pointers, in the calling thread: the twin the device forms are tested against, bit for bit.  Floating-point contraction is off
 * in it.  Before any launch, for all four: a NULL pointer BD_ERR_NULL; n < 0, n > 65535 or out_size < 1 BD_ERR_SHAPE; n == 0
 * returns BD_OK without a launch.
 *
 * Windows: replaces the torch forms of preprocess.square_bbox(box, padding) + preprocess.crop_intrinsics(K, window, out_size) (the
 * reference's square_bbox / _crop_image / adjust_intrinsic_matrix, src/datasets/utils/preprocess.py:22-45, :253-259, :277-300;
 * about 20 fp64 torch kernels), bit for bit.  det_boxes fp32 [n, 4] = x0 y0 x1 y1 detector boxes, K fp32 [n, 3, 3] intrinsics of
 * the full frame.  Everything is fp64 from the fp32 inputs, in those functions' operation order: center = (b0 + b2) / 2, extent =
 * (b2 - b0) / 2, size = max(ex, ey) * (1 + padding), lt = trunc(center - size), wh = trunc((center + size) - (center - size)),
 * windows int32 [n, 4] = lt, lt + wh; then sx = out_size / (x1 - x0) as torch evaluates `float / tensor`, (1 / (x1 - x0)) *
 * out_size, k00 *= sx, k02 = k02 * sx - x0 * sx (likewise y), the other entries copied: K_crop fp32 [n, 3, 3], rounded once.  A window whose sides differ after truncation is written as computed (the
 * crop kernel writes zeros for it); a non-finite box or a coordinate outside int32 gives the window 0 0 0 0. */
int bd_stream_windows(const float* det_boxes, const float* K, double padding, int out_size, int32_t* windows, float* K_crop, int n,
                      void* stream);
int bd_stream_windows_host(const float* det_boxes, const float* K, double padding, int out_size, int32_t* windows, float* K_crop,
                           int n);

/* Results: replaces the indexing, cat, nan_to_num and clone the facade enqueues after the pose solve (boxdreamer_amd/model.py:
 * _process_evaluation) and the demo loop's per-frame projections (src/demo/demo.py:1500-1564).  poses fp32 [n, 4, 4] and rms_px
 * fp32 [n] as the wave solver leaves them (an all-zero matrix on failure), kp_px fp32 [n, 8, 2] decoded corners in crop pixels,
 * windows / out_size the crop they were decoded in, K fp32 [n, 3, 3] of the FULL frame, bbox_3d fp32 [n, 8, 3].
 * rows fp32 [n, BD_STREAM_ROW_FLOATS]:
 *   [0, 16)  the pose, row-major, NaN and +-inf replaced by 0 (torch.nan_to_num(nan=0, posinf=0, neginf=0));
 *   [16]     rms_px;
 *   [17]     ok: 1 when pose[3][3] == 1 and all 16 entries are finite, else 0;
 *   [18, 34) kp_px, copied;
 *   [34, 50) the corners in full-frame pixels, x = x0 + kp_x * (x1 - x0) / out_size (likewise y; the inverse of the crop's
 *            intrinsics, no half-pixel term), fp64, rounded once;
 *   [50, 66) the 3-D box projected into the full frame with the pose: Xc = ((r0 x + r1 y) + r2 z) + t, u = ((k00 xc + k01 yc) +
 *            k02 zc) / zc, v = (k11 yc + k12 zc) / zc in fp64, in that order, rounded once; a point with zc <= 0 gives NaN for
 *            both; all 16 values are 0 when ok == 0. */
#define BD_STREAM_ROW_FLOATS 66
int bd_stream_results(const float* poses, const float* rms_px, const float* kp_px, const int32_t* windows, const float* K,
                      const float* bbox_3d, int out_size, float* rows, int n, void* stream);
int bd_stream_results_host(const float* poses, const float* rms_px, const float* kp_px, const int32_t* windows, const float* K,
                           const float* bbox_3d, int out_size, float* rows, int n);

/* bd_stream_track_windows: a second form of the step's first node (stream.PoseStream(track_boxes=True)): every object's crop box comes
 * from its OWN last pose while that pose is trusted, so a session needs no detector box per frame.  It replaces the reference demo's
 * offline segmentation pass over the whole video (src/demo/demo.py:379-476, the box/ files its loop reads) by the rule the reference's
 * OnePose data derives its boxes with (src/datasets/onepose.py:437-455: the min / max of the 8 projected corners of the 3-D box).  One
 * object per lane, 64 lanes per workgroup, like bd_stream_windows; the _host form runs the same __host__ __device__ arithmetic.
 * prev_rows fp32 [n, BD_STREAM_ROW_FLOATS]: the LAST step's result rows (read before this step's bd_stream_results overwrites them);
 * bbox_3d fp32 [n, 8, 3]; K fp32 [n, 3, 3] of this frame; det_boxes fp32 [n, 4]; det_valid int32 [n]: nonzero = a detection is
 * offered; force int32 [n]: nonzero = distrust this object's last pose on this step; state_box fp32 [n, 4]: the box used last step,
 * READ AND WRITTEN (an object touches its own four floats only).
 *   projection  the 8 corners through prev_rows[b][0:16] and K[b], the arithmetic of the row's box slots [50, 66) (one function
 *               serves both); a corner with zc <= 0 is NaN;
 *   tracked box (min u, min v, max u, max v) of those fp32 values;
 *   valid       all 16 values finite, and in fp64: min(max, frame) - max(min, 0) >= min_side_px on both axes (the extent clipped to
 *               [0, frame_w] x [0, frame_h]), max - min <= max_side_px on both axes (the unclipped extent);
 *   trusted     prev ok == 1.0f, prev rms_px <= max_rms_px (a comparison: a NaN rms fails it), force[b] == 0 and valid -- the rule of
 *               bd_stream_select_rows plus the geometry;
 *   source      trusted: the tracked box, NOT clipped (the crop kernel pads with black), BD_STREAM_BOX_TRACKED; else det_valid[b] != 0:
 *               det_boxes[b] as given, BD_STREAM_BOX_DETECTOR; else state_box[b], BD_STREAM_BOX_HELD.
 * Written per object: windows int32 [n, 4] and K_crop fp32 [n, 3, 3] exactly as bd_stream_windows writes them for that box (a
 * detector-sourced object gets its bits); state_box: the box; box_src int32 [n]: the source; keep_boxes int32 [n, 4] (may be NULL: not
 * written): the four box components truncated towards zero in fp64 -- the object's own box, not squared (the reference's bbox_obj,
 * src/datasets/base.py:550-552) -- all zeros when one of them is not finite or leaves int32; track fp32 [n, 5] (may be NULL: not
 * written): x0 y0 x1 y1 of the box and the source as a float, the tail a session copies to the host with its result rows.
 * Checked before any launch: a NULL pointer (but keep_boxes, track) BD_ERR_NULL; n < 0, n > 65535, out_size < 1, frame_h < 1,
 * frame_w < 1, min_side_px or max_side_px not positive (a NaN included) BD_ERR_SHAPE; n == 0 returns BD_OK without a launch. */
#define BD_STREAM_BOX_DETECTOR 0
#define BD_STREAM_BOX_TRACKED 1
#define BD_STREAM_BOX_HELD 2
int bd_stream_track_windows(const float* prev_rows, const float* bbox_3d, const float* K, const float* det_boxes,
                            const int32_t* det_valid, const int32_t* force, float* state_box, double padding, int out_size, int frame_h,
                            int frame_w, float max_rms_px, double min_side_px, double max_side_px, int32_t* windows, float* K_crop,
                            int32_t* box_src, int32_t* keep_boxes /* may be NULL */, float* track /* may be NULL */, int n, void* stream);
int bd_stream_track_windows_host(const float* prev_rows, const float* bbox_3d, const float* K, const float* det_boxes,
                                 const int32_t* det_valid, const int32_t* force, float* state_box, double padding, int out_size,
                                 int frame_h, int frame_w, float max_rms_px, double min_side_px, double max_side_px, int32_t* windows,
                                 float* K_crop, int32_t* box_src, int32_t* keep_boxes /* may be NULL */, float* track /* may be NULL */,
                                 int n);

/* bd_stream_select_rows: a streaming step's choice of references, on the device (stream.PoseStream(select_k=...)): each of the B
 * tracked objects owns a database of views, and every frame k of them are named in the decoder's source table by ONE launch, one
 * workgroup (4 waves) per object -- so a captured step replays unchanged while its references change.  Like bd_match_select_rows and
 * bd_pose_select_rows: no atomics on floating-point data, every sum in index order (an object's bits do not depend on the batch),
 * inconsistent device data reads and writes nothing out of bounds (n_refs[b] is clamped into [0, N_max], `rows` is not read past it).
 * sums fp32 [R, D], counts fp32 [R], poses fp32 [R, 4, 4]: the session's private copies of the database views' match summaries
 * (bd_match_view_sums) and poses; poses may be NULL when rule == BD_STREAM_SELECT_DINO (dist may then be NULL too and is not
 * written).  q_sums fp32 [B, D], q_counts fp32 [B]: bd_match_view_sums of this frame's query crops.  prev_rows fp32
 * [B, BD_STREAM_ROW_FLOATS]: the previous step's result rows (bd_stream_results: the pose at [0, 16), rms_px at [16], ok at [17]).
 * rows int32 [B, N_max]: the private row of every database slot; n_refs int32 [B]; force int32 [B]: nonzero = the appearance rule
 * for this object this frame.  1 <= k <= N_max <= 1024.
 * Both value arrays are computed every frame, whatever rule applies:
 *   scores fp32 [B, N_max]: bit-identical to bd_match_select_rows' for the same arguments (-inf for a slot past n_refs[b] and for a
 *     row outside [0, R));
 *   dist fp32 [B, N_max]: bit-identical to bd_pose_select_rows' dist for pred = prev_rows[:, 0:16], k = N_max and a `cand` table that
 *     names slot i at position i < n_refs[b] and -1 beyond (+inf for an invalid slot).
 * used int32 [B]: 1 when the pose rule chose, 0 when the appearance rule did.  The pose rule applies when rule ==
 * BD_STREAM_SELECT_TRACK, force[b] == 0, prev ok == 1.0f and prev rms_px <= max_rms_px -- a comparison, so a NaN rms selects the
 * appearance rule; the decision is uniform within the workgroup.
 * sel int32 [B, k], src int32 [B * (k + 1)]: the chosen slots in ascending order, and their private rows followed by -(b + 1), fresh
 * view b (the query): exactly what the kernel of the rule that applied writes -- bd_match_select_rows' sel / src (largest score,
 * ties to the lower slot, -inf an ordinary value), or bd_pose_select_rows' fine_pos / src with fk = k (smaller distance, ties to the
 * lower position, NaN last).  With fewer than k valid slots the remaining entries are -1 and 0x7fffffff.
 * Checked before any launch: a NULL pointer BD_ERR_NULL (poses with rule != DINO, dist with poses given, included); an unknown rule,
 * B <= 0, R < 0, N_max <= 0, N_max > 1024, k <= 0, k > N_max, L <= 0, D <= 0 BD_ERR_SHAPE. */
#define BD_STREAM_SELECT_DINO 0
#define BD_STREAM_SELECT_TRACK 1
int bd_stream_select_rows(const float* sums, const float* counts, const float* poses, int R, const float* q_sums,
                          const float* q_counts, const float* prev_rows, const int32_t* rows, const int32_t* n_refs,
                          const int32_t* force, int B, int N_max, int L, int D, int k, int rule, float max_rms_px,
                          float* scores, float* dist, int32_t* used, int32_t* sel, int32_t* src, void* stream);

/* ------------------------------------------------------------------------------------------
 * Whole-path entry points
 * ---------------------------------------------------------------------------------------- */
typedef struct bd_linear {
    const void* w;       /* [N, Kpad] operand dtype, nn.Linear layout; BF16X3: hi plane then lo plane */
    const float* b;      /* [N] */
    const float* wscale; /* [N] per-output-channel scale of an e4m3 weight (FP8 mode) or NULL */
    int w_qexp;          /* BD_PREC_F16C8: exponent E of the weight's e4m3 planes (q8 = e4m3(w * 2^E)) */
} bd_linear;

/* Per-Linear PROMOTION of the F16C8 family (round 4).  The F16C8 operand class keeps ~15 significant bits of every product; on
 * checkpoints with massive-activation channels / LayerNorm gain outliers a few Linears (found at load time by measurement,
 * boxdreamer_amd/calibrate.py) need the ~22 bits of the split-f16 class (BD_PREC_F16X3) to keep the heatmap logits inside 1e-3.  A set bit means:
 * THIS Linear's weight (`bd_linear.w`) is packed as BD_PREC_F16X3 planes and the whole-path entry points run it as a split-f16
 * product; the producer of its A operand (LayerNorm, attention, the fc1 epilogue) emits split-f16 planes instead of the F16C8
 * operand.  Honoured when `prec` is BD_PREC_F16C8 / BD_PREC_F16C8_QK16, and -- the same bits, the same hand-offs -- when it is BD_PREC_FP8,
 * where a set bit moves the Linear from e4m3 to BD_PREC_BF16 (the mixed e4m3 policy of configs[4]: "fp8_mixed" in
 * boxdreamer_amd/_lib.py); ignored otherwise.  With every bit set the path is
 * bit-identical to BD_PREC_F16X3_ATTN_X3. */
#define BD_PROMOTE_QKV 1
#define BD_PROMOTE_PROJ 2
#define BD_PROMOTE_FC1 4   /* implies BD_PROMOTE_FC2 (a split-f16 fc1 cannot emit the F16C8 operand) */
#define BD_PROMOTE_FC2 8
#define BD_PROMOTE_ATTN 16 /* blocks with q / k RMSNorm only: split-bf16 attention instead of the one-pass f16 attention */
/* bd_betr_weights.promote_misc / bd_dino_weights.promote_misc */
#define BD_PROMOTE_ADAPTER_FC1 1 /* BETR: feats16 must then be BD_PREC_F16X3 planes (bd_dino_weights.feats_prec); implies _FC2 */
#define BD_PROMOTE_ADAPTER_FC2 2
#define BD_PROMOTE_BBOX_EMB 4
#define BD_PROMOTE_BBOX_PROJ 8
#define BD_PROMOTE_PATCH_EMBED 1 /* DINOv2 */

typedef struct bd_block_weights {
    const float* ln1_w; const float* ln1_b; const float* ln2_w; const float* ln2_b;
    bd_linear qkv, proj, fc1, fc2;   /* DINO: LayerScale gamma pre-folded into proj / fc2 */
    const float* q_norm_w; const float* k_norm_w;   /* [head_dim]; NULL for DINOv2 */
    bd_linear qkv16;                                /* f16 single-plane copy of qkv (BD_PREC_F16C8_QK16 reads its q, k rows) or {NULL} */
    int promote;                                    /* BD_PROMOTE_* bits (F16C8 family only) */
    /* LayerNorm fold (ABI 8, F16C8 family only; all {NULL} elsewhere): the Linears that follow norm1 / norm2 with the norm's gain folded
     * into the weight columns and its shift into the bias (W' = g . W, b' = b + W beta), in the BD_PREC_F16C8 layout (qkv16_f: f16 single
     * plane), and the column sums s[n] = sum_k W'[n, k] of the ROUNDED weights each launch multiplies (qkv16_s: of the f16 copy's q, k rows) */
    bd_linear qkv_f, fc1_f, qkv16_f;
    const float* qkv_s; const float* fc1_s; const float* qkv16_s;
    int ln_resid3;    /* != 0: between folded LayerNorms the residual stream of this block may live in the 3-byte operand form only
                         (bd_gemm_args.ln_resid_in_op); 0: every residual Linear reads and writes the fp32 stream */
} bd_block_weights;

typedef struct bd_dino_weights {
    int depth, dim, heads, n_prefix, grid, patch, kpad;
    float ln_eps;
    bd_linear patch_embed;           /* [dim, kpad] */
    const float* pos_patch;          /* fp32 [grid*grid, dim] (resampled once at load) */
    const float* prefix_tokens;      /* fp32 [n_prefix, dim]: cls+pos[0], registers */
    const float* norm_w; const float* norm_b;
    const bd_block_weights* blocks;  /* [host] array of `depth` */
    int promote_misc;                /* BD_PROMOTE_PATCH_EMBED (F16C8 family only) */
    int feats_prec;                  /* operand class of feats16: 0 = the class of `prec`; BD_PREC_F16X3 (F16C8 family only) when the
                                        consumer's first Linear is promoted (BD_PROMOTE_ADAPTER_FC1) */
    int latency_mode;                /* ABI 9.  != 0: OPT-IN latency forms for calls of one or two poses (token stream <= BD_SPLITK_MAX_ROWS rows):
                                        the residual Linears of the F16C8 family may run split-K (bd_gemm_args.sk_ws; the workspace grows by
                                        the scratch region), BETR's QKV Linear runs as one F16C8 launch instead of the q,k / v column split,
                                        and attention launches of a few 256-query blocks take the 128-query kernel.  Deterministic, within the mode's tolerance, but a sample's bits then depend on
                                        whether its call took the latency forms -- 0 (default) keeps every row bit-identical across batch
                                        sizes, lanes and launch forms.  src/demo/demo.py:1501-1514 (one query + its references per frame). */
} bd_dino_weights;

typedef struct bd_betr_weights {
    int depth, dim, heads, grid, patch, box_dim, kpad;
    float ln_eps, adapter_ln_eps, rms_eps;
    bd_linear adapter_fc1, adapter_fc2, bbox_emb, bbox_proj;
    const float* pos_table;          /* fp32 [grid*grid, dim] 2-D sincos */
    const float* query_token;        /* fp32 [dim] */
    const bd_block_weights* blocks;  /* [host] */
    int promote_misc;                /* BD_PROMOTE_ADAPTER_FC1 | _ADAPTER_FC2 | _BBOX_EMB | _BBOX_PROJ (F16C8 family only) */
    int latency_mode;                /* as bd_dino_weights.latency_mode */
} bd_betr_weights;

/* DinoV2Wrapper.predict (encoder/dinov2.py:45-60): images [n_images, 3, size, size] in [0,1]
 * -> x_norm_patchtokens.  feats32: fp32 [n_images*grid*grid, dim] (may be NULL);
 * feats16: operand-dtype copy consumed by bd_decoder_forward (may be NULL). */
size_t bd_encoder_workspace_bytes(const bd_dino_weights* w /*[host]*/, int n_images, int prec);
int bd_encoder_forward(const bd_dino_weights* w /*[host]*/, const void* images, int img_dtype,
                       int n_images, int size, float* feats32, void* feats16, int64_t feats16_plane,
                       void* workspace, size_t workspace_bytes, int prec, void* stream);

/* BETR.forward (betr.py:249-308): bbox_feat [B, T, c, size, size] in [-1,1], feats16 from the encoder,
 * query_idx int32 [B] -> logits, heat fp32 [B, c, size, size]. */
size_t bd_decoder_workspace_bytes(const bd_betr_weights* w /*[host]*/, int B, int T, int prec);
int bd_decoder_forward(const bd_betr_weights* w /*[host]*/, const void* bbox_feat, int in_dtype,
                       const void* feats16, int64_t feats16_plane, const int32_t* query_idx, int B,
                       int T, int size, float* logits, float* heat, void* workspace,
                       size_t workspace_bytes, int prec, void* stream);

/* BETR.forward on a RAGGED batch: sample b has view_start[b + 1] - view_start[b] views (its references and its query), the batch's
 * n_views views are packed back to back.  The reference cannot express this (its dataset emits one `length` per batch, and its
 * sub_batchify pads with zero views that the joint attention then attends to, src/models/utils/data_utils.py:40-80); a caller that
 * batches queries of different objects can.  bbox_feat: [n_views, c, size, size]; feats16: the encoder's operand copy of the same
 * n_views images (bd_encoder_forward on the packed images: the encoder needs no ragged form); view_start: device int32 [B + 1];
 * query_view: device int32 [B], the query's index inside its sample; n_views / max_views: the host's total and largest per-sample count
 * (B <= n_views, max_views <= n_views - (B - 1), max_views * B >= n_views) -> logits, heat fp32 [B, c, size, size].
 * The same chain of launches as bd_decoder_forward on M = n_views * P token rows -- the Linears, LayerNorm fold, 3-byte residual stream,
 * per-Linear promotion and QK16 split are row-wise and unchanged; attention (bd_attention_varlen, one launch per block), the query-token
 * substitution and the query-row gather take the sample boundaries from view_start.  No launch is sized by B * max_views.  A sample's
 * outputs are bit-identical to bd_decoder_forward on that sample alone (B = 1, T = its views).  bd_betr_weights.latency_mode is ignored
 * (no latency forms for ragged calls).  Needs grid * grid % 128 == 0 and head_dim 96 (BD_ERR_SHAPE otherwise).
 * bd_decoder_workspace_bytes_ragged(w, B * T, B, prec) == bd_decoder_workspace_bytes(w, B, T, prec).
 * Sub-batch lanes: there is no _lanes form of the ragged call yet -- it runs as ONE lane on `stream` (a split at sample boundaries,
 * balanced on cumulative views, through the machinery below is the planned form). */
size_t bd_decoder_workspace_bytes_ragged(const bd_betr_weights* w /*[host]*/, int n_views, int B, int prec);
int bd_decoder_forward_ragged(const bd_betr_weights* w /*[host]*/, const void* bbox_feat, int in_dtype, const void* feats16,
                              int64_t feats16_plane, const int32_t* view_start, const int32_t* query_view, int B, int n_views,
                              int max_views, int size, float* logits, float* heat, void* workspace, size_t workspace_bytes,
                              int prec, void* stream);

/* Sub-batch lanes (ABI v6).  The same two operators with ONE batch run as `lanes` (1..4) contiguous sub-batches on `lanes`
 * streams: lane 0 on `stream`, the others on side streams the library owns (per device), forked from and joined back into
 * `stream` by events inside the call, so the call is stream-ordered for the caller exactly like the plain form (and capturable
 * into a HIP graph: the event wait pulls the side streams into the caller's capture).  Samples are independent on this path
 * (BETR attends within a sample, betr.py:282-296; the reference's per-sample loop is prediction_utils.py:63-101) and a row's
 * result does not depend on the launch geometry, so the outputs are BIT-identical to the plain form; what changes is that the
 * kernels of one lane fill the CUs the other lane's ragged last round leaves idle.  `lanes` <= 1 (or more lanes than samples)
 * IS the plain form.  The workspace is the sum of the lanes' workspaces (*_workspace_bytes_lanes).  bd_lanes_prepare creates
 * the current device's side streams / events ahead of a stream capture (they are otherwise created on first use).
 * CONCURRENCY.  The side streams and the fork / join events belong to the calling HOST THREAD (per device; round 6 -- they were
 * process-global before): laned calls from several host threads on one device are independent, and a thread that is CAPTURING `stream`
 * into a HIP graph pulls only its own side streams into the capture, whatever other threads enqueue meanwhile.  Call bd_lanes_prepare
 * on the thread that will capture, before the capture opens (stream creation is not capturable).  The objects are never destroyed: a
 * host thread that exits leaves its three side streams and four events behind. */
int bd_lanes_prepare(void);
size_t bd_encoder_workspace_bytes_lanes(const bd_dino_weights* w /*[host]*/, int n_images, int prec, int lanes);
int bd_encoder_forward_lanes(const bd_dino_weights* w /*[host]*/, const void* images, int img_dtype,
                             int n_images, int size, float* feats32, void* feats16, int64_t feats16_plane,
                             void* workspace, size_t workspace_bytes, int prec, int lanes, void* stream);
size_t bd_decoder_workspace_bytes_lanes(const bd_betr_weights* w /*[host]*/, int B, int T, int prec, int lanes);
int bd_decoder_forward_lanes(const bd_betr_weights* w /*[host]*/, const void* bbox_feat, int in_dtype,
                             const void* feats16, int64_t feats16_plane, const int32_t* query_idx, int B,
                             int T, int size, float* logits, float* heat, void* workspace,
                             size_t workspace_bytes, int prec, int lanes, void* stream);

/* Decoder-entry tokens kept in a bank (cache.RefFeatureBank with decoder=): a reference's entry row
 *     x[v] = bbox_emb(patchify(bbox_feat[v])) + pos + LN(adapter_fc2(gelu(adapter_fc1(feat[v]))))        (betr.py:313-329, :367-399)
 * is row-wise and independent of the query, so it is computed ONCE, when the reference enters the bank, and a forward neither reads
 * bbox_feat nor re-embeds it.
 *
 * bd_decoder_entry_tokens: the entry rows of n_views free-standing views -> x_out, caller-owned fp32 [n_views * P, dim].  bbox_feat:
 * [n_views, c, size, size] (in_dtype BD_DTYPE_*); feats16: the encoder's operand copy of the same views, in the class of adapter fc1
 * (bd_betr_weights.promote_misc).  Exactly the five launches with which bd_decoder_forward builds its token stream (adapter fc1,
 * adapter fc2, the no-affine LayerNorm, bd_patchify_heatmaps, the bbox_emb GEMM with its pos-table / residual epilogue) on
 * M = n_views * P rows, in the same operand classes: a row's bits equal the row bd_decoder_forward's stream holds for that view before
 * the query substitution.  No query row is touched.  workspace: bd_decoder_entry_tokens_workspace_bytes(w, n_views, prec) bytes. */
size_t bd_decoder_entry_tokens_workspace_bytes(const bd_betr_weights* w /*[host]*/, int n_views, int prec);
int bd_decoder_entry_tokens(const bd_betr_weights* w /*[host]*/, const void* bbox_feat, int in_dtype, const void* feats16,
                            int64_t feats16_plane, int n_views, int size, float* x_out, void* workspace, size_t workspace_bytes,
                            int prec, void* stream);

/* bd_decoder_forward_entry: BETR.forward (betr.py:249-308) on banked entry rows.  bank_x: fp32 [bank_views, P, dim], rows of
 * bd_decoder_entry_tokens; src: device int32 [B * T], bd_assemble_entry_tokens' source table of the batch -- per sample its
 * references by bank row and its query view as -(b + 1); feats16: the encoder's operand copy of the B QUERY views, in sample order;
 * query_idx: device int32 [B], the slot src marks as the sample's query.  The adapter (fc1, fc2, LayerNorm; betr.py:313-317) runs on
 * the B * P query rows only, ONE bd_assemble_entry_tokens launch writes the token stream, then the block stack and the head of
 * bd_decoder_forward run as planned there: no patchify launch, no bbox_emb GEMM, no bbox_feat.  Outputs are bit-identical to
 * bd_decoder_forward on the same views (latency_mode: within the mode's tolerance, as ever).  `lanes`: bd_decoder_forward_lanes'
 * sub-batch lanes (lane l reads src from its first sample's views on); <= 1 is one lane on `stream`.
 * bd_decoder_forward_entry_ragged: the same on a ragged batch -- view_start / query_view / n_views / max_views and their constraints
 * are bd_decoder_forward_ragged's, src is int32 [n_views] -- as ONE lane. */
size_t bd_decoder_entry_workspace_bytes(const bd_betr_weights* w /*[host]*/, int B, int T, int prec, int lanes);
int bd_decoder_forward_entry(const bd_betr_weights* w /*[host]*/, const float* bank_x, int bank_views, const int32_t* src,
                             const void* feats16, int64_t feats16_plane, const int32_t* query_idx, int B, int T, int size,
                             float* logits, float* heat, void* workspace, size_t workspace_bytes, int prec, int lanes, void* stream);
size_t bd_decoder_entry_workspace_bytes_ragged(const bd_betr_weights* w /*[host]*/, int n_views, int B, int prec);
int bd_decoder_forward_entry_ragged(const bd_betr_weights* w /*[host]*/, const float* bank_x, int bank_views, const int32_t* src,
                                    const void* feats16, int64_t feats16_plane, const int32_t* view_start, const int32_t* query_view,
                                    int B, int n_views, int max_views, int size, float* logits, float* heat, void* workspace,
                                    size_t workspace_bytes, int prec, void* stream);

/* ------------------------------------------------------------------------------------------
 * Launch tracing (measurement aid for bench.py; off by default; the only library state).
 * Between bd_trace_begin and bd_trace_end every GEMM (kind 0: M,N,K) and attention (kind 1:
 * M = batch*heads, N = seq, K = head_dim) launch is bracketed by HIP events on its stream.
 * bd_trace_end synchronises those events, fills `out` [host] and returns the record count.
 * ---------------------------------------------------------------------------------------- */
typedef struct bd_trace_record { int kind, M, N, K; float ms; } bd_trace_record;
int bd_trace_begin(int capacity);
int bd_trace_end(bd_trace_record* out /*[host]*/, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* BOXDREAMER_HIP_H */
