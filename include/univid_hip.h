/* univid_hip.h - C ABI of libunivid_hip.so (MI355X / gfx950 only).
 *
 * This is the drop-in boundary for UniVid's diffusion-decoder hot path. The reference has no native code
 * and no FFI: its seam is a set of PyTorch op sequences inside
 * models/wan/utils/modules/{model,attention,vae2_2}.py and models/wan/utils/fm_solvers_unipc.py. Each entry
 * point below replaces one such sequence (cited per function, paths relative to the reference root) and is what
 * a ctypes / pybind11 / cffi stub on the reference side would bind (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated; no torch types.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream). Calls are asynchronous on it and never
 *     synchronise, allocate or free (uv_init() does the one-time allocations), so they can be graph-captured.
 *   - bf16 tensors are raw uint16 bit patterns; leading dimensions (ld*) are in ELEMENTS.
 *   - return 0 on success; non-zero on a rejected argument or failed launch, with uv_last_error() describing it.
 *     Nothing is written on a rejected call. There is no CPU fallback anywhere in this library.
 */
#ifndef UNIVID_HIP_H
#define UNIVID_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- library ---------------------------------------------------------------------------------------------- */
int uv_version(void);                      /* 200 = 0.2.0 */
const char* uv_build_id(void);             /* digest of the kernel sources the library was built from (loader checks it) */
int uv_init(void);                         /* one-time allocations for the CURRENT device; call once per device before use */
const char* uv_last_error(void);           /* thread-local text of the last failure */
int uv_device_arch(char* buf, int len);    /* e.g. "gfx950:sramecc+:xnack-" */
/* Host scheduling policy of the CURRENT device: on = hipDeviceScheduleBlockingSync (a waiting host thread sleeps instead of spinning),
 * 0 = the runtime's default. Never set implicitly (process-wide policy); one-rank-per-GPU launchers call it once per device. */
int uv_host_blocking_sync(int on);

/* Developer options: process-wide switches for A/B tools and tests, set EXPLICITLY through these calls - the library never reads the
 * environment. Defaults are what production runs; none of them changes results beyond the f32 summation order noted per key.
 *   UV_OPT_CONV_HALO  -1 automatic (default) | 0 never | 1 whenever the geometry fits: which 3x3 stride-1 convolutions of uv_conv3d_* take
 *                     the LDS-halo kernel instead of the gather kernel (the two sum their k-tiles in different orders: ~1e-5 apart)
 *   UV_OPT_GEMM_GM    0 automatic (default) | 1..64: tile-walk group height of the persistent GEMM (tile order only, results unchanged)
 *   UV_OPT_ATTN_CUT   0 automatic (default) | v: flash_attn_fwd12_kernel cuts every head with v - 1 eight-unit blocks (results unchanged)
 *   UV_OPT_ATTN_WIN_FORM   0 automatic (default: the span rule of uv_flash_attn_win_plan) | 1 the 12-wave | 2 the 4-wave form of uv_flash_attn_win_bf16 (results unchanged)
 * uv_set_option rejects unknown keys / out-of-range values; uv_reset_options restores every default. Host-only, thread-safe. */
#define UV_OPT_CONV_HALO 0
#define UV_OPT_GEMM_GM 1
#define UV_OPT_ATTN_CUT 2
#define UV_OPT_ATTN_WIN_FORM 3
int uv_set_option(int key, int value);
int uv_get_option(int key, int* value);
int uv_reset_options(void);

/* ---- DiT: GEMMs -------------------------------------------------------------------------------------------- */
/* epilogue selectors of uv_gemm_bf16_nt */
#define UV_EPI_BF16 0            /* out_bf16 = bf16(acc + bias)                               nn.Linear under autocast */
#define UV_EPI_GELU_BF16 1       /* out_bf16 = bf16(gelu_tanh(bf16(acc + bias)))              ffn.0 + GELU, model.py:212-213 */
#define UV_EPI_F32_FROM_BF16 2   /* out_f32  = float(bf16(acc + bias))                        patch_embedding, model.py:448 */
#define UV_EPI_RESID_F32 3       /* x_f32   += float(bf16(acc + bias))                        x + cross_attn(...), model.py:251 */
#define UV_EPI_GATE_RESID_F32 4  /* x_f32    = x + float(bf16(acc + bias)) * gate[tid[m]][n]  x + y*e, model.py:247,255 */
#define UV_EPI_BF16_T 5          /* outT_bf16[n][m] = bf16(acc + bias)                        V^T for uv_flash_attn_bf16 */
/* (6 = UV_EPI_BF16 + per-group sums of squares: reached through uv_gemm_bf16_nt_ssq, which carries the extra output) */

/* C[M,N] = A[M,K] . W[N,K]^T + bias, bf16 operands, fp32 accumulate (MFMA 16x16x32).
 * Replaces nn.Linear q/k/v/o, ffn.0/ffn.2, text_embedding, patch_embedding (model.py:119-122, 212-214, 378-382).
 * K % 64 == 0, N % 16 == 0; M arbitrary. bias: bf16 [N] or NULL. gate/gate_tid only for UV_EPI_GATE_RESID_F32
 * (gate: f32 [n_t, gate_stride]; gate_tid: int32 [M] or NULL = row 0). tile_cfg 0 = auto. */
int uv_gemm_bf16_nt(const void* A, long lda, const void* W, long ldw, const void* bias_bf16, int M, int N, int K,
                    int epilogue, void* out, long ldo, const float* gate, const int32_t* gate_tid, long gate_stride,
                    int tile_cfg, void* stream);

/* uv_gemm_bf16_nt with a caller-owned workspace: the rows a large projection leaves after whole rounds of 256x256 tiles (1 120 of
 * the 22 880 rows of the CFG pair at 49 x 704 x 1280) run, for K >= 8192 (ffn.2, model.py:214,255), as ONE round of 256x256 tiles x
 * split-K 4 instead of 128x128 tiles: four f32 partial tiles per output tile, published through the workspace and summed IN SLICE ORDER
 * by the last-arriving workgroup, which then applies the ordinary epilogue. Deterministic (same bits run to run); the strip's rows differ
 * from uv_gemm_bf16_nt's by the f32 summation order only (4 partial sums instead of one chain; <= 1 ulp of the epilogue's 16-bit rounding).
 * workspace: device memory, 256-byte aligned, workspace_bytes >= uv_gemm_splitk_ws_bytes(M, N, K); contents need no initialisation and
 * are scratch afterwards; launches that share a workspace must be ordered (same stream). NULL / too small: exactly uv_gemm_bf16_nt.
 * tile_cfg 19 / 20 (tests, tools): the whole problem as split-K 4 / 2 (epilogues 0, 3, 4; workspace 4096 + tiles x split x 256 KiB). */
int uv_gemm_bf16_nt_ws(const void* A, long lda, const void* W, long ldw, const void* bias_bf16, int M, int N, int K,
                       int epilogue, void* out, long ldo, const float* gate, const int32_t* gate_tid, long gate_stride,
                       int tile_cfg, void* workspace, long workspace_bytes, void* stream);
long uv_gemm_splitk_ws_bytes(int M, int N, int K);   /* 0: tile_cfg 0 has no split-K strip for this shape */
/* The launch plan of a uv_gemm_bf16_nt / _ws / _ssq call (f16 != 0: uv_gemm_f16_nt) of this shape on the current device (256 CUs without
 * one), before anything is launched: *steps = 1 or 2, and for step i the kernel's name at kernels + i * len (PERSIST, PINGPONG, RING128,
 * T128, T256, T256x192, SPLITK4, SPLITK2, or DIAG<tile_cfg> for the configurations only tests and tools select) and the rows
 * m0[i] .. m0[i] + rows[i] - 1 it computes. ws_bytes: the workspace the call would pass (0: none; a non-zero size counts as aligned).
 * The same shape checks as the call itself. Host only. */
int uv_gemm_plan(int M, int N, int K, int epilogue, long ldo, int tile_cfg, int f16, long ws_bytes, int* steps, char* kernels, int len,
                 int* m0, int* rows);

/* uv_gemm_bf16_nt with IEEE fp16 operands, bias and 16-bit outputs (fp32 accumulate): the dtype the reference runs the SigLIP2
 * ranker in (models/BAGEL/eval_understanding.py:172,181,191: fp16 autocast). Same epilogues; tile_cfg must be 0. */
int uv_gemm_f16_nt(const void* A, long lda, const void* W, long ldw, const void* bias_f16, int M, int N, int K, int epilogue,
                   void* out, long ldo, const float* gate, const int32_t* gate_tid, long gate_stride, int tile_cfg, void* stream);

/* The q projection whose RMSNorm the attention kernel applies itself (WanSelfAttention / WanCrossAttention: q = norm_q(self.q(x)),
 * model.py:138, 169; WanRMSNorm over ALL heads' columns, :82-85): out = bf16(A W^T + bias) exactly as UV_EPI_BF16, and in the same pass
 * ssq[m][g] = sum over the 32 columns n in [32 g, 32 g + 32) of float(out[m][n])^2, f32 [M, ld_ssq], N % 32 == 0, ld_ssq >= N / 32.
 * Every group is summed in ONE fixed order whatever kernel and tile shape computes it (quads of 4 consecutive columns left to right, then
 * (s_k + s_{k+4}) pairs, then a balanced tree), so the values do not depend on the schedule. uv_rms_scale_from_ssq turns them into the
 * per-row scale uv_flash_attn_bf16_qnorm consumes: one pass over q (read + write of [M, N] bf16) is gone. */
int uv_gemm_bf16_nt_ssq(const void* A, long lda, const void* W, long ldw, const void* bias_bf16, int M, int N, int K, void* out, long ldo,
                        float* ssq, long ld_ssq, int tile_cfg, void* stream);
/* rs[m] = 1 / sqrt(sum_g ssq[m][g] / C + eps), groups added in a fixed order (four ascending quarter sums, then (p0 + p1) + (p2 + p3)):
 * WanRMSNorm's x.pow(2).mean(-1) + eps, rsqrt (model.py:85). */
int uv_rms_scale_from_ssq(const float* ssq, long ld_ssq, int M, int groups, int C, float eps, float* rs, void* stream);

/* Down-projection of an UN-MERGED LoRA adapter (peft==0.17.1 peft/tuners/lora/layer.py `Linear.forward`:
 * `result = result + lora_B(lora_A(dropout(x))) * scaling`, as the reference runs it after LoRAManager.load_lora_weights ->
 * PeftModel.from_pretrained, models/model_pipeline.py:724-750): out[m][j] = bf16(scale[j] * sum_k x[m][k] A[j][k]) for j < R and
 * exactly 0 for R <= j < Rpad. x bf16 [M, ldx], A bf16 [R, lda] (the lora_A weights of every adapter / projection reading x, stacked
 * row-wise), scale f32 [R] (lora_alpha / r, rslora, per-module patterns, run-time strength: applied before the ONE rounding to bf16,
 * which is lora_A(x)'s), fp32 accumulate. K % 64 == 0, 1 <= R <= Rpad, Rpad % 128 == 0, leading dimensions multiples of 8, pointers
 * 16-byte aligned. out may be x + K (same rows, disjoint columns): the projection then runs as uv_gemm_bf16_nt over
 * [x | out] . [W | B | 0]^T with K + Rpad columns, so the adapter lands in the fp32 accumulator in front of the fused epilogue.
 * Nothing outside [0, M) x [0, Rpad) of out is written, nothing beyond column K or row M of x is read. Every output element is one
 * fixed-order chain over k (no split-K, no atomics): a row's bits do not depend on the other rows of the launch. */
int uv_lora_down_bf16(const void* x, long ldx, const void* A, long lda, const float* scale, int M, int K, int R, void* out, long ldo,
                      int Rpad, void* stream);
/* The same down-projection with one scale ROW PER SEGMENT of seg_rows consecutive rows of x (per-sample adapter weights inside one
 * stacked forward: a segment is a stacked sample): row m belongs to segment s = m / seg_rows, scale f32 [nseg, ld_scale], and
 * out[m][j] = +0 if scale[s][j] == 0 (whatever the accumulator holds - an adapter that is off for a sample contributes exact +0, never
 * -0 or NaN), else bf16(scale[s][j] * sum_k x[m][k] A[j][k]) in uv_lora_down_bf16's accumulation order: with one segment, or segment by
 * segment, the bits are that entry point's. Columns [R, Rpad) are +0. A segment boundary may fall anywhere (the scale is looked up per
 * output row); the last segment may be partial. A 32-row workgroup skips a 128-rank pass - no read of x, no MFMA, zero stores only -
 * when the pass's scale entries are zero for every segment its rows touch. Every check of uv_lora_down_bf16 applies; seg_rows >= 1,
 * nseg >= 1, nseg * seg_rows >= M, ld_scale >= R, scale 4-byte aligned. */
int uv_lora_down_seg_bf16(const void* x, long ldx, const void* A, long lda, const float* scale, long ld_scale, int seg_rows, int nseg,
                          int M, int K, int R, void* out, long ldo, int Rpad, void* stream);

/* ---- DiT: MXFP8 GEMMs (opt-in fast mode of ffn.0 / ffn.2; WanModel.set_ffn_precision("mxfp8")) ---------------------------------
 * Format (OCP Microscaling, MXFP8): elements are e4m3fn (the OCP encoding: bias 7, largest finite 448, no infinity, NaN = 0x7F / 0xFF;
 * not the fnuz encoding), in blocks of 32 CONSECUTIVE K ELEMENTS OF ONE ROW, with one e8m0 scale byte (2^(e - 127)) per block:
 *   amax    = largest magnitude of the block
 *   e       = clamp(biased_fp32_exponent(amax) - 8, 0, 254), i.e. the scale 2^(floor(log2 amax) - 8); an all-zero block: e = 0, codes 0
 *   element = round-to-nearest-even of x / 2^(e - 127) to e4m3 AFTER clamping to +-448 (the scaled amax lies in [256, 512), above
 *             e4m3's 448: the clamp is explicit, the conversion's own overflow behaviour is never relied on; no code is ever a NaN)
 * Layouts: codes uint8 [rows, ld] (ld in bytes, ld % 16 == 0); scales uint8 [rows, ld_s] row-major, ld_s >= K / 32, ld_s % 4 == 0;
 * K % 128 == 0 (one 16x16x128 instruction step). Code pointers 16-byte, scale pointers 4-byte aligned. */

/* bf16 x [M, ldx] -> codes [M, ldc] + scales [M, ld_s] as above, one pass (16-byte loads and stores). Quantises the activations in front
 * of uv_gemm_mxfp8_nt and, once at prepare time, the weights (from the bf16 operand copy uv_gemm_bf16_nt would read: the two modes differ
 * by the quantisation only). Replaces nothing in the reference (models/wan/utils/modules/model.py:212-214 run in bf16 there): it is
 * what the fast mode adds. With finite inputs the bytes of a row are a pure function of that row - not of M, the row offset or the
 * other rows; non-finite inputs are outside the contract and stay confined to their own row. Columns >= K of codes and >= K / 32 of
 * scales are not written. */
int uv_mx_quant_bf16(const void* x, long ldx, void* codes, long ldc, void* scales, long ld_s, int M, int K, void* stream);

/* C[M,N] = deq(A)[M,K] . deq(W)[N,K]^T + bias on v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulate: uv_gemm_bf16_nt for MXFP8 operands
 * (replaces the same lines for ffn.0 / ffn.2, model.py:212-214, 252-255, in the fast mode). A codes [M, lda] with A_scale [M, ld_as],
 * W codes [N, ldw] with W_scale [N, ld_ws]; bias bf16 [N] (8-byte aligned) or NULL. Epilogues UV_EPI_BF16, UV_EPI_GELU_BF16,
 * UV_EPI_F32_FROM_BF16, UV_EPI_RESID_F32, UV_EPI_GATE_RESID_F32 with exactly the semantics of uv_gemm_bf16_nt (same device code);
 * out / ldo / gate / gate_tid / gate_stride as there. M arbitrary, N % 256 == 0, K % 128 == 0; anything else is rejected and nothing is
 * written. Every output element is ONE fixed-order chain over K (one instruction per 128-element K step, K steps in order; no split-K,
 * no atomics): a row's bits do not depend on M, on the row offset, or on which tile shape of the launch plan computed it. */
int uv_gemm_mxfp8_nt(const void* A, long lda, const void* A_scale, long ld_as, const void* W, long ldw, const void* W_scale, long ld_ws,
                     const void* bias_bf16, int M, int N, int K, int epilogue, void* out, long ldo, const float* gate,
                     const int32_t* gate_tid, long gate_stride, void* stream);

/* ---- DiT: MXFP8 attention projections (opt-in fast mode; WanModel.set_proj_precision("mxfp8")) -----------------------------------
 * The self-attention q / k / v / o and the cross-attention q / o Linears (models/wan/utils/modules/model.py:119-122, 138-140, 154,
 * 170-179) on uv_gemm_mxfp8_nt, and the producer in front of them (model.py:239-251). NARROWER than the reference's bf16. */

/* uv_gemm_mxfp8_nt with the transposed 16-bit output (UV_EPI_BF16_T; the v projection writing V^T): outT bf16 [N, ldo], ldo >= M and
 * % 4 == 0, and outT[n][m] carries EXACTLY the bits uv_gemm_mxfp8_nt(UV_EPI_BF16) writes at [m][n] - that is the definition (the same
 * product and rounding; the 16-bit values are transposed inside quads of lanes and leave as 8-byte stores along m). Columns >= M of outT
 * are not written. The argument checks (nothing is written on rejection), the launch plan and the one fixed-order chain over K - a row's
 * bits do not depend on M, the row offset or the tile shape - are uv_gemm_mxfp8_nt's. */
int uv_gemm_mxfp8_nt_t(const void* A, long lda, const void* A_scale, long ld_as, const void* W, long ldw, const void* W_scale, long ld_ws,
                       const void* bias_bf16, int M, int N, int K, void* outT, long ldo, void* stream);

/* uv_gemm_mxfp8_nt(UV_EPI_BF16) plus the output's sums of squares (UV_EPI_BF16_SSQ; the cross-attention q projection in front of
 * uv_rms_scale_from_ssq / uv_flash_attn_bf16_qnorm, model.py:170-171): out carries UV_EPI_BF16's bits, ssq f32 [M, ld_ssq],
 * ld_ssq >= N / 32, ssq[m][g] = the sum of float(out[m][n])^2 over columns [32 g, 32 g + 32) in the ONE summation order stated at
 * uv_gemm_bf16_nt_ssq (same device code). Columns >= N / 32 of ssq are not written. Checks, plan and K chain: uv_gemm_mxfp8_nt's. */
int uv_gemm_mxfp8_nt_ssq(const void* A, long lda, const void* A_scale, long ld_as, const void* W, long ldw, const void* W_scale,
                         long ld_ws, const void* bias_bf16, int M, int N, int K, void* out, long ldo, float* ssq, long ld_ssq,
                         void* stream);

/* uv_layernorm_mod (modes 1 and 2, round_ln 0 / 1, tid present or NULL) with an MXFP8 store: codes uint8 [L, ldc] and e8m0 scales uint8
 * [L, ld_s] in the format stated above. DEFINITION: the bytes are, bit for bit, uv_mx_quant_bf16 applied to what
 * uv_layernorm_mod(out_bf16 = 1) writes for the same inputs - the value is rounded to bf16 first, then quantised by the rule above (an
 * all-zero block: e = 0, codes 0; the +-448 clamp is explicit; no code is ever a NaN). No bf16 copy is written: the activation does not
 * make a bf16 round trip through memory in front of the q / k / v, cross q and ffn.0 GEMMs (WanLayerNorm + modulation, model.py:239-251).
 * C % 256 == 0, C <= 8192, ldc >= C and % 16 == 0, ld_s >= C / 32 and % 4 == 0, x / codes 16-byte and scales 4-byte aligned. Columns >= C
 * of codes and >= C / 32 of scales are not written. A row's bytes are a pure function of that row and its parameters. */
int uv_layernorm_mod_mx(const float* x, long ldx, void* codes, long ldc, void* scales, long ld_s, int L, int C, float eps, int mode,
                        const float* tab, long tab_stride, int shift_off, int scale_off, const int32_t* tid, const float* w,
                        const float* b, int round_ln, void* stream);

/* C[M,N] = A[M,K] . W[N,K]^T + bias (+ resid), all fp32, exact-f32 MFMA (16x16x4).
 * Replaces Head.head (fp32 island, model.py:286-290) and the VAE's 1x1 convolutions (vae2_2.py:211,249-250,766-767).
 * K % 4 == 0, N % 4 == 0. */
int uv_gemm_f32_nt(const float* A, long lda, const float* W, long ldw, const float* bias, int M, int N, int K, float* out,
                   long ldo, const float* resid, long ldr, void* stream);

/* ---- DiT: attention ---------------------------------------------------------------------------------------- */
/* out[Lq, H*D] = softmax(q k^T * softmax_scale) v per head, non-causal, all Lk keys attended, for `batch` independent
 * samples. Replaces flash_attention() (attention.py:24-130) as called at model.py:145-150 and :175.
 * q [batch*Lq, ldq], k [batch*Lk, ldk] bf16 (samples stacked along the token axis) with head h at columns
 * [h*D, (h+1)*D); vt = V TRANSPOSED, bf16 [H*D, ldvt]: sample b's keys are columns [b*Lk, (b+1)*Lk) (so one
 * UV_EPI_BF16_T GEMM over the stacked rows produces it), ldvt >= (batch-1)*Lk + roundup(Lk, 64), every column up to
 * that bound finite, Lk % 8 == 0 when batch > 1; out [batch*Lq, ldo]; head_dim D in {64, 128}. */
int uv_flash_attn_bf16(const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, void* out, long ldo,
                       int batch, int Lq, int Lk, int H, int head_dim, float softmax_scale, void* stream);

/* uv_flash_attn_bf16 on the RAW q projection: the Q prologue of every kernel applies norm_q - q'[m][c] = bf16( bf16(q[m][c] * q_rs[m]) * q_weight[c] ),
 * the roundings of uv_rmsnorm_rope - before the first MFMA. q_rs f32 [batch * Lq] (uv_rms_scale_from_ssq), q_weight f32 [H * D] (norm_q.weight).
 * No rotary embedding: the cross-attention form (model.py:160-180). k / vt as for uv_flash_attn_bf16 (k already normalised). */
int uv_flash_attn_bf16_qnorm(const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, void* out, long ldo,
                             int batch, int Lq, int Lk, int H, int head_dim, float softmax_scale, const float* q_rs, const float* q_weight,
                             void* stream);

/* uv_flash_attn_bf16 with IEEE fp16 q / k / vt / out (SigLIP2 ranker: transformers' attention under fp16 autocast). */
int uv_flash_attn_f16(const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, void* out, long ldo,
                      int batch, int Lq, int Lk, int H, int head_dim, float softmax_scale, void* stream);

/* Name of the kernel uv_flash_attn_bf16 (f16 = 0) / uv_flash_attn_f16 (f16 = 1) dispatches for a problem of this geometry
 * (selection depends on Lk, head_dim and the leading dimensions only); for benchmark / profile labels. Host-only. */
int uv_flash_attn_kernel_name(int Lk, int head_dim, long ldk, long ldvt, int f16, char* buf, int len);

/* The whole launch plan of uv_flash_attn_bf16 (f16 = 0) / uv_flash_attn_f16 (f16 = 1) for a problem, on the current device (256 compute
 * units without one) and under the current UV_OPT_ATTN_CUT: the kernel's name as above, *q_blocks query blocks per (sample, head), of
 * which the first *n12 own 12 units of 32 queries and the others 8 (flash_attn_fwd12_kernel; 0 for the other kernels, whose blocks own
 * 128 queries), and *grid = q_blocks * H * batch workgroups. Host-only; for tests and tuning tools. */
int uv_flash_attn_plan(int batch, int Lq, int Lk, int H, int head_dim, long ldk, long ldvt, int f16, char* kernel, int len,
                       int* q_blocks, int* n12, int* grid);

/* ---- DiT: sliding-window / causal self-attention (opt-in; WanModel.set_attn_window) -----------------------------------------------
 * uv_flash_attn_bf16 for Lq == Lk == L with flash_attn_varlen_func's window_size = (win_left, win_right) (attention.py:113-127 as called at
 * model.py:145-150; WanModel's window_size, a key of every checkpoint's config.json): query i of a sample attends key j iff
 * max(0, i - win_left) <= j <= min(L - 1, i + win_right), -1 = unbounded on that side; causal is win_right = 0. Every sample of the batch
 * restarts at i = 0. Exact - the same softmax over fewer keys: key tiles outside a workgroup's window are neither staged nor visited, and
 * (-1, -1), which visits every tile, or any window that covers every key reproduces uv_flash_attn_bf16 bit for bit. A query's bits do
 * not depend on the kernel form, the query-block cut, the batch or its neighbours. q / k / vt / out / ld* / batch / H / softmax_scale:
 * uv_flash_attn_bf16's meaning and checks (the ldvt cover and its finite pad, L % 8 == 0 when batch > 1), and 64 ldk, 128 ldvt < 2^30
 * elements. head_dim 128 only; win_left, win_right >= -1. Anything else is rejected and nothing is written. Bottom-right alignment for
 * Lq != Lk and ragged key lengths are not built. */
int uv_flash_attn_win_bf16(const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, void* out, long ldo, int batch, int L,
                           int H, int head_dim, float softmax_scale, int win_left, int win_right, void* stream);

/* The launch plan of uv_flash_attn_win_bf16, as uv_flash_attn_plan reports uv_flash_attn_bf16's: flash_attn_win12_kernel when the keys one
 * workgroup streams, min(L, 384 + win_left + win_right) with an unbounded side counted as L, are at least 2048 (the cut and grid of
 * uv_flash_attn_plan for the same batch, L, H), else flash_attn_win4_kernel (blocks of 128 queries, *n12 = 0). Host-only. */
int uv_flash_attn_win_plan(int batch, int L, int H, int head_dim, int win_left, int win_right, char* kernel, int len, int* q_blocks, int* n12,
                           int* grid);

/* ---- DiT: block-sparse self-attention from a key-tile mask (opt-in; WanModel.set_attn_block_mask) -----------------------------------
 * uv_flash_attn_bf16 for Lq == Lk == L under a block mask of 128-query x 64-key tiles (no counterpart in the reference, whose attention.py
 * knows global, causal and sliding-window attention): with nqb = ceil(L / 128), nkb = ceil(L / 64), query i of head h attends key j iff
 * mask[h][i / 128][j / 64] and j < L. The mask arrives as a schedule prepared once per mask: tile_idx int32 [mask_heads, nqb, nkb] holds
 * each (mask head, query block)'s visible key tiles in ascending order (the entries behind the count are never used), tile_cnt int32
 * [mask_heads, nqb] how many; mask_heads = 1 (one mask for all heads) or H; both on the device, shared by the samples of a stacked launch.
 * Every count should be >= 1 (univid_amd._lib.prepare_block_mask refuses a mask with an empty row); a block whose count is <= 0 gets zero
 * rows. The kernel clamps what it reads - the count into [0, nkb], an entry into [0, nkb - 1], an entry that is not its list's last into
 * the full tiles - so no list content reads outside k / vt; an unsorted or repeating list is computed as listed. Exact - the same softmax
 * over fewer keys: unlisted tiles are neither staged nor visited, the all-ones mask reproduces uv_flash_attn_bf16 bit for bit, and a
 * query's bits depend on its 32-query unit and on its block's list only. q / k / vt / out / ld* / batch / H / softmax_scale:
 * uv_flash_attn_win_bf16's meaning and checks. head_dim 128 only. Anything else is rejected and nothing is written. */
int uv_flash_attn_bs_bf16(const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, void* out, long ldo, int batch, int L,
                          int H, int head_dim, float softmax_scale, const int* tile_idx, const int* tile_cnt, int mask_heads, void* stream);

/* The launch plan of uv_flash_attn_bs_bf16: flash_attn_bs4_kernel on blocks of 128 queries, *q_blocks = ceil(L / 128), *grid = *q_blocks * H *
 * batch - whatever the mask holds. Host-only. */
int uv_flash_attn_bs_plan(int batch, int L, int H, int head_dim, char* kernel, int len, int* q_blocks, int* grid);

/* ---- DiT: data-dependent block-sparse self-attention - top-k key tiles chosen on the device (opt-in; TopKBlockMask) -------------------
 * No counterpart in the reference. uv_flash_attn_bs_bf16's domain (Lq == Lk == L, head_dim 128, bf16, nqb = ceil(L / 128), nkb =
 * ceil(L / 64)) with lists that a kernel builds per forward, sample, head and query block from pooled q.k scores. Three launches on one
 * stream: uv_attn_pool_qk, uv_attn_bs_select, uv_flash_attn_bs_lists_bf16. Deterministic: no atomics, fixed summation order.
 *
 * uv_attn_pool_qk: q, k bf16 [batch * L, >= H * 128] (row stride ldq / ldk elements, multiples of 8, head h at column 128 h; sample b = rows
 * [b L, (b + 1) L)) -> qbar fp32 [batch, H, nqb, 128] = the mean of the q rows of each 128-query block and kbar fp32 [batch, H, nkb, 128] =
 * the mean of the k rows of each 64-key tile: the fp32 sum of the block's VALID rows (a ragged last block / tile holds L % 128 / L % 64 of
 * them) divided by their count. Both contiguous. q and k are read once. Pointers 16-byte aligned; head_dim 128 only; batch > 1 needs
 * L % 8 == 0 (uv_flash_attn_bs_bf16's rule). Anything else is rejected and nothing is written. */
int uv_attn_pool_qk(const void* q, long ldq, const void* k, long ldk, void* qbar, void* kbar, int batch, int L, int H, int head_dim, void* stream);

/* uv_attn_bs_select: the lists of (sample b, head h, query block i) from qbar / kbar as uv_attn_pool_qk writes them. s[j] = sum_d
 * qbar[b][h][i][d] kbar[b][h][j][d] in fp32 (no softmax, no scale). keep: uint8 [keep_heads, nqb, nkb] (non-zero = the tile is always
 * listed), keep_heads = 1 (one keep mask for all heads) or H, shared by the samples; null = nothing is kept (keep_heads is still checked).
 * Among the tiles of the row that are NOT kept, the top_k best under the total order (score descending, tile index ascending) are listed as
 * well; fewer than top_k candidates: all of them. Scores are compared through an order-preserving unsigned image of their bits (-0 taken as
 * +0; NaNs sort at the two ends), so the choice is deterministic and, whatever the scores hold, the list is valid: tile_cnt[b][h][i] =
 * keepcount + min(top_k, nkb - keepcount) in [1, nkb], the first tile_cnt entries of tile_idx[b][h][i][:] strictly ascending in
 * [0, nkb - 1] (the ragged tile nkb - 1 can only be last). Entries behind the count are left as they were. tile_idx int32 [batch, H, nqb,
 * nkb], tile_cnt int32 [batch, H, nqb]: uv_flash_attn_bs_lists_bf16's format with mask_heads = H, mask_samples = batch. top_k >= 1; nkb <=
 * 4096 (the row is sorted in LDS); qbar / kbar 16-byte aligned. Anything else is rejected and nothing is written. */
int uv_attn_bs_select(const void* qbar, const void* kbar, const void* keep, int keep_heads, int top_k, int* tile_idx, int* tile_cnt, int batch,
                      int L, int H, void* stream);

/* uv_flash_attn_bs_bf16 under lists with a leading sample axis: tile_idx int32 [mask_samples, mask_heads, nqb, nkb], tile_cnt int32
 * [mask_samples, mask_heads, nqb]; mask_samples = 1 (the samples share the lists: uv_flash_attn_bs_bf16 exactly, bit for bit) or batch
 * (sample b walks its own lists). The same kernel, checks and guarantees; the lists may have been written by a kernel launched before on the
 * same stream (uv_attn_bs_select). */
int uv_flash_attn_bs_lists_bf16(const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, void* out, long ldo, int batch,
                                int L, int H, int head_dim, float softmax_scale, const int* tile_idx, const int* tile_cnt, int mask_heads,
                                int mask_samples, void* stream);

/* ---- DiT: self-attention with MXFP8 q / k (opt-in mode; WanModel.set_attn_precision("mxfp8_qk")) ------------------------------
 * uv_flash_attn_bf16 with q and k in the MXFP8 format stated above (e4m3fn codes, one e8m0 byte per 32 consecutive elements of a row, e =
 * clamp(exp(amax) - 8, 0, 254), clamp to +-448 then RNE, never a NaN code): replaces attention.py:24-130 as called at model.py:145-150 with
 * q and k NARROWER than the reference's bf16. The 32-element blocks run along the head dimension: each (row, head) has four scale bytes.
 * q_codes uint8 [batch*Lq, ldq] with head h at bytes [128 h, 128 h + 128), q_scales uint8 [batch*Lq, ld_qs] with head h at bytes
 * [4 h, 4 h + 4); k likewise over batch*Lk rows. ldq, ldk >= H*128 and % 16 == 0; ld_qs, ld_ks >= H*4 and % 4 == 0; code pointers 16-byte,
 * scale pointers 4-byte aligned (codes may be column slices of a wider buffer). vt, out, batch, Lq, Lk, H, softmax_scale: exactly
 * uv_flash_attn_bf16's meaning and checks (ldvt, the finite pad, Lk % 8 == 0 when batch > 1). head_dim 128 only; anything else is
 * rejected and nothing is written. S^T = K Q^T runs on v_mfma_scale_f32_32x32x64_f8f6f4 (the scales applied in hardware, products exact,
 * f32 accumulate); P.V and everything behind S is the bf16 kernels' arithmetic. Every S element is ONE chain: the instruction over
 * head-dim elements 0..63, then the one over 64..127, into the same accumulator - a query's bits do not depend on the kernel, the
 * query-block cut, the batch or its neighbours. Code and scale rows at Lk and beyond are never read (the ragged tile clamps both). */
int uv_flash_attn_mxqk(const void* q_codes, long ldq, const void* q_scales, long ld_qs, const void* k_codes, long ldk, const void* k_scales,
                       long ld_ks, const void* vt, long ldvt, void* out, long ldo, int batch, int Lq, int Lk, int H, int head_dim,
                       float softmax_scale, void* stream);

/* The launch plan of uv_flash_attn_mxqk, as uv_flash_attn_plan reports uv_flash_attn_bf16's: flash_attn_mxqk12_kernel (Lk >= 2048; *n12 of the
 * *q_blocks own 12 units of 32 queries, the others 8) or flash_attn_mxqk4_kernel (blocks of 128 queries, *n12 = 0). Host-only. */
int uv_flash_attn_mxqk_plan(int batch, int Lq, int Lk, int H, int head_dim, char* kernel, int len, int* q_blocks, int* n12, int* grid);

/* ---- DiT: self-attention with MXFP8 q / k AND an MXFP8 P.V (opt-in mode; WanModel.set_attn_precision("mxfp8_qk_pv")) ----------------
 * uv_flash_attn_mxqk with V and the softmax weights P narrow as well: O^T = V^T P^T runs on v_mfma_scale_f32_32x32x64_f8f6f4 with f32
 * accumulate (one instruction per 32 channels and 64-key tile in place of sixteen bf16 ones). q and k are exactly uv_flash_attn_mxqk's
 * operands (same producer uv_rmsnorm_rope_qk_mx, every S element the same single chain). head_dim 128 only.
 *
 * V^T format. Elements and scales follow the MXFP8 rule above (e = clamp(exp(amax) - 8, 0, 254), clamp to +-448 then RNE, never a NaN code);
 * a block is 32 CONSECUTIVE KEYS of one (head, head-dim channel) row, counted from EACH SAMPLE'S first key (not from column 0 of the stacked
 * buffer). Each sample's keys are zero-padded to Lkp = roundup(Lk, 64): pad codes are 0; a block that holds no key at all has the scale byte
 * 127 (a block with keys and pad follows the rule over its keys and zeros). No tile reads outside its sample; no pad can be a NaN.
 *   vt_codes  uint8 [H*128, ldvc], sample b at columns [b*Lkp, (b+1)*Lkp), ldvc >= batch*Lkp, ldvc % 16 == 0, 16-byte aligned.
 *             KEY ORDER INSIDE A 32-KEY BLOCK: key kappa (0..31) of the block is stored at byte perm34(kappa) = kappa with bits 3 and 4
 *             swapped, i.e. the four 8-key groups in the order 0, 2, 1, 3. (The contraction does not care and the scale is per block; in this
 *             order the instruction's A fragment is two plain 16-byte LDS reads against the lane map of the P accumulator.)
 *   vt_scales uint8 [H, ld_vs], TILE-MAJOR: the 64-key tile t of sample b of head h owns the 256 bytes at h*ld_vs + (b*Lkp/64 + t)*256; byte
 *             4*(r + 32*k) + d of them is the scale of channel 32*d + r (d = 0..3, r = 0..31) for the tile's key half k (keys 64 t + 32 k ..
 *             + 31 of the sample). ld_vs >= batch*Lkp*4, ld_vs % 4 == 0, 4-byte aligned. (One 4-byte LDS-DMA per lane stages a tile's scales,
 *             and lane l's dword holds the four bytes the instruction selects by op_sel.)
 * P format. code = e4m3_RNE(P * 2^PSHIFT) with the instruction's scale byte 127 - PSHIFT on every lane; P = exp2((s - m) * scale * log2 e) against
 * the query's running reference maximum m, which the query moves (once per 64-key tile, by its own scores alone) when a P would exceed
 * 2^DEFER. DEFER + PSHIFT = 8: the largest code is 256 < 448, the conversion's overflow behaviour is never relied on. With DEFER 1 / PSHIFT 7
 * normal codes reach down to P = 2^-13 and subnormal ones to 2^-16; smaller P are dropped from the numerator (a P of exactly 2^-17 ties to
 * even = 0). (DEFER 8 / PSHIFT 0 would flush every P below 2^-10: at 11 440 keys a diffuse tail of that size can carry as much mass as the
 * peak.) The denominator l sums the UNROUNDED f32 P, as the bf16 and mxqk kernels do. Masked keys (>= Lk) give code 0.
 * A query's bits do not depend on the kernel, the query-block cut, the batch or its neighbours.
 * Measured on one MI355X (profiles/mxpv_attn_bench.md, profiles/mxpv_parity_margins.json), against mxfp8_qk in the same process: attention launch + all
 * producers 0.934 x (L = 11 440) / 0.870 x (L = 27 280) of its time. The price: one TI2V-5B-width block is 3.83 x (48 tokens) / 1.28 x (2 304 tokens)
 * further from the unrounded result than the bf16 mode (mxfp8_qk: 2.87 x / 1.18 x); the kernel matches a CPU emulation of the format (truth ratio 1.0000 /
 * 1.0018). Not measured: the 30-block model and the 121-frame step in the mode. */
#define UV_ATT_MXPV_DEFER 1
#define UV_ATT_MXPV_PSHIFT 7

/* bf16 V^T [H*128, ldvt] as the UV_EPI_BF16_T GEMM writes it (sample b at columns [b*Lk, (b+1)*Lk); Lk % 8 == 0 when batch > 1; ldvt % 8 == 0,
 * ldvt >= (batch-1)*Lk + roundup(Lk, 8); columns at Lk and beyond of a sample are never used) -> vt_codes / vt_scales in the format above, pads
 * included, one pass. Replaces nothing in the reference (it is what the mode adds). For finite input the bytes of a (row, block) are a pure
 * function of that block's 32 values. head_dim 128 only. */
int uv_vt_mx_quant(const void* vt, long ldvt, void* vt_codes, long ldvc, void* vt_scales, long ld_vs, int batch, int Lk, int H, int head_dim,
                   void* stream);

/* uv_flash_attn_mxqk with vt_codes / vt_scales (above) in place of the bf16 V^T. q / k / out / batch / Lq / Lk / H / softmax_scale and their
 * checks: uv_flash_attn_mxqk's. Anything else is rejected and nothing is written. */
int uv_flash_attn_mxpv(const void* q_codes, long ldq, const void* q_scales, long ld_qs, const void* k_codes, long ldk, const void* k_scales,
                       long ld_ks, const void* vt_codes, long ldvc, const void* vt_scales, long ld_vs, void* out, long ldo, int batch, int Lq,
                       int Lk, int H, int head_dim, float softmax_scale, void* stream);

/* The launch plan of uv_flash_attn_mxpv: uv_flash_attn_mxqk_plan's geometry with flash_attn_mxpv12_kernel / flash_attn_mxpv4_kernel. Host-only. */
int uv_flash_attn_mxpv_plan(int batch, int Lq, int Lk, int H, int head_dim, char* kernel, int len, int* q_blocks, int* n12, int* grid);

/* Operator-seam helpers: what flash_attention(q, k, v, ...) (attention.py:24-130) does around the core when it is handed
 * [B, L, N, C] tensors of any float dtype: `half(x)` casts (:59-83), and `.type(out_dtype)` of the result (:130); the
 * transpose produces the V^T operand of uv_flash_attn_* from token-major V rows.
 * uv_transpose_16: out[c][l] = in[l][c] (16-bit elements, l < L, c < C); columns L .. Lpad-1 are written as zero. */
int uv_transpose_16(const void* in, long ldi, void* out, long ldo, int L, int C, int Lpad, void* stream);
/* contiguous f32 -> bf16 (f16 = 0) / IEEE fp16 (f16 = 1), round to nearest even; and the exact widening back */
int uv_cast_f32_to16(const float* in, void* out, long n, int f16, void* stream);
int uv_cast_16_to_f32(const void* in, float* out, long n, int f16, void* stream);

/* umT5 text-encoder attention (models/wan/utils/modules/t5.py:93-120), one prompt of n <= 1024 tokens, head_dim 64, bf16:
 * scores = bf16(bf16(q k^T) + rel_bias[h][key - query]) (no scaling), P = bf16(softmax_fp32(scores)), out = bf16(P v) - the
 * reference's rounding points. q, k, v, out [n, H*64]; rel_bias fp32 [H, 2*span - 1] (bf16 values of T5RelativeEmbedding for
 * relative positions -(span-1) .. span-1), span >= n. */
int uv_t5_attention_bf16(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, void* out, long ldo, int n, int H,
                         const float* rel_bias, int span, void* stream);

/* ---- DiT: fused HBM-bound glue ------------------------------------------------------------------------------ */
/* LayerNorm(no affine) over C then mode 0: y | 1: y*(1+scale[t])+shift[t] (t = tid[row]) | 2: y*w+b.
 * Replaces WanLayerNorm + AdaLN modulation (model.py:93-98, 239-245, 253, 287-290). round_ln=1 rounds y to bf16 first
 * (block 0, whose residual stream is still bf16). out is f32 (out_bf16=0), bf16 (1) or IEEE fp16 (2). C % 256 == 0, C <= 8192. */
int uv_layernorm_mod(const float* x, long ldx, void* out, long ldo, int L, int C, float eps, int mode, const float* tab,
                     long tab_stride, int shift_off, int scale_off, const int32_t* tid, const float* w, const float* b,
                     int round_ln, int out_bf16, void* stream);

/* out = bf16( RoPE( float(bf16(x * rsqrt(mean(x^2)+eps))) * weight ) ); RoPE (complex128 table `freqs`
 * [1024, head_dim/2] as (re,im) doubles) is skipped when freqs == NULL and for tokens >= F*Hh*Ww. Row i is token
 * row0 + i of the sequence (row0 > 0 for a sequence-parallel shard, distributed/sequence_parallel.py:47-56).
 * Replaces WanRMSNorm (model.py:82-85) + rope_apply (model.py:38-66) + the bf16 cast of attention.py:59-83. */
int uv_rmsnorm_rope(const void* x, long ldx, void* out, long ldo, const float* weight, int L, int C, int head_dim,
                    float eps, const double* freqs, int F, int Hh, int Ww, int row0, void* stream);
/* uv_rmsnorm_rope for q AND k of a self-attention in one launch (model.py:138-139, 146-147): same geometry, own norm weights;
 * the L rows hold L / Ls stacked samples whose RoPE positions restart every Ls rows. */
int uv_rmsnorm_rope_qk(const void* q, void* q_out, const float* q_weight, const void* k, void* k_out, const float* k_weight,
                       long ldx, long ldo, int L, int Ls, int C, int head_dim, float eps, const double* freqs, int F, int Hh,
                       int Ww, int row0, void* stream);

/* uv_rmsnorm_rope_qk with an MXFP8 output (the producer of uv_flash_attn_mxqk; same reference lines plus the quantisation the mode adds):
 * for q and for k, codes uint8 [L, ldc] (ldc >= C, % 16 == 0) and scales uint8 [L, ld_s] (ld_s >= C / 32, % 4 == 0). The bytes are, bit for
 * bit, uv_mx_quant_bf16 applied to what uv_rmsnorm_rope_qk writes for the same inputs (stacked samples and row0 included) - that equality
 * is the definition. head_dim 128 only, C % 128 == 0, C <= 4096. q and k are only read (no in-place form); columns >= C of the codes and
 * >= C / 32 of the scales are not written. */
int uv_rmsnorm_rope_qk_mx(const void* q, const float* q_weight, void* q_codes, void* q_scales, const void* k, const float* k_weight,
                          void* k_codes, void* k_scales, long ldx, long ldc, long ld_s, int L, int Ls, int C, int head_dim, float eps,
                          const double* freqs, int F, int Hh, int Ww, int row0, void* stream);

/* latent [Cin,F,H,W] f32 -> im2col rows [L, Kpad] bf16, column order (c,kt,kh,kw) = Conv3d.weight.flatten(1)
 * (model.py:378-379, 448-451). */
int uv_patchify_bf16(const float* x, void* out, long ldo, int Cin, int F, int H, int W, int pt, int ph, int pw, int Kpad,
                     void* stream);
/* head rows [L, pt*ph*pw*Cout] f32 -> [Cout, Fp*pt, Hp*ph, Wp*pw] f32 (WanModel.unpatchify, model.py:499-522). */
int uv_unpatchify_f32(const float* in, long ldi, float* out, int Cout, int Fp, int Hp, int Wp, int pt, int ph, int pw,
                      void* stream);
/* sinusoidal_embedding_1d (model.py:14-24): out[n, dim] f32 = cos||sin(t * 10000^(-i/half)) evaluated in fp64. */
int uv_sinusoid_f32(const float* t, float* out, int n, int dim, void* stream);
/* out[r][n] = act_in(x[r]) . W[n] + b[n], fp32, for the few distinct timestep rows (time_embedding / time_projection,
 * model.py:384-386, 465-468). act_in: 0 none, 1 SiLU. */
int uv_linear_rows_f32(const float* x, long ldx, const float* W, const float* b, float* out, long ldo, int R, int N, int K,
                       int act_in, void* stream);
/* out[r][i] = mod[i] + e0[r][i]  (modulation + e, model.py:239, 287) */
int uv_add_rows_f32(const float* mod, const float* e0, float* out, int R, long n, void* stream);
int uv_cast_f32_bf16(const float* in, void* out, long n, void* stream);
/* the same for [R, C] rows with leading dimensions (an output buffer that carries a LoRA slot behind its C columns); C % 4 == 0 */
int uv_cast_f32_bf16_rows(const float* in, long ldi, void* out, long ldo, int R, int C, void* stream);
/* x_f32 += float(y_bf16): un-fused residual used when WanCrossAttention.forward has been re-assigned (UniVid's hook). */
int uv_add_bf16_resid(float* x, long ldx, const void* y, long ldy, int L, int C, void* stream);
/* UniVid's dynamic text weight on the embedded context of ONE sample (Wan22ContextWrapper's per-layer hook,
 * models/model_pipeline.py:1779-1797: `context * weight_mask`, weight_mask = ones_like(context) with rows [0, text_len) `*= w`):
 * out[r] = bf16(in[r] * bf16(w)) for r < n_scaled, out[r] = in[r] for n_scaled <= r < R. in / out bf16 [R, C], C % 8 == 0; in == out allowed.
 * The result is what the K / V projections of the hooked layers read (WanModel.set_text_weight). */
int uv_text_weight_rows_bf16(const void* in, long ldi, void* out, long ldo, int R, int n_scaled, int C, float w, void* stream);

/* out[r] = x[r] / max(||x[r]||_2, eps): torch.nn.functional.normalize(dim=-1) of the SigLIP2 ranker's embeddings
 * (models/BAGEL/eval_understanding.py:185,195). */
int uv_l2_normalize_rows_f32(const float* x, long ldx, float* out, long ldo, int R, int C, float eps, void* stream);

/* ContextProjector glue (models/model_pipeline.py:1516-1523, 1532-1549; the module is bf16): exact (erf) GELU of a bf16 tensor,
 * and F.interpolate(mode='linear', align_corners=False) along the token axis of [Lin, C] bf16 rows. */
int uv_gelu_erf_bf16(const void* in, void* out, long n, void* stream);
int uv_interp_linear_rows_bf16(const void* in, long ldi, void* out, long ldo, int Lin, int Lout, int C, void* stream);

/* umT5 encoder glue (t5.py, bf16 module): bf16 residual add (:175-176); fc1 * GELU(gate) with the reference's op-by-op bf16 GELU
 * (:46-50, :138). */
int uv_add_bf16(const void* x, const void* y, void* out, long n, void* stream);
int uv_t5_gated_gelu_bf16(const void* gate, const void* fc1, void* out, long n, void* stream);

/* ---- sampler (CFG + flow UniPC order 2 / bh2 / predict-x0) -------------------------------------------------- */
/* noise_pred = uncond + gs*(cond - uncond) (textimage2video.py:385); x0 = sample - sigma*noise_pred
 * (fm_solvers_unipc.py:323). noise_pred may be NULL. */
int uv_cfg_convert(const float* cond, const float* uncond, const float* sample, float guide_scale, float sigma,
                   float* noise_pred, float* x0, long n, void* stream);
/* multistep_uni_c_bh_update (fm_solvers_unipc.py:545-628) with host-computed fp32 coefficients. */
int uv_unipc_corrector(const float* x_last, const float* m0, const float* m_prev, const float* model_t, float* out, float r,
                       float c1, float c2, float rho0, float rho_last, float rk, int order, long n, void* stream);
/* multistep_uni_p_bh_update (fm_solvers_unipc.py:397-486). */
int uv_unipc_predictor(const float* x, const float* m0, const float* m_prev, float* out, float r, float c1, float c2,
                       float rk, int order, long n, void* stream);
/* DPM-Solver++ update of sample_solver='dpm++' (textimage2video.py:343-351): dpm_solver_first_order_update (fm_solvers.py:417-485,
 * order 1) and multistep_dpm_solver_second_order_update, midpoint (fm_solvers.py:488-595, order 2; m1 = the older x0), with the
 * host-computed fp32 scalars r = sigma_t/sigma_s0, c = alpha_t*(exp(-h)-1), inv_r0 = 1/r0. */
int uv_dpmpp_update(const float* x, const float* m0, const float* m1, float* out, float r, float c, float inv_r0, int order,
                    long n, void* stream);

/* ---- step cache (WanTI2V.denoise(step_cache=): skipped steps forecast the block stack's residual) ------------- */
/* ctl: 4 floats in DEVICE memory, [have, k, c1, c2], read by the kernels on every launch (a captured graph serves every step; the host
 * writes the table before each replay). have = number of valid difference buffers before this launch (0 .. order + 1). order in
 * {0, 1, 2}: only d0 .. d[order] exist, the others are NULL and never touched. All tensors fp32, n contiguous elements, n > 0; 16-byte
 * loads / stores when every buffer is 16-byte aligned, element by element otherwise. Every operation below is one fp32 rounding.
 * update, after the blocks of a computed step (k = steps since the last computed one): r = x_out - x_in;
 *   order >= 1 and have >= 1: n1 = (r - d0) / k;  order >= 2 and have >= 2: n2 = (n1 - d1) / k;
 *   then d0 = r, d1 = n1, d2 = n2 where formed; a buffer that was not formed is not written. x_out and x_in are only read. */
int uv_step_cache_update(const float* x_out, const float* x_in, float* d0, float* d1, float* d2, const float* ctl, long n, int order,
                         void* stream);
/* apply, instead of the blocks of a skipped step (x holds x_in): rh = d0; have >= 2: rh = rh + d1 * c1; have >= 3: rh = rh + d2 * c2;
 *   x = x + rh in place. k is not read. */
int uv_step_cache_apply(float* x, const float* d0, const float* d1, const float* d2, const float* ctl, long n, int order, void* stream);
/* out[i] = (sum_j |rows[i+1][j] - rows[i][j]|) / (sum_j |rows[i][j]|), i < n_rows - 1: rows fp32 [n_rows, K] contiguous, n_rows >= 2.
 * Both sums in fp64 in a fixed order (one workgroup per pair, no atomics: the same bits on every launch), the fp64 quotient rounded to
 * fp32 once. A zero row gives inf or NaN. */
int uv_rows_rel_l1(const float* rows, float* out, int n_rows, int K, void* stream);

/* ---- VAE (fp32, channels-last [T, H, W, C]) -------------------------------------------------------------------- */
/* Causal 3D / 2D convolution as implicit GEMM on the exact-f32 MFMA. Replaces CausalConv3d (vae2_2.py:17-42) and the
 * Resample convolutions (vae2_2.py:86-108, 153-155). in: input ring [Tin, Hin, Win, ld_in]; w: [Cout, kt*kh*kw*Cin]
 * (tap-major, channel-minor); out rows = output pixels (t,h,w) row-major, [M, ldo]. Input frame of tap dt for output
 * frame t is t*st + dt + t_off; rows/cols are h*sh + dh - ph, w*sw + dw - pw, out-of-range taps contribute zero.
 * up=1: the input is read through a nearest-exact 2x spatial upsample (Hin/Win are the PRE-upsample sizes).
 * up=2+2a+b (a, b in {0,1}): ONE OUTPUT PHASE of such an upsampling 3x3 convolution. On the 2x nearest-upsampled image the three taps
 * of a row collapse onto two source rows (phase a=0: {dy=0} -> y-1, {1,2} -> y; a=1: {0,1} -> y, {2} -> y+1; columns alike), so output
 * pixels (2y+a, 2x+b) are a 2x2 convolution of the SOURCE image with the pre-summed weights of the collapsed taps: 16 instead of 36
 * multiply-adds per four output pixels. The launch takes that 2x2 kernel (kh = kw = 2, ph = 1-a, pw = 1-b), Hout/Wout = the SOURCE
 * resolution, and stores pixel (t, y, x) at (t, 2y+a, 2x+b) of the [Tout, 2 Hout, 2 Wout, ldo] output; four launches make the layer.
 * interleave=1: output channel halves become consecutive frames (Resample.time_conv, vae2_2.py:143-151).
 * Cin % 32 == 0 (zero-pad channels), Cout % 4 == 0. */
int uv_conv3d_f32(const float* in, long ld_in, int Tin, int Hin, int Win, const float* w, const float* bias, float* out,
                  long ldo, int Tout, int Hout, int Wout, int Cin, int Cout, int kt, int kh, int kw, int st, int sh, int sw,
                  int t_off, int ph, int pw, int up, int interleave, const float* resid, long ldr, void* stream);
/* The launch plan of a uv_conv3d_* call of this geometry on the current device (256 CUs without one) under the current UV_OPT_CONV_HALO:
 * the kernel's name (one of 23: 16 gather-kernel instantiations "G<rows>x<columns>+<prec>" / "G160+<prec>", 7 LDS-halo kernels "HALO_*"),
 * and its grid, tiles_m row tiles (halo kernels: pixel patches) x tiles_n output-channel tiles. prec: 0 uv_conv3d_f32, 1 / 2 uv_conv3d_bf16x3
 * without / with in_split, 3 uv_conv3d_bf16x6, 4 uv_conv3d_f16x3 (and uv_conv3d_f16, asked with HALF its Cin). Runs the geometry checks of the call itself. Host only. */
int uv_conv3d_plan(int prec, int Tout, int Hout, int Wout, int Hin, int Win, int Cin, int Cout, int kt, int kh, int kw, int st, int sh,
                   int sw, int ph, int pw, int up, int interleave, char* kernel, int len, int* tiles_m, int* tiles_n);
/* uv_conv3d_f32 with the products computed on the bf16 matrix pipe by exact three-way splitting of both f32 operands (x = x0 + x1 + x2,
 * round-to-nearest bf16 planes; the six terms with i + j <= 2; f32 accumulate): per-product error below 2^-26 (under f32 rounding).
 * Activations / bias / residual / output as in uv_conv3d_f32 (split in registers); w_split6 = uv_split_weights_bf16x6 of the f32
 * weights. Replaces the same reference lines as uv_conv3d_f32. */
int uv_conv3d_bf16x6(const float* in, long ld_in, int Tin, int Hin, int Win, const void* w_split6, const float* bias, float* out, long ldo,
                     int Tout, int Hout, int Wout, int Cin, int Cout, int kt, int kh, int kw, int st, int sh, int sw, int t_off, int ph,
                     int pw, int up, int interleave, const float* resid, long ldr, void* stream);
/* w [rows][K] f32 (K % 32 == 0) -> [rows][K/32][32 p0 | 32 p1 | 32 p2] bf16, w = p0 + p1 + p2 exactly (n = rows * K elements in,
 * 3 n bf16 out). */
int uv_split_weights_bf16x6(const float* w, void* out, long n, void* stream);
/* The same convolution in split-bf16 ("bf16x3") arithmetic: x*w ~ xh*wh + xh*wl + xl*wh on the bf16 MFMA with f32 accumulate
 * (relative error per product ~1e-5; up to 16/3 x the f32-MFMA rate). w_split comes from uv_split_weights_bf16x3.
 * in_split=1: the input ring already holds split activations ([C/32][32 hi | 32 lo] bf16 per pixel, as written by
 * uv_vae_rms_silu(split_out=1)); in_split=0: f32 activations, split in registers. */
int uv_conv3d_bf16x3(const float* in, long ld_in, int Tin, int Hin, int Win, const void* w_split, const float* bias, float* out,
                     long ldo, int Tout, int Hout, int Wout, int Cin, int Cout, int kt, int kh, int kw, int st, int sh, int sw,
                     int t_off, int ph, int pw, int up, int interleave, const float* resid, long ldr, int in_split, void* stream);
/* w [n] f32 (rows of K, K % 32 == 0) -> [n/32][32 hi | 32 lo] bf16 with hi = bf16(w), lo = bf16(w - hi) */
int uv_split_weights_bf16x3(const float* w, void* out, long n, void* stream);
/* The same convolution, f32-GRADE, in THREE fp16 MFMA passes ("f16x3"): both operands pre-split into two IEEE fp16 pieces (hi = fp16(x),
 * lo = fp16(x - hi): x to 2^-22 relative), x*w ~ xh*wh + xh*wl + xl*wh on v_mfma_f32_16x16x32_f16, f32 accumulate. Against an fp64
 * convolution it is as close as uv_conv3d_f32: at K = 27 C both are dominated by the f32 accumulation error (tests: test_conv3d_f16x3_is_f32_grade).
 * `in` holds PRE-SPLIT activations ([C/32][32 hi | 32 lo] fp16 per pixel = the bytes of an f32 pixel; written by uv_vae_rms_silu(split_out=2);
 * |x| < 65 504: an RMS-normalised row is bounded by sqrt(C) max|gamma|, which the caller checks); w_split = uv_split_weights_f16x3(w, w_scale)
 * with w_scale a power of two (max|w| * w_scale in [2^13, 2^14) keeps the lo pieces normal); out = acc / w_scale + bias (+ resid), f32.
 * act_scale: NULL, or a DEVICE scalar the result is multiplied by too - the 1 / s of activations split by uv_vae_split_f16 under a
 * per-tensor power-of-two scale (convolutions whose input is not an RMS_norm output: Resample, vae2_2.py:86-108).
 * Replaces the same reference lines as uv_conv3d_f32 for the convolutions that follow an RMS_norm (ResidualBlock, heads: vae2_2.py:193-235). */
int uv_conv3d_f16x3(const float* in, long ld_in, int Tin, int Hin, int Win, const void* w_split, const float* bias, float* out, long ldo,
                    int Tout, int Hout, int Wout, int Cin, int Cout, int kt, int kh, int kw, int st, int sh, int sw, int t_off, int ph,
                    int pw, int up, int interleave, const float* resid, long ldr, float w_scale, const float* act_scale, void* stream);
/* The same convolution in ONE fp16 MFMA pass ("f16"): an opt-in NARROW arithmetic (11-bit operands), a third of f16x3's MFMA work and half
 * its operand bytes. out = (sum_k fp16(x_k * s_a) * fp16(w_k * s_w)) / (s_a * s_w) + bias (+ resid): products exact, f32 accumulate on
 * v_mfma_f32_16x16x32_f16, descale an exact power-of-two multiply. `in` holds PLAIN fp16 channels-last rows (uv_vae_rms_silu(split_out=3):
 * s_a = 1; uv_vae_cast_f16: s_a found on the device, 1 / s_a passed as act_scale); here ld_in and Cin count CHANNELS (fp16 elements):
 * Cin % 64 == 0, ld_in % 8 == 0. w16 = [Cout][kt*kh*kw*Cin] fp16 of w * w_scale, tap-major and channel-minor (uv_cast_weights_f16; w_scale
 * a power of two by uv_split_weights_f16x3's rule). Everything else as uv_conv3d_f16x3. Launch plan: that of an f16x3 call of HALF the
 * channels, uv_conv3d_plan(4, .., Cin / 2, ..); the kernel it names runs in its plain-row form. */
int uv_conv3d_f16(const float* in, long ld_in, int Tin, int Hin, int Win, const void* w16, const float* bias, float* out, long ldo,
                  int Tout, int Hout, int Wout, int Cin, int Cout, int kt, int kh, int kw, int st, int sh, int sw, int t_off, int ph,
                  int pw, int up, int interleave, const float* resid, long ldr, float w_scale, const float* act_scale, void* stream);
/* w [n] f32 (n % 64 == 0) -> out [n] fp16 = fp16(w * scale), scale = 2^s: the hi pieces of uv_split_weights_f16x3 as one plain matrix */
int uv_cast_weights_f16(const float* w, void* out, long n, float scale, void* stream);
/* uv_vae_split_f16 for uv_conv3d_f16: the same scale search and scale[0] <- 1 / s contract, stream-ordered, no host round trip; `out` rows
 * (ld_out in f32-sized slots, >= C / 2) receive PLAIN fp16: fp16(x * s) of channel c at fp16 slot c = the hi pieces of uv_vae_split_f16.
 * C % 64 == 0. `out` must not alias `x`. */
int uv_vae_cast_f16(const float* x, long ld, float* out, long ld_out, long P, int C, float* scale, void* stream);
/* x [P, C] f32 rows (any feature map; C % 32 == 0) -> `out`: the same bytes per pixel holding [C/32][32 hi | 32 lo] IEEE fp16 pieces of
 * x * s, s a per-tensor power of two found on the device: 1 while max|x| < 2^15 (then this equals uv_vae_rms_silu's split_out=2 format of
 * the same values), else the scale that puts max|x| into [2^14, 2^15). scale: two device floats; scale[0] <- 1 / s for uv_conv3d_f16x3's
 * act_scale, scale[1] = work space. Three stream-ordered operations (memset; split under s = 1 with the maximum found in the same pass; a second
 * launch that writes 1 / s and re-splits only if s != 1); no host round trip. `out` must not alias `x`. */
int uv_vae_split_f16(const float* x, long ld, float* out, long ld_out, long P, int C, float* scale, void* stream);
/* w [n] f32 (rows of K, K % 32 == 0) -> [n/32][32 hi | 32 lo] IEEE fp16 with hi = fp16(w * scale), lo = fp16(w * scale - hi); scale = 2^s */
int uv_split_weights_f16x3(const float* w, void* out, long n, float scale, void* stream);
/* y = x / max(||x||,1e-12) * sqrt(C) * gamma [-> SiLU] per pixel (RMS_norm + SiLU, vae2_2.py:45-59, 201-206).
 * split_out: 0 = f32 rows; 1 = [C/32][32 hi | 32 lo] bf16 pieces (uv_conv3d_bf16x3 in_split); 2 = the same layout in IEEE fp16 (uv_conv3d_f16x3);
 * 3 = plain fp16 (uv_conv3d_f16; C % 64 == 0): the row's C values in its first C / 2 f32-sized slots, bit for bit the hi pieces of 2; the slots
 * behind them are not written. ld_out counts f32-sized slots in every format. */
int uv_vae_rms_silu(const float* in, long ld_in, const float* gamma, float* out, long ld_out, long P, int C, int do_silu,
                    int split_out, void* stream);
/* in-place row softmax of x*scale (AttentionBlock's SDPA, vae2_2.py:267-271) */
int uv_softmax_rows_f32(float* x, long ld, int R, int n, float scale, void* stream);
/* out += DupUp3D(x) (vae2_2.py:390-412); out += AvgDown3D(x) (vae2_2.py:335-367) */
int uv_vae_dupup_add(const float* x, float* out, int T, int H, int W, int Cin, int Cout, int ft, int drop, void* stream);
int uv_vae_avgdown_add(const float* x, float* out, int T, int H, int W, int Cin, int Cout, int ft, int fs, void* stream);
/* latent / video layout conversions at the VAE boundary (vae2_2.py:280-313, 803-808, 814-818, 1045) */
int uv_vae_latent_in(const float* z, const float* mean, const float* inv_std, float* out, long ld, int Z, long P, void* stream);
int uv_vae_latent_out(const float* mu, long ld, const float* mean, const float* inv_std, float* out, int Z, long P, void* stream);
int uv_vae_video_in(const float* vid, float* out, long ld, int F, int H, int W, int f0, int T, void* stream);
int uv_vae_video_out(const float* y, long ld, float* vid, int F, int Hp, int Wp, int f0, int T, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVID_HIP_H */
