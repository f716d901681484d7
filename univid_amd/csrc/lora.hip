// Un-merged LoRA on the GEMM path: the adapter's down-projection T = bf16(s o (x A^T)), written into the slot of whole 128-column
// groups behind the activation's K columns, so that the projection's own GEMM runs as [x | T] [W | B]^T with its fused epilogue
// (include/univid_hip.h: uv_lora_down_bf16). Plus the strided f32 -> bf16 cast that lets the cross_attn_norm = False path write an
// activation buffer that carries such a slot.
#include "common.h"

// ------------------------------------------------------------------------------------------------
// Skinny GEMM, bound by reading x once (M x K bf16; A is at most a few MB and lives in L2).
//   workgroup = 2 waves x 16 rows = 32 rows of x (715 workgroups at M = 22 880: three per CU, resident together - what the chip's HBM
//   rate needs is every CU streaming, and 64-row workgroups would leave 358 of them on 256 CUs), one pass of up to 128 ranks
//   (blockIdx.y; NT = 16-rank tiles computed in it)
//   K in chunks of KC (256, or 128 for the widest pass): x fragments global -> registers (one 16-byte load per lane and 32 k: lane l holds
//   x[row l & 15][8 (l >> 4) ...], the A operand of v_mfma_f32_16x16x32_bf16; 8 KB per wave in flight), the chunk of A global -> registers
//   -> LDS (shared by the two waves; row pitch KC * 2 + 16 bytes so that the 16 rows of a ds_read_b128 fragment fall into different
//   banks); the next chunk's loads are issued before the current chunk's MFMAs.
// Every output element is ONE accumulator slot fed in ascending k: a row's bits do not depend on the other rows of the launch
// (no split-K, no atomics). Columns >= K of x and rows >= M are never read; rows >= R of A are never read (zeros in LDS).
// Epilogue: scale, one rounding to bf16, through LDS to 16-byte row stores; columns [R, Rpad) are stored as 0.
// ------------------------------------------------------------------------------------------------
#define LD_WAVES 2
#define LD_THREADS (LD_WAVES * 64)
#define LD_ROWS (LD_WAVES * 16)
#define LD_OPITCH (128 + 8)

// SEG (uv_lora_down_seg_bf16): the scale is a matrix, one row per segment of seg_rows consecutive rows of x (a stacked sample). The row's
// scale is looked up per output row in the epilogue (a segment boundary may fall anywhere in a 16-row tile), an entry that is == 0
// stores +0 whatever the accumulator holds, and a workgroup whose scale entries of this pass are zero for every segment its 32 rows touch
// skips the pass before the K loop: no read of x, no MFMA, zero stores only. !SEG is uv_lora_down_bf16: it never skips or selects.
template <int NT, int KC, bool SEG>
__global__ __launch_bounds__(LD_THREADS) void lora_down_kernel(const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ A, long lda,
                                                               const float* __restrict__ scale, long ld_scale, int seg_rows, int M, int K, int R,
                                                               bf16_t* out, long ldo) {
    constexpr int PITCH = KC + 8, XS = KC / 32, CPR = KC / 8, AS = NT * 16 * CPR / LD_THREADS;      // x loads / chunks per A row / A loads per lane
    __shared__ __attribute__((aligned(16))) bf16_t sA[NT * 16 * PITCH];
    __shared__ __attribute__((aligned(16))) bf16_t sO[LD_WAVES][16 * LD_OPITCH];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r16 = lane & 15, g = lane >> 4;
    const long row0 = (long)blockIdx.x * LD_ROWS + wave * 16;
    const int j0 = blockIdx.y * 128;                    // first rank of this pass
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    bool live = j0 < R;                                  // (uniform per workgroup: a pass without ranks only stores zeros)
    if constexpr (SEG) {
        if (live) {
            const int m0 = blockIdx.x * LD_ROWS, m1 = min(m0 + LD_ROWS, M) - 1;         // m0 < M: the grid covers M rows
            const int s0 = m0 / seg_rows, ns = m1 / seg_rows - s0 + 1, nr = min(R - j0, 128);
            int on = 0;
            for (int idx = tid; idx < ns * nr; idx += LD_THREADS) on |= scale[(long)(s0 + idx / nr) * ld_scale + j0 + idx % nr] != 0.f;
            live = __syncthreads_or(on) != 0;
        }
    }
    if (live) {
        const long m = row0 + r16;
        const bool row_ok = m < M;
        const bf16_t* xrow = x + (row_ok ? m : 0) * ldx + g * 8;
        f32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        u32x4 xn[XS], an[AS];

        auto fetch = [&](int k0) {
#pragma unroll
            for (int s = 0; s < XS; ++s) {
                const int k = k0 + s * 32;
                xn[s] = (row_ok && k + g * 8 < K) ? *(const u32x4*)(xrow + k) : zero4;
            }
#pragma unroll
            for (int i = 0; i < AS; ++i) {
                const int idx = i * LD_THREADS + tid, r = idx / CPR, c = idx % CPR;
                const int j = j0 + r, k = k0 + c * 8;
                an[i] = (j < R && k < K) ? *(const u32x4*)(A + (long)j * lda + k) : zero4;
            }
        };

        fetch(0);
        for (int k0 = 0; k0 < K; k0 += KC) {
            __syncthreads();                             // the previous chunk's fragment reads are done
            u32x4 xc[XS];
#pragma unroll
            for (int s = 0; s < XS; ++s) xc[s] = xn[s];
#pragma unroll
            for (int i = 0; i < AS; ++i) {
                const int idx = i * LD_THREADS + tid, r = idx / CPR, c = idx % CPR;
                *(u32x4*)(sA + r * PITCH + c * 8) = an[i];
            }
            __syncthreads();
            if (k0 + KC < K) fetch(k0 + KC);
#pragma unroll
            for (int s = 0; s < XS; ++s) {
                const bf16x8 xa = __builtin_bit_cast(bf16x8, xc[s]);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const bf16x8 b = *(const bf16x8*)(sA + (t * 16 + r16) * PITCH + s * 32 + g * 8);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa, b, acc[t], 0, 0, 0);
                }
            }
        }
        // C/D map: column (rank) = lane & 15, row = (lane >> 4) * 4 + i
        int seg[4];                                      // SEG: the segment of each of the lane's four output rows (rows >= M: the last row's)
        if constexpr (SEG) {
#pragma unroll
            for (int i = 0; i < 4; ++i) seg[i] = (int)min(row0 + g * 4 + i, (long)M - 1) / seg_rows;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = t * 16 + r16, j = j0 + col;
            if constexpr (SEG) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float s = j < R ? scale[(long)seg[i] * ld_scale + j] : 0.f;
                    sO[wave][(g * 4 + i) * LD_OPITCH + col] = s != 0.f ? f2bf(__fmul_rn(s, acc[t][i])) : (bf16_t)0;
                }
            } else {
                const float s = j < R ? scale[j] : 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    sO[wave][(g * 4 + i) * LD_OPITCH + col] = j < R ? f2bf(__fmul_rn(s, acc[t][i])) : (bf16_t)0;
            }
        }
        __syncthreads();
    }
    const int ncol = live ? NT * 16 : 0;                // columns of this pass that came through sO
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = q * 64 + lane, r = idx >> 4, c = (idx & 15) * 8;
        const long m = row0 + r;
        if (m < M) *(u32x4*)(out + m * ldo + j0 + c) = c < ncol ? *(const u32x4*)(&sO[wave][r * LD_OPITCH + c]) : zero4;
    }
}

// the argument checks and the launch shared by the two entry points (seg_rows == 0: uv_lora_down_bf16, the scale is one vector)
static int lora_down_launch(const char* fn, const void* x, long ldx, const void* A, long lda, const float* scale, long ld_scale, int seg_rows,
                            int M, int K, int R, void* out, long ldo, int Rpad, void* stream) {
    UV_CHECK_ARG(x && A && scale && out, "%s: null pointer", fn);
    UV_CHECK_ARG(M > 0 && K > 0 && K % 64 == 0, "%s: M = %d, K = %d (K must be a positive multiple of 64)", fn, M, K);
    UV_CHECK_ARG(R >= 1 && R <= Rpad && Rpad % 128 == 0, "%s: R = %d, Rpad = %d (1 <= R <= Rpad, Rpad %% 128 == 0)", fn, R, Rpad);
    UV_CHECK_ARG(ldx >= K && lda >= K && ldo >= Rpad && ldx % 8 == 0 && lda % 8 == 0 && ldo % 8 == 0,
                 "%s: leading dimensions (%ld, %ld, %ld) must cover the rows and be multiples of 8", fn, ldx, lda, ldo);
    UV_CHECK_ARG((((uintptr_t)x | (uintptr_t)A | (uintptr_t)out) & 15) == 0 && ((uintptr_t)scale & 3) == 0, "%s: misaligned pointers", fn);
    const long gx = ((long)M + LD_ROWS - 1) / LD_ROWS;
    UV_CHECK_ARG(gx <= 0x7fffffffL &&Rpad / 128 <= 65535, "%s: launch too large", fn);
    const dim3 grid((unsigned)gx, (unsigned)(Rpad / 128)), block(LD_THREADS);
    const int nr = R < 128 ? R : 128;                    // ranks of the widest pass
    const bf16_t *xp = (const bf16_t*)x, *ap = (const bf16_t*)A;
    bf16_t* op = (bf16_t*)out;
    hipStream_t st = (hipStream_t)stream;
#define LD_LAUNCH(NT, KC)                                                                                                                  \
    do {                                                                                                                                   \
        if (seg_rows) hipLaunchKernelGGL((lora_down_kernel<NT, KC, true>), grid, block, 0, st, xp, ldx, ap, lda, scale, ld_scale, seg_rows, \
                                         M, K, R, op, ldo);                                                                                \
        else hipLaunchKernelGGL((lora_down_kernel<NT, KC, false>), grid, block, 0, st, xp, ldx, ap, lda, scale, 0L, 0, M, K, R, op, ldo);   \
    } while (0)
    if (nr <= 16) LD_LAUNCH(1, 256);
    else if (nr <= 32) LD_LAUNCH(2, 256);
    else if (nr <= 64) LD_LAUNCH(4, 256);
    else LD_LAUNCH(8, 128);
#undef LD_LAUNCH
    UV_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int uv_lora_down_bf16(const void* x, long ldx, const void* A, long lda, const float* scale, int M, int K, int R, void* out,
                                 long ldo, int Rpad, void* stream) {
    return lora_down_launch("uv_lora_down_bf16", x, ldx, A, lda, scale, 0, 0, M, K, R, out, ldo, Rpad, stream);
}

extern "C" int uv_lora_down_seg_bf16(const void* x, long ldx, const void* A, long lda, const float* scale, long ld_scale, int seg_rows, int nseg,
                                     int M, int K, int R, void* out, long ldo, int Rpad, void* stream) {
    UV_CHECK_ARG(seg_rows >= 1 && nseg >= 1 && (long)nseg * seg_rows >= M,
                 "uv_lora_down_seg_bf16: seg_rows = %d, nseg = %d must be >= 1 and cover M = %d rows", seg_rows, nseg, M);
    UV_CHECK_ARG(ld_scale >= R, "uv_lora_down_seg_bf16: ld_scale = %ld < R = %d", ld_scale, R);
    return lora_down_launch("uv_lora_down_seg_bf16", x, ldx, A, lda, scale, ld_scale, seg_rows, M, K, R, out, ldo, Rpad, stream);
}

// out[r][c] = bf16(in[r][c]) for rows with their own leading dimensions (uv_cast_f32_bf16 for an output that carries a LoRA slot)
__global__ void cast_f32_bf16_rows_kernel(const float* in, long ldi, bf16_t* out, long ldo, int R, int C) {
    const int c4 = C >> 2;
    const long total = (long)R * c4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / c4;
        const int c = (int)(i % c4) * 4;
        const f32x4 v = *(const f32x4*)(in + r * ldi + c);
        const u32x2 o = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
        *(u32x2*)(out + r * ldo + c) = o;
    }
}

extern "C" int uv_cast_f32_bf16_rows(const float* in, long ldi, void* out, long ldo, int R, int C, void* stream) {
    UV_CHECK_ARG(in && out && R > 0 && C > 0 && C % 4 == 0 && ldi >= C && ldo >= C && ldi % 4 == 0 && ldo % 4 == 0,
                 "uv_cast_f32_bf16_rows: bad arguments (C and the leading dimensions must be multiples of 4)");
    UV_CHECK_ARG((((uintptr_t)in & 15) | ((uintptr_t)out & 7)) == 0, "uv_cast_f32_bf16_rows: misaligned pointers");
    const int blocks = (int)min(((long)R * (C / 4) + 255) / 256, (long)4096);
    hipLaunchKernelGGL(cast_f32_bf16_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, in, ldi, (bf16_t*)out, ldo, R, C);
    UV_CHECK_LAUNCH("uv_cast_f32_bf16_rows");
    return 0;
}
