// OCP MXFP8 (e4m3fn elements, one e8m0 scale per 32 consecutive K elements of a row) "NT" GEMM on the block-scaled matrix instruction
// v_mfma_scale_f32_16x16x128_f8f6f4, and the bf16 -> MXFP8 quantiser that feeds it. Format, layouts and invariants: include/univid_hip.h.
// The opt-in fast mode of the DiT's two FFN projections (WanModel.set_ffn_precision("mxfp8")): ffn Linear/GELU/Linear and the gated fp32
// residual, models/wan/utils/modules/model.py:212-214, 252-255. The fused epilogues are those of the bf16 GEMM (gemm_bf16_kernels.h).
//
// Kernel: the BM x BN tile / NS-stage LDS ring structure of gemm_bf16_nt_kernel. A K tile of 128 e4m3 elements is 128 bytes per row - the byte
// geometry of the bf16 kernels' 64-element tile - so the LDS-DMA staging and the XOR swizzle carry over; what changes is the fragment
// read, the scale bytes (staged through LDS with the tile: one 4-byte LDS-DMA per row and K tile = the row's four block scales; a lane
// then reads its byte per fragment - loading them per lane straight from global memory cost more than half of the kernel's speed:
// ffn.0 854 -> 1 897 TFLOP/s) and the MFMA (one 16x16x128 instruction per fragment pair and K tile). The product is issued as
// D = Wfrag x Afrag like the bf16 kernels, so a lane ends up with 4 consecutive n of one m.
// Operand lane map of the instruction with 8-bit elements, MEASURED (one-hot W against per-block scale bytes; tests/test_mxfp8.py keeps
// it pinned with exact integer data): lane l = (row r = l & 15, group g = l >> 4) holds K bytes 16 g .. 16 g + 15 in its first four
// operand registers and K bytes 64 + 16 g .. 64 + 16 g + 15 in the last four - the 128-element step is two 64-element halves, each
// spread over the four lane groups like a 16x16x64 step - and the scale operand of lane (r, b) carries the byte of row r's MX block b
// (K elements 32 b .. 32 b + 31). So a lane does NOT hold one whole MX block: block b's 32 bytes sit in lane groups 2 (b & 1) and
// 2 (b & 1) + 1, register half b >> 1.
// Every output element is ONE chain over K: K tile after K tile into the same accumulator, one instruction per K tile, no split-K,
// no atomics - in both tile shapes. A row's bits therefore do not depend on M, the row offset, or which step of the plan computed it.
#include "gemm_bf16_kernels.h"

typedef __attribute__((ext_vector_type(8))) int i32x8;

struct MxArgs {
    GemmArgs g;               // A / W: the e4m3 code bytes (lda / ldw in bytes); everything the shared epilogues read
    const uint8_t* As;        // [M, ld_as] e8m0 scale bytes of A
    const uint8_t* Ws;        // [N, ld_ws] e8m0 scale bytes of W
    long ld_as, ld_ws;
};

// UV_EPI_BF16_T on the plain product's fragment (the lane holds n = nb + 4 fq + {0..3} of m = mb + frow): the 16-bit values are those of
// epi_frag<UV_EPI_BF16> - same additions, same packed rounding - and are then transposed 4 x 4 inside each quad of lanes (three quad
// permutes), after which lane (frow = 4 a + i, fq) owns the rows m = mb + 4 a + {0..3} of column n = nb + 4 fq + i: one 8-byte store along
// m. The exchange moves bits only, so outT[n][m] IS the UV_EPI_BF16 value of [m][n]. Every lane of the wave must be active.
// A ragged M tail stores element by element like epi_frag's T branch (ldo pads M to a multiple of 4 at least).
__device__ __forceinline__ void epi_frag_mx_t(const GemmArgs& p, int mb, int nb, const f32x4& a, int frow, int fq) {
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = a[e];
    if (p.bias) {
        const u32x2 bb = *(const u32x2*)(p.bias + min(nb + 4 * fq, p.N - 4));
        v[0] += in16<false>((bf16_t)(bb[0] & 0xffff));
        v[1] += in16<false>((bf16_t)(bb[0] >> 16));
        v[2] += in16<false>((bf16_t)(bb[1] & 0xffff));
        v[3] += in16<false>((bf16_t)(bb[1] >> 16));
    }
    const uint64_t own = (uint64_t)pack16_2<false>(v[0], v[1]) | (uint64_t)pack16_2<false>(v[2], v[3]) << 32;
    const int i = frow & 3;
    // round r: the lane hands its element i ^ r to lane i ^ r of its quad and takes that lane's element i, which is row 4 a + (i ^ r)
    uint64_t t = (own >> (16 * i) & 0xffffu) << (16 * i);
    {
        const int s1 = (int)(own >> (16 * (i ^ 1)) & 0xffffu);
        const int r1 = __builtin_amdgcn_update_dpp(0, s1, 0xB1, 0xf, 0xf, true);      // quad_perm [1, 0, 3, 2]
        t |= (uint64_t)(uint32_t)r1 << (16 * (i ^ 1));
        const int s2 = (int)(own >> (16 * (i ^ 2)) & 0xffffu);
        const int r2 = __builtin_amdgcn_update_dpp(0, s2, 0x4E, 0xf, 0xf, true);      // quad_perm [2, 3, 0, 1]
        t |= (uint64_t)(uint32_t)r2 << (16 * (i ^ 2));
        const int s3 = (int)(own >> (16 * (i ^ 3)) & 0xffffu);
        const int r3 = __builtin_amdgcn_update_dpp(0, s3, 0x1B, 0xf, 0xf, true);      // quad_perm [3, 2, 1, 0]
        t |= (uint64_t)(uint32_t)r3 << (16 * (i ^ 3));
    }
    const int n = nb + 4 * fq + i, m = mb + (frow & ~3);
    if (n >= p.N || m >= p.M) return;
    bf16_t* op = (bf16_t*)p.out + (long)n * p.ldo + m;
    if (m + 3 < p.M) {
        *(u32x2*)op = (u32x2){(uint32_t)t, (uint32_t)(t >> 32)};
    } else {
        for (int e = 0; e < 4 && m + e < p.M; ++e) op[e] = (bf16_t)(t >> (16 * e) & 0xffffu);
    }
}

template <int BM, int BN, int WM, int WN, int NS, int EPI>
__global__ __launch_bounds__(WM* WN * 64) void gemm_mx_nt_kernel(MxArgs q) {
    const GemmArgs& p = q.g;
    constexpr int NW = WM * WN;
    constexpr int TM = BM / WM / 16;  // 16-row m tiles per wave
    constexpr int TN = BN / WN / 16;
    constexpr int A_BYTES = BM * 128;
    constexpr int W_BYTES = BN * 128;
    constexpr int SC_OFF = A_BYTES + W_BYTES;              // the stage's scale bytes: [BM rows of A | BN rows of W] x 4 blocks
    constexpr int STAGE_BYTES = SC_OFF + (BM + BN) * 4;
    constexpr int SC_ROWS = (BM + BN) / NW;                // scale rows (one dword each) a wave stages per K tile
    constexpr int A_INSTR = BM / 8 / NW;  // glds wave-instructions per wave for the A tile (8 rows x 128 B each)
    constexpr int W_INSTR = BN / 8 / NW;
    static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0 && (BM / WM) % 16 == 0 && (BN / WN) % 16 == 0, "tile/wave mismatch");
    static_assert(SC_ROWS <= 64 && (BM + BN) % NW == 0, "a wave stages at most one scale dword per lane and K tile");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // XCD-aware tile mapping and GM-tall column groups, as in gemm_bf16_nt_kernel
    const int nblk = p.tiles_m * p.tiles_n;
    int bid = blockIdx.x;
    {
        const int qq = nblk >> 3, r = nblk & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + idx;
    }
    constexpr int GM = 4;
    const int group_sz = GM * p.tiles_n;
    const int group = bid / group_sz;
    const int first_m = group * GM;
    const int gm = min(GM, p.tiles_m - first_m);
    const int in_group = bid - group * group_sz;
    const int m0 = (first_m + in_group % gm) * BM, n0 = (in_group / gm) * BN;

    // ---- per-lane staging source pointers (row clamp keeps every load in bounds)
    const uint8_t* const Ac = (const uint8_t*)p.A;
    const uint8_t* const Wc = (const uint8_t*)p.W;
    const int srow = lane >> 3;   // row inside the 8-row glds piece
    const int pchunk = lane & 7;  // physical 16-B chunk inside the 128-B row
    const uint8_t* a_src[A_INSTR];
    const uint8_t* w_src[W_INSTR];
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i) {
        const int row = (i * NW + wave) * 8 + srow;
        const int c = pchunk ^ ((row >> 1) & 7);
        a_src[i] = Ac + (long)min(m0 + row, p.M - 1) * p.lda + c * 16;
    }
#pragma unroll
    for (int i = 0; i < W_INSTR; ++i) {
        const int row = (i * NW + wave) * 8 + srow;
        const int c = pchunk ^ ((row >> 1) & 7);
        w_src[i] = Wc + (long)min(n0 + row, p.N - 1) * p.ldw + c * 16;
    }
    // the wave's scale rows: row wave * SC_ROWS + lane of [A rows | W rows], one dword (the four block scales of the K tile) per row
    const int sc_row = wave * SC_ROWS + lane;
    const bool sc_on = lane < SC_ROWS;
    const uint8_t* const sc_src = sc_row < BM ? q.As + (long)min(m0 + sc_row, p.M - 1) * q.ld_as
                                                      : q.Ws + (long)min(n0 + sc_row - BM, p.N - 1) * q.ld_ws;
    auto stage = [&](int kt, int buf) {
        char* base = smem + buf * STAGE_BYTES;
        const long koff = (long)kt * 128;
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) glds16(a_src[i] + koff, (lds_void*)(base + (i * NW + wave) * 1024));
#pragma unroll
        for (int i = 0; i < W_INSTR; ++i) glds16(w_src[i] + koff, (lds_void*)(base + A_BYTES + (i * NW + wave) * 1024));
        if (sc_on) __builtin_amdgcn_global_load_lds(sc_src + 4 * kt, (lds_void*)(base + SC_OFF + wave * SC_ROWS * 4), 4, 0, 0);
    };

    f32x4 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // fragment reads: row = base + (lane & 15), logical 16-byte chunks fq and 4 + fq (the lane map above); scale byte [row][4 kt + fq]
    const int frow = lane & 15;
    const int fq = lane >> 4;
    // (every fragment row of a lane has the same swizzle key: the rows differ by multiples of 16)
    const int key = (frow >> 1) & 7;
    const int c0 = (fq ^ key) << 4, c1 = c0 ^ 64;
    const int a_row0 = (wm * (BM / WM) + frow) * 128, w_row0 = A_BYTES + (wn * (BN / WN) + frow) * 128;
    const int a_sc0 = SC_OFF + (wm * (BM / WM) + frow) * 4 + fq, w_sc0 = SC_OFF + (BM + wn * (BN / WN) + frow) * 4 + fq;
    auto frag = [&](const char* row) {
        const u32x4 lo = *(const u32x4*)(row + c0);
        const u32x4 hi = *(const u32x4*)(row + c1);
        return (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    };
    // (A fragments four at a time: eight of them beside the 128 accumulator registers of the 256x256 tile would spill)
    constexpr int JH = TM > 4 ? 4 : TM;
    auto compute = [&](const char* base) {
        int sa[TM], sw[TN];
#pragma unroll
        for (int j = 0; j < TM; ++j) sa[j] = *(const uint8_t*)(base + a_sc0 + j * 64);
#pragma unroll
        for (int i = 0; i < TN; ++i) sw[i] = *(const uint8_t*)(base + w_sc0 + i * 64);
#pragma unroll
        for (int j0 = 0; j0 < TM; j0 += JH) {
            i32x8 af[JH];
#pragma unroll
            for (int j = 0; j < JH; ++j) af[j] = frag(base + a_row0 + (j0 + j) * 2048);
#pragma unroll
            for (int i = 0; i < TN; ++i) {
                const i32x8 wf = frag(base + w_row0 + i * 2048);
#pragma unroll
                for (int j = 0; j < JH; ++j)
                    acc[i][j0 + j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf, af[j], acc[i][j0 + j], 0, 0, 0, sw[i], 0, sa[j0 + j]);
            }
        }
    };

    // NS-deep ring (the schedule of gemm_bf16_nt_kernel's ring form): NS - 1 K tiles stay in flight across raw barriers, the only VMEM
    // wait is a counted vmcnt. After barrier kt every wave has finished the MFMAs (so the LDS reads) of tile kt - 1: its buffer can
    // take tile kt + NS - 1. Every wave issues the same LPS loads per K tile (the scale dword with part of its lanes when SC_ROWS < 64).
    constexpr int LPS = A_INSTR + W_INSTR + 1;
    static_assert((NS - 2) * LPS < 64, "vmcnt range");
    const int nk = p.K / 128;
#pragma unroll
    for (int s0 = 0; s0 < NS - 1; ++s0)
        if (s0 < nk) stage(s0, s0);
    int buf = 0, nbuf = NS - 1;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + NS - 2 < nk) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * LPS) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        if (kt + NS - 1 < nk) stage(kt + NS - 1, nbuf);
        compute(smem + buf * STAGE_BYTES);
        buf = buf + 1 == NS ? 0 : buf + 1;
        nbuf = nbuf + 1 == NS ? 0 : nbuf + 1;
    }

    // ---- epilogue: the bf16 GEMM's device code, fragment by fragment
    if constexpr (EPI == UV_EPI_RESID_F32 || EPI == UV_EPI_GATE_RESID_F32) {
        constexpr int NF = TM * TN;
        int mb[NF], nb[NF];
        f32x4 av[NF];
#pragma unroll
        for (int j = 0; j < TM; ++j)
#pragma unroll
            for (int i = 0; i < TN; ++i) {
                mb[j * TN + i] = m0 + wm * (BM / WM) + j * 16;
                nb[j * TN + i] = n0 + wn * (BN / WN) + i * 16;
                av[j * TN + i] = acc[i][j];
            }
        epi_rmw_pipe<EPI, NF, (NF >= 8 ? 4 : 2)>(p, mb, nb, av, frow, fq);
    } else if constexpr (EPI == UV_EPI_BF16_SSQ) {
        static_assert(TN % 2 == 0 && (BN / WN) % 32 == 0, "UV_EPI_BF16_SSQ needs whole 32-column groups per wave");
#pragma unroll
        for (int j = 0; j < TM; ++j)
#pragma unroll
            for (int i = 0; i < TN; i += 2)
                epi_pair_ssq<false>(p, m0 + wm * (BM / WM) + j * 16, n0 + wn * (BN / WN) + i * 16, acc[i][j], acc[i + 1][j], frow, fq);
    } else if constexpr (EPI == UV_EPI_BF16_T) {
#pragma unroll
        for (int j = 0; j < TM; ++j)
#pragma unroll
            for (int i = 0; i < TN; ++i)
                epi_frag_mx_t(p, m0 + wm * (BM / WM) + j * 16, n0 + wn * (BN / WN) + i * 16, acc[i][j], frow, fq);
    } else {
#pragma unroll
        for (int j = 0; j < TM; ++j)
#pragma unroll
            for (int i = 0; i < TN; ++i)
                epi_frag<EPI>(p, m0 + wm * (BM / WM) + j * 16, n0 + wn * (BN / WN) + i * 16, acc[i][j], frow, fq);
    }
}

// ---- plan: which rows go to which tile shape ------------------------------------------------------------------------------------------
enum MxKernel {
    MK_T256,      // 256x256 tiles, 8 waves, 2 stages (135 KiB of LDS: one workgroup per CU)
    MK_T128,      // 128x128 tiles, 4 waves, 2 stages (two workgroups per CU): problems under one round of 256x256 tiles
};
struct MxStep { MxKernel kernel; int m0, rows; };      // rows m0 .. m0 + rows - 1
struct MxPlan { int n; MxStep step[2]; };

// Pure. 256x256 tiles once they fill at least one round of the chip (a ragged last row tile rides along: 96 of 22 880 rows at the DiT's
// shape, under 1 % of the tiles' work), 128x128 tiles for smaller problems. Same arithmetic per element either way. One step today; the
// launcher runs whatever steps a plan names, so a leftover-row strip would be decided here and nowhere else.
static MxPlan plan_gemm_mx(int M, int N, int ncus) {
    const long tiles = (long)((M + 255) / 256) * (N / 256);
    return MxPlan{1, {{tiles >= ncus ? MK_T256 : MK_T128, 0, M}}};
}

static MxArgs mx_rows_of(const MxArgs& a, int epilogue, long m0, int rows) {
    MxArgs r = a;
    r.g.M = rows;
    r.g.A = (const bf16_t*)((const uint8_t*)a.g.A + m0 * a.g.lda);
    r.As = a.As + m0 * a.ld_as;
    if (a.g.gate_tid) r.g.gate_tid = a.g.gate_tid + m0;
    if (a.g.ssq) r.g.ssq = a.g.ssq + m0 * a.g.ld_ssq;
    if (epilogue == UV_EPI_BF16_T) r.g.out = (bf16_t*)a.g.out + m0;
    else if (epilogue == UV_EPI_BF16 || epilogue == UV_EPI_GELU_BF16 || epilogue == UV_EPI_BF16_SSQ) r.g.out = (bf16_t*)a.g.out + m0 * a.g.ldo;
    else r.g.out = (float*)a.g.out + m0 * a.g.ldo;
    return r;
}

constexpr unsigned UV_MX_EPIS = 1u << UV_EPI_BF16 | 1u << UV_EPI_GELU_BF16 | 1u << UV_EPI_F32_FROM_BF16 | 1u << UV_EPI_RESID_F32 |
                                1u << UV_EPI_GATE_RESID_F32;
// (every epilogue the kernel is built with; each entry point accepts its own subset: uv_gemm_mxfp8_nt the five above)
constexpr unsigned UV_MX_EPIS_BUILT = UV_MX_EPIS | 1u << UV_EPI_BF16_T | 1u << UV_EPI_BF16_SSQ;

template <int BM, int BN, int WM, int WN, int NS>
static int launch_mx(const MxArgs& a0, int epi, const char* fn, hipStream_t stream) {
    MxArgs a = a0;
    a.g.tiles_m = (a.g.M + BM - 1) / BM;
    a.g.tiles_n = a.g.N / BN;
    const dim3 grid(a.g.tiles_m * a.g.tiles_n);
    constexpr int LDS = NS * (BM + BN) * 132;
    return launch_epi<UV_MX_EPIS_BUILT>(epi, [&](auto e) {
        auto kern = gemm_mx_nt_kernel<BM, BN, WM, WN, NS, decltype(e)::value>;
        UV_ONCE_PER_DEVICE(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
        hipLaunchKernelGGL(kern, grid, dim3(WM * WN * 64), LDS, stream, a);
        UV_CHECK_LAUNCH(fn);
        return 0;
    });
}

// The one body of the three entry points. `fn`: the entry point's name (error texts); `epis`: the epilogues it accepts.
static int gemm_mx_entry(const char* fn, unsigned epis, const void* A, long lda, const void* A_scale, long ld_as, const void* W, long ldw,
                         const void* W_scale, long ld_ws, const void* bias_bf16, int M, int N, int K, int epilogue, void* out, long ldo,
                         const float* gate, const int32_t* gate_tid, long gate_stride, float* ssq, long ld_ssq, void* stream) {
    UV_CHECK_ARG(A && W && out, "%s: null pointer", fn);
    UV_CHECK_ARG(A_scale && W_scale, "%s: null scale pointer", fn);
    UV_CHECK_ARG(M > 0 && N > 0 && K > 0, "%s: bad shape M=%d N=%d K=%d", fn, M, N, K);
    UV_CHECK_ARG(K % 128 == 0, "%s: K=%d must be a multiple of 128", fn, K);
    UV_CHECK_ARG(N % 256 == 0, "%s: N=%d must be a multiple of 256", fn, N);
    UV_CHECK_ARG(epi_in(epis, epilogue), "%s: epilogue %d is not built for MXFP8 operands here", fn, epilogue);
    UV_CHECK_ARG(lda >= K && ldw >= K && lda % 16 == 0 && ldw % 16 == 0, "%s: lda/ldw must be >= K and multiples of 16 bytes", fn);
    UV_CHECK_ARG(ld_as >= K / 32 && ld_ws >= K / 32 && ld_as % 4 == 0 && ld_ws % 4 == 0,
                 "%s: ld_as/ld_ws must be >= K / 32 = %d and multiples of 4 (ld_as=%ld ld_ws=%ld)", fn, K / 32, ld_as, ld_ws);
    UV_CHECK_ARG(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)out & 15) == 0,
                 "%s: pointers must be 16-byte aligned", fn);
    UV_CHECK_ARG(((uintptr_t)A_scale & 3) == 0 && ((uintptr_t)W_scale & 3) == 0 && ((uintptr_t)bias_bf16 & 7) == 0,
                 "%s: scale pointers must be 4-byte, the bias 8-byte aligned", fn);
    UV_CHECK_ARG((long)M * ld_as < (1L << 31) && (long)N * ld_ws < (1L << 31), "%s: scale arrays of 2 GiB and more are not supported", fn);
    if (epilogue == UV_EPI_BF16_T)
        UV_CHECK_ARG(ldo >= M && ldo % 4 == 0, "%s: ldo must be >= M and a multiple of 4 elements", fn);
    else
        UV_CHECK_ARG(ldo >= N && ldo % 4 == 0, "%s: ldo must be >= N and a multiple of 4 elements", fn);
    if (epilogue == UV_EPI_BF16_SSQ)
        UV_CHECK_ARG(ssq && ((uintptr_t)ssq & 3) == 0 && ld_ssq >= N / 32, "%s: ssq required, ld_ssq >= N / 32 = %d (ld_ssq=%ld)", fn, N / 32, ld_ssq);
    if (epilogue == UV_EPI_GATE_RESID_F32)
        UV_CHECK_ARG(gate && gate_stride % 4 == 0, "%s: gate table required (stride %% 4 == 0)", fn);
    MxArgs a;
    GemmArgs& g = a.g;
    g.A = (const bf16_t*)A; g.W = (const bf16_t*)W; g.bias = (const bf16_t*)bias_bf16;
    g.out = out; g.gate = gate; g.gate_tid = gate_tid;
    g.lda = lda; g.ldw = ldw; g.ldo = ldo; g.gate_stride = gate_stride;
    g.M = M; g.N = N; g.K = K; g.tiles_m = g.tiles_n = 0;
    g.ssq = ssq; g.ld_ssq = ld_ssq; g.ws_slab = nullptr; g.ws_cnt = nullptr; g.gm = 0;
    g.zeros = uv_zero_page();
    UV_CHECK_ARG(g.zeros, "%s: zero page missing (call uv_init)", fn);
    a.As = (const uint8_t*)A_scale; a.Ws = (const uint8_t*)W_scale;
    a.ld_as = ld_as; a.ld_ws = ld_ws;
    const MxPlan plan = plan_gemm_mx(M, N, uv_num_cus());
    for (int i = 0; i < plan.n; ++i) {
        const MxStep& st = plan.step[i];
        const MxArgs r = mx_rows_of(a, epilogue, st.m0, st.rows);
        const int rc = st.kernel == MK_T256 ? launch_mx<256, 256, 2, 4, 2>(r, epilogue, fn, (hipStream_t)stream)
                                            : launch_mx<128, 128, 2, 2, 2>(r, epilogue, fn, (hipStream_t)stream);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int uv_gemm_mxfp8_nt(const void* A, long lda, const void* A_scale, long ld_as, const void* W, long ldw, const void* W_scale,
                                long ld_ws, const void* bias_bf16, int M, int N, int K, int epilogue, void* out, long ldo,
                                const float* gate, const int32_t* gate_tid, long gate_stride, void* stream) {
    return gemm_mx_entry("uv_gemm_mxfp8_nt", UV_MX_EPIS, A, lda, A_scale, ld_as, W, ldw, W_scale, ld_ws, bias_bf16, M, N, K, epilogue, out, ldo,
                         gate, gate_tid, gate_stride, nullptr, 0, stream);
}

// outT[n][m] = the bits uv_gemm_mxfp8_nt(UV_EPI_BF16) writes at [m][n] (V^T for the attention kernels): same checks, plan and K chain.
extern "C" int uv_gemm_mxfp8_nt_t(const void* A, long lda, const void* A_scale, long ld_as, const void* W, long ldw, const void* W_scale,
                                  long ld_ws, const void* bias_bf16, int M, int N, int K, void* outT, long ldo, void* stream) {
    return gemm_mx_entry("uv_gemm_mxfp8_nt_t", 1u << UV_EPI_BF16_T, A, lda, A_scale, ld_as, W, ldw, W_scale, ld_ws, bias_bf16, M, N, K,
                         UV_EPI_BF16_T, outT, ldo, nullptr, nullptr, 0, nullptr, 0, stream);
}

// UV_EPI_BF16's output plus ssq[m][n / 32], the header's one summation order (ssq_group32): the cross-attention q projection in front of
// uv_rms_scale_from_ssq and the q-norm attention kernel.
extern "C" int uv_gemm_mxfp8_nt_ssq(const void* A, long lda, const void* A_scale, long ld_as, const void* W, long ldw, const void* W_scale,
                                    long ld_ws, const void* bias_bf16, int M, int N, int K, void* out, long ldo, float* ssq, long ld_ssq,
                                    void* stream) {
    return gemm_mx_entry("uv_gemm_mxfp8_nt_ssq", 1u << UV_EPI_BF16_SSQ, A, lda, A_scale, ld_as, W, ldw, W_scale, ld_ws, bias_bf16, M, N, K,
                         UV_EPI_BF16_SSQ, out, ldo, nullptr, nullptr, 0, ssq, ld_ssq, stream);
}

// ---- quantiser ------------------------------------------------------------------------------------------------------------------------
// One lane = 16 consecutive elements of a row (two 16-byte loads, one 16-byte store), two lanes = one MX block, eight lanes = the four
// blocks of one 128-element group, whose scale bytes leave as one dword. Everything a lane computes comes from its own block: the bytes
// are a pure function of the input row.
__global__ __launch_bounds__(256) void mx_quant_bf16_kernel(const bf16_t* __restrict__ x, long ldx, uint8_t* __restrict__ codes, long ldc,
                                                            uint8_t* __restrict__ scales, long ld_s, long total, int lanes_per_row) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    // (whole groups of 8 lanes are inside or outside: total % 8 == 0; the shuffles below stay inside a group of 8)
    const bool live = t < total;
    const long row = live ? t / lanes_per_row : 0;
    const int c16 = live ? (int)(t - row * lanes_per_row) : 0;
    const u32x4* src = (const u32x4*)(x + row * ldx + (long)c16 * 16);
    u32x4 in[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    if (live) {
        in[0] = src[0];
        in[1] = src[1];
    }
    float v[16];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[h * 8 + 2 * e] = __builtin_bit_cast(float, in[h][e] << 16);
            v[h * 8 + 2 * e + 1] = __builtin_bit_cast(float, in[h][e] & 0xffff0000u);
        }
    // amax through the integer magnitudes (monotonic for finite values; no NaN semantics of a floating-point maximum involved)
    uint32_t amax = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) amax = max(amax, __builtin_bit_cast(uint32_t, v[e]) & 0x7fffffffu);
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1, 64));
    const int eb = max((int)(amax >> 23) - 8, 0);                            // the e8m0 byte: 2^(floor(log2 amax) - 8), clamped below
    const float inv = __builtin_bit_cast(float, (uint32_t)(254 - eb) << 23); // 2^(127 - eb): a normal f32 for every eb a bf16 amax can give
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float s[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = fminf(fmaxf(__fmul_rn(v[4 * e + i], inv), -448.f), 448.f);      // exact scaling, explicit clamp
        int pk = __builtin_amdgcn_cvt_pk_fp8_f32(s[0], s[1], 0, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(s[2], s[3], pk, true);
        w[e] = (uint32_t)pk;
    }
    // the four scale bytes of the 128-element group, gathered in its first lane
    const int l8 = threadIdx.x & 7;
    const int base = (threadIdx.x & 63) - l8;
    const uint32_t e1 = (uint32_t)__shfl(eb, base + 2, 64), e2 = (uint32_t)__shfl(eb, base + 4, 64), e3 = (uint32_t)__shfl(eb, base + 6, 64);
    if (!live) return;
    *(u32x4*)(codes + row * ldc + (long)c16 * 16) = (u32x4){w[0], w[1], w[2], w[3]};
    if (l8 == 0) *(uint32_t*)(scales + row * ld_s + (c16 >> 3) * 4) = (uint32_t)eb | e1 << 8 | e2 << 16 | e3 << 24;
}

extern "C" int uv_mx_quant_bf16(const void* x, long ldx, void* codes, long ldc, void* scales, long ld_s, int M, int K, void* stream) {
    UV_CHECK_ARG(x && codes && scales, "uv_mx_quant_bf16: null pointer");
    UV_CHECK_ARG(M > 0 && K > 0, "uv_mx_quant_bf16: bad shape M=%d K=%d", M, K);
    UV_CHECK_ARG(K % 128 == 0, "uv_mx_quant_bf16: K=%d must be a multiple of 128", K);
    UV_CHECK_ARG(ldx >= K && ldx % 8 == 0, "uv_mx_quant_bf16: ldx must be >= K and a multiple of 8 elements");
    UV_CHECK_ARG(ldc >= K && ldc % 16 == 0, "uv_mx_quant_bf16: ldc must be >= K and a multiple of 16 bytes");
    UV_CHECK_ARG(ld_s >= K / 32 && ld_s % 4 == 0, "uv_mx_quant_bf16: ld_s must be >= K / 32 = %d and a multiple of 4 (ld_s=%ld)", K / 32, ld_s);
    UV_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)codes & 15) == 0 && ((uintptr_t)scales & 3) == 0,
                 "uv_mx_quant_bf16: x / codes must be 16-byte, scales 4-byte aligned");
    const int lanes_per_row = K / 16;
    const long total = (long)M * lanes_per_row;
    const long blocks = (total + 255) / 256;
    UV_CHECK_ARG(blocks <= 0x7fffffffL, "uv_mx_quant_bf16: too many elements (M=%d K=%d)", M, K);
    hipLaunchKernelGGL(mx_quant_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, (uint8_t*)codes,
                       ldc, (uint8_t*)scales, ld_s, total, lanes_per_row);
    UV_CHECK_LAUNCH("uv_mx_quant_bf16");
    return 0;
}
