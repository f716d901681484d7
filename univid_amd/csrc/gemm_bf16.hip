// bf16 / fp16 "NT" GEMM entry points: C[M,N] = A[M,K] . W[N,K]^T (+ bias) with the fused epilogues the Wan DiT block needs.
// Kernels and launch helpers: gemm_bf16_kernels.h (the reference lines each epilogue replaces are cited there). This file holds
// plan_gemm - the ONE place that decides which rows of a call go to which kernel (the shape-based choice of tile_cfg 0, the leftover-row
// split, the numbered configurations) - and the entry points that run its steps; configurations that only tests and developer tools
// select live in gemm_bf16_diag.hip.
#include "gemm_bf16_kernels.h"
#include <limits.h>

// gemm_bf16_diag.hip: tile_cfg 2, 3, 4, 10, 11, 13, 14 (A/B and race-screen references; bf16 only)
int uv_gemm_diag_launch(const GemmArgs& a, int epilogue, int tile_cfg, hipStream_t s);

// The caller's split-K workspace (uv_gemm_bf16_nt_ws), or nothing.
struct GemmWs { void* p = nullptr; long bytes = 0; };

enum GemmKernel {
    GK_PERSIST,      // persistent 8-wave ping-pong kernel, whole 256x256 tiles (tile_cfg 17)
    GK_PINGPONG,     // the same schedule (VAR 5), one tile per workgroup (tile_cfg 7)
    GK_RING128,      // 128x128 tiles, 8 waves, 4-stage ring (tile_cfg 12)
    GK_T128,         // 128x128 tiles, 4 waves, 2 stages (tile_cfg 1)
    GK_T256,         // 256x256 tiles, 16 waves (tile_cfg 5)
    GK_T256x192,     // 256x192 tiles, 16 waves (tile_cfg 6)
    GK_SPLITK4,      // one-tile ping-pong kernel x split-K 4 / 2 through the workspace (tile_cfg 19 / 20)
    GK_SPLITK2,
    GK_DIAG,         // pass tile_cfg on to gemm_bf16_diag.hip
};
// their names, as uv_gemm_plan reports them (GK_DIAG: followed by the tile_cfg it passes on, "DIAG14")
static const char* const kGemmKernelName[] = {"PERSIST", "PINGPONG", "RING128", "T128", "T256", "T256x192", "SPLITK4", "SPLITK2", "DIAG"};
struct GemmStep { GemmKernel kernel; int m0, rows; };      // rows m0 .. m0 + rows - 1
struct GemmPlan { int n; GemmStep step[2]; };

// The two row cuts, both multiples of 256 rows. Rows below the cut fill 256x256 tiles; the rows from the cut on (which would otherwise
// cost a whole extra round of tiles on a fraction of the CUs) run as a strip of their own. Same arithmetic per element either way.
// whole_rounds_cut (tile_cfg 8 / 9 / 18 and the short problems of tile_cfg 0): the row tiles of the whole rounds of the chip.
static long whole_rounds_cut(int M, int N, int ncus) {
    const long tiles_n = (N + 255) / 256, tiles_m = (M + 255) / 256;
    const long rounds = tiles_m * tiles_n / ncus;
    return rounds * ncus / tiles_n * 256;
}
// persistent_cut (tile_cfg 0, N % 256 == 0): every whole 256-row tile - or, when the tile count is just above a whole number of rounds
// (the partial round under 45 % full: *short_round), only the whole rounds.
static long persistent_cut(int M, int N, int ncus, bool* short_round) {
    const long tiles = (long)((M + 255) / 256) * (N / 256);
    const long rounds = tiles / ncus, rest = tiles - rounds * ncus;
    *short_round = rounds >= 1 && rest > 0 && rest * 100 < 45 * ncus;
    return *short_round ? whole_rounds_cut(M, N, ncus) : (long)(M / 256) * 256;
}

// Which rows of C[M, N] = A[M, K] . W[N, K]^T go to which kernel: at most two steps. Pure (the device's CU count and the caller's
// workspace come in as numbers), so uv_gemm_splitk_ws_bytes sizes the workspace from the very decision the launch will take.
static GemmPlan plan_gemm(int M, int N, int K, int epilogue, long ldo, int tile_cfg, bool F16, int ncus, long ws_bytes, bool ws_aligned) {
    auto whole = [&](GemmKernel k) { return GemmPlan{1, {{k, 0, M}}}; };
    // a cut of 0 or at / beyond M leaves the whole problem to `main`
    auto cut_at = [&](long cut, GemmKernel main, GemmKernel strip) {
        return cut <= 0 || cut >= M ? whole(main) : GemmPlan{2, {{main, 0, (int)cut}, {strip, (int)cut, M - (int)cut}}};
    };
    switch (tile_cfg) {
        case 0: break;
        case 1: return whole(GK_T128);
        case 5: return whole(GK_T256);
        case 6: return whole(GK_T256x192);
        case 7: return whole(GK_PINGPONG);
        case 8: return cut_at(whole_rounds_cut(M, N, ncus), GK_PINGPONG, GK_RING128);
        case 9: return cut_at(whole_rounds_cut(M, N, ncus), GK_T256, GK_RING128);
        case 12: return whole(GK_RING128);
        case 17: return whole(GK_PERSIST);
        case 18: {      // the persistent kernel + a strip of the rows beyond the last whole tile; in whole tiles: the whole-rounds cut
            const long tm = (long)(M / 256) * 256;
            return cut_at(tm > 0 && tm < M ? tm : whole_rounds_cut(M, N, ncus), GK_PERSIST, GK_RING128);
        }
        case 19: return whole(GK_SPLITK4);      // tests / tools: the WHOLE problem as split-K
        case 20: return whole(GK_SPLITK2);
        default: return whole(GK_DIAG);
    }
    if (M >= 2048 && N >= 1024 && N % 256 == 0 && K % 128 == 0 && K >= 384 &&
        (ldo % 8 == 0 || epilogue == UV_EPI_BF16_T || (epilogue >= UV_EPI_F32_FROM_BF16 && epilogue != UV_EPI_BF16_SSQ))) {
        // Large projections: 256x256 tiles on the PERSISTENT 8-wave ping-pong kernel (one workgroup per CU walking its tile
        // list). It takes whole tiles only; rows beyond the last multiple of 256 - and, when the tile count is just above a
        // whole number of rounds, the rows of that partial round - run as 128x128 tiles on the small-tile kernel.
        bool short_round = false;
        const long cut = persistent_cut(M, N, ncus, &short_round);
        // under two rounds of work (or a transposed output whose leading dimension does not allow the persistent kernel's 16-byte
        // stores): the one-tile-per-workgroup launch
        if (cut / 256 * (N / 256) < 2L * ncus || (epilogue == UV_EPI_BF16_T && ldo % 8 != 0))
            return short_round ? cut_at(whole_rounds_cut(M, N, ncus), GK_PINGPONG, GK_RING128) : whole(GK_PINGPONG);
        // Does the strip run as ONE round of 256x256 tiles x split-K 4? Only where that measured faster than the 128x128 ring
        // (tools/gemm_bench.py, round 6): the long-K strips (ffn.2: K = 14 336, 144 -> 121 us in isolation); at K = 3 072 a slice is
        // 12 K tiles and the publish + combine (~40 us: 63 MB of partial tiles out and back in) costs more than the whole ring launch
        // (63 against 35 us). Needs the residual / bf16 epilogues, whole slices, at most one round of workgroups, and a caller-provided
        // workspace.
        const int rows = M - (int)cut;
        const long strip_tiles = (long)((rows + 255) / 256) * (N / 256);
        const bool splitk = !F16 && (epilogue == UV_EPI_BF16 || epilogue == UV_EPI_RESID_F32 || epilogue == UV_EPI_GATE_RESID_F32) &&
                            K >= 8192 && K % 512 == 0 && strip_tiles * 4 <= ncus && ws_aligned && ws_bytes >= splitk_ws_bytes(rows, N, 4);
        return cut_at(cut, GK_PERSIST, splitk ? GK_SPLITK4 : GK_RING128);
    }
    if (M < 2048 || N < 1024) {
        // tall and narrow (the SigLIP2 towers: 16 384 x 768): 256x256 tiles on the ping-pong kernel beat 128x128 tiles even
        // at 3/4 of a round of workgroups (q / k / v / o 33.7 -> 30.1 us, fc2 with K = 3072 89.7 -> 71.9 us)
        if (M >= 4096 && N >= 512 && N % 256 == 0 && K % 128 == 0 && K >= 256 && ldo % 8 == 0 && M % 256 == 0 &&
            2L * (M / 256) * (N / 256) >= ncus)
            return whole(GK_PINGPONG);
        // few tiles (at most ~2 per CU): 8 waves on a 4-stage ring hide the DMA/LDS latency that one 4-wave
        // workgroup per CU leaves exposed; many tiles: 4-wave workgroups, 2-3 resident per CU
        const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
        return whole(t128 <= 2 * ncus ? GK_RING128 : GK_T128);
    }
    const long tm = (M + 255) / 256;
    const long t256 = tm * ((N + 255) / 256), t192 = tm * ((N + 191) / 192);
    // cost ~ rounds x tile area; 256x192 tiles carry 3/4 of the work of 256x256 at slightly lower efficiency
    const double c256 = (double)((t256 + 255) / 256) * 1.00, c192 = (double)((t192 + 255) / 256) * 0.78;
    return whole(!F16 && N % 192 == 0 && c192 < c256 && K <= 4096 && epilogue != UV_EPI_BF16_SSQ ? GK_T256x192 : GK_T256);
}

// `a` cut to its rows m0 .. m0 + rows - 1.
static GemmArgs rows_of(const GemmArgs& a, int epilogue, long m0, int rows) {
    GemmArgs r = a;
    r.M = rows;
    r.A = a.A + m0 * a.lda;
    if (a.gate_tid) r.gate_tid = a.gate_tid + m0;
    if (a.ssq) r.ssq = a.ssq + m0 * a.ld_ssq;
    if (epilogue == UV_EPI_BF16_T) r.out = (bf16_t*)a.out + m0;
    else if (epilogue == UV_EPI_BF16 || epilogue == UV_EPI_GELU_BF16 || epilogue == UV_EPI_BF16_SSQ) r.out = (bf16_t*)a.out + m0 * a.ldo;
    else r.out = (float*)a.out + m0 * a.ldo;
    return r;
}

// One step of a plan. Only the kernels tile_cfg 0 picks are built for fp16 operands.
template <bool F16>
static int launch_step(GemmKernel kernel, const GemmArgs& a, int epilogue, int tile_cfg, hipStream_t s, const GemmWs& ws) {
    switch (kernel) {
        case GK_PERSIST:
            UV_CHECK_ARG(a.K % 128 == 0 && a.K >= 384, "uv_gemm_bf16_nt: tile_cfg 17 needs K %% 128 == 0 and K >= 384 (K=%d)", a.K);
            return launch_8ph_persist<F16>(a, epilogue, s);
        case GK_PINGPONG:
            UV_CHECK_ARG(a.K % 128 == 0 && a.K >= 256, "uv_gemm_bf16_nt: tile_cfg 7 needs K %% 128 == 0 and K >= 256 (K=%d)", a.K);
            return launch_8ph<5, F16>(a, epilogue, s);
        case GK_RING128: return launch_cfg<128, 128, 4, 2, 4, F16>(a, epilogue, s);
        case GK_T128: return launch_cfg<128, 128, 2, 2, 2, F16>(a, epilogue, s);
        case GK_T256: return launch_cfg<256, 256, 4, 4, 2, F16>(a, epilogue, s);
        case GK_T256x192: if constexpr (!F16) return launch_cfg<256, 192, 4, 4>(a, epilogue, s); break;
        case GK_SPLITK4: if constexpr (!F16) return launch_8ph_splitk<4, false>(a, epilogue, s, ws.p, ws.bytes); break;
        case GK_SPLITK2: if constexpr (!F16) return launch_8ph_splitk<2, false>(a, epilogue, s, ws.p, ws.bytes); break;
        case GK_DIAG: if constexpr (!F16) return uv_gemm_diag_launch(a, epilogue, tile_cfg, s); break;      // test / tool configurations
    }
    uv_set_error("uv_gemm_f16_nt: tile_cfg %d is not built for fp16 operands", tile_cfg);
    return -1;
}

template <bool F16>
static int gemm_entry(const void* A, long lda, const void* W, long ldw, const void* bias_bf16, int M, int N, int K, int epilogue,
                      void* out, long ldo, const float* gate, const int32_t* gate_tid, long gate_stride, int tile_cfg, void* stream,
                      float* ssq = nullptr, long ld_ssq = 0, const GemmWs& ws = GemmWs()) {
    UV_CHECK_ARG(A && W && out, "uv_gemm_bf16_nt: null pointer");
    UV_CHECK_ARG(M > 0 && N > 0 && K > 0, "uv_gemm_bf16_nt: bad shape M=%d N=%d K=%d", M, N, K);
    UV_CHECK_ARG(K % UV_BK == 0, "uv_gemm_bf16_nt: K=%d must be a multiple of %d", K, UV_BK);
    UV_CHECK_ARG(N % 16 == 0, "uv_gemm_bf16_nt: N=%d must be a multiple of 16", N);
    UV_CHECK_ARG(lda % 8 == 0 && ldw % 8 == 0, "uv_gemm_bf16_nt: lda/ldw must be multiples of 8 elements");
    UV_CHECK_ARG(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)out & 15) == 0,
                 "uv_gemm_bf16_nt: pointers must be 16-byte aligned");
    UV_CHECK_ARG(ldo % 4 == 0, "uv_gemm_bf16_nt: ldo must be a multiple of 4 elements");
    if (epilogue == UV_EPI_GATE_RESID_F32)
        UV_CHECK_ARG(gate && gate_stride % 4 == 0, "uv_gemm_bf16_nt: gate table required (stride %% 4 == 0)");
    GemmArgs a;
    a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.bias = (const bf16_t*)bias_bf16;
    a.out = out; a.gate = gate; a.gate_tid = gate_tid;
    a.lda = lda; a.ldw = ldw; a.ldo = ldo; a.gate_stride = gate_stride;
    a.M = M; a.N = N; a.K = K; a.tiles_m = a.tiles_n = 0;
    a.ssq = ssq; a.ld_ssq = ld_ssq;
    a.ws_slab = nullptr; a.ws_cnt = nullptr; a.gm = 0;
    if (epilogue == UV_EPI_BF16_SSQ)
        UV_CHECK_ARG(ssq && N % 32 == 0 && ld_ssq >= N / 32 && ldo % 8 == 0, "uv_gemm_bf16_nt_ssq: needs N %% 32 == 0, ld_ssq >= N / 32, ldo %% 8 == 0 (N=%d ld_ssq=%ld ldo=%ld)", N, ld_ssq, ldo);
    a.zeros = uv_zero_page();
    UV_CHECK_ARG(a.zeros, "uv_gemm_bf16_nt: zero page missing (call uv_init)");
    const GemmPlan plan = plan_gemm(M, N, K, epilogue, ldo, tile_cfg, F16, uv_num_cus(), ws.p ? ws.bytes : 0, ((uintptr_t)ws.p & 255) == 0);
    for (int i = 0; i < plan.n; ++i) {
        const GemmStep& st = plan.step[i];
        const int rc = launch_step<F16>(st.kernel, rows_of(a, epilogue, st.m0, st.rows), epilogue, tile_cfg, (hipStream_t)stream, ws);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int uv_gemm_bf16_nt(const void* A, long lda, const void* W, long ldw, const void* bias_bf16,
                               int M, int N, int K, int epilogue, void* out, long ldo,
                               const float* gate, const int32_t* gate_tid, long gate_stride,
                               int tile_cfg, void* stream) {
    return gemm_entry<false>(A, lda, W, ldw, bias_bf16, M, N, K, epilogue, out, ldo, gate, gate_tid, gate_stride, tile_cfg, stream);
}

// uv_gemm_bf16_nt with a caller-owned WORKSPACE (see include/univid_hip.h): lets the leftover-row strip of a long-K projection run as one
// round of split-K workgroups. Without a (large enough) workspace it IS uv_gemm_bf16_nt.
extern "C" int uv_gemm_bf16_nt_ws(const void* A, long lda, const void* W, long ldw, const void* bias_bf16,
                                  int M, int N, int K, int epilogue, void* out, long ldo,
                                  const float* gate, const int32_t* gate_tid, long gate_stride,
                                  int tile_cfg, void* workspace, long workspace_bytes, void* stream) {
    UV_CHECK_ARG(workspace_bytes >= 0 && (workspace || workspace_bytes == 0), "uv_gemm_bf16_nt_ws: bad workspace");
    GemmWs ws;
    ws.p = workspace; ws.bytes = workspace_bytes;
    return gemm_entry<false>(A, lda, W, ldw, bias_bf16, M, N, K, epilogue, out, ldo, gate, gate_tid, gate_stride, tile_cfg, stream, nullptr, 0, ws);
}

// Bytes of workspace with which uv_gemm_bf16_nt_ws(M, N, K, tile_cfg 0) takes its split-K strip (0: this shape has none): what the
// plan's strip needs, given any workspace. The epilogue and ldo are not known here: assumed are one of the epilogues the strip is built
// for and an output whose rows are N elements (ldo % 8 == 0), as in every projection that passes a workspace.
extern "C" long uv_gemm_splitk_ws_bytes(int M, int N, int K) {
    const GemmPlan plan = plan_gemm(M, N, K, UV_EPI_RESID_F32, N, 0, false, uv_num_cus(), LONG_MAX, true);
    const GemmStep& strip = plan.step[plan.n - 1];
    return strip.kernel == GK_SPLITK4 ? splitk_ws_bytes(strip.rows, N, 4) : 0;
}

// The plan a uv_gemm_bf16_nt / _ws / _ssq (f16 != 0: uv_gemm_f16_nt) call of this shape runs on the current device (256 CUs without one):
// exactly what plan_gemm returns to gemm_entry. ws_bytes: the workspace the caller would pass (0: none); a non-zero size counts as
// 256-byte aligned. *steps = 1 or 2; step i: its kernel's name (kGemmKernelName) at kernels + i * len, and its rows m0[i] ..
// m0[i] + rows[i] - 1. The shape checks are gemm_entry's. Host only.
extern "C" int uv_gemm_plan(int M, int N, int K, int epilogue, long ldo, int tile_cfg, int f16, long ws_bytes, int* steps, char* kernels,
                            int len, int* m0, int* rows) {
    UV_CHECK_ARG(steps && kernels && len > 0 && m0 && rows, "uv_gemm_plan: null pointer");
    UV_CHECK_ARG(M > 0 && N > 0 && K > 0, "uv_gemm_plan: bad shape M=%d N=%d K=%d", M, N, K);
    UV_CHECK_ARG(K % UV_BK == 0, "uv_gemm_plan: K=%d must be a multiple of %d", K, UV_BK);
    UV_CHECK_ARG(N % 16 == 0, "uv_gemm_plan: N=%d must be a multiple of 16", N);
    UV_CHECK_ARG(ldo % 4 == 0, "uv_gemm_plan: ldo must be a multiple of 4 elements");
    UV_CHECK_ARG(epilogue >= UV_EPI_BF16 && epilogue <= UV_EPI_BF16_SSQ, "uv_gemm_plan: unknown epilogue %d", epilogue);
    if (epilogue == UV_EPI_BF16_SSQ)
        UV_CHECK_ARG(N % 32 == 0 && ldo % 8 == 0, "uv_gemm_plan: the sums of squares need N %% 32 == 0, ldo %% 8 == 0 (N=%d ldo=%ld)", N, ldo);
    UV_CHECK_ARG(!f16 || tile_cfg == 0, "uv_gemm_plan: only tile_cfg 0 (automatic) is built for fp16 operands");
    UV_CHECK_ARG(ws_bytes >= 0, "uv_gemm_plan: bad workspace");
    const GemmPlan plan = plan_gemm(M, N, K, epilogue, ldo, tile_cfg, f16 != 0, uv_num_cus(), ws_bytes, true);
    *steps = plan.n;
    for (int i = 0; i < plan.n; ++i) {
        const GemmStep& st = plan.step[i];
        if (st.kernel == GK_DIAG) snprintf(kernels + (long)i * len, len, "%s%d", kGemmKernelName[st.kernel], tile_cfg);
        else snprintf(kernels + (long)i * len, len, "%s", kGemmKernelName[st.kernel]);
        m0[i] = st.m0; rows[i] = st.rows;
    }
    return 0;
}

// UV_EPI_BF16 plus the output's sums of squares per aligned 32-column group (see include/univid_hip.h): the q projection whose RMSNorm is applied
// by the attention kernel's prologue (uv_flash_attn_bf16_qnorm) instead of a pass of its own over q.
extern "C" int uv_gemm_bf16_nt_ssq(const void* A, long lda, const void* W, long ldw, const void* bias_bf16, int M, int N, int K,
                                   void* out, long ldo, float* ssq, long ld_ssq, int tile_cfg, void* stream) {
    return gemm_entry<false>(A, lda, W, ldw, bias_bf16, M, N, K, UV_EPI_BF16_SSQ, out, ldo, nullptr, nullptr, 0, tile_cfg, stream, ssq, ld_ssq);
}

// The same GEMM with IEEE fp16 operands / bias / 16-bit outputs (fp32 accumulate): the SigLIP2 ranker's reference dtype
// (models/BAGEL/eval_understanding.py:172). Only the automatic tile choice (tile_cfg 0) is built for fp16.
extern "C" int uv_gemm_f16_nt(const void* A, long lda, const void* W, long ldw, const void* bias_f16,
                              int M, int N, int K, int epilogue, void* out, long ldo,
                              const float* gate, const int32_t* gate_tid, long gate_stride,
                              int tile_cfg, void* stream) {
    UV_CHECK_ARG(tile_cfg == 0, "uv_gemm_f16_nt: only tile_cfg 0 (automatic) is built for fp16 operands");
    return gemm_entry<true>(A, lda, W, ldw, bias_f16, M, N, K, epilogue, out, ldo, gate, gate_tid, gate_stride, tile_cfg, stream);
}
