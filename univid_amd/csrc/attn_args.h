// The flash-attention kernels' shared host and device pieces (attention.hip; attention_mx.hip; attention_mxpv.hip; tools/diag/attn_pw4.hip): the argument block and constants,
// plan_attn - the ONE place that decides which kernel serves a call, on what query-block cut and on what grid -, and the device code the
// kernels have in common.
#pragma once
#include "common.h"

#define UV_ATT_QW 32     // queries per 32x32 MFMA block
#define UV_ATT_KV 64     // keys per staged tile
#define UV_ATT_DEFER 8.0f   // log2 of the largest P allowed before the reference maximum is moved
// attention_mxpv.hip (P as e4m3 codes; include/univid_hip.h: UV_ATT_MXPV_DEFER / UV_ATT_MXPV_PSHIFT): code = e4m3(P 2^PSHIFT), P <= 2^DEFER_PV,
// DEFER_PV + PSHIFT = 8: the largest code is 256
#define UV_ATT_DEFER_PV 1
#define UV_ATT_PSHIFT 7

struct AttnArgs {
    const bf16_t* q;   // [Lq, ldq]   head h at column h*128
    const bf16_t* k;   // [Lk, ldk]
    const bf16_t* vt;  // [H*128, ldvt]  (V transposed; ldvt >= roundup(Lk, 64), pad finite)
    bf16_t* out;       // [Lq, ldo]
    long ldq, ldk, ldvt, ldo;
    int Lq, Lk, H, q_blocks, batch;
    int n12;           // flash_attn_fwd12_kernel: query blocks per head that own 12 units; the other q_blocks - n12 own 8
    float scale_log2;  // softmax_scale * log2(e)
    // uv_flash_attn_bf16_qnorm: q holds the RAW projection; the kernels' Q prologue applies WanRMSNorm to it (model.py:82-85, 138 / 169):
    // q_rs [batch * Lq] f32 = 1 / sqrt(mean(q_row^2) + eps) over ALL heads' columns (uv_rms_scale_from_ssq), q_w [H * 128] f32 = norm_q.weight
    const float* q_rs;
    const float* q_w;
};

// attention_win.hip: AttnArgs (Lq == Lk, q_rs / q_w unused) plus the window, every bound already resolved: 0 <= left, right <= L
struct AttnWinArgs : AttnArgs {
    int left, right;
};

// attention_bs.hip: AttnArgs (Lq == Lk, q_rs / q_w unused) plus the key-tile schedule of a block mask: per (mask head, 128-query block) the
// ascending list of visible 64-key tiles and its length. mask_heads = 1 (one mask for all heads) or H; mask_samples = 1 (the samples of a
// stacked launch share the lists: uv_flash_attn_bs_bf16) or batch (one set of lists per sample: uv_flash_attn_bs_lists_bf16).
struct AttnBsArgs : AttnArgs {
    const int* tile_idx;   // [mask_samples, mask_heads, q_blocks, nkb]  the first tile_cnt entries of a row are read, nothing else
    const int* tile_cnt;   // [mask_samples, mask_heads, q_blocks]
    int mask_heads, nkb;   // nkb = ceil(L / 64)
    int mask_samples;
};

enum AttnKernel { ATT_FWD12 = 0, ATT_FWD3 = 1, ATT_FWD_D128 = 2, ATT_FWD_D64 = 3, ATT_MXQK12 = 4, ATT_MXQK4 = 5, ATT_MXPV12 = 6, ATT_MXPV4 = 7,
                  ATT_WIN12 = 8, ATT_WIN4 = 9, ATT_BS4 = 10 };
static const char* const kAttnKernelName[] = {"flash_attn_fwd12_kernel", "flash_attn_fwd3_kernel", "flash_attn_fwd_kernel<128>",
                                              "flash_attn_fwd_kernel<64>", "flash_attn_mxqk12_kernel", "flash_attn_mxqk4_kernel",
                                              "flash_attn_mxpv12_kernel", "flash_attn_mxpv4_kernel",
                                              "flash_attn_win12_kernel", "flash_attn_win4_kernel", "flash_attn_bs4_kernel"};
struct AttnPlan {
    int kernel;            // AttnKernel
    int q_blocks, n12;     // query blocks per (sample, head); of them the 12-unit ones (flash_attn_fwd12_kernel only, else 0)
    int grid, block;       // workgroups = q_blocks * H * batch; threads per workgroup
};

// Which kernel serves this attention call, how each (sample, head) is cut into query blocks, and on what grid. ncus = the device's CU
// count, force_cut = UV_OPT_ATTN_CUT (A/B tools and tests; 0 = automatic): the callers read both and pass them in. Pure: the same answer
// for the same arguments, whatever ran before (the memo below only saves the scan).
static inline AttnPlan plan_attn(int batch, int Lq, int Lk, int H, int head_dim, long ldk, long ldvt, bool f16, int ncus, int force_cut) {
    const int nbh = H * batch;
    auto blocks128 = [&](int kernel) {       // the 4-wave kernels: 128 queries per workgroup
        const int qb = (Lq + 4 * UV_ATT_QW - 1) / (4 * UV_ATT_QW);
        return AttnPlan{kernel, qb, 0, qb * nbh, 256};
    };
    if (head_dim != 128) return blocks128(ATT_FWD_D64);
    // fwd12 / fwd3 address their LDS-DMA pieces with 32-bit lane offsets from a uniform base
    if (f16 || 128 * ldvt >= (1L << 30) || 64 * ldk >= (1L << 30)) return blocks128(ATT_FWD_D128);
    // long key sequences: one 12-wave workgroup per CU shares each K / V^T tile among up to 384 queries (a third of the L2 -> LDS
    // traffic; -2.8 % on the self-attention launches); short ones (cross-attention, Lk = 512: prologue and last round weigh
    // more) keep the 4-wave workgroups (the 12-wave form is 24 % slower there)
    if (Lk < 2048) return blocks128(ATT_FWD3);

    // flash_attn_fwd12_kernel: the cut of a (sample, head)'s NWU = ceil(Lq / 32) query units into n12 blocks of 12 units followed by n8
    // blocks of 8 units. Model: a 12-unit workgroup takes time 1, an 8-unit one T8 = 0.76 (measured), every XCD's CUs pick their
    // workgroups up in id order (12-unit blocks first = longest-first list scheduling); the cut with the smallest simulated makespan
    // wins, ties go to fewer workgroups. Measured at the DiT shape (batch 2, 48 heads x 358 units): 26 + 6 blocks 2.86 ms against
    // 2.90 ms for 30 + 0; mixes with more 8-unit blocks lose (24 + 9: 3.03 ms). At batch 1 the model picks 30 + 0 (720 workgroups on
    // 256 CUs: three rounds, the last one 81 % full).
    const int nwu = (Lq + UV_ATT_QW - 1) / UV_ATT_QW;
    auto cut = [&](int n12, int n8) { return AttnPlan{ATT_FWD12, n12 + n8, n12, (n12 + n8) * nbh, 768}; };
    auto n12_beside = [&](int n8) { return nwu > 8 * n8 ? (nwu - 8 * n8 + 11) / 12 : 0; };
    if (force_cut > 0) return cut(n12_beside(force_cut - 1), force_cut - 1);      // n8 = force_cut - 1 eight-unit blocks per head
    // small per-thread memo (ctypes releases the GIL: two host threads, one per GPU, may be in here with different shapes at once;
    // alternating shapes must not re-run the list-scheduling scan, ~ blocks x CUs x cuts host operations, on every call)
    struct Memo { int nwu, nbh, ncus, n12, n8; };
    static thread_local Memo memo[8];
    static thread_local int memo_next = 0;
    for (const Memo& e : memo)
        if (e.nwu == nwu && e.nbh == nbh && e.ncus == ncus) return cut(e.n12, e.n8);
    const double T8 = 0.76;   // measured: all-8-unit cut 0.365 ms per round of workgroups, all-12-unit cut 0.48 ms (batch 2, L = 11 440)
    int best12 = (nwu + 11) / 12, best8 = 0;
    double best = 1e30;
    for (int n8 = 0; n8 * 8 < nwu + 8; ++n8) {
        const int n12 = n12_beside(n8);
        if (n12 == 0 && n8 * 8 - nwu >= 8) break;
        // list scheduling on ncus identical machines: loads kept in a small array (ncus <= 1024)
        double load[1024];
        const int m = ncus < 1024 ? ncus : 1024;
        for (int i = 0; i < m; ++i) load[i] = 0.0;
        auto place = [&](long count, double t) {
            for (long j = 0; j < count; ++j) {
                int arg = 0;
                for (int i = 1; i < m; ++i) if (load[i] < load[arg]) arg = i;
                load[arg] += t;
            }
        };
        place((long)n12 * nbh, 1.0);
        place((long)n8 * nbh, T8);
        double mk = 0.0;
        for (int i = 0; i < m; ++i) mk = load[i] > mk ? load[i] : mk;
        if (mk < best - 1e-9) { best = mk; best12 = n12; best8 = n8; }
    }
    memo[memo_next] = Memo{nwu, nbh, ncus, best12, best8};
    memo_next = (memo_next + 1) & 7;
    return cut(best12, best8);
}

// The MXFP8-q/k kernels (attention_mx.hip; head_dim 128, 64-bit piece addresses: no leading-dimension limit): plan_attn's decision for the bf16
// problem of the same shape - the same Lk threshold, query-block cut and grid - with the kernel of the same size. plan_attn stays the one place
// that chooses.
static inline AttnPlan plan_attn_mxqk(int batch, int Lq, int Lk, int H, int ncus, int force_cut) {
    AttnPlan plan = plan_attn(batch, Lq, Lk, H, 128, 8, 8, false, ncus, force_cut);
    plan.kernel = plan.kernel == ATT_FWD12 ? ATT_MXQK12 : ATT_MXQK4;
    return plan;
}

// The MXFP8 q/k + P.V kernels (attention_mxpv.hip): the same decision once more, with the kernel of the same size.
static inline AttnPlan plan_attn_mxpv(int batch, int Lq, int Lk, int H, int ncus, int force_cut) {
    AttnPlan plan = plan_attn(batch, Lq, Lk, H, 128, 8, 8, false, ncus, force_cut);
    plan.kernel = plan.kernel == ATT_FWD12 ? ATT_MXPV12 : ATT_MXPV4;
    return plan;
}

// The sliding-window / causal kernels (attention_win.hip; self-attention, Lq == Lk == L, head_dim 128, bf16): query i attends keys
// max(0, i - left) .. min(L - 1, i + right), -1 = unbounded on that side. plan_attn's decision for the dense problem whose key count is the
// span of keys ONE workgroup streams, min(L, 384 + left + right) with an unbounded side counted as L: the dense plan's Lk >= 2048 threshold
// applied to what a 12-wave workgroup of 384 queries actually stages (carried over from the dense plan; profiles/attn_window_bench.md
// holds what was measured around it). The cut and the grid are the dense plan's for (batch, L, H). Workgroups of a causal or one-sided
// launch stream unequal key counts; the makespan model assumes equal ones (known, unmeasured).
static inline AttnPlan plan_attn_win(int batch, int L, int H, int left, int right, int ncus, int force_cut, int force_form = 0) {
    long span = 384L + (left < 0 ? L : left) + (right < 0 ? L : right);
    if (span > L) span = L;
    if (force_form) span = force_form == 1 ? 2048 : 1;       // UV_OPT_ATTN_WIN_FORM (A/B tools): the form whatever the span; a query's bits do not depend on it
    AttnPlan plan = plan_attn(batch, L, (int)span, H, 128, 8, 8, false, ncus, force_cut);
    plan.kernel = plan.kernel == ATT_FWD12 ? ATT_WIN12 : ATT_WIN4;
    return plan;
}

// The block-sparse kernel (attention_bs.hip; self-attention, Lq == Lk == L, head_dim 128, bf16): one 4-wave workgroup per (sample, head,
// 128-query block), whatever the mask holds - the key count a workgroup streams is its list's, not the problem's. Grid ids map to blocks in
// flash_attn_fwd3_kernel's XCD-contiguous order.
static inline AttnPlan plan_attn_bs(int batch, int L, int H) {
    const int qb = (L + 4 * UV_ATT_QW - 1) / (4 * UV_ATT_QW);
    return AttnPlan{ATT_BS4, qb, 0, qb * H * batch, 256};
}

// ---- device code the kernels share
typedef __attribute__((address_space(3))) void lds_void_a;

// One LDS-DMA piece with a UNIFORM base pointer (SGPR pair) and a 32-bit lane offset: "global_load_lds_dwordx4 voff, s[base]".
// hipcc selects only the 64-bit-VGPR-address form for the builtin (one v_lshl_add_u64 and a live register pair per piece).
// M0 = wave-uniform LDS byte address of the piece; saved and restored around the statement (the compiler owns M0).
__device__ __forceinline__ void glds16_sbase(const char* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_dst)
                 : "memory");
}

constexpr int UV_ATT_AHEAD = 3;      // fwd3 / fwd12: fragment reads in flight ahead of their MFMA (2 .. 5 measured: all within 0.5 %)

// Independent samples are stacked along the token axis: rows of q / k / out, COLUMNS of V^T. Moves the argument block to sample b.
template <int QN>
__device__ __forceinline__ void attn_sample_offset(AttnArgs& p, long b) {
    p.q += b * p.Lq * p.ldq;
    if (QN) p.q_rs += b * p.Lq;
    p.k += b * p.Lk * p.ldk;
    p.vt += (long)b * p.Lk;
    p.out += b * p.Lq * p.ldo;
}

// O row of one query straight from the MFMA layout: op = the row's first element of this lane (column hcol + 4 h), 4 ND pieces of 8 bytes.
// Any ldo % 4 == 0.
template <bool F16, int ND>
__device__ __forceinline__ void attn_store_direct(bf16_t* op, const f32x16 (&oacc)[ND], float inv) {
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            u32x2 o = {pack16_2<F16>(oacc[d][4 * g + 0] * inv, oacc[d][4 * g + 1] * inv),
                       pack16_2<F16>(oacc[d][4 * g + 2] * inv, oacc[d][4 * g + 3] * inv)};
            *(u32x2*)(op + 32 * d + 8 * g) = o;
        }
}

// Q fragments of one wave: lane (r, h) holds Q[qrow][hcol + 16 kk + 8 h .. + 7], kk = 0 .. NKK-1. QN = 1: q is the RAW projection and the row's
// RMSNorm is applied by attn_apply_qnorm with the rounding points of rmsnorm_rope_kernel (dit_glue.hip): bf16( bf16(q * rs) * w ), products in
// f32 - bit for bit what that kernel writes for the same rs. Two steps on purpose: the loads (q, the row scale, the lane's 8 NKK weights) are
// ISSUED with the Q loads at the top of the kernel, the arithmetic runs behind the first K / V tile's LDS-DMA issue - applied right at the load it
// made the prologue wait for the Q data before staging anything (measured: + 3 us per cross-attention workgroup).
template <int NKK, int QN>
struct AttnQNorm {
    float rs;
    f32x4 w[QN ? 2 * NKK : 1];
};

template <int NKK, int QN>
__device__ __forceinline__ void attn_load_q(const AttnArgs& p, bf16x8 (&qf)[NKK], AttnQNorm<NKK, QN>& qn, int qrow, long hcol, int h) {
    const bf16_t* qp = p.q + (long)qrow * p.ldq + hcol + 8 * h;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) qf[kk] = *(const bf16x8*)(qp + 16 * kk);
    if constexpr (QN >= 1) {
        qn.rs = p.q_rs[qrow];
        const float* wp = p.q_w + hcol + 8 * h;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            qn.w[2 * kk] = *(const f32x4*)(wp + 16 * kk);
            qn.w[2 * kk + 1] = *(const f32x4*)(wp + 16 * kk + 4);
        }
    }
}

template <int NKK, int QN>
__device__ __forceinline__ void attn_apply_qnorm(bf16x8 (&qf)[NKK], const AttnQNorm<NKK, QN>& qn) {
    if constexpr (QN >= 1) {
        __builtin_amdgcn_sched_barrier(0);       // (not hoisted above the staging that precedes the call)
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            const u32x4 raw = __builtin_bit_cast(u32x4, qf[kk]);
            u32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float lo = bf2f((bf16_t)(raw[e] & 0xffff)), hi = bf2f((bf16_t)(raw[e] >> 16));
                const f32x4& wv = qn.w[2 * kk + (e >> 1)];
                o[e] = pack_bf2(__fmul_rn(round_bf(__fmul_rn(lo, qn.rs)), wv[(2 * e) & 3]), __fmul_rn(round_bf(__fmul_rn(hi, qn.rs)), wv[(2 * e + 1) & 3]));
            }
            qf[kk] = __builtin_bit_cast(bf16x8, o);
        }
    }
}

__device__ __forceinline__ int perm23(int i) {  // swap bits 2 and 3
    return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1);
}

// Fragment read addresses of flash_attn_fwd3_kernel / flash_attn_fwd12_kernel (LDS byte addresses; buffer, key-half and d-tile offsets are
// instruction immediates). K: row r of 256 bytes, logical chunk 2 kk + h, physical chunk ^= r & 15. V^T (at v_off): row r of 128 bytes, logical
// chunk 4 T + 2 s + h, physical chunk ^= (r >> 1) & 7.
__device__ __forceinline__ void attn_frag_addrs(unsigned smem_a, unsigned v_off, int r, int h, unsigned (&kaddr)[8], unsigned (&vaddr)[2][2]) {
    const int k_key = r & 15, v_key = (r >> 1) & 7;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) kaddr[kk] = smem_a + r * 256 + (((2 * kk + h) ^ k_key) << 4);
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) vaddr[T][s2] = smem_a + v_off + r * 128 + (((4 * T + 2 * s2 + h) ^ v_key) << 4);
}

// O rows of one wave through a wave-private LDS image (flash_attn_fwd12_kernel's epilogue, for kernels written after it): 32 rows x (128 + 16)
// bytes at img, two passes of two d-blocks; every store instruction writes 8 whole 128-byte lines. ldo % 8 == 0. The caller owns the LDS
// (every reader of what it held has passed a barrier).
__device__ __forceinline__ void attn_store_lds(char* img, bf16_t* out0, long ldo, int rows, int lane, const f32x16 (&oacc)[4], float inv) {
    constexpr int RS = 144;
    const int r = lane & 31, h = lane >> 5, srow = lane >> 3, chunk = lane & 7;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int dd = 0; dd < 2; ++dd)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = 2 * half + dd;
                u32x2 o = {pack16_2<false>(oacc[d][4 * g + 0] * inv, oacc[d][4 * g + 1] * inv),
                           pack16_2<false>(oacc[d][4 * g + 2] * inv, oacc[d][4 * g + 3] * inv)};
                *(u32x2*)(img + r * RS + 64 * dd + 16 * g + 8 * h) = o;
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // wave-private image: no barrier
        u32x4 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = *(const u32x4*)(img + (8 * i + srow) * RS + chunk * 16);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the second pass overwrites the image
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = 8 * i + srow;
            if (row < rows) *(u32x4*)(out0 + (long)row * ldo + 64 * half + chunk * 8) = v[i];
        }
    }
}
