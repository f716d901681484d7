// The flash-attention kernels' shared host and device pieces (attention.hip; attention_win.hip; attention_bs.hip; attention_mx.hip; attention_mxpv.hip;
// tools/diag/attn_pw4.hip): the argument block and constants, plan_attn - the ONE place that decides which kernel serves a call, on what
// query-block cut and on what grid -, and the device code the kernels have in common: the per-wave QK^T / softmax / P.V of a 32-key half, the
// ragged-tile mask, the staging of the 64 KiB layout and the O stores are defined here.
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

// The argument checks the self-attention entries (uv_flash_attn_win_bf16, uv_flash_attn_bs_bf16 / _lists_bf16) have in common, in two parts:
// each entry's own check (the window's sides; mask_heads) stands between them, where it always stood - the order of the refusals is part of
// the entries' behaviour.
static inline int attn_self_check_shape(const char* name, const void* q, const void* k, const void* vt, const void* out, int batch, int L, int H,
                                        int head_dim) {
    UV_CHECK_ARG(q && k && vt && out, "%s: null pointer", name);
    UV_CHECK_ARG(head_dim == 128, "%s: head_dim %d unsupported (128 only)", name, head_dim);
    UV_CHECK_ARG(L > 0 && L <= (1 << 30) && H > 0 && batch > 0, "%s: bad shape B=%d L=%d H=%d", name, batch, L, H);
    return 0;
}

static inline int attn_self_check_layout(const char* name, const void* q, const void* k, const void* vt, const void* out, long ldq, long ldk,
                                         long ldvt, long ldo, int batch, int L) {
    UV_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldo % 4 == 0, "%s: leading dimensions must be multiples of 8 elements", name);
    UV_CHECK_ARG(ldvt >= (long)(batch - 1) * L + (long)((L + 63) / 64) * 64,
                 "%s: ldvt=%ld must cover (batch-1)*L + L rounded up to 64 (batch=%d L=%d)", name, ldvt, batch, L);
    UV_CHECK_ARG(batch == 1 || L % 8 == 0, "%s: batch > 1 needs L %% 8 == 0 (L=%d)", name, L);
    // the LDS-DMA pieces are addressed with 32-bit lane offsets from a uniform base (the dense entry falls back to flash_attn_fwd_kernel there)
    UV_CHECK_ARG(128 * ldvt < (1L << 30) && 64 * ldk < (1L << 30), "%s: ldk=%ld / ldvt=%ld too large for 32-bit piece offsets", name, ldk, ldvt);
    UV_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)out) & 15) == 0, "%s: pointers must be 16-byte aligned", name);
    return 0;
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

// The lane id, produced HERE (two VALU instructions, volatile: not hoisted): the rare branches and the epilogues derive their lane constants from it
// instead of keeping them - or the lane id itself - in registers across the tile loops, where they were spilled.
__device__ __forceinline__ int attn_lane_here() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// The windowed and block-sparse kernels' "unset" reference maximum and masked score. A lane's query can have no visible key in a 32-key half
// while its maximum is still unset; the dense kernels' -INFINITY would compute -inf - -inf there. With this FINITE sentinel and P of a masked
// element SELECTED to 0 (attn_softmax_half<true>) such a lane gets mt = unset, grow = 0 (no move of its own), alpha = exp2(0) = 1 exactly if a
// neighbour moves, P = 0, l += 0; at its first visible key alpha = exp2(-1e30 scale) = 0 on l = 0, O = 0 - what the dense kernels compute from -inf.
#define UV_WIN_UNSET (-1.0e30f)

// ---- one 32-key half of a staged tile, per wave (fwd3 / fwd12 / bs; the softmax also win and mxqk): S^T = K.Q^T, online softmax, O^T += V^T.P^T.
// A kernel that measured worse with one of these keeps its own copy and says so at the copy (win_body: QK^T and P.V; mxpv_body: mask and O store).
typedef const __attribute__((address_space(3))) bf16x8* lds_frag_p;

// The 8 fragment reads of a half go UV_ATT_AHEAD ahead of the 8 MFMAs that consume them (ID = the sync id of the group).
template <int ID>
__device__ __forceinline__ void attn_reads_ahead() {
    __builtin_amdgcn_sched_group_barrier(0x100, UV_ATT_AHEAD, ID);
#pragma unroll
    for (int i = 0; i < 8 - UV_ATT_AHEAD; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, ID);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, ID);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, UV_ATT_AHEAD, ID);
    __builtin_amdgcn_sched_barrier(0);
}

// S^T of a half: off = buffer parity * K bytes + T * 32 K rows (an instruction immediate when the parity is a compile-time constant).
__device__ __forceinline__ f32x16 attn_qk_half(const unsigned (&kaddr)[8], const bf16x8 (&qf)[8], int off) {
    f32x16 sacc;
#pragma unroll
    for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
        const bf16x8 kf = *(lds_frag_p)(kaddr[kk] + off);
        sacc = mfma_32x32x16<false>(kf, qf[kk], sacc);
    }
    attn_reads_ahead<0>();
    return sacc;
}

// The ragged last tile of the dense kernels: accumulator register e of half T holds key kv0 + perm23(32 T + (e & 3) + 8 (e >> 2) + 4 h).
__device__ __forceinline__ void attn_mask_ragged(f32x16& sacc, int kv0, int T, int h, int Lk) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int i = 32 * T + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (kv0 + perm23(i) >= Lk) sacc[e] = -INFINITY;
    }
}

// Online softmax of a half (query on the lane; masked scores already replaced by the caller: -INFINITY dense, UV_WIN_UNSET win / bs). The row
// maximum meets the other half-wave's by v_permlane32_swap (one VALU op, no ds_bpermute round trip). The reference maximum m_run moves only when
// some row's maximum outgrows it by more than 2^UV_ATT_DEFER in the exponent domain (then P <= 2^UV_ATT_DEFER instead of <= 1 until the next move;
// P, l and O share one scale and bf16 / f32 relative precision is scale-invariant): with the exact running maximum about half of all tiles of a
// long sequence still see a new maximum in SOME row of the wave and pay the O rescale. SELECT: P of an element whose vis bit is clear is
// selected to 0, not computed (else vis is ignored). pf = P in bf16, the B operand of attn_pv_half.
template <bool SELECT>
__device__ __forceinline__ void attn_softmax_half(const f32x16& sacc, unsigned vis, float scale_log2, float& m_run, float& l_run,
                                                  f32x16 (&oacc)[4], bf16x8 (&pf)[2]) {
    float mt = sacc[0];
#pragma unroll
    for (int e = 1; e < 16; ++e) mt = fmaxf(mt, sacc[e]);
    {
        const unsigned u = __builtin_bit_cast(unsigned, mt);
        const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
        mt = fmaxf(__builtin_bit_cast(float, (unsigned)sw[0]), __builtin_bit_cast(float, (unsigned)sw[1]));
    }
    const float grow = (mt - m_run) * scale_log2;      // +inf on the first tile (m_run = -inf); win / bs: 0 while both are unset
    if (__any(grow > UV_ATT_DEFER)) {
        const float m_new = fmaxf(m_run, mt);
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * scale_log2);
        l_run *= alpha;
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int e = 0; e < 16; ++e) oacc[d][e] *= alpha;
        m_run = m_new;
    }
    const float mneg = -m_run * scale_log2;
    float psum = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[8 * s2 + j], scale_log2, mneg));
            if constexpr (SELECT) pv = ((vis >> (8 * s2 + j)) & 1u) ? pv : 0.f;
            psum += pv;
            pf[s2][j] = (__bf16)pv;
        }
    l_run += psum;
}

// O^T += V^T . P^T of a half: vaddr = the half's two fragment addresses, off = buffer parity * V^T bytes (0 with a single V^T buffer).
__device__ __forceinline__ void attn_pv_half(const unsigned (&vaddr)[2], int off, const bf16x8 (&pf)[2], f32x16 (&oacc)[4]) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const bf16x8 vf = *(lds_frag_p)(vaddr[s2] + off + d * 32 * 128);
            oacc[d] = mfma_32x32x16<false>(vf, pf[s2], oacc[d]);
        }
    attn_reads_ahead<1>();
}

// ---- staging of the 64 KiB layout (K and V^T both double-buffered; fwd12 / win / bs): the 32 one-KiB pieces of a tile (K pieces 0..15 = 4 LDS
// rows each, V^T pieces 0..15 = 8 rows each) are dealt round-robin over the NW waves. K pieces of equal pc & 3 share the swizzle key and the row
// permutation bits, V^T pieces of equal parity the swizzle key: at 12 waves (K w, w + 12 (w < 4); V^T w - 4 (w >= 4), w + 8 (w < 8)) and at 4
// (K and V^T w, w + 4, w + 8, w + 12) ONE lane offset per operand serves all of a wave's pieces; the piece's row / column step goes into the
// uniform base. kb_t / vb_t = the tile's first key row of the head / first key column (the kernels keep their own base pointers).
template <int NW>
struct AttnStage {
    static_assert(NW == 12 || NW == 4, "two forms");
    static constexpr int K_BYTES = UV_ATT_KV * 256, V_BYTES = 128 * 128, V_OFF = 2 * K_BYTES;
    unsigned koff, voff;      // lane offsets in bytes, relative to the tile's first key row / key column
    long k16, v8;             // 16 K rows / 8 V^T rows in bytes
    unsigned smem_a;          // LDS byte address of K buffer 0
    int wave;
    int ldk;                  // K's leading dimension in elements: clamped() builds its row offsets from it

    __device__ __forceinline__ AttnStage(unsigned smem_a_, int wave_u, int lane, long ldk_, long ldvt) : k16(16 * ldk_ * 2), v8(8 * ldvt * 2),
                                                                                                       smem_a(smem_a_), wave(wave_u), ldk((int)ldk_) {
        const int s4 = lane >> 4, s8 = lane >> 3, p3 = wave_u & 3;
        const int c = (lane & 15) ^ ((4 * p3 + s4) & 15);
        const int swap2 = ((p3 & 1) << 1) | (p3 >> 1);
        koff = (unsigned)((s4 + 4 * swap2) * (int)ldk_ + c * 8) * 2u;
        const int cv = (lane & 7) ^ ((4 * (wave_u & 1) + (s8 >> 1)) & 7);
        voff = (unsigned)(s8 * (int)ldvt + cv * 8) * 2u;
    }
    __device__ __forceinline__ void v(const char* vb_t, int buf) const {
        if constexpr (NW == 12) {
            const int vq0 = wave - 4, vq1 = wave + 8;
            if (wave >= 4) glds16_sbase(vb_t + vq0 * v8, voff, smem_a + V_OFF + buf * V_BYTES + vq0 * 1024);
            if (wave < 8) glds16_sbase(vb_t + vq1 * v8, voff, smem_a + V_OFF + buf * V_BYTES + vq1 * 1024);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) glds16_sbase(vb_t + (wave + 4 * i) * v8, voff, smem_a + V_OFF + buf * V_BYTES + (wave + 4 * i) * 1024);
        }
    }
    __device__ __forceinline__ void full(const char* kb_t, const char* vb_t, int buf) const {
        if constexpr (NW == 12) {
            glds16_sbase(kb_t + (wave >> 2) * k16, koff, smem_a + buf * K_BYTES + wave * 1024);
            if (wave < 4) glds16_sbase(kb_t + 3 * k16, koff, smem_a + buf * K_BYTES + (wave + 12) * 1024);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) glds16_sbase(kb_t + i * k16, koff, smem_a + buf * K_BYTES + (wave + 4 * i) * 1024);
        }
        v(vb_t, buf);
    }
    // the ragged last tile: K rows clamped to last_row (the last key's row inside the tile) in the lane offset; the row inside the tile is
    // 16 (pc >> 2) + the lane's row of its 16. Rare: its lane constants come from attn_lane_here(), not from registers kept across the tile loops.
    __device__ __forceinline__ void clamped(const char* kb_t, const char* vb_t, int last_row, int buf) const {
        const int p3 = wave & 3;
        const int ln = attn_lane_here();
        const int r4 = ln >> 4;
        const int krl = r4 + 4 * (((p3 & 1) << 1) | (p3 >> 1));
        const unsigned c16 = (unsigned)(((ln & 15) ^ ((4 * p3 + r4) & 15)) << 4);
#pragma unroll
        for (int i = 0; i < (NW == 12 ? 2 : 4); ++i) {
            const int pc = wave + NW * i;
            if (pc < 16) glds16_sbase(kb_t, (unsigned)(min(16 * (pc >> 2) + krl, last_row) * ldk) * 2u + c16, smem_a + buf * K_BYTES + pc * 1024);
        }
        v(vb_t, buf);
    }
};

// O rows of one wave through a wave-private LDS image: 32 rows x (128 + 16) bytes at img, two passes of two d-blocks; every store instruction
// writes 8 whole 128-byte lines (directly from the MFMA layout it touches 32 rows with 16 bytes each; self-attention at the DiT shape 2.724 ->
// 2.711 ms in a same-device A/B, bit-identical). ldo % 8 == 0. The caller owns the LDS (every reader of what it held has passed a barrier).
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
