// Flash attention forward with a sliding window and / or a causal mask (head_dim 128, bf16 in / fp32 softmax + accumulate / bf16 out) for gfx950:
// the opt-in local self-attention of the DiT (WanModel.set_attn_window; Lq == Lk == L, every sample attends all L keys).
//
// Replaces: flash_attention(..., causal=, window_size=)  models/wan/utils/modules/attention.py:113-127 (flash_attn_varlen_func's window_size /
//           causal arguments) as called from WanSelfAttention.forward model.py:145-150.
//
// Query i of a sample attends key j iff max(0, i - left) <= j <= min(L - 1, i + right); the host resolves "unbounded" (-1) and causal to
// 0 <= left, right <= L before the launch. Exact: the same softmax over fewer keys - a workgroup does not STAGE key tiles outside the window of
// its queries and a wave does not COMPUTE tiles outside the window of its own 32.
//
// A workgroup owning queries [qa, qb] stages tiles t_lo = lo(qa) / 64 .. t_hi = hi(qb) / 64 and each of its waves classifies every one of them
// wave-uniformly for its queries [wa, wb]:
//   outside   t < lo(wa) / 64 or t > hi(wb) / 64: the wave takes its share of the staging and the barrier, nothing else
//   interior  lo(wb) <= 64 t and 64 t + 63 <= hi(wa): all 64 keys visible to all 32 queries (and below L): the unmasked body, no masking code
//   edge      everything else: per-element mask with the TRUE key index (kv0 + perm23(i) in the K.Q^T accumulator layout) against the lane's
//             query; lanes of padded query rows (q >= L) are duplicates of row L - 1, mask included
// EMPTY ROWS IN AN EDGE HALF: a lane's query can have no visible key in a 32-key half while its reference maximum is still unset (left = 100:
// the wave's last query sees nothing of the first tile its first query needs). The "unset" maximum and a masked score are therefore the FINITE
// sentinel UV_WIN_UNSET, and P of a masked element is SELECTED to 0 by its visibility bit (attn_args.h: UV_WIN_UNSET, attn_softmax_half<true>).
// The online softmax of a half is the dense kernels' own code (attn_args.h: attn_softmax_half; the staging and the O stores too) and the QK^T / P.V
// loops around it are attn_qk_half's / attn_pv_half's statements: a window that covers every key reproduces the dense launch bit for bit, and a
// query's bits depend on its 32-query unit only, never on the query-block cut, the form or the other queries of the launch.
//
// One body in two forms (plan_attn_win, attn_args.h, decides):
//   flash_attn_win12_kernel  a workgroup's key span >= 2048: flash_attn_fwd12_kernel's 12-wave workgroup - 12 / 8 unit query blocks, loader-only
//                            waves, XCD-aware id order, SGPR-base LDS-DMA pieces dealt round-robin, O through LDS
//   flash_attn_win4_kernel   shorter spans: 4 waves x 32 queries in flash_attn_fwd3_kernel's XCD-contiguous id order. It keeps the 12-wave form's
//                            staging (K and V^T both double-buffered, 64 KiB, one barrier per tile: two workgroups per CU where fwd3 has three
//                            on 48 KiB and two barriers) - one body, correct, not tuned
// Tile schedule of a computing wave: generic tiles (parity, class, "is the next tile full" at run time; ONE instantiation, in loops of its own - no
// if / else chain of instantiations for the register allocator to spill across, attention.hip "PAR = -1") up to the wave's first interior tile on
// an even buffer, then pairs of interior tiles with compile-time parity (the dense main loop), then generic tiles again.
#include "attn_args.h"
#include <stdio.h>
#include <type_traits>

template <int NW>
__device__ __forceinline__ void win_body(AttnWinArgs p, char* smem) {
    constexpr int D = 128, KROW = 256, NKK = 8, ND = 4;
    constexpr int K_BYTES = UV_ATT_KV * KROW, V_BYTES = D * 128;
    constexpr int V_OFF = 2 * K_BYTES;
    static_assert(NW == 12 || NW == 4, "two forms");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int r = lane & 31, h = lane >> 5;
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = p.Lq;
    const int nwu = (L + UV_ATT_QW - 1) / UV_ATT_QW;

    int bh, u0, units;
    if constexpr (NW == 12) {       // flash_attn_fwd12_kernel's order: 12-unit blocks first, XCD-contiguous id ranges when both totals divide by 8
        const int nbh = p.H * p.batch, n8 = p.q_blocks - p.n12;
        const int tot12 = p.n12 * nbh, tot8 = n8 * nbh;
        int id = blockIdx.x;
        if ((tot12 & 7) == 0 && (tot8 & 7) == 0) {
            const int x = blockIdx.x & 7, j = blockIdx.x >> 3, c12 = tot12 >> 3, c8 = tot8 >> 3;
            id = j < c12 ? x * c12 + j : tot12 + x * c8 + (j - c12);
        }
        if (id < tot12) {
            bh = id / p.n12;
            u0 = (id - bh * p.n12) * 12;
            units = 12;
        } else {
            const int v2 = id - tot12;
            bh = v2 / n8;
            u0 = p.n12 * 12 + (v2 - bh * n8) * 8;
            units = 8;
        }
    } else {                        // flash_attn_fwd3_kernel's order: XCD x works through a contiguous range of (sample, head, block) ids
        const int nb = gridDim.x, per = nb >> 3, rem = nb & 7;
        const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
        const int vb = x * per + min(x, rem) + j;
        bh = vb / p.q_blocks;
        u0 = (vb - bh * p.q_blocks) * 4;
        units = 4;
    }
    units = min(units, nwu - u0);                  // the head's last block may be ragged
    // A forced cut (UV_OPT_ATTN_CUT) can hand out blocks behind the head's last unit. They own no query and no window: with a bounded left
    // their first tile would lie behind the sample (t_lo > t_hi, a negative row clamp). Nothing to stage, nothing to store; the whole
    // workgroup leaves here, before its first fetch and before any barrier.
    if (units <= 0) return;
    const bool compute_wave = wave_u < units;      // the other waves are loader-only: their share of the staging and every barrier
    const int head = bh % p.H;
    attn_sample_offset<0>(p, bh / p.H);
    const int q0w = (u0 + wave_u) * UV_ATT_QW;
    const long hcol = (long)head * D;

    // ---- the window in tiles. Workgroup: the tiles it stages; wave: the tiles it computes and, of them, the interior run
    const int qa = u0 * UV_ATT_QW, qb = min(L, (u0 + units) * UV_ATT_QW) - 1;
    const int t_lo = max(0, qa - p.left) / UV_ATT_KV, t_hi = min(L - 1, qb + p.right) / UV_ATT_KV;
    const int wa = min(q0w, L - 1), wb = min(q0w + UV_ATT_QW - 1, L - 1);
    const int w_lo = max(0, wa - p.left) / UV_ATT_KV, w_hi = min(L - 1, wb + p.right) / UV_ATT_KV;
    const int i_lo = (max(0, wb - p.left) + UV_ATT_KV - 1) / UV_ATT_KV, i_hi = (min(L - 1, wa + p.right) + 1) / UV_ATT_KV - 1;   // may be empty
    // the lane's own bounds (a padded row is a duplicate of row L - 1)
    const int qm = min(q0w + r, L - 1);
    const int jlo = max(0, qm - p.left), jhi = min(L - 1, qm + p.right);

    bf16x8 qf[NKK];
    AttnQNorm<NKK, 0> qnorm;
    attn_load_q<NKK, 0>(p, qf, qnorm, qm, hcol, h);

    // ---- staging: AttnStage (attn_args.h) with this kernel's running base pointers; the ragged last tile clamps its K rows to L - 1
    const unsigned smem_a = (unsigned)(uintptr_t)(lds_void_a*)smem;
    AttnStage<NW> stage(smem_a, wave_u, lane, p.ldk, p.ldvt);
    const long kstep = (long)UV_ATT_KV * p.ldk * 2;
    const char* kbase = (const char*)(p.k + hcol) + t_lo * kstep;                          // tile t_lo; += kstep per tile
    const char* vbase = (const char*)(p.vt + hcol * p.ldvt) + (long)t_lo * 2 * UV_ATT_KV;  // += 128 B per tile

    unsigned kaddr[NKK];
    unsigned vaddr[2][2];
    attn_frag_addrs(smem_a, V_OFF, r, h, kaddr, vaddr);

    f32x16 oacc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;
    float m_run = UV_WIN_UNSET, l_run = 0.f;

    const int nt_full = L / UV_ATT_KV;
    if (t_lo < nt_full) stage.full(kbase, vbase, 0);
    else stage.clamped(kbase, vbase, L - 1 - t_lo * UV_ATT_KV, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) asm volatile("" : "+v"(qf[kk]), "+v"(kaddr[kk]));      // every prologue load has landed before the loops
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(vaddr[i >> 1][i & 1]));
    asm volatile("" : "+v"(stage.koff), "+v"(stage.voff));
    __syncthreads();

    if (!compute_wave) {
        for (int t = t_lo; t <= t_hi; ++t) {
            vbase += 2 * UV_ATT_KV;
            kbase += kstep;
            const int nbuf = ((t - t_lo) & 1) ^ 1;
            if (t < t_hi) {
                if (t + 1 < nt_full) stage.full(kbase, vbase, nbuf);
                else stage.clamped(kbase, vbase, L - 1 - (t + 1) * UV_ATT_KV, nbuf);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        return;
    }

    // One staged tile. par_tag >= 0: an INTERIOR tile of that buffer parity whose successor is interior (hence full) too - the dense kernels' main
    // loop, no masking code. par_tag = -1: the generic form - parity, outside / interior / edge and the next tile's kind decided at run time.
    auto tile = [&](int t, auto par_tag) {
        constexpr bool DYN = decltype(par_tag)::value < 0;
        const int PAR = DYN ? ((t - t_lo) & 1) : decltype(par_tag)::value;
        const int kv0 = t * UV_ATT_KV;
        vbase += 2 * UV_ATT_KV;
        kbase += kstep;
        if constexpr (!DYN) {
            stage.full(kbase, vbase, PAR ^ 1);
        } else if (t < t_hi) {
            if (t + 1 < nt_full) stage.full(kbase, vbase, PAR ^ 1);
            else stage.clamped(kbase, vbase, L - 1 - kv0 - UV_ATT_KV, PAR ^ 1);
        }
        const bool active = !DYN || (t >= w_lo && t <= w_hi);
        const bool edge = DYN && !(t >= i_lo && t <= i_hi);
        if (active) {
#pragma unroll
            for (int T = 0; T < 2; ++T) {
                // its own copies of attn_qk_half / attn_pv_half and their attn_reads_ahead ladders (attn_args.h), the same statements: through the
                // shared ones flash_attn_win12_kernel measured 0.6 - 0.9 % slower on whole sequences, outside the run-to-run spread
                // (profiles/attn_shared_pieces.md)
                f32x16 sacc;
#pragma unroll
                for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
#pragma unroll
                for (int kk = 0; kk < NKK; ++kk) {
                    const bf16x8 kf = *(lds_frag_p)(kaddr[kk] + PAR * K_BYTES + T * 32 * KROW);
                    sacc = mfma_32x32x16<false>(kf, qf[kk], sacc);
                }
                __builtin_amdgcn_sched_group_barrier(0x100, UV_ATT_AHEAD, 0);
#pragma unroll
                for (int i_ = 0; i_ < 8 - UV_ATT_AHEAD; ++i_) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, UV_ATT_AHEAD, 0);
                __builtin_amdgcn_sched_barrier(0);
                // visibility of the half's 16 accumulator rows for this lane's query: register e holds key kv0 + perm23(32 T + (e & 3) +
                // 8 (e >> 2) + 4 h) = kv0 + 32 T + 8 h + (e & 3) + 4 ((e >> 2) & 1) + 16 (e >> 3)
                unsigned vis = 0xffffu;
                if (DYN && edge) {
                    const int a = jlo - kv0 - 32 * T - 8 * h, b = jhi - kv0 - 32 * T - 8 * h;
                    vis = 0u;
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int c = (e & 3) + 4 * ((e >> 2) & 1) + 16 * (e >> 3);
                        const bool ok = c >= a && c <= b;
                        vis |= (ok ? 1u : 0u) << e;
                        sacc[e] = ok ? sacc[e] : UV_WIN_UNSET;
                    }
                }
                bf16x8 pf[2];
                attn_softmax_half<DYN>(sacc, vis, p.scale_log2, m_run, l_run, oacc, pf);      // generic form: a masked element's P is selected to 0
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int d = 0; d < ND; ++d)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        const bf16x8 vf = *(lds_frag_p)(vaddr[T][s2] + PAR * V_BYTES + d * 32 * 128);
                        oacc[d] = mfma_32x32x16<false>(vf, pf[s2], oacc[d]);
                    }
                __builtin_amdgcn_sched_group_barrier(0x100, UV_ATT_AHEAD, 1);
#pragma unroll
                for (int i_ = 0; i_ < 8 - UV_ATT_AHEAD; ++i_) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 1);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, UV_ATT_AHEAD, 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };

    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    using PD = std::integral_constant<int, -1>;
    int fast0 = i_lo <= i_hi ? i_lo : t_hi + 1;      // the first interior tile that sits in buffer 0
    fast0 += (fast0 - t_lo) & 1;
    int t = t_lo;
    // two passes over ONE generic loop (before and behind the interior pairs): the generic form is instantiated once
#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {
        const int end = pass == 0 ? min(fast0, t_hi + 1) : t_hi + 1;
        for (; t < end; ++t) tile(t, PD{});
        if (pass == 0) {
            for (; t + 2 <= i_hi; t += 2) {           // tiles t, t + 1, t + 2 interior: both successors are full tiles
                tile(t, P0{});
                tile(t + 1, P1{});
            }
        }
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    const int lane_e = attn_lane_here();
    if ((p.ldo & 7) == 0) {
        // O through LDS: wave-private images over the K / V^T buffers (free: the last tile ended on a barrier that every wave took)
        attn_store_lds(smem + wave_u * (32 * 144), p.out + (long)q0w * p.ldo + hcol, p.ldo, L - q0w, lane_e, oacc, inv);
    } else if (q0w + (lane_e & 31) < L) {
        attn_store_direct<false, ND>(p.out + (long)(q0w + (lane_e & 31)) * p.ldo + hcol + 4 * (lane_e >> 5), oacc, inv);
    }
}

constexpr int UV_WIN_SMEM = 2 * UV_ATT_KV * 256 + 2 * 128 * 128;      // K and V^T double-buffered: 64 KiB (>= 12 O images of 32 x 144 B)

__global__ __launch_bounds__(768) __attribute__((amdgpu_waves_per_eu(3, 3))) void flash_attn_win12_kernel(AttnWinArgs p) {
    __shared__ __attribute__((aligned(16))) char smem[UV_WIN_SMEM];
    win_body<12>(p, smem);
}

__global__ __launch_bounds__(256, 2) void flash_attn_win4_kernel(AttnWinArgs p) {
    __shared__ __attribute__((aligned(16))) char smem[UV_WIN_SMEM];
    win_body<4>(p, smem);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
static void launch_attn_win(AttnWinArgs a, const AttnPlan& plan, hipStream_t st) {
    a.q_blocks = plan.q_blocks;
    a.n12 = plan.n12;
    void (*kern)(AttnWinArgs) = plan.kernel == ATT_WIN12 ? flash_attn_win12_kernel : flash_attn_win4_kernel;
    hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(plan.block), 0, st, a);
}

// The plan uv_flash_attn_win_bf16 launches for this problem on the current device (256 CUs without one) under the current UV_OPT_ATTN_CUT and
// UV_OPT_ATTN_WIN_FORM.
extern "C" int uv_flash_attn_win_plan(int batch, int L, int H, int head_dim, int win_left, int win_right, char* kernel, int len, int* q_blocks,
                                      int* n12, int* grid) {
    UV_CHECK_ARG(kernel && len > 0 && q_blocks && n12 && grid, "uv_flash_attn_win_plan: null pointer");
    UV_CHECK_ARG(head_dim == 128, "uv_flash_attn_win_plan: head_dim %d unsupported (128 only)", head_dim);
    UV_CHECK_ARG(L > 0 && H > 0 && batch > 0, "uv_flash_attn_win_plan: bad shape B=%d L=%d H=%d", batch, L, H);
    UV_CHECK_ARG(win_left >= -1 && win_right >= -1, "uv_flash_attn_win_plan: window (%d, %d): each side >= 0, or -1 = unbounded", win_left, win_right);
    const AttnPlan plan = plan_attn_win(batch, L, H, win_left, win_right, uv_num_cus(), uv_option(UV_OPT_ATTN_CUT), uv_option(UV_OPT_ATTN_WIN_FORM));
    snprintf(kernel, len, "%s", kAttnKernelName[plan.kernel]);
    *q_blocks = plan.q_blocks; *n12 = plan.n12; *grid = plan.grid;
    return 0;
}

extern "C" int uv_flash_attn_win_bf16(const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, void* out, long ldo, int batch,
                                      int L, int H, int head_dim, float softmax_scale, int win_left, int win_right, void* stream) {
    const char* name = "uv_flash_attn_win_bf16";
    if (attn_self_check_shape(name, q, k, vt, out, batch, L, H, head_dim)) return -1;
    UV_CHECK_ARG(win_left >= -1 && win_right >= -1, "%s: window (%d, %d): each side >= 0, or -1 = unbounded", name, win_left, win_right);
    if (attn_self_check_layout(name, q, k, vt, out, ldq, ldk, ldvt, ldo, batch, L)) return -1;
    AttnWinArgs a;
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.vt = (const bf16_t*)vt; a.out = (bf16_t*)out;
    a.ldq = ldq; a.ldk = ldk; a.ldvt = ldvt; a.ldo = ldo;
    a.Lq = L; a.Lk = L; a.H = H; a.batch = batch;
    a.scale_log2 = softmax_scale * 1.4426950408889634f;
    a.q_rs = nullptr; a.q_w = nullptr;
    a.left = win_left < 0 || win_left > L ? L : win_left;        // unbounded = every earlier key
    a.right = win_right < 0 || win_right > L ? L : win_right;
    launch_attn_win(a, plan_attn_win(batch, L, H, win_left, win_right, uv_num_cus(), uv_option(UV_OPT_ATTN_CUT), uv_option(UV_OPT_ATTN_WIN_FORM)),
                    (hipStream_t)stream);
    UV_CHECK_LAUNCH(name);
    return 0;
}
