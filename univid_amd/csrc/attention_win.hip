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
// the wave's last query sees nothing of the first tile its first query needs). The dense kernels' -INFINITY scheme would compute -inf - -inf
// there. Here the "unset" maximum and a masked score are the FINITE sentinel UV_WIN_UNSET, and P of a masked element is SELECTED to 0 by the
// visibility bit, not computed: such a lane gets mt = unset, grow = 0 (no move of its own), alpha = exp2(0) = 1 exactly if a neighbour moves,
// P = 0, l += 0, and its maximum stays unset until its first visible key (then alpha = exp2(-1e30 scale) = 0 on l = 0, O = 0 - what the dense
// kernels compute from -inf).
// Everything else is flash_attn_fwd12_kernel's arithmetic operation for operation (32-key halves, UV_ATT_DEFER, order within a tile, bf16
// rounding of P, 1 / l): a window that covers every key reproduces the dense launch bit for bit, and a query's bits depend on its 32-query unit
// only, never on the query-block cut, the form or the other queries of the launch.
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

#define UV_WIN_UNSET (-1.0e30f)

// The lane id, produced HERE (two VALU instructions, volatile: not hoisted): the rare branches and the epilogue derive their lane constants from it
// instead of keeping them - or the lane id itself - in registers across the tile loops, where they were spilled.
__device__ __forceinline__ int win_lane_here() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

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

    // ---- staging (flash_attn_fwd12_kernel's): the 32 one-KiB pieces of a tile (K pieces 0..15 = 4 LDS rows each, V^T pieces 0..15 = 8 rows
    // each) are dealt round-robin over the waves. K pieces of equal pc & 3 share the swizzle key and the row permutation bits, V^T pieces of
    // equal parity the swizzle key: at 12 waves (K w, w + 12; V^T w - 4, w + 8) and at 4 (K and V^T w, w + 4, w + 8, w + 12) ONE lane offset
    // per operand serves all of a wave's pieces; the piece's row / column step goes into the uniform base.
    const int s4 = lane >> 4, s8 = lane >> 3;
    unsigned koff, voff;
    {
        const int p3 = wave_u & 3;
        const int c = (lane & 15) ^ ((4 * p3 + s4) & 15);
        const int swap2 = ((p3 & 1) << 1) | (p3 >> 1);
        koff = (unsigned)((s4 + 4 * swap2) * (int)p.ldk + c * 8) * 2u;
        const int cv = (lane & 7) ^ ((4 * (wave_u & 1) + (s8 >> 1)) & 7);
        voff = (unsigned)(s8 * (int)p.ldvt + cv * 8) * 2u;
    }
    const long kstep = (long)UV_ATT_KV * p.ldk * 2;
    const long k16 = 16 * p.ldk * 2, v8 = 8 * p.ldvt * 2;
    const char* kbase = (const char*)(p.k + hcol) + t_lo * kstep;                          // tile t_lo; += kstep per tile
    const char* vbase = (const char*)(p.vt + hcol * p.ldvt) + (long)t_lo * 2 * UV_ATT_KV;  // += 128 B per tile
    const unsigned smem_a = (unsigned)(uintptr_t)(lds_void_a*)smem;
    auto fetch_v = [&](const char* vb_t, int buf) {
        if constexpr (NW == 12) {
            const int vq0 = wave_u - 4, vq1 = wave_u + 8;
            if (wave_u >= 4) glds16_sbase(vb_t + vq0 * v8, voff, smem_a + V_OFF + buf * V_BYTES + vq0 * 1024);
            if (wave_u < 8) glds16_sbase(vb_t + vq1 * v8, voff, smem_a + V_OFF + buf * V_BYTES + vq1 * 1024);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) glds16_sbase(vb_t + (wave_u + 4 * i) * v8, voff, smem_a + V_OFF + buf * V_BYTES + (wave_u + 4 * i) * 1024);
        }
    };
    auto fetch_full = [&](const char* kb_t, const char* vb_t, int buf) {
        if constexpr (NW == 12) {
            glds16_sbase(kb_t + (wave_u >> 2) * k16, koff, smem_a + buf * K_BYTES + wave_u * 1024);
            if (wave_u < 4) glds16_sbase(kb_t + 3 * k16, koff, smem_a + buf * K_BYTES + (wave_u + 12) * 1024);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) glds16_sbase(kb_t + i * k16, koff, smem_a + buf * K_BYTES + (wave_u + 4 * i) * 1024);
        }
        fetch_v(vb_t, buf);
    };
    // the ragged last tile: K rows clamped to L - 1 in the lane offset (the row inside the tile is 16 (pc >> 2) + the lane's row of its 16)
    auto fetch_clamped = [&](int kv0, const char* kb_t, const char* vb_t, int buf) {
        const int last = L - 1 - kv0;
        const int p3 = wave_u & 3;
        const int ln = win_lane_here();
        const int r4 = ln >> 4;
        const int krl = r4 + 4 * (((p3 & 1) << 1) | (p3 >> 1));
        const unsigned c16 = (unsigned)(((ln & 15) ^ ((4 * p3 + r4) & 15)) << 4);
#pragma unroll
        for (int i = 0; i < (NW == 12 ? 2 : 4); ++i) {
            const int pc = wave_u + NW * i;
            if (pc < 16) glds16_sbase(kb_t, (unsigned)(min(16 * (pc >> 2) + krl, last) * (int)p.ldk) * 2u + c16, smem_a + buf * K_BYTES + pc * 1024);
        }
        fetch_v(vb_t, buf);
    };

    typedef const __attribute__((address_space(3))) bf16x8* lds_frag_p;
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
    if (t_lo < nt_full) fetch_full(kbase, vbase, 0);
    else fetch_clamped(t_lo * UV_ATT_KV, kbase, vbase, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) asm volatile("" : "+v"(qf[kk]), "+v"(kaddr[kk]));      // every prologue load has landed before the loops
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(vaddr[i >> 1][i & 1]));
    asm volatile("" : "+v"(koff), "+v"(voff));
    __syncthreads();

    if (!compute_wave) {
        for (int t = t_lo; t <= t_hi; ++t) {
            vbase += 2 * UV_ATT_KV;
            kbase += kstep;
            const int nbuf = ((t - t_lo) & 1) ^ 1;
            if (t < t_hi) {
                if (t + 1 < nt_full) fetch_full(kbase, vbase, nbuf);
                else fetch_clamped((t + 1) * UV_ATT_KV, kbase, vbase, nbuf);
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
            fetch_full(kbase, vbase, PAR ^ 1);
        } else if (t < t_hi) {
            if (t + 1 < nt_full) fetch_full(kbase, vbase, PAR ^ 1);
            else fetch_clamped(kv0 + UV_ATT_KV, kbase, vbase, PAR ^ 1);
        }
        const bool active = !DYN || (t >= w_lo && t <= w_hi);
        const bool edge = DYN && !(t >= i_lo && t <= i_hi);
        if (active) {
#pragma unroll
            for (int T = 0; T < 2; ++T) {
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
                float mt = sacc[0];
#pragma unroll
                for (int e = 1; e < 16; ++e) mt = fmaxf(mt, sacc[e]);
                {
                    const unsigned u = __builtin_bit_cast(unsigned, mt);
                    const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
                    mt = fmaxf(__builtin_bit_cast(float, (unsigned)sw[0]), __builtin_bit_cast(float, (unsigned)sw[1]));
                }
                const float grow = (mt - m_run) * p.scale_log2;      // 0 while both are unset, ~1e30 scale at the first visible key
                if (__any(grow > UV_ATT_DEFER)) {
                    const float m_new = fmaxf(m_run, mt);
                    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * p.scale_log2);
                    l_run *= alpha;
#pragma unroll
                    for (int d = 0; d < ND; ++d)
#pragma unroll
                        for (int e = 0; e < 16; ++e) oacc[d][e] *= alpha;
                    m_run = m_new;
                }
                const float mneg = -m_run * p.scale_log2;
                float psum = 0.f;
                bf16x8 pf[2];
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[8 * s2 + j], p.scale_log2, mneg));
                        if constexpr (DYN) pv = ((vis >> (8 * s2 + j)) & 1u) ? pv : 0.f;      // a masked element's P is selected, not computed
                        psum += pv;
                        pf[s2][j] = (__bf16)pv;
                    }
                l_run += psum;
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
    const int lane_e = win_lane_here();
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
    UV_CHECK_ARG(q && k && vt && out, "%s: null pointer", name);
    UV_CHECK_ARG(head_dim == 128, "%s: head_dim %d unsupported (128 only)", name, head_dim);
    UV_CHECK_ARG(L > 0 && L <= (1 << 30) && H > 0 && batch > 0, "%s: bad shape B=%d L=%d H=%d", name, batch, L, H);
    UV_CHECK_ARG(win_left >= -1 && win_right >= -1, "%s: window (%d, %d): each side >= 0, or -1 = unbounded", name, win_left, win_right);
    UV_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldo % 4 == 0, "%s: leading dimensions must be multiples of 8 elements", name);
    UV_CHECK_ARG(ldvt >= (long)(batch - 1) * L + (long)((L + 63) / 64) * 64,
                 "%s: ldvt=%ld must cover (batch-1)*L + L rounded up to 64 (batch=%d L=%d)", name, ldvt, batch, L);
    UV_CHECK_ARG(batch == 1 || L % 8 == 0, "%s: batch > 1 needs L %% 8 == 0 (L=%d)", name, L);
    // the LDS-DMA pieces are addressed with 32-bit lane offsets from a uniform base (the dense entry falls back to flash_attn_fwd_kernel there)
    UV_CHECK_ARG(128 * ldvt < (1L << 30) && 64 * ldk < (1L << 30), "%s: ldk=%ld / ldvt=%ld too large for 32-bit piece offsets", name, ldk, ldvt);
    UV_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)out) & 15) == 0, "%s: pointers must be 16-byte aligned", name);
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
