// Flash attention forward under a block mask (head_dim 128, bf16 in / fp32 softmax + accumulate / bf16 out) for gfx950: the opt-in block-sparse
// self-attention of the DiT (WanModel.set_attn_block_mask; Lq == Lk == L, every sample attends all L keys).
//
// No counterpart in the reference: its flash_attention (models/wan/utils/modules/attention.py:24-130) knows global, causal and sliding-window
// attention only. The masks meant are the block-sparse ones of the training-free sparse-attention schemes for video DiTs (3-D tile
// neighbourhoods, spatial / temporal heads, densities that decay with frame distance): sets of key tiles per query block that are not contiguous
// in the flattened (frame, row, column) order and may differ per head.
//
// Query i of head h attends key j iff mask[h][i / 128][j / 64] and j < L. Exact: the same softmax over fewer keys. The mask arrives as a tile
// SCHEDULE prepared once per mask (univid_amd/_lib.py: prepare_block_mask): tile_idx [Hm, nqb, nkb] holds each (mask head, query block)'s visible
// 64-key tiles in ascending order, tile_cnt [Hm, nqb] how many, Hm = 1 (shared by the heads) or H; the samples of a stacked launch share it
// (uv_flash_attn_bs_bf16) or bring one set of lists each, a leading sample axis (uv_flash_attn_bs_lists_bf16: attention_sel.hip builds them).
//
// One 4-wave workgroup per (sample, head, 128-query block) in flash_attn_fwd3_kernel's XCD-contiguous id order, flash_attn_win4_kernel's
// staging (K and V^T both double-buffered, 64 KiB, one barrier per tile, uniform-base LDS-DMA pieces). It walks its LIST: the index of tile
// n + 1 is read (wave-uniformly, plain loads) during tile n - 1, so tile n's fetch of its successor is issued where the windowed kernel issues
// it. All four waves compute every listed tile - the granularity is the workgroup's, there is no per-wave "outside" class.
//   tiles 0 .. cnt - 2   the unmasked dense body in pairs with compile-time buffer parity (the dense main loop); a short generic tail
//   tile cnt - 1         generic; if it is the ragged tile nkb - 1 (L % 64 != 0), the windowed kernel's edge path: K rows clamped to L - 1,
//                        visibility key < L, masked scores replaced by the finite UV_WIN_UNSET, P of a masked element SELECTED to 0 (V^T's pad
//                        columns behind a stacked sample are the next sample's keys: finite, not zero)
// NO LIST CONTENT READS OUTSIDE k / V^T: the count is clamped into [0, nkb]; an entry that is not the list's last is clamped into the FULL
// tiles [0, L / 64 - 1] (a valid list holds the ragged tile last or not at all), the last entry into [0, nkb - 1] and fetched by what it is.
// A block whose clamped count is 0 (the host refuses such masks) leaves before its first fetch and before any barrier and writes zero rows.
// The per-wave arithmetic of a half is the dense kernels' own code (attn_args.h: attn_qk_half, attn_softmax_half, attn_pv_half; the staging is
// AttnStage<4>, the O stores attn_store_lds / attn_store_direct; padded query rows are duplicates of row L - 1): a query's bits depend on its
// 32-query unit and on the ascending list of tiles it visits, on nothing else - the all-ones mask reproduces the dense launch bit for bit, and a
// block's result is the dense kernels' on K / V gathered to its tiles.
#include "attn_args.h"
#include <stdio.h>
#include <type_traits>

constexpr int UV_BS_SMEM = 2 * UV_ATT_KV * 256 + 2 * 128 * 128;      // K and V^T double-buffered: 64 KiB (>= 4 O images of 32 x 144 B)

__global__ __launch_bounds__(256, 2) void flash_attn_bs4_kernel(AttnBsArgs p) {
    constexpr int D = 128, KROW = 256, NKK = 8, ND = 4;
    constexpr int K_BYTES = UV_ATT_KV * KROW, V_BYTES = D * 128;
    constexpr int V_OFF = 2 * K_BYTES;
    __shared__ __attribute__((aligned(16))) char smem[UV_BS_SMEM];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int r = lane & 31, h = lane >> 5;
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = p.Lq;

    // flash_attn_fwd3_kernel's order: XCD x works through a contiguous range of (sample, head, block) ids
    const int nb = gridDim.x, per = nb >> 3, rem = nb & 7;
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int vb = x * per + min(x, rem) + j;
    const int bh = vb / p.q_blocks;
    const int qblk = vb - bh * p.q_blocks;
    const int head = bh % p.H;
    const int sample = bh / p.H;
    attn_sample_offset<0>(p, sample);
    const int q0w = (qblk * 4 + wave_u) * UV_ATT_QW;
    const long hcol = (long)head * D;

    // ---- this block's schedule: its row of the list, the clamped count
    const int nkb = p.nkb, nt_full = L / UV_ATT_KV;
    const int row = ((p.mask_samples == 1 ? 0 : sample) * p.mask_heads + (p.mask_heads == 1 ? 0 : head)) * p.q_blocks + qblk;
    // the list and the counts are read through the constant address space: nothing writes them while the kernel runs, and a uniform read of
    // it is a scalar load - which neither waits for the LDS-DMA pieces in flight (a vector load's vmcnt would) nor occupies a lane register.
    // uv_flash_attn_bs_lists_bf16: ANOTHER KERNEL on the same stream (uv_attn_bs_select) wrote them just before. What the read rests on: that
    // kernel has completed before this one's first wave starts (stream order: the dispatch packet's barrier bit), its plain vector stores
    // were written back to the L2 at its end (the packet's release fence), and this kernel's dispatch starts with the packet's acquire
    // fence, which invalidates the scalar data cache together with the vector L1 - HSA's kernel-boundary rule (LLVM's AMDGPU memory model:
    // "kernel dispatch acquire"), the same one that makes any kernel's plain loads see its predecessor's stores; eager launches and HIP
    // graph replays on one stream both keep it. Nothing inside a kernel would: a list written DURING this kernel could be read stale.
    typedef const __attribute__((address_space(4))) int* const_int_p;
    const const_int_p lst = (const_int_p)(p.tile_idx + (long)row * nkb);
    const int cnt = __builtin_amdgcn_readfirstlane(min(max(((const_int_p)p.tile_cnt)[row], 0), nkb));
    if (cnt == 0) {
        // nothing to attend (refused by the host; a corrupt count): zero rows, no fetch, no barrier
        const int ln = attn_lane_here();
        const int qr = q0w + (ln & 31);
        if (qr < L) {
            bf16_t* op = p.out + (long)qr * p.ldo + hcol + 64 * (ln >> 5);
            const u32x2 z = {0u, 0u};
#pragma unroll
            for (int i = 0; i < 16; ++i) *(u32x2*)(op + 4 * i) = z;
        }
        return;
    }
    // entry n of the list as a tile that may be fetched: never past the row (the read), never past the operand (the value). Two steps: the
    // read is issued a tile ahead, the clamp runs behind that tile's closing wait - never a wait of its own in front of a fetch
    const int hi_inner = max(nt_full, 1) - 1;
    auto raw_at = [&](int n) { return lst[min(n, nkb - 1)]; };
    auto clamp_at = [&](int raw, int n) { return min(max(raw, 0), n < cnt - 1 ? hi_inner : nkb - 1); };

    // the lane's query (a padded row is a duplicate of row L - 1)
    const int qm = min(q0w + r, L - 1);
    bf16x8 qf[NKK];
    AttnQNorm<NKK, 0> qnorm;
    attn_load_q<NKK, 0>(p, qf, qnorm, qm, hcol, h);

    // ---- staging: AttnStage (attn_args.h), the tile's base computed from its index; the ragged last tile clamps its K rows to L - 1
    const unsigned smem_a = (unsigned)(uintptr_t)(lds_void_a*)smem;
    AttnStage<4> stage(smem_a, wave_u, lane, p.ldk, p.ldvt);
    const long kstep = (long)UV_ATT_KV * p.ldk * 2;
    const char* khead = (const char*)(p.k + hcol);                     // tile t: + t kstep
    const char* vhead = (const char*)(p.vt + hcol * p.ldvt);           // tile t: + 128 t bytes
    auto fetch_full = [&](int t, int buf) { stage.full(khead + t * kstep, vhead + (long)t * 2 * UV_ATT_KV, buf); };
    auto fetch_any = [&](int t, int buf) {
        if (t < nt_full) fetch_full(t, buf);
        else stage.clamped(khead + t * kstep, vhead + (long)t * 2 * UV_ATT_KV, L - 1 - t * UV_ATT_KV, buf);
    };

    unsigned kaddr[NKK];
    unsigned vaddr[2][2];
    attn_frag_addrs(smem_a, V_OFF, r, h, kaddr, vaddr);

    f32x16 oacc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;
    float m_run = UV_WIN_UNSET, l_run = 0.f;

    int t_cur = clamp_at(raw_at(0), 0), t_nxt = clamp_at(raw_at(1), 1);
    fetch_any(t_cur, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) asm volatile("" : "+v"(qf[kk]), "+v"(kaddr[kk]));      // every prologue load has landed before the loops
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(vaddr[i >> 1][i & 1]));
    asm volatile("" : "+v"(stage.koff), "+v"(stage.voff));
    __syncthreads();

    // One staged tile: entry n of the list, tile t, its successor t_next. par_tag >= 0: a FULL tile in the buffer of that parity whose successor
    // is full too - the dense kernels' main loop, no masking code. par_tag = -1: the generic form - parity, "is there a successor, is it
    // full" and "is this the ragged tile" decided at run time.
    auto tile = [&](int n, int t, int t_next, auto par_tag) {
        constexpr bool DYN = decltype(par_tag)::value < 0;
        const int PAR = DYN ? (n & 1) : decltype(par_tag)::value;
        if constexpr (!DYN) {
            fetch_full(t_next, PAR ^ 1);
        } else if (n + 1 < cnt) {
            fetch_any(t_next, PAR ^ 1);
        }
        const bool edge = DYN && t >= nt_full;
        const int kv0 = t * UV_ATT_KV;
#pragma unroll
        for (int T = 0; T < 2; ++T) {
            f32x16 sacc = attn_qk_half(kaddr, qf, PAR * K_BYTES + T * 32 * KROW);
            // visibility of the half's 16 accumulator rows: register e holds key kv0 + 32 T + 8 h + (e & 3) + 4 ((e >> 2) & 1) + 16 (e >> 3)
            // (perm23 of the accumulator row); visible iff it is below L
            unsigned vis = 0xffffu;
            if (DYN && edge) {
                const int b = L - 1 - kv0 - 32 * T - 8 * h;
                vis = 0u;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int c = (e & 3) + 4 * ((e >> 2) & 1) + 16 * (e >> 3);
                    const bool ok = c <= b;
                    vis |= (ok ? 1u : 0u) << e;
                    sacc[e] = ok ? sacc[e] : UV_WIN_UNSET;
                }
            }
            bf16x8 pf[2];
            attn_softmax_half<DYN>(sacc, vis, p.scale_log2, m_run, l_run, oacc, pf);      // generic form: a masked element's P is selected to 0
            attn_pv_half(vaddr[T], PAR * V_BYTES, pf, oacc);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };

    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    using PD = std::integral_constant<int, -1>;
    int n = 0;
    // pairs while entries n + 1 and n + 2 are not the list's last: tiles n, n + 1 and both successors are full tiles. n stays even: buffer 0.
    for (; n + 2 < cnt - 1; n += 2) {
        const int r2 = raw_at(n + 2), r3 = raw_at(n + 3);
        tile(n, t_cur, t_nxt, P0{});
        const int t2 = clamp_at(r2, n + 2);
        tile(n + 1, t_nxt, t2, P1{});
        t_cur = t2;
        t_nxt = clamp_at(r3, n + 3);
    }
    // the last one to three tiles, the list's last entry among them: ONE instantiation of the generic form
    for (; n < cnt; ++n) {
        const int r2 = raw_at(n + 2);
        tile(n, t_cur, t_nxt, PD{});
        t_cur = t_nxt;
        t_nxt = clamp_at(r2, n + 2);
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

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
// The plan uv_flash_attn_bs_bf16 launches for this problem: one kernel, blocks of 128 queries, grid = q_blocks * H * batch.
extern "C" int uv_flash_attn_bs_plan(int batch, int L, int H, int head_dim, char* kernel, int len, int* q_blocks, int* grid) {
    UV_CHECK_ARG(kernel && len > 0 && q_blocks && grid, "uv_flash_attn_bs_plan: null pointer");
    UV_CHECK_ARG(head_dim == 128, "uv_flash_attn_bs_plan: head_dim %d unsupported (128 only)", head_dim);
    UV_CHECK_ARG(L > 0 && L <= (1 << 30) && H > 0 && batch > 0, "uv_flash_attn_bs_plan: bad shape B=%d L=%d H=%d", batch, L, H);
    const AttnPlan plan = plan_attn_bs(batch, L, H);
    snprintf(kernel, len, "%s", kAttnKernelName[plan.kernel]);
    *q_blocks = plan.q_blocks; *grid = plan.grid;
    return 0;
}

// Both entries: the checks, the argument block, the launch. mask_samples was checked by the caller.
static int attn_bs_launch(const char* name, const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, void* out, long ldo,
                          int batch, int L, int H, int head_dim, float softmax_scale, const int* tile_idx, const int* tile_cnt, int mask_heads,
                          int mask_samples, void* stream) {
    UV_CHECK_ARG(tile_idx && tile_cnt, "%s: null pointer", name);
    if (attn_self_check_shape(name, q, k, vt, out, batch, L, H, head_dim)) return -1;
    UV_CHECK_ARG(mask_heads == 1 || mask_heads == H, "%s: mask_heads=%d must be 1 (one mask for all heads) or H=%d", name, mask_heads, H);
    if (attn_self_check_layout(name, q, k, vt, out, ldq, ldk, ldvt, ldo, batch, L)) return -1;
    UV_CHECK_ARG((((uintptr_t)tile_idx | (uintptr_t)tile_cnt) & 3) == 0, "%s: tile_idx / tile_cnt must be 4-byte aligned", name);
    const AttnPlan plan = plan_attn_bs(batch, L, H);
    AttnBsArgs a;
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.vt = (const bf16_t*)vt; a.out = (bf16_t*)out;
    a.ldq = ldq; a.ldk = ldk; a.ldvt = ldvt; a.ldo = ldo;
    a.Lq = L; a.Lk = L; a.H = H; a.batch = batch;
    a.scale_log2 = softmax_scale * 1.4426950408889634f;
    a.q_rs = nullptr; a.q_w = nullptr;
    a.q_blocks = plan.q_blocks; a.n12 = 0;
    a.tile_idx = tile_idx; a.tile_cnt = tile_cnt; a.mask_heads = mask_heads; a.nkb = (L + UV_ATT_KV - 1) / UV_ATT_KV; a.mask_samples = mask_samples;
    hipLaunchKernelGGL(flash_attn_bs4_kernel, dim3(plan.grid), dim3(plan.block), 0, (hipStream_t)stream, a);
    UV_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int uv_flash_attn_bs_bf16(const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, void* out, long ldo, int batch,
                                     int L, int H, int head_dim, float softmax_scale, const int* tile_idx, const int* tile_cnt, int mask_heads,
                                     void* stream) {
    return attn_bs_launch("uv_flash_attn_bs_bf16", q, ldq, k, ldk, vt, ldvt, out, ldo, batch, L, H, head_dim, softmax_scale, tile_idx, tile_cnt,
                          mask_heads, 1, stream);
}

// The same kernel under lists with a leading sample axis (csrc/attention_sel.hip: uv_attn_bs_select writes them on the device).
extern "C" int uv_flash_attn_bs_lists_bf16(const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, void* out, long ldo,
                                           int batch, int L, int H, int head_dim, float softmax_scale, const int* tile_idx, const int* tile_cnt,
                                           int mask_heads, int mask_samples, void* stream) {
    UV_CHECK_ARG(mask_samples == 1 || mask_samples == batch,
                 "uv_flash_attn_bs_lists_bf16: mask_samples=%d must be 1 (the samples share the lists) or batch=%d", mask_samples, batch);
    return attn_bs_launch("uv_flash_attn_bs_lists_bf16", q, ldq, k, ldk, vt, ldvt, out, ldo, batch, L, H, head_dim, softmax_scale, tile_idx,
                          tile_cnt, mask_heads, mask_samples, stream);
}
