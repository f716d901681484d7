// Flash attention forward with MXFP8 q / k (e4m3fn codes + one e8m0 byte per 32 head-dim elements; format: include/univid_hip.h), bf16 V^T and
// output, head_dim 128, for gfx950: the opt-in "mxfp8_qk" mode of the DiT's self-attention (WanModel.set_attn_precision).
//
// Replaces: flash_attention()  models/wan/utils/modules/attention.py:24-130 as called from WanSelfAttention.forward model.py:145-150 - with q and k
//           NARROWER than the reference's bf16 (3 mantissa bits); everything behind S is the bf16 kernels' arithmetic (attention.hip).
//
// S^T = K.Q^T runs on the block-scaled matrix instruction v_mfma_scale_f32_32x32x64_f8f6f4: two instructions per 32-key half (head-dim
// elements 0..63, then 64..127, into the same accumulator: every S element is ONE chain) in place of eight 32x32x16 bf16 ones, on 128-byte K rows.
// The instruction's C/D layout is the 32x32 one of the bf16 form, so the rest of a tile is the bf16 kernels' own code (attn_args.h): masking with the
// true key index (attn_mask_ragged), the deferred reference maximum reconsidered per 32-key half, exp2 and P in bf16 as the B operand of
// O^T = V^T.P^T (attn_softmax_half), O through LDS (attn_store_lds).
//
// Operand lane map of the instruction with 8-bit elements, MEASURED with exact integer data (one-hot e4m3 codes against per-lane scale bytes;
// tests/test_attn_mxqk.py keeps it pinned through the kernel): lane l = (row / column r = l & 31, half h = l >> 5) holds K-index bytes
// 16 h .. 16 h + 15 in its first four operand registers and 32 + 16 h .. 32 + 16 h + 15 in its last four - the 64-element step is two 32-element
// halves, each spread over the two lane halves like a 32x32x32 step. Byte p of lane half h of A meets byte p of lane half h of B and no other.
// MX block b of the step (K indices 32 b .. 32 b + 31) is therefore register half b of BOTH lane halves, and its scale is read from lane (r, h = b):
// the byte of that lane's scale register that op_sel (0 .. 3) names. A lane does not hold a whole block. Here: a row's four scale bytes travel
// as one dword s; lane (r, h) passes s >> 8 h, step 0 (head-dim blocks 0, 1) selects byte 0, step 1 (blocks 2, 3) byte 2. The first operand's
// rows are the accumulator's rows ((e & 3) + 8 (e >> 2) + 4 h in register e), the second operand's columns sit on the lanes.
//
// One kernel body in two sizes, the same per-wave arithmetic (a query's bits do not depend on the size, the query-block cut, the batch or its
// neighbours):
//   flash_attn_mxqk12_kernel  Lk >= 2048: flash_attn_fwd12_kernel's 12-wave workgroup, 12 / 8 unit cut, XCD order and loader-only waves
//   flash_attn_mxqk4_kernel   shorter Lk: 4 waves x 32 queries, plain (sample, head, block) order; correct, not tuned
// plan_attn_mxqk (attn_args.h, on top of plan_attn) decides between them; launch below is the one launch site.
// A staged tile = 64 keys: K codes [64][128 B] (LDS row i <- key perm23(i), 16-byte chunk ^= (row >> 1) & 7 - the V^T tile's geometry, so
// its conflict-free fragment read carries over), V^T [128][64] bf16 as in attention.hip, and the 64 keys' scale dwords (256 B, one 4-byte
// LDS-DMA per lane of one wave). 24 one-KiB LDS-DMA pieces + the scales per tile, dealt round-robin over the waves (two per wave at 12 waves);
// tiles double-buffered, tile t + 1 requested at the top of tile t, one vmcnt(0) + barrier per tile. Every tile runs ONE generic form (row
// clamp and "ragged?" decided at run time): no chain of tail instantiations for the register allocator to spill across.
#include "attn_args.h"
#include <stdio.h>

typedef __attribute__((address_space(3))) void lds_void_a;
typedef __attribute__((ext_vector_type(8))) int i32x8;

struct AttnMxArgs {
    const uint8_t* qc;   // [batch * Lq, ldq] e4m3 codes, head h at byte h * 128
    const uint8_t* qs;   // [batch * Lq, ld_qs] e8m0 bytes, head h at byte h * 4
    const uint8_t* kc;   // [batch * Lk, ldk]
    const uint8_t* ks;   // [batch * Lk, ld_ks]
    const bf16_t* vt;    // [H * 128, ldvt] as AttnArgs
    bf16_t* out;         // [batch * Lq, ldo]
    long ldq, ld_qs, ldk, ld_ks, ldvt, ldo;
    int Lq, Lk, H, q_blocks, batch, n12;
    float scale_log2;
};

constexpr int MXA_K_BYTES = UV_ATT_KV * 128;          // 8 KiB of codes
constexpr int MXA_V_BYTES = 128 * 128;                // 16 KiB of V^T
constexpr int MXA_S_OFF = MXA_K_BYTES + MXA_V_BYTES;  // the tile's 64 scale dwords
constexpr int MXA_STAGE = MXA_S_OFF + UV_ATT_KV * 4;
constexpr int MXA_PIECES = (MXA_K_BYTES + MXA_V_BYTES) / 1024;   // 8 of K, then 16 of V^T: piece pc lands at stage + 1024 pc
// the O epilogue's twelve wave-private images (32 rows x 144 B) need more than the two stages: the allocation must not shrink below them
constexpr int MXA_SMEM = 2 * MXA_STAGE > 12 * 32 * 144 ? 2 * MXA_STAGE : 12 * 32 * 144;

template <int NW>
__device__ __forceinline__ void mxqk_body(AttnMxArgs p, char* smem) {
    constexpr int ND = 4, NP = MXA_PIECES / NW;
    static_assert(MXA_PIECES % NW == 0, "pieces are dealt evenly");
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int r = lane & 31, h = lane >> 5;
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);

    int bh, q0w;
    bool compute_wave = true;
    if constexpr (NW == 12) {       // flash_attn_fwd12_kernel's block order: 12-unit blocks first, XCD-contiguous ranges when the totals divide by 8
        const int nbh = p.H * p.batch, n8 = p.q_blocks - p.n12;
        const int tot12 = p.n12 * nbh, tot8 = n8 * nbh;
        int id = blockIdx.x;
        if ((tot12 & 7) == 0 && (tot8 & 7) == 0) {
            const int x = blockIdx.x & 7, j = blockIdx.x >> 3, c12 = tot12 >> 3, c8 = tot8 >> 3;
            id = j < c12 ? x * c12 + j : tot12 + x * c8 + (j - c12);
        }
        int u0, units;
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
        const int nwu = (p.Lq + UV_ATT_QW - 1) / UV_ATT_QW;
        compute_wave = wave_u < min(units, nwu - u0);      // the others are loader-only: their share of the staging and every barrier
        q0w = (u0 + wave_u) * UV_ATT_QW;
    } else {
        bh = blockIdx.x / p.q_blocks;
        q0w = (blockIdx.x - bh * p.q_blocks) * (NW * UV_ATT_QW) + wave_u * UV_ATT_QW;
    }
    const int head = bh % p.H;
    {   // independent samples: rows of q / k / out (codes and scales alike), columns of V^T
        const long b = bh / p.H;
        p.qc += b * p.Lq * p.ldq;  p.qs += b * p.Lq * p.ld_qs;
        p.kc += b * p.Lk * p.ldk;  p.ks += b * p.Lk * p.ld_ks;
        p.vt += b * p.Lk;
        p.out += b * p.Lq * p.ldo;
    }
    const long hcol = (long)head * 128;

    // ---- Q fragments (B operand): step i = head-dim bytes 64 i .. 64 i + 63; lane (r, h) holds bytes 64 i + 16 h .. + 15 and 64 i + 32 + 16 h .. + 15
    i32x8 qf[2];
    int qsc;
    {
        const long qrow = min(q0w + r, p.Lq - 1);
        const uint8_t* qp = p.qc + qrow * p.ldq + hcol + 16 * h;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const u32x4 lo = *(const u32x4*)(qp + 64 * i), hi = *(const u32x4*)(qp + 64 * i + 32);
            qf[i] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        }
        qsc = (int)(*(const uint32_t*)(p.qs + qrow * p.ld_qs + head * 4) >> (8 * h));
    }

    // ---- staging: this wave's NP pieces (piece pc = wave + NW i) and, on the last wave, the tile's scale dwords
    const char* pbase[NP];      // the piece's source of tile 0 without the key-row term (K) / at key column 0 (V^T)
    int pkrow[NP];              // K pieces: the key row (inside the tile) this lane's LDS row holds
    const int s8 = lane >> 3, pch = lane & 7;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int pc = wave_u + NW * i;
        if (pc < 8) {
            const int lrow = 8 * pc + s8;
            pkrow[i] = perm23(lrow);
            pbase[i] = (const char*)p.kc + hcol + ((pch ^ ((lrow >> 1) & 7)) << 4);
        } else {
            const int drow = 8 * (pc - 8) + s8;
            pkrow[i] = 0;
            pbase[i] = (const char*)(p.vt + (hcol + drow) * p.ldvt + ((pch ^ ((drow >> 1) & 7)) << 3));
        }
    }
    const int sc_krow = perm23(lane);
    const uint8_t* const sc_base = p.ks + head * 4;
    auto fetch = [&](int t, int buf) {      // rows at Lk and beyond are never read: the ragged tile clamps codes and scales alike
        char* stage = smem + buf * MXA_STAGE;
        const int kv0 = t * UV_ATT_KV;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int pc = wave_u + NW * i;
            const char* src = pc < 8 ? pbase[i] + (long)min(kv0 + pkrow[i], p.Lk - 1) * p.ldk : pbase[i] + 2L * kv0;
            __builtin_amdgcn_global_load_lds(src, (lds_void_a*)(stage + pc * 1024), 16, 0, 0);
        }
        if (wave_u == NW - 1)
            __builtin_amdgcn_global_load_lds(sc_base + (long)min(kv0 + sc_krow, p.Lk - 1) * p.ld_ks, (lds_void_a*)(stage + MXA_S_OFF), 4, 0, 0);
    };

    // fragment read offsets inside a stage. K codes and V^T rows are both 128 B with chunk ^= (row >> 1) & 7 ((32 x + r) >> 1 & 7 == (r >> 1) & 7):
    //   K  : row 32 T + r, step i, register half s: logical chunk 4 i + 2 s + h        V^T: row 32 d + r, logical chunk 4 T + 2 s + h
    int foff[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int s = 0; s < 2; ++s) foff[a][s] = r * 128 + (((4 * a + 2 * s + h) ^ ((r >> 1) & 7)) << 4);

    f32x16 oacc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const int nt = (p.Lk + UV_ATT_KV - 1) / UV_ATT_KV;
    const int nt_full = p.Lk / UV_ATT_KV;
    fetch(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < 2; ++i) asm volatile("" : "+v"(qf[i]));     // every prologue load has landed before the loop (see flash_attn_fwd_kernel)
    asm volatile("" : "+v"(qsc));
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        const char* base = smem + (t & 1) * MXA_STAGE;
        if (t + 1 < nt) fetch(t + 1, (t + 1) & 1);       // the other stage: last read in tile t - 1, fenced by its barrier
        if (compute_wave) {
            const int kv0 = t * UV_ATT_KV;
            const bool masked = t >= nt_full;
#pragma unroll
            for (int T = 0; T < 2; ++T) {
                // ---- S^T half: 32 keys x 32 queries, two block-scaled steps into one accumulator
                const char* kb = base + T * 32 * 128;
                const int ksc = (int)(*(const uint32_t*)(base + MXA_S_OFF + (32 * T + r) * 4) >> (8 * h));
                i32x8 kf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const u32x4 lo = *(const u32x4*)(kb + foff[i][0]), hi = *(const u32x4*)(kb + foff[i][1]);
                    kf[i] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
                }
                f32x16 sacc;
#pragma unroll
                for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
                sacc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf[0], qf[0], sacc, 0, 0, 0, ksc, 0, qsc);
                sacc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf[1], qf[1], sacc, 0, 0, 2, ksc, 2, qsc);
                if (masked) attn_mask_ragged(sacc, kv0, T, h, p.Lk);
                // ---- online softmax of the half: the bf16 kernels' (attn_args.h)
                bf16x8 pf[2];
                attn_softmax_half<false>(sacc, 0u, p.scale_log2, m_run, l_run, oacc, pf);
                // ---- O^T += V^T . P^T
#pragma unroll
                for (int d = 0; d < ND; ++d)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        const bf16x8 vf = *(const bf16x8*)(base + MXA_K_BYTES + d * 32 * 128 + foff[T][s2]);
                        oacc[d] = mfma_32x32x16<false>(vf, pf[s2], oacc[d]);
                    }
            }
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // this wave's share of tile t + 1 has landed; own LDS reads retired
        __builtin_amdgcn_s_barrier();
    }
    if (!compute_wave) return;

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    const int q = q0w + r;
    if ((p.ldo & 7) == 0) {
        // O through LDS: wave-private images over the stages (free: the last tile ended on a barrier every wave took)
        attn_store_lds(smem + wave_u * (32 * 144), p.out + (long)q0w * p.ldo + hcol, p.ldo, p.Lq - q0w, lane, oacc, inv);
    } else if (q < p.Lq) {
        attn_store_direct<false, ND>(p.out + (long)q * p.ldo + hcol + 4 * h, oacc, inv);
    }
}

__global__ __launch_bounds__(768) __attribute__((amdgpu_waves_per_eu(3, 3))) void flash_attn_mxqk12_kernel(AttnMxArgs p) {
    __shared__ __attribute__((aligned(16))) char smem[MXA_SMEM];
    mxqk_body<12>(p, smem);
}

__global__ __launch_bounds__(256) void flash_attn_mxqk4_kernel(AttnMxArgs p) {
    __shared__ __attribute__((aligned(16))) char smem[MXA_SMEM];
    mxqk_body<4>(p, smem);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
static void launch_attn_mxqk(AttnMxArgs a, const AttnPlan& plan, hipStream_t st) {
    a.q_blocks = plan.q_blocks;
    a.n12 = plan.n12;
    void (*kern)(AttnMxArgs) = plan.kernel == ATT_MXQK12 ? flash_attn_mxqk12_kernel : flash_attn_mxqk4_kernel;
    hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(plan.block), 0, st, a);
}

// The plan uv_flash_attn_mxqk launches for this problem on the current device (256 CUs without one) under the current UV_OPT_ATTN_CUT.
extern "C" int uv_flash_attn_mxqk_plan(int batch, int Lq, int Lk, int H, int head_dim, char* kernel, int len, int* q_blocks, int* n12, int* grid) {
    UV_CHECK_ARG(kernel && len > 0 && q_blocks && n12 && grid, "uv_flash_attn_mxqk_plan: null pointer");
    UV_CHECK_ARG(head_dim == 128, "uv_flash_attn_mxqk_plan: head_dim %d unsupported (128 only)", head_dim);
    UV_CHECK_ARG(Lq > 0 && Lk > 0 && H > 0 && batch > 0, "uv_flash_attn_mxqk_plan: bad shape B=%d Lq=%d Lk=%d H=%d", batch, Lq, Lk, H);
    const AttnPlan plan = plan_attn_mxqk(batch, Lq, Lk, H, uv_num_cus(), uv_option(UV_OPT_ATTN_CUT));
    snprintf(kernel, len, "%s", kAttnKernelName[plan.kernel]);
    *q_blocks = plan.q_blocks; *n12 = plan.n12; *grid = plan.grid;
    return 0;
}

extern "C" int uv_flash_attn_mxqk(const void* q_codes, long ldq, const void* q_scales, long ld_qs, const void* k_codes, long ldk,
                                  const void* k_scales, long ld_ks, const void* vt, long ldvt, void* out, long ldo, int batch, int Lq, int Lk,
                                  int H, int head_dim, float softmax_scale, void* stream) {
    const char* name = "uv_flash_attn_mxqk";
    UV_CHECK_ARG(q_codes && k_codes && vt && out, "%s: null pointer", name);
    UV_CHECK_ARG(q_scales && k_scales, "%s: null scale pointer", name);
    UV_CHECK_ARG(head_dim == 128, "%s: head_dim %d unsupported (128 only)", name, head_dim);
    UV_CHECK_ARG(Lq > 0 && Lk > 0 && H > 0 && batch > 0, "%s: bad shape B=%d Lq=%d Lk=%d H=%d", name, batch, Lq, Lk, H);
    UV_CHECK_ARG(ldq >= (long)H * 128 && ldk >= (long)H * 128 && ldq % 16 == 0 && ldk % 16 == 0,
                 "%s: ldq/ldk must be >= H * 128 and multiples of 16 bytes (ldq=%ld ldk=%ld)", name, ldq, ldk);
    UV_CHECK_ARG(ld_qs >= (long)H * 4 && ld_ks >= (long)H * 4 && ld_qs % 4 == 0 && ld_ks % 4 == 0,
                 "%s: ld_qs/ld_ks must be >= H * 4 = %d and multiples of 4 (ld_qs=%ld ld_ks=%ld)", name, H * 4, ld_qs, ld_ks);
    UV_CHECK_ARG(ldvt % 8 == 0 && ldo % 4 == 0, "%s: ldvt must be a multiple of 8, ldo of 4 elements", name);
    UV_CHECK_ARG(ldvt >= (long)(batch - 1) * Lk + (long)((Lk + 63) / 64) * 64,
                 "%s: ldvt=%ld must cover (batch-1)*Lk + Lk rounded up to 64 (batch=%d Lk=%d)", name, ldvt, batch, Lk);
    UV_CHECK_ARG(batch == 1 || Lk % 8 == 0, "%s: batch > 1 needs Lk %% 8 == 0 (Lk=%d)", name, Lk);
    UV_CHECK_ARG((((uintptr_t)q_codes | (uintptr_t)k_codes | (uintptr_t)vt | (uintptr_t)out) & 15) == 0,
                 "%s: codes / vt / out pointers must be 16-byte aligned", name);
    UV_CHECK_ARG((((uintptr_t)q_scales | (uintptr_t)k_scales) & 3) == 0, "%s: scale pointers must be 4-byte aligned", name);
    AttnMxArgs a;
    a.qc = (const uint8_t*)q_codes; a.qs = (const uint8_t*)q_scales; a.kc = (const uint8_t*)k_codes; a.ks = (const uint8_t*)k_scales;
    a.vt = (const bf16_t*)vt; a.out = (bf16_t*)out;
    a.ldq = ldq; a.ld_qs = ld_qs; a.ldk = ldk; a.ld_ks = ld_ks; a.ldvt = ldvt; a.ldo = ldo;
    a.Lq = Lq; a.Lk = Lk; a.H = H; a.batch = batch;
    a.scale_log2 = softmax_scale * 1.4426950408889634f;
    launch_attn_mxqk(a, plan_attn_mxqk(batch, Lq, Lk, H, uv_num_cus(), uv_option(UV_OPT_ATTN_CUT)), (hipStream_t)stream);
    UV_CHECK_LAUNCH(name);
    return 0;
}
