// Flash attention forward with MXFP8 q / k AND an MXFP8 P.V (format: include/univid_hip.h), bf16 output, head_dim 128, for gfx950: the opt-in
// "mxfp8_qk_pv" mode of the DiT's self-attention (WanModel.set_attn_precision). The second half of attention_mx.hip's mode.
//
// Replaces: flash_attention()  models/wan/utils/modules/attention.py:24-130 as called from WanSelfAttention.forward model.py:145-150 - with q, k, v
//           and the softmax weights NARROWER than the reference's bf16 (3 mantissa bits each).
//
// S^T = K.Q^T is attention_mx.hip's, instruction for instruction (same operands, same single chain per S element). O^T += V^T.P^T runs on the same
// block-scaled instruction v_mfma_scale_f32_32x32x64_f8f6f4: ONE instruction per 32 head-dim channels and 64-key tile (four per tile) in place of
// sixteen bf16 32x32x16 ones, on 64-byte V^T code rows (8 KiB per tile instead of 16 KiB of bf16).
//   A = V^T codes: rows = channels 32 d + r, the 64 keys of the tile along K; MX block b = the tile's key half b, its scale byte = op_sel d of the dword
//       lane (r, h = b) passes (the tile's scales are staged so that lane l's dword holds its four bytes: no shift, no shuffle).
//   B = P codes: e4m3(P 2^PSHIFT) with the constant scale byte 127 - PSHIFT. The S accumulator of key half T holds, in lane (r, h) register e, the
//       score of query r against LDS key row 32 T + (e & 3) + 8 (e >> 2) + 4 h = key 32 T + (e & 7) + 8 h + 16 (e >> 3) of the tile. The lane's sixteen
//       values are packed in register order (byte e of register half T), i.e. at K index 32 T + 16 h + e (the lane map at the top of attention_mx.hip):
//       key kappa of a 32-key block sits at K index perm34(kappa) (bits 3 and 4 swapped). uv_vt_mx_quant stores V^T in that order, so the A fragment
//       is two plain 16-byte LDS reads.
// The reference maximum is reconsidered once per 64-key tile and PER QUERY: a query moves its own maximum when one of the tile's scores would give
// P > 2^DEFER_PV (the rescale runs when any lane moves; the others multiply by exactly 1), so a query's bits depend on nothing but its own row
// and the keys - not on the kernel size, the cut, the batch or its neighbours. DEFER_PV + PSHIFT = 8: the largest code is 256 < 448. l sums the
// unrounded f32 P.
//
// One kernel body in two sizes, as attention_mx.hip: flash_attn_mxpv12_kernel (Lk >= 2048; 12 waves, 12 / 8 unit cut, XCD order, loader-only
// waves) and flash_attn_mxpv4_kernel; plan_attn_mxpv (attn_args.h) decides. A staged tile = 64 keys: K codes [64][128 B] as attention_mx.hip,
// V^T codes [128][64 B] (16-byte chunk ^= (row >> 2) & 3: the four 16-lane groups of a 16-byte LDS read each cover all 64 banks), the K scale
// dwords and the V scale dwords (256 B each, one 4-byte LDS-DMA per lane of one wave). 16 one-KiB pieces per tile dealt round-robin over the
// waves; tiles double-buffered, one vmcnt(0) + barrier per tile, one generic tile form.
#include "attn_args.h"
#include <stdio.h>

typedef __attribute__((address_space(3))) void lds_void_a;
typedef __attribute__((ext_vector_type(8))) int i32x8;

struct AttnMxPvArgs {
    const uint8_t* qc;   // [batch * Lq, ldq] e4m3 codes, head h at byte h * 128
    const uint8_t* qs;   // [batch * Lq, ld_qs] e8m0 bytes, head h at byte h * 4
    const uint8_t* kc;   // [batch * Lk, ldk]
    const uint8_t* ks;   // [batch * Lk, ld_ks]
    const uint8_t* vc;   // [H * 128, ldvc] V^T codes, sample b at columns b * Lkp, keys permuted inside each 32-key block
    const uint8_t* vs;   // [H, ld_vs] V^T scale bytes, 256 per (sample, 64-key tile)
    bf16_t* out;         // [batch * Lq, ldo]
    long ldq, ld_qs, ldk, ld_ks, ldvc, ld_vs, ldo;
    int Lq, Lk, Lkp, H, q_blocks, batch, n12;
    float scale_log2;
};

constexpr int MXP_K_BYTES = UV_ATT_KV * 128;          // 8 KiB of K codes
constexpr int MXP_V_BYTES = 128 * UV_ATT_KV;          // 8 KiB of V^T codes
constexpr int MXP_KS_OFF = MXP_K_BYTES + MXP_V_BYTES; // the tile's 64 K scale dwords
constexpr int MXP_VS_OFF = MXP_KS_OFF + UV_ATT_KV * 4;  // the tile's 64 V scale dwords (one per lane)
constexpr int MXP_STAGE = MXP_VS_OFF + 256;
constexpr int MXP_PIECES = (MXP_K_BYTES + MXP_V_BYTES) / 1024;   // 8 of K, then 8 of V^T: piece pc lands at stage + 1024 pc
constexpr int MXP_PSCALE = (127 - UV_ATT_PSHIFT) * 0x01010101;   // the scale byte of P, whatever byte op_sel names
// the O epilogue's wave-private images (32 rows x 144 B per wave) lie over the stages
constexpr int mxp_smem(int nw) { return 2 * MXP_STAGE > nw * 32 * 144 ? 2 * MXP_STAGE : nw * 32 * 144; }

template <int NW>
__device__ __forceinline__ void mxpv_body(AttnMxPvArgs p, char* smem) {
    constexpr int ND = 4, NP = (MXP_PIECES + NW - 1) / NW;
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
    {   // independent samples: rows of q / k / out (codes and scales alike), padded column ranges of the V^T codes, tile ranges of its scales
        const long b = bh / p.H;
        p.qc += b * p.Lq * p.ldq;  p.qs += b * p.Lq * p.ld_qs;
        p.kc += b * p.Lk * p.ldk;  p.ks += b * p.Lk * p.ld_ks;
        p.vc += b * p.Lkp;
        p.vs += head * p.ld_vs + b * p.Lkp * 4;
        p.out += b * p.Lq * p.ldo;
    }
    const long hcol = (long)head * 128;

    // ---- Q fragments (B operand of S^T), as attention_mx.hip
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

    // ---- staging: this wave's pieces (piece pc = wave + NW i, pc < 16) and, on the last two waves, the tile's K / V scale dwords
    const char* pbase[NP];      // the piece's source of tile 0 without the key-row term (K) / at the sample's key column 0 (V^T)
    int pkrow[NP];              // K pieces: the key row (inside the tile) this lane's LDS row holds
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int pc = wave_u + NW * i;
        if (pc < 8) {
            const int lrow = 8 * pc + (lane >> 3);
            pkrow[i] = perm23(lrow);
            pbase[i] = (const char*)p.kc + hcol + (((lane & 7) ^ ((lrow >> 1) & 7)) << 4);
        } else {                // 16 channel rows of 64 bytes; (row >> 2) & 3 == (lane >> 4) & 3
            const int drow = 16 * (pc - 8) + (lane >> 2);
            pkrow[i] = 0;
            pbase[i] = (const char*)p.vc + (hcol + drow) * p.ldvc + (((lane & 3) ^ ((lane >> 4) & 3)) << 4);
        }
    }
    const int sc_krow = perm23(lane);
    const uint8_t* const sc_base = p.ks + head * 4;
    auto fetch = [&](int t, int buf) {      // K rows at Lk and beyond are never read (clamped); V^T is padded to whole tiles by its producer
        char* stage = smem + buf * MXP_STAGE;
        const int kv0 = t * UV_ATT_KV;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int pc = wave_u + NW * i;
            if (pc < MXP_PIECES) {
                const char* src = pc < 8 ? pbase[i] + (long)min(kv0 + pkrow[i], p.Lk - 1) * p.ldk : pbase[i] + kv0;
                __builtin_amdgcn_global_load_lds(src, (lds_void_a*)(stage + pc * 1024), 16, 0, 0);
            }
        }
        if (wave_u == NW - 1)
            __builtin_amdgcn_global_load_lds(sc_base + (long)min(kv0 + sc_krow, p.Lk - 1) * p.ld_ks, (lds_void_a*)(stage + MXP_KS_OFF), 4, 0, 0);
        if (wave_u == NW - 2)
            __builtin_amdgcn_global_load_lds(p.vs + (long)t * 256 + lane * 4, (lds_void_a*)(stage + MXP_VS_OFF), 4, 0, 0);
    };

    // fragment read offsets inside a stage
    //   K  : row 32 T + r of 128 B, step i, register half s: logical chunk 4 i + 2 s + h, physical ^= (r >> 1) & 7
    //   V^T: row 32 d + r of 64 B, register half (= key half = MX block) b: logical chunk 2 b + h, physical ^= (r >> 2) & 3
    int foff[2][2], voff[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int s = 0; s < 2; ++s) foff[a][s] = r * 128 + (((4 * a + 2 * s + h) ^ ((r >> 1) & 7)) << 4);
        voff[a] = MXP_K_BYTES + r * 64 + (((2 * a + h) ^ ((r >> 2) & 3)) << 4);
    }

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
        const char* base = smem + (t & 1) * MXP_STAGE;
        if (t + 1 < nt) fetch(t + 1, (t + 1) & 1);       // the other stage: last read in tile t - 1, fenced by its barrier
        if (compute_wave) {
            const int kv0 = t * UV_ATT_KV;
            const bool masked = t >= nt_full;
            // ---- S^T: two halves of 32 keys x 32 queries, two block-scaled steps each into one accumulator (attention_mx.hip's chain)
            f32x16 sacc[2];
#pragma unroll
            for (int T = 0; T < 2; ++T) {
                const char* kb = base + T * 32 * 128;
                const int ksc = (int)(*(const uint32_t*)(base + MXP_KS_OFF + (32 * T + r) * 4) >> (8 * h));
                i32x8 kf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const u32x4 lo = *(const u32x4*)(kb + foff[i][0]), hi = *(const u32x4*)(kb + foff[i][1]);
                    kf[i] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) sacc[T][e] = 0.f;
                sacc[T] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf[0], qf[0], sacc[T], 0, 0, 0, ksc, 0, qsc);
                sacc[T] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf[1], qf[1], sacc[T], 0, 0, 2, ksc, 2, qsc);
                if (masked) {      // its own copy of attn_mask_ragged (attn_args.h): through the shared one flash_attn_mxpv4_kernel takes 248 registers for 244
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int i = 32 * T + (e & 3) + 8 * (e >> 2) + 4 * h;
                        if (kv0 + perm23(i) >= p.Lk) sacc[T][e] = -INFINITY;
                    }
                }
            }
            // ---- the tile's maximum per query, and the query's own decision to move its reference
            float mt = fmaxf(sacc[0][0], sacc[1][0]);
#pragma unroll
            for (int e = 1; e < 16; ++e) mt = fmaxf(mt, fmaxf(sacc[0][e], sacc[1][e]));
            {
                const unsigned u = __builtin_bit_cast(unsigned, mt);
                const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
                mt = fmaxf(__builtin_bit_cast(float, (unsigned)sw[0]), __builtin_bit_cast(float, (unsigned)sw[1]));
            }
            const bool move = (mt - m_run) * p.scale_log2 > (float)UV_ATT_DEFER_PV;
            if (__any(move)) {
                const float m_new = move ? fmaxf(m_run, mt) : m_run;
                const float alpha = move ? __builtin_amdgcn_exp2f((m_run - m_new) * p.scale_log2) : 1.0f;
                l_run *= alpha;
#pragma unroll
                for (int d = 0; d < ND; ++d)
#pragma unroll
                    for (int e = 0; e < 16; ++e) oacc[d][e] *= alpha;
                m_run = m_new;
            }
            // ---- P = exp2(s - m) in f32 (summed unrounded), its e4m3 codes of P 2^PSHIFT in register order: key half T = register half T = MX block T
            const float mneg = -m_run * p.scale_log2;
            float psum = 0.f;
            i32x8 pf;
#pragma unroll
            for (int T = 0; T < 2; ++T)
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    float pv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        pv[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[T][4 * w + j], p.scale_log2, mneg));
                        psum += pv[j];
                        pv[j] *= (float)(1 << UV_ATT_PSHIFT);
                    }
                    int pk = __builtin_amdgcn_cvt_pk_fp8_f32(pv[0], pv[1], 0, false);
                    pf[4 * T + w] = __builtin_amdgcn_cvt_pk_fp8_f32(pv[2], pv[3], pk, true);
                }
            l_run += psum;
            // ---- O^T += V^T . P^T: one block-scaled instruction per 32 channels
            const int vsc = (int)*(const uint32_t*)(base + MXP_VS_OFF + lane * 4);
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const u32x4 lo = *(const u32x4*)(base + d * 32 * 64 + voff[0]), hi = *(const u32x4*)(base + d * 32 * 64 + voff[1]);
                const i32x8 vf = {(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
                if (d == 0) oacc[0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf, pf, oacc[0], 0, 0, 0, vsc, 0, MXP_PSCALE);
                if (d == 1) oacc[1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf, pf, oacc[1], 0, 0, 1, vsc, 0, MXP_PSCALE);
                if (d == 2) oacc[2] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf, pf, oacc[2], 0, 0, 2, vsc, 0, MXP_PSCALE);
                if (d == 3) oacc[3] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf, pf, oacc[3], 0, 0, 3, vsc, 0, MXP_PSCALE);
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
        // O through LDS: its own copy of attn_store_lds (attn_args.h) over the stages (free: the last tile ended on a barrier every wave took).
        // Through the shared one flash_attn_mxpv12_kernel measured 2 086 - 2 095 us for 2 051 - 2 054 (L = 11 440, B 2; profiles/attn_shared_pieces.md)
        constexpr int RS = 144;
        char* const img = smem + wave_u * (32 * RS);
        const int srow = lane >> 3, chunk = lane & 7;
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
                if (q0w + row < p.Lq) *(u32x4*)(p.out + (long)(q0w + row) * p.ldo + hcol + 64 * half + chunk * 8) = v[i];
            }
        }
    } else if (q < p.Lq) {
        attn_store_direct<false, ND>(p.out + (long)q * p.ldo + hcol + 4 * h, oacc, inv);
    }
}

__global__ __launch_bounds__(768) __attribute__((amdgpu_waves_per_eu(3, 3))) void flash_attn_mxpv12_kernel(AttnMxPvArgs p) {
    __shared__ __attribute__((aligned(16))) char smem[mxp_smem(12)];
    mxpv_body<12>(p, smem);
}

__global__ __launch_bounds__(256) void flash_attn_mxpv4_kernel(AttnMxPvArgs p) {
    __shared__ __attribute__((aligned(16))) char smem[mxp_smem(4)];
    mxpv_body<4>(p, smem);
}

// ---- the V^T quantiser ----------------------------------------------------------------------------------------------------------------------
// One lane = 8 consecutive keys of one (channel row, sample) (one 16-byte load, one 8-byte store), four lanes = one MX block. Keys at Lk and
// beyond count as zero and are not read when the whole group lies there; a block that holds no key at all gets the scale byte 127. The
// quantisation is uv_mx_quant_bf16's (gemm_mx.hip), operation for operation.
__global__ __launch_bounds__(256) void vt_mx_quant_kernel(const bf16_t* __restrict__ vt, long ldvt, uint8_t* __restrict__ codes, long ldvc,
                                                          uint8_t* __restrict__ scales, long ld_vs, int Lk, int Lkp, int batch, long total) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = t < total;             // (whole groups of 4 lanes are inside or outside: Lkp / 8 is a multiple of 8)
    const int g8 = Lkp >> 3;
    const long per_row = (long)batch * g8;
    const long row = live ? t / per_row : 0;
    const int rem = live ? (int)(t - row * per_row) : 0;
    const int b = rem / g8, c8 = rem - b * g8, k0 = 8 * c8;
    u32x4 in = {0u, 0u, 0u, 0u};
    if (live && k0 < Lk) in = *(const u32x4*)(vt + row * ldvt + (long)b * Lk + k0);
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[2 * e] = k0 + 2 * e < Lk ? __builtin_bit_cast(float, in[e] << 16) : 0.f;
        v[2 * e + 1] = k0 + 2 * e + 1 < Lk ? __builtin_bit_cast(float, in[e] & 0xffff0000u) : 0.f;
    }
    uint32_t amax = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = max(amax, __builtin_bit_cast(uint32_t, v[e]) & 0x7fffffffu);
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1, 64));
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2, 64));
    const int eb = max((int)(amax >> 23) - 8, 0);
    const float inv = __builtin_bit_cast(float, (uint32_t)(254 - eb) << 23);
    uint32_t w[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        float s[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = fminf(fmaxf(__fmul_rn(v[4 * e + i], inv), -448.f), 448.f);      // exact scaling, explicit clamp
        int pk = __builtin_amdgcn_cvt_pk_fp8_f32(s[0], s[1], 0, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(s[2], s[3], pk, true);
        w[e] = (uint32_t)pk;
    }
    if (!live) return;
    const int g = c8 & 3, blk = c8 >> 2;     // key group g of the block lands at group perm34's: bits 0 and 1 of g swapped
    *(u32x2*)(codes + row * ldvc + (long)b * Lkp + 32 * blk + 8 * (((g & 1) << 1) | (g >> 1))) = (u32x2){w[0], w[1]};
    if (g == 0) {
        const int head = (int)(row >> 7), ch = (int)(row & 127);
        scales[head * ld_vs + ((long)b * (Lkp >> 6) + (blk >> 1)) * 256 + 4 * ((ch & 31) + 32 * (blk & 1)) + (ch >> 5)] =
            (uint8_t)(32 * blk < Lk ? eb : 127);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
extern "C" int uv_vt_mx_quant(const void* vt, long ldvt, void* vt_codes, long ldvc, void* vt_scales, long ld_vs, int batch, int Lk, int H,
                              int head_dim, void* stream) {
    const char* name = "uv_vt_mx_quant";
    UV_CHECK_ARG(vt && vt_codes && vt_scales, "%s: null pointer", name);
    UV_CHECK_ARG(head_dim == 128, "%s: head_dim %d unsupported (128 only)", name, head_dim);
    UV_CHECK_ARG(Lk > 0 && H > 0 && batch > 0, "%s: bad shape B=%d Lk=%d H=%d", name, batch, Lk, H);
    const long Lkp = (long)((Lk + 63) / 64) * 64;
    UV_CHECK_ARG(batch * Lkp < (1L << 28), "%s: batch * roundup(Lk, 64) = %ld keys are not supported", name, batch * Lkp);
    UV_CHECK_ARG(batch == 1 || Lk % 8 == 0, "%s: batch > 1 needs Lk %% 8 == 0 (Lk=%d)", name, Lk);
    UV_CHECK_ARG(ldvt % 8 == 0 && ldvt >= (long)(batch - 1) * Lk + (long)((Lk + 7) / 8) * 8,
                 "%s: ldvt=%ld must be a multiple of 8 and cover (batch-1)*Lk + Lk rounded up to 8 (batch=%d Lk=%d)", name, ldvt, batch, Lk);
    UV_CHECK_ARG(ldvc % 16 == 0 && ldvc >= batch * Lkp, "%s: ldvc=%ld must be a multiple of 16 and >= batch * roundup(Lk, 64) = %ld", name, ldvc,
                 batch * Lkp);
    UV_CHECK_ARG(ld_vs % 4 == 0 && ld_vs >= batch * Lkp * 4, "%s: ld_vs=%ld must be a multiple of 4 and >= batch * roundup(Lk, 64) * 4 = %ld", name,
                 ld_vs, batch * Lkp * 4);
    UV_CHECK_ARG((((uintptr_t)vt | (uintptr_t)vt_codes) & 15) == 0, "%s: vt / vt_codes pointers must be 16-byte aligned", name);
    UV_CHECK_ARG(((uintptr_t)vt_scales & 3) == 0, "%s: vt_scales must be 4-byte aligned", name);
    const long total = (long)H * 128 * batch * (Lkp / 8);
    const long blocks = (total + 255) / 256;
    UV_CHECK_ARG(blocks <= 0x7fffffffL, "%s: too many elements (B=%d Lk=%d H=%d)", name, batch, Lk, H);
    hipLaunchKernelGGL(vt_mx_quant_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)vt, ldvt, (uint8_t*)vt_codes,
                       ldvc, (uint8_t*)vt_scales, ld_vs, Lk, (int)Lkp, batch, total);
    UV_CHECK_LAUNCH(name);
    return 0;
}

static void launch_attn_mxpv(AttnMxPvArgs a, const AttnPlan& plan, hipStream_t st) {
    a.q_blocks = plan.q_blocks;
    a.n12 = plan.n12;
    void (*kern)(AttnMxPvArgs) = plan.kernel == ATT_MXPV12 ? flash_attn_mxpv12_kernel : flash_attn_mxpv4_kernel;
    hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(plan.block), 0, st, a);
}

// The plan uv_flash_attn_mxpv launches for this problem on the current device (256 CUs without one) under the current UV_OPT_ATTN_CUT.
extern "C" int uv_flash_attn_mxpv_plan(int batch, int Lq, int Lk, int H, int head_dim, char* kernel, int len, int* q_blocks, int* n12, int* grid) {
    UV_CHECK_ARG(kernel && len > 0 && q_blocks && n12 && grid, "uv_flash_attn_mxpv_plan: null pointer");
    UV_CHECK_ARG(head_dim == 128, "uv_flash_attn_mxpv_plan: head_dim %d unsupported (128 only)", head_dim);
    UV_CHECK_ARG(Lq > 0 && Lk > 0 && H > 0 && batch > 0, "uv_flash_attn_mxpv_plan: bad shape B=%d Lq=%d Lk=%d H=%d", batch, Lq, Lk, H);
    const AttnPlan plan = plan_attn_mxpv(batch, Lq, Lk, H, uv_num_cus(), uv_option(UV_OPT_ATTN_CUT));
    snprintf(kernel, len, "%s", kAttnKernelName[plan.kernel]);
    *q_blocks = plan.q_blocks; *n12 = plan.n12; *grid = plan.grid;
    return 0;
}

extern "C" int uv_flash_attn_mxpv(const void* q_codes, long ldq, const void* q_scales, long ld_qs, const void* k_codes, long ldk,
                                  const void* k_scales, long ld_ks, const void* vt_codes, long ldvc, const void* vt_scales, long ld_vs, void* out,
                                  long ldo, int batch, int Lq, int Lk, int H, int head_dim, float softmax_scale, void* stream) {
    const char* name = "uv_flash_attn_mxpv";
    UV_CHECK_ARG(q_codes && k_codes && vt_codes && out, "%s: null pointer", name);
    UV_CHECK_ARG(q_scales && k_scales && vt_scales, "%s: null scale pointer", name);
    UV_CHECK_ARG(head_dim == 128, "%s: head_dim %d unsupported (128 only)", name, head_dim);
    UV_CHECK_ARG(Lq > 0 && Lk > 0 && H > 0 && batch > 0, "%s: bad shape B=%d Lq=%d Lk=%d H=%d", name, batch, Lq, Lk, H);
    UV_CHECK_ARG(ldq >= (long)H * 128 && ldk >= (long)H * 128 && ldq % 16 == 0 && ldk % 16 == 0,
                 "%s: ldq/ldk must be >= H * 128 and multiples of 16 bytes (ldq=%ld ldk=%ld)", name, ldq, ldk);
    UV_CHECK_ARG(ld_qs >= (long)H * 4 && ld_ks >= (long)H * 4 && ld_qs % 4 == 0 && ld_ks % 4 == 0,
                 "%s: ld_qs/ld_ks must be >= H * 4 = %d and multiples of 4 (ld_qs=%ld ld_ks=%ld)", name, H * 4, ld_qs, ld_ks);
    const long Lkp = (long)((Lk + 63) / 64) * 64;
    UV_CHECK_ARG(batch * Lkp < (1L << 28), "%s: batch * roundup(Lk, 64) = %ld keys are not supported", name, batch * Lkp);
    UV_CHECK_ARG(ldvc % 16 == 0 && ldvc >= batch * Lkp, "%s: ldvc=%ld must be a multiple of 16 and >= batch * roundup(Lk, 64) = %ld", name, ldvc,
                 batch * Lkp);
    UV_CHECK_ARG(ld_vs % 4 == 0 && ld_vs >= batch * Lkp * 4, "%s: ld_vs=%ld must be a multiple of 4 and >= batch * roundup(Lk, 64) * 4 = %ld", name,
                 ld_vs, batch * Lkp * 4);
    UV_CHECK_ARG(ldo % 4 == 0, "%s: ldo must be a multiple of 4 elements", name);
    UV_CHECK_ARG((((uintptr_t)q_codes | (uintptr_t)k_codes | (uintptr_t)vt_codes | (uintptr_t)out) & 15) == 0,
                 "%s: codes / out pointers must be 16-byte aligned", name);
    UV_CHECK_ARG((((uintptr_t)q_scales | (uintptr_t)k_scales | (uintptr_t)vt_scales) & 3) == 0, "%s: scale pointers must be 4-byte aligned", name);
    AttnMxPvArgs a;
    a.qc = (const uint8_t*)q_codes; a.qs = (const uint8_t*)q_scales; a.kc = (const uint8_t*)k_codes; a.ks = (const uint8_t*)k_scales;
    a.vc = (const uint8_t*)vt_codes; a.vs = (const uint8_t*)vt_scales; a.out = (bf16_t*)out;
    a.ldq = ldq; a.ld_qs = ld_qs; a.ldk = ldk; a.ld_ks = ld_ks; a.ldvc = ldvc; a.ld_vs = ld_vs; a.ldo = ldo;
    a.Lq = Lq; a.Lk = Lk; a.Lkp = (int)Lkp; a.H = H; a.batch = batch;
    a.scale_log2 = softmax_scale * 1.4426950408889634f;
    launch_attn_mxpv(a, plan_attn_mxpv(batch, Lq, Lk, H, uv_num_cus(), uv_option(UV_OPT_ATTN_CUT)), (hipStream_t)stream);
    UV_CHECK_LAUNCH(name);
    return 0;
}
