// Data-dependent key-tile lists for the block-sparse self-attention (attention_bs.hip) for gfx950: the opt-in top-k mode of the DiT
// (univid_amd.wan.attention.TopKBlockMask; Lq == Lk == L, head_dim 128, bf16, every sample attends all L keys).
//
// No counterpart in the reference. What is meant are the training-free sparse-attention schemes that choose, per forward, layer, head and
// sample, the key tiles that pooled q.k scores rank highest, beside a static local / sink neighbourhood. With QB = 128 queries, KB = 64 keys,
// nqb = ceil(L / 128), nkb = ceil(L / 64), per (sample b, head h):
//   qbar[i][:]  = fp32 mean of the q rows of query block i, kbar[j][:] = fp32 mean of the k rows of key tile j (a ragged last block / tile:
//                 the fp32 sum of its valid rows divided by their count) - of the q / k the attention kernel consumes (after RMSNorm + RoPE)
//   s[i][j]     = sum_d qbar[i][d] kbar[j][d] in fp32 (no softmax, no scale: the order of a row's scores does not depend on either)
//   list of i   = the tiles keep[h or 0][i][:] marks, plus the top_k best of the others under the total order (score descending, tile index
//                 ascending); fewer candidates than top_k: all of them. Written ascending by tile index - the ragged tile nkb - 1 can only
//                 be last, which flash_attn_bs4_kernel needs. keepcount + min(top_k, nkb - keepcount) >= 1 entries.
// Two kernels, both deterministic (no atomics, fixed order), all stores plain vector stores:
//   attn_pool_kernel     one workgroup per (sample, head, query block or key tile): 16-byte loads of the rows, 16 row lanes x 16 column
//                        chunks, each lane an fp32 running sum of its rows in ascending order, the 16 lanes' sums added in ascending lane
//                        order through LDS. q and k are read once.
//   attn_select_kernel   one workgroup per (sample, head, query block): the row's scores as 64-bit KEYS in LDS (high word: the score's bits
//                        mapped to an unsigned integer of the same order, -0 taken as +0; low word: ~tile index, so a tie goes to the lower
//                        index and no two keys are equal; 0: a kept tile or padding, below every candidate), the lane's own 16 keys kept
//                        in registers, an LDS bitonic sort (descending) of the keys, the top_k-th key as threshold, flags, and an ascending
//                        compaction by prefix sum over the workgroup. Whatever the scores hold (NaN, inf), the keys are a total order, so
//                        the list is valid: count in [1, nkb], entries in range, strictly ascending.
#include "common.h"
#include <stdio.h>

constexpr int UV_SEL_MAX_NKB = 4096;      // the LDS sort array: 4096 keys of 8 bytes
constexpr int UV_SEL_CHUNK = UV_SEL_MAX_NKB / 256;

struct AttnPoolArgs {
    const bf16_t* q;
    const bf16_t* k;
    float* qbar;      // [batch, H, nqb, 128]
    float* kbar;      // [batch, H, nkb, 128]
    long ldq, ldk;
    int L, H, nqb, nkb;
};

__global__ __launch_bounds__(256) void attn_pool_kernel(AttnPoolArgs p) {
    __shared__ float part[16][132];
    const int tid = threadIdx.x;
    const int c = tid & 15, rl = tid >> 4;
    const int nblk = p.nqb + p.nkb;
    const int blk = blockIdx.x % nblk;
    const int bh = blockIdx.x / nblk;
    const int head = bh % p.H, b = bh / p.H;
    const bool isq = blk < p.nqb;
    const int i = isq ? blk : blk - p.nqb;
    const int rows_per = isq ? 128 : 64;
    const int r0 = i * rows_per;
    const int nrows = min(rows_per, p.L - r0);                 // >= 1
    const long ld = isq ? p.ldq : p.ldk;
    const bf16_t* src = (isq ? p.q : p.k) + ((long)b * p.L + r0) * ld + (long)head * 128 + 8 * c;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int r = rl; r < nrows; r += 16) {
        const u32x4 v = *(const u32x4*)(src + (long)r * ld);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[2 * e] += bf2f((bf16_t)(v[e] & 0xffff));
            acc[2 * e + 1] += bf2f((bf16_t)(v[e] >> 16));
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[rl][8 * c + e] = acc[e];
    __syncthreads();
    if (tid < 128) {
        float s = part[0][tid];
#pragma unroll
        for (int l = 1; l < 16; ++l) s += part[l][tid];
        float* dst = isq ? p.qbar + (((long)b * p.H + head) * p.nqb + i) * 128 : p.kbar + (((long)b * p.H + head) * p.nkb + i) * 128;
        dst[tid] = s / (float)nrows;
    }
}

struct AttnSelArgs {
    const float* qbar;
    const float* kbar;
    const unsigned char* keep;      // [keep_heads, nqb, nkb] or null
    int* tile_idx;                  // [batch, H, nqb, nkb]
    int* tile_cnt;                  // [batch, H, nqb]
    int H, nqb, nkb, keep_heads, top_k, npow2;
};

__global__ __launch_bounds__(256) void attn_select_kernel(AttnSelArgs p) {
    __shared__ unsigned long long key[UV_SEL_MAX_NKB];
    __shared__ __attribute__((aligned(16))) float qs[128];
    __shared__ int wsum[4];
    const int tid = threadIdx.x;
    const int nkb = p.nkb, n2 = p.npow2;
    const int i = blockIdx.x % p.nqb;
    const int bh = blockIdx.x / p.nqb;
    const int head = bh % p.H;
    const long row = (long)bh * p.nqb + i;
    if (tid < 128) qs[tid] = p.qbar[row * 128 + tid];
    __syncthreads();

    // ---- scores -> keys. 16 lanes per tile: lane c holds columns 4c .. 4c+3 and 64 + 4c .. 64 + 4c + 3; the 16 partial sums are added by a
    // butterfly (every lane ends with the same bits: each step adds the same two values on both sides)
    const int c = tid & 15, g = tid >> 4;
    const f32x4 qa = *(const f32x4*)(qs + 4 * c), qb = *(const f32x4*)(qs + 64 + 4 * c);
    const float* kb0 = p.kbar + (long)bh * nkb * 128;
    const unsigned char* kp = p.keep ? p.keep + ((long)(p.keep_heads == 1 ? 0 : head) * p.nqb + i) * nkb : nullptr;
    for (int j0 = 0; j0 < n2; j0 += 16) {
        const int j = j0 + g;
        float s = 0.f;
        if (j < nkb) {
            const f32x4 ka = *(const f32x4*)(kb0 + (long)j * 128 + 4 * c), kb = *(const f32x4*)(kb0 + (long)j * 128 + 64 + 4 * c);
            s = qa[0] * ka[0];
            s += qa[1] * ka[1]; s += qa[2] * ka[2]; s += qa[3] * ka[3];
            s += qb[0] * kb[0]; s += qb[1] * kb[1]; s += qb[2] * kb[2]; s += qb[3] * kb[3];
        }
        s += __shfl_xor(s, 8, 64);
        s += __shfl_xor(s, 4, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 1, 64);
        if (c == 0 && j < n2) {
            unsigned long long kv = 0ull;
            if (j < nkb && !(kp && kp[j])) {
                unsigned u = __builtin_bit_cast(unsigned, s);
                if (u == 0x80000000u) u = 0u;                               // -0 ties with +0
                u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;                 // unsigned order == float order (NaNs at the two ends)
                kv = ((unsigned long long)u << 32) | (unsigned)~(unsigned)j;
            }
            key[j] = kv;
        }
    }
    __syncthreads();

    // ---- the lane's own tiles [16 tid, 16 tid + 16): keys into registers before the sort moves them
    unsigned long long mine[UV_SEL_CHUNK];
#pragma unroll
    for (int e = 0; e < UV_SEL_CHUNK; ++e) {
        const int j = UV_SEL_CHUNK * tid + e;
        mine[e] = j < nkb ? key[j] : 0ull;
    }
    __syncthreads();

    // ---- bitonic sort of key[0 .. n2), descending
    for (int k2 = 2; k2 <= n2; k2 <<= 1)
        for (int jj = k2 >> 1; jj > 0; jj >>= 1) {
            for (int pr = tid; pr < (n2 >> 1); pr += 256) {
                const int lo = ((pr & ~(jj - 1)) << 1) | (pr & (jj - 1)), hi = lo | jj;
                const unsigned long long a = key[lo], b = key[hi];
                const bool desc = (lo & k2) == 0;
                if (desc ? a < b : a > b) { key[lo] = b; key[hi] = a; }
            }
            __syncthreads();
        }
    // the top_k-th best key; 0: fewer candidates than top_k - all of them are listed
    const unsigned long long thr = key[min(p.top_k, n2) - 1];

    // ---- flags, ascending compaction
    unsigned flags = 0u;
#pragma unroll
    for (int e = 0; e < UV_SEL_CHUNK; ++e) {
        const int j = UV_SEL_CHUNK * tid + e;
        if (j < nkb) {
            const bool kept = mine[e] == 0ull;                              // a candidate's key is never 0
            if (kept || mine[e] >= thr) flags |= 1u << e;
        }
    }
    const int mycnt = __builtin_popcount(flags);
    int incl = mycnt;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int v = wsum[w];
        if (w < wave) base += v;
        total += v;
    }
    int pos = base + incl - mycnt;                                          // <= nkb - mycnt: one slot per flagged tile of the row
    int* out = p.tile_idx + row * nkb;
#pragma unroll
    for (int e = 0; e < UV_SEL_CHUNK; ++e)
        if ((flags >> e) & 1u) out[pos++] = UV_SEL_CHUNK * tid + e;
    if (tid == 0) p.tile_cnt[row] = total;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
extern "C" int uv_attn_pool_qk(const void* q, long ldq, const void* k, long ldk, void* qbar, void* kbar, int batch, int L, int H, int head_dim,
                               void* stream) {
    const char* name = "uv_attn_pool_qk";
    UV_CHECK_ARG(q && k && qbar && kbar, "%s: null pointer", name);
    UV_CHECK_ARG(head_dim == 128, "%s: head_dim %d unsupported (128 only)", name, head_dim);
    UV_CHECK_ARG(L > 0 && L <= (1 << 30) && H > 0 && batch > 0, "%s: bad shape B=%d L=%d H=%d", name, batch, L, H);
    UV_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldq >= (long)H * 128 && ldk >= (long)H * 128,
                 "%s: leading dimensions must be multiples of 8 elements and cover H*128 (ldq=%ld ldk=%ld)", name, ldq, ldk);
    UV_CHECK_ARG(batch == 1 || L % 8 == 0, "%s: batch > 1 needs L %% 8 == 0 (L=%d)", name, L);
    UV_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)qbar | (uintptr_t)kbar) & 15) == 0, "%s: pointers must be 16-byte aligned", name);
    AttnPoolArgs a;
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.qbar = (float*)qbar; a.kbar = (float*)kbar;
    a.ldq = ldq; a.ldk = ldk; a.L = L; a.H = H;
    a.nqb = (L + 127) / 128; a.nkb = (L + 63) / 64;
    const long grid = (long)(a.nqb + a.nkb) * H * batch;
    UV_CHECK_ARG(grid < (1L << 31), "%s: grid of %ld workgroups too large", name, grid);
    hipLaunchKernelGGL(attn_pool_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    UV_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int uv_attn_bs_select(const void* qbar, const void* kbar, const void* keep, int keep_heads, int top_k, int* tile_idx, int* tile_cnt,
                                 int batch, int L, int H, void* stream) {
    const char* name = "uv_attn_bs_select";
    UV_CHECK_ARG(qbar && kbar && tile_idx && tile_cnt, "%s: null pointer", name);
    UV_CHECK_ARG(L > 0 && L <= (1 << 30) && H > 0 && batch > 0, "%s: bad shape B=%d L=%d H=%d", name, batch, L, H);
    UV_CHECK_ARG(top_k >= 1, "%s: top_k=%d must be >= 1", name, top_k);
    UV_CHECK_ARG(keep_heads == 1 || keep_heads == H, "%s: keep_heads=%d must be 1 (one keep mask for all heads) or H=%d", name, keep_heads, H);
    const int nqb = (L + 127) / 128, nkb = (L + 63) / 64;
    UV_CHECK_ARG(nkb <= UV_SEL_MAX_NKB, "%s: %d key tiles (L=%d) exceed the %d the selection sorts in LDS", name, nkb, L, UV_SEL_MAX_NKB);
    UV_CHECK_ARG((((uintptr_t)qbar | (uintptr_t)kbar) & 15) == 0, "%s: qbar / kbar must be 16-byte aligned", name);
    UV_CHECK_ARG((((uintptr_t)tile_idx | (uintptr_t)tile_cnt) & 3) == 0, "%s: tile_idx / tile_cnt must be 4-byte aligned", name);
    AttnSelArgs a;
    a.qbar = (const float*)qbar; a.kbar = (const float*)kbar; a.keep = (const unsigned char*)keep;
    a.tile_idx = tile_idx; a.tile_cnt = tile_cnt;
    a.H = H; a.nqb = nqb; a.nkb = nkb; a.keep_heads = keep_heads; a.top_k = top_k;
    int n2 = 1;
    while (n2 < nkb) n2 <<= 1;
    a.npow2 = n2;
    const long grid = (long)nqb * H * batch;
    UV_CHECK_ARG(grid < (1L << 31), "%s: grid of %ld workgroups too large", name, grid);
    hipLaunchKernelGGL(attn_select_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    UV_CHECK_LAUNCH(name);
    return 0;
}
