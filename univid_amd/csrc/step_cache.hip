// Step cache of the denoise loop: on some sampler steps the DiT's block stack is not run, and its effect on the fp32 residual stream
// (r = x_out - x_in) is forecast from what it was on the steps that were run - a Taylor expansion in the step index over backward
// finite differences, as TaylorSeer does per module (models/BAGEL/modeling/cache_utils/taylorseer.py: derivative_approximation,
// taylor_formula), here once for the whole stack.
//
//   update (after the blocks of a computed step):  r = x_out - x_in;  n1 = (r - d0) / k;  n2 = (n1 - d1) / k;  d0 = r, d1 = n1, d2 = n2
//   apply  (instead of the blocks of a skipped step):  x += d0 + d1 * c1 + d2 * c2      (each term only while its buffer is valid)
//
// Both are one HBM pass: 16-byte loads and stores, a grid-stride loop, a scalar tail for n % 4. `have` (valid buffers), k, c1 and c2 are
// read from a 4-float table in device memory, so ONE captured HIP graph per kind serves every step; the branch on `have` is uniform.
// Every product, quotient, sum and difference is rounded to fp32 on its own (explicit round-to-nearest intrinsics; the file is built
// without contraction as well): the torch fp32 expressions give the same bits.
//
//   rows_rel_l1: out[i] = sum_j |rows[i+1][j] - rows[i][j]| / sum_j |rows[i][j]|, TeaCache's indicator over the time-embedding rows of
//   consecutive steps; fp64 sums in a fixed order (no atomics), one workgroup per pair.
#include "common.h"

#define SC_THREADS 256
#define SC_MAX_BLOCKS 2048

struct sc_ctl {
    int have;
    float k, c1, c2;
};
__device__ __forceinline__ sc_ctl sc_read_ctl(const float* ctl) {
    // every lane reads the same four words: the compiler keeps them uniform, the branches below do not diverge
    sc_ctl c;
    c.have = (int)ctl[0];
    c.k = ctl[1];
    c.c1 = ctl[2];
    c.c2 = ctl[3];
    return c;
}

// one element of the update; F1 / F2: the first / second difference is formed (uniform)
template <bool F1, bool F2> __device__ __forceinline__ void sc_update_one(float xo, float xi, float& d0, float& d1, float& d2, float k) {
    const float r = __fsub_rn(xo, xi);
    if (F1) {
        const float n1 = __fdiv_rn(__fsub_rn(r, d0), k);
        if (F2) d2 = __fdiv_rn(__fsub_rn(n1, d1), k);
        d1 = n1;
    }
    d0 = r;
}

template <bool F1, bool F2>
__device__ __forceinline__ void sc_update_body(const float* __restrict__ x_out, const float* __restrict__ x_in, float* d0, float* d1, float* d2,
                                               float k, long n, long nv) {
    const long stride = (long)gridDim.x * blockDim.x;
    const long t0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
    for (long i = t0; i < nv; i += stride) {
        const f32x4 xo = ((const f32x4*)x_out)[i], xi = ((const f32x4*)x_in)[i];
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a, c = a;
        if (F1) a = ((const f32x4*)d0)[i];
        if (F2) b = ((const f32x4*)d1)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a_ = a[e], b_ = b[e], c_ = 0.f;
            sc_update_one<F1, F2>(xo[e], xi[e], a_, b_, c_, k);
            a[e] = a_, b[e] = b_, c[e] = c_;
        }
        ((f32x4*)d0)[i] = a;
        if (F1) ((f32x4*)d1)[i] = b;
        if (F2) ((f32x4*)d2)[i] = c;
    }
    for (long i = nv * 4 + t0; i < n; i += stride) {       // n % 4 elements (all of them when a buffer is not 16-byte aligned)
        float a_ = F1 ? d0[i] : 0.f, b_ = F2 ? d1[i] : 0.f, c_ = 0.f;
        sc_update_one<F1, F2>(x_out[i], x_in[i], a_, b_, c_, k);
        d0[i] = a_;
        if (F1) d1[i] = b_;
        if (F2) d2[i] = c_;
    }
}

template <int ORDER>
__global__ void __launch_bounds__(SC_THREADS) step_cache_update_kernel(const float* __restrict__ x_out, const float* __restrict__ x_in, float* d0,
                                                                       float* d1, float* d2, const float* __restrict__ ctl, long n, long nv) {
    const sc_ctl c = sc_read_ctl(ctl);
    if (ORDER >= 2 && c.have >= 2) sc_update_body<true, true>(x_out, x_in, d0, d1, d2, c.k, n, nv);
    else if (ORDER >= 1 && c.have >= 1) sc_update_body<true, false>(x_out, x_in, d0, d1, d2, c.k, n, nv);
    else sc_update_body<false, false>(x_out, x_in, d0, d1, d2, c.k, n, nv);
}

// T1 / T2: the first / second difference takes part (uniform)
template <bool T1, bool T2> __device__ __forceinline__ float sc_apply_one(float x, float a, float b, float c, float c1, float c2) {
    float rh = a;
    if (T1) rh = __fadd_rn(rh, __fmul_rn(b, c1));
    if (T2) rh = __fadd_rn(rh, __fmul_rn(c, c2));
    return __fadd_rn(x, rh);
}

template <bool T1, bool T2>
__device__ __forceinline__ void sc_apply_body(float* x, const float* __restrict__ d0, const float* __restrict__ d1, const float* __restrict__ d2,
                                              float c1, float c2, long n, long nv) {
    const long stride = (long)gridDim.x * blockDim.x;
    const long t0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
    for (long i = t0; i < nv; i += stride) {
        f32x4 v = ((const f32x4*)x)[i];
        const f32x4 a = ((const f32x4*)d0)[i];
        f32x4 b = {0.f, 0.f, 0.f, 0.f}, c = b;
        if (T1) b = ((const f32x4*)d1)[i];
        if (T2) c = ((const f32x4*)d2)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = sc_apply_one<T1, T2>(v[e], a[e], b[e], c[e], c1, c2);
        ((f32x4*)x)[i] = v;
    }
    for (long i = nv * 4 + t0; i < n; i += stride)
        x[i] = sc_apply_one<T1, T2>(x[i], d0[i], T1 ? d1[i] : 0.f, T2 ? d2[i] : 0.f, c1, c2);
}

template <int ORDER>
__global__ void __launch_bounds__(SC_THREADS) step_cache_apply_kernel(float* x, const float* __restrict__ d0, const float* __restrict__ d1,
                                                                      const float* __restrict__ d2, const float* __restrict__ ctl, long n, long nv) {
    const sc_ctl c = sc_read_ctl(ctl);
    if (ORDER >= 2 && c.have >= 3) sc_apply_body<true, true>(x, d0, d1, d2, c.c1, c.c2, n, nv);
    else if (ORDER >= 1 && c.have >= 2) sc_apply_body<true, false>(x, d0, d1, d2, c.c1, c.c2, n, nv);
    else sc_apply_body<false, false>(x, d0, d1, d2, c.c1, c.c2, n, nv);
}

static inline bool sc_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline int sc_blocks(long n, long nv) {
    const long work = nv > 0 ? nv : n;
    long b = (work + SC_THREADS - 1) / SC_THREADS;
    return (int)(b < 1 ? 1 : (b > SC_MAX_BLOCKS ? SC_MAX_BLOCKS : b));
}

extern "C" int uv_step_cache_update(const float* x_out, const float* x_in, float* d0, float* d1, float* d2, const float* ctl, long n, int order,
                                    void* stream) {
    UV_CHECK_ARG(x_out && x_in && d0 && ctl && n > 0, "uv_step_cache_update: bad arguments");
    UV_CHECK_ARG(order >= 0 && order <= 2, "uv_step_cache_update: order %d is not 0, 1 or 2", order);
    UV_CHECK_ARG((order < 1 || d1) && (order < 2 || d2), "uv_step_cache_update: order %d needs d1%s", order, order == 2 ? " and d2" : "");
    const bool vec = sc_aligned16(x_out) && sc_aligned16(x_in) && sc_aligned16(d0) && (order < 1 || sc_aligned16(d1)) && (order < 2 || sc_aligned16(d2));
    const long nv = vec ? n / 4 : 0;
    const dim3 grid(sc_blocks(n, nv)), block(SC_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (order == 2) hipLaunchKernelGGL(step_cache_update_kernel<2>, grid, block, 0, s, x_out, x_in, d0, d1, d2, ctl, n, nv);
    else if (order == 1) hipLaunchKernelGGL(step_cache_update_kernel<1>, grid, block, 0, s, x_out, x_in, d0, d1, (float*)nullptr, ctl, n, nv);
    else hipLaunchKernelGGL(step_cache_update_kernel<0>, grid, block, 0, s, x_out, x_in, d0, (float*)nullptr, (float*)nullptr, ctl, n, nv);
    UV_CHECK_LAUNCH("uv_step_cache_update");
    return 0;
}

extern "C" int uv_step_cache_apply(float* x, const float* d0, const float* d1, const float* d2, const float* ctl, long n, int order, void* stream) {
    UV_CHECK_ARG(x && d0 && ctl && n > 0, "uv_step_cache_apply: bad arguments");
    UV_CHECK_ARG(order >= 0 && order <= 2, "uv_step_cache_apply: order %d is not 0, 1 or 2", order);
    UV_CHECK_ARG((order < 1 || d1) && (order < 2 || d2), "uv_step_cache_apply: order %d needs d1%s", order, order == 2 ? " and d2" : "");
    const bool vec = sc_aligned16(x) && sc_aligned16(d0) && (order < 1 || sc_aligned16(d1)) && (order < 2 || sc_aligned16(d2));
    const long nv = vec ? n / 4 : 0;
    const dim3 grid(sc_blocks(n, nv)), block(SC_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (order == 2) hipLaunchKernelGGL(step_cache_apply_kernel<2>, grid, block, 0, s, x, d0, d1, d2, ctl, n, nv);
    else if (order == 1) hipLaunchKernelGGL(step_cache_apply_kernel<1>, grid, block, 0, s, x, d0, d1, (const float*)nullptr, ctl, n, nv);
    else hipLaunchKernelGGL(step_cache_apply_kernel<0>, grid, block, 0, s, x, d0, (const float*)nullptr, (const float*)nullptr, ctl, n, nv);
    UV_CHECK_LAUNCH("uv_step_cache_apply");
    return 0;
}

// One workgroup per pair of consecutive rows. Thread t sums columns t, t + 256, ... in fp64; the 64 lanes of a wave combine through the
// xor butterfly and the four waves in wave order: the order of the additions is a function of K alone.
__global__ void __launch_bounds__(SC_THREADS) rows_rel_l1_kernel(const float* __restrict__ rows, float* __restrict__ out, int K) {
    __shared__ double part[2][SC_THREADS / UV_WAVE];
    const float* a = rows + (long)blockIdx.x * K;
    const float* b = a + K;
    double num = 0.0, den = 0.0;
    for (int j = threadIdx.x; j < K; j += SC_THREADS) {
        const double u = (double)a[j], v = (double)b[j];
        num += fabs(v - u);
        den += fabs(u);
    }
    num = wave_sum_d(num);
    den = wave_sum_d(den);
    if ((threadIdx.x & (UV_WAVE - 1)) == 0) {
        part[0][threadIdx.x / UV_WAVE] = num;
        part[1][threadIdx.x / UV_WAVE] = den;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sn = part[0][0], sd = part[1][0];
        for (int w = 1; w < SC_THREADS / UV_WAVE; ++w) sn += part[0][w], sd += part[1][w];
        out[blockIdx.x] = (float)(sn / sd);
    }
}

extern "C" int uv_rows_rel_l1(const float* rows, float* out, int n_rows, int K, void* stream) {
    UV_CHECK_ARG(rows && out && n_rows >= 2 && K > 0, "uv_rows_rel_l1: bad arguments (n_rows %d, K %d)", n_rows, K);
    hipLaunchKernelGGL(rows_rel_l1_kernel, dim3(n_rows - 1), dim3(SC_THREADS), 0, (hipStream_t)stream, rows, out, K);
    UV_CHECK_LAUNCH("uv_rows_rel_l1");
    return 0;
}
