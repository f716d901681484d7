// The VAE convolution kernels' shared host and device pieces (conv3d_f32.hip: gather kernel, every geometry; conv3d_halo.hip /
// conv3d_halo16.hip: LDS-halo kernels for the 3x3(x3) stride-1 convolutions): the argument block, plan_conv - the ONE place that decides
// which of the 23 kernels runs a call and on what grid -, the launch helper, and the device code the kernels have in common.
#pragma once
#include "common.h"

struct ConvArgs {
    const float* in;     // [Tin, Hin, Win, ld_in] channels-last
    const float* w;      // [Cout, taps * Cin]
    const float* bias;   // [Cout] or nullptr
    const float* resid;  // [M, ldr] or nullptr
    float* out;
    const float* zeros;
    long ld_in, ldo, ldr;
    int Tout, Hout, Wout, Tin, Hin, Win;
    int Cin, Cout, kt, kh, kw, st, sh, sw, t_off, ph, pw, up, interleave;
    int M, tiles_m, tiles_n;
    int ophase;          // -1: plain; 0..3 = (a, b) = (ophase >> 1, ophase & 1): output pixel (t, y, x) of this launch is stored at
                         // (t, 2y + a, 2x + b) of a [Tout, 2 Hout, 2 Wout] tensor (one phase of a 2x-upsampling convolution, see uv_conv3d_f32)
    const float* act_scale;   // f16x3: nullptr, or a device scalar the result is multiplied by as well (uv_vae_split_f16's 1 / s)
    float out_scale;     // f16x3 (PREC 4): the accumulators carry the power-of-two scale of the split weights; out = acc * out_scale + bias
    int plain;           // PREC 4 only: the 128-byte operand rows hold 64 PLAIN fp16 channels instead of [32 hi | 32 lo] (uv_conv3d_f16: ONE fp16
                         // pass); Cin, ld_in and the weight rows are still counted in f32-sized units = HALF the channels
};

// The 23 kernels. A gather tile + prec names conv3d_f32_kernel<BM, BN, .., prec> (G160: 128 x 160, 64 x 160 for bf16x6); which of the sums
// exist is plan_conv's ladder below and launch_conv_gather's switch. The halo kernels carry their arithmetic in the name.
// The single-pass fp16 arithmetic (uv_conv3d_f16, ConvArgs::plain) adds NO names: it is planned as prec 4 of HALF its channel count (its
// 64-channel rows are the 128-byte rows of 32 split channels) and runs the PLAIN instantiation of whichever "+4" gather tile or HALO_F16_*
// kernel that plan names - eight more instantiations behind the same 23 names, and uv_conv3d_plan(4, .., Cin / 2, ..) reports its plan.
enum ConvKernel {
    G256x16 = 0, G160 = 8, G128x128 = 16, G256x128 = 24, G256x256 = 32,
    HALO_BF16X6 = 40, HALO_F32_160, HALO_F32_128,                      // conv3d_halo.hip
    HALO_F16_N16, HALO_F16_160, HALO_F16_SQUARE, HALO_F16_128,         // conv3d_halo16.hip
};
// their names, as uv_conv3d_plan reports them (gather: tile + PREC; 0 where the sum names no kernel)
static const char* const kConvKernelName[HALO_F16_128 + 1] = {
    "G256x16+0", 0, 0, "G256x16+3", "G256x16+4", 0, 0, 0,
    "G160+0", 0, 0, "G160+3", 0, 0, 0, 0,
    "G128x128+0", "G128x128+1", "G128x128+2", "G128x128+3", "G128x128+4", 0, 0, 0,
    0, "G256x128+1", "G256x128+2", 0, "G256x128+4", 0, 0, 0,
    0, "G256x256+1", "G256x256+2", 0, "G256x256+4", 0, 0, 0,
    "HALO_BF16X6", "HALO_F32_160", "HALO_F32_128", "HALO_F16_N16", "HALO_F16_160", "HALO_F16_SQUARE", "HALO_F16_128",
};
struct ConvPlan {
    int kernel, tiles_m, tiles_n;
};

// The geometry checks of a uv_conv3d_* call and the geometry part of its ConvArgs (everything plan_conv reads): the ONE fill that
// conv_common (conv3d_f32.hip) and the plan query uv_conv3d_plan share, so that the query plans what the call launches.
static inline int conv_geometry(ConvArgs& a, int Tout, int Hout, int Wout, int Hin, int Win, int Cin, int Cout, int kt, int kh, int kw,
                                int st, int sh, int sw, int ph, int pw, int up, int interleave) {
    UV_CHECK_ARG(Cin % 32 == 0, "uv_conv3d: Cin=%d must be a multiple of 32 (pad channels with zeros)", Cin);
    UV_CHECK_ARG(Cout % 4 == 0, "uv_conv3d: Cout=%d must be a multiple of 4", Cout);
    UV_CHECK_ARG(Tout > 0 && Hout > 0 && Wout > 0 && kt > 0 && kh > 0 && kw > 0, "uv_conv3d: bad geometry");
    UV_CHECK_ARG(!interleave || Cout % 8 == 0, "uv_conv3d: interleave needs Cout %% 8 == 0 and no residual");
    UV_CHECK_ARG(up >= 0 && up <= 5, "uv_conv3d: up=%d (0 plain, 1 nearest-2x folded into the gather, 2..5 one output phase of it)", up);
    UV_CHECK_ARG(up < 2 || (!interleave && sh == 1 && sw == 1 && st == 1), "uv_conv3d: an output-phase launch (up >= 2) takes no residual, interleave or stride");
    a.Tout = Tout; a.Hout = Hout; a.Wout = Wout; a.Hin = Hin; a.Win = Win;
    a.Cin = Cin; a.Cout = Cout; a.kt = kt; a.kh = kh; a.kw = kw; a.st = st; a.sh = sh; a.sw = sw;
    a.ph = ph; a.pw = pw; a.up = up == 1; a.ophase = up >= 2 ? up - 2 : -1; a.interleave = interleave;
    a.M = Tout * Hout * Wout;
    return 0;
}

static inline long conv_patches(const ConvArgs& a, int th, int tw) { return (long)((a.Hout + th - 1) / th) * ((a.Wout + tw - 1) / tw); }

// Which kernel runs this convolution, on what grid. prec = the PREC of conv3d_f32.hip, force = UV_OPT_CONV_HALO (developer A/B switch and
// test hook; never the environment): 0 = never a halo kernel, 1 = whenever the geometry fits (also launches too small to fill the chip,
// which the tests use), -1 = automatic. Pure: the same answer for the same arguments, whatever ran before.
static inline ConvPlan plan_conv(const ConvArgs& a, int prec, int force, int ncus) {
    // ---- the LDS-halo kernels: 3x3 spatial taps, stride 1, padding 1 (plain or behind the 2x upsampling: the halo image is filled through
    // the nearest-exact map), no interleave, whole 32-channel input blocks (all callers pad). Not an output-phase launch: the halo kernels
    // store to plain positions. bf16x3 (prec 1, 2) has no halo kernel.
    const int mul = a.up ? 2 : 1;
    if (force != 0 && (prec == 0 || prec == 3 || prec == 4) && a.ophase < 0 && a.kh == 3 && a.kw == 3 && (a.kt == 3 || a.kt == 1) &&
        a.st == 1 && a.sh == 1 && a.sw == 1 && a.ph == 1 && a.pw == 1 && !a.interleave && a.Hin * mul == a.Hout && a.Win * mul == a.Wout &&
        a.Cin % 32 == 0) {
        // output-channel tile: whole 128-wide tiles, or whole 160-wide ones (the encoder's 160 / 320-channel stages)
        const int bn = a.Cout % 128 == 0 ? 128 : a.Cout % 160 == 0 ? 160 : 0;
        int kernel = -1, th = 8, tw = 32, tiles_n = bn ? a.Cout / bn : 0;
        long fill = ncus;      // workgroups that four frames must bring (below)
        if (prec == 3) {
            if (bn == 128) kernel = HALO_BF16X6;
        } else if (prec == 0) {
            // exact f32: 8 x 16 patches on 4-wave workgroups, two per CU - 6.28 s against 6.43 s per 49 x 720 x 1280 decode on the gather kernel,
            // same process, interleaved; the 8-wave form of round 3's first version lost to it, 6.49 s, with one workgroup per CU.
            // 128-wide tile: single weight buffer, 39 KiB of LDS and 168 registers, three workgroups per CU (6.19-6.21 s against 6.26 s per
            // decode with two double-buffered workgroups per CU, same process, interleaved, bit-identical: the k order is the same)
            tw = 16;
            fill = 2 * ncus;
            if (bn) kernel = bn == 128 ? HALO_F32_128 : HALO_F32_160;
        } else if (a.Cout <= 16) {
            // f16x3, the narrow-output kernel (the decoder's head): plain geometry only
            if (!a.up) kernel = HALO_F16_N16;
            tiles_n = 1;
        } else if (bn == 160) {
            kernel = HALO_F16_160;
        } else if (bn == 128 && !((a.kt * (a.Cin >> 5)) & 1)) {      // two-tap steps pair the channel groups: even counts only
            // 16 x 16 patches where a frame cuts into FEWER of them than 8 x 32 ones (45 x 80: 3 x 5 = 15 against 6 x 3 = 18; 360 x 640: 920
            // against 900). A per-frame rule, and the results do not depend on the patch shape anyway (the kernel's note on TW).
            const bool square = conv_patches(a, 16, 16) < conv_patches(a, 8, 32);
            kernel = square ? HALO_F16_SQUARE : HALO_F16_128;
            if (square) th = tw = 16;
        }
        // enough workgroups to fill the chip at four frames per pass. Counted per FRAME: the choice must not depend on how many frames a pass
        // carries (the pass length is a memory / speed knob that leaves results bit-identical, and the halo and gather kernels sum their
        // k-tiles in different orders)
        const long patches = conv_patches(a, th, tw);
        if (kernel >= 0 && (force == 1 || 4 * patches * tiles_n >= fill)) return {kernel, (int)(a.Tout * patches), tiles_n};
    }
    // ---- the gather kernel's tile
    struct { int id, bm, bn; } t = {G128x128, 128, 128};      // the 4-wave tile of the low-resolution stages
    const long rows256 = (a.M + 255) / 256;
    if (prec == 0 || prec == 3) {
        // exact f32 and bf16x6: 128-wide column tiles, except where they would mostly compute padding:
        //   Cout <= 16 (the decoder's last convolution, 256 -> 12 channels on full-resolution frames): 256 x 16 tiles
        //     (a 128-wide tile computes 128 columns for 12);
        //   Cout a multiple of 160 but not of 128 (the encoder's 160 / 320 channel stages): 160-wide tiles, no padded columns
        //     (128-wide ones compute 256 columns for 160: 37.5 % of the MFMA work wasted; 384 for 320: 17 %). bf16x6 carries 30 KiB of
        //     weight planes per stage there: 64 rows keep two workgroups per CU (2 x 76 KiB of LDS).
        if (a.Cout <= 16) t = {G256x16, 256, 16};
        else if (a.Cout % 160 == 0 && a.Cout % 128 != 0) t = {G160, prec == 3 ? 64 : 128, 160};
    } else {
        // the three-pass arithmetics: 256x256 (16 waves, 4 per SIMD) when Cout >= 256 and the grid still fills the chip: halves the A gather
        // per output; 256x128 (8 waves) next. f16x3 has the 256 x 16 tile for Cout <= 16 too.
        if (prec == 4 && a.Cout <= 16) t = {G256x16, 256, 16};
        else if (a.Cout >= 256 && rows256 * ((a.Cout + 255) / 256) >= 256) t = {G256x256, 256, 256};
        else if (rows256 * ((a.Cout + 127) / 128) >= 256) t = {G256x128, 256, 128};
    }
    return {t.id + prec, (a.M + t.bm - 1) / t.bm, (a.Cout + t.bn - 1) / t.bn};
}

// Launches KERN on the plan's grid with LDS bytes of dynamic LDS. Up to 64 KiB a kernel may use as it is; more takes the attribute, set
// once per device.
template <auto KERN, int THREADS, int LDS>
static inline void conv_launch(ConvArgs a, const ConvPlan& plan, hipStream_t stream) {
    a.tiles_m = plan.tiles_m;
    a.tiles_n = plan.tiles_n;
    if constexpr (LDS > 64 * 1024) UV_ONCE_PER_DEVICE(hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
    hipLaunchKernelGGL(KERN, dim3(a.tiles_m * a.tiles_n), dim3(THREADS), LDS, stream, a);
}

// ---- device code that conv3d_halo_kernel and conv3d_halo_f16_kernel share
// Epilogue of four accumulators: out[m, n .. n + 3] = acc (* scale: f16x3's power-of-two descale, exact) + bias (+ residual)
template <bool SCALE>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& p, f32x4 v, long m, int n, float scale) {
    if constexpr (SCALE) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= scale;
    }
    if (p.bias) {
        const f32x4 b = *(const f32x4*)(p.bias + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += b[e];
    }
    if (p.resid) {
        const f32x4 rr = *(const f32x4*)(p.resid + m * p.ldr + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += rr[e];
    }
    *(f32x4*)(p.out + m * p.ldo + n) = v;
}

// Their grid: blockIdx.x -> output-channel tile (fastest), TH x TW pixel patch at (ty0, tx0) of output frame tf
template <int TH, int TW>
__device__ __forceinline__ void conv_patch(const ConvArgs& p, int& tile_n, int& tx0, int& ty0, int& tf) {
    const int tiles_w = (p.Wout + TW - 1) / TW, tiles_h = (p.Hout + TH - 1) / TH;
    tile_n = blockIdx.x % p.tiles_n;
    int mt = blockIdx.x / p.tiles_n;
    tx0 = (mt % tiles_w) * TW;
    mt /= tiles_w;
    ty0 = (mt % tiles_h) * TH;
    tf = mt / tiles_h;
}

// the launchers of conv3d_halo.hip (HALO_BF16X6 .. HALO_F32_128) and conv3d_halo16.hip (HALO_F16_*)
void launch_conv_halo(const ConvArgs& a, const ConvPlan& plan, hipStream_t stream);
void launch_conv_halo16(const ConvArgs& a, const ConvPlan& plan, hipStream_t stream);
