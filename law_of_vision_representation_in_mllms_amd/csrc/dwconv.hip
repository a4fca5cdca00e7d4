// ConvNeXt kernels: the depthwise 7x7 convolution on channels-last token rows that also leaves the LayerNorm statistics of its output, and the
// LayerNorm + 2x2 space-to-depth gather in front of a stage's downsampling GEMM.
//
// dwconv7x7_stats_tile<TH, TW>: one workgroup = one image, one slab of 64 channels, one TH x TW tile of output pixels.  The (TH + 6) x (TW + 6)
// input halo of the slab is staged ONCE into LDS with 16-byte loads (zeros outside the image: padding 3, and a tile never reads another image);
// a thread owns 8 channels of a run of 8 output pixels along x: 64 fp32 accumulators as 32 packed pairs, one LDS read of 16 bytes per input pixel
// of the run's row (14 per tap row, each feeding up to 7 outputs), the 7 x 8 weights of a tap row in registers.  49 packed FMAs per pair of
// channels and output, in tap order (ky major, kx minor) from acc = bias: the same chain visrep_dwconv7x7_stats_cpu computes with fmaf.
// The eight lanes that hold one pixel's 64 channels are neighbours: the output row is written as 128 contiguous bytes (16 per lane) and the
// slab's (sum, sum of squares) of the bf16-ROUNDED outputs takes three xor-shuffles.
// Two tile shapes: 16 x 16 (256 threads, halo 1.9 pixels read per output) for large maps, 8 x 8 (one wave, halo 3.1) for small or ragged ones;
// the launcher takes the one that computes fewer padded outputs.
#include "common.h"
#include "visrep_internal.h"

namespace {

constexpr int DW_PIX_BYTES = 144;   // LDS bytes per staged pixel: 64 bf16 + 16 bytes, so that runs 8 or (TW + 6) pixels apart do not share a bank group

VR_DEV f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

template <int TH, int TW>
__global__ __launch_bounds__(TH * TW) void dwconv7x7_stats_tile(const bf16_t* __restrict__ x, int ldx, const float* __restrict__ wt,
                                                                const float* __restrict__ bias, bf16_t* __restrict__ y, int ldy,
                                                                float2* __restrict__ part, int slots, int H, int W, int C, int tiles_x, int tiles_y) {
    constexpr int NT = TH * TW, HWD = TW + 6, HP = (TH + 6) * HWD, RUNS_X = TW / 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char dw_lds[];
    int bid = blockIdx.x;
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y; bid /= tiles_y;
    const int nslab = C >> 6;
    const int slab = bid % nslab, b = bid / nslab;
    const int y0 = ty * TH, x0 = tx * TW;
    const size_t img = (size_t)b * H * W;                            // first token row of this image
    const bf16_t* xb = x + img * ldx + slab * 64;
    for (int i = threadIdx.x; i < HP * 8; i += NT) {
        const int pix = i >> 3, c8 = i & 7;
        const int hy = pix / HWD, hx = pix - hy * HWD;
        const int gy = y0 - 3 + hy, gx = x0 - 3 + hx;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const u32x4*>(xb + ((size_t)gy * W + gx) * ldx + c8 * 8);
        *reinterpret_cast<u32x4*>(dw_lds + pix * DW_PIX_BYTES + c8 * 16) = v;
    }
    __syncthreads();
    const int cg = threadIdx.x & 7, run = threadIdx.x >> 3;
    const int ry = run / RUNS_X, rx = (run - ry * RUNS_X) * 8;       // the run's row inside the tile and its first output column
    const int ch = slab * 64 + cg * 8;
    f32x2 acc[8][4];
    {
        const float4 b0 = *reinterpret_cast<const float4*>(bias + ch), b1 = *reinterpret_cast<const float4*>(bias + ch + 4);
#pragma unroll
        for (int p = 0; p < 8; ++p) { acc[p][0] = f32x2{b0.x, b0.y}; acc[p][1] = f32x2{b0.z, b0.w}; acc[p][2] = f32x2{b1.x, b1.y}; acc[p][3] = f32x2{b1.z, b1.w}; }
    }
#pragma unroll 1
    for (int ky = 0; ky < 7; ++ky) {
        f32x2 w[7][4];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
            const float* wp = wt + (size_t)(ky * 7 + kx) * C + ch;
            const float4 a0 = *reinterpret_cast<const float4*>(wp), a1 = *reinterpret_cast<const float4*>(wp + 4);
            w[kx][0] = f32x2{a0.x, a0.y}; w[kx][1] = f32x2{a0.z, a0.w}; w[kx][2] = f32x2{a1.x, a1.y}; w[kx][3] = f32x2{a1.z, a1.w};
        }
        const unsigned char* row = dw_lds + ((ry + ky) * HWD + rx) * DW_PIX_BYTES + cg * 16;
#pragma unroll
        for (int xi = 0; xi < 14; ++xi) {                            // halo column rx + xi feeds outputs xi - 6 .. xi through taps kx = xi - xo
            const u32x4 v = *reinterpret_cast<const u32x4*>(row + xi * DW_PIX_BYTES);
            f32x2 in[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) in[k] = f32x2{bf_lo(v[k]), bf_hi(v[k])};
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const int xo = xi - kx;
                if (xo >= 0 && xo < 8) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[xo][k] = fma2(in[k], w[kx][k], acc[xo][k]);
                }
            }
        }
    }
    const int gy = y0 + ry;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int gx = x0 + rx + p;
        const bool valid = gy < H && gx < W;                         // the same for the eight lanes of a pixel
        u32x4 o;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k] = pack_bf16(acc[p][k].x, acc[p][k].y);
            const float lo = bf_lo(o[k]), hi = bf_hi(o[k]);          // the statistics are those of the values the GEMM will read
            s1 += lo; s2 = __builtin_fmaf(lo, lo, s2);
            s1 += hi; s2 = __builtin_fmaf(hi, hi, s2);
        }
#pragma unroll
        for (int m = 1; m <= 4; m <<= 1) { s1 += __shfl_xor(s1, m); s2 += __shfl_xor(s2, m); }
        if (valid) {
            const size_t r = img + (size_t)gy * W + gx;
            *reinterpret_cast<u32x4*>(y + r * ldy + ch) = o;
            if (cg == 0) part[r * slots + slab] = float2{s1, s2};
        }
    }
}

// ln_stats_finalize_rows (rowops.hip) for an ODD slot count (C = 64, 192, 320 ...): that kernel reads two slots per 16-byte load.  Same sums in
// the same slot order, same var = E[x^2] - mean^2 in fp32.
__global__ __launch_bounds__(256) void ln_stats_finalize_rows_odd(const float2* __restrict__ part, int slots, float2* __restrict__ rt, long M,
                                                                  float inv_d, float eps) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= M) return;
    const float2* src = part + (size_t)row * slots;
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < slots; ++k) { const float2 v = src[k]; s1 += v.x; s2 += v.y; }
    const float mean = s1 * inv_d;
    const float var = fmaxf(s2 * inv_d - mean * mean, 0.f);
    const float rstd = 1.0f / sqrtf(var + eps);
    rt[row] = float2{rstd, -mean * rstd};
}

// Downsampling layer, first half: out[(b, oy, ox)][(i * 2 + j) * C + c] = bf16(LayerNorm(x[b, 2 oy + i, 2 ox + j, :])[c]) - the rows of the 2x2
// stride-2 convolution's GEMM.  The four pixels of a window have their own statistics, so the norm cannot ride in that GEMM's epilogue.
// One wave per INPUT pixel, the row in registers (C <= 4096), two-pass fp32 statistics as layernorm_rows.
constexpr int S2D_CH = 8;
__global__ __launch_bounds__(256) void ln_space_to_depth2_rows(const bf16_t* __restrict__ x, int ldx, const float* __restrict__ g,
                                                               const float* __restrict__ bta, bf16_t* __restrict__ out, int ldo, long M, int H, int W,
                                                               int C, float eps) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nch = C >> 3;
    const bf16_t* xr = x + (size_t)row * ldx;
    float f[S2D_CH][8];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < S2D_CH; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nch) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(xr + ch * 8);
#pragma unroll
            for (int k = 0; k < 4; ++k) { f[c][2 * k] = bf_lo(v[k]); f[c][2 * k + 1] = bf_hi(v[k]); }
#pragma unroll
            for (int k = 0; k < 8; ++k) sum += f[c][k];
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) f[c][k] = 0.f;
        }
    }
    const float mean = wave_sum(sum) / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < S2D_CH; ++c)
        if (lane + 64 * c < nch) {
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float t = f[c][k] - mean; sq = __builtin_fmaf(t, t, sq); }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)C + eps);
    const int px = (int)(row % W);
    const long t = row / W;
    const int py = (int)(t % H);
    const long b = t / H;
    const size_t orow = ((size_t)b * (H >> 1) + (py >> 1)) * (W >> 1) + (px >> 1);
    bf16_t* o = out + orow * ldo + (size_t)((py & 1) * 2 + (px & 1)) * C;
#pragma unroll
    for (int c = 0; c < S2D_CH; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nch) {
            const float4 g0 = *reinterpret_cast<const float4*>(g + ch * 8), g1 = *reinterpret_cast<const float4*>(g + ch * 8 + 4);
            const float4 b0 = *reinterpret_cast<const float4*>(bta + ch * 8), b1 = *reinterpret_cast<const float4*>(bta + ch * 8 + 4);
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (f[c][k] - mean) * rstd * gg[k] + bb[k];
            u32x4 w = {pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
            *reinterpret_cast<u32x4*>(o + ch * 8) = w;
        }
    }
}

template <int TH, int TW>
int launch_dwconv(const bf16_t* x, int ldx, const float* wt, const float* bias, bf16_t* y, int ldy, float2* part, int slots, int B, int H, int W,
                  int C, hipStream_t s) {
    static VisrepLdsOptIn optin;
    constexpr int lds = (TH + 6) * (TW + 6) * DW_PIX_BYTES;
    const void* kern = (const void*)dwconv7x7_stats_tile<TH, TW>;
    if (lds > 48 * 1024) (void)visrep_lds_opt_in(optin, kern, lds);   // a failed opt-in is reported with the launch error below
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const long blocks = (long)B * (C / 64) * tiles_x * tiles_y;
    if (blocks > 0x7fffffffL) return visrep_set_error(VISREP_ERR_SHAPE, "dwconv7x7: too many tiles for one launch");
    hipLaunchKernelGGL((dwconv7x7_stats_tile<TH, TW>), dim3((unsigned)blocks), dim3(TH * TW), lds, s, x, ldx, wt, bias, y, ldy, part, slots, H, W, C,
                       tiles_x, tiles_y);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "dwconv7x7: launch failed");
}

}  // namespace

extern "C" int visrep_dwconv7x7_stats(const void* x, int ldx, const float* wt, const float* bias, void* y, int ldy, void* partial, void* rt, int B,
                                      int H, int W, int C, float eps, void* stream) {
    if (!x || !wt || !bias || !y || !partial || !rt) return visrep_set_error(VISREP_ERR_ARG, "dwconv7x7: null pointer");
    if (((uintptr_t)x | (uintptr_t)wt | (uintptr_t)bias | (uintptr_t)y) & 15) return visrep_set_error(VISREP_ERR_ARG, "dwconv7x7: x, wt, bias and y must be 16-byte aligned");
    if (((uintptr_t)partial | (uintptr_t)rt) & 7) return visrep_set_error(VISREP_ERR_ARG, "dwconv7x7: partial and rt must be 8-byte aligned");
    if (x == y) return visrep_set_error(VISREP_ERR_ARG, "dwconv7x7: y must not alias x (a tile reads its neighbours' pixels)");
    if (C <= 0 || C % 64) return visrep_set_error(VISREP_ERR_SHAPE, "dwconv7x7: C must be a positive multiple of 64");
    if (B < 0 || H < 1 || W < 1) return visrep_set_error(VISREP_ERR_SHAPE, "dwconv7x7: need B >= 0, H >= 1, W >= 1");
    if (ldx % 8 || ldy % 8 || ldx < C || ldy < C) return visrep_set_error(VISREP_ERR_SHAPE, "dwconv7x7: ldx / ldy must be multiples of 8 and >= C");
    if ((long)B * H * W > 0x7fffffffL) return visrep_set_error(VISREP_ERR_SHAPE, "dwconv7x7: B * H * W must fit 31 bits");
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int slots = C / 64, rows = B * H * W;
    const long area16 = (long)((H + 15) / 16) * ((W + 15) / 16) * 256, area8 = (long)((H + 7) / 8) * ((W + 7) / 8) * 64;   // outputs computed, padding included
    int rc;
    if (area8 < area16) {
        visrep_count_route(VISREP_ROUTE_DWCONV_8);
        rc = launch_dwconv<8, 8>((const bf16_t*)x, ldx, wt, bias, (bf16_t*)y, ldy, (float2*)partial, slots, B, H, W, C, s);
    } else {
        visrep_count_route(VISREP_ROUTE_DWCONV_16);
        rc = launch_dwconv<16, 16>((const bf16_t*)x, ldx, wt, bias, (bf16_t*)y, ldy, (float2*)partial, slots, B, H, W, C, s);
    }
    if (rc) return rc;
    visrep_count_route(VISREP_ROUTE_DWCONV_FINALIZE);
    if (!(slots & 1)) return visrep_ln_stats_finalize((const float2*)partial, slots, (float2*)rt, rows, C, eps, s);
    hipLaunchKernelGGL(ln_stats_finalize_rows_odd, dim3((rows + 255) / 256), dim3(256), 0, s, (const float2*)partial, slots, (float2*)rt, (long)rows,
                       1.0f / (float)C, eps);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "dwconv7x7: statistics finalize launch failed");
}

extern "C" int visrep_ln_space_to_depth2(const void* x, int ldx, const float* gamma, const float* beta, void* out, int ldo, int B, int H, int W, int C,
                                         float eps, void* stream) {
    if (!x || !gamma || !beta || !out) return visrep_set_error(VISREP_ERR_ARG, "ln_space_to_depth2: null pointer");
    if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15) return visrep_set_error(VISREP_ERR_ARG, "ln_space_to_depth2: pointers must be 16-byte aligned");
    if (x == out) return visrep_set_error(VISREP_ERR_ARG, "ln_space_to_depth2: out must not alias x");
    if (C <= 0 || C % 8 || C > 4096) return visrep_set_error(VISREP_ERR_SHAPE, "ln_space_to_depth2: C must be a multiple of 8, at most 4096");
    if (B < 0 || H < 2 || W < 2 || (H & 1) || (W & 1)) return visrep_set_error(VISREP_ERR_SHAPE, "ln_space_to_depth2: H and W must be even and >= 2");
    if (ldx % 8 || ldo % 8 || ldx < C || (long)ldo < 4L * C) return visrep_set_error(VISREP_ERR_SHAPE, "ln_space_to_depth2: ldx % 8, ldo % 8, ldx >= C and ldo >= 4 C required");
    const long M = (long)B * H * W;
    if (M > 0x7fffffffL) return visrep_set_error(VISREP_ERR_SHAPE, "ln_space_to_depth2: B * H * W must fit 31 bits");
    if (M == 0) return 0;
    visrep_count_route(VISREP_ROUTE_LN_S2D);
    hipLaunchKernelGGL(ln_space_to_depth2_rows, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, gamma, beta,
                       (bf16_t*)out, ldo, M, H, W, C, eps);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "ln_space_to_depth2: launch failed");
}
