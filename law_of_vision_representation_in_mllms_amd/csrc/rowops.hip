// Row-wise / gather kernels around the GEMMs: LayerNorm, patch im2col, CLS+pos row, casts.  All HBM-bound:
// 16-byte vector accesses, one wave per row for the reductions (wave64 shuffles, no LDS).
#include "common.h"
#include "visrep_internal.h"

namespace {

// ------------------------------------------------------------------------------------------------ LayerNorm
// y[row] = (x[row] - mean) * rsqrt(var + eps) * gamma + beta   (two-pass over registers, fp32 statistics).
// One wave per row, d <= 2048, d % 8 == 0.  In-place (y == x) is safe: a lane reads all its chunks before writing.
__global__ __launch_bounds__(256) void layernorm_rows(const bf16_t* __restrict__ x, int ldx, const float* __restrict__ g,
                                                      const float* __restrict__ bta, bf16_t* __restrict__ y, int ldy,
                                                      int M, int d, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nch = d >> 3;
    const bf16_t* xr = x + (size_t)row * ldx;
    float f[4][8];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
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
    const float mean = wave_sum(sum) / (float)d;
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (lane + 64 * c < nch) {
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float t = f[c][k] - mean; sq += t * t; }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)d + eps);
    bf16_t* yr = y + (size_t)row * ldy;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nch) {
            const float4 g0 = *reinterpret_cast<const float4*>(g + ch * 8), g1 = *reinterpret_cast<const float4*>(g + ch * 8 + 4);
            const float4 b0 = *reinterpret_cast<const float4*>(bta + ch * 8), b1 = *reinterpret_cast<const float4*>(bta + ch * 8 + 4);
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = (f[c][k] - mean) * rstd * gg[k] + bb[k];
            u32x4 w = {pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3]), pack_bf16(o[4], o[5]), pack_bf16(o[6], o[7])};
            *reinterpret_cast<u32x4*>(yr + ch * 8) = w;
        }
    }
}

// LayerNorm statistics only: rt[row] = (rstd, -mean * rstd).  The normalisation itself is folded into the consuming GEMM
// (gamma into its weights, the mean / rstd terms into its epilogue: visrep_gemm_bf16_ln), so the normalised tensor is never
// written: this pass only READS the residual stream.  One wave per row, same two-pass fp32 statistics as layernorm_rows.
__global__ __launch_bounds__(256) void layernorm_stats_rows(const bf16_t* __restrict__ x, int ldx, float2* __restrict__ rt, int M, int d, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nch = d >> 3;
    const bf16_t* xr = x + (size_t)row * ldx;
    float f[4][8];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
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
    const float mean = wave_sum(sum) / (float)d;
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (lane + 64 * c < nch) {
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float t = f[c][k] - mean; sq += t * t; }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)d + eps);
    if (lane == 0) rt[row] = float2{rstd, -mean * rstd};
}

// Row statistics from the partial sums a residual GEMM's epilogue left behind (gemm_epilogue.h, HAS_ST): slot k of row m holds
// (sum, sum of squares) of 64 output columns; summed here in slot order (deterministic), var = E[x^2] - mean^2 in fp32.
__global__ __launch_bounds__(256) void ln_stats_finalize_rows(const float2* __restrict__ part, int slots, float2* __restrict__ rt, int M,
                                                              float inv_d, float eps) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= M) return;
    const float4* src = reinterpret_cast<const float4*>(part + (size_t)row * slots);   // slots is even: two slots per 16-B load
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < slots / 2; ++k) {
        const float4 v = src[k];
        s1 += v.x; s2 += v.y;
        s1 += v.z; s2 += v.w;
    }
    const float mean = s1 * inv_d;
    const float var = fmaxf(s2 * inv_d - mean * mean, 0.f);
    const float rstd = 1.0f / sqrtf(var + eps);
    rt[row] = float2{rstd, -mean * rstd};
}

// ------------------------------------------------------------------------------------------------ RMSNorm (InternViT)
// y[row] = x[row] * rsqrt(mean(x^2) + eps) * gamma  (HF InternVLVisionRMSNorm).  One wave per row, d <= 4096 (eight 16-byte chunks per lane),
// d % 8 == 0; fp32 sum of squares; one rounding to bf16.  In place (y == x) is safe: a lane reads all its chunks before it writes.
constexpr int RMS_CH = 8;                                          // chunks of 8 bf16 per lane: 64 lanes * 8 chunks * 8 = 4096 columns
VR_DEV float rms_load_row(const bf16_t* __restrict__ xr, int nch, int lane, float (&f)[RMS_CH][8]) {
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < RMS_CH; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nch) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(xr + ch * 8);
#pragma unroll
            for (int k = 0; k < 4; ++k) { f[c][2 * k] = bf_lo(v[k]); f[c][2 * k + 1] = bf_hi(v[k]); }
#pragma unroll
            for (int k = 0; k < 8; ++k) sq = __builtin_fmaf(f[c][k], f[c][k], sq);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) f[c][k] = 0.f;
        }
    }
    return wave_sum(sq);
}
VR_DEV void rms_store_row(bf16_t* __restrict__ yr, const float* __restrict__ g, int nch, int lane, float rstd, const float (&f)[RMS_CH][8]) {
#pragma unroll
    for (int c = 0; c < RMS_CH; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nch) {
            const float4 g0 = *reinterpret_cast<const float4*>(g + ch * 8), g1 = *reinterpret_cast<const float4*>(g + ch * 8 + 4);
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = f[c][k] * rstd * gg[k];
            u32x4 w = {pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3]), pack_bf16(o[4], o[5]), pack_bf16(o[6], o[7])};
            *reinterpret_cast<u32x4*>(yr + ch * 8) = w;
        }
    }
}

__global__ __launch_bounds__(256) void rms_rows(const bf16_t* __restrict__ x, int ldx, const float* __restrict__ g, bf16_t* __restrict__ y, int ldy,
                                                int M, int d, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float f[RMS_CH][8];
    const float ss = rms_load_row(x + (size_t)row * ldx, d >> 3, lane, f);
    const float rstd = 1.0f / sqrtf(ss / (float)d + eps);
    rms_store_row(y + (size_t)row * ldy, g, d >> 3, lane, rstd, f);
}

// RMS statistics only: rt[row] = (rstd, 0) - the (rstd, -mean * rstd) pair of layernorm_stats_rows with "mean" exactly zero, so the folded-LN
// GEMM epilogue fma(acc, rt.x, rt.y * s[n]) computes rstd * acc: Linear(RMSNorm(x)) with W = gamma o W_orig.
__global__ __launch_bounds__(256) void rms_stats_rows(const bf16_t* __restrict__ x, int ldx, float2* __restrict__ rt, int M, int d, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nch = d >> 3;
    const bf16_t* xr = x + (size_t)row * ldx;
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < RMS_CH; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nch) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(xr + ch * 8);
#pragma unroll
            for (int k = 0; k < 4; ++k) { const float a = bf_lo(v[k]), b = bf_hi(v[k]); sq = __builtin_fmaf(a, a, sq); sq = __builtin_fmaf(b, b, sq); }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)d + eps);
    if (lane == 0) rt[row] = float2{rstd, 0.f};
}

// RMS form of ln_stats_finalize_rows: only the sum-of-squares slot of the residual GEMM's partial sums is used.
__global__ __launch_bounds__(256) void rms_stats_finalize_rows(const float2* __restrict__ part, int slots, float2* __restrict__ rt, int M,
                                                               float inv_d, float eps) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= M) return;
    const float4* src = reinterpret_cast<const float4*>(part + (size_t)row * slots);   // slots is even: two slots per 16-B load
    float s2 = 0.f;
    for (int k = 0; k < slots / 2; ++k) {
        const float4 v = src[k];
        s2 += v.y;
        s2 += v.w;
    }
    rt[row] = float2{1.0f / sqrtf(s2 * inv_d + eps), 0.f};
}

// QK normalisation (HF InternVLVisionAttention, use_qk_norm): in place on the Q|K GEMM's output [M, ldqk], Q in columns [0, da), K in [da, 2 da).
// One wave per (row, half): RMSNorm over the half's da columns - all heads, zero-padded head lanes included, which add nothing to the sum -
// with the mean taken over the TRUE width (inv_dt = 1 / (heads * head_dim)); x * rstd * g[c] in fp32, one rounding.  g is zero in padded columns.
__global__ __launch_bounds__(256) void qk_rmsnorm_rows(bf16_t* __restrict__ qk, int ldqk, int da, float inv_dt, const float* __restrict__ qg,
                                                       const float* __restrict__ kg, int M, float eps) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long row = item >> 1;
    const int half = (int)(item & 1);
    if (row >= M) return;
    bf16_t* xr = qk + (size_t)row * ldqk + (size_t)half * da;
    float f[RMS_CH][8];
    const float ss = rms_load_row(xr, da >> 3, lane, f);
    const float rstd = 1.0f / sqrtf(ss * inv_dt + eps);
    rms_store_row(xr, half ? kg : qg, da >> 3, lane, rstd, f);
}

// fp32 forms for the reference-precision tower (any d % 4 == 0); one wave per row / per (row, half)
__global__ __launch_bounds__(256) void rms_f32_rows(const float* x, int ldx, const float* __restrict__ g, float* y, int ldy,
                                                    long items, int d, int halves, float inv_d, float eps, const float* __restrict__ g2) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= items) return;
    const long row = item / halves;
    const int half = (int)(item - row * halves);
    const float* xr = x + (size_t)row * ldx + (size_t)half * d;
    float* yr = y + (size_t)row * ldy + (size_t)half * d;
    const float* gg = half ? g2 : g;
    float q = 0.f;
    for (int c = lane; c < d; c += 64) q = __builtin_fmaf(xr[c], xr[c], q);
    const float rstd = 1.0f / sqrtf(wave_sum(q) * inv_d + eps);
    for (int c = lane; c < d; c += 64) yr[c] = xr[c] * rstd * gg[c];
}

// ------------------------------------------------------------------------------------------------ im2col
// pixels [B, 3, H, W] (fp32 or bf16) -> cols [B*gh*gw, Kpad] bf16 with k = c*p*p + i*p + j (Conv2d weight order),
// zero-filled for k >= 3*p*p; gh = H / p, gw = W / p floored (the last H % p rows and W % p columns are never read).  One thread per 8 output elements (16-B store).
template <typename TIN>
__global__ __launch_bounds__(256) void im2col_patches(const TIN* __restrict__ px, bf16_t* __restrict__ cols, int B, int Himg,
                                                      int Wimg, int patch, int Kpad) {
    const int gh = Himg / patch, gw = Wimg / patch;
    const int kch = Kpad >> 3;
    const long total = (long)B * gh * gw * kch;
    const int K = 3 * patch * patch, pp = patch * patch;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int ch = (int)(idx % kch);
        const long row = idx / kch;
        const int gx = (int)(row % gw);
        const int gy = (int)((row / gw) % gh);
        const int b = (int)(row / ((long)gw * gh));
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = ch * 8 + e;
            float val = 0.f;
            if (k < K) {
                const int c = k / pp, rem = k - c * pp;
                const int i = rem / patch, j = rem - i * patch;
                const size_t off = (((size_t)b * 3 + c) * Himg + (gy * patch + i)) * Wimg + gx * patch + j;
                if (sizeof(TIN) == 4) val = reinterpret_cast<const float*>(px)[off];
                else val = bf2f(reinterpret_cast<const bf16_t*>(px)[off]);
            }
            v[e] = val;
        }
        u32x4 w = {pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
        *reinterpret_cast<u32x4*>(cols + row * Kpad + ch * 8) = w;
    }
}

// x[b*T + 0][:] = cls + pos[0]
__global__ void cls_rows(bf16_t* __restrict__ x, int ldx, const float* __restrict__ cls, const float* __restrict__ pos,
                         int B, int T, int d) {
    const int b = blockIdx.x;
    for (int n = threadIdx.x; n < d; n += blockDim.x) x[(size_t)b * T * ldx + n] = f2bf(cls[n] + pos[n]);
}

// x[b*T + r][:] = table[r] + pos[r], r < prefix (the class token and the register tokens; the registers' pos rows are zero)
__global__ void prefix_rows(bf16_t* __restrict__ x, int ldx, const float* __restrict__ table, const float* __restrict__ pos,
                            int B, int T, int d) {
    const int b = blockIdx.x, r = blockIdx.y;
    for (int n = threadIdx.x; n < d; n += blockDim.x) x[((size_t)b * T + r) * ldx + n] = f2bf(table[(size_t)r * d + n] + pos[(size_t)r * d + n]);
}

__global__ void cast_f32_to_bf16(const float* __restrict__ src, bf16_t* __restrict__ dst, long n) {
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 2; i < n; i += (long)gridDim.x * blockDim.x * 2) {
        if (i + 1 < n) *reinterpret_cast<uint32_t*>(dst + i) = pack_bf16(src[i], src[i + 1]);
        else dst[i] = f2bf(src[i]);
    }
}

}  // namespace

extern "C" int visrep_layernorm(const void* x, int ldx, const float* gamma, const float* beta, void* y, int ldy, int rows,
                                int d, float eps, void* stream) {
    if (rows <= 0) return 0;
    if (d % 8 || d > 2048 || (ldx % 8) || (ldy % 8)) return visrep_set_error(VISREP_ERR_SHAPE, "layernorm: need d % 8 == 0, d <= 2048");
    hipLaunchKernelGGL(layernorm_rows, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, gamma, beta,
                       (bf16_t*)y, ldy, rows, d, eps);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "layernorm: launch failed");
}

extern "C" int visrep_layernorm_stats(const void* x, int ldx, void* rt, int rows, int d, float eps, void* stream) {
    if (rows <= 0) return 0;
    if (d % 8 || d > 2048 || (ldx % 8)) return visrep_set_error(VISREP_ERR_SHAPE, "layernorm_stats: need d % 8 == 0, d <= 2048");
    visrep_count_route(VISREP_ROUTE_STATS_ROWS);
    hipLaunchKernelGGL(layernorm_stats_rows, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, (float2*)rt, rows, d, eps);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "layernorm_stats: launch failed");
}

int visrep_ln_stats_finalize(const float2* partial, int slots, float2* rt, int rows, int d, float eps, hipStream_t s) {
    if (rows <= 0) return 0;
    if (slots <= 0 || (slots & 1)) return visrep_set_error(VISREP_ERR_SHAPE, "ln_stats_finalize: slot count must be even");
    visrep_count_route(VISREP_ROUTE_STATS_EPILOGUE);
    hipLaunchKernelGGL(ln_stats_finalize_rows, dim3((rows + 255) / 256), dim3(256), 0, s, partial, slots, rt, rows, 1.0f / (float)d, eps);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "ln_stats_finalize: launch failed");
}

int visrep_rms_stats_finalize(const float2* partial, int slots, float2* rt, int rows, int d, float eps, hipStream_t s) {
    if (rows <= 0) return 0;
    if (slots <= 0 || (slots & 1)) return visrep_set_error(VISREP_ERR_SHAPE, "rms_stats_finalize: slot count must be even");
    visrep_count_route(VISREP_ROUTE_STATS_EPILOGUE);
    visrep_count_route(VISREP_ROUTE_RMS);
    hipLaunchKernelGGL(rms_stats_finalize_rows, dim3((rows + 255) / 256), dim3(256), 0, s, partial, slots, rt, rows, 1.0f / (float)d, eps);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "rms_stats_finalize: launch failed");
}

extern "C" int visrep_rmsnorm(const void* x, int ldx, const float* gamma, void* y, int ldy, int rows, int d, float eps, void* stream) {
    if (!x || !gamma || !y) return visrep_set_error(VISREP_ERR_ARG, "rmsnorm: null pointer");
    if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)y) & 15) return visrep_set_error(VISREP_ERR_ARG, "rmsnorm: x, gamma and y must be 16-byte aligned");
    if (d <= 0 || d % 8 || d > 4096 || (ldx % 8) || (ldy % 8) || ldx < d || ldy < d)
        return visrep_set_error(VISREP_ERR_SHAPE, "rmsnorm: need d % 8 == 0, d <= 4096, ldx / ldy % 8 == 0 and >= d");
    if (rows <= 0) return 0;
    visrep_count_route(VISREP_ROUTE_RMS);
    hipLaunchKernelGGL(rms_rows, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, gamma, (bf16_t*)y, ldy, rows, d, eps);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "rmsnorm: launch failed");
}

extern "C" int visrep_rmsnorm_stats(const void* x, int ldx, void* rt, int rows, int d, float eps, void* stream) {
    if (!x || !rt) return visrep_set_error(VISREP_ERR_ARG, "rmsnorm_stats: null pointer");
    if (((uintptr_t)x & 15) || ((uintptr_t)rt & 7)) return visrep_set_error(VISREP_ERR_ARG, "rmsnorm_stats: x must be 16-byte, rt 8-byte aligned");
    if (d <= 0 || d % 8 || d > 4096 || (ldx % 8) || ldx < d) return visrep_set_error(VISREP_ERR_SHAPE, "rmsnorm_stats: need d % 8 == 0, d <= 4096, ldx % 8 == 0 and >= d");
    if (rows <= 0) return 0;
    visrep_count_route(VISREP_ROUTE_STATS_ROWS);
    visrep_count_route(VISREP_ROUTE_RMS);
    hipLaunchKernelGGL(rms_stats_rows, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, (float2*)rt, rows, d, eps);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "rmsnorm_stats: launch failed");
}

extern "C" int visrep_qk_rmsnorm(void* qk, int ldqk, int width, int d_true, const float* qn_g, const float* kn_g, int rows, float eps, void* stream) {
    if (!qk || !qn_g || !kn_g) return visrep_set_error(VISREP_ERR_ARG, "qk_rmsnorm: null pointer");
    if (((uintptr_t)qk | (uintptr_t)qn_g | (uintptr_t)kn_g) & 15) return visrep_set_error(VISREP_ERR_ARG, "qk_rmsnorm: qk, qn_g and kn_g must be 16-byte aligned");
    if (width <= 0 || width % 8 || width > 4096) return visrep_set_error(VISREP_ERR_SHAPE, "qk_rmsnorm: width must be a multiple of 8, at most 4096");
    if (ldqk % 8 || ldqk < 2 * width) return visrep_set_error(VISREP_ERR_SHAPE, "qk_rmsnorm: ldqk % 8 == 0 and ldqk >= 2 * width required");
    if (d_true <= 0 || d_true > width) return visrep_set_error(VISREP_ERR_SHAPE, "qk_rmsnorm: 0 < d_true <= width required");
    if (rows <= 0) return 0;
    visrep_count_route(VISREP_ROUTE_QK_NORM);
    const long items = 2L * rows;
    hipLaunchKernelGGL(qk_rmsnorm_rows, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)qk, ldqk, width, 1.0f / (float)d_true,
                       qn_g, kn_g, rows, eps);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "qk_rmsnorm: launch failed");
}

extern "C" int visrep_rmsnorm_f32(const float* x, int ldx, const float* gamma, float* y, int ldy, int rows, int d, float eps, void* stream) {
    if (!x || !gamma || !y) return visrep_set_error(VISREP_ERR_ARG, "rmsnorm_f32: null pointer");
    if (d <= 0 || ldx < d || ldy < d) return visrep_set_error(VISREP_ERR_SHAPE, "rmsnorm_f32: ldx, ldy >= d > 0 required");
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(rms_f32_rows, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, ldx, gamma, y, ldy, (long)rows, d, 1, 1.0f / (float)d, eps, gamma);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "rmsnorm_f32: launch failed");
}

extern "C" int visrep_qk_rmsnorm_f32(float* qk, int ldqk, int width, int d_true, const float* qn_g, const float* kn_g, int rows, float eps, void* stream) {
    if (!qk || !qn_g || !kn_g) return visrep_set_error(VISREP_ERR_ARG, "qk_rmsnorm_f32: null pointer");
    if (width <= 0 || ldqk < 2 * width || d_true <= 0 || d_true > width) return visrep_set_error(VISREP_ERR_SHAPE, "qk_rmsnorm_f32: ldqk >= 2 * width, 0 < d_true <= width required");
    if (rows <= 0) return 0;
    const long items = 2L * rows;
    hipLaunchKernelGGL(rms_f32_rows, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, (hipStream_t)stream, qk, ldqk, qn_g, qk, ldqk, items, width, 2,
                       1.0f / (float)d_true, eps, kn_g);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "qk_rmsnorm_f32: launch failed");
}

extern "C" int visrep_im2col(const void* pixels, int pixel_dtype, void* cols, int B, int Himg, int Wimg, int patch, int Kpad,
                             void* stream) {
    if (B <= 0) return 0;
    // Himg / patch floors like Conv2d(k = s = patch): trailing pixels that fill no patch are dropped (384 / 14 = 27 patches, 6 pixels unused)
    if (patch <= 0 || Himg < patch || Wimg < patch || Kpad % 8 || Kpad < 3 * patch * patch)
        return visrep_set_error(VISREP_ERR_SHAPE, "im2col: image must hold at least one patch, Kpad >= 3*p*p and % 8");
    const long total = (long)B * (Himg / patch) * (Wimg / patch) * (Kpad / 8);
    const int grid = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
    if (pixel_dtype == VISREP_F32)
        hipLaunchKernelGGL(im2col_patches<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)pixels, (bf16_t*)cols, B,
                           Himg, Wimg, patch, Kpad);
    else if (pixel_dtype == VISREP_BF16)
        hipLaunchKernelGGL(im2col_patches<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)pixels, (bf16_t*)cols, B,
                           Himg, Wimg, patch, Kpad);
    else
        return visrep_set_error(VISREP_ERR_ARG, "im2col: pixel dtype must be VISREP_F32 or VISREP_BF16");
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "im2col: launch failed");
}

extern "C" int visrep_cls_rows(void* x, int ldx, const float* cls, const float* pos, int B, int T, int d, void* stream) {
    if (B <= 0) return 0;
    hipLaunchKernelGGL(cls_rows, dim3(B), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x, ldx, cls, pos, B, T, d);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "cls_rows: launch failed");
}

extern "C" int visrep_prefix_rows(void* x, int ldx, const float* table, const float* pos, int B, int T, int prefix, int d, void* stream) {
    if (B <= 0) return 0;
    if (!x || !table || !pos) return visrep_set_error(VISREP_ERR_ARG, "prefix_rows: null pointer");
    if (prefix < 1 || prefix > T || B > 65535) return visrep_set_error(VISREP_ERR_SHAPE, "prefix_rows: 1 <= prefix <= T");
    if (prefix == 1) return visrep_cls_rows(x, ldx, table, pos, B, T, d, stream);
    hipLaunchKernelGGL(prefix_rows, dim3(B, prefix), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x, ldx, table, pos, B, T, d);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "prefix_rows: launch failed");
}

extern "C" int visrep_cast_f32_bf16(const float* src, void* dst, long n, void* stream) {
    if (n <= 0) return 0;
    long blocks = (n / 2 + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(cast_f32_to_bf16, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, src, (bf16_t*)dst, n);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "cast: launch failed");
}
