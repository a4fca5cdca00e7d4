// C-ABI glue: error handling, the standalone GEMM entry point and the composed ViT tower forward.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include <cstdlib>
#include "common.h"
#include "visrep_internal.h"

static thread_local char g_err[256] = "";
// A failed dynamic-LDS opt-in (visrep_lds_opt_in) leaves its HIP error here; the launch that follows fails too, and whatever message that
// launcher reports gets the real cause appended instead of a bare "launch failed".
static thread_local char g_lds_note[96] = "";

int visrep_set_error(int code, const char* msg) {
    if (code == VISREP_ERR_LAUNCH && g_lds_note[0]) {
        snprintf(g_err, sizeof(g_err), "%s (%s)", msg, g_lds_note);
        g_lds_note[0] = 0;
        return code;
    }
    strncpy(g_err, msg, sizeof(g_err) - 1);
    g_err[sizeof(g_err) - 1] = 0;
    return code;
}

hipError_t visrep_lds_opt_in_slow(VisrepLdsOptIn& st, const void* kernel, int bytes, int dev) {
    static std::mutex mu;                                        // slow path only: a kernel's first launch per (device, size)
    std::lock_guard<std::mutex> lock(mu);
    if (st.bytes[dev].load(std::memory_order_acquire) >= bytes) return hipSuccess;       // another thread raised it meanwhile
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        snprintf(g_lds_note, sizeof(g_lds_note), "LDS opt-in to %d bytes failed: %s", bytes, hipGetErrorString(e));
        (void)hipGetLastError();                                 // the sticky error belongs to this call, not to the launch behind it
        return e;
    }
    st.bytes[dev].store(bytes, std::memory_order_release);       // recorded only after the attribute holds: never larger than what is set
    g_lds_note[0] = 0;                                           // a stale note of an earlier failed opt-in must not ride on an unrelated later error
    return hipSuccess;
}

extern "C" int visrep_version(void) { return VISREP_VERSION; }

thread_local long t_visrep_routes[VISREP_ROUTE_COUNT] = {};

extern "C" int visrep_debug_routes(long* out, int reset) {
    for (int i = 0; i < VISREP_ROUTE_COUNT; ++i) {
        if (out) out[i] = t_visrep_routes[i];
        if (reset) t_visrep_routes[i] = 0;
    }
    return VISREP_ROUTE_COUNT;
}

namespace {
// visrep_debug_mfma_probe: a free-running MFMA stream (tools/probes/mfma_probe.hip, variant V0 / 16x16x32), operands in registers
__global__ __launch_bounds__(512, 2) void mfma_probe_kernel(float* sink, int iters, int rnd) {
    const int lane = threadIdx.x & 63;
    bf16x8 a[4], b[4];
    unsigned st = (threadIdx.x * 2654435761u) ^ (blockIdx.x * 40503u) ^ 0x9e3779b9u;
    for (int i = 0; i < 4; ++i)
        for (int e = 0; e < 8; ++e) {
            if (rnd) {      // sign | biased exponent 0x7d..0x80 | random mantissa: |x| in [0.25, 4) - activations-sized values, every bit toggling
                st = st * 1664525u + 1013904223u; unsigned r = st >> 8;
                a[i][e] = (short)(((r & 1) << 15) | ((0x7d + ((r >> 1) & 3)) << 7) | ((r >> 3) & 0x7f));
                st = st * 1664525u + 1013904223u; r = st >> 8;
                b[i][e] = (short)(((r & 1) << 15) | ((0x7d + ((r >> 1) & 3)) << 7) | ((r >> 3) & 0x7f));
            } else {
                a[i][e] = (short)(e == 0 ? lane + i : e);
                b[i][e] = (short)(e == 0 ? lane * 3 + i : e);
            }
        }
    f32x4 acc[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned long long c0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();   // shader-clock cycles / 100-MHz ticks
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 32; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i & 3], b[(i >> 2) & 3], acc[i], 0, 0, 0);
        if ((it & 63) == 63) {                                   // keep the sums finite and the accumulator bits moving: restart from a small value
#pragma unroll
            for (int i = 0; i < 32; ++i) acc[i] *= 1e-3f;
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) s += acc[i][1];
    if (s == 123.456f) sink[0] = s;                              // keeps the accumulators live; never true in practice
    const unsigned long long c1 = __builtin_readcyclecounter(), r1 = __builtin_amdgcn_s_memrealtime();
    if (blockIdx.x == 0 && threadIdx.x == 0) {                   // the clock this stream ran at: (c1 - c0) / ((r1 - r0) * 10 ns)
        unsigned long long* o = reinterpret_cast<unsigned long long*>(sink);
        o[1] = c1 - c0;
        o[2] = r1 - r0;
    }
}
}  // namespace

extern "C" int visrep_debug_mfma_probe(int iters, int random, void* sink, double* flop, void* stream) {
    if (iters <= 0 || !sink) return visrep_set_error(VISREP_ERR_ARG, "mfma_probe: iters > 0 and a device sink are required");
    const int ncu = visrep_cu_count();
    if (flop) *flop = (double)ncu * 8.0 * iters * 32.0 * 16384.0;
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(ncu), dim3(512), 0, (hipStream_t)stream, (float*)sink, iters, random);
    return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, "mfma_probe: launch failed");
}

extern "C" int visrep_set_gemm_variant(int variant) {            // per-thread (see visrep_internal.h); returns the previous value
#ifdef VISREP_EXPERIMENTS
    const bool ok = variant >= 1 && variant <= 8;
#else
    const bool ok = variant == 1 || variant == 2 || variant == 5 || variant == 6 || variant == 7 || variant == 8;
#endif
    if (!ok) return visrep_set_error(VISREP_ERR_ARG, "gemm variant must be 1, 2, 5, 6, 7 or 8 (3 / 4: VISREP_EXPERIMENTS builds only)");
    const int old = t_visrep_gemm_variant;
    t_visrep_gemm_variant = variant;
    return old;
}

extern "C" int visrep_debug_gemm_ablation(int mask) {   // timing experiments only: results are WRONG when mask != 0
    const int old = g_visrep_gemm_dbg;
    g_visrep_gemm_dbg = mask;
    return old;
}

extern "C" int visrep_debug_gemm_timing_buffer(void* dev_u64x16) {   // ablation builds only: 16 x u64 per-segment cycle sums
    g_visrep_gemm_dbg_buf = (unsigned long long*)dev_u64x16;
    return 0;
}

extern "C" size_t visrep_last_error(char* buf, size_t n) {
    const size_t len = strlen(g_err);
    if (buf && n) {
        const size_t c = len < n - 1 ? len : n - 1;
        memcpy(buf, g_err, c);
        buf[c] = 0;
    }
    return len;
}

extern "C" int visrep_device_cu_count(void) { return visrep_cu_count(); }

extern "C" int visrep_set_scratch(void* ptr, size_t bytes) {
    if ((ptr == nullptr) != (bytes == 0)) return visrep_set_error(VISREP_ERR_ARG, "set_scratch: pass (ptr, bytes) or (NULL, 0)");
    if ((size_t)ptr & 15) return visrep_set_error(VISREP_ERR_ARG, "set_scratch: pointer must be 16-byte aligned");
    return visrep_scratch_register(true, nullptr, ptr, bytes);   // device-wide registration of the CURRENT device
}

extern "C" int visrep_set_stream_scratch(void* stream, void* ptr, size_t bytes) {
    if ((ptr == nullptr) != (bytes == 0)) return visrep_set_error(VISREP_ERR_ARG, "set_stream_scratch: pass (ptr, bytes) or (NULL, 0)");
    if ((size_t)ptr & 15) return visrep_set_error(VISREP_ERR_ARG, "set_stream_scratch: pointer must be 16-byte aligned");
    return visrep_scratch_register(false, (hipStream_t)stream, ptr, bytes);   // keyed by (current device, stream)
}

// Output / residual alignment the GEMM epilogues are written for (8-byte stores and residual loads at the least; fp32 outputs are stored
// 16 bytes at a time).  Every in-tree caller passes whole rows of an allocation or a column window at a multiple of 4 elements; anything less
// is refused before a launch, as visrep_gemm_bf16_gated always did.
static int gemm_refuse_misaligned(const char* who, const void* C, const void* resid, bool f32_out) {   // 0 = aligned, else the error code
    const char* why = ((uintptr_t)C & (f32_out ? 15 : 7)) ? (f32_out ? "C must be 16-byte aligned for EPI_F32" : "C must be 8-byte aligned")
                      : ((uintptr_t)resid & 7) ? "resid must be 8-byte aligned" : nullptr;
    if (!why) return 0;
    char msg[96];
    snprintf(msg, sizeof msg, "%s: %s", who, why);
    return visrep_set_error(VISREP_ERR_ARG, msg);
}

extern "C" int visrep_gemm_bf16(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, int M, int N,
                                int K, int epilogue, int act, const void* resid, const float* ls, void* stream) {
    if (!A || !W || !C) return visrep_set_error(VISREP_ERR_ARG, "gemm: null pointer");
    if (epilogue == VISREP_EPI_PATCH) return visrep_set_error(VISREP_ERR_ARG, "gemm: EPI_PATCH is internal to visrep_vit_forward");
    if (epilogue == VISREP_EPI_RESID && !resid) return visrep_set_error(VISREP_ERR_ARG, "gemm: EPI_RESID needs resid");
    if (const int rc = gemm_refuse_misaligned("gemm", C, epilogue == VISREP_EPI_RESID ? resid : nullptr, epilogue == VISREP_EPI_F32)) return rc;
    GemmArgs a{};
    a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = (bf16_t*)C; a.bias = bias;
    a.resid = (const bf16_t*)resid; a.ls = ls; a.pos = nullptr;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.epi = epilogue; a.act = act;
    return visrep_gemm_dispatch(a, (hipStream_t)stream);
}

extern "C" int visrep_gemm_bf16_ln(const void* A, int lda, const void* W, int ldw, const float* bias, const void* ln_rt, const float* ln_s,
                                   void* C, int ldc, int M, int N, int K, int epilogue, int act, void* stream) {
    if (!A || !W || !C || !ln_rt || !ln_s) return visrep_set_error(VISREP_ERR_ARG, "gemm_ln: null pointer");
    if (epilogue != VISREP_EPI_BIAS && epilogue != VISREP_EPI_ACT && epilogue != VISREP_EPI_VT)
        return visrep_set_error(VISREP_ERR_ARG, "gemm_ln: epilogue must be BIAS, ACT or VT");
    if (const int rc = gemm_refuse_misaligned("gemm_ln", C, nullptr, false)) return rc;
    GemmArgs a{};
    a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = (bf16_t*)C; a.bias = bias; a.ln_rt = (const float2*)ln_rt; a.ln_s = ln_s;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.epi = epilogue; a.act = act;
    return visrep_gemm_dispatch(a, (hipStream_t)stream);
}

extern "C" int visrep_gemm_bf16_gated(const void* A, int lda, const void* W, int ldw, const float* bias, const void* ln_rt, const float* ln_s,
                                      void* C, int ldc, int M, int N, int K, void* stream) {
    if (!A || !W || !C || ((ln_rt == nullptr) != (ln_s == nullptr))) return visrep_set_error(VISREP_ERR_ARG, "gemm_gated: null pointer (ln_rt and ln_s come together)");
    if ((uintptr_t)C & 7) return visrep_set_error(VISREP_ERR_ARG, "gemm_gated: C must be 8-byte aligned");
    GemmArgs a{};
    a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = (bf16_t*)C; a.bias = bias; a.ln_rt = (const float2*)ln_rt; a.ln_s = ln_s;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.epi = EPI_GATED;
    return visrep_gemm_dispatch(a, (hipStream_t)stream);
}

thread_local int t_visrep_fuse_gate = 1;
extern "C" int visrep_set_fuse_gate(int on) {
    const int old = t_visrep_fuse_gate;
    t_visrep_fuse_gate = on ? 1 : 0;
    return old;
}

extern "C" int visrep_debug_gated_refusal(int which) {
    static char dummy[64];                                       // never dereferenced: every combination below is refused before a launch
    GemmArgs a{};
    a.A = (const bf16_t*)dummy; a.W = (const bf16_t*)dummy; a.C = (bf16_t*)dummy;
    a.M = 256; a.N = 256; a.K = 64; a.lda = 64; a.ldw = 64; a.ldc = 128; a.epi = EPI_GATED;
    switch (which) {
        case 1: a.conv = 1; a.cH = a.cW = a.cHo = a.cWo = 16; a.cC = 64; a.cstride = 1; a.cpad = 1; a.K = 576; break;
        case 2: a.a_period = 4; a.a_stride = 8; a.a_first = 0; break;
        case 3: a.stat_rt = (float2*)dummy; a.stat_partial = (float2*)dummy; break;
        case 4: a.gn_partial = (float2*)dummy; a.gn_cpg = 4; a.gn_hw = 128; break;
        default: return visrep_set_error(VISREP_ERR_ARG, "debug_gated_refusal: which must be 1 .. 4");
    }
    const long before = t_visrep_routes[VISREP_ROUTE_GEMM_256] + t_visrep_routes[VISREP_ROUTE_GEMM_128] + t_visrep_routes[VISREP_ROUTE_SPLITK];
    const int rc = visrep_gemm_dispatch(a, nullptr);
    const long after = t_visrep_routes[VISREP_ROUTE_GEMM_256] + t_visrep_routes[VISREP_ROUTE_GEMM_128] + t_visrep_routes[VISREP_ROUTE_SPLITK];
    if (rc == 0 || after != before) { visrep_set_error(VISREP_ERR_ARG, "debug_gated_refusal: the dispatcher accepted the combination"); return 1; }
    return rc;
}

extern "C" int visrep_gemm_bf16_rows(const void* A, int lda, int row_period, int row_stride, int row_first, const void* W, int ldw,
                                     const float* bias, const void* ln_rt, const float* ln_s, void* C, int ldc, int M, int N, int K, int epilogue,
                                     int act, void* stream) {
    if (!A || !W || !C || ((ln_rt == nullptr) != (ln_s == nullptr))) return visrep_set_error(VISREP_ERR_ARG, "gemm_rows: null pointer");
    if (row_period <= 0 || row_stride < row_period || row_first < 0) return visrep_set_error(VISREP_ERR_ARG, "gemm_rows: bad row map");
    if (epilogue == VISREP_EPI_VT && row_period % 4) return visrep_set_error(VISREP_ERR_ARG, "gemm_rows: EPI_VT needs row_period % 4 == 0");
    if (const int rc = gemm_refuse_misaligned("gemm_rows", C, nullptr, epilogue == VISREP_EPI_F32)) return rc;
    GemmArgs a{};
    a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = (bf16_t*)C; a.bias = bias; a.ln_rt = (const float2*)ln_rt; a.ln_s = ln_s;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.epi = epilogue; a.act = act;
    a.a_period = row_period; a.a_stride = row_stride; a.a_first = row_first;
    return visrep_gemm_dispatch(a, (hipStream_t)stream);
}

extern "C" int visrep_gemm_bf16_resid_stats(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, int M, int N,
                                            int K, const void* resid, const float* ls, void* rt, void* partial, float eps, void* stream) {
    if (!A || !W || !C || !resid || !rt || !partial) return visrep_set_error(VISREP_ERR_ARG, "gemm_resid_stats: null pointer");
    if (N > 2048) return visrep_set_error(VISREP_ERR_SHAPE, "gemm_resid_stats: N <= 2048");
    if (const int rc = gemm_refuse_misaligned("gemm_resid_stats", C, resid, false)) return rc;
    GemmArgs a{};
    a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = (bf16_t*)C; a.bias = bias; a.resid = (const bf16_t*)resid; a.ls = ls;
    a.stat_rt = (float2*)rt; a.stat_partial = (float2*)partial; a.stat_eps = eps;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.epi = EPI_RESID;
    return visrep_gemm_dispatch(a, (hipStream_t)stream);
}

extern "C" int visrep_gemm_bf16_resid_rms_stats(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, int M, int N,
                                                int K, const void* resid, const float* ls, void* rt, void* partial, float eps, void* stream) {
    if (!A || !W || !C || !resid || !rt || !partial) return visrep_set_error(VISREP_ERR_ARG, "gemm_resid_rms_stats: null pointer");
    if (N > 4096 || N % 8) return visrep_set_error(VISREP_ERR_SHAPE, "gemm_resid_rms_stats: N <= 4096, N % 8 == 0");
    if (ldc % 8 || ((uintptr_t)C & 15)) return visrep_set_error(VISREP_ERR_SHAPE, "gemm_resid_rms_stats: C must be 16-byte aligned with ldc % 8 == 0");
    GemmArgs a{};
    a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = (bf16_t*)C; a.bias = bias; a.resid = (const bf16_t*)resid; a.ls = ls;
    a.stat_rt = (float2*)rt; a.stat_partial = (float2*)partial; a.stat_eps = eps; a.stat_rms = 1;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.epi = EPI_RESID;
    return visrep_gemm_dispatch(a, (hipStream_t)stream);
}

extern "C" int visrep_conv3x3_bf16(const void* x, int B, int H, int W, int C, const void* Wt, int ldw, const float* bias, void* out, int ldc,
                                   int Cout, int stride, int pad_mode, int upsample, int epilogue, const void* resid, void* stream) {
    if (!x || !Wt || !out) return visrep_set_error(VISREP_ERR_ARG, "conv3x3: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || Cout <= 0) return visrep_set_error(VISREP_ERR_SHAPE, "conv3x3: empty problem");
    if (C % 64) return visrep_set_error(VISREP_ERR_SHAPE, "conv3x3: C must be a multiple of 64 (use visrep_im2col3x3 + visrep_gemm_bf16 otherwise)");
    if ((stride != 1 && stride != 2) || (pad_mode != 0 && pad_mode != 1) || (upsample != 0 && upsample != 1))
        return visrep_set_error(VISREP_ERR_ARG, "conv3x3: stride 1|2, pad_mode 0 (symmetric 1) | 1 (0,1,0,1), upsample 0|1");
    if (epilogue != VISREP_EPI_BIAS && epilogue != VISREP_EPI_RESID && epilogue != VISREP_EPI_F32)
        return visrep_set_error(VISREP_ERR_ARG, "conv3x3: epilogue must be BIAS, RESID or F32");
    if (epilogue == VISREP_EPI_RESID && !resid) return visrep_set_error(VISREP_ERR_ARG, "conv3x3: EPI_RESID needs resid");
    const int Hl = H << upsample, Wl = W << upsample, pad_total = pad_mode == 0 ? 2 : 1;
    GemmArgs a{};
    a.A = (const bf16_t*)x; a.W = (const bf16_t*)Wt; a.C = (bf16_t*)out; a.bias = bias; a.resid = (const bf16_t*)resid;
    a.conv = 1; a.cH = H; a.cW = W; a.cC = C; a.cstride = stride; a.cpad = pad_mode == 0 ? 1 : 0; a.cup = upsample;
    a.cHo = (Hl + pad_total - 3) / stride + 1;
    a.cWo = (Wl + pad_total - 3) / stride + 1;
    a.M = B * a.cHo * a.cWo; a.N = Cout; a.K = 9 * C; a.lda = 8; a.ldw = ldw; a.ldc = ldc; a.epi = epilogue;
    return visrep_gemm_dispatch(a, (hipStream_t)stream);
}

// Rows and groups must fit the epilogue's slots (64-row slots inside one image, a group inside a lane quad pair / quartet), and asking for the
// sums must not cost the convolution its kernel: the 128x128 kernel emits them from its epilogue for both epilogues, the 256x256 kernel (whole
// rounds of its tiles, Cout % 256 == 0) for EPI_BIAS (round 5: a pass over the accumulators in front of the epilogue); a residual
// convolution there keeps the separate statistics pass unless VISREP_GN_RESID_256=1 (round 6: built, measured slower, opt-in).  visrep_conv_gn_supported is the round-4 query (no epilogue argument: the
// conservative answer that holds for both).
extern "C" int visrep_conv_gn_supported_epi(int B, int HWo, int Cout, int groups, int epilogue) {
    if (B <= 0 || HWo <= 0 || Cout <= 0 || groups <= 0 || Cout % groups) return 0;
    if (epilogue != VISREP_EPI_BIAS && epilogue != VISREP_EPI_RESID) return 0;
    const int cpg = Cout / groups;
    if (!(HWo % 128 == 0 && Cout % 64 == 0 && (cpg == 4 || cpg == 8 || cpg == 16))) return 0;
    // residual convolutions that the 256x256 kernel takes: round 6 built their partial sums too (gemm_gn_partials_prepass<.., RES>: the pre-pass reads
    // the residual tile as well) and measured the SD1.5 forward 0.4-0.6 ms SLOWER with them than with the separate statistics pass (70.8 / 71.0 ->
    // 71.2 / 71.6 ms, tools/diag/ab_gn_resid256.sh: the second fetch of the residual tile + 7 spilled registers cost what the pass saved) - opt-in:
    // VISREP_GN_RESID_256=1 (read per call, so that tests can switch it)
    const char* e_ = getenv("VISREP_GN_RESID_256");
    const bool resid256 = e_ && e_[0] == '1';
    if (!resid256 && epilogue != VISREP_EPI_BIAS && Cout % 256 == 0 && ((long)B * HWo + 255) / 256 * (Cout / 256) >= 2L * visrep_cu_count()) return 0;
    return 1;
}
extern "C" int visrep_conv_gn_supported(int B, int HWo, int Cout, int groups) {
    return visrep_conv_gn_supported_epi(B, HWo, Cout, groups, VISREP_EPI_RESID);
}

extern "C" size_t visrep_conv_gn_partial_bytes(int B, int HWo, int groups) {
    return (B > 0 && HWo > 0 && groups > 0) ? (size_t)B * (HWo / 64) * groups * sizeof(float2) : 0;
}

extern "C" int visrep_conv3x3_bf16_gn(const void* x, int B, int H, int W, int C, const void* Wt, int ldw, const float* bias, void* out, int ldc,
                                      int Cout, int stride, int pad_mode, int epilogue, const void* resid, void* gn_partial, int groups, void* stream) {
    if (!x || !Wt || !out || !gn_partial) return visrep_set_error(VISREP_ERR_ARG, "conv3x3_gn: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || Cout <= 0) return visrep_set_error(VISREP_ERR_SHAPE, "conv3x3_gn: empty problem");
    if (C % 64) return visrep_set_error(VISREP_ERR_SHAPE, "conv3x3_gn: C must be a multiple of 64");
    if ((stride != 1 && stride != 2) || (pad_mode != 0 && pad_mode != 1)) return visrep_set_error(VISREP_ERR_ARG, "conv3x3_gn: stride 1|2, pad_mode 0|1");
    if (epilogue != VISREP_EPI_BIAS && epilogue != VISREP_EPI_RESID) return visrep_set_error(VISREP_ERR_ARG, "conv3x3_gn: epilogue must be BIAS or RESID");
    if (epilogue == VISREP_EPI_RESID && !resid) return visrep_set_error(VISREP_ERR_ARG, "conv3x3_gn: EPI_RESID needs resid");
    const int pad_total = pad_mode == 0 ? 2 : 1;
    GemmArgs a{};
    a.A = (const bf16_t*)x; a.W = (const bf16_t*)Wt; a.C = (bf16_t*)out; a.bias = bias; a.resid = (const bf16_t*)resid;
    a.conv = 1; a.cH = H; a.cW = W; a.cC = C; a.cstride = stride; a.cpad = pad_mode == 0 ? 1 : 0; a.cup = 0;
    a.cHo = (H + pad_total - 3) / stride + 1;
    a.cWo = (W + pad_total - 3) / stride + 1;
    if (!visrep_conv_gn_supported_epi(B, a.cHo * a.cWo, Cout, groups, epilogue))
        return visrep_set_error(VISREP_ERR_SHAPE, "conv3x3_gn: needs Ho Wo % 128 == 0, 4 | 8 | 16 channels per group and a kernel that emits the sums for this epilogue (see visrep_conv_gn_supported_epi)");
    a.M = B * a.cHo * a.cWo; a.N = Cout; a.K = 9 * C; a.lda = 8; a.ldw = ldw; a.ldc = ldc; a.epi = epilogue;
    a.gn_partial = (float2*)gn_partial; a.gn_cpg = Cout / groups; a.gn_hw = a.cHo * a.cWo;
    return visrep_gemm_dispatch(a, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ ViT forward
namespace {
inline size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }
struct Ws {
    size_t h, qk, vt, vcls, mlp, rt, part, total;
    int ldvt;
};
// true and padded head width of the bf16 tower (0 = derived: d / heads, no padding) and the attention side's width da = heads * padded
inline int vit_head_dim(const visrep_vit_config* c) { return c->head_dim > 0 ? c->head_dim : (c->heads > 0 ? c->d / c->heads : 0); }
inline int vit_head_pad(const visrep_vit_config* c) { return c->head_pad > 0 ? c->head_pad : vit_head_dim(c); }
Ws layout(const visrep_vit_config* c, int B) {
    Ws w;
    const size_t M = (size_t)B * c->tokens;
    const size_t Mp = up(M, 128);
    const size_t da = (size_t)c->heads * vit_head_pad(c), dh = da > (size_t)c->d ? da : (size_t)c->d;   // da == d for 64-wide heads
    w.ldvt = (int)(up(M, 64) + 64);
    size_t off = 0;
    w.h = off;   off += up(Mp * dh * 2, 256);                       // LayerNorm output [M, d] / attention output [M, da]
    w.qk = off;  off += up(Mp * 2 * da * 2, 256);
    w.vt = off;  off += up(da * w.ldvt * 2, 256);
    w.vcls = off; off += up((size_t)B * (1 + (c->registers > 0 ? c->registers : 0)) * da * 2, 256);   // V rows of the CLS (and register) tokens (image-aligned attention)
    // SwiGLU towers: the gated fc1 writes [Mp, mlp] like every other activation; the unfused A/B route (visrep_set_fuse_gate(0)) keeps the
    // [Mp, 2 mlp] GEMM output in front of it
    const size_t mlp_b = Mp * c->mlp * 2 * ((c->act == VISREP_ACT_SWIGLU && !t_visrep_fuse_gate) ? 3 : 1);
    const size_t cols_b = up((size_t)B * (c->tokens - c->has_cls - c->registers), 128) * c->kpad * 2;
    w.mlp = off; off += up(mlp_b > cols_b ? mlp_b : cols_b, 256);   // im2col columns alias the MLP buffer
    w.rt = off;  off += up((Mp + 8) * sizeof(float2), 256);         // folded-LayerNorm row statistics (zero past M)
    w.part = off; off += up(Mp * (c->d / 64) * sizeof(float2), 256);  // per-row partial sums left by the residual GEMM epilogues
    w.total = off;
    return w;
}
}  // namespace

extern "C" size_t visrep_vit_workspace_bytes(const visrep_vit_config* cfg, int B) {
    if (!cfg || B <= 0) return 0;
    return layout(cfg, B).total;
}

#define VR_TRY(x) do { const int rc_ = (x); if (rc_) return rc_; } while (0)

extern "C" int visrep_vit_forward(const visrep_vit_config* c, const visrep_vit_weights* w, const void* pixels, int pixel_dtype,
                                  void* hidden, int B, int n_layers, void* workspace, void* stream) {
    if (!c || !w || !pixels || !hidden || !workspace) return visrep_set_error(VISREP_ERR_ARG, "vit_forward: null pointer");
    if (B <= 0) return 0;
    if (n_layers < 0 || n_layers > c->layers) return visrep_set_error(VISREP_ERR_ARG, "vit_forward: n_layers out of range");
    const int hd = vit_head_dim(c), dp = vit_head_pad(c);
    if (c->heads <= 0 || c->d != c->heads * hd) return visrep_set_error(VISREP_ERR_SHAPE, "vit_forward: d must be heads * head_dim");
    if (dp > 128) return visrep_set_error(VISREP_ERR_SHAPE, "vit_forward: head_dim above 128 is not supported (head_pad must be 64, 96 or 128)");
    if ((dp != 64 && dp != 96 && dp != 128) || hd > dp)
        return visrep_set_error(VISREP_ERR_SHAPE, "vit_forward: head_pad must be 64, 96 or 128 and >= head_dim (the packer zero-pads every head)");
    if (dp != 64 && c->q_prescaled) return visrep_set_error(VISREP_ERR_ARG, "vit_forward: pre-scaled Q (q_prescaled != 0) is built for head_pad 64");
    if (c->d % 128 || c->mlp % 128 || c->kpad % 64)
        return visrep_set_error(VISREP_ERR_SHAPE, "vit_forward: d, mlp % 128 and kpad % 64 required (mlp = the zero-padded MLP width)");
    const int grid = c->image_size / c->patch;
    if (c->registers < 0 || (c->registers > 0 && !c->has_cls)) return visrep_set_error(VISREP_ERR_SHAPE, "vit_forward: register tokens need a CLS token (registers >= 0)");
    const int prefix = (c->has_cls ? 1 : 0) + c->registers;       // non-patch rows in front of every image's patches
    if (grid * grid + prefix != c->tokens) return visrep_set_error(VISREP_ERR_SHAPE, "vit_forward: tokens != grid^2 + cls + registers");
    if (c->has_cls && !w->cls) return visrep_set_error(VISREP_ERR_ARG, "vit_forward: a CLS tower needs the cls table");
    if (c->act < VISREP_ACT_NONE || c->act > VISREP_ACT_SWIGLU) return visrep_set_error(VISREP_ERR_ARG, "vit_forward: unknown activation code");
    if (c->norm != 0 && c->norm != 1) return visrep_set_error(VISREP_ERR_ARG, "vit_forward: norm must be 0 (LayerNorm) or 1 (RMSNorm)");
    const bool rms = c->norm == 1;
    if (rms && c->pre_ln) return visrep_set_error(VISREP_ERR_ARG, "vit_forward: pre_ln with RMSNorm blocks is not supported");
    if (rms && c->d > 4096) return visrep_set_error(VISREP_ERR_SHAPE, "vit_forward: RMSNorm blocks need d <= 4096");
    if (c->qk_norm) {
        if (c->heads * dp > 4096) return visrep_set_error(VISREP_ERR_SHAPE, "vit_forward: qk_norm needs heads * head_pad <= 4096");
        for (int l = 0; l < n_layers; ++l)
            if (!w->layers[l].qn_g || !w->layers[l].kn_g) return visrep_set_error(VISREP_ERR_ARG, "vit_forward: a qk_norm tower needs qn_g and kn_g in every layer");
    }
    hipStream_t s = (hipStream_t)stream;
    const Ws L = layout(c, B);
    char* base = (char*)workspace;
    bf16_t* x = (bf16_t*)hidden;
    bf16_t* h = (bf16_t*)(base + L.h);
    bf16_t* qk = (bf16_t*)(base + L.qk);
    bf16_t* vt = (bf16_t*)(base + L.vt);
    bf16_t* vcls = (bf16_t*)(base + L.vcls);
    bf16_t* mlp = (bf16_t*)(base + L.mlp);
    const int d = c->d, T = c->tokens, P = grid * grid, M = B * T;
    const int da = c->heads * dp;                         // width of Q, of K, of V and of the attention output (== d when dp == 64 == head_dim)

    // ---- embeddings: conv(k = s = patch) as im2col + GEMM with fused (bias, position add, CLS row skip)
    VR_TRY(visrep_im2col(pixels, pixel_dtype, mlp, B, c->image_size, c->image_size, c->patch, c->kpad, stream));
    GemmArgs g{};
    g.A = mlp; g.lda = c->kpad; g.W = (const bf16_t*)w->patch_w; g.ldw = c->kpad; g.C = x; g.ldc = d;
    g.bias = w->patch_b; g.pos = w->pos; g.M = B * P; g.N = d; g.K = c->kpad; g.epi = EPI_PATCH;
    g.patches = P; g.tokens = T; g.cls_off = prefix;
    VR_TRY(visrep_gemm_dispatch(g, s));
    if (prefix == 1) VR_TRY(visrep_cls_rows(x, d, w->cls, w->pos, B, T, d, stream));
    else if (prefix > 1) VR_TRY(visrep_prefix_rows(x, d, w->cls, w->pos, B, T, prefix, d, stream));
    if (c->pre_ln) VR_TRY(visrep_layernorm(x, d, w->pre_ln_g, w->pre_ln_b, x, d, M, d, c->eps, stream));

    // V^T columns past B*T are read (with zero softmax weight) by the last key tile: keep them finite
    if (hipMemsetAsync(vt, 0, (size_t)da * L.ldvt * 2, s) != hipSuccess) return visrep_set_error(VISREP_ERR_LAUNCH, "vit_forward: memset failed");

    float2* rt = (float2*)(base + L.rt);
    if (hipMemsetAsync(rt, 0, (up(M, 128) + 8) * sizeof(float2), s) != hipSuccess) return visrep_set_error(VISREP_ERR_LAUNCH, "vit_forward: memset failed");

    float2* part = (float2*)(base + L.part);
    const float scale = c->q_prescaled ? 0.f : 1.f / sqrtf((float)hd);   // the TRUE head_dim^-0.5 (64: 0.125 exactly); 0 = folded into the Q weights (attn_fwd PS)
    // Image-aligned attention (attn_fwd_cls): the patch tokens of an image are whole key tiles and the CLS key is a side term, so V is
    // projected by two row-mapped GEMMs - the patch rows into V^T (column b (T - 1) + t - 1), the CLS rows into vcls [B, d]
    const bool side = c->q_prescaled >= 2 && dp == 64 && hd == 64 && t_visrep_attn_variant == 1;
    const bool aligned = side && prefix == 1 && visrep_mhsa_cls_supported(T);
    // the same with CLS + registers as a prefix of side keys (attn_fwd_prefix): patch rows -> V^T column b P + t - prefix, prefix rows -> vcls [B prefix, d]
    const bool aligned_pre = side && prefix >= 2 && visrep_mhsa_prefix_supported(T, prefix);
    bool rt_ready = false;        // rt already holds the statistics of x (left by the previous layer's fc2 GEMM)
    for (int l = 0; l < n_layers; ++l) {
        const visrep_vit_layer& W = w->layers[l];
        const bool fold = W.sqkv && W.s1;     // LayerNorm folded into the QK / V / fc1 GEMMs: only its statistics are computed,
        const bool fold_next = l + 1 < n_layers && w->layers[l + 1].sqkv && w->layers[l + 1].s1;   // and those by the GEMM that writes x
        GemmArgs a{};
        if (fold) {
            if (!rt_ready) VR_TRY(rms ? visrep_rmsnorm_stats(x, d, rt, M, d, c->eps, stream) : visrep_layernorm_stats(x, d, rt, M, d, c->eps, stream));
            a.A = x; a.ln_rt = rt; a.ln_s = W.sqkv;
        } else {
            VR_TRY(rms ? visrep_rmsnorm(x, d, W.ln1_g, h, d, M, d, c->eps, stream) : visrep_layernorm(x, d, W.ln1_g, W.ln1_b, h, d, M, d, c->eps, stream));
            a.A = h;
        }
        a.lda = d; a.K = d; a.M = M;
        // Q | K projection
        a.W = (const bf16_t*)W.wqkv; a.ldw = d; a.N = 2 * da; a.C = qk; a.ldc = 2 * da; a.bias = W.bqkv; a.epi = EPI_BIAS;
        VR_TRY(visrep_gemm_dispatch(a, s));
        // QK normalisation over the whole width, in place, before any attention route reads Q | K
        if (c->qk_norm) VR_TRY(visrep_qk_rmsnorm(qk, 2 * da, da, d, W.qn_g, W.kn_g, M, VISREP_QK_NORM_EPS, stream));
        // V projection written transposed + perm16 for the attention kernel
        a.W = (const bf16_t*)W.wqkv + (size_t)2 * da * d; a.N = da; a.C = vt; a.ldc = L.ldvt; a.bias = W.bqkv + 2 * da; a.epi = EPI_VT;
        if (fold) a.ln_s = W.sqkv + 2 * da;
        if (aligned) {
            GemmArgs v = a;
            v.M = B * (T - 1); v.a_period = T - 1; v.a_stride = T; v.a_first = 1;
            VR_TRY(visrep_gemm_dispatch(v, s));
            v.M = B; v.a_period = 1; v.a_first = 0; v.C = vcls; v.ldc = d; v.epi = EPI_BIAS;
            VR_TRY(visrep_gemm_dispatch(v, s));
            VR_TRY(visrep_mhsa_cls_fwd(qk, 2 * d, vt, L.ldvt, vcls, d, h, d, B, T, c->heads, 64, stream));
        } else if (aligned_pre) {
            GemmArgs v = a;
            v.M = B * P; v.a_period = P; v.a_stride = T; v.a_first = prefix;
            VR_TRY(visrep_gemm_dispatch(v, s));
            v.M = B * prefix; v.a_period = prefix; v.a_first = 0; v.C = vcls; v.ldc = d; v.epi = EPI_BIAS;
            VR_TRY(visrep_gemm_dispatch(v, s));
            VR_TRY(visrep_mhsa_prefix_fwd(qk, 2 * d, vt, L.ldvt, vcls, d, h, d, B, T, prefix, c->heads, 64, stream));
        } else {
            VR_TRY(visrep_gemm_dispatch(a, s));
            VR_TRY(visrep_mhsa_fwd(qk, 2 * da, vt, L.ldvt, h, da, B, T, c->heads, dp, scale, stream));
        }
        // out projection + LayerScale + residual (in place on x)
        a.A = h; a.lda = da; a.K = da; a.ldw = da; a.ln_rt = nullptr; a.ln_s = nullptr;
        a.W = (const bf16_t*)W.wo; a.N = d; a.C = x; a.ldc = d; a.bias = W.bo; a.epi = EPI_RESID; a.resid = x; a.ls = W.ls1;
        if (fold) { a.stat_rt = rt; a.stat_partial = part; a.stat_eps = c->eps; a.stat_rms = rms; }   // LN2's statistics come out of this GEMM
        VR_TRY(visrep_gemm_dispatch(a, s));
        GemmArgs f{};
        if (fold) {
            f.A = x; f.ln_rt = rt; f.ln_s = W.s1;
        } else {
            VR_TRY(rms ? visrep_rmsnorm(x, d, W.ln2_g, h, d, M, d, c->eps, stream) : visrep_layernorm(x, d, W.ln2_g, W.ln2_b, h, d, M, d, c->eps, stream));
            f.A = h;
        }
        f.lda = d; f.K = d; f.M = M; f.W = (const bf16_t*)W.w1; f.ldw = d; f.N = c->mlp; f.C = mlp; f.ldc = c->mlp;
        f.bias = W.b1; f.epi = EPI_ACT; f.act = c->act;
        if (c->act == VISREP_ACT_SWIGLU) {                   // HF Dinov2SwiGLUFFN: w1 has 2 mlp rows
            f.N = 2 * c->mlp; f.act = 0;
            if (t_visrep_fuse_gate) {                            // gate in the epilogue: the [M, 2 mlp] intermediate never exists (w1 interleaved)
                f.epi = EPI_GATED;
                VR_TRY(visrep_gemm_dispatch(f, s));
            } else {                                             // A/B baseline: plain GEMM behind the hidden buffer, then the element-wise pass (w1 in HF order)
                bf16_t* gu = mlp + up(M, 128) * (size_t)c->mlp;
                f.epi = EPI_BIAS; f.C = gu; f.ldc = 2 * c->mlp;
                VR_TRY(visrep_gemm_dispatch(f, s));
                VR_TRY(visrep_swiglu(gu, 2 * c->mlp, mlp, c->mlp, M, c->mlp, stream));
            }
        } else
        VR_TRY(visrep_gemm_dispatch(f, s));
        f.ln_rt = nullptr; f.ln_s = nullptr;
        f.A = mlp; f.lda = c->mlp; f.K = c->mlp; f.W = (const bf16_t*)W.w2; f.ldw = c->mlp; f.N = d; f.C = x; f.ldc = d;
        f.bias = W.b2; f.epi = EPI_RESID; f.act = 0; f.resid = x; f.ls = W.ls2;
        if (fold_next) { f.stat_rt = rt; f.stat_partial = part; f.stat_eps = c->eps; f.stat_rms = rms; }   // the next layer's LN1
        rt_ready = fold_next;
        VR_TRY(visrep_gemm_dispatch(f, s));
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ ConvNeXt forward
namespace {
struct CnWs { size_t x, y, h, rt, part, total; };
inline int cn_wp(int c) { return (c + 127) / 128 * 128; }
CnWs cn_layout(const visrep_convnext_config* c, int B) {
    CnWs w;
    size_t ex = 0, ey = 0, eh = 0, ep = 0, side = (size_t)c->image_size / 4;
    const size_t M0 = up((size_t)B * side * side, 256);
    eh = M0 * c->kpad;                                               // the stem's im2col columns alias the pwconv1 output
    for (int s = 0; s < 4; ++s) {                                    // elements each buffer needs at its largest stage; rows padded to whole 256-row tiles
        if (s) side /= 2;
        const size_t M = up((size_t)B * side * side, 256), C = c->widths[s];
        ex = std::max(ex, M * cn_wp((int)C));                        // residual stream [M_s, wp(s)]
        ey = std::max(ey, M * std::max(C, s ? (size_t)4 * c->widths[s - 1] : C));   // dwconv output [M_s, C_s] / space-to-depth rows [M_s, 4 C_(s-1)]
        eh = std::max(eh, M * 4 * C);                                // pwconv1 output [M_s, 4 C_s]
        ep = std::max(ep, M * (C / 64));
    }
    size_t off = 0;
    w.x = off;  off += up(ex * 2, 256);
    w.y = off;  off += up(ey * 2, 256);
    w.h = off;  off += up(eh * 2, 256);
    w.rt = off; off += up((M0 + 8) * sizeof(float2), 256);
    w.part = off; off += up(ep * sizeof(float2), 256);
    w.total = off;
    return w;
}
int cn_check(const visrep_convnext_config* c) {
    if (c->image_size <= 0 || c->image_size % 32) return visrep_set_error(VISREP_ERR_SHAPE, "convnext: image_size must be a positive multiple of 32");
    if (c->kpad < 48 || c->kpad % 64) return visrep_set_error(VISREP_ERR_SHAPE, "convnext: kpad must be a multiple of 64 (48 stem taps zero-padded)");
    for (int s = 0; s < 4; ++s) {
        if (c->widths[s] <= 0 || c->widths[s] % 64) return visrep_set_error(VISREP_ERR_SHAPE, "convnext: every stage width must be a multiple of 64");
        if (c->depths[s] < 0) return visrep_set_error(VISREP_ERR_SHAPE, "convnext: negative depth");
    }
    if (c->widths[0] > 2048) return visrep_set_error(VISREP_ERR_SHAPE, "convnext: stem width above 2048 is not supported (visrep_layernorm)");
    return 0;
}
}  // namespace

extern "C" size_t visrep_convnext_workspace_bytes(const visrep_convnext_config* cfg, int B) {
    if (!cfg || B <= 0 || cn_check(cfg)) return 0;
    return cn_layout(cfg, B).total;
}

extern "C" int visrep_convnext_forward(const visrep_convnext_config* c, const visrep_convnext_weights* w, const void* pixels, int pixel_dtype,
                                       void* hidden, int B, int n_stages, void* workspace, void* stream) {
    if (!c || !w || !pixels || !hidden || !workspace || !w->blocks) return visrep_set_error(VISREP_ERR_ARG, "convnext_forward: null pointer");
    if (B <= 0) return 0;
    if (n_stages < 0 || n_stages > 4) return visrep_set_error(VISREP_ERR_ARG, "convnext_forward: n_stages must be 0 .. 4");
    VR_TRY(cn_check(c));
    hipStream_t s = (hipStream_t)stream;
    const CnWs L = cn_layout(c, B);
    char* base = (char*)workspace;
    bf16_t* x = (bf16_t*)(base + L.x);
    bf16_t* y = (bf16_t*)(base + L.y);
    bf16_t* h = (bf16_t*)(base + L.h);
    float2* rt = (float2*)(base + L.rt);
    float2* part = (float2*)(base + L.part);
    int side = c->image_size / 4, C = c->widths[0], Cp = cn_wp(C), M = B * side * side;
    if (hipMemsetAsync(rt, 0, (up((size_t)M, 256) + 8) * sizeof(float2), s) != hipSuccess) return visrep_set_error(VISREP_ERR_LAUNCH, "convnext_forward: memset failed");
    // ---- stem: conv(k = s = 4) as im2col + GEMM, then LayerNorm over the true width (the padded columns of x are and stay zero)
    VR_TRY(visrep_im2col(pixels, pixel_dtype, h, B, c->image_size, c->image_size, 4, c->kpad, stream));
    VR_TRY(visrep_gemm_bf16(h, c->kpad, w->stem_w, c->kpad, w->stem_b, x, Cp, M, Cp, c->kpad, VISREP_EPI_BIAS, 0, nullptr, nullptr, stream));
    VR_TRY(visrep_layernorm(x, Cp, w->stem_ln_g, w->stem_ln_b, x, Cp, M, C, c->eps, stream));
    const visrep_convnext_block* blk = w->blocks;
    for (int st = 0; st < n_stages; ++st) {
        if (st > 0) {                                                // LayerNorm + 2x2 stride-2 convolution: gather kernel + plain GEMM, x is rewritten
            const int Ci = C;
            if (!w->ds_ln_g[st] || !w->ds_ln_b[st] || !w->ds_w[st]) return visrep_set_error(VISREP_ERR_ARG, "convnext_forward: a downsampling layer's weights are missing");
            VR_TRY(visrep_ln_space_to_depth2(x, Cp, w->ds_ln_g[st], w->ds_ln_b[st], y, 4 * Ci, B, side, side, Ci, c->eps, stream));
            side /= 2; C = c->widths[st]; Cp = cn_wp(C); M = B * side * side;
            VR_TRY(visrep_gemm_bf16(y, 4 * Ci, w->ds_w[st], 4 * Ci, w->ds_b[st], x, Cp, M, Cp, 4 * Ci, VISREP_EPI_BIAS, 0, nullptr, nullptr, stream));
        }
        for (int i = 0; i < c->depths[st]; ++i, ++blk) {
            if (!blk->dw_w || !blk->dw_b || !blk->w1 || !blk->s1 || !blk->w2) return visrep_set_error(VISREP_ERR_ARG, "convnext_forward: a block's weights are missing");
            VR_TRY(visrep_dwconv7x7_stats(x, Cp, blk->dw_w, blk->dw_b, y, C, part, rt, B, side, side, C, c->eps, stream));
            VR_TRY(visrep_gemm_bf16_ln(y, C, blk->w1, C, blk->b1, rt, blk->s1, h, 4 * C, M, 4 * C, C, VISREP_EPI_ACT, VISREP_ACT_GELU_ERF, stream));
            VR_TRY(visrep_gemm_bf16(h, 4 * C, blk->w2, 4 * C, blk->b2, x, Cp, M, Cp, 4 * C, VISREP_EPI_RESID, 0, x, blk->ls, stream));
        }
    }
    // hidden is [B, side^2, C] without the padded columns
    if (hipMemcpy2DAsync(hidden, (size_t)C * 2, x, (size_t)Cp * 2, (size_t)C * 2, (size_t)M, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return visrep_set_error(VISREP_ERR_LAUNCH, "convnext_forward: copy of the hidden state failed");
    return 0;
}

// ------------------------------------------------------------------------------------------------ SAM ViT forward
namespace {
constexpr size_t SAM_TABLE_BYTES = (size_t)64 << 20;             // per table (rel_h, rel_w): the image chunk of a layer's attention is sized to it
thread_local size_t t_sam_table_bytes = SAM_TABLE_BYTES;         // visrep_debug_sam_table_bytes
struct SamWs { size_t x, h, ow, qk, vt, qkw, vtw, mlp, rt, part, tab, neck, total; int ldvt, ldvw, nw; long Mw; };
SamWs sam_layout(const visrep_sam_config* c, int B) {
    SamWs w;
    const int g = c->image_size / c->patch, d = c->d;
    const size_t M = (size_t)B * g * g, Mp = up(M, 256);
    w.nw = (g + c->window - 1) / c->window;
    w.Mw = (long)B * w.nw * w.nw * c->window * c->window;
    const size_t Mwp = up((size_t)w.Mw, 256);
    w.ldvt = (int)(up(M, 64) + 64);
    w.ldvw = (int)(up((size_t)w.Mw, 64) + 64);
    size_t off = 0;
    w.x = off;   off += up(Mp * d * 2, 256);                        // residual stream
    w.h = off;   off += up(Mp * d * 2, 256);                        // attention output, map rows
    w.ow = off;  off += up(Mwp * d * 2, 256);                       // attention output of a windowed layer, window rows
    w.qk = off;  off += up(Mp * 2 * d * 2, 256);
    w.vt = off;  off += up((size_t)d * w.ldvt * 2, 256);
    w.qkw = off; off += up(Mwp * 2 * d * 2, 256);                   // windowed Q | K
    w.vtw = off; off += up((size_t)d * w.ldvw * 2, 256);
    const size_t mlp_b = Mp * c->mlp * 2, cols_b = Mp * c->kpad * 2;
    w.mlp = off; off += up(std::max(mlp_b, cols_b), 256);
    w.rt = off;  off += up((Mp + 8) * sizeof(float2), 256);
    w.part = off; off += up(Mp * (d / 64 + 1) * sizeof(float2), 256);
    w.tab = off; off += 2 * SAM_TABLE_BYTES;
    w.neck = off; off += up(2 * Mp * c->out_ch * 2, 256);
    w.total = off;
    return w;
}
int sam_check(const visrep_sam_config* c) {
    if (c->image_size <= 0 || c->patch <= 0 || c->image_size % c->patch) return visrep_set_error(VISREP_ERR_SHAPE, "sam: image_size must be a positive multiple of patch");
    const int g = c->image_size / c->patch;
    if (c->heads <= 0 || c->d != c->heads * 64) return visrep_set_error(VISREP_ERR_SHAPE, "sam: heads must be 64 wide (d = heads * 64)");
    if (c->d % 128 || c->mlp % 128 || c->kpad % 64 || c->kpad < 3 * c->patch * c->patch) return visrep_set_error(VISREP_ERR_SHAPE, "sam: d, mlp % 128 and kpad % 64 (>= 3 patch^2) required");
    if (c->out_ch <= 0 || c->out_ch % 64 || c->out_ch > 2048) return visrep_set_error(VISREP_ERR_SHAPE, "sam: out_ch must be a multiple of 64, at most 2048");
    if (c->layers < 0 || c->layers > 64) return visrep_set_error(VISREP_ERR_SHAPE, "sam: at most 64 layers (global_mask)");
    if (g < 2 || g > 64) return visrep_set_error(VISREP_ERR_SHAPE, "sam: the patch grid side must be 2 .. 64 (global attention)");
    if (c->window < 2 || c->window > 64) return visrep_set_error(VISREP_ERR_SHAPE, "sam: window must be 2 .. 64");
    return 0;
}
}  // namespace

extern "C" size_t visrep_debug_sam_table_bytes(size_t bytes) {
    const size_t old = t_sam_table_bytes;
    t_sam_table_bytes = bytes == 0 || bytes > SAM_TABLE_BYTES ? SAM_TABLE_BYTES : bytes;
    return old;
}

extern "C" size_t visrep_sam_workspace_bytes(const visrep_sam_config* cfg, int B) {
    if (!cfg || B <= 0 || sam_check(cfg)) return 0;
    return sam_layout(cfg, B).total;
}

extern "C" int visrep_sam_forward(const visrep_sam_config* c, const visrep_sam_weights* w, const void* pixels, int pixel_dtype, void* hidden, int B,
                                  int n_state, void* workspace, void* stream) {
    if (!c || !w || !pixels || !hidden || !workspace || !w->layers) return visrep_set_error(VISREP_ERR_ARG, "sam_forward: null pointer");
    if (B <= 0) return 0;
    VR_TRY(sam_check(c));
    if (n_state < 0 || n_state > c->layers + 1) return visrep_set_error(VISREP_ERR_ARG, "sam_forward: n_state must be 0 .. layers + 1");
    hipStream_t s = (hipStream_t)stream;
    const SamWs L = sam_layout(c, B);
    char* base = (char*)workspace;
    bf16_t* x = (bf16_t*)(base + L.x);
    bf16_t* h = (bf16_t*)(base + L.h);
    bf16_t* ow = (bf16_t*)(base + L.ow);
    bf16_t* qk = (bf16_t*)(base + L.qk);
    bf16_t* vt = (bf16_t*)(base + L.vt);
    bf16_t* qkw = (bf16_t*)(base + L.qkw);
    bf16_t* vtw = (bf16_t*)(base + L.vtw);
    bf16_t* mlp = (bf16_t*)(base + L.mlp);
    float2* rt = (float2*)(base + L.rt);
    float2* part = (float2*)(base + L.part);
    float* tab_h = (float*)(base + L.tab);
    float* tab_w = (float*)(base + L.tab + SAM_TABLE_BYTES);
    const int d = c->d, g = c->image_size / c->patch, P = g * g, M = B * P, H = c->heads, wd = c->window;
    const float scale = 0.125f;

    VR_TRY(visrep_im2col(pixels, pixel_dtype, mlp, B, c->image_size, c->image_size, c->patch, c->kpad, stream));
    GemmArgs e{};
    e.A = mlp; e.lda = c->kpad; e.W = (const bf16_t*)w->patch_w; e.ldw = c->kpad; e.C = x; e.ldc = d;
    e.bias = w->patch_b; e.pos = w->pos; e.M = M; e.N = d; e.K = c->kpad; e.epi = EPI_PATCH; e.patches = P; e.tokens = P; e.cls_off = 0;
    VR_TRY(visrep_gemm_dispatch(e, s));
    // V^T columns that belong to no key are read with zero softmax weight: keep them finite
    if (hipMemsetAsync(vt, 0, (size_t)d * L.ldvt * 2, s) != hipSuccess || hipMemsetAsync(vtw, 0, (size_t)d * L.ldvw * 2, s) != hipSuccess ||
        hipMemsetAsync(rt, 0, (up(M, 256) + 8) * sizeof(float2), s) != hipSuccess)
        return visrep_set_error(VISREP_ERR_LAUNCH, "sam_forward: memset failed");

    const int n_layers = n_state > c->layers ? c->layers : n_state;
    bool rt_ready = false;
    for (int l = 0; l < n_layers; ++l) {
        const visrep_sam_layer& W = w->layers[l];
        if (!W.wqkv || !W.bqkv || !W.sqkv || !W.bqkv_raw || !W.rel_h || !W.rel_w || !W.wo || !W.w1 || !W.s1 || !W.w2)
            return visrep_set_error(VISREP_ERR_ARG, "sam_forward: a layer's weights are missing");
        const bool global = (c->global_mask >> l) & 1ull;
        if (!rt_ready) VR_TRY(visrep_layernorm_stats(x, d, rt, M, d, c->eps, stream));
        GemmArgs a{};
        a.A = x; a.ln_rt = rt; a.ln_s = W.sqkv; a.lda = d; a.K = d; a.M = M;
        a.W = (const bf16_t*)W.wqkv; a.ldw = d; a.N = 2 * d; a.C = qk; a.ldc = 2 * d; a.bias = W.bqkv; a.epi = EPI_BIAS;
        VR_TRY(visrep_gemm_dispatch(a, s));
        a.W = (const bf16_t*)W.wqkv + (size_t)2 * d * d; a.N = d; a.C = vt; a.ldc = L.ldvt; a.bias = W.bqkv + 2 * d; a.epi = EPI_VT; a.ln_s = W.sqkv + 2 * d;
        VR_TRY(visrep_gemm_dispatch(a, s));
        // attention over grids of side S: the whole map, or the windows of the gathered projections; in image chunks that fit the table buffer
        const int S = global ? g : wd, T = S * S, gpi = global ? 1 : L.nw * L.nw;     // grids per image
        const bf16_t* aq = qk; const bf16_t* av = vt; int aldv = L.ldvt; bf16_t* ao = h;
        if (!global) {
            VR_TRY(visrep_sam_window_partition(qk, 2 * d, vt, L.ldvt, W.bqkv_raw, qkw, 2 * d, vtw, L.ldvw, B, g, wd, d, stream));
            aq = qkw; av = vtw; aldv = L.ldvw; ao = ow;
        }
        // chunk rule: as many images as fit one table buffer, at least one.  A chunk is a range of grids of the same buffers (the key tiles stay
        // the buffers' global 64-key blocks), so the result does not depend on the chunk size.
        const size_t per_image = (size_t)gpi * H * T * S * sizeof(float), fit = t_sam_table_bytes / per_image;
        if (per_image > SAM_TABLE_BYTES) return visrep_set_error(VISREP_ERR_SHAPE, "sam_forward: one image's position tables exceed the table buffer");
        const int chunk = (int)std::min<size_t>((size_t)B, std::max<size_t>(fit, 1));
        for (int b0 = 0; b0 < B; b0 += chunk) {
            const int nb = std::min(chunk, B - b0) * gpi;
            const size_t r0 = (size_t)b0 * gpi * T;                 // first token row of the chunk
            VR_TRY(visrep_relpos_tables(aq + r0 * 2 * d, 2 * d, W.rel_h, W.rel_w, tab_h, tab_w, nb, S, H, 64, stream));
            VR_TRY(visrep_mhsa_relpos_range(aq, 2 * d, av, aldv, tab_h, tab_w, ao, d, B * gpi, b0 * gpi, nb, S, H, 64, scale, s));
        }
        if (!global) VR_TRY(visrep_sam_window_unpartition(ow, d, h, d, B, g, wd, d, stream));
        a.A = h; a.lda = d; a.K = d; a.ldw = d; a.ln_rt = nullptr; a.ln_s = nullptr; a.M = M;
        a.W = (const bf16_t*)W.wo; a.N = d; a.C = x; a.ldc = d; a.bias = W.bo; a.epi = EPI_RESID; a.resid = x; a.ls = nullptr;
        a.stat_rt = rt; a.stat_partial = part; a.stat_eps = c->eps;
        VR_TRY(visrep_gemm_dispatch(a, s));
        GemmArgs f{};
        f.A = x; f.ln_rt = rt; f.ln_s = W.s1; f.lda = d; f.K = d; f.M = M; f.W = (const bf16_t*)W.w1; f.ldw = d; f.N = c->mlp; f.C = mlp; f.ldc = c->mlp;
        f.bias = W.b1; f.epi = EPI_ACT; f.act = VISREP_ACT_GELU_ERF;
        VR_TRY(visrep_gemm_dispatch(f, s));
        f.ln_rt = nullptr; f.ln_s = nullptr; f.A = mlp; f.lda = c->mlp; f.K = c->mlp; f.W = (const bf16_t*)W.w2; f.ldw = c->mlp; f.N = d; f.C = x; f.ldc = d;
        f.bias = W.b2; f.epi = EPI_RESID; f.act = 0; f.resid = x; f.ls = nullptr;
        const bool next = l + 1 < n_layers;
        if (next) { f.stat_rt = rt; f.stat_partial = part; f.stat_eps = c->eps; }
        rt_ready = next;
        VR_TRY(visrep_gemm_dispatch(f, s));
    }
    if (n_state <= c->layers) {
        if (hipMemcpyAsync(hidden, x, (size_t)M * d * 2, hipMemcpyDeviceToDevice, s) != hipSuccess) return visrep_set_error(VISREP_ERR_LAUNCH, "sam_forward: copy of the hidden state failed");
        return 0;
    }
    // ---- neck: conv1x1 (no bias) -> LayerNorm over channels -> conv3x3 pad 1 (no bias) -> LayerNorm over channels
    if (!w->neck_w1 || !w->neck_ln1_g || !w->neck_ln1_b || !w->neck_w2 || !w->neck_ln2_g || !w->neck_ln2_b)
        return visrep_set_error(VISREP_ERR_ARG, "sam_forward: the neck's weights are missing");
    const int oc = c->out_ch;
    bf16_t* n1 = (bf16_t*)(base + L.neck);
    bf16_t* n2 = n1 + up(M, 256) * (size_t)oc;
    visrep_count_route(VISREP_ROUTE_SAM_NECK);
    VR_TRY(visrep_gemm_bf16(x, d, w->neck_w1, d, nullptr, n1, oc, M, oc, d, VISREP_EPI_BIAS, 0, nullptr, nullptr, stream));
    VR_TRY(visrep_layernorm(n1, oc, w->neck_ln1_g, w->neck_ln1_b, n1, oc, M, oc, c->neck_eps, stream));
    VR_TRY(visrep_conv3x3_bf16(n1, B, g, g, oc, w->neck_w2, 9 * oc, nullptr, n2, oc, oc, 1, 0, 0, VISREP_EPI_BIAS, nullptr, stream));
    VR_TRY(visrep_layernorm(n2, oc, w->neck_ln2_g, w->neck_ln2_b, hidden, oc, M, oc, c->neck_eps, stream));
    return 0;
}
