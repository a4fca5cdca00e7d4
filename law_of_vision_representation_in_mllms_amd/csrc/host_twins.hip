// HOST twins of the composed entry points ("CPU twins with identical signatures minus stream (`*_cpu`) back config 1";
// BASELINE configs[0]: CLIP-L/14 tower on CPU fp32, "plumbing, no GPU").
//
// Plain C++ on host threads (std::thread, no OpenMP runtime dependency), fp32 throughout, HOST pointers.  An INDEPENDENT implementation:
// nothing here calls or shares code with oracle/ (test infrastructure) or with the device kernels; it exists so that the reference's
// plug-in surface can be exercised on a box without a GPU - selected ONLY by an explicit device="cpu" on the Python side
// (engine.VitEngineCPU, ascore_ops.max_cos_mean_cpu, cscore_ops.transfer_cpu), never as a fallback: every device entry point still fails
// loudly without a GPU (tests/test_abi_symbols.py).  Not a performance path: a blocked fp32 GEMM at a few GFLOP/s per core.
//
// Reference arithmetic restated (file:line in /root/reference and the installed transformers it delegates to):
//   visrep_vit_forward_cpu        clip_encoder.py:39-51 / dinov2_encoder.py:42-54 / siglip_encoder.py:40-52 -> HF CLIPVisionModel /
//                                 Dinov2Model / SiglipVisionModel(output_hidden_states=True).hidden_states[k] (pre-LN ViT blocks)
//   visrep_ascore_maxcos_cpu      A_score/compute.py:12-15 (normalize_feat) and :54-72 (F.cosine_similarity -> max(dim=1) -> mean)
//   visrep_cscore_transfer_cpu    C_score/pck_train.py:24-29, pck_train_two.py:24-36, utils/utils_correspondence.py:297-337,345-382
//   visrep_cscore_transfer2_cpu   the same on two per-encoder banks (pck_train_two.py:38-51)
//   visrep_pck_count_cpu          C_score/pck_train.py:101,149-163
#include <math.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <thread>
#include <vector>

#include "visrep_internal.h"

namespace {

int clamp_threads(int threads) {
    if (threads <= 0) {
        const unsigned hc = std::thread::hardware_concurrency();
        threads = hc ? (int)std::min(hc, 32u) : 4;                // torch-style oversubscription does not pay on many-core hosts
    }
    return std::max(1, std::min(threads, 256));
}

// dynamic work queue: fn(i) for i in [0, n)
void parallel_for(long n, int threads, const std::function<void(long)>& fn) {
    threads = (int)std::min<long>(clamp_threads(threads), std::max<long>(n, 1));
    if (threads <= 1) {
        for (long i = 0; i < n; ++i) fn(i);
        return;
    }
    std::atomic<long> next(0);
    std::vector<std::thread> pool;
    pool.reserve(threads);
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([&]() {
            for (;;) {
                const long i = next.fetch_add(1);
                if (i >= n) return;
                fn(i);
            }
        });
    for (auto& th : pool) th.join();
}

// C[M, N] (ldc) = A[M, K] (lda) * W[N, K]^T (ldw) + bias[N]: nn.Linear.  Rows of A are independent work items (blocks of 8 rows); the
// inner loop is a dot product over contiguous K that the compiler vectorises.  fp32 accumulation in eight partial sums (pairwise-ish).
void linear_rows(const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc, long M, int N, int K, int threads) {
    const long blocks = (M + 7) / 8;
    parallel_for(blocks, threads, [&](long b) {
        const long m0 = b * 8, m1 = std::min<long>(M, m0 + 8);
        for (int n = 0; n < N; ++n) {
            const float* w = W + (size_t)n * ldw;
            for (long m = m0; m < m1; ++m) {
                const float* a = A + (size_t)m * lda;
                float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                int k = 0;
                for (; k + 8 <= K; k += 8)
                    for (int u = 0; u < 8; ++u) s[u] += a[k + u] * w[k + u];
                float t = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
                for (; k < K; ++k) t += a[k] * w[k];
                C[(size_t)m * ldc + n] = t + (bias ? bias[n] : 0.f);
            }
        }
    });
}

void layernorm_rows_cpu(const float* x, const float* g, const float* b, float* y, long rows, int d, float eps, int threads) {
    parallel_for((rows + 63) / 64, threads, [&](long blk) {
        for (long r = blk * 64; r < std::min<long>(rows, blk * 64 + 64); ++r) {
            const float* xr = x + (size_t)r * d;
            float* yr = y + (size_t)r * d;
            double mean = 0.0;
            for (int i = 0; i < d; ++i) mean += xr[i];
            mean /= d;
            double var = 0.0;
            for (int i = 0; i < d; ++i) { const double t = xr[i] - mean; var += t * t; }
            var /= d;                                              // biased, like torch.nn.LayerNorm
            const float rstd = (float)(1.0 / sqrt(var + (double)eps)), mu = (float)mean;
            for (int i = 0; i < d; ++i) yr[i] = (xr[i] - mu) * rstd * g[i] + b[i];
        }
    });
}

// RMSNorm of `halves` consecutive blocks of d floats per row (HF InternVLVisionRMSNorm): y = x * rsqrt(sum(x^2) / d_true + eps) * g, the sum in
// double and in column order (zero-padded columns add exactly nothing).  halves = 1: the block norm; 2: Q | K with gains g / g2.  y may alias x.
void rmsnorm_rows_cpu(const float* x, int ldx, const float* g, const float* g2, float* y, int ldy, long rows, int d, int halves, int d_true, float eps,
                      int threads) {
    parallel_for((rows + 63) / 64, threads, [&](long blk) {
        for (long r = blk * 64; r < std::min<long>(rows, blk * 64 + 64); ++r)
            for (int hf = 0; hf < halves; ++hf) {
                const float* xr = x + (size_t)r * ldx + (size_t)hf * d;
                float* yr = y + (size_t)r * ldy + (size_t)hf * d;
                const float* gg = hf ? g2 : g;
                double ss = 0.0;
                for (int i = 0; i < d; ++i) ss += (double)xr[i] * xr[i];
                const float rstd = (float)(1.0 / sqrt(ss / d_true + (double)eps));
                for (int i = 0; i < d; ++i) yr[i] = xr[i] * rstd * gg[i];
            }
    });
}

float act_cpu(float x, int act) {
    switch (act) {
        case VISREP_ACT_QUICK_GELU: return x * (1.0f / (1.0f + expf(-1.702f * x)));                     // HF QuickGELUActivation
        case VISREP_ACT_GELU_ERF: return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f));             // nn.GELU()
        case VISREP_ACT_GELU_TANH: return 0.5f * x * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
        default: return x;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ RMSNorm twins
extern "C" int visrep_rmsnorm_cpu(const float* x, int ldx, const float* gamma, float* y, int ldy, long rows, int d, float eps, int threads) {
    if (!x || !gamma || !y) return visrep_set_error(VISREP_ERR_ARG, "rmsnorm_cpu: null pointer");
    if (d <= 0 || ldx < d || ldy < d) return visrep_set_error(VISREP_ERR_SHAPE, "rmsnorm_cpu: ldx, ldy >= d > 0 required");
    if (rows > 0) rmsnorm_rows_cpu(x, ldx, gamma, gamma, y, ldy, rows, d, 1, d, eps, threads);
    return 0;
}

extern "C" int visrep_rmsnorm_stats_cpu(const float* x, int ldx, float* rt, long rows, int d, float eps, int threads) {
    if (!x || !rt) return visrep_set_error(VISREP_ERR_ARG, "rmsnorm_stats_cpu: null pointer");
    if (d <= 0 || ldx < d) return visrep_set_error(VISREP_ERR_SHAPE, "rmsnorm_stats_cpu: ldx >= d > 0 required");
    parallel_for((rows + 63) / 64, threads, [&](long blk) {
        for (long r = blk * 64; r < std::min<long>(rows, blk * 64 + 64); ++r) {
            double ss = 0.0;
            for (int i = 0; i < d; ++i) ss += (double)x[(size_t)r * ldx + i] * x[(size_t)r * ldx + i];
            rt[2 * r] = (float)(1.0 / sqrt(ss / d + (double)eps));
            rt[2 * r + 1] = 0.f;
        }
    });
    return 0;
}

extern "C" int visrep_qk_rmsnorm_cpu(float* qk, int ldqk, int width, int d_true, const float* qn_g, const float* kn_g, long rows, float eps, int threads) {
    if (!qk || !qn_g || !kn_g) return visrep_set_error(VISREP_ERR_ARG, "qk_rmsnorm_cpu: null pointer");
    if (width <= 0 || ldqk < 2 * width || d_true <= 0 || d_true > width)
        return visrep_set_error(VISREP_ERR_SHAPE, "qk_rmsnorm_cpu: ldqk >= 2 * width, 0 < d_true <= width required");
    if (rows > 0) rmsnorm_rows_cpu(qk, ldqk, qn_g, kn_g, qk, ldqk, rows, width, 2, d_true, eps, threads);
    return 0;
}

// ------------------------------------------------------------------------------------------------ ViT tower
extern "C" int visrep_vit_forward_cpu(const visrep_vit_config* c, const visrep_vit_weights* w, const float* pixels, float* hidden, int B, int n_layers,
                                      int threads) {
    if (!c || !w || !pixels || !hidden) return visrep_set_error(VISREP_ERR_ARG, "vit_forward_cpu: null pointer");
    if (B <= 0) return 0;
    if (n_layers < 0 || n_layers > c->layers) return visrep_set_error(VISREP_ERR_ARG, "vit_forward_cpu: n_layers out of range");
    if (c->heads <= 0 || c->d % c->heads) return visrep_set_error(VISREP_ERR_SHAPE, "vit_forward_cpu: d must be a multiple of heads");
    const int grid = c->image_size / c->patch, P = grid * grid, T = c->tokens, d = c->d, p = c->patch, S = c->image_size;
    // S / patch floors like Conv2d(k = s = patch): trailing pixels fill no patch (384 / 14 = 27)
    if (c->registers < 0 || (c->registers > 0 && !c->has_cls)) return visrep_set_error(VISREP_ERR_SHAPE, "vit_forward_cpu: register tokens need a CLS token");
    if (grid <= 0 || P + (c->has_cls ? 1 : 0) + c->registers != T) return visrep_set_error(VISREP_ERR_SHAPE, "vit_forward_cpu: tokens != grid^2 + cls + registers");
    const int kp = 3 * p * p, kpad = c->kpad > 0 ? c->kpad : kp;       // patch_w rows are kpad floats wide (zero padded past 3 p p)
    if (kpad < kp) return visrep_set_error(VISREP_ERR_SHAPE, "vit_forward_cpu: kpad < 3 * patch^2");
    if (c->norm != 0 && c->norm != 1) return visrep_set_error(VISREP_ERR_ARG, "vit_forward_cpu: norm must be 0 (LayerNorm) or 1 (RMSNorm)");
    const bool rms = c->norm == 1;
    if (rms && c->pre_ln) return visrep_set_error(VISREP_ERR_ARG, "vit_forward_cpu: pre_ln with RMSNorm blocks is not supported");
    if (c->qk_norm)
        for (int l = 0; l < n_layers; ++l)
            if (!w->layers[l].qn_g || !w->layers[l].kn_g) return visrep_set_error(VISREP_ERR_ARG, "vit_forward_cpu: a qk_norm tower needs qn_g and kn_g in every layer");
    const long M = (long)B * T;
    const int dh = d / c->heads, mlp = c->mlp;
    const float* pw = (const float*)w->patch_w;
    // ---- embeddings: Conv2d(3, d, k = s = patch) as im2col (column order (channel, ky, kx) = the conv weight's own flattening) + Linear
    std::vector<float> cols((size_t)B * P * kp);
    parallel_for((long)B * P, threads, [&](long i) {
        const int b = (int)(i / P), pi = (int)(i % P), gy = pi / grid, gx = pi % grid;
        float* o = cols.data() + (size_t)i * kp;
        for (int ch = 0; ch < 3; ++ch)
            for (int ky = 0; ky < p; ++ky)
                memcpy(o + (ch * p + ky) * p, pixels + (((size_t)b * 3 + ch) * S + gy * p + ky) * S + gx * p, sizeof(float) * p);
    });
    std::vector<float> emb((size_t)B * P * d);
    linear_rows(cols.data(), kp, pw, kpad, w->patch_b, emb.data(), d, (long)B * P, d, kp, threads);
    const int off = (c->has_cls ? 1 : 0) + c->registers;      // prefix rows: the class token, then the registers (cls = [off, d], their pos rows zero)
    parallel_for(M, threads, [&](long r) {
        const int b = (int)(r / T), t = (int)(r % T);
        float* x = hidden + (size_t)r * d;
        const float* pos = w->pos + (size_t)t * d;
        if (t < off) {
            const float* pre = w->cls + (size_t)t * d;
            for (int i = 0; i < d; ++i) x[i] = pre[i] + pos[i];
        } else {
            const float* e = emb.data() + ((size_t)b * P + (t - off)) * d;
            for (int i = 0; i < d; ++i) x[i] = e[i] + pos[i];
        }
    });
    std::vector<float>().swap(cols);
    std::vector<float>().swap(emb);
    if (c->pre_ln) layernorm_rows_cpu(hidden, w->pre_ln_g, w->pre_ln_b, hidden, M, d, c->eps, threads);
    const bool swiglu = c->act == VISREP_ACT_SWIGLU;          // HF Dinov2SwiGLUFFN: w1 [2 mlp, d] = gate rows, then value rows
    const int mw = swiglu ? 2 * mlp : mlp;                    // width of fc1's output
    std::vector<float> h((size_t)M * d), qkv((size_t)M * 3 * d), att((size_t)M * d), mid((size_t)M * mw), tmp((size_t)M * d);
    const float scale = 1.0f / sqrtf((float)dh);
    for (int l = 0; l < n_layers; ++l) {
        const visrep_vit_layer& L = w->layers[l];
        if (rms) rmsnorm_rows_cpu(hidden, d, L.ln1_g, L.ln1_g, h.data(), d, M, d, 1, d, c->eps, threads);
        else layernorm_rows_cpu(hidden, L.ln1_g, L.ln1_b, h.data(), M, d, c->eps, threads);
        linear_rows(h.data(), d, (const float*)L.wqkv, d, L.bqkv, qkv.data(), 3 * d, M, 3 * d, d, threads);
        if (c->qk_norm) rmsnorm_rows_cpu(qkv.data(), 3 * d, L.qn_g, L.kn_g, qkv.data(), 3 * d, M, d, 2, d, VISREP_QK_NORM_EPS, threads);
        // softmax(q k^T / sqrt(dh)) v per (image, head, query row), fp32 with a max-subtracted exponent like torch.softmax
        parallel_for((long)B * c->heads, threads, [&](long bh) {
            const int b = (int)(bh / c->heads), hd = (int)(bh % c->heads);
            std::vector<float> sc(T);
            for (int tq = 0; tq < T; ++tq) {
                const float* q = qkv.data() + ((size_t)b * T + tq) * 3 * d + hd * dh;
                float mx = -INFINITY;
                for (int tk = 0; tk < T; ++tk) {
                    const float* k = qkv.data() + ((size_t)b * T + tk) * 3 * d + d + hd * dh;
                    float s = 0.f;
                    for (int i = 0; i < dh; ++i) s += q[i] * k[i];
                    sc[tk] = s * scale;
                    mx = std::max(mx, sc[tk]);
                }
                float den = 0.f;
                for (int tk = 0; tk < T; ++tk) { sc[tk] = expf(sc[tk] - mx); den += sc[tk]; }
                float* o = att.data() + ((size_t)b * T + tq) * d + hd * dh;
                for (int i = 0; i < dh; ++i) o[i] = 0.f;
                for (int tk = 0; tk < T; ++tk) {
                    const float pr = sc[tk] / den;
                    const float* v = qkv.data() + ((size_t)b * T + tk) * 3 * d + 2 * d + hd * dh;
                    for (int i = 0; i < dh; ++i) o[i] += pr * v[i];
                }
            }
        });
        linear_rows(att.data(), d, (const float*)L.wo, d, L.bo, tmp.data(), d, M, d, d, threads);
        parallel_for((M + 63) / 64, threads, [&](long blk) {
            for (long r = blk * 64; r < std::min<long>(M, blk * 64 + 64); ++r)
                for (int i = 0; i < d; ++i) hidden[(size_t)r * d + i] += (L.ls1 ? L.ls1[i] : 1.f) * tmp[(size_t)r * d + i];
        });
        if (rms) rmsnorm_rows_cpu(hidden, d, L.ln2_g, L.ln2_g, h.data(), d, M, d, 1, d, c->eps, threads);
        else layernorm_rows_cpu(hidden, L.ln2_g, L.ln2_b, h.data(), M, d, c->eps, threads);
        linear_rows(h.data(), d, (const float*)L.w1, d, L.b1, mid.data(), mw, M, mw, d, threads);
        const int act = c->act;
        if (swiglu) {                                         // x1, x2 = chunk(2); silu(x1) * x2, left in the first mlp columns of each row
            parallel_for(M, threads, [&](long r) {
                float* row = mid.data() + (size_t)r * mw;
                for (int i = 0; i < mlp; ++i) row[i] = row[i] / (1.0f + expf(-row[i])) * row[mlp + i];
            });
        } else {
            parallel_for((M + 15) / 16, threads, [&](long blk) {
                for (size_t i = (size_t)blk * 16 * mlp; i < (size_t)std::min<long>(M, blk * 16 + 16) * mlp; ++i) mid[i] = act_cpu(mid[i], act);
            });
        }
        linear_rows(mid.data(), mw, (const float*)L.w2, mlp, L.b2, tmp.data(), d, M, d, mlp, threads);
        parallel_for((M + 63) / 64, threads, [&](long blk) {
            for (long r = blk * 64; r < std::min<long>(M, blk * 64 + 64); ++r)
                for (int i = 0; i < d; ++i) hidden[(size_t)r * d + i] += (L.ls2 ? L.ls2[i] : 1.f) * tmp[(size_t)r * d + i];
        });
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ A score
extern "C" int visrep_ascore_maxcos_cpu(const float* other, const float* ref, int n_img, int Nt, int Nr, int D, float* scores, int threads) {
    if (n_img <= 0) return 0;
    if (!other || !ref || !scores) return visrep_set_error(VISREP_ERR_ARG, "ascore_cpu: null pointer");
    if (Nt <= 0 || Nr <= 0 || D <= 0) return visrep_set_error(VISREP_ERR_SHAPE, "ascore_cpu: empty tensor");
    // both normalisations of a row (compute.py:12-15: x / (|x| + 1e-10); cosine_similarity: / max(|x'|, 1e-8)) as one factor
    auto row_factor = [D](const float* x) {
        double ss = 0.0;
        for (int i = 0; i < D; ++i) ss += (double)x[i] * x[i];
        const float n = (float)sqrt(ss), f1 = 1.0f / (n + 1e-10f);
        return f1 / std::max(n * f1, 1e-8f);
    };
    std::vector<float> row_max((size_t)n_img * Nt);
    parallel_for((long)n_img * ((Nt + 15) / 16), threads, [&](long item) {
        const int tb = (Nt + 15) / 16, img = (int)(item / tb), t0 = (int)(item % tb) * 16, t1 = std::min(Nt, t0 + 16);
        const float* R = ref + (size_t)img * Nr * D;
        std::vector<float> rf(Nr);
        for (int s = 0; s < Nr; ++s) rf[s] = row_factor(R + (size_t)s * D);
        for (int t = t0; t < t1; ++t) {
            const float* o = other + ((size_t)img * Nt + t) * D;
            const float of = row_factor(o);
            float best = -INFINITY;
            for (int s = 0; s < Nr; ++s) {
                const float* r = R + (size_t)s * D;
                float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                int k = 0;
                for (; k + 8 <= D; k += 8)
                    for (int u = 0; u < 8; ++u) acc[u] += o[k + u] * r[k + u];
                float dot = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
                for (; k < D; ++k) dot += o[k] * r[k];
                best = std::max(best, dot * of * rf[s]);
            }
            row_max[(size_t)img * Nt + t] = best;
        }
    });
    for (int img = 0; img < n_img; ++img) {
        double s = 0.0;
        for (int t = 0; t < Nt; ++t) s += row_max[(size_t)img * Nt + t];
        scores[img] = (float)(s / Nt);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ C score
// One body for both entry points.  feats_b == nullptr: one bank of C = C_a channels per position, normalised in the blocks [0, split) /
// [split, C) when split > 0.  feats_b != nullptr (position-major only): channels [0, C_a) come from bank A, [C_a, C_a + C_b) from bank B, both
// indexed by the same image slots, and split = C_a - the descriptor is gathered into one C-vector first, so everything after the gather is
// the same code on the same values as the one-bank call on the concatenation.
static int cscore_transfer_host(const float* feats, int C_a, const float* feats_b, int C_b, const int* img1, const int* img2, const int* patch_idx,
                                const int* nkp, const float* lin, float* xy, int n_pairs, int kmax, int P, int split, int window, int soft_eval,
                                float beta, float anno_stride, float anno_half, int layout, int threads) {
    const int C = C_a + C_b;
    const int PP = P * P;
    const size_t map = (size_t)PP * C_a, map_b = (size_t)PP * C_b;
    // descriptor of patch p of image im as a normalised C-vector (pck_train.py:24-29; two encoders: pck_train_two.py:24-36)
    auto descriptor = [&](int im, int pidx, float* out) {
        const float* base = feats + (size_t)im * map;
        for (int ch = 0; ch < C_a; ++ch) out[ch] = layout ? base[(size_t)pidx * C_a + ch] : base[(size_t)ch * PP + pidx];
        if (feats_b) {
            const float* bb = feats_b + (size_t)im * map_b + (size_t)pidx * C_b;
            for (int ch = 0; ch < C_b; ++ch) out[C_a + ch] = bb[ch];
        }
        auto norm = [&](int c0, int c1) {
            double ss = 0.0;
            for (int ch = c0; ch < c1; ++ch) ss += (double)out[ch] * out[ch];
            const float f = 1.0f / ((float)sqrt(ss) + 1e-10f);
            for (int ch = c0; ch < c1; ++ch) out[ch] *= f;
        };
        if (split > 0) { norm(0, split); norm(split, C); }
        norm(0, C);
    };
    parallel_for(n_pairs, threads, [&](long z) {
        const int K = nkp[z];
        std::vector<float> tgt((size_t)PP * C), src(C), sim(PP), prob(PP);
        for (int q = 0; q < PP; ++q) descriptor(img2[z], q, tgt.data() + (size_t)q * C);
        for (int k = 0; k < kmax; ++k) {
            float* o = xy + ((size_t)z * kmax + k) * 2;
            if (k >= K) { o[0] = o[1] = 0.f; continue; }
            const int pidx = patch_idx[(size_t)z * kmax + k];
            if (pidx < 0 || pidx >= PP) { o[0] = o[1] = 0.f; continue; }
            descriptor(img1[z], pidx, src.data());
            int am = 0;
            for (int q = 0; q < PP; ++q) {
                const float* t = tgt.data() + (size_t)q * C;
                float s = 0.f;
                for (int ch = 0; ch < C; ++ch) s += src[ch] * t[ch];
                sim[q] = s;
                if (s > sim[am]) am = q;
            }
            float px, py;
            if (!soft_eval) {
                px = (float)(am % P); py = (float)(am / P);
            } else {
                // get_flow (utils_correspondence.py:297-337): entries outside the clamped window become ZERO (not -inf) and stay in the softmax
                if (window > 0) {
                    const int mx = am % P, my = am / P;
                    const int x0 = std::max(0, mx - window), x1 = std::min(P - 1, mx + window), y0 = std::max(0, my - window), y1 = std::min(P - 1, my + window);
                    for (int q = 0; q < PP; ++q) {
                        const int qx = q % P, qy = q / P;
                        if (qx < x0 || qx > x1 || qy < y0 || qy > y1) sim[q] = 0.f;
                    }
                } else if (window < 0) {
                    // "kernel soft-argmax" (apply_gaussian_kernel, utils_correspondence.py:278-295): a Gaussian of sigma = -window patches around the
                    // argmax target weights every similarity before the softmax (the reference hard-wires a 60 x 60 grid; any P here)
                    const float mx = (float)(am % P), my = (float)(am / P), two_s2 = 2.f * (float)(window * window);
                    for (int q = 0; q < PP; ++q) {
                        const float dx = (float)(q % P) - mx, dy = (float)(q / P) - my;
                        sim[q] *= expf(-(dx * dx + dy * dy) / two_s2);
                    }
                }
                float mxv = sim[0];
                for (int q = 1; q < PP; ++q) mxv = std::max(mxv, sim[q]);
                double den = 0.0;
                for (int q = 0; q < PP; ++q) { prob[q] = expf((sim[q] - mxv) / beta); den += prob[q]; }
                double gx = 0.0, gy = 0.0;
                for (int q = 0; q < PP; ++q) {
                    const double pr = prob[q] / den;
                    gx += pr * lin[q % P];
                    gy += pr * lin[q / P];
                }
                px = (float)((gx + 1.0) * (P - 1) / 2.0);
                py = (float)((gy + 1.0) * (P - 1) / 2.0);
                px = std::min(std::max(px, 0.f), (float)(P - 1));
                py = std::min(std::max(py, 0.f), (float)(P - 1));
            }
            o[0] = px * anno_stride + anno_half;
            o[1] = py * anno_stride + anno_half;
        }
    });
    return 0;
}

extern "C" int visrep_cscore_transfer_cpu(const float* feats, const int* img1, const int* img2, const int* patch_idx, const int* nkp, const float* lin,
                                          float* xy, int n_pairs, int kmax, int P, int C, int split, int window, int soft_eval, float beta,
                                          float anno_stride, float anno_half, int layout, int threads) {
    if (n_pairs <= 0) return 0;
    if (!feats || !img1 || !img2 || !patch_idx || !nkp || !lin || !xy) return visrep_set_error(VISREP_ERR_ARG, "cscore_transfer_cpu: null pointer");
    if (P <= 0 || C <= 0 || kmax <= 0 || split < 0 || split >= C) return visrep_set_error(VISREP_ERR_SHAPE, "cscore_transfer_cpu: bad shape");
    return cscore_transfer_host(feats, C, nullptr, 0, img1, img2, patch_idx, nkp, lin, xy, n_pairs, kmax, P, split, window, soft_eval, beta, anno_stride,
                                anno_half, layout, threads);
}

// Two per-encoder banks, position-major [n_images, P*P, C_a] / [n_images, P*P, C_b] (pck_train_two.py:38-51 loads two maps per image)
extern "C" int visrep_cscore_transfer2_cpu(const float* feats_a, int C_a, const float* feats_b, int C_b, const int* img1, const int* img2,
                                           const int* patch_idx, const int* nkp, const float* lin, float* xy, int n_pairs, int kmax, int P, int window,
                                           int soft_eval, float beta, float anno_stride, float anno_half, int threads) {
    if (n_pairs <= 0) return 0;
    if (!feats_a || !feats_b || !img1 || !img2 || !patch_idx || !nkp || !lin || !xy)
        return visrep_set_error(VISREP_ERR_ARG, "cscore_transfer2_cpu: null pointer");
    if (P <= 0 || C_a <= 0 || C_b <= 0 || kmax <= 0) return visrep_set_error(VISREP_ERR_SHAPE, "cscore_transfer2_cpu: bad shape");
    return cscore_transfer_host(feats_a, C_a, feats_b, C_b, img1, img2, patch_idx, nkp, lin, xy, n_pairs, kmax, P, C_a, window, soft_eval, beta,
                                anno_stride, anno_half, 1, threads);
}

extern "C" int visrep_pck_count_cpu(const float* xy, const float* kps1, const float* kps2, const double* thresholds, const int* nkp, int n_pairs,
                                    int kmax, const float* alphas3, int* counts) {
    if (n_pairs <= 0) return 0;
    if (!xy || !kps1 || !kps2 || !thresholds || !nkp || !alphas3 || !counts) return visrep_set_error(VISREP_ERR_ARG, "pck_count_cpu: null pointer");
    for (int z = 0; z < n_pairs; ++z) {
        int hit[3] = {0, 0, 0}, vis = 0;
        for (int k = 0; k < nkp[z] && k < kmax; ++k) {
            const float* a = kps1 + ((size_t)z * kmax + k) * 3;
            const float* b = kps2 + ((size_t)z * kmax + k) * 3;
            if (!(a[2] * b[2] > 0.f)) continue;                   // vis = img1_kps[:, 2] * img2_kps[:, 2] > 0 (pck_train.py:101)
            ++vis;
            const float dx = b[0] - xy[((size_t)z * kmax + k) * 2], dy = b[1] - xy[((size_t)z * kmax + k) * 2 + 1];
            const float err = sqrtf(dy * dy + dx * dx);           // fp32 norm of the (y, x) difference (pck_train.py:149-152)
            for (int j = 0; j < 3; ++j)
                if ((double)err < (double)alphas3[j] * thresholds[z]) ++hit[j];       // float32 alpha x float64 bbox threshold (:157-160)
        }
        counts[z * 4 + 0] = hit[0]; counts[z * 4 + 1] = hit[1]; counts[z * 4 + 2] = hit[2]; counts[z * 4 + 3] = vis;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ ConvNeXt twins
// HF ConvNextLayer.forward (dwconv -> channels-last LayerNorm) and ConvNextStage.downsampling_layer (LayerNorm -> 2x2 stride-2 convolution),
// restated on the device kernels' contract: bf16 storage in and out (HOST pointers), fp32 fmaf chains in the device order.
namespace {
inline float bf16_to_f32(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }
inline uint16_t f32_to_bf16(float f) {                              // round to nearest even; NaN stays NaN
    uint32_t u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
}  // namespace

extern "C" int visrep_dwconv7x7_stats_cpu(const void* x_, int ldx, const float* wt, const float* bias, void* y_, int ldy, float* rt, int B, int H, int W,
                                          int C, float eps, int threads) {
    if (!x_ || !wt || !bias || !y_ || !rt) return visrep_set_error(VISREP_ERR_ARG, "dwconv7x7_cpu: null pointer");
    if (x_ == y_) return visrep_set_error(VISREP_ERR_ARG, "dwconv7x7_cpu: y must not alias x");
    if (C <= 0 || C % 64) return visrep_set_error(VISREP_ERR_SHAPE, "dwconv7x7_cpu: C must be a positive multiple of 64");
    if (B < 0 || H < 1 || W < 1) return visrep_set_error(VISREP_ERR_SHAPE, "dwconv7x7_cpu: need B >= 0, H >= 1, W >= 1");
    if (ldx % 8 || ldy % 8 || ldx < C || ldy < C) return visrep_set_error(VISREP_ERR_SHAPE, "dwconv7x7_cpu: ldx / ldy must be multiples of 8 and >= C");
    const uint16_t* x = (const uint16_t*)x_;
    uint16_t* y = (uint16_t*)y_;
    parallel_for((long)B * H, threads, [&](long item) {
        const long b = item / H;
        const int oy = (int)(item - b * H);
        for (int ox = 0; ox < W; ++ox) {
            const size_t r = ((size_t)b * H + oy) * W + ox;
            double s1 = 0.0, s2 = 0.0;
            for (int c = 0; c < C; ++c) {
                float acc = bias[c];
                for (int ky = 0; ky < 7; ++ky) {
                    const int iy = oy + ky - 3;
                    if (iy < 0 || iy >= H) continue;                  // a zero-padded tap adds fmaf(0, w, acc) = acc
                    for (int kx = 0; kx < 7; ++kx) {
                        const int ix = ox + kx - 3;
                        if (ix < 0 || ix >= W) continue;
                        acc = fmaf(bf16_to_f32(x[(((size_t)b * H + iy) * W + ix) * ldx + c]), wt[(size_t)(ky * 7 + kx) * C + c], acc);
                    }
                }
                const uint16_t h = f32_to_bf16(acc);
                y[r * ldy + c] = h;
                const double v = bf16_to_f32(h);                       // statistics of the ROUNDED outputs: what the GEMM reads
                s1 += v; s2 += v * v;
            }
            const double mean = s1 / C, var = std::max(s2 / C - mean * mean, 0.0);
            const double rstd = 1.0 / sqrt(var + (double)eps);
            rt[2 * r] = (float)rstd;
            rt[2 * r + 1] = (float)(-mean * rstd);
        }
    });
    return 0;
}

extern "C" int visrep_ln_space_to_depth2_cpu(const void* x_, int ldx, const float* gamma, const float* beta, void* out_, int ldo, int B, int H, int W,
                                             int C, float eps, int threads) {
    if (!x_ || !gamma || !beta || !out_) return visrep_set_error(VISREP_ERR_ARG, "ln_space_to_depth2_cpu: null pointer");
    if (x_ == out_) return visrep_set_error(VISREP_ERR_ARG, "ln_space_to_depth2_cpu: out must not alias x");
    if (C <= 0 || C % 8 || C > 4096) return visrep_set_error(VISREP_ERR_SHAPE, "ln_space_to_depth2_cpu: C must be a multiple of 8, at most 4096");
    if (B < 0 || H < 2 || W < 2 || (H & 1) || (W & 1)) return visrep_set_error(VISREP_ERR_SHAPE, "ln_space_to_depth2_cpu: H and W must be even and >= 2");
    if (ldx % 8 || ldo % 8 || ldx < C || (long)ldo < 4L * C) return visrep_set_error(VISREP_ERR_SHAPE, "ln_space_to_depth2_cpu: ldx % 8, ldo % 8, ldx >= C and ldo >= 4 C required");
    const uint16_t* x = (const uint16_t*)x_;
    uint16_t* out = (uint16_t*)out_;
    parallel_for((long)B * H, threads, [&](long item) {
        const long b = item / H;
        const int py = (int)(item - b * H);
        for (int px = 0; px < W; ++px) {
            const uint16_t* xr = x + (((size_t)b * H + py) * W + px) * ldx;
            double mean = 0.0;
            for (int c = 0; c < C; ++c) mean += bf16_to_f32(xr[c]);
            mean /= C;
            double var = 0.0;
            for (int c = 0; c < C; ++c) { const double t = bf16_to_f32(xr[c]) - mean; var += t * t; }
            const float rstd = (float)(1.0 / sqrt(var / C + (double)eps)), mu = (float)mean;
            uint16_t* o = out + (((size_t)b * (H / 2) + py / 2) * (W / 2) + px / 2) * ldo + (size_t)((py & 1) * 2 + (px & 1)) * C;
            for (int c = 0; c < C; ++c) o[c] = f32_to_bf16((bf16_to_f32(xr[c]) - mu) * rstd * gamma[c] + beta[c]);
        }
    });
    return 0;
}

// ------------------------------------------------------------------------------------------------ SAM twins
// SamVisionAttention's decomposed relative-position term and the attention that consumes it (visrep_relpos_tables / visrep_mhsa_relpos_fwd),
// restated in plain C++: the tables as the device's single fmaf chain over c = 0 .. 63 (bit-equal), the attention in fp32 logits with
// float64 sums and no bf16 rounding (a statement of the contract, not of the kernel's roundings).
extern "C" int visrep_relpos_tables_cpu(const void* qk_, int ldqk, const float* Rh, const float* Rw, float* rel_h, float* rel_w, int NB, int S, int H,
                                        int head_dim, int threads) {
    if (head_dim != 64) return visrep_set_error(VISREP_ERR_SHAPE, "relpos_tables_cpu: only head_dim 64 is implemented");
    if (S < 2 || S > 64) return visrep_set_error(VISREP_ERR_SHAPE, "relpos_tables_cpu: the grid side S must be 2 .. 64");
    if (!qk_ || !Rh || !Rw || !rel_h || !rel_w) return visrep_set_error(VISREP_ERR_ARG, "relpos_tables_cpu: null pointer");
    if (NB <= 0 || H <= 0) return visrep_set_error(VISREP_ERR_SHAPE, "relpos_tables_cpu: empty problem");
    if ((ldqk % 8) || ldqk < H * 64) return visrep_set_error(VISREP_ERR_SHAPE, "relpos_tables_cpu: ldqk % 8 == 0 and >= H 64");
    const uint16_t* qk = (const uint16_t*)qk_;
    const int T = S * S;
    parallel_for((long)NB * H * T, threads, [&](long row) {
        const int qi = (int)(row % T), h = (int)((row / T) % H);
        const long g = row / T / H;
        const int qh = qi / S, qw = qi % S;
        const uint16_t* qp = qk + ((size_t)g * T + qi) * ldqk + h * 64;
        for (int j = 0; j < 2 * S; ++j) {
            const bool isw = j >= S;
            const int kx = isw ? j - S : j;
            const float* R = (isw ? Rw : Rh) + (size_t)((isw ? qw : qh) - kx + S - 1) * 64;
            float acc = 0.f;
            for (int c = 0; c < 64; ++c) acc = fmaf(bf16_to_f32(qp[c]), R[c], acc);
            (isw ? rel_w : rel_h)[row * S + kx] = acc;
        }
    });
    return 0;
}

extern "C" int visrep_mhsa_relpos_cpu(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* rel_h, const float* rel_w,
                                      float* out, int ldo, int NB, int S, int H, int head_dim, float scale, int threads) {
    if (head_dim != 64) return visrep_set_error(VISREP_ERR_SHAPE, "mhsa_relpos_cpu: only head_dim 64 is implemented");
    if (S < 2 || S > 64) return visrep_set_error(VISREP_ERR_SHAPE, "mhsa_relpos_cpu: the grid side S must be 2 .. 64");
    if (!q || !k || !v || !rel_h || !rel_w || !out) return visrep_set_error(VISREP_ERR_ARG, "mhsa_relpos_cpu: null pointer");
    if (NB <= 0 || H <= 0) return visrep_set_error(VISREP_ERR_SHAPE, "mhsa_relpos_cpu: empty problem");
    if (!(scale > 0.f)) return visrep_set_error(VISREP_ERR_ARG, "mhsa_relpos_cpu: scale must be > 0");
    if (ldq < H * 64 || ldk < H * 64 || ldv < H * 64 || ldo < H * 64) return visrep_set_error(VISREP_ERR_SHAPE, "mhsa_relpos_cpu: leading dimensions must cover H 64");
    const int T = S * S;
    parallel_for((long)NB * H * T, threads, [&](long row) {
        const int qi = (int)(row % T), h = (int)((row / T) % H);
        const long g = row / T / H;
        const float* qp = q + ((size_t)g * T + qi) * ldq + h * 64;
        const float *bh = rel_h + row * S, *bw = rel_w + row * S;
        std::vector<float> t(T);
        float m = -INFINITY;
        for (int kk = 0; kk < T; ++kk) {
            const float* kp = k + ((size_t)g * T + kk) * ldk + h * 64;
            float dot = 0.f;
            for (int c = 0; c < 64; ++c) dot = fmaf(qp[c], kp[c], dot);
            t[kk] = fmaf(dot, scale, bh[kk / S] + bw[kk % S]);
            m = std::max(m, t[kk]);
        }
        double l = 0.0, o[64] = {};
        for (int kk = 0; kk < T; ++kk) {
            const double p = exp((double)t[kk] - (double)m);
            const float* vp = v + ((size_t)g * T + kk) * ldv + h * 64;
            l += p;
            for (int c = 0; c < 64; ++c) o[c] += p * vp[c];
        }
        float* op = out + ((size_t)g * T + qi) * ldo + h * 64;
        for (int c = 0; c < 64; ++c) op[c] = (float)(o[c] / l);
    });
    return 0;
}
