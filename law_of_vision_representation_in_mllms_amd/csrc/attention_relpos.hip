// Self-attention over NB independent S x S token grids whose logits carry a decomposed relative-position term (ViTDet / the Segment
// Anything image encoder, transformers modeling_sam.py SamVisionAttention):
//
//   O[g, q, h, :] = softmax_k( scale * Q[g,q,h,:] . K[g,k,h,:] + rel_h[g,h,q, k / S] + rel_w[g,h,q, k % S] ) V[g,k,h,:]
//
// attn_fwd_relpos is a COPY of attn_fwd<1> (attention.hip: layouts, global 64-key tiles, swapped S^T = K Q^T, LDS ring, masks) - a copy and
// not a shared template body, so that the existing instantiations keep their code.  What it adds:
//   * the two fp32 tables of the block's 128 queries are staged once into LDS behind the K / V^T ring, row q at float offset q (2 S + 1)
//     (odd stride: the 32 lanes of a half-wave read one column of 32 different rows without a bank conflict): rel_h in [0, S), rel_w in
//     [S, 2 S).  Rows of queries past T are zero.
//   * after the Q.K^T MFMAs every score becomes the exponent of 2 it stands for:  t = fma(s, scale log2 e, (rel_h + rel_w) log2 e)
//     - one fp32 add, one multiply, one fma - with kh = kl / S by multiply-shift (kl < 4096, S <= 64: exact), kl = the key's index inside
//     its grid, clamped into it (keys outside the grid are masked afterwards, as before).
//   * the running maximum works on t (deferred by up to 2^8, as attn_fwd): p = exp2(t - m).
// relpos_tables_rows builds the tables from the Q half of a qk buffer; sam_window_* are the gather / scatter between the token rows of a
// [B, g, g] map and its zero-padded w x w windows.
#include <cstdlib>

#include "common.h"
#include "visrep_internal.h"

namespace {

constexpr int KT = 64;
constexpr int TILE_B = KT * 64 * 2;
constexpr float LOG2E_F = 1.4426950408889634f;
constexpr int RP_THR = 8;                  // the reference moves when a row's tile maximum exceeds it by more than 2^8

struct RelposArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* vt; bf16_t* out;
    const float* rel_h; const float* rel_w;
    int T, S, H, Mk, g0, ldq, ldk, ldvt, ldo;
    unsigned magic;                        // ceil(2^20 / S): n / S = (n * magic) >> 20 for n < 8192
    float sc;                              // softmax scale * log2(e)
};

__global__ __launch_bounds__(256, 2) void attn_fwd_relpos(const RelposArgs p) {
    constexpr int STAGE_B = 2 * TILE_B;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* tab = reinterpret_cast<float*>(smem + 2 * STAGE_B);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lq = lane & 31, hi = lane >> 5;
    const int nqt = (p.T + 127) >> 7;
    int id = xcd_remap(blockIdx.x, gridDim.x);
    const int qt = id % nqt; id /= nqt;
    const int h = id % p.H;
    const int bl = id / p.H, b = bl + p.g0;                    // grid inside this launch (its tables), grid inside the buffers
    const int tok0 = b * p.T, tok1 = tok0 + p.T;
    const int S = p.S, TS = 2 * S + 1;

    const int qloc = qt * 128 + wave * 32 + lq;
    const size_t qrow = (size_t)b * p.T + (qloc < p.T ? qloc : p.T - 1);
    bf16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = *reinterpret_cast<const bf16x8*>(p.q + qrow * p.ldq + h * 64 + kk * 16 + hi * 8);

    const int srow = tid >> 3;
    const int lslot = (tid & 7) ^ ((srow >> 1) & 7);
    const int m_begin = tok0 & ~63;
    const int ntile = (((tok1 + 63) & ~63) - m_begin) >> 6;
    const bf16_t* kcur = p.k + h * 64 + lslot * 8 + (size_t)(m_begin + srow) * p.ldk;
    const bf16_t* vcur = p.vt + (size_t)(h * 64 + srow) * p.ldvt + lslot * 8 + m_begin;
    const size_t kstep = (size_t)KT * p.ldk, khalf = (size_t)32 * p.ldk, vhalf = (size_t)32 * p.ldvt;
    int mt_stage = m_begin;
    auto stage = [&](int buf) {
        char* sk = smem + buf * STAGE_B + wave * 1024;
        char* sv = sk + TILE_B;
        if (mt_stage + KT <= p.Mk) {
#pragma unroll
            for (int j = 0; j < 2; ++j) glds16(kcur + j * khalf, sk + j * 4096);
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int mk = mt_stage + j * 32 + srow;    // rows past the last token are masked below: re-read the last row
                const bf16_t* kr = mk < p.Mk ? kcur + j * khalf : kcur - (size_t)(mt_stage + srow - (p.Mk - 1)) * p.ldk;
                glds16(kr, sk + j * 4096);
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) glds16(vcur + j * vhalf, sv + j * 4096);
        kcur += kstep; vcur += KT; mt_stage += KT;
    };

    stage(0);
    {   // the tables of this block's queries: 128 S contiguous floats of each (fewer in a grid's last query tile; zero behind them)
        const int q0 = qt * 128, nq = p.T - q0 < 128 ? p.T - q0 : 128, nval = nq * S, nall = 128 * S;
        const size_t off = ((size_t)(bl * p.H + h) * p.T + q0) * S;
        for (int i = tid; i < nall; i += 256) {
            const int r = (int)(((unsigned)i * p.magic) >> 20), c = i - r * S;
            tab[r * TS + c] = i < nval ? p.rel_h[off + i] : 0.f;
            tab[r * TS + S + c] = i < nval ? p.rel_w[off + i] : 0.f;
        }
    }
    __syncthreads();

    const int rsw = (lq >> 1) & 7;
    const int rbase = lq * 128;
    const float* trow = tab + (wave * 32 + lq) * TS;

    f32x16 o[2];
    o[0] = f32x16{}; o[1] = f32x16{};
    float m_run = -INFINITY, l_run = 0.f;

    if (qt * 128 + wave * 32 >= p.T) {                         // an empty wave only stages its share and meets the barriers
        for (int it = 0; it < ntile; ++it) {
            if (it + 1 < ntile) stage((it & 1) ^ 1);
            __syncthreads();
        }
        return;
    }
    for (int it = 0; it < ntile; ++it) {
        const int cur = it & 1;
        if (it + 1 < ntile) stage(cur ^ 1);
        const char* sk = smem + cur * STAGE_B;
        const char* sv = sk + TILE_B;

        f32x16 s[2];
        s[0] = f32x16{}; s[1] = f32x16{};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sk + kt2 * 4096 + rbase + (((2 * kk + hi) ^ rsw) << 4));
                s[kt2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], s[kt2], 0, 0, 0);
            }
        // ---- scores -> exponents of 2 with the position term
        const int mt = m_begin + it * KT;
        const int kl0 = mt - tok0 + 4 * hi;
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int kl = kl0 + kt2 * 32 + (r & 3) + 8 * (r >> 2);
                kl = kl < 0 ? 0 : (kl >= p.T ? p.T - 1 : kl);
                const int kh = (int)(((unsigned)kl * p.magic) >> 20), kw = kl - kh * S;
                const float bias = trow[kh] + trow[S + kw];
                s[kt2][r] = __builtin_fmaf(s[kt2][r], p.sc, bias * LOG2E_F);
            }
        if ((mt < tok0) || (mt + KT > tok1)) {                 // wave-uniform: first / last tile of the grid
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = mt + kt2 * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (key < tok0 || key >= tok1) s[kt2][r] = -INFINITY;
                }
        }
        float mloc = fmaxf(fmaxf(s[0][0], s[0][1]), s[0][2]), mloc1 = fmaxf(fmaxf(s[1][0], s[1][1]), s[1][2]);
#pragma unroll
        for (int r = 3; r < 15; r += 2) {
            mloc = fmaxf(fmaxf(mloc, s[0][r]), s[0][r + 1]);
            mloc1 = fmaxf(fmaxf(mloc1, s[1][r]), s[1][r + 1]);
        }
        mloc = fmaxf(fmaxf(mloc, s[0][15]), fmaxf(mloc1, s[1][15]));
        {
            const unsigned u = __builtin_bit_cast(unsigned, mloc);
            const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
            mloc = fmaxf(__builtin_bit_cast(float, (unsigned)sw[0]), __builtin_bit_cast(float, (unsigned)sw[1]));
        }
        const float m_new = __any(mloc - m_run > (float)RP_THR) ? fmaxf(m_run, mloc) : m_run;   // finite: a grid's first tile holds >= 1 valid key
        float psum = 0.f;
        uint32_t pb[2][8];
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float p0 = __builtin_amdgcn_exp2f(s[kt2][r] - m_new), p1 = __builtin_amdgcn_exp2f(s[kt2][r + 1] - m_new);
                psum += p0 + p1;
                pb[kt2][r >> 1] = pack_bf16(p0, p1);
            }
        if (__any(m_new > m_run)) {
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            l_run *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) { o[0][r] *= alpha; o[1][r] *= alpha; }
            m_run = m_new;
        }
        l_run += psum;

#pragma unroll
        for (int c = 0; c < 4; ++c) {
            bf16x8 pf;
            {
                u32x4 w = {pb[c >> 1][4 * (c & 1) + 0], pb[c >> 1][4 * (c & 1) + 1], pb[c >> 1][4 * (c & 1) + 2], pb[c >> 1][4 * (c & 1) + 3]};
                pf = *reinterpret_cast<bf16x8*>(&w);
            }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const bf16x8 vf = *reinterpret_cast<const bf16x8*>(sv + dt * 4096 + rbase + (((2 * c + hi) ^ rsw) << 4));
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[dt], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    l_run += __shfl_xor(l_run, 32);
    const float inv = 1.f / l_run;
    bf16_t* orow = p.out + ((size_t)b * p.T + (qloc < p.T ? qloc : p.T - 1)) * p.ldo + h * 64;
    const bool wide = (p.ldo & 7) == 0 && (reinterpret_cast<uintptr_t>(p.out) & 15) == 0;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int rg = 0; rg < 4; rg += 2) {
            u32x2 a = {pack_bf16(o[dt][4 * rg + 0] * inv, o[dt][4 * rg + 1] * inv), pack_bf16(o[dt][4 * rg + 2] * inv, o[dt][4 * rg + 3] * inv)};
            u32x2 c = {pack_bf16(o[dt][4 * rg + 4] * inv, o[dt][4 * rg + 5] * inv), pack_bf16(o[dt][4 * rg + 6] * inv, o[dt][4 * rg + 7] * inv)};
            if (wide) {
                const auto w0 = __builtin_amdgcn_permlane32_swap(a[0], c[0], false, false);
                const auto w1 = __builtin_amdgcn_permlane32_swap(a[1], c[1], false, false);
                if (qloc < p.T) {
                    const u32x4 q4 = {(unsigned)w0[0], (unsigned)w1[0], (unsigned)w0[1], (unsigned)w1[1]};
                    *reinterpret_cast<u32x4*>(orow + dt * 32 + (rg + hi) * 8) = q4;
                }
            } else if (qloc < p.T) {
                *reinterpret_cast<u32x2*>(orow + dt * 32 + rg * 8 + hi * 4) = a;
                *reinterpret_cast<u32x2*>(orow + dt * 32 + (rg + 1) * 8 + hi * 4) = c;
            }
        }
}

// One thread per table entry: idx = ((g H + h) T + q) 2 S + j; j < S: rel_h[.., kh = j], else rel_w[.., kw = j - S].  The dot product is
// one fmaf chain over c = 0 .. 63 in ascending order starting from +0 (the host twin runs the same chain: equal bit for bit).
__global__ __launch_bounds__(256) void relpos_tables_rows(const bf16_t* __restrict__ q, int ldq, const float* __restrict__ Rh, const float* __restrict__ Rw,
                                                          float* __restrict__ rel_h, float* __restrict__ rel_w, long total, int T, int S, int H) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % (2 * S));
    const long row = idx / (2 * S);                            // (g H + h) T + qi
    const int qi = (int)(row % T);
    const long gh = row / T;
    const int h = (int)(gh % H);
    const long g = gh / H;
    const int qh = qi / S, qw = qi - qh * S;
    const bool isw = j >= S;
    const int kx = isw ? j - S : j;
    const float* R = (isw ? Rw : Rh) + (size_t)((isw ? qw : qh) - kx + S - 1) * 64;
    const bf16_t* qp = q + ((size_t)g * T + qi) * ldq + h * 64;
    float acc = 0.f;
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(qp + c8 * 8);
        const float4 r0 = *reinterpret_cast<const float4*>(R + c8 * 8), r1 = *reinterpret_cast<const float4*>(R + c8 * 8 + 4);
        acc = __builtin_fmaf(bf_lo(w[0]), r0.x, acc); acc = __builtin_fmaf(bf_hi(w[0]), r0.y, acc);
        acc = __builtin_fmaf(bf_lo(w[1]), r0.z, acc); acc = __builtin_fmaf(bf_hi(w[1]), r0.w, acc);
        acc = __builtin_fmaf(bf_lo(w[2]), r1.x, acc); acc = __builtin_fmaf(bf_hi(w[2]), r1.y, acc);
        acc = __builtin_fmaf(bf_lo(w[3]), r1.z, acc); acc = __builtin_fmaf(bf_hi(w[3]), r1.w, acc);
    }
    (isw ? rel_w : rel_h)[row * S + kx] = acc;
}

// Window row r = ((b nw + wy) nw + wx) w w + iy w + ix  <->  map token (b, y = wy w + iy, x = wx w + ix); positions with y >= g or x >= g are
// the zero padding of window_partition, whose projection is the raw bias.
struct WinArgs { int B, g, w, nw, d; };
VR_DEV long win_src(const WinArgs& a, long r) {               // token row of window row r, or -1 for a pad position
    const int ww = a.w * a.w;
    const int t = (int)(r % ww);
    long wi = r / ww;
    const int wx = (int)(wi % a.nw); wi /= a.nw;
    const int wy = (int)(wi % a.nw);
    const long b = wi / a.nw;
    const int iy = t / a.w, ix = t - iy * a.w, y = wy * a.w + iy, x = wx * a.w + ix;
    return (y < a.g && x < a.g) ? (b * a.g + y) * a.g + x : -1;
}
VR_DEV int perm16d(long m) { return (int)((m & ~15L) | ((((m >> 2) & 1) << 1 | ((m >> 3) & 1)) << 2) | (m & 3)); }

// Q | K rows: one block per window row, 16 bytes per thread and step (2 d / 8 chunks)
__global__ __launch_bounds__(256) void sam_window_partition_qk(const bf16_t* __restrict__ qk, int ldqk, const float* __restrict__ bias, bf16_t* __restrict__ out,
                                                               int ldo, const WinArgs a) {
    const long r = blockIdx.x;
    const long src = win_src(a, r);
    for (int c = threadIdx.x; c < 2 * a.d / 8; c += 256) {
        u32x4 v;
        if (src >= 0) v = *reinterpret_cast<const u32x4*>(qk + (size_t)src * ldqk + c * 8);
        else {
            const float4 b0 = *reinterpret_cast<const float4*>(bias + c * 8), b1 = *reinterpret_cast<const float4*>(bias + c * 8 + 4);
            v = u32x4{pack_bf16(b0.x, b0.y), pack_bf16(b0.z, b0.w), pack_bf16(b1.x, b1.y), pack_bf16(b1.z, b1.w)};
        }
        *reinterpret_cast<u32x4*>(out + (size_t)r * ldo + c * 8) = v;
    }
}
// V^T columns: out[n, perm16(r)] = vt[n, perm16(src(r))] or bf16(bias_v[n]); thread = window row r, blockIdx.y = channel n
__global__ __launch_bounds__(256) void sam_window_partition_vt(const bf16_t* __restrict__ vt, int ldvt, const float* __restrict__ bias_v, bf16_t* __restrict__ out,
                                                               int ldo, long rows, const WinArgs a) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int n = blockIdx.y;
    const long src = win_src(a, r);
    out[(size_t)n * ldo + perm16d(r)] = src >= 0 ? vt[(size_t)n * ldvt + perm16d(src)] : f2bf(bias_v[n]);
}
// the inverse on attention output rows: one block per map token, pad queries are dropped
__global__ __launch_bounds__(256) void sam_window_unpartition_rows(const bf16_t* __restrict__ win, int ldw, bf16_t* __restrict__ out, int ldo, const WinArgs a) {
    const long m = blockIdx.x;
    const int x = (int)(m % a.g);
    const long by = m / a.g;
    const int y = (int)(by % a.g);
    const long b = by / a.g;
    const int wy = y / a.w, wx = x / a.w;
    const long r = ((b * a.nw + wy) * a.nw + wx) * a.w * a.w + (y - wy * a.w) * a.w + (x - wx * a.w);
    for (int c = threadIdx.x; c < a.d / 8; c += 256)
        *reinterpret_cast<u32x4*>(out + (size_t)m * ldo + c * 8) = *reinterpret_cast<const u32x4*>(win + (size_t)r * ldw + c * 8);
}

inline bool misaligned(uintptr_t mask, const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & mask) != 0;
}
inline int launched(const char* msg) { return hipGetLastError() == hipSuccess ? 0 : visrep_set_error(VISREP_ERR_LAUNCH, msg); }

}  // namespace

// Grids g0 .. g0 + nb - 1 of buffers that hold NB grids; the tables are those of the nb grids only.  The key tiles stay the global 64-key
// blocks of the whole buffers, so a grid's result does not depend on which launch computes it (visrep_sam_forward's image chunks).
int visrep_mhsa_relpos_range(const void* qk, int ldqk, const void* vt, int ldvt, const float* rel_h, const float* rel_w, void* out, int ldo, int NB,
                             int g0, int nb, int S, int H, int head_dim, float scale, hipStream_t stream) {
    if (head_dim != 64) return visrep_set_error(VISREP_ERR_SHAPE, "mhsa_relpos: only head_dim 64 is implemented");
    if (S < 2 || S > 64) return visrep_set_error(VISREP_ERR_SHAPE, "mhsa_relpos: the grid side S must be 2 .. 64");
    if (!qk || !vt || !rel_h || !rel_w || !out) return visrep_set_error(VISREP_ERR_ARG, "mhsa_relpos: null pointer");
    if (misaligned(15, qk, vt)) return visrep_set_error(VISREP_ERR_ARG, "mhsa_relpos: qk and vt must be 16-byte aligned");
    if (misaligned(7, out)) return visrep_set_error(VISREP_ERR_ARG, "mhsa_relpos: out must be 8-byte aligned");
    if (misaligned(3, rel_h, rel_w)) return visrep_set_error(VISREP_ERR_ARG, "mhsa_relpos: rel_h and rel_w must be 4-byte aligned");
    if (NB <= 0 || H <= 0 || g0 < 0 || nb <= 0 || g0 + nb > NB) return visrep_set_error(VISREP_ERR_SHAPE, "mhsa_relpos: empty problem");
    if (!(scale > 0.f)) return visrep_set_error(VISREP_ERR_ARG, "mhsa_relpos: scale must be > 0 (there is no pre-scaled-Q form: the position term uses the unscaled query)");
    if ((ldqk % 8) || (ldvt % 64) || (ldo % 4)) return visrep_set_error(VISREP_ERR_SHAPE, "mhsa_relpos: bad leading dimension");
    if (ldqk < 2 * H * 64 || ldo < H * 64) return visrep_set_error(VISREP_ERR_SHAPE, "mhsa_relpos: ldqk must cover Q | K (2 H 64 columns) and ldo H 64");
    const int T = S * S;
    const long Mk = (long)NB * T;
    if (Mk > 0x7fffffffL - 64 || (long)((T + 127) / 128) * H * nb > 0x7fffffffL) return visrep_set_error(VISREP_ERR_SHAPE, "mhsa_relpos: more than 2^31 key rows or blocks");
    if (ldvt < ((Mk + 63) / 64) * 64) return visrep_set_error(VISREP_ERR_SHAPE, "mhsa_relpos: ldvt must cover round_up(NB S S, 64)");
    RelposArgs a;
    a.q = (const bf16_t*)qk; a.k = (const bf16_t*)qk + (size_t)H * 64; a.vt = (const bf16_t*)vt; a.out = (bf16_t*)out; a.rel_h = rel_h; a.rel_w = rel_w;
    a.T = T; a.S = S; a.H = H; a.Mk = (int)Mk; a.g0 = g0; a.ldq = ldqk; a.ldk = ldqk; a.ldvt = ldvt; a.ldo = ldo;
    a.magic = ((1u << 20) + S - 1) / S;
    a.sc = scale * LOG2E_F;
    const int lds = 4 * TILE_B + 128 * (2 * S + 1) * 4;        // 32 KB ring + at most 64.5 KB of tables
    static VisrepLdsOptIn opt;
    if (visrep_lds_opt_in(opt, (const void*)attn_fwd_relpos, lds) != hipSuccess) return visrep_set_error(VISREP_ERR_LAUNCH, "mhsa_relpos: LDS opt-in failed");
    visrep_count_route(VISREP_ROUTE_ATTN_RELPOS);
    hipLaunchKernelGGL(attn_fwd_relpos, dim3(((T + 127) / 128) * H * nb), dim3(256), (size_t)lds, stream, a);
    return launched("mhsa_relpos: launch failed");
}

extern "C" int visrep_mhsa_relpos_fwd(const void* qk, int ldqk, const void* vt, int ldvt, const float* rel_h, const float* rel_w, void* out, int ldo,
                                      int NB, int S, int H, int head_dim, float scale, void* stream) {
    return visrep_mhsa_relpos_range(qk, ldqk, vt, ldvt, rel_h, rel_w, out, ldo, NB, 0, NB, S, H, head_dim, scale, (hipStream_t)stream);
}

extern "C" int visrep_relpos_tables(const void* qk, int ldqk, const float* Rh, const float* Rw, float* rel_h, float* rel_w, int NB, int S, int H,
                                    int head_dim, void* stream) {
    if (head_dim != 64) return visrep_set_error(VISREP_ERR_SHAPE, "relpos_tables: only head_dim 64 is implemented");
    if (S < 2 || S > 64) return visrep_set_error(VISREP_ERR_SHAPE, "relpos_tables: the grid side S must be 2 .. 64");
    if (!qk || !Rh || !Rw || !rel_h || !rel_w) return visrep_set_error(VISREP_ERR_ARG, "relpos_tables: null pointer");
    if (misaligned(15, qk, Rh, Rw)) return visrep_set_error(VISREP_ERR_ARG, "relpos_tables: qk, Rh and Rw must be 16-byte aligned");
    if (misaligned(3, rel_h, rel_w)) return visrep_set_error(VISREP_ERR_ARG, "relpos_tables: rel_h and rel_w must be 4-byte aligned");
    if (NB <= 0 || H <= 0) return visrep_set_error(VISREP_ERR_SHAPE, "relpos_tables: empty problem");
    if ((ldqk % 8) || ldqk < H * 64) return visrep_set_error(VISREP_ERR_SHAPE, "relpos_tables: ldqk % 8 == 0 and >= H 64");
    const long total = (long)NB * H * S * S * 2 * S, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) return visrep_set_error(VISREP_ERR_SHAPE, "relpos_tables: more than 2^31 blocks");
    visrep_count_route(VISREP_ROUTE_RELPOS_TABLES);
    hipLaunchKernelGGL(relpos_tables_rows, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qk, ldqk, Rh, Rw, rel_h, rel_w, total,
                       S * S, S, H);
    return launched("relpos_tables: launch failed");
}

static int win_check(int B, int g, int w, int d, WinArgs& a) {
    if (B <= 0 || g <= 0 || w <= 0 || d <= 0 || d % 8) return visrep_set_error(VISREP_ERR_SHAPE, "sam_window: B, g, window > 0 and d % 8 == 0 required");
    a.B = B; a.g = g; a.w = w; a.nw = (g + w - 1) / w; a.d = d;
    if ((long)B * a.nw * a.nw * w * w > 0x7fffffffL) return visrep_set_error(VISREP_ERR_SHAPE, "sam_window: more than 2^31 window rows");
    return 0;
}

extern "C" int visrep_sam_window_partition(const void* qk, int ldqk, const void* vt, int ldvt, const float* bias, void* qk_win, int ldqw, void* vt_win,
                                           int ldvw, int B, int g, int window, int d, void* stream) {
    if (!qk || !vt || !bias || !qk_win || !vt_win) return visrep_set_error(VISREP_ERR_ARG, "sam_window_partition: null pointer");
    if (misaligned(15, qk, bias, qk_win)) return visrep_set_error(VISREP_ERR_ARG, "sam_window_partition: qk, bias and qk_win must be 16-byte aligned");
    if (misaligned(1, vt, vt_win)) return visrep_set_error(VISREP_ERR_ARG, "sam_window_partition: vt and vt_win must be 2-byte aligned");
    WinArgs a;
    if (int rc = win_check(B, g, window, d, a)) return rc;
    const long rows = (long)B * a.nw * a.nw * window * window, M = (long)B * g * g;
    if ((ldqk % 8) || (ldqw % 8) || ldqk < 2 * d || ldqw < 2 * d) return visrep_set_error(VISREP_ERR_SHAPE, "sam_window_partition: ldqk, ldqw % 8 == 0 and >= 2 d");
    if (ldvt < (M + 15) / 16 * 16 || ldvw < (rows + 15) / 16 * 16) return visrep_set_error(VISREP_ERR_SHAPE, "sam_window_partition: ldvt / ldvw must cover the rows rounded up to 16");
    if (d > 65535) return visrep_set_error(VISREP_ERR_SHAPE, "sam_window_partition: d <= 65535");
    hipStream_t s = (hipStream_t)stream;
    visrep_count_route(VISREP_ROUTE_SAM_PARTITION);
    hipLaunchKernelGGL(sam_window_partition_qk, dim3((unsigned)rows), dim3(256), 0, s, (const bf16_t*)qk, ldqk, bias, (bf16_t*)qk_win, ldqw, a);
    hipLaunchKernelGGL(sam_window_partition_vt, dim3((unsigned)((rows + 255) / 256), (unsigned)d), dim3(256), 0, s, (const bf16_t*)vt, ldvt, bias + 2 * d,
                       (bf16_t*)vt_win, ldvw, rows, a);
    return launched("sam_window_partition: launch failed");
}

extern "C" int visrep_sam_window_unpartition(const void* win, int ldw, void* out, int ldo, int B, int g, int window, int d, void* stream) {
    if (!win || !out) return visrep_set_error(VISREP_ERR_ARG, "sam_window_unpartition: null pointer");
    if (misaligned(15, win, out)) return visrep_set_error(VISREP_ERR_ARG, "sam_window_unpartition: win and out must be 16-byte aligned");
    WinArgs a;
    if (int rc = win_check(B, g, window, d, a)) return rc;
    if ((ldw % 8) || (ldo % 8) || ldw < d || ldo < d) return visrep_set_error(VISREP_ERR_SHAPE, "sam_window_unpartition: ldw, ldo % 8 == 0 and >= d");
    visrep_count_route(VISREP_ROUTE_SAM_PARTITION);
    hipLaunchKernelGGL(sam_window_unpartition_rows, dim3((unsigned)((long)B * g * g)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)win, ldw, (bf16_t*)out, ldo, a);
    return launched("sam_window_unpartition: launch failed");
}
