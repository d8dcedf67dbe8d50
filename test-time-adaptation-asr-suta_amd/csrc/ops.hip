// Non-GEMM kernels of the SUTA step for gfx950: waveform normalisation, conv0 stencil,
// GroupNorm forward+backward with per-utterance affine gradients (LayerNorm: norm.hip), attention
// softmax forward/backward, the fused entropy+MCC loss-and-grad, and AdamW with
// duplicate-entry multiplicity.  All reductions are fixed-order (bitwise reproducible).
#include "ops.h"
#include <algorithm>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>

namespace {

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
    // 256-thread block reduction (4 waves)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    T s = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return s;
}

// ------------------------------------------------------------------------------------------
// waveform normalisation (one block per utterance)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wave_normalize_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                             long N, const int* __restrict__ lens) {
    __shared__ double red[4];
    const float* xb = x + (long)blockIdx.x * N;
    float* yb = y + (long)blockIdx.x * N;
    const long n = lens ? lens[blockIdx.x] : N;  // ragged batch: utterance length within the N stride
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) s += xb[i];
    s = block_sum(s, red);
    const double mean = s / (double)n;
    double q = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) {
        const double d = (double)xb[i] - mean;
        q += d * d;
    }
    q = block_sum(q, red);
    const float meanf = (float)mean;
    const float denom = (float)sqrt(q / (double)n + 1e-7);
    for (long i = threadIdx.x; i < N; i += 256) yb[i] = i < n ? (xb[i] - meanf) / denom : 0.f;
}

// ------------------------------------------------------------------------------------------
// conv0 (1 -> C channels, kernel K <= 16, stride S): time-major output
// block: 32 output frames x all channels; x segment staged in LDS
// ------------------------------------------------------------------------------------------
constexpr int C0_ROWS = 32;
__global__ __launch_bounds__(256) void conv0_kernel(const float* __restrict__ x, long N, const float* __restrict__ W,
                                                    const float* __restrict__ bias, long wstride,
                                                    float* __restrict__ z, int L0, int C, int K, int S) {
    __shared__ float xs[C0_ROWS * 16 + 16];
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * C0_ROWS;
    const float* xb = x + (long)b * N;
    const float* Wb = W + (long)b * wstride;
    const float* bb = bias ? bias + (long)b * wstride : nullptr;
    const int nx = (C0_ROWS - 1) * S + K;
    for (int i = threadIdx.x; i < nx; i += 256) {
        const long gi = (long)t0 * S + i;
        xs[i] = gi < N ? xb[gi] : 0.f;
    }
    __syncthreads();
    const int rows = min(C0_ROWS, L0 - t0);
    float* zb = z + ((long)b * L0 + t0) * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        float w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = k < K ? Wb[(long)k * C + c] : 0.f;
        const float bv = bb ? bb[c] : 0.f;
        for (int r = 0; r < rows; ++r) {
            float acc = 0.f;
            // same summation order as a k-ordered dot product
            for (int k = 0; k < K; ++k) acc = fmaf(xs[r * S + k], w[k], acc);
            zb[(long)r * C + c] = acc + bv;
        }
    }
}

// Vectorised form (layer-norm conv stack: conv0 output stored): a thread owns 4 consecutive channels
// (C / 4 threads per frame, 256 / (C / 4) frames per pass), taps KT / stride ST compile-time, 16-B stores;
// per-element arithmetic and order as conv0_kernel.  Requires C % 4 == 0 and 256 % (C / 4) == 0.
constexpr int C0V_ROWS = 64;
template <int KT, int ST>
__global__ __launch_bounds__(256) void conv0_vec_kernel(const float* __restrict__ x, long N,
                                                        const float* __restrict__ W, const float* __restrict__ bias,
                                                        long wstride, float* __restrict__ z, int L0, int C,
                                                        __bf16* __restrict__ zb) {
    __shared__ float xs[C0V_ROWS * ST + KT + 16];
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * C0V_ROWS;
    const float* xb = x + (long)b * N;
    const int nx = (C0V_ROWS - 1) * ST + KT;
    for (int i = threadIdx.x; i < nx; i += 256) {
        const long gi = (long)t0 * ST + i;
        xs[i] = gi < N ? xb[gi] : 0.f;
    }
    __syncthreads();
    const int cpr = C / 4, fpp = 256 / cpr;  // threads per frame, frames per pass
    const int c = 4 * (threadIdx.x % cpr), fr = threadIdx.x / cpr;
    const float* Wb = W + (long)b * wstride;
    f32x4 w[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) w[k] = *reinterpret_cast<const f32x4*>(Wb + (long)k * C + c);
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias) bv = *reinterpret_cast<const f32x4*>(bias + (long)b * wstride + c);
    const int rows = min(C0V_ROWS, L0 - t0);
    const long o0 = ((long)b * L0 + t0) * C + c;
    for (int r = fr; r < rows; r += fpp) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const float xv = xs[r * ST + k];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(xv, w[k][e], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = acc[e] + bv[e];
        if (zb) store_bf16x4(zb + o0 + (long)r * C, acc);  // bf16 storage (conv stack on bf16 planes)
        else *reinterpret_cast<f32x4*>(z + o0 + (long)r * C) = acc;
    }
}

// ------------------------------------------------------------------------------------------
// per-utterance column statistics (GroupNorm with groups == channels), double partials
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void col_stats_final(const double* __restrict__ part, int nchunk, int rows, int C,
                                                       float eps, float* __restrict__ mean, float* __restrict__ rstd,
                                                       const int* __restrict__ rows_b) {
    const int b = blockIdx.y;
    if (rows_b) rows = rows_b[b];
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) {
        const double* pb = part + ((long)b * nchunk + ch) * 2 * C;
        s += pb[c];
        q += pb[C + c];
    }
    const double m = s / rows;
    double var = q / rows - m * m;
    if (var < 0) var = 0;
    mean[(long)b * C + c] = (float)m;
    rstd[(long)b * C + c] = (float)(1.0 / sqrt(var + (double)eps));
}

// finalize: dgamma = sum dg*xhat, dbeta = sum dg; also writes coefficients for the dx pass
__global__ __launch_bounds__(256) void gn_bwd_final(const double* __restrict__ part, int nchunk, int C,
                                                    float* __restrict__ dgamma, float* __restrict__ dbeta, long gstride,
                                                    float* __restrict__ coef) {
    const int b = blockIdx.y;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) {
        const double* pb = part + ((long)b * nchunk + ch) * 2 * C;
        s += pb[c];
        q += pb[C + c];
    }
    dgamma[(long)b * gstride + c] = (float)q;
    dbeta[(long)b * gstride + c] = (float)s;
    coef[((long)b * C + c) * 2 + 0] = (float)s;
    coef[((long)b * C + c) * 2 + 1] = (float)q;
}
// ------------------------------------------------------------------------------------------
// Fused conv0 + GroupNorm(+GELU) front-end (feat_extract_norm "group").  conv0 (K <= 16 taps,
// 1 input channel) is recomputed from the waveform in every pass instead of being stored, so the
// front-end moves the 512-channel activation through HBM only as a0 (written once) and da0/dg
// (read/written in the backward).  Block: F0_ROWS frames x all channels, waveform segment in LDS.
//   MODE 0: per-channel partial sum / sum of squares of z (double)          -> part
//   MODE 1: a = gelu(((z - mean) * rstd) * g + beta)                         -> a
//   MODE 2: dg = da * gelu'(xhat * g + beta): partial sum(dg), sum(dg * xhat) (read-only pass)
//   MODE 3: dg recomputed from da as in MODE 2, dz = rstd*g*(dg - S/L - xhat*Q/L); partial
//           dW[k][c] = sum_t dz[t][c] x[s t + k]   (the backward reads da twice and writes nothing
//           activation-sized: dg is never stored)
// ------------------------------------------------------------------------------------------
constexpr int F0_ROWS = 128;
// KT/ST: compile-time taps/stride (every wav2vec2 conv0 is K = 10, S = 5) -- keeps the filter in
// statically indexed registers and lets the tap loop unroll; KT = 0 is the generic (K <= 16) path.
template <int MODE, int KT, int ST, bool FG = false>  // FG: branch-free GELU / GELU' (common.h gelu_fast)
__global__ __launch_bounds__(256) void conv0_gn_kernel(const float* __restrict__ x, long N, const float* __restrict__ W,
                                                       const float* __restrict__ bias, long wstride, int L0, int C,
                                                       int K, int S, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const float* __restrict__ g,
                                                       const float* __restrict__ beta, float* __restrict__ io,
                                                       const float* __restrict__ coef, double* __restrict__ dpart,
                                                       float* __restrict__ fpart, int nchunk,
                                                       const int* __restrict__ L0s) {
    __shared__ float xs[F0_ROWS * 16 + 16];
    if (KT > 0) {
        K = KT;
        S = ST;
    }
    const int b = blockIdx.y, ch = blockIdx.x;
    const int t0 = ch * F0_ROWS;
    const float* xb = x + (long)b * N;
    const int nx = (F0_ROWS - 1) * S + K;
    for (int i = threadIdx.x; i < nx; i += 256) {
        const long gi = (long)t0 * S + i;
        xs[i] = gi < N ? xb[gi] : 0.f;
    }
    __syncthreads();
    // ragged batch: statistics and gradients over the utterance's Lb valid frames; MODE 1 also
    // fills the padding frames of the layout (finite values, never read as data)
    const int Lb = L0s ? L0s[b] : L0;
    const int rows = MODE == 1 ? min(F0_ROWS, L0 - t0) : min(F0_ROWS, Lb - t0);
    const float* Wb = W + (long)b * wstride;
    const float* bb = bias ? bias + (long)b * wstride : nullptr;
    float* iob = io ? io + ((long)b * L0 + t0) * C : nullptr;
    const float invL = 1.0f / Lb;
    for (int c = threadIdx.x; c < C; c += 256) {
        float w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = k < K ? Wb[(long)k * C + c] : 0.f;
        const float bv = bb ? bb[c] : 0.f;
        float mu = 0.f, rs = 0.f, gg = 0.f, bt = 0.f, sS = 0.f, sQ = 0.f;
        if (MODE >= 1) {
            mu = mean[(long)b * C + c];
            rs = rstd[(long)b * C + c];
            gg = g[(long)b * wstride + c];
            bt = beta[(long)b * wstride + c];
        }
        if (MODE == 3) {
            sS = coef[((long)b * C + c) * 2 + 0] * invL;
            sQ = coef[((long)b * C + c) * 2 + 1] * invL;
        }
        double a0 = 0.0, a1 = 0.0;
        float dw[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) dw[k] = 0.f;
#pragma unroll 8  // 8 rows of io loads in flight per lane (the backward modes are latency-bound at 2)
        for (int r = 0; r < rows; ++r) {
            float z = 0.f;
#pragma unroll
            for (int k = 0; k < (KT > 0 ? KT : 16); ++k)  // same order as conv0_kernel
                if (KT > 0 || k < K) z = fmaf(xs[r * S + k], w[k], z);
            z += bv;
            if (MODE == 0) {
                a0 += z;
                a1 += (double)z * z;
            } else {
                const float xh = (z - mu) * rs;
                const long o = (long)r * C + c;
                if (MODE == 1) {
                    iob[o] = FG ? gelu_fast(xh * gg + bt) : gelu_f(xh * gg + bt);
                } else if (MODE == 2) {
                    const float dg = iob[o] * (FG ? dgelu_fast(xh * gg + bt) : dgelu_f(xh * gg + bt));
                    a0 += dg;
                    a1 += (double)dg * xh;
                } else {
                    // recomputed bitwise, as in MODE 2
                    const float dg = iob[o] * (FG ? dgelu_fast(xh * gg + bt) : dgelu_f(xh * gg + bt));
                    const float dz = rs * gg * (dg - sS - xh * sQ);
#pragma unroll
                    for (int k = 0; k < (KT > 0 ? KT : 16); ++k)
                        if (KT > 0 || k < K) dw[k] = fmaf(dz, xs[r * S + k], dw[k]);
                }
            }
        }
        if (MODE == 0 || MODE == 2) {
            double* pb = dpart + ((long)b * nchunk + ch) * 2 * C;
            pb[c] = a0;
            pb[C + c] = a1;
        }
        if (MODE == 3) {
            float* pf = fpart + ((long)b * nchunk + ch) * K * (long)C;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < K) pf[(long)k * C + c] = dw[k];
        }
    }
}

// dW[b][k][c] = sum over chunks (fixed order) of the MODE-3 partials
__global__ __launch_bounds__(256) void conv0_dw_reduce(const float* __restrict__ fpart, int nchunk, int KC,
                                                       float* __restrict__ dW, long gstride) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= KC) return;
    double s = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) s += fpart[((long)b * nchunk + ch) * KC + i];
    dW[(long)b * gstride + i] = (float)s;
}


// ------------------------------------------------------------------------------------------
// Grouped positional conv (wav2vec2 pos_conv_embed: K taps, G groups of CG channels, "same" padding)
// as one kernel: out[t][co] = sum_q sum_ci x[t + q - pad][ci] W[q][ci][co] over one group, x rows
// outside [0, len) are zero.  Block = WB waves = 16*WB output frames x CG channels of one
// (utterance, group): the input window (16*WB + K - 1 frames) is staged in LDS once, the group's
// weights stream through two LDS buffers of CHT taps (register-staged, one barrier per chunk), and
// each wave runs exact-fp32 v_mfma_f32_16x16x4_f32 on its 16 frames x CG channels (CG/16 fragments).
//   FWD: C = R + gelu(acc + bias), C2 = acc + bias (pre-activation);  BWD: C = acc + R, rows >= len -> 0
//   STK (a layer of data2vec-audio's positional stack; LayerNorm and GELU follow in ln_gelu_fwd_kernel):
//   FWD: C = acc + bias only;  BWD: C = acc (+ R when given: the layer nearest the stack's input), rows >= len -> 0
// K is a multiple of CHT: a kernel size that is not (data2vec's 19) comes with zero taps appended to the weights
// (launch_posconv_stack), whose window rows exist and contribute nothing.
// Blocks of one group run on one XCD (its weights stay in that L2).
// ------------------------------------------------------------------------------------------
template <int CG>
struct PcLayout {
    static constexpr int XS = CG + 4;                        // window row stride (conflict-free A reads)
    static constexpr int WS = (CG % 64 == 0) ? CG + 16 : CG;  // weight row stride (conflict-free B reads)
};

template <int CG, int WB, int CHT, bool FWD, bool STK = false>
__global__ __launch_bounds__(WB * 64, 1) void posconv_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                             const float* __restrict__ bias,
                                                             const float* __restrict__ R, float* __restrict__ C,
                                                             float* __restrict__ C2, int T, int H, int G, int K,
                                                             int pad, const int* __restrict__ tlen, int ntile,
                                                             int nutt) {
    constexpr int NT = WB * 64, NC = CG / 16, XS = PcLayout<CG>::XS, WS = PcLayout<CG>::WS;
    constexpr int WROWS = 16 * WB;
    constexpr int CHUNK4 = CHT * CG * CG / 4;             // float4 per weight chunk
    constexpr int LPT = (CHUNK4 + NT - 1) / NT;           // float4 per thread per chunk
    extern __shared__ __attribute__((aligned(16))) float pc_smem[];
    float* win = pc_smem;                                  // [WROWS + K - 1][XS]
    float* wbuf = pc_smem + (WROWS + K - 1) * XS;          // 2 x [CHT*CG][WS]

    // block -> (group, utterance, tile) with each XCD owning whole groups: hardware block b runs on
    // XCD b % 8; logical id = xcd-major
    const int nb = gridDim.x;
    int L = blockIdx.x;
    if ((nb & 7) == 0) L = (L & 7) * (nb >> 3) + (L >> 3);
    const int tile = L % ntile;
    const int u = (L / ntile) % nutt;
    const int gi = L / (ntile * nutt);
    const int t0 = tile * WROWS;
    const int tl = tlen ? tlen[u] : T;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, g = lane >> 4;
    const float* xb = x + (long)u * T * H + gi * CG;
    const float* wg = W + (long)gi * K * CG * CG;

    // input window: frames t0 - pad .. t0 + WROWS - 1 + (K - 1 - pad)
    const int nwin = (WROWS + K - 1) * (CG / 4);
    for (int it = threadIdx.x; it < nwin; it += NT) {
        const int row = it / (CG / 4), c4 = (it % (CG / 4)) * 4;
        const int t = t0 - pad + row;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < tl) v = *reinterpret_cast<const f32x4*>(xb + (long)t * H + c4);
        *reinterpret_cast<f32x4*>(win + row * XS + c4) = v;
    }
    f32x4 st[LPT];
    auto load_chunk = [&](int c) {
        const float* src = wg + (long)c * CHT * CG * CG;
#pragma unroll
        for (int n = 0; n < LPT; ++n) {
            const int it = threadIdx.x + n * NT;
            st[n] = it < CHUNK4 ? *reinterpret_cast<const f32x4*>(src + it * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_chunk = [&](int buf) {
        float* dst = wbuf + buf * (CHT * CG * WS);
#pragma unroll
        for (int n = 0; n < LPT; ++n) {
            const int it = threadIdx.x + n * NT;
            if (it < CHUNK4) {
                const int row = (it * 4) / CG, col = (it * 4) % CG;
                *reinterpret_cast<f32x4*>(dst + row * WS + col) = st[n];
            }
        }
    };
    f32x4 acc[NC];
#pragma unroll
    for (int nf = 0; nf < NC; ++nf) acc[nf] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nch = K / CHT;
    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    const float* arow = win + (16 * w + r) * XS + g;
    for (int c = 0; c < nch; ++c) {
        if (c + 1 < nch) load_chunk(c + 1);
        const float* wb = wbuf + (c & 1) * (CHT * CG * WS) + g * WS + r;
#pragma unroll
        for (int qq = 0; qq < CHT; ++qq) {
            const float* ap = arow + (c * CHT + qq) * XS;
            const float* bp = wb + qq * CG * WS;
#pragma unroll
            for (int j = 0; j < CG / 4; ++j) {
                const float a = ap[4 * j];
                float b[NC];
#pragma unroll
                for (int nf = 0; nf < NC; ++nf) b[nf] = bp[4 * j * WS + 16 * nf];
#pragma unroll
                for (int nf = 0; nf < NC; ++nf) acc[nf] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[nf], acc[nf], 0, 0, 0);
            }
        }
        if (c + 1 < nch) store_chunk((c + 1) & 1);
        __syncthreads();
    }
    // epilogue: lane holds out[t0 + 16w + 4g + i][16nf + r]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + 16 * w + 4 * g + i;
        if (t >= T) continue;
        const long o = ((long)u * T + t) * H + gi * CG;
#pragma unroll
        for (int nf = 0; nf < NC; ++nf) {
            const int co = 16 * nf + r;
            float v;
            if (FWD) {
                v = acc[nf][i] * 1.0f + bias[gi * CG + co];
                if (!STK) {
                    C2[o + co] = v;
                    v = gelu_f(v) + R[o + co];
                }
            } else {
                v = acc[nf][i];
                if (!STK || R) v += R[o + co];
                if (tlen && t >= tl) v = 0.f;
            }
            C[o + co] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Positional conv in bf16 mode (config C4, group width 64): the same contraction as posconv_kernel
// with the operands rounded to bf16 (RNE) on v_mfma_f32_32x32x16_bf16, fp32 accumulation and epilogue.
// Block = WB waves = 32*WB output frames x 64 channels of one (group, utterance, frame tile); the input
// window (32*WB + K - 1 frames) is staged once as a bf16 image [row][64 + 8] (144-B rows: the 16-B
// fragment reads of 32 consecutive rows are conflict-free); the group's bf16 weights Wt[tap][n][k]
// (n = output channel, k = input channel, built once at suta_create) stream through two LDS chunks of
// PCB_CHT taps, register-staged.  Wave = 32 frames x 64 channels = two 32x32 accumulators; per tap 4
// k-steps x 2 MFMAs.  FWD / BWD epilogues as posconv_kernel.
// ------------------------------------------------------------------------------------------
constexpr int PCB_CHT = 4;   // taps per weight chunk
constexpr int PCB_RS = 72;   // bf16 row stride of the window and weight images
template <int WB, bool FWD>
__global__ __launch_bounds__(WB * 64, 1) void posconv_bf16_kernel(const float* __restrict__ x,
                                                                  const __bf16* __restrict__ Wt,
                                                                  const float* __restrict__ bias,
                                                                  const float* __restrict__ R, float* __restrict__ C,
                                                                  float* __restrict__ C2, int T, int H, int G, int K,
                                                                  int pad, const int* __restrict__ tlen, int ntile,
                                                                  int nutt) {
    constexpr int CG = 64, NT = WB * 64, WROWS = 32 * WB;
    constexpr int CHUNK = PCB_CHT * CG * CG / 8;  // 16-B items per weight chunk
    constexpr int LPT = (CHUNK + NT - 1) / NT;
    extern __shared__ __attribute__((aligned(16))) __bf16 pcb_smem[];
    __bf16* win = pcb_smem;                             // [WROWS + K - 1][PCB_RS]
    __bf16* wbuf = pcb_smem + (WROWS + K - 1) * PCB_RS;  // 2 x [PCB_CHT * 64][PCB_RS]
    typedef __bf16 b8 __attribute__((ext_vector_type(8)));
    typedef __bf16 b4 __attribute__((ext_vector_type(4)));

    const int nb = gridDim.x;
    int L = blockIdx.x;
    if ((nb & 7) == 0) L = (L & 7) * (nb >> 3) + (L >> 3);  // a group's blocks on one XCD
    const int tile = L % ntile;
    const int u = (L / ntile) % nutt;
    const int gi = L / (ntile * nutt);
    const int t0 = tile * WROWS;
    const int tl = tlen ? tlen[u] : T;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, l32 = lane & 31, h = lane >> 5;
    const float* xb = x + (long)u * T * H + gi * CG;
    const __bf16* wg = Wt + (long)gi * K * CG * CG;

    const int nwin = (WROWS + K - 1) * (CG / 4);
    for (int it = threadIdx.x; it < nwin; it += NT) {
        const int row = it / (CG / 4), c4 = (it % (CG / 4)) * 4;
        const int t = t0 - pad + row;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < tl) v = *reinterpret_cast<const f32x4*>(xb + (long)t * H + c4);
        b4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (__bf16)v[e];
        *reinterpret_cast<b4*>(win + row * PCB_RS + c4) = o;
    }
    b8 st[LPT];
    auto load_chunk = [&](int c) {
        const b8* src = reinterpret_cast<const b8*>(wg + (long)c * PCB_CHT * CG * CG);
#pragma unroll
        for (int n = 0; n < LPT; ++n) {
            const int it = threadIdx.x + n * NT;
            if (it < CHUNK) st[n] = src[it];
        }
    };
    auto store_chunk = [&](int buf) {
        __bf16* dst = wbuf + buf * (PCB_CHT * CG * PCB_RS);
#pragma unroll
        for (int n = 0; n < LPT; ++n) {
            const int it = threadIdx.x + n * NT;
            if (it < CHUNK) *reinterpret_cast<b8*>(dst + (it >> 3) * PCB_RS + (it & 7) * 8) = st[n];
        }
    };
    f32x16 acc[2];
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[nf][v] = 0.f;
    const int nch = K / PCB_CHT;
    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    const __bf16* arow = win + (32 * w + l32) * PCB_RS + 8 * h;
    for (int c = 0; c < nch; ++c) {
        if (c + 1 < nch) load_chunk(c + 1);
        const __bf16* wb = wbuf + (c & 1) * (PCB_CHT * CG * PCB_RS) + l32 * PCB_RS + 8 * h;
#pragma unroll
        for (int qq = 0; qq < PCB_CHT; ++qq) {
            const __bf16* ap = arow + (c * PCB_CHT + qq) * PCB_RS;
            const __bf16* bp = wb + qq * CG * PCB_RS;
#pragma unroll
            for (int kc = 0; kc < CG / 16; ++kc) {
                const b8 a = *reinterpret_cast<const b8*>(ap + 16 * kc);
#pragma unroll
                for (int nf = 0; nf < 2; ++nf)
                    acc[nf] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        a, *reinterpret_cast<const b8*>(bp + 32 * nf * PCB_RS + 16 * kc), acc[nf], 0, 0, 0);
            }
        }
        if (c + 1 < nch) store_chunk((c + 1) & 1);
        __syncthreads();
    }
    // epilogue: acc[nf][v] = out[t0 + 32 w + r8(v, h)][32 nf + l32]
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int t = t0 + 32 * w + 8 * (v >> 2) + 4 * h + (v & 3);
        if (t >= T) continue;
        const long o = ((long)u * T + t) * H + gi * CG;
#pragma unroll
        for (int nf = 0; nf < 2; ++nf) {
            const int co = 32 * nf + l32;
            float val;
            if (FWD) {
                val = acc[nf][v] + bias[gi * CG + co];
                C2[o + co] = val;
                val = gelu_f(val) + R[o + co];
            } else {
                val = acc[nf][v] + R[o + co];
                if (tlen && t >= tl) val = 0.f;
            }
            C[o + co] = val;
        }
    }
}

// ------------------------------------------------------------------------------------------
// attention softmax over rows of length T (<= 64*NPL), one wave per row
// ------------------------------------------------------------------------------------------
template <int NPL>
__global__ __launch_bounds__(256) void softmax_rows_kernel(float* __restrict__ s, long nrows, int T, long ld,
                                                           const int* __restrict__ tlen, long rows_per_utt) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;
    float* r = s + row * ld;
    const int Tl = T;  // layout width; keys >= the utterance's length get probability 0
    if (tlen) T = tlen[row / rows_per_utt];
    float v[NPL];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int c = lane + i * 64;
        v[i] = c < T ? r[c] : -INFINITY;
        mx = fmaxf(mx, v[i]);
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int c = lane + i * 64;
        v[i] = c < T ? expf(v[i] - mx) : 0.f;
        sum += v[i];
    }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int c = lane + i * 64;
        if (c < Tl) r[c] = c < T ? v[i] * inv : 0.f;
    }
}

// delta[b][h][t] = sum_d dO[b][t][h*dh + d] * O[b][t][h*dh + d]   (= rowsum(P * dP) of the softmax backward)
// delta[b][h][t] = sum_d dctx[b,t,h,d] * ctx[b,t,h,d].  Items (row, head) are dh contiguous floats, so
// G = dh/4 lanes each load one 16-B vector of an item and reduce over their lane group (coalesced).
template <int G>
__global__ __launch_bounds__(256) void attn_delta_kernel(const f32x4* __restrict__ dO, const f32x4* __restrict__ O,
                                                         float* __restrict__ delta, long items, int T, int NH) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long item = g / G;
    float s = 0.f;
    if (item < items) {
        const f32x4 a = dO[g], c = O[g];
        s = fmaf(a[3], c[3], fmaf(a[2], c[2], fmaf(a[1], c[1], a[0] * c[0])));  // (gemm_hbx's EPI_DELTA: same order)
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (item < items && (g % G) == 0) {
        const long row = item / NH;
        const int hh = (int)(item % NH);
        const long b = row / T, t = row % T;
        delta[(b * NH + hh) * T + t] = s;
    }
}

// Head dims that are no power of two (80, 120: XLS-R 1B / 2B): 32 lanes per item, the first dh / 4 of them load
// one 16-B vector each (dh <= 128), the same lane-group reduction.
__global__ __launch_bounds__(256) void attn_delta_pad32_kernel(const f32x4* __restrict__ dO, const f32x4* __restrict__ O,
                                                               float* __restrict__ delta, long items, int T, int NH,
                                                               int nv) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long item = g >> 5;
    const int j = (int)(g & 31);
    float s = 0.f;
    if (item < items && j < nv) {
        const f32x4 a = dO[item * nv + j], c = O[item * nv + j];
        s = fmaf(a[3], c[3], fmaf(a[2], c[2], fmaf(a[1], c[1], a[0] * c[0])));
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (item < items && j == 0) {
        const long row = item / NH;
        const int hh = (int)(item % NH);
        const long b = row / T, t = row % T;
        delta[(b * NH + hh) * T + t] = s;
    }
}

__global__ __launch_bounds__(256) void attn_delta_scalar(const float* __restrict__ dO, const float* __restrict__ O,
                                                         float* __restrict__ delta, long items, int T, int NH,
                                                         int dh) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    float s = 0.f;
    for (int d = 0; d < dh; ++d) s = fmaf(dO[i * dh + d], O[i * dh + d], s);
    const long row = i / NH;
    const long b = row / T, t = row % T;
    delta[(b * NH + i % NH) * T + t] = s;
}

__global__ __launch_bounds__(256) void dgelu_mul_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                        float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = g[i] * dgelu_f(z[i]);
}

// ------------------------------------------------------------------------------------------
// fused SUTA loss + gradient, one 256-thread block per utterance, V <= 64 (lane = class)
// The MCC term divides by the reference's mcc_loss default class_num = 32 (main.py:30, 42; the call at
// main.py:198 never passes the vocabulary size), not by V.
// scratch per utterance: P[T][64], H[T] (floats)
// ------------------------------------------------------------------------------------------
constexpr int MCC_CLASS_NUM = 32;

__global__ __launch_bounds__(256) void suta_loss_kernel(const float* __restrict__ logits, int T, int V, LossHP hp,
                                                        float* __restrict__ dlogits, float* __restrict__ loss_out,
                                                        float* __restrict__ scratch, const int* __restrict__ tlen) {
    __shared__ double Cm[64 * 64];
    __shared__ float Sm[64 * 64];
    __shared__ double redd[4][4];
    __shared__ double colsum[4][64];
    __shared__ double rvec[64], rho[64], clsv[64];
    __shared__ double scal[8];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int Tl = T;  // layout stride (frames); the utterance has T <= Tl valid frames
    const float* L = logits + (long)b * Tl * V;
    float* dL = dlogits + (long)b * Tl * V;
    float* Ps = scratch + (long)b * Tl * 66;
    float* Hs = Ps + (long)Tl * 64;
    if (tlen) {
        T = tlen[b];
        for (long i = (long)T * V + threadIdx.x; i < (long)Tl * V; i += 256) dL[i] = 0.f;  // padding frames
    }
    float* Ws = Hs + Tl;
    const bool act = lane < V;
    const float invt = 1.0f / hp.temp;

    // ---- phase 1: per-row softmax, entropy, argmax ----
    double kcnt = 0.0, wsum = 0.0, hsum_m = 0.0, hsum_all = 0.0;
    double cls = 0.0;  // per-lane column sum of raw logits (div loss)
    for (int t = w; t < T; t += 4) {
        const float l = act ? L[(long)t * V + lane] : -INFINITY;
        if (act) cls += l;
        const float zv = l * invt;
        const float mx = wave_max(zv);
        const float e = act ? expf(zv - mx) : 0.f;
        const float s = wave_sum(e);
        const float p = e / s;
        const float lp = zv - mx - logf(s);
        const float H = -wave_sum(act ? p * lp : 0.f);
        // argmax of raw logits, first max wins
        float bv = l;
        int bi = act ? lane : 1 << 30;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        const bool m = bi != 0;
        Ps[(long)t * 64 + lane] = p;
        if (lane == 0) Hs[t] = H;
        kcnt += m ? 1.0 : 0.0;
        wsum += 1.0 + exp(-(double)H);
        hsum_m += m ? (double)H : 0.0;
        hsum_all += H;
    }
    if (lane == 0) {
        redd[w][0] = kcnt;
        redd[w][1] = wsum;
        redd[w][2] = hsum_m;
        redd[w][3] = hsum_all;
    }
    colsum[w][lane] = cls;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 0; j < 4; ++j) scal[j] = redd[0][j] + redd[1][j] + redd[2][j] + redd[3][j];
    }
    if (threadIdx.x < 64) clsv[threadIdx.x] = colsum[0][threadIdx.x] + colsum[1][threadIdx.x] +
                                              colsum[2][threadIdx.x] + colsum[3][threadIdx.x];
    __syncthreads();
    const double K = scal[0], Wsum = scal[1];
    const bool use_mcc = 1.0f - hp.em_coef > 0.f;
    for (int t = threadIdx.x; t < T; t += 256)
        Ws[t] = hp.reweight ? (float)((double)T * (1.0 + exp(-(double)Hs[t])) / Wsum) : 1.f;
    __syncthreads();

    // ---- phase 2: C = P^T diag(w_hat) P ----
    double mcc = 0.0;
    if (use_mcc) {
        // P and w staged through LDS 64 frames at a time; each entry still sums over t in order
        __shared__ float Pch[64 * 64], Wch[64];
        double acc[16];  // V * V <= 4096 entries over 256 threads
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0;
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int n = min(64, T - t0);
            __syncthreads();
            for (int i = threadIdx.x; i < n * 64; i += 256) Pch[i] = Ps[(long)t0 * 64 + i];
            if (threadIdx.x < n) Wch[threadIdx.x] = Ws[t0 + threadIdx.x];
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int idx = threadIdx.x + 256 * e;
                if (idx < V * V) {
                    const int a = idx / V, c = idx % V;
                    for (int tt = 0; tt < n; ++tt)
                        acc[e] += (double)Wch[tt] * (double)Pch[tt * 64 + a] * (double)Pch[tt * 64 + c];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int idx = threadIdx.x + 256 * e;
            if (idx < V * V) Cm[(idx / V) * 64 + idx % V] = acc[e];
        }
        __syncthreads();
        if (threadIdx.x < V) {  // r_j = sum_k C_jk (torch.sum(C, dim=1))
            const int j = threadIdx.x;
            double s = 0.0;
            for (int k = 0; k < V; ++k) s += Cm[j * 64 + k];
            rvec[j] = s;
        }
        __syncthreads();
        if (threadIdx.x < V) {  // rho_a = sum_i G_ia C_ia / r_a^2, G = (1 - delta)/32
            const int a = threadIdx.x;
            double s = 0.0;
            for (int i = 0; i < V; ++i)
                if (i != a) s += Cm[i * 64 + a];
            rho[a] = s / MCC_CLASS_NUM / (rvec[a] * rvec[a]);
        }
        __syncthreads();
        double part = 0.0;
        for (int idx = threadIdx.x; idx < V * V; idx += 256) {
            const int i = idx / V, j = idx % V;
            if (i != j) part += Cm[i * 64 + j] / rvec[j];
        }
        part = block_sum(part, &redd[0][0]);
        mcc = part / MCC_CLASS_NUM;
        // S = dC + dC^T, dC_ab = G_ab / r_b - rho_a
        for (int idx = threadIdx.x; idx < V * V; idx += 256) {
            const int a = idx / V, c = idx % V;
            const double dab = (a != c ? 1.0 / MCC_CLASS_NUM / rvec[c] : 0.0) - rho[a];
            const double dba = (a != c ? 1.0 / MCC_CLASS_NUM / rvec[a] : 0.0) - rho[c];
            Sm[a * 64 + c] = (float)(dab + dba);
        }
    }
    // div loss: q = softmax(mean_t logits[1:])
    double Hq = 0.0;
    __shared__ float qv[64], lqv[64];
    if (hp.div_coef > 0.f && threadIdx.x < 64) {
        const bool a2 = lane >= 1 && lane < V;
        const float c = a2 ? (float)(clsv[lane] / T) : -INFINITY;
        const float mx = wave_max(c);
        const float e = a2 ? expf(c - mx) : 0.f;
        const float s = wave_sum(e);
        const float q = e / s;
        const float lq = c - mx - logf(s);
        const float h = -wave_sum(a2 ? q * lq : 0.f);
        qv[lane] = a2 ? q : 0.f;
        lqv[lane] = a2 ? lq : 0.f;
        if (lane == 0) scal[4] = h;
    }
    __syncthreads();
    if (hp.div_coef > 0.f) Hq = scal[4];

    // ---- phase 3: gradient rows ----
    const double Kd = K;
    const float em = hp.em_coef;
    for (int t = w; t < T; t += 4) {
        const float p = act ? Ps[(long)t * 64 + lane] : 0.f;
        const float H = Hs[t];
        const float l = act ? L[(long)t * V + lane] : -INFINITY;
        // recompute mask and log p
        float bv = l;
        int bi = act ? lane : 1 << 30;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        const bool m = bi != 0;
        const float zv = l * invt;
        const float mx = wave_max(zv);
        const float e = act ? expf(zv - mx) : 0.f;
        const float lp = zv - mx - logf(wave_sum(e));
        float dz = 0.f;
        if (em > 0.f) {
            const float dH = act ? -p * (lp + H) : 0.f;
            if (hp.non_blank) {
                if (m && Kd > 0) dz += em * (float)(1.0 / Kd) * dH;
            } else {
                dz += em * (1.0f / T) * dH;
            }
        }
        if (use_mcc) {
            const float wt = Ws[t];
            // dP_j = wt * sum_a p_a S_aj
            float dp = 0.f;
            for (int a = 0; a < V; ++a) {
                const float pa = __shfl(p, a, 64);
                if (act) dp += pa * Sm[a * 64 + lane];
            }
            dp *= wt;
            const float sd = wave_sum(act ? dp * p : 0.f);
            dz += (1.0f - em) * (act ? p * (dp - sd) : 0.f);
        }
        float g = dz * invt;
        if (hp.div_coef > 0.f && act && lane >= 1) g += hp.div_coef * qv[lane] * (lqv[lane] + (float)Hq) / T;
        if (act) dL[(long)t * V + lane] = g;
    }
    if (threadIdx.x == 0 && loss_out) {
        double lv = 0.0;
        if (em > 0.f) {
            if (hp.non_blank) lv += em * (K > 0 ? scal[2] / K : NAN);
            else lv += em * scal[3] / T;
        }
        if (use_mcc) lv += (1.0 - em) * mcc;
        if (hp.div_coef > 0.f) lv += hp.div_coef * (-Hq);
        loss_out[b] = (float)lv;
    }
}

__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ logits, long rows, int V,
                                                     int* __restrict__ ids) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const float* l = logits + r * V;
    float bv = l[0];
    int bi = 0;
    for (int j = 1; j < V; ++j)
        if (l[j] > bv) {
            bv = l[j];
            bi = j;
        }
    ids[r] = bi;
}

// One wave per row (V > 64): each lane scans its classes in ascending order, then the (value, index) pairs are
// reduced with the lower index winning a tie: the first maximum, as the row-per-thread form above.
__device__ __forceinline__ int wave_argmax_row(const float* __restrict__ l, int V, int lane) {
    float bv = -INFINITY;
    int bi = 1 << 30;
    if (lane < V) {
        bv = l[lane];
        bi = lane;
    }
    for (int c = lane + 64; c < V; c += 64)
        if (l[c] > bv) {
            bv = l[c];
            bi = c;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
        }
    }
    return bi;
}

__global__ __launch_bounds__(256) void argmax_wave_kernel(const float* __restrict__ logits, long rows, int V,
                                                          int* __restrict__ ids) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const int bi = wave_argmax_row(logits + r * V, V, lane);
    if (lane == 0) ids[r] = bi;
}

// ------------------------------------------------------------------------------------------
// SUTA loss + gradient for any class count (1 <= V <= 1024): five small kernels, fp64 throughout.
//
// The MCC term never needs the V x V matrix C = P^T diag(w) P itself.  With softmax rows (sum_k p_tk = 1):
//   r_a   = sum_k C_ak = sum_t w_t p_ta                      (torch.sum(C, dim=1); C is symmetric)
//   o_a   = sum_{i != a} C_ia = sum_t w_t p_ta (1 - p_ta)    (column sum without the diagonal)
//   mcc   = sum_a (o_a / r_a) / 32                           (mcc_loss's class_num default: 32 whatever V is)
//   dmcc/dC_ab = (1 - delta_ab) / (32 r_b) - rho_a,  rho_a = o_a / (32 r_a^2)
//   dP_tj = w_t sum_a p_ta (dC_aj + dC_ja) = w_t ((1 - 2 p_tj) / (32 r_j) - rho_j) + (a term constant in j)
// and the softmax backward p_j (dP_j - sum_k p_k dP_k) drops what is constant in j.  So the loss and its gradient
// are row reductions over V and column reductions over T, O(T V) work instead of two 2 V^2 T products.
//
// scratch (doubles): rows[B*Tl][5] = {max z, log sum exp, H, w_hat, non-blank}; utt[B][8] = {K, sum(1 + e^-H),
// sum_m H, sum H, H_q}; cls[B][V][5] = {r | 1/(32 r), o | rho, sum_t logit | q, log q, -}.
// Probabilities are recomputed from (max, lse) in each pass (same expression, same bits).  Every sum has a fixed
// order: per-lane strided partials, the xor butterfly, then waves 0..3.
// ------------------------------------------------------------------------------------------
constexpr int LW_ROW = 5, LW_UTT = 8, LW_CLS = 5;

__device__ __forceinline__ double block_max_d(double v, double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    const double s = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return s;
}

// one wave per frame: softmax statistics at temperature, entropy, raw-logit argmax mask; padding frames' gradient = 0
__global__ __launch_bounds__(256) void loss_wide_rows_kernel(const float* __restrict__ logits, int Tl, int V, long rows,
                                                             double temp, float* __restrict__ dlogits,
                                                             double* __restrict__ rowd, const int* __restrict__ tlen) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)(r / Tl), t = (int)(r % Tl);
    const float* l = logits + r * V;
    if (tlen && t >= tlen[b]) {
        float* d = dlogits + r * V;
        for (int c = lane; c < V; c += 64) d[c] = 0.f;
        return;
    }
    const int bi = wave_argmax_row(l, V, lane);
    double mx = -INFINITY;
    for (int c = lane; c < V; c += 64) mx = fmax(mx, (double)l[c] / temp);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    double s = 0.0, u = 0.0;  // sum e, sum e (z - max)
    for (int c = lane; c < V; c += 64) {
        const double zc = (double)l[c] / temp - mx;
        const double e = exp(zc);
        s += e;
        u += e * zc;
    }
    s = wave_sum_d(s);
    u = wave_sum_d(u);
    if (lane == 0) {
        const double lse = log(s);
        double* o = rowd + r * LW_ROW;
        o[0] = mx;
        o[1] = lse;
        o[2] = lse - u / s;  // H = -sum p log p, log p = z - max - lse
        o[4] = bi != 0 ? 1.0 : 0.0;
    }
}

// one block per utterance: K, the reweighting normaliser, the entropy sums; then w_hat per frame
__global__ __launch_bounds__(256) void loss_wide_utt_kernel(int Tl, int reweight, double* __restrict__ rowd,
                                                            double* __restrict__ utt, const int* __restrict__ tlen) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const int T = tlen ? tlen[b] : Tl;
    double* R = rowd + (long)b * Tl * LW_ROW;
    double k = 0.0, ws = 0.0, hm = 0.0, ha = 0.0;
    for (int t = threadIdx.x; t < T; t += 256) {
        const double H = R[(long)t * LW_ROW + 2], m = R[(long)t * LW_ROW + 4];
        k += m;
        ws += 1.0 + exp(-H);
        hm += m * H;
        ha += H;
    }
    k = block_sum(k, red);
    ws = block_sum(ws, red);
    hm = block_sum(hm, red);
    ha = block_sum(ha, red);
    if (threadIdx.x == 0) {
        double* u = utt + (long)b * LW_UTT;
        u[0] = k;
        u[1] = ws;
        u[2] = hm;
        u[3] = ha;
    }
    for (int t = threadIdx.x; t < T; t += 256)
        R[(long)t * LW_ROW + 3] = reweight ? (double)T * (1.0 + exp(-R[(long)t * LW_ROW + 2])) / ws : 1.0;
}

// block (chunk of 64 classes, utterance): sums over the frames; wave w takes frames t = w (mod 4)
__global__ __launch_bounds__(256) void loss_wide_cols_kernel(const float* __restrict__ logits, int Tl, int V,
                                                             double temp, const double* __restrict__ rowd,
                                                             double* __restrict__ cls, const int* __restrict__ tlen) {
    __shared__ double part[4][3][64];
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int T = tlen ? tlen[b] : Tl;
    const float* L = logits + (long)b * Tl * V;
    const double* R = rowd + (long)b * Tl * LW_ROW;
    double r = 0.0, o = 0.0, cs = 0.0;
    if (c < V)
        for (int t = w; t < T; t += 4) {
            const double l = L[(long)t * V + c];
            const double* rt = R + (long)t * LW_ROW;
            const double p = exp(l / temp - rt[0] - rt[1]);
            const double wp = rt[3] * p;
            r += wp;
            o += wp * (1.0 - p);
            cs += l;
        }
    part[w][0][lane] = r;
    part[w][1][lane] = o;
    part[w][2][lane] = cs;
    __syncthreads();
    if (w == 0 && c < V) {
        double* out = cls + ((long)b * V + c) * LW_CLS;
#pragma unroll
        for (int j = 0; j < 3; ++j) out[j] = ((part[0][j][lane] + part[1][j][lane]) + part[2][j][lane]) + part[3][j][lane];
    }
}

// one block per utterance: the MCC value and its per-class gradient coefficients, the div-loss softmax, the loss
__global__ __launch_bounds__(256) void loss_wide_finish_kernel(int Tl, int V, LossHP hp, double* __restrict__ cls,
                                                               double* __restrict__ utt, float* __restrict__ loss_out,
                                                               const int* __restrict__ tlen) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const int T = tlen ? tlen[b] : Tl;
    double* C = cls + (long)b * V * LW_CLS;
    double* u = utt + (long)b * LW_UTT;
    const double em = hp.em_coef, g = 1.0 / MCC_CLASS_NUM;
    const bool use_mcc = 1.0f - hp.em_coef > 0.f;
    double mcc = 0.0;
    if (use_mcc) {
        for (int c = threadIdx.x; c < V; c += 256) {
            const double r = C[c * LW_CLS + 0], o = C[c * LW_CLS + 1];
            mcc += o / r;
            C[c * LW_CLS + 0] = g / r;
            C[c * LW_CLS + 1] = g * o / (r * r);
        }
        mcc = block_sum(mcc, red) * g;
    }
    double Hq = 0.0;
    if (hp.div_coef > 0.f) {  // q = softmax(mean_t logits[1:])
        double mx = -INFINITY;
        for (int c = 1 + threadIdx.x; c < V; c += 256) mx = fmax(mx, C[c * LW_CLS + 2] / T);
        mx = block_max_d(mx, red);
        double s = 0.0;
        for (int c = 1 + threadIdx.x; c < V; c += 256) s += exp(C[c * LW_CLS + 2] / T - mx);
        s = block_sum(s, red);
        const double lse = log(s);
        double h = 0.0;
        for (int c = 1 + threadIdx.x; c < V; c += 256) {
            const double lq = C[c * LW_CLS + 2] / T - mx - lse;
            const double q = exp(lq);
            C[c * LW_CLS + 2] = q;
            C[c * LW_CLS + 3] = lq;
            h -= q * lq;
        }
        Hq = block_sum(h, red);
    }
    if (threadIdx.x == 0) {
        u[4] = Hq;
        if (loss_out) {
            double lv = 0.0;
            if (hp.em_coef > 0.f) {
                if (hp.non_blank) lv += em * (u[0] > 0 ? u[2] / u[0] : (double)NAN);
                else lv += em * u[3] / T;
            }
            if (use_mcc) lv += (1.0 - em) * mcc;
            if (hp.div_coef > 0.f) lv += (double)hp.div_coef * (-Hq);
            loss_out[b] = (float)lv;
        }
    }
}

// one wave per frame: dL/dlogits
__global__ __launch_bounds__(256) void loss_wide_grad_kernel(const float* __restrict__ logits, int Tl, int V, long rows,
                                                             LossHP hp, const double* __restrict__ rowd,
                                                             const double* __restrict__ utt,
                                                             const double* __restrict__ cls, float* __restrict__ dlogits,
                                                             const int* __restrict__ tlen) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)(r / Tl), t = (int)(r % Tl);
    const int T = tlen ? tlen[b] : Tl;
    if (t >= T) return;  // zeroed by the rows kernel
    const float* l = logits + r * V;
    float* d = dlogits + r * V;
    const double* rt = rowd + r * LW_ROW;
    const double* u = utt + (long)b * LW_UTT;
    const double* C = cls + (long)b * V * LW_CLS;
    const double temp = hp.temp, em = hp.em_coef;
    const double mx = rt[0], lse = rt[1], H = rt[2], wt = rt[3];
    const bool m = rt[4] != 0.0;
    const bool use_mcc = 1.0f - hp.em_coef > 0.f;
    double ce = 0.0;  // coefficient of dH_j = -p_j (log p_j + H)
    if (hp.em_coef > 0.f) {
        if (hp.non_blank) ce = (m && u[0] > 0) ? em / u[0] : 0.0;
        else ce = em / T;
    }
    double sd = 0.0;  // sum_k p_k dP_k
    if (use_mcc) {
        for (int c = lane; c < V; c += 64) {
            const double p = exp((double)l[c] / temp - mx - lse);
            sd += p * (wt * (C[c * LW_CLS + 0] * (1.0 - 2.0 * p) - C[c * LW_CLS + 1]));
        }
        sd = wave_sum_d(sd);
    }
    const double dq = hp.div_coef > 0.f ? (double)hp.div_coef / T : 0.0, Hq = u[4];
    for (int c = lane; c < V; c += 64) {
        const double lp = (double)l[c] / temp - mx - lse;
        const double p = exp(lp);
        double dz = -ce * p * (lp + H);
        if (use_mcc) dz += (1.0 - em) * p * (wt * (C[c * LW_CLS + 0] * (1.0 - 2.0 * p) - C[c * LW_CLS + 1]) - sd);
        double gr = dz / temp;
        if (dq > 0.0 && c >= 1) gr += dq * C[c * LW_CLS + 2] * (C[c * LW_CLS + 3] + Hq);
        d[c] = (float)gr;
    }
}

// ------------------------------------------------------------------------------------------
// AdamW (torch single-tensor path, decoupled wd) with k sub-steps per element
// ------------------------------------------------------------------------------------------
// One block = ADAM_GPT x 256 consecutive 16-B groups of ONE run (block -> run from the host's
// cumulative block table, a uniform scalar search), so the multiplicity K is a template constant and
// the K sub-steps unroll with their step sizes in scalar registers.  Every load of a thread is issued
// before its first update.  Run starts are 4-float aligned; elements past a run's end inside its last
// group are loaded and stored back unchanged.  At device step 0 the moments are zero by definition
// (every reset sets the step counter to 0), so they are not read: the episodic reset needs no memset.
constexpr int ADAM_GPT = 2;

template <int K>
__device__ __forceinline__ void adam_body(float* __restrict__ P, const float* __restrict__ G, float* __restrict__ M,
                                          float* __restrict__ Vv, long base, long g0, long ngroups, long len,
                                          const AdamArgs& a, const float* __restrict__ tab, bool first) {
    float ss[K], bs[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        ss[j] = tab ? tab[(K - 1) * 5 + j] : a.step_size[K - 1][j];
        bs[j] = tab ? tab[25 + (K - 1) * 5 + j] : a.bc2_sqrt[K - 1][j];
    }
    // AdamW's decoupled decay p *= 1 - lr_i wd (adam.py: param.mul_(1 - lr * weight_decay)), the factor rounded from
    // double with the step's scheduled lr; off (the reference's wd 0) when lr_wd == 0
    const float wdf = tab ? tab[50] : 1.0f - a.lr_wd;
    f32x4 g4[ADAM_GPT], p4[ADAM_GPT], m4[ADAM_GPT], v4[ADAM_GPT];
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < ADAM_GPT; ++u) {
        const long gi = g0 + u * 256;
        m4[u] = v4[u] = g4[u] = p4[u] = z;
        if (gi < ngroups) {
            const long idx = base + 4 * gi;
            g4[u] = *reinterpret_cast<const f32x4*>(G + idx);
            p4[u] = *reinterpret_cast<const f32x4*>(P + idx);
            if (!first) {
                m4[u] = *reinterpret_cast<const f32x4*>(M + idx);
                v4[u] = *reinterpret_cast<const f32x4*>(Vv + idx);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < ADAM_GPT; ++u) {
        const long gi = g0 + u * 256;
        if (gi >= ngroups) continue;
        const int nv = (int)min(4L, len - 4 * gi);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= nv) break;
            const float g = g4[u][e];
            float p = p4[u][e], m = m4[u][e], v = v4[u][e];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (a.lr_wd != 0.f) p *= wdf;
                m = m + a.omb1 * (g - m);                 // lerp_(g, 1-beta1), weight < 0.5 form
                v = v * a.beta2 + a.omb2 * (g * g);        // mul_(beta2).addcmul_(g, g, 1-beta2)
                const float denom = sqrtf(v) / bs[j] + a.eps;
                p = p + (-ss[j]) * (m / denom);           // addcdiv_(m, denom, -step_size)
            }
            p4[u][e] = p;
            m4[u][e] = m;
            v4[u][e] = v;
        }
        const long idx = base + 4 * gi;
        *reinterpret_cast<f32x4*>(P + idx) = p4[u];
        *reinterpret_cast<f32x4*>(M + idx) = m4[u];
        *reinterpret_cast<f32x4*>(Vv + idx) = v4[u];
    }
}

// torch.optim.SGD, single-tensor path at momentum 0 and weight decay 0 (sgd.py _single_tensor_sgd: param.add_(grad,
// alpha=-lr), once per collect_params entry): K fused multiply-adds p = g (-lr_i) + p (ATen's CPU add kernel is
// vec::fmadd(b, alpha, a)); no moments are read or written
template <int K>
__device__ __forceinline__ void sgd_body(float* __restrict__ P, const float* __restrict__ G, long base, long g0,
                                         long ngroups, long len, float nlr) {
    f32x4 g4[ADAM_GPT], p4[ADAM_GPT];
#pragma unroll
    for (int u = 0; u < ADAM_GPT; ++u) {
        const long gi = g0 + u * 256;
        if (gi < ngroups) {
            g4[u] = *reinterpret_cast<const f32x4*>(G + base + 4 * gi);
            p4[u] = *reinterpret_cast<const f32x4*>(P + base + 4 * gi);
        }
    }
#pragma unroll
    for (int u = 0; u < ADAM_GPT; ++u) {
        const long gi = g0 + u * 256;
        if (gi >= ngroups) continue;
        const int nv = (int)min(4L, len - 4 * gi);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= nv) break;
            float p = p4[u][e];
#pragma unroll
            for (int j = 0; j < K; ++j) p = fmaf(g4[u][e], nlr, p);
            p4[u][e] = p;
        }
        *reinterpret_cast<f32x4*>(P + base + 4 * gi) = p4[u];
    }
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ P, const float* __restrict__ G,
                                                   float* __restrict__ M, float* __restrict__ Vv, long pstride,
                                                   AdamArgs a) {
    const int bx = blockIdx.x;
    // this block's run: an unrolled uniform select (constant indices keep the kernel arguments in scalar
    // registers; a dynamic index would copy the argument block to scratch per thread)
    long start = 0, len = 0;
    int k = 1, blk = 0;
#pragma unroll
    for (int r = 0; r < SUTA_MAX_RUNS; ++r)
        if (r < a.nruns && bx >= a.blk0[r]) {
            start = a.runs[r].start;
            len = a.runs[r].len;
            k = a.runs[r].k;
            blk = a.blk0[r];
        }
    const long ngroups = (len + 3) / 4;
    const long g0 = (long)(bx - blk) * (256 * ADAM_GPT) + threadIdx.x;
    const long base = (long)blockIdx.y * pstride + start;
    const int step = a.step ? *a.step : 1;
    const float* tab = a.tab ? a.tab + (long)step * ADAM_TAB : nullptr;
    const bool first = a.step && step == 0;
    if (a.sgd) {
        const float nlr = tab ? tab[51] : -a.step_size[0][0];
        switch (k) {
            case 1: sgd_body<1>(P, G, base, g0, ngroups, len, nlr); break;
            case 2: sgd_body<2>(P, G, base, g0, ngroups, len, nlr); break;
            case 3: sgd_body<3>(P, G, base, g0, ngroups, len, nlr); break;
            case 4: sgd_body<4>(P, G, base, g0, ngroups, len, nlr); break;
            default: sgd_body<5>(P, G, base, g0, ngroups, len, nlr); break;
        }
        return;
    }
    switch (k) {
        case 1: adam_body<1>(P, G, M, Vv, base, g0, ngroups, len, a, tab, first); break;
        case 2: adam_body<2>(P, G, M, Vv, base, g0, ngroups, len, a, tab, first); break;
        case 3: adam_body<3>(P, G, M, Vv, base, g0, ngroups, len, a, tab, first); break;
        case 4: adam_body<4>(P, G, M, Vv, base, g0, ngroups, len, a, tab, first); break;
        default: adam_body<5>(P, G, M, Vv, base, g0, ngroups, len, a, tab, first); break;
    }
}

}  // namespace

// ==========================================================================================
// launchers
// ==========================================================================================
void launch_wave_normalize(const float* x, float* y, int B, long N, const int* lens, hipStream_t st) {
    hipLaunchKernelGGL(wave_normalize_kernel, dim3(B), dim3(256), 0, st, x, y, N, lens);
}

void launch_conv0(const float* x, long N, const float* W, const float* bias, long wstride, float* z, int B, int L0,
                  int C, int K, int S, hipStream_t st, void* zb) {
    auto a16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const bool vec = K == 10 && S == 5 && C % 4 == 0 && C / 4 <= 256 && 256 % (C / 4) == 0 && wstride % 4 == 0 &&
                     a16(W) && (zb ? (reinterpret_cast<uintptr_t>(zb) & 7) == 0 : a16(z)) && (!bias || a16(bias));
    if (zb && !vec) throw std::invalid_argument("conv0: bf16 output needs the vectorised kernel (K 10, S 5)");
    if (vec) {  // every wav2vec2 conv0
        hipLaunchKernelGGL((conv0_vec_kernel<10, 5>), dim3(cdiv(L0, C0V_ROWS), B), dim3(256), 0, st, x, N, W, bias,
                           wstride, z, L0, C, reinterpret_cast<__bf16*>(zb));
        return;
    }
    hipLaunchKernelGGL(conv0_kernel, dim3(cdiv(L0, C0_ROWS), B), dim3(256), 0, st, x, N, W, bias, wstride, z, L0, C,
                       K, S);
}

static int ew_grid(long n) { return (int)std::min<long>(2048, std::max<long>(1, (n + 255) / 256)); }

void launch_softmax_rows(float* s, long nrows, int T, long ld, const int* tlen, long rows_per_utt, hipStream_t st) {
    dim3 grid((unsigned)((nrows + 3) / 4));
    if (T <= 256) hipLaunchKernelGGL(softmax_rows_kernel<4>, grid, dim3(256), 0, st, s, nrows, T, ld, tlen,
                                    rows_per_utt);
    else if (T <= 512) hipLaunchKernelGGL(softmax_rows_kernel<8>, grid, dim3(256), 0, st, s, nrows, T, ld, tlen,
                                    rows_per_utt);
    else if (T <= 1024) hipLaunchKernelGGL(softmax_rows_kernel<16>, grid, dim3(256), 0, st, s, nrows, T, ld, tlen,
                                    rows_per_utt);
    else hipLaunchKernelGGL(softmax_rows_kernel<32>, grid, dim3(256), 0, st, s, nrows, T, ld, tlen,
                                    rows_per_utt);
}

constexpr int PC_CHT = 2;  // taps per weight chunk: two chunks + the base window fit 2 blocks per CU
#define HIPCHK_OPS(x)                                                                        \
    do {                                                                                     \
        if ((x) != hipSuccess) throw std::runtime_error("hipFuncSetAttribute(posconv) failed"); \
    } while (0)

template <int CG, bool FWD, bool STK>
static void posconv_go(int WB, dim3 grid, size_t lds, hipStream_t st, const float* x, const float* W,
                       const float* bias, const float* R, float* C, float* C2, int T, int H, int G, int K, int pad,
                       const int* tlen, int ntile, int B) {
    // > 64 KiB of dynamic LDS must be allowed per kernel (once per instantiation)
#define PC(WB_)                                                                                                   \
    do {                                                                                                          \
        set_max_lds_once(reinterpret_cast<const void*>(&posconv_kernel<CG, WB_, PC_CHT, FWD, STK>), 160 * 1024,  \
                         "posconv_kernel");                                                                       \
        hipLaunchKernelGGL((posconv_kernel<CG, WB_, PC_CHT, FWD, STK>), grid, dim3(WB_ * 64), lds, st, x, W, bias, \
                           R, C, C2, T, H, G, K, pad, tlen, ntile, B);                                            \
    } while (0)
    switch (WB) {
        case 4: PC(4); break;
        case 5: PC(5); break;
        case 6: PC(6); break;
        case 7: PC(7); break;
        default: PC(8); break;
    }
#undef PC
}

template <bool STK>
static bool posconv_launch(bool fwd, const float* x, const float* W, const float* bias, const float* R, float* C,
                           float* C2, int B, int T, int H, int G, int K, int pad, const int* tlen, hipStream_t st) {
    const int CG = H / G;
    if ((CG != 48 && CG != 64) || K % PC_CHT || H % 4) return false;
    // waves per block: fewest padded frames over ceil(T / (16 WB)) tiles (T = 399 -> 5 waves, 400 rows)
    int WB = 8;
    long best = 1L << 40;
    for (int wb = 8; wb >= 4; --wb) {
        const long tiles = (T + 16 * wb - 1) / (16 * wb);
        const long waste = tiles * 16 * wb - T;
        if (waste < best) {
            best = waste;
            WB = wb;
        }
    }
    const int ntile = (T + 16 * WB - 1) / (16 * WB);
    const int XS = CG + 4, WS = (CG % 64 == 0) ? CG + 16 : CG;
    const size_t lds = ((size_t)(16 * WB + K - 1) * XS + 2 * PC_CHT * CG * WS) * sizeof(float);
    if (lds > 160 * 1024) return false;
    const dim3 grid((unsigned)((long)G * B * ntile));
    if (CG == 48) {
        if (fwd) posconv_go<48, true, STK>(WB, grid, lds, st, x, W, bias, R, C, C2, T, H, G, K, pad, tlen, ntile, B);
        else posconv_go<48, false, STK>(WB, grid, lds, st, x, W, bias, R, C, C2, T, H, G, K, pad, tlen, ntile, B);
    } else {
        if (fwd) posconv_go<64, true, STK>(WB, grid, lds, st, x, W, bias, R, C, C2, T, H, G, K, pad, tlen, ntile, B);
        else posconv_go<64, false, STK>(WB, grid, lds, st, x, W, bias, R, C, C2, T, H, G, K, pad, tlen, ntile, B);
    }
    return true;
}

bool launch_posconv(bool fwd, const float* x, const float* W, const float* bias, const float* R, float* C, float* C2,
                    int B, int T, int H, int G, int K, int pad, const int* tlen, hipStream_t st) {
    return posconv_launch<false>(fwd, x, W, bias, R, C, C2, B, T, H, G, K, pad, tlen, st);
}

int posconv_stack_taps(int K) { return (K + PC_CHT - 1) / PC_CHT * PC_CHT; }

bool launch_posconv_stack(bool fwd, const float* x, const float* W, const float* bias, const float* R, float* C, int B,
                          int T, int H, int G, int K, const int* tlen, hipStream_t st) {
    if (K < 1 || (fwd && !bias)) return false;
    // forward taps reach K / 2 frames back (HF pads K / 2 and drops the last frame of an even K), the flipped taps
    // of the backward K - 1 - K / 2; the appended zero taps lie past the last real one in both
    return posconv_launch<true>(fwd, x, W, bias, R, C, nullptr, B, T, H, G, posconv_stack_taps(K),
                                fwd ? K / 2 : K - 1 - K / 2, tlen, st);
}

template <bool FWD>
static void posconv_bf16_go(int WB, dim3 grid, size_t lds, hipStream_t st, const float* x, const __bf16* W,
                            const float* bias, const float* R, float* C, float* C2, int T, int H, int G, int K, int pad,
                            const int* tlen, int ntile, int B) {
#define PCB(WB_)                                                                                                  \
    do {                                                                                                          \
        set_max_lds_once(reinterpret_cast<const void*>(&posconv_bf16_kernel<WB_, FWD>), 160 * 1024,              \
                         "posconv_bf16_kernel");                                                                  \
        hipLaunchKernelGGL((posconv_bf16_kernel<WB_, FWD>), grid, dim3(WB_ * 64), lds, st, x, W, bias, R, C, C2, T, \
                           H, G, K, pad, tlen, ntile, B);                                                         \
    } while (0)
    switch (WB) {
        case 4: PCB(4); break;
        case 5: PCB(5); break;
        case 6: PCB(6); break;
        case 7: PCB(7); break;
        default: PCB(8); break;
    }
#undef PCB
}

bool launch_posconv_bf16(bool fwd, const float* x, const void* Wt, const float* bias, const float* R, float* C,
                         float* C2, int B, int T, int H, int G, int K, int pad, const int* tlen, hipStream_t st) {
    if (H / G != 64 || H % G || K % PCB_CHT || !Wt) return false;
    int WB = 8;  // waves per block: fewest padded frames over ceil(T / (32 WB)) tiles (T = 399 -> 7 waves)
    long best = 1L << 40;
    for (int wb = 8; wb >= 4; --wb) {
        const long tiles = (T + 32 * wb - 1) / (32 * wb);
        const long waste = tiles * 32 * wb - T;
        if (waste < best) {
            best = waste;
            WB = wb;
        }
    }
    const int ntile = (T + 32 * WB - 1) / (32 * WB);
    const size_t lds = ((size_t)(32 * WB + K - 1) * PCB_RS + 2 * PCB_CHT * 64 * PCB_RS) * sizeof(__bf16);
    if (lds > 160 * 1024) return false;
    const dim3 grid((unsigned)((long)G * B * ntile));
    const __bf16* W = reinterpret_cast<const __bf16*>(Wt);
    if (fwd) posconv_bf16_go<true>(WB, grid, lds, st, x, W, bias, R, C, C2, T, H, G, K, pad, tlen, ntile, B);
    else posconv_bf16_go<false>(WB, grid, lds, st, x, W, bias, R, C, C2, T, H, G, K, pad, tlen, ntile, B);
    return true;
}

void launch_dgelu_mul(const float* g, const float* z, float* out, long n, hipStream_t st) {
    hipLaunchKernelGGL(dgelu_mul_kernel, dim3(ew_grid(n)), dim3(256), 0, st, g, z, out, n);
}

void launch_suta_loss(const float* logits, int B, int T, int V, LossHP hp, const int* tlen, float* dlogits, float* loss,
                      float* scratch, hipStream_t st) {
    if (V < 1 || V > SUTA_MAX_VOCAB) throw std::runtime_error("suta loss: vocab_size outside [1, 1024]");
    if (V <= 64 && !suta_switches().loss_wide) {
        hipLaunchKernelGGL(suta_loss_kernel, dim3(B), dim3(256), 0, st, logits, T, V, hp, dlogits, loss, scratch, tlen);
        return;
    }
    // any V: rows -> utterance sums -> class sums -> utterance finish -> gradient rows (the layout above)
    double* rowd = reinterpret_cast<double*>(scratch);
    double* utt = rowd + (size_t)B * T * LW_ROW;
    double* cls = utt + (size_t)B * LW_UTT;
    const long rows = (long)B * T;
    const dim3 rgrid((unsigned)((rows + 3) / 4));
    const double temp = hp.temp;
    hipLaunchKernelGGL(loss_wide_rows_kernel, rgrid, dim3(256), 0, st, logits, T, V, rows, temp, dlogits, rowd, tlen);
    hipLaunchKernelGGL(loss_wide_utt_kernel, dim3(B), dim3(256), 0, st, T, hp.reweight, rowd, utt, tlen);
    hipLaunchKernelGGL(loss_wide_cols_kernel, dim3((V + 63) / 64, B), dim3(256), 0, st, logits, T, V, temp, rowd, cls,
                       tlen);
    hipLaunchKernelGGL(loss_wide_finish_kernel, dim3(B), dim3(256), 0, st, T, V, hp, cls, utt, loss, tlen);
    hipLaunchKernelGGL(loss_wide_grad_kernel, rgrid, dim3(256), 0, st, logits, T, V, rows, hp, rowd, utt, cls, dlogits,
                       tlen);
}

size_t suta_loss_scratch_floats(int B, long T, int V) {
    const size_t narrow = (size_t)B * T * 66 + 64;  // suta_loss_kernel: P[T][64], H[T], w[T] per utterance
    const size_t wide = 2 * ((size_t)B * T * LW_ROW + (size_t)B * LW_UTT + (size_t)B * V * LW_CLS) + 64;  // doubles
    return std::max(narrow, wide);
}

void launch_argmax(const float* logits, long rows, int V, int* ids, hipStream_t st) {
    if (V > 64)
        hipLaunchKernelGGL(argmax_wave_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, logits, rows, V, ids);
    else
        hipLaunchKernelGGL(argmax_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, logits, rows, V, ids);
}

__global__ __launch_bounds__(256) void broadcast_kernel(f32x4* __restrict__ dst, const f32x4* __restrict__ src,
                                                        long n4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) dst[(long)blockIdx.y * n4 + i] = src[i];
}

void launch_broadcast(float* dst, const float* src, long n, int B, hipStream_t st) {
    if (n % 4) throw std::runtime_error("broadcast length not a multiple of 4");
    const long n4 = n / 4;
    hipLaunchKernelGGL(broadcast_kernel, dim3((unsigned)((n4 + 255) / 256), B), dim3(256), 0, st,
                       reinterpret_cast<f32x4*>(dst), reinterpret_cast<const f32x4*>(src), n4);
}

__global__ void step_advance_kernel(int* step) { *step += 1; }

void launch_step_advance(int* step, hipStream_t st) {
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, st, step);
}

void launch_adam(float* P, const float* G, float* M, float* V, long pstride, int B, const AdamArgs& a,
                 hipStream_t st) {
    AdamArgs aa = a;
    long nblk = 0;
    for (int r = 0; r < a.nruns; ++r) {
        if (a.runs[r].start % 4) throw std::runtime_error("adam run start not 16-B aligned");
        if (a.runs[r].k < 1 || a.runs[r].k > 5) throw std::runtime_error("adam multiplicity outside [1, 5]");
        aa.blk0[r] = (int)nblk;
        nblk += ((a.runs[r].len + 3) / 4 + 256 * ADAM_GPT - 1) / (256 * ADAM_GPT);
    }
    if (nblk == 0) return;
    if (pstride % 4) throw std::runtime_error("adam slot stride not a multiple of 4");
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)nblk, B), dim3(256), 0, st, P, G, M, V, pstride, aa);
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel.  Several engines' host threads launch concurrently
// (--gpu_engines), so the "done" set is guarded (advisor r5: the former per-call-site static flags were data races).
void set_max_lds_once(const void* fn, size_t bytes, const char* name) {
    static std::mutex mu;
    static std::map<const void*, size_t> done;
    std::lock_guard<std::mutex> lk(mu);
    auto it = done.find(fn);
    if (it != done.end() && it->second >= bytes) return;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
        throw std::runtime_error(std::string("hipFuncSetAttribute(") + name + ") failed");
    done[fn] = bytes;
}

static thread_local SutaSwitches g_switches{};  // per host thread (common.h)

void suta_latch_switches() {
    auto on = [](const char* name) {  // default on; "0" selects the replaced path
        const char* ev = std::getenv(name);
        return (ev && atoi(ev) == 0) ? 0 : 1;
    };
    SutaSwitches s{};
    s.fast_gelu = on("SUTA_FAST_GELU");
    s.flash_fwd_plane = on("SUTA_FLASH_FWD_PLANE");
    s.flash_bwd_plane = on("SUTA_FLASH_BWD_PLANE");
    s.flash_bf16_img = on("SUTA_FLASH_BF16_IMG");
    s.conv_planes = on("SUTA_CONV_PLANES");
    s.pre_bf16 = on("SUTA_PRE_BF16");
    s.conv_z_bf16 = on("SUTA_CONV_Z_BF16");
    s.dy_planes = on("SUTA_DY_PLANES");
    s.conv_dx_planes = on("SUTA_CONV_DX_PLANES");
    s.fused_conv_ln = on("SUTA_FUSED_CONV_LN");
    const char* hbx = std::getenv("SUTA_HBX");
    s.hbx = hbx ? atoi(hbx) : 1;
    s.splitk = on("SUTA_SPLITK");
    const char* hbxt = std::getenv("SUTA_HBX_T");
    s.hbx_t = hbxt ? std::min(2, std::max(0, atoi(hbxt))) : 2;
    s.fused_delta = on("SUTA_FUSED_DELTA");
    const char* lrpw = std::getenv("SUTA_LN_RPW");
    s.ln_rpw = lrpw ? atoi(lrpw) : 2;
    const char* hform = std::getenv("SUTA_HBX_FORM");
    s.hbx_form = hform ? atoi(hform) : 4;
    const char* ht4 = std::getenv("SUTA_HBT4");
    s.hbt4 = ht4 ? atoi(ht4) : 1;
    const char* hdbg = std::getenv("SUTA_HBX_DBG");
    s.hbx_dbg = hdbg ? atoi(hdbg) : 0;
    const char* fnw = std::getenv("SUTA_FLASH_FWD_NW");
    s.flash_fwd_nw = (fnw && atoi(fnw) == 8) ? 8 : 4;
    s.epi_fast = on("SUTA_EPI_FAST");
    s.hbp_conv = on("SUTA_HBP_CONV");
    const char* lw = std::getenv("SUTA_LOSS_WIDE");
    s.loss_wide = (lw && atoi(lw) != 0) ? 1 : 0;
    const char* f32p = std::getenv("SUTA_F32P");
    s.f32p = f32p ? std::min(2, std::max(0, atoi(f32p))) : 1;
    const char* sw = std::getenv("SUTA_SDPL_WIDE");
    s.sdpl_wide = (sw && atoi(sw) != 0) ? 1 : 0;
    s.latched = 1;
    g_switches = s;
}

const SutaSwitches& suta_switches() {
    if (!g_switches.latched) suta_latch_switches();
    return g_switches;
}

// SUTA_FAST_GELU=0: the erff GELU / GELU' everywhere (A/B runs); default: the branch-free form (common.h gelu_fast,
// erfc fractional error < 1.2e-7: fp32-accurate) in the conv front-end and every GEMM epilogue
static bool fast_gelu_on() { return suta_switches().fast_gelu != 0; }
template <int MODE, typename... Args>
static void launch_conv0_gn(dim3 grid, hipStream_t st, int K, int S, Args... args) {
    if (K == 10 && S == 5 && fast_gelu_on())
        hipLaunchKernelGGL((conv0_gn_kernel<MODE, 10, 5, true>), grid, dim3(256), 0, st, args...);
    else if (K == 10 && S == 5)
        hipLaunchKernelGGL((conv0_gn_kernel<MODE, 10, 5>), grid, dim3(256), 0, st, args...);
    else
        hipLaunchKernelGGL((conv0_gn_kernel<MODE, 0, 0>), grid, dim3(256), 0, st, args...);
}

void launch_front_gn_fwd(const float* x, long N, const float* W, const float* bias, long wstride, int B, int L0, int C,
                         int K, int S, const float* g, const float* beta, float* mean, float* rstd, float* a,
                         double* dpart, const int* L0s, hipStream_t st) {
    const int nchunk = cdiv(L0, F0_ROWS);
    launch_conv0_gn<0>(dim3(nchunk, B), st, K, S, x, N, W, bias, wstride, L0, C, K, S,
                       (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                       (float*)nullptr, (const float*)nullptr, dpart, (float*)nullptr, nchunk, L0s);
    hipLaunchKernelGGL(col_stats_final, dim3(cdiv(C, 256), B), dim3(256), 0, st, dpart, nchunk, L0, C, 1e-5f, mean,
                       rstd, L0s);
    launch_conv0_gn<1>(dim3(nchunk, B), st, K, S, x, N, W, bias, wstride, L0, C, K, S,
                       mean, rstd, g, beta, a, (const float*)nullptr, (double*)nullptr, (float*)nullptr, nchunk, L0s);
}

void launch_front_gn_bwd(const float* x, long N, const float* W, const float* bias, long wstride, int B, int L0, int C,
                         int K, int S, const float* g, const float* beta, const float* mean, const float* rstd,
                         float* da, float* dgamma, float* dbeta, float* dW, long gstride, double* dpart, float* fpart,
                         const int* L0s, hipStream_t st) {
    const int nchunk = cdiv(L0, F0_ROWS);
    launch_conv0_gn<2>(dim3(nchunk, B), st, K, S, x, N, W, bias, wstride, L0, C, K, S,
                       mean, rstd, g, beta, da, (const float*)nullptr, dpart, (float*)nullptr, nchunk, L0s);
    float* coef = reinterpret_cast<float*>(dpart + (long)B * nchunk * 2 * C);
    hipLaunchKernelGGL(gn_bwd_final, dim3(cdiv(C, 256), B), dim3(256), 0, st, dpart, nchunk, C, dgamma, dbeta, gstride,
                       coef);
    launch_conv0_gn<3>(dim3(nchunk, B), st, K, S, x, N, W, bias, wstride, L0, C, K, S,
                       mean, rstd, g, beta, da, coef, (double*)nullptr, fpart, nchunk, L0s);
    hipLaunchKernelGGL(conv0_dw_reduce, dim3(cdiv((long)K * C, 256), B), dim3(256), 0, st, fpart, nchunk, K * C, dW,
                       gstride);
}

void launch_attn_delta(const float* dO, const float* O, float* delta, int B, int T, int NH, int dh, hipStream_t st) {
    const long items = (long)B * T * NH;
    const long vec = items * (dh / 4);
    const dim3 grid((unsigned)((vec + 255) / 256));
    const f32x4* a = reinterpret_cast<const f32x4*>(dO);
    const f32x4* c = reinterpret_cast<const f32x4*>(O);
    switch (dh) {
        case 16: hipLaunchKernelGGL(attn_delta_kernel<4>, grid, dim3(256), 0, st, a, c, delta, items, T, NH); return;
        case 32: hipLaunchKernelGGL(attn_delta_kernel<8>, grid, dim3(256), 0, st, a, c, delta, items, T, NH); return;
        case 64: hipLaunchKernelGGL(attn_delta_kernel<16>, grid, dim3(256), 0, st, a, c, delta, items, T, NH); return;
        case 128: hipLaunchKernelGGL(attn_delta_kernel<32>, grid, dim3(256), 0, st, a, c, delta, items, T, NH); return;
        default:
            if (dh % 4 == 0 && dh <= 128 && (reinterpret_cast<uintptr_t>(dO) & 15) == 0 &&
                (reinterpret_cast<uintptr_t>(O) & 15) == 0) {
                hipLaunchKernelGGL(attn_delta_pad32_kernel, dim3((unsigned)((items * 32 + 255) / 256)), dim3(256), 0, st,
                                   a, c, delta, items, T, NH, dh / 4);
                return;
            }
            hipLaunchKernelGGL(attn_delta_scalar, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, dO, O, delta,
                               items, T, NH, dh);
    }
}
