// MMS attention adapter (HF Wav2Vec2AttnAdapterLayer, modeling_wav2vec2.py: the stable-LN encoder layer's
//   h = h + linear_2(relu(linear_1(norm(h)))),  norm = nn.LayerNorm(H), linear_1 [A][H], linear_2 [H][A], A = 16)
// as one forward and one backward kernel per layer.  norm's gamma / beta are per-slot trainables, the two linears
// are frozen and shared.  Exact fp32 in every precision mode (suta.h): the two skinny products run on
// v_mfma_f32_16x16x4_f32, whose N = 16 is the adapter width.
//
// Tiling: a block of NW waves (4 up to H = 1024, 8 above) owns 16 rows of one utterance.  Lane l of wave w stands for
// row r = l & 15 and quarter q = l >> 4; of the row's 16-column chunks j the wave owns j = w, w + NW, ..., and the
// lane holds columns 16 j + 4 q .. + 3 of each as one 16-B register group: the row tile is read from HBM once and
// stays in registers for the statistics, the products and the residual.  Both products are taken transposed (the
// weight is the MFMA's A operand, the data its B operand), so a result lands in the lane that holds the same row:
// D[m][n = r] in lane (r, q) is m = 4 q + i.  The MFMA's four k of a step are fed as k = 4 q + i of the chunk, the
// same for both operands, so every operand is one 16-B load.  linear_1's product is split over the waves along K = H
// and summed through LDS in wave order; the weights are read from L2 per row tile (W1 + W2 are 160 KB at H = 1280:
// not LDS-resident in fp32), zero-padded at creation to [NA][Hp] / [Hp][NA] (NA = 16 for A <= 16, else 64; Hp = H
// rounded up to 16) so that padded columns contribute exactly zero, through relu' too (their pre-activation is 0, and
// relu'(0) = 0 as in torch).
#include <stdexcept>

#include "common.h"
#include "ops.h"

namespace {

constexpr int AD_ROWS = 16;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// acc += Wrow[k] * v[k] over the lane group's four k: two accumulator chains (a dependent 16x16x4 issues every 40
// cycles, an independent one every 32)
__device__ __forceinline__ void mfma_k4(f32x4 wv, f32x4 v, f32x4& a0, f32x4& a1) {
    a0 = mfma4(wv.x, v.x, a0);
    a1 = mfma4(wv.y, v.y, a1);
    a0 = mfma4(wv.z, v.z, a0);
    a1 = mfma4(wv.w, v.w, a1);
}

// sum over the 16 lanes that share l >> 4 (one DPP row), the same value in every lane
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_f<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    v += dpp_f<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    v += dpp_f<0x141>(v);  // row_half_mirror
    v += dpp_f<0x140>(v);  // row_mirror
    return v;
}

__device__ __forceinline__ float hsum(f32x4 v) { return (v.x + v.y) + (v.z + v.w); }

// sum of one value per row over the row's lanes: the 4 quarters of a wave, then the NW waves in wave order
template <int NW>
__device__ __forceinline__ float row_sum(float s, float (*red)[AD_ROWS], int w, int r, int q) {
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    __syncthreads();  // (the previous use of red is read)
    if (q == 0) red[w][r] = s;
    __syncthreads();
    float t = red[0][r];
#pragma unroll
    for (int v = 1; v < NW; ++v) t += red[v][r];
    return t;
}
// a per-lane 16-B value summed over the NW waves in wave order through LDS (every wave gets the sum)
template <int NW, int NT>
__device__ __forceinline__ void wave_reduce(f32x4 (*part)[NT][64], const f32x4* a0, const f32x4* a1, f32x4* out, int w,
                                            int lane) {
    __syncthreads();  // (the previous use of part is read)
#pragma unroll
    for (int t = 0; t < NT; ++t) part[w][t][lane] = a0[t] + a1[t];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        f32x4 s = part[0][t][lane];
#pragma unroll
        for (int v = 1; v < NW; ++v) s += part[v][t][lane];
        out[t] = s;
    }
}

template <int NJ, int NW, int NT>
__global__ __launch_bounds__(NW * 64) void adapter_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                              const float* __restrict__ beta, long pstride, int T,
                                                              int H, AdapterW wt, float eps, float* __restrict__ out,
                                                              float* __restrict__ meanp, float* __restrict__ rstdp) {
    __shared__ float red[NW][AD_ROWS];
    __shared__ f32x4 part[NW][NT][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int u = blockIdx.y, tr = blockIdx.x * AD_ROWS + r;
    const bool valid = tr < T;
    const long row = (long)u * T + (valid ? tr : T - 1);  // (rows past the utterance: a clamped load, nothing stored)
    const float* xr = x + row * H;
    const float* gu = g + (long)u * pstride;
    const float* bu = beta + (long)u * pstride;
    const int nch = wt.Hp / 16;

    f32x4 xv[NJ];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int k = 16 * (w + NW * i) + 4 * q;
        const bool in = k < H;
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + (in ? k : 0));
        xv[i] = in ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        s += hsum(xv[i]);
    }
    const float mean = row_sum<NW>(s, red, w, r, q) / H;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int k = 16 * (w + NW * i) + 4 * q;
        const f32x4 d = xv[i] - mean;
        sq += k < H ? hsum(d * d) : 0.f;
    }
    const float rs = 1.0f / sqrtf(row_sum<NW>(sq, red, w, r, q) / H + eps);

    // z^T = W1 y^T over this wave's chunks
    f32x4 a0[NT], a1[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) a0[t] = a1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int j = w + NW * i;
        if (j < nch) {  // (uniform per wave)
            const int k = 16 * j + 4 * q;
            const bool in = k < H;
            const f32x4 gm = *reinterpret_cast<const f32x4*>(gu + (in ? k : 0));
            const f32x4 bt = *reinterpret_cast<const f32x4*>(bu + (in ? k : 0));
            f32x4 y = (xv[i] - mean) * rs * gm + bt;
            if (!in) y = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wt.w1 + (long)(16 * t + r) * wt.Hp + k);
                mfma_k4(wv, y, a0[t], a1[t]);
            }
        }
    }
    f32x4 z[NT];
    wave_reduce<NW, NT>(part, a0, a1, z, w, lane);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const f32x4 pre = z[t] + *reinterpret_cast<const f32x4*>(wt.b1 + 16 * t + 4 * q);
        z[t] = f32x4{fmaxf(pre.x, 0.f), fmaxf(pre.y, 0.f), fmaxf(pre.z, 0.f), fmaxf(pre.w, 0.f)};
    }
    // out^T = x^T + W2 z^T + b2, a 16-column chunk at a time
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int j = w + NW * i;
        if (j < nch) {
            const int k = 16 * j + 4 * q;
            f32x4 o0 = f32x4{0.f, 0.f, 0.f, 0.f}, o1 = o0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wt.w2 + (long)(16 * j + r) * wt.NA + 16 * t + 4 * q);
                mfma_k4(wv, z[t], o0, o1);
            }
            const f32x4 b2 = *reinterpret_cast<const f32x4*>(wt.b2 + k);
            if (valid && k < H) *reinterpret_cast<f32x4*>(out + row * H + k) = xv[i] + ((o0 + o1) + b2);
        }
    }
    if (w == 0 && q == 0 && valid) {
        meanp[row] = mean;
        rstdp[row] = rs;
    }
}

// dx = g + LN-bwd(W1^T ((W2^T g) [z > 0])); per-tile dgamma / dbeta partials into part[u][tile][2][H]
template <int NJ, int NW, int NT>
__global__ __launch_bounds__(NW * 64) void adapter_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gin,
                                                          const float* __restrict__ meanp,
                                                          const float* __restrict__ rstdp, const float* __restrict__ g,
                                                          const float* __restrict__ beta, long pstride, int T, int H,
                                                          AdapterW wt, const int* __restrict__ tlen,
                                                          float* __restrict__ dx, float* __restrict__ partials) {
    __shared__ float red[NW][AD_ROWS];
    __shared__ f32x4 part[NW][NT][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int u = blockIdx.y, tr = blockIdx.x * AD_ROWS + r;
    const bool valid = tr < T;
    const bool live = valid && (tlen == nullptr || tr < tlen[u]);  // padding frames of a ragged batch carry no gradient
    const long row = (long)u * T + (valid ? tr : T - 1);
    const float* xr = x + row * H;
    const float* gr = gin + row * H;
    const float* gu = g + (long)u * pstride;
    const float* bu = beta + (long)u * pstride;
    const int nch = wt.Hp / 16;
    const float mean = valid ? meanp[row] : 0.f, rs = valid ? rstdp[row] : 0.f;

    f32x4 xh[NJ], gv[NJ];  // x-hat (recomputed: bitwise the forward's); the incoming gradient, then g + rstd dy gamma
    f32x4 a0[NT], a1[NT], c0[NT], c1[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) a0[t] = a1[t] = c0[t] = c1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int j = w + NW * i;
        const int k = 16 * j + 4 * q;
        const bool in = k < H;
        const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 xl = *reinterpret_cast<const f32x4*>(xr + (in ? k : 0));
        const f32x4 gl = *reinterpret_cast<const f32x4*>(gr + (in ? k : 0));
        xh[i] = in ? (xl - mean) * rs : zero;
        gv[i] = (in && live) ? gl : zero;
        if (j < nch) {
            const f32x4 gm = *reinterpret_cast<const f32x4*>(gu + (in ? k : 0));
            const f32x4 bt = *reinterpret_cast<const f32x4*>(bu + (in ? k : 0));
            const f32x4 y = in ? xh[i] * gm + bt : zero;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const long o = (long)(16 * t + r) * wt.Hp + k;
                mfma_k4(*reinterpret_cast<const f32x4*>(wt.w1 + o), y, a0[t], a1[t]);       // z^T = W1 y^T
                mfma_k4(*reinterpret_cast<const f32x4*>(wt.w2t + o), gv[i], c0[t], c1[t]);  // W2^T g^T
            }
        }
    }
    f32x4 dz[NT], zp[NT];
    wave_reduce<NW, NT>(part, a0, a1, zp, w, lane);
    wave_reduce<NW, NT>(part, c0, c1, dz, w, lane);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const f32x4 pre = zp[t] + *reinterpret_cast<const f32x4*>(wt.b1 + 16 * t + 4 * q);
        const f32x4 up = dz[t];
        dz[t] = f32x4{pre.x > 0.f ? up.x : 0.f, pre.y > 0.f ? up.y : 0.f, pre.z > 0.f ? up.z : 0.f,
                      pre.w > 0.f ? up.w : 0.f};
    }
    float* pp = partials + ((long)u * gridDim.x + blockIdx.x) * 2 * H;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int j = w + NW * i;
        if (j < nch) {
            const int k = 16 * j + 4 * q;
            const bool in = k < H;
            f32x4 o0 = f32x4{0.f, 0.f, 0.f, 0.f}, o1 = o0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wt.w1t + (long)(16 * j + r) * wt.NA + 16 * t + 4 * q);
                mfma_k4(wv, dz[t], o0, o1);  // dy^T = W1^T dz^T
            }
            const f32x4 dy = o0 + o1;
            const f32x4 gm = *reinterpret_cast<const f32x4*>(gu + (in ? k : 0));
            const f32x4 pg = dy * xh[i];
            const f32x4 dgm = f32x4{row16_sum(pg.x), row16_sum(pg.y), row16_sum(pg.z), row16_sum(pg.w)};
            const f32x4 dbt = f32x4{row16_sum(dy.x), row16_sum(dy.y), row16_sum(dy.z), row16_sum(dy.w)};
            if (r == 0 && in) {
                *reinterpret_cast<f32x4*>(pp + k) = dgm;
                *reinterpret_cast<f32x4*>(pp + H + k) = dbt;
            }
            const f32x4 dg = in ? dy * gm : f32x4{0.f, 0.f, 0.f, 0.f};
            s1 += hsum(dg);
            s2 += hsum(dg * xh[i]);
            gv[i] = gv[i] + rs * dg;
        }
    }
    const float m1 = row_sum<NW>(s1, red, w, r, q) / H;
    const float m2 = row_sum<NW>(s2, red, w, r, q) / H;
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int k = 16 * (w + NW * i) + 4 * q;
        if (valid && k < H) *reinterpret_cast<f32x4*>(dx + row * H + k) = gv[i] - rs * (m1 + xh[i] * m2);
    }
}

// tile partials [B][ntile][2][H] summed over the tiles in order (as ops.hip chunk_reduce)
__global__ __launch_bounds__(256) void adapter_reduce_kernel(const float* __restrict__ part, int ntile, int H,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                             long gstride) {
    const int b = blockIdx.y;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= H) return;
    for (int v = 0; v < 2; ++v) {
        float* out = v == 0 ? dgamma : dbeta;
        if (!out) continue;
        const float* p = part + ((long)b * ntile * 2 + v) * H + c;
        const long cs = 2L * H;
        float s = 0.f;
        int ch = 0;
        for (; ch + 8 <= ntile; ch += 8) {  // 8 loads in flight, summed in tile order: the serial loop's result
            float t[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) t[i] = p[(ch + i) * cs];
#pragma unroll
            for (int i = 0; i < 8; ++i) s += t[i];
        }
        for (; ch < ntile; ++ch) s += p[ch * cs];
        out[(long)b * gstride + c] = s;
    }
}

bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

void check(const AdapterW& w, int H, long pstride, const void* g, const void* beta) {
    if (H < 4 || H % 4 || H > 2048) throw std::invalid_argument("adapter: hidden must be a multiple of 4, <= 2048");
    if (w.A < 1 || w.A > 64 || w.NA != adapter_padded_width(w.A) || w.Hp != (H + 15) / 16 * 16)
        throw std::invalid_argument("adapter: 1 <= adapter_attn_dim <= 64 and padded weights expected");
    if (!a16(g) || !a16(beta) || pstride % 4) throw std::invalid_argument("adapter: 16-B aligned gamma / beta expected");
}

}  // namespace

int adapter_padded_width(int A) { return A <= 16 ? 16 : 64; }
long adapter_part_floats(int B, int rows_per_utt, int H) { return (long)B * ((rows_per_utt + AD_ROWS - 1) / AD_ROWS) * 2 * H; }

// NJ chunks per lane = ceil(H / 16 / NW): 4 waves up to H = 1024, 8 above (the row tile stays in registers)
#define AD_GO(KERNEL, NJ_, NW_, ...)                                                                              \
    do {                                                                                                          \
        if (w.NA == 16) hipLaunchKernelGGL((KERNEL<NJ_, NW_, 1>), grid, dim3(NW_ * 64), 0, st, __VA_ARGS__);      \
        else hipLaunchKernelGGL((KERNEL<NJ_, NW_, 4>), grid, dim3(NW_ * 64), 0, st, __VA_ARGS__);                 \
    } while (0)
#define AD_DISPATCH(KERNEL, ...)                                \
    do {                                                        \
        if (H <= 256) AD_GO(KERNEL, 4, 4, __VA_ARGS__);         \
        else if (H <= 512) AD_GO(KERNEL, 8, 4, __VA_ARGS__);    \
        else if (H <= 1024) AD_GO(KERNEL, 16, 4, __VA_ARGS__);  \
        else if (H <= 1280) AD_GO(KERNEL, 10, 8, __VA_ARGS__);  \
        else AD_GO(KERNEL, 16, 8, __VA_ARGS__);                 \
    } while (0)

void launch_adapter_fwd(const float* x, const float* g, const float* beta, long pstride, int rows_per_utt, int B, int H,
                        const AdapterW& w, float eps, float* out, float* mean, float* rstd, hipStream_t st) {
    check(w, H, pstride, g, beta);
    if (!a16(x) || !a16(out)) throw std::invalid_argument("adapter_fwd: 16-B aligned rows expected");
    const dim3 grid((rows_per_utt + AD_ROWS - 1) / AD_ROWS, B);
    AD_DISPATCH(adapter_fwd_kernel, x, g, beta, pstride, rows_per_utt, H, w, eps, out, mean, rstd);
}

void launch_adapter_bwd(const float* x, const float* dout, const float* mean, const float* rstd, const float* g,
                        const float* beta, long pstride, int rows_per_utt, int B, int H, const AdapterW& w,
                        const int* tlen, float* dx, float* dgamma, float* dbeta, long gstride, float* part,
                        hipStream_t st, void* dxb) {
    check(w, H, pstride, g, beta);
    if (!a16(x) || !a16(dout) || !a16(dx) || !a16(part)) throw std::invalid_argument("adapter_bwd: 16-B aligned rows expected");
    const int ntile = (rows_per_utt + AD_ROWS - 1) / AD_ROWS;
    const dim3 grid(ntile, B);
    AD_DISPATCH(adapter_bwd_kernel, x, dout, mean, rstd, g, beta, pstride, rows_per_utt, H, w, tlen, dx, part);
    if (dxb) launch_to_bf16(dx, H, (long)B * rows_per_utt, H, dxb, st);
    hipLaunchKernelGGL(adapter_reduce_kernel, dim3((H + 255) / 256, B), dim3(256), 0, st, part, ntile, H, dgamma, dbeta,
                       gstride);
}
