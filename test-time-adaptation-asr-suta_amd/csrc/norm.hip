// The LayerNorm family for gfx950: LayerNorm forward / backward with per-utterance affine gradients (scalar,
// vectorised and fused-conv forms), the positional stack's LayerNorm -> GELU, the chunk / column sums they share; all
// reductions fixed-order (bitwise reproducible).  norm.h: a route computed from site and operands picks the kernel.
#include "norm.h"
#include <stdexcept>

namespace {

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

constexpr int CS_ROWS = 128;
// ------------------------------------------------------------------------------------------
// LayerNorm over D (<= 2048): one wave per row
// ------------------------------------------------------------------------------------------
template <int NPL>  // elements per lane = ceil(D / 64)
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                            const float* __restrict__ beta, long pstride,
                                                            int rows_per_utt, float* __restrict__ y,
                                                            float* __restrict__ xhat, float* __restrict__ rstd,
                                                            int rows, int D, float eps, int gelu_out,
                                                            float* __restrict__ meanp) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int u = (int)(row / rows_per_utt);
    const float* xr = x + row * D;
    float v[NPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int c = lane + i * 64;
        v[i] = c < D ? xr[c] : 0.f;
        s += v[i];
    }
    s = wave_sum(s);
    const float mean = s / D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int c = lane + i * 64;
        const float d = c < D ? v[i] - mean : 0.f;
        q += d * d;
    }
    q = wave_sum(q);
    const float rs = 1.0f / sqrtf(q / D + eps);
    const float* gu = g + (long)u * pstride;
    const float* bu = beta + (long)u * pstride;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int c = lane + i * 64;
        if (c < D) {
            const float xh = (v[i] - mean) * rs;
            if (xhat) xhat[row * D + c] = xh;
            const float o = xh * gu[c] + bu[c];
            y[row * D + c] = gelu_out ? gelu_f(o) : o;
        }
    }
    if (lane == 0) {
        rstd[row] = rs;
        if (meanp) meanp[row] = mean;
    }
}

// ------------------------------------------------------------------------------------------
// data2vec-audio positional stack: LayerNorm(no affine) -> GELU over D (<= 2048), one wave per row, the layout of
// layernorm_fwd_kernel.  Rows at or past the utterance's length (tlen, may be null) are written as 0 in both
// directions, so the next layer's conv sees zero padding there and no gradient leaves them.
//   fwd: a = gelu(xhat) (+ resid: the stack's last layer adds the stack's input), mean and rstd stored
//   bwd: dy = da * gelu'(xhat), dz = rstd * (dy - mean(dy) - xhat * mean(dy * xhat)); xhat recomputed from z
// ------------------------------------------------------------------------------------------
template <int NPL>
__global__ __launch_bounds__(256) void ln_gelu_fwd_kernel(const float* __restrict__ z, const float* __restrict__ resid,
                                                          float* __restrict__ a, float* __restrict__ meanp,
                                                          float* __restrict__ rstd, int rows, int rows_per_utt, int D,
                                                          float eps, const int* __restrict__ tlen) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int u = (int)(row / rows_per_utt);
    const bool valid = !tlen || (int)(row - (long)u * rows_per_utt) < tlen[u];
    const float* zr = z + row * D;
    float v[NPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int c = lane + i * 64;
        v[i] = (valid && c < D) ? zr[c] : 0.f;
        s += v[i];
    }
    s = wave_sum(s);
    const float mean = s / D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int c = lane + i * 64;
        const float d = c < D ? v[i] - mean : 0.f;
        q += d * d;
    }
    q = wave_sum(q);
    const float rs = 1.0f / sqrtf(q / D + eps);
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int c = lane + i * 64;
        if (c < D) {
            float o = valid ? gelu_f((v[i] - mean) * rs) : 0.f;
            if (resid) o += resid[row * D + c];
            a[row * D + c] = o;
        }
    }
    if (lane == 0) {
        rstd[row] = rs;
        meanp[row] = mean;
    }
}

template <int NPL>
__global__ __launch_bounds__(256) void ln_gelu_bwd_kernel(const float* __restrict__ da, const float* __restrict__ z,
                                                          const float* __restrict__ meanp,
                                                          const float* __restrict__ rstd, float* __restrict__ dz,
                                                          int rows, int rows_per_utt, int D,
                                                          const int* __restrict__ tlen) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int u = (int)(row / rows_per_utt);
    const bool valid = !tlen || (int)(row - (long)u * rows_per_utt) < tlen[u];
    if (!valid) {
        for (int c = lane; c < D; c += 64) dz[row * D + c] = 0.f;
        return;
    }
    const float mean = meanp[row], rs = rstd[row];
    float xh[NPL], dy[NPL];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {  // all loads first; columns past D hold xhat = 0, dy = 0
        const int c = lane + i * 64;
        xh[i] = c < D ? z[row * D + c] : mean;
        dy[i] = c < D ? da[row * D + c] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        xh[i] = (xh[i] - mean) * rs;
        dy[i] *= dgelu_f(xh[i]);
        s1 += dy[i];
        s2 += dy[i] * xh[i];
        // erff's polynomial takes ~20 registers per element in flight: without the fence the scheduler interleaves
        // all NPL of them (176 VGPRs at NPL = 16, scratch at 32)
        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    s1 = wave_sum(s1) / D;
    s2 = wave_sum(s2) / D;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int c = lane + i * 64;
        if (c < D) dz[row * D + c] = rs * (dy[i] - s1 - xh[i] * s2);
    }
}

constexpr int LNB_ROWS = 16;
template <int NPL>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ xhat,
                                                            const float* __restrict__ rstd, const float* __restrict__ g,
                                                            const float* __restrict__ beta, long pstride,
                                                            int rows_per_utt, int D, int gelu_in,
                                                            const float* __restrict__ post_aux,
                                                            const float* __restrict__ resid, float* __restrict__ dx,
                                                            float* __restrict__ part, int nchunk,
                                                            const float* __restrict__ xin,
                                                            const float* __restrict__ meanp) {
    // the block's gamma / beta partials cross LDS; D > 1024 (NPL = 32) does the two in turn through one plane
    // (both planes at once would be the whole 64 KB of static LDS)
    constexpr int RP = NPL <= 16 ? 2 : 1;
    __shared__ float red[4][RP][NPL * 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u = blockIdx.y, ch = blockIdx.x;
    const float* gu = g + (long)u * pstride;
    const float* bu = beta + (long)u * pstride;
    float gam[NPL], bet[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int c = lane + i * 64;
        gam[i] = c < D ? gu[c] : 0.f;
        bet[i] = c < D ? bu[c] : 0.f;
    }
    float pg[NPL], pb[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) pg[i] = pb[i] = 0.f;
    const int r0 = ch * LNB_ROWS, r1 = min(rows_per_utt, r0 + LNB_ROWS);
    for (int r = r0 + w; r < r1; r += 4) {
        const long row = (long)u * rows_per_utt + r;
        float gi[NPL], xh[NPL];
        float s1 = 0.f, s2 = 0.f;
        const float rs = rstd[row];
        const float mu = xhat ? 0.f : meanp[row];
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const int c = lane + i * 64;
            if (c < D) {
                xh[i] = xhat ? xhat[row * D + c] : (xin[row * D + c] - mu) * rs;  // recomputed: bitwise the fwd x-hat
                float d = dy[row * D + c];
                if (gelu_in) d *= dgelu_f(xh[i] * gam[i] + bet[i]);
                gi[i] = d;
                pg[i] += d * xh[i];
                pb[i] += d;
                const float dg = d * gam[i];
                s1 += dg;
                s2 += dg * xh[i];
            } else {
                xh[i] = gi[i] = 0.f;
            }
        }
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        const float m1 = s1 / D, m2 = s2 / D;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const int c = lane + i * 64;
            if (c < D) {
                float o = rs * (gi[i] * gam[i] - m1 - xh[i] * m2);
                if (post_aux) o *= dgelu_f(post_aux[row * D + c]);
                if (resid) o += resid[row * D + c];
                dx[row * D + c] = o;
            }
        }
    }
    if (part) {
        float* pp = part + ((long)u * nchunk + ch) * 2 * D;
        if constexpr (RP == 2) {
#pragma unroll
            for (int i = 0; i < NPL; ++i) {
                red[w][0][lane + i * 64] = pg[i];
                red[w][1][lane + i * 64] = pb[i];
            }
            __syncthreads();
            for (int c = threadIdx.x; c < D; c += 256) {
                pp[c] = red[0][0][c] + red[1][0][c] + red[2][0][c] + red[3][0][c];
                pp[D + c] = red[0][1][c] + red[1][1][c] + red[2][1][c] + red[3][1][c];
            }
        } else {
#pragma unroll
            for (int i = 0; i < NPL; ++i) red[w][0][lane + i * 64] = pg[i];
            __syncthreads();
            for (int c = threadIdx.x; c < D; c += 256) pp[c] = red[0][0][c] + red[1][0][c] + red[2][0][c] + red[3][0][c];
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NPL; ++i) red[w][0][lane + i * 64] = pb[i];
            __syncthreads();
            for (int c = threadIdx.x; c < D; c += 256)
                pp[D + c] = red[0][0][c] + red[1][0][c] + red[2][0][c] + red[3][0][c];
        }
    }
}

// Vectorised LayerNorm forward for D = 256 * NV: one wave per row, lane l owns the 16-B column
// groups l + 64 i.  gamma / beta are read as scalars (their offsets in the flat parameter buffer need
// not be 16-B aligned).
// RPW rows per wave (the bf16-input conv-stack instantiation): every row's loads are issued before the first row's
// reductions, RPW x the bytes in flight per wave (a 1-KB bf16 row per wave kept the conv LayerNorms latency-bound)
// FG (bf16-input conv-stack instantiations, SUTA_FAST_GELU): the output GELU by the packed A&S form of the bf16-plane
// GEMM epilogues (common.h gelu2_bf16ep) instead of erff
template <int NV, bool GV, bool XB = false, int RPW = 1, bool FG = false>  // XB: x is a bf16 plane (widened exactly)
__global__ __launch_bounds__(256) void layernorm_fwd_vec_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ g,
                                                                const float* __restrict__ beta, long pstride,
                                                                int rows_per_utt, float* __restrict__ y,
                                                                float* __restrict__ xhat, float* __restrict__ rstd,
                                                                int rows, float eps, int gelu_out,
                                                                __bf16* __restrict__ yb, float* __restrict__ meanp) {
    constexpr int D = 256 * NV;
    const int lane = threadIdx.x & 63;
    const long row0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
    f32x4 vv[RPW][NV];
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const long rj = min(row0 + j, (long)rows - 1);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if constexpr (XB) vv[j][i] = load_bf16x4(reinterpret_cast<const __bf16*>(x) + rj * D + 4 * (lane + 64 * i));
            else vv[j][i] = reinterpret_cast<const f32x4*>(x + rj * D)[lane + 64 * i];
        }
    }
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
    const long row = row0 + j;
    if (row >= rows) return;
    const int u = (int)(row / rows_per_utt);
    f32x4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = vv[j][i];
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    s = wave_sum(s);
    const float mean = s / D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = v[i][e] - mean;
            q += d * d;
        }
    q = wave_sum(q);
    const float rs = 1.0f / sqrtf(q / D + eps);
    const float* gu = g + (long)u * pstride;
    const float* bu = beta + (long)u * pstride;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = 4 * (lane + 64 * i);
        f32x4 xh, o, gg, bb;
        if constexpr (GV) {  // 16-B aligned gamma / beta (the launcher checks): one load each per 4 columns
            gg = *reinterpret_cast<const f32x4*>(gu + c);
            bb = *reinterpret_cast<const f32x4*>(bu + c);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                gg[e] = gu[c + e];
                bb[e] = bu[c + e];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xh[e] = (v[i][e] - mean) * rs;
            const float t = xh[e] * gg[e] + bb[e];
            o[e] = (gelu_out && !FG) ? gelu_f(t) : t;
        }
        if (FG && gelu_out) {
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
                const f32x2v g2 = gelu2_bf16ep(f32x2v{o[e], o[e + 1]});
                o[e] = g2.x;
                o[e + 1] = g2.y;
            }
        }
        if (xhat) reinterpret_cast<f32x4*>(xhat + row * D)[lane + 64 * i] = xh;
        if (y) reinterpret_cast<f32x4*>(y + row * D)[lane + 64 * i] = o;  // null: only the bf16 plane is read
        if (yb) store_bf16x4(yb + row * D + c, o);  // the bf16 plane of the next GEMM's A operand
    }
    if (lane == 0) {
        rstd[row] = rs;
        if (meanp) meanp[row] = mean;
    }
    }
}

// Vectorised LayerNorm backward for D = 256 * NV: lane l owns the 16-B column groups l + 64 i
// (i < NV) of every row, so every row access is a fully coalesced 1-KiB wave load.  Same arithmetic,
// order and partial layout as layernorm_bwd_kernel.  DYB: dy is a bf16 plane (the input gradient of the linear
// the LayerNorm feeds, written by that GEMM in bf16 only -- torch autocast's bf16 matmul gradient), widened
// exactly on load.
template <int NV, bool GV, bool DYB = false>
__global__ __launch_bounds__(256) void layernorm_bwd_vec_kernel(
    const float* __restrict__ dy, const float* __restrict__ xhat, const float* __restrict__ rstd,
    const float* __restrict__ g, const float* __restrict__ beta, long pstride, int rows_per_utt, int gelu_in,
    const float* __restrict__ post_aux, const float* __restrict__ resid, float* __restrict__ dx,
    float* __restrict__ part, int nchunk, __bf16* __restrict__ dxb, const float* __restrict__ xin,
    const float* __restrict__ meanp) {
    constexpr int D = 256 * NV;
    __shared__ f32x4 red[4][2][NV * 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u = blockIdx.y, ch = blockIdx.x;
    const float* gu = g + (long)u * pstride;
    const float* bu = beta + (long)u * pstride;
    f32x4 gam[NV], bet[NV], pg[NV], pb[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = 4 * (lane + 64 * i);
        if constexpr (GV) {
            gam[i] = *reinterpret_cast<const f32x4*>(gu + c);
            bet[i] = *reinterpret_cast<const f32x4*>(bu + c);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (!GV) {
                gam[i][e] = gu[c + e];
                bet[i][e] = bu[c + e];
            }
            pg[i][e] = pb[i][e] = 0.f;
        }
    }
    const int r0 = ch * LNB_ROWS, r1 = min(rows_per_utt, r0 + LNB_ROWS);
    for (int r = r0 + w; r < r1; r += 4) {
        const long row = (long)u * rows_per_utt + r;
        const f32x4* xr = reinterpret_cast<const f32x4*>((xhat ? xhat : xin) + row * D);
        const f32x4* dr = reinterpret_cast<const f32x4*>(dy + row * D);
        f32x4 gi[NV], xh[NV], pa[NV], rr[NV];
        float s1 = 0.f, s2 = 0.f;
        const float rs = rstd[row];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            xh[i] = xr[lane + 64 * i];
            if constexpr (DYB) gi[i] = load_bf16x4(reinterpret_cast<const __bf16*>(dy) + row * D + 4 * (lane + 64 * i));
            else gi[i] = dr[lane + 64 * i];
        }
        // every load of the row in flight together (the epilogue operands used to wait behind the reductions)
        if (post_aux) {
#pragma unroll
            for (int i = 0; i < NV; ++i) pa[i] = reinterpret_cast<const f32x4*>(post_aux + row * D)[lane + 64 * i];
        }
        if (resid) {
#pragma unroll
            for (int i = 0; i < NV; ++i) rr[i] = reinterpret_cast<const f32x4*>(resid + row * D)[lane + 64 * i];
        }
        if (!xhat) {  // x-hat recomputed from the LayerNorm input: bitwise the forward's value
            const float mu = meanp[row];
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) xh[i][e] = (xh[i][e] - mu) * rs;
        }
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float d = gi[i][e];
                if (gelu_in) d *= dgelu_f(xh[i][e] * gam[i][e] + bet[i][e]);
                gi[i][e] = d;
                pg[i][e] += d * xh[i][e];
                pb[i][e] += d;
                const float dg = d * gam[i][e];
                s1 += dg;
                s2 += dg * xh[i][e];
            }
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        const float m1 = s1 / D, m2 = s2 / D;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] = rs * (gi[i][e] * gam[i][e] - m1 - xh[i][e] * m2);
                if (post_aux) o[e] *= dgelu_f(pa[i][e]);
                if (resid) o[e] += rr[i][e];
            }
            reinterpret_cast<f32x4*>(dx + row * D)[lane + 64 * i] = o;
            if (dxb) store_bf16x4(dxb + row * D + 4 * (lane + 64 * i), o);
        }
    }
    if (part) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            red[w][0][lane + i * 64] = pg[i];
            red[w][1][lane + i * 64] = pb[i];
        }
        __syncthreads();
        f32x4* pp = reinterpret_cast<f32x4*>(part + ((long)u * nchunk + ch) * 2 * D);
        for (int c = threadIdx.x; c < D / 4; c += 256) {
            pp[c] = red[0][0][c] + red[1][0][c] + red[2][0][c] + red[3][0][c];
            pp[D / 4 + c] = red[0][1][c] + red[1][1][c] + red[2][1][c] + red[3][1][c];
        }
    }
}

// Layer-mode conv stack: LayerNorm backward of conv i (D = 512, NV = 2) that also sums what the layer's
// other two consumers of dz_i read it for -- the conv bias gradient (column sums of dz_i) and, for conv0
// (KT = kernel taps), the weight gradient dW0[k][c] = sum_t x[S0 t + k] dz0[t][c] -- so dz_i is read once
// instead of three times (the separate column-sum pass and the conv0 weight-gradient GEMM, 3.4 GB each
// at 64 x 8 s on wav2vec2-large).  Rows in chunks of CROWS per block (larger chunks for the long layers
// keep the partial slabs small); partial layout [B][nchunk][2 + 1 + KT][D]: dgamma, dbeta, dbias, dW0 rows;
// fixed-order reductions (waves, then chunks in order): deterministic.
// FG (SUTA_FAST_GELU, the bf16-plane instantiations): GELU' by the packed A&S form (common.h dgelu2_bf16ep)
template <int NV, bool GV, int KT, bool DYB = false, bool XB = false, bool FG = false>  // DYB / XB: dy / x as bf16
__global__ __launch_bounds__(256) void layernorm_bwd_conv_kernel(
    const float* __restrict__ dy, const float* __restrict__ rstd, const float* __restrict__ g,
    const float* __restrict__ beta, long pstride, int rows_per_utt, float* __restrict__ dx, float* __restrict__ part,
    int nchunk, int crows, const float* __restrict__ xin, const float* __restrict__ meanp,
    const float* __restrict__ xw, long xws, int xs, __bf16* __restrict__ dxb) {
    constexpr int D = 256 * NV;
    constexpr int NVEC = 3 + KT;
    __shared__ f32x4 red[4][2][NV * 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u = blockIdx.y, ch = blockIdx.x;
    const float* gu = g + (long)u * pstride;
    const float* bu = beta + (long)u * pstride;
    f32x4 gam[NV], bet[NV], acc[NVEC][NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = 4 * (lane + 64 * i);
        if constexpr (GV) {
            gam[i] = *reinterpret_cast<const f32x4*>(gu + c);
            bet[i] = *reinterpret_cast<const f32x4*>(bu + c);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                gam[i][e] = gu[c + e];
                bet[i][e] = bu[c + e];
            }
        }
#pragma unroll
        for (int v = 0; v < NVEC; ++v) acc[v][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float* xu = xw ? xw + (long)u * xws : nullptr;
    const int r0 = ch * crows, r1 = min(rows_per_utt, r0 + crows);
    for (int r = r0 + w; r < r1; r += 4) {
        const long row = (long)u * rows_per_utt + r;
        const f32x4* xr = reinterpret_cast<const f32x4*>(xin + row * D);
        const f32x4* dr = reinterpret_cast<const f32x4*>(dy + row * D);
        f32x4 gi[NV], xh[NV];
        float s1 = 0.f, s2 = 0.f;
        const float rs = rstd[row];
        const float mu = meanp[row];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if constexpr (XB) xh[i] = load_bf16x4(reinterpret_cast<const __bf16*>(xin) + row * D + 4 * (lane + 64 * i));
            else xh[i] = xr[lane + 64 * i];
            if constexpr (DYB) gi[i] = load_bf16x4(reinterpret_cast<const __bf16*>(dy) + row * D + 4 * (lane + 64 * i));
            else gi[i] = dr[lane + 64 * i];
        }
        float xt[KT > 0 ? KT : 1];
        if constexpr (KT > 0) {
#pragma unroll
            for (int k = 0; k < KT; ++k) xt[k] = xu[(long)xs * r + k];
        }
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) xh[i][e] = (xh[i][e] - mu) * rs;  // x-hat recomputed bitwise
        if constexpr (FG) {
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int e = 0; e < 4; e += 2) {
                    const f32x2v g2 = dgelu2_bf16ep(f32x2v{xh[i][e] * gam[i][e] + bet[i][e],
                                                           xh[i][e + 1] * gam[i][e + 1] + bet[i][e + 1]});
                    gi[i][e] *= g2.x;
                    gi[i][e + 1] *= g2.y;
                }
        }
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = FG ? gi[i][e] : gi[i][e] * dgelu_f(xh[i][e] * gam[i][e] + bet[i][e]);
                gi[i][e] = d;
                acc[0][i][e] += d * xh[i][e];
                acc[1][i][e] += d;
                const float dg = d * gam[i][e];
                s1 += dg;
                s2 += dg * xh[i][e];
            }
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        const float m1 = s1 / D, m2 = s2 / D;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = rs * (gi[i][e] * gam[i][e] - m1 - xh[i][e] * m2);
            if (dx) reinterpret_cast<f32x4*>(dx + row * D)[lane + 64 * i] = o;  // (null: only the plane is read)
            if (dxb) store_bf16x4(dxb + row * D + 4 * (lane + 64 * i), o);  // the conv GEMMs' bf16 operand plane
            acc[2][i] += o;
#pragma unroll
            for (int k = 0; k < KT; ++k) acc[3 + k][i] += xt[k] * o;
        }
    }
    f32x4* pp = reinterpret_cast<f32x4*>(part + ((long)u * nchunk + ch) * NVEC * D);
#pragma unroll
    for (int v = 0; v < NVEC; v += 2) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            red[w][0][lane + i * 64] = acc[v][i];
            if (v + 1 < NVEC) red[w][1][lane + i * 64] = acc[v + 1][i];
        }
        __syncthreads();
        for (int c = threadIdx.x; c < D / 4; c += 256) {
            pp[v * (D / 4) + c] = red[0][0][c] + red[1][0][c] + red[2][0][c] + red[3][0][c];
            if (v + 1 < NVEC) pp[(v + 1) * (D / 4) + c] = red[0][1][c] + red[1][1][c] + red[2][1][c] + red[3][1][c];
        }
    }
}

// chunk sums of layernorm_bwd_conv_kernel's partials in chunk order: vector 0 -> dgamma, 1 -> dbeta,
// 2 -> dbias (may be null), 3 + k -> dW row k (w_out + k * D)
__global__ __launch_bounds__(256) void chunk_reduce_conv(const float* __restrict__ part, int nchunk, int nvec, int D,
                                                         float* __restrict__ dgam, float* __restrict__ dbet,
                                                         float* __restrict__ dbias, float* __restrict__ wout,
                                                         long ostride) {
    const int b = blockIdx.y, v = blockIdx.z;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    float* out = v == 0 ? dgam : v == 1 ? dbet : v == 2 ? dbias : (wout ? wout + (long)(v - 3) * D : nullptr);
    if (!out) return;
    const float* q = part + ((long)b * nchunk * nvec + v) * D + c;
    const long cs = (long)nvec * D;
    float s = 0.f;
    int chn = 0;
    for (; chn + 8 <= nchunk; chn += 8) {
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = q[(chn + k) * cs];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += t[k];
    }
    for (; chn < nchunk; ++chn) s += q[chn * cs];
    out[(long)b * ostride + c] = s;
}

// sum partial slabs [B][nchunk][nvec][D] over chunks in order -> out_v[b*ostride + c]
// (loads issued 8 chunks at a time, summed in chunk order: the result is that of the serial loop)
__global__ __launch_bounds__(256) void chunk_reduce(const float* __restrict__ part, int nchunk, int nvec, int D,
                                                    float* __restrict__ out0, float* __restrict__ out1, long ostride) {
    const int b = blockIdx.y;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    for (int v = 0; v < nvec; ++v) {
        float* out = v == 0 ? out0 : out1;
        if (!out) continue;
        const float* q = part + ((long)b * nchunk * nvec + v) * D + c;
        const long cs = (long)nvec * D;  // chunk stride
        float s = 0.f;
        int ch = 0;
        for (; ch + 8 <= nchunk; ch += 8) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = q[(ch + u) * cs];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += t[u];
        }
        for (; ch < nchunk; ++ch) s += q[ch * cs];
        out[(long)b * ostride + c] = s;
    }
}

__global__ __launch_bounds__(256) void colsum_partial(const float* __restrict__ x, int rows, int C,
                                                      float* __restrict__ part, int nchunk) {
    const int b = blockIdx.y, ch = blockIdx.x;
    const int r0 = ch * CS_ROWS, r1 = min(rows, r0 + CS_ROWS);
    const float* xb = x + (long)b * rows * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f;
        int r = r0;
        for (; r + 8 <= r1; r += 8) {  // 8 loads in flight, summed in row order
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = xb[(long)(r + u) * C + c];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += t[u];
        }
        for (; r < r1; ++r) s += xb[(long)r * C + c];
        part[((long)b * nchunk + ch) * C + c] = s;
    }
}
// ------------------------------------------------------------------------------------------
// routes: which instantiation a launch takes
// ------------------------------------------------------------------------------------------
bool al(const void* q, int a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }  // (null is aligned)
bool a16(const void* q) { return al(q, 16); }
int npl_of(int D) { return D <= 256 ? 4 : D <= 512 ? 8 : D <= 1024 ? 16 : 32; }  // 32: hidden 1280 / 1920 (XLS-R 1B / 2B)
int scalar_npl(int D, const char* what) {
    if (D > 2048) throw std::invalid_argument(std::string(what) + ": D > 2048");
    return npl_of(D);
}
int conv_crows(int rows_per_utt) { return rows_per_utt >= 4096 ? 128 : 16; }  // larger chunks for the long layers

// The fused conv backward (D = 512, GELU after the LayerNorm, x-hat recomputed), or None when it does not apply.
// On bf16 planes (x, and dy below the last layer): 16-B gamma / beta (every SUTA layout); 8-B planes suffice.
LnRoute conv_bwd_route(const LnSite& s, const LnBwd& io) {
    const LnConvGrads& c = *io.conv;
    const bool xb = io.x.bf16, dyb = io.dy.bf16;
    LnRoute r;
    r.xb = xb;
    r.dyb = dyb;
    r.gv = a16(s.g) && a16(s.beta) && s.pstride % 4 == 0;
    r.part_floats = layernorm_bwd_conv_part_floats(s.B, s.rows_per_utt, s.D, c.ktaps);
    if (s.D != 512 || !s.gelu || s.xhat || !s.mean || !(c.ktaps == 0 || c.ktaps == 10) || (c.ktaps && !c.wave) ||
        !(io.x.f32 || xb) || !s.dgamma || !s.dbeta || (!io.dx.f32 && !io.dx.bf16 && !c.ktaps) || io.post_aux ||
        io.resid || !(dyb || a16(io.dy.f32)) || !(xb || a16(io.x.f32)) || !a16(io.dx.f32) || !a16(io.part) ||
        r.part_floats > io.part_floats || ((xb || dyb) && !(xb && r.gv)))
        return LnRoute{};
    r.kind = LnKernel::ConvBwd;
    r.nv = 2;
    r.kt = c.ktaps;
    r.fg = xb && suta_switches().fast_gelu != 0;  // SUTA_FAST_GELU: the packed A&S GELU'
    r.crows = conv_crows(s.rows_per_utt);
    r.gx = r.nchunk = cdiv(s.rows_per_utt, r.crows);
    r.gy = s.B;
    r.plane_in_kernel = r.sums_conv_grads = true;
    return r;
}

// kernels of a route (every instantiation the library holds is named here, and only here)
using FwdK = decltype(&layernorm_fwd_kernel<4>);
using FwdVecK = decltype(&layernorm_fwd_vec_kernel<2, true>);
using BwdK = decltype(&layernorm_bwd_kernel<4>);
using BwdVecK = decltype(&layernorm_bwd_vec_kernel<2, true>);
using ConvK = decltype(&layernorm_bwd_conv_kernel<2, true, 0>);
template <int NV>
FwdVecK fwd_vec_kernel(const LnRoute& r) {
    if (!r.xb) return r.gv ? layernorm_fwd_vec_kernel<NV, true> : layernorm_fwd_vec_kernel<NV, false>;
    if (r.rpw == 2) return r.fg ? layernorm_fwd_vec_kernel<NV, true, true, 2, true> : layernorm_fwd_vec_kernel<NV, true, true, 2, false>;
    return r.fg ? layernorm_fwd_vec_kernel<NV, true, true, 1, true> : layernorm_fwd_vec_kernel<NV, true, true, 1, false>;
}
template <int NV>
BwdVecK bwd_vec_kernel(const LnRoute& r) {
    if (r.dyb) return layernorm_bwd_vec_kernel<NV, true, true>;
    return r.gv ? layernorm_bwd_vec_kernel<NV, true> : layernorm_bwd_vec_kernel<NV, false>;
}
template <int KT>
ConvK conv_kernel(const LnRoute& r) {
    if (!r.xb) return r.gv ? layernorm_bwd_conv_kernel<2, true, KT> : layernorm_bwd_conv_kernel<2, false, KT>;
    if (r.dyb) return r.fg ? layernorm_bwd_conv_kernel<2, true, KT, true, true, true> : layernorm_bwd_conv_kernel<2, true, KT, true, true>;
    return r.fg ? layernorm_bwd_conv_kernel<2, true, KT, false, true, true> : layernorm_bwd_conv_kernel<2, true, KT, false, true>;
}
template <int N>
using Int = std::integral_constant<int, N>;
template <class F>
auto by_nv(int nv, F f) { return nv == 2 ? f(Int<2>{}) : nv == 3 ? f(Int<3>{}) : f(Int<4>{}); }
template <class F>
auto by_npl(int npl, F f) {
    return npl == 4 ? f(Int<4>{}) : npl == 8 ? f(Int<8>{}) : npl == 16 ? f(Int<16>{}) : f(Int<32>{});
}
// (the XB / DYB kernels take their bf16 plane through the fp32 parameter and widen it: the one cast is here)
const float* kernel_arg(const LnIn& in) { return in.f32 ? in.f32 : static_cast<const float*>(in.bf16); }

}  // namespace

bool ln_vec_width(int D) { return D == 512 || D == 768 || D == 1024; }

long layernorm_bwd_conv_part_floats(int B, int rows_per_utt, int D, int ktaps) {
    return (long)B * cdiv(rows_per_utt, conv_crows(rows_per_utt)) * (3 + ktaps) * D;
}

LnRoute ln_fwd_route(const LnSite& s, const LnFwd& io) {
    if (!s.xhat && !s.mean) throw std::runtime_error("layernorm_fwd: x-hat or the row means must be stored");
    if (!io.x.f32 == !io.x.bf16) throw std::invalid_argument("layernorm_fwd: the input is one of fp32 and bf16");
    const long rows = (long)s.B * s.rows_per_utt;
    LnRoute r;
    r.gv = a16(s.g) && a16(s.beta) && s.pstride % 4 == 0;
    if (io.x.bf16) {  // conv stack on bf16 planes: the vectorised widths, 16-B gamma / beta only
        if (!ln_vec_width(s.D) || !al(io.x.bf16, 8) || !a16(io.y.f32) || !a16(s.xhat) || !r.gv)
            throw std::invalid_argument("layernorm_fwd: a bf16 input plane needs the vectorised widths");
        r.xb = true;
        r.rpw = suta_switches().ln_rpw == 2 ? 2 : 1;  // SUTA_LN_RPW: rows per wave of this form
        r.fg = suta_switches().fast_gelu != 0;        // SUTA_FAST_GELU: the packed A&S GELU
    } else if (!io.y.f32 && !(io.y.bf16 && ln_vec_width(s.D))) {
        throw std::runtime_error("layernorm_fwd: the fp32 output may be skipped only beside a bf16 plane");
    }
    if (r.xb || (ln_vec_width(s.D) && a16(io.x.f32) && a16(io.y.f32) && a16(s.xhat))) {
        r.kind = LnKernel::Vec;
        r.nv = s.D / 256;
        r.plane_in_kernel = true;
    } else {
        // (the scalar kernels write y unconditionally, and the plane would be rounded from it afterwards)
        if (!io.y.f32) throw std::invalid_argument("layernorm_fwd: no fp32 output needs 16-B aligned operands");
        r.kind = LnKernel::Scalar;
        r.npl = scalar_npl(s.D, "layernorm_fwd");
    }
    r.gx = cdiv(rows, 4 * r.rpw);
    return r;
}

LnRoute ln_bwd_route(const LnSite& s, const LnBwd& io) {
    if (!io.dy.f32 == !io.dy.bf16) throw std::invalid_argument("layernorm_bwd: dy is one of fp32 and bf16");
    if (io.conv) return conv_bwd_route(s, io);
    if (!s.xhat && (!io.x.f32 || !s.mean)) throw std::runtime_error("layernorm_bwd: x-hat or (x, row means) needed");
    if (!io.dx.f32) throw std::invalid_argument("layernorm_bwd: the fp32 dx is always written");
    LnRoute r;
    r.crows = LNB_ROWS;
    r.gx = r.nchunk = cdiv(s.rows_per_utt, LNB_ROWS);
    r.gy = s.B;
    r.part_floats = (s.dgamma || s.dbeta) ? (long)s.B * r.nchunk * 2 * s.D : 0;
    r.gv = a16(s.g) && a16(s.beta) && s.pstride % 4 == 0;
    const bool vec = ln_vec_width(s.D) && a16(io.dy.f32) && a16(s.xhat) && a16(io.x.f32) && a16(io.dx.f32) &&
                     a16(io.post_aux) && a16(io.resid) && a16(io.part);
    // a bf16 dy plane: the vectorised widths only (the engine's dead-buffer predicate guarantees them)
    if (io.dy.bf16 && !(vec && r.gv && al(io.dy.bf16, 8)))
        throw std::invalid_argument("layernorm_bwd: a bf16 dy plane needs the vectorised widths and 16-B gamma");
    r.dyb = io.dy.bf16;
    if (vec) {
        r.kind = LnKernel::Vec;
        r.nv = s.D / 256;
        r.plane_in_kernel = true;
    } else {
        r.kind = LnKernel::Scalar;
        r.npl = scalar_npl(s.D, "layernorm_bwd");
    }
    return r;
}

void ln_forward(const LnSite& s, const LnFwd& io, hipStream_t st) {
    const LnRoute r = ln_fwd_route(s, io);
    const int rows = s.B * s.rows_per_utt;
    if (r.kind == LnKernel::Vec) {
        const FwdVecK k = by_nv(r.nv, [&](auto n) { return fwd_vec_kernel<decltype(n)::value>(r); });
        hipLaunchKernelGGL(k, dim3(r.gx), dim3(256), 0, st, kernel_arg(io.x), s.g, s.beta, s.pstride, s.rows_per_utt,
                           io.y.f32, s.xhat, s.rstd, rows, s.eps, (int)s.gelu, static_cast<__bf16*>(io.y.bf16), s.mean);
    } else {
        const FwdK k = by_npl(r.npl, [](auto n) { return &layernorm_fwd_kernel<decltype(n)::value>; });
        hipLaunchKernelGGL(k, dim3(r.gx), dim3(256), 0, st, io.x.f32, s.g, s.beta, s.pstride, s.rows_per_utt, io.y.f32,
                           s.xhat, s.rstd, rows, s.D, s.eps, (int)s.gelu, s.mean);
    }
    if (io.y.bf16 && !r.plane_in_kernel) launch_to_bf16(io.y.f32, s.D, rows, s.D, io.y.bf16, st);
}

void ln_backward(const LnSite& s, const LnBwd& io, hipStream_t st) {
    const LnRoute r = ln_bwd_route(s, io);
    const dim3 grid(r.gx, r.gy), rgrid(cdiv(s.D, 256), s.B);
    __bf16* dxb = static_cast<__bf16*>(io.dx.bf16);
    if (r.kind == LnKernel::None) throw std::invalid_argument("layernorm_bwd: the fused conv backward does not apply");
    if (r.kind == LnKernel::ConvBwd) {
        const LnConvGrads& c = *io.conv;
        const ConvK k = r.kt ? conv_kernel<10>(r) : conv_kernel<0>(r);
        hipLaunchKernelGGL(k, grid, dim3(256), 0, st, kernel_arg(io.dy), s.rstd, s.g, s.beta, s.pstride, s.rows_per_utt,
                           io.dx.f32, io.part, r.nchunk, r.crows, kernel_arg(io.x), s.mean, c.wave, c.wave_stride,
                           c.hop, dxb);
        hipLaunchKernelGGL(chunk_reduce_conv, dim3(rgrid.x, rgrid.y, 3 + r.kt), dim3(256), 0, st, io.part, r.nchunk,
                           3 + r.kt, s.D, s.dgamma, s.dbeta, c.dbias, c.dw, s.gstride);
        return;
    }
    float* pp = r.part_floats ? io.part : nullptr;
    if (r.kind == LnKernel::Vec) {
        const BwdVecK k = by_nv(r.nv, [&](auto n) { return bwd_vec_kernel<decltype(n)::value>(r); });
        hipLaunchKernelGGL(k, grid, dim3(256), 0, st, kernel_arg(io.dy), s.xhat, s.rstd, s.g, s.beta, s.pstride,
                           s.rows_per_utt, (int)s.gelu, io.post_aux, io.resid, io.dx.f32, pp, r.nchunk, dxb, io.x.f32,
                           s.mean);
    } else {
        const BwdK k = by_npl(r.npl, [](auto n) { return &layernorm_bwd_kernel<decltype(n)::value>; });
        hipLaunchKernelGGL(k, grid, dim3(256), 0, st, io.dy.f32, s.xhat, s.rstd, s.g, s.beta, s.pstride, s.rows_per_utt,
                           s.D, (int)s.gelu, io.post_aux, io.resid, io.dx.f32, pp, r.nchunk, io.x.f32, s.mean);
    }
    if (dxb && !r.plane_in_kernel) launch_to_bf16(io.dx.f32, s.D, (long)s.B * s.rows_per_utt, s.D, dxb, st);
    if (pp)
        hipLaunchKernelGGL(chunk_reduce, rgrid, dim3(256), 0, st, pp, r.nchunk, 2, s.D, s.dgamma, s.dbeta, s.gstride);
}

void launch_colsum(const float* x, int B, int rows, int C, float* out, long ostride, float* part, hipStream_t st) {
    const int nchunk = cdiv(rows, CS_ROWS);
    hipLaunchKernelGGL(colsum_partial, dim3(nchunk, B), dim3(256), 0, st, x, rows, C, part, nchunk);
    hipLaunchKernelGGL(chunk_reduce, dim3(cdiv(C, 256), B), dim3(256), 0, st, part, nchunk, 1, C, out, (float*)nullptr,
                       ostride);
}

void launch_ln_gelu_fwd(const float* z, const float* resid, float* a, float* mean, float* rstd, int rows,
                        int rows_per_utt, int D, float eps, const int* tlen, hipStream_t st) {
    if (D > 2048) throw std::runtime_error("launch_ln_gelu_fwd: D > 2048");
    const auto k = by_npl(npl_of(D), [](auto n) { return &ln_gelu_fwd_kernel<decltype(n)::value>; });
    hipLaunchKernelGGL(k, dim3((rows + 3) / 4), dim3(256), 0, st, z, resid, a, mean, rstd, rows, rows_per_utt, D, eps,
                       tlen);
}

void launch_ln_gelu_bwd(const float* da, const float* z, const float* mean, const float* rstd, float* dz, int rows,
                        int rows_per_utt, int D, const int* tlen, hipStream_t st) {
    if (D > 2048) throw std::runtime_error("launch_ln_gelu_bwd: D > 2048");
    const auto k = by_npl(npl_of(D), [](auto n) { return &ln_gelu_bwd_kernel<decltype(n)::value>; });
    hipLaunchKernelGGL(k, dim3((rows + 3) / 4), dim3(256), 0, st, da, z, mean, rstd, dz, rows, rows_per_utt, D, tlen);
}
