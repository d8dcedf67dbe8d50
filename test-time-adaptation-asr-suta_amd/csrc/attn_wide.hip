// Flash attention for head dims 64 < dh <= 128, dh % 8 == 0 (XLS-R 1B: 80, XLS-R 2B: 120), any T, ragged batches:
// the contract of attn.hip's dh = 64 kernels (ctx and LSE = max + log(sum) from the forward; the backward recomputes
// P and writes dQ, dK, dV; no T x T matrix, fixed summation order, no float atomics).
//
// The head dim is padded inside the kernels to DP = 96 (dh <= 96) or 128 columns: the LDS images and register rows
// hold zeros in columns dh .. DP - 1 (loads past dh are not issued), and no store touches a column >= dh.
//
//   flash_fwd_wide_kernel  block = 4 waves of one (utterance, head); wave = 32 queries whose Q row stays in registers
//                          (DP / 2 VGPRs per lane).  Key tiles of 32 stream through LDS (double-buffered, one barrier
//                          per tile): K row-major, V transposed.  S^T = K Q^T, online softmax in registers,
//                          O^T += V^T P^T over DP / 32 accumulator tiles.
//   flash_bwd_wide_kernel  block = 4 waves = 128 keys of one (utterance, head); wave = 32 keys.  At DP = 128 the K and V
//                          rows of the dh = 64 kernel (2 DP VGPRs per lane) plus the dK^T / dV^T accumulators (2 DP
//                          more) cannot fit 256 VGPRs, so only V stays in registers: K lives in LDS as a row image that
//                          feeds both S = Q K^T (A and B operands both from LDS rows) and the dQ product (which needs
//                          the block's keys in LDS anyway).  4 waves per block leave each wave a whole SIMD's register
//                          file.  Query tiles of 32 (Q, dO, LSE, delta) are double-buffered through LDS; dS crosses LDS
//                          once and the block's dQ partial goes to scratch in MFMA-fragment order.
//   flash_dq_reduce_wide   dQ = sum over key blocks in fixed order, transposed through LDS, rows written whole.
//
// fp32: v_mfma_f32_32x32x2_f32 / 16x16x4_f32; BF16: the operands rounded to bf16 (RNE) at the fragment reads on
// v_mfma_f32_32x32x16_bf16 / 16x16x32_bf16, fp32 accumulation, and the bf16 planes of ctx / dqkv written beside the
// fp32 values.  These kernels read fp32 rows in both modes (the bf16-plane-reading kernels are dh = 64 only).
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdexcept>
#include <type_traits>

#include "attn_common.h"
#include "common.h"
#include "ops.h"

namespace {

constexpr int FW_NW = 4;    // waves per block, forward and backward
constexpr int FW_LDT = 36;  // transposed V tile [DP][32 keys + 4]

// row stride of the [row][DP] images: DP + 4 floats is an odd number of 16-B slots (25 / 33), so the 32 row reads of
// a fragment (lane l32 -> row l32, ds_read_b128) spread over all 16 slot residues, as FA_LD = 68 does at dh = 64
template <int DP>
constexpr int fw_ld() { return DP + 4; }

// The lane's DP-wide register row (B operand of wprod_lr): fp32 X[row][(DP/2) h + 4 m + e], m < DP / 8;
// bf16 X[row][16 s + 8 h + j], s < DP / 16.  Columns >= dh are zero.
template <int DP, bool BF16>
struct WRow;
template <int DP>
struct WRow<DP, false> {
    f32x4 v[DP / 8];
    __device__ __forceinline__ void load(const float* __restrict__ row, int h, int dh) {
#pragma unroll
        for (int m = 0; m < DP / 8; ++m) {
            const int c = (DP / 2) * h + 4 * m;
            v[m] = c < dh ? *reinterpret_cast<const f32x4*>(row + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
};
template <int DP>
struct WRow<DP, true> {
    fbf16x8 v[DP / 16];
    __device__ __forceinline__ void load(const float* __restrict__ row, int h, int dh) {
#pragma unroll
        for (int s = 0; s < DP / 16; ++s) {
            const int c = 16 * s + 8 * h;  // (dh % 8 == 0: an 8-column chunk is whole or empty)
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            v[s] = c < dh ? cvt8(*reinterpret_cast<const f32x4*>(row + c), *reinterpret_cast<const f32x4*>(row + c + 4))
                          : cvt8(z, z);
        }
    }
};

// acc[r8(v,h)][l32] += sum_d L[i][d] X[l32][d]: L = 32 LDS rows of stride fw_ld<DP>() (row i read by lane i), X the
// lane's register row
template <int DP, bool BF16>
__device__ __forceinline__ void wprod_lr(f32x16& acc, const float* __restrict__ L, const WRow<DP, BF16>& x, int l32,
                                         int h) {
    const float* lr = L + l32 * fw_ld<DP>();
    if constexpr (!BF16) {
#pragma unroll
        for (int m = 0; m < DP / 8; ++m) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(lr + (DP / 2) * h + 4 * m);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], x.v[m][e], acc, 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int s = 0; s < DP / 16; ++s) {
            const fbf16x8 a = cvt8(*reinterpret_cast<const f32x4*>(lr + 16 * s + 8 * h),
                                   *reinterpret_cast<const f32x4*>(lr + 16 * s + 8 * h + 4));
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, x.v[s], acc, 0, 0, 0);
        }
    }
}

// the same product with X an LDS row image too (row j read by lane j): acc[i][j] += sum_d L[i][d] X[j][d]
template <int DP, bool BF16>
__device__ __forceinline__ void wprod_ll(f32x16& acc, const float* __restrict__ L, const float* __restrict__ X,
                                         int l32, int h) {
    const float* lr = L + l32 * fw_ld<DP>();
    const float* xr = X + l32 * fw_ld<DP>();
    if constexpr (!BF16) {
#pragma unroll
        for (int m = 0; m < DP / 8; ++m) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(lr + (DP / 2) * h + 4 * m);
            const f32x4 b = *reinterpret_cast<const f32x4*>(xr + (DP / 2) * h + 4 * m);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc, 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int s = 0; s < DP / 16; ++s) {
            const fbf16x8 a = cvt8(*reinterpret_cast<const f32x4*>(lr + 16 * s + 8 * h),
                                   *reinterpret_cast<const f32x4*>(lr + 16 * s + 8 * h + 4));
            const fbf16x8 b = cvt8(*reinterpret_cast<const f32x4*>(xr + 16 * s + 8 * h),
                                   *reinterpret_cast<const f32x4*>(xr + 16 * s + 8 * h + 4));
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
        }
    }
}

// o[t][r8(v,h)][l32] += sum_r L[r][32 t + n] pv_r, t < DP / 32: the contraction index r is the accumulator row of pv
// (pv[v] = row r8(v,h) of column l32); A operand = L read by column (row-major [r][fw_ld], one float per lane)
template <int DP, bool BF16>
__device__ __forceinline__ void wapply_rows(f32x16 (&o)[DP / 32], const float* __restrict__ L, const f32x16& pv,
                                            int l32, int h) {
    constexpr int LD = fw_ld<DP>();
    if constexpr (!BF16) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const float* lr = L + r8(v, h) * LD + l32;
#pragma unroll
            for (int t = 0; t < DP / 32; ++t) o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(lr[32 * t], pv[v], o[t], 0, 0, 0);
        }
    } else {
        // MFMA c takes k-slot 8h + j <-> accumulator register v = 8c + j (row r8(8c + j, h))
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            fbf16x8 b;
#pragma unroll
            for (int j = 0; j < 8; ++j) b[j] = (__bf16)pv[8 * c + j];
#pragma unroll
            for (int t = 0; t < DP / 32; ++t) {
                fbf16x8 a;
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] = (__bf16)L[r8(8 * c + j, h) * LD + 32 * t + l32];
                o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, o[t], 0, 0, 0);
            }
        }
    }
}

// the same contraction with L stored transposed (Lt[n][FW_LDT], n the output row): 16-B reads of four consecutive
// contraction rows r8(4a + 0..3, h) = 8a + 4h + 0..3
template <int DP, bool BF16>
__device__ __forceinline__ void wapply_cols(f32x16 (&o)[DP / 32], const float* __restrict__ Lt, const f32x16& pv,
                                            int l32, int h) {
#pragma unroll
    for (int t = 0; t < DP / 32; ++t) {
        const float* lr = Lt + (32 * t + l32) * FW_LDT + 4 * h;
        if constexpr (!BF16) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(lr + 8 * a);
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[b], pv[4 * a + b], o[t], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                fbf16x8 b;
#pragma unroll
                for (int j = 0; j < 8; ++j) b[j] = (__bf16)pv[8 * c + j];
                const fbf16x8 a = cvt8(*reinterpret_cast<const f32x4*>(lr + 16 * c),
                                       *reinterpret_cast<const f32x4*>(lr + 16 * c + 8));
                o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, o[t], 0, 0, 0);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// LDS: 2 x (K [32][LD] + V^T [DP][36]): DP = 128 -> 69 KB, 96 -> 52 KB (two blocks per CU)
template <int DP>
constexpr size_t fwf_lds_bytes() {
    return sizeof(float) * 2 * ((size_t)32 * fw_ld<DP>() + DP * FW_LDT);
}

template <int DP, bool BF16>
__global__ __launch_bounds__(FW_NW * 64) void flash_fwd_wide_kernel(const float* __restrict__ qkv,
                                                                    float* __restrict__ ctx, float* __restrict__ lse,
                                                                    int T, int NH, int H, int dh, float scale,
                                                                    const int* __restrict__ tlen, int nqb,
                                                                    __bf16* __restrict__ ctxb) {
    constexpr int NT = FW_NW * 64, LD = fw_ld<DP>(), NTL = DP / 32, CPR = DP / 4;
    constexpr int NPT = 32 * CPR / NT;  // float4 of a 32 x DP tile per thread
    static_assert(32 * CPR % NT == 0, "tile items divide over the block");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float(*Ks)[32 * LD] = reinterpret_cast<float(*)[32 * LD]>(smem);                     // [2][32][LD]
    float(*Vt)[DP * FW_LDT] = reinterpret_cast<float(*)[DP * FW_LDT]>(smem + 2 * 32 * LD);  // [2][DP][FW_LDT]
    const int id = xcd_block();
    const int qb = id % nqb, bh = id / nqb, hd = bh % NH, u = bh / NH;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, l32 = lane & 31, h = lane >> 5;
    const int tl = tlen ? tlen[u] : T;
    const long ld = 3L * H;
    const float* Qb = qkv + (long)u * T * ld + hd * dh;
    const float* Kb = Qb + H;
    const float* Vb = Qb + 2 * H;
    const int q0 = (qb * FW_NW + w) * 32;
    const int q = q0 + l32;
    if (tl <= 0) {  // no valid key (block-uniform; the host rejects zero-frame utterances): ctx = 0, LSE = -inf
        if (q < T) {
            for (int c = (dh / 2) * h; c < (dh / 2) * (h + 1); ++c) {
                ctx[((long)u * T + q) * H + hd * dh + c] = 0.f;
                if (ctxb) ctxb[((long)u * T + q) * H + hd * dh + c] = (__bf16)0.f;
            }
            if (h == 0) lse[(long)bh * T + q] = -INFINITY;
        }
        return;
    }
    const bool active = q0 < T;
    const float sl2 = scale * LOG2E;
    WRow<DP, BF16> qv;
    qv.load(Qb + (long)min(q, T - 1) * ld, h, dh);

    // K: CPR lanes per row (row-major image).  V: a wave-instruction covers 16 keys x 4 column chunks, so the
    // transposed 4-byte writes (c4 + e) * FW_LDT + key hit 64 distinct banks (4 * 36 = 16 mod 64 per chunk)
    auto vmap = [](int it, int& key, int& c4) {
        const int l = it & 63, wi = it >> 6;
        key = (l & 15) + 16 * (wi & 1);
        c4 = 4 * ((l >> 4) + 4 * (wi >> 1));
    };
    f32x4 kr[NPT], vr[NPT];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int n = 0; n < NPT; ++n) {
            const int it = threadIdx.x + n * NT, row = it / CPR, c4 = (it % CPR) * 4, key = kt * 32 + row;
            int vk, vc;
            vmap(it, vk, vc);
            kr[n] = vr[n] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (key < T && c4 < dh) kr[n] = *reinterpret_cast<const f32x4*>(Kb + (long)key * ld + c4);
            if (kt * 32 + vk < T && vc < dh) vr[n] = *reinterpret_cast<const f32x4*>(Vb + (long)(kt * 32 + vk) * ld + vc);
        }
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int n = 0; n < NPT; ++n) {
            const int it = threadIdx.x + n * NT, row = it / CPR, c4 = (it % CPR) * 4;
            int vk, vc;
            vmap(it, vk, vc);
            *reinterpret_cast<f32x4*>(&Ks[buf][row * LD + c4]) = kr[n];
#pragma unroll
            for (int e = 0; e < 4; ++e) Vt[buf][(vc + e) * FW_LDT + vk] = vr[n][e];
        }
    };

    const int nkt = (tl + 31) >> 5;  // key tiles holding a valid key (later ones have probability 0)
    f32x16 o[NTL];
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) o[t][v] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;  // log2-domain running maximum; this lane's half of the sum
    fetch(0);
    put(0);
    __syncthreads();
    // full tiles run a body without masks; the utterance's last tile, with the masks, is peeled
    auto tile = [&](int kt, auto last_tag) {
        constexpr bool LAST = decltype(last_tag)::value;
        const int buf = kt & 1;
        if (!LAST) fetch(kt + 1);
        if (active) {
            f32x16 s;
#pragma unroll
            for (int v = 0; v < 16; ++v) s[v] = 0.f;
            wprod_lr<DP, BF16>(s, Ks[buf], qv, l32, h);  // S^T: key r8(v,h), query l32
            float mx = -INFINITY;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const bool ok = !LAST || kt * 32 + r8(v, h) < tl;
                s[v] = ok ? sl2 * s[v] : -INFINITY;
                mx = fmaxf(mx, s[v]);
            }
            mx = half_swap_max(mx);
            const float m_new = fmaxf(m_run, mx);
            float ls = 0.f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                s[v] = __builtin_amdgcn_exp2f(s[v] - m_new);
                ls += s[v];
            }
            if (m_new != m_run) {  // rescale only when the maximum moved (exact: alpha = 1 otherwise)
                const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // 0 on the first tile
                l_run *= alpha;
#pragma unroll
                for (int t = 0; t < NTL; ++t)
#pragma unroll
                    for (int v = 0; v < 16; ++v) o[t][v] *= alpha;
                m_run = m_new;
            }
            l_run += ls;
            wapply_cols<DP, BF16>(o, Vt[buf], s, l32, h);  // O^T[n][q] += sum_key V[key][n] P[q][key]
        }
        if (!LAST) put(buf ^ 1);
        __syncthreads();
    };
    for (int kt = 0; kt + 1 < nkt; ++kt) tile(kt, std::false_type{});
    tile(nkt - 1, std::true_type{});
    if (!active) return;
    const float l_tot = half_swap_sum(l_run);
    if (q >= T) return;
    const float inv = 1.0f / l_tot;
    const long ob = ((long)u * T + q) * H + hd * dh + 4 * h;
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int c = 32 * t + 8 * a;  // columns c + 4h + 0..3 (dh % 8 == 0: in or out as a whole)
            if (c + 4 * h >= dh) continue;
            f32x4 r;
#pragma unroll
            for (int b = 0; b < 4; ++b) r[b] = o[t][4 * a + b] * inv;
            *reinterpret_cast<f32x4*>(ctx + ob + c) = r;
            if (ctxb) {  // bf16 plane of the out-projection's A operand
                fbf16x4 b;
#pragma unroll
                for (int e = 0; e < 4; ++e) b[e] = (__bf16)r[e];
                *reinterpret_cast<fbf16x4*>(ctxb + ob + c) = b;
            }
        }
    if (h == 0) lse[(long)bh * T + q] = (m_run + log2f(l_tot)) * (1.0f / LOG2E);  // natural-log LSE
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
constexpr int FWB_KBP = FW_NW * 32 + 4;  // row stride of the dS tile [32 queries][128 keys + 4]
// LDS: K [128][LD] + dS [32][KBP] + 2 x (Q, dO [32][LD]) + 2 x (LSE, delta [32]): DP = 128 -> 149 KB, 96 -> 117 KB
template <int DP>
constexpr size_t fwb_lds_bytes() {
    return sizeof(float) * ((size_t)(FW_NW * 32 + 4 * 32) * fw_ld<DP>() + 32 * FWB_KBP + 128);
}

template <int DP, bool BF16>
__global__ __launch_bounds__(FW_NW * 64, 1) void flash_bwd_wide_kernel(
    const float* __restrict__ qkv, const float* __restrict__ dctx, const float* __restrict__ lse,
    const float* __restrict__ delta, float* __restrict__ dqkv, float* __restrict__ dqp, int T, int NH, int H, int dh,
    float scale, const int* __restrict__ tlen, int nkb, int gpb, int B, __bf16* __restrict__ dqkvb) {
    constexpr int NW = FW_NW, NT = NW * 64, LD = fw_ld<DP>(), NTL = DP / 32, CPR = DP / 4, KBP = FWB_KBP;
    constexpr int QPT = 32 * CPR / NT;   // float4 of a 32 x DP tile per thread
    constexpr int NSUB = 2 * (DP / 16);  // 16 x 16 dQ sub-tiles of a 32 x DP tile
    constexpr int SUB = NSUB / NW;       // per wave
    static_assert(NSUB % NW == 0, "dQ sub-tiles divide over the waves");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Kr = smem;                  // [128][LD]: K rows of the block's keys (zero past T and past dh)
    float* Ss = Kr + NW * 32 * LD;     // [32][KBP]: dS of the current query tile
    float* Qs = Ss + 32 * KBP;         // [2][32][LD]
    float* Ds = Qs + 2 * 32 * LD;      // [2][32][LD]  (dO = dctx rows)
    float* Ls = Ds + 2 * 32 * LD;      // [2][32] LSE
    float* Dl = Ls + 64;               // [2][32] delta
    const int id = xcd_block();
    const int kb = id % nkb, bh = id / nkb, hd = bh % NH, u = bh / NH;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, l32 = lane & 31, h = lane >> 5;
    const int tl = tlen ? tlen[u] : T;
    const int ng = (T + 31) >> 5;
    const int g0 = kb * gpb, ngb = min(gpb, ng - g0);  // key groups of this block (<= NW)
    const int kbase = g0 * 32;
    const long ld = 3L * H;
    const float* Qb = qkv + (long)u * T * ld + hd * dh;
    const float* Kb = Qb + H;
    const float* Vb = Qb + 2 * H;
    const float* Ob = dctx + (long)u * T * H + hd * dh;
    const float* lb = lse + (long)bh * T;
    const float* db = delta + (long)bh * T;
    const bool active = w < ngb && kbase + 32 * w < tl;
    const int key = kbase + 32 * w + l32;
    const float sl2 = scale * LOG2E;
    WRow<DP, BF16> vv;
    vv.load(Vb + (long)min(key, T - 1) * ld, h, dh);

    // the block's K rows (zero past T and in the padding columns)
    for (int it = threadIdx.x; it < ngb * 32 * CPR; it += NT) {
        const int row = it / CPR, c4 = (it % CPR) * 4, k = kbase + row;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (k < T && c4 < dh) x = *reinterpret_cast<const f32x4*>(Kb + (long)k * ld + c4);
        *reinterpret_cast<f32x4*>(Kr + row * LD + c4) = x;
    }
    // query tiles: Q and dO rows, LSE and delta; tile qt + 1 is loaded into registers at the start of tile qt and
    // written to the other LDS image at its end
    f32x4 qr[QPT], orr[QPT];
    float lr = 0.f;
    auto fetch = [&](int qt) {
#pragma unroll
        for (int n = 0; n < QPT; ++n) {
            const int it = threadIdx.x + n * NT, row = it / CPR, c4 = (it % CPR) * 4, q = qt * 32 + row;
            qr[n] = orr[n] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (q < T && c4 < dh) {
                qr[n] = *reinterpret_cast<const f32x4*>(Qb + (long)q * ld + c4);
                orr[n] = *reinterpret_cast<const f32x4*>(Ob + (long)q * H + c4);
            }
        }
        lr = 0.f;
        const int qq = qt * 32 + (threadIdx.x & 31);
        if (threadIdx.x < 64 && qq < T) lr = threadIdx.x < 32 ? lb[qq] : db[qq];
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int n = 0; n < QPT; ++n) {
            const int it = threadIdx.x + n * NT, row = it / CPR, c4 = (it % CPR) * 4;
            *reinterpret_cast<f32x4*>(Qs + (buf * 32 + row) * LD + c4) = qr[n];
            *reinterpret_cast<f32x4*>(Ds + (buf * 32 + row) * LD + c4) = orr[n];
        }
        if (threadIdx.x < 32) Ls[buf * 32 + threadIdx.x] = lr;
        else if (threadIdx.x < 64) Dl[buf * 32 + threadIdx.x - 32] = lr;
    };

    f32x16 dv[NTL], dk[NTL];
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) dv[t][v] = dk[t][v] = 0.f;
    const int g = lane >> 4, l16 = lane & 15;
    const int kq = ngb * 32;  // contraction length of the dQ product
    const int NQT = (T + 31) >> 5;                              // query tiles of the layout
    const long dq_stride = (long)B * NH * NQT * (NSUB * 256);  // one key block's partials: [B * NH][NQT][NSUB][64][4]
    float* dqb = dqp + kb * dq_stride + (long)bh * NQT * (NSUB * 256);

    const int nqt = (tl + 31) >> 5;  // query tiles past the length: dO rows are 0, nothing to add
    if (!active && w < ngb)         // keys past the length: their dS columns stay 0 for the dQ product
        for (int r = h; r < 32; r += 2) Ss[r * KBP + 32 * w + l32] = 0.f;
    fetch(0);
    put(0);
    __syncthreads();
    for (int qt = 0; qt < nqt; ++qt) {
        const int q0 = qt * 32, buf = qt & 1;
        if (qt + 1 < nqt) fetch(qt + 1);
        const float* Qt = Qs + buf * 32 * LD;
        const float* Dt = Ds + buf * 32 * LD;
        const float* Lt = Ls + buf * 32;
        const float* Dlt = Dl + buf * 32;
        if (active) {
            f32x16 s, dp;
#pragma unroll
            for (int v = 0; v < 16; ++v) s[v] = dp[v] = 0.f;
            wprod_ll<DP, BF16>(s, Qt, Kr + 32 * w * LD, l32, h);  // S[q][key]: query r8(v,h), key on the lane
            wprod_lr<DP, BF16>(dp, Dt, vv, l32, h);               // dP[q][key]
            const bool kok = key < tl;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const f32x4 lq = *reinterpret_cast<const f32x4*>(Lt + 8 * a + 4 * h);
                const f32x4 dq = *reinterpret_cast<const f32x4*>(Dlt + 8 * a + 4 * h);
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int v = 4 * a + b, r = r8(v, h);
                    const bool ok = kok && q0 + r < T;
                    const float p = ok ? __builtin_amdgcn_exp2f(sl2 * s[v] - LOG2E * lq[b]) : 0.f;
                    s[v] = p;
                    dp[v] = scale * (p * (dp[v] - dq[b]));
                }
            }
            wapply_rows<DP, BF16>(dv, Dt, s, l32, h);   // dV^T[n][key] += sum_q dO[q][n] P[q][key]
            wapply_rows<DP, BF16>(dk, Qt, dp, l32, h);  // dK^T[d][key] += sum_q Q[q][d] dS[q][key]
#pragma unroll
            for (int v = 0; v < 16; ++v) Ss[r8(v, h) * KBP + 32 * w + l32] = dp[v];
        }
        __syncthreads();  // dS tile complete
#pragma unroll
        for (int j = 0; j < SUB; ++j) {  // dQ partial of this key block: dQ[q][d] = sum_key dS[q][key] K[key][d]
            const int st = w * SUB + j, qi = st & 1, di = st >> 1;
            if (16 * di >= dh) continue;  // (wave-uniform) a sub-tile of padding columns only: never read
            const float* ar = Ss + (16 * qi + l16) * KBP;
            const float* bc = Kr + 16 * di + l16;  // column of K, one key per LD floats
            f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0;
            if constexpr (!BF16) {
                for (int kc = 0; kc < kq; kc += 32) {
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(ar + kc + 4 * g);
                    const f32x4 a1 = *reinterpret_cast<const f32x4*>(ar + kc + 16 + 4 * g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], bc[(kc + 4 * g + e) * LD], c0, 0, 0, 0);
                        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], bc[(kc + 16 + 4 * g + e) * LD], c1, 0, 0, 0);
                    }
                }
            } else {
                for (int kc = 0; kc < kq; kc += 32) {
                    const fbf16x8 a = cvt8(*reinterpret_cast<const f32x4*>(ar + kc + 8 * g),
                                           *reinterpret_cast<const f32x4*>(ar + kc + 8 * g + 4));
                    fbf16x8 b;
#pragma unroll
                    for (int e = 0; e < 8; ++e) b[e] = (__bf16)bc[(kc + 8 * g + e) * LD];
                    c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c0, 0, 0, 0);
                }
            }
            // fragment order (flash_dq_reduce_wide transposes): one 16-B store per lane, 1 KB contiguous per wave
            *reinterpret_cast<f32x4*>(dqb + ((long)qt * NSUB + st) * 256 + lane * 4) = c0 + c1;
        }
        if (qt + 1 < nqt) put(buf ^ 1);
        __syncthreads();  // next tile visible; dS tile free
    }
    // dK, dV rows of this wave's keys (0 past the length): lane = key, registers = 4 consecutive columns
    if (w < ngb && key < T) {
        const long ob = ((long)u * T + key) * ld + H + hd * dh + 4 * h;
#pragma unroll
        for (int t = 0; t < NTL; ++t)
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int c = 32 * t + 8 * a;
                if (c + 4 * h >= dh) continue;
                f32x4 x, y;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    x[b] = dk[t][4 * a + b];
                    y[b] = dv[t][4 * a + b];
                }
                if (dqkv) {
                    *reinterpret_cast<f32x4*>(dqkv + ob + c) = x;
                    *reinterpret_cast<f32x4*>(dqkv + ob + H + c) = y;
                }
                if (dqkvb) {
                    fbf16x4 bx, by;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        bx[e] = (__bf16)x[e];
                        by[e] = (__bf16)y[e];
                    }
                    *reinterpret_cast<fbf16x4*>(dqkvb + ob + c) = bx;
                    *reinterpret_cast<fbf16x4*>(dqkvb + ob + H + c) = by;
                }
            }
    }
}

// dQ = sum over key blocks in order (query rows < tl; rows past it get 0, as their dS is 0).  Partials in fragment
// order ([kb][B * NH][NQT][NSUB sub-tiles][64 lanes][4]: lane (g, l16) of sub-tile st = qi + 2 di holds rows
// 16 qi + 4 g + 0..3, column 16 di + l16 of its 32 x DP tile): one block per (head, query tile) sums the key blocks'
// tiles in key-block order, transposes them through LDS and writes the tile's dQ rows whole.
template <int DP>
__global__ __launch_bounds__(256) void flash_dq_reduce_wide(const float* __restrict__ dqp, float* __restrict__ dqkv,
                                                            int B, int T, int NH, int H, int dh, int nkb,
                                                            const int* __restrict__ tlen, __bf16* __restrict__ dqkvb) {
    constexpr int NSUB = 2 * (DP / 16), TILE = NSUB * 256;
    __shared__ __attribute__((aligned(16))) float tile[32][DP + 4];
    const int NQT = (T + 31) >> 5;
    const long bt = blockIdx.x;  // bh * NQT + qt
    const int qt = (int)(bt % NQT);
    const long bh = bt / NQT;
    const int hd = (int)(bh % NH), u = (int)(bh / NH);
    const int tl = tlen ? tlen[u] : T;
    const int q0 = qt * 32;
    if (q0 < tl) {  // (block-uniform)
        const long stride = (long)B * NH * NQT * TILE;
        for (int f = threadIdx.x; f < NSUB * 64; f += 256) {  // fragment = sub-tile * 64 + lane
            const int st = f >> 6, ln = f & 63, qi = st & 1, di = st >> 1, g = ln >> 4, l16 = ln & 15;
            if (16 * di >= dh) continue;  // padding columns: not written by the backward
            const f32x4* p = reinterpret_cast<const f32x4*>(dqp + bt * TILE) + f;
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < nkb; ++k) s += p[k * (stride / 4)];
#pragma unroll
            for (int r = 0; r < 4; ++r) tile[16 * qi + 4 * g + r][16 * di + l16] = s[r];
        }
    }
    __syncthreads();
    const int c8n = dh >> 3;  // 8-column chunks per row
    for (int it = threadIdx.x; it < 32 * c8n; it += 256) {
        const int r = it / c8n, c8 = (it % c8n) * 8, q = q0 + r;
        if (q >= T) continue;
        f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
        if (q < tl) {
            lo = *reinterpret_cast<const f32x4*>(&tile[r][c8]);
            hi = *reinterpret_cast<const f32x4*>(&tile[r][c8 + 4]);
        }
        const long o = ((long)u * T + q) * 3 * H + hd * dh + c8;
        if (dqkv) {
            *reinterpret_cast<f32x4*>(dqkv + o) = lo;
            *reinterpret_cast<f32x4*>(dqkv + o + 4) = hi;
        }
        if (dqkvb) *reinterpret_cast<fbf16x8*>(dqkvb + o) = cvt8(lo, hi);
    }
}

template <int DP, bool BF16>
void fwd_go(dim3 grid, hipStream_t st, const float* qkv, float* ctx, float* lse, int T, int NH, int H, int dh,
            float scale, const int* tlen, int nqb, __bf16* ctxb) {
    constexpr size_t lds = fwf_lds_bytes<DP>();
    set_max_lds_once(reinterpret_cast<const void*>(&flash_fwd_wide_kernel<DP, BF16>), lds, "flash_fwd_wide_kernel");
    hipLaunchKernelGGL((flash_fwd_wide_kernel<DP, BF16>), grid, dim3(FW_NW * 64), lds, st, qkv, ctx, lse, T, NH, H, dh,
                       scale, tlen, nqb, ctxb);
}

template <int DP, bool BF16>
void bwd_go(dim3 grid, hipStream_t st, const float* qkv, const float* dctx, const float* lse, const float* delta,
            float* dqkv, float* dqp, int T, int NH, int H, int dh, float scale, const int* tlen, int nkb, int gpb, int B,
            __bf16* dqkvb) {
    constexpr size_t lds = fwb_lds_bytes<DP>();
    static_assert(lds <= 160 * 1024, "flash_bwd_wide_kernel: LDS image over 160 KB");
    set_max_lds_once(reinterpret_cast<const void*>(&flash_bwd_wide_kernel<DP, BF16>), lds, "flash_bwd_wide_kernel");
    hipLaunchKernelGGL((flash_bwd_wide_kernel<DP, BF16>), grid, dim3(FW_NW * 64), lds, st, qkv, dctx, lse, delta, dqkv,
                       dqp, T, NH, H, dh, scale, tlen, nkb, gpb, B, dqkvb);
    const dim3 rgrid((unsigned)((long)B * NH * ((T + 31) / 32)));
    hipLaunchKernelGGL(flash_dq_reduce_wide<DP>, rgrid, dim3(256), 0, st, dqp, dqkv, B, T, NH, H, dh, nkb, tlen, dqkvb);
}

}  // namespace

bool flash_wide_dh(int dh) { return dh > 64 && dh <= 128 && dh % 8 == 0; }

// padded head dim of the kernels' images: the smallest multiple of 32 that holds dh (fewer MFMAs and less LDS than
// running 80 in the 128-wide form)
static int fw_dp(int dh) { return dh <= 96 ? 96 : 128; }

long flash_wide_dq_scratch_floats(int B, int T, int NH, int dh) {
    const int ng = (T + 31) / 32, nkb = (ng + FW_NW - 1) / FW_NW;
    return (long)nkb * B * NH * ng * 32 * fw_dp(dh) + 64;
}

bool launch_flash_wide_fwd(const float* qkv, float* ctx, float* lse, int B, int T, int NH, int H, int dh, float scale,
                           const int* tlen, bool bf16, hipStream_t st, void* ctxb_) {
    if (!flash_wide_dh(dh) || T < 1 || H != NH * dh) return false;
    if (!qkv) throw std::invalid_argument("flash_fwd: head dims above 64 read the fp32 qkv, which was not written");
    __bf16* ctxb = reinterpret_cast<__bf16*>(ctxb_);
    const int ng = (T + 31) / 32, nqb = (ng + FW_NW - 1) / FW_NW;
    const dim3 grid((unsigned)((long)B * NH * nqb));
    if (fw_dp(dh) == 96) {
        if (bf16) fwd_go<96, true>(grid, st, qkv, ctx, lse, T, NH, H, dh, scale, tlen, nqb, ctxb);
        else fwd_go<96, false>(grid, st, qkv, ctx, lse, T, NH, H, dh, scale, tlen, nqb, ctxb);
    } else {
        if (bf16) fwd_go<128, true>(grid, st, qkv, ctx, lse, T, NH, H, dh, scale, tlen, nqb, ctxb);
        else fwd_go<128, false>(grid, st, qkv, ctx, lse, T, NH, H, dh, scale, tlen, nqb, ctxb);
    }
    return true;
}

bool launch_flash_wide_bwd(const float* qkv, const float* dctx, const float* lse, const float* delta, float* dqkv,
                           float* dqp, int B, int T, int NH, int H, int dh, float scale, const int* tlen, bool bf16,
                           hipStream_t st, void* dqkvb_) {
    if (!flash_wide_dh(dh) || T < 1 || H != NH * dh) return false;
    if (!qkv || !dctx)
        throw std::invalid_argument("flash_bwd: head dims above 64 read the fp32 qkv and dctx, which were not written");
    __bf16* dqkvb = reinterpret_cast<__bf16*>(dqkvb_);
    const int ng = (T + 31) / 32;
    const int nkb = (ng + FW_NW - 1) / FW_NW;  // key blocks per head
    const int gpb = (ng + nkb - 1) / nkb;      // key groups per block (balanced)
    const dim3 grid((unsigned)((long)B * NH * nkb));
    if (fw_dp(dh) == 96) {
        if (bf16) bwd_go<96, true>(grid, st, qkv, dctx, lse, delta, dqkv, dqp, T, NH, H, dh, scale, tlen, nkb, gpb, B, dqkvb);
        else bwd_go<96, false>(grid, st, qkv, dctx, lse, delta, dqkv, dqp, T, NH, H, dh, scale, tlen, nkb, gpb, B, dqkvb);
    } else {
        if (bf16) bwd_go<128, true>(grid, st, qkv, dctx, lse, delta, dqkv, dqp, T, NH, H, dh, scale, tlen, nkb, gpb, B, dqkvb);
        else bwd_go<128, false>(grid, st, qkv, dctx, lse, delta, dqkv, dqp, T, NH, H, dh, scale, tlen, nkb, gpb, B, dqkvb);
    }
    return true;
}
