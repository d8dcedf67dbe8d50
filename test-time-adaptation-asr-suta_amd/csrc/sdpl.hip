// SDPL objective (reference main_SDPL.py:143-209): pseudo-label CTC loss on the
// model's own greedy transcript, mixed with the SUTA loss:  L = (1 - pl) * L_suta + pl * L_ctc.
//
// pseudo_labeling_loss (main_SDPL.py:192-209), restated:
//   target  = vocab ids of processor.batch_decode(argmax ids): collapse repeats, drop blank 0, the
//             word delimiter '|' (4) decodes to a space and the transcript is strip()ped, so leading
//             and trailing delimiters vanish; every character maps back through vocab.json (a
//             special token <s>, </s>, <unk> decodes to several characters and the reference raises
//             KeyError: flagged here, reported by the engine)
//   lp      = outputs.log_softmax(1): log-softmax over TIME (dim 1 of (1, T, V)), per class
//   L_ctc   = nn.CTCLoss(blank=0, reduction='mean')(lp, target) = nll / max(U, 1)
//   dL/dlp  = torch's CTC backward (LossCTC.cpp): exp(lp) - exp(lcab + nll - lp), lcab = log sum over
//             the extended-target states s with label c of alpha_t(s) beta_t(s); the exp(lp) term
//             assumes lp is normalised over classes, which it is not here -- reproduced as is
//   dL/dz   = through the time log-softmax: g - softmax_t(z)[t,c] * sum_t' g[t',c]
// Two paths.  The 32-letter path below (V <= 32, the 960h rule, no table: ids 1..3 fail, 4 is the delimiter)
// and, further down, the any-vocabulary path, which follows a checkpoint's own vocab.json through a
// pseudo-label table (suta_set_pseudo_labels) and runs every other case (above 32 classes the engine
// refuses SDPL until such a table is set).
// Kernels of the 32-letter path: (1) per utterance (one block): greedy ids, target, time log-softmax, the alpha and beta
// recursions in log space (fp32, torch's 3-term max-shifted log-sum-exp); (2) one thread per
// (frame, class): posterior occupancy and dL/dlp; (3) per utterance: the time-softmax backward and
// the (1 - pl, pl) mix into the SUTA gradient and loss already in dlogits / loss.  Fixed-order sums
// throughout (bitwise reproducible).
#include "ops.h"

namespace {

constexpr int SD_MAXT = 2048;

__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return logf(expf(a - m) + expf(b - m)) + m;
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
    float m = fmaxf(a, fmaxf(b, c));
    if (m == -INFINITY) return -INFINITY;
    return logf(expf(a - m) + expf(b - m) + expf(c - m)) + m;
}

struct SdplScratch {
    float* lp;     // [Tl][32]
    float* g;      // [Tl][32]
    float* alpha;  // [Tl][S]
    float* beta;   // [Tl][S]
    int* tgt;      // [Tl]
    int* meta;     // [4]: U, error flag, T
    float* nll;    // [1]
};

__device__ __forceinline__ SdplScratch sdpl_scratch(float* base, int Tl) {
    const long S = 2L * Tl + 1;
    SdplScratch s;
    s.lp = base;
    s.g = s.lp + (long)Tl * 32;
    s.alpha = s.g + (long)Tl * 32;
    s.beta = s.alpha + (long)Tl * S;
    s.tgt = reinterpret_cast<int*>(s.beta + (long)Tl * S);
    s.meta = s.tgt + Tl;
    s.nll = reinterpret_cast<float*>(s.meta + 4);
    return s;
}

__global__ __launch_bounds__(256) void sdpl_prep_kernel(const float* __restrict__ logits, int Tl, int V,
                                                        const int* __restrict__ tlen, float* __restrict__ scratch,
                                                        long sstride) {
    __shared__ int ids[SD_MAXT];
    __shared__ int tg[SD_MAXT];
    __shared__ float rowa[2 * SD_MAXT + 1], rowb[2 * SD_MAXT + 1];
    __shared__ int sU;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int T = tlen ? tlen[b] : Tl;
    const float* L = logits + (long)b * Tl * V;
    SdplScratch sc = sdpl_scratch(scratch + (long)b * sstride, Tl);

    // greedy ids (first max, torch.argmax)
    for (int t = tid; t < T; t += 256) {
        const float* l = L + (long)t * V;
        float bv = l[0];
        int bi = 0;
        for (int j = 1; j < V; ++j)
            if (l[j] > bv) {
                bv = l[j];
                bi = j;
            }
        ids[t] = bi;
    }
    __syncthreads();
    if (tid == 0) {  // transcript -> target ids (HF decode + strip + vocab lookup)
        int U = 0, prev = -1, err = 0;
        for (int t = 0; t < T; ++t) {
            const int i = ids[t];
            if (i == prev) continue;
            prev = i;
            if (i == 0) continue;
            tg[U++] = i;
        }
        int lo = 0, hi = U;
        while (lo < hi && tg[lo] == 4) ++lo;
        while (hi > lo && tg[hi - 1] == 4) --hi;
        U = hi - lo;
        for (int j = 0; j < U; ++j) {
            tg[j] = tg[lo + j];
            if (tg[j] >= 1 && tg[j] <= 3) err = 1;
        }
        sU = U;
        sc.meta[0] = U;
        sc.meta[1] = err;
        sc.meta[2] = T;
    }
    __syncthreads();
    const int U = sU, S = 2 * U + 1;
    for (int j = tid; j < U; j += 256) sc.tgt[j] = tg[j];

    // lp = log_softmax over time, per class (one wave per class, fixed-order reductions)
    for (int c = w; c < V; c += 4) {
        float m = -INFINITY;
        for (int t = lane; t < T; t += 64) m = fmaxf(m, L[(long)t * V + c]);
        m = wave_max(m);
        float s = 0.f;
        for (int t = lane; t < T; t += 64) s += expf(L[(long)t * V + c] - m);
        s = wave_sum(s);
        const float lz = m + logf(s);
        for (int t = lane; t < T; t += 64) sc.lp[(long)t * 32 + c] = L[(long)t * V + c] - lz;
    }
    __syncthreads();

    auto lab = [&](int s) { return (s & 1) ? tg[s >> 1] : 0; };
    // alpha (Graves eq. 6-7, torch LossCTC.cpp): alpha_0(0) = lp[0][0], alpha_0(1) = lp[0][l1]
    for (int s = tid; s < S; s += 256) {
        float v = -INFINITY;
        if (s == 0) v = sc.lp[0];
        else if (s == 1) v = sc.lp[lab(1)];
        rowa[s] = v;
        sc.alpha[s] = v;
    }
    __syncthreads();
    float* prev = rowa;
    float* cur = rowb;
    for (int t = 1; t < T; ++t) {
        for (int s = tid; s < S; s += 256) {
            const int l = lab(s);
            const float a1 = prev[s];
            const float a2 = s > 0 ? prev[s - 1] : -INFINITY;
            const float a3 = (s > 1 && l != 0 && l != lab(s - 2)) ? prev[s - 2] : -INFINITY;
            const float v = lse3(a1, a2, a3) + sc.lp[(long)t * 32 + l];
            cur[s] = v;
            sc.alpha[(long)t * S + s] = v;
        }
        __syncthreads();
        float* tmp = prev;
        prev = cur;
        cur = tmp;
    }
    if (tid == 0) {
        const float l1 = prev[S - 1];
        const float l2 = S > 1 ? prev[S - 2] : -INFINITY;
        sc.nll[0] = -lse2(l1, l2);
    }
    __syncthreads();
    // beta: beta_{T-1}(S-1) = lp[T-1][l'(S-1)], beta_{T-1}(S-2) = lp[T-1][l'(S-2)]
    for (int s = tid; s < S; s += 256) {
        float v = -INFINITY;
        if (s == S - 1 || s == S - 2) v = sc.lp[(long)(T - 1) * 32 + lab(s)];
        rowa[s] = v;
        sc.beta[(long)(T - 1) * S + s] = v;
    }
    __syncthreads();
    prev = rowa;
    cur = rowb;
    for (int t = T - 2; t >= 0; --t) {
        for (int s = tid; s < S; s += 256) {
            const int l = lab(s);
            const float b1 = prev[s];
            const float b2 = s < S - 1 ? prev[s + 1] : -INFINITY;
            const float b3 = (s < S - 2 && l != 0 && l != lab(s + 2)) ? prev[s + 2] : -INFINITY;
            const float v = lse3(b1, b2, b3) + sc.lp[(long)t * 32 + l];
            cur[s] = v;
            sc.beta[(long)t * S + s] = v;
        }
        __syncthreads();
        float* tmp = prev;
        prev = cur;
        cur = tmp;
    }
}

// g[t][c] = (exp(lp) - sum_{s: l'(s) = c} exp(alpha + beta + nll - lp)) / max(U, 1)
__global__ __launch_bounds__(256) void sdpl_grad_kernel(int Tl, float* __restrict__ scratch, long sstride) {
    const int b = blockIdx.y;
    SdplScratch sc = sdpl_scratch(scratch + (long)b * sstride, Tl);
    const int U = sc.meta[0], T = sc.meta[2], S = 2 * U + 1;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)Tl * 32) return;
    const int t = (int)(i >> 5), c = (int)(i & 31);
    if (t >= T) {
        sc.g[i] = 0.f;
        return;
    }
    const float lp = sc.lp[i], nll = sc.nll[0];
    const float* al = sc.alpha + (long)t * S;
    const float* be = sc.beta + (long)t * S;
    float occ = 0.f;
    if (c == 0) {
        for (int s = 0; s < S; s += 2) occ += expf(al[s] + be[s] + nll - lp);
    } else {
        for (int j = 0; j < U; ++j)
            if (sc.tgt[j] == c) occ += expf(al[2 * j + 1] + be[2 * j + 1] + nll - lp);
    }
    sc.g[i] = (expf(lp) - occ) / (float)max(U, 1);
}

// dz[t][c] = g[t][c] - exp(lp[t][c]) * sum_t g[t][c];  dlogits = (1 - pl) dlogits + pl dz;
// loss = (1 - pl) loss + pl nll / max(U, 1)
__global__ __launch_bounds__(256) void sdpl_combine_kernel(int Tl, int V, float pl, float* __restrict__ dlogits,
                                                           float* __restrict__ loss, float* __restrict__ scratch,
                                                           long sstride, int* __restrict__ err) {
    __shared__ float Gc[32];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    SdplScratch sc = sdpl_scratch(scratch + (long)b * sstride, Tl);
    const int U = sc.meta[0], T = sc.meta[2];
    for (int c = w; c < 32; c += 4) {
        float s = 0.f;
        for (int t = lane; t < T; t += 64) s += sc.g[(long)t * 32 + c];
        s = wave_sum(s);
        if (lane == 0) Gc[c] = s;
    }
    __syncthreads();
    float* dL = dlogits + (long)b * Tl * V;
    const float keep = 1.0f - pl;
    for (long i = tid; i < (long)T * V; i += 256) {
        const int t = (int)(i / V), c = (int)(i % V);
        const long k = (long)t * 32 + c;
        const float dz = sc.g[k] - expf(sc.lp[k]) * Gc[c];
        dL[i] = keep * dL[i] + pl * dz;
    }
    if (tid == 0) {
        loss[b] = keep * loss[b] + pl * (sc.nll[0] / (float)max(U, 1));
        if (sc.meta[1]) atomicOr(err, 1);
    }
}

// ------------------------------------------------------------------------------------------
// Any-vocabulary path (V <= SUTA_MAX_VOCAB, a pseudo-label table, T <= SD_MAXT): six launches.
//   argmax        greedy ids of every frame (ops.hip launch_argmax: a wave per row above 64 classes, first max)
//   wide_lz       lz[c] = log sum_t exp(z[t][c]): a block per (64-class chunk, utterance), lanes along classes so a
//                 row read is contiguous, the time axis over SDW_PART waves combined in wave order; lp = z - lz is
//                 recomputed where it is used instead of stored as a [T][V] plane
//   wide_target   per utterance: collapse repeats, expand every id through the table (dropped / space / lookup
//                 failure / its characters' ids), strip leading and trailing spaces, map inner spaces, check that the
//                 alignment is feasible (U + adjacent repeats <= T), and counting-sort the target positions by class
//   wide_ab       the alpha / beta recursions as sdpl_prep_kernel's, reading lp at the blank and label classes only
//   wide_occ0     the blank's posterior occupancy per frame (a wave per frame over the U + 1 blank states)
//   wide_grad     a block per (64-class chunk, utterance): g = (exp(lp) - occ) / max(U, 1) with occ summed over the
//                 class's position list in position order, Gc = sum_t g over SDW_PART waves in wave order, then the
//                 time-softmax backward and the (1 - pl, pl) mix.  O(T (V + S)) work, fixed-order sums.
// Padding rows t >= T_b enter no statistic; their dlogits stay as the SUTA loss kernel wrote them (0).
// ------------------------------------------------------------------------------------------
constexpr int SDW_PART = 16;  // waves per block of the class-chunk kernels = partial sums over time

struct SdplWide {
    float* lz;     // [V]
    float* g;      // [Tl][V]
    float* alpha;  // [Tl][S]
    float* beta;   // [Tl][S]
    float* occ0;   // [Tl]
    int* tgt;      // [Tl]
    int* pos;      // [Tl] target positions sorted by class (stable)
    int* cstart;   // [V + 1] first entry of each class in pos
    int* meta;     // [8]: U, flags, T
    float* nll;    // [1]
};

__host__ __device__ inline long sdpl_wide_floats(int Tl, int V) {
    const long S = 2L * Tl + 1;
    return (long)V + (long)Tl * V + 2L * Tl * S + 3L * Tl + (V + 1) + 8 + 1 + 16;
}

__device__ __forceinline__ SdplWide sdpl_wide(float* base, int Tl, int V) {
    const long S = 2L * Tl + 1;
    SdplWide s;
    s.lz = base;
    s.g = s.lz + V;
    s.alpha = s.g + (long)Tl * V;
    s.beta = s.alpha + (long)Tl * S;
    s.occ0 = s.beta + (long)Tl * S;
    s.tgt = reinterpret_cast<int*>(s.occ0 + Tl);
    s.pos = s.tgt + Tl;
    s.cstart = s.pos + Tl;
    s.meta = s.cstart + V + 1;
    s.nll = reinterpret_cast<float*>(s.meta + 8);
    return s;
}

__global__ __launch_bounds__(64 * SDW_PART) void sdpl_wide_lz_kernel(const float* __restrict__ logits, int Tl, int V,
                                                                     const int* __restrict__ tlen,
                                                                     float* __restrict__ scratch, long sstride) {
    __shared__ float red[SDW_PART][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const bool ok = c < V;
    const int T = tlen ? tlen[b] : Tl;
    const float* L = logits + (long)b * Tl * V + (ok ? c : 0);
    float m = -INFINITY;
    if (ok)
        for (int t = w; t < T; t += SDW_PART) m = fmaxf(m, L[(long)t * V]);
    red[w][lane] = m;
    __syncthreads();
    m = red[0][lane];
#pragma unroll
    for (int i = 1; i < SDW_PART; ++i) m = fmaxf(m, red[i][lane]);
    __syncthreads();
    float s = 0.f;
    if (ok)
        for (int t = w; t < T; t += SDW_PART) s += expf(L[(long)t * V] - m);
    red[w][lane] = s;
    __syncthreads();
    if (w == 0 && ok) {
        s = red[0][lane];
#pragma unroll
        for (int i = 1; i < SDW_PART; ++i) s += red[i][lane];
        sdpl_wide(scratch + (long)b * sstride, Tl, V).lz[c] = m + logf(s);
    }
}

__global__ __launch_bounds__(256) void sdpl_wide_target_kernel(const int* __restrict__ ids_all, int Tl, int V,
                                                               const int* __restrict__ tlen, SdplTable tab,
                                                               float* __restrict__ scratch, long sstride) {
    __shared__ int tg[SD_MAXT];
    __shared__ int cnt[SUTA_MAX_VOCAB + 1];
    __shared__ int cur[SUTA_MAX_VOCAB];
    __shared__ int sU;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = tlen ? tlen[b] : Tl;
    const int* ids = ids_all + (long)b * Tl;
    SdplWide sc = sdpl_wide(scratch + (long)b * sstride, Tl, V);
    for (int c = tid; c <= V; c += 256) cnt[c] = 0;
    __syncthreads();
    if (tid == 0) {
        int U = 0, prev = -1, flags = 0, spaces = 0;
        bool full = false;
        auto push = [&](int v) {  // a feasible target has U <= T <= SD_MAXT labels
            if (U >= T) full = true;
            else tg[U++] = v;
        };
        for (int t = 0; t < T && !full; ++t) {
            const int i = ids[t];
            if (i == prev) continue;
            prev = i;
            const int k = tab.kind[i];
            if (k == SDPL_KIND_DROP) continue;
            if (k == SDPL_KIND_FAIL) {
                flags |= SDPL_FLAG_LOOKUP;
                continue;
            }
            if (k == SDPL_KIND_SPACE) {  // strip(): kept only between two labels
                if (U > 0) ++spaces;
                continue;
            }
            const int q0 = tab.off[i], q1 = tab.off[i + 1];
            if (q1 > q0) {
                for (; spaces > 0 && !full; --spaces) {
                    if (tab.space_id < 0) flags |= SDPL_FLAG_LOOKUP;
                    else push(tab.space_id);
                }
                spaces = 0;
            }
            for (int q = q0; q < q1 && !full; ++q) push(tab.ids[q]);
        }
        int rep = 0;
        for (int j = 1; j < U; ++j) rep += tg[j] == tg[j - 1];
        if (full || U + rep > T) flags |= SDPL_FLAG_INFEASIBLE;
        if (flags) U = 0;  // the engine raises after the call; the kernels below stay in bounds and finite
        for (int j = 0; j < U; ++j) ++cnt[tg[j] + 1];
        for (int c = 0; c < V; ++c) {
            cnt[c + 1] += cnt[c];
            cur[c] = cnt[c];
        }
        for (int j = 0; j < U; ++j) sc.pos[cur[tg[j]]++] = j;
        sU = U;
        sc.meta[0] = U;
        sc.meta[1] = flags;
        sc.meta[2] = T;
    }
    __syncthreads();
    const int U = sU;
    for (int j = tid; j < U; j += 256) sc.tgt[j] = tg[j];
    for (int c = tid; c <= V; c += 256) sc.cstart[c] = cnt[c];
}

__global__ __launch_bounds__(256) void sdpl_wide_ab_kernel(const float* __restrict__ logits, int Tl, int V,
                                                           float* __restrict__ scratch, long sstride) {
    __shared__ int tg[SD_MAXT];
    __shared__ float lzt[SD_MAXT];
    __shared__ float rowa[2 * SD_MAXT + 1], rowb[2 * SD_MAXT + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* L = logits + (long)b * Tl * V;
    SdplWide sc = sdpl_wide(scratch + (long)b * sstride, Tl, V);
    const int U = sc.meta[0], T = sc.meta[2], S = 2 * U + 1;
    const float lz0 = sc.lz[0];
    for (int j = tid; j < U; j += 256) {
        const int c = sc.tgt[j];
        tg[j] = c;
        lzt[j] = sc.lz[c];
    }
    __syncthreads();
    auto lab = [&](int s) { return (s & 1) ? tg[s >> 1] : 0; };
    auto lp = [&](int t, int s) {  // log-softmax over time at the state's class
        return (s & 1) ? L[(long)t * V + tg[s >> 1]] - lzt[s >> 1] : L[(long)t * V] - lz0;
    };
    for (int s = tid; s < S; s += 256) {
        const float v = s < 2 ? lp(0, s) : -INFINITY;
        rowa[s] = v;
        sc.alpha[s] = v;
    }
    __syncthreads();
    float* prev = rowa;
    float* cur = rowb;
    for (int t = 1; t < T; ++t) {
        for (int s = tid; s < S; s += 256) {
            const int l = lab(s);
            const float a1 = prev[s];
            const float a2 = s > 0 ? prev[s - 1] : -INFINITY;
            const float a3 = (s > 1 && l != 0 && l != lab(s - 2)) ? prev[s - 2] : -INFINITY;
            const float v = lse3(a1, a2, a3) + lp(t, s);
            cur[s] = v;
            sc.alpha[(long)t * S + s] = v;
        }
        __syncthreads();
        float* tmp = prev;
        prev = cur;
        cur = tmp;
    }
    if (tid == 0) {
        const float l1 = prev[S - 1];
        const float l2 = S > 1 ? prev[S - 2] : -INFINITY;
        sc.nll[0] = -lse2(l1, l2);
    }
    __syncthreads();
    for (int s = tid; s < S; s += 256) {
        const float v = (s == S - 1 || s == S - 2) ? lp(T - 1, s) : -INFINITY;
        rowa[s] = v;
        sc.beta[(long)(T - 1) * S + s] = v;
    }
    __syncthreads();
    prev = rowa;
    cur = rowb;
    for (int t = T - 2; t >= 0; --t) {
        for (int s = tid; s < S; s += 256) {
            const int l = lab(s);
            const float b1 = prev[s];
            const float b2 = s < S - 1 ? prev[s + 1] : -INFINITY;
            const float b3 = (s < S - 2 && l != 0 && l != lab(s + 2)) ? prev[s + 2] : -INFINITY;
            const float v = lse3(b1, b2, b3) + lp(t, s);
            cur[s] = v;
            sc.beta[(long)t * S + s] = v;
        }
        __syncthreads();
        float* tmp = prev;
        prev = cur;
        cur = tmp;
    }
}

// occ0[t] = sum over the blank states s = 0, 2, .., 2U of exp(alpha + beta + nll - lp[t][0])
__global__ __launch_bounds__(256) void sdpl_wide_occ0_kernel(const float* __restrict__ logits, int Tl, int V,
                                                             float* __restrict__ scratch, long sstride) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    SdplWide sc = sdpl_wide(scratch + (long)b * sstride, Tl, V);
    const int U = sc.meta[0], T = sc.meta[2], S = 2 * U + 1;
    if (t >= T) return;
    const float lp = logits[((long)b * Tl + t) * V] - sc.lz[0], nll = sc.nll[0];
    const float* al = sc.alpha + (long)t * S;
    const float* be = sc.beta + (long)t * S;
    float occ = 0.f;
    for (int j = lane; j <= U; j += 64) occ += expf(al[2 * j] + be[2 * j] + nll - lp);
    occ = wave_sum(occ);
    if (lane == 0) sc.occ0[t] = occ;
}

__global__ __launch_bounds__(64 * SDW_PART) void sdpl_wide_grad_kernel(const float* __restrict__ logits, int Tl, int V,
                                                                       float pl, float* __restrict__ dlogits,
                                                                       float* __restrict__ loss,
                                                                       float* __restrict__ scratch, long sstride,
                                                                       int* __restrict__ err) {
    __shared__ float red[SDW_PART][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const bool ok = c < V;
    SdplWide sc = sdpl_wide(scratch + (long)b * sstride, Tl, V);
    const int U = sc.meta[0], T = sc.meta[2], S = 2 * U + 1;
    const float un = (float)max(U, 1), nll = sc.nll[0];
    const float* L = logits + (long)b * Tl * V;
    float lzc = 0.f, gs = 0.f;
    if (ok) {
        lzc = sc.lz[c];
        const int q0 = sc.cstart[c], q1 = sc.cstart[c + 1];
        for (int t = w; t < T; t += SDW_PART) {
            const float lp = L[(long)t * V + c] - lzc;
            float occ = 0.f;
            if (c == 0) {
                occ = sc.occ0[t];
            } else {
                const float* al = sc.alpha + (long)t * S;
                const float* be = sc.beta + (long)t * S;
                for (int q = q0; q < q1; ++q) {
                    const int s = 2 * sc.pos[q] + 1;
                    occ += expf(al[s] + be[s] + nll - lp);
                }
            }
            const float g = (expf(lp) - occ) / un;
            sc.g[(long)t * V + c] = g;
            gs += g;
        }
    }
    red[w][lane] = gs;
    __syncthreads();
    float Gc = red[0][lane];
#pragma unroll
    for (int i = 1; i < SDW_PART; ++i) Gc += red[i][lane];
    if (ok) {
        float* dL = dlogits + (long)b * Tl * V;
        const float keep = 1.0f - pl;
        for (int t = w; t < T; t += SDW_PART) {  // each thread reads back the g it wrote
            const long k = (long)t * V + c;
            const float dz = sc.g[k] - expf(L[k] - lzc) * Gc;
            dL[k] = keep * dL[k] + pl * dz;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        loss[b] = (1.0f - pl) * loss[b] + pl * (nll / un);
        if (sc.meta[1]) atomicOr(err, sc.meta[1]);
    }
}

}  // namespace

long sdpl_scratch_floats(int Tl, int V) {
    const long S = 2L * Tl + 1;
    const long legacy = 64L * Tl + 2L * Tl * S + Tl + 4 + 1 + 16;
    return std::max(legacy, sdpl_wide_floats(Tl, V)) + Tl;  // + the utterance's share of the greedy-id array
}

void launch_sdpl_loss(const float* logits, int B, int Tl, int V, float pl_coef, const int* tlen, float* dlogits,
                      float* loss, float* scratch, int* err, const SdplTable* tab, hipStream_t st) {
    const long ss = sdpl_scratch_floats(Tl, V) - Tl;  // B per-utterance blocks, then the greedy ids [B][Tl]
    if (tab) {
        int* ids_all = reinterpret_cast<int*>(scratch + (long)B * ss);
        const dim3 cgrid((V + 63) / 64, B);
        launch_argmax(logits, (long)B * Tl, V, ids_all, st);
        hipLaunchKernelGGL(sdpl_wide_lz_kernel, cgrid, dim3(64 * SDW_PART), 0, st, logits, Tl, V, tlen, scratch, ss);
        hipLaunchKernelGGL(sdpl_wide_target_kernel, dim3(B), dim3(256), 0, st, ids_all, Tl, V, tlen, *tab, scratch, ss);
        hipLaunchKernelGGL(sdpl_wide_ab_kernel, dim3(B), dim3(256), 0, st, logits, Tl, V, scratch, ss);
        hipLaunchKernelGGL(sdpl_wide_occ0_kernel, dim3((Tl + 3) / 4, B), dim3(256), 0, st, logits, Tl, V, scratch, ss);
        hipLaunchKernelGGL(sdpl_wide_grad_kernel, cgrid, dim3(64 * SDW_PART), 0, st, logits, Tl, V, pl_coef, dlogits,
                           loss, scratch, ss, err);
        return;
    }
    hipLaunchKernelGGL(sdpl_prep_kernel, dim3(B), dim3(256), 0, st, logits, Tl, V, tlen, scratch, ss);
    hipLaunchKernelGGL(sdpl_grad_kernel, dim3((unsigned)((Tl * 32L + 255) / 256), B), dim3(256), 0, st, Tl, scratch,
                       ss);
    hipLaunchKernelGGL(sdpl_combine_kernel, dim3(B), dim3(256), 0, st, Tl, V, pl_coef, dlogits, loss, scratch, ss,
                       err);
}
