// Launchers for the non-GEMM kernels of the SUTA step (ops.hip).  All tensors are fp32,
// time-major ([frame][channel]) and packed over the utterances of a batch.
#pragma once
#include "common.h"

// HF feature-extractor normalisation (feature_extraction_wav2vec2.py:78-97), per utterance:
// y = (x - mean) / sqrt(var + 1e-7), population variance.  lens (device, may be null): ragged batch,
// utterance b has lens[b] <= N samples at stride N; its padding samples are written as 0.
void launch_wave_normalize(const float* x, float* y, int B, long N, const int* lens, hipStream_t st);

// conv0: z[b][t][c] = sum_k x[b][s*t + k] * W[b][k][c] (+ bias[b][c]);  W stored [k][c] per utterance.
void launch_conv0(const float* x, long N, const float* W, const float* bias, long wstride, float* z, int B, int L0,
                  int C, int K, int S, hipStream_t st, void* zb = nullptr);  // zb: bf16 output instead of z

// Fused conv0 + GroupNorm + GELU (group mode): conv0 is recomputed from the waveform in each pass.
// fwd: mean/rstd per (utterance, channel) and a = gelu(GN(conv0(x))).  dpart: >= B*ceil(L0/128)*2*C + B*C doubles.
// L0s (device, may be null): ragged batch, utterance b has L0s[b] <= L0 valid frames (statistics and
// gradients over those only).
void launch_front_gn_fwd(const float* x, long N, const float* W, const float* bias, long wstride, int B, int L0, int C,
                         int K, int S, const float* g, const float* beta, float* mean, float* rstd, float* a,
                         double* dpart, const int* L0s, hipStream_t st);
// bwd: da (overwritten with dg) -> dgamma, dbeta and the conv0 weight gradient dW[k][c] (gstride per
// utterance).  fpart: >= B*ceil(L0/128)*K*C floats.
void launch_front_gn_bwd(const float* x, long N, const float* W, const float* bias, long wstride, int B, int L0, int C,
                         int K, int S, const float* g, const float* beta, const float* mean, const float* rstd,
                         float* da, float* dgamma, float* dbeta, float* dW, long gstride, double* dpart, float* fpart,
                         const int* L0s, hipStream_t st);

// LayerNorm forward / backward: norm.h (norm.hip, with the column sums and the stack's LayerNorm -> GELU below)
#include "norm.h"
// Column sums per utterance: out[b][c] = sum_{t < rows} x[b][t][c]   (bias gradients).
void launch_colsum(const float* x, int B, int rows, int C, float* out, long ostride, float* part, hipStream_t st);

// MMS attention adapter of a stable-LN layer (adapter.hip): out = x + W2 relu(W1 LN(x) + b1) + b2, LN's gamma / beta
// of utterance (row / rows_per_utt) at pstride, eps torch's LayerNorm default.  Exact fp32 on v_mfma_f32_16x16x4_f32.
// The frozen linears come zero-padded (NA = adapter_padded_width(A): 16 for A <= 16, else 64; Hp = H rounded up to
// 16) in both orientations:
// w1 [NA][Hp] (linear_1.weight), w1t [Hp][NA] (its transpose), w2 [Hp][NA] (linear_2.weight), w2t [NA][Hp], b1 [NA],
// b2 [Hp]; 1 <= A <= 64, H % 4 == 0, H <= 2048.
struct AdapterW {
    const float *w1, *w1t, *w2, *w2t, *b1, *b2;
    int A, NA, Hp;
};
// fwd: stores the row means and rstd; x stays the backward's input, so out is a separate buffer
void launch_adapter_fwd(const float* x, const float* g, const float* beta, long pstride, int rows_per_utt, int B, int H,
                        const AdapterW& w, float eps, float* out, float* mean, float* rstd, hipStream_t st);
// bwd: dx = dout + LN-bwd(W1^T ((W2^T dout) [z > 0])), x-hat and z recomputed from x; dgamma / dbeta (may be null)
// per utterance at gstride, over the utterance's first tlen[u] frames (tlen null: all), summed through 16-row tile
// partials in tile order (no atomics).  part: >= adapter_part_floats(B, rows_per_utt, H) floats.  dxb: optional bf16
// copy of dx.
int adapter_padded_width(int A);
long adapter_part_floats(int B, int rows_per_utt, int H);
void launch_adapter_bwd(const float* x, const float* dout, const float* mean, const float* rstd, const float* g,
                        const float* beta, long pstride, int rows_per_utt, int B, int H, const AdapterW& w,
                        const int* tlen, float* dx, float* dgamma, float* dbeta, long gstride, float* part,
                        hipStream_t st, void* dxb = nullptr);

// Flash-style fused attention (attn.hip), head dim 64, any T: forward writes ctx and the per-row
// log-sum-exp lse[b][head][t] (no T x T matrix); backward recomputes P from lse and writes dQ, dK, dV
// into dqkv's Q/K/V columns (dqp: flash_dq_scratch_floats floats of per-key-block dQ partials).
// delta[b][head][t] = rowsum(dctx * ctx) (launch_attn_delta).  bf16: operands rounded to bf16 on the bf16
// MFMAs (config C4).  Head dim 64 runs attn.hip's kernels, head dims 64 < dh <= 128 with dh % 8 == 0 those of
// attn_wide.hip (fp32 rows in both modes); false (nothing launched) for any other dh.
bool flash_dh_ok(int dh);  // a head dim the flash kernels take
long flash_dq_scratch_floats(int B, int T, int NH, int dh);
// ctxb / dqkvb (may be null): bf16 copies of ctx / dqkv for the bf16-plane GEMMs that consume them.
// qkv may be null when the launch takes the bf16-plane kernel (flash_*_reads_plane[s]: the engine's test for
// leaving the fp32 qkv unwritten); the launch throws otherwise.  The plane-reading kernels are dh = 64 only.
bool flash_fwd_reads_plane(bool bf16, const void* qkvb, int H, int dh);
bool flash_bwd_reads_planes(bool bf16, const void* qkvb, const void* dctxb, int H, int dh);
bool launch_flash_fwd(const float* qkv, float* ctx, float* lse, int B, int T, int NH, int H, int dh, float scale,
                      const int* tlen, bool bf16, hipStream_t st, void* ctxb = nullptr, const void* qkvb = nullptr);
bool launch_flash_bwd(const float* qkv, const float* dctx, const float* lse, const float* delta, float* dqkv,
                      float* dqp, int B, int T, int NH, int H, int dh, float scale, const int* tlen, bool bf16,
                      hipStream_t st, void* dqkvb = nullptr, const void* qkvb = nullptr,
                      const void* dctxb = nullptr);
// attn_wide.hip (reached through the two launches above)
bool flash_wide_dh(int dh);
long flash_wide_dq_scratch_floats(int B, int T, int NH, int dh);
bool launch_flash_wide_fwd(const float* qkv, float* ctx, float* lse, int B, int T, int NH, int H, int dh, float scale,
                           const int* tlen, bool bf16, hipStream_t st, void* ctxb);
bool launch_flash_wide_bwd(const float* qkv, const float* dctx, const float* lse, const float* delta, float* dqkv,
                           float* dqp, int B, int T, int NH, int H, int dh, float scale, const int* tlen, bool bf16,
                           hipStream_t st, void* dqkvb);
// grouped positional conv (group width 48 or 64, exact fp32 MFMA); fwd: C = R + gelu(conv + bias), C2 = conv + bias;
// bwd: C = conv + R (rows >= tlen -> 0).  false (nothing launched) outside the supported shapes
bool launch_posconv(bool fwd, const float* x, const float* W, const float* bias, const float* R, float* C, float* C2,
                    int B, int T, int H, int G, int K, int pad, const int* tlen, hipStream_t st);
// One conv of data2vec-audio's positional stack on the same kernel, any K >= 1: W = [G][posconv_stack_taps(K)][CG][CG]
// with the taps past K zero (the kernel streams taps in pairs).  fwd: C = conv + bias (pad K / 2); bwd: W the flipped
// taps, pad K - 1 - K / 2, C = conv (+ R when given), rows >= tlen -> 0.  Input rows >= tlen read as zero in both.
int posconv_stack_taps(int K);
bool launch_posconv_stack(bool fwd, const float* x, const float* W, const float* bias, const float* R, float* C, int B,
                          int T, int H, int G, int K, const int* tlen, hipStream_t st);
// LayerNorm(no affine) -> GELU of the stack's rows (D <= 2048; one wave per row).  fwd: a = gelu(xhat) (+ resid when
// given), row mean / rstd stored; bwd: dz = rstd * (dy - mean(dy) - xhat * mean(dy * xhat)), dy = da * gelu'(xhat),
// xhat recomputed from z.  Rows >= tlen[row / rows_per_utt] (tlen may be null) are written as 0 (fwd: resid alone).
void launch_ln_gelu_fwd(const float* z, const float* resid, float* a, float* mean, float* rstd, int rows,
                        int rows_per_utt, int D, float eps, const int* tlen, hipStream_t st);
void launch_ln_gelu_bwd(const float* da, const float* z, const float* mean, const float* rstd, float* dz, int rows,
                        int rows_per_utt, int D, const int* tlen, hipStream_t st);
// bf16 mode, group width 64: Wt = bf16 weights [G][K][n][k] (n = output channel, k = input channel)
bool launch_posconv_bf16(bool fwd, const float* x, const void* Wt, const float* bias, const float* R, float* C,
                         float* C2, int B, int T, int H, int G, int K, int pad, const int* tlen, hipStream_t st);
// In-place row softmax of `nrows` rows of length T (row stride ld).  tlen (device, may be null):
// ragged batch, rows of utterance row / rows_per_utt use their first tlen[u] keys; the rest get 0.
// (GEMM attention path: head dims other than 64)
void launch_softmax_rows(float* s, long nrows, int T, long ld, const int* tlen, long rows_per_utt, hipStream_t st);

// delta[b][h][t] = dot(dO[b][t][head h], O[b][t][head h]): the softmax-backward row term sum_j P_ij dP_ij.
void launch_attn_delta(const float* dO, const float* O, float* delta, int B, int T, int NH, int dh, hipStream_t st);

// out = g * gelu'(z), n elements.
void launch_dgelu_mul(const float* g, const float* z, float* out, long n, hipStream_t st);

// SUTA loss + dL/dlogits for each utterance (reference main.py:26-60, 181-203).
struct LossHP {
    float temp, em_coef, div_coef;
    int reweight, non_blank;
};
// tlen (device, may be null): ragged batch, utterance b has tlen[b] <= T frames at stride T; the
// gradient of its padding frames is written as 0.
// V <= 64: one fused kernel, a block per utterance.  64 < V <= SUTA_MAX_VOCAB, or any V with the SUTA_LOSS_WIDE
// switch: the matrix-free fp64 path (five kernels, a wave per frame / a block per 64-class chunk; ops.hip).  Both
// divide the MCC term by the reference's class_num default 32, whatever V is.  scratch: 8-byte aligned,
// suta_loss_scratch_floats(B, T, V) floats (enough for either path).
#define SUTA_MAX_VOCAB 1024
size_t suta_loss_scratch_floats(int B, long T, int V);
void launch_suta_loss(const float* logits, int B, int T, int V, LossHP hp, const int* tlen, float* dlogits, float* loss,
                      float* scratch, hipStream_t st);

// SDPL pseudo-label CTC objective (main_SDPL.py:143-209; sdpl.hip): mixes pl_coef * L_ctc into the
// SUTA loss / gradient already in loss / dlogits.  scratch: B * sdpl_scratch_floats(T, V) floats (enough for
// either path).  tab == null: the 32-letter kernels (V <= 32, the 960h rule); otherwise the any-vocabulary
// kernels (V <= SUTA_MAX_VOCAB, T <= 2048) with the pseudo-label table in device memory: class id i expands to
// ids[off[i] .. off[i + 1]) (each in [1, V)) when kind[i] is NORMAL, to nothing when DROP (the pad token), to
// a space when SPACE (the word delimiter: stripped at both ends, space_id inside, a lookup failure when
// space_id < 0) and fails the reference's vocab lookup when FAIL.
// *err |= SDPL_FLAG_LOOKUP when a pseudo-label transcript holds a character that is no token (the reference
// raises KeyError), |= SDPL_FLAG_INFEASIBLE when the target admits no alignment in T frames (torch: inf loss,
// NaN gradient); the wide path then computes with an empty target, so nothing non-finite is written.
enum { SDPL_KIND_NORMAL = 0, SDPL_KIND_DROP = 1, SDPL_KIND_SPACE = 2, SDPL_KIND_FAIL = 3 };
enum { SDPL_FLAG_LOOKUP = 1, SDPL_FLAG_INFEASIBLE = 2 };
struct SdplTable {
    const int* off;   // [V + 1]
    const int* ids;   // [off[V]]
    const int* kind;  // [V]
    int space_id;
};
long sdpl_scratch_floats(int T, int V);
void launch_sdpl_loss(const float* logits, int B, int T, int V, float pl_coef, const int* tlen, float* dlogits,
                      float* loss, float* scratch, int* err, const SdplTable* tab, hipStream_t st);

// Argmax ids per frame (first max, like torch.argmax): a row per thread for V <= 64, a wave per row above.
void launch_argmax(const float* logits, long rows, int V, int* ids, hipStream_t st);

// AdamW single-tensor semantics with per-run multiplicity k (k sub-steps with the same gradient).
struct AdamRun {
    long start, len;
    int k;
};
#define SUTA_MAX_RUNS 32
#define ADAM_TAB 52  // floats per optimizer step in the device step table
struct AdamArgs {
    int nruns;
    AdamRun runs[SUTA_MAX_RUNS];
    int blk0[SUTA_MAX_RUNS];  // first block of each run (filled by launch_adam)
    float beta1, beta2, omb1, omb2, eps, lr_wd;  // omb = (1 - beta) rounded from double; lr_wd = lr * wd
    int sgd;  // SUTA_OPT_SGD: p = fma(g, -lr, p) per sub-step (no moments); the step table's [51] holds -lr
    // per sub-step j (1-based t = step0*k + j): step_size and sqrt(bias_correction2), indexed [k-1][j-1]
    float step_size[5][5];
    float bc2_sqrt[5][5];
    // device-resident alternative (graph-replayable): tab[step0 * ADAM_TAB + {0|25} + (k-1) * 5 + j-1] =
    // step_size | bc2_sqrt, tab[.. + 50] = the weight-decay factor 1 - lr_i wd, tab[.. + 51] = -lr_i (SGD), lr_i
    // the scheduled lr of step step0; step0 read from *step (advanced by launch_step_advance); used when tab !=
    // null.  At *step == 0 the moments are taken as zero (not read): every reset of the slots sets the step
    // counter to 0
    const float* tab;
    const int* step;
};
// dst[b][0:n] = src[0:n] for b in [0, B) (n a multiple of 4, 16-B aligned): the episodic slot reset.
void launch_broadcast(float* dst, const float* src, long n, int B, hipStream_t st);
// *step += 1 (one thread): the Adam step counter of graph-replayed SUTA steps.
void launch_step_advance(int* step, hipStream_t st);
void launch_adam(float* P, const float* G, float* M, float* V, long pstride, int B, const AdamArgs& a,
                 hipStream_t st);
