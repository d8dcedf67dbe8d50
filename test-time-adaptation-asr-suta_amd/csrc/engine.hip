// libsuta engine: the SUTA adapt loop (reference main.py:172-215, 327-398) on gfx950.
//
// Per batch of utterances (same length, one slot each) the engine runs, per step:
//   forward with saved activations -> fused entropy+MCC loss-and-grad -> hand-written backward
//   (dX through every frozen op, dW only for collect_params' tensors) -> AdamW with the
//   duplicate-entry multiplicity -> next step's forward doubles as this step's re-inference.
// Layout: every activation is time-major [utterance][frame][channel] in HBM; trainable tensors
// of slot b live in one flat buffer P[b][Pn] (conv weights stored [k][c_in][c_out] so every
// conv layer is a strided-row GEMM); frozen encoder weights are shared by all slots.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/suta.h"
#include "common.h"
#include "ops.h"

namespace {

thread_local std::string g_err;

struct SutaError : std::runtime_error {
    int code;
    SutaError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define HIPCHK(x)                                                                                        \
    do {                                                                                                 \
        hipError_t _e = (x);                                                                             \
        if (_e != hipSuccess)                                                                            \
            throw SutaError(_e == hipErrorOutOfMemory ? SUTA_ERR_OOM : SUTA_ERR_HIP,                      \
                            std::string(#x) + ": " + hipGetErrorString(_e));                             \
    } while (0)

inline long rup(long a, long b) { return (a + b - 1) / b * b; }

// shortest decimal of a float, read back as a double (0.9f -> 0.9)
inline double py_double(float f) {
    char buf[48];
    snprintf(buf, sizeof buf, "%.9g", (double)f);
    double best = atof(buf);
    for (int prec = 1; prec <= 9; ++prec) {
        snprintf(buf, sizeof buf, "%.*g", prec, (double)f);
        const double d = atof(buf);
        if ((float)d == f) {
            best = d;
            break;
        }
    }
    return best;
}

struct Cfg {
    int H, L, NH, F, V, nconv;
    int C[SUTA_MAX_CONV], K[SUTA_MAX_CONV], S[SUTA_MAX_CONV];
    int conv_bias, layer_mode, stable, posK, posG;
    int A;  // attention-adapter width of the stable-LN layers (MMS: 16); 0 = none
    float eps;
    int family;  // SUTA_FAMILY_*: the state-dict prefix; data2vec-audio also the positional stack below
    // data2vec-audio: the positional embedding is posD layers of grouped conv (posK taps each, posG groups) +
    // LayerNorm(no affine) + GELU; 0 = the single weight-normed conv of posK taps (wav2vec2, HuBERT)
    int posD;
};
constexpr int MAX_POS_STACK = 8;
constexpr float POS_STACK_EPS = 1e-5f;  // HF builds the stack's nn.LayerNorm with torch's default eps

// trainable tensor descriptor
struct TP {
    std::string name;
    std::vector<long> shape;  // HF shape
    long off = 0, numel = 0;
    bool conv_w = false;      // stored permuted [k][cin][cout]
    bool ln_member = false;   // belongs to an nn.LayerNorm module
    bool is_bias = false;
    int feat_depth = 0;       // feature-branch module count containing it (train_feature)
};

// kernel families of the per-launch timing (suta_get_timing_ex); the legacy 6-family view folds
// F_ATTN into F_GEMM and F_FRONT into F_NORM
enum Fam { F_GEMM = 0, F_SOFTMAX = 1, F_NORM = 2, F_EW = 3, F_LOSS = 4, F_ADAM = 5, F_FRONT = 6, F_ATTN = 7, NFAM = 8 };

struct DevBuf {
    float* p = nullptr;
    size_t bytes = 0;
    // returns true when (re)allocated
    bool alloc(size_t b) {
        if (b <= bytes) return false;
        if (p) HIPCHK(hipFree(p));
        p = nullptr;
        bytes = 0;
        HIPCHK(hipMalloc(&p, b));
        bytes = b;
        return true;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

// SUTA_FUSED_CONV_LN=0: the layer-mode conv stack's LayerNorm backward without the fused bias / conv0 weight
// gradient sums (separate column-sum pass and GEMM), for A/B runs; from the call's switch snapshot
static bool fused_conv_ln() { return suta_switches().fused_conv_ln != 0; }

struct Arena {
    char* base = nullptr;
    size_t off = 0, cap = 0;
    bool dry = true;
    template <typename T>
    T* take(size_t n) {
        off = rup(off, 256);
        T* r = dry ? nullptr : reinterpret_cast<T*>(base + off);
        off += n * sizeof(T);
        return r;
    }
};

// Algorithmic (compulsory) HBM bytes of one GEMM launch: every operand element touched once — A's unique
// rows (overlapping strided conv rows and conv-A windows counted once), B once per distinct batch slice
// (shared weights once), C written (read too when accumulating), and the epilogue's stored
// pre-activation, residual and auxiliary operands.  Split-K partials and tile re-reads are not counted.
// Element sizes follow what the launch reads and writes: 2 B for a bf16 operand plane (Ab, Bb), the bf16 C
// plane (Cb) and the bf16 pre-activation operands (preb: C2 / aux), 4 B for fp32 operands; an fp32 C that is
// not written (p.C null: the bf16 plane is the only output) costs nothing.  a_fp32: A is read as fp32 even
// though p.Ab is set (the to_bf16 conversion inside the same timed launch reads the fp32 source once).
double gemm_alg_bytes(const GemmParams& p, bool a_fp32 = false) {
    auto zeff = [&](long s0, long s1) -> double {
        if (s0 == 0 && s1 == 0) return 1.0;
        if (s0 == 0) return (double)((p.Z + p.zdiv - 1) / std::max(1, p.zdiv));
        return (double)p.Z;
    };
    const bool bf = p.mode == SUTA_PRECISION_BF16;
    const double ea = (bf && p.Ab && !a_fp32) ? 2.0 : 4.0;
    const double eb = (bf && p.Bb) ? 2.0 : 4.0;
    const double epre = p.preb ? 2.0 : 4.0;
    double a;
    if (p.segK > 0) {
        const long rows = std::min<long>((long)p.M + p.K / p.segK - 1, p.Mvalid > 0 ? p.Mvalid : p.M);
        a = (double)rows * p.segK;
    } else if (!p.ta) {
        const long lda = (bf && p.Ab && !a_fp32) ? p.ldab : p.lda;
        a = lda < p.K ? (double)(p.M - 1) * lda + p.K : (double)p.M * p.K;
    } else {
        const long lda = (bf && p.Ab && !a_fp32) ? p.ldab : p.lda;
        a = lda < p.M ? (double)(p.K - 1) * lda + p.M : (double)p.M * p.K;
    }
    const double mn = (double)p.M * p.N;
    double bytes = ea * a * zeff(p.sA0, p.sA1) + eb * (double)p.K * p.N * zeff(p.sB0, p.sB1);
    double c = 0.0;
    if (p.C) c += 4.0 * mn * ((p.epi & EPI_ACCUM) ? 2 : 1);
    if (p.Cb && bf) c += 2.0 * mn;
    if (p.epi & EPI_STORE_PRE) c += epre * mn;
    if (p.epi & EPI_RESID) c += 4.0 * mn;
    if (p.epi & EPI_DGELU) c += epre * mn;
    if (p.epi & EPI_SMBWD) c += 4.0 * mn;
    if (p.epi & EPI_DELTA) c += 4.0 * mn + 4.0 * (double)p.M * p.dNH;  // O read, delta written
    bytes += c * p.Z;
    return bytes;
}

// ---- GEMM descriptors: forward() and backward() describe every launch through these ----
// One operand: base pointer, row stride, and its batch strides (s0 per z % zdiv, s1 per z / zdiv)
struct Mat {
    const float* p;
    long ld;
    long s0 = 0, s1 = 0;
};
// an operand with one slice per utterance (Z = B, zdiv = 1)
inline Mat utt(const float* p, long ld, long s1) { return {p, ld, 0, s1}; }

// C[z] = op(A[z]) op(B[z]) for z < Z; ta / tb: the operand is stored transposed (common.h)
GemmParams batched(int M, int N, int K, Mat A, int ta, Mat B, int tb, Mat C, int Z, int zdiv) {
    GemmParams g;
    gemm_init(g);
    g.M = M;
    g.N = N;
    g.K = K;
    g.Z = Z;
    g.zdiv = zdiv;
    g.A = A.p;
    g.ta = ta;
    g.lda = A.ld;
    g.sA0 = A.s0;
    g.sA1 = A.s1;
    g.B = B.p;
    g.tb = tb;
    g.ldb = B.ld;
    g.sB0 = B.s0;
    g.sB1 = B.s1;
    g.C = const_cast<float*>(C.p);
    g.ldc = C.ld;
    g.sC0 = C.s0;
    g.sC1 = C.s1;
    return g;
}
// [M][K] activations times a frozen weight: x W^T (tb = 1, W [N][K]) or the input gradient dY W (tb = 0, W [K][N]).
// Ab: bf16 plane of A written by its producer; Cb: bf16 plane of C for the next kernel (bf16 mode; null: none).
// A / C null: the fp32 copy is not read / written (the plane is the operand)
GemmParams linear(const float* A, const void* Ab, const float* W, int tb, float* C, void* Cb, int M, int N, int K) {
    GemmParams g = batched(M, N, K, {A, K}, 0, {W, tb ? K : N}, tb, {C, N}, 1, 1);
    g.Ab = Ab;
    g.ldab = K;
    g.Cb = Cb;
    g.ldcb = N;
    return g;
}
// epilogue operands (common.h: the order the epilogue applies them in)
inline void add_bias(GemmParams& g, const float* b, long s0 = 0, long s1 = 0) {
    g.epi |= EPI_BIAS;
    g.bias = b;
    g.sBias0 = s0;
    g.sBias1 = s1;
}
inline void store_pre(GemmParams& g, Mat pre) {  // C2 = the value before GELU
    g.epi |= EPI_STORE_PRE;
    g.C2 = const_cast<float*>(pre.p);
    g.ldc2 = pre.ld;
    g.sC20 = pre.s0;
    g.sC21 = pre.s1;
}
inline void set_aux(GemmParams& g, int epi, Mat aux) {  // EPI_DGELU: * gelu'(aux); EPI_SMBWD: * aux
    g.epi |= epi;
    g.aux = aux.p;
    g.ldaux = aux.ld;
    g.sAux0 = aux.s0;
    g.sAux1 = aux.s1;
}
inline void set_row_vec(GemmParams& g, const float* v, long s0, long s1) {  // EPI_SMBWD: - v[m]
    g.rowv = v;
    g.sRow0 = s0;
    g.sRow1 = s1;
}
inline void add_resid(GemmParams& g, Mat R) {
    g.epi |= EPI_RESID;
    g.R = R.p;
    g.ldr = R.ld;
    g.sR0 = R.s0;
    g.sR1 = R.s1;
}
// bf16 planes of both operands given by the caller (conv stack; row strides in bf16 elements)
inline void set_planes(GemmParams& g, const void* Ab, long ldab, const void* Bb, long ldbb) {
    g.Ab = Ab;
    g.ldab = ldab;
    g.Bb = Bb;
    g.ldbb = ldbb;
}
// bf16 plane of a per-utterance C (s1 in bf16 elements)
inline void set_c_plane(GemmParams& g, void* Cb, long ldcb, long s1) {
    g.Cb = Cb;
    g.ldcb = ldcb;
    g.sCb1 = s1;
}

struct LayerBufs {
    float *x_in, *xhat1, *rstd1, *y1, *qkv, *P, *lse, *ctx, *hmid, *xhat2, *rstd2, *y2, *u, *x_out;
    float *mean1, *mean2;  // row means when x-hat is recomputed from the stored LayerNorm input (xhat null)
    // attention adapter (A > 0): its input (the FFN output; the adapter kernel writes x_out) and LayerNorm row statistics
    float *ad_in, *ad_mean, *ad_rstd;
};

struct Plan {
    int B = 0;
    long N = 0;
    int Lc[SUTA_MAX_CONV];
    int T = 0, Tp = 0;
    // ragged batch: utterance b has n[b] <= N samples, L0[b] conv0 frames and T[b] <= T frames
    // (device copies); the layout (strides) stays that of the longest utterance, N
    bool ragged = false;
    int *len_n = nullptr, *len_L0 = nullptr, *len_T = nullptr;
    std::vector<int> h_n, h_T;
    // forward
    float *xraw, *x;
    float *z[SUTA_MAX_CONV], *a[SUTA_MAX_CONV], *crstd[SUTA_MAX_CONV], *cmean[SUTA_MAX_CONV];
    float *gn_mean, *gn_rstd;
    float *fp_rstd, *fp_y, *h0, *pz, *e, *enc_rstd, *enc_y;
    // data2vec-audio positional stack: per layer the conv output z_j (the LayerNorm's input) and its row mean / rstd,
    // kept for the backward; the layers' activations a_j ping-pong through two buffers (the last goes into e)
    float *stk_z[MAX_POS_STACK], *stk_mean[MAX_POS_STACK], *stk_rstd[MAX_POS_STACK], *stk_a[2];
    float *fp_mean, *enc_mean;
    // LayerNorms whose input stays stored keep only the row means (x-hat recomputed in the backward):
    // the conv LNs of layer mode, the feature-projection LN, the encoder LN, and every LN of stable
    // (pre-LN) layers; post-LN layers' LN inputs are transient and keep x-hat
    std::vector<LayerBufs> lay;
    long lnpart_floats = 0;
    float *ctx, *gu, *rtmp, *logits;
    // backward
    float *dlogits, *d1, *d2, *d3, *dqkv, *dP, *dqp, *du, *dzc, *dzc2, *lnpart, *loss, *loss_scratch, *c0part, *delta;
    bool flash = false;  // flash attention kernels (head dim 64, or 72 .. 128 in steps of 8): no T x T matrices, per-row LSE
    double* dpart;
    int* ids;
    float* splitws;
    long splitws_floats;
    size_t bytes = 0;
};

}  // namespace

struct suta_engine {
    Cfg c;
    int device = 0;
    hipStream_t st = nullptr;
    int max_batch = 0;
    long max_samples = 0;
    bool attn_fused = true;  // fused attention fwd/bwd kernels where their shape holds; env SUTA_ATTN_FUSED=0 off
    bool posconv_kernel = true;  // dedicated positional-conv kernel (exact fp32 mode); env SUTA_POSCONV=0 off
    bool bf16_planes = true;     // bf16 mode: linears on bf16 operand planes; env SUTA_BF16_PLANES=0 off
    // frozen weights
    std::vector<float*> wqkv, bqkv, wo, bo, w1, b1, w2, b2;
    std::vector<AdapterW> adw;  // attention adapters' frozen linears, zero-padded in both orientations (ops.h)
    float *wpos_f = nullptr, *wpos_b = nullptr, *bpos = nullptr, *wlm = nullptr, *blm = nullptr;
    // bf16 positional-conv weights [G][K][n][k] (fwd: n = c_out, k = c_in; bwd: taps flipped, n = c_in, k = c_out)
    // for posconv_bf16_kernel (group width 64); null otherwise
    void *wpos_bf_f = nullptr, *wpos_bf_b = nullptr;
    // data2vec-audio positional stack (frozen, no weight norm): per layer the conv weights regrouped
    // [G][posconv_stack_taps(posK)][Cg][Cg] in both orientations as wpos_f / wpos_b are (taps past posK zero), and the bias
    std::vector<float*> wstk_f, wstk_b, bstk;
    // trainable
    std::vector<TP> tps;
    std::map<std::string, int> tpi;
    long Pn = 0;
    float *P0 = nullptr, *P = nullptr, *G = nullptr, *Mo = nullptr, *Vo = nullptr;
    long opt_steps = 0;
    // offsets of trainable pieces
    long o_cw[SUTA_MAX_CONV], o_cb[SUTA_MAX_CONV], o_cg[SUTA_MAX_CONV], o_cbeta[SUTA_MAX_CONV];
    long o_fpg, o_fpb, o_pw, o_pb, o_eg, o_eb;
    std::vector<long> o_l1g, o_l1b, o_l2g, o_l2b, o_adg, o_adb;
    // workspace
    DevBuf ws;
    Plan plan;
    DevBuf sdpl_ws;  // SDPL CTC scratch (+ error flag), allocated on first use
    bool sdpl_used = false;
    int* sdpl_err = nullptr;
    // pseudo-label table (suta_set_pseudo_labels; the 960h rule until one is set): [off V+1 | kind V | ids] on the
    // device.  Replacing it drops the captured loop, and pl_epoch is part of the graph key: a capture made with
    // another table is never replayed.
    int* pl_buf = nullptr;
    SdplTable pl_tab{};
    bool pl_default = true;  // the table is the 960h rule: V <= 32 runs the 32-letter kernels
    bool pl_given = false;   // a caller's table is in place (suta_set_pseudo_labels), not the built-in rule
    int pl_epoch = 0;
    void set_pl_table(const std::vector<int>& off, const std::vector<int>& ids, const std::vector<int>& kind,
                      int space_id);
    void default_pl_table(std::vector<int>& off, std::vector<int>& ids, std::vector<int>& kind, int& space_id) const;
    // null = the 32-letter kernels
    // Above 32 classes the 32-letter rule names no vocabulary (which token is id 33?): SDPL there stays refused,
    // as it always was, until the caller hands over the checkpoint's own table.
    const SdplTable* sdpl_table() const {
        if (c.V > 32 && !pl_given)
            throw SutaError(SUTA_ERR_UNSUPPORTED,
                            "SDPL objective at vocab_size > 32 needs the checkpoint's pseudo-label table "
                            "(suta_set_pseudo_labels); without one only vocab_size <= 32 runs, by the 32-letter rule");
        return (c.V <= 32 && pl_default && !suta_switches().sdpl_wide) ? nullptr : &pl_tab;
    }
    // after a call that ran the SDPL objective: the flags its kernels raised (ops.h SDPL_FLAG_*)
    void check_sdpl() {
        if (!sdpl_used) return;
        int e = 0;
        HIPCHK(hipMemcpy(&e, sdpl_err, sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemset(sdpl_err, 0, sizeof(int)));
        sdpl_used = false;
        if (e & SDPL_FLAG_LOOKUP)
            throw SutaError(SUTA_ERR_UNSUPPORTED,
                            "SDPL pseudo label contains a special token (<s>, </s>, <unk>) or another character "
                            "that is no token of the vocabulary: the reference's vocab lookup raises KeyError "
                            "(main_SDPL.py:196-202)");
        if (e & SDPL_FLAG_INFEASIBLE)
            throw SutaError(SUTA_ERR_UNSUPPORTED,
                            "SDPL pseudo label longer than the utterance allows: the expanded target has no CTC "
                            "alignment in the utterance's frames (torch returns an inf loss and NaN gradients, "
                            "main_SDPL.py:204-207); the step ran on an empty target, reset the engine");
    }
    // timing
    bool timing = false;
    double fam_ms[NFAM] = {0};
    long fam_n[NFAM] = {0};
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;
    std::vector<hipEvent_t> evpool;
    bool use_graphs = true;
    int gemm_mode = 0;  // SUTA_PRECISION_*
    // Adam step tables on the device (tab[step0][step_size | bc2_sqrt][k-1][j-1]) and the step counter the
    // kernel reads: a captured SUTA step replays with the right bias corrections
    float* d_adam_tab = nullptr;
    long adam_tab_cap = 0;
    int* d_step = nullptr;
    int h_step = 0;
    // host rows [0, h_lr.size()) of the table for the optimizer scalars in tab_hp (h_lr = each step's scheduled lr,
    // the StepLR chained product carried row to row); rows [0, dev_rows) are on the device.  A non-episodic run
    // grows them by `steps` rows per call instead of rebuilding every row since its start (advisor r5)
    std::vector<float> h_tab;
    std::vector<double> h_lr;
    long dev_rows = 0;
    suta_hparams tab_hp{};
    double lr_at(const suta_hparams& hp, long i);
    // the whole S-step loop of one suta_adapt call (slot reset, forward, S x (backward + Adam + forward),
    // recorded argmax ids and logits into device staging) captured as one graph per key
    struct GraphKey {
        int B = 0;
        long N = 0;
        int ragged = 0, mode = 0, steps = 0, want_logits = 0, want_ids = 0;
        suta_hparams hp{};
        std::vector<int> rec;
        SutaSwitches sw{};  // the call's A/B switch snapshot (buffer formats and kernel choices captured)
        int pl_epoch = 0;   // which pseudo-label table the SDPL kernels were captured with
    };
    hipGraphExec_t loop_graph = nullptr;
    int last_loop_mode = SUTA_LOOP_EAGER;  // suta_get_graph_stats
    long graph_captures = 0, graph_launches = 0;
    GraphKey gkey;
    bool gkey_seen = false;  // key of the previous suta_adapt call (its lazy allocations are done)
    DevBuf recbuf;           // recorded logits [nrec][B*T*V] then ids [nrec][B*T]
    void prepare_adam(const suta_hparams& hp, int steps);
    bool graph_key_repeats(const GraphKey& k);
    void adapt_loop(int B, const suta_hparams& hp, int steps, const int* rec, int nrec, float* rec_logits,
                    int* rec_ids);
    void run_adapt_loop(int B, const suta_hparams& hp, int steps, const int* rec, int nrec, float* rec_logits,
                        int* rec_ids, bool graph_ok);
    void drop_graph() {
        if (loop_graph) (void)hipGraphExecDestroy(loop_graph);
        loop_graph = nullptr;
        gkey_seen = false;
    }
    std::vector<float*> owned;

    ~suta_engine();

    // ---------------- helpers ----------------
    float* dalloc(long n) {
        float* p = nullptr;
        HIPCHK(hipMalloc(&p, std::max<long>(n, 1) * sizeof(float)));
        owned.push_back(p);
        return p;
    }
    hipEvent_t ev() {
        if (!evpool.empty()) {
            hipEvent_t e = evpool.back();
            evpool.pop_back();
            return e;
        }
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        return e;
    }
    double fam_bytes[NFAM] = {0};  // algorithmic HBM bytes of the timed launches (each operand touched once)
    template <typename Fn>
    void timed(int fam, Fn&& fn, double alg_bytes = 0.0) {
        if (!timing) {
            fn();
            return;
        }
        fam_bytes[fam] += alg_bytes;
        hipEvent_t a = ev(), b = ev();
        HIPCHK(hipEventRecord(a, st));
        fn();
        HIPCHK(hipEventRecord(b, st));
        pending.push_back({fam, {a, b}});
        pending_shape.push_back(fam == F_GEMM ? gemm_shape : std::string());
    }
    std::vector<std::string> pending_shape;  // per pending pair: the GEMM shape (census on), else empty
    std::string gemm_shape;
    void collect_timing() {
        for (size_t i = 0; i < pending.size(); ++i) {
            auto& pe = pending[i];
            float ms = 0.f;
            HIPCHK(hipEventSynchronize(pe.second.second));
            HIPCHK(hipEventElapsedTime(&ms, pe.second.first, pe.second.second));
            fam_ms[pe.first] += ms;
            fam_n[pe.first] += 1;
            if (i < pending_shape.size() && !pending_shape[i].empty()) gemm_census_time(pending_shape[i], ms);
            evpool.push_back(pe.second.first);
            evpool.push_back(pe.second.second);
        }
        pending.clear();
        pending_shape.clear();
    }
    // bf16 mode: bf16 planes of the frozen linear weights, {[N][K] for x W^T, [in][out] for dY W}, keyed by
    // the fp32 weight pointer (built once when the mode is selected), and the A plane of the current GEMM
    std::map<const float*, std::pair<void*, void*>> wplanes;
    DevBuf abuf;
    // two bf16 activation planes [B*T][<= max(3H, F)] (ping-pong): written by the producer of a linear's A
    // operand (LayerNorm, flash attention, GEMM epilogue), read by the linear right after
    DevBuf planebuf;
    bool bf16_mode() const { return gemm_mode == SUTA_PRECISION_BF16; }
    bool use_planes() const { return bf16_mode() && !wplanes.empty(); }
    // planes 0 / 1: the ping-pong A planes; plane 2: dctx's plane (the flash backward's dO operand)
    void* plane(int i) {
        if (!use_planes()) return nullptr;
        const size_t half = rup((long)plan.B * plan.T * std::max(3 * c.H, c.F) * 2, 256);
        if (planebuf.alloc(3 * half)) drop_graph();
        return reinterpret_cast<char*>(planebuf.p) + i * half;
    }
    // layer-mode conv stack on bf16 planes (bf16 mode): the conv LayerNorm forwards write bf16 activation planes
    // (ping-pong) that the next conv GEMM reads as its A operand, and the per-slot conv weights are re-laid
    // [C_out][tap * C_in] in bf16 (the B operand) at the start of every forward; SUTA_CONV_PLANES=0 keeps the
    // fp32-staged one-plane kernels
    DevBuf convact, convwt;
    bool conv_planes() const {
        if (!use_planes() || !c.layer_mode) return false;
        if (!suta_switches().conv_planes) return false;
        for (int i = 0; i < c.nconv; ++i)
            if (c.C[i] != 512 || (i > 0 && ((long)c.K[i] * c.C[i - 1] % 8 || (long)c.S[i] * c.C[i - 1] % 8))) return false;
        return true;
    }
    void* conv_act_plane(int i) {  // layer i < nconv - 1: [B][L_i][C_i] bf16, kept for the weight gradients
        size_t off = 0, tot = 0;
        for (int j = 0; j + 1 < c.nconv; ++j) {
            const size_t n = rup((long)plan.B * plan.Lc[j] * c.C[j] * 2, 256);
            if (j < i) off += n;
            tot += n;
        }
        if (convact.alloc(tot)) drop_graph();
        return reinterpret_cast<char*>(convact.p) + off;
    }
    DevBuf convdz;
    // bf16 plane of the current conv layer's dz (the weight gradient's B operand)
    void* conv_dz_plane() {
        size_t n = 0;
        for (int j = 1; j < c.nconv; ++j) n = std::max(n, (size_t)rup((long)plan.B * plan.Lc[j] * c.C[j] * 2, 256));
        if (convdz.alloc(n)) drop_graph();
        return convdz.p;
    }
    // layer i >= 1, native = 0: [B][C_i][K_i * C_{i-1}] bf16 (forward B operand); native = 1: the source layout
    // [B][K_i][C_{i-1}][C_i] (the input gradient's per-tap B segments)
    void* conv_wt_plane(int i, int native = 0) {
        size_t off = 0, tot = 0;
        for (int j = 1; j < c.nconv; ++j) {
            const size_t n = rup((long)plan.B * c.C[j] * c.K[j] * c.C[j - 1] * 2, 256);
            if (j < i) off += n;
            tot += n;
        }
        if (convwt.alloc(2 * tot)) drop_graph();
        return reinterpret_cast<char*>(convwt.p) + native * tot + off;
    }
    // with bf16 planes, fp32 activations read only as a frozen linear's A operand are not written (the linear
    // reads the plane; no weight gradient reads them): stable-LN outputs, gelu(FFN1), dU.  Only where every
    // producer and consumer takes its plane path (the vectorised LayerNorm widths, K % 8 == 0).  One predicate
    // for the forward and the backward.
    bool fp32_acts_dead() const { return use_planes() && ln_vec_width(c.H) && c.F % 8 == 0; }
    // ---- LayerNorm sites: each LayerNorm described once, for forward() and backward() alike (parameters and their
    // gradients at the same offsets of P and G; which statistics a site keeps: see Plan) ----
    LnSite ln_site(long og, long ob, int rows_per_utt, int D, float eps, bool gelu, float* xhat, float* mean,
                   float* rstd) const {
        return {P + og, P + ob, G + og, G + ob, Pn, Pn, rows_per_utt, plan.B, D, eps, gelu, xhat, mean, rstd};
    }
    LnSite conv_ln(int i) const {  // layer mode: GELU follows
        return ln_site(o_cg[i], o_cbeta[i], plan.Lc[i], c.C[i], 1e-5f, true, nullptr, plan.cmean[i], plan.crstd[i]);
    }
    LnSite feat_proj_ln() const {
        return ln_site(o_fpg, o_fpb, plan.T, c.C[c.nconv - 1], c.eps, false, nullptr, plan.fp_mean, plan.fp_rstd);
    }
    LnSite encoder_ln() const { return ln_site(o_eg, o_eb, plan.T, c.H, c.eps, false, nullptr, plan.enc_mean, plan.enc_rstd); }
    LnSite layer_ln(int l, int which) const {
        const LayerBufs& lb = plan.lay[l];
        return which == 1 ? ln_site(o_l1g[l], o_l1b[l], plan.T, c.H, c.eps, false, lb.xhat1, lb.mean1, lb.rstd1)
                          : ln_site(o_l2g[l], o_l2b[l], plan.T, c.H, c.eps, false, lb.xhat2, lb.mean2, lb.rstd2);
    }
    // conv i's output z_i, the conv LayerNorm's input: bf16 in place in its fp32 buffer with conv_z_bf16()
    LnIn conv_z(int i) const { return conv_z_bf16() ? ln_bf16(plan.z[i]) : ln_f32(plan.z[i]); }
    // a backward on the engine's partial-sum buffer; x: the LayerNorm's stored input (sites without x-hat)
    LnBwd ln_bwd(LnIn dy, LnOut dx, LnIn x = {}, const float* resid = nullptr) const {
        return {dy, x, /*post_aux*/ nullptr, resid, dx, plan.lnpart, plan.lnpart_floats, /*conv*/ nullptr};
    }
    // bf16 mode with planes: the FFN pre-activation u (stored by FFN1, read by the FFN2 input gradient's gelu')
    // kept in bf16 (SUTA_PRE_BF16=0: fp32, for A/B runs)
    bool pre_bf16() const {
        return use_planes() && suta_switches().pre_bf16;
    }
    // layer-mode conv stack on bf16 planes: the conv outputs z_i (conv0's by conv0_vec, the others by the conv GEMMs'
    // epilogues) and the activation gradients da_i (the conv input-gradient GEMMs) stored in bf16 only, in place in
    // their fp32 buffers; the conv LayerNorms read them widened -- torch autocast's bf16 conv outputs and gradients,
    // about half the conv stack's LayerNorm bytes (SUTA_CONV_Z_BF16=0: fp32 storage, for A/B runs)
    bool conv_z_bf16() const {
        if (!conv_planes() || !conv_dx_planes() || !fused_conv_ln() || c.K[0] != 10 || c.S[0] != 5) return false;
        return suta_switches().conv_z_bf16 != 0;
    }
    // stable-LN layers: the input gradients of QKV and FFN1 (the dy of LN1 / LN2 backward) written by their GEMMs as a
    // bf16 plane only (plane 2) and read so by the LayerNorm backward -- torch autocast's bf16 matmul gradient; 104 MB
    // less written and read per LayerNorm backward on C4 (SUTA_DY_PLANES=0: fp32 dy, for A/B runs)
    bool dy_planes() const {
        return fp32_acts_dead() && c.stable && suta_switches().dy_planes;
    }
    // conv input gradients on the bf16 planes too (SUTA_CONV_DX_PLANES=0: fp32-staged x6 kernels, for A/B runs)
    bool conv_dx_planes() const {
        return conv_planes() && suta_switches().conv_dx_planes;
    }
    // bf16 plane of layer l's qkv [B*T][3H], or null: written by the QKV GEMM, read by the flash forward and, in the
    // backward, by the flash backward (kept for every layer, like the fp32 qkv).  Only the head-dim-64 flash kernels
    // read planes (head dims above 64 read fp32 rows).
    // (The forward used to ask `flash && d == 64`, the backward `flash && plane(0) && d == 64`: the same, since
    // plane(0) and this plane are both null exactly when use_planes() is false.)
    DevBuf qkvplanes;
    void* qkv_plane(int l) {
        if (!plan.flash || c.H / c.NH != 64 || !use_planes() || c.H % 8) return nullptr;
        const size_t per = rup((long)plan.B * plan.T * 3 * c.H * 2, 256);
        if (qkvplanes.alloc(per * c.L)) drop_graph();
        return reinterpret_cast<char*>(qkvplanes.p) + l * per;
    }
    // dctx's bf16 plane (the flash backward's dO operand), or null: given exactly when the qkv planes are
    void* dctx_plane() { return qkv_plane(0) ? plane(2) : nullptr; }
    // the flash forward / backward of this call read their bf16 planes: the launches' own tests (ops.h), so the byte
    // counts and the launches cannot disagree
    bool flash_fwd_on_plane() { return flash_fwd_reads_plane(bf16_mode(), qkv_plane(0), c.H, c.H / c.NH); }
    bool flash_bwd_on_planes() {
        return flash_bwd_reads_planes(bf16_mode(), qkv_plane(0), dctx_plane(), c.H, c.H / c.NH);
    }
    // the fp32 qkv of this call is not written: both flash kernels read its bf16 plane only.  One predicate for the
    // QKV GEMM, the flash forward and the flash backward.
    // (The forward used to write `qkvp && P0 && fwd_reads(qkvp) && bwd_reads(qkvp, plane(2))`, the backward
    // `qkvp && fwd_reads(qkvp) && bwd_reads(qkvp, dctxp)`: qkvp non-null implies P0, both tests are false on a null
    // qkvp, and dctxp is plane(2) whenever qkvp is non-null -- the same value in every configuration.)
    bool qkv_fp32_dead() { return flash_fwd_on_plane() && flash_bwd_on_planes(); }
    // positional conv on its dedicated kernel instead of the conv-A GEMM, forward and backward alike: exact fp32 mode,
    // group widths 48 / 64 ...
    bool posconv_fp32_kernel() const {
        return posconv_kernel && gemm_mode == SUTA_PRECISION_FP32_MFMA && (c.H / c.posG == 48 || c.H / c.posG == 64) &&
               c.posK % 2 == 0;
    }
    // ... or bf16 mode, group width 64 (config C4): posconv_bf16_kernel (its forward and flipped-tap backward weights
    // wpos_bf_f / wpos_bf_b are built together)
    bool posconv_bf16() const { return posconv_kernel && bf16_mode() && wpos_bf_f && wpos_bf_b && c.posK % 4 == 0; }
    // The stack's convs on the same kernel (its epilogue-free form, any kernel size): exact fp32 mode, group widths
    // 48 / 64.  Every other mode and width runs them on the mode's conv-A GEMM; LayerNorm and GELU are fp32 always.
    bool stack_on_kernel() const {
        return posconv_kernel && gemm_mode == SUTA_PRECISION_FP32_MFMA && (c.H / c.posG == 48 || c.H / c.posG == 64);
    }
    // One conv of the stack.  fwd: out = conv_j(in) + bias_j; bwd: out = conv_j^T(in) (+ res), rows at or past the
    // utterance's length written as 0.  Input rows at or past the length read as zero in both.
    void stack_conv(bool fwd, int j, const float* in, const float* res, float* out) {
        const int Cg = c.H / c.posG, Kp = posconv_stack_taps(c.posK);
        const float* w = fwd ? wstk_f[j] : wstk_b[j];
        if (stack_on_kernel()) {
            // input window and output once (+ residual), the layer's weights once
            const double bytes = 4.0 * ((double)plan.B * plan.T * c.H * (res ? 3 : 2) + (double)c.posK * Cg * c.H);
            timed(F_GEMM, [&] {
                if (!launch_posconv_stack(fwd, in, w, fwd ? bstk[j] : nullptr, res, out, plan.B, plan.T, c.H, c.posG,
                                          c.posK, rT(), st))
                    throw SutaError(SUTA_ERR_UNSUPPORTED, "positional conv shape");
            }, timing ? bytes : 0.0);
            return;
        }
        auto group = [&](const float* p) { return Mat{p, c.H, Cg, (long)plan.T * c.H}; };
        GemmParams g = batched(plan.T, Cg, c.posK * Cg, group(in), 0, {w, Cg, (long)Kp * Cg * Cg, 0}, 0, group(out),
                               plan.B * c.posG, c.posG);
        g.segK = Cg;
        g.pad = fwd ? c.posK / 2 : c.posK - 1 - c.posK / 2;
        g.Mvalid = plan.T;
        g.zmvalid = rT();
        if (res) add_resid(g, group(res));
        if (fwd) add_bias(g, bstk[j], Cg);
        else if (plan.ragged) {
            g.epi |= EPI_ROWMASK;
            g.zrows = rT();
        }
        gemm(g);
    }
    void build_weight_planes();
    // Where the bf16 planes of a GEMM's operands come from.  resolve_planes() sets the engine's precision mode in p
    // and routes the frozen weight's plane; it changes nothing else and launches nothing.
    enum Planes {
        CALLER_PLANES,   // both planes given by the caller (conv stack)
        PRODUCER_PLANE,  // linear with a frozen weight: the weight's plane, and A's plane written by A's producer
        CONVERT_A,       // the same, but A's plane is yet to be converted from the fp32 A (gemm() does, into abuf)
        PLANELESS,       // fp32 operands (a plane given for a non-frozen B is ignored)
    };
    Planes resolve_planes(GemmParams& p) {
        p.mode = gemm_mode;
        if (bf16_mode() && p.Ab && p.Bb) return CALLER_PLANES;
        if (bf16_mode() && p.segK == 0 && !p.ta && p.Z == 1 && p.K % 8 == 0 && p.lda % 4 == 0 &&
            (reinterpret_cast<uintptr_t>(p.A) & 15) == 0) {
            auto it = wplanes.find(p.B);
            if (it != wplanes.end() && (p.tb ? p.ldb == p.K : p.ldb == p.N)) {
                p.Bb = p.tb ? it->second.first : it->second.second;
                p.ldbb = p.K;
                return p.Ab ? PRODUCER_PLANE : CONVERT_A;
            }
        }
        p.Ab = nullptr;
        return PLANELESS;
    }
    // whether gemm(p0) takes the 256 x 256 bf16-plane kernel's C^T epilogue (the producer's A plane given, B a frozen
    // weight with planes): the condition for fusing EPI_DELTA into it
    bool routes_to_hbx_t(const GemmParams& p0) {
        GemmParams p = p0;
        return p.Ab && resolve_planes(p) == PRODUCER_PLANE && gemm_hbx_t_selected(p);
    }
    void gemm(const GemmParams& p0) {
        GemmParams p = p0;
        const Planes planes = resolve_planes(p);
        gemm_shape.clear();
        if (timing && gemm_census_is_on()) {  // per-shape time table (census + timing: tools/gemm_shapes.py)
            char key[200];
            snprintf(key, sizeof key, "M=%d N=%d K=%d z=%d %s%s epi=%d%s%s%s%s", p.M, p.N, p.K, p.Z, p.ta ? "T" : "N",
                     p.tb ? "T" : "N", p.epi, p.segK > 0 ? " conv" : "", p0.Ab ? " Ab" : "", p.C ? " C" : "",
                     p.Cb ? " Cb" : "");
            gemm_shape = key;
        }
        if (planes == CONVERT_A) {
            if (!p.A) throw SutaError(SUTA_ERR_UNSUPPORTED, "gemm: neither an fp32 A nor its bf16 plane");
            if (abuf.alloc((size_t)p.M * p.K * 2 + 256)) drop_graph();
            p.Ab = abuf.p;
            p.ldab = p.K;
        } else if (planes == PLANELESS) {
            if (!p.C) throw SutaError(SUTA_ERR_UNSUPPORTED, "gemm: fp32 output skipped on a plane-less GEMM");
            if (!p.A) throw SutaError(SUTA_ERR_UNSUPPORTED, "gemm: fp32 A not written (bf16-plane producer) on a plane-less GEMM");
            if (p.Cb) throw SutaError(SUTA_ERR_UNSUPPORTED, "gemm: a bf16 C plane (read by the next kernel) requested on a plane-less GEMM");
        }
        timed(F_GEMM, [&] {
            if (planes == CONVERT_A) launch_to_bf16(p.A, p.lda, p.M, p.K, abuf.p, st);
            gemm_launch(p, st, plan.splitws, plan.splitws_floats);
        }, timing ? gemm_alg_bytes(p, planes == CONVERT_A) : 0.0);
    }

    // one GEMM per utterance (trainable per-slot weights, conv layers): operands by utt()
    GemmParams per_utt(int M, int N, int K, Mat A, int ta, Mat B, int tb, Mat C) const {
        return batched(M, N, K, A, ta, B, tb, C, plan.B, 1);
    }
    // one GEMM per (utterance, head) of the unfused attention, on these three operand views:
    // head h's d columns of a [B*T][3H] qkv buffer (p: qkv for Q, + H for K, + 2H for V; dqkv alike),
    Mat head_qkv(const float* p) const { return {p, 3L * c.H, c.H / c.NH, (long)plan.T * 3 * c.H}; }
    // its d columns of a [B*T][H] buffer (ctx, dctx),
    Mat head_rows(const float* p) const { return {p, c.H, c.H / c.NH, (long)plan.T * c.H}; }
    // and its T x Tp score matrix (P, dP)
    Mat head_scores(const float* p) const { return {p, plan.Tp, (long)plan.T * plan.Tp, (long)c.NH * plan.T * plan.Tp}; }
    GemmParams per_head(int M, int N, int K, Mat A, int ta, Mat B, int tb, Mat C) const {
        return batched(M, N, K, A, ta, B, tb, C, plan.B * c.NH, c.NH);
    }
    // The positional conv as a conv-A GEMM per (utterance, group): out = conv(in, w; pad) + res, w [G][posK][Cg][Cg],
    // zero padding at each utterance's own end.  The forward (bias, pre given) computes
    // pre = conv + bias, out = gelu(pre) + res; the backward (flipped taps) adds its row mask itself.
    GemmParams posconv_gemm(const float* in, const float* w, int pad, float* out, const float* res,
                            const float* bias = nullptr, float* pre = nullptr) const {
        const int Cg = c.H / c.posG;
        auto group = [&](const float* p) { return Mat{p, c.H, Cg, (long)plan.T * c.H}; };
        GemmParams g = batched(plan.T, Cg, c.posK * Cg, group(in), 0, {w, Cg, (long)c.posK * Cg * Cg, 0}, 0, group(out),
                               plan.B * c.posG, c.posG);
        g.segK = Cg;
        g.pad = pad;
        g.Mvalid = plan.T;
        g.zmvalid = rT();
        add_resid(g, group(res));
        if (bias) {
            add_bias(g, bias, Cg);
            store_pre(g, group(pre));
            g.epi |= EPI_GELU;
        }
        return g;
    }

    int multiplicity(const TP& t, int train_feature, int bias_only) const {
        int k = 0;
        if (t.ln_member && (!bias_only || t.is_bias)) k += 1;
        if (train_feature) k += t.feat_depth;
        return k;
    }

    void build_plan(int B, long N);
    void set_lengths(int B, const int64_t* ns);
    const int* rN() const { return plan.ragged ? plan.len_n : nullptr; }
    const int* rL0() const { return plan.ragged ? plan.len_L0 : nullptr; }
    const int* rT() const { return plan.ragged ? plan.len_T : nullptr; }
    void forward(int B);
    void backward(int B, const suta_hparams& hp);
    void adam(int B, const suta_hparams& hp);
    void reset_slots(int B, bool zero_moments);
    void stage_input(const float* wav, int on_dev, int norm, int B, long N, long stride = 0);
};

suta_engine::~suta_engine() {
    if (loop_graph) (void)hipGraphExecDestroy(loop_graph);
    if (d_adam_tab) (void)hipFree(d_adam_tab);
    if (pl_buf) (void)hipFree(pl_buf);
    for (float* p : owned) (void)hipFree(p);
    for (auto& pe : pending) {
        (void)hipEventDestroy(pe.second.first);
        (void)hipEventDestroy(pe.second.second);
    }
    for (auto e : evpool) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
}

// ----------------------------------------------------------------------------------------------
// workspace plan
// ----------------------------------------------------------------------------------------------
void suta_engine::build_plan(int B, long N) {
    if (plan.B == B && plan.N == N) return;
    drop_graph();
    const Cfg& k = c;
    Plan pl;
    pl.B = B;
    pl.N = N;
    long L = N;
    for (int i = 0; i < k.nconv; ++i) {
        // (a conv input shorter than its kernel has no output frame: torch's Conv1d raises; C division would
        // round (L - K) / S toward zero and report one frame)
        if (L < k.K[i]) throw SutaError(SUTA_ERR_ARG, "utterance too short for the conv feature encoder");
        L = (L - k.K[i]) / k.S[i] + 1;
        pl.Lc[i] = (int)L;
    }
    pl.T = pl.Lc[k.nconv - 1];
    pl.Tp = (int)rup(pl.T, 4);
    if (pl.T > 2048) throw SutaError(SUTA_ERR_UNSUPPORTED, "T > 2048 frames (max 600000 samples in the reference)");
    const long T = pl.T, H = k.H, BT = (long)B * T;
    long maxLC = 0;
    for (int i = 0; i < k.nconv; ++i) maxLC = std::max(maxLC, (long)pl.Lc[i] * k.C[i]);
    for (int pass = 0; pass < 2; ++pass) {
        Arena ar;
        ar.dry = pass == 0;
        ar.base = reinterpret_cast<char*>(ws.p);
        pl.xraw = ar.take<float>((size_t)B * N);
        pl.x = ar.take<float>((size_t)B * N);
        for (int i = 0; i < k.nconv; ++i) {
            const long n = (long)B * pl.Lc[i] * k.C[i];
            pl.z[i] = (i == 0 && !k.layer_mode) ? nullptr : ar.take<float>(n);  // group-mode conv0 is recomputed
            pl.a[i] = ar.take<float>(n);
            if (k.layer_mode) {
                pl.crstd[i] = ar.take<float>((size_t)B * pl.Lc[i]);
                pl.cmean[i] = ar.take<float>((size_t)B * pl.Lc[i]);
            } else {
                pl.crstd[i] = pl.cmean[i] = nullptr;
            }
        }
        pl.gn_mean = ar.take<float>((size_t)B * k.C[0]);
        pl.gn_rstd = ar.take<float>((size_t)B * k.C[0]);
        const long C6 = k.C[k.nconv - 1];
        pl.fp_mean = ar.take<float>(BT);
        pl.fp_rstd = ar.take<float>(BT);
        pl.fp_y = ar.take<float>(BT * C6);
        pl.h0 = ar.take<float>(BT * H);
        pl.pz = k.posD ? nullptr : ar.take<float>(BT * H);
        for (int j = 0; j < MAX_POS_STACK; ++j) {
            const bool on = j < k.posD;
            pl.stk_z[j] = on ? ar.take<float>(BT * H) : nullptr;
            pl.stk_mean[j] = on ? ar.take<float>(BT) : nullptr;
            pl.stk_rstd[j] = on ? ar.take<float>(BT) : nullptr;
        }
        for (int j = 0; j < 2; ++j) pl.stk_a[j] = k.posD > 1 ? ar.take<float>(BT * H) : nullptr;
        pl.e = ar.take<float>(BT * H);
        pl.enc_mean = ar.take<float>(BT);
        pl.enc_rstd = ar.take<float>(BT);
        pl.enc_y = ar.take<float>(BT * H);
        pl.lay.assign(k.L, LayerBufs{});
        pl.flash = attn_fused && flash_dh_ok(k.H / k.NH);
        const long Psz = pl.flash ? 0 : (long)B * k.NH * T * pl.Tp;
        for (int l = 0; l < k.L; ++l) {
            LayerBufs& lb = pl.lay[l];
            lb.xhat1 = k.stable ? nullptr : ar.take<float>(BT * H);
            lb.mean1 = k.stable ? ar.take<float>(BT) : nullptr;
            lb.rstd1 = ar.take<float>(BT);
            lb.y1 = ar.take<float>(BT * H);
            lb.qkv = ar.take<float>(BT * 3 * H);
            lb.P = pl.flash ? nullptr : ar.take<float>(Psz);
            lb.lse = pl.flash ? ar.take<float>((size_t)B * k.NH * T) : nullptr;
            lb.ctx = ar.take<float>(BT * H);
            lb.hmid = k.stable ? ar.take<float>(BT * H) : nullptr;
            lb.xhat2 = k.stable ? nullptr : ar.take<float>(BT * H);
            lb.mean2 = k.stable ? ar.take<float>(BT) : nullptr;
            lb.rstd2 = ar.take<float>(BT);
            lb.y2 = k.stable ? ar.take<float>(BT * H) : nullptr;
            lb.u = ar.take<float>(BT * k.F);
            lb.x_out = ar.take<float>(BT * H);
            const bool ad = k.stable && k.A > 0;
            lb.ad_in = ad ? ar.take<float>(BT * H) : nullptr;
            lb.ad_mean = ad ? ar.take<float>(BT) : nullptr;
            lb.ad_rstd = ad ? ar.take<float>(BT) : nullptr;
        }
        for (int l = 0; l < k.L; ++l) {
            pl.lay[l].x_in = l == 0 ? (k.stable ? pl.e : pl.enc_y) : pl.lay[l - 1].x_out;
            if (!k.stable) pl.lay[l].y2 = pl.lay[l].x_out;
        }
        pl.ctx = ar.take<float>(BT * H);
        pl.gu = ar.take<float>(BT * k.F);
        pl.rtmp = ar.take<float>(BT * H);
        pl.logits = ar.take<float>(BT * k.V);
        pl.dlogits = ar.take<float>(BT * k.V);
        pl.d1 = ar.take<float>(BT * H);
        pl.d2 = ar.take<float>(BT * H);
        pl.d3 = ar.take<float>(BT * H);
        pl.dqkv = ar.take<float>(BT * 3 * H);
        pl.dP = pl.flash ? nullptr : ar.take<float>(Psz);
        pl.dqp = pl.flash ? ar.take<float>(flash_dq_scratch_floats(B, pl.T, k.NH, k.H / k.NH)) : nullptr;
        pl.delta = ar.take<float>((size_t)B * k.NH * T);
        pl.du = ar.take<float>(BT * k.F);
        pl.dzc = ar.take<float>((size_t)B * maxLC);
        pl.dzc2 = ar.take<float>((size_t)B * maxLC);
        const long lnrows = std::max<long>(pl.Lc[0], T);
        pl.lnpart_floats = (long)B * ((lnrows + 15) / 16) * 2 * std::max<long>(H, maxLC / pl.Lc[0] + 1) + 64;
        if (k.layer_mode && k.C[0] == 512)  // the fused conv LayerNorm backwards' partial slabs (short inputs too)
            for (int i = 0; i < k.nconv; ++i)
                pl.lnpart_floats = std::max(pl.lnpart_floats,
                                            layernorm_bwd_conv_part_floats(B, pl.Lc[i], k.C[i], i == 0 ? 10 : 0));
        if (k.stable && k.A > 0) pl.lnpart_floats = std::max(pl.lnpart_floats, adapter_part_floats(B, T, H));
        pl.lnpart = ar.take<float>((size_t)pl.lnpart_floats);
        pl.dpart = ar.take<double>((size_t)B * ((pl.Lc[0] + 127) / 128 + 2) * 2 * k.C[0] + (size_t)B * k.C[0] * 2);
        pl.c0part = ar.take<float>((size_t)B * ((pl.Lc[0] + 127) / 128) * k.K[0] * k.C[0] + 64);
        pl.loss = ar.take<float>(B);
        pl.loss_scratch = ar.take<float>(suta_loss_scratch_floats(B, T, k.V));  // either loss path (ops.h)
        pl.ids = ar.take<int>((size_t)BT);
        pl.len_n = ar.take<int>((size_t)B);
        pl.len_L0 = ar.take<int>((size_t)B);
        pl.len_T = ar.take<int>((size_t)B);
        pl.splitws_floats = 32L << 20;
        pl.splitws = ar.take<float>(pl.splitws_floats);
        pl.bytes = ar.off;
        // a fresh workspace starts zeroed (on the engine stream, ordered before any use): the padding
        // frames of ragged batches must hold finite values
        if (pass == 0 && ws.alloc(ar.off + 256)) HIPCHK(hipMemsetAsync(ws.p, 0, ws.bytes, st));
    }
    plan = pl;
}

// Per-utterance lengths of a ragged batch (null: every utterance has the layout length plan.N).
void suta_engine::set_lengths(int B, const int64_t* ns) {
    Plan& pl = plan;
    pl.ragged = false;
    pl.h_n.assign(B, (int)pl.N);
    pl.h_T.assign(B, pl.T);
    if (!ns) return;
    std::vector<int> l0(B);
    for (int b = 0; b < B; ++b) {
        if (ns[b] < 1 || ns[b] > pl.N) throw SutaError(SUTA_ERR_ARG, "n_samples[b] outside [1, layout length]");
        long L = ns[b];
        for (int i = 0; i < c.nconv; ++i) {
            if (L < c.K[i]) throw SutaError(SUTA_ERR_ARG, "utterance too short for the conv feature encoder");
            L = (L - c.K[i]) / c.S[i] + 1;
            if (i == 0) l0[b] = (int)L;
        }
        pl.h_n[b] = (int)ns[b];
        pl.h_T[b] = (int)L;
        if (ns[b] != pl.N) pl.ragged = true;
    }
    if (!pl.ragged) return;
    HIPCHK(hipMemcpyAsync(pl.len_n, pl.h_n.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pl.len_L0, l0.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pl.len_T, pl.h_T.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // host vectors are pageable and reused
}

// ----------------------------------------------------------------------------------------------
// forward (saves everything the backward needs)
// ----------------------------------------------------------------------------------------------
void suta_engine::forward(int B) {
    const Cfg& k = c;
    Plan& pl = plan;
    const int T = pl.T, H = k.H, NH = k.NH, d = H / NH;
    const long BT = (long)B * T;
    if (!k.layer_mode) {
        // conv0 + GroupNorm + GELU, conv0 recomputed in each pass (never stored)
        timed(F_FRONT, [&] {
            launch_front_gn_fwd(pl.x, pl.N, P + o_cw[0], k.conv_bias ? P + o_cb[0] : nullptr, Pn, B, pl.Lc[0], k.C[0],
                                k.K[0], k.S[0], P + o_cg[0], P + o_cbeta[0], pl.gn_mean, pl.gn_rstd, pl.a[0],
                                pl.dpart, rL0(), st);
        }, 4.0 * B * ((double)pl.N + (double)pl.Lc[0] * k.C[0]));  // waveform read, activation written
    }
    const bool zbf = k.layer_mode && conv_z_bf16();  // z_i in bf16, in place in the fp32 buffers
    if (k.layer_mode) {
        timed(F_FRONT, [&] {
            launch_conv0(pl.x, pl.N, P + o_cw[0], k.conv_bias ? P + o_cb[0] : nullptr, Pn, pl.z[0], B, pl.Lc[0],
                         k.C[0], k.K[0], k.S[0], st, zbf ? pl.z[0] : nullptr);
        }, (zbf ? 2.0 : 4.0) * B * ((double)pl.N + (double)pl.Lc[0] * k.C[0]));
    }
    const bool cpl = conv_planes();
    if (k.layer_mode) {
        timed(F_NORM, [&] {
            // with conv planes only the bf16 activation is read (the next conv GEMM and its weight gradient)
            ln_forward(conv_ln(0), {conv_z(0), cpl ? ln_plane(conv_act_plane(0)) : ln_out(pl.a[0])}, st);
        });
    }
    for (int i = 1; i < k.nconv; ++i) {
        // conv_i(a_{i-1}) as a strided-row GEMM: row t of A is the K_i * C_{i-1} inputs from frame S_i * t on.
        // Layer mode stores z_i (LayerNorm and GELU follow); group mode stores z_i as the pre-activation and a_i.
        // (bf16 planes: the per-slot weights are re-laid [C_i][K_i * C_{i-1}], one such block per utterance)
        const int Kc = k.K[i] * k.C[i - 1], Ci = k.C[i];
        const long zi = (long)pl.Lc[i] * Ci;  // elements of one utterance's z_i / a_i
        float* out = !k.layer_mode ? pl.a[i] : zbf ? nullptr : pl.z[i];
        GemmParams g = per_utt(pl.Lc[i], Ci, Kc, utt(pl.a[i - 1], (long)k.S[i] * k.C[i - 1], (long)pl.Lc[i - 1] * k.C[i - 1]),
                               0, utt(P + o_cw[i], Ci, cpl ? (long)Ci * Kc : Pn), 0, utt(out, Ci, zi));
        if (cpl) {  // bf16 planes: activations written by the previous LayerNorm, weights re-laid per slot
            void* wt = conv_wt_plane(i);
            timed(F_EW, [&] {
                launch_transpose_bf16(P + o_cw[i], Pn, B, Kc, Ci, wt, st, conv_dx_planes() ? conv_wt_plane(i, 1) : nullptr);
            });
            // (the activation plane has the fp32 buffer's element strides)
            set_planes(g, conv_act_plane(i - 1), g.lda, wt, Kc);
        }
        if (k.conv_bias) add_bias(g, P + o_cb[i], 0, Pn);
        if (!k.layer_mode) {
            store_pre(g, utt(pl.z[i], Ci, zi));
            g.epi |= EPI_GELU;
            gemm(g);
        } else {
            if (zbf) set_c_plane(g, pl.z[i], Ci, zi);  // bf16 z_i only (the LayerNorm forward and backward read it widened)
            gemm(g);
            timed(F_NORM, [&] {
                const bool pln = cpl && i + 1 < k.nconv;
                ln_forward(conv_ln(i), {conv_z(i), pln ? ln_plane(conv_act_plane(i)) : ln_out(pl.a[i])}, st);
            });
        }
    }
    const int C6 = k.C[k.nconv - 1];
    const float* feat = pl.a[k.nconv - 1];
    timed(F_NORM, [&] { ln_forward(feat_proj_ln(), {ln_f32(feat), ln_out(pl.fp_y)}, st); });
    {  // projection (per-utterance trainable W, b)
        GemmParams g = per_utt(T, H, C6, utt(pl.fp_y, C6, (long)T * C6), 0, utt(P + o_pw, C6, Pn), 1, utt(pl.h0, H, (long)T * H));
        add_bias(g, P + o_pb, 0, Pn);
        gemm(g);
    }
    // data2vec-audio: e = h0 + stack(h0), a layer = conv + bias -> LayerNorm(no affine) -> GELU; z_j and the row
    // statistics stay for the backward, the last layer's row kernel adds h0
    if (k.posD) {
        const float* in = pl.h0;
        for (int j = 0; j < k.posD; ++j) {
            const bool last = j + 1 == k.posD;
            float* out = last ? pl.e : pl.stk_a[j & 1];
            stack_conv(true, j, in, nullptr, pl.stk_z[j]);
            timed(F_NORM, [&] {
                launch_ln_gelu_fwd(pl.stk_z[j], last ? pl.h0 : nullptr, out, pl.stk_mean[j], pl.stk_rstd[j], (int)BT, T,
                                   H, POS_STACK_EPS, rT(), st);
            }, 4.0 * BT * H * (last ? 3 : 2));
            in = out;
        }
    }
    // positional conv: e = h0 + gelu(posconv(h0)); pz = pre-activation
    // dedicated kernel in exact fp32 mode for group widths 48 / 64 (timed with the MFMA contractions)
    else if (posconv_fp32_kernel())
        timed(F_GEMM, [&] {
            if (!launch_posconv(true, pl.h0, wpos_f, bpos, pl.h0, pl.e, pl.pz, B, T, H, k.posG, k.posK, k.posK / 2,
                                rT(), st))
                throw SutaError(SUTA_ERR_UNSUPPORTED, "positional conv shape");
        });
    else if (posconv_bf16())
        timed(F_GEMM, [&] {
            if (!launch_posconv_bf16(true, pl.h0, wpos_bf_f, bpos, pl.h0, pl.e, pl.pz, B, T, H, k.posG, k.posK,
                                     k.posK / 2, rT(), st))
                throw SutaError(SUTA_ERR_UNSUPPORTED, "positional conv shape");
        });
    else
        gemm(posconv_gemm(pl.h0, wpos_f, k.posK / 2, pl.e, pl.h0, bpos, pl.pz));
    if (!k.stable) timed(F_NORM, [&] { ln_forward(encoder_ln(), {ln_f32(pl.e), ln_out(pl.enc_y, plane(0))}, st); });
    const float scale = 1.0f / std::sqrt((float)d);
    // bf16 mode: producers of the linears' A operands also write bf16 planes (P0 / P1, ping-pong)
    void* P0 = plane(0);
    void* P1 = plane(1);
    const bool dead = fp32_acts_dead();  // (P0 non-null exactly then)
    float* gu32 = dead ? nullptr : pl.gu;
    for (int l = 0; l < k.L; ++l) {
        LayerBufs& lb = pl.lay[l];
        const float* attn_in = lb.x_in;
        if (k.stable) {
            timed(F_NORM, [&] { ln_forward(layer_ln(l, 1), {ln_f32(lb.x_in), ln_out(dead ? nullptr : lb.y1, P0)}, st); });
            attn_in = dead ? nullptr : lb.y1;  // (dead: the QKV GEMM reads the LN1 plane only)
        }
        void* qkvp = qkv_plane(l);  // the flash kernels' operands
        // both flash kernels read qkv's bf16 plane only (the backward's dO plane is plane 2): no fp32 qkv
        float* qkv32 = qkv_fp32_dead() ? nullptr : lb.qkv;
        {  // fused QKV (A plane: the LN output's -- stable: LN1; post-LN: the previous LayerNorm)
            GemmParams g = linear(attn_in, P0, wqkv[l], 1, qkv32, qkvp, (int)BT, 3 * H, H);
            add_bias(g, bqkv[l]);
            gemm(g);
        }
        // flash attention (head dim 64 or 72 .. 128, any T): ctx and the per-row LSE, no T x T matrix
        const bool fused = pl.flash;
        if (fused)
            timed(F_ATTN, [&] {
                if (!launch_flash_fwd(qkv32, lb.ctx, lb.lse, B, T, NH, H, d, scale, rT(), bf16_mode(), st, P0, qkvp))
                    throw SutaError(SUTA_ERR_UNSUPPORTED, "flash attention shape");
            }, (double)BT * ((flash_fwd_on_plane() ? 2.0 : 4.0) * 3.0 * H + 4.0 * H + (P0 && bf16_mode() ? 2.0 * H : 0.0) +
                            4.0 * NH));  // Q, K, V read; ctx (+ plane), LSE written
        if (!fused) {
            {  // S = Q K^T * scale
                GemmParams g = per_head(T, T, d, head_qkv(lb.qkv), 0, head_qkv(lb.qkv + H), 1, head_scores(lb.P));
                g.alpha = scale;
                gemm(g);
            }
            timed(F_SOFTMAX, [&] { launch_softmax_rows(lb.P, (long)B * NH * T, T, pl.Tp, rT(), (long)NH * T, st); });
            // ctx = P V
            gemm(per_head(T, d, T, head_scores(lb.P), 0, head_qkv(lb.qkv + 2 * H), 0, head_rows(lb.ctx)));
        }
        {  // out projection + residual (the flash forward wrote ctx's plane)
            GemmParams g = linear(lb.ctx, fused ? P0 : nullptr, wo[l], 1, k.stable ? lb.hmid : pl.rtmp, nullptr, (int)BT, H, H);
            add_bias(g, bo[l]);
            add_resid(g, {lb.x_in, H});
            gemm(g);
        }
        const float* ffn_in;
        const float* ffn_res;
        float* ffn_out;
        if (k.stable) {
            timed(F_NORM, [&] { ln_forward(layer_ln(l, 2), {ln_f32(lb.hmid), ln_out(dead ? nullptr : lb.y2, P0)}, st); });
            ffn_in = dead ? nullptr : lb.y2;
            ffn_res = lb.hmid;
            ffn_out = k.A > 0 ? lb.ad_in : lb.x_out;  // (the adapter kernel writes x_out)
        } else {
            timed(F_NORM, [&] { ln_forward(layer_ln(l, 1), {ln_f32(pl.rtmp), ln_out(lb.y1, P0)}, st); });
            ffn_in = lb.y1;
            ffn_res = lb.y1;
            ffn_out = pl.rtmp;
        }
        {  // u = in W1^T + b1 (stored), gu = gelu(u)
            // with planes FFN2 reads only gelu(u)'s bf16 plane P1 (no weight gradient): no fp32 gu
            GemmParams g = linear(ffn_in, P0, w1[l], 1, gu32, P1, (int)BT, k.F, H);
            add_bias(g, b1[l]);
            store_pre(g, {lb.u, k.F});  // (dead: bf16 elements, the first half of the fp32 buffer)
            g.preb = dead && pre_bf16();
            g.epi |= EPI_GELU;
            gemm(g);
        }
        {  // out = gu W2^T + b2 + residual
            GemmParams g = linear(gu32, P1, w2[l], 1, ffn_out, nullptr, (int)BT, H, k.F);
            add_bias(g, b2[l]);
            add_resid(g, {ffn_res, H});
            gemm(g);
        }
        if (k.stable && k.A > 0)  // x_out = h + adapter(h): h read once, the sum written once
            timed(F_NORM, [&] {
                launch_adapter_fwd(lb.ad_in, P + o_adg[l], P + o_adb[l], Pn, T, B, H, adw[l], 1e-5f, lb.x_out, lb.ad_mean,
                                   lb.ad_rstd, st);
            });
        if (!k.stable) timed(F_NORM, [&] { ln_forward(layer_ln(l, 2), {ln_f32(pl.rtmp), ln_out(lb.x_out, P0)}, st); });
    }
    const float* hfin = pl.lay[k.L - 1].x_out;
    if (k.stable) {
        timed(F_NORM, [&] { ln_forward(encoder_ln(), {ln_f32(hfin), ln_out(dead ? nullptr : pl.enc_y, P0)}, st); });
        hfin = dead ? nullptr : pl.enc_y;
    }
    {  // lm_head
        // (A plane: the final LayerNorm output's -- stable: enc LN; post-LN: the last layer's LN2)
        GemmParams g = linear(hfin, P0, wlm, 1, pl.logits, nullptr, (int)BT, k.V, H);
        add_bias(g, blm);
        gemm(g);
    }
}

// ----------------------------------------------------------------------------------------------
// backward: grads of the trainable tensors into G[b] (fully overwritten for every k > 0 tensor)
// ----------------------------------------------------------------------------------------------
void suta_engine::backward(int B, const suta_hparams& hp) {
    const Cfg& k = c;
    Plan& pl = plan;
    const int T = pl.T, H = k.H, NH = k.NH, d = H / NH;
    const long BT = (long)B * T;
    const float scale = 1.0f / std::sqrt((float)d);
    LossHP lh{hp.temp, hp.em_coef, hp.div_coef, hp.reweight, hp.non_blank};
    timed(F_LOSS,
          [&] { launch_suta_loss(pl.logits, B, T, k.V, lh, rT(), pl.dlogits, pl.loss, pl.loss_scratch, st); });
    if (hp.pl_coef > 0.f) {  // SDPL: (1 - pl) * SUTA + pl * pseudo-label CTC (main_SDPL.py:143-209)
        const long per = sdpl_scratch_floats(T, k.V);
        // [error flag | 63 pad | B x per-utterance scratch]: the flag stays at a fixed offset
        if (sdpl_ws.alloc(((size_t)B * per + 64) * sizeof(float)))
            HIPCHK(hipMemsetAsync(sdpl_ws.p, 0, sdpl_ws.bytes, st));
        int* err = reinterpret_cast<int*>(sdpl_ws.p);
        const SdplTable* tab = sdpl_table();
        timed(F_LOSS, [&] {
            launch_sdpl_loss(pl.logits, B, T, k.V, hp.pl_coef, rT(), pl.dlogits, pl.loss, sdpl_ws.p + 64, err,
                             tab, st);
        });
        sdpl_used = true;
        sdpl_err = err;
    }

    void* P0 = plane(0);  // bf16 planes of the linears' A operands (ping-pong), null outside bf16 mode
    void* P1 = plane(1);
    // with bf16 planes (the forward's condition) dU = dH W2 * gelu'(u) is read only through its plane by the
    // FFN1 input-gradient GEMM (no weight gradient): its fp32 copy is not written
    const bool dead = fp32_acts_dead();
    float* du32 = dead ? nullptr : pl.du;
    // du = (dy @ W2) * gelu'(u) of layer l (u in bf16 where the forward stored it so); dy's plane is P0, du's P1
    auto du_gemm = [&](const float* dy, int l) {
        GemmParams g = linear(dy, P0, w2[l], 0, du32, P1, (int)BT, k.F, H);
        set_aux(g, EPI_DGELU, {pl.lay[l].u, k.F});
        g.preb = dead && pre_bf16();
        gemm(g);
    };
    // d hfin = dlogits @ Wlm
    gemm(linear(pl.dlogits, nullptr, wlm, 0, pl.d1, nullptr, (int)BT, H, k.V));
    float* dx = pl.d1;  // grad wrt current residual stream
    float* t1 = pl.d2;
    float* t2 = pl.d3;
    if (k.stable) {
        timed(F_NORM, [&] {
            ln_backward(encoder_ln(), ln_bwd(ln_f32(dx), ln_out(t1, P0), ln_f32(pl.lay[k.L - 1].x_out)), st);
        });
        std::swap(dx, t1);
    }
    for (int l = k.L - 1; l >= 0; --l) {
        LayerBufs& lb = pl.lay[l];
        float* dhres;  // grad flowing into the attention-block output (residual point)
        if (!k.stable) {
            // dr2 = LN2 bwd(dx)
            timed(F_NORM, [&] { ln_backward(layer_ln(l, 2), ln_bwd(ln_f32(dx), ln_out(t1, P0)), st); });
            // du = (dr2 @ W2) * gelu'(u)
            du_gemm(t1, l);
            {  // dh1 = du @ W1 + dr2
                GemmParams g = linear(du32, P1, w1[l], 0, t2, nullptr, (int)BT, H, k.F);
                add_resid(g, {t1, H});
                gemm(g);
            }
            // dr1 = LN1 bwd(dh1)
            timed(F_NORM, [&] { ln_backward(layer_ln(l, 1), ln_bwd(ln_f32(t2), ln_out(t1, P0)), st); });
            dhres = t1;  // dr1
        } else {
            if (k.A > 0) {  // through the adapter first: dh = dx + adapter-bwd(dx) (its plane P0 for du_gemm)
                timed(F_NORM, [&] {
                    launch_adapter_bwd(lb.ad_in, dx, lb.ad_mean, lb.ad_rstd, P + o_adg[l], P + o_adb[l], Pn, T, B, H,
                                       adw[l], rT(), t1, G + o_adg[l], G + o_adb[l], Pn, pl.lnpart, st, P0);
                });
                std::swap(dx, t1);
            }
            // du = (dx @ W2) * gelu'(u); dy2 = du @ W1; dhmid = LN2 bwd(dy2) + dx
            du_gemm(dx, l);
            void* dyp = dy_planes() ? plane(2) : nullptr;  // (plane 2's dctx of the layer above is consumed)
            gemm(linear(du32, P1, w1[l], 0, dyp ? nullptr : t2, dyp, (int)BT, H, k.F));
            timed(F_NORM, [&] {
                ln_backward(layer_ln(l, 2), ln_bwd(dyp ? ln_bf16(dyp) : ln_f32(t2), ln_out(t1, P0), ln_f32(lb.hmid), dx), st);
            });
            dhres = t1;  // dhmid
        }
        // dctx = dhres @ Wo
        void* dctxp = dctx_plane();  // dO plane of the flash backward
        void* qkvp = qkv_plane(l);
        // softmax-backward row term delta = rowsum(dctx * ctx) per head: in the dctx GEMM's epilogue when it takes the
        // C^T-epilogue kernel and the flash backward reads the dctx plane (the fp32 dctx is then not written), else a
        // separate pass over the fp32 dctx
        bool delta_fused = false;
        if (suta_switches().fused_delta && flash_bwd_on_planes()) {
            GemmParams g = linear(dhres, P0, wo[l], 0, nullptr, dctxp, (int)BT, H, H);
            g.epi = EPI_DELTA;
            g.dlt_o = lb.ctx;
            g.ldo = H;
            g.delta = pl.delta;
            g.dT = T;
            g.dNH = NH;
            if (routes_to_hbx_t(g)) {
                gemm(g);
                delta_fused = true;
            }
        }
        if (!delta_fused) {
            gemm(linear(dhres, P0, wo[l], 0, pl.ctx, dctxp, (int)BT, H, H));
            timed(F_SOFTMAX, [&] { launch_attn_delta(pl.ctx, lb.ctx, pl.delta, B, T, NH, d, st); });
        }
        // flash backward: P recomputed from the LSE, dQ, dK, dV into dqkv (else the GEMM path below)
        const bool fused_bwd = pl.flash;
        // with bf16 planes the QKV input-gradient GEMM reads only dqkv's bf16 plane: the fp32 copy is not written
        float* dqkv32 = (fused_bwd && P1 && dead) ? nullptr : pl.dqkv;
        void* dqkvp = fused_bwd ? P1 : nullptr;  // dqkv's plane, written by the flash backward
        if (fused_bwd) {
            // (the forward's test: the fp32 qkv was not written when both flash kernels read its plane)
            const float* qkv32 = qkv_fp32_dead() ? nullptr : lb.qkv;
            timed(F_ATTN, [&] {
                if (!launch_flash_bwd(qkv32, pl.ctx, lb.lse, pl.delta, dqkv32, pl.dqp, B, T, NH, H, d, scale, rT(),
                                      bf16_mode(), st, P1, qkvp, dctxp))
                    throw SutaError(SUTA_ERR_UNSUPPORTED, "flash attention shape");
            },  // Q, K, V, dO, LSE, delta read; dQ, dK, dV written (fp32 and / or the bf16 plane)
                  (double)BT * ((flash_bwd_on_planes() ? 2.0 : 4.0) * 4.0 * H + 4.0 * 2.0 * NH + (dqkv32 ? 12.0 * H : 0.0) +
                                (P1 && bf16_mode() ? 6.0 * H : 0.0)));
        } else {
            {  // dS = scale * P * (dctx_h @ V_h^T - delta)
                GemmParams g = per_head(T, T, d, head_rows(pl.ctx), 0, head_qkv(lb.qkv + 2 * H), 1, head_scores(pl.dP));
                g.alpha = scale;
                set_aux(g, EPI_SMBWD, head_scores(lb.P));
                set_row_vec(g, pl.delta, T, (long)NH * T);
                gemm(g);
            }
            // dQ = dS K_h
            gemm(per_head(T, d, T, head_scores(pl.dP), 0, head_qkv(lb.qkv + H), 0, head_qkv(pl.dqkv)));
            // dK = dS^T Q_h
            gemm(per_head(T, d, T, head_scores(pl.dP), 1, head_qkv(lb.qkv), 0, head_qkv(pl.dqkv + H)));
            // dV = P^T dctx_h
            gemm(per_head(T, d, T, head_scores(lb.P), 1, head_rows(pl.ctx), 0, head_qkv(pl.dqkv + 2 * H)));
        }
        if (!k.stable) {
            // dx_in = dqkv @ Wqkv + dr1
            GemmParams g = linear(dqkv32, dqkvp, wqkv[l], 0, t2, nullptr, (int)BT, H, 3 * H);
            add_resid(g, {dhres, H});
            gemm(g);
            std::swap(dx, t2);
        } else {
            // dy1 = dqkv @ Wqkv ; dx_in = LN1 bwd(dy1) + dhmid
            // (plane 2 held dctx, consumed by the flash backward above)
            void* dyp = (dy_planes() && dqkvp) ? plane(2) : nullptr;
            gemm(linear(dqkv32, dqkvp, wqkv[l], 0, dyp ? nullptr : t2, dyp, (int)BT, H, 3 * H));
            timed(F_NORM, [&] {
                ln_backward(layer_ln(l, 1), ln_bwd(dyp ? ln_bf16(dyp) : ln_f32(t2), ln_out(dx, P0), ln_f32(lb.x_in), dhres), st);
            });
            // dx now holds grad wrt x_in; t1/t2 free
        }
    }
    // encoder input
    float* de = dx;
    if (!k.stable) {
        timed(F_NORM, [&] { ln_backward(encoder_ln(), ln_bwd(ln_f32(dx), ln_out(t1), ln_f32(pl.e)), st); });
        de = t1;
    }
    // dpz, dh0: the two of d1, d2, d3 that de does not occupy, in cyclic order after de (checked against the nested
    // conditionals this replaces, for de = d1, d2 and d3: the same pair in the same order)
    float *dpz, *dh0;
    if (de == pl.d1) {
        dpz = pl.d2;
        dh0 = pl.d3;
    } else if (de == pl.d2) {
        dpz = pl.d3;
        dh0 = pl.d1;
    } else {
        dpz = pl.d1;
        dh0 = pl.d2;
    }
    if (!k.posD) timed(F_EW, [&] { launch_dgelu_mul(de, pl.pz, dpz, BT * H, st); });
    // dh0 = posconv^T(dpz) + de: the forward's kernel choice, on the flipped taps
    if (k.posD) {
        // data2vec-audio: dz_j = LayerNorm/GELU backward of da_j (da of the last layer = de), da_{j-1} = conv_j^T(dz_j)
        // on the flipped taps; dh0 = conv_0^T(dz_0) + de
        const float* da = de;
        for (int j = k.posD - 1; j >= 0; --j) {
            timed(F_NORM, [&] {
                launch_ln_gelu_bwd(da, pl.stk_z[j], pl.stk_mean[j], pl.stk_rstd[j], dpz, (int)BT, T, H, rT(), st);
            }, 4.0 * BT * H * 3);
            stack_conv(false, j, dpz, j == 0 ? de : nullptr, dh0);
            da = dh0;
        }
    } else if (posconv_fp32_kernel())
        timed(F_GEMM, [&] {
            if (!launch_posconv(false, dpz, wpos_b, nullptr, de, dh0, nullptr, B, T, H, k.posG, k.posK,
                                k.posK - 1 - k.posK / 2, rT(), st))
                throw SutaError(SUTA_ERR_UNSUPPORTED, "positional conv shape");
        });
    else if (posconv_bf16())
        timed(F_GEMM, [&] {
            if (!launch_posconv_bf16(false, dpz, wpos_bf_b, nullptr, de, dh0, nullptr, B, T, H, k.posG, k.posK,
                                     k.posK - 1 - k.posK / 2, rT(), st))
                throw SutaError(SUTA_ERR_UNSUPPORTED, "positional conv shape");
        });
    else {
        GemmParams g = posconv_gemm(dpz, wpos_b, k.posK - 1 - k.posK / 2, dh0, de);
        if (plan.ragged) {  // padding frames receive conv gradient from valid ones: keep them at 0
            g.epi |= EPI_ROWMASK;
            g.zrows = rT();
        }
        gemm(g);
    }
    const int C6 = k.C[k.nconv - 1];
    if (hp.train_feature) {
        // dWproj = dh0^T fp_y  (per utterance)
        gemm(per_utt(H, C6, T, utt(dh0, H, (long)T * H), 1, utt(pl.fp_y, C6, (long)T * C6), 0, utt(G + o_pw, C6, Pn)));
        timed(F_NORM, [&] { launch_colsum(dh0, B, T, H, G + o_pb, Pn, pl.lnpart, st); });
    }
    // d fp_y = dh0 @ Wproj  (per utterance W)
    gemm(per_utt(T, C6, H, utt(dh0, H, (long)T * H), 0, utt(P + o_pw, C6, Pn), 0, utt(pl.dzc, C6, (long)T * C6)));
    const int last = k.nconv - 1;
    // feature-projection LN bwd; in group mode also * gelu'(z_last) => dz_last
    float* cur = pl.dzc2;
    timed(F_NORM, [&] {
        LnBwd b = ln_bwd(ln_f32(pl.dzc), ln_out(cur), ln_f32(pl.a[last]));
        if (!k.layer_mode && hp.train_feature) b.post_aux = pl.z[last];
        ln_backward(feat_proj_ln(), b, st);
    });
    if (!hp.train_feature) return;
    float* other = pl.dzc;
    // bf16 conv storage: z_i and (below the last layer) da_i are bf16 planes in place in their fp32 buffers
    const bool zbf = k.layer_mode && conv_z_bf16();
    auto conv_dy = [&](int i) { return zbf && i < last ? ln_bf16(cur) : ln_f32(cur); };  // cur = da_i
    for (int i = last; i >= 1; --i) {
        // cur: group mode -> dz_i ; layer mode -> da_i
        bool fused = false;  // the LayerNorm backward also sums the conv bias gradient (one read of dz_i)
        const bool cpl = conv_planes();
        if (k.layer_mode) {
            const LnConvGrads cg{k.conv_bias ? G + o_cb[i] : nullptr};  // (no weight gradient: a GEMM below)
            float* dz32 = cpl && conv_dx_planes() ? nullptr : other;  // both conv GEMMs read dz_i's plane: no fp32 copy
            LnBwd b = ln_bwd(conv_dy(i), ln_out(dz32, cpl ? conv_dz_plane() : nullptr), conv_z(i));
            b.conv = &cg;
            fused = (fused_conv_ln() || cpl) && ln_bwd_route(conv_ln(i), b).sums_conv_grads;
            if (!fused) {  // the plain backward; launch_colsum follows (only the fused one writes the dz plane)
                if (zbf) throw SutaError(SUTA_ERR_UNSUPPORTED, "conv stack in bf16: the fused LayerNorm backward is required");
                if (cpl) throw SutaError(SUTA_ERR_UNSUPPORTED, "conv planes: dz plane not written");
                b = ln_bwd(ln_f32(cur), ln_out(other), ln_f32(pl.z[i]));
            }
            timed(F_NORM, [&] { ln_backward(conv_ln(i), b, st); });
            std::swap(cur, other);
        }
        if (k.conv_bias && !fused)
            timed(F_NORM, [&] { launch_colsum(cur, B, pl.Lc[i], k.C[i], G + o_cb[i], Pn, pl.lnpart, st); });
        {  // dW_i = im2col(a_{i-1})^T dz_i
            GemmParams g = per_utt(k.K[i] * k.C[i - 1], k.C[i], pl.Lc[i],
                                   utt(pl.a[i - 1], (long)k.S[i] * k.C[i - 1], (long)pl.Lc[i - 1] * k.C[i - 1]), 1,
                                   utt(cur, k.C[i], (long)pl.Lc[i] * k.C[i]), 0, utt(G + o_cw[i], k.C[i], Pn));
            if (cpl) {  // bf16 planes: the forward's activation plane and the LayerNorm-written dz plane (the fp32
                        // activation was not stored)
                g.A = nullptr;
                set_planes(g, conv_act_plane(i - 1), g.lda, conv_dz_plane(), g.ldb);
            }
            gemm(g);
        }
        {  // da_{i-1} = conv_i^T(dz_i): one GEMM per output-row residue rho (rows S*m + rho), whose K
           // runs over the taps k = rho + S*j (segment seg = nj-1-j reads dz row m - j and weight tap k)
            const int S_ = k.S[i], Kt = k.K[i], Cin = k.C[i - 1], Cout = k.C[i];
            const int Lin = pl.Lc[i - 1], Lout = pl.Lc[i];
            const float* zprev = (!k.layer_mode && i - 1 >= 1) ? pl.z[i - 1] : nullptr;
            for (int rho = 0; rho < S_; ++rho) {
                const int Mrows = (Lin - rho + S_ - 1) / S_;
                const int nj = (Kt - rho + S_ - 1) / S_;
                if (Mrows <= 0) continue;
                if (nj <= 0) throw SutaError(SUTA_ERR_UNSUPPORTED, "conv stride > kernel");
                const long tap0 = (long)(rho + S_ * (nj - 1)) * Cin * Cout;  // segment 0's weight tap
                GemmParams g = per_utt(Mrows, Cin, nj * Cout, utt(cur, Cout, (long)Lout * Cout), 0,
                                       utt(P + o_cw[i] + tap0, Cout, Pn), 1,
                                       utt(other + (long)rho * Cin, (long)S_ * Cin, (long)Lin * Cin));
                g.segK = Cout;
                g.pad = nj - 1;
                g.Mvalid = Lout;
                g.segB = 1;
                g.sBseg = -(long)S_ * Cin * Cout;
                if (zprev) set_aux(g, EPI_DGELU, utt(zprev + (long)rho * Cin, (long)S_ * Cin, (long)Lin * Cin));
                if (cpl && conv_dx_planes()) {  // bf16 planes: the LayerNorm-written dz plane and the forward's
                                                // source-layout bf16 weights (strides in bf16 elements)
                    g.A = nullptr;
                    g.B = nullptr;
                    set_planes(g, conv_dz_plane(), Cout, static_cast<char*>(conv_wt_plane(i, 1)) + tap0 * 2, Cout);
                    g.tb = 0;
                    g.sB1 = (long)Kt * Cin * Cout;
                    if (zbf) {  // da_{i-1} in bf16 only (the next LayerNorm backward reads it widened)
                        g.C = nullptr;
                        set_c_plane(g, reinterpret_cast<__bf16*>(other) + (long)rho * Cin, (long)S_ * Cin, (long)Lin * Cin);
                    }
                }
                gemm(g);
            }
        }
        std::swap(cur, other);
    }
    // conv0: cur = da0
    if (!k.layer_mode) {
        timed(F_FRONT, [&] {
            launch_front_gn_bwd(pl.x, pl.N, P + o_cw[0], k.conv_bias ? P + o_cb[0] : nullptr, Pn, B, pl.Lc[0], k.C[0],
                                k.K[0], k.S[0], P + o_cg[0], P + o_cbeta[0], pl.gn_mean, pl.gn_rstd, cur, G + o_cg[0],
                                G + o_cbeta[0], G + o_cw[0], Pn, pl.dpart, pl.c0part, rL0(), st);
        }, 4.0 * B * ((double)pl.N + (double)pl.Lc[0] * k.C[0]));  // waveform and activation gradient read
        return;
    }
    // fused: the LayerNorm backward also sums the conv0 bias and weight gradients (dz0 read once, consumed in
    // registers: not stored)
    const LnConvGrads cg{k.conv_bias ? G + o_cb[0] : nullptr, G + o_cw[0], pl.x, pl.N, k.S[0], k.K[0]};
    LnBwd b = ln_bwd(conv_dy(0), LnOut{}, conv_z(0));
    b.conv = &cg;
    const bool fused0 = (fused_conv_ln() || zbf) && ln_bwd_route(conv_ln(0), b).sums_conv_grads;
    if (!fused0) {
        if (zbf) throw SutaError(SUTA_ERR_UNSUPPORTED, "conv stack in bf16: the fused conv0 LayerNorm backward is required");
        b = ln_bwd(ln_f32(cur), ln_out(other), ln_f32(pl.z[0]));
    }
    timed(F_NORM, [&] { ln_backward(conv_ln(0), b, st); });
    if (fused0) return;
    if (k.conv_bias)
        timed(F_NORM, [&] { launch_colsum(other, B, pl.Lc[0], k.C[0], G + o_cb[0], Pn, pl.lnpart, st); });
    // dW0[k][c] = sum_t x[S0 t + k] dz0[t][c]
    gemm(per_utt(k.K[0], k.C[0], pl.Lc[0], utt(pl.x, k.S[0], pl.N), 1, utt(other, k.C[0], (long)pl.Lc[0] * k.C[0]), 0,
                 utt(G + o_cw[0], k.C[0], Pn)));
}

// The optimizer scalars a table row depends on (the rest of suta_hparams only shapes the loss)
static bool same_opt_scalars(const suta_hparams& a, const suta_hparams& b) {
    return a.lr == b.lr && a.beta1 == b.beta1 && a.beta2 == b.beta2 && a.weight_decay == b.weight_decay &&
           a.optimizer == b.optimizer && a.lr_step_size == b.lr_step_size && a.lr_gamma == b.lr_gamma;
}

// lr of optimizer step i counted from the last reset: torch.optim.lr_scheduler.StepLR (main.py:20-21, step_size 1 and
// gamma 0.7 there) multiplies the group's lr by gamma, in double, each time its step count (advanced after every
// optimizer step, main.py:207-208) reaches a multiple of step_size (StepLR.get_lr, the chained form); the episodic
// reset restores it (main.py:147-152).  Carried as a running product over h_lr (rows are only ever appended while
// the scalars stay the same), so step i costs O(1) amortised and equals the chained loop bitwise.
double suta_engine::lr_at(const suta_hparams& hp, long i) {
    if (h_lr.empty() || !same_opt_scalars(hp, tab_hp)) {
        h_lr.clear();
        h_tab.clear();
        dev_rows = 0;
        tab_hp = hp;
        h_lr.push_back(py_double(hp.lr));
    }
    const double g = py_double(hp.lr_gamma);
    while ((long)h_lr.size() <= i) {
        const long e = (long)h_lr.size();
        const double prev = h_lr.back();
        h_lr.push_back(hp.lr_step_size > 0 && e % hp.lr_step_size == 0 ? prev * g : prev);
    }
    return h_lr[i];
}

static void check_optimizer(const suta_hparams& hp) {
    if (hp.optimizer != SUTA_OPT_ADAMW && hp.optimizer != SUTA_OPT_SGD)
        throw SutaError(SUTA_ERR_UNSUPPORTED, "optimizer: SUTA_OPT_ADAMW or SUTA_OPT_SGD");
    if (hp.lr_step_size < 0) throw SutaError(SUTA_ERR_ARG, "lr_step_size < 0");
}

void suta_engine::adam(int B, const suta_hparams& hp) {
    AdamArgs a{};
    check_optimizer(hp);
    // Python floats are doubles: recover the decimal the caller meant (0.9f -> 0.9) so the
    // scalars match torch's double-precision host arithmetic (adam.py:495-510)
    const double lr = lr_at(hp, opt_steps), b1 = py_double(hp.beta1), b2 = py_double(hp.beta2);
    a.beta1 = (float)b1;
    a.beta2 = (float)b2;
    a.omb1 = (float)(1.0 - b1);
    a.omb2 = (float)(1.0 - b2);
    a.eps = (float)py_double(hp.adam_eps);
    a.lr_wd = (float)(py_double(hp.lr) * py_double(hp.weight_decay));  // (a flag: the per-step factor is in the table)
    a.sgd = hp.optimizer == SUTA_OPT_SGD;
    // runs of equal multiplicity over the flat layout
    a.nruns = 0;
    int kmax = 0;
    for (const TP& t : tps) {
        const int m = multiplicity(t, hp.train_feature, hp.bias_only);
        kmax = std::max(kmax, m);
        if (m == 0) continue;
        if (a.nruns > 0 && a.runs[a.nruns - 1].k == m && a.runs[a.nruns - 1].start + a.runs[a.nruns - 1].len == t.off) {
            a.runs[a.nruns - 1].len += t.numel;
        } else {
            if (a.nruns >= SUTA_MAX_RUNS) throw SutaError(SUTA_ERR_UNSUPPORTED, "too many Adam runs");
            a.runs[a.nruns++] = AdamRun{t.off, t.numel, m};
        }
    }
    if (kmax > 5) throw SutaError(SUTA_ERR_UNSUPPORTED, "multiplicity > 5");
    for (int kk = 1; kk <= 5; ++kk)
        for (int j = 1; j <= kk; ++j) {
            const double t = (double)(opt_steps * kk + j);
            const double bc1 = 1.0 - std::pow(b1, t);
            const double bc2 = 1.0 - std::pow(b2, t);
            a.step_size[kk - 1][j - 1] = (float)(a.sgd ? lr : lr / bc1);
            a.bc2_sqrt[kk - 1][j - 1] = (float)std::sqrt(bc2);
        }
    a.tab = d_adam_tab;
    a.step = d_step;
    timed(F_ADAM, [&] {
        launch_adam(P, G, Mo, Vo, Pn, B, a, st);
        launch_step_advance(d_step, st);
    });
    opt_steps += 1;
}

// Device optimizer tables for steps [0, opt_steps + steps) and the device step counter = opt_steps.
void suta_engine::prepare_adam(const suta_hparams& hp, int steps) {
    check_optimizer(hp);
    const long need = opt_steps + std::max(steps, 1);
    (void)lr_at(hp, need - 1);  // (re)starts the host rows when the optimizer scalars changed
    if (need > adam_tab_cap) {
        const long cap = std::max<long>(need, 2 * adam_tab_cap);
        if (d_adam_tab) HIPCHK(hipFree(d_adam_tab));
        HIPCHK(hipMalloc(&d_adam_tab, cap * ADAM_TAB * sizeof(float)));
        adam_tab_cap = cap;
        dev_rows = 0;
        drop_graph();  // captured steps point at the old table
    }
    const double b1 = py_double(hp.beta1), b2 = py_double(hp.beta2), wd = py_double(hp.weight_decay);
    const long have = (long)(h_tab.size() / ADAM_TAB);
    if (need > have) h_tab.resize(need * ADAM_TAB, 0.f);
    for (long s0 = have; s0 < need; ++s0) {
        const double lr = h_lr[s0];
        float* row = h_tab.data() + s0 * ADAM_TAB;
        for (int kk = 1; kk <= 5; ++kk)
            for (int j = 1; j <= kk; ++j) {
                const double t = (double)(s0 * kk + j);
                row[(kk - 1) * 5 + (j - 1)] = (float)(lr / (1.0 - std::pow(b1, t)));
                row[25 + (kk - 1) * 5 + (j - 1)] = (float)std::sqrt(1.0 - std::pow(b2, t));
            }
        row[50] = (float)(1.0 - lr * wd);
        row[51] = (float)(-lr);
    }
    h_step = (int)opt_steps;
    if (need > dev_rows) {  // rows already on the device hold the same values: only the new ones go up
        HIPCHK(hipMemcpyAsync(d_adam_tab + dev_rows * ADAM_TAB, h_tab.data() + dev_rows * ADAM_TAB,
                              (need - dev_rows) * ADAM_TAB * sizeof(float), hipMemcpyHostToDevice, st));
        dev_rows = need;
    }
    HIPCHK(hipMemcpyAsync(d_step, &h_step, sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // pageable sources
}

// The device work of one suta_adapt call after its input is staged: episodic slot reset (pristine
// tensors broadcast into the slots; the moments are implicit zeros at Adam step 0), the vanilla forward,
// then S x (backward, Adam, forward); at each recorded step the logits are copied and the greedy ids
// computed into device staging.  Ordered on the engine stream only, so it captures as one graph.
void suta_engine::adapt_loop(int B, const suta_hparams& hp, int steps, const int* rec, int nrec, float* rec_logits,
                             int* rec_ids) {
    const long rows = (long)B * plan.T;
    if (hp.episodic) launch_broadcast(P, P0, Pn, B, st);
    for (int s = 0; s <= steps; ++s) {
        if (s > 0) {
            backward(B, hp);
            adam(B, hp);
        }
        forward(B);
        for (int i = 0; i < nrec; ++i) {
            if (rec[i] != s) continue;
            if (rec_logits)
                HIPCHK(hipMemcpyAsync(rec_logits + i * rows * c.V, plan.logits, rows * c.V * sizeof(float),
                                      hipMemcpyDeviceToDevice, st));
            if (rec_ids) launch_argmax(plan.logits, rows, c.V, rec_ids + i * rows, st);
        }
    }
}

// With graphs on, per-kernel timing off and `graph_ok` (this call repeats the previous call's key: batch,
// layout, ragged, precision, hparams, steps, record set, outputs), the whole loop is captured once and
// replayed per call; a one-off key runs eagerly (no capture cost).  Replay == eager bitwise (GPU test).
void suta_engine::run_adapt_loop(int B, const suta_hparams& hp, int steps, const int* rec, int nrec,
                                 float* rec_logits, int* rec_ids, bool graph_ok) {
    if (!use_graphs || timing || !graph_ok) {
        adapt_loop(B, hp, steps, rec, nrec, rec_logits, rec_ids);
        last_loop_mode = SUTA_LOOP_EAGER;
        return;
    }
    last_loop_mode = loop_graph ? SUTA_LOOP_REPLAYED : SUTA_LOOP_CAPTURED;
    if (!loop_graph) {
        const long steps0 = opt_steps;
        hipGraph_t g = nullptr;
        HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
        try {
            adapt_loop(B, hp, steps, rec, nrec, rec_logits, rec_ids);
        } catch (...) {
            (void)hipStreamEndCapture(st, &g);
            if (g) (void)hipGraphDestroy(g);
            opt_steps = steps0;
            throw;
        }
        HIPCHK(hipStreamEndCapture(st, &g));
        opt_steps = steps0;  // the capture recorded the Adam steps without running them
        HIPCHK(hipGraphInstantiate(&loop_graph, g, nullptr, nullptr, 0));
        HIPCHK(hipGraphDestroy(g));
        ++graph_captures;
    }
    HIPCHK(hipGraphLaunch(loop_graph, st));
    ++graph_launches;
    opt_steps += steps;
    if (hp.pl_coef > 0.f && steps > 0) sdpl_used = true;  // the replayed SDPL kernels may raise the error flag
}

// Key of this call; true when it equals the previous call's (graph capture pays off from the 2nd call)
// The 960h rule at this engine's class count: id 0 pad, 1..3 lookup failures, 4 the delimiter (an inner space is
// id 4 again), every other id itself (main_SDPL.py:194-203 with the vocab.json the reference ships).
void suta_engine::default_pl_table(std::vector<int>& off, std::vector<int>& ids, std::vector<int>& kind,
                                   int& space_id) const {
    const int V = c.V;
    off.assign(1, 0);
    ids.clear();
    kind.assign(V, SDPL_KIND_NORMAL);
    for (int i = 0; i < V; ++i) {
        if (i == 0) kind[i] = SDPL_KIND_DROP;
        else if (i <= 3) kind[i] = SDPL_KIND_FAIL;
        else if (i == 4) kind[i] = SDPL_KIND_SPACE;
        else ids.push_back(i);
        off.push_back((int)ids.size());
    }
    space_id = V > 4 ? 4 : -1;
}

void suta_engine::set_pl_table(const std::vector<int>& off, const std::vector<int>& ids, const std::vector<int>& kind,
                               int space_id) {
    const int V = c.V;
    std::vector<int> h(off);
    h.insert(h.end(), kind.begin(), kind.end());
    h.insert(h.end(), ids.begin(), ids.end());
    int* d = nullptr;
    HIPCHK(hipSetDevice(device));
    if (st) HIPCHK(hipStreamSynchronize(st));
    drop_graph();
    HIPCHK(hipMalloc(&d, h.size() * sizeof(int)));
    if (pl_buf) (void)hipFree(pl_buf);
    pl_buf = d;
    HIPCHK(hipMemcpy(d, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
    pl_tab.off = d;
    pl_tab.kind = d + V + 1;
    pl_tab.ids = d + 2 * V + 1;
    pl_tab.space_id = space_id;
    std::vector<int> doff, dids, dkind;
    int dsp;
    default_pl_table(doff, dids, dkind, dsp);
    pl_default = off == doff && ids == dids && kind == dkind && space_id == dsp;
    ++pl_epoch;
}

bool suta_engine::graph_key_repeats(const GraphKey& k) {
    const bool same = gkey_seen && gkey.B == k.B && gkey.N == k.N && gkey.ragged == k.ragged &&
                      gkey.mode == k.mode && gkey.steps == k.steps && gkey.want_logits == k.want_logits &&
                      gkey.want_ids == k.want_ids && gkey.rec == k.rec && gkey.pl_epoch == k.pl_epoch &&
                      std::memcmp(&gkey.hp, &k.hp, sizeof(suta_hparams)) == 0 &&
                      std::memcmp(&gkey.sw, &k.sw, sizeof(SutaSwitches)) == 0;
    if (!same) {
        drop_graph();
        gkey = k;
        gkey_seen = true;
    }
    return same;
}

// bf16 planes of the frozen linear weights (RNE, as the bf16 GEMMs round every operand): W [N][K] for the
// forward x W^T and W^T [in][out] for the input gradient dY W, so both GEMMs read k-contiguous planes.
void suta_engine::build_weight_planes() {
    if (!wplanes.empty()) return;
    auto add = [&](const float* w, long rows, long cols) {  // w: [rows = out][cols = in]
        std::vector<float> hw((size_t)rows * cols);
        HIPCHK(hipMemcpy(hw.data(), w, hw.size() * 4, hipMemcpyDeviceToHost));
        std::vector<__bf16> a(hw.size()), t(hw.size());
        for (long r = 0; r < rows; ++r)
            for (long c2 = 0; c2 < cols; ++c2) {
                const __bf16 v = (__bf16)hw[(size_t)r * cols + c2];
                a[(size_t)r * cols + c2] = v;
                t[(size_t)c2 * rows + r] = v;
            }
        float* pa = dalloc((long)(a.size() + 1) / 2 + 4);
        float* pt = dalloc((long)(t.size() + 1) / 2 + 4);
        HIPCHK(hipMemcpy(pa, a.data(), a.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(pt, t.data(), t.size() * 2, hipMemcpyHostToDevice));
        wplanes[w] = {pa, pt};
    };
    const long H = c.H, F = c.F;
    for (int l = 0; l < c.L; ++l) {
        add(wqkv[l], 3 * H, H);
        add(wo[l], H, H);
        add(w1[l], F, H);
        add(w2[l], H, F);
    }
    add(wlm, c.V, H);
}

// Pristine tensors into slots [0, B) and the Adam step counter to 0.  The moments need no clearing: the
// Adam kernel takes them as zero at step 0 (zero_moments only keeps unused slots deterministic).
void suta_engine::reset_slots(int B, bool zero_moments) {
    launch_broadcast(P, P0, Pn, B, st);
    if (zero_moments) {
        HIPCHK(hipMemsetAsync(Mo, 0, (size_t)B * Pn * sizeof(float), st));
        HIPCHK(hipMemsetAsync(Vo, 0, (size_t)B * Pn * sizeof(float), st));
    }
    opt_steps = 0;
    h_step = 0;
    HIPCHK(hipMemcpyAsync(d_step, &h_step, sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
}

void suta_engine::stage_input(const float* wav, int on_dev, int norm, int B, long N, long stride) {
    const hipMemcpyKind kind = on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (!plan.ragged) {
        HIPCHK(hipMemcpyAsync(plan.xraw, wav, (size_t)B * N * sizeof(float), kind, st));
    } else {  // utterance b: n[b] samples at wav + b * stride -> slot b of the N-stride layout, zero padded
        HIPCHK(hipMemsetAsync(plan.xraw, 0, (size_t)B * N * sizeof(float), st));
        for (int b = 0; b < B; ++b)
            HIPCHK(hipMemcpyAsync(plan.xraw + (long)b * N, wav + (long)b * stride, (size_t)plan.h_n[b] * sizeof(float),
                                  kind, st));
    }
    if (norm) timed(F_EW, [&] { launch_wave_normalize(plan.xraw, plan.x, B, N, rN(), st); });
    else HIPCHK(hipMemcpyAsync(plan.x, plan.xraw, (size_t)B * N * sizeof(float), hipMemcpyDeviceToDevice, st));
}

// ==============================================================================================
// C ABI
// ==============================================================================================
namespace {

template <typename Fn>
int32_t guard(Fn&& fn) {
    try {
        fn();
        return SUTA_OK;
    } catch (const SutaError& e) {
        g_err = e.what();
        return e.code;
    } catch (const std::exception& e) {
        g_err = e.what();
        return SUTA_ERR_ARG;
    }
}

Cfg make_cfg(const suta_model_config* m, const suta_model_family* fam) {
    Cfg c{};
    c.H = m->hidden_size;
    c.L = m->num_hidden_layers;
    c.NH = m->num_attention_heads;
    c.F = m->intermediate_size;
    c.V = m->vocab_size;
    c.nconv = m->num_conv_layers;
    if (c.nconv < 2 || c.nconv > SUTA_MAX_CONV) throw SutaError(SUTA_ERR_ARG, "num_conv_layers out of range");
    for (int i = 0; i < c.nconv; ++i) {
        c.C[i] = m->conv_dim[i];
        c.K[i] = m->conv_kernel[i];
        c.S[i] = m->conv_stride[i];
        if (c.C[i] % 4 || c.C[i] <= 0) throw SutaError(SUTA_ERR_UNSUPPORTED, "conv_dim must be a multiple of 4");
    }
    if (c.K[0] > 16) throw SutaError(SUTA_ERR_UNSUPPORTED, "conv0 kernel > 16");
    c.conv_bias = m->conv_bias;
    c.layer_mode = m->feat_extract_norm_layer;
    c.stable = m->do_stable_layer_norm;
    c.posK = m->num_conv_pos_embeddings;
    c.posG = m->num_conv_pos_embedding_groups;
    c.eps = m->layer_norm_eps;
    c.family = fam ? fam->model_family : SUTA_FAMILY_WAV2VEC2;
    if (c.family < SUTA_FAMILY_WAV2VEC2 || c.family > SUTA_FAMILY_DATA2VEC_AUDIO)
        throw SutaError(SUTA_ERR_ARG, "model_family is none of SUTA_FAMILY_*");
    c.posD = 0;
    if (c.family == SUTA_FAMILY_DATA2VEC_AUDIO) {
        if (!c.layer_mode) throw SutaError(SUTA_ERR_ARG, "data2vec-audio requires feat_extract_norm_layer = 1");
        if (c.stable) throw SutaError(SUTA_ERR_ARG, "data2vec-audio requires do_stable_layer_norm = 0");
        c.posD = m->num_conv_pos_embeddings;
        c.posK = fam->conv_pos_kernel_size;
        if (c.posD < 1 || c.posD > MAX_POS_STACK)
            throw SutaError(SUTA_ERR_UNSUPPORTED, "data2vec-audio: num_conv_pos_embeddings (the stack's depth) outside 1 .. 8");
        if (c.posK < 1 || c.posK > 128)
            throw SutaError(SUTA_ERR_UNSUPPORTED, "data2vec-audio: conv_pos_kernel_size outside 1 .. 128");
    }
    // HF builds the attention adapter in wav2vec2's stable-LN layer class only; the post-LN class and the other
    // families ignore the field
    c.A = (c.stable && c.family == SUTA_FAMILY_WAV2VEC2) ? m->adapter_attn_dim : 0;
    if (c.A < 0) throw SutaError(SUTA_ERR_ARG, "adapter_attn_dim < 0");
    if (c.A > 64) throw SutaError(SUTA_ERR_UNSUPPORTED, "adapter_attn_dim > 64 (the adapter kernels hold 1 <= A <= 64)");
    if (c.H % c.NH || c.H % c.posG) throw SutaError(SUTA_ERR_ARG, "hidden_size not divisible by heads/groups");
    // the conv-A GEMM's segmented-K loaders move 16-B chunks (4 floats; 8 bf16 on the planes), each inside one segment
    if ((c.H / c.posG) % 8) throw SutaError(SUTA_ERR_UNSUPPORTED, "pos-conv group width must be a multiple of 8");
    if (c.V < 1) throw SutaError(SUTA_ERR_ARG, "vocab_size < 1");
    if (c.V > SUTA_MAX_VOCAB)
        throw SutaError(SUTA_ERR_UNSUPPORTED, "vocab_size > 1024 (the loss path handles 1 <= vocab_size <= 1024)");
    if (c.H > 2048) throw SutaError(SUTA_ERR_UNSUPPORTED, "hidden > 2048");
    if (c.C[c.nconv - 1] > 1024) throw SutaError(SUTA_ERR_UNSUPPORTED, "conv_dim > 1024");
    return c;
}

}  // namespace

extern "C" {

const char* suta_last_error(void) { return g_err.c_str(); }

int32_t suta_num_frames(const suta_model_config* cfg, int64_t n, int64_t* out) {
    return guard([&] {
        long L = n;
        for (int i = 0; i < cfg->num_conv_layers; ++i)  // 0 frames once a layer's input is shorter than its kernel
            L = L < cfg->conv_kernel[i] ? 0 : (L - cfg->conv_kernel[i]) / cfg->conv_stride[i] + 1;
        *out = L;
    });
}

int32_t suta_create(const suta_model_config* cfg, const char* const* names, const float* const* data,
                    const int64_t* numels, int32_t n, int32_t device, int32_t max_batch, int64_t max_samples,
                    suta_engine** out) {
    return suta_create_family(cfg, nullptr, names, data, numels, n, device, max_batch, max_samples, out);
}

int32_t suta_create_family(const suta_model_config* cfg, const suta_model_family* fam, const char* const* names,
                           const float* const* data, const int64_t* numels, int32_t n, int32_t device,
                           int32_t max_batch, int64_t max_samples, suta_engine** out) {
    return guard([&] {
        if (!cfg || !out || max_batch < 1) throw SutaError(SUTA_ERR_ARG, "null argument");
        std::unique_ptr<suta_engine> e(new suta_engine());
        e->c = make_cfg(cfg, fam);
        const Cfg& c = e->c;
        e->device = device;
        e->max_batch = max_batch;
        e->max_samples = max_samples;
        if (const char* af = std::getenv("SUTA_ATTN_FUSED")) e->attn_fused = af[0] != '0';
        if (const char* pc = std::getenv("SUTA_POSCONV")) e->posconv_kernel = pc[0] != '0';
        if (const char* bp = std::getenv("SUTA_BF16_PLANES")) e->bf16_planes = bp[0] != '0';
        // SUTA_GRAPHS=0: no graph capture (as suta_set_graphs(e, 0)); profiling runs under rocprofv3 --pmc, which
        // crashes (SIGSEGV in a profiler thread) once a captured graph is launched -- the kernels are the same
        if (const char* gr = std::getenv("SUTA_GRAPHS")) e->use_graphs = gr[0] != '0';
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking));
        e->d_step = reinterpret_cast<int*>(e->dalloc(1));
        HIPCHK(hipMemset(e->d_step, 0, sizeof(int)));
        std::map<std::string, std::pair<const float*, long>> w;
        for (int i = 0; i < n; ++i) w[names[i]] = {data[i], numels[i]};
        auto get = [&](const std::string& nm, long numel) -> const float* {
            auto it = w.find(nm);
            if (it == w.end()) throw SutaError(SUTA_ERR_ARG, "missing weight " + nm);
            if (it->second.second != numel)
                throw SutaError(SUTA_ERR_ARG, "size mismatch for " + nm + ": got " + std::to_string(it->second.second) +
                                                  " expected " + std::to_string(numel));
            return it->second.first;
        };
        auto up = [&](const std::string& nm, long numel) {
            const float* h = get(nm, numel);
            float* dptr = e->dalloc(numel);
            HIPCHK(hipMemcpy(dptr, h, numel * sizeof(float), hipMemcpyHostToDevice));
            return dptr;
        };
        const std::string pfx = c.family == SUTA_FAMILY_HUBERT           ? "hubert."
                                : c.family == SUTA_FAMILY_DATA2VEC_AUDIO ? "data2vec_audio."
                                                                         : "wav2vec2.";
        const int H = c.H;
        // ---- trainable layout ----
        auto add = [&](const std::string& nm, std::vector<long> shape, bool conv_w, bool ln, bool bias, int depth) {
            TP t;
            t.name = nm;
            t.shape = shape;
            t.numel = 1;
            for (long s : shape) t.numel *= s;
            t.conv_w = conv_w;
            t.ln_member = ln;
            t.is_bias = bias;
            t.feat_depth = depth;
            t.off = rup(e->Pn, 4);
            e->Pn = t.off + t.numel;
            e->tpi[nm] = (int)e->tps.size();
            e->tps.push_back(t);
            return t.off;
        };
        for (int i = 0; i < c.nconv; ++i) {  // conv-layer norms first (layer mode: k = 5)
            const std::string b = pfx + "feature_extractor.conv_layers." + std::to_string(i) + ".layer_norm.";
            if (c.layer_mode) {
                e->o_cg[i] = add(b + "weight", {c.C[i]}, false, true, false, 4);
                e->o_cbeta[i] = add(b + "bias", {c.C[i]}, false, true, true, 4);
            } else if (i == 0) {
                e->o_cg[i] = add(b + "weight", {c.C[i]}, false, false, false, 4);
                e->o_cbeta[i] = add(b + "bias", {c.C[i]}, false, false, true, 4);
            } else {
                e->o_cg[i] = e->o_cbeta[i] = -1;
            }
        }
        for (int i = 0; i < c.nconv; ++i) {
            const std::string b = pfx + "feature_extractor.conv_layers." + std::to_string(i) + ".conv.";
            const long cin = i == 0 ? 1 : c.C[i - 1];
            e->o_cw[i] = add(b + "weight", {c.C[i], cin, c.K[i]}, true, false, false, 4);
            e->o_cb[i] = c.conv_bias ? add(b + "bias", {c.C[i]}, false, false, true, 4) : -1;
        }
        const int C6 = c.C[c.nconv - 1];
        e->o_fpg = add(pfx + "feature_projection.layer_norm.weight", {C6}, false, true, false, 2);
        e->o_fpb = add(pfx + "feature_projection.layer_norm.bias", {C6}, false, true, true, 2);
        e->o_pw = add(pfx + "feature_projection.projection.weight", {H, C6}, false, false, false, 2);
        e->o_pb = add(pfx + "feature_projection.projection.bias", {H}, false, false, true, 2);
        e->o_eg = add(pfx + "encoder.layer_norm.weight", {H}, false, true, false, 0);
        e->o_eb = add(pfx + "encoder.layer_norm.bias", {H}, false, true, true, 0);
        for (int l = 0; l < c.L; ++l) {
            const std::string b = pfx + "encoder.layers." + std::to_string(l) + ".";
            e->o_l1g.push_back(add(b + "layer_norm.weight", {H}, false, true, false, 0));
            e->o_l1b.push_back(add(b + "layer_norm.bias", {H}, false, true, true, 0));
            e->o_l2g.push_back(add(b + "final_layer_norm.weight", {H}, false, true, false, 0));
            e->o_l2b.push_back(add(b + "final_layer_norm.bias", {H}, false, true, true, 0));
            if (c.A > 0) {  // the adapter's nn.LayerNorm: collect_params takes it like any other
                e->o_adg.push_back(add(b + "adapter_layer.norm.weight", {H}, false, true, false, 0));
                e->o_adb.push_back(add(b + "adapter_layer.norm.bias", {H}, false, true, true, 0));
            }
        }
        e->Pn = rup(e->Pn, 64);
        std::vector<float> hp0(e->Pn, 0.f);
        for (const TP& t : e->tps) {
            const float* src = get(t.name, t.numel);
            if (t.conv_w) {  // [co][ci][k] -> [k][ci][co]
                const long co = t.shape[0], ci = t.shape[1], kk = t.shape[2];
                for (long o = 0; o < co; ++o)
                    for (long i2 = 0; i2 < ci; ++i2)
                        for (long q = 0; q < kk; ++q) hp0[t.off + (q * ci + i2) * co + o] = src[(o * ci + i2) * kk + q];
            } else {
                std::memcpy(&hp0[t.off], src, t.numel * sizeof(float));
            }
        }
        e->P0 = e->dalloc(e->Pn);
        HIPCHK(hipMemcpy(e->P0, hp0.data(), e->Pn * sizeof(float), hipMemcpyHostToDevice));
        e->P = e->dalloc((long)max_batch * e->Pn);
        e->G = e->dalloc((long)max_batch * e->Pn);
        e->Mo = e->dalloc((long)max_batch * e->Pn);
        e->Vo = e->dalloc((long)max_batch * e->Pn);
        HIPCHK(hipMemset(e->G, 0, (size_t)max_batch * e->Pn * sizeof(float)));
        // ---- frozen encoder weights ----
        for (int l = 0; l < c.L; ++l) {
            const std::string b = pfx + "encoder.layers." + std::to_string(l) + ".";
            std::vector<float> qkv((size_t)3 * H * H), bq((size_t)3 * H);
            const char* parts[3] = {"q_proj", "k_proj", "v_proj"};
            for (int j = 0; j < 3; ++j) {
                std::memcpy(&qkv[(size_t)j * H * H], get(b + "attention." + parts[j] + ".weight", (long)H * H),
                            sizeof(float) * H * H);
                std::memcpy(&bq[(size_t)j * H], get(b + "attention." + parts[j] + ".bias", H), sizeof(float) * H);
            }
            float* dq = e->dalloc(3L * H * H);
            HIPCHK(hipMemcpy(dq, qkv.data(), qkv.size() * 4, hipMemcpyHostToDevice));
            float* dbq = e->dalloc(3L * H);
            HIPCHK(hipMemcpy(dbq, bq.data(), bq.size() * 4, hipMemcpyHostToDevice));
            e->wqkv.push_back(dq);
            e->bqkv.push_back(dbq);
            e->wo.push_back(up(b + "attention.out_proj.weight", (long)H * H));
            e->bo.push_back(up(b + "attention.out_proj.bias", H));
            e->w1.push_back(up(b + "feed_forward.intermediate_dense.weight", (long)c.F * H));
            e->b1.push_back(up(b + "feed_forward.intermediate_dense.bias", c.F));
            e->w2.push_back(up(b + "feed_forward.output_dense.weight", (long)c.F * H));
            e->b2.push_back(up(b + "feed_forward.output_dense.bias", H));
            if (c.A > 0) {  // zero-padded to [NA][Hp] / [Hp][NA], each linear in both orientations
                const int A = c.A, NA = adapter_padded_width(A), Hp = (int)rup(H, 16);
                const std::string a = b + "adapter_layer.";
                const float* l1 = get(a + "linear_1.weight", (long)A * H);  // [A][H]
                const float* l1b = get(a + "linear_1.bias", A);
                const float* l2 = get(a + "linear_2.weight", (long)H * A);  // [H][A]
                const float* l2b = get(a + "linear_2.bias", H);
                std::vector<float> w1p((size_t)NA * Hp, 0.f), w1t((size_t)Hp * NA, 0.f), w2p((size_t)Hp * NA, 0.f),
                    w2t((size_t)NA * Hp, 0.f), b1p(NA, 0.f), b2p(Hp, 0.f);
                for (int n = 0; n < A; ++n)
                    for (int h = 0; h < H; ++h) {
                        w1p[(size_t)n * Hp + h] = w1t[(size_t)h * NA + n] = l1[(size_t)n * H + h];
                        w2p[(size_t)h * NA + n] = w2t[(size_t)n * Hp + h] = l2[(size_t)h * A + n];
                    }
                std::copy(l1b, l1b + A, b1p.begin());
                std::copy(l2b, l2b + H, b2p.begin());
                auto upv = [&](const std::vector<float>& v) {
                    float* dptr = e->dalloc((long)v.size());
                    HIPCHK(hipMemcpy(dptr, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
                    return dptr;
                };
                AdapterW aw{};
                aw.w1 = upv(w1p);
                aw.w1t = upv(w1t);
                aw.w2 = upv(w2p);
                aw.w2t = upv(w2t);
                aw.b1 = upv(b1p);
                aw.b2 = upv(b2p);
                aw.A = A;
                aw.NA = NA;
                aw.Hp = Hp;
                e->adw.push_back(aw);
            }
        }
        e->wlm = up("lm_head.weight", (long)c.V * H);
        e->blm = up("lm_head.bias", c.V);
        // ---- data2vec-audio positional stack: plain grouped convs, regrouped as below, zero taps appended ----
        for (int j = 0; j < c.posD; ++j) {
            const int K = c.posK, Kp = posconv_stack_taps(K), G = c.posG, Cg = H / G;
            const std::string b = pfx + "encoder.pos_conv_embed.layers." + std::to_string(j) + ".conv.";
            const float* v = get(b + "weight", (long)H * Cg * K);
            std::vector<float> wf((size_t)G * Kp * Cg * Cg, 0.f), wb((size_t)G * Kp * Cg * Cg, 0.f);
            for (int gi = 0; gi < G; ++gi)
                for (int co = 0; co < Cg; ++co)
                    for (int ci = 0; ci < Cg; ++ci)
                        for (int q = 0; q < K; ++q) {
                            const float wv = v[(((long)gi * Cg + co) * Cg + ci) * K + q];
                            wf[(((size_t)gi * Kp + q) * Cg + ci) * Cg + co] = wv;
                            wb[(((size_t)gi * Kp + (K - 1 - q)) * Cg + co) * Cg + ci] = wv;
                        }
            float* df = e->dalloc((long)wf.size());
            float* db = e->dalloc((long)wb.size());
            HIPCHK(hipMemcpy(df, wf.data(), wf.size() * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(db, wb.data(), wb.size() * 4, hipMemcpyHostToDevice));
            e->wstk_f.push_back(df);
            e->wstk_b.push_back(db);
            e->bstk.push_back(up(b + "bias", H));
        }
        // ---- positional conv: weight norm (dim=2) precomputed, regrouped for the conv-A GEMM ----
        if (!c.posD) {
            const int K = c.posK, G = c.posG, Cg = H / G;
            const std::string b = pfx + "encoder.pos_conv_embed.conv.";
            const float* g = get(b + "parametrizations.weight.original0", K);
            const float* v = get(b + "parametrizations.weight.original1", (long)H * Cg * K);
            std::vector<double> nrm(K, 0.0);
            for (long o = 0; o < H; ++o)
                for (long i2 = 0; i2 < Cg; ++i2)
                    for (int q = 0; q < K; ++q) {
                        const double x = v[(o * Cg + i2) * K + q];
                        nrm[q] += x * x;
                    }
            // ATen _weight_norm: w = v * (g / ||v||) in fp32
            std::vector<float> nf(K);
            for (int q = 0; q < K; ++q) nf[q] = (float)std::sqrt(nrm[q]);
            std::vector<float> wf((size_t)G * K * Cg * Cg), wb((size_t)G * K * Cg * Cg);
            const bool bfw = Cg == 64;  // bf16-mode kernel weights (group width 64)
            std::vector<uint16_t> bf_f(bfw ? wf.size() : 0), bf_b(bfw ? wf.size() : 0);
            auto rne = [](float f) {  // fp32 -> bf16 bits, round to nearest even (finite values), as (__bf16)f
                uint32_t u;
                std::memcpy(&u, &f, 4);
                return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
            };
            for (int gi = 0; gi < G; ++gi)
                for (int co = 0; co < Cg; ++co)
                    for (int ci = 0; ci < Cg; ++ci)
                        for (int q = 0; q < K; ++q) {
                            const long o = (long)gi * Cg + co;
                            const float wv = v[(o * Cg + ci) * K + q] * (g[q] / nf[q]);  // ATen _weight_norm
                            // fwd B[(q, ci)][co] ; bwd B[(q', co)][ci] with q' = K-1-q
                            wf[(((size_t)gi * K + q) * Cg + ci) * Cg + co] = wv;
                            wb[(((size_t)gi * K + (K - 1 - q)) * Cg + co) * Cg + ci] = wv;
                            if (bfw) {  // [g][q][n][k]: fwd n = co, k = ci; bwd (q' = K-1-q) n = ci, k = co
                                bf_f[(((size_t)gi * K + q) * Cg + co) * Cg + ci] = rne(wv);
                                bf_b[(((size_t)gi * K + (K - 1 - q)) * Cg + ci) * Cg + co] = rne(wv);
                            }
                        }
            e->wpos_f = e->dalloc((long)wf.size());
            e->wpos_b = e->dalloc((long)wb.size());
            HIPCHK(hipMemcpy(e->wpos_f, wf.data(), wf.size() * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(e->wpos_b, wb.data(), wb.size() * 4, hipMemcpyHostToDevice));
            if (bfw) {
                e->wpos_bf_f = e->dalloc((long)(bf_f.size() + 1) / 2);
                e->wpos_bf_b = e->dalloc((long)(bf_b.size() + 1) / 2);
                HIPCHK(hipMemcpy(e->wpos_bf_f, bf_f.data(), bf_f.size() * 2, hipMemcpyHostToDevice));
                HIPCHK(hipMemcpy(e->wpos_bf_b, bf_b.data(), bf_b.size() * 2, hipMemcpyHostToDevice));
            }
            e->bpos = up(b + "bias", H);
        }
        {
            std::vector<int> off, ids, kind;
            int space_id;
            e->default_pl_table(off, ids, kind, space_id);
            e->set_pl_table(off, ids, kind, space_id);
            e->pl_epoch = 0;
        }
        e->reset_slots(max_batch, true);
        HIPCHK(hipStreamSynchronize(e->st));
        *out = e.release();
    });
}

int32_t suta_destroy(suta_engine* e) {
    return guard([&] {
        if (!e) return;
        (void)hipStreamSynchronize(e->st);
        delete e;
    });
}

int32_t suta_reset(suta_engine* e) {
    return guard([&] {
        e->reset_slots(e->max_batch, true);
        HIPCHK(hipStreamSynchronize(e->st));
    });
}

static void check_batch(suta_engine* e, int32_t batch, int64_t n) {
    if (batch < 1 || batch > e->max_batch) throw SutaError(SUTA_ERR_ARG, "batch outside [1, max_batch]");
    if (n < 1) throw SutaError(SUTA_ERR_ARG, "n_samples < 1");
    if (e->max_samples > 0 && n > e->max_samples)
        throw SutaError(SUTA_ERR_ARG, "n_samples > max_samples given to suta_create");
}

int32_t suta_forward(suta_engine* e, const float* wav, int32_t on_dev, int32_t norm, int32_t batch, int64_t n,
                     float* logits_out) {
    return guard([&] {
        check_batch(e, batch, n);
        HIPCHK(hipSetDevice(e->device));
        suta_latch_switches();
        e->build_plan(batch, n);
        e->set_lengths(batch, nullptr);
        e->stage_input(wav, on_dev, norm, batch, n);
        e->forward(batch);
        HIPCHK(hipMemcpyAsync(logits_out, e->plan.logits, (size_t)batch * e->plan.T * e->c.V * 4, hipMemcpyDeviceToHost,
                              e->st));
        HIPCHK(hipStreamSynchronize(e->st));
        if (e->timing) e->collect_timing();
        e->check_sdpl();
    });
}

int32_t suta_step_ex(suta_engine* e, const float* wav, int32_t on_dev, int32_t norm, int32_t batch, int64_t n,
                     const suta_hparams* hp, int32_t repeat_inference, float* logits_out, int32_t logits_on_dev,
                     float* loss_out) {
    return guard([&] {
        check_batch(e, batch, n);
        if (!logits_out) throw SutaError(SUTA_ERR_ARG, "logits_out is null");
        HIPCHK(hipSetDevice(e->device));
        suta_latch_switches();
        if (hp->pl_coef > 0.f) (void)e->sdpl_table();  // refuses before any launch
        e->build_plan(batch, n);
        e->set_lengths(batch, nullptr);
        e->stage_input(wav, on_dev, norm, batch, n);
        e->prepare_adam(*hp, 1);
        const size_t lbytes = (size_t)batch * e->plan.T * e->c.V * 4;
        const hipMemcpyKind lk = logits_on_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        e->forward(batch);
        // repeat_inference == False (main.py:212-215): the caller gets the grad forward's logits, taken before the
        // backward reuses any buffer
        if (!repeat_inference) HIPCHK(hipMemcpyAsync(logits_out, e->plan.logits, lbytes, lk, e->st));
        e->backward(batch, *hp);
        e->adam(batch, *hp);
        if (repeat_inference) {
            e->forward(batch);
            HIPCHK(hipMemcpyAsync(logits_out, e->plan.logits, lbytes, lk, e->st));
        }
        if (loss_out)
            HIPCHK(hipMemcpyAsync(loss_out, e->plan.loss, (size_t)batch * 4, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipStreamSynchronize(e->st));
        if (e->timing) e->collect_timing();
        e->check_sdpl();
    });
}

int32_t suta_step(suta_engine* e, const float* wav, int32_t on_dev, int32_t norm, int32_t batch, int64_t n,
                  const suta_hparams* hp, float* logits_out, float* loss_out) {
    return suta_step_ex(e, wav, on_dev, norm, batch, n, hp, 1, logits_out, 0, loss_out);
}

}  // extern "C"

// suta_adapt / suta_adapt_varlen body: ns == null -> every utterance has n samples (stride n)
static void adapt_impl(suta_engine* e, const float* wav, int32_t on_dev, int32_t norm, int32_t batch, int64_t n,
                       const int64_t* ns, int64_t stride, int32_t steps, const suta_hparams* hp, const int32_t* rec,
                       int32_t nrec, float* logits_out, int32_t logits_on_dev, int32_t* ids_out, int64_t* frames_out) {
    check_batch(e, batch, n);
    if (steps < 0) throw SutaError(SUTA_ERR_ARG, "steps < 0");
    suta_latch_switches();
    if (hp->pl_coef > 0.f && steps > 0) (void)e->sdpl_table();  // refuses before any launch
    for (int i = 0; i < nrec; ++i)
        if (rec[i] < 0 || rec[i] > steps) throw SutaError(SUTA_ERR_ARG, "record step outside [0, steps]");
    HIPCHK(hipSetDevice(e->device));
    e->build_plan(batch, n);
    e->set_lengths(batch, ns);
    const int T = e->plan.T, V = e->c.V;
    if (frames_out) {
        if (ns) for (int b = 0; b < batch; ++b) frames_out[b] = e->plan.h_T[b];
        else *frames_out = T;
    }
    const size_t per = (size_t)batch * T * V;
    e->stage_input(wav, on_dev, norm, batch, n, stride);
    if (hp->episodic) e->opt_steps = 0;  // slots are reset inside the loop (adapt_loop)
    e->prepare_adam(*hp, steps);
    // device staging of the recorded outputs (the loop is graph-captured; it never touches host memory)
    const size_t rl = logits_out ? (size_t)nrec * per : 0, ri = ids_out ? (size_t)nrec * batch * T : 0;
    if (e->recbuf.alloc((rl + ri) * sizeof(float) + 256)) e->drop_graph();
    float* rec_logits = logits_out ? e->recbuf.p : nullptr;
    int* rec_ids = ids_out ? reinterpret_cast<int*>(e->recbuf.p + rl) : nullptr;
    suta_engine::GraphKey key;
    key.B = batch;
    key.N = e->plan.N;
    key.ragged = e->plan.ragged;
    key.mode = e->gemm_mode;
    key.steps = steps;
    key.want_logits = logits_out != nullptr;
    key.want_ids = ids_out != nullptr;
    key.hp = *hp;
    key.rec.assign(rec, rec + nrec);
    key.sw = suta_switches();
    key.pl_epoch = e->pl_epoch;
    const bool graph_ok = e->graph_key_repeats(key);
    e->run_adapt_loop(batch, *hp, steps, rec, nrec, rec_logits, rec_ids, graph_ok);
    // the loop ran to completion with this key, so every buffer it needs is allocated now: a lazy allocation during
    // it (drop_graph) must not cost the next call of the key its capture (config C4 allocated its bf16 conversion
    // buffer in the first call, which pushed the capture to the third)
    e->gkey_seen = true;
    if (logits_out && nrec)
        HIPCHK(hipMemcpyAsync(logits_out, rec_logits, rl * 4, logits_on_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                              e->st));
    if (ids_out && nrec) HIPCHK(hipMemcpyAsync(ids_out, rec_ids, ri * 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    if (e->timing) e->collect_timing();
    e->check_sdpl();
}

extern "C" {

int32_t suta_adapt(suta_engine* e, const float* wav, int32_t on_dev, int32_t norm, int32_t batch, int64_t n,
                   int32_t steps, const suta_hparams* hp, const int32_t* rec, int32_t nrec, float* logits_out,
                   int32_t logits_on_dev, int32_t* ids_out, int64_t* frames_out) {
    return guard([&] {
        adapt_impl(e, wav, on_dev, norm, batch, n, nullptr, n, steps, hp, rec, nrec, logits_out, logits_on_dev,
                   ids_out, frames_out);
    });
}

int32_t suta_adapt_varlen(suta_engine* e, const float* wav, int32_t on_dev, int32_t norm, int32_t batch,
                          const int64_t* n_samples, int64_t stride, int32_t steps, const suta_hparams* hp,
                          const int32_t* rec, int32_t nrec, float* logits_out, int32_t logits_on_dev, int32_t* ids_out,
                          int64_t* frames_out) {
    return guard([&] {
        if (!n_samples || batch < 1) throw SutaError(SUTA_ERR_ARG, "n_samples is null or batch < 1");
        int64_t nmax = 0;
        for (int b = 0; b < batch; ++b) nmax = std::max<int64_t>(nmax, n_samples[b]);
        if (stride < nmax) throw SutaError(SUTA_ERR_ARG, "stride < max(n_samples)");
        if (e->max_samples > 0 && nmax > e->max_samples)
            throw SutaError(SUTA_ERR_ARG, "n_samples > max_samples given to suta_create");
        // the layout length is `stride`: callers quantise it so repeated layouts reuse the captured step
        adapt_impl(e, wav, on_dev, norm, batch, stride, n_samples, stride, steps, hp, rec, nrec, logits_out,
                   logits_on_dev, ids_out, frames_out);
    });
}

int32_t suta_loss_grad(suta_engine* e, const float* logits, int32_t batch, int64_t frames, const suta_hparams* hp,
                       float* dlogits_out, float* loss_out) {
    return guard([&] {
        if (batch < 1 || frames < 1) throw SutaError(SUTA_ERR_ARG, "empty logits");
        HIPCHK(hipSetDevice(e->device));
        suta_latch_switches();  // SUTA_LOSS_WIDE picks the loss path
        const int V = e->c.V;
        const SdplTable* tab = hp->pl_coef > 0.f ? e->sdpl_table() : nullptr;  // refuses before any launch
        const size_t n = (size_t)batch * frames * V;
        const size_t nscr = suta_loss_scratch_floats(batch, frames, V);
        DevBuf buf;
        buf.alloc((nscr + 2 * n + batch) * sizeof(float));
        float* scr = buf.p;  // first: the wide path reads it as doubles (8-byte aligned)
        float* dl = scr + nscr;
        float* dd = dl + n;
        float* ls = dd + n;
        HIPCHK(hipMemcpyAsync(dl, logits, n * 4, hipMemcpyHostToDevice, e->st));
        LossHP lh{hp->temp, hp->em_coef, hp->div_coef, hp->reweight, hp->non_blank};
        e->timed(F_LOSS, [&] { launch_suta_loss(dl, batch, (int)frames, V, lh, nullptr, dd, ls, scr, e->st); });
        DevBuf sbuf;
        if (hp->pl_coef > 0.f) {
            if (frames > 2048) throw SutaError(SUTA_ERR_UNSUPPORTED, "T > 2048 frames");
            const long per = sdpl_scratch_floats((int)frames, V);
            sbuf.alloc(((size_t)batch * per + 64) * sizeof(float));
            HIPCHK(hipMemsetAsync(sbuf.p, 0, sbuf.bytes, e->st));
            int* err = reinterpret_cast<int*>(sbuf.p);
            e->timed(F_LOSS, [&] {
                launch_sdpl_loss(dl, batch, (int)frames, V, hp->pl_coef, nullptr, dd, ls, sbuf.p + 64, err, tab,
                                 e->st);
            });
            e->sdpl_used = true;
            e->sdpl_err = err;
        }
        HIPCHK(hipMemcpyAsync(dlogits_out, dd, n * 4, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipMemcpyAsync(loss_out, ls, (size_t)batch * 4, hipMemcpyDeviceToHost, e->st));
        HIPCHK(hipStreamSynchronize(e->st));
        if (e->timing) e->collect_timing();  // before the scratch buffers above go
        e->check_sdpl();
    });
}

int32_t suta_get_param(suta_engine* e, int32_t slot, const char* name, float* out, int64_t numel) {
    return guard([&] {
        auto it = e->tpi.find(name);
        if (it == e->tpi.end()) throw SutaError(SUTA_ERR_ARG, std::string("not a trainable tensor: ") + name);
        if (slot < 0 || slot >= e->max_batch) throw SutaError(SUTA_ERR_ARG, "slot out of range");
        const TP& t = e->tps[it->second];
        if (numel != t.numel) throw SutaError(SUTA_ERR_ARG, "numel mismatch");
        std::vector<float> h(t.numel);
        HIPCHK(hipStreamSynchronize(e->st));
        HIPCHK(hipMemcpy(h.data(), e->P + (long)slot * e->Pn + t.off, t.numel * 4, hipMemcpyDeviceToHost));
        if (t.conv_w) {
            const long co = t.shape[0], ci = t.shape[1], kk = t.shape[2];
            for (long o = 0; o < co; ++o)
                for (long i2 = 0; i2 < ci; ++i2)
                    for (long q = 0; q < kk; ++q) out[(o * ci + i2) * kk + q] = h[(q * ci + i2) * co + o];
        } else {
            std::memcpy(out, h.data(), t.numel * 4);
        }
    });
}

int32_t suta_param_info(suta_engine* e, const char* name, int32_t train_feature, int32_t bias_only, int32_t* k,
                        int64_t* numel) {
    return guard([&] {
        auto it = e->tpi.find(name);
        if (it == e->tpi.end()) {
            *k = 0;
            *numel = 0;
            return;
        }
        const TP& t = e->tps[it->second];
        *k = e->multiplicity(t, train_feature, bias_only);
        *numel = t.numel;
    });
}

int32_t suta_sync(suta_engine* e) { return guard([&] { HIPCHK(hipStreamSynchronize(e->st)); }); }

void* suta_stream(suta_engine* e) { return (void*)e->st; }

int32_t suta_set_timing(suta_engine* e, int32_t enable) {
    return guard([&] {
        e->timing = enable != 0;
        for (int i = 0; i < NFAM; ++i) {
            e->fam_ms[i] = 0;
            e->fam_n[i] = 0;
            e->fam_bytes[i] = 0;
        }
    });
}

int32_t suta_get_timing(suta_engine* e, double* ms, int64_t* n) {
    return guard([&] {
        e->collect_timing();
        for (int i = 0; i < 6; ++i) {
            ms[i] = e->fam_ms[i];
            n[i] = e->fam_n[i];
        }
        ms[F_GEMM] += e->fam_ms[F_ATTN];
        n[F_GEMM] += e->fam_n[F_ATTN];
        ms[F_NORM] += e->fam_ms[F_FRONT];
        n[F_NORM] += e->fam_n[F_FRONT];
    });
}

int32_t suta_get_timing_ex(suta_engine* e, int32_t nfam, double* ms, int64_t* n, double* alg_bytes) {
    return guard([&] {
        if (nfam < 1 || nfam > NFAM) throw SutaError(SUTA_ERR_ARG, "nfam outside [1, SUTA_TIMING_FAMILIES]");
        e->collect_timing();
        for (int i = 0; i < nfam; ++i) {
            ms[i] = e->fam_ms[i];
            n[i] = e->fam_n[i];
            if (alg_bytes) alg_bytes[i] = e->fam_bytes[i];
        }
    });
}

int32_t suta_set_precision(suta_engine* e, int32_t mode) {
    return guard([&] {
        if (mode != SUTA_PRECISION_FP32_MFMA && mode != SUTA_PRECISION_FP32_SPLIT_BF16 && mode != SUTA_PRECISION_BF16)
            throw SutaError(SUTA_ERR_ARG, "unknown precision mode");
        HIPCHK(hipSetDevice(e->device));
        if (mode == SUTA_PRECISION_BF16 && e->bf16_planes) e->build_weight_planes();
        e->gemm_mode = mode;
    });
}

int32_t suta_set_pseudo_labels(suta_engine* e, const int32_t* offsets, const int32_t* ids, const int32_t* kinds,
                               int32_t space_id) {
    return guard([&] {
        const int V = e->c.V;
        if (!offsets && !ids && !kinds) {  // back to the 960h rule
            std::vector<int> off, id, kind;
            int sp;
            e->default_pl_table(off, id, kind, sp);
            e->set_pl_table(off, id, kind, sp);
            e->pl_given = false;
            return;
        }
        if (!offsets || !kinds) throw SutaError(SUTA_ERR_ARG, "pseudo-label table: offsets or kinds is null");
        if (offsets[0] != 0) throw SutaError(SUTA_ERR_ARG, "pseudo-label table: offsets[0] != 0");
        for (int i = 0; i < V; ++i) {
            if (offsets[i + 1] < offsets[i]) throw SutaError(SUTA_ERR_ARG, "pseudo-label table: offsets not monotone");
            if (kinds[i] < SDPL_KIND_NORMAL || kinds[i] > SDPL_KIND_FAIL)
                throw SutaError(SUTA_ERR_ARG, "pseudo-label table: kind out of range");
            if (kinds[i] != SDPL_KIND_NORMAL && offsets[i + 1] != offsets[i])
                throw SutaError(SUTA_ERR_ARG, "pseudo-label table: only a normal token has an expansion");
        }
        const int n = offsets[V];
        if (n > 0 && !ids) throw SutaError(SUTA_ERR_ARG, "pseudo-label table: ids is null");
        for (int q = 0; q < n; ++q)
            if (ids[q] <= 0 || ids[q] >= V)
                throw SutaError(SUTA_ERR_ARG, "pseudo-label table: expansion id outside [1, vocab_size)");
        if (space_id < -1 || space_id == 0 || space_id >= V)
            throw SutaError(SUTA_ERR_ARG, "pseudo-label table: space_id outside {-1} and [1, vocab_size)");
        e->set_pl_table(std::vector<int>(offsets, offsets + V + 1), std::vector<int>(ids, ids + n),
                        std::vector<int>(kinds, kinds + V), space_id);
        e->pl_given = true;
    });
}

int32_t suta_set_graphs(suta_engine* e, int32_t enable) {
    return guard([&] { e->use_graphs = enable != 0; });
}

int32_t suta_get_graph_stats(suta_engine* e, int32_t* last_mode, int64_t* captures, int64_t* launches) {
    return guard([&] {
        if (last_mode) *last_mode = e->last_loop_mode;
        if (captures) *captures = e->graph_captures;
        if (launches) *launches = e->graph_launches;
    });
}

int32_t suta_get_workspace_bytes(suta_engine* e, int64_t* bytes_out) {
    return guard([&] { *bytes_out = (int64_t)e->plan.bytes; });
}

int32_t suta_set_census(int32_t enable) {
    return guard([&] { gemm_census_enable(enable != 0); });
}

int32_t suta_get_census(char* buf, int64_t cap, int64_t* needed) {
    return guard([&] {
        const std::string t = gemm_census_text();
        if (needed) *needed = (int64_t)t.size() + 1;
        if (!buf || cap < (int64_t)t.size() + 1) throw SutaError(SUTA_ERR_ARG, "census buffer too small");
        memcpy(buf, t.c_str(), t.size() + 1);
    });
}

}  // extern "C"
