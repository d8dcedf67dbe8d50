// LayerNorm over the last dim D (<= 2048) of B * rows_per_utt rows (norm.hip): one description of a LayerNorm for
// its forward and its backward, typed operands, and a pure route that names the kernel before anything is launched.
#pragma once
#include "common.h"

// What the two passes of one LayerNorm share.  gamma / beta of utterance (row / rows_per_utt) at pstride; dgamma /
// dbeta (may be null) summed per utterance at gstride.  gelu: y = gelu(LN(x)) (the layer-mode conv stack).  Saved by
// the forward: rstd and either x-hat or, when xhat is null, the row means (the backward then recomputes x-hat
// from the LayerNorm's stored input).
struct LnSite {
    const float *g, *beta;
    float *dgamma, *dbeta;
    long pstride, gstride;
    int rows_per_utt, B, D;
    float eps;
    bool gelu;
    float *xhat, *mean, *rstd;
};
struct LnIn { const float* f32; const void* bf16; };  // exactly one set
struct LnOut { float* f32; void* bf16; };  // either or both (bf16: the plane of the GEMM that reads the result)
inline LnIn ln_f32(const float* p) { return {p, nullptr}; }
inline LnIn ln_bf16(const void* p) { return {nullptr, p}; }
inline LnOut ln_out(float* f, void* plane = nullptr) { return {f, plane}; }
inline LnOut ln_plane(void* plane) { return {nullptr, plane}; }
struct LnFwd { LnIn x; LnOut y; };
// The conv layer's other readers of dx, summed by the fused conv backward: the bias gradient (may be null) and, with
// ktaps taps (conv0), the weight gradient dw[k][c] = sum_t wave[hop t + k] dx[t][c] (wave_stride per utterance).
struct LnConvGrads {
    float *dbias, *dw;
    const float* wave;
    long wave_stride; int hop, ktaps;
};
// gin = dy (times gelu'(xhat g + beta) when site.gelu); dx = LN-bwd(gin) (times gelu'(post_aux)) (+ resid).
// x: the LayerNorm's input, read when x-hat is recomputed.  part: part_floats floats of partial sums.
struct LnBwd {
    LnIn dy, x;
    const float *post_aux, *resid;
    LnOut dx;
    float* part;
    long part_floats;
    const LnConvGrads* conv;  // null: the plain backward
};

enum class LnKernel { None, Scalar, Vec, ConvBwd };
// None: conv gradients were asked for and the fused conv backward does not take these operands (nothing is launched;
// the caller runs the plain backward, launch_colsum and its weight-gradient GEMM).  Scalar: NPL = npl; Vec: NV = nv
// with GV / XB / DYB / RPW / FG; ConvBwd: NV 2 with GV / XB / DYB / FG and KT = kt.
struct LnRoute {
    LnKernel kind = LnKernel::None;
    int npl = 0, nv = 0, rpw = 1, kt = 0;
    bool gv = false, xb = false, dyb = false, fg = false;
    int gx = 0, gy = 1, nchunk = 0, crows = 0;  // grid; backward: row chunks per utterance, rows per chunk
    long part_floats = 0;        // partial sums the launch writes
    bool plane_in_kernel = false;  // the bf16 copy is written by the kernel (else by a following launch_to_bf16)
    bool sums_conv_grads = false;  // the kernel sums conv->dbias and conv->dw itself
};
bool ln_vec_width(int D);  // the widths of the vectorised kernels (D = 256 NV)
long layernorm_bwd_conv_part_floats(int B, int rows_per_utt, int D, int ktaps);
// Pure: the arguments and the latched switches (ln_rpw, fast_gelu) in, the launch out; std::invalid_argument /
// std::runtime_error for operands no kernel takes.
LnRoute ln_fwd_route(const LnSite& s, const LnFwd& io);
LnRoute ln_bwd_route(const LnSite& s, const LnBwd& io);
void ln_forward(const LnSite& s, const LnFwd& io, hipStream_t st);
void ln_backward(const LnSite& s, const LnBwd& io, hipStream_t st);
