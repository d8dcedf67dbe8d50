// Register-staged fp32 MFMA GEMM family (operands that are not 16-B aligned / k-contiguous with K % 4).
#include "gemm_kernels.h"

void gemm_run_f32(int BM, int BN, int stages, const GemmParams& p, dim3 grid, hipStream_t st) {
    with_tile128(BM, BN, [&](auto bm, auto bn) {
        if (stages == 2) launch_tile<decltype(bm)::value, decltype(bn)::value, 2>(p, grid, st);
        else launch_tile<decltype(bm)::value, decltype(bn)::value, 1>(p, grid, st);
    });
}
