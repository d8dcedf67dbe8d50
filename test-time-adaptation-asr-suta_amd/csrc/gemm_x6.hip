// Register-staged bf16-plane GEMM family: x6 (3 planes, 6 products) and its one-plane bf16 form.
#include "gemm_kernels.h"

// npl 3: K-step 32 on one LDS stage, or 16 double-buffered; npl 1 (bf16 products): K-step 32, one stage, and the big
// tiles 256 x 128 / 128 x 256 (wave tile 128 x 64 / 64 x 128: 1.3x fewer L2 bytes per flop)
void gemm_run_x6(int BM, int BN, int bk, int npl, const GemmParams& p, dim3 grid, hipStream_t st) {
    if (npl == 1 && BM == 256 && BN == 128) return launch_x6<256, 128, 32, 1, 1>(p, grid, st);
    if (npl == 1 && BM == 128 && BN == 256) return launch_x6<128, 256, 32, 1, 1>(p, grid, st);
    with_tile128(BM, BN, [&](auto bm, auto bn) {
        constexpr int M = decltype(bm)::value, N = decltype(bn)::value;
        if (npl == 1) launch_x6<M, N, 32, 1, 1>(p, grid, st);
        else if (bk == 16) launch_x6<M, N, 16, 2>(p, grid, st);
        else launch_x6<M, N, 32, 1>(p, grid, st);
    });
}
