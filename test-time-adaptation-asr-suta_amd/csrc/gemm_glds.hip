// LDS-DMA fp32 MFMA GEMM family (the default exact path).
#include "gemm_kernels.h"

// K-step x stages: 32 x 2 (default), 64 x 2, 16 x 4, 16 x 3, 32 x 3 (benchmark variants)
void gemm_run_glds(int BM, int BN, int bk, int stages, const GemmParams& p, dim3 grid, hipStream_t st) {
    if (bk == 64 && stages == 2) launch_glds_tile<64, 2>(BM, BN, p, grid, st);
    else if (bk == 16 && stages == 4) launch_glds_tile<16, 4>(BM, BN, p, grid, st);
    else if (bk == 16 && stages == 3) launch_glds_tile<16, 3>(BM, BN, p, grid, st);
    else if (bk == 32 && stages == 3) launch_glds_tile<32, 3>(BM, BN, p, grid, st);
    else if (bk == 32 && stages == 2) launch_glds_tile<32, 2>(BM, BN, p, grid, st);
    else throw std::invalid_argument("glds: no such stage variant");
}
