// LDS-DMA stages + register bf16 conversion: bf16 GEMM (1 product) and the register-split x6 (6 products).
#include "gemm_kernels.h"

void gemm_run_gbf(int BM, int BN, int bk, int nprod, const GemmParams& p, dim3 grid, hipStream_t st) {
    if (nprod == 1) {
        if (bk == 64) launch_gbf_tile<64, 2, 1>(BM, BN, p, grid, st);
        else launch_gbf_tile<32, 2, 1>(BM, BN, p, grid, st);
    } else {
        if (bk == 64) launch_gbf_tile<64, 2, 6>(BM, BN, p, grid, st);
        else launch_gbf_tile<32, 2, 6>(BM, BN, p, grid, st);
    }
}
