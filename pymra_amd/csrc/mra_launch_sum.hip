// mra_launch_sum.hip - MRA_KERNEL_SUM (covariance mode 5: a sum of up to four closed-form kernels, cov_sum_of_dist2) in the batched GEMM
// kernels: the <EPI_COV, DIM, 5> instances of k_gemm_nt, k_gemm_nt_lds and k_leaf_gemm for DIM = 1, 2 and 3, and their launches.
//
// As mra_launch_nu3.hip does for the 3-D quadrature, this unit includes the kernel templates under names of their own (k_*_sum) and
// instantiates nothing but mode 5 - here for all three dimensions, so that no existing unit gains a kernel: the DIM = 3 list of the
// closed forms stays closed (tests/test_resource_usage_3d.py) and every kernel from before keeps its object code by construction.
// tests/test_kernel_sum_resources.py holds the instances to their own rule: no scratch, no spilled VGPRs, no AGPRs.
// The row and site kernels of mode 5 are in mra_launch_sum2.hip.  The dispatch chains of mra_launch_gemm.hip hand their mode-5 case
// to the functions below, with the grids they computed.
#define MRA_KERNELS_TEMPLATES_ONLY
#define k_gemm_nt k_gemm_nt_sum
#define k_gemm_nt_lds k_gemm_nt_lds_sum
#define k_leaf_gemm k_leaf_gemm_sum
#include "mra_plan_types.h"

// Waves per SIMD.  k_gemm_nt and k_gemm_nt_lds keep the closed forms' four (101 to 128 registers).  The wide leaf residual (4) and the
// one-launch prior level (3) spill with the component loop in their epilogue - 4 to 6 and 19 to 20 VGPRs - so both run two waves per
// SIMD, the shapes the Kanter taper and MRA_KERNEL_MATERN use (144 to 198 registers, no scratch).
#define MRA_SUM_LG_WPE 2
#define MRA_SUM_PL_WPE 2

#define MRA_SUM_DIMS(CALL) do { if (pl->d == 1) { CALL(1); } else if (pl->d == 3) { CALL(3); } else { CALL(2); } } while (0)

void mra_sum_gemm(mra_plan* pl, bool lds, dim3 grid, const GemmProb* probs, unsigned gxs, unsigned gy, unsigned S) {
#define MRA_SUM_LDS(D) hipLaunchKernelGGL((k_gemm_nt_lds<EPI_COV, D, 5>), grid, dim3(256), 0, pl->stream, probs, pl->kp, gxs, gy, S)
#define MRA_SUM_DIRECT(D) hipLaunchKernelGGL((k_gemm_nt<EPI_COV, D, 5>), grid, dim3(256), 0, pl->stream, probs, pl->kp, gxs, gy, S)
    if (lds) MRA_SUM_DIMS(MRA_SUM_LDS);
    else MRA_SUM_DIMS(MRA_SUM_DIRECT);
#undef MRA_SUM_LDS
#undef MRA_SUM_DIRECT
}

// the leaves' residual in its two shapes (launch_leaf_gemm) and the one-launch prior level (mra_launch_prior_level)
void mra_sum_leaf_gemm(mra_plan* pl, bool wide, dim3 grid, const GemmProb* probs) {
#define MRA_SUM_WIDE(D) hipLaunchKernelGGL((k_leaf_gemm<EPI_COV, D, 5, 1, 8, 512, MRA_SUM_LG_WPE>), grid, dim3(512), 0, pl->stream, probs, pl->kp)
#define MRA_SUM_NARROW(D) hipLaunchKernelGGL((k_leaf_gemm<EPI_COV, D, 5, 2, 7, 256, 2>), grid, dim3(256), 0, pl->stream, probs, pl->kp)
    if (wide) MRA_SUM_DIMS(MRA_SUM_WIDE);
    else MRA_SUM_DIMS(MRA_SUM_NARROW);
#undef MRA_SUM_WIDE
#undef MRA_SUM_NARROW
}
void mra_sum_prior_level(mra_plan* pl, dim3 grid, const GemmProb* probs) {
#define MRA_SUM_PL(D) hipLaunchKernelGGL((k_leaf_gemm<EPI_COV, D, 5, 2, 4, 256, (D == 3 ? 2 : MRA_SUM_PL_WPE), 1>), grid, dim3(256), 0, pl->stream, probs, pl->kp)
    MRA_SUM_DIMS(MRA_SUM_PL);
#undef MRA_SUM_PL
}
