// mra_launch_loc.hip - MRA_KERNEL_LOCAL (covariance mode 6: local ranges in the last coordinate column, cov_local) in the batched GEMM
// kernels: the <EPI_COV, DIM, 6> instances of k_gemm_nt, k_gemm_nt_lds and k_leaf_gemm for DIM = 2 (rows (x, lam)) and DIM = 3 (rows
// (x, y, lam)), and their launches.
//
// As mra_launch_sum.hip does for MRA_KERNEL_SUM, this unit includes the kernel templates under names of their own (k_*_loc) and
// instantiates nothing but mode 6, so that no existing unit gains a kernel: the DIM = 3 list of the closed forms stays closed
// (tests/test_resource_usage_3d.py) and every kernel from before keeps its object code by construction.
// tests/test_local_range_resources.py holds the instances to their own rule: no scratch, no spilled VGPRs, no AGPRs.
// The row and site kernels of mode 6 are in mra_launch_loc2.hip.  The dispatch chains of mra_launch_gemm.hip hand their mode-6 case
// to the functions below, with the grids they computed.  A plan with d = 1 never has this mode (mra_plan_set_kernel refuses it).
#define MRA_KERNELS_TEMPLATES_ONLY
#define k_gemm_nt k_gemm_nt_loc
#define k_gemm_nt_lds k_gemm_nt_lds_loc
#define k_leaf_gemm k_leaf_gemm_loc
#include "mra_plan_types.h"

// Waves per SIMD (DESIGN.md section 25 has the register counts).
#define MRA_LOC_LG_WPE 2
#define MRA_LOC_PL_WPE 2

#define MRA_LOC_DIMS(CALL) do { if (pl->d == 3) { CALL(3); } else if (pl->d == 2) { CALL(2); } else mra_bad_mode("MRA_KERNEL_LOCAL on 1-D coordinates", 6); } while (0)

void mra_loc_gemm(mra_plan* pl, bool lds, dim3 grid, const GemmProb* probs, unsigned gxs, unsigned gy, unsigned S) {
#define MRA_LOC_LDS(D) hipLaunchKernelGGL((k_gemm_nt_lds<EPI_COV, D, 6>), grid, dim3(256), 0, pl->stream, probs, pl->kp, gxs, gy, S)
#define MRA_LOC_DIRECT(D) hipLaunchKernelGGL((k_gemm_nt<EPI_COV, D, 6>), grid, dim3(256), 0, pl->stream, probs, pl->kp, gxs, gy, S)
    if (lds) MRA_LOC_DIMS(MRA_LOC_LDS);
    else MRA_LOC_DIMS(MRA_LOC_DIRECT);
#undef MRA_LOC_LDS
#undef MRA_LOC_DIRECT
}

// the leaves' residual in its two shapes (launch_leaf_gemm) and the one-launch prior level (mra_launch_prior_level)
void mra_loc_leaf_gemm(mra_plan* pl, bool wide, dim3 grid, const GemmProb* probs) {
#define MRA_LOC_WIDE(D) hipLaunchKernelGGL((k_leaf_gemm<EPI_COV, D, 6, 1, 8, 512, MRA_LOC_LG_WPE>), grid, dim3(512), 0, pl->stream, probs, pl->kp)
#define MRA_LOC_NARROW(D) hipLaunchKernelGGL((k_leaf_gemm<EPI_COV, D, 6, 2, 7, 256, 2>), grid, dim3(256), 0, pl->stream, probs, pl->kp)
    if (wide) MRA_LOC_DIMS(MRA_LOC_WIDE);
    else MRA_LOC_DIMS(MRA_LOC_NARROW);
#undef MRA_LOC_WIDE
#undef MRA_LOC_NARROW
}
void mra_loc_prior_level(mra_plan* pl, dim3 grid, const GemmProb* probs) {
#define MRA_LOC_PL(D) hipLaunchKernelGGL((k_leaf_gemm<EPI_COV, D, 6, 2, 4, 256, MRA_LOC_PL_WPE, 1>), grid, dim3(256), 0, pl->stream, probs, pl->kp)
    MRA_LOC_DIMS(MRA_LOC_PL);
#undef MRA_LOC_PL
}
