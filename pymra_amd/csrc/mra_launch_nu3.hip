// mra_launch_nu3.hip - MRA_KERNEL_MATERN (covariance mode 4, the quadrature of matern_nu_of_t) on 3-D coordinates: the <DIM = 3, MODE = 4>
// instances of every kernel that is templated on the covariance, and their launches.
//
// The DIM = 3 instances of the closed-form covariances are a closed list with a register budget of its own (DESIGN.md section 17,
// tests/test_resource_usage_3d.py).  The quadrature's 3-D instances are kept apart from it: this unit includes the same kernel
// templates under names of their own (k_*_nu3), instantiates nothing but <3, 4>, and tests/test_matern_nu_resources.py holds them to
// their own rule (no scratch, no spilled VGPRs).  No other unit sees these names, so every other kernel keeps its object code.
// The other units' dispatch chains hand their <3, 4> case to the functions below, with the grids they computed.
#define MRA_KERNELS_TEMPLATES_ONLY
#define MRA_COV_TEMPLATES_ONLY
#define MRA_GEMM_LDS_WPE 3          /* k_gemm_nt_lds<COV, 3, 4>: 132 registers; at four waves per SIMD (128) its epilogue spills 4 */
#define k_gemm_nt k_gemm_nt_nu3
#define k_gemm_nt_lds k_gemm_nt_lds_nu3
#define k_leaf_gemm k_leaf_gemm_nu3
#define k_solve_rows k_solve_rows_nu3
#define k_cov_rows k_cov_rows_nu3
#define k_site_basis k_site_basis_nu3
#define k_site_leaf k_site_leaf_nu3
#define k_site_mean k_site_mean_nu3
#define k_site_gram k_site_gram_nu3
#define k_site_inert k_site_inert_nu3
#define k_site_leaf_gram k_site_leaf_gram_nu3
#define k_cv_gram k_cv_gram_nu3
#include "mra_solve_kernels.h"
#include "mra_cov_kernels.h"
#include "mra_site_kernels.h"
#include "mra_launch_sites.inc"

void mra_nu3_gemm(mra_plan* pl, bool lds, dim3 grid, const GemmProb* probs, unsigned gxs, unsigned gy, unsigned S) {
    if (lds) hipLaunchKernelGGL((k_gemm_nt_lds<EPI_COV, 3, 4>), grid, dim3(256), 0, pl->stream, probs, pl->kp, gxs, gy, S);
    else hipLaunchKernelGGL((k_gemm_nt<EPI_COV, 3, 4>), grid, dim3(256), 0, pl->stream, probs, pl->kp, gxs, gy, S);
}

// the leaves' residual (two waves per SIMD in either shape, as the Kanter taper) and the one-launch prior level
void mra_nu3_leaf_gemm(mra_plan* pl, bool wide, dim3 grid, const GemmProb* probs) {
    if (wide) hipLaunchKernelGGL((k_leaf_gemm<EPI_COV, 3, 4, 1, 8, 512, 2>), grid, dim3(512), 0, pl->stream, probs, pl->kp);
    else hipLaunchKernelGGL((k_leaf_gemm<EPI_COV, 3, 4, 2, 7, 256, 2>), grid, dim3(256), 0, pl->stream, probs, pl->kp);
}
void mra_nu3_prior_level(mra_plan* pl, dim3 grid, const GemmProb* probs) {
    hipLaunchKernelGGL((k_leaf_gemm<EPI_COV, 3, 4, 2, 4, 256, 2, 1>), grid, dim3(256), 0, pl->stream, probs, pl->kp);
}

// launch_rows<3> of mra_launch_solve.hip and launch_cov_rows<3> of mra_launch_cov.hip
void mra_nu3_solve_rows(mra_plan* pl) {
    mra_plan::Solver& S = pl->slv;
    hipLaunchKernelGGL((k_solve_rows<3, 4>), dim3((unsigned)((pl->P / 16 + 3) / 4)), dim3(256), 0, pl->stream, S.leaves.p, pl->maps.tile_leaf.p, pl->W.p,
                       (long)pl->ldw, pl->X.p, pl->maps.rep.p, pl->kp, S.out.p, pl->P);
}
void mra_nu3_cov_rows(mra_plan* pl) {
    mra_plan::Cov& V = pl->cov;
    hipLaunchKernelGGL((k_cov_rows<3, 4>), dim3((unsigned)((pl->P / 16 + 3) / 4)), dim3(256), 0, pl->stream, V.leaves.p, pl->maps.tile_leaf.p, pl->W.p,
                       (long)pl->ldw, pl->X.p, pl->maps.rep.p, pl->maps.knot.p, pl->kp, V.ab.p, V.out.p, pl->P);
}

// MRA_SITES_DISPATCH's case <3, 4> (mra_launch_sites.hip)
void launch_basis_nu3(mra_plan* pl, long n) { launch_basis<3, 4>(pl, n); }
void launch_leaf_nu3(mra_plan* pl, long n) { launch_leaf<3, 4>(pl, n); }
void launch_mean_nu3(mra_plan* pl, long n, int nc) { launch_mean<3, 4>(pl, n, nc); }
void launch_gram_nu3(mra_plan* pl, long n, long tile0, long rows, bool post) { launch_gram<3, 4>(pl, n, tile0, rows, post); }
void launch_leaf_gram_nu3(mra_plan* pl, long n, int nt_max, bool post) { launch_leaf_gram<3, 4>(pl, n, nt_max, post); }
void launch_cv_gram_nu3(mra_plan* pl, long n, int nt_max) { launch_cv_gram<3, 4>(pl, n, nt_max); }
