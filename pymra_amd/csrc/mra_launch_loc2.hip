// mra_launch_loc2.hip - MRA_KERNEL_LOCAL (covariance mode 6) in the kernels on the retained factors: the <DIM, 6> instances of k_solve_rows,
// k_cov_rows and the seven site and cross-validation kernels for DIM = 2 and 3, under names of their own (k_*_loc), and their
// launches.  The second half of mra_launch_loc.hip (see there): nothing but mode 6 is instantiated here, and no other unit sees these
// names.
#define MRA_KERNELS_TEMPLATES_ONLY
#define MRA_COV_TEMPLATES_ONLY
#define k_solve_rows k_solve_rows_loc
#define k_cov_rows k_cov_rows_loc
#define k_site_basis k_site_basis_loc
#define k_site_leaf k_site_leaf_loc
#define k_site_mean k_site_mean_loc
#define k_site_gram k_site_gram_loc
#define k_site_inert k_site_inert_loc
#define k_site_leaf_gram k_site_leaf_gram_loc
#define k_cv_gram k_cv_gram_loc
#include "mra_solve_kernels.h"
#include "mra_cov_kernels.h"
#include "mra_site_kernels.h"
#include "mra_launch_sites.inc"

#define MRA_LOC_DIMS(CALL) do { if (pl->d == 3) { CALL(3); } else if (pl->d == 2) { CALL(2); } else mra_bad_mode("MRA_KERNEL_LOCAL on 1-D coordinates", 6); } while (0)

// launch_rows of mra_launch_solve.hip and launch_cov_rows of mra_launch_cov.hip
void mra_loc_solve_rows(mra_plan* pl) {
    mra_plan::Solver& S = pl->slv;
#define MRA_LOC_ROWS(D) hipLaunchKernelGGL((k_solve_rows<D, 6>), dim3((unsigned)((pl->P / 16 + 3) / 4)), dim3(256), 0, pl->stream, S.leaves.p, pl->maps.tile_leaf.p, \
                                           pl->W.p, (long)pl->ldw, pl->X.p, pl->maps.rep.p, pl->kp, S.out.p, pl->P)
    MRA_LOC_DIMS(MRA_LOC_ROWS);
#undef MRA_LOC_ROWS
}
void mra_loc_cov_rows(mra_plan* pl) {
    mra_plan::Cov& V = pl->cov;
#define MRA_LOC_ROWS(D) hipLaunchKernelGGL((k_cov_rows<D, 6>), dim3((unsigned)((pl->P / 16 + 3) / 4)), dim3(256), 0, pl->stream, V.leaves.p, pl->maps.tile_leaf.p, \
                                           pl->W.p, (long)pl->ldw, pl->X.p, pl->maps.rep.p, pl->maps.knot.p, pl->kp, V.ab.p, V.out.p, pl->P)
    MRA_LOC_DIMS(MRA_LOC_ROWS);
#undef MRA_LOC_ROWS
}

// MRA_SITES_DISPATCH's mode-6 case (mra_launch_sites.hip)
void launch_basis_loc(mra_plan* pl, long n) {
#define MRA_LOC_CALL(D) launch_basis<D, 6>(pl, n)
    MRA_LOC_DIMS(MRA_LOC_CALL);
#undef MRA_LOC_CALL
}
void launch_leaf_loc(mra_plan* pl, long n) {
#define MRA_LOC_CALL(D) launch_leaf<D, 6>(pl, n)
    MRA_LOC_DIMS(MRA_LOC_CALL);
#undef MRA_LOC_CALL
}
void launch_mean_loc(mra_plan* pl, long n, int nc) {
#define MRA_LOC_CALL(D) launch_mean<D, 6>(pl, n, nc)
    MRA_LOC_DIMS(MRA_LOC_CALL);
#undef MRA_LOC_CALL
}
void launch_gram_loc(mra_plan* pl, long n, long tile0, long rows, bool post) {
#define MRA_LOC_CALL(D) launch_gram<D, 6>(pl, n, tile0, rows, post)
    MRA_LOC_DIMS(MRA_LOC_CALL);
#undef MRA_LOC_CALL
}
void launch_leaf_gram_loc(mra_plan* pl, long n, int nt_max, bool post) {
#define MRA_LOC_CALL(D) launch_leaf_gram<D, 6>(pl, n, nt_max, post)
    MRA_LOC_DIMS(MRA_LOC_CALL);
#undef MRA_LOC_CALL
}
void launch_cv_gram_loc(mra_plan* pl, long n, int nt_max) {
#define MRA_LOC_CALL(D) launch_cv_gram<D, 6>(pl, n, nt_max)
    MRA_LOC_DIMS(MRA_LOC_CALL);
#undef MRA_LOC_CALL
}
