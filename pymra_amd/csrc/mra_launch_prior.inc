// mra_launch_prior.inc - dispatch of the prior cascade kernels over block width, depth and covariance family for ONE spatial
// dimension (MRA_TU_DIM) and one kernel (MRA_TU_KNOT: k_knot_chain, else k_prior_cascade in row and knot mode).  Included by
// the six mra_launch_prior_*.hip translation units: the 108 instantiations are most of the library's compile time, split
// six ways they build in parallel.
#define MRA_KERNELS_TEMPLATES_ONLY
#include "mra_plan_types.h"

#ifndef MRA_TU_KNOT
template <int CWT, int NLMAX, int MODE>
static void launch_cascade_inst(mra_plan* pl, const CascadeArgs& ar) {
    constexpr int DIM = MRA_TU_DIM;
    // (the row pass with twelve waves per workgroup, three per SIMD, was measured at C3: 168 registers per lane spill
    // 264 bytes and 64 row tiles do not divide over twelve waves -- 1.44 ms against 1.29 ms with eight)
    ensure_big_lds(pl, {(const void*)k_prior_cascade<CWT, NLMAX, DIM, MODE, true>, (const void*)k_prior_cascade<CWT, NLMAX, DIM, MODE, false>});
    if (pl->prepare_only) return;
    if (pl->cascade_stage_all)
        hipLaunchKernelGGL((k_prior_cascade<CWT, NLMAX, DIM, MODE, true>), dim3((unsigned)ar.n_wg), dim3(ar.knot_mode ? ar.knot_threads : 512),
                           std::max<size_t>(pl->cascade_lds_all, 40960), pl->stream, ar, pl->kp);
    else
        hipLaunchKernelGGL((k_prior_cascade<CWT, NLMAX, DIM, MODE, false>), dim3((unsigned)ar.n_wg), dim3(ar.knot_mode ? ar.knot_threads : 64 * pl->cascade_wpw),
                           std::max<size_t>(pl->cascade_lds, 40960), pl->stream, ar, pl->kp);
}
template <int CWT, int NLMAX>
static void launch_cascade(mra_plan* pl, const CascadeArgs& ar) {
    if (ar.n_wg <= 0) return;
    const int mode = pl->kp.mode;
    if (mode == 0) launch_cascade_inst<CWT, NLMAX, 0>(pl, ar);
    else if (mode == 1) launch_cascade_inst<CWT, NLMAX, 1>(pl, ar);
    else if (mode == 2) launch_cascade_inst<CWT, NLMAX, 2>(pl, ar);
    else if (mode == 3) launch_cascade_inst<CWT, NLMAX, 3>(pl, ar);
    else mra_bad_mode("the fused prior cascade", mode);      // (mode 4, MRA_KERNEL_MATERN, has no fused instance: path_of keeps it off this path)
}
void MRA_TU_NAME(mra_plan* pl, const CascadeArgs& ar) {
    if (pl->CWT == 1) launch_cascade<1, 8>(pl, ar);
    else if (pl->CWT == 2) launch_cascade<2, 8>(pl, ar);
    else launch_cascade<4, 4>(pl, ar);
}
#else
template <int CWT, int NLMAX, int MODE>
static void launch_knot_chain_inst(mra_plan* pl, const KnotChainArgs& ka) {
    constexpr int DIM = MRA_TU_DIM;
    ensure_big_lds(pl, {(const void*)k_knot_chain<CWT, NLMAX, DIM, MODE>});
    if (pl->prepare_only) return;
    hipLaunchKernelGGL((k_knot_chain<CWT, NLMAX, DIM, MODE>), dim3((unsigned)pl->lev[ka.nl - 1].nodes.size()), dim3(256), pl->knot_chain_lds,
                       pl->stream, ka, pl->kp);
}
template <int CWT, int NLMAX>
static void launch_knot_chain_cw(mra_plan* pl, const KnotChainArgs& ka) {
    const int mode = pl->kp.mode;
    if (mode == 0) launch_knot_chain_inst<CWT, NLMAX, 0>(pl, ka);
    else if (mode == 1) launch_knot_chain_inst<CWT, NLMAX, 1>(pl, ka);
    else if (mode == 2) launch_knot_chain_inst<CWT, NLMAX, 2>(pl, ka);
    else if (mode == 3) launch_knot_chain_inst<CWT, NLMAX, 3>(pl, ka);
    else mra_bad_mode("the fused knot chain", mode);
}
void MRA_TU_NAME(mra_plan* pl, const KnotChainArgs& ka) {
    if (pl->CWT == 1) launch_knot_chain_cw<1, 8>(pl, ka);
    else if (pl->CWT == 2) launch_knot_chain_cw<2, 8>(pl, ka);
    else launch_knot_chain_cw<4, 4>(pl, ka);
}
#endif
