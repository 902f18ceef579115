// mra_launch_sites.inc - the launches of the site kernels that are templated on dimension and covariance (k_site_basis, k_site_leaf,
// k_site_mean, k_site_gram, k_site_inert + k_site_leaf_gram, k_cv_gram), one function template each.  Included by mra_launch_sites.hip
// (every instance but one) and by mra_launch_nu3.hip (DIM = 3 with MRA_KERNEL_MATERN, where the kernels carry names of their own).
template <int DIM, int MODE>
static void launch_basis(mra_plan* pl, long n) {
    mra_plan::Sites& T = pl->sit;
    hipLaunchKernelGGL((k_site_basis<DIM, MODE>), dim3((unsigned)n), dim3(64), 0, pl->stream, pl->slv.leaves.p, T.nodes.p, T.chain_ptr.p, T.chain.p,
                       T.tleaf.p, T.xs.p, pl->W.p, (long)pl->ldw, pl->X.p, pl->kp, T.a.p, (long)T.anc_max * 16);
}

template <int DIM, int MODE>
static void launch_leaf(mra_plan* pl, long n) {
    mra_plan::Sites& T = pl->sit;
    hipLaunchKernelGGL((k_site_leaf<DIM, MODE>), dim3((unsigned)n), dim3(64), 0, pl->stream, pl->slv.leaves.p, T.tleaf.p, T.xs.p, pl->X.p, pl->kp,
                       T.a.p, T.b.p, (long)T.anc_max * 16, T.t.p, (long)T.nop_max * 16, T.var.p);
}

template <int DIM, int MODE>
static void launch_mean(mra_plan* pl, long n, int nc) {
    mra_plan::Sites& T = pl->sit;
    hipLaunchKernelGGL((k_site_mean<DIM, MODE>), dim3((unsigned)n), dim3(64), 0, pl->stream, pl->slv.leaves.p, T.tleaf.p, T.xs.p, pl->X.p, pl->kp,
                       T.a.p, (long)T.anc_max * 16, nc, T.mean.p, n * 16);
}

template <int DIM, int MODE>
static void launch_gram(mra_plan* pl, long n, long tile0, long rows, bool post) {
    mra_plan::Sites& T = pl->sit;
    const dim3 grid((unsigned)n, (unsigned)rows);
    if (post)
        hipLaunchKernelGGL((k_site_gram<DIM, MODE, true>), grid, dim3(64), 0, pl->stream, pl->slv.leaves.p, T.nodes.p, T.chain_ptr.p, T.chain.p, T.tleaf.p,
                           T.xs.p, pl->kp, T.a.p, T.b.p, (long)T.anc_max * 16, T.t.p, (long)T.nop_max * 16, tile0, T.gram.p, n * 16);
    else
        hipLaunchKernelGGL((k_site_gram<DIM, MODE, false>), grid, dim3(64), 0, pl->stream, pl->slv.leaves.p, T.nodes.p, T.chain_ptr.p, T.chain.p, T.tleaf.p,
                           T.xs.p, pl->kp, T.a.p, T.b.p, (long)T.anc_max * 16, T.t.p, (long)T.nop_max * 16, tile0, T.gram.p, n * 16);
}

template <int DIM, int MODE>
static void launch_leaf_gram(mra_plan* pl, long n, int nt_max, bool post) {
    mra_plan::Sites& T = pl->sit;
    const dim3 grid((unsigned)n, (unsigned)nt_max);
    const long as = (long)T.anc_max * 16, ts = (long)T.nop_max * 16;
    if (post) {
        hipLaunchKernelGGL((k_site_inert<MODE, true>), dim3((unsigned)n), dim3(64), 0, pl->stream, pl->slv.leaves.p, T.tleaf.p, pl->kp, T.a.p, as, T.t.p, ts,
                           T.sslot.p, T.live.p);
        hipLaunchKernelGGL((k_site_leaf_gram<DIM, MODE, true>), grid, dim3(64), 0, pl->stream, pl->slv.leaves.p, T.tleaf.p, T.dtile.p, T.xs.p, pl->kp,
                           T.a.p, as, T.t.p, ts, T.live.p, T.G.p);
    } else {
        hipLaunchKernelGGL((k_site_inert<MODE, false>), dim3((unsigned)n), dim3(64), 0, pl->stream, pl->slv.leaves.p, T.tleaf.p, pl->kp, T.a.p, as, T.t.p, ts,
                           T.sslot.p, T.live.p);
        hipLaunchKernelGGL((k_site_leaf_gram<DIM, MODE, false>), grid, dim3(64), 0, pl->stream, pl->slv.leaves.p, T.tleaf.p, T.dtile.p, T.xs.p, pl->kp,
                           T.a.p, as, T.t.p, ts, T.live.p, T.G.p);
    }
}

template <int DIM, int MODE>
static void launch_cv_gram(mra_plan* pl, long n, int nt_max) {
    mra_plan::Sites& T = pl->sit;
    hipLaunchKernelGGL((k_cv_gram<DIM, MODE>), dim3((unsigned)n, (unsigned)nt_max), dim3(64), 0, pl->stream, pl->slv.leaves.p, T.tleaf.p, T.dtile.p, T.xs.p, pl->kp,
                       T.a.p, T.b.p, (long)T.anc_max * 16, T.t.p, (long)T.nop_max * 16, T.sslot.p, mra_cv_rows(pl), T.G.p);
}
