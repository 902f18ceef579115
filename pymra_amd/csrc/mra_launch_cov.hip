// mra_launch_cov.hip - mra_cov_apply: descriptors, work buffers and the launch sequence of one block of at most
// 16 vectors through the MRA prior (or posterior) covariance.  A translation unit of its own: the kernels of the pass and of
// mra_solve keep their object code.
#define MRA_KERNELS_TEMPLATES_ONLY
#include "mra_cov_kernels.h"

// After mra_solver_build: the cov path launches its fronts by the solver's level offsets.  It owns its node buffers: the posterior's
// sweeps (mra_solver_block) write slv.nb.
void mra_cov_build(mra_plan* pl) {
    mra_plan::Cov& V = pl->cov;
    if (V.built) return;
    if (!pl->slv.built) throw MraError(MRA_ERR_STATE, "mra_cov_apply: the solver's descriptors come first");
    const long P = pl->P;
    const size_t nl = pl->leaf_nodes.size();
    // node buffers: a leaf's t and t' (anc x16 each), a front's [tau ; tau_chain] ((cw + anc) x16); the column layout was checked
    // by mra_solver_build
    const NodeLayout lay = mra_node_layout(pl, 2, false, V.nb, V.fronts, V.kids);
    const std::vector<long>& noff = lay.noff;
    const std::vector<int>& anc = lay.anc;
    V.ab.alloc((size_t)16 * P); V.out.alloc((size_t)16 * P);
    V.gpart.alloc((size_t)COV_GRAM_BLOCKS * 256); V.gram.alloc(256);
    V.work_bytes = sizeof(double) * ((size_t)noff[pl->n_nodes] + (size_t)32 * P + (size_t)COV_GRAM_BLOCKS * 256 + 256);
    std::vector<CovLeaf> lv(nl);
    for (size_t t = 0; t < nl; ++t) {
        const int i = pl->leaf_nodes[t];
        const int p = pl->parent[i];
        if (pl->row0[i] < 0 || pl->row1[i] > P || (pl->row0[i] & 15) || (pl->row1[i] & 15) || (anc[i] & 15))
            throw MraError(MRA_ERR_STATE, "mra_cov_apply: a leaf's rows or ancestor columns are not whole 16-tiles");
        CovLeaf L{};
        L.t = V.nb.p + noff[i];
        L.tp = L.t + (long)anc[i] * 16;
        L.chain = p >= 0 ? V.nb.p + noff[p] : nullptr;
        L.row0 = pl->row0[i]; L.nrows = (int)(pl->row1[i] - pl->row0[i]);
        L.anc = anc[i]; L.a0 = pl->asuf[pl->node_level[i]];
        if (L.a0 + L.anc > pl->ldw) throw MraError(MRA_ERR_STATE, "mra_cov_apply: ancestor columns past the row stride of W");
        lv[t] = L;
    }
    if (nl) V.leaves.upload(lv);
    V.built = true;
}

template <int DIM>
static void launch_cov_rows(mra_plan* pl) {
    mra_plan::Cov& V = pl->cov;
    const dim3 grid((unsigned)((pl->P / 16 + 3) / 4)), block(256);
#define MRA_COV_ROWS(MD) hipLaunchKernelGGL((k_cov_rows<DIM, MD>), grid, block, 0, pl->stream, V.leaves.p, pl->maps.tile_leaf.p, pl->W.p, (long)pl->ldw, \
                                            pl->X.p, pl->maps.rep.p, pl->maps.knot.p, pl->kp, V.ab.p, V.out.p, pl->P)
    switch (pl->kp.mode) {
        case 0: MRA_COV_ROWS(0); break;
        case 1: MRA_COV_ROWS(1); break;
        case 2: MRA_COV_ROWS(2); break;
        case 3: MRA_COV_ROWS(3); break;
        case 4: if constexpr (DIM != 3) MRA_COV_ROWS(4); else mra_nu3_cov_rows(pl); break;      // (3-D: the instance of mra_launch_nu3.hip)
        case 5: mra_sum_cov_rows(pl); break;        // (MRA_KERNEL_SUM, every dimension: the instances of mra_launch_sum2.hip)
        case 6: mra_loc_cov_rows(pl); break;        // (MRA_KERNEL_LOCAL, d = 2 and 3: the instances of mra_launch_loc2.hip)
        default: mra_bad_mode("mra_cov_apply", pl->kp.mode);
    }
#undef MRA_COV_ROWS
}

void mra_cov_block(mra_plan* pl, bool posterior, bool want_gram) {
    mra_plan::Cov& V = pl->cov;
    mra_plan::Solver& S = pl->slv;
    const long P = pl->P;
    const unsigned nl = (unsigned)pl->leaf_nodes.size();
    if (pl->d < 1 || pl->d > 3) throw MraError(MRA_ERR_INVALID, "mra_cov_apply: 1-, 2- or 3-D locations only");
    // 1. leaves; 2. fronts bottom-up; 3. fronts top-down (a single-leaf tree has no ancestors: none of the three reads anything)
    if (nl)
        hipLaunchKernelGGL(k_cov_leaf_proj, dim3(nl), dim3(256), 0, pl->stream, V.leaves.p, pl->W.p, (long)pl->ldw, V.ab.p, pl->maps.rep.p, pl->maps.knot.p, P);
    for (int m = pl->n_levels - 1; m >= 0; --m) {
        const unsigned n = (unsigned)(S.lev_off[m + 1] - S.lev_off[m]);
        if (n) hipLaunchKernelGGL(k_cov_up, dim3(n), dim3(256), 0, pl->stream, V.fronts.p + S.lev_off[m], V.kids.p);
    }
    for (int m = 1; m < pl->n_levels; ++m) {
        const unsigned n = (unsigned)(S.lev_off[m + 1] - S.lev_off[m]);
        if (n) hipLaunchKernelGGL(k_cov_down, dim3(n), dim3(256), 0, pl->stream, V.fronts.p + S.lev_off[m]);
    }
    // 4. rows
    if (pl->d == 1) launch_cov_rows<1>(pl); else if (pl->d == 2) launch_cov_rows<2>(pl); else launch_cov_rows<3>(pl);
    // 5. posterior: out -= mean_MRA(out at the observed rows)
    if (posterior) {
        const long n = 16 * P;
        hipLaunchKernelGGL(k_cov_to_rhs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, pl->stream, V.out.p, S.yb.p, n);
        mra_solver_block(pl, true, false);
        hipLaunchKernelGGL(k_cov_sub, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, pl->stream, V.out.p, S.out.p, pl->maps.rep.p, P);
    }
    // 6. gram
    if (want_gram) {
        const long ntile = P / 16, nt = (ntile + COV_GRAM_BLOCKS - 1) / COV_GRAM_BLOCKS;
        hipLaunchKernelGGL(k_cov_gram_part, dim3(COV_GRAM_BLOCKS), dim3(256), 0, pl->stream, V.ab.p, V.out.p, pl->maps.rep.p, P, nt, V.gpart.p);
        hipLaunchKernelGGL(k_cov_gram_sum, dim3(1), dim3(256), 0, pl->stream, V.gpart.p, COV_GRAM_BLOCKS, V.gram.p);
    }
}
