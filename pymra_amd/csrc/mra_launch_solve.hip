// mra_launch_solve.hip - mra_solve: descriptors, work buffers and the launch sequence of one block of at most
// 16 right-hand sides over the factors a likelihood pass left in the plan.  A translation unit of its own: the kernels of the pass
// keep their object code.
#define MRA_KERNELS_TEMPLATES_ONLY
#include "mra_solve_kernels.h"

static const int SOLVE_QUAD_BLOCKS = 512;

NodeLayout mra_node_layout(mra_plan* pl, int leaf_blocks, bool with_F, DevVec<double>& nb, DevVec<SolveFront>& fronts, DevVec<const double*>& kids) {
    const int nn = pl->n_nodes;
    NodeLayout Y;
    Y.noff.assign(nn + 1, 0); Y.anc.assign(nn, 0);
    for (int i = 0; i < nn; ++i) {
        const int m = pl->node_level[i];
        Y.anc[i] = pl->Ka - pl->asuf[m];
        Y.noff[i + 1] = Y.noff[i] + (pl->leaf[i] ? (long)leaf_blocks * Y.anc[i] : (long)pl->cw[m] + Y.anc[i]) * 16;
    }
    nb.alloc((size_t)std::max<long>(Y.noff[nn], 1));
    std::vector<const double*> kv;
    Y.lev_off.assign(pl->n_levels + 1, 0);
    for (int m = 0; m < pl->n_levels; ++m) {
        const LevelData& lvl = pl->lev[m];
        Y.lev_off[m] = Y.fronts.size();
        for (size_t s = 0; s < lvl.nodes.size(); ++s) {
            const int i = lvl.nodes[s];
            const int p = pl->parent[i];
            SolveFront N{};
            N.F = with_F ? lvl.F_of(s) : nullptr;
            N.buf = nb.p + Y.noff[i];
            N.chain = p >= 0 ? nb.p + Y.noff[p] : nullptr;
            N.ld = with_F ? lvl.ldf : 0; N.cw = lvl.cw; N.anc = Y.anc[i];
            N.kid0 = (int)kv.size();
            for (int k = pl->child_ptr[i]; k < pl->child_ptr[i + 1]; ++k) {
                const int ch = pl->child_list[k];
                // a leaf hands up its first block (cw + anc rows), a front the ancestor part of its buffer
                kv.push_back(nb.p + Y.noff[ch] + (pl->leaf[ch] ? 0 : (long)pl->cw[pl->node_level[ch]] * 16));
            }
            N.nkid = (int)kv.size() - N.kid0;
            Y.fronts.push_back(N);
        }
    }
    Y.lev_off[pl->n_levels] = Y.fronts.size();
    if (kv.empty()) kv.push_back(nullptr);
    fronts.upload(Y.fronts.empty() ? std::vector<SolveFront>(1) : Y.fronts);
    kids.upload(kv);
    return Y;
}

void mra_solver_build(mra_plan* pl) {
    mra_plan::Solver& S = pl->slv;
    if (S.built) return;
    if (pl->knots_pending) throw MraError(MRA_ERR_STATE, "knot rows not set");
    const long P = pl->P;
    const size_t nl = pl->leaf_nodes.size();
    const int nn = pl->n_nodes;
    // the column layout the sweeps assume, checked here for every call on the retained factors
    for (int i = 0; i < nn; ++i) {
        const int m = pl->node_level[i], p = pl->parent[i], anc = pl->Ka - pl->asuf[m];
        if (!pl->leaf[i] && pl->lev[m].nf != pl->cw[m] + anc + MRA_YB) throw MraError(MRA_ERR_STATE, "mra_solve: front size does not match the column layout");
        if (p >= 0 && anc != pl->cw[pl->node_level[p]] + pl->Ka - pl->asuf[pl->node_level[p]]) throw MraError(MRA_ERR_STATE, "mra_solve: ancestor chain does not match the column layout");
        if (p < 0 && anc != 0) throw MraError(MRA_ERR_STATE, "mra_solve: the root has ancestor columns");
    }
    for (int m = 0; m < pl->n_levels; ++m)
        for (size_t s = 0; s < pl->lev[m].nodes.size(); ++s)
            if (pl->node_slot[pl->lev[m].nodes[s]] != (int)s) throw MraError(MRA_ERR_STATE, "mra_solve: node slot order");
    mra_row_maps(pl);
    // node buffers: a leaf's g / beta (anc x16), a front's [z ; g] / [alpha ; chain] ((cw + anc) x16)
    const NodeLayout lay = mra_node_layout(pl, 1, true, S.nb, S.fronts, S.kids);
    const std::vector<long>& noff = lay.noff;
    const std::vector<int>& anc = lay.anc;
    S.lev_off = lay.lev_off;
    const long n_uy = pl->obs_off_host.empty() ? 0 : pl->obs_off_host.back() * 16;
    S.uy.alloc((size_t)std::max<long>(n_uy, 1));
    S.yb.alloc((size_t)16 * P); S.out.alloc((size_t)16 * P);
    S.qpart.alloc((size_t)SOLVE_QUAD_BLOCKS * 256); S.quad.alloc(256);
    S.msave.alloc(P); S.vsave.alloc(P);
    S.work_bytes = sizeof(double) * ((size_t)noff[nn] + (size_t)n_uy + (size_t)34 * P + (size_t)SOLVE_QUAD_BLOCKS * 256 + 256);
    std::vector<SolveLeaf> lv(nl);
    std::vector<SolveSeg> segs;
    for (size_t t = 0; t < nl; ++t) {
        const int i = pl->leaf_nodes[t];
        const int m = pl->node_level[i], nop = pl->leaf_nop[t], p = pl->parent[i];
        SolveLeaf L{};
        L.Lc = leaf_C(pl, t); L.Ut = leaf_Ut(pl, t);
        L.obs = pl->obs_idx.p + pl->obs_off_host[t];
        L.uy = S.uy.p + pl->obs_off_host[t] * 16;
        L.gb = S.nb.p + noff[i];
        L.chain = p >= 0 ? S.nb.p + noff[p] : nullptr;
        L.row0 = pl->row0[i]; L.nrows = (int)(pl->row1[i] - pl->row0[i]);
        L.nop = nop; L.anc = anc[i]; L.a0 = pl->asuf[m];
        lv[t] = L;
        if (nop) segs.push_back(SolveSeg{L.uy, nop, 1});
    }
    for (const SolveFront& N : lay.fronts) segs.push_back(SolveSeg{N.buf, N.cw, -1});
    S.lev_lds.assign(pl->n_levels, 0);
    for (int m = 0; m < pl->n_levels; ++m) {
        const int cw = pl->lev[m].cw;
        S.lev_lds[m] = sizeof(double) * ((size_t)cw * 16 + (cw <= SOLVE_FRONT_STAGE ? (size_t)cw * cw : 0));
        if (S.lev_lds[m] > 64 * 1024) throw MraError(MRA_ERR_INVALID, "mra_solve: blocks wider than 512 columns are not supported");
    }
    if (segs.empty()) segs.push_back(SolveSeg{nullptr, 0, 1});
    if (nl) S.leaves.upload(lv);
    S.segs.upload(segs);
    // the archive of MRA_SOLVE_FULL_QUAD: a segment's first row in a block's panel; the panels go with the descriptors they mirror
    std::vector<long> soff(segs.size());
    S.arch_rows = 0;
    for (size_t k = 0; k < segs.size(); ++k) { soff[k] = S.arch_rows; S.arch_rows += segs[k].n; }
    S.seg_off.upload(soff);
    S.arch.release(); S.cpart.release(); S.qfull.release(); S.arch_blocks = 0;
    S.built = true;
}

void mra_solver_archive(mra_plan* pl, int n_blocks) {
    mra_plan::Solver& S = pl->slv;
    if (n_blocks <= S.arch_blocks) return;
    // (4 rows of slack: the masked tail of the last segment computes addresses past its rows, it does not read them)
    S.arch.alloc((size_t)n_blocks * (size_t)std::max<long>(S.arch_rows, 1) * 16 + 64);
    S.qfull.alloc((size_t)n_blocks * n_blocks * 256);
    if (!S.cpart.n) S.cpart.alloc((size_t)6 * SOLVE_QUAD_BLOCKS * 256);
    S.arch_blocks = n_blocks;
}

// The block pairs in groups of four panels: the blocks in twos, a group per pair of twos (I <= J) - its six pairs are the four between
// the twos and the one inside each, wanted the first time that two is seen.  64 columns: one group, six pairs, every row read once.
void mra_solver_quad_cross(mra_plan* pl, int n_blocks) {
    mra_plan::Solver& S = pl->slv;
    if (n_blocks < 2) return;
    const int nseg = (int)S.segs.n, nb = std::min(SOLVE_QUAD_BLOCKS, std::max(nseg, 1)), ldq = 16 * S.arch_blocks;
    const long panel = std::max<long>(S.arch_rows, 1) * 16;
    const int n2 = (n_blocks + 1) / 2;
    std::vector<char> seen((size_t)n2, 0);
    auto blk = [&](int two, int k) { const int b = 2 * two + k; return b < n_blocks ? b : -1; };
    auto group = [&](int I, int J) {      // J < 0: the one two of a call of two blocks
        QuadGroup G{};
        G.blk[0] = blk(I, 0); G.blk[1] = blk(I, 1); G.blk[2] = J < 0 ? -1 : blk(J, 0); G.blk[3] = J < 0 ? -1 : blk(J, 1);
        static const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
        for (int p = 0; p < 6; ++p) G.out[p] = G.blk[pa[p]] >= 0 && G.blk[pb[p]] >= 0;
        if (seen[(size_t)I]) G.out[0] = 0;
        if (J >= 0 && seen[(size_t)J]) G.out[5] = 0;
        seen[(size_t)I] = 1;
        if (J >= 0) seen[(size_t)J] = 1;
        hipLaunchKernelGGL(k_solve_quad_cross, dim3((unsigned)nb), dim3(256), 0, pl->stream, S.segs.p, S.seg_off.p, nseg, S.arch.p, panel, G, S.cpart.p);
        hipLaunchKernelGGL(k_solve_quad_cross_sum, dim3(6), dim3(256), 0, pl->stream, S.cpart.p, nb, G, S.qfull.p, ldq);
    };
    if (n2 == 1) { group(0, -1); return; }
    for (int I = 0; I < n2; ++I)
        for (int J = I + 1; J < n2; ++J) group(I, J);
}

void mra_trend_rows(mra_plan* pl) {
    mra_plan::Trend& T = pl->trend;
    hipLaunchKernelGGL(k_trend_rows, dim3((unsigned)((pl->P + 63) / 64)), dim3(64), 0, pl->stream, T.m.p, T.X.p, T.coef.p, T.coef.p + MRA_TREND_LD,
                       T.var_pass.p, pl->maps.rep.p, T.p, pl->P, T.mean.p, T.var.p);
}

template <int DIM>
static void launch_rows(mra_plan* pl) {
    mra_plan::Solver& S = pl->slv;
    const dim3 grid((unsigned)((pl->P / 16 + 3) / 4)), block(256);
#define MRA_SOLVE_ROWS(MD) hipLaunchKernelGGL((k_solve_rows<DIM, MD>), grid, block, 0, pl->stream, S.leaves.p, pl->maps.tile_leaf.p, pl->W.p, (long)pl->ldw, \
                                              pl->X.p, pl->maps.rep.p, pl->kp, S.out.p, pl->P)
    switch (pl->kp.mode) {
        case 0: MRA_SOLVE_ROWS(0); break;
        case 1: MRA_SOLVE_ROWS(1); break;
        case 2: MRA_SOLVE_ROWS(2); break;
        case 3: MRA_SOLVE_ROWS(3); break;
        case 4: if constexpr (DIM != 3) MRA_SOLVE_ROWS(4); else mra_nu3_solve_rows(pl); break;      // (3-D: the instance of mra_launch_nu3.hip)
        case 5: mra_sum_solve_rows(pl); break;      // (MRA_KERNEL_SUM, every dimension: the instances of mra_launch_sum2.hip)
        case 6: mra_loc_solve_rows(pl); break;      // (MRA_KERNEL_LOCAL, d = 2 and 3: the instances of mra_launch_loc2.hip)
        default: mra_bad_mode("mra_solve", pl->kp.mode);
    }
#undef MRA_SOLVE_ROWS
}

void mra_solver_block(mra_plan* pl, bool want_mean, bool want_quad, bool want_rows, int archive) {
    mra_plan::Solver& S = pl->slv;
    const unsigned nl = (unsigned)pl->leaf_nodes.size();
    if (pl->d < 1 || pl->d > 3) throw MraError(MRA_ERR_INVALID, "mra_solve: 1-, 2- or 3-D locations only");
    // 1. forward, leaves
    if (nl) {
        hipLaunchKernelGGL(k_solve_leaf_trsm<false>, dim3(nl), dim3(64), 0, pl->stream, S.leaves.p, S.yb.p, pl->P);
        hipLaunchKernelGGL(k_solve_leaf_g, dim3(nl), dim3(256), 0, pl->stream, S.leaves.p);
    }
    // 2. forward, fronts bottom-up
    for (int m = pl->n_levels - 1; m >= 0; --m) {
        const unsigned n = (unsigned)(S.lev_off[m + 1] - S.lev_off[m]);
        if (n) hipLaunchKernelGGL(k_solve_front_fwd, dim3(n), dim3(256), S.lev_lds[m], pl->stream, S.fronts.p + S.lev_off[m], S.kids.p);
    }
    // 3. quadratic form (the z of the fronts are overwritten by the backward sweep); the same vectors into the block's panel
    if (archive >= 0) {
        const int nseg = (int)S.segs.n;
        hipLaunchKernelGGL(k_solve_archive, dim3((unsigned)std::min(std::max(nseg, 1), 65535)), dim3(256), 0, pl->stream, S.segs.p, S.seg_off.p, nseg,
                           S.arch.p + (size_t)archive * (size_t)std::max<long>(S.arch_rows, 1) * 16);
    }
    if (want_quad) {
        const int nseg = (int)S.segs.n;
        const int nb = std::min(SOLVE_QUAD_BLOCKS, std::max(nseg, 1));
        hipLaunchKernelGGL(k_solve_quad_part, dim3((unsigned)nb), dim3(256), 0, pl->stream, S.segs.p, nseg, S.qpart.p);
        hipLaunchKernelGGL(k_solve_quad_sum, dim3(1), dim3(256), 0, pl->stream, S.qpart.p, nb, S.quad.p);
    }
    if (!want_mean) return;
    // 4. backward, fronts top-down
    for (int m = 0; m < pl->n_levels; ++m) {
        const unsigned n = (unsigned)(S.lev_off[m + 1] - S.lev_off[m]);
        if (n) hipLaunchKernelGGL(k_solve_front_bwd, dim3(n), dim3(256), S.lev_lds[m], pl->stream, S.fronts.p + S.lev_off[m]);
    }
    // 5. backward, leaves; 6. rows
    if (nl) {
        hipLaunchKernelGGL(k_solve_leaf_sbeta, dim3(nl), dim3(256), 0, pl->stream, S.leaves.p);
        hipLaunchKernelGGL(k_solve_leaf_trsm<true>, dim3(nl), dim3(64), 0, pl->stream, S.leaves.p, S.yb.p, pl->P);
    }
    if (!want_rows) return;          // mra_predict_sites: beta and q are read from the leaves' gb / uy
    if (pl->d == 1) launch_rows<1>(pl); else if (pl->d == 2) launch_rows<2>(pl); else launch_rows<3>(pl);
}

void mra_solver_pseudo(mra_plan* pl, const double* y, const double* x, const SampleZ& zs, long slot0) {
    if (pl->noise_on) {
        hipLaunchKernelGGL(k_solve_pseudo_rows, dim3((unsigned)((pl->P + 255) / 256)), dim3(256), 0, pl->stream, y, x, zs, slot0, pl->noise_sd.p,
                           pl->slv.yb.p, pl->P);
        return;
    }
    hipLaunchKernelGGL(k_solve_pseudo, dim3((unsigned)((pl->P + 255) / 256)), dim3(256), 0, pl->stream, y, x, zs, slot0, std::sqrt(pl->R),
                       pl->slv.yb.p, pl->P);
}
void mra_solver_addmean(mra_plan* pl, double* x, int ns) {
    const long n = (long)ns * pl->P;
    hipLaunchKernelGGL(k_solve_addmean, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, pl->stream, x, pl->slv.out.p, n);
}
