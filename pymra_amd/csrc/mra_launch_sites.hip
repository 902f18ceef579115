// mra_launch_sites.hip - mra_predict_sites: descriptors, work buffers and the launches of one chunk of site tiles
// over the state a likelihood pass left in the plan, and the Gram launch of mra_sites_cov (section 13) over the same buffers.  A
// translation unit of its own: the kernels of the pass keep their object code.  The inert, leaf Gram, zeta and draw launches of
// mra_sample_sites (section 14) run over the same buffers, a batch of whole leaves at a time; so do the launches of mra_cv (section 18) and mra_cv_trend (section 22).
#define MRA_KERNELS_TEMPLATES_ONLY
#include "mra_site_kernels.h"

void mra_sites_build(mra_plan* pl) {
    mra_plan::Sites& T = pl->sit;
    if (T.built) return;
    mra_solver_build(pl);                       // the leaves' descriptors, and the checks of the column layout
    const size_t nl = pl->leaf_nodes.size();
    std::vector<SiteNode> nv((size_t)pl->n_nodes);
    for (int m = 0; m < pl->n_levels; ++m) {
        const LevelData& lvl = pl->lev[m];
        for (size_t s = 0; s < lvl.nodes.size(); ++s) {
            const int i = lvl.nodes[s];
            SiteNode N{};
            N.Lp = lvl.Lp_of(s); N.F = lvl.F_of(s);
            N.knots = pl->knot_idx.p + pl->knot_idx_off[i];
            N.ld = lvl.ldf; N.cw = lvl.cw; N.c0 = pl->coff[m]; N.anc = pl->Ka - pl->asuf[m];
            nv[i] = N;
        }
    }
    std::vector<int> chain, chain_ptr(nl + 1, 0);
    T.anc_max = 0; T.nop_max = 0;
    for (size_t t = 0; t < nl; ++t) {
        const int i = pl->leaf_nodes[t];
        const std::vector<int> up = leaf_ancestors(pl, i);      // root first, zero-width levels included
        int width = 0;
        for (int p : up) width += pl->cw[pl->node_level[p]];
        const int anc = pl->Ka - pl->asuf[pl->node_level[i]];
        if (width != anc) throw MraError(MRA_ERR_STATE, "mra_predict_sites: a leaf's ancestor blocks do not fill its ancestor columns");
        chain.insert(chain.end(), up.begin(), up.end());
        chain_ptr[t + 1] = (int)chain.size();
        T.anc_max = std::max(T.anc_max, anc);
        T.nop_max = std::max(T.nop_max, pl->leaf_nop[t]);
    }
    if (chain.empty()) chain.push_back(0);
    T.nodes.upload(nv); T.chain.upload(chain); T.chain_ptr.upload(chain_ptr);
    T.cap_tiles = 0;                            // the strides of the work buffers follow anc_max / nop_max
    T.built = true;
}

// a and b (anc_max x16 each), t (nop_max x16), the sites, the leaf slot, 16 variances and a 16 x 16 block of means
size_t mra_sites_tile_bytes(const mra_plan* pl) {
    const mra_plan::Sites& T = pl->sit;
    return sizeof(double) * 16 * ((size_t)2 * T.anc_max + T.nop_max + pl->d + 1 + 16) + sizeof(int);
}

void mra_sites_reserve(mra_plan* pl, long n) {
    mra_plan::Sites& T = pl->sit;
    if (n <= T.cap_tiles) return;
    T.cap_tiles = 0;
    T.tleaf.alloc((size_t)n);
    T.xs.alloc((size_t)n * 16 * pl->d);
    T.a.alloc(std::max<size_t>((size_t)n * T.anc_max * 16, 1)); T.b.alloc(std::max<size_t>((size_t)n * T.anc_max * 16, 1));
    T.t.alloc(std::max<size_t>((size_t)n * T.nop_max * 16, 1));
    T.var.alloc((size_t)n * 16); T.mean.alloc((size_t)n * 256);
    T.cap_tiles = n;
}

void mra_sites_timed(mra_plan* pl, int which, const std::function<void()>& work) {
    if (!pl->ktiming) { work(); return; }
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); throw MraError(MRA_ERR_HIP, "hipEventCreate failed"); }
    struct Pair { hipEvent_t a, b; ~Pair() { hipEventDestroy(a); hipEventDestroy(b); } } pair{e0, e1};
    HIP_TRY(hipEventRecord(e0, pl->stream));
    work();
    HIP_TRY(hipEventRecord(e1, pl->stream));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (pl->sit.ms_sink ? pl->sit.ms_sink : pl->sit.ms)[which] += ms;
}
static void timed(mra_plan* pl, int which, const std::function<void()>& work) { mra_sites_timed(pl, which, work); }

#include "mra_launch_sites.inc"      // launch_basis, launch_leaf, launch_mean, launch_gram, launch_leaf_gram, launch_cv_gram <DIM, MODE>

// the <DIM, MODE> instance of the plan's dimension and kernel, as the solver's row kernel is chosen (<3, 4>: FN_nu3 of mra_launch_nu3.hip; mode 5 in every dimension: FN_sum of mra_launch_sum2.hip; mode 6, d = 2 and 3: FN_loc of mra_launch_loc2.hip)
#define MRA_SITES_DISPATCH(FN, ...)                                                                                  \
    do {                                                                                                             \
        if (pl->d < 1 || pl->d > 3) throw MraError(MRA_ERR_INVALID, "mra_predict_sites: 1-, 2- or 3-D locations only"); \
        if (pl->kp.mode < 0 || pl->kp.mode > 6) mra_bad_mode("mra_predict_sites", pl->kp.mode);                                                   \
        if (pl->kp.mode == 5) { FN##_sum(__VA_ARGS__); break; }                                                      \
        if (pl->kp.mode == 6) { FN##_loc(__VA_ARGS__); break; }                                                      \
        switch ((pl->d - 1) * 5 + pl->kp.mode) {                                                                     \
            case 0: FN<1, 0>(__VA_ARGS__); break; case 1: FN<1, 1>(__VA_ARGS__); break; case 2: FN<1, 2>(__VA_ARGS__); break; case 3: FN<1, 3>(__VA_ARGS__); break; case 4: FN<1, 4>(__VA_ARGS__); break;\
            case 5: FN<2, 0>(__VA_ARGS__); break; case 6: FN<2, 1>(__VA_ARGS__); break; case 7: FN<2, 2>(__VA_ARGS__); break; case 8: FN<2, 3>(__VA_ARGS__); break; case 9: FN<2, 4>(__VA_ARGS__); break;\
            case 10: FN<3, 0>(__VA_ARGS__); break; case 11: FN<3, 1>(__VA_ARGS__); break; case 12: FN<3, 2>(__VA_ARGS__); break; case 13: FN<3, 3>(__VA_ARGS__); break; case 14: FN##_nu3(__VA_ARGS__); break;\
        }                                                                                                            \
    } while (0)

static void check_chunk(const mra_plan* pl, long n) {
    if (n <= 0 || n > pl->sit.cap_tiles) throw MraError(MRA_ERR_STATE, "mra_predict_sites: chunk larger than its work buffers");
}

void mra_sites_basis(mra_plan* pl, long n) {
    check_chunk(pl, n);
    timed(pl, 0, [&] { MRA_SITES_DISPATCH(launch_basis, pl, n); });
}

void mra_sites_var(mra_plan* pl, long n) {
    check_chunk(pl, n);
    mra_plan::Sites& T = pl->sit;
    timed(pl, 1, [&] { MRA_SITES_DISPATCH(launch_leaf, pl, n); });
    timed(pl, 2, [&] {
        hipLaunchKernelGGL(k_site_chain, dim3((unsigned)n), dim3(64), 0, pl->stream, pl->slv.leaves.p, T.nodes.p, T.chain_ptr.p, T.chain.p, T.tleaf.p,
                           T.b.p, (long)T.anc_max * 16, T.var.p);
    });
}

void mra_sites_mean(mra_plan* pl, long n, int nc, int which) {
    check_chunk(pl, n);
    if (nc < 1 || nc > 16) throw MraError(MRA_ERR_STATE, "mra_predict_sites: a column block has 1 to 16 columns");
    timed(pl, which, [&] { MRA_SITES_DISPATCH(launch_mean, pl, n, nc); });
}

void mra_sites_gram(mra_plan* pl, long n, long tile0, long rows, bool posterior) {
    check_chunk(pl, n);
    if (tile0 < 0 || rows < 1 || rows > 65535 || tile0 + rows > n || (size_t)rows * 16 * (size_t)n * 16 > pl->sit.gram.n)
        throw MraError(MRA_ERR_STATE, "mra_sites_cov: row panel outside its tiles or larger than its buffer");
    timed(pl, 3, [&] { MRA_SITES_DISPATCH(launch_gram, pl, n, tile0, rows, posterior); });
}

// ---- mra_sample_sites ------------------------------------------------------------------------------------------
void mra_sites_draw_reserve(mra_plan* pl, long n, size_t g_doubles, long n_leaves) {
    mra_plan::Sites& T = pl->sit;
    mra_sites_reserve(pl, n);
    if (T.dtile.n < (size_t)n) T.dtile.alloc((size_t)n);
    if (T.sslot.n < (size_t)n * 16) { T.sslot.alloc((size_t)n * 16); T.live.alloc((size_t)n * 16); }
    if (T.zl.n < (size_t)n * 256) { T.zl.alloc((size_t)n * 256); T.dout.alloc((size_t)n * 256); }
    if (T.G.n < g_doubles) T.G.alloc(g_doubles);
    if (T.invd.n < (size_t)n * 256) T.invd.alloc((size_t)n * 256);
    if (T.dprob.n < (size_t)n_leaves) { T.dprob.alloc((size_t)n_leaves); T.dn.alloc((size_t)n_leaves); }
    if (!T.derr.n) T.derr.alloc(1);
}

static void check_batch(const mra_plan* pl, long n) {
    const mra_plan::Sites& T = pl->sit;
    if (n <= 0 || n > T.cap_tiles || (size_t)n > T.dtile.n || (size_t)n * 16 > T.sslot.n || (size_t)n * 256 > T.zl.n)
        throw MraError(MRA_ERR_STATE, "mra_sample_sites: batch larger than its work buffers");
}

void mra_sites_leaf_gram(mra_plan* pl, long n, int nt_max, bool posterior) {
    check_batch(pl, n);
    if (nt_max < 1 || nt_max > 65535) throw MraError(MRA_ERR_STATE, "mra_sample_sites: a leaf of the batch has no tile or too many");
    timed(pl, 3, [&] { MRA_SITES_DISPATCH(launch_leaf_gram, pl, n, nt_max, posterior); });
}

void mra_sites_zeta(mra_plan* pl, long n, const SampleZ& zs, long n_coarse, bool from_caller) {
    check_batch(pl, n);
    mra_plan::Sites& T = pl->sit;
    if (from_caller && T.zin.n < (size_t)n * 256) throw MraError(MRA_ERR_STATE, "mra_sample_sites: the caller's leaf draws are not staged");
    timed(pl, 5, [&] {
        hipLaunchKernelGGL(k_site_zeta, dim3((unsigned)((n * 256 + 255) / 256)), dim3(256), 0, pl->stream, zs, n_coarse, T.sslot.p, T.live.p,
                           from_caller ? T.zin.p : nullptr, n * 16, T.zl.p);
    });
}

void mra_sites_draw(mra_plan* pl, long n, bool posterior) {
    check_batch(pl, n);
    mra_plan::Sites& T = pl->sit;
    timed(pl, 5, [&] {
        hipLaunchKernelGGL(k_site_draw, dim3((unsigned)n), dim3(64), 0, pl->stream, T.tleaf.p, T.dtile.p, T.dchain_ptr.p, T.dchain.p, posterior ? T.b.p : T.a.p,
                           (long)T.anc_max * 16, T.zc.p, T.G.p, T.zl.p, posterior ? T.mean.p : nullptr, T.dout.p, n * 16);
    });
}

// ---- mra_cv --------------------------------------------------------------------------------------------------------
// timing entries of a call (sit.cv_ms through the sink): 0 .. 2 the site kernels, 3 mean and sweeps, 4 Gram, 5 Cholesky, 6 solve and
// reduction, 7 uploads, 8 downloads
void mra_cv_reserve(mra_plan* pl, long n, size_t g_doubles, long n_leaves) {
    mra_plan::Sites& T = pl->sit;
    mra_sites_draw_reserve(pl, n, g_doubles, n_leaves);
    if (T.cvx.n < g_doubles) T.cvx.alloc(g_doubles);
    if (T.cvgroup.n < (size_t)n_leaves) T.cvgroup.alloc((size_t)n_leaves);
    const size_t P = (size_t)pl->P, nn = (size_t)pl->n_nodes, nl = pl->leaf_nodes.size();
    if (T.cvrow.n != 5 * P) T.cvrow.alloc(5 * P);
    if (T.cvgl.n != nn) T.cvgl.alloc(nn);
    if (!T.cvpart.n) { T.cvpart.alloc((size_t)CV_BLOCKS * MRA_CV_NRES); T.cvres.alloc(MRA_CV_NRES); }
    if (T.cvleaf.n != nl) {
        std::vector<long> rows(2 * nl);
        for (size_t t = 0; t < nl; ++t) { rows[2 * t] = pl->row0[pl->leaf_nodes[t]]; rows[2 * t + 1] = pl->row1[pl->leaf_nodes[t]]; }
        T.cvleaf.upload(pl->leaf_nodes); T.cvleaf_row.upload(rows);
    }
    // all-ones bytes are a NaN: rows and nodes that nothing writes stay NaN
    HIP_TRY(hipMemsetAsync(T.cvrow.p, 0xFF, 5 * P * sizeof(double), pl->stream));
    HIP_TRY(hipMemsetAsync(T.cvgl.p, 0xFF, nn * sizeof(double), pl->stream));
}

CvRows mra_cv_rows(const mra_plan* pl) { return CvRows{pl->y.p, pl->noise_on ? pl->noise.p : nullptr, pl->R}; }
CvOut mra_cv_out(const mra_plan* pl) {
    double* b = pl->sit.cvrow.p;
    const long P = pl->P;
    return CvOut{b, b + P, b + 2 * P, b + 3 * P, b + 4 * P};
}

static void check_cv_batch(const mra_plan* pl, long n) {
    const mra_plan::Sites& T = pl->sit;
    if (n <= 0 || n > T.cap_tiles || (size_t)n > T.dtile.n || (size_t)n * 16 > T.sslot.n || (size_t)n * 256 > T.zl.n || T.cvrow.n != 5 * (size_t)pl->P)
        throw MraError(MRA_ERR_STATE, "mra_cv: batch larger than its work buffers");
}

void mra_cv_sites(mra_plan* pl, long n) {
    check_cv_batch(pl, n);
    mra_plan::Sites& T = pl->sit;
    timed(pl, 7, [&] { hipLaunchKernelGGL(k_cv_sites, dim3((unsigned)((n * 16 + 255) / 256)), dim3(256), 0, pl->stream, T.sslot.p, pl->X.p, pl->d, n * 16, T.xs.p); });
}

void mra_cv_loo(mra_plan* pl, long n) {
    check_cv_batch(pl, n);
    mra_plan::Sites& T = pl->sit;
    timed(pl, 6, [&] {
        hipLaunchKernelGGL(k_cv_loo, dim3((unsigned)((n * 16 + 255) / 256)), dim3(256), 0, pl->stream, T.sslot.p, n * 16, T.var.p, T.mean.p, mra_cv_rows(pl),
                           mra_cv_out(pl), T.derr.p);
    });
}

void mra_cv_gram(mra_plan* pl, long n, int nt_max) {
    check_cv_batch(pl, n);
    if (nt_max < 1 || nt_max > 65535) throw MraError(MRA_ERR_STATE, "mra_cv: a leaf of the batch has no tile or too many");
    timed(pl, 4, [&] { MRA_SITES_DISPATCH(launch_cv_gram, pl, n, nt_max); });
}

void mra_cv_solve(mra_plan* pl, long n, long n_groups) {
    check_cv_batch(pl, n);
    mra_plan::Sites& T = pl->sit;
    if (n_groups < 1 || (size_t)n_groups > T.cvgroup.n || (size_t)n_groups > T.dn.n) throw MraError(MRA_ERR_STATE, "mra_cv: more groups than the batch holds");
    timed(pl, 6, [&] {
        hipLaunchKernelGGL(k_cv_fwd, dim3((unsigned)n_groups), dim3(64), 0, pl->stream, T.cvgroup.p, T.sslot.p, T.mean.p, mra_cv_rows(pl), T.G.p, T.dn.p, T.zl.p,
                           T.cvgl.p);
        hipLaunchKernelGGL(k_cv_solve, dim3((unsigned)n), dim3(64), 0, pl->stream, T.dtile.p, T.sslot.p, T.var.p, T.mean.p, mra_cv_rows(pl), T.G.p, T.zl.p,
                           T.cvx.p, mra_cv_out(pl));
    });
}

void mra_cv_reduce(mra_plan* pl, bool by_leaf) {
    mra_plan::Sites& T = pl->sit;
    if (T.cvrow.n != 5 * (size_t)pl->P || !T.cvpart.n) throw MraError(MRA_ERR_STATE, "mra_cv: the row results are not allocated");
    const int nl = (int)pl->leaf_nodes.size();
    timed(pl, 6, [&] {
        if (!by_leaf && nl)
            hipLaunchKernelGGL(k_cv_leaf_sum, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, pl->stream, T.cvleaf.p, T.cvleaf_row.p, nl, mra_cv_out(pl).lpd, T.cvgl.p);
        hipLaunchKernelGGL(k_cv_part, dim3(CV_BLOCKS), dim3(256), 0, pl->stream, mra_cv_rows(pl), mra_cv_out(pl), (long)pl->P, T.cvgl.p, pl->n_nodes, T.cvpart.p);
        hipLaunchKernelGGL(k_cv_sum, dim3(1), dim3(64 * MRA_CV_NRES), 0, pl->stream, T.cvpart.p, CV_BLOCKS, T.cvres.p);
    });
}

// ---- mra_cv_trend --------------------------------------------------------------------------------------------------
// timing entries of a call (sit.cvt_ms through the sink): mra_cv's nine, then 9 the trend's sweeps, 10 k_cv_trend, 11 k_cv_downdate
static int cv_trend_qn(const mra_plan* pl) { return (pl->trend.p + 3) & ~3; }

size_t mra_cv_trend_tile_bytes(const mra_plan* pl) { return (size_t)cv_trend_qn(pl) * 16 * sizeof(double); }

void mra_cv_trend_reserve(mra_plan* pl, long n) {
    mra_plan::Sites& T = pl->sit;
    const size_t P = (size_t)pl->P, need = (size_t)n * cv_trend_qn(pl) * 16;
    if (T.cvw.n < need) T.cvw.alloc(need);
    if (T.cvwsq.n != P) T.cvwsq.alloc(P);
    if (!T.cvtpart.n) { T.cvtpart.alloc((size_t)CV_BLOCKS * MRA_CVT_NRES); T.cvtres.alloc(MRA_CVT_NRES); }
    HIP_TRY(hipMemsetAsync(T.cvwsq.p, 0, P * sizeof(double), pl->stream));
}

static void check_cv_trend_batch(const mra_plan* pl, long n) {
    const mra_plan::Sites& T = pl->sit;
    const mra_plan::Trend& R = pl->trend;
    check_cv_batch(pl, n);
    if (R.p < 1 || R.p > MRA_TREND_MAX || R.X.n != (size_t)R.p * pl->P || R.m.n != (size_t)(R.p + 1) * pl->P || !R.coef.n ||
        (size_t)n * cv_trend_qn(pl) * 16 > T.cvw.n || T.cvwsq.n != (size_t)pl->P)
        throw MraError(MRA_ERR_STATE, "mra_cv_trend: the trend's means or the batch's W are not allocated");
}

void mra_cv_trend_rows(mra_plan* pl, long n, bool add_v) {
    check_cv_trend_batch(pl, n);
    mra_plan::Sites& T = pl->sit;
    const mra_plan::Trend& R = pl->trend;
    timed(pl, 10, [&] {
        hipLaunchKernelGGL(k_cv_trend, dim3((unsigned)n), dim3(64), 0, pl->stream, T.sslot.p, R.X.p, R.m.p + pl->P, (long)pl->P, R.p, R.coef.p,
                           R.coef.p + MRA_TREND_MAX + 1, add_v ? 1 : 0, T.mean.p, T.var.p, T.cvw.p, T.cvwsq.p);
    });
}

void mra_cv_trend_downdate(mra_plan* pl, long n, int nt_max) {
    check_cv_trend_batch(pl, n);
    if (nt_max < 1 || nt_max > 65535) throw MraError(MRA_ERR_STATE, "mra_cv_trend: a leaf of the batch has no tile or too many");
    mra_plan::Sites& T = pl->sit;
    timed(pl, 11, [&] {
        hipLaunchKernelGGL(k_cv_downdate, dim3((unsigned)n, (unsigned)nt_max), dim3(64), 0, pl->stream, T.dtile.p, T.cvw.p, cv_trend_qn(pl), T.G.p);
    });
}

void mra_cv_trend_reduce(mra_plan* pl, bool h_has_w) {
    mra_plan::Sites& T = pl->sit;
    if (T.cvrow.n != 5 * (size_t)pl->P || T.cvwsq.n != (size_t)pl->P || !T.cvtpart.n) throw MraError(MRA_ERR_STATE, "mra_cv_trend: the row results are not allocated");
    timed(pl, 6, [&] {
        hipLaunchKernelGGL(k_cv_trend_part, dim3(CV_BLOCKS), dim3(256), 0, pl->stream, mra_cv_rows(pl), mra_cv_out(pl), T.cvwsq.p, h_has_w ? 1 : 0, (long)pl->P,
                           T.cvtpart.p);
        hipLaunchKernelGGL(k_cv_trend_sum, dim3(1), dim3(64 * MRA_CVT_NRES), 0, pl->stream, T.cvtpart.p, CV_BLOCKS, T.cvtres.p);
    });
}
