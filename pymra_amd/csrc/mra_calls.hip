// mra_calls.hip - the host drivers of the calls on the retained factors: mra_solve, mra_plan_set_trend / mra_trend_fit, mra_cov_apply,
// mra_predict_sites, mra_sites_cov, mra_sample_sites, mra_cv / mra_cv_trend and the two Laplace fits.  Host code only: every kernel
// is reached through the launchers of the other units, so an edit here recompiles no kernel.
#define MRA_KERNELS_TEMPLATES_ONLY
#include "mra_plan_types.h"
#include <atomic>

// ---- what the calls on the retained factors share ------------------------------------------------------------
// The plan's row maps: rep = a leaf's row that is a knot of some node, knot = a knot of its own leaf, tile_leaf = the leaf of a row tile.
const mra_plan::RowMaps& mra_row_maps(mra_plan* pl) {
    mra_plan::RowMaps& R = pl->maps;
    if (R.built) return R;
    const long P = pl->P;
    std::vector<unsigned char> is_knot(P, 0);
    R.knot_host.assign(P, 0); R.rep_host.assign(P, 0);
    for (int i = 0; i < pl->n_nodes; ++i)
        for (long k = pl->knot_ptr[i]; k < pl->knot_ptr[i + 1]; ++k) {
            const long row = pl->knot_rows[k];
            if (row < 0 || row >= P) throw MraError(MRA_ERR_INVALID, "knot row out of range");
            is_knot[row] = 1;
            if (pl->leaf[i]) R.knot_host[row] = 1;
        }
    std::vector<int> tile_leaf((size_t)(P / 16), -1);
    for (size_t t = 0; t < pl->leaf_nodes.size(); ++t) {
        const int i = pl->leaf_nodes[t];
        for (long r = pl->row0[i]; r < pl->row1[i]; ++r) R.rep_host[r] = is_knot[r];
        for (long tl = pl->row0[i] / 16; tl < pl->row1[i] / 16; ++tl) tile_leaf[tl] = (int)t;
    }
    R.rep.upload(R.rep_host); R.knot.upload(R.knot_host); R.tile_leaf.upload(tile_leaf);
    R.built = true;
    return R;
}

// latent slots of the non-leaf nodes: node order, cw[level] each.  zoff (may be nullptr): per node its first slot (-1: leaf)
long mra_coarse_slots(const mra_plan* pl, std::vector<long>* zoff) {
    long kn = 0;
    if (zoff) zoff->assign((size_t)pl->n_nodes, -1);
    for (int i = 0; i < pl->n_nodes; ++i)
        if (!pl->leaf[i]) { if (zoff) (*zoff)[(size_t)i] = kn; kn += pl->cw[pl->node_level[i]]; }
    return kn;
}

// What the caller reads back after a call that runs passes of its own (mra_sample, mra_solve): the last mra_run's likelihood, mean and
// var - and the device y when ysave is given - are saved on pl->stream and put back when the scope ends, on success and error paths alike.
KeepResults::KeepResults(mra_plan* p, double* ys, double* ms, double* vs)
    : pl(p), ysave(ys), msave(ms), vsave(vs), had_ran(p->ran), had_flags(p->run_flags), had_d(p->res_d), had_u(p->res_u),
      had_pred(p->ran && (p->run_flags & MRA_RUN_PREDICT)), bytes(p->P * sizeof(double)) {
    if (ysave) HIP_TRY(hipMemcpyAsync(ysave, pl->y.p, bytes, hipMemcpyDeviceToDevice, pl->stream));
    if (had_pred) HIP_TRY(hipMemcpyAsync(msave, pl->mean.p, bytes, hipMemcpyDeviceToDevice, pl->stream));
    if (had_pred) HIP_TRY(hipMemcpyAsync(vsave, pl->var.p, bytes, hipMemcpyDeviceToDevice, pl->stream));
}
KeepResults::~KeepResults() {
    if (ysave) hipMemcpyAsync(pl->y.p, ysave, bytes, hipMemcpyDeviceToDevice, pl->stream);
    if (had_pred) hipMemcpyAsync(pl->mean.p, msave, bytes, hipMemcpyDeviceToDevice, pl->stream);
    if (had_pred) hipMemcpyAsync(pl->var.p, vsave, bytes, hipMemcpyDeviceToDevice, pl->stream);
    hipStreamSynchronize(pl->stream);
    pl->ran = had_ran; pl->run_flags = had_flags; pl->res_d = had_d; pl->res_u = had_u;
}

// What every call on the retained factors refuses before it looks at its own arguments, in this order.  `who` names the export;
// host_cannot / sharded_cannot finish "<who>: MRA_KERNEL_HOST plans ..." and "<who>: sharded plans ...".
// (the prior basis is computed by the plan's likelihood pass, which reads the observation layout: set_obs comes first for every call)
// (dry_last: the caller has refusals of its own that a dry-run plan must reach; it refuses the dry run itself, behind them)
void mra_retained_check_plan(const mra_plan* pl, const char* who, uint32_t flags, uint32_t accepted, const char* host_cannot, const char* sharded_cannot,
                                bool dry_last) {
    char m[200];
    if (g_dry && !dry_last) refuse_dry_run();
    if (flags & ~accepted) { snprintf(m, sizeof m, "unknown %s flags", who); throw MraError(MRA_ERR_INVALID, m); }
    if (!(pl->have_locs && pl->have_kernel)) { snprintf(m, sizeof m, "%s needs set_locs and set_kernel first", who); throw MraError(MRA_ERR_STATE, m); }
    if (!pl->have_obs) { snprintf(m, sizeof m, "%s needs set_obs first", who); throw MraError(MRA_ERR_STATE, m); }
    if (pl->host_cov || pl->kp.kind == MRA_KERNEL_HOST) { snprintf(m, sizeof m, "%s: MRA_KERNEL_HOST plans %s", who, host_cannot); throw MraError(MRA_ERR_INVALID, m); }
    if (pl->reduce_level >= 0 || pl->comm || pl->n_ranks > 1) { snprintf(m, sizeof m, "%s: sharded plans %s", who, sharded_cannot); throw MraError(MRA_ERR_INVALID, m); }
}

void mra_check_sample0(int64_t sample0, int64_t n) {      // the n sample numbers from sample0 on
    if (sample0 < 0 || (n > 0 && sample0 > INT64_MAX - (n - 1))) throw MraError(MRA_ERR_INVALID, "sample0 < 0, or a sample number past 2^63 - 1");
}

// "<who>: <noun> is not finite at <where> (column, padded row)": the n columns of M (P each) at the rows of the mask
static void check_finite_rows(const mra_plan* pl, const char* who, const char* noun, const char* where, const std::vector<unsigned char>& mask,
                              const double* M, int64_t n) {
    const long P = pl->P;
    for (int64_t k = 0; k < n; ++k)
        for (long p = 0; p < P; ++p)
            if (mask[p] && !std::isfinite(M[k * P + p])) {
                char m[128];
                snprintf(m, sizeof m, "%s: %s is not finite at %s (column %lld, padded row %ld)", who, noun, where, (long long)k, p);
                throw MraError(MRA_ERR_INVALID, m);
            }
}

// W at every row and the factors, valid: one likelihood pass (as sample_all's prior pass) unless the last one still stands.  What the
// caller reads back afterwards - the last mra_run's likelihood, mean and var - is put back; y and the options are not touched.  After
// mra_solver_build (msave / vsave).
static void ensure_factors(mra_plan* pl) {
    mra_plan::Solver& S = pl->slv;
    if (S.valid) {
        for (int k = 0; k < KF_COUNT; ++k) pl->kstat[k] = mra_plan::KStat();      // the kernel statistics describe this call: no pass ran
        return;
    }
    KeepResults keep(pl, nullptr, S.msave.p, S.vsave.p);
    pl->trend.var_valid = false;         // mra_trend_fit's copy of the predictive variance belonged to the factors that stood
    mra_run_all(pl, MRA_RUN_LIKELIHOOD, true);
    stream_wait(pl);
    S.pass_d = pl->res_d;
    S.valid = true;
}

// nc columns of src (P each) into columns [at, at + nc) of a 16 x P block on the device, the tail behind them zeroed
static void stage_columns(mra_plan* pl, const double* src, int nc, double* dev, hipMemcpyKind kind = hipMemcpyHostToDevice, int at = 0) {
    const size_t P = (size_t)pl->P;
    const int end = at + nc;
    HIP_TRY(hipMemcpyAsync(dev + (size_t)at * P, src, (size_t)nc * P * sizeof(double), kind, pl->stream));
    if (end < 16) HIP_TRY(hipMemsetAsync(dev + (size_t)end * P, 0, (size_t)(16 - end) * P * sizeof(double), pl->stream));
}

// A block that has run is waited for; before that, its 16 x 16 tile (tile_dev) is asked for - timed into entry `which` of the site
// times when >= 0 - and afterwards it lands in the diagonal block at c0 of the n x n host matrix `tile` (nullptr: the wait alone).
static void fetch_diag_tile(mra_plan* pl, const double* tile_dev, double* tile, int64_t n, int64_t c0, int nc, int which = -1) {
    double tb[256];
    const auto copy = [&] { HIP_TRY(hipMemcpyAsync(tb, tile_dev, sizeof tb, hipMemcpyDeviceToHost, pl->stream)); };
    if (tile && which >= 0) mra_sites_timed(pl, which, copy);
    else if (tile) copy();
    stream_wait(pl);
    if (tile)
        for (int i = 0; i < nc; ++i)
            for (int j = 0; j < nc; ++j) tile[(c0 + i) * n + c0 + j] = tb[i * 16 + j];
}

// The n columns of `in`, 16 at a time: staged into in_dev, run_block(), then the block's rows (rows_dev -> rows, when rows is given) and
// its 16 x 16 tile (tile_dev -> the diagonal block of the n x n matrix `tile`, NaN elsewhere, when tile is given) brought back.
static void column_blocks(mra_plan* pl, int64_t n, const double* in, double* in_dev, double* rows, const double* rows_dev, double* tile,
                          const double* tile_dev, const std::function<void()>& run_block) {
    const long P = pl->P;
    if (tile) for (int64_t e = 0; e < n * n; ++e) tile[e] = std::nan("");
    for (int64_t c0 = 0; c0 < n; c0 += 16) {
        const int nc = (int)std::min<int64_t>(16, n - c0);
        stage_columns(pl, in + c0 * P, nc, in_dev);
        run_block();
        if (rows) HIP_TRY(hipMemcpyAsync(rows + c0 * P, rows_dev, (size_t)nc * P * sizeof(double), hipMemcpyDeviceToHost, pl->stream));
        fetch_diag_tile(pl, tile_dev, tile, n, c0, nc);
    }
}

// room for the Kn x16 non-leaf draws of a block of samples (grow-only)
void mra_reserve_coarse(DevVec<double>& v, long Kn) { if (v.n < (size_t)std::max<long>(Kn, 1) * 16) v.alloc((size_t)std::max<long>(Kn, 1) * 16); }

// ---- solver (mra_solve) ------------------------------------------------------------------------------------
// the tiles between the nblk archived blocks, from slv.qfull into the n x n host matrix (the tiles on its diagonal are not touched)
static void fetch_cross_tiles(mra_plan* pl, int nblk, int64_t n, double* quad) {
    mra_plan::Solver& S = pl->slv;
    const int ldq = 16 * S.arch_blocks;
    std::vector<double> q((size_t)nblk * 16 * ldq);
    HIP_TRY(hipMemcpyAsync(q.data(), S.qfull.p, q.size() * sizeof(double), hipMemcpyDeviceToHost, pl->stream));
    stream_wait(pl);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < n; ++j)
            if (i / 16 != j / 16) quad[i * n + j] = q[(size_t)i * ldq + j];
}

void mra_solve_all(mra_plan* pl, uint32_t flags, int64_t n, const double* Y, double* mean, double* quad) {
    mra_retained_check_plan(pl, "mra_solve", flags, MRA_SOLVE_FULL_QUAD, "cannot solve (C(S, o) is evaluated on the device)", "cannot solve");
    if (n < 0) throw MraError(MRA_ERR_INVALID, "n_cols < 0");
    const bool full = (flags & MRA_SOLVE_FULL_QUAD) != 0;
    if (full && n > MRA_FULL_QUAD_MAX) throw MraError(MRA_ERR_INVALID, "mra_solve: MRA_SOLVE_FULL_QUAD takes at most MRA_FULL_QUAD_MAX = 256 columns");
    if (pl->knots_pending) throw MraError(MRA_ERR_STATE, "knot rows not set");
    if (n == 0) return;
    if (!Y) throw MraError(MRA_ERR_INVALID, "Y is NULL");
    check_finite_rows(pl, "mra_solve", "Y", "an observed row", pl->y_finite_host, Y, n);
    HIP_TRY(mraSetDevice(pl->device));
    mra_solver_build(pl);
    ensure_factors(pl);
    mra_plan::Solver& S = pl->slv;
    const int nblk = (int)((n + 15) / 16);
    const bool cross = full && quad && nblk > 1;      // one block: the flagless call already returns the whole matrix
    if (cross) mra_solver_archive(pl, nblk);
    int b = 0;
    column_blocks(pl, n, Y, S.yb.p, mean, S.out.p, quad, S.quad.p, [&] { mra_solver_block(pl, mean != nullptr, quad != nullptr, true, cross ? b++ : -1); });
    if (!cross) return;
    mra_solver_quad_cross(pl, nblk);
    fetch_cross_tiles(pl, nblk, n, quad);
}

// ---- regression trend (mra_plan_set_trend / mra_trend_fit) -----------------------------------------------------
// X: p x P by padded row (phantom rows 0).  Every value is checked before anything changes; nothing but the trend changes.
void mra_trend_set(mra_plan* pl, int32_t p, const double* X) {
    const long P = pl->P;
    if (p < 0) throw MraError(MRA_ERR_INVALID, "mra_plan_set_trend: p < 0");
    if (p > MRA_TREND_MAX) throw MraError(MRA_ERR_INVALID, "mra_plan_set_trend: p > MRA_TREND_MAX = 63 ([y | X] is at most 64 columns)");
    if (p > 0 && !X) throw MraError(MRA_ERR_INVALID, "mra_plan_set_trend: X is NULL with p > 0");
    if (p > 0 && X) {
        std::atomic<long> bad{-1};
        parallel_rows((int64_t)p * P, [&](int64_t a, int64_t b) {
            for (int64_t e = a; e < b; ++e)
                if (!std::isfinite(X[e])) { bad = (long)e; return; }
        });
        if (bad >= 0) {
            char m[160];
            const long e = bad;
            snprintf(m, sizeof m, "mra_plan_set_trend: X is not finite (column %ld, padded row %ld)", e / P, e % P);
            throw MraError(MRA_ERR_INVALID, m);
        }
    }
    mra_plan::Trend& T = pl->trend;
    if (p == 0 || !X) {
        T.p = 0;
        T.X.release(); T.m.release();
        return;
    }
    HIP_TRY(mraSetDevice(pl->device));
    if (T.X.n != (size_t)p * P) T.X.alloc((size_t)p * P);
    HIP_TRY(mraMemcpy(T.X.p, X, (size_t)p * P * sizeof(double), hipMemcpyHostToDevice));
    if (T.p != p) T.m.release();
    T.p = p;
}

// mra_sites_timed adds to trend.ms while this lives (scopes may nest: the outer one's sink is put back)
struct TrendMsSink {
    mra_plan::Sites& s; double* prev;
    explicit TrendMsSink(mra_plan* pl) : s(pl->sit), prev(pl->sit.ms_sink) { s.ms_sink = pl->trend.ms; }
    ~TrendMsSink() { s.ms_sink = prev; }
};

// What the GLS step leaves on the host beside beta and cov_beta: G_tt - b^T beta^, log det A, the extreme pivots of A, and beta^ and
// L^-1 (row stride MRA_TREND_MAX + 1) as k_trend_rows reads them.
struct TrendGls {
    double resid = 0.0, logdet = 0.0, pmin = INFINITY, pmax = 0.0;
    std::vector<double> Li, bt;
};

// room for the kriging means of the 1 + p columns [y | X] (trend.m) and for beta^ and L^-1 as the kernels read them (trend.coef)
static void trend_reserve(mra_plan* pl) {
    mra_plan::Trend& T = pl->trend;
    constexpr size_t LD = MRA_TREND_MAX + 1;
    const size_t need = (size_t)(T.p + 1) * (size_t)pl->P;
    if (T.m.n != need) T.m.alloc(need);
    if (!T.coef.n) T.coef.alloc(LD + LD * LD);
}

// beta^ of a GLS step - and L^-1 behind it when with_Li - into trend.coef, timed into entry `which`.  (R's host arrays are read by
// the copies until the stream is next synchronised.)
static void trend_upload_coef(mra_plan* pl, const TrendGls& R, bool with_Li, int which) {
    constexpr size_t LD = MRA_TREND_MAX + 1;
    double* coef = pl->trend.coef.p;
    mra_sites_timed(pl, which, [&] {
        HIP_TRY(hipMemcpyAsync(coef, R.bt.data(), LD * sizeof(double), hipMemcpyHostToDevice, pl->stream));
        if (with_Li) HIP_TRY(hipMemcpyAsync(coef + LD, R.Li.data(), LD * LD * sizeof(double), hipMemcpyHostToDevice, pl->stream));
    });
}

// The GLS step of mra_trend_fit and of every iteration of mra_plan_fit_laplace_trend, on factors that stand: G = [y | X]^T K^-1 [y | X]
// block by block from the device's own y and X, A = L L^T and beta^ = A^-1 b on the host.  pred: the backward sweeps and the row
// kernel per block as well, the kriging means of the 1 + p columns into trend.m.  `who` names the export in the refusal.
static void trend_gls(mra_plan* pl, const char* who, bool pred, double* beta, double* cov_beta, TrendGls& R) {
    mra_plan::Trend& T = pl->trend;
    mra_plan::Solver& S = pl->slv;
    const long P = pl->P;
    const int p = T.p, n = p + 1, nblk = (n + 15) / 16;
    TrendMsSink sink(pl);
    // G = [y | X]^T K^-1 [y | X], block by block from the device's own y and X (timed as the site calls are, into trend.ms)
    if (nblk > 1) mra_solver_archive(pl, nblk);
    std::vector<double> G((size_t)n * n, 0.0);
    for (int b = 0; b < nblk; ++b) {
        const int c0 = 16 * b, nc = std::min(16, n - c0);
        mra_sites_timed(pl, 0, [&] {      // (the first block is [y | X's first columns]: p >= 1, so it has at least one of them)
            if (b == 0) {
                HIP_TRY(hipMemcpyAsync(S.yb.p, pl->y.p, (size_t)P * sizeof(double), hipMemcpyDeviceToDevice, pl->stream));
                stage_columns(pl, T.X.p, nc - 1, S.yb.p, hipMemcpyDeviceToDevice, 1);
            } else stage_columns(pl, T.X.p + (size_t)(c0 - 1) * P, nc, S.yb.p, hipMemcpyDeviceToDevice);
        });
        mra_sites_timed(pl, 1, [&] { mra_solver_block(pl, pred, true, true, nblk > 1 ? b : -1); });
        if (pred)
            mra_sites_timed(pl, 0, [&] {
                HIP_TRY(hipMemcpyAsync(T.m.p + (size_t)c0 * P, S.out.p, (size_t)nc * P * sizeof(double), hipMemcpyDeviceToDevice, pl->stream));
            });
        fetch_diag_tile(pl, S.quad.p, G.data(), n, c0, nc, 4);
    }
    if (nblk > 1) {
        mra_sites_timed(pl, 2, [&] { mra_solver_quad_cross(pl, nblk); });
        mra_sites_timed(pl, 4, [&] { fetch_cross_tiles(pl, nblk, n, G.data()); });
    }
    // A = L L^T on the host (at most 63 x 63); Li = L^-1
    constexpr int LD = MRA_TREND_MAX + 1;
    std::vector<double> L((size_t)p * p, 0.0);
    std::vector<double>&Li = R.Li, &bt = R.bt;
    Li.assign((size_t)LD * LD, 0.0); bt.assign((size_t)LD, 0.0);
    double dmax = 0.0, pmin = INFINITY, pmax = 0.0, logdet = 0.0;
    for (int i = 0; i < p; ++i) dmax = std::max(dmax, G[(size_t)(i + 1) * n + i + 1]);
    const double floor_ = (double)p * 2.220446049250313e-16 * dmax;
    for (int j = 0; j < p; ++j) {
        double piv = G[(size_t)(j + 1) * n + j + 1];
        for (int k = 0; k < j; ++k) piv -= L[(size_t)j * p + k] * L[(size_t)j * p + k];
        if (!(piv > 0.0) || !(piv >= floor_) || !std::isfinite(piv)) {
            char msg[128];
            snprintf(msg, sizeof msg, "%s: trend columns are linearly dependent at the observed rows", who);
            throw MraError(MRA_ERR_NOT_SPD, msg);
        }
        const double ljj = std::sqrt(piv);
        L[(size_t)j * p + j] = ljj;
        pmin = std::min(pmin, piv); pmax = std::max(pmax, piv); logdet += std::log(piv);
        for (int i = j + 1; i < p; ++i) {
            double v = G[(size_t)(i + 1) * n + j + 1];
            for (int k = 0; k < j; ++k) v -= L[(size_t)i * p + k] * L[(size_t)j * p + k];
            L[(size_t)i * p + j] = v / ljj;
        }
    }
    for (int c = 0; c < p; ++c)              // L Li = I, column by column
        for (int i = c; i < p; ++i) {
            double v = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) v -= L[(size_t)i * p + k] * Li[(size_t)k * LD + c];
            Li[(size_t)i * LD + c] = v / L[(size_t)i * p + i];
        }
    std::vector<double> wv((size_t)p, 0.0);  // w = L^-1 b; beta = L^-T w
    for (int i = 0; i < p; ++i) {
        double v = 0.0;
        for (int k = 0; k <= i; ++k) v += Li[(size_t)i * LD + k] * G[(size_t)(k + 1) * n];
        wv[i] = v;
    }
    for (int i = 0; i < p; ++i) {
        double v = 0.0;
        for (int k = i; k < p; ++k) v += Li[(size_t)k * LD + i] * wv[k];
        beta[i] = v; bt[i] = v;
    }
    if (cov_beta)
        for (int i = 0; i < p; ++i)
            for (int j = 0; j < p; ++j) {
                double v = 0.0;
                for (int k = std::max(i, j); k < p; ++k) v += Li[(size_t)k * LD + i] * Li[(size_t)k * LD + j];
                cov_beta[(size_t)i * p + j] = v;
            }
    double bb = 0.0;
    for (int i = 0; i < p; ++i) bb += G[(size_t)(i + 1) * n] * beta[i];
    R.resid = G[0] - bb; R.logdet = logdet; R.pmin = pmin; R.pmax = pmax;
}

// trend.ms of a call that is about to run its sweeps: the times start at 0, the last two are what one block's sweeps move
static void trend_ms_reset(mra_plan* pl) {
    mra_plan::Trend& T = pl->trend;
    for (double& v : T.ms) v = 0.0;
    for (size_t t = 0; t < pl->leaf_nodes.size(); ++t)
        T.ms[5] += 8.0 * (double)(pl->Ka - pl->asuf[pl->node_level[pl->leaf_nodes[t]]]) * (double)pl->leaf_nop[t];
    T.ms[6] = 8.0 * 16.0 * (double)pl->slv.arch_rows;
}

static long observed_rows(const mra_plan* pl) {
    long nobs = 0;
    for (size_t t = 0; t < pl->leaf_nodes.size(); ++t)
        for (long r = pl->row0[pl->leaf_nodes[t]]; r < pl->row1[pl->leaf_nodes[t]]; ++r) nobs += pl->y_finite_host[r] ? 1 : 0;
    return nobs;
}

void mra_trend_fit_all(mra_plan* pl, uint32_t flags, double* beta, double* cov_beta, double* mean, double* var, double* info) {
    mra_retained_check_plan(pl, "mra_trend_fit", flags, MRA_TREND_PREDICT, "cannot fit a trend (C(S, o) is evaluated on the device)", "cannot fit a trend");
    mra_plan::Trend& T = pl->trend;
    if (T.p == 0) throw MraError(MRA_ERR_STATE, "mra_trend_fit needs mra_plan_set_trend first");
    if (!beta || !info) throw MraError(MRA_ERR_INVALID, "mra_trend_fit: beta or info is NULL");
    const bool pred = (flags & MRA_TREND_PREDICT) != 0;
    if (!pred && (mean || var)) throw MraError(MRA_ERR_INVALID, "mra_trend_fit: mean_perm or var_perm given without MRA_TREND_PREDICT");
    if (pl->knots_pending) throw MraError(MRA_ERR_STATE, "knot rows not set");
    const long P = pl->P;
    const int p = T.p;
    HIP_TRY(mraSetDevice(pl->device));
    mra_solver_build(pl);
    mra_plan::Solver& S = pl->slv;
    if (pred) {
        trend_reserve(pl);
        if (T.var_pass.n != (size_t)P) { T.var_pass.alloc((size_t)P); T.mean.alloc((size_t)P); T.var.alloc((size_t)P); T.var_valid = false; }
        if (!(S.valid && T.var_valid)) {
            // the variance of a predict pass on the plan's own y; that pass rewrites W, so the factors are made again behind it
            {
                KeepResults keep(pl, nullptr, S.msave.p, S.vsave.p);
                mra_run_all(pl, MRA_RUN_LIKELIHOOD | MRA_RUN_PREDICT);
                HIP_TRY(hipMemcpyAsync(T.var_pass.p, pl->var.p, (size_t)P * sizeof(double), hipMemcpyDeviceToDevice, pl->stream));
            }
            S.valid = false;
            ensure_factors(pl);
            T.var_valid = true;
        } else ensure_factors(pl);
    } else ensure_factors(pl);
    trend_ms_reset(pl);
    TrendMsSink sink(pl);                    // the GLS step, the upload of beta and L^-1, k_trend_rows and the downloads: all into trend.ms
    TrendGls R;
    trend_gls(pl, "mra_trend_fit", pred, beta, cov_beta, R);
    info[0] = S.pass_d; info[1] = R.resid; info[2] = R.logdet; info[3] = info[0] + info[1]; info[4] = info[3] + info[2];
    info[5] = (double)observed_rows(pl); info[6] = (double)p; info[7] = R.pmin / R.pmax;
    if (!pred) return;
    trend_upload_coef(pl, R, true, 4);
    mra_sites_timed(pl, 3, [&] { mra_trend_rows(pl); });
    mra_sites_timed(pl, 4, [&] {
        if (mean) HIP_TRY(hipMemcpyAsync(mean, T.mean.p, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, pl->stream));
        if (var) HIP_TRY(hipMemcpyAsync(var, T.var.p, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, pl->stream));
    });
    stream_wait(pl);
}

// ---- covariance operator (mra_cov_apply) ------------------------------------------------------------------
void mra_cov_all(mra_plan* pl, uint32_t flags, int64_t n, const double* A, double* out, double* gram) {
    mra_retained_check_plan(pl, "mra_cov_apply", flags, MRA_COV_POSTERIOR, "cannot apply the covariance (C(S, S) is evaluated on the device)",
                        "cannot apply the covariance");
    if (n < 0) throw MraError(MRA_ERR_INVALID, "n_cols < 0");
    if (pl->knots_pending) throw MraError(MRA_ERR_STATE, "knot rows not set");
    if (n == 0) return;
    if (!A) throw MraError(MRA_ERR_INVALID, "A is NULL");
    const bool post = flags & MRA_COV_POSTERIOR;
    HIP_TRY(mraSetDevice(pl->device));
    mra_solver_build(pl);
    mra_cov_build(pl);
    check_finite_rows(pl, "mra_cov_apply", "A", "a reported row", mra_row_maps(pl).rep_host, A, n);
    ensure_factors(pl);      // W at every row and, for the posterior, the factors
    mra_plan::Cov& V = pl->cov;
    column_blocks(pl, n, A, V.ab.p, out, V.out.p, gram, V.gram.p, [&] { mra_cov_block(pl, post, gram != nullptr); });
}

// ---- prediction at new sites (mra_predict_sites) ----------------------------------------------------------------
// The tiles of a call: the sites grouped by leaf (stable: a leaf's sites keep the caller's order), each group padded to a multiple of 16
// with copies of its first site.  slot[tile * 16 + k] = the caller's site of that column, -1 for padding.  Plain host code.
// sites 0 .. n-1 grouped by leaf slot, a stable counting sort: leaf t's sites are order[cnt[t] .. cnt[t + 1]), in the caller's order
static void group_by_leaf(const std::vector<int>& lslot, int64_t n, size_t nl, std::vector<int64_t>& cnt, std::vector<int64_t>& order) {
    cnt.assign(nl + 1, 0); order.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) ++cnt[(size_t)lslot[(size_t)i] + 1];
    for (size_t t = 0; t < nl; ++t) cnt[t + 1] += cnt[t];
    std::vector<int64_t> at(cnt.begin(), cnt.end() - 1);
    for (int64_t i = 0; i < n; ++i) order[(size_t)at[(size_t)lslot[(size_t)i]]++] = i;
}

static void sites_tiles(const std::vector<int>& slot_of_leaf_site, int64_t n, size_t nl, std::vector<int64_t>& slot, std::vector<int>& tile_leaf) {
    std::vector<int64_t> cnt, order;
    group_by_leaf(slot_of_leaf_site, n, nl, cnt, order);
    slot.clear(); tile_leaf.clear();
    for (size_t t = 0; t < nl; ++t) {
        const int64_t g0 = cnt[t], g1 = cnt[t + 1];
        if (g1 == g0) continue;
        for (int64_t g = g0; g < g1; g += 16) {
            tile_leaf.push_back((int)t);
            for (int64_t k = 0; k < 16; ++k) slot.push_back(g + k < g1 ? order[(size_t)(g + k)] : -1);
        }
    }
}

// What the three site calls check before anything is launched, in this order: the plan (sites_check_plan), then the call's own
// arguments, then the sites (sites_check_sites, which also gives each site's leaf slot).  `who` names the export in the messages.
static void sites_check_plan(const mra_plan* pl, const char* who, uint32_t flags, uint32_t accepted, int64_t n) {
    mra_retained_check_plan(pl, who, flags, accepted, "cannot predict at new sites (C(Q, s) is evaluated on the device)", "cannot predict at new sites");
    if (n < 0) throw MraError(MRA_ERR_INVALID, "n_sites < 0");
}

static std::vector<int> sites_check_sites(const mra_plan* pl, const char* who, int64_t n, const double* sites, const int32_t* leaf) {
    if (pl->knots_pending) throw MraError(MRA_ERR_STATE, "knot rows not set");
    if (n > 0 && (!sites || !leaf)) throw MraError(MRA_ERR_INVALID, "sites or leaf is NULL");
    const int d = pl->d;
    std::vector<int> lslot((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        char m[128];
        if (leaf[i] < 0 || leaf[i] >= pl->n_nodes || !pl->leaf[leaf[i]] || pl->leaf_slot[leaf[i]] < 0) {
            snprintf(m, sizeof m, "%s: leaf[%lld] = %d is not a leaf node", who, (long long)i, (int)leaf[i]);
            throw MraError(MRA_ERR_INVALID, m);
        }
        lslot[(size_t)i] = pl->leaf_slot[leaf[i]];
        for (int e = 0; e < d; ++e)
            if (!std::isfinite(sites[i * d + e])) {
                snprintf(m, sizeof m, "%s: site %lld has a non-finite coordinate", who, (long long)i);
                throw MraError(MRA_ERR_INVALID, m);
            }
        if (pl->kp.mode == 6 && !(sites[i * d + d - 1] > 0.0)) {       // MRA_KERNEL_LOCAL: the site's range, as mra_plan_set_locs checks the plan's
            snprintf(m, sizeof m, "%s: site %lld has a range (last column) that is not positive", who, (long long)i);
            throw MraError(MRA_ERR_INVALID, m);
        }
    }
    return lslot;
}

// the sites of the three site calls as the kernels read them: the caller's own without a metric, else A s by the metric's one function
static const double* sites_in_metric(const mra_plan* pl, int64_t n, const double* sites, std::vector<double>& store) {
    if (!pl->metric_on || n <= 0) return sites;
    const int d = pl->d;
    store.resize((size_t)n * d);
    for (int64_t i = 0; i < n; ++i) mra_metric_row_d(d, pl->metric_A, sites + i * d, store.data() + i * d);
    return store.data();
}

// The state the site calls run on: the site descriptors, and W at every row and the factors
static void sites_ensure_state(mra_plan* pl) {
    HIP_TRY(mraSetDevice(pl->device));
    mra_sites_build(pl);
    ensure_factors(pl);
}

// mra_sites_timed adds to the n entries of `ms`, which start at 0, instead of sit.ms while this lives
struct SitesSink {
    mra_plan::Sites& T;
    SitesSink(mra_plan::Sites& t, double* ms, int n) : T(t) { std::fill(ms, ms + n, 0.0); T.ms_sink = ms; }
    ~SitesSink() { T.ms_sink = nullptr; }
};

// the coordinates of tiles [t0, t0 + nt) for the device: padding columns repeat their tile's first site
static void sites_gather(const std::vector<int64_t>& slot, long t0, long nt, int d, const double* sites, double* xs) {
    for (long e = 0; e < nt * 16; ++e) {
        const int64_t src = slot[(size_t)(t0 * 16 + e)];
        const int64_t i = src >= 0 ? src : slot[(size_t)((t0 * 16 + e) & ~(int64_t)15)];
        for (int k = 0; k < d; ++k) xs[(size_t)e * d + k] = sites[i * d + k];
    }
}

void mra_predict_sites_all(mra_plan* pl, uint32_t flags, int64_t n, const double* sites, const int32_t* leaf, int64_t nc,
                              const double* Y, double* mean, double* var) {
    sites_check_plan(pl, "mra_predict_sites", flags, 0, n);
    if (nc < 0) throw MraError(MRA_ERR_INVALID, "n_cols < 0");
    if (!Y && nc != 1) throw MraError(MRA_ERR_INVALID, "Y is NULL (the plan's own observations): n_cols must be 1");
    const std::vector<int> lslot = sites_check_sites(pl, "mra_predict_sites", n, sites, leaf);
    std::vector<double> msites;
    sites = sites_in_metric(pl, n, sites, msites);
    const long P = pl->P;
    const int d = pl->d;
    const bool want_mean = mean != nullptr && nc > 0;
    if (Y) check_finite_rows(pl, "mra_predict_sites", "Y", "an observed row", pl->y_finite_host, Y, nc);
    if (n == 0) return;
    sites_ensure_state(pl);
    mra_plan::Solver& S = pl->slv;
    mra_plan::Sites& T = pl->sit;
    for (double& v : T.ms) v = 0.0;
    std::vector<int64_t> slot;
    std::vector<int> tile_leaf;
    sites_tiles(lslot, n, pl->leaf_nodes.size(), slot, tile_leaf);
    const long n_tiles = (long)tile_leaf.size();
    const size_t budget = T.chunk_bytes ? T.chunk_bytes : SITES_CHUNK_BYTES;
    const long per_chunk = std::min<long>(n_tiles, std::max<long>(1, (long)(budget / mra_sites_tile_bytes(pl))));
    mra_sites_reserve(pl, per_chunk);
    std::vector<double> xs((size_t)per_chunk * 16 * d), vh((size_t)per_chunk * 16), mh(want_mean ? (size_t)per_chunk * 256 : 0);
    const int64_t n_blocks = want_mean ? (nc + 15) / 16 : (var ? 1 : 0);
    for (int64_t cb = 0; cb < n_blocks; ++cb) {
        const int ncb = want_mean ? (int)std::min<int64_t>(16, nc - cb * 16) : 0;
        if (want_mean) {
            // the block's beta (leaves' gb) and q (leaves' uy): the solver's sweeps without its row step
            if (Y) stage_columns(pl, Y + cb * 16 * P, ncb, S.yb.p);
            else stage_columns(pl, pl->y.p, 1, S.yb.p, hipMemcpyDeviceToDevice);      // (n_cols is 1)
            mra_sites_timed(pl, 4, [&] { mra_solver_block(pl, true, false, false); });
        }
        for (long t0 = 0; t0 < n_tiles; t0 += per_chunk) {
            const long nt = std::min(per_chunk, n_tiles - t0);
            sites_gather(slot, t0, nt, d, sites, xs.data());
            mra_sites_timed(pl, 5, [&] {
                HIP_TRY(hipMemcpyAsync(T.xs.p, xs.data(), (size_t)nt * 16 * d * sizeof(double), hipMemcpyHostToDevice, pl->stream));
                HIP_TRY(hipMemcpyAsync(T.tleaf.p, tile_leaf.data() + t0, (size_t)nt * sizeof(int), hipMemcpyHostToDevice, pl->stream));
            });
            mra_sites_basis(pl, nt);
            const bool do_var = var && cb == 0;
            if (do_var) {
                mra_sites_var(pl, nt);
                mra_sites_timed(pl, 6, [&] { HIP_TRY(hipMemcpyAsync(vh.data(), T.var.p, (size_t)nt * 16 * sizeof(double), hipMemcpyDeviceToHost, pl->stream)); });
            }
            if (want_mean) {
                mra_sites_mean(pl, nt, ncb);
                mra_sites_timed(pl, 6, [&] { HIP_TRY(hipMemcpyAsync(mh.data(), T.mean.p, (size_t)ncb * nt * 16 * sizeof(double), hipMemcpyDeviceToHost, pl->stream)); });
            }
            stream_wait(pl);
            for (long e = 0; e < nt * 16; ++e) {
                const int64_t i = slot[(size_t)(t0 * 16 + e)];
                if (i < 0) continue;
                if (do_var) var[i] = vh[(size_t)e];
                for (int c = 0; c < ncb; ++c) mean[(cb * 16 + c) * n + i] = mh[(size_t)c * nt * 16 + e];
            }
        }
    }
}

// ---- joint covariance of new sites (mra_sites_cov) ---------------------------------------------------------------
// Every tile's a (prior) or a, t, b (posterior) stays on the device for the call; the matrix comes back in row panels of whole tiles,
// each block at or after the diagonal computed once and written to both triangles here: `out` is symmetric by construction.
void mra_sites_cov_all(mra_plan* pl, uint32_t flags, int64_t n, const double* sites, const int32_t* leaf, double* out) {
    sites_check_plan(pl, "mra_sites_cov", flags, MRA_COV_POSTERIOR, n);
    if (n > MRA_SITES_COV_MAX) {
        char m[200];
        snprintf(m, sizeof m, "mra_sites_cov: n_sites = %lld is above MRA_SITES_COV_MAX = %d (the result is a dense matrix, 2 GiB at the cap)", (long long)n, MRA_SITES_COV_MAX);
        throw MraError(MRA_ERR_INVALID, m);
    }
    if (n > 0 && !out) throw MraError(MRA_ERR_INVALID, "out is NULL");
    const std::vector<int> lslot = sites_check_sites(pl, "mra_sites_cov", n, sites, leaf);
    std::vector<double> msites;
    sites = sites_in_metric(pl, n, sites, msites);
    if (n == 0) return;
    const bool post = (flags & MRA_COV_POSTERIOR) != 0;
    const int d = pl->d;
    sites_ensure_state(pl);
    mra_plan::Sites& T = pl->sit;
    SitesSink sink(T, T.cov_ms, 6);
    std::vector<int64_t> slot;
    std::vector<int> tile_leaf;
    sites_tiles(lslot, n, pl->leaf_nodes.size(), slot, tile_leaf);
    const long n_tiles = (long)tile_leaf.size(), ld = n_tiles * 16;
    const size_t budget = T.chunk_bytes ? T.chunk_bytes : SITES_CHUNK_BYTES;
    const long rows = std::min<long>(std::min<long>(n_tiles, 65535), std::max<long>(1, (long)(budget / ((size_t)16 * ld * sizeof(double)))));
    mra_sites_reserve(pl, n_tiles);
    if (T.gram.n < (size_t)rows * 16 * ld) T.gram.alloc((size_t)rows * 16 * ld);
    {
        std::vector<double> xs((size_t)n_tiles * 16 * d);
        sites_gather(slot, 0, n_tiles, d, sites, xs.data());
        mra_sites_timed(pl, 4, [&] {
            HIP_TRY(hipMemcpyAsync(T.xs.p, xs.data(), xs.size() * sizeof(double), hipMemcpyHostToDevice, pl->stream));
            HIP_TRY(hipMemcpyAsync(T.tleaf.p, tile_leaf.data(), (size_t)n_tiles * sizeof(int), hipMemcpyHostToDevice, pl->stream));
        });
        mra_sites_basis(pl, n_tiles);
        if (post) mra_sites_var(pl, n_tiles);
        stream_wait(pl);       // xs is read by the copy until here
    }
    std::vector<double> panel((size_t)rows * 16 * ld);
    for (long t0 = 0; t0 < n_tiles; t0 += rows) {
        const long nr = std::min(rows, n_tiles - t0);
        mra_sites_gram(pl, n_tiles, t0, nr, post);
        // the panel from its first diagonal block on: what lies before it in the first row is never written
        const size_t first = (size_t)t0 * 16, count = (size_t)nr * 16 * ld - first;
        mra_sites_timed(pl, 5, [&] { HIP_TRY(hipMemcpyAsync(panel.data() + first, T.gram.p + first, count * sizeof(double), hipMemcpyDeviceToHost, pl->stream)); });
        stream_wait(pl);
        for (long I = t0; I < t0 + nr; ++I)
            for (long J = I; J < n_tiles; ++J)
                for (int a = 0; a < 16; ++a) {
                    const int64_t u = slot[(size_t)(I * 16 + a)];
                    if (u < 0) continue;
                    const double* row = panel.data() + ((size_t)(I - t0) * 16 + a) * ld + J * 16;
                    for (int b = (I == J ? a : 0); b < 16; ++b) {
                        const int64_t w = slot[(size_t)(J * 16 + b)];
                        if (w < 0) continue;
                        out[u * n + w] = row[b];
                        out[w * n + u] = row[b];
                    }
                }
    }
}

// ---- batches of whole leaves (mra_sample_sites and mra_cv, DESIGN.md sections 14 and 18) ------------------------------------------------
// visit(t, nt): the runs of equal tile_leaf among the tiles [t0, t0 + n) - each the nt tiles of one leaf, the first of them tile t0 + t
static void leaf_runs(const std::vector<int>& tile_leaf, long t0, long n, const std::function<void(long, long)>& visit) {
    for (long t = 0; t < n;) {
        long t1 = t;
        while (t1 < n && tile_leaf[(size_t)(t0 + t1)] == tile_leaf[(size_t)(t0 + t)]) ++t1;
        visit(t, t1 - t);
        t = t1;
    }
}

// The tiles [t0, t0 + nt) of a call: n_leaves whole leaves, the largest of nt_max tiles, g doubles of dense blocks ((16 nt_l)^2 a leaf).
// cap_t, cap_l, cap_g: the most tiles, leaves and block doubles of any batch.
struct LeafBatch { long t0, nt, n_leaves; size_t g; int nt_max; };
struct LeafBatches { std::vector<LeafBatch> bat; long cap_t = 0, cap_l = 0; size_t cap_g = 0; };
// Consecutive whole leaves while their bytes stay within the budget (at least one leaf per batch): tile_bytes per tile, and `blocks`
// dense blocks per leaf.  blocks == 0: no leaf has a block, and g stays 0.
static LeafBatches leaf_batches(const std::vector<int>& tile_leaf, size_t tile_bytes, size_t budget, int blocks) {
    LeafBatches B;
    LeafBatch cur{0, 0, 0, 0, 0};
    size_t bytes = 0;
    leaf_runs(tile_leaf, 0, (long)tile_leaf.size(), [&](long t0, long nt) {
        const size_t g = blocks ? (size_t)(16 * nt) * (size_t)(16 * nt) : 0, need = (size_t)nt * tile_bytes + (size_t)blocks * g * sizeof(double);
        if (cur.nt && bytes + need > budget) { B.bat.push_back(cur); cur = LeafBatch{t0, 0, 0, 0, 0}; bytes = 0; }
        cur.nt += nt; ++cur.n_leaves; cur.g += g; cur.nt_max = std::max(cur.nt_max, (int)nt); bytes += need;
    });
    B.bat.push_back(cur);
    for (const LeafBatch& b : B.bat) { B.cap_t = std::max(B.cap_t, b.nt); B.cap_l = std::max(B.cap_l, b.n_leaves); B.cap_g = std::max(B.cap_g, b.g); }
    return B;
}

// One batch's descriptors on the host: every tile's SiteDrawTile and every leaf's PanelProb - its block in sit.G (at 0 for every leaf
// when the batch has no blocks) and its inverted diagonal blocks in sit.invd.  leaf(k, d, node): the batch's leaf k, d as its tiles carry it.
static void leaf_batch_fill(mra_plan* pl, const std::vector<int>& tile_leaf, const LeafBatch& b, std::vector<SiteDrawTile>& dt, std::vector<PanelProb>& pp,
                            const std::function<void(long, const SiteDrawTile&, int)>& leaf) {
    mra_plan::Sites& T = pl->sit;
    size_t goff = 0;
    long k = 0;
    leaf_runs(tile_leaf, b.t0, b.nt, [&](long t, long nt) {
        const SiteDrawTile d{(long)goff, (int)t, (int)nt};
        std::fill(dt.begin() + t, dt.begin() + t + nt, d);
        pp[(size_t)k] = PanelProb{T.G.p + goff, T.invd.p + (size_t)t * 256, 16 * nt, (int)nt, (int)nt, (int)k};
        leaf(k, d, pl->leaf_nodes[(size_t)tile_leaf[(size_t)(b.t0 + t)]]);
        if (b.g) goff += (size_t)(16 * nt) * (size_t)(16 * nt);
        ++k;
    });
}

// ---- draws at new sites (mra_sample_sites) -----------------------------------------------------------------------
// Exact duplicates (same leaf, equal coordinates) collapse to their first occurrence: -> first[i] = the caller's index of it; distinct =
// the sites that are their own first, in the caller's order.  Refuses a leaf that receives too many distinct sites.
static std::vector<int64_t> collapse_duplicates(const mra_plan* pl, const std::vector<int>& lslot, int64_t n, const double* sites, std::vector<int64_t>& distinct) {
    const int d = pl->d;
    const size_t nl = pl->leaf_nodes.size();
    std::vector<int64_t> first((size_t)n);
    // grouped by leaf, then each leaf's sites by coordinates: equal sites become neighbours, first index first
    std::vector<int64_t> order, cnt;
    group_by_leaf(lslot, n, nl, cnt, order);
    auto less = [&](int64_t x, int64_t y) {
        for (int e = 0; e < d; ++e)
            if (sites[x * d + e] != sites[y * d + e]) return sites[x * d + e] < sites[y * d + e];
        return x < y;
    };
    for (size_t t = 0; t < nl; ++t) std::sort(order.begin() + cnt[t], order.begin() + cnt[t + 1], less);
    for (int64_t k = 0; k < n; ++k) {
        const int64_t i = order[(size_t)k], h = k ? first[(size_t)order[(size_t)(k - 1)]] : -1;
        bool same = k > 0 && lslot[(size_t)i] == lslot[(size_t)h];
        for (int e = 0; same && e < d; ++e) same = sites[i * d + e] == sites[h * d + e];
        first[(size_t)i] = same ? h : i;
    }
    std::vector<int64_t> per_leaf(nl, 0);
    for (int64_t i = 0; i < n; ++i)
        if (first[(size_t)i] == i) {
            distinct.push_back(i);
            if (++per_leaf[(size_t)lslot[(size_t)i]] == (int64_t)MRA_SAMPLE_SITES_LEAF_MAX + 1) {
                char m[200];
                snprintf(m, sizeof m, "mra_sample_sites: leaf %d receives more than MRA_SAMPLE_SITES_LEAF_MAX = %d distinct sites (its block is dense, 128 MiB at the cap)",
                         pl->leaf_nodes[(size_t)lslot[(size_t)i]], MRA_SAMPLE_SITES_LEAF_MAX);
                throw MraError(MRA_ERR_INVALID, m);
            }
        }
    return first;
}

// a leaf's chain for the coarse term: first row in a / p, first latent slot, width - root first, as mra_sites_build's chain.  -> the
// latent slots of the non-leaf nodes
static long draw_chains(mra_plan* pl) {
    const size_t nl = pl->leaf_nodes.size();
    std::vector<long> zoff;
    const long Kn = mra_coarse_slots(pl, &zoff);
    std::vector<SiteDrawChain> ch;
    std::vector<int> ptr(nl + 1, 0);
    for (size_t t = 0; t < nl; ++t) {
        const int i = pl->leaf_nodes[t], a0 = pl->asuf[pl->node_level[i]];
        for (int p : leaf_ancestors(pl, i)) {
            const int k = pl->node_level[p];
            if (pl->cw[k]) ch.push_back(SiteDrawChain{pl->coff[k] - a0, (int)zoff[(size_t)p], pl->cw[k], 0});
        }
        ptr[t + 1] = (int)ch.size();
    }
    if (ch.empty()) ch.push_back(SiteDrawChain{0, 0, 0, 0});
    pl->sit.dchain.upload(ch); pl->sit.dchain_ptr.upload(ptr);
    return Kn;
}

// What the batches of one call share: the caller's arguments, the tiles of the distinct sites (slot[] = the caller's index of each
// column), the latent slots, and the host buffers of one batch
struct SiteDraw {
    int64_t n, ns_all; const double* sites; uint64_t seed; int64_t sample0; const double* z; double* out; bool post;
    long Kn = 0, n_slots = 0;
    std::vector<int64_t> slot;
    std::vector<int> tile_leaf, leaf_of_prob;
    std::vector<double> xs, oh, zch, zlh;
    std::vector<SiteDrawTile> dt; std::vector<PanelProb> pp;
};

// the caller's draws of samples [s0, s0 + ns) in the layouts the kernels read, to the device: the non-leaf slots sample-major (ldz =
// Kn) into sit.zcin, the batch's leaf slots [site][16] into sit.zin
static void draw_stage_z(mra_plan* pl, SiteDraw& D, const LeafBatch& b, int64_t s0, int ns) {
    mra_plan::Sites& T = pl->sit;
    const long Kn = D.Kn;
    for (int s = 0; s < ns; ++s) {
        const double* zr = D.z + (s0 + s) * D.n_slots;
        for (long k = 0; k < Kn; ++k) D.zch[(size_t)s * Kn + k] = zr[k];
        for (long u = 0; u < b.nt * 16; ++u) {
            const int64_t i = D.slot[(size_t)(b.t0 * 16 + u)];
            D.zlh[(size_t)u * 16 + s] = i >= 0 ? zr[Kn + i] : 0.0;
        }
    }
    for (int s = ns; s < 16; ++s)
        for (long u = 0; u < b.nt * 16; ++u) D.zlh[(size_t)u * 16 + s] = 0.0;
    mra_sites_timed(pl, 7, [&] {
        if (Kn) HIP_TRY(hipMemcpyAsync(T.zcin.p, D.zch.data(), (size_t)ns * Kn * sizeof(double), hipMemcpyHostToDevice, pl->stream));
        HIP_TRY(hipMemcpyAsync(T.zin.p, D.zlh.data(), (size_t)b.nt * 256 * sizeof(double), hipMemcpyHostToDevice, pl->stream));
    });
}

// One batch: its sites and descriptors to the device, the basis (the posterior: the moments too), the leaves' blocks and their Cholesky
// factors, then the draws, 16 samples at a time, into the caller's columns.  Every block of samples ends with a synchronisation: the
// host buffers are free for the next one.
static void draw_batch(mra_plan* pl, SiteDraw& D, const LeafBatch& b) {
    mra_plan::Sites& T = pl->sit;
    const long Kn = D.Kn;
    sites_gather(D.slot, b.t0, b.nt, pl->d, D.sites, D.xs.data());
    leaf_batch_fill(pl, D.tile_leaf, b, D.dt, D.pp, [&](long k, const SiteDrawTile&, int node) { D.leaf_of_prob[(size_t)k] = node; });
    mra_sites_timed(pl, 7, [&] {
        HIP_TRY(hipMemcpyAsync(T.xs.p, D.xs.data(), (size_t)b.nt * 16 * pl->d * sizeof(double), hipMemcpyHostToDevice, pl->stream));
        HIP_TRY(hipMemcpyAsync(T.tleaf.p, D.tile_leaf.data() + b.t0, (size_t)b.nt * sizeof(int), hipMemcpyHostToDevice, pl->stream));
        HIP_TRY(hipMemcpyAsync(T.dtile.p, D.dt.data(), (size_t)b.nt * sizeof(SiteDrawTile), hipMemcpyHostToDevice, pl->stream));
        HIP_TRY(hipMemcpyAsync(T.sslot.p, D.slot.data() + b.t0 * 16, (size_t)b.nt * 16 * sizeof(long), hipMemcpyHostToDevice, pl->stream));
        HIP_TRY(hipMemcpyAsync(T.dprob.p, D.pp.data(), (size_t)b.n_leaves * sizeof(PanelProb), hipMemcpyHostToDevice, pl->stream));
    });
    mra_sites_basis(pl, b.nt);
    if (D.post) { mra_sites_var(pl, b.nt); mra_sites_mean(pl, b.nt, 1, 6); }
    mra_sites_leaf_gram(pl, b.nt, b.nt_max, D.post);
    mra_sites_timed(pl, 4, [&] {
        HIP_TRY(hipMemsetAsync(T.derr.p, 0, sizeof(int), pl->stream));
        mra_panel_chol(pl, T.dprob.p, (size_t)b.n_leaves, T.dn.p, T.derr.p);
    });
    if (const int e = stream_wait_err(pl, T.derr.p)) {
        char m[200];
        snprintf(m, sizeof m, "mra_sample_sites: leaf %d: the covariance of its sites' leaf terms is not positive definite (Cholesky pivot <= 0 or NaN; near-duplicate sites?)",
                 D.leaf_of_prob[(size_t)(e - 1)]);
        throw MraError(MRA_ERR_NOT_SPD, m);
    }
    for (int64_t s0 = 0; s0 < D.ns_all; s0 += 16) {
        const int ns = (int)std::min<int64_t>(16, D.ns_all - s0);
        SampleZ zs{nullptr, D.n_slots, (unsigned long long)D.seed, (long)(D.sample0 + s0), ns};
        if (D.z) { draw_stage_z(pl, D, b, s0, ns); zs.z = T.zcin.p; zs.ldz = Kn; }
        if (Kn) mra_sites_timed(pl, 5, [&] { mra_sample_draw(pl, zs, Kn, T.zc.p); });
        mra_sites_zeta(pl, b.nt, zs, Kn, D.z != nullptr);
        mra_sites_draw(pl, b.nt, D.post);
        mra_sites_timed(pl, 8, [&] { HIP_TRY(hipMemcpyAsync(D.oh.data(), T.dout.p, (size_t)ns * b.nt * 16 * sizeof(double), hipMemcpyDeviceToHost, pl->stream)); });
        stream_wait(pl);
        for (int s = 0; s < ns; ++s)
            for (long u = 0; u < b.nt * 16; ++u) {
                const int64_t i = D.slot[(size_t)(b.t0 * 16 + u)];
                if (i >= 0) D.out[(s0 + s) * D.n + i] = D.oh[(size_t)s * b.nt * 16 + u];
            }
    }
}

void mra_sample_sites_all(mra_plan* pl, uint32_t flags, int64_t n, const double* sites, const int32_t* leaf, int64_t ns_all, uint64_t seed,
                             int64_t sample0, const double* z, double* out) {
    sites_check_plan(pl, "mra_sample_sites", flags, MRA_COV_POSTERIOR, n);
    if (ns_all < 0) throw MraError(MRA_ERR_INVALID, "n_samples < 0");
    mra_check_sample0(sample0, ns_all);
    if (n > 0 && ns_all > 0 && !out) throw MraError(MRA_ERR_INVALID, "out is NULL");
    const std::vector<int> lslot = sites_check_sites(pl, "mra_sample_sites", n, sites, leaf);
    std::vector<double> msites;
    sites = sites_in_metric(pl, n, sites, msites);      // (the duplicate collapse compares what the kernels read)
    std::vector<int64_t> distinct;
    const std::vector<int64_t> first = collapse_duplicates(pl, lslot, n, sites, distinct);
    if (n == 0 || ns_all == 0) return;
    SiteDraw D{n, ns_all, sites, seed, sample0, z, out, (flags & MRA_COV_POSTERIOR) != 0};
    sites_ensure_state(pl);
    mra_plan::Solver& S = pl->slv;
    mra_plan::Sites& T = pl->sit;
    SitesSink sink(T, T.draw_ms, 9);
    // the tiles of the distinct sites; slot[] then holds the caller's index of each column
    const int64_t nd = (int64_t)distinct.size();
    {
        std::vector<int> ls((size_t)nd);
        for (int64_t k = 0; k < nd; ++k) ls[(size_t)k] = lslot[(size_t)distinct[(size_t)k]];
        sites_tiles(ls, nd, pl->leaf_nodes.size(), D.slot, D.tile_leaf);
        for (int64_t& v : D.slot) if (v >= 0) v = distinct[(size_t)v];
    }
    const long Kn = D.Kn = draw_chains(pl);
    D.n_slots = Kn + n;
    // batches of whole leaves: work arrays of the tiles + the leaf's block, its inverted diagonal blocks, its draws and results
    const size_t tile_bytes = mra_sites_tile_bytes(pl) + sizeof(SiteDrawTile) + 16 * (sizeof(long) + sizeof(int)) + 3 * 256 * sizeof(double);
    const LeafBatches B = leaf_batches(D.tile_leaf, tile_bytes, T.chunk_bytes ? T.chunk_bytes : SITES_CHUNK_BYTES, 1);
    mra_sites_draw_reserve(pl, B.cap_t, B.cap_g, B.cap_l);
    mra_reserve_coarse(T.zc, Kn);
    if (z) {
        mra_reserve_coarse(T.zcin, Kn);
        if (T.zin.n < (size_t)B.cap_t * 256) T.zin.alloc((size_t)B.cap_t * 256);
    }
    if (D.post) {
        // beta (leaves' gb) and q (leaves' uy) of the plan's own observations: the solver's sweeps without its row step, once per call
        stage_columns(pl, pl->y.p, 1, S.yb.p, hipMemcpyDeviceToDevice);
        mra_sites_timed(pl, 6, [&] { mra_solver_block(pl, true, false, false); });
    }
    D.xs.resize((size_t)B.cap_t * 16 * pl->d); D.oh.resize((size_t)B.cap_t * 256);
    D.zch.resize(z ? (size_t)std::max<long>(Kn, 1) * 16 : 0); D.zlh.resize(z ? (size_t)B.cap_t * 256 : 0);
    D.dt.resize((size_t)B.cap_t); D.pp.resize((size_t)B.cap_l); D.leaf_of_prob.resize((size_t)B.cap_l);
    for (const LeafBatch& b : B.bat) draw_batch(pl, D, b);
    if (nd < n)
        for (int64_t s = 0; s < ns_all; ++s)
            for (int64_t i = 0; i < n; ++i)
                if (first[(size_t)i] != i) out[s * n + i] = out[s * n + first[(size_t)i]];
}

// ---- cross-validation (mra_cv) -------------------------------------------------------------------------------------
// The sites are the plan's own observed rows, each in its own leaf: batches of whole leaves as mra_sample_sites_all, the four site kernels
// with the plan's y as the one column, then the leave-one-out step or, by leaf, N_G, its Cholesky factor and the solves.  The per-row
// results are scattered by padded row on the device and reduced there after the last batch, so nothing depends on the batches.
// The trend fit of mra_cv_trend, on the plan's own y and on factors that stand: the GLS step with the backward sweeps (the kriging means
// of [y | X] into trend.m), beta^ and L_A^-1 into trend.coef.  No predict pass: the variance mra_trend_fit(MRA_TREND_PREDICT) keeps is
// neither read nor touched, nor are that call's times (the sweeps' go into entry 9 of the call's own).
static void cv_trend_fit(mra_plan* pl) {
    mra_plan::Trend& T = pl->trend;
    trend_reserve(pl);
    double keep_ms[7], beta[MRA_TREND_MAX + 1];
    std::copy(T.ms, T.ms + 7, keep_ms);
    for (double& v : T.ms) v = 0.0;
    struct PutBack { double* to; const double* from; double* sum; ~PutBack() { *sum += to[0] + to[1] + to[2] + to[4]; std::copy(from, from + 7, to); } }
        put_back{T.ms, keep_ms, (pl->sit.ms_sink ? pl->sit.ms_sink : pl->sit.ms) + 9};
    TrendGls R;
    trend_gls(pl, "mra_cv_trend", true, beta, nullptr, R);
    trend_upload_coef(pl, R, true, 7);
    stream_wait(pl);       // (R's host arrays are read by the copies)
}

// trend (mra_cv_trend, section 22): the same call with the trend's GLS fit in front of the sweep of y, k_cv_trend behind the mean kernel
// and, when beta is estimated again without each leaf, k_cv_downdate in front of the Cholesky; info has 12 entries.
// What the batches of one call share: the export's name, its mode, the tiles (slot[] = the padded row of each column) and the host
// copies of one batch's descriptors
struct CvCall {
    const char* who; bool trend, by_leaf, refit;
    std::vector<int64_t> slot;
    std::vector<int> tile_leaf;
    std::vector<SiteDrawTile> dt; std::vector<PanelProb> pp; std::vector<CvGroup> gr;
};

// the observed rows, leaf by leaf in row order: site i is padded row rows[i] of leaf slot lslot[i].  Refuses a noise variance of 0.
static void cv_observed_rows(const mra_plan* pl, const char* who, std::vector<int64_t>& rows, std::vector<int>& lslot) {
    for (size_t t = 0; t < pl->leaf_nodes.size(); ++t)
        for (long p = pl->row0[pl->leaf_nodes[t]]; p < pl->row1[pl->leaf_nodes[t]]; ++p) {
            if (!pl->y_finite_host[p]) continue;
            if ((pl->noise_on ? pl->noise_host[(size_t)p] : pl->R) == 0.0) {
                char m[240];
                snprintf(m, sizeof m, "%s: the noise variance is 0 at observed padded row %ld (the leave-out distributions divide by it)", who, p);
                throw MraError(MRA_ERR_INVALID, m);
            }
            rows.push_back(p); lslot.push_back((int)t);
        }
}

// by leaf: a leaf's block is dense in its observed rows
static void cv_check_leaf_cap(const mra_plan* pl, const char* who, const std::vector<int>& lslot) {
    std::vector<int64_t> per_leaf(pl->leaf_nodes.size(), 0);
    for (const int t : lslot)
        if (++per_leaf[(size_t)t] == (int64_t)MRA_SAMPLE_SITES_LEAF_MAX + 1) {
            char m[240];
            snprintf(m, sizeof m, "%s: leaf %d has more than MRA_SAMPLE_SITES_LEAF_MAX = %d observed rows (its block is dense, 128 MiB at the cap)",
                     who, pl->leaf_nodes[(size_t)t], MRA_SAMPLE_SITES_LEAF_MAX);
            throw MraError(MRA_ERR_INVALID, m);
        }
}

// e = 1 + the batch's leaf (by leaf) or the padded row (by row) whose leave-out distribution does not exist
[[noreturn]] static void cv_not_spd(const CvCall& C, int e) {
    char m[240];
    if (C.by_leaf && C.refit)
        snprintf(m, sizeof m, "mra_cv_trend: leaf %d: D - Sigma_post - W W^T over its observed rows is not positive definite (Cholesky pivot <= 0 or NaN; "
                 "the leaf may carry the only information on a covariate; no jitter is added)", C.gr[(size_t)(e - 1)].node);
    else if (C.by_leaf)
        snprintf(m, sizeof m, "%s: leaf %d: D - Sigma_post over its observed rows is not positive definite (Cholesky pivot <= 0 or NaN; no jitter is added)",
                 C.who, C.gr[(size_t)(e - 1)].node);
    else if (C.refit)
        snprintf(m, sizeof m, "mra_cv_trend: padded row %d: 1 - (v + |w|^2) / r <= 0 or NaN (the row may carry the only information on a covariate; "
                 "no jitter is added)", e - 1);
    else
        snprintf(m, sizeof m, "%s: padded row %d: 1 - v / r <= 0 or NaN (the posterior variance reaches the noise variance; no jitter is added)", C.who, e - 1);
    throw MraError(MRA_ERR_NOT_SPD, m);
}

// One batch: its descriptors to the device, the four site kernels on the plan's y, the trend's rows, then the leave-one-out step or,
// by leaf, N_G, its downdate, its Cholesky factor and the solves
static void cv_batch(mra_plan* pl, CvCall& C, const LeafBatch& b) {
    mra_plan::Sites& T = pl->sit;
    leaf_batch_fill(pl, C.tile_leaf, b, C.dt, C.pp,
                    [&](long k, const SiteDrawTile& d, int node) { C.gr[(size_t)k] = CvGroup{d.goff, d.first, d.nt, node, 0}; });
    mra_sites_timed(pl, 7, [&] {
        HIP_TRY(hipMemcpyAsync(T.tleaf.p, C.tile_leaf.data() + b.t0, (size_t)b.nt * sizeof(int), hipMemcpyHostToDevice, pl->stream));
        HIP_TRY(hipMemcpyAsync(T.sslot.p, C.slot.data() + b.t0 * 16, (size_t)b.nt * 16 * sizeof(long), hipMemcpyHostToDevice, pl->stream));
        if (C.by_leaf) {
            HIP_TRY(hipMemcpyAsync(T.dtile.p, C.dt.data(), (size_t)b.nt * sizeof(SiteDrawTile), hipMemcpyHostToDevice, pl->stream));
            HIP_TRY(hipMemcpyAsync(T.dprob.p, C.pp.data(), (size_t)b.n_leaves * sizeof(PanelProb), hipMemcpyHostToDevice, pl->stream));
            HIP_TRY(hipMemcpyAsync(T.cvgroup.p, C.gr.data(), (size_t)b.n_leaves * sizeof(CvGroup), hipMemcpyHostToDevice, pl->stream));
        }
    });
    mra_cv_sites(pl, b.nt);
    mra_sites_basis(pl, b.nt);
    mra_sites_var(pl, b.nt);
    mra_sites_mean(pl, b.nt, 1, 3);
    if (C.trend) mra_cv_trend_rows(pl, b.nt, C.refit && !C.by_leaf);
    if (C.by_leaf) {
        mra_cv_gram(pl, b.nt, b.nt_max);
        if (C.refit) mra_cv_trend_downdate(pl, b.nt, b.nt_max);
        mra_sites_timed(pl, 5, [&] { mra_panel_chol(pl, T.dprob.p, (size_t)b.n_leaves, T.dn.p, T.derr.p); });
    } else mra_cv_loo(pl, b.nt);
    // (the host arrays of the uploads above are reused by the next batch: the copy of the error slot waits for them too)
    if (const int e = stream_wait_err(pl, T.derr.p)) cv_not_spd(C, e);
    if (C.by_leaf) mra_cv_solve(pl, b.nt, b.n_leaves);
}

// res: mra_cv_reduce's sums (MRA_CV_NRES), rt: mra_cv_trend_reduce's three
static void cv_info(const CvCall& C, const double* res, const double* rt, long n_groups, double* info) {
    info[0] = res[0];
    info[1] = C.by_leaf ? (double)n_groups : res[0];
    info[2] = C.by_leaf ? res[6] : res[1];      // every row its own group: the groups' joint densities are the rows' marginal ones
    info[3] = res[1]; info[4] = res[2]; info[5] = res[3]; info[6] = res[4]; info[7] = res[5];
    if (C.trend) {
        if (C.refit) info[5] = rt[2];
        info[6] = rt[0]; info[8] = rt[1];
        info[10] = info[6] - info[7]; info[11] = info[8] - info[7];
    }
}

void mra_cv_all(mra_plan* pl, bool trend, uint32_t flags, double* mean, double* var, double* lpd, double* group_lpd, double* info) {
    const char* who = trend ? "mra_cv_trend" : "mra_cv";
    char m[240];
    mra_retained_check_plan(pl, who, flags, trend ? (MRA_CV_LEAF | MRA_CV_TREND_REFIT) : MRA_CV_LEAF, "cannot cross-validate (C(s, s) is evaluated on the device)",
                        "cannot cross-validate", trend);
    if (trend && pl->trend.p == 0) throw MraError(MRA_ERR_STATE, "mra_cv_trend needs mra_plan_set_trend first");
    if (!info) { snprintf(m, sizeof m, "%s: info is NULL", who); throw MraError(MRA_ERR_INVALID, m); }
    if (pl->knots_pending) throw MraError(MRA_ERR_STATE, "knot rows not set");
    CvCall C{who, trend, (flags & MRA_CV_LEAF) != 0, trend && (flags & MRA_CV_TREND_REFIT) != 0};
    const long P = pl->P;
    std::vector<int64_t> rows;
    std::vector<int> lslot;
    cv_observed_rows(pl, who, rows, lslot);
    const int64_t n = (int64_t)rows.size();
    if (C.by_leaf) cv_check_leaf_cap(pl, who, lslot);
    if (g_dry) refuse_dry_run();      // (a dry-run plan reaches every refusal above; it cannot run)
    for (int k = 0; k < (trend ? 12 : 8); ++k) info[k] = 0.0;
    if (trend) info[9] = (double)pl->trend.p;
    for (double* o : {mean, var, lpd})
        if (o) std::fill(o, o + P, std::nan(""));
    if (group_lpd) std::fill(group_lpd, group_lpd + pl->n_nodes, std::nan(""));
    if (n == 0) return;
    sites_ensure_state(pl);
    mra_plan::Solver& S = pl->slv;
    mra_plan::Sites& T = pl->sit;
    SitesSink sink(T, trend ? T.cvt_ms : T.cv_ms, trend ? 12 : 9);
    if (trend) cv_trend_fit(pl);
    sites_tiles(lslot, n, pl->leaf_nodes.size(), C.slot, C.tile_leaf);
    for (int64_t& v : C.slot) if (v >= 0) v = rows[(size_t)v];
    // batches of whole leaves: work arrays of the tiles + (by leaf) the leaf's block twice, N_G and X
    const size_t tile_bytes = mra_sites_tile_bytes(pl) + sizeof(SiteDrawTile) + 16 * (sizeof(long) + sizeof(int)) + 3 * 256 * sizeof(double) +
                              (trend ? mra_cv_trend_tile_bytes(pl) : 0);
    const LeafBatches B = leaf_batches(C.tile_leaf, tile_bytes, T.chunk_bytes ? T.chunk_bytes : SITES_CHUNK_BYTES, C.by_leaf ? 2 : 0);
    mra_cv_reserve(pl, B.cap_t, B.cap_g, B.cap_l);
    if (trend) mra_cv_trend_reserve(pl, B.cap_t);
    HIP_TRY(hipMemsetAsync(T.derr.p, 0, sizeof(int), pl->stream));
    // beta (leaves' gb) and q (leaves' uy) of the plan's own observations: the solver's sweeps without its row step, once per call
    stage_columns(pl, pl->y.p, 1, S.yb.p, hipMemcpyDeviceToDevice);
    mra_sites_timed(pl, 3, [&] { mra_solver_block(pl, true, false, false); });
    C.dt.resize((size_t)B.cap_t); C.pp.resize((size_t)B.cap_l); C.gr.resize((size_t)B.cap_l);
    long n_groups = 0;
    for (const LeafBatch& b : B.bat) { cv_batch(pl, C, b); n_groups += b.n_leaves; }
    mra_cv_reduce(pl, C.by_leaf);
    if (trend) mra_cv_trend_reduce(pl, C.refit && !C.by_leaf);
    double res[MRA_CV_NRES], rt[3] = {0.0, 0.0, 0.0};
    const CvOut O = mra_cv_out(pl);
    mra_sites_timed(pl, 8, [&] {
        HIP_TRY(hipMemcpyAsync(res, T.cvres.p, sizeof res, hipMemcpyDeviceToHost, pl->stream));
        if (trend) HIP_TRY(hipMemcpyAsync(rt, T.cvtres.p, sizeof rt, hipMemcpyDeviceToHost, pl->stream));
        if (mean) HIP_TRY(hipMemcpyAsync(mean, O.mean, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, pl->stream));
        if (var) HIP_TRY(hipMemcpyAsync(var, O.var, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, pl->stream));
        if (lpd) HIP_TRY(hipMemcpyAsync(lpd, O.lpd, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, pl->stream));
        if (group_lpd) HIP_TRY(hipMemcpyAsync(group_lpd, T.cvgl.p, (size_t)pl->n_nodes * sizeof(double), hipMemcpyDeviceToHost, pl->stream));
    });
    stream_wait(pl);
    cv_info(C, res, rt, n_groups, info);
}

// ---- Laplace fit (mra_plan_fit_laplace) ---------------------------------------------------------------------
// Newton / IRLS for the mode of x given non-Gaussian data: every iteration is one likelihood + predict pass on the pseudo-observations
// t = x + g / D with noise r = 1 / D, which one launch writes into the plan's y / noise / noise_sd; the step and the sums of the
// result come from one reduction (two launches) after the pass.  Every argument is checked before anything changes.
static inline double lgamma_of(double v) { int sign; return lgamma_r(v, &sign); }      // (std::lgamma writes the global signgam: not for threads)
// The argument checks of mra_plan_fit_laplace and mra_plan_fit_laplace_trend (`who`; x0_name: what the start is called), in the
// header's order, before anything changes.  seen: the rows the plan observes.
static void laplace_check(const mra_plan* pl, const char* who, const char* x0_name, int family, const double* z, const double* aux,
                          const double* off, const double* x0, int max_iter, double tol, const double* info, std::vector<unsigned char>& seen) {
    char m[200];
    auto invalid = [&](const char* what, long p) {
        if (p >= 0) snprintf(m, sizeof m, "%s: %s (padded row %ld)", who, what, p); else snprintf(m, sizeof m, "%s: %s", who, what);
        throw MraError(MRA_ERR_INVALID, m);
    };
    if (!(pl->have_locs && pl->have_obs && pl->have_kernel)) { snprintf(m, sizeof m, "%s needs set_locs, set_obs and set_kernel first", who); throw MraError(MRA_ERR_STATE, m); }
    if (family != MRA_FAMILY_GAUSSIAN && family != MRA_FAMILY_POISSON && family != MRA_FAMILY_BINOMIAL) invalid("unknown family", -1);
    const long P = pl->P;
    const bool need_aux = family != MRA_FAMILY_POISSON;
    const bool readable = z && info && (aux || !need_aux);
    // observed: a finite y inside a leaf, as mra_plan_set_noise reads it (rows outside every leaf are nobody's)
    seen.assign((size_t)P, 0);
    for (size_t t = 0; t < pl->leaf_nodes.size(); ++t)
        for (long p = pl->row0[pl->leaf_nodes[t]]; p < pl->row1[pl->leaf_nodes[t]]; ++p) seen[p] = pl->y_finite_host[p];
    if (readable) {
        for (size_t t = 0; t < pl->leaf_nodes.size(); ++t)
            for (long p = pl->row0[pl->leaf_nodes[t]]; p < pl->row1[pl->leaf_nodes[t]]; ++p)
                if ((std::isfinite(z[p]) ? 1 : 0) != seen[p]) invalid("z is not finite exactly where the plan observes: the mask is that of the last mra_plan_set_obs", p);
        if (family != MRA_FAMILY_GAUSSIAN)
            for (long p = 0; p < P; ++p) if (seen[p] && z[p] < 0.0) invalid("z < 0 at an observed row (a count)", p);
        if (family == MRA_FAMILY_BINOMIAL)
            for (long p = 0; p < P; ++p) if (seen[p] && (aux[p] < z[p] || aux[p] <= 0.0)) invalid("binomial trials aux < z or aux <= 0 at an observed row", p);
        if (family == MRA_FAMILY_GAUSSIAN)
            for (long p = 0; p < P; ++p) if (seen[p] && aux[p] <= 0.0) invalid("Gaussian variance aux <= 0 at an observed row", p);
        char what[64];
        for (long p = 0; p < P; ++p) {
            if (!seen[p]) continue;
            if (need_aux && !std::isfinite(aux[p])) invalid("aux is not finite at an observed row", p);
            if (off && !std::isfinite(off[p])) invalid("offset is not finite at an observed row", p);
            if (x0 && !std::isfinite(x0[p])) { snprintf(what, sizeof what, "%s is not finite at an observed row", x0_name); invalid(what, p); }
        }
    }
    if (max_iter < 1) invalid("max_iter < 1", -1);
    if (!(tol > 0.0)) invalid("tol must be greater than 0", -1);
    if (!readable) invalid(!z || !info ? "z or info is NULL" : "aux is NULL (only the Poisson family reads none)", -1);
    // (mra_plan_fit_laplace's own last refusal; mra_plan_fit_laplace_trend never gets here with a sharded plan: mra_retained_check_plan refuses it first)
    if (pl->reduce_level >= 0 || pl->comm || pl->n_ranks > 1) invalid("sharded plans cannot iterate (the mean of a pass lives on its rank)", -1);
}

// The data of a fit by padded row (z: NaN where the plan does not observe) and its start into the plan's Laplace buffers; the noise
// vector goes on.  -> the constants of -2 log p that do not depend on x.
static double laplace_upload(mra_plan* pl, int family, const double* z, const double* aux, const double* off, const double* x0,
                             const std::vector<unsigned char>& seen) {
    const long P = pl->P;
    const bool need_aux = family != MRA_FAMILY_POISSON;
    // the data by padded row (z: NaN where the plan does not observe), the start, and the constants of -2 log p that do not depend on x
    std::vector<double> zh((size_t)P, std::nan("")), ah((size_t)P, 1.0), oh((size_t)P, 0.0), xh((size_t)P, 0.0);
    // (chunks of 65536 rows over a few host threads; a chunk's sum is compensated (Kahan) - a plain serial sum of 26 000 constants loses
    // 1e-13 of it, a hundred times what the device's tree of partial sums loses - and the chunks' sums are added in chunk order,
    // whatever the number of threads)
    const long CH = 65536, nch = (P + CH - 1) / CH;
    std::vector<double> kpart((size_t)nch, 0.0);
    parallel_rows(nch, [&](int64_t c0, int64_t c1) {
        for (int64_t c = c0; c < c1; ++c) {
            double k = 0.0, lost = 0.0;
            auto add = [&](double v) { const double y = v - lost, t = k + y; lost = (t - k) - y; k = t; };
            for (long p = c * CH; p < std::min<long>(P, (c + 1) * CH); ++p) {
                if (!seen[p]) continue;
                const double zp = z[p], a = need_aux ? aux[p] : 1.0, o = off ? off[p] : 0.0;
                zh[p] = zp; ah[p] = a; oh[p] = o;
                if (family == MRA_FAMILY_POISSON) {
                    add(2.0 * lgamma_of(zp + 1.0));
                    xh[p] = std::log(zp + 0.5) - o;
                } else if (family == MRA_FAMILY_BINOMIAL) {
                    add(-2.0 * (lgamma_of(a + 1.0) - lgamma_of(zp + 1.0) - lgamma_of(a - zp + 1.0)));
                    xh[p] = std::log((zp + 0.5) / (a - zp + 0.5)) - o;
                } else {
                    add(std::log(6.283185307179586 * a));
                    xh[p] = zp - o;
                }
                if (x0) xh[p] = x0[p];
            }
            kpart[(size_t)c] = k;
        }
    }, 1);
    double konst = 0.0;
    for (long c = 0; c < nch; ++c) konst += kpart[(size_t)c];
    HIP_TRY(mraSetDevice(pl->device));
    mra_laplace_reserve(pl);
    mra_plan::Laplace& L = pl->lap;
    const size_t bytes = (size_t)P * sizeof(double);
    HIP_TRY(mraMemcpy(L.z.p, zh.data(), bytes, hipMemcpyHostToDevice));
    HIP_TRY(mraMemcpy(L.aux.p, ah.data(), bytes, hipMemcpyHostToDevice));
    HIP_TRY(mraMemcpy(L.off.p, oh.data(), bytes, hipMemcpyHostToDevice));
    HIP_TRY(mraMemcpy(L.x.p, xh.data(), bytes, hipMemcpyHostToDevice));
    pl->slv.valid = false;
    if (!pl->noise_on) mra_set_leaf_diag_add(pl, 0.0);      // the noise vector goes on as in mra_plan_set_noise; every pass below rewrites it
    pl->noise_on = true;
    pl->noise_host.assign((size_t)P, 0.0);
    return konst;
}

// What the two fits share around their loops.  An iteration that has been waited for: the reduction's record into res; false ends the
// loop.  A step that is not finite (the reduction keeps a NaN or inf of the mean): the iterate has left the doubles.  The fit ends
// there, not converged, with that step in info[6].  (A guard: a pass whose t is NaN is as a rule refused before it has a mean - r = 0
// at an upper node's knot row has no positive pivot - DESIGN.md section 16.)
static bool laplace_goes_on(const mra_plan* pl, double tol, double* res, bool& converged) {
    std::copy(pl->host_res + MRA_HOST_RES_LAPLACE, pl->host_res + MRA_HOST_RES_LAPLACE + MRA_LAPLACE_NRES, res);
    if (!std::isfinite(res[0])) return false;
    converged = res[0] <= tol * std::max(1.0, res[1]);
    return !converged;
}
// the host mirror of the noise follows the device, whatever ends the loop (a pass that fails leaves its own r in the plan)
static hipError_t laplace_mirror_noise(mra_plan* pl) {
    return mraMemcpy(pl->noise_host.data(), pl->noise.p, (size_t)pl->P * sizeof(double), hipMemcpyDeviceToHost);
}
static void laplace_info(double* info, const double* res, double konst, int passes, bool converged) {
    info[2] = -2.0 * res[4] + konst;
    info[3] = res[2]; info[4] = res[3];
    info[5] = passes; info[6] = res[0]; info[7] = converged ? 1.0 : 0.0;
}

void mra_fit_laplace(mra_plan* pl, int family, const double* z, const double* aux, const double* off, const double* x0, int max_iter,
                        double tol, double* info) {
    std::vector<unsigned char> seen;
    laplace_check(pl, "mra_plan_fit_laplace", "x0", family, z, aux, off, x0, max_iter, tol, info, seen);
    if (g_dry) refuse_dry_run();
    const double konst = laplace_upload(pl, family, z, aux, off, x0, seen);
    mra_plan::Laplace& L = pl->lap;

    double res[MRA_LAPLACE_NRES] = {0, 0, 0, 0, 0};
    int passes = 0;
    bool converged = false;
    // the reduction rides behind every pass's last kernel (finish_run), so that an iteration synchronises once
    struct TailGuard { mra_plan* pl; ~TailGuard() { pl->pass_tail = nullptr; } } guard{pl};
    pl->pass_tail = [&] { KTimer kt(pl, KF_MISC, 0); mra_laplace_reduce(pl, family, pl->host_res_dev + MRA_HOST_RES_LAPLACE); };
    try {
        for (int it = 0; it < max_iter; ++it) {
            { KTimer kt(pl, KF_MISC, 0); mra_laplace_linearise(pl, family, it ? pl->mean.p : L.x.p); }
            mra_run_all(pl, MRA_RUN_LIKELIHOOD | MRA_RUN_PREDICT);
            ++passes;
            if (!laplace_goes_on(pl, tol, res, converged)) break;
        }
    } catch (...) { hipStreamSynchronize(pl->stream); laplace_mirror_noise(pl); throw; }
    HIP_TRY(laplace_mirror_noise(pl));
    info[0] = pl->res_d; info[1] = pl->res_u;
    laplace_info(info, res, konst, passes, converged);
}

// ---- Laplace fit with a regression trend (mra_plan_fit_laplace_trend) ------------------------------------------
// eta = X beta + x + offset with a flat prior on beta; the iteration runs on e = X beta + x at the observed rows (lap.x).  Every
// iteration: the linearisation at e (k_laplace_linearise, as mra_plan_fit_laplace), one likelihood pass for the factors of this r
// (ensure_factors), the GLS step of mra_trend_fit on [t | X] with the kriging means of the columns (trend_gls), and one reduction that
// forms e^ = m_t + (X - m_X)^T beta^, makes it the iterate and returns the step and the sums (k_laplace_trend_part, k_laplace_sum).
// No predict pass: nothing in the iteration reads a variance.  What the caller reads back from its own last mra_run stays.
void mra_fit_laplace_trend(mra_plan* pl, int family, const double* z, const double* aux, const double* off, const double* e0, int max_iter,
                              double tol, double* beta, double* cov_beta, double* info) {
    const char* who = "mra_plan_fit_laplace_trend";
    mra_retained_check_plan(pl, who, 0, 0, "cannot fit a trend (C(S, o) is evaluated on the device)", "cannot fit a trend", true);
    mra_plan::Trend& T = pl->trend;
    if (T.p == 0) throw MraError(MRA_ERR_STATE, "mra_plan_fit_laplace_trend needs mra_plan_set_trend first");
    std::vector<unsigned char> seen;
    laplace_check(pl, who, "e0", family, z, aux, off, e0, max_iter, tol, info, seen);
    if (!beta) throw MraError(MRA_ERR_INVALID, "mra_plan_fit_laplace_trend: beta is NULL");
    if (g_dry) refuse_dry_run();
    if (pl->knots_pending) throw MraError(MRA_ERR_STATE, "knot rows not set");
    const int p = T.p;
    // what can still be refused (the solver's buffers, (1 + p) P doubles for the means) before the plan changes, as in trend_fit
    HIP_TRY(mraSetDevice(pl->device));
    mra_solver_build(pl);
    trend_reserve(pl);
    mra_laplace_reserve(pl);
    const double konst = laplace_upload(pl, family, z, aux, off, e0, seen);
    mra_plan::Laplace& L = pl->lap;
    mra_plan::Solver& S = pl->slv;
    trend_ms_reset(pl);
    TrendMsSink sink(pl);                    // the upload of beta and the tail are timed into trend.ms as the sweeps are

    double res[MRA_LAPLACE_NRES] = {0, 0, 0, 0, 0};
    int passes = 0;
    bool converged = false;
    TrendGls R;
    // the kernel statistics describe the whole call: every pass opens with its own cleared (open_pass), so they are summed here.
    // harvest: the stream has been synchronised, so the events recorded since the last pass have their times
    mra_plan::KStat total[KF_COUNT];
    for (int k = 0; k < KF_COUNT; ++k) pl->kstat[k] = mra_plan::KStat();
    auto fold_stats = [&](bool harvest) {
        if (harvest) mra_harvest_kernel_events(pl);
        for (int k = 0; k < KF_COUNT; ++k) {
            const mra_plan::KStat& s = pl->kstat[k];
            total[k].launches += s.launches; total[k].ms += s.ms; total[k].flops += s.flops; total[k].flops_exec += s.flops_exec; total[k].bytes += s.bytes;
            pl->kstat[k] = mra_plan::KStat();
        }
    };
    auto publish_stats = [&] { fold_stats(true); for (int k = 0; k < KF_COUNT; ++k) pl->kstat[k] = total[k]; };
    try {
        for (int it = 0; it < max_iter; ++it) {
            { KTimer kt(pl, KF_MISC, 0); mra_laplace_linearise(pl, family, L.x.p); }
            fold_stats(false);               // (its event is harvested by the pass that follows)
            S.valid = false;                 // only the noise changed: the prior and its residual are reused as in any pass (options 24, 25)
            ensure_factors(pl);
            ++passes;
            trend_gls(pl, who, true, beta, cov_beta, R);
            trend_upload_coef(pl, R, false, 4);
            mra_sites_timed(pl, 3, [&] { KTimer kt(pl, KF_MISC, 0); mra_laplace_trend_reduce(pl, family, pl->host_res_dev + MRA_HOST_RES_LAPLACE); });
            stream_wait(pl);
            fold_stats(true);
            if (!laplace_goes_on(pl, tol, res, converged)) break;
        }
    } catch (...) { hipStreamSynchronize(pl->stream); publish_stats(); laplace_mirror_noise(pl); throw; }
    publish_stats();
    HIP_TRY(laplace_mirror_noise(pl));
    info[0] = S.pass_d; info[1] = R.resid;
    laplace_info(info, res, konst, passes, converged);
    info[8] = R.logdet;
    info[9] = info[0] + info[1] + info[2] + info[3] - info[4];
    info[10] = info[9] + info[8] - (double)p * std::log(6.283185307179586);
    info[11] = (double)observed_rows(pl);
}
