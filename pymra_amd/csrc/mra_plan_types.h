// mra_plan_types.h - the plan object and the small host helpers shared by the translation units of libmra_hip.so
// (mra_plan.hip: plan construction, launch sequence, C ABI; mra_launch_*.hip: the dispatchers of the heavily templated
// kernels, compiled separately so that the library builds in parallel).
#pragma once
#include "mra_kernels.h"
#include "../../include/mra_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <initializer_list>
#include <rccl/rccl.h>      // types and enum values only: the library itself is loaded with dlopen at run time
#include <set>
#include <string>
#include <thread>
#include <vector>
#include <time.h>

#define MRA_VERSION_STR "mra_hip 0.2 (gfx950)"

// ---- host dry run (test instrumentation, never a compute path) ------------------------------------------------------
// With MRA_HOST_DRYRUN=1 in the environment the plan is built entirely in host memory: every "device" buffer is a
// malloc, uploads are memcpy, no stream / event / kernel is ever created and mra_run refuses to run.  The point is
// to push the ~1500 lines of index arithmetic of plan construction (the steps of build_static and build_leaf, the host-cov block
// bookkeeping) and the native tree replay through AddressSanitizer / UBSan on a machine without a GPU
// (`make asan`, tests/test_asan_host.py).  Nothing is computed in this mode.
static const bool g_dry = []() { const char* e = getenv("MRA_HOST_DRYRUN"); return e && e[0] == '1'; }();
// Device allocations go through a small process-wide cache (mra_plan.hip): blocks of a destroyed plan are kept and handed to the
// next plan that asks for the same size on the same device.  The reference's MLE pattern builds a NEW MRATree per objective call
// (README.md:96-104): without the cache every call pays hipMalloc + hipFree of ~4 GB (~30 ms at 1024^2) around a 6 ms pass.
hipError_t mraMalloc(void** p, size_t n);
hipError_t mraFree(void* p);
static inline hipError_t mraMemcpy(void* d, const void* s_, size_t n, hipMemcpyKind k) { if (g_dry) { memcpy(d, s_, n); return hipSuccess; } return hipMemcpy(d, s_, n, k); }
static inline hipError_t mraMemset(void* d, int v, size_t n) { if (g_dry) { memset(d, v, n); return hipSuccess; } return hipMemset(d, v, n); }
static inline hipError_t mraMemcpy2D(void* d, size_t dp, const void* s_, size_t sp, size_t w, size_t h, hipMemcpyKind k) {
    if (g_dry) { for (size_t i = 0; i < h; ++i) memcpy((char*)d + i * dp, (const char*)s_ + i * sp, w); return hipSuccess; }
    return hipMemcpy2D(d, dp, s_, sp, w, h, k);
}
static inline hipError_t mraSetDevice(int dev) { return g_dry ? hipSuccess : hipSetDevice(dev); }

static thread_local std::string g_last_error;

// ---- the metric of mra_plan_set_metric ------------------------------------------------------------------
// t = A x for one row of coordinates, A d x d row-major: row i is A[i][0] x[0], then one fma per further column, in column order.
// The ONE arithmetic of the transform: the device kernel (k_metric_apply), the knot coordinates and the sites staged on the host all
// go through this function, and explicit fma leaves nothing to contraction: the same bits everywhere.  A = I returns x.
template <int DIM>
__host__ __device__ __forceinline__ void mra_metric_row(const double* __restrict__ A, const double* x, double* t) {
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
        double acc = A[i * DIM] * x[0];
#pragma unroll
        for (int k = 1; k < DIM; ++k) acc = __builtin_fma(A[i * DIM + k], x[k], acc);
        t[i] = acc;
    }
}
// the same for d known at run time (x and t must not overlap)
static inline void mra_metric_row_d(int d, const double* A, const double* x, double* t) {
    if (d == 1) mra_metric_row<1>(A, x, t); else if (d == 2) mra_metric_row<2>(A, x, t); else mra_metric_row<3>(A, x, t);
}

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) {                                                           \
            char _b[512];                                                                 \
            snprintf(_b, sizeof _b, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                     __FILE__, __LINE__);                                                 \
            throw MraError(MRA_ERR_HIP, _b);                                              \
        }                                                                                 \
    } while (0)

struct MraError {
    int code;
    std::string msg;
    MraError(int c, const std::string& m) : code(c), msg(m) {}
};
// the end of every dispatch chain over KernelParams::mode: a mode without an instance is an error, never another family's kernel
[[noreturn]] static inline void mra_bad_mode(const char* who, int mode) {
    throw MraError(MRA_ERR_STATE, std::string(who) + ": no kernel instance for covariance mode " + std::to_string(mode));
}

enum KFam {
    KF_PRIOR_RESID = 0, KF_PRIOR_CHOL, KF_PRIOR_TRSM, KF_LEAF_RESID, KF_LEAF_CHOL, KF_LEAF_SYRK,
    KF_LEAF_UPDATE, KF_FRONT_CHOL, KF_FRONT_SCHUR, KF_PRED_TRSM, KF_PRED_UPDATE, KF_MISC, KF_COUNT
};
// family names = the kernels that actually run (rocprofv3 kernel names), by path: [0] fused cascades on regular trees, [1] general
// level-by-level path; kfam_name_hi: KF_PRED_TRSM and KF_PRED_UPDATE of [1] with the two-kernel predictive cascade of deep 64-wide trees.
// tools/summarize_profiles.py maps the trace's kernel names onto the same strings.
static const char* kfam_name[2][KF_COUNT] = {
    {"k_gemm_nt_lds<COV> prior residual (unused on the fused path)",
     "k_knot_chain + k_prior_cascade<KNOT> knot pass (knot rows, kInv, Cholesky)",
     "k_prior_cascade row pass (W of all levels)",
     "k_leaf_gemm<COV> leaf residual V[S,o] and C",
     "k_chol_wave + k_trsm_rows2 leaf factor and solves (Lc, Ut, Tt)",
     "k_parent_front (children's Ut -> parent front -> Lt, Zt, Schur)",
     "k_gemm_nt_lds<SUB> / k_leaf_solve_update leaf update (separate launch)",
     "k_front (assembly + partial Cholesky + Schur per level)",
     "k_gemm_nt<SUB> front Schur complement (fronts too large for LDS)",
     "k_trsm_rows2 predict (unused on the fused path)",
     "k_predict_cascade (leaf update + all levels, mean/var)",
     "small kernels (k_assemble, k_leaf_cphantom, k_sum_dnode, ...)"},
    {"k_leaf_gemm<COV,SOLVE> prior of a level: residual + kernel + row solve (or k_gemm_nt_lds<COV> residual only)",
     "k_gemm_nt_lds<COV> knots' residual block + k_panel_chol prior kInv Cholesky per level",
     "k_trsm_rows2 prior W = R L^-T per level",
     "k_leaf_gemm<COV> leaf residual V[S,o] and C",
     "k_chol_wave + k_trsm_rows2 (or k_panel_chol) leaf factor and solves",
     "k_gemm_nt<SET> / k_parent_front leaf or parent SYRK",
     "k_gemm_nt_lds<SUB> leaf update W[S,anc] -= Tt^T Ut",
     "k_front / k_panel_chol front partial Cholesky",
     "k_gemm_nt<SUB> front Schur complement",
     "k_trsm_rows2 predict X = W Lt^-T per level",
     "k_gemm_nt_lds<SUB> predict update per level",
     "small kernels (k_assemble, k_gather_kinv, k_leaf_moments, k_sum_dnode, ...)"}};
static const char* kfam_name_hi[2] = {"k_predict_cascade (the four coarse levels of a deep tree)",
                                      "k_predict_hi (four deepest levels in registers + one sweep over the coarse columns)"};

// Work of a launch (or a family of launches): algorithmic flops with TRUE sizes (true ranks, true observation counts, a
// one-column y), the flops the MFMA tiles actually execute on the 16-padded layout, and the algorithmic HBM bytes of the
// launch (each operand array of the padded layout read or written once).  bench.py prices `alg` against the FP64 roof and
// `bytes` against the HBM roof; `exec` is reported as the executed-MFMA rate.
struct Work {
    double alg = 0, exec = 0, bytes = 0;
    Work() {}
    Work(double a) : alg(a), exec(a) {}
    Work(double a, double e, double b = 0) : alg(a), exec(e), bytes(b) {}
    Work& operator+=(const Work& o) { alg += o.alg; exec += o.exec; bytes += o.bytes; return *this; }
    Work operator+(const Work& o) const { Work w = *this; w += o; return w; }
    Work with_bytes(double b) const { Work w = *this; w.bytes = b; return w; }
};

// (MRA_TRACE_PLAN: number of descriptor uploads and the time spent in them)
struct UploadStats { long n = 0; double ms = 0; };
inline UploadStats& upload_stats() { static thread_local UploadStats s; return s; }

// Descriptor arena: a plan uploads ~170 small arrays (problem descriptors, index lists) while it is built - each one a device
// allocation and a synchronous pageable copy, ~20 us apiece, a third of the construction time of a 1024^2 tree.  Inside an
// ArenaScope the small ones (< 256 KB) are bump-allocated from ONE device block of the plan and staged in a pinned host mirror;
// the scope's end sends what was added in one copy.  Pointers are final at once (descriptors embed each other's addresses).
// A full arena simply falls back to the stand-alone path.
struct UploadArena {
    char* dev = nullptr;
    char* host = nullptr;           // pinned mirror (plain memory in a host dry run)
    size_t cap = 0, used = 0, flushed = 0;
    static constexpr size_t SMALL = 256 * 1024;
    void* take(size_t bytes, const void* src) {
        const size_t at = (used + 255) & ~(size_t)255;
        if (!dev || at + bytes > cap) return nullptr;
        memcpy(host + at, src, bytes);
        used = at + bytes;
        return dev + at;
    }
    void flush() {
        if (used > flushed) {
            if (mraMemcpy(dev + flushed, host + flushed, used - flushed, hipMemcpyHostToDevice) != hipSuccess) throw MraError(MRA_ERR_HIP, "hipMemcpy H2D failed (descriptor arena)");
            flushed = used;
        }
    }
};
inline UploadArena*& current_arena() { static thread_local UploadArena* a = nullptr; return a; }
struct ArenaScope {
    UploadArena* prev;
    UploadArena* mine;
    explicit ArenaScope(UploadArena* a) : prev(current_arena()), mine(a) { current_arena() = a; }
    void finish() { current_arena() = prev; if (mine) { UploadArena* a = mine; mine = nullptr; a->flush(); } }
    ~ArenaScope() { current_arena() = prev; if (mine) { try { mine->flush(); } catch (...) {} } }      // (error paths: the plan is torn down anyway)
};

template <class T>
struct DevVec {
    T* p = nullptr;
    size_t n = 0;
    bool in_arena = false;          // p points into the plan's descriptor arena: nothing to free
    void upload(const std::vector<T>& h) {
        static const bool trace = getenv("MRA_TRACE_PLAN") != nullptr;
        timespec t0{}, t1{};
        if (trace) clock_gettime(CLOCK_MONOTONIC, &t0);
        release();
        n = h.size();
        if (n) {
            UploadArena* a = current_arena();
            void* q = (a && n * sizeof(T) < UploadArena::SMALL) ? a->take(n * sizeof(T), h.data()) : nullptr;
            if (q) { p = (T*)q; in_arena = true; }
            else {
                if (mraMalloc((void**)&p, n * sizeof(T)) != hipSuccess) throw MraError(MRA_ERR_HIP, "hipMalloc failed (descriptor array)");
                if (mraMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) throw MraError(MRA_ERR_HIP, "hipMemcpy H2D failed");
            }
        }
        if (trace) { clock_gettime(CLOCK_MONOTONIC, &t1); upload_stats().n += 1; upload_stats().ms += (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6; }
    }
    // copy into the EXISTING allocation (descriptors already point into it)
    void fill(const std::vector<T>& h) {
        if (h.size() != n) throw MraError(MRA_ERR_STATE, "DevVec::fill: size changed");
        if (n && mraMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) throw MraError(MRA_ERR_HIP, "hipMemcpy H2D failed");
    }
    void alloc(size_t count) {
        release();
        n = count;
        if (n && mraMalloc((void**)&p, n * sizeof(T)) != hipSuccess) {
            char b[160];
            snprintf(b, sizeof b, "hipMalloc of %.3f GB failed", (double)(n * sizeof(T)) / 1e9);
            p = nullptr;
            throw MraError(MRA_ERR_HIP, b);
        }
    }
    void swap(DevVec& o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(in_arena, o.in_arena); }
    void release() {
        if (p && !in_arena) mraFree(p);
        p = nullptr;
        n = 0;
        in_arena = false;
    }
    ~DevVec() { release(); }
};

// ---- mra_solve: descriptors of the solve kernels (mra_solve_kernels.h, launched from mra_launch_solve.hip) ----
struct SolveLeaf {              // one leaf
    const double* Lc;           // nop x nop (ld nop): lower Cholesky factor of v_M(o, o) + R I, identity rows at phantom observations
    const double* Ut;           // anc (+ the y block, not read) x nop: Ut[a][k] = (L_c^-1 W[o, a0 + a])[k]
    const int* obs;             // nop padded rows of the observations (-1: padding)
    double* uy;                 // nop x16: U_y, then s, then q
    double* gb;                 // anc x16: g (forward), then beta (backward)
    const double* chain;        // anc x16: the parent's [alpha ; chain] (nullptr when anc == 0)
    long row0;
    int nrows, nop, anc, a0;    // a0: first ancestor column in W
};
struct SolveFront {             // one non-leaf node
    const double* F;            // Lt in rows [0, cw), Zt in rows [cw, cw + anc) (its y block below is not read); row stride ld
    double* buf;                // (cw + anc) x16: [z ; g] after the forward sweep, [alpha ; chain] after the backward sweep
    const double* chain;        // anc x16: the parent's buf (nullptr for the root)
    int ld, cw, anc;
    int kid0, nkid;             // children's g blocks ((cw + anc) x16 each) in the kid pointer list
};
struct SolveSeg { const double* p; int n; int sign; };      // rows of the quadratic form: sign * sum_rows v v^T

// ---- mra_cov_apply: descriptors of the covariance kernels (mra_cov_kernels.h, launched from mra_launch_cov.hip).
// The fronts go through SolveFront with buffers of the cov path's own (F is not read: nullptr).
struct CovLeaf {                // one leaf
    double* t;                  // anc x16: W[S, anc]^T (rep o A)[S], what the leaf hands up to its parent
    double* tp;                 // anc x16: W[S, anc]^T (knot o rep o A)[S]
    const double* chain;        // anc x16: the parent's [tau ; tau_chain] (nullptr when anc == 0)
    long row0;
    int nrows, anc, a0;         // a0: first ancestor column in W
};

// ---- mra_predict_sites: descriptors of the site kernels (mra_site_kernels.h, launched from mra_launch_sites.hip).
// The leaves go through the solver's SolveLeaf (Lc, Ut, obs; beta in gb and q in uy after the backward sweep).
struct SiteNode {               // one non-leaf node, as an ancestor of a site
    const double* Lp;           // cw x cw (ld cw): the prior factor L_j (identity rows at phantom knots)
    const double* F;            // Lt in rows [0, cw), Zt in rows [cw, cw + anc) (its y block below is not read); row stride ld
    const int* knots;           // cw padded rows of the node's knots (-1: phantom)
    int ld, cw, c0, anc;        // c0: first column of the node's own block in W; its ancestors' columns are [c0 + cw, c0 + cw + anc)
};

// ---- mra_sample_sites: descriptors of the draw kernels (mra_site_kernels.h)
struct SiteDrawTile {           // one tile of a batch of whole leaves
    long goff;                  // its leaf's block G_l in the batch's block buffer ((16 nt)^2 doubles, row stride 16 nt)
    int first, nt;              // the leaf's first tile in the batch and its tile count
};
struct SiteDrawChain { int row, zoff, width, pad; };      // one ancestor of a leaf: its first row in a / p, its first latent slot, its width

// ---- mra_cv: descriptors of the cross-validation kernels (mra_site_kernels.h).  The sites are the observed rows.
struct CvRows {                 // what the plan holds by padded row
    const double* y;            // the observations
    const double* noise;        // their noise variances (nullptr: the scalar R everywhere)
    double R;
};
struct CvOut {                  // results by padded row (P each), NaN where nothing is observed
    double *mean, *var, *lpd;   // mu_p, S_pp, log N(y_p; mu_p, S_pp)
    double *h, *rho;            // v_p / r_p and y_p - m_p: what the reduction reads
};
struct CvGroup {                // one leaf of a batch, as a group
    long goff;                  // its block N_G in the batch's block buffer (SiteDrawTile::goff of its tiles)
    int first, nt, node, pad;   // its first tile in the batch, its tile count, its node index
};
constexpr int MRA_CV_NRES = 7;  // rows, sum lpd, sum z^2, max h, tr K^-1, alpha^T alpha, sum of the groups' joint lpd

struct LevelData {
    std::vector<int> nodes;          // non-leaf nodes of this level
    int cw = 0, cwt = 0, c0 = 0, a0 = 0, nf = 0, na = 0;
    int ldf = 0;                     // row stride of a front in F: nf, or cw when only the panel columns [Lt ; Zt] are kept (panel_only)
    bool panel_only = false;
    long max_rows = 0;               // largest row range among the nodes
    DevVec<double> Lp, invP, F, invF;
    DevVec<GemmProb> gResid, gSchur, gUpdate;
    // one-launch prior of the level (k_leaf_gemm<COV, SOLVE>): the knots' residual block straight into Lp (both sides gathered through
    // the knot list), then residual + kernel + row solve on blocks of rows
    DevVec<GemmProb> gKnotResid, gResidFused;
    DevVec<GemmProb> gResidLik;               // ... over the gathered rows a likelihood needs (ensure_lik_general)
    double lik_share = 1.0;                   // their share of the level's rows
    bool prior_level_ok = false;
    Work fl_knot_resid;
    std::vector<GemmProb> hResid;
    DevVec<KinvProb> gKinv;
    DevVec<PanelProb> gPriorChol, gFrontChol;
    DevVec<TrsmNode> gTrsmPrior, gTrsmPost;
    DevVec<Trsm2Prob> gTrsm2Prior, gTrsm2Post;
    long max_tiles = 0;
    DevVec<int> tile_node;
    DevVec<long> tile_row0;
    long ntiles = 0;
    DevVec<AsmProb> gAsm;
    DevVec<FrontProb> gFront;
    int front_mode = 0;               // 0: separate launches, 1: k_front<PANEL>, 2: k_front<FULL> (whole front in LDS)
    size_t front_lds = 0;
    Work fl_resid, fl_pchol, fl_trsm, fl_fchol, fl_schur, fl_update;
    // the buffers' layout, per node slot s: the prior factor (cw x cw), the front (nf rows of stride ldf, [Lt ; Zt] in its first cw
    // columns), and the inverted 16 x 16 diagonal blocks of either factor (cwt of them)
    double* Lp_of(size_t s) const { return Lp.p + s * (size_t)cw * cw; }
    double* F_of(size_t s) const { return F.p + s * (size_t)nf * ldf; }
    double* invP_of(size_t s) const { return invP.p + s * (size_t)cwt * 256; }
    double* invF_of(size_t s) const { return invF.p + s * (size_t)cwt * 256; }
};

// ---- the route of a pass: WHICH launch sequence it runs, decided once by route_for (mra_plan.hip) from the tree's shape, the run
// flags, the options and the capability marks, stored in the plan when the pass opens and constant until it ends -----------------
constexpr int LEAF_MAX_TILES = 12;  // widest leaf observation block, in 16-row tiles, of k_chol_wave<LEAF_MAX_TILES> and the LDS row solve behind it
constexpr int TRSM2_MAX_NT = 12;    // widest block of launch_trsm2 (k_trsm_rows2<TRSM2_MAX_NT>); wider levels take k_trsm_rows
static_assert(LEAF_MAX_TILES <= TRSM2_MAX_NT, "the leaves' row solve goes through launch_trsm2 without a fall-back");
// a "small" leaf: at most this many observation tiles.  The tile count of the instances k_chol_tiles<8, 4>, k_trsm_rows2<8> and
// k_leaf_solve_update<8, 13, true> that take the small leaves; order_small_first (mra_plan.hip) puts them first in every ordered list
// and, with MRA_OPT_LEAF_ORDER, the leaves of most tiles first inside either part
constexpr int LEAF_SMALL_TILES = 8;
static_assert(LEAF_SMALL_TILES <= LEAF_MAX_TILES, "the small leaves are a subset of those the LDS row solve takes");
// (the integer values are the MRA_ROUTE_* numbers of include/mra_hip.h: mra_get_route reports them)
enum class PassPath { Fused = MRA_ROUTE_PATH_FUSED, Hi = MRA_ROUTE_PATH_HI, Levels = MRA_ROUTE_PATH_LEVELS };      // one-kernel cascades of a regular tree / level-by-level with k_predict_hi (deep 64-wide trees) / level-by-level
// no observations / the gathered COV product wrote all of C / k_leaf_cphantom / k_leaf_fill
enum class LeafCFix { None = MRA_ROUTE_CFIX_NONE, InProduct = MRA_ROUTE_CFIX_IN_PRODUCT, Phantom = MRA_ROUTE_CFIX_PHANTOM, Fill = MRA_ROUTE_CFIX_FILL };
// k_chol_tiles<10,4> / <8,4> + <10,4> / k_chol_wave / right-looking panels + trailing GEMM
enum class LeafChol { TilesOne = MRA_ROUTE_CHOL_TILES_ONE, TilesSplit = MRA_ROUTE_CHOL_TILES_SPLIT, Wave = MRA_ROUTE_CHOL_WAVE, BigPanels = MRA_ROUTE_CHOL_BIG_PANELS };
enum class LeafVar { None = MRA_ROUTE_VAR_NONE, FinishVar = MRA_ROUTE_VAR_FINISH_VAR, Moments = MRA_ROUTE_VAR_MOMENTS };            // variance of a predict pass: the cascade's own / k_leaf_finish_var / k_leaf_moments
// W[S,anc] -= Tt^T Ut: no predict / in k_predict_cascade (larger leaves: GEMM) / in k_predict_hi / k_leaf_solve_update, one or two workgroups per leaf / k_gemm_nt_lds<SUB> / k_leaf_gemm<SUB>
enum class LeafUpdate { None = MRA_ROUTE_UPDATE_NONE, InCascade = MRA_ROUTE_UPDATE_IN_CASCADE, InPredictHi = MRA_ROUTE_UPDATE_IN_PREDICT_HI, SolveWhole = MRA_ROUTE_UPDATE_SOLVE_WHOLE,
                        SolveHalves = MRA_ROUTE_UPDATE_SOLVE_HALVES, Gemm = MRA_ROUTE_UPDATE_GEMM, LeafGemm = MRA_ROUTE_UPDATE_LEAF_GEMM };
struct PassRoute {
    PassPath path = PassPath::Levels;
    bool predict = false, init_yblock = false, acc_var = false;     // k_init_yblock runs (every path but Fused); the row solves accumulate the variance on the way
    int n_chain = 0;                            // Fused: levels of the k_knot_chain launch (0: one knot launch per level)
    bool prior_level = false;                   // level-by-level prior: one launch per level where lv.prior_level_ok
    bool c_only = false, lik_rows = false, lik_general = false;     // likelihood-only: C from a gathered product; W at the needed rows only (Fused / not)
    bool scatter_ut = false;                    // Fused: the row cascade scatters the leaves' Ut rows (MRA_OPT_UT_GATHER off)
    bool leaf_resident = false;                 // leaf residual on k_leaf_gemm
    LeafCFix c_fix = LeafCFix::None; LeafChol chol = LeafChol::Wave; LeafVar var = LeafVar::None; LeafUpdate update = LeafUpdate::None;
    bool solve_fused = false;                   // Fused + predict: the small leaves solve their Ut rows only, k_leaf_solve_update does the rest
    const Trsm2Prob *trsm_small = nullptr, *trsm_all = nullptr;     // row-solve lists: leaves [0, n_trsm_small) (Fused only) and the others (same index)
    // the leaves' parents' fronts straight from the children's Ut; by k_parent_front in one launch; k_front where the level's front_mode allows it
    bool direct_parent = false, parent_front = false, front_fused = false;
    bool syrk_blk = false, syrk_dma = false;    // the grandparents' signed SYRK on k_syrk_blk (its DMA-staged form)
    bool side = false;                          // predict-only leaf work forked to the side stream (sharded runs, never with kernel timing)
    bool extract_mean = false;                  // k_extract_mean after the level-by-level predictive pass
};

struct mra_plan {
    int device = 0;
    UploadArena arena;                   // the small descriptor arrays of this plan (device block + pinned mirror, see UploadArena)
    hipStream_t stream = nullptr;        // the pass; carries the chain of small dependent launches and the all-reduce (high priority)
    hipStream_t stream2 = nullptr;       // side stream: the leaf update runs here, beside the front chain / all-reduce (low priority)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool side_pending = false;           // work on stream2 that the predictive pass has to wait for
    // MRA_OPT_LEAF_ORDER (1, the default: the fork and the order; 0: neither; 2, 3, 4 for A/B runs: the fork alone, the order alone, 1 with
    // the residual product in that order as well)
    bool use_leaf_fork = true;           // read by open_pass: leaf_fork below
    bool leaf_longest_first = true;      // read by build_leaf: order_small_first sorts each of its two parts by decreasing tile count
    bool resid_longest_first = false;    // read by build_leaf: the residual product's problems in that order too (else leaf order)
    bool leaf_fork = false;              // this pass: the leaves of more than LEAF_SMALL_TILES tiles factorise, solve and update on stream2 beside the small ones
    hipEvent_t ev_leaf_fork = nullptr, ev_leaf_join = nullptr;      // the events of that fork (SideFork)
    std::string err;
    // topology (host)
    long P = 0;
    int d = 0, n_levels = 0, n_nodes = 0;
    std::vector<long> level_ptr, row0, row1, knot_ptr, knot_rows;
    bool knots_pending = false;         // mra_plan_create_replay_2d: built beside the knot draws; knot_rows (and the leaves' knot_ptr) arrive later (plan_set_knots)
    std::vector<uint8_t> leaf;
    std::vector<int> parent, child_ptr, child_list, cw, node_level;
    // layout
    int Ka = 0, ldw = 0;
    std::vector<int> coff, asuf, nf, na;
    // state
    bool have_locs = false, have_obs = false, have_kernel = false, ran = false, split_pending = false;
    uint32_t run_flags = 0;
    KernelParams kp{};
    bool host_cov = false;
    DevVec<double> nu_tab;              // MRA_KERNEL_MATERN: the quadrature table kp.nu_tab points at, built for nu_tab_nu (host memory on
    double nu_tab_nu = 0.0;             // MRA_HOST_DRYRUN plans); set_kernel rebuilds it when nu changes and at no other time
    // MRA_KERNEL_LOCAL reads a range out of the last coordinate column: what set_locs remembers of that column (the smallest value, NaN if
    // any is not finite), so that whichever of set_locs and set_kernel comes second can refuse a range that is not positive and finite
    double last_col_min = 0.0;
    DevVec<double> sum_tab;             // MRA_KERNEL_SUM: MRA_SUM_MAX records of MRA_SUM_REC doubles, kp.nu_tab of such plans; every set_kernel(7) fills it
    double R = 0.0;
    // the metric of mra_plan_set_metric: while metric_on the kernels' X (and the knot coordinates of the fused levels) hold A x and
    // Xraw the caller's coordinates; knot_raw[m] = the untransformed knot coordinates of fused level m as set_knot_coords lays them
    // out (phantom knots included), so that a new A needs no host locations.  Nothing of this is allocated before the first metric.
    bool metric_on = false;
    double metric_A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    DevVec<double> Xraw;
    std::vector<std::vector<double>> knot_raw;
    // per-observation noise variances (mra_plan_set_noise): while noise_on the leaves' C = v_M(o,o) + diag(r_o) - the leaf descriptors
    // carry diag_add = 0 and run_leaf_noise adds r on the diagonal; noise_sd = sqrt(r) for the pseudo-data of conditional draws.
    // By padded row, 0 at rows the plan does not observe.  Dropped by the next mra_plan_set_obs (pl->R holds again).
    bool noise_on = false;
    DevVec<double> noise, noise_sd;
    std::vector<double> noise_host;
    int reduce_level = -1;
    // device data
    DevVec<double> X, y, W, var, mean, dnode, scal, covsrc, covdiag, stamps, pstamps, tstamps, kstamps, kstamps2;
    double* host_res = nullptr;      // pinned, device-mapped {d, u, below, err} record of the last pass; from MRA_HOST_RES_LAPLACE on the reduction of mra_plan_fit_laplace
    double* host_res_dev = nullptr;  // the same memory as the device sees it
    DevVec<int> errflag, knot_idx, row_leaf;
    DevVec<long> knots_dev;
    std::vector<long> knot_idx_off;      // per node offset into knot_idx (padded to cw)
    std::vector<LevelData> lev;
    std::vector<int> node_slot;          // index of a non-leaf node inside its level's arrays
    // leaves
    std::vector<int> leaf_nodes;         // node numbers
    std::vector<int> leaf_slot;          // node -> leaf index or -1
    std::vector<int> leaf_nop;
    std::vector<long> leaf_poff, leaf_goff, leaf_ioff;
    DevVec<double> panel, leafInv, Gt;
    DevVec<int> obs_idx, obs_pos, leaf_nobs, leaf_nop_dev, ft_leaf;
    DevVec<double*> leaf_ut;
    DevVec<LeafProb> gLeaf;
    DevVec<GemmProb> gLeafResid, gLeafSyrk, gLeafUpdate, gLeafResidLik;
    DevVec<GemmProb> gLeafResidSorted, gLeafResidLikSorted;      // resid_longest_first: those of the device kernels once more, in the order of order_small_first (else empty); gLeafResid stays leaf-indexed (MRA_KERNEL_HOST points its problems at the host blocks by leaf)
    std::vector<GemmProb> hLeafResid, hLeafResidLik;      // host copies: MRA_KERNEL_HOST and mra_plan_set_noise patch them and send them again
    std::vector<size_t> leaf_order;                       // order_small_first, the order of the *Sorted lists
    std::vector<int> leaf_nobs_host;
    DevVec<PanelProb> gLeafCholFull, gLeafCholLik, gLeafCholC, gLeafCholSorted;
    // leaves with more than 192 observations: right-looking blocked factorisation, 64 columns per step (one panel launch +
    // one trailing-update GEMM per step); [variant 0 full / 1 likelihood-only][step] -> descriptors of all leaves
    std::vector<DevVec<PanelProb>> gBigPanel[2];
    std::vector<DevVec<GemmProb>> gBigTrail[2];
    std::vector<long> bigM[2], bigN[2];
    DevVec<Trsm2Prob> gLeafTrsmFull, gLeafTrsmLik, gLeafTrsmFullPlain, gLeafTrsmLikPlain, gLeafTrsmFullPlainG, gLeafTrsmLikPlainG;
    DevVec<LeafSolveProb> gLeafSolve;     // k_leaf_solve_update, same order as the *Plain arrays (order_small_first)
    DevVec<LeafSolveProb> gLeafSolveHalf; // the small leaves again, two workgroups each (row tiles split in two): shorter workgroups on the
    size_t n_leaf_solve_half = 0;         // side stream free their CUs sooner for the high-priority front chain (MRA_OPT_LEAF_SOLVE_SPLIT)
    int leaf_solve_split = 2;             // measured on an eighth of C3: 1.086 -> 1.066 ms
    DevVec<GemmProb> gLeafUpdatePlain;    // the leaf update in that order (for the leaves the fused kernel does not take)
    bool use_leaf_solve = true, leaf_solve_ok = false;
    int use_chol_lds = 1;                     // leaf Cholesky with one workgroup per matrix (k_chol_tiles): 1 when a CU sees at most two leaves, 2 always, 0 never
    size_t n_chol_small = 0;
    bool ut_gather = true;                    // fused path: the leaves' Ut rows gathered from W by the row solve (no scatter in the row cascade: 1.21 -> 1.03 ms there, +0.16 ms in the solve)
    bool cphantom_valid = false;              // the phantom observation rows of the leaves' C blocks hold their identity rows
    // What the last pass left of its PRIOR for the next one (MRA_OPT_PRIOR_REUSE; DESIGN.md section 4, "the prior of the last pass").  The
    // prior depends on the locations, the knots and the kernel - not on y, the noise or (where W was written at every row) the mask.
    // Read by prior_step_for, written where the launches are enqueued, reset by prior_keep_reset (mra_plan.hip) - the one invalidation.
    struct PriorKeep {
        enum class Rows { None, Observed, All };      // Observed: at the rows of the mask of the last build_leaf (a lik_rows pass)
        enum class Dirty { Clean, Oversized, All };   // leaves whose rows of W a later stage of the last pass overwrote (Oversized: those of
                                                      // more than LEAF_SMALL_TILES observation tiles - the plain update beside InCascade)
        bool knots_valid = false;                     // Lp / invP / Wk of every level belong to the current kernel and locations
        Rows rows = Rows::None;                       // W's level columns hold the prior basis at these rows
        bool var_valid = false;                       // var_prior holds the prior variance of every row
        Dirty dirty = Dirty::Clean;
    } keep;
    // What the last pass left of the leaves' RESIDUAL (MRA_OPT_RESID_REUSE): V0 = V[S,o] = kernel(x_S, x_o) - W_S W_o^T
    // and C0 = v(o,o) + 0 depend on what the prior depends on and on the mask - not on y, R or a noise vector.  A pass on an eligible
    // route (resid_step_for) writes them into `resid` instead of the panel; k_chol_tiles, k_trsm_rows2 and k_leaf_solve_update read them
    // there and store L, Tt and W where they always did, so the next pass launches no residual product.  Reset with `keep`
    // (prior_keep_reset) and by a mra_plan_set_obs whose observed-row list differs from the standing one.
    struct ResidKeep {
        enum class Form { None, COnly, Full };        // COnly: C0 from the gathered k_gemm_nt_lds product; Full: C0 and V0 from k_leaf_gemm.
                                                      // The two sum in different orders: a pass never takes the other form's C0
        Form resid = Form::None;
        bool phantom = false;                         // C0's phantom observation rows hold their identity rows
    } rkeep;
    bool use_resid_reuse = true;              // MRA_OPT_RESID_REUSE
    // [per leaf: C0 (nop x nop) ; V0 (N_j x nop)], row stride nop, leaves in leaf order: allocated by the first eligible pass (a refused
    // allocation: resid_refused, no pass keeps until the next mra_plan_set_obs), and the descriptor lists that point into it - the
    // plan's own lists with C / C2 / src / V redirected and diag_add 0, rebuilt after every build_leaf (resid_lists)
    DevVec<double> resid;
    std::vector<long> leaf_koff;              // [leaf + 1] offsets into resid
    bool resid_lists = false, resid_refused = false;
    std::vector<int> obs_list_host;           // obs_idx as build_leaf uploaded it: the mask `rkeep` belongs to
    std::vector<PanelProb> hLeafCholSorted;   // host copies of the lists the kept ones are made from (build_leaf)
    std::vector<Trsm2Prob> hLeafTrsmFullPlainG;
    std::vector<LeafSolveProb> hLeafSolve, hLeafSolveHalf;
    std::vector<size_t> hLeafSolveHalfPos;    // a half's position in hLeafSolve
    std::vector<LeafProb> hLeaf;
    DevVec<GemmProb> kLeafResid, kLeafResidLik;       // in the order run_leaf_product launches (sorted when the plan's are)
    DevVec<PanelProb> kLeafCholSorted;
    DevVec<Trsm2Prob> kLeafTrsmFullPlainG;
    DevVec<LeafSolveProb> kLeafSolve, kLeafSolveHalf;
    DevVec<LeafProb> kLeaf;
    bool use_prior_reuse = true;              // MRA_OPT_PRIOR_REUSE
    DevVec<double> var_prior;                 // [P] the prior variance the row cascade wrote (allocated by the first pass that keeps it)
    // the row cascade's workgroups over the oversized leaves' tiles (build_leaf): first tile and tile count, one leaf per workgroup run,
    // tile numbers as in ft_row0.  big: of the current mask - the leaves the next plain update dirties; stale: of the mask under which
    // the standing keep.dirty == Oversized was set, where a set_obs has come between (n_wg 0: none, the current list is the one)
    struct LeafTileWgs {
        DevVec<long> wg0;
        DevVec<int> wgn;
        long n_wg = 0, n_tiles = 0;
        void swap(LeafTileWgs& o) { wg0.swap(o.wg0); wgn.swap(o.wgn); std::swap(n_wg, o.n_wg); std::swap(n_tiles, o.n_tiles); }
    } big, stale;
    int use_hi_fold = 1;                      // deep 64-wide trees: the leaf update W -= Tt Ut^T inside k_predict_hi instead of a pass over all of W (option 16)
    bool use_prior_level = true;              // levels of the level-by-level prior with blocks <= 64 wide: residual + kernel + row solve in one launch (option 15)
    bool parent_panel_lds_ok = false;         // every parent-panel problem fits the step table of the LDS-tiled segmented product
    bool grand_syrk_dma_ok = false;           // ... and the smaller one of its DMA-staged form
    bool grand_syrk_blk_ok = false;           // every grandparent problem fits k_syrk_blk's step table
    int use_syrk_blk = 1;                     // the grandparents' signed SYRK on 96 x 96 blocks through LDS (k_syrk_blk) instead of 32 x 32 wave tiles (option 14)
    bool seg_gemm_lds = true;                 // the parents' panel product (segmented: sum over the children's Ut blocks) on the LDS-tiled GEMM (6.3 -> 5.4 ms at config 5)
    bool use_pred_update = true;              // leaf update folded into the predictive cascade
    DevVec<long> leaf_row0_dev;
    DevVec<unsigned char> leaf_upd_dev;
    size_t leaf_solve_lds = 0;
    int leaf_solve_mode = 2;              // MRA_OPT_LEAF_SOLVE: 0 off, 1 always, 2 (default) when the leaves are few per CU
    size_t n_trsm_small = 0;            // = n_chol_small: the small leaves, first in the *Plain arrays and in gLeafCholSorted (order_small_first)
    int trsm_small_nt = 0, trsm_small_tiles_full = 0, trsm_small_tiles_lik = 0;
    DevVec<GemmProb> gParentSyrk;        // fused path: fronts of the leaves' parents straight from the children's Ut
    DevVec<GemmSeg> parentSegs;
    DevVec<FrontProb> gParentFront;      // the same nodes for k_parent_front (SYRK + factorisation in one launch)
    int parent_front_nacc = 0;           // 0: not available (front too large for the register-resident SYRK)
    size_t parent_front_lds = 0;
    int parent_pair_nacc = 0;            // k_parent_front_pair<17|23> can take these fronts (parent_pair_ok); 0: it cannot
    size_t parent_pair_lds = 0;
    double parent_pair_idle_exec = 0;    // flops its empty accumulator slots execute in a pass (they repeat tile (0, 0))
    int use_parent_pair = 1;             // MRA_OPT_PARENT_PAIR, read at launch: 0 never, 1 where a CU gets more than one front, 2 wherever it can
    bool parent_syrk = false;
    // Large fronts at the level of the leaves' parents (config 5: 528^2 per node, 36 GB in all) are never formed: F = I + U U^T with
    // U = the children's Ut blocks side by side has rank <= sum(n_obs), so only its panel columns [F_oo ; F_ao] = U U_o^T (+ I) are
    // built and factorised ([Lt ; Zt]), and the grandparents' fronts come straight from the leaves and the panels:
    //     F_grand = I + sum_leaves Ut[anc] Ut[anc]^T - sum_parents Zt Zt^T        (Schur complement = F_aa - Zt Zt^T, MRANode.py:476-480)
    // one signed, segmented SYRK instead of SYRK + Schur update + assembly of 528^2 blocks (95 GB of HBM traffic -> 37 GB).
    bool lowrank_parent = false;
    DevVec<GemmProb> gParentPanel, gGrandSyrk;
    DevVec<GemmSeg> grandSegs, parentSegsAo;
    DevVec<FrontProb> gParentOwn;         // k_parent_front on the own (cw x cw) block alone: F_oo = I + U_o U_o^T -> Lt, inverted diagonal blocks, log det
    DevVec<Trsm2Prob> gParentZt;          // Zt = F_ao Lt^-T, row solve of the panel's lower part in place
    size_t parent_own_lds = 0;
    Work fl_parent_panel, fl_grand_syrk;
    bool shape_regular = false;          // every leaf sits on the last level (all other levels hold non-leaf nodes only)
    std::vector<AsmChild> hKids;         // host copies: the leaves' Gt blocks are allocated only when something needs them
    std::vector<int> kid_leaf;
    std::vector<GemmProb> hLeafSyrk;
    int leaf_max_tiles_full = 0, leaf_max_tiles_lik = 0;
    DevVec<AsmChild> asmKids;
    long leaf_max_rows = 0;
    int leaf_max_nop = 0, leaf_max_na = 0, leaf_max_ht = 0;
    Work fl_leaf_resid, fl_leaf_chol, fl_leaf_chol_lik, fl_leaf_syrk, fl_leaf_update, fl_leaf_c_only;
    double by_leaf_ut = 0, by_leaf_tt = 0, by_leaf_c = 0;     // bytes of all leaves' Ut / Tt (= V) / C blocks
    std::vector<long> anc_rank;          // per node: sum of the TRUE ranks of its ancestors
    // fused ("regular tree") path
    // deep trees with 64-wide blocks (5 - 8 non-leaf levels of four tiles: BASELINE config 5): too many tiles per row for the one-kernel
    // cascades; the predictive pass runs as k_predict_hi (four deepest levels) + k_predict_cascade (coarse levels)
    bool regular_hi = false;
    DevVec<long> hi_wg0_8;
    DevVec<int> hi_wgleaf;                    // [k_predict_hi workgroup] leaf slot of its tiles
    DevVec<int> hi_wgn_8;
    long n_hi_wg8 = 0;
    bool regular = false, use_fused = true, gemm_lds = true, use_front_fused = true, use_leaf_gemm = true, leaf_gemm_update = false;
    PassRoute route;                    // the launch sequence of the open pass: fixed by mra_run_all, read by every stage and by mra_run_resume
    bool route_set = false;             // a pass has fixed `route` (mra_get_route)
    int dbg = 0;
    int NL = 0, CWT = 0;
    struct FusedLevel {
        DevVec<double> kx, Wk;
        DevVec<int> kvalid, kt_rows, kt_chain, kt_knot0, kt_wgn;
        DevVec<GemmProb> gKinv;
        DevVec<long> kt_wg0;
        long n_ktiles = 0, n_kwg = 0;
        int k_threads = 256;        // workgroup size of the level's knot launch (512 when sibling families share a workgroup)
    };
    std::vector<FusedLevel> fl;
    DevVec<long> ft_row0, ft_wg0, ft_wg0_x;
    DevVec<int> ft_chain, ft_wgn, ft_wgn_x, ft_wgleaf_x;
    long n_ftiles = 0, n_fwg = 0, n_fwg_x = 0;
    size_t cascade_lds = 0, cascade_lds_all = 0;
    bool cascade_stage_all = false;   // all levels' operands fit in LDS: one workgroup per leaf, staged once
    bool cascade_group_siblings = false;
    int n_cu = 256;
    // knot pass of all levels in one launch (k_knot_chain)
    bool use_knot_chain = true, knot_chain_ok = false;
    int kc_levels = 0;                    // levels 0 .. kc_levels-1 go through the chain kernel
    size_t knot_chain_lds = 0;
    DevVec<int> kc_chain;                 // [bottom slot][8]
    std::vector<int> kc_chain_host;
    DevVec<int> kc_ownmask;               // [bottom slot] bit m: the workgroup writes its level-m ancestor's results
    DevVec<double> kc_knots;              // [bottom slot][level][cw * (d + 1)] packed knots of the chain (mra_plan_set_locs)
    int cascade_wpw = 4;          // row tiles (= waves) per workgroup of the per-level cascade kernels (4 or 8; 4 measured faster)
    // likelihood-only passes: the row cascade walks gathered tiles of the leaves' OBSERVED rows only (obs_idx is the gather list);
    // per-tile chain / leaf and the workgroup list are built when such a pass first runs (ensure_lik_tiles)
    DevVec<int> lik_chain, lik_leaf, lik_wgn;
    DevVec<long> lik_wg0;
    long n_lik_wg = 0, n_lik_tiles = 0;
    bool lik_tiles_valid = false;
    // level-by-level path: the rows a likelihood needs = observed rows and knots, per leaf (padded to 16 with -1), leaves concatenated
    DevVec<int> need_idx;
    std::vector<unsigned char> y_finite_host; // [P] 1 where the row is observed (set_obs)
    bool lik_general_valid = false, lik_general_ok = false;
    bool use_lik_rows = true;                 // option 17
    std::vector<long> obs_off_host;           // [leaf + 1] offset of the leaf's list in obs_idx (multiples of 16)
    DevVec<long> ft_wg0_leaf;
    DevVec<int> ft_wgn_leaf;
    long n_fwg_leaf = 0;
    // host cov staging (MRA_KERNEL_HOST)
    std::vector<long> cov_off;           // per node offset into covsrc
    std::vector<double> cov_host, covdiag_host;
    // results
    double res_d = 0, res_u = 0;
    // timers
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double phase_ms[5] = {0, 0, 0, 0, 0};
    bool ktiming = false;
    struct KStat { int launches = 0; double ms = 0, flops = 0, flops_exec = 0, bytes = 0; } kstat[KF_COUNT];
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> kev;
    // The row maps of the calls on the retained factors ("What the calls on the retained factors share").  They
    // follow from the topology and the knot rows alone: built once per plan, by the first call that reads them (mra_row_maps), and
    // reset by no set_* and no option.
    struct RowMaps {
        bool built = false;
        std::vector<unsigned char> rep_host, knot_host;      // [P] reported row (a leaf's row that is a knot of some node); knot row of its own leaf
        DevVec<unsigned char> rep, knot;          // the same two on the device
        DevVec<int> tile_leaf;                    // [P / 16] leaf of a row tile (-1: none)
    } maps;
    // sampler (mra_sample): chains built and device buffers allocated on the first call, so that a plan that never samples keeps
    // its footprint.  Leaves go through their Gram / factor stage in batches of bounded size (batch b = leaves [bat[b], bat[b+1])).
    // The row maps are the plan's (maps).
    struct Sampler {
        bool built = false;
        long n_coarse = 0;                        // latent slots of the non-leaf nodes
        std::vector<long> zoff;                   // per node: its first latent slot (-1: leaf)
        DevVec<int> chain_ptr;                    // [n_leaves + 1] into chain
        DevVec<SampleChain> chain;                // a leaf's ancestors of non-zero width, leaf to root
        DevVec<SampleLeaf> leaves;                // every leaf, G pointing into the batch buffer
        DevVec<GemmProb> gram;
        DevVec<PanelProb> chol;
        std::vector<size_t> bat;
        std::vector<long> bat_rows;               // largest leaf of a batch
        DevVec<double> G, invd, zc, out, zh, ysave, msave, vsave, dn;
        DevVec<int> err;
        int factored = -1;                        // batch whose factors G holds (-1: none)
        bool use_solve = false;                   // this call conditions its draws through mra_solve's sweeps (MRA_OPT_SAMPLE_SOLVE)
        size_t gram_bytes = 0;                    // MRA_OPT_SAMPLE_GRAM_BYTES (0: SAMPLE_GRAM_BUDGET); a change rebuilds the batches
    } smp;
    // solver (mra_solve): the factors of a likelihood pass with W at every row, kept for any number of right-hand sides.  Descriptors
    // and work buffers are built on the first call (and again after new observations: the leaves' panels move); the node buffers are
    // laid out by mra_node_layout, the row maps are the plan's (maps).
    struct Solver {
        bool built = false;
        bool valid = false;                       // "factors valid, W complete": set by mra_solve's own pass, cleared by mra_run,
                                                  // mra_run_resume, mra_sample and every set_*
        int in_sampler = 0;                       // MRA_OPT_SAMPLE_SOLVE
        DevVec<SolveLeaf> leaves;
        DevVec<SolveFront> fronts;                // by level, then slot
        std::vector<size_t> lev_off, lev_lds;     // [level]: first front of the level in `fronts`; dynamic LDS of its launches
        DevVec<const double*> kids;
        DevVec<SolveSeg> segs;
        DevVec<double> yb, out, uy, nb, qpart, quad, msave, vsave;      // 16 x P in / out blocks; U_y / s / q; node buffers; Q
        size_t work_bytes = 0;
        double pass_d = 0.0;                      // log-determinant of the pass that set `valid` (it does not depend on y)
        // MRA_SOLVE_FULL_QUAD (and mra_trend_fit): the forward vectors of every 16-column block of a call, one panel of arch_rows x16
        // per block (segment k of segs at row seg_off[k]), the partial sums of one group of block pairs and the dense matrix.  Allocated
        // by flagged calls only (grow-only in the number of blocks); released when the descriptors are rebuilt.
        long arch_rows = 0;
        int arch_blocks = 0;                      // panels the archive holds
        DevVec<long> seg_off;
        DevVec<double> arch, cpart, qfull;        // qfull: (16 blocks) x (16 blocks) doubles, row stride 16 * arch_blocks
    } slv;
    // regression trend (mra_plan_set_trend / mra_trend_fit): the design matrix by padded row, resident on the
    // device; a property of the plan like the noise vector (no set_* drops it, it enters no factorisation).  The rest is allocated by
    // the first predicting fit: the kriging means of [y | X], the variance of a predict pass on the plan's y (var_valid: it belongs to
    // the factors that stand - cleared whenever ensure_factors runs a pass), beta and L^-1 for k_trend_rows, its results.
    struct Trend {
        int p = 0;
        DevVec<double> X;                         // p x P
        DevVec<double> m, var_pass, coef, mean, var;      // (1 + p) x P; P; 64 (beta) + 64 x 64 (L^-1); P; P
        bool var_valid = false;
        // stream ms of the last mra_trend_fit with MRA_OPT_KERNEL_TIMING: staging, sweeps, cross quad, rows, transfers; then what the
        // sweeps of one block move: bytes of the leaves' Ut (read once by the forward sweep, twice more by the backward one) and of
        // the block's archive panel (written once, read once)
        double ms[7] = {0, 0, 0, 0, 0, 0, 0};
    } trend;
    // covariance operator (mra_cov_apply): reads W of the pass mra_solve keeps (slv.valid), the plan's row maps (maps), the solver's
    // level offsets and, for the posterior, its sweeps.  Its node buffers are its own, laid out by mra_node_layout as the solver's are.
    // Built on the first call and again whenever the solver's descriptors are.
    struct Cov {
        bool built = false;
        DevVec<CovLeaf> leaves;
        DevVec<SolveFront> fronts;                // by level, then slot (the solver's lev_off)
        DevVec<const double*> kids;
        DevVec<double> ab, out, nb, gpart, gram;  // 16 x P in / out blocks; node buffers; gram partial sums; 16 x 16
        size_t work_bytes = 0;
    } cov;
    // prediction at new sites (mra_predict_sites): reads W, the prior factors and the fronts of the pass mra_solve keeps (slv.valid), the
    // solver's leaf descriptors and, for the mean, its sweeps.  Descriptors are built on the first call and again whenever the solver's
    // are; the work buffers hold one chunk of site tiles (MRA_OPT_SITES_CHUNK_BYTES) and grow on demand.
    struct Sites {
        bool built = false;
        DevVec<SiteNode> nodes;                   // [n_nodes] (leaves: unused)
        DevVec<int> chain, chain_ptr;             // a leaf's ancestors, root first: chain[chain_ptr[t] .. chain_ptr[t + 1])
        int anc_max = 0, nop_max = 0;             // widest ancestor chain / observation block among the leaves
        size_t chunk_bytes = 0;                   // MRA_OPT_SITES_CHUNK_BYTES (0: SITES_CHUNK_BYTES)
        long cap_tiles = 0;                       // tiles the work buffers hold
        DevVec<int> tleaf;                        // [tile] leaf slot
        DevVec<double> xs, a, b, t, var, mean;    // [tile]: 16 x d sites; a, b (anc_max x16); t (nop_max x16); 16 variances; 16 x 16 means
        double ms[7] = {0, 0, 0, 0, 0, 0, 0};     // stream ms of the last call with MRA_OPT_KERNEL_TIMING: basis, leaf, chain, mean, the solver's sweeps, uploads, downloads
        // mra_sites_cov: every tile's a, b, t stay in the buffers above for the call; one row panel of the result
        DevVec<double> gram;                      // rows of whole tiles x the padded site count
        double cov_ms[6] = {0, 0, 0, 0, 0, 0};    // stream ms of the last mra_sites_cov: basis, leaf, chain, gram, uploads, downloads
        double* ms_sink = nullptr;                // where mra_sites_timed adds (nullptr: ms); mra_sites_cov points it at cov_ms for its call
        // mra_sample_sites: one batch of whole leaves at a time - their tiles' a, b, t in the buffers above, their
        // blocks G_l (factorised in place), and one block of 16 samples
        DevVec<SiteDrawTile> dtile;               // [tile of the batch]
        DevVec<SiteDrawChain> dchain;             // a leaf's ancestors, root first: dchain[dchain_ptr[t] .. dchain_ptr[t + 1])
        DevVec<int> dchain_ptr, live, derr;       // [n_leaves + 1]; [tile][16] 1: the site has a leaf term (not padding, not inert); Cholesky error slot
        DevVec<long> sslot;                       // [tile][16] the caller's index of the site (-1: padding)
        DevVec<PanelProb> dprob;                  // [leaf of the batch]
        DevVec<double> G, invd, dn;               // the batch's blocks; their inverted diagonal blocks; log-determinants (not read)
        DevVec<double> zc, zcin, zl, zin, dout;   // Kn x16 non-leaf draws (and the caller's, 16 x Kn); [tile][16] x16 leaf draws (and the caller's); 16 x [tile][16] results
        double draw_ms[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // stream ms of the last mra_sample_sites: basis, leaf, chain, leaf Gram, leaf Cholesky, draw, mean (+ sweeps), uploads, downloads
        // mra_cv: the sites are the observed rows, a batch of whole leaves at a time over the buffers above (sslot:
        // padded rows; G: the groups' N_G, factorised in place; zl: w = L^-1 rho) - and the results by padded row for the call
        DevVec<CvGroup> cvgroup;                  // [leaf of the batch]
        DevVec<double> cvx;                       // the batch's X = L^-1 column tiles, laid out as G
        DevVec<double> cvrow, cvgl, cvpart, cvres;      // 5 x P: mean, var, lpd, h, rho; [n_nodes] group values; the reduction's partial and final results
        DevVec<int> cvleaf;                       // [n_leaves] node index
        DevVec<long> cvleaf_row;                  // [n_leaves][2] first and one-past-last padded row
        double cv_ms[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};        // stream ms of the last mra_cv: basis, leaf, chain, mean (+ sweeps), Gram, Cholesky, solve (+ reduction), uploads, downloads
        // mra_cv_trend: per tile of a batch W^T = L_A^-1 h^T (qn x16, qn = p rounded up to 4), |w|^2 by padded
        // row for the call, and the trend's share of the reduction
        DevVec<double> cvw, cvwsq, cvtpart, cvtres;
        double cvt_ms[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // stream ms of the last mra_cv_trend: cv_ms's nine, then the trend's sweeps, k_cv_trend, k_cv_downdate
    } sit;
    // Laplace fit (mra_plan_fit_laplace): the data of the call by padded row (z: NaN at rows the plan does not
    // observe), the linearisation point of the running pass, and the reduction's partial results.  Allocated by the first call.
    struct Laplace {
        DevVec<double> z, aux, off, x, part;
    } lap;
    // comm
    void* rccl = nullptr;
    ncclComm_t comm = nullptr;
    ncclResult_t (*allreduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    int n_ranks = 1, rank = 0;
    std::function<void()> pass_tail;     // launches behind the last kernel of a pass, before its one synchronisation (set by mra_plan_fit_laplace for its call)
    bool pass_open = false;              // a pass was started and has not reached finish_run (error or abandoned split)
    // kernels whose dynamic-LDS limit was raised for THIS plan's device (the attribute is per device, a plan lives on one)
    std::set<const void*> big_lds_done;
    bool prepare_only = false;           // mra_plan_prepare: the launch helpers set their attributes and return
};

// The panel of leaf t, row stride nop = leaf_nop[t]: [C ; Ut ; V] = the observation block (nop rows; factorised in place: Lc), the
// ancestor columns and the y block (na rows), one row per row of the leaf (V, then Tt).  Sized in build_leaf (leaf_poff).
static inline double* leaf_C(const mra_plan* pl, size_t t) { return pl->panel.p + pl->leaf_poff[t]; }
static inline double* leaf_Ut(const mra_plan* pl, size_t t) { const size_t nop = pl->leaf_nop[t]; return leaf_C(pl, t) + nop * nop; }
static inline double* leaf_V(const mra_plan* pl, size_t t) {
    const size_t nop = pl->leaf_nop[t], na = pl->na[pl->node_level[pl->leaf_nodes[t]]];
    return leaf_C(pl, t) + (nop + na) * nop;
}

// The non-leaf ancestors of a node, root first (levels of zero width included: the caller skips them where its chain has no use for them)
static inline std::vector<int> leaf_ancestors(const mra_plan* pl, int node) {
    std::vector<int> up;
    for (int p = pl->parent[node]; p >= 0; p = pl->parent[p]) up.push_back(p);
    std::reverse(up.begin(), up.end());
    return up;
}

// Dynamic LDS above 64 KiB has to be requested per kernel and per DEVICE.  The record is kept per plan (a plan lives on one
// device; mra_plan_prepare reports its size) AND per (device, kernel) for the process, so that the second plan of a process - the
// reference's MLE pattern builds a new MRATree per objective call - does not pay ~20 us per kernel again in its first pass.
bool mra_big_lds_once(int device, const void* fn);      // mra_plan.hip: true the first time this (device, kernel) pair is seen
static inline void ensure_big_lds(mra_plan* pl, std::initializer_list<const void*> fns) {
    for (const void* f : fns) {
        if (pl->big_lds_done.count(f)) continue;
        if (!g_dry && mra_big_lds_once(pl->device, f)) hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        pl->big_lds_done.insert(f);
    }
}

// ---- small things every host unit uses ------------------------------------------------------------------------------
// a plan built in host memory (g_dry) has nothing to run on: the one refusal of a pass and of every call that would launch
[[noreturn]] static inline void refuse_dry_run() { throw MraError(MRA_ERR_STATE, "MRA_HOST_DRYRUN plan: built in host memory for the sanitizers, it cannot run"); }
// everything queued on the plan's stream has run, and none of it failed ... and the device's error slot as they left it (0, or 1 + what failed)
static inline void stream_wait(mra_plan* pl) { HIP_TRY(hipStreamSynchronize(pl->stream)); HIP_TRY(hipGetLastError()); }
static inline int stream_wait_err(mra_plan* pl, const int* err) {
    int e = 0;
    HIP_TRY(hipMemcpyAsync(&e, err, sizeof(int), hipMemcpyDeviceToHost, pl->stream));
    stream_wait(pl);
    return e;
}
// a few host threads over a range of rows (or of leaves: min_per_thread is the smallest share worth a thread)
template <class F>
static void parallel_rows(int64_t n, F fn, int64_t min_per_thread = 65536) {
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(4, std::thread::hardware_concurrency()), n / min_per_thread));
    if (T <= 1) { fn(0, n); return; }
    std::vector<std::thread> pool;
    for (int t = 0; t < T; ++t) pool.emplace_back(fn, n * t / T, n * (t + 1) / T);
    for (auto& th : pool) th.join();
}
// one launch in the plan's kernel statistics: its work now, its time (with kernel timing on) between two events on pl->stream
struct KTimer {
    mra_plan* pl; int fam; hipEvent_t a = nullptr, b = nullptr;
    KTimer(mra_plan* p, int f, const Work& w) : pl(p), fam(f) {
        pl->kstat[fam].launches += 1;
        pl->kstat[fam].flops += w.alg;
        pl->kstat[fam].flops_exec += w.exec;
        pl->kstat[fam].bytes += w.bytes;
        if (pl->ktiming) {
            hipEventCreate(&a); hipEventCreate(&b);
            hipEventRecord(a, pl->stream);
        }
    }
    ~KTimer() {
        if (pl->ktiming) {
            hipEventRecord(b, pl->stream);
            pl->kev.push_back({fam, {a, b}});
        }
    }
};

// ---- dispatchers defined in the mra_launch_*.hip translation units ----------------------------------------------------
// batched C (=|-=) f(A B^T) with epilogue EPI_SET / EPI_SUB / EPI_COV / EPI_HOSTCOV; lower_tri: every problem has .lower set and M == N
// mra_launch_nu3.hip: MRA_KERNEL_MATERN (covariance mode 4) on 3-D coordinates - the launches the dispatch chains of the other units
// hand their <3, 4> case to, with the grids they computed
void mra_nu3_gemm(mra_plan* pl, bool lds, dim3 grid, const GemmProb* probs, unsigned gxs, unsigned gy, unsigned S);
void mra_nu3_leaf_gemm(mra_plan* pl, bool wide, dim3 grid, const GemmProb* probs);
void mra_nu3_prior_level(mra_plan* pl, dim3 grid, const GemmProb* probs);
void mra_nu3_solve_rows(mra_plan* pl);
void mra_nu3_cov_rows(mra_plan* pl);
void launch_basis_nu3(mra_plan* pl, long n);
void launch_leaf_nu3(mra_plan* pl, long n);
void launch_mean_nu3(mra_plan* pl, long n, int nc);
void launch_gram_nu3(mra_plan* pl, long n, long tile0, long rows, bool post);
void launch_leaf_gram_nu3(mra_plan* pl, long n, int nt_max, bool post);
void launch_cv_gram_nu3(mra_plan* pl, long n, int nt_max);
// mra_launch_sum.hip / mra_launch_sum2.hip: MRA_KERNEL_SUM (covariance mode 5) in every dimension - the launches the dispatch chains hand
// their mode-5 case to; each picks the instance of pl->d
void mra_sum_gemm(mra_plan* pl, bool lds, dim3 grid, const GemmProb* probs, unsigned gxs, unsigned gy, unsigned S);
void mra_sum_leaf_gemm(mra_plan* pl, bool wide, dim3 grid, const GemmProb* probs);
void mra_sum_prior_level(mra_plan* pl, dim3 grid, const GemmProb* probs);
void mra_sum_solve_rows(mra_plan* pl);
void mra_sum_cov_rows(mra_plan* pl);
void launch_basis_sum(mra_plan* pl, long n);
void launch_leaf_sum(mra_plan* pl, long n);
void launch_mean_sum(mra_plan* pl, long n, int nc);
void launch_gram_sum(mra_plan* pl, long n, long tile0, long rows, bool post);
void launch_leaf_gram_sum(mra_plan* pl, long n, int nt_max, bool post);
void launch_cv_gram_sum(mra_plan* pl, long n, int nt_max);
// mra_launch_loc.hip / mra_launch_loc2.hip: MRA_KERNEL_LOCAL (covariance mode 6, local ranges in the last coordinate column), d = 2 and 3 -
// the launches the dispatch chains hand their mode-6 case to
void mra_loc_gemm(mra_plan* pl, bool lds, dim3 grid, const GemmProb* probs, unsigned gxs, unsigned gy, unsigned S);
void mra_loc_leaf_gemm(mra_plan* pl, bool wide, dim3 grid, const GemmProb* probs);
void mra_loc_prior_level(mra_plan* pl, dim3 grid, const GemmProb* probs);
void mra_loc_solve_rows(mra_plan* pl);
void mra_loc_cov_rows(mra_plan* pl);
void launch_basis_loc(mra_plan* pl, long n);
void launch_leaf_loc(mra_plan* pl, long n);
void launch_mean_loc(mra_plan* pl, long n, int nc);
void launch_gram_loc(mra_plan* pl, long n, long tile0, long rows, bool post);
void launch_leaf_gram_loc(mra_plan* pl, long n, int nt_max, bool post);
void launch_cv_gram_loc(mra_plan* pl, long n, int nt_max);
void mra_launch_gemm(mra_plan* pl, int epi, const GemmProb* probs, size_t nprob, long maxM, long maxN, bool allow_lds = true, bool lower_tri = false);
void mra_launch_leaf_gemm(mra_plan* pl, int epi, const GemmProb* probs, size_t nprob);
void mra_launch_syrk_blk(mra_plan* pl, const GemmProb* probs, size_t nprob, long M, bool dma);
void mra_launch_prior_level(mra_plan* pl, const GemmProb* probs, size_t nprob);
void launch_cascade_d1(mra_plan* pl, const CascadeArgs& ar);       // one translation unit per spatial dimension
void launch_cascade_d2(mra_plan* pl, const CascadeArgs& ar);
void launch_cascade_d3(mra_plan* pl, const CascadeArgs& ar);
void launch_knot_chain_d1(mra_plan* pl, const KnotChainArgs& ka);
void launch_knot_chain_d2(mra_plan* pl, const KnotChainArgs& ka);
void launch_knot_chain_d3(mra_plan* pl, const KnotChainArgs& ka);
static inline void launch_cascade_any(mra_plan* pl, const CascadeArgs& ar) { if (pl->d == 1) launch_cascade_d1(pl, ar); else if (pl->d == 2) launch_cascade_d2(pl, ar); else launch_cascade_d3(pl, ar); }
static inline void launch_knot_chain(mra_plan* pl, const KnotChainArgs& ka) { if (pl->d == 1) launch_knot_chain_d1(pl, ka); else if (pl->d == 2) launch_knot_chain_d2(pl, ka); else launch_knot_chain_d3(pl, ka); }
void launch_predict_any(mra_plan* pl, const PredArgs& ar, size_t lds);
void launch_predict_hi(mra_plan* pl, const PredHiArgs& hi, const PredArgs& low, size_t lds_low, bool upd);
// mra_plan.hip: the plan's row maps (mra_plan::RowMaps), built on the first call; holds the one "knot row out of range" check
const mra_plan::RowMaps& mra_row_maps(mra_plan* pl);
// mra_launch_solve.hip: the node buffers of a sweep over the tree and the fronts that point into them.  A leaf's buffer holds leaf_blocks
// blocks of anc x16, a front's (cw + anc) x16; nb is allocated here, fronts (by level, then slot) and kids are uploaded.  with_F: the
// fronts read their factor (F_of / ldf; the solver), else nullptr / 0 (the covariance path).
struct NodeLayout {
    std::vector<long> noff;                   // [n_nodes + 1] a node's first double in nb
    std::vector<int> anc;                     // [n_nodes] ancestor columns
    std::vector<size_t> lev_off;              // [n_levels + 1] first front of a level
    std::vector<SolveFront> fronts;           // the host copy of what was uploaded
};
NodeLayout mra_node_layout(mra_plan* pl, int leaf_blocks, bool with_F, DevVec<double>& nb, DevVec<SolveFront>& fronts, DevVec<const double*>& kids);
// mra_launch_solve.hip: descriptors + work buffers of mra_solve; one block of <= 16 columns (slv.yb -> slv.out, slv.quad; launches
// only, on pl->stream); the 16-column glue of the sampler's MRA_OPT_SAMPLE_SOLVE path
void mra_solver_build(mra_plan* pl);
// archive >= 0: the block's forward vectors are copied into that panel of the archive behind the forward sweep (after mra_solver_archive)
void mra_solver_block(mra_plan* pl, bool want_mean, bool want_quad, bool want_rows = true, int archive = -1);      // want_rows false: stop before step 6 (beta and q stay in the leaves' gb / uy)
// MRA_SOLVE_FULL_QUAD: room for n_blocks panels; the tiles between the n_blocks archived blocks into slv.qfull (row stride
// 16 * slv.arch_blocks; tiles on the diagonal are not written), launches only
constexpr int MRA_FULL_QUAD_BLOCKS = 16;
void mra_solver_archive(mra_plan* pl, int n_blocks);
void mra_solver_quad_cross(mra_plan* pl, int n_blocks);
// mra_trend_fit: trend.mean / trend.var from trend.m, trend.X, trend.coef and trend.var_pass (k_trend_rows), launch only
void mra_trend_rows(mra_plan* pl);
void mra_solver_pseudo(mra_plan* pl, const double* y, const double* x, const SampleZ& zs, long slot0);
void mra_solver_addmean(mra_plan* pl, double* x, int ns);
// mra_launch_cov.hip: descriptors + work buffers of mra_cov_apply; one block of <= 16 columns (cov.ab -> cov.out, cov.gram; launches
// only, on pl->stream; the posterior goes through slv.yb, mra_solver_block and slv.out)
void mra_cov_build(mra_plan* pl);
void mra_cov_block(mra_plan* pl, bool posterior, bool want_gram);
// mra_launch_sites.hip: descriptors + work buffers of mra_predict_sites; the kernels of one chunk of n_tiles site tiles (sit.xs, sit.tleaf
// -> sit.var, sit.mean; launches only, on pl->stream).  mra_sites_tile_bytes: work memory of one tile.
constexpr size_t SITES_CHUNK_BYTES = (size_t)256 << 20;
void mra_sites_build(mra_plan* pl);
size_t mra_sites_tile_bytes(const mra_plan* pl);
void mra_sites_reserve(mra_plan* pl, long n_tiles);
void mra_sites_basis(mra_plan* pl, long n_tiles);
void mra_sites_var(mra_plan* pl, long n_tiles);
void mra_sites_mean(mra_plan* pl, long n_tiles, int n_cols, int which = 3);      // which: the timing entry of the launch
// mra_sites_cov: one row panel of the joint covariance of the n_tiles resident tiles - tile rows [tile0, tile0 + n_rows) against every
// tile at or after them, into sit.gram with row stride n_tiles * 16 (blocks before the diagonal are not written: the caller mirrors)
void mra_sites_gram(mra_plan* pl, long n_tiles, long tile0, long n_rows, bool posterior);
// mra_sample_sites: the kernels of one batch of whole leaves whose n_tiles tiles are resident (sit.dtile, sit.sslot uploaded).
// mra_sites_leaf_gram: sit.live and the leaves' blocks G_l into sit.G (nt_max: tiles of the batch's largest leaf); mra_sites_zeta: the
// leaf draws of one block of samples into sit.zl (from sit.zin when from_caller, else Philox at slot n_coarse + the caller's index);
// mra_sites_draw: coarse term (sit.zc) + leaf term (sit.G factorised, sit.zl) [+ sit.mean] -> sit.dout, 16 x (n_tiles * 16)
void mra_sites_draw_reserve(mra_plan* pl, long n_tiles, size_t g_doubles, long n_leaves);
void mra_sites_leaf_gram(mra_plan* pl, long n_tiles, int nt_max, bool posterior);
void mra_sites_zeta(mra_plan* pl, long n_tiles, const SampleZ& zs, long n_coarse, bool from_caller);
void mra_sites_draw(mra_plan* pl, long n_tiles, bool posterior);
// ... and of mra_cv (section 18): the call's row results (NaN everywhere) and the batch buffers; the sites of a batch out of the plan's
// rows; the elementwise leave-one-out step; N_G of a batch's leaves; w, the groups' values and the per-row results; the reduction into
// res[MRA_CV_NRES] on the device (leaf mode: group_lpd is summed as it stands; otherwise the leaves' sums of lpd are formed first)
void mra_cv_reserve(mra_plan* pl, long n_tiles, size_t g_doubles, long n_leaves);
CvRows mra_cv_rows(const mra_plan* pl);
CvOut mra_cv_out(const mra_plan* pl);
void mra_cv_sites(mra_plan* pl, long n_tiles);
void mra_cv_loo(mra_plan* pl, long n_tiles);
void mra_cv_gram(mra_plan* pl, long n_tiles, int nt_max);
void mra_cv_solve(mra_plan* pl, long n_tiles, long n_groups);
void mra_cv_reduce(mra_plan* pl, bool by_leaf);
// ... and of mra_cv_trend (section 22) on top of them: qn x16 doubles per tile and |w|^2 by padded row; k_cv_trend on a batch behind
// mra_sites_mean (add_v: |w|^2 into the tiles' v as well); k_cv_downdate between mra_cv_gram and the Cholesky; the trend's sums into
// res[3] = {tr K^-1, tr P, max (v + |w|^2) / r} behind mra_cv_reduce (h_has_w: k_cv_trend ran with add_v)
size_t mra_cv_trend_tile_bytes(const mra_plan* pl);
void mra_cv_trend_reserve(mra_plan* pl, long n_tiles);
void mra_cv_trend_rows(mra_plan* pl, long n_tiles, bool add_v);
void mra_cv_trend_downdate(mra_plan* pl, long n_tiles, int nt_max);
void mra_cv_trend_reduce(mra_plan* pl, bool h_has_w);
// mra_launch_laplace.hip: the work buffers of mra_plan_fit_laplace (and the plan's noise / noise_sd); one linearisation at x_in (lap.x
// itself, or the mean of the last pass) -> y, noise, noise_sd, lap.x; the reduction after a pass -> res[MRA_LAPLACE_NRES] = {step,
// max |x^|, sum log D, sum D (t - x^)^2, sum of the x-dependent part of log p}, res a device-visible pointer (the plan's pinned record).
// Launches only, on pl->stream.
constexpr int MRA_LAPLACE_NRES = 5;
constexpr int MRA_HOST_RES_DOUBLES = 16, MRA_HOST_RES_LAPLACE = 8;      // the pinned result record of a pass (mra_plan::host_res)
void mra_laplace_reserve(mra_plan* pl);
void mra_laplace_linearise(mra_plan* pl, int family, const double* x_in);
void mra_laplace_reduce(mra_plan* pl, int family, double* res);
// mra_plan_fit_laplace_trend: the same five results with x^ := e^ = m_t + (X - m_X)^T beta^ from trend.m, trend.X and the beta at the
// head of trend.coef; e^ replaces lap.x at the observed rows (k_laplace_trend_part, k_laplace_sum)
void mra_laplace_trend_reduce(mra_plan* pl, int family, double* res);
void mra_metric_apply(mra_plan* pl);                  // X = A Xraw by row (k_metric_apply), on the plan's stream
// with MRA_OPT_KERNEL_TIMING: `work` between two events on pl->stream, the time added to sit.ms[which] (sit.ms_sink[which] when set; one synchronisation each: a measuring mode)
void mra_sites_timed(mra_plan* pl, int which, const std::function<void()>& work);

// ---- between mra_plan.hip (plans, passes, mra_sample, the C ABI) and mra_calls.hip (the calls on the retained factors) ----------------
// mra_plan.hip, for the calls: one pass (full_rows: W at every row); the kernel times of the events recorded so far, the stream waited
// for; the diag_add of every leaf residual problem; k_panel_chol with the caller's own log-determinant and error slots (nprob > 0) and
// the non-leaf draws of a block of samples, slot-major into zc (Kn > 0) - the two kernels of that unit the calls launch themselves
void mra_run_all(mra_plan* pl, uint32_t flags, bool full_rows = false);
void mra_harvest_kernel_events(mra_plan* pl);
void mra_set_leaf_diag_add(mra_plan* pl, double v);
void mra_panel_chol(mra_plan* pl, const PanelProb* probs, size_t nprob, double* dn, int* err);
void mra_sample_draw(mra_plan* pl, const SampleZ& zs, long Kn, double* zc);
// mra_calls.hip, for mra_sample: the latent slots of the non-leaf nodes, the preamble of every call on the retained factors, the
// sample numbers' check, room for a block's non-leaf draws, and the scope that puts the last mra_run's results back
long mra_coarse_slots(const mra_plan* pl, std::vector<long>* zoff);
void mra_retained_check_plan(const mra_plan* pl, const char* who, uint32_t flags, uint32_t accepted, const char* host_cannot, const char* sharded_cannot,
                             bool dry_last = false);
void mra_check_sample0(int64_t sample0, int64_t n);
void mra_reserve_coarse(DevVec<double>& v, long Kn);
struct KeepResults {
    mra_plan* pl; double *ysave, *msave, *vsave;
    const bool had_ran; const uint32_t had_flags; const double had_d, had_u; const bool had_pred; const size_t bytes;
    KeepResults(mra_plan* p, double* ys, double* ms, double* vs);
    ~KeepResults();
};
// ... and for the C ABI: the drivers of the exports, one each (mra_cv_all: mra_cv and mra_cv_trend)
void mra_solve_all(mra_plan* pl, uint32_t flags, int64_t n, const double* Y, double* mean, double* quad);
void mra_trend_set(mra_plan* pl, int32_t p, const double* X);
void mra_trend_fit_all(mra_plan* pl, uint32_t flags, double* beta, double* cov_beta, double* mean, double* var, double* info);
void mra_cov_all(mra_plan* pl, uint32_t flags, int64_t n, const double* A, double* out, double* gram);
void mra_predict_sites_all(mra_plan* pl, uint32_t flags, int64_t n, const double* sites, const int32_t* leaf, int64_t nc, const double* Y, double* mean, double* var);
void mra_sites_cov_all(mra_plan* pl, uint32_t flags, int64_t n, const double* sites, const int32_t* leaf, double* out);
void mra_sample_sites_all(mra_plan* pl, uint32_t flags, int64_t n, const double* sites, const int32_t* leaf, int64_t ns_all, uint64_t seed, int64_t sample0,
                          const double* z, double* out);
void mra_cv_all(mra_plan* pl, bool trend, uint32_t flags, double* mean, double* var, double* lpd, double* group_lpd, double* info);
void mra_fit_laplace(mra_plan* pl, int family, const double* z, const double* aux, const double* off, const double* x0, int max_iter, double tol, double* info);
void mra_fit_laplace_trend(mra_plan* pl, int family, const double* z, const double* aux, const double* off, const double* e0, int max_iter, double tol,
                           double* beta, double* cov_beta, double* info);
