// mra_plan.hip - host side of libmra_hip.so: plan construction, batched-problem descriptors, the
// launch sequence of one inference pass, mra_sample and the C ABI of include/mra_hip.h.  (The host drivers of the other calls on the
// retained factors are in mra_calls.hip; what the two units see of each other is declared at the end of mra_plan_types.h.)
//
// One pass (mra_run) = what pyMRA's Node.__init__ recursion computes (pyMRA/MRANode.py:23-115):
//   1. prior, top-down per level    (calculatePrior, MRANode.py:378-395, with the conditional
//                                    covariance of :73-80)            -> whitened basis W
//   2. leaves, observation space    (leaf branch of calculatePosterior, :411-430, :450-459)
//   3. non-leaf fronts, bottom-up   (:432-480)
//   4. predictive moments, bottom-up(:486-520)
// DESIGN.md section 3 derives the factorised form; oracle/mra_levelwise.py is its NumPy twin.
#include "mra_plan_types.h"
#include "mra_topology.h"
#include <atomic>
#include <limits>
#include <chrono>
#include <memory>
#include <mutex>
#include <thread>

// MRA_TRACE_PLAN=1: host-side phase times of plan construction on stderr (tools/e2e_breakdown.py)
namespace {
struct PlanTrace {
    bool on;
    double t0, last;
    const char* what;
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    explicit PlanTrace(const char* w) : on(getenv("MRA_TRACE_PLAN") != nullptr), t0(now()), last(t0), what(w) {}
    void mark(const char* label) { if (on) { const double t = now(); fprintf(stderr, "  [%s] %-34s %7.2f ms\n", what, label, t - last); last = t; } }
    ~PlanTrace() { if (on) fprintf(stderr, "  [%s] total %.2f ms (descriptor uploads of this thread so far: %ld, %.2f ms)\n", what, now() - t0, upload_stats().n, upload_stats().ms); }
};
}  // namespace

// ---- device memory cache --------------------------------------------------------------------------------------------
#include <map>
#include <unordered_map>
namespace {
struct DevPool {
    std::mutex mu;
    std::unordered_map<void*, std::pair<int, size_t>> live;           // pointer -> (device, bytes) of pooled-size blocks in use
    std::multimap<std::pair<int, size_t>, void*> idle;                // (device, bytes) -> cached block
    size_t idle_bytes = 0;
    static constexpr size_t MIN_BLOCK = 256 * 1024;                   // smaller blocks are not worth keeping
    // Idle bytes above the cap go back to the driver at once (another runtime in the process - RCCL, a caller's torch - must not
    // run out of memory while blocks sit here).  MRA_POOL_MAX_GB sets it (0 switches the cache off); the default is 16 GB or an
    // eighth of the device's memory, whichever is smaller: four C3-sized plans, not a config-5 one (18 GB of W alone - an MLE
    // loop at that size should keep its plan and call mra_plan_set_kernel, as bench.py does).
    size_t max_idle() {
        if (cap_known) return cap;
        cap = (size_t)16 << 30;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && tot / 8 < cap) cap = tot / 8;
        if (const char* e = getenv("MRA_POOL_MAX_GB")) { const double g = atof(e); cap = g > 0 ? (size_t)(g * (double)((size_t)1 << 30)) : 0; }
        cap_known = true;
        return cap;
    }
    size_t cap = 0;
    bool cap_known = false;
    void flush_locked() {
        for (auto& e : idle) hipFree(e.second);
        idle.clear();
        idle_bytes = 0;
    }
    ~DevPool() { /* process exit: the driver reclaims everything; calling into HIP from a static destructor is not safe */ }
};
DevPool g_pool;
// MRA_POOL_POISON=1 (debug): every block handed out - fresh or reused - is filled with NaNs first, so that a buffer that relies on
// zero-initialised or left-over contents shows up in the results (tests/test_gpu_parity.py runs the oracle parity cases once this way)
inline bool pool_poison() { const char* e = getenv("MRA_POOL_POISON"); return e && e[0] && e[0] != '0'; }
inline hipError_t poison_block(void* p, size_t n) {
    if (!pool_poison() || !p || !n) return hipSuccess;
    hipError_t e = hipMemset(p, 0xFF, n);                              // 0xFFFF...: a quiet NaN in every double, -1 in every int
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e;
}
}  // namespace

hipError_t mraMalloc(void** p, size_t n) {
    if (g_dry) { *p = malloc(n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
    if (n < DevPool::MIN_BLOCK) { hipError_t e = hipMalloc(p, n); return e == hipSuccess ? poison_block(*p, n) : e; }
    int dev = 0;
    hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(g_pool.mu);
    auto it = g_pool.idle.find({dev, n});
    if (it != g_pool.idle.end()) {
        *p = it->second;
        g_pool.idle.erase(it);
        g_pool.idle_bytes -= n;
        g_pool.live[*p] = {dev, n};
        return poison_block(*p, n);
    }
    hipError_t e = hipMalloc(p, n);
    if (e != hipSuccess && !g_pool.idle.empty()) {                    // out of memory with blocks cached: give them back and retry
        (void)hipGetLastError();
        g_pool.flush_locked();
        e = hipMalloc(p, n);
    }
    if (e == hipSuccess) { g_pool.live[*p] = {dev, n}; e = poison_block(*p, n); }
    return e;
}

hipError_t mraFree(void* p) {
    if (g_dry) { free(p); return hipSuccess; }
    if (!p) return hipSuccess;
    std::lock_guard<std::mutex> lock(g_pool.mu);
    auto it = g_pool.live.find(p);
    if (it == g_pool.live.end()) return hipFree(p);
    const std::pair<int, size_t> key = it->second;
    g_pool.live.erase(it);
    if (g_pool.idle_bytes + key.second > g_pool.max_idle()) return hipFree(p);
    g_pool.idle.insert({key, p});
    g_pool.idle_bytes += key.second;
    return hipSuccess;
}

// ---- stream cache: creating the two prioritised streams of a plan costs milliseconds (each is a hardware queue), destroying them
// as much; a process that builds a new MRATree per objective call (README.md:96-104) gets the pair of the previous plan back
namespace {
struct StreamPair { hipStream_t hi, lo; double* host_res; double* host_res_dev; char* arena_host; };      // + the pinned result record and the pinned mirror of the descriptor arena
std::mutex g_streams_mu;
std::multimap<int, StreamPair> g_streams;                           // device -> idle pair (both synchronised when they were returned)
}  // namespace
static void acquire_streams(mra_plan* pl) {
    {
        std::lock_guard<std::mutex> lock(g_streams_mu);
        auto it = g_streams.find(pl->device);
        if (it != g_streams.end()) {
            pl->stream = it->second.hi; pl->stream2 = it->second.lo; pl->host_res = it->second.host_res; pl->host_res_dev = it->second.host_res_dev;
            pl->arena.host = it->second.arena_host;
            g_streams.erase(it);
            return;
        }
    }
    int lo = 0, hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_TRY(hipStreamCreateWithPriority(&pl->stream, hipStreamDefault, hi));
    HIP_TRY(hipStreamCreateWithPriority(&pl->stream2, hipStreamDefault, lo));
}
static void return_streams(mra_plan* pl) {
    if (!pl->stream || !pl->stream2) {
        if (pl->stream) hipStreamDestroy(pl->stream);
        if (pl->stream2) hipStreamDestroy(pl->stream2);
    } else {
        std::lock_guard<std::mutex> lock(g_streams_mu);
        if (g_streams.count(pl->device) < 4) { g_streams.insert({pl->device, StreamPair{pl->stream, pl->stream2, pl->host_res, pl->host_res_dev, pl->arena.host}}); pl->host_res = nullptr; pl->arena.host = nullptr; }
        else { hipStreamDestroy(pl->stream); hipStreamDestroy(pl->stream2); }
    }
    if (pl->host_res) hipHostFree(pl->host_res);
    if (pl->arena.host) { hipHostFree(pl->arena.host); pl->arena.host = nullptr; }
    pl->host_res = pl->host_res_dev = nullptr;
    pl->stream = pl->stream2 = nullptr;
}

// the plan's descriptor arena: a 16 MB device block (from the block cache) and its pinned mirror (kept with the stream pair)
static void init_arena(mra_plan* pl) {
    UploadArena& a = pl->arena;
    a.cap = (size_t)16 << 20;
    a.used = a.flushed = 0;
    if (mraMalloc((void**)&a.dev, a.cap) != hipSuccess) { a.dev = nullptr; a.cap = 0; return; }       // no arena: stand-alone uploads
    if (!a.host) {
        if (g_dry) a.host = (char*)malloc(a.cap);
        else if (hipHostMalloc((void**)&a.host, a.cap, hipHostMallocDefault) != hipSuccess) a.host = nullptr;
    }
    if (!a.host) { mraFree(a.dev); a.dev = nullptr; a.cap = 0; }
}
static void drop_arena(mra_plan* pl) {
    if (pl->arena.dev) mraFree(pl->arena.dev);
    pl->arena.dev = nullptr;
    if (g_dry && pl->arena.host) { free(pl->arena.host); pl->arena.host = nullptr; }
}

bool mra_big_lds_once(int device, const void* fn) {
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    std::lock_guard<std::mutex> lock(mu);
    return done.insert({device, fn}).second;
}

static void derive_kernel_params(KernelParams& kp) {
    kp.mode = 0; kp.a1 = 0.0; kp.a2 = 0.0; kp.amp = kp.scale * kp.sig;
    kp.inv_2l2 = 1.0 / (2.0 * (kp.l * kp.l));
    double c = 1.0;
    switch (kp.kind) {
        case 0: kp.amp = kp.scale; break;                       // ExpCovFun has no sig
        case 1: c = 1.7320508075688772; kp.a1 = 1.0; break;
        case 2: c = 2.23606797749979; kp.a1 = 1.0; kp.a2 = 1.0 / 3.0; break;
        case 3: kp.mode = 1; break;
        case 5: kp.mode = 3; kp.amp = kp.scale; break;                // KanterCovFun(radius = l)
        case MRA_KERNEL_MATERN:                                       // the caller has set kp.nu (and owns kp.nu_tab / nu_n)
            kp.mode = 4; c = std::sqrt(2.0 * kp.nu);
            kp.nu_a = kp.nu < 1.0 ? std::tgamma(1.0 - kp.nu) / (std::tgamma(1.0 + kp.nu) * std::pow(4.0, kp.nu)) : 0.0;
            break;
        default: kp.mode = 2; kp.amp = kp.scale; break;               // Iden (callers refuse unknown kinds before they get here)
    }
    kp.c_inv_l = c / kp.l;
}

// MRA_KERNEL_MATERN: the nodes of the trapezoid rule for K_nu(t) = int_0^inf exp(-t cosh u) cosh(nu u) du (matern_nu_of_t, mra_kernels.h),
// pairs (cosh(k h), c h cosh(nu k h)) with c = 2^(1-nu) / Gamma(nu) and the weight halved at k = 0.  h = 0.2 and 191 nodes (u <= 38):
// 1.1e-14 absolute on M_nu for 0.1 <= nu <= 5 and t >= 2^-40; h = 0.25 is 3e-12 at nu = 5.
static const int MRA_NU_NODES = 191;
static const double MRA_NU_H = 0.2;
static std::vector<double> matern_nu_table(double nu) {
    std::vector<double> t((size_t)2 * MRA_NU_NODES);
    const double c = std::exp((1.0 - nu) * 0.6931471805599453 - std::lgamma(nu));
    for (int k = 0; k < MRA_NU_NODES; ++k) {
        const double u = k * MRA_NU_H;
        t[2 * k] = std::cosh(u);
        t[2 * k + 1] = (k ? 1.0 : 0.5) * (c * MRA_NU_H * std::cosh(nu * u));
    }
    return t;
}
// kind and parameters of mra_plan_set_kernel / mra_eval_kernel, checked before anything changes
static void check_kernel_params(const char* who, int kind, const double* params, int n) {
    const std::string w(who);
    if (kind < 0 || kind > MRA_KERNEL_LOCAL || n < 3) throw MraError(MRA_ERR_INVALID, w + ": unknown kernel kind or too few parameters (need l, sig, scale)");
    if (kind == MRA_KERNEL_LOCAL) {          // params = {l, sig, scale, 0, base_kind}; what depends on the plan (d, metric, the ranges) is checked by mra_plan_set_kernel
        if (n < 5) throw MraError(MRA_ERR_INVALID, w + ": MRA_KERNEL_LOCAL takes {l, sig, scale, 0, base_kind}");
        const double b = params[4];
        if (!(b == MRA_KERNEL_EXP || b == MRA_KERNEL_MATERN32 || b == MRA_KERNEL_MATERN52 || b == MRA_KERNEL_GAUSSIAN))
            throw MraError(MRA_ERR_INVALID, w + ": the base kind of MRA_KERNEL_LOCAL must be EXP, MATERN32, MATERN52 or GAUSSIAN (scale mixtures of Gaussians)");
        if (params[3] != 0.0) throw MraError(MRA_ERR_INVALID, w + ": MRA_KERNEL_LOCAL has no circular distance");
        if (!std::isfinite(params[0]) || !(params[0] > 0.0)) throw MraError(MRA_ERR_INVALID, w + ": length scale (the multiplier l of the range field) must be positive and finite");
        if (!std::isfinite(params[1]) || !(params[1] >= 0.0) || !std::isfinite(params[2])) throw MraError(MRA_ERR_INVALID, w + ": sig must be finite and not negative, scale finite");
        return;
    }
    if (kind == MRA_KERNEL_SUM) {            // params = {K, 0, scale, circular, kind_0, l_0, sig_0, ...}
        const double K = params[0];
        if (!(K >= 1.0 && K <= (double)MRA_SUM_MAX) || K != std::floor(K))
            throw MraError(MRA_ERR_INVALID, w + ": unknown kernel kind or parameter layout: MRA_KERNEL_SUM takes {K, 0, scale, circular, ...} with K an integer in 1.." +
                                            std::to_string(MRA_SUM_MAX) + ", the number of components");
        if (n < 4 + 3 * (int)K) throw MraError(MRA_ERR_INVALID, w + ": MRA_KERNEL_SUM takes {K, 0, scale, circular, kind_0, l_0, sig_0, ...}: too few parameters");
        for (int c = 0; c < (int)K; ++c) {
            const double kc = params[4 + 3 * c], lc = params[5 + 3 * c], sc = params[6 + 3 * c];
            if (!(kc == MRA_KERNEL_EXP || kc == MRA_KERNEL_MATERN32 || kc == MRA_KERNEL_MATERN52 || kc == MRA_KERNEL_GAUSSIAN || kc == MRA_KERNEL_IDEN))
                throw MraError(MRA_ERR_INVALID, w + ": a component of MRA_KERNEL_SUM must be EXP, MATERN32, MATERN52, GAUSSIAN or IDEN");
            if (!std::isfinite(lc) || !(lc > 0.0)) throw MraError(MRA_ERR_INVALID, w + ": length scale must be positive and finite in every component");
            if (!std::isfinite(sc) || !(sc >= 0.0)) throw MraError(MRA_ERR_INVALID, w + ": sig must be finite and not negative in every component");
        }
        return;
    }
    if (kind != MRA_KERNEL_MATERN) return;
    if (n < 5) throw MraError(MRA_ERR_INVALID, w + ": MRA_KERNEL_MATERN takes {l, sig, scale, circular, nu}");
    if (!std::isfinite(params[4]) || params[4] < 0.1 || params[4] > 5.0) throw MraError(MRA_ERR_INVALID, w + ": nu must lie in [0.1, 5]");
    if (!(params[0] > 0.0)) throw MraError(MRA_ERR_INVALID, w + ": length scale must be positive");
}

// MRA_KERNEL_SUM: one record {submode, c_inv_l, inv_2l2, a1, a2, amp_c} per component (cov_sum_of_dist2, mra_kernels.h), each derived by
// derive_kernel_params from (kind_c, l_c, sig_c, scale) - amp_c = scale sig_c for every kind: a component's sig is its sill, which is 1
// for the single kinds that have none (EXP, IDEN), where scale * 1 is scale - and kp.amp = their sum in component order.
static std::vector<double> sum_records(KernelParams& kp, const double* params) {
    const int K = (int)params[0];
    std::vector<double> rec((size_t)MRA_SUM_REC * K);
    double amp = 0.0;
    for (int c = 0; c < K; ++c) {
        KernelParams q{};
        q.kind = (int)params[4 + 3 * c]; q.l = params[5 + 3 * c]; q.sig = params[6 + 3 * c]; q.scale = kp.scale;
        derive_kernel_params(q);
        double* r = &rec[(size_t)MRA_SUM_REC * c];
        r[0] = (double)q.mode; r[1] = q.c_inv_l; r[2] = q.inv_2l2; r[3] = q.a1; r[4] = q.a2; r[5] = kp.scale * q.sig;
        amp += r[5];
    }
    kp.mode = 5; kp.nu_n = K; kp.amp = amp;
    kp.c_inv_l = 0.0; kp.inv_2l2 = 0.0; kp.a1 = 0.0; kp.a2 = 0.0; kp.nu = 0.0; kp.nu_a = 0.0;
    return rec;
}

// MRA_KERNEL_LOCAL: the base kind's derived constants in the fields the closed forms use (c_inv_l, inv_2l2, a1, a2 by
// derive_kernel_params for the base kind), amp = scale sig for every base (sig is the sill, as in MRA_KERNEL_SUM), and nu_n = 1 for
// the Gaussian base, whose t is D^2 / (2 l^2 q) - cov_local_of, mra_kernels.h.  KernelParams keeps its layout.
static void derive_local_params(KernelParams& kp, const double* params) {
    KernelParams q{};
    q.kind = (int)params[4]; q.l = params[0]; q.sig = params[1]; q.scale = params[2];
    derive_kernel_params(q);
    kp.mode = 6; kp.nu_n = q.mode == 1 ? 1 : 0; kp.nu_tab = nullptr; kp.nu = 0.0; kp.nu_a = 0.0;
    kp.c_inv_l = q.c_inv_l; kp.inv_2l2 = q.inv_2l2; kp.a1 = q.a1; kp.a2 = q.a2; kp.amp = params[2] * params[1];
}

// the last coordinate column of n rows of d: its smallest value, NaN if any is not finite (MRA_KERNEL_LOCAL reads a range there)
static double last_column_min(const double* locs, int64_t n, int d) {
    double mn = std::numeric_limits<double>::infinity();
    for (int64_t i = 0; i < n; ++i) {
        const double v = locs[i * d + d - 1];
        if (!std::isfinite(v)) return std::nan("");
        mn = std::min(mn, v);
    }
    return mn;
}
static void require_ranges(const char* who, double mn) {
    if (!(mn > 0.0)) throw MraError(MRA_ERR_INVALID, std::string(who) + ": MRA_KERNEL_LOCAL reads a range out of the last coordinate column, which must be positive and finite at every row");
}

static int fail(mra_plan* p, const MraError& e) {
    if (p) p->err = e.msg;
    g_last_error = e.msg;
    return e.code;
}

static void fill_knot_arrays(mra_plan* pl);

// Workgroups of the full row cascade when it stages all its levels at once (ft_wg0_leaf / ft_wgn_leaf; tile numbers as in ft_row0,
// leaves in order): one per leaf ... or one per family of sibling leaves (same parent = same operand image on every level, staged
// once for all of them) when cascade_group_siblings holds - the cost model of siblings_share_workgroup or MRA_OPT_CASCADE_GROUP.
static void build_leaf_workgroups(mra_plan* pl) {
    std::vector<long> wg0;
    std::vector<int> wgn;
    long tile = 0;
    for (size_t t = 0; t < pl->leaf_nodes.size(); ++t) {
        const int i = pl->leaf_nodes[t];
        const int nt = (int)((pl->row1[i] - pl->row0[i]) / 16);
        const bool join = pl->cascade_group_siblings && t > 0 && pl->parent[i] >= 0 && pl->parent[i] == pl->parent[pl->leaf_nodes[t - 1]] && !wgn.empty();
        if (join) wgn.back() += nt;
        else { wg0.push_back(tile); wgn.push_back(nt); }
        tile += nt;
    }
    pl->ft_wg0_leaf.upload(wg0); pl->ft_wgn_leaf.upload(wgn); pl->n_fwg_leaf = (long)wg0.size();
}

// ------------------------------------------------------------------------------------------------
//  plan construction, part one: what does not depend on the observations.  build_static, at the end of this section, calls the steps
//  in order; the order of the allocations and uploads is part of the result (it is the layout of the descriptor arena).
// ------------------------------------------------------------------------------------------------
// slots of a node's non-leaf ancestors, by level (and of the node itself unless it is a leaf); 0 at the levels below it
static void chain_of(const mra_plan* pl, int node, int* out) {
    for (int k = 0; k < 8; ++k) out[k] = 0;
    for (int i = node; i >= 0; i = pl->parent[i])
        if (!pl->leaf[i]) out[pl->node_level[i]] = pl->node_slot[i];
}

static int device_cu_count(const mra_plan* pl) {
    hipDeviceProp_t prop;
    if (!g_dry && hipGetDeviceProperties(&prop, pl->device) == hipSuccess && prop.multiProcessorCount > 0) return prop.multiProcessorCount;
    return 256;
}

// column layout of W, per-node level and ancestor ranks; the checks of the topology
static void static_layout_and_checks(mra_plan* pl) {
    const int L = pl->n_levels;
    pl->Ka = 0;
    for (int m = 0; m < L; ++m) {
        if (pl->cw[m] % 16) throw MraError(MRA_ERR_INVALID, "cw must be a multiple of 16");
        pl->Ka += pl->cw[m];
    }
    pl->ldw = pl->Ka + MRA_YB;
    pl->coff.assign(L, 0); pl->asuf.assign(L, 0); pl->nf.assign(L, 0); pl->na.assign(L, 0);
    for (int m = 0; m < L; ++m) {
        int s = 0;
        for (int k = m + 1; k < L; ++k) s += pl->cw[k];
        pl->coff[m] = s;
        pl->asuf[m] = s + pl->cw[m];
        pl->nf[m] = pl->ldw - pl->coff[m];
        pl->na[m] = pl->ldw - pl->asuf[m];
    }
    pl->node_level.assign(pl->n_nodes, 0);
    for (int m = 0; m < L; ++m)
        for (long i = pl->level_ptr[m]; i < pl->level_ptr[m + 1]; ++i) pl->node_level[i] = m;
    pl->anc_rank.assign(pl->n_nodes, 0);
    for (int i = 0; i < pl->n_nodes; ++i) {             // nodes are numbered level by level: a parent precedes its children
        const int pa = pl->parent[i];
        if (pa >= 0 && pa < i) pl->anc_rank[i] = pl->anc_rank[pa] + (pl->knot_ptr[pa + 1] - pl->knot_ptr[pa]);
    }
    for (int i = 0; i < pl->n_nodes; ++i) {
        if ((pl->row0[i] % 16) || (pl->row1[i] % 16) || pl->row1[i] < pl->row0[i] || pl->row1[i] > pl->P)
            throw MraError(MRA_ERR_INVALID, "node row ranges must be 16-aligned and inside [0,P)");
        const int m = pl->node_level[i];
        const long rk = pl->knot_ptr[i + 1] - pl->knot_ptr[i];
        if (!pl->leaf[i] && (rk > pl->cw[m] || rk <= 0)) throw MraError(MRA_ERR_INVALID, "non-leaf rank must be in 1..cw[level]");
    }
}

// device arrays shared by everything
static void alloc_shared_arrays(mra_plan* pl) {
    pl->X.alloc((size_t)pl->P * pl->d);
    pl->y.alloc(pl->P);
    pl->W.alloc((size_t)pl->P * pl->ldw);
    pl->var.alloc(pl->P);
    pl->mean.alloc(pl->P);
    pl->dnode.alloc(pl->n_nodes);
    pl->scal.alloc(4);
    pl->errflag.alloc(1);
    HIP_TRY(mraMemset(pl->errflag.p, 0, sizeof(int)));       // k_sum_dnode reads it and clears it again at the end of every pass
    HIP_TRY(mraMemset(pl->W.p, 0, pl->W.n * sizeof(double)));
    HIP_TRY(mraMemset(pl->var.p, 0, pl->var.n * sizeof(double)));
    HIP_TRY(mraMemset(pl->dnode.p, 0, pl->dnode.n * sizeof(double)));
    pl->knots_dev.alloc((size_t)std::max<long>(pl->knot_ptr.back(), 1));       // contents: fill_knot_arrays
}

// The tree's shape, decided once.  shape_regular: every leaf sits on the last level, every other level holds non-leaf nodes only.
// regular (the one-kernel cascades): also one block width of 1, 2 or 4 tiles on at most 8 non-leaf levels, within the cascades'
// register budget.  regular_hi: 5 - 8 non-leaf levels of 64-wide blocks, too many tiles per row for those.  lowrank_parent: the
// fronts of the leaves' parents are too large for the register-resident k_parent_front, only their panels are kept.
static void classify_shape(mra_plan* pl) {
    const int L = pl->n_levels, NL = L - 1;
    bool last_only = true;
    for (int m = 0; m < L && last_only; ++m)
        for (long i = pl->level_ptr[m]; i < pl->level_ptr[m + 1] && last_only; ++i) if ((pl->leaf[i] != 0) != (m == L - 1)) last_only = false;
    bool uniform = true;
    for (int m = 0; m < NL; ++m) if (pl->cw[m] != pl->cw[0]) uniform = false;
    const int cwt = pl->cw[0] / 16;
    pl->shape_regular = L >= 2 && last_only;
    pl->lowrank_parent = L >= 3 && last_only && pl->nf[L - 2] > 256 && pl->cw[L - 2] <= 7 * 16 && !getenv("MRA_NO_LOWRANK_PARENT");
    pl->regular = pl->shape_regular && NL <= 8 && uniform && (cwt == 1 || cwt == 2 || cwt == 4) && cwt * NL <= 16;
    pl->regular_hi = !pl->regular && pl->shape_regular && NL >= 5 && NL <= 8 && uniform && pl->cw[0] == 64;
    if (pl->shape_regular) pl->NL = NL;
    if (pl->regular || pl->regular_hi) pl->CWT = cwt;
}

// knot index arrays for the gather side of the prior GEMM (padded to cw with -1: offsets here, contents in fill_knot_arrays) and the
// levels' factor and front buffers
static void alloc_level_buffers(mra_plan* pl) {
    const int L = pl->n_levels;
    pl->knot_idx_off.assign(pl->n_nodes, -1);
    long tot = 0;
    for (int i = 0; i < pl->n_nodes; ++i) {
        if (pl->leaf[i]) continue;
        pl->knot_idx_off[i] = tot;
        tot += pl->cw[pl->node_level[i]];
    }
    pl->knot_idx.alloc((size_t)std::max<long>(tot, 1));
    pl->lev.clear();
    pl->lev.resize(L);
    pl->node_slot.assign(pl->n_nodes, -1);
    for (int m = 0; m < L; ++m) {
        LevelData& lv = pl->lev[m];
        lv.cw = pl->cw[m]; lv.cwt = lv.cw / 16; lv.c0 = pl->coff[m]; lv.a0 = pl->asuf[m];
        lv.nf = pl->nf[m]; lv.na = pl->na[m];
        lv.panel_only = pl->lowrank_parent && m == L - 2;
        lv.ldf = lv.panel_only ? lv.cw : lv.nf;
        for (long i = pl->level_ptr[m]; i < pl->level_ptr[m + 1]; ++i)
            if (!pl->leaf[i]) { pl->node_slot[i] = (int)lv.nodes.size(); lv.nodes.push_back((int)i); }
        const size_t nn = lv.nodes.size();
        if (!nn) continue;
        if (lv.cw == 0) throw MraError(MRA_ERR_INVALID, "level with non-leaf nodes has cw == 0");
        lv.Lp.alloc(nn * (size_t)lv.cw * lv.cw);
        lv.invP.alloc(nn * (size_t)lv.cwt * 256);
        lv.F.alloc(nn * (size_t)lv.nf * lv.ldf + 16);
        lv.invF.alloc(nn * (size_t)lv.cwt * 256);
    }
}

// leaf numbering and the leaves' Schur blocks Gt
// (row_leaf - padded row -> leaf, 4 bytes per row - is read by two kernels of the general path only: built on first use, ensure_row_leaf)
static void build_leaf_maps(mra_plan* pl) {
    pl->leaf_nodes.clear();
    pl->leaf_slot.assign(pl->n_nodes, -1);
    for (int i = 0; i < pl->n_nodes; ++i)
        if (pl->leaf[i]) { pl->leaf_slot[i] = (int)pl->leaf_nodes.size(); pl->leaf_nodes.push_back(i); }
    pl->leaf_goff.assign(pl->leaf_nodes.size() + 1, 0);
    for (size_t t = 0; t < pl->leaf_nodes.size(); ++t) {
        const int na = pl->na[pl->node_level[pl->leaf_nodes[t]]];
        pl->leaf_goff[t + 1] = pl->leaf_goff[t] + (long)na * na;
    }
    // shape-regular trees build the leaves' parents straight from the children's Ut blocks (segmented SYRK),
    // so the per-leaf Schur blocks Gt (146 GB at 2048^2, M=8, r0=64) are only allocated on demand (ensure_gt)
    if (!pl->shape_regular) pl->Gt.alloc(pl->leaf_goff.back());
}

// one-launch prior of level m (blocks <= 64 wide: four column tiles in registers): the knots' residual block of every node, and the
// level's residual problems cut into blocks of rows with the row solve attached
static void build_prior_level(mra_plan* pl, int m, const std::vector<GemmProb>& resid) {
    LevelData& lv = pl->lev[m];
    const size_t nn = lv.nodes.size();
    const int Kanc = pl->Ka - lv.a0;
    lv.prior_level_ok = lv.cw <= 64 && lv.cw % 16 == 0;
    lv.fl_knot_resid = Work();
    if (!lv.prior_level_ok) return;
    std::vector<GemmProb> kn(nn), fz;
    const long blk = 512;                            // rows per workgroup: four passes of 4 waves x 2 row tiles
    for (size_t s = 0; s < nn; ++s) {
        const int i = lv.nodes[s];
        const long r0 = pl->row0[i], nr = pl->row1[i] - r0;
        const int* kix = pl->knot_idx.p + pl->knot_idx_off[i];
        GemmProb c{};
        c.A = pl->W.p + lv.a0; c.lda = pl->ldw; c.idxA = kix; c.B = c.A; c.ldb = pl->ldw; c.idxB = kix;
        c.C = lv.Lp_of(s); c.ldc = lv.cw; c.XA = pl->X.p; c.XB = pl->X.p;
        c.M = lv.cw; c.N = lv.cw; c.K = Kanc; c.lower = 0; c.sym_diag = 1; c.diag_add = 0.0;
        kn[s] = c;
        const double rkt = (double)(pl->knot_ptr[i + 1] - pl->knot_ptr[i]), anct = (double)pl->anc_rank[i];
        lv.fl_knot_resid += Work(2.0 * rkt * rkt * anct, 2.0 * lv.cw * lv.cw * Kanc, 8.0 * (rkt * (Kanc + pl->d) + (double)lv.cw * lv.cw));
        for (long b0 = 0; b0 < nr; b0 += blk) {
            GemmProb g = resid[s];
            g.A += b0 * pl->ldw; g.C += b0 * pl->ldw; g.XA += b0 * pl->d;
            g.M = (int)std::min(blk, nr - b0);
            g.solveL = lv.Lp_of(s); g.solveI = lv.invP_of(s); g.var = pl->var.p + r0 + b0;
            fz.push_back(g);
        }
    }
    lv.gKnotResid.upload(kn); lv.gResidFused.upload(fz);
}

// descriptors of level m's nodes: prior (residual, kInv, Cholesky, row solve), front (assembly, partial Cholesky, Schur complement)
// and predictive update; the nodes' children are appended to `kids` (uploaded as one array behind the last level)
static void build_level_descriptors(mra_plan* pl, int m, std::vector<AsmChild>& kids) {
    LevelData& lv = pl->lev[m];
    const size_t nn = lv.nodes.size();
    if (!nn) return;
    std::vector<GemmProb> resid(nn), schur(nn), upd(nn);
    std::vector<KinvProb> kinv(nn);
    std::vector<PanelProb> pch(nn), fch(nn);
    std::vector<TrsmNode> tpr(nn), tpo(nn);
    std::vector<Trsm2Prob> t2pr(nn), t2po(nn);
    std::vector<AsmProb> as(nn);
    std::vector<FrontProb> fr(nn);
    const int Kanc = pl->Ka - lv.a0;
    for (size_t s = 0; s < nn; ++s) {
        const int i = lv.nodes[s];
        const long r0 = pl->row0[i], nr = pl->row1[i] - r0;
        lv.max_rows = std::max(lv.max_rows, nr);
        const long rk = pl->knot_ptr[i + 1] - pl->knot_ptr[i];
        double *Lp = lv.Lp_of(s), *invP = lv.invP_of(s), *F = lv.F_of(s), *invF = lv.invF_of(s);
        double* Wown = pl->W.p + r0 * pl->ldw + lv.c0;       // the node's rows, its own columns
        GemmProb g{};
        g.A = pl->W.p + r0 * pl->ldw + lv.a0; g.lda = pl->ldw;
        g.B = pl->W.p + lv.a0; g.ldb = pl->ldw; g.idxB = pl->knot_idx.p + pl->knot_idx_off[i];
        g.C = Wown; g.ldc = pl->ldw;
        g.XA = pl->X.p + r0 * pl->d; g.XB = pl->X.p;
        g.M = (int)nr; g.N = lv.cw; g.K = Kanc; g.lower = 0;
        resid[s] = g;
        const double rkt = (double)rk, anct = (double)pl->anc_rank[i], nat = anct + 1.0;      // true rank, true ancestor columns, + y
        lv.fl_resid += Work(2.0 * nr * rkt * anct, 2.0 * nr * lv.cw * Kanc, 8.0 * nr * (Kanc + lv.cw + pl->d));
        kinv[s] = KinvProb{Lp, pl->knots_dev.p + pl->knot_ptr[i], (int)rk, lv.cw};
        pch[s] = PanelProb{Lp, invP, lv.cw, lv.cwt, lv.cwt, i};
        lv.fl_pchol += Work(rkt * rkt * rkt / 3.0, (double)lv.cw * lv.cw * lv.cw / 3.0, 8.0 * 2 * lv.cw * lv.cw);
        tpr[s] = TrsmNode{Lp, invP, lv.cw, lv.cwt};
        tpo[s] = TrsmNode{F, invF, lv.ldf, lv.cwt};
        lv.fl_trsm += Work((double)nr * rkt * rkt, (double)nr * lv.cw * lv.cw, 8.0 * 2 * nr * lv.cw);
        // (var -= |W^m[x]|^2 rides on the row solve: the prior variance of the level-by-level path, see k_init_yblock)
        t2pr[s] = Trsm2Prob{Lp, invP, Wown, pl->var.p + r0, lv.cw, pl->ldw, lv.cwt, (int)(nr / 16), 0, -1.0, nullptr, nullptr, 0, 0};
        t2po[s] = Trsm2Prob{F, invF, Wown, pl->var.p + r0, lv.ldf, pl->ldw, lv.cwt, (int)(nr / 16), 0, 1.0, nullptr, nullptr, 0, 0};
        lv.max_tiles = std::max(lv.max_tiles, nr / 16);
        fch[s] = PanelProb{F, invF, lv.ldf, lv.nf / 16, lv.cwt, i};
        lv.fl_fchol += Work(rkt * rkt * rkt / 3.0 + nat * rkt * rkt, (double)lv.cw * lv.cw * lv.cw / 3.0 + (double)lv.na * lv.cw * lv.cw,
                            8.0 * (2.5 * lv.nf * (lv.nf + 1) / 2));      // four children's Schur blocks in (lower halves; fewer for ragged trees), the front out
        GemmProb sc{};
        sc.A = F + (size_t)lv.cw * lv.ldf; sc.lda = lv.ldf; sc.B = sc.A; sc.ldb = lv.ldf;
        sc.C = lv.panel_only ? nullptr : F + (size_t)lv.cw * lv.nf + lv.cw; sc.ldc = lv.nf;      // panel_only: no Schur block is ever formed
        sc.M = lv.na; sc.N = lv.na; sc.K = lv.cw; sc.lower = 1;
        schur[s] = sc;
        lv.fl_schur += Work(nat * nat * rkt, (double)lv.na * lv.na * lv.cw, 0.0);
        GemmProb u{};
        u.A = Wown; u.lda = pl->ldw;
        u.B = F + (size_t)lv.cw * lv.ldf; u.ldb = lv.ldf;
        u.C = pl->W.p + r0 * pl->ldw + lv.a0; u.ldc = pl->ldw;
        u.M = (int)nr; u.N = lv.na; u.K = lv.cw; u.lower = 0;
        upd[s] = u;
        lv.fl_update += Work(2.0 * nr * nat * rkt, 2.0 * nr * lv.na * lv.cw, 8.0 * 2 * nr * lv.na);
        AsmProb a{};
        a.F = F; a.nf = lv.nf; a.cw = lv.cw; a.child0 = (int)kids.size();
        a.nchild = pl->child_ptr[i + 1] - pl->child_ptr[i]; a.add_identity = 1;
        for (int c = pl->child_ptr[i]; c < pl->child_ptr[i + 1]; ++c) {
            const int ch = pl->child_list[c];
            if (pl->node_level[ch] != m + 1) throw MraError(MRA_ERR_INVALID, "child must be one level below its parent");
            AsmChild k{};
            pl->kid_leaf.push_back(pl->leaf[ch] ? pl->leaf_slot[ch] : -1);
            if (pl->leaf[ch]) { k.G = pl->Gt.p ? pl->Gt.p + pl->leaf_goff[pl->leaf_slot[ch]] : nullptr; k.ld = pl->na[m + 1]; }
            else {
                const LevelData& cl = pl->lev[m + 1];
                // (children whose fronts are kept as panels have no Schur block: their parents are built by the signed SYRK)
                k.G = cl.panel_only ? nullptr : cl.F_of(pl->node_slot[ch]) + (size_t)cl.cw * cl.nf + cl.cw;
                k.ld = cl.nf;
            }
            if (pl->na[m + 1] != lv.nf) throw MraError(MRA_ERR_INVALID, "front size mismatch");
            kids.push_back(k);
        }
        as[s] = a;
        fr[s] = FrontProb{F, invF, lv.nf, lv.cwt, i, a.child0, a.nchild};
    }
    const long nt = lv.nf / 16;
    const size_t full = (size_t)(nt * (nt + 1) / 2 + lv.cwt) * FT_SZ * sizeof(double);
    const size_t panel = (size_t)(lv.cwt * nt - lv.cwt * (lv.cwt - 1) / 2 + lv.cwt) * FT_SZ * sizeof(double);
    lv.front_mode = full <= 160 * 1024 ? 2 : (panel <= 160 * 1024 ? 1 : 0);
    if (lv.panel_only) lv.front_mode = 0;
    lv.front_lds = lv.front_mode == 2 ? full : panel;
    lv.gFront.upload(fr);
    build_prior_level(pl, m, resid);
    lv.hResid = resid;
    lv.gResid.upload(resid); lv.gSchur.upload(schur); lv.gUpdate.upload(upd); lv.gKinv.upload(kinv);
    lv.gPriorChol.upload(pch); lv.gFrontChol.upload(fch); lv.gTrsmPrior.upload(tpr); lv.gTrsmPost.upload(tpo);
    lv.gAsm.upload(as);
    lv.gTrsm2Prior.upload(t2pr); lv.gTrsm2Post.upload(t2po);
    // (tile_node / tile_row0 - one entry per row tile of the level - serve the row solve of blocks wider than 192 only: ensure_tile_lists)
}

// deep 64-wide trees: row tiles of the leaves with their ancestor chains; one workgroup per leaf (<= 4 tiles) for k_predict_hi, groups
// of eight consecutive tiles below one level-(NL-5) node for the coarse cascade
static void build_hi_tiles(mra_plan* pl) {
    std::vector<long> r0s, wg0, wg0_8;
    std::vector<int> chains, wgn, wgn_8, wgl;
    const int nlo = pl->NL - 4;
    int prev_coarse = -1;
    for (size_t t = 0; t < pl->leaf_nodes.size(); ++t) {
        const int i = pl->leaf_nodes[t];
        int ch[8];
        chain_of(pl, i, ch);
        const int coarse = ch[nlo - 1];                          // slot of the deepest coarse level: same slot = same coarse chain
        for (long p = pl->row0[i]; p < pl->row1[i]; p += 16) {
            const long k = (p - pl->row0[i]) / 16;
            if (k % 4 == 0) { wg0.push_back((long)r0s.size()); wgn.push_back((int)std::min<long>(4, (pl->row1[i] - p) / 16)); wgl.push_back((int)t); }
            if (wgn_8.empty() || wgn_8.back() == 8 || coarse != prev_coarse) { wg0_8.push_back((long)r0s.size()); wgn_8.push_back(0); }
            ++wgn_8.back();
            prev_coarse = coarse;
            r0s.push_back(p);
            for (int k2 = 0; k2 < 8; ++k2) chains.push_back(ch[k2]);
        }
    }
    pl->ft_row0.upload(r0s); pl->ft_chain.upload(chains);
    pl->n_ftiles = (long)r0s.size();
    pl->ft_wg0.upload(wg0); pl->ft_wgn.upload(wgn); pl->n_fwg = (long)wg0.size();
    pl->hi_wgleaf.upload(wgl);
    pl->hi_wg0_8.upload(wg0_8); pl->hi_wgn_8.upload(wgn_8); pl->n_hi_wg8 = (long)wg0_8.size();
}

// regular trees, per non-leaf level: the knot pass's buffers, knot row tiles (with chains and workgroups) and kInv products
static void build_fused_levels(mra_plan* pl) {
    const int cw = pl->cw[0];
    pl->fl.clear();
    pl->fl.resize(pl->NL);
    for (int m = 0; m < pl->NL; ++m) {
        mra_plan::FusedLevel& f = pl->fl[m];
        const LevelData& lv = pl->lev[m];
        const size_t nn = lv.nodes.size();
        f.kx.alloc(nn * (size_t)cw * pl->d);
        f.Wk.alloc(std::max<size_t>(nn * (size_t)cw * (m * cw), 1));
        std::vector<int> kv(nn * (size_t)cw), rows, chain, knot0, wgn;
        std::vector<long> wg0;
        for (size_t sl = 0; sl < nn; ++sl) {
            const int i = lv.nodes[sl];
            const long rk = pl->knot_ptr[i + 1] - pl->knot_ptr[i];
            for (int c = 0; c < cw; ++c) kv[sl * cw + c] = c < rk ? 1 : 0;
            int ch[8];
            chain_of(pl, i, ch);
            // one workgroup per family of siblings (same ancestor chain: the staged operands are shared),
            // as long as it stays within 8 row tiles (one per wave on the level-by-level staging path)
            // (only on levels with many nodes, where workgroups run in several rounds per CU: on small levels
            // - the levels of a sharded rank - the longer per-workgroup chain costs more than it saves)
            const bool same_family = nn >= 512 && sl > 0 && pl->parent[i] >= 0 && pl->parent[i] == pl->parent[lv.nodes[sl - 1]] &&
                                     !wgn.empty() && wgn.back() + cw / 16 <= 8;
            if (same_family) wgn.back() += cw / 16;
            else { wg0.push_back((long)knot0.size()); wgn.push_back(cw / 16); }
            for (int tt = 0; tt < cw / 16; ++tt) {
                for (int r = 0; r < 16; ++r) rows.push_back(-1);          // contents: fill_knot_arrays
                for (int k = 0; k < 8; ++k) chain.push_back(ch[k]);
                knot0.push_back(tt * 16);
            }
        }
        f.kvalid.upload(kv); f.kt_rows.upload(rows); f.kt_chain.upload(chain); f.kt_knot0.upload(knot0);
        f.n_ktiles = (long)knot0.size();
        f.kt_wg0.upload(wg0); f.kt_wgn.upload(wgn); f.n_kwg = (long)wg0.size();
        f.k_threads = 256;
        for (int v : wgn) if (v > 4) f.k_threads = 512;
        // kInv of every node of the level: kernel(knots, knots) - Wk Wk^T as one batched COV product
        std::vector<GemmProb> gk(nn);
        for (size_t sl = 0; sl < nn; ++sl) {
            GemmProb g{};
            g.A = f.Wk.p + sl * (size_t)cw * (m * cw); g.lda = m * cw; g.B = g.A; g.ldb = m * cw;
            g.C = lv.Lp_of(sl); g.ldc = cw;
            g.XA = f.kx.p + sl * (size_t)cw * pl->d; g.XB = g.XA;
            g.M = cw; g.N = cw; g.K = m * cw; g.lower = 0;
            gk[sl] = g;
        }
        f.gKinv.upload(gk);
    }
}

// k_knot_chain: one workgroup per node of the last non-leaf level; owner of an upper node = first workgroup below it
// (it recomputes every ancestor in every workgroup, so it only pays while one round of workgroups covers the
// level: the chain covers levels 0 .. kc_levels-1, the deepest level with at most one workgroup per CU; deeper
// levels - many nodes, throughput-bound - keep their per-level launches)
static void build_knot_chain(mra_plan* pl, int ncu) {
    int nlv = 1;
    while (nlv < pl->NL && (long)pl->lev[nlv].nodes.size() <= ncu) ++nlv;
    pl->kc_levels = nlv;
    const int cwt = pl->CWT;
    const LevelData& lb = pl->lev[nlv - 1];
    std::vector<int> kch(lb.nodes.size() * 8, 0);
    std::vector<std::vector<int>> own(nlv);
    for (int m = 0; m < nlv; ++m) own[m].assign(pl->lev[m].nodes.size(), -1);
    for (size_t b = 0; b < lb.nodes.size(); ++b) {
        int* ch = kch.data() + b * 8;
        chain_of(pl, lb.nodes[b], ch);
        for (int m = 0; m < nlv; ++m) if (own[m][ch[m]] < 0) own[m][ch[m]] = (int)b;
    }
    pl->kc_chain.upload(kch);
    pl->kc_chain_host = kch;
    std::vector<int> mask(lb.nodes.size(), 0);
    for (size_t b = 0; b < lb.nodes.size(); ++b)
        for (int m = 0; m < nlv; ++m) if (own[m][kch[b * 8 + m]] == (int)b) mask[b] |= 1 << m;
    pl->kc_ownmask.upload(mask);
    pl->kc_knots.alloc(lb.nodes.size() * (size_t)nlv * cwt * 16 * (pl->d + 1));        // filled by mra_plan_set_locs
    const long off = (long)cwt * cwt * ((nlv - 1) * (nlv - 2) / 2) + (long)(nlv - 1) * (cwt * (cwt - 1) / 2 + cwt);
    pl->knot_chain_lds = (size_t)off * 2048 + (size_t)(cwt * (cwt + 1) / 2 + cwt) * FT_SZ * sizeof(double)
                         + (size_t)nlv * cwt * 16 * (pl->d + 1) * sizeof(double);    // + the chain's knots (coordinates, real/phantom flags)
    pl->knot_chain_ok = pl->knot_chain_lds <= 160 * 1024;
}

// The full row cascade, all levels staged at once: one workgroup (8 waves, the whole LDS) per leaf or per family of sibling leaves?
// Rounds of workgroups over the CUs times [staging the operand image (~5 us, exposed: one workgroup per CU) + rounds of 8 row tiles
// (~32 us each)].  Measured on shards of C3: 256 families on 256 CUs = one round of 64 tiles (261 us) against four rounds of 16
// (316 us); 128 families leave half the CUs idle (261 against 158 us).  (MRA_OPT_CASCADE_GROUP overrides the verdict.)
static bool siblings_share_workgroup(const mra_plan* pl, int ncu) {
    size_t nparents = 0;
    long ntiles_all = 0;
    for (size_t t = 0; t < pl->leaf_nodes.size(); ++t) {
        if (t == 0 || pl->parent[pl->leaf_nodes[t]] != pl->parent[pl->leaf_nodes[t - 1]]) ++nparents;
        ntiles_all += (pl->row1[pl->leaf_nodes[t]] - pl->row0[pl->leaf_nodes[t]]) / 16;
    }
    const size_t nl_ = std::max<size_t>(1, pl->leaf_nodes.size()), np_ = std::max<size_t>(1, nparents);
    const double t_leaf = std::ceil((double)ntiles_all / nl_ / 8.0), t_fam = std::ceil((double)ntiles_all / np_ / 8.0);
    const double cost_leaf = std::ceil((double)nl_ / ncu) * (5.0 + 32.0 * t_leaf), cost_fam = std::ceil((double)np_ / ncu) * (5.0 + 32.0 * t_fam);
    return cost_fam < cost_leaf;
}

// regular trees: the row tiles of the leaves with their chains, the cascades' workgroups (in tile order, and dealt to the XCDs for
// the predictive cascade), the cascades' LDS sizes
static void build_cascade_tiles(mra_plan* pl) {
    std::vector<long> r0s, fwg0;
    std::vector<int> chains, fwgn, tleaf;
    for (size_t t = 0; t < pl->leaf_nodes.size(); ++t) {
        const int i = pl->leaf_nodes[t];
        int ch[8];
        chain_of(pl, i, ch);
        for (long p = pl->row0[i]; p < pl->row1[i]; p += 16) {
            if (((p - pl->row0[i]) / 16) % pl->cascade_wpw == 0) {
                fwg0.push_back((long)r0s.size());
                fwgn.push_back((int)std::min<long>(pl->cascade_wpw, (pl->row1[i] - p) / 16));
            }
            r0s.push_back(p);
            tleaf.push_back((int)t);
            for (int k = 0; k < 8; ++k) chains.push_back(ch[k]);
        }
    }
    pl->ft_row0.upload(r0s); pl->ft_chain.upload(chains); pl->ft_leaf.upload(tleaf);
    pl->n_ftiles = (long)r0s.size();
    pl->ft_wg0.upload(fwg0); pl->ft_wgn.upload(fwgn); pl->n_fwg = (long)fwg0.size();
    // the same workgroups ordered for the predictive cascade: workgroup b runs on XCD b % 8, and the workgroups of
    // one leaf all stream that leaf's Ut block, so they are dealt to one XCD (one L2) -- empty slots pad the lanes
    std::vector<std::vector<size_t>> lane(8);
    for (size_t g = 0; g < fwg0.size(); ++g) lane[(size_t)tleaf[(size_t)fwg0[g]] % 8].push_back(g);
    size_t deep = 0;
    for (const auto& l : lane) deep = std::max(deep, l.size());
    std::vector<long> x0(deep * 8, 0);
    std::vector<int> xn(deep * 8, 0), xl(deep * 8, 0);
    for (size_t k = 0; k < deep; ++k)
        for (size_t x = 0; x < 8; ++x)
            if (k < lane[x].size()) { x0[k * 8 + x] = fwg0[lane[x][k]]; xn[k * 8 + x] = fwgn[lane[x][k]]; xl[k * 8 + x] = tleaf[(size_t)fwg0[lane[x][k]]]; }
    pl->ft_wg0_x.upload(x0); pl->ft_wgn_x.upload(xn); pl->ft_wgleaf_x.upload(xl); pl->n_fwg_x = (long)x0.size();
    const int cwt = pl->CWT, nl = pl->NL;
    pl->cascade_lds = (size_t)(cwt * (nl - 1) * cwt + cwt * (cwt - 1) / 2 + cwt) * 2048;
    pl->cascade_lds_all = (size_t)(cwt * cwt * (nl * (nl - 1) / 2) + nl * (cwt * (cwt - 1) / 2 + cwt)) * 2048;
    pl->cascade_stage_all = pl->cascade_lds_all <= 160 * 1024;
    build_leaf_workgroups(pl);
}

static void build_static(mra_plan* pl) {
    PlanTrace tr("build_static");
    ArenaScope arena(&pl->arena);
    static_layout_and_checks(pl);
    alloc_shared_arrays(pl);
    tr.mark("checks, allocations, memsets");
    classify_shape(pl);                     // (before the level buffers: the parents' fronts are sized by lowrank_parent)
    alloc_level_buffers(pl);
    tr.mark("knot_idx, level buffers");
    build_leaf_maps(pl);
    tr.mark("leaf maps (row_leaf upload)");
    std::vector<AsmChild> kids;
    pl->kid_leaf.clear();
    for (int m = 0; m < pl->n_levels; ++m) build_level_descriptors(pl, m, kids);
    pl->asmKids.upload(kids);
    pl->hKids = kids;
    tr.mark("per-level descriptors");
    if (pl->regular_hi) build_hi_tiles(pl);
    if (pl->regular) {
        const int ncu = device_cu_count(pl);
        pl->n_cu = ncu;                     // (regular trees only: route_for reads it on every path)
        build_fused_levels(pl);
        build_knot_chain(pl, ncu);
        tr.mark("fused levels, knot chain");
        pl->cascade_group_siblings = siblings_share_workgroup(pl, ncu);
        build_cascade_tiles(pl);
        tr.mark("row tiles of the cascades");
    }
    arena.finish();
    tr.mark("descriptor arena to the device");
    if (!pl->knots_pending) { fill_knot_arrays(pl); tr.mark("knot arrays"); }
}

// Everything in the plan that holds knot ROWS (as opposed to knot counts): the device copy of knot_rows, the padded per-node
// index lists of the prior products, the knot row tiles of the fused levels.  The arrays are sized by build_static; a plan
// built beside the knot draws (mra_plan_create_replay_2d) gets their contents here, once the draws are done.
static void fill_knot_arrays(mra_plan* pl) {
    if ((long)pl->knot_rows.size() != pl->knot_ptr.back()) throw MraError(MRA_ERR_INVALID, "knot_rows does not match knot_ptr");
    // (the device only ever looks at the knot rows of NON-leaf nodes - the kInv gather of the level-by-level prior; the leaves'
    //  entries, nine tenths of the 8 MB at 1024^2, stay on the host)
    {
        long kmax = 0;
        for (int i = 0; i < pl->n_nodes; ++i) if (!pl->leaf[i]) kmax = std::max(kmax, pl->knot_ptr[i + 1]);
        if (kmax > 0) HIP_TRY(mraMemcpy(pl->knots_dev.p, pl->knot_rows.data(), (size_t)kmax * sizeof(long), hipMemcpyHostToDevice));
    }
    std::vector<int> kidx(pl->knot_idx.n, -1);
    for (int i = 0; i < pl->n_nodes; ++i) {
        if (pl->leaf[i]) continue;
        const int m = pl->node_level[i];
        const long rk = pl->knot_ptr[i + 1] - pl->knot_ptr[i];
        for (int c = 0; c < pl->cw[m] && c < rk; ++c) kidx[pl->knot_idx_off[i] + c] = (int)pl->knot_rows[pl->knot_ptr[i] + c];
    }
    pl->knot_idx.fill(kidx);
    if (pl->regular) {
        const int cw = pl->cw[0];
        for (int m = 0; m < pl->NL; ++m) {
            const LevelData& lv = pl->lev[m];
            std::vector<int> rows(lv.nodes.size() * (size_t)cw, -1);
            for (size_t sl = 0; sl < lv.nodes.size(); ++sl) {
                const int i = lv.nodes[sl];
                const long rk = pl->knot_ptr[i + 1] - pl->knot_ptr[i];
                for (int c = 0; c < cw && c < rk; ++c) rows[sl * cw + c] = (int)pl->knot_rows[pl->knot_ptr[i] + c];
            }
            pl->fl[m].kt_rows.fill(rows);
        }
    }
}

// ------------------------------------------------------------------------------------------------
//  plan construction, part two: what depends on which rows are observed.  build_leaf, at the end of this section, runs on every
//  set_obs (on a plan whose static part exists) and calls the steps in order; nothing is kept from one call to the next.
// ------------------------------------------------------------------------------------------------
// host copies of the per-leaf lists and descriptors, in leaf order, as they pass from step to step
struct LeafDescs {
    std::vector<int> nobs;                      // observed rows per leaf
    std::vector<long> obs_off;                  // [leaf + 1] offset of the leaf's list in obs_idx (multiples of 16)
    std::vector<LeafProb> lp;
    std::vector<GemmProb> resid, resid_lik, syrk, upd;
    std::vector<PanelProb> chol_full, chol_lik, chol_c;
    std::vector<Trsm2Prob> trsm_full, trsm_lik;
};

// observed rows per leaf: counted and listed by a few threads over runs of leaves (one pass over y each); the panels' sizes
static void build_obs_lists(mra_plan* pl, const double* y, LeafDescs& d) {
    const size_t nl = pl->leaf_nodes.size();
    pl->leaf_nop.assign(nl, 0);
    pl->leaf_poff.assign(nl + 1, 0);
    pl->leaf_ioff.assign(nl + 1, 0);
    std::vector<int> obs, opos(pl->P);
    std::vector<int>& nobs = d.nobs;
    std::vector<long>& obs_off = d.obs_off;
    nobs.assign(nl, 0); obs_off.assign(nl + 1, 0);
    const int64_t leaves_per_thread = std::max<int64_t>(1, (int64_t)(65536 * nl / std::max<long>(pl->P, 1)));
    parallel_rows((int64_t)nl, [&](int64_t a, int64_t b) {
        for (int64_t t = a; t < b; ++t) {
            const int i = pl->leaf_nodes[t];
            int no = 0;
            for (long p = pl->row0[i]; p < pl->row1[i]; ++p) no += std::isfinite(y[p]) ? 1 : 0;
            nobs[t] = no;
        }
    }, leaves_per_thread);
    pl->leaf_max_rows = 0; pl->leaf_max_nop = 0; pl->leaf_max_na = 0; pl->leaf_max_ht = 0;
    for (size_t t = 0; t < nl; ++t) {
        const int i = pl->leaf_nodes[t];
        const int na = pl->na[pl->node_level[i]];
        const int no = nobs[t], nop = (no + 15) / 16 * 16;
        obs_off[t + 1] = obs_off[t] + nop;
        pl->leaf_nop[t] = nop;
        const long nr = pl->row1[i] - pl->row0[i];
        pl->leaf_poff[t + 1] = pl->leaf_poff[t] + (long)(nop + na + nr) * nop;
        pl->leaf_ioff[t + 1] = pl->leaf_ioff[t] + (long)(nop / 16) * 256;
        pl->leaf_max_rows = std::max(pl->leaf_max_rows, nr);
        pl->leaf_max_nop = std::max(pl->leaf_max_nop, nop);
        pl->leaf_max_na = std::max(pl->leaf_max_na, na);
        pl->leaf_max_ht = std::max(pl->leaf_max_ht, (int)((nop + na + nr) / 16));
    }
    obs.resize((size_t)obs_off[nl]);
    {
        // rows outside every leaf (orphan knot rows of a shard) are nobody's observation
        long covered = 0;
        for (size_t t = 0; t < nl; ++t) covered += pl->row1[pl->leaf_nodes[t]] - pl->row0[pl->leaf_nodes[t]];
        if (covered != pl->P) std::fill(opos.begin(), opos.end(), -1);
    }
    parallel_rows((int64_t)nl, [&](int64_t a, int64_t b) {
        for (int64_t t = a; t < b; ++t) {
            const int i = pl->leaf_nodes[t];
            int* o = obs.data() + obs_off[t];
            int no = 0;
            for (long p = pl->row0[i]; p < pl->row1[i]; ++p) {
                const bool f = std::isfinite(y[p]);
                opos[p] = f ? no : -1;
                if (f) o[no++] = (int)p;
            }
            for (int k = no; k < pl->leaf_nop[t]; ++k) o[k] = -1;
        }
    }, leaves_per_thread);
    pl->obs_idx.upload(obs); pl->obs_pos.upload(opos); pl->leaf_nobs.upload(nobs);
    pl->obs_list_host.swap(obs);                       // (the mask a kept residual belongs to: set_obs compares)
    pl->obs_off_host = obs_off; pl->lik_tiles_valid = false; pl->lik_general_valid = false;
    pl->y_finite_host.assign(pl->P, 0);
    for (long p2 = 0; p2 < pl->P; ++p2) pl->y_finite_host[p2] = std::isfinite(y[p2]) ? 1 : 0;
}

// per leaf: residual (full and likelihood-only), factorisation, row solves, SYRK and update problems, with their work counts
static void build_leaf_descriptors(mra_plan* pl, LeafDescs& d) {
    const size_t nl = pl->leaf_nodes.size();
    d.lp.resize(nl);
    d.resid.resize(nl); d.syrk.resize(nl); d.upd.resize(nl); d.resid_lik.resize(nl);
    d.chol_full.resize(nl); d.chol_lik.resize(nl); d.chol_c.resize(nl);
    d.trsm_full.resize(nl); d.trsm_lik.resize(nl);
    pl->leaf_max_tiles_full = pl->leaf_max_tiles_lik = 0;
    pl->fl_leaf_resid = pl->fl_leaf_chol = pl->fl_leaf_chol_lik = pl->fl_leaf_syrk = pl->fl_leaf_update = pl->fl_leaf_c_only = Work();
    pl->by_leaf_ut = pl->by_leaf_tt = pl->by_leaf_c = 0;
    for (size_t t = 0; t < nl; ++t) {
        const int i = pl->leaf_nodes[t];
        const int m = pl->node_level[i];
        const int na = pl->na[m], a0 = pl->asuf[m], nop = pl->leaf_nop[t];
        const long r0 = pl->row0[i], nr = pl->row1[i] - r0;
        const int Kanc = pl->Ka - a0;
        double *Pn = leaf_C(pl, t), *Ut = leaf_Ut(pl, t), *V = leaf_V(pl, t);
        LeafProb q{};
        q.Pn = Pn; q.obs = pl->obs_idx.p + d.obs_off[t]; q.row0 = r0; q.ld = nop; q.nrows = (int)nr;
        q.nop = nop; q.na = na; q.a0 = a0; q.node = i;
        d.lp[t] = q;
        GemmProb g{};
        g.A = pl->W.p + r0 * pl->ldw + a0; g.lda = pl->ldw;
        g.B = pl->W.p + a0; g.ldb = pl->ldw; g.idxB = q.obs;
        g.C = V; g.ldc = nop;
        g.XA = pl->X.p + r0 * pl->d; g.XB = pl->X.p;
        g.M = (int)nr; g.N = nop; g.K = Kanc; g.lower = 0;
        g.rowmap = pl->obs_pos.p + r0; g.C2 = Pn; g.diag_add = pl->R;
        d.resid[t] = g;
        {
            // likelihood-only runs need just C = v_m(o,o) + R I (diag_add 0 while a noise vector is set: run_leaf_noise): both sides gathered through the observation list
            GemmProb c{};
            c.A = pl->W.p + a0; c.lda = pl->ldw; c.idxA = q.obs; c.B = c.A; c.ldb = pl->ldw; c.idxB = q.obs;
            c.C = Pn; c.ldc = nop; c.XA = pl->X.p; c.XB = pl->X.p;
            c.M = nop; c.N = nop; c.K = Kanc; c.lower = 1; c.sym_diag = 1; c.diag_add = pl->R;
            d.resid_lik[t] = c;
        }
        const double no = (double)d.nobs[t], anct = (double)pl->anc_rank[i], nat = anct + 1.0;      // true sizes: observations, ancestor columns, + y
        pl->by_leaf_ut += 8.0 * na * nop; pl->by_leaf_tt += 8.0 * nr * nop; pl->by_leaf_c += 8.0 * nop * nop;
        pl->fl_leaf_resid += Work(2.0 * nr * no * anct, 2.0 * nr * nop * Kanc, 8.0 * (nr * (Kanc + pl->d) + (double)nr * nop + (double)nop * nop));
        pl->fl_leaf_c_only += Work(no * no * anct, (double)nop * nop * Kanc, 8.0 * (no * (Kanc + pl->d) + (double)nop * nop));
        double* inv = pl->leafInv.p + pl->leaf_ioff[t];
        d.chol_full[t] = PanelProb{Pn, inv, nop, (int)((nop + na + nr) / 16), nop / 16, i};
        d.chol_lik[t] = PanelProb{Pn, inv, nop, (nop + na) / 16, nop / 16, i};
        d.chol_c[t] = PanelProb{Pn, inv, nop, nop / 16, nop / 16, i};
        d.trsm_full[t] = Trsm2Prob{Pn, inv, Ut, pl->var.p + r0, nop, nop, nop / 16, (int)((na + nr) / 16), na / 16, -1.0, q.obs, pl->W.p + a0, pl->ldw, na / 16};
        d.trsm_lik[t] = Trsm2Prob{Pn, inv, Ut, nullptr, nop, nop, nop / 16, na / 16, 0, 1.0, q.obs, pl->W.p + a0, pl->ldw, na / 16};
        pl->leaf_max_tiles_full = std::max(pl->leaf_max_tiles_full, (int)((na + nr) / 16));
        pl->leaf_max_tiles_lik = std::max(pl->leaf_max_tiles_lik, na / 16);
        pl->fl_leaf_chol += Work(no * no * no / 3.0 + (nat + nr) * no * no, (double)nop * nop * nop / 3.0 + (double)(na + nr) * nop * nop,
                                 8.0 * (1.5 * nop * nop + 2.0 * (na + nr) * nop + 2.0 * nr));
        pl->fl_leaf_chol_lik += Work(no * no * no / 3.0 + nat * no * no, (double)nop * nop * nop / 3.0 + (double)na * nop * nop,
                                     8.0 * (1.5 * nop * nop + 2.0 * na * nop));
        GemmProb s{};
        s.A = Ut; s.lda = nop; s.B = s.A; s.ldb = nop;
        s.C = pl->Gt.p ? pl->Gt.p + pl->leaf_goff[t] : nullptr; s.ldc = na; s.M = na; s.N = na; s.K = nop; s.lower = 1;
        d.syrk[t] = s;
        pl->fl_leaf_syrk += Work(nat * nat * no, (double)na * na * nop, 8.0 * na * nop);
        GemmProb u{};
        u.A = V; u.lda = nop; u.B = Ut; u.ldb = nop;
        u.C = pl->W.p + r0 * pl->ldw + a0; u.ldc = pl->ldw; u.M = (int)nr; u.N = na; u.K = nop; u.lower = 0;
        u.zc = na - MRA_YB;                  // y block: C_in = 0 (the column still holds y itself)
        d.upd[t] = u;
        pl->fl_leaf_update += Work(2.0 * nr * nat * no, 2.0 * nr * na * nop, 8.0 * ((double)nr * nop + (double)na * nop + 2.0 * nr * na));
    }
}

// the Ut pointer list of the leaves, and the panels cleared
static void upload_leaf_ut_and_clear_panels(mra_plan* pl) {
    const size_t nl = pl->leaf_nodes.size();
    std::vector<double*> uts(nl);
    for (size_t t = 0; t < nl; ++t) uts[t] = leaf_Ut(pl, t);
    pl->leaf_ut.upload(uts);
    pl->leaf_nop_dev.upload(pl->leaf_nop);
    // the Ut blocks start from zero: rows of the y block beyond y itself and phantom observation columns stay zero
    if (pl->panel.n) HIP_TRY(mraMemset(pl->panel.p, 0, pl->panel.n * sizeof(double)));
}

// where a node's K segments sit in a segment list: (first, count)
typedef std::vector<std::pair<size_t, int>> SegRanges;

// fronts of the leaves' parents straight from the children's Ut (segmented SYRK): one segment per child
static void build_parent_syrk(mra_plan* pl, std::vector<GemmSeg>& segs, SegRanges& where) {
    const LevelData& lv = pl->lev[pl->NL - 1];
    std::vector<GemmProb> ps(lv.nodes.size());
    where.resize(lv.nodes.size());
    for (size_t sidx = 0; sidx < lv.nodes.size(); ++sidx) {
        const int i = lv.nodes[sidx];
        where[sidx] = {segs.size(), pl->child_ptr[i + 1] - pl->child_ptr[i]};
        for (int c = pl->child_ptr[i]; c < pl->child_ptr[i + 1]; ++c) {
            const int lt = pl->leaf_slot[pl->child_list[c]];
            const int nop = pl->leaf_nop[lt];
            double* ut = leaf_Ut(pl, lt);
            segs.push_back(GemmSeg{ut, ut, nop, nop, nop, 0});
        }
    }
    pl->parentSegs.upload(segs);
    for (size_t sidx = 0; sidx < lv.nodes.size(); ++sidx) {
        GemmProb g{};
        g.C = lv.panel_only ? nullptr : lv.F_of(sidx); g.ldc = lv.nf; g.M = lv.nf; g.N = lv.nf; g.lower = 1;      // (not launched when panel_only)
        g.segs = pl->parentSegs.p + where[sidx].first; g.nseg = where[sidx].second; g.diag_one = lv.cw;
        if (g.nseg == 0) { g.nseg = 0; g.K = 0; g.A = g.B = pl->W.p; }
        ps[sidx] = g;
    }
    pl->gParentSyrk.upload(ps);
    pl->parent_syrk = true;
}

// lowrank_parent - panels of the leaves' parents, in three launches: the own block F_oo = I + U_o U_o^T with its Cholesky
// (k_parent_front on a front of cw rows: everything in registers / LDS), the rows below F_ao = U_a U_o^T (one GEMM over the children's
// Ut segments, A = their ancestor rows, B = their own-block rows), and the row solve Zt = F_ao Lt^-T in place
static void build_parent_panels(mra_plan* pl, const LeafDescs& d, const std::vector<GemmSeg>& segs, const SegRanges& where) {
    const LevelData& lv = pl->lev[pl->NL - 1];
    std::vector<GemmSeg> segs_ao;
    for (const GemmSeg& sg : segs) segs_ao.push_back(GemmSeg{sg.A + (size_t)lv.cw * sg.lda, sg.B, sg.lda, sg.ldb, sg.K, 0});
    pl->parentSegsAo.upload(segs_ao);
    std::vector<GemmProb> pp(lv.nodes.size());
    std::vector<FrontProb> pown(lv.nodes.size());
    std::vector<Trsm2Prob> pzt(lv.nodes.size());
    for (size_t sidx = 0; sidx < lv.nodes.size(); ++sidx) {
        double* panel_s = lv.F_of(sidx);
        double* inv_s = lv.invF_of(sidx);
        GemmProb g{};
        g.C = panel_s + (size_t)lv.cw * lv.ldf; g.ldc = lv.ldf; g.M = lv.na; g.N = lv.cw; g.lower = 0;
        g.segs = pl->parentSegsAo.p + where[sidx].first; g.nseg = where[sidx].second; g.diag_one = 0;
        if (g.nseg == 0) { g.K = 0; g.A = g.B = pl->W.p; }
        pp[sidx] = g;
        pown[sidx] = FrontProb{panel_s, inv_s, lv.cw, lv.cwt, lv.nodes[sidx], (int)where[sidx].first, where[sidx].second};
        pzt[sidx] = Trsm2Prob{panel_s, inv_s, panel_s + (size_t)lv.cw * lv.ldf, nullptr, lv.ldf, lv.ldf, lv.cwt, lv.na / 16, 0, 1.0, nullptr, nullptr, 0, 0};
        const int i = lv.nodes[sidx];
        const double rkt = (double)(pl->knot_ptr[i + 1] - pl->knot_ptr[i]), nat = (double)pl->anc_rank[i] + 1.0;
        double kobs = 0, kpad = 0;
        for (int c = pl->child_ptr[i]; c < pl->child_ptr[i + 1]; ++c) { const int lt = pl->leaf_slot[pl->child_list[c]]; kobs += d.nobs[lt]; kpad += pl->leaf_nop[lt]; }
        pl->fl_parent_panel += Work(2.0 * (rkt + nat) * rkt * kobs, 2.0 * lv.nf * lv.cw * kpad, 8.0 * (lv.nf * kpad + (double)lv.nf * lv.cw));
    }
    pl->gParentPanel.upload(pp);
    // the LDS-tiled segmented product keeps its K steps as a table of SB_MAXST2 entries
    pl->parent_panel_lds_ok = true;
    for (size_t sidx = 0; sidx < lv.nodes.size() && pl->parent_panel_lds_ok; ++sidx) {
        long steps = 0;
        for (int k = 0; k < where[sidx].second; ++k) steps += segs_ao[where[sidx].first + k].K / 16;
        if (where[sidx].second > SB_MAXST2 || steps > SB_MAXST2) pl->parent_panel_lds_ok = false;
    }
    pl->gParentOwn.upload(pown);
    pl->gParentZt.upload(pzt);
    const long nt = lv.cwt, npanel = lv.cwt * nt - lv.cwt * (lv.cwt - 1) / 2;
    pl->parent_own_lds = (size_t)(2 * lv.cw * PF_LD + (npanel + lv.cwt) * FT_SZ) * sizeof(double);
}

// lowrank_parent - fronts of the grandparents: I + sum over grandchild leaves Ut[anc] Ut[anc]^T - sum over children Zt Zt^T
static void build_grand_syrk(mra_plan* pl, const LeafDescs& d) {
    const LevelData& lv = pl->lev[pl->NL - 1];
    const LevelData& lg = pl->lev[pl->NL - 2];
    std::vector<GemmSeg> gsegs;
    SegRanges gwhere(lg.nodes.size());
    for (size_t sidx = 0; sidx < lg.nodes.size(); ++sidx) {
        const int i = lg.nodes[sidx];
        const size_t first = gsegs.size();
        const double rkt = (double)(pl->knot_ptr[i + 1] - pl->knot_ptr[i]), nft = rkt + (double)pl->anc_rank[i] + 1.0;
        double kalg = 0, kpad = 0;
        for (int c = pl->child_ptr[i]; c < pl->child_ptr[i + 1]; ++c) {
            const int ch = pl->child_list[c];                  // a parent of leaves
            for (int c2 = pl->child_ptr[ch]; c2 < pl->child_ptr[ch + 1]; ++c2) {
                const int lt = pl->leaf_slot[pl->child_list[c2]];
                const int nop = pl->leaf_nop[lt];
                if (!nop) continue;
                double* ut = leaf_Ut(pl, lt) + (size_t)lv.cw * nop;      // rows of the ancestors of `ch`
                gsegs.push_back(GemmSeg{ut, ut, nop, nop, nop, 0});
                kalg += d.nobs[lt]; kpad += nop;
            }
            double* zt = lv.F_of(pl->node_slot[ch]) + (size_t)lv.cw * lv.ldf;
            gsegs.push_back(GemmSeg{zt, zt, lv.ldf, lv.ldf, lv.cw, 1});
            kalg += (double)(pl->knot_ptr[ch + 1] - pl->knot_ptr[ch]); kpad += lv.cw;
        }
        gwhere[sidx] = {first, (int)(gsegs.size() - first)};
        pl->fl_grand_syrk += Work(nft * nft * kalg, (double)lg.nf * lg.nf * kpad, 8.0 * (lg.nf * kpad + 0.5 * lg.nf * (lg.nf + 1)));
    }
    pl->grandSegs.upload(gsegs);
    std::vector<GemmProb> gp(lg.nodes.size());
    for (size_t sidx = 0; sidx < lg.nodes.size(); ++sidx) {
        GemmProb g{};
        g.C = lg.F_of(sidx); g.ldc = lg.nf; g.M = lg.nf; g.N = lg.nf; g.lower = 1;
        g.segs = pl->grandSegs.p + gwhere[sidx].first; g.nseg = gwhere[sidx].second; g.diag_one = lg.cw;
        if (g.nseg == 0) { g.K = 0; g.A = g.B = pl->W.p; }
        gp[sidx] = g;
    }
    pl->gGrandSyrk.upload(gp);
    // k_syrk_blk keeps the K steps of a problem as a table in LDS: SB_MAXST segments / 16-column steps at most
    pl->grand_syrk_blk_ok = pl->grand_syrk_dma_ok = (lg.nf % 16) == 0;
    for (size_t sidx = 0; sidx < lg.nodes.size() && pl->grand_syrk_blk_ok; ++sidx) {
        long steps = 0;
        for (int k = 0; k < gwhere[sidx].second; ++k) steps += gsegs[gwhere[sidx].first + k].K / 16;
        if (gwhere[sidx].second == 0 || gwhere[sidx].second > SB_MAXST || steps > SB_MAXST) pl->grand_syrk_blk_ok = false;
        if (gwhere[sidx].second == 0 || gwhere[sidx].second > SD_MAXST || steps > SD_MAXST) pl->grand_syrk_dma_ok = false;
    }
}

// LDS of k_parent_front_pair: the larger of its two uses of one region - two unpadded stages and the table of max_steps 16-column
// steps in the K loop, the panel tiles and inverted diagonal blocks afterwards
static size_t parent_pair_lds(long nf, long cwt, long max_steps) {
    const long nt = nf / 16, npanel = cwt * nt - cwt * (cwt - 1) / 2;
    const size_t kloop = (size_t)(2 * nf * 128) + (size_t)max_steps * sizeof(PpStep);
    const size_t fact = (size_t)(npanel + cwt) * FT_SZ * sizeof(double);
    return std::max(kloop, fact);
}

// the instantiation of k_parent_front_pair whose slots hold a front of nt row tiles with cwt panel columns (pp_tile's deal: 4 NPAN
// places for panel tiles, the other slots for the rest), 0 if neither does
static int parent_pair_nacc(long nt, long cwt) {
    const long ntiles = nt * (nt + 1) / 2, npanel = cwt * nt - cwt * (cwt - 1) / 2;
    if (nt > 2 * PP_MAXPC || ntiles > 92) return 0;
    for (int nacc : {17, 23}) {
        const long npan = pp_npan(nacc);
        if (ntiles - std::min(npanel, 4 * npan) <= 4 * (nacc - npan)) return nacc;
    }
    return 0;
}

// the parents' fronts for k_parent_front (SYRK + factorisation in one launch), where the front fits its registers and LDS
static void build_parent_front(mra_plan* pl, const std::vector<GemmSeg>& segs, const SegRanges& where) {
    const LevelData& lv = pl->lev[pl->NL - 1];
    std::vector<FrontProb> fr(lv.nodes.size());
    for (size_t sidx = 0; sidx < lv.nodes.size(); ++sidx)
        fr[sidx] = FrontProb{lv.F_of(sidx), lv.invF_of(sidx), lv.nf, lv.cwt, lv.nodes[sidx], (int)where[sidx].first, where[sidx].second};
    pl->gParentFront.upload(fr);
    const long nt = lv.nf / 16, ntiles = nt * (nt + 1) / 2;
    const long npanel = lv.cwt * nt - lv.cwt * (lv.cwt - 1) / 2;
    pl->parent_front_lds = (size_t)(2 * lv.nf * PF_LD + (npanel + lv.cwt) * FT_SZ) * sizeof(double);
    pl->parent_front_nacc = ntiles <= 16 ? 2 : (ntiles <= 32 ? 4 : (ntiles <= 64 ? 8 : (ntiles <= 96 ? 12 : 0)));
    if (pl->parent_front_lds > 160 * 1024 || lv.panel_only) pl->parent_front_nacc = 0;
    // parent_pair_ok: the same fronts in four-wave workgroups, two to a CU (at most 64 KB of LDS each)
    long max_steps = 0, all_steps = 0;
    for (size_t sidx = 0; sidx < lv.nodes.size(); ++sidx) {
        long steps = 0;
        for (int k = 0; k < where[sidx].second; ++k) steps += (segs[where[sidx].first + k].K + 15) / 16;
        max_steps = std::max(max_steps, steps);
        all_steps += steps;
    }
    pl->parent_pair_lds = parent_pair_lds(lv.nf, lv.cwt, max_steps);
    pl->parent_pair_nacc = (lv.panel_only || pl->parent_pair_lds > 64 * 1024) ? 0 : parent_pair_nacc(nt, lv.cwt);
    // its empty accumulator slots run one more tile per K step (four 16 x 16 x 4 MFMAs): executed, not algorithmic, work
    pl->parent_pair_idle_exec = !pl->parent_pair_nacc ? 0.0 : (double)all_steps * (double)(4 * pl->parent_pair_nacc - ntiles) * 4.0 * (2.0 * 16 * 16 * 4);
}

// shape-regular trees: the segmented products of the leaves' parents and, with lowrank_parent, of the grandparents
static void build_parent_products(mra_plan* pl, const LeafDescs& d) {
    pl->parent_syrk = false;
    if (!pl->shape_regular || pl->NL < 1) return;
    std::vector<GemmSeg> segs;
    SegRanges where;
    build_parent_syrk(pl, segs, where);
    pl->fl_parent_panel = pl->fl_grand_syrk = Work();
    if (pl->lowrank_parent && pl->NL >= 2) {
        build_parent_panels(pl, d, segs, where);
        build_grand_syrk(pl, d);
    }
    build_parent_front(pl, segs, where);
}

// leaves with more than 192 observations: right-looking blocked factorisation, 64 columns per step (mra_plan::gBigPanel)
static void build_big_panels(mra_plan* pl, const LeafDescs& d) {
    const size_t nl = pl->leaf_nodes.size();
    for (int v = 0; v < 2; ++v) { pl->gBigPanel[v].clear(); pl->gBigTrail[v].clear(); pl->bigM[v].clear(); pl->bigN[v].clear(); }
    if (pl->leaf_max_nop / 16 <= LEAF_MAX_TILES) return;
    const int NBT = 4;                                        // column tiles per step
    const int nsteps = (pl->leaf_max_nop / 16 + NBT - 1) / NBT;
    for (int v = 0; v < 2; ++v) {
        pl->gBigPanel[v].resize(nsteps); pl->gBigTrail[v].resize(nsteps);
        pl->bigM[v].assign(nsteps, 0); pl->bigN[v].assign(nsteps, 0);
        for (int st = 0; st < nsteps; ++st) {
            std::vector<PanelProb> pp(nl);
            std::vector<GemmProb> gg(nl);
            for (size_t t = 0; t < nl; ++t) {
                const PanelProb& full = v == 0 ? d.chol_full[t] : d.chol_lik[t];
                const int ntl = full.ne, c0 = st * NBT;               // column tiles of this leaf, first tile of the step
                const int ne = std::max(0, std::min(NBT, ntl - c0));
                const long nop = full.ld;
                PanelProb q = full;
                q.P = full.P + (size_t)c0 * 16 * nop + (size_t)c0 * 16;
                q.invd = full.invd + (size_t)c0 * 256;
                q.ht = ne > 0 ? full.ht - c0 : 0;
                q.ne = ne;
                pp[t] = q;
                GemmProb g{};
                const int c1 = c0 + ne;
                g.M = ne > 0 ? (full.ht - c1) * 16 : 0;
                g.N = ne > 0 ? (ntl - c1) * 16 : 0;
                if (g.N <= 0 || g.M <= 0) { g.M = 0; g.N = 0; }
                g.K = ne * 16;
                g.A = full.P + (size_t)c1 * 16 * nop + (size_t)c0 * 16; g.lda = nop;
                g.B = g.A; g.ldb = nop;
                g.C = full.P + (size_t)c1 * 16 * nop + (size_t)c1 * 16; g.ldc = nop;
                gg[t] = g;
                pl->bigM[v][st] = std::max<long>(pl->bigM[v][st], g.M);
                pl->bigN[v][st] = std::max<long>(pl->bigN[v][st], g.N);
            }
            pl->gBigPanel[v][st].upload(pp);
            pl->gBigTrail[v][st].upload(gg);
        }
    }
}

// Does a leaf of ta observation tiles go before one of tb in the small-first order?  The small ones (at most LEAF_SMALL_TILES tiles)
// before the others; longest_first: inside either part the one with more tiles - a leaf's Cholesky, row solve and residual product all
// take time in proportion to its tiles, and a launch that hands out its longest workgroups first ends with the shortest tail.
// False both ways for leaves that tie: a stable sort keeps them in leaf order.
static inline bool leaf_goes_before(int ta, int tb, bool longest_first) {
    const bool sa = ta <= LEAF_SMALL_TILES, sb = tb <= LEAF_SMALL_TILES;
    if (sa != sb) return sa;
    return longest_first && ta > tb;
}

// The small-first order of the leaves: those with at most LEAF_SMALL_TILES observation tiles (their count: the return value), then
// the others; inside each group by decreasing tile count (MRA_OPT_LEAF_ORDER, read here: it takes effect with the next
// mra_plan_set_obs), leaf order among equals - without the option leaf order throughout.  EVERY small-first list is this one
// permutation - gLeafCholSorted, the *Plain* row-solve lists, gLeafSolve, gLeafSolveHalf, gLeafUpdatePlain: the kernels index one list
// with a position taken from another, and mra_run_all steps into each by the number of small leaves.  (leaf_upd_dev is indexed by leaf.)
static size_t order_small_first(const mra_plan* pl, std::vector<size_t>& order) {
    const size_t nl = pl->leaf_nop.size();
    order.resize(nl);
    for (size_t t = 0; t < nl; ++t) order[t] = t;
    const bool longest_first = pl->leaf_longest_first;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return leaf_goes_before(pl->leaf_nop[a] / 16, pl->leaf_nop[b] / 16, longest_first); });
    size_t n_small = 0;
    while (n_small < nl && pl->leaf_nop[order[n_small]] / 16 <= LEAF_SMALL_TILES) ++n_small;
    return n_small;
}
template <class T>
static std::vector<T> in_order(const std::vector<T>& v, const std::vector<size_t>& order) {
    std::vector<T> out(order.size());
    for (size_t k = 0; k < order.size(); ++k) out[k] = v[order[k]];
    return out;
}

// the per-leaf descriptors to the device, in leaf order (and the C-only factorisations small first as well; with resid_longest_first
// the residual products of the device kernels too: every problem carries all its operands, so the list may be dealt in any order)
static void upload_leaf_descriptors(mra_plan* pl, const LeafDescs& d, const std::vector<size_t>& order) {
    pl->hLeafResid = d.resid; pl->hLeafResidLik = d.resid_lik; pl->leaf_order = order; pl->leaf_nobs_host = d.nobs;
    pl->gLeafResidLik.upload(d.resid_lik);
    pl->gLeafResidSorted.upload(pl->resid_longest_first ? in_order(d.resid, order) : std::vector<GemmProb>());
    pl->gLeafResidLikSorted.upload(pl->resid_longest_first ? in_order(d.resid_lik, order) : std::vector<GemmProb>());
    pl->gLeaf.upload(d.lp); pl->gLeafResid.upload(d.resid); pl->gLeafSyrk.upload(d.syrk); pl->gLeafUpdate.upload(d.upd);
    pl->gLeafCholFull.upload(d.chol_full); pl->gLeafCholLik.upload(d.chol_lik); pl->gLeafCholC.upload(d.chol_c);
    // (k_chol_tiles<8, 4> at three workgroups per CU for the small matrices, then the few larger ones)
    pl->hLeafCholSorted = in_order(d.chol_c, order);
    pl->gLeafCholSorted.upload(pl->hLeafCholSorted);
    pl->hLeaf = d.lp;
}

// The row solves: in leaf order (level-by-level path), and small first for the fused path - most leaves are small and get the
// LEAF_SMALL_TILES instance (fewer registers, two workgroups per CU), the few larger ones the TRSM2_MAX_NT instance.  "G": the Ut rows
// gathered from W by the row solve itself; plain: scattered there by the row cascade.
static void build_leaf_row_solves(mra_plan* pl, const LeafDescs& d, const std::vector<size_t>& order, size_t n_small) {
    pl->gLeafTrsmFull.upload(d.trsm_full); pl->gLeafTrsmLik.upload(d.trsm_lik);
    const std::vector<Trsm2Prob> tfg = in_order(d.trsm_full, order), tkg = in_order(d.trsm_lik, order);
    std::vector<Trsm2Prob> tf = tfg, tk = tkg;
    for (auto& e : tf) e.gtiles = 0;
    for (auto& e : tk) e.gtiles = 0;
    pl->trsm_small_nt = pl->trsm_small_tiles_full = pl->trsm_small_tiles_lik = 0;
    for (size_t k = 0; k < n_small; ++k) {
        pl->trsm_small_nt = std::max(pl->trsm_small_nt, tf[k].nt);
        pl->trsm_small_tiles_full = std::max(pl->trsm_small_tiles_full, tf[k].ntiles);
        pl->trsm_small_tiles_lik = std::max(pl->trsm_small_tiles_lik, tk[k].ntiles);
    }
    pl->gLeafTrsmFullPlain.upload(tf); pl->gLeafTrsmLikPlain.upload(tk);
    pl->gLeafTrsmFullPlainG.upload(tfg); pl->gLeafTrsmLikPlainG.upload(tkg);
    pl->hLeafTrsmFullPlainG = tfg;
}

// fused row solve + update (k_leaf_solve_update) for the small leaves, whole and in two halves, and the plain update of the others,
// all small first; per leaf in leaf order, its first row and whether that kernel takes it
static void build_leaf_solve_lists(mra_plan* pl, const LeafDescs& d, const std::vector<size_t>& order, size_t n_small) {
    const size_t nl = order.size();
    std::vector<LeafSolveProb> sp(nl);
    int nat_max = 0;
    for (size_t k = 0; k < nl; ++k) {
        const size_t t = order[k];
        const int i = pl->leaf_nodes[t];
        const int m = pl->node_level[i];
        const int na = pl->na[m], a0 = pl->asuf[m], nop = pl->leaf_nop[t];
        const long r0 = pl->row0[i], nr = pl->row1[i] - r0;
        LeafSolveProb q{};
        q.L = leaf_C(pl, t); q.invd = pl->leafInv.p + pl->leaf_ioff[t];
        q.V = leaf_V(pl, t); q.Ut = leaf_Ut(pl, t);
        q.Wr = pl->W.p + r0 * pl->ldw + a0; q.var = pl->var.p + r0;
        q.ldL = nop; q.ldx = nop; q.ldw = pl->ldw;
        q.nt = nop / 16; q.nrt = (int)(nr / 16); q.nat = na / 16; q.zt = (na - MRA_YB) / 16;
        sp[k] = q;
        if (k < n_small) nat_max = std::max(nat_max, q.nat);
    }
    pl->gLeafSolve.upload(sp);
    pl->gLeafUpdatePlain.upload(in_order(d.upd, order));
    std::vector<LeafSolveProb> half;
    pl->hLeafSolveHalfPos.clear();
    for (size_t k = 0; k < n_small; ++k) {
        const LeafSolveProb& q = sp[k];
        const int h0 = (q.nrt + 1) / 2;
        for (int part = 0; part < 2; ++part) {
            LeafSolveProb h = q;
            const int t0 = part ? h0 : 0, t1 = part ? q.nrt : h0;
            if (t1 <= t0) continue;
            h.V = q.V + (size_t)t0 * 16 * q.ldx; h.Wr = q.Wr + (size_t)t0 * 16 * q.ldw; h.var = q.var + (size_t)t0 * 16; h.nrt = t1 - t0;
            half.push_back(h);
            pl->hLeafSolveHalfPos.push_back(k);
        }
    }
    pl->n_leaf_solve_half = half.size();
    pl->gLeafSolveHalf.upload(half);
    pl->hLeafSolve = sp; pl->hLeafSolveHalf = half;
    std::vector<long> lr0(nl);
    std::vector<unsigned char> lup(nl, 0);
    for (size_t t = 0; t < nl; ++t) lr0[t] = pl->row0[pl->leaf_nodes[t]];
    for (size_t k = 0; k < n_small; ++k) lup[order[k]] = 1;
    pl->leaf_row0_dev.upload(lr0); pl->leaf_upd_dev.upload(lup);
    const int nts = pl->trsm_small_nt;
    pl->leaf_solve_lds = (size_t)((nts * (nts - 1) / 2 + nts) * FT_SZ + 2 * nat_max * 16 * LG_LD) * sizeof(double);
    pl->leaf_solve_ok = n_small > 0 && nat_max <= 13 && nat_max > 0 && pl->leaf_solve_lds <= 160 * 1024 && pl->leaf_max_rows >= 128;
}

// The row cascade's workgroups over the tiles of the leaves behind the small ones in `order` (those of more than LEAF_SMALL_TILES
// observation tiles): what a pass that keeps the last pass's W re-runs, because the plain update beside LeafUpdate::InCascade rewrote
// those leaves' rows.  One leaf per workgroup run (a workgroup stages ONE chain), as many tiles per workgroup as either form of the
// cascade walks (stage-all: any number, 8 = one per wave; else one tile per wave of its cascade_wpw).  If the standing dirty mark was
// set under the old mask its list is put aside (stale) for that re-run.
static void build_big_leaf_tiles(mra_plan* pl, const std::vector<size_t>& order, size_t n_small) {
    typedef mra_plan::PriorKeep K;
    if (pl->keep.dirty == K::Dirty::Oversized && !pl->stale.n_wg) pl->stale.swap(pl->big);
    pl->big.n_wg = pl->big.n_tiles = 0;
    if (!pl->regular || n_small >= order.size()) return;
    const size_t nl = pl->leaf_nodes.size();
    std::vector<long> first(nl + 1, 0);                      // a leaf's first tile in ft_row0 (build_cascade_tiles: leaves in order)
    for (size_t t = 0; t < nl; ++t) first[t + 1] = first[t] + (pl->row1[pl->leaf_nodes[t]] - pl->row0[pl->leaf_nodes[t]]) / 16;
    const long per_wg = pl->cascade_stage_all ? 8 : pl->cascade_wpw;
    std::vector<long> wg0;
    std::vector<int> wgn;
    for (size_t k = n_small; k < order.size(); ++k) {
        const size_t t = order[k];
        for (long a = first[t]; a < first[t + 1]; a += per_wg) { wg0.push_back(a); wgn.push_back((int)std::min(per_wg, first[t + 1] - a)); }
        pl->big.n_tiles += first[t + 1] - first[t];
    }
    pl->big.n_wg = (long)wg0.size();
    pl->big.wg0.upload(wg0); pl->big.wgn.upload(wgn);
}

static void build_leaf(mra_plan* pl, const double* y) {
    PlanTrace tr("build_leaf");
    ArenaScope arena(&pl->arena);
    pl->cphantom_valid = false;
    pl->resid_lists = pl->resid_refused = false;       // the kept residual's descriptors point into the panels as well
    pl->slv.valid = false; pl->slv.built = false;      // mra_solve's descriptors point into the leaves' panels
    pl->cov.built = false;                             // mra_cov_apply's read the solver's level offsets
    pl->sit.built = false;                             // mra_predict_sites' read the solver's leaf descriptors
    LeafDescs d;
    build_obs_lists(pl, y, d);
    tr.mark("observation lists");
    pl->panel.alloc(std::max<long>(pl->leaf_poff.back(), 1));
    pl->leafInv.alloc(std::max<long>(pl->leaf_ioff.back(), 1));
    tr.mark("panel allocation");
    build_leaf_descriptors(pl, d);
    tr.mark("leaf descriptors (host)");
    upload_leaf_ut_and_clear_panels(pl);
    tr.mark("panel memset");
    pl->hLeafSyrk = d.syrk;
    build_parent_products(pl, d);
    tr.mark("parent / grandparent descriptors");
    std::vector<size_t> order;
    const size_t n_small = order_small_first(pl, order);
    pl->n_chol_small = pl->n_trsm_small = n_small;      // (PanelProb::ne and Trsm2Prob::nt of a leaf are both its observation tiles)
    upload_leaf_descriptors(pl, d, order);
    build_big_panels(pl, d);
    build_leaf_row_solves(pl, d, order, n_small);
    build_leaf_solve_lists(pl, d, order, n_small);
    build_big_leaf_tiles(pl, order, n_small);
    arena.finish();
    tr.mark("descriptor arena to the device");
}

// ------------------------------------------------------------------------------------------------
//  launch helpers
// ------------------------------------------------------------------------------------------------
// ---- arrays that only the general (level-by-level) kernels read, built when one of those kernels is about to be launched ------
static void ensure_row_leaf(mra_plan* pl) {
    if (pl->row_leaf.p) return;
    std::vector<int> rl(pl->P, -1);
    for (size_t t = 0; t < pl->leaf_nodes.size(); ++t) {
        const int i = pl->leaf_nodes[t];
        for (long p = pl->row0[i]; p < pl->row1[i]; ++p) rl[p] = (int)t;
    }
    pl->row_leaf.upload(rl);
}
static void ensure_tile_lists(mra_plan* pl, int m) {
    LevelData& lv = pl->lev[m];
    if (lv.tile_node.p) return;
    std::vector<int> tnode;
    std::vector<long> trow;
    for (size_t s = 0; s < lv.nodes.size(); ++s) {
        const int i = lv.nodes[s];
        for (long t = pl->row0[i]; t < pl->row1[i]; t += 16) { tnode.push_back((int)s); trow.push_back(t); }
    }
    lv.ntiles = (long)tnode.size();
    lv.tile_node.upload(tnode); lv.tile_row0.upload(trow);
}

template <int EPI>
static void launch_gemm(mra_plan* pl, const GemmProb* probs, size_t nprob, long maxM, long maxN, bool allow_lds = true, bool lower_tri = false) {
    mra_launch_gemm(pl, EPI, probs, nprob, maxM, maxN, allow_lds, lower_tri);
}
template <int EPI>
static void launch_leaf_gemm(mra_plan* pl, const GemmProb* probs, size_t nprob) { mra_launch_leaf_gemm(pl, EPI, probs, nprob); }

static void launch_panel(mra_plan* pl, const PanelProb* probs, size_t nprob, int accumulate = 0) {
    if (!nprob) return;
    hipLaunchKernelGGL(k_panel_chol, dim3((unsigned)nprob), dim3(256), 0, pl->stream, probs, pl->dnode.p, pl->errflag.p, accumulate);
}
// for the calls outside a pass: k_panel_chol with the caller's own log-determinant and error slots (nprob > 0), and the non-leaf
// draws of a block of samples, slot-major into zc (Kn > 0)
void mra_panel_chol(mra_plan* pl, const PanelProb* probs, size_t nprob, double* dn, int* err) {
    hipLaunchKernelGGL(k_panel_chol, dim3((unsigned)nprob), dim3(256), 0, pl->stream, probs, dn, err, 0);
}
void mra_sample_draw(mra_plan* pl, const SampleZ& zs, long Kn, double* zc) {
    hipLaunchKernelGGL(k_sample_draw, dim3((unsigned)((Kn * 16 + 255) / 256)), dim3(256), 0, pl->stream, zs, Kn, zc);
}

// -DMRA_STAMPS (the tools/stamps_*.py builds): some kernels take one more argument, a buffer of per-workgroup clock stamps.  The
// argument lists below end in one of these macros; a default build compiles them to nothing.
#ifdef MRA_STAMPS
// at least n stamps: grown when too small, and then zeroed with the device idle before the kernel that writes it starts
static unsigned long long* stamp_buffer(DevVec<double>& b, size_t n) {
    if (b.n < n) { b.alloc(n); HIP_TRY(mraMemset(b.p, 0, b.n * sizeof(double))); HIP_TRY(hipDeviceSynchronize()); }
    return (unsigned long long*)b.p;
}
#define MRA_TSTAMP_VAL , tst                                            // launch_trsm2
#define MRA_LSTAMP_VAL , (unsigned long long*)pl->kstamps2.p            // k_leaf_solve_update, two workgroups per leaf
#define MRA_LSTAMP_NUL , (unsigned long long*)nullptr                   // ... one per leaf: no stamps
#else
#define MRA_TSTAMP_VAL
#define MRA_LSTAMP_VAL
#define MRA_LSTAMP_NUL
#endif

// row-tile triangular solve with L in LDS; returns false when nt is too large for the LDS path
static bool launch_trsm2(mra_plan* pl, const Trsm2Prob* probs, size_t nprob, int nt, long max_tiles, int tiles_per_wg) {
    if (!pl->prepare_only && (!nprob || max_tiles <= 0 || nt <= 0)) return true;
    if (nt > TRSM2_MAX_NT) return false;
    ensure_big_lds(pl, {(const void*)k_trsm_rows2<2>, (const void*)k_trsm_rows2<4>, (const void*)k_trsm_rows2<LEAF_SMALL_TILES>, (const void*)k_trsm_rows2<TRSM2_MAX_NT>});
    if (pl->prepare_only) return true;
    const size_t lds = (size_t)(nt * (nt - 1) / 2 + nt) * 2048 + (size_t)nt * 16 * sizeof(int);      // L image + the Ut gather list
    const unsigned gx = (unsigned)((max_tiles + tiles_per_wg - 1) / tiles_per_wg);
    const unsigned tb = 512;
#ifdef MRA_STAMPS
    // the last big launch wins the buffer (tools/stamps_trsm.py reads it after a pass)
    unsigned long long* tst = (nprob >= 1024 && max_tiles <= 64) ? stamp_buffer(pl->tstamps, nprob * 64 * 8) : nullptr;
#endif
    for (size_t off = 0; off < nprob; off += 65535) {
        dim3 grid(gx, (unsigned)std::min<size_t>(65535, nprob - off));
        if (nt <= 2) hipLaunchKernelGGL((k_trsm_rows2<2>), grid, dim3(tb), lds, pl->stream, probs + off, tiles_per_wg MRA_TSTAMP_VAL);
        else if (nt <= 4) hipLaunchKernelGGL((k_trsm_rows2<4>), grid, dim3(tb), lds, pl->stream, probs + off, tiles_per_wg MRA_TSTAMP_VAL);
        else if (nt <= LEAF_SMALL_TILES) hipLaunchKernelGGL((k_trsm_rows2<LEAF_SMALL_TILES>), grid, dim3(tb), lds, pl->stream, probs + off, tiles_per_wg MRA_TSTAMP_VAL);
        else hipLaunchKernelGGL((k_trsm_rows2<TRSM2_MAX_NT>), grid, dim3(tb), lds, pl->stream, probs + off, tiles_per_wg MRA_TSTAMP_VAL);
    }
    return true;
}

// row solve of all rows of level m's nodes: launch_trsm2, or k_trsm_rows where the level's block is too wide for it.  The prior and the
// posterior solve differ in their descriptor lists and in var (the posterior one subtracts the solved rows' squares from it)
static void launch_level_row_solve(mra_plan* pl, int m, const Trsm2Prob* probs2, const TrsmNode* nodes, double* var) {
    LevelData& lv = pl->lev[m];
    if (launch_trsm2(pl, probs2, lv.nodes.size(), lv.cwt, lv.max_tiles, 32)) return;
    ensure_tile_lists(pl, m);
    hipLaunchKernelGGL(k_trsm_rows, dim3((unsigned)((lv.ntiles + 3) / 4)), dim3(256), 0, pl->stream, nodes, lv.tile_node.p, lv.tile_row0.p,
                       lv.ntiles, pl->W.p, (long)pl->ldw, lv.c0, var);
}

// k_parent_front<nacc>, one workgroup per front (nacc: 2, 4, 8, anything else 12); pair: k_parent_front_pair<17|23> on the same
// descriptors, 256 threads, lds = parent_pair_lds
static void launch_parent_front(mra_plan* pl, int nacc, size_t nprob, size_t lds, const FrontProb* probs, bool pair = false) {
    ensure_big_lds(pl, {(const void*)k_parent_front<2>, (const void*)k_parent_front<4>, (const void*)k_parent_front<8>, (const void*)k_parent_front<12>,
                        (const void*)k_parent_front_pair<17>, (const void*)k_parent_front_pair<23>});
    const dim3 grid((unsigned)nprob);
    if (pair) {
        if (nacc == 17) hipLaunchKernelGGL(k_parent_front_pair<17>, grid, dim3(256), lds, pl->stream, probs, pl->parentSegs.p, pl->dnode.p, pl->errflag.p);
        else hipLaunchKernelGGL(k_parent_front_pair<23>, grid, dim3(256), lds, pl->stream, probs, pl->parentSegs.p, pl->dnode.p, pl->errflag.p);
        return;
    }
    switch (nacc) {
        case 2: hipLaunchKernelGGL(k_parent_front<2>, grid, dim3(512), lds, pl->stream, probs, pl->parentSegs.p, pl->dnode.p, pl->errflag.p); break;
        case 4: hipLaunchKernelGGL(k_parent_front<4>, grid, dim3(512), lds, pl->stream, probs, pl->parentSegs.p, pl->dnode.p, pl->errflag.p); break;
        case 8: hipLaunchKernelGGL(k_parent_front<8>, grid, dim3(512), lds, pl->stream, probs, pl->parentSegs.p, pl->dnode.p, pl->errflag.p); break;
        default: hipLaunchKernelGGL(k_parent_front<12>, grid, dim3(512), lds, pl->stream, probs, pl->parentSegs.p, pl->dnode.p, pl->errflag.p); break;
    }
}

// Cholesky of the nl leaves' C blocks where every one fits (LeafChol but BigPanels).  k_chol_tiles: one workgroup per matrix, tiles in
// registers, next diagonal block factorised beside the trailing update; k_chol_wave: one wave per matrix
// (TilesSplit is two launches: `part` picks the small leaves', the others', or both)
enum class LeafPart { All, Small, Rest };
// (out of place - resid_out_of_place - k_chol_tiles reads the kept C0 and puts the noise on its diagonal itself: the scalar, or the vector)
static bool resid_out_of_place(const mra_plan* pl, const PassRoute& r);
static void launch_leaf_chol(mra_plan* pl, const PassRoute& r, size_t nl, LeafPart part = LeafPart::All) {
    const size_t ns = pl->n_chol_small;      // (gLeafCholSorted: the leaves of at most LEAF_SMALL_TILES tiles first)
    const PanelProb* list = resid_out_of_place(pl, r) ? pl->kLeafCholSorted.p : pl->gLeafCholSorted.p;
    const double R = pl->noise_on ? 0.0 : pl->R;
    const double* noise = pl->noise_on ? pl->noise.p : nullptr;
    if (r.chol == LeafChol::TilesSplit) {
        if (ns && part != LeafPart::Rest) hipLaunchKernelGGL((k_chol_tiles<8, 4>), dim3((unsigned)ns), dim3(256), 0, pl->stream, list, pl->dnode.p, pl->errflag.p, R, noise);
        if (nl > ns && part != LeafPart::Small) hipLaunchKernelGGL((k_chol_tiles<10, 4>), dim3((unsigned)(nl - ns)), dim3(256), 0, pl->stream, list + ns, pl->dnode.p, pl->errflag.p, R, noise);
    }
    else if (r.chol == LeafChol::TilesOne) hipLaunchKernelGGL((k_chol_tiles<10, 4>), dim3((unsigned)nl), dim3(256), 0, pl->stream, list, pl->dnode.p, pl->errflag.p, R, noise);
    else hipLaunchKernelGGL((k_chol_wave<LEAF_MAX_TILES>), dim3((unsigned)((nl + 3) / 4)), dim3(256), 0, pl->stream, pl->gLeafCholC.p, (int)nl, pl->dnode.p, pl->errflag.p);
}

static double kernel_cov0(const mra_plan* pl) { return pl->kp.amp; }   // C(x,x) of every stationary kernel: amp * 1

// tiles of the likelihood-only row cascade: 16 observed rows each (obs_idx, padded with -1), with their leaf's ancestor chain; one
// workgroup per leaf (or per family of sibling leaves, as the full cascade groups them)
static void ensure_lik_tiles(mra_plan* pl) {
    if (pl->lik_tiles_valid) return;
    const size_t nl = pl->leaf_nodes.size();
    std::vector<int> chains, tleaf, wgn;
    std::vector<long> wg0;
    for (size_t t = 0; t < nl; ++t) {
        const int i = pl->leaf_nodes[t];
        const long nt = (pl->obs_off_host[t + 1] - pl->obs_off_host[t]) / 16;
        if (!nt) continue;
        int ch[8];
        chain_of(pl, i, ch);
        // the kernel stages the chain of a workgroup's FIRST tile for all of its tiles: join only a workgroup with this very chain (leaf
        // t - 1 may own no tile, and the last workgroup then belongs to another family)
        const bool join = pl->cascade_group_siblings && !wg0.empty() && wg0.back() + wgn.back() == pl->obs_off_host[t] / 16 &&
                          std::equal(ch, ch + 8, chains.begin() + wg0.back() * 8);
        if (join) wgn.back() += (int)nt;
        else { wg0.push_back(pl->obs_off_host[t] / 16); wgn.push_back((int)nt); }
        for (long k = 0; k < nt; ++k) { tleaf.push_back((int)t); for (int c = 0; c < 8; ++c) chains.push_back(ch[c]); }
    }
    // (tile numbers are positions in obs_idx / 16: leaves without observations own no tile, so the per-tile arrays are dense)
    pl->n_lik_tiles = (long)tleaf.size(); pl->n_lik_wg = (long)wg0.size();
    pl->lik_chain.upload(chains); pl->lik_leaf.upload(tleaf); pl->lik_wg0.upload(wg0); pl->lik_wgn.upload(wgn);
    pl->lik_tiles_valid = true;
}

// Level-by-level path, likelihood-only passes: W is needed at the observed rows (Ut, C) and at the knots (the deeper levels'
// residual products gather them) - at config 5 60 % of the rows.  The sorted list of such rows, padded to 16 with -1 wherever a
// non-leaf node's row range starts or ends; a node's list is a contiguous piece of it; per level the one-launch prior problems over
// blocks of 512 entries.
static bool ensure_lik_general(mra_plan* pl) {
    if (pl->lik_general_valid) return pl->lik_general_ok;
    pl->lik_general_valid = true;
    pl->lik_general_ok = false;
    for (int m = 0; m < pl->n_levels; ++m) if (!pl->lev[m].nodes.empty() && !pl->lev[m].prior_level_ok) return false;
    std::vector<unsigned char> need(pl->y_finite_host);
    if ((long)need.size() != pl->P) return false;
    for (int i = 0; i < pl->n_nodes; ++i)
        if (!pl->leaf[i]) for (long k = pl->knot_ptr[i]; k < pl->knot_ptr[i + 1]; ++k) need[pl->knot_rows[k]] = 1;
    // the list is cut (padded to 16) wherever a non-leaf node's row range starts or ends, so that every such node's rows are a
    // contiguous, tile-aligned piece of it (regular trees: at the boundaries of the leaves' parents, every 256 rows at config 5; a
    // 64-row leaf with 38 needed rows padded on its own would cost 48; a shard's orphan knot rows above its subtree are cut the same way)
    std::vector<long> cuts;
    for (int i = 0; i < pl->n_nodes; ++i) if (!pl->leaf[i]) { cuts.push_back(pl->row0[i]); cuts.push_back(pl->row1[i]); }
    cuts.push_back(0); cuts.push_back(pl->P);
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    std::vector<int> idx;
    std::vector<long> off(cuts.size(), 0);                   // position in idx of the first list entry at or behind row cuts[c]
    idx.reserve((size_t)pl->P);
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        off[c] = (long)idx.size();
        for (long p = cuts[c]; p < cuts[c + 1]; ++p) if (need[p]) idx.push_back((int)p);
        while (idx.size() % 16) idx.push_back(-1);
    }
    off[cuts.size() - 1] = (long)idx.size();
    if (idx.empty()) return false;
    pl->need_idx.upload(idx);
    const long blk = 512;
    for (int m = 0; m < pl->n_levels; ++m) {
        LevelData& lv = pl->lev[m];
        const size_t nn = lv.nodes.size();
        if (!nn) continue;
        std::vector<GemmProb> fz;
        long rows_needed = 0, rows_all = 0;
        const int Kanc = pl->Ka - lv.a0;
        for (size_t s = 0; s < nn; ++s) {
            const int i = lv.nodes[s];
            const size_t c0 = (size_t)(std::lower_bound(cuts.begin(), cuts.end(), pl->row0[i]) - cuts.begin());
            const size_t c1 = (size_t)(std::lower_bound(cuts.begin(), cuts.end(), pl->row1[i]) - cuts.begin());
            const long o0 = off[c0], o1 = off[c1];
            rows_needed += o1 - o0; rows_all += pl->row1[i] - pl->row0[i];
            for (long b0 = o0; b0 < o1; b0 += blk) {
                GemmProb g{};
                g.A = pl->W.p + lv.a0; g.lda = pl->ldw;
                g.B = pl->W.p + lv.a0; g.ldb = pl->ldw; g.idxB = pl->knot_idx.p + pl->knot_idx_off[i];
                g.C = pl->W.p + lv.c0; g.ldc = pl->ldw;
                g.XA = pl->X.p; g.XB = pl->X.p;
                g.M = (int)std::min(blk, o1 - b0); g.N = lv.cw; g.K = Kanc; g.lower = 0;
                g.idxA = pl->need_idx.p + b0;
                g.solveL = lv.Lp_of(s); g.solveI = lv.invP_of(s); g.var = pl->var.p;
                fz.push_back(g);
            }
        }
        lv.gResidLik.upload(fz);
        lv.lik_share = rows_all > 0 ? (double)rows_needed / (double)rows_all : 1.0;
    }
    pl->lik_general_ok = true;
    return true;
}

// ---- the route of a pass (PassRoute, mra_plan_types.h) ---------------------------------------------------------------------------
static PassPath path_of(const mra_plan* pl) {
    // (MRA_KERNEL_MATERN, mode 4: the fused cascades have no instance of it - DESIGN.md section 23 - so its regular trees take the prior level by level)
    if (pl->regular && pl->use_fused && !pl->host_cov && pl->kp.mode != 4 && pl->kp.mode != 5 && pl->kp.mode != 6) return PassPath::Fused;     // (nor of mode 5, MRA_KERNEL_SUM: section 24, nor of mode 6, MRA_KERNEL_LOCAL: section 25)
    return (pl->regular_hi && pl->use_fused && !pl->host_cov) ? PassPath::Hi : PassPath::Levels;     // (sharded plans too: the walk is per row tile)
}

// Pure: reads the plan, decides, touches nothing.  full_rows: the caller reads W at every row afterwards (mra_sample, mra_solve).
static PassRoute route_for(const mra_plan* pl, uint32_t flags, bool full_rows) {
    PassRoute r;
    const size_t nl = pl->leaf_nodes.size(), two_per_cu = (size_t)(2 * pl->n_cu);
    const int ntl = pl->leaf_max_nop / 16;
    const bool fit = ntl <= LEAF_MAX_TILES, obs = pl->leaf_max_nop > 0;      // every leaf's observation block fits k_chol_wave / the LDS row solve
    r.path = path_of(pl); r.predict = flags & MRA_RUN_PREDICT;
    const bool fused = r.path == PassPath::Fused, pred = r.predict;
    // ---- prior.  Level-by-level: when every level's row solve takes the LDS path and the leaves' solve subtracts |Tt|^2, the variance is
    // accumulated on the way instead of by a pass over all of W at the end
    r.init_yblock = !fused; r.acc_var = !fused && fit;              // (the fused prior cascade writes the y block itself)
    for (int m = 0; m < pl->n_levels; ++m) if (!pl->lev[m].nodes.empty() && pl->lev[m].cwt > TRSM2_MAX_NT) r.acc_var = false;
    r.n_chain = (pl->use_knot_chain && pl->knot_chain_ok && pl->kc_levels >= 2) ? pl->kc_levels : 0;
    r.prior_level = pl->use_prior_level && !pl->host_cov && pl->gemm_lds;
    // likelihood-only passes never need V[S,o]: just C = v_m(o,o) + R I from a small gathered product (the row solve gathers Ut itself, or
    // the row cascade has scattered it), and W at the rows they need only.  Fused: the row cascade walks gathered tiles of OBSERVED rows
    // (the knots had their own pass; 7 of a leaf's 16 tiles at C3).  Level-by-level: the one-launch prior levels walk the observed rows
    // and the knots when every level takes that path (ensure_lik_general's verdict; one not yet known counts as yes: open_pass then has
    // the list built and asks again).
    r.c_only = !pred && !pl->host_cov && pl->gemm_lds && fit && obs;
    const bool rows = r.c_only && !full_rows && pl->use_lik_rows;
    r.lik_rows = fused && rows && pl->cascade_stage_all && !pl->obs_off_host.empty() && pl->obs_off_host.back() > 0;
    r.lik_general = !fused && rows && pl->use_prior_level && (pl->lik_general_ok || !pl->lik_general_valid);
    r.scatter_ut = fit && obs && !pl->ut_gather;
    // ---- leaves.  The leaf-resident kernel pays off for leaves with many rows and a K loop of at least a few chunks; small leaves
    // (config 5: 64 rows, 32 observations) keep the 64x64-tile kernel
    r.leaf_resident = pl->use_leaf_gemm && pl->leaf_max_rows >= 128 && pl->leaf_max_nop >= 64;
    r.c_fix = !obs ? LeafCFix::None : r.c_only ? LeafCFix::InProduct : fit ? LeafCFix::Phantom : LeafCFix::Fill;
    // (round 4, with the blocked factorisation atom: one workgroup per matrix is at least as fast as one wave per matrix at
    //  every shard size - 5.507 / 3.00 / 1.601 / 0.922 ms against 5.528 / 3.00 / 1.621 / 0.959 for 1 / 2 / 4 / 8-way C3 -
    //  so option 11 = 1 (the default) takes it for matrices of five tiles and more at any count; small matrices - config 5:
    //  65536 of at most three tiles - stay on one wave each unless a CU sees at most two of them; 0 forces k_chol_wave)
    if (!fit) r.chol = LeafChol::BigPanels;
    else if (ntl <= 10 && (pl->use_chol_lds == 2 || (pl->use_chol_lds == 1 && (ntl >= 5 || nl <= two_per_cu))))
        r.chol = (pl->n_chol_small == nl || nl > two_per_cu) ? LeafChol::TilesSplit : LeafChol::TilesOne;
    else r.chol = LeafChol::Wave;
    // with the fused row solve + update the small leaves only need their Ut rows solved by the row solve
    // (one 8-wave workgroup per CU: a gain when a CU sees at most two leaves - 1.21 -> 1.13 ms on an eighth of C3 -
    // and a loss from four per CU on - 1.87 -> 1.90 ms on a quarter - where the update rides in the predictive
    // cascade at three workgroups per CU)
    r.solve_fused = fused && pred && nl && fit && pl->use_leaf_solve && pl->leaf_solve_ok && (pl->leaf_solve_mode == 1 || pl->n_trsm_small <= two_per_cu);
    if (fused) {
        const Trsm2Prob* likp = pl->ut_gather ? pl->gLeafTrsmLikPlainG.p : pl->gLeafTrsmLikPlain.p;
        r.trsm_all = pred ? (pl->ut_gather ? pl->gLeafTrsmFullPlainG.p : pl->gLeafTrsmFullPlain.p) : likp;
        r.trsm_small = r.solve_fused ? likp : r.trsm_all;
    } else r.trsm_all = pred ? pl->gLeafTrsmFull.p : pl->gLeafTrsmLik.p;
    // ---- fronts
    r.direct_parent = pl->parent_syrk && pl->reduce_level != pl->NL - 1;
    r.front_fused = pl->use_front_fused;
    r.parent_front = r.direct_parent && pl->use_front_fused && pl->parent_front_nacc > 0;
    r.syrk_blk = pl->use_syrk_blk && pl->grand_syrk_blk_ok; r.syrk_dma = pl->use_syrk_blk == 1 && pl->grand_syrk_dma_ok;
    r.extract_mean = pred && r.path == PassPath::Levels;
    if (!pred || !nl) return r;
    // ---- what only feeds the predictive pass.  In a sharded run it goes to the side stream, so that the front chain and the all-reduce
    // do not queue behind it (on one GPU it buys nothing); with per-kernel timing on it stays on the main stream so
    // that the hipEvent brackets measure one kernel at a time.
    r.side = !pl->ktiming && pl->reduce_level >= 0;
    r.var = r.acc_var ? LeafVar::FinishVar : (!fused || !fit) ? LeafVar::Moments : LeafVar::None;
    // deep 64-wide trees: the update rides in k_predict_hi (leaves of at most four observation tiles, 16 x 16-padded ancestors + y)
    // (a sharded rank keeps the separate product: it runs on the side stream beside the front chain and the all-reduce, whereas
    // k_predict_hi sits behind them on the rank's critical path; option 16 = 2 folds there too, for A/B runs)
    if (r.path == PassPath::Hi && pl->use_hi_fold && (pl->reduce_level < 0 || pl->use_hi_fold == 2) && pl->leaf_max_nop <= 64 &&
        pl->na[pl->NL] == (pl->NL * 4 + 1) * 16) r.update = LeafUpdate::InPredictHi;
    else if (!r.solve_fused && fused && pl->use_pred_update && pl->leaf_solve_ok && fit && pl->na[pl->NL] == (pl->NL * pl->CWT + 1) * 16)
        r.update = LeafUpdate::InCascade;
    else if (r.solve_fused) r.update = (pl->leaf_solve_split == 2 && pl->n_leaf_solve_half) ? LeafUpdate::SolveHalves : LeafUpdate::SolveWhole;
    // (measured: the leaf-resident form wins for the residual - 1.07 vs 1.15 ms at C3 - but not for the update,
    // 1.34-1.39 vs 1.29 ms, whatever the pass structure; MRA_OPT_LEAF_GEMM = 2 selects it for A/B runs)
    else r.update = (r.leaf_resident && pl->leaf_gemm_update) ? LeafUpdate::LeafGemm : LeafUpdate::Gemm;
    return r;
}

// ---- the prior of the last pass (mra_plan::PriorKeep, MRA_OPT_PRIOR_REUSE) ----------------------------------------------------------
// The one invalidation: nothing of the last pass's prior stands.  Called by every set_* that changes what the prior depends on (the
// kernel - on every set_kernel, values are not compared - the locations, the knots, a host covariance block, the reduce level), by every
// option but the three that spare slv.valid, by a pass that fails or is found open, and by every pass off the fused path (its stages
// rewrite W in place).  mra_plan_set_obs is narrower (set_obs); set_noise and the Laplace linearisation keep everything.
static void prior_keep_reset(mra_plan* pl) {
    pl->keep = mra_plan::PriorKeep();
    pl->stale.n_wg = pl->stale.n_tiles = 0;
    pl->rkeep = mra_plan::ResidKeep();       // the leaves' residual is built on the prior
}

// ---- the leaves' residual of the last pass (mra_plan::ResidKeep, MRA_OPT_RESID_REUSE) ------------------------------------------------
// Does this route run its leaf stage OUT OF PLACE - product into the kept buffer, Cholesky and solves reading it?  Pure.  The fused
// path with a device covariance, the Ut rows gathered by the row solve, and k_chol_tiles (either launch form, both halves of the leaf
// fork) - the one factorisation that loads its matrix whole before it stores.  Every other route (k_chol_wave, the big panels, host
// covariance, Hi, Levels, a residual product that is neither the gathered C-only one nor k_leaf_gemm) runs the in-place launch list.
static bool resid_route_eligible(const mra_plan* pl, const PassRoute& r) {
    if (r.path != PassPath::Fused || pl->host_cov || !pl->use_resid_reuse || (pl->dbg & 7) || pl->resid_refused) return false;
    if (!pl->ut_gather || r.scatter_ut || pl->leaf_nodes.empty()) return false;
    if (r.chol != LeafChol::TilesOne && r.chol != LeafChol::TilesSplit) return false;
    return r.c_only ? r.c_fix == LeafCFix::InProduct : (r.leaf_resident && r.c_fix == LeafCFix::Phantom);
}
// ... and has the buffer and its descriptor lists (run_leaf_product asks for them first): what every launch of the leaf stage reads
static bool resid_out_of_place(const mra_plan* pl, const PassRoute& r) { return pl->resid_lists && resid_route_eligible(pl, r); }

// What the residual product of a pass does, decided from the plan's record and the route; read at the launch (run_leaf_product), where
// the record is updated too.  Pure, like prior_step_for.  Keep: the record was left by this route's own product form, under this mask,
// on this prior (a pass whose prior stage ran its knots has reset the record before this is read).
enum class ResidStep { InPlace, Run, Keep };
static ResidStep resid_step_for(const mra_plan* pl, const PassRoute& r) {
    typedef mra_plan::ResidKeep K;
    if (!resid_out_of_place(pl, r)) return ResidStep::InPlace;
    const K::Form form = r.c_only ? K::Form::COnly : K::Form::Full;
    return (pl->keep.knots_valid && pl->rkeep.resid == form) ? ResidStep::Keep : ResidStep::Run;
}

// The kept buffer [per leaf: C0 ; V0] and the lists that point into it, for the mask of the last build_leaf.  A refused allocation
// clears the error and marks the plan: its passes run in place until the next mra_plan_set_obs asks again.
static void ensure_resid_lists(mra_plan* pl) {
    if (pl->resid_lists || pl->resid_refused) return;
    const size_t nl = pl->leaf_nodes.size();
    pl->leaf_koff.assign(nl + 1, 0);
    for (size_t t = 0; t < nl; ++t) {
        const long nop = pl->leaf_nop[t], nr = pl->row1[pl->leaf_nodes[t]] - pl->row0[pl->leaf_nodes[t]];
        pl->leaf_koff[t + 1] = pl->leaf_koff[t] + (nop + nr) * nop;
    }
    const size_t need = (size_t)std::max<long>(pl->leaf_koff.back(), 1);
    if (pl->resid.n != need) {
        pl->resid.release();
        pl->rkeep = mra_plan::ResidKeep();
        double* p = nullptr;
        if (mraMalloc((void**)&p, need * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); pl->resid_refused = true; return; }
        pl->resid.p = p; pl->resid.n = need;
    }
    auto C0 = [&](size_t t) { return pl->resid.p + pl->leaf_koff[t]; };
    auto V0 = [&](size_t t) { return C0(t) + (size_t)pl->leaf_nop[t] * pl->leaf_nop[t]; };
    const std::vector<size_t>& order = pl->leaf_order;
    std::vector<GemmProb> full = pl->hLeafResid, lik = pl->hLeafResidLik;
    std::vector<LeafProb> lp = pl->hLeaf;
    for (size_t t = 0; t < nl; ++t) {
        full[t].C = V0(t); full[t].C2 = C0(t); full[t].diag_add = 0.0;      // v(o,o) + 0, as while a noise vector is set
        lik[t].C = C0(t); lik[t].diag_add = 0.0;
        lp[t].Pn = C0(t);
    }
    pl->kLeafResid.upload(pl->gLeafResidSorted.n ? in_order(full, order) : full);
    pl->kLeafResidLik.upload(pl->gLeafResidLikSorted.n ? in_order(lik, order) : lik);
    pl->kLeaf.upload(lp);
    std::vector<PanelProb> ch = pl->hLeafCholSorted;
    std::vector<Trsm2Prob> ts = pl->hLeafTrsmFullPlainG;
    std::vector<LeafSolveProb> sp = pl->hLeafSolve, half = pl->hLeafSolveHalf;
    for (size_t k = 0; k < nl; ++k) {
        const size_t t = order[k];
        ch[k].src = C0(t); ch[k].obs = pl->obs_idx.p + pl->obs_off_host[t]; ch[k].n_obs = pl->leaf_nobs_host[t];
        ts[k].src = V0(t); ts[k].ldsrc = pl->leaf_nop[t];
        sp[k].V = V0(t);
    }
    for (size_t h = 0; h < half.size(); ++h) {
        const size_t k = pl->hLeafSolveHalfPos[h];
        half[h].V = sp[k].V + (half[h].V - pl->hLeafSolve[k].V);                // the same row tiles of V0
    }
    pl->kLeafCholSorted.upload(ch); pl->kLeafTrsmFullPlainG.upload(ts);
    pl->kLeafSolve.upload(sp); pl->kLeafSolveHalf.upload(half);
    pl->resid_lists = true;
}

// What the prior stage of a fused pass launches, decided from the plan's record and the route; read at the launch (run_prior_fused).
// Pure, like route_for and front_step_for, and like leaf_fork no PassRoute field: the route read-back does not show it.
enum class PriorRows { RunAll, KeepAll, KeepRerunDirty };      // the row cascade in full / nothing but the refresh / the refresh + the dirty leaves' tiles
struct PriorStep { bool run_knots = true; PriorRows rows = PriorRows::RunAll; };
static PriorStep prior_step_for(const mra_plan* pl, const PassRoute& r) {
    typedef mra_plan::PriorKeep K;
    PriorStep s;
    const K& k = pl->keep;
    if (r.path != PassPath::Fused || pl->host_cov || !pl->use_prior_reuse || (pl->dbg & 7) || !k.knots_valid) return s;
    s.run_knots = false;
    if (r.scatter_ut) return s;      // (MRA_OPT_UT_GATHER off: the row cascade also scatters the leaves' Ut rows, which every pass factorises in place)
    // a pass that reads W at every row (predict, full_rows) takes nothing less; a lik_rows pass also what the last one left at its mask's rows
    const bool have = (k.rows == K::Rows::All && k.var_valid) || (r.lik_rows && k.rows == K::Rows::Observed && k.dirty == K::Dirty::Clean);
    if (!have || k.dirty == K::Dirty::All) return s;
    s.rows = k.dirty == K::Dirty::Clean ? PriorRows::KeepAll : PriorRows::KeepRerunDirty;
    return s;
}

// ---- prior of a regular tree (PassPath::Fused): per level a tiny knot pass (knot rows cascade -> kInv -> Cholesky), then ONE cascade
// over all leaf row tiles that writes W once ----------------------------------------------------------------------------------------
// what every launch of the fused prior takes: the levels' knots and factors, X and W
static CascadeArgs prior_cascade_base(const mra_plan* pl) {
    CascadeArgs base{};
    base.ycol = -1;
    for (int m = 0; m < pl->NL; ++m) {
        base.lev[m].kx = pl->fl[m].kx.p; base.lev[m].kvalid = pl->fl[m].kvalid.p; base.lev[m].Wk = pl->fl[m].Wk.p;
        base.lev[m].L = pl->lev[m].Lp.p; base.lev[m].invd = pl->lev[m].invP.p;
        base.coff[m] = pl->coff[m];
    }
    base.X = pl->X.p; base.W = pl->W.p; base.ldw = pl->ldw;
    return base;
}

// leaves every level's Wk, prior factor Lp and inverted diagonal blocks: levels [0, n_chain) in one k_knot_chain launch, one launch each below
static void run_prior_fused_knots(mra_plan* pl, const CascadeArgs& base) {
    const int n_chain = pl->route.n_chain;
    if (n_chain) {
        Work fl;
        for (int m = 0; m < n_chain; ++m) fl += pl->lev[m].fl_pchol;
        KTimer kt(pl, KF_PRIOR_CHOL, fl);
        KnotChainArgs ka{};
        for (int m = 0; m < n_chain; ++m) {
            ka.lev[m] = base.lev[m];
            ka.node_base[m] = (int)pl->level_ptr[m];
        }
        ka.chain = pl->kc_chain.p; ka.ownmask = pl->kc_ownmask.p; ka.knots = pl->kc_knots.p; ka.nl = n_chain; ka.err = pl->errflag.p;
#ifdef MRA_STAMPS
        ka.stamps = stamp_buffer(pl->kstamps, pl->lev[n_chain - 1].nodes.size() * 64);
#endif
        launch_knot_chain(pl, ka);
    }
    for (int m = n_chain; m < pl->NL; ++m) {
        // one launch per level: knot rows cascade -> Wk, kInv, Cholesky factor, inverted diagonal blocks
        LevelData& lv = pl->lev[m];
        KTimer kt(pl, KF_PRIOR_CHOL, lv.fl_pchol);
        CascadeArgs ar = base;
        ar.knot_mode = 1; ar.mlast = m - 1; ar.n_wg = pl->fl[m].n_kwg; ar.knot_threads = pl->fl[m].k_threads;
        ar.wg_tile0 = pl->fl[m].kt_wg0.p; ar.wg_ntiles = pl->fl[m].kt_wgn.p;
        ar.tile_rows = pl->fl[m].kt_rows.p; ar.tile_chain = pl->fl[m].kt_chain.p; ar.tile_knot0 = pl->fl[m].kt_knot0.p;
        ar.Wk_out = pl->fl[m].Wk.p;
        ar.Lp_out = lv.Lp.p; ar.invd_out = lv.invP.p; ar.err = pl->errflag.p;
        ar.node_base = (int)pl->level_ptr[m];            // regular trees: slot s of level m is node level_ptr[m] + s
        launch_cascade_any(pl, ar);
    }
}

// leaves W (all levels and the y block) at every row - lik_rows: at the observed rows - the prior variance, and with scatter_ut the leaves' Ut.
// only: at the rows of these workgroups' tiles alone (whole tiles of ft_row0, never gathered) - the dirty leaves of a pass that keeps the rest
static void run_prior_fused_rows(mra_plan* pl, const CascadeArgs& base, const mra_plan::LeafTileWgs* only = nullptr) {
    const PassRoute& r = pl->route;
    Work fl;
    for (int m = 0; m < pl->NL; ++m) fl += pl->lev[m].fl_resid + pl->lev[m].fl_trsm;
    // one pass: coordinates and y in, W (all levels + y block) and the prior variance out, observed rows once more into Ut
    fl.bytes = 8.0 * pl->P * (pl->d + 1 + pl->ldw + 1) + pl->by_leaf_ut;
    if (only) {
        const double share = 16.0 * (double)only->n_tiles / (double)std::max<long>(pl->P, 1);
        fl.alg *= share; fl.exec *= share; fl.bytes = share * 8.0 * pl->P * (pl->d + 1 + pl->ldw + 1);
    }
    // a likelihood needs W at the OBSERVED rows only (Ut and the leaves' C = v(o,o) + R I are built from them)
    else if (r.lik_rows) {
        ensure_lik_tiles(pl);
        const double share = 16.0 * (double)pl->n_lik_tiles / (double)std::max<long>(pl->P, 1);
        fl.alg *= share; fl.exec *= share; fl.bytes = share * 8.0 * pl->P * (pl->d + 1 + pl->ldw) + pl->by_leaf_ut;
    }
    KTimer kt(pl, KF_PRIOR_TRSM, fl);
    CascadeArgs ar = base;
    ar.knot_mode = 0; ar.mlast = pl->NL - 1; ar.dbg = pl->dbg;
#ifdef MRA_STAMPS
    ar.stamps = stamp_buffer(pl->stamps, (size_t)pl->n_ftiles * 16);
#endif
    ar.var_out = pl->var.p; ar.cov0 = kernel_cov0(pl);
    ar.ycol = pl->Ka; ar.y = pl->y.p;
    if (r.scatter_ut) {
        ar.obs_pos = pl->obs_pos.p; ar.tile_leaf = pl->ft_leaf.p; ar.leaf_ut = pl->leaf_ut.p; ar.leaf_nop = pl->leaf_nop_dev.p;
        ar.y = pl->y.p;
        // Ut rows follow W's ancestor columns of a last-level leaf: a = column - asuf[NL]
        for (int m = 0; m < pl->NL; ++m) ar.ut_off[m] = pl->coff[m] - pl->asuf[pl->NL];
        ar.ut_yrow = pl->Ka - pl->asuf[pl->NL];
    }
    if (pl->cascade_stage_all) { ar.n_wg = pl->n_fwg_leaf; ar.wg_tile0 = pl->ft_wg0_leaf.p; ar.wg_ntiles = pl->ft_wgn_leaf.p; }
    else { ar.n_wg = pl->n_fwg; ar.wg_tile0 = pl->ft_wg0.p; ar.wg_ntiles = pl->ft_wgn.p; }
    ar.tile_row0 = pl->ft_row0.p; ar.tile_chain = pl->ft_chain.p;
    if (r.lik_rows) ar.var_out = nullptr;              // the prior variance is the predictive pass's (the y block stays: Ut's y row is gathered from it)
    if (only) { ar.n_wg = only->n_wg; ar.wg_tile0 = only->wg0.p; ar.wg_ntiles = only->wgn.p; }
    else if (r.lik_rows) {
        ar.row_gather = pl->obs_idx.p; ar.tile_chain = pl->lik_chain.p; ar.tile_leaf = pl->lik_leaf.p;
        ar.n_wg = pl->n_lik_wg; ar.wg_tile0 = pl->lik_wg0.p; ar.wg_ntiles = pl->lik_wgn.p;
    }
    launch_cascade_any(pl, ar);
}

// the y block of every row once more and, on a pass that writes the variance, the prior variance put back: what stands in for the row
// cascade where its W is kept
static void run_prior_refresh(mra_plan* pl, bool with_var) {
    KTimer kt(pl, KF_MISC, Work(0.0, 0.0, 8.0 * 16.0 * pl->n_ftiles * (MRA_YB + (with_var ? 3 : 1))));
    const long n = pl->n_ftiles * 64;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_refresh_yblock, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, pl->stream, pl->W.p, (long)pl->ldw, pl->Ka, pl->y.p,
                       pl->ft_row0.p, pl->n_ftiles, with_var ? pl->var.p : (double*)nullptr, pl->var_prior.p);
}

// the prior variance of a full row pass, kept for the passes that keep its W (one device copy of P doubles)
static void keep_prior_var(mra_plan* pl) {
    if (pl->var_prior.n != (size_t)pl->P) pl->var_prior.alloc((size_t)pl->P);
    KTimer kt(pl, KF_MISC, Work(0.0, 0.0, 16.0 * pl->P));
    HIP_TRY(hipMemcpyAsync(pl->var_prior.p, pl->var.p, (size_t)pl->P * sizeof(double), hipMemcpyDeviceToDevice, pl->stream));
}

// prior_step_for decides what runs; the plan's record (pl->keep) follows every launch as it is enqueued
static void run_prior_fused(mra_plan* pl) {
    typedef mra_plan::PriorKeep K;
    const PassRoute& r = pl->route;
    const PriorStep step = prior_step_for(pl, r);
    const CascadeArgs base = prior_cascade_base(pl);
    K& k = pl->keep;
    if (step.run_knots) {
        prior_keep_reset(pl);                // new factors: nothing that was built on the old ones stands
        run_prior_fused_knots(pl, base);
        k.knots_valid = true;
    }
    switch (step.rows) {
        case PriorRows::RunAll:
            run_prior_fused_rows(pl, base);
            k.rows = r.lik_rows ? K::Rows::Observed : K::Rows::All;
            k.dirty = K::Dirty::Clean;
            pl->stale.n_wg = pl->stale.n_tiles = 0;
            if (!r.lik_rows && pl->use_prior_reuse) { keep_prior_var(pl); k.var_valid = true; }
            return;
        case PriorRows::KeepRerunDirty:
            run_prior_refresh(pl, !r.lik_rows);
            run_prior_fused_rows(pl, base, pl->stale.n_wg ? &pl->stale : &pl->big);
            k.dirty = K::Dirty::Clean;
            pl->stale.n_wg = pl->stale.n_tiles = 0;
            return;
        case PriorRows::KeepAll:
            run_prior_refresh(pl, !r.lik_rows);
            return;
    }
}

// predictive pass of a deep 64-wide tree (regular_hi): W holds the whitened basis after the leaf update
static void run_predict_hi(mra_plan* pl) {
    const int NL = pl->NL, nlo = NL - 4;
    PredHiArgs hi{};
    Work fl_hi, fl_lo;
    for (int h = 0; h < 4; ++h) {
        const int m = nlo + h;
        hi.hi[h].F = pl->lev[m].F.p; hi.hi[h].invF = pl->lev[m].invF.p; hi.hi[h].nf = pl->lev[m].nf;
        hi.hi[h].ld = pl->lev[m].ldf; hi.hi[h].stride = (long)pl->lev[m].nf * pl->lev[m].ldf;
        hi.coff_hi[h] = pl->coff[m];
        fl_hi += pl->lev[m].fl_trsm + pl->lev[m].fl_update;
    }
    hi.W = pl->W.p; hi.var = pl->var.p; hi.ldw = pl->ldw;
    hi.col_low = pl->coff[nlo - 1]; hi.n_low = nlo * 4 + 1; hi.lev0 = nlo;
    hi.tile_row0 = pl->ft_row0.p; hi.tile_chain = pl->ft_chain.p; hi.wg_tile0 = pl->ft_wg0.p; hi.wg_ntiles = pl->ft_wgn.p;
    // W read once, its coarse columns and y block written once; var in and out
    fl_hi.bytes = 8.0 * pl->P * (pl->ldw + (pl->ldw - pl->coff[nlo - 1]) + 2);
    const bool fold = pl->route.update == LeafUpdate::InPredictHi;
    if (fold) {
        // the leaf update rides in k_predict_hi (Tt and Ut in, nothing out)
        hi.wg_leaf = pl->hi_wgleaf.p; hi.leaf_ut = pl->leaf_ut.p; hi.leaf_nop = pl->leaf_nop_dev.p; hi.leaf_row0 = pl->leaf_row0_dev.p; hi.na = pl->na[NL];
        fl_hi += Work(pl->fl_leaf_update.alg, pl->fl_leaf_update.exec, pl->by_leaf_tt + pl->by_leaf_ut);
    }
    PredArgs lo{};
    for (int m = 0; m < nlo; ++m) {
        lo.lev[m].F = pl->lev[m].F.p; lo.lev[m].invF = pl->lev[m].invF.p; lo.lev[m].nf = pl->lev[m].nf;
        lo.lev[m].ld = pl->lev[m].ldf; lo.lev[m].stride = (long)pl->lev[m].nf * pl->lev[m].ldf;
        lo.coff[m] = pl->coff[m];
        fl_lo += pl->lev[m].fl_trsm + pl->lev[m].fl_update;
    }
    lo.deep = lo.lev[nlo - 1];
    lo.W = pl->W.p; lo.mean = pl->mean.p; lo.var = pl->var.p; lo.ldw = pl->ldw; lo.ycol = pl->Ka;
    lo.tile_row0 = pl->ft_row0.p; lo.tile_chain = pl->ft_chain.p; lo.wg_tile0 = pl->hi_wg0_8.p; lo.wg_ntiles = pl->hi_wgn_8.p;
    lo.n_wg = pl->n_hi_wg8; lo.nl = nlo;
    fl_lo.bytes = 8.0 * pl->P * ((pl->ldw - pl->coff[nlo - 1]) + 3);
    const size_t lds_low = (size_t)(4 * 3 / 2 + 4 + ((nlo - 1) * 4 + 1) * 4) * 2048;
    // two launches; the kernel timer brackets both (the coarse share is reported with them: they are one pass over W's coarse half)
    KTimer kt(pl, KF_PRED_UPDATE, fl_hi + fl_lo);
    launch_predict_hi(pl, hi, lo, lds_low, fold);
}

static void run_predict_fused(mra_plan* pl) {
    PredArgs ar{};
    for (int m = 0; m < pl->NL; ++m) {
        ar.lev[m].F = pl->lev[m].F.p; ar.lev[m].invF = pl->lev[m].invF.p; ar.lev[m].nf = pl->lev[m].nf;
        ar.lev[m].ld = pl->lev[m].ldf; ar.lev[m].stride = (long)pl->lev[m].nf * pl->lev[m].ldf;
        ar.coff[m] = pl->coff[m];
    }
    ar.deep = ar.lev[pl->NL - 1];
    ar.W = pl->W.p; ar.mean = pl->mean.p; ar.var = pl->var.p; ar.ldw = pl->ldw; ar.ycol = pl->Ka;
    ar.tile_row0 = pl->ft_row0.p; ar.tile_chain = pl->ft_chain.p; ar.wg_tile0 = pl->ft_wg0_x.p; ar.wg_ntiles = pl->ft_wgn_x.p;
    ar.n_wg = pl->n_fwg_x; ar.nl = pl->NL;
    const int cwt = pl->CWT, mmax = pl->NL - 1;
    size_t lds = (size_t)(cwt * (cwt - 1) / 2 + cwt + (mmax * cwt + 1) * cwt) * 2048;
    Work fl;
    for (int m = 0; m < pl->NL; ++m) fl += pl->lev[m].fl_trsm + pl->lev[m].fl_update;
    fl.bytes = 8.0 * pl->P * (pl->ldw + 3);                // W once in, var in/out, mean out (the level operands stay in L2)
    if (pl->route.update == LeafUpdate::InCascade) {
        // the leaf update rides in this launch (two Ut chunk stages share the LDS with the level operands)
        ar.tile_leaf = pl->ft_leaf.p; ar.wg_leaf = pl->ft_wgleaf_x.p; ar.leaf_ut = pl->leaf_ut.p; ar.leaf_nop = pl->leaf_nop_dev.p; ar.leaf_row0 = pl->leaf_row0_dev.p;
        ar.leaf_upd = pl->leaf_upd_dev.p; ar.na = pl->na[pl->NL];
        // two 8-k chunks of Ut behind the deepest level's half A (which is requested while the last chunk's products issue)
        lds = std::max(lds, (size_t)(cwt * (cwt - 1) / 2 + cwt + (mmax / 2) * cwt * cwt) * 2048 + (size_t)(2 * (pl->NL * cwt + 1) * 128) * sizeof(double));
        fl += Work(pl->fl_leaf_update.alg, pl->fl_leaf_update.exec, pl->by_leaf_tt + pl->by_leaf_ut);    // Tt and Ut in, nothing out
    }
#ifdef MRA_STAMPS
    ar.stamps = stamp_buffer(pl->pstamps, (size_t)pl->n_ftiles * 16);
#endif
    KTimer kt(pl, KF_PRED_UPDATE, fl);
    if (ar.n_wg <= 0) return;
    launch_predict_any(pl, ar, lds);
}

// ---- the executor: a pass in stages ("the executor").  Every stage reads pl->route, launches on pl->stream and leaves what
// its comment says for the next one; mra_run_all and run_fronts_and_predict are the two drivers ----------------------------------------
// events 0 and 5 bracket every pass; the four inner phase boundaries are recorded only with kernel timing on
// (each hipEventRecord between dependent launches leaves a ~6 us gap on the stream)
static void phase_mark(mra_plan* pl, int k) { if (k == 0 || k == 5 || pl->ktiming) hipEventRecord(pl->ev[k], pl->stream); }

// allocate the per-leaf Schur blocks the first time a run needs them and point the descriptors at them
static void ensure_gt(mra_plan* pl) {
    if (pl->Gt.p || pl->leaf_goff.back() == 0) return;
    pl->Gt.alloc(pl->leaf_goff.back());
    for (size_t k = 0; k < pl->hKids.size(); ++k)
        if (pl->kid_leaf[k] >= 0) pl->hKids[k].G = pl->Gt.p + pl->leaf_goff[pl->kid_leaf[k]];
    pl->asmKids.upload(pl->hKids);
    for (size_t t = 0; t < pl->hLeafSyrk.size(); ++t) pl->hLeafSyrk[t].C = pl->Gt.p + pl->leaf_goff[t];
    pl->gLeafSyrk.upload(pl->hLeafSyrk);
}

// leaves an open pass: both streams idle of any abandoned pass, the pass state and the kernel statistics reset, pl->route fixed
static const PassRoute& open_pass(mra_plan* pl, uint32_t flags, bool full_rows) {
    if (g_dry) refuse_dry_run();
    if (!(pl->have_locs && pl->have_obs && pl->have_kernel))
        throw MraError(MRA_ERR_STATE, "mra_run needs set_locs, set_obs and set_kernel first");
    HIP_TRY(mraSetDevice(pl->device));
    if (pl->pass_open) {
        // the previous pass never reached finish_run (an error was thrown, or a split run was abandoned before
        // mra_run_resume): wait for whatever it left on the two streams (every fork's work is on one of them, whether its join
        // was recorded or not), and clear the device error flag that only the last kernel of a pass resets
        pl->cphantom_valid = false;
        prior_keep_reset(pl);
        if (pl->side_pending) HIP_TRY(hipStreamWaitEvent(pl->stream, pl->ev_join, 0));
        HIP_TRY(hipStreamSynchronize(pl->stream));
        HIP_TRY(hipStreamSynchronize(pl->stream2));
        HIP_TRY(hipMemsetAsync(pl->errflag.p, 0, sizeof(int), pl->stream));
        for (auto& e : pl->kev) { hipEventDestroy(e.second.first); hipEventDestroy(e.second.second); }
        pl->kev.clear();
    }
    pl->side_pending = false;
    pl->split_pending = false;
    pl->pass_open = true;
    pl->run_flags = flags;
    pl->slv.valid = false;               // whatever runs a pass rewrites the factors (mra_solve sets the mark again after its own)
    for (int k = 0; k < KF_COUNT; ++k) pl->kstat[k] = mra_plan::KStat();
    if (!pl->lik_general_valid && route_for(pl, flags, full_rows).lik_general) ensure_lik_general(pl);      // (once; route_for reads the verdict)
    pl->route = route_for(pl, flags, full_rows);
    pl->route_set = true;
    // MRA_OPT_LEAF_ORDER's fork (pass state, not part of the route read-back): there is a split to overlap - two launches per stage
    // (TilesSplit; TilesOne has one launch for all leaves) and leaves on either side of it
    const PassRoute& r = pl->route;
    pl->leaf_fork = pl->use_leaf_fork && r.path == PassPath::Fused && r.chol == LeafChol::TilesSplit &&
                    0 < pl->n_trsm_small && pl->n_trsm_small < pl->leaf_nodes.size();
    return pl->route;
}

// leaves W's y block holding y at every row and, with acc_var, var holding the prior variance C(x,x) for the row solves to subtract from
static void run_init_yblock(mra_plan* pl, const PassRoute& r) {
    KTimer kt(pl, KF_MISC, 0);
    const long n = pl->P * MRA_YB;
    hipLaunchKernelGGL(k_init_yblock, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, pl->stream, pl->W.p,
                       (long)pl->ldw, pl->Ka, pl->y.p, pl->P, r.acc_var ? pl->var.p : (double*)nullptr, pl->host_cov ? 0.0 : kernel_cov0(pl),
                       pl->host_cov ? pl->covdiag.p : (const double*)nullptr);
}

// ---- prior, level by level (PassPath::Hi and Levels; run_prior_fused is the Fused form).  Either form of a level leaves its prior
// factor Lp with inverted diagonal blocks and W's columns of the level at every row below its nodes (lik_general: at the needed rows)
// knots' residual block -> Lp (both sides gathered), its Cholesky, then residual + kernel + row solve of every row in one launch: the
// residual never visits HBM
static void run_prior_level_one_launch(mra_plan* pl, const PassRoute& r, LevelData& lv) {
    const size_t nn = lv.nodes.size();
    { KTimer kt(pl, KF_PRIOR_CHOL, lv.fl_knot_resid); launch_gemm<EPI_COV>(pl, lv.gKnotResid.p, nn, lv.cw, lv.cw); }
    { KTimer kt(pl, KF_PRIOR_CHOL, lv.fl_pchol); launch_panel(pl, lv.gPriorChol.p, nn); }
    if (r.lik_general) {
        Work w = lv.fl_resid + lv.fl_trsm.with_bytes(0.0);
        w.alg *= lv.lik_share; w.exec *= lv.lik_share; w.bytes *= lv.lik_share;
        KTimer kt(pl, KF_PRIOR_RESID, w);
        mra_launch_prior_level(pl, lv.gResidLik.p, lv.gResidLik.n);
    } else {
        KTimer kt(pl, KF_PRIOR_RESID, lv.fl_resid + lv.fl_trsm.with_bytes(0.0));
        mra_launch_prior_level(pl, lv.gResidFused.p, lv.gResidFused.n);
    }
}

// residual of every row into W, the knots' block gathered out of it, its Cholesky, the row solve
static void run_prior_level_four_launches(mra_plan* pl, int m) {
    LevelData& lv = pl->lev[m];
    const size_t nn = lv.nodes.size();
    {
        KTimer kt(pl, KF_PRIOR_RESID, lv.fl_resid);
        if (pl->host_cov) launch_gemm<EPI_HOSTCOV>(pl, lv.gResid.p, nn, lv.max_rows, lv.cw);
        else launch_gemm<EPI_COV>(pl, lv.gResid.p, nn, lv.max_rows, lv.cw);
    }
    {
        KTimer kt(pl, KF_MISC, 0);
        dim3 grid((unsigned)((lv.cw * lv.cw + 255) / 256), (unsigned)nn);
        hipLaunchKernelGGL(k_gather_kinv, grid, dim3(256), 0, pl->stream, lv.gKinv.p, pl->W.p, (long)pl->ldw, lv.c0);
    }
    { KTimer kt(pl, KF_PRIOR_CHOL, lv.fl_pchol); launch_panel(pl, lv.gPriorChol.p, nn); }
    { KTimer kt(pl, KF_PRIOR_TRSM, lv.fl_trsm); launch_level_row_solve(pl, m, lv.gTrsm2Prior.p, lv.gTrsmPrior.p, nullptr); }
}

static void run_prior_levels(mra_plan* pl, const PassRoute& r) {
    for (int m = 0; m < pl->n_levels; ++m) {
        LevelData& lv = pl->lev[m];
        if (lv.nodes.empty()) continue;
        if (r.prior_level && lv.prior_level_ok) run_prior_level_one_launch(pl, r, lv);
        else run_prior_level_four_launches(pl, m);
    }
}

// ---- leaves (nl of them, nl > 0).  A leaf's panel is [C ; Ut ; V] (leaf_C / leaf_Ut / leaf_V) ------------------------------------
// leaves every leaf's V[S,o] residual with C = v(o,o) + R I (+ 0 while a noise vector is set) on top of it, or with c_only nothing but C
// (resid_step_for: on an eligible route into the kept buffer, or not at all where the last pass's product stands)
static void run_leaf_product(mra_plan* pl, const PassRoute& r, size_t nl) {
    if (resid_route_eligible(pl, r)) ensure_resid_lists(pl);
    const ResidStep step = resid_step_for(pl, r);
    if (step == ResidStep::Keep) return;
    KTimer kt(pl, KF_LEAF_RESID, r.c_only ? pl->fl_leaf_c_only : pl->fl_leaf_resid);
    if (step == ResidStep::Run) {
        pl->rkeep.resid = mra_plan::ResidKeep::Form::None;      // (until the launch is enqueued)
        if (r.c_only) launch_gemm<EPI_COV>(pl, pl->kLeafResidLik.p, nl, pl->leaf_max_nop, pl->leaf_max_nop);
        else launch_leaf_gemm<EPI_COV>(pl, pl->kLeafResid.p, nl);
        pl->rkeep.resid = r.c_only ? mra_plan::ResidKeep::Form::COnly : mra_plan::ResidKeep::Form::Full;
        return;
    }
    if (pl->host_cov) {
        if (r.leaf_resident) launch_leaf_gemm<EPI_HOSTCOV>(pl, pl->gLeafResid.p, nl);
        else launch_gemm<EPI_HOSTCOV>(pl, pl->gLeafResid.p, nl, pl->leaf_max_rows, pl->leaf_max_nop);
    }
    else if (r.c_only) launch_gemm<EPI_COV>(pl, pl->gLeafResidLikSorted.n ? pl->gLeafResidLikSorted.p : pl->gLeafResidLik.p, nl, pl->leaf_max_nop, pl->leaf_max_nop);
    else if (r.leaf_resident) launch_leaf_gemm<EPI_COV>(pl, pl->gLeafResidSorted.n ? pl->gLeafResidSorted.p : pl->gLeafResid.p, nl);
    else launch_gemm<EPI_COV>(pl, pl->gLeafResid.p, nl, pl->leaf_max_rows, pl->leaf_max_nop);
}

// leaves C whole, identity rows at its phantom observations (the padding to 16) included; Fill: all of C gathered out of V, and Ut out of W
static void run_leaf_c_fix(mra_plan* pl, const PassRoute& r, size_t nl) {
    if (r.c_fix == LeafCFix::None) return;
    KTimer kt(pl, KF_MISC, 0);
    // (InProduct: nothing to do, the gathered COV product wrote the whole C block including phantom identities)
    if (r.c_fix == LeafCFix::Phantom && resid_out_of_place(pl, r)) {
        // the kept C0 is never factorised in place and the gathered C-only product writes identity rows there too: once per mask
        if (!pl->rkeep.phantom) {
            hipLaunchKernelGGL(k_leaf_cphantom, dim3((unsigned)nl), dim3(256), 0, pl->stream, pl->kLeaf.p, pl->leaf_nobs.p);
            pl->rkeep.phantom = true;
        }
    } else if (r.c_fix == LeafCFix::Phantom) {
        // C comes from the COV epilogue, Ut from the gather inside k_trsm_rows2: only the phantom rows remain
        // ... once: an identity row stays an identity row under the in-place factorisation (L[p][j] = 0, L[p][p] = 1 exactly) and
        // no epilogue writes there, so later passes find them in place.  (A failed pass - NaN times 0 - a new observation pattern
        // or a change of options bring the launch back.)
        if (!pl->cphantom_valid) {
            hipLaunchKernelGGL(k_leaf_cphantom, dim3((unsigned)nl), dim3(256), 0, pl->stream, pl->gLeaf.p, pl->leaf_nobs.p);
            pl->cphantom_valid = true;
        }
    } else if (r.c_fix == LeafCFix::Fill) {
        const long total = (long)(pl->leaf_max_nop + pl->leaf_max_na) * pl->leaf_max_nop;
        dim3 grid((unsigned)std::min<long>((total + 255) / 256, 64), (unsigned)nl);
        hipLaunchKernelGGL(k_leaf_fill, grid, dim3(256), 0, pl->stream, pl->gLeaf.p, pl->W.p, (long)pl->ldw, pl->noise_on ? 0.0 : pl->R);
    }
}

// (a noise vector is set) leaves C = v(o,o) + diag(r_o): the stages above wrote v(o,o) + 0, exactly v(o,o), so the diagonal takes the one
// rounding of the scalar path's v + R.  On the main stream, before the leaves' fork; every route and both kinds of pass come through here
// (out of place k_chol_tiles adds it as it loads the diagonal tiles: nothing to launch)
static void run_leaf_noise(mra_plan* pl, const PassRoute& r, size_t nl) {
    if (!pl->noise_on || resid_out_of_place(pl, r)) return;
    KTimer kt(pl, KF_MISC, 0);
    hipLaunchKernelGGL(k_leaf_noise, dim3((unsigned)((nl + 3) / 4)), dim3(256), 0, pl->stream, pl->gLeaf.p, pl->leaf_nobs.p, pl->noise.p, (int)nl);
}

// A fork to the side stream.  With `on` the launch helpers (they use pl->stream) go to stream2 between the constructor and join();
// without it nothing moves.  after: the event that orders stream2 behind what the main stream holds now (nullptr: stream2 is already
// behind everything the forked work reads); joined: recorded on stream2 by join(), for the main stream to wait for.  The leaves' fork
// has events of its own, so that no wait can be lost to a later record of the predict-only fork's.  A throw in
// between restores pl->stream (later launches must not land on the side stream) and records no join event; open_pass then waits for
// both streams.  Nothing meant for the main stream may be launched while a fork is open.
struct SideFork {
    mra_plan* pl; hipStream_t main_stream; bool side; hipEvent_t joined;
    SideFork(mra_plan* p, bool on, hipEvent_t after, hipEvent_t joined_) : pl(p), main_stream(p->stream), side(on), joined(joined_) {
        if (!side) return;
        if (after) {
            HIP_TRY(hipEventRecord(after, main_stream));
            HIP_TRY(hipStreamWaitEvent(pl->stream2, after, 0));
        }
        pl->stream = pl->stream2;
    }
    void join() {
        if (!side) return;
        pl->stream = main_stream;
        HIP_TRY(hipEventRecord(joined, pl->stream2));
    }
    ~SideFork() { pl->stream = main_stream; }
};

// every leaf's C fits k_chol_tiles / k_chol_wave: the Cholesky, then the LDS row solve of the rows below C.  leaf_fork: the few leaves
// of more than LEAF_SMALL_TILES tiles do both on the side stream meanwhile (two short launches of a handful of workgroups, which
// would otherwise hold the whole GPU in turn); the main stream waits for them here, behind its own row solve - before any consumer
// of a leaf's Ut, before mra_run_resume's part of a split pass, and inside the KF_LEAF_CHOL bracket of run_leaf_factor
static void run_leaf_chol_and_solve(mra_plan* pl, const PassRoute& r, size_t nl) {
    const int obs_tiles = pl->leaf_max_nop / 16;                                              // the widest C, in 16-row tiles
    const int row_tiles = r.predict ? pl->leaf_max_tiles_full : pl->leaf_max_tiles_lik;       // the most row tiles below one leaf's C
    if (r.path != PassPath::Fused) { launch_leaf_chol(pl, r, nl); launch_trsm2(pl, r.trsm_all, nl, obs_tiles, row_tiles, row_tiles); return; }
    // Fused: the small leaves (the first n_trsm_small of every list) on k_trsm_rows2<LEAF_SMALL_TILES>, one workgroup each
    const size_t n_small = pl->n_trsm_small;
    const int small_row_tiles = (r.predict && !r.solve_fused) ? pl->trsm_small_tiles_full : pl->trsm_small_tiles_lik;
    // the few leaves with more than LEAF_SMALL_TILES observation tiles: several workgroups per leaf when they are few
    // (one leaf per workgroup would put a single 65 us workgroup on the critical path)
    // out of place: the predict lists that read the kept V0 (the likelihood-only lists hold the Ut rows alone, gathered from W as ever)
    const bool oop = resid_out_of_place(pl, r);
    auto kept = [&](const Trsm2Prob* p) { return (oop && p == pl->gLeafTrsmFullPlainG.p) ? pl->kLeafTrsmFullPlainG.p : p; };
    const Trsm2Prob *trsm_all = kept(r.trsm_all), *trsm_small = kept(r.trsm_small);
    auto solve_rest = [&] { launch_trsm2(pl, trsm_all + n_small, nl - n_small, obs_tiles, row_tiles, (nl - n_small) < 512 ? 4 : row_tiles); };
    if (pl->leaf_fork) {
        SideFork fork(pl, true, pl->ev_leaf_fork, pl->ev_leaf_join);
        launch_leaf_chol(pl, r, nl, LeafPart::Rest);
        solve_rest();
        fork.join();
    }
    launch_leaf_chol(pl, r, nl, pl->leaf_fork ? LeafPart::Small : LeafPart::All);
    if (n_small) launch_trsm2(pl, trsm_small, n_small, pl->trsm_small_nt, small_row_tiles, small_row_tiles);
    if (pl->leaf_fork) HIP_TRY(hipStreamWaitEvent(pl->stream, pl->ev_leaf_join, 0));
    else if (nl > n_small) solve_rest();
}

// LeafChol::BigPanels.  Right-looking, 64 columns per step: the panel (factor + solve of ALL rows below, Ut and Tt included) on one
// workgroup per leaf, the rank-64 update of everything to its right as a batched GEMM over the whole GPU
// (a single workgroup factorising an 8560 x 8560 block column by column took 15 s: README example 1)
static void run_leaf_big_panels(mra_plan* pl, const PassRoute& r, size_t nl) {
    const int v = r.predict ? 0 : 1;
    for (size_t st = 0; st < pl->gBigPanel[v].size(); ++st) {
        launch_panel(pl, pl->gBigPanel[v][st].p, nl, st > 0 ? 1 : 0);
        if (pl->bigM[v][st] > 0 && pl->bigN[v][st] > 0)
            launch_gemm<EPI_SUB>(pl, pl->gBigTrail[v][st].p, nl, pl->bigM[v][st], pl->bigN[v][st]);
    }
}

// leaves C = Lc Lc^T factorised in place (log-determinants in dnode) and Ut = Lc^-1 Ut; where the route's row-solve lists hold them
// (every predict pass but the small leaves under solve_fused) the rows of V solved too: Tt
static void run_leaf_factor(mra_plan* pl, const PassRoute& r, size_t nl) {
    KTimer kt(pl, KF_LEAF_CHOL, r.predict ? pl->fl_leaf_chol : pl->fl_leaf_chol_lik);
    if (r.chol != LeafChol::BigPanels) run_leaf_chol_and_solve(pl, r, nl);
    else run_leaf_big_panels(pl, r, nl);
}

// (!direct_parent) leaves every leaf's Schur block Gt = Ut Ut^T for its parent's assembly
static void run_leaf_syrk(mra_plan* pl, size_t nl) {
    ensure_gt(pl);
    KTimer kt(pl, KF_LEAF_SYRK, pl->fl_leaf_syrk);
    launch_gemm<EPI_SET>(pl, pl->gLeafSyrk.p, nl, pl->leaf_max_na, pl->leaf_max_na, false, true);
}

// leaves var = max(C(x,x) - |W_anc[x]|^2 - |Tt[x]|^2, 0) and the y column of the leaves' rows reset (LeafVar::None: the fused kernels' own work)
static void run_leaf_var(mra_plan* pl, const PassRoute& r) {
    if (r.var == LeafVar::None) return;
    KTimer kt(pl, KF_MISC, 0);
    ensure_row_leaf(pl);
    if (r.var == LeafVar::FinishVar)
        hipLaunchKernelGGL(k_leaf_finish_var, dim3((unsigned)((pl->P + 255) / 256)), dim3(256), 0, pl->stream, pl->row_leaf.p, pl->W.p,
                           (long)pl->ldw, pl->Ka, pl->var.p, pl->P);
    else
        hipLaunchKernelGGL(k_leaf_moments, dim3((unsigned)((pl->P + 3) / 4)), dim3(256), 0, pl->stream, pl->gLeaf.p,
                           pl->row_leaf.p, pl->W.p, (long)pl->ldw, pl->Ka, pl->var.p, pl->host_cov ? 0.0 : kernel_cov0(pl),
                           pl->host_cov ? pl->covdiag.p : (const double*)nullptr, pl->P);
}

// LeafUpdate::SolveWhole / SolveHalves.  Tt = V Lc^-T, var -= |Tt|^2 and W -= Tt Ut^T in one launch for the leaves with
// <= LEAF_SMALL_TILES observation tiles; the few larger ones went through the full row solve and take the plain update product
static void run_leaf_solve_update(mra_plan* pl, const PassRoute& r, size_t nl) {
    ensure_big_lds(pl, {(const void*)k_leaf_solve_update<8, 13, true>});
    KTimer kt(pl, KF_LEAF_UPDATE, pl->fl_leaf_update);
    const size_t n_small = pl->n_trsm_small;
    const bool oop = resid_out_of_place(pl, r);          // the small leaves' V from the kept V0
#ifdef MRA_STAMPS
    stamp_buffer(pl->kstamps2, pl->n_leaf_solve_half * 8);
#endif
    if (r.update == LeafUpdate::SolveHalves)
        hipLaunchKernelGGL((k_leaf_solve_update<8, 13, true>), dim3((unsigned)pl->n_leaf_solve_half), dim3(512), pl->leaf_solve_lds, pl->stream, oop ? pl->kLeafSolveHalf.p : pl->gLeafSolveHalf.p MRA_LSTAMP_VAL);
    else
        hipLaunchKernelGGL((k_leaf_solve_update<8, 13, true>), dim3((unsigned)n_small), dim3(512), pl->leaf_solve_lds, pl->stream, oop ? pl->kLeafSolve.p : pl->gLeafSolve.p MRA_LSTAMP_NUL);
    if (nl > n_small) launch_gemm<EPI_SUB>(pl, pl->gLeafUpdatePlain.p + n_small, nl - n_small, pl->leaf_max_rows, pl->leaf_max_na);
}

// leaves W[S,anc] -= Tt Ut^T at every leaf that does not take its update inside the predictive kernel (LeafUpdate)
static void run_leaf_update(mra_plan* pl, const PassRoute& r, size_t nl) {
    typedef mra_plan::PriorKeep K;
    // what the update overwrites of the prior rows is marked here, where it is enqueued: a pass abandoned later must not look clean
    switch (r.update) {
        case LeafUpdate::None: return;
        case LeafUpdate::InPredictHi: pl->keep.dirty = K::Dirty::All; return;  // (nothing to launch here; k_predict_hi rewrites W)
        case LeafUpdate::InCascade: {
            // the small leaves (<= LEAF_SMALL_TILES observation tiles) take their update inside the predictive cascade; the few larger ones here
            // (leaf_fork: on the side stream, behind those leaves' row solve, unless the route has put this whole stage there already)
            const size_t n_small = pl->n_trsm_small;
            if (nl <= n_small) return;
            if (pl->keep.dirty == K::Dirty::Clean) pl->keep.dirty = K::Dirty::Oversized;
            const bool to_side = pl->leaf_fork && pl->stream != pl->stream2;
            SideFork fork(pl, to_side, nullptr, pl->ev_join);
            {
                KTimer kt(pl, KF_LEAF_UPDATE, 0);
                launch_gemm<EPI_SUB>(pl, pl->gLeafUpdatePlain.p + n_small, nl - n_small, pl->leaf_max_rows, pl->leaf_max_na);
            }
            fork.join();
            if (to_side) pl->side_pending = true;       // join_side_stream makes the main stream wait, just before the predictive pass
            return;
        }
        case LeafUpdate::SolveWhole: case LeafUpdate::SolveHalves: pl->keep.dirty = K::Dirty::All; run_leaf_solve_update(pl, r, nl); return;
        case LeafUpdate::LeafGemm: { pl->keep.dirty = K::Dirty::All; KTimer kt(pl, KF_LEAF_UPDATE, pl->fl_leaf_update); launch_leaf_gemm<EPI_SUB>(pl, pl->gLeafUpdate.p, nl); return; }
        case LeafUpdate::Gemm: { pl->keep.dirty = K::Dirty::All; KTimer kt(pl, KF_LEAF_UPDATE, pl->fl_leaf_update); launch_gemm<EPI_SUB>(pl, pl->gLeafUpdate.p, nl, pl->leaf_max_rows, pl->leaf_max_na); return; }
    }
}

// (predict) leaves var and W ready for the predictive pass, on the side stream (side_pending) where the route forks
static void run_leaf_predict_work(mra_plan* pl, const PassRoute& r, size_t nl) {
    SideFork fork(pl, r.side, pl->ev_fork, pl->ev_join);
    run_leaf_var(pl, r);
    run_leaf_update(pl, r, nl);
    fork.join();
    if (r.side) pl->side_pending = true;            // join_side_stream makes the main stream wait, just before the predictive pass
}

// ---- fronts, bottom-up ------------------------------------------------------------------------------------------------------------
// factorise the fronts of level m (already assembled in global memory unless do_assemble): fused kernel when the
// front (or at least its panel) fits in LDS, else panel Cholesky + Schur GEMM as separate launches
static bool run_front_fused(mra_plan* pl, int m, bool do_assemble, bool add_identity) {
    LevelData& lv = pl->lev[m];
    const size_t nn = lv.nodes.size();
    if (!nn) return true;
    if (!pl->route.front_fused || lv.front_mode == 0 || (do_assemble && lv.front_mode != 2)) return false;
    ensure_big_lds(pl, {(const void*)k_front<true>, (const void*)k_front<false>});
    KTimer kt(pl, KF_FRONT_CHOL, lv.fl_fchol + lv.fl_schur);
    if (lv.front_mode == 2)
        hipLaunchKernelGGL(k_front<true>, dim3((unsigned)nn), dim3(512), lv.front_lds, pl->stream, lv.gFront.p, pl->asmKids.p,
                           pl->dnode.p, pl->errflag.p, do_assemble ? 1 : 0, add_identity ? 1 : 0);
    else
        hipLaunchKernelGGL(k_front<false>, dim3((unsigned)nn), dim3(512), lv.front_lds, pl->stream, lv.gFront.p, pl->asmKids.p,
                           pl->dnode.p, pl->errflag.p, 0, add_identity ? 1 : 0);
    return true;
}

static void run_front_level(mra_plan* pl, int m) {
    LevelData& lv = pl->lev[m];
    const size_t nn = lv.nodes.size();
    if (!nn) return;
    { KTimer kt(pl, KF_FRONT_CHOL, lv.fl_fchol); launch_panel(pl, lv.gFrontChol.p, nn); }
    { KTimer kt(pl, KF_FRONT_SCHUR, lv.fl_schur); launch_gemm<EPI_SUB>(pl, lv.gSchur.p, nn, lv.na, lv.na, false, true); }
}

// sum_in / sum_n / sum_out: also add up that many log-determinants (in order) into *sum_out, in the same launch
static bool run_assemble_level(mra_plan* pl, int m, bool with_identity, const double* sum_in = nullptr, int sum_n = 0, double* sum_out = nullptr) {
    LevelData& lv = pl->lev[m];
    const size_t nn = lv.nodes.size();
    if (!nn) return false;
    KTimer kt(pl, KF_MISC, 0);
    const long total = (long)lv.nf * lv.nf;
    dim3 grid((unsigned)std::min<long>((total + 255) / 256, 64), (unsigned)(nn + (sum_in ? 1 : 0)));
    hipLaunchKernelGGL(k_assemble, grid, dim3(256), 0, pl->stream, lv.gAsm.p, pl->asmKids.p, with_identity ? 1 : 0, sum_in, sum_n, sum_out);
    return true;
}

static void run_add_identity(mra_plan* pl, int m) {
    LevelData& lv = pl->lev[m];
    const size_t nn = lv.nodes.size();
    if (!nn) return;
    KTimer kt(pl, KF_MISC, 0);
    hipLaunchKernelGGL(k_add_identity, dim3((unsigned)((lv.cw + 63) / 64), (unsigned)nn), dim3(64), 0, pl->stream, lv.gAsm.p);
}

// What happens to the fronts of level m, first match wins (direct_parent already excludes reduce_level == NL-1):
//   step          when                                                  form_front launches                              afterwards
//   Resumed       mra_run_resume's first level                          nothing: the caller summed the fronts, which      factor; the identity is missing
//                                                                       sit in HBM as the Reduce step left them           iff this is the reduce level
//   ParentFront   direct_parent, m == NL-1, parent_front                k_parent_front<nacc>: children's Ut -> front ->   level done
//                                                                       Lt, Zt, Schur block, never in HBM unfactorised
//   ParentPanels  direct_parent, m == NL-1, the level is panel_only     k_parent_front<2|4> on the own block, the panel   level done
//                                                                       GEMM, the LDS row solve (throws if too wide)
//   ParentSyrk    direct_parent, m == NL-1 otherwise                    the gParentSyrk GEMM: the front complete in HBM   factor
//   GrandSyrk     direct_parent, m == NL-2, level NL-1 is panel_only    k_syrk_blk or the GEMM (throws if this is the     factor
//                                                                       reduce level): the front complete in HBM
//   Reduce        m == reduce_level                                     k_assemble without identity + the log-det sum of  reduce_front (split: the pass is
//                                                                       everything below (k_sum_dnode if no assembly ran) suspended), factor, identity missing
//   Children      otherwise                                             nothing                                           factor, assembling on the way
enum class FrontStep { Resumed, ParentFront, ParentPanels, ParentSyrk, GrandSyrk, Reduce, Children };

// Pure, like route_for: reads the plan and the route, touches nothing.  resumed_here: mra_run_resume re-enters the loop at this level
static FrontStep front_step_for(const mra_plan* pl, const PassRoute& r, int m, bool resumed_here) {
    if (resumed_here) return FrontStep::Resumed;
    if (r.direct_parent && m == pl->NL - 1)
        return r.parent_front ? FrontStep::ParentFront : pl->lev[m].panel_only ? FrontStep::ParentPanels : FrontStep::ParentSyrk;
    if (r.direct_parent && m == pl->NL - 2 && pl->lev[pl->NL - 1].panel_only) return FrontStep::GrandSyrk;
    return m == pl->reduce_level ? FrontStep::Reduce : FrontStep::Children;
}

// FrontStep::ParentPanels.  Only the panel columns of these fronts exist: build them, factorise them, done with the level
static void run_parent_panels(mra_plan* pl, int m) {
    const LevelData& lv = pl->lev[m];
    const size_t nn = lv.nodes.size();
    {
        KTimer kt(pl, KF_LEAF_SYRK, pl->fl_parent_panel);
        launch_parent_front(pl, lv.cwt <= 4 ? 2 : 4, nn, pl->parent_own_lds, pl->gParentOwn.p);
        launch_gemm<EPI_SET>(pl, pl->gParentPanel.p, nn, lv.na, lv.cw, pl->seg_gemm_lds && pl->parent_panel_lds_ok, false);
    }
    KTimer kt(pl, KF_FRONT_CHOL, lv.fl_fchol.with_bytes(8.0 * 2 * nn * (double)lv.na * lv.cw));
    if (!launch_trsm2(pl, pl->gParentZt.p, nn, lv.cwt, lv.na / 16, lv.na / 16))
        throw MraError(MRA_ERR_STATE, "panel row solve: block too wide for the LDS row solve");
}

// FrontStep::Reduce.  The reduce level's fronts are summed over ranks WITHOUT their identity blocks; the 16-double tail of the buffer
// carries the rank-local log-det sum of everything below (in the assembly's launch; on its own where the level holds no node)
static void run_assemble_reduce_level(mra_plan* pl, int m) {
    LevelData& lv = pl->lev[m];
    const int lo = (int)pl->level_ptr[m + 1];
    double* tail = lv.F.p + (lv.F.n - 16);
    if (run_assemble_level(pl, m, false, pl->dnode.p + lo, pl->n_nodes - lo, tail)) return;
    KTimer kt(pl, KF_MISC, 0);
    hipLaunchKernelGGL(k_sum_dnode, dim3(1), dim3(256), 0, pl->stream, pl->dnode.p + lo, pl->n_nodes - lo, tail);
}

// form: leaves level m's fronts as the table's row says - factorised (ParentFront, ParentPanels), in HBM, or still in their children
static void form_front(mra_plan* pl, const PassRoute& r, FrontStep step, int m) {
    const LevelData& lv = pl->lev[m];
    switch (step) {
        case FrontStep::Resumed: case FrontStep::Children: return;
        case FrontStep::ParentFront: {
            KTimer kt(pl, KF_LEAF_SYRK, (pl->fl_leaf_syrk + lv.fl_fchol + lv.fl_schur).with_bytes(pl->by_leaf_ut + 8.0 * lv.nodes.size() * (0.5 * lv.nf * (lv.nf + 1))));
            // MRA_OPT_PARENT_PAIR (pass state, not part of the route): two four-wave workgroups per CU where a CU gets more than one
            // front; with at most one front per CU (an 8-way shard) a front finishes sooner on eight waves
            const bool pair = pl->parent_pair_nacc > 0 && (pl->use_parent_pair == 2 || (pl->use_parent_pair == 1 && lv.nodes.size() > (size_t)pl->n_cu));
            if (pair) {
                pl->kstat[KF_LEAF_SYRK].flops_exec += pl->parent_pair_idle_exec;
                launch_parent_front(pl, pl->parent_pair_nacc, lv.nodes.size(), pl->parent_pair_lds, pl->gParentFront.p, true);
            }
            else launch_parent_front(pl, pl->parent_front_nacc, lv.nodes.size(), pl->parent_front_lds, pl->gParentFront.p);
            return;
        }
        case FrontStep::ParentPanels: run_parent_panels(pl, m); return;
        case FrontStep::ParentSyrk: {
            KTimer kt(pl, KF_LEAF_SYRK, pl->fl_leaf_syrk);
            launch_gemm<EPI_SET>(pl, pl->gParentSyrk.p, lv.nodes.size(), lv.nf, lv.nf, false, true);
            return;
        }
        case FrontStep::GrandSyrk: {
            if (m == pl->reduce_level) throw MraError(MRA_ERR_STATE, "the reduce level cannot be the level above panel-only fronts");
            KTimer kt(pl, KF_FRONT_SCHUR, pl->fl_grand_syrk);
            if (r.syrk_blk) mra_launch_syrk_blk(pl, pl->gGrandSyrk.p, lv.nodes.size(), lv.nf, r.syrk_dma);
            else launch_gemm<EPI_SET>(pl, pl->gGrandSyrk.p, lv.nodes.size(), lv.nf, lv.nf, false, true);      // (64 x 64 LDS-tiled: 24.2 vs 23.7 ms at config 5)
            return;
        }
        case FrontStep::Reduce: run_assemble_reduce_level(pl, m); return;
    }
}

// reduce: leaves the reduce level's fronts summed over all ranks.  Returns false where that is the caller's job (MRA_RUN_SPLIT): the
// pass is suspended until mra_run_resume
static bool reduce_front(mra_plan* pl, int m) {
    LevelData& lv = pl->lev[m];
    if (pl->run_flags & MRA_RUN_SPLIT) { pl->split_pending = true; return false; }
    // a reduce level without a transport would silently build the likelihood from this rank's partial fronts
    if (!pl->comm || !pl->allreduce)
        throw MraError(MRA_ERR_STATE, "reduce level set but neither a communicator (mra_comm_init) nor MRA_RUN_SPLIT: "
                                      "the fronts of the reduce level would not be summed over ranks");
    if (pl->allreduce(lv.F.p, lv.F.p, lv.F.n, ncclDouble, ncclSum, pl->comm, pl->stream) != ncclSuccess)
        throw MraError(MRA_ERR_COMM, "ncclAllReduce failed");
    return true;
}

// factor: leaves level m's fronts factorised ([Lt ; Zt], inverted diagonal blocks, log-determinants) and their Schur blocks ready for
// the parents.  in_hbm: the fronts are assembled in global memory (else k_front<true> assembles them in LDS where the whole front fits,
// k_assemble where not; either adds the identity); needs_identity: ... but without their identity blocks
static void factor_front(mra_plan* pl, int m, bool in_hbm, bool needs_identity) {
    if (!in_hbm) {
        if (run_front_fused(pl, m, true, true)) return;
        run_assemble_level(pl, m, true);
    }
    if (run_front_fused(pl, m, false, needs_identity)) return;
    if (needs_identity) run_add_identity(pl, m);
    run_front_level(pl, m);
}

// ---- predictive pass --------------------------------------------------------------------------------------------------------------
// leaves the main stream waiting for the predict-only leaf work that run_leaf_predict_work put on the side stream
static void join_side_stream(mra_plan* pl) {
    if (!pl->side_pending) return;
    HIP_TRY(hipStreamWaitEvent(pl->stream, pl->ev_join, 0));
    pl->side_pending = false;
}

// PassPath::Levels: per level, bottom-up, the posterior row solve (var -= the solved rows' squares) and the update of the columns above
static void run_predict_levels(mra_plan* pl) {
    for (int m = pl->n_levels - 1; m >= 0; --m) {
        LevelData& lv = pl->lev[m];
        const size_t nn = lv.nodes.size();
        if (!nn) continue;
        { KTimer kt(pl, KF_PRED_TRSM, lv.fl_trsm); launch_level_row_solve(pl, m, lv.gTrsm2Post.p, lv.gTrsmPost.p, pl->var.p); }
        { KTimer kt(pl, KF_PRED_UPDATE, lv.fl_update); launch_gemm<EPI_SUB>(pl, lv.gUpdate.p, nn, lv.max_rows, lv.na); }
    }
}

// leaves the predictive variance in var and the mean in `mean` (Levels: in W's y block, for k_extract_mean)
static void run_predict(mra_plan* pl) {
    if (!pl->route.predict) return;
    switch (pl->route.path) {
        case PassPath::Fused: run_predict_fused(pl); return;
        case PassPath::Hi: run_predict_hi(pl); return;          // (sharded plans too: the fronts above the reduce level are complete by now)
        case PassPath::Levels: run_predict_levels(pl); return;
    }
}

// ---- the end of a pass ------------------------------------------------------------------------------------------------------------
// leaves the record {d, u, log-det carried by the reduce level, error flag} in pinned host memory (MRA_HOST_RES_DOUBLES doubles: the
// reduction of mra_plan_fit_laplace writes its five behind them) - written by the kernel
// straight into it: no copy command, no gap after the last launch - and with extract_mean the mean out of W's y block
static void launch_result(mra_plan* pl) {
    KTimer kt(pl, KF_MISC, 0);
    const int nsum = pl->reduce_level >= 0 ? (int)pl->level_ptr[pl->reduce_level + 1] : pl->n_nodes;
    const double* up;
    if (pl->leaf[0]) up = pl->Gt.p + pl->leaf_goff[pl->leaf_slot[0]] + (size_t)(pl->na[0] - MRA_YB) * pl->na[0] + (pl->na[0] - MRA_YB);
    else {
        const LevelData& l0 = pl->lev[0];
        up = l0.F.p + (size_t)(l0.nf - MRA_YB) * l0.nf + (l0.nf - MRA_YB);
    }
    const double* below = nullptr;
    if (pl->reduce_level >= 0) {
        const LevelData& lr = pl->lev[pl->reduce_level];
        if (lr.F.n) below = lr.F.p + (lr.F.n - 16);
    }
    if (!pl->host_res) {
        HIP_TRY(hipHostMalloc((void**)&pl->host_res, MRA_HOST_RES_DOUBLES * sizeof(double), hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer((void**)&pl->host_res_dev, pl->host_res, 0));
    }
    hipLaunchKernelGGL(k_sum_dnode, dim3(1), dim3(256), 0, pl->stream, pl->dnode.p, nsum, pl->host_res_dev, up, below, pl->errflag.p);
    if (pl->route.extract_mean)
        hipLaunchKernelGGL(k_extract_mean, dim3((unsigned)((pl->P + 255) / 256)), dim3(256), 0, pl->stream,
                           pl->W.p, (long)pl->ldw, pl->Ka, pl->mean.p, pl->P);
}

// the per-kernel times of the launches recorded so far (KTimer, kernel timing on) into the plan; drops their events.  The stream has
// been synchronised.
void mra_harvest_kernel_events(mra_plan* pl) {
    for (auto& e : pl->kev) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, e.second.first, e.second.second);
        pl->kstat[e.first].ms += ms;
        hipEventDestroy(e.second.first); hipEventDestroy(e.second.second);
    }
    pl->kev.clear();
}

// the finished pass's phase times (the inner four only with kernel timing on) and per-kernel times into the plan; drops the kernel events
static void harvest_timers(mra_plan* pl) {
    float ms;
    for (int k = 0; k < 4; ++k) {
        ms = 0.f;
        if (pl->ktiming) hipEventElapsedTime(&ms, pl->ev[k], pl->ev[k + 1]);
        pl->phase_ms[k] = ms;
    }
    hipEventElapsedTime(&ms, pl->ev[0], pl->ev[5]);
    pl->phase_ms[4] = ms;
    mra_harvest_kernel_events(pl);
}

// the pass is over, whatever it found: errv is the record's error flag (0, or 1 + the node whose Cholesky failed)
static void close_pass(mra_plan* pl, int errv) {
    pl->ran = true;
    pl->split_pending = false;
    pl->pass_open = false;
    if (!errv) return;
    pl->cphantom_valid = false;
    prior_keep_reset(pl);
    char b[160];
    snprintf(b, sizeof b, "matrix not positive definite in node %d (Cholesky pivot <= 0 or NaN)", errv - 1);
    throw MraError(MRA_ERR_NOT_SPD, b);
}

static void finish_run(mra_plan* pl) {
    launch_result(pl);
    phase_mark(pl, 5);
    if (pl->pass_tail) pl->pass_tail();      // (mra_plan_fit_laplace's reduction: behind the pass's last kernel, under its one synchronisation)
    HIP_TRY(hipStreamSynchronize(pl->stream));
    HIP_TRY(hipGetLastError());
    const int errv = (int)pl->host_res[3];
    pl->res_d = pl->host_res[0] + pl->host_res[2]; pl->res_u = pl->host_res[1];
    harvest_timers(pl);
    close_pass(pl, errv);
}

// ---- the two drivers --------------------------------------------------------------------------------------------------------------
// fronts bottom-up from level m_from, then the predictive pass and the result.  resume: mra_run_resume, after the caller has summed the
// reduce level's fronts over the ranks
static void run_fronts_and_predict(mra_plan* pl, int m_from, bool resume) {
    const PassRoute& r = pl->route;
    pl->slv.valid = false;
    for (int m = m_from; m >= 0; --m) {
        const FrontStep step = front_step_for(pl, r, m, resume && m == m_from);
        form_front(pl, r, step, m);
        switch (step) {
            case FrontStep::ParentFront: case FrontStep::ParentPanels: break;                                // formed and factorised in one
            case FrontStep::ParentSyrk: case FrontStep::GrandSyrk: factor_front(pl, m, true, false); break;
            case FrontStep::Resumed: factor_front(pl, m, true, m == pl->reduce_level); break;
            case FrontStep::Reduce:
                if (!reduce_front(pl, m)) return;                                                            // suspended: mra_run_resume goes on
                factor_front(pl, m, true, true);
                break;
            case FrontStep::Children: factor_front(pl, m, false, false); break;
        }
    }
    phase_mark(pl, 3);
    join_side_stream(pl);
    run_predict(pl);
    phase_mark(pl, 4);
    finish_run(pl);
}

// full_rows: the caller reads W at every row afterwards (sampler_prior); a likelihood-only pass then walks all rows
void mra_run_all(mra_plan* pl, uint32_t flags, bool full_rows) {
    const PassRoute& r = open_pass(pl, flags, full_rows);
    phase_mark(pl, 0);
    if (r.init_yblock) run_init_yblock(pl, r);
    // ---- 1. prior, top-down
    if (r.path == PassPath::Fused) run_prior_fused(pl);
    else { prior_keep_reset(pl); run_prior_levels(pl, r); }      // (Hi, Levels: their stages rewrite W in place - nothing is kept)
    phase_mark(pl, 1);
    // ---- 2. leaves
    const size_t nl = pl->leaf_nodes.size();
    if (nl) {
        run_leaf_product(pl, r, nl);
        run_leaf_c_fix(pl, r, nl);
        run_leaf_noise(pl, r, nl);
        run_leaf_factor(pl, r, nl);
        if (!r.direct_parent) run_leaf_syrk(pl, nl);
        if (r.predict) run_leaf_predict_work(pl, r, nl);
    }
    phase_mark(pl, 2);
    // ---- 3./4. fronts bottom-up, then predictive moments
    run_fronts_and_predict(pl, pl->n_levels - 1, false);
}

// ---- sampler (mra_sample) ------------------------------------------------------------------------------
// Latent slots: [0, Kn) the non-leaf nodes in node order, cw[level] each; [Kn, Kn + P) leaf terms by padded row (read at leaf knot
// rows); [Kn + P, Kn + 2P) observation noise by padded row (read at observed rows of a conditional draw).
static const size_t SAMPLE_GRAM_BUDGET = (size_t)1536 << 20;   // default bytes of leaf Gram blocks + inverted diagonal blocks per batch
static const size_t SAMPLE_LEAF_GRID = 65535;                  // leaves per launch of the kernels that take the leaf from blockIdx.y

static void sampler_build(mra_plan* pl) {
    mra_plan::Sampler& S = pl->smp;
    if (S.built) return;
    const long P = pl->P;
    mra_row_maps(pl);
    S.n_coarse = mra_coarse_slots(pl, &S.zoff);
    const size_t nl = pl->leaf_nodes.size();
    std::vector<int> chain_ptr(nl + 1, 0);
    std::vector<SampleChain> chain;
    for (size_t t = 0; t < nl; ++t) {
        const std::vector<int> up = leaf_ancestors(pl, pl->leaf_nodes[t]);
        for (auto p = up.rbegin(); p != up.rend(); ++p) {      // leaf to root: the order k_sample_coarse sums in
            const int k = pl->node_level[*p];
            if (pl->cw[k]) chain.push_back(SampleChain{pl->coff[k], (int)S.zoff[*p], pl->cw[k], 0});
        }
        chain_ptr[t + 1] = (int)chain.size();
    }
    // Gram batches: consecutive leaves while their nr^2 + 16 nr doubles stay within the budget (at least one leaf per batch)
    S.bat.assign(1, 0);
    S.bat_rows.clear();
    const size_t budget = S.gram_bytes ? S.gram_bytes : SAMPLE_GRAM_BUDGET;
    size_t cur = 0, gmax = 0, imax = 0, ncur = 0, nmax = 0, icur = 0;
    long rmax = 0;
    std::vector<long> goff(nl), ioff(nl);
    for (size_t t = 0; t < nl; ++t) {
        const int i = pl->leaf_nodes[t];
        const long nr = pl->row1[i] - pl->row0[i];
        const size_t need = (size_t)nr * nr + 16 * (size_t)nr;
        if (ncur && (cur + need) * sizeof(double) > budget) {
            S.bat.push_back(t); S.bat_rows.push_back(rmax);
            cur = 0; icur = 0; ncur = 0; rmax = 0;
        }
        goff[t] = (long)(cur - icur); ioff[t] = (long)icur;     // cur: Gram + inverted blocks of the batch so far, icur: the latter
        cur += need; icur += 16 * (size_t)nr; ++ncur; rmax = std::max(rmax, nr);
        gmax = std::max(gmax, cur - icur); imax = std::max(imax, icur); nmax = std::max(nmax, ncur);
    }
    if (nl) { S.bat.push_back(nl); S.bat_rows.push_back(rmax); }
    S.G.alloc(std::max<size_t>(gmax, 1)); S.invd.alloc(std::max<size_t>(imax, 1));
    S.dn.alloc(std::max<size_t>(nmax, 1)); S.err.alloc(1);
    std::vector<SampleLeaf> lv(nl);
    std::vector<GemmProb> gp(nl);
    std::vector<PanelProb> cp(nl);
    for (size_t b = 0; b + 1 < S.bat.size(); ++b)
        for (size_t t = S.bat[b]; t < S.bat[b + 1]; ++t) {
            const int i = pl->leaf_nodes[t];
            const long r0 = pl->row0[i], nr = pl->row1[i] - r0;
            const int a0 = pl->asuf[pl->node_level[i]];
            double* G = S.G.p + goff[t];
            lv[t] = SampleLeaf{G, r0, (int)nr};
            GemmProb g{};                                    // v_M(S, S) = C(S, S) - W_anc[S] W_anc[S]^T: the residual GEMM's COV epilogue
            g.A = pl->W.p + r0 * pl->ldw + a0; g.lda = pl->ldw;
            g.B = g.A; g.ldb = pl->ldw;
            g.C = G; g.ldc = nr;
            g.XA = pl->X.p + r0 * pl->d; g.XB = g.XA;
            g.M = (int)nr; g.N = (int)nr; g.K = pl->Ka - a0;
            gp[t] = g;
            cp[t] = PanelProb{G, S.invd.p + ioff[t], nr, (int)(nr / 16), (int)(nr / 16), (int)(t - S.bat[b])};
        }
    S.chain_ptr.upload(chain_ptr);
    if (chain.empty()) chain.push_back(SampleChain{0, 0, 0, 0});
    S.chain.upload(chain);
    if (nl) { S.leaves.upload(lv); S.gram.upload(gp); S.chol.upload(cp); }
    S.ysave.alloc(P); S.msave.alloc(P); S.vsave.alloc(P);
    S.factored = -1;
    S.built = true;
}

// v_M(K_j, K_j) of a batch of leaves, masked to the identity off the knots, factorised in place
static void sampler_factor(mra_plan* pl, size_t b) {
    mra_plan::Sampler& S = pl->smp;
    const size_t t0 = S.bat[b], n = S.bat[b + 1] - t0;
    const long rmax = S.bat_rows[b];
    launch_gemm<EPI_COV>(pl, S.gram.p + t0, n, rmax, rmax);
    for (size_t off = 0; off < n; off += SAMPLE_LEAF_GRID)
        hipLaunchKernelGGL(k_sample_mask, dim3((unsigned)std::min<long>((rmax * rmax + 255) / 256, 64), (unsigned)std::min(SAMPLE_LEAF_GRID, n - off)),
                           dim3(256), 0, pl->stream, S.leaves.p + t0 + off, pl->maps.knot.p);
    HIP_TRY(hipMemsetAsync(S.err.p, 0, sizeof(int), pl->stream));
    mra_panel_chol(pl, S.chol.p + t0, n, S.dn.p, S.err.p);
    const int e = stream_wait_err(pl, S.err.p);
    S.factored = (int)b;
    if (e) {
        S.factored = -1;
        char m[160];
        snprintf(m, sizeof m, "leaf %d: v_M(K, K) is not positive definite (Cholesky pivot <= 0 or NaN)", pl->leaf_nodes[t0 + e - 1]);
        throw MraError(MRA_ERR_NOT_SPD, m);
    }
}

// the likelihood pass with W at every row: the prior basis the sampler reads (option 17 is overridden by the route, not through the option)
static void sampler_prior(mra_plan* pl) { mra_run_all(pl, MRA_RUN_LIKELIHOOD, true); }

static void sample_all(mra_plan* pl, uint32_t flags, int64_t n, uint64_t seed, int64_t sample0, const double* z, double* out) {
    mra_retained_check_plan(pl, "mra_sample", flags, MRA_SAMPLE_CONDITIONAL, "cannot sample (leaf C(S, S) is not available)", "cannot sample");
    const bool cond = flags & MRA_SAMPLE_CONDITIONAL;
    if (n < 0) throw MraError(MRA_ERR_INVALID, "n_samples < 0");
    mra_check_sample0(sample0, n);
    if (pl->knots_pending) throw MraError(MRA_ERR_STATE, "knot rows not set");
    if (n == 0) return;
    if (!out) throw MraError(MRA_ERR_INVALID, "out is NULL");
    HIP_TRY(mraSetDevice(pl->device));
    sampler_build(pl);
    mra_plan::Sampler& S = pl->smp;
    S.use_solve = cond && pl->slv.in_sampler;
    if (S.use_solve) mra_solver_build(pl);
    const long P = pl->P, Kn = S.n_coarse, n_slots = Kn + 2 * P;
    const size_t nb = S.bat.size() - 1;
    // caller-given draws are staged a block of samples at a time (at most 512 MB of them)
    const int nsb = z ? (int)std::max<long>(1, std::min<long>(16, ((long)512 << 20) / (8 * n_slots))) : 16;
    mra_reserve_coarse(S.zc, Kn);
    if (S.out.n < (size_t)16 * P) S.out.alloc((size_t)16 * P);
    if (z && S.zh.n < (size_t)nsb * n_slots) S.zh.alloc((size_t)nsb * n_slots);
    {
        KeepResults keep(pl, S.ysave.p, S.msave.p, S.vsave.p);      // the last mra_run's results and the device y
        S.factored = -1;                      // the kernel, the locations or the observations may have changed since the last call
        bool w_prior = false;
        for (int64_t s0 = 0; s0 < n; s0 += nsb) {
            const int ns = (int)std::min<int64_t>(nsb, n - s0);
            SampleZ zs{nullptr, n_slots, (unsigned long long)seed, (long)(sample0 + s0), ns};
            if (z) {
                HIP_TRY(hipMemcpyAsync(S.zh.p, z + s0 * n_slots, (size_t)ns * n_slots * sizeof(double), hipMemcpyHostToDevice, pl->stream));
                zs.z = S.zh.p;
            }
            if (!w_prior) { sampler_prior(pl); w_prior = true; }
            // coarse term: all non-leaf draws of the block, then one wave per row tile
            if (Kn) mra_sample_draw(pl, zs, Kn, S.zc.p);
            hipLaunchKernelGGL(k_sample_coarse, dim3((unsigned)((P / 16 + 3) / 4)), dim3(256), 0, pl->stream, pl->W.p, (long)pl->ldw,
                               pl->maps.tile_leaf.p, S.chain_ptr.p, S.chain.p, S.zc.p, pl->maps.rep.p, S.out.p, P);
            // leaf term, batch by batch (a single batch is factorised once per call)
            for (size_t b = 0; b < nb; ++b) {
                if (S.factored != (int)b) sampler_factor(pl, b);
                const size_t t0 = S.bat[b], cnt = S.bat[b + 1] - t0;
                for (size_t off = 0; off < cnt; off += SAMPLE_LEAF_GRID)
                    hipLaunchKernelGGL(k_sample_leaf, dim3((unsigned)((S.bat_rows[b] + 15) / 16), (unsigned)std::min(SAMPLE_LEAF_GRID, cnt - off)),
                                       dim3(256), 0, pl->stream, S.leaves.p + t0 + off, pl->maps.knot.p, pl->maps.rep.p, zs, Kn, S.out.p, P);
            }
            if (cond && S.use_solve) {
                // conditioning by kriging, all draws of the block at once: the factors of the prior pass above are those of the
                // posterior mean (they do not depend on y), so the block's pseudo-data are 16 right-hand sides of mra_solve's sweeps
                mra_solver_pseudo(pl, S.ysave.p, S.out.p, zs, Kn + P);
                mra_solver_block(pl, true, false);
                mra_solver_addmean(pl, S.out.p, ns);
            } else if (cond) {
                // conditioning by kriging: x + mean_MRA(y - x_o - sqrt(r_o) eps), one likelihood + predict pass per sample
                for (int s = 0; s < ns; ++s) {
                    double* xs = S.out.p + (long)s * P;
                    if (pl->noise_on)
                        hipLaunchKernelGGL(k_sample_pseudo_rows, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, pl->stream, S.ysave.p, xs, zs, s,
                                           Kn + P, pl->noise_sd.p, pl->y.p, P);
                    else
                        hipLaunchKernelGGL(k_sample_pseudo, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, pl->stream, S.ysave.p, xs, zs, s,
                                           Kn + P, std::sqrt(pl->R), pl->y.p, P);
                    mra_run_all(pl, MRA_RUN_LIKELIHOOD | MRA_RUN_PREDICT);
                    hipLaunchKernelGGL(k_sample_addmean, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, pl->stream, xs, pl->mean.p, pl->maps.rep.p, P);
                }
                w_prior = false;              // the predict passes rewrote W
            }
            HIP_TRY(hipMemcpyAsync(out + s0 * P, S.out.p, (size_t)ns * P * sizeof(double), hipMemcpyDeviceToHost, pl->stream));
            stream_wait(pl);
            if (nb > 1) S.factored = -1;      // G holds the last batch only
        }
    }
    HIP_TRY(hipGetLastError());
}

// ---- caller-order variants: the permutation work of an end-to-end MRATree(...) call done inside the library -----------------
// A process-wide pinned staging area (grow-only): gathers land in it, the H2D / D2H copies run at the pinned rate (a pageable
// 16 MB copy costs ~5 ms, a pinned one ~0.7 ms), and a second plan in the same process does not pay for the allocation again.
static std::mutex g_stage_mutex;
static double* g_stage = nullptr;
static size_t g_stage_n = 0;
static double* stage_buffer(size_t n) {               // caller holds g_stage_mutex
    if (n > g_stage_n) {
        if (g_stage) { if (g_dry) free(g_stage); else hipHostFree(g_stage); g_stage = nullptr; g_stage_n = 0; }
        if (g_dry) g_stage = (double*)malloc(n * sizeof(double));
        else if (hipHostMalloc((void**)&g_stage, n * sizeof(double), hipHostMallocDefault) != hipSuccess) g_stage = nullptr;
        if (!g_stage) throw MraError(MRA_ERR_HIP, "pinned staging allocation failed");
        g_stage_n = n;
    }
    return g_stage;
}


// knot coordinates of the fused levels (locs: P x d in padded leaf order): per level for the cascades, and packed per workgroup
// for the knot chain
static void set_knot_coords_src(mra_plan* pl, const double* locs, const int64_t* src);
static void set_knot_coords(mra_plan* pl, const double* locs) { set_knot_coords_src(pl, locs, nullptr); }
// (src: locs is the CALLER's N x d array and padded row p holds caller row src[p]; nullptr: locs is already in padded order)
static void upload_knot_chain(mra_plan* pl, const std::vector<std::vector<double>>& kxh);
static void upload_knot_coords(mra_plan* pl);
static void set_knot_coords_src(mra_plan* pl, const double* locs, const int64_t* src) {
    prior_keep_reset(pl);
    if (!pl->regular) return;
    const int cw = pl->cw[0];
    std::vector<std::vector<double>> kxh(pl->kc_levels);
    if (pl->metric_on) pl->knot_raw.assign((size_t)pl->NL, std::vector<double>());
    for (int m = 0; m < pl->NL; ++m) {
        const LevelData& lv = pl->lev[m];
        std::vector<double> kx(lv.nodes.size() * (size_t)cw * pl->d);
        for (size_t e = 0; e < kx.size(); ++e)           // phantom knots: far away and far from each other
            kx[e] = MRA_FAR_AWAY * (double)(2 + (e / pl->d) % cw);
        for (size_t sl = 0; sl < lv.nodes.size(); ++sl) {
            const int i = lv.nodes[sl];
            const long rk = pl->knot_ptr[i + 1] - pl->knot_ptr[i];
            for (long c = 0; c < rk; ++c)
                for (int k = 0; k < pl->d; ++k)
                    kx[(sl * cw + c) * pl->d + k] = locs[(src ? src[pl->knot_rows[pl->knot_ptr[i] + c]] : pl->knot_rows[pl->knot_ptr[i] + c]) * pl->d + k];
        }
        if (pl->metric_on) { pl->knot_raw[m].swap(kx); continue; }      // (the metric's plans: kept raw, sent transformed below)
        HIP_TRY(mraMemcpy(pl->fl[m].kx.p, kx.data(), kx.size() * sizeof(double), hipMemcpyHostToDevice));
        if (m < pl->kc_levels) kxh[m].swap(kx);
    }
    if (pl->metric_on) { upload_knot_coords(pl); return; }
    upload_knot_chain(pl, kxh);
}

// k_knot_chain's packed records from the knot coordinates of its levels (kxh[m], m < kc_levels, as the kernels read them)
static void upload_knot_chain(mra_plan* pl, const std::vector<std::vector<double>>& kxh) {
    const int cw = pl->cw[0];
    // k_knot_chain: every workgroup's knots of all its levels in one record (coordinates, then 1.0 / 0.0 = real / phantom)
    if (pl->kc_levels >= 2 && pl->kc_knots.n) {
        const int nlv = pl->kc_levels, d = pl->d;
        const size_t rec = (size_t)cw * (d + 1), nb = pl->lev[nlv - 1].nodes.size();
        std::vector<double> pk(nb * nlv * rec);
        for (size_t b = 0; b < nb; ++b)
            for (int m = 0; m < nlv; ++m) {
                const int sl = pl->kc_chain_host[b * 8 + m];
                const int i = pl->lev[m].nodes[sl];
                const long rk = pl->knot_ptr[i + 1] - pl->knot_ptr[i];
                double* o = pk.data() + (b * nlv + m) * rec;
                std::memcpy(o, kxh[m].data() + (size_t)sl * cw * d, (size_t)cw * d * sizeof(double));
                for (int c = 0; c < cw; ++c) o[(size_t)cw * d + c] = c < rk ? 1.0 : 0.0;
            }
        HIP_TRY(mraMemcpy(pl->kc_knots.p, pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice));
    }
}

// The knot coordinates of a plan that has (or just dropped) a metric, from the raw ones it keeps: real knots through the metric's one
// function (mra_metric_row), phantom knots as they are - MRA_FAR_AWAY is a distance to stay away by, not a location.
static void upload_knot_coords(mra_plan* pl) {
    if (!pl->regular || pl->knot_raw.empty()) return;
    const int cw = pl->cw[0], d = pl->d;
    std::vector<std::vector<double>> kxh(pl->kc_levels);
    for (int m = 0; m < pl->NL; ++m) {
        const LevelData& lv = pl->lev[m];
        std::vector<double> kx = pl->knot_raw[m];
        if (pl->metric_on)
            for (size_t sl = 0; sl < lv.nodes.size(); ++sl) {
                const int i = lv.nodes[sl];
                const long rk = pl->knot_ptr[i + 1] - pl->knot_ptr[i];
                for (long c = 0; c < rk; ++c)
                    mra_metric_row_d(d, pl->metric_A, pl->knot_raw[m].data() + (sl * cw + c) * d, kx.data() + (sl * cw + c) * d);
            }
        HIP_TRY(mraMemcpy(pl->fl[m].kx.p, kx.data(), kx.size() * sizeof(double), hipMemcpyHostToDevice));
        if (m < pl->kc_levels) kxh[m].swap(kx);
    }
    upload_knot_chain(pl, kxh);
}

// ---- one plan lifetime ------------------------------------------------------------------------------------------------------
// Every plan is released by destroy_plan (mra_plan_destroy and every failed construction alike), so all of them give back the
// same things: the RCCL communicator, the streams' pending work, the events, the arena, the streams and the pinned buffers.
static void destroy_plan(mra_plan* pl) {
    if (!pl) return;
    mraSetDevice(pl->device);
    if (pl->comm && pl->rccl) {
        typedef ncclResult_t (*destroy_t)(ncclComm_t);
        destroy_t fn = (destroy_t)dlsym(pl->rccl, "ncclCommDestroy");
        if (fn) fn(pl->comm);
    }
    // the plan's device blocks go back to the cache and may be handed to another plan at once: nothing of this plan may still run
    if (pl->stream) hipStreamSynchronize(pl->stream);
    if (pl->stream2) hipStreamSynchronize(pl->stream2);
    for (int k = 0; k < 6; ++k) if (pl->ev[k]) hipEventDestroy(pl->ev[k]);
    drop_arena(pl);
    return_streams(pl);                              // (with the pinned result record and the arena's pinned mirror)
    for (hipEvent_t e : {pl->ev_fork, pl->ev_join, pl->ev_leaf_fork, pl->ev_leaf_join}) if (e) hipEventDestroy(e);
    delete pl;
}
struct PlanDeleter { void operator()(mra_plan* pl) const { destroy_plan(pl); } };
typedef std::unique_ptr<mra_plan, PlanDeleter> PlanPtr;

// A new plan on `device` with its streams, events and descriptor arena; the caller copies the topology in and runs build_static.
static PlanPtr new_plan(int device) {
    if (!g_dry) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            throw MraError(MRA_ERR_HIP, "no HIP device available: libmra_hip needs an AMD GPU (gfx950); there is no CPU fallback");
        if (device < 0 || device >= ndev) throw MraError(MRA_ERR_INVALID, "device ordinal out of range");
    }
    HIP_TRY(mraSetDevice(device));
    PlanPtr pl(new mra_plan());
    pl->device = device;
    if (!g_dry) {
        // The leaf update (one large GEMM) and [parent SYRK -> front Cholesky/Schur chain -> all-reduce of a sharded run]
        // only meet again in the predictive cascade: they are issued on two streams, so the collective and the
        // latency-bound chain never wait behind the update.  (On one GPU the update keeps every SIMD's register file
        // full and the pass time does not change; the point is the sharded run.)
        acquire_streams(pl.get());
        for (hipEvent_t* e : {&pl->ev_fork, &pl->ev_join, &pl->ev_leaf_fork, &pl->ev_leaf_join})
            HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
        for (int k = 0; k < 6; ++k) HIP_TRY(hipEventCreate(&pl->ev[k]));
    }
    init_arena(pl.get());
    return pl;
}

// ---- the C ABI's one exception boundary -------------------------------------------------------------------------------------
// The exports run their bodies through guarded(): an MraError returns its code, any other C++ exception (std::bad_alloc, the
// std::system_error of a thread that cannot start, ...) MRA_ERR_INVALID with its what(), anything else MRA_ERR_INVALID "unknown
// C++ exception"; the message goes to pl->err (pl not NULL) and to the calling thread's g_last_error.  Only exports that read
// plain fields stay outside it (tests/test_capi_cpu.py holds the same list): mra_version, mra_last_error, mra_device_count,
// mra_kernel_family_count, mra_get_timers, mra_plan_info, mra_get_kernel_stats, mra_get_kernel_work, mra_tree_sizes.
template <class F>
static int guarded(mra_plan* pl, F&& body) {
    try { return body(); }
    catch (const MraError& e) { return fail(pl, e); }
    catch (const std::exception& e) { return fail(pl, MraError(MRA_ERR_INVALID, e.what())); }
    catch (...) { return fail(pl, MraError(MRA_ERR_INVALID, "unknown C++ exception")); }
}
// argument checks of the exports, inside guarded(): the message names the function
static void require(bool ok, const char* msg) { if (!ok) throw MraError(MRA_ERR_INVALID, msg); }

// ---- inputs and results in padded leaf order (the exports, their caller-order variants and the one-call constructor) ----------
// X = A Xraw on the plan's stream, finished before the call returns (the uploads around it are synchronous copies)
static void metric_transform_X(mra_plan* pl) {
    mra_metric_apply(pl);
    if (!g_dry) { HIP_TRY(hipGetLastError()); HIP_TRY(hipStreamSynchronize(pl->stream)); }
}

// a device-to-device copy of n doubles ordered with the transform: on the plan's stream, finished before the call returns
static void metric_copy(mra_plan* pl, double* dst, const double* src, size_t n) {
    if (g_dry) { memcpy(dst, src, n * sizeof(double)); return; }
    HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToDevice, pl->stream));
    HIP_TRY(hipStreamSynchronize(pl->stream));
}

static void set_locs(mra_plan* pl, const double* locs) {
    // (every row the kernels read is one of these P, phantom padding rows included; refused before anything changes)
    // (d = 1 plans never have that kernel - mra_plan_set_kernel refuses it - and pay nothing for it)
    const double last_min = pl->d >= 2 ? last_column_min(locs, pl->P, pl->d) : 0.0;
    if (pl->have_kernel && pl->kp.mode == 6) require_ranges("mra_plan_set_locs", last_min);
    pl->last_col_min = last_min;
    HIP_TRY(mraSetDevice(pl->device));
    pl->slv.valid = false;
    prior_keep_reset(pl);
    // (a plan with a metric keeps the caller's coordinates in Xraw; X and the knot coordinates are A x)
    HIP_TRY(mraMemcpy(pl->metric_on ? pl->Xraw.p : pl->X.p, locs, (size_t)pl->P * pl->d * sizeof(double), hipMemcpyHostToDevice));
    if (pl->metric_on) metric_transform_X(pl);
    if (!pl->knots_pending) set_knot_coords(pl, locs);
    pl->have_locs = true;
}

// mra_plan_set_metric.  A: d x d row-major, nullptr: no metric.  Everything is checked before anything changes.
static void set_metric(mra_plan* pl, const double* A) {
    if (!pl->have_locs) throw MraError(MRA_ERR_STATE, "mra_plan_set_metric needs mra_plan_set_locs first (the metric transforms the plan's coordinates)");
    const int d = pl->d;
    if (A) {
        for (int k = 0; k < d * d; ++k)
            if (!std::isfinite(A[k])) throw MraError(MRA_ERR_INVALID, "mra_plan_set_metric: an entry of A is not finite");
        const double det = d == 1 ? A[0] : d == 2 ? A[0] * A[3] - A[1] * A[2]
                         : A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
        if (!(std::isfinite(det) && det != 0.0)) throw MraError(MRA_ERR_INVALID, "mra_plan_set_metric: A is singular (its determinant is 0 or not finite)");
        if (pl->host_cov) throw MraError(MRA_ERR_INVALID, "mra_plan_set_metric: MRA_KERNEL_HOST plans never read coordinates (apply the metric in the callable)");
        if (pl->have_kernel && pl->kp.circular) throw MraError(MRA_ERR_INVALID, "mra_plan_set_metric: the kernel is circular (the torus has period 1 in the raw coordinate)");
        if (pl->have_kernel && pl->kp.mode == 6) throw MraError(MRA_ERR_INVALID, "mra_plan_set_metric: the kernel is MRA_KERNEL_LOCAL (A would mix the range column into the distance)");
    }
    HIP_TRY(mraSetDevice(pl->device));
    pl->slv.valid = false;
    prior_keep_reset(pl);
    if (!A && !pl->metric_on) return;
    const size_t n = (size_t)pl->P * d;
    if (A) {
        if (!pl->metric_on) {
            // the first metric: the caller's coordinates move to an array of their own, and the raw knot coordinates of the fused
            // levels come back to the host once (the plan retains no host locations)
            pl->Xraw.alloc(n);
            metric_copy(pl, pl->Xraw.p, pl->X.p, n);
            pl->metric_on = true;
            if (pl->regular && !pl->knots_pending) {
                std::vector<double> raw(n);
                HIP_TRY(mraMemcpy(raw.data(), pl->Xraw.p, n * sizeof(double), hipMemcpyDeviceToHost));
                std::copy(A, A + d * d, pl->metric_A);
                metric_transform_X(pl);
                set_knot_coords(pl, raw.data());         // (keeps knot_raw, sends the transformed knots)
                return;
            }
        }
        std::copy(A, A + d * d, pl->metric_A);
        metric_transform_X(pl);
        upload_knot_coords(pl);
    } else {
        metric_copy(pl, pl->X.p, pl->Xraw.p, n);
        pl->metric_on = false;
        upload_knot_coords(pl);                          // (metric off: the raw knots as they are)
        pl->Xraw.release();
        pl->knot_raw.clear(); pl->knot_raw.shrink_to_fit();
    }
}

static void set_obs(mra_plan* pl, const double* y, double R) {
    if (!(R > 0.0)) throw MraError(MRA_ERR_INVALID, "R must be a positive scalar");
    HIP_TRY(mraSetDevice(pl->device));
    HIP_TRY(mraMemcpy(pl->y.p, y, (size_t)pl->P * sizeof(double), hipMemcpyHostToDevice));
    pl->R = R;
    pl->noise_on = false;               // a noise vector belongs to the mask it was checked against: the scalar holds again
    if (pl->host_cov) {
        // host-evaluated covariance blocks are per observed row: a new observation pattern invalidates them (and
        // build_leaf rebuilds the leaf descriptors without their Csrc pointers).  The caller has to select
        // MRA_KERNEL_HOST and upload the blocks again; until then mra_run reports MRA_ERR_STATE.
        pl->host_cov = false;
        pl->have_kernel = false;
        pl->covsrc.release();
        pl->covdiag.release();
        for (auto& lv : pl->lev)
            if (!lv.nodes.empty()) {
                for (auto& g : lv.hResid) { g.Csrc = nullptr; g.ldcs = 0; }
                lv.gResid.upload(lv.hResid);
            }
    }
    // the prior of the last pass stands (it does not depend on y or R), but W "at the observed rows" was at the old mask's
    if (pl->keep.rows == mra_plan::PriorKeep::Rows::Observed) pl->keep.rows = mra_plan::PriorKeep::Rows::None;
    // ... and the leaves' kept residual stands where the observed-row list does (new y on the old mask)
    std::vector<int> standing;
    standing.swap(pl->obs_list_host);
    build_leaf(pl, y);
    if (standing != pl->obs_list_host) pl->rkeep = mra_plan::ResidKeep();
    pl->have_obs = true;
}

// the diag_add of every leaf residual problem, in place: gLeafResid (the host-covariance problems included), gLeafResidLik and their
// sorted copies
void mra_set_leaf_diag_add(mra_plan* pl, double v) {
    for (auto& g : pl->hLeafResid) g.diag_add = v;
    for (auto& g : pl->hLeafResidLik) g.diag_add = v;
    pl->gLeafResid.fill(pl->hLeafResid); pl->gLeafResidLik.fill(pl->hLeafResidLik);
    if (pl->gLeafResidSorted.n) pl->gLeafResidSorted.fill(in_order(pl->hLeafResid, pl->leaf_order));
    if (pl->gLeafResidLikSorted.n) pl->gLeafResidLikSorted.fill(in_order(pl->hLeafResidLik, pl->leaf_order));
}

// r: P noise variances by padded row, read at observed rows only (nullptr: back to the scalar of the last set_obs).  Every value is
// checked before anything changes.  y, the mask, the leaf lists and the options stay; the retained factors do not.
static void set_noise(mra_plan* pl, const double* r) {
    if (!pl->have_obs) throw MraError(MRA_ERR_STATE, "mra_plan_set_noise needs mra_plan_set_obs first (the noise is read at the observed rows)");
    const long P = pl->P;
    // observed: a finite y inside a leaf (rows outside every leaf - dropped by a 1-D split, orphan knot rows of a shard - are nobody's)
    std::vector<unsigned char> seen((size_t)P, 0);
    if (r) {
        for (size_t t = 0; t < pl->leaf_nodes.size(); ++t)
            for (long p = pl->row0[pl->leaf_nodes[t]]; p < pl->row1[pl->leaf_nodes[t]]; ++p) seen[p] = pl->y_finite_host[p];
        for (long p = 0; p < P; ++p)
            if (seen[p] && !(std::isfinite(r[p]) && r[p] >= 0.0))
                throw MraError(MRA_ERR_INVALID, "mra_plan_set_noise: the noise variance of an observed row is negative or not finite");
    }
    HIP_TRY(mraSetDevice(pl->device));
    pl->slv.valid = false;
    if (!r) {
        if (pl->noise_on) { mra_set_leaf_diag_add(pl, pl->R); pl->noise_on = false; }
        return;
    }
    std::vector<double> sd((size_t)P);
    pl->noise_host.assign((size_t)P, 0.0);
    parallel_rows(P, [&](int64_t a, int64_t b) {
        for (int64_t p = a; p < b; ++p) {
            if (seen[p]) pl->noise_host[p] = r[p];
            sd[p] = std::sqrt(pl->noise_host[p]);
        }
    });
    if (pl->noise.n != (size_t)P) { pl->noise.alloc((size_t)P); pl->noise_sd.alloc((size_t)P); }
    HIP_TRY(mraMemcpy(pl->noise.p, pl->noise_host.data(), (size_t)P * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(mraMemcpy(pl->noise_sd.p, sd.data(), (size_t)P * sizeof(double), hipMemcpyHostToDevice));
    if (!pl->noise_on) mra_set_leaf_diag_add(pl, 0.0);
    pl->noise_on = true;
}

static void get_predict(mra_plan* pl, double* mean, double* var) {
    if (!pl->ran || !(pl->run_flags & MRA_RUN_PREDICT)) throw MraError(MRA_ERR_STATE, "mra_run with MRA_RUN_PREDICT has not completed");
    HIP_TRY(mraSetDevice(pl->device));
    HIP_TRY(mraMemcpy(mean, pl->mean.p, (size_t)pl->P * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(mraMemcpy(var, pl->var.p, (size_t)pl->P * sizeof(double), hipMemcpyDeviceToHost));
}

// mean, var (and sd when not NULL) in the caller's row order
static void get_predict_rows(mra_plan* pl, const int64_t* perm, const uint8_t* in_leaf, int64_t N, double* mean, double* var, double* sd) {
    PlanTrace tr("get_predict_rows");
    std::lock_guard<std::mutex> lock(g_stage_mutex);
    double* st = stage_buffer((size_t)pl->P * 2);
    tr.mark("staging buffer");
    get_predict(pl, st, st + pl->P);
    tr.mark("D2H mean, var");
    const double* mp = st; const double* vp = st + pl->P;
    // rows that no leaf reports (dropped by a partition, or another rank's) read 0 - written only when there are such rows
    std::atomic<int64_t> covered{0};
    parallel_rows(pl->P, [&](int64_t a, int64_t b) {
        int64_t c = 0;
        for (int64_t p = a; p < b; ++p) c += (in_leaf[p] && perm[p] >= 0 && perm[p] < N) ? 1 : 0;
        covered += c;
    });
    if (covered.load() != N) {
        parallel_rows(N, [&](int64_t a, int64_t b) { for (int64_t i = a; i < b; ++i) { mean[i] = 0.0; var[i] = 0.0; if (sd) sd[i] = 0.0; } });
        tr.mark("zero the caller's arrays");
    }
    // every caller row sits in at most one padded row, so the scatter has no write conflicts between threads
    parallel_rows(pl->P, [&](int64_t a, int64_t b) {
        for (int64_t p = a; p < b; ++p) if (in_leaf[p]) {
            const int64_t i = perm[p];
            if (i >= 0 && i < N) { mean[i] = mp[p]; var[i] = vp[p]; if (sd) sd[i] = std::sqrt(vp[p]); }
        }
    });
}

// ---- native tree replay (host only, no GPU needed) ---------------------------------------------------
struct mra_tree { mra_topo::Result r; };

// The replay behind the three replay exports; the tree is handed out only when the replay succeeds (nullptr: not a large-2-D tree).
// perm, src, in_leaf, knot_rows: the caller's arrays that the replay fills in place, or all nullptr.
static std::unique_ptr<mra_tree> replay_tree(const double* locs, int64_t N, int32_t r, int32_t M, uint32_t* mt_key, int32_t* mt_pos,
                                             int64_t* perm = nullptr, int64_t* src = nullptr, uint8_t* in_leaf = nullptr,
                                             int64_t* knot_rows = nullptr, mra_topo::LayoutHook hook = nullptr, void* hook_user = nullptr) {
    std::unique_ptr<mra_tree> t(new mra_tree());
    t->r.ext_perm = perm; t->r.ext_src = src; t->r.ext_in_leaf = in_leaf; t->r.ext_knot_rows = knot_rows;
    if (mra_topo::replay_quadtree(locs, N, r, M, mt_key, mt_pos, t->r, hook, hook_user) != 0) t.reset();
    return t;
}

// ---- MRATree.__init__ for large 2-D trees in one call ---------------------------------------------------------------------------
// The tree replay and the plan construction of an end-to-end MRATree(...) call, overlapped: as soon as the replay has the
// partition and the row layout (everything but the knots), a helper thread sizes and allocates the plan, gathers and uploads the
// locations and the observations and builds the leaf descriptors - while the caller's thread is still drawing knots, the one
// sequential part (it has to consume NumPy's MT19937 stream in the reference's order).  The knot rows, the leaves' knot
// counts and the knot coordinates go in when both are done.
namespace {
struct ReplayPlanCtx {
    const double* locs; const double* y; double R; int device;
    PlanPtr pl;                       // destroyed with the context unless mra_plan_create_replay_2d hands it out
    int rc = MRA_OK;
    std::string err;
};
// (runs on a helper thread of the replay and must not throw: a failure reaches the caller's thread as rc and err)
void replay_plan_hook(void* user, const mra_topo::Result& t) {
    ReplayPlanCtx& c = *(ReplayPlanCtx*)user;
    c.rc = guarded(nullptr, [&] {
        PlanTrace tr("plan beside the knot draws");
        PlanPtr pl = new_plan(c.device);
        pl->knots_pending = true;
        pl->P = t.P; pl->d = 2; pl->n_levels = t.n_levels; pl->n_nodes = t.n_nodes;
        pl->level_ptr.assign(t.level_ptr.begin(), t.level_ptr.end());
        pl->row0.assign(t.row0.begin(), t.row0.end());
        pl->row1.assign(t.row1.begin(), t.row1.end());
        pl->leaf.assign(t.leaf.begin(), t.leaf.end());
        pl->parent.assign(t.parent.begin(), t.parent.end());
        pl->child_ptr.assign(t.child_ptr.begin(), t.child_ptr.end());
        pl->child_list.assign(t.child_list.begin(), t.child_list.end());
        pl->knot_ptr.assign(t.knot_ptr.begin(), t.knot_ptr.end());      // non-leaf nodes final; the leaves' entries are provisional
        pl->cw.assign(t.cw.begin(), t.cw.end());
        tr.mark("streams, events, arena, copies of the topology");
        const int64_t* src = t.ext_perm ? t.ext_src : t.src.data();
        const int64_t* perm = t.ext_perm ? t.ext_perm : t.perm.data();
        std::lock_guard<std::mutex> lock(g_stage_mutex);
        double* xp = stage_buffer((size_t)pl->P * 3);
        double* yp = xp + (size_t)pl->P * 2;
        // the gather of locations and observations into leaf order runs beside build_static (neither needs the other)
        const long P = pl->P;
        bool gather_failed = false;
        std::thread gather([&, P]() {
            const double nan = std::nan("");
            const double* locs = c.locs; const double* y = c.y;
            try {
                parallel_rows(P, [&](int64_t a, int64_t b) {
                    for (int64_t p = a; p < b; ++p) {
                        const int64_t q = src[p];
                        xp[2 * p] = locs[2 * q]; xp[2 * p + 1] = locs[2 * q + 1];
                        yp[p] = perm[p] < 0 ? nan : y[q];
                    }
                });
            } catch (...) { gather_failed = true; }
        });
        struct Join { std::thread& t; ~Join() { if (t.joinable()) t.join(); } } join{gather};
        build_static(pl.get());
        tr.mark("build_static");
        gather.join();
        if (gather_failed) throw MraError(MRA_ERR_INVALID, "gathering locations / observations failed (thread creation)");
        tr.mark("(gather of locations and observations: beside it)");
        set_locs(pl.get(), xp);
        set_obs(pl.get(), yp, c.R);
        tr.mark("uploads, leaf descriptors");
        c.pl = std::move(pl);
        return MRA_OK;
    });
    if (c.rc != MRA_OK) c.err = g_last_error;                // (this thread's)
}
}  // namespace

// ------------------------------------------------------------------------------------------------
//  C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char* mra_version(void) { return MRA_VERSION_STR; }

const char* mra_last_error(mra_plan* plan) { return plan ? plan->err.c_str() : g_last_error.c_str(); }

int mra_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mra_plan_create(mra_plan** out, const mra_topology* t, int device) {
    return guarded(nullptr, [&] {
        require(out && t, "mra_plan_create: out or topology is NULL");
        *out = nullptr;
        if (t->P <= 0 || t->d < 1 || t->d > 3 || t->n_levels <= 0 || t->n_nodes <= 0)
            throw MraError(MRA_ERR_INVALID, "bad topology header");
        PlanTrace tr("mra_plan_create");
        PlanPtr pl = new_plan(device);
        tr.mark("streams, events, arena");
        pl->P = t->P; pl->d = t->d; pl->n_levels = t->n_levels; pl->n_nodes = t->n_nodes;
        pl->level_ptr.assign(t->level_ptr, t->level_ptr + t->n_levels + 1);
        pl->row0.assign(t->node_row0, t->node_row0 + t->n_nodes);
        pl->row1.assign(t->node_row1, t->node_row1 + t->n_nodes);
        pl->leaf.assign(t->node_leaf, t->node_leaf + t->n_nodes);
        pl->parent.assign(t->node_parent, t->node_parent + t->n_nodes);
        pl->child_ptr.assign(t->child_ptr, t->child_ptr + t->n_nodes + 1);
        pl->child_list.assign(t->child_list, t->child_list + pl->child_ptr.back());
        pl->knot_ptr.assign(t->knot_ptr, t->knot_ptr + t->n_nodes + 1);
        pl->knot_rows.assign(t->knot_rows, t->knot_rows + pl->knot_ptr.back());
        pl->cw.assign(t->cw, t->cw + t->n_levels);
        if (pl->level_ptr[0] != 0 || pl->level_ptr.back() != t->n_nodes) throw MraError(MRA_ERR_INVALID, "level_ptr inconsistent");
        tr.mark("copies of the topology");
        build_static(pl.get());
        *out = pl.release();
        return MRA_OK;
    });
}

int mra_plan_destroy(mra_plan* pl) { return guarded(nullptr, [&] { destroy_plan(pl); return MRA_OK; }); }     // (pl->err dies with pl)

int mra_release_cached_memory(void) {
    return guarded(nullptr, [&] {
        mra_topo::release_scratch();                      // the tree replay's work arrays (~100 MB at 1024^2, ~0.5 GB at config 5)
        if (g_dry) return MRA_OK;
        {
            std::lock_guard<std::mutex> lock(g_streams_mu);
            for (auto& e : g_streams) { hipStreamDestroy(e.second.hi); hipStreamDestroy(e.second.lo); if (e.second.host_res) hipHostFree(e.second.host_res); if (e.second.arena_host) hipHostFree(e.second.arena_host); }
            g_streams.clear();
        }
        {
            std::lock_guard<std::mutex> lock(g_stage_mutex);
            if (g_stage) { hipHostFree(g_stage); g_stage = nullptr; g_stage_n = 0; }
        }
        std::lock_guard<std::mutex> lock(g_pool.mu);
        g_pool.flush_locked();
        return MRA_OK;
    });
}

int mra_plan_set_locs(mra_plan* pl, const double* locs) {
    return guarded(pl, [&] { require(pl && locs, "mra_plan_set_locs: plan or locs is NULL"); set_locs(pl, locs); return MRA_OK; });
}

// ---- caller-order variants (helpers above the extern "C" block)
int mra_plan_set_locs_rows(mra_plan* pl, const double* locs, const int64_t* src) {
    return guarded(pl, [&] {
        require(pl && locs && src, "mra_plan_set_locs_rows: plan, locs or src is NULL");
        PlanTrace tr("set_locs_rows");
        std::lock_guard<std::mutex> lock(g_stage_mutex);
        const int d = pl->d;
        double* xp = stage_buffer((size_t)pl->P * d);
        tr.mark("staging buffer");
        parallel_rows(pl->P, [&](int64_t a, int64_t b) {
            if (d == 2) for (int64_t p = a; p < b; ++p) { const int64_t q = src[p]; xp[2 * p] = locs[2 * q]; xp[2 * p + 1] = locs[2 * q + 1]; }
            else if (d == 1) for (int64_t p = a; p < b; ++p) xp[p] = locs[src[p]];
            else for (int64_t p = a; p < b; ++p) { const int64_t q = src[p]; for (int e = 0; e < d; ++e) xp[d * p + e] = locs[d * q + e]; }
        });
        tr.mark("gather into leaf order");
        set_locs(pl, xp);
        tr.mark("upload X, knot coordinates");
        return MRA_OK;
    });
}

int mra_plan_set_obs_rows(mra_plan* pl, const double* y, const int64_t* src, const int64_t* perm, double R) {
    return guarded(pl, [&] {
        require(pl && y && src && perm, "mra_plan_set_obs_rows: plan, y, src or perm is NULL");
        PlanTrace tr("set_obs_rows");
        std::lock_guard<std::mutex> lock(g_stage_mutex);
        double* yp = stage_buffer((size_t)pl->P);
        const double nan = std::nan("");
        parallel_rows(pl->P, [&](int64_t a, int64_t b) { for (int64_t p = a; p < b; ++p) yp[p] = perm[p] < 0 ? nan : y[src[p]]; });
        tr.mark("gather into leaf order");
        set_obs(pl, yp, R);
        tr.mark("upload y, build_leaf");
        return MRA_OK;
    });
}

int mra_get_predict_rows(mra_plan* pl, const int64_t* perm, const uint8_t* in_leaf, int64_t N, double* mean, double* var) {
    return guarded(pl, [&] {
        require(pl && perm && in_leaf && mean && var && N > 0, "mra_get_predict_rows: plan, perm, in_leaf, mean or var is NULL, or N <= 0");
        get_predict_rows(pl, perm, in_leaf, N, mean, var, nullptr);
        return MRA_OK;
    });
}

int mra_get_predict_rows_sd(mra_plan* pl, const int64_t* perm, const uint8_t* in_leaf, int64_t N, double* mean, double* var, double* sd) {
    return guarded(pl, [&] {
        require(pl && perm && in_leaf && mean && var && N > 0, "mra_get_predict_rows_sd: plan, perm, in_leaf, mean or var is NULL, or N <= 0");
        get_predict_rows(pl, perm, in_leaf, N, mean, var, sd);
        return MRA_OK;
    });
}

int mra_plan_set_metric(mra_plan* pl, const double* A) {
    return guarded(pl, [&] { require(pl, "mra_plan_set_metric: plan is NULL"); set_metric(pl, A); return MRA_OK; });
}

int mra_plan_set_obs(mra_plan* pl, const double* y, double R) {
    return guarded(pl, [&] { require(pl && y, "mra_plan_set_obs: plan or y is NULL"); set_obs(pl, y, R); return MRA_OK; });
}

int mra_plan_set_noise(mra_plan* pl, const double* r_perm) {
    return guarded(pl, [&] { require(pl, "mra_plan_set_noise: plan is NULL"); set_noise(pl, r_perm); return MRA_OK; });
}

int mra_plan_set_noise_rows(mra_plan* pl, const double* r, const int64_t* src) {
    return guarded(pl, [&] {
        require(pl && r && src, "mra_plan_set_noise_rows: plan, r or src is NULL");
        std::lock_guard<std::mutex> lock(g_stage_mutex);
        double* rp = stage_buffer((size_t)pl->P);
        parallel_rows(pl->P, [&](int64_t a, int64_t b) { for (int64_t p = a; p < b; ++p) rp[p] = r[src[p]]; });
        set_noise(pl, rp);
        return MRA_OK;
    });
}

int mra_plan_fit_laplace(mra_plan* pl, int family, const double* z_perm, const double* aux_perm, const double* offset_perm, const double* x0_perm,
                         int max_iter, double tol, double* info) {
    return guarded(pl, [&] {
        require(pl, "mra_plan_fit_laplace: plan is NULL");
        mra_fit_laplace(pl, family, z_perm, aux_perm, offset_perm, x0_perm, max_iter, tol, info);
        return MRA_OK;
    });
}

int mra_plan_set_kernel(mra_plan* pl, int kind, const double* params, int n) {
    return guarded(pl, [&] {
        require(pl, "mra_plan_set_kernel: plan is NULL");
        if (pl->metric_on && kind == MRA_KERNEL_HOST)
            throw MraError(MRA_ERR_INVALID, "mra_plan_set_kernel: MRA_KERNEL_HOST on a plan with a metric (such plans never read coordinates; mra_plan_set_metric(NULL) first)");
        if (pl->metric_on && kind != MRA_KERNEL_HOST && params && n >= 4 && params[3] != 0.0)
            throw MraError(MRA_ERR_INVALID, "mra_plan_set_kernel: circular distances on a plan with a metric (the torus has period 1 in the raw coordinate)");
        if (kind != MRA_KERNEL_HOST) {       // refusals leave the previous kernel and everything retained in place
            require(params, "mra_plan_set_kernel: params is NULL");
            check_kernel_params("mra_plan_set_kernel", kind, params, n);
            if (!(params[0] > 0.0)) throw MraError(MRA_ERR_INVALID, "length scale must be positive");
            if (n >= 4 && params[3] != 0.0 && pl->d != 1) throw MraError(MRA_ERR_INVALID, "circular distances are defined for 1-D locations only");
            if (kind == MRA_KERNEL_LOCAL) {
                if (pl->d < 2) throw MraError(MRA_ERR_INVALID, "mra_plan_set_kernel: MRA_KERNEL_LOCAL needs d = 2 (x, range) or d = 3 (x, y, range) coordinates");
                if (pl->metric_on) throw MraError(MRA_ERR_INVALID, "mra_plan_set_kernel: MRA_KERNEL_LOCAL on a plan with a metric (A would mix the range column into the distance; mra_plan_set_metric(NULL) first)");
                if (pl->have_locs) require_ranges("mra_plan_set_kernel", pl->last_col_min);
            }
        } else if (!pl->have_obs) throw MraError(MRA_ERR_STATE, "MRA_KERNEL_HOST needs mra_plan_set_obs first (leaf blocks are per observed row)");
        // every refusal is above: from here on the call goes through
        pl->slv.valid = false;
        prior_keep_reset(pl);                // on every call: the values are not compared
        if (kind == MRA_KERNEL_HOST) {
            HIP_TRY(mraSetDevice(pl->device));
            // one padded block per node: non-leaf N_j x cw, leaf N_j x nop; leaves also C(x,x) per row
            pl->cov_off.assign(pl->n_nodes + 1, 0);
            for (int i = 0; i < pl->n_nodes; ++i) {
                const long nr = pl->row1[i] - pl->row0[i];
                const long ld = pl->leaf[i] ? pl->leaf_nop[pl->leaf_slot[i]] : pl->cw[pl->node_level[i]];
                pl->cov_off[i + 1] = pl->cov_off[i] + nr * ld;
            }
            pl->covsrc.alloc(std::max<long>(pl->cov_off.back(), 1));
            pl->covdiag.alloc(pl->P);
            HIP_TRY(mraMemset(pl->covsrc.p, 0, pl->covsrc.n * sizeof(double)));
            HIP_TRY(mraMemset(pl->covdiag.p, 0, pl->covdiag.n * sizeof(double)));
            for (int m = 0; m < pl->n_levels; ++m) {
                LevelData& lv = pl->lev[m];
                for (size_t sl = 0; sl < lv.nodes.size(); ++sl) {
                    lv.hResid[sl].Csrc = pl->covsrc.p + pl->cov_off[lv.nodes[sl]];
                    lv.hResid[sl].ldcs = lv.cw;
                }
                if (!lv.nodes.empty()) lv.gResid.upload(lv.hResid);
            }
            for (size_t t = 0; t < pl->leaf_nodes.size(); ++t) {
                pl->hLeafResid[t].Csrc = pl->covsrc.p + pl->cov_off[pl->leaf_nodes[t]];
                pl->hLeafResid[t].ldcs = pl->leaf_nop[t];
            }
            if (!pl->leaf_nodes.empty()) pl->gLeafResid.upload(pl->hLeafResid);
            pl->kp = KernelParams{};
            pl->host_cov = true;
            pl->have_kernel = true;
            return MRA_OK;
        }
        if (kind == MRA_KERNEL_MATERN && (pl->nu_tab.n == 0 || pl->nu_tab_nu != params[4])) {      // a change of l, sig or scale uploads nothing
            HIP_TRY(mraSetDevice(pl->device));
            pl->nu_tab.upload(matern_nu_table(params[4]));
            pl->nu_tab_nu = params[4];
        }
        pl->kp.nu = kind == MRA_KERNEL_MATERN ? params[4] : 0.0; pl->kp.nu_a = 0.0;
        pl->kp.nu_tab = kind == MRA_KERNEL_MATERN ? pl->nu_tab.p : nullptr;
        pl->kp.nu_n = kind == MRA_KERNEL_MATERN ? MRA_NU_NODES : 0;
        pl->kp.kind = kind; pl->kp.d = pl->d; pl->kp.l = params[0]; pl->kp.sig = params[1]; pl->kp.scale = params[2];
        pl->kp.circular = (n >= 4 && params[3] != 0.0) ? 1 : 0;
        if (kind == MRA_KERNEL_SUM) {        // the records go up on every call (at most 192 bytes), behind whatever the stream still runs
            HIP_TRY(mraSetDevice(pl->device));
            if (pl->sum_tab.n == 0) pl->sum_tab.alloc((size_t)MRA_SUM_REC * MRA_SUM_MAX + 1);
            std::vector<double> rec = sum_records(pl->kp, params);
            rec.push_back(pl->kp.amp);       // behind the records, for mra_get_buffer(17): no kernel reads it
            HIP_TRY(mraMemcpy(pl->sum_tab.p, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice));
            pl->kp.nu_tab = pl->sum_tab.p;
        } else if (kind == MRA_KERNEL_LOCAL) derive_local_params(pl->kp, params);
        else derive_kernel_params(pl->kp);
        pl->host_cov = false;
        pl->have_kernel = true;
        return MRA_OK;
    });
}

int mra_plan_set_cov_block(mra_plan* pl, int32_t node, const double* C, int64_t n_rows, int64_t n_cols, const double* diag) {
    return guarded(pl, [&] {
        require(pl && C, "mra_plan_set_cov_block: plan or C is NULL");
        pl->slv.valid = false;
        prior_keep_reset(pl);
        if (!pl->host_cov) throw MraError(MRA_ERR_STATE, "select MRA_KERNEL_HOST with mra_plan_set_kernel first");
        if (node < 0 || node >= pl->n_nodes) throw MraError(MRA_ERR_INVALID, "node out of range");
        HIP_TRY(mraSetDevice(pl->device));
        const long nr = pl->row1[node] - pl->row0[node];
        long ld, want_cols;
        if (pl->leaf[node]) {
            const int t = pl->leaf_slot[node];
            ld = pl->leaf_nop[t]; want_cols = pl->leaf_nobs_host[t];
            if (!diag) throw MraError(MRA_ERR_INVALID, "leaf blocks need diag (C(x,x) per row)");
        } else {
            ld = pl->cw[pl->node_level[node]]; want_cols = pl->knot_ptr[node + 1] - pl->knot_ptr[node];
        }
        if (n_rows != nr || n_cols != want_cols) {
            char b[200];
            snprintf(b, sizeof b, "block of node %d must be %ld x %ld (got %ld x %ld)", node, nr, want_cols, (long)n_rows, (long)n_cols);
            throw MraError(MRA_ERR_INVALID, b);
        }
        if (n_cols > 0)
            HIP_TRY(mraMemcpy2D(pl->covsrc.p + pl->cov_off[node], ld * sizeof(double), C, n_cols * sizeof(double),
                                n_cols * sizeof(double), nr, hipMemcpyHostToDevice));
        if (diag) HIP_TRY(mraMemcpy(pl->covdiag.p + pl->row0[node], diag, nr * sizeof(double), hipMemcpyHostToDevice));
        return MRA_OK;
    });
}

int mra_run(mra_plan* pl, uint32_t flags) {
    return guarded(pl, [&] {
        require(pl, "mra_run: plan is NULL");
        if (!(flags & (MRA_RUN_LIKELIHOOD | MRA_RUN_PREDICT))) throw MraError(MRA_ERR_INVALID, "flags must request likelihood and/or predict");
        mra_run_all(pl, flags);
        return MRA_OK;
    });
}

int mra_run_resume(mra_plan* pl) {
    return guarded(pl, [&] {
        require(pl, "mra_run_resume: plan is NULL");
        if (!pl->split_pending) throw MraError(MRA_ERR_STATE, "no split run pending");
        HIP_TRY(mraSetDevice(pl->device));
        run_fronts_and_predict(pl, pl->reduce_level, true);
        return MRA_OK;
    });
}

int mra_sample_slots(mra_plan* pl, int64_t* n_slots) {
    return guarded(pl, [&] {
        require(pl && n_slots, "mra_sample_slots: plan or n_slots is NULL");
        *n_slots = mra_coarse_slots(pl, nullptr) + 2 * pl->P;
        return MRA_OK;
    });
}

int mra_sample(mra_plan* pl, uint32_t flags, int64_t n_samples, uint64_t seed, int64_t sample0, const double* z, double* out) {
    return guarded(pl, [&] { require(pl, "mra_sample: plan is NULL"); sample_all(pl, flags, n_samples, seed, sample0, z, out); return MRA_OK; });
}

int mra_solve(mra_plan* pl, uint32_t flags, int64_t n_cols, const double* Y, double* mean, double* quad) {
    return guarded(pl, [&] { require(pl, "mra_solve: plan is NULL"); mra_solve_all(pl, flags, n_cols, Y, mean, quad); return MRA_OK; });
}
int mra_plan_fit_laplace_trend(mra_plan* pl, int family, const double* z_perm, const double* aux_perm, const double* offset_perm,
                               const double* e0_perm, int max_iter, double tol, double* beta, double* cov_beta, double* info) {
    return guarded(pl, [&] {
        require(pl, "mra_plan_fit_laplace_trend: plan is NULL");
        mra_fit_laplace_trend(pl, family, z_perm, aux_perm, offset_perm, e0_perm, max_iter, tol, beta, cov_beta, info);
        return MRA_OK;
    });
}
int mra_plan_set_trend(mra_plan* pl, int32_t p, const double* X_perm) {
    return guarded(pl, [&] { require(pl, "mra_plan_set_trend: plan is NULL"); mra_trend_set(pl, p, X_perm); return MRA_OK; });
}
int mra_trend_fit(mra_plan* pl, uint32_t flags, double* beta, double* cov_beta, double* mean_perm, double* var_perm, double* info) {
    return guarded(pl, [&] { require(pl, "mra_trend_fit: plan is NULL"); mra_trend_fit_all(pl, flags, beta, cov_beta, mean_perm, var_perm, info); return MRA_OK; });
}
int mra_cov_apply(mra_plan* pl, uint32_t flags, int64_t n_cols, const double* A, double* out, double* gram) {
    return guarded(pl, [&] { require(pl, "mra_cov_apply: plan is NULL"); mra_cov_all(pl, flags, n_cols, A, out, gram); return MRA_OK; });
}

int mra_predict_sites(mra_plan* pl, uint32_t flags, int64_t n_sites, const double* sites, const int32_t* leaf, int64_t n_cols, const double* Y,
                      double* mean, double* var) {
    return guarded(pl, [&] { require(pl, "mra_predict_sites: plan is NULL"); mra_predict_sites_all(pl, flags, n_sites, sites, leaf, n_cols, Y, mean, var); return MRA_OK; });
}

int mra_sites_cov(mra_plan* pl, uint32_t flags, int64_t n_sites, const double* sites, const int32_t* leaf, double* out) {
    return guarded(pl, [&] { require(pl, "mra_sites_cov: plan is NULL"); mra_sites_cov_all(pl, flags, n_sites, sites, leaf, out); return MRA_OK; });
}

int mra_sample_sites_slots(mra_plan* pl, int64_t n_sites, int64_t* n_slots) {
    return guarded(pl, [&] {
        require(pl && n_slots, "mra_sample_sites_slots: plan or n_slots is NULL");
        if (n_sites < 0) throw MraError(MRA_ERR_INVALID, "n_sites < 0");
        *n_slots = mra_coarse_slots(pl, nullptr) + n_sites;
        return MRA_OK;
    });
}

int mra_sample_sites(mra_plan* pl, uint32_t flags, int64_t n_sites, const double* sites, const int32_t* leaf, int64_t n_samples, uint64_t seed,
                     int64_t sample0, const double* z, double* out) {
    return guarded(pl, [&] {
        require(pl, "mra_sample_sites: plan is NULL");
        mra_sample_sites_all(pl, flags, n_sites, sites, leaf, n_samples, seed, sample0, z, out);
        return MRA_OK;
    });
}

int mra_cv(mra_plan* pl, uint32_t flags, double* mean_perm, double* var_perm, double* lpd_perm, double* group_lpd, double* info) {
    return guarded(pl, [&] { require(pl, "mra_cv: plan is NULL"); mra_cv_all(pl, false, flags, mean_perm, var_perm, lpd_perm, group_lpd, info); return MRA_OK; });
}
int mra_cv_trend(mra_plan* pl, uint32_t flags, double* mean_perm, double* var_perm, double* lpd_perm, double* group_lpd, double* info) {
    return guarded(pl, [&] { require(pl, "mra_cv_trend: plan is NULL"); mra_cv_all(pl, true, flags, mean_perm, var_perm, lpd_perm, group_lpd, info); return MRA_OK; });
}

int mra_get_likelihood(mra_plan* pl, double* d, double* u) {
    return guarded(pl, [&] {
        require(pl && d && u, "mra_get_likelihood: plan, d or u is NULL");
        if (!pl->ran) throw MraError(MRA_ERR_STATE, "mra_run has not completed");
        *d = pl->res_d; *u = pl->res_u;
        return MRA_OK;
    });
}

int mra_get_predict(mra_plan* pl, double* mean, double* var) {
    return guarded(pl, [&] { require(pl && mean && var, "mra_get_predict: plan, mean or var is NULL"); get_predict(pl, mean, var); return MRA_OK; });
}

int mra_get_buffer(mra_plan* pl, int what, double* out, int64_t cap, int64_t* n_avail) {
    return guarded(pl, [&] {
        require(pl && n_avail, "mra_get_buffer: plan or n_avail is NULL");
        HIP_TRY(mraSetDevice(pl->device));
        const double* src = nullptr; int64_t n = 0;
        if (what == 7) {             // host record: stream ms of the last mra_predict_sites by kernel (MRA_OPT_KERNEL_TIMING)
            *n_avail = 7;
            if (out && cap > 0) memcpy(out, pl->sit.ms, (size_t)std::min<int64_t>(cap, 7) * sizeof(double));
            return MRA_OK;
        }
        if (what == 8) {             // host record: stream ms of the last mra_sites_cov
            *n_avail = 6;
            if (out && cap > 0) memcpy(out, pl->sit.cov_ms, (size_t)std::min<int64_t>(cap, 6) * sizeof(double));
            return MRA_OK;
        }
        if (what == 9) {             // host record: stream ms of the last mra_sample_sites
            *n_avail = 9;
            if (out && cap > 0) memcpy(out, pl->sit.draw_ms, (size_t)std::min<int64_t>(cap, 9) * sizeof(double));
            return MRA_OK;
        }
        if (what == 12) {            // host record: stream ms of the last mra_cv
            *n_avail = 9;
            if (out && cap > 0) memcpy(out, pl->sit.cv_ms, (size_t)std::min<int64_t>(cap, 9) * sizeof(double));
            return MRA_OK;
        }
        if (what == 15) {            // host record: stream ms of the last mra_cv_trend
            *n_avail = 12;
            if (out && cap > 0) memcpy(out, pl->sit.cvt_ms, (size_t)std::min<int64_t>(cap, 12) * sizeof(double));
            return MRA_OK;
        }
        if (what == 14) {            // host record: stream ms of the last mra_trend_fit
            *n_avail = 7;
            if (out && cap > 0) memcpy(out, pl->trend.ms, (size_t)std::min<int64_t>(cap, 7) * sizeof(double));
            return MRA_OK;
        }
        if (what == 10) {            // host record: the noise variance by padded row (the scalar R everywhere when no vector is set)
            *n_avail = pl->P;
            const int64_t m = std::min<int64_t>(cap, pl->P);
            if (out && m > 0) {
                if (pl->noise_on) memcpy(out, pl->noise_host.data(), (size_t)m * sizeof(double));
                else std::fill(out, out + m, pl->R);
            }
            return MRA_OK;
        }
        if (what == 0) { src = pl->W.p; n = (int64_t)pl->W.n; }
        else if (what == 1) { src = pl->dnode.p; n = (int64_t)pl->dnode.n; }
        else if (what == 2) { src = pl->stamps.p; n = (int64_t)pl->stamps.n; }     // -DMRA_STAMPS builds: raw 64-bit clock stamps
        else if (what == 3) { src = pl->pstamps.p; n = (int64_t)pl->pstamps.n; }
        else if (what == 5) { src = pl->kstamps.p; n = (int64_t)pl->kstamps.n; }   // same, knot chain
        else if (what == 6) { src = pl->kstamps2.p; n = (int64_t)pl->kstamps2.n; } // same, fused leaf solve + update
        else if (what == 4) { src = pl->tstamps.p; n = (int64_t)pl->tstamps.n; }   // same, leaf row solves   // same, predictive cascade
        else if (what == 13) { src = pl->X.p; n = (int64_t)pl->P * pl->d; }         // the coordinates as the kernels read them (A x under mra_plan_set_metric)
        else if (what == 16) { src = pl->kp.nu_tab; n = pl->kp.mode == 4 ? 2 * (int64_t)pl->kp.nu_n : 0; }     // the quadrature table of MRA_KERNEL_MATERN, as the kernels are handed it
        else if (what == 17) { src = pl->kp.nu_tab; n = pl->kp.mode == 5 ? MRA_SUM_REC * (int64_t)pl->kp.nu_n + 1 : 0; }     // the component records of MRA_KERNEL_SUM, then kp.amp
        else if (what == 11) { src = pl->y.p; n = pl->P; }                         // the observations as the device holds them (the pseudo-observations t after mra_plan_fit_laplace)
        else throw MraError(MRA_ERR_INVALID, "unknown buffer id");
        *n_avail = n;
        if (out && cap > 0) HIP_TRY(mraMemcpy(out, src, (size_t)std::min(cap, n) * sizeof(double), hipMemcpyDeviceToHost));
        return MRA_OK;
    });
}

int mra_get_node_block(mra_plan* pl, int32_t node, int what, double* out, int64_t cap, int64_t* n_rows, int64_t* n_cols) {
    return guarded(pl, [&] {
        require(pl && n_rows && n_cols, "mra_get_node_block: plan, n_rows or n_cols is NULL");
        if (node < 0 || node >= pl->n_nodes) throw MraError(MRA_ERR_INVALID, "node out of range");
        if (!pl->ran) throw MraError(MRA_ERR_STATE, "mra_run has not completed");
        HIP_TRY(mraSetDevice(pl->device));
        const int m = pl->node_level[node];
        const double* src = nullptr;
        int64_t rows = 0, cols = 0, ld = 0;
        if (what == MRA_BLOCK_W_ROWS) {
            rows = pl->row1[node] - pl->row0[node]; cols = pl->ldw; ld = pl->ldw;
            src = pl->W.p + pl->row0[node] * (long)pl->ldw;
        } else if (what == MRA_BLOCK_LPRIOR || what == MRA_BLOCK_FRONT) {
            if (pl->leaf[node]) throw MraError(MRA_ERR_INVALID, "block exists for non-leaf nodes only");
            const LevelData& lv = pl->lev[m];
            const size_t sl = (size_t)pl->node_slot[node];
            if (what == MRA_BLOCK_LPRIOR) { rows = cols = ld = lv.cw; src = lv.Lp_of(sl); }
            else {
                if (lv.panel_only) throw MraError(MRA_ERR_STATE, "the fronts of this level are kept as their panel columns only (large fronts of the leaves' parents); "
                                                                  "set MRA_NO_LOWRANK_PARENT=1 before creating the plan to get whole fronts");
                rows = cols = ld = lv.nf; src = lv.F_of(sl);
            }
        } else if (what == MRA_BLOCK_LEAF) {
            if (!pl->leaf[node]) throw MraError(MRA_ERR_INVALID, "block exists for leaves only");
            const int t = pl->leaf_slot[node];
            const int nop = pl->leaf_nop[t];
            rows = nop + pl->na[m] + (pl->row1[node] - pl->row0[node]); cols = ld = nop;
            src = leaf_C(pl, t);
        } else throw MraError(MRA_ERR_INVALID, "unknown block id");
        *n_rows = rows; *n_cols = cols;
        const int64_t n = std::min<int64_t>(cap, rows * cols);
        if (out && n > 0) HIP_TRY(mraMemcpy(out, src, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        (void)ld;
        return MRA_OK;
    });
}

int mra_get_timers(mra_plan* pl, double* out, int cap) {
    if (!pl || !out) return 0;
    int n = std::min(cap, 5);
    for (int k = 0; k < n; ++k) out[k] = pl->phase_ms[k];
    return n;
}

static constexpr int OPT_KERNEL_SHAPE = 99;    // kernel-shape switches for A/B runs (no public name: tools only)

int mra_plan_set_option(mra_plan* pl, int option, int64_t value) {
    return guarded(pl, [&] {
        require(pl, "mra_plan_set_option: plan is NULL");
        // options that change which kernel produces or factorises the leaves' C blocks bring the phantom-row launch back; the others
        // (timing, front / knot / solve / update variants) never touch C
        if (option == MRA_OPT_FUSED || option == MRA_OPT_GEMM_LDS || option == MRA_OPT_LEAF_GEMM || option == MRA_OPT_CHOL_TILES || option == MRA_OPT_RESID_REUSE) pl->cphantom_valid = false;
        if (option != MRA_OPT_KERNEL_TIMING && option != MRA_OPT_SAMPLE_SOLVE && option != MRA_OPT_SITES_CHUNK_BYTES) {
            pl->slv.valid = false;     // the next pass may run other kernels: mra_solve factorises again
            prior_keep_reset(pl);      // ... and its prior stage may leave W, the factors or the variance in another state
        }
        switch (option) {
        case MRA_OPT_KERNEL_TIMING: pl->ktiming = value != 0; return MRA_OK;
        case MRA_OPT_FUSED: pl->use_fused = value != 0; return MRA_OK;
        case MRA_OPT_GEMM_LDS: pl->gemm_lds = value != 0; return MRA_OK;
        case MRA_OPT_FRONT_FUSED: pl->use_front_fused = value != 0; return MRA_OK;
        case MRA_OPT_KNOT_CHAIN: pl->use_knot_chain = value != 0; return MRA_OK;
        case MRA_OPT_LEAF_GEMM: pl->use_leaf_gemm = value != 0; pl->leaf_gemm_update = value == 2; return MRA_OK;
        case MRA_OPT_LEAF_SOLVE: pl->use_leaf_solve = value != 0; pl->leaf_solve_mode = (int)value; return MRA_OK;
        case MRA_OPT_PRED_UPDATE: pl->use_pred_update = value != 0; return MRA_OK;
        case MRA_OPT_LEAF_SOLVE_SPLIT: pl->leaf_solve_split = value == 2 ? 2 : 1; return MRA_OK;
        case MRA_OPT_CHOL_TILES: pl->use_chol_lds = (int)value; return MRA_OK;
        case MRA_OPT_SEG_GEMM_LDS: pl->seg_gemm_lds = value != 0; return MRA_OK;
        case MRA_OPT_SYRK_BLK: pl->use_syrk_blk = (int)value; return MRA_OK;
        case MRA_OPT_PRIOR_LEVEL: pl->use_prior_level = value != 0; return MRA_OK;
        case MRA_OPT_HI_FOLD: pl->use_hi_fold = (int)value; return MRA_OK;
        case MRA_OPT_LIK_ROWS: pl->use_lik_rows = value != 0; return MRA_OK;
        case MRA_OPT_UT_GATHER: pl->ut_gather = value != 0; return MRA_OK;
        case MRA_OPT_LEAF_ORDER:
            if (value < 0 || value > 4) throw MraError(MRA_ERR_INVALID, "option 22: 0, 1, 2 (the fork alone), 3 (the order alone) or 4 (1 and the residual product in that order)");
            pl->use_leaf_fork = value == 1 || value == 2 || value == 4;
            pl->leaf_longest_first = value == 1 || value == 3 || value == 4;
            pl->resid_longest_first = value == 4;
            return MRA_OK;
        case MRA_OPT_PARENT_PAIR:
            if (value < 0 || value > 2) throw MraError(MRA_ERR_INVALID, "option 23: 0, 1 (where a CU gets more than one front) or 2 (wherever the fronts fit)");
            pl->use_parent_pair = (int)value;
            return MRA_OK;
        case MRA_OPT_PRIOR_REUSE:
            if (value != 0 && value != 1) throw MraError(MRA_ERR_INVALID, "option 24: 0 or 1");
            pl->use_prior_reuse = value != 0;
            return MRA_OK;
        case MRA_OPT_RESID_REUSE:
            if (value != 0 && value != 1) throw MraError(MRA_ERR_INVALID, "option 25: 0 or 1");
            pl->use_resid_reuse = value != 0;
            return MRA_OK;
        case MRA_OPT_SAMPLE_GRAM_BYTES:
            if (value < 0) throw MraError(MRA_ERR_INVALID, "option 19: the Gram batch budget is a byte count >= 0");
            if ((size_t)value != pl->smp.gram_bytes) { pl->smp.gram_bytes = (size_t)value; pl->smp.built = false; }
            return MRA_OK;
        case MRA_OPT_SAMPLE_SOLVE:
            if (value != 0 && value != 1) throw MraError(MRA_ERR_INVALID, "option 20: 0 or 1");
            pl->slv.in_sampler = (int)value;
            return MRA_OK;
        case MRA_OPT_SITES_CHUNK_BYTES:
            if (value < 0) throw MraError(MRA_ERR_INVALID, "option 21: the site chunk budget is a byte count >= 0");
            pl->sit.chunk_bytes = (size_t)value;
            return MRA_OK;
        case MRA_OPT_CASCADE_GROUP:
            if (!pl->regular) return MRA_OK;          // (no fused cascade: nothing is grouped, the decision stays 0)
            pl->cascade_group_siblings = value != 0;
            pl->lik_tiles_valid = false;
            HIP_TRY(mraSetDevice(pl->device));
            build_leaf_workgroups(pl);
            return MRA_OK;
        case OPT_KERNEL_SHAPE:
            // kernel-shape switches for A/B runs.  Bits 8 and 32 keep the results (predictive cascade at two workgroups per CU, the
            // wide leaf-residual shape); bits 1, 2, 4 (no Ut scatter / no W stores / constant instead of the kernel) give WRONG results
            // and exist only in the diagnostic what-if build (`make whatif`, -DMRA_WHATIF): the product library refuses them.
#ifndef MRA_WHATIF
            if (value & ~(int64_t)(8 | 32)) throw MraError(MRA_ERR_INVALID, "option 99: bits other than 8 and 32 need the -DMRA_WHATIF diagnostic build");
#endif
            pl->dbg = (int)value;
            return MRA_OK;
        default: throw MraError(MRA_ERR_INVALID, "unknown option");
        }
    });
}

int mra_plan_get_option(mra_plan* pl, int option, int64_t* value) {
    return guarded(pl, [&] {
        require(pl && value, "mra_plan_get_option: plan or value is NULL");
        switch (option) {
            case MRA_OPT_KERNEL_TIMING: *value = pl->ktiming; break;
            case MRA_OPT_FUSED: *value = pl->use_fused; break;
            case MRA_OPT_GEMM_LDS: *value = pl->gemm_lds; break;
            case MRA_OPT_FRONT_FUSED: *value = pl->use_front_fused; break;
            case MRA_OPT_KNOT_CHAIN: *value = pl->use_knot_chain; break;
            case MRA_OPT_LEAF_GEMM: *value = pl->use_leaf_gemm ? (pl->leaf_gemm_update ? 2 : 1) : 0; break;
            case MRA_OPT_LEAF_SOLVE: *value = pl->leaf_solve_mode; break;
            case MRA_OPT_PRED_UPDATE: *value = pl->use_pred_update; break;
            case MRA_OPT_LEAF_SOLVE_SPLIT: *value = pl->leaf_solve_split; break;
            case MRA_OPT_CHOL_TILES: *value = pl->use_chol_lds; break;
            case MRA_OPT_SEG_GEMM_LDS: *value = pl->seg_gemm_lds; break;
            case MRA_OPT_SYRK_BLK: *value = pl->use_syrk_blk; break;
            case MRA_OPT_PRIOR_LEVEL: *value = pl->use_prior_level; break;
            case MRA_OPT_HI_FOLD: *value = pl->use_hi_fold; break;
            case MRA_OPT_LIK_ROWS: *value = pl->use_lik_rows; break;
            case MRA_OPT_UT_GATHER: *value = pl->ut_gather; break;
            case MRA_OPT_LEAF_ORDER: *value = pl->resid_longest_first ? 4 : pl->use_leaf_fork ? (pl->leaf_longest_first ? 1 : 2) : (pl->leaf_longest_first ? 3 : 0); break;
            case MRA_OPT_PARENT_PAIR: *value = pl->use_parent_pair; break;
            case MRA_OPT_PRIOR_REUSE: *value = pl->use_prior_reuse; break;
            case MRA_OPT_RESID_REUSE: *value = pl->use_resid_reuse; break;
            case MRA_OPT_CASCADE_GROUP: *value = pl->cascade_group_siblings; break;
            case MRA_OPT_SAMPLE_GRAM_BYTES: *value = (int64_t)pl->smp.gram_bytes; break;
            case MRA_OPT_SAMPLE_SOLVE: *value = pl->slv.in_sampler; break;
            case MRA_OPT_SITES_CHUNK_BYTES: *value = (int64_t)pl->sit.chunk_bytes; break;
            case OPT_KERNEL_SHAPE: *value = pl->dbg; break;
            default: throw MraError(MRA_ERR_INVALID, "unknown option");
        }
        return MRA_OK;
    });
}

// Raise the dynamic-LDS limit of every kernel this plan can launch on ITS device now instead of at first launch (the
// attribute is per device and per kernel; plans on different devices each do it).  n_kernels: how many kernels are on record.
int mra_plan_prepare(mra_plan* pl, int64_t* n_kernels) {
    return guarded(pl, [&] {
        require(pl, "mra_plan_prepare: plan is NULL");
        HIP_TRY(mraSetDevice(pl->device));
        pl->prepare_only = true;
        struct Guard { mra_plan* p; ~Guard() { p->prepare_only = false; } } guard{pl};
        launch_trsm2(pl, nullptr, 0, 1, 0, 1);
        ensure_big_lds(pl, {(const void*)k_front<true>, (const void*)k_front<false>, (const void*)k_parent_front<2>, (const void*)k_parent_front<4>,
                            (const void*)k_parent_front<8>, (const void*)k_parent_front<12>, (const void*)k_parent_front_pair<17>,
                            (const void*)k_parent_front_pair<23>, (const void*)k_leaf_solve_update<8, 13, true>});
        if (pl->regular) {
            if (pl->kp.mode != 4 && pl->kp.mode != 5 && pl->kp.mode != 6) {          // (MRA_KERNEL_MATERN, MRA_KERNEL_SUM and MRA_KERNEL_LOCAL have no fused prior: path_of never sends them down the fused path, whose two kernels these are)
                CascadeArgs ar{};
                ar.n_wg = 1;
                launch_cascade_any(pl, ar);
                KnotChainArgs ka{};
                ka.nl = 1;
                launch_knot_chain(pl, ka);
            }
            PredArgs pa{};
            pa.n_wg = 1;
            launch_predict_any(pl, pa, 0);
            pa.leaf_upd = (const unsigned char*)1;       // never dereferenced: prepare_only returns before any launch
            launch_predict_any(pl, pa, 0);
        }
        if (n_kernels) *n_kernels = (int64_t)pl->big_lds_done.size();
        return MRA_OK;
    });
}

int mra_get_kernel_stats(mra_plan* pl, int which, char* name, int name_cap, int* launches, double* ms, double* flops) {
    if (!pl || which < 0 || which >= KF_COUNT) return MRA_ERR_INVALID;
    const PassPath path = path_of(pl);         // (the plan's current state, not the pass that ran)
    const bool hi_name = path == PassPath::Hi && (which == KF_PRED_TRSM || which == KF_PRED_UPDATE);
    if (name && name_cap > 0) { strncpy(name, hi_name ? kfam_name_hi[which - KF_PRED_TRSM] : kfam_name[path == PassPath::Fused ? 0 : 1][which], name_cap - 1); name[name_cap - 1] = 0; }
    if (launches) *launches = pl->kstat[which].launches;
    if (ms) *ms = pl->kstat[which].ms;
    if (flops) *flops = pl->kstat[which].flops;
    return MRA_OK;
}

int mra_get_kernel_work(mra_plan* pl, int which, double* out, int cap) {
    if (!pl || !out || which < 0 || which >= KF_COUNT) return MRA_ERR_INVALID;
    const double v[4] = {pl->kstat[which].flops, pl->kstat[which].flops_exec, pl->kstat[which].bytes, pl->kstat[which].ms};
    for (int k = 0; k < std::min(cap, 4); ++k) out[k] = v[k];
    return MRA_OK;
}

int mra_device_synchronize(int device) {
    return guarded(nullptr, [&] { if (!g_dry) { HIP_TRY(hipSetDevice(device)); HIP_TRY(hipDeviceSynchronize()); } return MRA_OK; });
}

int mra_kernel_family_count(void) { return KF_COUNT; }

// Diagnostics: the route of the last pass as integers, in the order include/mra_hip.h documents.  Reads, changes nothing.
int mra_get_route(mra_plan* pl, int32_t* out, int cap) {
    return guarded(pl, [&] {
        require(pl && out, "mra_get_route: plan or out is NULL");
        if (!pl->route_set) throw MraError(MRA_ERR_STATE, "mra_get_route: no pass has run on this plan yet");
        const PassRoute& r = pl->route;
        const int32_t v[MRA_ROUTE_FIELDS] = {
            (int32_t)r.path, r.predict, r.init_yblock, r.acc_var, r.n_chain, r.prior_level, r.c_only, r.lik_rows, r.lik_general, r.scatter_ut,
            r.leaf_resident, (int32_t)r.c_fix, (int32_t)r.chol, (int32_t)r.var, (int32_t)r.update, r.solve_fused, r.direct_parent,
            r.parent_front, r.front_fused, r.syrk_blk, r.syrk_dma, r.side, r.extract_mean,
            (int32_t)pl->leaf_nodes.size(), (int32_t)pl->n_trsm_small, (int32_t)pl->n_chol_small, pl->n_cu};
        const int n = std::max(0, std::min(cap, (int)MRA_ROUTE_FIELDS));
        for (int k = 0; k < n; ++k) out[k] = v[k];
        return n;
    });
}

int mra_plan_info(mra_plan* pl, int64_t* out, int cap) {
    if (!pl || !out) return 0;
    int64_t v[10] = {pl->P, pl->ldw, pl->Ka, (int64_t)pl->leaf_nodes.size(), (int64_t)pl->W.n * 8,
                     (int64_t)pl->panel.n * 8, (int64_t)pl->Gt.n * 8, pl->n_nodes, pl->trend.p, (int64_t)pl->trend.X.n * 8};
    int n = std::min(cap, 10);
    for (int k = 0; k < n; ++k) out[k] = v[k];
    return n;
}

// Diagnostics: evaluate a device kernel on n distances (pyMRA/MRATools.py:265-301 on D = dist(...)).
int mra_eval_kernel(int kind, const double* params, int n_params, const double* D, int64_t n, double* out) {
    return guarded(nullptr, [&] {
        require(params && D && out, "mra_eval_kernel: params, D or out is NULL");
        require(n > 0, "mra_eval_kernel: n <= 0");
        check_kernel_params("mra_eval_kernel", kind, params, n_params);
        if (kind == MRA_KERNEL_LOCAL) throw MraError(MRA_ERR_INVALID, "mra_eval_kernel: MRA_KERNEL_LOCAL is no function of the distance alone (mra_eval_kernel_local)");
        KernelParams kp{};
        kp.kind = kind; kp.d = 1; kp.l = params[0]; kp.sig = params[1]; kp.scale = params[2];
        kp.circular = (n_params >= 4 && params[3] != 0.0) ? 1 : 0;
        if (kind == MRA_KERNEL_MATERN) kp.nu = params[4];
        std::vector<double> rec;
        if (kind == MRA_KERNEL_SUM) rec = sum_records(kp, params);
        else derive_kernel_params(kp);
        if (g_dry) throw MraError(MRA_ERR_STATE, "MRA_HOST_DRYRUN: nothing runs in this mode");
        DevVec<double> dD, dO, dT;
        dD.alloc(n);
        dO.alloc(n);
        HIP_TRY(mraMemcpy(dD.p, D, n * sizeof(double), hipMemcpyHostToDevice));
        if (kind == MRA_KERNEL_MATERN) {     // a kernel of its own: k_eval_kernel and the runtime cov_of_dist keep their object code
            dT.upload(matern_nu_table(kp.nu));
            kp.nu_tab = dT.p; kp.nu_n = MRA_NU_NODES;
            hipLaunchKernelGGL(k_eval_kernel_nu, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dD.p, dO.p, (long)n, kp);
        } else if (kind == MRA_KERNEL_SUM) {
            dT.upload(rec);
            kp.nu_tab = dT.p;
            hipLaunchKernelGGL(k_eval_kernel_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dD.p, dO.p, (long)n, kp);
        } else hipLaunchKernelGGL(k_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dD.p, dO.p, (long)n, kp);
        HIP_TRY(hipGetLastError());
        HIP_TRY(mraMemcpy(out, dO.p, n * sizeof(double), hipMemcpyDeviceToHost));
        return MRA_OK;
    });
}

// ... and MRA_KERNEL_LOCAL on n pairs: the distance D[i] over ds = 1 or 2 spatial dimensions and the two ranges la[i], lb[i]
int mra_eval_kernel_local(const double* params, int n_params, int ds, const double* D, const double* la, const double* lb, int64_t n, double* out) {
    return guarded(nullptr, [&] {
        require(params && D && la && lb && out, "mra_eval_kernel_local: params, D, la, lb or out is NULL");
        require(n > 0, "mra_eval_kernel_local: n <= 0");
        require(ds == 1 || ds == 2, "mra_eval_kernel_local: ds must be 1 or 2");
        check_kernel_params("mra_eval_kernel_local", MRA_KERNEL_LOCAL, params, n_params);
        require_ranges("mra_eval_kernel_local", std::min(last_column_min(la, n, 1), last_column_min(lb, n, 1)));
        KernelParams kp{};
        kp.kind = MRA_KERNEL_LOCAL; kp.d = ds + 1; kp.l = params[0]; kp.sig = params[1]; kp.scale = params[2];
        derive_local_params(kp, params);
        if (g_dry) throw MraError(MRA_ERR_STATE, "MRA_HOST_DRYRUN: nothing runs in this mode");
        DevVec<double> dD, dA, dB, dO;
        dD.alloc(n); dA.alloc(n); dB.alloc(n); dO.alloc(n);
        HIP_TRY(mraMemcpy(dD.p, D, n * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(mraMemcpy(dA.p, la, n * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(mraMemcpy(dB.p, lb, n * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_eval_kernel_local, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dD.p, dA.p, dB.p, dO.p, (long)n, ds, kp);
        HIP_TRY(hipGetLastError());
        HIP_TRY(mraMemcpy(out, dO.p, n * sizeof(double), hipMemcpyDeviceToHost));
        return MRA_OK;
    });
}

int mra_tree_replay_2d(const double* locs, int64_t N, int32_t r, int32_t M, uint32_t* mt_key, int32_t* mt_pos, mra_tree** out) {
    return guarded(nullptr, [&] {
        require(locs && mt_key && mt_pos && out, "mra_tree_replay_2d: locs, mt_key, mt_pos or out is NULL");
        *out = nullptr;
        *out = replay_tree(locs, N, r, M, mt_key, mt_pos).release();
        return *out ? MRA_OK : 1;
    });
}

int mra_tree_replay_2d_into(const double* locs, int64_t N, int32_t r, int32_t M, uint32_t* mt_key, int32_t* mt_pos, int64_t cap_rows,
                            int64_t* perm, int64_t* src, uint8_t* in_leaf, int64_t* knot_rows, mra_tree** out) {
    return guarded(nullptr, [&] {
        require(locs && mt_key && mt_pos && out && perm && src && in_leaf && knot_rows, "mra_tree_replay_2d_into: NULL array or out");
        *out = nullptr;
        require(M >= 0 && M <= 15 && cap_rows >= N + 15 * ((int64_t)1 << (2 * M)), "mra_tree_replay_2d_into: cap_rows must be at least N + 15 * 4^M");
        *out = replay_tree(locs, N, r, M, mt_key, mt_pos, perm, src, in_leaf, knot_rows).release();
        return *out ? MRA_OK : 1;
    });
}

int mra_plan_create_replay_2d(const double* locs, int64_t N, int32_t r, int32_t M, uint32_t* mt_key, int32_t* mt_pos,
                              const double* y, double R, int device, int64_t cap_rows,
                              int64_t* perm, int64_t* src, uint8_t* in_leaf, int64_t* knot_rows, mra_tree** tree_out, mra_plan** plan_out) {
    return guarded(nullptr, [&] {
        require(locs && mt_key && mt_pos && y && tree_out && plan_out && perm && src && in_leaf && knot_rows,
                "mra_plan_create_replay_2d: NULL array or out");
        *tree_out = nullptr; *plan_out = nullptr;
        require(M >= 0 && M <= 15 && cap_rows >= N + 15 * ((int64_t)1 << (2 * M)), "mra_plan_create_replay_2d: cap_rows must be at least N + 15 * 4^M");
        require(R > 0.0, "R must be a positive scalar");
        ReplayPlanCtx ctx{locs, y, R, device};
        std::unique_ptr<mra_tree> t = replay_tree(locs, N, r, M, mt_key, mt_pos, perm, src, in_leaf, knot_rows, replay_plan_hook, &ctx);
        if (!t) return 1;                                    // not a large-2-D tree: nothing is handed out
        if (ctx.rc != MRA_OK) throw MraError(ctx.rc, ctx.err);
        mra_plan* pl = ctx.pl.get();
        PlanTrace tr("knots into the plan");
        HIP_TRY(mraSetDevice(pl->device));
        pl->knot_ptr.assign(t->r.knot_ptr.begin(), t->r.knot_ptr.end());
        pl->knot_rows.assign(knot_rows, knot_rows + t->r.n_knot_rows);
        pl->knots_pending = false;
        fill_knot_arrays(pl);
        set_knot_coords_src(pl, locs, src);                  // knot coordinates straight from the caller's rows
        *tree_out = t.release();
        *plan_out = ctx.pl.release();
        return MRA_OK;
    });
}

int mra_tree_sizes(mra_tree* t, int64_t* out5) {
    if (!t || !out5) return MRA_ERR_INVALID;
    out5[0] = t->r.P; out5[1] = t->r.n_nodes; out5[2] = t->r.n_levels;
    out5[3] = (int64_t)t->r.child_list.size(); out5[4] = t->r.n_knot_rows;
    return MRA_OK;
}

int mra_tree_export(mra_tree* t, int64_t* perm, int64_t* src, uint8_t* in_leaf, int64_t* level_ptr, int32_t* node_level,
                    int64_t* row0, int64_t* row1, uint8_t* leaf, int32_t* parent, int32_t* child_ptr, int32_t* child_list,
                    int64_t* knot_ptr, int64_t* knot_rows, int32_t* cw, int32_t* preorder) {
    return guarded(nullptr, [&] {
        require(t, "mra_tree_export: tree is NULL");
        const mra_topo::Result& r = t->r;
        auto cp = [](auto* dst, const auto& v) { if (dst && !v.empty()) memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
        cp(perm, r.perm); cp(src, r.src); cp(in_leaf, r.in_leaf); cp(level_ptr, r.level_ptr); cp(node_level, r.level);
        cp(row0, r.row0); cp(row1, r.row1); cp(leaf, r.leaf); cp(parent, r.parent); cp(child_ptr, r.child_ptr);
        cp(child_list, r.child_list); cp(knot_ptr, r.knot_ptr); cp(knot_rows, r.knot_rows); cp(cw, r.cw); cp(preorder, r.preorder);
        return MRA_OK;
    });
}

int mra_tree_free(mra_tree* t) { return guarded(nullptr, [&] { delete t; return MRA_OK; }); }

// ---- multi-GPU ------------------------------------------------------------------------------------
int mra_plan_set_reduce_level(mra_plan* pl, int level) {
    return guarded(pl, [&] {
        require(pl, "mra_plan_set_reduce_level: plan is NULL");
        pl->slv.valid = false;
        prior_keep_reset(pl);
        if (level >= pl->n_levels) throw MraError(MRA_ERR_INVALID, "reduce level out of range");
        if (pl->lowrank_parent && level >= pl->n_levels - 3)
            throw MraError(MRA_ERR_INVALID, "reduce level too deep: the fronts of the leaves' parents are kept as panels on this plan (set MRA_NO_LOWRANK_PARENT=1 before creating it)");
        pl->reduce_level = level;
        return MRA_OK;
    });
}

int mra_reduce_size(mra_plan* pl, int64_t* n) {
    return guarded(pl, [&] {
        require(pl && n, "mra_reduce_size: plan or n is NULL");
        if (pl->reduce_level < 0) throw MraError(MRA_ERR_STATE, "no reduce level set");
        *n = (int64_t)pl->lev[pl->reduce_level].F.n;
        return MRA_OK;
    });
}

int mra_reduce_export(mra_plan* pl, double* out) {
    return guarded(pl, [&] {
        require(pl && out, "mra_reduce_export: plan or out is NULL");
        if (!pl->split_pending) throw MraError(MRA_ERR_STATE, "no split run pending");
        HIP_TRY(mraSetDevice(pl->device));
        HIP_TRY(hipStreamSynchronize(pl->stream));
        LevelData& lv = pl->lev[pl->reduce_level];
        HIP_TRY(mraMemcpy(out, lv.F.p, lv.F.n * sizeof(double), hipMemcpyDeviceToHost));
        return MRA_OK;
    });
}

int mra_reduce_import(mra_plan* pl, const double* in) {
    return guarded(pl, [&] {
        require(pl && in, "mra_reduce_import: plan or in is NULL");
        if (!pl->split_pending) throw MraError(MRA_ERR_STATE, "no split run pending");
        HIP_TRY(mraSetDevice(pl->device));
        LevelData& lv = pl->lev[pl->reduce_level];
        HIP_TRY(mraMemcpy(lv.F.p, in, lv.F.n * sizeof(double), hipMemcpyHostToDevice));
        return MRA_OK;
    });
}

int mra_comm_unique_id(char* out, int cap) {
    return guarded(nullptr, [&] {
        require(out && cap >= 128, "mra_comm_unique_id: out is NULL or cap < 128");
        void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) throw MraError(MRA_ERR_COMM, "cannot load librccl.so");
        typedef ncclResult_t (*uid_t_)(ncclUniqueId*);
        uid_t_ fn = (uid_t_)dlsym(h, "ncclGetUniqueId");
        if (!fn || fn((ncclUniqueId*)out) != ncclSuccess) throw MraError(MRA_ERR_COMM, "ncclGetUniqueId failed");
        return MRA_OK;
    });
}

int mra_comm_init(mra_plan* pl, const char* uid, int n_ranks, int rank) {
    return guarded(pl, [&] {
        require(pl && uid, "mra_comm_init: plan or uid is NULL");
        HIP_TRY(mraSetDevice(pl->device));
        pl->rccl = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!pl->rccl) pl->rccl = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!pl->rccl) throw MraError(MRA_ERR_COMM, "cannot load librccl.so");
        ncclUniqueId id;
        static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
        memcpy(&id, uid, sizeof id);
        typedef ncclResult_t (*init_t)(ncclComm_t*, int, ncclUniqueId, int);
        init_t fn = (init_t)dlsym(pl->rccl, "ncclCommInitRank");
        if (!fn) throw MraError(MRA_ERR_COMM, "ncclCommInitRank not found");
        pl->allreduce = (decltype(pl->allreduce))dlsym(pl->rccl, "ncclAllReduce");
        if (!pl->allreduce) throw MraError(MRA_ERR_COMM, "ncclAllReduce not found");
        if (fn(&pl->comm, n_ranks, id, rank) != ncclSuccess) { pl->comm = nullptr; throw MraError(MRA_ERR_COMM, "ncclCommInitRank failed"); }
        pl->n_ranks = n_ranks; pl->rank = rank;
        return MRA_OK;
    });
}

}  // extern "C"
