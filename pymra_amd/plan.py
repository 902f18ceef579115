"""ctypes binding of libmra_hip.so (include/mra_hip.h) - the only way the Python host reaches the GPU.

There is deliberately no CPU fallback: if the shared library is missing, or no AMD GPU is
visible when a plan is created, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os

import collections

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PYMRA_AMD_LIB: another build of the same library (tests/test_asan_host.py points it at the host-sanitizer build)
LIB_PATH = os.environ.get("PYMRA_AMD_LIB") or os.path.join(_HERE, "libmra_hip.so")

MRA_RUN_LIKELIHOOD = 1
MRA_RUN_PREDICT = 2
MRA_RUN_SPLIT = 4
MRA_KERNEL_SUM = 7           # a sum of up to four closed-form kernels (MRATools.KernelSum)
MRA_KERNEL_LOCAL = 8         # local ranges in the last coordinate column (MRATools.LocalRange)
MRA_KERNEL_HOST = 100
MRA_OPT_KERNEL_TIMING = 1
MRA_OPT_FUSED = 2
MRA_OPT_GEMM_LDS = 3
MRA_OPT_FRONT_FUSED = 4
MRA_OPT_KNOT_CHAIN = 5
MRA_OPT_LEAF_GEMM = 6
MRA_OPT_LEAF_SOLVE = 7
MRA_OPT_PRED_UPDATE = 8
MRA_OPT_LEAF_SOLVE_SPLIT = 10
MRA_OPT_CHOL_TILES = 11
MRA_OPT_SEG_GEMM_LDS = 12
MRA_OPT_UT_GATHER = 13
MRA_OPT_SYRK_BLK = 14
MRA_OPT_PRIOR_LEVEL = 15
MRA_OPT_HI_FOLD = 16
MRA_OPT_LIK_ROWS = 17
MRA_OPT_CASCADE_GROUP = 18
MRA_OPT_SAMPLE_GRAM_BYTES = 19
MRA_OPT_SAMPLE_SOLVE = 20
MRA_OPT_SITES_CHUNK_BYTES = 21
MRA_CV_LEAF = 1
MRA_CV_TREND_REFIT = 2
MRA_OPT_LEAF_ORDER = 22
MRA_OPT_PARENT_PAIR = 23
MRA_OPT_PRIOR_REUSE = 24
MRA_OPT_RESID_REUSE = 25
MRA_FAMILY_GAUSSIAN, MRA_FAMILY_POISSON, MRA_FAMILY_BINOMIAL = 0, 1, 2
LAPLACE_FAMILIES = {"gaussian": MRA_FAMILY_GAUSSIAN, "poisson": MRA_FAMILY_POISSON, "binomial": MRA_FAMILY_BINOMIAL}
# info[8..11] of mra_plan_fit_laplace_trend, behind the eight of LAPLACE_INFO
LAPLACE_TREND_INFO = ("logdetA", "profile", "reml", "n_obs")
LAPLACE_INFO = ("d", "u", "neg2logp", "sum_log_D", "sum_D_res2", "passes", "step", "converged")      # info[8] of mra_plan_fit_laplace
MRA_SAMPLE_CONDITIONAL = 1
MRA_COV_POSTERIOR = 1
MRA_SOLVE_FULL_QUAD = 1
MRA_FULL_QUAD_MAX = 256
MRA_TREND_MAX = 63
MRA_TREND_PREDICT = 1
MRA_SITES_COV_MAX = 16384
MRA_SAMPLE_SITES_LEAF_MAX = 4096
MRA_BLOCK_W_ROWS, MRA_BLOCK_LPRIOR, MRA_BLOCK_FRONT, MRA_BLOCK_LEAF = 0, 1, 2, 3

# mra_get_route (include/mra_hip.h): the fields in the order the library writes them, and the members of the four enums by value
ROUTE_FIELDS = ("path", "predict", "init_yblock", "acc_var", "n_chain", "prior_level", "c_only", "lik_rows", "lik_general", "scatter_ut",
                "leaf_resident", "c_fix", "chol", "var", "update", "solve_fused", "direct_parent", "parent_front", "front_fused",
                "syrk_blk", "syrk_dma", "side", "extract_mean", "n_leaves", "n_trsm_small", "n_chol_small", "n_cu")
ROUTE_ENUMS = {
    "path": ("Fused", "Hi", "Levels"),
    "c_fix": ("None", "InProduct", "Phantom", "Fill"),
    "chol": ("TilesOne", "TilesSplit", "Wave", "BigPanels"),
    "var": ("None", "FinishVar", "Moments"),
    "update": ("None", "InCascade", "InPredictHi", "SolveWhole", "SolveHalves", "Gemm", "LeafGemm"),
}
ROUTE_COUNTS = ("n_chain", "n_leaves", "n_trsm_small", "n_chol_small", "n_cu")

ERR_NAMES = {-1: "MRA_ERR_INVALID", -2: "MRA_ERR_HIP", -3: "MRA_ERR_NOT_SPD", -4: "MRA_ERR_STATE",
             -5: "MRA_ERR_COMM"}

# every symbol include/mra_hip.h declares (tests check that the library exports all of them)
EXPORTS = [
    "mra_device_count", "mra_release_cached_memory", "mra_plan_create", "mra_plan_destroy", "mra_plan_set_locs", "mra_plan_set_obs",
    "mra_plan_set_noise", "mra_plan_set_noise_rows", "mra_plan_fit_laplace", "mra_plan_fit_laplace_trend", "mra_plan_set_metric", "mra_plan_set_trend", "mra_trend_fit",
    "mra_plan_set_kernel", "mra_plan_set_locs_rows", "mra_plan_set_obs_rows", "mra_get_predict_rows", "mra_get_predict_rows_sd", "mra_eval_kernel", "mra_eval_kernel_local", "mra_plan_set_cov_block", "mra_run", "mra_get_likelihood", "mra_get_predict",
    "mra_sample_slots", "mra_sample", "mra_solve", "mra_cov_apply", "mra_predict_sites", "mra_sites_cov", "mra_sample_sites_slots", "mra_sample_sites", "mra_cv", "mra_cv_trend", "mra_get_buffer", "mra_get_node_block", "mra_get_timers", "mra_plan_set_option", "mra_plan_get_option", "mra_plan_prepare", "mra_kernel_family_count",
    "mra_get_kernel_stats", "mra_get_kernel_work", "mra_get_route", "mra_device_synchronize", "mra_plan_info", "mra_comm_unique_id", "mra_comm_init",
    "mra_plan_set_reduce_level", "mra_reduce_size", "mra_reduce_export", "mra_reduce_import",
    "mra_run_resume", "mra_last_error", "mra_version",
    "mra_tree_replay_2d", "mra_tree_replay_2d_into", "mra_plan_create_replay_2d", "mra_tree_sizes", "mra_tree_export", "mra_tree_free",
]


class MraTopologyStruct(C.Structure):
    _fields_ = [("P", C.c_int64), ("d", C.c_int32), ("n_levels", C.c_int32), ("n_nodes", C.c_int32),
                ("level_ptr", C.c_void_p), ("node_row0", C.c_void_p), ("node_row1", C.c_void_p),
                ("node_leaf", C.c_void_p), ("node_parent", C.c_void_p), ("child_ptr", C.c_void_p),
                ("child_list", C.c_void_p), ("knot_ptr", C.c_void_p), ("knot_rows", C.c_void_p),
                ("cw", C.c_void_p)]


# what HipPlan.trend_fit returns: beta (p), cov_beta (p x p), the profile and REML -2 log-likelihoods, d and u = G_yy - b^T beta
# (profile = d + u), the number of observed rows, and with predict=True the universal-kriging mean and variance in the caller's order
TrendFit = collections.namedtuple("TrendFit", "beta cov_beta profile reml d u n_obs mean var")


class MraError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERR_NAMES.get(code, str(code)), msg))
        self.code = code


def _check(lib, rc, handle=None):
    """Raise MraError for a nonzero return code, with mra_last_error of the plan `handle` (None: of the calling thread)."""
    if rc != 0:
        msg = lib.mra_last_error(handle)
        raise MraError(rc, msg.decode() if msg else "")


_lib = None


def load_library():
    """Load libmra_hip.so (built by __graft_entry__.build()).  Raises if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("pymra_amd: %s not found - build it with `python -c 'import __graft_entry__ as g; "
                          "g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, u32, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_double
    sig = {
        "mra_device_count": (C.c_int, []),
        "mra_release_cached_memory": (C.c_int, []),
        "mra_plan_create": (C.c_int, [C.POINTER(vp), C.POINTER(MraTopologyStruct), C.c_int]),
        "mra_plan_destroy": (C.c_int, [vp]),
        "mra_plan_set_locs": (C.c_int, [vp, vp]),
        "mra_plan_set_obs": (C.c_int, [vp, vp, dbl]),
        "mra_plan_set_noise": (C.c_int, [vp, vp]),
        "mra_plan_set_metric": (C.c_int, [vp, vp]),
        "mra_plan_set_noise_rows": (C.c_int, [vp, vp, vp]),
        "mra_plan_fit_laplace": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, C.c_int, dbl, vp]),
        "mra_plan_fit_laplace_trend": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, C.c_int, dbl, vp, vp, vp]),
        "mra_plan_set_locs_rows": (C.c_int, [vp, vp, vp]),
        "mra_plan_set_obs_rows": (C.c_int, [vp, vp, vp, vp, dbl]),
        "mra_get_predict_rows": (C.c_int, [vp, vp, vp, i64, vp, vp]),
        "mra_get_predict_rows_sd": (C.c_int, [vp, vp, vp, i64, vp, vp, vp]),
        "mra_plan_set_kernel": (C.c_int, [vp, C.c_int, vp, C.c_int]),
        "mra_plan_set_cov_block": (C.c_int, [vp, i32, vp, i64, i64, vp]),
        "mra_eval_kernel": (C.c_int, [C.c_int, vp, C.c_int, vp, i64, vp]),
        "mra_eval_kernel_local": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, i64, vp]),
        "mra_run": (C.c_int, [vp, u32]),
        "mra_run_resume": (C.c_int, [vp]),
        "mra_get_likelihood": (C.c_int, [vp, C.POINTER(dbl), C.POINTER(dbl)]),
        "mra_get_predict": (C.c_int, [vp, vp, vp]),
        "mra_sample_slots": (C.c_int, [vp, C.POINTER(i64)]),
        "mra_sample": (C.c_int, [vp, u32, i64, C.c_uint64, i64, vp, vp]),
        "mra_solve": (C.c_int, [vp, u32, i64, vp, vp, vp]),
        "mra_cov_apply": (C.c_int, [vp, u32, i64, vp, vp, vp]),
        "mra_plan_set_trend": (C.c_int, [vp, i32, vp]),
        "mra_trend_fit": (C.c_int, [vp, u32, vp, vp, vp, vp, vp]),
        "mra_predict_sites": (C.c_int, [vp, u32, i64, vp, vp, i64, vp, vp, vp]),
        "mra_sites_cov": (C.c_int, [vp, u32, i64, vp, vp, vp]),
        "mra_sample_sites_slots": (C.c_int, [vp, i64, C.POINTER(i64)]),
        "mra_sample_sites": (C.c_int, [vp, u32, i64, vp, vp, i64, C.c_uint64, i64, vp, vp]),
        "mra_cv": (C.c_int, [vp, u32, vp, vp, vp, vp, vp]),
        "mra_cv_trend": (C.c_int, [vp, u32, vp, vp, vp, vp, vp]),
        "mra_get_buffer": (C.c_int, [vp, C.c_int, vp, i64, C.POINTER(i64)]),
        "mra_get_node_block": (C.c_int, [vp, i32, C.c_int, vp, i64, C.POINTER(i64), C.POINTER(i64)]),
        "mra_get_timers": (C.c_int, [vp, vp, C.c_int]),
        "mra_plan_set_option": (C.c_int, [vp, C.c_int, i64]),
        "mra_plan_get_option": (C.c_int, [vp, C.c_int, C.POINTER(i64)]),
        "mra_plan_prepare": (C.c_int, [vp, C.POINTER(i64)]),
        "mra_kernel_family_count": (C.c_int, []),
        "mra_get_kernel_stats": (C.c_int, [vp, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(dbl), C.POINTER(dbl)]),
        "mra_get_kernel_work": (C.c_int, [vp, C.c_int, vp, C.c_int]),
        "mra_get_route": (C.c_int, [vp, vp, C.c_int]),
        "mra_device_synchronize": (C.c_int, [C.c_int]),
        "mra_plan_info": (C.c_int, [vp, vp, C.c_int]),
        "mra_comm_unique_id": (C.c_int, [C.c_char_p, C.c_int]),
        "mra_comm_init": (C.c_int, [vp, C.c_char_p, C.c_int, C.c_int]),
        "mra_plan_set_reduce_level": (C.c_int, [vp, C.c_int]),
        "mra_reduce_size": (C.c_int, [vp, C.POINTER(i64)]),
        "mra_reduce_export": (C.c_int, [vp, vp]),
        "mra_reduce_import": (C.c_int, [vp, vp]),
        "mra_tree_replay_2d": (C.c_int, [vp, i64, i32, i32, vp, C.POINTER(i32), C.POINTER(vp)]),
        "mra_tree_replay_2d_into": (C.c_int, [vp, i64, i32, i32, vp, C.POINTER(i32), i64, vp, vp, vp, vp, C.POINTER(vp)]),
        "mra_plan_create_replay_2d": (C.c_int, [vp, i64, i32, i32, vp, C.POINTER(i32), vp, dbl, C.c_int, i64, vp, vp, vp, vp,
                                                C.POINTER(vp), C.POINTER(vp)]),
        "mra_tree_sizes": (C.c_int, [vp, vp]),
        "mra_tree_export": (C.c_int, [vp] + [vp] * 15),
        "mra_tree_free": (C.c_int, [vp]),
        "mra_last_error": (C.c_char_p, [vp]),
        "mra_version": (C.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_cov_blocks(topo, cov, locs, obs):
    """The blocks mra_plan_set_cov_block wants from an opaque ``cov`` (callable on location arrays, or a dense N x N matrix), node by
    node as (node, C, diag): non-leaf nodes C(S_j, Q_j) (rows node_row0 .. node_row1, one column per knot), diag None; leaves
    C(S_j, O_j) with one column per observed row in ascending padded-row order (none: 0 columns) and diag = C(x,x) of every row of
    the leaf, phantom rows (at their ``src`` location) included.  Host arithmetic only: no plan, no device."""
    t = topo
    X = np.asarray(locs, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    y = np.asarray(obs, dtype=np.float64).reshape(-1)
    dense = None if callable(cov) else np.asarray(cov, dtype=np.float64)
    if dense is not None and dense.shape != (t.N, t.N):
        raise ValueError("a dense cov must be N x N")

    def block(ra, rb):
        if dense is not None:
            return dense[np.ix_(ra, rb)]
        return np.asarray(cov(X[ra], X[rb]), dtype=np.float64)

    def blocks():
        for i in range(t.n_nodes):
            rows = np.arange(t.node_row0[i], t.node_row1[i])
            ra = t.src[rows]
            if t.node_leaf[i]:
                real = t.perm[rows] >= 0
                obs_rows = rows[real & np.isfinite(np.where(real, y[ra], np.nan))]
                rb = t.src[obs_rows]
                C = block(ra, rb) if len(rb) else np.zeros((len(ra), 0))
                if dense is not None:
                    dg = np.diag(dense)[ra]
                else:
                    dg = np.diag(block(ra, ra))
                yield i, C, dg
            else:
                kq = t.knot_rows[t.knot_ptr[i]:t.knot_ptr[i + 1]]
                yield i, block(ra, t.src[kq]), None

    return blocks()


class HipPlan:
    """One MRA tree on one GPU.  Thin, stateful wrapper of the C ABI."""

    def __init__(self, topo, device: int = 0, _handle=None):
        self.lib = load_library()
        self.topo = topo
        self._h = C.c_void_p()
        if _handle is not None:                  # a plan the library has already built (create_with_replay)
            self._h = _handle
            self.P = int(topo.P)
            self.d = int(topo.d)
            return
        # keep the arrays alive (and of the exact dtypes the header declares) during the call
        arrs = dict(
            level_ptr=np.ascontiguousarray(topo.level_ptr, dtype=np.int64),
            node_row0=np.ascontiguousarray(topo.node_row0, dtype=np.int64),
            node_row1=np.ascontiguousarray(topo.node_row1, dtype=np.int64),
            node_leaf=np.ascontiguousarray(topo.node_leaf, dtype=np.uint8),
            node_parent=np.ascontiguousarray(topo.node_parent, dtype=np.int32),
            child_ptr=np.ascontiguousarray(topo.child_ptr, dtype=np.int32),
            child_list=np.ascontiguousarray(topo.child_list, dtype=np.int32),
            knot_ptr=np.ascontiguousarray(topo.knot_ptr, dtype=np.int64),
            knot_rows=np.ascontiguousarray(topo.knot_rows, dtype=np.int64),
            cw=np.ascontiguousarray(topo.cw, dtype=np.int32),
        )
        # the struct's d is the dimension of the coordinates the covariance is evaluated on (set_locs, sites): the topology's
        # coord_dim where it differs from the dimension the tree was partitioned on (lon/lat tree, xyz covariance)
        cd = int(getattr(topo, "coord_dim", 0) or topo.d)
        st = MraTopologyStruct(P=int(topo.P), d=cd, n_levels=int(topo.n_levels), n_nodes=int(topo.n_nodes),
                               **{k: _ptr(v) for k, v in arrs.items()})
        _check(self.lib, self.lib.mra_plan_create(C.byref(self._h), C.byref(st), int(device)))
        self.P = int(topo.P)
        self.d = cd

    # -- helpers -------------------------------------------------------------------------------
    def _check(self, rc):
        _check(self.lib, rc, self._h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.mra_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- inputs --------------------------------------------------------------------------------
    def _row_maps(self):
        if getattr(self, "_maps", None) is None:
            t = self.topo
            self._maps = (np.ascontiguousarray(t.src, dtype=np.int64), np.ascontiguousarray(t.perm, dtype=np.int64),
                          np.ascontiguousarray(t.in_leaf, dtype=np.uint8))
        return self._maps

    def set_locs(self, locs):
        """locs: the caller's N x d array; permuted/padded inside the library."""
        X = np.ascontiguousarray(locs, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        if X.shape != (self.topo.N, self.d):
            raise ValueError("locs must be N x d")
        src, _, _ = self._row_maps()
        self._check(self.lib.mra_plan_set_locs_rows(self._h, _ptr(X), _ptr(src)))

    def set_metric(self, A):
        """Distances become |A (a - b)| (mra_plan_set_metric): A d x d in the coordinates of ``set_locs``, None = no metric.  The
        plan keeps the caller's coordinates and hands every kernel A x (``buffer(13)``); ``set_locs``, ``set_obs`` and the sites of
        ``predict_sites`` and its siblings stay in the caller's coordinates.  Like ``set_kernel`` it drops the retained factors."""
        if A is None:
            self._check(self.lib.mra_plan_set_metric(self._h, None))
            return
        A = np.ascontiguousarray(A, dtype=np.float64)
        if A.shape != (self.d, self.d):
            raise ValueError("the metric must be a %d x %d matrix, got shape %r" % (self.d, self.d, A.shape))
        self._check(self.lib.mra_plan_set_metric(self._h, _ptr(A)))

    def _noise_rows(self, R):
        r = np.ascontiguousarray(np.asarray(R, dtype=np.float64))
        if r.ndim != 1:
            raise ValueError("a noise array must be 1-D: only a diagonal R (per-observation variances) is supported")
        if len(r) != self.topo.N:
            raise ValueError("a noise vector must have N entries")
        return r

    def set_obs(self, obs, R):
        """obs: the caller's N values (NaN = missing).  R: the scalar nugget, or N per-observation noise variances in the caller's
        order (read where obs is finite) - then the scalar that ``set_noise(None)`` returns to is their mean over the observed rows."""
        y = np.ascontiguousarray(np.asarray(obs, dtype=np.float64).reshape(-1))
        if len(y) != self.topo.N:
            raise ValueError("obs must have N entries")
        src, perm, _ = self._row_maps()
        if np.ndim(R) == 0:
            self._check(self.lib.mra_plan_set_obs_rows(self._h, _ptr(y), _ptr(src), _ptr(perm), float(R)))
            return
        r = self._noise_rows(R)
        in_leaf = np.zeros(len(y), dtype=bool)
        in_leaf[perm[(perm >= 0) & (self._row_maps()[2] != 0)]] = True
        ro = r[np.isfinite(y) & in_leaf]                                # the rows the plan observes
        if not (np.all(np.isfinite(ro)) and np.all(ro >= 0.0)):          # before the plan changes
            raise ValueError("the noise variance of an observed row is negative or not finite")
        scalar = float(ro.mean()) if ro.size and ro.mean() > 0.0 else 1.0
        self._check(self.lib.mra_plan_set_obs_rows(self._h, _ptr(y), _ptr(src), _ptr(perm), scalar))
        self._check(self.lib.mra_plan_set_noise_rows(self._h, _ptr(r), _ptr(src)))

    def set_noise(self, R):
        """Per-observation noise variances (mra_plan_set_noise): N values in the caller's order, read at the observed rows of the
        last ``set_obs``; None returns to that call's scalar.  y, the mask and the options stay."""
        if R is None:
            self._check(self.lib.mra_plan_set_noise(self._h, None))
            return
        r = self._noise_rows(R)
        src, _, _ = self._row_maps()
        self._check(self.lib.mra_plan_set_noise_rows(self._h, _ptr(r), _ptr(src)))

    def _padded(self, a, name):
        """The caller's N values in padded leaf order (NaN at the padding rows), or None."""
        if a is None:
            return None
        v = np.asarray(a, dtype=np.float64).reshape(-1)
        if len(v) != self.topo.N:
            raise ValueError("%s must have N entries" % name)
        src, perm, _ = self._row_maps()
        return np.ascontiguousarray(np.where(perm >= 0, v[src], np.nan))

    def fit_laplace(self, family, z, aux=None, offset=None, x0=None, max_iter=50, tol=1e-10):
        """Non-Gaussian data by a Laplace approximation (include/mra_hip.h, mra_plan_fit_laplace): Newton / IRLS on the device for the
        mode of x given z ~ ``family`` ("gaussian": N(eta, aux); "poisson": Poisson(e^eta); "binomial": Bin(aux, logistic eta)),
        eta = x + offset.  z, aux, offset, x0: the caller's N values; z finite exactly where the last ``set_obs`` observes (the mask
        is the plan's).  A scalar aux or offset holds at every row.  -> dict with d, u, neg2logp, sum_log_D, sum_D_res2, passes,
        step, converged and lik = -2 log q(z) = d + u + neg2logp + sum_log_D - sum_D_res2.  Afterwards the plan holds y = t and
        noise = 1 / D of the last pass: likelihood(), predict() and the calls on the retained factors serve the Laplace posterior."""
        fam = LAPLACE_FAMILIES.get(family, family) if isinstance(family, str) else family
        if isinstance(fam, str):
            raise ValueError("family must be one of %s" % sorted(LAPLACE_FAMILIES))
        full = lambda a: None if a is None else (np.full(self.topo.N, float(a)) if np.ndim(a) == 0 else a)
        zp, ap, op, xp = (self._padded(z, "z"), self._padded(full(aux), "aux"), self._padded(full(offset), "offset"), self._padded(x0, "x0"))
        info = np.zeros(8)
        opt = lambda a: None if a is None else _ptr(a)
        self._check(self.lib.mra_plan_fit_laplace(self._h, int(fam), opt(zp), opt(ap), opt(op), opt(xp), int(max_iter), float(tol), _ptr(info)))
        res = dict(zip(LAPLACE_INFO, info.tolist()))
        res["passes"], res["converged"] = int(res["passes"]), bool(res["converged"])
        res["info"] = info
        res["lik"] = info[0] + info[1] + info[2] + info[3] - info[4]
        return res

    def fit_laplace_trend(self, family, z, aux=None, offset=None, e0=None, max_iter=50, tol=1e-10):
        """Non-Gaussian data with a regression trend (include/mra_hip.h, mra_plan_fit_laplace_trend): eta = X beta + x + offset with
        the X of ``set_trend`` and a flat prior on beta; Newton / IRLS on the device for e = X beta + x, one likelihood pass and one
        GLS step per iteration.  z, aux, offset as in ``fit_laplace``; e0: the caller's N values of the start of e (None: the
        data-based start).  -> dict with ``fit_laplace``'s keys (``u`` is G_tt - b^T beta^, ``lik`` the profile value) plus beta,
        cov_beta, logdetA, profile, reml (beta integrated out) and n_obs.  Afterwards the plan holds y = t and noise = 1 / D of the
        last pass with the factors valid: ``trend_fit(predict=True)`` gives the mean and variance of e, the calls on the retained
        factors serve the Laplace posterior; likelihood() / predict() are unchanged."""
        fam = LAPLACE_FAMILIES.get(family, family) if isinstance(family, str) else family
        if isinstance(fam, str):
            raise ValueError("family must be one of %s" % sorted(LAPLACE_FAMILIES))
        full = lambda a: None if a is None else (np.full(self.topo.N, float(a)) if np.ndim(a) == 0 else a)
        zp, ap, op, ep = (self._padded(z, "z"), self._padded(full(aux), "aux"), self._padded(full(offset), "offset"), self._padded(e0, "e0"))
        p = int(getattr(self, "_trend_p", 0))
        beta, cov = np.zeros(max(p, 1)), np.zeros((max(p, 1), max(p, 1)))
        info = np.zeros(12)
        opt = lambda a: None if a is None else _ptr(a)
        self._check(self.lib.mra_plan_fit_laplace_trend(self._h, int(fam), opt(zp), opt(ap), opt(op), opt(ep), int(max_iter), float(tol),
                                                        _ptr(beta), _ptr(cov), _ptr(info)))
        res = dict(zip(LAPLACE_INFO + LAPLACE_TREND_INFO, info.tolist()))
        res["passes"], res["converged"], res["n_obs"] = int(res["passes"]), bool(res["converged"]), int(res["n_obs"])
        res["info"] = info
        res["lik"] = res["profile"]
        res["beta"], res["cov_beta"] = beta[:p].copy(), cov[:p, :p].copy()
        return res

    def set_kernel(self, kind, l=None, sig=1.0, scale=1.0, circular=False, nu=None, components=None):
        """nu: the smoothness of kind 6 (MRA_KERNEL_MATERN), sent behind circular; every other kind ignores it.
        Kind 7 (MRA_KERNEL_SUM): components = [(kind_c, l_c, sig_c), ...], 1 to 4 of them, value = scale * sum of sig_c k_c(D; l_c);
        they may also stand in l's place (a KernelSum's ``l`` is that list), and sig is not sent.
        Kind 8 (MRA_KERNEL_LOCAL, local ranges in the last coordinate column): l = (base kind, l), as a LocalRange's ``l`` is."""
        par = _kernel_params(kind, l, sig, scale, circular, nu, components)
        self._check(self.lib.mra_plan_set_kernel(self._h, int(kind), _ptr(par), len(par)))

    def sum_table(self):
        """The component records of a kind-7 plan as the device holds them: (K, 6) rows (submode, c / l, 1 / (2 l^2), a1, a2,
        scale sig_c); (0, 6) otherwise."""
        return self.buffer(17)[:-1].reshape(-1, 6)

    def sum_sill(self):
        """C(x, x) of a kind-7 plan as its kernels are handed it (the records' last entries added in component order); None otherwise."""
        b = self.buffer(17)
        return float(b[-1]) if b.size else None

    def matern_table(self):
        """The quadrature table of a kind-6 plan as the device holds it: (n, 2) rows (cosh(k h), c h cosh(nu k h)); (0, 2) otherwise."""
        return self.buffer(16).reshape(-1, 2)

    def set_kernel_host(self):
        """Covariance values will be supplied block by block (``set_cov_block``); call after ``set_obs``."""
        self._check(self.lib.mra_plan_set_kernel(self._h, MRA_KERNEL_HOST, None, 0))

    def set_cov_block(self, node, C, diag=None):
        C = np.ascontiguousarray(C, dtype=np.float64)
        d = None if diag is None else np.ascontiguousarray(diag, dtype=np.float64)
        self._check(self.lib.mra_plan_set_cov_block(self._h, int(node), _ptr(C), C.shape[0], C.shape[1],
                                                    None if d is None else _ptr(d)))

    def upload_host_cov(self, cov, locs, obs):
        """Evaluate an opaque ``cov`` (callable on location arrays, or a dense N x N matrix) block by block
        on the host - C(S_j, Q_j) for non-leaf nodes (pyMRA/MRANode.py:384), C(S_j, O_j) and C(x,x) for
        leaves - and hand the blocks to the library."""
        blocks = host_cov_blocks(self.topo, cov, locs, obs)      # (validates its arguments before the plan changes state)
        self.set_kernel_host()
        for i, C, dg in blocks:
            self.set_cov_block(i, C, dg)

    def set_option(self, option, value):
        self._check(self.lib.mra_plan_set_option(self._h, int(option), int(value)))

    def get_option(self, option):
        v = C.c_int64()
        self._check(self.lib.mra_plan_get_option(self._h, int(option), C.byref(v)))
        return int(v.value)

    def prepare(self):
        """Raise the dynamic-LDS limits of this plan's kernels on its device now; returns how many kernels are on record."""
        n = C.c_int64()
        self._check(self.lib.mra_plan_prepare(self._h, C.byref(n)))
        return int(n.value)

    # -- run / results -----------------------------------------------------------------------------
    def run(self, likelihood=True, predict=True, split=False):
        flags = (MRA_RUN_LIKELIHOOD if likelihood else 0) | (MRA_RUN_PREDICT if predict else 0) | (MRA_RUN_SPLIT if split else 0)
        self._check(self.lib.mra_run(self._h, flags))

    def resume(self):
        self._check(self.lib.mra_run_resume(self._h))

    def likelihood(self):
        d, u = C.c_double(), C.c_double()
        self._check(self.lib.mra_get_likelihood(self._h, C.byref(d), C.byref(u)))
        return d.value, u.value

    def predict(self, with_sd=False):
        """(mean[N], var[N]) in the caller's row order - with_sd: (mean, var, sd = sqrt(var)) -; rows outside every leaf report 0
        (see topology: rows that a partition drops, pyMRA/MRANode.py:222-228, 492-495)."""
        t = self.topo
        _, perm, in_leaf = self._row_maps()
        mean = np.empty(t.N)
        var = np.empty(t.N)
        sd = np.empty(t.N) if with_sd else None
        self._check(self.lib.mra_get_predict_rows_sd(self._h, _ptr(perm), _ptr(in_leaf), int(t.N), _ptr(mean), _ptr(var),
                                                     None if sd is None else _ptr(sd)))
        return (mean, var, sd) if with_sd else (mean, var)

    def sample_slots(self):
        """Number of latent slots of one draw (include/mra_hip.h: non-leaf nodes, leaf terms by padded row, noise by padded row)."""
        n = C.c_int64()
        self._check(self.lib.mra_sample_slots(self._h, C.byref(n)))
        return int(n.value)

    def sample(self, n, seed=0, z=None, conditional=False, sample0=0):
        """(n, P) draws from the MRA prior (conditional=False) or posterior, padded leaf order, unreported rows 0.  z: None = Philox
        draws on the device, a pure function of (seed, slot, sample0 + s); else an (n, sample_slots()) array of latent draws.
        sample0 >= 0 (MraError MRA_ERR_INVALID otherwise)."""
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        out = np.empty((n, self.topo.P))
        zp = None
        if z is not None:
            z = np.ascontiguousarray(z, dtype=np.float64)
            if z.shape != (n, self.sample_slots()):
                raise ValueError("z must have shape (n, sample_slots()) = (%d, %d)" % (n, self.sample_slots()))
            zp = _ptr(z)
        flags = MRA_SAMPLE_CONDITIONAL if conditional else 0
        self._check(self.lib.mra_sample(self._h, flags, n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample0), zp, _ptr(out)))
        return out

    def set_trend(self, X):
        """The design matrix of a regression trend (mra_plan_set_trend): (N, p) in the caller's order, p <= 63, copied to the device
        once and kept across every set_*; None (or p = 0) clears it.  It drops no factor."""
        if X is None:
            self._check(self.lib.mra_plan_set_trend(self._h, 0, None))
            self._trend_p = 0
            return
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        if X.ndim != 2 or X.shape[0] != self.topo.N:
            raise ValueError("X must have shape (N, p) = (%d, p)" % self.topo.N)
        src, perm, _ = self._row_maps()
        Xp = np.ascontiguousarray(np.where((perm >= 0)[None, :], X[src, :].T, 0.0))
        self._check(self.lib.mra_plan_set_trend(self._h, int(Xp.shape[0]), _ptr(Xp) if Xp.shape[0] else None))
        self._trend_p = int(Xp.shape[0])

    def trend_fit(self, predict=False):
        """Generalised least squares for the trend of ``set_trend`` on the plan's own y (mra_trend_fit) -> TrendFit.  predict=True:
        also the universal-kriging mean and variance in the caller's row order (rows outside every leaf report 0).  The factors are
        shared with solve(); y, the options and likelihood() / predict() are unchanged afterwards."""
        p = int(getattr(self, "_trend_p", 0))
        beta, cov = np.zeros(max(p, 1)), np.zeros((max(p, 1), max(p, 1)))
        info = np.zeros(8)
        mp = np.empty(self.topo.P) if predict else None
        vp = np.empty(self.topo.P) if predict else None
        self._check(self.lib.mra_trend_fit(self._h, MRA_TREND_PREDICT if predict else 0, _ptr(beta), _ptr(cov),
                                           None if mp is None else _ptr(mp), None if vp is None else _ptr(vp), _ptr(info)))
        mean = var = None
        if predict:
            t = self.topo
            _, perm, in_leaf = self._row_maps()
            good = (perm >= 0) & (in_leaf != 0)
            mean, var = np.zeros(t.N), np.zeros(t.N)
            mean[perm[good]] = mp[good]
            var[perm[good]] = vp[good]
        return TrendFit(beta[:p].copy(), cov[:p, :p].copy(), float(info[3]), float(info[4]), float(info[0]), float(info[1]), int(info[5]),
                        mean, var)

    def solve(self, Y, want_mean=True, want_quad=True, full_quad=False):
        """Factor once, solve many (include/mra_hip.h, mra_solve).  Y: (c, P) observation vectors in padded leaf order, read at the
        plan's observed rows only.  -> (mean (c, P) or None, quad (c, c) or None): mean[k] is the predictive mean for y = Y[k]
        (unreported rows 0), quad = Y_o^T (Sigma_MRA[o, o] + R I)^-1 Y_o, BLOCK-DIAGONAL in blocks of 16 columns (NaN elsewhere) -
        with full_quad=True (MRA_SOLVE_FULL_QUAD, c <= 256) the dense symmetric matrix.
        The factorisation is kept between calls; y, the options and likelihood() / predict() are unchanged afterwards."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim != 2 or Y.shape[1] != self.topo.P:
            raise ValueError("Y must have shape (c, P) = (c, %d)" % self.topo.P)
        c = Y.shape[0]
        mean = np.empty((c, self.topo.P)) if want_mean else None
        quad = np.empty((c, c)) if want_quad else None
        self._check(self.lib.mra_solve(self._h, MRA_SOLVE_FULL_QUAD if full_quad else 0, c, _ptr(Y), None if mean is None else _ptr(mean), None if quad is None else _ptr(quad)))
        return mean, quad

    def cov_apply(self, A, posterior=False, want_out=True, want_gram=True):
        """The MRA covariance applied to vectors (include/mra_hip.h, mra_cov_apply).  A: (c, P) in padded leaf order, read at the
        reported rows only.  -> (out (c, P) or None, gram (c, c) or None): out[k] = Sigma A[k] (posterior=True: Sigma_post A[k];
        unreported rows 0), gram = A Sigma A^T, BLOCK-DIAGONAL in blocks of 16 columns (NaN elsewhere).  The factorisation is shared
        with solve() and kept between calls; y, the options and likelihood() / predict() are unchanged afterwards."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        if A.ndim != 2 or A.shape[1] != self.topo.P:
            raise ValueError("A must have shape (c, P) = (c, %d)" % self.topo.P)
        c = A.shape[0]
        out = np.empty((c, self.topo.P)) if want_out else None
        gram = np.empty((c, c)) if want_gram else None
        flags = MRA_COV_POSTERIOR if posterior else 0
        self._check(self.lib.mra_cov_apply(self._h, flags, c, _ptr(A), None if out is None else _ptr(out), None if gram is None else _ptr(gram)))
        return out, gram

    def predict_sites(self, sites, leaf, Y=None, want_var=True):
        """Posterior mean and variance of the MRA process at locations that need not be rows of the tree (include/mra_hip.h,
        mra_predict_sites).  sites: (n, d) (or (n,) in 1-D); leaf: (n,) NODE indices of the leaf each site is assigned to; Y: (c, P)
        observation vectors in padded leaf order, read at the plan's observed rows only, or None: the plan's own observations (c = 1).
        -> (mean (c, n), var (n,) or None): var is the variance of the latent field (add R for a new observation).  The factorisation
        is shared with solve() / cov_apply() and kept between calls; y, the options and likelihood() / predict() are unchanged."""
        X = np.ascontiguousarray(sites, dtype=np.float64)
        if X.ndim == 1 and self.d == 1:
            X = X.reshape(-1, 1)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError("sites must have shape (n, d) = (n, %d)" % self.d)
        n = X.shape[0]
        lf = np.ascontiguousarray(leaf, dtype=np.int32)
        if lf.shape != (n,):
            raise ValueError("leaf must have shape (n,) = (%d,)" % n)
        c, Yp = 1, None
        if Y is not None:
            Y = np.ascontiguousarray(Y, dtype=np.float64)
            if Y.ndim != 2 or Y.shape[1] != self.topo.P:
                raise ValueError("Y must have shape (c, P) = (c, %d)" % self.topo.P)
            c, Yp = Y.shape[0], _ptr(Y)
        mean = np.empty((c, n))
        var = np.empty(n) if want_var else None
        self._check(self.lib.mra_predict_sites(self._h, 0, n, _ptr(X), _ptr(lf), c, Yp, _ptr(mean), None if var is None else _ptr(var)))
        return mean, var

    def sites_cov(self, sites, leaf, posterior=False):
        """The joint covariance of the latent MRA process at locations that need not be rows of the tree (include/mra_hip.h,
        mra_sites_cov).  sites: (n, d) (or (n,) in 1-D); leaf: (n,) NODE indices of the leaf each site is assigned to.  -> (n, n): the
        prior covariance, or with posterior=True the posterior one on the plan's observation mask; symmetric to the bit, no entry
        clamped, its posterior diagonal predict_sites' var up to rounding.  The factorisation is shared with solve() / cov_apply() /
        predict_sites() and kept between calls; y, the options and likelihood() / predict() are unchanged."""
        X = np.ascontiguousarray(sites, dtype=np.float64)
        if X.ndim == 1 and self.d == 1:
            X = X.reshape(-1, 1)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError("sites must have shape (n, d) = (n, %d)" % self.d)
        n = X.shape[0]
        lf = np.ascontiguousarray(leaf, dtype=np.int32)
        if lf.shape != (n,):
            raise ValueError("leaf must have shape (n,) = (%d,)" % n)
        out = np.empty((n, n)) if n <= MRA_SITES_COV_MAX else None       # above the cap the library refuses before it reads `out`
        self._check(self.lib.mra_sites_cov(self._h, MRA_COV_POSTERIOR if posterior else 0, n, _ptr(X), _ptr(lf), None if out is None else _ptr(out)))
        return out

    def sample_sites_slots(self, n_sites):
        """Number of latent slots of one draw at n_sites sites (include/mra_hip.h: the non-leaf nodes as sample() numbers them, then
        one leaf slot per site in the caller's order)."""
        n = C.c_int64()
        self._check(self.lib.mra_sample_sites_slots(self._h, int(n_sites), C.byref(n)))
        return int(n.value)

    def sample_sites(self, sites, leaf, n, seed=0, z=None, posterior=False, sample0=0):
        """(n, n_sites) draws of the latent MRA process at locations that need not be rows of the tree (include/mra_hip.h,
        mra_sample_sites): from the prior, or with posterior=True from the posterior on the plan's observation mask, the mean for the
        plan's own observations included.  sites: (n_sites, d) (or (n_sites,) in 1-D); leaf: (n_sites,) NODE indices of the leaf each
        site is assigned to.  z: None = Philox draws on the device, a pure function of (seed, slot, sample0 + s); else an
        (n, sample_sites_slots(n_sites)) array of latent draws.  The factorisation is shared with solve() / cov_apply() /
        predict_sites() / sites_cov() and kept between calls; y, the options and likelihood() / predict() are unchanged."""
        X = np.ascontiguousarray(sites, dtype=np.float64)
        if X.ndim == 1 and self.d == 1:
            X = X.reshape(-1, 1)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError("sites must have shape (n, d) = (n, %d)" % self.d)
        ns = X.shape[0]
        lf = np.ascontiguousarray(leaf, dtype=np.int32)
        if lf.shape != (ns,):
            raise ValueError("leaf must have shape (n,) = (%d,)" % ns)
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        zp = None
        if z is not None:
            z = np.ascontiguousarray(z, dtype=np.float64)
            if z.shape != (n, self.sample_sites_slots(ns)):
                raise ValueError("z must have shape (n, sample_sites_slots(n_sites)) = (%d, %d)" % (n, self.sample_sites_slots(ns)))
            zp = _ptr(z)
        out = np.empty((n, ns))
        self._check(self.lib.mra_sample_sites(self._h, MRA_COV_POSTERIOR if posterior else 0, ns, _ptr(X), _ptr(lf), n,
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample0), zp, _ptr(out)))
        return out

    def cv(self, leaf=False):
        """Cross-validation of the fitted model from the retained factors, without a refit (include/mra_hip.h, mra_cv): every observed
        row left out on its own, or with leaf=True the observed rows of each leaf left out together.  -> (mean, var, lpd, group_lpd,
        info): the leave-out predictive mean, the predictive variance of a new observation (noise included) and the marginal log
        predictive density by padded row, NaN where nothing is observed; the groups' log predictive densities by node (NaN for
        non-leaves and leaves without observations); info[8] as the header lists it (2: the CV log score, 5: max v / r).  The
        factorisation is shared with the other calls on the retained factors and kept between calls; y, the options and
        likelihood() / predict() are unchanged."""
        mean, var, lpd = np.empty(self.P), np.empty(self.P), np.empty(self.P)
        group = np.empty(self.info()["n_nodes"])
        info = np.zeros(8)
        self._check(self.lib.mra_cv(self._h, MRA_CV_LEAF if leaf else 0, _ptr(mean), _ptr(var), _ptr(lpd), _ptr(group), _ptr(info)))
        return mean, var, lpd, group, info

    def cv_trend(self, leaf=False, refit=True):
        """``cv`` for a plan with a regression trend (include/mra_hip.h, mra_cv_trend): the model is y = X beta + x + eps with the X
        of ``set_trend`` and a flat prior on beta.  refit=True: beta is estimated again without the left-out group (universal-kriging
        cross-validation; X without the group must keep full column rank); refit=False: the beta^ of the full fit is plugged in, which
        is ``cv`` on y - X beta^ reported on the scale of y.  -> (mean, var, lpd, group_lpd, info) as ``cv``, info[12] as the header
        lists it (5: the largest leverage the mode divides by, 6: tr K^-1, 7: |P y|^2, 8: tr P, 9: p, 10 / 11: the derivatives of the
        profile / REML -2 log-likelihood by a nugget added to every observed row).  The trend is fitted from the factors that stand;
        y, the options, likelihood() / predict() and what trend_fit() and cv() return are unchanged."""
        mean, var, lpd = np.empty(self.P), np.empty(self.P), np.empty(self.P)
        group = np.empty(self.info()["n_nodes"])
        info = np.zeros(12)
        flags = (MRA_CV_LEAF if leaf else 0) | (MRA_CV_TREND_REFIT if refit else 0)
        self._check(self.lib.mra_cv_trend(self._h, flags, _ptr(mean), _ptr(var), _ptr(lpd), _ptr(group), _ptr(info)))
        return mean, var, lpd, group, info

    def buffer(self, what):
        n = C.c_int64()
        self._check(self.lib.mra_get_buffer(self._h, what, None, 0, C.byref(n)))
        out = np.empty(n.value)
        self._check(self.lib.mra_get_buffer(self._h, what, _ptr(out), n.value, C.byref(n)))
        return out

    def node_block(self, node, what):
        """Raw per-node device block (include/mra_hip.h: MRA_BLOCK_*), as a 2-D array."""
        nr, nc = C.c_int64(), C.c_int64()
        self._check(self.lib.mra_get_node_block(self._h, int(node), int(what), None, 0, C.byref(nr), C.byref(nc)))
        out = np.empty((nr.value, nc.value))
        if out.size:
            self._check(self.lib.mra_get_node_block(self._h, int(node), int(what), _ptr(out), out.size, C.byref(nr), C.byref(nc)))
        return out

    def timers(self):
        out = np.zeros(5)
        k = self.lib.mra_get_timers(self._h, _ptr(out), 5)
        names = ["prior_ms", "leaf_ms", "fronts_ms", "predict_ms", "total_ms"]
        return dict(zip(names[:k], out[:k]))

    def kernel_stats(self):
        res = []
        for k in range(self.lib.mra_kernel_family_count()):
            name = C.create_string_buffer(128)
            n, ms, fl = C.c_int(), C.c_double(), C.c_double()
            self._check(self.lib.mra_get_kernel_stats(self._h, k, name, 128, C.byref(n), C.byref(ms), C.byref(fl)))
            w = np.zeros(4)
            self._check(self.lib.mra_get_kernel_work(self._h, k, _ptr(w), 4))
            res.append(dict(name=name.value.decode(), launches=n.value, ms=ms.value, flops=fl.value, flops_exec=float(w[1]), bytes=float(w[2])))
        return res

    def route(self):
        """Which kernels the last pass launched (mra_get_route): the fields of the library's PassRoute by name - the four enums as
        their member names (ROUTE_ENUMS), the counts as ints, everything else as bools.  MraError MRA_ERR_STATE before the first pass."""
        out = np.zeros(len(ROUTE_FIELDS), dtype=np.int32)
        n = self.lib.mra_get_route(self._h, _ptr(out), len(out))
        if n < 0:
            self._check(n)
        if n != len(ROUTE_FIELDS):
            raise RuntimeError("mra_get_route wrote %d fields, this binding knows %d" % (n, len(ROUTE_FIELDS)))
        res = {}
        for k, v in zip(ROUTE_FIELDS, (int(x) for x in out)):
            res[k] = ROUTE_ENUMS[k][v] if k in ROUTE_ENUMS else v if k in ROUTE_COUNTS else bool(v)
        return res

    def info(self):
        out = np.zeros(10, dtype=np.int64)
        self.lib.mra_plan_info(self._h, _ptr(out), len(out))
        keys = ["P", "ldw", "Ka", "n_leaves", "bytes_W", "bytes_panels", "bytes_Gt", "n_nodes", "trend_p", "bytes_trend"]
        return dict(zip(keys, (int(v) for v in out)))

    # -- multi-GPU ---------------------------------------------------------------------------------
    def set_reduce_level(self, level):
        self._check(self.lib.mra_plan_set_reduce_level(self._h, int(level)))

    def reduce_export(self):
        n = C.c_int64()
        self._check(self.lib.mra_reduce_size(self._h, C.byref(n)))
        out = np.empty(n.value)
        self._check(self.lib.mra_reduce_export(self._h, _ptr(out)))
        return out

    def reduce_import(self, buf):
        b = np.ascontiguousarray(buf, dtype=np.float64)
        self._check(self.lib.mra_reduce_import(self._h, _ptr(b)))

    def comm_init(self, uid: bytes, n_ranks: int, rank: int):
        self._check(self.lib.mra_comm_init(self._h, uid, int(n_ranks), int(rank)))


def create_with_replay(locs, r, M, J, obs, R, device: int = 0):
    """MRATree.__init__ for large 2-D trees in one library call (mra_plan_create_replay_2d): the tree replay and, beside its
    sequential knot draws, the plan with locations and observations already uploaded.  Consumes NumPy's global RNG exactly like
    pymra_amd.topology.build_topology.  Returns (HipPlan, Topology), or None when the tree does not follow the large-2-D rules
    (RNG state untouched: the caller takes the general path)."""
    from .topology import topology_from_tree
    coords = np.ascontiguousarray(np.asarray(locs, dtype=np.float64))
    if coords.ndim != 2 or coords.shape[1] != 2 or J != 4 or M < 1:
        return None
    y = np.ascontiguousarray(np.asarray(obs, dtype=np.float64).reshape(-1))
    N = len(coords)
    if len(y) != N:
        raise ValueError("obs must have N entries")
    state = np.random.get_state()
    if state[0] != "MT19937":
        return None
    lib = load_library()
    key = np.ascontiguousarray(state[1], dtype=np.uint32).copy()
    pos = C.c_int32(int(state[2]))
    cap = N + 15 * 4 ** int(M)
    perm, src = np.empty(cap, np.int64), np.empty(cap, np.int64)
    in_leaf, knot_rows = np.empty(cap, np.bool_), np.empty(N, np.int64)
    tree, ph = C.c_void_p(), C.c_void_p()
    rc = lib.mra_plan_create_replay_2d(_ptr(coords), N, int(r), int(M), _ptr(key), C.byref(pos), _ptr(y), float(R), int(device), cap,
                                       _ptr(perm), _ptr(src), _ptr(in_leaf), _ptr(knot_rows), C.byref(tree), C.byref(ph))
    if rc == 1:
        return None
    _check(lib, rc)
    try:
        topo = topology_from_tree(lib, tree, N, int(r), int(M), int(J), perm, src, in_leaf, knot_rows)
    except BaseException:
        lib.mra_plan_destroy(ph)
        raise
    finally:
        lib.mra_tree_free(tree)
    np.random.set_state((state[0], key, int(pos.value), state[3], state[4]))
    return HipPlan(topo, device, _handle=ph), topo


def comm_unique_id() -> bytes:
    lib = load_library()
    buf = C.create_string_buffer(128)
    _check(lib, lib.mra_comm_unique_id(buf, 128))
    return buf.raw


def _kernel_params(kind, l, sig, scale, circular, nu, components):
    """The parameter vector of mra_plan_set_kernel / mra_eval_kernel (include/mra_hip.h)."""
    if int(kind) == MRA_KERNEL_SUM:
        comps = l if components is None else components
        if comps is None or np.ndim(comps) != 2 or np.shape(comps)[1] != 3:
            raise ValueError("kind 7 takes components=[(kind, l, sig), ...]")
        return np.array([len(comps), 0.0, scale, 1.0 if circular else 0.0] + [float(v) for c in comps for v in c], dtype=np.float64)
    if components is not None:
        raise ValueError("components= belongs to kind 7")
    if int(kind) == MRA_KERNEL_LOCAL:      # {l, sig, scale, 0, base kind}: the pair (base kind, l) stands in l's place (a LocalRange's ``l``)
        if np.ndim(l) != 1 or len(l) != 2:
            raise ValueError("kind 8 takes l=(base kind, l)")
        return np.array([float(l[1]), sig, scale, 1.0 if circular else 0.0, float(l[0])], dtype=np.float64)
    return np.array([l, sig, scale, 1.0 if circular else 0.0] + ([] if nu is None else [nu]), dtype=np.float64)


def eval_kernel(kind, l=None, sig=1.0, scale=1.0, D=None, nu=None, components=None):
    """Device evaluation of a stationary kernel on an array of distances (tests); nu: the smoothness of kind 6, components: the
    (kind, l, sig) triples of kind 7."""
    lib = load_library()
    D = np.ascontiguousarray(D, dtype=np.float64).ravel()
    out = np.empty_like(D)
    par = _kernel_params(kind, l, sig, scale, False, nu, components)
    _check(lib, lib.mra_eval_kernel(int(kind), _ptr(par), len(par), _ptr(D), D.size, _ptr(out)))
    return out


def eval_kernel_local(base_kind, l, sig, scale, ds, D, la, lb):
    """Device evaluation of MRA_KERNEL_LOCAL on arrays of pairs (tests): distance D over ds spatial dimensions, local ranges la, lb."""
    lib = load_library()
    D, la, lb = (np.ascontiguousarray(v, dtype=np.float64).ravel() for v in (D, la, lb))
    if not (D.size == la.size == lb.size):
        raise ValueError("D, la and lb must have the same length")
    out = np.empty_like(D)
    par = _kernel_params(MRA_KERNEL_LOCAL, (base_kind, l), sig, scale, False, None, None)
    _check(lib, lib.mra_eval_kernel_local(_ptr(par), len(par), int(ds), _ptr(D), _ptr(la), _ptr(lb), D.size, _ptr(out)))
    return out


def device_count() -> int:
    return int(load_library().mra_device_count())


def device_synchronize(device: int = 0) -> None:
    """hipDeviceSynchronize on `device` through the library (no other GPU runtime needed for a barrier)."""
    lib = load_library()
    _check(lib, lib.mra_device_synchronize(int(device)))


def release_cached_memory() -> None:
    """Return the device blocks the library keeps from destroyed plans (reused by later plans of the same sizes) to the driver."""
    load_library().mra_release_cached_memory()
