"""Drop-in ``MRATree`` with pyMRA's constructor, ``getLikelihood()`` and ``predict()``.

Mirrors the public surface of pyMRA/MRATree.py:

* ``MRATree(locs, r, cov, obs, R, M=-1, J=-1, critDepth=-1, verbose=True)``   MRATree.py:23
  (``R``: a Python float, or a 1-D float array of N per-observation noise variances - the diagonal of the matrix ``R`` that
  MRANode.py:85-88 slices per child; ``setNoise`` re-sets it on the same tree)
* ``getLikelihood()`` -> 1x1 ``np.matrix`` (root.d + root.u)                  MRATree.py:82-84
* ``predict()`` -> (N x 1 ``np.matrix`` mean, (N,) ``ndarray`` sd)            MRATree.py:90-94
* attributes ``locs, d, r, J, M, obs_inds, root`` with ``root.d, root.u, root.mean, root.var``
* beyond pyMRA: ``cov_locs`` / ``metric="chordal"`` - the covariance is evaluated on other coordinates (N x k, k <= 3) than the
  ones the tree is partitioned on: points on a sphere keep a (lon, lat) tree and get chordal distances from their xyz

As in the reference all the work happens in the constructor - here it is: replay the tree on
the host (pymra_amd.topology), hand the flat tree + locations + observations to libmra_hip.so
through ctypes, run the HIP path once, copy the results back.  No NumPy fallback exists: without
the library or without a GPU the constructor raises.

``cov`` plug-in: the user's two-argument callable is probed once with symbolic location handles.
If it is built from this package's kernels (``mt.ExpCovFun``, ``mt.Matern32`` ... possibly times a
scalar) the probe yields a ``KernelSpec`` and the kernel is evaluated on the GPU.  Other callables
and dense ``np.matrix``/``ndarray`` covariances are evaluated block by block on the host and uploaded
(``MRA_KERNEL_HOST``, ``HipPlan.upload_host_cov``); everything else still runs on the GPU.

``critDepth`` is accepted for signature compatibility.  The reference's parallel mode forks one
process per subtree at that depth (MRANode.py:90-104); the forked children inherit the same RNG
state, so its 2-D knot draws - and therefore its results - differ from the serial mode.  This
implementation always reproduces the serial (default) mode; GPU parallelism is over all nodes of
a level, and multi-GPU sharding lives in pymra_amd.sharding.
"""
from __future__ import annotations

import logging
import os

import numpy as np

from . import MRATools as mt
from .plan import HipPlan, create_with_replay
from .topology import build_topology, resolve_tree_shape

logger = logging.getLogger("pyMRA.MRATree")


class CVResult:
    """What ``MRATree.crossValidate`` returns (its docstring lists the fields)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def __repr__(self):
        return "CVResult(kind=%r, n=%d, score=%.6g, leverage_max=%.4g)" % (self.kind, self.n, self.score, self.leverage_max)


class RootView:
    """The attributes of the reference's root ``Node`` that callers read (pyMRA/MRANode.py:26-45, 378-391,
    444-520).  ``d, u, mean, var`` come from the GPU pass; ``knots, B, kInv, k`` (the root's prior blocks,
    cov(locs, knots) etc.) are evaluated lazily on the host from the kernel when somebody asks."""

    def __init__(self, d, u, mean, var, N, topo, locs=None, kernel=None):
        self.d = np.matrix([[d]])
        self.u = np.matrix([[u]])
        self.mean = np.asmatrix(mean).reshape(N, 1) if mean is not None else None      # a view: no 8 MB copy
        self.var = var
        self.N = N
        self.res = 0
        self.ID = "r"
        self.leaf = bool(topo.node_leaf[0])
        kq = topo.knot_rows[topo.knot_ptr[0]:topo.knot_ptr[1]]
        self.kInds = np.sort(topo.perm[kq])
        self.children = []
        self.locs = locs
        self._kernel = kernel

    @property
    def knots(self):
        return np.asarray(self.locs)[self.kInds]

    @property
    def B(self):
        if self._kernel is None:
            raise AttributeError("root.B needs a device kernel (KernelSpec) to be evaluated lazily")
        return np.matrix(self._kernel.evaluate(np.asarray(self.locs), self.knots))

    @property
    def kInv(self):
        return self.B[self.kInds, :]

    @property
    def k(self):
        return np.linalg.inv(self.kInv)


def probe_cov(cov, d, locs=None):
    """Return a KernelSpec - or a KernelSum, for a sum of them - if ``cov`` is expressible as one of the device kernels, else None."""
    if isinstance(cov, (mt.KernelSpec, mt.KernelSum)):
        return cov
    if not callable(cov):
        return None
    try:
        out = cov(mt.SymbolicLocs("a", d, locs), mt.SymbolicLocs("b", d, locs))
    except Exception:
        return None
    return out if isinstance(out, (mt.KernelSpec, mt.KernelSum)) else None


def _check_noise(R, N):
    """The `R` argument: a Python float (scalar nugget) -> (R, False); a 1-D float array of N per-observation variances, the
    diagonal of the reference's matrix R (pyMRA/MRANode.py:85-88) -> (float64 array, True)."""
    if isinstance(R, float):
        return R, False
    if isinstance(R, np.ndarray) and R.dtype.kind == "f":
        if R.ndim != 1:
            raise ValueError("R must be a float or a 1-D array of per-observation variances: only a diagonal R is supported, "
                             "not a %d-D array (correlated noise)" % R.ndim)
        if len(R) != N:
            raise ValueError("a noise vector R must have one entry per location (%d), got %d" % (N, len(R)))
        return np.ascontiguousarray(R, dtype=np.float64), True
    # the reference indexes a non-float R as a matrix (MRANode.py:85-88) and fails on an int
    raise TypeError("R must be a Python float (scalar nugget variance) or a 1-D float array (per-observation variances); got %r" % type(R))


class MRATree(object):

    def __init__(self, locs, r, cov, obs, R, M=-1, J=-1, critDepth=-1, verbose=True, device=0,
                 want_predict=True, cov_locs=None, metric="euclidean", radius=1.0, X=None, local_range=None):
        """local_range: None, or N positive local ranges lam(s), one per location: a nonstationary covariance (mt.LocalRange, DESIGN.md
        section 25).  ``cov`` is then one of ExpCovFun, Matern32, Matern52 or GaussianCovFun on the spatial locations, its l a
        multiplier of the whole range field; the covariance coordinates become [locs | lam] and the sites of predictAt and its
        siblings are (n, d) with a mandatory local_range= of n values.  Not together with cov_locs or metric="chordal".
        X: None, or (N, p) covariates of a regression trend y = X beta + x + eps with a flat prior on beta (p <= 63; an intercept
        is a column of ones): see setTrend.
        cov_locs: N x k (k <= 3) coordinates the covariance is evaluated on, when they are not ``locs``; ``locs`` still builds
        the tree.  metric="chordal": ``locs`` are (lon, lat) in degrees on a sphere of the given radius and the covariance sees
        their chordal distances (cov_locs = mt.lonlat_to_xyz(locs, radius)); the sites of predictAt and its siblings are (lon, lat)
        too.  Under an explicit cov_locs the sites are given in covariance coordinates (n x k)."""
        self.locs = locs
        self.d = np.shape(self.locs)[1]
        N = len(locs)
        if metric not in ("euclidean", "chordal"):
            raise ValueError('metric must be "euclidean" or "chordal"')
        self.metric, self.radius = metric, float(radius)
        self.local_range = None
        if local_range is not None:
            if cov_locs is not None:
                raise ValueError("local_range builds the covariance coordinates [locs | lam] itself: do not pass cov_locs as well")
            if metric == "chordal":
                raise ValueError('local_range cannot be combined with metric="chordal" (the sphere would need four coordinate columns)')
            if np.ndim(locs) != 2 or self.d not in (1, 2):
                raise ValueError("local_range needs locs of shape (N, 1) or (N, 2): the range is the covariance's last of at most three columns")
            self.local_range = mt._check_ranges(local_range, N)
            cov_locs = np.column_stack([np.asarray(locs, dtype=np.float64), self.local_range])
        if metric == "chordal":
            if cov_locs is not None:
                raise ValueError('metric="chordal" derives the covariance coordinates from locs: do not pass cov_locs as well')
            if np.ndim(locs) != 2 or self.d != 2:
                raise ValueError('metric="chordal" needs locs of shape (N, 2): longitude and latitude in degrees')
            cov_locs = mt.lonlat_to_xyz(locs, self.radius)
        self._split_coords = cov_locs is not None           # the covariance has coordinates of its own
        if self._split_coords:
            cov_locs = np.ascontiguousarray(np.asarray(cov_locs, dtype=np.float64))
            if cov_locs.ndim == 1:
                cov_locs = cov_locs.reshape(-1, 1)
            if cov_locs.ndim != 2 or len(cov_locs) != N or not 1 <= cov_locs.shape[1] <= 3:
                raise ValueError("cov_locs must have shape (N, k) with N = %d and k <= 3" % N)
            if not np.all(np.isfinite(cov_locs)):
                raise ValueError("cov_locs must be finite")
            self.cov_locs = cov_locs
        else:
            self.cov_locs = np.asarray(locs, dtype=np.float64)
        self.cov_d = self.cov_locs.shape[1] if self.cov_locs.ndim == 2 else 1      # dimension the covariance is evaluated in
        self.r = r
        self.M, self.J = resolve_tree_shape(N, self.d, r, M, J)
        if critDepth < 0:
            critDepth = self.M + 1
        self.critDepth = critDepth
        R_in = R
        R, noise_vector = _check_noise(R, N)
        obs_arr = np.asarray(obs, dtype=np.float64)
        self._obs_inds = None                   # (the reference's obs_inds, MRATree.py:62: computed when somebody reads it)
        self.obs, self.R = obs_arr, R_in
        if noise_vector:
            # checked before anything is built; the scalar that the one-call constructor takes is only a placeholder
            ro = R[np.isfinite(obs_arr.reshape(-1))] if obs_arr.size == N else R
            if not (np.all(np.isfinite(ro)) and np.all(ro >= 0.0)):
                raise ValueError("the noise variance of an observed location is negative or not finite")

        spec = self._probe(cov)
        if spec is not None and spec.circular and self.cov_d != 1:
            raise ValueError("circular distances are defined for 1-D locations only")
        if spec is None and not callable(cov) and not isinstance(cov, np.ndarray):
            raise TypeError("cov must be a callable cov(locs1, locs2) or a dense N x N matrix")
        self._check_spec_metric(spec)
        self.kernel = spec          # None: opaque callable / dense matrix -> values come from the host

        logger.debug('r: %d, \tJ: %d,\tM: %d' % (self.r, self.J, self.M))
        # large 2-D trees: tree replay, plan construction and the uploads in one library call (the plan is built beside the
        # sequential knot draws); everything else - 1-D, small nodes, KMeans rules - the general path
        R_scalar = (float(ro.mean()) if ro.size and ro.mean() > 0.0 else 1.0) if noise_vector else R
        # (covariance coordinates of their own: the general path - the native 2-D replay still builds the tree)
        both = create_with_replay(locs, r, self.M, self.J, obs_arr, R_scalar, device) if self.d == 2 and not self._split_coords else None
        if both is not None:
            self.plan, self.topology = both
            if noise_vector:
                self.plan.set_noise(R)          # (the one-call constructor takes a scalar: the vector goes in before the first run)
        else:
            self.topology = build_topology(np.asarray(locs, dtype=np.float64), r, self.M, self.J,
                                           coord_dim=self.cov_d if self._split_coords else None)
            self.plan = HipPlan(self.topology, device=device)
            self.plan.set_locs(self.cov_locs if self._split_coords else locs)
            self.plan.set_obs(obs_arr, R)
        if spec is not None:
            if spec.A is not None:
                self.plan.set_metric(spec.A)        # (before the kernel, as reevaluate sends it)
            self.plan.set_kernel(spec.kind, spec.l, spec.sig, spec.scale, spec.circular, spec.nu)
        else:
            # cov-callable plug-in for anything the device cannot evaluate itself (pyMRA/MRANode.py:73-80,
            # 381-384): the host evaluates the raw covariance blocks, the GPU does everything else
            self.plan.upload_host_cov(cov, self.cov_locs if self._split_coords else locs, obs_arr)     # (the callable sees the covariance coordinates)
        self.plan.run(likelihood=True, predict=want_predict)
        d, u = self.plan.likelihood()
        if want_predict:
            mean, var, self._sd = self.plan.predict(with_sd=True)      # (sd beside var: predict() returns it, as the reference's np.sqrt(root.var))
        else:
            mean, var, self._sd = None, None, None
        self.root = RootView(d, u, mean, var, N, self.topology, self.cov_locs, spec)
        self._node_blocks = {}
        self.trend, self._X, self._X_arg, self._trend_y = None, None, None, None
        if X is not None:
            self.setTrend(X, want_predict=want_predict)

    # ---- regression trend (HipPlan.set_trend / trend_fit) ----------------------------------------------------------------------------
    def setTrend(self, X, want_predict=True):
        """Set (X: (N, p) covariates in the caller's row order, kept on the device) or clear (None) a regression trend
        y = X beta + x + eps with a flat prior on beta, fit it by generalised least squares from this tree's factors and return the
        likelihood.  With a trend set, getLikelihood() is the profile -2 log-likelihood (reml=True: the REML criterion), predict() the
        universal-kriging mean and sd (the uncertainty of beta included), ``trend`` the last TrendFit (beta, cov_beta, profile, reml,
        ...), reevaluate(cov) refits it without sending X again, and predictAt needs X_sites."""
        N = len(self.locs)
        self._node_blocks = {}
        if X is None:
            self.plan.set_trend(None)
            self.trend, self._X, self._X_arg, self._trend_y = None, None, None, None
            self.plan.run(likelihood=True, predict=want_predict)
            d, u = self.plan.likelihood()
            mean, var, self._sd = self.plan.predict(with_sd=True) if want_predict else (None, None, None)
            self.root = RootView(d, u, mean, var, N, self.topology, self.cov_locs, self.kernel)
            return self.getLikelihood()
        self._send_trend(X)
        self._trend_y = None
        self._fit_trend(want_predict)
        return self.getLikelihood()

    def _send_trend(self, X):
        """Check X ((N, p), finite) and send it to the device; ``_X_arg`` remembers the caller's own array."""
        N = len(self.locs)
        if self.kernel is None:
            raise NotImplementedError("a trend needs a device kernel: trees built from an opaque callable or a dense matrix cannot fit one")
        arg, X = X, np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        if X.ndim != 2 or X.shape[0] != N or X.shape[1] < 1:
            raise ValueError("X must have shape (N, p) with N = %d and p >= 1" % N)
        if not np.all(np.isfinite(X)):
            raise ValueError("X must be finite")
        self.plan.set_trend(X)
        self._X, self._X_arg = X, arg

    def _fit_trend(self, want_predict):
        fit = self.plan.trend_fit(predict=want_predict)
        self.trend = fit
        self._sd = np.sqrt(fit.var) if want_predict else None
        self.root = RootView(fit.d, fit.u, fit.mean, fit.var, len(self.locs), self.topology, self.cov_locs, self.kernel)

    def _no_trend(self, what):
        if self.trend is not None:
            raise NotImplementedError("%s does not support a regression trend yet (this tree has one: setTrend(None) clears it)" % what)

    def _probe(self, cov):
        """probe_cov on this tree's covariance coordinates; on a tree with local ranges ``cov`` is probed on the spatial locations and
        must be one of the four stationary base kernels, which mt.LocalRange wraps (its ValueErrors are the refusals)."""
        if self.local_range is None:
            return probe_cov(cov, self.cov_d, self.cov_locs)
        if isinstance(cov, mt.LocalRange):
            return mt.LocalRange(cov.base, self.local_range)
        base = probe_cov(cov, self.d, self.locs)
        if not isinstance(base, mt.KernelSpec):
            raise ValueError("with local_range, cov must be ExpCovFun, Matern32, Matern52 or GaussianCovFun on the spatial locations "
                             "(not a sum, an opaque callable or a matrix)")
        return mt.LocalRange(base, self.local_range)

    def setLocalRange(self, local_range, want_predict=False):
        """Another range field on the same tree (an MLE over a parametric lam(s; theta)): uploads the covariance coordinates
        [locs | lam] again, which drops what set_locs drops (the retained factors and the kept prior), runs a pass and returns the
        likelihood.  The tree, its knots and its observations stand."""
        if self.local_range is None:
            raise ValueError("this tree was built without local_range")
        lam = mt._check_ranges(local_range, len(self.locs))
        self.local_range = lam
        self.cov_locs = np.column_stack([np.asarray(self.locs, dtype=np.float64), lam])
        self.kernel = mt.LocalRange(self.kernel.base, lam)
        self._node_blocks = {}
        self.plan.set_locs(self.cov_locs)
        if self.trend is not None:
            self._fit_trend(want_predict)
            return self.getLikelihood()
        self.plan.run(likelihood=True, predict=want_predict)
        d, u = self.plan.likelihood()
        mean, var, self._sd = self.plan.predict(with_sd=True) if want_predict else (None, None, None)
        self.root = RootView(d, u, mean, var, len(self.locs), self.topology, self.cov_locs, self.kernel)
        return self.getLikelihood()

    def _check_spec_metric(self, spec):
        """A kernel's metric A (``mt.Matern32(..., metric=A)``) lives in the covariance coordinates: cov_d x cov_d (3 x 3 on the xyz
        coordinates under metric="chordal")."""
        if spec is not None and spec.A is not None and spec.A.shape != (self.cov_d, self.cov_d):
            raise ValueError("the kernel's metric must be a %d x %d matrix (the covariance is evaluated on %d coordinates), got shape %r"
                             % (self.cov_d, self.cov_d, self.cov_d, spec.A.shape))

    def _send_kernel(self, spec):
        """The kernel of a later pass on the same plan: a changed metric (or its removal) first, then the kernel."""
        old = self.kernel.A if self.kernel is not None else None
        if (spec.A is None) != (old is None) or (spec.A is not None and not np.array_equal(spec.A, old)):
            self.plan.set_metric(spec.A)
        self.kernel = spec
        self.plan.set_kernel(spec.kind, spec.l, spec.sig, spec.scale, spec.circular, spec.nu)

    @property
    def obs_inds(self):
        if self._obs_inds is None:
            self._obs_inds = np.where(np.logical_not(np.isnan(self.obs)))[0]
        return self._obs_inds

    def getLikelihood(self, reml=False):
        """d + u of the last pass; with a trend the profile -2 log-likelihood, or with reml=True the REML criterion (+ log det X^T K^-1 X)."""
        if self.trend is not None and reml:
            return np.matrix([[self.trend.reml]])
        if reml:
            raise ValueError("reml=True needs a trend (setTrend)")
        return self.root.d + self.root.u

    def predict(self):
        if self.root.mean is None:
            raise RuntimeError("constructed with want_predict=False")
        xP = self.root.mean
        sdP = self._sd if self._sd is not None else np.sqrt(self.root.var)
        return xP, sdP

    def simulate(self, nsim=1, distr="prior", seed=None):
        """(N, nsim) exact draws of the field in the caller's row order: from the MRA prior (distr="prior") or from the posterior
        given this tree's observations (distr="posterior"; conditioning by kriging, one device pass per draw).  Rows outside every
        leaf are 0, as in predict().  seed=None takes a 64-bit seed from NumPy's global RNG (np.random.seed makes runs repeatable).
        The scalable counterpart of pyMRA's dense simulate1D / simulateGRF (pyMRA/MRATools.py:395-484); getLikelihood() and
        predict() are unchanged afterwards."""
        self._no_trend("simulate")
        if distr not in ("prior", "posterior"):
            raise ValueError('distr must be "prior" or "posterior"')
        if self.kernel is None:
            raise NotImplementedError("simulate needs a device kernel: trees built from an opaque callable or a dense matrix cannot sample")
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)) * 2 + int(np.random.randint(0, 2))
        x = self.plan.sample(nsim, seed=seed, conditional=(distr == "posterior"))
        t = self.topology
        rows = (t.perm >= 0) & np.asarray(t.in_leaf, dtype=bool)
        out = np.zeros((len(self.locs), int(nsim)))
        out[t.perm[rows], :] = x[:, rows].T
        return out

    def solve(self, Y):
        """Kriging means and the quadratic form for c observation vectors at once, from ONE factorisation of this tree (the
        factors do not depend on the observed values).  Y: (N,) or (N, c) in the caller's row order, on this tree's observation
        mask (values at unobserved locations are ignored).  -> (mean (N, c), quad (c, c)): mean[:, k] is what predict() gives for
        observations Y[:, k] (rows outside every leaf 0), quad = Y_o^T (Sigma_MRA + R I)^-1 Y_o - exact within blocks of 16 columns,
        NaN between columns of different blocks.  getLikelihood() and predict() are unchanged afterwards."""
        if self.kernel is None:
            raise NotImplementedError("solve needs a device kernel: trees built from an opaque callable or a dense matrix cannot solve")
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y.reshape(-1, 1)
        if Y.ndim != 2 or Y.shape[0] != len(self.locs):
            raise ValueError("Y must have shape (N,) or (N, c) with N = %d" % len(self.locs))
        t = self.topology
        real = t.perm >= 0
        Yp = np.zeros((Y.shape[1], t.P))
        Yp[:, real] = Y[t.perm[real], :].T
        m, quad = self.plan.solve(Yp)
        rows = real & np.asarray(t.in_leaf, dtype=bool)
        mean = np.zeros((len(self.locs), Y.shape[1]))
        mean[t.perm[rows], :] = m[:, rows].T
        return mean, quad

    def crossValidate(self, kind="loo", trend=None):
        """Cross-validation of the fitted model without a refit, from the factors this tree's pass left on the device: every observed
        location left out on its own (kind="loo") or the observed locations of each leaf left out together (kind="leaf": spatial block
        cross-validation on the tree's own partition).  -> CVResult, per-row fields in the caller's row order and NaN where nothing
        is observed: mean and sd of the leave-out predictive distribution of a new observation (noise included), z = (y - mean) / sd,
        lpd = the marginal log predictive density; leaf_lpd {leaf node: log predictive density of its group (kind="leaf": joint)};
        score = their sum, the CV log score; n rows scored; leverage_max = max v / R (float64 loses about eps / (1 - leverage)^2);
        dlik_dR = the exact derivative of getLikelihood() with respect to a nugget added to every observed row.  getLikelihood() and
        predict() are unchanged afterwards.
        On a tree with a trend (setTrend) ``trend`` chooses what leaving a group out means: "refit" - beta is estimated again
        without the group (universal-kriging cross-validation; X without the group must keep full column rank), "fixed" - the beta^ of
        the full fit is plugged in.  The result also has trend (the choice), dlik_dR_reml (the derivative of
        getLikelihood(reml=True)), and leverage_max is the largest (v + |w|^2) / R under "refit".  A tree without a trend takes
        trend=None only (its result has trend = None and dlik_dR_reml = None)."""
        if self.trend is None and trend is not None:
            raise ValueError("trend=%r given, but this tree has no trend (setTrend)" % (trend,))
        if self.trend is not None and trend is None:
            raise NotImplementedError('crossValidate on a tree with a regression trend needs trend="refit" (beta estimated again without '
                                      'each group) or trend="fixed" (the full fit\'s beta plugged in)')
        if trend not in (None, "refit", "fixed"):
            raise ValueError('trend must be "refit" or "fixed"')
        if self.trend is not None and self._trend_y is not None:
            raise NotImplementedError("crossValidate after fitLaplace(X=X) is not supported: the trend of this tree was fitted to the "
                                      "pseudo-observations of a Laplace fit (HipPlan.cv_trend scores those)")
        if kind not in ("loo", "leaf"):
            raise ValueError('kind must be "loo" or "leaf"')
        if self.kernel is None:
            raise NotImplementedError("crossValidate needs a device kernel: trees built from an opaque callable or a dense matrix cannot cross-validate")
        if trend is None:
            mean, var, lpd, group, info = self.plan.cv(leaf=(kind == "leaf"))
            dlik, dlik_reml = float(info[6] - info[7]), None
        else:
            mean, var, lpd, group, info = self.plan.cv_trend(leaf=(kind == "leaf"), refit=(trend == "refit"))
            dlik, dlik_reml = float(info[10]), float(info[11])
        yp = self.plan.buffer(11)
        t = self.topology
        rows = t.perm >= 0
        N = len(self.locs)

        def by_caller(v):
            out = np.full(N, np.nan)
            out[t.perm[rows]] = v[rows]
            return out
        sd = np.sqrt(var)
        nodes = np.nonzero(~np.isnan(group))[0]
        return CVResult(kind=kind, mean=by_caller(mean), sd=by_caller(sd), z=by_caller((yp - mean) / sd), lpd=by_caller(lpd),
                        leaf_lpd={int(i): float(group[i]) for i in nodes}, score=float(info[2]), n=int(info[0]),
                        leverage_max=float(info[5]), dlik_dR=dlik, trend=trend, dlik_dR_reml=dlik_reml)

    def _sites(self, sites, local_range=None):
        """The caller's sites, checked, in covariance coordinates: (lon, lat) degrees -> xyz under metric="chordal", else as given
        (n x k under an explicit cov_locs, n x d otherwise).  The public calls convert once and hand the result to the private
        _locate / _predict_at / _covariance_at, which take covariance coordinates.  On a tree with local ranges the sites are (n, d)
        spatial locations and local_range their n ranges, mandatory: -> [sites | local_range]."""
        X = np.asarray(sites, dtype=np.float64)
        if self.local_range is not None:
            if local_range is None:
                raise ValueError("this tree has local ranges: the sites need local_range=, one positive range per site")
            if X.ndim == 1 and self.d == 1:
                X = X.reshape(-1, 1)
            if X.ndim != 2 or X.shape[1] != self.d:
                raise ValueError("sites must have shape (n, %d)" % self.d)
            if not np.all(np.isfinite(X)):
                raise ValueError("sites must be finite")
            return np.column_stack([X, mt._check_ranges(local_range, len(X))])
        if local_range is not None:
            raise ValueError("local_range given, but this tree was built without local ranges")
        din = 2 if self.metric == "chordal" else self.cov_d
        if X.ndim == 1 and din == 1:
            X = X.reshape(-1, 1)
        if X.ndim != 2 or X.shape[1] != din:
            raise ValueError("sites must have shape (n, %d)" % din)
        if not np.all(np.isfinite(X)):
            raise ValueError("sites must be finite")
        if self.metric == "chordal":
            X = mt.lonlat_to_xyz(X, self.radius)
        return X

    def locate(self, sites, local_range=None):
        """int32[n]: for each site the leaf (node index) of the nearest tree location that the tree reports - locations a 1-D split
        drops never win; on a circular 1-D kernel the distance wraps at 1.  The rule serves every partition of the tree replay
        (quadrants, terciles, knot boundaries, KMeans) and sends a site that coincides with a tree location to that location's leaf.
        Any assignment of sites to leaves gives a valid process: predictAt(leaf=...) overrides this one.  On a tree with local ranges
        "nearest" is nearest in space: the range column does not enter."""
        return self._locate(self._sites(sites, local_range))

    def _locate(self, X):
        from scipy.spatial import cKDTree
        t = self.topology
        if getattr(self, "_locator", None) is None:
            rows = np.nonzero((t.perm >= 0) & np.asarray(t.in_leaf, dtype=bool))[0]
            leaf_of = np.full(t.P, -1, dtype=np.int32)
            for i in np.nonzero(np.asarray(t.node_leaf, dtype=bool))[0]:
                leaf_of[int(t.node_row0[i]):int(t.node_row1[i])] = i
            # (nearest in covariance coordinates: by chord is by great circle, so the date line needs no special case)
            pts = np.asarray(self.cov_locs, dtype=np.float64).reshape(len(self.locs), -1)[t.perm[rows]]
            if self.local_range is not None:
                pts = pts[:, :self.d]               # (the last column is a range, no coordinate: it never moves)
            wrap = self.kernel is not None and self.kernel.circular
            self._locator = (cKDTree(np.mod(pts, 1.0) if wrap else pts, boxsize=1.0 if wrap else None), leaf_of[rows], wrap)
        kd, leaves, wrap = self._locator
        workers = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
        if self.local_range is not None:
            X = X[:, :self.d]
        return leaves[kd.query(np.mod(X, 1.0) if wrap else X, workers=workers)[1]].astype(np.int32)

    def predictAt(self, sites, Y=None, leaf=None, X_sites=None, local_range=None):
        """Posterior mean and standard deviation of the latent field at locations that need not be rows of `locs`, from this tree's
        factors - the tree (its knots, its likelihood) stays the one that was fitted.  sites: (n, d) - under metric="chordal" (n, 2)
        longitude / latitude in degrees, under an explicit cov_locs (n, k) in the covariance coordinates, here and in locate,
        covarianceAt, simulateAt and sampleAt; Y: None (this tree's observations) or (N,) / (N, c) observation vectors in the
        caller's row order on this tree's mask, as for solve(); leaf: None (locate(sites)) or int32[n] leaf node indices.  -> (mean (n, c), sd (n,)); add R to sd ** 2 for a new observation.  At a
        location of the tree, in that location's leaf, these are predict()'s values.  getLikelihood() and predict() are unchanged.
        With a trend (setTrend) X_sites, the (n, p) covariates at the sites, is mandatory and Y must be None: the result is the
        universal-kriging mean (n, 1) and sd (n,) for this tree's observations."""
        if self.kernel is None:
            raise NotImplementedError("predictAt needs a device kernel: trees built from an opaque callable or a dense matrix cannot predict at new sites")
        if self.trend is None:
            if X_sites is not None:
                raise ValueError("X_sites given, but this tree has no trend (setTrend)")
            return self._predict_at(self._sites(sites, local_range), Y, leaf)
        S = self._sites(sites, local_range)
        if X_sites is None:
            raise ValueError("this tree has a trend: predictAt needs X_sites, the (n, p) covariates at the sites")
        if Y is not None:
            raise NotImplementedError("predictAt with a trend predicts from this tree's own observations (Y must be None)")
        p = self._X.shape[1]
        Xs = np.asarray(X_sites, dtype=np.float64)
        if Xs.ndim == 1 and p == 1:
            Xs = Xs.reshape(-1, 1)
        if Xs.shape != (len(S), p) or not np.all(np.isfinite(Xs)):
            raise ValueError("X_sites must be a finite array of shape (n, p) = (%d, %d)" % (len(S), p))
        # zero-mean kriging of the columns [y | X] at the sites, then the formulas of the fit on the host
        # (the y of the fit: this tree's observations, or the pseudo-observations t of fitLaplace(X=...))
        y_fit = self.obs if self._trend_y is None else self._trend_y
        YX = np.column_stack([np.nan_to_num(np.asarray(y_fit, dtype=np.float64).reshape(-1)), self._X])
        m, sd = self._predict_at(S, YX, leaf)
        h = Xs - m[:, 1:]
        mean = m[:, 0] + h @ self.trend.beta
        var = sd ** 2 + np.einsum("ij,jk,ik->i", h, self.trend.cov_beta, h)
        return mean.reshape(-1, 1), np.sqrt(var)

    def _predict_at(self, X, Y=None, leaf=None):
        if leaf is None:
            leaf = self._locate(X)
        leaf = np.asarray(leaf)
        if leaf.shape != (len(X),):
            raise ValueError("leaf must have shape (n,) = (%d,)" % len(X))
        Yp = None
        if Y is not None:
            Y = np.asarray(Y, dtype=np.float64)
            if Y.ndim == 1:
                Y = Y.reshape(-1, 1)
            if Y.ndim != 2 or Y.shape[0] != len(self.locs):
                raise ValueError("Y must have shape (N,) or (N, c) with N = %d" % len(self.locs))
            t = self.topology
            real = t.perm >= 0
            Yp = np.zeros((Y.shape[1], t.P))
            Yp[:, real] = Y[t.perm[real], :].T
        mean, var = self.plan.predict_sites(X, leaf, Yp)
        return np.ascontiguousarray(mean.T), np.sqrt(var)

    def covarianceAt(self, sites, distr="posterior", leaf=None, local_range=None):
        """(n, n) joint covariance of the latent field at locations that need not be rows of `locs`, from this tree's factors:
        the posterior given this tree's observations (distr="posterior": its diagonal is predictAt's sd ** 2) or the prior
        (distr="prior").  sites: (n, d), (lon, lat) or covariance coordinates as for predictAt; leaf: None (locate(sites)) or
        int32[n] leaf node indices.  Symmetric to the bit; positive
        semi-definite down to roundoff only (duplicated sites and the Iden kernel make it singular).  w @ covarianceAt(grid) @ w is
        the variance of the functional w . x over a prediction grid.  getLikelihood() and predict() are unchanged."""
        if distr not in ("prior", "posterior"):
            raise ValueError('distr must be "prior" or "posterior"')
        if self.kernel is None:
            raise NotImplementedError("covarianceAt needs a device kernel: trees built from an opaque callable or a dense matrix cannot evaluate it at new sites")
        return self._covariance_at(self._sites(sites, local_range), distr, leaf)

    def _covariance_at(self, X, distr, leaf):
        if leaf is None:
            leaf = self._locate(X)
        leaf = np.asarray(leaf)
        if leaf.shape != (len(X),):
            raise ValueError("leaf must have shape (n,) = (%d,)" % len(X))
        return self.plan.sites_cov(X, leaf, posterior=(distr == "posterior"))

    def simulateAt(self, sites, nsim, distr="posterior", seed=None, leaf=None, z=None, local_range=None):
        """(n, nsim) draws of the latent field at locations that need not be rows of `locs`: mean + F z, with mean predictAt's for
        this tree's observations (0 for distr="prior"), F the symmetric square root of covarianceAt(sites, distr, leaf) (numpy.linalg.eigh,
        eigenvalues below 0 set to 0) and z (n, nsim) given, or standard normals from numpy.random.default_rng(seed)."""
        self._no_trend("simulateAt")
        if self.kernel is None:
            raise NotImplementedError("simulateAt needs a device kernel: trees built from an opaque callable or a dense matrix cannot simulate at new sites")
        if distr not in ("prior", "posterior"):
            raise ValueError('distr must be "prior" or "posterior"')
        X = self._sites(sites, local_range)
        if leaf is None:
            leaf = self._locate(X)
        S = self._covariance_at(X, distr, leaf)
        n = len(X)
        nsim = int(nsim)
        if z is None:
            z = np.random.default_rng(seed).standard_normal((n, nsim))
        z = np.asarray(z, dtype=np.float64)
        if z.shape != (n, nsim):
            raise ValueError("z must have shape (n, nsim) = (%d, %d)" % (n, nsim))
        lam, Q = np.linalg.eigh(S)
        F = (Q * np.sqrt(np.maximum(lam, 0.0))) @ Q.T
        x = F @ z
        if distr == "posterior" and n:
            x += self._predict_at(X, leaf=leaf)[0]
        return x

    def sampleAt(self, sites, nsim, distr="posterior", seed=None, leaf=None, z=None, local_range=None):
        """(n, nsim) draws of the latent field at locations that need not be rows of `locs`, at any number of sites: the scalable
        counterpart of simulateAt (no dense n x n matrix; a leaf may receive up to plan.MRA_SAMPLE_SITES_LEAF_MAX distinct sites).
        distr="posterior": draws given this tree's observations, predictAt's mean included; distr="prior": mean 0.  Their covariance
        is covarianceAt(sites, distr, leaf).  seed=None takes a 64-bit seed from NumPy's global RNG, as simulate() does; z: None
        (Philox draws on the device, a pure function of the seed) or (plan.sample_sites_slots(n), nsim) latent draws - the non-leaf
        nodes' slots first, shared with simulate(), then one per site.  leaf: None (locate(sites)) or int32[n] leaf node indices.
        getLikelihood() and predict() are unchanged."""
        self._no_trend("sampleAt")
        if distr not in ("prior", "posterior"):
            raise ValueError('distr must be "prior" or "posterior"')
        if self.kernel is None:
            raise NotImplementedError("sampleAt needs a device kernel: trees built from an opaque callable or a dense matrix cannot simulate at new sites")
        X = self._sites(sites, local_range)
        if leaf is None:
            leaf = self._locate(X)
        leaf = np.asarray(leaf)
        if leaf.shape != (len(X),):
            raise ValueError("leaf must have shape (n,) = (%d,)" % len(X))
        nsim = int(nsim)
        if z is not None:
            z = np.asarray(z, dtype=np.float64)
            slots = self.plan.sample_sites_slots(len(X))
            if z.shape != (slots, nsim):
                raise ValueError("z must have shape (sample_sites_slots(n), nsim) = (%d, %d)" % (slots, nsim))
            z = np.ascontiguousarray(z.T)
        elif seed is None:
            seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)) * 2 + int(np.random.randint(0, 2))
        x = self.plan.sample_sites(X, leaf, nsim, seed=seed or 0, z=z, posterior=(distr == "posterior"))
        return np.ascontiguousarray(x.T)

    def _cov_apply(self, A, distr):
        """Sigma A (or Sigma_post A) for A (N, c) in the caller's row order -> (A at the reported rows else 0 (N, c), out (N, c))."""
        if distr not in ("prior", "posterior"):
            raise ValueError('distr must be "prior" or "posterior"')
        if self.kernel is None:
            raise NotImplementedError("covariance needs a device kernel: trees built from an opaque callable or a dense matrix cannot apply it")
        t = self.topology
        rows = (t.perm >= 0) & np.asarray(t.in_leaf, dtype=bool)
        Ap = np.zeros((A.shape[1], t.P))
        Ap[:, rows] = A[t.perm[rows], :].T
        o, _ = self.plan.cov_apply(Ap, posterior=(distr == "posterior"), want_gram=False)
        Arep, out = np.zeros(A.shape), np.zeros(A.shape)
        Arep[t.perm[rows], :] = A[t.perm[rows], :]
        out[t.perm[rows], :] = o[:, rows].T
        return Arep, out

    def covariance(self, rows, distr="prior"):
        """(N, len(rows)) columns Sigma[:, rows] of the MRA covariance of the latent field, in the caller's row order: the prior
        (distr="prior": what simulate() draws from, and how well the MRA approximates the kernel) or the posterior given this
        tree's observations (distr="posterior": its diagonal is predict()'s variance).  Rows outside every leaf are 0, as a
        column and as an entry.  getLikelihood() and predict() are unchanged afterwards."""
        rows = np.atleast_1d(np.asarray(rows, dtype=np.int64))
        N = len(self.locs)
        if rows.ndim != 1 or np.any(rows < 0) or np.any(rows >= N):
            raise ValueError("rows must be indices into the %d locations" % N)
        A = np.zeros((N, len(rows)))
        A[rows, np.arange(len(rows))] = 1.0
        return self._cov_apply(A, distr)[1]

    def functionalCovariance(self, A, distr="prior"):
        """(c, c) covariance matrix of the linear functionals A[:, k]^T x of the latent field (a regional mean, a contrast between
        two areas): A^T Sigma A under the prior or the posterior.  A: (N,) or (N, c) in the caller's row order; rows outside every
        leaf do not enter.  The full matrix for any c (the product with Sigma A is formed on the host)."""
        A = np.asarray(A, dtype=np.float64)
        if A.ndim == 1:
            A = A.reshape(-1, 1)
        if A.ndim != 2 or A.shape[0] != len(self.locs):
            raise ValueError("A must have shape (N,) or (N, c) with N = %d" % len(self.locs))
        if not np.all(np.isfinite(A)):
            raise ValueError("A must be finite")
        Arep, out = self._cov_apply(A, distr)
        G = Arep.T @ out
        return 0.5 * (G + G.T)

    def getLikelihoods(self, Y):
        """(c,) likelihoods d + u_k of the columns of Y on this tree's observation mask (getLikelihood() per column; the
        log-determinant d is shared)."""
        _, quad = self.solve(Y)
        return float(np.asarray(self.root.d).ravel()[0]) + np.diag(quad)

    # ---- diagnostics surface (pyMRA/MRATree.py:101-132, 445-511); host-side de-whitening, see pymra_amd.diagnostics
    def getNodeBlocks(self, posterior=True):
        """Per-node ``B, kInv, k, kC`` (+ ``A, omg, kTil, kTilC, BTil[res]``, cumulative ``d, u``) of every node
        in level order - the attributes the reference keeps on its ``Node`` objects (pyMRA/MRANode.py:384-391,
        415-445, 486-507).  Costs two device passes."""
        from .diagnostics import collect_node_blocks
        key = bool(posterior)
        if key not in self._node_blocks:                    # two device passes + one block download per node: kept until reevaluate()
            self._node_blocks[key] = collect_node_blocks(self, posterior=posterior)
        return self._node_blocks[key]

    def getNodesBFS(self, groupByResolution=False):
        """Nodes in breadth-first order (pyMRA/MRATree.py:101-120) as ``NodeBlocks`` records.  (In the reference
        the tree is torn down at the end of construction, MRANode.py:108-111, and only the root is ever seen.)"""
        nodes = self.getNodeBlocks(posterior=True)
        if not groupByResolution:
            return nodes
        return [[nb for nb in nodes if nb.res == m] for m in range(self.topology.n_levels)]

    def getBasisFunctionsMatrix(self, distr="prior", groupByResolution=False, order='root', timesKC=False):
        """pyMRA/MRATree.py:445-511."""
        from .diagnostics import basis_functions_matrix
        return basis_functions_matrix(self, distr, groupByResolution, order, timesKC)

    # re-evaluate with other kernel parameters on the same tree (plan reuse for MLE loops,
    # README.md:96-104 builds a new MRATree per objective call)
    def reevaluate(self, cov, want_predict=False):
        spec = self._probe(cov)
        if spec is None:
            raise NotImplementedError("cov must be a device kernel")
        self._check_spec_metric(spec)
        self._node_blocks = {}
        self._send_kernel(spec)
        if self.trend is not None:           # the trend is refitted from the factors of the new kernel; X stays on the device
            self._fit_trend(want_predict)
            return self.getLikelihood()
        self.plan.run(likelihood=True, predict=want_predict)
        d, u = self.plan.likelihood()
        mean, var, self._sd = self.plan.predict(with_sd=True) if want_predict else (None, None, None)
        self.root = RootView(d, u, mean, var, len(self.locs), self.topology, self.cov_locs, spec)
        return self.getLikelihood()

    def setNoise(self, R, want_predict=False):
        """Re-set the observation noise on the same tree (a Python float, or a 1-D array of N per-observation variances), run a
        pass and return the likelihood - the counterpart of ``reevaluate`` for the noise."""
        R, vector = _check_noise(R, len(self.locs))
        if vector:
            self.plan.set_noise(R)
        else:
            self.plan.set_noise(np.full(len(self.locs), R))
        self.R = R
        self._node_blocks = {}
        if self.trend is not None:
            self._fit_trend(want_predict)
            return self.getLikelihood()
        self.plan.run(likelihood=True, predict=want_predict)
        d, u = self.plan.likelihood()
        mean, var, self._sd = self.plan.predict(with_sd=True) if want_predict else (None, None, None)
        self.root = RootView(d, u, mean, var, len(self.locs), self.topology, self.cov_locs, self.kernel)
        return self.getLikelihood()

    def fitLaplace(self, family, aux=None, offset=None, z=None, x0=None, cov=None, max_iter=50, tol=1e-10, X=None, reml=False):
        """Fit non-Gaussian data on this tree by a Laplace approximation (``HipPlan.fit_laplace``): family "gaussian" (variance
        ``aux``), "poisson" (``offset`` = log exposure) or "binomial" (``aux`` trials), eta = x + offset.  z: N values, finite
        exactly where this tree observes (default: the tree's ``obs``).  cov: other parameters of a device kernel, set without a
        pass of its own (MLE loops).  x0: the start; default the mean of the previous fit when there is one (a warm start), else the
        data-based start.  Updates ``root`` and ``predict()`` to the Laplace posterior N(x^, (Sigma^-1 + D)^-1), keeps the numbers
        of the fit in ``self.laplace`` and returns -2 log q(z); ``getLikelihood()`` keeps its meaning, d + u of the last pass.
        X: (N, p) covariates of a regression trend, eta = X beta + x + offset with a flat prior on beta
        (``HipPlan.fit_laplace_trend``).  X is sent to the device only when it is not the very array sent last (the object is
        compared, not its values: pass a new array after changing one in place); x0 is then the start of e = X beta + x, by default the
        e^ of the previous such fit.  Returns the profile -2 log q (beta at its mode), or with reml=True the value with beta
        integrated out; afterwards ``trend`` holds beta and cov_beta, predict() is the mean and sd of e = X beta + x with the
        uncertainty of beta in it, and predictAt(sites, X_sites=...) serves the same at new sites (exp(mean + log exposure) is a
        fitted count).  The plan then holds the pseudo-observations t and their noise 1 / D: a later setNoise(R) or reevaluate(cov)
        refits a Gaussian trend on t (with the caller's R in place of 1 / D) and is no Laplace fit any more - call fitLaplace(X=X,
        cov=...) again for other kernel parameters.  Without X a tree that has a trend is refused."""
        if X is not None:
            return self._fit_laplace_trend(family, aux, offset, z, x0, cov, max_iter, tol, X, reml)
        if reml:
            raise ValueError("reml=True needs X")
        self._no_trend("fitLaplace")
        if cov is not None:
            spec = self._probe(cov)
            if spec is None:
                raise NotImplementedError("cov must be a device kernel")
            self._check_spec_metric(spec)
            self._send_kernel(spec)
        if z is None:
            z = self.obs
        if x0 is None:
            x0 = getattr(self, "_laplace_mean", None)
        self._node_blocks = {}
        res = self.plan.fit_laplace(family, z, aux=aux, offset=offset, x0=x0, max_iter=max_iter, tol=tol)
        mean, var, self._sd = self.plan.predict(with_sd=True)
        self._laplace_mean = mean.copy() if res["converged"] else None      # (a fit that did not converge is no start for the next)
        self.laplace = res
        self.root = RootView(res["d"], res["u"], mean, var, len(self.locs), self.topology, self.cov_locs, self.kernel)
        return res["lik"]

    def _fit_laplace_trend(self, family, aux, offset, z, e0, cov, max_iter, tol, X, reml):
        if cov is not None:
            spec = self._probe(cov)
            if spec is None:
                raise NotImplementedError("cov must be a device kernel")
            self._check_spec_metric(spec)
            self._send_kernel(spec)
        if self.trend is None or X is not self._X_arg:
            self._send_trend(X)
        if z is None:
            z = self.obs
        if e0 is None:
            e0 = getattr(self, "_laplace_e", None)
        self._node_blocks = {}
        res = self.plan.fit_laplace_trend(family, z, aux=aux, offset=offset, e0=e0, max_iter=max_iter, tol=tol)
        fit = self.plan.trend_fit(predict=True)          # the factors stand: one predict pass for the variance, one for W again
        t = self.topology
        tp = self.plan.buffer(11)
        good = np.asarray(t.perm) >= 0
        self._trend_y = np.zeros(len(self.locs))
        self._trend_y[np.asarray(t.perm)[good]] = np.nan_to_num(tp[good])
        self.trend = fit
        self._sd = np.sqrt(fit.var)
        self._laplace_e = fit.mean.copy() if res["converged"] else None      # (a fit that did not converge is no start for the next)
        self.laplace = res
        self.root = RootView(res["d"], res["u"], fit.mean, fit.var, len(self.locs), self.topology, self.cov_locs, self.kernel)
        return res["reml"] if reml else res["profile"]
