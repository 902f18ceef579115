"""NumPy restatement of mra_cv_trend: tests/_treecv.tree_cv for the model y = X beta + x + eps with a flat prior
on beta, on top of tests/_treetrend.tree_trend - and the brute force it is checked against, which deletes the group and fits again.

Notation of _treecv.py, with K = Sigma[o, o] + D, A = X^T K^-1 X = L_A L_A^T, beta^ = A^-1 X^T K^-1 y, m_y / m_X the zero-mean kriging
means of y and of the columns of X (tree_trend's m), h_p = X_p - m_X(p), w_p = L_A^-1 h_p and rho~_p = y_p - m_y(p) - h_p^T beta^:

    refit  (beta estimated again without the group)    N~_G = N_G - W_G W_G^T:  mu_G = y_G - D_G N~_G^-1 rho~_G,  S_G = D_G N~_G^-1 D_G
    fixed  (the full fit's beta^ plugged in)           the same with the plain N_G

and tr K^-1 = sum (1 - v / r) / r, tr P = sum (1 - (v + |w|^2) / r) / r, |P y|^2 = sum (rho~ / r)^2 for P = K^-1 - K^-1 X A^-1 X^T K^-1.
Results are by PADDED row, as HipPlan.cv_trend returns them."""
import numpy as np
from scipy.linalg import solve_triangular as st

import _treecv as CV
import _treesitecov as TC
import _treesites as TS
import _treetrend as TT

LOG_2PI = CV.LOG_2PI

# The twin against the brute force (tests/test_cv_trend_cpu.py, where the measures are defined): the largest of the mean, variance, lpd
# and score errors per case over p = 1 and 3, both modes and both groupings, when the two were first compared; the device is held to
# max(1e-9, 100 x this) on the same case.
# g32_dense: dense_cv_trend against the twin on g32 with p = 3 (the rows' lpd by leaf), for the device's noise-vector results.
# grid48_r20 (tests/test_gpu_cov._shape_tree: leaves of 144 rows, groups of about 100) with design(coords=True), p = 3 and 17: all 16
# leaves and 40 seeded rows fitted again, the rows' marginal lpd by leaf included - mean 2.8e-10, variance 3.8e-10, lpd 1.1e-9 by leaf
# (3.4e-13, 3.2e-13, 1.3e-11 by row), at a largest leverage of 0.8117.
TWIN_ERR = {"g32": 3.3e-11, "c1": 5.2e-13, "kat3": 9.6e-13, "u3": 1.5e-11, "g32_dense": 8.9e-11, "grid48_r20": 1.1e-9}


def design(locs, p, seed=3, coords=False):
    """(N, p) covariates for the tests: an intercept, with coords=True the coordinates, then seeded standard normal columns.
    (On the four cases of tests/test_cv_trend_cpu.py the coordinates as columns 2 and 3 lift the largest (v + |w|^2) / r to 0.97215 on
    g32 and 0.97285 on u3, past the 0.972 its bound is measured under; two normal columns of this seed give 0.97196 and 0.96971.)"""
    L = np.asarray(locs, float).reshape(len(locs), -1)
    cols = [np.ones(len(L))] + ([L[:, k] for k in range(L.shape[1])] if coords else [])
    Z = np.random.default_rng(seed).standard_normal((len(L), max(p - len(cols), 0)))
    return np.column_stack(cols + [Z])[:, :p]


def tree_cv_trend(S, X, leaf, refit, locs=None, fit=None):
    """S: a tests/_treesites.SiteState (scalar R).  X: (N, p) in the caller's order.  leaf as tree_cv; refit: beta estimated again without
    the group, else the full fit's beta^ held fixed.  fit: tree_trend's result for (S, X) when the caller has it (else locs is needed).
    -> (mean, var, lpd (P each, NaN where nothing is scored), group_lpd (n_nodes), info[12])"""
    topo, r = S.topo, S.R
    X = np.asarray(X, float).reshape(len(S.y), -1)
    if fit is None:
        fit = TT.tree_trend(topo, locs, S.spec, S.y, r, X)
    p, lf = CV.scored_rows(S)
    c = topo.perm[p]
    sites = S.X[p]
    y = S.y[c]
    m, v = TS.tree_sites(topo, None, S.spec, None, r, sites, lf, state=S)
    Li = np.linalg.inv(np.linalg.cholesky(np.linalg.inv(fit["cov_beta"])))      # L_A^-1 (cov_beta = A^-1)
    h = X[c] - fit["m"][c, 1:]
    W = h @ Li.T
    w2 = (W * W).sum(1)
    rho = y - m[:, 0] - h @ fit["beta"]
    hv, ht = v / r, (v + w2) / r
    lev = ht if refit else hv
    mean, var, lpd = (np.full(topo.P, np.nan) for _ in range(3))
    group = np.full(topo.n_nodes, np.nan)
    if not leaf:
        mean[p], var[p] = y - rho / (1.0 - lev), r / (1.0 - lev)
        n_groups = len(p)
    else:
        n_groups = 0
        for i in np.unique(lf):
            g = np.nonzero(lf == i)[0]
            N = r * np.eye(len(g)) - TC.tree_sites_cov(S, sites[g], lf[g], posterior=True)
            if refit:
                N = N - W[g] @ W[g].T
            L = np.linalg.cholesky(.5 * (N + N.T))
            w = st(L, rho[g], lower=True)
            Linv = st(L, np.eye(len(g)), lower=True)
            mean[p[g]] = y[g] - r * st(L, w, lower=True, trans='T')
            var[p[g]] = r * r * np.einsum("ij,ij->j", Linv, Linv)
            group[i] = -.5 * (2.0 * len(g) * np.log(r) - 2.0 * np.log(np.diag(L)).sum() + w @ w + len(g) * LOG_2PI)
            n_groups += 1
    lpd[p] = -.5 * (LOG_2PI + np.log(var[p]) + (y - mean[p]) ** 2 / var[p])
    if not leaf:
        for i in np.unique(lf):
            group[i] = lpd[p[lf == i]].sum()
    trK, trP, py2 = ((1.0 - hv) / r).sum(), ((1.0 - ht) / r).sum(), ((rho / r) ** 2).sum()
    info = np.array([len(p), n_groups, np.nansum(group) if leaf else lpd[p].sum(), lpd[p].sum(), ((y - mean[p]) ** 2 / var[p]).sum(),
                     lev.max() if len(p) else 0.0, trK, py2, trP, X.shape[1], trK - py2, trP - py2])
    return mean, var, lpd, group, info


def ntilde(S, X, node, refit, locs=None, fit=None):
    """N_G (refit: N~_G = N_G - W_G W_G^T) of the leaf `node`, as tree_cv_trend forms it before the Cholesky"""
    topo, r = S.topo, S.R
    X = np.asarray(X, float).reshape(len(S.y), -1)
    if fit is None:
        fit = TT.tree_trend(topo, locs, S.spec, S.y, r, X)
    p, lf = CV.scored_rows(S)
    g = np.nonzero(lf == node)[0]
    N = r * np.eye(len(g)) - TC.tree_sites_cov(S, S.X[p[g]], lf[g], posterior=True)
    if refit:
        Li = np.linalg.inv(np.linalg.cholesky(np.linalg.inv(fit["cov_beta"])))
        c = topo.perm[p[g]]
        W = (X[c] - fit["m"][c, 1:]) @ Li.T
        N = N - W @ W.T
    return .5 * (N + N.T)


def _gls(K, Xo, yo):
    L = np.linalg.cholesky(.5 * (K + K.T))
    KX, Ky = st(L, Xo, lower=True), st(L, yo, lower=True)
    A = KX.T @ KX
    beta = np.linalg.solve(A, KX.T @ Ky)
    return L, A, beta


def brute_group_trend(Sigma, S, X, rows, beta_fixed=None):
    """The independent check.  Sigma: the MRA prior covariance over the padded rows (tests/_sampling.golden_prior_sigma); rows: the
    padded rows of one group.  The group is deleted, GLS is fitted on the rest against Sigma[o, o] + D and the group is kriged
    universally; beta_fixed: instead that beta is plugged in (simple kriging of y - X beta around X beta).
    -> (mu_G, S_G (noise included), log N(y_G; mu_G, S_G))"""
    topo, r = S.topo, S.R
    X = np.asarray(X, float).reshape(len(S.y), -1)
    p, _ = CV.scored_rows(S)
    rows = np.asarray(rows)
    o = np.setdiff1d(p, rows)
    K = Sigma[np.ix_(o, o)] + r * np.eye(len(o))
    Xo, yo, Xg, yg = X[topo.perm[o]], S.y[topo.perm[o]], X[topo.perm[rows]], S.y[topo.perm[rows]]
    L, A, beta = _gls(K, Xo, yo)
    c = st(L, Sigma[np.ix_(o, rows)], lower=True)              # L^-1 Sigma[o, G]
    Sg = Sigma[np.ix_(rows, rows)] - c.T @ c + r * np.eye(len(rows))
    if beta_fixed is None:
        hg = Xg - c.T @ st(L, Xo, lower=True)
        Sg = Sg + hg @ np.linalg.solve(A, hg.T)
    else:
        beta = np.asarray(beta_fixed, float)
    mu = Xg @ beta + c.T @ st(L, yo - Xo @ beta, lower=True)
    e = yg - mu
    Ls = np.linalg.cholesky(.5 * (Sg + Sg.T))
    w = st(Ls, e, lower=True)
    return mu, Sg, -.5 * (2.0 * np.log(np.diag(Ls)).sum() + w @ w + len(rows) * LOG_2PI)


def dense_fit(Sigma, S, X, r_add=0.0):
    """The dense fit on all the scored rows with the noise R + r_add: dict(beta, Ki, P, y, profile, reml) - K^-1 and
    P = K^-1 - K^-1 X A^-1 X^T K^-1 dense, the profile and REML -2 log-likelihoods"""
    topo = S.topo
    X = np.asarray(X, float).reshape(len(S.y), -1)
    p, _ = CV.scored_rows(S)
    K = Sigma[np.ix_(p, p)] + (S.R + r_add) * np.eye(len(p))
    Xo, yo = X[topo.perm[p]], S.y[topo.perm[p]]
    L, A, beta = _gls(K, Xo, yo)
    Li = st(L, np.eye(len(p)), lower=True)
    Ki = Li.T @ Li
    KX = Ki @ Xo
    P = Ki - KX @ np.linalg.solve(A, KX.T)
    prof = 2.0 * np.log(np.diag(L)).sum() + float(yo @ P @ yo)
    return dict(beta=beta, Ki=Ki, P=P, y=yo, profile=prof, reml=prof + np.linalg.slogdet(A)[1])


def dense_cv_trend(topo, Sigma, y, r, X, leaf, refit):
    """The same quantities with D = diag(r) from dense algebra on K = Sigma[o, o] + D alone (tests/_treecv.dense_cv with P for K^-1 under
    refit, and with y - X beta^ for y otherwise): what the device's noise-vector results are held to.  Sigma: (N x N) in the caller's
    order (tests/_noise.prior_cov); y, r: N values, X: (N, p), in the caller's order.  -> as tree_cv_trend."""
    yv = np.asarray(y, float).ravel()
    X = np.asarray(X, float).reshape(len(yv), -1)
    r = np.broadcast_to(np.asarray(r, float), yv.shape)
    lor = CV.leaf_of_rows(topo)
    p = np.nonzero((topo.perm >= 0) & (lor >= 0))[0]
    p = p[np.isfinite(yv[topo.perm[p]])]
    c, lf = topo.perm[p], lor[p]
    K = Sigma[np.ix_(c, c)] + np.diag(r[c])
    Ki = np.linalg.inv(.5 * (K + K.T))
    Ki = .5 * (Ki + Ki.T)
    KX = Ki @ X[c]
    A = X[c].T @ KX
    Pm = Ki - KX @ np.linalg.solve(A, KX.T)
    Pm = .5 * (Pm + Pm.T)
    Py = Pm @ yv[c]
    Q = Pm if refit else Ki
    mean, var, lpd = (np.full(topo.P, np.nan) for _ in range(3))
    group = np.full(topo.n_nodes, np.nan)
    leaves = list(np.unique(lf))
    groups = [np.nonzero(lf == i)[0] for i in leaves] if leaf else [np.array([k]) for k in range(len(p))]
    joint = np.zeros(len(groups))
    for n, g in enumerate(groups):
        Sg = np.linalg.inv(Q[np.ix_(g, g)])
        Sg = .5 * (Sg + Sg.T)
        mean[p[g]], var[p[g]] = yv[c[g]] - Sg @ Py[g], np.diag(Sg)
        e = yv[c[g]] - mean[p[g]]
        joint[n] = -.5 * (np.linalg.slogdet(Sg)[1] + e @ np.linalg.solve(Sg, e) + len(g) * LOG_2PI)
    lpd[p] = -.5 * (LOG_2PI + np.log(var[p]) + (yv[c] - mean[p]) ** 2 / var[p])
    for i in leaves:
        group[i] = joint[leaves.index(i)] if leaf else lpd[p[lf == i]].sum()
    lev = 1.0 - r[c] * np.diag(Q)
    trK, trP, py2 = np.trace(Ki), np.trace(Pm), Py @ Py
    info = np.array([len(p), len(groups), joint.sum() if leaf else lpd[p].sum(), lpd[p].sum(), ((yv[c] - mean[p]) ** 2 / var[p]).sum(),
                     lev.max() if len(p) else 0.0, trK, py2, trP, X.shape[1], trK - py2, trP - py2])
    return mean, var, lpd, group, info
