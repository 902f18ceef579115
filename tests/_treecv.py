"""NumPy restatement of mra_cv: the leave-group-out predictive distributions of a fitted tree from the state one
likelihood pass leaves behind, without a refit - and the brute force they are checked against, which refits.

With o the observed rows, D = R I the noise, m and Sigma_post the posterior mean and covariance of the latent field given all the data
and rho = y - m at the observed rows: for a group G of observed rows and N_G = D_G - Sigma_post[G, G] = L L^T

    mu_G = y_G - D_G N_G^-1 rho_G        S_G = D_G N_G^-1 D_G (noise included)
    log N(y_G; mu_G, S_G) = -1/2 [2 sum log r_p - log det N_G + |L^-1 rho_G|^2 + |G| log 2 pi]

m and the posterior variance come from tests/_treesites.tree_sites with the observed rows as sites, Sigma_post[G, G] inside a leaf from
tests/_treesitecov.tree_sites_cov(..., posterior=True).  Results are by PADDED row, as HipPlan.cv returns them."""
import numpy as np
from scipy.linalg import solve_triangular as st

import _treesites as TS
import _treesitecov as TC
from oracle.mra_levelwise import run_levelwise

LOG_2PI = float(np.log(2.0 * np.pi))

# The twin against the brute force (tests/test_cv_cpu.py, where the measures are defined), the largest of the mean, variance, lpd and
# score errors per case, by row or by leaf, when the two were first compared; the device is held to max(1e-9, 100 x this) on the same case.
# grid48_r20 (tests/test_gpu_cov._shape_tree: leaves of 144 rows, groups of about 100): all 16 leaves and 40 seeded rows refitted, the
# rows' marginal lpd by leaf included - mean 2.0e-10, variance 3.4e-10, lpd 8.8e-10 by leaf (1.7e-13, 3.1e-13, 4.5e-12 by row).
TWIN_ERR = {"g32": 3.3e-11, "c1": 2.3e-13, "kat3": 9.6e-13, "u3": 1.4e-11, "grid48_r20": 8.8e-10}


def leaf_of_rows(topo):
    """[P] leaf node of a padded row (-1 outside every leaf)"""
    out = np.full(topo.P, -1, dtype=np.int32)
    for i in np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]:
        out[int(topo.node_row0[i]):int(topo.node_row1[i])] = i
    return out


def scored_rows(S):
    """(padded rows, their leaf nodes) of the observations a cross-validation scores: observed and inside a leaf, in row order"""
    lor = leaf_of_rows(S.topo)
    p = np.nonzero(S.obs_p & (lor >= 0))[0]
    return p, lor[p]


def tree_cv(S, leaf):
    """S: a tests/_treesites.SiteState.  leaf: False - every observed row its own group; True - the observed rows of each leaf.
    -> (mean, var, lpd (P each, NaN where nothing is scored), group_lpd (n_nodes, NaN off the observed leaves), info[8])"""
    topo, r = S.topo, S.R
    p, lf = scored_rows(S)
    sites = S.X[p]
    y = S.y[topo.perm[p]]
    m, v = TS.tree_sites(topo, None, S.spec, None, r, sites, lf, state=S)
    rho, h = y - m[:, 0], v / r
    mean, var, lpd = (np.full(topo.P, np.nan) for _ in range(3))
    group = np.full(topo.n_nodes, np.nan)
    if not leaf:
        mean[p], var[p] = y - rho / (1.0 - h), r / (1.0 - h)
        n_groups = len(p)
    else:
        n_groups = 0
        for i in np.unique(lf):
            g = np.nonzero(lf == i)[0]
            N = r * np.eye(len(g)) - TC.tree_sites_cov(S, sites[g], lf[g], posterior=True)
            L = np.linalg.cholesky(.5 * (N + N.T))
            w = st(L, rho[g], lower=True)
            Li = st(L, np.eye(len(g)), lower=True)
            mean[p[g]] = y[g] - r * st(L, w, lower=True, trans='T')
            var[p[g]] = r * r * np.einsum("ij,ij->j", Li, Li)
            group[i] = -.5 * (2.0 * len(g) * np.log(r) - 2.0 * np.log(np.diag(L)).sum() + w @ w + len(g) * LOG_2PI)
            n_groups += 1
    lpd[p] = -.5 * (LOG_2PI + np.log(var[p]) + (y - mean[p]) ** 2 / var[p])
    if not leaf:
        for i in np.unique(lf):
            group[i] = lpd[p[lf == i]].sum()
    info = np.array([len(p), n_groups, np.nansum(group) if leaf else lpd[p].sum(), lpd[p].sum(), ((y - mean[p]) ** 2 / var[p]).sum(),
                     h.max() if len(p) else 0.0, ((1.0 - h) / r).sum(), ((rho / r) ** 2).sum()])
    return mean, var, lpd, group, info


def brute_group(cs, R, rows):
    """The refit: the observations at the padded rows `rows` (one group) set to NaN, the level-wise oracle run again on the same
    topology.  -> (mu_G from the refit's mean, S_G = the refit's posterior covariance block at those rows + R I, the block from
    tree_sites_cov on the refit's state (for one row: the oracle's own variance), log N(y_G; mu_G, S_G))"""
    topo, locs, spec = cs["topo"], cs["locs"], cs["spec"]
    y = np.asarray(cs["y_obs"], float).ravel()
    rows = np.asarray(rows)
    y2 = y.copy()
    y2[topo.perm[rows]] = np.nan
    ref = run_levelwise(topo, locs, spec, y2, R)
    mu = np.asarray(ref["mean"], float).ravel()[topo.perm[rows]]
    if len(rows) == 1:
        Sg = np.array([[float(np.asarray(ref["var"]).ravel()[topo.perm[rows[0]]]) + R]])
    else:
        S2 = TS.SiteState(topo, locs, spec, y2, R)
        Sg = TC.tree_sites_cov(S2, S2.X[rows], leaf_of_rows(topo)[rows], posterior=True) + R * np.eye(len(rows))
    e = y[topo.perm[rows]] - mu
    L = np.linalg.cholesky(.5 * (Sg + Sg.T))
    w = st(L, e, lower=True)
    return mu, Sg, -.5 * (2.0 * np.log(np.diag(L)).sum() + w @ w + len(rows) * LOG_2PI)


def dense_kinv_sums(S, prior_sigma):
    """(tr K^-1, alpha^T alpha) from the dense K = Sigma[o, o] + R I, Sigma the (P x P) MRA prior covariance by padded row"""
    p, _ = scored_rows(S)
    K = prior_sigma[np.ix_(p, p)] + S.R * np.eye(len(p))
    Ki = np.linalg.inv(.5 * (K + K.T))
    al = Ki @ S.y[S.topo.perm[p]]
    return float(np.trace(Ki)), float(al @ al)


def dense_cv(topo, Sigma, y, r, leaf):
    """The same quantities with D = diag(r) from dense algebra on K = Sigma[o, o] + D alone: S_G = (K^-1[G, G])^-1 and
    mu_G = y_G - S_G (K^-1 y)_G, the textbook form of the identities above (no r - v is formed).  Sigma: the (N x N) MRA prior
    covariance in the caller's order (tests/_noise.prior_cov); y, r: N values in the caller's order.  -> as tree_cv."""
    yv = np.asarray(y, float).ravel()
    r = np.broadcast_to(np.asarray(r, float), yv.shape)
    lor = leaf_of_rows(topo)
    p = np.nonzero((topo.perm >= 0) & (lor >= 0))[0]
    p = p[np.isfinite(yv[topo.perm[p]])]
    c, lf = topo.perm[p], lor[p]
    K = Sigma[np.ix_(c, c)] + np.diag(r[c])
    Ki = np.linalg.inv(.5 * (K + K.T))
    Ki = .5 * (Ki + Ki.T)
    al = Ki @ yv[c]
    mean, var, lpd = (np.full(topo.P, np.nan) for _ in range(3))
    group = np.full(topo.n_nodes, np.nan)
    groups = [np.nonzero(lf == i)[0] for i in np.unique(lf)] if leaf else [np.array([k]) for k in range(len(p))]
    joint = np.zeros(len(groups))
    for n, g in enumerate(groups):
        Sg = np.linalg.inv(Ki[np.ix_(g, g)])
        Sg = .5 * (Sg + Sg.T)
        mean[p[g]], var[p[g]] = yv[c[g]] - Sg @ al[g], np.diag(Sg)
        e = yv[c[g]] - mean[p[g]]
        joint[n] = -.5 * (np.linalg.slogdet(Sg)[1] + e @ np.linalg.solve(Sg, e) + len(g) * LOG_2PI)
    lpd[p] = -.5 * (LOG_2PI + np.log(var[p]) + (yv[c] - mean[p]) ** 2 / var[p])
    for i in np.unique(lf):
        group[i] = joint[list(np.unique(lf)).index(i)] if leaf else lpd[p[lf == i]].sum()
    h = 1.0 - r[c] * np.diag(Ki)
    info = np.array([len(p), len(groups), joint.sum() if leaf else lpd[p].sum(), lpd[p].sum(), ((yv[c] - mean[p]) ** 2 / var[p]).sum(),
                     h.max() if len(p) else 0.0, np.trace(Ki), al @ al])
    return mean, var, lpd, group, info
