"""NumPy restatement of mra_sites_cov: the joint prior or posterior covariance of the latent MRA process at
locations that are not rows of the tree.  Built on tests/_treesites.SiteState: per leaf the three arrays the site kernels leave behind -
a(s) (step 1), t(s) (step 2) and b, which after step 3 holds the chain vectors p_j(s) in place - and then, per pair of leaves, one
product over the trailing rows of both arrays: W's columns run deepest block first and end at Ka for every leaf, so the blocks of the
common ancestors of two leaves are the rows from the lowest common ancestor's own block to the end.

    prior      Sigma(u, w)      = C(s_u, s_w) inside a leaf, else sum_{k in tail} a_k(u) a_k(w)
    posterior  Sigma_post(u, w) = sum_{k in tail} p_k(u) p_k(w) + [same leaf] (C(s_u, s_w) - a(u) . a(w) - t(u) . t(w))

Nothing is clamped."""
import numpy as np
from scipy.linalg import solve_triangular as st

from oracle.mra_levelwise import YB


def leaf_arrays(S, i, sites):
    """(a, t, p) of the sites (n, d) assigned to leaf node i: (anc, n), (n_obs, n), (anc, n) - tree_sites' steps 1 to 3, unclamped"""
    topo, lay = S.topo, S.lay
    a0 = int(lay.asuf[int(S.level[i])])
    r0, r1 = int(topo.node_row0[i]), int(topo.node_row1[i])
    a = S.basis(i, sites)
    o = S.obsi[i]
    t, b = np.zeros((0, len(sites))), a.copy()
    if len(o):
        t = st(S.Lc[i], S.cov(S.X[r0:r1][o], sites), lower=True) - S.Ua[i] @ a
        b = a - S.Ua[i].T @ t
    for j in S.chain(i)[::-1]:
        k = int(S.level[j])
        c0, up, cw = int(lay.coff[k]) - a0, int(lay.asuf[k]) - a0, int(lay.cw[k])
        b[c0:c0 + cw] = st(S.Lt[j], b[c0:c0 + cw], lower=True)
        b[up:] -= S.Zt[j][:-YB] @ b[c0:c0 + cw]
    return a, t, b


def common_tail(S, i, k):
    """number of trailing rows two leaves' arrays share: from the own block of their lowest common ancestor to Ka (0: none)"""
    ci, ck = S.chain(i), S.chain(k)
    n = 0
    while n < min(len(ci), len(ck)) and ci[n] == ck[n]:
        n += 1
    return 0 if n == 0 else int(S.lay.Ka) - int(S.lay.coff[int(S.level[ci[n - 1]])])


def tree_sites_cov(state, sites, leaf, posterior):
    """sites (n, d) assigned to the leaf NODES leaf (n,) -> (n, n) covariance of the latent field at the sites"""
    S = state
    leaf = np.asarray(leaf)
    sites = np.asarray(sites, float).reshape(len(leaf), -1)
    n = len(leaf)
    out = np.zeros((n, n))
    leaves = [int(i) for i in np.unique(leaf)]
    who = {i: np.nonzero(leaf == i)[0] for i in leaves}
    arr = {i: leaf_arrays(S, i, sites[who[i]]) for i in leaves}
    for x, i in enumerate(leaves):
        a, t, p = arr[i]
        Css = S.cov(sites[who[i]], sites[who[i]])
        blk = (p.T @ p - a.T @ a - t.T @ t + Css) if posterior else Css
        out[np.ix_(who[i], who[i])] = .5 * (blk + blk.T)
        for k in leaves[x + 1:]:
            w = common_tail(S, i, k)
            xi, xk = (p, arr[k][2]) if posterior else (a, arr[k][0])
            blk = xi[xi.shape[0] - w:].T @ xk[xk.shape[0] - w:] if w else np.zeros((len(who[i]), len(who[k])))
            out[np.ix_(who[i], who[k])] = blk
            out[np.ix_(who[k], who[i])] = blk.T
    return out
