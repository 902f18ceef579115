"""NumPy restatement of mra_sample_sites: the factor F of the joint covariance of the latent MRA process at
locations that are not rows of the tree, x = [mean +] F z.  Built on tests/_treesitecov.leaf_arrays: per leaf the arrays a, t and p
of its sites, then

    coarse columns  F[u, slots of ancestor j] = a_j(u) (prior) or p_j(u) (posterior) for every ancestor j of the site's leaf
    leaf columns    F[S_l, Kn + S_l] = L_l,  L_l L_l^T = G_l = C(S_l, S_l) - a^T a [- t^T t]  (numpy.linalg.cholesky)

Latent slots: [0, Kn) the non-leaf nodes in node order, cw[level] each (mra_sample's numbering); [Kn, Kn + n) the leaf term of site u
by the caller's index.  Exact duplicates (same leaf, equal coordinates) are collapsed to their first occurrence: their rows of F are
copies of its rows and their own leaf columns are 0.  A site with G_uu <= 2^-40 C(s, s) is inert: its row and column of G_l become
the identity before the Cholesky and its leaf column is 0."""
import numpy as np

import _treesitecov as TC

INERT_REL = 2.0 ** -40


def coarse_slots(state):
    """(zoff per node (-1: leaf), Kn)"""
    S = state
    topo = S.topo
    zoff, kn = np.full(topo.n_nodes, -1, dtype=np.int64), 0
    for i in range(topo.n_nodes):
        if not topo.node_leaf[i]:
            zoff[i] = kn
            kn += int(S.lay.cw[int(S.level[i])])
    return zoff, kn


def site_draw_factor(state, sites, leaf, posterior, info=None):
    """sites (n, d) assigned to the leaf NODES leaf (n,) -> (F (n, Kn + n), slot_of_column (Kn + n,)): slot_of_column[c] is the latent
    slot column c of F multiplies (the identity here: columns are in slot order).  info (a dict, optional) receives `inert` (bool[n]),
    `first` (int[n], the first occurrence of each site) and `min_pivot` (the smallest Cholesky pivot relative to C(s, s))."""
    S = state
    leaf = np.asarray(leaf)
    sites = np.asarray(sites, float).reshape(len(leaf), -1)
    n = len(leaf)
    zoff, Kn = coarse_slots(S)
    F = np.zeros((n, Kn + n))
    first, seen = np.arange(n), {}
    for u in range(n):
        first[u] = seen.setdefault((int(leaf[u]), tuple(float(v) + 0.0 for v in sites[u])), u)
    inert = np.zeros(n, dtype=bool)
    min_pivot = np.inf
    lay = S.lay
    for i in [int(v) for v in np.unique(leaf)]:
        who = np.nonzero((leaf == i) & (first == np.arange(n)))[0]          # distinct sites of the leaf, the caller's order
        a, t, p = TC.leaf_arrays(S, i, sites[who])
        a0 = int(lay.asuf[int(S.level[i])])
        X = p if posterior else a
        for j in S.chain(i):
            k = int(S.level[j])
            c0, cw = int(lay.coff[k]) - a0, int(lay.cw[k])
            F[np.ix_(who, np.arange(zoff[j], zoff[j] + cw))] = X[c0:c0 + cw].T
        Css = S.cov(sites[who], sites[who])
        G = Css - a.T @ a - (t.T @ t if posterior else 0.0)
        G = .5 * (G + G.T)
        c = np.diag(Css)
        dead = np.diag(G) <= INERT_REL * c
        inert[who] = dead
        G[dead, :] = 0.0
        G[:, dead] = 0.0
        G[dead, dead] = 1.0
        L = np.linalg.cholesky(G)                                         # raises LinAlgError when a leaf block does not factor
        live = ~dead
        if live.any():
            min_pivot = min(min_pivot, float((np.diag(L)[live] ** 2 / c[live]).min()))
        L[dead, dead] = 0.0
        F[np.ix_(who, Kn + who)] = L
    dup = first != np.arange(n)
    F[dup] = F[first[dup]]
    inert[dup] = inert[first[dup]]
    if info is not None:
        info.update(inert=inert, first=first, min_pivot=min_pivot, Kn=Kn)
    return F, np.arange(Kn + n)
