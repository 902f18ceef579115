"""NumPy restatement of mra_predict_sites: the posterior mean and variance of the MRA process at locations that
are not rows of the tree, from the state one likelihood pass leaves behind - the prior W and factors L_j, each observed leaf's L_c
and U = L_c^-1 W[o], each front's Lt and Zt.  Built on run_levelwise(..., predict=False, keep=True) as tests/_treesolve.py is; the
leaves' L_c and U are recomputed as leaf_node does.  Same four steps and orderings as the device kernels (ancestor blocks level
m-1 ... 0, the y block of Zt left out); the prior covariance rows of a site are restated next to them, for the dense truths of
tests/test_sites_cpu.py."""
import numpy as np
from scipy.linalg import solve_triangular as st

from oracle.mra_levelwise import run_levelwise, YB


class SiteState:
    """What the four steps read, computed once per (tree, kernel, mask, R)."""

    def __init__(self, topo, locs, spec, y_obs, R):
        y = np.asarray(y_obs, float).ravel()
        self.topo, self.spec, self.R, self.y = topo, spec, float(R), y
        k = run_levelwise(topo, locs, spec, y, R, predict=False, keep=True)
        self.W, self.Lp, self.Lt, self.Zt, self.lay = k["W"], k["Lp"], k["Lt"], k["Zt"], k["layout"]
        self.X = np.asarray(locs, float).reshape(len(y), -1)[topo.src]
        self.obs_p = np.isfinite(y)[topo.src] & (topo.perm >= 0)
        self.level = np.asarray(topo.node_level)
        self.parent = np.asarray(topo.node_parent)
        self.Lc, self.Ua, self.obsi = {}, {}, {}
        Ka = self.lay.Ka
        for i in range(topo.n_nodes):
            if not topo.node_leaf[i]:
                continue
            a0 = int(self.lay.asuf[int(self.level[i])])
            r0, r1 = int(topo.node_row0[i]), int(topo.node_row1[i])
            o = np.nonzero(self.obs_p[r0:r1])[0]
            self.obsi[i] = o
            if len(o):
                Wa = self.W[r0:r1, a0:Ka]
                Cm = self.cov(self.X[r0:r1][o], self.X[r0:r1][o]) - Wa[o] @ Wa[o].T + self.R * np.eye(len(o))
                self.Lc[i] = np.linalg.cholesky(.5 * (Cm + Cm.T))
                self.Ua[i] = st(self.Lc[i], Wa[o], lower=True)

    def cov(self, a, b):
        return np.asarray(self.spec.evaluate(a, b), float)

    def chain(self, i):
        """ancestors of node i, root first"""
        up, p = [], int(self.parent[i])
        while p >= 0:
            up.append(p)
            p = int(self.parent[p])
        return up[::-1]

    def knots(self, j):
        t = self.topo
        return np.asarray(t.knot_rows[t.knot_ptr[j]:t.knot_ptr[j + 1]], dtype=np.int64)

    def basis(self, i, S):
        """step 1: a (anc, n) for sites S (n, d) of leaf i, in W's column order relative to the leaf's first ancestor column"""
        lay, Ka = self.lay, self.lay.Ka
        a0 = int(lay.asuf[int(self.level[i])])
        a = np.zeros((Ka - a0, len(S)))
        for j in self.chain(i):
            k = int(self.level[j])
            c0, up = int(lay.coff[k]) - a0, int(lay.asuf[k]) - a0
            kq = self.knots(j)
            res = self.cov(self.X[kq], S) - self.W[kq, int(lay.asuf[k]):Ka] @ a[up:]
            a[c0:c0 + len(kq)] = st(self.Lp[j][:len(kq), :len(kq)], res, lower=True)      # phantom knot columns stay 0
        return a

    def beta_q(self, Y):
        """the solver's sweeps (tests/_treesolve.py, steps 1, 2, 4, 5) for Y (N, c): {leaf: (beta (anc, c), q (n_o, c) or None)}"""
        t, lay = self.topo, self.lay
        Yp = Y[t.src]
        c = Y.shape[1]
        nn = t.n_nodes
        g, z, Uy = [None] * nn, [None] * nn, {}
        for i in range(nn):
            if not t.node_leaf[i]:
                continue
            m = int(self.level[i])
            r0, r1 = int(t.node_row0[i]), int(t.node_row1[i])
            g[i] = np.zeros((int(lay.na[m]) - YB, c))
            if len(self.obsi[i]):
                Uy[i] = st(self.Lc[i], Yp[r0:r1][self.obsi[i]], lower=True)
                g[i] = self.Ua[i].T @ Uy[i]
        for m in range(t.n_levels - 1, -1, -1):
            cwm = int(lay.cw[m])
            for i in range(int(t.level_ptr[m]), int(t.level_ptr[m + 1])):
                if t.node_leaf[i]:
                    continue
                f = sum(g[int(ch)] for ch in t.child_list[t.child_ptr[i]:t.child_ptr[i + 1]])
                z[i] = st(self.Lt[i], f[:cwm], lower=True)
                g[i] = f[cwm:] - self.Zt[i][:-YB] @ z[i]
        alpha, chain, out = [None] * nn, [None] * nn, {}
        for m in range(t.n_levels):
            for i in range(int(t.level_ptr[m]), int(t.level_ptr[m + 1])):
                p = int(self.parent[i])
                ch = np.zeros((0, c)) if p < 0 else np.vstack([alpha[p], chain[p]])
                chain[i] = ch
                if not t.node_leaf[i]:
                    alpha[i] = st(self.Lt[i], z[i] - self.Zt[i][:-YB].T @ ch, lower=True, trans='T')
                    continue
                if len(self.obsi[i]):
                    s = Uy[i] - self.Ua[i] @ ch
                    out[i] = (ch - self.Ua[i].T @ s, st(self.Lc[i], s, lower=True, trans='T'))
                else:
                    out[i] = (ch, None)
        return out


def tree_sites(topo, locs, spec, y_obs, R, sites, leaf, Y=None, state=None):
    """sites (n, d) assigned to the leaf NODES leaf (n,); Y: (N, c) in the caller's order, read where y_obs is finite (None: y_obs
    itself, c = 1).  -> (mean (n, c), var (n,)): the posterior mean and the variance of the latent field at the sites."""
    S = state if state is not None else SiteState(topo, locs, spec, y_obs, R)
    sites = np.asarray(sites, float).reshape(len(leaf), -1)
    leaf = np.asarray(leaf)
    Y = S.y.reshape(-1, 1) if Y is None else np.asarray(Y, float).reshape(len(S.y), -1)
    bq = S.beta_q(np.where(np.isfinite(S.y)[:, None], Y, 0.0))
    lay = S.lay
    mean, var = np.zeros((len(leaf), Y.shape[1])), np.zeros(len(leaf))
    c_ss = float(S.cov(sites[:1], sites[:1])[0, 0]) if len(sites) else 0.0      # a KernelSpec is stationary
    for i in np.unique(leaf):
        i = int(i)
        assert topo.node_leaf[i]
        who = np.nonzero(leaf == i)[0]
        a0 = int(lay.asuf[int(S.level[i])])
        r0, r1 = int(topo.node_row0[i]), int(topo.node_row1[i])
        a = S.basis(i, sites[who])                                                   # 1. basis
        o = S.obsi[i]
        b, v = a.copy(), c_ss - np.einsum("ij,ij->j", a, a)
        beta, q = bq[i]
        mu = a.T @ beta
        if len(o):                                                                   # 2. leaf
            Cso = S.cov(S.X[r0:r1][o], sites[who])
            tt = st(S.Lc[i], Cso, lower=True) - S.Ua[i] @ a
            b = a - S.Ua[i].T @ tt
            v = v - np.einsum("ij,ij->j", tt, tt)
            mu = mu + Cso.T @ q                                                      # 4. mean
        v = np.maximum(v, 0.0)
        for j in S.chain(i)[::-1]:                                                   # 3. chain, parent up to root
            k = int(S.level[j])
            c0, up, cw = int(lay.coff[k]) - a0, int(lay.asuf[k]) - a0, int(lay.cw[k])
            p = st(S.Lt[j], b[c0:c0 + cw], lower=True)
            b[up:] -= S.Zt[j][:-YB] @ p
            v = v + np.einsum("ij,ij->j", p, p)
        mean[who], var[who] = mu, v
    return mean, var


def site_prior_cov(state, sites, leaf):
    """(C_sr (n, P), C_ss (n, n)): the MRA prior covariance of the sites with every padded row (0 at unreported rows) and with each
    other - sum over the shared ancestors of a_j(s) . W_j[row] (a_j(s) . a_j(s')), plus v_M = C - a . W_anc inside a common leaf."""
    S, topo, lay = state, state.topo, state.lay
    Ka = lay.Ka
    sites = np.asarray(sites, float).reshape(len(leaf), -1)
    leaf = np.asarray(leaf)
    rep = (topo.perm >= 0) & np.asarray(topo.in_leaf, dtype=bool)
    n = len(leaf)
    Csr, Css = np.zeros((n, topo.P)), np.zeros((n, n))
    blocks = [None] * n                                  # per site: {ancestor node: its block of a}
    for i in np.unique(leaf):
        i = int(i)
        who = np.nonzero(leaf == i)[0]
        a0 = int(lay.asuf[int(S.level[i])])
        r0, r1 = int(topo.node_row0[i]), int(topo.node_row1[i])
        a = S.basis(i, sites[who])
        for j in S.chain(i):
            k = int(S.level[j])
            c0, cw = int(lay.coff[k]), int(lay.cw[k])
            j0, j1 = int(topo.node_row0[j]), int(topo.node_row1[j])
            Csr[who, j0:j1] += (S.W[j0:j1, c0:c0 + cw] @ a[c0 - a0:c0 - a0 + cw]).T
        Csr[who, r0:r1] += (S.cov(S.X[r0:r1], sites[who]) - S.W[r0:r1, a0:Ka] @ a).T
        for n_, w in enumerate(who):
            blocks[w] = {j: a[int(lay.coff[int(S.level[j])]) - a0:int(lay.asuf[int(S.level[j])]) - a0, n_] for j in S.chain(i)}
    Csr[:, ~rep] = 0.0
    for u in range(n):
        for w in range(u, n):
            if leaf[u] == leaf[w]:
                val = float(S.cov(sites[u:u + 1], sites[w:w + 1])[0, 0])
            else:
                val = sum(float(blocks[u][j] @ blocks[w][j]) for j in blocks[u] if j in blocks[w])
            Css[u, w] = Css[w, u] = val
    return Csr, Css
