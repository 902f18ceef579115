"""NumPy restatement of mra_solve: the retained factors of one likelihood pass - the prior W at every row,
each observed leaf's L_c and U = L_c^-1 W[o], each front's Lt and Zt - used as a sparse direct solver for c right-hand sides at
once.  Built on run_levelwise(..., predict=False, keep=True); the leaves' L_c and U are recomputed as leaf_node does.  It is the
reference the device kernels are debugged against: same steps, same orderings (ancestor blocks level m-1 ... 0, the y block
of Zt left out)."""
import numpy as np
from scipy.linalg import solve_triangular as st

from oracle.mra_levelwise import run_levelwise, YB


def tree_solve(topo, locs, spec, y_obs, R, Y):
    """Y: (N, c) in the caller's order, read where y_obs is finite.  -> (mean (N, c), Q (c, c)) with
    mean[:, k] = E[x | Y[o, k]] under the MRA and Q = Y_o^T (Sigma_MRA[o, o] + R I)^-1 Y_o."""
    y = np.asarray(y_obs, float).ravel()
    Y = np.asarray(Y, float).reshape(len(y), -1)
    c = Y.shape[1]
    k = run_levelwise(topo, locs, spec, y, R, predict=False, keep=True)
    W, Lt, Zt, lay = k["W"], k["Lt"], k["Zt"], k["layout"]
    Ka = lay.Ka
    X = np.asarray(locs, float).reshape(len(y), -1)[topo.src]
    obs_p = np.isfinite(y)[topo.src] & (topo.perm >= 0)
    Yp = Y[topo.src]
    nn = topo.n_nodes
    parent, level = np.asarray(topo.node_parent), np.asarray(topo.node_level)

    def kids(i):
        return [int(x) for x in topo.child_list[topo.child_ptr[i]:topo.child_ptr[i + 1]]]

    def covf(a, b):
        return np.asarray(spec.evaluate(a, b), float)

    Lc, Ua, Uy, obsi = {}, {}, {}, {}
    g, z = [None] * nn, [None] * nn
    Q = np.zeros((c, c))
    # 1. forward, leaves
    for i in range(nn):
        if not topo.node_leaf[i]:
            continue
        m = int(level[i])
        a0, na = int(lay.asuf[m]), int(lay.na[m])
        r0, r1 = int(topo.node_row0[i]), int(topo.node_row1[i])
        o = np.nonzero(obs_p[r0:r1])[0]
        obsi[i] = o
        Wa = W[r0:r1, a0:Ka]
        g[i] = np.zeros((na - YB, c))
        if len(o):
            Cm = covf(X[r0:r1][o], X[r0:r1][o]) - Wa[o] @ Wa[o].T + R * np.eye(len(o))
            Lc[i] = np.linalg.cholesky(.5 * (Cm + Cm.T))
            Ua[i] = st(Lc[i], Wa[o], lower=True)
            Uy[i] = st(Lc[i], Yp[r0:r1][o], lower=True)
            g[i] = Ua[i].T @ Uy[i]
            Q += Uy[i].T @ Uy[i]
    # 2. forward, fronts bottom-up; 3. the quadratic form
    for m in range(topo.n_levels - 1, -1, -1):
        cwm = int(lay.cw[m])
        for i in range(int(topo.level_ptr[m]), int(topo.level_ptr[m + 1])):
            if topo.node_leaf[i]:
                continue
            f = sum(g[ch] for ch in kids(i))
            z[i] = st(Lt[i], f[:cwm], lower=True)
            g[i] = f[cwm:] - Zt[i][:-YB] @ z[i]
            Q -= z[i].T @ z[i]
    # 4. backward, fronts top-down; 5. backward, leaves; 6. rows
    alpha, chain = [None] * nn, [None] * nn
    mean = np.zeros((topo.P, c))
    for m in range(topo.n_levels):
        for i in range(int(topo.level_ptr[m]), int(topo.level_ptr[m + 1])):
            p = int(parent[i])
            ch = np.zeros((0, c)) if p < 0 else np.vstack([alpha[p], chain[p]])      # ancestors: level m-1 first
            chain[i] = ch
            if not topo.node_leaf[i]:
                alpha[i] = st(Lt[i], z[i] - Zt[i][:-YB].T @ ch, lower=True, trans='T')
                continue
            a0 = int(lay.asuf[m])
            r0, r1 = int(topo.node_row0[i]), int(topo.node_row1[i])
            o = obsi[i]
            Wa = W[r0:r1, a0:Ka]
            beta = ch
            if len(o):
                s = Uy[i] - Ua[i] @ ch
                q = st(Lc[i], s, lower=True, trans='T')
                beta = ch - Ua[i].T @ s
                mean[r0:r1] = covf(X[r0:r1], X[r0:r1][o]) @ q
            mean[r0:r1] += Wa @ beta
    good = topo.in_leaf
    out = np.zeros((topo.N, c))
    out[topo.perm[good]] = mean[good]
    return out, Q
