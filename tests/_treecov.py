"""NumPy restatement of mra_cov_apply: the MRA prior covariance of the reported rows,
    Sigma = sum over non-leaf j of W_j W_j^T + sum over leaves l of v_M(K_l, K_l),   v_M(S, S) = C(S, S) - W_anc[S] W_anc[S]^T,
applied to c vectors at once from the whitened basis W of run_levelwise(..., keep=True), and the posterior
Sigma_post A = Sigma A - mean_MRA((Sigma A)_o) through tests/_treesolve.py.  Written from the topology in the six steps of the device
kernels, with their orderings (ancestor blocks level m-1 ... 0, children summed in child-list order): it is the reference the
kernels are debugged against."""
import numpy as np

from oracle.mra_levelwise import run_levelwise

import _treesolve as TS


def masks(topo):
    """(rep, knot) over the padded rows: reported rows (real rows inside a leaf); knot rows of the row's own leaf."""
    rep = (topo.perm >= 0) & np.asarray(topo.in_leaf, dtype=bool)
    knot = np.zeros(topo.P, dtype=bool)
    for i in range(topo.n_nodes):
        if topo.node_leaf[i]:
            knot[topo.knot_rows[topo.knot_ptr[i]:topo.knot_ptr[i + 1]]] = True
    return rep, knot


def tree_cov_padded(topo, locs, spec, y_obs, R, Ap):
    """Ap: (P, c) in padded leaf order, read at the reported rows -> Sigma Ap (P, c), unreported rows 0."""
    y = np.asarray(y_obs, float).ravel()
    k = run_levelwise(topo, locs, spec, y, R, predict=False, keep=True)
    W, lay = k["W"], k["layout"]
    Ka = lay.Ka
    X = np.asarray(locs, float).reshape(len(y), -1)[topo.src]
    rep, knot = masks(topo)
    c = Ap.shape[1]
    Abar = np.where(rep[:, None], Ap, 0.0)
    Ach = np.where((rep & knot)[:, None], Ap, 0.0)
    nn = topo.n_nodes
    parent, level = np.asarray(topo.node_parent), np.asarray(topo.node_level)

    def kids(i):
        return [int(x) for x in topo.child_list[topo.child_ptr[i]:topo.child_ptr[i + 1]]]

    def covf(a, b):
        return np.asarray(spec.evaluate(a, b), float)

    # 1. leaves: t = W[S, anc]^T Abar[S], t' = W[S, anc]^T Acheck[S]
    up, tp = [None] * nn, [None] * nn
    for i in range(nn):
        if not topo.node_leaf[i]:
            continue
        a0 = int(lay.asuf[int(level[i])])
        r0, r1 = int(topo.node_row0[i]), int(topo.node_row1[i])
        Wa = np.where(rep[r0:r1, None], W[r0:r1, a0:Ka], 0.0)
        up[i] = Wa.T @ Abar[r0:r1]
        tp[i] = Wa.T @ Ach[r0:r1]
    # 2. fronts, bottom-up: the children's chain buffers summed; the node keeps its own cw block tau_j and passes the rest up
    tau = [None] * nn
    for m in range(topo.n_levels - 1, -1, -1):
        cwm = int(lay.cw[m])
        for i in range(int(topo.level_ptr[m]), int(topo.level_ptr[m + 1])):
            if topo.node_leaf[i]:
                continue
            f = np.zeros((cwm + Ka - int(lay.asuf[m]), c))
            for ch in kids(i):
                f = f + up[ch]
            tau[i], up[i] = f[:cwm], f[cwm:]
    # 3. fronts, top-down: [tau_j ; tau_chain]; 4. rows
    full = [None] * nn
    out = np.zeros((topo.P, c))
    for m in range(topo.n_levels):
        for i in range(int(topo.level_ptr[m]), int(topo.level_ptr[m + 1])):
            p = int(parent[i])
            chain = np.zeros((0, c)) if p < 0 else full[p]           # ancestors: level m-1 first
            if not topo.node_leaf[i]:
                full[i] = np.vstack([tau[i], chain])
                continue
            a0 = int(lay.asuf[m])
            r0, r1 = int(topo.node_row0[i]), int(topo.node_row1[i])
            Wa = W[r0:r1, a0:Ka]
            kk = (rep & knot)[r0:r1]
            leaf = covf(X[r0:r1], X[r0:r1][kk]) @ Ach[r0:r1][kk] - Wa @ tp[i]
            out[r0:r1] = Wa @ chain + np.where(kk[:, None], leaf, 0.0)
    out[~rep] = 0.0
    return out


def tree_cov(topo, locs, spec, y_obs, R, A, posterior=False):
    """A: (N, c) in the caller's order, read at the reported rows.  -> (out (N, c), gram (c, c)): out = Sigma A (posterior: Sigma_post A),
    rows outside every leaf 0; gram = A_rep^T out."""
    y = np.asarray(y_obs, float).ravel()
    A = np.asarray(A, float).reshape(len(y), -1)
    rep, _ = masks(topo)
    Ap = np.zeros((topo.P, A.shape[1]))
    Ap[rep] = A[topo.perm[rep]]
    op = tree_cov_padded(topo, locs, spec, y, R, Ap)
    out = np.zeros(A.shape)
    out[topo.perm[rep]] = op[rep]
    if posterior:
        # 5. the second term is one solve on the block that is already there, read at the observed rows
        mean, _ = TS.tree_solve(topo, locs, spec, y, R, np.where(np.isfinite(y)[:, None], out, np.nan))
        out = out - mean
    Arep = np.zeros(A.shape)
    Arep[topo.perm[rep]] = A[topo.perm[rep]]
    return out, Arep.T @ out
