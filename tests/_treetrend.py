"""NumPy restatement of mra_trend_fit on tests/_treesolve.tree_solve: the columns [y | X] go through the
restated solver once, G = [y | X]^T K^-1 [y | X] is its dense Q, and the rest is the algebra of the header:
    beta = A^-1 b, cov(beta) = A^-1, profile = d + G_yy - b^T beta, reml = profile + log det A,
    mean = m_y + h beta, var = var_pass + h A^-1 h^T with h = X - m_X at the rows the tree reports (0 elsewhere).
d and var_pass come from the level-wise oracle's pass on y.  Same steps as the device call, nothing of its code."""
import numpy as np

import _treesolve as TS
from oracle.mra_levelwise import run_levelwise


def tree_trend(topo, locs, spec, y_obs, R, X, scaled_noise=False):
    """X: (N, p) in the caller's order.  -> dict(G, beta, cov_beta, d, u, logdetA, profile, reml, mean, var, add, var_pass, m).
    scaled_noise: the noise vector r = R s(x)^2 of tests/_noise.py instead of the scalar R, through its rescaling (the problem
    (C, [y | X], diag r) is (C', [y | X] / s, R I): G is the same matrix, the kriging means come back times s)."""
    y = np.asarray(y_obs, float).ravel()
    X = np.asarray(X, float).reshape(len(y), -1)
    p = X.shape[1]
    YX = np.column_stack([np.nan_to_num(y), X])
    if scaled_noise:
        import _noise as NZ
        s = NZ.s_of(locs)
        m, G = TS.tree_solve(topo, locs, NZ.ScaledSpec(spec), y / s, R, YX / s[:, None])
        m = m * s[:, None]
        own = NZ.scaled_oracle(topo, locs, spec, y_obs, R)
    else:
        m, G = TS.tree_solve(topo, locs, spec, y_obs, R, YX)
        own = run_levelwise(topo, locs, spec, y_obs, R)
    A, b = G[1:, 1:], G[1:, 0]
    L = np.linalg.cholesky(A)
    Li = np.linalg.inv(L)
    cov_beta = Li.T @ Li
    beta = cov_beta @ b
    d = float(own["d"])
    u = float(G[0, 0] - b @ beta)
    logdet = 2.0 * float(np.log(np.diag(L)).sum())
    rep = np.zeros(len(y), bool)
    rep[topo.perm[(topo.perm >= 0) & np.asarray(topo.in_leaf, bool)]] = True
    h = np.where(rep[:, None], X - m[:, 1:], 0.0)
    add = ((h @ Li.T) ** 2).sum(1)
    mean = np.where(rep, m[:, 0] + h @ beta, 0.0)
    var_pass = np.where(rep, np.asarray(own["var"], float).ravel(), 0.0)
    return dict(G=G, beta=beta, cov_beta=cov_beta, d=d, u=u, logdetA=logdet, profile=d + u, reml=d + u + logdet, mean=mean,
                var=var_pass + add, add=add, var_pass=var_pass, m=m, p=p)
