"""References for per-observation noise variances (mra_plan_set_noise).

``oracle/`` takes a scalar nugget.  A per-row-noise oracle of any size follows from it exactly, because the MRA construction is
equivariant under a diagonal rescaling of the process: with s(x) > 0 a function of the coordinates and r(x) = R s(x)^2, the problem
(C, y, diag r) is the problem (C', y', R I) with C'(a, b) = C(a, b) / (s(a) s(b)) and y' = y / s seen through x = s x'.  Knots, the
partition and every conditional independence assumption are the same on both sides, so

    u = u',   d = d' + sum over observed reported rows of log(r_i / R),   mean = s mean',   sd = s sd'.

``scaled_oracle`` hands run_levelwise the PLAIN callable C' (an object with ``.evaluate`` would take the oracle's stationary
shortcut for C(x, x)).  ``dense_reference`` is independent of that argument: the MRA prior covariance Sigma of the reported rows
(tests/_treecov.py), then dense algebra with Sigma[o, o] + diag(r_o).  ``ScaledSpec`` has ``.evaluate`` for the _tree* restatements,
which call the oracle with predict=False, where the shortcut is not taken into any result (tests/_treesites.tree_sites assumes a
stationary C(s, s): its variance cannot be used on the rescaled problem, its mean can)."""
import numpy as np


def s_of(X):
    """the scale s(x) in [1/2, 2]: 2 ** sin(2 pi x) in 1-D, 2 ** (sin(2 pi x0) cos(2 pi x1)) in 2-D"""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    if X.shape[1] == 1:
        return 2.0 ** np.sin(2 * np.pi * X[:, 0])
    return 2.0 ** (np.sin(2 * np.pi * X[:, 0]) * np.cos(2 * np.pi * X[:, 1]))


def noise_of(locs, R):
    """r(x) = R s(x)^2, in [R / 4, 4 R]"""
    return R * s_of(locs) ** 2


def scaled_cov(spec):
    """the plain callable C'(a, b) = C(a, b) / (s(a) s(b))"""
    def cov(a, b):
        return np.asarray(spec.evaluate(a, b), dtype=np.float64) / (s_of(a)[:, None] * s_of(b)[None, :])
    return cov


class ScaledSpec:
    """C' with ``.evaluate``, for tests/_treesolve.py, _treecov.py and _treesites.py"""

    def __init__(self, spec):
        self.spec = spec
        self._cov = scaled_cov(spec)

    def evaluate(self, a, b):
        return self._cov(a, b)


def reported(topo):
    """bool[N]: caller rows that some leaf reports"""
    rep = np.zeros(topo.N, dtype=bool)
    good = np.asarray(topo.in_leaf, dtype=bool) & (topo.perm >= 0)
    rep[topo.perm[good]] = True
    return rep


def scaled_oracle(topo, locs, spec, y, R, predict=True):
    """run_levelwise on the rescaled problem, mapped back: dict(lik, d, u, mean, var, sd) for the noise r = noise_of(locs, R)"""
    from oracle.mra_levelwise import run_levelwise
    s = s_of(locs)
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    o = run_levelwise(topo, locs, scaled_cov(spec), (yv / s).reshape(np.shape(y)), R, predict=predict)
    seen = np.isfinite(yv) & reported(topo)
    d = o["d"] + 2.0 * np.log(s[seen]).sum()
    return dict(lik=d + o["u"], d=d, u=o["u"], mean=s * o["mean"], var=s * s * o["var"], sd=s * o["sd"])


def prior_cov(topo, locs, spec, y):
    """Sigma (N x N, caller order): the MRA prior covariance of the reported rows, 0 elsewhere (it depends on neither y nor the noise)"""
    import _treecov
    assert topo.N <= 4096
    return _treecov.tree_cov(topo, locs, spec, y, 1.0, np.eye(topo.N))[0]


def dense_reference(topo, locs, spec, y, r, Sigma=None):
    """dense algebra on Sigma[o, o] + diag(r_o): dict(lik, d, u, mean, var, sd, Sigma, K_chol, o)"""
    from scipy.linalg import cho_solve
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), yv.shape)
    Sigma = prior_cov(topo, locs, spec, y) if Sigma is None else Sigma
    o = np.isfinite(yv) & reported(topo)
    K = Sigma[np.ix_(o, o)] + np.diag(r[o])
    L = np.linalg.cholesky(0.5 * (K + K.T))
    a = cho_solve((L, True), yv[o])
    d, u = 2.0 * np.log(np.diag(L)).sum(), float(yv[o] @ a)
    mean = Sigma[:, o] @ a
    T = np.linalg.solve(L, Sigma[o, :])
    var = np.maximum(np.diag(Sigma) - np.einsum("ij,ij->j", T, T), 0.0)
    return dict(lik=d + u, d=d, u=u, mean=mean, var=var, sd=np.sqrt(var), Sigma=Sigma, K_chol=L, o=o)
