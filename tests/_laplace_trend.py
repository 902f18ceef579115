"""The reference and the fixed inputs for mra_plan_fit_laplace_trend.

``dense_laplace_trend`` is the library's iteration in dense algebra on the MRA prior covariance Sigma of the reported rows
(tests/_noise.prior_cov): eta = X beta + x + offset, the linearisation, the floor on D and the stopping rule of
tests/_laplace.dense_laplace, and per pass K = Sigma_oo + diag r, generalised least squares for beta and
e^ = X_o beta^ + Sigma_oo K^-1 (t - X_o beta^).  It returns the twelve numbers of the call.  The inputs are seeded: the design is an
intercept and p - 1 columns of 0.25 N(0, 1), the data have eta = latent + X beta_true with the exposures (Poisson) and trials
(binomial) of tests/_laplace.inputs; the Gaussian family uses tests/_laplace.inputs unchanged."""
import functools

import numpy as np
from scipy.linalg import cho_factor, cho_solve, solve_triangular

import _laplace as LP


def design(N, p):
    X = 0.25 * np.random.default_rng(3).standard_normal((N, p))
    X[:, 0] = 1.0
    return X


def beta_true(p):
    b = np.linspace(0.5, -0.5, p)
    b[0] = 0.4
    return b


def inputs(locs, obs, family, p, seed=11):
    """(z[N] with NaN off ``obs``, aux[N] or None, offset[N] or None, X[N, p]); the generators draw the exposures and the trials
    first, as tests/_laplace.inputs does, so these are the same"""
    N = len(obs)
    X = design(N, p)
    if family == LP.GAUSSIAN:
        return LP.inputs(locs, obs, family, seed) + (X,)
    rng = np.random.RandomState(seed + family)
    eta = LP.latent(locs) + X @ beta_true(p)
    if family == LP.POISSON:
        E = np.exp(rng.uniform(np.log(0.5), np.log(20.0), size=N))
        z, aux, offset = rng.poisson(E * np.exp(eta)).astype(np.float64), None, np.log(E)
    else:
        aux = rng.randint(1, 30, size=N).astype(np.float64)
        z, offset = rng.binomial(aux.astype(np.int64), 1.0 / (1.0 + np.exp(-eta))).astype(np.float64), None
    return np.where(obs, z, np.nan), aux, offset, X


def dense_laplace_trend(Sigma, o, family, z, aux, offset, X, e0=None, max_iter=50, tol=1e-10):
    """The iteration of mra_plan_fit_laplace_trend on Sigma (N x N, caller order) and the observed rows o (bool[N]).  z, aux, offset,
    e0: N values read at o; X: (N, p).  -> dict(info[12], beta, cov_beta, mean[N], var[N], sd[N] (of e = X beta + x, the uncertainty
    of beta included), t, r (N values, NaN / 0 off o), a = K^-1 (t - X beta^), xhat, ehat, e_keep, D, logp, steps, maxe, A)."""
    N = Sigma.shape[0]
    X = np.asarray(X, dtype=np.float64)
    p = X.shape[1]
    z = np.asarray(z, dtype=np.float64).reshape(-1)[o]
    full = lambda v, fill: np.full(N, fill) if v is None else np.broadcast_to(np.asarray(v, dtype=np.float64), (N,))      # noqa: E731
    aux, offset = full(aux, 1.0)[o], full(offset, 0.0)[o]
    e = LP.start(family, z, aux, offset) if e0 is None else np.asarray(e0, dtype=np.float64).reshape(-1)[o]
    Soo, Xo = Sigma[np.ix_(o, o)], X[o]
    info = np.zeros(12)
    info[11] = len(z)
    steps, maxe = [], []

    def spread(v, fill):
        out = np.full(N, fill)
        out[o] = v
        return out

    for it in range(max_iter):
        with np.errstate(over="ignore", invalid="ignore"):
            g, D, _ = LP.terms(family, z, aux, e + offset)
            if family == LP.GAUSSIAN:
                t, r = z - offset, 1.0 / D
            else:
                t, r = e + g / D, 1.0 / D
        if not (np.all(np.isfinite(t)) and np.all(np.isfinite(r))):
            # the iterate has left the doubles: the fit ends with this pass, not converged
            info[:5], info[5], info[6], info[7], info[8:11] = np.nan, it + 1, np.nan, 0.0, np.nan
            nanN = np.full(N, np.nan)
            return dict(info=info, beta=np.full(p, np.nan), cov_beta=None, mean=nanN, var=nanN, sd=nanN, t=spread(t, np.nan), r=spread(r, 0.0),
                        a=None, xhat=None, ehat=None, e_keep=spread(e, np.nan), D=D, logp=np.nan, steps=steps + [np.nan], maxe=maxe, A=None, o=o)
        K = Soo + np.diag(r)
        L = np.linalg.cholesky(0.5 * (K + K.T))
        wt, wX = solve_triangular(L, t, lower=True), solve_triangular(L, Xo, lower=True)
        A, b = wX.T @ wX, wX.T @ wt
        cA = cho_factor(A)
        beta = cho_solve(cA, b)
        a = solve_triangular(L.T, wt - wX @ beta, lower=False)
        xh = Soo @ a
        eh = Xo @ beta + xh
        step = np.abs(eh - e).max()
        steps.append(step); maxe.append(np.abs(eh).max())
        info[5], info[6] = it + 1, step
        e_keep = e
        if step <= tol * max(1.0, np.abs(eh).max()):
            info[7] = 1.0
            break
        e = eh
    _, _, lp = LP.terms(family, z, aux, eh + offset)
    info[0], info[1] = 2.0 * np.log(np.diag(L)).sum(), float(wt @ wt - b @ beta)
    info[2], info[3], info[4] = -2.0 * lp.sum(), np.log(D).sum(), float((D * (t - eh) ** 2).sum())
    info[8] = 2.0 * np.log(np.diag(cA[0])).sum()
    info[9] = info[0] + info[1] + info[2] + info[3] - info[4]
    info[10] = info[9] + info[8] - p * np.log(2.0 * np.pi)
    cov_beta = cho_solve(cA, np.eye(p))
    T = solve_triangular(L, Sigma[o, :], lower=True)
    h = X - T.T @ wX
    mean = X @ beta + Sigma[:, o] @ a
    var = np.maximum(np.diag(Sigma) - np.einsum("ij,ij->j", T, T), 0.0) + np.einsum("ij,jk,ik->i", h, cov_beta, h)
    return dict(info=info, beta=beta, cov_beta=cov_beta, mean=mean, var=var, sd=np.sqrt(var), t=spread(t, np.nan), r=spread(r, 0.0), a=a,
                xhat=xh, ehat=eh, e_keep=spread(e_keep, np.nan), D=D, logp=lp.sum(), steps=steps, maxe=maxe, A=A, o=o)


def passes_are_pinned(ref, tol=1e-10):
    """True when each of the twin's last two steps lies at least a factor 2 from its threshold tol * max(1, max |e^|): rounding on
    the device cannot then move the pass at which the iteration stops"""
    out = True
    for s, m in list(zip(ref["steps"], ref["maxe"]))[-2:]:
        thr = tol * max(1.0, m)
        out = out and (s <= 0.5 * thr or s >= 2.0 * thr)
    return out


@functools.lru_cache(maxsize=None)
def t16_fit(family, p):
    """(z, aux, offset, X, dense_laplace_trend from the data-based start) on T16"""
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, X = inputs(locs, obs, family, p)
    return z, aux, offset, X, dense_laplace_trend(Sigma, o, family, z, aux, offset, X)
