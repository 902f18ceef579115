"""References and fixed inputs for mra_plan_fit_laplace.

``dense_laplace`` is the library's Newton iteration in dense algebra on the MRA prior covariance Sigma of the reported rows
(tests/_noise.prior_cov): the same linearisation, the same floor on D, the same stopping rule, the same eight numbers.  The inputs of
the GPU tests are fixed here with seeded generators: a smooth latent field of amplitude 1, Poisson counts with exposures in
[0.5, 20] (entering as the offset log E), binomial counts out of 1..29 trials, and a Gaussian family with a varying variance."""
import functools

import numpy as np
from scipy.linalg import cho_solve
from scipy.special import gammaln

GAUSSIAN, POISSON, BINOMIAL = 0, 1, 2
NAMES = {GAUSSIAN: "gaussian", POISSON: "poisson", BINOMIAL: "binomial"}
D_FLOOR = 2.0 ** -40


def terms(family, z, aux, eta):
    """(g, D, log p(z | eta) with every normalising constant) per row; D is floored"""
    if family == POISSON:
        mu = np.exp(eta)
        g, D, lp = z - mu, mu, z * eta - mu - gammaln(z + 1.0)
    elif family == BINOMIAL:
        p = 1.0 / (1.0 + np.exp(-eta))
        g, D = z - aux * p, aux * p * (1.0 - p)
        lp = z * eta - aux * np.logaddexp(0.0, eta) + gammaln(aux + 1.0) - gammaln(z + 1.0) - gammaln(aux - z + 1.0)
    else:
        g, D, lp = (z - eta) / aux, 1.0 / aux + 0.0 * eta, -0.5 * (z - eta) ** 2 / aux - 0.5 * np.log(2.0 * np.pi * aux)
    return g, np.maximum(D, D_FLOOR), lp


def start(family, z, aux, offset):
    """the data-based start of the table in include/mra_hip.h"""
    if family == POISSON:
        return np.log(z + 0.5) - offset
    if family == BINOMIAL:
        return np.log((z + 0.5) / (aux - z + 0.5)) - offset
    return z - offset


def dense_laplace(Sigma, o, family, z, aux=None, offset=None, x0=None, max_iter=50, tol=1e-10):
    """The iteration of mra_plan_fit_laplace on Sigma (N x N, caller order) and the observed rows o (bool[N]).  z, aux, offset, x0:
    N values, read at o.  -> dict(info[8], lik, mean[N], var[N], sd[N], t, r (N values, NaN / 0 off o), a, min_D, steps)."""
    N = Sigma.shape[0]
    z = np.asarray(z, dtype=np.float64).reshape(-1)[o]
    full = lambda v, fill: np.full(N, fill) if v is None else np.broadcast_to(np.asarray(v, dtype=np.float64), (N,))      # noqa: E731
    aux, offset = full(aux, 1.0)[o], full(offset, 0.0)[o]
    x = start(family, z, aux, offset) if x0 is None else np.asarray(x0, dtype=np.float64).reshape(-1)[o]
    Soo = Sigma[np.ix_(o, o)]
    info = np.zeros(8)
    min_D, steps = np.inf, []
    for it in range(max_iter):
        g, D, _ = terms(family, z, aux, x + offset)
        min_D = min(min_D, D.min())
        if family == GAUSSIAN:
            t, r = z - offset, 1.0 / D
        else:
            t, r = x + g / D, 1.0 / D
        K = Soo + np.diag(r)
        L = np.linalg.cholesky(0.5 * (K + K.T))
        a = cho_solve((L, True), t)
        xh = Soo @ a
        step = np.abs(xh - x).max()
        steps.append(step)
        info[5], info[6] = it + 1, step
        if step <= tol * max(1.0, np.abs(xh).max()):
            info[7] = 1.0
            break
        x = xh
    _, _, lp = terms(family, z, aux, xh + offset)
    info[0], info[1] = 2.0 * np.log(np.diag(L)).sum(), float(t @ a)
    info[2], info[3], info[4] = -2.0 * lp.sum(), np.log(D).sum(), float((D * (t - xh) ** 2).sum())
    mean = Sigma[:, o] @ a
    T = np.linalg.solve(L, Sigma[o, :])
    var = np.maximum(np.diag(Sigma) - np.einsum("ij,ij->j", T, T), 0.0)
    tN, rN = np.full(N, np.nan), np.zeros(N)
    tN[o], rN[o] = t, r
    return dict(info=info, lik=info[0] + info[1] + info[2] + info[3] - info[4], mean=mean, var=var, sd=np.sqrt(var), t=tN, r=rN, a=a,
                xhat=xh, D=D, logp=lp.sum(), min_D=min_D, steps=steps, K_chol=L, o=o)


def direct_neg2logq(Sigma, res, family):
    """-2 [log p(z | x^) - a^T Sigma_oo a / 2 - log|I + D^1/2 Sigma_oo D^1/2| / 2] from a dense_laplace result"""
    o, a, D = res["o"], res["a"], res["D"]
    Soo = Sigma[np.ix_(o, o)]
    s = np.sqrt(D)
    _, logdet = np.linalg.slogdet(np.eye(len(a)) + s[:, None] * Soo * s[None, :])
    return -2.0 * (res["logp"] - 0.5 * float(a @ Soo @ a) - 0.5 * logdet)


# ---- fixed inputs -----------------------------------------------------------------------------------------------------------------
def latent(locs):
    """a smooth function of the coordinates with amplitude 1"""
    X = np.asarray(locs, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    if X.shape[1] == 1:
        return np.sin(2 * np.pi * X[:, 0])
    return np.sin(2 * np.pi * X[:, 0]) * np.cos(2 * np.pi * X[:, 1])


def inputs(locs, obs, family, seed=11):
    """(z[N] with NaN off ``obs``, aux[N] or None, offset[N] or None) for a family"""
    rng = np.random.RandomState(seed + family)
    N = len(obs)
    x = latent(locs)
    if family == POISSON:
        E = np.exp(rng.uniform(np.log(0.5), np.log(20.0), size=N))
        z, aux, offset = rng.poisson(E * np.exp(x)).astype(np.float64), None, np.log(E)
    elif family == BINOMIAL:
        aux = rng.randint(1, 30, size=N).astype(np.float64)
        z, offset = rng.binomial(aux.astype(np.int64), 1.0 / (1.0 + np.exp(-x))).astype(np.float64), None
    else:
        aux = 0.02 * 4.0 ** rng.uniform(-1.0, 1.0, size=N)
        offset = 0.3 * np.cos(2 * np.pi * np.asarray(locs, dtype=np.float64).reshape(N, -1)[:, 0])
        z = x + offset + np.sqrt(aux) * rng.normal(size=N)
    return np.where(obs, z, np.nan), aux, offset


@functools.lru_cache(maxsize=None)
def t16():
    """(topo, locs, obs mask, y (N x 1, the mask as set_obs takes it), leaf counts, Sigma, o) of tree T16 with mask CLOUD"""
    import _noise as NZ
    import _route_cells as RC
    import test_gpu_likelihood_masks as MK
    topo, locs = MK._tree(*RC.TREES["T16"])
    obs = RC.make_obs(topo, locs, RC.CLOUD)
    y = MK._y(obs)
    Sigma = NZ.prior_cov(topo, locs, MK._spec(), y)
    return topo, locs, obs, y, MK.leaf_counts(topo, obs), Sigma, obs & NZ.reported(topo)


@functools.lru_cache(maxsize=None)
def t16_fit(family):
    """(z, aux, offset, dense_laplace from the data-based start) on T16"""
    topo, locs, obs, y, counts, Sigma, o = t16()
    z, aux, offset = inputs(locs, obs, family)
    return z, aux, offset, dense_laplace(Sigma, o, family, z, aux, offset)
