"""References and fixed inputs for mra_plan_fit_laplace.

``dense_laplace`` is the library's Newton iteration in dense algebra on the MRA prior covariance Sigma of the reported rows
(tests/_noise.prior_cov): the same linearisation, the same floor on D, the same stopping rule (a linearisation that is not finite
ends the fit, not converged), the same eight numbers.  ``terms`` is the float64 statement of g, D and log p, ``terms_mp`` the same
in 50 digits (mpmath), ``recompute_info`` the sums and maxima of a fit from the arrays the plan hands out.  The inputs of the GPU
tests are fixed here with seeded generators: a smooth latent field of amplitude 1, Poisson counts with exposures in [0.5, 20]
(entering as the offset log E), binomial counts out of 1..29 trials, a Gaussian family with a varying variance, and the four edge
cases of ``edge_inputs``."""
import functools
import math

import numpy as np
from scipy.linalg import cho_solve
from scipy.special import gammaln

GAUSSIAN, POISSON, BINOMIAL = 0, 1, 2
NAMES = {GAUSSIAN: "gaussian", POISSON: "poisson", BINOMIAL: "binomial"}
D_FLOOR = 2.0 ** -40
EPS = 2.0 ** -52


def terms_eta(family, z, aux, eta):
    """(g, D, the part of log p(z | eta) that depends on eta) per row in float64; D is floored.  Binomial: p and 1 - p each from its
    own logaddexp, so that neither cancels in the tails."""
    if family == POISSON:
        mu = np.exp(eta)
        g, D, lp = z - mu, mu, z * eta - mu
    elif family == BINOMIAL:
        p, q = np.exp(-np.logaddexp(0.0, -eta)), np.exp(-np.logaddexp(0.0, eta))
        g, D, lp = z - aux * p, aux * p * q, z * eta - aux * np.logaddexp(0.0, eta)
    else:
        g, D, lp = (z - eta) / aux, 1.0 / aux + 0.0 * eta, -0.5 * (z - eta) ** 2 / aux
    return g, np.maximum(D, D_FLOOR), lp


def const_terms(family, z, aux):
    """the terms of -2 log p(z | eta) that do not depend on eta, (rows x k): what the library sums on the host"""
    if family == POISSON:
        return np.stack([2.0 * gammaln(z + 1.0)], axis=-1)
    if family == BINOMIAL:
        return np.stack([-2.0 * gammaln(aux + 1.0), 2.0 * gammaln(z + 1.0), 2.0 * gammaln(aux - z + 1.0)], axis=-1)
    return np.stack([np.log(2.0 * np.pi * aux) + 0.0 * z], axis=-1)


def terms(family, z, aux, eta):
    """(g, D, log p(z | eta) with every normalising constant) per row; D is floored"""
    g, D, lp = terms_eta(family, z, aux, eta)
    return g, D, lp - 0.5 * const_terms(family, np.asarray(z, dtype=np.float64), np.asarray(aux, dtype=np.float64)).sum(axis=-1)


def terms_mp(family, z, aux, eta):
    """terms_eta in 50 digits: three object arrays of mpmath numbers (g, D floored, the eta-dependent part of log p), from the
    float64 inputs taken as exact"""
    import mpmath
    z, aux, eta = np.broadcast_arrays(np.asarray(z, dtype=np.float64), np.asarray(aux, dtype=np.float64), np.asarray(eta, dtype=np.float64))
    out = np.empty((3,) + z.shape, dtype=object)
    with mpmath.workdps(50):
        floor = mpmath.mpf(2) ** -40
        for i in np.ndindex(z.shape):
            zi, ai, ei = mpmath.mpf(float(z[i])), mpmath.mpf(float(aux[i])), mpmath.mpf(float(eta[i]))
            if family == POISSON:
                mu = mpmath.exp(ei)
                g, D, lp = zi - mu, mu, zi * ei - mu
            elif family == BINOMIAL:
                p, q = 1 / (1 + mpmath.exp(-ei)), 1 / (1 + mpmath.exp(ei))
                g, D, lp = zi - ai * p, ai * p * q, zi * ei - ai * mpmath.log1p(mpmath.exp(ei))
            else:
                g, D, lp = (zi - ei) / ai, 1 / ai, -(zi - ei) ** 2 / (2 * ai)
            out[(0,) + i], out[(1,) + i], out[(2,) + i] = g, max(D, floor), lp
    return out[0], out[1], out[2]


def err_mp(got, want, unit):
    """max |got - want| / unit in 50 digits (got: float64; want, unit: mpmath object arrays), as a float"""
    import mpmath
    with mpmath.workdps(50):
        worst = mpmath.mpf(0)
        for a, b, u in zip(np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=object).ravel(), np.asarray(unit, dtype=object).ravel()):
            worst = max(worst, abs(mpmath.mpf(float(a)) - b) / u)
        return float(worst)


def linearise_mp(family, z, aux, x):
    """one linearisation at x (offset 0) in 50 digits: (t, r, unit of t) as object arrays.  unit = |x| + (|z| + m) / D with m = e^eta
    (Poisson), aux p (binomial): the size of the terms that cancel in t = x + (z - m) / D.  The Gaussian family's t is z itself."""
    import mpmath
    g, D, _ = terms_mp(family, z, aux, x)
    z, aux, x = np.broadcast_arrays(np.asarray(z, dtype=np.float64), np.asarray(aux, dtype=np.float64), np.asarray(x, dtype=np.float64))
    t, r, unit = np.empty(z.shape, dtype=object), np.empty(z.shape, dtype=object), np.empty(z.shape, dtype=object)
    with mpmath.workdps(50):
        for i in np.ndindex(z.shape):
            zi, xi = mpmath.mpf(float(z[i])), mpmath.mpf(float(x[i]))
            r[i] = 1 / D[i]
            if family == GAUSSIAN:
                t[i], unit[i] = zi, abs(zi) + mpmath.mpf(2) ** -1000
            else:
                m = zi - g[i]                                          # e^eta, aux p
                t[i], unit[i] = xi + g[i] / D[i], abs(xi) + (abs(zi) + m) / D[i]
    return t, r, unit


def linearise(family, z, aux, offset, x):
    """(t, r) of one linearisation at x in float64, as the library's k_laplace_linearise states it"""
    g, D, _ = terms_eta(family, z, aux, x + offset)
    if family == GAUSSIAN:
        return z - offset + 0.0 * x, 1.0 / D
    return x + g / D, 1.0 / D


def eta_grid(n, outliers=True):
    """n values of eta for the tests of laplace_term: +-0, +-2^-60, the edge of the floor e^-|eta| = 2^-40 (|eta| = 27.7) from both
    sides, outliers to +-700 (where e^eta is near the largest double), and a dense band in [-40, 40] for the rest"""
    edge = 40.0 * math.log(2.0)
    head = [0.0, -0.0, 2.0 ** -60, -2.0 ** -60, 27.7, -27.7, edge, -edge, np.nextafter(edge, 100.0), -np.nextafter(edge, 100.0),
            np.nextafter(edge, 0.0), -np.nextafter(edge, 0.0), 40.0, -40.0]
    if outliers:
        head += [s * v for v in (50.0, 88.8, 100.0, 300.0, 600.0, 700.0) for s in (1.0, -1.0)]
    rng = np.random.RandomState(5)
    body = rng.uniform(-40.0, 40.0, size=n - len(head))
    return np.concatenate([head, body])[rng.permutation(n)]


KNOT_ETA_MAX = 30.0         # Poisson r = e^-eta at an upper node's knot stays above 9e-14 (see term_cases)


def term_cases(family, n, knots=()):
    """(z, aux, x) for the n rows of the laplace_term tests (offset 0, x = eta).  Poisson z by thirds: 0, 1, rint(min(e^eta, 2^52)) -
    z ~ mu, the cancelling case.  Binomial aux in {1, 29, 10^6}, z by thirds: 0, aux, rint(aux p).  Gaussian (no outliers): aux in
    {0.02, 1, 10^13} (the last beyond the floor), z by thirds: 0, eta, eta + 1.
    knots: positions among the n rows that are knots of a node above the leaves.  There the leaf's residual variance is 0 up to
    rounding (1e-16 of the prior variance), the pivot is that plus r, and a pass with r below the rounding is refused
    MRA_ERR_NOT_SPD.  A Poisson case with eta > KNOT_ETA_MAX at such a position changes places with a
    case of another position: the same cases, on rows where a pass can carry them."""
    x = eta_grid(n, outliers=family != GAUSSIAN)
    k = np.arange(n)
    if family == POISSON:
        aux = np.ones(n)
        z = np.where(k % 3 == 0, 0.0, np.where(k % 3 == 1, 1.0, np.rint(np.minimum(np.exp(x), 2.0 ** 52))))
    elif family == BINOMIAL:
        aux = np.array([1.0, 29.0, 1e6])[(k // 3) % 3]
        z = np.where(k % 3 == 0, 0.0, np.where(k % 3 == 1, aux, np.rint(aux * np.exp(-np.logaddexp(0.0, -x)))))
    else:
        aux = np.array([0.02, 1.0, 1e13])[(k // 3) % 3]
        z = np.where(k % 3 == 0, 0.0, np.where(k % 3 == 1, x, x + 1.0))
    if family == POISSON and len(knots):
        at_knot = np.zeros(n, dtype=bool)
        at_knot[list(knots)] = True
        move = np.nonzero(at_knot & (x > KNOT_ETA_MAX))[0]
        to = np.nonzero(~at_knot & (x <= KNOT_ETA_MAX))[0][:len(move)]
        for v in (z, aux, x):
            v[move], v[to] = v[to].copy(), v[move].copy()
        assert not np.any(x[at_knot] > KNOT_ETA_MAX)
    return z, aux, x


@functools.lru_cache(maxsize=None)
def term_errors(family, n, knots=()):
    """The laplace_term cases of a family with their 50-digit linearisation and the error of the float64 one against it:
    dict(z, aux, x, t (mp), r (mp), unit (mp), e_t, e_r, e_g, e_D, e_lp) - e_t in units of ``unit``, e_r and e_D relative, e_g in
    units of |z| + m, e_lp in units of |z eta| + |the other term|."""
    import mpmath
    z, aux, x = term_cases(family, n, knots)
    t, r, unit = linearise_mp(family, z, aux, x)
    t64, r64 = linearise(family, z, aux, 0.0, x)
    g, D, lp = terms_mp(family, z, aux, x)
    g64, D64, lp64 = terms_eta(family, z, aux, x)
    with mpmath.workdps(50):
        tiny = mpmath.mpf(2) ** -1000
        if family == GAUSSIAN:
            u_g = np.array([(abs(mpmath.mpf(float(a))) + abs(mpmath.mpf(float(b)))) / mpmath.mpf(float(c)) + tiny for a, b, c in zip(z, x, aux)], dtype=object)
            u_lp = np.array([abs(v) + tiny for v in lp], dtype=object)
        else:
            u_g = np.array([abs(mpmath.mpf(float(a))) + (mpmath.mpf(float(a)) - b) + tiny for a, b in zip(z, g)], dtype=object)
            u_lp = np.array([abs(mpmath.mpf(float(a)) * mpmath.mpf(float(e))) + abs(mpmath.mpf(float(a)) * mpmath.mpf(float(e)) - v) + tiny
                             for a, e, v in zip(z, x, lp)], dtype=object)
    return dict(z=z, aux=aux, x=x, t=t, r=r, unit=unit, e_t=err_mp(t64, t, unit), e_r=err_mp(r64, r, r),
                e_g=err_mp(g64, g, u_g), e_D=err_mp(D64, D, D), e_lp=err_mp(lp64, lp, u_lp))


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
        with np.errstate(over="ignore", invalid="ignore"):
            g, D, _ = terms(family, z, aux, x + offset)
            min_D = min(min_D, D.min())
            if family == GAUSSIAN:
                t, r = z - offset, 1.0 / D
            else:
                t, r = x + g / D, 1.0 / D
        if not (np.all(np.isfinite(t)) and np.all(np.isfinite(r))):
            # the iterate has left the doubles (e^eta = inf): the fit ends with this pass, not converged, and has no mean
            info[:5], info[5], info[6], info[7] = np.nan, it + 1, np.nan, 0.0
            nanN = np.full(N, np.nan)
            tN, rN, xN = nanN.copy(), np.zeros(N), nanN.copy()
            tN[o], rN[o], xN[o] = t, r, x
            return dict(info=info, lik=np.nan, mean=nanN, var=nanN, sd=nanN, t=tN, r=rN, a=None, xhat=None, D=D, logp=np.nan,
                        min_D=min_D, steps=steps + [np.nan], K_chol=None, o=o, x_keep=xN)
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
    tN, rN, xN = np.full(N, np.nan), np.zeros(N), np.full(N, np.nan)
    tN[o], rN[o], xN[o] = t, r, x
    return dict(info=info, lik=info[0] + info[1] + info[2] + info[3] - info[4], mean=mean, var=var, sd=np.sqrt(var), t=tN, r=rN, a=a,
                xhat=xh, D=D, logp=lp.sum(), min_D=min_D, steps=steps, K_chol=L, o=o, x_keep=xN)


def recompute_info(family, z, aux, offset, x_keep, mean, t, r, seen):
    """info[2], info[3], info[4], the step and max |x^| of a fit from arrays (N values each, read at ``seen``; aux, offset: None, a
    scalar or N values): x_keep the linearisation point of the last pass, mean its result, (t, r) what it conditioned on.  Sums by
    math.fsum (exactly rounded) of float64 terms: -2 x (the eta-dependent part of log p at eta^ = mean + offset, ``terms_eta``)
    and the constants of ``const_terms``; log D and D (t - x^)^2 with D = 1 / r.  S[k] = the sum of the absolute values of the
    terms of info[2 + k]: the scale of a summation error.  -> dict(info2, info3, info4, step, max_xhat, S)."""
    seen = np.asarray(seen, dtype=bool).ravel()
    n = len(seen)
    pick = lambda v, fill: (np.full(n, fill) if v is None else np.broadcast_to(np.asarray(v, dtype=np.float64).ravel(), (n,)))[seen]   # noqa: E731
    z, aux, offset = pick(z, np.nan), pick(aux, 1.0), pick(offset, 0.0)
    x_keep, xh, t, r = pick(x_keep, np.nan), pick(mean, np.nan), pick(t, np.nan), pick(r, np.nan)
    _, _, lp = terms_eta(family, z, aux, xh + offset)
    t2 = np.concatenate([-2.0 * lp, const_terms(family, z, aux).ravel()])
    D = 1.0 / r
    t3, t4 = np.log(D), D * (t - xh) * (t - xh)
    return dict(info2=math.fsum(t2), info3=math.fsum(t3), info4=math.fsum(t4), step=float(np.abs(xh - x_keep).max()),
                max_xhat=float(np.abs(xh).max()), S=(math.fsum(np.abs(t2)), math.fsum(np.abs(t3)), math.fsum(np.abs(t4))))


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
def t16_upper_knots():
    """positions, among T16's observed rows in caller order, of the rows that are knots of a node above the leaves (a tuple)"""
    topo, locs, obs, y, counts, Sigma, o = t16()
    n_upper = int(np.count_nonzero(~np.asarray(topo.node_leaf, dtype=bool)))
    knot = np.zeros(topo.N, dtype=bool)
    knot[topo.perm[np.asarray(topo.knot_rows)[:topo.knot_ptr[n_upper]]]] = True
    return tuple(int(i) for i in np.nonzero(knot[o])[0])


@functools.lru_cache(maxsize=None)
def t16_fit(family):
    """(z, aux, offset, dense_laplace from the data-based start) on T16"""
    topo, locs, obs, y, counts, Sigma, o = t16()
    z, aux, offset = inputs(locs, obs, family)
    return z, aux, offset, dense_laplace(Sigma, o, family, z, aux, offset)


# ---- the edges: the floor on D, saturated probabilities, counts in the thousands ----------------------------------------------------------
EDGES = ("tiny_exposure", "saturated", "gauss_floor", "big_counts")


@functools.lru_cache(maxsize=None)
def edge_inputs(name):
    """(family, z, aux, offset) on T16's mask, seeded.
    tiny_exposure: Poisson, exposure e^-30 where the first coordinate is below 0.25 (there D = e^eta is under the floor), 5 elsewhere;
    saturated:     binomial, 1..29 trials, all successes where the second coordinate is below 0.3, none above 0.7, p = 1/2 between;
    gauss_floor:   Gaussian, variance 1e13 (1 / aux under the floor) where the first coordinate is below 0.25, 0.02 elsewhere;
    big_counts:    Poisson, z ~ Poisson(2000 e^latent): Newton from x0 = 0 leaves the doubles in its second pass."""
    topo, locs, obs, y, counts, Sigma, o = t16()
    X = np.asarray(locs, dtype=np.float64)
    N = len(obs)
    x = latent(X)
    rng = np.random.RandomState(101 + EDGES.index(name))
    if name == "tiny_exposure":
        family, aux, offset = POISSON, None, np.where(X[:, 0] < 0.25, -30.0, np.log(5.0))
        z = rng.poisson(np.exp(x + offset)).astype(np.float64)
    elif name == "saturated":
        family, aux, offset = BINOMIAL, rng.randint(1, 30, size=N).astype(np.float64), None
        p = np.where(X[:, 1] < 0.3, 1.0, np.where(X[:, 1] > 0.7, 0.0, 0.5))
        z = rng.binomial(aux.astype(np.int64), p).astype(np.float64)
    elif name == "gauss_floor":
        family, aux = GAUSSIAN, np.where(X[:, 0] < 0.25, 1e13, 0.02)
        offset = 0.3 * np.cos(2 * np.pi * X[:, 0])
        z = x + offset + np.sqrt(aux) * rng.normal(size=N)
    elif name == "big_counts":
        family, aux, offset = POISSON, None, None
        z = rng.poisson(2000.0 * np.exp(x)).astype(np.float64)
    else:
        raise ValueError(name)
    return family, np.where(obs, z, np.nan), aux, offset


@functools.lru_cache(maxsize=None)
def edge_fit(name, zero_start=False, max_iter=50):
    """dense_laplace on an edge case from the data-based start (or from x0 = 0)"""
    topo, locs, obs, y, counts, Sigma, o = t16()
    family, z, aux, offset = edge_inputs(name)
    return dense_laplace(Sigma, o, family, z, aux, offset, x0=np.zeros(len(obs)) if zero_start else None, max_iter=max_iter)
