"""Universal kriging: a regression trend fitted with the field, on one tree.

Model: y = X beta + x + eps, a flat prior on beta, x the MRA field, eps ~ N(0, R).  `MRATree(..., X=X)` sends the covariates to the
device once; every fit - the constructor's, and each `reevaluate(cov)` of a search over kernel parameters - is then a few sweeps
over the factors of one likelihood pass: beta and its covariance by generalised least squares, the profile likelihood (or REML) to
maximise, and with predictions the universal-kriging mean and a standard deviation that carries the uncertainty of beta.
`examples/gls_trend.py` does the first step by hand from `solve()`; this is the whole of it.

    python examples/universal_kriging.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymra_amd.MRATools as mt          # noqa: E402
from pymra_amd import MRATree            # noqa: E402


def main(n=128, frac=0.4, R=1e-2, l_true=0.2, seed=4):
    rng = np.random.default_rng(seed)
    np.random.seed(seed)
    locs = mt.genLocations2d(Nx=n, Ny=n)
    N = n * n
    elevation = np.sin(3.0 * locs[:, 0]) * np.cos(2.0 * locs[:, 1]) + 0.3 * rng.standard_normal(N)
    X = np.column_stack([np.ones(N), locs[:, 1], elevation])          # intercept, latitude, elevation
    beta_true = np.array([2.0, -1.5, 0.75])
    w = rng.normal(size=(64, 2)) / l_true                              # a smooth field: random Fourier features, dense-free
    field = np.sqrt(2.0 / 64) * np.cos(locs @ w.T + rng.uniform(0, 2 * np.pi, 64)).sum(axis=1)
    y = X @ beta_true + field + np.sqrt(R) * rng.standard_normal(N)
    obs = rng.random(N) < frac
    y_obs = np.where(obs, y, np.nan).reshape(-1, 1)

    cov = lambda l: (lambda a, b=np.array([]): mt.Matern32(a, b, l=l, sig=1.0))          # noqa: E731
    tree = MRATree(locs, 32, cov(0.1), y_obs, R, M=3, J=4, verbose=False, X=X, want_predict=False)

    # the length scale by REML on the same tree: X is not sent again, each evaluation is one pass and the sweeps of the fit
    grid = [0.05, 0.1, 0.15, 0.2, 0.3, 0.45]
    crit = []
    for l in grid:
        tree.reevaluate(cov(l))
        crit.append(float(tree.getLikelihood(reml=True)[0, 0]))
        print("l = %.2f: profile %.2f, REML %.2f, beta %s" % (l, tree.trend.profile, crit[-1], np.round(tree.trend.beta, 3)))
    l_hat = grid[int(np.argmin(crit))]
    tree.reevaluate(cov(l_hat), want_predict=True)
    fit = tree.trend
    print("l_hat = %.2f (the field was drawn with %.2f)" % (l_hat, l_true))
    print("beta_hat     ", np.round(fit.beta, 4), " (truth", beta_true, ")")
    print("std. errors  ", np.round(np.sqrt(np.diag(fit.cov_beta)), 4))

    mean, sd = tree.predict()
    mean = np.asarray(mean).ravel()
    truth = X @ beta_true + field
    hid = ~obs
    z = (truth - mean)[hid] / sd[hid]
    print("RMSE at the %d hidden locations: %.4f; standardised errors: mean %.3f, sd %.3f" % (hid.sum(), np.sqrt(np.mean((truth - mean)[hid] ** 2)), z.mean(), z.std()))

    # new sites need their covariates; at a location of the tree predictAt reproduces predict()
    rows = rng.choice(N, 5, replace=False)
    m_at, sd_at = tree.predictAt(locs[rows], X_sites=X[rows])
    print("predictAt at tree locations - predict(): %.1e (mean), %.1e (sd)" % (np.abs(m_at[:, 0] - mean[rows]).max(), np.abs(sd_at - sd[rows]).max()))


if __name__ == "__main__":
    main()
