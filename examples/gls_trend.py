"""A linear trend by generalised least squares, from ONE factorisation of the tree.

Model: y = X beta + x + eps with x the MRA field and eps ~ N(0, R).  With A = Sigma_MRA[o, o] + R I at the observed locations,
    beta_hat = (X' A^-1 X)^-1 X' A^-1 y,        cov(beta_hat) = (X' A^-1 X)^-1,
and both come out of the quadratic form of the (1 + p) columns [y | 1 | x1 | x2]: quad = [y | X]' A^-1 [y | X] is what
MRATree.solve returns beside the kriging means.  The factors of the tree do not depend on the observed values, so the trend costs
one solve with four columns; the field is then predicted from the detrended data (the kriging mean is linear, so that prediction is
mean[:, 0] - mean[:, 1:] beta_hat from the same call: predict() on y - X beta_hat, shown below, gives the same numbers).

    python examples/gls_trend.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymra_amd.MRATools as mt          # noqa: E402
from pymra_amd import MRATree            # noqa: E402


def main(n=128, frac=0.4, R=1e-2, seed=4):
    np.random.seed(seed)
    locs = mt.genLocations2d(Nx=n, Ny=n)
    cov = lambda a, b=np.array([]): mt.Matern32(a, b, l=0.2, sig=1.0)          # noqa: E731
    N = n * n
    beta_true = np.array([2.0, -1.5, 0.75])
    X = np.column_stack([np.ones(N), locs[:, 0], locs[:, 1]])
    # a field with the right covariance on a coarse subsample would do; smooth random Fourier features keep the example dense-free
    w = np.random.normal(size=(64, 2)) / 0.2
    field = np.sqrt(2.0 / 64) * np.cos(locs @ w.T + np.random.uniform(0, 2 * np.pi, 64)).sum(axis=1)
    y = X @ beta_true + field + np.sqrt(R) * np.random.normal(size=N)
    obs = np.random.random(N) < frac
    y_obs = np.where(obs, y, np.nan).reshape(-1, 1)

    np.random.seed(seed + 1)                 # the tree's knot draws use the global RNG: the same seed gives the same tree below
    tree = MRATree(locs, 32, cov, y_obs, R, M=3, J=4, verbose=False)
    mean, quad = tree.solve(np.column_stack([np.nan_to_num(y_obs.ravel()), X]))   # columns [y | 1 | x1 | x2]
    Gxx, Gxy, Gyy = quad[1:, 1:], quad[1:, 0], quad[0, 0]
    cov_beta = np.linalg.inv(Gxx)
    beta_hat = cov_beta @ Gxy
    print("beta_hat      ", np.round(beta_hat, 4), " (truth", beta_true, ")")
    print("std. errors   ", np.round(np.sqrt(np.diag(cov_beta)), 4))
    print("profiled y'A^-1y - beta' X'A^-1y =", float(Gyy - Gxy @ beta_hat))

    field_hat = mean[:, 0] - mean[:, 1:] @ beta_hat                   # kriging mean of the detrended data, from the same call
    np.random.seed(seed + 1)
    tree2 = MRATree(locs, 32, cov, y_obs - (X @ beta_hat).reshape(-1, 1), R, M=3, J=4, verbose=False)
    m2 = np.asarray(tree2.predict()[0]).ravel()
    print("max |solve - predict() on y - X beta_hat| =", float(np.abs(field_hat - m2).max()))
    rmse = float(np.sqrt(np.mean((X @ beta_hat + field_hat - (X @ beta_true + field))[~obs] ** 2)))
    print("RMSE of trend + field at the unobserved locations:", round(rmse, 4))


if __name__ == "__main__":
    main()
