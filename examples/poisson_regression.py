#!/usr/bin/env python3
"""Poisson regression with a spatial random effect: z_i ~ Poisson(E_i exp(X_i beta + x(s_i))) with known exposures E_i, an intercept
and two covariates, and a latent Matern field x.  MRATree.fitLaplace(X=X) finds the joint mode of (beta, x) on the GPU - one
factorisation pass and one generalised-least-squares step per Newton iteration - and returns the Laplace -2 log q with beta at its
mode (reml=True: with beta integrated out).  The fixed effects are reported as beta^ +- se, and the fitted relative risk
exp(X beta + x) is read on a finer grid with predictAt, where the covariates are known everywhere.

    python examples/poisson_regression.py [grid_side] [M] [r0]
"""
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import pymra_amd.MRATools as mt
from pymra_amd import MRATree


def covariates(s):
    """an intercept and two covariates known at every location, both varying faster than the latent field does: stripes across
    the first coordinate and a narrow bump"""
    return np.column_stack([np.ones(len(s)), np.sin(6 * np.pi * s[:, 0]), np.exp(-((s[:, 0] - 0.3) ** 2 + (s[:, 1] - 0.6) ** 2) / 0.01)])


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    M = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    r0 = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    np.random.seed(31)
    locs = mt.genLocations2d(Nx=n, Ny=n)
    N = n * n
    l, sig = 0.25, 0.3
    beta_true = np.array([-0.2, 0.5, 0.8])
    cov = lambda a, b: mt.Matern32(a, b, l=l, sig=sig)                    # noqa: E731
    y_blank = np.full((N, 1), np.nan)
    y_blank[0] = 0.0                                  # the tree needs at least one observed row; a prior draw ignores them
    field = MRATree(locs, r0, cov, y_blank, 1.0, M=M, J=4).simulate(1, "prior")[:, 0]

    X = covariates(locs)
    seen = np.random.uniform(size=N) < 0.4
    E = np.exp(np.random.uniform(np.log(0.5), np.log(20.0), size=N))  # expected counts at relative risk 1
    z = np.full((N, 1), np.nan)
    z[seen, 0] = np.random.poisson(E[seen] * np.exp(X[seen] @ beta_true + field[seen]))
    offset = np.log(E)

    # the tree is built on the mask of the counts (its first, Gaussian pass is not used)
    tree = MRATree(locs, r0, cov, z, 1.0, M=M, J=4, want_predict=False)
    t0 = time.time()
    profile = tree.fitLaplace("poisson", offset=offset, X=X)
    dt = time.time() - t0
    fit, info = tree.trend, tree.laplace
    print("%d counts on %d sites (sum %d); %d Newton passes in %.2f s, converged: %s"
          % (seen.sum(), N, np.nansum(z), info["passes"], dt, info["converged"]))
    print("-2 log q: %.3f with beta at its mode, %.3f with beta integrated out" % (profile, info["reml"]))
    se = np.sqrt(np.diag(fit.cov_beta))
    for name, b, s, b0 in zip(("intercept", "stripes", "bump"), fit.beta, se, beta_true):
        print("  %-9s %+.3f +- %.3f   (truth %+.3f, z = %+.1f)" % (name, b, s, b0, (b - b0) / s))

    # the same X again (a warm start; X is not sent a second time): one pass
    tree.fitLaplace("poisson", offset=offset, X=X)
    print("a second fit from the mode: %d pass" % tree.laplace["passes"])

    mean, sd = (np.asarray(a).ravel() for a in tree.predict())
    truth = X @ beta_true + field
    print("log relative risk at the sites: rmse %.3f observed, %.3f unobserved"
          % (np.sqrt(np.mean((mean - truth)[seen] ** 2)), np.sqrt(np.mean((mean - truth)[~seen] ** 2))))
    # relative risk on a grid twice as fine, off the rows of the tree: median exp(m) and a 95 % band exp(m -+ 1.96 s), the
    # uncertainty of beta^ included
    g = (np.arange(2 * n) + 0.5) / (2 * n)
    fine = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    m, s = tree.predictAt(fine, X_sites=covariates(fine))
    rr = np.exp(m[:, 0])
    print("relative-risk map on %d x %d: range %.2f - %.2f, sites with the whole 95 %% band above 1: %d, below 1: %d"
          % (2 * n, 2 * n, rr.min(), rr.max(), int((m[:, 0] - 1.96 * s > 0).sum()), int((m[:, 0] + 1.96 * s < 0).sum())))


if __name__ == "__main__":
    main()
