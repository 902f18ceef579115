#!/usr/bin/env python3
"""Site averages of unequal numbers of replicates: y_i is the mean of n_i measurements with error variance tau^2 each, so its noise
variance is r_i = tau^2 / n_i - a vector R.  The fit with the right noise against the homoscedastic misfit that gives every site the
average variance: -2 log-likelihood, the error of the predictive mean and how well the predictive sd is calibrated, separately at
the sites with one replicate and at those with many.

    python examples/replicate_counts.py [grid_side] [M] [r0]
"""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import pymra_amd.MRATools as mt
from pymra_amd import MRATree


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    M = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    r0 = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    np.random.seed(23)
    locs = mt.genLocations2d(Nx=n, Ny=n)
    N = n * n
    cov = lambda a, b: mt.Matern32(a, b, l=0.2, sig=1.0)
    tau2 = 0.5
    y_blank = np.full((N, 1), np.nan)
    y_blank[0] = 0.0                                  # the tree needs at least one observed row; a prior draw ignores them
    truth = MRATree(locs, r0, cov, y_blank, tau2, M=M, J=4).simulate(1, "prior")[:, 0]

    seen = np.random.uniform(size=N) < 0.5
    counts = np.where(np.random.uniform(size=N) < 0.5, 1, 25)          # one replicate, or twenty-five
    r = tau2 / counts                                                   # the noise variance of a site average
    obs = np.full((N, 1), np.nan)
    obs[seen, 0] = truth[seen] + np.sqrt(r[seen]) * np.random.normal(size=int(seen.sum()))

    right = MRATree(locs, r0, cov, obs, r, M=M, J=4)                   # R: one variance per location (read where obs is finite)
    lik_right = float(right.getLikelihood()[0, 0])
    mean_r, sd_r = (np.asarray(a).ravel() for a in right.predict())
    lik_flat = float(right.setNoise(float(r[seen].mean()), want_predict=True)[0, 0])      # same tree, every site the average variance
    mean_f, sd_f = (np.asarray(a).ravel() for a in right.predict())

    print("%d observed sites of %d, %d with one replicate; tau^2 = %.2f" % (seen.sum(), N, (seen & (counts == 1)).sum(), tau2))
    print("-2 log-likelihood: r_i = tau^2 / n_i %.1f, one average variance %.1f (difference %.1f)" % (lik_right, lik_flat, lik_flat - lik_right))
    for name, who in (("one replicate", seen & (counts == 1)), ("25 replicates", seen & (counts == 25)), ("unobserved", ~seen)):
        zr, zf = (truth[who] - mean_r[who]) / sd_r[who], (truth[who] - mean_f[who]) / sd_f[who]
        print("%-14s rmse %.4f / %.4f, sd of the standardised error %.3f / %.3f  (vector / scalar; calibrated = 1)"
              % (name, np.sqrt(np.mean((truth[who] - mean_r[who]) ** 2)), np.sqrt(np.mean((truth[who] - mean_f[who]) ** 2)), zr.std(), zf.std()))


if __name__ == "__main__":
    main()
