#!/usr/bin/env python3
"""Block kriging: the posterior mean and standard error of the AVERAGE of the field over a rectangle, from one fitted tree.  The
per-location predictive sd cannot give it (the locations inside the rectangle are correlated); functionalCovariance applies the
posterior covariance to the averaging weights.  As a sanity print, the same standard error from 2000 posterior draws.

    python examples/regional_mean.py [grid_side] [M] [r0]
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
    np.random.seed(17)
    locs = mt.genLocations2d(Nx=n, Ny=n)
    N = n * n
    cov = lambda a, b: mt.Matern32(a, b, l=0.2, sig=1.0)
    R = 0.05
    y_blank = np.full((N, 1), np.nan)
    y_blank[0] = 0.0                                  # the tree needs at least one observed row; a prior draw ignores them
    truth = MRATree(locs, r0, cov, y_blank, R, M=M, J=4).simulate(1, "prior")[:, 0]
    obs = np.full((N, 1), np.nan)
    oi = np.random.choice(N, int(0.3 * N), replace=False)
    obs[oi, 0] = truth[oi] + np.sqrt(R) * np.random.normal(size=len(oi))
    tree = MRATree(locs, r0, cov, obs, R, M=M, J=4)

    box = (locs[:, 0] >= 0.30) & (locs[:, 0] <= 0.55) & (locs[:, 1] >= 0.40) & (locs[:, 1] <= 0.70)
    w = box / box.sum()                               # the averaging weights: a linear functional of the field
    mean = float(w @ np.asarray(tree.predict()[0]).ravel())
    se = float(np.sqrt(tree.functionalCovariance(w, "posterior")[0, 0]))
    se_prior = float(np.sqrt(tree.functionalCovariance(w, "prior")[0, 0]))
    print("average over %d locations: truth %.4f, posterior mean %.4f, standard error %.4f (prior sd %.4f)" % (box.sum(), w @ truth, mean, se, se_prior))
    draws = w @ tree.simulate(2000, "posterior")      # sanity: Monte Carlo gives the same number to two digits or so
    print("2000 posterior draws: mean %.4f, sd %.4f (Monte Carlo error of the sd ~ %.4f)" % (draws.mean(), draws.std(ddof=1), se / np.sqrt(2 * 2000)))


if __name__ == "__main__":
    main()
