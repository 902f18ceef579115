#!/usr/bin/env python3
"""Gap filling with conditional simulation: draw a synthetic field from the MRA prior (exact for the tree's model, no dense
Cholesky), observe 30 % of it with noise, then draw posterior realisations and summarise a nonlinear functional (the share of the
domain above a threshold) that the per-location predictive sd cannot answer.

    python examples/conditional_simulation.py [grid_side] [M] [r0] [n_draws]
"""
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import pymra_amd.MRATools as mt
from pymra_amd import MRATree


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    M = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    r0 = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    nsim = int(sys.argv[4]) if len(sys.argv) > 4 else 32
    np.random.seed(17)
    locs = mt.genLocations2d(Nx=n, Ny=n)
    N = n * n
    cov = lambda a, b: mt.Matern32(a, b, l=0.2, sig=1.0)
    R = 0.05

    # 1. a synthetic "truth": one draw from the MRA prior of a tree on these locations (observations only enter posterior draws)
    t0 = time.time()
    y_blank = np.full((N, 1), np.nan)
    y_blank[0] = 0.0                                  # the tree needs at least one observed row; a prior draw ignores them
    truth = MRATree(locs, r0, cov, y_blank, R, M=M, J=4).simulate(1, "prior")[:, 0]

    # 2. noisy observations at 30 % of the locations
    obs = np.full((N, 1), np.nan)
    oi = np.random.choice(N, int(0.3 * N), replace=False)
    obs[oi, 0] = truth[oi] + np.sqrt(R) * np.random.normal(size=len(oi))

    # 3. the fitted tree: kriging mean / sd and posterior realisations
    tree = MRATree(locs, r0, cov, obs, R, M=M, J=4)
    mean, sd = tree.predict()
    mean = np.asarray(mean).ravel()
    draws = tree.simulate(nsim, "posterior")
    t1 = time.time()

    gap = np.ones(N, dtype=bool)
    gap[oi] = False
    thr = 1.0
    share = (draws > thr).mean(axis=0)                # one value of the functional per realisation
    print("%d x %d grid, M=%d, r0=%d: %d posterior draws in %.2f s (tree, prior draw and fit included)" % (n, n, M, r0, nsim, t1 - t0))
    print("RMSE of the kriging mean in the gaps: %.4f (mean predictive sd there %.4f)" % (
        np.sqrt(np.mean((mean[gap] - truth[gap]) ** 2)), float(np.mean(sd[gap]))))
    print("coverage of +-2 sd in the gaps: %.3f" % np.mean(np.abs(mean[gap] - truth[gap]) <= 2 * sd[gap]))
    print("share of the domain above %.1f: truth %.4f, posterior %.4f +- %.4f (plug-in kriging mean: %.4f)" % (
        thr, np.mean(truth > thr), share.mean(), share.std(), np.mean(mean > thr)))


if __name__ == "__main__":
    main()
