#!/usr/bin/env python3
"""Choosing a covariance family by cross-validation, without refitting: a field sampled from a Gaussian process with a Matern 3/2
covariance is observed with noise at 40 % of a grid; the same tree is fitted once with an exponential and once with a Matern 3/2
covariance, and each fit is scored by leaving out the observations of one leaf at a time (spatial block cross-validation on the
tree's own partition) - every leave-out predictive distribution comes from the factors of that one fit.  Then the ten observations
the better model finds most surprising, leaving each out on its own.

    python examples/cross_validation.py [grid_side] [M] [r0]
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
    np.random.seed(23)
    locs = mt.genLocations2d(Nx=n, Ny=n)
    N = n * n
    R = 0.05
    families = {"ExpCovFun": lambda a, b: mt.ExpCovFun(a, b, l=0.2), "Matern32": lambda a, b: mt.Matern32(a, b, l=0.2, sig=1.0)}

    # the data: one draw from the MRA prior of a Matern 3/2 tree on these locations, 40 % of it observed with noise
    y_blank = np.full((N, 1), np.nan)
    y_blank[0] = 0.0
    truth = MRATree(locs, r0, families["Matern32"], y_blank, R, M=M, J=4, verbose=False).simulate(1, "prior")[:, 0]
    obs = np.full((N, 1), np.nan)
    oi = np.random.choice(N, int(0.4 * N), replace=False)
    obs[oi, 0] = truth[oi] + np.sqrt(R) * np.random.normal(size=len(oi))

    # one tree, one factorisation per family
    tree = MRATree(locs, r0, families["ExpCovFun"], obs, R, M=M, J=4, verbose=False)
    results = {}
    for name, cov in families.items():
        t0 = time.time()
        lik = float(tree.reevaluate(cov)[0, 0])
        t1 = time.time()
        cv = tree.crossValidate("leaf")
        t2 = time.time()
        results[name] = cv
        print("%-10s d + u %.2f | leave-a-leaf-out log score %.2f over %d leaves (%d observations), mean z^2 %.3f, max leverage %.3f, "
              "d(d + u)/dR %.1f | pass %.3f s, cross-validation %.3f s"
              % (name, lik, cv.score, len(cv.leaf_lpd), cv.n, float(np.nanmean(cv.z ** 2)), cv.leverage_max, cv.dlik_dR, t1 - t0, t2 - t1))
    best = max(results, key=lambda k: results[k].score)
    print("block cross-validation prefers %s (the data were drawn with Matern32)" % best)

    tree.reevaluate(families[best])
    loo = tree.crossValidate("loo")
    worst = np.argsort(-np.nan_to_num(np.abs(loo.z)))[:10]
    print("the ten largest |z| of %s, leaving one observation out at a time:" % best)
    for i in worst:
        print("  location (%.3f, %.3f): observed %+.3f, predicted %+.3f +- %.3f, z %+.2f" % (locs[i, 0], locs[i, 1], obs[i, 0], loo.mean[i], loo.sd[i], loo.z[i]))


if __name__ == "__main__":
    main()
