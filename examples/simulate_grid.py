#!/usr/bin/env python3
"""Fit on scattered data, then ask about a REGION of a prediction grid: conditional simulations on the grid cells inside it, and the
standard error of the regional mean from the joint posterior covariance of those cells, w^T Sigma_post w with w = 1 / n - put beside the
spread of the simulated regional means.  The tree is built on the observation locations alone: the grid cells are not rows of it, so
the model whose likelihood was maximised is the one that answers.

    python examples/simulate_grid.py [n_obs] [grid_side] [nsim] [M] [r0]
"""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import pymra_amd.MRATools as mt
from pymra_amd import MRATree


def main():
    n_obs = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    nsim = int(sys.argv[3]) if len(sys.argv) > 3 else 400
    M = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    r0 = int(sys.argv[5]) if len(sys.argv) > 5 else 16
    np.random.seed(23)
    locs = np.random.uniform(size=(n_obs, 2))         # scattered locations
    cov = lambda a, b: mt.Matern32(a, b, l=0.2, sig=1.0)
    R = 0.05
    y_blank = np.full((n_obs, 1), np.nan)
    y_blank[0] = 0.0                                  # the tree needs at least one observed row; a prior draw ignores them
    field = MRATree(locs, r0, cov, y_blank, R, M=M, J=4).simulate(1, "prior")
    y = field + np.sqrt(R) * np.random.normal(size=field.shape)
    tree = MRATree(locs, r0, cov, y, R, M=M, J=4)
    print("%d scattered observations, likelihood %.3f" % (n_obs, float(tree.getLikelihood()[0, 0])))

    g = (np.arange(side) + 0.5) / side
    grid = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    region = grid[np.all((grid >= [0.30, 0.55]) & (grid <= [0.50, 0.80]), axis=1)]      # the cells of one rectangle
    n = len(region)
    leaf = tree.locate(region)
    print("region: %d grid cells in %d leaves" % (n, len(np.unique(leaf))))

    mean, sd = tree.predictAt(region, leaf=leaf)
    S = tree.covarianceAt(region, leaf=leaf)          # (n, n) joint posterior covariance; its diagonal is sd ** 2
    w = np.full(n, 1.0 / n)
    se = np.sqrt(w @ S @ w)
    print("regional mean %.4f, standard error %.4f from covarianceAt (%.4f if the cells were taken as independent)"
          % (float(w @ mean[:, 0]), se, np.sqrt(w @ (sd ** 2 * w))))
    print("largest correlation between two different cells: %.3f" % np.max((S / np.outer(sd, sd))[~np.eye(n, dtype=bool)]))

    X = tree.simulateAt(region, nsim, seed=1, leaf=leaf)                  # (n, nsim) conditional simulations on the grid cells
    means = w @ X
    print("%d conditional simulations: regional means %.4f +- %.4f (sample sd; its own sampling error is ~%.4f)"
          % (nsim, means.mean(), means.std(ddof=1), se / np.sqrt(2.0 * (nsim - 1))))
    S0 = tree.covarianceAt(region, distr="prior", leaf=leaf)
    print("prior standard error of the same mean: %.4f" % np.sqrt(w @ S0 @ w))


if __name__ == "__main__":
    main()
