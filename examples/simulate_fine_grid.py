#!/usr/bin/env python3
"""Fit on scattered data, then conditional simulation on a FINE grid: 100 posterior draws of the latent field at 512 x 512 locations
that are not rows of the tree (sampleAt: no dense covariance matrix, no second tree), a map of the probability that the field exceeds a
threshold, and the standard error of a regional mean - from the draws, and exactly from covarianceAt on a 64 x 64 sub-grid of the region.

    python examples/simulate_fine_grid.py [n_obs] [grid_side] [n_draws] [M] [r0]
"""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import pymra_amd.MRATools as mt
from pymra_amd import MRATree


def main():
    n_obs = int(sys.argv[1]) if len(sys.argv) > 1 else 6000
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    n_draws = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    M = int(sys.argv[4]) if len(sys.argv) > 4 else 4              # 256 leaves: about 1000 grid points each (a leaf may receive 4096)
    r0 = int(sys.argv[5]) if len(sys.argv) > 5 else 16
    np.random.seed(29)
    locs = np.random.uniform(size=(n_obs, 2))         # scattered locations
    cov = lambda a, b: mt.Matern32(a, b, l=0.2, sig=1.0)
    R = 0.05
    y_blank = np.full((n_obs, 1), np.nan)
    y_blank[0] = 0.0                                  # the tree needs at least one observed row; a prior draw ignores them
    truth = MRATree(locs, r0, cov, y_blank, R, M=M, J=4).simulate(1, "prior", seed=1)
    y = truth + np.sqrt(R) * np.random.normal(size=truth.shape)
    tree = MRATree(locs, r0, cov, y, R, M=M, J=4)
    print("%d scattered observations, likelihood %.3f" % (n_obs, float(tree.getLikelihood()[0, 0])))

    g = (np.arange(side) + 0.5) / side
    grid = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    leaf = tree.locate(grid)
    per_leaf = np.bincount(leaf).max()
    print("grid %d x %d: %d sites in %d leaves, at most %d in one leaf" % (side, side, len(grid), len(np.unique(leaf)), per_leaf))
    draws = tree.sampleAt(grid, n_draws, "posterior", seed=7, leaf=leaf)          # (side^2, n_draws)
    mean, sd = tree.predictAt(grid, leaf=leaf)
    print("draws: |mean of draws - predictAt mean| at most %.3f (sd / sqrt(n) is about %.3f); sd of draws / predictAt sd in [%.2f, %.2f]"
          % (np.abs(draws.mean(1) - mean[:, 0]).max(), sd.max() / np.sqrt(n_draws), (draws.std(1) / np.maximum(sd, 1e-12)).min(), (draws.std(1) / np.maximum(sd, 1e-12)).max()))

    thr = 1.0                                          # exceedance probability map P(x(s) > thr | y)
    p_exc = (draws > thr).mean(1).reshape(side, side)
    print("P(x > %.1f | y): %.1f%% of the grid above 0.5, %.1f%% above 0.95" % (thr, 100 * (p_exc > 0.5).mean(), 100 * (p_exc > 0.95).mean()))
    # a nonlinear functional that needs joint draws: the area of the region where the field exceeds the threshold
    area = (draws > thr).mean(0)
    print("area of {x > %.1f}: %.4f +- %.4f of the domain" % (thr, area.mean(), area.std()))

    # the mean over the square [0.25, 0.5]^2: from the draws, and exactly from the joint covariance on a 64 x 64 sub-grid of it
    inside = np.all((grid >= 0.25) & (grid < 0.5), axis=1)
    reg = draws[inside].mean(0)
    sub = 0.25 + (np.arange(64) + 0.5) / 64 * 0.25
    sg = np.stack(np.meshgrid(sub, sub, indexing="ij"), axis=-1).reshape(-1, 2)
    S = tree.covarianceAt(sg, "posterior")
    w = np.full(len(sg), 1.0 / len(sg))
    print("regional mean over [0.25, 0.5]^2: %.4f, standard error from %d draws %.4f, from covarianceAt on 64 x 64 points %.4f"
          % (reg.mean(), n_draws, reg.std(ddof=1), np.sqrt(w @ S @ w)))


if __name__ == "__main__":
    main()
