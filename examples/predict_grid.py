#!/usr/bin/env python3
"""Fit on scattered data, predict on a regular grid: the tree is built on the observation locations alone, so the likelihood that was
maximised and the predictions belong to the same model, and the grid can be as fine as one likes.  Several fields observed at the same
locations (here: three simulated fields) are predicted from ONE factorisation as a column block Y.

    python examples/predict_grid.py [n_obs] [grid_side] [M] [r0]
"""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import pymra_amd.MRATools as mt
from pymra_amd import MRATree


def main():
    n_obs = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    M = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    r0 = int(sys.argv[4]) if len(sys.argv) > 4 else 16
    np.random.seed(23)
    locs = np.random.uniform(size=(n_obs, 2))         # scattered locations
    cov = lambda a, b: mt.Matern32(a, b, l=0.2, sig=1.0)
    R = 0.05
    y_blank = np.full((n_obs, 1), np.nan)
    y_blank[0] = 0.0                                  # the tree needs at least one observed row; a prior draw ignores them
    fields = MRATree(locs, r0, cov, y_blank, R, M=M, J=4).simulate(3, "prior")
    Y = fields + np.sqrt(R) * np.random.normal(size=fields.shape)
    tree = MRATree(locs, r0, cov, Y[:, :1], R, M=M, J=4)                 # fitted on the first field; the factors do not depend on the values
    print("%d scattered observations, likelihood %.3f" % (n_obs, float(tree.getLikelihood()[0, 0])))

    g = (np.arange(side) + 0.5) / side
    grid = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    mean, sd = tree.predictAt(grid, Y=Y)              # (side^2, 3) means, (side^2,) sd of the latent field - the same for every column
    print("grid %d x %d: mean of field 0 in [%.3f, %.3f], predictive sd in [%.3f, %.3f] (sd of a new observation: sqrt(sd^2 + R))"
          % (side, side, mean[:, 0].min(), mean[:, 0].max(), sd.min(), sd.max()))
    leaf = tree.locate(grid)                          # which region of the finest partition answers for each grid point
    print("the grid falls into %d of the tree's %d leaves" % (len(np.unique(leaf)), int(np.count_nonzero(tree.topology.node_leaf))))
    near = tree.predictAt(locs[:5])[0][:, 0]          # at a fitted location this is predict()
    print("at five data locations: predictAt %s, predict %s" % (np.round(near, 4), np.round(np.asarray(tree.predict()[0]).ravel()[:5], 4)))


if __name__ == "__main__":
    main()
