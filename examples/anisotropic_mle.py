#!/usr/bin/env python3
"""Maximum-likelihood estimation of a geometrically anisotropic range - (l, ratio, angle) of mt.aniso2d - and of the two ranges of
a space-time kernel (mt.ard) with Nelder-Mead on ONE tree: every objective call sends the new metric and kernel to the plan
(MRATree.reevaluate -> mra_plan_set_metric + mra_plan_set_kernel) and runs a likelihood-only pass; the tree, the locations and the
observations stay on the GPU.

    python examples/anisotropic_mle.py [grid_side] [M] [r0]
"""
import sys
import time

import numpy as np
import scipy.optimize as opt

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import pymra_amd.MRATools as mt
from pymra_amd import MRATree


def fit(tree, cov_of, start):
    calls = [0]

    def objective(p):
        calls[0] += 1
        return float(tree.reevaluate(cov_of(p))[0, 0])

    t0 = time.time()
    res = opt.minimize(objective, start, method="nelder-mead", options={"xatol": 1e-3, "fatol": 1e-6, "maxfev": 400})
    dt = time.time() - t0
    print("  Nelder-Mead: %d likelihood evaluations in %.2f s (%.1f ms each)" % (calls[0], dt, 1e3 * dt / calls[0]))
    return res.x


def anisotropic(n, M, r0):
    locs = mt.genLocations2d(Nx=n, Ny=n)
    l, ratio, angle, me = 0.5, 3.0, 30.0, 1e-2
    true = lambda a, b: mt.Matern32(a, b, l=l, metric=mt.aniso2d(ratio, angle))
    np.random.seed(11)
    x = MRATree(locs, r0, true, np.zeros((n * n, 1)), me, M=M, J=4, want_predict=False).simulate(1, "prior", seed=3)
    rng = np.random.default_rng(5)
    y = x + np.sqrt(me) * rng.standard_normal(x.shape)
    y[rng.random(n * n) < 0.6] = np.nan                       # 60 % hidden
    np.random.seed(11)
    tree = MRATree(locs, r0, lambda a, b: mt.Matern32(a, b, l=0.3), y, me, M=M, J=4, want_predict=False)
    print("anisotropic field on %d x %d, truth l = %.2f, ratio = %.1f, angle = %.0f deg" % (n, n, l, ratio, angle))
    # parameters: log l, log ratio, angle in degrees
    p = fit(tree, lambda p: (lambda a, b: mt.Matern32(a, b, l=float(np.exp(p[0])), metric=mt.aniso2d(float(np.exp(p[1])), float(p[2])))),
            [np.log(0.3), np.log(1.5), 10.0])
    ratio_hat, angle_hat = float(np.exp(p[1])), float(p[2])
    if ratio_hat < 1.0:                                        # the same metric named by its other axis
        ratio_hat, angle_hat, p[0] = 1.0 / ratio_hat, angle_hat + 90.0, p[0] - p[1]
    print("  estimates: l = %.3f, ratio = %.2f, angle = %.1f deg" % (np.exp(p[0]), ratio_hat, (angle_hat + 90.0) % 180.0 - 90.0))


def space_time(n, nt, M, r0):
    """(x, y, t) data: the tree is partitioned on (x, y) - every time of a location lands in the same region - and the covariance is
    evaluated on (x, y, t) with a spatial and a temporal range of its own"""
    g = mt.genLocations2d(Nx=n, Ny=n)
    rng = np.random.default_rng(7)
    xy = np.repeat(g, nt, axis=0) + rng.uniform(-0.2, 0.2, size=(n * n * nt, 2)) / n     # (distinct rows for the partition)
    xyt = np.column_stack((xy, np.tile(np.linspace(0.0, 1.0, nt), n * n)))
    ls, lt, me = 0.3, 0.6, 1e-2
    true = lambda a, b: mt.Matern32(a, b, l=1.0, metric=mt.ard([ls, ls, lt]))
    N = len(xyt)
    np.random.seed(11)
    x = MRATree(xy, r0, true, np.zeros((N, 1)), me, M=M, J=4, want_predict=False, cov_locs=xyt).simulate(1, "prior", seed=4)
    y = x + np.sqrt(me) * rng.standard_normal(x.shape)
    y[rng.random(N) < 0.6] = np.nan
    np.random.seed(11)
    tree = MRATree(xy, r0, lambda a, b: mt.Matern32(a, b, l=0.2), y, me, M=M, J=4, want_predict=False, cov_locs=xyt)
    print("space-time field, %d locations x %d times, truth l_space = %.2f, l_time = %.2f" % (n * n, nt, ls, lt))
    p = fit(tree, lambda p: (lambda a, b: mt.Matern32(a, b, l=1.0, metric=mt.ard(np.exp([p[0], p[0], p[1]])))),
            [np.log(0.15), np.log(0.3)])
    print("  estimates: l_space = %.3f, l_time = %.3f" % (np.exp(p[0]), np.exp(p[1])))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    M = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    r0 = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    anisotropic(n, M, r0)
    space_time(max(n // 4, 16), 8, M, r0)


if __name__ == "__main__":
    main()
