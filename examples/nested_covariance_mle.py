#!/usr/bin/env python3
"""Fit a NESTED covariance model: a short-range Matern-3/2 structure plus a long-range exponential one, the sum evaluated on the
device as one kernel (mt.Matern32(...) + mt.ExpCovFun(...) is a KernelSum).  The field is simulated from the
two-structure model with simulate(); maximum likelihood over (log l1, log l2, the first structure's share of the sill) with
Nelder-Mead on one tree: every likelihood evaluation is tree.reevaluate(...) - the tree, the locations and the observations stay on
the GPU, a step of the optimiser uploads the table of the two components (96 bytes) and nothing else.

    python examples/nested_covariance_mle.py [grid_side] [M] [r0]
"""
import sys
import time

import numpy as np
import scipy.optimize as opt

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import pymra_amd.MRATools as mt
from pymra_amd import MRATree


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    M = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    r0 = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    np.random.seed(11)
    locs = mt.genLocations2d(Nx=n, Ny=n)
    true_l1, true_l2, true_share, me = 0.05, 0.8, 0.6, 1e-2

    def cov(l1, l2, share):
        return lambda a, b: mt.Matern32(a, b, l=l1, sig=share) + (1.0 - share) * mt.ExpCovFun(a, b, l=l2)

    # a draw from the MRA prior at the true parameters (a tree without observations)
    gen = MRATree(locs, r0, cov(true_l1, true_l2, true_share), np.full((n * n, 1), np.nan), me, M=M, J=4, verbose=False)
    x = gen.simulate(1, "prior", seed=5)
    y = x + np.sqrt(me) * np.random.normal(size=x.shape)
    y_obs = np.where(np.random.uniform(size=y.shape) < 0.4, y, np.nan)

    t0 = time.time()
    np.random.seed(11)                      # the same knots as the generating tree
    tree = MRATree(locs, r0, cov(0.1, 0.4, 0.5), y_obs, me, M=M, J=4, want_predict=False, verbose=False)
    print("tree + first likelihood: %.3f s, lik = %.4f; kernel %r on the %s route"
          % (time.time() - t0, tree.getLikelihood()[0, 0], tree.kernel, tree.plan.route()["path"]))
    calls = [0]

    def unpack(p):
        return float(np.exp(p[0])), float(np.exp(p[1])), float(1.0 / (1.0 + np.exp(-p[2])))

    def objective(p):
        calls[0] += 1
        return float(tree.reevaluate(cov(*unpack(p)))[0, 0])

    t0 = time.time()
    res = opt.minimize(objective, [np.log(0.1), np.log(0.4), 0.0], method="nelder-mead", options={"xatol": 1e-3, "fatol": 1e-4})
    dt = time.time() - t0
    l1, l2, share = unpack(res.x)
    print("Nelder-Mead: l1_hat = %.4f (true %.2f), l2_hat = %.4f (true %.2f), share_hat = %.3f (true %.2f) after %d likelihood evaluations "
          "in %.3f s (%.2f ms each)" % (l1, true_l1, l2, true_l2, share, true_share, calls[0], dt, 1e3 * dt / calls[0]))
    print("-2 log-likelihood: %.4f at the estimate, %.4f at the truth"
          % (res.fun, float(tree.reevaluate(cov(true_l1, true_l2, true_share))[0, 0])))


if __name__ == "__main__":
    main()
