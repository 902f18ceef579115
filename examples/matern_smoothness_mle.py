#!/usr/bin/env python3
"""Estimate the SMOOTHNESS of a field, not only its range: maximum likelihood over (l, nu) of a Matern covariance with
Nelder-Mead, on one tree.  The field is simulated from the model at nu = 0.8 with simulate(); every likelihood evaluation is
tree.reevaluate(...) - the tree, the locations and the observations stay on the GPU, a change of nu uploads a table of 191
quadrature nodes and nothing else, and mt.Matern(nu=...) is evaluated on the device for any 0.1 <= nu <= 5.

    python examples/matern_smoothness_mle.py [grid_side] [M] [r0]
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
    true_l, true_nu, sig, me = 0.2, 0.8, 1.0, 1e-2

    def cov(l, nu):
        return lambda a, b: mt.Matern(a, b, l=l, sig=sig, nu=nu)

    # a draw from the MRA prior at the true parameters (a tree without observations)
    gen = MRATree(locs, r0, cov(true_l, true_nu), np.full((n * n, 1), np.nan), me, M=M, J=4, verbose=False)
    x = gen.simulate(1, "prior", seed=5)
    y = x + np.sqrt(me) * np.random.normal(size=x.shape)
    y_obs = np.where(np.random.uniform(size=y.shape) < 0.4, y, np.nan)

    t0 = time.time()
    np.random.seed(11)                      # the same knots as the generating tree
    tree = MRATree(locs, r0, cov(0.4, 1.5), y_obs, me, M=M, J=4, want_predict=False, verbose=False)
    print("tree + first likelihood: %.3f s, lik(l=0.4, nu=1.5) = %.4f (kind %d: the closed form)"
          % (time.time() - t0, tree.getLikelihood()[0, 0], tree.kernel.kind))
    calls = [0]

    def objective(p):
        calls[0] += 1
        l, nu = float(np.exp(p[0])), float(np.clip(np.exp(p[1]), mt.NU_MIN, mt.NU_MAX))
        return float(tree.reevaluate(cov(l, nu))[0, 0])

    t0 = time.time()
    res = opt.minimize(objective, [np.log(0.4), np.log(1.4)], method="nelder-mead", options={"xatol": 1e-3, "fatol": 1e-4})
    dt = time.time() - t0
    l_hat, nu_hat = float(np.exp(res.x[0])), float(np.clip(np.exp(res.x[1]), mt.NU_MIN, mt.NU_MAX))
    print("Nelder-Mead: l_hat = %.4f (true %.2f), nu_hat = %.4f (true %.2f) after %d likelihood evaluations in %.3f s (%.1f ms each)"
          % (l_hat, true_l, nu_hat, true_nu, calls[0], dt, 1e3 * dt / calls[0]))
    print("-2 log-likelihood: %.4f at the estimate, %.4f at the truth" % (res.fun, float(tree.reevaluate(cov(true_l, true_nu))[0, 0])))


if __name__ == "__main__":
    main()
