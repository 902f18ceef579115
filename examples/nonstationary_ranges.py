#!/usr/bin/env python3
"""A field whose range grows tenfold across the unit square: short scales in the west, long ones in the east.
MRATree(..., local_range=lam) evaluates the nonstationary covariance of Paciorek & Schervish on the device: the covariance
coordinates are (x, y, lam), the kernel is mt.LocalRange.  The field is simulated from that model with simulate(); then, with the
true SHAPE of lam, maximum likelihood over (log l, log sig) - l multiplies the whole range field - with Nelder-Mead on one tree:
every evaluation is tree.reevaluate(...), which uploads five parameters.  Last, the predictive sd map is compared with the one of
the best stationary Matern-3/2 fitted to the same data: where the true range is short the stationary fit is too sure of itself
between the observations, where it is long it is not sure enough.

    python examples/nonstationary_ranges.py [grid_side] [M] [r0]
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
    shape = 10.0 ** (locs[:, 0] - 0.5)               # 0.32 .. 3.2: tenfold from west to east, 1 in the middle
    true_l, true_sig, me = 0.08, 1.5, 1e-2

    def cov(l, sig):
        return lambda a, b: mt.Matern32(a, b, l=l, sig=sig)

    # a draw from the MRA prior at the true parameters (a tree without observations)
    gen = MRATree(locs, r0, cov(true_l, true_sig), np.full((n * n, 1), np.nan), me, M=M, J=4, verbose=False, local_range=shape)
    x = gen.simulate(1, "prior", seed=5)
    y = x + np.sqrt(me) * np.random.normal(size=x.shape)
    y_obs = np.where(np.random.uniform(size=y.shape) < 0.2, y, np.nan)

    def fit(tree, start, make):
        calls = [0]

        def objective(p):
            calls[0] += 1
            return float(tree.reevaluate(make(float(np.exp(p[0])), float(np.exp(p[1]))))[0, 0])
        t0 = time.time()
        res = opt.minimize(objective, np.log(start), method="nelder-mead", options={"xatol": 1e-3, "fatol": 1e-4})
        dt = time.time() - t0
        l, sig = np.exp(res.x)
        tree.reevaluate(make(float(l), float(sig)), want_predict=True)
        return float(l), float(sig), res.fun, calls[0], 1e3 * dt / calls[0]

    np.random.seed(11)                      # the same knots as the generating tree
    local = MRATree(locs, r0, cov(0.2, 1.0), y_obs, me, M=M, J=4, want_predict=False, verbose=False, local_range=shape)
    print("kernel %r on the %s route" % (local.kernel, local.plan.route()["path"]))
    l, sig, lik_local, calls, ms = fit(local, [0.2, 1.0], cov)
    print("local ranges: l_hat = %.4f (true %.2f), sig_hat = %.3f (true %.2f), -2 log-likelihood %.2f after %d evaluations of %.2f ms"
          % (l, true_l, sig, true_sig, lik_local, calls, ms))
    np.random.seed(11)
    flat = MRATree(locs, r0, cov(0.2, 1.0), y_obs, me, M=M, J=4, want_predict=False, verbose=False)
    l0, sig0, lik_flat, calls, ms = fit(flat, [0.2, 1.0], cov)
    print("stationary:   l_hat = %.4f, sig_hat = %.3f, -2 log-likelihood %.2f (%.1f above) after %d evaluations of %.2f ms"
          % (l0, sig0, lik_flat, lik_flat - lik_local, calls, ms))

    # the predictive sd at the unobserved locations, by thirds of the square from west (short ranges) to east (long ranges)
    sd_l, sd_f = np.asarray(local.predict()[1]).ravel(), np.asarray(flat.predict()[1]).ravel()
    err_l = np.asarray(local.predict()[0]).ravel() - x[:, 0]
    err_f = np.asarray(flat.predict()[0]).ravel() - x[:, 0]
    miss = np.isnan(y_obs[:, 0]) & (sd_l > 0)
    print("unobserved locations      mean sd (local, stationary)    rmse (local, stationary)")
    for name, lo, hi in (("west  x < 1/3", 0.0, 1 / 3), ("middle", 1 / 3, 2 / 3), ("east  x > 2/3", 2 / 3, 1.01)):
        s = miss & (locs[:, 0] >= lo) & (locs[:, 0] < hi)
        print("  %-22s  %.3f  %.3f                   %.3f  %.3f"
              % (name, sd_l[s].mean(), sd_f[s].mean(), np.sqrt(np.mean(err_l[s] ** 2)), np.sqrt(np.mean(err_f[s] ** 2))))


if __name__ == "__main__":
    main()
