"""Does a covariate earn its place?  Cross-validating a regression trend without refitting.

Model: y = X beta + x + eps with a flat prior on beta (examples/universal_kriging.py).  The data have a mean that depends on an
elevation-like covariate; two trees are fitted on the same locations, one with an intercept alone and one with the intercept and the
covariate, and each is scored by spatial block cross-validation on the tree's own partition - every leaf left out in turn.

`crossValidate(kind, trend="refit")` estimates beta again without the left-out group, which is proper universal-kriging
cross-validation: the score pays for the uncertainty of beta.  `trend="fixed"` plugs in the beta of the full fit: the score of the
field model around a trend taken as known, always a little better, and the figure to compare with a zero-mean fit of detrended data.
Every leave-out distribution comes from the factors of the one fit and a few sweeps for the trend - no refit.

    python examples/trend_cross_validation.py [grid_side]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymra_amd.MRATools as mt          # noqa: E402
from pymra_amd import MRATree            # noqa: E402


def main(n=128, frac=0.4, R=1e-2, l=0.2, seed=4):
    rng = np.random.default_rng(seed)
    locs = mt.genLocations2d(Nx=n, Ny=n)
    N = n * n
    elevation = np.sin(3.0 * locs[:, 0]) * np.cos(2.0 * locs[:, 1]) + 0.3 * rng.standard_normal(N)
    w = rng.normal(size=(64, 2)) / l                                   # a smooth field: random Fourier features
    field = np.sqrt(2.0 / 64) * np.cos(locs @ w.T + rng.uniform(0, 2 * np.pi, 64)).sum(axis=1)
    y = 2.0 + 0.75 * elevation + field + np.sqrt(R) * rng.standard_normal(N)
    y_obs = np.where(rng.random(N) < frac, y, np.nan).reshape(-1, 1)
    cov = lambda a, b=np.array([]): mt.Matern32(a, b, l=l, sig=1.0)    # noqa: E731
    designs = {"intercept": np.ones((N, 1)), "intercept + elevation": np.column_stack([np.ones(N), elevation])}

    scores = {}
    for name, X in designs.items():
        np.random.seed(seed)                                           # the same knots for both trees
        tree = MRATree(locs, 32, cov, y_obs, R, M=3, J=4, verbose=False, X=X, want_predict=False)
        print("%s: beta %s +- %s, REML %.2f" % (name, np.round(tree.trend.beta, 3), np.round(np.sqrt(np.diag(tree.trend.cov_beta)), 3), tree.trend.reml))
        for kind in ("leaf", "loo"):
            for mode in ("refit", "fixed"):
                t0 = time.time()
                cv = tree.crossValidate(kind, trend=mode)
                scores[(name, kind, mode)] = cv.score
                print("  %-4s %-5s log score %10.2f over %d observations, mean z^2 %.3f, max leverage %.3f, d REML / dR %.1f (%.3f s)"
                      % (kind, mode, cv.score, cv.n, float(np.nanmean(cv.z ** 2)), cv.leverage_max, cv.dlik_dR_reml, time.time() - t0))
    for kind in ("leaf", "loo"):
        for mode in ("refit", "fixed"):
            gain = scores[("intercept + elevation", kind, mode)] - scores[("intercept", kind, mode)]
            print("the covariate changes the %s log score (%s) by %+.2f" % (kind, mode, gain))


if __name__ == "__main__":
    main(*([int(sys.argv[1])] if len(sys.argv) > 1 else []))
