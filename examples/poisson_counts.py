#!/usr/bin/env python3
"""Disease-mapping style counts on a grid: z_i ~ Poisson(E_i exp(x(s_i))) with known exposures E_i and a latent Matern field x.
The Laplace likelihood -2 log q(z) of MRATree.fitLaplace is minimised over the kernel's range and variance with Nelder-Mead - the
tree, the data and the previous fit's mode stay on the GPU between objective calls, so every call after the first starts warm - and
the fitted field is read as a relative-risk map exp(x) on a finer grid with predictAt.

    python examples/poisson_counts.py [grid_side] [M] [r0]
"""
import sys
import time

import numpy as np
import scipy.optimize as opt

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import pymra_amd.MRATools as mt
from pymra_amd import MRATree


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    M = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    r0 = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    np.random.seed(31)
    locs = mt.genLocations2d(Nx=n, Ny=n)
    N = n * n
    true_l, true_sig = 0.25, 0.6
    y_blank = np.full((N, 1), np.nan)
    y_blank[0] = 0.0                                  # the tree needs at least one observed row; a prior draw ignores them
    truth = MRATree(locs, r0, lambda a, b: mt.Matern32(a, b, l=true_l, sig=true_sig), y_blank, 1.0, M=M, J=4).simulate(1, "prior")[:, 0]

    seen = np.random.uniform(size=N) < 0.4
    E = np.exp(np.random.uniform(np.log(0.5), np.log(20.0), size=N))  # expected counts at relative risk 1
    z = np.full((N, 1), np.nan)
    z[seen, 0] = np.random.poisson(E[seen] * np.exp(truth[seen]))
    offset = np.log(E)

    # the tree is built on the mask of the counts (its first, Gaussian pass is not used); every fit below reuses it
    tree = MRATree(locs, r0, lambda a, b: mt.Matern32(a, b, l=0.5, sig=1.0), z, 1.0, M=M, J=4, want_predict=False)
    calls, passes = [0], []

    def objective(p):
        l, sig = float(np.exp(p[0])), float(np.exp(p[1]))
        calls[0] += 1
        lik = tree.fitLaplace("poisson", offset=offset, cov=lambda a, b: mt.Matern32(a, b, l=l, sig=sig))
        passes.append(tree.laplace["passes"])
        return lik if tree.laplace["converged"] else np.inf

    t0 = time.time()
    res = opt.minimize(objective, np.log([0.5, 1.0]), method="nelder-mead", options={"xatol": 1e-3, "fatol": 1e-3})
    dt = time.time() - t0
    l_hat, sig_hat = np.exp(res.x)
    print("%d counts on %d sites (sum %d); truth l = %.2f, sig = %.2f" % (seen.sum(), N, np.nansum(z), true_l, true_sig))
    print("Nelder-Mead on -2 log q: l = %.3f, sig = %.3f after %d fits in %.2f s; Newton passes per fit: first %d, then %.1f on average (warm starts)"
          % (l_hat, sig_hat, calls[0], dt, passes[0], np.mean(passes[1:])))

    tree.fitLaplace("poisson", offset=offset, cov=lambda a, b: mt.Matern32(a, b, l=float(l_hat), sig=float(sig_hat)))
    mean, sd = (np.asarray(a).ravel() for a in tree.predict())
    print("latent field at the sites: rmse %.3f observed, %.3f unobserved (prior sd %.3f)"
          % (np.sqrt(np.mean((mean - truth)[seen] ** 2)), np.sqrt(np.mean((mean - truth)[~seen] ** 2)), np.sqrt(true_sig)))
    # relative risk on a grid twice as fine, off the rows of the tree: median exp(m) and a 95 % band exp(m -+ 1.96 s)
    g = (np.arange(2 * n) + 0.5) / (2 * n)
    fine = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    m, s = tree.predictAt(fine)
    rr = np.exp(m[:, 0])
    print("relative-risk map on %d x %d: range %.2f - %.2f, sites with the whole 95 %% band above 1: %d, below 1: %d"
          % (2 * n, 2 * n, rr.min(), rr.max(), int((m[:, 0] - 1.96 * s > 0).sum()), int((m[:, 0] + 1.96 * s < 0).sum())))


if __name__ == "__main__":
    main()
