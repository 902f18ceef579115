"""The NumPy restatement of mra_predict_sites (tests/_treesites.py) against truths that do not share its algebra: at sites placed on
the tree's own rows the level-wise oracle's mean and var and the reference's own Sigma (tests/golden/*_nodes.npz); at sites off the
rows dense Gaussian conditioning on the augmented covariance [rows ; sites]; on a single-leaf tree plain kriging.  No GPU.

Bounds.  Where the suite already bounds the same quantity between float64 restatements the assertion is quoted:
  * mean against the level-wise oracle: tests/test_solve_cpu.py `assert e_m <= 1e-9` (the solver twin's mean against run_levelwise);
  * a covariance row against the reference's Sigma, and a posterior against dense conditioning of it: tests/test_cov_cpu.py
    `assert e_o <= TOL * scale` with TOL = 1e-9 and scale the largest prior variance.
The variance against the level-wise oracle has no such assertion: VAR_TOL is 100 x the 4e-15 seen when the four steps were first
checked in NumPy (2-D trees of 32^2 and 48^2 points, a 1-D tree of 700), scaled by the largest prior variance."""
import functools
import os

import numpy as np
import pytest

import _cases as K
import _sampling as SM
import _treesites as TS
from oracle.mra_levelwise import run_levelwise

CASES = ["g32", "c1", "kat3", "u3"]        # 2-D grids, 1-D trees (c1, kat3: rows a split drops), phantom knot columns (u3)
MEAN_TOL = 1e-9
DENSE_TOL = 1e-9
VAR_TOL = 4e-13


def leaf_of_rows(topo):
    """[P] leaf node of a padded row (-1 outside every leaf)"""
    out = np.full(topo.P, -1, dtype=np.int32)
    for i in np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]:
        out[int(topo.node_row0[i]):int(topo.node_row1[i])] = i
    return out


def nearest_leaf(topo, locs, sites):
    """MRATree.locate's rule, by brute force: the leaf of the nearest reported tree location"""
    rows = np.nonzero(SM.reported(topo))[0]
    pts = np.asarray(locs, float).reshape(topo.N, -1)[topo.perm[rows]]
    d2 = ((np.asarray(sites, float).reshape(len(sites), 1, -1) - pts[None]) ** 2).sum(-1)
    return leaf_of_rows(topo)[rows[np.argmin(d2, axis=1)]]


def off_row_sites(locs, n, seed):
    X = np.asarray(locs, float).reshape(len(locs), -1)
    lo, hi = X.min(0), X.max(0)
    return lo + (hi - lo) * np.random.default_rng(seed).random((n, X.shape[1]))


@functools.lru_cache(maxsize=None)
def _state(name):
    cs = K.load_case(name)
    return cs, TS.SiteState(cs["topo"], cs["locs"], cs["spec"], cs["y_obs"], float(cs["c"]["R"]))


@pytest.mark.parametrize("name", CASES)
def test_sites_on_tree_rows_are_the_oracles_predictions_and_the_references_sigma(name):
    cs, st = _state(name)
    topo, locs, spec, R = cs["topo"], cs["locs"], cs["spec"], float(cs["c"]["R"])
    rows = np.nonzero(SM.reported(topo))[0]
    X = np.asarray(locs, float).reshape(topo.N, -1)
    sites, leaf = X[topo.perm[rows]], leaf_of_rows(topo)[rows]
    mean, var = TS.tree_sites(topo, locs, spec, cs["y_obs"], R, sites, leaf, state=st)
    ref = run_levelwise(topo, locs, spec, cs["y_obs"], R)
    S = SM.golden_prior_sigma(name, topo)
    scale = np.abs(np.diag(S)).max()
    e_m = np.abs(mean[:, 0] - ref["mean"][topo.perm[rows]]).max()
    e_v = np.abs(var - ref["var"][topo.perm[rows]]).max()
    pick = np.unique(np.linspace(0, len(rows) - 1, 64).astype(int))          # covariance rows: 64 sites spread over the leaves
    Csr, Css = TS.site_prior_cov(st, sites[pick], leaf[pick])
    e_c = np.abs(Csr - S[rows[pick]]).max()
    e_s = np.abs(Css - S[np.ix_(rows[pick], rows[pick])]).max()
    print("%s: %d sites on rows: mean err %.2e, var err %.2e, Sigma row err %.2e, Sigma site-site err %.2e (scale %.3f)" % (name, len(rows), e_m, e_v, e_c, e_s, scale))
    assert e_m <= MEAN_TOL
    assert e_v <= VAR_TOL * scale
    assert e_c <= DENSE_TOL * scale
    assert e_s <= DENSE_TOL * scale


@pytest.mark.parametrize("name", CASES)
def test_off_row_sites_are_dense_conditioning_on_the_augmented_covariance(name):
    cs, st = _state(name)
    topo, locs, spec, R = cs["topo"], cs["locs"], cs["spec"], float(cs["c"]["R"])
    rows = np.nonzero(SM.reported(topo))[0]
    sites = off_row_sites(locs, 40, seed=3)
    leaf = nearest_leaf(topo, locs, sites)
    Y = np.where(np.isfinite(np.asarray(cs["y_obs"], float).reshape(-1, 1)), np.random.default_rng(4).standard_normal((topo.N, 3)), np.nan)
    Y[:, 0] = np.asarray(cs["y_obs"], float).ravel()
    mean, var = TS.tree_sites(topo, locs, spec, cs["y_obs"], R, sites, leaf, Y=Y, state=st)
    Csr, Css = TS.site_prior_cov(st, sites, leaf)
    S = SM.golden_prior_sigma(name, topo)[np.ix_(rows, rows)]
    aug = np.block([[S, Csr[:, rows].T], [Csr[:, rows], Css]])
    scale = np.abs(np.diag(aug)).max()
    ev = np.linalg.eigvalsh(aug).min()
    o = np.isfinite(Y[:, 0])[topo.perm[rows]]
    L = np.linalg.cholesky(S[np.ix_(o, o)] + R * np.eye(int(o.sum())))
    T = np.linalg.solve(L, Csr[:, rows][:, o].T)
    want_m = T.T @ np.linalg.solve(L, Y[topo.perm[rows]][o])
    want_v = np.diag(Css) - np.einsum("ij,ij->j", T, T)
    e_m, e_v = np.abs(mean - want_m).max(), np.abs(var - want_v).max()
    print("%s: 40 off-row sites: mean err %.2e, var err %.2e, smallest eigenvalue of the augmented covariance %.2e (scale %.3f)" % (name, e_m, e_v, ev, scale))
    assert e_m <= DENSE_TOL * max(1.0, np.abs(want_m).max())
    assert e_v <= DENSE_TOL * scale
    assert ev >= -DENSE_TOL * scale * len(aug)               # positive semi-definite down to roundoff (eigvalsh: ~ n eps |A|)


def test_a_single_leaf_is_plain_kriging():
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    rng = np.random.RandomState(18)
    locs = mt.genLocations2d(Nx=18, Ny=18)
    y = rng.normal(size=(len(locs), 1))
    y_obs = np.where(rng.uniform(size=(len(locs), 1)) < 0.5, y, np.nan)
    spec, R = mt.KernelSpec(mt.KIND_MATERN32, 0.3, 1.0), 2e-2
    topo = build_topology(locs, 16, 0, 4)
    assert topo.n_nodes == 1
    sites = off_row_sites(locs, 40, seed=5)
    mean, var = TS.tree_sites(topo, locs, spec, y_obs, R, sites, np.zeros(40, dtype=np.int32))
    _, km, ksd = K.kriging(np.vstack([locs, sites]), np.vstack([y_obs, np.full((40, 1), np.nan)]), spec, R)
    e_m, e_v = np.abs(mean[:, 0] - km[len(locs):]).max(), np.abs(var - ksd[len(locs):] ** 2).max()
    print("M = 0: mean err %.2e, var err %.2e" % (e_m, e_v))
    assert e_m <= DENSE_TOL and e_v <= DENSE_TOL


def test_sites_surface_is_exported():
    from pymra_amd import plan
    from pymra_amd.MRATree import MRATree
    assert "mra_predict_sites" in plan.EXPORTS
    assert callable(plan.HipPlan.predict_sites) and callable(MRATree.locate) and callable(MRATree.predictAt)
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    assert "int mra_predict_sites(mra_plan *plan, uint32_t flags, int64_t n_sites, const double *sites, const int32_t *leaf, int64_t n_cols," in hdr
    assert "#define MRA_OPT_SITES_CHUNK_BYTES 21" in hdr
