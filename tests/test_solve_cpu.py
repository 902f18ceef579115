"""The NumPy restatement of mra_solve (tests/_treesolve.py) against truths that do not share its algebra: the level-wise oracle run
once per column (mean and u), and dense Gaussian conditioning on the MRA prior covariance of the faithful oracle (the whole
quadratic form, off-diagonal entries included).  No GPU.  Bounds: those tests/test_oracle.py uses between float64 restatements
(mean 1e-9 absolute, u 1e-9 relative)."""
import numpy as np
import pytest

import _cases as K
import _treesolve as TS
from oracle.mra_levelwise import run_levelwise

CASES = ["g32", "c1", "kat3", "u3", "t201"]        # 2-D grids, 1-D trees (kat3, t201), phantom knot columns (u3)


def _columns(y_obs, c, seed=1):
    y = np.asarray(y_obs, float).ravel()
    obs = np.isfinite(y)
    Y = np.where(obs[:, None], np.random.default_rng(seed).standard_normal((len(y), c)), np.nan)
    Y[:, 0] = y
    return Y


def _check_columns(topo, locs, spec, y_obs, R, Y, mean, Q, cols):
    for k in cols:
        ref = run_levelwise(topo, locs, spec, Y[:, k], R)
        e_m = float(np.abs(mean[:, k] - ref["mean"]).max())
        e_u = abs(Q[k, k] - ref["u"]) / abs(ref["u"])
        print("column %d: mean err %.2e (scale %.2f), u rel err %.2e" % (k, e_m, np.abs(ref["mean"]).max(), e_u))
        assert e_m <= 1e-9
        assert e_u <= 1e-9


def _dense_quad(topo, locs, spec, y_obs, R, Y):
    from oracle.mra_faithful import prior_sigma_rows
    y = np.asarray(y_obs, float).ravel()
    rows = np.nonzero((topo.perm >= 0) & topo.in_leaf & np.isfinite(y)[topo.src])[0]
    S = prior_sigma_rows(topo, locs, spec.evaluate, rows)
    Yo = np.asarray(Y, float)[topo.perm[rows]]
    L = np.linalg.cholesky(S + R * np.eye(len(rows)))
    A = np.linalg.solve(L, Yo)
    return A.T @ A


@pytest.mark.parametrize("c", [1, 3, 16])
@pytest.mark.parametrize("name", CASES)
def test_restated_solve_matches_the_oracle_per_column(name, c):
    cs = K.load_case(name)
    topo, locs, spec, R = cs["topo"], cs["locs"], cs["spec"], float(cs["c"]["R"])
    Y = _columns(cs["y_obs"], c)
    mean, Q = TS.tree_solve(topo, locs, spec, cs["y_obs"], R, Y)
    assert mean.shape == (topo.N, c) and Q.shape == (c, c)
    _check_columns(topo, locs, spec, cs["y_obs"], R, Y, mean, Q, range(c))
    Qd = _dense_quad(topo, locs, spec, cs["y_obs"], R, Y)
    assert np.abs(Q - Qd).max() <= 1e-9 * np.abs(np.diag(Qd)).max()
    assert np.abs(Q - Q.T).max() <= 1e-12 * np.abs(np.diag(Q)).max()


@pytest.mark.parametrize("c", [1, 3, 16])
def test_restated_solve_on_a_mask_with_an_empty_leaf_and_an_empty_family(c):
    """The gap patterns of tests/test_gpu_likelihood_masks.py: a leaf without observations has q empty and beta = the chain's alpha;
    a whole family without observations contributes nothing to its parent's front."""
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    np.random.seed(7)
    locs = mt.genLocations2d(Nx=64, Ny=64)
    topo = build_topology(locs, 16, 3, 4)
    spec = mt.KernelSpec(mt.KIND_MATERN32, 0.25, 1.2)
    rng = np.random.default_rng(5)
    obs = rng.random(len(locs)) < 0.5
    leaves = [int(i) for i in np.nonzero(topo.node_leaf)[0]]
    fams = {}
    for i in leaves:
        fams.setdefault(int(topo.node_parent[i]), []).append(i)
    fam = sorted(fams)[2]
    for i in [leaves[0]] + fams[fam]:
        p = topo.perm[int(topo.node_row0[i]):int(topo.node_row1[i])]
        obs[p[p >= 0]] = False
    y_obs = np.where(obs, rng.standard_normal(len(locs)), np.nan)
    R = 2e-2
    Y = _columns(y_obs, c, seed=3)
    mean, Q = TS.tree_solve(topo, locs, spec, y_obs, R, Y)
    _check_columns(topo, locs, spec, y_obs, R, Y, mean, Q, sorted({0, c - 1}))
    Qd = _dense_quad(topo, locs, spec, y_obs, R, Y)
    assert np.abs(Q - Qd).max() <= 1e-9 * np.abs(np.diag(Qd)).max()


def test_solve_surface_is_exported():
    from pymra_amd import plan
    from pymra_amd.MRATree import MRATree
    assert "mra_solve" in plan.EXPORTS and plan.MRA_OPT_SAMPLE_SOLVE == 20
    assert callable(plan.HipPlan.solve) and callable(MRATree.solve) and callable(MRATree.getLikelihoods)
    import os
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    assert "int mra_solve(mra_plan *plan, uint32_t flags, int64_t n_cols, const double *Y, double *mean, double *quad);" in hdr
    assert "#define MRA_OPT_SAMPLE_SOLVE   20" in hdr
