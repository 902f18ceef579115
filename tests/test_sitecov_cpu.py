"""The NumPy restatement of mra_sites_cov (tests/_treesitecov.py) against truths that do not share its algebra: dense Gaussian
conditioning on the augmented covariance [rows ; sites] (tests/_treesites.site_prior_cov + the reference's own Sigma,
tests/golden/*_nodes.npz - the truth tests/test_sites_cpu.py uses), the reference's Sigma at sites placed on every reported row, the
variance of tests/_treesites.tree_sites on the diagonal, and plain kriging covariance on a single-leaf tree.  No GPU.

Bounds are tests/test_sites_cpu.py's for the same truths: DENSE_TOL (1e-9 of the largest prior variance) against dense conditioning and
against the reference's Sigma, VAR_TOL (4e-13) against tree_sites' variance, -DENSE_TOL * scale * n for the smallest eigenvalue.
Seen when the formulas were first checked (40 off-row sites, 3 duplicates, 5 sites on rows): posterior against dense conditioning at most
2.2e-14, prior 2.2e-16, the diagonal against tree_sites 2.4e-16, smallest eigenvalue -2.1e-17."""
import functools
import os

import numpy as np
import pytest

import _cases as K
import _sampling as SM
import _treesitecov as TC
import _treesites as TS
import test_sites_cpu as SC

CASES = SC.CASES
DENSE_TOL, VAR_TOL = SC.DENSE_TOL, SC.VAR_TOL


def dense_sites(cs, seed=3):
    """40 sites off the rows (locate's rule), the first 3 of them again, and 5 of the tree's own rows in their own leaves"""
    topo, locs = cs["topo"], cs["locs"]
    off = SC.off_row_sites(locs, 40, seed=seed)
    rows = np.nonzero(SM.reported(topo))[0]
    pick = rows[np.unique(np.linspace(0, len(rows) - 1, 5).astype(int))]
    X = np.asarray(locs, float).reshape(topo.N, -1)
    sites = np.vstack([off, off[:3], X[topo.perm[pick]]])
    leaf = np.concatenate([SC.nearest_leaf(topo, locs, off), SC.nearest_leaf(topo, locs, off[:3]), SC.leaf_of_rows(topo)[pick]])
    return sites, leaf.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _dense(name):
    """(sites, leaf, prior truth, posterior truth, scale, the twin's prior, the twin's posterior), computed once and read-only"""
    cs, st = SC._state(name)
    topo, R = cs["topo"], float(cs["c"]["R"])
    sites, leaf = dense_sites(cs)
    rows = np.nonzero(SM.reported(topo))[0]
    Csr, Css = TS.site_prior_cov(st, sites, leaf)
    S = SM.golden_prior_sigma(name, topo)[np.ix_(rows, rows)]
    o = np.isfinite(np.asarray(cs["y_obs"], float).ravel())[topo.perm[rows]]
    L = np.linalg.cholesky(S[np.ix_(o, o)] + R * np.eye(int(o.sum())))
    T = np.linalg.solve(L, Csr[:, rows][:, o].T)
    scale = max(np.abs(np.diag(S)).max(), np.abs(np.diag(Css)).max())
    out = (sites, leaf, Css, Css - T.T @ T, scale, TC.tree_sites_cov(st, sites, leaf, False), TC.tree_sites_cov(st, sites, leaf, True))
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", CASES)
def test_twin_is_dense_conditioning_on_the_augmented_covariance(name):
    sites, leaf, want0, want1, scale, got0, got1 = _dense(name)
    e0, e1 = np.abs(got0 - want0).max(), np.abs(got1 - want1).max()
    print("%s: %d sites: prior err %.2e, posterior err %.2e (scale %.3f)" % (name, len(leaf), e0, e1, scale))
    assert e0 <= DENSE_TOL * scale
    assert e1 <= DENSE_TOL * scale


@pytest.mark.parametrize("name", CASES)
def test_twin_on_every_reported_row_is_the_references_sigma(name):
    cs, st = SC._state(name)
    topo = cs["topo"]
    rows = np.nonzero(SM.reported(topo))[0]
    X = np.asarray(cs["locs"], float).reshape(topo.N, -1)
    got = TC.tree_sites_cov(st, X[topo.perm[rows]], SC.leaf_of_rows(topo)[rows], False)
    S = SM.golden_prior_sigma(name, topo)[np.ix_(rows, rows)]
    scale = np.abs(np.diag(S)).max()
    err = np.abs(got - S).max()
    print("%s: %d own rows: prior err %.2e (scale %.3f)" % (name, len(rows), err, scale))
    assert err <= DENSE_TOL * scale


@pytest.mark.parametrize("name", CASES)
def test_twin_diagonal_symmetry_and_eigenvalues(name):
    cs, st = SC._state(name)
    sites, leaf, _, _, scale, got0, got1 = _dense(name)
    _, var = TS.tree_sites(cs["topo"], cs["locs"], cs["spec"], cs["y_obs"], float(cs["c"]["R"]), sites, leaf, state=st)
    e_d = np.abs(np.diag(got1) - var).max()
    ev0, ev1 = np.linalg.eigvalsh(got0).min(), np.linalg.eigvalsh(got1).min()
    print("%s: |diag - tree_sites var| %.2e, smallest eigenvalue prior %.2e, posterior %.2e" % (name, e_d, ev0, ev1))
    assert e_d <= VAR_TOL * scale
    assert np.array_equal(got0, got0.T) and np.array_equal(got1, got1.T)
    assert ev0 >= -DENSE_TOL * scale * len(leaf) and ev1 >= -DENSE_TOL * scale * len(leaf)


def test_a_single_leaf_is_plain_kriging_covariance():
    cs = K.load_case("kat1")
    topo, locs, spec, R = cs["topo"], cs["locs"], cs["spec"], float(cs["c"]["R"])
    assert topo.n_nodes == 1
    st = TS.SiteState(topo, locs, spec, cs["y_obs"], R)
    sites = SC.off_row_sites(locs, 40, seed=5)
    leaf = np.zeros(40, dtype=np.int32)
    X = np.asarray(locs, float).reshape(topo.N, -1)
    o = np.isfinite(np.asarray(cs["y_obs"], float).ravel())
    Css = np.asarray(spec.evaluate(sites, sites))
    Cso = np.asarray(spec.evaluate(sites, X[o]))
    Koo = np.asarray(spec.evaluate(X[o], X[o])) + R * np.eye(int(o.sum()))
    want = Css - Cso @ np.linalg.solve(Koo, Cso.T)
    e0 = np.abs(TC.tree_sites_cov(st, sites, leaf, False) - Css).max()
    e1 = np.abs(TC.tree_sites_cov(st, sites, leaf, True) - want).max()
    print("M = 0: prior err %.2e, posterior err %.2e" % (e0, e1))
    assert e0 <= DENSE_TOL * np.abs(Css).max() and e1 <= DENSE_TOL * np.abs(Css).max()


def test_sitecov_surface_is_exported():
    from pymra_amd import plan
    from pymra_amd.MRATree import MRATree
    assert "mra_sites_cov" in plan.EXPORTS
    assert callable(plan.HipPlan.sites_cov) and callable(MRATree.covarianceAt) and callable(MRATree.simulateAt)
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    assert "int mra_sites_cov(mra_plan *plan, uint32_t flags, int64_t n_sites, const double *sites, const int32_t *leaf, double *out);" in hdr
    assert "#define MRA_SITES_COV_MAX 16384" in hdr and plan.MRA_SITES_COV_MAX == 16384
