"""The NumPy restatement of mra_cov_apply (tests/_treecov.py) against truths that do not share its algebra: the MRA prior covariance
assembled from the reference's own per-node B and kC (tests/golden/*_nodes.npz), the faithful oracle's prior_sigma_rows where no
node goldens exist (t201), and dense Gaussian conditioning of that Sigma on the case's mask and R.  No GPU.  Bounds: those
tests/test_solve_cpu.py uses between float64 restatements (1e-9), absolute and scaled by the largest prior variance, because
Sigma_post A is a difference of two terms of that size."""
import functools
import os

import numpy as np
import pytest

import _cases as K
import _sampling as SM
import _treecov as TC

CASES = ["g32", "c1", "kat3", "u3", "t201"]        # 2-D grids, 1-D trees (kat3, t201), phantom knot columns (u3)
TOL = 1e-9


@functools.lru_cache(maxsize=None)
def _truth(name):
    """(case, rep, Sigma[rep, rep], Sigma_post[rep, rep]) - computed once per case and never written to."""
    cs = K.load_case(name)
    topo = cs["topo"]
    rep = SM.reported(topo)
    rows = np.nonzero(rep)[0]
    if name == "t201":
        from oracle.mra_faithful import prior_sigma_rows
        S = prior_sigma_rows(topo, cs["locs"], cs["spec"].evaluate, rows)
    else:
        S = SM.golden_prior_sigma(name, topo)[np.ix_(rows, rows)]
    o = np.isfinite(np.asarray(cs["y_obs"], float).ravel())[topo.perm[rows]]
    R = float(cs["c"]["R"])
    L = np.linalg.cholesky(S[np.ix_(o, o)] + R * np.eye(int(o.sum())))
    T = np.linalg.solve(L, S[o, :])
    Sp = S - T.T @ T
    S.setflags(write=False)
    Sp.setflags(write=False)
    return cs, rep, S, Sp


def _columns(topo, c, seed):
    """(N, c + units): c random columns, then unit vectors at a root knot row, a leaf knot row and the first and last reported rows."""
    rep = SM.reported(topo)
    A = np.random.default_rng(seed).standard_normal((topo.N, c))
    leaves = np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]
    lk = [int(r) for i in leaves for r in topo.knot_rows[topo.knot_ptr[i]:topo.knot_ptr[i + 1]] if rep[r]]
    picks = [int(topo.knot_rows[topo.knot_ptr[0]]), lk[len(lk) // 2], int(np.nonzero(rep)[0][0]), int(np.nonzero(rep)[0][-1])]
    U = np.zeros((topo.N, len(picks)))
    U[topo.perm[picks], np.arange(len(picks))] = 1.0
    return np.hstack([A, U])


@pytest.mark.parametrize("c", [1, 3, 16])
@pytest.mark.parametrize("name", CASES)
def test_restated_cov_matches_the_reference_sigma_and_dense_conditioning(name, c):
    cs, rep, S, Sp = _truth(name)
    topo, locs, spec, R = cs["topo"], cs["locs"], cs["spec"], float(cs["c"]["R"])
    rows = np.nonzero(rep)[0]
    A = _columns(topo, c, seed=c)
    Ar = A[topo.perm[rows]]
    scale = np.abs(np.diag(S)).max()
    for post, truth in ((False, S), (True, Sp)):
        out, gram = TC.tree_cov(topo, locs, spec, cs["y_obs"], R, A, posterior=post)
        assert out.shape == A.shape and gram.shape == (A.shape[1],) * 2
        want = truth @ Ar
        e_o = np.abs(out[topo.perm[rows]] - want).max()
        e_g = np.abs(gram - Ar.T @ want).max()
        print("%s c=%d %s: out err %.2e, gram err %.2e (largest prior variance %.3f)" % (name, c, "posterior" if post else "prior", e_o, e_g, scale))
        assert e_o <= TOL * scale
        assert e_g <= TOL * scale
        outside = np.ones(topo.N, dtype=bool)
        outside[topo.perm[rows]] = False
        assert np.all(out[outside] == 0.0)


def test_cov_surface_is_exported():
    from pymra_amd import plan
    from pymra_amd.MRATree import MRATree
    assert "mra_cov_apply" in plan.EXPORTS and plan.MRA_COV_POSTERIOR == 1
    assert callable(plan.HipPlan.cov_apply) and callable(MRATree.covariance) and callable(MRATree.functionalCovariance)
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    assert "int mra_cov_apply(mra_plan *plan, uint32_t flags, int64_t n_cols, const double *A, double *out, double *gram);" in hdr
    assert "#define MRA_COV_POSTERIOR 1u" in hdr
