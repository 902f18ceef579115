"""The NumPy restatement of mra_sample_sites (tests/_treesitedraw.py) against the restatement of mra_sites_cov
(tests/_treesitecov.py, itself pinned to dense conditioning by tests/test_sitecov_cpu.py): F F^T is the joint covariance, prior and
posterior; the inert sites are exactly the sites on ancestors' knots; duplicated sites have equal rows; every leaf block factors.
And the exported surface of the feature.  No GPU.

The bound is tests/test_sites_cpu.py's DENSE_TOL (1e-9 of the largest prior variance).  Seen when the factorisation was first
checked (g32, c1, kat3, u3; 40 off-row sites, 3 duplicates, 5 sites on rows; and 40 off-row sites plus every reported row):
|F F^T - tree_sites_cov| at most 1.4e-14 of the scale; |G_uu| / C(s, s) at most 4.4e-16 at sites on ancestors' knots; the smallest
genuine relative diagonal 1.4e-8 and the smallest relative pivot 1.4e-9 (c1)."""
import os

import numpy as np
import pytest

import _cases as K
import _sampling as SM
import _treesitecov as TC
import _treesitedraw as TD
import test_sitecov_cpu as CC
import test_sites_cpu as SC

CASES = ["g32", "c1", "kat3", "u3"]
DENSE_TOL = SC.DENSE_TOL


def rows_and_off_sites(cs, seed=3):
    """the case's 40 off-row sites plus every reported row, each row in its own leaf -> (sites, leaf, padded row of a site or -1)"""
    topo, locs = cs["topo"], cs["locs"]
    off = SC.off_row_sites(locs, 40, seed=seed)
    rows = np.nonzero(SM.reported(topo))[0]
    X = np.asarray(locs, float).reshape(topo.N, -1)
    sites = np.vstack([off, X[topo.perm[rows]]])
    leaf = np.concatenate([SC.nearest_leaf(topo, locs, off), SC.leaf_of_rows(topo)[rows]]).astype(np.int32)
    return sites, leaf, np.concatenate([np.full(len(off), -1), rows])


def ancestor_knot_rows(topo):
    """padded rows that are a knot of a non-leaf node"""
    out = set()
    for j in range(topo.n_nodes):
        if not topo.node_leaf[j]:
            out.update(int(r) for r in topo.knot_rows[topo.knot_ptr[j]:topo.knot_ptr[j + 1]])
    return out


def _check(name, st, sites, leaf, tag):
    scale = None
    for post in (False, True):
        info = {}
        F, cols = TD.site_draw_factor(st, sites, leaf, post, info)      # numpy.linalg.cholesky raises when a leaf block does not factor
        assert F.shape == (len(leaf), info["Kn"] + len(leaf)) and np.array_equal(cols, np.arange(F.shape[1]))
        want = TC.tree_sites_cov(st, sites, leaf, post)
        scale = np.abs(np.diag(TC.tree_sites_cov(st, sites, leaf, False))).max() if scale is None else scale
        err = np.abs(F @ F.T - want).max()
        print("%s %s: %d sites, %s: |F F^T - tree_sites_cov| %.2e of the scale %.3f, %d inert, smallest relative pivot %.2e"
              % (name, tag, len(leaf), "posterior" if post else "prior", err / scale, scale, int(info["inert"].sum()), info["min_pivot"]))
        assert err <= DENSE_TOL * scale
        first = info["first"]
        assert np.array_equal(F, F[first])                               # duplicated sites have equal rows
        yield post, info


@pytest.mark.parametrize("name", CASES)
def test_twin_factor_on_the_dense_sites(name):
    cs, st = SC._state(name)
    sites, leaf = CC.dense_sites(cs)
    for post, info in _check(name, st, sites, leaf, "dense_sites"):
        assert (info["first"] != np.arange(len(leaf))).sum() == 3
        assert not info["inert"][:43].any()                              # sites off the rows have a leaf term


@pytest.mark.parametrize("name", CASES)
def test_twin_factor_on_every_reported_row_and_inert_sites_are_the_ancestor_knots(name):
    cs, st = SC._state(name)
    topo = cs["topo"]
    sites, leaf, row = rows_and_off_sites(cs)
    knots = ancestor_knot_rows(topo)
    on_knot = np.array([int(r) in knots for r in row])
    for post, info in _check(name, st, sites, leaf, "rows + 40"):
        dup = info["first"] != np.arange(len(leaf))
        want = on_knot.copy()
        want[dup] = on_knot[info["first"][dup]]                          # two rows at one location in one leaf share the first one's draw
        assert np.array_equal(info["inert"], want)
        assert info["min_pivot"] > TD.INERT_REL                           # the genuine pivots lie above the threshold, the knots' diagonals below


def test_sitedraw_surface_is_exported():
    from pymra_amd import plan
    from pymra_amd.MRATree import MRATree
    assert "mra_sample_sites" in plan.EXPORTS and "mra_sample_sites_slots" in plan.EXPORTS
    assert plan.MRA_SAMPLE_SITES_LEAF_MAX == 4096
    assert callable(plan.HipPlan.sample_sites) and callable(plan.HipPlan.sample_sites_slots) and callable(MRATree.sampleAt)
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    assert "#define MRA_SAMPLE_SITES_LEAF_MAX 4096" in hdr
    assert "int mra_sample_sites_slots(mra_plan *plan, int64_t n_sites, int64_t *n_slots);" in hdr
    assert ("int mra_sample_sites(mra_plan *plan, uint32_t flags, int64_t n_sites, const double *sites, const int32_t *leaf,\n"
            "                     int64_t n_samples, uint64_t seed, int64_t sample0, const double *z, double *out);") in hdr
