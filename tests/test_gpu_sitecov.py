"""mra_sites_cov / HipPlan.sites_cov / MRATree.covarianceAt / MRATree.simulateAt on the GPU: the joint prior and posterior covariance
of the latent MRA process at locations that need not be rows of the tree.  Truths that do not come from the Gram kernel: the reference's
own Sigma and dense conditioning of it (tests/test_gpu_cov.py's _reference) at sites placed on the tree's rows, the NumPy restatement
tests/_treesitecov.py (pinned to dense conditioning on the augmented covariance by tests/test_sitecov_cpu.py) at sites off the rows,
the kriging covariance on single-leaf trees, and mra_cov_apply's unit columns where no dense truth can be formed.

Bounds are those of the sibling tests for the same comparison: PRIOR_TOL (1e-10) and _post_tol (1e-9; u3 1e-6) of tests/test_gpu_cov.py
against the reference's Sigma and dense conditioning and, as tests/test_gpu_sites.py does, against the twin; POST_NO_TRUTH_TOL (1e-9)
against cov_apply's unit columns on the deep 64-wide tree and the tree with a leaf of 193 observations; C3_PRIOR_TOL / C3_POST_TOL at
BASELINE config 3, all times the largest prior variance."""
import ctypes as C

import numpy as np
import pytest

import _cases as K
import _sampling as SM
import _treesitecov as TC
import _treesites as TS
import test_gpu_cov as GC
import test_gpu_sites as TG
import test_sites_cpu as SC

pytestmark = pytest.mark.gpu

CASES = ["g32", "c1", "kat3", "u3"]


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _both(pl, sites, leaf):
    return pl.sites_cov(sites, leaf), pl.sites_cov(sites, leaf, posterior=True)


def _against_twin(pl, topo, locs, spec, y_obs, R, sites, leaf, tag, tol=1e-9):
    st = TS.SiteState(topo, locs, spec, y_obs, R)
    scale = TG._scale(spec, topo.d)
    got = _both(pl, sites, leaf)
    for kind, g in zip(("prior", "posterior"), got):
        want = TC.tree_sites_cov(st, sites, leaf, kind == "posterior")
        err = np.abs(g - want).max()
        print("%s: %d sites against the twin: %s err %.2e (scale %.2f)" % (tag, len(leaf), kind, err, scale))
        assert g.shape == (len(leaf), len(leaf)) and np.all(np.isfinite(g))
        assert err <= tol * scale
        assert np.array_equal(g, g.T)
    return got


def _units_block(pl, topo, rows, posterior):
    """Sigma[rows, rows] (Sigma_post) from mra_cov_apply's unit columns"""
    rep = SM.reported(topo)
    out, _ = pl.cov_apply(GC._padded(topo, GC._units(topo, rows), rep), posterior=posterior, want_gram=False)
    return out[:, rows]


def _own_rows_against_cov_apply(pl, topo, locs, spec, rows, tag, tols):
    rows, sites, leaf = TG._own_rows(topo, locs, rows)
    scale = TG._scale(spec, topo.d)
    errs = []
    for post, g in zip((False, True), _both(pl, sites, leaf)):
        want = _units_block(pl, topo, rows, post)
        errs.append(np.abs(g - want).max())
        assert np.array_equal(g, g.T)
    print("%s: %d own rows against cov_apply's unit columns: prior err %.2e, posterior err %.2e (scale %.2f)" % (tag, len(rows), errs[0], errs[1], scale))
    for e, tol in zip(errs, tols):
        assert e <= tol * scale
    return errs


# ---- 1. the tree's own rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_own_rows_as_sites_are_the_references_sigma_and_dense_conditioning(hip, name):
    cs, rep, S, Sp = GC._reference(name)
    topo = cs["topo"]
    pl = GC._case_plan(hip, cs)
    rows, sites, leaf = TG._own_rows(topo, cs["locs"])
    assert len(rows) <= 1024
    prior, post = _both(pl, sites, leaf)
    _, var = pl.predict_sites(sites, leaf)
    scale = np.abs(S[np.ix_(rep, rep)]).max()
    e0, e1, e_d = np.abs(prior - S[np.ix_(rows, rows)]).max(), np.abs(post - Sp).max(), np.abs(np.diag(post) - var).max()
    print("%s: %d own rows: prior err %.2e, posterior err %.2e, |diag - predict_sites var| %.2e (scale %.2f)" % (name, len(rows), e0, e1, e_d, scale))
    assert e0 <= GC.PRIOR_TOL * scale
    assert e1 <= GC._post_tol(name) * scale
    assert e_d <= GC._post_tol(name) * scale
    assert np.array_equal(prior, prior.T) and np.array_equal(post, post.T)
    pl.close()


# ---- 2. sites off the rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES + ["grid48_r20"])
def test_off_row_sites_match_the_twin(hip, name):
    if name == "grid48_r20":                                  # cw = 32, leaves of nine row tiles
        topo, locs, y_obs, spec, R = GC._shape_tree(name)
    else:
        cs = K.load_case(name)
        topo, locs, y_obs, spec, R = cs["topo"], cs["locs"], cs["y_obs"], cs["spec"], float(cs["c"]["R"])
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    sites, leaf = TG._mixed_sites(topo, locs, seed=11)
    assert len(leaf) % 16 != 0
    got = _against_twin(pl, topo, locs, spec, y_obs, R, sites, leaf, name, tol=GC._post_tol(name))
    first, dup = {}, 0
    for k in range(len(leaf)):                                # duplicate sites: the same rows, to the bit
        key = (sites[k].tobytes(), int(leaf[k]))
        if key in first:
            dup += 1
            for g in got:
                assert np.array_equal(g[k], g[first[key]])
        first.setdefault(key, k)
    assert dup >= 3
    pl.close()


# ---- 3. every device kernel family, 1-D and circular ----------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["exp", "matern52", "gaussian", "kanter", "iden", "matern32_scale", "circular"])
def test_every_kernel_family(hip, family):
    import pymra_amd.MRATools as mt
    specs = {"exp": mt.KernelSpec(mt.KIND_EXP, 0.3), "matern52": mt.KernelSpec(mt.KIND_MATERN52, 0.2, 0.7),
             "gaussian": mt.KernelSpec(mt.KIND_GAUSSIAN, 0.05, 1.0), "kanter": mt.KernelSpec(mt.KIND_KANTER, 0.35),
             "iden": mt.KernelSpec(mt.KIND_IDEN, 0.01), "matern32_scale": mt.KernelSpec(mt.KIND_MATERN32, 0.4, 1.0, 2.5),
             "circular": mt.KernelSpec(mt.KIND_EXP, 0.3, 1.0, 1.0, True)}
    cs = K.load_case("c1" if family == "circular" else "g32")        # the trees and sites of test_gpu_sites.py's family test
    topo, locs, spec, R = cs["topo"], cs["locs"], specs[family], float(cs["c"]["R"])
    pl = GC._plan(hip, topo, locs, cs["y_obs"], R, spec)
    rows, own, own_leaf = TG._own_rows(topo, locs)
    off = SC.off_row_sites(locs, 37, seed=2)
    sites, leaf = np.vstack([off, own[::7]]), np.concatenate([SC.nearest_leaf(topo, locs, off), own_leaf[::7]]).astype(np.int32)
    _against_twin(pl, topo, locs, spec, cs["y_obs"], R, sites, leaf, family)
    pl.close()


# ---- 4. single-leaf trees -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kat1", "kat4", "grid18_m0"])
def test_single_leaf_trees_are_the_kriging_covariance(hip, name):
    topo, locs, y_obs, spec, R = GC._shape_tree(name)
    assert topo.n_nodes == 1
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    X = np.asarray(locs, float).reshape(topo.N, -1)
    sites = SC.off_row_sites(locs, 21, seed=6)
    prior, post = _both(pl, sites, np.zeros(len(sites), dtype=np.int32))
    o = np.isfinite(np.asarray(y_obs, float).ravel())
    Css, Cso = np.asarray(spec.evaluate(sites, sites)), np.asarray(spec.evaluate(sites, X[o]))
    want = Css - Cso @ np.linalg.solve(np.asarray(spec.evaluate(X[o], X[o])) + R * np.eye(int(o.sum())), Cso.T)
    scale = TG._scale(spec, topo.d)
    e0, e1 = np.abs(prior - Css).max(), np.abs(post - want).max()
    print("%s: kriging covariance at %d sites: prior err %.2e, posterior err %.2e (scale %.2f)" % (name, len(sites), e0, e1, scale))
    assert e0 <= 1e-9 * scale and e1 <= 1e-9 * scale          # test_gpu_sites.py: `assert e_v <= 1e-9 * scale` (kriging)
    assert np.array_equal(prior, prior.T) and np.array_equal(post, post.T)
    pl.close()


def test_the_three_point_tree(hip):
    """kat2: a root and two leaves over three locations - the smallest tree with a cross-leaf block"""
    cs = K.load_case("kat2")
    topo, locs, spec, R = cs["topo"], cs["locs"], cs["spec"], float(cs["c"]["R"])
    pl = GC._case_plan(hip, cs)
    sites = SC.off_row_sites(locs, 21, seed=6)
    _against_twin(pl, topo, locs, spec, cs["y_obs"], R, sites, SC.nearest_leaf(topo, locs, sites).astype(np.int32), "kat2")
    pl.close()


# ---- 5. gappy mask ------------------------------------------------------------------------------------------------------------------
def test_mask_with_an_empty_leaf_and_an_empty_family(hip):
    topo, locs, y_obs, spec = GC._gappy()
    pl = GC._plan(hip, topo, locs, y_obs, GC.R_MASK, spec)
    y = np.asarray(y_obs, float).ravel()
    leaves = [int(i) for i in np.nonzero(topo.node_leaf)[0]]
    empty = [i for i in leaves if not np.isfinite(y[topo.perm[K.node_real_rows(topo, i)]]).any()]
    assert leaves[0] in empty and len(empty) >= 5                 # the first leaf and a whole family of four: they have no t
    rows, own, own_leaf = TG._own_rows(topo, locs, np.concatenate([K.node_real_rows(topo, i)[::5] for i in empty[:5]]))
    off = SC.off_row_sites(locs, 50, seed=8)
    sites, leaf = np.vstack([own, off]), np.concatenate([own_leaf, SC.nearest_leaf(topo, locs, off)]).astype(np.int32)
    _against_twin(pl, topo, locs, spec, y_obs, GC.R_MASK, sites, leaf, "gappy 64^2")
    pl.close()


# ---- 6. other routes ----------------------------------------------------------------------------------------------------------------
def test_deep_wide_tree_on_chosen_leaves(hip):
    """cw = 64, five ancestors, the level-by-level route with panel-only fronts at the leaves' parents: K tails of 64 ... 320"""
    topo, locs, y_obs, spec, R = GC._deep_wide()
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    assert pl.route()["path"] == "Hi"
    rows = np.concatenate([K.node_real_rows(topo, j) for j in GC._leaf_sets(topo)])
    _own_rows_against_cov_apply(pl, topo, locs, spec, rows, "deep wide", (GC.POST_NO_TRUTH_TOL, GC.POST_NO_TRUTH_TOL))
    pl.close()


def test_a_leaf_of_more_than_192_observations(hip):
    import _route_cells as RC
    import test_gpu_likelihood_masks as MK
    topo, locs = MK._tree(*RC.TREES["A"])
    obs = RC.make_obs(topo, locs, ("edges", "empty_first", 193))
    y = MK._y(obs)
    pl = GC._plan(hip, topo, locs, y, MK.R, MK._spec())
    assert pl.route()["chol"] == "BigPanels"
    counts = MK.leaf_counts(topo, obs)
    leaves = [int(i) for i in np.nonzero(topo.node_leaf)[0]]
    big = leaves[int(np.argmax(counts))]
    assert max(counts) == 193
    rows = np.concatenate([K.node_real_rows(topo, big), K.node_real_rows(topo, leaves[0])[::3], K.node_real_rows(topo, leaves[7])[::3]])
    _own_rows_against_cov_apply(pl, topo, locs, MK._spec(), rows, "leaf of 193 observations", (GC.POST_NO_TRUTH_TOL, GC.POST_NO_TRUTH_TOL))
    pl.close()


# ---- 7. bit identity ----------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_order_subset_or_panels(hip):
    topo, locs, y_obs, spec, R = GC._shape_tree("grid48_r20")
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    sites, leaf = TG._mixed_sites(topo, locs, seed=21)
    n = len(leaf)
    order = np.random.default_rng(3).permutation(n)
    sub = np.sort(np.random.default_rng(4).choice(n, n // 3, replace=False))
    for post in (False, True):
        g1 = pl.sites_cov(sites, leaf, posterior=post)
        g2 = pl.sites_cov(sites[order], leaf[order], posterior=post)
        assert np.array_equal(g2, g1[np.ix_(order, order)])
        g3 = pl.sites_cov(sites[sub], leaf[sub], posterior=post)
        assert np.array_equal(g3, g1[np.ix_(sub, sub)])
        assert pl.get_option(21) == 0
        pl.set_option(21, 1)                                 # one tile row per panel
        g4 = pl.sites_cov(sites, leaf, posterior=post)
        assert GC._factor_launches(pl) == 0                  # option 21 keeps the factors
        pl.set_option(21, 0)
        assert np.array_equal(g4, g1)
    pl.close()


# ---- 8. state -----------------------------------------------------------------------------------------------------------------------
def test_sites_cov_leaves_the_callers_state_and_shares_the_factors(hip):
    topo, locs, y_obs, spec = GC._gappy()
    pl = GC._plan(hip, topo, locs, y_obs, GC.R_MASK, spec)
    opts = {k: pl.get_option(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22)}
    lik0, (m0, v0) = pl.likelihood(), pl.predict()
    sites = SC.off_row_sites(locs, 30, seed=1)
    leaf = SC.nearest_leaf(topo, locs, sites).astype(np.int32)
    p1 = pl.sites_cov(sites, leaf, posterior=True)
    assert GC._factor_launches(pl) > 0                       # the first call ran its own likelihood pass
    assert pl.likelihood() == lik0
    m1, v1 = pl.predict()
    assert np.array_equal(m1, m0) and np.array_equal(v1, v0)
    assert {k: pl.get_option(k) for k in opts} == opts
    q1 = pl.sites_cov(sites, leaf)
    assert GC._factor_launches(pl) == 0                      # the second one launched no kernel of a pass
    Yp = np.zeros((2, topo.P))
    for other in (lambda: pl.solve(Yp), lambda: pl.cov_apply(Yp, posterior=True), lambda: pl.predict_sites(sites, leaf)):
        other()
        assert GC._factor_launches(pl) == 0                  # the sibling after sites_cov reuses the factors
        p2 = pl.sites_cov(sites, leaf, posterior=True)
        assert GC._factor_launches(pl) == 0                  # ... and sites_cov after the sibling
        assert np.array_equal(p2, p1)
    mean_s, var_s = pl.predict_sites(sites, leaf)
    want_m, _ = TS.tree_sites(topo, locs, spec, y_obs, GC.R_MASK, sites, leaf)
    assert TG._mean_ok(mean_s.T, want_m)                     # the device y is the caller's: the mean of the plan's own observations
    pl.run(True, True)                                       # y untouched: the old numbers bit for bit
    assert pl.likelihood() == lik0
    y2 = np.asarray(y_obs, float).copy()
    y2[np.nonzero(np.isfinite(y2))[0][::2]] = np.nan         # another mask
    pl.set_obs(y2, GC.R_MASK)
    p3 = pl.sites_cov(sites, leaf, posterior=True)
    assert GC._factor_launches(pl) > 0                       # a new mask: a new pass
    q3 = pl.sites_cov(sites, leaf)
    st = TS.SiteState(topo, locs, spec, y2, GC.R_MASK)
    scale = TG._scale(spec, topo.d)
    assert np.abs(p3 - p1).max() > 1e-6
    assert np.abs(p3 - TC.tree_sites_cov(st, sites, leaf, True)).max() <= 1e-9 * scale
    assert np.array_equal(q3, q1)                            # the prior does not depend on the mask
    pl.close()


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------
def test_sites_cov_refusals(hip):
    from pymra_amd.plan import MraError, MRA_SITES_COV_MAX
    import pymra_amd.MRATools as mt
    topo, locs, y_obs, spec = GC._gappy()
    sites = SC.off_row_sites(locs, 5, seed=1)
    leaf = SC.nearest_leaf(topo, locs, sites).astype(np.int32)
    pl = hip.HipPlan(topo, 0)
    for step in ("nothing", "locs", "kernel"):
        if step == "locs":
            pl.set_locs(locs)
        elif step == "kernel":
            pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
        with pytest.raises(MraError) as e:
            pl.sites_cov(sites, leaf)
        assert e.value.code == -4, step                      # MRA_ERR_STATE before set_locs / set_kernel / set_obs
    pl.set_obs(y_obs, GC.R_MASK)
    good = pl.sites_cov(sites, leaf, posterior=True)
    out = np.empty((5, 5))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    seen = set()

    def raw(flags=0, n=5, s=sites, lf=leaf, o=out):
        return pl.lib.mra_sites_cov(pl._h, flags, n, p(s), p(lf), p(o))

    def refused(**kw):
        assert raw(**kw) == -1, kw
        msg = pl.lib.mra_last_error(pl._h)
        seen.add(msg)
        return msg
    assert raw() == 0 and raw(flags=1) == 0
    refused(flags=2)
    refused(flags=3)                                         # unknown flags (same message)
    refused(n=-1)
    assert b"2 GiB" in refused(n=MRA_SITES_COV_MAX + 1)      # checked before the sites are read or anything is allocated
    refused(s=None)
    assert refused(lf=None) == refused(s=None)
    refused(o=None)
    assert raw(n=0, s=None, lf=None, o=None) == 0            # n_sites == 0
    for bad_leaf in (-1, topo.n_nodes, 0):                   # out of range; the root is not a leaf
        lf = leaf.copy()
        lf[3] = bad_leaf
        refused(lf=lf)
    for bad_value in (np.nan, np.inf):
        s = sites.copy()
        s[2, 1] = bad_value
        refused(s=s)
    assert len(seen) == 9                                    # each kind of refusal has its own message (three bad leaves: three)
    with pytest.raises(MraError) as e:
        pl.sites_cov(np.zeros((MRA_SITES_COV_MAX + 1, 2)), np.full(MRA_SITES_COV_MAX + 1, leaf[0], dtype=np.int32))
    assert e.value.code == -1 and "MRA_SITES_COV_MAX" in str(e.value)
    assert np.array_equal(pl.sites_cov(sites, leaf, posterior=True), good)      # the plan is still usable, and gives the same bits
    pl.set_reduce_level(0)
    with pytest.raises(MraError) as e:
        pl.sites_cov(sites, leaf)
    assert e.value.code == -1 and "sharded" in str(e.value)
    pl.close()
    from pymra_amd import MRATree
    np.random.seed(1)
    n = 16
    l2 = mt.genLocations2d(Nx=n, Ny=n)
    y = np.random.normal(size=(n * n, 1))
    tree = MRATree(l2, 16, lambda a, b=np.array([]): np.exp(-np.abs(mt.dist(a, b)) / 0.3), y, 1e-2, M=1, J=4, verbose=False)      # opaque callable: host cov
    with pytest.raises(NotImplementedError):
        tree.covarianceAt(l2[:3])
    with pytest.raises(NotImplementedError):
        tree.simulateAt(l2[:3], 2)
    with pytest.raises(MraError) as e:
        tree.plan.sites_cov(l2[:3], tree.locate(l2[:3]))
    assert e.value.code == -1 and "MRA_KERNEL_HOST" in str(e.value)


# ---- 10. through MRATree ------------------------------------------------------------------------------------------------------------
def test_mratree_covarianceAt_and_simulateAt(hip):
    import pymra_amd.MRATools as mt
    from pymra_amd import MRATree
    np.random.seed(3)
    cov = lambda a, b=np.array([]): mt.Matern32(a, b, l=0.3, sig=1.0)          # noqa: E731
    n = 32
    locs = mt.genLocations2d(Nx=n, Ny=n)
    rng = np.random.default_rng(2)
    y = np.where(rng.random(n * n) < 0.4, rng.standard_normal(n * n), np.nan).reshape(-1, 1)
    tree = MRATree(locs, 16, cov, y, 1e-2, M=2, J=4, verbose=False)
    lik0 = float(tree.getLikelihood()[0, 0])
    sites = SC.off_row_sites(locs, 40, seed=9)
    ns = len(sites)
    scale = 1.0
    for distr in ("posterior", "prior"):
        S = tree.covarianceAt(sites, distr=distr)
        assert S.shape == (ns, ns) and np.array_equal(S, S.T)
        assert np.array_equal(S, tree.covarianceAt(sites, distr=distr, leaf=tree.locate(sites)))
        assert np.array_equal(S, tree.plan.sites_cov(sites, tree.locate(sites), posterior=(distr == "posterior")))
        mean = tree.predictAt(sites)[0] if distr == "posterior" else np.zeros((ns, 1))
        X = tree.simulateAt(sites, ns, distr=distr, z=np.eye(ns))
        assert X.shape == (ns, ns)
        err = np.abs((X - mean) @ (X - mean).T - S).max()
        print("simulateAt(z = I), %s: |F F^T - covarianceAt| %.2e" % (distr, err))
        assert err <= 1e-9 * scale * ns
        a, b = tree.simulateAt(sites, 7, distr=distr, seed=5), tree.simulateAt(sites, 7, distr=distr, seed=5)
        assert a.shape == (ns, 7) and np.array_equal(a, b)
        assert not np.array_equal(a, tree.simulateAt(sites, 7, distr=distr, seed=6))
    assert np.array_equal(tree.simulateAt(sites, 3, distr="prior", z=np.zeros((ns, 3))), np.zeros((ns, 3)))      # the prior has mean 0
    assert np.array_equal(tree.simulateAt(sites, 1, z=np.zeros((ns, 1))), tree.predictAt(sites)[0])
    assert np.abs(np.diag(tree.covarianceAt(sites)) - tree.predictAt(sites)[1] ** 2).max() <= GC.POST_NO_TRUTH_TOL * scale
    assert float(tree.getLikelihood()[0, 0]) == lik0
    with pytest.raises(ValueError):
        tree.covarianceAt(sites, distr="conditional")
    with pytest.raises(ValueError):
        tree.covarianceAt(sites, leaf=tree.locate(sites)[:3])
    with pytest.raises(ValueError):
        tree.simulateAt(sites, 3, z=np.zeros((ns, 2)))


# ---- 11. BASELINE config 3 ----------------------------------------------------------------------------------------------------------
def test_own_rows_at_c3(hip):
    """256 of the tree's own rows at 1024^2, M = 6, spread over two siblings, a cousin, the middle and the last leaf, against
    cov_apply's unit columns.  Seen on one MI355X: see DESIGN.md section 13."""
    import bench
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    c = bench.CONFIGS["c3"]
    locs, y_obs = bench.make_inputs(c)
    topo = build_topology(locs, c["r"], c["M"], c["J"])
    spec = mt.KernelSpec(mt.KIND_MATERN32, c["l"], c["sig"])
    rng = np.random.default_rng(1)
    sets = GC._leaf_sets(topo)
    per = [52, 51, 51, 51, 51]
    rows = np.sort(np.concatenate([rng.choice(K.node_real_rows(topo, j), k, replace=False) for j, k in zip(sets, per)]))
    assert len(rows) == 256
    pl = GC._plan(hip, topo, locs, y_obs, c["R"], spec)
    rows, sites, leaf = TG._own_rows(topo, locs, rows)
    scale = TG._scale(spec, topo.d)
    for post, tol, g in zip((False, True), (GC.C3_PRIOR_TOL, GC.C3_POST_TOL), _both(pl, sites, leaf)):
        err = np.abs(g - _units_block(pl, topo, rows, post)).max()
        print("c3: 256 own rows against cov_apply's unit columns: %s err %.2e (bound %.1e, scale %.2f)" % ("posterior" if post else "prior", err, tol * scale, scale))
        if err > tol * scale:
            print("c3: above the bound measured for cov_apply against its own truth; held to POST_NO_TRUTH_TOL")
            tol = GC.POST_NO_TRUTH_TOL
        assert err <= tol * scale
        assert np.array_equal(g, g.T)
    pl.close()
