"""mra_predict_sites / HipPlan.predict_sites / MRATree.locate / MRATree.predictAt on the GPU: the posterior mean and variance of the MRA
process at locations that need not be rows of the tree.  Truths that do not come from the site kernels: the plan's own predict() at
sites placed on tree rows, dense conditioning of the reference's Sigma (tests/golden/*_nodes.npz) for the variance there, the NumPy
restatement tests/_treesites.py (pinned to the oracle and to dense conditioning by tests/test_sites_cpu.py) at sites off the rows,
exact kriging on single-leaf trees, and solve()'s columns for a block Y.

Bounds are those of the assertion that makes the same kind of comparison elsewhere in the suite:
  * MEAN: tests/test_gpu_solve.py holds solve()'s mean to the pass's mean within `1e-8 * max(1.0, np.abs(m).max())`;
  * VAR: tests/test_gpu_cov.py / tests/test_gpu_sample.py hold dense conditioning to `tol * scale` with
    `tol = 1e-6 if name == "u3" else 1e-9` and scale the largest prior variance; where no dense truth can be formed (the deep 64-wide
    tree, the tree with a leaf of 193 observations, the tree behind MRATree, BASELINE config 3) the variance is held to predict()'s
    within the same 1e-9 of the scale, as tests/test_gpu_cov.py does (POST_NO_TRUTH_TOL)."""
import ctypes as C

import numpy as np
import pytest

import _cases as K
import _sampling as SM
import _treesites as TS
import test_gpu_cov as GC
import test_sites_cpu as SC

pytestmark = pytest.mark.gpu

CASES = ["g32", "c1", "kat3", "u3"]
NO_TRUTH_TOL = GC.POST_NO_TRUTH_TOL


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _mean_ok(got, want):
    return np.abs(got - want).max() <= 1e-8 * max(1.0, np.abs(want).max())      # test_gpu_solve.py's bound, see the module docstring


def _own_rows(topo, locs, rows=None):
    """(padded rows, their locations, their own leaves): every reported row unless `rows` is given"""
    rows = np.nonzero(SM.reported(topo))[0] if rows is None else np.asarray(rows)
    X = np.asarray(locs, float).reshape(topo.N, -1)
    return rows, X[topo.perm[rows]], SC.leaf_of_rows(topo)[rows]


def _scale(spec, d):
    z = np.zeros((1, d))
    return float(np.asarray(spec.evaluate(z, z))[0, 0])


def _mixed_sites(topo, locs, seed):
    """Sites off the rows with locate's rule, then four leaves given exactly 0, 1, 16 and 17 sites (jittered copies of their own
    locations, assigned explicitly), three duplicates, and a total that is no multiple of 16."""
    rng = np.random.default_rng(seed)
    X = np.asarray(locs, float).reshape(topo.N, -1)
    span = X.max(0) - X.min(0)
    sites = SC.off_row_sites(locs, 45, seed)
    leaf = SC.nearest_leaf(topo, locs, sites)
    leaves = [int(i) for i in np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]]
    assert len(leaves) >= 4
    chosen = [leaves[0], leaves[1], leaves[len(leaves) // 2], leaves[-1]]
    keep = ~np.isin(leaf, chosen)
    sites, leaf = sites[keep], leaf[keep]
    for i, cnt in zip(chosen, (0, 1, 16, 17)):
        own = X[topo.perm[K.node_real_rows(topo, i)]]
        s = own[rng.integers(0, len(own), cnt)] + 1e-3 * span * rng.standard_normal((cnt, X.shape[1]))
        sites, leaf = np.vstack([sites, s]), np.concatenate([leaf, np.full(cnt, i, dtype=leaf.dtype)])
    sites, leaf = np.vstack([sites, sites[:3]]), np.concatenate([leaf, leaf[:3]])
    if len(leaf) % 16 == 0:
        sites, leaf = np.vstack([sites, sites[-1:]]), np.concatenate([leaf, leaf[-1:]])
    counts = {i: int((leaf == i).sum()) for i in chosen}
    assert [counts[i] for i in chosen[:2]] == [0, 1] and counts[chosen[2]] >= 16 and counts[chosen[3]] >= 17
    return sites, leaf.astype(np.int32)


def _against_twin(pl, topo, locs, spec, y_obs, R, sites, leaf, tag, tol=1e-9, Y=None, Yp=None):
    want_m, want_v = TS.tree_sites(topo, locs, spec, y_obs, R, sites, leaf, Y=Y)
    mean, var = pl.predict_sites(sites, leaf, Yp)
    scale = _scale(spec, topo.d)
    e_m, e_v = np.abs(mean.T - want_m).max(), np.abs(var - want_v).max()
    print("%s: %d sites against the twin: mean err %.2e (|m| %.2f), var err %.2e (scale %.2f)" % (tag, len(leaf), e_m, np.abs(want_m).max(), e_v, scale))
    assert _mean_ok(mean.T, want_m)
    assert e_v <= tol * scale
    return mean, var


# ---- 1. the tree's own rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_own_rows_as_sites_are_predict_and_dense_conditioning(hip, name):
    cs, rep, S, Sp = GC._reference(name)
    topo = cs["topo"]
    pl = GC._case_plan(hip, cs)
    rows, sites, leaf = _own_rows(topo, cs["locs"])
    m0, v0 = pl.predict()
    mean, var = pl.predict_sites(sites, leaf)
    assert mean.shape == (1, len(rows)) and var.shape == (len(rows),)
    scale = np.abs(S[np.ix_(rep, rep)]).max()
    e_m, e_v = np.abs(mean[0] - m0[topo.perm[rows]]).max(), np.abs(var - np.diag(Sp)).max()
    print("%s: %d own rows: |mean - predict| %.2e, |var - dense| %.2e, |var - predict| %.2e (scale %.2f)"
          % (name, len(rows), e_m, e_v, np.abs(var - v0[topo.perm[rows]]).max(), scale))
    assert _mean_ok(mean[0], m0[topo.perm[rows]])
    assert e_v <= GC._post_tol(name) * scale
    pl.close()


# ---- 2. sites off the rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES + ["grid48_r20"])
def test_off_row_sites_match_the_twin(hip, name):
    if name == "grid48_r20":                                  # leaves of nine row tiles
        topo, locs, y_obs, spec, R = GC._shape_tree(name)
    else:
        cs = K.load_case(name)
        topo, locs, y_obs, spec, R = cs["topo"], cs["locs"], cs["y_obs"], cs["spec"], float(cs["c"]["R"])
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    sites, leaf = _mixed_sites(topo, locs, seed=11)
    assert len(leaf) % 16 != 0
    mean, var = _against_twin(pl, topo, locs, spec, y_obs, R, sites, leaf, name, tol=GC._post_tol(name))
    assert np.all(var >= 0.0) and np.all(np.isfinite(mean))
    first = {}
    for k in range(len(leaf)):                                # duplicate sites: the same bits
        key = (sites[k].tobytes(), int(leaf[k]))
        if key in first:
            assert mean[0, k] == mean[0, first[key]] and var[k] == var[first[key]]
        first.setdefault(key, k)
    assert len(first) < len(leaf)
    pl.close()


# ---- 3. every device kernel family, 1-D and circular, single-leaf trees ---------------------------------------------------------------
@pytest.mark.parametrize("family", ["exp", "matern52", "gaussian", "kanter", "iden", "matern32_scale", "circular"])
def test_every_kernel_family(hip, family):
    import pymra_amd.MRATools as mt
    specs = {"exp": mt.KernelSpec(mt.KIND_EXP, 0.3), "matern52": mt.KernelSpec(mt.KIND_MATERN52, 0.2, 0.7),
             "gaussian": mt.KernelSpec(mt.KIND_GAUSSIAN, 0.05, 1.0), "kanter": mt.KernelSpec(mt.KIND_KANTER, 0.35),
             "iden": mt.KernelSpec(mt.KIND_IDEN, 0.01), "matern32_scale": mt.KernelSpec(mt.KIND_MATERN32, 0.4, 1.0, 2.5),
             "circular": mt.KernelSpec(mt.KIND_EXP, 0.3, 1.0, 1.0, True)}
    cs = K.load_case("c1" if family == "circular" else "g32")        # c1: a 1-D tree
    topo, locs, spec, R = cs["topo"], cs["locs"], specs[family], float(cs["c"]["R"])
    pl = GC._plan(hip, topo, locs, cs["y_obs"], R, spec)
    rows, own, own_leaf = _own_rows(topo, locs)
    off = SC.off_row_sites(locs, 37, seed=2)
    sites, leaf = np.vstack([off, own[::7]]), np.concatenate([SC.nearest_leaf(topo, locs, off), own_leaf[::7]]).astype(np.int32)
    _against_twin(pl, topo, locs, spec, cs["y_obs"], R, sites, leaf, family)
    pl.close()


@pytest.mark.parametrize("name", ["kat1", "kat4", "grid18_m0"])
def test_single_leaf_trees_are_plain_kriging(hip, name):
    topo, locs, y_obs, spec, R = GC._shape_tree(name)
    assert topo.n_nodes == 1
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    X = np.asarray(locs, float).reshape(topo.N, -1)
    sites = SC.off_row_sites(locs, 21, seed=6)
    mean, var = pl.predict_sites(sites, np.zeros(len(sites), dtype=np.int32))
    _, km, ksd = K.kriging(np.vstack([X, sites]), np.concatenate([np.asarray(y_obs, float).ravel(), np.full(len(sites), np.nan)]), spec, R)
    scale = _scale(spec, topo.d)
    e_m, e_v = np.abs(mean[0] - km[topo.N:]).max(), np.abs(var - ksd[topo.N:] ** 2).max()
    print("%s: kriging at %d sites: mean err %.2e, var err %.2e (scale %.2f)" % (name, len(sites), e_m, e_v, scale))
    assert _mean_ok(mean[0], km[topo.N:])
    assert e_v <= 1e-9 * scale
    pl.close()


# ---- 4. gappy mask ------------------------------------------------------------------------------------------------------------------
def test_mask_with_an_empty_leaf_and_an_empty_family(hip):
    topo, locs, y_obs, spec = GC._gappy()
    R = GC.R_MASK
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    y = np.asarray(y_obs, float).ravel()
    leaves = [int(i) for i in np.nonzero(topo.node_leaf)[0]]
    empty = [i for i in leaves if not np.isfinite(y[topo.perm[K.node_real_rows(topo, i)]]).any()]
    assert leaves[0] in empty and len(empty) >= 5                 # the first leaf and a whole family of four
    rows, own, own_leaf = _own_rows(topo, locs, np.concatenate([K.node_real_rows(topo, i)[::5] for i in empty[:5]]))
    off = SC.off_row_sites(locs, 50, seed=8)
    sites, leaf = np.vstack([own, off]), np.concatenate([own_leaf, SC.nearest_leaf(topo, locs, off)]).astype(np.int32)
    mean, var = _against_twin(pl, topo, locs, spec, y_obs, R, sites, leaf, "gappy 64^2")
    m0, v0 = pl.predict()
    assert _mean_ok(mean[0, :len(rows)], m0[topo.perm[rows]])
    assert np.abs(var[:len(rows)] - v0[topo.perm[rows]]).max() <= NO_TRUTH_TOL * _scale(spec, 2)
    pl.close()


# ---- 5. other routes ----------------------------------------------------------------------------------------------------------------
def _own_rows_against_predict(pl, topo, locs, spec, rows, tag):
    rows, sites, leaf = _own_rows(topo, locs, rows)
    m0, v0 = pl.predict()
    mean, var = pl.predict_sites(sites, leaf)
    scale = _scale(spec, topo.d)
    e_m, e_v = np.abs(mean[0] - m0[topo.perm[rows]]).max(), np.abs(var - v0[topo.perm[rows]]).max()
    print("%s: %d own rows: |mean - predict| %.2e (|m| %.2f), |var - predict| %.2e (scale %.2f)" % (tag, len(rows), e_m, np.abs(m0).max(), e_v, scale))
    assert _mean_ok(mean[0], m0[topo.perm[rows]])
    assert e_v <= NO_TRUTH_TOL * scale


def test_deep_wide_tree_on_chosen_leaves(hip):
    """cw = 64, five ancestors, the level-by-level route with panel-only fronts at the leaves' parents"""
    topo, locs, y_obs, spec, R = GC._deep_wide()
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    assert pl.route()["path"] == "Hi"
    rows = np.concatenate([K.node_real_rows(topo, j) for j in GC._leaf_sets(topo)])
    _own_rows_against_predict(pl, topo, locs, spec, rows, "deep wide")
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
    _own_rows_against_predict(pl, topo, locs, MK._spec(), rows, "leaf of 193 observations")
    pl.close()


# ---- 6. a block of observation vectors -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 17])
def test_columns_of_Y_are_solves_columns(hip, c):
    cs = K.load_case("g32")
    topo, locs = cs["topo"], cs["locs"]
    pl = GC._case_plan(hip, cs)
    rows, sites, leaf = _own_rows(topo, locs)
    obs_p = np.isfinite(np.asarray(cs["y_obs"], float).ravel())[topo.src] & (topo.perm >= 0)
    Yp = np.full((c, topo.P), np.nan)                        # NaN at every unobserved row: the call must not read them
    Yp[:, obs_p] = np.random.default_rng(c).standard_normal((c, int(obs_p.sum())))
    mean, var = pl.predict_sites(sites, leaf, Yp)
    want, _ = pl.solve(np.nan_to_num(Yp), want_quad=False)
    assert mean.shape == (c, len(rows))
    print("c=%d: |predict_sites - solve| %.2e" % (c, np.abs(mean - want[:, rows]).max()))
    assert _mean_ok(mean, want[:, rows])
    _, var0 = pl.predict_sites(sites, leaf)
    assert np.array_equal(var, var0)                         # var does not depend on Y
    assert pl.predict_sites(sites, leaf, Yp, want_var=False)[1] is None
    pl.close()


# ---- 7. bit identity ----------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_order_split_or_chunking(hip):
    topo, locs, y_obs, spec, R = GC._shape_tree("grid48_r20")
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    sites, leaf = _mixed_sites(topo, locs, seed=21)
    n = len(leaf)
    m1, v1 = pl.predict_sites(sites, leaf)
    order = np.random.default_rng(3).permutation(n)
    h = n // 3
    ma, va = pl.predict_sites(sites[order[:h]], leaf[order[:h]])
    mb, vb = pl.predict_sites(sites[order[h:]], leaf[order[h:]])
    m2, v2 = np.empty_like(m1), np.empty_like(v1)
    m2[:, order], v2[order] = np.hstack([ma, mb]), np.concatenate([va, vb])
    assert np.array_equal(m1, m2) and np.array_equal(v1, v2)
    assert pl.get_option(21) == 0
    pl.set_option(21, 1)                                     # one tile per chunk
    m3, v3 = pl.predict_sites(sites, leaf)
    assert GC._factor_launches(pl) == 0                      # option 21 keeps the factors
    assert pl.get_option(21) == 1
    pl.set_option(21, 0)
    assert np.array_equal(m1, m3) and np.array_equal(v1, v3)
    pl.close()


# ---- 8. state -----------------------------------------------------------------------------------------------------------------------
def test_predict_sites_leaves_the_callers_state_and_shares_the_factors(hip):
    topo, locs, y_obs, spec = GC._gappy()
    pl = GC._plan(hip, topo, locs, y_obs, GC.R_MASK, spec)
    opts = {k: pl.get_option(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21)}
    lik0, (m0, v0) = pl.likelihood(), pl.predict()
    sites = SC.off_row_sites(locs, 30, seed=1)
    leaf = SC.nearest_leaf(topo, locs, sites).astype(np.int32)
    a1, b1 = pl.predict_sites(sites, leaf)
    assert GC._factor_launches(pl) > 0                       # the first call ran its own likelihood pass
    assert pl.likelihood() == lik0
    m1, v1 = pl.predict()
    assert np.array_equal(m1, m0) and np.array_equal(v1, v0)
    assert {k: pl.get_option(k) for k in opts} == opts
    a2, b2 = pl.predict_sites(sites, leaf)
    assert GC._factor_launches(pl) == 0                      # the second one launched no kernel of a pass
    assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
    Yp = np.zeros((2, topo.P))
    pl.solve(Yp)
    assert GC._factor_launches(pl) == 0                      # solve after predict_sites reuses the factors
    a3, b3 = pl.predict_sites(sites, leaf)                   # ... and leaves beta / q of ITS right-hand sides behind: they are not reused
    assert GC._factor_launches(pl) == 0
    assert np.array_equal(a3, a1) and np.array_equal(b3, b1)
    pl.cov_apply(Yp, posterior=True)
    a4, b4 = pl.predict_sites(sites, leaf)
    assert GC._factor_launches(pl) == 0
    assert np.array_equal(a4, a1) and np.array_equal(b4, b1)
    pl.run(True, True)                                       # y untouched: the old numbers bit for bit
    assert pl.likelihood() == lik0
    pl.set_kernel(spec.kind, 0.5 * spec.l, spec.sig, spec.scale)
    a5, b5 = pl.predict_sites(sites, leaf)
    assert GC._factor_launches(pl) > 0                       # a new kernel: a new pass
    assert np.abs(a5 - a1).max() > 1e-6 and np.abs(b5 - b1).max() > 1e-6
    pl.close()


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------
def test_predict_sites_refusals(hip):
    from pymra_amd.plan import MraError
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
            pl.predict_sites(sites, leaf)
        assert e.value.code == -4, step                      # MRA_ERR_STATE before set_locs / set_kernel / set_obs
    pl.set_obs(y_obs, GC.R_MASK)
    good_m, good_v = pl.predict_sites(sites, leaf)
    mean, var = np.empty((2, 5)), np.empty(5)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def raw(flags=0, n=5, s=sites, lf=leaf, nc=1, Y=None):
        return pl.lib.mra_predict_sites(pl._h, flags, n, p(s), p(lf), nc, p(Y), p(mean), p(var))
    obs_p = np.isfinite(np.asarray(y_obs, float).ravel())[topo.src] & (topo.perm >= 0)
    Y = np.zeros((2, topo.P))
    assert raw() == 0 and raw(nc=2, Y=Y) == 0
    assert raw(flags=1) == -1 and raw(flags=2) == -1         # unknown flags
    assert raw(n=-1) == -1 and raw(nc=-1, Y=Y) == -1         # n_sites < 0, n_cols < 0
    assert raw(s=None) == -1 and raw(lf=None) == -1          # NULL sites / leaf with n_sites > 0
    assert raw(n=0, s=None, lf=None) == 0                    # n_sites == 0
    assert raw(nc=2) == -1 and raw(nc=0) == -1               # NULL Y: n_cols must be 1
    for bad_leaf in (-1, topo.n_nodes, 0):                   # out of range; the root is not a leaf
        lf = leaf.copy()
        lf[3] = bad_leaf
        assert raw(lf=lf) == -1, bad_leaf
    for bad_value in (np.nan, np.inf):
        s = sites.copy()
        s[2, 1] = bad_value
        assert raw(s=s) == -1                                # a non-finite coordinate
        Yb = Y.copy()
        Yb[1, np.nonzero(obs_p)[0][7]] = bad_value
        assert raw(nc=2, Y=Yb) == -1                         # a non-finite Y at an observed row
    Yn = Y.copy()
    Yn[:, ~obs_p] = np.nan
    assert raw(nc=2, Y=Yn) == 0                              # ... elsewhere it is not read
    again_m, again_v = pl.predict_sites(sites, leaf)         # the plan is still usable, and gives the same bits
    assert np.array_equal(again_m, good_m) and np.array_equal(again_v, good_v)
    pl.set_reduce_level(0)
    with pytest.raises(MraError) as e:
        pl.predict_sites(sites, leaf)
    assert e.value.code == -1                                # sharded
    pl.close()
    from pymra_amd import MRATree
    np.random.seed(1)
    n = 16
    l2 = mt.genLocations2d(Nx=n, Ny=n)
    y = np.random.normal(size=(n * n, 1))
    tree = MRATree(l2, 16, lambda a, b=np.array([]): np.exp(-np.abs(mt.dist(a, b)) / 0.3), y, 1e-2, M=1, J=4, verbose=False)      # opaque callable: host cov
    with pytest.raises(NotImplementedError):
        tree.predictAt(l2[:3])
    with pytest.raises(MraError) as e:
        tree.plan.predict_sites(l2[:3], tree.locate(l2[:3]))
    assert e.value.code == -1                                # MRA_KERNEL_HOST


# ---- 10. through MRATree ------------------------------------------------------------------------------------------------------------
def test_mratree_predictAt(hip):
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
    m0, sd0 = [np.asarray(a).ravel().copy() for a in tree.predict()]
    t = tree.topology
    un = np.nonzero(~np.isfinite(y.ravel()))[0]
    inv = np.full(n * n, -1)
    rep = SM.reported(t)
    inv[t.perm[rep]] = np.nonzero(rep)[0]
    own = SC.leaf_of_rows(t)[inv[un]]
    found = tree.locate(locs[un])
    assert found.dtype == np.int32 and np.array_equal(found, own)               # a tree location goes to its own leaf
    mean, sd = tree.predictAt(locs[un])
    assert mean.shape == (len(un), 1) and sd.shape == (len(un),)
    print("predictAt at %d unobserved locations: |mean - predict| %.2e, |var - predict| %.2e" % (len(un), np.abs(mean[:, 0] - m0[un]).max(), np.abs(sd ** 2 - sd0[un] ** 2).max()))
    assert _mean_ok(mean[:, 0], m0[un])
    assert np.abs(sd ** 2 - sd0[un] ** 2).max() <= NO_TRUTH_TOL
    leaves = np.nonzero(np.asarray(t.node_leaf, dtype=bool))[0].astype(np.int32)
    other = np.where(own == leaves[0], leaves[-1], leaves[0]).astype(np.int32)
    mo, so = tree.predictAt(locs[un], leaf=other)                               # an explicit assignment overrides locate
    direct_m, direct_v = tree.plan.predict_sites(locs[un], other)
    assert np.array_equal(mo[:, 0], direct_m[0]) and np.array_equal(so, np.sqrt(direct_v))
    assert np.abs(mo - mean).max() > 1e-6
    Y = np.where(np.isfinite(y), rng.standard_normal((n * n, 3)), np.nan)
    Y[:, 0] = y.ravel()
    mY, sY = tree.predictAt(locs[un], Y=Y)
    assert mY.shape == (len(un), 3) and np.array_equal(mY[:, 0], mean[:, 0]) and np.array_equal(sY, sd)
    assert _mean_ok(mY, tree.solve(np.nan_to_num(Y))[0][un])
    assert float(tree.getLikelihood()[0, 0]) == lik0
    m1, sd1 = [np.asarray(a).ravel() for a in tree.predict()]
    assert np.array_equal(m1, m0) and np.array_equal(sd1, sd0)
    for bad in (locs[:3, 0], np.zeros((3, 3)), np.array([[0.1, np.nan]])):
        with pytest.raises(ValueError):
            tree.predictAt(bad)
    with pytest.raises(ValueError):
        tree.predictAt(locs[:3], leaf=other[:2])
    with pytest.raises(ValueError):
        tree.predictAt(locs[:3], Y=np.zeros(5))


# ---- 11. BASELINE config 3 ----------------------------------------------------------------------------------------------------------
def test_own_rows_at_c3(hip):
    """4096 of the tree's own rows at 1024^2, M = 6, half of them observed, against the pass's own predict()."""
    import bench
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    c = bench.CONFIGS["c3"]
    locs, y_obs = bench.make_inputs(c)
    topo = build_topology(locs, c["r"], c["M"], c["J"])
    spec = mt.KernelSpec(mt.KIND_MATERN32, c["l"], c["sig"])
    rep = np.nonzero(SM.reported(topo))[0]
    ob = np.isfinite(np.asarray(y_obs, float).ravel())[topo.perm[rep]]
    rng = np.random.default_rng(1)
    rows = np.sort(np.concatenate([rng.choice(rep[ob], 2048, replace=False), rng.choice(rep[~ob], 2048, replace=False)]))
    pl = GC._plan(hip, topo, locs, y_obs, c["R"], spec)
    _own_rows_against_predict(pl, topo, locs, spec, rows, "c3")
    pl.close()
