"""Likelihood-only passes on gappy observation masks (GPU only).

A likelihood-only pass of the fused path walks gathered 16-row tiles of the OBSERVED rows only (MRA_OPT_LIK_ROWS), grouped into
workgroups per leaf or, with MRA_OPT_CASCADE_GROUP, per family of sibling leaves.  The cascade stages the ancestor chain of a
workgroup's first tile for all of its tiles, so a family whose first children have no observation must not be joined to the
previous family's workgroup.  Masks with block gaps (empty first children, empty families, clouds, exact observation counts
around the 16-row tile and the 192-row limit of the gathered path) on small regular trees, with grouping forced on and off:
the gathered pass must match the level-wise oracle, be bit-identical to the pass over all rows and to the ungrouped pass, and
match the predictive pass.  The same masks on the level-by-level path, on sharded plans and through MRATree.reevaluate."""
import os

import numpy as np
import pytest

import _cases as K

pytestmark = pytest.mark.gpu

R = 2e-2
TREES = [(64, 16, 3), (96, 32, 3), (128, 16, 4)]
COUNT_TREES = [(128, 16, 3), (128, 32, 3), (144, 16, 3)]          # leaves of at least 193 rows
COUNTS = (1, 15, 16, 17, 191, 192)
PRIOR_ROWS = "k_prior_cascade row pass"


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _spec():
    import pymra_amd.MRATools as mt
    return mt.KernelSpec(mt.KIND_MATERN32, 0.25, 1.2)


def _tree(n, r, M, seed=7):
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    np.random.seed(seed)                       # the knot draws of the tree replay use the global RNG
    locs = mt.genLocations2d(Nx=n, Ny=n)
    topo = build_topology(locs, r, M, 4)
    assert [int(v) for v in np.diff(topo.level_ptr)] == [4 ** k for k in range(M + 1)]
    return topo, locs


# ---- masks built from the topology ---------------------------------------------------------------------------------------------
def _leaf_callers(topo, i):
    p = topo.perm[int(topo.node_row0[i]):int(topo.node_row1[i])]
    return p[p >= 0]


def _families(topo):
    """Leaves in leaf (node) order, grouped by parent."""
    fams = []
    for i in np.nonzero(topo.node_leaf)[0]:
        if fams and topo.node_parent[fams[-1][-1]] == topo.node_parent[i]:
            fams[-1].append(int(i))
        else:
            fams.append([int(i)])
    return fams


def _empty(obs, topo, leaves):
    for i in leaves:
        obs[_leaf_callers(topo, i)] = False


def _cloud(obs, locs, x0=0.23, x1=0.61, y0=0.37, y1=0.71):
    lo, hi = locs.min(axis=0), locs.max(axis=0)
    u = (locs - lo) / (hi - lo)
    obs[(u[:, 0] >= x0) & (u[:, 0] <= x1) & (u[:, 1] >= y0) & (u[:, 1] <= y1)] = False


def _exact(obs, topo, leaf, count, rng):
    rows = _leaf_callers(topo, leaf)
    assert len(rows) >= count
    obs[rows] = False
    obs[rng.choice(rows, count, replace=False)] = True


def make_mask(topo, locs, pattern, seed=0):
    """Observed-location mask (bool[N]): seeded 40 % thinning outside the pattern's gaps."""
    rng = np.random.RandomState(seed)
    obs = rng.uniform(size=topo.N) < 0.4
    fams = _families(topo)
    leaves = [i for f in fams for i in f]
    if pattern == "first_child":
        _empty(obs, topo, [f[0] for f in fams])
    elif pattern == "first_two_alternate":
        _empty(obs, topo, [i for k, f in enumerate(fams) if k % 2 == 0 for i in f[:2]])
    elif pattern == "two_families":
        k = len(fams) // 2 - 1
        _empty(obs, topo, fams[k] + fams[k + 1])
    elif pattern == "last_child_only":
        _empty(obs, topo, [i for f in fams for i in f[:-1]])
    elif pattern == "first_family_last_leaf":
        _empty(obs, topo, fams[0] + [leaves[-1]])
    elif pattern == "one_leaf":
        _empty(obs, topo, [i for i in leaves if i != leaves[len(leaves) // 3]])
    elif pattern == "cloud":
        _cloud(obs, locs)
    elif pattern == "counts":
        # exact counts in the second child of every other family, whose first child is empty
        for k, c in enumerate(COUNTS):
            f = fams[2 * k + 1]
            _empty(obs, topo, f[:1])
            _exact(obs, topo, f[1], c, rng)
    elif pattern == "count_193":
        _exact(obs, topo, fams[1][1], 193, rng)
    else:
        raise ValueError(pattern)
    return obs


def leaf_counts(topo, obs):
    return np.array([int(obs[_leaf_callers(topo, i)].sum()) for i in np.nonzero(topo.node_leaf)[0]])


def cross_family_joins(topo, obs):
    """Leaves that the join rule 'same parent as leaf t - 1' (blind to leaves that own no tile) puts into a workgroup whose first
    tile belongs to another family: what a grouped likelihood-only pass computed against the wrong ancestors."""
    leaves = np.nonzero(topo.node_leaf)[0]
    nobs = leaf_counts(topo, obs)
    bad, head = 0, None
    for t, i in enumerate(leaves):
        if nobs[t] == 0:
            continue
        if head is not None and t > 0 and topo.node_parent[i] == topo.node_parent[leaves[t - 1]]:
            bad += int(topo.node_parent[head] != topo.node_parent[i])
        else:
            head = i
    return bad


def _y(obs, seed=1):
    y = np.random.RandomState(seed).normal(size=(len(obs), 1))
    return np.where(obs.reshape(-1, 1), y, np.nan)


# ---- passes --------------------------------------------------------------------------------------------------------------------
def _plan(hip, topo, locs, y):
    s = _spec()
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, R); pl.set_kernel(s.kind, s.l, s.sig, s.scale)
    return pl


def _row_flops(pl):
    st = [k for k in pl.kernel_stats() if k["name"].startswith(PRIOR_ROWS)]
    assert len(st) == 1 and st[0]["launches"] > 0, [k["name"] for k in pl.kernel_stats()]
    return st[0]["flops"]


def _lik_only(pl):
    pl.run(True, False)
    d, u = pl.likelihood()
    return d + u


def _oracle(topo, locs, y):
    from oracle.mra_levelwise import run_levelwise
    return run_levelwise(topo, locs, _spec(), y, R, predict=False)["lik"]


def _relerr(a, b):
    return abs(a - b) / max(abs(b), 1.0)


def check_fused(hip, topo, locs, y, tag, ref=None, gathered=True, make_plan=None):
    """Likelihood-only passes of one mask on one plan, sibling grouping forced on and off: each bit-identical to the pass over all
    rows (option 17 = 0) and to each other, equal to the predictive pass's likelihood (1e-12) and to ``ref`` (1e-11).  The
    gathered path must have run (fewer prior-row flops than the pass over all rows) - or, with ``gathered`` False, not.
    ``make_plan``: builds the plan instead of ``_plan`` (another kernel or noise variance; ``ref`` is then the caller's)."""
    pl = (make_plan or _plan)(hip, topo, locs, y)
    pl.set_option(hip.MRA_OPT_KERNEL_TIMING, 1)
    liks = {}
    for grp in (1, 0):
        pl.set_option(hip.MRA_OPT_CASCADE_GROUP, grp)
        assert pl.get_option(hip.MRA_OPT_CASCADE_GROUP) == grp
        lik = _lik_only(pl)
        fl = _row_flops(pl)
        pl.set_option(hip.MRA_OPT_LIK_ROWS, 0)
        lik_all = _lik_only(pl)
        fl_all = _row_flops(pl)
        pl.set_option(hip.MRA_OPT_LIK_ROWS, 1)
        if ref is not None:
            assert _relerr(lik, ref) <= 1e-11, "%s group=%d: rel err %.3e vs oracle" % (tag, grp, _relerr(lik, ref))
        assert lik == lik_all, "%s group=%d: gathered %.17g vs all rows %.17g (rel err %.3e)" % (tag, grp, lik, lik_all, _relerr(lik, lik_all))
        assert (fl < fl_all) if gathered else (fl == fl_all), (tag, grp, fl, fl_all)
        liks[grp] = lik
    assert liks[1] == liks[0], (tag, liks)
    pl.run(True, True)
    lik_pred = sum(pl.likelihood())
    assert _relerr(liks[1], lik_pred) <= 1e-12, (tag, liks[1], lik_pred)
    pl.close()
    return liks[1]


PATTERNS = ["first_child", "first_two_alternate", "two_families", "last_child_only", "first_family_last_leaf", "one_leaf", "cloud"]
# patterns whose gaps make the old join rule put some leaf into another family's workgroup (on every tree here)
STALE = {"first_child", "first_two_alternate", "last_child_only", "counts"}


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n,r,M", TREES)
def test_gappy_masks_on_the_fused_path(hip, n, r, M, pattern):
    topo, locs = _tree(n, r, M)
    obs = make_mask(topo, locs, pattern)
    nobs = leaf_counts(topo, obs)
    assert nobs.max() <= 192 and nobs.sum() > 0
    if pattern in STALE:
        assert cross_family_joins(topo, obs) > 0
    y = _y(obs)
    check_fused(hip, topo, locs, y, "%s %s" % ((n, r, M), pattern), ref=_oracle(topo, locs, y))


@pytest.mark.parametrize("n,r,M", COUNT_TREES)
def test_leaves_with_exact_observation_counts(hip, n, r, M):
    """Leaves of 1, 15, 16, 17, 191 and 192 observations (one tile + 1, a tile -1 / exactly / +1, the gathered path's limit), each
    behind an empty first child."""
    topo, locs = _tree(n, r, M)
    obs = make_mask(topo, locs, "counts")
    nobs = leaf_counts(topo, obs)
    assert set(COUNTS) <= set(nobs.tolist()) and nobs.max() == 192
    assert cross_family_joins(topo, obs) > 0
    y = _y(obs)
    check_fused(hip, topo, locs, y, "%s counts" % ((n, r, M),), ref=_oracle(topo, locs, y))


def test_193_observations_turn_the_gathered_path_off(hip):
    """One leaf of 193 observations (13 tiles): the likelihood-only pass goes over all rows, and still matches the oracle."""
    topo, locs = _tree(128, 16, 3)
    obs = make_mask(topo, locs, "count_193")
    assert leaf_counts(topo, obs).max() == 193
    y = _y(obs)
    check_fused(hip, topo, locs, y, "count_193", ref=_oracle(topo, locs, y), gathered=False)


def test_same_plan_new_mask_equals_a_fresh_plan(hip):
    """set_obs with another mask on a plan that already ran a grouped likelihood-only pass rebuilds its tile lists: bit-identical
    to a fresh plan of the new mask."""
    topo, locs = _tree(96, 32, 3)
    masks = [make_mask(topo, locs, p, seed=3) for p in ("cloud", "first_child", "one_leaf", "first_two_alternate")]
    pl = _plan(hip, topo, locs, _y(masks[0]))
    pl.set_option(hip.MRA_OPT_CASCADE_GROUP, 1)
    _lik_only(pl)
    for k, obs in enumerate(masks[1:]):
        y = _y(obs, seed=10 + k)
        pl.set_obs(y, R)
        lik = _lik_only(pl)
        fresh = _plan(hip, topo, locs, y)
        fresh.set_option(hip.MRA_OPT_CASCADE_GROUP, 1)
        assert lik == _lik_only(fresh), k
        fresh.close()
    pl.close()


def test_grouping_chosen_by_the_cost_model(hip):
    """512^2, r=32, M=5 (1024 leaves, 256 families): the cost model may group siblings by itself.  Its decision is reported, not
    assumed; the cloud and empty-first-child masks against the oracle with the plan's own decision and with it forced either way."""
    topo, locs = _tree(512, 32, 5)
    for pattern in ("cloud", "first_child"):
        obs = make_mask(topo, locs, pattern)
        assert leaf_counts(topo, obs).max() <= 192
        y = _y(obs)
        ref = _oracle(topo, locs, y)
        pl = _plan(hip, topo, locs, y)
        default = pl.get_option(hip.MRA_OPT_CASCADE_GROUP)
        print("512^2 r=32 M=5: MRA_OPT_CASCADE_GROUP chosen by the cost model = %d" % default)
        assert default in (0, 1)
        lik = _lik_only(pl)
        assert _relerr(lik, ref) <= 1e-11, "%s default group=%d: rel err %.3e" % (pattern, default, _relerr(lik, ref))
        pl.close()
        check_fused(hip, topo, locs, y, "512 " + pattern, ref=ref)


def test_mratree_reevaluate_on_the_sample_data_hole(hip):
    """pyMRA's sample data (a rectangular hole of 1440 locations) through MRATree + reevaluate(want_predict=False) with sibling
    grouping forced on, at two kappas, against a fresh predictive MRATree at each."""
    import pymra_amd
    import pymra_amd.MRATools as mt
    d = np.load(os.path.join(K.ROOT, "pymra_amd", "data", "large.npz"))
    locs, y_obs = d["locs"], d["y_obs"]
    assert int(np.isnan(y_obs).sum()) == 1440
    r0, M, me = 16, 4, 0.05
    cov = lambda k: (lambda a, b: mt.Matern32(a, b, l=k, sig=1.0))
    np.random.seed(11)
    tree = pymra_amd.MRATree(locs, r0, cov(0.2), y_obs, me, M=M, J=4, want_predict=False)
    assert cross_family_joins(tree.topology, np.isfinite(y_obs.ravel())) > 0        # the hole empties a first child
    tree.plan.set_option(hip.MRA_OPT_CASCADE_GROUP, 1)
    tree.plan.set_option(hip.MRA_OPT_KERNEL_TIMING, 1)
    for kappa in (0.1, 0.3):
        lik = tree.reevaluate(cov(kappa), want_predict=False)[0, 0]
        fl = _row_flops(tree.plan)
        tree.plan.set_option(hip.MRA_OPT_LIK_ROWS, 0)
        lik_all = tree.reevaluate(cov(kappa), want_predict=False)[0, 0]
        assert fl < _row_flops(tree.plan)                        # the gathered path ran
        tree.plan.set_option(hip.MRA_OPT_LIK_ROWS, 1)
        np.random.seed(11)
        fresh = pymra_amd.MRATree(locs, r0, cov(kappa), y_obs, me, M=M, J=4, want_predict=True)
        ref = fresh.getLikelihood()[0, 0]
        assert _relerr(lik, ref) <= 1e-12, "kappa %.2f: rel err %.3e" % (kappa, _relerr(lik, ref))
        assert lik == lik_all, kappa


def test_gappy_masks_on_the_level_by_level_path(hip):
    """A deep 64-wide tree (256^2, r=64, six levels) takes the level-by-level path; its likelihood-only passes walk the rows a
    likelihood needs (observed rows and knots): bit-identical to the pass over all rows, equal to the oracle."""
    topo, locs = _tree(256, 64, 5)
    for pattern in PATTERNS:
        obs = make_mask(topo, locs, pattern)
        y = _y(obs)
        pl = _plan(hip, topo, locs, y)
        pl.set_option(hip.MRA_OPT_KERNEL_TIMING, 1)
        lik = _lik_only(pl)
        st = pl.kernel_stats()
        assert not any(k["name"].startswith(PRIOR_ROWS) and k["launches"] > 0 for k in st), pattern
        fl = sum(k["flops"] for k in st)
        pl.set_option(hip.MRA_OPT_LIK_ROWS, 0)
        lik_all = _lik_only(pl)
        assert fl < sum(k["flops"] for k in pl.kernel_stats()), pattern          # the needed-rows path ran
        assert lik == lik_all, pattern
        ref = _oracle(topo, locs, y)
        assert _relerr(lik, ref) <= 1e-10, "%s: rel err %.3e" % (pattern, _relerr(lik, ref))
        pl.close()


@pytest.mark.parametrize("world", [4, 8])
def test_sharded_likelihood_only_on_gappy_masks(hip, world):
    """Every rank of an emulated 4- or 8-way run, likelihood only, grouping forced on and left to the cost model: one whole shard
    without observations, and a cloud across the shard boundaries."""
    topo, locs = _tree(128, 16, 4)
    for pattern in ("empty_shard", "cloud"):
        if pattern == "empty_shard":
            obs = make_mask(topo, locs, "first_child")
            first = int(topo.level_ptr[1])                       # the first level-1 subtree: rank 0 of 4, ranks 0 and 1 of 8
            obs[_leaf_callers(topo, first)] = False             # (a node's rows hold its whole subtree)
        else:
            obs = make_mask(topo, locs, "cloud")
        y = _y(obs)
        single = check_fused(hip, topo, locs, y, "single " + pattern, ref=_oracle(topo, locs, y))
        for opts in (((hip.MRA_OPT_CASCADE_GROUP, 1),), ()):
            liks, _, _, _ = K.emulate_world_on_one_gpu(hip, topo, locs, y, R, _spec(), world, predict=False, options=opts)
            assert len(liks) == world
            for rk, lk in enumerate(liks):
                assert _relerr(lk, single) <= 1e-12, "%s world %d rank %d %s: rel err %.3e" % (pattern, world, rk, opts, _relerr(lk, single))


@pytest.mark.parametrize("pivot", [13, 12])
def test_nan_pivot_in_the_last_panel_is_reported(hip, pivot):
    """A NaN on the diagonal of a dense covariance at one observed location of a one-node tree (14 observations, one 16 x 16
    panel): the factorisation meets it at pivot 13 (inside the last group of four, which a NaN-dropping minimum missed) or at
    pivot 12 (the first of the group).  Both must fail the pass with MRA_ERR_NOT_SPD instead of returning a NaN likelihood."""
    import pymra_amd
    import pymra_amd.MRATools as mt
    rng = np.random.RandomState(4)
    locs = rng.uniform(size=(14, 2))
    y = rng.normal(size=(14, 1))
    dense = np.asarray(mt.Matern32(locs, locs, l=0.3, sig=1.0))
    ok = pymra_amd.MRATree(locs, 4, np.matrix(dense), y, 1e-2, M=0)
    lik, _, _ = K.kriging(locs, y, mt.KernelSpec(mt.KIND_MATERN32, 0.3, 1.0), 1e-2)
    assert _relerr(ok.getLikelihood()[0, 0], lik) <= 1e-10
    assert np.array_equal(_leaf_callers(ok.topology, 0), np.arange(14))       # observation k of the panel is location k
    bad = dense.copy()
    bad[pivot, pivot] = np.nan
    with pytest.raises(hip.MraError) as ei:
        pymra_amd.MRATree(locs, 4, np.matrix(bad), y, 1e-2, M=0)
    assert ei.value.code == -3
