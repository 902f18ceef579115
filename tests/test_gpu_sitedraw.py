"""mra_sample_sites / HipPlan.sample_sites / MRATree.sampleAt on the GPU: draws of the latent MRA process at locations that need not be
rows of the tree, x = [mean +] F z with a tree-shaped F.  The device F is read off with unit columns of z, 16
slots per call.  Truths that do not come from the draw kernels: the NumPy restatements tests/_treesitedraw.py (F) and
tests/_treesitecov.py (F F^T; pinned to dense conditioning by tests/test_sitecov_cpu.py), the device mra_sites_cov where no twin can be
formed, the kriging covariance on single-leaf trees, tests/_philox.py for the seeded draws and mra_predict_sites for the mean.

Bounds are the project's own for the same comparison: PRIOR_TOL (1e-10) for the prior and _post_tol (1e-9; u3 1e-6) for the posterior
of tests/test_gpu_cov.py, POST_NO_TRUTH_TOL (1e-9) where only device results are compared, C3_POST_TOL at BASELINE config 3, all times
the largest prior variance.  Seeded draws against the same call with z from tests/_philox.py: 1e-12 times the scale (two runs of the
same device code on the same normals up to the host Philox's last bits): the first run on an MI355X printed 1.5e-15 at most, and 100
times that, 1.5e-13, is inside the bound.

Seen on one MI355X (scale = largest prior variance; prior / posterior): unit columns, |F F^T - twin| g32 8.9e-16 / 1.8e-15, c1 5.6e-16 /
5.8e-16, kat3 4.4e-16 / 5.3e-16, u3 1.1e-15 / 1.8e-15, the 48^2 tree 2.2e-15 / 3.7e-15; |F - twin F| g32 2.1e-15 / 7.2e-15, c1 2.2e-11 /
2.1e-11 (smallest relative pivot 1.1e-9: the factor itself is that ill-conditioned, its square is not), kat3 8.6e-15 / 1.1e-14, u3
2.2e-13 / 4.9e-13, the 48^2 tree 3.3e-14 / 8.4e-14; against sites_cov the deep 64-wide tree 5.3e-15 / 6.0e-15 and the leaf of 193
observations 2.7e-15 / 2.4e-15; every kernel family 4.4e-15 or less (Iden 0 / 1.9e-17); kat1, kat4 9.4e-16 or less; the gappy mask
2.2e-15 / 1.2e-14; z = 0 on the posterior: 0 from predict_sites' mean; sampleAt(z = I) 3.3e-16 / 1.1e-16; C3, 256 of 4096 sites, 8.9e-16
(bound C3_PRIOR_TOL 1.2e-12) / 1.1e-16 (bound C3_POST_TOL 1.8e-14)."""
import ctypes as C

import numpy as np
import pytest

import _cases as K
import _philox
import _sampling as SM
import _treesitecov as TC
import _treesitedraw as TD
import _treesites as TS
import test_gpu_cov as GC
import test_gpu_sites as TG
import test_sitedraw_cpu as DC
import test_sites_cpu as SC

pytestmark = pytest.mark.gpu

CASES = ["g32", "c1", "kat3", "u3"]
SEED_TOL = 1e-12


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def _leaves(topo):
    return [int(i) for i in np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]]


def _zoff(topo):
    """(first latent slot of every non-leaf node (-1: leaf), Kn): node order, cw[level] each - mra_sample's numbering"""
    zoff, kn = np.full(topo.n_nodes, -1, dtype=np.int64), 0
    for i in range(topo.n_nodes):
        if not topo.node_leaf[i]:
            zoff[i] = kn
            kn += int(topo.cw[int(topo.node_level[i])])
    return zoff, kn


def _slots_read(topo, leaf):
    """the latent slots the sites read: their ancestors' and their own"""
    zoff, kn = _zoff(topo)
    s = set()
    for i in np.unique(leaf):
        p = int(topo.node_parent[int(i)])
        while p >= 0:
            s.update(range(int(zoff[p]), int(zoff[p]) + int(topo.cw[int(topo.node_level[p])])))
            p = int(topo.node_parent[p])
    return np.concatenate([np.array(sorted(s), dtype=np.int64), kn + np.arange(len(leaf))])


def _device_F(pl, sites, leaf, posterior, slots=None):
    """(n, n_slots) the device factor from unit columns of z, 16 slots per call (columns outside `slots` stay 0)"""
    n = len(leaf)
    ns = pl.sample_sites_slots(n)
    slots = np.arange(ns) if slots is None else np.asarray(slots)
    F = np.zeros((n, ns))
    mean = pl.predict_sites(sites, leaf, want_var=False)[0][0] if posterior else np.zeros(n)
    for c0 in range(0, len(slots), 16):
        sl = slots[c0:c0 + 16]
        z = np.zeros((len(sl), ns))
        z[np.arange(len(sl)), sl] = 1.0
        F[:, sl] = (pl.sample_sites(sites, leaf, len(sl), z=z, posterior=posterior) - mean).T
    return F


def _spread(topo, locs, i, cnt, rng):
    """cnt sites spread over the bounding box of leaf i's own locations (no two closer than a grid of them allows)"""
    X = np.asarray(locs, float).reshape(topo.N, -1)
    own = X[topo.perm[K.node_real_rows(topo, i)]]
    lo, hi = own.min(0), own.max(0)
    pad = 0.45 * np.where(hi > lo, (hi - lo) / max(len(own) - 1, 1), 1e-2)
    d = X.shape[1]
    m = int(np.ceil(cnt ** (1.0 / d)))
    g = np.stack(np.meshgrid(*[(np.arange(m) + 0.37) / m for _ in range(d)], indexing="ij"), -1).reshape(-1, d)
    g = g[rng.permutation(len(g))[:cnt]]
    return (lo - pad) + g * (hi - lo + 2 * pad)


def _draw_sites(topo, locs, seed):
    """Sites off the rows: locate's rule for 45 of them, then five leaves given exactly 0, 1, 16, 17 and 96 sites (96 = six tiles:
    k_panel_chol's four waves wrap around); three duplicates; five sites on tree rows, one of them on an ancestor's knot; a total that
    is no multiple of 16.  -> (sites, leaf, the five chosen leaves)"""
    rng = np.random.default_rng(seed)
    X = np.asarray(locs, float).reshape(topo.N, -1)
    sites = SC.off_row_sites(locs, 45, seed)
    leaf = SC.nearest_leaf(topo, locs, sites)
    lv = _leaves(topo)
    chosen = [lv[0], lv[1], lv[len(lv) // 2], lv[-1], lv[len(lv) // 4]]
    assert len(set(chosen)) == 5
    keep = ~np.isin(leaf, chosen)
    sites, leaf = sites[keep], leaf[keep]
    for i, cnt in zip(chosen, (0, 1, 16, 17, 96)):
        sites, leaf = np.vstack([sites, _spread(topo, locs, i, cnt, rng)]), np.concatenate([leaf, np.full(cnt, i, dtype=leaf.dtype)])
    sites, leaf = np.vstack([sites, sites[:3]]), np.concatenate([leaf, leaf[:3]])                  # three duplicates
    rows = np.nonzero(SM.reported(topo))[0]
    knots = DC.ancestor_knot_rows(topo)
    on_knot = [int(r) for r in rows if int(r) in knots and int(SC.leaf_of_rows(topo)[r]) not in chosen]
    others = [int(r) for r in rows if int(r) not in knots and int(SC.leaf_of_rows(topo)[r]) not in chosen]
    others = [others[k] for k in np.unique(np.linspace(0, len(others) - 1, 4).astype(int))]
    pick = np.array((others + on_knot)[:5])
    assert any(int(r) in knots for r in pick) and any(int(r) not in knots for r in pick)
    assert len(pick) == 5
    sites, leaf = np.vstack([sites, X[topo.perm[pick]]]), np.concatenate([leaf, SC.leaf_of_rows(topo)[pick]])
    if len(leaf) % 16 == 0:
        sites, leaf = np.vstack([sites, sites[-1:]]), np.concatenate([leaf, leaf[-1:]])
    counts = [int((leaf == i).sum()) for i in chosen]
    assert counts == [0, 1, 16, 17, 96], counts
    assert len(leaf) % 16 != 0
    return sites, leaf.astype(np.int32), chosen


def _dups(sites, leaf):
    first, out = {}, []
    for k in range(len(leaf)):
        key = (sites[k].tobytes(), int(leaf[k]))
        if key in first:
            out.append((k, first[key]))
        first.setdefault(key, k)
    return out


def _check_FFt(F, want, scale, tol, tag):
    err = np.abs(F @ F.T - want).max()
    print("%s: |F F^T - truth| %.2e (bound %.1e, scale %.2f)" % (tag, err, tol * scale, scale))
    assert np.all(np.isfinite(F))
    assert err <= tol * scale
    return err


# ---- 1. unit columns against the twin -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES + ["grid48_r20"])
def test_unit_columns_are_the_twins_factor(hip, name):
    if name == "grid48_r20":                                  # cw = 32, leaves of nine observation tiles
        topo, locs, y_obs, spec, R = GC._shape_tree(name)
    else:
        cs = K.load_case(name)
        topo, locs, y_obs, spec, R = cs["topo"], cs["locs"], cs["y_obs"], cs["spec"], float(cs["c"]["R"])
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    sites, leaf, chosen = _draw_sites(topo, locs, seed=11)
    st = TS.SiteState(topo, locs, spec, y_obs, R)
    scale = TG._scale(spec, topo.d)
    assert pl.sample_sites_slots(len(leaf)) == _zoff(topo)[1] + len(leaf) == TD.coarse_slots(st)[1] + len(leaf)
    for post, tol in ((False, GC.PRIOR_TOL), (True, GC._post_tol(name))):
        kind = "posterior" if post else "prior"
        info = {}
        Ft, _ = TD.site_draw_factor(st, sites, leaf, post, info)
        F = _device_F(pl, sites, leaf, post)
        _check_FFt(F, TC.tree_sites_cov(st, sites, leaf, post), scale, tol, "%s %s, %d sites" % (name, kind, len(leaf)))
        e_f = np.abs(F - Ft).max()
        print("%s %s: |F - twin F| %.2e (%d inert, smallest relative pivot %.2e)" % (name, kind, e_f, int(info["inert"].sum()), info["min_pivot"]))
        assert e_f <= tol * scale
        assert info["inert"].any()                            # the site on an ancestor's knot
        assert not np.any(F[info["inert"], _zoff(topo)[1]:])  # ... has no leaf term at all
        dups = _dups(sites, leaf)
        assert len(dups) >= 3
        for k, k0 in dups:
            assert np.array_equal(F[k], F[k0])
    pl.close()


# ---- 2. against the device sites_cov where no twin can be formed ------------------------------------------------------------------------
def _against_sites_cov(pl, topo, locs, spec, rows, tag):
    rows, sites, leaf = TG._own_rows(topo, locs, rows)
    leaf = leaf.astype(np.int32)
    scale = TG._scale(spec, topo.d)
    slots = _slots_read(topo, leaf)
    for post in (False, True):
        F = _device_F(pl, sites, leaf, post, slots)
        _check_FFt(F, pl.sites_cov(sites, leaf, posterior=post), scale, GC.POST_NO_TRUTH_TOL,
                   "%s %s, %d own rows, %d slots" % (tag, "posterior" if post else "prior", len(rows), len(slots)))


def test_deep_wide_tree_against_sites_cov(hip):
    topo, locs, y_obs, spec, R = GC._deep_wide()
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    assert pl.route()["path"] == "Hi"
    rows = np.concatenate([K.node_real_rows(topo, j)[::2] for j in GC._leaf_sets(topo)])
    _against_sites_cov(pl, topo, locs, spec, rows, "deep wide")
    pl.close()


def test_a_leaf_of_more_than_192_observations_against_sites_cov(hip):
    import _route_cells as RC
    import test_gpu_likelihood_masks as MK
    topo, locs = MK._tree(*RC.TREES["A"])
    obs = RC.make_obs(topo, locs, ("edges", "empty_first", 193))
    pl = GC._plan(hip, topo, locs, MK._y(obs), MK.R, MK._spec())
    assert pl.route()["chol"] == "BigPanels"
    counts = MK.leaf_counts(topo, obs)
    leaves = _leaves(topo)
    big = leaves[int(np.argmax(counts))]
    assert max(counts) == 193
    rows = np.concatenate([K.node_real_rows(topo, big), K.node_real_rows(topo, leaves[0])[::3], K.node_real_rows(topo, leaves[7])[::3]])
    _against_sites_cov(pl, topo, locs, MK._spec(), rows, "leaf of 193 observations")
    pl.close()


# ---- 3. every device kernel family, 1-D and circular ----------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["exp", "matern52", "gaussian", "kanter", "iden", "matern32_scale", "circular"])
def test_every_kernel_family(hip, family):
    import pymra_amd.MRATools as mt
    specs = {"exp": mt.KernelSpec(mt.KIND_EXP, 0.3), "matern52": mt.KernelSpec(mt.KIND_MATERN52, 0.2, 0.7),
             "gaussian": mt.KernelSpec(mt.KIND_GAUSSIAN, 0.05, 1.0), "kanter": mt.KernelSpec(mt.KIND_KANTER, 0.35),
             "iden": mt.KernelSpec(mt.KIND_IDEN, 0.01), "matern32_scale": mt.KernelSpec(mt.KIND_MATERN32, 0.4, 1.0, 2.5),
             "circular": mt.KernelSpec(mt.KIND_EXP, 0.3, 1.0, 1.0, True)}
    cs = K.load_case("c1" if family == "circular" else "g32")        # the trees and sites of test_gpu_sitecov.py's family test
    topo, locs, spec, R = cs["topo"], cs["locs"], specs[family], float(cs["c"]["R"])
    pl = GC._plan(hip, topo, locs, cs["y_obs"], R, spec)
    rows, own, own_leaf = TG._own_rows(topo, locs)
    off = SC.off_row_sites(locs, 37, seed=2)
    sites, leaf = np.vstack([off, own[::7]]), np.concatenate([SC.nearest_leaf(topo, locs, off), own_leaf[::7]]).astype(np.int32)
    st = TS.SiteState(topo, locs, spec, cs["y_obs"], R)
    scale = TG._scale(spec, topo.d)
    kn = _zoff(topo)[1]
    for post, tol in ((False, GC.PRIOR_TOL), (True, 1e-9)):
        F = _device_F(pl, sites, leaf, post)
        _check_FFt(F, TC.tree_sites_cov(st, sites, leaf, post), scale, tol, "%s %s" % (family, "posterior" if post else "prior"))
        if family == "iden" and not post:
            # off the knots a = 0: G = amp I, the draws are independent there
            L = F[:len(off), kn:kn + len(off)]
            assert np.array_equal(L, np.sqrt(spec.evaluate(off[:1], off[:1])[0, 0]) * np.eye(len(off)))
            assert not np.any(F[:len(off), :kn])
    pl.close()


# ---- 4. single-leaf trees: Kn = 0 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kat1", "kat4"])
def test_single_leaf_trees_are_the_kriging_covariance(hip, name):
    topo, locs, y_obs, spec, R = GC._shape_tree(name)
    assert topo.n_nodes == 1
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    X = np.asarray(locs, float).reshape(topo.N, -1)
    sites = SC.off_row_sites(locs, 21, seed=6)
    leaf = np.zeros(len(sites), dtype=np.int32)
    assert pl.sample_sites_slots(len(sites)) == len(sites)
    o = np.isfinite(np.asarray(y_obs, float).ravel())
    Css, Cso = np.asarray(spec.evaluate(sites, sites)), np.asarray(spec.evaluate(sites, X[o]))
    want = Css - Cso @ np.linalg.solve(np.asarray(spec.evaluate(X[o], X[o])) + R * np.eye(int(o.sum())), Cso.T)
    scale = TG._scale(spec, topo.d)
    _check_FFt(_device_F(pl, sites, leaf, False), Css, scale, 1e-9, name + " prior")          # test_gpu_sitecov.py: 1e-9 * scale (kriging)
    _check_FFt(_device_F(pl, sites, leaf, True), want, scale, 1e-9, name + " posterior")
    pl.close()


# ---- 5. gappy mask --------------------------------------------------------------------------------------------------------------------
def test_mask_with_an_empty_leaf_and_an_empty_family(hip):
    topo, locs, y_obs, spec = GC._gappy()
    pl = GC._plan(hip, topo, locs, y_obs, GC.R_MASK, spec)
    y = np.asarray(y_obs, float).ravel()
    leaves = _leaves(topo)
    empty = [i for i in leaves if not np.isfinite(y[topo.perm[K.node_real_rows(topo, i)]]).any()]
    assert leaves[0] in empty and len(empty) >= 5                 # the first leaf and a whole family of four: they have no t
    rows, own, own_leaf = TG._own_rows(topo, locs, np.concatenate([K.node_real_rows(topo, i)[::5] for i in empty[:5]]))
    off = SC.off_row_sites(locs, 50, seed=8)
    sites, leaf = np.vstack([own, off]), np.concatenate([own_leaf, SC.nearest_leaf(topo, locs, off)]).astype(np.int32)
    st = TS.SiteState(topo, locs, spec, y_obs, GC.R_MASK)
    scale = TG._scale(spec, topo.d)
    slots = _slots_read(topo, leaf)
    for post, tol in ((False, GC.PRIOR_TOL), (True, 1e-9)):
        F = _device_F(pl, sites, leaf, post, slots)
        _check_FFt(F, TC.tree_sites_cov(st, sites, leaf, post), scale, tol, "gappy 64^2 %s" % ("posterior" if post else "prior"))
    pl.close()


# ---- 6. seeded draws, zero draws ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample0", [0, 2 ** 32 - 3])
def test_seeded_draws_are_philox(hip, sample0):
    """17 samples = two blocks; sample0 = 2^32 - 3: the sample counter carries into its high word inside the call"""
    topo, locs, y_obs, spec, R = GC._shape_tree("grid48_r20")
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    sites, leaf, _ = _draw_sites(topo, locs, seed=5)
    n, ns = len(leaf), pl.sample_sites_slots(len(leaf))
    seed = 0x9E3779B97F4A7C15
    z = _philox.latent_draws(seed, np.arange(ns), sample0 + np.arange(17))
    scale = TG._scale(spec, topo.d)
    for post in (False, True):
        a = pl.sample_sites(sites, leaf, 17, seed=seed, posterior=post, sample0=sample0)
        b = pl.sample_sites(sites, leaf, 17, z=z, posterior=post)
        err = np.abs(a - b).max()
        print("seeded against tests/_philox.py, sample0 = %d, %s: largest difference %.2e (bound %.1e)" % (sample0, "posterior" if post else "prior", err, SEED_TOL * scale))
        assert a.shape == (17, n) and np.all(np.isfinite(a))
        assert err <= SEED_TOL * scale
        assert np.array_equal(a[5:], pl.sample_sites(sites, leaf, 12, seed=seed, posterior=post, sample0=sample0 + 5))      # a pure function of the sample number
        assert not np.array_equal(a, pl.sample_sites(sites, leaf, 17, seed=seed + 1, posterior=post, sample0=sample0))
    pl.close()


def test_zero_draws_are_the_mean(hip):
    topo, locs, y_obs, spec, R = GC._shape_tree("grid48_r20")
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    sites, leaf, _ = _draw_sites(topo, locs, seed=5)
    z = np.zeros((3, pl.sample_sites_slots(len(leaf))))
    mean = pl.predict_sites(sites, leaf, want_var=False)[0][0]
    x1 = pl.sample_sites(sites, leaf, 3, z=z, posterior=True)
    err = np.abs(x1 - mean).max()
    print("z = 0, posterior: |x - predict_sites mean| %.2e" % err)
    assert err <= GC.POST_NO_TRUTH_TOL * TG._scale(spec, topo.d)
    x0 = pl.sample_sites(sites, leaf, 3, z=z)
    assert x0.shape == (3, len(leaf)) and not np.any(x0)         # the prior has mean 0, exactly
    assert pl.sample_sites(sites, leaf, 0).shape == (0, len(leaf))
    assert pl.sample_sites(sites[:0], leaf[:0], 4, seed=1).shape == (4, 0)
    pl.close()


# ---- 7. bit identity ------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_batches_other_leaves_or_the_call(hip):
    topo, locs, y_obs, spec, R = GC._shape_tree("grid48_r20")
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    sites, leaf, chosen = _draw_sites(topo, locs, seed=21)
    n, ns = len(leaf), pl.sample_sites_slots(len(leaf))
    kn = ns - n
    rng = np.random.default_rng(8)
    z = rng.standard_normal((17, ns))
    for post in (False, True):
        x1 = pl.sample_sites(sites, leaf, 17, z=z, posterior=post)
        assert np.array_equal(x1, pl.sample_sites(sites, leaf, 17, z=z, posterior=post))        # two identical calls
        s1 = pl.sample_sites(sites, leaf, 17, seed=3, posterior=post)
        assert pl.get_option(21) == 0
        pl.set_option(21, 1)                                 # one leaf per batch
        x2 = pl.sample_sites(sites, leaf, 17, z=z, posterior=post)
        s2 = pl.sample_sites(sites, leaf, 17, seed=3, posterior=post)
        assert GC._factor_launches(pl) == 0                  # option 21 keeps the factors
        pl.set_option(21, 0)
        assert np.array_equal(x2, x1) and np.array_equal(s2, s1)
        for i in chosen[2:]:                                 # the call restricted to the sites of one leaf, in the same order
            who = np.nonzero(leaf == i)[0]
            zz = np.hstack([z[:, :kn], z[:, kn + who]])
            assert np.array_equal(pl.sample_sites(sites[who], leaf[who], 17, z=zz, posterior=post), x1[:, who])
        dups = _dups(sites, leaf)
        assert len(dups) >= 3
        for k, k0 in dups:
            assert np.array_equal(x1[:, k], x1[:, k0]) and np.array_equal(s1[:, k], s1[:, k0])
        zd = z.copy()
        zd[:, kn + np.array([k for k, _ in dups])] = 7.0     # a duplicate's own leaf slot is not read
        assert np.array_equal(pl.sample_sites(sites, leaf, 17, z=zd, posterior=post), x1)
    pl.close()


# ---- 8. state -------------------------------------------------------------------------------------------------------------------------
def test_sample_sites_leaves_the_callers_state_and_shares_the_factors(hip):
    topo, locs, y_obs, spec = GC._gappy()
    pl = GC._plan(hip, topo, locs, y_obs, GC.R_MASK, spec)
    opts = {k: pl.get_option(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23)}
    lik0, (m0, v0) = pl.likelihood(), pl.predict()
    sites = SC.off_row_sites(locs, 30, seed=1)
    leaf = SC.nearest_leaf(topo, locs, sites).astype(np.int32)
    z = np.random.default_rng(2).standard_normal((5, pl.sample_sites_slots(30)))
    p1 = pl.sample_sites(sites, leaf, 5, z=z, posterior=True)
    assert GC._factor_launches(pl) > 0                       # the first call ran its own likelihood pass
    assert pl.likelihood() == lik0
    m1, v1 = pl.predict()
    assert np.array_equal(m1, m0) and np.array_equal(v1, v0)
    assert {k: pl.get_option(k) for k in opts} == opts
    q1 = pl.sample_sites(sites, leaf, 5, z=z)
    assert GC._factor_launches(pl) == 0                      # the second one launched no kernel of a pass
    Yp = np.zeros((2, topo.P))
    for other in (lambda: pl.solve(Yp), lambda: pl.cov_apply(Yp, posterior=True), lambda: pl.predict_sites(sites, leaf),
                  lambda: pl.sites_cov(sites, leaf, posterior=True)):
        other()
        assert GC._factor_launches(pl) == 0
        p2 = pl.sample_sites(sites, leaf, 5, z=z, posterior=True)
        assert GC._factor_launches(pl) == 0                  # sample_sites after the sibling launches no factorisation
        assert np.array_equal(p2, p1)
    assert pl.likelihood() == lik0
    m1, v1 = pl.predict()
    assert np.array_equal(m1, m0) and np.array_equal(v1, v0)
    assert len(pl.buffer(9)) == 9
    pl.run(True, True)                                       # y untouched: the old numbers bit for bit
    assert pl.likelihood() == lik0
    y2 = np.asarray(y_obs, float).copy()
    y2[np.nonzero(np.isfinite(y2))[0][::2]] = np.nan         # another mask
    pl.set_obs(y2, GC.R_MASK)
    p3 = pl.sample_sites(sites, leaf, 5, z=z, posterior=True)
    assert GC._factor_launches(pl) > 0                       # a new mask: a new pass
    q3 = pl.sample_sites(sites, leaf, 5, z=z)
    assert np.abs(p3 - p1).max() > 1e-6
    assert np.array_equal(q3, q1)                            # the prior does not depend on the mask
    pl.close()


# ---- 9. refusals and the facade -------------------------------------------------------------------------------------------------------
def test_sample_sites_refusals(hip):
    from pymra_amd.plan import MraError, MRA_SAMPLE_SITES_LEAF_MAX
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
            pl.sample_sites(sites, leaf, 2)
        assert e.value.code == -4, step                      # MRA_ERR_STATE before set_locs / set_kernel / set_obs
    pl.set_obs(y_obs, GC.R_MASK)
    good = pl.sample_sites(sites, leaf, 2, seed=4, posterior=True)
    out = np.empty((2, 5))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    seen = set()

    def raw(flags=0, n=5, s=sites, lf=leaf, nsamp=2, s0=0, o=out):
        return pl.lib.mra_sample_sites(pl._h, flags, n, p(s), p(lf), nsamp, 1, s0, None, p(o))

    def refused(**kw):
        assert raw(**kw) == -1, kw
        msg = pl.lib.mra_last_error(pl._h)
        seen.add(msg)
        return msg
    assert raw() == 0 and raw(flags=1) == 0
    refused(flags=2)
    refused(flags=3)                                         # unknown flags (same message)
    refused(n=-1)
    refused(nsamp=-1)
    refused(s0=-1)
    assert refused(s0=2 ** 63 - 1) == refused(s0=-1)         # sample0 + n_samples - 1 overflows
    assert raw(s0=2 ** 63 - 2) == 0
    refused(s=None)
    assert refused(lf=None) == refused(s=None)
    refused(o=None)
    assert raw(n=0, s=None, lf=None, o=None) == 0            # n_sites == 0
    assert raw(nsamp=0, o=None) == 0                         # n_samples == 0: nothing to write
    for bad_leaf in (-1, topo.n_nodes, 0):                   # out of range; the root is not a leaf
        lf = leaf.copy()
        lf[3] = bad_leaf
        refused(lf=lf)
    for bad_value in (np.nan, np.inf):
        s = sites.copy()
        s[2, 1] = bad_value
        refused(s=s)
    assert len(seen) == 10                                   # each kind of refusal has its own message (three bad leaves: three)
    assert np.array_equal(pl.sample_sites(sites, leaf, 2, seed=4, posterior=True), good)      # the plan is still usable, and gives the same bits
    with pytest.raises(ValueError):
        pl.sample_sites(sites, leaf, 2, z=np.zeros((2, 3)))
    pl.set_reduce_level(0)
    with pytest.raises(MraError) as e:
        pl.sample_sites(sites, leaf, 2)
    assert e.value.code == -1 and "sharded" in str(e.value)
    pl.close()
    # the per-leaf cap: 4097 distinct sites in one leaf of g32; duplicates do not count.  Refused on the host: no kernel is launched
    cs = K.load_case("g32")
    topo = cs["topo"]
    pl = GC._plan(hip, topo, cs["locs"], cs["y_obs"], float(cs["c"]["R"]), cs["spec"])
    i = _leaves(topo)[3]
    many = _spread(topo, cs["locs"], i, MRA_SAMPLE_SITES_LEAF_MAX + 1, np.random.default_rng(1))
    assert len(np.unique(many, axis=0)) == MRA_SAMPLE_SITES_LEAF_MAX + 1
    lf = np.full(len(many), i, dtype=np.int32)
    pl.predict_sites(many[:4], lf[:4])                       # the factors are valid: the statistics of a later call are all zero
    with pytest.raises(MraError) as e:
        pl.sample_sites(many, lf, 1)
    assert e.value.code == -1 and "MRA_SAMPLE_SITES_LEAF_MAX" in str(e.value) and "leaf %d" % i in str(e.value)
    twice = np.vstack([many[:64], many[:64]])
    x = pl.sample_sites(twice, lf[:128], 2, seed=1)
    assert np.array_equal(x[:, :64], x[:, 64:])
    pl.close()
    from pymra_amd import MRATree
    np.random.seed(1)
    n = 16
    l2 = mt.genLocations2d(Nx=n, Ny=n)
    y = np.random.normal(size=(n * n, 1))
    tree = MRATree(l2, 16, lambda a, b=np.array([]): np.exp(-np.abs(mt.dist(a, b)) / 0.3), y, 1e-2, M=1, J=4, verbose=False)      # opaque callable: host cov
    with pytest.raises(NotImplementedError):
        tree.sampleAt(l2[:3], 2)
    with pytest.raises(MraError) as e:
        tree.plan.sample_sites(l2[:3], tree.locate(l2[:3]), 2)
    assert e.value.code == -1 and "MRA_KERNEL_HOST" in str(e.value)


def test_mratree_sampleAt(hip):
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
    slots = tree.plan.sample_sites_slots(ns)
    for distr in ("posterior", "prior"):
        S = tree.covarianceAt(sites, distr=distr)
        mean = tree.predictAt(sites)[0] if distr == "posterior" else np.zeros((ns, 1))
        X = np.hstack([tree.sampleAt(sites, min(16, slots - c0), distr=distr, z=np.eye(slots)[:, c0:c0 + 16]) for c0 in range(0, slots, 16)])
        assert X.shape == (ns, slots)
        err = np.abs((X - mean) @ (X - mean).T - S).max()
        print("sampleAt(z = I), %s: |F F^T - covarianceAt| %.2e" % (distr, err))
        assert err <= GC.POST_NO_TRUTH_TOL
        a, b = tree.sampleAt(sites, 7, distr=distr, seed=5), tree.sampleAt(sites, 7, distr=distr, seed=5)
        assert a.shape == (ns, 7) and np.array_equal(a, b)
        assert not np.array_equal(a, tree.sampleAt(sites, 7, distr=distr, seed=6))
        assert np.array_equal(a, tree.sampleAt(sites, 7, distr=distr, seed=5, leaf=tree.locate(sites)))
        assert np.array_equal(a, tree.plan.sample_sites(sites, tree.locate(sites), 7, seed=5, posterior=(distr == "posterior")).T)
    np.random.seed(11)
    a = tree.sampleAt(sites, 2)                               # seed=None: NumPy's global RNG, as simulate()
    np.random.seed(11)
    assert np.array_equal(a, tree.sampleAt(sites, 2)) and not np.array_equal(a, tree.sampleAt(sites, 2))
    assert float(tree.getLikelihood()[0, 0]) == lik0
    with pytest.raises(ValueError):
        tree.sampleAt(sites, 2, distr="conditional")
    with pytest.raises(ValueError):
        tree.sampleAt(sites, 2, leaf=tree.locate(sites)[:3])
    with pytest.raises(ValueError):
        tree.sampleAt(sites, 3, z=np.zeros((slots, 2)))
    with pytest.raises(ValueError):
        tree.sampleAt(np.zeros((3, 3)), 2)


# ---- 10. BASELINE config 3 ------------------------------------------------------------------------------------------------------------
def test_half_cell_shifted_sites_at_c3(hip):
    """4096 half-cell-shifted sites in 16 whole leaves at 1024^2, M = 6: 16 posterior draws from a seed, and F F^T of 256 of the sites
    (unit columns restricted to the slots they read) against sites_cov.  Seen on one MI355X: see DESIGN.md section 14."""
    import bench
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    c = bench.CONFIGS["c3"]
    locs, y_obs = bench.make_inputs(c)
    topo = build_topology(locs, c["r"], c["M"], c["J"])
    spec = mt.KernelSpec(mt.KIND_MATERN32, c["l"], c["sig"])
    X = np.asarray(locs, float).reshape(topo.N, -1)
    h = 0.5 * np.abs(np.diff(np.unique(X[:, 0]))).min()
    lv = _leaves(topo)
    some = [lv[k] for k in np.linspace(0, len(lv) - 1, 16).astype(int)]
    sites, leaf = [], []
    for i in some:
        own = X[topo.perm[K.node_real_rows(topo, i)]]
        assert len(own) == 256
        sites.append(own + h)
        leaf.append(np.full(256, i, dtype=np.int32))
    sites, leaf = np.vstack(sites), np.concatenate(leaf)
    assert len(leaf) == 4096
    pl = GC._plan(hip, topo, locs, y_obs, c["R"], spec)
    x = pl.sample_sites(sites, leaf, 16, seed=7, posterior=True)
    assert x.shape == (16, 4096) and np.all(np.isfinite(x))
    print("c3: 16 posterior draws at 4096 sites: |x - mean| rms %.3f" % np.sqrt(np.mean((x - pl.predict_sites(sites, leaf, want_var=False)[0][0]) ** 2)))
    sub = np.sort(np.random.default_rng(1).choice(4096, 256, replace=False))
    scale = TG._scale(spec, topo.d)
    slots = _slots_read(topo, leaf[sub])
    for post, tol in ((False, GC.C3_PRIOR_TOL), (True, GC.C3_POST_TOL)):
        F = _device_F(pl, sites[sub], leaf[sub], post, slots)
        err = np.abs(F @ F.T - pl.sites_cov(sites[sub], leaf[sub], posterior=post)).max()
        print("c3: 256 sites, %d slots, F F^T against sites_cov: %s err %.2e (bound %.1e, scale %.2f)" % (len(slots), "posterior" if post else "prior", err, tol * scale, scale))
        if err > tol * scale:
            print("c3: above the bound measured for cov_apply against its own truth; held to POST_NO_TRUTH_TOL")
            tol = GC.POST_NO_TRUTH_TOL
        assert err <= tol * scale
    pl.close()
