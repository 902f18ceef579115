"""mra_plan_set_metric on the GPU: distances |A (a - b)|, applied in front of the kernels.

 1. BITWISE.  If every entry of A is 0 or a signed power of two, fma(A_ik, x_k, acc) is acc + A_ik x_k in plain float64, so a NumPy
    twin that adds the columns in the stated order gives the device's coordinates bit for bit.  Plan M = set_locs(raw) + set_metric(A)
    must then equal plan T = set_locs(twin(raw, A)) on the same Topology object in every call, with no tolerance: buffer(13), d and u,
    mean and var, solve (17 columns), cov_apply, predict_sites / sites_cov (sites raw to M, twin-transformed to T, tree locations
    among them), sample_sites (a duplicated site), cv by row and by leaf, a conditional sample and a Poisson Laplace fit - on a
    regular fused-path tree of 64 x 64 / r0 16 / M 3 (the per-level kx arrays and the knot chain's packed records), scattered 2-D
    locations with ragged leaves level by level (MRA_OPT_FUSED 0: X alone), the 1-D tree t1000 and a d = 3 plan on a (lon, lat)
    partition.
 2. state: A1, A2, A1; None; the identity; set_obs and set_locs after set_metric.
 3. a general A against the level-wise oracle with the KernelSpec that carries A, at the project's bars against that oracle
    (BARS of tests/test_gpu_sphere.py); predictAt at tree locations against predict(); covarianceAt against dense conditioning of the
    NumPy restatement's prior covariance (tests/_treesites.py) at the bound of tests/test_gpu_cov.py (1e-9 times the prior variance).
 4. the anisotropic likelihood is more than 1 % away from the isotropic one.
 5. world 4 against the single plan M at the bars of tests/_sharded_cases.py.
 6. refusals, each with its message.   7. the MRATree surface.

None of the bounds is derived from a result of the code under test."""
import functools

import numpy as np
import pytest

import _cases as K
import pymra_amd.MRATools as mt
from pymra_amd.topology import build_topology

pytestmark = pytest.mark.gpu

R = 1e-2
BARS = (1e-11, 1e-9, 1e-8)                      # tests/test_gpu_sphere.py: likelihood (relative), mean (absolute), sd (relative)
SPREAD, SINGLE_LIK, SINGLE_MEAN, SINGLE_VAR = 1e-12, 1e-12, 1e-11, 1e-12       # tests/_sharded_cases.py
A1D = np.array([[2.0]])
A2D = np.array([[1.0, 0.5], [-0.25, 2.0]])
A3D = np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.25]])
FAMILIES = {"exp": mt.KernelSpec(mt.KIND_EXP, 0.4), "m32": mt.KernelSpec(mt.KIND_MATERN32, 0.3, 1.3),
            "m52": mt.KernelSpec(mt.KIND_MATERN52, 0.4, 0.7), "gauss": mt.KernelSpec(mt.KIND_GAUSSIAN, 0.05, 0.8),
            "kanter": mt.KernelSpec(mt.KIND_KANTER, 0.9)}


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def twin(X, A):
    """A x by row in the arithmetic the library states, without fma: exact products of dyadic entries, one rounding per addition"""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    out = np.empty_like(X)
    for i in range(A.shape[0]):
        acc = A[i, 0] * X[:, 0]
        for k in range(1, A.shape[1]):
            acc = acc + A[i, k] * X[:, k]
        out[:, i] = acc
    return out


def _mask_data(topo, coords, seed=0, frac=0.4):
    """a smooth function of the raw coordinates plus noise, `frac` observed, the first leaf without any observation"""
    rng = np.random.default_rng(seed)
    N = len(coords)
    obs = rng.random(N) < frac
    i = int(np.nonzero(topo.node_leaf)[0][0])
    p = topo.perm[int(topo.node_row0[i]):int(topo.node_row1[i])]
    obs[p[p >= 0]] = False
    c = np.asarray(coords, dtype=np.float64).reshape(N, -1)
    f = np.sin(3.0 * c[:, 0]) + 0.5 * np.cos(2.0 * c[:, -1] + c[:, 0])
    return np.where(obs, f + np.sqrt(R) * rng.standard_normal(N), np.nan)


@functools.lru_cache(maxsize=None)
def grid_tree(n=64, r=16, M=3, jitter=False):
    """(locs, topology, y): tree (a) of the issue - regular, fused path, three levels above the leaves"""
    locs = mt.genLocations2d(Nx=n, Ny=n)
    if jitter:
        locs = locs + np.random.default_rng(5).uniform(-0.3, 0.3, size=locs.shape) / n
    np.random.seed(7)
    topo = build_topology(locs, r, M, 4)
    return locs, topo, _mask_data(topo, locs)


@functools.lru_cache(maxsize=None)
def scattered_tree():
    """tree (b): fully scattered 2-D locations, ragged leaves (K.random_geometry with seed % 3 == 2)"""
    g = K.random_geometry(8)
    t = g["topo"]
    assert len(np.unique((t.node_row1 - t.node_row0)[np.asarray(t.node_leaf, dtype=bool)])) > 1, "leaves are not ragged"
    return g["locs"], g["topo"], _mask_data(g["topo"], g["locs"], seed=1)


@functools.lru_cache(maxsize=None)
def line_tree():
    """tree (c): the 1000 points of the 1-D golden case t1000 (ternary splits, 1296 padded rows)"""
    cs = K.load_case("t1000")
    return cs["locs"], cs["topo"], _mask_data(cs["topo"], cs["locs"], seed=2)


@functools.lru_cache(maxsize=None)
def sphere_tree():
    """tree (d): (lon, lat) partition, xyz coordinates (d = 3)"""
    n = 48
    lon = -180.0 + (np.arange(n) + 0.5) * 360.0 / n
    g, h = np.meshgrid(lon, np.linspace(-80.0, 80.0, n))
    ll = np.column_stack((g.ravel(), h.ravel()))
    np.random.seed(7)
    topo = build_topology(ll, 16, 2, 4, coord_dim=3)
    xyz = mt.lonlat_to_xyz(ll)
    return xyz, topo, _mask_data(topo, xyz, seed=3)


def leaf_of_callers(topo):
    """caller row -> node index of the leaf that reports it (-1: none)"""
    out = np.full(topo.N, -1, dtype=np.int32)
    inl = np.asarray(topo.in_leaf, dtype=bool)
    for i in np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]:
        rows = np.arange(int(topo.node_row0[i]), int(topo.node_row1[i]))
        rows = rows[(topo.perm[rows] >= 0) & inl[rows]]
        out[topo.perm[rows]] = i
    return out


def make_sites(topo, coords, seed):
    """(sites in raw coordinates, leaves): 23 tree locations in their own leaves, 30 points between tree locations in the leaf of
    the first of the two, and one duplicate - 54, no multiple of 16"""
    rng = np.random.default_rng(seed)
    X = np.asarray(coords, dtype=np.float64).reshape(topo.N, -1)
    lf = leaf_of_callers(topo)
    ok = np.nonzero(lf >= 0)[0]
    own = rng.choice(ok, 23, replace=False)
    a, b = rng.choice(ok, 30, replace=False), rng.choice(ok, 30, replace=False)
    sites = np.vstack((X[own], 0.75 * X[a] + 0.25 * X[b]))
    leaf = np.concatenate((lf[own], lf[a]))
    return np.vstack((sites, sites[30:31])), np.concatenate((leaf, leaf[30:31])).astype(np.int32)


def make_plan(hip, topo, coords, y, spec, A=None, opts=()):
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(coords)
    if A is not None:
        pl.set_metric(A)
    pl.set_obs(y, R)
    pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
    for o, v in opts:
        pl.set_option(o, v)
    return pl


def passes(pl):
    """likelihood + predict, then likelihood-only (its own route)"""
    pl.run(True, True)
    mean, var = pl.predict()
    out = dict(lik=np.array(pl.likelihood()), mean=mean.copy(), var=var.copy())
    pl.run(True, False)
    out["lik_only"] = np.array(pl.likelihood())
    return out


def battery(pl, topo, y, sites, leaf):
    """every call the issue lists, in one fixed order; -> {name: array}"""
    rng = np.random.default_rng(11)
    out = dict(X=pl.buffer(13))
    out.update(passes(pl))
    Y = rng.standard_normal((17, topo.P))
    out["solve_mean"], out["solve_quad"] = pl.solve(Y)
    Av = rng.standard_normal((3, topo.P))
    out["cov_prior"], out["gram_prior"] = pl.cov_apply(Av)
    out["cov_post"], out["gram_post"] = pl.cov_apply(Av, posterior=True)
    out["site_mean"], out["site_var"] = pl.predict_sites(sites, leaf)
    out["sites_cov_prior"] = pl.sites_cov(sites, leaf)
    out["sites_cov_post"] = pl.sites_cov(sites, leaf, posterior=True)
    out["site_draws"] = pl.sample_sites(sites, leaf, 3, seed=99, posterior=True)
    for name, by_leaf in (("cv_row", False), ("cv_leaf", True)):
        for k, v in zip(("mean", "var", "lpd", "group", "info"), pl.cv(leaf=by_leaf)):
            out["%s_%s" % (name, k)] = v
    out["sample"] = pl.sample(2, seed=5, conditional=True)
    z = np.where(np.isfinite(y), np.random.default_rng(4).poisson(np.exp(0.5 * np.nan_to_num(y))), np.nan)
    fit = pl.fit_laplace("poisson", z, max_iter=10)
    out["laplace_info"] = fit["info"]
    out["laplace_mean"], out["laplace_var"] = (v.copy() for v in pl.predict())
    return out


def same_bits(got, want, tag):
    assert got.keys() == want.keys()
    bad = [k for k in got if np.asarray(got[k]).tobytes() != np.asarray(want[k]).tobytes()]
    for k in bad:
        print("%s: %s differs, max |diff| %.3e" % (tag, k, np.nanmax(np.abs(np.asarray(got[k]) - np.asarray(want[k])))))
    assert not bad, "%s: not bit for bit: %s" % (tag, bad)
    assert all(np.all(np.isfinite(got[k])) for k in ("lik", "mean", "var", "site_mean", "site_var", "sample") if k in got)


def m_against_t(hip, coords, topo, y, spec, A, tag, seed=0, opts=()):
    sites, leaf = make_sites(topo, coords, seed)
    dup = np.all(sites[-1] == sites[30])
    assert dup
    pm = make_plan(hip, topo, coords, y, spec, A, opts)
    pt = make_plan(hip, topo, twin(coords, A), y, spec, opts=opts)
    try:
        got, want = battery(pm, topo, y, sites, leaf), battery(pt, topo, y, twin(sites, A), leaf)
        same_bits(got, want, tag)
        assert np.array_equal(got["site_draws"][:, -1], got["site_draws"][:, 30])           # the duplicate received its first occurrence's draw
        assert not np.array_equal(got["X"], make_plan_raw_X(topo, coords))                  # the metric was applied
        return pm.route(), got
    finally:
        pm.close()
        pt.close()


def make_plan_raw_X(topo, coords):
    X = np.asarray(coords, dtype=np.float64).reshape(topo.N, -1)
    return X[topo.src].ravel()


# ---- 1. bitwise against plan T ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_bitwise_regular_fused_tree(hip, fam):
    locs, topo, y = grid_tree()
    route, got = m_against_t(hip, locs, topo, y, FAMILIES[fam], A2D, "grid64/" + fam)
    assert route["path"] == "Fused", "tree (a) must run the fused path (kx and the knot chain's records)"
    assert topo.n_levels == 4


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_bitwise_scattered_tree(hip, fam):
    locs, topo, y = scattered_tree()
    # MRA_OPT_FUSED 0: the level-by-level kernels, which read X alone (with the option on this tree is regular enough for the cascades)
    route, _ = m_against_t(hip, locs, topo, y, FAMILIES[fam], A2D, "scattered/" + fam, seed=1, opts=((2, 0),))
    assert route["path"] == "Levels", "tree (b) must be off the fused path"


def test_bitwise_scattered_tree_on_its_default_route(hip):
    locs, topo, y = scattered_tree()
    m_against_t(hip, locs, topo, y, FAMILIES["m32"], A2D, "scattered/default", seed=1)


def test_bitwise_line_with_dropped_rows(hip):
    locs, topo, y = line_tree()
    m_against_t(hip, locs, topo, y, mt.KernelSpec(mt.KIND_MATERN32, 0.2), A1D, "t1000", seed=2)


def test_bitwise_xyz_on_a_lonlat_partition(hip):
    xyz, topo, y = sphere_tree()
    m_against_t(hip, xyz, topo, y, mt.KernelSpec(mt.KIND_MATERN32, 0.5), A3D, "sphere", seed=3)


def test_bitwise_regular_tree_without_the_knot_chain(hip):
    """the cascades read the per-level kx arrays where the knot chain's packed records are not used (MRA_OPT_KNOT_CHAIN 0)"""
    locs, topo, y = grid_tree()
    spec = FAMILIES["m32"]
    pm = make_plan(hip, topo, locs, y, spec, A2D, opts=((5, 0),))
    pt = make_plan(hip, topo, twin(locs, A2D), y, spec, opts=((5, 0),))
    got, want = passes(pm), passes(pt)
    assert pm.route()["n_chain"] == 0
    for k in got:
        assert got[k].tobytes() == want[k].tobytes(), k
    pm.close()
    pt.close()


# ---- 2. state ------------------------------------------------------------------------------------------------------------------------
def _bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_a_change_of_metric_keeps_nothing(hip):
    locs, topo, y = grid_tree()
    A2 = np.array([[0.5, 0.0], [1.0, 4.0]])
    pl = make_plan(hip, topo, locs, y, FAMILIES["m32"], A2D)
    first = passes(pl)
    pl.set_metric(A2)
    second = passes(pl)
    pl.set_metric(A2D)
    third = passes(pl)
    assert _bits(first, third)
    assert not np.array_equal(first["lik"], second["lik"])
    fresh = make_plan(hip, topo, locs, y, FAMILIES["m32"], A2)
    assert _bits(second, passes(fresh))
    pl.close()
    fresh.close()


@pytest.mark.parametrize("which", ["grid", "scattered"])
def test_none_and_the_identity_are_a_plan_without_a_metric(hip, which):
    locs, topo, y = grid_tree() if which == "grid" else scattered_tree()
    spec = FAMILIES["m32"]
    plain = make_plan(hip, topo, locs, y, spec)
    want, Xraw = passes(plain), plain.buffer(13)
    pl = make_plan(hip, topo, locs, y, spec, A2D)
    passes(pl)
    pl.set_metric(None)
    assert pl.buffer(13).tobytes() == Xraw.tobytes()
    assert _bits(passes(pl), want)
    pl.set_metric(None)                                        # nothing to drop: accepted
    pl.set_metric(np.eye(2))
    assert np.array_equal(pl.buffer(13), Xraw)
    assert _bits(passes(pl), want)
    plain.close()
    pl.close()


def test_set_obs_and_set_locs_keep_the_metric(hip):
    locs, topo, y = grid_tree()
    spec = FAMILIES["m32"]
    pm = make_plan(hip, topo, locs, y, spec, A2D)
    pt = make_plan(hip, topo, twin(locs, A2D), y, spec)
    assert _bits(passes(pm), passes(pt))
    y2 = np.where(np.isfinite(y), y + 0.25, np.nan)            # new data on the same mask
    pm.set_obs(y2, R)
    pt.set_obs(y2, R)
    assert _bits(passes(pm), passes(pt))
    moved = locs * 0.75 + 0.125                                  # set_locs takes raw coordinates and transforms them again
    pm.set_locs(moved)
    pt.set_locs(twin(moved, A2D))
    assert pm.buffer(13).tobytes() == pt.buffer(13).tobytes()
    assert _bits(passes(pm), passes(pt))
    pm.close()
    pt.close()


# ---- 3. a general matrix against the oracle -------------------------------------------------------------------------------------------
GENERAL = {"aniso": (mt.aniso2d(3.0, 30.0), 0.5), "ard": (mt.ard([0.3, 0.1]), 1.0)}


def _with_metric(A, l):
    return mt.KernelSpec(mt.KIND_MATERN32, l, 1.0, A=A)


@functools.lru_cache(maxsize=None)
def general_oracle(which, jitter):
    from oracle.mra_levelwise import run_levelwise
    locs, topo, y = grid_tree(jitter=jitter)
    return run_levelwise(topo, locs, _with_metric(*GENERAL[which]), y, R)


@pytest.mark.parametrize("jitter", [False, True], ids=["grid", "jittered"])
@pytest.mark.parametrize("which", list(GENERAL))
def test_general_matrix_against_the_oracle(hip, which, jitter):
    locs, topo, y = grid_tree(jitter=jitter)
    ref = general_oracle(which, jitter)
    spec = _with_metric(*GENERAL[which])
    pl = make_plan(hip, topo, locs, y, spec, spec.A)
    pl.run(True, True)
    mean, _, sd = pl.predict(with_sd=True)
    lik = sum(pl.likelihood())
    pl.run(True, False)
    lik_only = sum(pl.likelihood())
    e = (abs(lik - ref["lik"]) / abs(ref["lik"]), float(np.max(np.abs(mean - ref["mean"]))),
         float(np.max(np.abs(sd - ref["sd"]) / np.maximum(ref["sd"], 1e-300))), abs(lik_only - ref["lik"]) / abs(ref["lik"]))
    print("%s jitter=%s: lik %.2e mean %.2e sd %.2e likelihood-only %.2e" % (which, jitter, *e))
    assert e[0] <= BARS[0] and e[1] <= BARS[1] and e[2] <= BARS[2] and e[3] <= BARS[0]
    pl.close()


def test_predictAt_at_tree_locations_is_predict(hip):
    from pymra_amd import MRATree
    locs, topo, y = grid_tree()
    A, l = GENERAL["aniso"]
    np.random.seed(7)
    tree = MRATree(locs, 16, lambda a, b: mt.Matern32(a, b, l=l, metric=A), y.reshape(-1, 1), R, M=3, J=4)
    mean, sd = tree.predict()
    rows = np.nonzero(leaf_of_callers(tree.topology) >= 0)[0][::7]
    m, s = tree.predictAt(locs[rows])
    # a site that is a tree location reproduces that row's coordinates bit for bit: the bars are those of the sites tests for own rows
    e_m, e_s = float(np.max(np.abs(m[:, 0] - np.asarray(mean).ravel()[rows]))), float(np.max(np.abs(s - sd[rows])))
    print("predictAt at %d tree locations: mean %.2e sd %.2e" % (len(rows), e_m, e_s))
    assert e_m <= BARS[1] and e_s <= BARS[1]


def test_covarianceAt_against_dense_conditioning(hip):
    import _treesites as TS
    from pymra_amd import MRATree
    n = 24
    locs = mt.genLocations2d(Nx=n, Ny=n)
    A, l = GENERAL["aniso"]
    spec = _with_metric(A, l)
    np.random.seed(7)
    topo0 = build_topology(locs, 16, 1, 4)
    y = _mask_data(topo0, locs)
    np.random.seed(7)
    tree = MRATree(locs, 16, spec, y.reshape(-1, 1), R, M=1, J=4)
    topo = tree.topology
    st = TS.SiteState(topo, locs, spec, y, R)
    lf = leaf_of_callers(topo)
    callers = np.nonzero(lf >= 0)[0]
    _, S = TS.site_prior_cov(st, locs[callers], lf[callers])                       # the MRA prior covariance of every reported location
    o = np.isfinite(y[callers])
    K_ = S[np.ix_(o, o)] + R * np.eye(int(o.sum()))
    Sp = S - S[:, o] @ np.linalg.solve(K_, S[o, :])
    pick = np.random.default_rng(3).choice(len(callers), 50, replace=False)
    sites, leaf = locs[callers[pick]], lf[callers[pick]]
    scale = float(spec.evaluate(np.zeros((1, 2)), np.zeros((1, 2)))[0, 0])
    for distr, want in (("prior", S), ("posterior", Sp)):
        got = tree.covarianceAt(sites, distr=distr, leaf=leaf)
        err = float(np.max(np.abs(got - want[np.ix_(pick, pick)])))
        print("covarianceAt %s: %.2e (scale %.2f)" % (distr, err, scale))
        assert err <= 1e-9 * scale                                                 # tests/test_gpu_cov.py: PRIOR_TOL 1e-10, _post_tol 1e-9
        assert np.array_equal(got, got.T)


# ---- 4. the model is really different -----------------------------------------------------------------------------------------------------
def test_the_anisotropic_likelihood_is_another_one(hip):
    locs, topo, y = grid_tree()
    A, l = GENERAL["aniso"]
    spec = mt.KernelSpec(mt.KIND_MATERN32, l)
    iso = make_plan(hip, topo, locs, y, spec)
    ani = make_plan(hip, topo, locs, y, spec, A)
    iso.run(True, False)
    ani.run(True, False)
    a, b = sum(iso.likelihood()), sum(ani.likelihood())
    print("isotropic %.6f anisotropic %.6f" % (a, b))
    assert abs(a - b) > 0.01 * abs(a)
    iso.close()
    ani.close()


# ---- 5. sharded ----------------------------------------------------------------------------------------------------------------------
def test_sharded_world_4_against_the_single_plan(hip):
    """the emulation of tests/_cases.py's emulate_world_on_one_gpu with set_metric on every rank"""
    from pymra_amd.sharding import shard_topology
    locs, topo, y = grid_tree()
    spec, A, world = FAMILIES["m32"], mt.aniso2d(3.0, 30.0), 4
    single = make_plan(hip, topo, locs, y, spec, A)
    single.run(True, True)
    lik1 = sum(single.likelihood())
    mean1, var1 = (v.copy() for v in single.predict())
    single.close()
    plans, bufs = [], []
    try:
        for r in range(world):
            lt, red = shard_topology(topo, world, r)
            p = hip.HipPlan(lt, 0)
            plans.append(p)
            p.set_locs(locs)
            p.set_metric(A)
            p.set_obs(y, R)
            p.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
            p.set_reduce_level(red)
            p.run(True, True, split=True)
            bufs.append(p.reduce_export())
        tot = np.sum(bufs, axis=0)
        liks, mean, var = [], np.zeros(topo.N), np.zeros(topo.N)
        for p in plans:
            p.reduce_import(tot)
            p.resume()
            liks.append(sum(p.likelihood()))
            mm, vv = p.predict()
            mean += mm
            var += vv
    finally:
        for p in plans:
            p.close()
    e = ((max(liks) - min(liks)) / abs(lik1), max(abs(v - lik1) for v in liks) / abs(lik1),
         float(np.max(np.abs(mean - mean1))), float(np.max(np.abs(var - var1))))
    print("world 4: spread %.2e lik %.2e mean %.2e var %.2e" % e)
    assert e[0] <= SPREAD and e[1] <= SINGLE_LIK and e[2] <= SINGLE_MEAN and e[3] <= SINGLE_VAR


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    locs, topo, y = grid_tree()
    pl = hip.HipPlan(topo, 0)
    with pytest.raises(hip.MraError, match="needs mra_plan_set_locs first") as e:
        pl.set_metric(A2D)
    assert e.value.code == -4
    pl.set_locs(locs)
    Xraw = pl.buffer(13)
    for bad, msg in ((np.array([[1.0, 2.0], [2.0, 4.0]]), "singular"), (np.array([[1.0, np.nan], [0.0, 1.0]]), "not finite"),
                     (np.array([[np.inf, 0.0], [0.0, 1.0]]), "not finite"), (np.zeros((2, 2)), "singular")):
        with pytest.raises(hip.MraError, match=msg) as e:
            pl.set_metric(bad)
        assert e.value.code == -1
    assert pl.buffer(13).tobytes() == Xraw.tobytes()           # checked before anything changed
    for shape in ((3, 3), (2,), (1, 1)):
        with pytest.raises(ValueError, match="2 x 2"):
            pl.set_metric(np.ones(shape))
    # MRA_KERNEL_HOST, in both orders
    pl.set_obs(y, R)
    pl.set_metric(A2D)
    with pytest.raises(hip.MraError, match="MRA_KERNEL_HOST on a plan with a metric"):
        pl.set_kernel_host()
    pl.set_metric(None)
    pl.set_kernel_host()
    with pytest.raises(hip.MraError, match="MRA_KERNEL_HOST plans never read coordinates"):
        pl.set_metric(A2D)
    pl.close()
    # a circular kernel, in both orders (1-D)
    l1, t1, y1 = line_tree()
    pl = hip.HipPlan(t1, 0)
    pl.set_locs(l1)
    pl.set_obs(y1, R)
    pl.set_kernel(mt.KIND_EXP, 0.2, circular=True)
    with pytest.raises(hip.MraError, match="the kernel is circular"):
        pl.set_metric(A1D)
    pl.set_kernel(mt.KIND_EXP, 0.2)
    pl.set_metric(A1D)
    with pytest.raises(hip.MraError, match="circular distances on a plan with a metric"):
        pl.set_kernel(mt.KIND_EXP, 0.2, circular=True)
    pl.run(True, False)                                         # the refused call left the plan usable
    assert np.isfinite(sum(pl.likelihood()))
    pl.close()


# ---- 7. the MRATree surface -----------------------------------------------------------------------------------------------------------
def _lik(tree):
    return float(tree.getLikelihood()[0, 0])


def test_mratree_constructor_and_reevaluate(hip):
    from pymra_amd import MRATree
    locs, _, y = grid_tree()
    yo = y.reshape(-1, 1)

    def cov(l, ratio, angle):
        return lambda a, b: mt.Matern32(a, b, l=l, metric=mt.aniso2d(ratio, angle))

    points = [(0.5, 3.0, 30.0), (0.4, 2.0, 75.0), (0.6, 1.5, -20.0)]
    np.random.seed(7)
    tree = MRATree(locs, 16, cov(*points[0]), yo, R, M=3, J=4)
    assert np.array_equal(tree.kernel.A, mt.aniso2d(3.0, 30.0))
    for k, (l, ratio, angle) in enumerate(points):
        if k:
            tree.reevaluate(cov(l, ratio, angle), want_predict=True)
        mean, sd = tree.predict()
        # a fresh tree on pre-transformed covariance coordinates: the same partition (locs), the isotropic kernel
        np.random.seed(7)
        fresh = MRATree(locs, 16, lambda a, b: mt.Matern32(a, b, l=l), yo, R, M=3, J=4, cov_locs=locs @ mt.aniso2d(ratio, angle).T)
        m2, s2 = fresh.predict()
        e = (abs(_lik(tree) - _lik(fresh)) / abs(_lik(fresh)), float(np.max(np.abs(np.asarray(mean) - np.asarray(m2)))),
             float(np.max(np.abs(sd - s2) / np.maximum(s2, 1e-300))))
        print("reevaluate %s: lik %.2e mean %.2e sd %.2e" % ((l, ratio, angle), *e))
        assert e[0] <= BARS[0] and e[1] <= BARS[1] and e[2] <= BARS[2]
    iso = tree.reevaluate(lambda a, b: mt.Matern32(a, b, l=0.5))                   # no metric any more: None goes to the plan
    np.random.seed(7)
    plain = MRATree(locs, 16, lambda a, b: mt.Matern32(a, b, l=0.5), yo, R, M=3, J=4, want_predict=False)
    assert float(iso[0, 0]) == _lik(plain)
    with pytest.raises(ValueError, match="2 x 2"):
        MRATree(locs, 16, lambda a, b: mt.Matern32(a, b, l=0.5, metric=np.eye(3)), yo, R, M=3, J=4)
    with pytest.raises(ValueError, match="2 x 2"):
        tree.reevaluate(lambda a, b: mt.Matern32(a, b, l=0.5, metric=np.eye(3)))


def test_mratree_chordal_with_a_3x3_metric(hip):
    from oracle.mra_levelwise import run_levelwise
    from pymra_amd import MRATree
    n = 48
    lon = -180.0 + (np.arange(n) + 0.5) * 360.0 / n
    g, h = np.meshgrid(lon, np.linspace(-80.0, 80.0, n))
    ll = np.column_stack((g.ravel(), h.ravel()))
    xyz = mt.lonlat_to_xyz(ll)
    A = np.diag([1.0, 1.0, 2.5])                                 # a shorter range along the axis of rotation
    np.random.seed(7)
    y = _mask_data(build_topology(ll, 16, 2, 4, coord_dim=3), xyz, seed=3)
    np.random.seed(7)
    tree = MRATree(ll, 16, lambda a, b: mt.Matern32(a, b, l=0.5, metric=A), y.reshape(-1, 1), R, M=2, J=4, metric="chordal")
    ref = run_levelwise(tree.topology, xyz, mt.KernelSpec(mt.KIND_MATERN32, 0.5, A=A), y, R)
    mean, sd = tree.predict()
    e = (abs(_lik(tree) - ref["lik"]) / abs(ref["lik"]), float(np.max(np.abs(np.asarray(mean).ravel() - ref["mean"]))),
         float(np.max(np.abs(sd - ref["sd"]) / np.maximum(ref["sd"], 1e-300))))
    print("chordal with A: lik %.2e mean %.2e sd %.2e" % e)
    assert e[0] <= BARS[0] and e[1] <= BARS[1] and e[2] <= BARS[2]
    rows = np.nonzero(leaf_of_callers(tree.topology) >= 0)[0][::11]
    m, s = tree.predictAt(ll[rows])                              # sites stay (lon, lat)
    assert float(np.max(np.abs(m[:, 0] - np.asarray(mean).ravel()[rows]))) <= BARS[1]
    with pytest.raises(ValueError, match="3 x 3"):
        MRATree(ll, 16, lambda a, b: mt.Matern32(a, b, l=0.5, metric=np.eye(2)), y.reshape(-1, 1), R, M=2, J=4, metric="chordal")
