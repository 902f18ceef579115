"""mra_plan_fit_laplace on the GPU: Poisson, binomial and Gaussian data by a Laplace approximation.

1. T16, Poisson with offsets and binomial with varying trials, against the dense twin of the iteration (tests/_laplace.py);
2. the Gaussian family is set_obs(z - offset, aux), bit for bit; 3. one cell each of the Fused, level-by-level and Hi routes and
a leaf of 193 observations: the fixed point and a fresh plan given (t, r); 4. the 1-D tree t201, whose partition drops rows;
5. an opaque callable (MRA_KERNEL_HOST); 6. a warm start; 7. the calls on the retained factors after a fit; 8. refusals;
9. MRATree.fitLaplace.

Trees, masks and expected routes are those of tests/_route_cells.py; bars are ORACLE_BARS and ROUTE_BARS of
tests/test_gpu_routes.py (Newton's map has zero derivative at its fixed point, so a pass's error is not amplified), and for the calls
on the retained factors the bars of their own GPU tests."""
import ctypes as C

import numpy as np
import pytest

import _cases as K
import _laplace as LP
import _noise as NZ
import _route_cells as RC
import test_gpu_likelihood_masks as MK
import test_gpu_routes as TR

pytestmark = pytest.mark.gpu

LEVELS = ((2, 0),)
TOL = 1e-10
STATE, INVALID = -4, -1


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _expect(key, recipe, opts):
    hit = [c["expect"] for c in RC.CELLS if (c["tree"], c["mask"], c["predict"], c["opts"]) == (key, recipe, True, tuple(opts))]
    assert len(hit) == 1, (key, recipe, opts)
    return hit[0]


def _seen(topo, z):
    """bool[N]: rows the plan observes - a finite datum at a row some leaf reports"""
    return np.isfinite(np.asarray(z).ravel()) & NZ.reported(topo)


def _caller(topo, buf):
    """a padded buffer in the caller's row order (0 at rows outside every leaf)"""
    rows = (topo.perm >= 0) & np.asarray(topo.in_leaf, dtype=bool)
    out = np.zeros(topo.N)
    out[topo.perm[rows]] = buf[rows]
    return out


def _state(pl):
    """(d + u, mean, sd) of the last pass, as the plan holds it (no pass is run)"""
    mean, _, sd = pl.predict(with_sd=True)
    return sum(pl.likelihood()), mean.copy(), sd.copy()


def _fit(pl, family, z, aux, offset, **kw):
    kw.setdefault("tol", TOL)
    return pl.fit_laplace(LP.NAMES[family], z, aux=aux, offset=offset, **kw)


def _same(a, b, tag):
    assert a[0] == b[0], "%s: likelihood %r != %r" % (tag, a[0], b[0])
    assert np.array_equal(a[1], b[1]), tag + ": mean"
    assert np.array_equal(a[2], b[2]), tag + ": sd"


def _y_mask(z):
    """the mask as set_obs takes it: 0 where z is finite, NaN elsewhere"""
    return np.where(np.isfinite(z), 0.0, np.nan).reshape(-1, 1)


# ---- 1. T16 against the dense twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [LP.POISSON, LP.BINOMIAL], ids=["poisson", "binomial"])
def test_t16_against_the_dense_twin(hip, family):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, ref = LP.t16_fit(family)
    pl = MK._plan(hip, topo, locs, y)
    res = _fit(pl, family, z, aux, offset)
    TR._check_route(pl, _expect("T16", RC.CLOUD, ()), "T16")
    got = _state(pl)
    print("%s: passes %d (dense %d), step %.2e" % (LP.NAMES[family], res["passes"], ref["info"][5], res["step"]))
    TR._against(topo, counts, got, (ref["info"][0] + ref["info"][1], ref["mean"], ref["sd"]), TR.ORACLE_BARS, "T16 %s vs dense" % LP.NAMES[family])
    for k in range(5):
        e = abs(res["info"][k] - ref["info"][k]) / abs(ref["info"][k])
        print("info[%d]: %.10f vs %.10f, rel %.2e" % (k, res["info"][k], ref["info"][k], e))
        assert e <= TR.ORACLE_BARS[0], "info[%d] rel err %.3e" % (k, e)
    assert abs(res["lik"] - ref["lik"]) <= TR.ORACLE_BARS[0] * abs(ref["lik"])
    assert res["info"][7] == 1.0 and res["converged"] is True
    assert res["passes"] == int(ref["info"][5])
    assert (res["d"], res["u"]) == pl.likelihood()
    pl.close()


# ---- 2. the Gaussian family ----------------------------------------------------------------------------------------------------------
def test_gaussian_family_is_set_obs_bit_for_bit(hip):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, ref = LP.t16_fit(LP.GAUSSIAN)
    assert aux[obs].max() > 2.0 * aux[obs].min()
    pl = MK._plan(hip, topo, locs, y)
    res = _fit(pl, LP.GAUSSIAN, z, aux, offset)
    assert res["info"][5] == 2 and res["info"][6] == 0.0 and res["info"][7] == 1.0
    got = _state(pl)
    fresh = hip.HipPlan(topo, 0)
    s = MK._spec()
    fresh.set_locs(locs); fresh.set_obs((z - offset).reshape(-1, 1), aux); fresh.set_kernel(s.kind, s.l, s.sig, s.scale)
    want = TR._predict(fresh)
    assert (res["d"], res["u"]) == fresh.likelihood()
    _same(got, want, "gaussian family vs set_obs(z - offset, aux)")
    n = int(o.sum())
    full = res["d"] + res["u"] + n * np.log(2 * np.pi)
    print("gaussian: lik %.12f, d + u + n log 2 pi %.12f" % (res["lik"], full))
    assert abs(res["lik"] - full) <= 1e-12 * abs(full)
    fresh.close(); pl.close()


# ---- 3. / 4. routes, a leaf of 193 observations, a 1-D tree with dropped rows ---------------------------------------------------------
def _fixed_point_and_fresh_plan(hip, pl, topo, locs, spec, z, offset, res, tag):
    """the checks without a dense oracle: convergence, t = x^ + g(eta^) / D(eta^) at the observed rows, and a fresh plan given (t, r)"""
    print("%s: passes %d, step %.2e" % (tag, res["passes"], res["step"]))
    assert res["info"][7] == 1.0, tag
    seen = _seen(topo, z)
    got = _state(pl)
    xh = got[1][seen]
    t, r = _caller(topo, pl.buffer(11)), _caller(topo, pl.buffer(10))
    g, D, _ = LP.terms(LP.POISSON, z[seen], 1.0, xh + offset[seen])
    e_t = np.abs(t[seen] - (xh + g / D)) / np.maximum(1.0, np.abs(xh))
    print("%s: fixed point %.2e" % (tag, e_t.max()))
    assert e_t.max() <= 10 * TOL, tag
    assert np.all(r[seen] > 0) and np.all(r[~seen] == 0)
    assert r[seen].max() < 2.0 ** 20, tag                             # D = 1 / r > 2^-20: the floor on D is not what this measures
    fresh = hip.HipPlan(topo, 0)
    fresh.set_locs(locs); fresh.set_obs(np.where(seen, t, np.nan).reshape(-1, 1), np.where(seen, r, np.nan))
    fresh.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
    return got, fresh


@pytest.mark.parametrize("key,recipe,opts", [("A", RC.CLOUD, ()), ("A", RC.CLOUD, LEVELS), ("H", RC.CLOUD, ()), ("A", RC.E193, ())],
                         ids=["A-fused", "A-levels", "H-hi", "A-193"])
def test_routes_fixed_point_and_fresh_plan(hip, key, recipe, opts):
    topo, locs = TR._tree(key)
    obs = RC.make_obs(topo, locs, recipe)
    if recipe == RC.E193:
        assert MK.leaf_counts(topo, obs)[0] == 0                      # an empty first leaf
    z, _, offset = LP.inputs(locs, obs, LP.POISSON)
    tag = "%s %s %s" % (key, recipe, opts)
    pl = MK._plan(hip, topo, locs, _y_mask(z))
    TR._set(pl, opts)
    res = _fit(pl, LP.POISSON, z, None, offset, max_iter=30)
    expect = _expect(key, recipe, opts)
    TR._check_route(pl, expect, tag)
    got, fresh = _fixed_point_and_fresh_plan(hip, pl, topo, locs, MK._spec(), z, offset, res, tag)
    TR._set(fresh, opts)
    want = TR._predict(fresh)
    TR._check_route(fresh, expect, tag + " fresh plan")
    assert (res["d"], res["u"]) == fresh.likelihood(), tag
    _same(got, want, tag + " vs a fresh plan given (t, r)")
    fresh.close(); pl.close()


def test_1d_tree_with_dropped_rows(hip):
    cs = K.load_case("t201")
    topo, locs, y, spec, R1 = cs["topo"], cs["locs"], cs["y_obs"], cs["spec"], float(cs["c"]["R"])
    rep = NZ.reported(topo)
    obs = np.isfinite(np.asarray(y).ravel())
    assert not rep.all() and (obs & ~rep).any()                       # data at rows outside every leaf: ignored
    z, _, offset = LP.inputs(locs, obs, LP.POISSON)
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, R1); pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale, spec.circular)
    res = _fit(pl, LP.POISSON, z, None, offset, max_iter=30)
    got, fresh = _fixed_point_and_fresh_plan(hip, pl, topo, locs, spec, z, offset, res, "t201")
    fresh.set_kernel(spec.kind, spec.l, spec.sig, spec.scale, spec.circular)
    want = TR._predict(fresh)
    assert (res["d"], res["u"]) == fresh.likelihood()
    _same(got, want, "t201 vs a fresh plan given (t, r)")
    assert np.all(got[1][~rep] == 0.0)
    # the data at the dropped rows are nobody's: other values there, the same bits
    z2 = z.copy()
    z2[obs & ~rep] += 5.0
    res2 = _fit(pl, LP.POISSON, z2, None, offset, max_iter=30)
    assert np.array_equal(res2["info"], res["info"])
    _same(_state(pl), got, "t201 with other data at the dropped rows")
    fresh.close(); pl.close()


# ---- 5. / 6. an opaque callable; a warm start ------------------------------------------------------------------------------------------
def test_opaque_callable(hip):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, _ = LP.t16_fit(LP.POISSON)
    s = MK._spec()
    cov = lambda a, b: np.asarray(s.evaluate(a, b))                   # noqa: E731  (opaque: evaluated on the host, block by block)
    dev = MK._plan(hip, topo, locs, y)
    want_res = _fit(dev, LP.POISSON, z, aux, offset)
    want = _state(dev)
    dev.close()
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, MK.R); pl.upload_host_cov(cov, locs, y)
    res = _fit(pl, LP.POISSON, z, aux, offset)                         # keeps the blocks (set_obs would drop them)
    TR._check_route(pl, dict(path="Levels"), "T16 host covariance")
    TR._against(topo, counts, _state(pl), want, TR.ROUTE_BARS, "T16 host covariance vs the device kernel")
    assert abs(res["lik"] - want_res["lik"]) <= TR.ROUTE_BARS[0] * abs(want_res["lik"])
    assert res["converged"] and res["passes"] == want_res["passes"]
    pl.close()


@pytest.mark.parametrize("family", [LP.POISSON, LP.BINOMIAL], ids=["poisson", "binomial"])
def test_warm_start_from_the_converged_mean(hip, family):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, _ = LP.t16_fit(family)
    pl = MK._plan(hip, topo, locs, y)
    cold = _fit(pl, family, z, aux, offset)
    want = _state(pl)
    warm = _fit(pl, family, z, aux, offset, x0=want[1])
    print("%s: cold %d passes, warm %d passes, step %.2e" % (LP.NAMES[family], cold["passes"], warm["passes"], warm["step"]))
    assert warm["converged"] and warm["passes"] <= 2
    TR._against(topo, counts, _state(pl), want, TR.ROUTE_BARS, "warm start vs the cold fit")
    assert abs(warm["lik"] - cold["lik"]) <= TR.ROUTE_BARS[0] * abs(cold["lik"])
    pl.close()


# ---- 7. the calls on the retained factors serve the Laplace posterior -----------------------------------------------------------------
def test_retained_factor_calls_after_a_fit(hip):
    import test_sites_cpu as SC
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, _ = LP.t16_fit(LP.POISSON)
    pl = MK._plan(hip, topo, locs, y)
    _fit(pl, LP.POISSON, z, aux, offset)
    lik, mean, sd = _state(pl)
    var = pl.predict()[1]
    scale = MK._spec().sig                                            # the prior variance: the scale of Sigma
    rows_ok = (topo.perm >= 0) & np.asarray(topo.in_leaf, dtype=bool)
    # solve(t) is the mean: tests/test_gpu_solve.py, 1e-9 * max(1, |mean|)
    t = pl.buffer(11)
    m, quad = pl.solve(np.where(np.isfinite(t), t, 0.0).reshape(1, -1))
    e_m = np.abs(_caller(topo, m[0]) - mean).max()
    print("solve(t): mean %.2e, quad %.2e" % (e_m, abs(quad[0, 0] - pl.likelihood()[1])))
    assert e_m <= 1e-9 * max(1.0, np.abs(mean).max())
    assert abs(quad[0, 0] - pl.likelihood()[1]) <= 1e-9 * abs(quad[0, 0])
    # the posterior covariance applied to 16 unit vectors has var on its diagonal: tests/test_gpu_cov.py, 1e-9 * scale
    pick = np.nonzero(rows_ok)[0][::251][:16]
    assert len(pick) == 16
    A = np.zeros((16, topo.P))
    A[np.arange(16), pick] = 1.0
    out, _ = pl.cov_apply(A, posterior=True)
    e_v = np.abs(out[np.arange(16), pick] - var[topo.perm[pick]]).max()
    print("cov_apply: var %.2e" % e_v)
    assert e_v <= 1e-9 * scale
    # 48 tree rows as sites of their own leaf: tests/test_gpu_sites.py, 1e-8 on the mean and 1e-9 on the variance
    rows = np.nonzero(rows_ok)[0][::85][:48]
    assert len(rows) == 48
    X = np.asarray(locs, float)
    sm, sv = pl.predict_sites(X[topo.perm[rows]], SC.leaf_of_rows(topo)[rows])
    e_m, e_v = np.abs(sm[0] - mean[topo.perm[rows]]).max(), np.abs(sv - var[topo.perm[rows]]).max()
    print("48 own rows: mean %.2e var %.2e" % (e_m, e_v))
    assert e_m <= 1e-8 * max(1.0, np.abs(mean).max()) and e_v <= 1e-9 * scale
    # likelihood() and predict() are what the fit left
    _same(_state(pl), (lik, mean, sd), "after the calls on the retained factors")
    pl.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_in_order_and_the_plan_unchanged(hip):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, _ = LP.t16_fit(LP.BINOMIAL)
    zg, auxg, offg, _ = LP.t16_fit(LP.GAUSSIAN)
    s = MK._spec()
    who = "mra_plan_fit_laplace"

    def refused(pl, code, starts, family, z_, aux_=None, off_=None, x0_=None, max_iter=50, tol=TOL):
        with pytest.raises(hip.MraError) as ei:
            pl.fit_laplace(family, z_, aux=aux_, offset=off_, x0=x0_, max_iter=max_iter, tol=tol)
        assert ei.value.code == code, (starts, str(ei.value))
        assert starts in str(ei.value) and who in str(ei.value), (starts, str(ei.value))

    pl = hip.HipPlan(topo, 0)
    # the state comes before the arguments
    refused(pl, STATE, who + " needs set_locs, set_obs and set_kernel first", 7, z, max_iter=0)
    pl.set_locs(locs)
    refused(pl, STATE, who + " needs", "poisson", z)
    pl.set_obs(y, MK.R)
    refused(pl, STATE, who + " needs", "poisson", z)
    pl.set_kernel(s.kind, s.l, s.sig, s.scale)
    before = TR._predict(pl)
    noise_before = pl.buffer(10)

    def unchanged(tag):
        _same(TR._predict(pl), before, "after the refusal: " + tag)
        assert np.array_equal(pl.buffer(10), noise_before), tag

    first, hole = np.nonzero(obs)[0][0], np.nonzero(~obs)[0][0]
    bad = lambda a, i, v: np.concatenate([a[:i], [v], a[i + 1:]])      # noqa: E731
    cases = [
        ("unknown family", (7, bad(z, first, np.nan)), dict(max_iter=0)),                    # ... and the family before everything else
        ("z is not finite exactly where the plan observes", ("poisson", bad(z, first, np.nan)), dict()),
        ("z is not finite exactly where the plan observes", ("poisson", bad(z, hole, 1.0)), dict()),
        ("z is not finite exactly where the plan observes", ("poisson", bad(bad(z, first, np.inf), hole, -1.0)), dict()),
        ("z < 0", ("poisson", bad(z, first, -1.0)), dict(max_iter=0)),
        ("binomial trials aux < z or aux <= 0", ("binomial", z, bad(aux, first, z[first] - 1.0)), dict()),
        ("binomial trials aux < z or aux <= 0", ("binomial", bad(z, first, 0.0), bad(aux, first, 0.0)), dict()),
        ("Gaussian variance aux <= 0", ("gaussian", zg, bad(auxg, first, 0.0), offg), dict()),
        ("aux is not finite", ("binomial", z, bad(aux, first, np.inf)), dict()),
        ("aux is not finite", ("gaussian", zg, bad(auxg, first, np.nan)), dict()),
        ("offset is not finite", ("poisson", z, None, bad(np.zeros(topo.N), first, np.nan)), dict(tol=0.0)),
        ("x0 is not finite", ("poisson", z, None, None, bad(np.zeros(topo.N), first, np.inf)), dict()),
        ("max_iter < 1", ("poisson", z), dict(max_iter=0, tol=0.0)),
        ("tol must be greater than 0", ("poisson", z), dict(tol=0.0)),
        ("tol must be greater than 0", ("poisson", z), dict(tol=float("nan"))),
        ("aux is NULL", ("binomial", z), dict()),
    ]
    for starts, args, kw in cases:
        refused(pl, INVALID, who + ": " + starts, *args, **kw)
        unchanged(starts)
    # NULL z or info: the raw export
    zp = np.ascontiguousarray(np.where(topo.perm >= 0, z[topo.src], np.nan))
    info = np.zeros(8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    for zq, iq in ((None, ptr(info)), (ptr(zp), None)):
        assert pl.lib.mra_plan_fit_laplace(pl._h, 1, zq, None, None, None, 50, TOL, iq) == INVALID
        assert pl.lib.mra_last_error(pl._h).decode().startswith(who + ": z or info is NULL")
        unchanged("NULL")
    assert pl.lib.mra_plan_fit_laplace(pl._h, 1, None, None, None, None, 0, TOL, ptr(info)) == INVALID
    assert pl.lib.mra_last_error(pl._h).decode().startswith(who + ": max_iter < 1")               # the stated order
    # a sharded plan, last
    pl.set_reduce_level(0)
    refused(pl, INVALID, who + ": sharded plans", "poisson", z)
    refused(pl, INVALID, who + ": tol must be greater than 0", "poisson", z, tol=0.0)
    pl.set_reduce_level(-1)
    unchanged("sharded")
    # values that are never read may be anything
    res = pl.fit_laplace("binomial", z, aux=bad(aux, hole, np.nan), offset=bad(np.zeros(topo.N), hole, np.inf), tol=TOL)
    assert res["converged"]
    # not converged within max_iter: MRA_OK with info[7] = 0
    res = pl.fit_laplace("poisson", z, max_iter=2, tol=TOL)
    assert res["passes"] == 2 and res["info"][7] == 0.0 and res["step"] > TOL
    # set_obs returns the plan to the Gaussian model
    pl.set_obs(y, MK.R)
    _same(TR._predict(pl), before, "set_obs after a fit")
    pl.close()


# ---- 9. MRATree ------------------------------------------------------------------------------------------------------------------------
def test_mratree_fit_laplace(hip):
    import pymra_amd
    import pymra_amd.MRATools as mt
    n, r0, M = RC.TREES["T16"]
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, _ = LP.t16_fit(LP.POISSON)
    s = MK._spec()
    pl = MK._plan(hip, topo, locs, y)
    want_res = _fit(pl, LP.POISSON, z, aux, offset, tol=1e-10)
    want = _state(pl)
    pl.close()
    cov = lambda a, b: mt.Matern32(a, b, l=s.l, sig=s.sig)           # noqa: E731
    np.random.seed(7)                                                 # as MK._tree does: the same knots
    mt.genLocations2d(Nx=n, Ny=n)
    tree = pymra_amd.MRATree(locs, r0, cov, z.reshape(-1, 1), MK.R, M=M, J=4)
    assert np.array_equal(tree.topology.knot_rows, topo.knot_rows)
    lik = tree.fitLaplace("poisson", offset=offset)                  # z: the tree's obs
    assert lik == want_res["lik"]
    mean, sd = tree.predict()
    assert np.array_equal(np.asarray(mean).ravel(), want[1]) and np.array_equal(np.asarray(sd).ravel(), want[2])
    assert float(np.asarray(tree.getLikelihood()).ravel()[0]) == want_res["d"] + want_res["u"]
    assert tree.laplace["passes"] == want_res["passes"]
    # another cov: set without a pass of its own, started from the previous mean
    cov2 = lambda a, b: mt.Matern32(a, b, l=1.1 * s.l, sig=s.sig)     # noqa: E731
    lik2 = tree.fitLaplace("poisson", offset=offset, cov=cov2)
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, MK.R); pl.set_kernel(s.kind, 1.1 * s.l, s.sig, s.scale)
    warm = _fit(pl, LP.POISSON, z, aux, offset, x0=want[1])
    cold = _fit(pl, LP.POISSON, z, aux, offset)
    pl.close()
    print("second cov: warm %d passes, cold %d" % (warm["passes"], cold["passes"]))
    assert lik2 == warm["lik"] and tree.laplace["passes"] == warm["passes"] and np.array_equal(tree.laplace["info"], warm["info"])
    assert abs(lik2 - lik) > 1e-6 * abs(lik)
    with pytest.raises(NotImplementedError):
        tree.fitLaplace("poisson", offset=offset, cov=lambda a, b: np.exp(-np.abs(a - b.T)))
    with pytest.raises(ValueError):
        tree.fitLaplace("gamma")
