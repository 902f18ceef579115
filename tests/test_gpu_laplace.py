"""mra_plan_fit_laplace on the GPU: Poisson, binomial and Gaussian data by a Laplace approximation.

1. T16, Poisson with offsets and binomial with varying trials, against the dense twin of the iteration (tests/_laplace.py);
2. the Gaussian family is set_obs(z - offset, aux), bit for bit; 3. one cell each of the Fused, level-by-level and Hi routes and
a leaf of 193 observations: the fixed point and a fresh plan given (t, r); 4. the 1-D tree t201, whose partition drops rows;
5. an opaque callable (MRA_KERNEL_HOST); 6. a warm start; 7. the calls on the retained factors after a fit; 8. refusals;
9. MRATree.fitLaplace; 10. laplace_term from eta = -700 to 700 against 50 digits; 11. the floor on D and saturated probabilities
against the dense twin; 12. an iterate that leaves the doubles is refused, never converged.  3. and 4. run the Poisson and the
binomial family, and one more pass from the converged mean whose info[2..4] and step are recomputed from arrays.

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
def _fixed_point_and_fresh_plan(hip, pl, topo, locs, spec, family, z, aux, offset, res, tag):
    """the checks without a dense oracle: convergence, t = x^ + g(eta^) / D(eta^) at the observed rows, and a fresh plan given (t, r)"""
    print("%s: passes %d, step %.2e" % (tag, res["passes"], res["step"]))
    assert res["info"][7] == 1.0, tag
    seen = _seen(topo, z)
    got = _state(pl)
    xh = got[1][seen]
    t, r = _caller(topo, pl.buffer(11)), _caller(topo, pl.buffer(10))
    g, D, _ = LP.terms(family, z[seen], 1.0 if aux is None else aux[seen], xh + (0.0 if offset is None else offset[seen]))
    e_t = np.abs(t[seen] - (xh + g / D)) / np.maximum(1.0, np.abs(xh))
    print("%s: fixed point %.2e" % (tag, e_t.max()))
    assert e_t.max() <= 10 * TOL, tag
    assert np.all(r[seen] > 0) and np.all(r[~seen] == 0)
    assert r[seen].max() < 2.0 ** 20, tag                             # D = 1 / r > 2^-20: the floor on D is not what this measures
    fresh = hip.HipPlan(topo, 0)
    fresh.set_locs(locs); fresh.set_obs(np.where(seen, t, np.nan).reshape(-1, 1), np.where(seen, r, np.nan))
    fresh.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
    return got, fresh


def _info_of_one_more_pass(pl, topo, family, z, aux, offset, x0, tag):
    """One pass from a copy of the converged mean: only here is the linearisation point known outside the library, so only here
    can info[2..4] and the step be recomputed from arrays (LP.recompute_info).  Bars: INFO_ULPS eps x the sum of the absolute
    values of a sum's terms - a term passes through at most 34 roundings on its way into a sum (tests/test_gpu_fullsize.py has the
    count), and exp, log and lgamma are good to a few ulp; the step is a maximum and has no rounding."""
    res = _fit(pl, family, z, aux, offset, x0=x0, max_iter=1)
    seen = _seen(topo, z)
    mean = pl.predict()[0]
    rc = LP.recompute_info(family, z, aux, offset, x0, mean, _caller(topo, pl.buffer(11)), _caller(topo, pl.buffer(10)), seen)
    for k, key in ((2, "info2"), (3, "info3"), (4, "info4")):
        e = abs(res["info"][k] - rc[key]) / (LP.EPS * rc["S"][k - 2])
        print("%s: info[%d] %.10f recomputed %.10f: %.2f eps x sum |term|" % (tag, k, res["info"][k], rc[key], e))
        assert e <= INFO_ULPS, "%s: info[%d]" % (tag, k)
    assert res["passes"] == 1 and res["info"][6] == rc["step"], tag
    assert res["info"][7] == float(rc["step"] <= TOL * max(1.0, rc["max_xhat"])), tag
    return res


INFO_ULPS = 128
ROUTE_CELLS = [("A", RC.CLOUD, ()), ("A", RC.CLOUD, LEVELS), ("H", RC.CLOUD, ()), ("A", RC.E193, ())]
ROUTE_IDS = ["A-fused", "A-levels", "H-hi", "A-193"]


def _route_cell(hip, key, recipe, opts, family):
    topo, locs = TR._tree(key)
    obs = RC.make_obs(topo, locs, recipe)
    if recipe == RC.E193:
        assert MK.leaf_counts(topo, obs)[0] == 0                      # an empty first leaf
    z, aux, offset = LP.inputs(locs, obs, family)
    tag = "%s %s %s %s" % (key, recipe, opts, LP.NAMES[family])
    pl = MK._plan(hip, topo, locs, _y_mask(z))
    TR._set(pl, opts)
    res = _fit(pl, family, z, aux, offset, max_iter=30)
    expect = _expect(key, recipe, opts)
    TR._check_route(pl, expect, tag)
    got, fresh = _fixed_point_and_fresh_plan(hip, pl, topo, locs, MK._spec(), family, z, aux, offset, res, tag)
    TR._set(fresh, opts)
    want = TR._predict(fresh)
    TR._check_route(fresh, expect, tag + " fresh plan")
    assert (res["d"], res["u"]) == fresh.likelihood(), tag
    _same(got, want, tag + " vs a fresh plan given (t, r)")
    _info_of_one_more_pass(pl, topo, family, z, aux, offset, got[1].copy(), tag)
    TR._check_route(pl, expect, tag + " one more pass")
    fresh.close(); pl.close()


@pytest.mark.parametrize("key,recipe,opts", ROUTE_CELLS, ids=ROUTE_IDS)
def test_routes_fixed_point_and_fresh_plan(hip, key, recipe, opts):
    _route_cell(hip, key, recipe, opts, LP.POISSON)


@pytest.mark.parametrize("key,recipe,opts", ROUTE_CELLS, ids=ROUTE_IDS)
def test_routes_fixed_point_and_fresh_plan_binomial(hip, key, recipe, opts):
    _route_cell(hip, key, recipe, opts, LP.BINOMIAL)


def _t201(hip, family):
    cs = K.load_case("t201")
    topo, locs, y, spec, R1 = cs["topo"], cs["locs"], cs["y_obs"], cs["spec"], float(cs["c"]["R"])
    rep = NZ.reported(topo)
    obs = np.isfinite(np.asarray(y).ravel())
    assert not rep.all() and (obs & ~rep).any()                       # data at rows outside every leaf: ignored
    z, aux, offset = LP.inputs(locs, obs, family)
    tag = "t201 " + LP.NAMES[family]
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, R1); pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale, spec.circular)
    res = _fit(pl, family, z, aux, offset, max_iter=30)
    got, fresh = _fixed_point_and_fresh_plan(hip, pl, topo, locs, spec, family, z, aux, offset, res, tag)
    fresh.set_kernel(spec.kind, spec.l, spec.sig, spec.scale, spec.circular)
    want = TR._predict(fresh)
    assert (res["d"], res["u"]) == fresh.likelihood()
    _same(got, want, tag + " vs a fresh plan given (t, r)")
    assert np.all(got[1][~rep] == 0.0)
    # the data at the dropped rows are nobody's: other values there, the same bits
    z2 = z.copy()
    z2[obs & ~rep] += 5.0
    res2 = _fit(pl, family, z2, aux, offset, max_iter=30)                # (binomial: aux < z2 there, and nobody looks)
    assert np.array_equal(res2["info"], res["info"])
    _same(_state(pl), got, tag + " with other data at the dropped rows")
    _info_of_one_more_pass(pl, topo, family, z, aux, offset, got[1].copy(), tag)
    fresh.close(); pl.close()


def test_1d_tree_with_dropped_rows(hip):
    _t201(hip, LP.POISSON)


def test_1d_tree_with_dropped_rows_binomial(hip):
    _t201(hip, LP.BINOMIAL)


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


# ---- 10. laplace_term across the range -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [LP.GAUSSIAN, LP.POISSON, LP.BINOMIAL], ids=["gaussian", "poisson", "binomial"])
def test_laplace_term_across_the_range(hip, family):
    """One linearisation at x0 = a grid of eta over T16's observed rows (LP.term_cases: +-0, +-2^-60, the edge of the floor, +-700,
    z = 0, z at its upper end and z ~ its mean), t and r against 50 digits.  r relatively; t in units of |x| + (|z| + m) / D, the
    terms that cancel in it.  Bar: four times the error of the float64 statement on the same grid (tests/test_laplace_cpu.py
    asserts that one), and not below 8 eps.  The step of the pass is a maximum and is compared exactly."""
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    e = LP.term_errors(family, int(o.sum()), LP.t16_upper_knots())
    zN, auxN, xN = np.full(topo.N, np.nan), np.ones(topo.N), np.zeros(topo.N)
    zN[o], auxN[o], xN[o] = e["z"], e["aux"], e["x"]
    pl = MK._plan(hip, topo, locs, y)
    res = _fit(pl, family, zN, auxN, None, x0=xN, max_iter=1)
    t, r = _caller(topo, pl.buffer(11)), _caller(topo, pl.buffer(10))
    e_t, e_r = LP.err_mp(t[o], e["t"], e["unit"]), LP.err_mp(r[o], e["r"], e["r"])
    bar_t, bar_r = max(8 * LP.EPS, 4 * e["e_t"]), max(8 * LP.EPS, 4 * e["e_r"])
    print("%s: t %.2f eps (float64 %.2f, bar %.2f), r %.2f eps (float64 %.2f, bar %.2f)"
          % (LP.NAMES[family], e_t / LP.EPS, e["e_t"] / LP.EPS, bar_t / LP.EPS, e_r / LP.EPS, e["e_r"] / LP.EPS, bar_r / LP.EPS))
    assert e_t <= bar_t and e_r <= bar_r
    assert np.all(r[~o] == 0.0) and (r[o] == 2.0 ** 40).sum() >= 100
    mean = pl.predict()[0]
    assert np.all(np.isfinite(mean))
    assert res["passes"] == 1 and res["info"][6] == np.abs(mean[o] - xN[o]).max()
    pl.close()


# ---- 11. the floor on D and saturated probabilities against the dense twin -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_exposure", "saturated", "gauss_floor"])
def test_floor_and_saturation_against_the_dense_twin(hip, name):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    family, z, aux, offset = LP.edge_inputs(name)
    ref = LP.edge_fit(name)
    pl = MK._plan(hip, topo, locs, y)
    res = _fit(pl, family, z, aux, offset)
    got = _state(pl)
    r = _caller(topo, pl.buffer(10))
    print("%s: passes %d (dense %d), step %.2e, %d rows at r = 2^40" % (name, res["passes"], ref["info"][5], res["step"], (r[o] == 2.0 ** 40).sum()))
    TR._against(topo, counts, got, (ref["info"][0] + ref["info"][1], ref["mean"], ref["sd"]), TR.ORACLE_BARS, "T16 %s vs dense" % name)
    for k in range(5):
        e = abs(res["info"][k] - ref["info"][k]) / abs(ref["info"][k])
        print("info[%d]: %.10f vs %.10f, rel %.2e" % (k, res["info"][k], ref["info"][k], e))
        assert e <= TR.ORACLE_BARS[0], "info[%d] rel err %.3e" % (k, e)
    assert abs(res["lik"] - ref["lik"]) <= TR.ORACLE_BARS[0] * abs(ref["lik"])
    assert res["info"][7] == 1.0 and res["converged"] is True
    assert res["passes"] == int(ref["info"][5])
    if name == "saturated":
        assert r[o].max() > 1e3 and np.abs(got[1][o]).max() > 5.0
    else:
        assert (r[o] == 2.0 ** 40).sum() >= 100                       # otherwise this does not test the floor
        assert np.array_equal(r[o] == 2.0 ** 40, ref["r"][o] == 2.0 ** 40)
    if name == "gauss_floor":
        fresh = hip.HipPlan(topo, 0)
        s = MK._spec()
        fresh.set_locs(locs); fresh.set_obs((z - offset).reshape(-1, 1), np.minimum(aux, 2.0 ** 40)); fresh.set_kernel(s.kind, s.l, s.sig, s.scale)
        want = TR._predict(fresh)
        assert (res["d"], res["u"]) == fresh.likelihood()
        _same(got, want, "gauss_floor vs set_obs(z - offset, min(aux, 2^40))")
        fresh.close()
    pl.close()


# ---- 12. an iterate that leaves the doubles --------------------------------------------------------------------------------------------------
NOT_SPD = -3


def test_non_finite_iterate_is_refused_never_converged(hip):
    """Poisson counts in the thousands from x0 = 0: pass 1 overshoots to max |x^| = 5139, pass 2 linearises at e^eta = inf, which
    gives t = NaN and r = 1 / inf = 0.  The dense twin ends there, not converged (tests/test_laplace_cpu.py).  The device pass does
    not get as far as a mean: r = 0 at a row that is an upper node's knot leaves that leaf no positive pivot, and the pass is
    refused MRA_ERR_NOT_SPD with the r of that pass in the plan: the call never returns converged with
    a mean that is not finite."""
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    family, z, aux, offset = LP.edge_inputs("big_counts")
    twin = LP.edge_fit("big_counts", True, 10)
    assert twin["info"][5] == 2 and twin["info"][7] == 0.0 and np.isnan(twin["info"][6])
    knot = np.zeros(int(o.sum()), dtype=bool)
    knot[list(LP.t16_upper_knots())] = True
    assert (np.isnan(twin["t"][o]) & (twin["r"][o] == 0.0) & knot).any()          # the rows the refusal comes from
    pl = MK._plan(hip, topo, locs, y)
    with pytest.raises(hip.MraError) as ei:
        _fit(pl, family, z, aux, offset, x0=np.zeros(topo.N), max_iter=10)
    print("big_counts from 0: %s" % ei.value)
    assert ei.value.code == NOT_SPD and "not positive definite" in str(ei.value)
    r = _caller(topo, pl.buffer(10))
    assert np.array_equal(r[o] == 0.0, twin["r"][o] == 0.0) and (r[o] == 0.0).any()          # pass 2's r, as the twin has it
    # the plan is not poisoned: the data-based start on the same data converges as the twin does
    ref = LP.edge_fit("big_counts")
    res = _fit(pl, family, z, aux, offset)
    assert res["converged"] and res["passes"] == int(ref["info"][5]) == 4
    TR._against(topo, counts, _state(pl), (ref["info"][0] + ref["info"][1], ref["mean"], ref["sd"]), TR.ORACLE_BARS, "T16 big_counts vs dense")
    assert abs(res["lik"] - ref["lik"]) <= TR.ORACLE_BARS[0] * abs(ref["lik"])
    pl.close()


def test_mratree_keeps_no_mode_of_a_fit_that_left_the_doubles(hip):
    import pymra_amd
    import pymra_amd.MRATools as mt
    n, r0, M = RC.TREES["T16"]
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    family, z, aux, offset = LP.edge_inputs("big_counts")
    s = MK._spec()
    cov = lambda a, b: mt.Matern32(a, b, l=s.l, sig=s.sig)           # noqa: E731
    np.random.seed(7)                                                 # as MK._tree does: the same knots
    mt.genLocations2d(Nx=n, Ny=n)
    tree = pymra_amd.MRATree(locs, r0, cov, z.reshape(-1, 1), MK.R, M=M, J=4)
    assert np.array_equal(tree.topology.knot_rows, topo.knot_rows)
    lik = tree.fitLaplace("poisson")
    mode = tree._laplace_mean.copy()
    assert tree.laplace["converged"] and tree.laplace["passes"] == 4
    with pytest.raises(pymra_amd.plan.MraError) as ei:
        tree.fitLaplace("poisson", x0=np.zeros(topo.N), max_iter=10)
    assert ei.value.code == NOT_SPD
    assert np.array_equal(tree._laplace_mean, mode)                   # the mode of the last converged fit, not of the refused one
    warm = tree.fitLaplace("poisson")                                 # started from that mode
    assert tree.laplace["converged"] and tree.laplace["passes"] <= 4 and np.all(np.isfinite(tree._laplace_mean))
    assert abs(warm - lik) <= TR.ROUTE_BARS[0] * abs(lik)
