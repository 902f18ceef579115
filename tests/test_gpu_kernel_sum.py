"""MRA_KERNEL_SUM on the GPU: a nested covariance model, the sum of up to four closed-form kernels, evaluated on the device (mode 5).

A. The function: mra_eval_kernel(kind 7) on the 40 001 distances of test_device_kernels_match_numpy_to_ulps plus 0, 1e150 and 1e300.
   A sum of ONE component is the single kind bit for bit (adding to 0 is exact).  The four-component sum against the host sum of the
   four single-kind device evaluations at 4 * 2^-52 * amp absolute: the components are the same bits, the device adds them in the
   same order, and a contracted multiply-add skips a rounding of at most 2^-53 amp_c in each of the three additions that have a
   non-zero partner - derived, not measured.  Exactly amp at D = 0 (also with an Iden component), exactly 0 at 1e150 and 1e300.
B. Passes of 0.7 Matern32(l) + 0.3 Exp(l / 5) + 0.1 Iden against run_levelwise at the project's bars (likelihood
   1e-10 relative, mean 1e-9, sd 1e-8 relative) on the smallest trees of the route tables, 40 % observed and the first leaf empty;
   the route from mra_get_route: the level-by-level prior.  One pass with a Gaussian component in place of the Exp.
C. One tree, three inputs: mode 5, the MRA_KERNEL_HOST plan fed by the same KernelSum.evaluate, and the oracle, pairwise.  A K = 1
   sum against the single-kind plan on the same level-by-level route, bit for bit.
D. Phantom knot columns with a Matern52 component: finite.
E. The calls on the retained factors on a 2-D tree and on the sphere, against the CPU twins at the bounds of their own test files.
F. reevaluate: changed ranges and sills equal a fresh tree bit for bit, back again reproduces the first bits, and a plain Matern32
   returns the plan to the fused route and to that tree's bits.
G. One sharded cell (world 2) against the sharded oracle."""
import functools

import numpy as np
import pytest

import _cases as K
import _line_cells as LC
import _route_cells as RC
import test_gpu_likelihood_masks as MK

pytestmark = pytest.mark.gpu

ORACLE_BARS = (1e-10, 1e-9, 1e-8)
R2 = MK.R
MRA_OPT_FUSED = 2


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _model(l, circular=False, second="exp"):
    """0.7 Matern32(l) + 0.3 Exp(l / 5) + 0.1 Iden (second = "gauss": a Gaussian in place of the Exp)"""
    import pymra_amd.MRATools as mt
    a, b = mt.SymbolicLocs("a", 1), mt.SymbolicLocs("b", 1)
    mid = mt.ExpCovFun(a, b, l=l / 5, circular=circular) if second == "exp" else mt.GaussianCovFun(a, b, l=l / 5, circular=circular)
    return 0.7 * mt.Matern32(a, b, l=l, circular=circular) + 0.3 * mid + 0.1 * mt.Iden(a, b, circular=circular)


def _cov(l, second="exp", s1=0.7, s2=0.3, s3=0.1, ratio=5.0):
    import pymra_amd.MRATools as mt
    mid = mt.ExpCovFun if second == "exp" else mt.GaussianCovFun
    return lambda a, b: s1 * mt.Matern32(a, b, l=l) + s2 * mid(a, b, l=l / ratio) + s3 * mt.Iden(a, b)


def _plan(hip, topo, locs, y, R, spec, opts=()):
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, R)
    pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale, spec.circular, spec.nu)
    for o, v in opts:
        pl.set_option(o, v)
    return pl


def _predict(pl):
    pl.run(True, True)
    mean, _, sd = pl.predict(with_sd=True)
    return sum(pl.likelihood()), mean.copy(), sd.copy()


def _errors(got, ref):
    ok = ref[2] > 0                       # rows outside every leaf report 0
    return (abs(got[0] - ref[0]) / abs(ref[0]), float(np.max(np.abs(got[1] - ref[1]))),
            float(np.max(np.abs(got[2][ok] - ref[2][ok]) / ref[2][ok])) if ok.any() else 0.0)


def _check(got, ref, bars, tag):
    e = _errors(got, ref)
    print("%s: lik %.2e mean %.2e sd %.2e" % (tag, *e))
    assert np.isfinite(got[0]) and np.all(np.isfinite(got[1])) and np.all(np.isfinite(got[2])), tag
    assert e[0] <= bars[0], "%s: likelihood rel err %.3e" % (tag, e[0])
    assert e[1] <= bars[1], "%s: mean abs err %.3e" % (tag, e[1])
    assert e[2] <= bars[2], "%s: sd rel err %.3e" % (tag, e[2])


def _ref3(ref):
    return ref["lik"], np.asarray(ref["mean"]).ravel(), np.asarray(ref["sd"]).ravel()


# ---- A. the function -----------------------------------------------------------------------------------------------------------------
SINGLE = ((0, 0.3, 1.0), (1, 0.3, 1.7), (2, 2.0, 0.4), (3, 0.8, 1.2), (4, 1.0, 1.0))       # (kind, l, sig): the parity test's, and Iden
SCALE = 1.5


@pytest.fixture(scope="module")
def distances():
    rng = np.random.RandomState(1)
    D = np.concatenate([[0.0], np.abs(rng.normal(size=20000)) * 0.7, 10.0 ** rng.uniform(-9, 2, size=20000)])
    assert len(D) == 40001
    return np.concatenate([D, [0.0, 1e150, 1e300]])


@pytest.mark.parametrize("kind,l,sig", SINGLE)
def test_a_sum_of_one_component_is_the_single_kind_bit_for_bit(hip, distances, kind, l, sig):
    got = hip.eval_kernel(7, scale=SCALE, D=distances, components=[(kind, l, sig)])
    want = hip.eval_kernel(kind, l, sig, SCALE, distances)
    amp = SCALE * sig
    print("kind %d: the single kind at 1e150 and 1e300: %r %r, the sum: %r %r" % (kind, want[-2], want[-1], got[-2], got[-1]))
    # (1e300 squared is inf: the single kinds' own value there is whatever inf gives them - the sum gives 0 - so the last entry is
    # compared only where the single kind has a number)
    n = len(distances) - (1 if np.isnan(want[-1]) else 0)
    assert np.array_equal(got[:n], want[:n])
    assert got[0] == amp and got[-3] == amp and got[-2] == 0.0 and got[-1] == 0.0
    assert np.all(np.isfinite(got))


def test_the_four_component_sum_against_the_sum_of_its_parts(hip, distances):
    comps = [(1, 0.3, 1.7), (2, 2.0, 0.4), (3, 0.8, 1.2), (0, 0.05, 1.0)]
    amp = ((SCALE * 1.7 + SCALE * 0.4) + SCALE * 1.2) + SCALE * 1.0
    got = hip.eval_kernel(7, scale=SCALE, D=distances, components=comps)
    parts = [hip.eval_kernel(k, l, s, SCALE, distances[:-1]) for k, l, s in comps]
    want = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    err = np.abs(got[:-1] - want)
    print("4 components: max |device sum - host sum of the parts| / amp %.3e (bar %.3e), %d of %d equal"
          % (err.max() / amp, 4 * 2.0 ** -52, int(np.sum(err == 0)), len(err)))
    assert np.all(np.isfinite(got))
    assert err.max() <= 4 * 2.0 ** -52 * amp
    assert got[0] == amp and got[-3] == amp and got[-2] == 0.0 and got[-1] == 0.0
    # with an Iden component: amp at D = 0, and the Iden is gone everywhere else
    withi = hip.eval_kernel(7, scale=SCALE, D=distances, components=comps[:3] + [(4, 1.0, 0.25)])
    ampi = ((SCALE * 1.7 + SCALE * 0.4) + SCALE * 1.2) + SCALE * 0.25
    three = hip.eval_kernel(7, scale=SCALE, D=distances, components=comps[:3])
    assert withi[0] == ampi and withi[-3] == ampi and withi[-2] == 0.0 and withi[-1] == 0.0
    nz = distances != 0.0
    assert np.array_equal(withi[nz], three[nz])


def test_eval_kernel_refuses_what_set_kernel_refuses(hip):
    for comps in ([(5, 0.3, 1.0)], [(6, 0.3, 1.0)], [(1, 0.0, 1.0)], [(1, 0.3, -1.0)], [(1, 0.3, 1.0)] * 5):
        with pytest.raises(hip.MraError) as e:
            hip.eval_kernel(7, D=np.zeros(3), components=comps)
        assert e.value.code == -1


# ---- B. passes -----------------------------------------------------------------------------------------------------------------------
def _mask(topo, seed=0):
    """40 % observed, the first leaf without any observation"""
    obs = np.random.RandomState(seed).uniform(size=topo.N) < 0.4
    MK._empty(obs, topo, [int(np.nonzero(topo.node_leaf)[0][0])])
    return obs


@functools.lru_cache(maxsize=None)
def _grid_problem(key):
    topo, locs = MK._tree(*RC.TREES[key])
    return topo, locs, MK._y(_mask(topo)), R2


@functools.lru_cache(maxsize=None)
def _problem(cell):
    """(topo, coordinates, y, R, l, circular) - the cells and the l of tests/test_gpu_matern_nu.py"""
    if cell in RC.TREES:
        return _grid_problem(cell) + (0.25, False)
    if cell.startswith("L16"):
        topo, locs, obs, y, counts = LC.problem("L16")
        assert counts[0] == 0
        return topo, locs, y.reshape(-1, 1), LC.R, 0.02, cell.endswith("circular")
    import test_gpu_sphere as SP
    ll, xyz, topo, y = SP.tree(64, 16, 2)
    assert len(xyz) <= 4096 and topo.coord_dim == 3
    return topo, xyz, y, SP.R, 0.5, False


@functools.lru_cache(maxsize=None)
def _oracle(cell, second="exp"):
    from oracle.mra_levelwise import run_levelwise
    topo, X, y, R, l, circ = _problem(cell)
    return _ref3(run_levelwise(topo, X, _model(l, circ, second), y, R))


CELLS = [("T16", ()), ("T16", ((MRA_OPT_FUSED, 0),)), ("A32", ()), ("C64", ()), ("L16", ()), ("L16circular", ()), ("sphere", ())]


@pytest.mark.parametrize("cell,opts", CELLS, ids=["%s%s" % (c, "-fused0" if o else "") for c, o in CELLS])
def test_passes_against_the_oracle(hip, cell, opts):
    topo, X, y, R, l, circ = _problem(cell)
    spec = _model(l, circ)
    pl = _plan(hip, topo, X, y, R, spec, opts)
    assert pl.sum_table().shape == (3, 6) and pl.sum_sill() == (0.7 + 0.3) + 0.1
    got = _predict(pl)
    rt = pl.route()
    assert rt["path"] == "Levels", rt                                 # no fused instance of mode 5: the prior goes level by level
    assert rt["prior_level"], rt                                     # ... through the one-launch prior levels (k_leaf_gemm<COV, SOLVE>)
    _check(got, _oracle(cell), ORACLE_BARS, "%s %s" % (cell, opts))
    pl.run(True, False)                                              # the likelihood-only pass (gathered rows)
    lik = sum(pl.likelihood())
    ref = _oracle(cell)[0]
    assert abs(lik - ref) <= ORACLE_BARS[0] * abs(ref), (lik, ref)
    assert pl.route()["path"] == "Levels"
    pl.close()


def test_a_gaussian_component_in_place_of_the_exp(hip):
    topo, X, y, R, l, circ = _problem("T16")
    pl = _plan(hip, topo, X, y, R, _model(l, circ, "gauss"))
    assert pl.sum_table()[1, 0] == 1.0
    _check(_predict(pl), _oracle("T16", "gauss"), ORACLE_BARS, "T16 gauss")
    assert abs(_oracle("T16", "gauss")[0] - _oracle("T16")[0]) > 1e-3 * abs(_oracle("T16")[0])
    pl.close()


# ---- C. one pass, three inputs ---------------------------------------------------------------------------------------------------------
def test_mode_5_the_host_route_and_the_oracle_agree(hip):
    topo, X, y, R, l, _ = _problem("T16")
    spec = _model(l)
    dev = _plan(hip, topo, X, y, R, spec)
    a = _predict(dev)
    host = hip.HipPlan(topo, 0)
    host.set_locs(X); host.set_obs(y, R)
    host.upload_host_cov(lambda p, q: spec.evaluate(p, q), X, y)
    b = _predict(host)
    o = _oracle("T16")
    _check(a, o, ORACLE_BARS, "mode 5 vs oracle")
    _check(b, o, ORACLE_BARS, "host blocks vs oracle")
    _check(a, b, ORACLE_BARS, "mode 5 vs host blocks")
    # and it is not one of its components alone: Matern32 at the same l with the whole sill is far away
    import pymra_amd.MRATools as mt
    dev.set_kernel(mt.KIND_MATERN32, l, 1.1, 1.0)
    dev.run(True, False)
    assert abs(sum(dev.likelihood()) - a[0]) > 1e-3 * abs(a[0])
    dev.close(); host.close()


@pytest.mark.parametrize("kind,l,sig", [(0, 0.25, 1.0), (1, 0.25, 1.2), (2, 0.25, 1.2), (3, 0.05, 1.2), (4, 1.0, 1.0)])
def test_a_sum_of_one_component_is_the_single_kind_plan_bit_for_bit(hip, kind, l, sig):
    """... on the route both can take: the single kind with MRA_OPT_FUSED = 0."""
    import pymra_amd.MRATools as mt
    topo, X, y, R, _, _ = _problem("T16")
    one = _plan(hip, topo, X, y, R, mt.KernelSpec(kind, l, sig, 0.8), ((MRA_OPT_FUSED, 0),))
    a = _predict(one)
    assert one.route()["path"] == "Levels"
    sm = hip.HipPlan(topo, 0)
    sm.set_locs(X); sm.set_obs(y, R)
    sm.set_kernel(7, components=[(kind, l, sig)], scale=0.8)
    b = _predict(sm)
    assert sm.route()["path"] == "Levels"
    e = _errors(b, a)
    print("kind %d: K = 1 sum against the single kind: lik %r %r, errors lik %.2e mean %.2e sd %.2e" % (kind, a[0], b[0], *e))
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    one.close(); sm.close()


# ---- D. phantom knots ------------------------------------------------------------------------------------------------------------------
def test_phantom_knot_columns_stay_finite(hip):
    """r0 = 20: blocks of 32 columns holding 20 knots - twelve phantom columns at MRA_FAR_AWAY in every knot block, where a Matern52
    component's a2 t^2 is 1e300 and more while its exponential is 0."""
    import pymra_amd.MRATools as mt
    import test_gpu_cov as GC
    from oracle.mra_levelwise import run_levelwise
    topo, locs, y_obs, _, R = GC._shape_tree("grid48_r20")
    assert int(topo.cw[0]) == 32 and int(topo.knot_ptr[1] - topo.knot_ptr[0]) == 20
    a, b = mt.SymbolicLocs("a", 2), mt.SymbolicLocs("b", 2)
    for l52 in (0.25, 1e-4):               # (1e-4: t^2 overflows without the clamp in front of the polynomial)
        spec = 0.6 * mt.Matern52(a, b, l=l52) + 0.3 * mt.ExpCovFun(a, b, l=0.05) + 0.1 * mt.GaussianCovFun(a, b, l=0.1)
        pl = _plan(hip, topo, locs, y_obs, R, spec)
        got = _predict(pl)
        _check(got, _ref3(run_levelwise(topo, locs, spec, y_obs, R)), ORACLE_BARS, "grid48_r20 l52=%g" % l52)
        pl.close()


# ---- E. the calls on the retained factors ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(hip):
    """MRATree on T16's grid with the model of B and its CPU state"""
    import pymra_amd.MRATools as mt
    from pymra_amd import MRATree
    import _treesites as TS
    topo0, locs, y, R, l, _ = _problem("T16")
    np.random.seed(7)
    tree = MRATree(locs, 16, _cov(l), y, R, M=2, J=4, verbose=False)
    assert isinstance(tree.kernel, mt.KernelSum) and tree.kernel.l == _model(l).l and tree.plan.route()["path"] == "Levels"
    state = TS.SiteState(tree.topology, locs, tree.kernel, y, R)
    yield tree, locs, y, R, state
    tree.plan.close()


def _padded_rows(t, rows, n):
    padded = np.full(n, -1, dtype=np.int64)                                       # prior_sigma_rows takes padded rows
    padded[t.perm[t.perm >= 0]] = np.nonzero(t.perm >= 0)[0]
    assert np.all(padded[rows] >= 0)
    return padded[rows]


def test_solve_predict_at_and_covariance_at(fitted):
    from oracle.mra_faithful import prior_sigma_rows
    tree, locs, y, R, state = fitted
    mean, sd = tree.predict()
    mean, sd = np.asarray(mean).ravel(), np.asarray(sd).ravel()
    scale = max(1.0, np.abs(mean).max())
    m1, quad = tree.solve(np.nan_to_num(y))
    print("solve vs predict: %.2e" % np.abs(m1[:, 0] - mean).max())
    assert np.abs(m1[:, 0] - mean).max() <= 1e-8 * scale                          # tests/test_gpu_solve.py
    rows = np.random.RandomState(3).choice(len(locs), 40, replace=False)
    pm, ps = tree.predictAt(locs[rows])
    print("predictAt vs predict: mean %.2e sd %.2e" % (np.abs(pm[:, 0] - mean[rows]).max(), np.abs(ps - sd[rows]).max()))
    assert np.abs(pm[:, 0] - mean[rows]).max() <= 1e-9 * scale                    # POST_NO_TRUTH_TOL, tests/test_gpu_sites.py
    assert np.abs(ps ** 2 - sd[rows] ** 2).max() <= 1e-9 * 1.1
    t = tree.topology
    S = prior_sigma_rows(t, locs, tree.kernel.evaluate, _padded_rows(t, rows, len(locs)))
    for distr, tol in (("prior", 1e-10), ("posterior", 1e-9)):                    # PRIOR_TOL / POST_NO_TRUTH_TOL, tests/test_gpu_cov.py
        cols = tree.covariance(rows, distr)
        at = tree.covarianceAt(locs[rows], distr)
        e = np.abs(at - cols[rows]).max()
        print("covarianceAt vs covariance(rows) %s: %.2e" % (distr, e))
        assert e <= tol * 1.1
        if distr == "prior":
            e = np.abs(cols[rows] - S).max()
            print("covariance(rows, prior) vs prior_sigma_rows: %.2e" % e)
            assert e <= 1e-10 * 1.1
        else:
            assert np.abs(np.diag(at) - sd[rows] ** 2).max() <= 1e-9 * 1.1


def test_sample_at_against_the_twin(fitted):
    import _treesitecov as TC
    import test_gpu_sitedraw as SD
    tree, locs, y, R, state = fitted
    rng = np.random.RandomState(5)
    sites = np.vstack([locs[rng.choice(len(locs), 12, replace=False)], rng.uniform(0.02, 0.98, size=(12, 2))])
    leaf = tree.locate(sites)
    for post, tol in ((False, 1e-10), (True, 1e-9)):                               # tests/test_gpu_sitedraw.py
        F = SD._device_F(tree.plan, sites, leaf, post)
        SD._check_FFt(F, TC.tree_sites_cov(state, sites, leaf, post), 1.1, tol, "sum %s" % ("posterior" if post else "prior"))
    z = rng.standard_normal((tree.plan.sample_sites_slots(len(sites)), 3))
    x = tree.sampleAt(sites, 3, "prior", leaf=leaf, z=z)
    F = SD._device_F(tree.plan, sites, leaf, False)
    assert np.abs(x - F @ z).max() <= 1e-12 * 1.1 * np.abs(z).sum(axis=0).max()


def test_cross_validation_against_the_twin(fitted):
    import _treecv as CV
    import test_gpu_cv as GV
    tree, locs, y, R, state = fitted
    ymax = np.nanmax(np.abs(y))
    for leaf in (False, True):
        want = CV.tree_cv(state, leaf)
        got = tree.plan.cv(leaf=leaf)
        e = GV._errors(got, want, ymax)
        print("cv %s: mean %.2e var %.2e lpd %.2e group %.2e info %.2e (max h %.4f)" % ("leaf" if leaf else "loo", *e, got[4][5]))
        assert max(e) <= GV._tol() * max(1.0, (0.02 / (1.0 - got[4][5])) ** 2)
    for kind in ("loo", "leaf"):
        res = tree.crossValidate(kind)
        assert res.n > 0 and np.isfinite(res.score)


def _trend_fit(hip, topo, X, y, R, spec):
    import _treetrend as TT
    import test_gpu_trend as GT
    Xd = GT._design(topo.N, 3)
    yt = GT._with_trend(y, Xd)
    GT._check_fit(hip, topo, X, spec, yt, R, Xd, TT.tree_trend(topo, X, spec, yt, R, Xd))


def test_a_trend_fit_against_the_twin(hip, fitted):
    tree, locs, y, R, state = fitted
    _trend_fit(hip, tree.topology, locs, y, R, tree.kernel)
    # and through the tree: setTrend refits on the kept plan, the likelihood is the profile value
    import test_gpu_trend as GT
    Xd = GT._design(len(locs), 3)
    lik0 = float(tree.getLikelihood()[0, 0])
    lik = float(tree.setTrend(Xd)[0, 0])
    assert np.isfinite(lik) and tree.trend.beta.shape == (3,) and lik != lik0
    assert float(tree.setTrend(None)[0, 0]) == lik0


def test_the_sphere_calls_on_the_retained_factors(hip):
    """coord_dim = 3: the DIM = 3 instances of mra_launch_sum2.hip - solve, predictAt, covarianceAt, covariance against prior_sigma_rows,
    sampleAt, both cross-validations against the CPU twin and a trend fit, at the bounds of tests/test_gpu_solve.py,
    tests/test_gpu_sites.py, tests/test_gpu_cov.py, tests/test_gpu_cv.py (its sphere case) and tests/test_gpu_trend.py."""
    import pymra_amd
    import pymra_amd.MRATools as mt
    import test_gpu_cv as GV
    import test_gpu_sphere as SP
    from oracle.mra_faithful import prior_sigma_rows
    ll, xyz, topo, y = SP.tree(64, 16, 2)
    np.random.seed(7)
    tree = pymra_amd.MRATree(ll, 16, _cov(0.5), y.reshape(-1, 1), SP.R, M=2, J=4, metric="chordal", verbose=False)
    assert tree.kernel.kind == mt.KIND_SUM and np.array_equal(tree.topology.perm, topo.perm) and tree.plan.route()["path"] == "Levels"
    mean, sd = (np.asarray(v).ravel() for v in tree.predict())
    scale = max(1.0, np.abs(mean).max())
    m1, _ = tree.solve(np.nan_to_num(y))
    print("sphere solve vs predict: %.2e" % np.abs(m1[:, 0] - mean).max())
    assert np.abs(m1[:, 0] - mean).max() <= 1e-8 * scale
    rows = np.random.RandomState(3).choice(len(ll), 40, replace=False)
    pm, ps = tree.predictAt(ll[rows])
    print("sphere predictAt vs predict: mean %.2e var %.2e" % (np.abs(pm[:, 0] - mean[rows]).max(), np.abs(ps ** 2 - sd[rows] ** 2).max()))
    assert np.abs(pm[:, 0] - mean[rows]).max() <= 1e-9 * scale and np.abs(ps ** 2 - sd[rows] ** 2).max() <= 1e-9 * 1.1
    S = prior_sigma_rows(tree.topology, xyz, tree.kernel.evaluate, _padded_rows(tree.topology, rows, len(ll)))
    for distr, tol in (("prior", 1e-10), ("posterior", 1e-9)):
        cols = tree.covariance(rows, distr)
        e = np.abs(tree.covarianceAt(ll[rows], distr) - cols[rows]).max()
        print("sphere covarianceAt vs covariance(rows) %s: %.2e" % (distr, e))
        assert e <= tol * 1.1
        if distr == "prior":
            e = np.abs(cols[rows] - S).max()
            print("sphere covariance(rows, prior) vs prior_sigma_rows: %.2e" % e)
            assert e <= 1e-10 * 1.1
    x = tree.sampleAt(ll[rows], 2, "posterior", z=np.zeros((tree.plan.sample_sites_slots(len(rows)), 2)))
    assert np.abs(x - pm[:, :1]).max() <= 1e-12 * scale                       # z = 0: the mean (tests/test_gpu_sitedraw.py)
    GV._against_twin(tree.plan, tree.topology, xyz, tree.kernel, y, SP.R, "sphere sum", GV._tol())
    _trend_fit(hip, tree.topology, xyz, np.asarray(y, float).ravel(), SP.R, tree.kernel)
    tree.plan.close()


# ---- F. other ranges and sills on a kept tree --------------------------------------------------------------------------------------------
def test_reevaluate_equals_a_fresh_tree_and_returns_to_the_fused_route(hip):
    import pymra_amd.MRATools as mt
    from pymra_amd import MRATree
    topo0, locs, y, R, l, _ = _problem("T16")

    def fresh(cov):
        np.random.seed(7)
        return MRATree(locs, 16, cov, y, R, M=2, J=4, verbose=False)
    first, second = _cov(l), _cov(0.4, s1=0.5, s2=0.45, s3=0.05, ratio=8.0)
    tree = fresh(first)
    lik1 = float(tree.getLikelihood()[0, 0])
    m1, s1 = (np.array(v).copy() for v in tree.predict())
    tab1 = tree.plan.sum_table().copy()
    lik2 = float(tree.reevaluate(second, want_predict=True)[0, 0])
    m2, s2 = (np.array(v).copy() for v in tree.predict())
    assert not np.array_equal(tree.plan.sum_table(), tab1) and tree.plan.route()["path"] == "Levels"
    other = fresh(second)
    assert lik2 == float(other.getLikelihood()[0, 0]) and lik2 != lik1
    om, os_ = other.predict()
    assert np.array_equal(m2, np.array(om)) and np.array_equal(s2, np.array(os_))
    # fewer components on the same plan: nothing of the third record is left behind
    two = lambda a, b: 0.5 * mt.Matern32(a, b, l=0.4) + 0.45 * mt.ExpCovFun(a, b, l=0.05)
    lik3 = float(tree.reevaluate(two)[0, 0])
    f3 = fresh(two)
    assert tree.plan.sum_table().shape == (2, 6) and lik3 == float(f3.getLikelihood()[0, 0])
    # back to the first model: the first bits
    assert float(tree.reevaluate(first, want_predict=True)[0, 0]) == lik1
    mb, sb = tree.predict()
    assert np.array_equal(np.array(mb), m1) and np.array_equal(np.array(sb), s1) and np.array_equal(tree.plan.sum_table(), tab1)
    # a plain Matern32: the fused route again, and that tree's bits
    plain = lambda a, b: mt.Matern32(a, b, l=l, sig=1.1)
    lik4 = float(tree.reevaluate(plain, want_predict=True)[0, 0])
    f4 = fresh(plain)
    assert tree.kernel.kind == mt.KIND_MATERN32 and tree.plan.sum_table().shape == (0, 6)
    assert tree.plan.route()["path"] == f4.plan.route()["path"] == "Fused"
    assert lik4 == float(f4.getLikelihood()[0, 0])
    m4, s4 = tree.predict()
    fm, fs = f4.predict()
    assert np.array_equal(np.array(m4), np.array(fm)) and np.array_equal(np.array(s4), np.array(fs))
    # and the sum once more
    assert float(tree.reevaluate(first)[0, 0]) == lik1 and tree.plan.route()["path"] == "Levels"
    for t in (tree, other, f3, f4):
        t.plan.close()


# ---- G. one sharded cell -----------------------------------------------------------------------------------------------------------------
def test_a_sharded_pass_against_the_sharded_oracle(hip):
    topo, X, y, R, l, _ = _problem("T16")
    spec = _model(l)
    liks, mean, var, lvl = K.emulate_world_on_one_gpu(hip, topo, X, y, R, spec, 2)
    rl, rm, rv, rlvl = K.emulate_world_oracle(topo, X, y, R, spec, 2)
    assert lvl == rlvl
    for a, b in zip(liks, rl):
        assert abs(a - b) <= ORACLE_BARS[0] * abs(b), (a, b)
    ok = rv > 0
    e_m, e_s = np.abs(mean - rm).max(), (np.abs(np.sqrt(var[ok]) - np.sqrt(rv[ok])) / np.sqrt(rv[ok])).max()
    print("world 2: lik %.2e mean %.2e sd %.2e" % (max(abs(a - b) / abs(b) for a, b in zip(liks, rl)), e_m, e_s))
    assert e_m <= ORACLE_BARS[1] and e_s <= ORACLE_BARS[2]
