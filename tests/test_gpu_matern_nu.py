"""MRA_KERNEL_MATERN on the GPU: the Matern covariance of any smoothness nu, evaluated on the device by quadrature (mode 4).

A. The function: mra_eval_kernel(kind 6) against the 40-digit golden (tests/golden/matern_nu.npz) for all ten nu at 1e-13 * amp
   absolute - ten times the 1.1e-14 of the method in float64 (tests/test_matern_nu_cpu.py), which leaves room for the roundings
   of the device's exponential and of t^nu; exactly amp at D = 0; exactly 0 (not NaN) at a phantom knot's distance and at t = 745;
   within the bar below the quadrature's clamp (t = 2^-41, 2^-60); nu = 1.5 and 2.5 through mode 4 against kinds 1 and 2.
B. Passes at nu = 0.8 (not a half-integer) and nu = 2 (where a Bessel series is singular) against run_levelwise with the scipy
   evaluation, at the project's bars (likelihood 1e-10 relative, mean 1e-9, sd 1e-8 relative), on the smallest
   trees of the route tables, 40 % observed and one leaf empty; the route from mra_get_route: the level-by-level prior.
   One 64 x 64 tree on the sphere (coord_dim = 3), with the calls on the retained factors: those instances live in a unit of their own.
C. One tree, one pass, three inputs: mode 4, the MRA_KERNEL_HOST plan fed by the scipy callable, and the oracle, pairwise - a
   dispatch chain that fell through to another family's kernel is off in the first digit.
D. Phantom knots (a node with fewer knots than its block is wide): finite likelihood and predictions.
E. The calls on the retained factors, which have instances of their own, at the bounds their own test files use for Matern32.
F. reevaluate with another nu equals a fresh tree bit for bit, and back again reproduces the first likelihood bit for bit."""
import functools
import os

import numpy as np
import pytest

import _cases as K
import _line_cells as LC
import _route_cells as RC
import test_gpu_likelihood_masks as MK

pytestmark = pytest.mark.gpu

ORACLE_BARS = (1e-10, 1e-9, 1e-8)
NUS = (0.8, 2.0)
R2 = MK.R


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _spec(nu, l=0.25, sig=1.2, circular=False):
    import pymra_amd.MRATools as mt
    return mt.KernelSpec(mt.KIND_MATERN, l, sig, 1.0, circular, nu=nu)


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
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(K.ROOT, "tests", "golden", "matern_nu.npz"))


@pytest.mark.parametrize("k", range(10))
def test_the_function_on_the_device(hip, golden, k):
    nu = float(golden["nu"][k])
    sig, scale = 1.5, 2.0
    amp = sig * scale
    l = float(np.sqrt(2.0 * nu))                    # sqrt(2 nu) / l is exactly 1 on the host: D is t
    t = np.concatenate((golden["t"], golden["t_edge"]))
    want = amp * np.concatenate((golden["M"][k], golden["M_edge"][k]))
    got = hip.eval_kernel(6, l, sig, scale, t, nu=nu)
    err = np.abs(got - want)
    print("nu %.2f: max |device - golden| / amp %.3e at t = %.6g" % (nu, err.max() / amp, t[np.argmax(err)]))
    assert np.all(np.isfinite(got))
    assert err.max() <= 1e-13 * amp
    assert got[0] == amp                             # D = 0
    edge = hip.eval_kernel(6, l, sig, scale, np.array([0.0, 1e150, 745.0, 2.0 ** -41, 1e300, 746.0]), nu=nu)
    assert edge[0] == amp and edge[1] == 0.0 and edge[2] == 0.0 and edge[4] == 0.0 and edge[5] == 0.0, edge
    assert np.isfinite(edge[3]) and abs(edge[3] - amp * golden["M_edge"][k][1]) <= 1e-13 * amp


@pytest.mark.parametrize("nu,kind", [(1.5, 1), (2.5, 2)])
def test_mode_4_against_the_closed_forms(hip, golden, nu, kind):
    sig, scale, l = 1.5, 2.0, 0.37
    D = np.concatenate((golden["t"], [1e150])) * l / np.sqrt(2.0 * nu)
    a, b = hip.eval_kernel(6, l, sig, scale, D, nu=nu), hip.eval_kernel(kind, l, sig, scale, D)
    print("nu %.1f through mode 4 against kind %d: %.3e" % (nu, kind, np.abs(a - b).max() / (sig * scale)))
    assert np.abs(a - b).max() <= 1e-13 * sig * scale


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
    """(topo, coordinates, y, R, l, circular)"""
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
def _oracle(cell, nu):
    from oracle.mra_levelwise import run_levelwise
    topo, X, y, R, l, circ = _problem(cell)
    return _ref3(run_levelwise(topo, X, _spec(nu, l, circular=circ), y, R))


CELLS = [("T16", ()), ("T16", ((2, 0),)), ("A32", ()), ("C64", ()), ("L16", ()), ("L16circular", ()), ("sphere", ())]


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("cell,opts", CELLS, ids=["%s%s" % (c, "-fused0" if o else "") for c, o in CELLS])
def test_passes_against_the_oracle(hip, cell, opts, nu):
    topo, X, y, R, l, circ = _problem(cell)
    pl = _plan(hip, topo, X, y, R, _spec(nu, l, circular=circ), opts)
    got = _predict(pl)
    rt = pl.route()
    assert rt["path"] == "Levels", rt                                 # no fused instance of mode 4: the prior goes level by level
    assert rt["prior_level"], rt                                     # ... through the one-launch prior levels (k_leaf_gemm<COV, SOLVE>)
    _check(got, _oracle(cell, nu), ORACLE_BARS, "%s %s nu=%g" % (cell, opts, nu))
    pl.run(True, False)                                              # the likelihood-only pass (gathered rows)
    lik = sum(pl.likelihood())
    ref = _oracle(cell, nu)[0]
    assert abs(lik - ref) <= ORACLE_BARS[0] * abs(ref), (lik, ref)
    assert pl.route()["path"] == "Levels"
    pl.close()


def test_the_sphere_calls_on_the_retained_factors(hip):
    """coord_dim = 3 runs kernel instances of its own (mra_launch_nu3.hip), the calls on the retained factors included: solve,
    predictAt, covarianceAt and covariance, and both cross-validations against the CPU twin, at the bounds of tests/test_gpu_solve.py,
    tests/test_gpu_sites.py, tests/test_gpu_cov.py and tests/test_gpu_cv.py (its sphere case)."""
    import pymra_amd
    import pymra_amd.MRATools as mt
    import test_gpu_cv as GV
    import test_gpu_sphere as SP
    ll, xyz, topo, y = SP.tree(64, 16, 2)
    np.random.seed(7)
    tree = pymra_amd.MRATree(ll, 16, lambda a, b: mt.Matern(a, b, l=0.5, nu=0.8), y.reshape(-1, 1), SP.R, M=2, J=4, metric="chordal", verbose=False)
    assert tree.kernel.kind == mt.KIND_MATERN and np.array_equal(tree.topology.perm, topo.perm) and tree.plan.route()["path"] == "Levels"
    mean, sd = (np.asarray(v).ravel() for v in tree.predict())
    scale = max(1.0, np.abs(mean).max())
    m1, _ = tree.solve(np.nan_to_num(y))
    print("sphere solve vs predict: %.2e" % np.abs(m1[:, 0] - mean).max())
    assert np.abs(m1[:, 0] - mean).max() <= 1e-8 * scale
    rows = np.random.RandomState(3).choice(len(ll), 40, replace=False)
    pm, ps = tree.predictAt(ll[rows])
    print("sphere predictAt vs predict: mean %.2e var %.2e" % (np.abs(pm[:, 0] - mean[rows]).max(), np.abs(ps ** 2 - sd[rows] ** 2).max()))
    assert np.abs(pm[:, 0] - mean[rows]).max() <= 1e-9 * scale and np.abs(ps ** 2 - sd[rows] ** 2).max() <= 1e-9
    for distr, tol in (("prior", 1e-10), ("posterior", 1e-9)):
        e = np.abs(tree.covarianceAt(ll[rows], distr) - tree.covariance(rows, distr)[rows]).max()
        print("sphere covarianceAt vs covariance(rows) %s: %.2e" % (distr, e))
        assert e <= tol
    x = tree.sampleAt(ll[rows], 2, "posterior", z=np.zeros((tree.plan.sample_sites_slots(len(rows)), 2)))
    assert np.abs(x - pm[:, :1]).max() <= 1e-12 * scale                       # z = 0: the mean (tests/test_gpu_sitedraw.py)
    GV._against_twin(tree.plan, tree.topology, xyz, tree.kernel, y, SP.R, "sphere nu=0.8", GV._tol())
    tree.plan.close()


# ---- C. one pass, three inputs ---------------------------------------------------------------------------------------------------------
def test_mode_4_the_host_route_and_the_oracle_agree(hip):
    topo, X, y, R, l, _ = _problem("T16")
    spec = _spec(2.0, l)
    dev = _plan(hip, topo, X, y, R, spec)
    a = _predict(dev)
    host = hip.HipPlan(topo, 0)
    host.set_locs(X); host.set_obs(y, R)
    host.upload_host_cov(lambda p, q: spec.evaluate(p, q), X, y)
    b = _predict(host)
    o = _oracle("T16", 2.0)
    _check(a, o, ORACLE_BARS, "mode 4 vs oracle")
    _check(b, o, ORACLE_BARS, "host blocks vs oracle")
    _check(a, b, ORACLE_BARS, "mode 4 vs host blocks")
    # and it is not another family's kernel: Matern32 at the same l and sig is far away
    import pymra_amd.MRATools as mt
    dev.set_kernel(mt.KIND_MATERN32, spec.l, spec.sig, spec.scale)
    dev.run(True, False)
    assert abs(sum(dev.likelihood()) - a[0]) > 1e-3 * abs(a[0])
    dev.close(); host.close()


# ---- D. phantom knots ------------------------------------------------------------------------------------------------------------------
def test_phantom_knot_columns_stay_finite(hip):
    """r0 = 20: blocks of 32 columns holding 20 knots - twelve phantom columns at MRA_FAR_AWAY in every knot block, where t^nu
    overflows and the sum underflows."""
    import test_gpu_cov as GC
    from oracle.mra_levelwise import run_levelwise
    topo, locs, y_obs, _, R = GC._shape_tree("grid48_r20")
    assert int(topo.cw[0]) == 32 and int(topo.knot_ptr[1] - topo.knot_ptr[0]) == 20
    for nu in NUS:
        spec = _spec(nu)
        pl = _plan(hip, topo, locs, y_obs, R, spec)
        got = _predict(pl)
        _check(got, _ref3(run_levelwise(topo, locs, spec, y_obs, R)), ORACLE_BARS, "grid48_r20 nu=%g" % nu)
        pl.close()


# ---- E. the calls on the retained factors ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(hip):
    """MRATree on T16's grid at nu = 0.8 with its CPU state"""
    import pymra_amd.MRATools as mt
    from pymra_amd import MRATree
    import _treesites as TS
    topo0, locs, y, R, l, _ = _problem("T16")
    np.random.seed(7)
    tree = MRATree(locs, 16, lambda a, b: mt.Matern(a, b, l=l, sig=1.2, nu=0.8), y, R, M=2, J=4, verbose=False)
    assert tree.kernel.kind == mt.KIND_MATERN and tree.kernel.nu == 0.8 and tree.plan.route()["path"] == "Levels"
    state = TS.SiteState(tree.topology, locs, tree.kernel, y, R)
    yield tree, locs, y, R, state
    tree.plan.close()


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
    assert np.abs(ps ** 2 - sd[rows] ** 2).max() <= 1e-9 * 1.2
    t = tree.topology
    padded = np.full(len(locs), -1, dtype=np.int64)                               # prior_sigma_rows takes padded rows
    padded[t.perm[t.perm >= 0]] = np.nonzero(t.perm >= 0)[0]
    assert np.all(padded[rows] >= 0)
    S = prior_sigma_rows(t, locs, tree.kernel.evaluate, padded[rows])
    for distr, tol in (("prior", 1e-10), ("posterior", 1e-9)):                    # PRIOR_TOL / POST_NO_TRUTH_TOL, tests/test_gpu_cov.py
        cols = tree.covariance(rows, distr)
        at = tree.covarianceAt(locs[rows], distr)
        e = np.abs(at - cols[rows]).max()
        print("covarianceAt vs covariance(rows) %s: %.2e" % (distr, e))
        assert e <= tol * 1.2
        if distr == "prior":
            e = np.abs(cols[rows] - S).max()
            print("covariance(rows, prior) vs prior_sigma_rows: %.2e" % e)
            assert e <= 1e-10 * 1.2
        else:
            assert np.abs(np.diag(at) - sd[rows] ** 2).max() <= 1e-9 * 1.2


def test_sample_at_against_the_twin(fitted):
    import _treesitecov as TC
    import test_gpu_sitedraw as SD
    tree, locs, y, R, state = fitted
    rng = np.random.RandomState(5)
    sites = np.vstack([locs[rng.choice(len(locs), 12, replace=False)], rng.uniform(0.02, 0.98, size=(12, 2))])
    leaf = tree.locate(sites)
    for post, tol in ((False, 1e-10), (True, 1e-9)):                               # tests/test_gpu_sitedraw.py
        F = SD._device_F(tree.plan, sites, leaf, post)
        SD._check_FFt(F, TC.tree_sites_cov(state, sites, leaf, post), 1.2, tol, "nu=0.8 %s" % ("posterior" if post else "prior"))
    z = rng.standard_normal((tree.plan.sample_sites_slots(len(sites)), 3))
    x = tree.sampleAt(sites, 3, "prior", leaf=leaf, z=z)
    F = SD._device_F(tree.plan, sites, leaf, False)
    assert np.abs(x - F @ z).max() <= 1e-12 * 1.2 * np.abs(z).sum(axis=0).max()


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
    res = tree.crossValidate("loo")
    assert res.n > 0 and np.isfinite(res.score)


# ---- F. a change of nu on a kept tree --------------------------------------------------------------------------------------------------
def test_reevaluate_with_another_nu_equals_a_fresh_tree(hip):
    import pymra_amd.MRATools as mt
    from pymra_amd import MRATree
    topo0, locs, y, R, l, _ = _problem("T16")
    cov = lambda nu, ll=l: (lambda a, b: mt.Matern(a, b, l=ll, sig=1.2, nu=nu))

    def fresh(nu, ll=l):
        np.random.seed(7)
        return MRATree(locs, 16, cov(nu, ll), y, R, M=2, J=4, verbose=False)
    tree = fresh(0.8)
    lik1 = float(tree.getLikelihood()[0, 0])
    m1, s1 = (np.array(v).copy() for v in tree.predict())
    tab1 = tree.plan.matern_table().copy()
    lik2 = float(tree.reevaluate(cov(2.0), want_predict=True)[0, 0])
    m2, s2 = (np.array(v).copy() for v in tree.predict())
    assert not np.array_equal(tree.plan.matern_table(), tab1)
    other = fresh(2.0)
    assert lik2 == float(other.getLikelihood()[0, 0]) and lik2 != lik1
    om, os_ = other.predict()
    assert np.array_equal(m2, np.array(om)) and np.array_equal(s2, np.array(os_))
    # a change of l alone sends no table
    tab2 = tree.plan.matern_table().copy()
    lik3 = float(tree.reevaluate(cov(2.0, 0.3))[0, 0])
    assert np.array_equal(tree.plan.matern_table(), tab2) and lik3 == float(fresh(2.0, 0.3).getLikelihood()[0, 0])
    # back to the first nu: the table is rebuilt, nothing stale
    assert float(tree.reevaluate(cov(0.8), want_predict=True)[0, 0]) == lik1
    mb, sb = tree.predict()
    assert np.array_equal(np.array(mb), m1) and np.array_equal(np.array(sb), s1) and np.array_equal(tree.plan.matern_table(), tab1)
    # a closed-form nu goes to the closed-form kind on the same tree
    tree.reevaluate(cov(1.5))
    assert tree.kernel.kind == mt.KIND_MATERN32 and tree.plan.matern_table().shape == (0, 2)
    tree.plan.close(); other.plan.close()
