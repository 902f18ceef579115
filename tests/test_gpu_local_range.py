"""MRA_KERNEL_LOCAL on the GPU: a nonstationary covariance with a local range at every location, evaluated on the device (mode 6).

A. The function: mra_eval_kernel_local against the longdouble formula on the 40 001 distances of the parity test, each paired with
   two ranges drawn over two decades, for ds = 1 and 2 and the four base kinds, at a bar derived from the device function's
   operation count (test_the_device_function_against_longdouble); D = 0 with la = lb gives exactly amp, a phantom-sized range exactly 0.
B. Passes against run_levelwise with LocalRange.evaluate at the project's bars (likelihood 1e-10 relative, mean
   1e-9, sd 1e-8 relative) on T16 (also with MRA_OPT_FUSED = 0), A32, C64 and the 1-D tree L16 with (x, lam) rows; the range varies
   tenfold across the domain, 40 % observed and the first leaf empty; predicting and likelihood-only; route and prior_level asserted.
C. A constant range against the stationary plan of range l * lam0, four base kinds; mode 6, the MRA_KERNEL_HOST plan fed by
   LocalRange.evaluate and the oracle pairwise.
D. The phantom-knot tree of tests/test_gpu_kernel_sum.py.
E. The calls on the retained factors against the CPU twins fed through evaluate (_treesolve with the whole quad block, _treesites,
   _treesitecov, _treesitedraw slot by slot, _treecv, _treetrend); reevaluate, setLocalRange, and a stationary kernel on the same
   plan: the fused route again; a 1-D MRATree(local_range=) and a noise vector against the rescaled oracle.
F. One sharded pass (world 2) against the sharded oracle."""
import dataclasses
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
BASES = (0, 1, 2, 3)
LD = np.longdouble


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _spec(kind=1, l=1.0, sig=1.1, scale=1.0):
    import pymra_amd.MRATools as mt
    return mt.LocalRange(mt.KernelSpec(kind, l, 1.0 if kind == 0 else sig, scale))


def _field(locs, lo):
    """a range that grows tenfold, lo .. 10 lo, along the first coordinate (with a ripple across the second)"""
    locs = np.asarray(locs, float).reshape(len(locs), -1)
    u = (locs[:, 0] - locs[:, 0].min()) / (locs[:, 0].max() - locs[:, 0].min())
    if locs.shape[1] > 1:
        u = u * (0.9 + 0.1 * np.sin(7.0 * locs[:, 1]))
    return lo * 10.0 ** u


def _plan(hip, topo, X, y, R, spec, opts=()):
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(X); pl.set_obs(y, R)
    pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale, spec.circular)
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
L0, SIG, SCALE = 0.8, 1.7, 1.5
N_EDGE = 8


@pytest.fixture(scope="module")
def pairs():
    """(D, la, lb): the parity test's distances with ranges over two decades, then the edge cases: D = 0 with la = lb (4), and a
    phantom-sized range on one side, on the other, on both, and on both with a phantom's distance (4)"""
    rng = np.random.RandomState(1)
    D = np.concatenate([[0.0], np.abs(rng.normal(size=20000)) * 0.7, 10.0 ** rng.uniform(-9, 2, size=20000)])
    assert len(D) == 40001
    la, lb = 10.0 ** rng.uniform(-2, 0, size=len(D)), 10.0 ** rng.uniform(-2, 0, size=len(D))
    eq = np.array([0.013, 0.37, 1.0, 7.3e-3])
    far = 1.0e150
    D = np.concatenate([D, np.zeros(4), [0.3, 0.3, 0.0, 3.0 * far]])
    la = np.concatenate([la, eq, [2.0 * far, 0.2, 5.0 * far, 2.0 * far]])
    lb = np.concatenate([lb, eq, [0.2, 14.0 * far, 5.0 * far, 33.0 * far]])
    return D, la, lb


def _longdouble(kind, ds, D, la, lb):
    D, la, lb = D.astype(LD), la.astype(LD), lb.astype(LD)
    q = (la ** 2 + lb ** 2) / LD(2)
    pref = (la * lb / q) ** (LD(ds) / LD(2))
    r = D / (LD(L0) * np.sqrt(q))
    if kind == 0:
        k0 = np.exp(-r)
    elif kind == 1:
        k0 = (1 + np.sqrt(LD(3)) * r) * np.exp(-np.sqrt(LD(3)) * r)
    elif kind == 2:
        k0 = (1 + np.sqrt(LD(5)) * r + LD(5) / LD(3) * r ** 2) * np.exp(-np.sqrt(LD(5)) * r)
    else:
        k0 = np.exp(-r ** 2 / LD(2))
    return LD(SCALE) * LD(1.0 if kind == 0 else SIG) * pref * k0


@pytest.mark.parametrize("ds", (1, 2))
@pytest.mark.parametrize("kind", BASES)
def test_the_device_function_against_longdouble(hip, pairs, kind, ds):
    """The bar, from the operation count of cov_local_of (mra_kernels.h), in units of eps = 2^-53 of the sill amp:
    t: D D (1), q = (la la + lb lb) / 2 (2), its reciprocal (rcp_pos: 1 ulp = 2) -> 5 with the product's own 1 -> s = D2 / q: 6;
       the root halves it and adds sqrt_pos's 1 ulp: 5; times c / l (a host constant with 1, and the product 1): t within 7 - the
       Gaussian base takes s times 1 / (2 l^2) (2) and the product (1): 9.  |d k0| <= max t |k0'(t)| times that: 0.62 * 7 (Matern52:
       t (t + t^2) e^-t / 3 <= 0.62) or 0.37 * 9 (t e^-t <= 1 / e): below 5;
    exp_neg (reduction 1/2, thirteen Horner steps whose roundings enter times |r|^k: 2, the final ldexp exact): 3;
    the polynomial's two fma: 2, its product with the exponential: 1;
    the prefactor: la lb (1) over q (2) as a correctly rounded quotient (1/2), in 1-D sqrt_pos (halves, + 2): 4; times amp, a host
       product (1), and the product (1): 6;  the last product: 1.
    Sum 18; the bar is 20 eps = 10 * 2^-52 amp.  The longdouble reference is 2^-11 eps away from the formula.
    Measured on an MI355X: 2.7 to 4.3 eps over the eight cases; D = 0 with la = lb exactly amp, phantom ranges exactly 0."""
    D, la, lb = pairs
    sig = 1.0 if kind == 0 else SIG
    amp = SCALE * sig
    got = hip.eval_kernel_local(kind, L0, sig, SCALE, ds, D, la, lb)
    assert np.all(np.isfinite(got))
    n = len(D) - N_EDGE
    err = np.abs(got[:n].astype(LD) - _longdouble(kind, ds, D[:n], la[:n], lb[:n]))
    print("kind %d ds %d: max |device - longdouble| / amp = %.3e = %.2f eps (bar 20 eps)" % (kind, ds, float(err.max()) / amp, float(err.max()) / amp * 2.0 ** 53))
    assert float(err.max()) <= 20 * 2.0 ** -53 * amp
    # D = 0 with la = lb: exactly amp - the quotient la lb / q takes the division's correction step, and la la == q to the bit
    print("D = 0, la = lb:", got[n:n + 4], "amp", amp, "phantom ranges:", got[n + 4:])
    assert np.all(got[n:n + 4] == amp)
    same = hip.eval_kernel_local(kind, L0, sig, SCALE, ds, np.zeros(n), la[:n], la[:n])
    assert np.all(same == amp)
    # a phantom's range on either side: exactly 0
    assert np.all(got[n + 4:] == 0.0)


def test_eval_kernel_local_refuses_what_set_kernel_refuses(hip):
    for kind, l, sig in ((4, 0.3, 1.0), (5, 0.3, 1.0), (1, 0.0, 1.0), (1, 0.3, -1.0)):
        with pytest.raises(hip.MraError) as e:
            hip.eval_kernel_local(kind, l, sig, 1.0, 2, np.zeros(3), np.ones(3), np.ones(3))
        assert e.value.code == -1
    with pytest.raises(hip.MraError):
        hip.eval_kernel_local(1, 0.3, 1.0, 1.0, 2, np.zeros(3), np.ones(3), np.array([1.0, 0.0, 1.0]))


# ---- B. passes -----------------------------------------------------------------------------------------------------------------------
def _mask(topo, seed=0):
    """40 % observed, the first leaf without any observation"""
    obs = np.random.RandomState(seed).uniform(size=topo.N) < 0.4
    MK._empty(obs, topo, [int(np.nonzero(topo.node_leaf)[0][0])])
    return obs


@functools.lru_cache(maxsize=None)
def _problem(cell):
    """(topology with one coordinate column more, [locs | lam], y, R, spatial locs, lam)"""
    if cell in RC.TREES:
        topo, locs = MK._tree(*RC.TREES[cell])
        y, R, lo = MK._y(_mask(topo)), R2, 0.05
    else:
        topo, locs, obs, y, counts = LC.problem("L16")
        assert counts[0] == 0
        y, R, lo = y.reshape(-1, 1), LC.R, 0.004
    lam = _field(locs, lo)
    assert lam.min() > 0 and 8.0 < lam.max() / lam.min() <= 10.0 + 1e-9
    locs = np.asarray(locs, float).reshape(len(lam), -1)
    return dataclasses.replace(topo, coord_dim=locs.shape[1] + 1), np.column_stack([locs, lam]), y, R, locs, lam


@functools.lru_cache(maxsize=None)
def _oracle(cell, kind=1):
    from oracle.mra_levelwise import run_levelwise
    topo, X, y, R, _, _ = _problem(cell)
    return _ref3(run_levelwise(topo, X, _spec(kind), y, R))


CELLS = [("T16", ()), ("T16", ((MRA_OPT_FUSED, 0),)), ("A32", ()), ("C64", ()), ("L16", ())]


@pytest.mark.parametrize("cell,opts", CELLS, ids=["%s%s" % (c, "-fused0" if o else "") for c, o in CELLS])
def test_passes_against_the_oracle(hip, cell, opts):
    topo, X, y, R, _, _ = _problem(cell)
    pl = _plan(hip, topo, X, y, R, _spec(), opts)
    assert pl.d == X.shape[1]
    got = _predict(pl)
    rt = pl.route()
    assert rt["path"] == "Levels", rt                                 # no fused instance of mode 6: the prior goes level by level
    assert rt["prior_level"], rt                                     # ... through the one-launch prior levels (k_leaf_gemm<COV, SOLVE>)
    _check(got, _oracle(cell), ORACLE_BARS, "%s %s" % (cell, opts))
    pl.run(True, False)                                              # the likelihood-only pass (gathered rows)
    lik = sum(pl.likelihood())
    ref = _oracle(cell)[0]
    print("%s likelihood-only: %.2e" % (cell, abs(lik - ref) / abs(ref)))
    assert abs(lik - ref) <= ORACLE_BARS[0] * abs(ref), (lik, ref)
    assert pl.route()["path"] == "Levels"
    pl.close()


@pytest.mark.parametrize("kind", (0, 2, 3))
def test_the_other_base_kinds_on_t16(hip, kind):
    topo, X, y, R, _, _ = _problem("T16")
    pl = _plan(hip, topo, X, y, R, _spec(kind))
    _check(_predict(pl), _oracle("T16", kind), ORACLE_BARS, "T16 base %d" % kind)
    assert abs(_oracle("T16", kind)[0] - _oracle("T16")[0]) > 1e-3 * abs(_oracle("T16")[0])
    pl.close()


# ---- C. a constant range; one pass, three inputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BASES)
def test_a_constant_range_is_the_stationary_plan(hip, kind):
    topo3, X, y, R, locs, _ = _problem("T16")
    topo2, _ = MK._tree(*RC.TREES["T16"])
    lam0, l = 0.25, 1.3
    Xc = np.column_stack([locs, np.full(len(locs), lam0)])
    loc = _plan(hip, topo3, Xc, y, R, _spec(kind, l=l, sig=1.2, scale=0.8))
    a = _predict(loc)
    assert loc.route()["path"] == "Levels"
    flat = hip.HipPlan(topo2, 0)
    flat.set_locs(locs); flat.set_obs(y, R)
    flat.set_kernel(kind, l * lam0, 1.0 if kind == 0 else 1.2, 0.8)
    b = _predict(flat)
    _check(a, b, ORACLE_BARS, "kind %d: constant range against the stationary plan" % kind)
    loc.close(); flat.close()


def test_mode_6_the_host_route_and_the_oracle_agree(hip):
    topo, X, y, R, _, _ = _problem("T16")
    spec = _spec()
    dev = _plan(hip, topo, X, y, R, spec)
    a = _predict(dev)
    host = hip.HipPlan(topo, 0)
    host.set_locs(X); host.set_obs(y, R)
    host.upload_host_cov(lambda p, q: spec.evaluate(p, q), X, y)
    b = _predict(host)
    o = _oracle("T16")
    _check(a, o, ORACLE_BARS, "mode 6 vs oracle")
    _check(b, o, ORACLE_BARS, "host blocks vs oracle")
    _check(a, b, ORACLE_BARS, "mode 6 vs host blocks")
    # and the range field matters: the stationary Matern32 of the median range is far away
    import pymra_amd.MRATools as mt
    dev.set_kernel(mt.KIND_MATERN32, float(np.median(X[:, 2])), 1.1, 1.0)
    dev.run(True, False)
    assert abs(sum(dev.likelihood()) - a[0]) > 1e-3 * abs(a[0])
    dev.close(); host.close()


# ---- D. phantom knots ------------------------------------------------------------------------------------------------------------------
def test_phantom_knot_columns_stay_finite(hip):
    """r0 = 20: blocks of 32 columns holding 20 knots - twelve phantom columns in every knot block."""
    import test_gpu_cov as GC
    from oracle.mra_levelwise import run_levelwise
    topo, locs, y_obs, _, R = GC._shape_tree("grid48_r20")
    assert int(topo.cw[0]) == 32 and int(topo.knot_ptr[1] - topo.knot_ptr[0]) == 20
    X = np.column_stack([locs, _field(locs, 0.05)])
    topo3 = dataclasses.replace(topo, coord_dim=3)
    for kind in (2, 3):
        spec = _spec(kind)
        pl = _plan(hip, topo3, X, y_obs, R, spec)
        got = _predict(pl)
        _check(got, _ref3(run_levelwise(topo3, X, spec, y_obs, R)), ORACLE_BARS, "grid48_r20 base %d" % kind)
        pl.close()


# ---- E. the calls on the retained factors ----------------------------------------------------------------------------------------------
def _cov(l=1.0, sig=1.1):
    import pymra_amd.MRATools as mt
    return lambda a, b: mt.Matern32(a, b, l=l, sig=sig)


def _fresh(locs, y, R, lam, cov):
    from pymra_amd import MRATree
    np.random.seed(7)
    return MRATree(locs, 16, cov, y, R, M=2, J=4, verbose=False, local_range=lam)


@pytest.fixture(scope="module")
def fitted(hip):
    """MRATree on T16's grid with the range field of B and its CPU state"""
    import pymra_amd.MRATools as mt
    import _treesites as TS
    topo0, X, y, R, locs, lam = _problem("T16")
    tree = _fresh(locs, y, R, lam, _cov())
    assert isinstance(tree.kernel, mt.LocalRange) and tree.kernel.l == (mt.KIND_MATERN32, 1.0) and tree.plan.route()["path"] == "Levels"
    assert tree.plan.d == 3 and np.array_equal(tree.cov_locs, X) and np.array_equal(tree.topology.perm, topo0.perm)
    state = TS.SiteState(tree.topology, X, tree.kernel, y, R)
    yield tree, X, locs, lam, y, R, state
    tree.plan.close()


def _padded_rows(t, rows, n):
    padded = np.full(n, -1, dtype=np.int64)                                       # prior_sigma_rows takes padded rows
    padded[t.perm[t.perm >= 0]] = np.nonzero(t.perm >= 0)[0]
    assert np.all(padded[rows] >= 0)
    return padded[rows]


def test_the_tree_against_the_oracle(fitted):
    tree, X, locs, lam, y, R, state = fitted
    mean, sd = tree.predict()
    got = (float(tree.getLikelihood()[0, 0]), np.asarray(mean).ravel(), np.asarray(sd).ravel())
    _check(got, _oracle("T16"), ORACLE_BARS, "MRATree(local_range=)")


def test_solve_predict_at_and_covariance_at(fitted):
    from oracle.mra_faithful import prior_sigma_rows
    tree, X, locs, lam, y, R, state = fitted
    mean, sd = tree.predict()
    mean, sd = np.asarray(mean).ravel(), np.asarray(sd).ravel()
    scale = max(1.0, np.abs(mean).max())
    m1, quad = tree.solve(np.nan_to_num(y))
    print("solve vs predict: %.2e" % np.abs(m1[:, 0] - mean).max())
    assert np.abs(m1[:, 0] - mean).max() <= 1e-8 * scale                          # tests/test_gpu_solve.py
    rows = np.random.RandomState(3).choice(len(locs), 40, replace=False)
    # at tree locations with their own range, predictAt reproduces predict()
    pm, ps = tree.predictAt(locs[rows], local_range=lam[rows])
    print("predictAt vs predict: mean %.2e sd %.2e" % (np.abs(pm[:, 0] - mean[rows]).max(), np.abs(ps - sd[rows]).max()))
    assert np.abs(pm[:, 0] - mean[rows]).max() <= 1e-9 * scale                    # POST_NO_TRUTH_TOL, tests/test_gpu_sites.py
    assert np.abs(ps ** 2 - sd[rows] ** 2).max() <= 1e-9 * 1.1
    with pytest.raises(ValueError):
        tree.predictAt(locs[rows])                                               # local_range is mandatory
    from pymra_amd.plan import MraError
    with pytest.raises(MraError):                                                # a site's range is checked as the plan's are
        tree.plan.predict_sites(np.column_stack([locs[rows], -lam[rows]]), tree.locate(locs[rows], local_range=lam[rows]))
    t = tree.topology
    S = prior_sigma_rows(t, X, tree.kernel.evaluate, _padded_rows(t, rows, len(locs)))
    for distr, tol in (("prior", 1e-10), ("posterior", 1e-9)):                    # PRIOR_TOL / POST_NO_TRUTH_TOL, tests/test_gpu_cov.py
        cols = tree.covariance(rows, distr)
        at = tree.covarianceAt(locs[rows], distr, local_range=lam[rows])
        e = np.abs(at - cols[rows]).max()
        print("covarianceAt vs covariance(rows) %s: %.2e" % (distr, e))
        assert e <= tol * 1.1
        if distr == "prior":
            e = np.abs(cols[rows] - S).max()
            print("covariance(rows, prior) vs prior_sigma_rows: %.2e" % e)
            assert e <= 1e-10 * 1.1
        else:
            assert np.abs(np.diag(at) - sd[rows] ** 2).max() <= 1e-9 * 1.1


def test_solve_against_the_twin(fitted):
    """five right-hand sides, the first the tree's own observations, against tests/_treesolve.py: the means and the whole quad block,
    at the bound of tests/test_gpu_solve.py (1e-9 of the field scale and of the largest quad)"""
    import _treesolve as TSV
    from test_gpu_solve import _columns
    tree, X, locs, lam, y, R, state = fitted
    Y = _columns(y, 5)
    mean, quad = tree.solve(Y)
    wm, wq = TSV.tree_solve(tree.topology, X, tree.kernel, y, R, Y)
    e_m, e_q = np.abs(mean - wm).max(), np.abs(quad - wq).max()
    print("solve vs the twin: mean %.2e (scale %.2f), quad %.2e (scale %.1f)" % (e_m, np.abs(wm).max(), e_q, np.abs(np.diag(wq)).max()))
    assert mean.shape == (len(locs), 5) and quad.shape == (5, 5)
    assert e_m <= 1e-9 * max(1.0, np.abs(wm).max())
    assert e_q <= 1e-9 * np.abs(np.diag(wq)).max()


def test_predict_at_new_sites_against_the_twin(fitted):
    import _treesites as TS
    tree, X, locs, lam, y, R, state = fitted
    rng = np.random.RandomState(11)
    sites = rng.uniform(0.02, 0.98, size=(24, 2))
    ls = 0.05 * 10.0 ** sites[:, 0] * rng.uniform(0.8, 1.2, size=24)
    leaf = tree.locate(sites, local_range=ls)
    pm, ps = tree.predictAt(sites, leaf=leaf, local_range=ls)
    wm, wv = TS.tree_sites(tree.topology, X, tree.kernel, y, R, np.column_stack([sites, ls]), leaf, state=state)
    wm, wv = np.asarray(wm), np.asarray(wv).ravel()
    scale = max(1.0, np.abs(wm).max())
    print("predictAt at new sites vs the twin: mean %.2e var %.2e" % (np.abs(pm[:, 0] - wm.ravel()).max(), np.abs(ps ** 2 - wv).max()))
    assert np.abs(pm[:, 0] - wm.ravel()).max() <= 1e-9 * scale and np.abs(ps ** 2 - wv).max() <= 1e-9 * 1.1


def test_sample_at_against_the_twin(fitted):
    import _treesitecov as TC
    import test_gpu_sitedraw as SD
    tree, X, locs, lam, y, R, state = fitted
    rng = np.random.RandomState(5)
    pick = rng.choice(len(locs), 12, replace=False)
    new = rng.uniform(0.02, 0.98, size=(12, 2))
    sites = np.vstack([locs[pick], new])
    ls = np.concatenate([lam[pick], 0.05 * 10.0 ** new[:, 0]])
    S3 = np.column_stack([sites, ls])
    leaf = tree.locate(sites, local_range=ls)
    import _treesitedraw as TD
    for post, tol in ((False, 1e-10), (True, 1e-9)):                               # tests/test_gpu_sitedraw.py
        F = SD._device_F(tree.plan, S3, leaf, post)
        truth = TC.tree_sites_cov(state, S3, leaf, post)
        SD._check_FFt(F, truth, 1.1, tol, "local %s" % ("posterior" if post else "prior"))
        Ft, _ = TD.site_draw_factor(state, S3, leaf, post, {})                    # the factor itself, slot by slot
        e_f = np.abs(F - Ft).max()
        at = tree.covarianceAt(sites, "posterior" if post else "prior", leaf=leaf, local_range=ls)      # tree locations and new sites
        e_c = np.abs(at - truth).max()
        print("local %s: |F - twin F| %.2e, |covarianceAt - twin| %.2e" % ("posterior" if post else "prior", e_f, e_c))
        assert e_f <= tol * 1.1 and e_c <= tol * 1.1
    z = rng.standard_normal((tree.plan.sample_sites_slots(len(sites)), 3))
    x = tree.sampleAt(sites, 3, "prior", leaf=leaf, z=z, local_range=ls)
    F = SD._device_F(tree.plan, S3, leaf, False)
    assert np.abs(x - F @ z).max() <= 1e-12 * 1.1 * np.abs(z).sum(axis=0).max()


def test_cross_validation_against_the_twin(fitted):
    import _treecv as CV
    import test_gpu_cv as GV
    tree, X, locs, lam, y, R, state = fitted
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


def test_a_trend_fit_against_the_twin(hip, fitted):
    import _treetrend as TT
    import test_gpu_trend as GT
    tree, X, locs, lam, y, R, state = fitted
    Xd = GT._design(len(locs), 3)
    yt = GT._with_trend(y, Xd)
    GT._check_fit(hip, tree.topology, X, tree.kernel, yt, R, Xd, TT.tree_trend(tree.topology, X, tree.kernel, yt, R, Xd))
    lik0 = float(tree.getLikelihood()[0, 0])
    lik = float(tree.setTrend(Xd)[0, 0])
    assert np.isfinite(lik) and tree.trend.beta.shape == (3,) and lik != lik0
    assert float(tree.setTrend(None)[0, 0]) == lik0


def test_reevaluate_set_local_range_and_back_to_a_stationary_kernel(hip):
    import pymra_amd.MRATools as mt
    topo0, X, y, R, locs, lam = _problem("T16")
    tree = _fresh(locs, y, R, lam, _cov())
    lik1 = float(tree.getLikelihood()[0, 0])
    m1, s1 = (np.array(v).copy() for v in tree.predict())
    # another l and sig: parameters only, and a fresh tree's bits
    lik2 = float(tree.reevaluate(_cov(1.4, 0.9), want_predict=True)[0, 0])
    m2, s2 = (np.array(v).copy() for v in tree.predict())
    other = _fresh(locs, y, R, lam, _cov(1.4, 0.9))
    assert lik2 == float(other.getLikelihood()[0, 0]) and lik2 != lik1 and tree.plan.route()["path"] == "Levels"
    om, os_ = other.predict()
    assert np.array_equal(m2, np.array(om)) and np.array_equal(s2, np.array(os_))
    # another range field
    lam3 = lam[::-1].copy()
    lik3 = float(tree.setLocalRange(lam3, want_predict=True)[0, 0])
    f3 = _fresh(locs, y, R, lam3, _cov(1.4, 0.9))
    assert lik3 == float(f3.getLikelihood()[0, 0]) and lik3 != lik2
    m3, s3 = tree.predict()
    fm, fs = f3.predict()
    assert np.array_equal(np.array(m3), np.array(fm)) and np.array_equal(np.array(s3), np.array(fs))
    with pytest.raises(ValueError):
        tree.setLocalRange(-lam)
    # back to the first model: the first bits
    tree.setLocalRange(lam)
    assert float(tree.reevaluate(_cov(), want_predict=True)[0, 0]) == lik1
    mb, sb = tree.predict()
    assert np.array_equal(np.array(mb), m1) and np.array_equal(np.array(sb), s1)
    # a stationary kernel on the same plan (the three columns are then plain coordinates): the fused route again, and a fresh plan's bits
    pl = tree.plan
    pl.set_kernel(mt.KIND_MATERN32, 0.3, 1.1, 1.0)
    a = _predict(pl)
    assert pl.route()["path"] == "Fused"
    plain = hip.HipPlan(tree.topology, 0)
    plain.set_locs(X); plain.set_obs(y, R); plain.set_kernel(mt.KIND_MATERN32, 0.3, 1.1, 1.0)
    b = _predict(plain)
    assert plain.route()["path"] == "Fused" and a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # ... and the local ranges once more
    assert float(tree.reevaluate(_cov())[0, 0]) == lik1 and pl.route()["path"] == "Levels"
    for t in (tree, other, f3):
        t.plan.close()
    plain.close()


def test_a_1d_tree_with_local_ranges(hip):
    """MRATree on (N, 1) locations: covariance coordinates (x, lam), the DIM = 2 instances, against the oracle of B's L16 cell"""
    import pymra_amd.MRATools as mt
    from pymra_amd import MRATree
    topo, X, y, R, locs, lam = _problem("L16")
    np.random.seed(7)
    tree = MRATree(locs, 16, _cov(), y, R, M=2, J=3, verbose=False, local_range=lam)
    assert tree.d == 1 and tree.plan.d == 2 and np.array_equal(tree.cov_locs, X) and np.array_equal(tree.topology.perm, topo.perm)
    assert isinstance(tree.kernel, mt.LocalRange) and tree.plan.route()["path"] == "Levels"
    mean, sd = tree.predict()
    got = (float(tree.getLikelihood()[0, 0]), np.asarray(mean).ravel(), np.asarray(sd).ravel())
    _check(got, _oracle("L16"), ORACLE_BARS, "1-D MRATree(local_range=)")
    rows = np.random.RandomState(3).choice(len(locs), 30, replace=False)
    pm, ps = tree.predictAt(locs[rows, 0], local_range=lam[rows])                # (n,) sites
    scale = max(1.0, np.abs(got[1]).max())
    print("1-D predictAt vs predict: mean %.2e var %.2e" % (np.abs(pm[:, 0] - got[1][rows]).max(), np.abs(ps ** 2 - got[2][rows] ** 2).max()))
    assert np.abs(pm[:, 0] - got[1][rows]).max() <= 1e-9 * scale and np.abs(ps ** 2 - got[2][rows] ** 2).max() <= 1e-9 * 1.1
    tree.plan.close()


def test_a_noise_vector_with_local_ranges(hip):
    """per-observation noise variances r = R s(x)^2 on a mode-6 plan against the rescaled oracle of tests/_noise.py (the problem
    (C, y, diag r) is (C / (s s'), y / s, R I)), at the bars of tests/test_gpu_noise.py; and through MRATree(R=array)"""
    import _noise as NZ
    topo, X, y, R, locs, lam = _problem("T16")
    spec = _spec()
    r = NZ.noise_of(locs, R)
    ref = NZ.scaled_oracle(topo, X, spec, y, R)
    pl = _plan(hip, topo, X, y, R, spec)
    scalar = _predict(pl)
    pl.set_noise(r)
    got = _predict(pl)
    assert pl.route()["path"] == "Levels" and got[0] != scalar[0]
    _check(got, (ref["lik"], np.asarray(ref["mean"]).ravel(), np.asarray(ref["sd"]).ravel()), ORACLE_BARS, "noise vector, mode 6")
    pl.close()
    tree = _fresh(locs, y, r, lam, _cov())
    mean, sd = tree.predict()
    tg = (float(tree.getLikelihood()[0, 0]), np.asarray(mean).ravel(), np.asarray(sd).ravel())
    _check(tg, (ref["lik"], np.asarray(ref["mean"]).ravel(), np.asarray(ref["sd"]).ravel()), ORACLE_BARS, "MRATree(R=array, local_range=)")
    tree.plan.close()


# ---- F. one sharded cell -----------------------------------------------------------------------------------------------------------------
def test_a_sharded_pass_against_the_sharded_oracle(hip):
    topo, X, y, R, _, _ = _problem("T16")
    spec = _spec()
    liks, mean, var, lvl = K.emulate_world_on_one_gpu(hip, topo, X, y, R, spec, 2)
    rl, rm, rv, rlvl = K.emulate_world_oracle(topo, X, y, R, spec, 2)
    assert lvl == rlvl
    for a, b in zip(liks, rl):
        assert abs(a - b) <= ORACLE_BARS[0] * abs(b), (a, b)
    ok = rv > 0
    e_m, e_s = np.abs(mean - rm).max(), (np.abs(np.sqrt(var[ok]) - np.sqrt(rv[ok])) / np.sqrt(rv[ok])).max()
    print("world 2: lik %.2e mean %.2e sd %.2e" % (max(abs(a - b) / abs(b) for a, b in zip(liks, rl)), e_m, e_s))
    assert e_m <= ORACLE_BARS[1] and e_s <= ORACLE_BARS[2]
