"""mra_cv_trend / HipPlan.cv_trend / MRATree.crossValidate(trend=...) on the GPU: cross-validation of a tree with a regression trend from
the retained factors, beta estimated again without each group ("refit") or held at the full fit's ("fixed").  Truths that do not come
from the new kernels: the NumPy restatement tests/_treecv_trend.py (pinned to brute force by tests/test_cv_trend_cpu.py), refits on
the device itself (a tree built again with the group's observations NaN: its predict()), mra_cv on y - X beta^, and central differences
of mra_trend_fit's profile and REML values.

Measures, as tests/test_cv_trend_cpu.py: mean |delta| / max|y|; variance relative; lpd and score |delta| / max(1, |value|); tr K^-1,
tr P, |P y|^2 and the leverage relative; the two derivatives relative to max(tr K^-1, |P y|^2), the terms they are the difference of.
Bound against the twin: max(1e-9, 100 x the twin's own error against brute force on that case, tests/_treecv_trend.TWIN_ERR); on
trees without a figure of their own that of the case with the largest leverage measured, g32 (0.972); where the leverage the mode
divides by exceeds 0.98 the bound is scaled by (0.02 / (1 - leverage))^2, what the identity loses there (tests/test_gpu_cv.py)."""
import ctypes as C

import numpy as np
import pytest

import _cases as K
import _sampling as SM
import _treecv as CV
import _treecv_trend as CT
import _treesites as TS
import _treetrend as TT
import test_gpu_cov as GC

pytestmark = pytest.mark.gpu

CASES = ["g32", "c1", "kat3", "u3"]
R_CV = 1e-2
H_MAX = 0.972
MODES = [(leaf, refit) for leaf in (False, True) for refit in (True, False)]


def _tol(name="g32"):
    return max(1e-9, 100.0 * CT.TWIN_ERR[name])


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _rel1(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def _name(leaf, refit):
    return "%s %s" % ("refit" if refit else "fixed", "by leaf" if leaf else "by row")


def _errors(got, want, ymax):
    """(mean, variance, lpd, group lpd, sums, by-products, derivatives) errors of two (mean, var, lpd, group, info[12]) results"""
    for a, b in zip(got[:4], want[:4]):
        assert np.array_equal(np.isnan(a), np.isnan(b))
    ok, gk = ~np.isnan(want[0]), ~np.isnan(want[3])
    gi, wi = got[4], want[4]
    e_m = np.abs(got[0][ok] - want[0][ok]).max() / ymax
    e_v = (np.abs(got[1][ok] - want[1][ok]) / want[1][ok]).max()
    e_l = _rel1(got[2][ok], want[2][ok]).max()
    e_g = _rel1(got[3][gk], want[3][gk]).max()
    e_s = max(_rel1(gi[k], wi[k]) for k in (2, 3, 4))
    e_b = max(abs(gi[k] - wi[k]) / abs(wi[k]) for k in (5, 6, 7, 8))
    e_d = max(abs(gi[k] - wi[k]) for k in (10, 11)) / max(abs(wi[6]), abs(wi[7]))
    assert gi.shape == (12,) and gi[0] == wi[0] and gi[1] == wi[1] and gi[9] == wi[9]
    assert gi[10] == gi[6] - gi[7] and gi[11] == gi[8] - gi[7]
    return e_m, e_v, e_l, e_g, e_s, e_b, e_d


def _plan(hip, topo, locs, y_obs, R, spec, X, run=True):
    pl = GC._plan(hip, topo, locs, y_obs, R, spec, run=run)
    pl.set_trend(X)
    return pl


def _against_twin(pl, topo, locs, spec, y_obs, R, X, tag, tol, modes=MODES, four_cases=False):
    S = TS.SiteState(topo, locs, spec, y_obs, R)
    fit = TT.tree_trend(topo, locs, spec, y_obs, R, X)
    ymax = np.nanmax(np.abs(np.asarray(y_obs, float)))
    out = {}
    for leaf, refit in modes:
        want = CT.tree_cv_trend(S, X, leaf, refit, fit=fit)
        got = pl.cv_trend(leaf=leaf, refit=refit)
        e = _errors(got, want, ymax)
        lev = got[4][5]
        print("%s p = %d %s: %d rows, %d groups against the twin: mean %.2e, var %.2e, lpd %.2e, group lpd %.2e, sums %.2e, by-products %.2e, "
              "derivatives %.2e (leverage %.6f, bound %.1e)" % (tag, X.shape[1], _name(leaf, refit), got[4][0], got[4][1], *e, lev, tol))
        assert lev <= H_MAX or not four_cases                  # the four cases: a condition of the test
        assert max(e) <= tol * max(1.0, (0.02 / (1.0 - lev)) ** 2)
        out[(leaf, refit)] = got
    return out


def _leaves(topo):
    return [int(i) for i in np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]]


# ---- 1. the device against the twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_device_against_the_twin(hip, name, p):
    cs = K.load_case(name)
    topo, locs, spec, y_obs = cs["topo"], cs["locs"], cs["spec"], cs["y_obs"]
    X = CT.design(locs, p)
    pl = _plan(hip, topo, locs, y_obs, R_CV, spec, X)
    got = _against_twin(pl, topo, locs, spec, y_obs, R_CV, X, name, _tol(name), four_cases=True)
    for key, (mean, var, lpd, group, info) in got.items():
        assert abs(np.nansum(group) - info[2]) <= 1e-12 * max(1.0, abs(info[2]))
        assert abs(np.nansum(lpd) - info[3]) <= 1e-12 * max(1.0, abs(info[3]))
        if not key[0]:
            assert info[2] == info[3]                            # every row its own group
    # |P y|^2, tr K^-1 and tr P do not depend on the grouping or the mode; the traces are formed from h~ by row under refit, else from h
    assert len({g[4][7] for g in got.values()}) == 1
    for k in (6, 8):
        v = [g[4][k] for g in got.values()]
        assert max(v) - min(v) <= 1e-12 * abs(v[0])
    pl.close()


# ---- 2. shapes where the new kernels can go wrong -------------------------------------------------------------------------------------
P_SHAPES = [1, 3, 4, 15, 16, 17, 63]              # the padding of W's rows at 4 and at 16, and all four 16-column blocks of L_A^-1


@pytest.mark.parametrize("p", P_SHAPES)
def test_covariate_counts_on_g32(hip, p):
    cs = K.load_case("g32")
    topo, locs, spec, y_obs = cs["topo"], cs["locs"], cs["spec"], cs["y_obs"]
    X = CT.design(locs, p, coords=True)
    pl = _plan(hip, topo, locs, y_obs, R_CV, spec, X)
    _against_twin(pl, topo, locs, spec, y_obs, R_CV, X, "g32", _tol())
    pl.close()


@pytest.mark.parametrize("p", P_SHAPES)
def test_covariate_counts_on_the_gappy_tree(hip, p):
    """64^2, r0 = 16, M = 3: an empty leaf, an empty family, observation counts that are no multiple of 4"""
    import test_gpu_trend as GT
    topo, locs, y_obs = GT._gappy()
    X = GT._design(topo.N, p)
    y = GT._with_trend(y_obs, X)
    pl = _plan(hip, topo, locs, y, GT.R_MASK, GT._spec(), X)
    got = _against_twin(pl, topo, locs, GT._spec(), y, GT.R_MASK, X, "gappy 64^2", _tol())
    first = _leaves(topo)[0]
    assert all(np.isnan(g[3][first]) for g in got.values())      # the empty first leaf has no group
    pl.close()


def test_leaves_of_1_16_and_17_observations(hip):
    cs = K.load_case("g32")
    topo, locs, spec = cs["topo"], cs["locs"], cs["spec"]
    y = np.asarray(cs["y_obs"], float).reshape(-1, 1).copy()
    full = np.random.default_rng(3).standard_normal(len(y))
    leaves = _leaves(topo)
    for i, cnt in zip((leaves[1], leaves[6], leaves[11]), (1, 16, 17)):   # padding columns of N~_G stay the identity: their w is 0
        rows = K.node_real_rows(topo, i)
        y[topo.perm[rows], 0] = np.nan
        y[topo.perm[rows[:cnt]], 0] = full[:cnt]
    X = CT.design(locs, 3, coords=True)
    pl = _plan(hip, topo, locs, y, R_CV, spec, X)
    got = _against_twin(pl, topo, locs, spec, y, R_CV, X, "g32 with leaves of 1, 16, 17", _tol())
    obs_p = np.isfinite(y.ravel())[topo.src] & (topo.perm >= 0)
    one = np.nonzero(obs_p[int(topo.node_row0[leaves[1]]):int(topo.node_row1[leaves[1]])])[0][0] + int(topo.node_row0[leaves[1]])
    for refit in (True, False):
        for k in range(3):                                                # a one-row group is the row's own leave-one-out
            a, b = got[(True, refit)][k][one], got[(False, refit)][k][one]
            assert abs(a - b) <= _tol() * max(1.0, abs(b))
    pl.close()


@pytest.mark.parametrize("p", [3, 17])
def test_leaves_of_nine_tiles(hip, p):
    topo, locs, y_obs, spec, R = GC._shape_tree("grid48_r20")            # leaves of 144 rows, 70 % observed: a multi-tile downdate
    X = CT.design(locs, p, coords=True)
    pl = _plan(hip, topo, locs, y_obs, R, spec, X)
    _against_twin(pl, topo, locs, spec, y_obs, R, X, "grid48_r20", _tol("grid48_r20"))
    pl.close()


def test_one_dimensional_tree(hip):
    import test_gpu_trend as GT
    cs = K.load_case("t201")
    topo, R = cs["topo"], float(cs["c"]["R"])
    X = GT._design(topo.N, 3)
    y = GT._with_trend(cs["y_obs"], X)
    pl = _plan(hip, topo, cs["locs"], y, R, cs["spec"], X)
    _against_twin(pl, topo, cs["locs"], cs["spec"], y, R, X, "t201", _tol())
    pl.close()


def test_chordal_tree_in_three_dimensions(hip):
    import test_gpu_sphere as SP
    ll, xyz, topo, y = SP.tree(*SP.TREES["g64"])
    X = CT.design(xyz, 5, coords=True)                                   # an intercept, x, y, z and one normal column
    pl = SP.make_plan(hip, topo, xyz, y.reshape(-1, 1), SP.M32)
    pl.run(True, True)
    pl.set_trend(X)
    _against_twin(pl, topo, xyz, SP.M32, y, SP.R, X, "sphere g64", _tol())
    pl.close()


def test_noise_vector(hip):
    import _noise as NZ
    cs = K.load_case("g32")
    topo, locs, spec, y_obs = cs["topo"], cs["locs"], cs["spec"], cs["y_obs"]
    X = CT.design(locs, 3)
    pl = _plan(hip, topo, locs, y_obs, R_CV, spec, X)
    scalar = {m: pl.cv_trend(*m) for m in MODES}
    pl.set_noise(np.full(topo.N, R_CV))
    pl.run(True, True)
    for m in MODES:                                                       # a constant vector is the scalar path, bit for bit
        for a, b in zip(pl.cv_trend(*m), scalar[m]):
            assert np.array_equal(a, b, equal_nan=True)
    rv = R_CV * np.random.default_rng(8).uniform(0.5, 2.0, topo.N)
    pl.set_noise(rv)
    pl.run(True, True)
    Sigma = NZ.prior_cov(topo, locs, spec, y_obs)
    ymax = np.nanmax(np.abs(np.asarray(y_obs, float)))
    tol = max(1e-9, 100.0 * CT.TWIN_ERR["g32_dense"])
    for leaf, refit in MODES:
        got = pl.cv_trend(leaf, refit)
        e = _errors(got, CT.dense_cv_trend(topo, Sigma, y_obs, rv, X, leaf, refit), ymax)
        print("g32 noise vector %s against the dense form with D = diag(r): mean %.2e, var %.2e, lpd %.2e, group lpd %.2e, sums %.2e, by-products %.2e, "
              "derivatives %.2e (leverage %.6f)" % (_name(leaf, refit), *e, got[4][5]))
        assert max(e) <= tol * max(1.0, (0.02 / (1.0 - got[4][5])) ** 2)
    pl.close()


# ---- 3. against refits on the device ----------------------------------------------------------------------------------------------------
def test_g32_against_refits_on_the_device(hip):
    """The 32 x 32 grid of g32 through MRATree(..., X=X), p = 3: every leaf in turn, then 12 single rows, set to NaN and the tree built
    again - its predict() at those rows is the refit's mean, sd^2 + R the variance of a new observation there.  Bounds as for the device
    refits of section 18 at c3: 1e-8 of max|y| for the mean, 1e-9 relative for the variance."""
    import pymra_amd.MRATools as mt
    from pymra_amd import MRATree
    cs = K.load_case("g32")
    c, locs = cs["c"], cs["locs"]
    y = np.asarray(cs["y_obs"], float).reshape(-1, 1)
    X = CT.design(locs, 3, coords=True)
    cov = lambda a, b=np.array([]): mt.ExpCovFun(a, b, l=c["l"])      # noqa: E731

    def build(yv):
        np.random.seed(5)                        # the tree's knot draws use the global RNG: the same seed gives the same tree
        return MRATree(locs, c["r"], cov, yv, R_CV, M=c["M"], J=c["J"], verbose=False, X=X)
    tree = build(y)
    t = tree.topology
    by_leaf, by_row = tree.crossValidate("leaf", trend="refit"), tree.crossValidate("loo", trend="refit")
    assert by_leaf.trend == by_row.trend == "refit" and by_leaf.n == by_row.n == int(np.isfinite(y).sum())
    ymax = np.nanmax(np.abs(y))
    obs = np.isfinite(y.ravel())

    def refit_at(idx):
        y2 = y.copy()
        y2[idx] = np.nan
        m, sd = build(y2).predict()
        return np.asarray(m).ravel()[idx], np.asarray(sd).ravel()[idx] ** 2 + R_CV
    e_m = e_v = 0.0
    leaves = _leaves(t)
    assert len(leaves) == 16
    for i in leaves:
        idx = t.perm[int(t.node_row0[i]):int(t.node_row1[i])]
        idx = idx[idx >= 0]
        idx = idx[obs[idx]]
        mu, S = refit_at(idx)
        e_m = max(e_m, np.abs(by_leaf.mean[idx] - mu).max() / ymax)
        e_v = max(e_v, (np.abs(by_leaf.sd[idx] ** 2 - S) / S).max())
    print("g32 p = 3 by leaf: 16 leaves against trees built again: mean %.2e, var %.2e (leverage %.6f)" % (e_m, e_v, by_leaf.leverage_max))
    assert e_m <= 1e-8 and e_v <= 1e-9
    e_m = e_v = 0.0
    for k in np.sort(np.random.default_rng(5).choice(np.nonzero(obs)[0], 12, replace=False)):
        mu, S = refit_at(np.array([k]))
        e_m = max(e_m, abs(by_row.mean[k] - mu[0]) / ymax)
        e_v = max(e_v, abs(by_row.sd[k] ** 2 - S[0]) / S[0])
    print("g32 p = 3 by row: 12 rows against trees built again: mean %.2e, var %.2e (leverage %.6f)" % (e_m, e_v, by_row.leverage_max))
    assert e_m <= 1e-8 and e_v <= 1e-9


# ---- 4. fixed mode and the derivatives --------------------------------------------------------------------------------------------------
def test_fixed_mode_is_mra_cv_on_the_detrended_data(hip):
    cs = K.load_case("g32")
    topo, locs, spec, y_obs = cs["topo"], cs["locs"], cs["spec"], cs["y_obs"]
    X = CT.design(locs, 3, coords=True)
    pl = _plan(hip, topo, locs, y_obs, R_CV, spec, X)
    beta = pl.trend_fit().beta
    trend = X @ beta
    fresh = GC._plan(hip, topo, locs, np.asarray(y_obs, float).reshape(-1, 1) - trend.reshape(-1, 1), R_CV, spec)
    rows = np.nonzero(np.isfinite(np.asarray(y_obs, float).ravel())[topo.src] & (topo.perm >= 0))[0]
    ymax = np.nanmax(np.abs(np.asarray(y_obs, float)))
    for leaf in (False, True):
        got, want = pl.cv_trend(leaf=leaf, refit=False), fresh.cv(leaf=leaf)
        gk = ~np.isnan(want[3])
        e = [np.abs(got[0][rows] - want[0][rows] - trend[topo.perm[rows]]).max() / ymax, (np.abs(got[1][rows] - want[1][rows]) / want[1][rows]).max(),
             _rel1(got[2][rows], want[2][rows]).max(), _rel1(got[3][gk], want[3][gk]).max(),
             max(_rel1(got[4][k], want[4][k]) for k in (2, 3, 4)), max(abs(got[4][k] - want[4][k]) / abs(want[4][k]) for k in (5, 6, 7))]
        print("g32 p = 3 %s: fixed mode against mra_cv on y - X beta^: mean %.2e, var %.2e, lpd %.2e, group lpd %.2e, sums %.2e, by-products %.2e"
              % ("by leaf" if leaf else "by row", *e))
        assert np.array_equal(np.isnan(got[3]), np.isnan(want[3])) and got[4][0] == want[4][0] and got[4][1] == want[4][1]
        assert max(e) <= 1e-10
    fresh.close(); pl.close()


def test_the_derivatives_are_those_of_the_profile_and_reml_values(hip):
    cs = K.load_case("g32")
    topo, locs, spec, y_obs = cs["topo"], cs["locs"], cs["spec"], cs["y_obs"]
    X = CT.design(locs, 3, coords=True)
    pl = _plan(hip, topo, locs, y_obs, R_CV, spec, X)
    info = pl.cv_trend()[4]
    pl.close()
    eps = 1e-6
    fits = []
    for R in (R_CV + eps, R_CV - eps):
        p2 = _plan(hip, topo, locs, y_obs, R, spec, X)
        fits.append(p2.trend_fit())
        p2.close()
    fd_prof, fd_reml = (fits[0].profile - fits[1].profile) / (2 * eps), (fits[0].reml - fits[1].reml) / (2 * eps)
    print("d profile / dR %.6f (central difference %.6f), d REML / dR %.6f (central difference %.6f)" % (info[10], fd_prof, info[11], fd_reml))
    assert abs(info[10] - fd_prof) <= 1e-5 * abs(fd_prof)                  # the bound tests/test_gpu_cv.py holds dlik_dR to
    assert abs(info[11] - fd_reml) <= 1e-5 * abs(fd_reml)


# ---- 5. the same bits, and the state the call leaves --------------------------------------------------------------------------------------
def test_same_bits_whatever_the_chunks_and_the_calls_before(hip):
    topo, locs, y_obs, spec, R = GC._shape_tree("grid48_r20")
    X = CT.design(locs, 5, coords=True)
    pl = _plan(hip, topo, locs, y_obs, R, spec, X)
    lik0, (m0, v0), y0 = pl.likelihood(), pl.predict(), pl.buffer(11)
    opts = {k: pl.get_option(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21)}
    cv0 = [pl.cv(leaf=leaf) for leaf in (False, True)]
    fit0 = pl.trend_fit(predict=True)
    first = {m: pl.cv_trend(*m) for m in MODES}

    def unchanged(tag):
        assert pl.likelihood() == lik0, tag
        m1, v1 = pl.predict()
        assert np.array_equal(m1, m0) and np.array_equal(v1, v0), tag
        assert np.array_equal(pl.buffer(11), y0, equal_nan=True), tag
        assert {k: pl.get_option(k) for k in opts} == opts, tag
    unchanged("after the first calls")

    def same(tag):
        for m in MODES:
            got = pl.cv_trend(*m)
            assert GC._factor_launches(pl) == 0, tag              # no kernel of a pass
            for a, b in zip(got, first[m]):
                assert np.array_equal(a, b, equal_nan=True), (tag, m)
    same("a second call")
    pl.set_option(21, 1)                                          # one leaf per batch
    same("one leaf per batch")
    pl.set_option(21, 0)
    Yp = np.zeros((2, topo.P))
    pl.solve(Yp)
    same("after solve")
    pl.cov_apply(Yp, posterior=True)
    same("after cov_apply")
    rows = np.nonzero(SM.reported(topo))[0][:40]
    L = np.asarray(locs, float).reshape(topo.N, -1)
    pl.predict_sites(L[topo.perm[rows]], CV.leaf_of_rows(topo)[rows])
    same("after predict_sites")
    unchanged("after every call")
    # mra_cv and mra_trend_fit give what they gave before
    for leaf in (False, True):
        for a, b in zip(pl.cv(leaf=leaf), cv0[leaf]):
            assert np.array_equal(a, b, equal_nan=True)
    fit1 = pl.trend_fit(predict=True)
    for a, b in zip(fit1, fit0):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    same("after mra_cv and mra_trend_fit")
    pl.set_option(1, 1)                                           # MRA_OPT_KERNEL_TIMING
    pl.cv_trend(leaf=True, refit=True)
    ms = pl.buffer(15)
    assert ms.shape == (12,) and np.all(ms >= 0.0) and ms[4] > 0.0 and ms[5] > 0.0 and ms[9] > 0.0 and ms[10] > 0.0 and ms[11] > 0.0
    pl.cv_trend(leaf=False, refit=True)
    assert pl.buffer(15)[11] == 0.0 and pl.buffer(15)[10] > 0.0   # by row nothing is downdated
    pl.close()


def test_the_first_call_runs_its_own_pass_and_no_predict_pass(hip):
    cs = K.load_case("g32")
    X = CT.design(cs["locs"], 3)
    pl = _plan(hip, cs["topo"], cs["locs"], cs["y_obs"], R_CV, cs["spec"], X, run=False)
    a = pl.cv_trend()
    n_first = GC._factor_launches(pl)
    assert n_first > 0
    b = pl.cv_trend()
    assert GC._factor_launches(pl) == 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    pl.close()
    pl = GC._plan(hip, cs["topo"], cs["locs"], cs["y_obs"], R_CV, cs["spec"], run=False)
    pl.cv()                                                       # mra_cv's first call: one likelihood pass - mra_cv_trend's ran no more
    assert GC._factor_launches(pl) == n_first
    pl.close()


def test_after_fit_laplace_trend_the_pseudo_observations_are_scored(hip):
    import _laplace as LP
    import _laplace_trend as LT
    import test_gpu_likelihood_masks as MK
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, X, ref = LT.t16_fit(LP.POISSON, 3)
    pl = MK._plan(hip, topo, locs, y)
    pl.set_trend(X)
    pl.fit_laplace_trend(LP.NAMES[LP.POISSON], z, aux=aux, offset=offset, tol=1e-10)
    got = {m: pl.cv_trend(*m) for m in MODES}
    t, r = pl.buffer(11), pl.buffer(10)
    rows = (topo.perm >= 0) & np.asarray(topo.in_leaf, dtype=bool)
    tc, rc = np.full(topo.N, np.nan), np.full(topo.N, 1.0)
    tc[topo.perm[rows]], rc[topo.perm[rows]] = t[rows], r[rows]
    rc[~np.isfinite(tc)] = 1.0
    s = MK._spec()
    fresh = hip.HipPlan(topo, 0)
    fresh.set_locs(locs); fresh.set_obs(tc.reshape(-1, 1), rc); fresh.set_kernel(s.kind, s.l, s.sig, s.scale)
    fresh.set_trend(X)
    for m in MODES:
        want = fresh.cv_trend(*m)
        assert want[4][0] > 0 and want[4][9] == 3
        for a, b in zip(got[m], want):
            assert np.array_equal(a, b, equal_nan=True)
    fresh.close(); pl.close()


# ---- 6. refusals and the tree's surface ---------------------------------------------------------------------------------------------------
def test_refusals(hip):
    from pymra_amd.plan import MraError
    cs = K.load_case("g32")
    topo, locs, spec, y_obs = cs["topo"], cs["locs"], cs["spec"], cs["y_obs"]
    X = CT.design(locs, 3)
    pl = hip.HipPlan(topo, 0)
    pl.lib.mra_last_error.restype = C.c_char_p
    for step in ("nothing", "locs", "kernel"):
        if step == "locs":
            pl.set_locs(locs)
        elif step == "kernel":
            pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
        with pytest.raises(MraError) as e:
            pl.cv_trend()
        assert e.value.code == -4 and "mra_cv_trend needs" in str(e.value), step      # MRA_ERR_STATE before set_locs / set_kernel / set_obs
    pl.set_obs(y_obs, R_CV)
    for m in MODES:
        with pytest.raises(MraError) as e:
            pl.cv_trend(*m)
        assert e.value.code == -4 and "mra_cv_trend needs mra_plan_set_trend first" in str(e.value)
    pl.set_trend(X)
    good = pl.cv_trend(leaf=True)
    info = np.zeros(12)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def raw(flags=0, inf=info, fn="mra_cv_trend"):
        return getattr(pl.lib, fn)(pl._h, flags, None, None, None, None, p(inf))

    def message():
        return pl.lib.mra_last_error(pl._h).decode()
    for flags in (0, 1, 2, 3):                                             # every output but info may be NULL
        assert raw(flags) == 0 and info[0] == good[4][0] and info[9] == 3
    assert np.array_equal(info, good[4])                                   # flags 3: by leaf, beta estimated again
    assert raw(4) == -1 and "unknown mra_cv_trend flags" in message()
    assert raw(inf=None) == -1 and "mra_cv_trend: info is NULL" in message()
    assert raw(2, fn="mra_cv") == -1 and "unknown mra_cv flags" in message()      # mra_cv is as it was
    assert raw(1, fn="mra_cv") == 0
    rv = np.full(topo.N, R_CV)                                             # a vector may hold a 0: one observed row is enough
    rv[np.nonzero(np.isfinite(np.asarray(y_obs, float).ravel()))[0][5]] = 0.0
    pl.set_noise(rv)
    for flags in (0, 1, 2, 3):
        assert raw(flags) == -1 and "mra_cv_trend: the noise variance is 0 at observed padded row" in message()
    pl.set_noise(None)
    Xd = X.copy()
    Xd[:, 2] = 2.0 * Xd[:, 0]                                              # dependent columns: the trend fit's own refusal
    pl.set_trend(Xd)
    with pytest.raises(MraError) as e:
        pl.cv_trend()
    assert e.value.code == -3 and "mra_cv_trend: trend columns are linearly dependent at the observed rows" in str(e.value)
    pl.set_trend(X)
    pl.set_obs(np.full((topo.N, 1), np.nan), R_CV)                         # no observed row: MRA_OK, info all zero but p
    none = pl.cv_trend()
    assert np.all(np.isnan(none[0])) and np.all(np.isnan(none[3])) and none[4][9] == 3 and np.all(np.delete(none[4], 9) == 0.0)
    pl.set_obs(y_obs, R_CV)
    again = pl.cv_trend(leaf=True)                                         # the plan is still usable, and gives the same bits
    for a, b in zip(again, good):
        assert np.array_equal(a, b, equal_nan=True)
    pl.set_reduce_level(0)
    with pytest.raises(MraError) as e:
        pl.cv_trend()
    assert e.value.code == -1 and "sharded" in str(e.value)
    pl.close()


def test_a_leaf_above_the_cap_is_refused_by_leaf_only(hip):
    import pymra_amd.MRATools as mt
    from pymra_amd.plan import MraError
    from pymra_amd.topology import build_topology
    locs = mt.genLocations2d(Nx=72, Ny=72)                                 # one leaf of 5184 rows, all observed: above the cap of 4096
    topo = build_topology(locs, 16, 0, 4)
    y = np.random.default_rng(1).standard_normal((len(locs), 1))
    pl = _plan(hip, topo, locs, y, 0.5, mt.KernelSpec(mt.KIND_EXP, 0.05), CT.design(locs, 2), run=False)
    for refit in (True, False):
        with pytest.raises(MraError) as e:
            pl.cv_trend(leaf=True, refit=refit)
        assert e.value.code == -1 and "mra_cv_trend: leaf" in str(e.value) and "MRA_SAMPLE_SITES_LEAF_MAX" in str(e.value)
    pl.close()


def test_mratree_crossValidate_with_a_trend(hip):
    import test_gpu_trend as GT
    locs, X, y_obs = GT._tree_inputs(n=32)
    tree, _ = GT._tree(locs, y_obs, 0.2, X=X)
    prof0, reml0 = float(tree.getLikelihood()[0, 0]), float(tree.getLikelihood(reml=True)[0, 0])
    m0, sd0 = tree.predict()
    t = tree.topology
    S = TS.SiteState(t, locs, tree.kernel, y_obs, 1e-2)
    fit = TT.tree_trend(t, locs, tree.kernel, y_obs, 1e-2, X)
    rows = t.perm >= 0
    N = len(locs)
    with pytest.raises(NotImplementedError) as e:
        tree.crossValidate()                                               # trend=None on a tree with a trend: as before
    assert "trend" in str(e.value) and '"refit"' in str(e.value) and '"fixed"' in str(e.value)
    with pytest.raises(ValueError):
        tree.crossValidate("loo", trend="both")
    with pytest.raises(ValueError):
        tree.crossValidate("kfold", trend="refit")
    for kind in ("loo", "leaf"):
        for mode in ("refit", "fixed"):
            res = tree.crossValidate(kind, trend=mode)
            want = CT.tree_cv_trend(S, X, kind == "leaf", mode == "refit", fit=fit)
            assert res.trend == mode and res.kind == kind
            assert res.mean.shape == res.sd.shape == res.z.shape == res.lpd.shape == (N,)
            assert np.array_equal(np.isnan(res.mean), np.isnan(y_obs.ravel()))       # NaN exactly where nothing is observed
            for got, w in ((res.mean, want[0]), (res.sd ** 2, want[1]), (res.lpd, want[2])):
                wc = np.full(N, np.nan)
                wc[t.perm[rows]] = w[rows]                                         # the caller's row order
                ok = ~np.isnan(wc)
                assert np.array_equal(ok, ~np.isnan(got))
                assert (np.abs(got[ok] - wc[ok]) / np.maximum(1.0, np.abs(wc[ok]))).max() <= _tol()
            ok = ~np.isnan(res.z)
            assert np.abs(res.z[ok] - (y_obs.ravel()[ok] - res.mean[ok]) / res.sd[ok]).max() <= 1e-12 * np.abs(res.z[ok]).max()
            assert sorted(res.leaf_lpd) == [int(i) for i in np.nonzero(~np.isnan(want[3]))[0]]
            assert res.n == int(np.isfinite(y_obs).sum())
            scale = max(abs(want[4][6]), abs(want[4][7]))
            print("crossValidate(%s, trend=%s): score %.6f (twin %.6f), dlik_dR %.6f (twin %.6f), dlik_dR_reml %.6f (twin %.6f), leverage %.4f (twin %.4f)"
                  % (kind, mode, res.score, want[4][2], res.dlik_dR, want[4][10], res.dlik_dR_reml, want[4][11], res.leverage_max, want[4][5]))
            assert abs(res.score - want[4][2]) <= _tol() * max(1.0, abs(want[4][2]))
            assert abs(res.dlik_dR - want[4][10]) <= _tol() * scale and abs(res.dlik_dR_reml - want[4][11]) <= _tol() * scale
            assert abs(res.leverage_max - want[4][5]) <= _tol()
    assert float(tree.getLikelihood()[0, 0]) == prof0 and float(tree.getLikelihood(reml=True)[0, 0]) == reml0
    m1, sd1 = tree.predict()
    assert np.array_equal(np.asarray(m1), np.asarray(m0)) and np.array_equal(sd1, sd0)
    plain, _ = GT._tree(locs, y_obs, 0.2)
    for mode in ("refit", "fixed", "both"):
        with pytest.raises(ValueError):
            plain.crossValidate(trend=mode)                                # a tree without a trend takes None only
    res = plain.crossValidate()
    assert res.trend is None and res.dlik_dR_reml is None
