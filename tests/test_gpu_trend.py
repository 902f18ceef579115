"""The regression trend on the GPU: MRA_SOLVE_FULL_QUAD, mra_plan_set_trend / mra_trend_fit, MRATree(..., X=X).
Truths: the flagless mra_solve (same-block entries bit for bit; a cross-block entry against the same entry with both columns in one
block), dense conditioning on the faithful oracle's covariance, the NumPy twin tests/_treetrend.py, and the plan's own pass on the
detrended data.  The tree is the gappy 64 x 64, r = 16, M = 3 tree of test_gpu_solve: an empty leaf, an empty family, observation
counts that are no multiple of 4 or 16.  Tolerances are cited where they are used."""
import ctypes as C
import functools

import numpy as np
import pytest

import _cases as K
import _noise as NZ
import _sampling as SM
import _treetrend as TT
from test_gpu_solve import R_MASK, _caller, _columns, _gappy_tree, _padded, _plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _spec():
    import pymra_amd.MRATools as mt
    return mt.KernelSpec(mt.KIND_MATERN32, 0.25, 1.2)


@functools.lru_cache(maxsize=None)
def _gappy():
    return _gappy_tree()


def _design(N, p, seed=3):
    """An intercept and p - 1 standard normal columns; the data get a mean the zero-mean model would miss."""
    X = np.random.default_rng(seed).standard_normal((N, p))
    X[:, 0] = 1.0
    return X


def _with_trend(y_obs, X):
    return np.asarray(y_obs, float).ravel() + X @ np.linspace(1.0, 2.0, X.shape[1])


@functools.lru_cache(maxsize=None)
def _twin(p):
    topo, locs, y_obs = _gappy()
    X = _design(topo.N, p)
    return TT.tree_trend(topo, locs, _spec(), _with_trend(y_obs, X), R_MASK, X)


def _factor_launches(pl):
    return sum(s["launches"] for s in pl.kernel_stats())


# ---- 1. the full quadratic form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [5, 16, 17, 40, 64])
def test_full_quad_fills_the_cross_blocks_and_keeps_the_rest(hip, c):
    topo, locs, y_obs = _gappy()
    pl = _plan(hip, topo, locs, y_obs, R_MASK, _spec())
    Yp = _padded(topo, _columns(y_obs, c, seed=c))
    quad0 = pl.solve(Yp, want_mean=False)[1]
    quad = pl.solve(Yp, want_mean=False, full_quad=True)[1]
    blk = np.arange(c) // 16
    same = blk[:, None] == blk[None, :]
    assert np.array_equal(quad[same], quad0[same])                       # bit for bit what the flagless call computes
    assert not np.any(np.isnan(quad))
    assert np.array_equal(quad, quad.T)
    assert np.array_equal(pl.solve(Yp, want_mean=False, full_quad=True)[1], quad)
    mq, _ = pl.solve(Yp, want_quad=False, full_quad=True)                # the flag without quad is a plain solve
    assert np.array_equal(mq, pl.solve(Yp, want_quad=False)[0])
    # every cross-block entry against the flagless call on a column set that puts its two columns into one block: for the block
    # pair (a, b) the four sets of eight columns of a with eight of b, all sets in one call (its quad is block-diagonal by set)
    sets = []
    for a in range(blk.max() + 1):
        for b in range(a + 1, blk.max() + 1):
            ca, cb = np.nonzero(blk == a)[0], np.nonzero(blk == b)[0]
            for ha in (ca[:8], ca[8:]):
                for hb in (cb[:8], cb[8:]):
                    if len(ha) and len(hb):
                        sets.append(np.concatenate([ha, hb, np.full(16 - len(ha) - len(hb), ha[0])]))
    if sets:
        cols = np.concatenate(sets)
        ref = pl.solve(np.ascontiguousarray(Yp[cols]), want_mean=False)[1]
        bound = 1e-12 * np.abs(np.diag(quad)).max()                      # test_gpu_solve's bound for quad between option paths
        worst, seen = 0.0, np.zeros((c, c), bool)
        for k, st in enumerate(sets):
            sub = ref[16 * k:16 * k + 16, 16 * k:16 * k + 16]
            cross = blk[st][:, None] != blk[st][None, :]
            err = np.abs(sub - quad[np.ix_(st, st)])[cross]
            worst = max(worst, err.max())
            seen[np.ix_(st, st)] |= cross
        print("c = %d: %d sets, worst cross-block difference %.2e (bound %.2e)" % (c, len(sets), worst, bound))
        assert np.array_equal(seen, ~same)                               # every cross-block entry was compared
        assert worst <= bound
    pl.close()


@pytest.mark.parametrize("name", ["g32", "c1", "kat3"])
def test_full_quad_matches_dense_conditioning(hip, name):
    from oracle.mra_faithful import prior_sigma_rows
    cs = K.load_case(name)
    topo, R = cs["topo"], cs["c"]["R"]
    pl = _plan(hip, topo, cs["locs"], cs["y_obs"], R, cs["spec"])
    Y = _columns(cs["y_obs"], 40)
    quad = pl.solve(_padded(topo, Y), want_mean=False, full_quad=True)[1]
    rows = np.nonzero(SM.reported(topo))[0]
    S = prior_sigma_rows(topo, cs["locs"], cs["spec"].evaluate, rows)
    o = np.isfinite(np.asarray(cs["y_obs"], float).ravel())[topo.perm[rows]]
    L = np.linalg.cholesky(S[np.ix_(o, o)] + R * np.eye(int(o.sum())))
    A = np.linalg.solve(L, Y[topo.perm[rows]][o])
    want = A.T @ A
    e_q = np.abs(quad - want).max()
    print("%s: quad err %.2e, quad scale %.1f" % (name, e_q, np.abs(np.diag(want)).max()))
    assert e_q <= 1e-9 * np.abs(np.diag(want)).max()                     # test_solve_matches_dense_conditioning
    pl.close()


def test_full_quad_refuses_more_than_256_columns(hip):
    topo, locs, y_obs = _gappy()
    pl = _plan(hip, topo, locs, y_obs, R_MASK, _spec(), run=False)
    with pytest.raises(hip.MraError) as e:
        pl.solve(np.zeros((257, topo.P)), want_mean=False, full_quad=True)
    assert e.value.code == -1 and "mra_solve: MRA_SOLVE_FULL_QUAD" in str(e.value)
    assert _factor_launches(pl) == 0                                     # refused before anything was launched
    assert pl.solve(np.zeros((257, topo.P)), want_mean=False)[1].shape == (257, 257)      # the flagless call has no such limit
    pl.close()


# ---- 2. / 3. the fit --------------------------------------------------------------------------------------------------------------------
def _check_fit(hip, topo, locs, spec, y, R, X, tw, noise=None):
    """One predicting fit against the twin `tw` and against the plan's own pass on the detrended data."""
    p = X.shape[1]
    pl = _plan(hip, topo, locs, y, R, spec, run=False)
    if noise is not None:
        pl.set_noise(noise)
    pl.set_trend(X)
    fit = pl.trend_fit(predict=True)
    assert fit.beta.shape == (p,) and fit.cov_beta.shape == (p, p) and fit.mean.shape == (topo.N,)
    # G, through the full quad of the same columns, against the twin: the bound of test_solve_matches_dense_conditioning for quad
    G = pl.solve(_padded(topo, np.column_stack([np.nan_to_num(y), X])), want_mean=False, full_quad=True)[1]
    gs = np.abs(np.diag(tw["G"])).max()
    e_g = np.abs(G - tw["G"]).max()
    # beta and cov(beta) inherit G's relative error times the condition number of A = X^T K^-1 X
    A = tw["G"][1:, 1:]
    cond = np.linalg.cond(A)
    e_b = np.abs(fit.beta - tw["beta"]).max()
    e_c = np.abs(fit.cov_beta - tw["cov_beta"]).max()
    print("p = %d: G err %.2e (scale %.1f), cond(A) %.1f, beta err %.2e, cov err %.2e" % (p, e_g, gs, cond, e_b, e_c))
    assert e_g <= 1e-9 * gs
    assert e_b <= 1e-9 * cond * max(1.0, np.abs(tw["beta"]).max())
    assert e_c <= 1e-9 * cond * np.abs(tw["cov_beta"]).max()
    assert np.array_equal(fit.cov_beta, fit.cov_beta.T) or np.abs(fit.cov_beta - fit.cov_beta.T).max() <= 1e-15 * np.abs(fit.cov_beta).max()
    assert abs(fit.profile - (fit.d + fit.u)) <= 1e-12 * abs(fit.profile)
    assert abs((fit.reml - fit.profile) - tw["logdetA"]) <= 1e-9 * cond * p      # p pivots, each within cond * 1e-9 relative
    obs = np.isfinite(y) & NZ.reported(topo)
    assert fit.n_obs == int(obs.sum())
    # the plan's own pass on y - X beta: d + u is the profile value, its mean + X beta the universal-kriging mean
    own = _plan(hip, topo, locs, np.where(np.isfinite(y), y - X @ fit.beta, np.nan), R, spec, run=False)
    if noise is not None:
        own.set_noise(noise)
    own.run(True, True)
    d, u = own.likelihood()
    m, v = own.predict()
    rep = NZ.reported(topo)
    want_mean = np.where(rep, m + X @ fit.beta, 0.0)
    scale = max(1.0, np.abs(want_mean).max())
    e_l = abs(fit.profile - (d + u)) / abs(d + u)
    e_m = np.abs(fit.mean - want_mean).max()
    prior_var = float(np.asarray(spec.evaluate(np.asarray(locs)[:1], np.asarray(locs)[:1])).ravel()[0])
    e_v = np.abs((fit.var - v) - tw["add"]).max()
    print("p = %d: profile rel err %.2e, mean err %.2e (scale %.2f), var term err %.2e (prior variance %.2f)" % (p, e_l, e_m, scale, e_v, prior_var))
    assert e_l <= 1e-9                                                   # _check_against_own_pass
    assert e_m <= 1e-8 * scale                                           # _check_against_own_pass
    assert e_v <= 1e-9 * prior_var
    assert np.all(fit.var >= v)
    assert np.all(fit.mean[~rep] == 0.0) and np.all(fit.var[~rep] == 0.0)
    own.close()
    pl.close()


@pytest.mark.parametrize("p", [1, 3, 15, 16, 40, 63])
def test_fit_matches_the_twin_and_the_plans_own_pass(hip, p):
    topo, locs, y_obs = _gappy()
    X = _design(topo.N, p)
    _check_fit(hip, topo, locs, _spec(), _with_trend(y_obs, X), R_MASK, X, _twin(p))


def test_fit_with_a_noise_vector(hip):
    topo, locs, y_obs = _gappy()
    X = _design(topo.N, 3)
    y = _with_trend(y_obs, X)
    tw = TT.tree_trend(topo, locs, _spec(), y, R_MASK, X, scaled_noise=True)
    _check_fit(hip, topo, locs, _spec(), y, R_MASK, X, tw, noise=NZ.noise_of(locs, R_MASK))


def test_fit_on_a_one_dimensional_tree(hip):
    cs = K.load_case("t201")
    topo, R = cs["topo"], float(cs["c"]["R"])
    X = _design(topo.N, 3)
    y = _with_trend(cs["y_obs"], X)
    _check_fit(hip, topo, cs["locs"], cs["spec"], y, R, X, TT.tree_trend(topo, cs["locs"], cs["spec"], y, R, X))


# ---- 4. state ---------------------------------------------------------------------------------------------------------------------------
def test_fit_leaves_the_callers_state_and_keeps_the_factors(hip):
    topo, locs, y_obs = _gappy()
    spec = _spec()
    X = _design(topo.N, 3)
    y = _with_trend(y_obs, X)
    pl = _plan(hip, topo, locs, y, R_MASK, spec, run=False)
    pl.run(True, False)                                                  # a likelihood-only pass: the call runs its own predict pass
    opts = {k: pl.get_option(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20)}
    lik0, y0 = pl.likelihood(), pl.buffer(11)
    pl.set_trend(X)
    f1 = pl.trend_fit(predict=True)
    assert _factor_launches(pl) > 0
    assert pl.likelihood() == lik0 and np.array_equal(pl.buffer(11), y0, equal_nan=True)
    assert {k: pl.get_option(k) for k in opts} == opts
    with pytest.raises(hip.MraError) as e:                               # still no predictions of the caller's: nothing was invented
        pl.predict()
    assert e.value.code == -4
    f2 = pl.trend_fit(predict=True)
    assert _factor_launches(pl) == 0                                     # no pass, neither for the factors nor for the variance
    assert np.array_equal(f1.beta, f2.beta) and np.array_equal(f1.mean, f2.mean) and np.array_equal(f1.var, f2.var) and f1.profile == f2.profile
    f3 = pl.trend_fit()
    assert _factor_launches(pl) == 0 and f3.mean is None and np.array_equal(f3.beta, f1.beta) and f3.reml == f1.reml
    pl.run(True, True)
    lik1, (m1, v1) = pl.likelihood(), pl.predict()
    assert lik1 == lik0
    f4 = pl.trend_fit(predict=True)                                      # mra_run dropped the factors: they are made again
    assert _factor_launches(pl) > 0
    assert pl.likelihood() == lik1 and np.array_equal(pl.predict()[0], m1) and np.array_equal(pl.predict()[1], v1)
    assert np.abs(f4.beta - f1.beta).max() <= 1e-12 * np.abs(f1.beta).max()
    assert np.abs(f4.var - f1.var).max() <= 1e-12 * max(1.0, f1.var.max())
    # new observations, then a new kernel: X stays, the fit follows the new state (a fresh plan is the reference)
    import pymra_amd.MRATools as mt
    y2 = np.where(np.isfinite(y), y + np.random.default_rng(9).standard_normal(len(y)), np.nan)
    spec2 = mt.KernelSpec(mt.KIND_MATERN32, 0.15, 1.0)
    for step in ("set_obs", "set_kernel"):
        if step == "set_obs":
            pl.set_obs(y2, R_MASK)
        else:
            pl.set_kernel(spec2.kind, spec2.l, spec2.sig, spec2.scale)
        assert pl.info()["trend_p"] == 3
        got = pl.trend_fit(predict=True)
        fresh = _plan(hip, topo, locs, y2, R_MASK, spec if step == "set_obs" else spec2, run=False)
        fresh.set_trend(X)
        want = fresh.trend_fit(predict=True)
        fresh.close()
        assert np.abs(got.beta - f1.beta).max() > 1e-6, step             # it did change
        assert np.abs(got.beta - want.beta).max() <= 1e-12 * np.abs(want.beta).max(), step
        assert abs(got.profile - want.profile) <= 1e-12 * abs(want.profile), step
        assert np.abs(got.mean - want.mean).max() <= 1e-12 * max(1.0, np.abs(want.mean).max()), step
        assert np.abs(got.var - want.var).max() <= 1e-12 * max(1.0, want.var.max()), step
    pl.set_trend(None)
    assert pl.info()["trend_p"] == 0
    pl.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def _raw_fit(pl, flags, p, beta=True, info=True, mean=False):
    b, i, m = np.zeros(max(p, 1)), np.zeros(8), np.zeros(pl.topo.P)
    rc = pl.lib.mra_trend_fit(pl._h, C.c_uint32(flags), hip_ptr(b) if beta else None, None, hip_ptr(m) if mean else None, None,
                              hip_ptr(i) if info else None)
    return rc, pl.lib.mra_last_error(pl._h).decode()


def hip_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_fit_refusals(hip):
    topo, locs, y_obs = _gappy()
    spec = _spec()
    y = np.asarray(y_obs, float).ravel()
    pl = _plan(hip, topo, locs, y_obs, R_MASK, spec, run=False)
    rc, msg = _raw_fit(pl, 0, 1)
    assert rc == -4 and msg.startswith("mra_trend_fit needs mra_plan_set_trend")          # no trend
    rc, msg = _raw_fit(pl, 1 << 7, 1)
    assert rc == -1 and msg == "unknown mra_trend_fit flags"                               # the preamble comes before the trend
    X = _design(topo.N, 3)
    pl.set_trend(X)
    for kw, what in ((dict(beta=False), "beta"), (dict(info=False), "info"), (dict(mean=True), "without MRA_TREND_PREDICT")):
        rc, msg = _raw_fit(pl, 0, 3, **kw)
        assert rc == -1 and msg.startswith("mra_trend_fit:") and what in msg, (kw, msg)
    # linearly dependent columns: finite inputs, a host check of a 3 x 3 matrix.  The first column is ten times as large, so the
    # floor 3 * 2^-52 * max diag(A) is far above the rounding of the pivot that two identical columns leave.
    z = np.random.default_rng(1).standard_normal(topo.N)
    for Xbad, what in ((np.column_stack([10.0 * X[:, 1], z, z]), "identical columns"),
                       (np.column_stack([10.0 * X[:, 1], z, np.where(np.isfinite(y), 0.0, 1.0)]), "a column that is 0 at every observed row")):
        pl.set_trend(Xbad)
        with pytest.raises(hip.MraError) as e:
            pl.trend_fit()
        assert e.value.code == -3 and "mra_trend_fit: trend columns are linearly dependent at the observed rows" in str(e.value), what
    pl.set_trend(X)
    assert pl.trend_fit().beta.shape == (3,)                             # the plan is whole
    pl.set_reduce_level(0)
    rc, msg = _raw_fit(pl, 0, 3)
    assert rc == -1 and msg == "mra_trend_fit: sharded plans cannot fit a trend"
    rc, msg = _raw_fit(pl, 1 << 7, 3)
    assert rc == -1 and msg == "unknown mra_trend_fit flags"                               # flags before sharding
    pl.close()
    # an MRA_KERNEL_HOST plan (opaque callable): refused as such before the missing trend is
    import pymra_amd.MRATools as mt
    from pymra_amd import MRATree
    np.random.seed(1)
    n = 16
    l2 = mt.genLocations2d(Nx=n, Ny=n)
    yh = np.random.normal(size=(n * n, 1))
    cov = lambda a, b=np.array([]): np.exp(-np.abs(mt.dist(a, b)) / 0.3)                  # noqa: E731
    tree = MRATree(l2, 16, cov, yh, 1e-2, M=1, J=4, verbose=False)
    rc, msg = _raw_fit(tree.plan, 0, 1)
    assert rc == -1 and msg.startswith("mra_trend_fit: MRA_KERNEL_HOST plans cannot fit a trend")
    with pytest.raises(NotImplementedError):
        tree.setTrend(np.ones((n * n, 1)))
    with pytest.raises(NotImplementedError):
        MRATree(l2, 16, cov, yh, 1e-2, M=1, J=4, verbose=False, X=np.ones((n * n, 1)))


# ---- 6. MRATree ---------------------------------------------------------------------------------------------------------------------------
def _tree_inputs(n=48, seed=4):
    import pymra_amd.MRATools as mt
    np.random.seed(seed)
    locs = mt.genLocations2d(Nx=n, Ny=n)
    N = n * n
    X = np.column_stack([np.ones(N), locs[:, 0], locs[:, 1]])
    rng = np.random.default_rng(seed)
    w = rng.normal(size=(32, 2)) / 0.2
    field = np.sqrt(2.0 / 32) * np.cos(locs @ w.T + rng.uniform(0, 2 * np.pi, 32)).sum(axis=1)
    y = X @ np.array([2.0, -1.5, 0.75]) + field + 0.1 * rng.normal(size=N)
    y_obs = np.where(rng.random(N) < 0.4, y, np.nan).reshape(-1, 1)
    return locs, X, y_obs


def _tree(locs, y_obs, l, X=None, seed=5):
    import pymra_amd.MRATools as mt
    from pymra_amd import MRATree
    np.random.seed(seed)                      # the tree's knot draws use the global RNG: the same seed gives the same tree
    cov = lambda a, b=np.array([]): mt.Matern32(a, b, l=l, sig=1.0)                       # noqa: E731
    return MRATree(locs, 16, cov, y_obs, 1e-2, M=2, J=4, verbose=False, X=X), cov


def test_mratree_with_a_trend(hip):
    import pymra_amd.MRATools as mt
    locs, X, y_obs = _tree_inputs()
    plain, _ = _tree(locs, y_obs, 0.2)
    lik_plain, (m_plain, sd_plain) = plain.getLikelihood(), plain.predict()
    assert plain.trend is None
    with pytest.raises(ValueError):
        plain.getLikelihood(reml=True)
    # the computation of examples/gls_trend.py on the tree without a trend
    mean, quad = plain.solve(np.column_stack([np.nan_to_num(y_obs.ravel()), X]))
    cov_beta = np.linalg.inv(quad[1:, 1:])
    beta_hat = cov_beta @ quad[1:, 0]
    assert float(plain.getLikelihood()[0, 0]) == float(lik_plain[0, 0])                  # ... which leaves the tree as it was
    assert np.array_equal(np.asarray(plain.predict()[0]), np.asarray(m_plain)) and np.array_equal(plain.predict()[1], sd_plain)
    tree, _ = _tree(locs, y_obs, 0.2, X=X)
    fit = tree.trend
    print("beta", fit.beta, "gls_trend", beta_hat)
    assert np.abs(fit.beta - beta_hat).max() <= 1e-9 * np.abs(beta_hat).max()
    assert np.abs(fit.cov_beta - cov_beta).max() <= 1e-9 * np.abs(cov_beta).max()
    prof = float(tree.getLikelihood()[0, 0])
    assert prof == fit.profile and float(tree.getLikelihood(reml=True)[0, 0]) == fit.reml
    assert abs(prof - (float(plain.root.d[0, 0]) + quad[0, 0] - quad[1:, 0] @ beta_hat)) <= 1e-9 * abs(prof)
    m, sd = tree.predict()
    m = np.asarray(m).ravel()
    field_hat = mean[:, 0] - mean[:, 1:] @ beta_hat
    scale = max(1.0, np.abs(m).max())
    assert np.abs(m - (X @ beta_hat + field_hat)).max() <= 1e-8 * scale
    assert np.all(sd >= sd_plain)
    # predictAt at tree locations reproduces predict()
    rows = np.random.default_rng(2).choice(len(locs), 50, replace=False)
    with pytest.raises(ValueError):
        tree.predictAt(locs[rows])
    ma, sda = tree.predictAt(locs[rows], X_sites=X[rows])
    print("predictAt: mean err %.2e, sd err %.2e" % (np.abs(ma[:, 0] - m[rows]).max(), np.abs(sda - sd[rows]).max()))
    assert ma.shape == (50, 1) and np.abs(ma[:, 0] - m[rows]).max() <= 1e-8 * scale
    assert np.abs(sda - sd[rows]).max() <= 1e-8 * max(1.0, sd.max())
    assert float(tree.getLikelihood()[0, 0]) == prof and np.array_equal(np.asarray(tree.predict()[0]).ravel(), m)
    # another length scale on the same tree: beta and the profile value move, and match a fresh tree
    cov2 = lambda a, b=np.array([]): mt.Matern32(a, b, l=0.35, sig=1.0)                  # noqa: E731
    prof2 = float(tree.reevaluate(cov2)[0, 0])
    fresh, _ = _tree(locs, y_obs, 0.35, X=X)
    assert np.abs(tree.trend.beta - fit.beta).max() > 1e-6 and abs(prof2 - prof) > 1e-6
    assert np.abs(tree.trend.beta - fresh.trend.beta).max() <= 1e-9 * np.abs(fresh.trend.beta).max()
    assert abs(prof2 - fresh.trend.profile) <= 1e-9 * abs(prof2)
    # what is out of scope says so
    for call in (lambda: tree.simulate(1), lambda: tree.simulateAt(locs[rows], 1), lambda: tree.sampleAt(locs[rows], 1),
                 lambda: tree.crossValidate(), lambda: tree.fitLaplace("gaussian", aux=1.0)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert "trend" in str(e.value)
    # clearing the trend gives the plain tree back
    tree.reevaluate(lambda a, b=np.array([]): mt.Matern32(a, b, l=0.2, sig=1.0))
    back = float(tree.setTrend(None)[0, 0])
    assert tree.trend is None and abs(back - float(lik_plain[0, 0])) <= 1e-12 * abs(back)
    assert np.abs(np.asarray(tree.predict()[0]).ravel() - np.asarray(m_plain).ravel()).max() <= 1e-12 * scale
