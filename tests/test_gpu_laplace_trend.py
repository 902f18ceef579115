"""mra_plan_fit_laplace_trend on the GPU: Poisson and binomial data with a regression trend, on T16 of
tests/_route_cells.py (64 x 64, r0 16, M 2, mask CLOUD, 1473 observed rows).

1. against the dense twin of the iteration (tests/_laplace_trend.py), p = 1, 3, 17 (the first cross-block tile inside the iteration)
and 40 (three blocks); 2. the Gaussian family is mra_trend_fit, bit for bit; 3. against mra_plan_fit_laplace with X beta^ in the
offset; 4. one factorisation pass per iteration and no predict pass; 5. the state the call leaves; 6. edges and refusals;
7. MRATree.fitLaplace(X=X).

Bars: ORACLE_BARS of tests/test_gpu_routes.py (1e-10 relative for likelihood-type numbers, 1e-9 for means, 1e-8 relative for sds),
and for beta^ and cov_beta 1e-9 of max |beta| and of max |cov_beta|, the bound of tests/test_gpu_trend.py."""
import ctypes as C

import numpy as np
import pytest

import _cases as K
import _laplace as LP
import _laplace_trend as LT
import _noise as NZ
import _route_cells as RC
import test_gpu_likelihood_masks as MK
import test_gpu_routes as TR

pytestmark = pytest.mark.gpu

TOL = 1e-10
NOT_SPD, STATE, INVALID = -3, -4, -1
CASES = [(f, p) for f in (LP.POISSON, LP.BINOMIAL) for p in (1, 3, 17, 40)]
CASE_IDS = ["%s-p%d" % (LP.NAMES[f], p) for f, p in CASES]


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _caller(topo, buf):
    """a padded buffer in the caller's row order (0 at rows outside every leaf)"""
    rows = (topo.perm >= 0) & np.asarray(topo.in_leaf, dtype=bool)
    out = np.zeros(topo.N)
    out[topo.perm[rows]] = buf[rows]
    return out


def _padded(topo, cols):
    """(N, c) columns in the caller's order -> (c, P) in padded leaf order, 0 at the padding"""
    cols = np.asarray(cols, dtype=np.float64).reshape(topo.N, -1)
    return np.ascontiguousarray(np.where((topo.perm >= 0)[None, :], cols[topo.src, :].T, 0.0))


def _plan(hip, topo, locs, y, X=None):
    pl = MK._plan(hip, topo, locs, y)
    if X is not None:
        pl.set_trend(X)
    return pl


def _fit(pl, family, z, aux, offset, **kw):
    kw.setdefault("tol", TOL)
    return pl.fit_laplace_trend(LP.NAMES[family], z, aux=aux, offset=offset, **kw)


def _launches(pl):
    return np.array([k["launches"] for k in pl.kernel_stats()])


# ---- 1. against the dense twin ---------------------------------------------------------------------------------------------------------
def test_the_twin_pins_the_pass_count_in_most_cases():
    """passes is compared where each of the twin's last two steps lies a factor 2 from the threshold: at least 6 of the 8 cases"""
    pinned = [LT.passes_are_pinned(LT.t16_fit(f, p)[4], TOL) for f, p in CASES]
    assert sum(pinned) >= 6, pinned


@pytest.mark.parametrize("family,p", CASES, ids=CASE_IDS)
def test_t16_against_the_dense_twin(hip, family, p):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, X, ref = LT.t16_fit(family, p)
    tag = "T16 %s p=%d" % (LP.NAMES[family], p)
    pl = _plan(hip, topo, locs, y, X)
    res = _fit(pl, family, z, aux, offset)
    print("%s: passes %d (dense %d), step %.2e (dense %.2e)" % (tag, res["passes"], ref["info"][5], res["step"], ref["info"][6]))
    e_b = np.abs(res["beta"] - ref["beta"]).max()
    e_c = np.abs(res["cov_beta"] - ref["cov_beta"]).max()
    print("%s: beta err %.2e (max %.2f), cov_beta err %.2e (max %.2e), cond A %.1f" % (tag, e_b, np.abs(ref["beta"]).max(), e_c,
                                                                                     np.abs(ref["cov_beta"]).max(), np.linalg.cond(ref["A"])))
    errs = {}
    for k in (0, 1, 2, 3, 4, 8, 9, 10):
        errs[k] = abs(res["info"][k] - ref["info"][k]) / abs(ref["info"][k])
        print("info[%d]: %.10f vs %.10f, rel %.2e" % (k, res["info"][k], ref["info"][k], errs[k]))
    fit = pl.trend_fit(predict=True)
    assert e_b <= 1e-9 * np.abs(ref["beta"]).max()
    assert e_c <= 1e-9 * np.abs(ref["cov_beta"]).max()
    for k, e in errs.items():
        assert e <= TR.ORACLE_BARS[0], "%s: info[%d] rel err %.3e" % (tag, k, e)
    assert res["profile"] == res["info"][9] == res["lik"] and res["reml"] == res["info"][10] and res["logdetA"] == res["info"][8]
    assert res["n_obs"] == int(o.sum()) == int(ref["info"][11])
    # e^ and its sd (the uncertainty of beta^ in it) from the plan as the call leaves it
    TR._against(topo, counts, (res["profile"], fit.mean, np.sqrt(fit.var)), (ref["info"][9], ref["mean"], ref["sd"]), TR.ORACLE_BARS, tag + " vs dense")
    assert np.abs(fit.beta - res["beta"]).max() <= 1e-12 * np.abs(res["beta"]).max()      # the same t and r: the same GLS
    assert res["converged"] is True and res["info"][7] == 1.0 == ref["info"][7]
    if LT.passes_are_pinned(ref, TOL):
        assert res["passes"] == int(ref["info"][5])
    pl.close()


# ---- 2. the Gaussian family ------------------------------------------------------------------------------------------------------------
def _raw_trend_fit(pl, p):
    beta, cov, info = np.zeros(p), np.zeros((p, p)), np.zeros(8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                         # noqa: E731
    rc = pl.lib.mra_trend_fit(pl._h, C.c_uint32(0), ptr(beta), ptr(cov), None, None, ptr(info))
    assert rc == 0, pl.lib.mra_last_error(pl._h)
    return beta, cov, info


@pytest.mark.parametrize("p", [3, 17])
def test_gaussian_family_is_trend_fit_bit_for_bit(hip, p):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, X, ref = LT.t16_fit(LP.GAUSSIAN, p)
    pl = _plan(hip, topo, locs, y, X)
    res = _fit(pl, LP.GAUSSIAN, z, aux, offset)
    assert res["passes"] == 2 and res["step"] == 0.0 and res["converged"]
    fresh = hip.HipPlan(topo, 0)
    s = MK._spec()
    fresh.set_locs(locs); fresh.set_obs((z - offset).reshape(-1, 1), aux); fresh.set_kernel(s.kind, s.l, s.sig, s.scale)
    fresh.set_trend(X)
    beta, cov, info = _raw_trend_fit(fresh, p)
    assert np.array_equal(res["beta"], beta) and np.array_equal(res["cov_beta"], cov)
    assert res["info"][0] == info[0] and res["info"][1] == info[1] and res["info"][8] == info[2]
    e_b = np.abs(beta - ref["beta"]).max()
    print("gaussian p=%d: beta err vs dense %.2e" % (p, e_b))
    assert e_b <= 1e-9 * np.abs(ref["beta"]).max()
    fresh.close(); pl.close()


# ---- 3. against the code that exists -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,p", [(LP.POISSON, 3), (LP.BINOMIAL, 17)], ids=["poisson-p3", "binomial-p17"])
def test_fit_laplace_with_the_trend_in_the_offset_reproduces_the_field(hip, family, p):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, X, ref = LT.t16_fit(family, p)
    pl = _plan(hip, topo, locs, y, X)
    res = _fit(pl, family, z, aux, offset)
    fit = pl.trend_fit(predict=True)
    rep = NZ.reported(topo)
    xh = np.where(rep, fit.mean - X @ res["beta"], 0.0)
    plain = _plan(hip, topo, locs, y)
    off2 = X @ res["beta"] + (0.0 if offset is None else offset)
    want = plain.fit_laplace(LP.NAMES[family], z, aux=aux, offset=off2, tol=TOL)
    m, _ = plain.predict()
    e_m = np.abs(xh - m).max()
    e_d, e_s = abs(res["d"] - want["d"]) / abs(want["d"]), abs(res["sum_log_D"] - want["sum_log_D"]) / abs(want["sum_log_D"])
    print("%s p=%d: x^ err %.2e, d rel %.2e, sum log D rel %.2e" % (LP.NAMES[family], p, e_m, e_d, e_s))
    assert want["converged"]
    assert e_m <= TR.ORACLE_BARS[1]
    assert e_d <= 1e-10 and e_s <= 1e-10
    plain.close(); pl.close()


# ---- 4. one pass per iteration -------------------------------------------------------------------------------------------------------------
def test_one_factorisation_pass_per_iteration_and_no_predict_pass(hip):
    """kernel_stats() sums the launches of the whole call.  F: the launches of a call of one pass on a fresh plan; L: of a call of one
    pass on that plan again (the prior and its residual stand: options 24 and 25).  A call of n passes on a fresh plan launches
    F + (n - 1) L, family by family, and nothing of the two predict families."""
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, X, ref = LT.t16_fit(LP.POISSON, 17)
    PRED = (9, 10)                                                       # KF_PRED_TRSM, KF_PRED_UPDATE
    a = _plan(hip, topo, locs, y, X)
    r1 = _fit(a, LP.POISSON, z, aux, offset, max_iter=1)
    F = _launches(a)
    assert r1["passes"] == 1 and not r1["converged"]
    _fit(a, LP.POISSON, z, aux, offset, max_iter=1)
    L = _launches(a)
    r2 = _fit(a, LP.POISSON, z, aux, offset, max_iter=2)
    assert r2["passes"] == 2 and np.array_equal(_launches(a), 2 * L)
    a.run(True, True)
    pred = _launches(a)
    assert sum(pred[k] for k in PRED) > 0                                # what a predict pass would have added
    print("launches by family: fresh pass %s, later pass %s, predict pass %s" % (F.tolist(), L.tolist(), pred.tolist()))
    assert F[2] > 0 and L[1] == 0 and L[2] == 0                          # the prior of the first pass is reused
    assert L[4] > 0 and L[4] == F[4]                                     # every pass factorises the leaves
    b = _plan(hip, topo, locs, y, X)
    res = _fit(b, LP.POISSON, z, aux, offset)
    total = _launches(b)
    n = res["passes"]
    print("call of %d passes: %s" % (n, total.tolist()))
    assert res["converged"] and n == int(ref["info"][5])
    assert np.array_equal(total, F + (n - 1) * L)
    assert all(total[k] == 0 for k in PRED)
    # a second call from e^ takes one pass
    e_hat = b.trend_fit(predict=True).mean
    again = _fit(b, LP.POISSON, z, aux, offset, e0=e_hat)
    assert again["passes"] == 1 and again["converged"]
    assert np.abs(again["beta"] - res["beta"]).max() <= 1e-9 * np.abs(res["beta"]).max()
    a.close(); b.close()


# ---- 5. state --------------------------------------------------------------------------------------------------------------------------------
def test_the_state_the_call_leaves(hip):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    family, p = LP.POISSON, 3
    z, aux, offset, X, ref = LT.t16_fit(family, p)
    seen = np.isfinite(z) & NZ.reported(topo)
    pl = _plan(hip, topo, locs, y, X)
    pl.run(True, True)
    lik0, (m0, v0) = pl.likelihood(), pl.predict()
    res = _fit(pl, family, z, aux, offset)
    assert pl.likelihood() == lik0 and np.array_equal(pl.predict()[0], m0) and np.array_equal(pl.predict()[1], v0)
    assert pl.info()["trend_p"] == p                                     # X is kept
    fit = pl.trend_fit(predict=True)
    assert pl.likelihood() == lik0 and np.array_equal(pl.predict()[0], m0)
    # buffers 10 / 11: r and t of the last pass.  At the fixed point t = e^ + g(eta^) / D(eta^) and r = 1 / D(eta^) up to the last
    # step (at most TOL max(1, max |e^|)); r is a smooth function of e with |d log r / d e| <= 1
    t, r = _caller(topo, pl.buffer(11)), _caller(topo, pl.buffer(10))
    eh = fit.mean[seen]
    g, D, _ = LP.terms(family, z[seen], 1.0, eh + offset[seen])
    e_t = np.abs(t[seen] - (eh + g / D)) / np.maximum(1.0, np.abs(eh))
    e_r = np.abs(r[seen] * D - 1.0)
    print("fixed point: t %.2e, r %.2e" % (e_t.max(), e_r.max()))
    assert e_t.max() <= 10 * TOL                                         # test_gpu_laplace._fixed_point_and_fresh_plan
    assert e_r.max() <= TOL * max(1.0, np.abs(eh).max()) + TR.ORACLE_BARS[1]
    assert np.all(r[seen] > 0) and np.all(r[~seen] == 0)
    # predict_sites at tree rows with Y = [t | X] composes to e^
    rows = np.random.default_rng(2).choice(np.nonzero(NZ.reported(topo))[0], 40, replace=False)
    leaf_of = np.full(topo.N, -1, dtype=np.int32)
    for i in np.nonzero(topo.node_leaf)[0]:
        leaf_of[MK._leaf_callers(topo, i)] = i
    Y = _padded(topo, np.column_stack([np.nan_to_num(t), X]))
    m, _ = pl.predict_sites(np.asarray(locs)[rows], leaf_of[rows], Y=Y, want_var=False)
    composed = m[0] + (X[rows] - m[1:].T) @ res["beta"]
    e_p = np.abs(composed - fit.mean[rows]).max()
    print("predict_sites composes to e^: %.2e" % e_p)
    assert e_p <= 1e-8 * max(1.0, np.abs(fit.mean).max())                # test_gpu_trend: predictAt against predict
    # set_obs returns the plan to the Gaussian model
    pl.set_obs(y, MK.R)
    back = TR._predict(pl)
    fresh = _plan(hip, topo, locs, y)
    want = TR._predict(fresh)
    assert back[0] == want[0] and np.array_equal(back[1], want[1]) and np.array_equal(back[2], want[2])
    # mra_plan_fit_laplace ignores a trend
    r_with = pl.fit_laplace(LP.NAMES[family], z, aux=aux, offset=offset, tol=TOL)
    s_with = (pl.likelihood(), pl.predict())
    r_without = fresh.fit_laplace(LP.NAMES[family], z, aux=aux, offset=offset, tol=TOL)
    assert np.array_equal(r_with["info"], r_without["info"])
    assert s_with[0] == fresh.likelihood() and np.array_equal(s_with[1][0], fresh.predict()[0]) and np.array_equal(s_with[1][1], fresh.predict()[1])
    assert pl.info()["trend_p"] == p
    fresh.close(); pl.close()


def test_trend_fit_still_times_its_rows_and_transfers(hip):
    """mra_get_buffer(14) of a predicting mra_trend_fit with kernel timing on: the staging, the sweeps, k_trend_rows and the
    transfers all land in the trend's own record (trend_gls is shared with the Laplace call; the record is the call's).  After mra_plan_fit_laplace_trend the same record holds the sweeps and the tail of its passes."""
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, X, ref = LT.t16_fit(LP.POISSON, 17)
    pl = _plan(hip, topo, locs, y, X)
    pl.set_option(hip.MRA_OPT_KERNEL_TIMING, 1)
    pl.trend_fit(predict=True)
    ms = pl.buffer(14)
    print("trend_fit(predict) ms: stage %.4f sweeps %.4f cross %.4f rows %.4f transfers %.4f" % tuple(ms[:5]))
    assert len(ms) == 7 and all(ms[k] > 0.0 for k in range(5))           # two blocks: the cross tiles too
    quad_only = pl.trend_fit()
    ms0 = pl.buffer(14)
    assert ms0[3] == 0.0 and ms0[1] > 0.0 and quad_only.mean is None     # no rows without MRA_TREND_PREDICT
    res = _fit(pl, LP.POISSON, z, aux, offset)
    ms1 = pl.buffer(14)
    print("fit_laplace_trend ms over %d passes: stage %.4f sweeps %.4f cross %.4f tail %.4f transfers %.4f" % ((res["passes"],) + tuple(ms1[:5])))
    assert res["converged"] and all(ms1[k] > 0.0 for k in range(5))
    pl.close()


# ---- 6. edges ------------------------------------------------------------------------------------------------------------------------------
def test_non_finite_iterate_is_refused_never_converged(hip):
    """Poisson counts in the thousands from e0 = 0: the dense twin's second pass linearises at e^eta = inf (t = NaN, r = 0) and
    ends there, not converged, with a step that is not finite.  The device pass does not get as far as a mean: r = 0 at a row that
    is an upper node's knot leaves that leaf no positive pivot, and the pass is refused MRA_ERR_NOT_SPD with the r of that pass in
    the plan, exactly as in mra_plan_fit_laplace (tests/test_gpu_laplace.py pins the same for the trendless call; a pass's own
    refusal propagates).  The call never returns converged, and the plan is not poisoned."""
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    family, z, aux, offset = LP.edge_inputs("big_counts")
    X = LT.design(topo.N, 3)
    twin = LT.dense_laplace_trend(Sigma, o, family, z, aux, offset, X, e0=np.zeros(topo.N), max_iter=10)
    assert twin["info"][5] == 2 and twin["info"][7] == 0.0 and not np.isfinite(twin["info"][6])
    pl = _plan(hip, topo, locs, y, X)
    knot = np.zeros(int(o.sum()), dtype=bool)
    knot[list(LP.t16_upper_knots())] = True
    assert (np.isnan(twin["t"][o]) & (twin["r"][o] == 0.0) & knot).any()          # the rows the refusal comes from
    with pytest.raises(hip.MraError) as ei:
        _fit(pl, family, z, aux, offset, e0=np.zeros(topo.N), max_iter=10)
    print("big_counts from 0: %s" % ei.value)
    assert ei.value.code == NOT_SPD and "not positive definite" in str(ei.value)
    r = _caller(topo, pl.buffer(10))
    assert np.array_equal(r[o] == 0.0, twin["r"][o] == 0.0) and (r[o] == 0.0).any()          # pass 2's r, as the twin has it
    ref = LT.dense_laplace_trend(Sigma, o, family, z, aux, offset, X)
    good = _fit(pl, family, z, aux, offset)                              # the data-based start on the same data
    assert good["converged"] and ref["info"][7] == 1.0
    assert np.abs(good["beta"] - ref["beta"]).max() <= 1e-9 * np.abs(ref["beta"]).max()
    assert abs(good["profile"] - ref["info"][9]) <= TR.ORACLE_BARS[0] * abs(ref["info"][9])
    pl.close()


def _raw(pl, fam, z_perm, beta=True):
    b, cv, i = np.zeros(64), np.zeros((64, 64)), np.zeros(12)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                         # noqa: E731
    rc = pl.lib.mra_plan_fit_laplace_trend(pl._h, fam, ptr(z_perm), None, None, None, 5, TOL, ptr(b) if beta else None, ptr(cv), ptr(i))
    return rc, pl.lib.mra_last_error(pl._h).decode()


def test_dependent_columns_and_the_refusals_in_order(hip):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, X, ref = LT.t16_fit(LP.POISSON, 3)
    zp = np.ascontiguousarray(np.where(topo.perm >= 0, z[topo.src], np.nan))
    WHO = "mra_plan_fit_laplace_trend"
    pl = _plan(hip, topo, locs, y)
    # no trend: MRA_ERR_STATE, before any argument
    rc, msg = _raw(pl, 9, zp, beta=False)
    assert rc == STATE and msg == WHO + " needs mra_plan_set_trend first"
    # a sharded plan: refused as such before the missing trend is
    pl.set_reduce_level(0)
    rc, msg = _raw(pl, 9, zp, beta=False)
    assert rc == INVALID and msg == WHO + ": sharded plans cannot fit a trend"
    pl.set_reduce_level(-1)
    # two identical columns: a pivot of A fails mra_trend_fit's test in the first pass; the plan holds that pass's t and r.  (The
    # first column is ten times as large, so the floor 3 * 2^-52 * max diag(A) is far above the rounding the pivot is left with.)
    c = X[:, 1]
    pl.set_trend(np.column_stack([np.full(topo.N, 10.0), c, c]))
    with pytest.raises(hip.MraError) as e:
        _fit(pl, LP.POISSON, z, aux, offset)
    assert e.value.code == NOT_SPD and WHO + ": trend columns are linearly dependent at the observed rows" in str(e.value)
    t, r = _caller(topo, pl.buffer(11)), _caller(topo, pl.buffer(10))
    t1, r1 = LP.linearise(LP.POISSON, z[o], 1.0, offset[o], LP.start(LP.POISSON, z[o], 1.0, offset[o]))
    assert np.abs(t[o] - t1).max() <= 1e-12 * np.abs(t1).max() and np.abs(r[o] / r1 - 1.0).max() <= 1e-12
    # the plan is whole: the independent columns on the same plan
    pl.set_trend(X)
    res = _fit(pl, LP.POISSON, z, aux, offset)
    assert res["converged"] and np.abs(res["beta"] - ref["beta"]).max() <= 1e-9 * np.abs(ref["beta"]).max()
    # NULL beta: the last of the refusals
    rc, msg = _raw(pl, LP.POISSON, zp, beta=False)
    assert rc == INVALID and msg == WHO + ": beta is NULL"
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
    rc, msg = _raw(tree.plan, 9, np.zeros(tree.plan.topo.P), beta=False)
    assert rc == INVALID and msg.startswith(WHO + ": MRA_KERNEL_HOST plans cannot fit a trend")
    with pytest.raises(NotImplementedError):
        tree.fitLaplace("gaussian", aux=1.0, X=np.ones((n * n, 1)))


def test_1d_tree_with_dropped_rows(hip):
    """t201, whose partition drops rows, p = 3: no dense covariance here, so the truth is the trendless fit with X beta^ in the
    offset (test 3) and the fixed point."""
    cs = K.load_case("t201")
    topo, locs, y, spec, R1 = cs["topo"], cs["locs"], cs["y_obs"], cs["spec"], float(cs["c"]["R"])
    rep = NZ.reported(topo)
    obs = np.isfinite(np.asarray(y).ravel())
    assert not rep.all() and (obs & ~rep).any()
    family = LP.POISSON
    z, aux, offset, X = LT.inputs(locs, obs, family, 3)
    seen = obs & rep

    def plan():
        q = hip.HipPlan(topo, 0)
        q.set_locs(locs); q.set_obs(y, R1); q.set_kernel(spec.kind, spec.l, spec.sig, spec.scale, spec.circular)
        return q

    pl = plan()
    pl.set_trend(X)
    res = _fit(pl, family, z, aux, offset, max_iter=30)
    fit = pl.trend_fit(predict=True)
    print("t201 p=3: passes %d, step %.2e, beta %s" % (res["passes"], res["step"], res["beta"]))
    assert res["converged"] and res["n_obs"] == int(seen.sum())
    assert np.all(fit.mean[~rep] == 0.0)
    plain = plan()
    want = plain.fit_laplace(LP.NAMES[family], z, aux=aux, offset=offset + X @ res["beta"], tol=TOL, max_iter=30)
    m, _ = plain.predict()
    xh = np.where(rep, fit.mean - X @ res["beta"], 0.0)
    e_m = np.abs(xh - m).max()
    print("t201 p=3: x^ err %.2e, d rel %.2e" % (e_m, abs(res["d"] - want["d"]) / abs(want["d"])))
    assert want["converged"] and e_m <= TR.ORACLE_BARS[1]
    assert abs(res["d"] - want["d"]) <= 1e-10 * abs(want["d"])
    # the score of beta vanishes at the mode: X_o^T g(eta^) = 0, in units of the sums of |X| (|z| + e^eta)
    g, D, _ = LP.terms(family, z[seen], 1.0, fit.mean[seen] + offset[seen])
    score = np.abs(X[seen].T @ g) / (np.abs(X[seen]).T @ (np.abs(z[seen]) + (z[seen] - g)))
    print("t201 p=3: score %s" % score)
    assert score.max() <= 1e-9
    plain.close(); pl.close()


# ---- 7. MRATree -----------------------------------------------------------------------------------------------------------------------------
def test_mratree_fit_laplace_with_a_trend(hip):
    import pymra_amd
    import pymra_amd.MRATools as mt
    n, r0, M = RC.TREES["T16"]
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    family, p = LP.POISSON, 3
    z, aux, offset, X, ref = LT.t16_fit(family, p)
    pl = _plan(hip, topo, locs, y, X)
    want = _fit(pl, family, z, aux, offset)
    want_fit = pl.trend_fit(predict=True)
    pl.close()
    s = MK._spec()
    cov = lambda a, b: mt.Matern32(a, b, l=s.l, sig=s.sig)           # noqa: E731
    np.random.seed(7)                                                 # as MK._tree does: the same knots
    mt.genLocations2d(Nx=n, Ny=n)
    tree = pymra_amd.MRATree(locs, r0, cov, z.reshape(-1, 1), MK.R, M=M, J=4)
    assert np.array_equal(tree.topology.knot_rows, topo.knot_rows)
    sent = []
    send = tree.plan.set_trend
    tree.plan.set_trend = lambda A: (sent.append(A is not None), send(A))[1]
    lik = tree.fitLaplace("poisson", offset=offset, X=X, tol=TOL)
    assert sent == [True]
    # equals the HipPlan path
    assert abs(lik - want["profile"]) <= 1e-12 * abs(want["profile"]) and tree.laplace["passes"] == want["passes"] and tree.laplace["converged"]
    assert np.abs(tree.trend.beta - want["beta"]).max() <= 1e-12 * np.abs(want["beta"]).max()
    assert np.abs(tree.trend.cov_beta - want["cov_beta"]).max() <= 1e-12 * np.abs(want["cov_beta"]).max()
    mean, sd = tree.predict()
    mean = np.asarray(mean).ravel()
    scale = max(1.0, np.abs(mean).max())
    assert np.abs(mean - want_fit.mean).max() <= 1e-12 * scale and np.abs(sd - np.sqrt(want_fit.var)).max() <= 1e-12 * max(1.0, sd.max())
    assert abs(float(np.asarray(tree.getLikelihood(reml=True))[0, 0]) - tree.trend.reml) == 0.0
    # predict() equals predictAt at tree locations
    rows = np.random.default_rng(2).choice(len(locs), 50, replace=False)
    ma, sda = tree.predictAt(locs[rows], X_sites=X[rows])
    print("predictAt: mean err %.2e, sd err %.2e" % (np.abs(ma[:, 0] - mean[rows]).max(), np.abs(sda - sd[rows]).max()))
    assert np.abs(ma[:, 0] - mean[rows]).max() <= 1e-8 * scale
    assert np.abs(sda - sd[rows]).max() <= 1e-8 * max(1.0, sd.max())
    # the same X object again: nothing is uploaded, and the warm start converges in one pass
    again = tree.fitLaplace("poisson", offset=offset, X=X, tol=TOL, reml=True)
    assert sent == [True] and tree.laplace["passes"] == 1 and tree.laplace["converged"]
    assert abs(again - want["reml"]) <= TR.ORACLE_BARS[0] * abs(want["reml"])
    # another array with the same values is sent
    tree.fitLaplace("poisson", offset=offset, X=X.copy(), tol=TOL)
    assert sent == [True, True]
    # without X a tree that has a trend still refuses
    with pytest.raises(NotImplementedError) as e:
        tree.fitLaplace("poisson", offset=offset)
    assert "trend" in str(e.value)
