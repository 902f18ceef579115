"""mra_cv / HipPlan.cv / MRATree.crossValidate on the GPU: leave-one-out and leave-a-leaf-out predictive distributions from the retained
factors, without a refit.  Truths that do not come from the new kernels: the NumPy restatement tests/_treecv.py (pinned to brute-force
refits of the level-wise oracle by tests/test_cv_cpu.py), brute-force refits on the device itself (set_obs with the group's rows NaN,
predict() and the posterior cov_apply of unit columns at those rows), and the per-row formula on predict()'s own mean and variance.

Measures, as tests/test_cv_cpu.py: mean |delta| / max|y|; variance relative; lpd and score |delta| / max(1, |value|).
Bound against the twin and against the device's refits: max(1e-9, 100 x the twin's own error against brute force on that case,
tests/_treecv.TWIN_ERR) - 1e-9 is what tests/test_gpu_sites.py holds means to, the second term is what the identity itself loses in
float64 on that case whatever computes it.  On trees without a twin error of their own (other shapes, kernels and masks) the bound is
that of the case with the largest leverage measured, g32 (max v / R 0.972), and the tree with leaves of nine tiles has a figure of
its own; the tests print max v / R, and where it exceeds 0.98 the bound is scaled by (0.02 / (1 - h))^2, what the identity loses there."""
import ctypes as C

import numpy as np
import pytest

import _cases as K
import _sampling as SM
import _treecv as CV
import _treesites as TS
import test_gpu_cov as GC

pytestmark = pytest.mark.gpu

CASES = ["g32", "c1", "kat3", "u3"]
R_CV = 1e-2
H_MAX = 0.98
LOG_2PI = CV.LOG_2PI


def _tol(name="g32"):
    return max(1e-9, 100.0 * CV.TWIN_ERR[name])


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _rel1(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def _errors(got, want, ymax):
    """(mean, variance, lpd, group lpd, score and by-product) errors of two (mean, var, lpd, group, info) results, NaN patterns equal"""
    for a, b in zip(got[:4], want[:4]):
        assert np.array_equal(np.isnan(a), np.isnan(b))
    ok, gk = ~np.isnan(want[0]), ~np.isnan(want[3])
    e_m = np.abs(got[0][ok] - want[0][ok]).max() / ymax
    e_v = (np.abs(got[1][ok] - want[1][ok]) / want[1][ok]).max()
    e_l = _rel1(got[2][ok], want[2][ok]).max()
    e_g = _rel1(got[3][gk], want[3][gk]).max()
    e_i = max(_rel1(got[4][k], want[4][k]) for k in (2, 3, 4)) + max(abs(got[4][k] - want[4][k]) / abs(want[4][k]) for k in (5, 6, 7))
    assert got[4][0] == want[4][0] and got[4][1] == want[4][1]
    return e_m, e_v, e_l, e_g, e_i


def _against_twin(pl, topo, locs, spec, y_obs, R, tag, tol, modes=(False, True)):
    S = TS.SiteState(topo, locs, spec, y_obs, R)
    ymax = np.nanmax(np.abs(np.asarray(y_obs, float)))
    out = {}
    for leaf in modes:
        want = CV.tree_cv(S, leaf)
        got = pl.cv(leaf=leaf)
        e = _errors(got, want, ymax)
        print("%s %s: %d rows, %d groups against the twin: mean %.2e, var %.2e, lpd %.2e, group lpd %.2e, info %.2e (max h %.6f, bound %.1e)"
              % (tag, "by leaf" if leaf else "by row", got[4][0], got[4][1], *e, got[4][5], tol))
        assert got[4][5] <= H_MAX or tag not in CASES          # the four cases: a condition of the test
        assert max(e) <= tol * max(1.0, (0.02 / (1.0 - got[4][5])) ** 2)      # beyond 0.98 the identity loses eps / (1 - h)^2: the bound follows
        out[leaf] = got
    return out


def _loo_against_predict(pl, topo, y_obs, r, rows, tag, tol_m, tol_v):
    """leave-one-out at the padded rows `rows` against the per-row formula on predict()'s own mean and variance (r: by padded row)"""
    m0, v0 = pl.predict()
    mean, var, lpd, group, info = pl.cv()
    y = np.asarray(y_obs, float).ravel()[topo.perm[rows]]
    m, v = m0[topo.perm[rows]], v0[topo.perm[rows]]
    h = v / r[rows]
    want_m, want_v = y - (y - m) / (1.0 - h), r[rows] / (1.0 - h)
    e_m, e_v = np.abs(mean[rows] - want_m).max() / np.abs(y).max(), (np.abs(var[rows] - want_v) / want_v).max()
    print("%s by row: %d rows against predict(): mean %.2e, var %.2e (max h %.6f)" % (tag, len(rows), e_m, e_v, info[5]))
    assert e_m <= tol_m and e_v <= tol_v
    return mean, var, lpd, group, info


def _refit_group(pl2, topo, y_obs, R, rows):
    """brute force on the device: the padded rows of one group set to NaN, a pass, predict() and the posterior covariance columns"""
    y2 = np.asarray(y_obs, float).reshape(-1, 1).copy()
    y2[topo.perm[rows]] = np.nan
    pl2.set_obs(y2, R)
    pl2.run(True, True)
    m, _ = pl2.predict()
    Ap = np.zeros((len(rows), topo.P))
    Ap[np.arange(len(rows)), rows] = 1.0
    out, _ = pl2.cov_apply(Ap, posterior=True, want_gram=False)
    Sg = out[:, rows] + R * np.eye(len(rows))
    mu = m[topo.perm[rows]]
    e = np.asarray(y_obs, float).ravel()[topo.perm[rows]] - mu
    L = np.linalg.cholesky(.5 * (Sg + Sg.T))
    w = np.linalg.solve(L, e)
    return mu, np.diag(Sg), -.5 * (2.0 * np.log(np.diag(L)).sum() + w @ w + len(rows) * LOG_2PI)


def _leaves_against_refits(hip, got, topo, locs, y_obs, R, spec, leaves, tag, tol_m, tol_v, tol_l):
    mean, var, lpd, group, info = got
    pl2 = GC._plan(hip, topo, locs, y_obs, R, spec, run=False)
    obs_p = np.isfinite(np.asarray(y_obs, float).ravel())[topo.src] & (topo.perm >= 0)
    ymax = np.nanmax(np.abs(np.asarray(y_obs, float)))
    e_m = e_v = e_l = 0.0
    for i in leaves:
        rows = np.arange(int(topo.node_row0[i]), int(topo.node_row1[i]))
        rows = rows[obs_p[rows]]
        mu, dg, lp = _refit_group(pl2, topo, y_obs, R, rows)
        e_m = max(e_m, np.abs(mean[rows] - mu).max() / ymax)
        e_v = max(e_v, (np.abs(var[rows] - dg) / dg).max())
        e_l = max(e_l, float(_rel1(group[i], lp)))
    pl2.close()
    print("%s by leaf: %d leaves against refits on the device: mean %.2e, var %.2e, group lpd %.2e (max h %.6f)" % (tag, len(leaves), e_m, e_v, e_l, info[5]))
    assert e_m <= tol_m and e_v <= tol_v and e_l <= tol_l


def _leaves(topo):
    return [int(i) for i in np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]]


# ---- 1. the device against the twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_device_against_the_twin(hip, name):
    cs = K.load_case(name)
    topo, locs, spec, y_obs = cs["topo"], cs["locs"], cs["spec"], cs["y_obs"]
    pl = GC._plan(hip, topo, locs, y_obs, R_CV, spec)
    got = _against_twin(pl, topo, locs, spec, y_obs, R_CV, name, _tol(name))
    for leaf in (False, True):
        mean, var, lpd, group, info = got[leaf]
        assert abs(np.nansum(group) - info[2]) <= 1e-12 * max(1.0, abs(info[2]))
        assert abs(np.nansum(lpd) - info[3]) <= 1e-12 * max(1.0, abs(info[3]))
    assert got[False][4][2] == got[False][4][3]               # every row its own group
    pl.close()


# ---- 2. the device against brute force on the device ------------------------------------------------------------------------------------
def test_g32_against_refits_on_the_device(hip):
    cs = K.load_case("g32")
    topo, locs, spec, y_obs = cs["topo"], cs["locs"], cs["spec"], cs["y_obs"]
    pl = GC._plan(hip, topo, locs, y_obs, R_CV, spec)
    tol = _tol("g32")
    by_leaf, by_row = pl.cv(leaf=True), pl.cv()
    pl.close()
    _leaves_against_refits(hip, by_leaf, topo, locs, y_obs, R_CV, spec, _leaves(topo), "g32", tol, tol, tol)
    obs_p = np.isfinite(np.asarray(y_obs, float).ravel())[topo.src] & (topo.perm >= 0)
    pick = np.sort(np.random.default_rng(5).choice(np.nonzero(obs_p)[0], 12, replace=False))
    pl2 = GC._plan(hip, topo, locs, y_obs, R_CV, spec, run=False)
    ymax = np.nanmax(np.abs(np.asarray(y_obs, float)))
    e_m = e_v = e_l = 0.0
    for row in pick:
        mu, dg, lp = _refit_group(pl2, topo, y_obs, R_CV, np.array([row]))
        e_m = max(e_m, abs(by_row[0][row] - mu[0]) / ymax)
        e_v = max(e_v, abs(by_row[1][row] - dg[0]) / dg[0])
        e_l = max(e_l, float(_rel1(by_row[2][row], lp)))
    pl2.close()
    print("g32 by row: 12 rows against refits on the device: mean %.2e, var %.2e, lpd %.2e" % (e_m, e_v, e_l))
    assert max(e_m, e_v, e_l) <= tol


# ---- 3. shapes where the kernels can go wrong -------------------------------------------------------------------------------------------
def test_leaves_of_nine_tiles(hip):
    topo, locs, y_obs, spec, R = GC._shape_tree("grid48_r20")            # leaves of 144 rows, 70 % observed: multi-tile Gram, Cholesky, solve
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    _against_twin(pl, topo, locs, spec, y_obs, R, "grid48_r20", _tol("grid48_r20"))
    pl.close()


def test_a_leaf_of_193_observations(hip):
    import _route_cells as RC
    import test_gpu_likelihood_masks as MK
    topo, locs = MK._tree(*RC.TREES["A"])
    obs = RC.make_obs(topo, locs, ("edges", "empty_first", 193))        # 13 tiles, an empty first leaf and an empty family
    y = MK._y(obs)
    spec = MK._spec()
    pl = GC._plan(hip, topo, locs, y, MK.R, spec)
    counts = MK.leaf_counts(topo, obs)
    leaves = _leaves(topo)
    assert max(counts) == 193 and counts[0] == 0
    obs_p = np.isfinite(np.asarray(y, float).ravel())[topo.src] & (topo.perm >= 0)
    r = np.full(topo.P, MK.R)
    got = _loo_against_predict(pl, topo, y, r, np.nonzero(obs_p)[0], "leaf of 193", _tol(), _tol())
    assert got[4][5] <= H_MAX
    assert np.isnan(got[3][leaves[0]])                                   # the empty first leaf has no group
    by_leaf = pl.cv(leaf=True)
    assert by_leaf[4][1] == sum(1 for c in counts if c > 0)
    pl.close()
    big = leaves[int(np.argmax(counts))]
    small = [i for i, c in zip(leaves, counts) if 0 < c][:2]
    _leaves_against_refits(hip, by_leaf, topo, locs, y, MK.R, spec, [big] + small, "leaf of 193", _tol(), _tol(), _tol())


def test_leaves_of_1_16_and_17_observations(hip):
    cs = K.load_case("g32")
    topo, locs, spec = cs["topo"], cs["locs"], cs["spec"]
    y = np.asarray(cs["y_obs"], float).reshape(-1, 1).copy()
    full = np.random.default_rng(3).standard_normal(len(y))
    leaves = _leaves(topo)
    for i, cnt in zip((leaves[1], leaves[6], leaves[11]), (1, 16, 17)):   # padding columns of N_G become the identity
        rows = K.node_real_rows(topo, i)
        y[topo.perm[rows], 0] = np.nan
        y[topo.perm[rows[:cnt]], 0] = full[:cnt]
    pl = GC._plan(hip, topo, locs, y, R_CV, spec)
    got = _against_twin(pl, topo, locs, spec, y, R_CV, "g32 with leaves of 1, 16, 17", _tol())
    obs_p = np.isfinite(y.ravel())[topo.src] & (topo.perm >= 0)
    for i, cnt in zip((leaves[1], leaves[6], leaves[11]), (1, 16, 17)):
        assert int(obs_p[int(topo.node_row0[i]):int(topo.node_row1[i])].sum()) == cnt
    one = np.nonzero(obs_p[int(topo.node_row0[leaves[1]]):int(topo.node_row1[leaves[1]])])[0][0] + int(topo.node_row0[leaves[1]])
    for k in range(3):                                                    # a one-row group is the row's own leave-one-out
        assert abs(got[True][k][one] - got[False][k][one]) <= _tol() * max(1.0, abs(got[False][k][one]))      # (two routes to r - v)
    pl.close()


def test_deep_wide_tree(hip):
    """cw = 64, five ancestors, panel-only fronts at the leaves' parents"""
    topo, locs, y_obs, spec, R = GC._deep_wide()
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    obs_p = np.isfinite(np.asarray(y_obs, float).ravel())[topo.src] & (topo.perm >= 0)
    rows = np.concatenate([K.node_real_rows(topo, j) for j in GC._leaf_sets(topo)])
    rows = rows[obs_p[rows]]
    got = _loo_against_predict(pl, topo, y_obs, np.full(topo.P, R), rows, "deep wide", _tol(), _tol())
    assert got[4][5] <= H_MAX
    by_leaf = pl.cv(leaf=True)
    pl.close()
    sets = [j for j in GC._leaf_sets(topo) if obs_p[int(topo.node_row0[j]):int(topo.node_row1[j])].any()][:2]
    _leaves_against_refits(hip, by_leaf, topo, locs, y_obs, R, spec, sets, "deep wide", _tol(), _tol(), _tol())


@pytest.mark.parametrize("family", ["exp", "matern52", "gaussian", "kanter", "iden", "matern32_scale", "circular"])
def test_every_kernel_family(hip, family):
    import pymra_amd.MRATools as mt
    specs = {"exp": mt.KernelSpec(mt.KIND_EXP, 0.3), "matern52": mt.KernelSpec(mt.KIND_MATERN52, 0.2, 0.7),
             "gaussian": mt.KernelSpec(mt.KIND_GAUSSIAN, 0.05, 1.0), "kanter": mt.KernelSpec(mt.KIND_KANTER, 0.35),
             "iden": mt.KernelSpec(mt.KIND_IDEN, 0.01), "matern32_scale": mt.KernelSpec(mt.KIND_MATERN32, 0.4, 1.0, 2.5),
             "circular": mt.KernelSpec(mt.KIND_EXP, 0.3, 1.0, 1.0, True)}
    cs = K.load_case("c1" if family == "circular" else "g32")             # c1: a 1-D tree
    topo, locs, spec = cs["topo"], cs["locs"], specs[family]
    pl = GC._plan(hip, topo, locs, cs["y_obs"], R_CV, spec)
    _against_twin(pl, topo, locs, spec, cs["y_obs"], R_CV, family, _tol())
    pl.close()


def test_chordal_tree_in_three_dimensions(hip):
    import test_gpu_sphere as SP
    ll, xyz, topo, y = SP.tree(*SP.TREES["g64"])
    pl = SP.make_plan(hip, topo, xyz, y.reshape(-1, 1), SP.M32)
    pl.run(True, True)
    got = _against_twin(pl, topo, xyz, SP.M32, y, SP.R, "sphere g64", _tol())
    first = _leaves(topo)[0]
    assert np.isnan(got[True][3][first]) and np.isnan(got[False][3][first])      # the first leaf has no observation
    pl.close()


# ---- 4. noise vectors -------------------------------------------------------------------------------------------------------------------
def test_noise_vector(hip):
    cs = K.load_case("g32")
    topo, locs, spec, y_obs = cs["topo"], cs["locs"], cs["spec"], cs["y_obs"]
    pl = GC._plan(hip, topo, locs, y_obs, R_CV, spec)
    scalar = [pl.cv(leaf=leaf) for leaf in (False, True)]
    pl.set_noise(np.full(topo.N, R_CV))
    pl.run(True, True)
    for leaf in (False, True):                                            # a constant vector is the scalar path, bit for bit
        got = pl.cv(leaf=leaf)
        for a, b in zip(got, scalar[leaf]):
            assert np.array_equal(a, b, equal_nan=True)
    rv = R_CV * np.random.default_rng(8).uniform(0.5, 2.0, topo.N)
    pl.set_noise(rv)
    pl.run(True, True)
    rp = pl.buffer(10)
    obs_p = np.isfinite(np.asarray(y_obs, float).ravel())[topo.src] & (topo.perm >= 0)
    rows = np.nonzero(obs_p)[0]
    assert np.array_equal(rp[rows], rv[topo.perm[rows]])
    by_row = _loo_against_predict(pl, topo, y_obs, rp, rows, "g32 noise vector", _tol("g32"), _tol("g32"))
    by_leaf = pl.cv(leaf=True)
    # the twin with D = diag(r): dense algebra on Sigma[o, o] + diag(r_o) (tests/_treecv.dense_cv, pinned to the tree twin on the CPU)
    import _noise as NZ
    Sigma = NZ.prior_cov(topo, locs, spec, y_obs)
    ymax = np.nanmax(np.abs(np.asarray(y_obs, float)))
    for leaf, got in ((False, by_row), (True, by_leaf)):
        e = _errors(got, CV.dense_cv(topo, Sigma, y_obs, rv, leaf), ymax)
        print("g32 noise vector %s against the twin with D = diag(r): mean %.2e, var %.2e, lpd %.2e, group lpd %.2e, info %.2e (max h %.6f)"
              % ("by leaf" if leaf else "by row", *e, got[4][5]))
        assert max(e) <= _tol("g32") * max(1.0, (0.02 / (1.0 - got[4][5])) ** 2)
    # by leaf with D = diag(r): S_G = D N^-1 D from the posterior covariance columns of the SAME fit (cov_apply), formed densely
    m0, _ = pl.predict()
    e_m = e_v = e_l = 0.0
    for i in _leaves(topo)[:4]:
        g = np.arange(int(topo.node_row0[i]), int(topo.node_row1[i]))
        g = g[obs_p[g]]
        Ap = np.zeros((len(g), topo.P))
        Ap[np.arange(len(g)), g] = 1.0
        out, _ = pl.cov_apply(Ap, posterior=True, want_gram=False)
        D = np.diag(rp[g])
        N = D - .5 * (out[:, g] + out[:, g].T)
        rho = np.asarray(y_obs, float).ravel()[topo.perm[g]] - m0[topo.perm[g]]
        Ni = np.linalg.inv(N)
        mu, Sg = np.asarray(y_obs, float).ravel()[topo.perm[g]] - D @ Ni @ rho, D @ Ni @ D
        lp = -.5 * (2.0 * np.log(rp[g]).sum() - np.linalg.slogdet(N)[1] + rho @ Ni @ rho + len(g) * LOG_2PI)
        e_m = max(e_m, np.abs(by_leaf[0][g] - mu).max() / ymax)
        e_v = max(e_v, (np.abs(by_leaf[1][g] - np.diag(Sg)) / np.diag(Sg)).max())
        e_l = max(e_l, float(_rel1(by_leaf[3][i], lp)))
    print("g32 noise vector by leaf: 4 leaves against the dense identity on cov_apply's columns: mean %.2e, var %.2e, group lpd %.2e" % (e_m, e_v, e_l))
    assert max(e_m, e_v, e_l) <= _tol("g32")
    assert by_row[4][6] == by_leaf[4][6] and by_row[4][7] == by_leaf[4][7]      # tr K^-1 and alpha^T alpha do not depend on the groups
    pl.close()


# ---- 5. after a Laplace fit -------------------------------------------------------------------------------------------------------------
def test_after_fit_laplace_the_pseudo_observations_are_scored(hip):
    import _laplace as LP
    import test_gpu_likelihood_masks as MK
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, ref = LP.t16_fit(LP.POISSON)
    pl = MK._plan(hip, topo, locs, y)
    pl.fit_laplace(LP.NAMES[LP.POISSON], z, aux=aux, offset=offset, tol=1e-10)
    got = [pl.cv(leaf=leaf) for leaf in (False, True)]
    t, r = pl.buffer(11), pl.buffer(10)
    rows = (topo.perm >= 0) & np.asarray(topo.in_leaf, dtype=bool)
    tc, rc = np.full(topo.N, np.nan), np.full(topo.N, 1.0)
    tc[topo.perm[rows]], rc[topo.perm[rows]] = t[rows], r[rows]
    rc[~np.isfinite(tc)] = 1.0
    s = MK._spec()
    fresh = hip.HipPlan(topo, 0)
    fresh.set_locs(locs); fresh.set_obs(tc.reshape(-1, 1), rc); fresh.set_kernel(s.kind, s.l, s.sig, s.scale)
    for leaf in (False, True):
        want = fresh.cv(leaf=leaf)
        assert want[4][0] > 0
        for a, b in zip(got[leaf], want):
            assert np.array_equal(a, b, equal_nan=True)
    fresh.close(); pl.close()


# ---- 6. purity and state ----------------------------------------------------------------------------------------------------------------
def test_same_bits_whatever_the_chunks_and_the_calls_before(hip):
    topo, locs, y_obs, spec, R = GC._shape_tree("grid48_r20")
    pl = GC._plan(hip, topo, locs, y_obs, R, spec)
    lik0, (m0, v0) = pl.likelihood(), pl.predict()
    opts = {k: pl.get_option(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21)}
    first = [pl.cv(leaf=leaf) for leaf in (False, True)]
    assert pl.likelihood() == lik0
    m1, v1 = pl.predict()
    assert np.array_equal(m1, m0) and np.array_equal(v1, v0)
    assert {k: pl.get_option(k) for k in opts} == opts

    def same(tag):
        for leaf in (False, True):
            got = pl.cv(leaf=leaf)
            assert GC._factor_launches(pl) == 0, tag              # no kernel of a pass
            for a, b in zip(got, first[leaf]):
                assert np.array_equal(a, b, equal_nan=True), tag
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
    X = np.asarray(locs, float).reshape(topo.N, -1)
    pl.predict_sites(X[topo.perm[rows]], CV.leaf_of_rows(topo)[rows])
    same("after predict_sites")
    assert pl.likelihood() == lik0
    m1, v1 = pl.predict()
    assert np.array_equal(m1, m0) and np.array_equal(v1, v0)
    pl.set_option(1, 1)                                           # MRA_OPT_KERNEL_TIMING
    pl.cv(leaf=True)
    ms = pl.buffer(12)
    assert ms.shape == (9,) and np.all(ms >= 0.0) and ms[4] > 0.0 and ms[5] > 0.0
    pl.close()


def test_the_first_call_runs_its_own_pass(hip):
    cs = K.load_case("g32")
    pl = GC._plan(hip, cs["topo"], cs["locs"], cs["y_obs"], R_CV, cs["spec"], run=False)
    a = pl.cv()
    assert GC._factor_launches(pl) > 0
    b = pl.cv()
    assert GC._factor_launches(pl) == 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    pl.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    from pymra_amd.plan import MraError
    import pymra_amd.MRATools as mt
    cs = K.load_case("g32")
    topo, locs, spec, y_obs = cs["topo"], cs["locs"], cs["spec"], cs["y_obs"]
    pl = hip.HipPlan(topo, 0)
    for step in ("nothing", "locs", "kernel"):
        if step == "locs":
            pl.set_locs(locs)
        elif step == "kernel":
            pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
        with pytest.raises(MraError) as e:
            pl.cv()
        assert e.value.code == -4 and "mra_cv needs" in str(e.value), step      # MRA_ERR_STATE before set_locs / set_kernel / set_obs
    pl.set_obs(y_obs, R_CV)
    good = pl.cv(leaf=True)
    info = np.zeros(8)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def raw(flags=0, inf=info):
        return pl.lib.mra_cv(pl._h, flags, None, None, None, None, p(inf))

    def message():
        return pl.lib.mra_last_error(pl._h).decode()
    pl.lib.mra_last_error.restype = C.c_char_p
    assert raw() == 0 and raw(1) == 0 and info[0] == good[4][0]            # every output but info may be NULL
    assert raw(2) == -1 and "unknown mra_cv flags" in message()
    assert raw(inf=None) == -1 and "info is NULL" in message()
    with pytest.raises(MraError) as e:                                     # a scalar R = 0 is MRA_ERR_INVALID at set_obs already
        pl.set_obs(y_obs, 0.0)
    assert e.value.code == -1
    assert raw(1) == 0 and info[0] == good[4][0]                           # ... and the plan keeps the R it had
    rv = np.full(topo.N, R_CV)                                             # a vector may hold a 0: one observed row is enough
    rv[np.nonzero(np.isfinite(np.asarray(y_obs, float).ravel()))[0][5]] = 0.0
    pl.set_noise(rv)
    for flags in (0, 1):
        assert raw(flags) == -1 and "noise variance is 0 at observed padded row" in message()
    pl.set_noise(None)
    pl.set_obs(np.full((topo.N, 1), np.nan), R_CV)                         # no observed row: MRA_OK, info all zero
    info[:] = 7.0
    none = pl.cv()
    assert raw() == 0 and np.all(info == 0.0)
    assert np.all(np.isnan(none[0])) and np.all(np.isnan(none[3])) and np.all(none[4] == 0.0)
    pl.set_obs(y_obs, R_CV)
    again = pl.cv(leaf=True)                                               # the plan is still usable, and gives the same bits
    for a, b in zip(again, good):
        assert np.array_equal(a, b, equal_nan=True)
    pl.set_reduce_level(0)
    with pytest.raises(MraError) as e:
        pl.cv()
    assert e.value.code == -1 and "sharded" in str(e.value)
    pl.close()
    from pymra_amd import MRATree
    np.random.seed(1)
    n = 16
    l2 = mt.genLocations2d(Nx=n, Ny=n)
    y = np.random.normal(size=(n * n, 1))
    tree = MRATree(l2, 16, lambda a, b=np.array([]): np.exp(-np.abs(mt.dist(a, b)) / 0.3), y, 1e-2, M=1, J=4, verbose=False)      # opaque callable: host cov
    with pytest.raises(NotImplementedError):
        tree.crossValidate()
    with pytest.raises(MraError) as e:
        tree.plan.cv()
    assert e.value.code == -1 and "MRA_KERNEL_HOST" in str(e.value)


def test_a_leaf_above_the_cap_is_refused_by_leaf_only(hip):
    import pymra_amd.MRATools as mt
    from pymra_amd.plan import MraError
    from pymra_amd.topology import build_topology
    locs = mt.genLocations2d(Nx=72, Ny=72)                                 # one leaf of 5184 rows, all observed: above the cap of 4096
    topo = build_topology(locs, 16, 0, 4)
    assert topo.n_nodes == 1
    y = np.random.default_rng(1).standard_normal((len(locs), 1))
    pl = GC._plan(hip, topo, locs, y, 0.5, mt.KernelSpec(mt.KIND_EXP, 0.05), run=False)
    with pytest.raises(MraError) as e:
        pl.cv(leaf=True)
    assert e.value.code == -1 and "MRA_SAMPLE_SITES_LEAF_MAX" in str(e.value)
    pl.close()


# ---- 8. through MRATree -----------------------------------------------------------------------------------------------------------------
def test_mratree_crossValidate(hip):
    import pymra_amd.MRATools as mt
    from pymra_amd import MRATree
    np.random.seed(3)
    cov = lambda a, b=np.array([]): mt.Matern32(a, b, l=0.3, sig=1.0)          # noqa: E731
    n = 32
    locs = mt.genLocations2d(Nx=n, Ny=n)
    rng = np.random.default_rng(2)
    y = np.where(rng.random(n * n) < 0.4, rng.standard_normal(n * n), np.nan).reshape(-1, 1)
    tree = MRATree(locs, 16, cov, y, R_CV, M=2, J=4, verbose=False)
    lik0 = float(tree.getLikelihood()[0, 0])
    t = tree.topology
    S = TS.SiteState(t, locs, tree.kernel, y, R_CV)
    rows = t.perm >= 0
    for kind in ("loo", "leaf"):
        res = tree.crossValidate(kind)
        want = CV.tree_cv(S, kind == "leaf")
        assert res.mean.shape == res.sd.shape == res.z.shape == res.lpd.shape == (n * n,)
        assert np.array_equal(np.isnan(res.mean), np.isnan(y.ravel()))         # NaN exactly where nothing is observed
        for got, w in ((res.mean, want[0]), (res.sd ** 2, want[1]), (res.lpd, want[2])):
            wc = np.full(n * n, np.nan)
            wc[t.perm[rows]] = w[rows]                                         # the caller's row order
            ok = ~np.isnan(wc)
            assert np.array_equal(ok, ~np.isnan(got))
            assert (np.abs(got[ok] - wc[ok]) / np.maximum(1.0, np.abs(wc[ok]))).max() <= _tol()
        ok = ~np.isnan(res.z)
        assert np.abs(res.z[ok] - (y.ravel()[ok] - res.mean[ok]) / res.sd[ok]).max() <= 1e-12 * np.abs(res.z[ok]).max()
        assert sorted(res.leaf_lpd) == [int(i) for i in np.nonzero(~np.isnan(want[3]))[0]]
        assert abs(sum(res.leaf_lpd.values()) - res.score) <= 1e-12 * abs(res.score)
        assert res.n == int(np.isfinite(y).sum()) and res.leverage_max <= H_MAX
        d = want[4][6] - want[4][7]
        print("crossValidate(%s): score %.6f (twin %.6f), dlik_dR %.6f (twin %.6f), max h %.4f" % (kind, res.score, want[4][2], res.dlik_dR, d, res.leverage_max))
        assert abs(res.score - want[4][2]) <= _tol() * max(1.0, abs(want[4][2]))
        assert abs(res.dlik_dR - d) <= _tol() * max(abs(want[4][6]), abs(want[4][7]))
    # dlik_dR is the derivative of getLikelihood() by the nugget: a central difference of two refits
    eps = 1e-6
    np.random.seed(3)
    lp = float(MRATree(locs, 16, cov, y, R_CV + eps, M=2, J=4, verbose=False).getLikelihood()[0, 0])
    np.random.seed(3)
    lm = float(MRATree(locs, 16, cov, y, R_CV - eps, M=2, J=4, verbose=False).getLikelihood()[0, 0])
    fd = (lp - lm) / (2.0 * eps)
    print("dlik_dR %.6f, central difference of getLikelihood() %.6f" % (res.dlik_dR, fd))
    assert abs(res.dlik_dR - fd) <= 1e-5 * abs(fd)
    assert float(tree.getLikelihood()[0, 0]) == lik0
    with pytest.raises(ValueError):
        tree.crossValidate("kfold")


# ---- 9. BASELINE config 3 ---------------------------------------------------------------------------------------------------------------
def test_c3(hip):
    """1024^2, M = 6, half observed: by leaf on the whole tree, 8 seeded leaves against refits on the device; by row, 256 seeded rows
    against the per-row formula on predict().  Bounds 1e-8 (mean) and 1e-9 relative (variance), as tests/test_gpu_sites.py
    test_own_rows_at_c3; if max v / R exceeds 0.98 they are scaled by (0.02 / (1 - h))^2, what the identity loses there."""
    import bench
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    c = bench.CONFIGS["c3"]
    locs, y_obs = bench.make_inputs(c)
    topo = build_topology(locs, c["r"], c["M"], c["J"])
    spec = mt.KernelSpec(mt.KIND_MATERN32, c["l"], c["sig"])
    pl = GC._plan(hip, topo, locs, y_obs, c["R"], spec)
    obs_p = np.isfinite(np.asarray(y_obs, float).ravel())[topo.src] & (topo.perm >= 0)
    by_leaf = pl.cv(leaf=True)
    h = by_leaf[4][5]
    scale = max(1.0, (0.02 / (1.0 - h)) ** 2)
    print("c3: %d rows, %d groups, score %.3f, max h %.6f, bounds scaled by %.2f" % (by_leaf[4][0], by_leaf[4][1], by_leaf[4][2], h, scale))
    assert by_leaf[4][0] == int(obs_p.sum())
    rng = np.random.default_rng(1)
    rows = np.sort(rng.choice(np.nonzero(obs_p)[0], 256, replace=False))
    _loo_against_predict(pl, topo, y_obs, np.full(topo.P, c["R"]), rows, "c3", 1e-8 * scale, 1e-9 * scale)
    pl.close()
    leaves = [int(i) for i in rng.choice(_leaves(topo), 8, replace=False)]
    _leaves_against_refits(hip, by_leaf, topo, locs, y_obs, c["R"], spec, leaves, "c3", 1e-8 * scale, 1e-9 * scale, 1e-8 * scale)
