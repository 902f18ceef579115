"""The NumPy restatement of mra_cv_trend (tests/_treecv_trend.py) against brute force, without a GPU: every group in turn deleted,
generalised least squares fitted on the rest against prior Sigma[o, o] + D (the reference's own per-node blocks, tests/golden/*_nodes.npz),
the group kriged universally (refit) or around the full fit's beta^ (fixed).

Cases: those of tests/test_cv_cpu.py (g32, c1, kat3 and u3's geometry at R = 1e-2), with p = 1 (an intercept) and p = 3 (an intercept
and two seeded normal columns, tests/_treecv_trend.design), both modes, both groupings.  Leave-out coverage: every leaf; every observed
row of c1 and kat3, 40 seeded rows of g32 and u3.

A condition, checked here: every leave-out keeps X at full column rank, and the largest leverage the refit mode divides by,
max (v + |w|^2) / r, stays at or below the 0.972 of section 18's cases.

Measures (tests/test_cv_cpu.py's): mean |delta| / max|y|; variance relative to the largest variance of the group; lpd and score
|delta| / max(1, |value|).

Bound.  TOL = 100 x the largest error seen when the twin was first checked against the brute force.  Seen then, the largest over p = 1
and 3 and the two modes (mean, variance, lpd, score; the largest leverage):
    g32    by row 5.7e-13, 1.2e-12, 1.5e-12, -          by leaf 3.1e-11, 3.3e-11, 1.1e-12, 1.2e-13     0.971961
    c1     by row 1.6e-14, 5.2e-13, 2.6e-13, 1.9e-14    by leaf 1.4e-14, 4.2e-13, 3.6e-13, 2.5e-14     0.799920
    kat3   by row 1.1e-13, 7.9e-13, 4.8e-13, 1.4e-13    by leaf 4.3e-13, 6.8e-13, 9.6e-13, 2.9e-13     0.961388
    u3     by row 1.4e-13, 6.9e-13, 6.0e-13, -          by leaf 4.5e-12, 1.5e-11, 6.3e-12, 3.5e-12     0.969710
The largest is 3.3e-11 (g32's variances by leaf, as in section 18: the trend changes them in the third digit), so TOL = 3.3e-9.
tr K^-1, tr P and |P y|^2 against the dense K^-1 and P (relative): at most 4.7e-14.  Fixed mode against tree_cv on y - X beta^: at most
6.2e-12 (g32's lpd by leaf).  info[10] and info[11] against central differences of dense fits at R +- 1e-6, relative to
max(tr K^-1, |P y|^2): at most 5.2e-9 (c1) - held to TOL_FD = 1e-7, the difference quotient's own accuracy: the two profile values
(up to 1e3) carry about 1e-13 of themselves, 1e-10, which the division by 2e-6 turns into 5e-5, over a scale of at least 500.
tests/_treecv_trend.TWIN_ERR keeps the largest figure of each case for the device tests."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _cases as K
import _sampling as SM
import _treecv as CV
import _treecv_trend as CT
import _treesites as TS
import _treetrend as TT

CASES = ["g32", "c1", "kat3", "u3"]
PS = [1, 3]
R_CV = 1e-2
H_MAX = 0.972
TOL = 3.3e-9
TOL_FD = 1e-7                     # central differences at a step of 1e-6: held to the difference quotient's accuracy (above)
LOO_ALL = ("c1", "kat3")


@functools.lru_cache(maxsize=None)
def _state(name):
    cs = K.load_case(name)
    return cs, TS.SiteState(cs["topo"], cs["locs"], cs["spec"], cs["y_obs"], R_CV)


@functools.lru_cache(maxsize=None)
def _sigma(name):
    return SM.golden_prior_sigma(name, _state(name)[0]["topo"])


@functools.lru_cache(maxsize=None)
def _fit(name, p):
    cs, S = _state(name)
    X = CT.design(cs["locs"], p)
    return X, TT.tree_trend(cs["topo"], cs["locs"], cs["spec"], cs["y_obs"], R_CV, X)


@functools.lru_cache(maxsize=None)
def _twin(name, p, leaf, refit):
    X, fit = _fit(name, p)
    return CT.tree_cv_trend(_state(name)[1], X, leaf, refit, fit=fit)


def rel1(a, b):
    return abs(a - b) / max(1.0, abs(b))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name", CASES)
def test_every_leave_out_keeps_full_rank_and_the_leverage_stays_in_the_regime(name, p):
    cs, S = _state(name)
    X, _ = _fit(name, p)
    rows, lf = CV.scored_rows(S)
    Xo = X[cs["topo"].perm[rows]]
    Q, _ = np.linalg.qr(Xo)
    H = Q @ Q.T                                   # the hat matrix of ordinary least squares: X without G has full rank iff I - H_GG is regular
    worst = max(H.diagonal().max(), max(np.linalg.eigvalsh(H[np.ix_(lf == i, lf == i)]).max() for i in np.unique(lf)))
    lev = max(_twin(name, p, leaf, True)[4][5] for leaf in (False, True))
    print("%s p = %d: largest eigenvalue of a group's hat block %.4f, max (v + |w|^2) / r %.6f" % (name, p, worst, lev))
    assert np.linalg.matrix_rank(Xo) == p and worst <= 0.9
    assert lev <= H_MAX, "outside the regime the bound was measured in"
    assert _twin(name, p, False, False)[4][5] <= lev


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name", CASES)
def test_leave_one_out_is_the_fit_without_the_row(name, p):
    cs, S = _state(name)
    topo = cs["topo"]
    X, fit = _fit(name, p)
    rows, _ = CV.scored_rows(S)
    pick = rows if name in LOO_ALL else np.sort(np.random.default_rng(11).choice(rows, 40, replace=False))
    ymax = np.abs(S.y[topo.perm[rows]]).max()
    for refit in (True, False):
        mean, var, lpd, group, info = _twin(name, p, False, refit)
        e_m = e_v = e_l = 0.0
        score = 0.0
        for row in pick:
            mu, Sg, lp = CT.brute_group_trend(_sigma(name), S, X, [row], beta_fixed=None if refit else fit["beta"])
            e_m = max(e_m, abs(mean[row] - mu[0]) / ymax)
            e_v = max(e_v, abs(var[row] - Sg[0, 0]) / Sg[0, 0])
            e_l = max(e_l, rel1(lpd[row], lp))
            score += lp
        e_s = rel1(info[2], score) if len(pick) == len(rows) else 0.0
        print("%s p = %d %s by row: %d of %d rows: mean err %.2e, var err %.2e, lpd err %.2e, score err %.2e (max leverage %.6f)"
              % (name, p, "refit" if refit else "fixed", len(pick), len(rows), e_m, e_v, e_l, e_s, info[5]))
        assert max(e_m, e_v, e_l, e_s) <= TOL


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name", CASES)
def test_leave_a_leaf_out_is_the_fit_without_the_leaf(name, p):
    cs, S = _state(name)
    topo = cs["topo"]
    X, fit = _fit(name, p)
    rows, lf = CV.scored_rows(S)
    ymax = np.abs(S.y[topo.perm[rows]]).max()
    for refit in (True, False):
        mean, var, lpd, group, info = _twin(name, p, True, refit)
        e_m = e_v = e_l = 0.0
        score = 0.0
        n_groups = 0
        for i in np.unique(lf):
            g = rows[lf == i]
            mu, Sg, lp = CT.brute_group_trend(_sigma(name), S, X, g, beta_fixed=None if refit else fit["beta"])
            e_m = max(e_m, np.abs(mean[g] - mu).max() / ymax)
            e_v = max(e_v, np.abs(var[g] - np.diag(Sg)).max() / np.diag(Sg).max())
            e_l = max(e_l, rel1(group[i], lp))
            score += lp
            n_groups += 1
        e_s = rel1(info[2], score)
        print("%s p = %d %s by leaf: %d groups: mean err %.2e, var err %.2e, group lpd err %.2e, score err %.2e (max leverage %.6f)"
              % (name, p, "refit" if refit else "fixed", n_groups, e_m, e_v, e_l, e_s, info[5]))
        assert info[1] == n_groups and info[9] == p
        assert max(e_m, e_v, e_l, e_s) <= TOL


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name", CASES)
def test_the_by_products_are_the_dense_inverse_and_the_derivatives(name, p):
    cs, S = _state(name)
    X, _ = _fit(name, p)
    D = CT.dense_fit(_sigma(name), S, X)
    trK, trP, py = np.trace(D["Ki"]), np.trace(D["P"]), D["P"] @ D["y"]
    h = 1e-6
    up, dn = CT.dense_fit(_sigma(name), S, X, h), CT.dense_fit(_sigma(name), S, X, -h)
    d_prof, d_reml = (up["profile"] - dn["profile"]) / (2 * h), (up["reml"] - dn["reml"]) / (2 * h)
    for leaf in (False, True):
        for refit in (True, False):
            info = _twin(name, p, leaf, refit)[4]
            e = [abs(info[6] - trK) / trK, abs(info[8] - trP) / trP, abs(info[7] - py @ py) / (py @ py)]
            scale = max(abs(info[6]), abs(info[7]))
            f = [abs(info[10] - d_prof) / scale, abs(info[11] - d_reml) / scale]
            print("%s p = %d: tr K^-1 %.6f (rel err %.2e), tr P %.6f (%.2e), |Py|^2 %.6f (%.2e); d profile / dR %.6f (%.2e), d REML / dR %.6f (%.2e)"
                  % (name, p, trK, e[0], trP, e[1], py @ py, e[2], d_prof, f[0], d_reml, f[1]))
            assert max(e) <= TOL
            assert info[10] == info[6] - info[7] and info[11] == info[8] - info[7]
            assert max(f) <= TOL_FD


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name", CASES)
def test_fixed_mode_is_the_plain_cross_validation_of_the_detrended_data(name, p):
    cs, S = _state(name)
    topo = cs["topo"]
    X, fit = _fit(name, p)
    trend = X @ fit["beta"]
    S0 = TS.SiteState(topo, cs["locs"], cs["spec"], np.asarray(cs["y_obs"], float).ravel() - trend, R_CV)
    rows, _ = CV.scored_rows(S)
    ymax = np.abs(S.y[topo.perm[rows]]).max()
    for leaf in (False, True):
        want, got = CV.tree_cv(S0, leaf), _twin(name, p, leaf, False)
        gk = ~np.isnan(want[3])
        e = [np.abs(got[0][rows] - want[0][rows] - trend[topo.perm[rows]]).max() / ymax, (np.abs(got[1][rows] - want[1][rows]) / want[1][rows]).max(),
             (np.abs(got[2][rows] - want[2][rows]) / np.maximum(1.0, np.abs(want[2][rows]))).max(),
             (np.abs(got[3][gk] - want[3][gk]) / np.maximum(1.0, np.abs(want[3][gk]))).max(),
             max(rel1(got[4][k], want[4][k]) for k in (2, 3, 4)), max(abs(got[4][k] - want[4][k]) / abs(want[4][k]) for k in (5, 6, 7))]
        print("%s p = %d %s: fixed mode against tree_cv on y - X beta^: mean %.2e, var %.2e, lpd %.2e, group lpd %.2e, sums %.2e, by-products %.2e"
              % (name, p, "by leaf" if leaf else "by row", *e))
        assert np.array_equal(np.isnan(got[3]), np.isnan(want[3])) and got[4][0] == want[4][0] and got[4][1] == want[4][1]
        assert max(e) <= TOL


def test_the_dense_form_with_a_noise_vector_agrees_at_a_constant_vector():
    """tests/_treecv_trend.dense_cv_trend (D = diag(r), dense algebra on K and P alone) is what the device's noise-vector results are
    held to: with r = R everywhere it must be the tree twin, within the bound of this file."""
    import _noise as NZ
    name, p = "g32", 3
    cs, S = _state(name)
    topo = cs["topo"]
    X, _ = _fit(name, p)
    Sigma = NZ.prior_cov(topo, cs["locs"], cs["spec"], cs["y_obs"])
    ymax = np.nanmax(np.abs(np.asarray(cs["y_obs"], float)))
    for leaf in (False, True):
        for refit in (True, False):
            want, got = _twin(name, p, leaf, refit), CT.dense_cv_trend(topo, Sigma, cs["y_obs"], np.full(topo.N, R_CV), X, leaf, refit)
            ok, gk = ~np.isnan(want[0]), ~np.isnan(want[3])
            assert np.array_equal(ok, ~np.isnan(got[0])) and np.array_equal(gk, ~np.isnan(got[3]))
            e = [np.abs(got[0][ok] - want[0][ok]).max() / ymax, (np.abs(got[1][ok] - want[1][ok]) / want[1][ok]).max(),
                 (np.abs(got[2][ok] - want[2][ok]) / np.maximum(1.0, np.abs(want[2][ok]))).max(),
                 (np.abs(got[3][gk] - want[3][gk]) / np.maximum(1.0, np.abs(want[3][gk]))).max(),
                 max(rel1(got[4][k], want[4][k]) for k in (2, 3, 4)), max(abs(got[4][k] - want[4][k]) / abs(want[4][k]) for k in (5, 6, 7, 8))]
            print("%s %s %s: dense form against the tree twin: mean %.2e, var %.2e, lpd %.2e, group lpd %.2e, sums %.2e, by-products %.2e"
                  % (name, "by leaf" if leaf else "by row", "refit" if refit else "fixed", *e))
            assert max(e) <= TOL


def test_a_leaf_that_carries_all_the_information_on_a_covariate_has_a_singular_block():
    """The indicator of one leaf as a covariate: without that leaf the column is 0 and beta cannot be estimated again, so the leaf's
    N~_G is singular (its smallest eigenvalue is rounding, relative to r), while the plain N_G and every other leaf's N~_G are not."""
    cs, S = _state("g32")
    topo = cs["topo"]
    rows, lf = CV.scored_rows(S)
    node = int(np.unique(lf)[3])
    ind = np.zeros(topo.N)
    ind[topo.perm[rows[lf == node]]] = 1.0
    X = np.column_stack([np.ones(topo.N), ind])
    fit = TT.tree_trend(topo, cs["locs"], cs["spec"], cs["y_obs"], R_CV, X)
    lo = {int(i): np.linalg.eigvalsh(CT.ntilde(S, X, int(i), True, fit=fit)).min() / R_CV for i in np.unique(lf)}
    plain = np.linalg.eigvalsh(CT.ntilde(S, X, node, False, fit=fit)).min() / R_CV
    others = min(v for i, v in lo.items() if i != node)
    print("smallest eigenvalue of N~_G / r: the leaf of the indicator %.2e, the other leaves >= %.4f; of its plain N_G / r %.4f" % (lo[node], others, plain))
    # (a block's smallest eigenvalue is below 1 - max h, section 18: 1.6e-3 at the least here, against rounding)
    assert abs(lo[node]) <= 1e-9
    assert others >= 1e-4 and plain >= 1e-4


def test_cv_trend_surface_is_exported():
    from pymra_amd import plan
    from pymra_amd.MRATree import MRATree
    import inspect
    assert "mra_cv_trend" in plan.EXPORTS and plan.MRA_CV_TREND_REFIT == 2 and plan.MRA_CV_LEAF == 1
    assert callable(plan.HipPlan.cv_trend)
    assert list(inspect.signature(plan.HipPlan.cv_trend).parameters) == ["self", "leaf", "refit"]
    assert list(inspect.signature(MRATree.crossValidate).parameters) == ["self", "kind", "trend"]
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    assert "#define MRA_CV_TREND_REFIT 2u" in hdr
    assert ("int mra_cv_trend(mra_plan *plan, uint32_t flags, double *mean_perm, double *var_perm, double *lpd_perm, double *group_lpd, "
            "double *info /* 12 */);") in hdr
    assert "int mra_cv(mra_plan *plan, uint32_t flags, double *mean_perm, double *var_perm, double *lpd_perm, double *group_lpd, double *info);" in hdr


def test_the_library_exports_the_entry_point(built_library):
    from pymra_amd import plan
    lib = plan.load_library()
    assert hasattr(lib, "mra_cv_trend")


def test_refusals_and_their_order_on_a_dry_run_plan(built_library, tmp_path):
    """The refusals of mra_cv_trend are host checks made before anything is launched, and a MRA_HOST_DRYRUN plan reaches all of them;
    only then does it say that it cannot run.  The order: the plan (flags, set_* missing, MRA_KERNEL_HOST, sharded), the missing
    trend, a NULL info, a zero noise variance at an observed row; mra_cv itself still refuses flag 2."""
    child = tmp_path / "child.py"
    child.write_text(r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["MRA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRA_ROOT"], "tests"))
import _cases as K
import pymra_amd.MRATools as mt
from pymra_amd import plan as P
cs = K.load_case("g64")
topo = cs["topo"]
N, Pn = int(topo.N), int(topo.P)
WHO = "mra_cv_trend"

def make(obs=True, kernel=True):
    pl = P.HipPlan(topo, 0)
    pl.set_locs(cs["locs"])
    if obs:
        pl.set_obs(cs["y_obs"], cs["c"]["R"])
    if kernel:
        pl.set_kernel(mt.KIND_EXP, 0.3, 1.0, 1.0)
    return pl

def call(pl, flags=0, info=True, fn="mra_cv_trend"):
    m, v, l, g, i = np.full(Pn, 7.0), np.full(Pn, 7.0), np.full(Pn, 7.0), np.full(pl.info()["n_nodes"], 7.0), np.full(12, 7.0)
    rc = getattr(pl.lib, fn)(pl._h, flags, P._ptr(m), P._ptr(v), P._ptr(l), P._ptr(g), P._ptr(i) if info else None)
    assert all(np.all(a == 7.0) for a in (m, v, l, g, i))     # a refused call writes nothing
    return rc, pl.lib.mra_last_error(pl._h).decode()

def expect(got, code, text):
    assert got[0] == code and text in got[1], (got, code, text)

pl = make()
expect(call(pl, flags=4, info=False), -1, "unknown " + WHO + " flags")
expect(call(pl, flags=8 | 3, info=False), -1, "unknown " + WHO + " flags")
bare = make(obs=False)
expect(call(bare, info=False), -4, WHO + " needs set_obs first")
bare.close()
for flags in (0, 1, 2, 3):
    expect(call(pl, flags=flags, info=False), -4, WHO + " needs mra_plan_set_trend first")       # no trend: before the arguments
host = make(kernel=False)
host.set_kernel_host()
expect(call(host, info=False), -1, WHO + ": MRA_KERNEL_HOST plans cannot cross-validate")          # the plan's kind before the missing trend
host.close()
pl.set_trend(np.ones((N, 2)))
pl.set_reduce_level(0)
expect(call(pl, info=False), -1, WHO + ": sharded plans cannot cross-validate")
pl.close()
pl = make()
pl.set_trend(np.ones((N, 2)))
expect(call(pl, flags=3, info=False), -1, WHO + ": info is NULL")
r = np.full(N, float(cs["c"]["R"]))
seen = np.nonzero(np.isfinite(np.asarray(cs["y_obs"], float).ravel()))[0]
r[seen[5]] = 0.0
pl.set_noise(r)
expect(call(pl, flags=2), -1, WHO + ": the noise variance is 0 at observed padded row")
expect(call(pl, flags=2, info=False), -1, WHO + ": info is NULL")
pl.set_noise(None)
for flags in (0, 1, 2, 3):
    expect(call(pl, flags=flags), -4, "MRA_HOST_DRYRUN plan: built in host memory for the sanitizers, it cannot run")
assert pl.info()["trend_p"] == 2
# mra_cv is as it was: flag 2 is not its flag, and it refuses the dry-run plan before it looks at anything
expect(call(pl, flags=2, fn="mra_cv"), -4, "MRA_HOST_DRYRUN plan")
pl.close()
print("CV_TREND_REFUSALS_OK")
''')
    env = dict(os.environ, MRA_ROOT=K.ROOT, MRA_HOST_DRYRUN="1")
    res = subprocess.run([sys.executable, str(child)], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "CV_TREND_REFUSALS_OK" in res.stdout, (res.stdout + res.stderr)[-3000:]
