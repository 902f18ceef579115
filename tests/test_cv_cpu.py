"""The NumPy restatement of mra_cv (tests/_treecv.py) against brute force: every group in turn set to NaN, the level-wise oracle run
again on the same topology, the group's predictive mean and covariance read off the refit.  No GPU.

Cases: g32, c1, kat3 at their own R = 1e-2, and u3's geometry at R = 1e-2 (at its own 1e-6 max v / R is 0.999997: float64 loses
eps / (1 - h)^2 there, whatever computes the identity).  max h <= 0.98 is a condition of the test.  Leave-out coverage: every leaf by
leaf; every observed row of c1 and kat3 and 40 seeded rows of g32 and u3 one by one (c1 and kat3 have leaves with 0 - 3 observations:
empty leaves and one-row groups).

Measures: mean |delta| / max|y|; variance (the whole block S_G by leaf) relative to the largest variance of the group; lpd and score
|delta| / max(1, |value|).

Bound.  TOL = 100 x the largest error seen when the twin was first checked against the brute force on these four cases, the rule
tests/test_sites_cpu.py used for its variance bound.  Seen then (mean, variance, lpd, score; max h):
    g32    by row 5.6e-13, 1.2e-12, 1.5e-12, -          by leaf 3.0e-11, 3.3e-11, 1.1e-12, 1.0e-13     max h 0.972
    c1     by row 1.1e-14, 4.3e-14, 9.0e-14, 3.7e-15    by leaf 1.1e-14, 1.4e-13, 2.2e-13, 5.7e-15     max h 0.793
    kat3   by row 1.2e-13, 7.7e-13, 5.4e-13, 1.4e-13    by leaf 4.0e-13, 6.5e-13, 9.6e-13, 3.0e-13     max h 0.960
    u3     by row 1.5e-13, 6.9e-13, 6.8e-13, -          by leaf 2.4e-12, 1.4e-11, 4.3e-12, 4.4e-13     max h 0.968
The largest is 3.3e-11 (g32's variances by leaf: a group of up to 32 rows is conditioned by the smallest eigenvalue of N_G / R, which
is below 1 - max h), so TOL = 3.3e-9.  tr K^-1 and alpha^T alpha against the dense K^-1 (relative): at most 4.9e-14 over the four cases.
tests/_treecv.TWIN_ERR keeps the largest figure of each case for the device tests."""
import functools

import numpy as np
import pytest

import _cases as K
import _sampling as SM
import _treecv as CV
import _treesites as TS

CASES = ["g32", "c1", "kat3", "u3"]
R_CV = 1e-2
H_MAX = 0.98
TOL = 3.3e-9
LOO_ALL = ("c1", "kat3")          # every observed row; the others: 40 seeded rows


@functools.lru_cache(maxsize=None)
def _state(name):
    cs = K.load_case(name)
    return cs, TS.SiteState(cs["topo"], cs["locs"], cs["spec"], cs["y_obs"], R_CV)


@functools.lru_cache(maxsize=None)
def _twin(name, leaf):
    return CV.tree_cv(_state(name)[1], leaf)


def rel1(a, b):
    return abs(a - b) / max(1.0, abs(b))


@pytest.mark.parametrize("name", CASES)
def test_leave_one_out_is_the_refit_without_the_row(name):
    cs, S = _state(name)
    topo = cs["topo"]
    mean, var, lpd, group, info = _twin(name, False)
    assert info[5] <= H_MAX, "outside the regime the bound was measured in"
    p, _ = CV.scored_rows(S)
    pick = p if name in LOO_ALL else np.sort(np.random.default_rng(11).choice(p, 40, replace=False))
    ymax = np.abs(S.y[topo.perm[p]]).max()
    e_m = e_v = e_l = 0.0
    score = 0.0
    for row in pick:
        mu, Sg, lp = CV.brute_group(cs, R_CV, [row])
        e_m = max(e_m, abs(mean[row] - mu[0]) / ymax)
        e_v = max(e_v, abs(var[row] - Sg[0, 0]) / Sg[0, 0])
        e_l = max(e_l, rel1(lpd[row], lp))
        score += lp
    e_s = rel1(info[2], score) if len(pick) == len(p) else 0.0
    print("%s by row: %d of %d rows refitted: mean err %.2e, var err %.2e, lpd err %.2e, score err %.2e (max h %.6f)"
          % (name, len(pick), len(p), e_m, e_v, e_l, e_s, info[5]))
    assert max(e_m, e_v, e_l, e_s) <= TOL


@pytest.mark.parametrize("name", CASES)
def test_leave_a_leaf_out_is_the_refit_without_the_leaf(name):
    cs, S = _state(name)
    topo = cs["topo"]
    mean, var, lpd, group, info = _twin(name, True)
    assert info[5] <= H_MAX, "outside the regime the bound was measured in"
    p, lf = CV.scored_rows(S)
    ymax = np.abs(S.y[topo.perm[p]]).max()
    e_m = e_v = e_l = 0.0
    score = 0.0
    sizes = []
    for i in np.unique(lf):
        rows = p[lf == i]
        sizes.append(len(rows))
        mu, Sg, lp = CV.brute_group(cs, R_CV, rows)
        e_m = max(e_m, np.abs(mean[rows] - mu).max() / ymax)
        e_v = max(e_v, np.abs(var[rows] - np.diag(Sg)).max() / np.diag(Sg).max())
        e_l = max(e_l, rel1(group[i], lp))
        score += lp
    e_s = rel1(info[2], score)
    print("%s by leaf: %d groups of %d to %d rows: mean err %.2e, var err %.2e, group lpd err %.2e, score err %.2e (max h %.6f)"
          % (name, len(sizes), min(sizes), max(sizes), e_m, e_v, e_l, e_s, info[5]))
    assert info[1] == len(sizes)
    assert max(e_m, e_v, e_l, e_s) <= TOL


@pytest.mark.parametrize("name", CASES)
def test_the_by_products_are_the_dense_inverse(name):
    cs, S = _state(name)
    tr, aa = CV.dense_kinv_sums(S, SM.golden_prior_sigma(name, cs["topo"]))
    for leaf in (False, True):
        info = _twin(name, leaf)[4]
        e_t, e_a = abs(info[6] - tr) / abs(tr), abs(info[7] - aa) / abs(aa)
        print("%s: tr K^-1 = %.6f (rel err %.2e), alpha^T alpha = %.6f (rel err %.2e)" % (name, tr, e_t, aa, e_a))
        assert max(e_t, e_a) <= TOL


@pytest.mark.parametrize("name", CASES)
def test_the_sums_add_up(name):
    cs, S = _state(name)
    p, lf = CV.scored_rows(S)
    for leaf in (False, True):
        mean, var, lpd, group, info = _twin(name, leaf)
        assert info[0] == len(p)
        assert info[3] == lpd[p].sum()
        assert np.array_equal(np.isnan(mean), np.isnan(lpd)) and np.array_equal(np.nonzero(~np.isnan(mean))[0], p)
        assert sorted(np.nonzero(~np.isnan(group))[0]) == sorted(np.unique(lf))
        assert abs(np.nansum(group) - info[2]) <= 1e-12 * max(1.0, abs(info[2]))
    info = _twin(name, False)[4]
    assert info[2] == info[3] and info[1] == len(p)       # every row its own group: the score is the sum of the rows' lpd


@pytest.mark.parametrize("name", ["g32", "kat3"])
def test_the_dense_form_with_a_noise_vector_agrees_at_a_constant_vector(name):
    """tests/_treecv.dense_cv (D = diag(r), dense algebra on K alone) is what the device's noise-vector results are held to: with
    r = R everywhere it must be the tree twin, within the bound of this file."""
    import _noise as NZ
    cs, S = _state(name)
    topo = cs["topo"]
    Sigma = NZ.prior_cov(topo, cs["locs"], cs["spec"], cs["y_obs"])
    ymax = np.nanmax(np.abs(np.asarray(cs["y_obs"], float)))
    for leaf in (False, True):
        want, got = _twin(name, leaf), CV.dense_cv(topo, Sigma, cs["y_obs"], np.full(topo.N, R_CV), leaf)
        ok, gk = ~np.isnan(want[0]), ~np.isnan(want[3])
        assert np.array_equal(ok, ~np.isnan(got[0])) and np.array_equal(gk, ~np.isnan(got[3]))
        e = [np.abs(got[0][ok] - want[0][ok]).max() / ymax, (np.abs(got[1][ok] - want[1][ok]) / want[1][ok]).max(),
             (np.abs(got[2][ok] - want[2][ok]) / np.maximum(1.0, np.abs(want[2][ok]))).max(),
             (np.abs(got[3][gk] - want[3][gk]) / np.maximum(1.0, np.abs(want[3][gk]))).max(),
             max(rel1(got[4][k], want[4][k]) for k in (2, 3, 4)), max(abs(got[4][k] - want[4][k]) / abs(want[4][k]) for k in (5, 6, 7))]
        print("%s %s: dense form against the tree twin: mean %.2e, var %.2e, lpd %.2e, group lpd %.2e, sums %.2e, by-products %.2e"
              % (name, "by leaf" if leaf else "by row", *e))
        assert got[4][0] == want[4][0] and got[4][1] == want[4][1]
        assert max(e) <= TOL


def test_cv_surface_is_exported():
    import os
    from pymra_amd import plan
    from pymra_amd.MRATree import MRATree
    assert "mra_cv" in plan.EXPORTS
    assert callable(plan.HipPlan.cv) and callable(MRATree.crossValidate)
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    assert "#define MRA_CV_LEAF 1u" in hdr
    assert "int mra_cv(mra_plan *plan, uint32_t flags, double *mean_perm, double *var_perm, double *lpd_perm, double *group_lpd, double *info);" in hdr
