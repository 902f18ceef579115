"""The regression trend without a GPU.  The NumPy restatement of mra_trend_fit (tests/_treetrend.py, built on the
restated solver) against a truth that shares none of its algebra: dense generalised least squares and universal kriging on the MRA
prior covariance of the faithful oracle.  Tolerances: those of tests/test_solve_cpu.py for the same trees (1e-9 of the scale; 1e-6
for u3, as test_gpu_solve.test_solve_matches_dense_conditioning).  And the refusals of mra_plan_set_trend on a host dry-run plan."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _cases as K
import _treetrend as TT

CASES = ["g32", "c1", "kat3", "u3"]


def design(N, p, seed=3):
    """An intercept and p - 1 standard normal columns."""
    X = np.random.default_rng(seed).standard_normal((N, p))
    X[:, 0] = 1.0
    return X


def dense_uk(topo, locs, spec, y_obs, R, X):
    """Dense GLS / universal kriging on Sigma_MRA at the reported rows -> dict in the caller's order (0 at unreported rows)."""
    from oracle.mra_faithful import prior_sigma_rows
    y = np.asarray(y_obs, float).ravel()
    rows = np.nonzero((topo.perm >= 0) & np.asarray(topo.in_leaf, bool))[0]
    S = prior_sigma_rows(topo, locs, spec.evaluate, rows)
    cr = topo.perm[rows]                                   # caller rows of the reported rows
    o = np.isfinite(y[cr])
    Xo, yo = X[cr][o], y[cr][o]
    Kc = np.linalg.cholesky(S[np.ix_(o, o)] + R * np.eye(int(o.sum())))
    wy, wX = np.linalg.solve(Kc, yo), np.linalg.solve(Kc, Xo)
    A = wX.T @ wX
    covb = np.linalg.inv(A)
    beta = covb @ (wX.T @ wy)
    res = wy - wX @ beta
    d = 2.0 * np.log(np.diag(Kc)).sum()
    T = np.linalg.solve(Kc, S[o, :])                       # K^-1/2 Sigma[o, :]
    h = X[cr] - T.T @ wX
    mean, var = np.zeros(len(y)), np.zeros(len(y))
    mean[cr] = X[cr] @ beta + T.T @ res
    var[cr] = np.diag(S) - np.einsum("ij,ij->j", T, T) + np.einsum("ij,jk,ik->i", h, covb, h)
    return dict(beta=beta, cov_beta=covb, profile=d + res @ res, reml=d + res @ res + np.linalg.slogdet(A)[1], mean=mean, var=var,
                scale=float(np.abs(S).max()))


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_restated_trend_matches_dense_gls_and_universal_kriging(name, p):
    cs = K.load_case(name)
    topo, locs, spec, R = cs["topo"], cs["locs"], cs["spec"], float(cs["c"]["R"])
    X = design(topo.N, p)
    y = np.asarray(cs["y_obs"], float).ravel() + X @ np.arange(1.0, p + 1.0)       # a mean the zero-mean model would miss
    tw = TT.tree_trend(topo, locs, spec, y, R, X)
    dn = dense_uk(topo, locs, spec, y, R, X)
    tol = 1e-6 if name == "u3" else 1e-9
    e_b = np.abs(tw["beta"] - dn["beta"]).max()
    e_c = np.abs(tw["cov_beta"] - dn["cov_beta"]).max()
    e_p, e_r = abs(tw["profile"] - dn["profile"]), abs(tw["reml"] - dn["reml"])
    e_m, e_v = np.abs(tw["mean"] - dn["mean"]).max(), np.abs(tw["var"] - dn["var"]).max()
    print("%s p=%d: beta %.2e cov %.2e profile %.2e reml %.2e mean %.2e var %.2e (scale %.2f)" % (name, p, e_b, e_c, e_p, e_r, e_m, e_v, dn["scale"]))
    assert e_b <= tol * max(1.0, np.abs(dn["beta"]).max())
    assert e_c <= tol * max(1.0, np.abs(dn["cov_beta"]).max())
    assert e_p <= tol * abs(dn["profile"]) and e_r <= tol * abs(dn["reml"])
    assert e_m <= tol * max(1.0, np.abs(dn["mean"]).max())
    assert e_v <= tol * max(1.0, dn["scale"])
    assert np.all(tw["var"] >= tw["var_pass"])


def test_trend_surface_is_exported():
    from pymra_amd import plan
    from pymra_amd.MRATree import MRATree
    assert {"mra_plan_set_trend", "mra_trend_fit"} <= set(plan.EXPORTS)
    assert plan.MRA_TREND_MAX == 63 and plan.MRA_FULL_QUAD_MAX == 256 and plan.MRA_SOLVE_FULL_QUAD == 1 and plan.MRA_TREND_PREDICT == 1
    assert callable(plan.HipPlan.set_trend) and callable(plan.HipPlan.trend_fit) and callable(MRATree.setTrend)
    assert plan.TrendFit._fields == ("beta", "cov_beta", "profile", "reml", "d", "u", "n_obs", "mean", "var")
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    for line in ("#define MRA_SOLVE_FULL_QUAD 1u", "#define MRA_FULL_QUAD_MAX 256", "#define MRA_TREND_MAX 63", "#define MRA_TREND_PREDICT 1u",
                 "int mra_plan_set_trend(mra_plan *plan, int32_t p, const double *X_perm);"):
        assert line in hdr, line


def test_set_trend_refusals_on_a_dry_run_plan(built_library, tmp_path):
    """mra_plan_set_trend checks everything on the host before anything changes; MRA_HOST_DRYRUN plans take it, so this runs here."""
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
pl = P.HipPlan(topo, 0)
pl.set_locs(cs["locs"]); pl.set_obs(cs["y_obs"], cs["c"]["R"]); pl.set_kernel(mt.KIND_EXP, 0.3, 1.0, 1.0)
lib, h, Pn = pl.lib, pl._h, int(topo.P)
def refused(call, what):
    rc = call()
    msg = lib.mra_last_error(h).decode()
    assert rc == -1, (what, rc)
    assert msg.startswith("mra_plan_set_trend:"), (what, msg)
X = np.ones((64, Pn))
assert pl.info()["trend_p"] == 0
refused(lambda: lib.mra_plan_set_trend(h, 64, P._ptr(X)), "p = 64")
refused(lambda: lib.mra_plan_set_trend(h, -1, P._ptr(X)), "p = -1")
refused(lambda: lib.mra_plan_set_trend(h, 2, None), "NULL X")
assert pl.info()["trend_p"] == 0                       # nothing changed
assert lib.mra_plan_set_trend(h, 3, P._ptr(X)) == 0
assert pl.info()["trend_p"] == 3 and pl.info()["bytes_trend"] == 3 * Pn * 8
bad = X.copy(); bad[2, Pn - 1] = np.nan                # the last entry of the 3 x P array, a phantom row or not
refused(lambda: lib.mra_plan_set_trend(h, 3, P._ptr(bad)), "NaN")
bad[2, Pn - 1] = np.inf
refused(lambda: lib.mra_plan_set_trend(h, 3, P._ptr(bad)), "inf")
assert pl.info()["trend_p"] == 3                       # the refused calls left the trend alone
pl.set_obs(cs["y_obs"], 0.5); pl.set_kernel(mt.KIND_EXP, 0.2, 1.0, 1.0); pl.set_locs(cs["locs"])
assert pl.info()["trend_p"] == 3                       # X survives set_obs, set_kernel, set_locs
pl.set_trend(np.ones((int(topo.N), 63)))               # the widest trend, through the binding's gather
assert pl.info()["trend_p"] == 63
assert lib.mra_plan_set_trend(h, 0, None) == 0
assert pl.info()["trend_p"] == 0 and pl.info()["bytes_trend"] == 0
pl.set_trend(np.ones((int(topo.N), 2))); pl.set_trend(None)
assert pl.info()["trend_p"] == 0
try:
    pl.trend_fit()
    raise SystemExit("a dry-run plan cannot fit")
except P.MraError as e:
    assert e.code == -4
pl.close()
print("SET_TREND_OK")
''')
    env = dict(os.environ, MRA_ROOT=K.ROOT, MRA_HOST_DRYRUN="1")
    res = subprocess.run([sys.executable, str(child)], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "SET_TREND_OK" in res.stdout, (res.stdout + res.stderr)[-2000:]
