"""mra_plan_fit_laplace_trend without a GPU: the dense twin of the iteration (tests/_laplace_trend.py) at its
fixed point, the identity behind info[10], and every refusal of the call, by code, message and order, on a host dry-run plan."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _cases as K
import _laplace as LP
import _laplace_trend as LT

FAMILIES = [LP.POISSON, LP.BINOMIAL]
IDS = ["poisson", "binomial"]


@pytest.mark.parametrize("p", [3, 17])
@pytest.mark.parametrize("family", FAMILIES, ids=IDS)
def test_twin_fixed_point_is_the_joint_mode(family, p):
    """At the mode of (beta, x): X_o^T g(eta^) = 0 (the flat prior on beta) and x^ = Sigma_oo g(eta^).  Both are sums of terms of
    the size of |z| + m (m = e^eta, aux p), so they are held to 1e-9 of the sums of those absolute terms."""
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, X, ref = LT.t16_fit(family, p)
    assert ref["info"][7] == 1.0 and ref["info"][5] == (6 if family == LP.POISSON else 5) and ref["steps"][-1] <= 2e-11
    zo = z[o]
    a_o = None if aux is None else aux[o]
    off_o = 0.0 if offset is None else offset[o]
    g, D, _ = LP.terms(family, zo, 1.0 if a_o is None else a_o, ref["ehat"] + off_o)
    m = zo - g
    Xo, Soo = X[o], Sigma[np.ix_(o, o)]
    score = np.abs(Xo.T @ g)
    scale_b = np.abs(Xo).T @ (np.abs(zo) + m)
    xh = ref["ehat"] - Xo @ ref["beta"]
    gap = np.abs(xh - Soo @ g)
    scale_x = np.abs(Soo) @ (np.abs(zo) + m)
    print("%s p=%d: |X^T g| / scale %.2e, |x^ - Sigma g| / scale %.2e" % (LP.NAMES[family], p, (score / scale_b).max(), (gap / scale_x).max()))
    assert np.all(score <= 1e-9 * scale_b)
    assert np.all(gap <= 1e-9 * scale_x)
    assert np.abs(xh - ref["xhat"]).max() <= 1e-12 * max(1.0, np.abs(xh).max())
    assert np.linalg.cond(ref["A"]) <= 3e2 and np.nanmax(z) <= 341


@pytest.mark.parametrize("p", [1, 3, 17])
@pytest.mark.parametrize("family", FAMILIES, ids=IDS)
def test_info_10_is_the_marginal_laplace_criterion(family, p):
    """info[10] against -2 [log p(z | eta^) - x^^T Sigma_oo^-1 x^ / 2] + log det(I + D^1/2 Sigma_oo D^1/2) + log det A - p log 2 pi,
    with D and A = X_o^T (Sigma_oo + D^-1)^-1 X_o evaluated at eta^ itself (the twin's are those of the last linearisation, one
    step of at most 2e-11 away), x^ = Sigma_oo a."""
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, X, ref = LT.t16_fit(family, p)
    zo = z[o]
    a_o = 1.0 if aux is None else aux[o]
    off_o = 0.0 if offset is None else offset[o]
    _, D, lp = LP.terms(family, zo, a_o, ref["ehat"] + off_o)
    Xo, Soo = X[o], Sigma[np.ix_(o, o)]
    s = np.sqrt(D)
    _, logdet = np.linalg.slogdet(np.eye(len(zo)) + s[:, None] * Soo * s[None, :])
    A = Xo.T @ np.linalg.solve(Soo + np.diag(1.0 / D), Xo)
    a = ref["a"]
    direct = -2.0 * (lp.sum() - 0.5 * float(a @ Soo @ a)) + logdet + np.linalg.slogdet(A)[1] - p * np.log(2.0 * np.pi)
    info = ref["info"]
    print("%s p=%d: info[10] %.10f direct %.10f rel %.2e" % (LP.NAMES[family], p, info[10], direct, abs(info[10] - direct) / abs(direct)))
    assert abs(info[10] - direct) <= 1e-9 * abs(direct)
    assert info[9] == info[0] + info[1] + info[2] + info[3] - info[4] and info[10] == info[9] + info[8] - p * np.log(2.0 * np.pi)
    # x^^T Sigma^-1 x^ = info[1] - info[4]
    assert abs((info[1] - info[4]) - float(a @ Soo @ a)) <= 1e-9 * abs(info[1])
    assert info[11] == int(o.sum())


def test_gaussian_twin_is_gls_in_two_passes():
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, X, ref = LT.t16_fit(LP.GAUSSIAN, 3)
    assert ref["info"][5] == 2 and ref["info"][6] == 0.0 and ref["info"][7] == 1.0
    K_ = Sigma[np.ix_(o, o)] + np.diag(aux[o])
    Xo, t = X[o], (z - offset)[o]
    beta = np.linalg.solve(Xo.T @ np.linalg.solve(K_, Xo), Xo.T @ np.linalg.solve(K_, t))
    assert np.abs(beta - ref["beta"]).max() <= 1e-10 * np.abs(beta).max()


def test_surface_is_exported():
    from pymra_amd import plan
    from pymra_amd.MRATree import MRATree
    import inspect
    assert "mra_plan_fit_laplace_trend" in plan.EXPORTS and callable(plan.HipPlan.fit_laplace_trend)
    sig = inspect.signature(plan.HipPlan.fit_laplace_trend)
    assert list(sig.parameters)[1:] == ["family", "z", "aux", "offset", "e0", "max_iter", "tol"]
    assert sig.parameters["max_iter"].default == 50 and sig.parameters["tol"].default == 1e-10
    tree_sig = inspect.signature(MRATree.fitLaplace)
    assert tree_sig.parameters["X"].default is None and tree_sig.parameters["reml"].default is False
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    assert "int mra_plan_fit_laplace_trend(mra_plan *plan, int family, const double *z_perm, const double *aux_perm, const double *offset_perm," in hdr


def test_refusals_and_their_order_on_a_dry_run_plan(built_library, tmp_path):
    """Every refusal of mra_plan_fit_laplace_trend is a host check made before anything changes, and a MRA_HOST_DRYRUN plan reaches
    all of them; only then does it say that it cannot run.  The order: the plan (set_* missing, MRA_KERNEL_HOST, sharded), the
    missing trend, the argument checks of mra_plan_fit_laplace in its order, a NULL beta."""
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
y = np.asarray(cs["y_obs"], float).ravel()
WHO = "mra_plan_fit_laplace_trend"

def make(obs=True, kernel=True):
    pl = P.HipPlan(topo, 0)
    pl.set_locs(cs["locs"])
    if obs:
        pl.set_obs(cs["y_obs"], cs["c"]["R"])
    if kernel:
        pl.set_kernel(mt.KIND_EXP, 0.3, 1.0, 1.0)
    return pl

pl = make()
ones = pl._padded(np.where(np.isfinite(y), 1.0, np.nan), "z")
seen = np.isfinite(ones)
row = int(np.nonzero(seen)[0][0])
ptr = lambda a: None if a is None else P._ptr(a)

def call(pl, fam=P.MRA_FAMILY_POISSON, z=ones, aux=None, off=None, e0=None, it=5, tol=1e-10, beta=True, info=True):
    b, cv, i = np.full(64, 7.0), np.zeros((64, 64)), np.full(12, 7.0)
    rc = pl.lib.mra_plan_fit_laplace_trend(pl._h, fam, ptr(z), ptr(aux), ptr(off), ptr(e0), it, tol, ptr(b) if beta else None, ptr(cv),
                                           ptr(i) if info else None)
    assert np.all(b == 7.0) and np.all(i == 7.0)             # a refused call writes nothing
    return rc, pl.lib.mra_last_error(pl._h).decode()

def expect(got, code, text):
    assert got[0] == code and text in got[1], (got, code, text)

def at(v, value):
    out = v.copy(); out[row] = value
    return out

# 1. the plan: what every call on the retained factors refuses - before the missing trend and before any argument
bare = make(obs=False)
expect(call(bare, fam=9, beta=False), -4, WHO + " needs set_obs first")
bare.close()
expect(call(pl, fam=9, beta=False), -4, WHO + " needs mra_plan_set_trend first")                 # 2. no trend: before the arguments
host = make(kernel=False)
host.set_kernel_host()
expect(call(host, fam=9), -1, WHO + ": MRA_KERNEL_HOST plans cannot fit a trend")                # the plan's kind before the missing trend
host.close()
pl.set_trend(np.ones((N, 2)))
pl.set_reduce_level(0)
expect(call(pl, fam=9), -1, WHO + ": sharded plans cannot fit a trend")
pl.close()
pl = make()
pl.set_trend(np.ones((N, 2)))
# 3. the arguments, in mra_plan_fit_laplace's order: each call carries every later fault as well
later = dict(it=0, tol=0.0, beta=False)
expect(call(pl, fam=9, **later), -1, WHO + ": unknown family")
expect(call(pl, z=at(ones, np.nan), **later), -1, WHO + ": z is not finite exactly where the plan observes")
expect(call(pl, z=at(ones, -1.0), **later), -1, WHO + ": z < 0 at an observed row (a count) (padded row %d)" % row)
two = np.full(Pn, 2.0)
expect(call(pl, fam=P.MRA_FAMILY_BINOMIAL, aux=at(two, 0.5), **later), -1, WHO + ": binomial trials aux < z or aux <= 0")
expect(call(pl, fam=P.MRA_FAMILY_GAUSSIAN, aux=at(two, 0.0), **later), -1, WHO + ": Gaussian variance aux <= 0")
expect(call(pl, fam=P.MRA_FAMILY_BINOMIAL, aux=at(two, np.inf), off=at(two, np.nan), **later), -1, WHO + ": aux is not finite at an observed row")
expect(call(pl, off=at(two, np.nan), e0=at(two, np.nan), **later), -1, WHO + ": offset is not finite at an observed row")
expect(call(pl, e0=at(two, np.inf), **later), -1, WHO + ": e0 is not finite at an observed row (padded row %d)" % row)
expect(call(pl, it=0, tol=0.0, z=None, beta=False), -1, WHO + ": max_iter < 1")
expect(call(pl, tol=0.0, z=None, beta=False), -1, WHO + ": tol must be greater than 0")
expect(call(pl, tol=np.nan, z=None, beta=False), -1, WHO + ": tol must be greater than 0")
expect(call(pl, z=None, beta=False), -1, WHO + ": z or info is NULL")
expect(call(pl, info=False, beta=False), -1, WHO + ": z or info is NULL")
expect(call(pl, fam=P.MRA_FAMILY_BINOMIAL, beta=False), -1, WHO + ": aux is NULL (only the Poisson family reads none)")
# 4. a NULL beta, the last of the refusals
expect(call(pl, beta=False), -1, WHO + ": beta is NULL")
# values off the mask are nobody's
junk = np.where(seen, 0.0, np.nan)
expect(call(pl, off=junk, e0=junk), -4, "MRA_HOST_DRYRUN plan")
# ... and then the dry-run plan says that it cannot run; nothing changed on the way
expect(call(pl), -4, "MRA_HOST_DRYRUN plan: built in host memory for the sanitizers, it cannot run")
assert pl.info()["trend_p"] == 2
assert np.array_equal(pl.buffer(11), pl._padded(y, "y"), equal_nan=True)
try:
    pl.fit_laplace_trend("poisson", np.where(np.isfinite(y), 1.0, np.nan))
    raise SystemExit("a dry-run plan cannot fit")
except P.MraError as e:
    assert e.code == -4
try:
    pl.fit_laplace_trend("gamma", y)
    raise SystemExit("an unknown family name")
except ValueError:
    pass
pl.close()
print("LAPLACE_TREND_REFUSALS_OK")
''')
    env = dict(os.environ, MRA_ROOT=K.ROOT, MRA_HOST_DRYRUN="1")
    res = subprocess.run([sys.executable, str(child)], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "LAPLACE_TREND_REFUSALS_OK" in res.stdout, (res.stdout + res.stderr)[-3000:]
