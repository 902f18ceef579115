"""MRA_KERNEL_MATERN (kind 6, any smoothness nu in [0.1, 5]) without a GPU.

The golden tests/golden/matern_nu.npz holds M_nu(t) = 2^(1-nu) / Gamma(nu) t^nu K_nu(t) from mpmath at 40 digits
(tests/golden/make_matern_nu.py).  Against it:

* ``mt.Matern`` on arrays (the host evaluation every CPU twin and oracle goes through): 5e-15 * sig.
* a NumPy restatement of the device sum - the plan's own host-built table, read back from a MRA_HOST_DRYRUN plan, summed
  sequentially in the device's order with the device's exits and selects: 2e-14, about twice the 1.1e-14 measured for the
  method in float64.  It pins the method apart from the device's own exponential.

And the C ABI on a host dry run, as tests/test_capi_cpu.py runs it: what mra_plan_set_kernel refuses (before anything changes,
the refusals found last included), the table itself, and mra_plan_prepare on a kind-6 plan."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _cases as K

GOLDEN = os.path.join(K.ROOT, "tests", "golden", "matern_nu.npz")
NODES, H, T_MIN, T_MAX = 191, 0.2, 2.0 ** -40, 745.0


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert list(g["nu"]) == [0.1, 0.25, 0.5, 0.8, 1.0, 1.5, 2.0, 2.5, 3.3, 5.0]
    assert g["t"][0] == 0.0 and len(g["t"]) == 206 and np.all(g["M"][:, 0] == 1.0)
    return g


def device_sum(tab, nu, t):
    """matern_nu_of_t (pymra_amd/csrc/mra_kernels.h) for one t in NumPy float64: same table, same order, same exits and selects."""
    if t == 0.0:
        return 1.0
    if t >= T_MAX:
        return 0.0
    if t < T_MIN:
        a = math.gamma(1.0 - nu) / (math.gamma(1.0 + nu) * 4.0 ** nu) if nu < 1.0 else 0.0
        return 1.0 - a * math.exp(2.0 * nu * math.log(t))
    S = 0.0
    for ch, w in tab:
        x = t * ch
        if not x < T_MAX:
            break
        S = S + w * math.exp(-x)
    return math.exp(nu * math.log(t)) * S


def test_host_matern_against_the_golden(golden):
    import pymra_amd.MRATools as mt
    sig, l = 1.7, 0.4
    worst = 0.0
    for nu, ref, ref_edge in zip(golden["nu"], golden["M"], golden["M_edge"]):
        for t, want in ((golden["t"], ref), (golden["t_edge"], ref_edge)):
            # mt.Matern(0, x) is sig * matern_nu(sqrt(2 nu) |x| / l), to the bit; the function at the golden's own t
            # (l = sqrt(2 nu) would still round t on the way in)
            x = t.reshape(-1, 1)
            got = np.asarray(mt.Matern(np.zeros((1, 1)), x, l=l, sig=sig, nu=nu)).ravel()
            assert np.array_equal(got, sig * mt.matern_nu(np.sqrt(2.0 * nu) * t / l, nu))
            err = np.abs(sig * mt.matern_nu(t, nu) - sig * want)
            worst = max(worst, float(err.max()))
            assert np.all(err <= 5e-15 * sig), (nu, float(err.max()), float(t[np.argmax(err)]))
        x = (golden["t"] * 0.1).reshape(-1, 1)
        spec = mt.KernelSpec(mt.KIND_MATERN, l, sig, 2.0, nu=nu)
        assert np.array_equal(spec.evaluate(np.zeros((1, 1)), x), 2.0 * np.asarray(mt.Matern(np.zeros((1, 1)), x, l=l, sig=sig, nu=nu)))
    print("mt.Matern against the golden: %.2e" % worst)


def test_half_integer_nu_returns_the_closed_forms():
    import pymra_amd.MRATools as mt
    from pymra_amd.MRATree import probe_cov
    a, b = mt.SymbolicLocs("a", 2), mt.SymbolicLocs("b", 2)
    s = mt.Matern(a, b, l=0.3, sig=1.5, nu=0.5)
    assert (s.kind, s.l, s.sig, s.scale, s.nu) == (mt.KIND_EXP, 0.3, 1.0, 1.5, None)
    s = mt.Matern(a, b, l=0.3, sig=1.5, nu=1.5)
    assert (s.kind, s.l, s.sig, s.scale, s.nu) == (mt.KIND_MATERN32, 0.3, 1.5, 1.0, None)
    s = mt.Matern(a, b, l=0.3, sig=1.5, nu=2.5)
    assert (s.kind, s.l, s.sig, s.scale, s.nu) == (mt.KIND_MATERN52, 0.3, 1.5, 1.0, None)
    s = probe_cov(lambda p, q: 2.0 * mt.Matern(p, q, l=0.3, sig=1.5, nu=0.8, circular=True), 1)
    assert (s.kind, s.l, s.sig, s.scale, s.nu, s.circular) == (mt.KIND_MATERN, 0.3, 1.5, 2.0, 0.8, True)
    assert "nu=0.8" in repr(s) and "nu" not in repr(mt.KernelSpec(mt.KIND_EXP, 0.3))
    assert (s / 4.0).nu == 0.8 and (s / 4.0).scale == 0.5
    # the closed forms are the same functions
    x = np.random.RandomState(0).uniform(size=(40, 2))
    for nu, fn in ((1.5, mt.Matern32), (2.5, mt.Matern52)):
        assert np.max(np.abs(np.asarray(mt.Matern(x, x, l=0.3, sig=1.5, nu=nu)) - np.asarray(fn(x, x, l=0.3, sig=1.5)))) < 5e-15
    assert np.max(np.abs(np.asarray(mt.Matern(x, x, l=0.3, sig=1.5, nu=0.5)) - 1.5 * np.asarray(mt.ExpCovFun(x, x, l=0.3)))) < 5e-15
    for bad in (0.05, 5.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mt.Matern(a, b, nu=bad)
        with pytest.raises(ValueError):
            mt.Matern(x, x, nu=bad)
    with pytest.raises(ValueError):
        mt.KernelSpec(mt.KIND_MATERN, 0.3)


CHILD = r'''
import math, os, sys
import numpy as np
sys.path.insert(0, os.environ["MRA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRA_ROOT"], "tests"))
import _cases as K
import pymra_amd.MRATools as mt
from pymra_amd import plan as P
from pymra_amd.plan import _ptr
import test_matern_nu_cpu as T

cs = K.load_case("g64")
pl = P.HipPlan(cs["topo"], 0)
pl.set_locs(cs["locs"]); pl.set_obs(cs["y_obs"], cs["c"]["R"])
pl.set_kernel(mt.KIND_MATERN32, 0.3, 1.0, 1.0)
assert pl.matern_table().shape == (0, 2)


def refused(kind, par):
    par = np.array(par, dtype=np.float64)
    rc = pl.lib.mra_plan_set_kernel(pl._h, kind, _ptr(par), len(par))
    assert rc == -1, (kind, par, rc)                       # MRA_ERR_INVALID
    return pl.lib.mra_last_error(pl._h).decode()


# refusals on a Matern32 plan: the kernel stays (a kind-6 kernel would show its table)
for nu in (0.05, 5.5, float("nan"), float("inf"), -1.0):
    assert "nu" in refused(6, [0.3, 1.0, 1.0, 0.0, nu])
    assert pl.matern_table().shape == (0, 2)
assert "MRA_KERNEL_MATERN" in refused(6, [0.3, 1.0, 1.0, 0.0])          # n_params = 4
refused(6, [0.0, 1.0, 1.0, 0.0, 0.8]); refused(6, [-1.0, 1.0, 1.0, 0.0, 0.8])
assert "unknown kernel kind" in refused(7, [0.3, 1.0, 1.0, 0.0, 0.8])
refused(-1, [0.3, 1.0, 1.0]); refused(99, [0.3, 1.0, 1.0])
assert pl.matern_table().shape == (0, 2)

g = np.load(T.GOLDEN)
worst = 0.0
for i, nu in enumerate(g["nu"]):
    pl.set_kernel(mt.KIND_MATERN, 0.3, 1.2, 1.0, False, nu)
    tab = pl.matern_table()
    assert tab.shape == (T.NODES, 2)
    # the table: cosh(k h) and c h cosh(nu k h), the weight halved at k = 0
    u = T.H * np.arange(T.NODES)
    c = 2.0 ** (1.0 - nu) / math.gamma(nu)
    w = c * T.H * np.cosh(nu * u); w[0] *= 0.5
    assert tab[0, 0] == 1.0 and abs(tab[0, 1] - 0.5 * c * T.H) <= 4e-16 * c
    assert np.all(np.abs(tab[:, 0] - np.cosh(u)) <= 4e-16 * np.cosh(u)), nu
    assert np.all(np.abs(tab[:, 1] - w) <= 1e-14 * w), nu
    # refused on a kind-6 plan: table and kernel stand
    refused(6, [0.3, 1.0, 1.0, 0.0, 7.0]); refused(7, [0.3, 1.0, 1.0, 0.0, 0.8])
    assert np.array_equal(pl.matern_table(), tab)
    # a change of l, sig or scale leaves the table alone
    pl.set_kernel(mt.KIND_MATERN, 0.7, 0.9, 2.0, False, nu)
    assert np.array_equal(pl.matern_table(), tab)
    # the device sum restated on this table against the golden
    for t, want in zip(np.concatenate((g["t"], g["t_edge"])), np.concatenate((g["M"][i], g["M_edge"][i]))):
        e = abs(T.device_sum(tab, nu, float(t)) - want)
        worst = max(worst, e)
        assert e <= 2e-14, (nu, t, e)
    assert T.device_sum(tab, nu, 745.0) == 0.0 and T.device_sum(tab, nu, 1e150) == 0.0 and T.device_sum(tab, nu, 0.0) == 1.0
# mra_plan_prepare on a kind-6 plan: the fused prior kernels, which have no instance of it, are not warmed up
pl.set_kernel(mt.KIND_MATERN32, 0.3, 1.0, 1.0)
n_m32 = pl.prepare()
pl.set_kernel(mt.KIND_MATERN, 0.3, 1.0, 1.0, False, 0.8)
assert 0 < pl.prepare() <= n_m32 and pl.prepare() == pl.prepare()
# a refusal that is found late leaves a kind-6 plan as it was: circular distances on this 2-D plan, for another kind and for kind 6
tab = pl.matern_table().copy()
assert tab.shape == (T.NODES, 2)
assert "circular" in refused(1, [0.3, 1.0, 1.0, 1.0]) and "circular" in refused(6, [0.3, 1.0, 1.0, 1.0, 2.0])
refused(1, [0.0, 1.0, 1.0])
assert np.array_equal(pl.matern_table(), tab)            # (0 rows once the plan's mode is no longer 4)
# back to another kind: no table on show, and kind 6 again rebuilds it
pl.set_kernel(mt.KIND_EXP, 0.3)
assert pl.matern_table().shape == (0, 2)
pl.set_kernel(mt.KIND_MATERN, 0.3, 1.0, 1.0, False, 0.8)
assert pl.matern_table().shape == (T.NODES, 2)
pl.close()
# mra_eval_kernel checks the same things (and launches nothing on a dry run)
D = np.zeros(4); out = np.zeros(4)
for kind, par in ((6, [0.3, 1.0, 1.0, 0.0, 9.0]), (6, [0.3, 1.0, 1.0, 0.0]), (7, [0.3, 1.0, 1.0, 0.0, 0.8])):
    par = np.array(par)
    assert P.load_library().mra_eval_kernel(kind, _ptr(par), len(par), _ptr(D), 4, _ptr(out)) == -1
print("MATERN_NU_OK worst %.3e" % worst)
'''


def test_set_kernel_refusals_table_and_device_sum_on_a_dry_run(built_library, tmp_path, golden):
    child = tmp_path / "child.py"
    child.write_text(CHILD)
    env = dict(os.environ, MRA_ROOT=K.ROOT, MRA_HOST_DRYRUN="1")
    res = subprocess.run([sys.executable, str(child)], env=env, capture_output=True, text=True, timeout=600)
    print(res.stdout[-500:])
    assert res.returncode == 0 and "MATERN_NU_OK" in res.stdout, (res.stdout + res.stderr)[-3000:]
