"""Nested covariance models (MRA_KERNEL_SUM, kind 7: a sum of up to four closed-form kernels) without a GPU.

* the Python side: ``KernelSpec + KernelSpec`` on a tree's symbolic locations is a ``KernelSum`` (it was a TypeError, and
  ``probe_cov`` turned the tree into a host-evaluated one), what it refuses, and that its ``evaluate`` is the NumPy sum of the
  single-kind array functions bit for bit - the oracles and CPU twins take it through ``.evaluate`` unchanged;
* the C side on an MRA_HOST_DRYRUN plan: kind 7 is accepted, every refusal leaves the previous kernel and its table in place, the
  table holds what derive_kernel_params derives for each component, C(x, x) is the total sill, and mra_plan_prepare goes through.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import _cases as K
import pymra_amd.MRATools as mt
from pymra_amd.MRATree import probe_cov


def _sym(d=2):
    return mt.SymbolicLocs("a", d), mt.SymbolicLocs("b", d)


def test_adding_two_kernels_on_symbolic_locations_gives_a_sum():
    sa, sb = _sym()
    k = mt.Matern32(sa, sb, l=.1, sig=.6) + mt.ExpCovFun(sa, sb, l=.8)
    assert isinstance(k, mt.KernelSum) and k.kind == mt.KIND_SUM == 7 and len(k.components) == 2
    assert [c.kind for c in k.components] == [mt.KIND_MATERN32, mt.KIND_EXP]
    assert k.scale == 1.0 and k.circular is False and k.A is None and k.nu is None
    assert k.l == ((mt.KIND_MATERN32, .1, .6), (mt.KIND_EXP, .8, 1.0)) and k.sig == 1.6
    assert np.array_equal(k.params(), [2, 0, 1, 0, 1, .1, .6, 0, .8, 1.0])
    assert repr(k).startswith("KernelSum(KernelSpec(kind=1") and "scale=" not in repr(k).split(")")[-2]
    got = probe_cov(lambda a, b: mt.Matern32(a, b, l=0.05, sig=0.6) + mt.ExpCovFun(a, b, l=0.8), 2)
    assert isinstance(got, mt.KernelSum) and got.l == ((1, 0.05, 0.6), (0, 0.8, 1.0))
    assert probe_cov(k, 2) is k


def test_sums_flatten_and_scale():
    sa, sb = _sym()
    m, e, g, i = mt.Matern32(sa, sb, l=.3, sig=1.7), mt.ExpCovFun(sa, sb, l=.05), mt.GaussianCovFun(sa, sb, l=.8, sig=1.2), mt.Iden(sa, sb)
    s3 = (m + e) + g
    assert isinstance(s3, mt.KernelSum) and [c.kind for c in s3.components] == [1, 0, 3]
    s4 = (m + e) + (g + 0.1 * i)
    assert [c.kind for c in s4.components] == [1, 0, 3, 4] and s4.l[3] == (mt.KIND_IDEN, 1.0, 0.1)
    assert [c.kind for c in (i + (m + e)).components] == [4, 1, 0]
    # a scalar scales the sum; adding to a scaled sum folds its scale into its components
    t = 1.5 * (m + e)
    assert isinstance(t, mt.KernelSum) and t.scale == 1.5 and t.components == (m + e).components and (t / 3.0).scale == 0.5
    assert ((m + e) * 2).scale == 2.0
    f = t + g
    assert f.scale == 1.0 and f.l == ((1, .3, 1.5 * 1.7), (0, .05, 1.5), (3, .8, 1.2))
    # the component's own scale is part of its sill: 0.7 * Matern32(sig = 2) has sill 1.4, 0.3 * Exp sill 0.3
    w = 0.7 * mt.Matern32(sa, sb, l=.2, sig=2.0) + 0.3 * e
    assert w.l == ((1, .2, 0.7 * 2.0), (0, .05, 0.3)) and w.sig == 0.7 * 2.0 + 0.3
    assert "scale=2" in repr(2 * w)


def test_what_a_sum_refuses():
    sa, sb = _sym(1)
    m, e = mt.Matern32(sa, sb, l=.3), mt.ExpCovFun(sa, sb, l=.05)
    with pytest.raises(ValueError, match="1 to 4"):
        m + e + m + e + m
    with pytest.raises(ValueError, match="1 to 4"):
        (m + e + m) + (e + m)
    with pytest.raises(ValueError, match="Kanter"):
        m + mt.KanterCovFun(sa, sb, radius=0.3)
    with pytest.raises(ValueError, match="Matern\\(nu\\)"):
        mt.Matern(sa, sb, l=.3, nu=0.8) + e
    assert isinstance(mt.Matern(sa, sb, l=.3, nu=1.5) + e, mt.KernelSum)         # (nu = 1.5 is the closed form)
    with pytest.raises(ValueError, match="circular"):
        m + mt.ExpCovFun(sa, sb, l=.05, circular=True)
    assert (mt.Matern32(sa, sb, l=.3, circular=True) + mt.ExpCovFun(sa, sb, l=.05, circular=True)).circular is True
    A, B = np.array([[2.0]]), np.array([[3.0]])
    with pytest.raises(ValueError, match="metric"):
        mt.Matern32(sa, sb, l=.3, metric=A) + e
    with pytest.raises(ValueError, match="metric"):
        mt.Matern32(sa, sb, l=.3, metric=A) + mt.ExpCovFun(sa, sb, l=.05, metric=B)
    s = mt.Matern32(sa, sb, l=.3, metric=A) + mt.ExpCovFun(sa, sb, l=.05, metric=A.copy())
    assert np.array_equal(s.A, A)
    with pytest.raises(ValueError, match="sill"):
        m + (-0.5) * e
    with pytest.raises(TypeError):
        m + 1.0


def test_evaluate_is_the_numpy_sum_of_the_array_functions_bit_for_bit():
    rng = np.random.RandomState(3)
    a, b = rng.uniform(size=(40, 2)), rng.uniform(size=(30, 2))
    a[:5] = b[:5]                                        # some zero distances, for Iden
    sa, sb = _sym()
    cov = lambda x, y: mt.Matern32(x, y, l=.1, sig=.6) + mt.ExpCovFun(x, y, l=.8)
    assert np.array_equal(np.asarray(cov(sa, sb).evaluate(a, b)), np.asarray(cov(a, b)))
    cov4 = lambda x, y: 0.7 * mt.Matern32(x, y, l=.3) + 0.3 * mt.ExpCovFun(x, y, l=.06) + mt.Matern52(x, y, l=.2, sig=.4) + 0.1 * mt.Iden(x, y)
    k4 = cov4(sa, sb)
    want = np.asarray(cov4(a, b))
    assert np.array_equal(np.asarray(k4.evaluate(a, b)), want) and np.count_nonzero(np.asarray(mt.Iden(a, b))) == 5
    assert np.array_equal(np.asarray((2.0 * k4).evaluate(a, b)), 2.0 * want)
    A = np.array([[1.0, 0.5], [0.0, 2.0]])
    covA = lambda x, y: mt.Matern32(x, y, l=.1, sig=.6, metric=A) + mt.GaussianCovFun(x, y, l=.8, metric=A)
    assert np.array_equal(np.asarray(covA(sa, sb).evaluate(a, b)), np.asarray(covA(a, b)))
    t = np.linspace(0, 1, 17).reshape(-1, 1)
    covC = lambda x, y: mt.Matern32(x, y, l=.1, circular=True) + 0.3 * mt.ExpCovFun(x, y, l=.8, circular=True)
    assert np.array_equal(np.asarray(covC(*_sym(1)).evaluate(t, t)), np.asarray(covC(t, t)))


def test_plan_side_parameter_vector():
    from pymra_amd import plan as P
    par = P._kernel_params(7, None, 1.0, 1.5, False, None, [(1, .3, 1.7), (0, .05, 1.0)])
    assert np.array_equal(par, [2, 0, 1.5, 0, 1, .3, 1.7, 0, .05, 1.0])
    sa, sb = _sym()
    k = 1.5 * (mt.Matern32(sa, sb, l=.3, sig=1.7) + mt.ExpCovFun(sa, sb, l=.05))
    # a KernelSum through the call written for a KernelSpec
    assert np.array_equal(P._kernel_params(k.kind, k.l, k.sig, k.scale, k.circular, k.nu, None), par) and np.array_equal(k.params(), par)
    with pytest.raises(ValueError):
        P._kernel_params(7, None, 1.0, 1.0, False, None, None)
    with pytest.raises(ValueError):
        P._kernel_params(1, .3, 1.0, 1.0, False, None, [(1, .3, 1.7)])


CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["MRA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRA_ROOT"], "tests"))
import _cases as K
import _line_cells as LC
import pymra_amd.MRATools as mt
from pymra_amd import plan as P
from pymra_amd.plan import _ptr

cs = K.load_case("g64")
pl = P.HipPlan(cs["topo"], 0)
pl.set_locs(cs["locs"]); pl.set_obs(cs["y_obs"], cs["c"]["R"])
pl.set_kernel(mt.KIND_MATERN32, 0.3, 1.0, 1.0)
assert pl.sum_table().shape == (0, 6) and pl.sum_sill() is None


def refused(p, kind, par, rc_want=-1):
    par = np.array(par, dtype=np.float64)
    rc = p.lib.mra_plan_set_kernel(p._h, kind, _ptr(par), len(par))
    assert rc == rc_want, (kind, par, rc)                  # MRA_ERR_INVALID
    return p.lib.mra_last_error(p._h).decode()


def derived(kind, l, sig, scale):
    """derive_kernel_params for one component: (submode, c / l, 1 / (2 l^2), a1, a2, scale * sig)"""
    c, a1, a2, sub = {0: (1.0, 0.0, 0.0, 0.0), 1: (1.7320508075688772, 1.0, 0.0, 0.0), 2: (2.23606797749979, 1.0, 1.0 / 3.0, 0.0),
                      3: (1.0, 0.0, 0.0, 1.0), 4: (1.0, 0.0, 0.0, 2.0)}[kind]
    return [sub, c / l, 1.0 / (2.0 * (l * l)), a1, a2, scale * sig]


BAD = [([0, 0, 1, 0], "K"), ([5, 0, 1, 0] + [1, .3, 1.0] * 5, "K"), ([1.5, 0, 1, 0, 1, .3, 1.0, 1, .3, 1.0], "K"),
       ([float("nan"), 0, 1, 0, 1, .3, 1.0], "K"), ([-1, 0, 1, 0, 1, .3, 1.0], "K"),
       ([2, 0, 1, 0, 1, .3, 1.0, 0, .05], "too few"), ([1, 0, 1], "too few"), ([1, 0, 1, 0, 1, .3], "too few"),
       ([1, 0, 1, 0, 5, .3, 1.0], "component"), ([1, 0, 1, 0, 6, .3, 1.0], "component"), ([2, 0, 1, 0, 1, .3, 1.0, 7, .3, 1.0], "component"),
       ([1, 0, 1, 0, -1, .3, 1.0], "component"), ([1, 0, 1, 0, 1.5, .3, 1.0], "component"), ([1, 0, 1, 0, float("nan"), .3, 1.0], "component"),
       ([1, 0, 1, 0, 1, 0.0, 1.0], "length"), ([1, 0, 1, 0, 1, -.3, 1.0], "length"), ([1, 0, 1, 0, 1, float("inf"), 1.0], "length"),
       ([2, 0, 1, 0, 1, .3, 1.0, 0, float("nan"), 1.0], "length"),
       ([1, 0, 1, 0, 1, .3, -1e-300], "sig"), ([1, 0, 1, 0, 1, .3, float("nan")], "sig"), ([2, 0, 1, 0, 1, .3, 1.0, 0, .3, float("inf")], "sig"),
       ([1, 0, 1, 1, 1, .3, 1.0], "circular")]                       # (a 2-D plan)

# on a Matern32 plan: refused, and no table appears
for par, word in BAD:
    assert word in refused(pl, 7, par), (par, word)
    assert pl.sum_table().shape == (0, 6)

comps = [(1, .3, 1.7), (2, 2.0, .4), (3, .8, 1.2), (0, .05, 1.0)]
pl.set_kernel(7, components=comps, scale=1.5)
tab = pl.sum_table()
assert tab.shape == (4, 6)
assert np.array_equal(tab, [derived(k, l, s, 1.5) for k, l, s in comps])
assert pl.sum_sill() == ((1.5 * 1.7 + 1.5 * .4) + 1.5 * 1.2) + 1.5              # C(x, x): the records' last entries in component order
# the same components standing in l's place, and an Iden component with a sill; sig = 0 is a component that is switched off
pl.set_kernel(7, comps, 1.0, 1.5)
assert np.array_equal(pl.sum_table(), tab)
pl.set_kernel(7, components=[(1, .3, .7), (0, .06, .3), (4, 1.0, .1)], scale=2.0)
t3 = pl.sum_table()
assert np.array_equal(t3, [derived(1, .3, .7, 2.0), derived(0, .06, .3, 2.0), derived(4, 1.0, .1, 2.0)]) and pl.sum_sill() == (1.4 + .6) + .2
pl.set_kernel(7, components=[(1, .3, 0.0)])
assert pl.sum_table()[0, 5] == 0.0 and pl.sum_sill() == 0.0
pl.set_kernel(7, components=[(1, .3, .7), (0, .06, .3), (4, 1.0, .1)], scale=2.0)
# on a kind-7 plan: every refusal leaves kernel and table as they were (other kinds' refusals too)
for par, word in BAD:
    assert word in refused(pl, 7, par), (par, word)
    assert np.array_equal(pl.sum_table(), t3) and pl.sum_sill() == (1.4 + .6) + .2
refused(pl, 1, [0.0, 1.0, 1.0]); refused(pl, 6, [0.3, 1.0, 1.0, 0.0, 9.0]); refused(pl, 8, [1, 0, 1, 0, 1, .3, 1.0]); refused(pl, 99, [0.3, 1.0, 1.0])
assert "circular" in refused(pl, 1, [0.3, 1.0, 1.0, 1.0])
assert np.array_equal(pl.sum_table(), t3)
# a K = 1 sum holds the single kind's own derived values
for kind in (0, 1, 2, 3, 4):
    pl.set_kernel(7, components=[(kind, .25, 1.0 if kind in (0, 4) else 1.3)], scale=0.8)
    assert np.array_equal(pl.sum_table(), [derived(kind, .25, 1.0 if kind in (0, 4) else 1.3, 0.8)])
# mra_plan_prepare: the fused prior's kernels, which have no mode-5 instance, are not warmed up
pl.set_kernel(mt.KIND_MATERN32, 0.3, 1.0, 1.0)
n_m32 = pl.prepare()
assert pl.sum_table().shape == (0, 6)
pl.set_kernel(7, components=comps, scale=1.5)
assert 0 < pl.prepare() <= n_m32 and pl.prepare() == pl.prepare()
assert np.array_equal(pl.sum_table(), tab)
# the quadrature table of kind 6 and the component table do not show through each other
assert pl.matern_table().shape == (0, 2)
pl.set_kernel(mt.KIND_MATERN, 0.3, 1.0, 1.0, False, 0.8)
assert pl.sum_table().shape == (0, 6) and pl.matern_table().shape[0] > 0
pl.set_kernel(7, components=comps, scale=1.5)
assert np.array_equal(pl.sum_table(), tab) and pl.matern_table().shape == (0, 2)
pl.close()

# circular: accepted on a 1-D plan, refused once it has a metric - and then the kernel from before stands
topo1, locs1, _, y1, _ = LC.problem("L16")
p1 = P.HipPlan(topo1, 0)
p1.set_locs(locs1); p1.set_obs(y1.reshape(-1, 1), LC.R)
p1.set_kernel(7, components=[(1, .02, .7), (0, .004, .3)], circular=True)
t1 = p1.sum_table()
assert t1.shape == (2, 6)
p1.set_kernel(7, components=[(1, .02, .7)], circular=False)
p1.set_metric(np.array([[2.0]]))
assert "circular" in refused(p1, 7, [2, 0, 1, 1, 1, .02, .7, 0, .004, .3])
assert p1.sum_table().shape == (1, 6)
p1.set_kernel(7, components=[(1, .02, .7), (0, .004, .3)])
p1.close()

# mra_eval_kernel checks the same things (and launches nothing on a dry run: a good call ends in MRA_ERR_STATE)
lib = P.load_library()
D = np.zeros(4); out = np.zeros(4)
for par, word in BAD[:-1]:
    par = np.array(par, dtype=np.float64)
    assert lib.mra_eval_kernel(7, _ptr(par), len(par), _ptr(D), 4, _ptr(out)) == -1, par
par = np.array([2, 0, 1.5, 0, 1, .3, 1.7, 0, .05, 1.0])
assert lib.mra_eval_kernel(7, _ptr(par), len(par), _ptr(D), 4, _ptr(out)) == -4
print("KERNEL_SUM_OK")
'''


def test_kind_7_on_a_dry_run_plan(built_library, tmp_path):
    child = tmp_path / "child.py"
    child.write_text(CHILD)
    env = dict(os.environ, MRA_ROOT=K.ROOT, MRA_HOST_DRYRUN="1")
    res = subprocess.run([sys.executable, str(child)], env=env, capture_output=True, text=True, timeout=600)
    print(res.stdout[-500:])
    assert res.returncode == 0 and "KERNEL_SUM_OK" in res.stdout, (res.stdout + res.stderr)[-3000:]
