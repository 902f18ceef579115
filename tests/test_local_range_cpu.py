"""Local ranges (MRA_KERNEL_LOCAL, kind 8: a nonstationary covariance whose range varies over the domain) without a GPU.

* ``mt.LocalRange.evaluate``, the float64 NumPy statement of the formula that every oracle and CPU twin uses, against a longdouble
  evaluation of the same formula, for ds = 1 and 2 and each base kind; a constant range field against the stationary kernel of
  range l * lam0; symmetry to the bit, the diagonal exactly scale * sig, and validity on 400 random points with a tenfold range;
* the Python refusals (``LocalRange`` and ``MRATree(local_range=)``), ``MRATree._sites`` and ``_locate`` on the spatial columns;
* the C side on an MRA_HOST_DRYRUN plan: kind 8 is accepted, every refusal leaves the previous kernel in place, the metric refusal
  holds in both orders, a range that is not positive or not finite is refused by whichever of set_locs and set_kernel comes
  second, and mra_plan_prepare goes through.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import _cases as K
import pymra_amd.MRATools as mt

BASES = (mt.KIND_EXP, mt.KIND_MATERN32, mt.KIND_MATERN52, mt.KIND_GAUSSIAN)
LD = np.longdouble
EPS = 2.0 ** -53


def _base(kind, l=0.7, sig=1.3, scale=1.5):
    return mt.KernelSpec(kind, l, 1.0 if kind == mt.KIND_EXP else sig, scale)


def _points(ds, n, seed, decade=1.0):
    """n points in the unit interval / square, ranges over `decade` decades that grow with the first coordinate"""
    rng = np.random.RandomState(seed)
    x = rng.uniform(size=(n, ds))
    lam = 0.05 * 10.0 ** (decade * x[:, 0]) * rng.uniform(0.9, 1.1, size=n)
    return np.column_stack([x, lam])


def _longdouble(spec, a, b):
    """the formula of DESIGN.md section 25 in longdouble, written independently of LocalRange.evaluate"""
    a, b = a.astype(LD), b.astype(LD)
    ds = a.shape[1] - 1
    D = np.sqrt(sum((a[:, k][:, None] - b[:, k][None, :]) ** 2 for k in range(ds)))
    la, lb = a[:, -1][:, None], b[:, -1][None, :]
    q = (la ** 2 + lb ** 2) / LD(2)
    pref = (la * lb / q) ** (LD(ds) / LD(2))
    kind, l = spec.base.kind, LD(spec.base.l)
    r = D / (l * np.sqrt(q))
    if kind == mt.KIND_EXP:
        k0 = np.exp(-r)
    elif kind == mt.KIND_MATERN32:
        k0 = (1 + np.sqrt(LD(3)) * r) * np.exp(-np.sqrt(LD(3)) * r)
    elif kind == mt.KIND_MATERN52:
        k0 = (1 + np.sqrt(LD(5)) * r + LD(5) / LD(3) * r ** 2) * np.exp(-np.sqrt(LD(5)) * r)
    else:
        k0 = np.exp(-r ** 2 / LD(2))
    return LD(spec.scale) * LD(spec.sig) * pref * k0


@pytest.mark.parametrize("ds", (1, 2))
@pytest.mark.parametrize("kind", BASES)
def test_evaluate_against_the_longdouble_formula(kind, ds):
    """The bar, from the operation count of ``evaluate``: t = c sqrt(D2 / q) / l carries at most 8 roundings (two squares and a sum
    in D2 - the subtraction of nearby coordinates is exact - three in q, the quotient, the root, c and the two operations with it),
    so |dt| <= 8 eps t, and |d k0| <= max_t t |k0'(t)| * 8 eps <= 0.62 * 8 eps < 5 eps of the sill (t e^-t <= 0.37; Matern52:
    t (t + t^2) e^-t / 3 <= 0.62); exp, the polynomial and their product add 4, the prefactor (product, quotient, the root in 1-D)
    4, the two products with the sill 2: 15 eps.  The bar is 16 eps = 8 ulp of the sill."""
    spec = mt.LocalRange(_base(kind))
    a, b = _points(ds, 60, 1, 2.0), _points(ds, 70, 2, 2.0)
    got = spec.evaluate(a, b)
    want = _longdouble(spec, a, b)
    err = float(np.max(np.abs(got.astype(LD) - want))) / (spec.scale * spec.sig)
    print("kind %d ds %d: max error %.2f eps of the sill" % (kind, ds, err / EPS))
    assert got.shape == (60, 70) and got.dtype == np.float64
    assert err <= 16 * EPS
    if np.finfo(LD).eps < 2.0 ** -60:           # (a longdouble that is float64 would compare the formula with itself)
        assert err > 0.0


@pytest.mark.parametrize("ds", (1, 2))
@pytest.mark.parametrize("kind", BASES)
def test_a_constant_range_is_the_stationary_kernel(kind, ds):
    """lam = lam0 everywhere: q = lam0^2 and the prefactor 1 exactly, C = k0(D / (l lam0)).  Both sides round t a few times (here
    sqrt(D2 / q) / l * c, there c * D / (l lam0)): 6 + 4 roundings, 10 eps t, at most 0.62 * 10 eps < 7 eps of the sill, and each
    side's exp, polynomial and products 4 more: 15 eps.  The bar is 16 eps = 8 ulp of the sill."""
    lam0 = 0.37
    base = _base(kind)
    spec = mt.LocalRange(base)
    a, b = _points(ds, 50, 3), _points(ds, 40, 4)
    a[:, -1] = lam0
    b[:, -1] = lam0
    flat = mt.KernelSpec(kind, base.l * lam0, base.sig, base.scale).evaluate(a[:, :ds], b[:, :ds])
    err = float(np.max(np.abs(spec.evaluate(a, b) - flat))) / (spec.scale * spec.sig)
    print("kind %d ds %d: constant range against the stationary kernel: %.2f eps of the sill" % (kind, ds, err / EPS))
    assert err <= 16 * EPS


@pytest.mark.parametrize("ds", (1, 2))
@pytest.mark.parametrize("kind", BASES)
def test_symmetry_diagonal_and_validity(kind, ds):
    spec = mt.LocalRange(_base(kind))
    X = _points(ds, 400, 5, 1.0)
    assert X[:, -1].max() / X[:, -1].min() > 8.0
    S = spec.evaluate(X, X)
    assert np.array_equal(S, S.T)                                   # to the bit
    assert np.all(np.diag(S) == spec.scale * spec.sig)              # exactly scale * sig
    w = np.linalg.eigvalsh(S)
    print("kind %d ds %d: eigenvalues %.3e .. %.3e" % (kind, ds, w[0], w[-1]))
    assert w[0] >= -1e-12 * w[-1]


def test_the_python_side():
    sa, sb = mt.SymbolicLocs("a", 2), mt.SymbolicLocs("b", 2)
    k = mt.LocalRange(2.0 * mt.Matern32(sa, sb, l=0.5, sig=1.2))
    assert k.kind == mt.KIND_LOCAL == 8 and k.circular is False and k.A is None and k.nu is None and k.lam is None
    assert k.l == (mt.KIND_MATERN32, 0.5) and k.sig == 1.2 and k.scale == 2.0
    assert np.array_equal(k.params(), [0.5, 1.2, 2.0, 0.0, 1.0])
    k3 = 3.0 * k
    assert isinstance(k3, mt.LocalRange) and k3.scale == 6.0 and (k / 2.0).scale == 1.0 and "LocalRange" in repr(k3)
    e = mt.LocalRange(0.5 * mt.ExpCovFun(sa, sb, l=0.2))
    assert np.array_equal(e.params(), [0.2, 1.0, 0.5, 0.0, 0.0])
    assert mt.LocalRange(k.base, lam=[1.0, 2.0]).lam.tolist() == [1.0, 2.0]
    for bad in (mt.Iden(sa, sb), mt.KanterCovFun(sa, sb, radius=0.3), mt.Matern(sa, sb, l=0.3, nu=0.8),
                mt.Matern32(mt.SymbolicLocs("a", 1), mt.SymbolicLocs("b", 1), l=0.3, circular=True),
                mt.Matern32(sa, sb, l=0.3, metric=np.eye(2)), mt.Matern32(sa, sb, l=-1.0)):
        with pytest.raises(ValueError):
            mt.LocalRange(bad)
    with pytest.raises(TypeError):
        mt.LocalRange(mt.Matern32(sa, sb, l=0.3) + mt.ExpCovFun(sa, sb, l=0.1))
    for lam in ([1.0, -1.0], [1.0, 0.0], [1.0, np.nan], [[1.0, 2.0], [3.0, 4.0]]):
        with pytest.raises(ValueError):
            mt.LocalRange(k.base, lam=lam)
    with pytest.raises(ValueError):
        k.evaluate(np.ones((3, 1)), np.ones((3, 1)))                # no range column
    with pytest.raises(ValueError):
        k.evaluate(np.array([[0.1, 0.2, -1.0]]), np.array([[0.1, 0.2, 1.0]]))


def _bare_tree(locs, lam):
    """an MRATree that has only what _sites, _locate and _probe read (no library, no device)"""
    from pymra_amd import MRATree
    from pymra_amd.topology import build_topology
    np.random.seed(7)
    t = MRATree.__new__(MRATree)
    t.locs, t.d = locs, locs.shape[1]
    t.local_range = None if lam is None else mt._check_ranges(lam, len(locs))
    t.cov_locs = locs if lam is None else np.column_stack([locs, t.local_range])
    t.cov_d = t.cov_locs.shape[1]
    t.metric, t.radius = "euclidean", 1.0
    t.topology = build_topology(locs, 16, 1, 4)
    t.kernel = types.SimpleNamespace(circular=False)
    return t


def test_sites_and_locate_use_the_spatial_columns_only():
    locs = mt.genLocations2d(Nx=16, Ny=16)
    # ranges that would win a three-column nearest-neighbour search: neighbours in space differ by 100 in the range
    lam = np.where(np.arange(256) % 2 == 0, 1.0, 101.0)
    t = _bare_tree(locs, lam)
    rows = np.array([3, 40, 77, 130, 201, 255])
    sites = locs[rows] + 1e-4
    S = t._sites(sites, local_range=np.full(len(rows), 50.0))
    assert S.shape == (6, 3) and np.array_equal(S[:, :2], sites) and np.all(S[:, 2] == 50.0)
    leaf = t.locate(sites, local_range=np.full(len(rows), 50.0))
    topo = t.topology
    leaf_of = np.full(topo.P, -1)
    for i in np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]:
        leaf_of[int(topo.node_row0[i]):int(topo.node_row1[i])] = i
    padded = np.full(256, -1)
    ok = topo.perm >= 0
    padded[topo.perm[ok]] = np.nonzero(ok)[0]
    assert np.array_equal(leaf, leaf_of[padded[rows]])              # the leaf of the spatially nearest row, whatever its range
    assert np.array_equal(t.locate(sites, local_range=np.full(len(rows), 1e-3)), leaf)
    with pytest.raises(ValueError):
        t._sites(sites)                                             # local_range is mandatory
    with pytest.raises(ValueError):
        t._sites(sites, local_range=np.ones(5))
    with pytest.raises(ValueError):
        t._sites(sites, local_range=-np.ones(6))
    with pytest.raises(ValueError):
        t._sites(S, local_range=np.ones(6))                         # (n, d), not (n, d + 1)
    with pytest.raises(ValueError):
        _bare_tree(locs, None)._sites(sites, local_range=np.ones(6))
    # what cov the tree takes
    k = t._probe(lambda a, b: 0.5 * mt.Matern52(a, b, l=1.0, sig=2.0))
    assert isinstance(k, mt.LocalRange) and k.l == (mt.KIND_MATERN52, 1.0) and k.sig == 2.0 and k.scale == 0.5 and k.lam is t.local_range
    for bad in (lambda a, b: mt.Matern32(a, b, l=1.0) + mt.ExpCovFun(a, b, l=0.1), lambda a, b: mt.Iden(a, b),
                lambda a, b: np.eye(len(a)), np.eye(4), lambda a, b: mt.Matern32(a, b, l=1.0, metric=np.eye(2))):
        with pytest.raises(ValueError):
            t._probe(bad)


def test_the_tree_refuses_before_it_builds_anything():
    from pymra_amd import MRATree
    locs = mt.genLocations2d(Nx=8, Ny=8)
    y = np.zeros((64, 1))
    cov = lambda a, b: mt.Matern32(a, b, l=1.0)
    lam = np.full(64, 0.3)
    for kw in (dict(cov_locs=np.column_stack([locs, lam])), dict(metric="chordal")):
        with pytest.raises(ValueError):
            MRATree(locs, 4, cov, y, 0.1, M=1, J=4, local_range=lam, verbose=False, **kw)
    with pytest.raises(ValueError):
        MRATree(np.column_stack([locs, lam]), 4, cov, y, 0.1, M=1, J=4, local_range=lam, verbose=False)     # three columns already
    for bad in (lam[:-1], -lam, np.where(np.arange(64) == 5, np.nan, lam), np.where(np.arange(64) == 5, 0.0, lam)):
        with pytest.raises(ValueError):
            MRATree(locs, 4, cov, y, 0.1, M=1, J=4, local_range=bad, verbose=False)


CHILD = r'''
import dataclasses, os, sys
import numpy as np
sys.path.insert(0, os.environ["MRA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRA_ROOT"], "tests"))
import _cases as K
import _line_cells as LC
import pymra_amd.MRATools as mt
from pymra_amd import plan as P
from pymra_amd.plan import _ptr

cs = K.load_case("g64")
topo3 = dataclasses.replace(cs["topo"], coord_dim=3)
N = len(cs["locs"])
lam = 0.05 * 10.0 ** cs["locs"][:, 0]
X3 = np.column_stack([cs["locs"], lam])


def refused(p, kind, par, rc_want=-1):
    par = np.array(par, dtype=np.float64)
    rc = p.lib.mra_plan_set_kernel(p._h, kind, _ptr(par), len(par))
    assert rc == rc_want, (kind, par, rc)                  # MRA_ERR_INVALID
    return p.lib.mra_last_error(p._h).decode()


def kernel_stands(p, want):
    """Which kernel the plan holds, read off what it does (nothing runs on a dry-run plan): a metric is refused by name while the
    kernel is kind 8 and accepted under the Matern32 from before."""
    A = np.eye(p.d); A[0, 0] = 2.0
    rc = p.lib.mra_plan_set_metric(p._h, _ptr(A))
    if rc == 0:
        p.set_metric(None)
        got = "Matern32"
    else:
        assert rc == -1 and "MRA_KERNEL_LOCAL" in p.lib.mra_last_error(p._h).decode()
        got = "Local"
    assert got == want, (got, want)


pl = P.HipPlan(topo3, 0)
assert pl.d == 3
pl.set_locs(X3); pl.set_obs(cs["y_obs"], cs["c"]["R"])
pl.set_kernel(mt.KIND_MATERN32, 0.3, 1.0, 1.0)
kernel_stands(pl, "Matern32")
# every refusal leaves the Matern32 in place
BAD = [([1.0, 1.0, 1.0, 0.0], "base_kind"), ([1.0, 1.0, 1.0], "base_kind"), ([1.0, 1.0, 1.0, 0.0, 4.0], "base kind"),
       ([1.0, 1.0, 1.0, 0.0, 5.0], "base kind"), ([1.0, 1.0, 1.0, 0.0, 6.0], "base kind"), ([1.0, 1.0, 1.0, 0.0, 1.5], "base kind"),
       ([1.0, 1.0, 1.0, 0.0, float("nan")], "base kind"), ([1.0, 1.0, 1.0, 1.0, 1.0], "circular"),
       ([0.0, 1.0, 1.0, 0.0, 1.0], "length"), ([-1.0, 1.0, 1.0, 0.0, 1.0], "length"), ([float("inf"), 1.0, 1.0, 0.0, 1.0], "length"),
       ([float("nan"), 1.0, 1.0, 0.0, 1.0], "length"), ([1.0, -1.0, 1.0, 0.0, 1.0], "sig"), ([1.0, float("nan"), 1.0, 0.0, 1.0], "sig")]
for par, word in BAD:
    assert word in refused(pl, 8, par), (par, word)
    kernel_stands(pl, "Matern32")
# accepted: each base kind; the plan takes the level-by-level prior
for base in (0, 1, 2, 3):
    pl.set_kernel(8, (base, 1.0), 1.2, 0.8)
    kernel_stands(pl, "Local")
# ... and the refusals leave THAT kernel in place as well
for par, word in BAD:
    assert word in refused(pl, 8, par), (par, word)
refused(pl, 99, [0.3, 1.0, 1.0]); refused(pl, 9, [0.3, 1.0, 1.0]); refused(pl, 1, [0.0, 1.0, 1.0])
kernel_stands(pl, "Local")
# mra_plan_prepare: the fused prior's kernels, which have no mode-6 instance, are not warmed up
pl.set_kernel(mt.KIND_MATERN32, 0.3, 1.0, 1.0)
n_m32 = pl.prepare()
pl.set_kernel(8, (1, 1.0), 1.2, 0.8)
assert 0 < pl.prepare() <= n_m32 and pl.prepare() == pl.prepare()

# the metric, both orders
A = np.diag([1.0, 2.0, 1.0])
rc = pl.lib.mra_plan_set_metric(pl._h, _ptr(A))
assert rc == -1 and "MRA_KERNEL_LOCAL" in pl.lib.mra_last_error(pl._h).decode()
assert np.array_equal(pl.buffer(13).reshape(-1, 3)[:, 1].max(), X3[:, 1].max())      # the coordinates are the caller's still
pl.set_metric(None)                                           # NULL is no metric: accepted
kernel_stands(pl, "Local")
pl.set_kernel(mt.KIND_MATERN32, 0.3, 1.0, 1.0)
pl.set_metric(A)
assert "metric" in refused(pl, 8, [1.0, 1.0, 1.0, 0.0, 1.0])
kernel_stands(pl, "Matern32")
pl.set_metric(None)
pl.set_kernel(8, (1, 1.0), 1.2, 0.8)

# a range that is not positive and finite: set_locs second ...
for bad in (0.0, -1.0, float("nan"), float("inf")):
    Xb = X3.copy(); Xb[N // 2, 2] = bad
    try:
        pl.set_locs(Xb)
        raise AssertionError("set_locs accepted a range of %r" % bad)
    except P.MraError as e:
        assert e.code == -1 and "range" in str(e), str(e)
    kernel_stands(pl, "Local")          # the coordinates from before stand: the plan still runs
    assert np.array_equal(pl.buffer(13).reshape(-1, 3)[:, 2].max(), X3[:, 2].max())
# ... and set_kernel second
for bad in (0.0, -1.0, float("nan"), float("inf")):
    Xb = X3.copy(); Xb[7, 2] = bad
    # straight after set_locs, before the plan has any kernel
    p2 = P.HipPlan(topo3, 0)
    p2.set_locs(Xb)                                           # set_locs itself takes such a column: without kind 8 it is a coordinate
    assert "range" in refused(p2, 8, [1.0, 1.0, 1.0, 0.0, 1.0]), bad
    p2.close()
    # ... and with another kernel in place, which then stands
    p2 = P.HipPlan(topo3, 0)
    p2.set_locs(Xb)
    p2.set_obs(cs["y_obs"], cs["c"]["R"])
    p2.set_kernel(mt.KIND_MATERN32, 0.3, 1.0, 1.0)
    assert "range" in refused(p2, 8, [1.0, 1.0, 1.0, 0.0, 1.0]), bad
    kernel_stands(p2, "Matern32")
    p2.set_locs(X3)                                           # good ranges: accepted
    p2.set_kernel(8, (1, 1.0), 1.2, 0.8)
    kernel_stands(p2, "Local")
    p2.close()
# kind 8 before any locations: accepted, and then set_locs checks
p3 = P.HipPlan(topo3, 0)
p3.set_kernel(8, (3, 1.0), 1.0, 1.0)
Xb = X3.copy(); Xb[0, 2] = 0.0
try:
    p3.set_locs(Xb)
    raise AssertionError("set_locs accepted a range of 0")
except P.MraError as e:
    assert e.code == -1
p3.set_locs(X3)
p3.close()
pl.close()

# d = 1: refused; d = 2 with (x, lam) rows: accepted
topo1, locs1, _, y1, _ = LC.problem("L16")
p1 = P.HipPlan(topo1, 0)
p1.set_locs(locs1); p1.set_obs(y1.reshape(-1, 1), LC.R)
p1.set_kernel(mt.KIND_MATERN32, 0.02, 1.0, 1.0)
assert "d = 2" in refused(p1, 8, [1.0, 1.0, 1.0, 0.0, 1.0])
p1.close()
topo2 = dataclasses.replace(topo1, coord_dim=2)
p2 = P.HipPlan(topo2, 0)
assert p2.d == 2
p2.set_locs(np.column_stack([locs1, 0.01 * (1.0 + locs1[:, 0])])); p2.set_obs(y1.reshape(-1, 1), LC.R)
p2.set_kernel(8, (1, 1.0), 1.0, 1.0)
kernel_stands(p2, "Local")
p2.close()

# mra_eval_kernel_local checks the same parameters (and launches nothing on a dry run: a good call ends in MRA_ERR_STATE);
# mra_eval_kernel refuses the kind
lib = P.load_library()
D = np.zeros(4); la = np.ones(4); lb = np.ones(4); out = np.zeros(4)
for par, word in BAD:
    par = np.array(par, dtype=np.float64)
    assert lib.mra_eval_kernel_local(_ptr(par), len(par), 2, _ptr(D), _ptr(la), _ptr(lb), 4, _ptr(out)) == -1, par
par = np.array([1.0, 1.0, 1.0, 0.0, 1.0])
assert lib.mra_eval_kernel_local(_ptr(par), 5, 3, _ptr(D), _ptr(la), _ptr(lb), 4, _ptr(out)) == -1          # ds
lb0 = np.array([1.0, 0.0, 1.0, 1.0])
assert lib.mra_eval_kernel_local(_ptr(par), 5, 2, _ptr(D), _ptr(la), _ptr(lb0), 4, _ptr(out)) == -1
assert lib.mra_eval_kernel_local(_ptr(par), 5, 2, _ptr(D), _ptr(la), _ptr(lb), 4, _ptr(out)) == -4
assert lib.mra_eval_kernel(8, _ptr(par), 5, _ptr(D), 4, _ptr(out)) == -1
print("LOCAL_RANGE_OK")
'''


def test_kind_8_on_a_dry_run_plan(built_library, tmp_path):
    child = tmp_path / "child.py"
    child.write_text(CHILD)
    env = dict(os.environ, MRA_ROOT=K.ROOT, MRA_HOST_DRYRUN="1")
    res = subprocess.run([sys.executable, str(child)], env=env, capture_output=True, text=True, timeout=600)
    print(res.stdout[-500:])
    print(res.stderr[-3000:])
    assert res.returncode == 0 and "LOCAL_RANGE_OK" in res.stdout
