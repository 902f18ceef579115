"""The metric of mra_plan_set_metric on the host: KernelSpec.A, the kernels' ``metric=`` keyword, the helpers
aniso2d and ard, and the one thing tests/test_gpu_metric.py leans on - that the level-wise oracle given raw coordinates and a
KernelSpec with A agrees with the oracle given locs @ A.T an order of magnitude inside the bars the GPU is held to against it."""
import os
import re

import numpy as np
import pytest

import _cases as K
import pymra_amd.MRATools as mt
from pymra_amd.MRATree import probe_cov
from pymra_amd.topology import build_topology

BARS = (1e-11, 1e-9, 1e-8)                      # tests/test_gpu_sphere.py: likelihood (relative), mean (absolute), sd (relative)
DYADIC = np.array([[1.0, 0.5], [-0.25, 2.0]])
GENERAL = np.array([[0.9, 0.3], [-1.7, 2.2]])
KERNELS = {"exp": (mt.ExpCovFun, dict(l=0.3)), "m32": (mt.Matern32, dict(l=0.3, sig=1.3)), "m52": (mt.Matern52, dict(l=0.4, sig=0.7)),
           "gauss": (mt.GaussianCovFun, dict(l=0.2, sig=0.8)), "kanter": (mt.KanterCovFun, dict(radius=0.9)), "iden": (mt.Iden, dict(l=1))}


def test_kernelspec_carries_A_through_scaling_and_probing():
    A = mt.aniso2d(3.0, 30.0)
    s = mt.KernelSpec(mt.KIND_MATERN32, 0.3, 1.0, A=A)
    for t in (s * 2.5, 2.5 * s, s / 4.0):
        assert np.array_equal(t.A, A) and t.kind == s.kind and t.l == s.l
    assert (s * 2.5).scale == 2.5 and mt.KernelSpec(mt.KIND_EXP, 0.3).A is None
    assert "A=" in repr(s) and "A=" not in repr(mt.KernelSpec(mt.KIND_EXP, 0.3))
    for name, (fn, kw) in KERNELS.items():
        p = probe_cov(lambda a, b: 1.5 * fn(a, b, metric=A, **kw), 2, np.zeros((4, 2)))
        assert p is not None and np.array_equal(p.A, A) and p.scale == 1.5, name
        assert probe_cov(lambda a, b: fn(a, b, **kw), 2, np.zeros((4, 2))).A is None
    A[0, 0] = 99.0                                             # the spec holds a copy
    assert s.A[0, 0] != 99.0
    with pytest.raises(ValueError, match="d x d"):
        mt.KernelSpec(mt.KIND_EXP, 0.3, A=np.ones((2, 3)))


@pytest.mark.parametrize("name", list(KERNELS))
def test_array_path_with_metric_is_the_kernel_on_transformed_locations(name):
    fn, kw = KERNELS[name]
    rng = np.random.default_rng(0)
    a, b = rng.uniform(size=(40, 2)), rng.uniform(size=(25, 2))
    for A, tol in ((DYADIC, 0.0), (GENERAL, 1e-15)):
        for second in (b, None):
            got = np.asarray(fn(a, b, metric=A, **kw) if second is not None else fn(a, metric=A, **kw))
            want = np.asarray(fn(a @ A.T, b @ A.T, **kw) if second is not None else fn(a @ A.T, **kw))
            assert got.shape == want.shape and np.max(np.abs(got - want)) <= tol
    spec = probe_cov(lambda x, y: fn(x, y, metric=GENERAL, **kw), 2, a)
    assert np.max(np.abs(spec.evaluate(a, b) - np.asarray(fn(a @ GENERAL.T, b @ GENERAL.T, **kw)))) <= 1e-15
    with pytest.raises(ValueError, match="3 x 3"):
        fn(a, b, metric=np.eye(3), **kw)


def test_aniso2d_and_ard():
    rng = np.random.default_rng(1)
    x = rng.uniform(size=(30, 2))
    for angle in (0.0, 30.0, 117.0):
        Q = mt.aniso2d(1.0, angle)                            # ratio 1: a rotation, distances unchanged
        assert np.allclose(Q @ Q.T, np.eye(2), atol=1e-15)
        assert np.max(np.abs(np.asarray(mt.dist(x @ Q.T)) - np.asarray(mt.dist(x)))) <= 1e-15
    A = mt.aniso2d(3.0, 30.0)
    u = np.array([np.cos(np.pi / 6), np.sin(np.pi / 6)])
    v = np.array([-u[1], u[0]])
    assert abs(np.linalg.norm(A @ u) - 1.0) <= 1e-15          # along the major axis: range l
    assert abs(np.linalg.norm(A @ v) - 3.0) <= 1e-15          # across it: range l / ratio
    assert np.allclose(mt.aniso2d(3.0, np.pi / 6, degrees=False), A, atol=1e-16)
    l = 0.4
    along = mt.ExpCovFun(np.zeros((1, 2)), (l * u)[None, :], l=l, metric=A)[0, 0]
    across = mt.ExpCovFun(np.zeros((1, 2)), (l / 3.0 * v)[None, :], l=l, metric=A)[0, 0]
    assert abs(along - np.exp(-1.0)) <= 1e-15 and abs(across - np.exp(-1.0)) <= 1e-15
    assert np.array_equal(mt.ard([0.5, 0.25, 2.0]), np.diag([2.0, 4.0, 0.5]))
    st = mt.ExpCovFun(np.zeros((1, 3)), np.array([[0.0, 0.0, 2.0]]), l=1, metric=mt.ard([0.5, 0.25, 2.0]))[0, 0]
    assert abs(st - np.exp(-1.0)) <= 1e-15                    # the temporal range of a space-time kernel
    for bad in (lambda: mt.aniso2d(0.0, 10.0), lambda: mt.ard([1.0, -1.0]), lambda: mt.ard([])):
        with pytest.raises(ValueError):
            bad()


def test_metric_with_circular_is_refused():
    x = np.linspace(0.0, 1.0, 7).reshape(-1, 1)
    for fn, kw in KERNELS.values():
        with pytest.raises(ValueError, match="circular"):
            fn(x, x, circular=True, metric=np.array([[2.0]]), **kw)
    with pytest.raises(ValueError, match="circular"):
        mt.KernelSpec(mt.KIND_EXP, 0.3, circular=True, A=np.array([[2.0]]))
    assert mt.KernelSpec(mt.KIND_EXP, 0.3, circular=True).circular


@pytest.mark.parametrize("which", ["aniso", "ard"])
def test_oracle_on_raw_coordinates_with_A_is_the_oracle_on_transformed_coordinates(which):
    """the coordinate rounding of locs @ A.T against the device's fma rows, as the oracle sees it: an order of magnitude inside BARS"""
    from oracle.mra_levelwise import run_levelwise
    A, l = {"aniso": (mt.aniso2d(3.0, 30.0), 0.5), "ard": (mt.ard([0.3, 0.1]), 1.0)}[which]
    n = 32
    locs = mt.genLocations2d(Nx=n, Ny=n)
    np.random.seed(7)
    topo = build_topology(locs, 16, 2, 4)
    rng = np.random.default_rng(0)
    y = np.where(rng.random(n * n) < 0.4, np.sin(3.0 * locs[:, 0]) + 0.1 * rng.standard_normal(n * n), np.nan)
    a = run_levelwise(topo, locs, mt.KernelSpec(mt.KIND_MATERN32, l, 1.0, A=A), y, 1e-2)
    # the device's coordinates: fma rows (math.fma needs Python 3.13; two-term rows in longdouble round once, as fma does)
    T = np.empty_like(locs)
    for i in range(2):
        T[:, i] = (np.longdouble(A[i, 0]) * locs[:, 0] + np.longdouble(A[i, 1]) * locs[:, 1]).astype(np.float64)
    for coords in (locs @ A.T, T):
        b = run_levelwise(topo, coords, mt.KernelSpec(mt.KIND_MATERN32, l, 1.0), y, 1e-2)
        e = (abs(a["lik"] - b["lik"]) / abs(b["lik"]), float(np.max(np.abs(a["mean"] - b["mean"]))),
             float(np.max(np.abs(a["sd"] - b["sd"]) / np.maximum(b["sd"], 1e-300))))
        print("%s: lik %.2e mean %.2e sd %.2e" % (which, *e))
        assert e[0] <= BARS[0] / 10 and e[1] <= BARS[1] / 10 and e[2] <= BARS[2] / 10


def test_header_declares_mra_plan_set_metric():
    text = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    assert re.search(r"^int mra_plan_set_metric\(mra_plan \*plan, const double \*A\);", text, re.M)
    from pymra_amd import plan
    assert "mra_plan_set_metric" in plan.EXPORTS
