"""Who is right where the reference and this implementation disagree?  An 80-bit evaluation of the
same model (oracle/mra_extended.py) says: the float64 level-wise algorithm (the one the GPU runs) is
accurate to ~1e-12, the reference's Matern32 predictive sd is not (explicit inverses + eigh square
root, pyMRA/MRANode.py:444-445, 504-507).  CPU only, small trees."""
import numpy as np
import pytest

import _cases as K
from oracle.mra_extended import run_extended
from oracle.mra_levelwise import run_levelwise


@pytest.mark.parametrize("name", ["g32", "c1", "g64m", "g128m", "u3"])
def test_float64_algorithm_against_extended_precision(name):
    cs = K.load_case(name)
    g = cs["g"]
    ext = run_extended(cs["topo"], cs["locs"], cs["spec"], cs["y_obs"], cs["c"]["R"])
    lw = run_levelwise(cs["topo"], cs["locs"], cs["spec"], cs["y_obs"], cs["c"]["R"])
    hard = name == "u3"
    # (i) the algorithm the GPU executes vs extended-precision truth: meets the 1e-6 bar with margin
    assert abs(lw["lik"] - ext["lik"]) <= (1e-7 if hard else 1e-11) * abs(ext["lik"])
    assert np.max(np.abs(lw["mean"] - ext["mean"])) < (1e-7 if hard else 1e-9)
    assert K.rel(lw["sd"], ext["sd"]) < (1e-6 if hard else 1e-9)
    # (ii) the reference vs the same truth
    ref_sd = K.rel(g["sd"], ext["sd"])
    ref_lik = abs(float(g["lik"]) - ext["lik"]) / abs(ext["lik"])
    if name == "g64m":
        assert ref_sd > 1e-8          # the reference's own sd error is far above rounding here
        assert ref_sd < 1e-5 and ref_lik < 1e-10
    if name == "g128m":
        # 128^2 (SURVEY.md section 7.5's own adjudication size): the reference's sd is off by up to 7e-4, a tenth of the
        # locations by more than north_star's 1e-6, while its likelihood and mean are fine
        e = np.abs(g["sd"] - ext["sd"]) / ext["sd"]
        assert 1e-4 < e.max() < 2e-3 and (e > 1e-6).mean() > 0.05 and ref_lik < 1e-10
        assert np.max(np.abs(np.asarray(g["mean"]).ravel() - ext["mean"])) < 1e-7
    if name == "u3":
        assert ref_lik > 1e-5         # ill-conditioned: the reference is off by ~2e-4 in the likelihood itself
    if name in ("g32", "c1"):
        assert ref_sd < 1e-8 and ref_lik < 1e-10


def test_c3_geometry_subtree_adjudication():
    """C3's own geometry: one level-3 subtree of the 1024^2 tree with pruned ancestors (tests/golden/make_c3_subtree_ext.py).
    The float64 level-wise algorithm reproduces the stored 80-bit results to 1e-9 (sd) on all 16 384 locations; the numbers the
    generating script recorded for the reference's algorithm say where the C3 sd gap comes from."""
    import json
    import os
    import sys
    sys.path.insert(0, K.GOLD)
    import make_c3_subtree_ext as mk
    g = np.load(os.path.join(K.GOLD, "c3_subtree_ext.npz"))
    prm = json.loads(str(g["params"]))
    c, locs, y_obs, lt, red, spec = mk.local_problem(prm["which"])
    assert abs(float(np.nansum(y_obs)) - float(g["y_checksum"])) < 1e-9
    own = lt.perm[lt.in_leaf]
    assert np.array_equal(own, g["own"])
    lw = run_levelwise(lt, locs, spec, y_obs, c["R"], reduce_level=red, allreduce=lambda b: b)
    assert abs(lw["lik"] - float(g["lik"])) <= 1e-12 * abs(float(g["lik"]))
    assert np.max(np.abs(lw["mean"][own] - g["mean"])) < 1e-9
    assert K.rel(lw["sd"][own], g["sd"]) < 1e-9
    assert float(g["ref_alg_sd_rel_max"]) > 1e-5 and float(g["ref_alg_sd_frac_above_1e6"]) > 0.05
    assert float(g["ref_alg_lik_rel"]) < 1e-10


def _spec(kind, **kw):
    import pymra_amd.MRATools as mt
    return mt.KernelSpec(kind, **kw)


@pytest.mark.parametrize("name,spec", [("kanter", _spec(5, l=0.05, scale=1.3)), ("exp_circular", _spec(0, l=0.02, circular=True)),
                                      ("m32_circular", _spec(1, l=0.05, sig=1.2, circular=True)), ("iden", _spec(4, scale=0.7))])
def test_extended_kernel_is_the_host_kernel(name, spec):
    """The 80-bit kernel evaluation against pymra_amd.MRATools' float64 one on 1-D points: equal to rounding, inside and beyond a
    taper's radius, at distance 0, and across the seam of a circular kernel (where the two distances differ by order 1)."""
    from oracle.mra_extended import _kernel
    a = np.concatenate((np.linspace(0.0, 1.0, 41), [0.001, 0.999, 0.5]))[:, None]
    b = np.concatenate((np.linspace(0.0, 1.0, 29), [0.001, 0.9995, 0.5, 0.54]))[:, None]
    ext = np.asarray(_kernel(spec, a, b), dtype=np.float64)
    host = np.asarray(spec.evaluate(a, b), dtype=np.float64)
    assert ext.shape == host.shape == (len(a), len(b))
    # float64 rounds the distance (and 1 - distance round the seam) to 1.1e-16 absolute; the kernels' slope in it is at most ~2 / l
    assert np.abs(ext - host).max() <= 8 * np.finfo(float).eps * max(1.0, 1.0 / spec.l) * spec.scale * spec.sig
    assert ext[-1, -2] == spec.scale * (spec.sig if spec.kind != 4 and spec.kind != 5 and spec.kind != 0 else 1.0)       # distance 0
    if spec.circular:
        flat = np.asarray(_kernel(_spec(spec.kind, l=spec.l, sig=spec.sig), a, b), dtype=np.float64)
        assert abs(ext[-3, -3] - flat[-3, -3]) > 0.5               # 0.001 and 0.9995: 0.0015 apart round the seam, 0.9985 apart on the line
        assert ext[-3, -3] > 0.9 * spec.scale * spec.sig
    if spec.kind == 5:
        assert ext[-1, -1] > 0 and np.all(ext[np.abs(a - b.T) > spec.l] == 0)             # 0.04 apart: inside the radius 0.05
        assert not np.array_equal(ext, np.asarray(_kernel(_spec(4, scale=spec.scale), a, b), dtype=np.float64))


def test_extended_kernel_refuses_what_it_does_not_know():
    """An unknown kind used to be evaluated as Iden, silently: Kanter's likelihood came out 5.6 (relative) off."""
    from oracle.mra_extended import _kernel
    x = np.linspace(0.0, 1.0, 5)[:, None]
    with pytest.raises(ValueError):
        _kernel(_spec(6), x, x)
    with pytest.raises(ValueError):
        _kernel(_spec(-1), x, x)
    with pytest.raises(ValueError):
        _kernel(_spec(0, l=0.1, circular=True), np.zeros((3, 2)), np.zeros((3, 2)))


def test_extended_oracle_on_a_kanter_and_on_a_circular_tree():
    """run_extended against run_levelwise on a small 1-D tree (243 points, r0 = 4, M = 2) with the two kernels it lacked"""
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    np.random.seed(7)
    locs = mt.genLocations(243)
    topo = build_topology(locs, 4, 2, 3)
    rng = np.random.default_rng(0)
    y = np.where(rng.random(243) < 0.5, np.sin(9.0 * locs.ravel()) + 0.1 * rng.standard_normal(243), np.nan)
    for spec in (_spec(5, l=0.2), _spec(0, l=0.1, circular=True)):
        ext = run_extended(topo, locs, spec, y, 1e-2)
        lw = run_levelwise(topo, locs, spec, y, 1e-2)
        good = ext["sd"] > 0
        assert abs(lw["lik"] - ext["lik"]) <= 1e-11 * abs(ext["lik"])
        assert np.max(np.abs(lw["mean"] - ext["mean"])) < 1e-9 and K.rel(lw["sd"][good], ext["sd"][good]) < 1e-9
        assert np.array_equal(lw["sd"] > 0, good)
