"""Covariances evaluated on 3-D coordinates: MRA on the sphere.  GPU only.

The tree is partitioned on (lon, lat); the kernels see the points' xyz, so the covariance is a function of the chordal distance.
Geometry unless noted: lon in [-180, 180) with a half-cell offset, lat in [-80, 80], radius 1, R = 1e-2, 40 % observed plus one
leaf without any observation.

 1. parity with the level-wise oracle (run on the same topology with the xyz coordinates) at the smallest trees that reach each
    kernel: 64x64 / r0 16 / M 2 (fused path: k_knot_chain, the stage-all row cascade, k_leaf_gemm) and the same tree level by level
    (k_gemm_nt* COV, the one-launch prior levels), 80x80 / 16 / 3 (leaves under 128 rows); likelihood + predict and likelihood-only;
    six covariance families on the first tree.  The two 128x128 trees (CWT = 2 and 4) take the oracle 5 - 7 s each, so they are
    held to the same tree's MRA_KERNEL_HOST plan instead (3.)
 2. 3000 scattered points (the general partitioner, irregular leaves)
 3. device kernel against host blocks (spec.evaluate on xyz through MRA_KERNEL_HOST) on every tree of 1., CWT = 2 and 4 and the
    deep 64-wide tree (PassPath::Hi): likelihood + predict and likelihood-only, fused, with the knot chain off (k_prior_cascade in
    knot mode, n_chain == 0) and level by level; the row cascade with its operands staged level by level (CWT = 4 with four levels
    against host blocks, CWT = 2 with seven levels against the level-by-level kernels)
 4. rotation invariance - which no planar treatment has - and the planar treatment of the same data, more than 1 % away
 5. M = 0 is exact kriging on the chordal distance
 6. the calls on the retained factors, each against its CPU restatement with xyz   7. a noise vector, a Poisson Laplace fit
 8. sharded passes   9. the MRATree facade   10. refusals   11. a 2-D plan before and after a 3-D plan lived in the process

Bars: likelihood 1e-11 relative, mean 1e-9 absolute, sd 1e-8 relative against the oracle (BARS); for the other calls the bars of
their own 2-D GPU tests, cited where they are used.  None is derived from a result of the code under test."""
import dataclasses
import functools

import numpy as np
import pytest

import _cases as K
import pymra_amd.MRATools as mt
from pymra_amd.topology import build_topology

pytestmark = pytest.mark.gpu

R = 1e-2
BARS = (1e-11, 1e-9, 1e-8)                      # likelihood (relative), mean (absolute), sd (relative)
HOST_BARS = (1e-11, 1e-9, 1e-8)                 # tests/test_gpu_hostcov.py: stationary callable vs device kernel
M32 = mt.KernelSpec(mt.KIND_MATERN32, 0.5)
FAMILIES = {"exp": mt.KernelSpec(mt.KIND_EXP, 0.5), "m32": M32, "m52": mt.KernelSpec(mt.KIND_MATERN52, 0.5, 1.3),
            "gauss": mt.KernelSpec(mt.KIND_GAUSSIAN, 0.3, 0.8), "kanter": mt.KernelSpec(mt.KIND_KANTER, 0.8),
            "iden": mt.KernelSpec(mt.KIND_IDEN, 1.0, 1.0, scale=0.7)}


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def lonlat_grid(nx, ny):
    lon = -180.0 + (np.arange(nx) + 0.5) * 360.0 / nx
    lat = np.linspace(-80.0, 80.0, ny)
    g, h = np.meshgrid(lon, lat)
    return np.column_stack((g.ravel(), h.ravel()))


def _leaf_callers(topo, i):
    p = topo.perm[int(topo.node_row0[i]):int(topo.node_row1[i])]
    return p[p >= 0]


def _data(topo, xyz, seed=0):
    """a smooth function of the position on the sphere plus noise of variance R, 40 % observed, and the first leaf without any
    observation"""
    rng = np.random.default_rng(seed)
    N = len(xyz)
    obs = rng.random(N) < 0.4
    obs[_leaf_callers(topo, int(np.nonzero(topo.node_leaf)[0][0]))] = False
    x, y, z = xyz.T
    f = np.sin(3.0 * x) + y * z + 0.5 * np.cos(2.0 * z + x)
    return np.where(obs, f + np.sqrt(R) * rng.standard_normal(N), np.nan)


@functools.lru_cache(maxsize=None)
def tree(n, r, M, scattered=False):
    """(lonlat, xyz, topology with coord_dim = 3, y)"""
    if scattered:
        rng = np.random.default_rng(12)
        ll = np.column_stack((rng.uniform(-180.0, 180.0, n), np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n)))))     # uniform on the sphere
    else:
        ll = lonlat_grid(n, n)
    np.random.seed(7)
    topo = build_topology(ll, r, M, 4, coord_dim=3)
    xyz = mt.lonlat_to_xyz(ll)
    return ll, xyz, topo, _data(topo, xyz)


@functools.lru_cache(maxsize=None)
def oracle(n, r, M, fam="m32", scattered=False):
    from oracle.mra_levelwise import run_levelwise
    ll, xyz, topo, y = tree(n, r, M, scattered)
    return run_levelwise(topo, xyz, FAMILIES[fam], y, R)


def make_plan(hip, topo, coords, y, spec, noise=R, opts=()):
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(coords)
    pl.set_obs(y, noise)
    pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
    for o, v in opts:
        pl.set_option(o, v)
    return pl


def predict_pass(pl):
    pl.run(True, True)
    mean, _, sd = pl.predict(with_sd=True)
    return sum(pl.likelihood()), mean.copy(), sd.copy()


def errors(got, ref):
    lik, mean, sd = got
    return (abs(lik - ref[0]) / abs(ref[0]), float(np.max(np.abs(mean - ref[1]))),
            float(np.max(np.abs(sd - ref[2]) / np.maximum(np.abs(ref[2]), 1e-300))))


def check(got, ref, bars, tag):
    e = errors(got, ref)
    print("%s: lik %.2e mean %.2e sd %.2e" % (tag, *e))
    assert e[0] <= bars[0], "%s: likelihood rel err %.3e" % (tag, e[0])
    assert e[1] <= bars[1], "%s: mean abs err %.3e" % (tag, e[1])
    assert e[2] <= bars[2], "%s: sd rel err %.3e" % (tag, e[2])


def ref3(ref):
    return ref["lik"], ref["mean"], ref["sd"]


def both_passes(pl, ref, bars, tag):
    """likelihood + predict against ref, then the likelihood-only pass (its own route: gathered tiles of observed rows, C by the
    sym_diag product) against the same likelihood"""
    got = predict_pass(pl)
    route = pl.route()
    check(got, ref, bars, tag)
    pl.run(True, False)
    lik = sum(pl.likelihood())
    e = abs(lik - ref[0]) / abs(ref[0])
    print("%s, likelihood only: %.2e (lik_rows=%s lik_general=%s)" % (tag, e, pl.route()["lik_rows"], pl.route()["lik_general"]))
    assert e <= bars[0], "%s: likelihood-only rel err %.3e" % (tag, e)
    return got, route, pl.route()


# ---- 1. parity with the oracle -----------------------------------------------------------------------------------------------------------
TREES = {"g64": (64, 16, 2), "g80": (80, 16, 3), "g128w2": (128, 32, 3), "g128w4": (128, 64, 3)}


@pytest.mark.parametrize("key,fused", [("g64", 1), ("g64", 0), ("g80", 1), ("g80", 0)])
def test_parity_with_the_oracle(hip, key, fused):
    ll, xyz, topo, y = tree(*TREES[key])
    pl = make_plan(hip, topo, xyz, y, M32, opts=((hip.MRA_OPT_FUSED, fused),))
    assert pl.d == 3 and topo.d == 2
    _, route, route_lik = both_passes(pl, ref3(oracle(*TREES[key])), BARS, "%s fused=%d" % (key, fused))
    print("%s fused=%d route: %s" % (key, fused, {k: route[k] for k in ("path", "n_chain", "prior_level", "leaf_resident")}))
    assert route["path"] == ("Fused" if fused else "Levels")
    if fused:
        assert route["n_chain"] >= 2 and route_lik["lik_rows"]          # k_knot_chain; the stage-all row cascade on gathered tiles
    else:
        assert route["prior_level"] and route_lik["lik_general"]        # the one-launch prior levels
    if key == "g64":
        assert route["leaf_resident"]                                   # k_leaf_gemm
    else:
        leaf_rows = np.asarray(topo.node_row1 - topo.node_row0)[np.asarray(topo.node_leaf, dtype=bool)]
        assert not route["leaf_resident"] and int(leaf_rows.max()) < 128
    pl.close()


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_every_covariance_family(hip, fam):
    ll, xyz, topo, y = tree(*TREES["g64"])
    ref = ref3(oracle(*TREES["g64"], fam=fam))
    pl = make_plan(hip, topo, xyz, y, FAMILIES[fam])
    both_passes(pl, ref, BARS, "g64 %s fused" % fam)
    pl.set_option(hip.MRA_OPT_FUSED, 0)
    both_passes(pl, ref, BARS, "g64 %s level by level" % fam)
    pl.close()


# ---- 2. scattered points ------------------------------------------------------------------------------------------------------------------
def test_scattered_points(hip):
    ll, xyz, topo, y = tree(3000, 20, 2, True)
    sizes = np.asarray(topo.node_row1 - topo.node_row0)[np.asarray(topo.node_leaf, dtype=bool)]
    assert len(set(sizes.tolist())) > 1                                  # irregular leaves
    pl = make_plan(hip, topo, xyz, y, M32)
    both_passes(pl, ref3(oracle(3000, 20, 2, scattered=True)), BARS, "3000 scattered points")
    pl.close()


# ---- 3. device kernel against host blocks --------------------------------------------------------------------------------------------------
def _host_against_device(hip, ll, xyz, topo, y, tag, expect_path=None, stage_all=True):
    from pymra_amd.MRATree import probe_cov
    opaque = lambda a, b: np.asarray(M32.evaluate(a, b), dtype=np.float64) + 0.0      # noqa: E731
    assert probe_cov(opaque, 3, xyz) is None
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(xyz); pl.set_obs(y, R); pl.upload_host_cov(opaque, xyz, y)
    host = predict_pass(pl)
    assert pl.route()["path"] == "Levels"
    pl.set_kernel(M32.kind, M32.l, M32.sig, M32.scale)
    _, route, route_lik = both_passes(pl, host, HOST_BARS, "%s: device vs host blocks" % tag)
    print("%s: route %s, likelihood only lik_rows=%s" % (tag, {k: route[k] for k in ("path", "n_chain", "leaf_resident")}, route_lik["lik_rows"]))
    if expect_path:
        assert route["path"] == expect_path, route["path"]
    if expect_path == "Fused" and stage_all:
        assert route["n_chain"] >= 2 and route_lik["lik_rows"]          # k_knot_chain; gathered tiles through the stage-all row cascade
    elif expect_path == "Fused":
        assert route["n_chain"] == 0 and not route_lik["lik_rows"]      # operands beyond the LDS: no knot chain, no gathered tiles
    # the knot pass level by level: k_prior_cascade in knot mode with its tail (kInv, factor, inverted diagonal blocks) in the launch
    pl.set_option(hip.MRA_OPT_KNOT_CHAIN, 0)
    _, route, _ = both_passes(pl, host, HOST_BARS, "%s: device, knot chain off, vs host blocks" % tag)
    assert route["n_chain"] == 0 and (not expect_path or route["path"] == expect_path)
    pl.set_option(hip.MRA_OPT_KNOT_CHAIN, 1)
    pl.set_option(hip.MRA_OPT_FUSED, 0)
    _, route, route_lik = both_passes(pl, host, HOST_BARS, "%s: device (level by level) vs host blocks" % tag)
    assert route["path"] == "Levels" and route["prior_level"] and route_lik["lik_general"]       # the one-launch prior levels, gathered rows
    pl.close()


@pytest.mark.parametrize("key", list(TREES))
def test_device_kernel_against_host_blocks(hip, key):
    ll, xyz, topo, y = tree(*TREES[key])
    if key.startswith("g128"):
        assert int(topo.cw[0]) == (32 if key == "g128w2" else 64)       # CWT = 2 and 4
    _host_against_device(hip, ll, xyz, topo, y, key, "Fused")


def test_device_kernel_against_host_blocks_deep_wide_tree(hip):
    ll, xyz, topo, y = tree(256, 64, 5)
    _host_against_device(hip, ll, xyz, topo, y, "256x256 r0=64 M=5", "Hi")


def _row_cascade_launches(pl):
    return sum(k["launches"] for k in pl.kernel_stats() if "k_prior_cascade row pass" in k["name"])


def test_staged_row_cascade_four_tiles_wide(hip):
    """k_prior_cascade<4, 4, 3, *, false>: with CWT = 4 and four levels above the leaves the operands of all levels take
    (16 * 6 + 4 * 10) tiles * 2 KB = 272 KB, more than the 160 KB of LDS, so the row cascade stages them level by level"""
    ll, xyz, topo, y = tree(256, 64, 4)
    assert int(topo.cw[0]) == 64 and topo.n_levels == 5
    _host_against_device(hip, ll, xyz, topo, y, "256x256 r0=64 M=4", "Fused", stage_all=False)
    pl = make_plan(hip, topo, xyz, y, M32, opts=((hip.MRA_OPT_KERNEL_TIMING, 1),))
    predict_pass(pl)
    assert _row_cascade_launches(pl) > 0
    pl.close()


def test_staged_row_cascade_two_tiles_wide_seven_levels(hip):
    """k_prior_cascade<2, 8, 3, *, false>: CWT = 2 and seven levels above the leaves, (4 * 21 + 7 * 3) tiles * 2 KB = 210 KB.  A tree
    of this depth is too large for the oracle and for host blocks in a test: the fused pass against the level-by-level kernels
    of the same plan (held to the oracle and to host blocks on the smaller trees), at the bars
    tests/test_gpu_parity.py::test_fused_cascades_at_every_depth uses for the same comparison in 2-D"""
    ll, xyz, topo, y = tree(768, 32, 7)
    assert [int(v) for v in np.diff(topo.level_ptr)] == [4 ** k for k in range(8)] and int(topo.cw[0]) == 32
    pl = make_plan(hip, topo, xyz, y, M32, opts=((hip.MRA_OPT_KERNEL_TIMING, 1),))
    fused = predict_pass(pl)
    assert pl.route()["path"] == "Fused" and _row_cascade_launches(pl) > 0
    pl.set_option(hip.MRA_OPT_FUSED, 0)
    lev = predict_pass(pl)
    assert pl.route()["path"] == "Levels"
    check(fused, lev, (1e-11, 1e-9, 1e-8), "768x768 r0=32 M=7: fused (staged row cascade) vs level by level")
    pl.close()


# ---- 4. rotation invariance ------------------------------------------------------------------------------------------------------------------
def test_rotation_invariance_and_the_planar_treatment(hip):
    ll, xyz, topo, y = tree(*TREES["g64"])
    a, b = np.radians(77.0), np.radians(40.0)
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    pl = make_plan(hip, topo, xyz, y, M32)
    base = predict_pass(pl)
    pl.set_locs(np.ascontiguousarray(xyz @ (Rx @ Rz).T))
    rot = predict_pass(pl)
    pl.close()
    e_l, e_m = abs(rot[0] - base[0]) / abs(base[0]), float(np.max(np.abs(rot[1] - base[1])))
    print("rotated by 77 deg about z, 40 deg about x: lik %.2e mean %.2e" % (e_l, e_m))
    assert e_l <= 1e-11 and e_m <= 1e-9
    flat = make_plan(hip, dataclasses.replace(topo, coord_dim=0), ll / 180.0, y, M32)
    assert flat.d == 2
    planar = predict_pass(flat)
    flat.close()
    print("planar lon/lat/180: lik %.6f against chordal %.6f" % (planar[0], base[0]))
    assert abs(planar[0] - base[0]) > 1e-2 * abs(base[0])


# ---- 5. M = 0 is exact kriging -------------------------------------------------------------------------------------------------------------
def test_a_single_node_is_exact_kriging_on_the_chord(hip):
    ll = lonlat_grid(20, 20)
    xyz = mt.lonlat_to_xyz(ll)
    topo = build_topology(ll, 16, 0, 4, coord_dim=3)
    assert topo.n_nodes == 1
    rng = np.random.default_rng(4)
    y = np.where(rng.random(400) < 0.4, rng.standard_normal(400), np.nan)
    pl = make_plan(hip, topo, xyz, y, M32)
    got = predict_pass(pl)
    pl.close()
    lik, mean, sd = K.kriging(xyz, y, M32, R)
    e = errors(got, (lik, mean, sd))
    print("M = 0 against kriging: lik %.2e mean %.2e sd %.2e" % e)
    assert e[0] <= 1e-9 and e[1] < 1e-9 and e[2] < 1e-8               # test_mratree_reproduces_exact_kriging


# ---- 6. the calls on the retained factors -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_tree(hip):
    import pymra_amd
    ll, xyz, topo, y = tree(*TREES["g64"])
    np.random.seed(7)
    t = pymra_amd.MRATree(ll, 16, lambda a, b: mt.Matern32(a, b, l=0.5), y.reshape(-1, 1), R, M=2, J=4, metric="chordal")
    for f in ("perm", "src", "knot_rows", "node_row0"):
        assert np.array_equal(getattr(t.topology, f), getattr(topo, f)), f
    return t


@functools.lru_cache(maxsize=None)
def site_state():
    import _treesites as TS
    ll, xyz, topo, y = tree(*TREES["g64"])
    return TS.SiteState(topo, xyz, M32, y, R)


def _off_tree_sites():
    """40 sites (lon, lat) off the grid; the first three: 0.1 degree either side of the date line and one 5 degrees away"""
    rng = np.random.default_rng(9)
    s = np.column_stack((rng.uniform(-180.0, 180.0, 40), rng.uniform(-79.0, 79.0, 40)))
    s[0], s[1], s[2] = (179.9, 11.3), (-179.9, 11.3), (174.9, 11.3)
    return s


def test_solve_17_columns(hip, sphere_tree):
    import _treesolve as TSV
    ll, xyz, topo, y = tree(*TREES["g64"])
    Y = np.random.default_rng(1).standard_normal((len(y), 17))
    Y[:, 0] = np.nan_to_num(y)
    mean, quad = sphere_tree.solve(Y)
    want_mean, want_quad = TSV.tree_solve(topo, xyz, M32, y, R, Y)
    e_m = float(np.abs(mean - want_mean).max())
    blk = np.arange(17)[:, None] // 16 == np.arange(17)[None, :] // 16
    e_q = float(np.abs(quad - want_quad)[blk].max())
    print("solve: mean %.2e quad %.2e (scale %.1f)" % (e_m, e_q, np.abs(np.diag(want_quad)).max()))
    assert np.all(np.isnan(quad[~blk]))
    assert e_m <= 1e-9 * max(1.0, np.abs(want_mean).max())          # tests/test_gpu_solve.py
    assert e_q <= 1e-9 * np.abs(np.diag(want_quad)).max()


@pytest.mark.parametrize("distr", ["prior", "posterior"])
def test_covariance_columns(hip, sphere_tree, distr):
    import _treecov as TCV
    ll, xyz, topo, y = tree(*TREES["g64"])
    rows = np.array([0, 63, 64 * 31 + 5, 64 * 64 - 1, 1234])          # both sides of the date line, both edges in latitude
    A = np.zeros((len(y), len(rows)))
    A[rows, np.arange(len(rows))] = 1.0
    want, _ = TCV.tree_cov(topo, xyz, M32, y, R, A, posterior=(distr == "posterior"))
    got = sphere_tree.covariance(rows, distr)
    err = float(np.abs(got - want).max())
    print("covariance(%s): %.2e" % (distr, err))
    assert err <= 1e-9 * M32.sig * M32.scale                          # tests/test_gpu_cov.py: tol * the largest prior variance


def test_predictAt(hip, sphere_tree):
    import _treesites as TS
    ll, xyz, topo, y = tree(*TREES["g64"])
    t = sphere_tree
    xP, sdP = t.predict()
    own = np.arange(0, len(ll), 7)
    m, sd = t.predictAt(ll[own])
    assert np.abs(m[:, 0] - np.asarray(xP).ravel()[own]).max() <= 1e-8 * max(1.0, np.abs(xP).max())        # tests/test_gpu_sites.py
    assert np.abs(sd ** 2 - sdP[own] ** 2).max() <= 1e-9
    sites = _off_tree_sites()
    leaf = t.locate(sites)
    m, sd = t.predictAt(sites, leaf=leaf)
    want_m, want_v = TS.tree_sites(topo, xyz, M32, y, R, mt.lonlat_to_xyz(sites), leaf, state=site_state())
    e_m, e_v = float(np.abs(m - want_m).max()), float(np.abs(sd ** 2 - want_v).max())
    print("predictAt, 40 off-tree sites: mean %.2e var %.2e" % (e_m, e_v))
    assert e_m <= 1e-8 * max(1.0, np.abs(want_m).max()) and e_v <= 1e-9
    assert leaf[0] != leaf[1] and topo.node_parent[leaf[0]] != topo.node_parent[leaf[1]]      # +-179.9: opposite ends of the tree
    with pytest.raises(ValueError):
        t.predictAt(mt.lonlat_to_xyz(sites))                          # under metric="chordal" the sites are (lon, lat)


def test_the_date_line_is_no_edge_of_the_field(hip):
    """Sites 0.1 degree either side of the date line lie in leaves at opposite ends of the tree, yet their means differ by less than
    either differs from the sites 5 degrees east and west of the line - at six latitudes, in the CPU restatement and on the device.

    An MRA has a jump of the order of the posterior sd (0.1 - 0.3 here) across every partition boundary, the date line being one,
    so the statement is about a field whose change over 5 degrees is well above that: 10 cos(lat) sin(lon), which changes by
    0.87 cos(lat) >= 0.59 over 5 degrees of longitude at the line for |lat| <= 47; same tree, mask, R and kernel as above."""
    import _treesites as TS
    import pymra_amd
    ll, xyz, topo, y0 = tree(*TREES["g64"])
    y = np.where(np.isfinite(y0), 10.0 * xyz[:, 1] + np.sqrt(R) * np.random.default_rng(21).standard_normal(len(xyz)), np.nan)
    np.random.seed(7)
    t = pymra_amd.MRATree(ll, 16, lambda a, b: mt.Matern32(a, b, l=0.5), y.reshape(-1, 1), R, M=2, J=4, metric="chordal", want_predict=False)
    assert np.array_equal(t.topology.perm, topo.perm)
    lats = np.array([-41.0, -23.0, -7.0, 11.3, 29.0, 47.0])
    sites = np.concatenate([np.column_stack((np.full(len(lats), lon), lats)) for lon in (179.9, -179.9, 174.9, -174.9)])
    leaf = t.locate(sites)
    m, _ = t.predictAt(sites, leaf=leaf)
    want, _ = TS.tree_sites(topo, xyz, M32, y, R, mt.lonlat_to_xyz(sites), leaf)
    assert np.abs(m - want).max() <= 1e-8 * max(1.0, np.abs(want).max())
    n = len(lats)
    assert np.all(topo.node_parent[leaf[:n]] != topo.node_parent[leaf[n:2 * n]])
    for name, v in (("CPU restatement", want[:, 0].reshape(4, n)), ("device", m[:, 0].reshape(4, n))):
        pair = np.abs(v[0] - v[1])
        away = np.min([np.abs(v[a] - v[b]) for a in (0, 1) for b in (2, 3)], axis=0)
        print("%s: |m(179.9) - m(-179.9)| %s, least difference from a site 5 degrees away %s" % (name, np.round(pair, 4), np.round(away, 4)))
        assert np.all(pair < away), name


def test_covarianceAt_and_simulateAt(hip, sphere_tree):
    import _treesitecov as TC
    t = sphere_tree
    sites = _off_tree_sites()
    leaf = t.locate(sites)
    sx = mt.lonlat_to_xyz(sites)
    for distr in ("prior", "posterior"):
        S = t.covarianceAt(sites, distr, leaf=leaf)
        assert np.array_equal(S, S.T)
        want = TC.tree_sites_cov(site_state(), sx, leaf, distr == "posterior")
        err = float(np.abs(S - want).max())
        print("covarianceAt(%s): %.2e" % (distr, err))
        assert err <= 1e-9                                            # tests/test_gpu_sitecov.py: _post_tol * scale, scale 1
        x = t.simulateAt(sites, len(sites), distr, leaf=leaf, z=np.eye(len(sites)))
        mean = t.predictAt(sites, leaf=leaf)[0] if distr == "posterior" else 0.0
        F = x - mean
        assert np.abs(F @ F.T - S).max() <= 1e-12                     # the symmetric square root of S itself
    sd = t.predictAt(sites, leaf=leaf)[1]
    assert np.abs(np.diag(t.covarianceAt(sites, "posterior", leaf=leaf)) - sd ** 2).max() <= 1e-9


def test_sampleAt_with_given_draws(hip, sphere_tree):
    import _treesitedraw as TD
    t = sphere_tree
    sites = _off_tree_sites()
    leaf = t.locate(sites)
    sx = mt.lonlat_to_xyz(sites)
    slots = t.plan.sample_sites_slots(len(sites))
    z = np.random.default_rng(3).standard_normal((slots, 3))
    for distr in ("prior", "posterior"):
        F, _ = TD.site_draw_factor(site_state(), sx, leaf, distr == "posterior")
        assert F.shape == (len(sites), slots)
        mean = t.predictAt(sites, leaf=leaf)[0] if distr == "posterior" else 0.0
        x = t.sampleAt(sites, 3, distr, leaf=leaf, z=z)
        err = np.abs(x - (mean + F @ z))
        # tests/test_gpu_sitedraw.py holds every entry of F to 1e-9 of the prior variance (1 here): F z within 1e-9 sum_k |z_k|
        assert np.all(err <= 1e-9 * np.abs(z).sum(axis=0)[None, :]), err.max()
        print("sampleAt(%s): %.2e" % (distr, err.max()))
    a = t.sampleAt(sites, 5, seed=11)
    assert np.array_equal(a, t.sampleAt(sites, 5, seed=11)) and a.shape == (len(sites), 5)


def test_simulate_factor_is_the_prior_covariance(hip, sphere_tree):
    """plan.sample with unit draws on the slots one leaf reads: G G^T is the MRA prior covariance of the leaf's rows (the restatement
    of mra_cov_apply with xyz), and a zero draw of the posterior is the predictive mean"""
    import _sampling as SM
    import _treecov as TCV
    ll, xyz, topo, y = tree(*TREES["g64"])
    t = sphere_tree
    j = int(np.nonzero(topo.node_leaf)[0][5])
    prow = np.arange(int(topo.node_row0[j]), int(topo.node_row1[j]))
    prow = prow[SM.reported(topo)[prow]][::9]
    G, _ = SM.factor_columns(t.plan, SM.chain_slots(topo, j), rows=prow)
    A = np.zeros((len(y), len(prow)))
    A[topo.perm[prow], np.arange(len(prow))] = 1.0
    want = TCV.tree_cov(topo, xyz, M32, y, R, A)[0][topo.perm[prow]]
    err = float(np.abs(G @ G.T - want).max())
    print("simulate: G G^T against the prior covariance of %d rows of a leaf: %.2e" % (len(prow), err))
    assert err <= 1e-9                                                # tests/test_gpu_sample.py: tol * scale
    x0 = t.plan.sample(1, z=np.zeros((1, t.plan.sample_slots())), conditional=True)[0]
    rep = SM.reported(topo)
    assert np.abs(x0[rep] - np.asarray(t.predict()[0]).ravel()[topo.perm[rep]]).max() <= 1e-8
    s = t.simulate(2, "posterior", seed=5)
    assert s.shape == (len(y), 2) and np.all(np.isfinite(s))


# ---- 7. noise vector, Laplace -------------------------------------------------------------------------------------------------------------
def test_noise_vector_against_the_rescaled_oracle(hip):
    import _noise as NZ
    import pymra_amd
    ll, xyz, topo, y = tree(*TREES["g64"])
    r = NZ.noise_of(xyz, R)
    assert r.max() > 4.0 * r.min()
    ref = NZ.scaled_oracle(topo, xyz, M32, y.reshape(-1, 1), R)
    np.random.seed(7)
    t = pymra_amd.MRATree(ll, 16, lambda a, b: mt.Matern32(a, b, l=0.5), y.reshape(-1, 1), R, M=2, J=4, metric="chordal", want_predict=False)
    lik = float(t.setNoise(r, want_predict=True)[0, 0])
    xP, sdP = t.predict()
    check((lik, np.asarray(xP).ravel(), sdP), ref3(ref), (1e-10, 1e-9, 1e-8), "setNoise(r) vs the rescaled oracle on xyz")      # ORACLE_BARS
    back = float(t.setNoise(R, want_predict=True)[0, 0])
    assert abs(back - oracle(*TREES["g64"])["lik"]) <= 1e-10 * abs(back)


def test_poisson_laplace_fit(hip):
    import _laplace as LP
    import _noise as NZ
    import pymra_amd
    ll, xyz, topo, y = tree(*TREES["g64"])
    obs = np.isfinite(y)
    z, aux, offset = LP.inputs(xyz, obs, LP.POISSON)
    Sigma = NZ.prior_cov(topo, xyz, M32, y)
    ref = LP.dense_laplace(Sigma, obs & NZ.reported(topo), LP.POISSON, z, aux, offset)
    np.random.seed(7)
    t = pymra_amd.MRATree(ll, 16, lambda a, b: mt.Matern32(a, b, l=0.5), np.where(obs, 0.0, np.nan).reshape(-1, 1), R, M=2, J=4,
                          cov_locs=xyz, want_predict=False)
    lik = t.fitLaplace("poisson", offset=offset, z=z)
    xP, sdP = t.predict()
    print("poisson: passes %d (dense %d), -2 log q %.8f vs %.8f" % (t.laplace["passes"], ref["info"][5], lik, ref["lik"]))
    check((lik, np.asarray(xP).ravel(), sdP), (ref["lik"], ref["mean"], ref["sd"]), (1e-10, 1e-9, 1e-8), "fitLaplace vs the dense Newton")
    assert t.laplace["converged"] and t.laplace["passes"] == int(ref["info"][5])


# ---- 8. sharded ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
def test_sharded(hip, world):
    ll, xyz, topo, y = tree(128, 16, 4)
    pl = make_plan(hip, topo, xyz, y, M32)
    pl.run(True, True)
    lik = sum(pl.likelihood())
    mean, var = pl.predict()
    pl.close()
    liks, m, v, _ = K.emulate_world_on_one_gpu(hip, topo, xyz, y, R, M32, world)
    e = (max(abs(x - lik) for x in liks) / abs(lik), float(np.abs(m - mean).max()), float(np.abs(v - var).max()))
    print("%d ranks against one plan: lik %.2e mean %.2e var %.2e" % (world, *e))
    assert max(liks) - min(liks) <= 1e-12 * abs(lik)                  # tests/_sharded_cases.py: SPREAD, SINGLE_LIK, SINGLE_MEAN, SINGLE_VAR
    assert e[0] <= 1e-12 and e[1] < 1e-11 and e[2] < 1e-12


# ---- 9. the facade -----------------------------------------------------------------------------------------------------------------------------
def test_facade(hip, sphere_tree):
    import pymra_amd
    ll, xyz, topo, y = tree(*TREES["g64"])
    t = sphere_tree
    assert t.d == 2 and t.cov_d == 3 and np.array_equal(t.cov_locs, xyz) and t.plan.d == 3 and t.topology.coord_dim == 3
    assert isinstance(t.kernel, mt.KernelSpec) and t.kernel.kind == mt.KIND_MATERN32 and t.kernel.l == 0.5       # a pyMRA-style lambda
    assert t.plan.route()["path"] == "Fused"
    np.random.seed(7)
    u = pymra_amd.MRATree(ll, 16, lambda a, b: mt.Matern32(a, b, l=0.5), y.reshape(-1, 1), R, M=2, J=4, cov_locs=xyz)
    assert u.getLikelihood()[0, 0] == t.getLikelihood()[0, 0]
    assert np.array_equal(np.asarray(u.predict()[0]), np.asarray(t.predict()[0])) and np.array_equal(u.predict()[1], t.predict()[1])
    check((float(t.getLikelihood()[0, 0]), np.asarray(t.predict()[0]).ravel(), t.predict()[1]), ref3(oracle(*TREES["g64"])), BARS, "MRATree(chordal)")
    sites = _off_tree_sites()
    a, b = t.predictAt(sites), u.predictAt(mt.lonlat_to_xyz(sites))  # (lon, lat) under chordal, covariance coordinates under cov_locs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.abs(np.asarray(t.root.B) - M32.evaluate(xyz, xyz[t.root.kInds])).max() < 1e-15
    widths = []

    def opaque(p, q):
        widths.append((np.shape(p)[1], np.shape(q)[1]))
        return np.asarray(M32.evaluate(p, q), dtype=np.float64) + 0.0

    np.random.seed(7)
    h = pymra_amd.MRATree(ll, 16, opaque, y.reshape(-1, 1), R, M=2, J=4, metric="chordal")
    assert h.kernel is None and set(widths) == {(3, 3)} and h.plan.route()["path"] == "Levels"
    check((float(h.getLikelihood()[0, 0]), np.asarray(h.predict()[0]).ravel(), h.predict()[1]),
          (float(t.getLikelihood()[0, 0]), np.asarray(t.predict()[0]).ravel(), t.predict()[1]), HOST_BARS, "opaque callable on xyz")
    lik2 = t.reevaluate(lambda a, b: mt.Matern32(a, b, l=0.4))[0, 0]
    assert lik2 != u.getLikelihood()[0, 0] and t.kernel.l == 0.4
    t.reevaluate(lambda a, b: mt.Matern32(a, b, l=0.5), want_predict=True)


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    import pymra_amd
    ll, xyz, topo, y = tree(*TREES["g64"])
    with pytest.raises(hip.MraError) as e:
        hip.HipPlan(dataclasses.replace(topo, coord_dim=4), 0)
    assert e.value.code == -1
    pl = make_plan(hip, topo, xyz, y, M32)
    first = predict_pass(pl)
    with pytest.raises(hip.MraError) as e:
        pl.set_kernel(M32.kind, M32.l, M32.sig, M32.scale, circular=True)
    assert e.value.code == -1
    leaves = np.nonzero(topo.node_leaf)[0].astype(np.int32)
    for call in (lambda: pl.predict_sites(ll[:3], leaves[:3]), lambda: pl.sites_cov(ll[:3], leaves[:3]),
                 lambda: pl.sample_sites(ll[:3], leaves[:3], 1, seed=1), lambda: pl.set_locs(ll)):
        with pytest.raises(ValueError):
            call()                                                    # (n, 2) sites / locations on a plan whose d is 3
    again = predict_pass(pl)
    assert again[0] == first[0] and np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
    pl.close()
    cov = lambda a, b: mt.Matern32(a, b, l=0.5)      # noqa: E731
    yy = y.reshape(-1, 1)
    for kw in (dict(cov_locs=xyz[:-1]), dict(cov_locs=np.column_stack((xyz, xyz[:, 0]))), dict(metric="chordal", cov_locs=xyz),
               dict(metric="geodesic"), dict(cov_locs=np.where(np.arange(len(xyz))[:, None] == 3, np.nan, xyz))):
        with pytest.raises(ValueError):
            pymra_amd.MRATree(ll, 16, cov, yy, R, M=2, J=4, **kw)
    with pytest.raises(ValueError):
        pymra_amd.MRATree(xyz, 16, cov, yy, R, M=2, J=4, metric="chordal")       # chordal wants (lon, lat)
    with pytest.raises(ValueError):
        pymra_amd.MRATree(ll, 16, lambda a, b: mt.Matern32(a, b, l=0.5, circular=True), yy, R, M=2, J=4, metric="chordal")


# ---- 11. 2-D untouched ------------------------------------------------------------------------------------------------------------------------
def test_a_2d_plan_is_the_same_before_and_after_a_3d_plan(hip):
    cs = K.load_case("g32")

    def g32():
        pl = make_plan(hip, cs["topo"], cs["locs"], cs["y_obs"], cs["spec"], noise=cs["c"]["R"])
        out = predict_pass(pl)
        assert pl.d == 2
        pl.close()
        return out

    before = g32()
    ll, xyz, topo, y = tree(*TREES["g64"])
    pl = make_plan(hip, topo, xyz, y, M32)
    predict_pass(pl)
    pl.set_option(hip.MRA_OPT_FUSED, 0)
    predict_pass(pl)
    pl.close()
    after = g32()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    assert abs(before[0] - float(cs["g"]["lik"])) <= 1e-9 * abs(float(cs["g"]["lik"]))
