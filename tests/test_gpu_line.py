"""1-D problems at real block widths: ternary trees on every route (GPU only; DESIGN.md section 7, "1-D at size").

The golden 1-D trees (c1, kat3, t201, t1000) have r0 = 2 and leaves within one 16-row tile.  The trees of tests/_line_cells.py have
full knot blocks of 16, 32 and 64 columns and leaves of 80 to 480 rows; every one is ``regular`` and takes PassPath::Fused or Hi.

 a. parity with the level-wise oracle on L16, L16s, L16d, L32, L64: likelihood + predict and likelihood-only, fused and level by
    level, the expected route asserted each time
 b. every covariance family on L16, the circular one included (and predictAt across the seam 0 / 1)
 c. trees the oracle is too slow for: device kernels against host-evaluated blocks on L64x (the row cascade staged level by level)
    and LH (PassPath::Hi); L32x fused against its own level-by-level pass
 d. the leaf-size edges 0 .. 192, 193, 208 on LE under the option cases of tests/_route_cells.py
 e. gappy likelihood-only passes with families of three siblings on L16s
 f. MRA_OPT_PARENT_PAIR 0 and 2 bit-identical on fronts with three children
 g. the retained-factor calls on L16 for one family per MODE of the 1-D kernel dispatch, each against its CPU twin
 h. three emulated ranks on L16s     i. the MRATree facade; a 2-D plan before and after the 1-D plans lived in the process

Bars, none new and none derived from a HIP result: tests/test_gpu_routes.py's ORACLE_BARS (likelihood 1e-10 relative, mean 1e-9
absolute, sd 1e-8 relative) and ROUTE_BARS, tests/test_gpu_hostcov.py's HOST_BARS, tests/test_gpu_likelihood_masks.py's, and for the
other calls the bars of their own 2-D GPU tests, cited where they are used.  tests/test_line_cells_cpu.py shows that the float64
oracle alone stays 100 times inside ORACLE_BARS on these problems."""
import functools

import numpy as np
import pytest

import _cases as K
import _line_cells as LC
import _route_cells as RC
import pymra_amd.MRATools as mt
import test_gpu_likelihood_masks as MK
import test_gpu_routes as TR

pytestmark = pytest.mark.gpu

R = LC.R
ORACLE_BARS, ROUTE_BARS = TR.ORACLE_BARS, TR.ROUTE_BARS
HOST_BARS = (1e-11, 1e-9, 1e-8)                 # tests/test_gpu_hostcov.py: stationary callable vs device kernel
M32 = LC.M32


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


@functools.lru_cache(maxsize=None)
def oracle(key, recipe=LC.DEFAULT, fam="m32"):
    from oracle.mra_levelwise import run_levelwise
    topo, locs, obs, y, counts = LC.problem(key, recipe)
    return run_levelwise(topo, locs, LC.FAMILIES[fam], y, R)


def make_plan(hip, topo, locs, y, spec=M32, opts=()):
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, R); pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale, spec.circular)
    for o, v in opts:
        pl.set_option(o, v)
    return pl


def check_route(pl, expect, tag):
    expect = dict(expect)
    least = expect.pop("n_chain_min", None)
    got = TR._check_route(pl, expect, tag)
    if least is not None:
        assert got["n_chain"] >= least, (tag, got["n_chain"])
    # the expectations hold while the leaf count stays clear of route_for's 2 n_cu threshold
    assert got["n_leaves"] <= got["n_cu"], "%s: %d leaves against %d compute units" % (tag, got["n_leaves"], got["n_cu"])
    return got


def preconditions(c, topo, counts):
    assert LC.ntl(counts) == c["ntl"], (c["tree"], c["mask"], int(counts.max()))
    assert int(LC.leaf_rows(topo).min()) == c["rows_min"], c["tree"]


def lik_only(pl, ref_lik, bar, tag):
    pl.run(True, False)
    lik = sum(pl.likelihood())
    e = abs(lik - ref_lik) / abs(ref_lik)
    print("%s, likelihood only: lik %.2e" % (tag, e))
    assert e <= bar, "%s: likelihood-only rel err %.3e" % (tag, e)
    return lik


def both_passes(pl, topo, counts, ref, bars, tag):
    """likelihood + predict, then likelihood only, against ref = (lik, mean, sd); -> (result, predictive route, likelihood-only route)"""
    got = TR._predict(pl)
    route = pl.route()
    TR._against(topo, counts, got, ref, bars, tag)
    lik_only(pl, ref[0], bars[0], tag)
    return got, route, pl.route()


# ---- a. parity with the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "levels"])
@pytest.mark.parametrize("key", ["L16", "L16s", "L16d", "L32", "L64"])
def test_parity_with_the_oracle(hip, key, fused):
    topo, locs, obs, y, counts = LC.problem(key)
    ref = oracle(key)
    opts = () if fused else LC.LEVELS_OFF
    pl = make_plan(hip, topo, locs, y, opts=opts)
    assert pl.d == 1 and topo.d == 1
    tag = "%s %s" % (key, "fused" if fused else "level by level")
    c = LC.find(key, True, opts)
    preconditions(c, topo, counts)
    got = TR._predict(pl)
    check_route(pl, c["expect"], tag)
    TR._against(topo, counts, got, TR._ref3(ref), ORACLE_BARS, tag + " vs oracle")
    rep = LC.reported(topo)
    assert int((~rep).sum()) == LC.SHAPES[key][4]
    if not rep.all():
        pl.run(True, True)
        mean, var = pl.predict()
        assert np.all(mean[~rep] == 0.0) and np.all(var[~rep] == 0.0) and np.all(got[2][~rep] == 0.0)      # the dropped location
        assert np.all(ref["mean"][~rep] == 0.0) and np.all(ref["sd"][~rep] == 0.0)
    lik_only(pl, ref["lik"], ORACLE_BARS[0], tag)
    check_route(pl, LC.find(key, False, opts)["expect"], tag + " likelihood only")
    again = TR._predict(pl)
    assert again[0] == got[0] and np.array_equal(again[1], got[1]) and np.array_equal(again[2], got[2]), tag + ": second predictive pass differs"
    pl.close()


# ---- b. every covariance family -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", list(LC.FAMILIES))
def test_every_covariance_family(hip, fam):
    topo, locs, obs, y, counts = LC.problem("L16")
    ref = TR._ref3(oracle("L16", fam=fam))
    pl = make_plan(hip, topo, locs, y, LC.FAMILIES[fam])
    _, route, route_lik = both_passes(pl, topo, counts, ref, ORACLE_BARS, "L16 %s fused" % fam)
    assert route["path"] == "Fused" and route_lik["lik_rows"]
    pl.set_option(hip.MRA_OPT_FUSED, 0)
    _, route, route_lik = both_passes(pl, topo, counts, ref, ORACLE_BARS, "L16 %s level by level" % fam)
    assert route["path"] == "Levels" and route_lik["lik_general"]
    pl.close()


def line_tree(fam, spec=None):
    """MRATree on L16 with the family's pyMRA-style covariance function; its topology is LC.tree("L16")'s"""
    import pymra_amd
    s = spec or LC.FAMILIES[fam]
    cov = {"exp": lambda a, b: mt.ExpCovFun(a, b, l=s.l), "m32": lambda a, b: mt.Matern32(a, b, l=s.l),
           "m52": lambda a, b: mt.Matern52(a, b, l=s.l), "gauss": lambda a, b: mt.GaussianCovFun(a, b, l=s.l),
           "kanter": lambda a, b: mt.KanterCovFun(a, b, radius=s.l), "iden": lambda a, b: mt.Iden(a, b, l=s.l),
           "exp_circular": lambda a, b: mt.ExpCovFun(a, b, l=s.l, circular=True)}[fam]
    topo, locs, obs, y, counts = LC.problem("L16")
    np.random.seed(7)
    t = pymra_amd.MRATree(locs, 16, cov, y.reshape(-1, 1), R, M=2, J=3)
    for f in ("perm", "src", "knot_rows", "node_row0"):
        assert np.array_equal(getattr(t.topology, f), getattr(topo, f)), f
    k = t.kernel
    assert (k.kind, k.l, k.sig, k.scale, k.circular) == (s.kind, s.l, s.sig, s.scale, s.circular)
    return t


def test_the_seam_of_a_circular_kernel(hip):
    """Sites 0.001 either side of the seam 0 / 1 lie in the first and in the last leaf: predictAt against the CPU restatement, and
    against the same tree without the wrap, which it must differ from."""
    import _treesites as TS
    topo, locs, obs, y, counts = LC.problem("L16")
    spec = LC.FAMILIES["exp_circular"]
    t = line_tree("exp_circular")
    sites = np.array([[0.001], [0.999], [0.0004], [0.9997], [0.5003]])
    leaf = t.locate(sites)
    lv = LC.leaves(topo)
    assert leaf[0] == lv[0] and leaf[1] == lv[-1] and leaf[2] in (lv[0], lv[-1]) and leaf[3] == lv[-1]
    m, sd = t.predictAt(sites, leaf=leaf)
    want_m, want_v = TS.tree_sites(topo, locs, spec, y, R, sites, leaf)
    e_m, e_v = float(np.abs(m - want_m).max()), float(np.abs(sd ** 2 - want_v).max())
    print("circular predictAt at the seam: mean %.2e var %.2e" % (e_m, e_v))
    assert e_m <= 1e-8 * max(1.0, np.abs(want_m).max()) and e_v <= 1e-9          # tests/test_gpu_sites.py
    flat_m, flat_v = TS.tree_sites(topo, locs, LC.FAMILIES["exp"], y, R, sites, leaf)
    assert abs(flat_m[0, 0] - want_m[0, 0]) > 1e-6 or abs(flat_v[0] - want_v[0]) > 1e-6         # the first leaf is unobserved: the wrap reaches it


# ---- c. trees too slow for the oracle -----------------------------------------------------------------------------------------------
def _row_cascade_launches(pl):
    return sum(k["launches"] for k in pl.kernel_stats() if MK.PRIOR_ROWS in k["name"])


def _host_against_device(hip, key, expect_path):
    from pymra_amd.MRATree import probe_cov
    topo, locs, obs, y, counts = LC.problem(key)
    opaque = lambda a, b: np.asarray(M32.evaluate(a, b), dtype=np.float64) + 0.0      # noqa: E731
    assert probe_cov(opaque, 1, locs) is None
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, R); pl.upload_host_cov(opaque, locs, y)
    host = TR._predict(pl)
    assert pl.route()["path"] == "Levels"
    pl.set_kernel(M32.kind, M32.l, M32.sig, M32.scale)
    pl.set_option(hip.MRA_OPT_KERNEL_TIMING, 1)
    tag = "%s: device vs host blocks" % key
    preconditions(LC.find(key, True), topo, counts)
    got = TR._predict(pl)
    check_route(pl, LC.find(key, True)["expect"], tag)
    cascade = _row_cascade_launches(pl)
    TR._against(topo, counts, got, host, HOST_BARS, tag)
    lik_only(pl, host[0], HOST_BARS[0], tag)
    check_route(pl, LC.find(key, False)["expect"], tag + " likelihood only")
    pl.set_option(hip.MRA_OPT_KERNEL_TIMING, 0)
    # the knot pass level by level (k_prior_cascade in knot mode), then every level by its own kernels
    pl.set_option(hip.MRA_OPT_KNOT_CHAIN, 0)
    _, route, _ = both_passes(pl, topo, counts, host, HOST_BARS, "%s: device, knot chain off, vs host blocks" % key)
    assert route["n_chain"] == 0 and route["path"] == expect_path
    pl.set_option(hip.MRA_OPT_KNOT_CHAIN, 1)
    pl.set_option(hip.MRA_OPT_FUSED, 0)
    _, route, route_lik = both_passes(pl, topo, counts, host, HOST_BARS, "%s: device (level by level) vs host blocks" % key)
    assert route["path"] == "Levels" and route["prior_level"] and route_lik["lik_general"]
    pl.close()
    return cascade


def test_staged_row_cascade_four_tiles_wide(hip):
    """k_prior_cascade<4, 4, 1, *, false>: CWT 4 on four levels, 136 operand tiles against the 80 of the LDS"""
    topo, _ = LC.tree("L64x")
    assert int(topo.cw[0]) == 64 and topo.n_levels == 5
    assert _host_against_device(hip, "L64x", "Fused") > 0


def test_deep_wide_tree(hip):
    """PassPath::Hi with the update in k_predict_hi"""
    topo, _ = LC.tree("LH")
    assert int(topo.cw[0]) == 64 and topo.n_levels == 6
    _host_against_device(hip, "LH", "Hi")


def test_staged_row_cascade_two_tiles_wide_seven_levels(hip):
    """k_prior_cascade<2, 8, 1, *, false>: CWT 2 on seven levels, 105 operand tiles.  Too large for the oracle and for host blocks in a
    test: the fused pass against the level-by-level pass of the same plan, at the bars of
    tests/test_gpu_parity.py::test_fused_cascades_at_every_depth"""
    topo, locs, obs, y, counts = LC.problem("L32x")
    assert [int(v) for v in np.diff(topo.level_ptr)] == LC.SHAPES["L32x"][0] and int(topo.cw[0]) == 32
    pl = make_plan(hip, topo, locs, y, opts=((hip.MRA_OPT_KERNEL_TIMING, 1),))
    fused = TR._predict(pl)
    assert pl.route()["path"] == "Fused" and _row_cascade_launches(pl) > 0
    pl.set_option(hip.MRA_OPT_FUSED, 0)
    lev = TR._predict(pl)
    assert pl.route()["path"] == "Levels"
    TR._against(topo, counts, fused, lev, (1e-11, 1e-9, 1e-8), "L32x: fused (staged row cascade) vs level by level")
    pl.close()


# ---- d. leaf-size edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe,cls,top", LC.EDGE_MASKS, ids=["-".join(str(x) for x in m[1:]) for m, _, _ in LC.EDGE_MASKS])
def test_leaf_size_edges(hip, recipe, cls, top):
    topo, locs, obs, y, counts = LC.problem("LE", recipe)
    ref = oracle("LE", recipe)
    assert set(c for c in RC.EDGE_COUNTS if c <= 191) | {top} <= set(counts.tolist()) and counts.max() == top
    assert (counts[0], counts[-1]) == ((0, top) if recipe[1] == "empty_first" else (top, 0))
    assert int(LC.leaf_rows(topo).min()) >= 128
    base, cases = RC.EDGE_CLASSES[cls]
    pl = make_plan(hip, topo, locs, y)
    tag = "LE %s" % (recipe,)
    default = TR._run_cell(pl, topo, counts, ref, True, (), base, tag + " default")
    rt = pl.route()
    n_small = int((RC.tiles(counts) <= 8).sum())
    assert rt["n_trsm_small"] == n_small == rt["n_chol_small"] and rt["n_leaves"] == len(counts) <= rt["n_cu"]
    assert 0 < n_small < len(counts)
    for opts, effect, diff in cases:
        expect = dict(base, **diff)
        if not effect:
            assert expect == base
        TR._run_cell(pl, topo, counts, ref, True, opts, expect, "%s %s (%s)" % (tag, opts, "took effect" if effect else "overridden"), default)
    TR._run_cell(pl, topo, counts, ref, False, (), {"update": "None", "var": "None", "c_only": cls != "big", "lik_rows": cls != "big"}, tag + " likelihood only")
    TR._levels_on_the_same_plan(pl, topo, counts, ref, default, tag)
    pl.close()


def test_the_default_mask_on_the_edge_tree(hip):
    """81 leaves under the plain 40 % mask: 9 and 10 tiles beside at most 8, one k_chol_tiles<10> launch"""
    topo, locs, obs, y, counts = LC.problem("LE")
    c = LC.find("LE", True)
    preconditions(c, topo, counts)
    pl = make_plan(hip, topo, locs, y)
    got = TR._predict(pl)
    check_route(pl, c["expect"], "LE default mask")
    TR._set(pl, LC.LEVELS_OFF)
    lev = TR._predict(pl)
    TR._against(topo, counts, got, lev, (1e-11, 1e-9, 1e-8), "LE default mask: fused vs level by level")      # TR._levels_on_the_same_plan's
    pl.close()


# ---- e. gappy likelihood-only passes, families of three -------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", LC.GAPPY)
def test_gappy_masks_with_families_of_three(hip, pattern):
    from oracle.mra_levelwise import run_levelwise
    topo, locs, obs, y, counts = LC.problem("L16s", ("pattern", pattern))
    assert [len(f) for f in MK._families(topo)] == [3] * 9
    assert counts.max() <= 192 and counts.sum() > 0
    if pattern in MK.STALE:
        assert MK.cross_family_joins(topo, obs) > 0
    ref = run_levelwise(topo, locs, M32, y, R, predict=False)["lik"]
    lik = MK.check_fused(hip, topo, locs, y, "L16s " + pattern, ref=ref, make_plan=make_plan)
    print("L16s %s: lik %.2e" % (pattern, MK._relerr(lik, ref)))


# ---- f. parent fronts with three children ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["L16", "L32"])
def test_parent_pair_with_three_children(hip, key):
    topo, locs, obs, y, counts = LC.problem(key)
    pl = make_plan(hip, topo, locs, y, opts=((hip.MRA_OPT_KERNEL_TIMING, 1),))
    res = {}
    for v in (0, 2, 0):
        pl.set_option(hip.MRA_OPT_PARENT_PAIR, v)
        got = TR._predict(pl)
        assert pl.route()["path"] == "Fused" and pl.route()["parent_front"]
        fam = [k for k in pl.kernel_stats() if k["name"].startswith("k_parent_front")]
        assert len(fam) == 1 and fam[0]["launches"] == 1
        pl.run(True, False)
        out = (got, sum(pl.likelihood()), fam[0]["flops"], fam[0]["flops_exec"])
        if v in res:
            assert out[1] == res[v][1] and out[3] == res[v][3] and np.array_equal(out[0][1], res[v][0][1])
        res[v] = out
    a, b = res[0], res[2]
    assert b[3] > a[3] and b[2] == a[2], "the pair kernel did not run: executed flops %r against %r" % (b[3], a[3])
    assert a[0][0] == b[0][0] and a[1] == b[1] and np.array_equal(a[0][1], b[0][1]) and np.array_equal(a[0][2], b[0][2]), key
    e = TR._ref3(oracle(key))
    TR._against(topo, counts, b[0], e, ORACLE_BARS, "%s pair kernel vs oracle" % key)
    pl.close()


# ---- g. the retained-factor calls -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=LC.MODE_FAMILIES)
def fitted(request, hip):
    import _treesites as TS
    fam = request.param
    topo, locs, obs, y, counts = LC.problem("L16")
    spec = LC.FAMILIES[fam]
    return dict(fam=fam, spec=spec, t=line_tree(fam), state=TS.SiteState(topo, locs, spec, y, R))


def _sites():
    """24 sites off the grid; the first five: one in the leaf without observations, one either side of the boundary between the
    third and the fourth leaf, one below the first and one above the last location"""
    topo, locs, obs, y, counts = LC.problem("L16")
    x = np.sort(locs.ravel())
    lv = LC.leaves(topo)
    hi3 = locs[MK._leaf_callers(topo, lv[2])].max()
    lo4 = locs[MK._leaf_callers(topo, lv[3])].min()
    assert hi3 < lo4
    h = float(x[1] - x[0])
    s = np.random.default_rng(9).uniform(x[0], x[-1], 24)
    s[:5] = (float(locs[MK._leaf_callers(topo, lv[0])].mean()) + 0.3 * h, hi3 + 0.2 * h, lo4 - 0.2 * h, x[0] - 0.4 * h, x[-1] + 0.4 * h)
    return s.reshape(-1, 1)


def test_site_leaves(hip, fitted):
    topo, locs, obs, y, counts = LC.problem("L16")
    lv = LC.leaves(topo)
    leaf = fitted["t"].locate(_sites())
    assert counts[0] == 0 and leaf[0] == lv[0] and leaf[1] == lv[2] and leaf[2] == lv[3] and leaf[3] == lv[0] and leaf[4] == lv[-1]


def test_solve_17_columns(hip, fitted):
    import _treesolve as TSV
    topo, locs, obs, y, counts = LC.problem("L16")
    Y = np.random.default_rng(1).standard_normal((len(y), 17))
    Y[:, 0] = np.nan_to_num(y)
    mean, quad = fitted["t"].solve(Y)
    want_mean, want_quad = TSV.tree_solve(topo, locs, fitted["spec"], y, R, Y)
    e_m = float(np.abs(mean - want_mean).max())
    blk = np.arange(17)[:, None] // 16 == np.arange(17)[None, :] // 16
    e_q = float(np.abs(quad - want_quad)[blk].max())
    print("%s solve: mean %.2e quad %.2e (scale %.1f)" % (fitted["fam"], e_m, e_q, np.abs(np.diag(want_quad)).max()))
    assert np.all(np.isnan(quad[~blk]))
    assert e_m <= 1e-9 * max(1.0, np.abs(want_mean).max())          # tests/test_gpu_solve.py
    assert e_q <= 1e-9 * np.abs(np.diag(want_quad)).max()


@pytest.mark.parametrize("distr", ["prior", "posterior"])
def test_covariance_columns(hip, fitted, distr):
    import _treecov as TCV
    topo, locs, obs, y, counts = LC.problem("L16")
    spec = fitted["spec"]
    lv = LC.leaves(topo)
    rows = np.array([0, len(y) - 1, 1234, int(MK._leaf_callers(topo, lv[2]).max()), int(MK._leaf_callers(topo, lv[3]).min()), 100])
    A = np.zeros((len(y), len(rows)))
    A[rows, np.arange(len(rows))] = 1.0
    want, _ = TCV.tree_cov(topo, locs, spec, y, R, A, posterior=(distr == "posterior"))
    got = fitted["t"].covariance(rows, distr)
    err = float(np.abs(got - want).max())
    print("%s covariance(%s): %.2e" % (fitted["fam"], distr, err))
    assert err <= 1e-9 * spec.sig * spec.scale                        # tests/test_gpu_cov.py: tol * the largest prior variance


def test_predictAt(hip, fitted):
    import _treesites as TS
    topo, locs, obs, y, counts = LC.problem("L16")
    t, spec = fitted["t"], fitted["spec"]
    xP, sdP = t.predict()
    own = np.arange(0, len(locs), 7)
    m, sd = t.predictAt(locs[own])
    assert np.abs(m[:, 0] - np.asarray(xP).ravel()[own]).max() <= 1e-8 * max(1.0, np.abs(xP).max())        # tests/test_gpu_sites.py
    assert np.abs(sd ** 2 - sdP[own] ** 2).max() <= 1e-9
    sites = _sites()
    leaf = t.locate(sites)
    m, sd = t.predictAt(sites, leaf=leaf)
    want_m, want_v = TS.tree_sites(topo, locs, spec, y, R, sites, leaf, state=fitted["state"])
    e_m, e_v = float(np.abs(m - want_m).max()), float(np.abs(sd ** 2 - want_v).max())
    print("%s predictAt, %d sites: mean %.2e var %.2e" % (fitted["fam"], len(sites), e_m, e_v))
    assert e_m <= 1e-8 * max(1.0, np.abs(want_m).max()) and e_v <= 1e-9


def test_covarianceAt_and_sampleAt(hip, fitted):
    import _treesitecov as TC
    import _treesitedraw as TD
    t = fitted["t"]
    sites = _sites()
    leaf = t.locate(sites)
    slots = t.plan.sample_sites_slots(len(sites))
    z = np.random.default_rng(3).standard_normal((slots, 3))
    for distr in ("prior", "posterior"):
        S = t.covarianceAt(sites, distr, leaf=leaf)
        assert np.array_equal(S, S.T)
        want = TC.tree_sites_cov(fitted["state"], sites, leaf, distr == "posterior")
        err = float(np.abs(S - want).max())
        print("%s covarianceAt(%s): %.2e" % (fitted["fam"], distr, err))
        assert err <= 1e-9                                            # tests/test_gpu_sitecov.py: _post_tol * scale, scale 1
        F, _ = TD.site_draw_factor(fitted["state"], sites, leaf, distr == "posterior")
        assert F.shape == (len(sites), slots)
        mean = t.predictAt(sites, leaf=leaf)[0] if distr == "posterior" else 0.0
        x = t.sampleAt(sites, 3, distr, leaf=leaf, z=z)
        e = np.abs(x - (mean + F @ z))
        # tests/test_gpu_sitedraw.py holds every entry of F to 1e-9 of the prior variance (1 here): F z within 1e-9 sum_k |z_k|
        assert np.all(e <= 1e-9 * np.abs(z).sum(axis=0)[None, :]), e.max()
        print("%s sampleAt(%s): %.2e" % (fitted["fam"], distr, e.max()))
    sd = t.predictAt(sites, leaf=leaf)[1]
    assert np.abs(np.diag(t.covarianceAt(sites, "posterior", leaf=leaf)) - sd ** 2).max() <= 1e-9


def test_sample_factor_is_the_prior_covariance(hip, fitted):
    """plan.sample with unit draws on the slots one leaf reads: G G^T is the MRA prior covariance of the leaf's rows, and a zero draw
    of the posterior is the predictive mean"""
    import _sampling as SM
    import _treecov as TCV
    topo, locs, obs, y, counts = LC.problem("L16")
    t, spec = fitted["t"], fitted["spec"]
    if fitted["fam"] == "gauss":
        # a draw factors the leaves' prior covariance without any noise on it: at l = 0.01 that matrix is singular in float64
        # (tests/test_line_cells_cpu.py; the library answers MRA_ERR_NOT_SPD), so the sampler gets the Gaussian range at which
        # LAPACK can factor it too
        spec = LC.GAUSS_SAMPLE
        t = line_tree("gauss", spec)
    j = LC.leaves(topo)[5]
    prow = np.arange(int(topo.node_row0[j]), int(topo.node_row1[j]))
    prow = prow[SM.reported(topo)[prow]][::9]
    G, _ = SM.factor_columns(t.plan, SM.chain_slots(topo, j), rows=prow)
    A = np.zeros((len(y), len(prow)))
    A[topo.perm[prow], np.arange(len(prow))] = 1.0
    want = TCV.tree_cov(topo, locs, spec, y, R, A)[0][topo.perm[prow]]
    err = float(np.abs(G @ G.T - want).max())
    print("%s sample: G G^T against the prior covariance of %d rows of a leaf: %.2e" % (fitted["fam"], len(prow), err))
    assert err <= 1e-9                                                # tests/test_gpu_sample.py: tol * scale
    x0 = t.plan.sample(1, z=np.zeros((1, t.plan.sample_slots())), conditional=True)[0]
    rep = SM.reported(topo)
    assert np.abs(x0[rep] - np.asarray(t.predict()[0]).ravel()[topo.perm[rep]]).max() <= 1e-8


# ---- h. sharded -----------------------------------------------------------------------------------------------------------------------
def test_three_ranks_against_one_plan(hip):
    topo, locs, obs, y, counts = LC.problem("L16s")
    pl = make_plan(hip, topo, locs, y)
    pl.run(True, True)
    lik = sum(pl.likelihood())
    mean, var = pl.predict()
    pl.close()
    ranks = K.emulate_world_on_one_gpu(hip, topo, locs, y, R, M32, 3, per_rank=True)
    liks = [r["lik"] for r in ranks]
    m, v = sum(r["mean"] for r in ranks), sum(r["var"] for r in ranks)
    e = (max(abs(x - lik) for x in liks) / abs(lik), float(np.abs(m - mean).max()), float(np.abs(v - var).max()))
    print("L16s, 3 ranks against one plan: lik %.2e mean %.2e var %.2e" % e)
    assert max(liks) - min(liks) <= 1e-12 * abs(lik)                  # tests/_sharded_cases.py: SPREAD, SINGLE_LIK, SINGLE_MEAN, SINGLE_VAR
    assert e[0] <= 1e-12 and e[1] < 1e-11 and e[2] < 1e-12
    c = LC.SHARDED[0]
    for rk, r in enumerate(ranks):
        assert len(LC.leaves(r["topo"])) == 9
        diff = {k: (r["route"][k], w) for k, w in c["expect"][rk].items() if r["route"][k] != w}
        assert not diff, "rank %d: route (got, expected) %s" % (rk, diff)


def test_a_rank_without_observations(hip):
    c = LC.SHARDED[1]
    topo, locs, obs, y, counts = LC.problem(c["tree"], c["mask"])
    assert counts[:9].sum() == 0 and counts[9:].min() > 0
    ref = oracle(c["tree"], c["mask"])["lik"]
    ranks = K.emulate_world_on_one_gpu(hip, topo, locs, y, R, M32, c["world"], predict=False, per_rank=True)
    for rk, r in enumerate(ranks):
        diff = {k: (r["route"][k], w) for k, w in c["expect"][rk].items() if r["route"][k] != w}
        assert not diff, "rank %d: route (got, expected) %s" % (rk, diff)
        e = abs(r["lik"] - ref) / abs(ref)
        print("L16s, first subtree unobserved, rank %d: lik %.2e" % (rk, e))
        assert e <= ORACLE_BARS[0]


# ---- i. the facade ----------------------------------------------------------------------------------------------------------------------
def test_facade_and_a_2d_plan_before_and_after(hip):
    cs = K.load_case("g32")

    def g32():
        s = cs["spec"]
        pl = hip.HipPlan(cs["topo"], 0)
        pl.set_locs(cs["locs"]); pl.set_obs(cs["y_obs"], cs["c"]["R"]); pl.set_kernel(s.kind, s.l, s.sig, s.scale)
        out = TR._predict(pl)
        assert pl.d == 2
        pl.close()
        return out

    before = g32()
    topo, locs, obs, y, counts = LC.problem("L16")
    t = line_tree("m32")
    assert t.d == 1 and t.cov_d == 1 and t.plan.d == 1 and t.J == 3 and t.M == 2
    assert t.plan.route()["path"] == "Fused"
    pl = make_plan(hip, topo, locs, y)
    got = TR._predict(pl)
    assert float(t.getLikelihood()[0, 0]) == got[0]
    assert np.array_equal(np.asarray(t.predict()[0]).ravel(), got[1]) and np.array_equal(t.predict()[1], got[2])
    pl.set_option(hip.MRA_OPT_FUSED, 0)
    TR._predict(pl)
    pl.close()
    TR._against(topo, counts, (float(t.getLikelihood()[0, 0]), np.asarray(t.predict()[0]).ravel(), t.predict()[1]), TR._ref3(oracle("L16")),
                ORACLE_BARS, "MRATree on L16 vs oracle")
    after = g32()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    assert abs(before[0] - float(cs["g"]["lik"])) <= 1e-9 * abs(float(cs["g"]["lik"]))
