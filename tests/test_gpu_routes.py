"""Which kernels a pass launched, and what they computed (GPU only).

``HipPlan.route()`` reads the route the library fixed for the last pass.  Every cell of tests/_route_cells.py asserts it - an
accepted option is not yet a kernel that ran - and compares likelihood, predictive mean and sd with the level-wise float64 oracle,
with the level-by-level kernels on the same plan, and bit for bit with a second predictive pass after a likelihood-only one.  The
leaf-size edge masks put leaves of 0 .. 192 (193, 208) observations into one tree, small and large leaves interleaved, so that the
sorted leaf lists of the fused path (leaves of at most 8 tiles first) are exercised in the middle; errors are reported per leaf with
its observation count.  Trees with non-leaf blocks wider than 192 columns (r0 = 200, 208) take k_trsm_rows and k_leaf_moments.

Bars (the project's standing ones, none derived from a HIP result): against run_levelwise lik 1e-10 rel, mean 1e-9 abs, sd 1e-8
rel; another route on the same plan against the default route lik 1e-12, mean 1e-10, sd 1e-9; against the 80-bit run_extended mean
and sd 1e-9."""
import functools

import numpy as np
import pytest

import _cases as K
import _route_cells as RC
import test_gpu_likelihood_masks as MK

pytestmark = pytest.mark.gpu

R = MK.R


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


@functools.lru_cache(maxsize=None)
def _tree(key):
    return MK._tree(*RC.TREES[key])


@functools.lru_cache(maxsize=None)
def _case(key, recipe):
    """(topo, locs, obs mask, y, leaf counts, oracle) of one (tree, mask): the oracle runs once for all option tuples."""
    from oracle.mra_levelwise import run_levelwise
    topo, locs = _tree(key)
    obs = RC.make_obs(topo, locs, recipe)
    y = MK._y(obs)
    return topo, locs, obs, y, MK.leaf_counts(topo, obs), run_levelwise(topo, locs, MK._spec(), y, R)


def _set(pl, opts):
    values = dict(RC.DEFAULTS)
    values.update(dict(opts))
    for o, v in values.items():
        pl.set_option(o, v)


def _check_route(pl, expect, tag):
    got = pl.route()
    diff = {k: (got[k], v) for k, v in expect.items() if got[k] != v}
    assert not diff, "%s: route (got, expected) %s" % (tag, diff)
    return got


def _predict(pl):
    pl.run(True, True)
    mean, _, sd = pl.predict(with_sd=True)
    return sum(pl.likelihood()), mean.copy(), sd.copy()


def _per_leaf(topo, counts, a, b, relative):
    """(worst error, 'leaf t (n observations): error' of the worst leaves) of a against b, leaf by leaf."""
    rows = []
    for t, i in enumerate(np.nonzero(topo.node_leaf)[0]):
        p = MK._leaf_callers(topo, i)
        e = np.abs(a[p] - b[p])
        if relative:
            e = e / np.maximum(np.abs(b[p]), 1e-300)
        rows.append((float(e.max()) if len(p) else 0.0, t, int(counts[t])))
    rows.sort(reverse=True)
    return rows[0][0], ", ".join("leaf %d (%d observations): %.3e" % (t, c, e) for e, t, c in rows[:4])


def _against(topo, counts, got, ref, bars, tag):
    lik, mean, sd = got
    e_l = abs(lik - ref[0]) / abs(ref[0])
    e_m, where_m = _per_leaf(topo, counts, mean, ref[1], False)
    e_s, where_s = _per_leaf(topo, counts, sd, ref[2], True)
    print("%s: lik %.2e mean %.2e sd %.2e" % (tag, e_l, e_m, e_s))
    assert e_l <= bars[0], "%s: likelihood rel err %.3e" % (tag, e_l)
    assert e_m <= bars[1], "%s: mean abs err by leaf: %s" % (tag, where_m)
    assert e_s <= bars[2], "%s: sd rel err by leaf: %s" % (tag, where_s)


ORACLE_BARS = (1e-10, 1e-9, 1e-8)
ROUTE_BARS = (1e-12, 1e-10, 1e-9)


def _ref3(ref):
    return ref["lik"], ref["mean"], ref["sd"]


def _run_cell(pl, topo, counts, ref, predict, opts, expect, tag, default=None):
    """One cell on an open plan: route, oracle, then a likelihood-only pass and a second predictive pass (bit-identical)."""
    _set(pl, opts)
    if not predict:
        pl.run(True, False)
        _check_route(pl, expect, tag)
        lik = sum(pl.likelihood())
        assert abs(lik - ref["lik"]) <= ORACLE_BARS[0] * abs(ref["lik"]), "%s: likelihood rel err %.3e" % (tag, abs(lik - ref["lik"]) / abs(ref["lik"]))
        pl.run(True, True)
        pl.run(True, False)
        assert sum(pl.likelihood()) == lik, tag
        return None
    got = _predict(pl)
    _check_route(pl, expect, tag)
    _against(topo, counts, got, _ref3(ref), ORACLE_BARS, tag + " vs oracle")
    if default is not None:
        _against(topo, counts, got, default, ROUTE_BARS, tag + " vs default route")
    pl.run(True, False)
    assert abs(sum(pl.likelihood()) - got[0]) <= 1e-12 * abs(got[0]), tag
    again = _predict(pl)
    assert again[0] == got[0] and np.array_equal(again[1], got[1]) and np.array_equal(again[2], got[2]), tag + ": second predictive pass differs"
    return got


def _levels_on_the_same_plan(pl, topo, counts, ref, got, tag):
    """MRA_OPT_FUSED off on the same plan: the level-by-level kernels against the oracle and against the fused result."""
    _set(pl, ((2, 0),))
    lev = _predict(pl)
    assert pl.route()["path"] == "Levels", tag
    _against(topo, counts, lev, _ref3(ref), ORACLE_BARS, tag + " level-by-level vs oracle")
    if got is not None:
        _against(topo, counts, lev, got, (1e-11, 1e-9, 1e-8), tag + " level-by-level vs this route")


# ---- B. the route table ---------------------------------------------------------------------------------------------------------
GROUPS = sorted(set((c["tree"], c["mask"]) for c in RC.CELLS))


@pytest.mark.parametrize("key,recipe", GROUPS, ids=["%s-%s" % (k, "-".join(str(x) for x in m)) for k, m in GROUPS])
def test_route_table(hip, key, recipe):
    topo, locs, obs, y, counts, ref = _case(key, recipe)
    pl = MK._plan(hip, topo, locs, y)
    with pytest.raises(hip.MraError) as ei:
        pl.route()
    assert ei.value.code == -4                                   # MRA_ERR_STATE before the first pass
    for c in RC.CELLS:
        if (c["tree"], c["mask"]) != (key, recipe):
            continue
        tag = "%s %s predict=%s %s" % (key, recipe, c["predict"], c["opts"])
        assert int(RC.tiles(counts).max()) == c["ntl"], (tag, int(counts.max()))
        got = _run_cell(pl, topo, counts, ref, c["predict"], c["opts"], c["expect"], tag)
        rt = pl.route()
        assert rt["n_leaves"] == len(counts) and rt["n_trsm_small"] == int((RC.tiles(counts) <= 8).sum()) == rt["n_chol_small"], tag
        # the table's leaf counts stay a factor of two away from the 2 n_cu threshold on either side
        assert rt["n_leaves"] <= rt["n_cu"] or rt["n_leaves"] >= 4 * rt["n_cu"], "leaf count too close to 2 n_cu for the table: %s" % rt
        if c["predict"] and dict(c["opts"]).get(2, 1) == 1:
            _levels_on_the_same_plan(pl, topo, counts, ref, got, tag)
    pl.close()


@pytest.mark.parametrize("c", RC.SHARDED, ids=["-".join(str(x) for x in c["mask"]) for c in RC.SHARDED])
def test_route_table_sharded(hip, c):
    """Four ranks emulated one after the other (as tests/_cases.py does), each rank's route asserted; the predict-only leaf work of a
    sharded rank goes to the side stream, a rank without any observation has no C block to fix."""
    from pymra_amd.sharding import shard_topology
    topo, locs, obs, y, counts, ref = _case(c["tree"], c["mask"])
    s = MK._spec()
    plans, bufs = [], []
    for rk in range(c["world"]):
        lt, red = shard_topology(topo, c["world"], rk)
        p = hip.HipPlan(lt, 0)
        p.set_locs(locs); p.set_obs(y, R); p.set_kernel(s.kind, s.l, s.sig, s.scale)
        p.set_reduce_level(red)
        _set(p, c["opts"])
        p.run(True, c["predict"], split=True)
        bufs.append(p.reduce_export())
        plans.append(p)
    tot = np.sum(bufs, axis=0)
    mean, sd = np.zeros(topo.N), np.zeros(topo.N)
    for rk, p in enumerate(plans):
        p.reduce_import(tot)
        p.resume()
        _check_route(p, c["expect"][rk], "%s rank %d" % (c["mask"], rk))
        lik = sum(p.likelihood())
        assert abs(lik - ref["lik"]) <= ORACLE_BARS[0] * abs(ref["lik"]), (rk, lik, ref["lik"])
        if c["predict"]:
            m, _, d = p.predict(with_sd=True)
            mean += m; sd += d
        p.close()
    if c["predict"]:
        _against(topo, counts, (ref["lik"], mean, sd), _ref3(ref), ORACLE_BARS, "sharded %s" % (c["mask"],))


# ---- C. leaf-size edges and mixed trees -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,recipe,cls,top", RC.EDGE_MASKS, ids=["%s-%s" % (k, "-".join(str(x) for x in m[1:])) for k, m, _, _ in RC.EDGE_MASKS])
def test_leaf_size_edges(hip, key, recipe, cls, top):
    topo, locs, obs, y, counts, ref = _case(key, recipe)
    cap = RC.leaf_capacity(topo)
    assert set(c for c in RC.EDGE_COUNTS if c <= min(cap, 191)) | {top} <= set(counts.tolist()) and counts.max() == top
    assert (counts[0], counts[-1]) == ((0, top) if recipe[1] == "empty_first" else (top, 0))
    base, cases = RC.EDGE_CLASSES[cls]
    pl = MK._plan(hip, topo, locs, y)
    tag = "%s %s" % (key, recipe)
    default = _run_cell(pl, topo, counts, ref, True, (), base, tag + " default")
    rt = pl.route()
    n_small = int((RC.tiles(counts) <= 8).sum())
    assert rt["n_trsm_small"] == n_small == rt["n_chol_small"] and rt["n_leaves"] == len(counts)
    if cls != "small":
        assert 0 < rt["n_trsm_small"] < rt["n_leaves"], rt
    for opts, effect, diff in cases:
        expect = dict(base, **diff)
        if not effect:
            assert expect == base                                 # overridden: the route stays the mask's default route
        _run_cell(pl, topo, counts, ref, True, opts, expect, "%s %s (%s)" % (tag, opts, "took effect" if effect else "overridden"), default)
    _run_cell(pl, topo, counts, ref, False, (), {"update": "None", "var": "None", "c_only": cls != "big", "lik_rows": cls != "big"}, tag + " likelihood only")
    _levels_on_the_same_plan(pl, topo, counts, ref, default, tag)
    pl.close()


@pytest.mark.parametrize("recipe", [("edges", "empty_first"), ("edges", "empty_first", 193)], ids=["192", "193"])
def test_leaf_size_edges_against_the_extended_oracle(hip, recipe):
    """sd = sqrt(cov0 - |W|^2 - |Tt|^2) cancels hardest at densely observed leaves: the masks with leaves of 16, 64, 128, 144, 160, 176
    and 192 (193) observations on the smallest tree against the 80-bit oracle, default route and level-by-level kernels."""
    from oracle.mra_extended import run_extended
    topo, locs, obs, y, counts, _ = _case("A", recipe)
    ext = run_extended(topo, locs, MK._spec(), y, R)
    pl = MK._plan(hip, topo, locs, y)
    for opts in ((), ((2, 0),)):
        _set(pl, opts)
        _, mean, sd = _predict(pl)
        e_m, where_m = _per_leaf(topo, counts, mean, ext["mean"], False)
        e_s, where_s = _per_leaf(topo, counts, sd, ext["sd"], True)
        print("%s %s vs extended: mean %.2e sd %.2e" % (recipe, opts, e_m, e_s))
        assert e_m < 1e-9, "%s %s: mean abs err by leaf: %s" % (recipe, opts, where_m)
        assert e_s < 1e-9, "%s %s: sd rel err by leaf: %s" % (recipe, opts, where_s)
    pl.close()


# ---- D. non-leaf blocks wider than 192 columns ----------------------------------------------------------------------------------
# name: (nx, ny, r0, M, observed fraction, kernel, jitter).  cw = r0 padded to 16: 208 for r0 = 200 (8 phantom knots) and 208, 192 for
# 192 - the last width k_trsm_rows2<12> takes.  Sparse masks keep every leaf within 12 observation tiles, dense ones need the big panels.
# "scattered": uniformly scattered 2-D locations, so that the nodes' row counts are ragged.
WIDE = {
    "r200_M1_sparse": (64, 64, 200, 1, 0.08, "m32", False),
    "r208_M1_dense_exp": (64, 64, 208, 1, 0.30, "exp", False),
    "r200_M2_dense": (128, 128, 200, 2, 0.30, "m32", False),
    "r208_M2_sparse_exp": (96, 96, 208, 2, 0.08, "exp", False),
    "r192_M1_sparse": (96, 96, 192, 1, 0.05, "m32", False),
    "r200_M1_scattered": (72, 72, 200, 1, 0.10, "m32", True),
}
ROW_SOLVES = ("prior", "predict")


@functools.lru_cache(maxsize=None)
def _wide(name):
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    from oracle.mra_levelwise import run_levelwise
    nx, ny, r, M, frac, kern, scattered = WIDE[name]
    rng = np.random.RandomState(31)
    np.random.seed(13)
    locs = rng.uniform(size=(nx * ny, 2)) if scattered else mt.genLocations2d(Nx=nx, Ny=ny)
    topo = build_topology(locs, r, M, 4)
    y = np.where(rng.uniform(size=(len(locs), 1)) < frac, rng.normal(size=(len(locs), 1)), np.nan)
    spec = mt.KernelSpec(mt.KIND_MATERN32, 0.25, 1.2) if kern == "m32" else mt.KernelSpec(mt.KIND_EXP, 0.3)
    return topo, locs, y, spec, run_levelwise(topo, locs, spec, y, R)


def _wide_plan(hip, topo, locs, y, spec):
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, R); pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
    return pl


@pytest.mark.parametrize("name", sorted(WIDE))
def test_blocks_wider_than_192(hip, name):
    from pymra_amd.sharding import shard_topology
    topo, locs, y, spec, ref = _wide(name)
    r0, M = WIDE[name][2], WIDE[name][3]
    cw = max(int(c) for c in topo.cw)
    assert cw == (r0 + 15) // 16 * 16 and [int(c) for c in topo.cw[:M]] == [cw] * M
    counts = MK.leaf_counts(topo, np.isfinite(y.ravel()))
    fit = int(RC.tiles(counts).max()) <= 12
    assert fit == ("sparse" in name or "scattered" in name), (name, int(counts.max()))
    if "scattered" in name:
        rows = (topo.node_row1 - topo.node_row0)[np.asarray(topo.node_leaf, dtype=bool)]
        assert len(set(int(v) for v in rows)) > 1                  # ragged row tiles
    pl = _wide_plan(hip, topo, locs, y, spec)
    pl.set_option(hip.MRA_OPT_KERNEL_TIMING, 1)
    got = _predict(pl)
    # wider than 192: no variance on the way (k_leaf_moments at the end); 192: the LDS row solves accumulate it
    narrow = cw <= 192
    expect = dict(path="Levels", acc_var=narrow and fit, var="FinishVar" if narrow and fit else "Moments", update="Gemm", solve_fused=False,
                  extract_mean=True, c_fix="Phantom" if fit else "Fill")
    if not fit:
        expect["chol"] = "BigPanels"
    _check_route(pl, expect, name)
    st = {k["name"]: k["launches"] for k in pl.kernel_stats()}
    for fam in ROW_SOLVES:
        hit = [nm for nm, n in st.items() if nm.startswith("k_trsm_rows2 " + fam) and n > 0]
        assert hit, "%s: no %s row-solve family launched: %s" % (name, fam, st)
    pl.set_option(hip.MRA_OPT_KERNEL_TIMING, 0)
    _against(topo, counts, got, _ref3(ref), ORACLE_BARS, name + " vs oracle")
    # likelihood only, options 17 on / off bit-identical
    pl.run(True, False)
    lik = sum(pl.likelihood())
    assert abs(lik - ref["lik"]) <= ORACLE_BARS[0] * abs(ref["lik"]), name
    pl.set_option(hip.MRA_OPT_LIK_ROWS, 0)
    pl.run(True, False)
    assert sum(pl.likelihood()) == lik, name
    pl.set_option(hip.MRA_OPT_LIK_ROWS, 1)
    again = _predict(pl)
    assert again[0] == got[0] and np.array_equal(again[1], got[1]) and np.array_equal(again[2], got[2]), name
    for opt in (hip.MRA_OPT_GEMM_LDS, hip.MRA_OPT_FRONT_FUSED):
        pl.set_option(opt, 0)
        other = _predict(pl)
        _against(topo, counts, other, _ref3(ref), ORACLE_BARS, "%s option %d = 0 vs oracle" % (name, opt))
        _against(topo, counts, other, got, ROUTE_BARS, "%s option %d = 0 vs default" % (name, opt))
        pl.set_option(opt, 1)
    pl.close()
    # a 2-way split run through export / import equals the single plan
    plans, bufs = [], []
    for rk in range(2):
        lt, red = shard_topology(topo, 2, rk)
        assert red == 0
        p = _wide_plan(hip, lt, locs, y, spec)
        p.set_reduce_level(red)
        p.run(True, True, split=True)
        bufs.append(p.reduce_export())
        plans.append(p)
    mean, sd = np.zeros(topo.N), np.zeros(topo.N)
    for p in plans:
        p.reduce_import(bufs[0] + bufs[1])
        p.resume()
        assert abs(sum(p.likelihood()) - got[0]) <= 1e-12 * abs(got[0]), name
        m, _, d = p.predict(with_sd=True)
        mean += m; sd += d
        p.close()
    _against(topo, counts, (got[0], mean, sd), got, ROUTE_BARS, name + " 2-way split vs single plan")


def test_solve_and_sample_on_a_wide_tree(hip):
    """mra_solve (3 columns) and the prior factor of mra_sample accept a tree with blocks of 208 columns: the solve against the
    plan's own passes, the factor against the faithful oracle's prior covariance."""
    import test_gpu_sample as TS
    import test_gpu_solve as TV
    topo, locs, y, spec, ref = _wide("r200_M1_sparse")
    pl = _wide_plan(hip, topo, locs, y, spec)
    pl.run(True, True)
    Y = TV._columns(y, 3)
    mean, quad = pl.solve(TV._padded(topo, Y))
    TV._check_against_own_pass(hip, topo, locs, y, R, spec, Y, TV._caller(topo, mean), quad, range(3))
    assert topo.P <= 4608
    assert TS._check_prior_factor(pl, topo, locs, spec) > 0          # r0 = 200: 8 phantom knot columns stay inert
    pl.close()
