"""The host-evaluated covariance path (MRA_KERNEL_HOST) on every route it can take (GPU only).

``cov`` is an opaque callable or a dense matrix: the host evaluates C(S_j, Q_j), C(S_j, O_j) and C(x,x) block by block
(HipPlan.upload_host_cov), the EPI_HOSTCOV epilogue of k_gemm_nt_lds, k_gemm_nt and k_leaf_gemm reads them back, k_init_yblock and
k_leaf_moments read C(x,x) per row.  The covariances of tests/_hostcov_cells.py are neither stationary nor isotropic, so a wrong
row offset, block stride or column order changes the numbers, and the comparator is the level-wise oracle run with the same
callable - not the device path, with which a stationary host run would share every bug but the epilogue's.

Every cell of the host table asserts its route (HipPlan.route()) and compares likelihood, predictive mean and sd with the oracle, a
non-default option tuple with the default route, a likelihood-only pass with the predictive one, and a second predictive pass bit
for bit.  Then the plan transitions (new mask, new parameters, host -> device kernel -> host) against fresh plans, the stationary
cross-check of host against device epilogue, a 4-way sharded host plan, and MRATree from a callable and from a dense matrix.

Bars: tests/test_gpu_routes.py's standing ones (ORACLE_BARS, ROUTE_BARS), none derived from a HIP result;
tests/test_hostcov_table.py shows that one ulp in every covariance value moves the oracle by less than a hundredth of them."""
import numpy as np
import pytest

import _cases as K
import _hostcov_cells as HC
import _route_cells as RC
import test_gpu_likelihood_masks as MK
import test_gpu_routes as TR
from test_gpu_routes import ORACLE_BARS, ROUTE_BARS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _host_plan(hip, topo, locs, y, R, cov):
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, R); pl.upload_host_cov(cov, locs, y)
    return pl


def _same_bits(a, b, tag):
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), \
        "%s: lik %.17g vs %.17g, mean differs at %d rows, sd at %d" % (tag, a[0], b[0], int((a[1] != b[1]).sum()), int((a[2] != b[2]).sum()))


# ---- a. the table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,recipe", HC.GROUPS, ids=["%s-%s" % (k, "-".join(str(x) for x in m)) for k, m in HC.GROUPS])
def test_hostcov_table(hip, key, recipe):
    topo, locs, cov, R, y, counts = HC.case(key, recipe)
    ref = HC.oracle(key, recipe)
    pl = _host_plan(hip, topo, locs, y, R, cov)
    assert pl.d == (1 if key == "T1" else 2)
    cells = [c for c in HC.CELLS if (c["tree"], c["mask"]) == (key, recipe)]
    assert cells[0]["predict"] and not cells[0]["opts"]          # the default route first: the others are compared with it
    default = None
    for c in cells:
        tag = "host %s %s predict=%s %s" % (key, recipe, c["predict"], c["opts"])
        assert int(RC.tiles(counts).max()) == c["ntl"], (tag, int(counts.max()))
        got = TR._run_cell(pl, topo, counts, ref, c["predict"], c["opts"], c["expect"], tag, default if c["opts"] else None)
        for o, v in {3: RC.DEFAULTS[3], 6: RC.DEFAULTS[6], **dict(c["opts"])}.items():
            assert pl.get_option(o) == v, (tag, o)               # the option took effect (the route alone does not show option 3)
        rt = pl.route()
        assert rt["n_leaves"] == len(counts) and rt["init_yblock"] and not rt["side"], tag
        print("%s: route %s" % (tag, " ".join("%s=%s" % (k, rt[k]) for k in ("path", "leaf_resident", "acc_var", "c_fix", "chol", "var", "update"))
                                + " MRA_OPT_GEMM_LDS=%d DIM=%d" % (pl.get_option(3), pl.d)))
        if c["predict"] and not c["opts"]:
            default = got
    pl.close()


# ---- b. plan transitions ----------------------------------------------------------------------------------------------------------
def _fresh(hip, topo, locs, y, R, cov):
    pl = _host_plan(hip, topo, locs, y, R, cov)
    out = TR._predict(pl)
    pl.close()
    return out


def test_plan_transitions_equal_a_fresh_plan(hip):
    """One plan on A through a new mask, new parameters and host -> device kernel -> host: every state bit for bit what a fresh plan
    gives; the calls a host plan refuses leave it as it was."""
    topo, locs, cov, R, y, counts = HC.case("A", HC.HEDGE)
    y2 = HC.case("A", HC.CLOUD)[4]
    other = HC.cov2_at(0.31)
    pl = _host_plan(hip, topo, locs, y, R, cov)
    first = TR._predict(pl)
    assert pl.route()["leaf_resident"] and pl.route()["path"] == "Levels"
    TR._against(topo, counts, first, TR._ref3(HC.oracle("A", HC.HEDGE)), ORACLE_BARS, "transitions: first pass vs oracle")

    # what a host plan cannot do stays an error code, and the next pass has the same bits
    leaves = np.nonzero(topo.node_leaf)[0].astype(np.int32)
    sites, at = np.asarray(locs[:3], dtype=np.float64) + 1e-3, leaves[:3]
    refused = [lambda: pl.solve(np.zeros((1, topo.P))), lambda: pl.cov_apply(np.zeros((1, topo.P))), lambda: pl.predict_sites(sites, at),
               lambda: pl.sites_cov(sites, at), lambda: pl.sample(1, seed=1), lambda: pl.sample_sites(sites, at, 1, seed=1)]
    for k, call in enumerate(refused):
        with pytest.raises(hip.MraError) as ei:
            call()
        assert ei.value.code == -1, k                              # MRA_ERR_INVALID
        if k % 2:
            _same_bits(TR._predict(pl), first, "pass after refused call %d" % k)
    _same_bits(TR._predict(pl), first, "pass after the refused calls")

    # a new mask invalidates the blocks: MRA_ERR_STATE until they are uploaded again, then a fresh plan's bits
    pl.set_obs(y2, R)
    with pytest.raises(hip.MraError) as ei:
        pl.run(True, True)
    assert ei.value.code == -4
    pl.upload_host_cov(cov, locs, y2)
    second = TR._predict(pl)
    _same_bits(second, _fresh(hip, topo, locs, y2, R, cov), "new mask vs fresh plan")
    assert second[0] != first[0]

    # new parameters without set_obs (an MLE over a callable)
    pl.upload_host_cov(other, locs, y2)
    third = TR._predict(pl)
    _same_bits(third, _fresh(hip, topo, locs, y2, R, other), "new parameters vs fresh plan")
    assert third[0] != second[0]

    # host -> device kernel -> host
    s = MK._spec()
    pl.set_kernel(s.kind, s.l, s.sig, s.scale)
    dev = TR._predict(pl)
    assert pl.route()["path"] == "Fused"
    fresh = MK._plan(hip, topo, locs, y2)
    _same_bits(dev, TR._predict(fresh), "device kernel after host blocks vs fresh device plan")
    fresh.close()
    pl.upload_host_cov(other, locs, y2)
    _same_bits(TR._predict(pl), third, "host blocks after a device kernel vs the host pass before it")
    assert pl.route()["path"] == "Levels"

    # and back to where it started
    pl.set_obs(y, R)
    pl.upload_host_cov(cov, locs, y)
    _same_bits(TR._predict(pl), first, "back on the first mask and covariance")
    pl.close()


# ---- c. stationary cross-check ----------------------------------------------------------------------------------------------------
def test_stationary_callable_equals_the_device_kernel_level_by_level(hip):
    """The one test that ties host and device together: MK._spec() through an opaque callable against the same plan's device pass
    with MRA_OPT_FUSED off - the same kernels apart from the epilogue - at the bars of TR._levels_on_the_same_plan."""
    from pymra_amd.MRATree import probe_cov
    topo, locs, _, R, y, counts = HC.case("A", HC.HEDGE)
    s = MK._spec()
    opaque = lambda a, b: np.asarray(s.evaluate(a, b), dtype=np.float64) + 0.0
    assert probe_cov(opaque, 2, np.asarray(locs, dtype=np.float64)) is None
    pl = _host_plan(hip, topo, locs, y, R, opaque)
    host = TR._predict(pl)
    assert pl.route()["path"] == "Levels" and pl.route()["leaf_resident"]
    pl.set_kernel(s.kind, s.l, s.sig, s.scale)
    pl.set_option(hip.MRA_OPT_FUSED, 0)
    dev = TR._predict(pl)
    assert pl.route()["path"] == "Levels"
    TR._against(topo, counts, host, dev, (1e-11, 1e-9, 1e-8), "stationary callable vs device kernel, level by level")
    pl.close()


# ---- d. sharded -------------------------------------------------------------------------------------------------------------------
def emulate_world_hostcov(hip, topo, locs, y, R, cov, world):
    """K.emulate_world_on_one_gpu with upload_host_cov on every rank's shard_topology in place of set_kernel.
    -> (liks[world], mean, sd, routes[world]), mean and sd assembled from the ranks' own rows."""
    from pymra_amd.sharding import shard_topology
    plans, bufs = [], []
    for rk in range(world):
        lt, red = shard_topology(topo, world, rk)
        p = hip.HipPlan(lt, 0)
        p.set_locs(locs); p.set_obs(y, R); p.upload_host_cov(cov, locs, y)
        p.set_reduce_level(red)
        p.run(True, True, split=True)
        bufs.append(p.reduce_export())
        plans.append(p)
    tot = np.sum(bufs, axis=0)
    liks, routes, mean, sd = [], [], np.zeros(topo.N), np.zeros(topo.N)
    for p in plans:
        p.reduce_import(tot)
        p.resume()
        liks.append(sum(p.likelihood()))
        routes.append(p.route())
        m, _, d = p.predict(with_sd=True)
        mean += m; sd += d
        p.close()
    return liks, mean, sd, routes


def test_sharded_host_plan(hip):
    """Four ranks of S emulated on one GPU: upper nodes' rows are kept children and orphan knot rows, the predict-only leaf work goes to
    the side stream."""
    c = HC.SHARDED
    topo, locs, cov, R, y, counts = HC.case(c["tree"], c["mask"])
    pl = _host_plan(hip, topo, locs, y, R, cov)
    single = TR._predict(pl)
    pl.close()
    liks, mean, sd, routes = emulate_world_hostcov(hip, topo, locs, y, R, cov, c["world"])
    assert len(liks) == c["world"]
    for rk, (lk, rt) in enumerate(zip(liks, routes)):
        diff = {k: (rt[k], v) for k, v in c["expect"].items() if rt[k] != v}
        assert not diff, "rank %d: route (got, expected) %s" % (rk, diff)
        assert abs(lk - single[0]) <= 1e-12 * abs(single[0]), "rank %d: likelihood rel err %.3e vs the single plan" % (rk, abs(lk - single[0]) / abs(single[0]))
    print("host sharded S world 4: route %s" % " ".join("%s=%s" % (k, routes[0][k]) for k in ("path", "side", "acc_var", "c_fix", "chol", "var", "update")))
    TR._against(topo, counts, (liks[0], mean, sd), single, ROUTE_BARS, "host sharded S world 4 vs single plan")
    o_liks, o_mean, o_var, _ = K.emulate_world_oracle(topo, locs, y, R, cov, c["world"])
    for rk in range(c["world"]):
        TR._against(topo, counts, (liks[rk], mean, sd), (o_liks[rk], o_mean, np.sqrt(o_var)), ORACLE_BARS, "host sharded S world 4 rank %d vs sharded oracle" % rk)
    TR._against(topo, counts, (liks[0], mean, sd), TR._ref3(HC.oracle(c["tree"], c["mask"])), ORACLE_BARS, "host sharded S world 4 vs oracle")


# ---- e. through MRATree -----------------------------------------------------------------------------------------------------------
def _tree_results(tree):
    mean, sd = tree.predict()
    return float(tree.getLikelihood()[0, 0]), np.asarray(mean).ravel().copy(), np.asarray(sd).ravel().copy()


def test_mratree_from_a_callable_and_from_a_dense_matrix(hip):
    import pymra_amd
    import pymra_amd.MRATools as mt
    topo, locs, cov, R, y, counts = HC.case("A", HC.HEDGE)
    n, r0, M = RC.TREES["A"]
    np.random.seed(7)                                                   # MK._tree's seed: the same knot draws, the cached oracle
    tree = pymra_amd.MRATree(locs, r0, cov, y, R, M=M, J=4)
    assert tree.kernel is None
    assert np.array_equal(tree.topology.perm, topo.perm) and np.array_equal(tree.topology.knot_rows, topo.knot_rows)
    got = _tree_results(tree)
    TR._against(topo, counts, got, TR._ref3(HC.oracle("A", HC.HEDGE)), ORACLE_BARS, "MRATree(cov2) on A vs oracle")
    # what needs a device kernel says so and leaves the tree as it was
    for call in (lambda: tree.simulate(1, seed=3), lambda: tree.solve(np.zeros(topo.N)), lambda: tree.predictAt(np.asarray(locs[:3]) + 1e-3),
                 lambda: tree.reevaluate(cov)):
        with pytest.raises(NotImplementedError):
            call()
        assert tree.kernel is None and float(tree.getLikelihood()[0, 0]) == got[0]
    tree.plan.run(True, True)
    assert sum(tree.plan.likelihood()) == got[0]

    # a dense ndarray on a 40 x 40 grid (r0 16, M 2) against the callable it was evaluated from
    g = mt.genLocations2d(Nx=40, Ny=40)
    yg = MK._y(np.random.RandomState(5).uniform(size=len(g)) < 0.4)
    np.random.seed(7)
    tc = pymra_amd.MRATree(g, 16, cov, yg, R, M=2, J=4)
    np.random.seed(7)
    td = pymra_amd.MRATree(g, 16, HC.cov2(g, g), yg, R, M=2, J=4)
    assert tc.kernel is None and td.kernel is None and np.array_equal(tc.topology.perm, td.topology.perm)
    cnt = MK.leaf_counts(tc.topology, np.isfinite(yg.ravel()))
    TR._against(tc.topology, cnt, _tree_results(td), _tree_results(tc), ROUTE_BARS, "MRATree(dense ndarray) vs MRATree(callable), 40 x 40")
