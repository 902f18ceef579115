"""Sharded passes on one GPU (every rank emulated in this process: MRA_RUN_SPLIT, export, host sum, import, resume) at the shard
depths, tree families and kernels that the other GPU tests leave out, and the sharded MLE loop itself.  GPU only.

The cases are tests/_sharded_cases.py's table (checked against the oracle alone by tests/test_sharded_cases_cpu.py).  For every case:

  A1  the ranks' owned caller rows are pairwise disjoint and together the reported rows of the unsharded tree;
  A2  a rank's mean and var are exactly 0.0 at every caller row it does not own;
  A3  the summed mean and sqrt(var), and every rank's likelihood, against the unsharded level-wise oracle at the single plan's bounds
      (test_hip_matches_oracle_and_reference_goldens: 1e-11 relative / 1e-10 / 1e-9 relative; u3 1e-8 / 1e-8 / 1e-6; the random
      geometries at test_random_geometries' 1e-9 max(1, |lik|) / 1e-8 / 1e-7 absolute);
  A4  the spread of the likelihood over the ranks within 1e-12 |lik|, and the sharded result against the single plan on the device
      within 1e-12 relative, 1e-11 (mean) and 1e-12 (var): test_sharded_4_and_8_ways_on_one_gpu's bounds (not for u3, where the
      oracle bound governs).

Every case prints its measured spread and errors before it asserts."""
import numpy as np
import pytest

import _cases as K
import _sharded_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _set_kernel(pl, spec):
    pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale, spec.circular)


def _plan(hip, topo, p, spec=None):
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(p["locs"]); pl.set_obs(p["y"], p["R"])
    _set_kernel(pl, spec or p["spec"])
    return pl


_SINGLE = {}


def _single(hip, cid):
    """(lik, mean, var) of one unsharded plan of the case, once per module."""
    if cid not in _SINGLE:
        p = SC.problem(cid)
        pl = _plan(hip, p["topo"], p)
        try:
            pl.run(True, True)
            _SINGLE[cid] = (sum(pl.likelihood()),) + tuple(pl.predict())
        finally:
            pl.close()
    return _SINGLE[cid]


def check_ranks(tag, topo, ranks, ref, bounds, single=None):
    """A1 - A4 for the per-rank results of one sharded predictive pass; prints the measured figures first.  -> (mean, var) summed."""
    own = SC.check_partition(topo, [r["topo"] for r in ranks])                 # A1
    SC.check_own_rows_only(ranks, own, topo.N)                                 # A2
    liks = [r["lik"] for r in ranks]
    mean, var = np.sum([r["mean"] for r in ranks], axis=0), np.sum([r["var"] for r in ranks], axis=0)
    spread = (max(liks) - min(liks)) / abs(ref["lik"])
    errs = [SC.errors_vs_oracle(l, mean, var, ref, bounds) for l in liks]
    e_l, e_m, e_s = max(e[0] for e in errs), errs[0][1], errs[0][2]
    line = "%s: rank spread %.2e | vs oracle lik %.2e mean %.2e sd %.2e" % (tag, spread, e_l, e_m, e_s)
    if single is not None:
        s_l = max(abs(l - single[0]) for l in liks) / abs(single[0])
        s_m, s_v = float(np.max(np.abs(mean - single[1]))), float(np.max(np.abs(var - single[2])))
        line += " | vs single plan lik %.2e mean %.2e var %.2e" % (s_l, s_m, s_v)
    print(line)
    assert np.all(np.isfinite(liks)) and np.all(np.isfinite(mean)) and np.all(np.isfinite(var)), tag
    assert e_l <= bounds[0] and e_m < bounds[1] and e_s < bounds[2], line      # A3
    assert spread <= SC.SPREAD, line                                           # A4
    if single is not None:
        assert s_l <= SC.SINGLE_LIK and s_m < SC.SINGLE_MEAN and s_v < SC.SINGLE_VAR, line
    return mean, var


def _emulate(hip, p, world, topo=None, spec=None):
    return K.emulate_world_on_one_gpu(hip, topo if topo is not None else p["topo"], p["locs"], p["y"], p["R"], spec or p["spec"], world, per_rank=True)


@pytest.mark.parametrize("cid,world", SC.CELLS, ids=SC.CELL_IDS)
def test_sharded_case(hip, cid, world):
    p = SC.problem(cid)
    topo = p["topo"]
    ref = SC.oracle(cid)
    single = _single(hip, cid) if p["single"] else None
    ranks = _emulate(hip, p, world)
    s = SC.SHARD_LEVEL[cid, world]
    assert len(ranks) == world and all(r["red"] == s - 1 for r in ranks)
    rt = ranks[0]["route"]
    print("%s-w%d: shard level %d of %d levels, path %s, direct_parent %s, side %s" % (cid, world, s, topo.n_levels, rt["path"], rt["direct_parent"], rt["side"]))
    check_ranks("%s-w%d" % (cid, world), topo, ranks, ref, p["bounds"], single)
    if cid in ("g32", "deep"):
        assert all(r["route"]["path"] == "Fused" for r in ranks)
    if s == topo.n_levels - 1:
        # the reduce level is the leaves' parents: their fronts are assembled from the leaves' Schur blocks, without the identity
        assert not any(r["route"]["direct_parent"] for r in ranks)
    if cid == "empty":
        # rank 0 owns no observation: nothing to fix in a C block, the predict-only leaf work has nothing to do.  Its rows still hear of
        # the other ranks' observations through the knots of the levels above (the oracle's mean there reaches 1.07 and its variance
        # is below the prior's), so rank 0's rows are held to the oracle on their own
        own0 = K.owned_rows(ranks[0]["topo"])
        assert not np.isfinite(p["y"].ravel()[own0]).any()
        assert all(r["route"]["side"] for r in ranks)              # the side stream was opened on rank 0 too
        assert ranks[0]["route"]["c_fix"] == "None" and all(r["route"]["c_fix"] != "None" for r in ranks[1:]), [r["route"]["c_fix"] for r in ranks]
        e_m = float(np.max(np.abs(ranks[0]["mean"][own0] - ref["mean"][own0])))
        e_s = K.rel(np.sqrt(ranks[0]["var"][own0]), ref["sd"][own0])
        print("empty-w4 rank 0 rows: mean %.2e sd %.2e vs oracle" % (e_m, e_s))
        assert e_m < p["bounds"][1] and e_s < p["bounds"][2]
        assert np.max(np.abs(ref["mean"][own0])) > 0.5


# ---- the MLE loop ---------------------------------------------------------------------------------------------------------------
class _World:
    """``world`` shard plans created once and reused pass after pass, as bench.py --gpus N --mle keeps them."""

    def __init__(self, hip, p, world):
        self.plans, self.topos = [], []
        try:
            for lt, red in SC.local_topologies(p["topo"], world):
                pl = _plan(hip, lt, p)
                self.plans.append(pl)
                self.topos.append(lt)
                pl.set_reduce_level(red)
        except BaseException:
            self.close()
            raise

    def set_kernel(self, spec):
        for pl in self.plans:
            _set_kernel(pl, spec)

    def run(self, predict):
        """One sharded pass: every rank up to the reduce level, the host sum of the exported buffers, import and resume on each."""
        bufs = []
        for pl in self.plans:
            pl.run(True, predict, split=True)
            bufs.append(pl.reduce_export())
        tot = np.sum(bufs, axis=0)
        ranks = []
        for pl, lt in zip(self.plans, self.topos):
            pl.reduce_import(tot)
            pl.resume()
            r = dict(topo=lt, lik=sum(pl.likelihood()))
            if predict:
                r["mean"], r["var"] = pl.predict()
            ranks.append(r)
        return ranks

    def close(self):
        for pl in self.plans:
            pl.close()


def test_sharded_mle_loop_on_one_device(hip):
    """BASELINE config 5's pattern in one process: four shard plans created once, Nelder-Mead over the range parameter through
    sharding.sharded_minimize, every evaluation set_kernel + a likelihood-only split pass on each rank with one host sum in between,
    then one predictive pass at the optimum.

    Data: g64m's tree (64^2, r 16, M 3, shard level 1) and mask, with the values of test_sharded_nelder_mead_equals_single_rank's
    recipe at this size - a draw of the Matern32 field at l = 0.15 by a dense Cholesky of all 4096 points (three seconds of host
    time, so the smaller g32 stand-in is not needed) plus noise of variance R - so that the optimum is interior, near 0.15."""
    from oracle.mra_levelwise import run_levelwise
    from pymra_amd.sharding import sharded_minimize
    mt = K.mt
    cs = K.load_case("g64m")
    topo, locs, R, N = cs["topo"], cs["locs"], cs["c"]["R"], len(cs["locs"])
    rng = np.random.RandomState(5)
    S = np.asarray(mt.Matern32(locs, locs, l=0.15, sig=1.0))
    f = np.linalg.cholesky(S + 1e-10 * np.eye(N)) @ rng.normal(size=N)
    y = np.where(np.isfinite(np.asarray(cs["y_obs"]).ravel()), f + np.sqrt(R) * rng.normal(size=N), np.nan).reshape(-1, 1)
    spec = lambda kappa: mt.KernelSpec(mt.KIND_MATERN32, kappa, 1.0)
    p = dict(topo=topo, locs=locs, y=y, R=R, spec=spec(0.3))
    world = 4
    W = _World(hip, p, world)
    one = _plan(hip, topo, p)
    try:
        spreads = []

        def evaluate(kappa):
            W.set_kernel(spec(kappa))
            liks = [r["lik"] for r in W.run(False)]
            spreads.append((max(liks) - min(liks)) / abs(liks[0]))
            assert spreads[-1] <= SC.SPREAD, (kappa, liks)
            return liks[0]

        def evaluate_one(kappa):
            _set_kernel(one, spec(kappa))
            one.run(True, False)
            return sum(one.likelihood())

        k_hat, f_hat, calls, res = sharded_minimize(evaluate, 0.3, 0, lambda b: b, maxfev=40)
        assert 5 < len(calls) <= 41
        # (a) every evaluation against a single unsharded plan reused the same way
        e_a = max(abs(v - evaluate_one(k)) / abs(v) for k, v in calls)
        # (c) the optimiser on the single plan: both stop within xatol = 1e-3 of the optimum, not necessarily by the same simplex path
        k_one, f_one, calls_one, _ = sharded_minimize(evaluate_one, 0.3, 0, lambda b: b, maxfev=40)
        # (b) the oracle at the first, the best and the last kappa
        best = min(calls, key=lambda kv: kv[1])
        e_b = max(abs(v - run_levelwise(topo, locs, spec(k), y, R, predict=False)["lik"]) / abs(v) for k, v in (calls[0], best, calls[-1]))
        print("mle: %d evaluations, kappa_hat %.6f (single plan %.6f, %d evaluations), worst rank spread %.2e, vs single plan %.2e, vs oracle %.2e"
              % (len(calls), k_hat, k_one, len(calls_one), max(spreads), e_a, e_b))
        assert e_a <= SC.SINGLE_LIK
        assert e_b <= SC.STD[0]
        assert 0.05 < k_hat < 0.29 and abs(k_hat - k_one) <= 2e-3
        assert best[1] <= f_hat < calls[0][1]
        # (e) the first kappa again, after all the others: bit for bit
        assert evaluate(calls[0][0]) == calls[0][1]
        # (d) one predictive pass at kappa_hat on the plans the loop used, against fresh sharded plans, the single plan and the oracle:
        # nothing stale from the likelihood-only passes (W rows, cached leaf blocks)
        W.set_kernel(spec(k_hat))
        ranks = W.run(True)
        ref = run_levelwise(topo, locs, spec(k_hat), y, R)
        _set_kernel(one, spec(k_hat))
        one.run(True, True)
        single = (sum(one.likelihood()),) + tuple(one.predict())
        check_ranks("mle predict at kappa_hat", topo, ranks, ref, SC.STD, single)
        fresh = _emulate(hip, p, world, spec=spec(k_hat))
        e_d = [max(abs(a["lik"] - b["lik"]) / abs(b["lik"]) for a, b in zip(ranks, fresh)),
               max(float(np.max(np.abs(a["mean"] - b["mean"]))) for a, b in zip(ranks, fresh)),
               max(float(np.max(np.abs(a["var"] - b["var"]))) for a, b in zip(ranks, fresh))]
        print("mle predict at kappa_hat, reused plans vs fresh sharded plans, rank by rank: lik %.2e mean %.2e var %.2e" % tuple(e_d))
        assert e_d[0] <= SC.SINGLE_LIK and e_d[1] < SC.SINGLE_MEAN and e_d[2] < SC.SINGLE_VAR
    finally:
        W.close()
        one.close()


# ---- the refusal of deep reduce levels, and plan state at the leaves' parents ----------------------------------------------------
def _finite_lik(pl):
    lik = sum(pl.likelihood())
    assert np.isfinite(lik)
    return lik


@pytest.mark.parametrize("world,red", [(17, 2), (65, 3)])
def test_reduce_level_too_deep_is_refused(hip, world, red):
    """The deep tree keeps the fronts of the leaves' parents as their panel columns only: a reduce level at the leaves' grandparents
    (world 17: shard level 3) or parents (world 65: the leaf level) is refused with MRA_ERR_INVALID and the way out, and the plan is
    as good as new afterwards."""
    from pymra_amd.sharding import shard_topology
    p = SC.problem("deep")
    lt, r = shard_topology(p["topo"], world, 0)
    assert r == red == (p["topo"].n_levels - 3 if world == 17 else p["topo"].n_levels - 2)
    pl, fresh = _plan(hip, lt, p), None
    try:
        with pytest.raises(hip.MraError) as e:
            pl.set_reduce_level(red)
        assert e.value.code == -1 and "MRA_NO_LOWRANK_PARENT" in str(e.value)
        pl.set_reduce_level(-1)
        pl.run(True, True)
        lik = _finite_lik(pl)
        mean, var = pl.predict()
        fresh = _plan(hip, lt, p)
        fresh.run(True, True)
        m2, v2 = fresh.predict()
        assert lik == _finite_lik(fresh) and np.array_equal(mean, m2) and np.array_equal(var, v2)
    finally:
        pl.close()
        if fresh is not None:
            fresh.close()


def test_deepest_accepted_reduce_level(hip):
    """World 5 on the deep tree: shard level 2, reduce level 1 - the deepest one a plan with panel-only parent fronts takes."""
    from pymra_amd.sharding import shard_topology
    p = SC.problem("deep")
    lt, red = shard_topology(p["topo"], 5, 0)
    assert red == 1 == p["topo"].n_levels - 4
    pl = _plan(hip, lt, p)
    try:
        pl.set_reduce_level(red)
    finally:
        pl.close()


def test_whole_parent_fronts_take_the_deep_reduce_level(hip, monkeypatch):
    """MRA_NO_LOWRANK_PARENT=1 before the plans are created, as the refusal says: 17 ranks on the deep tree (shard level 3, the reduce
    level at the leaves' grandparents) against the default single plan and the oracle."""
    p = SC.problem("deep")
    single = _single(hip, "deep")                       # the default plan: before the variable is set
    ref = SC.oracle("deep")
    monkeypatch.setenv("MRA_NO_LOWRANK_PARENT", "1")
    ranks = _emulate(hip, p, 17)
    assert all(r["red"] == 2 for r in ranks)
    check_ranks("deep-w17 whole parent fronts", p["topo"], ranks, ref, p["bounds"], single)


def test_state_errors_at_the_leaves_parents(hip):
    """test_state_errors_are_status_codes_not_faults' parts (2) and (3) on a g32 world-16 rank, whose reduce level is the leaves'
    parents: resume without a split pending and a pass that would skip the exchange are MRA_ERR_STATE, and a split run abandoned
    half way leaves nothing behind - the next complete one gives the bits of a fresh plan."""
    from pymra_amd.sharding import shard_topology
    p = SC.problem("g32")
    lt, red = shard_topology(p["topo"], 16, 3)
    assert red == p["topo"].n_levels - 2

    def complete(pl):
        pl.run(True, True, split=True)
        pl.reduce_import(pl.reduce_export())
        pl.resume()
        return (sum(pl.likelihood()),) + tuple(pl.predict())

    pl, fresh = _plan(hip, lt, p), None
    try:
        pl.set_reduce_level(red)
        with pytest.raises(hip.MraError) as e:
            pl.resume()
        assert e.value.code == -4
        with pytest.raises(hip.MraError) as e:
            pl.run(True, True)
        assert e.value.code == -4
        pl.run(True, True, split=True)                   # abandoned: never resumed
        got = complete(pl)
        fresh = _plan(hip, lt, p)
        fresh.set_reduce_level(red)
        want = complete(fresh)
        assert np.isfinite(got[0]) and got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        again = complete(pl)
        assert again[0] == got[0] and np.array_equal(again[1], got[1]) and np.array_equal(again[2], got[2])
    finally:
        pl.close()
        if fresh is not None:
            fresh.close()
