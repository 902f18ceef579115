"""MRA_OPT_PRIOR_REUSE (option 24): a fused pass that follows one with the same kernel, locations and knots keeps that pass's prior
(GPU only).

The prior of a pass - Lp / invP / Wk per level, W at every row, the prior variance - does not depend on y, the noise or (where W was
written at every row) the mask.  A pass that keeps it launches neither prior kernel: it writes W's y block again, puts the prior
variance back and re-runs the row cascade on the leaves whose rows the last pass's plain update rewrote (those of more than eight
observation tiles beside LeafUpdate::InCascade).  It runs the same kernels on the same bits in the same order as a pass that computes
its prior, so EVERY comparison here is bit for bit (np.array_equal on the likelihood terms, mean and var): a difference is a stale or
missing refresh, not rounding.  "Fresh" is a new plan that runs only that one pass.  Kernel timing is on before the first pass, and
``kernel_stats()`` tells which prior family launched: the knot family (k_knot_chain + k_prior_cascade<KNOT>) and the row family
(k_prior_cascade row pass) - "full": the flops of the fresh plan's launch, "dirty": one launch of fewer flops, "none": no launch.

The refused pass of the invalidation cases: the issue names the NaN pivot of tests/test_gpu_likelihood_masks.py.  That recipe needs
host-evaluated covariance blocks on a one-node tree, which never takes the fused path and has no prior launch to count; it is run
here as it stands (results only), and the case that matters - a refused pass on a FUSED plan whose kernel is not set again - is
provoked by the Poisson fit of tests/test_gpu_laplace.py that leaves the doubles in its second pass (MRA_ERR_NOT_SPD, handled)."""
import numpy as np
import pytest

import _cases as K
import _laplace as LP
import _line_cells as LC
import _route_cells as RC
import _sharded_cases as SH
import test_gpu_likelihood_masks as MK
import test_gpu_sphere as SP

pytestmark = pytest.mark.gpu

R = MK.R
KNOTS, ROWS = "k_knot_chain + k_prior_cascade<KNOT> knot pass", "k_prior_cascade row pass"
IN_CASCADE = ((7, 0),)                      # MRA_OPT_LEAF_SOLVE 0: with at most 2 n_cu leaves the default is the fused solve + update
T96 = (96, 32, 3)                           # 64 leaves of 144 rows: a fully observed leaf has 9 tiles, one over the 8-tile split


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


# ---- plans, passes, launches ---------------------------------------------------------------------------------------------------------
def _plan(hip, topo, locs, y, spec=None, opts=(), noise=R):
    s = spec or MK._spec()
    pl = hip.HipPlan(topo, 0)
    pl.set_option(hip.MRA_OPT_KERNEL_TIMING, 1)
    for o, v in opts:
        pl.set_option(o, v)
    pl.set_locs(locs); pl.set_obs(y, noise); pl.set_kernel(s.kind, s.l, s.sig, s.scale, bool(getattr(s, "circular", False)))
    return pl


def _fam(pl, name):
    st = [k for k in pl.kernel_stats() if k["name"].startswith(name)]
    assert len(st) == 1, [k["name"] for k in pl.kernel_stats()]
    return st[0]


def _pass(pl, predict=True):
    """one pass -> dict(lik (d, u), mean, var (None without predict), knots: launches of the knot family, rows: (launches, flops))"""
    pl.run(True, predict)
    mean, var = pl.predict() if predict else (None, None)
    rows = _fam(pl, ROWS)
    return dict(lik=pl.likelihood(), mean=mean, var=var, knots=_fam(pl, KNOTS)["launches"], rows=(rows["launches"], rows["flops"]))


def _same(got, want, tag):
    assert got["lik"] == want["lik"], "%s: likelihood terms %r vs fresh %r" % (tag, got["lik"], want["lik"])
    if want["mean"] is not None:
        assert np.array_equal(got["mean"], want["mean"]), "%s: mean differs at %d rows" % (tag, int(np.sum(got["mean"] != want["mean"])))
        assert np.array_equal(got["var"], want["var"]), "%s: var differs at %d rows" % (tag, int(np.sum(got["var"] != want["var"])))


def _launched(got, fresh, knots, rows, tag):
    """knots: True (the family launched as in the fresh pass) / False (no launch); rows: "full" / "dirty" / "none" """
    assert fresh["knots"] > 0 and fresh["rows"][0] == 1, (tag, fresh["knots"], fresh["rows"])
    assert got["knots"] == (fresh["knots"] if knots else 0), "%s: knot family launched %d times" % (tag, got["knots"])
    n, fl = got["rows"]
    if rows == "full":
        assert (n, fl) == fresh["rows"], "%s: row family %r, fresh %r" % (tag, got["rows"], fresh["rows"])
    elif rows == "dirty":
        assert n == 1 and 0 < fl < fresh["rows"][1], "%s: row family %r, fresh %r" % (tag, got["rows"], fresh["rows"])
    else:
        assert rows == "none" and n == 0, "%s: row family launched %d times" % (tag, n)


def _fresh(hip, topo, locs, y, predict=True, **kw):
    pl = _plan(hip, topo, locs, y, **kw)
    out = _pass(pl, predict)
    pl.close()
    return out


# ---- masks with leaves on both sides of the 8-tile split ---------------------------------------------------------------------------
def _split_mask(topo, full_every, seed):
    """40 % thinning, every ``full_every``-th leaf (from leaf ``seed % full_every``) fully observed"""
    obs = np.random.RandomState(seed).uniform(size=topo.N) < 0.4
    for k, i in enumerate(np.nonzero(topo.node_leaf)[0]):
        if k % full_every == seed % full_every:
            obs[MK._leaf_callers(topo, i)] = True
    return obs


def _both_sides(topo, obs):
    t = RC.tiles(MK.leaf_counts(topo, obs))
    return int((t > 8).sum()) > 0 and int((t <= 8).sum()) > 0 and t.max() <= 12


def _t96(seed=1, full_every=2):
    topo, locs = MK._tree(*T96)
    obs = _split_mask(topo, full_every, seed)
    assert _both_sides(topo, obs)
    return topo, locs, obs, MK._y(obs, seed=seed)


# ---- 1. both sides of the 8-tile split ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["96x96 r32 M3", "A32 edge counts to 192"])
def test_three_predict_passes_on_both_sides_of_the_split(hip, case):
    """predict, predict, predict with the leaf update inside the predictive cascade: the second and third pass keep the first one's
    prior, re-run the row cascade on the oversized leaves alone, and equal the first pass and a fresh plan to the bit."""
    if case.startswith("96"):
        topo, locs, obs, y = _t96()
    else:                                      # the cell of tests/_route_cells.py with update = InCascade and leaves of 0 .. 12 tiles
        topo, locs = MK._tree(*RC.TREES["A32"])
        obs = RC.make_obs(topo, locs, RC.E192)
        assert _both_sides(topo, obs)
        y = MK._y(obs)
    fresh = _fresh(hip, topo, locs, y, opts=IN_CASCADE)
    pl = _plan(hip, topo, locs, y, opts=IN_CASCADE)
    first = _pass(pl)
    assert pl.route()["update"] == "InCascade" and pl.route()["path"] == "Fused"
    _same(first, fresh, case + " pass 1")
    _launched(first, fresh, True, "full", case + " pass 1")
    for k in (2, 3):
        got = _pass(pl)
        _same(got, first, "%s pass %d vs pass 1" % (case, k))
        _same(got, fresh, "%s pass %d" % (case, k))
        _launched(got, fresh, False, "dirty", "%s pass %d" % (case, k))
    pl.close()


# ---- 2. pass kinds in sequence on one plan --------------------------------------------------------------------------------------------
def test_pass_kinds_in_sequence_on_one_plan(hip):
    topo, locs, obs1, y1 = _t96(seed=1)
    _, _, obs2, y2 = _t96(seed=4, full_every=3)                # other leaf counts, other oversized leaves
    assert not np.array_equal(MK.leaf_counts(topo, obs1) > 128, MK.leaf_counts(topo, obs2) > 128)
    y3 = np.where(obs2.reshape(-1, 1), np.random.RandomState(9).normal(size=(topo.N, 1)), np.nan)      # the same mask, new y
    fr = {(tag, pred): _fresh(hip, topo, locs, y, predict=pred, opts=IN_CASCADE)
          for tag, y in (("y1", y1), ("y2", y2), ("y3", y3)) for pred in (False, True)}
    assert fr[("y1", False)]["rows"][1] < fr[("y1", True)]["rows"][1]                # the likelihood-only pass walks gathered rows
    pl = _plan(hip, topo, locs, y1, opts=IN_CASCADE)
    steps = [
        ("lik, gathered rows", None, "y1", False, True, "full"),
        ("lik, rows kept as Observed", None, "y1", False, False, "none"),
        ("predict, knots kept, rows run", None, "y1", True, False, "full"),
        ("predict, all kept", None, "y1", True, False, "dirty"),              # (the oversized leaves' rows were rewritten by the last update)
        ("lik after predict", None, "y1", False, False, "dirty"),
        ("set_obs new mask, lik", y2, "y2", False, False, "none"),
        ("then predict", None, "y2", True, False, "none"),
        ("set_obs same mask new y, predict", y3, "y3", True, False, "dirty"),
        ("once more", None, "y3", True, False, "dirty"),
    ]
    for tag, new_y, key, pred, knots, rows in steps:
        if new_y is not None:
            pl.set_obs(new_y, R)
        got = _pass(pl, pred)
        assert pl.route()["path"] == "Fused" and (not pred or pl.route()["update"] == "InCascade")
        _same(got, fr[(key, pred)], tag)
        # a kept pass's "full" row launch is that of its own kind of pass; "dirty" is measured against the fresh launch of a predict pass
        _launched(got, fr[(key, True if rows == "dirty" else pred)], knots, rows, tag)
    pl.close()


def test_dirty_leaves_of_the_old_mask_are_rerun_after_set_obs(hip):
    """predict (dirties mask 1's oversized leaves), then set_obs with a mask whose oversized leaves are others, then predict: the leaves
    to re-run are the OLD mask's."""
    topo, locs, obs1, y1 = _t96(seed=1)
    _, _, obs2, y2 = _t96(seed=4, full_every=3)
    pl = _plan(hip, topo, locs, y1, opts=IN_CASCADE)
    _pass(pl)
    pl.set_obs(y2, R)
    pl.set_obs(y2, R)                                            # (twice: the list put aside at the first call must survive the second)
    fresh = _fresh(hip, topo, locs, y2, opts=IN_CASCADE)
    got = _pass(pl)
    _same(got, fresh, "new mask after a predict pass")
    _launched(got, fresh, False, "dirty", "new mask after a predict pass")
    pl.close()


# ---- 3. invalidation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["set_kernel", "set_locs", "lik_rows_off", "option_off"])
def test_invalidation(hip, what):
    topo, locs, obs, y = _t96()
    s = MK._spec()
    pl = _plan(hip, topo, locs, y, opts=IN_CASCADE)
    _pass(pl)
    assert _pass(pl)["knots"] == 0                               # the state to invalidate: a pass that keeps its prior
    kw = dict(opts=IN_CASCADE)
    if what == "set_kernel":
        pl.set_kernel(s.kind, 0.6 * s.l, s.sig, s.scale)
        pl.set_kernel(s.kind, s.l, s.sig, s.scale)
    elif what == "set_locs":
        locs = locs + 1e-4 * np.random.RandomState(2).uniform(-1.0, 1.0, size=locs.shape)
        pl.set_locs(locs)
    elif what == "lik_rows_off":
        pl.set_option(hip.MRA_OPT_LIK_ROWS, 0)
        kw = dict(opts=IN_CASCADE + ((hip.MRA_OPT_LIK_ROWS, 0),))
    else:
        pl.set_option(hip.MRA_OPT_PRIOR_REUSE, 0)
        assert pl.get_option(hip.MRA_OPT_PRIOR_REUSE) == 0
        kw = dict(opts=IN_CASCADE + ((hip.MRA_OPT_PRIOR_REUSE, 0),))
    fresh = _fresh(hip, topo, locs, y, **kw)
    for k in (1, 2) if what == "option_off" else (1,):           # option 24 = 0: every pass computes its prior
        got = _pass(pl)
        _same(got, fresh, what)
        _launched(got, fresh, True, "full", what)
    pl.close()


def test_a_refused_pass_on_the_fused_path_invalidates(hip):
    """Poisson counts in the thousands from x0 = 0 (tests/test_gpu_laplace.py): the fit's second pass is refused MRA_ERR_NOT_SPD.  Its
    first pass left a prior to keep and the kernel is never set again: the next pass computes its prior, and equals a fresh plan."""
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    family, z, aux, offset = LP.edge_inputs("big_counts")
    pl = _plan(hip, topo, locs, y)
    _pass(pl)
    assert pl.route()["path"] == "Fused"
    with pytest.raises(hip.MraError) as ei:
        pl.fit_laplace(family, z, aux, offset, x0=np.zeros(topo.N), max_iter=10)
    assert ei.value.code == -3
    pl.set_obs(y, R)                                             # (y and the scalar noise again; set_obs keeps what stands)
    fresh = _fresh(hip, topo, locs, y)
    got = _pass(pl)
    _same(got, fresh, "after the refused fit")
    _launched(got, fresh, True, "full", "after the refused fit")
    assert _pass(pl)["knots"] == 0
    pl.close()


@pytest.mark.parametrize("pivot", [13, 12])
def test_a_nan_pivot_in_host_blocks_then_good_blocks(hip, pivot):
    """tests/test_gpu_likelihood_masks.py::test_nan_pivot_in_the_last_panel_is_reported on one plan: the refused pass, then the good
    matrix on the same plan equals a fresh plan (a one-node tree: no fused path, no prior launch to count)."""
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    rng = np.random.RandomState(4)
    locs = rng.uniform(size=(14, 2))
    y = rng.normal(size=(14, 1))
    dense = np.asarray(mt.Matern32(locs, locs, l=0.3, sig=1.0))
    np.random.seed(7)
    topo = build_topology(locs, 4, 0, 4)
    bad = dense.copy()
    bad[pivot, pivot] = np.nan

    def run(pl, cov):
        pl.upload_host_cov(np.matrix(cov), locs, y)
        pl.run(True, True)
        return pl.likelihood(), pl.predict()

    fresh = hip.HipPlan(topo, 0)
    fresh.set_locs(locs); fresh.set_obs(y, 1e-2)
    want = run(fresh, dense)
    fresh.close()
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, 1e-2)
    with pytest.raises(hip.MraError) as ei:
        run(pl, bad)
    assert ei.value.code == -3
    got = run(pl, dense)
    assert got[0] == want[0] and np.array_equal(got[1][0], want[1][0]) and np.array_equal(got[1][1], want[1][1])
    pl.close()


# ---- 4. routes whose update rewrites every leaf ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts,update", [(((7, 0), (8, 0)), "Gemm"), (((7, 1),), "SolveHalves")])
def test_all_dirty_routes_keep_the_knots_only(hip, opts, update):
    topo, locs, obs, y = _t96()
    fresh = _fresh(hip, topo, locs, y, opts=opts)
    pl = _plan(hip, topo, locs, y, opts=opts)
    for k, knots in ((1, True), (2, False), (3, False)):
        got = _pass(pl)
        assert pl.route()["update"] == update and pl.route()["solve_fused"] == (update == "SolveHalves")
        _same(got, fresh, "%s pass %d" % (update, k))
        _launched(got, fresh, knots, "full", "%s pass %d" % (update, k))
    pl.close()


# ---- 5. other dimensions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", ["line", "sphere"])
def test_other_dimensions(hip, dim):
    if dim == "line":
        topo, locs, obs, y, counts = LC.problem("L16")
        spec, noise = LC.M32, LC.R
    else:
        ll, locs, topo, y = SP.tree(*SP.TREES["g64"])
        spec, noise = SP.M32, SP.R
    fresh = _fresh(hip, topo, locs, y, spec=spec, noise=noise)
    pl = _plan(hip, topo, locs, y, spec=spec, noise=noise)
    for k in (1, 2, 3):
        got = _pass(pl)
        assert pl.route()["path"] == "Fused"
        _same(got, fresh, "%s pass %d" % (dim, k))
        assert got["knots"] == (fresh["knots"] if k == 1 else 0), (dim, k, got["knots"])
    pl.close()


# ---- 6. the library's own loops, option 24 on against off ---------------------------------------------------------------------------
def _on_off(hip, topo, locs, y, work, opts=()):
    out = []
    for v in (1, 0):
        pl = _plan(hip, topo, locs, y, opts=tuple(opts) + ((hip.MRA_OPT_PRIOR_REUSE, v),))
        out.append(work(pl))
        pl.close()
    return out


def test_fit_laplace_on_against_off(hip):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset = LP.inputs(locs, obs, LP.POISSON)

    def work(pl):
        res = pl.fit_laplace("poisson", z, aux, offset)
        assert pl.route()["path"] == "Fused" and res["converged"]
        return res["info"].copy(), pl.predict()
    (i1, p1), (i0, p0) = _on_off(hip, topo, locs, y, work)
    assert i1[5] == i0[5] and i1[5] > 1                           # the same number of passes
    assert np.array_equal(i1, i0), (i1, i0)
    assert np.array_equal(p1[0], p0[0]) and np.array_equal(p1[1], p0[1])


def test_conditional_sample_on_against_off(hip):
    topo, locs, obs, y = _t96()
    work = lambda pl: (pl.sample(4, seed=3, conditional=True), pl.sample(2, seed=3))      # noqa: E731
    (c1, u1), (c0, u0) = _on_off(hip, topo, locs, y, work, opts=IN_CASCADE)
    assert np.array_equal(c1, c0) and np.array_equal(u1, u0)
    assert np.all(np.isfinite(c1))


def test_solve_and_predict_sites_after_a_kept_pass(hip):
    topo, locs, obs, y = _t96()
    rng = np.random.RandomState(6)
    rows = rng.choice(topo.N, 40, replace=False)
    leaf_of = np.full(topo.N, -1)
    for i in np.nonzero(topo.node_leaf)[0]:
        leaf_of[MK._leaf_callers(topo, i)] = i
    rows = rows[leaf_of[rows] >= 0]
    sites = locs[rows] + 1e-3 * rng.uniform(-1.0, 1.0, size=(len(rows), 2))
    Y = rng.normal(size=(3, topo.P))

    def work(pl):
        a, b = _pass(pl), _pass(pl)
        _same(b, a, "second pass")
        return pl.solve(Y), pl.predict_sites(sites, leaf_of[rows]), _pass(pl)
    (s1, q1, r1), (s0, q0, r0) = _on_off(hip, topo, locs, y, work, opts=IN_CASCADE)
    assert np.array_equal(s1[0], s0[0]) and np.array_equal(s1[1], s0[1], equal_nan=True)
    assert np.array_equal(q1[0], q0[0]) and np.array_equal(q1[1], q0[1])
    _same(r1, r0, "the pass after the retained-factor calls")


# ---- 7. split passes ----------------------------------------------------------------------------------------------------------------
def _two_ranks(hip, p, reuse, rounds=2):
    """world = 2 on one GPU: split + resume ``rounds`` times with the same kernel -> per round and rank (lik terms, mean, var), routes"""
    from pymra_amd.sharding import shard_topology
    plans, out, routes = [], [], []
    try:
        for rk in range(2):
            lt, red = shard_topology(p["topo"], 2, rk)
            pl = _plan(hip, lt, p["locs"], p["y"], spec=p["spec"], noise=p["R"], opts=((hip.MRA_OPT_PRIOR_REUSE, reuse),))
            pl.set_reduce_level(red)
            plans.append(pl)
        for _ in range(rounds):
            bufs = []
            for pl in plans:
                pl.run(True, True, split=True)
                bufs.append(pl.reduce_export())
            tot = np.sum(bufs, axis=0)
            for pl in plans:
                pl.reduce_import(tot)
                pl.resume()
                out.append((pl.likelihood(),) + tuple(pl.predict()))
                routes.append(pl.route())
    finally:
        for pl in plans:
            pl.close()
    return out, routes


def test_split_passes_on_against_off(hip):
    """The smallest case of tests/_sharded_cases.py whose two ranks take the fused path."""
    for cid in ("m1-32-16", "m1-48-32", "m1-64-64", "empty", "fam-m52"):
        p = SH.problem(cid)
        off, routes = _two_ranks(hip, p, 0)
        if all(r["path"] == "Fused" for r in routes):
            break
    else:
        pytest.fail("no case of tests/_sharded_cases.py is fused on two ranks")
    on, _ = _two_ranks(hip, p, 1)
    assert len(on) == len(off) == 4
    for k, (a, b) in enumerate(zip(on, off)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (cid, k)
    for rk in range(2):                                           # the second round equals the first on either rank
        assert on[rk][0] == on[2 + rk][0] and np.array_equal(on[rk][1], on[2 + rk][1]) and np.array_equal(on[rk][2], on[2 + rk][2]), (cid, rk)
