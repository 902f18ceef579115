"""MRA_OPT_RESID_REUSE (option 25): a fused pass keeps the leaves' residual of the last pass on the same prior and mask (GPU only).

V[S,o] = kernel(x_S, x_o) - W_S W_o^T and v(o,o) depend on the kernel, the locations, the knots and the mask - not on y, R or a noise
vector.  On an eligible route (fused path, device covariance, Ut rows gathered, k_chol_tiles) the residual product writes them into a
buffer of the plan's own; k_chol_tiles (which adds the noise to the diagonal as it loads), k_trsm_rows2 and k_leaf_solve_update read
them there and store where they always did.  The next pass on the same prior and mask launches no residual product.  The same kernels
run on the same bits in the same order, so EVERY comparison here is bit for bit (np.array_equal) against a fresh plan that runs only
that pass, and against option 25 = 0.  Launches are counted per family through ``kernel_stats()`` (kernel timing on before the first
pass); RESID is the family of the residual product, whichever of its two forms runs.

The refused pass is the Poisson fit of tests/test_gpu_laplace.py that leaves the doubles in its second pass (MRA_ERR_NOT_SPD), as in
tests/test_gpu_prior_reuse.py."""
import numpy as np
import pytest

import _laplace as LP
import _route_cells as RC
import _sharded_cases as SH
import test_gpu_likelihood_masks as MK
import test_gpu_prior_reuse as PR

pytestmark = pytest.mark.gpu

R = MK.R
RESID = "k_leaf_gemm<COV> leaf residual"
IN_CASCADE = PR.IN_CASCADE
OPT = 25


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    assert plan.MRA_OPT_RESID_REUSE == OPT
    return plan


# ---- plans, passes, launches ---------------------------------------------------------------------------------------------------------
def _plan(hip, topo, locs, y, opts=(), noise=R, spec=None):
    return PR._plan(hip, topo, locs, y, spec=spec, opts=opts, noise=noise)


def _pass(pl, predict=True):
    """one pass -> dict(lik, mean, var, resid: launches of the residual family, launches: {family: launches})"""
    pl.run(True, predict)
    mean, var = pl.predict() if predict else (None, None)
    st = {k["name"]: k["launches"] for k in pl.kernel_stats()}
    resid = [n for name, n in st.items() if name.startswith(RESID)]
    assert len(resid) == 1, sorted(st)
    return dict(lik=pl.likelihood(), mean=mean, var=var, resid=resid[0], launches=st)


def _fresh(hip, topo, locs, y, predict=True, **kw):
    pl = _plan(hip, topo, locs, y, **kw)
    out = _pass(pl, predict)
    pl.close()
    return out


_same = PR._same
OFF = ((OPT, 0),)


def _eligible(pl):
    r = pl.route()
    return r["path"] == "Fused" and r["chol"] in ("TilesOne", "TilesSplit") and not r["scatter_ut"] and (r["c_only"] or r["leaf_resident"])


# ---- 1. three predict passes, leaves on both sides of the 8-tile split ------------------------------------------------------------------
@pytest.mark.parametrize("tree,opts,update,chol", [
    ("T96", (), "SolveHalves", "TilesOne"), ("T96", IN_CASCADE, "InCascade", "TilesOne"), ("T96", ((7, 0), (8, 0)), "Gemm", "TilesOne"),
    ("A", (), "SolveHalves", "TilesSplit"), ("A", IN_CASCADE, "InCascade", "TilesSplit")])
def test_three_predict_passes(hip, tree, opts, update, chol):
    """T96 (96 x 96, r = 32, M = 3): 64 leaves of 144 rows, at most 8 tiles and 9 - both row-solve launches and the leaf fork, one
    k_chol_tiles<10, 4> launch (64 leaves are at most two per CU).  A (tests/_route_cells.py, the cloud mask): every leaf small, the
    k_chol_tiles<8, 4> launch of TilesSplit.  (TilesSplit with leaves on BOTH sides - the second launch reading the kept list from
    n_chol_small on - needs more than two leaves per CU, over 512 leaves: config c3 runs it, and profiles/resid_reuse_bench_ab.txt
    compares its outputs with the in-place build's, array for array.)  Passes 2 and 3 launch nothing in the residual family and equal pass 1, a fresh plan and
    option 25 = 0."""
    if tree == "T96":
        topo, locs, obs, y = PR._t96()
    else:
        topo, locs = MK._tree(*RC.TREES["A"])
        y = MK._y(RC.make_obs(topo, locs, RC.CLOUD))
    fresh = _fresh(hip, topo, locs, y, opts=opts)
    off = _fresh(hip, topo, locs, y, opts=opts + OFF)
    _same(fresh, off, "fresh, on vs off")
    assert fresh["resid"] == off["resid"] == 1
    pl = _plan(hip, topo, locs, y, opts=opts)
    for k in (1, 2, 3):
        got = _pass(pl)
        assert _eligible(pl) and pl.route()["update"] == update and pl.route()["chol"] == chol, pl.route()
        _same(got, fresh, "%s %s pass %d" % (tree, update, k))
        assert got["resid"] == (1 if k == 1 else 0), (tree, update, k, got["resid"])
    pl.close()


# ---- 2. leaf shapes: n_obs not a multiple of 16, an exact multiple, none; scalar R and a noise vector -----------------------------------
def _shapes():
    topo, locs, obs, y = PR._t96()
    rng = np.random.RandomState(11)
    leaves = [int(i) for i in np.nonzero(topo.node_leaf)[0]]
    for pos, count in ((1, 0), (3, 48), (5, 37), (7, 128), (9, 1), (11, 129)):
        MK._exact(obs, topo, leaves[pos], count, rng)
    counts = MK.leaf_counts(topo, obs)
    assert {0, 48, 37, 128, 1, 129, 144} <= set(int(c) for c in counts) and RC.tiles(counts).max() <= 10
    return topo, locs, obs, MK._y(obs, seed=3)


@pytest.mark.parametrize("noise", ["scalar", "vector"])
@pytest.mark.parametrize("opts", [(), IN_CASCADE], ids=["solve_update", "in_cascade"])
def test_leaf_shapes(hip, noise, opts):
    topo, locs, obs, y = _shapes()
    r = R if noise == "scalar" else np.random.RandomState(5).uniform(0.5 * R, 4.0 * R, size=topo.N)
    fresh = {p: _fresh(hip, topo, locs, y, predict=p, opts=opts, noise=r) for p in (True, False)}
    off = {p: _fresh(hip, topo, locs, y, predict=p, opts=opts + OFF, noise=r) for p in (True, False)}
    pl = _plan(hip, topo, locs, y, opts=opts, noise=r)
    for k, pred in enumerate((True, True, False, False, True)):
        got = _pass(pl, pred)
        assert _eligible(pl)
        _same(got, fresh[pred], "%s pass %d" % (noise, k))
        _same(got, off[pred], "%s pass %d vs option off" % (noise, k))
        assert got["resid"] == (0, 1)[k in (0, 2, 4)], (noise, k, got["resid"])      # (a change of product form runs it again)
    pl.close()


# ---- 3. new R, new noise vector, new y on the same mask: kept ---------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [(), IN_CASCADE], ids=["solve_update", "in_cascade"])
def test_new_noise_and_new_y_keep_the_residual(hip, opts):
    topo, locs, obs, y = PR._t96()
    rng = np.random.RandomState(8)
    r1, r2 = (rng.uniform(0.5 * R, 3.0 * R, size=topo.N) for _ in range(2))
    y2 = np.where(obs.reshape(-1, 1), rng.normal(size=(topo.N, 1)), np.nan)
    pl = _plan(hip, topo, locs, y, opts=opts)
    assert _pass(pl)["resid"] == 1
    steps = [("noise vector", lambda p: p.set_noise(r1), y, r1), ("another noise vector", lambda p: p.set_noise(r2), y, r2),
             ("back to the scalar", lambda p: p.set_noise(None), y, R), ("set_obs: new y, new R, same mask", lambda p: p.set_obs(y2, 3.0 * R), y2, 3.0 * R),
             ("set_obs: new y and a noise vector", lambda p: p.set_obs(y, r2), y, r2)]
    for tag, change, yy, rr in steps:
        change(pl)
        got = _pass(pl)
        assert _eligible(pl)
        _same(got, _fresh(hip, topo, locs, yy, opts=opts, noise=rr), tag)
        assert got["resid"] == 0, (tag, got["resid"])
    pl.close()


# ---- 4. new mask, invalidation, refusal: recomputed --------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["new_mask", "set_kernel", "set_locs", "option", "option_25_off_on"])
def test_invalidation(hip, what):
    topo, locs, obs, y = PR._t96()
    s = MK._spec()
    opts = IN_CASCADE
    pl = _plan(hip, topo, locs, y, opts=opts)
    _pass(pl)
    assert _pass(pl)["resid"] == 0                                # the state to invalidate
    if what == "new_mask":
        _, _, obs2, y = PR._t96(seed=4, full_every=3)
        assert not np.array_equal(obs, obs2)
        pl.set_obs(y, R)
    elif what == "set_kernel":
        pl.set_kernel(s.kind, 0.6 * s.l, s.sig, s.scale)
        pl.set_kernel(s.kind, s.l, s.sig, s.scale)
    elif what == "set_locs":
        locs = locs + 1e-4 * np.random.RandomState(2).uniform(-1.0, 1.0, size=locs.shape)
        pl.set_locs(locs)
    elif what == "option":
        pl.set_option(hip.MRA_OPT_PARENT_PAIR, 0)
        opts = opts + ((hip.MRA_OPT_PARENT_PAIR, 0),)
    else:
        pl.set_option(OPT, 0)
        assert pl.get_option(OPT) == 0
        off = _pass(pl)
        _same(off, _fresh(hip, topo, locs, y, opts=opts + OFF), "option 25 off")
        assert off["resid"] == 1 and _pass(pl)["resid"] == 1      # in place: every pass runs its product
        pl.set_option(OPT, 1)
    fresh = _fresh(hip, topo, locs, y, opts=opts)
    got = _pass(pl)
    _same(got, fresh, what)
    assert got["resid"] == 1, (what, got["resid"])
    again = _pass(pl)
    _same(again, fresh, what + ", the pass after")
    assert again["resid"] == 0
    pl.close()


def test_a_refused_pass_invalidates(hip):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    family, z, aux, offset = LP.edge_inputs("big_counts")
    pl = _plan(hip, topo, locs, y)
    _pass(pl)
    kept = _pass(pl)
    if not _eligible(pl):
        pytest.fail("the Laplace tree is not on an eligible route: %r" % (pl.route(),))
    assert kept["resid"] == 0
    with pytest.raises(hip.MraError) as ei:
        pl.fit_laplace(family, z, aux, offset, x0=np.zeros(topo.N), max_iter=10)
    assert ei.value.code == -3
    pl.set_obs(y, R)                                              # (the same mask: set_obs alone would keep)
    fresh = _fresh(hip, topo, locs, y)
    got = _pass(pl)
    _same(got, fresh, "after the refused fit")
    assert got["resid"] == 1
    assert _pass(pl)["resid"] == 0
    pl.close()


# ---- 5. the form rule: the gathered C-only product and k_leaf_gemm never share a C0 ------------------------------------------------------
def test_likelihood_only_and_predict_never_cross_forms(hip):
    topo, locs, obs, y = PR._t96()
    fresh = {p: _fresh(hip, topo, locs, y, predict=p, opts=IN_CASCADE) for p in (True, False)}
    assert fresh[False]["launches"] != fresh[True]["launches"]
    pl = _plan(hip, topo, locs, y, opts=IN_CASCADE)
    for k, (pred, runs) in enumerate(((False, 1), (True, 1), (False, 1), (False, 0), (True, 1), (True, 0), (False, 1))):
        got = _pass(pl, pred)
        assert _eligible(pl) and pl.route()["c_only"] == (not pred)
        _same(got, fresh[pred], "pass %d (predict %s)" % (k, pred))
        assert got["resid"] == runs, (k, pred, got["resid"])
    pl.close()


# ---- 6. ineligible routes: the in-place launch list, launch for launch ----------------------------------------------------------------
def _on_off_passes(hip, make, n=2, predict=True):
    out = []
    for v in (1, 0):
        pl = make(v)
        out.append(([_pass(pl, predict) for _ in range(n)], pl.route()))
        pl.close()
    (on, route), (off, _) = out
    for k, (a, b) in enumerate(zip(on, off)):
        _same(a, b, "pass %d on vs off" % k)
        assert a["launches"] == b["launches"], (k, a["launches"], b["launches"])
    return on, route


@pytest.mark.parametrize("opts,field,value", [(((11, 0),), "chol", "Wave"), (((6, 0),), "leaf_resident", False), (((13, 0),), "scatter_ut", True)])
def test_ineligible_routes_by_option(hip, opts, field, value):
    topo, locs, obs, y = PR._t96()
    on, route = _on_off_passes(hip, lambda v: _plan(hip, topo, locs, y, opts=opts + ((OPT, v),)))
    assert route["path"] == "Fused" and route[field] == value, route
    assert [p["resid"] for p in on] == [1, 1]


def test_ineligible_host_covariance(hip):
    import pymra_amd.MRATools as mt
    topo, locs, obs, y = PR._t96()
    s = MK._spec()
    cov = lambda a, b: np.asarray(mt.Matern32(a, b, l=s.l, sig=s.sig))      # noqa: E731

    def make(v):
        pl = hip.HipPlan(topo, 0)
        pl.set_option(hip.MRA_OPT_KERNEL_TIMING, 1); pl.set_option(OPT, v)
        pl.set_locs(locs); pl.set_obs(y, R); pl.upload_host_cov(cov, locs, y)
        return pl
    on, route = _on_off_passes(hip, make)
    assert route["path"] == "Levels"
    assert [p["resid"] for p in on] == [1, 1]


def test_ineligible_hi_path(hip):
    """The deep 64-wide tree of tests/_route_cells.py with option 11 = 2: k_chol_tiles, but on the Hi path."""
    topo, locs = MK._tree(*RC.TREES["H"])
    y = MK._y(RC.make_obs(topo, locs, RC.CLOUD))
    on, route = _on_off_passes(hip, lambda v: _plan(hip, topo, locs, y, opts=((11, 2), (OPT, v))))
    assert route["path"] == "Hi" and route["chol"] == "TilesSplit", route
    assert [p["resid"] for p in on] == [1, 1]


# ---- 7. the library's own loops, option 25 on against off ---------------------------------------------------------------------------
def _on_off(hip, topo, locs, y, work, opts=()):
    out = []
    for v in (1, 0):
        pl = _plan(hip, topo, locs, y, opts=tuple(opts) + ((OPT, v),))
        out.append(work(pl))
        pl.close()
    return out


def test_fit_laplace_on_against_off(hip):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset = LP.inputs(locs, obs, LP.POISSON)

    def work(pl):
        res = pl.fit_laplace("poisson", z, aux, offset)
        assert pl.route()["path"] == "Fused" and res["converged"]
        st = {k["name"]: k["launches"] for k in pl.kernel_stats()}
        return res["info"].copy(), pl.predict(), [n for name, n in st.items() if name.startswith(RESID)][0], _eligible(pl)
    (i1, p1, n1, e1), (i0, p0, n0, _) = _on_off(hip, topo, locs, y, work)
    assert i1[5] == i0[5] and i1[5] > 1
    assert np.array_equal(i1, i0), (i1, i0)
    assert np.array_equal(p1[0], p0[0]) and np.array_equal(p1[1], p0[1])
    assert n0 == 1 and n1 == (0 if e1 else 1)                    # the last Newton pass kept the first one's residual


@pytest.mark.parametrize("opts", [(), IN_CASCADE], ids=["solve_update", "in_cascade"])
def test_conditional_sample_on_against_off(hip, opts):
    topo, locs, obs, y = PR._t96()
    work = lambda pl: (pl.sample(4, seed=3, conditional=True), pl.sample(2, seed=3))      # noqa: E731
    (c1, u1), (c0, u0) = _on_off(hip, topo, locs, y, work, opts=opts)
    assert np.array_equal(c1, c0) and np.array_equal(u1, u0)
    assert np.all(np.isfinite(c1))


@pytest.mark.parametrize("opts", [(), IN_CASCADE], ids=["solve_update", "in_cascade"])
def test_retained_factor_calls_after_a_kept_pass(hip, opts):
    """solve, predict_sites and sites_cov read the factors a kept pass stored in the panels"""
    topo, locs, obs, y = PR._t96()
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
        assert b["resid"] == pl.get_option(OPT) ^ 1
        return (pl.solve(Y), pl.predict_sites(sites, leaf_of[rows]), pl.sites_cov(sites, leaf_of[rows], posterior=True),
                pl.sites_cov(sites, leaf_of[rows]), _pass(pl))
    (s1, q1, c1, d1, r1), (s0, q0, c0, d0, r0) = _on_off(hip, topo, locs, y, work, opts=opts)
    assert np.array_equal(s1[0], s0[0]) and np.array_equal(s1[1], s0[1], equal_nan=True)
    assert np.array_equal(q1[0], q0[0]) and np.array_equal(q1[1], q0[1])
    assert np.array_equal(np.asarray(c1), np.asarray(c0)) and np.array_equal(np.asarray(d1), np.asarray(d0))
    _same(r1, r0, "the pass after the retained-factor calls")


# ---- 8. two ranks on one GPU, split passes with mra_run_resume ------------------------------------------------------------------------
def _two_ranks(hip, p, reuse, rounds=3):
    from pymra_amd.sharding import shard_topology
    plans, out, routes, resid = [], [], [], []
    try:
        for rk in range(2):
            lt, red = shard_topology(p["topo"], 2, rk)
            pl = _plan(hip, lt, p["locs"], p["y"], spec=p["spec"], noise=p["R"], opts=((OPT, reuse),))
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
                resid.append(sum(k["launches"] for k in pl.kernel_stats() if k["name"].startswith(RESID)))
    finally:
        for pl in plans:
            pl.close()
    return out, routes, resid


def test_split_passes_on_two_ranks_on_against_off(hip):
    """The smallest case of tests/_sharded_cases.py whose two ranks take the fused path."""
    for cid in ("m1-32-16", "m1-48-32", "m1-64-64", "empty", "fam-m52"):
        p = SH.problem(cid)
        off, routes, n_off = _two_ranks(hip, p, 0)
        if all(r["path"] == "Fused" for r in routes):
            break
    else:
        pytest.fail("no case of tests/_sharded_cases.py is fused on two ranks")
    on, routes_on, n_on = _two_ranks(hip, p, 1)
    assert len(on) == len(off) == 6
    for k, (a, b) in enumerate(zip(on, off)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (cid, k)
    assert n_off == [1] * 6
    for k, (r, n) in enumerate(zip(routes_on, n_on)):
        kept = k >= 2 and r["chol"] in ("TilesOne", "TilesSplit") and not r["scatter_ut"] and (r["leaf_resident"] or r["c_only"])
        assert n == (0 if kept else 1), (cid, k, n, r)
