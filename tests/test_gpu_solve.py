"""mra_solve / HipPlan.solve / MRATree.solve on the GPU: factor once, solve many.  Truths: dense Gaussian conditioning on the MRA prior
covariance of the faithful oracle; the plan's own pass per column (set_obs + run + predict); the caller's state before the call.
Tolerances are those the existing tests use for the same quantities (cited at each assertion)."""
import numpy as np
import pytest

import _cases as K
import _sampling as SM

pytestmark = pytest.mark.gpu

CASES = ["g32", "c1", "kat3", "u3"]          # the trees of test_posterior_factor_matches_dense_conditioning
R_MASK = 2e-2


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _plan(plan_mod, topo, locs, y_obs, R, spec, run=True):
    pl = plan_mod.HipPlan(topo, 0)
    pl.set_locs(locs)
    pl.set_obs(y_obs, R)
    pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
    if run:
        pl.run(True, True)
    return pl


def _padded(topo, Y):
    """(N, c) caller order -> (c, P) padded leaf order (phantom rows 0)."""
    Y = np.asarray(Y, float).reshape(topo.N, -1)
    real = topo.perm >= 0
    Yp = np.zeros((Y.shape[1], topo.P))
    Yp[:, real] = np.nan_to_num(Y[topo.perm[real], :].T)
    return Yp


def _caller(topo, m):
    rep = SM.reported(topo)
    out = np.zeros((topo.N, m.shape[0]))
    out[topo.perm[rep], :] = m[:, rep].T
    return out


def _columns(y_obs, c, seed=1):
    y = np.asarray(y_obs, float).ravel()
    Y = np.random.default_rng(seed).standard_normal((len(y), c))
    Y[:, 0] = np.nan_to_num(y)
    return Y


def _gappy_tree(n=64, r=16, M=3, seed=7):
    """A regular tree with an empty leaf, an empty family and a cloud-shaped gap (the patterns of test_gpu_likelihood_masks)."""
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    np.random.seed(seed)
    locs = mt.genLocations2d(Nx=n, Ny=n)
    topo = build_topology(locs, r, M, 4)
    rng = np.random.default_rng(5)
    obs = rng.random(len(locs)) < 0.5
    leaves = [int(i) for i in np.nonzero(topo.node_leaf)[0]]
    fams = {}
    for i in leaves:
        fams.setdefault(int(topo.node_parent[i]), []).append(i)
    for i in [leaves[0]] + fams[sorted(fams)[2]]:
        p = topo.perm[int(topo.node_row0[i]):int(topo.node_row1[i])]
        obs[p[p >= 0]] = False
    u = (locs - locs.min(0)) / (locs.max(0) - locs.min(0))
    obs[(u[:, 0] >= 0.23) & (u[:, 0] <= 0.61) & (u[:, 1] >= 0.37) & (u[:, 1] <= 0.71)] = False
    y_obs = np.where(obs, rng.standard_normal(len(locs)), np.nan)
    return topo, locs, y_obs


def _check_against_own_pass(hip, topo, locs, y_obs, R, spec, Y, mean, quad, cols):
    """Column k of solve against set_obs(Y[:, k]) + run + predict(): mean within 1e-8 of the scale (test_random_geometries'
    predictive-mean tolerance between option paths), d + quad[k, k] against the run's likelihood at 1e-9 relative."""
    obs = np.isfinite(np.asarray(y_obs, float).ravel())
    pl = _plan(hip, topo, locs, y_obs, R, spec, run=False)
    for k in cols:
        pl.set_obs(np.where(obs, Y[:, k], np.nan), R)
        pl.run(True, True)
        d, u = pl.likelihood()
        m, _ = pl.predict()
        scale = max(1.0, np.abs(m).max())
        e_m = np.abs(mean[:, k] - m).max()
        e_l = abs((d + quad[k, k]) - (d + u)) / abs(d + u)
        print("column %d: mean err %.2e (scale %.2f), likelihood rel err %.2e" % (k, e_m, scale, e_l))
        assert e_m <= 1e-8 * scale
        assert e_l <= 1e-9
    pl.close()


# ---- 1. dense conditioning ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_solve_matches_dense_conditioning(hip, name):
    from oracle.mra_faithful import prior_sigma_rows
    cs = K.load_case(name)
    topo, R = cs["topo"], cs["c"]["R"]
    pl = _plan(hip, topo, cs["locs"], cs["y_obs"], R, cs["spec"])
    Y = _columns(cs["y_obs"], 5)
    mean, quad = pl.solve(_padded(topo, Y))
    rep = SM.reported(topo)
    rows = np.nonzero(rep)[0]
    S = prior_sigma_rows(topo, cs["locs"], cs["spec"].evaluate, rows)
    o = np.isfinite(np.asarray(cs["y_obs"], float).ravel())[topo.perm[rows]]
    Yo = Y[topo.perm[rows]][o]
    L = np.linalg.cholesky(S[np.ix_(o, o)] + R * np.eye(int(o.sum())))
    A = np.linalg.solve(L, Yo)
    want_mean = np.linalg.solve(L, S[o, :]).T @ A          # Sigma[:, o] (Sigma_oo + R I)^-1 Y_o
    want_quad = A.T @ A
    tol = 1e-6 if name == "u3" else 1e-9                   # test_posterior_factor_matches_dense_conditioning
    scale = np.abs(S).max()
    e_m = np.abs(mean[:, rows].T - want_mean).max()
    e_q = np.abs(quad - want_quad).max()
    print("%s: mean err %.2e, quad err %.2e, scale %.2f, quad scale %.1f" % (name, e_m, e_q, scale, np.abs(np.diag(want_quad)).max()))
    assert e_m <= tol * max(1.0, np.abs(want_mean).max())               # of the field scale
    assert e_q <= tol * np.abs(np.diag(want_quad)).max()
    assert np.all(mean[:, ~rep] == 0.0)
    pl.close()


# ---- 2. the plan's own pass per column -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 5, 16, 17, 40])
def test_solve_matches_the_plans_own_pass_on_a_gappy_mask(hip, c):
    import pymra_amd.MRATools as mt
    topo, locs, y_obs = _gappy_tree()
    spec = mt.KernelSpec(mt.KIND_MATERN32, 0.25, 1.2)
    pl = _plan(hip, topo, locs, y_obs, R_MASK, spec)
    Y = _columns(y_obs, c, seed=c)
    mp, quad = pl.solve(_padded(topo, Y))
    assert mp.shape == (c, topo.P) and quad.shape == (c, c)
    blk = np.arange(c) // 16
    same = blk[:, None] == blk[None, :]
    assert np.all(np.isfinite(quad[same])) and np.all(np.isnan(quad[~same]))      # block-diagonal, documented in the header
    assert np.abs(quad[same] - quad.T[same]).max() <= 1e-12 * np.abs(np.diag(quad)).max()
    cols = sorted({0, c // 2, c - 1, min(c - 1, 16)})
    _check_against_own_pass(hip, topo, locs, y_obs, R_MASK, spec, Y, _caller(topo, mp), quad, cols)
    pl.close()


@pytest.mark.parametrize("kind", ["KIND_EXP", "KIND_MATERN32", "KIND_MATERN52", "KIND_GAUSSIAN", "KIND_KANTER"])
@pytest.mark.parametrize("tree", [(64, 16, 3), (96, 32, 3)])
def test_solve_in_every_device_kernel_family(hip, kind, tree):
    import pymra_amd.MRATools as mt
    topo, locs, y_obs = _gappy_tree(*tree)
    spec = mt.KernelSpec(getattr(mt, kind), 0.25 if kind != "KIND_GAUSSIAN" else 0.05, 1.2)
    pl = _plan(hip, topo, locs, y_obs, R_MASK, spec)
    Y = _columns(y_obs, 5, seed=11)
    mp, quad = pl.solve(_padded(topo, Y))
    _check_against_own_pass(hip, topo, locs, y_obs, R_MASK, spec, Y, _caller(topo, mp), quad, [0, 4])
    pl.close()


def test_solve_on_a_one_dimensional_tree_and_through_mratree(hip):
    cs = K.load_case("kat3")
    topo, R = cs["topo"], cs["c"]["R"]
    pl = _plan(hip, topo, cs["locs"], cs["y_obs"], R, cs["spec"])
    Y = _columns(cs["y_obs"], 3)
    mp, quad = pl.solve(_padded(topo, Y))
    _check_against_own_pass(hip, topo, cs["locs"], cs["y_obs"], R, cs["spec"], Y, _caller(topo, mp), quad, [0, 1, 2])
    pl.close()
    import pymra_amd.MRATools as mt
    from pymra_amd import MRATree
    np.random.seed(3)
    cov = lambda a, b=np.array([]): mt.Matern32(a, b, l=0.3, sig=1.0)          # noqa: E731
    n = 32
    locs = mt.genLocations2d(Nx=n, Ny=n)
    rng = np.random.default_rng(2)
    y = np.where(rng.random(n * n) < 0.4, rng.standard_normal(n * n), np.nan).reshape(-1, 1)
    tree = MRATree(locs, 16, cov, y, 1e-2, M=2, J=4, verbose=False)
    lik0 = float(tree.getLikelihood()[0, 0])
    m0 = np.asarray(tree.predict()[0]).ravel()
    Yc = _columns(y, 3)
    mean, quad = tree.solve(Yc)
    assert mean.shape == (n * n, 3) and quad.shape == (3, 3)
    assert np.abs(mean[:, 0] - m0).max() <= 1e-8 * max(1.0, np.abs(m0).max())
    liks = tree.getLikelihoods(Yc)
    assert abs(liks[0] - lik0) <= 1e-9 * abs(lik0)
    m1, q1 = tree.solve(Yc[:, 1])
    assert m1.shape == (n * n, 1) and np.abs(m1[:, 0] - mean[:, 1]).max() <= 1e-12 * max(1.0, np.abs(mean).max())
    assert float(tree.getLikelihood()[0, 0]) == lik0 and np.array_equal(np.asarray(tree.predict()[0]).ravel(), m0)


# ---- full size ---------------------------------------------------------------------------------------------------------------------
def _fullsize(hip, name, ncol):
    import bench
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    c = bench.CONFIGS[name]
    locs, y_obs = bench.make_inputs(c)
    topo = build_topology(locs, c["r"], c["M"], c["J"])
    spec = mt.KernelSpec(mt.KIND_MATERN32, c["l"], c["sig"])
    pl = _plan(hip, topo, locs, y_obs, c["R"], spec, run=False)
    Y = _columns(y_obs, ncol, seed=9)
    mp, quad = pl.solve(_padded(topo, Y))
    mean = _caller(topo, mp)
    obs = np.isfinite(np.asarray(y_obs, float).ravel())
    for k in range(ncol):
        pl.set_obs(np.where(obs, Y[:, k], np.nan).reshape(-1, 1), c["R"])
        pl.run(True, True)
        d, u = pl.likelihood()
        m, _ = pl.predict()
        e_m, e_l = np.abs(mean[:, k] - m).max(), abs(quad[k, k] - u) / abs(d + u)
        print("%s column %d: mean err %.2e (scale %.2f), likelihood rel err %.2e" % (name, k, e_m, np.abs(m).max(), e_l))
        assert e_m <= 1e-8 * max(1.0, np.abs(m).max())
        assert e_l <= 1e-9
    pl.close()


def test_solve_three_columns_at_c3(hip):
    _fullsize(hip, "c3", 3)


def test_solve_two_columns_at_c5(hip):
    _fullsize(hip, "c5", 2)


# ---- 3. state ----------------------------------------------------------------------------------------------------------------------
def _factor_launches(pl):
    return sum(s["launches"] for s in pl.kernel_stats())


def test_solve_leaves_the_callers_state_and_keeps_the_factors(hip):
    import pymra_amd.MRATools as mt
    topo, locs, y_obs = _gappy_tree()
    spec = mt.KernelSpec(mt.KIND_MATERN32, 0.25, 1.2)
    pl = _plan(hip, topo, locs, y_obs, R_MASK, spec)
    opts = {k: pl.get_option(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20)}
    lik0, (m0, v0) = pl.likelihood(), pl.predict()
    Y = _columns(y_obs, 5, seed=4)
    Yp = _padded(topo, Y)
    mean1, quad1 = pl.solve(Yp)
    assert _factor_launches(pl) > 0                                     # the first solve ran its own likelihood pass
    assert pl.likelihood() == lik0
    m1, v1 = pl.predict()
    assert np.array_equal(m1, m0) and np.array_equal(v1, v0)
    assert {k: pl.get_option(k) for k in opts} == opts
    mean2, quad2 = pl.solve(Yp)
    assert _factor_launches(pl) == 0                                    # the second one launched no kernel of a pass
    assert np.array_equal(mean1, mean2) and np.array_equal(quad1, quad2)
    pl.run(True, True)                                                  # y untouched: the old numbers bit for bit
    assert pl.likelihood() == lik0
    m2, v2 = pl.predict()
    assert np.array_equal(m2, m0) and np.array_equal(v2, v0)
    # run, set_obs, set_kernel and sample clear the mark; the next solve factorises again and is still right
    for what in ("run", "set_obs", "set_kernel", "sample"):
        if what == "set_obs":
            pl.set_obs(y_obs, R_MASK)
        elif what == "set_kernel":
            pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
        elif what == "sample":
            pl.sample(2, seed=1, conditional=True)
        else:
            pl.run(True, False)
        mean3, quad3 = pl.solve(Yp)
        assert _factor_launches(pl) > 0, what
        assert np.abs(mean3 - mean1).max() <= 1e-12 * max(1.0, np.abs(mean1).max()), what
        assert np.abs(quad3 - quad1).max() <= 1e-12 * np.abs(np.diag(quad1)).max(), what
    # a new mask: the descriptors are rebuilt
    y2 = np.where(np.random.default_rng(8).random(len(locs)) < 0.3, 1.0, np.nan)
    pl.set_obs(y2, R_MASK)
    Y2 = _columns(y2, 2, seed=6)
    mp, quad = pl.solve(_padded(topo, Y2))
    _check_against_own_pass(hip, topo, locs, y2, R_MASK, spec, Y2, _caller(topo, mp), quad, [0, 1])
    assert pl.solve(np.zeros((0, topo.P)))[1].shape == (0, 0)
    pl.close()


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------
def test_solve_refusals(hip):
    from pymra_amd.plan import MraError
    import pymra_amd.MRATools as mt
    topo, locs, y_obs = _gappy_tree()
    spec = mt.KernelSpec(mt.KIND_MATERN32, 0.25, 1.2)
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs)
    pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
    with pytest.raises(MraError) as e:
        pl.solve(np.zeros((1, topo.P)))
    assert e.value.code == -4                            # before set_obs
    pl.set_obs(y_obs, R_MASK)
    Yp = _padded(topo, _columns(y_obs, 2))
    bad = Yp.copy()
    row = int(np.nonzero(np.isfinite(np.asarray(y_obs).ravel())[topo.src] & (topo.perm >= 0))[0][3])
    bad[1, row] = np.nan
    with pytest.raises(MraError) as e:
        pl.solve(bad)
    assert e.value.code == -1
    unobs = Yp.copy()
    unobs[:, ~(np.isfinite(np.asarray(y_obs).ravel())[topo.src] & (topo.perm >= 0))] = np.nan     # ignored where nothing is observed
    assert np.array_equal(pl.solve(unobs)[0], pl.solve(Yp)[0])
    pl.set_reduce_level(0)
    with pytest.raises(MraError) as e:
        pl.solve(Yp)
    assert e.value.code == -1                          # sharded
    pl.close()
    from pymra_amd import MRATree
    np.random.seed(1)
    n = 16
    l2 = mt.genLocations2d(Nx=n, Ny=n)
    y = np.random.normal(size=(n * n, 1))
    tree = MRATree(l2, 16, lambda a, b=np.array([]): np.exp(-np.abs(mt.dist(a, b)) / 0.3), y, 1e-2, M=1, J=4, verbose=False)      # opaque callable: host cov
    with pytest.raises(NotImplementedError):
        tree.solve(y)
    with pytest.raises(MraError) as e:
        tree.plan.solve(np.zeros((1, tree.topology.P)))
    assert e.value.code == -1


# ---- 5. the sampler on the solve path ------------------------------------------------------------------------------------------------
def test_conditional_draws_through_the_solver(hip):
    import pymra_amd.MRATools as mt
    from pymra_amd.plan import MRA_OPT_SAMPLE_SOLVE
    topo, locs, y_obs = _gappy_tree()
    spec = mt.KernelSpec(mt.KIND_MATERN32, 0.25, 1.2)
    pl = _plan(hip, topo, locs, y_obs, R_MASK, spec)
    assert pl.get_option(MRA_OPT_SAMPLE_SOLVE) == 0
    z = np.random.default_rng(3).standard_normal((19, pl.sample_slots()))
    off_c, off_p = pl.sample(19, z=z, conditional=True), pl.sample(19, z=z)
    lik0 = pl.likelihood()
    pl.set_option(MRA_OPT_SAMPLE_SOLVE, 1)
    assert pl.get_option(MRA_OPT_SAMPLE_SOLVE) == 1
    on_c, on_p = pl.sample(19, z=z, conditional=True), pl.sample(19, z=z)
    assert np.array_equal(on_p, off_p)                                  # prior draws do not go through the solver
    scale = max(1.0, np.abs(off_c).max())
    print("conditional draws, option on against off: %.2e (scale %.2f)" % (np.abs(on_c - off_c).max(), scale))
    assert np.abs(on_c - off_c).max() <= 1e-8 * scale                   # test_draws_do_not_depend_on_options
    seeded_on = pl.sample(5, seed=77, conditional=True)
    pl.set_option(MRA_OPT_SAMPLE_SOLVE, 0)
    assert np.abs(seeded_on - pl.sample(5, seed=77, conditional=True)).max() <= 1e-8 * scale
    assert pl.likelihood() == lik0
    pl.close()
