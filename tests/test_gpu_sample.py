"""mra_sample / HipPlan.sample / MRATree.simulate on the GPU.  Exactness is checked against truths that do not come from the device:
the MRA prior covariance Sigma = sum_j B_j k_j B_j^T assembled from the reference's own per-node blocks (tests/golden/*_nodes.npz),
dense Gaussian conditioning of Sigma on the case's observations, the NumPy restatement of the latent draws (_philox), and - within
one leaf of a full-size tree, where the MRA is exact - the covariance kernel itself."""
import numpy as np
import pytest

import _cases as K
import _philox
import _sampling as SM

pytestmark = pytest.mark.gpu

CASES = ["g32", "c1", "kat3", "u3"]


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _plan(plan_mod, cs):
    pl = plan_mod.HipPlan(cs["topo"], 0)
    pl.set_locs(cs["locs"])
    pl.set_obs(cs["y_obs"], cs["c"]["R"])
    s = cs["spec"]
    pl.set_kernel(s.kind, s.l, s.sig, s.scale)
    pl.run(True, True)
    return pl


def _reported(topo):
    return SM.reported(topo)


def _prior_sigma(cs):
    """Sigma over the padded rows from the reference's per-node B and kC (k = kC kC^T)."""
    return SM.golden_prior_sigma(cs["_name"], cs["topo"])


def _factor(pl, conditional=False, chunk=256):
    """G with sample(z = e_k) = G[:, k] (prior); for conditional: G_c[:, k] = sample(e_k) - sample(0), and sample(0)."""
    return SM.factor_columns(pl, np.arange(pl.sample_slots()), conditional=conditional, chunk=chunk)


def _load(name):
    cs = K.load_case(name)
    cs["_name"] = name
    return cs


@pytest.mark.parametrize("name", CASES)
def test_prior_factor_matches_reference_sigma(hip, name):
    cs = _load(name)
    pl = _plan(hip, cs)
    G, _ = _factor(pl)
    rep = _reported(cs["topo"])
    S = _prior_sigma(cs)
    GG = G @ G.T
    scale = np.abs(S[np.ix_(rep, rep)]).max()
    assert np.abs(GG[np.ix_(rep, rep)] - S[np.ix_(rep, rep)]).max() <= 1e-10 * scale
    assert np.all(G[~rep] == 0.0)


@pytest.mark.parametrize("name", CASES)
def test_posterior_factor_matches_dense_conditioning(hip, name):
    cs = _load(name)
    pl = _plan(hip, cs)
    topo = cs["topo"]
    rep = _reported(topo)
    Gc, x0 = _factor(pl, conditional=True)
    S = _prior_sigma(cs)
    y = np.full(topo.P, np.nan)
    y[topo.perm >= 0] = np.asarray(cs["y_obs"], dtype=float).ravel()[topo.perm[topo.perm >= 0]]
    o = np.isfinite(y) & rep
    R = cs["c"]["R"]
    L = np.linalg.cholesky(S[np.ix_(o, o)] + R * np.eye(int(o.sum())))
    T = np.linalg.solve(L, S[o, :])
    Spost = S - T.T @ T
    scale = np.abs(S[np.ix_(rep, rep)]).max()
    tol = 1e-6 if name == "u3" else 1e-9
    assert np.abs((Gc @ Gc.T)[np.ix_(rep, rep)] - Spost[np.ix_(rep, rep)]).max() <= tol * scale
    assert np.all(Gc[~rep] == 0.0) and np.all(x0[~rep] == 0.0)
    # z = 0: the conditional draw is the plan's own predictive mean
    mean, _ = pl.predict()
    xc = np.zeros(topo.N)
    xc[topo.perm[rep]] = x0[rep]
    assert np.max(np.abs(xc - mean)) <= 1e-12 * max(1.0, np.abs(mean).max())


def test_seeded_draws(hip):
    cs = _load("g32")
    pl = _plan(hip, cs)
    topo = cs["topo"]
    rep = _reported(topo)
    n = pl.sample_slots()
    G, _ = _factor(pl)
    seed = 0x1234_5678_9ABC_DEF0
    x = pl.sample(8, seed=seed)
    zh = _philox.latent_draws(seed, np.arange(n), np.arange(8))
    assert np.max(np.abs(x - zh @ G.T)) <= 1e-12 * max(1.0, np.abs(x).max())
    assert np.array_equal(x, pl.sample(8, seed=seed))
    assert np.array_equal(x, np.vstack([pl.sample(3, seed=seed), pl.sample(5, seed=seed, sample0=3)]))
    assert not np.array_equal(x, pl.sample(8, seed=seed + 1))
    # moments: 2048 prior draws, 512 posterior draws, 6 standard errors
    S = _prior_sigma(cs)
    xs = pl.sample(2048, seed=11)[:, rep]
    v = np.diag(S)[rep]
    assert np.all(np.abs((xs ** 2).mean(0) - v) <= 6 * np.sqrt(2.0 / 2048) * v)
    mean, var = pl.predict()
    mp = np.zeros(topo.P)
    vp = np.zeros(topo.P)
    mp[rep], vp[rep] = mean[topo.perm[rep]], var[topo.perm[rep]]
    xc = pl.sample(512, seed=12, conditional=True)[:, rep]
    m, vv = mp[rep], vp[rep]
    assert np.all(np.abs(xc.mean(0) - m) <= 6 * np.sqrt(vv / 512))
    assert np.all(np.abs(((xc - m) ** 2).mean(0) - vv) <= 6 * np.sqrt(2.0 / 512) * vv)


def test_state_after_simulate(hip):
    import pymra_amd
    import pymra_amd.MRATools as mt
    from pymra_amd.plan import MraError
    cs = _load("g32")
    c = cs["c"]
    cov = lambda a, b: mt.ExpCovFun(a, b, l=c["l"])
    import make_golden as mg
    mg.make_inputs(c)
    tree = pymra_amd.MRATree(cs["locs"], c["r"], cov, cs["y_obs"], c["R"], M=c["M"], J=c["J"])
    lik0 = float(tree.getLikelihood()[0, 0])
    mean0, sd0 = (np.array(a) for a in tree.predict())
    d0, u0 = tree.plan.likelihood()
    pm0, pv0 = tree.plan.predict()
    opts = {k: tree.plan.get_option(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19)}
    np.random.seed(5)
    a = tree.simulate(3, "posterior")
    np.random.seed(5)
    b = tree.simulate(3, "posterior")
    assert a.shape == (len(cs["locs"]), 3) and np.array_equal(a, b)
    p = tree.simulate(2, "prior", seed=3)
    assert p.shape == (len(cs["locs"]), 2) and np.all(np.isfinite(p))
    assert float(tree.getLikelihood()[0, 0]) == lik0
    assert np.array_equal(np.array(tree.predict()[0]), mean0) and np.array_equal(tree.predict()[1], sd0)
    try:
        assert tree.plan.likelihood() == (d0, u0)
    except MraError as e:
        assert e.code == -4
    try:
        pm, pv = tree.plan.predict()
        assert np.array_equal(pm, pm0) and np.array_equal(pv, pv0)
    except MraError as e:
        assert e.code == -4
    assert {k: tree.plan.get_option(k) for k in opts} == opts
    # the plan still runs the caller's data
    tree.plan.run(True, True)
    assert tree.plan.likelihood() == (d0, u0)
    with pytest.raises(ValueError):
        tree.simulate(1, "sideways")
    opaque = lambda a, b: np.asarray(cs["spec"].evaluate(a, b)) + 0.0
    mg.make_inputs(c)
    t1 = pymra_amd.MRATree(cs["locs"], c["r"], opaque, cs["y_obs"], c["R"], M=c["M"], J=c["J"])
    with pytest.raises(NotImplementedError):
        t1.simulate(1)
    with pytest.raises(MraError) as ei:
        t1.plan.sample(1)
    assert ei.value.code == -1
    assert tree.plan.lib.mra_sample(tree.plan._h, 0, -1, 0, 0, None, None) == -1          # n_samples < 0


def test_fullsize_leaf_blocks_are_exact(hip):
    """256 x 256 Matern32 grid, M = 4, r0 = 16: within a leaf the MRA is exact, so the leaf's chain + knot slots alone give
    G_j with G_j G_j^T = C(S_j, S_j) on the leaf's real rows."""
    import pymra_amd
    import pymra_amd.MRATools as mt
    np.random.seed(3)
    n = 256
    locs = mt.genLocations2d(Nx=n, Ny=n)
    y = np.random.normal(size=(n * n, 1))
    y[np.random.rand(n * n) < 0.6] = np.nan
    spec = mt.KernelSpec(mt.KIND_MATERN32, 0.1, 1.0)
    tree = pymra_amd.MRATree(locs, 16, lambda a, b: mt.Matern32(a, b, l=0.1, sig=1.0), y, 0.05, M=4, J=4)
    topo, pl = tree.topology, tree.plan
    leaves = np.where(np.asarray(topo.node_leaf, dtype=bool))[0]
    for j in (leaves[0], leaves[len(leaves) // 2], leaves[-1]):
        X, _ = SM.factor_columns(pl, SM.chain_slots(topo, j), chunk=1 << 30)
        X = X.T
        rows = K.node_real_rows(topo, j)
        Gj = X[:, rows].T
        Cj = np.asarray(spec.evaluate(locs[topo.perm[rows]], locs[topo.perm[rows]]))
        assert np.abs(Gj @ Gj.T - Cj).max() <= 1e-9


def test_c3_geometry(hip):
    import make_golden as mg
    from pymra_amd.topology import build_topology
    import pymra_amd.MRATools as mt
    c = mg.CASES["c3"]
    locs, y_obs, _ = mg.make_inputs(c)
    topo = build_topology(locs, c["r"], c["M"], c["J"])
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs)
    pl.set_obs(y_obs, c["R"])
    pl.set_kernel(mt.KIND_MATERN32, c["l"], c["sig"], 1.0)
    pl.run(True, True)
    lik = sum(pl.likelihood())
    mean, _ = pl.predict()
    x = pl.sample(16, seed=1)
    assert np.all(np.isfinite(x))
    xc = pl.sample(2, seed=2, conditional=True)
    assert np.all(np.isfinite(xc))
    rep = _reported(topo)
    x0 = pl.sample(1, z=np.zeros((1, pl.sample_slots())), conditional=True)[0]
    xm = np.zeros(topo.N)
    xm[topo.perm[rep]] = x0[rep]
    assert np.max(np.abs(xm - mean)) <= 1e-12 * max(1.0, np.abs(mean).max())
    pl.run(True, True)
    assert abs(sum(pl.likelihood()) - lik) <= 1e-12 * abs(lik)


# ---- exactness where the toy trees above do not reach ----------------------------------------------------------------------------
def _grid(nx, ny, r, M, seed=7, jitter=0.0, frac=0.4):
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    rng = np.random.RandomState(100 + seed)
    np.random.seed(seed)                       # the knot draws of the tree replay use the global RNG
    locs = mt.genLocations2d(Nx=nx, Ny=ny)
    if jitter:
        locs = locs + rng.uniform(-jitter, jitter, size=locs.shape) / max(nx, ny)
    topo = build_topology(locs, r, M, 4)
    y = rng.normal(size=(len(locs), 1))
    y_obs = np.where(rng.uniform(size=(len(locs), 1)) < frac, y, np.nan)
    return topo, locs, y_obs


def _spec_plan(hip, topo, locs, y_obs, spec, R=2e-2):
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs)
    pl.set_obs(y_obs, R)
    pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale, spec.circular)
    pl.run(True, True)
    return pl


def _mid_tree(name):
    """(topo, locs, y_obs, spec, R) of the mid-size trees: cw 32 and 64, a chain of three, r0 with phantom knot columns, 1-D."""
    import pymra_amd.MRATools as mt
    m32 = mt.KernelSpec(mt.KIND_MATERN32, 0.2, 1.1)
    if name == "grid64_r32":
        return _grid(64, 64, 32, 2) + (m32, 2e-2)
    if name == "jitter_r64":
        return _grid(48, 72, 64, 2, seed=3, jitter=0.3) + (mt.KernelSpec(mt.KIND_MATERN52, 0.25, 0.8), 5e-2)
    if name == "grid40_r5":
        return _grid(40, 40, 5, 3, seed=5) + (mt.KernelSpec(mt.KIND_EXP, 0.3), 1e-2)
    if name == "grid48_r20":
        return _grid(48, 48, 20, 2, seed=9, frac=0.7) + (m32, 1e-2)
    cs = _load(name)                                                       # golden trees: g64m (M = 3), t1000 (1-D, dropped rows)
    return cs["topo"], cs["locs"], cs["y_obs"], cs["spec"], cs["c"]["R"]


def _check_prior_factor(pl, topo, locs, spec):
    """Unit-z factor over the prior slots against the faithful oracle's Sigma; inert slots and unreported rows exactly 0."""
    from oracle.mra_faithful import prior_sigma_rows
    zoff, Kn = SM.coarse_offsets(topo)
    G, _ = SM.factor_columns(pl, np.arange(Kn + topo.P), chunk=256)
    rep = SM.reported(topo)
    rr = np.nonzero(rep)[0]
    S = prior_sigma_rows(topo, locs, spec.evaluate, rr)
    scale = np.abs(S).max()
    assert np.abs(G[rr] @ G[rr].T - S).max() <= 1e-10 * scale
    assert np.all(G[~rep] == 0.0)
    inert = [zoff[i] + k for i in zoff
             for k in range(int(topo.knot_ptr[i + 1] - topo.knot_ptr[i]), int(topo.cw[topo.node_level[i]]))]      # phantom knot columns
    leaf_knot = np.zeros(topo.P, dtype=bool)
    for j in np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]:
        leaf_knot[topo.knot_rows[topo.knot_ptr[j]:topo.knot_ptr[j + 1]]] = True
    inert += [Kn + int(r) for r in np.nonzero(~leaf_knot)[0]]                                                     # unread leaf slots
    assert np.all(G[:, inert] == 0.0)
    return len(inert) - int((~leaf_knot).sum())


@pytest.mark.parametrize("name", ["grid64_r32", "jitter_r64", "g64m", "grid40_r5", "grid48_r20", "t1000"])
def test_prior_factor_on_mid_trees(hip, name):
    """cw 32 / 64 (the coarse kernel's k0 loop runs 2 / 4 times per ancestor), a chain of three ancestors (g64m), r0 = 5 / 20 (phantom
    knot columns must stay inert), and a 1-D tree with dropped rows and leaves of mixed sizes in one Gram launch."""
    topo, locs, y_obs, spec, R = _mid_tree(name)
    assert topo.P <= 4608
    pl = _spec_plan(hip, topo, locs, y_obs, spec, R)
    n_phantom = _check_prior_factor(pl, topo, locs, spec)
    if name in ("grid40_r5", "grid48_r20"):
        assert n_phantom > 0
    if name == "jitter_r64":
        assert max(int(c) for c in topo.cw) == 64


def _families_specs():
    import pymra_amd.MRATools as mt
    return {"matern52": mt.KernelSpec(mt.KIND_MATERN52, 0.2, 0.7), "gaussian": mt.KernelSpec(mt.KIND_GAUSSIAN, 0.05, 1.0),
            "kanter": mt.KernelSpec(mt.KIND_KANTER, 0.35), "iden": mt.KernelSpec(mt.KIND_IDEN, 0.01),
            "matern32_scale": mt.KernelSpec(mt.KIND_MATERN32, 0.4, 1.0, 2.5)}


@pytest.mark.parametrize("family", ["matern52", "gaussian", "kanter", "iden", "matern32_scale", "circular"])
def test_prior_factor_every_kernel_family(hip, family):
    """The leaf Gram reuses the residual GEMM's COV epilogue: every device kernel family (g32), and the circular 1-D distance (c1)."""
    import pymra_amd.MRATools as mt
    cs = _load("c1" if family == "circular" else "g32")
    spec = mt.KernelSpec(mt.KIND_EXP, 0.3, 1.0, 1.0, True) if family == "circular" else _families_specs()[family]
    pl = _spec_plan(hip, cs["topo"], cs["locs"], cs["y_obs"], spec, cs["c"]["R"])
    _check_prior_factor(pl, cs["topo"], cs["locs"], spec)


def _single_leaf_tree(name):
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    if name != "grid18_m0":
        cs = _load(name)
        return cs["topo"], cs["locs"], cs["y_obs"], cs["spec"], cs["c"]["R"]
    rng = np.random.RandomState(18)
    locs = mt.genLocations2d(Nx=18, Ny=18)
    topo = build_topology(locs, 16, 0, 4)
    y = rng.normal(size=(len(locs), 1))
    return topo, locs, np.where(rng.uniform(size=(len(locs), 1)) < 0.5, y, np.nan), mt.KernelSpec(mt.KIND_MATERN32, 0.3, 1.0), 2e-2


@pytest.mark.parametrize("name", ["kat1", "kat4", "grid18_m0"])
def test_single_leaf_trees_are_exact_kriging(hip, name):
    """M = 0: no coarse slot, one leaf Gram with K = 0 ancestor columns - the MRA is the GP itself.  The prior factor reproduces
    C(S, S), the conditional factor dense GP conditioning, and the z = 0 conditional draw kriging()'s mean."""
    topo, locs, y_obs, spec, R = _single_leaf_tree(name)
    assert topo.n_nodes == 1
    pl = _spec_plan(hip, topo, locs, y_obs, spec, R)
    _, Kn = SM.coarse_offsets(topo)
    assert Kn == 0
    rep = SM.reported(topo)
    rr = np.nonzero(rep)[0]
    C = np.asarray(spec.evaluate(locs[topo.perm[rr]], locs[topo.perm[rr]]))
    G, _ = SM.factor_columns(pl, np.arange(topo.P), chunk=256)
    assert np.all(G[~rep] == 0.0)
    assert np.abs(G[rr] @ G[rr].T - C).max() <= 1e-10 * np.abs(C).max()
    Gc, x0 = SM.factor_columns(pl, np.arange(2 * topo.P), conditional=True, chunk=256)
    y = np.asarray(y_obs, dtype=float).ravel()[topo.perm[rr]]
    o = np.isfinite(y)
    L = np.linalg.cholesky(C[np.ix_(o, o)] + R * np.eye(int(o.sum())))
    T = np.linalg.solve(L, C[o, :])
    assert np.abs(Gc[rr] @ Gc[rr].T - (C - T.T @ T)).max() <= 1e-9 * np.abs(C).max()
    _, mean, _ = K.kriging(locs, y_obs, spec, R)
    assert np.abs(x0[rr] - mean[topo.perm[rr]]).max() <= 1e-10 * max(1.0, np.abs(mean).max())


def _leaf_sets(topo):
    """Leaves whose lowest common ancestors differ: two siblings, a cousin (same grandparent), the middle leaf and the last."""
    leaves = np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]
    par = np.asarray(topo.node_parent)
    sib = [j for j in leaves[1:] if par[j] == par[leaves[0]]][0]
    cousin = [j for j in leaves if par[j] != par[leaves[0]] and par[par[j]] == par[par[leaves[0]]]][0]
    return [int(j) for j in (leaves[0], sib, cousin, leaves[len(leaves) // 2], leaves[-1])]


def _check_lineages(pl, topo, locs, spec, leaves, seeded=True):
    """G[rows, chain slots] of the given leaves (unit z on the union of their chains) against the oracle's Sigma[rows, rows]; a slot
    outside a row's chain gives exactly 0 there; seeded draws at the rows equal G @ _philox, across a carry of the sample counter."""
    from oracle.mra_faithful import prior_sigma_rows
    zoff, Kn = SM.coarse_offsets(topo)
    rows = [K.node_real_rows(topo, j) for j in leaves]
    chains = [SM.chain_slots(topo, j, zoff, Kn) for j in leaves]
    slots = np.array(sorted(set().union(*chains)))
    allr = np.concatenate(rows)
    G, _ = SM.factor_columns(pl, slots, rows=allr, chunk=16)
    S = prior_sigma_rows(topo, locs, spec.evaluate, allr)
    assert np.abs(G @ G.T - S).max() <= 1e-10 * np.abs(S).max()
    a = 0
    for r, ch in zip(rows, chains):
        outside = ~np.isin(slots, ch)
        assert outside.any() and np.all(G[a:a + len(r), outside] == 0.0)
        a += len(r)
    if seeded:
        seed, s0, n = 0xFEDC_BA98_0000_0011, 2 ** 32 - 5, 11
        x = pl.sample(n, seed=seed, sample0=s0)[:, allr]
        ref = _philox.latent_draws(seed, slots, s0 + np.arange(n)) @ G.T
        assert np.abs(x - ref).max() <= 1e-12 * np.abs(ref).max()


def test_lineages_of_the_deep_wide_tree(hip):
    """256^2, r = 64, M = 5 (the tree of test_deep_wide_tree_leaf_update_inside_predict_hi): chains of five 64-wide ancestors."""
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    n = 256
    np.random.seed(29)
    locs = mt.genLocations2d(Nx=n, Ny=n)
    y = np.random.normal(size=(n * n, 1))
    y_obs = np.where(np.random.uniform(size=(n * n, 1)) < 0.2, y, np.nan)
    topo = build_topology(locs, 64, 5, 4)
    spec = mt.KernelSpec(mt.KIND_MATERN32, 0.25, 1.2)
    pl = _spec_plan(hip, topo, locs, y_obs, spec)
    _check_lineages(pl, topo, locs, spec, _leaf_sets(topo))


def test_lineages_of_c3(hip):
    """BASELINE config 3 (1024^2, M = 6): two Gram batches, factors rebuilt for every sample block."""
    import make_golden as mg
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    c = mg.CASES["c3"]
    locs, y_obs, _ = mg.make_inputs(c)
    topo = build_topology(locs, c["r"], c["M"], c["J"])
    spec = mt.KernelSpec(mt.KIND_MATERN32, c["l"], c["sig"])
    pl = _spec_plan(hip, topo, locs, y_obs, spec, c["R"])
    _check_lineages(pl, topo, locs, spec, _leaf_sets(topo))


def test_seeded_draws_on_a_whole_tree_across_the_counter_carry(hip):
    cs = _load("g32")
    pl = _plan(hip, cs)
    n = pl.sample_slots()
    G, _ = _factor(pl)
    seed, s0 = 0xFEDC_BA98_7654_3210, 2 ** 32 - 5
    x = pl.sample(11, seed=seed, sample0=s0)
    ref = _philox.latent_draws(seed, np.arange(n), s0 + np.arange(11)) @ G.T
    assert np.abs(x - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(x[5:], pl.sample(6, seed=seed, sample0=2 ** 32))         # samples 2^32 .. : the high counter word is 1


# ---- options ------------------------------------------------------------------------------------------------------------------------
OPTION_VALUES = {2: (0, 1), 3: (0, 1), 4: (0, 1), 5: (0, 1), 6: (0, 1, 2), 7: (0, 1, 2), 8: (0, 1), 10: (1, 2), 11: (0, 1, 2),
                 12: (0, 1), 13: (0, 1), 14: (0, 1, 2), 15: (0, 1), 16: (0, 1, 2), 17: (0, 1), 18: (0, 1)}


def _deep_wide(frac=0.2):
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    np.random.seed(29)
    locs = mt.genLocations2d(Nx=256, Ny=256)
    y = np.random.normal(size=(256 * 256, 1))
    y_obs = np.where(np.random.uniform(size=(256 * 256, 1)) < frac, y, np.nan)
    return build_topology(locs, 64, 5, 4), locs, y_obs, mt.KernelSpec(mt.KIND_MATERN32, 0.25, 1.2), 2e-2


@pytest.mark.parametrize("tree", ["grid64_r32", "deep_wide"])
def test_draws_do_not_depend_on_options(hip, tree):
    """The prior pass and every conditional pass go through run_all under the caller's options: each option at each documented value,
    one at a time.  Prior draws within 1e-11 of the field scale of the default's, conditional draws within the predictive-mean
    tolerance the option tests allow (1e-8, test_random_geometries); the options read back unchanged."""
    topo, locs, y_obs, spec, R = _deep_wide() if tree == "deep_wide" else _mid_tree(tree)
    pl = _spec_plan(hip, topo, locs, y_obs, spec, R)
    x0 = pl.sample(4, seed=21)
    c0 = pl.sample(2, seed=22, conditional=True)
    scale = np.abs(x0).max()
    default = {k: pl.get_option(k) for k in OPTION_VALUES}
    for opt, values in OPTION_VALUES.items():
        for v in values:
            pl.set_option(opt, v)
            want = {**default, opt: pl.get_option(opt)}
            x = pl.sample(4, seed=21)
            c = pl.sample(2, seed=22, conditional=True)
            assert {k: pl.get_option(k) for k in OPTION_VALUES} == want, (opt, v)
            assert np.abs(x - x0).max() <= 1e-11 * scale, (opt, v)
            assert np.abs(c - c0).max() <= 1e-8 * scale, (opt, v)
        pl.set_option(opt, default[opt])
    assert {k: pl.get_option(k) for k in OPTION_VALUES} == default


# ---- conditional draws on gappy masks ------------------------------------------------------------------------------------------------
def _masked_tree(n, r, M, pattern):
    import test_gpu_likelihood_masks as LM
    topo, locs = LM._tree(n, r, M)
    if pattern == "full_leaves":                     # every other leaf fully observed, the rest thinned
        obs = np.random.RandomState(0).uniform(size=topo.N) < 0.4
        for k, i in enumerate(np.nonzero(topo.node_leaf)[0]):
            if k % 2 == 0:
                obs[LM._leaf_callers(topo, i)] = True
    else:
        obs = LM.make_mask(topo, locs, pattern)
    return topo, locs, LM._y(obs), LM._spec(), LM.R, obs


@pytest.mark.parametrize("pattern", ["first_child", "first_two_alternate", "two_families", "first_family_last_leaf", "one_leaf",
                                     "full_leaves"])
def test_conditional_draws_on_gappy_masks(hip, pattern):
    """x_c(z) = x(z) + mean(y - x_o(z) - sqrt(R) eps(z)) with mean from the level-wise oracle, for caller-given z: leaves without
    observations, families whose first child is empty, whole empty families, fully observed leaves."""
    from oracle.mra_levelwise import run_levelwise
    topo, locs, y_obs, spec, R, obs = _masked_tree(64, 16, 3, pattern)
    pl = _spec_plan(hip, topo, locs, y_obs, spec, R)
    _, Kn = SM.coarse_offsets(topo)
    P = topo.P
    rng = np.random.RandomState(7)
    Z = rng.normal(size=(3, pl.sample_slots()))
    xc = pl.sample(3, z=Z, conditional=True)
    x = pl.sample(3, z=Z)
    rep = SM.reported(topo)
    real = topo.perm >= 0
    scale = np.abs(x).max()
    y = np.asarray(y_obs, dtype=float).ravel()
    for s in range(3):
        ps = np.full(topo.N, np.nan)
        o = real & np.isfinite(np.where(real, y[topo.perm], np.nan))
        ps[topo.perm[o]] = y[topo.perm[o]] - x[s, o] - np.sqrt(R) * Z[s, Kn + P + np.nonzero(o)[0]]
        mean = run_levelwise(topo, locs, spec, ps.reshape(-1, 1), R)["mean"]
        assert np.abs(xc[s, rep] - (x[s, rep] + mean[topo.perm[rep]])).max() <= 1e-9 * scale
        assert np.all(xc[s, ~rep] == 0.0)


def test_conditional_factor_with_an_empty_leaf_matches_dense_conditioning(hip):
    from oracle.mra_faithful import prior_sigma_rows
    topo, locs, y_obs, spec, R, obs = _masked_tree(32, 16, 2, "first_child")
    assert topo.P <= 2048
    pl = _spec_plan(hip, topo, locs, y_obs, spec, R)
    rr = np.nonzero(SM.reported(topo))[0]
    Gc, _ = SM.factor_columns(pl, np.arange(pl.sample_slots()), rows=rr, conditional=True, chunk=256)
    S = prior_sigma_rows(topo, locs, spec.evaluate, rr)
    o = np.isfinite(np.asarray(y_obs, dtype=float).ravel()[topo.perm[rr]])
    L = np.linalg.cholesky(S[np.ix_(o, o)] + R * np.eye(int(o.sum())))
    T = np.linalg.solve(L, S[o, :])
    assert np.abs(Gc @ Gc.T - (S - T.T @ T)).max() <= 1e-9 * np.abs(S).max()


# ---- state, errors, batches --------------------------------------------------------------------------------------------------------
def test_not_spd_leaf_gram_leaves_the_plan_as_it_was(hip):
    """A NaN location at an unobserved row that is a knot of its leaf and of no ancestor: the plan's own likelihood pass never reads
    the row, the leaf's v_M(K, K) is NaN in that row and column, and its Cholesky must report MRA_ERR_NOT_SPD.  Afterwards the device
    y, the last likelihood / predict and every option are as before, and after a clean set_locs the draws equal a fresh plan's."""
    from pymra_amd.plan import MraError
    topo, locs, y_obs, spec, R = _mid_tree("grid64_r32")
    pl = _spec_plan(hip, topo, locs, y_obs, spec, R)
    lik0, (m0, v0) = pl.likelihood(), pl.predict()
    opts = {k: pl.get_option(k) for k in OPTION_VALUES}
    x0 = pl.sample(3, seed=5)
    anc = set()
    for i in np.nonzero(~np.asarray(topo.node_leaf, dtype=bool))[0]:
        anc.update(int(r) for r in topo.knot_rows[topo.knot_ptr[i]:topo.knot_ptr[i + 1]])
    y = np.asarray(y_obs, dtype=float).ravel()
    j = np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0][5]
    cand = [int(r) for r in topo.knot_rows[topo.knot_ptr[j]:topo.knot_ptr[j + 1]]
            if int(r) not in anc and topo.perm[r] >= 0 and not np.isfinite(y[topo.perm[r]])]
    bad = locs.copy()
    bad[topo.perm[cand[0]]] = np.nan
    pl.set_locs(bad)
    with pytest.raises(MraError) as ei:
        pl.sample(2, seed=5)
    assert ei.value.code == -3
    assert pl.likelihood() == lik0
    m, v = pl.predict()
    assert np.array_equal(m, m0) and np.array_equal(v, v0)
    assert {k: pl.get_option(k) for k in OPTION_VALUES} == opts
    pl.set_locs(locs)
    assert np.array_equal(pl.sample(3, seed=5), x0)
    pl.run(True, True)
    assert pl.likelihood() == lik0                                        # the device y came back
    fresh = _spec_plan(hip, topo, locs, y_obs, spec, R)
    assert np.array_equal(pl.sample(3, seed=5), fresh.sample(3, seed=5))


def test_simulate_is_sample_through_perm(hip):
    import pymra_amd
    import pymra_amd.MRATools as mt
    cs = _load("t201")
    c, t = cs["c"], cs["topo"]
    tree = pymra_amd.MRATree(cs["locs"], c["r"], lambda a, b: mt.ExpCovFun(a, b, l=c["l"]), cs["y_obs"], c["R"], M=c["M"], J=c["J"])
    assert np.array_equal(tree.topology.perm, t.perm)
    dropped = t.perm[(t.perm >= 0) & ~np.asarray(t.in_leaf, dtype=bool)]
    assert len(dropped) > 0
    rows = SM.reported(t)
    for distr, cond in (("prior", False), ("posterior", True)):
        sim = tree.simulate(3, distr, seed=77)
        x = tree.plan.sample(3, seed=77, conditional=cond)
        ref = np.zeros((len(cs["locs"]), 3))
        ref[t.perm[rows]] = x[:, rows].T
        assert np.array_equal(sim, ref) and np.all(sim[dropped] == 0.0)


def test_sample0_must_be_non_negative(hip):
    from pymra_amd.plan import MraError
    pl = _plan(hip, _load("g32"))
    for s0, n in ((-1, 1), (-(2 ** 63), 1), (2 ** 63 - 1, 2)):
        with pytest.raises(MraError) as ei:
            pl.sample(n, seed=1, sample0=s0)
        assert ei.value.code == -1
    x = pl.sample(1, seed=1, sample0=2 ** 63 - 1)                         # the last sample number
    assert np.all(np.isfinite(x))


def test_gram_budget_does_not_change_the_draws(hip):
    """MRA_OPT_SAMPLE_GRAM_BYTES: one leaf per batch, about three leaves per batch and the default (one batch) give bit-identical
    prior and conditional draws, with n > 16 so that several sample blocks refactor their batches."""
    from pymra_amd.plan import MRA_OPT_SAMPLE_GRAM_BYTES, MraError
    topo, locs, y_obs, spec, R = _mid_tree("g64m")
    pl = _spec_plan(hip, topo, locs, y_obs, spec, R)
    assert pl.get_option(MRA_OPT_SAMPLE_GRAM_BYTES) == 0
    leaves = np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]
    nr = int(max(topo.node_row1[j] - topo.node_row0[j] for j in leaves))
    out = []
    for budget in (0, 1, 3 * (nr * nr + 16 * nr) * 8, 0):
        pl.set_option(MRA_OPT_SAMPLE_GRAM_BYTES, budget)
        assert pl.get_option(MRA_OPT_SAMPLE_GRAM_BYTES) == budget
        out.append((pl.sample(21, seed=3), pl.sample(18, seed=4, conditional=True)))
    for x, c in out[1:]:
        assert np.array_equal(x, out[0][0]) and np.array_equal(c, out[0][1])
    with pytest.raises(MraError) as ei:
        pl.set_option(MRA_OPT_SAMPLE_GRAM_BYTES, -1)
    assert ei.value.code == -1
    assert pl.get_option(MRA_OPT_SAMPLE_GRAM_BYTES) == 0
