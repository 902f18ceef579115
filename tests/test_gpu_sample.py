"""mra_sample / HipPlan.sample / MRATree.simulate on the GPU.  Exactness is checked against truths that do not come from the device:
the MRA prior covariance Sigma = sum_j B_j k_j B_j^T assembled from the reference's own per-node blocks (tests/golden/*_nodes.npz),
dense Gaussian conditioning of Sigma on the case's observations, the NumPy restatement of the latent draws (_philox), and - within
one leaf of a full-size tree, where the MRA is exact - the covariance kernel itself."""
import numpy as np
import pytest

import _cases as K
import _philox

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
    return (topo.perm >= 0) & np.asarray(topo.in_leaf, dtype=bool)


def _prior_sigma(cs):
    """Sigma over the padded rows from the reference's per-node B and kC (k = kC kC^T)."""
    topo = cs["topo"]
    gold = K.load_node_goldens(cs["_name"])
    S = np.zeros((topo.P, topo.P))
    for i in range(len(topo.node_row0)):
        g = gold[topo.node_ident[i]]
        rows = K.node_real_rows(topo, i)
        B, kC = np.asarray(g["B"]), np.asarray(g["kC"])
        assert B.shape[0] == len(rows)
        BK = B @ kC
        S[np.ix_(rows, rows)] += BK @ BK.T
    return S


def _factor(pl, conditional=False, chunk=256):
    """G with sample(z = e_k) = G[:, k] (prior); for conditional: G_c[:, k] = sample(e_k) - sample(0), and sample(0)."""
    n = pl.sample_slots()
    x0 = pl.sample(1, z=np.zeros((1, n)), conditional=conditional)[0]
    G = np.empty((pl.topo.P, n))
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        z = np.zeros((b - a, n))
        z[np.arange(b - a), np.arange(a, b)] = 1.0
        G[:, a:b] = (pl.sample(b - a, z=z, conditional=conditional) - (x0 if conditional else 0.0)).T
    return G, x0


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
    opts = {k: tree.plan.get_option(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18)}
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
    nslots = pl.sample_slots()
    zoff, k = {}, 0
    for i in range(len(topo.node_row0)):
        if not topo.node_leaf[i]:
            zoff[i] = k
            k += int(topo.cw[topo.node_level[i]])
    Kn = k
    leaves = np.where(np.asarray(topo.node_leaf, dtype=bool))[0]
    for j in (leaves[0], leaves[len(leaves) // 2], leaves[-1]):
        slots = []
        p = int(topo.node_parent[j])
        while p >= 0:
            slots.extend(range(zoff[p], zoff[p] + int(topo.cw[topo.node_level[p]])))
            p = int(topo.node_parent[p])
        kr = topo.knot_rows[topo.knot_ptr[j]:topo.knot_ptr[j + 1]]
        slots.extend(Kn + int(r) for r in kr)
        z = np.zeros((len(slots), nslots))
        z[np.arange(len(slots)), slots] = 1.0
        X = pl.sample(len(slots), z=z)
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
