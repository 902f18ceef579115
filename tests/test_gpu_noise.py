"""Per-observation noise variances on the GPU (mra_plan_set_noise).

1. a constant vector equals the scalar path bit for bit on every (path, Cholesky form, c_fix) the leaves can take;
2. a varying vector r = R s(x)^2 against the rescaled oracle of tests/_noise.py on the same cells, a second pass bit-identical,
   set_noise(None) back on the scalar result bit for bit;
3. T16 against dense algebra; 4. the 1-D tree t201, whose partition drops rows; 5. an opaque callable (MRA_KERNEL_HOST);
6. four emulated ranks; 7. the retained-factor calls against dense algebra; 8. conditional mra_sample; 9. MRATree.

Trees, masks and expected routes are those of tests/_route_cells.py: every run asserts its cell's route, which must not depend on
the noise.  Bars: ORACLE_BARS and ROUTE_BARS of tests/test_gpu_routes.py; for the retained-factor calls the bars their own GPU
tests use against dense conditioning (cited at each assertion)."""
import functools

import numpy as np
import pytest

import _cases as K
import _noise as NZ
import _route_cells as RC
import _sampling as SM
import test_gpu_likelihood_masks as MK
import test_gpu_routes as TR

pytestmark = pytest.mark.gpu

R = MK.R
LEVELS = ((2, 0),)
# one cell per distinct (path, Cholesky form, c_fix): (tree, mask, predict, options)
NOISE_CELLS = [
    ("A", RC.CLOUD, True, ()), ("A", RC.CLOUD, False, ()), ("A", RC.CLOUD, True, LEVELS), ("A", RC.CLOUD, False, LEVELS),
    ("B", RC.CLOUD, True, ()), ("S", RC.CLOUD, True, ()), ("A", RC.E193, True, ()), ("A", RC.E193, False, ()),
    ("H", RC.CLOUD, True, ()), ("H", RC.CLOUD, False, ()),
]
GROUPS = sorted(set((t, m) for t, m, _, _ in NOISE_CELLS))
IDS = ["%s-%s" % (k, "-".join(str(x) for x in m)) for k, m in GROUPS]


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _expect(key, recipe, predict, opts):
    hit = [c["expect"] for c in RC.CELLS if (c["tree"], c["mask"], c["predict"], c["opts"]) == (key, recipe, predict, tuple(opts))]
    assert len(hit) == 1, (key, recipe, predict, opts)
    return hit[0]


@functools.lru_cache(maxsize=None)
def _case(key, recipe):
    """(topo, locs, y, leaf counts, r) of one (tree, mask)"""
    topo, locs = TR._tree(key)
    obs = RC.make_obs(topo, locs, recipe)
    return topo, locs, MK._y(obs), MK.leaf_counts(topo, obs), NZ.noise_of(locs, R)


@functools.lru_cache(maxsize=None)
def _oracle(key, recipe):
    topo, locs, y, _, _ = _case(key, recipe)
    return NZ.scaled_oracle(topo, locs, MK._spec(), y, R)


def _pass(pl, predict):
    """(lik, mean, sd) of one pass; mean and sd None for a likelihood-only one"""
    if predict:
        return TR._predict(pl)
    pl.run(True, False)
    return sum(pl.likelihood()), None, None


def _same(a, b, tag):
    assert a[0] == b[0], "%s: likelihood %r != %r" % (tag, a[0], b[0])
    if a[1] is not None:
        assert np.array_equal(a[1], b[1]), tag + ": mean"
        assert np.array_equal(a[2], b[2]), tag + ": sd"


def _cells_of(key, recipe):
    return [(p, o) for t, m, p, o in NOISE_CELLS if (t, m) == (key, recipe)]


# ---- 1. a constant vector is the scalar path, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("key,recipe", GROUPS, ids=IDS)
def test_constant_vector_equals_scalar_bit_for_bit(hip, key, recipe):
    topo, locs, y, counts, _ = _case(key, recipe)
    pl = MK._plan(hip, topo, locs, y)
    const = np.full(topo.N, R)
    const[~np.isfinite(y.ravel())] = np.nan                          # never read
    for predict, opts in _cells_of(key, recipe):
        tag = "%s %s predict=%s %s" % (key, recipe, predict, opts)
        TR._set(pl, opts)
        pl.set_noise(None)
        scalar = _pass(pl, predict)
        TR._check_route(pl, _expect(key, recipe, predict, opts), tag + " scalar")
        pl.set_noise(const)
        vector = _pass(pl, predict)
        TR._check_route(pl, _expect(key, recipe, predict, opts), tag + " vector")
        _same(vector, scalar, tag)
        assert np.all(pl.buffer(10)[np.isfinite(y.ravel())[topo.src] & (topo.perm >= 0)] == R)
    pl.close()


# ---- 2. a varying vector against the rescaled oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("key,recipe", GROUPS, ids=IDS)
def test_varying_vector_against_the_rescaled_oracle(hip, key, recipe):
    topo, locs, y, counts, r = _case(key, recipe)
    ref = _oracle(key, recipe)
    pl = MK._plan(hip, topo, locs, y)
    for predict, opts in _cells_of(key, recipe):
        tag = "%s %s predict=%s %s" % (key, recipe, predict, opts)
        expect = _expect(key, recipe, predict, opts)
        TR._set(pl, opts)
        pl.set_noise(None)
        scalar = _pass(pl, predict)
        pl.set_noise(r)
        got = _pass(pl, predict)
        TR._check_route(pl, expect, tag)
        e_l = abs(got[0] - ref["lik"]) / abs(ref["lik"])
        print("%s: lik %.2e" % (tag, e_l))
        assert e_l <= TR.ORACLE_BARS[0], "%s: likelihood rel err %.3e" % (tag, e_l)
        if predict:
            TR._against(topo, counts, got, TR._ref3(ref), TR.ORACLE_BARS, tag + " vs rescaled oracle")
            assert np.abs(got[1] - scalar[1]).max() > 1e-3                   # the vector is no small perturbation
        assert abs(got[0] - scalar[0]) > 1e-6 * abs(scalar[0])
        _same(_pass(pl, predict), got, tag + " second pass")
        pl.set_noise(None)
        _same(_pass(pl, predict), scalar, tag + " back on the scalar")
        TR._check_route(pl, expect, tag + " back on the scalar")
    pl.close()


# ---- 3. / 4. / 5. dense algebra, a 1-D tree with dropped rows, an opaque callable -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _t16():
    topo, locs, y, counts, r = _case("T16", RC.CLOUD)
    assert topo.N == 4096
    return topo, locs, y, counts, r, NZ.dense_reference(topo, locs, MK._spec(), y, r)


def test_t16_against_dense_algebra(hip):
    topo, locs, y, counts, r, ref = _t16()
    pl = hip.HipPlan(topo, 0)
    s = MK._spec()
    pl.set_locs(locs); pl.set_obs(y, r); pl.set_kernel(s.kind, s.l, s.sig, s.scale)       # the vector through set_obs
    got = TR._predict(pl)
    TR._check_route(pl, _expect("T16", RC.CLOUD, True, ()), "T16")
    TR._against(topo, counts, got, TR._ref3(ref), TR.ORACLE_BARS, "T16 vs dense algebra")
    d, u = pl.likelihood()
    assert abs(d - ref["d"]) <= TR.ORACLE_BARS[0] * abs(ref["d"]) and abs(u - ref["u"]) <= TR.ORACLE_BARS[0] * abs(ref["u"])
    pl.close()


def test_1d_tree_with_dropped_rows(hip):
    cs = K.load_case("t201")
    topo, locs, y, spec, R1 = cs["topo"], cs["locs"], cs["y_obs"], cs["spec"], float(cs["c"]["R"])
    assert not NZ.reported(topo).all()
    r = NZ.noise_of(locs, R1)
    r[~NZ.reported(topo)] = np.nan                                    # rows no leaf reports are nobody's observation
    ref = NZ.scaled_oracle(topo, locs, spec, y, R1)
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, R1); pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
    pl.set_noise(r)
    lik, mean, sd = TR._predict(pl)
    rep = NZ.reported(topo)
    e_l, e_m = abs(lik - ref["lik"]) / abs(ref["lik"]), np.abs(mean - ref["mean"])[rep].max()
    e_s = (np.abs(sd - ref["sd"])[rep] / ref["sd"][rep]).max()
    print("t201: lik %.2e mean %.2e sd %.2e" % (e_l, e_m, e_s))
    assert e_l <= TR.ORACLE_BARS[0] and e_m <= TR.ORACLE_BARS[1] and e_s <= TR.ORACLE_BARS[2]
    assert np.all(mean[~rep] == 0.0)
    pl.close()


def test_opaque_callable_with_a_vector(hip):
    topo, locs, y, counts, r, _ = _t16()
    s = MK._spec()
    cov = lambda a, b: np.asarray(s.evaluate(a, b))                   # noqa: E731  (opaque: evaluated on the host, block by block)
    ref = _oracle("T16", RC.CLOUD)
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, R); pl.upload_host_cov(cov, locs, y)
    pl.set_noise(r)                                                   # keeps the blocks (set_obs would drop them)
    got = TR._predict(pl)
    TR._check_route(pl, dict(path="Levels"), "T16 host covariance")
    TR._against(topo, counts, got, TR._ref3(ref), TR.ORACLE_BARS, "T16 host covariance vs rescaled oracle")
    pl.run(True, False)
    assert abs(sum(pl.likelihood()) - ref["lik"]) <= TR.ORACLE_BARS[0] * abs(ref["lik"])
    pl.close()


# ---- 6. sharded ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("predict", [True, False], ids=["predict", "likelihood"])
def test_four_ranks_equal_the_single_plan(hip, predict):
    topo, locs, y, counts, r = _case("A4", RC.CLOUD)
    s = MK._spec()
    pl = MK._plan(hip, topo, locs, y)
    pl.set_noise(r)
    one = _pass(pl, predict)
    pl.set_noise(None)
    flat = _pass(pl, predict)
    pl.close()
    assert abs(one[0] - flat[0]) > 1e-6 * abs(flat[0])
    ranks = K.emulate_world_on_one_gpu(hip, topo, locs, y, r, s, 4, predict=predict, per_rank=True)
    expect = RC.SHARDED[0]["expect"] if predict else [dict(path="Fused", side=False, c_fix="InProduct", update="None")] * 4
    mean, var = np.zeros(topo.N), np.zeros(topo.N)
    for k, rk in enumerate(ranks):
        diff = {f: (rk["route"][f], v) for f, v in expect[k].items() if rk["route"][f] != v}
        assert not diff, "rank %d: route (got, expected) %s" % (k, diff)
        assert abs(rk["lik"] - one[0]) <= TR.ROUTE_BARS[0] * abs(one[0]), (k, rk["lik"], one[0])
        if predict:
            mean += rk["mean"]; var += rk["var"]
    if predict:
        TR._against(topo, counts, (one[0], mean, np.sqrt(var)), one, TR.ROUTE_BARS, "4 ranks vs the single plan")


# ---- 7. the retained-factor calls against dense algebra ------------------------------------------------------------------------------
def test_retained_factor_calls_against_dense_algebra(hip):
    import _treesites as TS
    import test_gpu_cov as GC
    import test_gpu_solve as TV
    import test_sites_cpu as SC
    topo, locs, y, counts, r, ref = _t16()
    s = MK._spec()
    Sigma, L, o = ref["Sigma"], ref["K_chol"], ref["o"]
    T = np.linalg.solve(L, Sigma[o, :])
    Sp = Sigma - T.T @ T                                              # Sigma_post = Sigma - Sigma[:, o] K^-1 Sigma[o, :]
    scale = np.abs(Sigma).max()
    pl = MK._plan(hip, topo, locs, y)
    pl.set_noise(r)
    rep_p = SM.reported(topo)
    # solve: test_gpu_solve.py `e_m <= tol * max(1.0, np.abs(want_mean).max())`, `e_q <= tol * np.abs(np.diag(want_quad)).max()`, tol 1e-9
    Y = TV._columns(y, 3)
    mean, quad = pl.solve(TV._padded(topo, Y))
    A = np.linalg.solve(L, Y[o])
    want_mean, want_quad = T.T @ A, A.T @ A
    e_m, e_q = np.abs(TV._caller(topo, mean) - want_mean).max(), np.abs(quad - want_quad).max()
    print("solve: mean %.2e quad %.2e" % (e_m, e_q))
    assert e_m <= 1e-9 * max(1.0, np.abs(want_mean).max())
    assert e_q <= 1e-9 * np.abs(np.diag(want_quad)).max()
    # cov_apply, posterior: test_gpu_cov.py `err <= _post_tol(name) * scale` (1e-9)
    Ap = GC._random(topo, rep_p, 16, seed=4)
    out, gram = pl.cov_apply(GC._padded(topo, Ap, rep_p), posterior=True)
    Ac = np.zeros((topo.N, 16)); Ac[topo.perm[rep_p]] = Ap[rep_p]
    want_out, want_gram = Sp @ Ac, Ac.T @ Sp @ Ac
    e_o, e_g = np.abs(TV._caller(topo, out) - want_out).max(), np.abs(gram - want_gram).max()
    print("cov_apply: out %.2e gram %.2e (scale %.2f)" % (e_o, e_g, scale))
    assert e_o <= 1e-9 * scale and e_g <= 1e-9 * scale
    # 48 tree rows as sites of their own leaf: test_gpu_sites.py `_mean_ok` (1e-8 of the scale) and `e_v <= _post_tol * scale`;
    # test_gpu_sitecov.py `e1 <= GC._post_tol(name) * scale`
    rows = np.nonzero(rep_p)[0][::85][:48]
    assert len(rows) == 48
    X = np.asarray(locs, float)
    sites, leaf, cr = X[topo.perm[rows]], SC.leaf_of_rows(topo)[rows], topo.perm[rows]
    m, v = pl.predict_sites(sites, leaf)
    e_m, e_v = np.abs(m[0] - ref["mean"][cr]).max(), np.abs(v - np.diag(Sp)[cr]).max()
    cv = pl.sites_cov(sites, leaf, posterior=True)
    e_c = np.abs(cv - Sp[np.ix_(cr, cr)]).max()
    print("48 own rows: mean %.2e var %.2e cov %.2e" % (e_m, e_v, e_c))
    assert e_m <= 1e-8 * max(1.0, np.abs(ref["mean"]).max())
    assert e_v <= 1e-9 * scale and e_c <= 1e-9 * scale
    # 16 sites off the rows: the restatement's mean on the rescaled problem, times s(site)
    off = SC.off_row_sites(locs, 16, seed=9)
    off_leaf = SC.nearest_leaf(topo, locs, off).astype(np.int32)
    want_off, _ = TS.tree_sites(topo, locs, NZ.ScaledSpec(s), (y.ravel() / NZ.s_of(locs)).reshape(y.shape), R, off, off_leaf)
    want_off = want_off[:, 0] * NZ.s_of(off)
    m_off, _ = pl.predict_sites(off, off_leaf)
    print("16 sites off the rows: mean %.2e" % np.abs(m_off[0] - want_off).max())
    assert np.abs(m_off[0] - want_off).max() <= 1e-8 * max(1.0, np.abs(want_off).max())
    # sample_sites, posterior: the mean of the antithetic pair z, -z is predict_sites' mean
    z = np.random.default_rng(12).standard_normal((1, pl.sample_sites_slots(16)))
    pair = pl.sample_sites(off, off_leaf, 2, z=np.vstack([z, -z]), posterior=True)
    assert np.abs(pair[0] - pair[1]).max() > 1e-3
    assert np.abs(0.5 * (pair[0] + pair[1]) - m_off[0]).max() <= 1e-8 * max(1.0, np.abs(want_off).max())
    pl.close()


# ---- 8. conditional draws -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", [0, 1])
def test_conditional_draw_uses_the_rows_own_noise(hip, solve):
    topo, locs, y, counts, r, _ = _t16()
    pl = MK._plan(hip, topo, locs, y)
    pl.set_noise(r)
    pl.set_option(hip.MRA_OPT_SAMPLE_SOLVE, solve)
    P = topo.P
    Kn = pl.sample_slots() - 2 * P
    z = np.random.default_rng(21).standard_normal((1, Kn + 2 * P))
    x = pl.sample(1, z=z)[0]                                          # the prior draw with the same z
    draw = pl.sample(1, z=z, conditional=True)[0]
    eps = z[0, Kn + P:]
    yp = np.where(topo.perm >= 0, y.ravel()[topo.src], np.nan)
    seen = np.isfinite(yp)
    rp = r[topo.src]
    Yp = np.zeros((1, P))
    Yp[0, seen] = yp[seen] - x[seen] - np.sqrt(rp[seen]) * eps[seen]
    mean, _ = pl.solve(Yp, want_quad=False)
    rep = SM.reported(topo)
    err = np.abs(draw - (x + mean[0]))[rep].max()
    flat = np.zeros((1, P))
    flat[0, seen] = yp[seen] - x[seen] - np.sqrt(R) * eps[seen]
    print("MRA_OPT_SAMPLE_SOLVE %d: %.2e (with sqrt(R) in the place of sqrt(r): %.2e)" % (solve, err, np.abs(flat - Yp).max()))
    assert err <= 1e-9
    assert np.abs(flat - Yp).max() > 1e-2                             # sqrt(R) eps would have been another draw
    pl.close()


# ---- 9. MRATree ------------------------------------------------------------------------------------------------------------------------
def test_mratree_with_a_noise_vector(hip):
    import pymra_amd
    import pymra_amd.MRATools as mt
    n, r0, M = RC.TREES["A"]
    topo, locs, y, counts, r = _case("A", RC.CLOUD)
    s = MK._spec()
    cov = lambda a, b: mt.Matern32(a, b, l=s.l, sig=s.sig)           # noqa: E731
    np.random.seed(7)                                                 # as MK._tree does: the same knots
    mt.genLocations2d(Nx=n, Ny=n)
    tree = pymra_amd.MRATree(locs, r0, cov, y, r, M=M, J=4)
    assert tree.R is r and np.array_equal(tree.topology.knot_rows, topo.knot_rows)
    pl = MK._plan(hip, topo, locs, y)
    pl.set_noise(r)
    want = TR._predict(pl)
    pl.close()
    lik = lambda v: float(np.asarray(v).ravel()[0])                   # noqa: E731
    mean, sd = tree.predict()
    assert lik(tree.getLikelihood()) == want[0]
    assert np.array_equal(np.asarray(mean).ravel(), want[1]) and np.array_equal(np.asarray(sd).ravel(), want[2])
    # setNoise: the scalar, then the vector again
    flat = MK._plan(hip, topo, locs, y)
    lik_flat = MK._lik_only(flat)
    flat.close()
    assert lik(tree.setNoise(R)) == lik_flat and tree.R == R
    assert lik(tree.setNoise(r, want_predict=True)) == want[0] and np.array_equal(np.asarray(tree.predict()[0]).ravel(), want[1])
    with pytest.raises(TypeError):
        pymra_amd.MRATree(locs, r0, cov, y, 1, M=M, J=4)
    with pytest.raises(TypeError):
        tree.setNoise(1)


def test_node_blocks_with_a_noise_vector(hip):
    """debug-posterior.py:97-109 with R = diag(r): B (I + B^T H^T R^-1 H B)^-1 B^T from the prior basis is the posterior covariance
    - predict()'s variance on its diagonal, BP BP^T from the posterior basis (whose leaves' kTil come from A = B_o^T diag(1 / r_o) B_o
    in pymra_amd.diagnostics).  Bars: those of tests/test_gpu_diagnostics.py."""
    import make_golden as mg
    import pymra_amd
    import scipy.linalg as lng
    cs = K.load_case("g32")
    c = cs["c"]
    assert c["dim"] == 2 and not c.get("data")
    r = NZ.noise_of(cs["locs"], float(c["R"]))
    mg.make_inputs(c)                                                 # global RNG where the reference had it when it drew its knots
    tree = pymra_amd.MRATree(cs["locs"], c["r"], cs["covfun"], cs["y_obs"], r, M=c["M"], J=c["J"])
    xP, sdP = tree.predict()
    nodes = tree.getNodeBlocks()
    assert len(nodes) == tree.topology.n_nodes
    B = np.asarray(tree.getBasisFunctionsMatrix(distr="prior", timesKC=True))
    BP = np.asarray(tree.getBasisFunctionsMatrix(distr="posterior", timesKC=True))
    obs = np.isfinite(np.asarray(cs["y_obs"]).ravel())
    Bo = B[obs]
    rec = B @ lng.inv(np.eye(B.shape[1]) + Bo.T @ (Bo / r[obs, None])) @ B.T
    assert np.max(np.abs(np.diag(rec) - np.asarray(sdP).ravel() ** 2)) < 1e-9
    assert np.max(np.abs(BP @ BP.T - rec)) < 1e-8
    mean_rec = rec[:, obs] @ (np.asarray(cs["y_obs"]).ravel()[obs] / r[obs])
    assert np.max(np.abs(mean_rec - np.asarray(xP).ravel())) < 1e-8
    flat = B @ lng.inv(np.eye(B.shape[1]) + Bo.T @ Bo / float(np.mean(r[obs]))) @ B.T
    assert np.max(np.abs(np.diag(flat) - np.diag(rec))) > 1e-4        # a scalar in its place is visibly another posterior
