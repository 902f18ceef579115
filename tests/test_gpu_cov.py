"""mra_cov_apply / HipPlan.cov_apply / MRATree.covariance / MRATree.functionalCovariance on the GPU: the MRA prior and posterior
covariance applied to vectors.  Truths that do not come from the device operator: Sigma = sum_j B_j k_j B_j^T from the reference's own
per-node blocks (tests/golden/*_nodes.npz), the faithful oracle's lineage-restricted prior_sigma_rows, dense Gaussian conditioning of
either on the case's mask, the covariance kernel itself on single-leaf trees, the sampler's factor G, and predict()'s variance.

Bounds are those of the assertion in tests/test_gpu_sample.py / tests/test_gpu_solve.py that makes the same kind of comparison
(cited where used).  Those assertions bound ENTRIES of Sigma (|G G^T - S| <= 1e-10 of the scale), so the random columns here are
weights of unit 1-norm, as a regional mean's are: every entry of Sigma A is then a signed average of entries of Sigma and the
entrywise bound applies to it unchanged.  (With N(0, 1) entries a column weighs ~800 entries of Sigma, and the oracle's own error is
multiplied by that: on g32 with the Gaussian kernel, whose knot blocks are close to singular, prior_sigma_rows is itself unsymmetric
by 2.5e-11, and both the device and the float64 restatement of tests/_treecov.py differ from it by the same 1.44e-10 on such a column;
by 9e-13 on unit vectors.)

Two comparisons have no such assertion and carry MEASURED bounds: 10 x the worst error seen on one MI355X against the dense /
oracle truth (never against cov_apply itself), absolute and scaled by the largest prior variance.
  * The posterior's own diagonal entry against predict()'s variance, on the cases with a dense truth.  Worst error against dense
    conditioning over the five unit rows, cov_apply / predict(): g32 5.33e-15 / 2.22e-15, c1 1.11e-15 / 1.29e-15,
    kat3 5.55e-16 / 2.86e-16, u3 1.44e-15 / 1.23e-15  ->  POST_DIAG_TOL = 5.3e-14, 1.3e-14, 5.6e-15, 1.4e-14.
    (|cov - predict| itself was at most 7.6e-15, 1.1e-15, 2.8e-16, 3.8e-16.)
  * BASELINE config 3: the prior at 200 rows against prior_sigma_rows, worst error 1.19e-13  ->  C3_PRIOR_TOL = 1.2e-12; the posterior
    unit column's own entry against predict()'s variance there, 1.77e-15  ->  C3_POST_TOL = 1.8e-14.
Where no dense truth can be formed (the deep 64-wide tree, the tree behind MRATree) the diagonal is held to POST_NO_TRUTH_TOL = 1e-9:
both sides are float64 evaluations of the same Sigma_post[i, i], and the existing tests accept each within 1e-9 of the scale of
dense conditioning (seen there: 1.9e-14)."""
import functools

import numpy as np
import pytest

import _cases as K
import _sampling as SM

pytestmark = pytest.mark.gpu

CASES = ["g32", "c1", "kat3", "u3"]
R_MASK = 2e-2
PRIOR_TOL = 1e-10            # test_gpu_sample.py: `assert np.abs(GG[...] - S[...]).max() <= 1e-10 * scale` (and its three siblings)
POST_DIAG_TOL = {"g32": 5.3e-14, "c1": 1.3e-14, "kat3": 5.6e-15, "u3": 1.4e-14}      # measured, see the module docstring
C3_PRIOR_TOL = 1.2e-12
C3_POST_TOL = 1.8e-14
POST_NO_TRUTH_TOL = 1e-9


def _post_tol(name):
    return 1e-6 if name == "u3" else 1e-9      # test_gpu_sample.py: `tol = 1e-6 if name == "u3" else 1e-9` (dense conditioning)


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def _plan(plan_mod, topo, locs, y_obs, R, spec, run=True):
    pl = plan_mod.HipPlan(topo, 0)
    pl.set_locs(locs)
    pl.set_obs(y_obs, R)
    pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale, spec.circular)
    if run:
        pl.run(True, True)
    return pl


def _padded(topo, A, rep):
    """(P, c) values at padded rows -> (c, P) with NaN at every unreported row: the call must not read them."""
    Ap = np.full((A.shape[1], topo.P), np.nan)
    Ap[:, rep] = A[rep].T
    return Ap


def _random(topo, rep, c, seed):
    """c random columns supported on the rows `rep`, each of unit 1-norm (see the module docstring)."""
    A = np.zeros((topo.P, c))
    A[rep] = np.random.default_rng(seed).standard_normal((int(rep.sum()), c))
    return A / np.abs(A).sum(0)


def _units(topo, rows):
    A = np.zeros((topo.P, len(rows)))
    A[rows, np.arange(len(rows))] = 1.0
    return A


def _unit_rows(topo, rep):
    """Padded rows for unit vectors: a root knot row, a mid-level knot row, a leaf knot row, the last reported row of the last leaf, a
    reported row next to a phantom (next to an unreported row; the first reported row where the tree has none)."""
    lev = np.asarray(topo.node_level)
    nonleaf = [i for i in range(topo.n_nodes) if not topo.node_leaf[i]]
    leaves = [i for i in range(topo.n_nodes) if topo.node_leaf[i]]
    knots = lambda i: [int(r) for r in topo.knot_rows[topo.knot_ptr[i]:topo.knot_ptr[i + 1]] if rep[r]]      # noqa: E731
    rows = []
    if nonleaf:
        rows.append(knots(nonleaf[0])[0])
        mid = [i for i in nonleaf if lev[i] == max(lev[j] for j in nonleaf)]
        rows.append(knots(mid[len(mid) // 2])[-1])
    rows.append(knots(leaves[len(leaves) // 2])[0])
    last = leaves[-1]
    rows.append(int(np.nonzero(rep[:int(topo.node_row1[last])])[0][-1]))
    rr = np.nonzero(rep)[0]
    edge = [int(r) for r in rr if (r + 1 < topo.P and not rep[r + 1]) or (r > 0 and not rep[r - 1])]
    rows.append(edge[len(edge) // 2] if edge else int(rr[0]))
    return rows


def _dense_posterior(S, o, R):
    L = np.linalg.cholesky(S[np.ix_(o, o)] + R * np.eye(int(o.sum())))
    T = np.linalg.solve(L, S[o, :])
    return S - T.T @ T


def _observed(topo, y_obs, rows):
    return np.isfinite(np.asarray(y_obs, float).ravel())[topo.perm[rows]]


def _check_gram(A, out, gram, rep):
    """gram = A_rep out^T inside the 16-column blocks - the mean of an entry and its mirror image, as the header says -, NaN outside them,
    symmetric to the bit."""
    c = A.shape[1]
    blk = np.arange(c) // 16
    same = blk[:, None] == blk[None, :]
    assert np.all(np.isfinite(gram[same])) and np.all(np.isnan(gram[~same]))
    want = A[rep].T @ out[:, rep].T
    want = 0.5 * (want + want.T)
    # test_gpu_solve.py: `assert np.abs(quad[same] - quad.T[same]).max() <= 1e-12 * np.abs(np.diag(quad)).max()` (one quantity, two orders of summation)
    assert np.abs(gram[same] - want[same]).max() <= 1e-12 * np.abs(np.diag(want)).max()
    assert np.array_equal(gram[same], gram.T[same])


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(case, rep, Sigma over the padded rows, Sigma_post[rep, rep]) of a golden case, computed once and read-only."""
    cs = K.load_case(name)
    topo = cs["topo"]
    rep = SM.reported(topo)
    S = SM.golden_prior_sigma(name, topo)
    rr = np.nonzero(rep)[0]
    Sp = _dense_posterior(S[np.ix_(rr, rr)], _observed(topo, cs["y_obs"], rr), float(cs["c"]["R"]))
    S.setflags(write=False)
    Sp.setflags(write=False)
    return cs, rep, S, Sp


def _case_plan(hip, cs):
    return _plan(hip, cs["topo"], cs["locs"], cs["y_obs"], float(cs["c"]["R"]), cs["spec"])


# ---- 1. the reference's Sigma ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 5, 16, 17, 40])
@pytest.mark.parametrize("name", CASES)
def test_prior_matches_the_reference_sigma(hip, name, c):
    cs, rep, S, _ = _reference(name)
    topo = cs["topo"]
    pl = _case_plan(hip, cs)
    scale = np.abs(S[np.ix_(rep, rep)]).max()
    for A in (_random(topo, rep, c, seed=c), _units(topo, _unit_rows(topo, rep))):
        out, gram = pl.cov_apply(_padded(topo, A, rep))
        assert out.shape == (A.shape[1], topo.P) and gram.shape == (A.shape[1],) * 2
        want = S[:, rep] @ A[rep]
        err = np.abs(out[:, rep].T - want[rep]).max()
        print("%s c=%d: prior err %.2e (scale %.2f, |Sigma A| %.1f)" % (name, A.shape[1], err, scale, np.abs(want[rep]).max()))
        assert err <= PRIOR_TOL * scale
        assert np.all(out[:, ~rep] == 0.0)                       # exactly, with NaN in A at those rows
        _check_gram(A, out, gram, rep)
    pl.close()


@pytest.mark.parametrize("name", CASES)
def test_posterior_matches_dense_conditioning_and_predict(hip, name):
    cs, rep, S, Sp = _reference(name)
    topo = cs["topo"]
    pl = _case_plan(hip, cs)
    rr = np.nonzero(rep)[0]
    scale = np.abs(S[np.ix_(rep, rep)]).max()
    urows = _unit_rows(topo, rep)
    A = np.hstack([_random(topo, rep, 17, seed=3), _units(topo, urows)])
    out, gram = pl.cov_apply(_padded(topo, A, rep), posterior=True)
    err = np.abs(out[:, rep].T - Sp @ A[rep]).max()
    print("%s: posterior err %.2e (scale %.2f)" % (name, err, scale))
    assert err <= _post_tol(name) * scale
    assert np.all(out[:, ~rep] == 0.0)
    _check_gram(A, out, gram, rep)
    # the unit columns' own entries are predict()'s variance
    _, var = pl.predict()
    pos = {int(r): k for k, r in enumerate(rr)}
    for k, r in enumerate(urows):
        mine, pred, dense = out[17 + k, r], var[topo.perm[r]], Sp[pos[r], pos[r]]
        print("%s row %d: |cov - dense| %.2e, |predict - dense| %.2e, |cov - predict| %.2e" % (name, r, abs(mine - dense), abs(pred - dense), abs(mine - pred)))
        assert abs(mine - pred) <= POST_DIAG_TOL[name] * scale
    pl.close()


def test_prior_is_the_samplers_factor_squared(hip):
    cs, rep, S, _ = _reference("g32")
    topo = cs["topo"]
    pl = _case_plan(hip, cs)
    G, _ = SM.factor_columns(pl, np.arange(pl.sample_slots()), chunk=256)
    urows = _unit_rows(topo, rep)
    out, _ = pl.cov_apply(_padded(topo, _units(topo, urows), rep), want_gram=False)
    want = G @ G[urows].T
    assert np.abs(out.T - want).max() <= PRIOR_TOL * np.abs(S[np.ix_(rep, rep)]).max()
    pl.close()


# ---- 2. shapes where these kernels can break -----------------------------------------------------------------------------------------------
def _grid(nx, ny, r, M, seed=7, frac=0.4):
    """The builder of test_gpu_sample.py's mid-size trees, restated."""
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    rng = np.random.RandomState(100 + seed)
    np.random.seed(seed)                       # the knot draws of the tree replay use the global RNG
    locs = mt.genLocations2d(Nx=nx, Ny=ny)
    topo = build_topology(locs, r, M, 4)
    y = rng.normal(size=(len(locs), 1))
    return topo, locs, np.where(rng.uniform(size=(len(locs), 1)) < frac, y, np.nan)


def _shape_tree(name):
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    m32 = mt.KernelSpec(mt.KIND_MATERN32, 0.2, 1.1)
    if name == "grid48_r20":                   # leaves of 144 rows = 9 tiles
        return _grid(48, 48, 20, 2, seed=9, frac=0.7) + (m32, 1e-2)
    if name == "grid40_r5":                    # phantom knot columns
        return _grid(40, 40, 5, 3, seed=5) + (mt.KernelSpec(mt.KIND_EXP, 0.3), 1e-2)
    if name == "grid18_m0":                    # one leaf, no ancestors
        rng = np.random.RandomState(18)
        locs = mt.genLocations2d(Nx=18, Ny=18)
        y = rng.normal(size=(len(locs), 1))
        return build_topology(locs, 16, 0, 4), locs, np.where(rng.uniform(size=(len(locs), 1)) < 0.5, y, np.nan), mt.KernelSpec(mt.KIND_MATERN32, 0.3, 1.0), 2e-2
    cs = K.load_case(name)                     # kat1, kat4 (one leaf), t1000, kat3 (1-D, dropped rows)
    return cs["topo"], cs["locs"], cs["y_obs"], cs["spec"], float(cs["c"]["R"])


def _check_against_sigma(pl, topo, locs, y_obs, R, S, rr, name, c=17):
    """Prior and posterior of c random columns and the unit vectors against S = Sigma[rr, rr] over all reported rows rr."""
    rep = SM.reported(topo)
    scale = np.abs(S).max()
    A = np.hstack([_random(topo, rep, c, seed=5), _units(topo, _unit_rows(topo, rep))])
    Ap = _padded(topo, A, rep)
    out, gram = pl.cov_apply(Ap)
    e0 = np.abs(out[:, rr].T - S @ A[rr]).max()
    assert np.all(out[:, ~rep] == 0.0)
    _check_gram(A, out, gram, rep)
    Sp = _dense_posterior(S, _observed(topo, y_obs, rr), R)
    outp, gramp = pl.cov_apply(Ap, posterior=True)
    e1 = np.abs(outp[:, rr].T - Sp @ A[rr]).max()
    print("%s: prior err %.2e, posterior err %.2e (scale %.2f)" % (name, e0, e1, scale))
    assert e0 <= PRIOR_TOL * scale             # test_gpu_sample.py: `assert np.abs(G[rr] @ G[rr].T - S).max() <= 1e-10 * scale`
    assert e1 <= 1e-9 * scale                  # test_gpu_sample.py: `assert np.abs(Gc @ Gc.T - (S - T.T @ T)).max() <= 1e-9 * np.abs(S).max()`
    assert np.all(outp[:, ~rep] == 0.0)
    _check_gram(A, outp, gramp, rep)


@pytest.mark.parametrize("name", ["kat1", "kat4", "grid18_m0"])
def test_single_leaf_trees_are_the_kernel_itself(hip, name):
    topo, locs, y_obs, spec, R = _shape_tree(name)
    assert topo.n_nodes == 1
    pl = _plan(hip, topo, locs, y_obs, R, spec)
    rr = np.nonzero(SM.reported(topo))[0]
    C = np.asarray(spec.evaluate(locs[topo.perm[rr]], locs[topo.perm[rr]]))
    _check_against_sigma(pl, topo, locs, y_obs, R, C, rr, name)
    pl.close()


@pytest.mark.parametrize("name", ["grid48_r20", "grid40_r5", "t1000"])
def test_leaves_of_nine_tiles_phantom_columns_and_dropped_rows(hip, name):
    from oracle.mra_faithful import prior_sigma_rows
    topo, locs, y_obs, spec, R = _shape_tree(name)
    assert topo.P <= 4608
    if name == "grid48_r20":
        assert max(int(topo.node_row1[i] - topo.node_row0[i]) for i in range(topo.n_nodes) if topo.node_leaf[i]) == 144
    pl = _plan(hip, topo, locs, y_obs, R, spec)
    rr = np.nonzero(SM.reported(topo))[0]
    _check_against_sigma(pl, topo, locs, y_obs, R, prior_sigma_rows(topo, locs, spec.evaluate, rr), rr, name)
    pl.close()


def _deep_wide(frac=0.2):
    """256^2, r = 64, M = 5 (test_gpu_sample.py's _deep_wide, restated): the HI route, chains of five 64-wide ancestors."""
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    np.random.seed(29)
    locs = mt.genLocations2d(Nx=256, Ny=256)
    y = np.random.normal(size=(256 * 256, 1))
    y_obs = np.where(np.random.uniform(size=(256 * 256, 1)) < frac, y, np.nan)
    return build_topology(locs, 64, 5, 4), locs, y_obs, mt.KernelSpec(mt.KIND_MATERN32, 0.25, 1.2), 2e-2


def _leaf_sets(topo):
    """Leaves whose lowest common ancestors differ: two siblings, a cousin (same grandparent), the middle leaf and the last."""
    leaves = np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]
    par = np.asarray(topo.node_parent)
    sib = [j for j in leaves[1:] if par[j] == par[leaves[0]]][0]
    cousin = [j for j in leaves if par[j] != par[leaves[0]] and par[par[j]] == par[par[leaves[0]]]][0]
    return [int(j) for j in (leaves[0], sib, cousin, leaves[len(leaves) // 2], leaves[-1])]


def test_deep_wide_tree_on_chosen_lineages(hip):
    """cw = 64: the fronts' blocks are not staged in LDS by the solver above 64 columns, the chain is 5 x 64 columns.  Vectors supported
    on five leaves against the lineage-restricted oracle; the posterior's own diagonal against predict()'s variance."""
    from oracle.mra_faithful import prior_sigma_rows
    topo, locs, y_obs, spec, R = _deep_wide()
    assert max(int(c) for c in topo.cw) == 64
    pl = _plan(hip, topo, locs, y_obs, R, spec)
    assert pl.route()["path"] == "Hi"
    rep = SM.reported(topo)
    allr = np.concatenate([K.node_real_rows(topo, j) for j in _leaf_sets(topo)])
    S = prior_sigma_rows(topo, locs, spec.evaluate, allr)
    on = np.zeros(topo.P, dtype=bool)
    on[allr] = True
    urows = [int(allr[0]), int(allr[len(allr) // 2]), int(allr[-1])]
    A = np.hstack([_random(topo, on & rep, 5, seed=2), _units(topo, urows)])
    Ap = _padded(topo, A, rep)
    out, gram = pl.cov_apply(Ap)
    err = np.abs(out[:, allr].T - S @ A[allr]).max()
    print("deep wide: prior err %.2e (scale %.2f)" % (err, np.abs(S).max()))
    assert err <= PRIOR_TOL * np.abs(S).max()                   # test_gpu_sample.py: `assert np.abs(G @ G.T - S).max() <= 1e-10 * np.abs(S).max()`
    assert np.all(out[:, ~rep] == 0.0)
    _check_gram(A, out, gram, rep)
    outp, _ = pl.cov_apply(Ap, posterior=True, want_gram=False)
    _, var = pl.predict()
    for k, r in enumerate(urows):
        d = abs(outp[5 + k, r] - var[topo.perm[r]])
        print("deep wide row %d: |cov - predict| %.2e" % (r, d))
        assert d <= POST_NO_TRUTH_TOL * np.abs(S).max()
    pl.close()


# ---- 3. every device kernel family, the circular distance ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["exp", "matern52", "gaussian", "kanter", "iden", "matern32_scale", "circular"])
def test_every_kernel_family(hip, family):
    import pymra_amd.MRATools as mt
    from oracle.mra_faithful import prior_sigma_rows
    specs = {"exp": mt.KernelSpec(mt.KIND_EXP, 0.3), "matern52": mt.KernelSpec(mt.KIND_MATERN52, 0.2, 0.7),
             "gaussian": mt.KernelSpec(mt.KIND_GAUSSIAN, 0.05, 1.0), "kanter": mt.KernelSpec(mt.KIND_KANTER, 0.35),
             "iden": mt.KernelSpec(mt.KIND_IDEN, 0.01), "matern32_scale": mt.KernelSpec(mt.KIND_MATERN32, 0.4, 1.0, 2.5),
             "circular": mt.KernelSpec(mt.KIND_EXP, 0.3, 1.0, 1.0, True)}
    cs = K.load_case("c1" if family == "circular" else "g32")
    topo, locs, spec, R = cs["topo"], cs["locs"], specs[family], float(cs["c"]["R"])
    pl = _plan(hip, topo, locs, cs["y_obs"], R, spec)
    rr = np.nonzero(SM.reported(topo))[0]
    _check_against_sigma(pl, topo, locs, cs["y_obs"], R, prior_sigma_rows(topo, locs, spec.evaluate, rr), rr, family, c=5)
    pl.close()


# ---- 4. gappy masks ------------------------------------------------------------------------------------------------------------------
def _gappy_tree(n=64, r=16, M=3, seed=7):
    """A regular tree with an empty first leaf, an empty family and a cloud-shaped gap (test_gpu_solve.py's, restated)."""
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
    return topo, locs, np.where(obs, rng.standard_normal(len(locs)), np.nan)


@functools.lru_cache(maxsize=None)
def _gappy():
    import pymra_amd.MRATools as mt
    topo, locs, y_obs = _gappy_tree()
    for a in (locs, y_obs):
        a.setflags(write=False)
    return topo, locs, y_obs, mt.KernelSpec(mt.KIND_MATERN32, 0.25, 1.2)


def test_posterior_on_a_mask_with_an_empty_leaf_and_an_empty_family(hip):
    from oracle.mra_faithful import prior_sigma_rows
    topo, locs, y_obs, spec = _gappy()
    pl = _plan(hip, topo, locs, y_obs, R_MASK, spec)
    rr = np.nonzero(SM.reported(topo))[0]
    _check_against_sigma(pl, topo, locs, y_obs, R_MASK, prior_sigma_rows(topo, locs, spec.evaluate, rr), rr, "gappy 64^2", c=5)
    pl.close()


# ---- 5. state ----------------------------------------------------------------------------------------------------------------------
def _factor_launches(pl):
    return sum(s["launches"] for s in pl.kernel_stats())


def test_cov_apply_leaves_the_callers_state_and_shares_the_factors_with_solve(hip):
    topo, locs, y_obs, spec = _gappy()
    pl = _plan(hip, topo, locs, y_obs, R_MASK, spec)
    rep = SM.reported(topo)
    opts = {k: pl.get_option(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20)}
    lik0, (m0, v0) = pl.likelihood(), pl.predict()
    Ap = _padded(topo, _random(topo, rep, 5, seed=4), rep)
    Yp = np.nan_to_num(Ap)
    o1, g1 = pl.cov_apply(Ap, posterior=True)
    assert _factor_launches(pl) > 0                                     # the first call ran its own likelihood pass
    assert pl.likelihood() == lik0
    m1, v1 = pl.predict()
    assert np.array_equal(m1, m0) and np.array_equal(v1, v0)
    assert {k: pl.get_option(k) for k in opts} == opts
    o2, g2 = pl.cov_apply(Ap, posterior=True)
    assert _factor_launches(pl) == 0                                    # the second one launched no kernel of a pass
    assert np.array_equal(o1, o2) and np.array_equal(g1, g2)            # the same bits: fixed order of summation
    p1, _ = pl.cov_apply(Ap)
    assert _factor_launches(pl) == 0
    mean1, quad1 = pl.solve(Yp)                                         # solve after cov_apply reuses the factors
    assert _factor_launches(pl) == 0
    o3, _ = pl.cov_apply(Ap, posterior=True)                            # the solver's node buffers are not the cov path's
    assert np.array_equal(o3, o1)
    pl.run(True, True)                                                  # y untouched: the old numbers bit for bit
    assert pl.likelihood() == lik0
    m2, v2 = pl.predict()
    assert np.array_equal(m2, m0) and np.array_equal(v2, v0)
    mean2, _ = pl.solve(Yp)                                             # the run invalidated the factors
    assert _factor_launches(pl) > 0
    o4, g4 = pl.cov_apply(Ap, posterior=True)                           # cov_apply after solve reuses them
    assert _factor_launches(pl) == 0
    # test_gpu_solve.py: `assert np.abs(mean3 - mean1).max() <= 1e-12 * max(1.0, np.abs(mean1).max()), what`
    assert np.abs(o4 - o1).max() <= 1e-12 * max(1.0, np.abs(o1).max())
    assert np.abs(mean2 - mean1).max() <= 1e-12 * max(1.0, np.abs(mean1).max())
    for what in ("run", "set_obs", "set_kernel", "sample"):
        if what == "set_obs":
            pl.set_obs(y_obs, R_MASK)
        elif what == "set_kernel":
            pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
        elif what == "sample":
            pl.sample(2, seed=1, conditional=True)
        else:
            pl.run(True, False)
        o5, _ = pl.cov_apply(Ap)
        assert _factor_launches(pl) > 0, what
        assert np.abs(o5 - p1).max() <= 1e-12 * max(1.0, np.abs(p1).max()), what
    out0, gram0 = pl.cov_apply(np.zeros((0, topo.P)))
    assert out0.shape == (0, topo.P) and gram0.shape == (0, 0)
    assert pl.cov_apply(Ap, want_out=False)[0] is None and pl.cov_apply(Ap, want_gram=False)[1] is None
    pl.close()


def test_cov_apply_refusals(hip):
    import ctypes as C
    from pymra_amd.plan import MraError
    import pymra_amd.MRATools as mt
    topo, locs, y_obs, spec = _gappy()
    rep = SM.reported(topo)
    A = _random(topo, rep, 2, seed=1)
    Ap = _padded(topo, A, rep)
    pl = hip.HipPlan(topo, 0)
    for step in ("nothing", "locs", "kernel"):
        if step == "locs":
            pl.set_locs(locs)
        elif step == "kernel":
            pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
        with pytest.raises(MraError) as e:
            pl.cov_apply(Ap)
        assert e.value.code == -4, step                  # MRA_ERR_STATE before set_locs / set_kernel / set_obs
    pl.set_obs(y_obs, R_MASK)
    good, _ = pl.cov_apply(Ap)
    out = np.empty((2, topo.P))

    def raw(flags, n, a, o=out):
        return pl.lib.mra_cov_apply(pl._h, flags, n, None if a is None else a.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), None)
    Az = np.nan_to_num(Ap)
    assert raw(2, 2, Az) == -1 and raw(3, 2, Az) == -1   # unknown flags
    assert raw(0, -1, Az) == -1                          # n_cols < 0
    assert raw(0, 2, None) == -1                         # NULL A with n_cols > 0
    assert raw(0, 0, None) == 0                          # n_cols == 0
    for bad_value in (np.nan, np.inf):
        bad = Ap.copy()
        bad[1, np.nonzero(rep)[0][7]] = bad_value
        with pytest.raises(MraError) as e:
            pl.cov_apply(bad)
        assert e.value.code == -1
    assert np.array_equal(pl.cov_apply(Ap)[0], good)     # the plan is still usable, and gives the same bits
    pl.set_reduce_level(0)
    with pytest.raises(MraError) as e:
        pl.cov_apply(Ap)
    assert e.value.code == -1                            # sharded
    pl.close()
    from pymra_amd import MRATree
    np.random.seed(1)
    n = 16
    l2 = mt.genLocations2d(Nx=n, Ny=n)
    y = np.random.normal(size=(n * n, 1))
    tree = MRATree(l2, 16, lambda a, b=np.array([]): np.exp(-np.abs(mt.dist(a, b)) / 0.3), y, 1e-2, M=1, J=4, verbose=False)      # opaque callable: host cov
    with pytest.raises(NotImplementedError):
        tree.covariance([0])
    with pytest.raises(NotImplementedError):
        tree.functionalCovariance(np.ones(n * n))
    with pytest.raises(MraError) as e:
        tree.plan.cov_apply(np.zeros((1, tree.topology.P)))
    assert e.value.code == -1                            # MRA_KERNEL_HOST


# ---- 6. through MRATree ------------------------------------------------------------------------------------------------------------------
def test_mratree_covariance_is_cov_apply_through_perm(hip):
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
    m0, sd0 = [np.asarray(a).ravel().copy() for a in tree.predict()]
    t = tree.topology
    rep = SM.reported(t)
    inv = np.full(n * n, -1)
    inv[t.perm[rep]] = np.nonzero(rep)[0]                                       # caller row -> padded row
    rows = np.array([0, 5, n * n - 1, 517])
    for distr in ("prior", "posterior"):
        cols = tree.covariance(rows, distr=distr)
        assert cols.shape == (n * n, len(rows))
        direct, _ = tree.plan.cov_apply(_padded(t, _units(t, inv[rows]), rep), posterior=(distr == "posterior"))
        want = np.zeros((n * n, len(rows)))
        want[t.perm[rep]] = direct[:, rep].T
        assert np.array_equal(cols, want)
        A = rng.standard_normal((n * n, 20))
        F = tree.functionalCovariance(A, distr=distr)
        assert F.shape == (20, 20) and np.all(np.isfinite(F)) and np.array_equal(F, F.T)
        Ap = np.zeros((t.P, 20))
        Ap[rep] = A[t.perm[rep]]
        o, g = tree.plan.cov_apply(_padded(t, Ap, rep), posterior=(distr == "posterior"))
        full = Ap[rep].T @ o[:, rep].T
        assert np.abs(F - 0.5 * (full + full.T)).max() <= 1e-12 * np.abs(np.diag(full)).max()
        same = (np.arange(20) // 16)[:, None] == (np.arange(20) // 16)[None, :]
        assert np.abs(F[same] - g[same]).max() <= 1e-12 * np.abs(np.diag(full)).max()
        assert tree.functionalCovariance(A[:, 0], distr=distr).shape == (1, 1)
    var = tree.covariance(rows, distr="posterior")[rows, np.arange(len(rows))]
    assert np.abs(var - sd0[rows] ** 2).max() <= POST_NO_TRUTH_TOL
    assert float(tree.getLikelihood()[0, 0]) == lik0
    m1, sd1 = [np.asarray(a).ravel() for a in tree.predict()]
    assert np.array_equal(m1, m0) and np.array_equal(sd1, sd0)
    with pytest.raises(ValueError):
        tree.covariance([n * n])
    with pytest.raises(ValueError):
        tree.covariance([0], distr="conditional")


# ---- 7. BASELINE config 3 ------------------------------------------------------------------------------------------------------------
def test_regional_mean_and_a_unit_column_at_c3(hip):
    """Two columns at 1024^2, M = 6: the indicator / n of a rectangle that covers parts of four leaves in two families, and a unit vector.
    The prior at ~200 chosen rows against the lineage-restricted oracle; the posterior unit column's own entry against predict()."""
    import bench
    import pymra_amd.MRATools as mt
    from oracle.mra_faithful import prior_sigma_rows
    from pymra_amd.topology import build_topology
    c = bench.CONFIGS["c3"]
    locs, y_obs = bench.make_inputs(c)
    topo = build_topology(locs, c["r"], c["M"], c["J"])
    spec = mt.KernelSpec(mt.KIND_MATERN32, c["l"], c["sig"])
    rep = SM.reported(topo)
    leaves = np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]
    leaf_of = np.full(topo.P, -1)
    for j in leaves:
        leaf_of[int(topo.node_row0[j]):int(topo.node_row1[j])] = j
    caller_leaf = np.full(topo.N, -1)
    caller_leaf[topo.perm[rep]] = leaf_of[rep]
    par = np.asarray(topo.node_parent)
    h = 3.5 / (c["n"] - 1)                                   # a 7 x 7 block of grid points around a leaf's corner
    box = None
    for j in leaves[len(leaves) // 2:]:
        pts = locs[topo.perm[K.node_real_rows(topo, int(j))]]
        corner = pts.max(0) + 0.5 / (c["n"] - 1)
        inside = np.all(np.abs(locs - corner) <= h, axis=1) & (caller_leaf >= 0)
        hit = np.unique(caller_leaf[inside])
        if len(hit) == 4 and len(set(par[hit])) == 2:
            box = inside
            break
    assert box is not None and 36 <= box.sum() <= 64
    inv = np.full(topo.N, -1)
    inv[topo.perm[rep]] = np.nonzero(rep)[0]
    box_rows = inv[np.nonzero(box)[0]]
    rng = np.random.default_rng(1)
    far = K.node_real_rows(topo, int(leaves[7]))
    near = np.concatenate([K.node_real_rows(topo, int(j)) for j in hit])
    rows = np.unique(np.concatenate([box_rows, rng.choice(near, 120, replace=False), rng.choice(far, 30, replace=False)]))
    unit = int(box_rows[0])
    A = np.zeros((topo.P, 2))
    A[box_rows, 0] = 1.0 / len(box_rows)
    A[unit, 1] = 1.0
    pl = _plan(hip, topo, locs, y_obs, c["R"], spec)
    Ap = _padded(topo, A, rep)
    out, gram = pl.cov_apply(Ap)
    S = prior_sigma_rows(topo, locs, spec.evaluate, rows)
    scale = np.abs(S).max()
    err = np.abs(out[:, rows].T - S @ A[rows]).max()
    print("c3: %d rows, prior err %.2e (scale %.2f), prior variance of the regional mean %.6f" % (len(rows), err, scale, gram[0, 0]))
    assert err <= C3_PRIOR_TOL * scale
    assert np.all(out[:, ~rep] == 0.0)
    _check_gram(A, out, gram, rep)
    outp, gramp = pl.cov_apply(Ap, posterior=True)
    _, var = pl.predict()
    d = abs(outp[1, unit] - var[topo.perm[unit]])
    print("c3: posterior unit entry %.12f, predict variance %.12f, |diff| %.2e; posterior sd of the regional mean %.6f"
          % (outp[1, unit], var[topo.perm[unit]], d, np.sqrt(gramp[0, 0])))
    assert d <= C3_POST_TOL * scale
    assert 0.0 < gramp[0, 0] < gram[0, 0] and abs(gramp[1, 1] - outp[1, unit]) <= 1e-12 * scale
    pl.close()
