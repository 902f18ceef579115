"""MRA_OPT_LEAF_ORDER (GPU only): the oversized leaves' Cholesky, row solve and update on the side stream beside the small leaves', and
every ordered leaf list longest first.  All of it is scheduling - which stream a launch goes to and which workgroup takes which
leaf - so every result must be BITWISE what option 0 (leaf order, serial launches) gives.

One tree (tests/_leaf_order_case.py): 1024 leaves of 144 rows, so that the leaf Cholesky is split in two launches beside leaves of
nine tiles; its mask has an empty leaf, leaves of one tile, of exactly eight tiles and three of nine tiles in three families.  Against
the level-wise oracle (fixture tests/golden/leaf_order.npz, sampled rows) the bounds are those tests/test_gpu_parity.py holds the
fused path to on leaves above 128 observations: 1e-10 relative on the likelihood, 1e-9 on the mean, 1e-8 relative on the sd."""
import numpy as np
import pytest

import _cases as K
import _leaf_order_case as LC
import _route_cells as RC
import test_gpu_likelihood_masks as MK

pytestmark = pytest.mark.gpu

OPT = 22                    # MRA_OPT_LEAF_ORDER
SETTINGS = (0, 1, 2, 3, 4)  # serial and leaf order / fork and longest first / the fork alone / the order alone / 1 and the residual product


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    assert plan.MRA_OPT_LEAF_ORDER == OPT
    return plan


@pytest.fixture(scope="module")
def case():
    topo, locs, obs, y = LC.build()
    return dict(topo=topo, locs=locs, obs=obs, y=y, counts=MK.leaf_counts(topo, obs))


def _sites(topo, locs):
    """A site next to the first row of a few leaves (an empty one, one tile, eight tiles, nine tiles), assigned to that leaf."""
    leaves = [int(i) for i in np.nonzero(topo.node_leaf)[0]]
    pick = [leaves[p] for p in (5, 0, 6, 1, 7, 500, 1023, 300)]
    X = np.asarray(locs, float)
    sites = np.array([X[MK._leaf_callers(topo, i)[0]] + 1e-4 for i in pick])
    return sites, np.asarray(pick, dtype=np.int32)


def _passes(pl):
    """A likelihood + predict pass, a likelihood-only pass, a second predict pass (the phantom rows of C are reused)."""
    out = {}
    for tag, predict in (("predict", True), ("likelihood", False), ("predict again", True)):
        pl.run(True, predict)
        out[tag] = dict(lik=pl.likelihood(), route=pl.route())
        if predict:
            m, v = pl.predict()
            out[tag].update(mean=m.copy(), var=v.copy())
    return out


@pytest.fixture(scope="module")
def runs(hip, case):
    """{setting: results} on ONE plan, set_obs again after each switch (the order is read when the leaf lists are built)."""
    topo, locs, y = case["topo"], case["locs"], case["y"]
    s = MK._spec()
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, LC.R); pl.set_kernel(s.kind, s.l, s.sig, s.scale)
    Yp = np.zeros((16, topo.P))
    real = topo.perm >= 0
    Yp[:, real] = np.random.default_rng(3).standard_normal((16, int(real.sum())))
    Yp[0, real] = np.nan_to_num(y.ravel()[topo.perm[real]])
    sites, leaf = _sites(topo, locs)
    out = {}
    for v in SETTINGS + (1,):                     # (ends on the default; its second visit must reproduce the first)
        pl.set_option(OPT, v)
        assert pl.get_option(OPT) == v
        pl.set_obs(y, LC.R)
        res = _passes(pl)
        pl.set_option(7, 1)                       # k_leaf_solve_update for the small leaves: the others' plain update follows the join
        res["solve_fused"] = _passes(pl)["predict"]
        pl.set_option(7, 2)
        res["solve"] = pl.solve(Yp)
        res["sites"] = pl.predict_sites(sites, leaf)
        if v in out:
            _same_passes(out[v], res, "setting %d, second visit" % v)
        out[v] = res
    pl.close()
    return out


def _same_passes(a, b, what):
    for tag in ("predict", "likelihood", "predict again", "solve_fused"):
        assert a[tag]["lik"] == b[tag]["lik"], (what, tag)
        assert a[tag]["route"] == b[tag]["route"], (what, tag)
        if "mean" in a[tag]:
            assert np.array_equal(a[tag]["mean"], b[tag]["mean"]) and np.array_equal(a[tag]["var"], b[tag]["var"]), (what, tag)


def test_the_mask_has_every_kind_of_leaf(case):
    counts, tl = case["counts"], RC.tiles(case["counts"])
    assert len(counts) == 1024 and all(counts[p] == c for p, c in LC.EXACT.items())
    assert (counts == 0).sum() >= 1 and (tl == 1).sum() >= 3 and (counts == 128).sum() == 1 and (tl == 8).sum() >= 2
    big = np.nonzero(tl >= 9)[0]
    assert tuple(big) == LC.OVERSIZED and len(set(int(p) // 4 for p in big)) == 3 and int(tl.max()) == 9
    assert tl[0] < tl.max() and tl[0] < tl[1]                     # neither order is the identity


def test_the_side_chain_runs_and_the_route_read_back_is_unchanged(hip, runs):
    for v in SETTINGS:
        for tag in ("predict", "likelihood", "predict again", "solve_fused"):
            r = runs[v][tag]["route"]
            assert r["path"] == "Fused" and r["chol"] == "TilesSplit", (v, tag, r)
            assert r["n_leaves"] == 1024 and r["n_trsm_small"] == 1024 - len(LC.OVERSIZED) == r["n_chol_small"], (v, tag, r)
            assert 0 < r["n_trsm_small"] < r["n_leaves"]
            assert r == runs[0][tag]["route"], (v, tag)
    assert runs[1]["predict"]["route"]["update"] == "InCascade" and runs[1]["likelihood"]["route"]["c_only"]
    assert runs[1]["solve_fused"]["route"]["update"] in ("SolveHalves", "SolveWhole")


@pytest.mark.parametrize("v", SETTINGS[1:])
def test_passes_are_bitwise_those_of_leaf_order_and_serial_launches(runs, v):
    _same_passes(runs[0], runs[v], "setting %d against 0" % v)
    a = runs[v]
    assert a["predict"]["lik"] == a["predict again"]["lik"] and np.array_equal(a["predict"]["mean"], a["predict again"]["mean"])
    assert np.array_equal(a["predict"]["var"], a["predict again"]["var"])


@pytest.mark.parametrize("v", SETTINGS[1:])
def test_retained_factor_consumers_are_bitwise_the_same(runs, v):
    m0, q0 = runs[0]["solve"]
    m1, q1 = runs[v]["solve"]
    assert np.array_equal(m0, m1) and np.array_equal(q0, q1, equal_nan=True)
    assert np.isfinite(m0).all() and np.isfinite(np.diag(q0)).all()
    (sm0, sv0), (sm1, sv1) = runs[0]["sites"], runs[v]["sites"]
    assert np.array_equal(sm0, sm1) and np.array_equal(sv0, sv1) and np.isfinite(sm0).all() and (sv0 > 0).all()


def test_default_setting_matches_the_oracle(case, runs):
    g = np.load(LC.FIXTURE)
    assert abs(float(np.nansum(case["y"])) - float(g["y_checksum"])) < 1e-9 and int(case["obs"].sum()) == int(g["n_obs"]), "input recipe drifted"
    rows = g["rows"]
    assert np.array_equal(rows, LC.sample_rows(case["topo"]))
    res = runs[1]["predict"]
    lik = sum(res["lik"])
    e_l = abs(lik - float(g["lik"])) / abs(float(g["lik"]))
    e_m = float(np.max(np.abs(res["mean"][rows] - g["mean"])))
    e_s = K.rel(np.sqrt(res["var"][rows]), g["sd"])
    print("likelihood rel %.2e, mean abs %.2e, sd rel %.2e on %d rows" % (e_l, e_m, e_s, len(rows)))
    assert e_l <= 1e-10 and e_m < 1e-9 and e_s < 1e-8
    assert abs(sum(runs[1]["likelihood"]["lik"]) - float(g["lik"])) <= 1e-10 * abs(float(g["lik"]))


def test_a_failed_pass_is_reported_once_and_joins_both_streams(hip, case, runs):
    """The numerically singular kernel of tests/test_gpu_parity.py::test_a_failed_pass_leaves_nothing_behind: MRA_ERR_NOT_SPD, once;
    the next passes on the same plan (forks on) give what an untroubled plan gave."""
    import pymra_amd.MRATools as mt
    topo, locs, y = case["topo"], case["locs"], case["y"]
    s = MK._spec()
    pl = hip.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, LC.R)
    assert pl.get_option(OPT) == 1
    pl.set_kernel(mt.KIND_GAUSSIAN, 50.0, 1.0, 1.0)
    with pytest.raises(hip.MraError) as ei:
        pl.run(True, True)
    assert ei.value.code == -3
    pl.set_kernel(s.kind, s.l, s.sig, s.scale)
    for tag, predict in (("predict", True), ("likelihood", False)):
        pl.run(True, predict)
        assert pl.likelihood() == runs[1][tag]["lik"], tag
    pl.run(True, True)
    m, v = pl.predict()
    assert np.array_equal(m, runs[1]["predict"]["mean"]) and np.array_equal(v, runs[1]["predict"]["var"])
    pl.close()
