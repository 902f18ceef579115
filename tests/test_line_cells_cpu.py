"""The 1-D problems of tests/_line_cells.py, without a GPU: the trees have the shapes their names promise, the masks the counts they
claim, the expected routes cover what a regular ternary tree can reach, and the float64 oracle the GPU tests are held to agrees with
the 80-bit one to 1/100 of the GPU tests' bars on every (tree, family) of at most 4096 points - the condition that keeps a failure
of tests/test_gpu_line.py the kernels' and not the problem's."""
import numpy as np
import pytest

import _line_cells as LC
import _route_cells as RC
import test_gpu_likelihood_masks as MK

ORACLE_BARS = (1e-10, 1e-9, 1e-8)              # tests/test_gpu_routes.py: likelihood relative, mean absolute, sd relative


@pytest.mark.parametrize("key", list(LC.TREES))
def test_tree_shapes(key):
    topo, locs = LC.tree(key)
    N, r0, M = LC.TREES[key]
    levels, cw, lo, hi, dropped = LC.SHAPES[key]
    assert topo.d == 1 and topo.N == N and levels == [3 ** k for k in range(M + 1)]
    assert [int(v) for v in np.diff(topo.level_ptr)] == levels                           # ternary whatever J says
    assert [int(c) for c in topo.cw] == [cw] * M + [0] and cw == r0
    leaf = np.asarray(topo.node_leaf, dtype=bool)
    assert np.array_equal(np.nonzero(leaf)[0], np.arange(int(topo.level_ptr[M]), int(topo.level_ptr[M + 1])))      # leaves on the last level only
    assert set(np.diff(topo.knot_ptr)[~leaf].tolist()) == {r0}                           # full knot blocks: no phantom column
    rows = LC.leaf_rows(topo)
    assert (int(rows.min()), int(rows.max())) == (lo, hi)
    rep = LC.reported(topo)
    assert int((~rep).sum()) == dropped
    if key in ("L16d", "L64"):
        assert not rep.all()
    if key == "LE":
        assert LC.leaf_real_rows(topo).min() >= 208 and RC.leaf_capacity(topo) >= 208
    # leaves follow the coordinate: the first leaf holds the smallest locations, the last the largest
    lv = LC.leaves(topo)
    assert locs[MK._leaf_callers(topo, lv[0])].max() < locs[MK._leaf_callers(topo, lv[1])].min()
    assert locs[MK._leaf_callers(topo, lv[-1])].max() == locs.max()


def test_lds_budgets_of_the_cascades():
    """cascade_lds_all of build_static (mra_plan.hip): tiles of 2 KB against the 80 that 160 KB hold"""
    def tiles(cwt, nl):
        return cwt * cwt * (nl * (nl - 1) // 2) + nl * (cwt * (cwt - 1) // 2 + cwt)
    assert tiles(4, 4) == 136 and tiles(2, 7) == 105                                     # L64x, L32x: staged level by level
    for key in ("L16", "L16s", "L16d", "L32", "L64", "LE"):
        N, r0, M = LC.TREES[key]
        assert tiles(r0 // 16, M) <= 80, key                                             # stage-all: lik_rows can be True
    N, r0, M = LC.TREES["LH"]
    assert r0 == 64 and M == 5 and (r0 // 16) * M > 16                                   # not ``regular``: regular_hi


@pytest.mark.parametrize("key", [k for k in LC.TREES if k != "L32x"])
def test_default_mask_and_the_cells_preconditions(key):
    topo, locs, obs, y, counts = LC.problem(key)
    assert counts[0] == 0 and counts[1:].min() > 0                                       # one leaf without any observation
    rest = np.ones(topo.N, dtype=bool)
    rest[MK._leaf_callers(topo, LC.leaves(topo)[0])] = False
    assert abs(obs[rest].mean() - 0.4) < 0.03 and np.array_equal(np.isfinite(y), obs)
    assert not obs[~LC.reported(topo)].any()
    cells = LC.cells_of(key)
    assert cells
    for c in cells:
        assert LC.ntl(counts) == c["ntl"] and int(LC.leaf_rows(topo).min()) == c["rows_min"], (key, int(counts.max()))
        small = int((RC.tiles(counts) <= 8).sum())
        if c["expect"].get("chol") == "TilesSplit":
            assert small == len(counts) and c["ntl"] <= 8
        if c["expect"].get("chol") == "TilesOne":
            assert 0 < small < len(counts) and c["ntl"] <= 10
        if c["expect"].get("chol") == "BigPanels":
            assert c["ntl"] > 12
        if c["expect"].get("leaf_resident"):
            assert c["rows_min"] >= 128 and counts.max() > 48
        if c["expect"].get("solve_fused"):
            N, r0, M = LC.TREES[key]
            assert c["rows_min"] >= 128 and c["ntl"] <= 12 and (M * r0 + 16) // 16 <= 13
    if key == "LH":
        assert counts.max() <= 64                                                        # k_predict_hi folds the update: <= 4 observation tiles


def test_edge_masks_hold_their_counts():
    topo, locs = LC.tree("LE")
    for recipe, cls, top in LC.EDGE_MASKS:
        cnt = LC.problem("LE", recipe)[4]
        assert set(c for c in RC.EDGE_COUNTS if c <= 191) | {top} <= set(cnt.tolist()) and cnt.max() == top, recipe
        assert (cnt[0], cnt[-1]) == ((0, top) if recipe[1] == "empty_first" else (top, 0)), recipe
        small = RC.tiles(cnt) <= 8
        assert 0 < small.sum() < len(cnt)
        assert int(np.count_nonzero(np.diff(small.astype(int)))) + 1 >= 10                # small and large leaves alternate in leaf order


def test_gappy_masks_on_families_of_three():
    topo, locs = LC.tree("L16s")
    fams = MK._families(topo)
    assert [len(f) for f in fams] == [3] * 9
    want = {"first_child": lambda c: all(c[3 * k] == 0 and c[3 * k + 1] > 0 and c[3 * k + 2] > 0 for k in range(9)),
            "first_two_alternate": lambda c: all((c[3 * k] == 0 and c[3 * k + 1] == 0) == (k % 2 == 0) and c[3 * k + 2] > 0 for k in range(9)),
            "two_families": lambda c: c[9:15].sum() == 0 and c[:9].min() > 0 and c[15:].min() > 0,
            "last_child_only": lambda c: all(c[3 * k] == 0 and c[3 * k + 1] == 0 and c[3 * k + 2] > 0 for k in range(9)),
            "first_family_last_leaf": lambda c: c[:3].sum() == 0 and c[-1] == 0 and c[3:-1].min() > 0,
            "one_leaf": lambda c: np.count_nonzero(c) == 1 and c[9] > 0}
    assert set(want) == set(LC.GAPPY)
    for p in LC.GAPPY:
        topo, locs, obs, y, cnt = LC.problem("L16s", ("pattern", p))
        assert want[p](cnt), (p, cnt.tolist())
        assert (MK.cross_family_joins(topo, obs) > 0) == (p in MK.STALE), p             # the join rule that was wrong once would be wrong here


def test_sharded_masks():
    topo, locs, obs, y, cnt = LC.problem("L16s", ("empty_shard",))
    assert cnt[:9].sum() == 0 and cnt[9:].min() > 0
    from pymra_amd.sharding import shard_topology
    for rk in range(3):
        lt, red = shard_topology(topo, 3, rk)
        assert len(LC.leaves(lt)) == 9


# Route members no regular ternary tree reaches on one GPU, each with the line of route_for that makes it so
UNREACHED = {}
SWITCHES = ("solve_fused", "parent_front", "scatter_ut", "leaf_resident", "lik_rows", "lik_general", "side")


def test_the_expected_routes_reach_every_route_member():
    """Every member of the PassRoute enums and both values of every switch are the expectation of some cell: three children per
    node close no branch of route_for (it counts leaves, tiles and rows, never children), so nothing is excused."""
    from pymra_amd import plan as P
    seen = {}
    for _, e in LC.all_expected_routes():
        for k, v in e.items():
            seen.setdefault(k, set()).add(v)
    missing = ["%s::%s" % (f, m) for f, members in P.ROUTE_ENUMS.items() for m in members if m not in seen.get(f, ())]
    missing += ["%s=%s" % (f, v) for f in SWITCHES for v in (False, True) if v not in seen.get(f, ())]
    assert [m for m in missing if m not in UNREACHED] == []
    assert 0 in seen["n_chain"] and 2 in seen["n_chain_min"]


CONDITIONING = [("L16", f) for f in LC.FAMILIES] + [("L16s", "m32"), ("L16d", "m32"), ("L64", "m32")]


@pytest.mark.parametrize("key,fam", CONDITIONING, ids=["%s-%s" % c for c in CONDITIONING])
def test_the_float64_oracle_is_100_times_inside_the_bars(key, fam):
    from oracle.mra_extended import run_extended
    from oracle.mra_levelwise import run_levelwise
    topo, locs, obs, y, counts = LC.problem(key)
    assert topo.N <= 4096
    spec = LC.FAMILIES[fam]
    lw = run_levelwise(topo, locs, spec, y, LC.R)
    ext = run_extended(topo, locs, spec, y, LC.R)
    rep = LC.reported(topo)
    e_l = abs(lw["lik"] - ext["lik"]) / abs(ext["lik"])
    e_m = float(np.abs(lw["mean"] - ext["mean"]).max())
    e_s = float(np.max(np.abs(lw["sd"] - ext["sd"])[rep] / ext["sd"][rep]))
    print("%s %s: float64 against 80-bit: lik %.2e mean %.2e sd %.2e" % (key, fam, e_l, e_m, e_s))
    assert e_l <= ORACLE_BARS[0] / 100 and e_m <= ORACLE_BARS[1] / 100 and e_s <= ORACLE_BARS[2] / 100
    assert np.all(ext["mean"][~rep] == 0.0) and np.all(ext["sd"][~rep] == 0.0)
    if fam == "exp_circular":
        flat = run_levelwise(topo, locs, LC.FAMILIES["exp"], y, LC.R)
        assert abs(flat["lik"] - lw["lik"]) > 1e-6 * abs(lw["lik"])                       # the wrap is felt
    if fam == "kanter":
        iden = run_levelwise(topo, locs, LC.FAMILIES["iden"], y, LC.R)
        assert abs(iden["lik"] - lw["lik"]) > 0.1 * abs(lw["lik"])                        # what an oracle that took Kanter for Iden would give


def test_the_gaussian_prior_of_a_leaf_is_singular_at_the_likelihood_range():
    """What mra_sample has to factor: the MRA prior covariance of a leaf's own rows.  Gaussian, l = 0.01, 230 points 1 / 2048 apart:
    not positive definite in float64 for LAPACK either, so a refusal by the device is the problem's; at LC.GAUSS_SAMPLE it is."""
    import _treecov as TCV
    topo, locs, obs, y, counts = LC.problem("L16")
    rows = MK._leaf_callers(topo, LC.leaves(topo)[5])
    A = np.zeros((len(y), len(rows)))
    A[rows, np.arange(len(rows))] = 1.0
    C = TCV.tree_cov(topo, locs, LC.FAMILIES["gauss"], y, LC.R, A)[0][rows]
    assert np.linalg.eigvalsh(0.5 * (C + C.T)).min() < 1e-13
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(C)
    assert LC.GAUSS_SAMPLE.kind == LC.FAMILIES["gauss"].kind and LC.GAUSS_SAMPLE.l == 0.001
    C = TCV.tree_cov(topo, locs, LC.GAUSS_SAMPLE, y, LC.R, A)[0][rows]
    assert np.linalg.eigvalsh(0.5 * (C + C.T)).min() > 1e-9
    np.linalg.cholesky(C)
