"""The host-evaluated covariance table of tests/_hostcov_cells.py (no GPU): its covariances are what makes a covdiag or a stride bug
visible, its masks hold their counts, its expectations reach every route value a host plan can take on these trees, the block
builder of HipPlan.upload_host_cov hands over exactly the blocks mra_plan_set_cov_block demands, and the bars of
tests/test_gpu_hostcov.py stand two orders of magnitude above what one ulp in every covariance value does to the oracle."""
import numpy as np
import pytest

import _hostcov_cells as HC
import _route_cells as RC
import test_gpu_likelihood_masks as MK
import test_gpu_routes as TR

# members no host cell reaches, each with the route_for line that makes it so (none)
EXCUSED = set()
HOST_VALUES = {
    "leaf_resident": (False, True), "acc_var": (False, True), "predict": (False, True), "gemm_lds": (0, 1),
    "c_fix": ("Phantom", "Fill"), "var": ("FinishVar", "Moments", "None"), "update": ("Gemm", "LeafGemm", "None"),
    "chol": ("TilesOne", "TilesSplit", "Wave", "BigPanels"),
}


def _reached(routes):
    seen = {}
    for _, e in routes:
        for k, v in e.items():
            seen.setdefault(k, set()).add(v)
    missing = ["%s::%s" % (f, v) for f, values in HOST_VALUES.items() for v in values if v not in seen.get(f, ())]
    return [m for m in missing if m not in EXCUSED]


# ---- the covariances ----------------------------------------------------------------------------------------------------------------
def test_the_covariances_are_opaque_and_neither_stationary_nor_isotropic():
    from pymra_amd.MRATree import probe_cov
    for key in ("A", "T1"):
        topo, locs, cov, _ = HC.tree(key)
        X = np.asarray(locs, dtype=np.float64).reshape(topo.N, -1)
        assert probe_cov(cov, X.shape[1], X) is None and probe_cov(cov, X.shape[1]) is None
        out = cov(X[:5], X[:7])
        assert type(out) is np.ndarray and out.shape == (5, 7) and out.dtype == np.float64
        assert np.array_equal(cov(X[:7], X[:5]), out.T)                          # symmetric to the bit
        assert np.array_equal(cov(X[2:5], X[3:7]), out[2:5, 3:7])                # a pair's bits do not depend on the block asked for
        diag = np.array([cov(X[k:k + 1], X[k:k + 1])[0, 0] for k in range(0, topo.N, max(1, topo.N // 997))])
        assert diag.min() > 0 and diag.max() > 2.0 * diag.min(), (key, diag.min(), diag.max())
    # equal Euclidean distance, covariances more than 10 % apart: along the two axes (2-D), at two places of the warp (1-D)
    h = 0.1
    a = np.array([[0.4, 0.4]])
    c0, c1 = HC.cov2(a, a + [[h, 0.0]])[0, 0], HC.cov2(a, a + [[0.0, h]])[0, 0]
    assert abs(c0 - c1) > 0.1 * max(c0, c1), (c0, c1)
    c0, c1 = HC.cov1(np.array([[0.05]]), np.array([[0.05 + h]]))[0, 0], HC.cov1(np.array([[0.75]]), np.array([[0.75 + h]]))[0, 0]
    assert abs(c0 - c1) > 0.1 * max(c0, c1), (c0, c1)
    # a dense matrix of either is positive definite once the nugget is on (they are PSD by construction)
    X = np.random.RandomState(0).uniform(size=(200, 2))
    assert np.linalg.eigvalsh(HC.cov2(X, X)).min() > -1e-12
    assert np.linalg.eigvalsh(HC.cov1(X[:, :1], X[:, :1])).min() > -1e-12


def test_one_ulp_moves_every_value_by_one_ulp_the_same_way_everywhere():
    X = np.random.RandomState(2).uniform(size=(60, 2))
    moved = HC.one_ulp(HC.cov2)
    v, w = HC.cov2(X, X), moved(X, X)
    assert np.all(w != v) and np.array_equal(np.abs(w - v), np.spacing(np.minimum(np.abs(v), np.abs(w))))
    up = (w > v).mean()
    assert 0.3 < up < 0.7                                                       # both directions
    assert np.array_equal(moved(X[10:20], X[5:40]), w[10:20, 5:40]) and np.array_equal(w, w.T)


# ---- the masks ----------------------------------------------------------------------------------------------------------------------
def test_host_masks_hold_their_counts():
    """The edge masks on A hold every count of RC.EDGE_COUNTS and 96, 97, 112, 113 (the 6 / 7-tile boundary, exactly seven tiles and
    seven plus one) in one tree, the first leaf empty, the last the largest, small and large leaves interleaved; two_families has a
    whole family of empty leaves; every (tree, mask) has the largest leaf its cells were derived from."""
    assert {96, 97, 112, 113} <= set(HC.HOST_EDGE_COUNTS) and set(RC.EDGE_COUNTS) <= set(HC.HOST_EDGE_COUNTS)
    for recipe, top in ((HC.HEDGE, 192), (HC.HEDGE193, 193), (HC.HEDGE160, 160)):
        topo, _, _, _, _, cnt = HC.case("A", recipe)
        want = set(c for c in HC.HOST_EDGE_COUNTS if c < min(top, 192)) | {top}
        assert want <= set(cnt.tolist()) and cnt.max() == top and (cnt[0], cnt[-1]) == (0, top), recipe
        small = RC.tiles(cnt) <= 8
        assert 0 < small.sum() < len(cnt)
        # interleaved, not "all small first" (160: the four leaves beyond 8 tiles are 129, 144, 159 and, last, 160 - eight runs)
        assert int(np.count_nonzero(np.diff(small.astype(int)))) + 1 >= (10 if top >= 192 else 8), recipe
        seven = RC.tiles(cnt) <= 7
        assert 0 < seven.sum() < len(cnt)                                        # leaves of one and of two column passes
    topo, _, _, _, _, cnt = HC.case("S", HC.FAMILIES)
    empty = [[cnt[list(np.nonzero(topo.node_leaf)[0]).index(i)] == 0 for i in f] for f in MK._families(topo)]
    assert sum(all(f) for f in empty) >= 2 and any(not any(f) for f in empty)
    for key, recipe in HC.GROUPS:
        topo, _, _, _, y, cnt = HC.case(key, recipe)
        assert cnt.sum() == np.isfinite(y).sum() > 0
        for c in HC.CELLS:
            if (c["tree"], c["mask"]) == (key, recipe):
                assert int(RC.tiles(cnt).max()) == c["ntl"], (key, recipe, int(cnt.max()))
        rows = (topo.node_row1 - topo.node_row0)[np.asarray(topo.node_leaf, dtype=bool)]
        resident = rows.max() >= 128 and int(RC.tiles(cnt).max()) * 16 >= 64    # route_for's leaf_resident, option 6 at its default
        assert all(c["expect"]["leaf_resident"] == resident for c in HC.CELLS
                   if (c["tree"], c["mask"]) == (key, recipe) and dict(c["opts"]).get(6, 1) != 0), (key, recipe)
    topo = HC.tree("W200")[0]
    assert [int(c) for c in topo.cw] == [208, 0] and int(topo.knot_ptr[1] - topo.knot_ptr[0]) == 200
    topo = HC.tree("T1")[0]
    assert topo.d == 1 and set(int(c) for c in topo.cw[:-1]) == {16} and int(topo.knot_ptr[1] - topo.knot_ptr[0]) == 2
    assert np.any(topo.perm < 0)                                               # leaves of about 12 rows padded to 16: phantom rows in every leaf


# ---- coverage -----------------------------------------------------------------------------------------------------------------------
def test_the_host_table_reaches_every_host_route_value():
    assert not EXCUSED
    routes = HC.all_expected_routes()
    assert _reached(routes) == []
    for label, e in routes:
        assert (e["path"], e["prior_level"], e["c_only"], e["lik_rows"], e["lik_general"]) == ("Levels", False, False, False, False), label
        assert e["extract_mean"] == e["predict"], label
        assert set(("leaf_resident", "acc_var", "c_fix", "chol", "var", "update")) <= set(e), label
    for key in HC.TREES:                          # a likelihood-only cell and the direct GEMM on every tree
        mine = [c for c in HC.CELLS if c["tree"] == key]
        assert any(not c["predict"] for c in mine) and any(dict(c["opts"]).get(3) == 0 for c in mine), key
    lik_only = {(c["tree"], c["mask"]): c["expect"]["c_fix"] for c in HC.CELLS if not c["predict"]}
    assert lik_only[("A", HC.HEDGE193)] == "Fill" and set(v for k, v in lik_only.items() if k != ("A", HC.HEDGE193)) == {"Phantom"}
    assert HC.SHARDED["expect"]["side"] is True


def test_deleting_the_only_row_of_a_member_is_noticed():
    """The coverage check bites: without the one option 6 = 2 cell LeafGemm is reported missing; without the 193 mask Fill and
    BigPanels are, and without W200 as well Moments is; without the option 3 = 0 cells the direct GEMM is."""
    routes = HC.all_expected_routes()
    assert sum(e["update"] == "LeafGemm" for _, e in routes) == 1
    assert _reached([(l, e) for l, e in routes if e["update"] != "LeafGemm"]) == ["update::LeafGemm"]
    assert sorted(_reached([(l, e) for l, e in routes if "193" not in l])) == ["c_fix::Fill", "chol::BigPanels"]
    assert _reached([(l, e) for l, e in routes if "160" not in l]) == ["chol::TilesOne"]
    assert "var::Moments" in _reached([(l, e) for l, e in routes if "193" not in l and not l.startswith("W200")])
    assert _reached([(l, e) for l, e in routes if e["gemm_lds"] == 1]) == ["gemm_lds::0"]


# ---- the block builder --------------------------------------------------------------------------------------------------------------
def _recorder(topo):
    """A HipPlan without library and device: upload_host_cov itself runs, set_kernel_host and set_cov_block record."""
    from pymra_amd import plan as P

    class Recorder(P.HipPlan):
        def __init__(self, topo):
            self.topo, self._h, self.blocks, self.selected = topo, None, [], 0

        def set_kernel_host(self):
            assert not self.blocks
            self.selected += 1

        def set_cov_block(self, node, C, diag=None):
            assert self.selected == 1                                           # MRA_KERNEL_HOST is selected before the first block
            self.blocks.append((int(node), np.array(C, dtype=np.float64), None if diag is None else np.array(diag, dtype=np.float64)))

    return Recorder(topo)


def _check_blocks(topo, locs, cov, y, blocks, tag):
    X = np.asarray(locs, dtype=np.float64).reshape(len(y), -1)
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    assert sorted(b[0] for b in blocks) == list(range(topo.n_nodes)), tag       # every node once
    zero_cols = 0
    for i, C, dg in blocks:
        r0, r1 = int(topo.node_row0[i]), int(topo.node_row1[i])
        xs = X[topo.src[r0:r1]]
        assert C.ndim == 2 and C.shape[0] == r1 - r0, (tag, i, C.shape)
        if topo.node_leaf[i]:
            # the library's own count (build_leaf): the leaf's real rows with a finite observation, in ascending padded-row order
            cols = [p for p in range(r0, r1) if topo.perm[p] >= 0 and np.isfinite(yv[topo.perm[p]])]
            assert C.shape[1] == len(cols), (tag, i, C.shape, len(cols))
            zero_cols += len(cols) == 0
            if cols:
                assert np.array_equal(C, cov(xs, X[topo.perm[cols]])), (tag, i)
            assert dg is not None and dg.shape == (r1 - r0,), (tag, i)
            assert np.array_equal(dg, np.array([cov(xs[k:k + 1], xs[k:k + 1])[0, 0] for k in range(r1 - r0)])), (tag, i)   # phantom rows included
        else:
            kq = topo.knot_rows[topo.knot_ptr[i]:topo.knot_ptr[i + 1]]
            assert C.shape[1] == len(kq) and dg is None, (tag, i, C.shape)
            assert np.array_equal(C, cov(xs, X[topo.src[kq]])), (tag, i)
    return zero_cols


def test_upload_host_cov_hands_over_the_blocks_the_library_demands():
    """Rows node_row1 - node_row0; columns the knot count, or the leaf's observed rows in ascending padded-row order, 0 columns
    included; a leaf's diag is cov at every one of its rows.  S two_families (8 leaves without observations) and the four ranks of its
    4-way sharding (upper nodes' rows: kept children and orphan knot rows), from a callable and from a dense matrix."""
    from pymra_amd.sharding import shard_topology
    topo, locs, cov, _, y, cnt = HC.case("S", HC.FAMILIES)
    rec = _recorder(topo)
    rec.upload_host_cov(cov, locs, y)
    assert _check_blocks(topo, locs, cov, y, rec.blocks, "single") == int((cnt == 0).sum()) == 8
    assert np.any(topo.perm < 0)                                                # phantom rows exist on this tree
    empty_ranks = 0
    for rk in range(4):
        lt, red = shard_topology(topo, 4, rk)
        assert red == 0
        upper = int(lt.level_ptr[1])
        orphans = (lt.perm >= 0) & ~np.asarray(lt.in_leaf, dtype=bool)
        assert orphans.any() and lt.node_row1[0] - lt.node_row0[0] == lt.P < topo.P and upper == 1
        rec = _recorder(lt)
        rec.upload_host_cov(cov, locs, y)
        empty_ranks += _check_blocks(lt, locs, cov, y, rec.blocks, "rank %d" % rk)
    assert empty_ranks == 8
    # a dense matrix gives the same blocks as the callable it was evaluated from (a tree small enough for N x N)
    topo, locs, cov, _ = HC.tree("T1")
    y = HC.make_obs("T1", HC.GOLDEN)[1]
    a, b = _recorder(topo), _recorder(topo)
    a.upload_host_cov(cov, locs, y)
    b.upload_host_cov(cov(locs, locs), locs, y)
    assert all(i == j and np.array_equal(C, D) and (d is e is None or np.array_equal(d, e)) for (i, C, d), (j, D, e) in zip(a.blocks, b.blocks))
    _check_blocks(topo, locs, cov, y, b.blocks, "dense")
    with pytest.raises(ValueError):
        _recorder(topo).upload_host_cov(np.eye(3), locs, y)


# ---- the bars have margin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,recipe", HC.GROUPS, ids=["%s-%s" % (k, "-".join(str(x) for x in m)) for k, m in HC.GROUPS])
def test_one_ulp_in_every_covariance_value_stays_a_hundredth_of_the_bars(key, recipe):
    """The oracle alone is the evidence that ORACLE_BARS = (1e-10 lik rel, 1e-9 mean abs, 1e-8 sd rel) leave room for a correct
    implementation: run_levelwise with cov against run_levelwise with every covariance value moved by one ulp (HC.one_ulp) must stay
    below 1/100 of each bar.  Measured (float64, NumPy / LAPACK on the CPU):

        tree  mask                 lik rel    mean abs   sd rel
        S     cloud                8.3e-16    3.7e-13    1.1e-13
        S     two_families         1.2e-15    2.7e-13    9.0e-14
        A     host_edges           1.2e-15    5.7e-13    2.0e-13
        A     host_edges 160       1.1e-15    5.7e-13    2.0e-13
        A     host_edges 193       9.4e-16    5.7e-13    2.0e-13
        A     cloud                2.5e-15    5.6e-13    1.9e-13
        C64   cloud                1.3e-16    8.9e-13    2.1e-13
        W200  fraction 0.08        9.5e-16    2.2e-13    7.8e-14
        T1    golden (cov1)        7.2e-16    2.0e-14    6.2e-14

    three to five orders of magnitude under the bars."""
    from oracle.mra_levelwise import run_levelwise
    topo, locs, cov, R, y, _ = HC.case(key, recipe)
    ref = HC.oracle(key, recipe)
    moved = run_levelwise(topo, locs, HC.one_ulp(cov), y, R)
    assert np.all(ref["sd"][np.asarray(topo.perm[topo.in_leaf])] > 0)
    rep = ref["sd"] > 0
    e_l = abs(moved["lik"] - ref["lik"]) / abs(ref["lik"])
    e_m = float(np.abs(moved["mean"] - ref["mean"]).max())
    e_s = float((np.abs(moved["sd"] - ref["sd"])[rep] / ref["sd"][rep]).max())
    print("%s %s one ulp: lik %.1e mean %.1e sd %.1e" % (key, recipe, e_l, e_m, e_s))
    assert e_l < TR.ORACLE_BARS[0] / 100 and e_m < TR.ORACLE_BARS[1] / 100 and e_s < TR.ORACLE_BARS[2] / 100, (e_l, e_m, e_s)
