"""The route table of tests/test_gpu_routes.py (asserted on a GPU) and tests/test_route_table.py (its coverage, on the CPU).

A cell is (tree, mask recipe, run flags, option tuple) -> the fields of the library's PassRoute (``HipPlan.route()``) that the pass
must show.  The expectations are written down from ``route_for`` (pymra_amd/csrc/mra_plan.hip), not read back from a run.  Its
thresholds count leaves against ``2 * n_cu`` (512 on an MI355X), so every tree here has 16, 64 or 1024 leaves - far from 512 on
any part with 32 to 500 compute units; the GPU test asserts that.

Trees (n x n grid, r0, M; J = 4), all with leaves of one size:
  A    128^2, 16, 3   64 leaves of 256 rows                  B    144^2, 16, 3   64 leaves of 324 rows
  A32  128^2, 32, 3   64 leaves of 256 rows, blocks of 32    C64  128^2, 64, 3   64 leaves, blocks of 64 (no k_parent_front)
  S     80^2, 16, 3   64 leaves of 100 rows (< 128: leaf_solve_ok and leaf_resident are off)
  T16   64^2, 16, 2   16 leaves of 256 rows                  A4   128^2, 16, 4   256 leaves of 64 rows (the sharded cells: 64 per rank)
  H    256^2, 64, 5   1024 leaves of 64 rows: the deep 64-wide tree (PassPath::Hi)
"""
import numpy as np

import test_gpu_likelihood_masks as MK

TREES = {"A": (128, 16, 3), "A32": (128, 32, 3), "B": (144, 16, 3), "C64": (128, 64, 3), "S": (80, 16, 3), "T16": (64, 16, 2),
         "A4": (128, 16, 4), "H": (256, 64, 5)}

# options a cell may set, with the library's defaults (every cell starts from these)
DEFAULTS = {2: 1, 3: 1, 4: 1, 6: 1, 7: 2, 8: 1, 10: 2, 11: 1, 13: 1, 16: 1, 17: 1}

# ---- masks ------------------------------------------------------------------------------------------------------------------------
# exact observation counts around every leaf-size threshold of the predictive side: the 16-row tile (15 / 16 / 17), 4 tiles
# (63 / 64 / 65: k_predict_hi's fold, k_leaf_gemm), 8 tiles (127 / 128 / 129: fused row solve, k_leaf_solve_update, k_chol_tiles<8>),
# 9 and 10 tiles (144, 159 / 160 / 161: k_chol_tiles<10>), 11 and 12 tiles (176, 191 / 192: k_chol_wave, LEAF_MAX_TILES)
EDGE_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 144, 159, 160, 161, 176, 191, 192)


def leaf_capacity(topo):
    return min(len(MK._leaf_callers(topo, i)) for i in np.nonzero(topo.node_leaf)[0])


def edge_counts_in_leaf_order(topo, variant, top):
    """{leaf position: count}: ``EDGE_COUNTS`` (those a leaf of this tree can hold, and a fully observed leaf where it cannot hold 192;
    the largest one replaced by ``top`` when that is larger) over the leaves, small and large counts alternating in leaf order.
    variant "empty_first": the first leaf is the empty one and the last leaf the largest; "empty_last": the other way round."""
    cap = leaf_capacity(topo)
    counts = sorted(set(c for c in EDGE_COUNTS if c <= cap) | ({cap} if cap < max(EDGE_COUNTS) else set()))
    if top is not None and top > counts[-1]:
        assert top <= cap
        counts[-1] = top
    nl = int(np.count_nonzero(topo.node_leaf))
    mid = counts[1:-1]
    h = (len(mid) + 1) // 2
    small, large = mid[:h], mid[h:][::-1]
    inter = [c for pair in zip(small, large + [None]) for c in pair if c is not None]
    assert sorted(inter) == mid and len(mid) + 2 <= nl
    stride = (nl - 2) // len(mid)
    assert stride >= 2                      # a thinned leaf between any two exact ones
    where = {1 + k * stride: c for k, c in enumerate(inter)}
    ends = (counts[0], counts[-1]) if variant == "empty_first" else (counts[-1], counts[0])
    assert variant in ("empty_first", "empty_last")
    where[0], where[nl - 1] = ends
    return where


def edge_mask(topo, variant, top=None, seed=0):
    """40 % thinning, then the exact counts of ``edge_counts_in_leaf_order``."""
    rng = np.random.RandomState(seed)
    obs = rng.uniform(size=topo.N) < 0.4
    leaves = [int(i) for i in np.nonzero(topo.node_leaf)[0]]
    where = edge_counts_in_leaf_order(topo, variant, top)
    for pos, c in where.items():
        MK._exact(obs, topo, leaves[pos], c, rng)
    return obs


def make_obs(topo, locs, recipe):
    kind = recipe[0]
    if kind == "pattern":                    # a pattern of tests/test_gpu_likelihood_masks.py (40 % thinning outside its gaps)
        return MK.make_mask(topo, locs, recipe[1])
    if kind == "empty_shard":                # ... with the whole first level-1 subtree unobserved: rank 0 of a 4-way run sees no observation
        obs = MK.make_mask(topo, locs, "first_child")
        obs[MK._leaf_callers(topo, int(topo.level_ptr[1]))] = False
        return obs
    if kind == "edges":
        return edge_mask(topo, recipe[1], recipe[2] if len(recipe) > 2 else None)
    raise ValueError(recipe)


def tiles(counts):
    return (np.asarray(counts) + 15) // 16


# ---- the table --------------------------------------------------------------------------------------------------------------------
def cell(tree, mask, predict, opts, ntl, **expect):
    """ntl: observation tiles of the largest leaf, the precondition the expectation was derived from (asserted from the mask)."""
    return dict(tree=tree, mask=mask, predict=predict, opts=tuple(opts), ntl=ntl, world=None, expect=expect)


CLOUD = ("pattern", "cloud")
E192 = ("edges", "empty_first")
E193 = ("edges", "empty_first", 193)

# what a default predictive pass of a regular tree with leaves of >= 128 rows and at most 8 observation tiles shows
FUSED8 = dict(path="Fused", chol="TilesSplit", c_fix="Phantom", var="None", update="SolveHalves", solve_fused=True, leaf_resident=True,
              scatter_ut=False, lik_rows=False, lik_general=False, side=False, acc_var=False, extract_mean=False)

CELLS = [
    # -- A, at most 8 tiles per leaf (40 % of 256 rows): every leaf "small"; ntl >= 5 and n_chol_small == n_leaves -> TilesSplit
    cell("A", CLOUD, True, (), 8, parent_front=True, **FUSED8),
    cell("A", CLOUD, False, (), 8, path="Fused", chol="TilesSplit", c_fix="InProduct", var="None", update="None", solve_fused=False,
         lik_rows=True, lik_general=False, c_only=True),
    cell("A", CLOUD, True, ((10, 1),), 8, **dict(FUSED8, update="SolveWhole")),
    cell("A", CLOUD, True, ((7, 0),), 8, **dict(FUSED8, update="InCascade", solve_fused=False)),
    cell("A", CLOUD, True, ((7, 0), (8, 0)), 8, **dict(FUSED8, update="Gemm", solve_fused=False)),
    cell("A", CLOUD, True, ((7, 0), (8, 0), (6, 2)), 8, **dict(FUSED8, update="LeafGemm", solve_fused=False)),
    cell("A", CLOUD, True, ((6, 0),), 8, **dict(FUSED8, leaf_resident=False)),
    cell("A", CLOUD, True, ((13, 0),), 8, **dict(FUSED8, scatter_ut=True)),
    cell("A", CLOUD, True, ((11, 0),), 8, **dict(FUSED8, chol="Wave")),
    # MRA_OPT_FUSED off: level-by-level kernels; every leaf <= 12 tiles and every block <= 192 wide -> the row solves accumulate the variance
    cell("A", CLOUD, True, ((2, 0),), 8, path="Levels", chol="TilesSplit", c_fix="Phantom", var="FinishVar", update="Gemm", solve_fused=False,
         acc_var=True, extract_mean=True, lik_rows=False),
    cell("A", CLOUD, False, ((2, 0),), 8, path="Levels", chol="TilesSplit", c_fix="InProduct", var="None", update="None", lik_rows=False,
         lik_general=True),
    cell("T16", CLOUD, True, (), 8, parent_front=True, **FUSED8),
    # -- B (40 % of 324 rows: 9 and 10 tiles beside <= 8): not all leaves small, 64 leaves <= 2 n_cu -> one k_chol_tiles<10,4> launch
    cell("B", CLOUD, True, (), 10, **dict(FUSED8, chol="TilesOne")),
    cell("B", CLOUD, True, ((11, 0),), 10, **dict(FUSED8, chol="Wave")),
    # -- 11 and 12 tiles: k_chol_wave whatever option 11 says; one leaf of 193: right-looking panels, k_leaf_fill, k_leaf_moments
    cell("A", E192, True, (), 12, **dict(FUSED8, chol="Wave")),
    cell("A", E192, True, ((11, 2),), 12, **dict(FUSED8, chol="Wave")),
    cell("A", E193, True, (), 13, **dict(FUSED8, chol="BigPanels", c_fix="Fill", var="Moments", update="Gemm", solve_fused=False)),
    cell("A", E193, False, (), 13, path="Fused", chol="BigPanels", c_fix="Fill", var="None", update="None", c_only=False, lik_rows=False),
    # -- S: leaves of 100 rows -> no k_leaf_solve_update, no fold into the cascade, no k_leaf_gemm
    cell("S", CLOUD, True, (), 4, **dict(FUSED8, update="Gemm", solve_fused=False, leaf_resident=False)),
    cell("S", E192, True, (), 7, **dict(FUSED8, update="Gemm", solve_fused=False, leaf_resident=False)),
    # -- blocks of 64: the parents' fronts (13 x 13 tiles) exceed k_parent_front
    cell("C64", CLOUD, True, (), 8, parent_front=False, **FUSED8),
    # -- H, the deep 64-wide tree (1024 leaves > 2 n_cu, at most 3 tiles each: one wave per leaf unless option 11 = 2).  Its leaves hold
    # 64 rows, so "one leaf of 65 - 80 observations" cannot be built on it; option 16 = 0 is what takes the update out of k_predict_hi here
    cell("H", CLOUD, True, (), 3, path="Hi", chol="Wave", c_fix="Phantom", var="FinishVar", update="InPredictHi", solve_fused=False,
         leaf_resident=False, acc_var=True, parent_front=False, extract_mean=False),
    cell("H", CLOUD, True, ((16, 0),), 3, path="Hi", chol="Wave", c_fix="Phantom", var="FinishVar", update="Gemm", solve_fused=False),
    cell("H", CLOUD, True, ((11, 2),), 3, path="Hi", chol="TilesSplit", c_fix="Phantom", var="FinishVar", update="InPredictHi"),
    cell("H", CLOUD, False, (), 3, path="Hi", chol="Wave", c_fix="InProduct", var="None", update="None", lik_general=True, lik_rows=False),
]

# sharded cells (4 ranks emulated on one GPU, tests/_cases.py): expect is per rank; the predict-only leaf work goes to the side stream
SHARDED = [
    dict(tree="A4", mask=CLOUD, predict=True, opts=(), world=4, ntl=2,
         expect=[dict(path="Fused", side=True, c_fix="Phantom", var="None", solve_fused=False, update="Gemm")] * 4),
    dict(tree="A4", mask=("empty_shard",), predict=False, opts=(), world=4, ntl=2,
         expect=[dict(path="Fused", side=False, c_fix="None", update="None")] + [dict(path="Fused", side=False, c_fix="InProduct", update="None")] * 3),
]

# ---- leaf-size edges: the option tuples that move leaves between kernels, and what route() must show for each -------------------
# (options, took effect?, route fields that differ from the mask's default route).  "fit": the largest leaf has 11 or 12 tiles, leaves
# on both sides of the 8-tile split, leaves of >= 128 rows (trees A, A32, B).  Default route there: FUSED8 with chol = Wave.
OPTION_CASES_FIT = [
    (((7, 0),), True, dict(solve_fused=False, update="InCascade")),
    (((7, 1),), True, dict()),                                                  # "always": what the default (64 leaves <= 2 n_cu) already does
    (((7, 2),), True, dict()),
    (((8, 0),), False, dict()),                                                 # overridden: k_leaf_solve_update carries the update
    (((8, 1),), True, dict()),
    (((7, 0), (8, 0)), True, dict(solve_fused=False, update="Gemm")),
    (((10, 1),), True, dict(update="SolveWhole")),
    (((10, 2),), True, dict()),
    (((11, 0),), True, dict()),                                                 # k_chol_wave either way
    (((11, 1),), True, dict()),
    (((11, 2),), False, dict()),                                                # overridden: k_chol_tiles takes at most 10 tiles
    (((13, 0),), True, dict(scatter_ut=True)),
    (((13, 1),), True, dict()),
    (((6, 0),), True, dict(leaf_resident=False)),
    (((6, 1),), True, dict()),
    (((6, 2),), False, dict()),                                                 # overridden for the update (k_leaf_solve_update has it)
    (((6, 2), (7, 0), (8, 0)), True, dict(solve_fused=False, update="LeafGemm")),
]
FIT_DEFAULT = dict(FUSED8, chol="Wave")
# "big": one leaf of 193 or 208 observations.  Nothing fits k_chol_wave / the LDS row solve: options 7, 8, 10, 11 and 13 are all overridden
BIG_DEFAULT = dict(FUSED8, chol="BigPanels", c_fix="Fill", var="Moments", update="Gemm", solve_fused=False)
OPTION_CASES_BIG = [
    (((7, 0),), False, dict()), (((7, 1),), False, dict()), (((7, 2),), False, dict()),
    (((8, 0),), False, dict()), (((8, 1),), False, dict()),
    (((10, 1),), False, dict()), (((10, 2),), False, dict()),
    (((11, 0),), False, dict()), (((11, 1),), False, dict()), (((11, 2),), False, dict()),
    (((13, 0),), False, dict()), (((13, 1),), False, dict()),
    (((6, 0),), True, dict(leaf_resident=False)),
    (((6, 1),), True, dict()),
    (((6, 2),), True, dict(update="LeafGemm")),
]
# "small": tree S (100 rows per leaf, at most 7 tiles, all leaves small): options 6, 7, 8 and 10 are overridden by the leaf size
SMALL_DEFAULT = dict(FUSED8, update="Gemm", solve_fused=False, leaf_resident=False)
OPTION_CASES_SMALL = [
    (((7, 0),), False, dict()), (((7, 1),), False, dict()), (((7, 2),), False, dict()),
    (((8, 0),), False, dict()), (((8, 1),), False, dict()),
    (((10, 1),), False, dict()), (((10, 2),), False, dict()),
    (((11, 0),), True, dict(chol="Wave")), (((11, 1),), True, dict()), (((11, 2),), True, dict()),
    (((13, 0),), True, dict(scatter_ut=True)), (((13, 1),), True, dict()),
    (((6, 0),), False, dict()), (((6, 1),), False, dict()), (((6, 2),), False, dict()),
]

# (tree, mask recipe, class, largest count)
EDGE_MASKS = [(t, ("edges", v) + ((top,) if top else ()), cls, top or 192)
              for t in ("A", "A32", "B")
              for v, top, cls in (("empty_first", None, "fit"), ("empty_last", None, "fit"), ("empty_first", 193, "big"), ("empty_last", 208, "big"))]
EDGE_MASKS += [("S", ("edges", "empty_first"), "small", 100), ("S", ("edges", "empty_last"), "small", 100)]
EDGE_CLASSES = {"fit": (FIT_DEFAULT, OPTION_CASES_FIT), "big": (BIG_DEFAULT, OPTION_CASES_BIG), "small": (SMALL_DEFAULT, OPTION_CASES_SMALL)}


def all_expected_routes():
    """Every expected route of the table, as (label, dict)."""
    out = [("%s %s predict=%s %s" % (c["tree"], c["mask"], c["predict"], c["opts"]), c["expect"]) for c in CELLS]
    for c in SHARDED:
        out += [("%s %s world %d rank %d" % (c["tree"], c["mask"], c["world"], k), e) for k, e in enumerate(c["expect"])]
    for t, m, cls, _ in EDGE_MASKS:
        base, cases = EDGE_CLASSES[cls]
        out.append(("%s %s default" % (t, m), base))
        out += [("%s %s %s" % (t, m, o), dict(base, **diff)) for o, _, diff in cases]
    return out
