"""1-D problems at real block widths: the trees, data, masks and expected routes of tests/test_gpu_line.py (asserted on a GPU) and
tests/test_line_cells_cpu.py (their shapes, counts, coverage and conditioning, on the CPU).

A 1-D tree is ternary whatever J is passed: its leaves sit on the last level and every non-leaf node holds exactly r0 knots, so the
tree is ``regular`` (classify_shape, pymra_amd/csrc/mra_plan.hip) and a pass takes PassPath::Fused, or PassPath::Hi for 64-wide blocks
on five or more non-leaf levels.  Trees (mt.genLocations(N), np.random.seed(7), build_topology(locs, r0, M, 3)):

  name   N, r0, M        nodes per level           cw   padded leaf rows
  L16    2048, 16, 2     1 3 9                     16   224 - 240
  L16s   2048, 16, 3     1 3 9 27                  16   80 - 96      (< 128: leaf_solve_ok and leaf_resident are off)
  L16d   4096, 16, 2     1 3 9                     16   448 - 480    (one location dropped by the partition)
  L32    8192, 32, 3     1 3 9 27                  32   304 - 336
  L64    4096, 64, 2     1 3 9                     64   448 - 480    (one location dropped)
  L64x   8192, 64, 4     1 3 9 27 81               64   112          CWT 4 on four levels: the row cascade's operands take 136 tiles
                                                                     against the 80 of the LDS (cascade_lds_all), it stages level by level
  LH     16384, 64, 5    1 3 9 27 81 243           64   64 - 80      PassPath::Hi; at most 64 padded observations per leaf
  L32x   73728, 32, 7    1 3 ... 2187              32   32 - 48      CWT 2 on seven levels: 105 tiles against 80
  LE     24576, 16, 4    1 3 9 27 81               16   304 - 336    every leaf holds at least 208 real rows (the leaf-size edges)

Expected routes are written down from ``route_for`` (mra_plan.hip), not read back from a run; each states the preconditions it was
derived from (the largest leaf's observation tiles ``ntl``, the leaves' rows), which the tests assert from the mask.  route_for
counts leaves against ``2 * n_cu``; every tree but L32x has at most 243 leaves, below n_cu on an MI355X - the GPU test asserts it.
"""
import functools

import numpy as np

import _route_cells as RC
import test_gpu_likelihood_masks as MK

R = 1e-2

# name: (N, r0, M)
TREES = {"L16": (2048, 16, 2), "L16s": (2048, 16, 3), "L16d": (4096, 16, 2), "L32": (8192, 32, 3), "L64": (4096, 64, 2),
         "L64x": (8192, 64, 4), "LH": (16384, 64, 5), "L32x": (73728, 32, 7), "LE": (24576, 16, 4)}
# name: (nodes per level, cw, fewest and most padded rows of a leaf, locations the partition drops)
SHAPES = {"L16": ([1, 3, 9], 16, 224, 240, 0), "L16s": ([1, 3, 9, 27], 16, 80, 96, 0), "L16d": ([1, 3, 9], 16, 448, 480, 1),
          "L32": ([1, 3, 9, 27], 32, 304, 336, 0), "L64": ([1, 3, 9], 64, 448, 480, 1), "L64x": ([1, 3, 9, 27, 81], 64, 112, 112, 0),
          "LH": ([1, 3, 9, 27, 81, 243], 64, 64, 80, 0), "L32x": ([3 ** k for k in range(8)], 32, 32, 48, 538),
          "LE": ([1, 3, 9, 27, 81], 16, 304, 336, 0)}


def _families():
    import pymra_amd.MRATools as mt
    return {"exp": mt.KernelSpec(mt.KIND_EXP, 0.02), "m32": mt.KernelSpec(mt.KIND_MATERN32, 0.02),
            "m52": mt.KernelSpec(mt.KIND_MATERN52, 0.02), "gauss": mt.KernelSpec(mt.KIND_GAUSSIAN, 0.01),
            "kanter": mt.KernelSpec(mt.KIND_KANTER, 0.05), "iden": mt.KernelSpec(mt.KIND_IDEN, 1.0),
            "exp_circular": mt.KernelSpec(mt.KIND_EXP, 0.02, circular=True)}


FAMILIES = _families()
M32 = FAMILIES["m32"]
# one family per MODE of the 1-D kernel dispatch beside Matern32 (MODE 0: Exp and the Materns; Gaussian, Iden and Kanter have their own)
MODE_FAMILIES = ("m32", "gauss", "iden", "kanter")
# mra_sample factors the leaves' prior covariance with no noise on it.  For a Gaussian kernel on points 1 / 2048 apart that matrix is
# singular in float64 from l = 0.0015 on (LAPACK refuses it as well, tests/test_line_cells_cpu.py); at l = 0.001 its smallest
# eigenvalue is 1e-8
GAUSS_SAMPLE = type(FAMILIES["gauss"])(FAMILIES["gauss"].kind, 0.001)


@functools.lru_cache(maxsize=None)
def tree(key):
    """(topology, locations (N, 1))"""
    import pymra_amd.MRATools as mt
    from pymra_amd.topology import build_topology
    N, r0, M = TREES[key]
    np.random.seed(7)
    locs = mt.genLocations(N)
    return build_topology(locs, r0, M, 3), locs


def leaves(topo):
    return [int(i) for i in np.nonzero(topo.node_leaf)[0]]


def leaf_rows(topo):
    """padded rows of every leaf, in leaf order"""
    return np.asarray(topo.node_row1 - topo.node_row0)[np.asarray(topo.node_leaf, dtype=bool)]


def leaf_real_rows(topo):
    return np.array([len(MK._leaf_callers(topo, i)) for i in leaves(topo)])


def reported(topo):
    """bool[N]: locations that lie in a leaf (the partition may drop one at a boundary; mean and variance stay 0 there)"""
    rep = np.zeros(topo.N, dtype=bool)
    good = np.asarray(topo.in_leaf, dtype=bool) & (topo.perm >= 0)
    rep[topo.perm[good]] = True
    return rep


def values(locs, obs, seed=0):
    """a smooth function of x plus noise of variance R at the observed locations, NaN elsewhere"""
    x = np.asarray(locs, dtype=np.float64).ravel()
    f = np.sin(12.0 * x) + 0.5 * np.cos(31.0 * x + 1.0) + x
    noise = np.random.default_rng(seed + 100).standard_normal(len(x))
    return np.where(obs, f + np.sqrt(R) * noise, np.nan)


def default_mask(topo, seed=0):
    """40 % observed, the first leaf without any observation"""
    obs = np.random.default_rng(seed).random(topo.N) < 0.4
    obs[MK._leaf_callers(topo, leaves(topo)[0])] = False
    return obs


# ---- masks --------------------------------------------------------------------------------------------------------------------------
# ("default",): default_mask; ("pattern", name): MK.make_mask, 40 % thinning outside the gaps of a pattern of
# tests/test_gpu_likelihood_masks.py; ("edges", variant[, top]): RC.edge_mask, the exact counts of RC.EDGE_COUNTS
GAPPY = ("first_child", "first_two_alternate", "two_families", "last_child_only", "first_family_last_leaf", "one_leaf")


def make_obs(key, recipe):
    topo, locs = tree(key)
    if recipe[0] == "default":
        return default_mask(topo)
    if recipe[0] == "empty_shard":                   # the whole first level-1 subtree unobserved: rank 0 of a 3-way run sees no observation
        obs = default_mask(topo)
        obs[MK._leaf_callers(topo, int(topo.level_ptr[1]))] = False
        return obs
    if recipe[0] == "pattern":
        assert recipe[1] in GAPPY                    # ("cloud" is a rectangle in two coordinates)
        return MK.make_mask(topo, locs, recipe[1])
    if recipe[0] == "edges":
        return RC.edge_mask(topo, recipe[1], recipe[2] if len(recipe) > 2 else None)
    raise ValueError(recipe)


@functools.lru_cache(maxsize=None)
def problem(key, recipe=("default",)):
    """(topology, locations, observed mask, y (N,), observations per leaf)"""
    topo, locs = tree(key)
    obs = make_obs(key, recipe)
    return topo, locs, obs, values(locs, obs), MK.leaf_counts(topo, obs)


def ntl(counts):
    return int(RC.tiles(counts).max())


# ---- expected routes ----------------------------------------------------------------------------------------------------------------
# route_for, for a regular tree on one GPU (reduce_level < 0), device kernel, default options, nl leaves <= 2 n_cu:
#   fit = ntl <= 12.  chol: BigPanels if not fit; else (ntl <= 10 and option 11 = 1 and (ntl >= 5 or nl <= 2 n_cu), the latter always
#   true here) TilesSplit if every leaf has at most 8 tiles, TilesOne if not; Wave for ntl 11, 12 or option 11 = 0.
#   predictive: c_fix Phantom if fit else Fill; leaf_resident = leaf rows >= 128 and at least 64 padded observations in some leaf;
#   solve_fused = Fused and fit and leaf_solve_ok (leaf rows >= 128, na / 16 <= 13); update SolveHalves (option 10 = 2) with it,
#   else InCascade needs leaf_solve_ok too, so Gemm; var None on the fused path unless not fit (Moments).
#   likelihood only: c_only = fit; c_fix InProduct; lik_rows = Fused and c_only and cascade_stage_all (the cascade's operands in 160 KB).
#   MRA_OPT_FUSED 0: path Levels, acc_var = fit (every block <= 192 wide), var FinishVar, update Gemm, extract_mean; likelihood only
#   lik_general (every level's cw <= 64).
FUSED8 = RC.FUSED8                                                       # leaves of >= 128 rows, 5 <= ntl <= 8
SMALL = RC.SMALL_DEFAULT                                                 # leaves under 128 rows
LEVELS = dict(path="Levels", c_fix="Phantom", var="FinishVar", update="Gemm", solve_fused=False, acc_var=True, extract_mean=True,
              lik_rows=False)
LIK_FUSED = dict(path="Fused", c_fix="InProduct", var="None", update="None", solve_fused=False, lik_rows=True, lik_general=False, c_only=True)
LIK_LEVELS = dict(path="Levels", c_fix="InProduct", var="None", update="None", lik_rows=False, lik_general=True, c_only=True)
BIG = RC.BIG_DEFAULT                                                     # ntl >= 13
LIK_BIG = dict(path="Fused", chol="BigPanels", c_fix="Fill", var="None", update="None", c_only=False, lik_rows=False, lik_general=False)
LEVELS_BIG = dict(path="Levels", chol="BigPanels", c_fix="Fill", var="Moments", update="Gemm", solve_fused=False, acc_var=False,
                  extract_mean=True)
LIK_LEVELS_BIG = dict(path="Levels", chol="BigPanels", c_fix="Fill", var="None", update="None", c_only=False, lik_rows=False,
                      lik_general=False)
HI = dict(path="Hi", chol="TilesSplit", c_fix="Phantom", var="FinishVar", update="InPredictHi", solve_fused=False, leaf_resident=False,
          acc_var=True, parent_front=False, extract_mean=False)


def cell(tree, mask, predict, opts, ntl, rows_min, **expect):
    """ntl: observation tiles of the largest leaf; rows_min: fewest padded rows of a leaf - the preconditions the expectation was
    derived from (asserted from the mask and the tree).  ``n_chain_min`` in expect: route()["n_chain"] is at least that."""
    return dict(tree=tree, mask=mask, predict=predict, opts=tuple(opts), ntl=ntl, rows_min=rows_min, expect=expect)


DEFAULT = ("default",)
LEVELS_OFF = ((2, 0),)                                                   # MRA_OPT_FUSED 0
# nf of the leaves' parents = cw + (levels above them) * cw + 16: 48 (L16: 6 tiles), 112 (L32: 28 tiles) fit k_parent_front; 336 and 400
# (L64x, LH) are more than 256, kept as panels (lowrank_parent): no k_parent_front
CELLS = [
    # -- L16: 9 leaves of 224 - 240 rows, every leaf within 8 tiles; 3 nodes on level 1 <= n_cu: the knot chain covers both levels
    cell("L16", DEFAULT, True, (), 8, 224, parent_front=True, n_chain_min=2, **FUSED8),
    cell("L16", DEFAULT, False, (), 8, 224, chol="TilesSplit", **LIK_FUSED),
    cell("L16", DEFAULT, True, LEVELS_OFF, 8, 224, chol="TilesSplit", **LEVELS),
    cell("L16", DEFAULT, False, LEVELS_OFF, 8, 224, chol="TilesSplit", **LIK_LEVELS),
    # -- L16s: 27 leaves of 80 - 96 rows, at most 3 tiles (ntl < 5, but 27 leaves <= 2 n_cu: still k_chol_tiles)
    cell("L16s", DEFAULT, True, (), 3, 80, n_chain_min=2, **SMALL),
    cell("L16s", DEFAULT, False, (), 3, 80, chol="TilesSplit", **LIK_FUSED),
    cell("L16s", DEFAULT, True, LEVELS_OFF, 3, 80, chol="TilesSplit", **LEVELS),
    cell("L16s", DEFAULT, False, LEVELS_OFF, 3, 80, chol="TilesSplit", **LIK_LEVELS),
    # -- L16d, L64: 9 leaves of 448 - 480 rows; 40 % of them is 177 - 203 observations, 13 tiles: right-looking panels, k_leaf_fill, k_leaf_moments
    cell("L16d", DEFAULT, True, (), 13, 448, parent_front=True, n_chain_min=2, **BIG),
    cell("L16d", DEFAULT, False, (), 13, 448, **LIK_BIG),
    cell("L16d", DEFAULT, True, LEVELS_OFF, 13, 448, **LEVELS_BIG),
    cell("L16d", DEFAULT, False, LEVELS_OFF, 13, 448, **LIK_LEVELS_BIG),
    cell("L64", DEFAULT, True, (), 13, 448, n_chain_min=2, **BIG),
    cell("L64", DEFAULT, False, (), 13, 448, **LIK_BIG),
    cell("L64", DEFAULT, True, LEVELS_OFF, 13, 448, **LEVELS_BIG),
    cell("L64", DEFAULT, False, LEVELS_OFF, 13, 448, **LIK_LEVELS_BIG),
    # -- L32: 27 leaves of 304 - 336 rows, 9 and 10 tiles beside <= 8: one k_chol_tiles<10> launch
    cell("L32", DEFAULT, True, (), 10, 304, parent_front=True, n_chain_min=2, **dict(FUSED8, chol="TilesOne")),
    cell("L32", DEFAULT, False, (), 10, 304, chol="TilesOne", **LIK_FUSED),
    cell("L32", DEFAULT, True, LEVELS_OFF, 10, 304, chol="TilesOne", **LEVELS),
    cell("L32", DEFAULT, False, LEVELS_OFF, 10, 304, chol="TilesOne", **LIK_LEVELS),
    # -- L64x: leaves of 112 rows; neither the knot chain (78 operand tiles + its own) nor the stage-all row cascade fits the LDS
    cell("L64x", DEFAULT, True, (), 4, 112, parent_front=False, n_chain=0, **SMALL),
    cell("L64x", DEFAULT, False, (), 4, 112, chol="TilesSplit", **dict(LIK_FUSED, lik_rows=False)),
    # -- LH: 243 leaves (<= 2 n_cu: k_chol_tiles, unlike the 1024 leaves of the 2-D tree H) of at most 3 tiles; na = (5 * 4 + 1) * 16
    cell("LH", DEFAULT, True, (), 3, 64, **HI),
    cell("LH", DEFAULT, False, (), 3, 64, path="Hi", chol="TilesSplit", c_fix="InProduct", var="None", update="None", lik_general=True,
         lik_rows=False),
    # -- LE under the default mask: 81 leaves of 304 - 336 rows, 10 tiles at most
    cell("LE", DEFAULT, True, (), 10, 304, parent_front=True, **dict(FUSED8, chol="TilesOne")),
]

# three ranks of L16s (one level-1 subtree each, 9 leaves): the predict-only leaf work goes to the side stream; a rank whose subtree
# holds no observation has no C block to fix
SHARDED = [
    dict(tree="L16s", mask=DEFAULT, predict=True, world=3,
         expect=[dict(path="Fused", side=True, c_fix="Phantom", var="None", solve_fused=False, update="Gemm")] * 3),
    dict(tree="L16s", mask=("empty_shard",), predict=False, world=3,
         expect=[dict(path="Fused", side=False, c_fix="None", update="None")] + [dict(path="Fused", side=False, c_fix="InProduct", update="None")] * 2),
]

# the leaf-size edges on LE: (mask recipe, class of RC.EDGE_CLASSES, largest count).  Every leaf has at least 128 rows, so the "fit" and
# "big" option cases of tests/_route_cells.py apply as they stand (81 leaves <= 2 n_cu, na / 16 = 5 <= 13)
EDGE_MASKS = [(("edges", "empty_first"), "fit", 192), (("edges", "empty_last"), "fit", 192),
              (("edges", "empty_first", 193), "big", 193), (("edges", "empty_last", 208), "big", 208)]


def cells_of(tree, mask=DEFAULT):
    return [c for c in CELLS if c["tree"] == tree and c["mask"] == mask]


def find(tree, predict, opts=(), mask=DEFAULT):
    hit = [c for c in cells_of(tree, mask) if c["predict"] == predict and c["opts"] == tuple(opts)]
    assert len(hit) == 1, (tree, predict, opts)
    return hit[0]


def all_expected_routes():
    """Every expected route of this module, as (label, dict)."""
    out = [("%s %s predict=%s %s" % (c["tree"], c["mask"], c["predict"], c["opts"]), c["expect"]) for c in CELLS]
    for c in SHARDED:
        out += [("%s %s world %d rank %d" % (c["tree"], c["mask"], c["world"], k), e) for k, e in enumerate(c["expect"])]
    for m, cls, _ in EDGE_MASKS:
        base, cases = RC.EDGE_CLASSES[cls]
        out.append(("LE %s default" % (m,), base))
        out += [("LE %s %s" % (m, o), dict(base, **diff)) for o, _, diff in cases]
    return out
