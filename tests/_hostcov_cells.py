"""The host-evaluated covariance path (MRA_KERNEL_HOST): covariances, trees, masks and the route table of tests/test_gpu_hostcov.py
(asserted on a GPU) and tests/test_hostcov_table.py (its coverage, the block builder and the margin of the bars, on the CPU).

Covariances no KernelSpec can express - a positive variance field times a stationary kernel of an injectively warped coordinate,
positive semi-definite by construction - so that C(x,x) varies from row to row (covdiag) and equal Euclidean distances give
different values (block strides, row / column order):
  cov2(a, b) = s(a) s(b) (1 + t) exp(-t),  t = sqrt(3) |A (a - b)| / l,  A = [[1, 0], [0.6, 2]],  s(x) = 1 + 0.3 sin(3 x0) cos(2 x1),  l = 0.22
  cov1(a, b) = s(a) s(b) exp(-|w(a) - w(b)| / 0.3),  w(x) = x + 0.15 sin 4x (w' >= 0.4),  s(x) = 1 + 0.3 cos 5x
Every value is an elementwise function of its own pair of locations (no matrix product), so a pair has the same bits in whatever
block it is asked for, and cov(a, b) == cov(b, a) to the bit.

Trees:
  S     80^2, 16, 3   leaves of 100 rows: leaf_resident off, k_gemm_nt_lds<HOSTCOV> (k_gemm_nt<HOSTCOV> under option 3 = 0) on the leaves
  A    128^2, 16, 3   leaves of 256 rows: leaf_resident on, k_leaf_gemm<HOSTCOV, D, 0, 2, 7, 256, 2>; edge masks with a largest leaf
                      of 160, 192 and 193 observations (k_chol_tiles<10> in one launch, k_chol_wave, the big panels)
  C64  128^2, 64, 3   64-wide level blocks on the four-launch prior
  W200  64^2, r0 200, M 1, 8 % observed: cw 208 with 8 phantom knot columns; no variance on the way, k_leaf_moments reads covdiag
  T1   golden case t1000 (1-D, r 2, J 3, M 4) with cov1: the DIM = 1 instantiations, 1-D terciles, cw 16 with 2 real knots

A cell is (tree, mask recipe, predict, option tuple) -> the PassRoute fields the pass must show.  The expectations are written down
from ``route_for`` (pymra_amd/csrc/mra_plan.hip) with host_cov = true, not read back from a run: path_of gives Levels; prior_level
and c_only carry ``!host_cov``, so lik_rows and lik_general (which need c_only) are off and a likelihood-only pass still forms V[S,o]
and fixes C's phantom rows (c_fix Phantom, Fill beyond 12 tiles) instead of writing C in the product; acc_var = fit and every level
at most 12 tiles wide; var = FinishVar with acc_var, else Moments; update = LeafGemm with leaf_resident under option 6 = 2, else Gemm.
"""
import functools

import numpy as np

import _cases as K
import _route_cells as RC
import test_gpu_likelihood_masks as MK

# ---- covariances ------------------------------------------------------------------------------------------------------------------
L2 = 0.22


def _s2(x):
    return 1.0 + 0.3 * np.sin(3.0 * x[:, 0]) * np.cos(2.0 * x[:, 1])


def cov2(a, b, l=L2):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d0 = a[:, None, 0] - b[None, :, 0]
    d1 = a[:, None, 1] - b[None, :, 1]
    u1 = 0.6 * d0 + 2.0 * d1
    t = np.sqrt(3.0) * np.sqrt(d0 * d0 + u1 * u1) / l
    return (_s2(a)[:, None] * _s2(b)[None, :]) * ((1.0 + t) * np.exp(-t))


def cov2_at(l):
    """cov2 at another length scale (what an MLE over a callable uploads next)."""
    return lambda a, b: cov2(a, b, l)


def _w1(x):
    return x + 0.15 * np.sin(4.0 * x)


def _s1(x):
    return 1.0 + 0.3 * np.cos(5.0 * x)


def cov1(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return (_s1(a)[:, None] * _s1(b)[None, :]) * np.exp(-np.abs(_w1(a)[:, None] - _w1(b)[None, :]) / 0.3)


def one_ulp(cov):
    """``cov`` with every value moved by one ulp, up or down by a hash of the value's own bits: the same pair of locations gets the
    same moved value wherever it is asked for (and cov(a, b) == cov(b, a) stays true)."""
    def moved(a, b):
        v = np.ascontiguousarray(cov(a, b), dtype=np.float64)
        h = (v.view(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(63)
        return np.nextafter(v, np.where(h == 1, np.inf, -np.inf))
    return moved


# ---- trees and masks --------------------------------------------------------------------------------------------------------------
TREES = ("S", "A", "C64", "W200", "T1")
W200 = (64, 64, 200, 1, 0.08)                   # nx, ny, r0, M, observed fraction (tests/test_gpu_routes.py WIDE["r200_M1_sparse"])

CLOUD = ("pattern", "cloud")
FAMILIES = ("pattern", "two_families")
HEDGE = ("host_edges",)
HEDGE193 = ("host_edges", 193)
HEDGE160 = ("host_edges", 160)                  # the counts up to 160 only: a largest leaf of 10 tiles
SPARSE = ("fraction", W200[4])
GOLDEN = ("golden",)

# RC.EDGE_COUNTS and the boundaries of k_leaf_gemm<HOSTCOV>'s seven column tiles: 6 / 7 tiles (96 / 97), exactly seven - one column
# pass - (112) and seven plus one - the second pass, j0 += CT - (113)
HOST_EDGE_COUNTS = tuple(sorted(set(RC.EDGE_COUNTS) | {96, 97, 112, 113}))


@functools.lru_cache(maxsize=None)
def tree(key):
    """(topo, locs, cov, R) of a tree."""
    if key == "T1":
        cs = K.load_case("t1000")
        return cs["topo"], cs["locs"], cov1, float(cs["c"]["R"])
    if key == "W200":
        import pymra_amd.MRATools as mt
        from pymra_amd.topology import build_topology
        nx, ny, r, M, _ = W200
        np.random.seed(13)
        locs = mt.genLocations2d(Nx=nx, Ny=ny)
        return build_topology(locs, r, M, 4), locs, cov2, MK.R
    topo, locs = MK._tree(*RC.TREES[key])
    return topo, locs, cov2, MK.R


def host_edge_counts_in_leaf_order(topo, top=None):
    """{leaf position: count} as RC.edge_counts_in_leaf_order's "empty_first" does it, for HOST_EDGE_COUNTS: the first leaf empty, the
    last leaf the largest (``top`` in place of 192 when larger; the counts up to ``top`` only when smaller), small and large counts
    alternating in between."""
    counts = [c for c in HOST_EDGE_COUNTS if top is None or top > HOST_EDGE_COUNTS[-1] or c <= top]
    assert RC.leaf_capacity(topo) >= (top or counts[-1])
    if top is not None:
        assert top >= counts[-1]
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
    where[0], where[nl - 1] = counts[0], counts[-1]
    return where


def make_obs(key, recipe, seed=0):
    """(obs mask bool[N], y (N, 1) with NaN where unobserved)."""
    topo, locs, _, _ = tree(key)
    kind = recipe[0]
    if kind == "golden":
        y = np.asarray(K.load_case("t1000")["y_obs"], dtype=np.float64).reshape(-1, 1)
        return np.isfinite(y.ravel()), y
    if kind == "fraction":
        rng = np.random.RandomState(31 + seed)
        y = np.where(rng.uniform(size=(topo.N, 1)) < recipe[1], rng.normal(size=(topo.N, 1)), np.nan)
        return np.isfinite(y.ravel()), y
    if kind == "pattern":
        obs = MK.make_mask(topo, locs, recipe[1], seed=seed)
    elif kind == "host_edges":
        rng = np.random.RandomState(seed)
        obs = rng.uniform(size=topo.N) < 0.4
        leaves = [int(i) for i in np.nonzero(topo.node_leaf)[0]]
        for pos, c in host_edge_counts_in_leaf_order(topo, recipe[1] if len(recipe) > 1 else None).items():
            MK._exact(obs, topo, leaves[pos], c, rng)
    else:
        raise ValueError(recipe)
    return obs, MK._y(obs)


@functools.lru_cache(maxsize=None)
def case(key, recipe):
    """(topo, locs, cov, R, y, leaf counts) of one (tree, mask)."""
    topo, locs, cov, R = tree(key)
    obs, y = make_obs(key, recipe)
    return topo, locs, cov, R, y, MK.leaf_counts(topo, obs)


@functools.lru_cache(maxsize=None)
def oracle(key, recipe):
    """run_levelwise with the callable, once per (tree, mask) for every test of the process; nobody writes into it."""
    from oracle.mra_levelwise import run_levelwise
    topo, locs, cov, R, y, _ = case(key, recipe)
    return run_levelwise(topo, locs, cov, y, R)


# ---- the table --------------------------------------------------------------------------------------------------------------------
HOST = dict(path="Levels", prior_level=False, c_only=False, lik_rows=False, lik_general=False)


def cell(tree, mask, predict, opts, ntl, **expect):
    """ntl: observation tiles of the largest leaf, the precondition the expectation was derived from (asserted from the mask)."""
    e = dict(HOST, extract_mean=predict, **expect)
    if not predict:
        e.update(var="None", update="None")
    else:
        e.setdefault("update", "Gemm")
    return dict(tree=tree, mask=mask, predict=predict, opts=tuple(opts), ntl=ntl, expect=e)


GEMM_DIRECT = ((3, 0),)                 # MRA_OPT_GEMM_LDS off: k_gemm_nt<HOSTCOV> wherever launch_gemm<EPI_HOSTCOV> runs
# leaves of 100 rows: never leaf_resident; all leaves at most 8 tiles and 64 leaves <= 2 n_cu -> k_chol_tiles in two launches
SMALL = dict(leaf_resident=False, acc_var=True, c_fix="Phantom", chol="TilesSplit")
# A with leaves of up to 192 observations (12 tiles > 10): k_chol_wave; every level 16 wide and every leaf fits -> variance on the way
EDGE = dict(leaf_resident=True, acc_var=True, c_fix="Phantom", chol="Wave")
# leaves of up to 160 observations (10 tiles, not all within 8) and 64 leaves <= 2 n_cu: k_chol_tiles<10> in one launch
TEN = dict(leaf_resident=True, acc_var=True, c_fix="Phantom", chol="TilesOne")
# one leaf of 193 (13 tiles): nothing fits the LDS row solve
BIG = dict(leaf_resident=True, acc_var=False, c_fix="Fill", chol="BigPanels")
# 64-wide blocks (4 tiles <= 12), leaves of at most 8 tiles
WIDE64 = dict(leaf_resident=True, acc_var=True, c_fix="Phantom", chol="TilesSplit")
# 208-wide blocks (13 tiles > 12): no variance on the way; 4 leaves of at most 7 tiles
WIDE208 = dict(leaf_resident=True, acc_var=False, c_fix="Phantom", chol="TilesSplit")
# 81 leaves of about 12 rows, one tile each
ONE_D = dict(leaf_resident=False, acc_var=True, c_fix="Phantom", chol="TilesSplit")

CELLS = [
    cell("S", CLOUD, True, (), 4, var="FinishVar", **SMALL),
    cell("S", CLOUD, True, GEMM_DIRECT, 4, var="FinishVar", **SMALL),
    cell("S", CLOUD, False, (), 4, **SMALL),
    cell("S", FAMILIES, True, (), 4, var="FinishVar", **SMALL),
    cell("S", FAMILIES, True, GEMM_DIRECT, 4, var="FinishVar", **SMALL),
    cell("S", FAMILIES, False, (), 4, **SMALL),
    cell("A", CLOUD, True, (), 8, var="FinishVar", **dict(EDGE, chol="TilesSplit")),
    cell("A", CLOUD, False, GEMM_DIRECT, 8, **dict(EDGE, chol="TilesSplit")),
    cell("A", HEDGE, True, (), 12, var="FinishVar", **EDGE),
    cell("A", HEDGE, True, ((6, 0),), 12, var="FinishVar", **dict(EDGE, leaf_resident=False)),
    cell("A", HEDGE, True, GEMM_DIRECT, 12, var="FinishVar", **EDGE),
    cell("A", HEDGE, True, ((6, 0), (3, 0)), 12, var="FinishVar", **dict(EDGE, leaf_resident=False)),
    cell("A", HEDGE, True, ((6, 2),), 12, var="FinishVar", update="LeafGemm", **EDGE),
    cell("A", HEDGE, False, (), 12, **EDGE),
    cell("A", HEDGE160, True, (), 10, var="FinishVar", **TEN),
    cell("A", HEDGE160, True, ((6, 0), (3, 0)), 10, var="FinishVar", **dict(TEN, leaf_resident=False)),
    cell("A", HEDGE193, True, (), 13, var="Moments", **BIG),
    cell("A", HEDGE193, True, GEMM_DIRECT, 13, var="Moments", **BIG),
    cell("A", HEDGE193, False, (), 13, **BIG),
    cell("C64", CLOUD, True, (), 8, var="FinishVar", **WIDE64),
    cell("C64", CLOUD, True, GEMM_DIRECT, 8, var="FinishVar", **WIDE64),
    cell("C64", CLOUD, False, (), 8, **WIDE64),
    cell("W200", SPARSE, True, (), 7, var="Moments", **WIDE208),
    cell("W200", SPARSE, True, GEMM_DIRECT, 7, var="Moments", **WIDE208),
    cell("W200", SPARSE, False, (), 7, **WIDE208),
    cell("T1", GOLDEN, True, (), 1, var="FinishVar", **ONE_D),
    cell("T1", GOLDEN, True, GEMM_DIRECT, 1, var="FinishVar", **ONE_D),
    cell("T1", GOLDEN, False, (), 1, **ONE_D),
]

GROUPS = sorted(set((c["tree"], c["mask"]) for c in CELLS), key=lambda g: (TREES.index(g[0]), g[1]))

# what a 4-way rank of S shows: the host route, its predict-only leaf work on the side stream
SHARDED = dict(tree="S", mask=CLOUD, world=4, expect=dict(HOST, side=True, extract_mean=True, var="FinishVar", update="Gemm", **SMALL))


def all_expected_routes():
    """Every expected route of the host table with the value of MRA_OPT_GEMM_LDS it ran under, as (label, dict)."""
    out = []
    for c in CELLS:
        e = dict(c["expect"], predict=c["predict"], gemm_lds=dict(c["opts"]).get(3, RC.DEFAULTS[3]))
        out.append(("%s %s predict=%s %s" % (c["tree"], c["mask"], c["predict"], c["opts"]), e))
    return out
