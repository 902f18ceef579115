"""The tree and mask of tests/test_gpu_leaf_order.py, and of the recipe of its oracle fixture (tests/golden/make_leaf_order.py).

The leaf Cholesky is split in two launches (LeafChol::TilesSplit) beside oversized leaves only where a GPU sees more than two
leaves per compute unit, i.e. more than 512 on an MI355X: the smallest regular 2-D tree with that many leaves (4^5 = 1024) whose
leaves can hold more than 128 observations is the 384 x 384 grid with r0 = 16, M = 5 (144 rows per leaf).  The level-wise oracle
takes about 20 s on it, so its likelihood and its moments at SAMPLE rows are a fixture."""
import os

import numpy as np

import test_gpu_likelihood_masks as MK

TREE = (384, 16, 5)
R = MK.R
# leaf position (leaf order) -> exact observation count; every other leaf keeps the 40 % thinning (3 to 5 tiles).  An empty leaf,
# leaves of one tile (1, 15, 16), two tiles (17), seven (112), exactly eight (113, 128) and nine tiles (129, 137, 144 = every row)
# in three families; the first leaf (one observation) is the smallest, so no ordering is the identity.
EXACT = {0: 1, 1: 128, 2: 15, 5: 0, 6: 16, 7: 129, 10: 17, 11: 112, 500: 144, 700: 113, 1023: 137}
OVERSIZED = (7, 500, 1023)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "leaf_order.npz")


def build():
    """-> (topo, locs, obs mask (bool[N]), y_obs (N, 1) with NaN where unobserved)."""
    topo, locs = MK._tree(*TREE)
    rng = np.random.RandomState(0)
    obs = rng.uniform(size=topo.N) < 0.4
    leaves = [int(i) for i in np.nonzero(topo.node_leaf)[0]]
    for pos, c in sorted(EXACT.items()):
        MK._exact(obs, topo, leaves[pos], c, rng)
    return topo, locs, obs, MK._y(obs)


def sample_rows(topo):
    """Caller rows the fixture keeps: every row of the leaves with an exact count, and every 61st row of the grid."""
    leaves = [int(i) for i in np.nonzero(topo.node_leaf)[0]]
    rows = [MK._leaf_callers(topo, leaves[pos]) for pos in sorted(EXACT)] + [np.arange(0, topo.N, 61)]
    return np.unique(np.concatenate(rows))
