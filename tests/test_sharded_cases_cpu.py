"""The sharded case table (tests/_sharded_cases.py) against the CPU oracle alone: for every case and world, ``shard_topology``'s local
trees partition the reported rows, and the in-process emulation of all ranks through the level-wise oracle reproduces the unsharded
oracle.  This keeps the table and the index bookkeeping honest without a GPU, so that a disagreement in tests/test_gpu_sharded.py is
a finding about the device path.  Measured over the whole table: lik 4.7e-16 relative, mean 7.5e-14, var 1.9e-16 at worst - the
bounds here are two decades and more above that."""
import numpy as np
import pytest

import _cases as K
import _sharded_cases as SC


def test_the_table_reaches_what_it_names():
    from pymra_amd.sharding import choose_shard_level
    for cid, w in SC.CELLS:
        if cid != "deep":
            assert choose_shard_level(SC.problem(cid)["topo"], w) == SC.SHARD_LEVEL[cid, w], (cid, w)
    leaf_level = lambda cid: SC.problem(cid)["topo"].n_levels - 1
    # the leaf level as shard level: fused 2-D trees (one leaf per rank, and shares of 4, 3, 3, 3, 3 leaves), 1-D, J = 3 in 2-D, ragged
    for cid, w in [("g32", 5), ("g32", 16), ("c1", 10), ("t201", 10), ("u3", 9), ("rnd2", 16), ("rnd4", 16), ("rnd8", 16)] + \
                  [(c, 3) for c in ("m1-32-16", "m1-48-32", "m1-64-64")] + [("kat2", 2)]:
        assert SC.SHARD_LEVEL[cid, w] == leaf_level(cid), (cid, w)
    assert [int(SC.problem(c)["topo"].cw[0]) for c in ("m1-32-16", "m1-48-32", "m1-64-64")] == [16, 32, 64]
    assert [SC.problem("rnd%d" % s)["r"] for s in (2, 4, 6, 8)] == [8, 32, 20, 16]
    assert tuple(s for s in (2, 4, 6, 8) if SC.problem("rnd%d" % s)["M"] == 2) == SC.RND_M2_SEEDS
    assert [SC.problem("rnd%d" % s)["spec"].kind for s in (2, 4, 6, 8)] == [K.mt.KIND_MATERN52, K.mt.KIND_MATERN32, K.mt.KIND_MATERN32, K.mt.KIND_GAUSSIAN]
    for s in (2, 4, 6, 8):                      # ragged leaves
        t = SC.problem("rnd%d" % s)["topo"]
        assert len(set(len(SC.MK._leaf_callers(t, i)) for i in np.nonzero(t.node_leaf)[0])) > 1, s
    t = SC.problem("t201")["topo"]
    assert t.N - len(K.owned_rows(t)) == 2                                     # the rows a 1-D split drops
    assert [len(K.owned_rows(lt)) for lt, _ in SC.local_topologies(SC.problem("c1")["topo"], 2)] == [66, 34]       # subtrees 2 + 1
    # "empty": rank 0 of 4 owns no observation
    p = SC.problem("empty")
    own = [K.owned_rows(lt) for lt, _ in SC.local_topologies(p["topo"], 4)]
    nobs = [int(np.isfinite(p["y"].ravel()[rows]).sum()) for rows in own]
    assert nobs[0] == 0 and min(nobs[1:]) > 0, nobs


@pytest.mark.parametrize("cid,world", SC.CELLS, ids=SC.CELL_IDS)
def test_oracle_emulation_equals_the_unsharded_oracle(cid, world):
    p = SC.problem(cid)
    topo = p["topo"]
    locals_ = SC.local_topologies(topo, world)
    assert len(set(red for _, red in locals_)) == 1 and locals_[0][1] == SC.SHARD_LEVEL[cid, world] - 1
    SC.check_partition(topo, [lt for lt, _ in locals_])                        # A1
    if cid == "deep":
        return                                                                 # ten and twenty seconds of oracle: the GPU module holds the device to one run
    full = SC.oracle(cid)
    liks, mean, var, s = K.emulate_world_oracle(topo, p["locs"], p["y"], p["R"], p["spec"], world)
    assert s == SC.SHARD_LEVEL[cid, world] and len(liks) == world
    assert max(abs(l - full["lik"]) for l in liks) <= 1e-13 * abs(full["lik"])
    assert np.max(np.abs(mean - full["mean"])) < 1e-12
    assert np.max(np.abs(var - full["var"])) < 1e-13
