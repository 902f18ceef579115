"""The case table of the sharded tests (tests/test_gpu_sharded.py on the GPU, tests/test_sharded_cases_cpu.py on the oracle alone):
the smallest trees that reach each path of a sharded pass the other GPU tests leave out - the leaf level as shard level on the fused
path, 1-D trees with dropped rows and orphan knot rows of several levels, irregular 2-D trees, uneven rank shares, a rank without
any observation on a predictive pass, every device kernel family and the torus distance, and a deep 64-wide tree whose parent
fronts are kept as panels.  The truth of every case is the unsharded level-wise oracle on the full tree."""
import functools

import numpy as np

import _cases as K
import test_gpu_likelihood_masks as MK

# bounds against the oracle, (lik relative, mean absolute, sd, sd is relative?): test_hip_matches_oracle_and_reference_goldens' for the
# single plan (u3: R = 1e-6, cond ~1e9) and test_random_geometries' (lik there relative to max(1, |lik|))
STD = (1e-11, 1e-10, 1e-9, True)
HARD = (1e-8, 1e-8, 1e-6, True)
RND = (1e-9, 1e-8, 1e-7, False)
# the sharded result against the single plan on the same device (test_sharded_4_and_8_ways_on_one_gpu): spread of the likelihood over
# the ranks and the likelihood relative, mean and var absolute
SPREAD, SINGLE_LIK, SINGLE_MEAN, SINGLE_VAR = 1e-12, 1e-12, 1e-11, 1e-12

DEEP_TREE = (96, 64, 4)          # levels of 1, 4, 16, 64 and 256 nodes, cw 64: the fronts of the leaves' parents are kept as panels


def _specs_fam():
    mt = K.mt
    return [mt.KernelSpec(mt.KIND_MATERN52, 0.25, 1.3), mt.KernelSpec(mt.KIND_GAUSSIAN, 0.05, 0.8),
            mt.KernelSpec(mt.KIND_MATERN32, 0.3, 1.0, scale=2.5), mt.KernelSpec(mt.KIND_KANTER, 0.35),
            mt.KernelSpec(mt.KIND_IDEN, 1.0, 1.0, scale=0.7)]          # test_other_device_kernels_against_oracle's five


FAM_NAMES = ("m52", "gauss", "m32x2.5", "kanter", "iden")
RND_M2_SEEDS = (2, 4, 8)           # the seeds of "rnd" whose tree has two levels below the root (asserted by the CPU module)

# (id, worlds, shard level of each world)
TABLE = [
    ("g32", (5, 16), (2, 2)),
    ("m1-32-16", (3,), (1,)), ("m1-48-32", (3,), (1,)), ("m1-64-64", (3,), (1,)),
    ("kat2", (2,), (1,)),
    ("c1", (2, 3, 10), (1, 1, 3)),
    ("t201", (3, 10), (1, 3)),
    ("kat3", (3,), (1,)),
    ("u3", (2, 9), (1, 2)),
] + [("rnd%d" % s, (3, 16), (1, 2)) if s in RND_M2_SEEDS else ("rnd%d" % s, (3,), (1,)) for s in (2, 4, 6, 8)] + \
    [("fam-" + n, (4,), (1,)) for n in FAM_NAMES] + [
    ("circ", (3,), (1,)),
    ("empty", (4,), (1,)),
    ("deep", (5,), (2,)),
]
CELLS = [(cid, w) for cid, worlds, _ in TABLE for w in worlds]
CELL_IDS = ["%s-w%d" % c for c in CELLS]
SHARD_LEVEL = {(cid, w): lv[k] for cid, worlds, lv in TABLE for k, w in enumerate(worlds)}


def deep_problem():
    """``DEEP_TREE`` with 30 % of the locations observed, Matern32 l = 0.3, R = 1e-2."""
    topo, locs = MK._tree(*DEEP_TREE)
    obs = np.random.RandomState(0).uniform(size=topo.N) < 0.3
    return dict(topo=topo, locs=locs, y=MK._y(obs), R=1e-2, spec=K.mt.KernelSpec(K.mt.KIND_MATERN32, 0.3, 1.0), bounds=STD, single=True)


@functools.lru_cache(maxsize=None)
def problem(cid):
    """-> dict(topo, locs, y, R, spec, bounds (against the oracle), single (compare with the single plan on the device too))."""
    mt = K.mt
    if cid.startswith("m1-"):
        n, r = (int(v) for v in cid.split("-")[1:])
        topo, locs = MK._tree(n, r, 1)
        return dict(topo=topo, locs=locs, y=MK._y(MK.make_mask(topo, locs, "cloud")), R=MK.R, spec=MK._spec(), bounds=STD, single=True)
    if cid.startswith("rnd"):
        cs = K.random_geometry(int(cid[3:]))
        return dict(topo=cs["topo"], locs=cs["locs"], y=cs["y_obs"], R=cs["c"]["R"], spec=cs["spec"], bounds=RND, single=True, M=cs["M"], r=cs["r"])
    if cid.startswith("fam-"):
        cs = K.load_case("g32")
        return dict(topo=cs["topo"], locs=cs["locs"], y=cs["y_obs"], R=cs["c"]["R"], spec=_specs_fam()[FAM_NAMES.index(cid[4:])], bounds=STD, single=True)
    if cid == "circ":
        cs = K.load_case("c1")
        return dict(topo=cs["topo"], locs=cs["locs"], y=cs["y_obs"], R=cs["c"]["R"], spec=mt.KernelSpec(mt.KIND_EXP, 0.2, 1.0, 1.0, circular=True),
                    bounds=STD, single=True)
    if cid == "empty":
        # as test_sharded_likelihood_only_on_gappy_masks: every family's first child and the whole first level-1 subtree (rank 0 of 4) empty
        topo, locs = MK._tree(64, 16, 3)
        obs = MK.make_mask(topo, locs, "first_child")
        obs[MK._leaf_callers(topo, int(topo.level_ptr[1]))] = False
        return dict(topo=topo, locs=locs, y=MK._y(obs), R=MK.R, spec=MK._spec(), bounds=STD, single=True)
    if cid == "deep":
        return deep_problem()
    cs = K.load_case(cid)
    return dict(topo=cs["topo"], locs=cs["locs"], y=cs["y_obs"], R=cs["c"]["R"], spec=cs["spec"], bounds=HARD if cid == "u3" else STD, single=cid != "u3")


@functools.lru_cache(maxsize=None)
def oracle(cid):
    """The unsharded level-wise oracle on the full tree, once per process (``deep``: about ten seconds of host time)."""
    from oracle.mra_levelwise import run_levelwise
    p = problem(cid)
    return run_levelwise(p["topo"], p["locs"], p["spec"], p["y"], p["R"])


def local_topologies(topo, world):
    from pymra_amd.sharding import shard_topology
    return [shard_topology(topo, world, rk) for rk in range(world)]


def check_partition(topo, locals_):
    """A1: the ranks' owned caller rows are pairwise disjoint and together the reported rows of the unsharded topology.
    -> the owned rows of each rank."""
    own = [K.owned_rows(lt) for lt in locals_]
    seen = np.zeros(topo.N, dtype=np.int64)
    for rows in own:
        assert len(np.unique(rows)) == len(rows)
        seen[rows] += 1
    assert seen.max() <= 1, "caller rows owned by more than one rank: %s" % np.nonzero(seen > 1)[0][:8]
    reported = np.zeros(topo.N, dtype=bool)
    reported[K.owned_rows(topo)] = True
    assert np.array_equal(seen == 1, reported), "the ranks' rows are not the reported rows of the unsharded tree"
    return own


def check_own_rows_only(ranks, own, N):
    """A2: a rank's mean and var are exactly 0.0 at every caller row it does not own (rows a 1-D split drops: on every rank)."""
    for rk, (r, rows) in enumerate(zip(ranks, own)):
        other = np.ones(N, dtype=bool)
        other[rows] = False
        for what in ("mean", "var"):
            bad = np.nonzero(other & (r[what] != 0.0))[0]
            assert len(bad) == 0, "rank %d writes %s at rows it does not own: %s" % (rk, what, bad[:8])


def errors_vs_oracle(lik, mean, var, ref, bounds):
    """(lik, mean, sd) errors in the units of ``bounds``."""
    rel_sd = bounds[3]
    e_l = abs(lik - ref["lik"]) / (abs(ref["lik"]) if rel_sd else max(1.0, abs(ref["lik"])))
    e_m = float(np.max(np.abs(mean - ref["mean"])))
    sd = np.sqrt(np.maximum(var, 0.0)) if not rel_sd else np.sqrt(var)
    e_s = K.rel(sd, ref["sd"]) if rel_sd else float(np.max(np.abs(sd - ref["sd"])))
    return e_l, e_m, e_s
