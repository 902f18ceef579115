"""Cost of mra_cv on a bench config (default c3): wall and stream milliseconds (mra_get_buffer 12) of both groupings with the factors
valid, medians of three - and the way without it: refits with one leaf's rows masked (set_obs, then a likelihood + predict pass),
8 of them timed and scaled to one refit per observed leaf.  Prints one JSON line (profiles/cv_timing.txt).
usage: python tools/cv_timing.py [config]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from pymra_amd import plan as P
from pymra_amd.topology import build_topology
import pymra_amd.MRATools as mt
name = sys.argv[1] if len(sys.argv) > 1 else "c3"
c = bench.CONFIGS[name]
locs, y_obs = bench.make_inputs(c)
topo = build_topology(locs, c["r"], c["M"], c["J"])
pl = P.HipPlan(topo, 0); pl.set_locs(locs); pl.set_obs(y_obs, c["R"]); pl.set_kernel(mt.KIND_MATERN32, c["l"], c["sig"], 1.0)
pl.run(True, True)
NAMES = ["basis", "leaf", "chain", "mean_and_sweeps", "gram", "cholesky", "solve_and_reduction", "uploads", "downloads"]
out = {"config": name, "P": int(topo.P), "n_leaves": int(np.count_nonzero(topo.node_leaf)), "n_obs": int(np.isfinite(y_obs).sum())}
pl.cv()                                                     # the pass with W at every row, and the work buffers
for leaf in (False, True):
    pl.cv(leaf=leaf)
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        info = pl.cv(leaf=leaf)[4]
        wall.append(1e3 * (time.perf_counter() - t0))
    pl.set_option(P.MRA_OPT_KERNEL_TIMING, 1)                # a measuring mode: one synchronisation per entry
    stream = []
    for _ in range(3):
        pl.cv(leaf=leaf)
        stream.append(pl.buffer(12))
    pl.set_option(P.MRA_OPT_KERNEL_TIMING, 0)
    med = np.median(np.array(stream), axis=0)
    out["leaf" if leaf else "loo"] = {"wall_ms_median_of_3": round(float(np.median(wall)), 3), "wall_ms": [round(w, 3) for w in wall],
                                      "stream_ms_median_of_3": {k: round(float(v), 4) for k, v in zip(NAMES, med)},
                                      "stream_ms_total": round(float(med.sum()), 3),
                                      "rows": int(info[0]), "groups": int(info[1]), "score": float(info[2]), "max_h": float(info[5])}
# without mra_cv: one refit per left-out leaf
y = np.asarray(y_obs, float).reshape(-1, 1)
obs_p = np.isfinite(y.ravel())[topo.src] & (topo.perm >= 0)
leaves = [int(i) for i in np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]]
n_obs_leaves = sum(1 for i in leaves if obs_p[int(topo.node_row0[i]):int(topo.node_row1[i])].any())
pick = [int(i) for i in np.random.default_rng(1).choice(leaves, 8, replace=False)]
P.device_synchronize(0)
t0 = time.perf_counter()
for i in pick:
    rows = np.arange(int(topo.node_row0[i]), int(topo.node_row1[i]))
    y2 = y.copy()
    y2[topo.perm[rows[obs_p[rows]]]] = np.nan
    pl.set_obs(y2, c["R"])
    pl.run(True, True)
    pl.predict()
refit = 1e3 * (time.perf_counter() - t0)
out["refits"] = {"timed": len(pick), "wall_ms": round(refit, 3), "wall_ms_each": round(refit / len(pick), 3), "observed_leaves": n_obs_leaves,
                 "wall_ms_scaled_to_every_leaf": round(refit / len(pick) * n_obs_leaves, 1)}
out["refits_over_leaf_cv"] = round(out["refits"]["wall_ms_scaled_to_every_leaf"] / out["leaf"]["wall_ms_median_of_3"], 1)
print(json.dumps(out))
