"""Cost of mra_cv_trend on a bench config (default c3): wall and stream milliseconds (mra_get_buffer 15) of both modes and both
groupings with the factors valid, p = 3 and p = 63, medians of three - against its floor, mra_cv on y - X beta^ in the same process
(mra_get_buffer 12), and against the way without it: refits of the trend with one leaf's rows masked (set_obs, then mra_trend_fit with
its predict pass), 8 of them timed and scaled to one refit per observed leaf.  The stream table gives the share of the trend's sweeps
and of the two new kernels.  Prints one JSON line per p (profiles/cv_trend_timing.txt).
usage: python tools/cv_trend_timing.py [config]"""
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
N = len(locs)
NAMES = ["basis", "leaf", "chain", "mean_and_sweeps", "gram", "cholesky", "solve_and_reduction", "uploads", "downloads", "trend_sweeps",
         "k_cv_trend", "k_cv_downdate"]
y = np.asarray(y_obs, float).reshape(-1, 1)
obs_p = np.isfinite(y.ravel())[topo.src] & (topo.perm >= 0)
leaves = [int(i) for i in np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]]
n_obs_leaves = sum(1 for i in leaves if obs_p[int(topo.node_row0[i]):int(topo.node_row1[i])].any())


def timed(pl, call, what, names):
    call()
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        info = call()[4]
        wall.append(1e3 * (time.perf_counter() - t0))
    pl.set_option(P.MRA_OPT_KERNEL_TIMING, 1)                # a measuring mode: one synchronisation per entry
    stream = []
    for _ in range(3):
        call()
        stream.append(pl.buffer(what))
    pl.set_option(P.MRA_OPT_KERNEL_TIMING, 0)
    med = np.median(np.array(stream), axis=0)
    return {"wall_ms_median_of_3": round(float(np.median(wall)), 3), "wall_ms": [round(w, 3) for w in wall],
            "stream_ms_median_of_3": {k: round(float(v), 4) for k, v in zip(names, med)}, "stream_ms_total": round(float(med.sum()), 3),
            "rows": int(info[0]), "groups": int(info[1]), "score": float(info[2]), "max_leverage": float(info[5])}


for p in (3, 63):
    X = np.column_stack([np.ones(N), np.asarray(locs, float).reshape(N, -1), np.random.default_rng(3).standard_normal((N, 64))])[:, :p]
    pl = P.HipPlan(topo, 0); pl.set_locs(locs); pl.set_obs(y_obs, c["R"]); pl.set_kernel(mt.KIND_MATERN32, c["l"], c["sig"], 1.0)
    pl.set_trend(X)
    pl.run(True, True)
    out = {"config": name, "p": p, "P": int(topo.P), "n_leaves": len(leaves), "n_obs": int(np.isfinite(y_obs).sum())}
    pl.cv_trend()                                            # the pass with W at every row, and the work buffers
    for leaf in (False, True):
        for refit in (True, False):
            key = ("leaf" if leaf else "loo") + ("_refit" if refit else "_fixed")
            out[key] = timed(pl, lambda: pl.cv_trend(leaf=leaf, refit=refit), 15, NAMES)
    # the floor: mra_cv on the detrended data, in the same process
    beta = pl.trend_fit().beta
    fl = P.HipPlan(topo, 0); fl.set_locs(locs); fl.set_obs(y - (X @ beta).reshape(-1, 1), c["R"]); fl.set_kernel(mt.KIND_MATERN32, c["l"], c["sig"], 1.0)
    fl.run(True, True)
    fl.cv()
    for leaf in (False, True):
        out["floor_" + ("leaf" if leaf else "loo")] = timed(fl, lambda: fl.cv(leaf=leaf), 12, NAMES[:9])
    fl.close()
    for leaf in ("loo", "leaf"):
        for mode in ("refit", "fixed"):
            out[leaf + "_" + mode + "_over_floor_stream"] = round(out[leaf + "_" + mode]["stream_ms_total"] / out["floor_" + leaf]["stream_ms_total"], 2)
    # without mra_cv_trend: one refit of the trend per left-out leaf
    pick = [int(i) for i in np.random.default_rng(1).choice(leaves, 8, replace=False)]
    P.device_synchronize(0)
    t0 = time.perf_counter()
    for i in pick:
        rows = np.arange(int(topo.node_row0[i]), int(topo.node_row1[i]))
        y2 = y.copy()
        y2[topo.perm[rows[obs_p[rows]]]] = np.nan
        pl.set_obs(y2, c["R"])
        pl.trend_fit(predict=True)
    refit = 1e3 * (time.perf_counter() - t0)
    out["refits"] = {"timed": len(pick), "wall_ms": round(refit, 3), "wall_ms_each": round(refit / len(pick), 3), "observed_leaves": n_obs_leaves,
                     "wall_ms_scaled_to_every_leaf": round(refit / len(pick) * n_obs_leaves, 1)}
    out["refits_over_leaf_refit_cv"] = round(out["refits"]["wall_ms_scaled_to_every_leaf"] / out["leaf_refit"]["wall_ms_median_of_3"], 1)
    pl.close()
    print(json.dumps(out), flush=True)
