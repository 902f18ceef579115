"""Cost of the third coordinate: a 1024x1024 lon/lat grid (M = 6, J = 4, r0 = 32, Matern-3/2, 40 % observed), the
resident likelihood + predict pass and the likelihood-only pass, once with planar 2-D coordinates (lon/lat/180) and once with
coord_dim = 3 (xyz on the unit sphere) on the SAME topology, alternating in blocks in one process; per pass the hipEvent total of
the pass (HipPlan.timers()["total_ms"]).  Prints one JSON line (profiles/sphere_timing.txt).
usage: python tools/sphere_timing.py [rounds [passes per block [grid side]]]"""
import dataclasses, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pymra_amd import plan as P
from pymra_amd.topology import build_topology
import pymra_amd.MRATools as mt
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
per = int(sys.argv[2]) if len(sys.argv) > 2 else 10
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
M, J, r0, l, R = 6, 4, 32, 0.3, 1e-2
lon = -180.0 + (np.arange(n) + 0.5) * 360.0 / n
g, h = np.meshgrid(lon, np.linspace(-80.0, 80.0, n))
ll = np.column_stack((g.ravel(), h.ravel()))
xyz = mt.lonlat_to_xyz(ll)
rng = np.random.default_rng(11)
y_obs = np.where(rng.random(n * n) < 0.4, np.sin(3.0 * xyz[:, 0]) + xyz[:, 1] * xyz[:, 2] + 0.1 * rng.standard_normal(n * n), np.nan)
np.random.seed(11)
topo3 = build_topology(ll, r0, M, J, coord_dim=3)
topo2 = dataclasses.replace(topo3, coord_dim=0)
plans = {}
for name, topo, X in (("2d", topo2, ll / 180.0), ("3d", topo3, xyz)):
    pl = P.HipPlan(topo, 0); pl.set_locs(X); pl.set_obs(y_obs, R); pl.set_kernel(mt.KIND_MATERN32, l, 1.0, 1.0)
    plans[name] = pl
ms = {(m, k): [] for m in plans for k in ("predict", "likelihood")}
lik, route = {}, {}
for rnd in range(rounds):
    for mode, pl in plans.items():
        for kind in ("predict", "likelihood"):
            for i in range(3 + per):
                pl.run(True, kind == "predict")
                if i >= 3:
                    ms[(mode, kind)].append(pl.timers()["total_ms"])
            lik[(mode, kind)] = sum(pl.likelihood())
            route[(mode, kind)] = pl.route()["path"]
out = {"grid": "%dx%d lon/lat" % (n, n), "M": M, "J": J, "r0": r0, "kernel": "Matern32 l=%g" % l, "P": int(topo3.P),
       "n_leaves": int(np.count_nonzero(topo3.node_leaf)), "n_obs": int(np.isfinite(y_obs).sum()), "rounds": rounds, "passes_per_block": per}
for kind in ("predict", "likelihood"):
    a, b = np.array(ms[("2d", kind)]), np.array(ms[("3d", kind)])
    blocks_a, blocks_b = a.reshape(rounds, per).mean(1), b.reshape(rounds, per).mean(1)
    out[kind] = {"passes_each": int(len(a)), "route_2d": route[("2d", kind)], "route_3d": route[("3d", kind)],
                 "planar_2d_median_ms": round(float(np.median(a)), 4), "xyz_3d_median_ms": round(float(np.median(b)), 4),
                 "3d_minus_2d_ms": round(float(np.median(b) - np.median(a)), 4),
                 "3d_minus_2d_percent": round(float(100.0 * (np.median(b) - np.median(a)) / np.median(a)), 3),
                 "planar_2d_block_means_ms": [round(float(x), 4) for x in blocks_a],
                 "xyz_3d_block_means_ms": [round(float(x), 4) for x in blocks_b],
                 "planar_2d_block_spread_ms": round(float(blocks_a.max() - blocks_a.min()), 4),
                 "lik_2d": lik[("2d", kind)], "lik_3d": lik[("3d", kind)]}
for pl in plans.values():
    pl.close()
print(json.dumps(out))
