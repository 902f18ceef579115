"""Cost of a noise vector (mra_plan_set_noise) on config c3: predictive and likelihood-only passes with the scalar R and with a
varying vector, alternating in blocks in one process; per pass the hipEvent total of the pass (HipPlan.timers()["total_ms"]).
Prints one JSON line (profiles/obs_noise_timing.txt).
usage: python tools/obs_noise_timing.py [rounds [passes per block]]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from pymra_amd import plan as P
from pymra_amd.topology import build_topology
import pymra_amd.MRATools as mt
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
per = int(sys.argv[2]) if len(sys.argv) > 2 else 10
c = bench.CONFIGS["c3"]
locs, y_obs = bench.make_inputs(c)
topo = build_topology(locs, c["r"], c["M"], c["J"])
pl = P.HipPlan(topo, 0); pl.set_locs(locs); pl.set_obs(y_obs, c["R"]); pl.set_kernel(mt.KIND_MATERN32, c["l"], c["sig"], 1.0)
r = c["R"] * 4.0 ** (np.sin(2 * np.pi * locs[:, 0]) * np.cos(2 * np.pi * locs[:, 1]))          # in [R / 4, 4 R]
ms = {(m, k): [] for m in ("scalar", "vector") for k in ("predict", "likelihood")}
lik = {}
for rnd in range(rounds):
    for mode in ("scalar", "vector"):
        pl.set_noise(r if mode == "vector" else None)
        for kind in ("predict", "likelihood"):
            for i in range(3 + per):
                pl.run(True, kind == "predict")
                if i >= 3:
                    ms[(mode, kind)].append(pl.timers()["total_ms"])
            lik[(mode, kind)] = sum(pl.likelihood())
out = {"config": "c3", "P": int(topo.P), "n_leaves": int(np.count_nonzero(topo.node_leaf)), "n_obs": int(np.isfinite(y_obs).sum()),
       "rounds": rounds, "passes_per_block": per}
for kind in ("predict", "likelihood"):
    s, v = np.array(ms[("scalar", kind)]), np.array(ms[("vector", kind)])
    blocks_s = s.reshape(rounds, per).mean(1)
    out[kind] = {"passes_each": int(len(s)), "scalar_median_ms": round(float(np.median(s)), 4), "vector_median_ms": round(float(np.median(v)), 4),
                 "vector_minus_scalar_ms": round(float(np.median(v) - np.median(s)), 4),
                 "vector_minus_scalar_percent": round(float(100.0 * (np.median(v) - np.median(s)) / np.median(s)), 3),
                 "scalar_block_means_ms": [round(float(x), 4) for x in blocks_s],
                 "scalar_block_spread_ms": round(float(blocks_s.max() - blocks_s.min()), 4),
                 "lik_scalar": lik[("scalar", kind)], "lik_vector": lik[("vector", kind)]}
print(json.dumps(out))
