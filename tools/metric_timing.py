"""Cost of mra_plan_set_metric on a bench config (default c3), medians of 5 in one process: set_metric (the transform launch, the
knot rebuild and its uploads; wall time with the device synchronised, which contains the stream time), set_locs of a pre-transformed
array, an MRATree(...) rebuild on pre-transformed cov_locs, the likelihood-only pass that follows set_metric against the one that
follows set_kernel alone (wall, and the stream total of mra_get_timers), and the wall time per evaluation of an MLE loop over
(l, ratio, angle) through MRATree.reevaluate.  Prints one JSON line (profiles/metric_timing.txt).
usage: python tools/metric_timing.py [config]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from pymra_amd import MRATree, plan as P
from pymra_amd.topology import build_topology
import pymra_amd.MRATools as mt
name = sys.argv[1] if len(sys.argv) > 1 else "c3"
c = bench.CONFIGS[name]
locs, y_obs = bench.make_inputs(c)
np.random.seed(1)
topo = build_topology(locs, c["r"], c["M"], c["J"])
pl = P.HipPlan(topo, 0); pl.set_locs(locs); pl.set_obs(y_obs, c["R"]); pl.set_kernel(mt.KIND_MATERN32, c["l"], c["sig"], 1.0)
pl.run(True, False)
As = [mt.aniso2d(1.0 + 0.5 * k, 10.0 * k) for k in range(1, 7)]


def timed(fn, sync=True):
    P.device_synchronize(0)
    t0 = time.perf_counter()
    fn()
    if sync:
        P.device_synchronize(0)
    return 1e3 * (time.perf_counter() - t0)


def med(v):
    return round(float(np.median(v)), 3)


out = {"config": name, "P": int(topo.P), "d": int(locs.shape[1])}
out["first_set_metric_wall_ms"] = round(timed(lambda: pl.set_metric(As[0])), 3)          # allocates the raw array, reads the knots back
out["set_metric_wall_ms"] = med([timed(lambda: pl.set_metric(A)) for A in As[1:]])
after_metric, after_kernel, sm, sk = [], [], [], []
for A in As[1:]:
    pl.set_metric(A); pl.set_kernel(mt.KIND_MATERN32, c["l"], c["sig"], 1.0)
    after_metric.append(timed(lambda: pl.run(True, False))); sm.append(pl.timers()["total_ms"])
    pl.set_kernel(mt.KIND_MATERN32, c["l"] * 1.01, c["sig"], 1.0)
    after_kernel.append(timed(lambda: pl.run(True, False))); sk.append(pl.timers()["total_ms"])
out["lik_pass_after_set_metric_ms"] = {"wall": med(after_metric), "stream": med(sm)}
out["lik_pass_after_set_kernel_ms"] = {"wall": med(after_kernel), "stream": med(sk)}
pl.set_metric(None)
pre = [np.ascontiguousarray(locs @ A.T) for A in As[1:]]
out["set_locs_pretransformed_wall_ms"] = med([timed(lambda: pl.set_locs(X)) for X in pre])
pl.close()


def rebuild(X):
    np.random.seed(1)
    t = MRATree(locs, c["r"], lambda a, b: mt.Matern32(a, b, l=c["l"], sig=c["sig"]), y_obs, c["R"], M=c["M"], J=c["J"], want_predict=False,
                cov_locs=X, verbose=False)
    t.plan.close()


rebuild(pre[0])
out["mratree_rebuild_wall_ms"] = med([timed(lambda: rebuild(X)) for X in pre])
np.random.seed(1)
tree = MRATree(locs, c["r"], lambda a, b: mt.Matern32(a, b, l=c["l"], sig=c["sig"], metric=As[0]), y_obs, c["R"], M=c["M"], J=c["J"],
               want_predict=False, verbose=False)
ev = [timed(lambda: tree.reevaluate(lambda a, b: mt.Matern32(a, b, l=c["l"] * (1 + 0.01 * k), sig=c["sig"], metric=As[k % 6])), sync=False)
      for k in range(1, 11)]
out["mle_evaluation_wall_ms"] = {"median_of_10": med(ev), "min": round(min(ev), 3), "max": round(max(ev), 3)}
print(json.dumps(out))
