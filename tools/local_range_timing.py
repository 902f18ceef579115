"""What local ranges cost (profiles/local_range_timing.txt): a 256 x 256 grid, M = 4, r0 = 16, 40 % observed (bench.py's c2) or the
1024 x 1024, M = 6, r0 = 32 of c3, one plan per kernel, medians of five passes after one warm-up.

  device   a likelihood-only pass and a predict pass, wall milliseconds, for
             matern32            Matern32 on (x, y), its default route (the fused cascades)
             matern32_d3_levels  Matern32 on the d = 3 coordinates (x, y, lam) level by level (MRA_OPT_FUSED = 0): the kernels of the
                                 commit before MRA_KERNEL_LOCAL on the route it takes - the yardstick of what the evaluation costs
             local_matern32      LocalRange(Matern32), the range tenfold across the square
           then (c2) one pass each under MRA_OPT_KERNEL_TIMING for the per-family stream milliseconds of mra_get_kernel_stats.
  host     (c2) what such a covariance cost before: the MRA_KERNEL_HOST route fed by LocalRange.evaluate, mra_plan_set_cov_block per
           node and a likelihood-only pass, end to end per likelihood evaluation as an MLE loop pays it.

    python tools/local_range_timing.py [c2|c3] [--host-only | --device-only]

Prints one JSON line per measurement."""
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pymra_amd.MRATools as mt                          # noqa: E402
from pymra_amd import plan as P                          # noqa: E402
from pymra_amd.topology import build_topology            # noqa: E402

CONFIGS = {"c2": dict(n=256, M=4, r=16, l=0.3), "c3": dict(n=1024, M=6, r=32, l=0.3)}
REPS = 5


def wall(fn):
    P.device_synchronize(0)
    t0 = time.perf_counter()
    fn()
    P.device_synchronize(0)
    return 1e3 * (time.perf_counter() - t0)


def median_ms(fn):
    fn()
    return float(np.median([wall(fn) for _ in range(REPS)]))


def families(pl, predict):
    pl.set_option(P.MRA_OPT_KERNEL_TIMING, 1)
    pl.run(True, predict)
    st = {k["name"]: round(k["ms"], 4) for k in pl.kernel_stats() if k["launches"]}
    pl.set_option(P.MRA_OPT_KERNEL_TIMING, 0)
    return st


def main(cfg, host_only, device_only=False):
    c = CONFIGS[cfg]
    np.random.seed(11)
    locs = mt.genLocations2d(Nx=c["n"], Ny=c["n"])
    N = len(locs)
    y = np.where(np.random.uniform(size=(N, 1)) < 0.4, np.random.normal(size=(N, 1)), np.nan)
    topo = build_topology(locs, c["r"], c["M"], 4)
    topo3 = dataclasses.replace(topo, coord_dim=3)
    R = 1e-2
    l = c["l"]
    lam = l * 10.0 ** (locs[:, 0] - 0.5)                 # l / sqrt(10) .. l sqrt(10): tenfold, l in the middle
    X3 = np.column_stack([locs, lam])
    spec = mt.LocalRange(mt.KernelSpec(mt.KIND_MATERN32, 1.0, 1.0))

    def plan(three):
        pl = P.HipPlan(topo3 if three else topo, 0)
        pl.set_locs(X3 if three else locs); pl.set_obs(y, R)
        return pl

    if not host_only:
        base = {}
        rows = [("matern32", False, False, ()), ("matern32_d3_levels", True, False, ((P.MRA_OPT_FUSED, 0),)), ("local_matern32", True, True, ())]
        for name, three, local, opts in rows:
            pl = plan(three)
            for o, v in opts:
                pl.set_option(o, v)
            if local:
                pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
            else:
                pl.set_kernel(mt.KIND_MATERN32, l, 1.0, 1.0)
            lik = median_ms(lambda: pl.run(True, False))
            pred = median_ms(lambda: pl.run(True, True))
            out = dict(config=cfg, kernel=name, path=pl.route()["path"], lik_ms=round(lik, 3), predict_ms=round(pred, 3))
            if cfg == "c2":
                out.update(lik_families_ms=families(pl, False), predict_families_ms=families(pl, True))
            if not local:
                base[name] = (lik, pred)
            else:
                out["lik_over_matern32"] = round(lik / base["matern32"][0], 2)
                out["predict_over_matern32"] = round(pred / base["matern32"][1], 2)
                out["lik_over_matern32_d3_levels"] = round(lik / base["matern32_d3_levels"][0], 3)
                out["predict_over_matern32_d3_levels"] = round(pred / base["matern32_d3_levels"][1], 3)
            print(json.dumps(out), flush=True)
            pl.close()

    if not device_only and cfg == "c2":
        pl = plan(True)

        def evaluation():
            pl.upload_host_cov(lambda a, b: spec.evaluate(a, b), X3, y)       # the blocks of every node, evaluated on the host and sent
            pl.run(True, False)
        evaluation()
        ms = [wall(evaluation) for _ in range(REPS)]
        print(json.dumps(dict(config=cfg, kernel="host_local_matern32", path=pl.route()["path"], lik_eval_ms=round(float(np.median(ms)), 1))), flush=True)
        pl.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args[0] if args else "c2", "--host-only" in sys.argv, "--device-only" in sys.argv)
