"""Wall time of mra_sample at BASELINE configs 3 and 5: 16 prior draws (one block of 16) and 16 conditional draws (one likelihood +
predict pass each), against one likelihood + predict pass of the same plan.  Each timing is taken after a warm-up call of the same
shape (the first call builds the sampler's index maps and allocates its buffers).  Prints one JSON line per configuration.

    python tools/sample_timing.py [c3] [c5]

With --solve, after those lines: 16 conditional draws with MRA_OPT_SAMPLE_SOLVE off and then on (same plan, same process, in that
order), and mra_solve for 16 columns with the factors already valid (mean + quad, upload and 16 x P download included), each as the
median of three repeats; one more JSON line per configuration (profiles/solve_timing.txt)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import pymra_amd.MRATools as mt          # noqa: E402
from pymra_amd import plan as P          # noqa: E402
from pymra_amd.topology import build_topology   # noqa: E402


def make(cfg):
    if cfg == "c3":
        import make_golden as mg
        c = mg.CASES["c3"]
        locs, y_obs, _ = mg.make_inputs(c)
        topo = build_topology(locs, c["r"], c["M"], c["J"])
        kern, R = (mt.KIND_MATERN32, c["l"], c["sig"]), c["R"]
    else:                                # config 5 as tools/c5_run.py builds it
        n = 2048
        np.random.seed(11)
        locs = mt.genLocations2d(Nx=n, Ny=n)
        y = np.random.normal(size=(n * n, 1))
        oi = np.sort(np.random.choice(n * n, int(0.4 * n * n), replace=False))
        y_obs = np.full((n * n, 1), np.nan)
        y_obs[oi] = y[oi]
        topo = build_topology(locs, 64, 8, 4)
        kern, R = (mt.KIND_MATERN32, 0.3, 1.0), 1e-2
    pl = P.HipPlan(topo, 0)
    pl.set_locs(locs)
    pl.set_obs(y_obs, R)
    pl.set_kernel(kern[0], kern[1], kern[2], 1.0)
    return pl, topo


def timed(fn):
    P.device_synchronize(0)
    t0 = time.perf_counter()
    out = fn()
    P.device_synchronize(0)
    return 1e3 * (time.perf_counter() - t0), out


def main(cfgs, solve=False):
    for cfg in cfgs:
        pl, topo = make(cfg)
        pl.run(True, True)
        pass_ms = min(timed(lambda: pl.run(True, True))[0] for _ in range(3))
        pl.sample(16, seed=1)                                   # warm-up: index maps, buffers, Gram batches
        prior_ms, x = timed(lambda: pl.sample(16, seed=2))
        pl.sample(1, seed=3, conditional=True)
        cond_ms, xc = timed(lambda: pl.sample(16, seed=4, conditional=True))
        print(json.dumps({"config": cfg, "P": int(topo.P), "n_nodes": int(topo.n_nodes), "latent_slots": pl.sample_slots(),
                          "lik_predict_pass_ms": round(pass_ms, 2), "prior_16_draws_ms": round(prior_ms, 2),
                          "conditional_16_draws_ms": round(cond_ms, 2), "finite": bool(np.isfinite(x).all() and np.isfinite(xc).all())}),
              flush=True)
        if solve:
            med = lambda fn: float(np.median([timed(fn)[0] for _ in range(3)]))          # noqa: E731
            off_ms = med(lambda: pl.sample(16, seed=4, conditional=True))
            pl.set_option(P.MRA_OPT_SAMPLE_SOLVE, 1)
            xs = pl.sample(16, seed=4, conditional=True)                                  # warm-up: the solver's buffers
            on_ms = med(lambda: pl.sample(16, seed=4, conditional=True))
            pl.set_option(P.MRA_OPT_SAMPLE_SOLVE, 0)
            Y = np.random.default_rng(5).standard_normal((16, topo.P))
            first_ms, _ = timed(lambda: pl.solve(Y))                                       # factorises: one likelihood pass inside
            solve_ms = med(lambda: pl.solve(Y))
            quad_ms = med(lambda: pl.solve(Y, want_mean=False))
            print(json.dumps({"config": cfg, "conditional_16_draws_option_off_ms": round(off_ms, 2),
                              "conditional_16_draws_option_on_ms": round(on_ms, 2),
                              "max_abs_on_minus_off": float(np.abs(xs - xc).max()),
                              "solve_16_columns_first_call_ms": round(first_ms, 2), "solve_16_columns_factors_valid_ms": round(solve_ms, 2),
                              "solve_16_columns_quad_only_ms": round(quad_ms, 2)}), flush=True)
        pl.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--solve"]
    main(args or ["c3", "c5"], solve="--solve" in sys.argv[1:])
