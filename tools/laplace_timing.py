"""Cost of the Laplace fit (mra_plan_fit_laplace) at config c3's shape with Poisson counts: one full fit from
the data-based start, its time per iteration (total / passes, and the marginal cost of an iteration from fits stopped after 2 passes),
the plain likelihood + predict pass of the same plan, and the same Newton iteration driven from Python through predict / set_obs with
a noise vector.  Wall-clock medians of three around calls that return synchronised; the device time of the launches the fit adds
between two passes from the kernel events of one more fit.  Prints one JSON line
(profiles/laplace_timing.txt).
usage: python tools/laplace_timing.py [repeats]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from pymra_amd import plan as P
from pymra_amd.topology import build_topology
import pymra_amd.MRATools as mt

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
TOL = 1e-10
c = bench.CONFIGS["c3"]
locs, y_obs = bench.make_inputs(c)
topo = build_topology(locs, c["r"], c["M"], c["J"])
seen = np.isfinite(y_obs.ravel())
rng = np.random.RandomState(5)
x_true = np.sin(2 * np.pi * locs[:, 0]) * np.cos(2 * np.pi * locs[:, 1])
E = np.exp(rng.uniform(np.log(0.5), np.log(20.0), size=len(seen)))
z = np.where(seen, rng.poisson(E * np.exp(x_true)).astype(np.float64), np.nan)
offset = np.log(E)
pl = P.HipPlan(topo, 0); pl.set_locs(locs); pl.set_obs(y_obs, c["R"]); pl.set_kernel(mt.KIND_MATERN32, c["l"], c["sig"], 1.0)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def median_of(fn):
    runs = [timed(fn) for _ in range(reps)]
    return float(np.median([r[0] for r in runs])), runs[-1][1]


def python_loop(max_iter=50):
    """the iteration of mra_plan_fit_laplace through the Gaussian calls: per pass a download of the mean, NumPy, set_obs with a vector"""
    x = np.log(z[seen] + 0.5) - offset[seen]
    t, r = np.full(len(seen), np.nan), np.full(len(seen), np.nan)
    for it in range(max_iter):
        mu = np.exp(x + offset[seen])
        D = np.maximum(mu, 2.0 ** -40)
        t[seen], r[seen] = x + (z[seen] - mu) / D, 1.0 / D
        pl.set_obs(t, r)
        pl.run(True, True)
        xh = pl.predict()[0][seen]
        step = np.abs(xh - x).max()
        if step <= TOL * max(1.0, np.abs(xh).max()):
            return it + 1, sum(pl.likelihood())
        x = xh
    return max_iter, sum(pl.likelihood())


pl.fit_laplace("poisson", z, offset=offset, tol=TOL)                  # warm-up: allocations, LDS limits
fit_ms, res = median_of(lambda: pl.fit_laplace("poisson", z, offset=offset, tol=TOL))
passes = res["passes"]
two_ms, _ = median_of(lambda: pl.fit_laplace("poisson", z, offset=offset, tol=TOL, max_iter=2))
for _ in range(3):
    pl.run(True, True)
pass_ms, _ = median_of(lambda: pl.run(True, True))
pass_dev_ms = pl.timers()["total_ms"]
python_loop(2)
loop_ms, (loop_passes, loop_du) = median_of(python_loop)
# what the fit adds between two passes, on the device: the small-kernel family of the fit's last pass (k_laplace_linearise before
# it, k_laplace_part + k_laplace_sum + the copy of five doubles behind it) against that of a plain pass, hipEvent times
misc = lambda: [k["ms"] for k in pl.kernel_stats() if k["name"].startswith("small kernels")][0]      # noqa: E731
pl.set_option(P.MRA_OPT_KERNEL_TIMING, 1)
pl.fit_laplace("poisson", z, offset=offset, tol=TOL)
fit_misc_ms = misc()
pl.run(True, True)
plain_misc_ms = misc()
pl.set_option(P.MRA_OPT_KERNEL_TIMING, 0)
pl.set_obs(y_obs, c["R"])
out = {"config": "c3", "P": int(topo.P), "n_obs": int(seen.sum()), "family": "poisson", "tol": TOL, "repeats": reps,
       "fit_ms": round(fit_ms, 3), "passes": passes, "converged": res["converged"], "fit_ms_per_iteration": round(fit_ms / passes, 3),
       "fit_2_passes_ms": round(two_ms, 3), "marginal_ms_per_iteration": round((fit_ms - two_ms) / max(passes - 2, 1), 3),
       "plain_pass_ms": round(pass_ms, 3), "plain_pass_device_ms": round(pass_dev_ms, 3),
       "python_loop_ms": round(loop_ms, 3), "python_loop_passes": loop_passes, "python_loop_ms_per_iteration": round(loop_ms / loop_passes, 3),
       "small_kernels_ms_last_pass_of_fit": round(fit_misc_ms, 4), "small_kernels_ms_plain_pass": round(plain_misc_ms, 4),
       "lik": res["lik"], "d_plus_u": res["d"] + res["u"], "python_loop_d_plus_u": loop_du}
print(json.dumps(out))
