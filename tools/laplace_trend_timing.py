"""Cost of the Laplace fit with a regression trend (mra_plan_fit_laplace_trend) at config c3's shape with Poisson
counts, p = 3 and p = 63: one full fit from the data-based start and its time per iteration, split on the device (kernel timing on:
hipEvent times, summed over the passes of one more fit) into the factorisation pass, the sweeps of the ceil((1 + p) / 16) blocks
(with staging, cross tiles and transfers) and the tail (k_laplace_trend_part + k_laplace_sum) - the pass is the sum of the kernel families' event times (mra_get_kernel_stats, which
records the kernels of a pass and the two elementwise launches of the fit, not the solver's sweeps: those are timed only into the
trend's record, mra_get_buffer(14)) less the tail, which both count; the trendless mra_plan_fit_laplace
iteration of the same plan in the same session; and the composition a caller had before: set_obs(t) + set_noise(r) +
trend_fit(predict=True) per iteration from Python.  The tail's bytes over its time against the HBM peak: `useful` counts the
observed rows only, `touched` every row (a 40 % random mask leaves no 128-byte line of a column unread).  Wall-clock medians of
three after a warm-up around calls that return synchronised.  Prints one JSON line per p (profiles/laplace_trend_timing.txt).
usage: python tools/laplace_trend_timing.py [repeats]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from pymra_amd import plan as P
from pymra_amd.topology import build_topology
import pymra_amd.MRATools as mt

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
TOL = 1e-10
HBM_PEAK = 8.0e12
c = bench.CONFIGS["c3"]
locs, y_obs = bench.make_inputs(c)
topo = build_topology(locs, c["r"], c["M"], c["J"])
N = len(locs)
seen = np.isfinite(y_obs.ravel())
rng = np.random.RandomState(5)
x_true = np.sin(2 * np.pi * locs[:, 0]) * np.cos(2 * np.pi * locs[:, 1])
E = np.exp(rng.uniform(np.log(0.5), np.log(20.0), size=N))
offset = np.log(E)
pl = P.HipPlan(topo, 0); pl.set_locs(locs); pl.set_obs(y_obs, c["R"]); pl.set_kernel(mt.KIND_MATERN32, c["l"], c["sig"], 1.0)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def median_of(fn):
    runs = [timed(fn) for _ in range(reps)]
    return float(np.median([r[0] for r in runs])), runs[-1][1]


def python_loop(z, max_iter=50):
    """the iteration through the calls a caller had before: per pass NumPy, set_obs, set_noise and a predicting trend fit"""
    e = np.log(z[seen] + 0.5) - offset[seen]
    t, r = np.full(N, np.nan), np.full(N, np.nan)
    for it in range(max_iter):
        mu = np.exp(e + offset[seen])
        D = np.maximum(mu, 2.0 ** -40)
        t[seen], r[seen] = e + (z[seen] - mu) / D, 1.0 / D
        pl.set_obs(t, 1.0)
        pl.set_noise(r)
        fit = pl.trend_fit(predict=True)
        eh = fit.mean[seen]
        step = np.abs(eh - e).max()
        if step <= TOL * max(1.0, np.abs(eh).max()):
            return it + 1, fit.beta
        e = eh
    return max_iter, fit.beta


for p in (3, 63):
    X = 0.25 * np.random.default_rng(3).standard_normal((N, p))
    X[:, 0] = 1.0
    beta_true = np.linspace(0.5, -0.5, p); beta_true[0] = 0.4
    z = np.where(seen, np.random.RandomState(6).poisson(E * np.exp(x_true + X @ beta_true)).astype(np.float64), np.nan)
    pl.set_obs(y_obs, c["R"])
    upload_ms, _ = timed(lambda: pl.set_trend(X))
    fit = lambda **kw: pl.fit_laplace_trend("poisson", z, offset=offset, tol=TOL, **kw)      # noqa: E731
    fit()                                                                 # warm-up: allocations, LDS limits
    fit_ms, res = median_of(fit)
    passes = res["passes"]
    two_ms, _ = median_of(lambda: fit(max_iter=2))
    plain = lambda **kw: pl.fit_laplace("poisson", z, offset=offset + X @ res["beta"], tol=TOL, **kw)      # noqa: E731
    plain()
    plain_ms, plain_res = median_of(plain)
    python_loop(z, 2)
    loop_ms, (loop_passes, loop_beta) = median_of(lambda: python_loop(z))
    # the split on the device
    pl.set_option(P.MRA_OPT_KERNEL_TIMING, 1)
    timed_res = fit()
    ms = pl.buffer(14)
    all_kernels_ms = sum(k["ms"] for k in pl.kernel_stats())
    n_t = timed_res["passes"]
    tail_ms = ms[3] / n_t
    pass_ms = (all_kernels_ms - ms[3]) / n_t                              # (the tail's two kernels are counted among the small kernels too)
    sweeps_ms = (ms[0] + ms[1] + ms[2] + ms[4]) / n_t
    pl.set_option(P.MRA_OPT_KERNEL_TIMING, 0)
    tbps = lambda b: round(b / (tail_ms * 1e-3) / 1e12, 3) if tail_ms > 0 else None      # noqa: E731
    n_obs = int(seen.sum())
    useful = 8.0 * n_obs * (2 * p + 1 + 6)                                # m (1 + p), X (p), z, e, t, r, offset read; e written
    touched = 8.0 * topo.P * (2 * p + 1) + 8.0 * (topo.P + 5 * n_obs)
    out = {"config": "c3", "P": int(topo.P), "n_obs": n_obs, "family": "poisson", "p": p, "blocks": (p + 16) // 16, "tol": TOL, "repeats": reps,
           "set_trend_upload_ms": round(upload_ms, 2), "fit_ms": round(fit_ms, 3), "passes": passes, "converged": res["converged"],
           "fit_ms_per_iteration": round(fit_ms / passes, 3), "fit_2_passes_ms": round(two_ms, 3),
           "marginal_ms_per_iteration": round((fit_ms - two_ms) / max(passes - 2, 1), 3),
           "device_ms_per_iteration": {"pass": round(pass_ms, 3), "sweeps": round(sweeps_ms, 3), "tail": round(tail_ms, 4)},
           "trendless_fit_ms": round(plain_ms, 3), "trendless_passes": plain_res["passes"],
           "trendless_ms_per_iteration": round(plain_ms / plain_res["passes"], 3),
           "python_loop_ms": round(loop_ms, 3), "python_loop_passes": loop_passes, "python_loop_ms_per_iteration": round(loop_ms / loop_passes, 3),
           "tail_bytes_useful": useful, "tail_bytes_touched": touched, "tail_TBps_useful": tbps(useful), "tail_TBps_touched": tbps(touched),
           "tail_share_of_hbm_peak_touched": tbps(touched) and round(tbps(touched) * 1e12 / HBM_PEAK, 3),
           "beta_max_abs_diff_vs_python_loop": float(np.abs(res["beta"] - loop_beta).max()), "profile": res["profile"], "reml": res["reml"]}
    print(json.dumps(out), flush=True)
