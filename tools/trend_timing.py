"""Wall and device time of mra_trend_fit at BASELINE configs 3 and 5, with p = 3 and p = 63 covariates: the fit alone and the fit
with prediction, against HipPlan.solve on the same columns [y | X] - the path a caller had before the trend (columns from pageable
host memory on every call, means downloaded, the dense quad through MRA_SOLVE_FULL_QUAD).  Every timing is taken with the factors
valid, after a warm-up call of the same shape, as the median of three repeats; the first fit after an mra_run (one likelihood pass
with W at every row inside) and the first predicting call (two passes inside) are timed once.  The device times are those of a further call
with MRA_OPT_KERNEL_TIMING (one synchronisation per stage: a measuring mode, not part of the wall times), beside the bytes the
sweeps move: Ut once per block, the archive written once and read once.  One JSON line per configuration and p
(profiles/trend_timing.txt).

    python tools/trend_timing.py [c3] [c5]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pymra_amd import plan as P          # noqa: E402
from sample_timing import make, timed    # noqa: E402

HBM_TBS = 8.0                            # MI355X peak HBM bandwidth, TB/s


def med(fn):
    return float(np.median([timed(fn)[0] for _ in range(3)]))


def main(cfgs, ps=(3, 63)):
    for cfg in cfgs:
        pl, topo = make(cfg)
        N, Pn = int(topo.N), int(topo.P)
        y = np.nan_to_num(pl.buffer(11))                             # the observations by padded row
        pl.run(True, False)
        lik_ms = min(timed(lambda: pl.run(True, False))[0] for _ in range(3))
        for p in ps:
            X = np.random.default_rng(p).standard_normal((N, p))
            X[:, 0] = 1.0
            set_ms, _ = timed(lambda: pl.set_trend(X))
            pl.run(True, False)                                      # drops the factors: the next call makes them
            first_ms, _ = timed(lambda: pl.trend_fit())              # one likelihood pass with W at every row + the fit
            fit_ms = med(lambda: pl.trend_fit())
            first_pred_ms, _ = timed(lambda: pl.trend_fit(predict=True))      # a predict pass for the variance + the factors again
            pred_ms = med(lambda: pl.trend_fit(predict=True))
            pl.set_option(P.MRA_OPT_KERNEL_TIMING, 1)
            pl.trend_fit()
            dev_fit = pl.buffer(14)
            pl.trend_fit(predict=True)
            dev_pred = pl.buffer(14)
            pl.set_option(P.MRA_OPT_KERNEL_TIMING, 0)
            fit = pl.trend_fit(predict=True)
            # the same columns through HipPlan.solve: what the parent commit offered (its quad block-diagonal; the dense one is new)
            src = np.ascontiguousarray(topo.src)
            YX = np.empty((p + 1, Pn))
            YX[0] = y
            YX[1:] = np.where((np.asarray(topo.perm) >= 0)[None, :], X[src, :].T, 0.0)
            pl.solve(YX, want_mean=False, full_quad=True)
            solve_quad_ms = med(lambda: pl.solve(YX, want_mean=False, full_quad=True))
            solve_blockdiag_ms = med(lambda: pl.solve(YX, want_mean=False))
            solve_mean_ms = med(lambda: pl.solve(YX, full_quad=True))
            G = pl.solve(YX, want_mean=False, full_quad=True)[1]
            beta = np.linalg.solve(G[1:, 1:], G[1:, 0])
            nblk = (p + 16) // 16
            ut, arch = float(dev_fit[5]), float(dev_fit[6])
            moved = nblk * (ut + arch) + (nblk * arch if nblk > 1 else 0.0)      # forward sweeps: Ut once and the panel written per block; cross quad: every panel read once
            dev_sweeps = float(dev_fit[1] + dev_fit[2])
            print(json.dumps({
                "config": cfg, "P": Pn, "p": p, "blocks": nblk,
                "likelihood_pass_ms": round(lik_ms, 2), "set_trend_upload_ms": round(set_ms, 2),
                "fit_first_call_ms": round(first_ms, 2), "fit_ms": round(fit_ms, 2),
                "fit_predict_first_call_ms": round(first_pred_ms, 2), "fit_predict_ms": round(pred_ms, 2),
                "solve_quad_only_full_ms": round(solve_quad_ms, 2), "solve_quad_only_block_diagonal_ms": round(solve_blockdiag_ms, 2),
                "solve_mean_and_quad_ms": round(solve_mean_ms, 2),
                "device_ms_fit": {"stage": round(float(dev_fit[0]), 3), "sweeps": round(float(dev_fit[1]), 3), "cross_quad": round(float(dev_fit[2]), 3),
                                  "transfers": round(float(dev_fit[4]), 3)},
                "device_ms_fit_predict": {"stage": round(float(dev_pred[0]), 3), "sweeps": round(float(dev_pred[1]), 3),
                                          "cross_quad": round(float(dev_pred[2]), 3), "trend_rows": round(float(dev_pred[3]), 3),
                                          "transfers": round(float(dev_pred[4]), 3)},
                "bytes_Ut": ut, "bytes_archive_per_block": arch, "bytes_moved_fit": moved,
                "fit_sweeps_TBps": round(moved / (dev_sweeps * 1e-3) / 1e12, 3) if dev_sweeps > 0 else None,
                "fit_sweeps_share_of_hbm_peak": round(moved / (dev_sweeps * 1e-3) / 1e12 / HBM_TBS, 3) if dev_sweeps > 0 else None,
                "beta_max_abs_diff_vs_solve": float(np.abs(fit.beta - beta).max()), "finite": bool(np.isfinite(fit.mean).all() and np.isfinite(fit.var).all()),
            }), flush=True)
        pl.close()


if __name__ == "__main__":
    main(sys.argv[1:] or ["c3", "c5"])
