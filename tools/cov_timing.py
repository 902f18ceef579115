"""Wall time of mra_cov_apply at BASELINE configs 3 and 5: 16 prior and 16 posterior columns with the factors already valid (the
first call, which runs the one likelihood pass and allocates the work buffers, is timed apart), each as the median of three repeats,
upload of the 16 x P input and download of the 16 x P result included; the same with gram only (no download), and mra_solve for 16
columns on the same plan for comparison.  Prints one JSON line per configuration (profiles/cov_timing.txt).

    python tools/cov_timing.py [c3] [c5]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sample_timing import make, timed          # noqa: E402  (the plans of tools/sample_timing.py)


def main(cfgs):
    for cfg in cfgs:
        pl, topo = make(cfg)
        pl.run(True, True)
        pass_ms = min(timed(lambda: pl.run(True, True))[0] for _ in range(3))
        rep = (topo.perm >= 0) & np.asarray(topo.in_leaf, dtype=bool)
        A = np.zeros((16, topo.P))
        A[:, rep] = np.random.default_rng(5).standard_normal((16, int(rep.sum())))
        med = lambda fn: float(np.median([timed(fn)[0] for _ in range(3)]))          # noqa: E731
        first_ms, _ = timed(lambda: pl.cov_apply(A))                                  # factorises: one likelihood pass inside
        prior_ms = med(lambda: pl.cov_apply(A))
        first_post_ms, _ = timed(lambda: pl.cov_apply(A, posterior=True))             # the solver's buffers are there already
        post_ms = med(lambda: pl.cov_apply(A, posterior=True))
        prior_gram_ms = med(lambda: pl.cov_apply(A, want_out=False))
        post_gram_ms = med(lambda: pl.cov_apply(A, posterior=True, want_out=False))
        solve_ms = med(lambda: pl.solve(A))
        out, gram = pl.cov_apply(A, posterior=True)
        print(json.dumps({"config": cfg, "P": int(topo.P), "n_nodes": int(topo.n_nodes), "lik_predict_pass_ms": round(pass_ms, 2),
                          "cov_16_prior_first_call_ms": round(first_ms, 2), "cov_16_prior_ms": round(prior_ms, 2),
                          "cov_16_posterior_first_call_ms": round(first_post_ms, 2), "cov_16_posterior_ms": round(post_ms, 2),
                          "cov_16_prior_gram_only_ms": round(prior_gram_ms, 2), "cov_16_posterior_gram_only_ms": round(post_gram_ms, 2),
                          "solve_16_columns_factors_valid_ms": round(solve_ms, 2),
                          "finite": bool(np.isfinite(out).all() and np.isfinite(gram).all())}), flush=True)
        pl.close()


if __name__ == "__main__":
    main(sys.argv[1:] or ["c3", "c5"])
