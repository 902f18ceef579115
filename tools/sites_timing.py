"""Wall and stream time of mra_predict_sites at BASELINE config 3: 2^20 sites - the 1024^2 grid shifted by half a cell - with the factors
already valid (the first call, which runs the one likelihood pass and allocates the work buffers, is timed apart), mean and variance for
the plan's own observations, medians of three in one process.  A second set of three runs with MRA_OPT_KERNEL_TIMING on gives the
stream time split by kernel, the solver's sweeps, the uploads and the downloads (events on the plan's stream; one synchronisation per
launch, so their wall time is not quoted).  Against it, what the same answer costs without the entry point: a second MRATree on
locs + sites with NaN observations at the sites, end to end (construction, likelihood + predict pass, predict()).
Prints one JSON line per configuration (profiles/sites_timing.txt).

    python tools/sites_timing.py [c3]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import pymra_amd.MRATools as mt                          # noqa: E402
from pymra_amd import MRATree, plan as P                 # noqa: E402

PARTS = ("basis", "leaf", "chain", "mean", "solver_sweeps", "upload", "download")


def timed(fn):
    P.device_synchronize(0)
    t0 = time.perf_counter()
    out = fn()
    P.device_synchronize(0)
    return 1e3 * (time.perf_counter() - t0), out


def main(cfgs):
    import make_golden as mg
    for cfg in cfgs:
        c = mg.CASES[cfg]
        locs, y_obs, _ = mg.make_inputs(c)
        cov = lambda a, b=np.array([]): mt.Matern32(a, b, l=c["l"], sig=c["sig"])      # noqa: E731
        build_ms, tree = timed(lambda: MRATree(locs, c["r"], cov, y_obs, c["R"], M=c["M"], J=c["J"], verbose=False))
        pl = tree.plan
        n = int(round(np.sqrt(len(locs))))
        sites = locs + 0.5 * (locs.max(0) - locs.min(0)) / (n - 1)
        locate_ms, leaf = timed(lambda: tree.locate(sites))
        first_ms, _ = timed(lambda: pl.predict_sites(sites, leaf))                     # factorises: one likelihood pass inside
        wall = sorted(timed(lambda: pl.predict_sites(sites, leaf))[0] for _ in range(3))[1]
        var_only = sorted(timed(lambda: pl.lib.mra_predict_sites(pl._h, 0, len(sites), P._ptr(sites), P._ptr(leaf), 1, None, None,
                                                                   P._ptr(np.empty(len(sites)))))[0] for _ in range(3))[1]
        pl.set_option(P.MRA_OPT_KERNEL_TIMING, 1)
        parts = []
        for _ in range(3):
            mean, var = pl.predict_sites(sites, leaf)
            parts.append(pl.buffer(7))
        pl.set_option(P.MRA_OPT_KERNEL_TIMING, 0)
        parts = np.median(np.array(parts), axis=0)
        info = pl.info()
        t = tree.topology
        rows = np.nonzero((t.perm >= 0) & np.asarray(t.in_leaf, dtype=bool))[0]
        leaf_of = np.zeros(t.P, dtype=np.int64)
        for i in np.nonzero(np.asarray(t.node_leaf, dtype=bool))[0]:
            leaf_of[int(t.node_row0[i]):int(t.node_row1[i])] = i
        ob = np.isfinite(np.asarray(y_obs, float).ravel())[t.perm[rows]]
        nop_max = (int(np.bincount(leaf_of[rows][ob]).max()) + 15) // 16 * 16
        tile_bytes = 8 * 16 * (2 * info["Ka"] + nop_max + locs.shape[1] + 1 + 16) + 4      # mra_sites_tile_bytes
        n_tiles = int(sum((c + 15) // 16 for c in np.bincount(leaf)))
        # the parent commit's way: the sites as extra rows of a new tree
        both = np.vstack([locs, sites])
        y_both = np.vstack([np.asarray(y_obs, float).reshape(-1, 1), np.full((len(sites), 1), np.nan)])

        def rebuild():
            t = MRATree(both, c["r"], cov, y_both, c["R"], M=c["M"], J=c["J"], verbose=False)
            return t.predict()
        rebuild_ms = sorted(timed(rebuild)[0] for _ in range(3))[1]
        out = {"config": cfg, "P": info["P"], "n_sites": len(sites), "n_tiles": n_tiles, "tile_work_bytes": tile_bytes, "tiles_per_default_chunk": (256 << 20) // tile_bytes,
               "tree_build_and_pass_ms": round(build_ms, 1), "locate_ms": round(locate_ms, 1),
               "predict_sites_first_call_ms": round(first_ms, 1), "predict_sites_wall_ms": round(wall, 1),
               "predict_sites_var_only_wall_ms": round(var_only, 1),
               "stream_ms": {k: round(float(v), 2) for k, v in zip(PARTS, parts)}, "stream_ms_kernels": round(float(parts[:4].sum()), 2),
               "second_tree_on_locs_and_sites_ms": round(rebuild_ms, 1),
               "finite": bool(np.isfinite(mean).all() and np.isfinite(var).all())}
        print(json.dumps(out), flush=True)
        pl.close()


if __name__ == "__main__":
    main(sys.argv[1:] or ["c3"])
