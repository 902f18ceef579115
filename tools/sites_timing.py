"""Wall and stream time of mra_predict_sites at BASELINE config 3: 2^20 sites - the 1024^2 grid shifted by half a cell - with the factors
already valid (the first call, which runs the one likelihood pass and allocates the work buffers, is timed apart), mean and variance for
the plan's own observations, medians of three in one process.  A second set of three runs with MRA_OPT_KERNEL_TIMING on gives the
stream time split by kernel, the solver's sweeps, the uploads and the downloads (events on the plan's stream; one synchronisation per
launch, so their wall time is not quoted).  Against it, what the same answer costs without the entry point: a second MRATree on
locs + sites with NaN observations at the sites, end to end (construction, likelihood + predict pass, predict()).
Prints one JSON line per configuration (profiles/sites_timing.txt).

    python tools/sites_timing.py [c3]

`cov` mode: mra_sites_cov at the same configuration, 4096 and 16384 sites of the shifted grid taken in WHOLE leaves - one family of four
siblings, a cousin family and leaves spread over the rest of the domain, so that tile pairs with every depth of lowest common ancestor
occur -, prior and posterior, medians of three with the factors valid; with MRA_OPT_KERNEL_TIMING the stream times of
mra_get_buffer(what = 8).  Against it the only way to the same numbers without the entry point: a second MRATree on locs + sites and
covariance(rows) in n / 16 sweeps - a DIFFERENT model (other knots), timed at 4096 sites.  One JSON line per site count
(profiles/sitecov_timing.txt).

    python tools/sites_timing.py cov [c3]

`draw` mode: mra_sample_sites at the same configuration, 16 prior and 16 posterior draws from a seed with the factors valid, medians of
three, wall and - with MRA_OPT_KERNEL_TIMING - the stream times of mra_get_buffer(what = 9): (a) the 2^20 sites of the shifted grid, 256
sites = 16 tiles in every leaf; (b) a 4 x 4 refinement of 64 leaves, 4096 sites = 256 tiles per leaf (MRA_SAMPLE_SITES_LEAF_MAX: a
block of 128 MiB each), once with all 64 leaves in one batch (MRA_OPT_SITES_CHUNK_BYTES = 12 GiB) and once, a single run, with the
default 256 MiB (one leaf per batch: the 64 Cholesky factorisations run one after the other on one compute unit each).  Last, the parent
commit's way at its cap: MRATree.simulateAt on 16384 sites (dense matrix + numpy.linalg.eigh on the host).  One JSON line each
(profiles/sitedraw_timing.txt).

    python tools/sites_timing.py draw [c3]
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


COV_PARTS = ("basis", "leaf", "chain", "gram", "upload", "download")


def whole_leaves(t, leaf, count):
    """indices of `count` sites in whole leaves: the first family, a cousin family, then leaves spread evenly over the leaf list"""
    leaves = np.nonzero(np.asarray(t.node_leaf, dtype=bool))[0]
    par = np.asarray(t.node_parent)
    fam = [j for j in leaves if par[j] == par[leaves[0]]]
    cousins = [j for j in leaves if par[j] != par[leaves[0]] and par[par[j]] == par[par[leaves[0]]]]
    cousins = [j for j in cousins if par[j] == par[cousins[0]]]
    per = max(1, int(np.bincount(leaf).max()))
    rest = [j for j in leaves[np.linspace(0, len(leaves) - 1, max(2, 2 * count // per)).astype(int)] if j not in fam and j not in cousins]
    idx = np.concatenate([np.nonzero(leaf == j)[0] for j in fam + cousins + rest])
    assert len(idx) >= count
    return idx[:count]


def main_cov(cfgs):
    import make_golden as mg
    for cfg in cfgs:
        c = mg.CASES[cfg]
        locs, y_obs, _ = mg.make_inputs(c)
        cov = lambda a, b=np.array([]): mt.Matern32(a, b, l=c["l"], sig=c["sig"])      # noqa: E731
        tree = MRATree(locs, c["r"], cov, y_obs, c["R"], M=c["M"], J=c["J"], verbose=False)
        pl = tree.plan
        n = int(round(np.sqrt(len(locs))))
        grid = locs + 0.5 * (locs.max(0) - locs.min(0)) / (n - 1)
        leaf_all = tree.locate(grid)
        info = pl.info()
        for count in (4096, 16384):
            idx = whole_leaves(tree.topology, leaf_all, count)
            sites, leaf = np.ascontiguousarray(grid[idx]), np.ascontiguousarray(leaf_all[idx])
            n_tiles = int(sum((k + 15) // 16 for k in np.bincount(leaf)))
            out = {"config": cfg, "P": info["P"], "Ka": info["Ka"], "n_sites": count, "n_leaves": int(len(np.unique(leaf))), "n_tiles": n_tiles,
                   "result_bytes": 8 * count * count}
            for kind, post in (("prior", False), ("posterior", True)):
                first_ms, _ = timed(lambda: pl.sites_cov(sites, leaf, posterior=post))      # the very first call factorises and allocates
                wall = sorted(timed(lambda: pl.sites_cov(sites, leaf, posterior=post))[0] for _ in range(3))[1]
                pl.set_option(P.MRA_OPT_KERNEL_TIMING, 1)
                parts = []
                for _ in range(3):
                    S = pl.sites_cov(sites, leaf, posterior=post)
                    parts.append(pl.buffer(8))
                pl.set_option(P.MRA_OPT_KERNEL_TIMING, 0)
                parts = np.median(np.array(parts), axis=0)
                out[kind] = {"first_call_ms": round(first_ms, 1), "wall_ms": round(wall, 1),
                             "stream_ms": {k: round(float(v), 2) for k, v in zip(COV_PARTS, parts)},
                             "symmetric": bool(np.array_equal(S, S.T)), "finite": bool(np.isfinite(S).all())}
            if count == 4096:
                both = np.vstack([locs, sites])
                y_both = np.vstack([np.asarray(y_obs, float).reshape(-1, 1), np.full((count, 1), np.nan)])
                rows = np.arange(len(locs), len(both))

                def rebuild():
                    t2 = MRATree(both, c["r"], cov, y_both, c["R"], M=c["M"], J=c["J"], verbose=False)
                    return np.vstack([t2.covariance(rows[k:k + 16], distr="posterior")[rows] for k in range(0, count, 16)])
                out["second_tree_covariance_in_sweeps_ms"] = round(timed(rebuild)[0], 1)
            print(json.dumps(out), flush=True)
        pl.close()


DRAW_PARTS = ("basis", "leaf", "chain", "leaf_gram", "leaf_cholesky", "draw", "mean_and_sweeps", "upload", "download")


def draw_case(pl, sites, leaf, reps, timed_reps):
    out = {}
    for kind, post in (("prior", False), ("posterior", True)):
        first_ms, x = timed(lambda: pl.sample_sites(sites, leaf, 16, seed=1, posterior=post))
        rec = {"first_call_ms": round(first_ms, 1), "finite": bool(np.isfinite(x).all())}
        if reps:
            rec["wall_ms"] = round(sorted(timed(lambda: pl.sample_sites(sites, leaf, 16, seed=1, posterior=post))[0] for _ in range(reps))[reps // 2], 1)
        pl.set_option(P.MRA_OPT_KERNEL_TIMING, 1)
        parts = []
        for _ in range(timed_reps):
            pl.sample_sites(sites, leaf, 16, seed=1, posterior=post)
            parts.append(pl.buffer(9))
        pl.set_option(P.MRA_OPT_KERNEL_TIMING, 0)
        parts = np.median(np.array(parts), axis=0)
        rec["stream_ms"] = {k: round(float(v), 2) for k, v in zip(DRAW_PARTS, parts)}
        rec["stream_ms_kernels"] = round(float(parts[:7].sum()), 2)
        out[kind] = rec
    return out


def main_draw(cfgs):
    import make_golden as mg
    for cfg in cfgs:
        c = mg.CASES[cfg]
        locs, y_obs, _ = mg.make_inputs(c)
        cov = lambda a, b=np.array([]): mt.Matern32(a, b, l=c["l"], sig=c["sig"])      # noqa: E731
        tree = MRATree(locs, c["r"], cov, y_obs, c["R"], M=c["M"], J=c["J"], verbose=False)
        pl = tree.plan
        n = int(round(np.sqrt(len(locs))))
        cell = (locs.max(0) - locs.min(0)) / (n - 1)
        grid = locs + 0.5 * cell
        leaf_all = tree.locate(grid)
        info = pl.info()
        pl.predict_sites(grid[:16], leaf_all[:16])            # the factors: one likelihood pass, not part of any figure below
        # (a) the whole shifted grid
        out = {"config": cfg, "case": "shifted grid", "P": info["P"], "Ka": info["Ka"], "n_sites": len(grid), "n_leaves": int(len(np.unique(leaf_all))),
               "sites_per_leaf_max": int(np.bincount(leaf_all).max()), "n_samples": 16, "chunk_bytes": "default (256 MiB)"}
        out.update(draw_case(pl, grid, leaf_all, 3, 3))
        print(json.dumps(out), flush=True)
        # (b) 64 leaves refined 4 x 4
        t = tree.topology
        leaves = np.nonzero(np.asarray(t.node_leaf, dtype=bool))[0]
        some = leaves[np.linspace(0, len(leaves) - 1, 64).astype(int)]
        off = np.stack(np.meshgrid((np.arange(4) + 0.5) / 4 - 0.5, (np.arange(4) + 0.5) / 4 - 0.5, indexing="ij"), -1).reshape(-1, 2) * cell
        sites, leaf = [], []
        for i in some:
            p = t.perm[int(t.node_row0[i]):int(t.node_row1[i])]
            own = locs[p[p >= 0]]
            sites.append((own[:, None, :] + off[None, :, :]).reshape(-1, 2))
            leaf.append(np.full(len(own) * 16, i, dtype=np.int32))
        sites, leaf = np.ascontiguousarray(np.vstack(sites)), np.concatenate(leaf)
        base = {"config": cfg, "case": "4 x 4 refinement of 64 leaves", "n_sites": len(sites), "n_leaves": 64, "sites_per_leaf_max": int(np.bincount(leaf).max()),
                "n_samples": 16, "block_bytes_per_leaf": 8 * int(np.bincount(leaf).max()) ** 2}
        pl.set_option(P.MRA_OPT_SITES_CHUNK_BYTES, 12 << 30)
        out = dict(base, chunk_bytes="12 GiB (one batch)")
        out.update(draw_case(pl, sites, leaf, 3, 3))
        print(json.dumps(out), flush=True)
        pl.set_option(P.MRA_OPT_SITES_CHUNK_BYTES, 0)
        out = dict(base, chunk_bytes="default (256 MiB: one leaf per batch)", runs="single")
        out.update(draw_case(pl, sites, leaf, 0, 1))
        print(json.dumps(out), flush=True)
        # the parent commit's way, at its cap
        idx = whole_leaves(t, leaf_all, P.MRA_SITES_COV_MAX)
        s16, l16 = np.ascontiguousarray(grid[idx]), np.ascontiguousarray(leaf_all[idx])
        ms, x = timed(lambda: tree.simulateAt(s16, 16, distr="posterior", seed=1, leaf=l16))
        ms2, x2 = timed(lambda: tree.sampleAt(s16, 16, distr="posterior", seed=1, leaf=l16))
        print(json.dumps({"config": cfg, "case": "simulateAt (dense matrix + eigh on the host) at its cap", "n_sites": len(idx), "n_samples": 16,
                          "simulateAt_wall_ms": round(ms, 1), "sampleAt_same_sites_wall_ms": round(ms2, 1),
                          "finite": bool(np.isfinite(x).all() and np.isfinite(x2).all())}), flush=True)
        pl.close()


if __name__ == "__main__":
    if sys.argv[1:2] == ["draw"]:
        main_draw(sys.argv[2:] or ["c3"])
    elif sys.argv[1:2] == ["cov"]:
        main_cov(sys.argv[2:] or ["c3"])
    else:
        main(sys.argv[1:] or ["c3"])
