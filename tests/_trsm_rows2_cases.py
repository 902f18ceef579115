"""The problems, pass scripts and digests of tests/test_gpu_trsm_rows2.py and tests/golden/make_trsm_rows2.py.

The leaves' row solve (k_trsm_rows2, body trsm2_row_tile) at the shapes where its paths differ: a leaf with no observation (nt = 0:
the body's early return), fully observed leaves, leaf after leaf with 1 and 8 observation tiles (the widest image of the <8>
instance), ragged last tiles, gathered Ut tiles alone (likelihood-only passes, and the default route of trees with at most two leaves
per CU) and gathered + streamed tiles (MRA_OPT_LEAF_SOLVE 0), in place and out of place (MRA_OPT_RESID_REUSE: Trsm2Prob::src), a
noise vector, a new mask.

Shapes: g64 - the 64 x 64 grid, M = 3, J = 4, r0 = 16: 64 leaves of 64 rows, at most 4 observation tiles, every pass in place;
A - tests/_route_cells.py's 128 x 128 tree: 64 leaves of 256 rows, 8 tiles = 128 observations, predict passes read the kept residual;
L16s - the 1-D ternary tree of tests/_line_cells.py: 27 leaves of 80 to 96 rows.

A script is: predict, predict (kept), likelihood-only, predict under a noise vector, predict and likelihood-only after set_obs with
another mask, then mra_cv by row (it reads the retained Ut and Tt).  Its digest holds, per pass, the likelihood terms (as hex floats),
SHA-256 of mean, var and of four leaves' panels [Lc ; Ut ; Tt], and 16 sampled values of mean and var for a reader of a failure."""
import functools
import hashlib

import numpy as np

import _line_cells as LC
import _route_cells as RC
import test_gpu_likelihood_masks as MK
import test_gpu_prior_reuse as PR

IN_CASCADE = PR.IN_CASCADE                  # MRA_OPT_LEAF_SOLVE 0: the row solve has the full list, Ut and Tt tiles
LEAF_ORDER_OFF = ((22, 0),)                 # launch order = leaf order: the alternating masks change the image size leaf after leaf
RESID_OFF = ((25, 0),)                      # every pass in place
CASES = [("g64", ()), ("g64", IN_CASCADE), ("g64", IN_CASCADE + LEAF_ORDER_OFF),
         ("A", ()), ("A", IN_CASCADE), ("A", IN_CASCADE + LEAF_ORDER_OFF), ("A", IN_CASCADE + RESID_OFF), ("A", LEAF_ORDER_OFF + RESID_OFF),
         ("L16s", ()), ("L16s", IN_CASCADE)]


def case_id(key, opts):
    return "%s-%s" % (key, "_".join("%d=%d" % o for o in opts) or "default")


def _alternating(topo, counts, shift, seed):
    """leaf k of the leaf order observes counts[(k + shift) % len(counts)] of its rows"""
    rng = np.random.RandomState(seed)
    obs = np.zeros(topo.N, dtype=bool)
    for k, i in enumerate(np.nonzero(topo.node_leaf)[0]):
        MK._exact(obs, topo, int(i), counts[(k + shift) % len(counts)], rng)
    return obs


@functools.lru_cache(maxsize=None)
def problem(key):
    """(topology, locations, kernel spec, R, y, y of a second mask)"""
    if key == "g64":            # no observation, 1 tile, fully observed (4 tiles), 2 tiles with a ragged last one
        topo, locs = MK._tree(64, 16, 3)
        counts = (0, 10, RC.leaf_capacity(topo), 17)
    elif key == "A":            # 1 tile beside 8 tiles, leaf after leaf; one leaf in eight without any observation
        topo, locs = MK._tree(*RC.TREES["A"])
        counts = (0, 128, 1, 127, 16, 128, 10, 113)
    else:
        topo, locs = LC.tree(key)
        obs = LC.default_mask(topo)
        obs[MK._leaf_callers(topo, LC.leaves(topo)[5])] = True                   # one leaf fully observed (the first has none)
        obs2 = LC.default_mask(topo, seed=3)
        return topo, locs, LC.M32, LC.R, LC.values(locs, obs), LC.values(locs, obs2, seed=1)
    obs, obs2 = _alternating(topo, counts, 0, 2), _alternating(topo, counts, 3, 5)
    t = RC.tiles(MK.leaf_counts(topo, obs))
    assert t.min() == 0 and t.max() == (4 if key == "g64" else 8) and np.any(np.abs(np.diff(t)) >= 3)
    return topo, locs, MK._spec(), MK.R, MK._y(obs, seed=2), MK._y(obs2, seed=4)


def watched(topo):
    lv = [int(i) for i in np.nonzero(topo.node_leaf)[0]]
    return [lv[0], lv[len(lv) // 3], lv[len(lv) // 2 + 1], lv[-1]]


def _snap(hip, pl, predict, watch):
    pl.run(True, predict)
    mean, var = pl.predict() if predict else (None, None)
    return dict(lik=pl.likelihood(), mean=mean, var=var, route=pl.route(), panels=[pl.node_block(i, hip.MRA_BLOCK_LEAF) for i in watch])


def run_script(hip, key, opts):
    """-> (the six passes' results, mra_cv's outputs)"""
    topo, locs, spec, R, y, y2 = problem(key)
    watch = watched(topo)
    noise = np.random.RandomState(9).uniform(0.5 * R, 3.0 * R, size=topo.N)
    pl = PR._plan(hip, topo, locs, y, spec=spec, opts=tuple(opts), noise=R)
    out = [_snap(hip, pl, True, watch), _snap(hip, pl, True, watch), _snap(hip, pl, False, watch)]
    pl.set_noise(noise)
    out.append(_snap(hip, pl, True, watch))
    pl.set_obs(y2, R)
    out.append(_snap(hip, pl, True, watch))
    out.append(_snap(hip, pl, False, watch))
    cv = pl.cv()
    pl.close()
    return out, cv


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def digest(passes, cv):
    d = []
    for p in passes:
        e = dict(lik=[float(v).hex() for v in p["lik"]], panels=[_sha(a) for a in p["panels"]])
        if p["mean"] is not None:
            idx = np.linspace(0, len(p["mean"]) - 1, 16).astype(int)
            e.update(mean=_sha(p["mean"]), var=_sha(p["var"]), mean_sample=[float(v).hex() for v in np.asarray(p["mean"])[idx]],
                     var_sample=[float(v).hex() for v in np.asarray(p["var"])[idx]])
        d.append(e)
    return dict(passes=d, cv=[_sha(a) for a in cv[:4]])
