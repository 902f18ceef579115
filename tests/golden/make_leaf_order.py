#!/usr/bin/env python3
"""Generate leaf_order.npz: the level-wise CPU oracle (oracle/mra_levelwise.py) on the tree and mask of tests/_leaf_order_case.py -
its likelihood, and its predictive mean and sd at the sampled rows.  About 20 s.

    python tests/golden/make_leaf_order.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _leaf_order_case as LC                    # noqa: E402
from oracle.mra_levelwise import run_levelwise   # noqa: E402

topo, locs, obs, y = LC.build()
ref = run_levelwise(topo, locs, LC.MK._spec(), y, LC.R)
rows = LC.sample_rows(topo)
np.savez_compressed(LC.FIXTURE, lik=np.float64(ref["lik"]), rows=rows.astype(np.int64), mean=np.asarray(ref["mean"])[rows],
                    sd=np.asarray(ref["sd"])[rows], y_checksum=np.float64(np.nansum(y)), n_obs=np.int64(obs.sum()))
print("leaf_order.npz: %d rows, lik %.12g" % (len(rows), ref["lik"]))
