"""Helpers for the sampler tests: the latent slot layout of include/mra_hip.h (mra_sample) restated from the topology, factor
columns G[:, slots] from unit-z draws restricted to chosen slots, and Sigma assembled from the reference's per-node goldens."""
import numpy as np

import _cases as K


def reported(topo):
    """Padded rows a draw reports: real rows inside a leaf."""
    return (topo.perm >= 0) & np.asarray(topo.in_leaf, dtype=bool)


def coarse_offsets(topo):
    """({non-leaf node: first latent slot}, Kn): the non-leaf nodes in node order, cw[level] slots each."""
    zoff, k = {}, 0
    for i in range(len(topo.node_row0)):
        if not topo.node_leaf[i]:
            zoff[i] = k
            k += int(topo.cw[topo.node_level[i]])
    return zoff, k


def leaf_of_row(topo, row):
    leaves = np.nonzero(np.asarray(topo.node_leaf, dtype=bool))[0]
    hit = leaves[(np.asarray(topo.node_row0)[leaves] <= row) & (row < np.asarray(topo.node_row1)[leaves])]
    assert len(hit) == 1
    return int(hit[0])


def ancestor_slots(topo, j, zoff=None):
    """The cw[level] slots of every ancestor of node j, root last."""
    if zoff is None:
        zoff, _ = coarse_offsets(topo)
    slots = []
    p = int(topo.node_parent[j])
    while p >= 0:
        slots.extend(range(zoff[p], zoff[p] + int(topo.cw[topo.node_level[p]])))
        p = int(topo.node_parent[p])
    return slots


def knot_slots(topo, j, Kn):
    """Leaf j's own terms: slot Kn + knot row."""
    return [Kn + int(r) for r in topo.knot_rows[topo.knot_ptr[j]:topo.knot_ptr[j + 1]]]


def chain_slots(topo, j, zoff=None, Kn=None):
    """Every slot a row of leaf j reads in a prior draw: its ancestors' slots and its own knot-row slots."""
    if zoff is None:
        zoff, Kn = coarse_offsets(topo)
    return ancestor_slots(topo, j, zoff) + knot_slots(topo, j, Kn)


def factor_columns(pl, slots, rows=None, conditional=False, chunk=64):
    """G[rows, slots] with G[:, k] = sample(z = e_k) (prior) or sample(e_k) - sample(0) (conditional); rows=None: all P rows.
    Also returns sample(0)[rows] (zero for the prior)."""
    slots = np.asarray(slots, dtype=np.int64)
    n = pl.sample_slots()
    sel = slice(None) if rows is None else np.asarray(rows)
    x0 = pl.sample(1, z=np.zeros((1, n)), conditional=conditional)[0][sel] if conditional else 0.0
    cols = []
    for a in range(0, len(slots), chunk):
        s = slots[a:a + chunk]
        z = np.zeros((len(s), n))
        z[np.arange(len(s)), s] = 1.0
        cols.append((pl.sample(len(s), z=z, conditional=conditional)[:, sel] - x0).T)
    G = np.concatenate(cols, axis=1) if cols else np.zeros((pl.topo.P if rows is None else len(rows), 0))
    return G, x0


def golden_prior_sigma(name, topo):
    """Sigma over the padded rows from the reference's per-node B and kC (k = kC kC^T), tests/golden/<name>_nodes.npz."""
    gold = K.load_node_goldens(name)
    S = np.zeros((topo.P, topo.P))
    for i in range(len(topo.node_row0)):
        g = gold[topo.node_ident[i]]
        rows = K.node_real_rows(topo, i)
        B, kC = np.asarray(g["B"]), np.asarray(g["kC"])
        assert B.shape[0] == len(rows)
        BK = B @ kC
        S[np.ix_(rows, rows)] += BK @ BK.T
    return S
