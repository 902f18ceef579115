"""The route table of tests/_route_cells.py covers the route space (no GPU): every member of the PassRoute enums and both values of
the switches that pick kernels are the expectation of at least one cell, so that tests/test_gpu_routes.py, which asserts each cell's
expectation through HipPlan.route(), has made every kernel family of the leaf stage run against the oracle."""
import os
import re

import _cases as K
import _route_cells as RC

# members that no cell can reach on one GPU, each with the route_for line that makes it so (at most two may be excused)
EXCUSED = {}

SWITCHES = ("solve_fused", "parent_front", "scatter_ut", "leaf_resident", "lik_rows", "lik_general", "side")


def _reached(routes):
    from pymra_amd import plan as P
    seen = {}
    for _, e in routes:
        for k, v in e.items():
            seen.setdefault(k, set()).add(v)
    missing = ["%s::%s" % (f, m) for f, members in P.ROUTE_ENUMS.items() for m in members if m not in seen.get(f, ())]
    missing += ["%s=%s" % (f, v) for f in SWITCHES for v in (False, True) if v not in seen.get(f, ())]
    return [m for m in missing if m not in EXCUSED]


def test_the_table_reaches_every_route_member():
    assert len(EXCUSED) <= 2
    assert _reached(RC.all_expected_routes()) == []


def test_deleting_the_only_row_of_a_member_is_noticed():
    """The coverage check bites: without the one sharded cell whose rank 0 sees no observation, LeafCFix::None is reported missing;
    without the cells of tree H, PassPath::Hi and LeafUpdate::InPredictHi are."""
    routes = RC.all_expected_routes()
    assert "c_fix::None" in _reached([(l, e) for l, e in routes if e.get("c_fix") != "None"])
    no_h = _reached([(l, e) for l, e in routes if not l.startswith("H ")])
    assert "path::Hi" in no_h and "update::InPredictHi" in no_h


def test_enum_numbers_are_those_of_the_header():
    """HipPlan.route() names the enum members by the MRA_ROUTE_* numbers of include/mra_hip.h, and the field list has the header's length."""
    from pymra_amd import plan as P
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    num = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MRA_ROUTE_\w+)\s+(\d+)", hdr)}
    assert num.pop("MRA_ROUTE_FIELDS") == len(P.ROUTE_FIELDS)
    prefix = {"path": "PATH", "c_fix": "CFIX", "chol": "CHOL", "var": "VAR", "update": "UPDATE"}
    snake = lambda s: re.sub(r"(?<!^)(?=[A-Z])", "_", s).upper()
    want = {"MRA_ROUTE_%s_%s" % (prefix[f], snake(m)): k for f, members in P.ROUTE_ENUMS.items() for k, m in enumerate(members)}
    assert want == num
    doc = hdr[hdr.index("the route of the last pass"):hdr.index("#define MRA_ROUTE_FIELDS")]
    listed = re.findall(r"(\d+) ([a-z_]+)", doc)
    assert [n for _, n in sorted(((int(k), n) for k, n in listed if n in P.ROUTE_FIELDS))] == list(P.ROUTE_FIELDS)


def test_edge_masks_hold_their_counts():
    """Every edge mask holds every intended count in one tree, small and large leaves interleaved, the first and the last leaf once
    empty and once the largest, and leaves on both sides of the 8-tile split where the leaves are large enough."""
    import numpy as np
    for t, recipe, cls, top in RC.EDGE_MASKS:
        topo, locs = RC.MK._tree(*RC.TREES[t])
        cnt = RC.MK.leaf_counts(topo, RC.make_obs(topo, locs, recipe))
        cap = RC.leaf_capacity(topo)
        want = set(c for c in RC.EDGE_COUNTS if c <= min(cap, 191)) | {top}
        assert want <= set(cnt.tolist()) and cnt.max() == top, (t, recipe)
        assert (cnt[0], cnt[-1]) == ((0, top) if recipe[1] == "empty_first" else (top, 0)), (t, recipe)
        small = RC.tiles(cnt) <= 8
        if cls != "small":
            assert 0 < small.sum() < len(cnt)
            runs = int(np.count_nonzero(np.diff(small.astype(int)))) + 1
            assert runs >= 10, (t, recipe, runs)              # small and large leaves alternate in leaf order, not "all small first"
