"""MRA_OPT_LEAF_ORDER without a GPU: the plan's leaf lists are built in host memory (MRA_HOST_DRYRUN=1) with the option at every
value, on masks with no oversized leaf (more than eight observation tiles), with one, and with nothing else; the option reads back
what was set and refuses other values.  A dry-run plan cannot run a pass (tests/test_asan_host.py pins that), so there is no route to
read here: that the route read-back does not depend on the option is asserted on the GPU, tests/test_gpu_leaf_order.py."""
import os
import subprocess
import sys

import _cases as K

CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["MRA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRA_ROOT"], "tests"))
import _route_cells as RC
import test_gpu_likelihood_masks as MK
from pymra_amd import plan as P
topo, locs = MK._tree(96, 16, 3)                  # 64 leaves of 144 rows
leaves = [int(i) for i in np.nonzero(topo.node_leaf)[0]]
rng = np.random.RandomState(2)
thin = rng.uniform(size=topo.N) < 0.4
one = thin.copy(); MK._exact(one, topo, leaves[9], 144, rng)
masks = {"none": thin, "one": one, "all": np.ones(topo.N, dtype=bool)}
over = {k: int((RC.tiles(MK.leaf_counts(topo, m)) > 8).sum()) for k, m in masks.items()}
assert over == {"none": 0, "one": 1, "all": 64}, over
s = MK._spec()
n = 0
for name, m in masks.items():
    y = MK._y(m)
    pl = P.HipPlan(topo, 0)
    pl.set_locs(locs); pl.set_obs(y, MK.R); pl.set_kernel(s.kind, s.l, s.sig, s.scale)
    assert pl.get_option(P.MRA_OPT_LEAF_ORDER) == 1                      # the default: both parts on
    for v in (0, 1, 2, 3, 4, 1):
        pl.set_option(P.MRA_OPT_LEAF_ORDER, v)
        assert pl.get_option(P.MRA_OPT_LEAF_ORDER) == v
        pl.set_obs(y, MK.R)                                              # the leaf lists again, in the order the option asks for
        assert pl.info()["n_leaves"] == 64
        try:
            pl.run(True, True)
            raise SystemExit("a dry-run plan must refuse to run")
        except P.MraError as e:
            assert e.code == -4
        n += 1
    for bad in (-1, 5):
        try:
            pl.set_option(P.MRA_OPT_LEAF_ORDER, bad)
            raise SystemExit("option 22 = %d must be refused" % bad)
        except P.MraError as e:
            assert e.code == -1, e.code
    assert pl.get_option(P.MRA_OPT_LEAF_ORDER) == 1
    pl.close()
print("LEAF_ORDER_CPU_OK", n)
'''


def test_leaf_lists_build_with_every_setting_on_three_masks(built_library, tmp_path):
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, MRA_ROOT=K.ROOT, MRA_HOST_DRYRUN="1", OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1")
    res = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "LEAF_ORDER_CPU_OK 18" in res.stdout, (res.stdout + res.stderr)[-3000:]


def test_option_is_declared_in_the_header_and_the_binding():
    from pymra_amd import plan
    assert plan.MRA_OPT_LEAF_ORDER == 22
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    assert "#define MRA_OPT_LEAF_ORDER     22" in hdr and "next mra_plan_set_obs" in hdr
