"""k_parent_front_pair without a GPU: what the compiler gave it, and MRA_OPT_PARENT_PAIR.

Two four-wave workgroups share a CU only if each wave stays within 256 registers, and the kernel is worth running only if those
registers hold the accumulators: no scratch, no AGPRs (tests/test_resource_usage.py holds every kernel to the last two; here the
instantiations are looked up by name, so that a build that lost them fails too).  The option is read on a plan built in host memory
(MRA_HOST_DRYRUN=1, as tests/test_leaf_order_cpu.py): default 1, 0 / 1 / 2 read back, anything else refused."""
import os
import subprocess
import sys

import pytest

import _cases as K

sys.path.insert(0, os.path.join(K.ROOT, "tools"))


@pytest.fixture(scope="module")
def usage(built_library):
    import resource_usage
    p = os.path.join(K.ROOT, "pymra_amd", "libmra_hip.resource_usage.txt")
    assert os.path.exists(p), "no resource-usage remarks next to the library"
    return resource_usage.parse(open(p).read())


@pytest.mark.parametrize("nacc", [17, 23])
def test_pair_kernel_fits_two_workgroups_per_cu(usage, nacc):
    hits = {n: r for n, r in usage.items() if "k_parent_front_pair<%d>" % nacc in n}
    assert len(hits) == 1, sorted(n for n in usage if "k_parent_front" in n)
    (name, r), = hits.items()
    print(name, r)
    assert r["scratch"] == 0 and r["spills"] == 0, r
    assert not r["agprs"], r
    assert r["vgprs"] is not None and r["vgprs"] <= 256, r
    assert r["occupancy"] is not None and r["occupancy"] >= 2, r
    assert r["lds"] == 0, r                     # (all of its LDS is dynamic: at most 64 KB, checked at plan build)


def test_the_eight_wave_kernels_are_still_there(usage):
    for nacc in (2, 4, 8, 12):
        assert any("k_parent_front<%d>" % nacc in n for n in usage), nacc


CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["MRA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRA_ROOT"], "tests"))
import test_gpu_likelihood_masks as MK
from pymra_amd import plan as P
topo, locs = MK._tree(64, 32, 3)
y = MK._y(np.random.RandomState(2).uniform(size=topo.N) < 0.4)
s = MK._spec()
pl = P.HipPlan(topo, 0)
pl.set_locs(locs); pl.set_obs(y, MK.R); pl.set_kernel(s.kind, s.l, s.sig, s.scale)
assert pl.get_option(P.MRA_OPT_PARENT_PAIR) == 1
for v in (0, 1, 2, 0, 2, 1):
    pl.set_option(P.MRA_OPT_PARENT_PAIR, v)
    assert pl.get_option(P.MRA_OPT_PARENT_PAIR) == v
    pl.set_obs(y, MK.R)                                  # the parents' descriptors (and the pair kernel's LDS size) again
    assert pl.get_option(P.MRA_OPT_PARENT_PAIR) == v
for bad in (-1, 3, 23):
    try:
        pl.set_option(P.MRA_OPT_PARENT_PAIR, bad)
        raise SystemExit("option 23 = %d must be refused" % bad)
    except P.MraError as e:
        assert e.code == -1, e.code
assert pl.get_option(P.MRA_OPT_PARENT_PAIR) == 1
pl.close()
print("PARENT_PAIR_CPU_OK")
'''


def test_option_defaults_to_one_round_trips_and_refuses_other_values(built_library, tmp_path):
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, MRA_ROOT=K.ROOT, MRA_HOST_DRYRUN="1", OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1")
    res = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "PARENT_PAIR_CPU_OK" in res.stdout, (res.stdout + res.stderr)[-3000:]


def test_option_is_declared_in_the_header_and_the_binding():
    from pymra_amd import plan
    assert plan.MRA_OPT_PARENT_PAIR == 23
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    assert "#define MRA_OPT_PARENT_PAIR    23" in hdr and "k_parent_front_pair" in hdr
