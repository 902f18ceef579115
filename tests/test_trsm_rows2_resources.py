"""k_trsm_rows2 without a GPU: what the compiler gave the row-tile body (trsm2_row_tile) in every instance.

A wave keeps the whole row of tiles x[NTMAX] in registers from its loads to its stores.  The body walks the column tiles through
trsm2_steps (nested compile-time steps, not an unrolled loop), in a gathered and a streamed instance; if the compiler stops
resolving x[jb] at compile time the row lands in scratch memory - a loop with early exits did exactly that to the <12> instance, 416
bytes per lane, while the narrower ones stayed clean.  So: no scratch, no spilled VGPR, no AGPR copies in any of the four
instances, and the <8> one within 128 registers.  Read from the remarks of the product build, as tests/test_resource_usage.py reads them; the instances are looked up by name,
so that a build that lost one fails too."""
import os
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


def _one(usage, name):
    hits = {n: r for n, r in usage.items() if name + "(" in n}
    assert len(hits) == 1, sorted(n for n in usage if "k_trsm_rows2" in n)
    (full, r), = hits.items()
    print(full, r)
    return r


@pytest.mark.parametrize("nt", [2, 4, 8, 12])
def test_row_solve_instances_keep_the_row_in_registers(usage, nt):
    """(tests/test_resource_usage.py holds <4>, <8> and <12> to zero scratch and no AGPRs among all kernels; here each of the four is
    looked up by name, and a spilled VGPR fails too)"""
    r = _one(usage, "k_trsm_rows2<%d>" % nt)
    assert r["scratch"] == 0 and r["spills"] == 0, r
    assert not r["agprs"], r


def test_the_small_leaves_instance_stays_within_128_registers(usage):
    """k_trsm_rows2<8> takes the small leaves of a fused pass.  At no more than 128 registers sixteen of its waves fit a CU's four
    SIMDs (512 registers each), and two of its workgroups' LDS images the CU's 160 KB: the register count is not what decides how many
    of its workgroups a CU holds (125 when this was written; the body before it had 116)."""
    r = _one(usage, "k_trsm_rows2<8>")
    assert r["vgprs"] is not None and r["vgprs"] <= 128, r
    assert 2 * trsm2_lds_bytes(8) == 148480 <= 160 * 1024


def trsm2_lds_bytes(nt):
    """launch_trsm2's dynamic LDS (mra_plan.hip): nt (nt - 1) / 2 strictly-lower tiles and nt inverted blocks of 2 KB, and the gather list"""
    return (nt * (nt - 1) // 2 + nt) * 2048 + nt * 16 * 4


def test_lds_formula_is_the_launchers():
    src = open(os.path.join(K.ROOT, "pymra_amd", "csrc", "mra_plan.hip")).read()
    assert "(size_t)(nt * (nt - 1) / 2 + nt) * 2048 + (size_t)nt * 16 * sizeof(int)" in src
    assert trsm2_lds_bytes(8) == 74240 and trsm2_lds_bytes(12) == 160512 <= 160 * 1024
