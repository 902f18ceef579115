"""The kernels of mra_cv_trend without a GPU: what the compiler gave them, and that nothing else moved.

k_cv_trend and k_cv_downdate run one wave per workgroup under __launch_bounds__(64, 4): four waves per SIMD need at most 128 registers
each, and the tile's h and the accumulators are worth holding only in registers - no scratch, no spilled registers, no AGPRs.  Read
from the remarks of the product build, as tests/test_parent_pair_resources.py reads them; the kernels are looked up by name, so that a
build that lost them fails too.

tests/golden/resource_usage_before_cv_trend.json is tools/resource_usage.parse() of the build before these kernels were added: every
kernel in it is still there with the same registers, scratch, spills, occupancy and LDS - the new entry point added kernels and changed
none (mra_cv and every pass keep their object code).  A change that alters one of those kernels on purpose writes the file again from
its own parent's build."""
import json
import os
import sys

import pytest

import _cases as K

sys.path.insert(0, os.path.join(K.ROOT, "tools"))

NEW = ("k_cv_trend(", "k_cv_downdate(", "k_cv_trend_part(", "k_cv_trend_sum(")


@pytest.fixture(scope="module")
def usage(built_library):
    import resource_usage
    p = os.path.join(K.ROOT, "pymra_amd", "libmra_hip.resource_usage.txt")
    assert os.path.exists(p), "no resource-usage remarks next to the library"
    return resource_usage.parse(open(p).read())


@pytest.mark.parametrize("kernel", ["k_cv_trend(", "k_cv_downdate("])
def test_the_new_kernels_fit_four_waves_per_simd_in_registers(usage, kernel):
    hits = {n: r for n, r in usage.items() if n.startswith(kernel)}
    assert len(hits) == 1, sorted(n for n in usage if "k_cv_" in n)
    (name, r), = hits.items()
    print(name, r)
    assert r["scratch"] == 0 and r["spills"] == 0 and r["sgpr_spills"] == 0, r
    assert not r["agprs"], r
    assert r["vgprs"] is not None and r["vgprs"] <= 128, r
    assert r["occupancy"] is not None and r["occupancy"] >= 4, r
    assert r["lds"] == 0, r                     # L_A^-1 comes out of L2: 32 KB of LDS per wave would leave one wave per SIMD


def test_the_reduction_kernels_are_there(usage):
    for kernel in ("k_cv_trend_part(", "k_cv_trend_sum("):
        hits = [r for n, r in usage.items() if n.startswith(kernel)]
        assert len(hits) == 1 and hits[0]["scratch"] == 0 and hits[0]["spills"] == 0, (kernel, hits)


def test_every_kernel_from_before_is_unchanged(usage):
    before = json.load(open(os.path.join(K.ROOT, "tests", "golden", "resource_usage_before_cv_trend.json")))
    assert len(before) > 400 and not any(n.startswith(NEW) for n in before)
    missing = sorted(n for n in before if n not in usage)
    assert not missing, missing[:5]
    changed = {n: (before[n], usage[n]) for n in before if usage[n] != before[n]}
    assert not changed, list(changed.items())[:5]
