"""The kernel instances of MRA_KERNEL_LOCAL (covariance mode 6: local ranges in the last coordinate column) without a GPU: that the
build has them, and what the compiler gave them.  Read from the remarks of the product build, by name, as
tests/test_kernel_sum_resources.py reads them.

Mode 6 needs an instance of every kernel that takes the covariance as a template parameter, for DIM = 2 (rows (x, lam)) and DIM = 3
(rows (x, y, lam)); a plan with d = 1 never has this mode.  All of them come from two translation units of their own
(mra_launch_loc.hip: the batched GEMMs; mra_launch_loc2.hip: the row and site kernels) under names of their own (k_*_loc), so that
no existing unit gains a kernel - tests/test_cv_trend_resources.py pins every kernel from before, tests/test_resource_usage_3d.py
closes the list of DIM = 3 instances under the existing names, tests/test_kernel_sum_resources.py holds the k_*_sum names to mode 5.
The new units instantiate nothing but mode 6, and every instance stays in registers: no scratch, no spilled VGPRs, no AGPRs.  The
fused prior cascades have no mode-6 instance; tests/test_gpu_local_range.py pins the level-by-level route such plans take."""
import os
import re
import sys

import pytest

import _cases as K

sys.path.insert(0, os.path.join(K.ROOT, "tools"))

EPI_COV = "2"
DIMS = ("2", "3")
ROW_AND_SITE = ("k_solve_rows", "k_cov_rows", "k_site_basis", "k_site_leaf", "k_site_mean", "k_cv_gram")
WITH_POST = ("k_site_gram", "k_site_leaf_gram")
GEMMS = ("k_gemm_nt", "k_gemm_nt_lds", "k_leaf_gemm")


@pytest.fixture(scope="module")
def usage(built_library):
    import resource_usage
    p = os.path.join(K.ROOT, "pymra_amd", "libmra_hip.resource_usage.txt")
    assert os.path.exists(p), "no resource-usage remarks next to the library"
    return resource_usage.parse(open(p).read())


def _instances(usage, kernel):
    """{template arguments as a tuple of strings: resources} of one kernel template."""
    out = {}
    for name, r in usage.items():
        m = re.match(r"(?:void )?%s<([^>]*)>\(" % re.escape(kernel), name)
        if m:
            out[tuple(a.strip() for a in m.group(1).split(","))] = r
    return out


def _in_registers(kernel, args, r):
    print(kernel, args, r)
    assert r["scratch"] == 0 and r["spills"] == 0 and r["agprs"] == 0, (kernel, args, r)


def test_the_eval_kernel_is_there(usage):
    hits = [r for n, r in usage.items() if n.startswith("k_eval_kernel_local(")]
    assert len(hits) == 1, hits
    _in_registers("k_eval_kernel_local", (), hits[0])


def test_the_gemm_instances_are_there_and_nothing_but_mode_6(usage):
    want = {"k_gemm_nt_loc": [(EPI_COV, d, "6") for d in DIMS], "k_gemm_nt_lds_loc": [(EPI_COV, d, "6") for d in DIMS]}
    got_leaf = _instances(usage, "k_leaf_gemm_loc")
    # the leaves' residual in its two shapes and the one-launch prior level (SOLVE = 1), whatever occupancy they were given
    shapes = sorted((a[0], a[1], a[2], a[3], a[4], a[5], a[7]) for a in got_leaf)
    assert shapes == sorted((EPI_COV, d, "6") + s for d in DIMS for s in (("1", "8", "512", "0"), ("2", "7", "256", "0"), ("2", "4", "256", "1"))), shapes
    for args, r in got_leaf.items():
        _in_registers("k_leaf_gemm_loc", args, r)
    for kernel, inst in want.items():
        got = _instances(usage, kernel)
        assert sorted(got) == sorted(inst), (kernel, sorted(got))
        for args, r in got.items():
            _in_registers(kernel, args, r)


def test_the_row_and_site_instances_are_there_and_nothing_but_mode_6(usage):
    for kernel in ROW_AND_SITE:
        got = _instances(usage, kernel + "_loc")
        assert sorted(got) == sorted((d, "6") for d in DIMS), (kernel, sorted(got))
        for args, r in got.items():
            _in_registers(kernel + "_loc", args, r)
    for kernel in WITH_POST:
        got = _instances(usage, kernel + "_loc")
        assert sorted(got) == sorted((d, "6", p) for d in DIMS for p in ("true", "false")), (kernel, sorted(got))
        for args, r in got.items():
            _in_registers(kernel + "_loc", args, r)
    got = _instances(usage, "k_site_inert_loc")                     # (no DIM: it reads no coordinates)
    assert sorted(got) == [("6", "false"), ("6", "true")], sorted(got)
    for args, r in got.items():
        _in_registers("k_site_inert_loc", args, r)


def test_no_mode_6_instance_under_an_existing_name(usage):
    """... nor under the names of MRA_KERNEL_SUM and of the 3-D quadrature, and every new name is in the build"""
    for suffix in ("", "_sum", "_nu3"):
        for kernel in GEMMS:
            assert not [a for a in _instances(usage, kernel + suffix) if a[0] == EPI_COV and a[2] == "6"], kernel + suffix
        for kernel in ROW_AND_SITE + WITH_POST:
            assert not [a for a in _instances(usage, kernel + suffix) if a[1] == "6"], kernel + suffix
        assert not [a for a in _instances(usage, "k_site_inert" + suffix) if a[0] == "6"]
    for kernel in ("k_prior_cascade", "k_knot_chain"):
        assert not [a for a in _instances(usage, kernel) if a[3] == "6"], kernel
    known = set(k + "_loc" for k in GEMMS + ROW_AND_SITE + WITH_POST + ("k_site_inert",))
    named = set(re.match(r"(?:void )?(\w+)", n).group(1) for n in usage if re.match(r"(?:void )?\w+_loc[<(]", n))
    assert known == named, (sorted(known - named), sorted(named - known))
