"""The kernel instances of MRA_KERNEL_MATERN (covariance mode 4) without a GPU: that the build has them, and what the compiler gave
them.  Read from the remarks of the product build, by name, as tests/test_cv_trend_resources.py reads them (which also pins that
no kernel from before moved).

Mode 4 needs an instance of every kernel that takes the covariance as a template parameter, in every dimension - a dispatch
chain without one ends in an error (mra_bad_mode), never in another family's kernel.  The DIM = 3 instances come from a
translation unit of their own under names of their own (k_*_nu3, mra_launch_nu3.hip): the DIM = 3 instances of the closed-form
covariances are a closed list (tests/test_resource_usage_3d.py), and the rule of that list - no scratch, no spilled VGPRs - is
applied to the new ones here.  The kernels on the retained factors
(k_site_*, k_cv_gram, k_solve_rows, k_cov_rows) evaluate one value at a time and must stay in registers: no scratch, no spilled
VGPRs.  The fused prior cascades (k_prior_cascade, k_knot_chain) have NO mode-4 instance: at their register limit the quadrature
loop costs 544 bytes of scratch per lane, so path_of sends such plans down the level-by-level prior, which
tests/test_gpu_matern_nu.py pins from mra_get_route."""
import os
import re
import sys

import pytest

import _cases as K

sys.path.insert(0, os.path.join(K.ROOT, "tools"))

EPI_COV = 2


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


def test_the_eval_kernel_is_there(usage):
    hits = [r for n, r in usage.items() if n.startswith("k_eval_kernel_nu(")]
    assert len(hits) == 1 and hits[0]["scratch"] == 0 and hits[0]["spills"] == 0, hits


@pytest.mark.parametrize("dim", ["1", "2"])
def test_every_covariance_family_has_a_mode_4_instance(usage, dim):
    cov = str(EPI_COV)
    for kernel in ("k_gemm_nt", "k_gemm_nt_lds"):
        assert (cov, dim, "4") in _instances(usage, kernel), (kernel, dim)
    leaf = _instances(usage, "k_leaf_gemm")
    # the leaves' residual in both shapes, and the one-launch prior level (SOLVE = 1): two waves per SIMD, as the Kanter taper
    for args in ((cov, dim, "4", "1", "8", "512", "2", "0"), (cov, dim, "4", "2", "7", "256", "2", "0"), (cov, dim, "4", "2", "4", "256", "2", "1")):
        assert args in leaf, (args, sorted(a for a in leaf if a[2] == "4"))
        assert leaf[args]["scratch"] == 0 and leaf[args]["spills"] == 0, (args, leaf[args])
    for kernel in ("k_solve_rows", "k_cov_rows", "k_site_basis", "k_site_leaf", "k_site_mean", "k_cv_gram"):
        assert (dim, "4") in _instances(usage, kernel), (kernel, dim)
    for kernel in ("k_site_gram", "k_site_leaf_gram"):
        for post in ("true", "false"):
            assert (dim, "4", post) in _instances(usage, kernel), (kernel, dim, post)
    assert ("4", "true") in _instances(usage, "k_site_inert") and ("4", "false") in _instances(usage, "k_site_inert")


def test_retained_factor_instances_stay_in_registers(usage):
    seen = 0
    for kernel in ("k_solve_rows", "k_cov_rows", "k_site_basis", "k_site_leaf", "k_site_mean", "k_site_gram", "k_site_leaf_gram", "k_cv_gram", "k_site_inert"):
        for args, r in _instances(usage, kernel).items():
            mode = args[0] if kernel == "k_site_inert" else args[1]
            if mode != "4":
                continue
            seen += 1
            print(kernel, args, r)
            assert r["scratch"] == 0 and r["spills"] == 0, (kernel, args, r)
    assert seen == 2 * 6 + 2 * 4 + 2, seen


def test_the_3d_instances_have_names_of_their_own_and_stay_in_registers(usage):
    cov = str(EPI_COV)
    want = {"k_gemm_nt_nu3": [(cov, "3", "4")], "k_gemm_nt_lds_nu3": [(cov, "3", "4")],
            "k_leaf_gemm_nu3": [(cov, "3", "4", "1", "8", "512", "2", "0"), (cov, "3", "4", "2", "7", "256", "2", "0"), (cov, "3", "4", "2", "4", "256", "2", "1")],
            "k_site_gram_nu3": [("3", "4", "true"), ("3", "4", "false")], "k_site_leaf_gram_nu3": [("3", "4", "true"), ("3", "4", "false")],
            "k_site_inert_nu3": [("4", "true"), ("4", "false")]}
    for k in ("k_solve_rows", "k_cov_rows", "k_site_basis", "k_site_leaf", "k_site_mean", "k_cv_gram"):
        want[k + "_nu3"] = [("3", "4")]
    for kernel, inst in want.items():
        got = _instances(usage, kernel)
        assert sorted(got) == sorted(inst), (kernel, sorted(got))          # nothing but <3, 4> in that unit
        for args, r in got.items():
            print(kernel, args, r)
            assert r["scratch"] == 0 and r["spills"] == 0, (kernel, args, r)
    # and no mode-4 instance with DIM = 3 under the names of the closed list
    for kernel in ("k_gemm_nt", "k_gemm_nt_lds", "k_leaf_gemm"):
        assert not [a for a in _instances(usage, kernel) if a[0] == cov and a[1] == "3" and a[2] == "4"], kernel
    for kernel in ("k_solve_rows", "k_cov_rows", "k_site_basis", "k_site_leaf", "k_site_mean", "k_site_gram", "k_site_leaf_gram", "k_cv_gram"):
        assert not [a for a in _instances(usage, kernel) if a[0] == "3" and a[1] == "4"], kernel
    # every mode-4 instance of the GEMM families, whatever the dimension: no scratch
    for kernel in ("k_gemm_nt", "k_gemm_nt_lds", "k_leaf_gemm"):
        for args, r in _instances(usage, kernel).items():
            if args[0] == cov and args[2] == "4":
                assert r["scratch"] == 0 and r["spills"] == 0, (kernel, args, r)


def test_the_fused_cascades_have_no_mode_4_instance(usage):
    casc, chain = _instances(usage, "k_prior_cascade"), _instances(usage, "k_knot_chain")
    assert len(casc) >= 72 and len(chain) >= 36                 # (CWT, NLMAX, DIM, MODE[, STAGE_ALL])
    assert sorted(set(a[3] for a in casc)) == ["0", "1", "2", "3"], sorted(set(a[3] for a in casc))
    assert sorted(set(a[3] for a in chain)) == ["0", "1", "2", "3"], sorted(set(a[3] for a in chain))
