"""Register / scratch budget of the DIM = 3 kernels, read from the remarks of the product build as
tests/test_resource_usage.py reads them: every kernel templated on the dimension has its DIM = 3 instantiations, none of them spills
a VGPR, and none uses scratch - the Kanter taper (mode 3) excepted, whose ocml sin / cos keep a private table of 544 bytes on
the stack (512 in the two-row-tile leaf product, in 2-D and 3-D alike), which is no spill.  SGPRs parked in the lanes of a VGPR
("SGPRs Spill": no memory traffic) are printed, not bounded: the stage-all row cascades have up to 98 of them in 3-D and up to 95 in 1-D and 2-D.

The 2-D one-launch prior level and the CWT = 4 row cascade are allowed a few parked registers by tests/test_resource_usage.py; their
3-D counterparts are not: the one-launch prior level runs at two workgroups per CU instead of three, and the row cascade rebuilds
three lane-only values where it needs them instead of holding them across the level loop."""
import itertools
import os
import re
import sys

import pytest

import _cases as K

sys.path.insert(0, os.path.join(K.ROOT, "tools"))

MODES = (0, 1, 2, 3)
BOOLS = ("true", "false")
OCML_STACK = 544


def _expected():
    names = []
    for (cwt, nl), md, sa in itertools.product(((1, 8), (2, 8), (4, 4)), MODES, BOOLS):
        names.append("k_prior_cascade<%d, %d, 3, %d, %s>" % (cwt, nl, md, sa))
    for (cwt, nl), md in itertools.product(((1, 8), (2, 8), (4, 4)), MODES):
        names.append("k_knot_chain<%d, %d, 3, %d>" % (cwt, nl, md))
    for md in MODES:
        names.append("k_leaf_gemm<2, 3, %d, 1, 8, 512, %d, 0>" % (md, 2 if md == 3 else 4))      # the leaves' residual product
        names.append("k_leaf_gemm<2, 3, %d, 2, 7, 256, 2, 0>" % md)                                # its two-row-tile shape (dbg bit 32)
        names.append("k_leaf_gemm<2, 3, %d, 2, 4, 256, 2, 1>" % md)                                # one-launch prior level
        names.append("k_gemm_nt<2, 3, %d>" % md)
        names.append("k_gemm_nt_lds<2, 3, %d>" % md)
        names.append("k_solve_rows<3, %d>" % md)
        names.append("k_cov_rows<3, %d>" % md)
        for k in ("basis", "leaf", "mean"):
            names.append("k_site_%s<3, %d>" % (k, md))
        for k, b in itertools.product(("gram", "leaf_gram"), BOOLS):
            names.append("k_site_%s<3, %d, %s>" % (k, md, b))
    return names


@pytest.fixture(scope="module")
def usage(built_library):
    import resource_usage
    p = os.path.join(K.ROOT, "pymra_amd", "libmra_hip.resource_usage.txt")
    if not os.path.exists(p):
        pytest.skip("no resource-usage remarks next to the library (built outside __graft_entry__.build / make lib)")
    return resource_usage.parse(open(p).read())


def _kernel(usage, name):
    hits = {n: r for n, r in usage.items() if re.search(r"\b" + re.escape(name) + r"\(", n)}
    assert len(hits) == 1, "%s: %d instantiations in the remarks" % (name, len(hits))
    return next(iter(hits.values()))


def test_every_dim3_instantiation_exists_and_spills_no_vgpr(usage):
    names = _expected()
    assert len(names) == 24 + 12 + 4 * 14
    bad = []
    for name in names:
        r = _kernel(usage, name)
        kanter = re.search(r"<2, 3, 3[,>]|<\d, \d, 3, 3[,>]|<3, 3[,>]", name) is not None
        ok = (0, 512) if kanter and "2, 7, 256" in name else (0, OCML_STACK) if kanter else (0,)
        print("%-48s vgprs %3d scratch %3d spilled VGPRs %d (SGPRs parked in VGPR lanes: %d)" % (name, r["vgprs"], r["scratch"], r["spills"], r["sgpr_spills"]))
        if r["spills"] != 0 or r["scratch"] not in ok:
            bad.append("%s: %d B/lane of scratch, %d spilled VGPRs" % (name, r["scratch"], r["spills"]))
    assert not bad, "\n".join(bad)


def test_no_dim3_kernel_was_missed(usage):
    """every kernel of the build whose template arguments carry DIM = 3 is one of the expected ones: a new DIM-templated kernel
    has to be added to the list above (and so to the no-spill rule)"""
    want = set(_expected())
    dim3 = [n for n in usage if re.search(r"k_(prior_cascade|knot_chain)<\d, \d, 3,|k_(leaf_gemm|gemm_nt|gemm_nt_lds)<2, 3,|"
                                          r"k_(solve_rows|cov_rows|site_basis|site_leaf|site_mean|site_gram|site_leaf_gram)<3,", n)]
    stray = [n for n in dim3 if not any(re.search(r"\b" + re.escape(w) + r"\(", n) for w in want)]
    assert not stray, stray
    # the epilogues without a covariance have no dimension: a 3-D plan runs their DIM = 2 instances
    assert not [n for n in usage if re.search(r"k_(leaf_gemm|gemm_nt|gemm_nt_lds)<[013], 3,", n)]
