"""The leaves' row solve (k_trsm_rows2) against the bits of the build that had its row-tile body inline (GPU only).

trsm2_row_tile runs gathered and streamed tiles as separate instances, issues a load for every gather-list entry and masks the
padding afterwards, leaves early for a leaf without observations, reads the variance in front of the row's loads and nests its solve
steps - none of which may change what a row computes.  tests/golden/trsm_rows2.json holds, for every case of
tests/_trsm_rows2_cases.py (shapes, masks and options are described there), the likelihood terms, SHA-256 of mean, var and four
leaves' panels [Lc ; Ut ; Tt] after each of six passes, and of mra_cv's outputs, as commit e7339b1's build computed them
(tests/golden/make_trsm_rows2.py).  Every comparison is bit for bit."""
import json
import os

import pytest

import _cases as K
import _trsm_rows2_cases as TC

pytestmark = pytest.mark.gpu

PASSES = ("predict", "predict, kept", "likelihood only", "predict, noise vector", "predict, new mask", "likelihood only, new mask")


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(K.ROOT, "tests", "golden", "trsm_rows2.json")))


@pytest.mark.parametrize("key,opts", TC.CASES, ids=[TC.case_id(k, o) for k, o in TC.CASES])
def test_passes_keep_the_bits(hip, golden, key, opts):
    want = golden[TC.case_id(key, opts)]
    passes, cv = TC.run_script(hip, key, opts)
    r = passes[0]["route"]
    assert r["path"] == "Fused" and r["n_trsm_small"] == r["n_leaves"] >= 27, r
    if TC.IN_CASCADE[0] in opts:
        assert not r["solve_fused"], r              # the row solve has the full list: gathered Ut tiles, then streamed Tt tiles
    if key == "A":                                  # eligible for the kept residual (read through src unless option 25 is off)
        assert r["chol"] in ("TilesOne", "TilesSplit") and r["leaf_resident"] and not r["scatter_ut"], r
    got = TC.digest(passes, cv)
    for k, (g, w) in enumerate(zip(got["passes"], want["passes"])):
        tag = "%s, pass %d (%s)" % (TC.case_id(key, opts), k, PASSES[k])
        assert g["lik"] == w["lik"], "%s: likelihood terms %r, golden %r" % (tag, g["lik"], w["lik"])
        if "mean" in w:
            assert g["mean_sample"] == w["mean_sample"] and g["var_sample"] == w["var_sample"], "%s: sampled mean / var %r %r, golden %r %r" % (
                tag, g["mean_sample"], g["var_sample"], w["mean_sample"], w["var_sample"])
            assert g["mean"] == w["mean"] and g["var"] == w["var"], "%s: mean or var differs from the golden bits away from the 16 samples" % tag
        assert g["panels"] == w["panels"], "%s: panels of the watched leaves %r" % (tag, [a == b for a, b in zip(g["panels"], w["panels"])])
    assert len(got["passes"]) == len(want["passes"]) == len(PASSES)
    assert got["cv"] == want["cv"], "%s: mra_cv outputs (mean, var, lpd, group lpd) %r" % (TC.case_id(key, opts), [a == b for a, b in zip(got["cv"], want["cv"])])
