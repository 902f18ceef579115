"""mra_plan_fit_laplace without a GPU: the dense twin of the iteration (tests/_laplace.py) on tree T16 - it
converges from the data-based start, its eight numbers give -2 log q(z) both ways, the Gaussian family is the Gaussian model, and
the floor on D is never what a test measures - and the binding's symbols, family names and argument handling."""
import numpy as np
import pytest

import _laplace as LP
import _noise as NZ
import test_gpu_likelihood_masks as MK


@pytest.mark.parametrize("family", [LP.POISSON, LP.BINOMIAL], ids=["poisson", "binomial"])
def test_newton_converges_from_the_data_based_start(family):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, res = LP.t16_fit(family)
    print("%s: passes %d, steps %s, min D %.3e" % (LP.NAMES[family], res["info"][5], ["%.1e" % s for s in res["steps"]], res["min_D"]))
    assert res["info"][7] == 1.0 and res["info"][5] <= 10
    assert res["min_D"] > 2.0 ** -20
    assert np.array_equal(np.isfinite(z), obs) and np.all(z[obs] >= 0)
    if family == LP.BINOMIAL:
        assert np.all(aux[obs] >= z[obs]) and aux.min() >= 1 and aux.max() <= 29
    else:
        E = np.exp(offset)
        assert 0.5 <= E.min() and E.max() <= 20.0
    # the mode: the gradient of log p(z | x) - x^T Sigma^-1 x / 2 vanishes, Sigma_oo g(x^) = x^
    g, _, _ = LP.terms(family, z[o], 1.0 if aux is None else aux[o], res["xhat"] + (0.0 if offset is None else offset[o]))
    assert np.abs(Sigma[np.ix_(o, o)] @ g - res["xhat"]).max() <= 1e-8


@pytest.mark.parametrize("family", [LP.GAUSSIAN, LP.POISSON, LP.BINOMIAL], ids=["gaussian", "poisson", "binomial"])
def test_the_eight_numbers_give_the_laplace_likelihood_both_ways(family):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, res = LP.t16_fit(family)
    direct = LP.direct_neg2logq(Sigma, res, family)
    print("%s: -2 log q %.10f, direct %.10f" % (LP.NAMES[family], res["lik"], direct))
    assert abs(res["lik"] - direct) <= 1e-10 * abs(direct)
    assert res["min_D"] > 2.0 ** -20


def test_gaussian_family_is_the_gaussian_model():
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, res = LP.t16_fit(LP.GAUSSIAN)
    ref = NZ.dense_reference(topo, locs, MK._spec(), (z - offset).reshape(-1, 1), aux, Sigma=Sigma)
    assert res["info"][5] == 2 and res["info"][6] == 0.0 and res["info"][7] == 1.0
    assert abs(res["info"][0] - ref["d"]) <= 1e-12 * abs(ref["d"]) and abs(res["info"][1] - ref["u"]) <= 1e-12 * abs(ref["u"])
    assert np.abs(res["mean"] - ref["mean"]).max() <= 1e-12 and np.abs(res["sd"] - ref["sd"]).max() <= 1e-12
    n = int(o.sum())
    # -2 log N(z - offset; 0, Sigma_oo + diag aux) = d + u + n log 2 pi
    want = ref["d"] + ref["u"] + n * np.log(2 * np.pi)
    assert abs(res["lik"] - want) <= 1e-12 * abs(want)


def test_binding_declares_the_call_and_the_family_names(built_library):
    from pymra_amd import plan
    lib = plan.load_library()
    assert "mra_plan_fit_laplace" in plan.EXPORTS and hasattr(lib, "mra_plan_fit_laplace")
    assert plan.LAPLACE_FAMILIES == {"gaussian": 0, "poisson": 1, "binomial": 2}
    assert (plan.MRA_FAMILY_GAUSSIAN, plan.MRA_FAMILY_POISSON, plan.MRA_FAMILY_BINOMIAL) == (LP.GAUSSIAN, LP.POISSON, LP.BINOMIAL)
    assert len(plan.LAPLACE_INFO) == 8
    import os
    import re
    import _cases as K
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    defs = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define\s+(MRA_FAMILY_\w+)\s+(\d+)", hdr))
    assert defs == {"MRA_FAMILY_" + k.upper(): v for k, v in plan.LAPLACE_FAMILIES.items()}
