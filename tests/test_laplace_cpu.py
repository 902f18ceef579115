"""mra_plan_fit_laplace without a GPU: the dense twin of the iteration (tests/_laplace.py) on tree T16 - it
converges from the data-based start, its eight numbers give -2 log q(z) both ways, the Gaussian family is the Gaussian model, and
the floor on D is not what those fits measure - the references of the edge tests: the float64 terms against 50 digits, the twin's
end of a fit that leaves the doubles, recompute_info against the twin, the seeded edge inputs (the floor on D, saturated
probabilities) - and the binding's symbols, family names and argument handling."""
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


# ---- the references of the edge tests (tests/test_gpu_laplace.py, tests/test_gpu_fullsize.py) --------------------------------------------
N_T16 = 1473                                                          # observed rows of T16's mask: the size of the laplace_term grid


@pytest.mark.parametrize("family", [LP.GAUSSIAN, LP.POISSON, LP.BINOMIAL], ids=["gaussian", "poisson", "binomial"])
def test_float64_terms_against_50_digits(family):
    """``terms`` (float64, what the twin and recompute_info use) against ``terms_mp`` on the grid of the GPU's laplace_term tests.
    Bars, in the units of ``term_errors``: an exp or log1p is good to 1 ulp and the four operations to 1/2, so g, D and t of the
    Poisson and Gaussian families carry a few eps: 8.  The binomial p = exp(-L), L = logaddexp(0, -eta) <= 40 in the band (beyond it
    L = |eta| exactly): rounding L costs eps L / 2 <= 20 eps on p, as much on q, and D = aux p q and t = x + g / D inherit both: 64."""
    knots = LP.t16_upper_knots()
    assert 20 <= len(knots) <= 80                                      # 80 knots above the leaves, 36 % of the rows observed
    e = LP.term_errors(family, N_T16, knots)
    print("%s: float64 terms vs 50 digits, in eps: t %.2f, r %.2f, g %.2f, D %.2f, log p %.2f"
          % (LP.NAMES[family], e["e_t"] / LP.EPS, e["e_r"] / LP.EPS, e["e_g"] / LP.EPS, e["e_D"] / LP.EPS, e["e_lp"] / LP.EPS))
    x = e["x"]
    assert len(x) == N_T16 and np.sum(x == 0.0) == 2 and np.sum(np.abs(x) == 2.0 ** -60) == 2 and np.sum(np.abs(x) == 27.7) == 2
    assert (np.abs(x).max() == 700.0) == (family != LP.GAUSSIAN)
    if family == LP.POISSON:
        assert x[list(knots)].max() <= LP.KNOT_ETA_MAX and np.array_equal(np.sort(x), np.sort(LP.term_cases(family, N_T16)[2]))
    floored = np.array([float(r) for r in e["r"]]) == 2.0 ** 40
    assert floored.sum() >= 100 and (~floored).sum() >= 100
    bar = (64 if family == LP.BINOMIAL else 8) * LP.EPS
    assert max(e["e_t"], e["e_r"], e["e_g"], e["e_D"], e["e_lp"]) <= bar


def test_stable_binomial_terms_in_the_tails():
    """p and 1 - p of the float64 terms keep their relative accuracy where 1 / (1 + e^-eta) and 1 - p lose it"""
    eta = np.array([-700.0, -40.0, 40.0, 700.0])
    g, D, _ = LP.terms_eta(LP.BINOMIAL, np.array([0.0, 0.0, 1.0, 1.0]), 1.0, eta)
    assert np.all(D == 2.0 ** -40) and g[0] == -np.exp(-700.0) and g[1] == -np.exp(-40.0)
    g, D, _ = LP.terms_eta(LP.BINOMIAL, 0.0, 1e18, np.array([-40.0, 40.0]))
    want = 1e18 * np.exp(-40.0)
    assert np.all(np.abs(D - want) <= 8 * LP.EPS * want)


def test_twin_ends_a_fit_that_leaves_the_doubles():
    """big_counts from x0 = 0: pass 1 is finite and overshoots into the thousands, the linearisation of pass 2 has e^eta = inf and
    t = NaN; the twin ends there, not converged.  From the data-based start the same data converge."""
    res = LP.edge_fit("big_counts", True, 10)
    print("big_counts from 0: steps %s" % res["steps"])
    assert res["info"][5] == 2 and res["info"][7] == 0.0 and np.isnan(res["info"][6])
    assert np.isfinite(res["steps"][0]) and res["steps"][0] > 710.0                  # e^710 overflows
    assert np.all(np.isnan(res["mean"])) and np.all(np.isnan(res["sd"])) and np.isnan(res["lik"])
    o = res["o"]
    assert np.isnan(res["t"][o]).any() and np.all(np.isfinite(res["x_keep"][o]))
    ok = LP.edge_fit("big_counts")
    print("big_counts from the data: passes %d, steps %s" % (ok["info"][5], ["%.1e" % s for s in ok["steps"]]))
    assert ok["info"][7] == 1.0 and ok["info"][5] <= 6 and np.all(np.isfinite(ok["mean"]))


@pytest.mark.parametrize("family", [LP.GAUSSIAN, LP.POISSON, LP.BINOMIAL], ids=["gaussian", "poisson", "binomial"])
def test_recompute_info_is_the_twins(family):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    z, aux, offset, res = LP.t16_fit(family)
    xh = np.zeros(len(o))
    xh[o] = res["xhat"]                                                # (the twin's mean at the observed rows is another product: other roundings)
    assert np.abs(xh[o] - res["mean"][o]).max() <= 1e-12
    rc = LP.recompute_info(family, z, aux, offset, res["x_keep"], xh, res["t"], res["r"], o)
    for k, key in ((2, "info2"), (3, "info3"), (4, "info4")):
        assert abs(rc[key] - res["info"][k]) <= 1e-13 * abs(res["info"][k]), (key, rc[key], res["info"][k])
        assert rc["S"][k - 2] >= abs(rc[key])
    assert rc["step"] == res["info"][6] and rc["max_xhat"] == np.abs(res["xhat"]).max()


@pytest.mark.parametrize("name", ["tiny_exposure", "saturated", "gauss_floor"])
def test_edge_inputs_converge_in_the_twin(name):
    topo, locs, obs, y, counts, Sigma, o = LP.t16()
    family, z, aux, offset = LP.edge_inputs(name)
    res = LP.edge_fit(name)
    floored = int((res["r"][o] == 2.0 ** 40).sum())
    direct = LP.direct_neg2logq(Sigma, res, family)
    print("%s: passes %d, steps %s, min D %.3e, %d rows at the floor, max |x^| %.2f, lik %.12f direct %.12f (rel %.1e)"
          % (name, res["info"][5], ["%.1e" % s for s in res["steps"]], res["min_D"], floored, np.abs(res["xhat"]).max(), res["lik"], direct,
             abs(res["lik"] - direct) / abs(direct)))
    assert np.array_equal(np.isfinite(z), obs)
    assert res["info"][7] == 1.0 and res["info"][5] <= 50
    if name == "saturated":
        assert floored == 0 and res["min_D"] < 1e-2 and np.abs(res["xhat"]).max() > 5.0
        sat = o & ((z == 0) | (z == aux))
        assert sat.sum() >= 500
    else:
        assert floored >= 100 and (res["r"][o] < 10.0).sum() >= 100          # r = 2^40 beside r of order 1
        assert res["min_D"] == 2.0 ** -40
    if name == "gauss_floor":
        assert res["info"][5] == 2 and res["info"][6] == 0.0
    assert abs(res["lik"] - direct) <= 1e-12 * abs(direct)


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
