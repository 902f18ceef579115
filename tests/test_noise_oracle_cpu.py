"""The two references of tests/_noise.py agree with each other (CPU): the rescaled level-wise oracle against dense algebra on the MRA
prior covariance with Sigma[o, o] + diag(r_o), on the 2-D tree T16 of tests/_route_cells.py and on the 1-D golden tree t201, whose
partition drops rows.  This pins the reference that tests/test_gpu_noise.py holds the device to; it passes with or without the
feature.

Bars: likelihood 1e-12 relative, mean 1e-10 absolute, sd 1e-10 relative - 50 to 300 times what T16 shows (3e-15, 2e-12, 2e-12)."""
import numpy as np
import pytest

import _cases as K
import _noise as NZ

BARS = (1e-12, 1e-10, 1e-10)


def _t16():
    import _route_cells as RC
    import test_gpu_likelihood_masks as MK
    topo, locs = MK._tree(*RC.TREES["T16"])
    y = MK._y(RC.make_obs(topo, locs, RC.CLOUD))
    return topo, locs, MK._spec(), y, MK.R


def _t201():
    cs = K.load_case("t201")
    return cs["topo"], cs["locs"], cs["spec"], cs["y_obs"], float(cs["c"]["R"])


@pytest.mark.parametrize("make", [_t16, _t201], ids=["T16", "t201"])
def test_rescaled_oracle_against_dense_algebra(make):
    topo, locs, spec, y, R = make()
    r = NZ.noise_of(locs, R)
    assert r.min() < 0.5 * R and r.max() > 2.0 * R
    if make is _t201:
        assert not NZ.reported(topo).all()                      # rows that the 1-D partition drops
    ref = NZ.dense_reference(topo, locs, spec, y, r)
    got = NZ.scaled_oracle(topo, locs, spec, y, R)
    rep = NZ.reported(topo)
    e_l = abs(got["lik"] - ref["lik"]) / abs(ref["lik"])
    e_d = abs(got["d"] - ref["d"]) / abs(ref["d"])
    e_m = np.abs(got["mean"] - ref["mean"])[rep].max()
    e_s = (np.abs(got["sd"] - ref["sd"])[rep] / ref["sd"][rep]).max()
    print("lik %.2e d %.2e mean %.2e sd %.2e" % (e_l, e_d, e_m, e_s))
    assert e_l <= BARS[0] and e_d <= BARS[0]
    assert e_m <= BARS[1]
    assert e_s <= BARS[2]
    # the vector is no small perturbation of the scalar: the tests that use these references discriminate
    flat = NZ.dense_reference(topo, locs, spec, y, R, Sigma=ref["Sigma"])
    assert np.abs(flat["mean"] - ref["mean"])[rep].max() > 1e-3
    assert np.abs(flat["sd"] - ref["sd"])[rep].max() > 1e-4
