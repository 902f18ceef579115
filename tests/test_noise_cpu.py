"""The host side of per-observation noise variances (mra_plan_set_noise, mra_plan_set_noise_rows, mra_get_buffer(10)) without a
GPU: one child process with MRA_HOST_DRYRUN=1 (the plan lives in host memory, nothing is launched) walks through the state
machine and prints one line per check; every test below asserts its line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _cases as K

CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["MRA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRA_ROOT"], "tests"))
import _cases as K
from pymra_amd import plan as P
cs = K.load_case("g32")
topo, locs, y = cs["topo"], cs["locs"], np.asarray(cs["y_obs"], float).ravel().copy()
N, PP, R = int(topo.N), int(topo.P), float(cs["c"]["R"])
y[::7] = np.nan                                    # some unobserved rows
seen = np.isfinite(y)
src, perm = np.asarray(topo.src), np.asarray(topo.perm)
seen_p = seen[src] & (perm >= 0)                   # by padded row
assert 0 < seen.sum() < N and seen_p.sum() == seen.sum()
rng = np.random.RandomState(3)
r = rng.uniform(0.5 * R, 2.0 * R, size=N)

def code(call):
    try:
        call()
    except P.MraError as e:
        return e.code
    return 0

def expect(rv):
    out = np.where(seen_p, rv[src], 0.0)
    return out

pl = P.HipPlan(topo, 0)
pl.set_locs(locs)
assert code(lambda: pl.set_noise(r)) == -4 and code(lambda: pl.set_noise(None)) == -4
rp = np.ascontiguousarray(r[src])
assert pl.lib.mra_plan_set_noise(pl._h, P._ptr(rp)) == -4
assert "set_obs first" in pl.lib.mra_last_error(pl._h).decode()
print("STATE_OK")

pl.set_obs(y, R)
b = pl.buffer(10)
assert b.shape == (PP,) and np.all(b == R)
print("SCALAR_BUFFER_OK")

r_nan = r.copy(); r_nan[~seen] = np.nan; r_nan[np.nonzero(~seen)[0][0]] = -1.0; r_nan[np.nonzero(~seen)[0][1]] = np.inf
pl.set_noise(r_nan)                                # NaN, a negative value and inf at unobserved rows are ignored
assert np.array_equal(pl.buffer(10), expect(r))
print("UNOBSERVED_IGNORED_OK")

first = int(np.nonzero(seen)[0][5])
for bad in (-1e-3, np.nan, np.inf, -np.inf):
    rb = 2.0 * r; rb[first] = bad
    assert code(lambda: pl.set_noise(rb)) == -1, bad
    assert "negative or not finite" in pl.lib.mra_last_error(pl._h).decode()
    assert np.array_equal(pl.buffer(10), expect(r)), bad           # the plan is as it was
    rbp = np.ascontiguousarray(rb[src])
    assert pl.lib.mra_plan_set_noise(pl._h, P._ptr(rbp)) == -1
    assert np.array_equal(pl.buffer(10), expect(r)), bad
print("INVALID_OK")

r0 = r.copy(); r0[first] = 0.0                     # zero is a variance
pl.set_noise(r0)
assert np.array_equal(pl.buffer(10), expect(r0))
r2p = np.ascontiguousarray((3.0 * r)[src])         # the padded-order export: P values
assert pl.lib.mra_plan_set_noise(pl._h, P._ptr(r2p)) == 0
assert np.array_equal(pl.buffer(10), expect(3.0 * r))
print("ROUND_TRIP_OK")

pl.set_noise(None)
assert np.all(pl.buffer(10) == R)
pl.set_noise(None)                                 # twice: still the scalar
assert np.all(pl.buffer(10) == R)
print("NULL_RESTORES_SCALAR_OK")

pl.set_noise(r)
pl.set_obs(y, 2.5 * R)
assert np.all(pl.buffer(10) == 2.5 * R)
y2 = y.copy(); y2[1::7] = np.nan                   # another mask: the vector is read at ITS observed rows
pl.set_obs(y2, R)
pl.set_noise(r)
seen2 = np.isfinite(y2)[src] & (perm >= 0)
assert np.array_equal(pl.buffer(10), np.where(seen2, r[src], 0.0))
pl.set_obs(y, R)
assert np.all(pl.buffer(10) == R)
print("SET_OBS_DROPS_VECTOR_OK")

pl.set_obs(y, r)                                   # HipPlan.set_obs with a length-N array
assert np.array_equal(pl.buffer(10), expect(r))
pl.set_noise(None)
assert np.all(pl.buffer(10) == r[seen].mean())     # the scalar behind it: the mean over the observed rows
rb = r.copy(); rb[first] = -1.0
for call in (lambda: pl.set_obs(y2, rb), lambda: pl.set_obs(y, r[:-1]), lambda: pl.set_obs(y, np.outer(r, r)), lambda: pl.set_noise(r[:-1]),
             lambda: pl.set_noise(np.outer(r, r))):
    try:
        call()
        raise SystemExit("a bad noise argument must be refused")
    except ValueError:
        pass
assert np.all(pl.buffer(10) == r[seen].mean())
print("SET_OBS_VECTOR_OK")

# host-covariance plans keep their blocks: set_noise does not reset the kernel as set_obs does
pl.set_obs(y, R)
pl.upload_host_cov(cs["covfun"], locs, y.reshape(-1, 1))
pl.set_noise(r)
assert np.array_equal(pl.buffer(10), expect(r))
assert code(lambda: pl.set_cov_block(0, np.zeros((1, 1)))) == -1      # still a MRA_KERNEL_HOST plan: a shape error, not MRA_ERR_STATE
pl.close()
print("HOST_COV_OK")
'''

CHECKS = ["STATE_OK", "SCALAR_BUFFER_OK", "UNOBSERVED_IGNORED_OK", "INVALID_OK", "ROUND_TRIP_OK", "NULL_RESTORES_SCALAR_OK",
          "SET_OBS_DROPS_VECTOR_OK", "SET_OBS_VECTOR_OK", "HOST_COV_OK"]


@pytest.fixture(scope="module")
def child_output(built_library, tmp_path_factory):
    child = tmp_path_factory.mktemp("noise") / "child.py"
    child.write_text(CHILD)
    env = dict(os.environ, MRA_ROOT=K.ROOT, MRA_HOST_DRYRUN="1")
    res = subprocess.run([sys.executable, str(child)], env=env, capture_output=True, text=True, timeout=600)
    return res.stdout.split(), (res.stdout + res.stderr)[-3000:]


@pytest.mark.parametrize("check", CHECKS)
def test_noise_state_machine(child_output, check):
    done, log = child_output
    assert check in done, log


def test_exports_and_bindings():
    from pymra_amd import plan
    from pymra_amd.MRATree import MRATree
    assert "mra_plan_set_noise" in plan.EXPORTS and "mra_plan_set_noise_rows" in plan.EXPORTS
    assert callable(getattr(plan.HipPlan, "set_noise", None)) and callable(getattr(MRATree, "setNoise", None))


def test_mratree_refuses_what_is_not_a_diagonal():
    """The argument checks come before anything is built: an int is still a TypeError, a 2-D array (correlated noise) a ValueError
    that says only a diagonal is supported, a vector of the wrong length or with a negative variance a ValueError."""
    import pymra_amd
    import pymra_amd.MRATools as mt
    cs = K.load_case("kat2")
    N = len(cs["locs"])
    cov = lambda a, b: mt.ExpCovFun(a, b, l=1.0)

    def build(R):
        return pymra_amd.MRATree(cs["locs"], cs["c"]["r"], cov, cs["y_obs"], R, M=cs["c"]["M"], J=cs["c"]["J"])

    for R in (1, np.ones(N, dtype=np.int64), [0.1] * N, None):
        with pytest.raises(TypeError):
            build(R)
    with pytest.raises(ValueError, match="diagonal"):
        build(np.eye(N))
    with pytest.raises(ValueError):
        build(np.ones(N - 1))
    with pytest.raises(ValueError):
        build(-np.ones(N))
