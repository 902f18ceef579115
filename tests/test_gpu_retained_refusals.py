"""What the six calls on the retained factors refuse before they look at their own arguments - mra_sample, mra_solve, mra_cov_apply,
mra_predict_sites, mra_sites_cov, mra_sample_sites - pinned by return code and by the exact bytes of mra_last_error, in the order the
refusals fire: unknown flags, set_locs / set_kernel missing, set_obs missing, MRA_KERNEL_HOST plan, sharded plan; then the call's own
first count argument.  The six share one preamble in the library (retained_check_plan); the strings below are literals on purpose, so
that the test says what a caller reads, whatever the library does to produce it.

One 32 x 32 tree (r = 16, M = 2: 1024 points, 16 leaves, gappy as test_gpu_cov.py's), one plan that walks through the states, and a
second plan on the same tree for the host-evaluated covariance, which a plan cannot leave again."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_cov as GC
import test_sites_cpu as SC

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -4
BAD_FLAG = 1 << 7            # no export defines it

# export: (accepted flag to combine with the unknown one, "MRA_KERNEL_HOST plans ...", "sharded plans ...", message of a count of -1)
_SITES = ("cannot predict at new sites (C(Q, s) is evaluated on the device)", "cannot predict at new sites", b"n_sites < 0")
EXPORTS = {
    "mra_sample": (1, "cannot sample (leaf C(S, S) is not available)", "cannot sample", b"n_samples < 0"),
    "mra_solve": (0, "cannot solve (C(S, o) is evaluated on the device)", "cannot solve", b"n_cols < 0"),
    "mra_cov_apply": (1, "cannot apply the covariance (C(S, S) is evaluated on the device)", "cannot apply the covariance", b"n_cols < 0"),
    "mra_predict_sites": (0,) + _SITES,
    "mra_sites_cov": (1,) + _SITES,
    "mra_sample_sites": (1,) + _SITES,
}


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return plan


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _callers(pl, sites, leaf):
    """name -> f(flags, n): the raw export with valid arguments, its first count argument replaced by n when n is given."""
    P, ns = pl.P, len(sites)
    col, out, sq = np.zeros((1, P)), np.empty((1, P)), np.empty((1, 1))
    m5, v5, c55 = np.empty((1, ns)), np.empty(ns), np.empty((ns, ns))
    lib, h = pl.lib, pl._h
    cnt = lambda n, default: default if n is None else n      # noqa: E731
    return {
        "mra_sample": lambda f, n=None: lib.mra_sample(h, f, cnt(n, 1), 3, 0, None, _ptr(out)),
        "mra_solve": lambda f, n=None: lib.mra_solve(h, f, cnt(n, 1), _ptr(col), _ptr(out), _ptr(sq)),
        "mra_cov_apply": lambda f, n=None: lib.mra_cov_apply(h, f, cnt(n, 1), _ptr(col), _ptr(out), _ptr(sq)),
        "mra_predict_sites": lambda f, n=None: lib.mra_predict_sites(h, f, cnt(n, ns), _ptr(sites), _ptr(leaf), 1, None, _ptr(m5), _ptr(v5)),
        "mra_sites_cov": lambda f, n=None: lib.mra_sites_cov(h, f, cnt(n, ns), _ptr(sites), _ptr(leaf), _ptr(c55)),
        "mra_sample_sites": lambda f, n=None: lib.mra_sample_sites(h, f, cnt(n, ns), _ptr(sites), _ptr(leaf), 1, 3, 0, None, _ptr(m5)),
    }


def _refused(pl, call, code, message, *args):
    assert call(*args) == code, (message, args)
    assert pl.lib.mra_last_error(pl._h) == message, args


def test_shared_refusals_of_the_six_exports_in_order(hip):
    import pymra_amd.MRATools as mt
    topo, locs, y_obs = GC._gappy_tree(n=32, r=16, M=2)
    spec = mt.KernelSpec(mt.KIND_MATERN32, 0.25, 1.2)
    assert len(locs) == 1024 and int(np.count_nonzero(topo.node_leaf)) == 16
    sites = np.ascontiguousarray(SC.off_row_sites(locs, 5, seed=1), dtype=np.float64)
    leaf = np.ascontiguousarray(SC.nearest_leaf(topo, locs, sites), dtype=np.int32)
    pl = hip.HipPlan(topo, 0)
    calls = _callers(pl, sites, leaf)

    def each(code, fmt, flags=0, n=None):
        for name, (_, host, sharded, count) in EXPORTS.items():
            want = count if fmt is None else fmt.format(who=name, host=host, sharded=sharded).encode()
            _refused(pl, calls[name], code, want, flags, n)

    def each_bad_flags():
        for name, (ok, _, _, _) in EXPORTS.items():
            for flags in (BAD_FLAG, BAD_FLAG | ok):
                _refused(pl, calls[name], INVALID, ("unknown %s flags" % name).encode(), flags)

    each(STATE, "{who} needs set_locs and set_kernel first")                     # a fresh plan
    each_bad_flags()                                                             # ... and the flags come before the state
    pl.set_locs(locs)
    each(STATE, "{who} needs set_locs and set_kernel first")
    pl.set_kernel(spec.kind, spec.l, spec.sig, spec.scale)
    each(STATE, "{who} needs set_obs first")
    each_bad_flags()                                                             # two violations at once: the flags are reported
    pl.set_obs(y_obs, GC.R_MASK)
    each_bad_flags()
    each(INVALID, None, n=-1)                                                    # the call's own arguments: after the plan's state
    each(INVALID, "unknown {who} flags", flags=BAD_FLAG, n=-1)
    pl.set_reduce_level(0)
    each(INVALID, "{who}: sharded plans {sharded}")
    each(INVALID, "{who}: sharded plans {sharded}", n=-1)                        # ... and before the call's own arguments
    each_bad_flags()
    pl.set_reduce_level(-1)

    host = hip.HipPlan(topo, 0)                                                  # the covariance evaluated by the caller
    host.set_locs(locs)
    host.set_obs(y_obs, GC.R_MASK)
    host.set_kernel_host()
    host_calls = _callers(host, sites, leaf)
    for sharded_too in (False, True):                                            # MRA_KERNEL_HOST is reported before the shards
        if sharded_too:
            host.set_reduce_level(0)
        for name, (_, why, _, _) in EXPORTS.items():
            _refused(host, host_calls[name], INVALID, ("%s: MRA_KERNEL_HOST plans %s" % (name, why)).encode(), 0)
            _refused(host, host_calls[name], INVALID, ("unknown %s flags" % name).encode(), BAD_FLAG)
    host.close()

    for name in EXPORTS:                                                         # still usable afterwards
        assert calls[name](0) == 0, (name, pl.lib.mra_last_error(pl._h))
    pl.close()
