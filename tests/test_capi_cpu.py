"""The C-ABI library on a machine WITHOUT a GPU: it builds, loads, exports every symbol the header
declares, and refuses to create a plan (no CPU fallback)."""
import os
import re

import numpy as np
import pytest

import _cases as K


def _header_functions():
    txt = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mra_[a-z_0-9]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol(built_library):
    from pymra_amd import plan
    declared = _header_functions()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(built_library, name), "libmra_hip.so lacks %s" % name
    assert sorted(plan.EXPORTS) == declared, "pymra_amd.plan.EXPORTS and include/mra_hip.h disagree"
    assert b"gfx950" in built_library.mra_version()


def test_product_path_never_imports_the_oracle():
    """pymra_amd must not reach into oracle/ (only tests, smoke() and bench's cpu_baseline may)."""
    pkg = os.path.join(K.ROOT, "pymra_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "oracle" not in re.sub(r'""".*?"""', "", src, flags=re.S), fn


def test_no_gpu_means_loud_failure(built_library):
    from pymra_amd import plan
    if plan.device_count() > 0:
        pytest.skip("a GPU is present")
    cs = K.load_case("kat2")
    with pytest.raises(plan.MraError) as ei:
        plan.HipPlan(cs["topo"], 0)
    assert ei.value.code == -2 and "no CPU fallback" in str(ei.value)
    import pymra_amd
    with pytest.raises(plan.MraError):
        pymra_amd.MRATree(cs["locs"], cs["c"]["r"], lambda a, b: pymra_amd.MRATools.ExpCovFun(a, b, l=1.0),
                          cs["y_obs"], cs["c"]["R"], M=cs["c"]["M"], J=cs["c"]["J"])


def test_cov_probe_recognises_device_kernels():
    import pymra_amd.MRATools as mt
    from pymra_amd.MRATree import probe_cov
    s = probe_cov(lambda a, b: 2.5 * mt.Matern32(a, b, l=0.3, sig=1.5), 2)
    assert (s.kind, s.l, s.sig, s.scale) == (mt.KIND_MATERN32, 0.3, 1.5, 2.5)
    assert probe_cov(lambda a, b: mt.ExpCovFun(a, b, l=0.7), 1).kind == mt.KIND_EXP
    assert probe_cov(lambda a, b: np.exp(-np.abs(a - b.T)), 1) is None          # opaque callable
    assert probe_cov(np.eye(3), 1) is None                                       # dense matrix
    # array inputs still give the reference's np.matrix values
    x = mt.genLocations(5)
    v = mt.Matern32(x, x, l=0.3, sig=2.0)
    assert isinstance(v, np.matrix) and v.shape == (5, 5) and abs(v[0, 0] - 2.0) < 1e-15
    assert np.allclose(np.asarray(s.evaluate(x, x)), 2.5 * np.asarray(mt.Matern32(x, x, l=0.3, sig=1.5)))


def test_option_numbers_agree_with_the_header():
    """pymra_amd/plan.py repeats the MRA_OPT_* numbers of include/mra_hip.h (ctypes has no header): they must not drift."""
    import re
    from pymra_amd import plan as P
    hdr = open(os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    defs = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define\s+(MRA_OPT_\w+)\s+(\d+)", hdr))
    assert len(defs) >= 12
    for name, val in defs.items():
        assert getattr(P, name) == val, name


def test_every_plan_raises_its_own_lds_limits(built_library, tmp_path):
    """The 160 KB dynamic-LDS attribute is per kernel AND per device: it is recorded per plan (a plan lives on one device),
    not behind a process-wide flag - two plans on different device ordinals in one process both take the path.  Host dry
    run (MRA_HOST_DRYRUN=1: plans are built in host memory, nothing is launched), so this runs without a GPU."""
    import subprocess
    import sys
    child = tmp_path / "child.py"
    child.write_text(r'''
import os, sys
sys.path.insert(0, os.environ["MRA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRA_ROOT"], "tests"))
import _cases as K
import pymra_amd.MRATools as mt
from pymra_amd import plan as P
cs = K.load_case("g64")
counts = []
for dev in (0, 1, 0):
    pl = P.HipPlan(cs["topo"], dev)
    pl.set_locs(cs["locs"]); pl.set_obs(cs["y_obs"], cs["c"]["R"]); pl.set_kernel(mt.KIND_EXP, 0.3, 1.0, 1.0)
    counts.append(pl.prepare())
    assert pl.prepare() == counts[-1]            # idempotent
    try:
        pl.set_option(99, 2)                     # what-if bits that change results are not in the product library
        raise SystemExit("option 99 bit 2 must be refused")
    except P.MraError as e:
        assert e.code == -1
    pl.set_option(99, 8); assert pl.get_option(99) == 8
    pl.set_option(P.MRA_OPT_FUSED, 0); assert pl.get_option(P.MRA_OPT_FUSED) == 0
    for opt, val in ((P.MRA_OPT_LEAF_SOLVE_SPLIT, 1), (P.MRA_OPT_CHOL_TILES, 2), (P.MRA_OPT_SEG_GEMM_LDS, 0), (P.MRA_OPT_UT_GATHER, 0)):
        pl.set_option(opt, val); assert pl.get_option(opt) == val
    try:
        pl.set_option(57, 1)
        raise SystemExit("an unknown option must be refused")
    except P.MraError as e:
        assert e.code == -1
    pl.close()
print("LDS_ATTR_OK", counts)
assert counts[0] >= 10 and counts[0] == counts[1] == counts[2]
''')
    env = dict(os.environ, MRA_ROOT=K.ROOT, MRA_HOST_DRYRUN="1")
    res = subprocess.run([sys.executable, str(child)], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "LDS_ATTR_OK" in res.stdout, (res.stdout + res.stderr)[-2000:]


def test_cascade_group_option_round_trip(built_library, tmp_path):
    """MRA_OPT_CASCADE_GROUP reports the plan's own decision (the cost model: off for a 64 x 64 tree, on for 512^2, r=32, M=5
    at 256 CUs) and forcing it either way rebuilds the leaf workgroup lists.  Host dry run, no GPU."""
    import subprocess
    import sys
    child = tmp_path / "child.py"
    child.write_text(r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["MRA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRA_ROOT"], "tests"))
import _cases as K
import pymra_amd.MRATools as mt
from pymra_amd import plan as P
from pymra_amd.topology import build_topology
cs = K.load_case("g64")
np.random.seed(2)
locs = mt.genLocations2d(Nx=512, Ny=512)
big = build_topology(locs, 32, 5, 4)
y = np.where(np.random.uniform(size=(512 * 512, 1)) < 0.4, 1.0, np.nan)
for topo, lc, yo, want in ((cs["topo"], cs["locs"], cs["y_obs"], 0), (big, locs, y, 1)):
    pl = P.HipPlan(topo, 0)
    pl.set_locs(lc); pl.set_obs(yo, 1e-2); pl.set_kernel(mt.KIND_EXP, 0.3, 1.0, 1.0)
    assert pl.get_option(P.MRA_OPT_CASCADE_GROUP) == want, (topo.N, pl.get_option(P.MRA_OPT_CASCADE_GROUP))
    for v in (1, 0, 1, want):
        pl.set_option(P.MRA_OPT_CASCADE_GROUP, v); assert pl.get_option(P.MRA_OPT_CASCADE_GROUP) == v
    pl.close()
print("CASCADE_GROUP_OK")
""")
    env = dict(os.environ, MRA_ROOT=K.ROOT, MRA_HOST_DRYRUN="1")
    res = subprocess.run([sys.executable, str(child)], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "CASCADE_GROUP_OK" in res.stdout, (res.stdout + res.stderr)[-2000:]


# exports that only read plain fields and stay outside the exception boundary (the list at guarded() in mra_plan.hip)
_UNGUARDED = {"mra_version", "mra_last_error", "mra_device_count", "mra_kernel_family_count", "mra_get_timers", "mra_plan_info",
              "mra_get_kernel_stats", "mra_get_kernel_work", "mra_tree_sizes"}


def test_every_export_goes_through_the_exception_boundary():
    """include/mra_hip.h promises that no C++ exception crosses the C ABI: every export of mra_plan.hip but the plain field
    readers returns guarded(...), the one boundary helper above the extern "C" block, and no catch clause sits in the block."""
    src = open(os.path.join(K.ROOT, "pymra_amd", "csrc", "mra_plan.hip")).read()
    begin, end = src.index('extern "C" {'), src.index('}  // extern "C"')
    assert src.index("static int guarded(") < begin
    block = re.sub(r"//[^\n]*", "", src[begin:end])
    assert not re.search(r"\bcatch\b", block), "catch clause inside the extern \"C\" block"
    heads = list(re.finditer(r"^(?:int|const char\*) (mra_\w+)\([^{]*\{", block, flags=re.M))
    assert sorted(m.group(1) for m in heads) == _header_functions()
    for m, nxt in zip(heads, heads[1:] + [None]):
        body = block[m.end():nxt.start() if nxt else len(block)].lstrip()
        if m.group(1) not in _UNGUARDED:
            assert body.startswith("return guarded("), "%s does not go through guarded()" % m.group(1)


def test_null_arguments_report_their_own_error(built_library, tmp_path):
    """A NULL argument returns MRA_ERR_INVALID and mra_last_error names the function that refused it (the plan's message, or the
    thread's when the plan itself is NULL), not whatever an earlier failure left there.  Host dry run, no GPU."""
    import subprocess
    import sys
    child = tmp_path / "child.py"
    child.write_text(r'''
import os, sys
import ctypes as C
import numpy as np
sys.path.insert(0, os.environ["MRA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRA_ROOT"], "tests"))
import _cases as K
import pymra_amd.MRATools as mt
from pymra_amd import plan as P
cs = K.load_case("g64")
pl = P.HipPlan(cs["topo"], 0)
pl.set_locs(cs["locs"]); pl.set_obs(cs["y_obs"], cs["c"]["R"]); pl.set_kernel(mt.KIND_EXP, 0.3, 1.0, 1.0)
lib, h, N = pl.lib, pl._h, int(cs["topo"].N)
x = np.zeros(4 * int(cs["topo"].P)); buf = P._ptr(x)
def earlier_error():
    try:
        pl.set_kernel(mt.KIND_EXP, -1.0)
        raise SystemExit("a negative length scale must be refused")
    except P.MraError as e:
        assert "length scale" in str(e) and "length scale" in lib.mra_last_error(None).decode()
def refused(name, call, handle):
    earlier_error()
    assert call() == -1, name
    msg = lib.mra_last_error(handle).decode()
    assert msg.startswith(name + ":"), (name, msg)
# plan-taking exports: (name, call with plan p and its other pointer arguments NULL, whether it has one)
plan_calls = [
    ("mra_plan_set_locs", lambda p: lib.mra_plan_set_locs(p, None), True),
    ("mra_plan_set_obs", lambda p: lib.mra_plan_set_obs(p, None, 1.0), True),
    ("mra_plan_set_locs_rows", lambda p: lib.mra_plan_set_locs_rows(p, buf, None), True),
    ("mra_plan_set_obs_rows", lambda p: lib.mra_plan_set_obs_rows(p, buf, None, None, 1.0), True),
    ("mra_get_predict_rows", lambda p: lib.mra_get_predict_rows(p, None, None, N, buf, buf), True),
    ("mra_get_predict_rows_sd", lambda p: lib.mra_get_predict_rows_sd(p, None, None, N, buf, buf, None), True),
    ("mra_plan_set_kernel", lambda p: lib.mra_plan_set_kernel(p, 0, None, 3), True),
    ("mra_plan_set_cov_block", lambda p: lib.mra_plan_set_cov_block(p, 0, None, 0, 0, None), True),
    ("mra_sample_slots", lambda p: lib.mra_sample_slots(p, None), True),
    ("mra_get_likelihood", lambda p: lib.mra_get_likelihood(p, None, None), True),
    ("mra_get_predict", lambda p: lib.mra_get_predict(p, None, None), True),
    ("mra_get_buffer", lambda p: lib.mra_get_buffer(p, 0, None, 0, None), True),
    ("mra_get_node_block", lambda p: lib.mra_get_node_block(p, 0, 0, None, 0, None, None), True),
    ("mra_plan_get_option", lambda p: lib.mra_plan_get_option(p, 1, None), True),
    ("mra_reduce_size", lambda p: lib.mra_reduce_size(p, None), True),
    ("mra_reduce_export", lambda p: lib.mra_reduce_export(p, None), True),
    ("mra_reduce_import", lambda p: lib.mra_reduce_import(p, None), True),
    ("mra_comm_init", lambda p: lib.mra_comm_init(p, None, 1, 0), True),
    ("mra_run", lambda p: lib.mra_run(p, 1), False),
    ("mra_run_resume", lambda p: lib.mra_run_resume(p), False),
    ("mra_sample", lambda p: lib.mra_sample(p, 0, 1, 0, 0, None, None), False),
    ("mra_plan_set_option", lambda p: lib.mra_plan_set_option(p, 1, 0), False),
    ("mra_plan_prepare", lambda p: lib.mra_plan_prepare(p, None), False),
    ("mra_plan_set_reduce_level", lambda p: lib.mra_plan_set_reduce_level(p, 0), False),
]
for name, call, has_ptr in plan_calls:
    if has_ptr:
        refused(name, lambda: call(h), h)
    refused(name, lambda: call(None), None)
# exports without a plan
i32 = C.c_int32(0)
for name, call in (
        ("mra_plan_create", lambda: lib.mra_plan_create(None, None, 0)),
        ("mra_eval_kernel", lambda: lib.mra_eval_kernel(0, None, 3, None, 1, None)),
        ("mra_comm_unique_id", lambda: lib.mra_comm_unique_id(None, 128)),
        ("mra_tree_replay_2d", lambda: lib.mra_tree_replay_2d(None, 1, 16, 2, None, C.byref(i32), None)),
        ("mra_tree_replay_2d_into", lambda: lib.mra_tree_replay_2d_into(None, 1, 16, 2, None, C.byref(i32), 100, None, None, None,
                                                                         None, None)),
        ("mra_plan_create_replay_2d", lambda: lib.mra_plan_create_replay_2d(None, 1, 16, 2, None, C.byref(i32), None, 1.0, 0, 100,
                                                                             None, None, None, None, None, None)),
        ("mra_tree_export", lambda: lib.mra_tree_export(*[None] * 16))):
    refused(name, call, None)
assert pl.get_option(P.MRA_OPT_FUSED) in (0, 1)              # the plan is still whole
pl.close()
print("NULL_ARGS_OK", len(plan_calls))
''')
    env = dict(os.environ, MRA_ROOT=K.ROOT, MRA_HOST_DRYRUN="1")
    res = subprocess.run([sys.executable, str(child)], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "NULL_ARGS_OK" in res.stdout, (res.stdout + res.stderr)[-2000:]
