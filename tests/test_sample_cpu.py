"""The sampler's CPU-side contract: the NumPy restatement of its Philox4x32-10 draws against the Random123 known-answer vectors,
and the Python / C surface it is reached through (HipPlan.sample, MRATree.simulate, mra_sample / mra_sample_slots)."""
import numpy as np

import _cases as K  # noqa: F401  (puts the repository on sys.path)
import _philox


def _hexwords(w):
    return ["%08x" % int(x) for x in np.asarray(w).ravel()]


def test_philox4x32_10_known_answers():
    kat = [
        ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
    ]
    for ctr, key, want in kat:
        got = _philox.philox4x32_10([np.array([c], dtype=np.uint32) for c in ctr], (np.uint32(key[0]), np.uint32(key[1])))
        assert " ".join(_hexwords(got)) == want


def test_latent_draws_are_a_function_of_seed_slot_sample():
    z = _philox.latent_draws(1234, np.arange(100), np.arange(5))
    assert z.shape == (5, 100) and np.all(np.isfinite(z))
    # chunking over samples or slots changes nothing
    assert np.array_equal(z[2:4], _philox.latent_draws(1234, np.arange(100), [2, 3]))
    assert np.array_equal(z[:, 40:60], _philox.latent_draws(1234, np.arange(40, 60), np.arange(5)))
    assert not np.array_equal(z, _philox.latent_draws(1235, np.arange(100), np.arange(5)))
    # 64-bit slot / sample / seed words all enter
    hi = _philox.latent_draws((1 << 40) + 7, [(1 << 33) + 1], [(1 << 35) + 2])
    assert hi.shape == (1, 1) and np.isfinite(hi[0, 0])
    big = _philox.latent_draws(7, np.arange(20000), [0]).ravel()
    assert abs(big.mean()) < 0.05 and abs(big.var() - 1.0) < 0.05


def test_sampler_surface_is_exported():
    from pymra_amd import plan
    from pymra_amd.MRATree import MRATree
    assert callable(getattr(plan.HipPlan, "sample", None)) and callable(getattr(plan.HipPlan, "sample_slots", None))
    assert callable(getattr(MRATree, "simulate", None))
    assert "mra_sample" in plan.EXPORTS and "mra_sample_slots" in plan.EXPORTS
    assert plan.MRA_SAMPLE_CONDITIONAL == 1
    hdr = open(K.os.path.join(K.ROOT, "include", "mra_hip.h")).read()
    assert "#define MRA_SAMPLE_CONDITIONAL 1u" in hdr


def test_gram_budget_option_round_trip(built_library, tmp_path):
    """MRA_OPT_SAMPLE_GRAM_BYTES (19) reads back what was set, 0 is the default and a negative budget is refused.  Host dry run
    (MRA_HOST_DRYRUN=1: the plan lives in host memory, nothing is launched), so this runs without a GPU."""
    import os
    import subprocess
    import sys
    child = tmp_path / "child.py"
    child.write_text(r'''
import os, sys
sys.path.insert(0, os.environ["MRA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRA_ROOT"], "tests"))
import _cases as K
from pymra_amd import plan as P
cs = K.load_case("g32")
pl = P.HipPlan(cs["topo"], 0)
assert pl.get_option(P.MRA_OPT_SAMPLE_GRAM_BYTES) == 0
for v in (1, 123456, 3 << 30, 0):
    pl.set_option(P.MRA_OPT_SAMPLE_GRAM_BYTES, v); assert pl.get_option(P.MRA_OPT_SAMPLE_GRAM_BYTES) == v
try:
    pl.set_option(P.MRA_OPT_SAMPLE_GRAM_BYTES, -1)
    raise SystemExit("a negative budget must be refused")
except P.MraError as e:
    assert e.code == -1
assert pl.get_option(P.MRA_OPT_SAMPLE_GRAM_BYTES) == 0
pl.close()
print("GRAM_OPT_OK")
''')
    env = dict(os.environ, MRA_ROOT=K.ROOT, MRA_HOST_DRYRUN="1")
    res = subprocess.run([sys.executable, str(child)], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "GRAM_OPT_OK" in res.stdout, (res.stdout + res.stderr)[-2000:]
