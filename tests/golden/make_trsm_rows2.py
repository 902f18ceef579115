#!/usr/bin/env python3
"""Generate trsm_rows2.json: the digests (tests/_trsm_rows2_cases.py) of every case's pass script, computed on an MI355X with the
library the caller points at (PYMRA_AMD_LIB, default the tree's).  The committed file was written by the build of commit e7339b1,
the last one whose k_trsm_rows2 carried its row-tile body inline: tests/test_gpu_trsm_rows2.py holds every later body to its bits.
A few seconds.

    python tests/golden/make_trsm_rows2.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import _trsm_rows2_cases as TC                   # noqa: E402
from pymra_amd import plan                       # noqa: E402

out = {}
for key, opts in TC.CASES:
    out[TC.case_id(key, opts)] = TC.digest(*TC.run_script(plan, key, opts))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "trsm_rows2.json")
json.dump(out, open(path, "w"), indent=1, sort_keys=True)
print("%s: %d cases" % (path, len(out)))
