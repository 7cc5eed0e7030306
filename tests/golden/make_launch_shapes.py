"""Writes tests/golden/launch_shapes.json: what the HIP library (D2D_LIB, or the one built in the tree) answers for the tables of
tests/test_launch_shapes_cpu.py.  Needs no GPU.  Run it against a library whose answers are known to be right -- the recording in
the tree comes from the library before the host dispatch was folded into pick_launch():
    python tests/golden/make_launch_shapes.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import drone2d_amd as pkg                  # noqa: E402
import test_launch_shapes_cpu as T         # noqa: E402

rec = dict(shapes=T.record_shapes(pkg), refusals=T.record_refusals(pkg))
with open(T.GOLDEN, 'w') as f:
    json.dump(rec, f, indent=1, sort_keys=True)
    f.write('\n')
print(f"{len(rec['shapes'])} shapes, {len(rec['refusals'])} refusals -> {T.GOLDEN}")
