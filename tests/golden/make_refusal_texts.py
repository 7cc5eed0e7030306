"""Writes tests/golden/refusal_texts.json: every text tests/test_refusal_texts_cpu.py replays -- the refusals of the backend gates,
of the `worlds` arguments and of the loaders, and the key sets of the metric batches' timings.  Needs no GPU, only the built
libraries.  The recording in the tree comes from the package as it was before its loaders, binders, gates and table drivers were
each stated once:
    python tests/golden/make_refusal_texts.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import drone2d_amd as pkg                  # noqa: E402
import test_refusal_texts_cpu as T         # noqa: E402
from oracle_lib import OracleBackend       # noqa: E402

rec = T.record(pkg, OracleBackend())
with open(T.GOLDEN, 'w') as f:
    json.dump(rec, f, indent=1, sort_keys=True)
    f.write('\n')
print(f'{len(rec)} records -> {T.GOLDEN}')
