#!/usr/bin/env python3
"""restamp_pmc.py PARENT_TREE : carries profiles/pmc_latest.json over a change of the kernel sources' text that leaves the device code
as it was (host code next to the kernels: a new entry point, say).

tests/test_profiles.py ties every PMC record to tools/src_hash.py's hash of the sources it was measured on, which also covers the host
code in csrc/d2d_hip.hip.  Where tools/device_code_sha.sh gives the same sha256 for this tree and for PARENT_TREE (a `git worktree` of
the commit the records were measured on), for the product build and the -DD2D_GAZE_EXACT_ONLY build, the measured kernels ARE the
shipped kernels, and the records take the new hash; `restamped` in the file keeps the old hash, the new one and the two sha256.
Anything else is refused: the records then have to be measured again (tools/gpu_profile_all.sh, tools/collect_profiles.sh)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from src_hash import source_hash  # noqa: E402

PMC = os.path.join(ROOT, 'profiles', 'pmc_latest.json')


def device_sha(tree, flags=''):
    env = dict(os.environ, D2D_EXTRA_FLAGS=flags)
    return subprocess.run(['bash', os.path.join(ROOT, 'tools', 'device_code_sha.sh'), tree], env=env, check=True, capture_output=True,
                          text=True).stdout.strip()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    parent = os.path.abspath(sys.argv[1])
    old, new = source_hash(parent), source_hash(ROOT)
    text = open(PMC).read()
    if old == new or old not in text:
        sys.exit(f'nothing to do: parent hash {old}, tree hash {new}, {text.count(old)} records carry the parent hash')
    shas = {}
    for name, flags in (('libd2d_hip.so', ''), ('libd2d_hip_exact.so', '-DD2D_GAZE_EXACT_ONLY')):
        a, b = device_sha(parent, flags), device_sha(ROOT, flags)
        if a != b:
            sys.exit(f'{name}: device code differs ({a} parent, {b} tree): measure the records again')
        shas[name] = b
    d = json.loads(text.replace(old, new))
    d.setdefault('restamped', []).append({'from': old, 'to': new, 'device_code_sha256': shas})
    with open(PMC, 'w') as f:
        json.dump(d, f, indent=1)
    print(f'{text.count(old)} records: {old} -> {new}', shas)


if __name__ == '__main__':
    main()
