#!/usr/bin/env python3
"""restamp_pmc.py PARENT_TREE [--added-kernels] : carries profiles/pmc_latest.json over a change of the kernel sources' text that leaves the device code
as it was (host code next to the kernels: a new entry point, say).

tests/test_profiles.py ties every PMC record to tools/src_hash.py's hash of the sources it was measured on, which also covers the host
code in csrc/d2d_hip.hip.  Where tools/device_code_sha.sh gives the same sha256 for this tree and for PARENT_TREE (a `git worktree` of
the commit the records were measured on), for the product build and the -DD2D_GAZE_EXACT_ONLY build, the measured kernels ARE the
shipped kernels, and the records take the new hash; `restamped` in the file keeps the old hash, the new one and the two sha256.

--added-kernels: for a tree that ADDS kernels to the library and changes none.  Its code object cannot have the parent's sha256, so the
two objects are compared function by function (tools/kernel_code_diff.py): every function and kernel descriptor of the parent has to be
in the tree with the same bytes, but for the pc-relative literals of references that new code displaced, each checked against the
symbols' displacements.  `restamped` then keeps the counts (identical, relocated only, added) in place of a common sha256.

Anything else is refused: the records then have to be measured again (tools/gpu_profile_all.sh, tools/collect_profiles.sh)."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from src_hash import source_hash  # noqa: E402

PMC = os.path.join(ROOT, 'profiles', 'pmc_latest.json')


def device_sha(tree, flags=''):
    env = dict(os.environ, D2D_EXTRA_FLAGS=flags)
    return subprocess.run(['bash', os.path.join(ROOT, 'tools', 'device_code_sha.sh'), tree], env=env, check=True, capture_output=True,
                          text=True).stdout.strip()


def device_object(tree, flags, out):
    """the device code object tools/device_code_sha.sh hashes, kept as `out`"""
    env = dict(os.environ, D2D_OUT=out, D2D_EXTRA_FLAGS=f'{flags} --cuda-device-only --no-gpu-bundle-output -cuid=d2d -c')
    return subprocess.Popen(['bash', os.path.join(tree, 'gym-drone2d-activeperception_amd', 'csrc', 'build.sh')], env=env,
                            stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)


def added_kernels(parent):
    """name of the build -> what kernel_code_diff.compare found, or exit where a function of the parent is changed or missing"""
    from kernel_code_diff import compare
    builds = (('libd2d_hip.so', ''), ('libd2d_hip_exact.so', '-DD2D_GAZE_EXACT_ONLY'))
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(name, which, device_object(tree, flags, os.path.join(tmp, f'{which}_{name}.co')))
                for name, flags in builds for which, tree in (('parent', parent), ('tree', ROOT))]
        for name, which, job in jobs:
            err = job.communicate()[1]
            if job.returncode:
                sys.exit(f'{name} ({which}): the build failed\n{err}')
        for name, _ in builds:
            identical, relocated, changed, added = compare(os.path.join(tmp, f'parent_{name}.co'), os.path.join(tmp, f'tree_{name}.co'))
            if changed or not added:
                sys.exit(f'{name}: {len(changed)} functions of the parent are changed or missing, {len(added)} symbols added '
                         f'({changed[:3]}): measure the records again')
            found[name] = {'identical': len(identical), 'relocated_only': len(relocated), 'relocated_literals': sum(relocated.values()),
                           'added': added}
    return found


def main():
    args = [a for a in sys.argv[1:] if a != '--added-kernels']
    if len(args) != 1:
        sys.exit(__doc__)
    parent = os.path.abspath(args[0])
    old, new = source_hash(parent), source_hash(ROOT)
    text = open(PMC).read()
    if old == new or old not in text:
        sys.exit(f'nothing to do: parent hash {old}, tree hash {new}, {text.count(old)} records carry the parent hash')
    if '--added-kernels' in sys.argv[1:]:
        found = added_kernels(parent)
        d = json.loads(text.replace(old, new))
        d.setdefault('restamped', []).append({'from': old, 'to': new, 'added_kernels': found})
        with open(PMC, 'w') as f:
            json.dump(d, f, indent=1)
        print(f'{text.count(old)} records: {old} -> {new}', found)
        return
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
