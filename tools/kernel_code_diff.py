#!/usr/bin/env python3
"""kernel_code_diff.py PARENT.co TREE.co : compares two gfx950 device code objects (what tools/device_code_sha.sh hashes; building with
D2D_OUT=<file> and its flags keeps one) function by function, for a tree that ADDS kernels and is meant to change none.

The whole-object sha256 of such a tree differs from its parent's, and so do a few bytes inside unchanged kernels: a kernel reaches its
constant tables (and a called function) through pc-relative 32-bit literals, and new code moves sections and functions against each
other.  So every function and kernel descriptor of PARENT is looked up in TREE by name and has to be
  identical    the same size and the same bytes, or
  relocated    the same size, and every 4-byte word that differs differs by exactly (displacement of some symbol both objects have)
               - (displacement of the function itself): the literal of a reference to that symbol from code that moved
A kernel descriptor is compared without its KERNEL_CODE_ENTRY_BYTE_OFFSET (bytes 16-23, the distance from the descriptor to the code).
Prints every symbol that is neither, the symbols only TREE has, a summary, and exits 0 only if nothing of PARENT is changed or missing.

tools/restamp_pmc.py --added-kernels uses this."""
import re
import struct
import subprocess
import sys

READELF = '/opt/rocm/llvm/bin/llvm-readelf'


def symbols(path):
    """name -> (address, bytes) of every FUNC and OBJECT symbol of the code object's symbol table"""
    data = open(path, 'rb').read()
    out = subprocess.run([READELF, '-S', '-s', '--wide', path], check=True, capture_output=True, text=True).stdout
    secs = {}
    for m in re.finditer(r'^\s*\[\s*(\d+)\]\s+(\S+)\s+(\S+)\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', out, re.M):
        secs[int(m.group(1))] = (m.group(3), int(m.group(4), 16), int(m.group(5), 16))
    syms = {}
    for m in re.finditer(r'^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)', out, re.M):
        addr, size, kind, ndx, name = int(m.group(1), 16), int(m.group(2)), m.group(3), int(m.group(4)), m.group(5)
        stype, saddr, soff = secs[ndx]
        b = b'' if stype == 'NOBITS' else data[addr - saddr + soff: addr - saddr + soff + size]
        if name.endswith('.kd'):
            b = b[:16] + b[24:]
        syms[name] = (kind, addr, b)
    return syms


def compare(parent, tree):
    """(identical, relocated {name: words}, changed [(name, why)], added) over the functions and kernel descriptors of `parent`"""
    a, b = symbols(parent), symbols(tree)
    moved = {n: b[n][1] - a[n][1] for n in a if n in b}                   # displacement of every symbol both objects have
    identical, relocated, changed = [], {}, []
    for n, (kind, addr, code) in sorted(a.items()):
        if kind != 'FUNC' and not n.endswith('.kd'):
            continue                                                      # (a table's bytes are compared where it is a kernel's operand: below)
        if n not in b:
            changed.append((n, 'missing'))
        elif b[n][2] == code:
            identical.append(n)
        elif len(b[n][2]) != len(code) or kind != 'FUNC':
            changed.append((n, f'{len(code)} -> {len(b[n][2])} bytes' if len(b[n][2]) != len(code) else 'descriptor differs'))
        else:
            allowed = {d - moved[n] for d in moved.values()} - {0}
            words = [o for o in range(0, len(code) - 3, 4) if code[o:o + 4] != b[n][2][o:o + 4]]
            off = [o for o in words if struct.unpack_from('<i', b[n][2], o)[0] - struct.unpack_from('<i', code, o)[0] not in allowed]
            if off or len(code) % 4:
                changed.append((n, f'{len(off)} words differ by something that is no displacement (first at byte {off[0] if off else -1})'))
            else:
                relocated[n] = len(words)
    tables = [(n, 'constant table differs') for n, (kind, _, data) in sorted(a.items())
              if kind == 'OBJECT' and not n.endswith('.kd') and '__hip_cuid' not in n and (n not in b or b[n][2] != data)]
    return identical, relocated, changed + tables, sorted(set(b) - set(a))


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    identical, relocated, changed, added = compare(sys.argv[1], sys.argv[2])
    for name, why in changed:
        print('CHANGED', name, why)
    for name in added:
        print('ADDED', name)
    print(f'{len(identical)} identical, {len(relocated)} relocated only ({sum(relocated.values())} literals), {len(changed)} changed, '
          f'{len(added)} added')
    sys.exit(1 if changed or not (identical or relocated) else 0)


if __name__ == '__main__':
    main()
