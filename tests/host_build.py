"""The gcc recipe that compiles a tests/csrc/*.c -- a header of the HIP libraries restated for the host -- once for every test module
that needs one.  Bit parity with libm and numpy rests on FLAGS: -ffp-contract=off (no fused multiply-add the source does not
spell out) and -mfma (the ones it does spell out are one instruction, as in the libm variants an FMA-capable CPU dispatches)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gym-drone2d-activeperception_amd', 'csrc')
FLAGS = ['-O2', '-ffp-contract=off', '-mfma']
SANITIZE = ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan']


def _source(name):
    return os.path.join(ROOT, 'tests', 'csrc', name)


def shared(source, tmpdir, name, include=CSRC, extra=()):
    """tests/csrc/`source` as the shared object `name` in `tmpdir`, loaded"""
    so = os.path.join(str(tmpdir), name)
    subprocess.check_call(['gcc'] + FLAGS + list(extra) + ['-fPIC', '-shared', '-I', include, '-o', so, _source(source), '-lm'])
    return C.CDLL(so)


def sanitized(sources, tmpdir, name, include=CSRC):
    """tests/csrc/`sources` as the stand-alone program `name` in `tmpdir` with AddressSanitizer and UBSan linked into it: run it as a
    child process; nothing sanitized is ever loaded into this one.  Returns its path."""
    exe = os.path.join(str(tmpdir), name)
    subprocess.check_call(['gcc'] + FLAGS + SANITIZE + ['-I', include, '-o', exe] + [_source(s) for s in sources] + ['-lm'])
    return exe


def _cpu_has_fma():
    try:
        return ' fma ' in open('/proc/cpuinfo').read()
    except OSError:
        return True


def needs_fma(reason):
    """skip mark for a comparison against code that takes another variant on a CPU without FMA; `reason` says which"""
    return pytest.mark.skipif(not _cpu_has_fma(), reason=reason)
