"""Hidden steps of the persistent closed loop (include/d2d.h, d2d_closed_loop), the parts a CPU can check: the header states the
visibility rule, the switch that makes every step visible reaches the library from Python, and the PMC records describe the kernels
in the tree (tests/test_profiles.py)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = 'D2D_OBS_EVERY_STEP'


def _closed_loop_comment():
    text = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int d2d_closed_loop\(', text, flags=re.S)
    assert m, 'no comment in front of d2d_closed_loop'
    return re.sub(r'\s*\n \*\s*', ' ', m.group(1))


def test_header_names_the_visibility_rule():
    doc = _closed_loop_comment()
    for phrase in ('obs_local and obs_yaw, together or not at all', 'the last step of the call', "`done` flag", 'D2D_DONE_FREEZE',
                   'exactly the bytes', SWITCH + '=1', 'plan->launch_args == NULL'):
        assert phrase in doc, phrase


def test_the_abi_version_is_unchanged():
    from drone2d_amd import _abi as A
    text = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    assert int(re.search(r'#define D2D_ABI_VERSION (\d+)', text).group(1)) == A.D2D_ABI_VERSION == 8


def test_the_switch_reaches_the_library():
    """_lib adds nothing of its own: the library reads the process environment at every call, and what os.environ is given is what
    the C library's getenv returns.  The kernels' source reads the switch and parks it with the launch arguments.
    What this does NOT show: the switch arriving at a launch.  No test here observes that.  A CPU test cannot, and the GPU test
    (tests/test_gpu_hidden_obs.py) cannot by comparing arrays, because both variants leave the same bytes by design: only a counter
    pass with the switch set (WRITE_SIZE per env-step back at the parent's figure, profiles/hidden_obs.json) would show it."""
    libc = C.CDLL(None)
    libc.getenv.restype = C.c_char_p
    old = os.environ.get(SWITCH)
    try:
        os.environ[SWITCH] = '1'
        assert libc.getenv(SWITCH.encode()) == b'1'
        del os.environ[SWITCH]
        assert libc.getenv(SWITCH.encode()) is None
    finally:
        if old is not None:
            os.environ[SWITCH] = old
    src = open(os.path.join(ROOT, 'gym-drone2d-activeperception_amd', 'csrc', 'd2d_hip.hip')).read()
    assert f'getenv("{SWITCH}")' in src and re.search(r'struct ClosedArgs \{[^}]*\bint obs_every;', src)
    from drone2d_amd import _lib
    assert SWITCH not in open(_lib.__file__).read()        # no second reader that could disagree with the library's


def test_pmc_records_match_the_kernel_sources():
    import test_profiles
    test_profiles.test_pmc_records_describe_the_kernels_in_the_tree()
