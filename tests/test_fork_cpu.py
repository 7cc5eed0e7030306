"""Slot forks without a GPU (VecDrone2DEnv.fork_items / load_slots / fork / sibling, whatif.branch_terms) on the CPU stand-ins of
tests/fork_backend.py, whose d2d_fork_slots is the numpy model (tests/fork_model.py): the twin test of tests/fork_cases.py for every
cell the stand-ins can step, the fork in place, branch_terms, the completeness walk, every refusal of load_slots() by its message,
and include/d2d_fork.h against its ctypes mirror.

The cell the stand-ins cannot step: primitive_cvm_noise (Primitive x CVM with var_cam = 2) -- no CPU backend draws the device's
measurement noise (supports_device_noise); tests/test_gpu_fork_slots.py runs it."""
import ctypes as C
import os
import re

import pytest
import torch

import fork_backend as FB
import fork_cases as FC
import host_build
from drone2d_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = open(os.path.join(ROOT, 'include', 'd2d_fork.h')).read()
CPU_CELLS = [c for c, v in FC.CELLS.items() if not v[2]]


def make_of(pkg, cell, turn=False):
    def make(B=FC.B_A):
        return FB.env_of(FC.params_of(pkg, cell), B, channels='swept_obs' in FC.CELLS[cell][1], turn=turn, **FC.env_kw(cell))
    return make


def test_the_cells_the_stand_ins_cannot_step_are_the_ones_named():
    assert sorted(set(FC.CELLS) - set(CPU_CELLS)) == ['primitive_cvm_noise'] and 'primitive_cvm_noise' in __doc__


@pytest.mark.parametrize('cell', CPU_CELLS)
def test_twins(pkg, cell):
    def held(env):                             # the Owl cell forks while a decision is being held
        if cell == 'jerk_cvm_owl':
            assert bool((env.gaze_state.owl_state[:, A.OWL_S_LEFT] > 0).all())
    FC.twins(make_of(pkg, cell), FB.sibling_of, FC.WITNESS[cell], at_fork=held)


@pytest.mark.parametrize('cell', ['primitive_cvm', 'jerk_rvo'])
def test_fork_in_place_then_diverge(pkg, cell):
    FC.in_place_case(make_of(pkg, cell))


def test_branch_terms(pkg):
    FC.branch_case(make_of(pkg, 'primitive_cvm', turn=True), FB.sibling_of)


def test_from_a_live_action_stream(pkg):
    def make(p, B):
        env = FB.env_of(p, B, turn=True, worlds='device', gaze='external')
        return env
    FC.stream_case(pkg, make, FB.sibling_of)


def test_branch_terms_refusals(pkg):
    from drone2d_amd import whatif
    env = make_of(pkg, 'primitive_cvm', turn=True)(2)
    cand = torch.zeros(3, dtype=torch.float64)
    with pytest.raises(ValueError, match='scratch has 4 slots'):
        whatif.branch_terms(env, FB.sibling_of(env, 4), cand, 2)
    with pytest.raises(TypeError, match='float64'):
        whatif.branch_terms(env, FB.sibling_of(env, 6), cand.float(), 2)
    owl = make_of(pkg, 'jerk_cvm_owl')(2)
    with pytest.raises(RuntimeError, match="gaze='external'"):
        whatif.branch_terms(owl, FB.sibling_of(owl, 6), cand, 2)


@pytest.mark.parametrize('cell', ['primitive_cvm_channels', 'jerk_owl_rvo'])
def test_completeness(pkg, cell):
    if cell == 'jerk_owl_rvo':
        p = pkg.Params(planner='Jerk_Primitive', gaze_method='Owl', motion_profile='RVO', pillar_number=2, map_id=1, **FC._BASE)
        env = FB.env_of(p, 3, gaze='Owl')
    else:
        env = make_of(pkg, cell)(3)
    names = FC.completeness(env)
    want = {'state.drone', 'state.agent_vel', 'state.agent_vel_out', 'state.pillars', 'jerk.choice', 'jerk.trk_radius0',
            'gaze_state.owl_state'} if cell == 'jerk_owl_rvo' else \
        {'state.drone', 'plugins.nodes', 'plugins.trk_radius0', 'plugins.seen_step', 'swept.map', 'seen.last_call', 'scan.pose',
         'scan.last_step', 'tracks.win', 'tracks.last_step'}
    assert want <= names and 'plugins.launch_args' not in names and 'seen.tab' not in names
    # ... and it is the test that fails when the next channel forgets to register
    env.lidar = {'ranges': torch.zeros(3, 8)}
    with pytest.raises(AssertionError, match='env.lidar'):
        FC.completeness(env)


def test_the_velocity_pair_is_listed_by_what_the_names_stand_for_now(pkg):
    env = make_of(pkg, 'primitive_rvo')(2)
    first = {n: t.data_ptr() for n, t, _ in env.fork_items()}
    FC.step(env, torch.zeros(2, dtype=torch.float64))
    now = {n: t.data_ptr() for n, t, _ in env.fork_items()}
    assert now['state.agent_vel'] == first['state.agent_vel_out'] and now['state.agent_vel_out'] == first['state.agent_vel']
    sib = FB.sibling_of(env, 2)                 # at the other parity: the load goes by name
    assert sib.load_slots(env, torch.tensor([1, 0], dtype=torch.int32)).tolist() == [1, 1]
    assert torch.equal(sib.state.agent_vel, env.state.agent_vel[[1, 0]]) and torch.equal(sib.state.agent_vel_out, env.state.agent_vel_out[[1, 0]])


# ---------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_of_load_slots_names_its_field(pkg):
    make = make_of(pkg, 'primitive_cvm', turn=True)
    env = make(2)
    ok = torch.tensor([1, 0], dtype=torch.int32)

    def other(cell=None, **kw):
        pk = dict(FC.CELLS['primitive_cvm'][0], **kw.pop('params', {}))
        ek = dict(FC.env_kw('primitive_cvm'), **kw)
        return FB.env_of(pkg.Params(map_id=8, **pk), 2, turn=True, **ek)

    with pytest.raises(ValueError, match=r'cfg\.L is 33 here and 25 in the source'):
        env.load_slots(other(params=dict(drone_view_depth=60)), ok)
    with pytest.raises(ValueError, match=r'cfg\.N'):
        env.load_slots(other(params=dict(agent_number=7)), ok)
    with pytest.raises(ValueError, match=r'cfg\.planner_mode'):
        env.load_slots(other(planner='NoMove'), ok)
    with pytest.raises(ValueError, match="planner is 'Primitive' here and 'Jerk_Primitive' in the source"):
        env.load_slots(FB.env_of(FC.params_of(pkg, 'jerk_cvm_owl'), 2, gaze='external'), ok)
    with pytest.raises(ValueError, match='device_plugins is True here and False'):
        env.load_slots(other(device_plugins=False, gaze=None), ok)
    with pytest.raises(ValueError, match='gaze is'):
        env.load_slots(other(gaze='Rotating'), ok)
    with pytest.raises(ValueError, match='motion_profile is'):
        env.load_slots(FB.env_of(FC.params_of(pkg, 'primitive_rvo'), 2, gaze='external'), ok)
    rich = make_of(pkg, 'primitive_cvm_channels')(2)
    with pytest.raises(ValueError, match='swept_obs is'):
        env.load_slots(rich, ok)
    with pytest.raises(ValueError, match='tracks_samples is'):
        rich.load_slots(FB.env_of(FC.params_of(pkg, 'primitive_cvm_channels'), 2, channels=True,
                                  **dict(FC.env_kw('primitive_cvm_channels'), tracks_samples=9)), ok)
    src = make(2)
    for bad, exc, text in ((ok.long(), TypeError, 'int32'), ([1, 0], TypeError, 'int32'),
                           (torch.zeros(3, dtype=torch.int32), ValueError, r'shape \(3,\)'),
                           (torch.zeros((2, 1), dtype=torch.int32), ValueError, r'shape \(2, 1\)')):
        with pytest.raises(exc, match=text):
            env.load_slots(src, bad)
    with pytest.raises(ValueError, match='on meta, this env has .2. slots on cpu'):
        env.load_slots(src, torch.zeros(2, dtype=torch.int32, device='meta'))
    with pytest.raises(TypeError, match='VecDrone2DEnv'):
        env.load_slots(object(), ok)
    # item names / row bytes: two envs that pass every other check and hold other tensors
    odd = make(2)
    odd.plugins.t['extra'] = torch.zeros(2, 3)
    with pytest.raises(ValueError, match='item plugins.extra'):
        env.load_slots(odd, ok)
    del odd.plugins.t['extra']
    odd.plugins.t['plan_stat'] = torch.zeros((2, 5), dtype=torch.int32)
    with pytest.raises(ValueError, match='item plugins.plan_stat.*16 bytes.*20 bytes'):
        env.load_slots(odd, ok)
    # set_noise() rows on either side
    noisy = make(2)
    noisy.set_noise(torch.zeros(2, noisy.cfg.N, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='noise: the source has set_noise'):
        env.load_slots(noisy, ok)
    with pytest.raises(RuntimeError, match='noise: this env has set_noise'):
        noisy.load_slots(env, ok)
    # an open stream on the destination; on the source it is fine
    live = FB.env_of(FC.params_of(pkg, 'primitive_cvm'), 2, turn=True, worlds='device', **FC.env_kw('primitive_cvm'))
    stream = live.action_stream(4)
    with pytest.raises(RuntimeError, match='stream: this env has an open action_stream'):
        live.load_slots(src, ok)
    dst = FB.sibling_of(live, 2)
    assert dst.load_slots(live, ok).tolist() == [1, 1]
    stream.close()
    assert live.load_slots(src, ok).tolist() == [1, 1]
    # a backend without the launch
    from stepped_backend import SteppedOracleBackend
    from drone2d_amd import vec_env
    plain_b = SteppedOracleBackend()
    plain = plain_b.attach(vec_env.VecDrone2DEnv(FC.params_of(pkg, 'primitive_cvm'), 2, device='cpu', backend=plain_b, planner='Primitive',
                                                 device_plugins=True, gaze='external'))
    with pytest.raises(NotImplementedError, match='has no slot fork'):
        plain.load_slots(src, ok)


def test_after_a_load_reset_and_auto_reset_refuse_as_after_a_stream(pkg):
    env, src = make_of(pkg, 'primitive_cvm')(2), make_of(pkg, 'primitive_cvm')(2)
    env.reset()
    env.load_slots(src, torch.tensor([-1, -1], dtype=torch.int32))
    with pytest.raises(RuntimeError, match='other worlds than its snapshot'):
        env.reset()
    with pytest.raises(RuntimeError, match='auto_reset=True.: this env has streamed episodes'):
        env.closed_loop(1, auto_reset=True)


def test_the_model_launch_refuses_what_the_library_refuses(pkg):
    env = make_of(pkg, 'primitive_cvm')(2)
    items = torch.zeros(40 * 65, dtype=torch.uint8)
    with pytest.raises(ValueError, match='D2D_FORK_MAX_ITEMS'):
        env.backend.fork_slots(items, 65, torch.zeros(2, dtype=torch.int32), 2, 0, torch.zeros(2, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------- the ABI
class Recorder:
    def __getattr__(self, name):
        fn = type('fn', (), {})()
        self.__dict__[name] = fn
        return fn


def define(name):
    return int(re.search(r'#define\s+' + name + r'\s+(\w+)', TEXT).group(1), 0)


def test_the_constants_are_the_header_s():
    assert A.D2D_FORK_VERSION == define('D2D_FORK_VERSION') == 1
    assert (A.FORK_MAX_ITEMS, A.FORK_PARTS, A.FORK_SMALL_BYTES) == (define('D2D_FORK_MAX_ITEMS'), define('D2D_FORK_PARTS'), define('D2D_FORK_SMALL_BYTES'))
    assert (A.FORK_LEFT, A.FORK_COPIED, A.FORK_REFUSED) == (define('D2D_FORK_LEFT'), define('D2D_FORK_COPIED'), define('D2D_FORK_REFUSED')) == (0, 1, 2)


def test_every_entry_point_is_bound_with_the_header_s_arguments():
    bound = A.bind_fork(Recorder())
    declared = re.findall(r'^(?:int|const char \*)\s*(d2d_fork_\w+)\(([^;]*)\);', TEXT, re.M)
    assert sorted(n for n, _ in declared) == ['d2d_fork_last_error', 'd2d_fork_slots', 'd2d_fork_version']
    assert sorted('d2d_fork_' + k for k in bound) == sorted(n for n, _ in declared)
    kinds = {'int32_t': C.c_int32, 'int64_t': C.c_int64}
    for name, args in declared:
        args = re.sub(r'/\*.*?\*/', '', args.replace('\n', ' ')).strip()
        want = [] if args == 'void' else [C.c_void_p if '*' in a else kinds[a.split()[0]] for a in args.split(',')]
        fn = bound[name[len('d2d_fork_'):]]
        assert fn.argtypes == want, name
        assert fn.restype is (C.c_char_p if name.endswith('last_error') else C.c_int), name


def test_the_item_struct_is_the_header_s_field_for_field(tmp_path):
    body = re.search(r'typedef struct d2d_fork_item \{(.*?)\} d2d_fork_item;', TEXT, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        names = [n.strip() for n in decl.split(',')]
        head = names[0].rsplit(None, 1)
        kind, names[0] = head[0], head[1]
        for n in names:
            ptr = '*' in kind or n.startswith('*')
            fields.append((n.lstrip('*'), C.c_void_p if ptr else {'int64_t': C.c_int64}[kind.strip()]))
    assert fields == list(A.ForkItem._fields_)
    lib = host_build.shared('fork_host.c', tmp_path, 'libforkhost.so')
    assert lib.fork_host_version() == A.D2D_FORK_VERSION and lib.fork_host_item_bytes() == C.sizeof(A.ForkItem) == 40
    assert [lib.fork_host_item_offset(k) for k in range(5)] == [getattr(A.ForkItem, n).offset for n, _ in A.ForkItem._fields_]
    assert [lib.fork_host_constant(k) for k in range(7)] == [A.FORK_MAX_ITEMS, A.FORK_PARTS, A.FORK_SMALL_BYTES, A.FORK_LEFT, A.FORK_COPIED,
                                                             A.FORK_REFUSED, 64]


def test_the_library_is_registered_with_the_loader():
    from drone2d_amd import _lib
    assert _lib._LIBRARIES['libd2d_fork.so'][2:] == ('D2D_FORK_VERSION', 'version', 'fork/build.sh')
    assert _lib.FORK_LIB_PATH.endswith(os.path.join('csrc', 'fork', 'libd2d_fork.so')) and _lib.HipBackend.supports_fork
