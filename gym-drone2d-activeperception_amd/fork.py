"""Slot forks — whole slot states copied between two VecDrone2DEnv or inside one, in one launch (include/d2d_fork.h,
VecDrone2DEnv.fork_items / load_slots / fork / sibling; whatif.branch_terms is the first user).

A slot's state is spread over the per-slot tensors of nine holders: `state.t`, `plugins.t` (and `trk_radius0`), `jerk.t` (and
`trk_radius0`), `gaze_state`, and the dicts of the four observation channels.  `slot_tensors(env)` is the one list of them.  It is
built by walking the holders, not by naming fields, so a tensor added to a holder later is copied without anybody remembering it; a
tensor that is NOT copied has a line in EXCLUDED that says why, and tests/test_gpu_fork_slots.py walks the holders a second time,
its own way, and fails for a per-slot tensor that is in neither.
"""
import numpy as np
import torch

from . import _abi as A

# name (or prefix ending in '.*') -> why the tensor is no part of a slot's state.  Nothing here is per-slot storage that a step
# reads: everything a slot's future or a caller's view of it depends on is copied (the default), dead or not.
EXCLUDED = {
    'plugins.launch_args': 'one argument block per batch (the persistent launch reads its own copy of cfg, state and plan): not per slot',
    'plugins.tables.*': "the planner's and the gaze policies' constant tables, equal in two envs of equal parameters (trk_radius0, "
                        'which is per slot, is listed under its own name)',
    'jerk.tables.*': "Jerk_Primitive's constant tables (headings, times, the tie table), equal in two envs of equal parameters",
    'gaze_state.owl_tab': "the Owl policy's constants, equal in two envs of equal parameters",
    'seen.tab': 'the table of the time-since-observed additions [2, n_calls], shared by every slot',
    'state._dummy': 'the target of empty fields (N == 0): never read as data',
    'state.noise': 'set_noise() rows belong to the envs they were drawn for; load_slots() refuses an env that has them',
}


def row_bytes(t):
    """bytes of one slot's row of the per-slot tensor t [B, ...]"""
    return (t.numel() // t.shape[0] if t.shape[0] else int(np.prod(t.shape[1:], dtype=np.int64))) * t.element_size()


def excluded(name):
    """the reason `name` is not copied, or None"""
    if name in EXCLUDED:
        return EXCLUDED[name]
    return next((why for k, why in EXCLUDED.items() if k.endswith('.*') and name.startswith(k[:-1])), None)


def slot_tensors(env):
    """[(name, tensor)] of every per-slot tensor of `env`, in holder order: a tensor is listed once, under the first name that reaches it
    (tracks.trk_radius is the device planner's).  Under RVO agent_vel and agent_vel_out are the buffers those names stand for NOW:
    the two swap every step, and two envs may be at different parity."""
    out, seen = [], set()

    def add(name, t):
        if not isinstance(t, torch.Tensor) or excluded(name) is not None:
            return
        if t.dim() < 1 or t.shape[0] != env.num_envs:
            raise RuntimeError(f'fork_items(): {name} has shape {tuple(t.shape)}: a per-slot tensor has num_envs = {env.num_envs} rows '
                               '(a shared tensor gets a line in fork.EXCLUDED)')
        if not t.is_contiguous():
            raise RuntimeError(f'fork_items(): {name} is not contiguous')
        if t.data_ptr() in seen or t.numel() == 0:
            return
        seen.add(t.data_ptr())
        out.append((name, t))

    for k, t in env.state.t.items():
        add('state.' + k, t)
    for holder, obj in (('plugins', env.plugins), ('jerk', env.jerk)):
        if obj is not None:
            for k, t in obj.t.items():
                add(f'{holder}.{k}', t)
            add(holder + '.trk_radius0', obj.trk_radius0)
    if env.gaze_state is not None:
        for k, t in vars(env.gaze_state).items():
            add('gaze_state.' + k, t)
    for holder in ('swept', 'seen', 'scan', 'tracks'):
        d = getattr(env, holder)
        if d is not None:
            for k, t in d.items():
                add(f'{holder}.{k}', t)
    return out


def signature(env):
    """the addresses of every tensor the holders hold, in the walk's order: what the packed item array of an env depends on (under
    RVO the velocity pair swaps every step, so an env has two).  Cheap enough for every call"""
    sig = [t.data_ptr() for t in env.state.t.values()]
    for obj in (env.plugins, env.jerk):
        if obj is not None:
            sig += [t.data_ptr() for t in obj.t.values()]
    if env.gaze_state is not None and env.gaze_state.owl_state is not None:
        sig.append(env.gaze_state.owl_state.data_ptr())
    for d in (env.swept, env.seen, env.scan, env.tracks):
        if d is not None:
            sig += [t.data_ptr() for t in d.values()]
    return tuple(sig)


def _ctor_views(env):
    """what two envs must agree in beyond cfg, as (field, value) pairs"""
    c = env._ctor
    yield 'planner', c['planner'] if c['planner'] is not None else env.params.planner
    yield 'device_plugins', bool(c['device_plugins'])
    yield 'gaze', env.device_gaze if (env.plugins is not None or env.jerk is not None) else c['gaze']
    yield 'motion_profile', env.params.motion_profile
    for ch in ('swept_obs', 'seen_obs', 'scan_obs', 'tracks_obs'):
        yield ch, getattr(env, ch)
    if env.tracks is not None:
        yield 'tracks_samples', int(env._tracks.samples)
        yield 'tracks_margin', float(env._tracks.margin)
    yield 'kf_enabled', bool(env.cfg.kf_enabled)


def check_now(dst, src, what):
    """the refusals of load_slots() that depend on what the two envs are doing, checked at every call"""
    for env, who in ((dst, 'this env'), (src, 'the source')):
        if env._own_noise:
            raise RuntimeError(f'{what}: noise: {who} has set_noise() rows installed, which belong to the envs they were drawn for and '
                               'not to the slots that pass through them; leave the draws to the device (var_cam != 0 on a backend with '
                               'supports_device_noise)')
    if getattr(dst, '_action_stream', None) is not None:
        raise RuntimeError(f'{what}: stream: this env has an open action_stream(), whose next turn would harvest the loaded slots under '
                           'episode numbers that are not theirs; close() it first (a SOURCE with an open stream is fine: it is only read)')


def check_pair(dst, src, what):
    """the refusals of load_slots() that compare what the two envs are, each naming its field: checked once per pair of buffer sets"""
    if dst is not src:
        for (n, _) in A.Cfg._fields_:
            if n != 'B' and getattr(dst.cfg, n) != getattr(src.cfg, n):
                raise ValueError(f'{what}: cfg.{n} is {getattr(dst.cfg, n)!r} here and {getattr(src.cfg, n)!r} in the source: two envs '
                                 'exchange slots only when they differ in the number of slots (cfg.B) alone')
        for (n, a), (_, b) in zip(_ctor_views(dst), _ctor_views(src)):
            if a != b:
                raise ValueError(f'{what}: {n} is {a!r} here and {b!r} in the source: the planner, device_plugins, the gaze policy, the '
                                 'motion profile and the observation channels of the two envs must be the same')
        if dst.device != src.device:
            raise ValueError(f'{what}: device is {dst.device} here and {src.device} in the source')


def items_of(dst, src, what='fork_items()'):
    """[(name, dst tensor, src tensor)]: slot_tensors of both envs side by side, or the ValueError that names the item whose name or
    row differs"""
    d, s = slot_tensors(dst), (slot_tensors(src) if src is not dst else None)
    if s is None:
        return [(n, t, t) for n, t in d]
    if [n for n, _ in d] != [n for n, _ in s]:
        odd = sorted(set(n for n, _ in d) ^ set(n for n, _ in s)) or ['(the order)']
        raise ValueError(f'{what}: item {odd[0]}: the two envs do not hold the same per-slot tensors ({", ".join(odd[:4])})')
    for (n, a), (_, b) in zip(d, s):
        if row_bytes(a) != row_bytes(b) or a.dtype != b.dtype:
            raise ValueError(f'{what}: item {n}: a slot\'s row is {row_bytes(a)} bytes of {a.dtype} here and {row_bytes(b)} bytes of '
                             f'{b.dtype} in the source')
    return [(n, a, b) for (n, a), (_, b) in zip(d, s)]


def pack_items(items, device):
    """(uint8 tensor on `device` holding the d2d_fork_item array, the number of items) of items_of()'s triples"""
    if len(items) > A.FORK_MAX_ITEMS:
        raise ValueError(f'd2d_fork_slots takes at most {A.FORK_MAX_ITEMS} items, got {len(items)}')
    arr = (A.ForkItem * max(len(items), 1))()
    for rec, (name, d, s) in zip(arr, items):
        rec.dst, rec.src, rec.dst_stride, rec.src_stride, rec.bytes = d.data_ptr(), s.data_ptr(), row_bytes(d), row_bytes(s), row_bytes(d)
    raw = np.frombuffer(bytes(arr), dtype=np.uint8).copy()
    return torch.from_numpy(raw).to(device), len(items)


def load_slots(dst, src, src_of, in_place):
    """VecDrone2DEnv.load_slots / fork: the checks, the packed items (kept per set of buffers: under RVO the velocity pair swaps every
    step, so there are up to four) and the one launch"""
    what = 'fork()' if in_place else 'load_slots()'
    from ._lib import backend_for
    backend_for(dst.backend, None, 'supports_fork', 'has no slot fork (include/d2d_fork.h: d2d_fork_slots): load_slots() / fork() run '
                'on the HIP backend, with csrc/fork/libd2d_fork.so built')
    if not hasattr(src, '_ctor') or not hasattr(src, 'state'):
        raise TypeError(f'{what}: the source is a VecDrone2DEnv')
    check_now(dst, src, what)
    if not isinstance(src_of, torch.Tensor) or src_of.dtype != torch.int32:
        raise TypeError(f'{what}: src_of is an int32 tensor on {dst.device} (got {getattr(src_of, "dtype", type(src_of).__name__)}): '
                        'the call reads nothing from the host')
    if tuple(src_of.shape) != (dst.num_envs,) or src_of.device != dst.state.action.device or not src_of.is_contiguous():
        raise ValueError(f'{what}: src_of has shape {tuple(src_of.shape)} on {src_of.device}, this env has [{dst.num_envs}] slots on '
                         f'{dst.state.action.device}')
    key = (signature(dst), signature(src))
    cache = dst.__dict__.setdefault('_fork_packed', {})
    if key not in cache:
        check_pair(dst, src, what)
        items = items_of(dst, src, what)
        if len(cache) >= 16:                   # (other sources come and go: the arrays are 2.5 KB each, the dict need not grow)
            cache.clear()
        cache[key] = pack_items(items, dst.device) + (items,)         # (the tensors outlive the launches)
    packed, n = cache[key][:2]
    status = torch.empty(dst.num_envs, dtype=torch.uint8, device=dst.device)
    if dst.num_envs:
        dst.backend.fork_slots(packed, n, src_of, src.num_envs, in_place, status)
        dst._streamed = True                   # the slots hold other worlds than the reset snapshot from here on
    return status
