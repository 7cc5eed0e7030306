"""What-if over gaze actions: K candidate actions tried from the present state of every slot of an env, for a few steps, in a scratch
env -- the lookahead baseline to put beside Oxford and Owl, and the inner loop of a tree search (which this is not: it is the
building block).  The state goes over by one launch (VecDrone2DEnv.load_slots, include/d2d_fork.h) and nothing is read back.

    env = VecDrone2DEnv(p, B, planner='Primitive', device_plugins=True, gaze='external', worlds='device')
    scratch, stream = env.sibling(K * B), env.action_stream()
    candidates = torch.linspace(-1, 1, K, dtype=torch.float64, device=env.device)
    actions = candidates[branch_terms(env, scratch, candidates, horizon=5)['newly_tracked'].argmax(0)]
    obs, terms, done, info = stream.step(actions)
"""
import torch

from . import _abi as A


def branch_terms(env, scratch, candidates, horizon, hold=True):
    """`candidates`: [K] or [K, B] float64 on the device (B = env.num_envs); `scratch`: env.sibling(K * B).  Slot k * B + e of
    `scratch` is loaded from slot e of `env` and stepped `horizon` times through the env's own episode loop, finished slots left
    alone: the first step with candidate k's action, the later ones with the same action (`hold`) or with 0.  Returns device
    tensors [K, B]: newly_tracked (the sum of the steps' newly tracked agents), explored (the increase of the slot's discovered
    cells, d2d_stream_explored behind the last step minus in front of the first), collision (0 none, 1 static, 2 dynamic), goal,
    dead_lock, freezing (as the branch ended) and steps (the steps the branch played before its episode ended; 0 for a slot that was
    finished already).  `env` is only read -- it may have an open action_stream -- and no host read happens."""
    if env.device_gaze is not None or (env.plugins is None and env.jerk is None):
        raise RuntimeError("branch_terms() needs device_plugins=True, planner='Primitive' or 'Jerk_Primitive' and gaze='external': the "
                           'candidates are the actions, and the episode loop leaves finished slots alone')
    B, dev = env.num_envs, env.device
    if not isinstance(candidates, torch.Tensor) or candidates.dtype != torch.float64 or candidates.device != env.state.action.device:
        raise TypeError(f'branch_terms(): candidates is a float64 tensor on {env.state.action.device}')
    if candidates.dim() not in (1, 2) or (candidates.dim() == 2 and candidates.shape[1] != B):
        raise ValueError(f'branch_terms(): candidates has shape {tuple(candidates.shape)}: [K] or [K, {B}]')
    K = int(candidates.shape[0])
    if scratch.num_envs != K * B:
        raise ValueError(f'branch_terms(): scratch has {scratch.num_envs} slots, {K} candidates x {B} slots need {K * B} (env.sibling)')
    from ._lib import backend_for
    backend_for(scratch.backend, None, 'supports_action_stream', 'has no per-slot count of discovered cells (include/d2d_worlds_turn.h: '
                'd2d_stream_explored)')
    s = scratch.state
    act = (candidates[:, None].expand(K, B) if candidates.dim() == 1 else candidates).reshape(K * B)
    src_of = torch.arange(K * B, dtype=torch.int32, device=dev) % max(B, 1)
    scratch.load_slots(env, src_of)
    i32 = dict(dtype=torch.int32, device=dev)
    before, after = torch.zeros(K * B, **i32), torch.zeros(K * B, **i32)
    newly, steps = torch.zeros(K * B, **i32), torch.zeros(K * B, **i32)
    live = torch.zeros(K * B, dtype=torch.bool, device=dev)
    if K * B:
        scratch.backend.stream_explored(scratch.cfg, scratch._st, before)
    for t in range(int(horizon)):
        if not K * B:
            break
        torch.eq(s.flags[:, A.F_DONE], 0, out=live)
        a = act if (t == 0 or hold) else torch.zeros_like(act)
        torch.where(live, a, s.action, out=s.action)          # a finished slot keeps its action, as it keeps everything else
        scratch._episode_steps(1)
        newly += torch.where(live, s.newly, torch.zeros_like(newly))
        steps += live.int()
    if K * B:
        scratch.backend.stream_explored(scratch.cfg, scratch._st, after)
    flags, sm = s.flags, s.counters[:, A.C_SM]
    return {'newly_tracked': newly.view(K, B), 'explored': (after - before).view(K, B),
            'collision': flags[:, A.F_COLLISION].clone().view(K, B), 'goal': (sm == A.SM_GOAL_REACHED).view(K, B),
            'dead_lock': flags[:, A.F_DEADLOCK].clone().view(K, B), 'freezing': flags[:, A.F_FREEZING].clone().view(K, B),
            'steps': steps.view(K, B)}
