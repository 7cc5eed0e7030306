"""The cells and the twin comparison of the slot-fork tests, shared by tests/test_fork_cpu.py (CPU stand-ins, tests/fork_backend.py)
and tests/test_gpu_fork_slots.py (the HIP library): an env A of 4 slots is stepped N0 times, a sibling S of 6 slots is loaded from it
with SRC_OF, and both are stepped N1 more times with slot e of S under the action of slot SRC_OF[e] of A; after the load and after
every step every item of S.fork_items() row e is bit-equal to A's row SRC_OF[e], and so are obs and done.
Test infrastructure: the product package never imports this."""
import numpy as np
import torch

from drone2d_amd import _abi as A

N0, N1 = 7, 25
B_A, B_S = 4, 6
SRC_OF = [3, 0, 0, -1, 2, 1]
CHANNELS = dict(swept_obs=True, seen_obs=True, scan_obs=True, tracks_obs=True)

# name -> (Params keywords, env keywords, the backend flags the cell needs that a CPU stand-in may lack)
# max_flight_time: the freezing rule ends every episode inside the N1 steps behind the fork, where nothing else has ended it
_BASE = dict(agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40, max_flight_time=2.5)
CELLS = {
    'primitive_cvm': (dict(_BASE, planner='Primitive'), dict(gaze='external'), ()),
    'primitive_rvo': (dict(_BASE, planner='Primitive', motion_profile='RVO'), dict(gaze='external'), ()),
    'jerk_cvm_owl': (dict(_BASE, planner='Jerk_Primitive', gaze_method='Owl'), dict(gaze='Owl'), ()),
    'jerk_rvo': (dict(_BASE, planner='Jerk_Primitive', motion_profile='RVO'), dict(gaze='external'), ()),
    'primitive_cvm_noise': (dict(_BASE, planner='Primitive', var_cam=2), dict(gaze='external'), ('supports_device_noise',)),
    'primitive_cvm_channels': (dict(_BASE, planner='Primitive'), dict(gaze='external', **CHANNELS), ()),
}
# The map id of slot 0 of A (slot i is map_id + i), and the witness per cell: (slot of A, its active trackers at the fork, the step
# that ended its episode) of a copied slot that has run a plan search before the fork, has an active tracker at the fork and ends its
# episode behind it.  Chosen with tools/fork_cells.py on the CPU stand-ins, the first base map id of 0, 4, .. 60 that has one, and
# asserted by the twin test itself on whichever backend runs it.  The stand-ins cannot draw the device's measurement noise: the
# noise cell's choice was made on its var_cam = 0 twin (the same agents and drone), and its tracker count is left to the device.
MAP_ID = {'primitive_cvm': 8, 'primitive_rvo': 8, 'jerk_cvm_owl': 8, 'jerk_rvo': 0, 'primitive_cvm_noise': 8, 'primitive_cvm_channels': 8}
WITNESS = {'primitive_cvm': (0, 1, 25), 'primitive_rvo': (0, 1, 25), 'jerk_cvm_owl': (0, 1, 25), 'jerk_rvo': (1, 1, 25),
           'primitive_cvm_noise': (0, None, 25), 'primitive_cvm_channels': (0, 1, 25)}


def params_of(pkg, cell, map_id=None):
    kw = dict(CELLS[cell][0])
    return pkg.Params(map_id=MAP_ID[cell] if map_id is None else map_id, **kw)


def env_kw(cell):
    return dict(CELLS[cell][1])


def actions(n, B, seed=0):
    """[n, B] seeded random actions in [-1, 1]"""
    return torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, (n, B)))


def raw(t):
    """the bytes of a tensor, so that NaNs compare as bit patterns"""
    return t.contiguous().reshape(-1).view(torch.uint8) if t.numel() else t


def step(env, act):
    """one step of the env's own episode loop, finished slots left alone, under the caller's action where the gaze is the caller's"""
    if env.device_gaze is None:
        live = env.state.flags[:, A.F_DONE] == 0
        env.state.action.copy_(torch.where(live, act.to(env.state.action.device), env.state.action))
    env._episode_steps(1)
    return env._result()


def check_rows(S, Aenv, src_of, where):
    """every item of S row e == A's row src_of[e], obs and done too"""
    pairs = [(e, s) for e, s in enumerate(src_of) if s >= 0]
    e_idx, s_idx = [e for e, _ in pairs], [s for _, s in pairs]
    for name, d, s in S.fork_items(Aenv):
        assert torch.equal(raw(d[e_idx]), raw(s[s_idx])), (where, name)
    (obs_s, _, done_s, _), (obs_a, _, done_a, _) = S._result(), Aenv._result()
    assert sorted(obs_s) == sorted(obs_a)
    for k in obs_s:
        assert torch.equal(raw(obs_s[k][e_idx]), raw(obs_a[k][s_idx])), (where, 'obs', k)
    assert torch.equal(done_s[e_idx], done_a[s_idx]), (where, 'done')


def searched(env):
    """[B] bool: the slot's planner has run a search (Primitive: plan_stat[0] counts them; Jerk_Primitive searches at every step)"""
    if env.plugins is not None:
        return env.plugins.t['plan_stat'][:, 0] > 0
    return env.state.counters[:, A.C_STEPS] > 0


def twins(make, sibling, witness=None, seed=0, at_fork=None):
    """the twin test of one cell.  `make()` builds A, `sibling(A, n)` its sibling; `at_fork(A)` looks at A as it is loaded from.
    Returns what the witness needs: per slot of A (searched before the fork, active trackers at the fork, the step that ended its
    episode or 0)"""
    Aenv = make()
    acts = actions(N0 + N1, B_A, seed)
    for t in range(N0):
        step(Aenv, acts[t])
    if at_fork is not None:
        at_fork(Aenv)
    S = sibling(Aenv, B_S)
    built = [(n, t[3].clone()) for n, t, _ in S.fork_items()]
    src_of = torch.tensor(SRC_OF, dtype=torch.int32, device=Aenv.device)
    status = S.load_slots(Aenv, src_of)
    assert status.tolist() == [1, 1, 1, 0, 1, 1]
    for (n, was), (_, now, _) in zip(built, S.fork_items()):
        assert torch.equal(raw(was), raw(now[3])), ('slot 3 as built', n)
    check_rows(S, Aenv, SRC_OF, 'load')
    seen_search, trackers = searched(Aenv).tolist(), Aenv.state.active.sum(1).tolist()
    gather = torch.tensor([max(s, 0) for s in SRC_OF])
    ended = [0] * B_A
    for t in range(N0, N0 + N1):
        step(Aenv, acts[t])
        step(S, acts[t][gather])
        check_rows(S, Aenv, SRC_OF, t)
        done = Aenv.state.flags[:, A.F_DONE].tolist()
        ended = [ended[i] or (t + 1 if done[i] else 0) for i in range(B_A)]
    got = [(bool(seen_search[i]), int(trackers[i]), int(ended[i])) for i in range(B_A)]
    if witness is not None:
        slot, n_trk, end = witness
        assert got[slot][0] and got[slot][1] > 0 and got[slot][1] == (got[slot][1] if n_trk is None else n_trk), (witness, got)
        assert got[slot][2] == end > N0, (witness, got)
        assert SRC_OF.count(slot) >= 1
    with np.testing.assert_raises(RuntimeError):
        S.reset()
    return got


def snapshot(env):
    """name -> a copy of every item of the env"""
    return {n: t.clone() for n, t, _ in env.fork_items()}


def same_slots(env, snap, slots, where):
    for n, t, _ in env.fork_items():
        assert torch.equal(raw(t[slots]), raw(snap[n][slots])), (where, n)


def in_place_case(make):
    """slots 1 .. 3 of a 4-slot env become slot 0: ten steps under equal actions leave the four equal in every item; under the actions
    [-1, -0.3, 0.3, 1] the four yaws differ after one step, and slot 0 equals an untouched twin that got -1 throughout"""
    env, twin = make(), make()
    acts = actions(N0 + 11, B_A, seed=3)
    for t in range(N0):
        step(env, acts[t])
        step(twin, acts[t])
    dev = env.device
    status = env.fork(torch.zeros(B_A, dtype=torch.int32, device=dev))
    assert status.tolist() == [0, 1, 1, 1]
    same_slots(env, snapshot(twin), [0], 'slot 0 is only read')
    for t in range(N0, N0 + 10):
        a0 = acts[t][:1].expand(B_A).clone()
        step(env, a0)
        step(twin, a0)
        for n, d, _ in env.fork_items():
            for e in (1, 2, 3):
                assert torch.equal(raw(d[e]), raw(d[0])), (t, n, e)
    spread = torch.tensor([-1.0, -0.3, 0.3, 1.0], dtype=torch.float64)
    step(env, spread)
    step(twin, torch.full((B_A,), -1.0, dtype=torch.float64))
    yaw = env.state.drone[:, A.D_YAW].tolist()
    assert len(set(yaw)) == B_A, yaw
    same_slots(env, snapshot(twin), [0], 'slot 0 against the untouched twin')
    with np.testing.assert_raises(RuntimeError):
        env.reset()


def branch_case(make, sibling, K=3, horizon=5):
    """whatif.branch_terms over K candidates of a 2-slot env against K twins built by hand and stepped: the [K, B] sums are equal and
    the env's tensors are bit-equal before and after"""
    from drone2d_amd import whatif
    B = 2
    env = make(B)
    acts = actions(N0, B, seed=5)
    for t in range(N0):
        step(env, acts[t])
    before = snapshot(env)
    cand = torch.tensor([-1.0, 0.25, 1.0], dtype=torch.float64, device=env.device)[:K]
    got = whatif.branch_terms(env, sibling(env, K * B), cand, horizon)
    same_slots(env, before, list(range(B)), 'branch_terms only reads the env')
    ident = torch.arange(B, dtype=torch.int32, device=env.device)
    for k in range(K):
        twin = sibling(env, B)
        assert twin.load_slots(env, ident).tolist() == [1] * B
        cells0 = (twin.state.logical('dmap') != 0).flatten(1).sum(1)
        newly = torch.zeros(B, dtype=torch.int64, device=env.device)
        steps = torch.zeros(B, dtype=torch.int64, device=env.device)
        for t in range(horizon):
            live = twin.state.flags[:, A.F_DONE] == 0
            step(twin, cand[k].expand(B).cpu())
            newly += torch.where(live, twin.state.newly.long(), torch.zeros_like(newly))
            steps += live.long()
        cells1 = (twin.state.logical('dmap') != 0).flatten(1).sum(1)
        assert got['newly_tracked'][k].long().tolist() == newly.tolist(), k
        assert got['explored'][k].long().tolist() == (cells1 - cells0).tolist(), k
        assert got['steps'][k].long().tolist() == steps.tolist(), k
        for name, col in (('collision', A.F_COLLISION), ('dead_lock', A.F_DEADLOCK), ('freezing', A.F_FREEZING)):
            assert got[name][k].tolist() == twin.state.flags[:, col].tolist(), (k, name)
        assert got['goal'][k].tolist() == (twin.state.counters[:, A.C_SM] == A.SM_GOAL_REACHED).tolist(), k
    assert all(tuple(v.shape) == (K, B) for v in got.values())
    assert bool((got['explored'] > 0).any()) and got['steps'].tolist() == [[horizon] * B] * K
    return got


# what hangs on the env itself with one row per slot and is no part of a slot's state, and why
ENV_TENSORS = {'reward': 'the reference\'s reward is 0 (drone_v2.py:257) and stays 0: nothing writes it',
               'tracker_radius': 'the host copy of the radii the worlds were built with: a constructor input, read by nothing afterwards'}
HOLDERS = ('state', 'plugins', 'jerk', 'gaze_state', 'swept', 'seen', 'scan', 'tracks')
NOT_HOLDERS = {'init_state': 'the reset snapshot: reset() refuses after a load'}


def reachable(env):
    """[(name, tensor)] of every tensor reachable from the holders, the test's own walk: the entries of a holder dict, of a holder's
    `t` under the holder's name, of its other dicts under theirs, and its tensor attributes"""
    out = []
    for h in HOLDERS:
        obj = getattr(env, h)
        if obj is None:
            continue
        if isinstance(obj, dict):
            out += [(f'{h}.{k}', v) for k, v in obj.items() if isinstance(v, torch.Tensor)]
            continue
        for k, v in vars(obj).items():
            if isinstance(v, torch.Tensor):
                out.append((f'{h}.{k}', v))
            elif isinstance(v, dict):
                out += [(f'{h}.{k2}' if k == 't' else f'{h}.{k}.{k2}', v2) for k2, v2 in v.items() if isinstance(v2, torch.Tensor)]
    return out


def completeness(env):
    """every reachable tensor with one row per slot is an item or has its line in fork.EXCLUDED; nothing else on the env looks like
    a holder"""
    from drone2d_amd import fork
    B = env.num_envs
    listed = {t.data_ptr() for _, t, _ in env.fork_items()}
    names = {n for n, _, _ in env.fork_items()}
    assert len(names) == len(env.fork_items()) <= A.FORK_MAX_ITEMS
    missing = [n for n, t in reachable(env) if t.dim() and t.shape[0] == B and t.numel() and t.data_ptr() not in listed
               and not fork.excluded(n)]
    assert not missing, missing
    assert all(isinstance(why, str) and len(why) > 20 for why in fork.EXCLUDED.values())
    for k, v in vars(env).items():
        per_slot = isinstance(v, torch.Tensor) and v.dim() and v.shape[0] == B
        holder = (isinstance(v, dict) and any(isinstance(x, torch.Tensor) for x in v.values())) or isinstance(getattr(v, 't', None), dict)
        if per_slot:
            assert k in ENV_TENSORS, f'env.{k}: a per-slot tensor on the env itself that no holder owns'
        if holder:
            assert k in HOLDERS or k in NOT_HOLDERS, f'env.{k}: a holder of tensors that fork_items() does not walk'
    return names


def stream_case(pkg, make, sibling):
    """four slots of a live action stream, refill_every = 1: after 12 steps all four are loaded into a sibling; the stream's next 8
    results equal the sibling's, slot for slot, until the slot refills (max_flight_time = 1.5 ends every episode inside those
    steps: the terminal step is compared, the steps of the next episodes are not); the stream's rows are those of a stream that
    was never read.  `make(params, B)` builds an env with device worlds and the caller's gaze"""
    p = pkg.Params(map_id=8, **dict(CELLS['primitive_cvm'][0], max_flight_time=1.5))
    env, ref = make(p, 4), make(p, 4)
    stream, unread = env.action_stream(12, refill_every=1), ref.action_stream(12, refill_every=1)
    dev = env.device
    acts = actions(20, 4, seed=7).to(dev)
    for t in range(12):
        stream.step(acts[t])
        unread.step(acts[t])
    S = sibling(env, 4)
    assert S.load_slots(env, torch.arange(4, dtype=torch.int32, device=dev)).tolist() == [1, 1, 1, 1]
    same, compared, ended = torch.ones(4, dtype=torch.bool, device=dev), 0, 0
    for t in range(12, 20):
        same &= env.state.flags[:, A.F_DONE] == 0         # a slot that is done refills at the start of this step
        obs, terms, done, info = stream.step(acts[t])
        unread.step(acts[t])
        obs_s, _, done_s, _ = step(S, acts[t])
        idx = same.nonzero().flatten()
        compared += len(idx)
        ended += int(done[idx].sum())
        for k in obs:
            assert torch.equal(raw(obs[k][idx]), raw(obs_s[k][idx])), (t, k)
        assert torch.equal(done[idx], done_s[idx]) and torch.equal(terms['newly_tracked'][idx], S.state.newly[idx]), t
        assert torch.equal(info['steps'][idx], S.state.counters[idx, A.C_STEPS]), t
        for name, d, s in S.fork_items(env):
            assert torch.equal(raw(d[idx]), raw(s[idx])), (t, name)
    stream.close()
    unread.close()
    assert 4 <= compared < 32 and ended == 4 and bool(done_s.all())     # every slot was followed to its episode's end and no further
    assert torch.equal(stream.rows, unread.rows) and bool((stream.rows[:4, 0] > 12).all())
