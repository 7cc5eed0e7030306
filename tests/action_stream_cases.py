"""Cases shared by tests/test_action_stream_cpu.py (the model backends of tests/action_stream_backend.py) and
tests/test_gpu_action_stream.py (the HIP backend): the four planner x motion-profile cells, the reference records of an episode
under the deterministic policy, and the comparisons of a whole stream, of a refilled slot and of the terminal state.  `make(params,
n, **kw)` builds a VecDrone2DEnv with device worlds and the caller's gaze on the backend under test.  Test infrastructure."""
import copy

import numpy as np
import torch

from action_stream_backend import policy
from drone2d_amd import _abi as A

BASE = dict(agent_number=6, agent_radius=10, agent_max_speed=40, drone_max_speed=40, max_flight_time=4)   # 41 steps end every episode
SLOTS, M = 5, 12
# the map ids at which, on the CPU model, an episode of the cell ends by collision and another by freezing (asserted where used)
CELLS = {
    'Primitive-CVM': dict(planner='Primitive', map_id=3),
    'Primitive-RVO': dict(planner='Primitive', motion_profile='RVO', map_id=3),
    'Jerk-CVM': dict(planner='Jerk_Primitive', map_id=100),
    'Jerk-RVO': dict(planner='Jerk_Primitive', motion_profile='RVO', map_id=100),
}
MAX_STEPS = 41
# ... and those at which, under one constant action, the five slots' first episodes do not all end at the same step
UNEVEN = {'Primitive-CVM': 3, 'Primitive-RVO': 3, 'Jerk-CVM': 200, 'Jerk-RVO': 200}


def params_of(pkg, cell, **kw):
    return pkg.Params(**dict(dict(BASE, **CELLS[cell]), **kw))


def unmasked_step(env, actions):
    """One step of every env, finished or not, with launches that exist without the stream: step() for Jerk_Primitive (perceive,
    plan, act), and perceive / d2d_plan_stage / act for the Primitive plugins, whose step() runs no plan stage"""
    if env.plugins is None:
        return env.step(actions)
    env.perceive()
    env.backend.plan_stage(env.cfg, env._st, env._plan)
    return env.act(actions)


def reference_records(make, p, n=M):
    """[n, 8]: an n-env batch of the map ids map_id + 0 .. n - 1, every env stepped with a = policy(env, step); each env's record
    (runner.batch_records) is kept from the first step at which its done byte is set"""
    from drone2d_amd import runner
    env = make(p, n)
    ep = torch.arange(n, device=env.device)
    rec = np.full((n, A.STREAM_ROW_F), -1, dtype=np.int64)
    for t in range(MAX_STEPS):
        unmasked_step(env, policy(ep, torch.full((n,), t, device=env.device)))
        now = runner.batch_records(env)
        new = (env.state.flags[:, A.F_DONE].cpu().numpy() != 0) & (rec[:, 0] < 0)
        rec[new] = now[new]
    assert (rec[:, 0] > 0).all()
    return rec


def drive(stream, on_call=None, limit=2000):
    """Steps `stream` until every episode is harvested.  The action of a slot is policy(episode, steps) of the step it is about to
    play: the driver queues the turn itself (ActionStream.turn) in front of the policy, so that the views of the previous call's info
    show a refilled slot at step 0 of its new episode -- with the turn left to step(), a fresh episode's first action would be the one
    computed from the terminal state of whichever episode the slot played before, and a record would depend on the slot.  Returns
    (calls, refills per slot)."""
    _, _, _, info = stream.result()
    calls, refills, last = 0, np.zeros(stream.env.num_envs, dtype=np.int64), info['episode'].cpu().numpy().copy()
    while stream.finished_now() < stream.num_episodes:
        assert calls < limit
        stream.turn()
        now = info['episode'].cpu().numpy()
        refills += (now != last) & (now >= 0)
        last = now.copy()
        out = stream.step(policy(info['episode'], info['steps']))
        info = out[3]
        calls += 1
        if on_call is not None:
            on_call(calls, out)
    return calls, refills


def stream_rows(make, p, slots, m, refill_every, **kw):
    env = make(p, slots)
    stream = env.action_stream(m, refill_every=refill_every, **kw)
    calls, refills = drive(stream)
    stream.close()
    return stream.rows.cpu().numpy().astype(np.int64), calls, refills


NOT_PER_SLOT = ('launch_args',)      # one block of launch arguments per batch: there is no row of a slot to compare


def tensors(env, e):
    """every per-slot tensor of d2d_state and of the plugin / Jerk / RVO state, row e (the list of tests/test_gpu_episode_stream.py)"""
    out = {'s.' + k: v[e] for k, v in env.state.t.items()}
    if env.plugins is not None:
        out.update({'p.' + k: v[e] for k, v in env.plugins.t.items() if k not in NOT_PER_SLOT})
        out['p.trk_radius0'] = env.plugins.trk_radius0[e]
    if env.jerk is not None:
        out.update({'j.' + k: v[e] for k, v in env.jerk.t.items()})
        out['j.trk_radius0'] = env.jerk.trk_radius0[e]
    return out


def differing(a, b):
    assert set(a) == set(b)
    return [k for k in sorted(a) if not torch.equal(a[k].reshape(-1).view(torch.uint8).cpu(), b[k].reshape(-1).view(torch.uint8).cpu())]


def check_refilled_slot_is_fresh(make, pkg, cell, slots=SLOTS, m=M):
    """Two streams get the same constant action: `a` turns at every call, `twin` never.  At the first call of `a` whose turn refills
    a slot, one step later: a refilled slot is env 0 of a fresh one-env VecDrone2DEnv of its map id after one unmasked step with the
    same action, in every tensor; every other slot is the twin's, bit for bit"""
    p = params_of(pkg, cell, map_id=UNEVEN[cell])
    a, twin = make(p, slots).action_stream(m, refill_every=1), make(p, slots).action_stream(m, refill_every=10 ** 9)
    act = torch.full((slots,), 0.25, dtype=torch.float64, device=a.env.device)
    before = None
    for call in range(MAX_STEPS + 2):
        before = a.slot_episode.cpu().numpy().copy()
        done_before = a.env.state.flags[:, A.F_DONE].cpu().numpy() != 0
        a.step(act)
        twin.step(act)
        if done_before.any():
            break
    a.env.sync()
    now = a.slot_episode.cpu().numpy()
    refilled = np.nonzero(done_before)[0]
    assert len(refilled) and 0 < len(refilled) < slots and (now[refilled] >= slots).all() and (now[~done_before] == before[~done_before]).all()
    assert a.refill.cpu().numpy().tolist() == done_before.astype(int).tolist()
    for e in range(slots):
        if e in refilled:
            q = copy.copy(a.env.params)
            q.map_id = p.map_id + int(now[e])
            fresh = make(q, 1)
            unmasked_step(fresh, act[:1])
            fresh.sync()
            assert differing(tensors(a.env, e), tensors(fresh, 0)) == [], (cell, e, 'fresh')
            assert int(a.explored[e]) == int((fresh.state.dmap != 0).sum()) > 0
        else:
            assert differing(tensors(a.env, e), tensors(twin.env, e)) == [], (cell, e, 'twin')
    a.close()
    twin.close()


def check_terminal_state(make, pkg, cell, slots=3, m=6):
    """In the call where done[e] first turns true the result is the finished episode's; the next call's harvest writes the row that
    agrees with it; after that call the slot shows the new episode, and explored is the fresh world's first-step count"""
    from drone2d_amd import runner
    p = params_of(pkg, cell, map_id=UNEVEN[cell])
    stream = make(p, slots).action_stream(m, refill_every=1)
    env = stream.env
    act = torch.full((slots,), -0.5, dtype=torch.float64, device=env.device)
    was_done = np.zeros(slots, dtype=bool)
    checked = 0
    for call in range(3 * MAX_STEPS):
        obs, terms, done, info = stream.step(act)
        d = done.cpu().numpy()
        first = np.nonzero(d & ~was_done)[0]
        if len(first) and checked == 0:
            e = int(first[0])
            k = int(info['episode'][e])
            assert k == e and bool(info['live'][e]) and int(info['steps'][e]) == int(env.state.counters[e, A.C_STEPS]) > 0
            rec = runner.batch_records(env)[e]
            flags = (int(terms['collision'][e]), int(terms['dead_lock'][e]), int(terms['freezing'][e]))
            assert flags == tuple(int(x) for x in rec[A.STREAM_R_FLAG0:A.STREAM_R_FLAG0 + 3])
            assert any(flags) or bool(terms['goal'][e])               # something ended the episode
            assert bool(terms['goal'][e]) == (rec[A.STREAM_R_SM] == A.SM_GOAL_REACHED)
            assert obs['local_map'].shape[0] == slots and torch.equal(obs['local_map'][e, 0], env.state.obs_local[e])
            assert int(stream.rows[k, 0]) == -1                       # not harvested yet: the turn sits at the start of the next call
            obs2, terms2, done2, info2 = stream.step(act)
            assert stream.rows[k].cpu().numpy().tolist() == rec.tolist()
            assert int(info2['episode'][e]) == slots + 0 and int(info2['steps'][e]) == 1 and not bool(done2[e]) and bool(info2['live'][e])
            assert int(terms2['explored'][e]) == int((env.state.dmap[e] != 0).sum()) > 0       # not a difference against the old world
            assert stream.finished_now() == len(first)
            checked = 1
            d = done2.cpu().numpy()
        was_done = d
        if checked:
            break
    assert checked
    stream.close()


TABLE_STARTS = [(50, 50), (250, 60), (60, 400), (300, 300)]
TABLE = [(3 + k, TABLE_STARTS[k % 4], [(420 - 30 * (k % 3), 430)]) for k in range(8)]      # (map id, start, target list)


def check_table_form(pkg, twin_of, env_of_worlds, device_worlds_of):
    """8 rows of (map id, start, target) over 3 slots with every action 1.0: the records of stream_episodes(episodes=...) on a twin env
    with gaze='Rotating', the one policy the device-gaze stream can check directly.  twin_of(params, table, slots) -> a
    runner.EpisodeStream; device_worlds_of(list of Params) -> DeviceWorlds; env_of_worlds(params, slots, worlds) -> the env"""
    from drone2d_amd import vec_env
    p = params_of(pkg, 'Primitive-CVM', gaze_method='Rotating')
    twin = twin_of(p, TABLE, 3)
    twin.run(refill_every=8)
    env = env_of_worlds(twin.params, 3, device_worlds_of(vec_env.table_params(twin.params, TABLE[:3])))
    stream = env.action_stream(episodes=TABLE, refill_every=1)
    ones = torch.ones(3, dtype=torch.float64, device=env.device)
    calls = 0
    while stream.finished_now() < len(TABLE):
        stream.step(ones)
        calls += 1
        assert calls < 400
    stream.close()
    rows = stream.rows.cpu().numpy()
    assert np.array_equal(rows, twin.records), (rows.tolist(), twin.records.tolist())
    assert len({tuple(r) for r in rows.tolist()}) > 3
