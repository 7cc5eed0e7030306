"""swept_obs, seen_obs and scan_obs switched on together: the comparisons tests/test_obs_channels_cpu.py (the combined model backends
of tests/obs_channels_backend.py) and tests/test_gpu_obs_channels.py (the HIP libraries) share.  The per-channel suites tie each
channel alone to its model and to the reference's recordings; here an env with several channels is tied to the envs with one -- same
worlds, same actions, the launch sequence the combination selects -- and to the env with none, whose world the channels must not move.
`make(params, n, **keywords) -> env`.  Every comparison is exact equality: integers, and the bit patterns of floats.  Test
infrastructure."""
import numpy as np
import torch

import action_stream_cases as AC
import scan_cases as SCAN
import seen_cases as SEEN
import seen_model
from action_stream_backend import policy
from drone2d_amd import _abi as A

CHANNELS = ('swept', 'seen', 'scan')
OBS_KEY = {'swept': 'swep_map', 'seen': 'age_map', 'scan': 'scan'}
KEYSETS = {'none': (), 'swept': ('swept',), 'seen': ('seen',), 'scan': ('scan',), 'seen+scan': ('seen', 'scan'), 'all': CHANNELS}
B_PATH = 6


def keywords(channels):
    return {c + '_obs': True for c in channels}


def raw(t):
    return t.reshape(-1).view(torch.uint8)


def records(env, channel, rows=slice(None)):
    """every buffer of the channel, rows `rows`: the observation and the full records behind it (swept_map, swept_count and the live
    bytes; seen_calls, the call of the latest update and refreshed; ray_end, ray_kind, the hit words, the counter of the latest
    update and the pose the rays were cast from)"""
    d = getattr(env, channel)
    return {k: v[rows] for k, v in d.items() if k != 'tab'}


def differing(a, b):
    assert set(a) == set(b), (sorted(a), sorted(b))
    return [k for k in sorted(a) if a[k].shape != b[k].shape or not torch.equal(raw(a[k]), raw(b[k]))]


def state_of(env):
    """every per-slot tensor of the env and its plugins (action_stream_cases.tensors), all slots at once"""
    return AC.tensors(env, slice(None))


def check_channels(full, twins, channels, where):
    """the env with several channels shows, channel for channel, what the envs of `twins` with fewer show"""
    for c in channels:
        for name, twin in twins.items():
            if getattr(twin, c) is not None and twin is not full:
                assert differing(records(full, c), records(twin, c)) == [], (where, c, name)


def check_fresh(env, e, channels=CHANNELS):
    """slot e is at step 0 of a world: a zero swept map, crop and count, the call-1 time-since-observed map, no rays"""
    if 'swept' in channels:
        assert not any(bool(v.any()) for k, v in records(env, 'swept', e).items() if k != 'live'), e
    if 'seen' in channels:
        SEEN.check_call_1(env, e)
    if 'scan' in channels:
        SCAN.check_cleared(env, e)


PER_STEP = (('scan', 'pose'), ('swept', 'live'))      # written for every slot in front of every step: what the launches read, not records


def kept_of(env, e, channels=CHANNELS):
    return {c: {k: v.clone() for k, v in records(env, c, e).items() if (c, k) not in PER_STEP} for c in channels}


def check_kept(env, e, kept, where):
    """slot e finished earlier: its channels are as they ended (the pose snapshot and the mark's live bytes, written for every slot at
    every step, aside)"""
    for c, old in kept.items():
        now = {k: v for k, v in records(env, c, e).items() if k in old}
        assert differing(now, old) == [], (where, e, c)


# ---------------------------------------------------------------------------------------------------------------- streams
def stream_matrix(make, p, slots, M, refill_every=4, limit=2000):
    """One action stream per keyword set, all driven by the same policy with the turn in front of it.  After every step: the
    records, terms, done, info, local_map and yaw_angle of all six are equal; each channel of the all-three stream equals the same
    channel of its alone stream and of the {seen, scan} stream in every buffer; every per-slot tensor of the all-three env equals
    the no-channel env's.  A refilled slot is fresh in all three channels at its step 0 and a finished slot keeps them until the
    turn.  Returns the coverage: refills, frozen slot-steps checked, episodes ended by collision and by freezing, and per channel
    the steps at which its observation was not all zero"""
    streams = {k: make(p, slots, **keywords(v)).action_stream(M, refill_every=refill_every) for k, v in KEYSETS.items()}
    a, none = streams['all'], streams['none']
    envs = {k: s.env for k, s in streams.items()}
    assert all(getattr(a.env, c) is not None for c in CHANNELS) and not any(getattr(none.env, c) is not None for c in CHANNELS)
    for e in range(slots):
        check_fresh(a.env, e)
    info = a.result()[3]
    kept, calls = {}, 0
    cov = dict(refills=0, frozen=0, collision=0, freezing=0, nonzero={c: 0 for c in CHANNELS})
    while a.finished_now() < M:
        assert calls < limit
        last = info['episode'].clone()
        turned = a.turn()
        assert all(s.turn() == turned for k, s in streams.items() if k != 'all')
        obs, terms, done, info = a.result()
        a.env.sync()
        for e in range(slots):
            if int(info['episode'][e]) != int(last[e]) and int(info['episode'][e]) >= 0:     # refilled: step 0 of a fresh world
                assert turned and int(info['steps'][e]) == 0 and not bool(done[e])
                check_fresh(a.env, e)
                kept.pop(e, None)
                cov['refills'] += 1
            elif e in kept:                                                                  # done, not yet refilled: as it ended
                assert bool(done[e])
                check_kept(a.env, e, kept[e], calls)
                cov['frozen'] += 1
        if turned:
            check_channels(a.env, envs, CHANNELS, ('turn', calls))
            assert differing(state_of(a.env), state_of(none.env)) == [], ('turn', calls)
        act = policy(info['episode'], info['steps'])
        out = {k: s.step(act) for k, s in streams.items()}
        oa, ta, da, ia = out['all']
        on, tn, dn, inf = out['none']
        assert sorted(set(oa) - set(on)) == ['age_map', 'scan'] and sorted(set(ta) - set(tn)) == ['refreshed']
        for k, (o, t, d, i) in out.items():
            assert torch.equal(streams[k].rows, none.rows) and torch.equal(d, dn), (calls, k)
            assert all(torch.equal(t[n], tn[n]) for n in tn) and all(torch.equal(i[n], inf[n]) for n in inf), (calls, k)
            assert torch.equal(o['local_map'], on['local_map']) and torch.equal(o['yaw_angle'], on['yaw_angle']), (calls, k)
            for c in KEYSETS[k]:                   # the observation the caller is handed is the channel's own buffer
                assert torch.equal(raw(o[OBS_KEY[c]]), raw(oa[OBS_KEY[c]])), (calls, k, c)
        check_channels(a.env, envs, CHANNELS, calls)
        assert differing(state_of(a.env), state_of(none.env)) == [], calls
        a.env.sync()
        for c in CHANNELS:
            cov['nonzero'][c] += int(bool(oa[OBS_KEY[c]].any()))
        for e in range(slots):
            if bool(ia['live'][e]):
                assert int(a.env.scan['last_step'][e]) == int(ia['steps'][e]) >= 1, (calls, e)
                assert int(a.env.seen['last_call'][e]) == int(ia['steps'][e]) + 1, (calls, e)
            if bool(da[e]) and e not in kept and bool(ia['live'][e]):
                kept[e] = kept_of(a.env, e)
                cov['collision'] += int(ta['collision'][e] != 0)
                cov['freezing'] += int(ta['freezing'][e] != 0)
        info = ia
        calls += 1
    for s in streams.values():
        s.close()
    assert all(torch.equal(s.rows, none.rows) for s in streams.values()) and int((a.rows[:, 0] > 0).sum()) == M
    return cov


def check_stream_coverage(cov, slots, M, swept_marks):
    """refills == episodes - slots, a frozen slot was looked at, an episode ended either way, and no channel was all zero throughout:
    an all-zero channel is equal to anything that is broken the same way.  `swept_marks`: False under Jerk_Primitive, whose swept map
    is zero by definition (an empty trajectory at every replan_check)"""
    assert cov['refills'] == M - slots and cov['frozen'] >= 1 and cov['collision'] >= 1 and cov['freezing'] >= 1, cov
    assert cov['nonzero']['seen'] > 0 and cov['nonzero']['scan'] > 0 and (cov['nonzero']['swept'] > 0) == swept_marks, cov


def stream_episodes_pair(make, p, slots, M, refill_every=8):
    """stream_episodes() -- the device's own policy, refilled through _refill_rest and not through the restore list -- with all
    three channels against no channel: a refilled slot is fresh in all three, the records are equal.  Returns the slots refilled"""
    a, b = make(p, slots, gaze='Rotating', **keywords(CHANNELS)), make(p, slots, gaze='Rotating')
    refilled = 0
    gb = b.stream_rounds(M, refill_every=refill_every)
    for finished, refill in a.stream_rounds(M, refill_every=refill_every):
        fb, rb = next(gb)
        assert fb == finished and torch.equal(rb, refill)
        a.sync()
        for e in np.nonzero(refill.cpu().numpy())[0]:
            check_fresh(a, int(e))
            refilled += 1
        assert differing(state_of(a), state_of(b)) == [], finished
    assert next(gb, None) is None                  # (both streams ran dry in the same round)
    assert torch.equal(a.stream_rows, b.stream_rows) and int((a.stream_rows[:, 0] > 0).sum()) == M
    return refilled


# ---------------------------------------------------------------------------------------------------------------- step paths
def check_scan_model(env, e):
    return SCAN.check_against_model(env, e)


def check_seen_model(env, e, seen, last):
    """slot e's time-since-observed records are the model's, kept by the caller in (seen [W, H] int32, last) from the poses the env
    reports: SN.update marks `seen` in place and returns (call, refreshed, crop), or None where the launch leaves the env alone"""
    cfg, tab = env.cfg, env.seen['tab'].cpu().numpy()
    out = seen_model.update(seen, last, int(env.state.counters[e, A.C_STEPS]), env.state.drone[e].cpu().numpy(), cfg, env.params.drone_view_range, tab)
    if out is not None:
        last, n, crop = out
        assert int(env.refreshed[e]) == n and np.array_equal(SEEN.bits(env.seen['obs'][e].cpu().numpy()), SEEN.bits(crop)), e
    assert int(env.seen['last_call'][e]) == last and np.array_equal(env.seen_calls[e].cpu().numpy(), seen), e
    return last


def actions_at(t, device):
    ep = torch.arange(B_PATH, device=device)
    return policy(ep, torch.full((B_PATH,), t, device=device))


def check_counters(env, where, stepped=True):
    """scan['last_step'] is the env's step counter and seen['last_call'] the counter + 1 (the map as the pose behind the step sees it)"""
    steps = env.state.counters[:, A.C_STEPS]
    if env.scan is not None and stepped:
        assert torch.equal(env.scan['last_step'], steps), where
    if env.seen is not None:
        assert torch.equal(env.seen['last_call'], steps + 1), where


def path_case(make, p, step, channels, steps=AC.MAX_STEPS, env_kw=None, each=None):
    """One env per keyword set on one step path: all of `channels`, each alone, and none, on the same worlds under the same actions.
    After every step the all-channels env equals its twins channel for channel and the no-channel env in every tensor, and the
    channels' counters follow the env's.  `step(env, actions)`; `each(full, t)`: the path's own checks.  Returns the envs"""
    env_kw = env_kw or {}
    full = make(p, B_PATH, **keywords(channels), **env_kw)
    twins = {c: make(p, B_PATH, **keywords((c,)), **env_kw) for c in channels} if len(channels) > 1 else {}
    none = make(p, B_PATH, **env_kw)
    everyone = [full, none] + list(twins.values())
    check_counters(full, 'start', stepped=False)
    for t in range(steps):
        act = actions_at(t, full.device)
        for env in everyone:
            step(env, act)
        full.sync()
        check_channels(full, twins, channels, t)
        assert differing(state_of(full), state_of(none)) == [], t
        check_counters(full, t)
        if each is not None:
            each(full, t)
    return full, none, twins


def plugins_step(env, act):
    env._set_action(act)
    env._plugins_step()


def perceive_act_case(make, p, steps=AC.MAX_STEPS, modelled=(0, 3)):
    """perceive() then act() with the two channels the path admits: the rays are ready behind perceive() -- the pose has not moved
    yet, and the counter has not either, so they are the rays of step counter + 1 only once act() has run -- and age_map behind
    act().  Both against their models directly on the envs of `modelled`, and against twins"""
    full = make(p, B_PATH, seen_obs=True, scan_obs=True)
    twins = {'seen': make(p, B_PATH, seen_obs=True), 'scan': make(p, B_PATH, scan_obs=True)}
    none = make(p, B_PATH)
    cfg = full.cfg
    model = {e: [np.zeros((cfg.W, cfg.H), dtype=np.int32), 0] for e in modelled}
    for e in modelled:
        model[e][1] = check_seen_model(full, e, *model[e])
    kinds = np.zeros(4, dtype=np.int64)
    for t in range(steps):
        act = actions_at(t, full.device)
        before = {c: {k: v.clone() for k, v in records(full, c).items()} for c in ('seen', 'scan')}
        pose = full.state.drone.clone()
        for env in (full, none, *twins.values()):
            env.perceive()
        full.sync()
        assert differing(records(full, 'seen'), before['seen']) == [], t         # perceive() leaves the map alone ...
        assert torch.equal(raw(full.scan['pose']), raw(pose)), t                 # ... and casts the rays from the pose it found
        check_channels(full, twins, ('seen', 'scan'), (t, 'perceive'))
        for e in modelled:                         # ready behind this half: the model's rays for the pose in front of it
            check_scan_model(full, e)
        for env in (full, none, *twins.values()):
            env.act(act)
        full.sync()
        check_channels(full, twins, ('seen', 'scan'), (t, 'act'))
        assert differing(state_of(full), state_of(none)) == [], t
        check_counters(full, t)
        for e in modelled:
            kinds += np.bincount(check_scan_model(full, e), minlength=4)
            model[e][1] = check_seen_model(full, e, *model[e])
    return full, kinds


def closed_loop_case(make, p, steps=AC.MAX_STEPS, modelled=tuple(range(B_PATH))):
    """closed_loop(1) with scan_obs, the one channel it admits, finished envs frozen: against the model, against a _plugins_step
    twin under the same action and against the same launch without the channel"""
    full, staged, none = make(p, B_PATH, scan_obs=True), make(p, B_PATH, scan_obs=True), make(p, B_PATH)
    kinds = np.zeros(4, dtype=np.int64)
    for t in range(steps):
        act = actions_at(t, full.device)
        live = full.state.flags[:, A.F_DONE] == 0
        for env in (full, none):
            env._set_action(torch.where(live, act, env.state.action))
            env.closed_loop(1, freeze_done=True)
        staged._set_action(torch.where(live, act, staged.state.action))
        staged._plugins_step()
        full.sync()
        assert differing(records(full, 'scan'), records(staged, 'scan')) == [], t
        assert differing(state_of(full), state_of(none)) == [], t
        check_counters(full, t)
        for e in modelled:                         # (a finished env's snapshot moves on to the pose it ended in; its rays stay)
            if bool(live[e]):
                kinds += np.bincount(check_scan_model(full, e), minlength=4)
    return full, kinds


def oxford_case(make, p, steps=AC.MAX_STEPS, split=10):
    """policy_step() for `split` steps, then run_episodes() to the end, gaze='Oxford', all three channels against twins and none.
    The channel's seen_calls in front of a step are the Oxford stage's own seen_step behind it (the stage marks from the pose of
    before the step, and nothing later writes it), for the envs playing; a finished env stays frozen in all three channels.  Returns
    (envs compared with the Oxford stage, frozen env-steps checked)"""
    kw = dict(gaze='Oxford')
    full = make(p, B_PATH, **keywords(CHANNELS), **kw)
    twins = {c: make(p, B_PATH, **keywords((c,)), **kw) for c in CHANNELS}
    none = make(p, B_PATH, **kw)
    everyone = [full, none] + list(twins.values())
    compared = frozen = 0
    kept = {}
    for t in range(split):
        live = full.state.flags[:, A.F_DONE] == 0
        calls = full.seen_calls.clone()
        for env in everyone:
            env.policy_step()
        full.sync()
        assert torch.equal(calls[live], full.plugins.t['seen_step'][live]), t
        compared += int(live.sum())
        check_channels(full, twins, CHANNELS, t)
        assert differing(state_of(full), state_of(none)) == [], t
        check_counters(full, t)
        for e in range(B_PATH):
            if e in kept:
                check_kept(full, e, kept[e], t)
                frozen += 1
            elif bool(full.state.flags[e, A.F_DONE]):
                kept[e] = kept_of(full, e)
    for chunk in (3, 10, 10, steps - split - 23):
        ran = {env.run_episodes(max_steps=chunk, check_every=chunk + 1) for env in everyone}
        assert ran == {chunk}
        full.sync()
        check_channels(full, twins, CHANNELS, ('run_episodes', chunk))
        assert differing(state_of(full), state_of(none)) == [], chunk
        check_counters(full, chunk)
        for e in range(B_PATH):
            if e in kept:
                check_kept(full, e, kept[e], chunk)
                frozen += 1
            elif bool(full.state.flags[e, A.F_DONE]):
                kept[e] = kept_of(full, e)
    assert bool(full.state.flags[:, A.F_DONE].all())
    return compared, frozen


def reset_case(make, p, before=7, after=7):
    """reset(mask) on half of the envs in mid-episode, all three channels: the masked half is fresh, the other half untouched bit for
    bit, and the next steps of both halves equal the twins' and -- the scan and the seen map of one env of either half -- the models'.
    The masked envs are back at step 0 while their channels last held step `before`: after `before` more steps the counters are
    equal again, and a launch that compared them with what the old episode left would skip the step"""
    full = make(p, B_PATH, **keywords(CHANNELS))
    twins = {c: make(p, B_PATH, **keywords((c,))) for c in CHANNELS}
    none = make(p, B_PATH)
    everyone = [full, none] + list(twins.values())
    mask = torch.tensor([1, 0, 1, 0, 1, 0], dtype=torch.uint8)
    t = 0

    def steps(n):
        nonlocal t
        for _ in range(n):
            act = actions_at(t, full.device)
            for env in everyone:
                plugins_step(env, act)
            full.sync()
            check_channels(full, twins, CHANNELS, t)
            assert differing(state_of(full), state_of(none)) == [], t
            t += 1
    steps(before)
    assert not bool(full.state.flags[:, A.F_DONE].any())
    assert full.scan['last_step'].tolist() == [before] * B_PATH and full.seen['last_call'].tolist() == [before + 1] * B_PATH
    old = {c: {k: v.clone() for k, v in records(full, c).items()} for c in CHANNELS}
    for env in everyone:
        env.reset(mask)
    full.sync()
    for e in range(B_PATH):
        if mask[e]:
            check_fresh(full, e)
        else:
            for c in CHANNELS:
                assert differing(records(full, c, e), {k: v[e] for k, v in old[c].items()}) == [], (e, c)
    check_channels(full, twins, CHANNELS, 'reset')
    assert differing(state_of(full), state_of(none)) == []
    model = {}
    for e in (0, 1):                               # one env of either half: the seen model starts from what the env holds now
        model[e] = [full.seen_calls[e].cpu().numpy().copy(), int(full.seen['last_call'][e])]
    for k in range(after):
        steps(1)
        want = torch.where(mask.bool().to(full.device), k + 1, before + k + 1).to(torch.int32)
        assert torch.equal(full.state.counters[:, A.C_STEPS], want), k
        check_counters(full, ('after', k))
        for e in (0, 1):
            check_scan_model(full, e)
            model[e][1] = check_seen_model(full, e, *model[e])
    return full
