"""Shared cases of the RVO tests: the recorded worlds (tests/golden/rvo_traces.npz) and seeded synthetic scenes with the Python
model's answer, computed once per process."""
import functools
import json
import os

import numpy as np

import rvo_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rvo_traces.npz')
SIX_LENGTH_SPEEDS = (31.98018040749264, 15.992981772452469)     # np.arange(0.02, v + 0.02, v / 5.0) has 6 elements


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(GOLDEN)


def world_names():
    return [str(n) for n in fixture()['names']]


def world(i):
    """the arrays of world i without their prefix"""
    d = fixture()
    pre = f'w{i}_'
    return {k[len(pre):]: d[k] for k in d.files if k.startswith(pre)}


def world_params(w):
    p = json.loads(str(w['params_json']))
    return dict(map_size=tuple(p['map_size']), scale=p['map_scale'], dt=p['dt'])


@functools.lru_cache(maxsize=None)
def world_model(i):
    """the model's replay of world i from its stored initial state -> (pos, vel, pref [T, N, 2], events)"""
    w = world(i)
    kw = world_params(w)
    pos, vel, pref = w['agent_pos'], w['agent_vel'], w['agent_pref']
    T = len(w['t_done'])
    out = [np.zeros((T,) + pos.shape) for _ in range(3)]
    events = {}
    for t in range(T):
        pos, vel, pref = M.step_world(pos, vel, pref, w['agent_radius'], w['obstacles'], events=events, **kw)
        out[0][t], out[1][t], out[2][t] = pos, vel, pref
    for a in out:
        a.setflags(write=False)
    return out[0], out[1], out[2], events


def with_speed(v, angle):
    return np.array([v * np.cos(angle), v * np.sin(angle)])


def scene(N, P, seed, kind='spread'):
    """One synthetic env -> dict(pos, vel, pref [N, 2], radius [N], pillars [P, 3] int32).
    spread: agents over the 500 x 500 map.  cluster: agents within a few radii of each other, so that most decisions find no
    suitable candidate.  Every scene with N >= 2 holds a pair closer than 2 * ROB_RAD; with P >= 1 agent 0 stands inside pillar 0's
    inflated radius; agent 0 has a 6-length speed; with N >= 3 agent 2 stands where its preferred velocity lies exactly on the
    apex of agent 1's cone (dif == 0 for the last candidate)."""
    rng = np.random.RandomState(seed)
    side = 500.0 if kind == 'spread' else 12.0 * max(2.0, np.sqrt(N))
    pos = rng.uniform(30, 30 + side, (N, 2))
    speed = rng.choice([4.0, 20.0, 30.0, 40.0], N)
    pref = np.stack([with_speed(s, a) for s, a in zip(speed, rng.uniform(0, 2 * np.pi, N))]) if N else np.zeros((0, 2))
    vel = pref * rng.uniform(0, 1, (N, 1)) + rng.uniform(-2, 2, (N, 2))
    vel[rng.rand(N) < 0.2] = 0.0
    radius = rng.uniform(8, 12, N)
    pillars = np.stack([rng.randint(60, 440, P), rng.randint(60, 440, P), rng.randint(5, 25, P)], axis=1).astype(np.int32).reshape(P, 3)
    if N >= 2:
        pos[1] = pos[0] + (radius[0] * 0.7, 3.0)
    if P >= 1:
        pillars[0, :2] = np.rint(pos[0]) + (4, -3)
    if N >= 1:
        v = SIX_LENGTH_SPEEDS[seed % 2]                # along an axis: the norm is the speed itself
        pref[0] = [(v, 0.0), (0.0, -v), (-v, 0.0), (0.0, v)][(seed // 2) % 4]
    if N >= 3:
        # apex of agent 1's cone as agent 2 sees it = p2 + 0.5 * (v1 + v2); the last candidate is pref2: dif = pref2 - 0.5 * (v1 + v2)
        vel[1] = (6.0, -2.0)
        vel[2] = (10.0, 4.0)
        pref[2] = (8.0, 1.0)
        pos[2] = (np.rint(pos[1][0]) - 25.0, np.rint(pos[1][1]) + 15.0)   # agent 1's cone then holds theta_dif = atan2(0, 0) = 0
    return dict(pos=pos, vel=vel, pref=pref, radius=radius, pillars=pillars)


# every N with every P; the model costs N * (N - 1 + P) * 161 atan2, so the large N take one kind per P
SCENES = [(N, P, kind) for N in (1, 2, 3) for P in (0, 1, 5) for kind in ('spread', 'cluster') if not (N == 1 and kind == 'cluster')] + \
         [(64, 0, 'cluster'), (64, 1, 'spread'), (64, 5, 'cluster'), (65, 0, 'spread'), (65, 1, 'cluster'), (65, 5, 'spread')]


@functools.lru_cache(maxsize=None)
def scene_model(N, P, seed, kind='spread'):
    """-> (scene, vel_out, pos_out, pref_out, events) of one model step"""
    s = scene(N, P, seed, kind)
    events = {}
    pos, vel, pref = M.step_world(s['pos'], s['vel'], s['pref'], s['radius'], s['pillars'], events=events)
    for a in (pos, vel, pref):
        a.setflags(write=False)
    return s, vel, pos, pref, events
