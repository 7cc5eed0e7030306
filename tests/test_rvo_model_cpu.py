"""tests/rvo_model.py (the Python model of include/d2d_rvo.h) against the recorded reference, tests/golden/rvo_traces.npz: every
stored step of every world from the stored initial state, bit for bit; the model's np.arange replay against numpy; the parallel
argmin rule against Python's min.

What the recorded worlds reach is asserted in test_the_fixture_holds_what_it_is_meant_to_hold.  They do reach a clamped `dist`
(overlapping agents: 2 cones in the pillar world, 1464 among the obstacle map's packed cell agents) and a candidate exactly on an apex
(321 times in the obstacle-map world: two cell agents of one group share their velocity, so the apex pA + 0.5 * (v + v) is pA + pref
and the last candidate has dif == 0, which divides a positive dist_tg by 0: an infinity).  They do not reach a 6-length candidate
radius list, and no finite input reaches a NaN key (0 / 0 needs dist_tg == 0, which needs a clamped cone, and the 3.14 of in_between
keeps theta_dif = atan2(0, 0) = 0 out of a cone that is pi wide); the synthetic scenes of rvo_cases.py cover the 6-length list against
the model only (test_rvo_host_build.py, test_gpu_rvo.py), and the NaN rule is held to Python's min here, on lists."""
import math

import numpy as np
import pytest

import host_build
import rvo_cases as RC
import rvo_model as M

needs_fma = host_build.needs_fma('numpy takes non-FMA norm / matmul variants on this CPU')


@needs_fma
@pytest.mark.parametrize('i', range(len(RC.world_names())), ids=RC.world_names())
def test_model_reproduces_every_recorded_step(i):
    w = RC.world(i)
    pos, vel, pref, _ = RC.world_model(i)
    assert len(w['t_done']) <= 40 and not w['t_done'].any()
    for t in range(len(w['t_done'])):
        assert M.bits_equal(vel[t], w['t_agent_vel'][t]), (t, 'vel')
        assert M.bits_equal(pos[t], w['t_agent_pos'][t]), (t, 'pos')
        assert M.bits_equal(pref[t], w['t_agent_pref'][t]), (t, 'pref')


@needs_fma
def test_the_fixture_holds_what_it_is_meant_to_hold():
    names = RC.world_names()
    assert names == ['readme', 'pillars300', 'n30', 'obstacle_map', 'one_agent', 'one_agent_pillars']
    ev = {n: RC.world_model(i)[3] for i, n in enumerate(names)}
    total = lambda key: sum(e.get(key, 0) for e in ev.values())   # noqa: E731
    assert total(('kind', M.PREF)) > 0                 # pref taken unchanged
    assert total(('kind', M.GRID)) > 0                 # a grid candidate chosen among suitable ones
    assert ev['pillars300'].get(('kind', M.NO_SUITABLE), 0) > 0 or ev['n30'].get(('kind', M.NO_SUITABLE), 0) > 0
    assert ev['n30'].get('rotated', 0) > 0             # a stuck agent's rotation
    assert total('flipped') > 0                        # a boundary flip
    assert ev['one_agent'] == {('kind', M.PREF): 40, ('C', 161): 40, 'rotated': 0, 'flipped': ev['one_agent']['flipped'], 'in_pillar_cone': 0,
                               'on_apex': 0, 'nan_keys': 0, 'clamped': 0}
    assert ev['pillars300']['clamped'] > 0 and ev['obstacle_map']['clamped'] > 1000      # a clamped dist: overlapping agents
    assert ev['obstacle_map']['on_apex'] > 0 and total('nan_keys') == 0                  # dif == 0 gives an infinity, never a NaN
    assert total(('C', 193)) == 0                                                        # no 6-length radius list
    # a pillar cone that makes a candidate unsuitable; for the lone agent among three pillars every cone is a pillar's
    assert ev['one_agent_pillars']['in_pillar_cone'] > 0 and ev['pillars300']['in_pillar_cone'] > 0
    w = RC.world(names.index('obstacle_map'))
    assert len(w['agent_radius']) == 24 and w['agent_radius'][0] != 5 and (w['agent_radius'][10:] == 5).all()
    assert M.bits_equal(w['agent_vel'][10:], w['agent_pref'][10:]) and not w['agent_vel'][:10].any()
    d = RC.fixture()
    assert float(d['w0_ref_seconds_per_step']) > 0 and 'w0_full_t_gt' in d.files and 'w1_full_t_obs_local' in d.files
    assert len(d['ep_actions']) == int(round(d['ep_row'][0] / 0.1))


def test_arange_replay_equals_numpy():
    rng = np.random.RandomState(7)
    speeds = np.concatenate([rng.uniform(0.5, 80, 60000), rng.choice([4, 10, 20, 30, 40, 60], 20000) * (1 + rng.uniform(-4, 4, 20000) * 2.0 ** -52),
                             np.exp(rng.uniform(-20, 8, 20000)), RC.SIX_LENGTH_SPEEDS])
    lengths = set()
    for v in speeds:
        want = np.arange(0.02, v + 0.02, v / 5.0)
        got = M.arange_replay(v)
        lengths.add(len(got))
        assert len(got) == len(want) and M.bits_equal(got, want), v
    assert {5, 6} <= lengths
    for v in RC.SIX_LENGTH_SPEEDS:
        assert len(M.arange_replay(v)) == 6
    assert np.array_equal(np.array(M.THETAS), np.arange(0, 2 * 3.14, 0.2)) and len(M.THETAS) == 32


def test_parallel_argmin_equals_pythons_min():
    nan = math.nan
    rng = np.random.RandomState(3)
    lists = [[1.0], [nan], [nan, 1.0, 0.5], [1.0, nan, 0.5], [2.0, 1.0, nan, 1.0], [3.0, 3.0, 3.0], [math.inf, math.inf], [math.inf, nan, 5.0],
             [nan] * 5, [1.0] + [nan] * 200]
    for n in (2, 63, 64, 65, 161, 193):
        for _ in range(20):
            k = rng.choice([0.25, 0.5, 1.0, 2.0, math.inf], n).tolist()     # many ties
            lists.append(k)
            k2 = list(k)
            for j in rng.randint(1, n, 3):
                k2[j] = nan                                                  # NaNs later than position 0
            lists.append(k2)
            lists.append([nan] + k[1:])                                      # a NaN at position 0
    for keys in lists:
        want = min(range(len(keys)), key=keys.__getitem__)
        assert M.seq_min(keys) == want, keys
        assert M.parallel_argmin(keys) == want, keys
