"""The plugin surface against what the reference's own classes and env computed (fixtures written by
tests/golden/make_golden.py from the reference): the package's host gaze policies against yaw_planner.LookAhead /
LookGoal on random observations, and the facade's measurement-noise path against the reference env with var_cam = 2."""
import json
import types

import numpy as np

from replay import load


def test_host_gaze_policies_equal_the_reference_classes(pkg):
    """gaze.LookAhead / gaze.LookGoal against yaw_planner.LookAhead / LookGoal on the same observations (golden
    `host_gaze_values`, make_golden.py gaze_values: the same seed and order of draws): same value, bit for bit, over random
    states incl. a drone at rest, the +-180 degree wrap, yaw outside [0, 360), empty trajectories and trajectories through
    explored / unexplored / out-of-map cells."""
    from drone2d_amd import gaze
    fx = load('host_gaze_values')
    want = fx['values']
    assert [str(n) for n in fx['names']] == ['LookAhead', 'LookGoal'] and want.shape == (4000, 2)
    P = types.SimpleNamespace(dt=0.1, drone_max_yaw_speed=80)
    rng = np.random.RandomState(11)

    class Map:
        def __init__(self, g):
            self.g = g

        def get_grid(self, x, y):
            if x >= 500 or x < 0 or y >= 500 or y < 0:
                return 1
            return self.g[int(x // 10), int(y // 10)]

    class Traj:
        def __init__(self, pts):
            self.positions = pts

        def __len__(self):
            return len(self.positions)

    n = 0
    for case in range(4000):
        vel = rng.uniform(-40, 40, 2) * rng.choice([0, 1, 1, 1], 2)
        if case % 7 == 0:
            vel = np.round(vel)
        yaw = rng.uniform(-400, 800) if case % 3 else float(rng.randint(0, 360))
        drone = types.SimpleNamespace(velocity=vel, yaw=yaw, x=float(rng.randint(0, 500)), y=float(rng.randint(0, 500)),
                                      map=Map(rng.choice([0, 1, 2], (50, 50), p=[0.2, 0.1, 0.7]).astype(np.uint8)))
        pts = [np.round(rng.uniform(-20, 520, 2)) for _ in range(rng.randint(0, 12))]
        if case % 11 == 0 and pts:
            pts[-1] = np.array([drone.x, drone.y])                     # atan2(-0.0, 0.0)
        obs = {'drone': drone, 'trajectory': Traj(pts), 'target': np.array([250., 250.])}
        for j, name in enumerate(('LookAhead', 'LookGoal')):
            a, b = getattr(gaze, name)(P).plan(obs), want[case, j]
            assert np.array_equal(np.float64(a), b) and np.signbit(a) == np.signbit(b), (name, case, a, b)
            n += a != 0
    assert n > 3000


def test_measurement_noise_through_the_facade(pkg, oracle):
    """var_cam != 0: the reference draws np.random.randn(2) per agent the rays hit, in agent order, from the global stream it
    seeded with map_id (utils.py:603-605, envs/drone_v2.py:80).  The facade keeps that stream, splits the step after the raycast
    and feeds the draws to the tracker stage: tracker means / covariances and active bits follow the reference env's (golden
    `facade_noise_var_cam2`, make_golden.py facade_noise: the drone put next to an agent every tenth step, random actions)."""
    from drone2d_amd import env as envmod
    fx = load('facade_noise_var_cam2')
    kw = json.loads(str(fx['cfg']))
    assert kw['var_cam'] == 2
    mine = envmod.Drone2DEnv2(pkg.Params(debug=True, **kw), backend=oracle)
    seen = 0
    for t in range(len(fx['action'])):
        x, y = (int(v) for v in fx['tele'][t])
        if x >= 0:                            # next to an agent, looking at it: rays hit, trackers start and update
            mine.drone.x, mine.drone.y = x, y
        mine.step(float(fx['action'][t]))
        for k, active in enumerate(fx['active'][t]):
            assert bool(active) == mine.drone.trackers[k].active, (t, k)
            if active:
                seen += 1
                assert np.allclose(fx['mu'][t, k], mine.drone.trackers[k].mu_upds[-1][:, 0], rtol=0, atol=1e-6), (t, k)
                assert np.allclose(fx['sigma'][t, k], mine.drone.trackers[k].Sigma_upds[-1], rtol=0, atol=1e-6), (t, k)
        assert np.array_equal(fx['gt'][t], mine.map_gt.grid_map) and fx['tracked'][t] == mine.tracked_agent
    assert seen > 50
