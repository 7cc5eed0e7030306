#!/usr/bin/env python3
"""Recorder of tests/golden/difficulty_tables.npz: the reference's own env_metrics(index) of script/difficulty_calculator/
traversibility_calculator.py and survivability_calculator.py on five settings.

Like make_vo_golden.py (whose reference_functions it reuses) it neither imports nor restates the scripts: their import statements
and function definitions are executed from their source at run time.  The intermediates are taken by wrapping, not by restating:
`np.mean` inside demos.traversibility records the eight distances of every start, `traversibility` inside envs.metric_env records
the grid it is given and the value it returns, the env's reset() records the agents it has just placed, and the script's own
np.mean records survive_times.  What is stored is data: per setting the index; for the traversability world the initial agents,
the ground-truth grid at reset, the eight distances and the value of each of the 81 starts and the metric; for the survival-fit
world the initial agents, survive_times (8 x 8), its mean and the agents after the last step; and the seconds each call took on the
recording machine.  Runs only where the reference is present.

Usage:  python tests/golden/make_difficulty_golden.py
"""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G   # noqa: E402  (installs the gym / pygame / cvxpy stubs, enters the reference's directory)
from make_vo_golden import reference_functions   # noqa: E402

# (agent_number, agent_size, agent_speed, map_id): the three of vo_feasibility.npz, and two of metrics_fit.csv's own grid
SETTINGS = [(10, 5, 20, 0), (20, 10, 40, 1), (30, 15, 60, 7), (28, 14, 55, 0), (12, 6, 25, 0)]


def agents_of(env):
    """[6, N]: position, pref_velocity, radius, radius ** 2 (the layout of the package's state)"""
    ag = env.agents
    pos = np.array([a.position for a in ag], dtype=np.float64).reshape(len(ag), 2)
    pref = np.array([a.pref_velocity for a in ag], dtype=np.float64).reshape(len(ag), 2)
    r = np.array([a.radius for a in ag], dtype=np.float64)
    return np.stack([pos[:, 0], pos[:, 1], pref[:, 0], pref[:, 1], r, r ** 2])


def main():
    with contextlib.redirect_stdout(io.StringIO()):
        import demos.traversibility as DT
        import envs.metric_env as ME
        from envs.drone_v2 import Drone2DEnv2
    made, lists, calls, resets = [], [], [], []

    class Numpy:
        def __getattr__(self, name):
            return getattr(np, name)

        @staticmethod
        def mean(a, *args, **kw):
            lists.append(list(a))
            return np.mean(a, *args, **kw)
    DT.np = Numpy()
    inner = ME.traversibility

    def traversibility(arr, start):
        n = len(lists)
        value = inner(arr, start)
        calls.append((np.array(arr).copy(), tuple(start), lists[n] if len(lists) > n else None, value))
        return value
    ME.traversibility = traversibility
    for cls in (ME.MetricEnv, Drone2DEnv2):
        def reset(self, _reset=cls.reset):
            out = _reset(self)
            resets.append(agents_of(self))
            return out
        cls.reset = reset

    trav, _ = reference_functions('traversibility_calculator.py', made)
    fit, seen = reference_functions('survivability_calculator.py', made)
    d = {'n': np.array(len(SETTINGS))}
    for i, (n, size, speed, map_id) in enumerate(SETTINGS):
        index = {'motion_profile': 'CVM', 'pillar_number': 0, 'agent_number': n, 'agent_speed': speed, 'agent_size': size, 'map_id': map_id}
        d[f's{i}_index'] = np.array(json.dumps(index))
        del made[:], lists[:], calls[:], resets[:]
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            metric = trav['env_metrics'](index)
        dt = time.perf_counter() - t0
        assert len(made) == 1 and len(resets) == 1 and len(calls) == 81 and all((c[0] == calls[0][0]).all() for c in calls)
        assert [c[1] for c in calls] == [(x, y) for x in range(5, 50, 5) for y in range(5, 50, 5)]
        dist = np.full((81, 8), -1.0)
        for k, (_, _, eight, value) in enumerate(calls):
            assert (eight is None) == (isinstance(value, int) and value == 0)
            if eight is not None:
                dist[k] = eight
        d[f's{i}_trav_agents'] = resets[0]
        d[f's{i}_gt'] = calls[0][0].astype(np.uint8)
        assert (d[f's{i}_gt'] == calls[0][0]).all()
        d[f's{i}_distances'] = dist                                   # -1: the start cell is occupied (the function returns 0)
        d[f's{i}_values'] = np.array([c[3] for c in calls], dtype=np.float64)
        d[f's{i}_traversibility'] = np.array(metric, dtype=np.float64)
        d[f's{i}_trav_ref_seconds'] = np.array(dt)
        occupied = int((dist[:, 0] < 0).sum())

        del made[:], seen[:], resets[:]
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            mean = fit['env_metrics'](index)
        dt = time.perf_counter() - t0
        assert len(made) == 1 and len(resets) == 1 and len(seen) == 2       # (the script prints the mean, then returns it)
        times = np.array(seen[0], dtype=np.float64)
        assert times.shape == (8, 8)
        d[f's{i}_fit_agents'] = resets[0]
        d[f's{i}_survive_times'] = times
        d[f's{i}_fit'] = np.array(mean, dtype=np.float64)
        d[f's{i}_fit_agents_end'] = agents_of(made[0])
        d[f's{i}_fit_ref_seconds'] = np.array(dt)
        print((n, size, speed, map_id), 'traversibility', repr(float(metric)), f'({occupied} occupied starts, {d[f"s{i}_trav_ref_seconds"]:.2f} s)',
              'fit', repr(float(mean)), f'({int((times >= 11.9).sum())} positions never hit, {dt:.2f} s)')
    G.save('difficulty_tables', d)


if __name__ == '__main__':
    main()
