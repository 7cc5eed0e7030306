#!/usr/bin/env python3
"""Recorder of tests/golden/vo_feasibility.npz: the reference's own env_metrics(index) of script/difficulty_calculator/
vo_calculator.py and density_calculator.py on three settings.

Both scripts run their whole sweep when they are imported, so they are neither imported nor restated here: their source is read
at run time, only its import statements and function definitions are kept (ast) and executed in a namespace whose `np.mean` also
records its argument -- the 256 per-position rates that env_metrics averages.  What is stored is data: per setting the index, the
agents' initial position / preferred velocity / radius, the rates, the returned mean, the density script's value, and the seconds
each call took on the recording machine.  Runs only where the reference is present (like make_golden.py, whose stubs it reuses).

Usage:  python tests/golden/make_vo_golden.py
"""
import ast
import json
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G   # noqa: E402  (installs the gym / pygame / cvxpy stubs, enters the reference's directory)

SETTINGS = [(10, 5, 20, 0), (20, 10, 40, 1), (30, 15, 60, 7)]     # (agent_number, agent_size, agent_speed, map_id)
SCRIPTS = os.path.join(G.REF, 'script', 'difficulty_calculator')


def reference_functions(script, made):
    """The import statements and function definitions of `script`, executed.  Returns (namespace, the list np.mean's arguments are
    appended to); every env the functions gym.make() is appended to `made`."""
    import gym
    from envs.drone_v2 import Drone2DEnv2
    sys.modules.setdefault('main', types.ModuleType('main'))      # density_calculator.py imports the experiment driver for nothing

    def make(name, params):
        if name == 'gym-metric-v1':
            from envs.metric_env import MetricEnv
            env = MetricEnv(params)
        else:
            env = Drone2DEnv2(params)
        made.append(env)
        return env
    gym.make = make
    tree = ast.parse(open(os.path.join(SCRIPTS, script)).read())
    tree.body = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom, ast.FunctionDef))]
    ns = {'__name__': 'reference_' + script[:-3]}
    exec(compile(tree, script, 'exec'), ns)
    seen = []

    class Numpy:
        def __getattr__(self, name):
            return getattr(np, name)

        @staticmethod
        def mean(a, *args, **kw):
            seen.append(list(a))
            return np.mean(a, *args, **kw)
    ns['np'] = Numpy()
    return ns, seen


def main():
    import contextlib
    import io
    d = {'n': np.array(len(SETTINGS))}
    made = []
    vo, seen = reference_functions('vo_calculator.py', made)
    den, _ = reference_functions('density_calculator.py', made)
    for i, (n, size, speed, map_id) in enumerate(SETTINGS):
        index = {'motion_profile': 'CVM', 'pillar_number': 0, 'agent_number': n, 'agent_speed': speed, 'agent_size': size, 'map_id': map_id}
        del made[:], seen[:]
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            mean = vo['env_metrics'](index)
        dt = time.perf_counter() - t0
        assert len(made) == 1 and seen and all(s == seen[0] for s in seen)     # (the script prints the mean, then returns it)
        ag = made[0].agents
        rates = seen[0]
        d[f's{i}_index'] = np.array(json.dumps(index))
        d[f's{i}_agent_pos'] = np.array([a.position for a in ag], dtype=np.float64).reshape(len(ag), 2)
        d[f's{i}_agent_pref'] = np.array([a.pref_velocity for a in ag], dtype=np.float64).reshape(len(ag), 2)
        d[f's{i}_agent_radius'] = np.array([a.radius for a in ag], dtype=np.float64)
        d[f's{i}_rates'] = np.array(rates, dtype=np.float64)
        d[f's{i}_collided'] = np.array([isinstance(r, int) for r in rates])     # the script appends the int 0 for those
        d[f's{i}_mean'] = np.array(mean, dtype=np.float64)
        d[f's{i}_ref_seconds'] = np.array(dt)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            d[f's{i}_density'] = np.array(den['env_metrics'](index), dtype=np.float64)
        d[f's{i}_density_ref_seconds'] = np.array(time.perf_counter() - t0)
        print(index, 'mean', float(mean), 'collided', int(d[f's{i}_collided'].sum()), 'zero rates', int((d[f's{i}_rates'] == 0).sum()),
              f'{dt:.1f} s; density', float(d[f's{i}_density']))
    G.save('vo_feasibility', d)


if __name__ == '__main__':
    main()
