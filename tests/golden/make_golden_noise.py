#!/usr/bin/env python3
"""Golden episodes with measurement noise: runs the REAL reference (imported through make_golden.py's stubs) with var_cam = 2 --
every agent the rays hit gets sigma * np.random.randn(2) from the global numpy stream the env seeded with map_id
(utils.py:603-605) -- and stores arrays only: the traces of make_golden.run_trace (every input and output of every step of the
reference's own closed loop) as noise_<name>.npz, and the CSV rows of the same settings driven like Experiment.run as
noise_rows.npz, next to this script.  Oxford + Primitive (twice), LookAhead + Primitive and NoControl + NoMove on the small
default map.

Runs only where the reference is present (like make_golden.py).

Usage:  python tests/golden/make_golden_noise.py
"""
import json
import warnings

import numpy as np

import make_golden as MG

BASE = dict(var_cam=2, agent_max_speed=20, agent_radius=15, drone_max_speed=40)
CASES = [
    ('oxford_primitive_map1', 'Oxford', dict(BASE, gaze_method='Oxford', planner='Primitive', agent_number=10, map_id=1)),
    ('oxford_primitive_map4', 'Oxford', dict(BASE, gaze_method='Oxford', planner='Primitive', agent_number=20, agent_radius=10,
                                             agent_max_speed=40, map_id=4)),
    ('lookahead_primitive_map2', 'LookAhead', dict(BASE, gaze_method='LookAhead', planner='Primitive', agent_number=20,
                                                   agent_radius=10, agent_max_speed=40, map_id=2)),
    ('nocontrol_nomove_map3', 'NoControl', dict(BASE, gaze_method='NoControl', planner='NoMove', agent_number=20,
                                                agent_max_speed=40, max_flight_time=12, map_id=3)),
]
MAX_STEPS = 400


def main():
    warnings.simplefilter('ignore')
    rows = {'n': np.array(len(CASES)), 'names': np.array([n for n, _, _ in CASES])}
    for i, (name, policy, kw) in enumerate(CASES):
        tr = MG.run_trace(MG.make_params(**kw), MAX_STEPS, policy=policy)
        tr['cfg'] = np.array(json.dumps(kw))
        hits = tr['t_hit'].sum(axis=1)
        print(name, len(tr['t_action']), 'steps, done', bool(tr['t_done'][-1]), '; agents in view per step: max', int(hits.max()),
              'total', int(hits.sum()), '; steps with none', int((hits == 0).sum()))
        MG.save('noise_' + name, tr)
        rows[f'r{i}_cfg'] = np.array(json.dumps(kw))
        # (Experiment.__init__ widens the view to 360 degrees under NoControl, experiment.py:28-29: the row is the sweep's)
        row_kw = dict(kw, drone_view_range=360) if policy == 'NoControl' else kw
        rows[f'r{i}_row'] = np.array(MG.experiment_row(MG.make_params(**row_kw), policy), dtype=np.float64)
        print('   row', rows[f'r{i}_row'])
    MG.save('noise_rows', rows)


if __name__ == '__main__':
    main()
