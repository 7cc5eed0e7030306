"""The recorded swept maps (tests/golden/swept_episodes.npz, written by tests/golden/make_swept_golden.py) and the comparisons
tests/test_swept_obs_cpu.py (the model backend of tests/swept_backend.py) and tests/test_gpu_swept_obs.py (the HIP library) share.
Test infrastructure."""
import functools
import json
import os

import numpy as np
import torch

from drone2d_amd import _abi as A

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'swept_episodes.npz')
EPISODES = 4


@functools.lru_cache(maxsize=None)
def episode(i):
    z = np.load(PATH)
    pre = f'e{i}_'
    d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    d['cfg'] = json.loads(str(d['cfg']))
    return d


def params_of(pkg, ep, **kw):
    return pkg.Params(**dict(dict(planner='Primitive'), **dict(ep['cfg'], **kw)))


def coverage():
    """(truncated maps, empty-trajectory steps, longest trajectory, steps whose crop lost marked cells) of the stored set"""
    eps = [episode(i) for i in range(EPISODES)]
    total = lambda a: a.reshape(len(a), -1).astype(np.int64).sum(1)     # noqa: E731
    return (sum(int((d['m'] < d['n']).sum()) for d in eps), sum(int((d['n'] == 0).sum()) for d in eps),
            max(int(d['n'].max()) for d in eps), sum(int((total(d['crop']) != total(d['map'])).sum()) for d in eps))


def replay(env, ep):
    """the episode's recorded actions through env._plugins_step, one env: map, count and crop of every step equal the reference's"""
    T = len(ep['n'])
    act = torch.zeros(1, dtype=torch.float64)
    for t in range(T):
        assert not bool(env.state.flags[0, A.F_DONE]), t
        act[0] = float(ep['action'][t])
        env._set_action(act)
        env._plugins_step()
        obs = env._result()[0]
        env.sync()
        assert int(env.swept_count[0]) == int(ep['m'][t]), (t, int(env.swept_count[0]), int(ep['m'][t]), int(ep['n'][t]))
        assert np.array_equal(env.swept_map[0].cpu().numpy(), ep['map'][t]), t
        assert obs['swep_map'].shape == (1, 1, env.cfg.L, env.cfg.L) and obs['swep_map'].dtype == torch.uint8
        assert np.array_equal(obs['swep_map'][0, 0].cpu().numpy(), ep['crop'][t]), t
    assert bool(env.state.flags[0, A.F_DONE])
    return T
