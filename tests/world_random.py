"""Random feasible worlds for the device world construction (include/d2d_worlds.h), shared by test_world_random_cpu.py (the
sequential host form) and test_gpu_device_worlds.py (the kernel).  A batch is 8 Params that agree on what vec_env.world_inputs
calls per-batch and differ in everything per-env; every comparison is array_equal against host_init.init_world.  The coverage
conditions (which carry sizes, how many regenerations, redraws, rejections the worlds go through) are computed from the
reference alone, with a `random.Random` that counts its calls: they are conditions on the inputs, not on the code under test.
This module holds no tests."""
import math
import random
import types

import numpy as np
import pytest

import world_cases as WC

SEED, COUNT, ENVS = 5, 60, 8         # the committed soak: 60 batches of 8 worlds, none left out
MAP_SIZES = ([480, 640], [250, 250], [330, 270], [210, 350], [640, 480], [1000, 800], [170, 510])
AGENT_NUMBERS = (0, 1, 2, 7, 10, 33, 63, 64, 65, 100, 130)
PILLAR_NUMBERS = (0, 0, 1, 3, 5, 8)
DRONE_RADII = (5, 10, 20)
STATIC_MAPS = ('maps/empty_map.npy', 'maps/random_map_0.npy', 'maps/obstacle_map.npy')
MAP_SCALES = (5, 10, 10, 20)
AGENT_RADII = (-1, 5, 7.5, 10, 12, 15, 20)
AGENT_SPEEDS = (20, 33.3, 40, 60)
MAX_AGENT_ATTEMPTS = 20000           # CountingRandom raises beyond: an infeasible draw fails instead of hanging


def _pick(rs, seq):
    return seq[int(rs.randint(len(seq)))]


def _r_top(agent_radius):
    """the largest radius uniform() can return for this setting"""
    return 15.0 if agent_radius == -1 else agent_radius + 2.0


def _feasible(map_size, agent_number, r_top):
    """discs of the largest radius any env can draw fill at most 30 % of the area the centres are drawn from"""
    return agent_number * math.pi * r_top ** 2 <= 0.30 * (map_size[0] - 40) * (map_size[1] - 40)


def _draw_batch(rs):
    """one batch: (per-batch keywords, list of per-env keywords, options), or None when it has to be drawn again"""
    size = list(_pick(rs, MAP_SIZES))
    W_px, H_px = size
    shared = dict(map_size=size, agent_number=_pick(rs, AGENT_NUMBERS), pillar_number=_pick(rs, PILLAR_NUMBERS),
                  drone_radius=_pick(rs, DRONE_RADII), static_map=STATIC_MAPS[0], map_scale=_pick(rs, MAP_SCALES),
                  var_cam=2 if rs.randint(2) else 0)
    n_tgt = int(rs.randint(1, 4))
    if size == [480, 640] and rs.randint(3):
        shared.update(static_map=STATIC_MAPS[int(rs.randint(3))], map_scale=10)
    opts = dict(grid_tile=16 if rs.uniform() < 0.4 else 0)
    # the envs draw their radius from the settings below a per-batch top: in half of the batches the largest one the map has room
    # for, which is where rejection sampling takes hundreds of attempts
    by_size = sorted(AGENT_RADII, key=_r_top)
    fits = [r for r in by_size if _feasible(size, shared['agent_number'], _r_top(r))]
    top = (fits[-1] if fits else None) if rs.randint(2) else _pick(rs, by_size)
    if top is None or top not in fits:
        return None
    radii = fits[:fits.index(top) + 1]
    envs = []
    for _ in range(ENVS):
        envs.append(dict(map_id=int(rs.randint(0, 2 ** 32, dtype=np.uint64)), agent_radius=_pick(rs, radii),
                         agent_max_speed=_pick(rs, AGENT_SPEEDS),
                         init_pos=[int(rs.randint(30, W_px - 29)), int(rs.randint(30, H_px - 29))],
                         target_list=[[int(rs.randint(20, W_px - 19)), int(rs.randint(20, H_px - 19))] for _ in range(n_tgt)]))
    assert _feasible(size, shared['agent_number'], max(_r_top(e['agent_radius']) for e in envs))
    return shared, envs, opts


def batches(seed, count):
    """yields `count` times (plist, opts): 8 Params (planner='NoMove') and dict(grid_tile=0 | 16)"""
    import drone2d_amd as pkg
    rs = np.random.RandomState(seed)
    for _ in range(count):
        drawn = None
        while drawn is None:
            drawn = _draw_batch(rs)
        shared, envs, opts = drawn
        yield [pkg.Params(planner='NoMove', **shared, **e) for e in envs], opts


class CountingRandom(random.Random):
    """random.Random that counts what host_init.init_world asks of it.  Overriding random AND getrandbits keeps _randbelow on
    getrandbits (Lib/random.py __init_subclass__), so the stream, and the world, are those of random.Random."""

    def __init__(self, seed):
        super().__init__(seed)
        self.n_random = self.n_bits = self.n_randint = 0

    def random(self):
        self.n_random += 1
        if self.n_random > 3 * MAX_AGENT_ATTEMPTS:
            raise RuntimeError(f'more than {MAX_AGENT_ATTEMPTS} agent attempts: the world is infeasible')
        return super().random()

    def getrandbits(self, k):
        self.n_bits += 1
        if self.n_bits > 6 * MAX_AGENT_ATTEMPTS:
            raise RuntimeError('the pillars cannot be placed: the world is infeasible')
        return super().getrandbits(k)

    def randint(self, a, b):
        self.n_randint += 1
        return super().randint(a, b)


def counted_world(p):
    """(host_init.init_world(p), counts) with CountingRandom in place of host_init._random for this one call.  counts:
    rounds (pillar candidates), redraws (_randbelow's rejected words), agent_attempts, pillar_words (words the pillars drew), and
    A = rounds + redraws + agent_attempts: the attempts in the sense of d2d_world_spec.max_attempts."""
    from drone2d_amd import host_init
    from drone2d_amd.params import with_defaults
    made = []

    def factory(seed):
        made.append(CountingRandom(seed))
        return made[-1]
    with pytest.MonkeyPatch.context() as m:
        m.setattr(host_init, '_random', types.SimpleNamespace(Random=factory))
        w = host_init.init_world(with_defaults(p))
    r, = made
    assert r.n_randint % 3 == 0 and r.n_random % 3 == 0
    c = dict(rounds=r.n_randint // 3, redraws=r.n_bits - r.n_randint, agent_attempts=r.n_random // 3, pillar_words=r.n_bits)
    c['A'] = c['rounds'] + c['redraws'] + c['agent_attempts']
    return w, c


def carry_sizes(pillar_words, agent_attempts):
    """Size of the carry at every regeneration of the agent phase, from the counts alone: the pillars leave
    (624 - pillar_words % 624) % 624 words of the key, a pass takes min(avail // 6, 64, left) attempts of six words, and a pass
    that finds fewer than six words moves them into the carry and regenerates."""
    avail, left, sizes = (624 - pillar_words % 624) % 624, agent_attempts, []
    while left > 0:
        if avail < 6:
            sizes.append(avail)
            avail += 624
        n = min(avail // 6, 64, left)
        avail -= 6 * n
        left -= n
    return sizes


_reference_cache = {}


def reference(seed=SEED, count=COUNT):
    """the batches of `seed` with what the reference makes of them, computed once: list of (plist, opts, expected, counts) --
    `expected` as world_cases.expected stacks it, `counts` one counted_world dict per env"""
    import drone2d_amd as pkg
    key = (seed, count)
    if key not in _reference_cache:
        out = []
        for plist, opts in batches(seed, count):
            ws, counts = zip(*(counted_world(p) for p in plist))
            out.append((plist, opts, WC.stack_worlds(pkg, list(ws), opts['grid_tile']), list(counts)))
        _reference_cache[key] = out
    return _reference_cache[key]


# ---------------------------------------------------------------------------------------- the cap boundary
CAP_CONFIGS = (dict(agent_number=10, agent_radius=15), dict(agent_number=60, agent_radius=15, pillar_number=5),
               dict(agent_number=100, agent_radius=15, pillar_number=3), dict(agent_number=1, pillar_number=8))
# one launch of 8 envs (map_id 0..7) capped at the median A of its envs; the second and third need more than 64 attempts, so
# their cap falls inside a pass or behind several
CAP_MIXED = (CAP_CONFIGS[0], CAP_CONFIGS[2], CAP_CONFIGS[1])
_cap_cache = {}


def cap_world(i, map_id):
    """(Params, expected of this one world, A) of CAP_CONFIGS[i] with `map_id`"""
    import drone2d_amd as pkg
    key = (i, map_id)
    if key not in _cap_cache:
        p = pkg.Params(planner='NoMove', map_id=map_id, **CAP_CONFIGS[i])
        w, c = counted_world(p)
        _cap_cache[key] = (p, w, c['A'])
    p, w, A = _cap_cache[key]
    return p, WC.stack_worlds(pkg, [w]), A


def cap_mixed(cfg):
    """8 envs of `cfg` and the median of their A as max_attempts: (plist, expected of all 8, A per env, cap)"""
    import drone2d_amd as pkg
    i = CAP_CONFIGS.index(cfg)
    ws = [cap_world(i, m) for m in range(8)]
    A = [w[2] for w in ws]
    cap = sorted(A)[3]
    assert min(A) <= cap < max(A), A                   # both kinds of env in the launch
    return [w[0] for w in ws], WC.stack_worlds(pkg, [_cap_cache[(i, m)][1] for m in range(8)]), A, cap


def env_slice(fields, sel):
    """the envs `sel` (index array or slice) of a dict of stacked fields"""
    return {k: (v if k == 'group' else np.asarray(v)[sel]) for k, v in fields.items()}
