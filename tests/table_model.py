"""Episode tables without a GPU (include/d2d_worlds_table.h; VecDrone2DEnv.stream_episodes(episodes=...)): d2d_stream_assign_table
restated as a loop in slot order, the CPU stream backends of tests/stream_backend.py with that assignment and with a world build that
reads each slot's own env_par / env_tgt row (start, targets, agent speed, D2D_WE_REDRAW), and the fixture of the reference's validation
episodes (tests/golden/validation_episodes.npz).  Test infrastructure: the product package never imports this."""
import copy
import functools
import json
import os

import numpy as np

import stream_backend as SB
import stream_model as SM
from drone2d_amd import _abi as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'validation_episodes.npz')


def assign_table(flags, slot_episode, map_id, env_par, env_tgt, refill, counts, ep_map_id, ep_par, ep_tgt):
    """d2d_stream_assign_table as a loop in slot order: slot_episode, map_id (uint32), env_par, env_tgt, refill and counts =
    [cursor, finished] in place.  A slot that is done and not retired takes the episode at the cursor and copies its row, or retires
    once the cursor stands at M; every other slot gets refill 0 and nothing else"""
    M = len(ep_map_id)
    cursor, finished = int(counts[0]), int(counts[1])
    for e in range(len(slot_episode)):
        refill[e] = 0
        if not (flags[e, A.F_DONE] != 0 and slot_episode[e] >= 0):
            continue
        finished += 1
        if cursor >= M:
            slot_episode[e] = -1
            continue
        slot_episode[e], map_id[e], env_par[e], env_tgt[e], refill[e] = cursor, ep_map_id[cursor], ep_par[cursor], ep_tgt[cursor], 1
        cursor += 1
    counts[0], counts[1] = cursor, finished


class _Table(SB._Stream):
    supports_episode_table = True

    def _build(self, spec, st, slots, flags):
        from drone2d_amd import host_init
        v = SM.world_views(spec, st)
        par = SM.at(spec.env_par, (spec.B, A.WORLDS_ENV_F), np.float64)
        tgt = SM.at(spec.env_tgt, (spec.B, spec.T, 2), np.float64)
        for e in slots:
            p = copy.copy(self.params)
            p.map_id = int(v['map_id'][e])
            p.init_position = [par[e, A.WE_X0], par[e, A.WE_Y0]]
            p.target_list = [list(t) for t in tgt[e, :int(par[e, A.WE_NTGT])]]
            p.agent_max_speed = par[e, A.WE_SPEED]
            SM.load_world(v, e, host_init.init_world(p, redraw=par[e, A.WE_REDRAW] != 0), spec.grid_tile, flags)

    def stream_assign_table(self, flags, ep_map_id, ep_par, ep_tgt, slot_episode, map_id, env_par, env_tgt, refill, counts):
        assign_table(flags.numpy(), slot_episode.numpy(), map_id.numpy().view(np.uint32), env_par.numpy(), env_tgt.numpy(), refill.numpy(),
                     counts.numpy(), ep_map_id.numpy().view(np.uint32), ep_par.numpy(), ep_tgt.numpy())


class TablePrimitiveBackend(_Table, SB.SteppedOracleBackend):
    name = 'oracle+rvo_host+live+stream+table'


class TableJerkBackend(_Table, SB.LiveJerkBackend):
    name = 'oracle+jerk_host+gaze_host+rvo_host+live+stream+table'


def backend_for_params(params):
    return (TableJerkBackend if params.planner == 'Jerk_Primitive' else TablePrimitiveBackend)().of(params)


def table_stream_of(params, episodes, slots, **kw):
    """runner.EpisodeStream(params, episodes=...) on a fresh table backend, attached"""
    from drone2d_amd import runner
    backend = backend_for_params(params)
    xs = runner.EpisodeStream(params, episodes=episodes, slots=slots, device='cpu', backend=backend, **kw)
    backend.attach(xs.env)
    return xs


def batch_of_worlds(params, plist, redraw, jerk_tie=None, backend=None):
    """ONE batch of the worlds of `plist`, host-built with build_worlds_of(..., redraw=...), with the cell's batch loop on `backend`
    (default: the cell's usual CPU backend); returns the env after every episode has ended"""
    from drone2d_amd import runner, vec_env
    from drone2d_amd.params import with_defaults
    jerk = params.planner == 'Jerk_Primitive'
    cpu = backend is None
    if cpu:
        backend = (SB.LiveJerkBackend if jerk else SB.SteppedOracleBackend)()
    if jerk or params.motion_profile == 'RVO':
        p = runner.SteppedExperimentBatch.accepted(params, backend)
    else:
        p = runner.ExperimentBatch.accepted(params, backend)[0]
    worlds = vec_env.build_worlds_of([with_defaults(q) for q in plist], redraw=redraw)
    env = vec_env.VecDrone2DEnv(p, len(plist), device='cpu' if cpu else backend.device, backend=backend, planner=p.planner, worlds=worlds,
                                device_plugins=True, gaze=p.gaze_method, jerk_tie=jerk_tie if jerk else None)
    if cpu:
        backend.attach(env)
    steps = int(np.ceil(p.max_flight_time / p.dt)) + 1
    if jerk or p.motion_profile == 'RVO':
        env.run_episodes(steps)
    else:
        env.closed_loop(steps, freeze_done=True)
    env.sync()
    return env


def rows_of_worlds(params, plist, redraw, agent_speed=None, jerk_tie=None, backend=None):
    from drone2d_amd import runner
    from drone2d_amd.params import with_defaults
    rec = runner.batch_records(batch_of_worlds(params, plist, redraw, jerk_tie, backend))
    return [runner.study_row(with_defaults(q), rec[k], agent_speed) for k, q in enumerate(plist)]


# ------------------------------------------------------------------------------------------------------ the fixture
@functools.lru_cache(maxsize=None)
def golden():
    d = np.load(GOLDEN)
    eps = []
    for i in range(int(d['n'])):
        e = {k[len(f'e{i}_'):]: d[k] for k in d.files if k.startswith(f'e{i}_')}
        e['cfg'] = json.loads(str(e['cfg']))
        eps.append(e)
    return eps, (d['tie_perm'], d['tie_eq'])


def golden_params(pkg, cfg):
    """the Params the script holds when it makes the episode's env"""
    planner, gaze = {'speed': ('Primitive', 'Oxford'), 'size': ('Jerk_Primitive', 'NoControl')}[cfg['form']]
    return pkg.Params(debug=False, map_id=cfg['map_id'], agent_number=cfg['agent_number'], agent_radius=cfg['agent_radius'],
                      agent_max_speed=cfg['agent_max_speed'], drone_max_speed=cfg['drone_max_speed'], static_map=cfg['static_map'],
                      max_flight_time=cfg['max_flight_time'], planner=planner, gaze_method=gaze, init_pos=tuple(cfg['start']),
                      target_list=[tuple(cfg['target'])])


def golden_cells(pkg):
    """the fixture's episodes grouped into stream cells: [(indices, list of Params, redraw, agent_speed)], every Params of a group
    equal in everything but map_id, start and target"""
    eps, _ = golden()
    groups = {}
    for i, e in enumerate(eps):
        c = e['cfg']
        key = (c['form'], c['agent_number'], c['agent_radius'], c['agent_max_speed'], c['drone_max_speed'], c['static_map'])
        groups.setdefault(key, []).append(i)
    return [(idx, [golden_params(pkg, eps[i]['cfg']) for i in idx], key[0] == 'speed', -1 if key[0] == 'speed' else None)
            for key, idx in groups.items()]


def row_numbers(row):
    """the ten numbers of a CSV row that the fixture records (columns 12 ..)"""
    return np.array([float(x) for x in row[12:]], dtype=np.float64)


def same_numbers(row, want):
    """Every number exact, NaN where NaN, but the mean tracked time.  There the script sums len(ts) * 0.1 over the n trackers, the
    record carries the integer sum of the lengths and record_row multiplies once: n products and n - 1 additions against one product,
    each rounding at most 2**-53 of a value that is at most the total, so the two differ by at most 2 n 2**-53 of the total (and
    the division by n adds one rounding to each side)."""
    got = row_numbers(row)
    n, mean = want[2], want[3]
    rest = [0, 1, 2] + list(range(4, 10))
    if not np.array_equal(got[rest], want[rest]):
        return False
    if n == 0:
        return bool(np.isnan(got[3]) and np.isnan(mean))
    return bool(abs(got[3] - mean) <= (2 * n + 2) * 2.0 ** -53 * mean)
