"""The measurement noise drawn on the device (var_cam != 0, d2d_state.rng; run with -m gpu): the log and the stream on their own,
every launch path against the oracle driven with numpy's draws, and the batched entry points that used to refuse var_cam != 0."""
import numpy as np
import pytest
import torch

import closed_loop_cases as CL
import noise_cases as NC
from rng_host import RNG_NREGEN, RNG_NPAIR, RNG_POS, assert_state_is, needs_fma, needs_glibc_235, numpy_pairs, numpy_stream

pytestmark = [pytest.mark.gpu, needs_glibc_235, needs_fma]     # numpy's draws go through this host's libm log


def _stream_of(seed):
    s = np.zeros(640, dtype=np.uint32)
    rs = np.random.RandomState(seed)
    rs.rand(100)
    _, s[:624], s[RNG_POS], _, _ = rs.get_state()
    return s


def test_rng_draw_equals_numpy(hip):
    """d2d_rng_draw: 5 streams, 12 calls with every stream's m from 0, 1, 63, 64, 65, 172 -- pairs and whole states bit-equal to
    numpy's; a stream regenerates its key three times and more, and attempts are rejected (fewer pairs than attempts used)"""
    B, sizes = 5, (0, 1, 63, 64, 65, 172)
    state = np.stack([_stream_of(s) for s in (0, 5, 77, 4242, 2 ** 31 - 1)])
    ref = [numpy_stream(s) for s in state]
    rng = torch.from_numpy(state.view(np.int32).copy()).to(hip.device)
    pick = np.random.RandomState(1)
    plan = [pick.permutation(sizes)[:B] for _ in range(12)]
    plan[3] = np.array([172, 172, 0, 65, 64])                  # (whatever the permutations gave: 172 twice in a row for stream 0)
    plan[4] = np.array([172, 1, 63, 0, 172])
    words0 = state[:, RNG_POS].astype(np.int64)
    total = np.zeros(B, dtype=np.int64)
    for i, m in enumerate(plan):
        out = torch.full((B, 172, 2), 7.0, dtype=torch.float64, device=hip.device)
        hip.rng_draw(rng, torch.from_numpy(m.astype(np.int32)).to(hip.device), out)
        hip.sync()
        got, now = out.cpu().numpy(), rng.cpu().numpy().view(np.uint32)
        for b in range(B):
            want = numpy_pairs(ref[b], int(m[b]))
            assert got[b, :m[b]].tobytes() == want.tobytes(), (i, b, int(m[b]))
            assert not got[b, m[b]:].any(), (i, b)             # the rest of the row is cleared
            assert_state_is(now[b], ref[b], (i, b))
        total += m
        assert np.array_equal(now[:, RNG_NPAIR], total)
    now = rng.cpu().numpy().view(np.uint32)
    assert int(now[:, RNG_NREGEN].max()) >= 3, now[:, RNG_NREGEN]
    words = now[:, RNG_NREGEN].astype(np.int64) * 624 + now[:, RNG_POS] - words0
    assert (words % 4 == 0).all() and (words // 4 > total).all(), (words // 4, total)      # every stream had attempts rejected


def test_rng_draw_refuses_positions_it_cannot_draw_from(hip):
    """a position above 624 or no multiple of 4 (state.check_rng refuses them on the host): NaN draws, the stream untouched"""
    state = np.stack([_stream_of(3)] * 3)
    state[1, RNG_POS], state[2, RNG_POS] = 202, 628
    rng = torch.from_numpy(state.view(np.int32).copy()).to(hip.device)
    out = torch.zeros((3, 4, 2), dtype=torch.float64, device=hip.device)
    hip.rng_draw(rng, torch.tensor([2, 2, 2], dtype=torch.int32, device=hip.device), out)
    got = out.cpu().numpy()
    assert np.isfinite(got[0, :2]).all() and np.isnan(got[1:, :2]).all() and not got[:, 2:].any()
    assert np.array_equal(rng.cpu().numpy().view(np.uint32)[1:], state[1:])


def _dev_step(dev, c, n, actions, t):
    from drone2d_amd import _abi
    if c['kind'] == 'closed':
        dev.closed_loop(n, **NC.mode_of(c))
    elif c['kind'] == 'rollout':
        dev.rollout(actions[t:t + n])
    elif c['kind'] == 'step':
        dev.step(actions[t])
    else:                                                      # the raycast in one launch, the trackers (and their draws) in the next
        dev._set_action(actions[t])
        dev.backend.run_stages(dev.cfg, dev._st, _abi.ST_FSM | _abi.ST_AGENTS | _abi.ST_RAYCAST)
        dev.backend.run_stages(dev.cfg, dev._st, _abi.ST_DYNGRID | _abi.ST_TRACKER)
        dev.backend.run_stages(dev.cfg, dev._st, _abi.ST_ACT)


@pytest.mark.parametrize('case', NC.CASES, ids=NC.case_id)
def test_launch_path_draws_what_numpy_draws(pkg, hip, oracle, case):
    from drone2d_amd import vec_env
    c, name = case, case['name']
    worlds = vec_env.build_worlds(NC.params_of(pkg, c), c['B'])
    dev = NC.make_env(pkg, hip, c, worlds, device_side=True)
    assert dev.device_noise and dev.state.noise is None
    if c['path'] is not None:
        assert CL.closed_loop_path(dev.cfg, dev._plan) == c['path'], name
    assert not CL.default_geometry(dev.cfg) and (dev.cfg.grid_tile != 0) == (c['layout'] == 'tiled')
    ref = NC.OracleWithHostDraws(pkg, oracle, c, worlds)
    actions = np.random.RandomState(c['kw']['map_id']).uniform(-1, 1, (c['T'], c['B']))
    oracle.lib.d2d_oracle_set_threads(8)
    regen = 0
    try:
        t = 0
        for n in CL.chunk_sizes(c):
            _dev_step(dev, c, n, actions, t)
            for i in range(n):
                ref.step(actions[t + i])
            t += n
            NC.assert_same_state(dev, ref.env, f'{name} after step {t}', plugins=c['kind'] == 'closed',
                                 skip=('action',) if c['kind'] == 'rollout' else ())      # (d2d_rollout reads its own [T][B] actions)
            regen = max(regen, ref.check_stream(dev, f'{name} after step {t}'))
    finally:
        oracle.lib.d2d_oracle_set_threads(1)
    # the row ran what it is there for
    assert regen >= 1, f'{name}: no stream crossed a regeneration of its key'
    assert ref.seen['none'] and ref.seen['many'], f'{name}: steps with no agent in view / with two and more: {ref.seen}'
    if c['on_done'] != 'continue':
        assert ref.seen['done'], f'{name}: no episode ended'
    if c['on_done'] == 'reset':
        # the device equals the oracle side after every call, in the first episode as in the second; and the second episode of an
        # env is its first over again: the stream was put back with the world
        full = [ep for ep in ref.episodes if len(ep) >= 3]
        assert full, f'{name}: no env finished two episodes'
        for ep in full:
            assert ep[1] == ep[0] and len(ep[0]) > 10, name


def test_closed_loop_runs_without_set_noise(pkg, hip, oracle):
    """VecDrone2DEnv(Params(var_cam=2, ...), 4, planner='Primitive', device_plugins=True, gaze='Oxford').closed_loop(50) with no
    set_noise(): refused before there was a device stream ("var_cam != 0 needs the noise input"); it runs, and it is the oracle's
    run with numpy's draws"""
    from drone2d_amd import vec_env
    c = dict(name='no-set-noise', path='k_closed<0>', kind='closed', on_done='continue', B=4, layout='rowmajor', planner='Primitive',
             gaze='Oxford', kw=dict(var_cam=2, agent_number=10, agent_radius=15, agent_max_speed=20, map_id=1))
    p = NC.params_of(pkg, c)
    env = vec_env.VecDrone2DEnv(p, 4, backend=hip, planner='Primitive', device_plugins=True, gaze='Oxford')
    assert CL.closed_loop_path(env.cfg, env._plan) == c['path']
    env.closed_loop(50)
    env.sync()
    ref = NC.OracleWithHostDraws(pkg, oracle, c, vec_env.build_worlds(p, 4))
    for _ in range(50):
        ref.step()
    NC.assert_same_state(env, ref.env, 'closed_loop(50)', plugins=True)
    ref.check_stream(env, 'closed_loop(50)')
    assert int(ref.pairs.sum()) > 0
