"""The traversability and survival-fit metrics on the device (include/d2d_metrics.h: d2d_trav_steps, d2d_fit_first_hit;
drone2d_amd.metrics) against the recorded reference (tests/golden/difficulty_tables.npz) and the Python model
(tests/difficulty_model.py).  Step counts and first hits are integers, the floats are compared on bit patterns: no tolerances."""
import numpy as np
import pytest
import torch

import difficulty_cases as DC
import difficulty_model as M
from drone2d_amd import _abi as A
from drone2d_amd import _lib, metrics, sweeps, vec_env

pytestmark = pytest.mark.gpu
G = 64          # guard elements on either side of an output buffer
PARAMS = sweeps._params(dict(agent_number=1, agent_size=10, agent_speed=40, map_id=0))     # the fit worlds' map, dt and drone_radius


def dev(a, hip, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(hip.device)


def guarded(hip, shape, dtype):
    """(whole, view): `view` of `shape` inside a buffer of 0x7f bytes with G elements of guard on either side"""
    n = int(np.prod(shape))
    raw = torch.full(((n + 2 * G) * torch.empty((), dtype=dtype).element_size(),), 0x7f, dtype=torch.uint8, device=hip.device)
    whole = raw.view(dtype)
    return whole, whole[G:G + n].view(shape)


def guards_intact(whole):
    g = torch.cat([whole[:G], whole[-G:]]).contiguous().view(torch.uint8)
    return bool((g == 0x7f).all())


def device_steps(hip, grids, starts):
    return metrics.trav_steps(dev(grids, hip, torch.uint8), starts, backend=hip).cpu().numpy()


def device_fit(hip, agents, pos, checks, drone_radius=10, params=PARAMS, want_agents=True):
    """one launch on host arrays: (first [B, P], agents_out [B, 6, N] or None) as host arrays"""
    p = sweeps._params(dict(agent_number=1, agent_size=10, agent_speed=40, map_id=0))
    p.map_size, p.drone_radius = list(params.map_size), drone_radius
    got = metrics.fit_first_hit(dev(agents, hip, torch.float64), dev(pos, hip, torch.float64), p, checks, backend=hip, return_agents=want_agents)
    hip.sync()
    return (got[0].cpu().numpy(), got[1].cpu().numpy()) if want_agents else (got.cpu().numpy(), None)


# ---- 1. d2d_trav_steps

@pytest.mark.parametrize('B', [1, 2, 3, 5])
def test_walks_on_the_recorded_grids(hip, B):
    fx = DC.fixture()[:B]
    steps = device_steps(hip, np.stack([rec['gt'] for _, rec in fx]), DC.AXIS_STARTS)
    assert steps.shape == (B, 81, 8) and steps.dtype == np.int32
    for i, (_, rec) in enumerate(fx):
        assert np.array_equal(steps[i], DC.fixture_trav_model(i)['steps'])
        values = metrics.trav_values(steps[i])
        assert DC.bits_equal(values, rec['values'])
        assert DC.bits_equal(np.float64(metrics.trav_metric(values)), rec['traversibility'])
    assert [int((steps[i, :, 0] < 0).sum()) for i in range(min(B, 3))] == [0, 1, 6][:B]


def test_walks_on_a_grid_that_is_not_square(hip):
    """7 x 5: corners and edges (walks of no step, diagonals that end at the border), cells of value 0, 1 and 3 stopping a ray"""
    want = DC.grid_model('small')
    assert np.array_equal(device_steps(hip, DC.small_grid()[None], DC.SMALL_STARTS)[0], want)
    for s, start in enumerate(DC.SMALL_STARTS):                                # every start alone: S = 1
        assert np.array_equal(device_steps(hip, DC.small_grid()[None], [start])[0, 0], want[s])


# W x H, S: one pass and more than one (8 * 33 > 256 threads); the largest grid staged in LDS (16384 cells), the first sizes above
# it and a 300 x 260 one, read from global memory
@pytest.mark.parametrize('W,H,S', [(50, 50, 1), (50, 50, 33), (128, 128, 33), (127, 129, 33), (128, 129, 33), (129, 128, 40), (300, 260, 33)])
def test_walks_on_random_grids_in_lds_and_in_global_memory(hip, W, H, S):
    want = DC.grid_model('random', W, H, S, 7)
    grid, starts = DC.GRIDS['random'](W, H, S, 7)
    assert want.max() > 3
    got = device_steps(hip, np.stack([grid, grid[::-1].copy(), grid]), starts)
    assert np.array_equal(got[0], want) and np.array_equal(got[2], want)
    assert np.array_equal(got[1], M.trav_steps(grid[::-1], starts))


@pytest.mark.parametrize('W,H', [(7, 5), (300, 260)])
def test_every_step_count_is_written_and_nothing_else(hip, W, H):
    grid, starts = (DC.small_grid(), DC.SMALL_STARTS) if W == 7 else DC.GRIDS['random'](W, H, 33, 7)
    want = M.trav_steps(grid, starts)
    gt = dev(np.stack([grid, grid]), hip, torch.uint8)
    st = dev(np.array(starts), hip, torch.int32)
    whole, steps = guarded(hip, (2, len(starts), 8), torch.int32)
    hip.trav_steps(gt, st, steps)
    hip.sync()
    first = steps.clone()
    hip.trav_steps(gt, st, steps)                                             # the same buffers again
    hip.sync()
    for got in (first, steps):
        assert np.array_equal(got[0].cpu().numpy(), want) and np.array_equal(got[1].cpu().numpy(), want)
    assert guards_intact(whole)


# ---- 2. d2d_fit_first_hit

@pytest.mark.parametrize('i', range(5))
def test_first_hits_and_final_agents_on_the_recorded_worlds(hip, i):
    index, rec = DC.fixture()[i]
    p = sweeps._params(index)
    first, end = device_fit(hip, rec['fit_agents'][None], DC.positions_of(p), DC.CHECKS, p.drone_radius, p)
    assert first.shape == (1, 64) and first.dtype == np.int32
    assert np.array_equal(first[0], DC.fixture_fit_model(i)['first'])
    times = metrics.fit_times(first[0].reshape(8, 8))
    assert DC.bits_equal(times, rec['survive_times']) and DC.bits_equal(np.mean(times), rec['fit'])
    assert DC.bits_equal(end[0], rec['fit_agents_end'])


@pytest.mark.parametrize('N', [1, 24, 64, 65, 70])
def test_agent_counts_around_the_wave(hip, N):
    """the adversarial world's first N agents: walls, the corner, the stuck-agent turn at speeds 4 and 5, the exact distance"""
    ag, m = DC.adversarial_fit_model(N)
    first, end = device_fit(hip, ag[None], DC.fit_positions(64), DC.CHECKS)
    assert np.array_equal(first[0], m['first']) and DC.bits_equal(end[0], m['agents_end'])
    if N == 1:
        assert (first == -1).all()                                            # dist == r + drone_radius exactly, and never hit
        first, _ = device_fit(hip, DC.adversarial_agents(True)[None, :, :1], DC.fit_positions(64), DC.CHECKS)
        assert first[0, 9] == 0 and (np.delete(first[0], 9) == -1).all()      # 0.001 px nearer: hit at check 0


@pytest.mark.parametrize('N', [128, 130, 192, 200, 256])
def test_agent_counts_of_two_three_and_four_tiles(hip, N):
    ag, m = DC.many_agents_model(N)
    first, end = device_fit(hip, ag[None], DC.fit_positions(64), 40)
    assert np.array_equal(first[0], m['first']) and DC.bits_equal(end[0], m['agents_end'])


@pytest.mark.parametrize('drone_radius', [0, 10])
@pytest.mark.parametrize('checks', [1, 120])
@pytest.mark.parametrize('P', [1, 64, 65])
def test_position_counts_checks_and_drone_radii(hip, P, checks, drone_radius):
    ag, m = DC.adversarial_fit_model(70, P, checks, drone_radius)
    first, end = device_fit(hip, ag[None], DC.fit_positions(P), checks, drone_radius)
    assert first.shape == (1, P) and np.array_equal(first[0], m['first']) and DC.bits_equal(end[0], m['agents_end'])
    again, none = device_fit(hip, ag[None], DC.fit_positions(P), checks, drone_radius, want_agents=False)     # agents_out = NULL
    assert none is None and np.array_equal(again, first)


@pytest.mark.parametrize('B', [1, 2, 3, 5])
def test_worlds_of_one_batch(hip, B):
    worlds = [DC.adversarial_fit_model(65, 65, roll=3 * b) for b in range(B)]
    first, end = device_fit(hip, np.stack([w[0] for w in worlds]), DC.fit_positions(65), DC.CHECKS)
    for b, (_, m) in enumerate(worlds):
        assert np.array_equal(first[b], m['first']) and DC.bits_equal(end[b], m['agents_end'])


def test_a_map_that_is_not_square(hip):
    p = sweeps._params(dict(agent_number=12, agent_size=12, agent_speed=45, map_id=4))
    p.map_size, p.target_list = [500, 300], [[50, 260]]
    w = DC.world_of(p)
    pos = DC.positions_of(p)
    assert len(pos) == 40
    m = M.fit_world(w['agents'], pos, p.drone_radius, p.map_size, p.map_scale, p.dt, DC.CHECKS)
    first, end = device_fit(hip, w['agents'][None], pos, DC.CHECKS, p.drone_radius, p)
    assert np.array_equal(first[0], m['first']) and DC.bits_equal(end[0], m['agents_end'])
    assert (m['agents_end'][1] < 300).all() and (m['first'] >= 0).any()


def test_every_first_hit_and_agent_is_written_and_nothing_else(hip):
    B, N, P = 2, 70, 65
    worlds = [DC.adversarial_fit_model(N, P, roll=5 * b) for b in range(B)]
    agents = dev(np.stack([w[0] for w in worlds]), hip, torch.float64)
    before = agents.clone()
    pos = dev(DC.fit_positions(P), hip, torch.float64)
    fw, first = guarded(hip, (B, P), torch.int32)
    ew, end = guarded(hip, (B, 6, N), torch.float64)
    for _ in range(2):                                                        # the second call on the same buffers
        hip.fit_first_hit(agents, pos, 10, 500, 500, 10, 0.1, DC.CHECKS, first, end)
        hip.sync()
        for b, (_, m) in enumerate(worlds):
            assert np.array_equal(first[b].cpu().numpy(), m['first']) and DC.bits_equal(end[b].cpu().numpy(), m['agents_end'])
    assert guards_intact(fw) and guards_intact(ew)
    assert torch.equal(agents.view(torch.int64), before.view(torch.int64))     # the input is not modified


@pytest.mark.parametrize('n,size,speed', [(10, 10, 40), (30, 5, 4)])
def test_final_agents_equal_the_step_library_s(hip, n, size, speed):
    """the existing fused step, 121 times, leaves the agents where one launch of d2d_fit_first_hit leaves them (8 worlds)"""
    p = sweeps._params(dict(agent_number=n, agent_size=size, agent_speed=speed, map_id=40))
    env = vec_env.VecDrone2DEnv(p, 8, backend=hip, planner='NoMove')
    start = env.state.t['agents'].clone()
    _, end = metrics.fit_first_hit(start, dev(DC.positions_of(p), hip, torch.float64), p, DC.CHECKS, backend=hip, return_agents=True)
    env.rollout(torch.zeros((DC.CHECKS + 1, 8), dtype=torch.float64, device=hip.device))
    env.sync()
    assert not torch.equal(start, env.state.t['agents'])
    assert torch.equal(end.view(torch.int64), env.state.t['agents'].view(torch.int64))


def test_sizes_are_checked_before_the_launch(hip):
    one = torch.ones((1, 2), dtype=torch.float64, device=hip.device)
    p = one.data_ptr()                                                        # (never read: the sizes are refused first)
    for args, rc in ((('fit_first_hit', p, p, 10.0, 500.0, 500.0, 10.0, 0.1, 1, A.FIT_MAX_N + 1, 1, 1, p, None), -4),
                     (('fit_first_hit', p, p, 10.0, 500.0, 500.0, 10.0, 0.1, 1, 1, A.FIT_MAX_P + 1, 1, p, None), -4),
                     (('fit_first_hit', p, p, 10.0, 500.0, 500.0, 10.0, 0.1, 1 << 20, 1, 1 << 12, 1, p, None), -4),
                     (('fit_first_hit', p, p, 10.0, 500.0, 500.0, 10.0, 0.1, 1, 0, 1, 1, p, None), -1),
                     (('fit_first_hit', p, p, 10.0, 500.0, 500.0, 10.0, 0.1, 1, 1, 1, -1, p, None), -1),
                     (('fit_first_hit', p, None, 10.0, 500.0, 500.0, 10.0, 0.1, 1, 1, 1, 1, p, None), -1),
                     (('trav_steps', p, 1, 1 << 16, 1 << 16, p, 1, p), -4), (('trav_steps', p, 1 << 20, 5, 5, p, 1 << 10, p), -4),
                     (('trav_steps', p, 1, 0, 5, p, 1, p), -1), (('trav_steps', p, 1, 5, 5, p, 0, p), -1)):
        with pytest.raises(_lib.D2DError, match=f'error {rc}:'):
            hip._metrics(*args)
    # no check at all: one update, every position -1
    first, end = device_fit(hip, DC.adversarial_agents()[None], DC.fit_positions(64), 0)
    assert (first == -1).all() and DC.bits_equal(end[0], M.agents_update(DC.adversarial_agents(), 500, 500, 10, 0.1))
    hip.sync()


# ---- 3. end to end

@pytest.mark.parametrize('worlds', [None, 'device'])
def test_tables_equal_the_recorded_means(hip, worlds):
    for index, rec in DC.fixture():
        args = ([index['map_id']], (index['agent_number'],), (index['agent_size'],), (index['agent_speed'],))
        t = metrics.traversibility_table(*args, backend=hip, worlds=worlds)
        assert len(t) == 1 and len(t[0]) == 1 and DC.bits_equal(np.float64(t[0][0]), rec['traversibility'])
        f = metrics.survival_fit_table(*args, backend=hip, worlds=worlds)
        assert len(f) == 1 and len(f[0]) == 1 and DC.bits_equal(np.float64(f[0][0]), rec['fit'])


def test_a_table_of_several_agent_counts_in_the_reference_s_order(hip):
    fx = DC.fixture()
    maps, ns, sizes, speeds = [0, 1], (10, 20), (5, 10), (20, 40)
    order = sweeps._table_order(maps, ns, sizes, speeds)
    host = metrics.traversibility_table(maps, ns, sizes, speeds, backend=hip)
    devw = metrics.traversibility_table(maps, ns, sizes, speeds, backend=hip, worlds='device')
    assert host == devw and len(host) == 2 and len(host[0]) == 8
    assert host[0][order.index(fx[0][0])] == float(fx[0][1]['traversibility'])
    assert host[1][order.index(fx[1][0]) - 8] == float(fx[1][1]['traversibility'])
    host = metrics.survival_fit_table(maps, ns, sizes, speeds, backend=hip)
    devw = metrics.survival_fit_table(maps, ns, sizes, speeds, backend=hip, worlds='device')
    assert host == devw
    assert host[0][order.index(fx[0][0])] == float(fx[0][1]['fit']) and host[1][order.index(fx[1][0]) - 8] == float(fx[1][1]['fit'])
