"""The velocity-obstacle feasibility metric on the device (include/d2d_metrics.h, drone2d_amd.metrics) against the recorded
reference (tests/golden/vo_feasibility.npz) and the Python model (tests/vo_model.py).  Counts and intermediates are compared with
torch.equal or on bit patterns: there are no tolerances."""
import functools

import numpy as np
import pytest
import torch

import vo_cases
import vo_model
from drone2d_amd import metrics, vec_env

pytestmark = pytest.mark.gpu


def bits(t):
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t, np.float64))
    return t.detach().cpu().contiguous().view(torch.int64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and torch.equal(a, b)


def assert_parts(count, parts, want, b):
    """world b of a vo_counts(return_parts=True) result against the model's dict"""
    assert torch.equal(count[b].cpu(), torch.from_numpy(want['count'])), 'count'
    assert torch.equal(parts['collided'][b].cpu(), torch.from_numpy(want['collided'])), 'collided'
    for k in ('arg', 'theta_ba', 'half', 'cone'):
        assert same_bits(parts[k][b], want[k]), k


def dev(a, hip, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(hip.device)


# ---- 1. the recorded reference

@pytest.mark.parametrize('worlds', [None, 'device'])
@pytest.mark.parametrize('i', range(3))
def test_rates_and_mean_equal_the_recorded_reference(hip, i, worlds):
    index, rec = vo_cases.fixture()[i]
    rates = metrics.vo_feasibility_batch([index], backend=hip, worlds=worlds)
    assert rates.shape == (1, 256) and rates.dtype == np.float64
    assert same_bits(rates[0], rec['rates'])
    got = metrics.vo_feasibility(index, backend=hip, worlds=worlds)
    assert same_bits(np.float64(got), rec['mean'])


@pytest.mark.parametrize('i', range(3))
def test_three_worlds_in_one_batch(hip, i):
    index, rec = vo_cases.fixture()[i]
    batch = [dict(index, map_id=index['map_id'] + k) for k in range(3)]
    host = metrics.vo_feasibility_batch(batch, backend=hip)
    devw = metrics.vo_feasibility_batch(batch, backend=hip, worlds='device')
    given = metrics.vo_feasibility_batch(batch, backend=hip, worlds=[vo_cases.world_of(metrics._params(ix)) for ix in batch])
    assert host.shape == (3, 256) and same_bits(host, devw) and same_bits(host, given)
    assert same_bits(host[0], rec['rates'])
    for k in (1, 2):
        assert same_bits(host[k], metrics.vo_feasibility_batch([batch[k]], backend=hip)[0])
    assert not same_bits(host[1], host[0]) and not same_bits(host[2], host[1])


# ---- 2. the model on small shapes, every intermediate

SMALL = {
    'one_agent': dict(agent_number=1),
    'n33': dict(agent_number=33, agent_radius=8),                                     # more agents than one tile of the count kernel
    'obstacle_map_n24': dict(agent_number=10, static_map='maps/obstacle_map.npy'),    # + 14 radius-5 agents on cells
    'map_500x300': dict(agent_number=8, map_size=[500, 300], target_list=[[50, 260]]),
}


def small_params(name, map_id):
    return vo_cases.vo_params(map_id=map_id, **SMALL[name])


@functools.lru_cache(maxsize=None)
def small_model(name, map_id):
    p = small_params(name, map_id)
    w = vo_cases.world_of(p)
    return w['agents'], vo_model.vo_world(w['agents'], vo_cases.positions_of(p, 120), vo_cases.candidates())


@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('name', list(SMALL))
def test_small_shapes_equal_the_model(hip, name, B):
    ids = [3 + 2 * k for k in range(B)]
    plist = [small_params(name, m) for m in ids]
    pos = vo_cases.positions_of(plist[0], 120)
    if name == 'map_500x300':
        assert len(pos) == 12
    if name == 'obstacle_map_n24':
        assert small_model(name, ids[0])[0].shape[1] == 24
    agents = vec_env.build_worlds_device_of(plist, backend=hip).state.t['agents']
    assert same_bits(agents, np.stack([small_model(name, m)[0] for m in ids]))
    count, parts = metrics.vo_counts(agents, dev(pos, hip), dev(vo_cases.candidates(), hip), backend=hip, return_parts=True)
    assert count.shape == (B, len(pos)) and count.dtype == torch.int32
    for b, m in enumerate(ids):
        assert_parts(count, parts, small_model(name, m)[1], b)


# ---- 3. the adversarial world

def test_adversarial_world_equals_the_model(hip):
    want = vo_cases.adversarial_model()
    count, parts = metrics.vo_counts(dev(vo_cases.adversarial()[None], hip), dev(vo_cases.ADV_POS, hip), dev(vo_cases.candidates(), hip),
                                     backend=hip, return_parts=True)
    assert_parts(count, parts, want, 0)
    assert count[0].tolist()[2] == -1 and want['arg'][1, 0] == 1.0 and want['theta_ba'][1, 1] == np.pi


# ---- 4. every output entry is written, nothing beside them

def test_every_entry_is_written_and_nothing_else(hip):
    ag = vo_cases.adversarial()
    agents = dev(np.stack([ag, np.roll(ag, 7, axis=1)]), hip)                 # B = 2, N = 70
    pos, cand = dev(vo_cases.ADV_POS, hip), dev(vo_cases.candidates(), hip)
    clean_count, clean = metrics.vo_counts(agents, pos, cand, backend=hip, return_parts=True)
    assert_parts(clean_count, clean, vo_cases.adversarial_model(), 0)
    B, P, N, G = 2, 3, 70, 64

    def guarded(shape, dtype):
        n = int(np.prod(shape))
        raw = torch.full(((n + 2 * G) * torch.empty((), dtype=dtype).element_size(),), 0x7f, dtype=torch.uint8, device=hip.device)
        whole = raw.view(dtype)
        return whole, whole[G:G + n].view(shape)
    arg_w, arg = guarded((B, P, N), torch.float64)
    tba_w, tba = guarded((B, P, N), torch.float64)
    col_w, col = guarded((B, P), torch.uint8)
    cone_w, cone = guarded((B, P, N, 2), torch.float64)
    cnt_w, cnt = guarded((B, P), torch.int32)
    hip.vo_geometry(agents, pos, 5.0, arg, tba, col)
    hip.vo_cones(tba, clean['half'], col, cone)
    hip.vo_count(agents, cand, cone, col, cnt)
    hip.sync()
    first = cnt.clone()
    hip.vo_count(agents, cand, cone, col, cnt)                                # the same buffers again: nothing accumulates
    hip.sync()
    assert torch.equal(first, clean_count) and torch.equal(cnt, clean_count)
    assert torch.equal(col, clean['collided'])
    assert same_bits(arg, clean['arg']) and same_bits(tba, clean['theta_ba']) and same_bits(cone, clean['cone'])
    for whole in (arg_w, tba_w, col_w, cone_w, cnt_w):
        g = torch.cat([whole[:G], whole[-G:]]).contiguous().view(torch.uint8)
        assert bool((g == 0x7f).all())


# ---- 5. the candidate set's edges

@functools.lru_cache(maxsize=None)
def custom_candidates(C):
    rng = np.random.RandomState(100 + C)
    return np.round(rng.uniform(-60, 60, (C, 2)), 1)


@pytest.mark.parametrize('C', [1, 64, 65, 630])
def test_candidate_counts_that_are_no_multiple_of_the_wave(hip, C):
    index, rec = vo_cases.fixture()[1]
    ag = vo_cases.fixture_agents(rec)
    pos = vo_cases.positions_of(metrics._params(index), 120)
    cand = custom_candidates(C)
    want = vo_model.vo_world(ag, pos, cand)
    count, parts = metrics.vo_counts(dev(ag[None], hip), dev(pos, hip), dev(cand, hip), backend=hip, return_parts=True)
    assert_parts(count, parts, want, 0)
    assert int(count.max()) <= C and int((count >= 0).sum()) > 0


# ---- sizes the launch cannot take are refused before anything is launched

def test_sizes_are_checked_before_the_launch(hip):
    from drone2d_amd import _abi as A
    from drone2d_amd import _lib
    one = torch.ones((1, 2), dtype=torch.float64, device=hip.device)
    assert metrics.vo_counts(torch.ones((1, 6, 1), dtype=torch.float64, device=hip.device), 50 * one, one, backend=hip).tolist() == [[1]]
    p = one.data_ptr()                                                        # (never read: the sizes are refused first)
    for args, rc in ((('vo_count', p, p, p, p, 1, 1, A.VO_MAX_P + 1, 630, p), -4), (('vo_count', p, p, p, p, A.VO_MAX_B + 1, 1, 1, 1, p), -4),
                     (('vo_geometry', p, p, 5.0, 32768, 1024, 1024, p, p, p), -4), (('vo_cones', p, p, p, 0, 1, 1, p), -1),
                     (('vo_count', p, p, p, p, 1, 1, 1, 0, p), -1)):
        with pytest.raises(_lib.D2DError, match=f'error {rc}:'):
            hip._metrics(*args)
    hip.sync()
