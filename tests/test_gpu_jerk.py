"""The kernels of libd2d_jerk.so (include/d2d_jerk.h) against the Python model (tests/jerk_model.py), bit for bit (run with -m gpu):
d2d_jerk_plan alone on the synthetic batches of tests/jerk_cases.py -- 257 envs (a count no launch shape divides), grids 50 x 50
row-major and 37 x 45 tiled (not a multiple of the tile), N in {0, 3, 70} (70: more than a wave of trackers), v_max in {7, 20, 40,
72} (S = 51, 18, 9 and the 0.5 s clamp's 5) -- then d2d_jerk_reset with a mask, and three batches sized so that trk_radius, wp and
dmap of the last env end on the last byte of their device allocation."""
import math

import numpy as np
import pytest
import torch

from drone2d_amd import _abi as A
import jerk_cases as JC
import jerk_model as M

pytestmark = pytest.mark.gpu
PAGE = 2 << 20


def upload(arr, dev):
    return {k: (None if v is None else torch.from_numpy(v).to(dev)) for k, v in arr.items()}


def plan_on_device(hip, b, t):
    call = JC.call_of(b, lambda x: x.data_ptr(), t)
    hip.jerk_plan(call)
    hip.sync()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in t.items()}


def check(got, want, b):
    assert not want['unknown'].any()                                   # the model alone says: no tie pattern outside the table
    assert np.array_equal(got['plan_ok'], want['plan_ok']) and np.array_equal(got['wp_valid'], want['plan_ok'])
    assert np.array_equal(got['choice'], want['choice'])
    assert M.bits_equal(got['wp'], want['wp'])
    assert np.array_equal(got['stat'] & A.JERK_STAT_TIE != 0, want['tie'])
    assert not (got['stat'] & A.JERK_STAT_UNKNOWN).any()
    assert np.array_equal(got['stat'] >> A.JERK_STAT_SHIFT, want['tested'])
    if b['N']:
        assert M.bits_equal(got['trk_radius'], b['radius_after']) and np.array_equal(got['trk_prev'], b['prev_after'])


@pytest.mark.parametrize('B,N,v_max,W,H,tile', JC.BATCHES, ids=lambda v: str(v))
def test_plan_equals_the_model_on_synthetic_batches(hip, B, N, v_max, W, H, tile):
    b, want = JC.batch(B, N, v_max, W, H, tile), JC.answers(B, N, v_max, W, H, tile)
    got = plan_on_device(hip, b, upload(JC.host_arrays(b), hip.device))
    check(got, want, b)
    kinds = np.array(b['kinds'])
    assert (want['plan_ok'][kinds == 'blocked'] == 0).all() and want['plan_ok'][kinds == 'open'].any()
    assert want['tie'][kinds == 'wall'].any() and want['tie'][kinds == 'on_pf'].any()
    if N >= 3:
        assert want['tie'][kinds == 'axis'].any()
        assert (b['radius_after'] != b['radius0']).any()              # archived trackers: the radius went back to agent_radius


def test_var_cam_enters_the_tracker_limit(hip):
    b, want = JC.batch(257, 3, 20, 50, 50, 0, seed=1), JC.answers(257, 3, 20, 50, 50, 0, seed=1)
    check(plan_on_device(hip, b, upload(JC.host_arrays(b), hip.device)), want, b)


def test_a_second_step_sees_the_archived_radius_and_reset_restores_the_masked_envs(hip):
    B, N = 257, 3
    b = JC.batch(B, N, 20, 50, 50, 0)
    t = upload(JC.host_arrays(b), hip.device)
    plan_on_device(hip, b, t)
    # step 2: every tracker active again -- the archived ones now with agent_radius in their limit
    b2 = dict(b, active=np.ones((B, N), np.uint8), radius0=b['radius_after'], prev=b['prev_after'])
    b2['radius_after'], b2['prev_after'] = b['radius_after'].copy(), np.ones((B, N), np.uint8)
    t['active'].fill_(1)
    got = plan_on_device(hip, b2, t)
    for e in range(0, B, 5):
        r = M.plan(JC.scene_of(b2, e))
        assert got['choice'][e] == r['choice'] and M.bits_equal(got['wp'][e], r['wp']), e
    assert M.bits_equal(got['trk_radius'], b['radius_after']) and got['trk_prev'].all()
    mask = torch.zeros((B, 2), dtype=torch.uint8, device=hip.device)
    mask[::3, 0] = 1
    mask[:, 1] = 1                                                     # the stride's other column is not looked at
    r0 = torch.from_numpy(b['radius0']).to(hip.device)
    hip.jerk_reset(t['trk_radius'], t['trk_prev'], r0, mask, 2)
    hip.sync()
    on = mask[:, 0].bool().cpu().numpy()
    rad, prev = t['trk_radius'].cpu().numpy(), t['trk_prev'].cpu().numpy()
    assert M.bits_equal(rad[on], b['radius0'][on]) and M.bits_equal(rad[~on], b['radius_after'][~on])
    assert not prev[on].any() and prev[~on].all()
    hip.jerk_reset(t['trk_radius'], t['trk_prev'], r0)
    hip.sync()
    assert M.bits_equal(t['trk_radius'].cpu().numpy(), b['radius0']) and not t['trk_prev'].any()


def test_sizes_the_library_cannot_take_are_refused(hip):
    from drone2d_amd import _lib
    D2DError = _lib.D2DError
    b = JC.batch(257, 0, 40, 50, 50, 0)
    t = upload(JC.host_arrays(b), hip.device)
    call = JC.call_of(b, lambda x: x.data_ptr(), t)
    call.S = A.JERK_MAX_S + 1
    with pytest.raises(D2DError, match='-4'):
        hip.jerk_plan(call)
    call.S, call.tie_perm = 9, None
    with pytest.raises(D2DError, match='table pointer is NULL'):
        hip.jerk_plan(call)
    call = JC.call_of(b, lambda x: x.data_ptr(), t)
    call.N = A.JERK_MAX_N + 1
    with pytest.raises(D2DError, match='-4'):
        hip.jerk_plan(call)


def _ends_its_allocation(t):
    end = t.data_ptr() + t.numel() * t.element_size()
    for seg in torch.cuda.memory_snapshot():
        if seg['address'] <= t.data_ptr() < seg['address'] + seg['total_size']:
            return end == seg['address'] + seg['total_size']
    return False


@pytest.mark.parametrize('buf,N,v_max,W,H,tile', [('trk_radius', 64, 40, 50, 50, 0), ('wp', 3, 40, 37, 45, 16), ('dmap', 3, 7, 37, 45, 16)])
def test_buffer_ending_on_a_page_boundary(hip, buf, N, v_max, W, H, tile):
    """as tests/test_gpu_guard_pages.py: the batch is a whole number of copies of 64 synthetic envs, sized so that `buf` is a whole
    number of 2 MiB pages and an allocation of its own -- a read or write past the last env's record faults instead of landing in a
    neighbour -- and every copy must equal the 64-env run"""
    b = JC.batch(64, N, v_max, W, H, tile)
    arr = JC.host_arrays(b)
    small = upload(arr, hip.device)
    got = plan_on_device(hip, b, small)
    check(got, JC.answers(64, N, v_max, W, H, tile), b)
    per_env = arr[buf].nbytes // 64
    b0 = PAGE // math.gcd(per_env, PAGE)
    b0 = b0 * 64 // math.gcd(b0, 64)
    B = b0 * max(1, -(-(24 << 20) // (per_env * b0)))
    reps = B // 64
    per_env_fields = ('drone', 'target', 'active', 'kf', 'dmap', 'trk_radius', 'trk_prev', 'plan_ok', 'wp_valid', 'wp', 'choice', 'stat')
    big = {k: v for k, v in upload(arr, hip.device).items()}
    for k in per_env_fields:
        if big[k] is not None:
            big[k] = big[k].repeat((reps,) + (1,) * (big[k].dim() - 1))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    plugs = []
    for _ in range(32):
        tb = torch.empty_like(big[buf])
        if _ends_its_allocation(tb):
            break
        plugs.append(tb)
    tb.copy_(big[buf])
    big[buf] = tb
    assert tb.numel() * tb.element_size() == per_env * B and (per_env * B) % PAGE == 0
    assert _ends_its_allocation(tb), f'{buf}: the allocator placed the buffer inside a larger segment'
    bb = dict(b, B=B)
    hip.jerk_plan(JC.call_of(bb, lambda x: x.data_ptr(), big))
    hip.sync()
    for k in ('plan_ok', 'wp_valid', 'choice', 'stat', 'trk_radius', 'trk_prev'):
        want = torch.from_numpy(got[k]).to(hip.device)
        assert bool((big[k].view(reps, *want.shape) == want.unsqueeze(0)).all()), k
    want = torch.from_numpy(got['wp']).to(hip.device).view(torch.int64)
    assert bool((big['wp'].view(torch.int64).view(reps, 64, 6) == want.unsqueeze(0)).all())
    del big, plugs
    torch.cuda.empty_cache()
